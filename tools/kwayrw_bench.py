#!/usr/bin/env python3
"""Cost and effect of ek_kway_refine_w after ek_partition_kway_ml:
the headline workload (bench.py's: the largest component of
Hypergraph.generate(1.15, 1)) and ibm01, k = 4, 8, 16, under unit weights and
under §12's synthetic weights (node 1 + id mod 5, net 1 + e mod 3), partition
and refinement both at imbalance 0.03.

    python tools/kwayrw_bench.py [--out profiles/kwayrw/kwayrw_headline.json]

One box, one warm context.  Each row: the partition once, then 2 warm-ups and 7
timed runs of the device refinement (medians), the host checker 3 times, and
ek_kway_refine on the same start in the same process for its time a round.  The
part vector, the round log and the result integers are identical in every run
and on both paths (asserted)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

TIMES = ("t_setup", "t_rounds", "t_metrics")
FIXED = ("rounds", "moves", "gain_total", "total_weight", "bound_min", "bound_max", "part_w_min", "part_w_max",
         "parts_over_bound", "connectivity_w_before", "cut_nets", "connectivity", "connectivity_w", "soed")


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kwayrw", "kwayrw_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    ctx = ek.Context(0)
    out = {"imbalance": a.imbalance, "warmup": a.warmup, "runs": a.runs, "rows": []}
    try:
        for wl in a.workloads:
            if wl == "headline":
                base, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
            else:
                base = ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", f"{wl}.hgr"))
            nets, nodes, pins = base.dims()
            net_ptr, pin_ids = base.pins()
            for weights in ("ones", "synthetic"):
                h = ek.Hypergraph.from_pins(nodes, net_ptr, pin_ids)
                if weights == "synthetic":
                    h.set_weights((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))
                for k in a.ks:
                    t = time.perf_counter()
                    start, mres = ctx.partition_kway_ml(h, k, a.imbalance)
                    t_part = time.perf_counter() - t
                    rows = []
                    for i in range(a.warmup + a.runs):
                        t = time.perf_counter()
                        part, r, log = ctx.kway_refine_w(h, start, k, a.imbalance)
                        r["wall"] = time.perf_counter() - t
                        r["total"] = sum(r[x] for x in TIMES)
                        if i >= a.warmup:
                            rows.append(r)
                    hosts = []
                    for _ in range(3):
                        hpart, hr, hlog = ek.kway_refine_w_host(h, start, k, a.imbalance)
                        hr["total"] = sum(hr[x] for x in TIMES)
                        hosts.append(hr)
                    assert np.array_equal(part, hpart) and np.array_equal(log, hlog), "device and host differ"
                    first = rows[0]
                    assert all(all(r[f] == first[f] for f in FIXED) for r in rows + hosts), "runs differ"
                    plain = []  # ek_kway_refine on the same start: the unweighted round, for its time a round
                    for i in range(a.warmup + a.runs):
                        _, ur, _ = ctx.kway_refine(h, start, k, a.imbalance)
                        if i >= a.warmup:
                            plain.append(ur)
                    rounds_run = first["rounds"] + 1  # the round that accepts nothing runs too
                    row = {"workload": wl, "nodes": nodes, "nets": nets, "pins": pins, "weights": weights, "k": k,
                           **{f: first[f] for f in FIXED}, "round_log": log.tolist(),
                           "partition_kway_ml": {"ms": 1e3 * t_part, "connectivity_w": mres["connectivity_w"],
                                                 "part_w_min": mres["part_w_min"], "part_w_max": mres["part_w_max"],
                                                 "part_bound": mres["part_bound"]},
                           "device_ms": {x: med(rows, x) for x in TIMES + ("total", "wall")},
                           "host_ms": {x: med(hosts, x) for x in TIMES + ("total",)},
                           "kway_refine": {"rounds": plain[0]["rounds"], "moves": plain[0]["moves"],
                                           "t_rounds_ms": med(plain, "t_rounds")}}
                    row["device_us_per_round"] = 1e3 * row["device_ms"]["t_rounds"]["median"] / rounds_run
                    row["kway_refine"]["us_per_round"] = (1e3 * row["kway_refine"]["t_rounds_ms"]["median"]
                                                          / (plain[0]["rounds"] + 1))
                    out["rows"].append(row)
                    d, hm = row["device_ms"], row["host_ms"]
                    print(f"{wl}/{weights} k {k}: connectivity_w {first['connectivity_w_before']} -> "
                          f"{first['connectivity_w']}; {first['rounds']} rounds, {first['moves']} moves, part weights "
                          f"{first['part_w_min']}..{first['part_w_max']} (bound {first['bound_max']}, over "
                          f"{first['parts_over_bound']}); device {d['total']['median']:.2f} ms (setup "
                          f"{d['t_setup']['median']:.2f}, rounds {d['t_rounds']['median']:.3f} = "
                          f"{row['device_us_per_round']:.1f} us x {rounds_run}, metrics {d['t_metrics']['median']:.2f}); "
                          f"host {hm['total']['median']:.2f} ms; ek_kway_refine "
                          f"{row['kway_refine']['us_per_round']:.1f} us a round; partition {1e3 * t_part:.0f} ms",
                          flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
