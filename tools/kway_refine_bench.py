#!/usr/bin/env python3
"""Cost and effect of ek_kway_refine on the headline workload (bench.py's: the
largest component of Hypergraph.generate(1.15, 1)) for k = 4, 8, 16 at
imbalance 0.03, from the output of ek_partition_kway, beside two yardsticks
from the same run: ek_kway_refine_host (single-threaded, the checker) and the
ek_partition_kway time of the same k.

    python tools/kway_refine_bench.py [--out profiles/kway_refine/refine_headline.json]

Each k: 2 warm-ups and 7 timed runs of the device refinement (medians); the
host refinement 3 times; the partition 1 warm-up and 3 runs.  The part vector,
rounds and metrics are identical in every run and on both paths (asserted)."""
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


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kway_refine", "refine_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    ek = _load_package()
    h, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
    nets, nodes, pins = h.dims()
    net_ptr, pin_ids = h.pins()
    ctx = ek.Context(0)
    out = {"workload": {"mult": a.mult, "seed": a.seed, "nets": nets, "nodes": nodes, "pins": pins},
           "imbalance": a.imbalance, "warmup": a.warmup, "runs": a.runs, "refine": []}
    try:
        for k in a.ks:
            parts = []
            for i in range(4):
                t = time.perf_counter()
                start, pres = ctx.partition_kway(h, k)
                if i:
                    parts.append(time.perf_counter() - t)
            before = ek.kway_metrics_host(net_ptr, pin_ids, start, k)
            rows = []
            for i in range(a.warmup + a.runs):
                t = time.perf_counter()
                part, r, log = ctx.kway_refine(h, start, k, a.imbalance)
                r["wall"] = time.perf_counter() - t
                r["total"] = sum(r[x] for x in TIMES)
                if i >= a.warmup:
                    rows.append(r)
            hosts = []
            for _ in range(3):
                hpart, hr, hlog = ek.kway_refine_host(h, start, k, a.imbalance)
                hr["total"] = sum(hr[x] for x in TIMES)
                hosts.append(hr)
            assert np.array_equal(part, hpart) and np.array_equal(log, hlog), "device and host differ"
            first = rows[0]
            fixed = ("rounds", "moves", "gain_total", "max_part", "part_min", "part_max", "connectivity_before",
                     "cut_nets", "connectivity", "soed")
            assert all(all(r[f] == first[f] for f in fixed) for r in rows + hosts), "runs differ"
            rounds_run = first["rounds"] + 1  # the round that accepts nothing runs too
            row = {"k": k, **{f: first[f] for f in fixed},
                   "before": dict(zip(("cut_nets", "connectivity", "soed"), before)),
                   "part_sizes": np.bincount(part, minlength=k).tolist(),
                   "round_log": log.tolist(),
                   "device_ms": {x: med(rows, x) for x in TIMES + ("total", "wall")},
                   "host_ms": {x: med(hosts, x) for x in TIMES + ("total",)},
                   "partition_kway_ms": {"median": 1e3 * statistics.median(parts), "min": 1e3 * min(parts),
                                         "max": 1e3 * max(parts)}}
            row["device_us_per_round"] = 1e3 * row["device_ms"]["t_rounds"]["median"] / rounds_run
            row["host_over_device_rounds"] = row["host_ms"]["t_rounds"]["median"] / row["device_ms"]["t_rounds"]["median"]
            row["host_over_device_total"] = row["host_ms"]["total"]["median"] / row["device_ms"]["total"]["median"]
            row["device_total_over_partition"] = row["device_ms"]["total"]["median"] / row["partition_kway_ms"]["median"]
            out["refine"].append(row)
            d, hm = row["device_ms"], row["host_ms"]
            print(f"k {k}: connectivity {before[1]} -> {first['connectivity']}, cut nets {before[0]} -> "
                  f"{first['cut_nets']}, SOED {before[2]} -> {first['soed']}; {first['rounds']} rounds, "
                  f"{first['moves']} moves, parts {first['part_min']}..{first['part_max']} (max {first['max_part']}); "
                  f"device {d['total']['median']:.2f} ms (setup {d['t_setup']['median']:.2f}, rounds "
                  f"{d['t_rounds']['median']:.3f} = {row['device_us_per_round']:.1f} us x {rounds_run}, metrics "
                  f"{d['t_metrics']['median']:.2f}); host {hm['total']['median']:.2f} ms (rounds "
                  f"{hm['t_rounds']['median']:.2f}); partition {row['partition_kway_ms']['median']:.1f} ms", flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
