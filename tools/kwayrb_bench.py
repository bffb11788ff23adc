#!/usr/bin/env python3
"""Cost and effect of ek_kway_rebalance: the headline workload
(bench.py's: the largest component of Hypergraph.generate(1.15, 1)) and ibm01,
under unit weights and under §12's synthetic weights (node 1 + id mod 5, net 1 +
e mod 3), k = 4, 8, 16, the default options.

    python tools/kwayrb_bench.py [--out profiles/rebalance/rebalance_headline.json]

One box, one warm context, 1 warm-up and --runs timed runs (medians).  Starts:
  * ek_partition_kway_ml's output at imbalance 0.03, rebalanced to 0.01 and to 0;
  * the same output with a tenth of part 0's nodes handed to part 1, rebalanced
    to 0.03.
Per start: rounds, moves, the excess and the weighted connectivity before and
after, the weighted connectivity after a following ek_kway_jet, the device's
milliseconds a round beside the host checker's and beside an ek_kway_refine_w
round and an ek_kway_jet iteration from the same start in the same process.
Then the direct driver with and without the rebalancing step: time and final
weighted connectivity.  The part vector, the round log and the result integers
are identical in every run and on both paths (asserted)."""
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
FIXED = ("rounds", "moves", "total_weight", "bound_max", "parts_over_before", "parts_over_bound", "excess_before",
         "excess", "connectivity_w_before", "connectivity_w", "part_w_min", "part_w_max")


def med(rows, key):
    return 1e3 * statistics.median(r[key] for r in rows)


def rebalance_row(ek, ctx, h, start, k, eps, a):
    rows = []
    for i in range(1 + a.runs):
        part, r, log = ctx.kway_rebalance(h, start, k, eps)
        if i >= 1:
            rows.append(r)
    first = rows[0]
    assert all(all(r[f] == first[f] for f in FIXED) for r in rows), "runs differ"
    hpart, hr, hlog = ek.kway_rebalance_host(h, start, k, eps)
    assert np.array_equal(part, hpart) and np.array_equal(log, hlog), "device and host differ"
    assert all(hr[f] == first[f] for f in FIXED), "device and host differ"
    row = {**{f: first[f] for f in FIXED}, "to": eps, "round_log": log.tolist(),
           "device_ms": {x: med(rows, x) for x in TIMES}, "host_ms": {x: 1e3 * hr[x] for x in TIMES}}
    n = max(first["rounds"], 1)
    row["device_us_per_round"] = 1e3 * row["device_ms"]["t_rounds"] / n
    row["host_us_per_round"] = 1e3 * row["host_ms"]["t_rounds"] / n
    # the yardsticks from the same start: a §17 round, a §18 iteration; and Jet after the rebalancer
    ws, js = [], []
    for i in range(1 + a.runs):
        _, wr, _ = ctx.kway_refine_w(h, start, k, eps)
        _, jr, _ = ctx.kway_jet(h, part, k, eps)
        if i >= 1:
            ws.append(wr)
            js.append(jr)
    row["refine_w_us_per_round"] = 1e3 * med(ws, "t_rounds") / max(ws[0]["rounds"], 1)
    row["jet_us_per_iter"] = 1e3 * med(js, "t_iters") / max(js[0]["iters"], 1)
    row["jet_after"] = {"connectivity_w": js[0]["connectivity_w"], "iters": js[0]["iters"],
                        "parts_over_bound": js[0]["parts_over_bound"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rebalance", "rebalance_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    ctx = ek.Context(0)
    out = {"warmup": 1, "runs": a.runs, "rebalance": [], "direct": []}
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
                tag = {"workload": wl, "nodes": nodes, "nets": nets, "pins": pins, "weights": weights}
                for k in a.ks:
                    ml, _ = ctx.partition_kway_ml(h, k, 0.03)
                    shifted = ml.copy()
                    mine = np.flatnonzero(ml == 0)
                    shifted[mine[:max(1, len(mine) // 10)]] = 1
                    for name, start, eps in (("partition_kway_ml@0.03", ml, 0.01), ("partition_kway_ml@0.03", ml, 0.0),
                                             ("a tenth of part 0 in part 1", shifted, 0.03)):
                        row = rebalance_row(ek, ctx, h, start, k, eps, a)
                        row.update(tag, k=k, start=name)
                        out["rebalance"].append(row)
                        print(f"{wl}/{weights} k {k} {name} -> {eps}: {row['rounds']} rounds, {row['moves']} moves, excess "
                              f"{row['excess_before']} -> {row['excess']}, over {row['parts_over_before']} -> "
                              f"{row['parts_over_bound']}, connectivity_w {row['connectivity_w_before']} -> "
                              f"{row['connectivity_w']} -> jet {row['jet_after']['connectivity_w']}; "
                              f"{row['device_us_per_round']:.0f} us a round (host {row['host_us_per_round']:.0f}, refine_w "
                              f"{row['refine_w_us_per_round']:.0f}, jet {row['jet_us_per_iter']:.0f})", flush=True)
                    for co in ("match", "cluster"):
                        d = {}
                        for rb in (False, True):
                            ts = []
                            for i in range(1 + a.runs):
                                t = time.perf_counter()
                                _, r = ctx.partition_kway_direct(h, k, 0.03, coarsening=co, rebalance=rb)
                                if i >= 1:
                                    ts.append(time.perf_counter() - t)
                            d["rebalance" if rb else "plain"] = {
                                "ms": 1e3 * statistics.median(ts), "connectivity_w": r["connectivity_w"],
                                "parts_over_bound": r["parts_over_bound"], "over_before": r.get("over_before"),
                                "rb_rounds": r.get("rb_rounds"), "excess_after": r.get("excess_after")}
                        out["direct"].append({**tag, "k": k, "coarsening": co, **d})
                        print(f"{wl}/{weights} k {k} direct/{co}: plain {d['plain']['connectivity_w']} in "
                              f"{d['plain']['ms']:.0f} ms (over {d['plain']['parts_over_bound']}), --rebalance "
                              f"{d['rebalance']['connectivity_w']} in {d['rebalance']['ms']:.0f} ms (over "
                              f"{d['rebalance']['parts_over_bound']}, levels over {d['rebalance']['over_before']})",
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
