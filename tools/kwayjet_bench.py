#!/usr/bin/env python3
"""Cost and effect of ek_kway_jet: the headline workload
(bench.py's: the largest component of Hypergraph.generate(1.15, 1)) and ibm01,
under unit weights and under §12's synthetic weights (node 1 + id mod 5, net 1 +
e mod 3), everything at imbalance 0.03 and the default options.

    python tools/kwayjet_bench.py [--out profiles/kwayjet/kwayjet_headline.json]

One box, one warm context.  Three blocks:
  * k = 4, 8, 16 from two starts, ek_partition_kway_ml's and ek_partition_kway's
    output: 1 warm-up and --runs timed runs of the device pass (medians), the
    host checker once, and ek_kway_refine_w from the same start in the same
    process (the yardstick for quality and for microseconds a round);
  * k = 2 from the median + KL best-prefix start, beside ek_fm_refine_w at its
    default stall, same process: final weighted cut and total ms of both;
  * neg_num / neg_den = 0, 1/4 and 3/4 on the headline's k = 8 multilevel start.
The part vector, the iteration log and the result integers are identical in
every run and on both paths (asserted)."""
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

TIMES = ("t_setup", "t_iters", "t_metrics")
FIXED = ("iters", "best_iter", "moves", "total_weight", "bound_min", "bound_max", "part_w_min", "part_w_max",
         "parts_over_bound", "connectivity_w_before", "cut_nets", "connectivity", "connectivity_w", "soed")


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def jet_row(ek, ctx, h, start, k, eps, a, neg=(1, 4), host=True):
    """The device pass timed, the host checker once, both identical."""
    rows = []
    for i in range(1 + a.runs):
        t = time.perf_counter()
        part, r, log = ctx.kway_jet(h, start, k, eps, neg=neg)
        r["wall"] = time.perf_counter() - t
        r["total"] = sum(r[x] for x in TIMES)
        if i >= 1:
            rows.append(r)
    first = rows[0]
    assert all(all(r[f] == first[f] for f in FIXED) for r in rows), "runs differ"
    row = {**{f: first[f] for f in FIXED}, "neg": list(neg), "iter_log": log.tolist(),
           "device_ms": {x: med(rows, x) for x in TIMES + ("total", "wall")}}
    row["device_us_per_iter"] = 1e3 * row["device_ms"]["t_iters"]["median"] / max(first["iters"], 1)
    if host:
        hpart, hr, hlog = ek.kway_jet_host(h, start, k, eps, neg=neg)
        assert np.array_equal(part, hpart) and np.array_equal(log, hlog), "device and host differ"
        assert all(hr[f] == first[f] for f in FIXED), "device and host differ"
        row["host_ms"] = {x: 1e3 * hr[x] for x in TIMES}
        row["host_ms"]["total"] = sum(row["host_ms"].values())
    return part, row


def refine_w_row(ctx, h, start, k, eps, a):
    rows = []
    for i in range(1 + a.runs):
        _, r, _ = ctx.kway_refine_w(h, start, k, eps)
        r["total"] = sum(r[x] for x in ("t_setup", "t_rounds", "t_metrics"))
        if i >= 1:
            rows.append(r)
    r = rows[0]
    return {"rounds": r["rounds"], "moves": r["moves"], "connectivity_w": r["connectivity_w"],
            "part_w_max": r["part_w_max"], "parts_over_bound": r["parts_over_bound"],
            "ms": {x: med(rows, x) for x in ("t_setup", "t_rounds", "t_metrics", "total")},
            "us_per_round": 1e3 * 1e3 * statistics.median(x["t_rounds"] for x in rows) / (r["rounds"] + 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kwayjet", "kwayjet_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    ctx = ek.Context(0)
    eps = a.imbalance
    out = {"imbalance": eps, "warmup": 1, "runs": a.runs, "kway": [], "bipartition": [], "neg_sweep": []}
    try:
        for wl in a.workloads:
            if wl == "headline":
                base, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
            else:
                base = ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", f"{wl}.hgr"))
            nets, nodes, pins = base.dims()
            net_ptr, pin_ids = base.pins()
            # the median + KL best-prefix sides (structure only)
            ctx.spmv_setup_pins(base)
            ctx.lanczos_fiedler()
            ctx.kl_graph_setup(base.kl_graph())
            ctx.kl_nets_setup(net_ptr, pin_ids)
            ctx.kl_set_partition_fiedler()
            ctx.kl_run()
            kl_side = np.ascontiguousarray(ctx.kl_sides(1), np.uint8)
            for weights in ("ones", "synthetic"):
                h = ek.Hypergraph.from_pins(nodes, net_ptr, pin_ids)
                if weights == "synthetic":
                    h.set_weights((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))
                tag = {"workload": wl, "nodes": nodes, "nets": nets, "pins": pins, "weights": weights}
                # k = 2 against the serial FM pass
                fms = []
                for i in range(1 + a.runs):
                    t = time.perf_counter()
                    _, _, _, fr = ctx.fm_refine_w(h, kl_side, eps)
                    fr["wall"] = time.perf_counter() - t
                    if i >= 1:
                        fms.append(fr)
                _, jrow = jet_row(ek, ctx, h, kl_side.astype(np.int32), 2, eps, a)
                fm = {"cut": fms[0]["cut"], "moves_kept": fms[0]["moves_kept"], "w0": fms[0]["w0"], "w1": fms[0]["w1"],
                      "max_part": fms[0]["max_part"], "wall_ms": med(fms, "wall")}
                out["bipartition"].append({**tag, "k": 2, "start": "median+KL", "jet": jrow, "fm_refine_w": fm})
                print(f"{wl}/{weights} k 2 (median + KL): weighted cut {jrow['connectivity_w_before']} -> jet "
                      f"{jrow['connectivity_w']} in {jrow['device_ms']['total']['median']:.2f} ms ({jrow['iters']} "
                      f"iterations, best {jrow['best_iter']}), fm {fm['cut']} in {fm['wall_ms']['median']:.1f} ms",
                      flush=True)
                for k in a.ks:
                    t = time.perf_counter()
                    ml, _ = ctx.partition_kway_ml(h, k, eps)
                    t_ml = time.perf_counter() - t
                    flat, _ = ctx.partition_kway(h, k)
                    for name, start in (("partition_kway_ml", ml), ("partition_kway", flat)):
                        _, row = jet_row(ek, ctx, h, start, k, eps, a)
                        row.update(tag, k=k, start=name, kway_refine_w=refine_w_row(ctx, h, start, k, eps, a))
                        if name == "partition_kway_ml":
                            row["partition_ms"] = 1e3 * t_ml
                        out["kway"].append(row)
                        d, rw = row["device_ms"], row["kway_refine_w"]
                        print(f"{wl}/{weights} k {k} from {name}: connectivity_w {row['connectivity_w_before']} -> jet "
                              f"{row['connectivity_w']} ({row['iters']} iterations, best {row['best_iter']}, "
                              f"{row['moves']} moves, weights ..{row['part_w_max']} of {row['bound_max']}, over "
                              f"{row['parts_over_bound']}); device {d['total']['median']:.2f} ms (setup "
                              f"{d['t_setup']['median']:.2f}, iterations {d['t_iters']['median']:.2f} = "
                              f"{row['device_us_per_iter']:.0f} us each, metrics {d['t_metrics']['median']:.2f}), host "
                              f"{row['host_ms']['total']:.0f} ms; refine_w -> {rw['connectivity_w']} in "
                              f"{rw['ms']['total']['median']:.2f} ms, {rw['us_per_round']:.0f} us a round", flush=True)
                    if wl == "headline" and k == 8:
                        for neg in ((0, 1), (1, 4), (3, 4)):
                            _, row = jet_row(ek, ctx, h, ml, k, eps, a, neg=neg, host=False)
                            row.update(tag, k=k, start="partition_kway_ml")
                            out["neg_sweep"].append(row)
                            print(f"{wl}/{weights} k 8 neg {neg[0]}/{neg[1]}: {row['connectivity_w_before']} -> "
                                  f"{row['connectivity_w']}, {row['iters']} iterations (best {row['best_iter']}), "
                                  f"{row['moves']} moves, {row['device_ms']['total']['median']:.2f} ms", flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
