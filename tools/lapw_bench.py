#!/usr/bin/env python3
"""Quality and cost of the net-weighted Laplacian (ek_spmv_setup_pins_w,
EK_ML_WEIGHTED_LAPLACIAN) on the headline workload (bench.py's:
the largest component of Hypergraph.generate(1.15, 1)) and on ibm01, with
all-ones weights and under the synthetic weighting of DESIGN.md §12, at
imbalance 0.03.  One process, one warm context, medians of `runs` after a
warm-up.

    python tools/lapw_bench.py [--out profiles/lapw/lapw_headline.json]

Each (workload, weighting):
  * the multilevel driver without and with the flag (identical sides over the
    runs asserted): the coarsest cut, the final cut, the phase seconds;
  * the coarsest level H_L (the driver's: device matching = host matching),
    where the driver builds the Laplacian: ek_spmv_setup_pins against
    ek_spmv_setup_pins_w, whether the matrix stays coded, its distinct values,
    and the Lanczos solve's time and matvecs on either operator;
  * the same two set-ups on the input hypergraph itself."""
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

TIMES = ("t_match", "t_contract", "t_lanczos", "t_sweep", "t_fm", "t_total")


def med(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def setup_and_solve(ek, ctx, g, weighted, runs):
    """Set-up ms, format, and the Lanczos solve on the operator, warm."""
    ts, ls, st, lam = [], [], None, None
    for i in range(1 + runs):
        t = time.perf_counter()
        on_device = ctx.spmv_setup_pins(g, weighted=weighted)
        t1 = time.perf_counter()
        try:
            lam, _, st = ctx.lanczos_fiedler()
        except ek.EKError as e:  # (EK_ENOCONV: the driver then takes its fallback)
            lam, st = float("nan"), {"matvecs": -1, "converged": False, "error": str(e)}
        t2 = time.perf_counter()
        if i:
            ts.append(1e3 * (t1 - t))
            ls.append(1e3 * (t2 - t1))
    L = g.laplacian(weighted=weighted)
    return {"setup_ms": med(ts), "on_device": bool(on_device), "coded": bool(ctx.spmv_format()[0]),
            "stored_bytes": int(ctx.spmv_format()[1]), "distinct_values": int(len(np.unique(L.val.view(np.uint64)))),
            "nnz": int(len(L.val)), "lanczos_ms": med(ls), "matvecs": int(st["matvecs"]), "converged": bool(st["converged"]),
            "lambda": float(lam)}


def coarsest(ek, ctx, h, coarse_nodes, cap):
    cur, levels = h, 0
    while cur.nodes > coarse_nodes and levels < ek.ML_LEVELS:
        _, cluster, _, m = ctx.match(cur, cap)
        if 10 * m["n_coarse"] > 9 * cur.nodes:
            break
        cur = cur.contract(cluster, m["n_coarse"])
        levels += 1
    return cur, levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lapw", "lapw_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--coarse-nodes", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    ek = _load_package()
    headline, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
    ibm01 = ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", "ibm01.hgr"))
    eps = a.imbalance
    ctx = ek.Context(0)
    out = {"imbalance": eps, "coarse_nodes": a.coarse_nodes, "runs": a.runs, "workloads": []}
    try:
        for name, h in (("headline", headline), ("ibm01", ibm01)):
            nets, nodes, pins = h.dims()
            for weighting in ("ones", "synthetic"):
                if weighting == "synthetic":
                    h.set_weights((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))
                else:
                    h.set_weights(np.ones(nodes, np.int32), np.ones(nets, np.int32))
                wl = {"name": name, "weighting": weighting, "nets": nets, "nodes": nodes, "pins": pins}
                for key, flag in (("driver", False), ("driver_wlap", True)):
                    runs = [ctx.multilevel_bipartition(h, eps, a.coarse_nodes, weighted_laplacian=flag)
                            for _ in range(1 + a.runs)]
                    side, res = runs[-1]
                    assert all(np.array_equal(s, side) for s, _ in runs), "runs differ"
                    wl[key] = {"levels": res["levels"], "coarsest_nodes": res["nodes"][-1],
                               "coarsest_fallback": res["coarsest_fallback"], "sweep_feasible": res["sweep_feasible"],
                               "coarsest_cut": res["cut_before"][-1], "coarsest_cut_after_fm": res["cut_after"][-1],
                               "cut": res["cut"], "cut_nets": res["cut_nets"], "w0": res["w0"], "w1": res["w1"],
                               "within": bool(max(res["w0"], res["w1"]) <= res["max_part"]),
                               "max_cluster": res["max_cluster"],
                               "seconds": {k: med(r[k] for _, r in runs[1:]) for k in TIMES}}
                g, levels = coarsest(ek, ctx, h, a.coarse_nodes, wl["driver"]["max_cluster"])
                assert levels == wl["driver"]["levels"] and g.nodes == wl["driver"]["coarsest_nodes"]
                gw = g.weights()[1]
                wl["coarsest_level"] = {"nodes": g.nodes, "nets": g.nets,
                                        "net_w_max": int(gw.max()), "net_w_distinct": int(len(np.unique(gw))),
                                        "unweighted": setup_and_solve(ek, ctx, g, False, a.runs),
                                        "weighted": setup_and_solve(ek, ctx, g, True, a.runs)}
                wl["input_level"] = {"unweighted": setup_and_solve(ek, ctx, h, False, a.runs),
                                     "weighted": setup_and_solve(ek, ctx, h, True, a.runs)}
                out["workloads"].append(wl)
                d, w = wl["driver"], wl["driver_wlap"]
                print(f"{name} / {weighting}: {nodes} nodes -> {d['coarsest_nodes']} in {d['levels']} levels; coarsest cut "
                      f"{d['coarsest_cut']} -> {w['coarsest_cut']} with the flag, final {d['cut']} -> {w['cut']} "
                      f"(within {d['within']} / {w['within']}); driver {1e3 * d['seconds']['t_total']['median']:.1f} -> "
                      f"{1e3 * w['seconds']['t_total']['median']:.1f} ms (lanczos phase "
                      f"{1e3 * d['seconds']['t_lanczos']['median']:.1f} -> {1e3 * w['seconds']['t_lanczos']['median']:.1f})",
                      flush=True)
                for lvl in ("coarsest_level", "input_level"):
                    for k in ("unweighted", "weighted"):
                        s = wl[lvl][k]
                        print(f"    {lvl} {k}: setup {s['setup_ms']['median']:.3f} ms, coded {s['coded']}, distinct "
                              f"{s['distinct_values']} of {s['nnz']}, lanczos {s['lanczos_ms']['median']:.2f} ms, "
                              f"{s['matvecs']} matvecs, converged {s['converged']}", flush=True)
            h.set_weights(None, None)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
