#!/usr/bin/env python3
"""Quality and cost of the multilevel bipartition (ek_multilevel_bipartition)
on the headline workload (bench.py's: the largest component of
Hypergraph.generate(1.15, 1)) and on ibm01, with all-ones weights and under the
synthetic weighting of DESIGN.md §12 (node weight 1 + (id mod 5), net weight
1 + (e mod 3)), at imbalance 0.03.

    python tools/ml_bench.py [--out profiles/ml/ml_headline.json]

Each (workload, weighting):
  * the driver, 1 warm-up + 3 timed runs (identical sides asserted): its
    per-level integers and its phase seconds;
  * the same V-cycle composed here from the device entries, level by level:
    ek_match against ek_match_host (same mate, cluster and log asserted), the
    contraction, ek_fm_refine_w; its final sides are the driver's (asserted);
  * the flat paths at the same imbalance on the same context: median split +
    KL + ek_fm_refine_w, and the weighted sweep cut + ek_fm_refine_w without KL;
  * a warm ek_solve_file step on the same hypergraph (2 untimed + 3 timed)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "cut_before", "cut_after", "fm_moves")
INTS = ("levels", "coarsest_fallback", "sweep_feasible", "max_cluster", "total_weight", "max_part", "cut", "cut_nets",
        "w0", "w1", "n0", "n1")
TIMES = ("t_match", "t_contract", "t_lanczos", "t_sweep", "t_fm", "t_total")


def flat(ek, ctx, h, start, eps):
    before = ek.bipart_metrics_host(h, start)
    t = time.perf_counter()
    _, _, _, r = ctx.fm_refine_w(h, start, eps)
    return {"start_cut": int(before[0]), "cut": r["cut"], "cut_nets": r["cut_nets"], "w0": r["w0"], "w1": r["w1"],
            "within": bool(max(r["w0"], r["w1"]) <= r["max_part"]), "moves_kept": r["moves_kept"],
            "fm_ms": 1e3 * (time.perf_counter() - t)}


def composed(ek, ctx, h, eps, coarse_nodes, cap):
    """The V-cycle from the device entries, timed level by level; (side, rows)."""
    rows, levels, clusters, cur = [], [h], [], h
    while cur.nodes > coarse_nodes and len(clusters) < ek.ML_LEVELS:
        dev = [ctx.match(cur, cap) for _ in range(3)]
        host = ek.match_host(cur, cap)
        assert all(np.array_equal(x, y) for x, y in zip(dev[-1][:3], host[:3])), "device and host matching differ"
        m = dev[-1][3]
        if 10 * m["n_coarse"] > 9 * cur.nodes:
            break
        t = time.perf_counter()
        nxt = cur.contract(dev[-1][1], m["n_coarse"])
        rows.append({"level": len(clusters), "nodes": cur.nodes, "nets": cur.nets, "rounds": m["rounds"],
                     "pairs": m["pairs"], "eligible_nets": m["eligible_nets"],
                     "match_device_ms": 1e3 * statistics.median(d[3]["t_setup"] + d[3]["t_rounds"] for d in dev),
                     "match_device_rounds_ms": 1e3 * statistics.median(d[3]["t_rounds"] for d in dev),
                     "match_host_ms": 1e3 * (host[3]["t_setup"] + host[3]["t_rounds"]),
                     "match_host_rounds_ms": 1e3 * host[3]["t_rounds"],
                     "contract_ms": 1e3 * (time.perf_counter() - t)})
        clusters.append(dev[-1][1])
        levels.append(nxt)
        cur = nxt
    rows.append({"level": len(clusters), "nodes": cur.nodes, "nets": cur.nets})
    ctx.spmv_setup_pins(cur)
    _, v, st = ctx.lanczos_fiedler()
    sweep, _, _, _ = ctx.sweep_cut_w(cur, v, eps)
    side = ek.rank_split(v, sweep["n1"])
    for l in range(len(levels) - 1, -1, -1):
        if l < len(levels) - 1:
            side = side[clusters[l]]
        t = time.perf_counter()
        side, _, _, fm = ctx.fm_refine_w(levels[l], side, eps)
        rows[l].update(fm_ms=1e3 * (time.perf_counter() - t), cut_before=fm["cut_before"], cut_after=fm["cut"],
                       fm_moves=fm["moves_kept"], fm_passes=fm["passes"])
    return side, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ml", "ml_headline.json"))
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
        with tempfile.TemporaryDirectory() as tmp:
            for name, h in (("headline", headline), ("ibm01", ibm01)):
                nets, nodes, pins = h.dims()
                path = os.path.join(tmp, f"{name}.hgr")
                h.write(path)  # (unweighted: ek_solve_file reads structure only)
                solves = [ctx.solve_file(path, write_results=False)[0] for _ in range(2 + a.runs)][2:]
                net_ptr, pin_ids = h.pins()
                ctx.spmv_setup_pins(h)
                lam, v, _ = ctx.lanczos_fiedler()
                ctx.kl_graph_setup(h.kl_graph())
                ctx.kl_nets_setup(net_ptr, pin_ids)
                ctx.kl_set_partition_fiedler()
                _, kl = ctx.kl_run()
                median_kl_side = ctx.kl_sides(1)
                for weighting in ("ones", "synthetic"):
                    if weighting == "synthetic":
                        h.set_weights((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))
                    else:
                        h.set_weights(np.ones(nodes, np.int32), np.ones(nets, np.int32))
                    runs = [ctx.multilevel_bipartition(h, eps, a.coarse_nodes) for _ in range(1 + a.runs)]
                    side, res = runs[-1]
                    assert all(np.array_equal(s, side) for s, _ in runs), "runs differ"
                    cside, rows = composed(ek, ctx, h, eps, a.coarse_nodes, res["max_cluster"])
                    assert np.array_equal(cside, side), "the composed V-cycle differs from the driver"
                    sweep, _, _, _ = ctx.sweep_cut_w(h, v, eps)
                    wl = {"name": name, "weighting": weighting, "nets": nets, "nodes": nodes, "pins": pins, "lambda1": lam,
                          "multilevel": {**{k: res[k] for k in INTS + LEVEL_FIELDS},
                                         "within": bool(max(res["w0"], res["w1"]) <= res["max_part"]),
                                         "seconds": {k: {"median": statistics.median(r[k] for _, r in runs[1:]),
                                                         "min": min(r[k] for _, r in runs[1:]),
                                                         "max": max(r[k] for _, r in runs[1:])} for k in TIMES}},
                          "levels": rows,
                          "flat_median_kl_fm": {"kl_net_cut_best": kl["net_cut_best"],
                                                **flat(ek, ctx, h, median_kl_side, eps)},
                          "flat_sweepw_fm_no_kl": {"sweep_cut": sweep["cut"], "feasible": sweep["feasible"],
                                                   **flat(ek, ctx, h, ek.rank_split(v, sweep["n1"]), eps)},
                          "solve_file_warm_s": {"median": statistics.median(s["t_total"] for s in solves),
                                                "min": min(s["t_total"] for s in solves),
                                                "max": max(s["t_total"] for s in solves)}}
                    out["workloads"].append(wl)
                    m = wl["multilevel"]
                    print(f"{name} / {weighting}: {nodes} nodes; multilevel {m['levels']} levels to {m['nodes'][-1]} nodes "
                          f"(max_cluster {m['max_cluster']}), coarsest cut {m['cut_before'][-1]}, final cut {m['cut']} "
                          f"(within L_max {m['within']}), {1e3 * m['seconds']['t_total']['median']:.1f} ms (match "
                          f"{1e3 * m['seconds']['t_match']['median']:.1f}, contract "
                          f"{1e3 * m['seconds']['t_contract']['median']:.1f}, lanczos "
                          f"{1e3 * m['seconds']['t_lanczos']['median']:.1f}, sweep "
                          f"{1e3 * m['seconds']['t_sweep']['median']:.1f}, fm {1e3 * m['seconds']['t_fm']['median']:.1f}); "
                          f"flat median+KL+FM {wl['flat_median_kl_fm']['cut']}, flat sweepw+FM "
                          f"{wl['flat_sweepw_fm_no_kl']['cut']}; warm solve_file "
                          f"{1e3 * wl['solve_file_warm_s']['median']:.1f} ms", flush=True)
                    for r in rows:
                        print("   ", {k: (round(x, 3) if isinstance(x, float) else x) for k, x in r.items()}, flush=True)
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
