#!/usr/bin/env python3
"""Matching against multi-node clustering as the coarsening of ek_partition_kway_direct: the headline
workload (bench.py's: the largest component of Hypergraph.generate(1.15, 1)) and ibm01, under unit weights and under
§12's synthetic weights (node 1 + id mod 5, net 1 + e mod 3), k = 4, 8, 16, imbalance 0.03, the default options,
nothing tuned.

    python tools/kwayd_cluster_bench.py [--out profiles/cluster/cluster_headline.json]

One box, one warm context, both coarsenings in the same process.  Two blocks per (workload, weights, k):
  * the driver: 1 warm-up and --runs timed runs under EK_COARSEN_MATCH and under EK_COARSEN_CLUSTER (medians; the
    runs of one coarsening give the same integers, asserted): the levels and their nodes, the rounds, the times, the
    final weighted connectivity, parts_over_bound;
  * the hierarchy the driver builds under the clustering, level by level (the driver's max_cluster, its 10 % rule):
    ek_cluster, uploads and downloads included, against ek_cluster_host (the same outputs, asserted) and against
    ek_match on the same level, 1 warm-up and --runs timed runs each; the heaviest cluster of every level."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

TIMES = ("t_match", "t_contract", "t_initial", "t_jet", "t_metrics", "t_total")
FIXED = ("levels", "total_weight", "part_bound", "max_cluster", "part_w_min", "part_w_max", "parts_over_bound",
         "empty_parts", "cut_nets", "connectivity", "connectivity_w", "soed", "initial_fallbacks", "infeasible_sweeps")


def spread(xs):
    return {"median": 1e3 * statistics.median(xs), "min": 1e3 * min(xs), "max": 1e3 * max(xs)}


def timed(fn, runs):
    out, ts = None, []
    for i in range(1 + runs):
        t = time.perf_counter()
        out = fn()
        if i >= 1:
            ts.append(time.perf_counter() - t)
    return out, ts


def direct_row(ctx, h, k, eps, coarsening, runs):
    rows = []
    for i in range(1 + runs):
        _, r = ctx.partition_kway_direct(h, k, eps, coarsening=coarsening)
        if i >= 1:
            rows.append(r)
    first = rows[0]
    assert all(all(r[f] == first[f] for f in FIXED) and r["nodes"] == first["nodes"] for r in rows), "runs differ"
    row = {f: first[f] for f in FIXED}
    row.update(nodes=first["nodes"], coarsest_nodes=first["nodes"][-1], rounds=first["match_rounds"][:-1],
               joins=first["match_pairs"][:-1], conn_w_before=first["conn_w_before"],
               conn_w_after=first["conn_w_after"], jet_iters=first["jet_iters"], jet_moves=first["jet_moves"],
               ms={t: spread([r[t] for r in rows]) for t in TIMES})
    return row


def level_rows(ek, ctx, h, max_cluster, coarse, runs):
    """Every level of the hierarchy the driver builds under the clustering."""
    out, cur = [], h
    while cur.nodes > coarse and len(out) < ek.ML_LEVELS:
        dev, t_dev = timed(lambda: ctx.cluster(cur, max_cluster), runs)
        host, t_host = timed(lambda: ek.cluster_host(cur, max_cluster), runs)
        mat, t_mat = timed(lambda: ctx.match(cur, max_cluster), runs)
        assert all(np.array_equal(x, y) for x, y in zip(dev[:3], host[:3])), "device and host differ"
        assert all(dev[3][f] == host[3][f] for f in ("n_coarse", "joins", "rounds", "eligible_nets", "heaviest"))
        res = dev[3]
        nets, nodes, pins = cur.dims()
        out.append({"level": len(out), "nodes": nodes, "nets": nets, "pins": pins, "cluster_n_coarse": res["n_coarse"],
                    "cluster_rounds": res["rounds"], "heaviest": res["heaviest"], "round_log": dev[2].tolist(),
                    "match_n_coarse": mat[3]["n_coarse"], "match_rounds": mat[3]["rounds"],
                    "cluster_device_ms": spread(t_dev), "cluster_host_ms": spread(t_host), "match_device_ms": spread(t_mat)})
        if 10 * res["n_coarse"] > 9 * cur.nodes:
            out[-1]["kept"] = False  # the driver's 10 % rule: the level is not taken
            break
        out[-1]["kept"] = True
        cur = ctx.hgr_contract(cur, dev[1], res["n_coarse"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cluster", "cluster_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    ctx = ek.Context(0)
    eps = a.imbalance
    out = {"imbalance": eps, "warmup": 1, "runs": a.runs, "kway": [], "levels": []}
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
                    row = {**tag, "k": k}
                    for coarsening in ("match", "cluster"):
                        row[coarsening] = r = direct_row(ctx, h, k, eps, coarsening, a.runs)
                        d = r["ms"]
                        print(f"{wl}/{weights} k {k} {coarsening}: nodes {r['nodes']}, rounds {r['rounds']}, "
                              f"connectivity_w {r['connectivity_w']} (initial {r['conn_w_before'][-1]}), heaviest part "
                              f"{r['part_w_max']} of {r['part_bound']}, over {r['parts_over_bound']}; "
                              f"{d['t_total']['median']:.1f} ms (coarsen {d['t_match']['median']:.1f}, contract "
                              f"{d['t_contract']['median']:.1f}, initial {d['t_initial']['median']:.1f}, jet "
                              f"{d['t_jet']['median']:.1f}, metrics {d['t_metrics']['median']:.1f})", flush=True)
                    out["kway"].append(row)
                    node_w, _ = h.weights()
                    W = int(node_w.sum()) if node_w is not None else nodes
                    share = -(-W // k)
                    coarse = max(512, 128 * k)
                    cap = max(1, min(-(-4 * W // coarse), max(1, int(math.floor((1.0 + eps) * share)) - share)))
                    assert cap == row["cluster"]["max_cluster"]
                    rows = level_rows(ek, ctx, h, cap, coarse, a.runs)
                    row["levels_block_is_the_drivers_hierarchy"] = \
                        [r["nodes"] for r in rows if r["kept"]] == row["cluster"]["nodes"][:-1]
                    for r in rows:
                        out["levels"].append({**tag, "k": k, "max_cluster": cap, **r})
                        print(f"{wl}/{weights} k {k} level {r['level']}: {r['nodes']} nodes -> cluster "
                              f"{r['cluster_n_coarse']} in {r['cluster_rounds']} rounds (heaviest {r['heaviest']} of {cap}"
                              f"{'' if r['kept'] else ', not kept'}), device {r['cluster_device_ms']['median']:.2f} ms, "
                              f"host {r['cluster_host_ms']['median']:.2f} ms; match {r['match_n_coarse']} in "
                              f"{r['match_rounds']} rounds, device {r['match_device_ms']['median']:.2f} ms", flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
