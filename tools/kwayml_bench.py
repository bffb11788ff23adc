#!/usr/bin/env python3
"""Quality and cost of the k-way partition by recursive multilevel bisection
(ek_partition_kway_ml) against the flat k-way path
(ek_partition_kway, and ek_partition_kway + ek_kway_refine) in one process on
one warm context: the headline workload (bench.py's: the largest component of
Hypergraph.generate(1.15, 1)) and ibm01, with all-ones weights and under the
synthetic weighting of DESIGN.md §12 (node weight 1 + (id mod 5), net weight
1 + (e mod 3)), k = 2, 4, 8, 16 at imbalance 0.03.

    python tools/kwayml_bench.py [--out profiles/kwayml/kwayml_headline.json]

Each (workload, k): the flat path and its refinement once per timed run (they
read the structure alone, so one measurement serves both weightings; their
weighted metrics are counted under each weighting by ek_kway_metrics_w_host);
each (workload, weighting, k): the multilevel path, 1 warm-up + 3 timed runs
(identical parts asserted), medians of its phase seconds."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

ML_TIMES = ("t_total", "t_induce", "t_ml", "t_match", "t_contract", "t_lanczos", "t_sweep", "t_fm", "t_metrics")
ML_INTS = ("bisections", "coarsest_fallbacks", "infeasible_sweeps", "total_weight", "part_bound", "part_w_min",
           "part_w_max", "parts_over_bound", "empty_parts", "cut_nets", "connectivity", "connectivity_w", "soed",
           "levels_total", "fm_moves")


def med(xs):
    xs = list(xs)
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def quality(ek, h, part, k):
    (cut, conn, connw, soed), pw = ek.kway_metrics_w_host(h, part, k)
    return {"cut_nets": cut, "connectivity": conn, "connectivity_w": connw, "soed": soed, "part_w_min": int(pw.min()),
            "part_w_max": int(pw.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kwayml", "kwayml_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--coarse-nodes", type=int, default=512)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    eps = a.imbalance
    hs = {}
    if "headline" in a.workloads:
        hs["headline"] = ek.Hypergraph.generate(a.mult, a.seed).largest_component()[0]
    if "ibm01" in a.workloads:
        hs["ibm01"] = ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", "ibm01.hgr"))
    ctx = ek.Context(0)
    out = {"imbalance": eps, "coarse_nodes": a.coarse_nodes, "runs": a.runs, "rows": []}
    try:
        for name, h in hs.items():
            nets, nodes, pins = h.dims()
            weights = {"ones": (np.ones(nodes, np.int32), np.ones(nets, np.int32)),
                       "synthetic": ((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))}
            for k in a.ks:
                h.set_weights(None, None)
                flat = [ctx.partition_kway(h, k) for _ in range(1 + a.runs)][1:]
                assert all(np.array_equal(p, flat[0][0]) for p, _ in flat), "flat runs differ"
                refined = [ctx.kway_refine(h, flat[0][0], k, eps) for _ in range(a.runs)]
                fpart, fres = flat[-1]
                rpart, rres, _ = refined[-1]
                assert (fres["connectivity"], rres["connectivity"]) == (
                    ek.kway_metrics_host(*h.pins(), fpart, k)[1], ek.kway_metrics_host(*h.pins(), rpart, k)[1])
                for weighting, (node_w, net_w) in weights.items():
                    h.set_weights(node_w, net_w)
                    runs = [ctx.partition_kway_ml(h, k, eps, a.coarse_nodes) for _ in range(1 + a.runs)]
                    part, res = runs[-1]
                    assert all(np.array_equal(p, part) for p, _ in runs), "multilevel runs differ"
                    q = quality(ek, h, part, k)
                    assert all(q[f] == res[f] for f in q), "the driver's metrics differ from the host's"
                    row = {"workload": name, "nodes": nodes, "nets": nets, "pins": pins, "weighting": weighting, "k": k,
                           "kway_ml": {**{f: res[f] for f in ML_INTS},
                                       "seconds": {t: med(r[t] for _, r in runs[1:]) for t in ML_TIMES}},
                           "kway_flat": {**quality(ek, h, fpart, k), "part_min": fres["part_min"],
                                         "part_max": fres["part_max"],
                                         "seconds": {t: med(r[t] for _, r in flat)
                                                     for t in ("t_total", "t_induce", "t_lanczos", "t_kl", "t_metrics")}},
                           "kway_flat_refined": {**quality(ek, h, rpart, k), "part_min": rres["part_min"],
                                                 "part_max": rres["part_max"], "rounds": rres["rounds"],
                                                 "moves": rres["moves"],
                                                 "seconds_refine": med(r["t_setup"] + r["t_rounds"] + r["t_metrics"]
                                                                       for _, r, _ in refined)}}
                    out["rows"].append(row)
                    m, f, r = row["kway_ml"], row["kway_flat"], row["kway_flat_refined"]
                    s = m["seconds"]
                    print(f"{name} / {weighting} / k={k}: ml connectivity {m['connectivity']} (weighted "
                          f"{m['connectivity_w']}), cut nets {m['cut_nets']}, part weights {m['part_w_min']}.."
                          f"{m['part_w_max']} (bound {m['part_bound']}, over {m['parts_over_bound']}), "
                          f"{1e3 * s['t_total']['median']:.1f} ms (induce {1e3 * s['t_induce']['median']:.1f}, match "
                          f"{1e3 * s['t_match']['median']:.1f}, contract {1e3 * s['t_contract']['median']:.1f}, lanczos "
                          f"{1e3 * s['t_lanczos']['median']:.1f}, sweep {1e3 * s['t_sweep']['median']:.1f}, fm "
                          f"{1e3 * s['t_fm']['median']:.1f}); flat connectivity {f['connectivity']} (weighted "
                          f"{f['connectivity_w']}), cut nets {f['cut_nets']}, part weights {f['part_w_min']}.."
                          f"{f['part_w_max']}, {1e3 * f['seconds']['t_total']['median']:.1f} ms; flat + refine "
                          f"connectivity {r['connectivity']} (weighted {r['connectivity_w']}), cut nets {r['cut_nets']}, "
                          f"part weights {r['part_w_min']}..{r['part_w_max']}, + "
                          f"{1e3 * r['seconds_refine']['median']:.1f} ms", flush=True)
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
