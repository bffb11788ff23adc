#!/usr/bin/env python3
"""Effect and cost of the weighted sweep cut (ek_sweep_cut_w,
ek_kl_set_partition_fiedler_sweep_w) on the headline workload (bench.py's: the
largest component of Hypergraph.generate(1.15, 1)) and on ibm01, under the
synthetic weighting of DESIGN.md §12 (node weight 1 + (id mod 5), net weight
1 + (e mod 3)) and under explicit all-ones weights, for imbalance 0, 0.03 and
0.10.

    python tools/sweepw_bench.py [--out profiles/sweepw/sweepw_headline.json]

Each (workload, weighting): the Laplacian on the device, one Lanczos solve, the
KL graph and nets.  Per imbalance: ek_sweep_cut_w on the returned vector 2
warm-ups + 7 timed runs (its sort / profile / select times, medians) against
ek_sweep_cut_w_host 3 times, and on the all-ones rows ek_sweep_cut in the same
process the same way; then ek_fm_refine_w (imbalance 0.03, default stall) from
four starts: the median split + KL, the count sweep + KL, the weighted sweep +
KL, and the weighted sweep alone; for each the weighted cut before and after
and whether the sides end within L_max.  The order, the profiles and the result
integers are identical in every run and on both paths (asserted)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

TIMES = ("t_sort", "t_profile", "t_select")
INTS = ("n", "n0", "n1", "s_lo", "s_hi", "feasible", "total_weight", "max_part", "w0", "w1", "cut", "cut_nets",
        "cut_half", "spanning_nets")
FM_EPS = 0.03


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def timed(call, warmup, runs):
    rows = []
    for i in range(warmup + runs):
        out = call()
        out[0]["total"] = sum(out[0][x] for x in TIMES)
        if i >= warmup:
            rows.append(out[0])
    return rows, out


def refine(ek, ctx, h, start):
    """ek_fm_refine_w from start: the weighted cut before and after, the sides' weights, within L_max or not."""
    before = ek.bipart_metrics_host(h, start)
    _, _, _, r = ctx.fm_refine_w(h, start, FM_EPS)
    return {"start_cut": int(before[0]), "start_w0": int(before[2]), "start_w1": int(before[3]),
            "start_within": bool(max(before[2], before[3]) <= r["max_part"]), "cut": r["cut"], "cut_nets": r["cut_nets"],
            "w0": r["w0"], "w1": r["w1"], "max_part": r["max_part"], "within": bool(max(r["w0"], r["w1"]) <= r["max_part"]),
            "passes": r["passes"], "moves_kept": r["moves_kept"], "fm_ms": 1e3 * (r["t_setup"] + r["t_passes"] + r["t_metrics"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweepw", "sweepw_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--imbalances", type=float, nargs="+", default=[0.0, 0.03, 0.10])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    ek = _load_package()
    headline, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
    ibm01 = ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", "ibm01.hgr"))
    ctx = ek.Context(0)
    out = {"imbalances": a.imbalances, "fm_imbalance": FM_EPS, "warmup": a.warmup, "runs": a.runs, "workloads": []}
    try:
        for name, h in (("headline", headline), ("ibm01", ibm01)):
            nets, nodes, pins = h.dims()
            net_ptr, pin_ids = h.pins()
            ctx.spmv_setup_pins(h)
            lam, v, st = ctx.lanczos_fiedler()
            ctx.kl_graph_setup(h.kl_graph())
            ctx.kl_nets_setup(net_ptr, pin_ids)
            for weighting in ("synthetic", "ones"):
                if weighting == "synthetic":
                    h.set_weights((1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32))
                else:
                    h.set_weights(np.ones(nodes, np.int32), np.ones(nets, np.int32))
                ctx.kl_set_partition_fiedler()
                _, kl = ctx.kl_run()
                median_kl = refine(ek, ctx, h, ctx.kl_sides(1))
                wl = {"name": name, "weighting": weighting, "nets": nets, "nodes": nodes, "pins": pins, "lambda1": lam,
                      "median_split_kl": {"kl_net_cut_best": kl["net_cut_best"], **median_kl}, "sweep": []}
                print(f"{name} / {weighting}: {nodes} nodes, {nets} nets; median split + KL + fmw: weighted cut "
                      f"{median_kl['start_cut']} -> {median_kl['cut']}, within L_max {median_kl['within']}", flush=True)
                for eps in a.imbalances:
                    rows, (res, order, profw, prefix) = timed(lambda: ctx.sweep_cut_w(h, v, eps), a.warmup, a.runs)
                    hosts, (hres, horder, hprofw, hprefix) = timed(lambda: ek.sweep_cut_w_host(h, v, eps), 0, 3)
                    assert np.array_equal(order, horder) and np.array_equal(profw, hprofw) and \
                        np.array_equal(prefix, hprefix), "device and host differ"
                    assert all(all(r[f] == res[f] for f in INTS) for r in rows + hosts), "runs differ"
                    row = {"imbalance": eps, **{f: res[f] for f in INTS},
                           "device_ms": {x: med(rows, x) for x in TIMES + ("total",)},
                           "host_ms": {x: med(hosts, x) for x in TIMES + ("total",)}}
                    if weighting == "ones":  # the unweighted entry, same process, same vector
                        urows, (ures, uorder, uprofile) = timed(lambda: ctx.sweep_cut(h, v, eps), a.warmup, a.runs)
                        assert np.array_equal(uorder, order) and np.array_equal(uprofile, profw) and \
                            (ures["n1"], ures["cut"], ures["s_lo"], ures["s_hi"]) == \
                            (res["n1"], res["cut"], res["s_lo"], res["s_hi"]), "all ones: not the unweighted sweep"
                        row["unweighted_device_ms"] = {x: med(urows, x) for x in TIMES + ("total",)}
                    # the four starts of ek_fm_refine_w (the first is median_split_kl above)
                    cs = ctx.kl_set_partition_fiedler_sweep(h, eps)
                    _, kl = ctx.kl_run()
                    row["count_sweep_kl"] = {"n1": cs["n1"], "kl_net_cut_best": kl["net_cut_best"],
                                             **refine(ek, ctx, h, ctx.kl_sides(1))}
                    ws = ctx.kl_set_partition_fiedler_sweep_w(h, eps)
                    assert all(ws[f] == res[f] for f in INTS), "context path differs"
                    _, kl = ctx.kl_run()
                    row["weighted_sweep_kl"] = {"kl_net_cut_best": kl["net_cut_best"], **refine(ek, ctx, h, ctx.kl_sides(1))}
                    row["weighted_sweep_alone"] = refine(ek, ctx, h, ek.rank_split(v, res["n1"]))
                    wl["sweep"].append(row)
                    d, hm = row["device_ms"], row["host_ms"]
                    print(f"  eps {eps}: window {res['s_lo']}..{res['s_hi']} (feasible {res['feasible']}), n1 {res['n1']}, "
                          f"w0 {res['w0']} | w1 {res['w1']}, cut_half {res['cut_half']} -> cut {res['cut']} "
                          f"({res['cut_nets']} nets); device {d['total']['median']:.3f} ms (sort "
                          f"{d['t_sort']['median']:.3f}, profile {d['t_profile']['median']:.3f}, select "
                          f"{d['t_select']['median']:.3f}); host {hm['total']['median']:.2f} ms"
                          + (f"; ek_sweep_cut {row['unweighted_device_ms']['total']['median']:.3f} ms"
                             if weighting == "ones" else ""), flush=True)
                    for start in ("count_sweep_kl", "weighted_sweep_kl", "weighted_sweep_alone"):
                        s = row[start]
                        print(f"    {start}: {s['start_cut']} (within {s['start_within']}) -> fmw {s['cut']}, "
                              f"w0 {s['w0']} | w1 {s['w1']} (L_max {s['max_part']}, within {s['within']})", flush=True)
                out["workloads"].append(wl)
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
