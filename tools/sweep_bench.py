#!/usr/bin/env python3
"""Effect and cost of the sweep cut (ek_kl_set_partition_fiedler_sweep) on the
headline workload (bench.py's: the largest component of
Hypergraph.generate(1.15, 1)) and on ibm01, for imbalance 0, 0.03 and 0.10 and
both objectives, beside the median split of the same Fiedler vector on the
same box.

    python tools/sweep_bench.py [--out profiles/sweep/sweep_headline.json]

Each workload: the Laplacian on the device, one Lanczos solve, the KL graph and
nets; then the median split + KL once, and per (imbalance, objective) the sweep
split + KL once and ek_sweep_cut on the returned vector 2 warm-ups + 7 timed
runs (its sort / profile / select times, medians) against ek_sweep_cut_host 3
times.  The order, the profile and the result integers are identical in every
run and on both paths (asserted)."""
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
INTS = ("n", "n0", "n1", "s_lo", "s_hi", "max_part", "cut", "cut_mid", "spanning_nets")


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweep", "sweep_headline.json"))
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
    out = {"imbalances": a.imbalances, "warmup": a.warmup, "runs": a.runs, "workloads": []}
    try:
        for name, h in (("headline", headline), ("ibm01", ibm01)):
            nets, nodes, pins = h.dims()
            net_ptr, pin_ids = h.pins()
            ctx.spmv_setup_pins(h)
            lam, v, st = ctx.lanczos_fiedler()
            ctx.kl_graph_setup(h.kl_graph())
            ctx.kl_nets_setup(net_ptr, pin_ids)
            _, n0, n1 = ctx.kl_set_partition_fiedler()
            _, kl = ctx.kl_run()
            wl = {"name": name, "nets": nets, "nodes": nodes, "pins": pins, "lambda1": lam,
                  "median_split": {"n0": n0, "n1": n1, "net_cut_initial": kl["net_cut_initial"],
                                   "net_cut_best": kl["net_cut_best"], "kl_iterations": kl["iterations"],
                                   "kl_loop_ms": kl["loop_ms"]},
                  "sweep": []}
            print(f"{name}: {nodes} nodes, {nets} nets; median split {n0} | {n1}: cut {kl['net_cut_initial']} -> KL "
                  f"best {kl['net_cut_best']}", flush=True)
            for eps in a.imbalances:
                for ratio in (False, True):
                    res = ctx.kl_set_partition_fiedler_sweep(h, eps, ratio)
                    _, kl = ctx.kl_run()
                    rows = []
                    for i in range(a.warmup + a.runs):
                        r, order, profile = ctx.sweep_cut(h, v, eps, ratio)
                        r["total"] = sum(r[x] for x in TIMES)
                        if i >= a.warmup:
                            rows.append(r)
                    hosts = []
                    for _ in range(3):
                        hr, horder, hprofile = ek.sweep_cut_host(h, v, eps, ratio)
                        hr["total"] = sum(hr[x] for x in TIMES)
                        hosts.append(hr)
                    assert np.array_equal(order, horder) and np.array_equal(profile, hprofile), "device and host differ"
                    assert all(all(r[f] == res[f] for f in INTS) for r in rows + hosts), "runs differ"
                    row = {"imbalance": eps, "objective": "ratio" if ratio else "min-cut", **{f: res[f] for f in INTS},
                           "kl_net_cut_initial": kl["net_cut_initial"], "kl_net_cut_best": kl["net_cut_best"],
                           "kl_iterations": kl["iterations"], "kl_loop_ms": kl["loop_ms"],
                           "device_ms": {x: med(rows, x) for x in TIMES + ("total",)},
                           "host_ms": {x: med(hosts, x) for x in TIMES + ("total",)}}
                    wl["sweep"].append(row)
                    d, hm = row["device_ms"], row["host_ms"]
                    print(f"  eps {eps} {row['objective']}: window {res['s_lo']}..{res['s_hi']}, n1 {res['n1']}, cut_mid "
                          f"{res['cut_mid']}, cut {res['cut']}, KL best {kl['net_cut_best']} ({kl['iterations']} swaps, "
                          f"{kl['loop_ms']:.1f} ms); device {d['total']['median']:.3f} ms (sort "
                          f"{d['t_sort']['median']:.3f}, profile {d['t_profile']['median']:.3f}, select "
                          f"{d['t_select']['median']:.3f}); host {hm['total']['median']:.2f} ms", flush=True)
            out["workloads"].append(wl)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
