#!/usr/bin/env python3
"""Cost and effect of the weighted FM refinement (ek_fm_refine_w) beside the
unweighted one (ek_fm_refine), on the headline workload (bench.py's: the
largest component of Hypergraph.generate(1.15, 1)) and on ibm01.

    python tools/fmw_bench.py [--out profiles/fmw/fmw_headline.json]

Each workload: the Laplacian on the device, one Lanczos solve, the KL graph and
nets, the median split and the KL loop; every run starts from the sides of KL's
best prefix, at imbalance 0.03.  Two weightings: "synthetic" (node weight 1 +
(id mod 5), net weight 1 + (e mod 3)) and "ones" (explicit all-ones arrays,
under which the weighted rule is the unweighted one: asserted).  Per weighting
and stall, on a warm context, --warmup warm-ups + --runs timed rounds; a round
is one ek_fm_refine_w and then one ek_fm_refine of the same sides, so the two
alternate.  Medians of the set-up / passes / metrics times and microseconds
per move tried for both, and the single-threaded ek_fm_refine_w_host on the
same input.  Device and host give the same sides, logs and result integers in
every run (asserted)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

TIMES = ("t_setup", "t_passes", "t_metrics")
INTS = ("n", "total_weight", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut",
        "cut_nets_before", "cut_nets", "w0", "w1", "n0", "n1")
SHARED = ("n", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut", "n0", "n1")


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def summary(rows, tried):
    out = {x: med(rows, x) for x in TIMES + ("total",)}
    out["us_per_move"] = 1e3 * out["t_passes"]["median"] / max(tried, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fmw", "fmw_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--stalls", type=int, nargs="+", default=[1000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"], choices=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    load = {"headline": lambda: ek.Hypergraph.generate(a.mult, a.seed).largest_component()[0],
            "ibm01": lambda: ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", "ibm01.hgr"))}
    ctx = ek.Context(0)
    out = {"workloads": []}
    try:
        for name in a.workloads:
            h = load[name]()
            nets, nodes, pins = h.dims()
            net_ptr, pin_ids = h.pins()
            ctx.spmv_setup_pins(h)
            ctx.lanczos_fiedler()
            ctx.kl_graph_setup(h.kl_graph())
            ctx.kl_nets_setup(net_ptr, pin_ids)
            ctx.kl_set_partition_fiedler()
            _, kl = ctx.kl_run()
            side = ctx.kl_sides(1)
            wl = {"name": name, "nets": nets, "nodes": nodes, "pins": pins, "kl_net_cut_best": kl["net_cut_best"],
                  "fmw": []}
            out["workloads"].append(wl)
            print(f"{name}: {nodes} nodes, {nets} nets, KL net cut {kl['net_cut_best']}", flush=True)
            weightings = {"synthetic": ((1 + np.arange(nodes) % 5).astype(np.int32),
                                        (1 + np.arange(nets) % 3).astype(np.int32)),
                          "ones": (np.ones(nodes, np.int32), np.ones(nets, np.int32))}
            plain = ek.Hypergraph.from_pins(nodes, net_ptr, pin_ids)
            for wname, (node_w, net_w) in weightings.items():
                h.set_weights(node_w, net_w)
                for stall in a.stalls:
                    wrows, urows, last, ulast = [], [], None, None
                    for i in range(a.warmup + a.runs):
                        got = ctx.fm_refine_w(h, side, a.imbalance, 0, stall, move_cap=len(last[2]) if last else None)
                        ugot = ctx.fm_refine(plain, side, a.imbalance, 0, stall, move_cap=len(ulast[2]) if ulast else None)
                        assert last is None or (np.array_equal(got[0], last[0]) and np.array_equal(got[2], last[2]))
                        last, ulast = got, ugot
                        print(f"    {wname} stall {stall} round {i}: weighted {got[3]['t_passes']:.3f} s, unweighted "
                              f"{ugot[3]['t_passes']:.3f} s of passes", flush=True)
                        if i >= a.warmup:
                            wrows.append(dict(got[3], total=sum(got[3][x] for x in TIMES)))
                            urows.append(dict(ugot[3], total=sum(ugot[3][x] for x in TIMES)))
                    hosts = []
                    for _ in range(a.host_runs):
                        hgot = ek.fm_refine_w_host(h, side, a.imbalance, 0, stall, move_cap=len(last[2]))
                        hosts.append(dict(hgot[3], total=sum(hgot[3][x] for x in TIMES)))
                    assert np.array_equal(last[0], hgot[0]) and np.array_equal(last[1], hgot[1]), "device and host differ"
                    assert np.array_equal(last[2], hgot[2]), "device and host move logs differ"
                    res, ures = last[3], ulast[3]
                    assert all(all(r[f] == res[f] for f in INTS) for r in wrows + hosts), "runs differ"
                    assert ures["cut_before"] == kl["net_cut_best"] == res["cut_nets_before"]
                    if wname == "ones":  # the weighted rule under unit weights is the unweighted rule
                        assert np.array_equal(last[0], ulast[0]) and np.array_equal(last[1], ulast[1])
                        assert np.array_equal(last[2], ulast[2]) and all(res[f] == ures[f] for f in SHARED)
                    row = {"weights": wname, "imbalance": a.imbalance, "stall": stall, "warmup": a.warmup, "runs": a.runs,
                           "host_runs": a.host_runs, **{f: res[f] for f in INTS}, "pass_log": last[1].tolist(),
                           "weighted_device_ms": summary(wrows, res["moves_tried"]),
                           "weighted_host_ms": summary(hosts, res["moves_tried"]),
                           "unweighted": {f: ures[f] for f in SHARED},
                           "unweighted_device_ms": summary(urows, ures["moves_tried"])}
                    wl["fmw"].append(row)
                    d, u, hm = row["weighted_device_ms"], row["unweighted_device_ms"], row["weighted_host_ms"]
                    print(f"  {wname} stall {stall}: weighted cut {res['cut_before']} -> {res['cut']} (cut nets "
                          f"{res['cut_nets_before']} -> {res['cut_nets']}), {res['passes']} passes ({res['passes_run']} run), "
                          f"moves {res['moves_kept']} / {res['moves_tried']}, weights {res['w0']} | {res['w1']} (max "
                          f"{res['max_part']}); weighted device {d['total']['median']:.2f} ms ({d['us_per_move']:.2f} us/move), "
                          f"unweighted device {u['total']['median']:.2f} ms ({u['us_per_move']:.2f} us/move, "
                          f"{ures['moves_tried']} moves); weighted host {hm['total']['median']:.2f} ms "
                          f"({hm['us_per_move']:.2f} us/move)", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:  # (after every workload: a long run leaves what it finished)
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        ctx.close()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
