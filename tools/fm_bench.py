#!/usr/bin/env python3
"""Effect and cost of the FM refinement (ek_fm_refine) after the KL loop, on the
headline workload (bench.py's: the largest component of
Hypergraph.generate(1.15, 1)) and on ibm01.

    python tools/fm_bench.py [--out profiles/fm/fm_headline.json]

Each workload: the Laplacian on the device, one Lanczos solve, the KL graph and
nets; then three starts, each the sides of KL's best prefix: from the median
split (FM at imbalance 0.03) and from the sweep cut at imbalance 0.03 and 0.10
(FM at the same imbalance).  Per start and per stall (the default 1000, and 0:
a pass runs until no node can move) ek_fm_refine on a warm context, --warmup
warm-ups + --runs timed runs (2 + 7 by default; every row records its own) (medians of its set-up / passes / metrics times, microseconds
per move tried) against the single-threaded ek_fm_refine_host on the same
input.  The sides, both logs and the result integers are identical in every
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

TIMES = ("t_setup", "t_passes", "t_metrics")
INTS = ("n", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut", "n0", "n1")


def med(rows, key):
    return {"median": 1e3 * statistics.median(r[key] for r in rows), "min": 1e3 * min(r[key] for r in rows),
            "max": 1e3 * max(r[key] for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fm", "fm_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stalls", type=int, nargs="+", default=[1000, 0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--append", action="store_true",
                    help="add the rows to the workloads of an existing --out file (a long measurement in several runs)")
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"], choices=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    load = {"headline": lambda: ek.Hypergraph.generate(a.mult, a.seed).largest_component()[0],
            "ibm01": lambda: ek.Hypergraph.read(os.path.join(REPO, "tests", "golden", "circuit", "ibm01.hgr"))}
    ctx = ek.Context(0)
    out = {"workloads": []}
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    try:
        for name in a.workloads:
            h = load[name]()
            nets, nodes, pins = h.dims()
            net_ptr, pin_ids = h.pins()
            ctx.spmv_setup_pins(h)
            ctx.lanczos_fiedler()
            ctx.kl_graph_setup(h.kl_graph())
            ctx.kl_nets_setup(net_ptr, pin_ids)
            wl = next((w for w in out["workloads"] if w["name"] == name), None)
            if wl is None:
                wl = {"name": name, "nets": nets, "nodes": nodes, "pins": pins, "fm": []}
                out["workloads"].append(wl)
            print(f"{name}: {nodes} nodes, {nets} nets", flush=True)
            for start, eps in (("median", 0.03), ("sweep", 0.03), ("sweep", 0.10)):
                if start == "median":
                    ctx.kl_set_partition_fiedler()
                else:
                    ctx.kl_set_partition_fiedler_sweep(h, eps, False)
                _, kl = ctx.kl_run()
                side = ctx.kl_sides(1)
                for stall in a.stalls:
                    rows, last = [], None
                    for i in range(a.warmup + a.runs):
                        got = ctx.fm_refine(h, side, eps, 0, stall, move_cap=len(last[2]) if last else None)
                        assert last is None or (np.array_equal(got[0], last[0]) and np.array_equal(got[2], last[2]))
                        last = got
                        print(f"    {start} eps {eps} stall {stall} run {i}: {got[3]['t_passes']:.3f} s of passes, "
                              f"{got[3]['passes_run']} passes run", flush=True)
                        if i >= a.warmup:
                            rows.append(dict(got[3], total=sum(got[3][x] for x in TIMES)))
                    hosts = []
                    for _ in range(a.host_runs):
                        hgot = ek.fm_refine_host(h, side, eps, 0, stall, move_cap=len(last[2]))
                        hosts.append(dict(hgot[3], total=sum(hgot[3][x] for x in TIMES)))
                    assert np.array_equal(last[0], hgot[0]) and np.array_equal(last[1], hgot[1]), "device and host differ"
                    assert np.array_equal(last[2], hgot[2]), "device and host move logs differ"
                    res = last[3]
                    assert all(all(r[f] == res[f] for f in INTS) for r in rows + hosts), "runs differ"
                    assert res["cut_before"] == kl["net_cut_best"]
                    tried = max(res["moves_tried"], 1)
                    row = {"start": start, "imbalance": eps, "stall": stall, "warmup": a.warmup, "runs": a.runs,
                           "host_runs": a.host_runs, "kl_net_cut_best": kl["net_cut_best"],
                           "kl_iterations": kl["iterations"], "kl_loop_ms": kl["loop_ms"], **{f: res[f] for f in INTS},
                           "pass_log": last[1].tolist(),
                           "device_ms": {x: med(rows, x) for x in TIMES + ("total",)},
                           "device_us_per_move": 1e3 * med(rows, "t_passes")["median"] / tried,
                           "host_ms": {x: med(hosts, x) for x in TIMES + ("total",)},
                           "host_us_per_move": 1e3 * med(hosts, "t_passes")["median"] / tried}
                    wl["fm"].append(row)
                    d, hm = row["device_ms"], row["host_ms"]
                    print(f"  {start} eps {eps} stall {stall}: cut {res['cut_before']} -> {res['cut']}, {res['passes']} "
                          f"passes ({res['passes_run']} run), moves {res['moves_kept']} / {res['moves_tried']}, sizes "
                          f"{res['n0']} | {res['n1']} (max {res['max_part']}); device {d['total']['median']:.2f} ms (setup "
                          f"{d['t_setup']['median']:.2f}, passes {d['t_passes']['median']:.2f}, metrics "
                          f"{d['t_metrics']['median']:.2f}; {row['device_us_per_move']:.2f} us/move); host "
                          f"{hm['total']['median']:.2f} ms ({row['host_us_per_move']:.2f} us/move)", flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:  # (after every workload: a long run leaves what it finished)
                json.dump(out, f, indent=1)
                f.write("\n")
    finally:
        ctx.close()
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
