#!/usr/bin/env python3
"""Cost and effect of ek_partition_kway_direct and ek_hgr_contract_device: the headline workload
(bench.py's: the largest component of Hypergraph.generate(1.15, 1)) and ibm01, under unit weights and under §12's
synthetic weights (node 1 + id mod 5, net 1 + e mod 3), everything at imbalance 0.03 and the default options.

    python tools/kwayd_bench.py [--out profiles/kwayd/kwayd_headline.json]

One box, one warm context.  Two blocks:
  * k = 4, 8, 16: 1 warm-up and --runs timed runs of the driver with the device and with the host contraction
    (medians; the two give the same part vector, asserted), beside ek_partition_kway_ml alone and followed by
    ek_kway_jet, --ml-runs timed runs each, in the same process;
  * the contraction of every level of the driver's hierarchy (k = 8's max_cluster): ek_hgr_contract_device, uploads
    and download included, against ek_hgr_contract, 1 warm-up and --runs timed runs each, the same fields (asserted)."""
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


def direct_row(ctx, h, k, eps, host, runs):
    rows, part = [], None
    for i in range(1 + runs):
        part, r = ctx.partition_kway_direct(h, k, eps, host_contract=host)
        if i >= 1:
            rows.append(r)
    first = rows[0]
    assert all(all(r[f] == first[f] for f in FIXED) for r in rows), "runs differ"
    row = {f: first[f] for f in FIXED}
    row.update(nodes=first["nodes"], conn_w_before=first["conn_w_before"], conn_w_after=first["conn_w_after"],
               jet_iters=first["jet_iters"], jet_moves=first["jet_moves"],
               ms={t: spread([r[t] for r in rows]) for t in TIMES})
    return part, row


def contraction_rows(ek, ctx, h, max_cluster, coarse, runs):
    """Every level of the hierarchy the driver builds: device against host, the same process."""
    out, cur = [], h
    while cur.nodes > coarse:
        _, cluster, _, mr = ctx.match(cur, max_cluster)
        if 10 * mr["n_coarse"] > 9 * cur.nodes:
            break
        dev, host, nxt = [], [], None
        for i in range(1 + runs):
            t = time.perf_counter()
            nxt = cur.contract(cluster, mr["n_coarse"])
            t_host = time.perf_counter() - t
            t = time.perf_counter()
            got = ctx.hgr_contract(cur, cluster, mr["n_coarse"])
            t_dev = time.perf_counter() - t
            if i >= 1:
                host.append(t_host)
                dev.append(t_dev)
        a, b = nxt.pins(), got.pins()
        assert nxt.dims() == got.dims() and all(np.array_equal(x, y) for x, y in zip(a, b)), "device and host differ"
        assert all(np.array_equal(x, y) for x, y in zip(nxt.weights(), got.weights())), "device and host differ"
        nets, nodes, pins = cur.dims()
        out.append({"level": len(out), "nodes": nodes, "nets": nets, "pins": pins, "coarse_nodes": nxt.nodes,
                    "coarse_nets": nxt.nets, "device_ms": spread(dev), "host_ms": spread(host)})
        cur = nxt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kwayd", "kwayd_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--imbalance", type=float, default=0.03)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ml-runs", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["headline", "ibm01"])
    a = ap.parse_args()
    ek = _load_package()
    ctx = ek.Context(0)
    eps = a.imbalance
    out = {"imbalance": eps, "warmup": 1, "runs": a.runs, "ml_runs": a.ml_runs, "kway": [], "contraction": []}
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
                    part_d, dev = direct_row(ctx, h, k, eps, False, a.runs)
                    part_h, host = direct_row(ctx, h, k, eps, True, a.runs)
                    assert part_d.tobytes() == part_h.tobytes() and all(dev[f] == host[f] for f in FIXED)
                    ml_t, jet_t, ml, jr = [], [], None, None
                    for _ in range(a.ml_runs):
                        t = time.perf_counter()
                        start, ml = ctx.partition_kway_ml(h, k, eps)
                        ml_t.append(time.perf_counter() - t)
                        t = time.perf_counter()
                        _, jr, _ = ctx.kway_jet(h, start, k, eps)
                        jet_t.append(time.perf_counter() - t)
                    row = {**tag, "k": k, "direct": dev, "direct_host_contract_ms": host["ms"],
                           "kway_ml": {"connectivity_w": ml["connectivity_w"], "part_w_max": ml["part_w_max"],
                                       "parts_over_bound": ml["parts_over_bound"], "ms": spread(ml_t)},
                           "kway_ml_jet": {"connectivity_w": jr["connectivity_w"], "part_w_max": jr["part_w_max"],
                                           "parts_over_bound": jr["parts_over_bound"],
                                           "ms": spread([x + y for x, y in zip(ml_t, jet_t)])}}
                    out["kway"].append(row)
                    d = dev["ms"]
                    print(f"{wl}/{weights} k {k}: direct connectivity_w {dev['connectivity_w']} (initial "
                          f"{dev['conn_w_before'][-1]}, {dev['levels']} levels to {dev['nodes'][-1]} nodes), heaviest "
                          f"{dev['part_w_max']} of {dev['part_bound']}, over {dev['parts_over_bound']}; "
                          f"{d['t_total']['median']:.1f} ms (match {d['t_match']['median']:.1f}, contract "
                          f"{d['t_contract']['median']:.1f} [host {host['ms']['t_contract']['median']:.1f}], initial "
                          f"{d['t_initial']['median']:.1f}, jet {d['t_jet']['median']:.1f}, metrics "
                          f"{d['t_metrics']['median']:.1f}); host-contract total {host['ms']['t_total']['median']:.1f} ms; "
                          f"kway_ml {ml['connectivity_w']} in {row['kway_ml']['ms']['median']:.0f} ms, + jet "
                          f"{jr['connectivity_w']} in {row['kway_ml_jet']['ms']['median']:.0f} ms", flush=True)
                # the hierarchy of k = 8 (the defaults' max_cluster)
                k = 8
                node_w, _ = h.weights()
                W = int(node_w.sum()) if node_w is not None else nodes
                share = -(-W // k)
                coarse = max(512, 128 * k)
                cap = max(1, min(-(-4 * W // coarse), max(1, int(math.floor((1.0 + eps) * share)) - share)))
                for r in contraction_rows(ek, ctx, h, cap, coarse, a.runs):
                    out["contraction"].append({**tag, "max_cluster": cap, **r})
                    print(f"{wl}/{weights} contraction level {r['level']}: {r['nodes']} nodes, {r['nets']} nets, "
                          f"{r['pins']} pins -> {r['coarse_nodes']} nodes, {r['coarse_nets']} nets: device "
                          f"{r['device_ms']['median']:.2f} ms ({r['device_ms']['min']:.2f}..{r['device_ms']['max']:.2f}), "
                          f"host {r['host_ms']['median']:.2f} ms ({r['host_ms']['min']:.2f}..{r['host_ms']['max']:.2f})",
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
