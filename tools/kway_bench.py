#!/usr/bin/env python3
"""Cost of ek_partition_kway on the headline workload (bench.py's: the largest
component of Hypergraph.generate(1.15, 1)) for k = 2, 4, 8, 16, beside a warm
ek_solve_file step on the same machine as the yardstick.

    python tools/kway_bench.py [--out profiles/kway/kway_headline.json]

Each k: 3 warm-ups and 10 timed runs; the medians of the wall time and of the
per-phase times, the matvecs, KL swaps and the three metrics (identical in
every run: the solver is deterministic)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load_package  # noqa: E402

PHASES = ("t_induce", "t_lanczos", "t_kl", "t_metrics", "t_total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kway", "kway_headline.json"))
    ap.add_argument("--mult", type=float, default=1.15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8, 16])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    ek = _load_package()
    h, _ = ek.Hypergraph.generate(a.mult, a.seed).largest_component()
    nets, nodes, pins = h.dims()
    ctx = ek.Context(0)
    out = {"workload": {"mult": a.mult, "seed": a.seed, "nets": nets, "nodes": nodes, "pins": pins},
           "warmup": a.warmup, "runs": a.runs, "kway": []}
    try:
        # the yardstick: a warm ek_solve_file step (bench.py's flagship step) on this machine
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "headline.hgr")
            h.write(path)
            steps = []
            for i in range(a.warmup + a.runs):
                t = time.perf_counter()
                res, _ = ctx.solve_file(path, out_dir=d)
                if i >= a.warmup:
                    steps.append({"wall_ms": 1e3 * (time.perf_counter() - t),
                                  "compute_ms": 1e3 * (res["t_total"] - res["t_read"] - res["t_write"])})
        out["solve_file"] = {k: {"median": statistics.median(s[k] for s in steps), "min": min(s[k] for s in steps),
                                 "max": max(s[k] for s in steps)} for k in ("wall_ms", "compute_ms")}
        for k in a.ks:
            rows = []
            for i in range(a.warmup + a.runs):
                t = time.perf_counter()
                _, r = ctx.partition_kway(h, k)
                r["wall"] = time.perf_counter() - t
                if i >= a.warmup:
                    rows.append(r)
            first = rows[0]
            fixed = ("bisections", "fallback_splits", "part_min", "part_max", "cut_nets", "connectivity", "soed",
                     "matvecs", "kl_swaps")
            assert all(all(r[f] == first[f] for f in fixed) for r in rows), "runs differ"
            row = {"k": k, **{f: first[f] for f in fixed}}
            for p in PHASES + ("wall",):
                row[p + "_ms"] = {"median": 1e3 * statistics.median(r[p] for r in rows),
                                  "min": 1e3 * min(r[p] for r in rows), "max": 1e3 * max(r[p] for r in rows)}
            row["t_level_ms"] = [1e3 * statistics.median(r["t_level"][j] for r in rows) for j in range(8)]
            row["ratio_to_solve_compute"] = row["t_total_ms"]["median"] / out["solve_file"]["compute_ms"]["median"]
            out["kway"].append(row)
            print(f"k {k}: {row['t_total_ms']['median']:.2f} ms (lanczos {row['t_lanczos_ms']['median']:.2f}, kl "
                  f"{row['t_kl_ms']['median']:.2f}, induce {row['t_induce_ms']['median']:.2f}, metrics "
                  f"{row['t_metrics_ms']['median']:.2f}), {first['matvecs']} matvecs, {first['kl_swaps']} swaps, cut nets "
                  f"{first['cut_nets']}, connectivity {first['connectivity']}, SOED {first['soed']}", flush=True)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"solve_file step: compute {out['solve_file']['compute_ms']['median']:.2f} ms "
          f"[{out['solve_file']['compute_ms']['min']:.2f}, {out['solve_file']['compute_ms']['max']:.2f}]; wrote {a.out}")


if __name__ == "__main__":
    main()
