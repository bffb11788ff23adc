"""The direct k-way driver with the rebalancing step (ek_partition_kway_direct_rb) on the GPU.  It is a composition of
public entries, so the same cycle composed here (the coarsening, ctx.partition_kway_ml, then per level the part
weights, ctx.kway_rebalance when a part is above Lk, and ctx.kway_jet) must give the same part vector and the same
integers; without an overweight level it is ek_partition_kway_direct_ex; with one, it may not end with more parts
above the bound than that entry does."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import contract_cases as cc
from conftest import PKG_DIR, circuit_path

pytestmark = pytest.mark.gpu

LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "conn_w_before", "conn_w_after", "jet_iters",
                "jet_moves")
RB_FIELDS = ("over_before", "excess_before", "rb_rounds", "rb_moves", "excess_after")
INTS = ("k", "levels", "initial_fallbacks", "infeasible_sweeps", "total_weight", "part_bound", "max_cluster",
        "part_w_min", "part_w_max", "parts_over_bound", "empty_parts", "cut_nets", "connectivity", "connectivity_w",
        "soed")
COARSE = {"fract": 16, "ibm01": 0}  # 0: the default, max(512, 128 k)
# (circuit, §12's synthetic weights, k, eps, coarsening); OVER: a level starts above the bound (found by a search over
# k = 3, 5, 8 at eps = 0 with both coarsenings; the first that does), CALM: none does
OVER = ("fract", True, 5, 0.0, "match")
CALM = ("ibm01", False, 2, 0.10, "match")
CASES = [OVER, CALM, ("fract", True, 8, 0.0, "cluster"), ("ibm01", True, 5, 0.0, "match"),
         ("ibm01", True, 8, 0.03, "cluster")]


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def circuit(ek, name, weighted):
    h = ek.Hypergraph.read(circuit_path(name))
    if weighted:
        h.set_weights(*cc.synthetic_weights(h.nodes, h.nets))
    return h


def ints(res, fields=LEVEL_FIELDS):
    return {f: res[f] for f in INTS} | {f: list(res[f]) for f in fields}


def compose(ek, ctx, h, k, eps, coarse_nodes, coarsening):
    """§19.1's cycle with §21's step from the public pieces: the driver's integers."""
    node_w, _ = h.weights()
    W = int(node_w.sum()) if node_w is not None else h.nodes
    share = -(-W // k)
    Lk = int(math.floor((1.0 + eps) * float(share)))
    coarse = coarse_nodes if coarse_nodes > 0 else max(512, 128 * k)
    max_cluster = max(1, min(-(-4 * W // coarse), max(1, Lk - share)))
    levels, clusters = [h], []
    r = {f: [] for f in LEVEL_FIELDS + RB_FIELDS}
    while levels[-1].nodes > coarse and len(clusters) < ek.ML_LEVELS:
        cur = levels[-1]
        if coarsening == "cluster":
            cluster, _, cr = ctx.cluster(cur, max_cluster)[-3:]
            n_coarse, rounds, pairs = cr["n_coarse"], cr["rounds"], cr["joins"]
        else:
            _, cluster, _, mr = ctx.match(cur, max_cluster)
            n_coarse, rounds, pairs = mr["n_coarse"], mr["rounds"], mr["pairs"]
        if 10 * n_coarse > 9 * cur.nodes:
            break
        levels.append(cur.contract(cluster, n_coarse))
        clusters.append(cluster)
        r["match_rounds"].append(rounds)
        r["match_pairs"].append(pairs)
    L = len(clusters)
    r["match_rounds"].append(0)
    r["match_pairs"].append(0)
    for g in levels:
        nets, nodes, pins = g.dims()
        r["nodes"].append(nodes)
        r["nets"].append(nets)
        r["pins"].append(pins)
    part, ir = ctx.partition_kway_ml(levels[L], k, eps)
    for f in ("conn_w_before", "conn_w_after", "jet_iters", "jet_moves") + RB_FIELDS:
        r[f] = [0] * (L + 1)
    for l in range(L, -1, -1):
        if l < L:
            part = part[clusters[l]]
        pw = ek.kway_metrics_w_host(levels[l], part, k)[1]
        r["over_before"][l] = int(np.count_nonzero(pw > Lk))
        r["excess_before"][l] = r["excess_after"][l] = int(np.maximum(pw - Lk, 0).sum())
        if r["over_before"][l]:
            part, br, _ = ctx.kway_rebalance(levels[l], part, k, eps)
            r["rb_rounds"][l], r["rb_moves"][l], r["excess_after"][l] = br["rounds"], br["moves"], br["excess"]
        part, jr, _ = ctx.kway_jet(levels[l], part, k, eps)
        r["conn_w_before"][l], r["conn_w_after"][l] = jr["connectivity_w_before"], jr["connectivity_w"]
        r["jet_iters"][l], r["jet_moves"][l] = jr["iters"], jr["moves"]
    (cut, conn, connw, soed), pw = ctx.kway_metrics_w(h, part, k)
    r.update(k=k, levels=L, initial_fallbacks=ir["coarsest_fallbacks"], infeasible_sweeps=ir["infeasible_sweeps"],
             total_weight=W, part_bound=Lk, max_cluster=max_cluster, part_w_min=int(min(pw)), part_w_max=int(max(pw)),
             parts_over_bound=int(sum(int(x) > Lk for x in pw)),
             empty_parts=int(k - np.count_nonzero(np.bincount(part, minlength=k))), cut_nets=cut, connectivity=conn,
             connectivity_w=connw, soed=soed)
    return part.astype(np.int32), r


@pytest.mark.parametrize("name, weighted, k, eps, coarsening", CASES)
def test_driver_equals_its_composition(ek, ctx, name, weighted, k, eps, coarsening):
    h = circuit(ek, name, weighted)
    part, res = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name], coarsening=coarsening, rebalance=True)
    want, r = compose(ek, ctx, h, k, eps, COARSE[name], coarsening)
    assert part.tobytes() == want.tobytes()
    assert ints(res, LEVEL_FIELDS + RB_FIELDS) == ints(r, LEVEL_FIELDS + RB_FIELDS)
    for l in range(res["levels"] + 1):
        assert res["excess_after"][l] <= res["excess_before"][l]
        assert (res["rb_rounds"][l] > 0) == (res["rb_moves"][l] > 0) and (res["over_before"][l] > 0 or not res["rb_moves"][l])


def test_without_an_overweight_level_it_is_the_plain_driver(ek, ctx):
    name, weighted, k, eps, coarsening = CALM
    h = circuit(ek, name, weighted)
    part, res = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name], coarsening=coarsening, rebalance=True)
    assert not any(res["over_before"]) and not any(res["rb_rounds"]) and not any(res["excess_after"])
    plain, pres = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name], coarsening=coarsening)
    assert part.tobytes() == plain.tobytes() and ints(res) == ints(pres)
    assert "over_before" not in pres  # the default is the entry it was


def test_an_overweight_level_is_rebalanced(ek, ctx):
    name, weighted, k, eps, coarsening = OVER
    h = circuit(ek, name, weighted)
    part, res = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name], coarsening=coarsening, rebalance=True)
    assert any(x > 0 for x in res["over_before"]), res["over_before"]  # (or the test shows nothing)
    _, pres = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name], coarsening=coarsening)
    print(f"{OVER}: over_before {res['over_before']}, excess {res['excess_before']} -> {res['excess_after']}, "
          f"parts_over_bound {pres['parts_over_bound']} -> {res['parts_over_bound']}, connectivity_w "
          f"{pres['connectivity_w']} -> {res['connectivity_w']}")
    assert res["parts_over_bound"] <= pres["parts_over_bound"]
    for l in range(res["levels"] + 1):
        assert res["excess_after"][l] <= res["excess_before"][l], l
    assert part.min() >= 0 and part.max() < k


def test_cli_rebalance_line(ek, ctx, tmp_path):
    fract = circuit_path("fract")
    h = ek.Hypergraph.read_weighted(fract)
    part, res = ctx.partition_kway_direct(h, 5, 0.0, coarse_nodes=16, coarsening="cluster", rebalance=True)
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    args = [tool, fract, "-EIG", "--k", "5", "--kway-direct", "0", "--ml-coarse", "16", "--coarsen", "cluster"]
    r = subprocess.run(args + ["--rebalance"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "fract.hgr.part.5").read_text()
    assert [int(x) for x in text.split()] == part.tolist()
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("kway-direct:")]) == 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("rebalance:")]
    assert len(line) == 1
    got = [int(x) for x in re.findall(r"-?\d+", line[0].rsplit(",", 1)[0])]
    assert got == [sum(x > 0 for x in res["over_before"]), sum(res["rb_rounds"]), sum(res["rb_moves"]),
                   res["excess_after"][0]], line[0]
    plain = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and not [ln for ln in plain.stdout.splitlines() if ln.startswith("rebalance:")]
