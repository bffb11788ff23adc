"""The direct k-way multilevel driver (ek_partition_kway_direct) on the GPU.  It is a composition of public entries and
nothing else, so the same cycle composed here from ctx.match, Hypergraph.contract, ctx.partition_kway_ml and
ctx.kway_jet must give the same part vector and the same result integers; the device and the host contraction must
give the same result; and the four promises of DESIGN.md §19 must hold at every level."""
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
INTS = ("k", "levels", "initial_fallbacks", "infeasible_sweeps", "total_weight", "part_bound", "max_cluster",
        "part_w_min", "part_w_max", "parts_over_bound", "empty_parts", "cut_nets", "connectivity", "connectivity_w",
        "soed")
CASES = [(name, weighted, k, eps) for name in ("fract", "ibm01") for weighted in (False, True) for k in (2, 3, 8)
         for eps in (0.03, 0.10)]
COARSE = {"fract": 16, "ibm01": 0}  # 0: the default, max(512, 128 k)


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


def ints(res):
    return {f: res[f] for f in INTS} | {f: list(res[f]) for f in LEVEL_FIELDS}


def part_weights(ek, h, part, k):
    return ek.kway_metrics_w_host(h, part, k)[1]


def compose(ek, ctx, h, k, eps, coarse_nodes):
    """The cycle of §19 from the public pieces.  Returns (part, the driver's result integers, the part weights after
    the initial partition, [(part weights before, after the projection) per projected level])."""
    node_w, _ = h.weights()
    W = int(node_w.sum()) if node_w is not None else h.nodes
    share = -(-W // k)
    Lk = int(math.floor((1.0 + eps) * float(share)))
    coarse = coarse_nodes if coarse_nodes > 0 else max(512, 128 * k)
    max_cluster = max(1, min(-(-4 * W // coarse), max(1, Lk - share)))
    levels, clusters = [h], []
    r = {f: [] for f in LEVEL_FIELDS}
    while levels[-1].nodes > coarse and len(clusters) < ek.ML_LEVELS:
        cur = levels[-1]
        _, cluster, _, mr = ctx.match(cur, max_cluster)
        if 10 * mr["n_coarse"] > 9 * cur.nodes:
            break
        levels.append(cur.contract(cluster, mr["n_coarse"]))
        clusters.append(cluster)
        r["match_rounds"].append(mr["rounds"])
        r["match_pairs"].append(mr["pairs"])
    L = len(clusters)
    r["match_rounds"].append(0)
    r["match_pairs"].append(0)
    for g in levels:
        nets, nodes, pins = g.dims()
        r["nodes"].append(nodes)
        r["nets"].append(nets)
        r["pins"].append(pins)
    part, ir = ctx.partition_kway_ml(levels[L], k, eps)
    initial_w = part_weights(ek, levels[L], part, k)
    before, after, iters, moves, projections = [0] * (L + 1), [0] * (L + 1), [0] * (L + 1), [0] * (L + 1), []
    for l in range(L, -1, -1):
        if l < L:
            coarse_w = part_weights(ek, levels[l + 1], part, k)
            part = part[clusters[l]]
            projections.append((coarse_w, part_weights(ek, levels[l], part, k)))
        part, jr, _ = ctx.kway_jet(levels[l], part, k, eps)
        before[l], after[l], iters[l], moves[l] = (jr["connectivity_w_before"], jr["connectivity_w"], jr["iters"],
                                                   jr["moves"])
    r.update(conn_w_before=before, conn_w_after=after, jet_iters=iters, jet_moves=moves)
    (cut, conn, connw, soed), pw = ctx.kway_metrics_w(h, part, k)
    r.update(k=k, levels=L, initial_fallbacks=ir["coarsest_fallbacks"], infeasible_sweeps=ir["infeasible_sweeps"],
             total_weight=W, part_bound=Lk, max_cluster=max_cluster, part_w_min=int(min(pw)), part_w_max=int(max(pw)),
             parts_over_bound=int(sum(int(x) > Lk for x in pw)),
             empty_parts=int(k - np.count_nonzero(np.bincount(part, minlength=k))), cut_nets=cut, connectivity=conn,
             connectivity_w=connw, soed=soed)
    return part.astype(np.int32), r, initial_w, projections


@pytest.mark.parametrize("name, weighted, k, eps", CASES)
def test_driver_equals_its_composition_and_keeps_its_promises(ek, ctx, name, weighted, k, eps):
    h = circuit(ek, name, weighted)
    part, res = ctx.partition_kway_direct(h, k, eps, coarse_nodes=COARSE[name])
    want, r, initial_w, projections = compose(ek, ctx, h, k, eps, COARSE[name])
    assert part.tobytes() == want.tobytes()
    assert ints(res) == ints(r)
    # the host contraction: the same result
    part_h, res_h = ctx.partition_kway_direct(h, k, eps, host_contract=True, coarse_nodes=COARSE[name])
    assert part_h.tobytes() == part.tobytes() and ints(res_h) == ints(res)
    # every node has a part
    assert part.min() >= 0 and part.max() < k
    L = res["levels"]
    assert L >= 1 or name == "fract"  # (fract at k = 8: a part's slack is below 2, so nothing may be matched)
    for l in range(L):  # the weighted connectivity survives the projection
        assert res["conn_w_before"][l] == res["conn_w_after"][l + 1], l
    for l in range(L + 1):  # Jet never returns worse than it was given
        assert res["conn_w_after"][l] <= res["conn_w_before"][l], l
    assert res["connectivity_w"] == res["conn_w_after"][0]
    assert len(projections) == L
    for coarse_w, fine_w in projections:  # part weights are unchanged by projection
        assert list(coarse_w) == list(fine_w)
    final_w = part_weights(ek, h, part, k)
    for p in range(k):  # no part ends above max(Lk, its weight after the initial partition)
        assert final_w[p] <= max(res["part_bound"], initial_w[p]), p
    assert res["parts_over_bound"] == sum(int(x) > res["part_bound"] for x in final_w)


@pytest.mark.parametrize("name, weighted", [("fract", True), ("ibm01", False)])
def test_two_runs_give_the_same_bytes(ek, ctx, name, weighted):
    h = circuit(ek, name, weighted)
    a, ra = ctx.partition_kway_direct(h, 3, 0.03, coarse_nodes=COARSE[name])
    b, rb = ctx.partition_kway_direct(h, 3, 0.03, coarse_nodes=COARSE[name])
    assert a.tobytes() == b.tobytes() and ints(ra) == ints(rb)


def test_zero_levels_is_the_initial_partition_then_jet(ek, ctx):
    h = circuit(ek, "fract", True)  # 149 nodes, below the default coarse_nodes
    for k in (2, 5):
        part, res = ctx.partition_kway_direct(h, k, 0.05)
        start, _ = ctx.partition_kway_ml(h, k, 0.05)
        want, jr, _ = ctx.kway_jet(h, start, k, 0.05)
        assert res["levels"] == 0 and part.tobytes() == want.astype(np.int32).tobytes()
        assert (res["conn_w_before"], res["conn_w_after"]) == ([jr["connectivity_w_before"]], [jr["connectivity_w"]])
        assert res["connectivity_w"] == jr["connectivity_w"]


def test_weighted_laplacian_flag_reaches_the_initial_partition(ek, ctx):
    h = circuit(ek, "ibm01", True)
    part, res = ctx.partition_kway_direct(h, 3, 0.03, weighted_laplacian=True)
    assert part.min() >= 0 and part.max() < 3 and res["connectivity_w"] == res["conn_w_after"][0]
    levels = res["levels"]
    assert all(res["conn_w_before"][l] == res["conn_w_after"][l + 1] for l in range(levels))


def test_argument_and_state_errors(ek):
    import ctypes
    h = circuit(ek, "fract", False)
    one = ek.Context(0)
    try:
        for k in (1, 257):
            with pytest.raises(ek.EKError) as e:
                one.partition_kway_direct(h, k)
            assert e.value.code == ek.EK_EINVAL
        for eps in (-0.01, float("nan"), float("inf")):
            with pytest.raises(ek.EKError) as e:
                one.partition_kway_direct(h, 2, eps)
            assert e.value.code == ek.EK_EINVAL
        o = ek.KwayDirectOpts()
        ek.lib.ek_kway_direct_default_opts(ctypes.byref(o))
        o.flags = 4
        part = np.zeros(h.nodes, np.int32)
        assert ek.lib.ek_partition_kway_direct(one._c, h._h, ctypes.byref(o), part.ctypes.data, None) == ek.EK_EINVAL
        assert ek.lib.ek_partition_kway_direct(one._c, None, None, part.ctypes.data, None) == ek.EK_EINVAL
        assert ek.lib.ek_partition_kway_direct(one._c, h._h, None, None, None) == ek.EK_EINVAL
        # opts NULL: k = 2 at the defaults
        assert ek.lib.ek_partition_kway_direct(one._c, h._h, None, part.ctypes.data, None) == ek.EK_OK
        assert part.tobytes() == one.partition_kway_direct(h, 2)[0].tobytes()

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:  # a multi-rank context
            one.partition_kway_direct(h, 2)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


CLI_KEYS = ("k|levels|coarsest_nodes|max_cluster|fallbacks|infeasible|total_weight|part_bound|over_bound|empty|"
            "cut nets|connectivity|connectivity_w|SOED|jet iterations|jet moves")


@pytest.mark.parametrize("host", [False, True])
def test_cli_kway_direct(ek, ctx, tmp_path, host):
    h = circuit(ek, "ibm01", True)
    src = tmp_path / "ibm01w.hgr"
    h.write(src)  # fmt 11
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), str(src), "-EIG", "--k", "5", "--kway-direct", "0.03",
                        "--ml-coarse", "700", "--jet-iters", "40"] + (["--contract-host"] if host else []),
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("kway-direct:")]
    assert len(line) == 1, r.stdout
    got = {k: int(v) for k, v in re.findall(rf"\b({CLI_KEYS}) (-?\d+)", line[0])}
    lo, hi = (int(x) for x in re.search(r"part weights (\d+)\.\.(\d+)", line[0]).groups())
    part = np.array((tmp_path / "results" / "ibm01w.hgr.part.5").read_text().split(), np.int32)
    want, res = ctx.partition_kway_direct(h, 5, 0.03, host_contract=host, coarse_nodes=700, jet={"max_iters": 40})
    assert part.tobytes() == want.tobytes()
    assert got == {"k": 5, "levels": res["levels"], "coarsest_nodes": res["nodes"][-1], "max_cluster": res["max_cluster"],
                   "fallbacks": res["initial_fallbacks"], "infeasible": res["infeasible_sweeps"],
                   "total_weight": res["total_weight"], "part_bound": res["part_bound"],
                   "over_bound": res["parts_over_bound"], "empty": res["empty_parts"], "cut nets": res["cut_nets"],
                   "connectivity": res["connectivity"], "connectivity_w": res["connectivity_w"], "SOED": res["soed"],
                   "jet iterations": sum(res["jet_iters"]), "jet moves": sum(res["jet_moves"])}
    assert (lo, hi) == (res["part_w_min"], res["part_w_max"])
    assert f"contract {'host' if host else 'device'}," in line[0]
    assert f"(initial {res['conn_w_before'][-1]})" in line[0]
    # the library's file entry writes the same file
    part_f, res_f = ctx.partition_kway_direct_file(str(src), 5, 0.03, host_contract=host, coarse_nodes=700,
                                                   jet={"max_iters": 40}, out_dir=str(tmp_path / "lib"))
    assert part_f.tobytes() == want.tobytes() and ints(res_f) == ints(res)
    assert (tmp_path / "lib" / "results" / "ibm01w.hgr.part.5").read_text() == \
           (tmp_path / "results" / "ibm01w.hgr.part.5").read_text()
