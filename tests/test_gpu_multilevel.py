"""The multilevel bipartition (ek_multilevel_bipartition) against the same
V-cycle composed here from the public pieces: ek.match_host,
Hypergraph.contract, the context's Lanczos on the coarsest level,
ek.sweep_cut_w_host and ek.fm_refine_w_host.  Every piece is device = host bit
for bit (test_gpu_match.py, test_gpu_sweepw.py, test_gpu_fmw.py), so the
driver's sides and per-level integers must be the composition's."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

CONFIGS = [(name, weighted, eps) for name in ("fract", "ibm01") for weighted in (False, True) for eps in (0.03, 0.10)]
COARSE = {"fract": 16, "ibm01": 512}
LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "cut_before", "cut_after", "fm_moves")
INTS = ("levels", "coarsest_fallback", "sweep_feasible", "max_cluster", "total_weight", "max_part", "cut", "cut_nets",
        "w0", "w1", "n0", "n1")


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def max_part(total, eps):
    return math.floor((1.0 + eps) * float((total + 1) // 2))


def compose(ek, ctx, h, eps, coarse_nodes):
    """(side, result dict) of the V-cycle as eigkl.h states it, from the host checkers and the context's Lanczos."""
    node_w = h.weights()[0]
    W = h.nodes if node_w is None else int(node_w.sum())
    lmax = max_part(W, eps)
    cap = max(1, min(2 * lmax - W + 1, -(-4 * W // coarse_nodes)))
    res = {k: [] for k in LEVEL_FIELDS}
    levels, clusters, cur = [h], [], h
    while cur.nodes > coarse_nodes and len(clusters) < ek.ML_LEVELS:
        _, cluster, _, m = ek.match_host(cur, cap, 64, 8)
        if 10 * m["n_coarse"] > 9 * cur.nodes:
            break
        res["match_rounds"].append(m["rounds"])
        res["match_pairs"].append(m["pairs"])
        cur = cur.contract(cluster, m["n_coarse"])
        levels.append(cur)
        clusters.append(cluster)
    res["match_rounds"].append(0)
    res["match_pairs"].append(0)
    for g in levels:
        nets, nodes, pins = g.dims()
        res["nodes"].append(nodes)
        res["nets"].append(nets)
        res["pins"].append(pins)
    ptr, _ = cur.pins()
    spectral = bool(np.any(np.diff(ptr) >= 2)) and cur.nodes >= 4
    if spectral:
        ctx.spmv_setup_pins(cur)
        try:
            _, v, _ = ctx.lanczos_fiedler()
        except ek.EKError as e:
            if e.code != ek.EK_ENOCONV:
                raise
            spectral = False
    if not spectral:
        v = -np.arange(cur.nodes, dtype=np.float64)
    sweep, _, _, _ = ek.sweep_cut_w_host(cur, v, eps)
    side = ek.rank_split(v, sweep["n1"])
    before, after, moves = [], [], []
    for l in range(len(levels) - 1, -1, -1):
        if l < len(levels) - 1:
            side = side[clusters[l]]
        side, _, _, fm = ek.fm_refine_w_host(levels[l], side, eps)
        before.insert(0, fm["cut_before"])
        after.insert(0, fm["cut"])
        moves.insert(0, fm["moves_kept"])
    res.update(cut_before=before, cut_after=after, fm_moves=moves, levels=len(clusters),
               coarsest_fallback=0 if spectral else 1, sweep_feasible=sweep["feasible"], max_cluster=cap, total_weight=W,
               max_part=lmax)
    cut, cut_nets, w0, w1 = ek.bipart_metrics_host(h, side)
    n1 = int(side.sum())
    res.update(cut=cut, cut_nets=cut_nets, w0=w0, w1=w1, n0=h.nodes - n1, n1=n1)
    return side, res


@pytest.fixture(scope="module")
def runs(ek, ctx):
    """both(name, weighted, eps) -> (hypergraph, the driver's (side, result), the composition's), each configuration
    computed once and shared (read-only)."""
    done = {}

    def both(name, weighted, eps):
        if (name, weighted, eps) not in done:
            h = mc.circuit(ek, name, weighted)
            done[name, weighted, eps] = (h, ctx.multilevel_bipartition(h, eps, COARSE[name]),
                                         compose(ek, ctx, h, eps, COARSE[name]))
        return done[name, weighted, eps]
    yield both
    done.clear()


@pytest.mark.parametrize("name, weighted, eps", CONFIGS)
def test_driver_equals_composition(runs, name, weighted, eps):
    _, (side, res), (want_side, want) = runs(name, weighted, eps)
    for k in LEVEL_FIELDS + INTS:
        assert res[k] == want[k], k
    assert np.array_equal(side, want_side)
    print(f"{name} weighted={weighted} eps={eps}: levels {res['levels']}, nodes {res['nodes']}, max_cluster "
          f"{res['max_cluster']}, cut per level {list(zip(res['cut_before'], res['cut_after']))}, final {res['cut']}")


@pytest.mark.parametrize("name, weighted, eps", CONFIGS)
def test_metrics_balance_monotone(ek, runs, name, weighted, eps):
    h, (side, res), _ = runs(name, weighted, eps)
    assert set(np.unique(side).tolist()) <= {0, 1}
    assert ek.bipart_metrics_host(h, side) == (res["cut"], res["cut_nets"], res["w0"], res["w1"])
    assert (res["n0"], res["n1"]) == (h.nodes - int(side.sum()), int(side.sum()))
    assert res["w0"] + res["w1"] == res["total_weight"] and res["max_part"] == max_part(res["total_weight"], eps)
    if res["sweep_feasible"] == 1:  # FM never moves a node across the bound, and projection keeps the weights
        assert max(res["w0"], res["w1"]) <= res["max_part"]
    L = res["levels"]
    assert L >= 1 and all(len(res[k]) == L + 1 for k in LEVEL_FIELDS)
    assert res["nodes"][0] == h.nodes and res["nodes"][L] <= res["nodes"][L - 1] * 9 // 10
    for l in range(L + 1):
        assert res["cut_after"][l] <= res["cut_before"][l]  # FM keeps a prefix only when it lowers (cut, |S0 - S1|)
        if l < L:
            assert res["cut_before"][l] == res["cut_after"][l + 1]  # projection preserves the weighted cut
            assert res["nodes"][l] - res["nodes"][l + 1] == res["match_pairs"][l]
    assert res["cut"] == res["cut_after"][0]


def test_no_slack_means_no_level(ek, ctx):
    """ibm01, unit weights, eps = 0: W = 12,752 is even, so 2 L_max - W + 1 = 1, no pair fits under the cap, the
    first matching shrinks nothing, and the driver is the flat path (Lanczos, weighted sweep, FM) on the input."""
    h = mc.circuit(ek, "ibm01", False)
    side, res = ctx.multilevel_bipartition(h, 0.0)
    want_side, want = compose(ek, ctx, h, 0.0, 512)
    assert res["levels"] == 0 and res["max_cluster"] == 1 and res["nodes"] == [h.nodes]
    assert all(res[k] == want[k] for k in LEVEL_FIELDS + INTS) and np.array_equal(side, want_side)
    ctx.spmv_setup_pins(h)
    _, v, _ = ctx.lanczos_fiedler()
    flat, _, _, _ = ctx.sweep_cut_w(h, v, 0.0)
    assert res["cut_before"] == [flat["cut"]] and res["w0"] == res["w1"] == h.nodes // 2


def test_two_runs_give_the_same_bytes(ek, ctx):
    h = mc.circuit(ek, "fract", True)
    a, ra = ctx.multilevel_bipartition(h, 0.03, 16)
    b, rb = ctx.multilevel_bipartition(h, 0.03, 16)
    assert a.tobytes() == b.tobytes() and all(ra[k] == rb[k] for k in LEVEL_FIELDS + INTS)


def test_state_and_argument_errors(ek):
    h = mc.circuit(ek, "fract", False)
    one = ek.Context(0)
    try:
        for eps in (-0.5, float("nan")):
            with pytest.raises(ek.EKError) as e:
                one.multilevel_bipartition(h, eps)
            assert e.value.code == ek.EK_EINVAL

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:  # a multi-rank context
            one.multilevel_bipartition(h)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


ML_KEYS = "levels|coarsest_nodes|max_cluster|fallback|feasible|coarsest_cut|cut|cut_nets|w0|w1|total_weight|max_part|n0|n1"


def test_cli_multilevel(ek, ctx, tmp_path):
    h = mc.circuit(ek, "ibm01", True)
    src = tmp_path / "ibm01w.hgr"
    h.write(src)  # fmt 11
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), str(src), "-EIG", "--multilevel", "0.03",
                        "--ml-coarse", "256", "--fm-stall", "500"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ml:")]
    assert len(line) == 1, r.stdout
    got = {k: int(v) for k, v in re.findall(rf"\b({ML_KEYS}) (-?\d+)", line[0])}
    assert len(got) == 14
    part = np.array((tmp_path / "results" / "ibm01w.hgr.part.2").read_text().split(), np.uint8)
    assert ek.bipart_metrics_host(h, part) == (got["cut"], got["cut_nets"], got["w0"], got["w1"])
    assert (got["n0"], got["n1"]) == (h.nodes - int(part.sum()), int(part.sum()))
    side, res = ctx.multilevel_bipartition(h, 0.03, 256, stall=500)  # the library, with the CLI's options
    assert np.array_equal(part, side)
    L = res["levels"]
    assert got == {"levels": L, "coarsest_nodes": res["nodes"][L], "max_cluster": res["max_cluster"],
                   "fallback": res["coarsest_fallback"], "feasible": res["sweep_feasible"],
                   "coarsest_cut": res["cut_before"][L], **{k: res[k] for k in ("cut", "cut_nets", "w0", "w1",
                                                                                "total_weight", "max_part", "n0", "n1")}}
    side2, _ = ctx.multilevel_bipartition_file(str(src), 0.03, 256, out_dir=str(tmp_path / "lib"), stall=500)
    assert np.array_equal(side2, side)
    assert (tmp_path / "lib" / "results" / "ibm01w.hgr.part.2").read_text() == \
           (tmp_path / "results" / "ibm01w.hgr.part.2").read_text()
