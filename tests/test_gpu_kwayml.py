"""The k-way multilevel path on the GPU.  The bounded sweep and
FM: device = host bit for bit on the case lists of the weighted tests, under
the symmetric and the unequal bounds.  ek_kway_metrics_w against its host
checker.  ek_multilevel_bipartition_b against ek_multilevel_bipartition_ex
(symmetric bound) and against the V-cycle composed from the host checkers
(2 : 1).  ek_partition_kway_ml against the recursion composed from
Hypergraph.induce, ek_kway_bisect_bounds and ek_multilevel_bipartition_b."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fmw_cases as fw
import kwayml_cases as kc
import match_cases as mc
import sweepw_cases as sw
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu

COARSE = {"fract": 16, "ibm01": 512}
LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "cut_before", "cut_after", "fm_moves")
ML_INTS = ("levels", "coarsest_fallback", "sweep_feasible", "max_cluster", "total_weight", "max_part", "cut", "cut_nets",
           "w0", "w1", "n0", "n1")
KWAY_INTS = ("k", "bisections", "coarsest_fallbacks", "infeasible_sweeps", "total_weight", "part_bound", "part_w_min",
             "part_w_max", "parts_over_bound", "empty_parts", "cut_nets", "connectivity", "connectivity_w", "soed",
             "levels_total", "fm_moves")
KS = (2, 3, 4, 5, 8)
KWAY_CONFIGS = [(name, weighted, eps) for name in ("fract", "ibm01") for weighted in (False, True) for eps in (0.03, 0.10)]


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------
# the bounded sweep and FM
def sweep_bounds(name):
    nodes, _, _, node_w, _, _, epsilons = sw.cases()[name]
    W = kc.total_weight(nodes, node_w)
    return [kc.symmetric(W, eps) for eps in epsilons] + kc.all_bounds(W)


@pytest.mark.parametrize("name", sw.names())
def test_sweep_device_equals_host(ek, ctx, name):
    """The case list of test_gpu_sweepw.py (the scans' block edges at n + 1 = 2,047 | 2,048 | 2,049 words, nets of
    8 | 9 and 64 | 65 pins, the contended difference words, no feasible split), every case under its symmetric
    bounds and under 2 : 1 and 3 : 2 at eps 0 and 0.03."""
    h, v, _ = sw.hypergraph(ek, name)
    for bounds in dict.fromkeys(sweep_bounds(name)):
        kc.same_sweep(ctx.sweep_cut_wb(h, v, bounds), ek.sweep_cut_wb_host(h, v, bounds))


def test_sweep_select_blocks_and_scan_second_step(ek, ctx):
    """n = 524,288: 512 select blocks of 1,024 splits and the scans' second top step, under 2 : 1 bounds."""
    n, ptr, pins, node_w, net_w, v = sw.big_case()
    h = ek.Hypergraph.from_pins(n, ptr, pins)
    h.set_weights(node_w, net_w)
    bounds = kc.ratio_bounds(int(node_w.sum()), (2, 1), 0.03)
    got = ctx.sweep_cut_wb(h, v, bounds)
    kc.same_sweep(got, ek.sweep_cut_wb_host(h, v, bounds))
    assert got[0]["feasible"] == 1 and got[0]["w0"] <= bounds[0] and got[0]["w1"] <= bounds[1]


@pytest.mark.parametrize("name", fw.names())
def test_fm_device_equals_host(ek, ctx, name):
    """The case list of test_gpu_fmw.py (n = C - 1 | C | C + 1 | 2 C + 1, the hub, the keys in LDS and in global
    memory, a start above the bound, stall and pass limits), every case under its symmetric bounds and under 2 : 1
    and 3 : 2; the two half-million-node key cases under the symmetric bounds and 2 : 1 at eps 0.03 only."""
    h, (side, eps, max_passes, stall) = fw.hypergraph(ek, name)
    W = kc.total_weight(h.nodes, h.weights()[0])
    unequal = [kc.ratio_bounds(W, (2, 1), 0.03)] if name.startswith("keys_") else kc.all_bounds(W)
    for bounds in dict.fromkeys([kc.symmetric(W, eps)] + unequal):
        kc.same_fm(ctx.fm_refine_wb(h, side, bounds, max_passes, stall),
                   ek.fm_refine_wb_host(h, side, bounds, max_passes, stall))


def test_symmetric_bounds_are_the_weighted_entries(ek, ctx):
    for name in ("random+all", "heavy_node", "n2049"):
        h, v, epsilons = sw.hypergraph(ek, name)
        W = kc.total_weight(h.nodes, h.weights()[0])
        a, b = ctx.sweep_cut_wb(h, v, kc.symmetric(W, epsilons[0])), ctx.sweep_cut_w(h, v, epsilons[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))
        assert all(a[0][k] == b[0][k] for k in sw.INTS if k != "max_part")
    for name in ("n513", "heavy", "tie_heavier_side", "hub"):
        h, (side, eps, max_passes, stall) = fw.hypergraph(ek, name)
        W = kc.total_weight(h.nodes, h.weights()[0])
        a = ctx.fm_refine_wb(h, side, kc.symmetric(W, eps), max_passes, stall)
        b = ctx.fm_refine_w(h, side, eps, max_passes, stall)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
        assert all(a[3][k] == b[3][k] for k in fw.RESULT_INTS if k != "max_part")


def test_bounded_entries_refuse_bad_bounds_and_multirank(ek, ctx):
    h, v, _ = sw.hypergraph(ek, "window_of_one")  # W = 8
    hf, (side, *_) = fw.hypergraph(ek, "n3")  # W = 3
    for bounds in ((-1, 8), (9, 4), (3, 4)):
        with pytest.raises(ek.EKError) as e:
            ctx.sweep_cut_wb(h, v, bounds)
        assert e.value.code == ek.EK_EINVAL
    for bounds in ((4, 1), (1, 1)):
        with pytest.raises(ek.EKError) as e:
            ctx.fm_refine_wb(hf, side, bounds)
        assert e.value.code == ek.EK_EINVAL
        with pytest.raises(ek.EKError) as e:
            ctx.multilevel_bipartition_b(hf, bounds)
        assert e.value.code == ek.EK_EINVAL
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        for call in (lambda: one.fm_refine_wb(hf, side, (3, 3)), lambda: one.multilevel_bipartition_b(hf, (3, 3)),
                     lambda: one.partition_kway_ml(hf, 2)):
            with pytest.raises(ek.EKError) as e:
                call()
            assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


# ---------------------------------------------------------------------------
# the weighted k-way metrics
@pytest.mark.parametrize("k", [2, 64, 65, 256])
def test_kway_metrics_w_equals_host(ek, ctx, k):
    nodes, ptr, pins, node_w, net_w = kc.metrics_hypergraph()
    assert {8, 9, 64, 65} <= set(np.diff(ptr).tolist())
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    part = np.random.default_rng(k).integers(0, k, nodes).astype(np.int32)
    for weights in ((None, None), (node_w, net_w), (node_w, None), (None, net_w)):
        h.set_weights(*weights)
        m, pw = ctx.kway_metrics_w(h, part, k)
        wm, wpw = ek.kway_metrics_w_host(h, part, k)
        assert m == wm and pw.tobytes() == wpw.tobytes()
    h.set_weights(None, None)
    assert (m[0], m[1], m[3]) == ctx.kway_metrics(ptr, pins, part, k)


# ---------------------------------------------------------------------------
# the V-cycle under bounds
@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("weighted", [False, True])
def test_ml_b_at_the_symmetric_bound_is_ml_ex(ek, ctx, name, weighted):
    h = mc.circuit(ek, name, weighted)
    W = kc.total_weight(h.nodes, h.weights()[0])
    for eps, wlap in ((0.03, False), (0.10, True)):
        want_side, want = ctx.multilevel_bipartition(h, eps, COARSE[name], weighted_laplacian=wlap)
        side, res = ctx.multilevel_bipartition_b(h, kc.symmetric(W, eps), COARSE[name], weighted_laplacian=wlap)
        assert side.tobytes() == want_side.tobytes()
        assert all(res[k] == want[k] for k in LEVEL_FIELDS + ML_INTS)


def compose_b(ek, ctx, h, bounds, coarse_nodes):
    """(side, result dict) of the bounded V-cycle as eigkl.h states it, from the host checkers and the context's
    Lanczos: test_gpu_multilevel.py's composition with the bounded sweep and FM."""
    node_w = h.weights()[0]
    W = kc.total_weight(h.nodes, node_w)
    cap = max(1, min(bounds[0] + bounds[1] - W + 1, -(-4 * W // coarse_nodes)))
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
    sweep, _, _, _ = ek.sweep_cut_wb_host(cur, v, bounds)
    side = ek.rank_split(v, sweep["n1"])
    before, after, moves = [], [], []
    for l in range(len(levels) - 1, -1, -1):
        if l < len(levels) - 1:
            side = side[clusters[l]]
        side, _, _, fm = ek.fm_refine_wb_host(levels[l], side, bounds)
        before.insert(0, fm["cut_before"])
        after.insert(0, fm["cut"])
        moves.insert(0, fm["moves_kept"])
    res.update(cut_before=before, cut_after=after, fm_moves=moves, levels=len(clusters),
               coarsest_fallback=0 if spectral else 1, sweep_feasible=sweep["feasible"], max_cluster=cap, total_weight=W,
               max_part=max(bounds))
    cut, cut_nets, w0, w1 = ek.bipart_metrics_host(h, side)
    n1 = int(side.sum())
    res.update(cut=cut, cut_nets=cut_nets, w0=w0, w1=w1, n0=h.nodes - n1, n1=n1)
    return side, res


@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("weighted", [False, True])
def test_ml_b_at_two_to_one_is_the_composition(ek, ctx, name, weighted):
    h = mc.circuit(ek, name, weighted)
    bounds = kc.ratio_bounds(kc.total_weight(h.nodes, h.weights()[0]), (2, 1), 0.03)
    side, res = ctx.multilevel_bipartition_b(h, bounds, COARSE[name])
    want_side, want = compose_b(ek, ctx, h, bounds, COARSE[name])
    for k in LEVEL_FIELDS + ML_INTS:
        assert res[k] == want[k], k
    assert side.tobytes() == want_side.tobytes()
    if res["sweep_feasible"]:
        assert res["w0"] <= bounds[0] and res["w1"] <= bounds[1]
    print(f"{name} weighted={weighted} bounds={bounds}: levels {res['levels']}, w {res['w0']} | {res['w1']}, cut {res['cut']}")


# ---------------------------------------------------------------------------
# the k-way driver
def kway_mult(k, eps):
    depth = max(1, (k - 1).bit_length())
    return 1.0 + eps if depth == 1 else (1.0 + eps) ** (1.0 / depth)


def compose_kway(ek, ctx, h, k, eps, coarse_nodes):
    """part of the recursion as eigkl.h states it: depth first, side 0 first, Hypergraph.induce,
    ek_kway_bisect_bounds (again without the part cap where a block outweighs it), ek_multilevel_bipartition_b."""
    W = kc.total_weight(h.nodes, h.weights()[0])
    Lk = math.floor((1.0 + eps) * float(-(-W // k)))
    mult = kway_mult(k, eps)
    part = np.full(h.nodes, -1, np.int32)
    count = {"bisections": 0, "coarsest_fallbacks": 0, "infeasible_sweeps": 0, "levels_total": 0, "fm_moves": 0}

    def bisect(g, ids, kb, base):
        if kb == 1 or g.nodes < 2:
            part[ids] = base
            return
        Wb = kc.total_weight(g.nodes, g.weights()[0])
        bounds = ek.kway_bisect_bounds(Wb, kb, Lk, mult)
        if sum(bounds) < Wb:
            bounds = ek.kway_bisect_bounds(Wb, kb, Wb, mult)
        side, res = ctx.multilevel_bipartition_b(g, bounds, coarse_nodes)
        count["bisections"] += 1
        count["coarsest_fallbacks"] += res["coarsest_fallback"]
        count["infeasible_sweeps"] += 0 if res["sweep_feasible"] else 1
        count["levels_total"] += res["levels"]
        count["fm_moves"] += sum(res["fm_moves"])
        k0 = (kb + 1) // 2
        for s, ks, bs in ((0, k0, base), (1, kb // 2, base + k0)):
            keep = side == s
            if ks == 1 or int(keep.sum()) < 2:
                part[ids[keep]] = bs
            else:
                bisect(g.induce(keep.astype(np.uint8))[0], ids[keep], ks, bs)
    bisect(h, np.arange(h.nodes), k, 0)
    return part, count, W, Lk


@pytest.fixture(scope="module")
def kway_runs(ek, ctx):
    """run(name, weighted, eps, k) -> (hypergraph, the driver's (part, result)), computed once and shared."""
    done = {}

    def run(name, weighted, eps, k):
        key = (name, weighted, eps, k)
        if key not in done:
            h = mc.circuit(ek, name, weighted)
            done[key] = (h, ctx.partition_kway_ml(h, k, eps, COARSE[name]))
        return done[key]
    yield run
    done.clear()


@pytest.mark.parametrize("name, weighted, eps", KWAY_CONFIGS)
def test_kway_ml_equals_composition_and_metrics(ek, ctx, kway_runs, name, weighted, eps):
    for k in KS:
        h, (part, res) = kway_runs(name, weighted, eps, k)
        want, count, W, Lk = compose_kway(ek, ctx, h, k, eps, COARSE[name])
        assert part.tobytes() == want.tobytes(), k
        (cut, conn, connw, soed), pw = ek.kway_metrics_w_host(h, part, k)
        sizes = np.bincount(part, minlength=k)
        assert {f: res[f] for f in KWAY_INTS} == {
            "k": k, **count, "total_weight": W, "part_bound": Lk, "part_w_min": int(pw.min()),
            "part_w_max": int(pw.max()), "parts_over_bound": int((pw > Lk).sum()), "empty_parts": int((sizes == 0).sum()),
            "cut_nets": cut, "connectivity": conn, "connectivity_w": connw, "soed": soed}, k
        if not weighted:  # the derived guarantee: unit weights keep every part within Lk
            assert res["parts_over_bound"] == 0 and res["part_w_max"] <= res["part_bound"]
            assert res["infeasible_sweeps"] == 0
        print(f"{name} weighted={weighted} eps={eps} k={k}: part weights {res['part_w_min']}..{res['part_w_max']} (bound "
              f"{Lk}), over {res['parts_over_bound']}, connectivity {conn}, cut nets {cut}")


@pytest.mark.parametrize("name, weighted, eps", KWAY_CONFIGS)
def test_kway_ml_at_k2_is_the_multilevel_bipartition(ek, ctx, kway_runs, name, weighted, eps):
    h, (part, res) = kway_runs(name, weighted, eps, 2)
    side, ml = ctx.multilevel_bipartition(h, eps, COARSE[name])
    assert part.astype(np.uint8).tobytes() == side.tobytes()
    assert (res["bisections"], res["levels_total"], res["fm_moves"]) == (1, ml["levels"], sum(ml["fm_moves"]))
    assert (res["cut_nets"], res["connectivity_w"]) == (ml["cut_nets"], ml["cut"])


def test_kway_ml_two_runs_give_the_same_bytes(ek, ctx, kway_runs):
    for name, k in (("fract", 5), ("ibm01", 8)):
        h, (part, res) = kway_runs(name, True, 0.03, k)
        again, res2 = ctx.partition_kway_ml(h, k, 0.03, COARSE[name])
        assert part.tobytes() == again.tobytes() and all(res[f] == res2[f] for f in KWAY_INTS)


def test_kway_ml_leaves_no_state_behind(ek, ctx):
    ibm01 = circuit_path("ibm01")
    ctx.partition_kway_ml(mc.circuit(ek, "ibm01", True), 3, 0.03)
    res, log = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    assert res["kl"]["net_cut_best"] == 367  # its usual result (the smoke test's)
    fresh = ek.Context(0)
    try:
        res0, log0 = fresh.solve_file(ibm01, write_results=False, log_cap=8192)
    finally:
        fresh.close()
    swap_fields_equal(log, log0)
    assert res["kl"]["net_cut_best"] == res0["kl"]["net_cut_best"] and res["lambda"] == res0["lambda"]


def test_kway_ml_argument_errors(ek, ctx):
    h = mc.circuit(ek, "fract", False)
    for k, eps in ((1, 0.03), (257, 0.03), (4, -0.5), (4, float("nan"))):
        with pytest.raises(ek.EKError) as e:
            ctx.partition_kway_ml(h, k, eps)
        assert e.value.code == ek.EK_EINVAL


KWAY_KEYS = ("k|bisections|fallbacks|infeasible|total_weight|part_bound|over_bound|empty|cut nets|connectivity|"
             "connectivity_w|SOED|levels|fm_moves")


def test_cli_kway_multilevel(ek, ctx, tmp_path):
    h = mc.circuit(ek, "ibm01", True)
    src = tmp_path / "ibm01w.hgr"
    h.write(src)  # fmt 11
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), str(src), "-EIG", "--k", "5", "--kway-multilevel", "0.03",
                        "--ml-coarse", "256"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("k-way-ml:")]
    assert len(line) == 1, r.stdout
    got = {k: int(v) for k, v in re.findall(rf"\b({KWAY_KEYS}) (-?\d+)", line[0])}
    lo, hi = (int(x) for x in re.search(r"part weights (\d+)\.\.(\d+)", line[0]).groups())
    part = np.array((tmp_path / "results" / "ibm01w.hgr.part.5").read_text().split(), np.int32)
    want, res = ctx.partition_kway_ml(h, 5, 0.03, 256)  # the library, with the CLI's options
    assert part.tobytes() == want.tobytes()
    assert got == {"k": 5, "bisections": res["bisections"], "fallbacks": res["coarsest_fallbacks"],
                   "infeasible": res["infeasible_sweeps"], "total_weight": res["total_weight"],
                   "part_bound": res["part_bound"], "over_bound": res["parts_over_bound"], "empty": res["empty_parts"],
                   "cut nets": res["cut_nets"], "connectivity": res["connectivity"],
                   "connectivity_w": res["connectivity_w"], "SOED": res["soed"], "levels": res["levels_total"],
                   "fm_moves": res["fm_moves"]}
    assert (lo, hi) == (res["part_w_min"], res["part_w_max"])
    part2, _ = ctx.partition_kway_ml_file(str(src), 5, 0.03, 256, out_dir=str(tmp_path / "lib"))
    assert part2.tobytes() == want.tobytes()
    assert (tmp_path / "lib" / "results" / "ibm01w.hgr.part.5").read_text() == \
           (tmp_path / "results" / "ibm01w.hgr.part.5").read_text()
