"""The host side of the k-way multilevel path: the new symbols
and structs, ek_kway_bisect_bounds, the bounded sweep and FM checkers against
the symmetric entries and against the rules restated in kwayml_cases, and
ek_kway_metrics_w_host.  No GPU."""
import ctypes
import math

import numpy as np
import pytest

import fmw_cases as fw
import kwayml_cases as kc
import sweepw_cases as sw

SMALL = 300  # nodes up to which the Python restatements run (they recompute everything at every step)


def test_symbols_structs_defaults(ek):
    for name in ("ek_sweep_cut_wb_host", "ek_sweep_cut_wb", "ek_fm_refine_wb_host", "ek_fm_refine_wb",
                 "ek_multilevel_bipartition_b", "ek_kway_bisect_bounds", "ek_kway_metrics_w_host", "ek_kway_metrics_w",
                 "ek_kway_ml_default_opts", "ek_partition_kway_ml", "ek_partition_kway_ml_file"):
        assert hasattr(ek.lib, name), name
    assert ek.lib.ek_abi_version() == 4  # no struct of the earlier entries changed
    assert ctypes.sizeof(ek.SweepWBResult) == ctypes.sizeof(ek.SweepWResult) + 8 == 15 * 8 + 3 * 8
    assert ctypes.sizeof(ek.FmWBResult) == ctypes.sizeof(ek.FmWResult) + 8 == 4 * 8 + 2 * 4 + 10 * 8 + 3 * 8
    assert ctypes.sizeof(ek.KwayMlOpts) == 32 + ctypes.sizeof(ek.MlOpts)
    assert ctypes.sizeof(ek.KwayMlResult) == 4 * 4 + 12 * 8 + 9 * 8 + ek.KWAY_LEVELS * 8
    o = ek.KwayMlOpts()
    ctypes.memset(ctypes.byref(o), 0xFF, ctypes.sizeof(o))
    ek.lib.ek_kway_ml_default_opts(ctypes.byref(o))
    assert (o.k, o.flags, o.imbalance, o.write_results, o.out_dir) == (2, 0, 0.03, 0, None)
    m = ek.MlOpts()
    ek.lib.ek_ml_default_opts(ctypes.byref(m))
    assert bytes(o.ml) == bytes(m) and o.ml.coarse_nodes == 512


@pytest.mark.parametrize("k", [2, 3, 5, 8, 256])
def test_bisect_bounds(ek, k):
    rng = np.random.default_rng(k)
    for W in [0, 1, 2, 3, 7, 100, 12752, 2 ** 40 + 3] + rng.integers(1, 10 ** 6, 20).tolist():
        for eps in (0.0, 0.03, 0.10):
            Lk = math.floor((1.0 + eps) * float(-(-W // k)))
            depth = max(1, (k - 1).bit_length())
            mult = 1.0 + eps if depth == 1 else (1.0 + eps) ** (1.0 / depth)
            # down the recursion: every block within kb Lk gets jointly satisfiable bounds, and a side within its
            # bound is such a block again
            blocks = [(W, k)]
            while blocks:
                Wb, kb = blocks.pop()
                if kb < 2:
                    continue
                L0, L1 = ek.kway_bisect_bounds(Wb, kb, Lk, mult)
                k0, k1 = (kb + 1) // 2, kb // 2
                for L, ks in ((L0, k0), (L1, k1)):
                    assert L == min(Wb, ks * Lk, math.floor(mult * float(-(-Wb * ks // kb))))
                assert Wb <= kb * Lk and L0 + L1 >= Wb and 0 <= L0 <= Wb and 0 <= L1 <= Wb
                assert L0 <= k0 * Lk and L1 <= k1 * Lk
                if kb > 3 and len(blocks) < 64:  # the heaviest sides the bounds allow
                    blocks += [(L0, k0), (L1, k1)]


def test_bisect_bounds_at_k2_is_the_bipartition_bound(ek):
    for W in (2, 9, 149, 12752, 38207, 10 ** 9 + 7):
        for eps in (0.0, 0.03, 0.10):
            lmax = math.floor((1.0 + eps) * float((W + 1) // 2))  # refine_max_part(W, 2, eps)
            assert ek.kway_bisect_bounds(W, 2, lmax, 1.0 + eps) == (min(W, lmax), min(W, lmax))


def test_bisect_bounds_einval(ek):
    for args in ((-1, 2, 5, 1.0), (10, 1, 5, 1.0), (10, 257, 5, 1.0), (10, 2, -1, 1.0), (10, 2, 5, 0.5),
                 (10, 2, 5, float("nan")), (10, 2, 5, float("inf")), (2 ** 61 + 1, 2, 5, 1.0)):
        with pytest.raises(ek.EKError) as e:
            ek.kway_bisect_bounds(*args)
        assert e.value.code == ek.EK_EINVAL, args
    assert ek.lib.ek_kway_bisect_bounds(10, 2, 5, 1.0, None) == ek.EK_EINVAL


@pytest.mark.parametrize("name", sw.names())
def test_sweep_symmetric_bound_is_the_weighted_sweep(ek, name):
    h, v, epsilons = sw.hypergraph(ek, name)
    W = kc.total_weight(h.nodes, h.weights()[0])
    for eps in epsilons:
        want, worder, wprofw, wprefix = ek.sweep_cut_w_host(h, v, eps)
        res, order, profw, prefix = ek.sweep_cut_wb_host(h, v, kc.symmetric(W, eps))
        assert order.tobytes() == worder.tobytes() and profw.tobytes() == wprofw.tobytes()
        assert prefix.tobytes() == wprefix.tobytes()
        assert all(res[k] == want[k] for k in sw.INTS if k != "max_part")
        assert res["bound0"] == res["bound1"] == min(W, want["max_part"])


@pytest.mark.parametrize("name", fw.names())
def test_fm_symmetric_bound_is_the_weighted_fm(ek, name):
    h, (side, eps, max_passes, stall) = fw.hypergraph(ek, name)
    W = kc.total_weight(h.nodes, h.weights()[0])
    want = ek.fm_refine_w_host(h, side, eps, max_passes, stall)
    got = ek.fm_refine_wb_host(h, side, kc.symmetric(W, eps), max_passes, stall)
    for a, b in zip(got[:3], want[:3]):
        assert a.tobytes() == b.tobytes()
    assert all(got[3][k] == want[3][k] for k in fw.RESULT_INTS if k != "max_part")
    assert got[3]["bound0"] == got[3]["bound1"] == min(W, want[3]["max_part"])


@pytest.mark.parametrize("name", [x for x in sw.names() if sw.cases()[x][0] <= SMALL])
def test_sweep_unequal_bounds_follow_the_rule(ek, name):
    nodes, ptr, pins, node_w, net_w, v, _ = sw.cases()[name]
    h, _, _ = sw.hypergraph(ek, name)
    for bounds in kc.all_bounds(kc.total_weight(nodes, node_w)):
        kc.same_sweep(ek.sweep_cut_wb_host(h, v, bounds), kc.sweepwb_ref(nodes, ptr, pins, node_w, net_w, v, bounds))


@pytest.mark.parametrize("name", [x for x in fw.names() if fw.cases()[x][0] <= SMALL])
def test_fm_unequal_bounds_follow_the_rule(ek, name):
    nodes, ptr, pins, node_w, net_w, side, _, max_passes, stall = fw.cases()[name]
    h, _ = fw.hypergraph(ek, name)
    for bounds in kc.all_bounds(kc.total_weight(nodes, node_w)):
        kc.same_fm(ek.fm_refine_wb_host(h, side, bounds, max_passes, stall),
                   kc.fmwb_ref(nodes, ptr, pins, node_w, net_w, side, bounds, max_passes, stall))


def test_sweep_without_a_feasible_split(ek):
    """heavy_node: one node of weight 100 in W = 106; under 2 : 1 bounds (71, 36) neither side can hold it, so the
    fallback picks the split of the least slack difference."""
    nodes, ptr, pins, node_w, net_w, v, _ = sw.cases()["heavy_node"]
    h, _, _ = sw.hypergraph(ek, "heavy_node")
    bounds = kc.ratio_bounds(106, (2, 1), 0.0)
    assert bounds == (71, 36)
    got = ek.sweep_cut_wb_host(h, v, bounds)
    kc.same_sweep(got, kc.sweepwb_ref(nodes, ptr, pins, node_w, net_w, v, bounds))
    assert (got[0]["feasible"], got[0]["s_lo"], got[0]["s_hi"]) == (0, 0, 0)
    # ... and the unequal window is not the symmetric one shifted: v = 0.1 .. 0.5 ascending, side 1 = the low ranks
    ptr2, pins2 = sw.pack([[0, 1], [1, 2], [2, 3], [0, 3]])
    h2 = ek.Hypergraph.from_pins(4, ptr2, pins2)
    h2.set_weights(np.array([3, 1, 2, 2], np.int32), None)
    res, _, _, prefix = ek.sweep_cut_wb_host(h2, np.arange(4.0), (5, 3))  # P = 0 3 4 6 8: only s = 1 has P <= 3, W - P <= 5
    assert prefix.tolist() == [0, 3, 4, 6, 8] and (res["feasible"], res["s_lo"], res["s_hi"], res["n1"]) == (1, 1, 1, 1)
    res, _, _, _ = ek.sweep_cut_wb_host(h2, np.arange(4.0), (3, 5))  # mirrored: W - P <= 3 needs P >= 5, P <= 5: none
    assert res["feasible"] == 0 and res["n1"] == 2  # D = |10 - 2 P|: 2 at P = 4 and at P = 6, both cut 2 nets: the lesser s


def test_fm_start_above_one_bound(ek):
    """Everything starts on side 1 (S1 = W > L1): side 1 never receives, side 0 takes nodes until L0 is full."""
    rng = np.random.default_rng(3)
    n = 40
    nets = [rng.choice(n, int(rng.integers(2, 5)), replace=False).tolist() for _ in range(70)]
    ptr, pins = sw.pack(nets)
    node_w = rng.integers(1, 5, n).astype(np.int32)
    net_w = rng.integers(1, 6, len(nets)).astype(np.int32)
    side = np.ones(n, np.uint8)
    side[:3] = 0
    h = ek.Hypergraph.from_pins(n, ptr, pins)
    h.set_weights(node_w, net_w)
    W = int(node_w.sum())
    bounds = kc.ratio_bounds(W, (2, 1), 0.03)
    assert W - int(node_w[:3].sum()) > bounds[1]
    got = ek.fm_refine_wb_host(h, side, bounds, 0, 0)
    kc.same_fm(got, kc.fmwb_ref(n, ptr, pins, node_w, net_w, side, bounds, 0, 0))
    assert got[3]["moves_tried"] > 0 and side[int(got[2][0]["node"])] == 1  # side 0's top has nowhere to go
    assert got[3]["w0"] <= bounds[0]


def test_fm_equal_gains_go_to_the_side_of_less_slack(ek):
    """One net {0, 1} of weight 2, node 1 on side 0, node 0 on side 1, nodes 2 and 3 (weight 3, on no net) one a
    side: both candidates have g = 2 and S = 4 | 4, W = 8.  Under one bound the weights tie and the smaller id, node
    0, moves.  Under (5, 6) side 0 has less slack (-1 against -2), so its node 1 moves first; under (6, 5) side 1
    has, so node 0; under (5, 5) the slacks tie and the smaller id moves."""
    ptr, pins = sw.pack([[0, 1]])
    h = ek.Hypergraph.from_pins(4, ptr, pins)
    node_w, net_w = np.array([1, 1, 3, 3], np.int32), np.array([2], np.int32)
    h.set_weights(node_w, net_w)
    side = np.array([1, 0, 0, 1], np.uint8)
    first = lambda run: int(run[2][0]["node"])
    assert first(ek.fm_refine_w_host(h, side, 1.0)) == 0
    for bounds, node in (((5, 6), 1), ((6, 5), 0), ((5, 5), 0), ((8, 8), 0)):
        got = ek.fm_refine_wb_host(h, side, bounds)
        kc.same_fm(got, kc.fmwb_ref(4, ptr, pins, node_w, net_w, side, bounds))
        assert got[2][0]["gain"] == 2 and first(got) == node, bounds


def test_bounds_einval(ek):
    h, v, _ = sw.hypergraph(ek, "window_of_one")  # W = 8
    hf, (side, *_) = fw.hypergraph(ek, "n3")  # W = 3
    for bounds in ((-1, 8), (9, 4), (4, 9), (3, 4)):
        with pytest.raises(ek.EKError) as e:
            ek.sweep_cut_wb_host(h, v, bounds)
        assert e.value.code == ek.EK_EINVAL, bounds
    for bounds in ((-1, 3), (4, 1), (1, 1)):
        with pytest.raises(ek.EKError) as e:
            ek.fm_refine_wb_host(hf, side, bounds)
        assert e.value.code == ek.EK_EINVAL, bounds
    o = ek.SweepOpts()
    ek.lib.ek_sweep_default_opts(ctypes.byref(o))
    o.objective = 1  # no ratio objective under weights
    b = np.array([8, 8], np.int64)
    assert ek.lib.ek_sweep_cut_wb_host(h._h, v.ctypes.data, ctypes.byref(o), b.ctypes.data, None, None, None,
                                       None) == ek.EK_EINVAL
    o.objective, o.imbalance = 0, -5.0  # the imbalance is ignored
    assert ek.lib.ek_sweep_cut_wb_host(h._h, v.ctypes.data, ctypes.byref(o), b.ctypes.data, None, None, None,
                                       None) == ek.EK_OK


@pytest.mark.parametrize("k", [1, 2, 3, 64, 65, 256])
def test_kway_metrics_w_host(ek, k):
    nodes, ptr, pins, node_w, net_w = kc.metrics_hypergraph()
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    part = np.random.default_rng(k).integers(0, k, nodes).astype(np.int32)
    # unit weights: cut nets, connectivity and SOED are ek_kway_metrics_host's
    m, pw = ek.kway_metrics_w_host(h, part, k)
    assert (m[0], m[1], m[3]) == ek.kway_metrics_host(ptr, pins, part, k) and m[2] == m[1]
    assert pw.tolist() == np.bincount(part, minlength=k).tolist()
    h.set_weights(node_w, net_w)
    m, pw = ek.kway_metrics_w_host(h, part, k)
    want, wpw = kc.kway_metrics_w_ref(nodes, ptr, pins, node_w, net_w, part, k)
    assert m == want and pw.tolist() == wpw
    bad = part.copy()
    bad[11] = k
    with pytest.raises(ek.EKError) as e:
        ek.kway_metrics_w_host(h, bad, k)
    assert e.value.code == ek.EK_EINVAL


def test_kway_multilevel_cli_misuse_prints_usage(tmp_path):
    """Refused while the arguments are read: no GPU work.  --multilevel keeps refusing --k; the k-way driver has a
    switch of its own, which needs --k in 2..256 and excludes --multilevel and --refine."""
    import os
    import subprocess

    from conftest import PKG_DIR, circuit_path
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    for args in (("-EIG", "--kway-multilevel", "0.03"), ("--k", "4", "--kway-multilevel", "0.03"),
                 ("-EIG", "--k", "300", "--kway-multilevel", "0.03"), ("-EIG", "--k", "4", "--kway-multilevel", "-1"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine", "0.05"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--multilevel", "0.03"),
                 ("-EIG", "--k", "4", "--multilevel", "0.03", "--kway-multilevel", "0.03"),
                 ("-EIG", "--k", "4", "--multilevel", "0.03"), ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--fm", "0.1")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--kway-multilevel" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.4").exists()
