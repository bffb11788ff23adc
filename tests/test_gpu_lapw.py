"""The net-weighted clique Laplacian built on the device (ek_spmv_setup_pins_w,
kernels_build.hip k_rows<true> / k_rows_long<true>) against the
host build (ek_laplacian_build_w, pinned by test_lapw_host.py to the references
of lapw_cases.py), test_gpu_build_shapes.py's pattern: two contexts, the
device-built matrix must give the host-built one's SpMV bit for bit.  Then the
fallbacks that must carry the weights, the dictionary's overflow paths, which
weights make reachable at small n, the Lanczos solve on the weighted operator,
and the multilevel driver's flag against the same V-cycle composed from the
public pieces.  Run on an MI355X: pytest -m gpu."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import build_cases as bc
import lapw_cases as lw
import match_cases as mc
from conftest import PKG_DIR, circuit_path

pytestmark = pytest.mark.gpu

SHAPES = ("short-edge", "long-pow2", "long-dups", "long-selfpin", "cap-exact", "degenerate-nonets", "degenerate-n1",
          "degenerate-tiny-nets", "degenerate-ends")


@pytest.fixture(scope="module")
def ctxs(ek):
    a, b = ek.Context(0), ek.Context(0)
    yield a, b
    a.close()
    b.close()


@functools.lru_cache(maxsize=None)
def _hgr(name, kind):
    from conftest import load_package
    return lw.hypergraph(load_package(), name, kind)


@functools.lru_cache(maxsize=None)
def _reference(name, kind):
    """(x, y, absrow): per row math.fsum of ref_ordered's products with a seeded
    normal x, and sum_j |a_ij x_j|; computed once per (case, weighting)."""
    c = lw.cases()[name]
    rowptr, col, val = lw.ref_ordered(name, kind)
    x = c.x()
    prod = val.view(np.float64) * x[col]
    y, a = np.zeros(c.n), np.zeros(c.n)
    for r in np.flatnonzero(np.diff(rowptr) > 1):
        p = prod[rowptr[r]:rowptr[r + 1]]
        y[r] = math.fsum(p)
        a[r] = math.fsum(np.abs(p))
    lone = np.flatnonzero(np.diff(rowptr) == 1)
    y[lone] = prod[rowptr[lone]]
    a[lone] = np.abs(prod[rowptr[lone]])
    return x, y, a


def _host_rows(ctx, h, weighted=True):
    L = h.laplacian(weighted=weighted)
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)


def _same_as_host(name, kind, dev_ctx, host_ctx, h, on_device, same_format=True):
    """The weighted device build of h against the weighted host build, both against the reference."""
    x, y_ref, absrow = _reference(name, kind)
    _host_rows(host_ctx, h)
    assert dev_ctx.spmv_setup_pins(h, weighted=True) is on_device
    if same_format:
        assert dev_ctx.spmv_format() == host_ctx.spmv_format()
    assert dev_ctx.spmv_bytes() == host_ctx.spmv_bytes()
    y_dev, y_host = dev_ctx.spmv_host(x), host_ctx.spmv_host(x)
    bad = np.flatnonzero(y_dev.view(np.uint64) != y_host.view(np.uint64))
    assert bad.size == 0, (bad[:8], y_dev[bad[:8]], y_host[bad[:8]])
    for y in (y_dev, y_host):
        err = np.abs(y - y_ref)
        print(name, kind, "max |y - ref| / sum|a x| =", float((err / np.where(absrow > 0, absrow, 1.0)).max()))
        assert np.all(err <= 1e-14 * absrow)
    return y_dev


@pytest.mark.parametrize("kind", ["mod3", "wide"])
@pytest.mark.parametrize("name", SHAPES)
def test_device_build_equals_host_build(ek, ctxs, monkeypatch, name, kind):
    """The coding decision, the stored bytes and y = L x are the weighted host build's, and both lie within
    1e-14 sum_j |a_ij x_j| of the exactly rounded row sums of lapw_cases.ref_ordered."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    monkeypatch.delenv("EK_HOST_LAPLACIAN", raising=False)
    dev_ctx, host_ctx = ctxs
    y = _same_as_host(name, kind, dev_ctx, host_ctx, _hgr(name, kind), True)
    assert dev_ctx.spmv_format()[0] is True
    if name == "long-dups":  # the weights reached the kernels: not the unweighted operator
        dev_ctx.spmv_setup_pins(_hgr(name, kind))
        assert not np.array_equal(dev_ctx.spmv_host(_reference(name, kind)[0]), y)


def test_host_fallbacks_carry_the_weights(ek, ctxs, monkeypatch):
    """cap-over (a row past the LDS sort) before and after cap-exact on a fresh context, as
    test_over_long_row_on_a_fresh_context; then EK_HOST_LAPLACIAN; then EK_SPMV_PLAIN."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    monkeypatch.delenv("EK_HOST_LAPLACIAN", raising=False)
    _, host_ctx = ctxs
    fresh = ek.Context(0)
    try:
        _same_as_host("cap-over", "mod3", fresh, host_ctx, _hgr("cap-over", "mod3"), False)
        _same_as_host("cap-exact", "mod3", fresh, host_ctx, _hgr("cap-exact", "mod3"), True)
        _same_as_host("cap-over", "mod3", fresh, host_ctx, _hgr("cap-over", "mod3"), False)
        monkeypatch.setenv("EK_HOST_LAPLACIAN", "1")
        _same_as_host("long-dups", "wide", fresh, host_ctx, _hgr("long-dups", "wide"), False)
        monkeypatch.delenv("EK_HOST_LAPLACIAN")
        monkeypatch.setenv("EK_SPMV_PLAIN", "1")
        _same_as_host("long-dups", "wide", fresh, host_ctx, _hgr("long-dups", "wide"), True)
        assert fresh.spmv_format()[0] is False
    finally:
        fresh.close()


@pytest.mark.parametrize("name", bc.SMALL)
def test_unit_vectors_recover_the_matrix(ek, ctxs, monkeypatch, name):
    """L e_j is column j itself, so the dense result equals ref_ordered bit for bit; zeros compare by value
    (test_gpu_build_shapes.py says why)."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, _ = ctxs
    c = lw.cases()[name]
    A = lw.dense(name, "mod3")
    assert dev_ctx.spmv_setup_pins(_hgr(name, "mod3"), weighted=True) is True
    got = np.empty_like(A)
    for j in range(c.n):
        e = np.zeros(c.n)
        e[j] = 1.0
        got[:, j] = dev_ctx.spmv_host(e)
    zero = A == 0.0
    assert np.all(got[zero] == 0.0)
    bad = np.argwhere((got.view(np.uint64) != A.view(np.uint64)) & ~zero)
    assert bad.size == 0, (bad[:8], [(got[i, j], A[i, j]) for i, j in bad[:8]])


@pytest.mark.parametrize("plain", [False, True])
def test_dictionary_overflow_leaves_the_matrix_plain(ek, ctxs, monkeypatch, plain):
    """dict-half: 40,004 distinct values, over half the 65,536-slot table (the nd test); dict-full: 70,004, over
    the table itself (k_dict_insert's overflow count, which shares counters[1] with "row too long": that count
    was read as zero before the dictionary ran).  Both are built on the device and left plain, y is the host
    build's bit for bit (the host path codes dict-half: the same row blocks, so the same sums), and a
    unit-weight build of fract on the same context is coded again."""
    if plain:
        monkeypatch.setenv("EK_SPMV_PLAIN", "1")
    else:
        monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    for name in lw.DICT_NAMES:
        _same_as_host(name, "own", dev_ctx, host_ctx, _hgr(name, "own"), True, same_format=False)
        assert dev_ctx.spmv_format()[0] is False
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    h = ek.Hypergraph.read(circuit_path("fract"))
    h.set_weights(None, np.ones(h.nets, np.int32))
    _host_rows(host_ctx, h, weighted=False)
    assert dev_ctx.spmv_setup_pins(h, weighted=True) is True
    assert dev_ctx.spmv_format() == host_ctx.spmv_format() and dev_ctx.spmv_format()[0] is True
    x = np.random.default_rng(5).standard_normal(h.nodes)
    assert np.array_equal(dev_ctx.spmv_host(x).view(np.uint64), host_ctx.spmv_host(x).view(np.uint64))


@pytest.mark.parametrize("name", ["long-dups", "long-selfpin", "degenerate-ends"])
def test_without_weights_it_is_the_unweighted_call(ek, ctxs, monkeypatch, name):
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, other = ctxs
    h = _hgr(name, None)
    x = lw.cases()[name].x()
    assert other.spmv_setup_pins(h) is True
    want = (other.spmv_format(), other.spmv_bytes(), other.spmv_host(x).tobytes())
    assert dev_ctx.spmv_setup_pins(h, weighted=True) is True  # no weights: net_w = NULL
    assert (dev_ctx.spmv_format(), dev_ctx.spmv_bytes(), dev_ctx.spmv_host(x).tobytes()) == want
    net_ptr, pins = h.pins()
    dev = ctypes.c_int32(0)
    for net_w in (None, np.ones(h.nets, np.int32)):
        rc = ek.lib.ek_spmv_setup_pins_w(dev_ctx._c, h.nodes, h.nets, ek._p(net_ptr), ek._p(pins),
                                         None if net_w is None else ek._p(net_w), ctypes.byref(dev))
        assert rc == ek.EK_OK and dev.value == 1
        assert (dev_ctx.spmv_format(), dev_ctx.spmv_bytes(), dev_ctx.spmv_host(x).tobytes()) == want
    bad = np.ones(h.nets, np.int32)
    bad[h.nets // 2] = 0
    assert ek.lib.ek_spmv_setup_pins_w(dev_ctx._c, h.nodes, h.nets, ek._p(net_ptr), ek._p(pins), ek._p(bad),
                                       ctypes.byref(dev)) == ek.EK_EINVAL


def test_shards(ek, ctxs, monkeypatch):
    """long-dups under mod3 at 3 ranks, every rank in turn on one context (test_shards_with_an_empty_rank's
    trick): the rows of ek_shard_map, y within the 1e-14 absrow bar of the full weighted matrix's rows."""
    monkeypatch.setenv("EK_MR_HALO", "0")
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    h = _hgr("long-dups", "mod3")
    n = h.nodes
    x, _, _ = _reference("long-dups", "mod3")
    _host_rows(host_ctx, h)
    y_full = host_ctx.spmv_host(x)

    def never(*_):
        raise AssertionError("no collective expected")

    try:
        off = ek.shard_map(h, 3)
        for r in range(3):
            dev_ctx.comm_init_host(3, r, never, never)
            assert dev_ctx.spmv_setup_pins(h, weighted=True) is True
            row0, nrows = int(off[r]), int(off[r + 1] - off[r])
            assert dev_ctx.spmv_dims() == (n, row0, nrows) and nrows > 0
            y = dev_ctx.spmv_host(x)
            S = h.laplacian_rows(row0, row0 + nrows, weighted=True)
            absrow = np.add.reduceat(np.abs(S.val * x[S.col]), S.rowptr[:-1])
            assert np.all(np.abs(y - y_full[row0: row0 + nrows]) <= 1e-14 * absrow + 1e-300)
    finally:
        dev_ctx.comm_init_host(1, 0, never, never)


# ------------------------------------------------------------------ Lanczos on the weighted operator
@pytest.mark.parametrize("heavy, together", [(((0, 1), (2, 3)), ((0, 1), (2, 3))),
                                             (((1, 2), (3, 0)), ((1, 2), (3, 0)))])
def test_lanczos_sees_the_weights(ek, ctxs, monkeypatch, heavy, together):
    """Four clusters in a ring; with unit weights lambda_2 = lambda_3, and weight 8 on two opposite links
    decides which pairs of clusters stay together."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, _ = ctxs
    n, nets, w = lw.ring_of_clusters(heavy)
    ev1 = np.linalg.eigvalsh(lw.dense_of(n, nets, np.ones(len(nets), np.int32)))
    assert abs(ev1[2] - ev1[1]) <= 1e-12  # degenerate without the weights
    evals, evecs = np.linalg.eigh(lw.dense_of(n, nets, w))
    assert abs(evals[0]) <= 1e-12 and (evals[2] - evals[1]) / evals[1] >= 1.0  # the precondition
    assert abs(evals[1] - 0.404947) <= 1e-6 and abs(evals[2] - 1.257071) <= 1e-6
    ptr, pins = mc.pack(nets)
    h = ek.Hypergraph.from_pins(n, ptr, pins)
    h.set_weights(None, w)
    assert dev_ctx.spmv_setup_pins(h, weighted=True) is True
    lam, v, st = dev_ctx.lanczos_fiedler()
    assert st["converged"] and abs(lam - evals[1]) <= 1e-10, (lam, evals[1])
    ref = evecs[:, 1]
    v = v * np.sign(v @ ref)
    assert np.abs(v - ref).max() <= 1e-8
    _, bits = ek.median_split(v)
    cl = bits.reshape(4, 8)
    assert np.all(cl == cl[:, :1])  # whole clusters
    for a, b in together:
        assert cl[a, 0] == cl[b, 0]
    assert int(bits.sum()) == 16


def test_pow2_scales_lambda(ek, ctxs, monkeypatch):
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, _ = ctxs
    h = ek.Hypergraph.read(circuit_path("fract"))
    dev_ctx.spmv_setup_pins(h)
    lam0, v0, st0 = dev_ctx.lanczos_fiedler()
    h.set_weights(None, lw.weights("pow2", h.nets))
    assert dev_ctx.spmv_setup_pins(h, weighted=True) is True
    lam1, v1, st1 = dev_ctx.lanczos_fiedler()
    assert st0["converged"] and st1["converged"]
    assert abs(lam1 - 32.0 * lam0) <= 1e-10 * 32.0 * lam0, (lam0, lam1)
    v1 = v1 * np.sign(v1 @ v0)
    assert np.array_equal(ek.rank_split(v0, h.nodes // 2), ek.rank_split(v1, h.nodes // 2))


# ------------------------------------------------------------------ the multilevel driver's flag
COARSE = {"fract": 16, "ibm01": 512}
LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "cut_before", "cut_after", "fm_moves")
INTS = ("levels", "coarsest_fallback", "sweep_feasible", "max_cluster", "total_weight", "max_part", "cut", "cut_nets",
        "w0", "w1", "n0", "n1")
EPS = 0.03


def compose(ek, ctx, h, eps, coarse_nodes):
    """test_gpu_multilevel.py's composition of the V-cycle from the host checkers, the coarsest level's set-up
    being the weighted one."""
    node_w = h.weights()[0]
    W = h.nodes if node_w is None else int(node_w.sum())
    lmax = math.floor((1.0 + eps) * float((W + 1) // 2))
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
    assert cur.nodes >= 4 and cur.weights()[1] is not None and cur.weights()[1].max() > 1
    ctx.spmv_setup_pins(cur, weighted=True)
    _, v, _ = ctx.lanczos_fiedler()
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
    res.update(cut_before=before, cut_after=after, fm_moves=moves, levels=len(clusters), coarsest_fallback=0,
               sweep_feasible=sweep["feasible"], max_cluster=cap, total_weight=W, max_part=lmax)
    cut, cut_nets, w0, w1 = ek.bipart_metrics_host(h, side)
    n1 = int(side.sum())
    res.update(cut=cut, cut_nets=cut_nets, w0=w0, w1=w1, n0=h.nodes - n1, n1=n1)
    return side, res


@pytest.mark.parametrize("name", ["fract", "ibm01"])
def test_flagged_driver_equals_composition(ek, ctxs, monkeypatch, name):
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    ctx, _ = ctxs
    h = mc.circuit(ek, name, True)
    side, res = ctx.multilevel_bipartition(h, EPS, COARSE[name], weighted_laplacian=True)
    want_side, want = compose(ek, ctx, h, EPS, COARSE[name])
    for k in LEVEL_FIELDS + INTS:
        assert res[k] == want[k], k
    assert np.array_equal(side, want_side)
    if res["sweep_feasible"] == 1:
        assert max(res["w0"], res["w1"]) <= res["max_part"]
    again, res2 = ctx.multilevel_bipartition(h, EPS, COARSE[name], weighted_laplacian=True)
    assert again.tobytes() == side.tobytes() and all(res[k] == res2[k] for k in LEVEL_FIELDS + INTS)
    _, plain = ctx.multilevel_bipartition(h, EPS, COARSE[name])
    print(f"{name}: coarsest cut {plain['cut_before'][-1]} -> {res['cut_before'][-1]} with the flag, final "
          f"{plain['cut']} -> {res['cut']}")


def test_ex_entry_flags(ek, ctxs):
    """flags = 0 is the old entry, byte for byte; any bit but bit 0 is EK_EINVAL."""
    ctx, _ = ctxs
    h = mc.circuit(ek, "fract", True)
    old, ro = ctx.multilevel_bipartition(h, EPS, 16)
    o = ek._ml_opts(EPS, 16, ek.ML_LEVELS, 0, 64, 8, 0, 1000, None)
    side = np.full(h.nodes, 255, np.uint8)
    r = ek.MlResult()
    assert ek.lib.ek_multilevel_bipartition_ex(ctx._c, h._h, ctypes.byref(o), 0, ek._p(side), ctypes.byref(r)) == ek.EK_OK
    rn = ek._ml_result(r)
    assert side.tobytes() == old.tobytes() and all(ro[k] == rn[k] for k in LEVEL_FIELDS + INTS)
    for flags in (2, 3, 1 << 30, -2):
        side[:] = 255
        assert ek.lib.ek_multilevel_bipartition_ex(ctx._c, h._h, ctypes.byref(o), flags, ek._p(side),
                                                   ctypes.byref(r)) == ek.EK_EINVAL
        assert np.all(side == 255)


def test_cli_weighted_laplacian(ek, ctxs, tmp_path):
    ctx, _ = ctxs
    h = mc.circuit(ek, "fract", True)
    src = tmp_path / "fractw.hgr"
    h.write(src)  # fmt 11
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    base = [tool, str(src), "-EIG", "--multilevel", "0.03", "--ml-coarse", "16"]
    r = subprocess.run(base + ["--ml-weighted-laplacian"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ml:")]
    assert len(line) == 1 and line[0].endswith(", wlap=1"), r.stdout
    part = np.array((tmp_path / "results" / "fractw.hgr.part.2").read_text().split(), np.uint8)
    side, res = ctx.multilevel_bipartition(h, 0.03, 16, weighted_laplacian=True)
    assert np.array_equal(part, side)
    assert int(re.search(r"\bcut (\d+)", line[0]).group(1)) == res["cut"]
    r = subprocess.run(base, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ml:")]
    assert len(line) == 1 and "wlap" not in line[0] and line[0].endswith(".part.2"), r.stdout
    r = subprocess.run([tool, str(src), "-EIG", "--ml-weighted-laplacian"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--ml-weighted-laplacian" in r.stdout
