"""The device Laplacian build (ek_spmv_setup_pins, kernels_build.hip) on the
hypergraphs of build_cases.py, each placed on one of its branch points
(test_build_cases_host.py proves the placement and pins the host build to two
references of its own): the thread / workgroup / host-fallback row paths at
their limits, the bitonic sort at its padded sizes, repeated pins, the scan at
its tile and carry edges, the code-bit limit, no nets and a rank without rows.
The device-built matrix must give the host-built one's SpMV bit for bit.
Run on an MI355X: pytest -m gpu.  Wall times there: hub-8ranks 3.4 s to build
and 3.1 s over its 8 shards (one thread orders the hub's 8,092 incidences),
the cap-exact round trip 1.6 s, long-pow2 1.1 s, every other test under 1 s."""
import functools
import math

import numpy as np
import pytest

import build_cases as bc
from conftest import circuit_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(ek):
    a, b = ek.Context(0), ek.Context(0)
    yield a, b
    a.close()
    b.close()


@functools.lru_cache(maxsize=None)
def _hgr(name):
    from conftest import load_package
    return bc.cases()[name].hypergraph(load_package())


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(x, y, absrow): per row math.fsum of ref_ordered's products with a seeded
    normal x, and sum_j |a_ij x_j|; computed once per case."""
    c = bc.cases()[name]
    rowptr, col, val = bc.ref_ordered(name)
    x = c.x()
    prod = val.view(np.float64) * x[col]
    y, a = np.zeros(c.n), np.zeros(c.n)
    for r in np.flatnonzero(np.diff(rowptr) > 1):  # (a lone diagonal is the isolated row's -0.0)
        p = prod[rowptr[r]:rowptr[r + 1]]
        y[r] = math.fsum(p)
        a[r] = math.fsum(np.abs(p))
    lone = np.flatnonzero(np.diff(rowptr) == 1)
    y[lone] = prod[rowptr[lone]]
    a[lone] = np.abs(prod[rowptr[lone]])
    return x, y, a


def _host_rows(ctx, h):
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)


def _same_as_host(name, dev_ctx, host_ctx, h, on_device):
    """The device build of h against the host build, both against the reference."""
    x, y_ref, absrow = _reference(name)
    _host_rows(host_ctx, h)
    assert dev_ctx.spmv_setup_pins(h) is on_device
    assert dev_ctx.spmv_format() == host_ctx.spmv_format()
    assert dev_ctx.spmv_bytes() == host_ctx.spmv_bytes()
    y_dev, y_host = dev_ctx.spmv_host(x), host_ctx.spmv_host(x)
    bad = np.flatnonzero(y_dev.view(np.uint64) != y_host.view(np.uint64))
    assert bad.size == 0, (bad[:8], y_dev[bad[:8]], y_host[bad[:8]])
    for y in (y_dev, y_host):
        err = np.abs(y - y_ref)
        print(name, "max |y - ref| / sum|a x| =", float((err / np.where(absrow > 0, absrow, 1.0)).max()))
        assert np.all(err <= 1e-14 * absrow)
    return y_dev


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_build_equals_host_build(ek, ctxs, monkeypatch, name):
    """Every case but cap-over is built on the device; the coding decision, the
    stored bytes and y = L x are the host build's, and both lie within
    1e-14 sum_j |a_ij x_j| of the exactly rounded row sums of ref_ordered (the
    bar of test_gpu_spmv_shapes.py).  codes-over: built on the device and
    left uncoded because its values outnumber the 2,048 codes."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    _same_as_host(name, dev_ctx, host_ctx, _hgr(name), name != "cap-over")
    assert dev_ctx.spmv_format()[0] is (name != "codes-over")


@pytest.mark.parametrize("name", bc.SMALL)
def test_unit_vectors_recover_the_matrix(ek, ctxs, monkeypatch, name):
    """L e_j is column j itself: each product is exact and every other term of
    the row sum is a zero, so the dense result equals ref_ordered bit for bit.
    What this cannot see is the sign of a zero (an isolated row's diagonal is
    -0.0, and the sum of zeros of both signs is +0.0): zeros compare by value."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, _ = ctxs
    c = bc.cases()[name]
    A = bc.dense(name)
    assert dev_ctx.spmv_setup_pins(_hgr(name)) is True
    got = np.empty_like(A)
    for j in range(c.n):
        e = np.zeros(c.n)
        e[j] = 1.0
        got[:, j] = dev_ctx.spmv_host(e)
    zero = A == 0.0
    assert np.all(got[zero] == 0.0)
    bad = np.argwhere((got.view(np.uint64) != A.view(np.uint64)) & ~zero)
    assert bad.size == 0, (bad[:8], [(got[i, j], A[i, j]) for i, j in bad[:8]])


@pytest.mark.parametrize("name", ["long-pow2", "long-dups", "long-selfpin"])
def test_plain_form_from_the_device_arrays(ek, ctxs, monkeypatch, name):
    """EK_SPMV_PLAIN=1: the SpMV reads the CSR the build kernels wrote, no coding between."""
    monkeypatch.setenv("EK_SPMV_PLAIN", "1")
    dev_ctx, host_ctx = ctxs
    _same_as_host(name, dev_ctx, host_ctx, _hgr(name), True)
    assert dev_ctx.spmv_format()[0] is False


def test_over_long_row_on_a_fresh_context(ek, ctxs, monkeypatch):
    """A row past the LDS sort as the first build of a context, whose length
    buffers no earlier build has written: the host fallback, the host's
    result; then the largest row the device sorts, then the over-long one
    again after that large build."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    _, host_ctx = ctxs
    fresh = ek.Context(0)
    try:
        _same_as_host("cap-over", fresh, host_ctx, _hgr("cap-over"), False)
        _same_as_host("cap-exact", fresh, host_ctx, _hgr("cap-exact"), True)
        _same_as_host("cap-over", fresh, host_ctx, _hgr("cap-over"), False)
    finally:
        fresh.close()


@pytest.mark.parametrize("name,ranks", [("hub-8ranks", 8), ("long-dups", 3)])
def test_shards_with_an_empty_rank(ek, ctxs, monkeypatch, name, ranks):
    """Every rank in turn on one context (collectives that raise, EK_MR_HALO=0,
    as test_device_build_shard_rows): the rows of ek_shard_map, y within the
    1e-14 absrow bar of the full matrix's rows; hub-8ranks' rank 1 owns no rows,
    returns an empty vector and leaves the context usable for the next rank."""
    monkeypatch.setenv("EK_MR_HALO", "0")
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    h = _hgr(name)
    n = h.nodes
    x, _, _ = _reference(name)
    _host_rows(host_ctx, h)
    y_full = host_ctx.spmv_host(x)

    def never(*_):
        raise AssertionError("no collective expected")

    try:
        off = ek.shard_map(h, ranks)
        assert (name == "hub-8ranks") == bool(np.any(np.diff(off) == 0))
        for r in range(ranks):
            dev_ctx.comm_init_host(ranks, r, never, never)
            assert dev_ctx.spmv_setup_pins(h) is True
            row0, nrows = int(off[r]), int(off[r + 1] - off[r])
            assert dev_ctx.spmv_dims() == (n, row0, nrows)
            y = dev_ctx.spmv_host(x)
            assert y.shape == (nrows,)
            if nrows == 0:
                continue
            S = h.laplacian_rows(row0, row0 + nrows)
            absrow = np.add.reduceat(np.abs(S.val * x[S.col]), S.rowptr[:-1])
            assert np.all(np.abs(y - y_full[row0: row0 + nrows]) <= 1e-14 * absrow + 1e-300)
    finally:
        dev_ctx.comm_init_host(1, 0, never, never)


@pytest.mark.parametrize("name", ["long-selfpin", "cap-exact"])
def test_written_and_read_back(ek, ctxs, monkeypatch, tmp_path, name):
    """The case through Hypergraph.write and Hypergraph.read (repeated pins and
    all): the same pins, and the device build of what was read gives the bits
    of the from_pins build.  (Context.spmv_setup_pins hands the library copies
    of the pins, so the reader's raw-entry count — which lets ek_solve_file
    skip the input scans — is not used on this route.)"""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    h = _hgr(name)
    y = _same_as_host(name, dev_ctx, host_ctx, h, True)
    path = str(tmp_path / f"{name}.hgr")
    h.write(path)
    h2 = ek.Hypergraph.read(path)
    for a, b in zip(h.pins(), h2.pins()):
        assert np.array_equal(a, b)
    y2 = _same_as_host(name, dev_ctx, host_ctx, h2, True)
    assert np.array_equal(y.view(np.uint64), y2.view(np.uint64))


def test_leftovers_fract_after_the_cases(ek, ctxs, monkeypatch):
    """After every case above (fallbacks, empty ranks, a million rows), the same
    contexts still build a circuit right."""
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    dev_ctx, host_ctx = ctxs
    h = ek.Hypergraph.read(circuit_path("fract"))
    for ctx in (dev_ctx, host_ctx):
        other = host_ctx if ctx is dev_ctx else dev_ctx
        _host_rows(other, h)
        assert ctx.spmv_setup_pins(h) is True
        assert ctx.spmv_format() == other.spmv_format() and ctx.spmv_bytes() == other.spmv_bytes()
        x = np.random.default_rng(5).standard_normal(h.nodes)
        assert np.array_equal(ctx.spmv_host(x).view(np.uint64), other.spmv_host(x).view(np.uint64))
