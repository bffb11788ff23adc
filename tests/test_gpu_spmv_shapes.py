"""The SpMV kernels on matrices placed on their branch points (spmv_cases.py;
test_spmv_cases_host.py proves the placement): the adaptive form, coded and
plain, against the exactly rounded row sums, and the column-panel form over
several panels (EK_PANEL_PB=10: 1,024 columns each) against the sequential
left-to-right row sum, bit for bit.  Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import spmv_cases as sc
from conftest import circuit_path, eig_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def _env(monkeypatch, plain=False, panel=False):
    for k, on, v in (("EK_SPMV_PLAIN", plain, "1"), ("EK_SPMV_PANEL", panel, "1"), ("EK_PANEL_PB", panel, str(sc.PB))):
        if on:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)


def _setup(ctx, c):
    ctx.spmv_setup(c.n, 0, c.rowptr, c.col, c.val)


@pytest.mark.parametrize("name", list(sc.cases()))
def test_adaptive_form_coded_and_plain(ek, ctx, monkeypatch, name):
    """|y - exact| <= 1e-14 sum_j |a_ij x_j| per row (the kernel's
    summation depth is at most ceil(len / 256) + 9 roundings: 3.3e-15 relative
    at the 5,000-entry row), exactly 0.0 where that sum is 0; the coded and the
    plain form give the same bits; the coded form is taken exactly where the
    values fit the codes."""
    c = sc.cases()[name]
    y_ref, absrow, _ = sc.reference(name)
    out = {}
    for plain in (False, True):
        _env(monkeypatch, plain=plain)
        _setup(ctx, c)
        packed, stored = ctx.spmv_format()
        assert packed == (c.packed and not plain)
        if packed:  # the segments are SEG entries: the cases sit on the edges they claim
            assert stored == sc.coded_bytes(c)
        else:
            assert stored == ctx.spmv_bytes() == 12 * c.nnz + 4 * (c.n + 1) + 16 * c.n
        y = ctx.spmv_host(c.x)
        err = np.abs(y - y_ref)
        worst = float((err / np.where(absrow > 0, absrow, 1.0)).max())
        print(name, "plain" if plain else "coded", "max |y - ref| / sum|a x| =", worst)
        assert np.all(err <= 1e-14 * absrow)
        assert np.all(y[absrow == 0.0] == 0.0)
        out[plain] = y
    assert np.array_equal(out[False].view(np.uint64), out[True].view(np.uint64))


def test_segment_size_is_768(ek, ctx, monkeypatch):
    """The cases take SEG = 768 without reading the headers: the coded form's
    stored bytes must be those of 768-entry segments (3,072 B of words, 258 row
    starts and one descriptor per block, the long row in the overflow area),
    against 12 B per entry unpacked."""
    _env(monkeypatch)
    c = sc.cases()["seg-exact"]
    _setup(ctx, c)
    blocks = sc.row_blocks(c.rowptr)
    packed, stored = ctx.spmv_format()
    assert packed
    assert stored - 16 * c.n - 8 * c.ncodes == len(blocks) * (768 * 4 + 258 * 2 + 16) + 769 * 4
    assert ctx.spmv_bytes() == 12 * c.nnz + 4 * (c.n + 1) + 16 * c.n


@pytest.mark.parametrize("name", sc.PANEL_CASES)
def test_panel_form_several_panels(ek, ctx, monkeypatch, name):
    """The panel walk at 1,024 columns per panel: rows whose runs lie in
    several panels, empty leading buckets, buckets of three chunks, columns
    either side of a boundary, the value table in LDS and in global memory.
    Each row is the sequential left-to-right sum, bit for bit."""
    c = sc.cases()[name]
    _, _, y_seq = sc.reference(name)
    _env(monkeypatch, panel=True)
    _setup(ctx, c)
    packed, stored = ctx.spmv_format()
    G = sc.panel_groups(c, stored)
    print(name, "panels", -(-c.n >> sc.PB), "workgroups", G)
    assert packed and G is not None and G >= 1 and stored != sc.coded_bytes(c)  # the panel form was built
    y = ctx.spmv_host(c.x)
    bad = np.flatnonzero(y.view(np.uint64) != y_seq.view(np.uint64))
    assert bad.size == 0, (bad[:8], y[bad[:8]], y_seq[bad[:8]])
    # a second x through the same layout: e_j picks single columns, boundary ones included
    for j in {0, 1023, 1024, c.n - 1} & set(range(c.n)):
        e = np.zeros(c.n)
        e[j] = 1.0
        want = sc.sequential_rows(c, e)
        assert np.array_equal(ctx.spmv_host(e).view(np.uint64), want.view(np.uint64)), j


@pytest.mark.parametrize("path", ["host_csr", "pins"])
def test_panel_form_ibm01_13_panels(ek, ctx, monkeypatch, path):
    """ibm01 (12,752 columns: 13 panels at pb 10) through both setup paths:
    the sequential row sums bit for bit, and the Fiedler pair of the solve on
    that layout held to the golden's tolerances."""
    from test_gpu_parity import _fiedler_parity
    h = ek.Hypergraph.read(circuit_path("ibm01"))
    L = h.laplacian()
    _env(monkeypatch, panel=True)
    if path == "pins":
        assert ctx.spmv_setup_pins(h) is True
    else:
        ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    assert -(-h.nodes >> sc.PB) == 13
    full = sc.Case("ibm01", h.nodes, L.rowptr, L.col, L.val, np.random.default_rng(3).standard_normal(h.nodes))
    packed, stored = ctx.spmv_format()
    assert packed and sc.panel_groups(full, stored) is not None
    y = ctx.spmv_host(full.x)
    assert np.array_equal(y.view(np.uint64), sc.sequential_rows(L, full.x).view(np.uint64))
    lam, v, st = ctx.lanczos_fiedler()
    assert st["converged"] and st["residual"] < 1e-9
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path("ibm01"), h.nodes)
    _fiedler_parity("ibm01", lam, v, lam_ref, med_ref, bits_ref, v_ref, ek)
