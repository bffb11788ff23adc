"""The net-weighted clique Laplacian on the host (ek_laplacian_build_w,
ek_laplacian_build_rows_w) against the references of
lapw_cases.py: bit for bit against the ordered restatement, within the derived
rounding bound of exact arithmetic, and bit for bit the unweighted build where
the weights are absent or all ones.  No GPU: test_gpu_lapw.py runs the device
build against this one."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import build_cases as bc
import lapw_cases as lw
from conftest import REPO

SHAPES = ("short-edge", "long-dups", "long-selfpin", "long-pow2", "degenerate-nonets", "degenerate-n1",
          "degenerate-tiny-nets", "degenerate-ends")
ORDERED = [(n, k) for n in SHAPES + lw.DICT_NAMES for k in ("mod3", "wide")] + [(n, "own") for n in lw.DICT_NAMES]
EXACT = [(n, k) for n in SHAPES for k in ("mod3", "wide")] + [("dict-half", "own")]
U = Fraction(1, 1 << 53)


@pytest.fixture(scope="module")
def built(ek):
    """(name, kind) -> (Hypergraph, weighted host Laplacian), each built once."""
    out = {}

    def get(name, kind):
        if (name, kind) not in out:
            h = lw.hypergraph(ek, name, kind)
            out[name, kind] = (h, h.laplacian(weighted=True))
        return out[name, kind]
    return get


def _same_bits(L, rowptr, col, val):
    assert np.array_equal(L.rowptr, rowptr)
    assert np.array_equal(L.col, col)
    bad = np.flatnonzero(L.val.view(np.uint64) != val)
    assert bad.size == 0, (bad[:8], L.val[bad[:8]], val.view(np.float64)[bad[:8]])


@pytest.mark.parametrize("name, kind", ORDERED)
def test_host_build_equals_ref_ordered(built, name, kind):
    _, L = built(name, kind)
    _same_bits(L, *lw.ref_ordered(name, kind))


def test_the_weights_change_the_matrix(ek, built):
    """What fails without the feature: under mod3 the weighted build differs from the unweighted one."""
    h, L = built("long-dups", "mod3")
    L0 = h.laplacian()
    assert np.array_equal(L.col, L0.col) and np.count_nonzero(L.val != L0.val) > 100
    hub, cols = bc.cases()["long-dups"].meta["hub"], bc.cases()["long-dups"].meta["cols"]
    t = lw.contributions("long-dups", "mod3", hub, cols[0])
    assert len(t) == 44 and len(set(t)) > 4  # the weights multiply the distinct terms
    s = 0.0
    for x in t:
        s = s + x
    a = int(L.rowptr[hub])
    assert L.val[a + L.col[a:int(L.rowptr[hub + 1])].tolist().index(cols[0])] == s


@pytest.mark.parametrize("name", [n for n in bc.NAMES])
def test_no_weights_and_unit_weights_are_the_unweighted_build(ek, name):
    h = bc.cases()[name].hypergraph(ek)
    L0 = h.laplacian()
    _same_bits(h.laplacian(weighted=True), L0.rowptr, L0.col, L0.val.view(np.uint64))
    h.set_weights(None, np.ones(h.nets, np.int32))
    _same_bits(h.laplacian(weighted=True), L0.rowptr, L0.col, L0.val.view(np.uint64))
    L1 = h.laplacian()  # the unweighted entry ignores the weights h carries
    _same_bits(L1, L0.rowptr, L0.col, L0.val.view(np.uint64))


@pytest.mark.parametrize("name", SHAPES)
def test_pow2_scales_exactly(ek, built, name):
    h, L = built(name, "pow2")
    L0 = h.laplacian()
    assert np.array_equal(L.rowptr, L0.rowptr) and np.array_equal(L.col, L0.col)
    want = np.ldexp(L0.val, 5)
    assert np.array_equal(L.val.view(np.uint64), want.view(np.uint64))


def _bounds(name, kind, L):
    """Per stored entry (row, col, value, exact, bound): bound = t 2^-53 sum|terms|, t the
    fp64 terms summed into the entry (the diagonal: the row's), one rounding for each
    term's division and at most t - 1 for the additions it passes through."""
    c = lw.cases()[name]
    exact = lw.ref_exact(name, kind)
    for r in range(c.n):
        a, b = int(L.rowptr[r]), int(L.rowptr[r + 1])
        cols, vals = L.col[a:b].tolist(), L.val[a:b].tolist()
        if r not in exact:
            assert cols == [r] and vals == [0.0]
            continue
        ent, _ = exact[r]
        assert sorted(ent) == cols
        for cc, v in zip(cols, vals):
            x, t, s = ent[cc]
            yield r, cc, Fraction(v), x, t * U * s


@pytest.mark.parametrize("name, kind", EXACT)
def test_within_bound_of_exact_symmetric_zero_row_sums(built, name, kind):
    _, L = built(name, kind)
    got, worst = {}, Fraction(0)
    rowsum, rowbound = {}, {}
    for r, cc, v, x, bound in _bounds(name, kind, L):
        err = abs(v - x)
        assert err <= bound, (r, cc, float(v), float(err), float(bound))
        if bound:
            worst = max(worst, err / bound)
        got[r, cc] = (v, bound)
        rowsum[r] = rowsum.get(r, Fraction(0)) + v
        rowbound[r] = rowbound.get(r, Fraction(0)) + bound
    print(name, kind, "max error / bound =", float(worst))
    for (r, cc), (v, bound) in got.items():  # both within their bounds of one exact value
        assert (cc, r) in got
        assert abs(v - got[cc, r][0]) <= bound + got[cc, r][1], (r, cc)
    exact = lw.ref_exact(name, kind)
    for r, s in rowsum.items():  # the exact row sums are zero (but for the (r, r) terms the diagonal replaced)
        assert abs(s - exact[r][1]) <= rowbound[r], (r, float(s), float(rowbound[r]))
    assert any(x[1] for x in exact.values()) == (name in ("long-selfpin", "degenerate-n1", "degenerate-ends"))


@pytest.mark.parametrize("name, kind", [("long-dups", "mod3"), ("long-selfpin", "wide"), ("degenerate-ends", "mod3"),
                                        ("dict-half", "own")])
def test_rows_over_a_three_way_split(built, name, kind):
    h, L = built(name, kind)
    n = h.nodes
    cuts = [0, n // 3, n // 3, n] if name == "degenerate-ends" else [0, n // 3, 2 * n // 3 + 1, n]
    parts = [h.laplacian_rows(a, b, weighted=True) for a, b in zip(cuts[:-1], cuts[1:])]
    for S, a, b in zip(parts, cuts[:-1], cuts[1:]):
        assert np.array_equal(S.rowptr, L.rowptr[a:b + 1] - L.rowptr[a])
    assert np.array_equal(np.concatenate([S.col for S in parts]), L.col)
    assert np.array_equal(np.concatenate([S.val for S in parts]).view(np.uint64), L.val.view(np.uint64))
    S0 = h.laplacian_rows(0, n // 3)  # the unweighted rows differ
    assert not np.array_equal(S0.val, parts[0].val)


def test_dict_cases_hold_their_shape(built):
    """dict-half: more distinct values than half the device table, fewer than the table and than the
    2^(32 - colbits) codes, so only the nd <= TSIZE / 2 test leaves it plain; dict-full: more than the table."""
    for name, m in (("dict-half", lw.DICT_HALF), ("dict-full", lw.DICT_FULL)):
        c = lw.cases()[name]
        w = c.meta["own"]
        assert c.n == m + 1 and len(c.nets) == m and len(np.unique(w)) == m and w.min() == 1 and w.max() == m
        _, L = built(name, "own")
        distinct = len(np.unique(L.val.view(np.uint64)))
        colbits = 1
        while (1 << colbits) < c.n:
            colbits += 1
        print(name, "distinct values", distinct, "colbits", colbits)
        if name == "dict-half":
            assert lw.TSIZE // 2 < distinct <= min(lw.TSIZE, 1 << (32 - colbits)) - 1000
        else:
            assert distinct > lw.TSIZE
    src = open(os.path.join(REPO, "eig-kl-algorithm_amd", "csrc", "ctx_spmv.cpp")).read()
    assert "constexpr int TSIZE = 1 << 16;" in src and "nd <= TSIZE / 2" in src


def test_argument_errors(ek):
    h = bc.cases()["degenerate-ends"].hypergraph(ek)
    out = ctypes.c_void_p()
    assert ek.lib.ek_laplacian_build_w(None, ctypes.byref(out)) == ek.EK_EINVAL
    assert ek.lib.ek_laplacian_build_w(h._h, None) == ek.EK_EINVAL
    assert ek.lib.ek_laplacian_build_rows_w(None, 0, 1, ctypes.byref(out)) == ek.EK_EINVAL
    assert ek.lib.ek_laplacian_build_rows_w(h._h, 0, 1, None) == ek.EK_EINVAL
    assert ek.lib.ek_laplacian_build_rows_w(h._h, -1, 1, ctypes.byref(out)) == ek.EK_EINVAL
    assert ek.lib.ek_laplacian_build_rows_w(h._h, 0, h.nodes + 1, ctypes.byref(out)) == ek.EK_EINVAL
    assert not out.value
    with pytest.raises(ek.EKError) as e:  # weights below 1 never reach the build
        h.set_weights(None, np.zeros(h.nets, np.int32))
    assert e.value.code == ek.EK_EINVAL


NEW_SYMBOLS = ["ek_laplacian_build_w", "ek_laplacian_build_rows_w", "ek_spmv_setup_pins_w",
               "ek_multilevel_bipartition_ex", "ek_multilevel_bipartition_file_ex"]


def test_new_symbols_are_declared_and_exported(ek):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "eigkl.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ek_[a-z0-9_]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(ek.lib, s), s
    assert re.search(r"#define EIGKL_ABI_VERSION 4\b", text) and ek.lib.ek_abi_version() == 4
    assert re.search(r"#define EK_ML_WEIGHTED_LAPLACIAN 1\b", text) and ek.ML_WEIGHTED_LAPLACIAN == 1


def test_cli_flag_needs_multilevel(tmp_path):
    """Refused while the arguments are read: no GPU work."""
    import subprocess
    from conftest import PKG_DIR, circuit_path
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    for args in (("-EIG", "--ml-weighted-laplacian"), ("--ml-weighted-laplacian",),
                 ("-EIG", "--ml-weighted-laplacian", "--fm", "0.03")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--ml-weighted-laplacian" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.2").exists()
