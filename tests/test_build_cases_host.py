"""The device-build shape cases (build_cases.py) hold the shapes they are named
for, and the host build (graph_build.cpp) equals both of their references:
ref_ordered bit for bit, ref_exact within the bound of M rounded terms added
one after the other.  No GPU: test_gpu_build_shapes.py runs the kernels on
the same cases."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import build_cases as bc
from conftest import PKG_DIR


@pytest.fixture(scope="module")
def cases():
    return bc.cases()


@pytest.fixture(scope="module")
def built(ek, cases):
    """name -> (Hypergraph, host Laplacian), each built once."""
    out = {}

    def get(name):
        if name not in out:
            h = cases[name].hypergraph(ek)
            out[name] = (h, h.laplacian())
        return out[name]
    return get


def _colbits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def _row(L, r):
    a, b = int(L.rowptr[r]), int(L.rowptr[r + 1])
    return L.col[a:b], L.val[a:b]


def test_build_constants():
    """The cases take the kernels' limits without reading the headers; here they
    are held to the sources."""
    assert (bc.ROW_SHORT, bc.LONG_CAP, bc.SCAN_TILE, bc.SCAN_CHUNK, bc.HOST_INSERTION, bc.SEG) == \
        (256, 8192, 1024, 256, 48, 768)
    src = open(os.path.join(PKG_DIR, "csrc", "kernels_build.hip")).read()
    for name, v in (("BT", bc.SCAN_CHUNK), ("ROW_SHORT", bc.ROW_SHORT), ("LONG_CAP", bc.LONG_CAP),
                    ("SCAN_TILE", bc.SCAN_TILE)):
        assert re.search(rf"constexpr int {name} = {v}\b", src), name
    assert "for (int b0 = 0; b0 < ntiles; b0 += BT)" in src  # k_scan_sums: BT tiles per trip
    host = open(os.path.join(PKG_DIR, "csrc", "graph_build.cpp")).read()
    assert f"row.size() <= {bc.HOST_INSERTION}" in host
    assert set(bc.NAMES) == set(bc.cases()) and set(bc.SMALL) <= set(bc.NAMES)


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_build_equals_ref_ordered(cases, built, name):
    _, L = built(name)
    rowptr, col, val = bc.ref_ordered(name)
    assert np.array_equal(L.rowptr, rowptr)
    assert np.array_equal(L.col, col)
    bad = np.flatnonzero(L.val.view(np.uint64) != val)
    assert bad.size == 0, (bad[:8], L.val[bad[:8]], val.view(np.float64)[bad[:8]])


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_build_within_bound_of_exact(cases, built, name):
    """|a_rc - exact| <= gamma_M S: M the row's raw-entry count, S the exact sum
    of its 2/k terms, gamma_M = M u / (1 - M u), u = 2^-53 — every entry is a
    sum of at most M terms, each rounded once (2.0 / k) and then added one after
    the other, the diagonal over the merged entries included."""
    c = cases[name]
    _, L = built(name)
    exact = bc.ref_exact(name)
    raw = c.raw_counts()
    u = Fraction(1, 1 << 53)
    lens = np.diff(L.rowptr.astype(np.int64))
    iso = np.ones(c.n, bool)
    iso[list(exact)] = False
    at = L.rowptr[:-1][iso]
    assert np.all(lens[iso] == 1) and np.array_equal(L.col[at], np.flatnonzero(iso)) and np.all(L.val[at] == 0.0)
    assert np.all(raw[iso] == 0)
    worst = Fraction(0)
    for r, (ent, M, S) in exact.items():
        assert M == raw[r] and M > 0
        cols, vals = _row(L, r)
        assert sorted(ent) == cols.tolist()
        bound = M * u / (1 - M * u) * S
        for cc, v in zip(cols.tolist(), vals.tolist()):
            err = abs(Fraction(v) - ent[cc])
            assert err <= bound, (r, cc, v, float(err), float(bound))
            worst = max(worst, err / bound)
    print(name, "max error / bound =", float(worst))


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_shards_equal_the_full_rows(ek, cases, built, name):
    """laplacian_rows over the shard maps at 3 and 8 ranks, empty ranks included."""
    h, _ = built(name)
    rowptr, col, val = bc.ref_ordered(name)
    for ranks in (3, 8):
        off = ek.shard_map(h, ranks)
        assert off[0] == 0 and off[-1] == cases[name].n and np.all(np.diff(off) >= 0)
        for r in range(ranks):
            a, b = int(off[r]), int(off[r + 1])
            S = h.laplacian_rows(a, b)
            assert np.array_equal(S.rowptr, rowptr[a:b + 1] - rowptr[a])
            assert np.array_equal(S.col, col[rowptr[a]:rowptr[b]])
            assert np.array_equal(S.val.view(np.uint64), val[rowptr[a]:rowptr[b]])


# ------------------------------------------------------------------ shapes
def test_short_edge(cases, built):
    c = cases["short-edge"]
    raw = c.raw_counts()
    _, L = built("short-edge")
    lens = np.diff(L.rowptr)
    assert c.n <= 600
    assert sorted(c.meta["hubs"]) == [47, 48, 49, 255, 256, 257]
    for want, v in c.meta["hubs"].items():
        assert raw[v] == want and lens[v] == want + 1  # distinct neighbours: nothing merges
        assert raw[v - 2] == 0 and raw[v - 1] == 1 and raw[v + 1] == 2
        cols, _ = _row(L, v)
        assert cols[0] < v < cols[-1]  # the diagonal goes in between
    assert np.all(raw[c.meta["ones"]] == 1) and np.all(raw[c.meta["twos"]] == 2)
    assert np.count_nonzero(raw > bc.ROW_SHORT) == 1


def test_long_pow2(cases, built):
    c = cases["long-pow2"]
    raw = c.raw_counts()
    _, L = built("long-pow2")
    lens = np.diff(L.rowptr)
    assert sorted(c.meta["hubs"]) == [257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192]
    for want, v in c.meta["hubs"].items():
        assert raw[v] == want and lens[v] == want + 1
        cols, _ = _row(L, v)
        assert cols[0] < v < cols[-1]
        first = [u for e in c.nets if v in e for u in e if u != v]  # the columns in raw order: not sorted
        assert first != sorted(first)
    assert sorted(raw[raw > bc.ROW_SHORT]) == sorted(c.meta["hubs"]) and raw.max() == bc.LONG_CAP
    assert lens.max() == bc.LONG_CAP + 1 > bc.SEG and np.count_nonzero(lens > bc.SEG) == 8  # 1,023 + 1 and up


def test_long_dups_is_order_sensitive(cases, built):
    c = cases["long-dups"]
    raw = c.raw_counts()
    hub = c.meta["hub"]
    _, L = built("long-dups")
    cols, vals = _row(L, hub)
    assert 1000 <= raw[hub] <= bc.LONG_CAP and np.count_nonzero(raw > bc.ROW_SHORT) == 1
    assert cols[0] < hub < cols[-1] and sum(v > hub for v in c.meta["cols"]) == 2
    changed = 0
    for cc in c.meta["cols"]:
        t = bc.contributions(c, hub, cc)
        assert len(t) == 44 and len(set(t)) == 4  # -2/3, -2/5, -2/7, -2/11, dozens in all
        assert t != sorted(t) and len({tuple(t[i:i + 4]) for i in range(0, 44, 4)}) > 1  # interleaved
        s = 0.0
        for w in t:
            s = s + w
        assert vals[cols.tolist().index(cc)] == s  # the host build sums in net order
        other = 0.0
        for w in sorted(t):  # the same terms grouped by size: what a sort that is not stable may do
            other = other + w
        changed += other != s
    assert changed >= 1  # bit-identity can tell a stable sort from another


def test_long_selfpin(cases, built):
    c = cases["long-selfpin"]
    raw = c.raw_counts()
    m = c.meta
    A = bc.dense("long-selfpin")
    _, L = built("long-selfpin")
    lens = np.diff(L.rowptr)
    assert c.n <= 600
    assert raw[m["L"]] > bc.ROW_SHORT and raw[m["P"]] > bc.ROW_SHORT and raw[m["S"]] <= bc.ROW_SHORT
    assert raw.max() <= bc.LONG_CAP
    assert A[m["L"], m["P"]] == -300.0 and A[m["P"], m["L"]] == -300.0 and A[m["S"], m["Q"]] == -20.0
    for hub in (m["L"], m["S"]):
        assert len(bc.contributions(c, hub, hub)) > 4  # raw (r, r) entries: the diagonal replaces their sum
        cols, _ = _row(L, hub)
        others = {u for e in c.nets if hub in e for u in e}
        assert lens[hub] == len(others) and hub in others  # no entry added for the diagonal
        assert A[hub, hub] > 0 and [hub, hub] in c.nets
    assert raw[m["v2"]] == 2 and lens[m["v2"]] == 1 and A[m["v2"], m["v2"]] == 2.0
    assert raw[m["w2"]] == 6 and lens[m["w2"]] == 1 and abs(A[m["w2"], m["w2"]] - 4.0) < 1e-15


@pytest.mark.parametrize("name,want", [("cap-exact", 8192), ("cap-over", 8193), ("hub-8ranks", 8192)])
def test_cap(ek, cases, built, name, want):
    c = cases[name]
    raw = c.raw_counts()
    hub = c.meta["hub"]
    assert raw[hub] == want and (want > bc.LONG_CAP) == (name == "cap-over")
    assert np.delete(raw, hub).max() <= 3
    assert max(len(e) for e in c.nets) <= 4  # a hub of small nets, not one net of thousands of pins
    if name == "hub-8ranks":
        h, _ = built(name)
        off = ek.shard_map(h, 8)
        assert hub == 0 and off[1] == off[2] == 1  # rank 0 owns the hub alone, rank 1 nothing
        assert np.all(np.diff(off)[2:] > 0)
        assert np.all(np.diff(ek.shard_map(h, 3)) > 0)
    else:
        assert 0 < hub


def test_degenerate(cases, built):
    c = cases["degenerate-nonets"]
    assert c.n == 5 and len(c.nets) == 0 and len(c.pins) == 0
    c = cases["degenerate-n1"]
    assert c.n == 1 and [0, 0] in c.nets and c.raw_counts()[0] == 2
    c = cases["degenerate-tiny-nets"]
    assert max(len(e) for e in c.nets) == 1 and min(len(e) for e in c.nets) == 0 and c.raw_counts().max() == 0
    c = cases["degenerate-ends"]
    raw = c.raw_counts()
    assert c.nets[0] == [] and c.nets[-1] == [] and raw[0] == 0 and raw[-1] == 0 and np.all(raw[1:-1] > 0)
    assert 0 in c.pins  # (in a one-pin net: no entry)
    for name in ("degenerate-nonets", "degenerate-tiny-nets"):
        _, L = built(name)
        assert np.array_equal(L.rowptr, np.arange(cases[name].n + 1)) and np.all(L.val == 0.0)


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_scan_edges(cases, n):
    c = cases[f"scan-{n}"]
    raw = c.raw_counts()
    assert c.n == n and (n - 1) // bc.SCAN_TILE + 1 == (2 if n == 1025 else 1)
    for v in (0, n - 1, 1022, 1023, 1024):
        if v < n:
            assert raw[v] > 0, v
    assert 0 < np.count_nonzero(raw == 0) and len(np.unique(raw)) > 5  # the scanned counts vary


def test_scan_carry(cases):
    c = cases["scan-carry"]
    raw = c.raw_counts()
    tiles = -(-c.n // bc.SCAN_TILE)
    assert c.n == 256 * 1024 + 1025 and tiles == 258 and bc.SCAN_CHUNK < tiles <= 2 * bc.SCAN_CHUNK
    assert 200 <= len(c.nets) <= 400 and max(len(e) for e in c.nets) <= 4
    for v in (0, c.n - 1, 262143, 262144, 263167, 263168):
        assert raw[v] > 0, v
    live = np.flatnonzero(raw)
    assert len(live) < 1500 and np.any(live // bc.SCAN_TILE == 256) and np.any(live // bc.SCAN_TILE == 257)
    assert raw.max() <= bc.LONG_CAP


def test_codes_over(cases, built):
    c = cases["codes-over"]
    _, L = built("codes-over")
    assert c.n == (1 << 20) + 1 and _colbits(c.n) == 21
    distinct = len(np.unique(L.val.view(np.uint64)))
    print("codes-over distinct values", distinct)
    assert (1 << (32 - 21)) == 2048 < distinct < 3000  # over the codes, far under half the 65,536-slot table
    raw = c.raw_counts()
    assert raw.max() <= bc.ROW_SHORT and np.count_nonzero(raw) < 50000 and raw[c.n - 1] > 0 and raw[0] > 0
    assert {len(e) for e in c.nets} == {2, 3, 5, 7}
