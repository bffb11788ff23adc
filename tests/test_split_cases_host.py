"""The split cases (split_cases.py) are what they are named for, and the numpy
reference they are checked against agrees with the host entry points
(ek_median_split, ek_rank_split).  No GPU: test_gpu_split.py runs the device
kernels on the same cases.

The constants split_cases.py restates are held to the sources as text
(csrc/kernels_kl.hip, csrc/kernels_kway.hip): the library exports none of
them."""
import os
import re

import numpy as np
import pytest

import split_cases as sc
from conftest import PKG_DIR
from kway_cases import ord_key


def test_constants():
    kl = open(os.path.join(PKG_DIR, "csrc", "kernels_kl.hip")).read()
    kw = open(os.path.join(PKG_DIR, "csrc", "kernels_kway.hip")).read()
    m = re.search(r"constexpr int SEL_THREADS = (\d+), SEL_PER = (\d+), SEL_PASSES = (\d+);", kl)
    assert int(m.group(1)) * int(m.group(2)) == sc.SEL_TILE and int(m.group(3)) == 8
    assert int(re.search(r"constexpr int SEL_SUB = (\d+);", kl).group(1)) == sc.SEL_SUB
    m = re.search(r"constexpr int PART_THREADS = (\d+), PART_PER = (\d+), PART_BLOCK = PART_THREADS \* PART_PER;", kl)
    assert int(m.group(1)) * int(m.group(2)) == sc.PART_BLOCK and int(m.group(1)) == sc.PLACE_STRIDE
    m = re.search(r"constexpr int RK_THREADS = (\d+), RK_PER = (\d+), RK_BLOCK = RK_THREADS \* RK_PER,", kw)
    assert int(m.group(1)) * int(m.group(2)) == sc.PART_BLOCK and int(m.group(1)) == sc.PLACE_STRIDE
    # the loops whose second trip the trip2 cases reach
    assert "for (int b = t; b < int(blockIdx.x); b += PART_THREADS) before += bcount[b];" in kl
    assert "for (int b = t; b < nb; b += RK_THREADS) {" in kw
    assert "const unsigned gsize = (nb - g + SEL_SUB - 1) / SEL_SUB, ngroups = nb < SEL_SUB ? nb : SEL_SUB;" in kl


def test_key_value_inverts_ord_key():
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.standard_normal(1000), [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.7e308, -1.7e308]])
    k = ord_key(v)
    assert np.array_equal(sc.key_value(k).view(np.uint64), v.view(np.uint64))  # by bits: the zeros' signs too
    keys = rng.integers(1 << 56, (0xff << 56) - 1, 1000, dtype=np.uint64)  # top byte 0x01..0xfe: no NaN
    assert np.array_equal(ord_key(sc.key_value(keys)), keys)
    # the order of the keys is the order of the values, -0 before +0
    o = np.argsort(k, kind="stable")
    assert np.all(np.diff(v[o]) >= 0) and ord_key(np.array([-0.0]))[0] + np.uint64(1) == ord_key(np.array([0.0]))[0]


def test_no_case_holds_a_nan():
    for name, v in sc.median_cases().items():
        assert v.dtype == np.float64 and not np.isnan(v).any(), name
    for name, (v, n1) in sc.rank_cases().items():
        assert not np.isnan(v).any() and 1 <= n1 < len(v), name


def test_block_and_tile_counts():
    c = sc.median_cases()
    assert sorted(len(c[f"tiny-{k}-{n}"]) for k in ("distinct", "equal") for n in (1, 2, 3, 4)) == [1, 1, 2, 2, 3, 3, 4, 4]
    for n in (1, 2, 3, 4):
        assert np.unique(c[f"tiny-distinct-{n}"]).size == n and np.unique(c[f"tiny-equal-{n}"]).size == 1
    # one place block is 1,024 nodes and one select tile 2,048 keys: a node short, exact, a node over
    assert [sc.place_blocks(n) for n in (1023, 1024, 1025)] == [1, 1, 2]
    assert [sc.select_blocks(n) for n in (2047, 2048, 2049, 4097)] == [1, 1, 2, 3]
    assert [sc.place_blocks(n) for n in (2047, 2048, 2049, 4097)] == [2, 2, 3, 5]
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4097):
        assert len(c[f"edge-{n}"]) == n
    # the arrival counters: every nb of the issue at an odd and an even n
    got = {}
    for name, v in c.items():
        if name.startswith("ctr-"):
            nb = sc.select_blocks(len(v))
            assert name == f"ctr-nb{nb}-{len(v)}"
            got.setdefault(nb, set()).add(len(v) % 2)
    assert got == {nb: {0, 1} for nb in (15, 16, 17, 32, 33)}
    assert {30720, 32768, 32769, 65536, 65537} <= {len(v) for k, v in c.items() if k.startswith("ctr-")}
    # nb < 16: fifteen groups of one block; 16: sixteen of one; 17 and 33: uneven groups; 32: sixteen of two
    assert sc.group_sizes(15) == [1] * 15 and sc.group_sizes(16) == [1] * 16
    assert sc.group_sizes(17) == [2] + [1] * 15 and sc.group_sizes(32) == [2] * 16
    assert sc.group_sizes(33) == [3] + [2] * 15
    for nb in (1, 2, 3, 15, 16, 17, 32, 33, 129):
        assert sum(sc.group_sizes(nb)) == nb
        assert sc.group_sizes(nb) == [len(range(g, nb, sc.SEL_SUB)) for g in range(min(nb, sc.SEL_SUB))]


def test_second_trip_cases():
    c = sc.median_cases()
    assert [sc.place_blocks(n) for n in (262144, 262145, 263169)] == [256, 257, 258]
    assert 263169 - 257 * sc.PART_BLOCK == 1  # the last block holds one node
    assert max(sc.median_ns()) == 263169 == sc.BIG_N
    for n in (262144, 262145, 263169):
        for kind in ("ascending", "descending", "random"):
            assert len(c[f"trip2-{kind}-{n}"]) == n
        assert np.all(np.diff(c[f"trip2-ascending-{n}"]) >= 0) and np.all(np.diff(c[f"trip2-descending-{n}"]) <= 0)
    # block 257's "blocks before" loop is the only one with a second trip (b = 256):
    # the side-0 count of block 256 is what it adds, and it must not be zero
    for kind, want in (("ascending", 1024), ("random", None)):
        _, exp = sc.median_expected(f"trip2-{kind}-263169")
        b256 = int((exp["side"][256 * 1024: 257 * 1024] == 0).sum())
        assert b256 == want if want else 300 < b256 < 724, (kind, b256)
    # and the side-0 share differs strongly between the first 256 blocks and the rest
    _, exp = sc.median_expected("trip2-ascending-263169")
    assert (exp["side"][: 256 * 1024] == 0).mean() < 0.51 and (exp["side"][256 * 1024:] == 0).all()
    _, exp = sc.median_expected("trip2-descending-263169")
    assert (exp["side"][256 * 1024:] == 1).all()


@pytest.mark.parametrize("n", (2050, 4098))
@pytest.mark.parametrize("p", range(8))
def test_parting_pass(n, p):
    keys, k_lo, k_hi = sc.parting_keys(n, p, 1000 * n + p)
    v = sc.median_cases()[f"part-p{p}-{n}"]
    assert np.array_equal(ord_key(v), keys) and np.unique(keys).size == n
    s = np.sort(keys)
    assert int(s[n // 2 - 1]) == k_lo and int(s[n // 2]) == k_hi
    lo, hi = k_lo.to_bytes(8, "big"), k_hi.to_bytes(8, "big")
    first = next(q for q in range(8) if lo[q] != hi[q])
    assert first == p and lo[:p] == hi[:p]
    if p == 0:
        a, b = sc.key_value(np.array([k_lo, k_hi], np.uint64))
        assert a < 0 < b
    if p == 7:
        a, b = sc.key_value(np.array([k_lo, k_hi], np.uint64))
        assert k_hi == k_lo + 1 and np.nextafter(a, np.inf) == b
    # decoys sharing the p-byte prefix, a side
    pre = k_lo >> (64 - 8 * p) if p else 0
    share = np.array([(int(k) >> (64 - 8 * p) if p else 0) == pre for k in keys])
    assert int((share & (keys < np.uint64(k_lo))).sum()) >= 64 and int((share & (keys > np.uint64(k_hi))).sum()) >= 64
    # every pass of either rank sees more than one live bin: of the keys that
    # share the rank's q-byte prefix, byte q takes more than one value
    for mid in (k_lo, k_hi):
        for q in range(8):
            live = [int(k) for k in keys if q == 0 or int(k) >> (64 - 8 * q) == mid >> (64 - 8 * q)]
            assert len({(k >> (56 - 8 * q)) & 255 for k in live}) > 1, (mid, q)


@pytest.mark.parametrize("n", (2049, 2050, 4098))
def test_tie_runs_cover_the_ranks_they_claim(n):
    c = sc.median_cases()
    h = n // 2
    lo = h - 1 if n % 2 == 0 else h
    names = set(sc.tie_runs(n))
    assert {"hi-only-starts", "both-wide", "ends-at-hi"} <= names
    if n % 2 == 0:
        assert {"lo-only-ends", "starts-at-lo", "just-both"} <= names
    for name, (r0, r1) in sc.tie_runs(n).items():
        v = c[f"tie-{name}-{n}"]
        s = np.sort(v)
        run = np.flatnonzero(s == 0.25)
        assert (int(run[0]), int(run[-1])) == (r0, r1) and run.size == r1 - r0 + 1, name
        assert np.unique(s).size == n - run.size + 1, name  # everything else is distinct
        holds = {r for r in {lo, h} if r0 <= r <= r1}
        want = {"hi-only-starts": {h}, "both-wide": {lo, h}, "ends-at-hi": {lo, h}, "lo-only-ends": {lo},
                "starts-at-lo": {lo, h}, "just-both": {lo, h}}[name]
        assert holds == want, name
    assert sc.tie_runs(n)["hi-only-starts"][0] == h and sc.tie_runs(n)["ends-at-hi"][1] == h
    if n % 2 == 0:
        assert sc.tie_runs(n)["lo-only-ends"][1] == h - 1 and sc.tie_runs(n)["starts-at-lo"][0] == h - 1
    # the run placed by node id: crosses node 1024 and reaches (n = 2049) or crosses node 2048
    v = c[f"tie-nodes-{n}"]
    ids = np.flatnonzero(v == 0.25)
    assert ids[0] == 1000 and np.all(np.diff(ids) == 1) and ids[-1] == min(2060, n) - 1 >= 2048
    s = np.sort(v)
    assert s[lo] == s[h] == 0.25
    # all equal: the median is the value and side 1 is empty
    med, exp = sc.median_expected(f"tie-all-equal-{n}")
    assert med == 0.25 and exp["n0"] == n and exp["n1"] == 0


def test_value_edges():
    c = sc.median_cases()
    for n in (2049, 2050):
        z = c[f"val-signed-zeros-{n}"]
        assert np.all(z == 0) and 0 < np.signbit(z).sum() < n
        assert sc.median_expected(f"val-signed-zeros-{n}")[0] == 0.0
        v = np.sort(c[f"val-inf-ends-{n}"])
        assert np.isneginf(v[:3]).all() and np.isposinf(v[-3:]).all() and np.isfinite(v[3:-3]).all()
        assert np.isfinite(sc.median_expected(f"val-inf-ends-{n}")[0])
        assert np.isposinf(c[f"val-inf-most-pos-{n}"]).sum() > n // 2 and np.isneginf(c[f"val-inf-most-pos-{n}"]).any()
        assert np.isneginf(c[f"val-inf-most-neg-{n}"]).sum() > n // 2 and np.isposinf(c[f"val-inf-most-neg-{n}"]).any()
        assert sc.median_expected(f"val-inf-most-pos-{n}")[0] == np.inf
        med, exp = sc.median_expected(f"val-inf-most-neg-{n}")
        assert med == -np.inf and exp["n1"] == 0
        d = c[f"val-denormals-{n}"]
        assert np.all(np.abs(d) < 2.2250738585072014e-308) and np.unique(d).size > n - 8 and (d < 0).any() and (d > 0).any()
        assert np.all(c[f"val-negative-{n}"] < 0)
        m = np.abs(c[f"val-magnitudes-{n}"])
        assert m.min() < 1e-290 and m.max() > 1e290 and m.min() >= 1e-300 and m.max() <= 1e300
    v = c["val-inf-halves-2050"]
    assert np.isneginf(v).sum() == np.isposinf(v).sum() == 1025
    med, exp = sc.median_expected("val-inf-halves-2050")
    assert med != med and exp["n0"] == 2050 and exp["n1"] == 0


def test_big_rank_case_blocks():
    rc = sc.rank_cases()
    v = sc.big_rank_vector()
    a, b = sc.BIG_RUN
    assert len(v) == sc.BIG_N and a == 261000 and b > 263100
    assert np.array_equal(np.flatnonzero(v == sc.BIG_C), np.arange(a, b))
    # the run crosses the block boundaries at 261,120, 262,144 and 263,168
    for edge in (261120, 262144, 263168):
        assert edge % sc.PART_BLOCK == 0 and a < edge < b
    below = int((v < sc.BIG_C).sum())
    want_block = {"blk254-last": 254, "blk255-first": 255, "blk255": 255, "blk256-first": 256, "blk256": 256,
                  "blk256-last": 256, "blk257": 257}
    assert set(want_block) == set(sc.big_rank_needs())
    for name, need in sc.big_rank_needs().items():
        _, n1 = rc[f"trip2-{name}"]
        assert n1 == below + need and 1 <= need <= b - a
        last = a + need - 1  # the last of the run's nodes side 1 takes
        assert last // sc.PART_BLOCK == want_block[name], name
        exp = sc.rank_expected(f"trip2-{name}")
        assert exp["side"][last] == 1 and (last + 1 == b or exp["side"][last + 1] == 0), name
        assert exp["n1"] == n1
    assert {"blk255", "blk256", "blk257"} <= set(want_block)
    assert rc["trip2-n1-1"][1] == 1 and rc["trip2-n1-last"][1] == sc.BIG_N - 1
    # blocks 256 and 257 hold keys below or equal to K in every one of these cases' counts:
    # a place block that drops the counts of the blocks from 256 on gets `need` wrong
    assert (v[256 * 1024:] <= sc.BIG_C).any()


# ---------------------------------------------------------------------------
# the reference against the host entry points
def test_median_reference_equals_host_median_split(ek):
    for name, v in sc.median_cases().items():
        med, bits = ek.median_split(v)
        want, exp = sc.median_expected(name)
        assert sc.same_value(med, want), (name, med, want)  # by ==; the NaN median of inf-halves as NaN
        if name != "val-inf-halves-2050":
            assert med == want, (name, med, want)
        assert np.array_equal(bits, exp["side"]), name
        assert exp["n0"] + exp["n1"] == len(v)


def test_rank_reference_equals_host_rank_split(ek):
    for name, (v, n1) in sc.rank_cases().items():
        assert np.array_equal(ek.rank_split(v, n1), sc.rank_expected(name)["side"]), name


def test_lists_ref():
    exp = sc.lists_ref(np.array([1, 0, 0, 1, 1, 0], np.uint8))
    assert exp["order0"].tolist() == [1, 2, 5] and exp["order1"].tolist() == [0, 3, 4]
    assert exp["plist"].tolist() == [0x80000000, 0, 1, 0x80000001, 0x80000002, 2]
    assert (exp["n0"], exp["n1"]) == (3, 3)


def test_ring_csr():
    for n in (1, 2, 3, 7):
        rowptr, col, w = sc.ring_csr(n)
        assert len(rowptr) == n + 1 and rowptr[-1] == len(col) == len(w) and np.all(w == 1)
        for i in range(n):
            nb = sorted({(i - 1) % n, (i + 1) % n} - {i})
            assert col[rowptr[i]:rowptr[i + 1]].tolist() == nb
