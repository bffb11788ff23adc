"""The KL shape cases (kl_cases.py) hold the shapes they are named for, and the
numpy reference they are checked against is cKL's KL().  No GPU:
test_gpu_kl_shapes.py runs the swap loops on the same cases.

The constants kl_cases.py restates are held to the sources as text
(csrc/ek_internal.hpp and csrc/kernels_kl.hip): the library exports none of
them.  reference_kl is pinned to the oracle (oracle/eko_kl.cpp, itself pinned
to the real cKL by test_oracle_golden.py) on every pin-derived case and on
fract; only then do the direct-CSR cases, which the oracle cannot take, rest
on it."""
import math
import os
import re

import numpy as np
import pytest

import kl_cases as kc
from conftest import PKG_DIR, circuit_path, eig_path, swap_fields_equal

CH = (kc.CHUNK, kc.CHUNK_GB)


@pytest.fixture(scope="module")
def cases():
    return kc.cases()


def _planted_counts(name, chunk=kc.CHUNK):
    c, r = kc.cases()[name], kc.reference(name)
    t = r.trace[0]
    assert (t.posA, t.posB) == c.planted, name   # swap 0 is the planted pair
    assert not np.any(np.isin([t.A, t.B], t.rows["node"]))   # the pair is not adjacent
    assert np.unique(t.rows["node"]).size == len(t.rows)     # and has no common neighbour
    return kc.swap_counts(t, chunk), t


def test_constants():
    hpp = open(os.path.join(PKG_DIR, "csrc", "ek_internal.hpp")).read()
    hip = open(os.path.join(PKG_DIR, "csrc", "kernels_kl.hip")).read()

    def const(src, pat):
        m = re.search(pat, src)
        assert m, pat
        return m.group(1)

    assert int(const(hpp, r"#define EK_KL_CHUNK (\d+)")) == kc.CHUNK
    assert int(const(hpp, r"#define EK_KL_CHUNK_GB (\d+)")) == kc.CHUNK_GB
    assert int(const(hpp, r"constexpr int KL_WDICT_CAP = (\d+);")) == kc.WDICT_CAP
    assert 2 * int(const(hpp, r"constexpr int KL_SEG_LANES = (\d+);")) == kc.INLINE
    assert int(const(hpp, r"constexpr int KL_ITEM_CAP = (\d+);")) == kc.ITEM_CAP
    assert int(const(hip, r"constexpr int KL_AB_CAP = (\d+);")) == kc.AB_CAP
    assert int(const(hip, r"constexpr int KL_STAGE_ROWS = (\d+);")) == kc.STAGE_ROWS
    assert const(hip, r"constexpr int KL_FIX_NCK = ([^;]+);") == "131072 / KL_CHUNK" and 131072 // kc.CHUNK == kc.FIX_NCK
    bad = re.findall(r"any_tag \|\| tot > (\d+) \|\|", hip)   # (the swap loop and the overlapped one)
    assert len(bad) == 2 and set(bad) == {str(kc.BAD_TOT)}
    assert const(hip, r"return \(m \+ (\d+)\) / \d+ \* \d+;") == str(kc.SEL_PAD - 1)
    # rows a gain wave takes per pass: 64 lanes over 4 (coded) or 8 (plain) lanes a row; three gain waves
    assert const(hip, r"constexpr int LPR = SEGC \? (\d+ : \d+), RPW = 64 / LPR;") == "4 : 8"
    assert 64 // 4 == kc.STAGE_ROWS and 64 // 8 == kc.STAGE_ROWS_PLAIN
    threads = int(const(hpp, r"#define EK_KL_THREADS (\d+)"))
    eparts = int(const(hip, r"#define EK_KL_EPARTS (\d+)"))
    assert threads // 64 - 1 - 2 * eparts == kc.GAIN_WAVES


@pytest.mark.parametrize("name", list(kc.cases()))
def test_case_is_valid(cases, name):
    c, r = cases[name], kc.reference(name)
    if c.pins is None:
        kc.check_csr(c.rowptr, c.col, c.w)
    assert r.res["iterations"] == len(r.log) == len(r.trace) >= 1
    assert (r.stop == "side") == (r.res["iterations"] == min(len(c.order0), len(c.order1)))
    # the initial cut does not hang on the order of its fp64 sum
    side = r.sides_init
    _, ext = kc.all_gains(c.rowptr.astype(np.int64), c.col, c.w, side)
    assert np.float32(math.fsum(ext[side == 0].astype(np.float64))) == r.res["initial_cut"]
    if name not in kc.LONG:
        assert c.n <= 17000


def test_row_gain_is_sequential(cases):
    c = cases["order-matters"]
    side = kc.reference("order-matters").sides_init
    rp = c.rowptr.astype(np.int64)
    g, _ = kc.all_gains(rp, c.col, c.w, side)
    for u in range(0, c.n, 7):
        a = kc.row_gain_loop(rp, c.col, c.w, side, u)
        assert a.view(np.uint32) == kc.row_gain(rp, c.col, c.w, side, u).view(np.uint32) == g[u].view(np.uint32)


@pytest.mark.parametrize("N,ch", [(2047, kc.CHUNK), (2048, kc.CHUNK), (2049, kc.CHUNK), (4096, kc.CHUNK_GB),
                                  (4097, kc.CHUNK_GB)])
def test_list_cases(cases, N, ch):
    c, r = cases[f"list-{N}"], kc.reference(f"list-{N}")
    n1 = len(c.order1)
    assert len(c.order0) == N and -(-N // ch) == (1 if N <= ch else 2) and -(-n1 // ch) == 3
    t0, t1 = r.trace[0], r.trace[1]
    assert (t0.posA, t0.posB) == (N - 1, n1 - 1)          # the last valid position of each list
    assert t1.posB == (n1 - 1) // ch * ch and t1.posB % kc.CHUNK == 0   # the first position of the last chunk
    assert t1.posA == 0                                   # and of a chunk of list 0
    assert r.log["gain"][0] > r.log["gain"][1] > 0 and r.res["iterations"] > 2


def test_loop_ends(cases):
    for name, n0, n1 in (("one-node-side-n0", 1, 50), ("one-node-side-n1", 50, 1)):
        c, r = cases[name], kc.reference(name)
        assert (len(c.order0), len(c.order1)) == (n0, n1)
        assert r.res["iterations"] == 1 and r.stop == "side"
    c, r = cases["limit-0"], kc.reference("limit-0")
    assert c.limit == 0 and r.limit == 0 and r.stop == "limit"
    assert r.log["gain"][-1] <= 0 and np.all(r.log["gain"][:-1] > 0) and r.res["iterations"] > 10
    r = kc.reference("no-gain")
    assert np.all(r.log["gain"] <= 0) and r.res["best_iter"] == 0 and r.stop == "limit"
    assert r.res["iterations"] == r.limit + 1 == int(math.log2(200)) + 6
    assert np.array_equal(r.sides_best, r.sides_init) and not np.array_equal(r.sides_final, r.sides_init)
    assert r.res["best_cut"] == r.res["initial_cut"]
    c, r = cases["best-is-last"], kc.reference("best-is-last")
    assert np.all(r.log["gain"] > 0) and r.stop == "side"
    assert r.res["best_iter"] == r.res["iterations"] == len(c.order0) == 40
    assert np.array_equal(r.sides_best, r.sides_final)


@pytest.mark.parametrize("name", ["ties-ring", "ties-grid"])
def test_ties(cases, name):
    c, r = cases[name], kc.reference(name)
    n0 = len(c.order0)
    assert np.all(c.w == 1) and n0 == len(c.order1) and kc.CHUNK < n0 < 2 * kc.CHUNK
    assert np.array_equal(c.order0, np.arange(n0)) and np.array_equal(c.order1, np.arange(n0, 2 * n0))
    assert r.stop == "side" and r.res["iterations"] == n0
    # nearly every swap is decided among equal gains, on both lists, on both sides of the chunk end
    g = kc.all_gains(c.rowptr.astype(np.int64), c.col, c.w, r.sides_init)[0]
    assert np.count_nonzero(g[c.order0] == g[c.order0].max()) >= 2
    for f in ("max_gain", "min_gain"):
        v, k = np.unique(r.log[f], return_counts=True)
        assert v.size <= 8 and k.max() > n0 // 4
    posA = np.array([t.posA for t in r.trace])
    posB = np.array([t.posB for t in r.trace])
    for p in (posA, posB):
        assert np.any(p < kc.CHUNK) and np.any(p >= kc.CHUNK)
        assert np.count_nonzero(np.diff(p // kc.CHUNK)) >= 1


@pytest.mark.parametrize("name,k0,k1", [("own-chunk-16", 16, 16), ("own-chunk-17", 17, 17), ("own-chunk-17-16", 17, 16),
                                        ("own-chunk-16-17", 16, 17)])
def test_own_chunk(cases, name, k0, k1):
    c = cases[name]
    assert len(c.order0) <= kc.CHUNK and len(c.order1) <= kc.CHUNK   # one chunk a list
    for ch in CH:
        s, _ = _planted_counts(name, ch)
        assert s == {"tot": k0 + k1, "own0": k0, "own1": k1, "other": 0, "locked": 0}
    assert kc.AB_CAP == 16


@pytest.mark.parametrize("k", [16, 17])
def test_own_chunk_last(cases, k):
    name = f"own-chunk-{k}-last"
    c, r = cases[name], kc.reference(name)
    s, t = _planted_counts(name)
    assert s == {"tot": 49, "own0": k, "own1": 49 - k, "other": 0, "locked": 0}
    last = t.rows[-1]   # entry 48: alone in the last staging pass at 16 and at 8 rows a wave
    assert len(t.rows) - 1 == kc.GAIN_WAVES * kc.STAGE_ROWS == 2 * kc.GAIN_WAVES * kc.STAGE_ROWS_PLAIN
    assert last["list"] == 0 and last["active"] and np.count_nonzero(t.rows["list"][:48] == 0) == k - 1
    g0 = r.gains0[c.order0].copy()
    g0[t.posA] = -np.inf
    assert int(np.argmax(g0)) == last["pos"] and last["old"] == np.float32(96.5) and last["new"] == np.float32(-95.5)
    assert r.trace[1].A != last["node"] and r.log["max_gain"][1] < last["old"]   # its old gain must not be selected


@pytest.mark.parametrize("K", [64, 65, 256, 257])
def test_other_chunks(cases, K):
    name = f"other-{K}"
    c, r = cases[name], kc.reference(name)
    for ch in CH:
        assert -(-len(c.order0) // ch) >= 3 and -(-len(c.order1) // ch) >= 3
        s, _ = _planted_counts(name, ch)
        assert s == {"tot": K, "own0": 0, "own1": 0, "other": K, "locked": 0}
        fallen, risen = kc.winner_moves(c, r, ch)
        for lst in (0, 1):   # on each list a tagged chunk and a merged one, apart
            f = {x for x in fallen if x[0] == lst}
            u = {x for x in risen if x[0] == lst}
            assert len(f) == 1 and len(u) == 1 and not (f & u)
    assert (K > kc.BAD_TOT) == (K in (65, 256, 257)) and (K > kc.ITEM_CAP) == (K == 257)


@pytest.mark.parametrize("L", [31, 32, 33, 64, 65])
def test_rowlen(cases, L):
    name = f"rowlen-{L}"
    c, r = cases[name], kc.reference(name)
    s, t = _planted_counts(name)
    assert s["tot"] == 12 and s["locked"] == 0
    assert np.all(t.rows["len"] == L)
    lens = np.diff(c.rowptr)
    assert np.array_equal(np.sort(np.array(c.nbr_nodes)), np.sort(t.rows["node"]))
    assert lens.max() == L and np.count_nonzero(lens == L) == 12
    for u in t.rows["node"]:
        for e in (31, 32):   # the entries on either side of the inline edge: on side 1, and the sum's bits hang on them
            if e < L:
                p = c.rowptr[u] + e
                assert r.sides_init[c.col[p]] == 1 and c.w[p] > 0
                w2 = c.w.copy()
                w2[p] = 0
                rp = c.rowptr.astype(np.int64)
                assert kc.row_gain(rp, c.col, w2, r.sides_init, u) != kc.row_gain(rp, c.col, c.w, r.sides_init, u)
    assert np.unique(c.w).size < kc.WDICT_CAP - 1


@pytest.mark.parametrize("K", [7, 8, 9, 15, 16, 17, 24, 25, 48, 49])
def test_stage(K):
    s, _ = _planted_counts(f"stage-{K}")
    assert s["tot"] == K == s["own0"] + s["own1"] and s["locked"] == 0
    # wave ends at 8 / 16 rows, pass ends at 24 / 48 (plain / coded inline rows)
    assert kc.GAIN_WAVES * kc.STAGE_ROWS_PLAIN == 24 and kc.GAIN_WAVES * kc.STAGE_ROWS == 48


def _pairwise(x):
    if len(x) <= 1:
        return np.float32(x[0]) if len(x) else np.float32(0)
    h = len(x) // 2
    return np.float32(_pairwise(x[:h]) + _pairwise(x[h:]))


def test_order_matters(cases):
    c, r = cases["order-matters"], kc.reference("order-matters")
    lens = np.diff(c.rowptr)
    assert lens.min() >= 20 and lens.max() <= 40
    assert np.unique(c.w.view(np.uint32)).size < kc.WDICT_CAP - 1   # the coded form runs
    assert c.w.min() < 2.0 ** -18 and c.w.max() > 2.0 ** 3 and c.w.min() >= 2.0 ** -20 and c.w.max() <= 2.0 ** 5
    side = r.sides_init
    differ_pw = differ_sorted = 0
    for u in range(c.n):
        a, b = c.rowptr[u], c.rowptr[u + 1]
        ww, s0 = c.w[a:b], side[c.col[a:b]] == 0
        seq = [np.cumsum(x, dtype=np.float32)[-1] if x.size else np.float32(0) for x in (ww[s0], ww[~s0])]
        pw = [_pairwise(x) for x in (ww[s0], ww[~s0])]
        so = [np.cumsum(np.sort(x), dtype=np.float32)[-1] if x.size else np.float32(0) for x in (ww[s0], ww[~s0])]
        differ_pw += np.float32(seq[1] - seq[0]) != np.float32(pw[1] - pw[0])
        differ_sorted += np.float32(seq[1] - seq[0]) != np.float32(so[1] - so[0])
    assert differ_pw > c.n // 2 and differ_sorted > c.n // 2, (differ_pw, differ_sorted, c.n)
    assert r.res["iterations"] > 100


def test_wdict(cases):
    a = cases["wdict-4096"]
    for N in (4095, 4096, 4097):
        c = cases[f"wdict-{N}"]
        assert np.unique(c.w.view(np.uint32)).size == N and not np.any(c.w == 0)
        assert np.array_equal(c.rowptr, a.rowptr) and np.array_equal(c.col, a.col)
        assert kc.reference(f"wdict-{N}").res["iterations"] > 100
    # code 0 is the padding's 0.0f, so the table holds 4095 weights: 4095 is the last coded count
    assert kc.WDICT_CAP == 4096


@pytest.mark.parametrize("nets", [256, 257])
def test_nets_edge(cases, nets):
    c, r = cases[f"nets-edge-{nets}"], kc.reference(f"nets-edge-{nets}")
    assert len(c.net_ptr) - 1 == nets and -(-nets // 256) == (1 if nets == 256 else 2)
    net = lambda e: c.pins[c.net_ptr[e]:c.net_ptr[e + 1]]
    e_empty, e_one, e_rep, e_s0, e_s1 = c.special
    assert len(net(e_empty)) == 0 and len(net(e_one)) == 1
    assert len(net(e_rep)) == 3 and np.unique(net(e_rep)).size == 2
    assert np.all(r.sides_init[net(e_s0)] == 0) and np.all(r.sides_init[net(e_s1)] == 1)
    cut = lambda e, s: len(net(e)) > 0 and bool(np.any(s[net(e)] != s[net(e)[0]]))
    recut = [e for e in range(nets) if cut(e, r.sides_init) and not cut(e, r.sides_best) and cut(e, r.sides_final)]
    assert len(recut) >= 1
    assert 0 < r.res["best_iter"] < r.res["iterations"]


@pytest.mark.parametrize("name,nck", [("sel-pad-33", kc.SEL_PAD), ("fix-65", kc.FIX_NCK)])
def test_long_lists(cases, name, nck):
    c, r = cases[name], kc.reference(name)
    n0, n1 = len(c.order0), len(c.order1)
    assert (n0, n1) == (nck * kc.CHUNK, nck * kc.CHUNK + 1)
    assert -(-n0 // kc.CHUNK) == nck and -(-n1 // kc.CHUNK) == nck + 1   # the longer list alone crosses the step
    assert np.all(c.w == 1) and np.all(np.diff(c.rowptr) == 2) and c.limit == 3
    # the planted misplaced nodes are swapped first, gain 4 each, some from the long list's last chunk
    k = c.nmis
    assert np.all(r.log["gain"][:k] == 4) and np.all(r.log["gain"][k:] <= 0)
    assert r.res["best_iter"] == k and r.res["iterations"] == k + 4 and r.stop == "limit"
    posB = np.array([t.posB for t in r.trace[:k]])
    posA = np.array([t.posA for t in r.trace[:k]])
    assert np.count_nonzero(posB // kc.CHUNK == nck) == 1 and np.any(posB // kc.CHUNK == 0)
    assert np.all(posA // kc.CHUNK == nck - 1)


# ------------------------------------------------------- reference == oracle
def _against_oracle(g, o0, o1, limit=-1):
    rowptr, col, w, _ = g.kl_csr()
    r = kc.reference_kl(rowptr, col, w, o0, o1, limit)
    olog, ores = g.kl(np.asarray(o0), np.asarray(o1), limit)
    swap_fields_equal(r.log, olog)
    for k in ("iterations", "best_iter"):
        assert r.res[k] == ores[k], k
    for k in ("initial_cut", "best_cut", "final_cut"):
        assert np.float32(r.res[k]).view(np.uint32) == np.float32(ores[k]).view(np.uint32), k
    assert g.net_cut(r.sides_init) == ores["net_cut_initial"]
    assert g.net_cut(r.sides_best) == ores["net_cut_best"]
    assert g.net_cut(r.sides_final) == ores["net_cut_final"]
    return r, ores


@pytest.mark.parametrize("nets", [256, 257])
def test_reference_is_the_oracle_on_pin_cases(cases, oracle, nets):
    c = cases[f"nets-edge-{nets}"]
    g = oracle.Graph.from_pins(c.n, c.net_ptr, c.pins)
    r, ores = _against_oracle(g, c.order0, c.order1, c.limit)
    for k, s in (("net_cut_initial", r.sides_init), ("net_cut_best", r.sides_best), ("net_cut_final", r.sides_final)):
        assert kc.net_cut(c.net_ptr, c.pins, s) == ores[k]
    _against_oracle(g, c.order0, c.order1, 0)


@pytest.mark.parametrize("split", ["golden", "random"])
def test_reference_is_the_oracle_on_fract(oracle, split):
    g = oracle.Graph.read(circuit_path("fract"))
    if split == "golden":
        _, _, _, _, o0, o1 = oracle.read_eig_file(eig_path("fract"))
    else:
        o0, o1 = oracle.random_split(g.nodes, 5)
    r, _ = _against_oracle(g, o0, o1)
    assert r.res["iterations"] > 5
