"""Shape cases for the KL swap loops (csrc/kernels_kl.hip) and a plain numpy
reference of cKL's KL() over an arbitrary fp32 CSR.

reference_kl is written from the parity rules at the top of kernels_kl.hip and
from oracle/eko_kl.cpp, not from the kernels; test_kl_cases_host.py pins it to
the oracle on pin-derived graphs before it is trusted on direct-CSR ones.

How the swap loop counts (read from G1 of k_kl_swap_loop, restated in
swap_counts):
  * tot = len(row node1) + len(row node2): every stored entry of the two rows,
    locked rows, the pair's own rows (when node1 and node2 are adjacent) and a
    common neighbour's second occurrence included.  tot decides the staging
    passes (16 rows a gain wave with coded inline rows, 8 with plain ones,
    three gain waves), the "bad" path (tot > 64) and the LDS item list
    (entries 256 and up are rederived in G2c).
  * Only unlocked rows other than the pair get a new gain.  Of those, the ones
    on list 0 in node1's chunk and the ones on list 1 in node2's chunk go to
    the two short lists (own0 / own1, more than 16: the chunk is rescanned);
    locked rows and the pair's own rows do not count there.  The rest are
    "other" rows: a risen key is merged, a fallen winner tags its chunk.
The planted cases keep node1 and node2 apart, give them no common neighbour and
run swap 0 with nothing locked, so tot = own0 + own1 + other there.

A planted pair: node1 has two anchor neighbours of weight 64 on side 1 and
node2 two on side 0, so gain(node1) is about +128 and gain(node2) about -128
while every other |gain| stays under 100: swap 0 is known.
"""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

F32 = np.float32
SWAP_DTYPE = np.dtype([("iter", "<u4"), ("node_left", "<u4"), ("node_right", "<u4"),
                       ("max_gain", "<f4"), ("min_gain", "<f4"), ("gain", "<f4"),
                       ("cut", "<f4"), ("pad", "<u4")])
ROW_DTYPE = np.dtype([("node", "<i4"), ("list", "<i4"), ("pos", "<i8"), ("len", "<i4"), ("active", "?"),
                      ("old", "<f4"), ("new", "<f4")])

# the loop's branch points (asserted against the sources by test_kl_cases_host.py)
CHUNK, CHUNK_GB = 2048, 4096   # positions per chunk key (LDS forms / off-chip-bitmap form)
AB_CAP = 16                    # updated rows kept per own chunk
BAD_TOT = 64                   # tot above it: the "bad" path
ITEM_CAP = 256                 # LDS item list
INLINE = 32                    # inline row entries (2 * KL_SEG_LANES)
STAGE_ROWS, STAGE_ROWS_PLAIN, GAIN_WAVES = 16, 8, 3
FIX_NCK = 64                   # chunks per list of the fixed LDS layout
SEL_PAD = 32                   # kl_sel_pad's step
WDICT_CAP = 4096               # weight codes (code 0 is the padding's 0.0f)


# ------------------------------------------------------------------ reference
def check_csr(rowptr, col, w):
    """What the loop's edge lookup and neighbour updates assume of a CSR given directly."""
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    c = col.astype(np.int64)
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(w) and np.all(np.diff(rowptr) >= 0)
    assert len(c) == 0 or (c.min() >= 0 and c.max() < n)
    assert not np.any(row == c), "self loop"
    k, kt = row * n + c, c * n + row
    assert np.unique(k).size == k.size, "repeated column in a row"
    a, b = np.argsort(k), np.argsort(kt)
    assert np.array_equal(k[a], kt[b]), "not structurally symmetric"
    assert np.array_equal(w[a].view(np.uint32), w[b].view(np.uint32)), "weights differ between the two directions"
    assert np.all(np.isfinite(w))


def all_gains(rowptr, col, w, side):
    """gain(u) = E - I and E for every row: fp32 accumulators run left to right
    over the row as stored (entry k of every row at step k), I over side 0."""
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    I, E = np.zeros(n, F32), np.zeros(n, F32)
    for k in range(int(lens.max()) if n else 0):
        rows = np.flatnonzero(lens > k)
        p = rowptr[rows] + k
        s0 = side[col[p]] == 0
        wk = w[p]
        I[rows] = I[rows] + np.where(s0, wk, F32(0))   # + 0.0f leaves a sum (never -0) unchanged
        E[rows] = E[rows] + np.where(s0, F32(0), wk)
    return E - I, E


def row_gain(rowptr, col, w, side, u):
    a, b = int(rowptr[u]), int(rowptr[u + 1])
    if a == b:
        return F32(0)
    s0 = side[col[a:b]] == 0
    ww = w[a:b]
    # np.cumsum adds strictly in order, in the dtype given
    I = np.cumsum(np.where(s0, ww, F32(0)), dtype=F32)[-1]
    E = np.cumsum(np.where(s0, F32(0), ww), dtype=F32)[-1]
    return F32(E - I)


def row_gain_loop(rowptr, col, w, side, u):
    """row_gain spelt out (the host test holds row_gain to it)."""
    I, E = F32(0), F32(0)
    for p in range(int(rowptr[u]), int(rowptr[u + 1])):
        if side[col[p]] == 0:
            I = F32(I + w[p])
        else:
            E = F32(E + w[p])
    return F32(E - I)


def reference_kl(rowptr, col, w, order0, order1, limit=-1):
    """cKL's KL() (cKL.cpp:288-406) over an fp32 CSR from the given remain[] lists."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int32)
    w = np.asarray(w, F32)
    order0 = np.asarray(order0, np.int64)
    order1 = np.asarray(order1, np.int64)
    n, n0, n1 = len(rowptr) - 1, len(order0), len(order1)
    side = np.full(n, 2, np.uint8)
    side[order0] = 0
    side[order1] = 1
    assert n0 + n1 == n and not np.any(side == 2)
    lst = side.astype(np.int32)
    pos = np.empty(n, np.int64)
    pos[order0] = np.arange(n0)
    pos[order1] = np.arange(n1)
    lens = np.diff(rowptr).astype(np.int32)
    lim = int(limit) if limit >= 0 else int(math.log2(n)) + 5
    side_init = side.copy()

    gains, ext = all_gains(rowptr, col, w, side)
    gains0 = gains.copy()
    # initial cut: fp64 sum, by ascending node, of the side-0 rows' fp32 external sums, rounded once
    e0 = ext[side == 0].astype(np.float64)
    cut = F32(np.cumsum(e0)[-1]) if e0.size else F32(0)
    initial_cut = best = cut
    best_iter = 0
    g0 = gains[order0].copy()   # by position; a locked position never wins
    g1 = gains[order1].copy()
    assert np.all(np.isfinite(g0)) and np.all(np.isfinite(g1))
    locked = np.zeros(n, bool)
    log, trace = [], []
    it = term = 0
    stop = "side"
    while it < n0 and it < n1:
        i, j = int(np.argmax(g0)), int(np.argmin(g1))   # the first position of the maximum / minimum
        max_gain, min_gain = g0[i], g1[j]
        a, b = int(order0[i]), int(order1[j])
        ra = col[rowptr[a]:rowptr[a + 1]]
        rb = col[rowptr[b]:rowptr[b + 1]]
        hit = np.flatnonzero(ra == b)
        wab = w[rowptr[a] + hit[0]] if hit.size else F32(0)
        gain = F32(F32(max_gain - min_gain) - F32(F32(2) * wab))
        cut = F32(cut - gain)
        if cut < best:
            best, best_iter = cut, it + 1
        locked[a] = locked[b] = True
        side[a], side[b] = 1, 0
        g0[i], g1[j] = -np.inf, np.inf
        ent = np.concatenate([ra, rb]).astype(np.int64)
        rows = np.zeros(len(ent), ROW_DTYPE)
        rows["node"], rows["list"], rows["pos"], rows["len"] = ent, lst[ent], pos[ent], lens[ent]
        rows["active"] = ~locked[ent]
        rows["old"] = gains[ent]
        for u in np.unique(ent[~locked[ent]]):
            g = row_gain(rowptr, col, w, side, u)
            gains[u] = g
            (g1 if lst[u] else g0)[pos[u]] = g
        rows["new"] = gains[ent]
        it += 1
        log.append((it, a, b, max_gain, min_gain, gain, cut, 0))
        trace.append(SimpleNamespace(posA=i, posB=j, A=a, B=b, la=len(ra), lb=len(rb), rows=rows))
        if gain <= 0:
            term += 1
            if term > lim:
                stop = "limit"
                break
        else:
            term = 0
    log = np.array(log, SWAP_DTYPE) if log else np.zeros(0, SWAP_DTYPE)
    sides_best = side_init.copy()
    sides_best[log["node_left"][:best_iter]] = 1
    sides_best[log["node_right"][:best_iter]] = 0
    res = {"iterations": it, "best_iter": best_iter, "initial_cut": F32(initial_cut), "best_cut": F32(best),
           "final_cut": F32(cut)}
    return SimpleNamespace(log=log, res=res, sides_init=side_init, sides_best=sides_best, sides_final=side.copy(),
                           trace=trace, stop=stop, gains0=gains0, limit=lim)


def swap_counts(t, chunk):
    """The swap loop's item counts of one traced swap at `chunk` positions a key (module docstring)."""
    r = t.rows
    cA, cB = t.posA // chunk, t.posB // chunk
    act = r["active"]
    own0 = int(np.count_nonzero(act & (r["list"] == 0) & (r["pos"] // chunk == cA)))
    own1 = int(np.count_nonzero(act & (r["list"] == 1) & (r["pos"] // chunk == cB)))
    n_act = int(np.count_nonzero(act))
    return {"tot": len(r), "own0": own0, "own1": own1, "other": n_act - own0 - own1, "locked": len(r) - n_act}


def winner_moves(case, ref, chunk):
    """Swap 0 against the chunk winners before it: (fallen, risen) as sets of
    (list, chunk) other than the pair's chunks.  fallen: the chunk's winner is an
    updated row whose new key is worse; risen: an updated row's new key beats
    the chunk's old winner."""
    t = ref.trace[0]
    fallen, risen = set(), set()
    for s, order in ((0, case.order0), (1, case.order1)):
        g = ref.gains0[order] * (F32(-1) if s else F32(1))   # larger is better on both lists
        own = (t.posB if s else t.posA) // chunk
        for r in t.rows[t.rows["active"] & (t.rows["list"] == s)]:
            c = int(r["pos"]) // chunk
            if c == own:
                continue
            lo = c * chunk
            win = lo + int(np.argmax(g[lo:lo + chunk]))
            new = -r["new"] if s else r["new"]
            if win == r["pos"] and new < g[win]:
                fallen.add((s, c))
            elif new > g[win] or (new == g[win] and r["pos"] < win):
                risen.add((s, c))
    return fallen, risen


def net_cut(net_ptr, pins, sides):
    """Nets with pins on both sides."""
    cut = 0
    for e in range(len(net_ptr) - 1):
        s = sides[pins[net_ptr[e]:net_ptr[e + 1]]]
        cut += int(s.size > 0 and np.any(s != s[0]))
    return cut


# ---------------------------------------------------------------------- cases
class Builder:
    """Rows in insertion order: edge(u, v, w) appends v to row u and u to row v."""

    def __init__(self, n):
        self.n = n
        self.rows = [[] for _ in range(n)]

    def edge(self, u, v, w):
        self.rows[u].append((v, w))
        self.rows[v].append((u, w))

    def csr(self):
        lens = np.array([len(r) for r in self.rows], np.int64)
        rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        col = np.array([v for r in self.rows for v, _ in r], np.int32)
        w = np.array([x for r in self.rows for _, x in r], F32)
        return rowptr, col, w


def _case(name, rowptr, col, w, order0, order1, limit=-1, direct=True, **meta):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    col = np.ascontiguousarray(col, np.int32)
    w = np.ascontiguousarray(w, F32)
    if direct:
        check_csr(rowptr, col, w)
    c = SimpleNamespace(name=name, n=len(rowptr) - 1, rowptr=rowptr, col=col, w=w,
                        order0=np.ascontiguousarray(order0, np.int32), order1=np.ascontiguousarray(order1, np.int32),
                        limit=limit, net_ptr=None, pins=None, **meta)
    assert len(np.unique(np.concatenate([c.order0, c.order1]))) == c.n == len(c.order0) + len(c.order1)
    return c


def _lists(n0, n1, seed):
    ids = np.random.default_rng(seed).permutation(n0 + n1)
    return ids[:n0], ids[n0:]


def planted(name, n0, n1, posA, posB, x, z, y, v, seed, rowlen=0, limit=-1, ring=False, second=None, last_y=None):
    """One planted pair.  x / z: list-1 / list-0 positions of node1's neighbours,
    y / v: list-0 / list-1 positions of node2's; the first two of x and of y are
    the anchors.  Each other neighbour gets one leaf of its own on the far side
    (a distinct weight each), or, with rowlen, every neighbour row is filled to
    exactly rowlen entries with entries 31 and 32 on side 1.  A leaf is no
    neighbour of the pair, so where it sits changes no count.  last_y: one more
    list-0 neighbour of node2, the last entry of its row, tied to it by weight 96
    with a leaf of 0.5: the best gain of list 0 after node1 before the swap
    (96.5, above the anchors' 64), far from it after (-95.5)."""
    rng = np.random.default_rng(seed)
    o0, o1 = _lists(n0, n1, seed)
    b = Builder(n0 + n1)
    used0 = set([posA]) | set(z) | set(y)
    used1 = set([posB]) | set(x) | set(v)
    if last_y is not None:
        used0.add(last_y)
    if second:
        used0 |= {second[0]} | set(second[3])
        used1 |= {second[1]} | set(second[2])
    free0 = iter([p for p in range(n0) if p not in used0])   # leaves: the unused positions, ascending
    free1 = iter([p for p in range(n1) if p not in used1])
    A, B = int(o0[posA]), int(o1[posB])
    k = [0]

    def fill(u, far, near, leaf_w):
        # u's row after its pair edge: one leaf, or rowlen - 1 of them
        if not rowlen:
            if leaf_w is not None:
                k[0] += 1
                b.edge(u, far(), F32(leaf_w + k[0] / 1024.0))
            return
        for e in range(1, rowlen):
            on1 = e in (31, 32) or e % 2 == 1
            leaf = int(o1[next(free1)]) if on1 else int(o0[next(free0)])
            b.edge(u, leaf, F32(rng.uniform(0.5, 1.5) / 16))

    f0 = lambda: int(o0[next(free0)])
    f1 = lambda: int(o1[next(free1)])
    for i, p in enumerate(x):
        u = int(o1[p])
        b.edge(A, u, F32(64 if i < 2 else 1))
        fill(u, f0, f1, None if i < 2 else 2.0)
    for p in z:
        u = int(o0[p])
        b.edge(A, u, F32(0.25))
        fill(u, f1, f0, 0.5)
    for i, p in enumerate(y):
        u = int(o0[p])
        b.edge(B, u, F32(64 if i < 2 else 1))
        fill(u, f1, f0, None if i < 2 else 2.0)
    for p in v:
        u = int(o1[p])
        b.edge(B, u, F32(0.25))
        fill(u, f0, f1, 3.5)
    if last_y is not None:
        b.edge(B, int(o0[last_y]), F32(96))
        b.edge(int(o0[last_y]), f1(), F32(0.5))
    if second:  # a second, weaker pair: (posA', posB', its list-1 neighbours, its list-0 neighbours)
        A2, B2 = int(o0[second[0]]), int(o1[second[1]])
        for p in second[2]:
            b.edge(A2, int(o1[p]), F32(40))
        for p in second[3]:
            b.edge(B2, int(o0[p]), F32(40))
    if ring:  # unit-weight rings along each list: a background of tied gains
        for o in (o0, o1):
            for i in range(len(o)):
                if len(o) > 2:
                    b.edge(int(o[i]), int(o[(i + 1) % len(o)]), F32(1))
    return _case(name, *b.csr(), o0, o1, limit=limit, planted=(posA, posB), rowlen=rowlen,
                 nbr_nodes=[int(o1[p]) for p in list(x) + list(v)] + [int(o0[p]) for p in list(z) + list(y)])


def _split(k):
    """la or lb entries: two anchors, the rest halved between the far and the near side."""
    rest = k - 2
    return 2 + rest - rest // 2, rest // 2


def _list_case(N, ch):
    # list 0 has N positions; list 1 three chunks of `ch`.  Swap 0's pair sits at the
    # last valid position of each list, swap 1's at the first position of each last chunk.
    n1 = 2 * ch + 904
    lastc0, lastc1 = (N - 1) // ch * ch, (n1 - 1) // ch * ch
    second = (lastc0 if lastc0 != N - 1 else max(lastc0 - ch, 0), lastc1, [3, 4], [3, 4])
    return planted(f"list-{N}", N, n1, N - 1, n1 - 1, [1, 2], [], [1, 2], [], seed=N, ring=True, second=second,
                   limit=4)


def _random_graph(n, deg, rng, weights):
    b = Builder(n)
    seen = set()
    for u in range(n):
        for _ in range(deg):
            v = int(rng.integers(n))
            if v != u and (u, v) not in seen and (v, u) not in seen:
                seen.add((u, v))
                b.edge(u, v, weights(len(seen)))
    return b


def _ring_long(name, n0, n1, nmis=6):
    """Ring of unit weights by node id, contiguous halves, nmis misplaced nodes a side."""
    n = n0 + n1
    ids = np.arange(n, dtype=np.int64)
    rowptr = 2 * np.arange(n + 1, dtype=np.int32)
    col = np.stack([(ids - 1) % n, (ids + 1) % n], axis=1).reshape(-1).astype(np.int32)
    w = np.ones(2 * n, F32)
    lo = np.arange(n0)            # ids of the first half
    hi = np.arange(n0, n)
    mis_lo = lo[np.linspace(1000, n0 - 1000, nmis).astype(int)]   # first-half ids put on list 1
    mis_hi = hi[np.linspace(1000, n1 - 1000, nmis).astype(int)]   # second-half ids put on list 0
    order0 = np.concatenate([np.setdiff1d(lo, mis_lo), mis_hi])   # its misplaced nodes in the last chunk
    keep_hi = np.setdiff1d(hi, mis_hi)
    order1 = np.concatenate([mis_lo[:nmis // 2], keep_hi, mis_lo[nmis // 2:]])   # half first, half in the last chunk
    assert len(order0) == n0 and len(order1) == n1
    return _case(name, rowptr, col, w, order0, order1, limit=3, nmis=nmis)


def _pins_case(name, nets, oracle, seed):
    rng = np.random.default_rng(seed)
    n = 300
    o0, o1 = _lists(150, 150, seed)
    groups = [[], [int(o0[5])], [int(o0[7]), int(o0[7]), int(o1[9])], [int(o0[i]) for i in (11, 12, 13)],
              [int(o1[i]) for i in (11, 12, 13)]]  # empty, 1 pin, a repeated pin, wholly on side 0 / side 1
    while len(groups) < nets:
        k = int(rng.integers(2, 6))
        groups.append([int(t) for t in rng.choice(n, k, replace=False)])
    order = rng.permutation(len(groups))
    groups = [groups[i] for i in order]
    net_ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    pins = np.array([p for g in groups for p in g], np.int32)
    g = oracle.Graph.from_pins(n, net_ptr, pins)
    rowptr, col, w, _ = g.kl_csr()
    c = _case(name, rowptr, col, w, o0, o1, direct=False)
    c.net_ptr, c.pins, c.special = net_ptr, pins, [int(np.flatnonzero(order == i)[0]) for i in range(5)]
    return c


_CASES = None


def cases(oracle=None):
    """name -> case.  The pin-derived ones need the oracle module (their CSR is cKL's own)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    if oracle is None:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
        import oracle
    C = {}

    def add(c):
        assert c.name not in C
        C[c.name] = c

    for N in (2047, 2048, 2049):
        add(_list_case(N, CHUNK))
    for N in (4096, 4097):
        add(_list_case(N, CHUNK_GB))

    # ends of the loop
    for nm, n0, n1 in (("one-node-side-n0", 1, 50), ("one-node-side-n1", 50, 1)):
        rng = np.random.default_rng(7)
        b = _random_graph(n0 + n1, 3, rng, lambda k: F32(0.25 * (1 + k % 7)))
        add(_case(nm, *b.csr(), *_lists(n0, n1, 7)))
    rng = np.random.default_rng(8)
    b = _random_graph(400, 3, rng, lambda k: F32(0.125 * (1 + k % 11)))
    add(_case("limit-0", *b.csr(), *_lists(200, 200, 8), limit=0))
    # no-gain: 30 unit edges a node inside each side (more than the limit's 13 swaps can undo), a few light ones across
    b = Builder(200)
    for s in (0, 100):
        for i in range(100):
            for d in range(1, 16):
                b.edge(s + i, s + (i + d) % 100, F32(1))
    for i in range(0, 100, 9):
        b.edge(i, 100 + (i * 3) % 100, F32(0.5))
    add(_case("no-gain", *b.csr(), np.arange(100), np.arange(100, 200)))
    # best-is-last: p_i - r_i cut edges (distinct weights), the r's held by a heavy ring, q's isolated;
    # every swap (p_i, q_j) gains w_i > 0 until list 0 is empty
    m = 40
    b = Builder(3 * m + 10)
    for i in range(m):
        b.edge(i, m + i, F32(4 + ((i * 17) % m) / 64.0))
        b.edge(m + i, m + (i + 1) % m, F32(8))
    add(_case("best-is-last", *b.csr(), np.arange(m), np.concatenate([np.arange(2 * m, 3 * m + 10), np.arange(m, 2 * m)])))

    # ties: unit weights, contiguous halves, run until a side is empty
    n = 5000
    b = Builder(n)
    for i in range(n):
        b.edge(i, (i + 1) % n, F32(1))
    add(_case("ties-ring", *b.csr(), np.arange(n // 2), np.arange(n // 2, n), limit=1 << 20))
    R = 72
    b = Builder(R * R)
    for r in range(R):
        for c in range(R):
            if c + 1 < R:
                b.edge(r * R + c, r * R + c + 1, F32(1))
            if r + 1 < R:
                b.edge(r * R + c, (r + 1) * R + c, F32(1))
    add(_case("ties-grid", *b.csr(), np.arange(R * R // 2), np.arange(R * R // 2, R * R), limit=1 << 20))

    # own chunk: one chunk a list, K rows updated in node1's chunk and K in node2's
    def own(name, k0, k1):
        nz, nv = k0 // 4, k1 // 4
        ny, nx = k0 - nz, k1 - nv
        return planted(name, 1500, 1500, 700, 800, range(10, 10 + nx), range(40, 40 + nz), range(100, 100 + ny),
                       range(140, 140 + nv), seed=k0 * 100 + k1)
    add(own("own-chunk-16", 16, 16))
    add(own("own-chunk-17", 17, 17))
    add(own("own-chunk-17-16", 17, 16))
    add(own("own-chunk-16-17", 16, 17))
    # the 16th / 17th row of node1's chunk is the last of 49 rows in all (entry 48: the only row of the
    # last staging pass, coded or plain, so the last to be appended to the short list) and was the chunk's
    # best before the swap: an early rescan reads its old gain, and only the short list (16) or the forced
    # rescan (17) can tell that it is stale.  33 / 32 list-1 rows fill entries 0 .. 47 with the other 15 / 16.
    for k in (16, 17):
        add(planted(f"own-chunk-{k}-last", 1500, 1500, 700, 800, range(10, 30), range(40, 44),
                    range(100, 100 + k - 5), range(140, 152 + 17 - k), seed=7000 + k, last_y=300))

    # other chunks: five chunks a list (three of 4096), the pair in chunk 0, every updated row from
    # position 4096 up: the anchors and the far-side neighbours (their chunk's winners, which fall)
    # in [4096, 8192), the near-side ones (which rise past their chunk's winner) from 8192 up.
    # 8400 positions a list is the least that keeps both groups out of the pair's 4096-position chunk.
    for K in (64, 65, 256, 257):
        la, lb = K - K // 2, K // 2
        (nx, nz), (ny, nv) = _split(la), _split(lb)
        add(planted(f"other-{K}", 8400, 8400, 3, 5, range(4100, 4100 + nx), range(8200, 8200 + nz),
                    range(4300, 4300 + ny), range(8200, 8200 + nv), seed=K))

    # row length: every updated row exactly L entries long
    for L in (31, 32, 33, 64, 65):
        add(planted(f"rowlen-{L}", 2500, 2500, 100, 200, [10, 11, 12, 13], [20, 21], [30, 31, 32, 33], [40, 41],
                    seed=L, rowlen=L))

    # staging passes: tot rows in all
    for K in (7, 8, 9, 15, 16, 17, 24, 25, 48, 49):
        la, lb = K - K // 2, K // 2
        (nx, nz), (ny, nv) = _split(la), _split(lb)
        add(planted(f"stage-{K}", 1200, 1300, 600, 500, range(10, 10 + nx), range(40, 40 + nz),
                    range(100, 100 + ny), range(140, 140 + nv), seed=1000 + K))

    # order-matters: rows of 20-40 entries, weights over 2^-20 .. 2^4 from a palette of 3000
    rng = np.random.default_rng(21)
    pal = (np.exp2(rng.uniform(-20, 4, 3000)) * rng.uniform(1, 2, 3000)).astype(F32)
    pal = np.unique(pal)
    n = 1400
    b = Builder(n)
    adj = [set() for _ in range(n)]
    def link(u, v):
        adj[u].add(v)
        adj[v].add(u)
        b.edge(u, v, pal[int(rng.integers(len(pal)))])
    for u in range(n):
        for d in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89):
            link(u, (u + d) % n)
    for _ in range(8 * n):
        u, v = int(rng.integers(n)), int(rng.integers(n))
        if u != v and v not in adj[u] and len(adj[u]) < 40 and len(adj[v]) < 40:
            link(u, v)
    add(_case("order-matters", *b.csr(), *_lists(700, 700, 21)))

    # weight codes: the same structure with N distinct weight bit patterns
    for N in (4095, 4096, 4097):
        n = 1200
        b = Builder(n)
        e = 0
        for u in range(n):
            for d in (1, 7, 31, 101):
                b.edge(u, (u + d) % n, F32(0.5 + (e % N) / 8192.0))
                e += 1
        add(_case(f"wdict-{N}", *b.csr(), *_lists(600, 600, 4096), nweights=N))

    for nets in (256, 257):
        add(_pins_case(f"nets-edge-{nets}", nets, oracle, seed=nets))

    add(_ring_long("sel-pad-33", SEL_PAD * CHUNK, SEL_PAD * CHUNK + 1))
    add(_ring_long("fix-65", FIX_NCK * CHUNK, FIX_NCK * CHUNK + 1))
    _CASES = C
    return C


LONG = ("sel-pad-33", "fix-65")
_REFS = {}


def reference(name):
    """reference_kl of a case, computed once and shared (treat it as read-only)."""
    if name not in _REFS:
        c = cases()[name]
        _REFS[name] = reference_kl(c.rowptr, c.col, c.w, c.order0, c.order1, c.limit)
    return _REFS[name]
