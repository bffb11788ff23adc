"""Small hypergraphs placed on the branch points of the device Laplacian build
(kernels_build.hip, ek_spmv_setup_pins), with two references that share no
code with graph_build.cpp; shared by test_build_cases_host.py (which proves
each case holds the shape it is named for) and test_gpu_build_shapes.py (which
runs the kernels on them).

The branch points: a row's raw entries (per incidence of a net of k >= 2 pins,
its k - 1 other pins: k_net_count's rcnt) against ROW_SHORT (a thread's
insertion sort / a workgroup's LDS sort) and LONG_CAP (LDS sort / host
fallback); the bitonic sort's padding to a power of two; repeated pins
(merge_row's hd, k_row_write's placed); the scan's tiles of SCAN_TILE rows and
its carry between chunks of SCAN_CHUNK tiles; the 2^(32 - colbits) value codes;
a coded row past SEG entries; no nets at all and a rank without rows."""
import functools
from fractions import Fraction

import numpy as np

ROW_SHORT = 256    # raw entries a thread sorts in place (k_rows)
LONG_CAP = 8192    # raw entries a workgroup sorts in LDS (k_rows_long)
SCAN_TILE = 1024   # elements per scan tile (k_scan_tiles)
SCAN_CHUNK = 256   # tiles per trip of k_scan_sums' loop
HOST_INSERTION = 48  # raw entries the host build sorts by insertion (graph_build.cpp)
SEG = 768          # entries per coded segment (SPMV_SEG_NNZ)


class Case:
    """A hypergraph (nodes, net_ptr, pins) and what the host test checks of it."""

    def __init__(self, name, n, nets, **meta):
        self.name, self.n = name, int(n)
        self.nets = [list(map(int, e)) for e in nets]
        self.net_ptr = np.concatenate([[0], np.cumsum([len(e) for e in self.nets])]).astype(np.int64)
        self.pins = np.array([v for e in self.nets for v in e], np.int32)
        self.meta = meta
        assert len(self.pins) == 0 or (self.pins.min() >= 0 and self.pins.max() < self.n)

    def hypergraph(self, ek):
        return ek.Hypergraph.from_pins(self.n, self.net_ptr, self.pins)

    def raw_counts(self):
        """rcnt of k_net_count, restated: per node the sum over its incidences of k - 1."""
        raw = np.zeros(self.n, np.int64)
        for e in self.nets:
            if len(e) >= 2:
                for v in e:
                    raw[v] += len(e) - 1
        return raw

    def x(self):
        return np.random.default_rng(len(self.pins) + self.n).standard_normal(self.n)


# ------------------------------------------------------------------ references
def _incidences(c):
    """node -> [(net, position)], ascending: the nets are walked in order."""
    inc = {}
    for e, net in enumerate(c.nets):
        if len(net) >= 2:
            for pos, v in enumerate(net):
                inc.setdefault(v, []).append((e, pos))
    return inc


def _assemble(c, rows):
    """rows: node -> [(col, fp64 value)] of the non-isolated rows; every other
    row holds the lone diagonal -(0.0).  CSR (rowptr int64, col int32, val uint64 bits)."""
    lens = np.ones(c.n, np.int64)
    for r, ent in rows.items():
        lens[r] = len(ent)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.repeat(np.arange(c.n, dtype=np.int32), lens)  # (right for the isolated rows)
    val = np.full(int(rowptr[-1]), -0.0)
    for r, ent in rows.items():
        a = int(rowptr[r])
        col[a:a + len(ent)] = [x[0] for x in ent]
        val[a:a + len(ent)] = [x[1] for x in ent]
    return rowptr, col, val.view(np.uint64)


@functools.lru_cache(maxsize=None)
def ref_ordered(name):
    """The specified order, in plain Python: per row the incidences by ascending
    net, then pin position; each net gives -(2.0 / k) per other pin; a stable
    sort by column; duplicates summed left to right; the diagonal is minus the
    left-to-right sum over the ascending columns, and replaces an (r, r) entry
    that repeated pins made."""
    c = cases()[name]
    rows = {}
    for r, inc in _incidences(c).items():
        raw = []
        for e, pos in inc:
            net = c.nets[e]
            w = -(2.0 / float(len(net)))
            raw.extend((v, w) for p, v in enumerate(net) if p != pos)
        raw.sort(key=lambda t: t[0])  # stable
        merged = []
        for v, w in raw:
            if merged and merged[-1][0] == v:
                merged[-1][1] = merged[-1][1] + w
            else:
                merged.append([v, w])
        s = 0.0
        for _, w in merged:
            s = s + w
        out, placed = [], False
        for v, w in merged:
            if v == r:
                out.append((r, -s))
                placed = True
                continue
            if not placed and v > r:
                out.append((r, -s))
                placed = True
            out.append((v, w))
        if not placed:
            out.append((r, -s))
        rows[r] = out
    return _assemble(c, rows)


@functools.lru_cache(maxsize=None)
def ref_exact(name):
    """The same matrix in exact arithmetic: node -> ({col: Fraction}, M, S) of
    the non-isolated rows, M the raw-entry count and S the sum of the row's
    2/k terms; an isolated row is {r: 0}."""
    c = cases()[name]
    rows = {}
    for r, inc in _incidences(c).items():
        ent, M, S = {}, 0, Fraction(0)
        for e, pos in inc:
            net = c.nets[e]
            w = Fraction(2, len(net))
            for p, v in enumerate(net):
                if p != pos:
                    ent[v] = ent.get(v, Fraction(0)) - w
                    M += 1
                    S += w
        ent[r] = S  # minus the sum of every raw entry, an (r, r) one included
        rows[r] = (ent, M, S)
    return rows


def contributions(c, r, col):
    """The fp64 terms summed into entry (r, col), in the specified order."""
    out = []
    for e, net in enumerate(c.nets):
        if len(net) >= 2:
            for pos, v in enumerate(net):
                if v == r:
                    out.extend(-(2.0 / float(len(net))) for p, u in enumerate(net) if p != pos and u == col)
    return out


def dense(name):
    """ref_ordered as a dense n x n array (small cases)."""
    c = cases()[name]
    rowptr, col, val = ref_ordered(name)
    A = np.zeros((c.n, c.n))
    A[np.repeat(np.arange(c.n), np.diff(rowptr)), col] = val.view(np.float64)
    return A


# ------------------------------------------------------------------ generators
class _Builder:
    def __init__(self):
        self.n, self.nets = 0, []

    def fresh(self, k=1):
        a = self.n
        self.n += k
        return list(range(a, a + k))

    def net(self, *pins):
        self.nets.append(list(pins))

    def hub(self, v, raw, sizes=(2, 3, 4), pool=None):
        """Nets of `sizes` pins around v until it holds exactly `raw` raw entries;
        its neighbours are `raw` fresh nodes (or `pool`'s, distinct within the hub
        while raw <= len(pool)) in a seeded shuffle; v's position in the net rotates."""
        pool = list(self.fresh(raw) if pool is None else pool)
        np.random.default_rng(raw).shuffle(pool)  # (the columns arrive unsorted)
        left, i, at = raw, 0, 0
        while left > 0:
            k = sizes[i % len(sizes)]
            if k - 1 > left:
                k = 2
            others = [pool[(at + j) % len(pool)] for j in range(k - 1)]
            at += k - 1
            pos = i % k
            self.net(*others[:pos], v, *others[pos:])
            left -= k - 1
            i += 1

    def case(self, name, n=None, **meta):
        return Case(name, self.n if n is None else n, self.nets, **meta)


SHORT_EDGE_RAW = (HOST_INSERTION - 1, HOST_INSERTION, HOST_INSERTION + 1, ROW_SHORT - 1, ROW_SHORT, ROW_SHORT + 1)


def case_short_edge():
    """Rows of 47, 48, 49 (the host's insertion sort / std::stable_sort), 255,
    256 (k_rows) and 257 (k_rows_long) raw entries, each between an isolated
    row, a row of 1 and a row of 2 raw entries; the neighbours come from a
    pool of 260 nodes, so n stays small enough to recover the whole matrix."""
    b = _Builder()
    hubs, ones, twos = {}, [], []
    pool = b.fresh(130)  # half of the neighbours below the hubs, half above
    for raw in SHORT_EDGE_RAW:
        b.fresh()  # isolated
        ones += b.fresh()
        hubs[raw] = b.fresh()[0]
        twos += b.fresh()
    pool += b.fresh(130)
    for raw, v in hubs.items():
        b.hub(v, raw, pool=pool)
    for i in range(0, 6, 2):
        b.net(ones[i + 1], ones[i])
    for i in range(0, 6, 3):
        b.net(twos[i], twos[i + 2], twos[i + 1])
    return b.case("short-edge", hubs=hubs, ones=ones, twos=twos)


LONG_POW2_RAW = (257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)


def case_long_pow2():
    """Rows at, one below and one above the bitonic sort's padded sizes, each
    with distinct neighbours (merged length = raw count); the 8,192-entry row
    stores 8,193 entries: a coded row in the overflow area, the SpMV's vector
    mode.  The hubs lie between their neighbours' ids."""
    b = _Builder()
    hubs = {}
    for raw in LONG_POW2_RAW:
        below = b.fresh(raw // 3)
        hubs[raw] = b.fresh()[0]
        b.hub(hubs[raw], raw, sizes=(4, 2, 3), pool=below + b.fresh(raw - raw // 3))
    return b.case("long-pow2", hubs=hubs)


DUP_SIZES = (3, 5, 7, 11)


def case_long_dups():
    """A long row in which 5 columns each receive 44 contributions of -2/3,
    -2/5, -2/7 and -2/11, interleaved in net order: their sums depend on the
    order, so a sort that is not stable changes bits."""
    b = _Builder()
    cols = b.fresh(3)
    b.fresh(4)  # isolated, below the hub
    hub = b.fresh()[0]
    cols += b.fresh(2)  # two of the five columns lie past the diagonal
    for i in range(220):
        k = DUP_SIZES[(i + i // 5 + i // 20) % 4]
        fill = b.fresh(k - 2)
        pos = i % (k - 1)
        b.net(*fill[:pos], hub, *fill[pos:], cols[i % 5]) if i % 2 else b.net(cols[i % 5], *fill[:pos], hub, *fill[pos:])
    return b.case("long-dups", hub=hub, cols=cols)


def case_long_selfpin():
    """Repeated pins on the workgroup path and on the thread path: a node listed
    twice in nets of 3 and 4 pins, a net that is {v, v} only, and a node pair
    shared by 300 two-pin nets (-300 exactly; 20 on the short row)."""
    b = _Builder()
    L, P, S, Q, v2, w2 = b.fresh(6)
    pool = b.fresh(40)
    for hub, peer, shared in ((L, P, 300), (S, Q, 20)):
        for i in range(shared):
            b.net(hub, peer) if i % 2 else b.net(peer, hub)
            if i % 10 == 0:
                a = pool[i // 10]
                b.net(hub, a, hub)              # twice in a 3-pin net
                b.net(a, hub, pool[-1], hub)    # twice in a 4-pin net
        b.net(hub, hub)                         # a net that is the node twice: raw 2, all on the diagonal
    b.net(v2, v2)                               # ... and a row that holds nothing else
    b.net(w2, w2, w2)
    b.hub(L, 100, pool=pool)
    return b.case("long-selfpin", L=L, P=P, S=S, Q=Q, v2=v2, w2=w2)


def _cap(name, raw, hub_first=False, sizes=(2, 3, 4)):
    b = _Builder()
    if not hub_first:
        b.fresh(37)
        for i in range(0, 36, 3):
            b.net(i, i + 1, i + 2)
    hub = b.fresh()[0]
    b.hub(hub, raw, sizes=sizes)
    return b.case(name, hub=hub)


def case_cap(raw):
    """One hub row of LONG_CAP (the largest LDS sort) or LONG_CAP + 1 (the host
    fallback) raw entries; every other row holds at most 3."""
    return _cap("cap-exact" if raw == LONG_CAP else "cap-over", raw)


def case_hub_8ranks():
    """cap-exact's hub at node 0, built from two-pin nets but for a hundred of
    three: its weight (1 + 8,192) exceeds 2/8 of the total, so ek_shard_map at
    8 ranks starts ranks 1 and 2 at row 1 and rank 1 owns no rows."""
    return _cap("hub-8ranks", LONG_CAP, hub_first=True, sizes=(2,) * 80 + (3,))


def case_degenerate():
    return [Case("degenerate-nonets", 5, []),
            Case("degenerate-n1", 1, [[0], [0, 0], []]),
            Case("degenerate-tiny-nets", 7, [[3], [], [0], [6], [], [3]]),
            # empty nets first and last, nodes 0 and 8 isolated, a repeated pin, a one-pin net of node 0
            Case("degenerate-ends", 9, [[], [], [1, 2, 3], [0], [4, 2], [5, 6, 7, 5], [3, 1], [], []])]


def _sprinkle(b_nets, rng, n, count):
    for _ in range(count):
        k = int(rng.integers(2, 5))
        b_nets.append([int(v) for v in rng.choice(n, k, replace=False)])


def case_scan(n):
    """n nodes at a scan tile's edge: nets on rows 0 and n - 1 and on the rows
    either side of index 1023 / 1024, and 300 small nets elsewhere."""
    rng = np.random.default_rng(n)
    edge = sorted({v for v in (0, 1, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, n - 2, n - 1) if 0 <= v < n})
    nets = [[a, b] for a, b in zip(edge[:-1], edge[1:])] + [[edge[-1], edge[0], edge[len(edge) // 2]]]
    _sprinkle(nets, rng, n, 300)
    return Case(f"scan-{n}", n, nets, edge=edge)


SCAN_CARRY_N = SCAN_CHUNK * SCAN_TILE + SCAN_TILE + 1


def case_scan_carry():
    """258 scan tiles: k_scan_sums goes round its loop twice (256 tiles, then 2
    with the carry).  A few hundred small nets on row 0, the last row and the
    rows either side of the chunk's edge (262,143 / 262,144) and of the
    following tile's (263,167 / 263,168); every other row is isolated."""
    n = SCAN_CARRY_N
    rng = np.random.default_rng(n)
    c = SCAN_CHUNK * SCAN_TILE
    edge = [0, 1, c - 2, c - 1, c, c + 1, c + SCAN_TILE - 1, c + SCAN_TILE, n - 2, n - 1]
    nets = [[a, b] for a, b in zip(edge[:-1], edge[1:])] + [[edge[-1], edge[3], edge[0]]]
    for _ in range(300):
        k = int(rng.integers(2, 5))
        near = rng.choice(edge, 1)[0] + rng.integers(-3000, 3000, k)
        nets.append([int(v) for v in np.unique(np.clip(near, 0, n - 1))])
    return Case("scan-carry", n, nets, edge=edge)


CODES_N = (1 << 20) + 1
CODE_SIZES = (2, 3, 5, 7)


def case_codes_over():
    """n = 2^20 + 1: 21 column bits, 2,048 value codes.  1,371 node pairs joined
    by a, b, c, d copies (each 0..6, c even, not all 0) of nets of 2, 3, 5 and 7
    pins with fresh filler nodes: 2,359 distinct bit patterns (every c gives
    3,829), so the coded form is given up because of the code-bit limit, far
    below the table's own limits.  Every other row is isolated."""
    b = _Builder()
    combos = [(a, bb, cc, d) for a in range(7) for bb in range(7) for cc in range(0, 7, 2) for d in range(7)]
    combos = [t for t in combos if any(t)]
    pairs = b.fresh(2 * len(combos))
    pairs[-1] = CODES_N - 1  # the last column: bit 20
    for i, t in enumerate(combos):
        u, v = pairs[2 * i], pairs[2 * i + 1]
        todo = [k for k, m in zip(CODE_SIZES, t) for _ in range(m)]
        for j, k in enumerate(todo[i % 3:] + todo[:i % 3]):  # (the sizes' order varies with the pair)
            fill = b.fresh(k - 2)
            b.net(u, *fill, v) if j % 2 else b.net(v, *fill, u)
    assert b.n < CODES_N - 1
    return b.case("codes-over", n=CODES_N, pairs=pairs)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, every case built once."""
    out = [case_short_edge(), case_long_pow2(), case_long_dups(), case_long_selfpin(), case_cap(LONG_CAP),
           case_cap(LONG_CAP + 1), *case_degenerate(), case_scan(SCAN_TILE - 1), case_scan(SCAN_TILE),
           case_scan(SCAN_TILE + 1), case_scan_carry(), case_codes_over(), case_hub_8ranks()]
    return {c.name: c for c in out}


NAMES = ("short-edge", "long-pow2", "long-dups", "long-selfpin", "cap-exact", "cap-over", "degenerate-nonets",
         "degenerate-n1", "degenerate-tiny-nets", "degenerate-ends", "scan-1023", "scan-1024", "scan-1025",
         "scan-carry", "codes-over", "hub-8ranks")
SMALL = ("short-edge", "long-selfpin", "degenerate-nonets", "degenerate-n1", "degenerate-tiny-nets",
         "degenerate-ends")  # n <= 600: the whole matrix is recovered column by column
