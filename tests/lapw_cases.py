"""Inputs and references of the net-weighted clique Laplacian,
shared by test_lapw_host.py and test_gpu_lapw.py: the hypergraphs of
build_cases.py under four net weightings, two paths whose weights outgrow the
device build's value dictionary, and build_cases' two references restated with
the weighted term

    w(e) = -(float(2 * c(e)) / float(k))        k = |e| >= 2, repeated pins counted

in plain Python floats (fp64, so bit-exact) and in Fractions.  Nothing here
shares code with graph_build.cpp or kernels_build.hip."""
import functools
from fractions import Fraction

import numpy as np

import build_cases as bc

TSIZE = 1 << 16  # the device dictionary's table slots (ctx_spmv.cpp)
WIDE = (1, 2 ** 31 - 1, 3, 65537, 2 ** 30, 12345, 2, 99991)
WEIGHTINGS = ("mod3", "pow2", "wide", "distinct")


def weights(kind, nets):
    """int32 net weights of a weighting; "own": the case's own (dict cases), None elsewhere."""
    e = np.arange(nets, dtype=np.int64)
    if kind == "mod3":      # DESIGN.md §12's synthetic net weights
        w = 1 + e % 3
    elif kind == "pow2":    # an exact scaling by 2^5
        w = np.full(nets, 32)
    elif kind == "wide":    # 2 c(e) up to 2^32 - 2: the int64 product, the widest fp64 terms
        w = np.array(WIDE, np.int64)[e % len(WIDE)]
    elif kind == "distinct":
        w = 1 + e
    elif kind == "ones":
        w = np.ones(nets, np.int64)
    else:
        raise KeyError(kind)
    return w.astype(np.int32)


def _zigzag(m):
    """1, m, 2, m - 1, 3, ...: m distinct weights whose neighbouring sums take two values."""
    w = np.empty(m, np.int64)
    w[0::2] = np.arange(1, (m + 1) // 2 + 1)
    w[1::2] = np.arange(m, (m + 1) // 2, -1)
    return w.astype(np.int32)


def case_dict(name, m):
    """A path of m two-pin nets {e, e + 1} with m distinct weights in zigzag
    order.  Off the diagonal the values are the m numbers -c(e); on it
    c(e - 1) + c(e) is m + 1 or m + 2 (plus the two ends), so the matrix holds
    m + 4 distinct values: the weights alone decide which dictionary limit is
    crossed.  The nets alternate their pin order."""
    nets = [[e, e + 1] if e % 2 else [e + 1, e] for e in range(m)]
    return bc.Case(name, m + 1, nets, own=_zigzag(m))


DICT_HALF, DICT_FULL = 40000, 70000
DICT_NAMES = ("dict-half", "dict-full")


@functools.lru_cache(maxsize=None)
def cases():
    out = dict(bc.cases())
    out["dict-half"] = case_dict("dict-half", DICT_HALF)
    out["dict-full"] = case_dict("dict-full", DICT_FULL)
    return out


def case_weights(name, kind):
    c = cases()[name]
    if kind == "own":
        return c.meta["own"]
    if kind is None:
        return None
    return weights(kind, len(c.nets))


def hypergraph(ek, name, kind):
    """The case as a Hypergraph carrying the weighting's net weights (kind None: no weights)."""
    h = cases()[name].hypergraph(ek)
    w = case_weights(name, kind)
    if w is not None:
        h.set_weights(None, w)
    return h


def term(cw, k):
    """The fp64 value one net gives each ordered pin pair: one rounded division."""
    return -(float(2 * int(cw)) / float(k))


# ------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def ref_ordered(name, kind):
    """build_cases.ref_ordered with the weighted term: CSR (rowptr int64, col int32, val uint64 bits)."""
    c = cases()[name]
    w = case_weights(name, kind)
    if name in DICT_NAMES:
        return _ref_path(c, w)
    rows = {}
    for r, inc in bc._incidences(c).items():
        raw = []
        for e, pos in inc:
            net = c.nets[e]
            t = term(1 if w is None else w[e], len(net))
            raw.extend((v, t) for p, v in enumerate(net) if p != pos)
        raw.sort(key=lambda x: x[0])  # stable
        merged = []
        for v, t in raw:
            if merged and merged[-1][0] == v:
                merged[-1][1] = merged[-1][1] + t
            else:
                merged.append([v, t])
        s = 0.0
        for _, t in merged:
            s = s + t
        out, placed = [], False
        for v, t in merged:
            if v == r:
                out.append((r, -s))
                placed = True
                continue
            if not placed and v > r:
                out.append((r, -s))
                placed = True
            out.append((v, t))
        if not placed:
            out.append((r, -s))
        rows[r] = out
    return bc._assemble(c, rows)


def _ref_path(c, w):
    """The same rule on a path of two-pin nets, written out: row r holds
    (r - 1, t(r - 1)), the diagonal -(t(r - 1) + t(r)) summed left to right, and
    (r + 1, t(r)); numpy's elementwise fp64 operations are the Python ones."""
    m = len(c.nets)
    t = -((2 * (np.ones(m, np.int64) if w is None else w.astype(np.int64))).astype(np.float64) / 2.0)
    n = c.n
    lens = np.full(n, 3, np.int64)
    lens[0] = lens[-1] = 2
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.empty(int(rowptr[-1]), np.int32)
    val = np.empty(int(rowptr[-1]))
    r = np.arange(1, n - 1)
    a = rowptr[r]
    col[a], col[a + 1], col[a + 2] = r - 1, r, r + 1
    val[a], val[a + 2] = t[r - 1], t[r]
    val[a + 1] = -(t[r - 1] + t[r])
    col[0:2], val[0:2] = (0, 1), (-(0.0 + t[0]), t[0])
    col[-2:], val[-2:] = (n - 2, n - 1), (t[-1], -(0.0 + t[-1]))
    return rowptr, col, val.view(np.uint64)


@functools.lru_cache(maxsize=None)
def ref_exact(name, kind):
    """node -> ({col: (exact Fraction, terms, sum of |terms|)}, self): per entry
    its exact value, the count t of fp64 terms summed into it and the exact sum
    of their magnitudes; the diagonal's t and sum are the whole row's (every raw
    entry goes through the row sum, at most t roundings each).  self: the sum
    of the (r, r) terms that repeated pins made — the diagonal replaces them,
    so the stored row sums to `self`, zero without repeated pins."""
    c = cases()[name]
    w = case_weights(name, kind)
    rows = {}
    for r, inc in bc._incidences(c).items():
        ent, M, S = {}, 0, Fraction(0)
        for e, pos in inc:
            net = c.nets[e]
            x = Fraction(2 * int(1 if w is None else w[e]), len(net))
            for p, v in enumerate(net):
                if p != pos:
                    a = ent.get(v, (Fraction(0), 0, Fraction(0)))
                    ent[v] = (a[0] - x, a[1] + 1, a[2] + x)
                    M += 1
                    S += x
        self_sum = ent.get(r, (Fraction(0), 0, Fraction(0)))[2]
        ent[r] = (S, M, S)
        rows[r] = (ent, self_sum)
    return rows


def contributions(name, kind, r, col):
    """The fp64 terms summed into entry (r, col), in the specified order."""
    c = cases()[name]
    w = case_weights(name, kind)
    out = []
    for e, net in enumerate(c.nets):
        if len(net) >= 2:
            for pos, v in enumerate(net):
                if v == r:
                    out.extend(term(1 if w is None else w[e], len(net)) for p, u in enumerate(net) if p != pos and u == col)
    return out


def dense(name, kind):
    c = cases()[name]
    rowptr, col, val = ref_ordered(name, kind)
    A = np.zeros((c.n, c.n))
    A[np.repeat(np.arange(c.n), np.diff(rowptr)), col] = val.view(np.float64)
    return A


# ------------------------------------------------------------------ the ring of clusters (test_gpu_lapw.py)
def ring_of_clusters(heavy, weight=8):
    """Four clusters of 8 nodes in a ring.  In each cluster, for i < 8, a 3-pin
    net {i, i + 1, i + 3} and a 2-pin net {i, i + 2} (mod 8), c = 1; between the
    adjacent clusters c and c + 1 two 2-pin nets {8 c + j, 8 (c + 1) + 7 - j},
    j = 0, 1, of weight `weight` when (c, c + 1 mod 4) is in `heavy`, else 1.
    Returns (nodes, nets, net weights)."""
    nets, w = [], []
    for c in range(4):
        for i in range(8):
            nets.append([8 * c + i, 8 * c + (i + 1) % 8, 8 * c + (i + 3) % 8])
            nets.append([8 * c + i, 8 * c + (i + 2) % 8])
            w += [1, 1]
    for c in range(4):
        d = (c + 1) % 4
        for j in (0, 1):
            nets.append([8 * c + j, 8 * d + 7 - j])
            w.append(weight if (c, d) in heavy else 1)
    return 32, nets, np.array(w, np.int32)


def dense_of(n, nets, w):
    """The weighted Laplacian of a small hypergraph as a dense array, from the rule (float64 sums in net order)."""
    A = np.zeros((n, n))
    for e, net in enumerate(nets):
        t = term(w[e], len(net))
        for p, u in enumerate(net):
            for q, v in enumerate(net):
                if p != q:
                    A[u, v] += t
    A[np.arange(n), np.arange(n)] = 0.0
    A[np.arange(n), np.arange(n)] = -A.sum(axis=1)
    return A
