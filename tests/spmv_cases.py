"""Square CSR matrices placed on the SpMV's branch points, with plain references,
shared by test_spmv_cases_host.py (which proves each case holds the shapes it is
named for) and test_gpu_spmv_shapes.py (which runs the kernels on them).

The branch points (spmv_host.cpp, kernels_spmv.hip, kernels_panel.hip): row
blocks of at most SEG entries and ROWS rows, a row above SEG entries alone in a
block (vector mode), lanes per row 64..1 from the block's row count, colbits
from n, 2^(32 - colbits) value codes, panels of 2^pb columns."""
import functools
import math

import numpy as np

SEG = 768    # entries per row block / coded segment (SPMV_SEG_NNZ)
ROWS = 256   # rows per row block (SPMV_THREADS)
REL = 258    # row starts stored per coded block (SPMV_REL_STRIDE)
PB = 10      # the panel tests' EK_PANEL_PB: panels of 1,024 columns
PCHUNK = 512  # entries per chunk of the panel walk


class Case:
    """n x n CSR (col ascending within a row, repeats allowed where stated) and an x."""

    def __init__(self, name, n, rowptr, col, val, x, packed=True):
        self.name, self.n = name, int(n)
        self.rowptr = np.ascontiguousarray(rowptr, np.int32)
        self.col = np.ascontiguousarray(col, np.int32)
        self.val = np.ascontiguousarray(val, np.float64)
        self.x = np.ascontiguousarray(x, np.float64)
        self.packed = packed  # spmv_format()[0] without EK_SPMV_PLAIN
        assert len(self.rowptr) == self.n + 1 and self.rowptr[0] == 0 and self.rowptr[-1] == len(self.col)
        assert len(self.col) == len(self.val) and len(self.x) == self.n

    @property
    def nnz(self):
        return len(self.col)

    @property
    def lens(self):
        return np.diff(self.rowptr.astype(np.int64))

    @property
    def ncodes(self):
        """Distinct stored values by bit pattern (+0.0 and -0.0 differ)."""
        return len(np.unique(self.val.view(np.uint64)))


# ------------------------------------------------------------------ references
def sequential_rows(L, x):
    """y[r] = (((0 + v0 x0) + v1 x1) + ...) over the row in ascending column
    order: every product rounded, then added left to right (no FMA)."""
    rp = L.rowptr.astype(np.int64)
    ln = np.diff(rp)
    y = np.zeros(len(ln))
    for k in range(int(ln.max())):
        live = ln > k
        e = rp[:-1][live] + k
        y[live] = y[live] + L.val[e] * x[L.col[e]]
    return y


def ref_exact(c):
    """(y, absrow): per row the correctly rounded sum of the fp64 products
    (math.fsum) and sum_j |a_ij x_j|."""
    prod = c.val * c.x[c.col]
    y, a = np.zeros(c.n), np.zeros(c.n)
    rp = c.rowptr
    for r in np.flatnonzero(c.lens):
        p = prod[rp[r]:rp[r + 1]]
        y[r] = math.fsum(p)
        a[r] = math.fsum(np.abs(p))
    return y, a


def row_blocks(rowptr, block_nnz=SEG, max_rows=ROWS):
    """spmv_row_blocks restated: [(row0, nrows, nnz)] per block."""
    n = len(rowptr) - 1
    starts, rows_in, nnz_in = [0], 0, 0
    for r in range(n):
        ln = int(rowptr[r + 1]) - int(rowptr[r])
        if rows_in > 0 and (nnz_in + ln > block_nnz or rows_in == max_rows):
            starts.append(r)
            rows_in = nnz_in = 0
        rows_in += 1
        nnz_in += ln
        if ln > block_nnz:  # a long row: a block of its own
            starts.append(r + 1)
            rows_in = nnz_in = 0
    if starts[-1] != n:
        starts.append(n)
    return [(a, b - a, int(rowptr[b]) - int(rowptr[a])) for a, b in zip(starts[:-1], starts[1:])]


def lanes_per_row(nrows):
    """The stream mode's L: the largest power of two with nrows * L <= 256, at most 64."""
    return min(64, 1 << int(math.floor(math.log2(ROWS // max(nrows, 1)))))


def coded_bytes(c):
    """Bytes ek_spmv_format reports for the coded segment form at SEG-entry segments."""
    blocks = row_blocks(c.rowptr)
    over = sum(nnz for _, _, nnz in blocks if nnz > SEG)
    return len(blocks) * (SEG * 4 + REL * 2 + 16) + over * 4 + c.ncodes * 8 + 8 * c.n + 8 * c.n


def panel_groups(c, stored, pb=PB):
    """The workgroup count G of the panel form if `stored` (ek_spmv_format) is
    its size for ceil(n / 2^pb) panels, else None."""
    P = -(-c.n >> pb)
    rest = stored - 16 * c.n - 6 * c.nnz - 8 * c.ncodes - 4
    return rest // (8 * P + 4) if rest > 0 and rest % (8 * P + 4) == 0 else None


# ------------------------------------------------------------------ generators
_SMALL_VALS = np.concatenate([-2.0 / np.arange(2, 41), np.arange(1, 24) / 7.0])  # 62 values


def _cols(rng, lo, hi, k):
    """k distinct ascending columns in [lo, hi)."""
    assert 0 <= k <= hi - lo
    if 4 * k >= hi - lo:
        return np.sort(rng.choice(hi - lo, k, replace=False)) + lo
    got = np.unique(rng.integers(lo, hi, k))
    while len(got) < k:
        got = np.unique(np.concatenate([got, rng.integers(lo, hi, k - len(got))]))
    return got


def _small_vals(rng, k):
    """k values of the 62, skewed so the table has a frequency order."""
    return _SMALL_VALS[np.minimum(rng.geometric(0.15, k) - 1, len(_SMALL_VALS) - 1)]


def _assemble(name, n, rows, rng, vals=None, x=None, packed=True):
    """rows: per-row column arrays (ascending); vals: picker (rng, k) -> values."""
    lens = np.array([len(r) for r in rows], np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]) if lens.sum() else np.zeros(0, np.int64)
    val = (vals or _small_vals)(rng, len(col))
    return Case(name, n, rowptr, col, val, rng.standard_normal(n) if x is None else x, packed)


def _by_lengths(name, n, lens, seed, **kw):
    rng = np.random.default_rng(seed)
    return _assemble(name, n, [_cols(rng, 0, n, int(k)) for k in lens], rng, **kw)


def case_rows256():
    """Blocks of exactly 256 rows: lengths 1-3, all 3 (also exactly SEG entries),
    all empty, 1-3 again; a tail block of 1 row.  n = 1,025: two panels at pb 10."""
    rng = np.random.default_rng(256)
    lens = np.concatenate([rng.integers(1, 4, ROWS), np.full(ROWS, 3), np.zeros(ROWS, np.int64),
                           rng.integers(1, 4, ROWS), [2]])
    n = len(lens)
    rng = np.random.default_rng(2560)
    rows = [_cols(rng, 0, n, int(k)) for k in lens]
    for r in (0, 255, 256, 511, 800, n - 1):  # the second panel's one column (the row's last: still ascending)
        rows[r][-1] = n - 1
    return _assemble("rows256", n, rows, rng)


def case_seg_exact():
    """A row of SEG entries, a row of SEG + 1 (vector mode), 100 rows summing to
    SEG exactly, 85 rows summing to SEG - 3 followed by a row of 4."""
    rng = np.random.default_rng(768)
    a = np.array([8] * 68 + [7] * 32)
    rng.shuffle(a)
    n = 1000
    lens = np.concatenate([[SEG, SEG + 1], a, np.full(85, 9), [4]])
    lens = np.concatenate([lens, rng.integers(1, 4, n - len(lens))])
    return _by_lengths("seg-exact", n, lens, 7680)


LANE_BLOCKS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255)


def case_lanes():
    """Blocks of LANE_BLOCKS rows, each between two long rows (blocks of their
    own), so L takes 64, 32, 16, 8, 4, 2 and 1; row lengths include L - 1,
    L + 1 and other non-multiples of L."""
    rng = np.random.default_rng(64)
    n = sum(LANE_BLOCKS) + len(LANE_BLOCKS) + 1
    lens = [SEG + 1]
    for i, k in enumerate(LANE_BLOCKS):
        L = lanes_per_row(k)
        cap = min(SEG // k, 3 * L + 5)
        ln = rng.integers(1, cap + 1, k)
        ln[0] = max(1, min(L - 1, cap))
        if k > 1:
            ln[1] = min(L + 1, cap)
        if k == 1:
            ln[0] = 700  # 10 strides of 64 lanes and 60 more
        lens.extend(ln.tolist())
        lens.append(SEG + 1 + i)
    return _by_lengths("lanes", n, np.array(lens), 640)


def case_long_rows():
    rng = np.random.default_rng(5000)
    n = 6000
    lens = rng.integers(0, 4, n)
    for r, k in ((10, 769), (11, 0), (700, 1024), (701, 1025), (702, 0), (3000, 5000), (n - 1, 769)):
        lens[r] = k
    return _by_lengths("long-rows", n, lens, 50000)


def case_empty():
    z = np.zeros(0)
    x = np.random.default_rng(1).standard_normal(1000)
    return [Case("empty-1000", 1000, np.zeros(1001, np.int32), z, z, x),
            Case("empty-n1", 1, [0, 1], [0], [-0.4], [1.7]),
            Case("empty-n2", 2, [0, 2, 3], [0, 1, 0], [1.5, -0.5, -0.5], [0.3, -1.1])]


def case_colbits(n):
    """n = 4,096: 12 column bits; 4,097: 13.  Entries in columns 0 and n - 1."""
    rng = np.random.default_rng(n)
    rows = [_cols(rng, 0, n, int(k)) for k in rng.integers(0, 6, n)]
    for r in (0, 1, n // 2, n - 1):
        rows[r] = np.unique(np.concatenate([rows[r], [0, n - 1]]))
    rows[2] = np.array([n - 1])
    rows[3] = np.array([0])
    return _assemble(f"colbits-{n}", n, rows, rng)


def case_dict_edge(ndistinct):
    """n = 2^19 + 1 (20 column bits, 4,096 codes), 4,296 entries in 600 rows,
    `ndistinct` distinct values: 4,096 fit the codes, 4,097 do not."""
    rng = np.random.default_rng(4096)  # the same structure for both
    n, nnz = (1 << 19) + 1, 4096 + 200
    live = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 598)]))
    per = np.full(len(live), nnz // len(live))
    per[:nnz - per.sum()] += 1
    rows = {int(r): _cols(rng, 0, n, int(k)) for r, k in zip(live, per)}
    rows[n - 1][-1] = n - 1
    rows[0][0] = 0
    lens = np.zeros(n, np.int64)
    lens[live] = per
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.concatenate([rows[int(r)] for r in live])
    distinct = (np.arange(ndistinct) - 2000.5) / 512.0  # exact in fp64, none zero
    val = np.concatenate([distinct, distinct[rng.integers(0, 40, nnz - ndistinct)]])  # the repeats: a frequency order
    rng.shuffle(val)
    return Case(f"dict-edge-{ndistinct}", n, rowptr, col, val, rng.standard_normal(n), packed=ndistinct <= 4096)


def case_all_distinct():
    rng = np.random.default_rng(300)
    n = 300
    return _by_lengths("all-distinct", n, rng.integers(15, 26, n), 3000, vals=lambda g, k: g.standard_normal(k))


SPECIAL_VALS = np.array([0.0, -0.0, 5e-324, 1e-300, -1e-300, 1e300, -1e300])


def case_signed_zero():
    """+0.0, -0.0, a subnormal, +-1e-300 and +-1e300 among the stored values;
    0.5 is the most frequent value (code 0), so a summed padding word (word 0:
    column 0, code 0) would add 0.5 x[0]; |x| <= 1, so no product overflows.
    Rows 0-7 hold only +-0.0: their sum of |a x| is 0."""
    rng = np.random.default_rng(0)
    n = 200
    rows = [_cols(rng, 0, n, int(k)) for k in rng.integers(1, 9, n)]

    def vals(g, k):
        v = np.where(g.random(k) < 0.5, 0.5, SPECIAL_VALS[g.integers(0, len(SPECIAL_VALS), k)])
        return v

    c = _assemble("signed-zero", n, rows, rng, vals=vals, x=np.zeros(n))
    val = c.val.copy()
    val[:c.rowptr[8]] = np.where(rng.random(int(c.rowptr[8])) < 0.5, 0.0, -0.0)
    x = rng.uniform(-1.0, 1.0, n)
    x[0] = 0.75  # what a summed padding word would gather
    x[1:5] = [1.0, -1.0, 0.5, -0.5]
    return Case("signed-zero", n, c.rowptr, c.col, val, x)


def _panel_rows(n, rng, big=True):
    P = -(-n >> PB)
    w = 1 << PB
    rows = [_cols(rng, 0, n, int(k)) for k in rng.integers(0, 7, n)]
    if P >= 2:
        for r in range(0, 40):  # the last panel only: the earlier buckets of the workgroup are empty
            lo = (P - 1) * w
            rows[r] = _cols(rng, lo, n, min(int(rng.integers(1, 9)), n - lo))
        for b in range(1, P):  # columns either side of each panel boundary
            for r, cs in ((50 + 4 * b, [b * w - 1]), (51 + 4 * b, [b * w]), (52 + 4 * b, [b * w - 1, b * w]),
                          (53 + 4 * b, [0, b * w - 1, b * w, n - 1])):
                rows[r] = np.unique(cs)
    if P >= 3:
        for r in range(100, 140):  # panels 0 and 2 only
            rows[r] = np.concatenate([_cols(rng, 0, w, int(rng.integers(1, 6))),
                                      _cols(rng, 2 * w, min(3 * w, n), int(rng.integers(1, 6)))])
    if big:
        # 1,500 entries in panel 1 (1,024 columns: columns repeat, ascending): three chunks of one bucket
        rows[200] = np.sort(rng.integers(w, 2 * w, 1500))
        rows[300] = np.arange(n)  # two dense rows across every panel
        rows[301] = np.arange(n)
    return rows


def case_panel(n, many_values, big=True):
    """EK_PANEL_PB=10: ceil(n / 1024) panels.  many_values: more than 2,048
    distinct values (the table gathered from global memory), else 62 (in LDS)."""
    rng = np.random.default_rng(n + (7 if many_values else 0))
    vals = (lambda g, k: np.round(g.standard_normal(k), 6)) if many_values else None
    name = f"panel-{n}-{'gdict' if many_values else 'ldsdict'}"
    return _assemble(name, n, _panel_rows(n, rng, big), rng, vals=vals)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, every case built once."""
    out = [case_rows256(), case_seg_exact(), case_lanes(), case_long_rows(), *case_empty(), case_colbits(4096),
           case_colbits(4097), case_dict_edge(4096), case_dict_edge(4097), case_all_distinct(), case_signed_zero(),
           case_panel(3000, False), case_panel(3000, True), case_panel(1024, False, big=False),
           case_panel(1025, False, big=False)]
    return {c.name: c for c in out}


PANEL_CASES = ("panel-3000-ldsdict", "panel-3000-gdict", "panel-1024-ldsdict", "panel-1025-ldsdict", "long-rows",
               "rows256")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref_exact y, absrow, sequential_rows y) of a case, computed once."""
    c = cases()[name]
    y, a = ref_exact(c)
    return y, a, (sequential_rows(c, c.x) if c.nnz else np.zeros(c.n))
