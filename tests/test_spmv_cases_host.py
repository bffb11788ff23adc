"""The SpMV shape cases (spmv_cases.py) hold the shapes they are named for: the
row blocks spmv_row_blocks cuts from them (restated in spmv_cases.row_blocks at
768-entry segments, 256 rows), the lanes per row, the column bits, the value
counts and the panel buckets.  No GPU: test_gpu_spmv_shapes.py runs the kernels
on the same cases and checks the segment size on the device side."""
import numpy as np
import pytest

import spmv_cases as sc


@pytest.fixture(scope="module")
def cases():
    return sc.cases()


def _colbits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def test_segment_constants():
    assert sc.SEG == 768 and sc.ROWS == 256 and sc.REL == 258


@pytest.mark.parametrize("name", list(sc.cases()))
def test_case_is_a_valid_csr(cases, name):
    c = cases[name]
    assert np.all(c.lens >= 0) and (c.nnz == 0 or (c.col.min() >= 0 and c.col.max() < c.n))
    row = np.repeat(np.arange(c.n), c.lens)
    assert np.all(np.diff(c.col.astype(np.int64))[row[1:] == row[:-1]] >= 0)  # ascending within a row
    assert np.all(np.isfinite(c.x)) and np.all(np.isfinite(c.val * c.x[c.col]))
    blocks = sc.row_blocks(c.rowptr)
    assert sum(b[1] for b in blocks) == c.n and sum(b[2] for b in blocks) == c.nnz
    for r0, nr, nnz in blocks:
        assert 1 <= nr <= sc.ROWS and (nnz <= sc.SEG or nr == 1)
    # references agree with each other within the kernels' own bar
    y, a, yseq = sc.reference(name)
    assert np.all(np.abs(yseq - y) <= 1e-14 * a)
    assert (c.ncodes <= (1 << (32 - _colbits(c.n)))) == c.packed
    if name not in ("all-distinct", "panel-3000-gdict") and not name.startswith("dict-edge"):
        assert c.ncodes <= 64


def test_rows256(cases):
    c = cases["rows256"]
    blocks = sc.row_blocks(c.rowptr)
    assert [b[1] for b in blocks] == [256, 256, 256, 256, 1]
    assert blocks[1][2] == sc.SEG  # 256 rows and 768 entries at once
    assert blocks[2][2] == 0       # a block whose rows are all empty
    for b in (blocks[0], blocks[3]):
        ln = c.lens[b[0]:b[0] + 256]
        assert ln.min() == 1 and ln.max() == 3
    assert c.n == 1025  # two panels at pb 10, the second of one column
    assert np.count_nonzero(c.col == 1024) >= 6 and np.count_nonzero(c.col < 1024) > 1000


def test_seg_exact(cases):
    c = cases["seg-exact"]
    blocks = sc.row_blocks(c.rowptr)
    assert blocks[0] == (0, 1, sc.SEG)          # a single row of SEG entries: stream mode
    assert blocks[1] == (1, 1, sc.SEG + 1)      # SEG + 1: vector mode
    assert blocks[2] == (2, 100, sc.SEG)        # rows summing to SEG exactly
    assert blocks[3] == (102, 85, sc.SEG - 3)   # the next row (4 entries) would make SEG + 1
    assert c.lens[187] == 4 and blocks[4][0] == 187
    assert sum(b[2] > sc.SEG for b in blocks) == 1


def test_lanes(cases):
    c = cases["lanes"]
    blocks = sc.row_blocks(c.rowptr)
    short = [b for b in blocks if b[2] <= sc.SEG]
    assert tuple(b[1] for b in short[:len(sc.LANE_BLOCKS)]) == sc.LANE_BLOCKS
    assert len([b for b in blocks if b[2] > sc.SEG]) == len(sc.LANE_BLOCKS) + 1
    seen = set()
    for r0, nr, _ in short[:len(sc.LANE_BLOCKS)]:
        L = sc.lanes_per_row(nr)
        seen.add(L)
        ln = c.lens[r0:r0 + nr]
        assert ln.min() >= 1
        if L > 1:
            assert np.any(ln % L != 0) and (nr == 1 or np.any(ln < L))  # (the 1-row block: 700 = 10 * 64 + 60)
    assert seen == {64, 32, 16, 8, 4, 2, 1}


def test_long_rows(cases):
    c = cases["long-rows"]
    assert c.n == 6000
    long_lens = sorted(int(k) for k in c.lens if k > sc.SEG)
    assert long_lens == [769, 769, 1024, 1025, 5000]
    assert c.lens[11] == 0 and c.lens[702] == 0 and c.lens[701] == 1025 and c.lens[700] == 1024
    assert np.count_nonzero(c.lens == 0) > 100 and c.lens[-1] == 769


def test_empty(cases):
    assert cases["empty-1000"].nnz == 0 and cases["empty-1000"].n == 1000
    assert [b[1:] for b in sc.row_blocks(cases["empty-1000"].rowptr)] == [(256, 0)] * 3 + [(232, 0)]
    assert cases["empty-n1"].n == 1 and cases["empty-n1"].nnz == 1
    assert cases["empty-n2"].n == 2


@pytest.mark.parametrize("n,bits", [(4096, 12), (4097, 13)])
def test_colbits(cases, n, bits):
    c = cases[f"colbits-{n}"]
    assert _colbits(c.n) == bits
    assert np.count_nonzero(c.col == n - 1) >= 4 and np.count_nonzero(c.col == 0) >= 4
    assert c.lens[2] == 1 and c.col[c.rowptr[2]] == n - 1 and c.lens[3] == 1 and c.col[c.rowptr[3]] == 0


def test_dict_edge(cases):
    a, b = cases["dict-edge-4096"], cases["dict-edge-4097"]
    for c in (a, b):
        assert c.n == (1 << 19) + 1 and _colbits(c.n) == 20 and c.nnz == 4096 + 200
        assert np.count_nonzero(c.lens) <= 600 and c.col.max() == c.n - 1 and c.col.min() == 0
        assert c.lens[0] > 0 and c.lens[-1] > 0
        _, counts = np.unique(c.val, return_counts=True)
        assert counts.max() > 1  # a frequency order to sort
    assert a.ncodes == 4096 and a.packed is True
    assert b.ncodes == 4097 and b.packed is False
    assert np.array_equal(a.rowptr, b.rowptr) and np.array_equal(a.col, b.col)


def test_all_distinct(cases):
    c = cases["all-distinct"]
    assert c.n == 300 and c.ncodes == c.nnz and 15 <= c.lens.min() and c.lens.max() <= 25 and c.packed


def test_signed_zero(cases):
    c = cases["signed-zero"]
    bits = c.val.view(np.uint64)
    for v in sc.SPECIAL_VALS:
        assert np.any(bits == np.float64(v).view(np.uint64)), v
    u, counts = np.unique(bits, return_counts=True)
    assert u[np.argmax(counts)] == np.float64(0.5).view(np.uint64)  # code 0 is 0.5
    assert counts.max() > np.sort(counts)[-2]
    assert c.x[0] != 0.0 and np.abs(c.x).max() <= 1.0
    _, a, _ = sc.reference("signed-zero")
    assert np.all(a[:8] == 0.0) and np.all(c.lens[:8] > 0)
    both = {int(b) for b in bits[:c.rowptr[8]]}
    assert both == {0, 1 << 63}
    assert c.ncodes == 8


@pytest.mark.parametrize("name", ["panel-3000-ldsdict", "panel-3000-gdict", "panel-1024-ldsdict",
                                  "panel-1025-ldsdict"])
def test_panel_cases(cases, name):
    c = cases[name]
    w = 1 << sc.PB
    P = -(-c.n // w)
    assert P == {3000: 3, 1024: 1, 1025: 2}[c.n]
    assert (c.ncodes > 2048) == name.endswith("gdict")
    panel = c.col >> sc.PB
    row = np.repeat(np.arange(c.n), c.lens)
    in_panel = np.zeros((c.n, P), np.int64)
    np.add.at(in_panel, (row, panel), 1)
    assert np.all(in_panel.sum(axis=0) > 0)  # every panel is used
    if P == 1:
        assert c.col.max() == c.n - 1
        return
    live = in_panel > 0
    only_last = live[:, -1] & (live.sum(axis=1) == 1)
    assert only_last[:40].all()  # leading rows: every earlier bucket of their workgroup is empty
    for b in range(1, P):
        assert np.any(c.col == b * w - 1) and np.any(c.col == b * w)
        r = 52 + 4 * b
        assert list(c.col[c.rowptr[r]:c.rowptr[r + 1]]) == [b * w - 1, b * w]  # a row's run ends / starts on the boundary
    if P == 3:
        assert np.all(live[100:140] == [True, False, True])
        assert c.lens[200] == 1500 and in_panel[200, 1] == 1500 > 2 * sc.PCHUNK
        for r in (300, 301):
            assert c.lens[r] == c.n and np.all(in_panel[r] > sc.PCHUNK // 2)
        assert in_panel[300].tolist() == [1024, 1024, 952]
