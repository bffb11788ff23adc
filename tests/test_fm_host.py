"""ek_fm_refine_host (no GPU): against the plain-Python restatement of the rule
on every shared case, the invariants the rule promises, the planted hill the
k = 2 connectivity refinement cannot climb, the EK_EINVAL guards, the struct
layouts."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fm_cases as fc
from conftest import PKG_DIR, REPO


def run_host(ek, name):
    nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    return ek.fm_refine_host(h, side, eps, max_passes, stall)


def test_constants_are_the_kernels(ek):
    assert (fc.C, fc.T, fc.LDS_CHUNKS) == (ek.FM_CHUNK, ek.FM_THREADS, ek.FM_LDS_CHUNKS)
    text = open(os.path.join(PKG_DIR, "csrc", "ek_internal.hpp")).read()
    for name, val in (("FM_CHUNK", fc.C), ("FM_THREADS", fc.T), ("FM_LDS_CHUNKS", fc.LDS_CHUNKS)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", text).group(1)) == val


@pytest.mark.parametrize("name", fc.names())
def test_host_equals_restatement(ek, name):
    fc.same(run_host(ek, name), fc.reference(name))


@pytest.mark.parametrize("name", fc.names())
def test_invariants(ek, name):
    nodes, ptr, pins, start, eps, max_passes, stall = fc.cases()[name]
    side, plog, mlog, res = run_host(ek, name)

    def cut_of(s):
        return ek.kway_metrics_host(ptr, pins, s.astype(np.int32), 2)[0] if len(pins) else 0

    assert res["cut_before"] == cut_of(start) and res["cut"] == cut_of(side)
    # each move's cut is the one before it minus its gain; the rollback returns to the best prefix's cut, and a
    # counted pass lowers (c, d) strictly
    at, before, before_d = 0, res["cut_before"], abs_dist(start)
    for tried, best, cut, dist in plog.tolist():
        rows = mlog[at:at + tried]
        chain = np.concatenate([[before], rows["cut"]])
        assert np.array_equal(chain[:-1] - rows["gain"], chain[1:])
        assert chain[best] == cut and chain[:best + 1].min() == cut == chain.min()
        assert (cut, dist) < (before, before_d) if best else (cut, dist) == (before, before_d)
        before, before_d = cut, dist
        at += tried
    assert at == len(mlog) == res["moves_tried"]
    assert np.all(np.diff(np.concatenate([[res["cut_before"]], plog[:, 2]])) <= 0)
    lmax = fc.max_part(nodes, eps)
    assert res["max_part"] == lmax
    for s in (0, 1):
        assert int(np.count_nonzero(side == s)) <= max(lmax, int(np.count_nonzero(start == s)))
    assert (res["n0"], res["n1"]) == (int(np.count_nonzero(side == 0)), int(np.count_nonzero(side == 1)))
    assert res["moves_kept"] == int(plog[:, 1].sum()) and res["passes_run"] == len(plog)
    assert res["passes"] == int(np.count_nonzero(plog[:, 1] > 0))
    assert len(plog) >= 1 and (plog[-1, 1] == 0 or (max_passes > 0 and res["passes"] == max_passes))
    if len(plog):
        assert res["cut"] == plog[-1, 2] and abs(res["n0"] - res["n1"]) == plog[-1, 3]
    live = {v for s in fc.live_nets(ptr, pins) for v in s}
    assert set(mlog["node"].tolist()) <= live
    if stall > 0:
        assert np.all(plog[:, 0] - plog[:, 1] <= stall)
    if max_passes > 0:
        assert res["passes"] <= max_passes


def abs_dist(side):
    return abs(int(np.count_nonzero(side == 0)) - int(np.count_nonzero(side == 1)))


def test_even_ring_at_zero_imbalance_makes_no_move(ek):
    side, plog, mlog, res = run_host(ek, "ring100_eps0.0")
    assert len(mlog) == 0 and plog.tolist() == [[0, 0, 2, 0]] and res["passes"] == 0 and res["passes_run"] == 1
    assert np.array_equal(side, fc.cases()["ring100_eps0.0"][3])
    # the odd ring has one node of slack: moves happen, every gain ties, and the ids and sizes decide
    side, plog, mlog, res = run_host(ek, "ring101_eps0.0")
    assert res["moves_tried"] > 0 and res["cut"] == 2


def test_planted_hill(ek):
    nodes, ptr, pins, start, eps, _, _ = fc.cases()["hill"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    part, rres, rlog = ek.kway_refine_host(h, start.astype(np.int32), 2, eps)
    assert rres["moves"] == 0 and np.array_equal(part, start)  # no single move gains: the refinement stays
    side, plog, mlog, res = run_host(ek, "hill")
    assert res["cut_before"] == 4 and res["cut"] == 0 < res["cut_before"]
    assert mlog[:2].tolist() == [(0, -1, 5), (1, 5, 0)]  # downhill first, then the gain
    assert side.tolist() == [1] * 6 + [0] * 6


def test_einval_guards(ek):
    nodes, ptr, pins, start, _, _, _ = fc.cases()["degenerate"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    for bad in (2, 255):
        side = start.copy()
        side[11] = bad
        with pytest.raises(ek.EKError) as e:
            ek.fm_refine_host(h, side)
        assert e.value.code == ek.EK_EINVAL, bad
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.fm_refine_host(h, start, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    # more than INT32_MAX - 1 nodes (no pins: the node count alone is refused, before the sides are read)
    big = ek.Hypergraph.from_pins(2 ** 31 - 1, np.zeros(1, np.int64), np.zeros(0, np.int32))
    o, r = ek.FmOpts(), ek.FmResult()
    ek.lib.ek_fm_default_opts(ctypes.byref(o))
    assert (o.imbalance, o.max_passes, o.stall) == (0.03, 0, 1000)
    one = np.zeros(1, np.uint8)
    rc = ek.lib.ek_fm_refine_host(big._h, ctypes.byref(o), one.ctypes.data, None, 0, None, 0, ctypes.byref(r))
    assert rc == ek.EK_EINVAL
    with pytest.raises(ValueError):
        ek.fm_refine_host(h, start[:-1])


def test_logs_are_cut_at_their_caps(ek):
    nodes, ptr, pins, start, eps, max_passes, stall = fc.cases()["stall3_passes0"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    side, plog, mlog, res = ek.fm_refine_host(h, start, eps, max_passes, stall)
    assert len(plog) >= 2 and len(mlog) >= 5
    o, r = ek.FmOpts(), ek.FmResult()
    ek.lib.ek_fm_default_opts(ctypes.byref(o))
    o.imbalance, o.max_passes, o.stall = eps, max_passes, stall
    out = start.copy()
    p = np.full((2, 4), -7, np.int64)
    m = np.zeros(4, ek.FM_MOVE_DTYPE)
    m["node"] = -7
    assert ek.lib.ek_fm_refine_host(h._h, ctypes.byref(o), out.ctypes.data, p.ctypes.data, 1, m.ctypes.data, 3,
                                    ctypes.byref(r)) == 0
    assert np.array_equal(out, side) and r.moves_tried == len(mlog) and r.passes_run == len(plog)
    assert np.array_equal(p[0], plog[0]) and np.all(p[1] == -7)
    assert m[:3].tolist() == mlog[:3].tolist() and m["node"][3] == -7


def test_struct_layout_matches_python_mirror(ek, tmp_path):
    opts = [n for n, _ in ek.FmOpts._fields_]
    res = [n for n, _ in ek.FmResult._fields_]
    move = list(ek.FM_MOVE_DTYPE.names)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu %zu %zu\\n", sizeof(ek_fm_opts), sizeof(ek_fm_result), sizeof(ek_fm_move));']
    lines += [f'  printf("%zu\\n", offsetof(ek_fm_opts, {n}));' for n in opts]
    lines += [f'  printf("%zu\\n", offsetof(ek_fm_result, {n}));' for n in res]
    lines += [f'  printf("%zu\\n", offsetof(ek_fm_move, {n}));' for n in move]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(ek.FmOpts), ctypes.sizeof(ek.FmResult), ek.FM_MOVE_DTYPE.itemsize]
    want += [getattr(ek.FmOpts, n).offset for n in opts]
    want += [getattr(ek.FmResult, n).offset for n in res]
    want += [ek.FM_MOVE_DTYPE.fields[n][1] for n in move]
    assert got == want
    assert ek.ABI_VERSION == 4  # new structs only: no existing layout changed


def test_new_symbols_are_exported(ek):
    hdr = open(os.path.join(REPO, "include", "eigkl.h")).read()
    for name in ("ek_fm_default_opts", "ek_fm_refine_host", "ek_fm_refine"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(ek.lib, name)
