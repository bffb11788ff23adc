"""Weights in the data model and the weighted FM refinement on the host (no
GPU): the hMETIS reader and the writer, weights through induce and
largest_component, ek_bipart_metrics_host against a plain count,
ek_fm_refine_w_host against ek_fm_refine_host under unit weights and against
the plain-Python restatement of the weighted rule, the invariants, the
EK_EINVAL guards, the struct layout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fm_cases as fc
import fmw_cases as wc
from conftest import REPO


# ---------------------------------------------------------------------------
# reader and writer
NETS = [[1, 2, 3], [2, 4], [5, 1], [4]]  # 1-based, as in the file
NET_W = [3, 1, 7, 2]
NODE_W = [4, 0, 2, 9, 1]


def hgr_text(fmt, comments=True):
    """A 4-net, 5-node file in the hMETIS form `fmt` (None: no fmt token)."""
    lines = ["% a comment before the header"] if comments else []
    lines.append("4 5" + ("" if fmt is None else f" {fmt}"))
    for e, pins in enumerate(NETS):
        if comments and e == 2:
            lines.append("% a comment between two nets")
        head = [str(NET_W[e])] if fmt in (1, 11) else []
        lines.append(" ".join(head + [str(p) for p in pins]))
    if fmt in (10, 11):
        for v, w in enumerate(NODE_W):
            if comments and v == 1:
                lines.append("%% node weights")
            lines.append(str(w))
    return "\n".join(lines) + "\n"


def state(h):
    ptr, pins = h.pins()
    node_w, net_w = h.weights()
    return (h.dims(), ptr.tolist(), pins.tolist(), None if node_w is None else node_w.tolist(),
            None if net_w is None else net_w.tolist())


@pytest.mark.parametrize("fmt", [None, 0, 1, 10, 11])
def test_read_weighted_and_write_round_trip(ek, tmp_path, fmt):
    src = tmp_path / "in.hgr"
    src.write_text(hgr_text(fmt))
    h = ek.Hypergraph.read_weighted(src)
    want = ((4, 5, 8), [0, 3, 5, 7, 8], [0, 1, 2, 1, 3, 4, 0, 3], NODE_W if fmt in (10, 11) else None,
            NET_W if fmt in (1, 11) else None)
    assert state(h) == want
    out = tmp_path / "out.hgr"
    h.write(out)
    assert out.read_text() == hgr_text(fmt if fmt else None, comments=False)
    assert state(ek.Hypergraph.read_weighted(out)) == want
    if not fmt:  # an unweighted file without comments: the reference reader gives the same
        assert state(ek.Hypergraph.read(out)) == want


def test_copy_weights_writes_ones_for_an_absent_array(ek):
    h = ek.Hypergraph.from_pins(3, [0, 2, 3], [0, 1, 2])
    node_w, net_w = np.zeros(3, np.int32), np.zeros(2, np.int32)
    assert ek.lib.ek_hgr_copy_weights(h._h, node_w.ctypes.data, net_w.ctypes.data) == 0
    assert node_w.tolist() == [1, 1, 1] and net_w.tolist() == [1, 1] and h.weights() == (None, None)
    h.set_weights([0, 5, 2], None)
    assert h.weights()[0].tolist() == [0, 5, 2] and h.weights()[1] is None
    h.set_weights(None, [4, 1])
    assert h.weights()[0] is None and h.weights()[1].tolist() == [4, 1]
    for node_w, net_w in (([0, -1, 2], None), (None, [1, 0]), (None, [-3, 1])):
        with pytest.raises(ek.EKError) as e:
            h.set_weights(node_w, net_w)
        assert e.value.code == ek.EK_EINVAL
    assert h.weights()[0] is None and h.weights()[1].tolist() == [4, 1]  # a refused call changes nothing
    with pytest.raises(ValueError):
        h.set_weights([1, 2], None)


@pytest.mark.parametrize("text", [
    "4 5 2\n1 2\n", "4 5 100\n1 2\n", "2 3 1\n2 1 2\n\n", "2 3 1\n2 1 2\n", "2 3 1\n0 1 2\n3 1 2\n",
    "2 3 1\n-1 1 2\n3 1 2\n", "1 3 10\n1 2\n4\n-2\n1\n", "1 3 10\n1 2\n4\n2\n", "1 3 11\n5 1 2\n4\n\n2\n1\n",
    "1 3 10\n1 2\n4 4\n2\n1\n", "1 3\n1 4\n", "1 3\n1 x\n", "1\n", "1 3 1 1\n1 1 2\n", "1 3 1\n3000000000 1 2\n"],
    ids=["fmt2", "fmt100", "blank_net_line_fmt1", "missing_net_line_fmt1", "net_weight_0", "net_weight_negative",
         "node_weight_negative", "too_few_node_lines", "blank_node_line", "two_node_weights", "pin_out_of_range",
         "not_a_number", "short_header", "long_header", "net_weight_above_int32"])
def test_read_weighted_rejects(ek, tmp_path, text):
    src = tmp_path / "bad.hgr"
    src.write_text(text)
    with pytest.raises(ek.EKError) as e:
        ek.Hypergraph.read_weighted(src)
    assert e.value.code == ek.EK_EINVAL


def test_unweighted_write_is_byte_identical(ek, tmp_path):
    for name in ("degenerate", "n255", "hill"):
        nodes, ptr, pins, *_ = fc.cases()[name]
        h = ek.Hypergraph.from_pins(nodes, ptr, pins)
        text = f"{len(ptr) - 1} {nodes}\n" + "".join(
            " ".join(str(int(p) + 1) for p in pins[ptr[e]:ptr[e + 1]]) + "\n" for e in range(len(ptr) - 1))
        h.write(tmp_path / "plain.hgr")
        assert (tmp_path / "plain.hgr").read_bytes() == text.encode()
        # ... and again once weights were set and cleared
        h.set_weights(np.ones(nodes, np.int32), np.ones(len(ptr) - 1, np.int32))
        h.set_weights(None, None)
        h.write(tmp_path / "plain2.hgr")
        assert (tmp_path / "plain2.hgr").read_bytes() == text.encode()
        # both readers agree on it
        assert state(ek.Hypergraph.read(tmp_path / "plain.hgr")) == state(ek.Hypergraph.read_weighted(tmp_path / "plain.hgr"))


def test_induce_and_largest_component_carry_weights(ek):
    # two components, {0, 1, 2, 3} and {4, 5}; net 2 has one pin, net 4 is empty
    nets = [[0, 1, 2], [2, 3], [3], [4, 5], [], [1, 3]]
    ptr, pins = fc.pack(nets)
    h = ek.Hypergraph.from_pins(6, ptr, pins)
    node_w, net_w = [5, 0, 7, 1, 9, 2], [2, 3, 4, 5, 6, 8]
    h.set_weights(node_w, net_w)
    c, m = h.largest_component()
    assert m.tolist() == [0, 1, 2, 3, -1, -1]
    assert c.weights()[0].tolist() == [5, 0, 7, 1] and c.weights()[1].tolist() == [2, 3, 4, 8]
    assert c.pins()[0].tolist() == [0, 3, 5, 6, 8]
    sub, m = h.induce([0, 1, 1, 1, 1, 1])
    assert m.tolist() == [-1, 0, 1, 2, 3, 4]
    # net 0 keeps {1, 2}, net 1 {2, 3}, net 3 {4, 5}, net 5 {1, 3}; nets 2 and 4 fall out
    assert sub.weights()[0].tolist() == [0, 7, 1, 9, 2] and sub.weights()[1].tolist() == [2, 3, 5, 8]
    # one array only; none
    h.set_weights(None, net_w)
    assert h.induce([1] * 6)[0].weights()[0] is None and h.induce([1] * 6)[0].weights()[1].tolist() == [2, 3, 5, 8]
    h.set_weights(node_w, None)
    assert h.largest_component()[0].weights()[1] is None
    h.set_weights(None, None)
    assert h.induce([1] * 6)[0].weights() == (None, None) and h.largest_component()[0].weights() == (None, None)


# ---------------------------------------------------------------------------
# metrics
@pytest.mark.parametrize("name", wc.names())
def test_bipart_metrics_against_a_plain_count(ek, name):
    nodes, ptr, pins, node_w, net_w, side, *_ = wc.cases()[name]
    h, _ = wc.hypergraph(ek, name)
    for s in (side, 1 - side, (np.arange(nodes) % 2).astype(np.uint8)):
        assert ek.bipart_metrics_host(h, s) == wc.metrics(nodes, ptr, pins, node_w, net_w, s)
    h.set_weights(None, None)  # unit weights: the weighted cut is the cut nets, and k = 2's
    got = ek.bipart_metrics_host(h, side)
    cut_nets = ek.kway_metrics_host(ptr, pins, side.astype(np.int32), 2)[0] if len(pins) else 0
    assert got[0] == got[1] == cut_nets
    assert (got[2], got[3]) == (int(np.count_nonzero(side == 0)), int(np.count_nonzero(side == 1)))


def test_bipart_metrics_rejects_a_bad_side(ek):
    h, (side, *_) = wc.hypergraph(ek, "degenerate")
    bad = side.copy()
    bad[4] = 2
    with pytest.raises(ek.EKError) as e:
        ek.bipart_metrics_host(h, bad)
    assert e.value.code == ek.EK_EINVAL
    with pytest.raises(ValueError):
        ek.bipart_metrics_host(h, side[:-1])


# ---------------------------------------------------------------------------
# unit weights: the weighted entry is the unweighted rule
SHARED_INTS = ("n", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut", "n0", "n1")
_unweighted = {}


def unweighted_host(ek, name):
    """ek_fm_refine_host on an fm_cases case, computed once and shared."""
    if name not in _unweighted:
        nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
        _unweighted[name] = ek.fm_refine_host(ek.Hypergraph.from_pins(nodes, ptr, pins), side, eps, max_passes, stall)
    return _unweighted[name]


@pytest.mark.parametrize("form", ["none", "ones", "node_w_only", "net_w_only"])
@pytest.mark.parametrize("name", fc.names())
def test_unit_weights_reduce_to_the_unweighted_rule(ek, name, form):
    nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    ones = (np.ones(nodes, np.int32), np.ones(len(ptr) - 1, np.int32))
    h.set_weights(ones[0] if form in ("ones", "node_w_only") else None, ones[1] if form in ("ones", "net_w_only") else None)
    want = unweighted_host(ek, name)
    got = ek.fm_refine_w_host(h, side, eps, max_passes, stall)
    wc.same(got, want, SHARED_INTS)
    res = got[3]
    assert (res["total_weight"], res["w0"], res["w1"]) == (nodes, res["n0"], res["n1"])
    assert (res["cut_nets_before"], res["cut_nets"]) == (res["cut_before"], res["cut"])


# ---------------------------------------------------------------------------
# the weighted rule
def run_host(ek, name):
    h, (side, eps, max_passes, stall) = wc.hypergraph(ek, name)
    return ek.fm_refine_w_host(h, side, eps, max_passes, stall)


@pytest.mark.parametrize("name", wc.names())
def test_host_equals_restatement(ek, name):
    wc.same(run_host(ek, name), wc.reference(name))


@pytest.mark.parametrize("name", wc.names())
def test_invariants(ek, name):
    nodes, ptr, pins, node_w, net_w, start, eps, max_passes, stall = wc.cases()[name]
    h, _ = wc.hypergraph(ek, name)
    side, plog, mlog, res = run_host(ek, name)
    w = np.ones(nodes, np.int64) if node_w is None else node_w.astype(np.int64)
    before, after = ek.bipart_metrics_host(h, start), ek.bipart_metrics_host(h, side)
    assert (res["cut_before"], res["cut_nets_before"]) == before[:2]
    assert (res["cut"], res["cut_nets"], res["w0"], res["w1"]) == after
    assert res["total_weight"] == int(w.sum()) == res["w0"] + res["w1"]
    # each move's cut is the one before it minus its gain; the rollback returns to the best prefix's cut, and a
    # counted pass lowers (c, d) strictly
    at, c, d = 0, before[0], abs(before[2] - before[3])
    for tried, best, cut, dist in plog.tolist():
        rows = mlog[at:at + tried]
        chain = np.concatenate([[c], rows["cut"]])
        assert np.array_equal(chain[:-1] - rows["gain"], chain[1:])
        assert chain[best] == cut and chain[:best + 1].min() == cut == chain.min()
        assert (cut, dist) < (c, d) if best else (cut, dist) == (c, d)
        assert len(set(rows["node"].tolist())) == tried  # a node moves at most once a pass
        c, d = cut, dist
        at += tried
    assert at == len(mlog) == res["moves_tried"]
    assert np.all(np.diff(np.concatenate([[res["cut_before"]], plog[:, 2]])) <= 0)
    lmax = wc.max_part(int(w.sum()), eps)
    assert res["max_part"] == lmax
    # no side that received a node ends above L_max
    for s in (0, 1):
        received = np.any((side == s) & (start != s))
        assert not received or after[2 + s] <= lmax
        assert after[2 + s] <= max(lmax, before[2 + s])
    assert (res["n0"], res["n1"]) == (int(np.count_nonzero(side == 0)), int(np.count_nonzero(side == 1)))
    assert res["moves_kept"] == int(plog[:, 1].sum()) and res["passes_run"] == len(plog)
    assert res["passes"] == int(np.count_nonzero(plog[:, 1] > 0))
    assert len(plog) >= 1 and (plog[-1, 1] == 0 or (max_passes > 0 and res["passes"] == max_passes))
    assert res["cut"] == plog[-1, 2] and abs(res["w0"] - res["w1"]) == plog[-1, 3]
    live = {v for s, _ in wc.live_nets(ptr, pins, net_w) for v in s}
    assert set(mlog["node"].tolist()) <= live  # no deg-0 node is in the log
    if stall > 0:
        assert np.all(plog[:, 0] - plog[:, 1] <= stall)
    if max_passes > 0:
        assert res["passes"] <= max_passes


def test_heavy_node_never_moves_and_its_side_never_receives(ek):
    nodes, ptr, pins, node_w, net_w, start, eps, _, _ = wc.cases()["heavy"]
    side, plog, mlog, res = run_host(ek, "heavy")
    assert 2 * int(node_w[7]) > res["total_weight"] and int(node_w[7]) > res["max_part"]
    assert any(7 in s for s, _ in wc.live_nets(ptr, pins, net_w))  # (it is on nets: only its weight holds it)
    assert 7 not in mlog["node"].tolist() and res["moves_tried"] > 0
    assert all(start[v] == 0 for v in mlog["node"].tolist())  # side 0, above L_max with node 7 on it, receives nothing


def test_top_node_that_does_not_fit_leaves_its_side_without_a_candidate(ek):
    side, plog, mlog, res = run_host(ek, "top_does_not_fit")
    # node 1 has g = 1 > 0 and fits (10 + 1 <= 11), but side 0's top is node 0 (g = 4, w = 5), which does not
    assert (res["total_weight"], res["max_part"], res["w0"], res["w1"]) == (20, 11, 10, 10)
    assert res["moves_tried"] == 0 and plog.tolist() == [[0, 0, 6, 0]] and res["cut_before"] == res["cut"] == 6


def test_equal_gains_go_to_the_heavier_side_then_the_smaller_id(ek):
    side, plog, mlog, res = run_host(ek, "tie_heavier_side")
    assert mlog[0].tolist() == (1, 2, 0)  # node 1 leaves side 0 (S = 4 | 1) although node 0 ties on g
    side, plog, mlog, res = run_host(ek, "tie_smaller_id")
    assert mlog[0].tolist() == (0, 2, 0)  # S = 4 | 4: the smaller id


def test_weighted_hills(ek):
    side, plog, mlog, res = run_host(ek, "hill_bridges5")
    assert res["cut_before"] == 20 and res["cut"] == 0 and mlog[0].tolist() == (0, 7, 13)
    side, plog, mlog, res = run_host(ek, "hill_joins5")
    assert res["cut_before"] == 4 and res["cut"] == 0 and mlog[:2].tolist() == [(0, -13, 17), (1, 17, 0)]


def test_einval_guards(ek):
    h, (start, *_) = wc.hypergraph(ek, "degenerate")
    for bad in (2, 255):
        side = start.copy()
        side[11] = bad
        with pytest.raises(ek.EKError) as e:
            ek.fm_refine_w_host(h, side)
        assert e.value.code == ek.EK_EINVAL, bad
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.fm_refine_w_host(h, start, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    with pytest.raises(ValueError):
        ek.fm_refine_w_host(h, start[:-1])
    # the nets on one node sum to 2^31: one more than a gain holds (2^31 - 1 is the case gain_bound)
    ptr, pins = fc.pack([[0, 1], [0, 2]])
    h = ek.Hypergraph.from_pins(3, ptr, pins)
    h.set_weights(None, [2 ** 30, 2 ** 30])
    with pytest.raises(ek.EKError) as e:
        ek.fm_refine_w_host(h, [0, 1, 1])
    assert e.value.code == ek.EK_EINVAL
    h.set_weights(None, [2 ** 30, 2 ** 30 - 1])
    assert ek.fm_refine_w_host(h, [0, 1, 1], 1.0)[3]["cut_before"] == 2 ** 31 - 1
    # a repeated pin counts once towards that sum, and a net that takes no part not at all
    ptr, pins = fc.pack([[0, 1, 0], [0, 0], [0]])
    h = ek.Hypergraph.from_pins(2, ptr, pins)
    h.set_weights(None, [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1])
    assert ek.fm_refine_w_host(h, [0, 1], 1.0)[3]["cut_before"] == 2 ** 31 - 1
    # more than INT32_MAX - 1 nodes
    big = ek.Hypergraph.from_pins(2 ** 31 - 1, np.zeros(1, np.int64), np.zeros(0, np.int32))
    o, r = ek.FmOpts(), ek.FmWResult()
    ek.lib.ek_fm_default_opts(ctypes.byref(o))
    one = np.zeros(1, np.uint8)
    assert ek.lib.ek_fm_refine_w_host(big._h, ctypes.byref(o), one.ctypes.data, None, 0, None, 0,
                                      ctypes.byref(r)) == ek.EK_EINVAL


def test_struct_layout_and_abi(ek, tmp_path):
    res = [n for n, _ in ek.FmWResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu %d\\n", sizeof(ek_fm_w_result), EIGKL_ABI_VERSION);']
    lines += [f'  printf("%zu\\n", offsetof(ek_fm_w_result, {n}));' for n in res]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(ek.FmWResult), 4] + [getattr(ek.FmWResult, n).offset for n in res]
    assert ek.ABI_VERSION == 4 == ek.lib.ek_abi_version()  # a new struct only: no existing layout changed


def test_new_symbols_are_exported(ek):
    hdr = open(os.path.join(REPO, "include", "eigkl.h")).read()
    for name in ("ek_hgr_set_weights", "ek_hgr_weights", "ek_hgr_copy_weights", "ek_hgr_read_weighted",
                 "ek_bipart_metrics_host", "ek_fm_refine_w_host", "ek_fm_refine_w"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(ek.lib, name)
