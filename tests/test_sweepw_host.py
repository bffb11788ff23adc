"""The weighted sweep cut on the host (ek_sweep_cut_w_host, the device path's
checker) against the rule restated in Python (sweepw_cases.sweepw_ref),
against the unweighted entry under all-ones weights, against the rank split
and ek_bipart_metrics_host, and on cases whose answer is known."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
import sweepw_cases as wc
from conftest import REPO, circuit_path


def check_result(res, profw, prefix):
    n, W, lmax = res["n"], res["total_weight"], res["max_part"]
    assert len(profw) == len(prefix) == n + 1
    assert profw[0] == 0 and profw[n] == 0 and prefix[0] == 0 and prefix[n] == W
    assert np.all(np.diff(prefix) >= 0) and np.all(profw >= 0)
    assert 1 <= res["n1"] <= n - 1 and res["n0"] + res["n1"] == n
    assert (res["w1"], res["w0"]) == (prefix[res["n1"]], W - prefix[res["n1"]])
    assert res["cut"] == profw[res["n1"]] and res["cut_half"] == profw[n // 2]
    assert res["cut_nets"] <= res["spanning_nets"] and res["cut_nets"] <= res["cut"]
    feasible = np.flatnonzero((prefix[1:n] <= lmax) & (W - prefix[1:n] <= lmax)) + 1
    if res["feasible"]:
        assert res["w0"] <= lmax and res["w1"] <= lmax
        # the window is one contiguous range, and no feasible split lies outside it
        assert feasible.tolist() == list(range(res["s_lo"], res["s_hi"] + 1))
        assert res["s_lo"] <= res["n1"] <= res["s_hi"]
    else:
        assert feasible.size == 0 and (res["s_lo"], res["s_hi"]) == (0, 0)


@pytest.mark.parametrize("name", wc.names())
def test_host_equals_the_rule(ek, name):
    h, v, epsilons = wc.hypergraph(ek, name)
    for eps in epsilons:
        res, order, profw, prefix = ek.sweep_cut_w_host(h, v, eps)
        want, worder, wprofw, wprefix, _ = wc.reference(name, eps)
        assert np.array_equal(order, worder), eps
        assert np.array_equal(profw, wprofw), eps
        assert np.array_equal(prefix, wprefix), eps
        assert wc.ints(res) == want, eps
        check_result(res, profw, prefix)


def test_known_answers(ek):
    # no feasible split: node 2 (weight 100 of W = 106) is on one side of every split.  |2 P - W| is 104, 100, 100,
    # 102 at s = 1..4; of s = 2 and 3, profile_w is 1 + 3 = 4 and 2 + 3 = 5
    h, v, _ = wc.hypergraph(ek, "heavy_node")
    res, _, profw, prefix = ek.sweep_cut_w_host(h, v, 0.03)
    assert prefix.tolist() == [0, 1, 3, 103, 104, 106] and profw.tolist() == [0, 7, 4, 5, 10, 0]
    assert (res["feasible"], res["s_lo"], res["s_hi"], res["n1"], res["w0"], res["w1"], res["cut"]) == (0, 0, 0, 2, 103, 3, 4)
    assert res["max_part"] == 54
    # a window of exactly one split
    h, v, _ = wc.hypergraph(ek, "window_of_one")
    for eps, window in ((0.0, (2, 2)), (0.03, (2, 2)), (0.25, (1, 2))):
        res, _, _, prefix = ek.sweep_cut_w_host(h, v, eps)
        assert prefix.tolist() == [0, 3, 4, 6, 8]
        assert (res["feasible"], res["s_lo"], res["s_hi"]) == (1, *window)
    # a window that is one run of zero-weight nodes: every split of it perfectly balanced
    h, v, _ = wc.hypergraph(ek, "zero_run")
    res, order, profw, prefix = ek.sweep_cut_w_host(h, v, 0.0)
    n, k = 64, 6
    assert (res["s_lo"], res["s_hi"]) == (n // 2 - k, n // 2 + k) and res["w0"] == res["w1"]
    assert len(set(prefix[n // 2 - k:n // 2 + k + 1].tolist())) == 1
    window = profw[n // 2 - k:n // 2 + k + 1]
    assert res["n1"] == n // 2 - k + int(np.argmin(window))  # (argmin: the first of equal minima, the least s)
    # sums beyond 2^32 in both arrays
    h, v, _ = wc.hypergraph(ek, "cross_2_32")
    res, _, profw, prefix = ek.sweep_cut_w_host(h, v, 0.03)
    assert int(profw.max()) == 3 * wc.INT32_MAX + 3 > 2 ** 32 and int(prefix[-1]) == 3 * wc.INT32_MAX + 13 > 2 ** 32


def all_ones_equals_unweighted(ek, nodes, ptr, pins, v, eps):
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    want, worder, wprofile = ek.sweep_cut_host(h, v, eps)
    for explicit in (False, True):
        if explicit:
            h.set_weights(np.ones(nodes, np.int32), np.ones(len(ptr) - 1, np.int32))
        res, order, profw, prefix = ek.sweep_cut_w_host(h, v, eps)
        assert np.array_equal(order, worder) and np.array_equal(profw, wprofile)
        assert prefix.tolist() == list(range(nodes + 1))
        assert res["feasible"] == 1 and res["total_weight"] == nodes
        for a, b in (("n", "n"), ("n0", "n0"), ("n1", "n1"), ("s_lo", "s_lo"), ("s_hi", "s_hi"), ("max_part", "max_part"),
                     ("cut", "cut"), ("cut_nets", "cut"), ("cut_half", "cut_mid"), ("spanning_nets", "spanning_nets"),
                     ("w0", "n0"), ("w1", "n1")):
            assert res[a] == want[b], (a, explicit)


@pytest.mark.parametrize("name", sorted(sc.small_hypergraphs()))
def test_all_ones_is_the_unweighted_rule_small(ek, name):
    nodes, ptr, pins = sc.small_hypergraphs()[name]
    for fam, v in sc.value_families(nodes).items():
        for eps in sc.EPSILONS if fam == "normal" else (0.03,):
            all_ones_equals_unweighted(ek, nodes, ptr, pins, v, eps)


def test_all_ones_is_the_unweighted_rule_other_cases(ek):
    for n in (2, 3, 10, 11, 64, 65):
        nodes, ptr, pins = sc.path_hypergraph(n)
        for eps in sc.EPSILONS:
            all_ones_equals_unweighted(ek, nodes, ptr, pins, np.arange(n, dtype=np.float64), eps)
    nodes, ptr, pins = sc.ten_node_case()
    for eps in (0.0, 0.5, 10.0):
        all_ones_equals_unweighted(ek, nodes, ptr, pins, np.arange(10, dtype=np.float64), eps)
    for n in (2, 3, 63, 65, sc.TILE + 1):
        nodes, ptr, pins = sc.shape_hypergraph(n)
        all_ones_equals_unweighted(ek, nodes, ptr, pins, sc.value_families(n)["normal"], 0.03)
    h = ek.Hypergraph.read(circuit_path("fract"))
    all_ones_equals_unweighted(ek, h.nodes, *h.pins(), sc.value_families(h.nodes)["normal"], 0.03)


def cross_check(ek, h, v, splits):
    """profile_w, the count profile and P against the metrics of the rank split, computed by other code."""
    _, order, profw, prefix = ek.sweep_cut_w_host(h, v)
    _, order0, profile = ek.sweep_cut_host(h, v)
    assert np.array_equal(order, order0)
    W = int(prefix[-1])
    for s in splits:
        bits = ek.rank_split(v, s)
        assert ek.bipart_metrics_host(h, bits) == (profw[s], profile[s], W - prefix[s], prefix[s]), s
        assert set(order[:s].tolist()) == set(np.flatnonzero(bits).tolist()), s


@pytest.mark.parametrize("name", ["random", "metrics+all", "hubs", "degenerate", "cross_2_32", "zero_run", "heavy_node",
                                  "family-three-values", "family-inf-denormal-nan"])
def test_profile_and_prefix_are_the_metrics_of_every_rank_split(ek, name):
    h, v, _ = wc.hypergraph(ek, name)
    cross_check(ek, h, v, range(h.nodes + 1))


def test_profile_and_prefix_are_the_metrics_of_sampled_rank_splits_ibm01(ek):
    h = ek.Hypergraph.read(circuit_path("ibm01"))
    h.set_weights(*wc.synthetic_weights(h.nodes, h.nets))
    nodes = h.nodes
    rng = np.random.default_rng(4)
    v = rng.standard_normal(nodes)
    v[rng.integers(0, nodes, nodes // 4)] = 0.5  # a long run of equal keys
    splits = sorted({0, 1, nodes // 2, nodes - 1, nodes} | set(rng.integers(0, nodes + 1, 45).tolist()))
    cross_check(ek, h, v, splits)
    for eps in wc.EPSILONS:
        res, _, profw, prefix = ek.sweep_cut_w_host(h, v, eps)
        check_result(res, profw, prefix)
        assert res["feasible"] == 1 and res["max_part"] == wc.max_part(res["total_weight"], eps)


def test_einval_guards(ek):
    h, v, _ = wc.hypergraph(ek, "random")
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.sweep_cut_w_host(h, v, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    one = ek.Hypergraph.from_pins(1, np.array([0, 1], np.int64), np.array([0], np.int32))
    with pytest.raises(ek.EKError) as e:  # n < 2
        ek.sweep_cut_w_host(one, np.zeros(1))
    assert e.value.code == ek.EK_EINVAL
    o = ek.SweepOpts()
    ek.lib.ek_sweep_default_opts(ctypes.byref(o))
    r = ek.SweepWResult()
    args = (h._h, v.ctypes.data_as(ctypes.c_void_p), ctypes.byref(o), None, None, None)
    for objective in (-1, 1, 2):  # no ratio objective in the weighted entries
        o.objective = objective
        assert ek.lib.ek_sweep_cut_w_host(*args, ctypes.byref(r)) == ek.EK_EINVAL, objective
    # the outputs are optional, and so are the opts (objective 0, imbalance 0.03)
    o.objective = 0
    assert ek.lib.ek_sweep_cut_w_host(*args, None) == 0
    assert ek.lib.ek_sweep_cut_w_host(h._h, v.ctypes.data_as(ctypes.c_void_p), None, None, None, None,
                                      ctypes.byref(r)) == 0
    assert r.max_part == wc.max_part(r.total_weight, 0.03)
    assert ek.lib.ek_sweep_cut_w_host(None, v.ctypes.data_as(ctypes.c_void_p), None, None, None, None, None) == ek.EK_EINVAL
    assert ek.lib.ek_sweep_cut_w_host(h._h, None, None, None, None, None, None) == ek.EK_EINVAL
    # (W or the sum of c(e) above 2^62 cannot be built: fewer than 2^31 int32 weights sum to less than 2^62, and
    # ek_hgr_set_weights refuses a negative node weight and a net weight below 1 before the sweep would see one;
    # those two range checks are stated by the rule and not reachable from here)
    with pytest.raises(ek.EKError):
        h.set_weights(-np.ones(h.nodes, np.int32), None)


def test_exports_and_struct_layout(ek, tmp_path):
    for name in ("ek_sweep_cut_w_host", "ek_sweep_cut_w", "ek_kl_set_partition_fiedler_sweep_w"):
        assert hasattr(ek.lib, name), name
    res = [n for n, _ in ek.SweepWResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(ek_sweep_w_result));']
    lines += [f'  printf("%zu\\n", offsetof(ek_sweep_w_result, {n}));' for n in res]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(ek.SweepWResult)] + [getattr(ek.SweepWResult, n).offset for n in res]
    assert ek.ABI_VERSION == 4 and ek.lib.ek_abi_version() == 4  # a new struct only: no existing layout changed
