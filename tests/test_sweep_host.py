"""The sweep cut on the host (ek_sweep_cut_host, the device path's checker)
against the rule restated in Python (sweep_cases.sweep_ref), against the
existing rank split and k-way metrics, and on cases whose answer is known."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
from conftest import REPO, circuit_path


@pytest.fixture(scope="module")
def graphs(ek):
    out = {}
    for name, (nodes, ptr, pins) in sc.small_hypergraphs().items():
        out[name] = (ek.Hypergraph.from_pins(nodes, ptr, pins), nodes, ptr, pins)
    for name in ("fract", "ibm01"):
        h = ek.Hypergraph.read(circuit_path(name))
        out[name] = (h, h.nodes, *h.pins())
    return out


def check_result(res, order, profile, n, eps):
    lmax, s_lo, s_hi = sc.window(n, eps)
    assert (res["max_part"], res["s_lo"], res["s_hi"]) == (lmax, s_lo, s_hi)
    assert s_lo <= n // 2 <= s_hi and s_lo <= res["n1"] <= s_hi and res["n0"] + res["n1"] == n == res["n"]
    assert res["cut"] == profile[res["n1"]] and res["cut_mid"] == profile[n // 2]
    assert res["cut"] <= res["cut_mid"] <= res["spanning_nets"]
    assert profile[0] == 0 and profile[n] == 0 and len(profile) == n + 1
    assert sorted(order.tolist()) == list(range(n))
    assert max(res["n0"], res["n1"]) <= lmax


@pytest.mark.parametrize("name", sorted(sc.small_hypergraphs()) + ["fract"])
@pytest.mark.parametrize("ratio", [False, True])
def test_host_equals_the_rule(ek, graphs, name, ratio):
    h, nodes, ptr, pins = graphs[name]
    for fam, v in sc.value_families(nodes).items():
        for eps in sc.EPSILONS if fam == "normal" else (0.03,):
            res, order, profile = ek.sweep_cut_host(h, v, eps, ratio)
            want, worder, wprofile = sc.sweep_ref(nodes, ptr, pins, v, eps, ratio)
            assert np.array_equal(order, worder), (fam, eps)
            assert np.array_equal(profile, wprofile), (fam, eps)
            assert sc.ints(res) == want, (fam, eps)
            check_result(res, order, profile, nodes, eps)


def cross_check(ek, g, v, splits):
    _, nodes, ptr, pins = g
    _, order, profile = ek.sweep_cut_host(g[0], v)
    for s in splits:
        bits = ek.rank_split(v, s)
        assert profile[s] == ek.kway_metrics_host(ptr, pins, bits.astype(np.int32), 2)[0], s
        assert set(order[:s].tolist()) == set(np.flatnonzero(bits).tolist()), s


@pytest.mark.parametrize("name", ["random", "metrics+all", "hubs"])
def test_profile_is_the_cut_of_every_rank_split(ek, graphs, name):
    nodes = graphs[name][1]
    fams = sc.value_families(nodes, 1)
    for fam in ("normal", "three-values", "inf-denormal-nan"):
        cross_check(ek, graphs[name], fams[fam], range(nodes + 1))


def test_profile_is_the_cut_of_sampled_rank_splits_ibm01(ek, graphs):
    nodes = graphs["ibm01"][1]
    rng = np.random.default_rng(4)
    v = rng.standard_normal(nodes)
    v[rng.integers(0, nodes, nodes // 4)] = 0.5  # a long run of equal keys
    splits = sorted({0, 1, nodes // 2, nodes - 1, nodes} | set(rng.integers(0, nodes + 1, 45).tolist()))
    cross_check(ek, graphs["ibm01"], v, splits)


@pytest.mark.parametrize("n", [2, 3, 10, 11, 64, 65])
@pytest.mark.parametrize("ratio", [False, True])
def test_path_takes_the_most_balanced_split(ek, n, ratio):
    nodes, ptr, pins = sc.path_hypergraph(n)
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    for eps in sc.EPSILONS:
        res, order, profile = ek.sweep_cut_host(h, np.arange(n, dtype=np.float64), eps, ratio)
        assert order.tolist() == list(range(n))
        assert profile.tolist() == [0] + [1] * (n - 1) + [0]
        assert (res["n1"], res["cut"], res["cut_mid"], res["spanning_nets"]) == (n // 2, 1, 1, n - 1)
        check_result(res, order, profile, n, eps)


def test_minimum_cut_and_ratio_cut_differ_where_they_should(ek):
    nodes, ptr, pins = sc.ten_node_case()
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    v = np.arange(10, dtype=np.float64)
    res, _, profile = ek.sweep_cut_host(h, v, 10.0, False)
    assert profile.tolist() == [0, 1, 3, 3, 3, 2, 3, 3, 3, 3, 0]
    assert (res["s_lo"], res["s_hi"], res["n1"], res["cut"], res["cut_mid"]) == (1, 9, 1, 1, 2)
    res, _, _ = ek.sweep_cut_host(h, v, 10.0, True)  # 2/25 < 1/9
    assert (res["n1"], res["cut"]) == (5, 2)
    for ratio in (False, True):  # eps 0: the window is the median alone
        res, _, _ = ek.sweep_cut_host(h, v, 0.0, ratio)
        assert (res["s_lo"], res["s_hi"], res["n1"]) == (5, 5, 5)
        # eps 0.5: L_max = 7, the window 3..7 leaves s = 1 out
        res, _, _ = ek.sweep_cut_host(h, v, 0.5, ratio)
        assert (res["s_lo"], res["s_hi"], res["n1"], res["cut"]) == (3, 7, 5, 2)


def test_value_families_order(ek, graphs):
    h, nodes, _, _ = graphs["random"]
    _, order, _ = ek.sweep_cut_host(h, np.full(nodes, -3.5))
    assert order.tolist() == list(range(nodes))  # all equal: id order
    v = np.resize(np.array([1.0, 0.0, -0.0]), nodes)
    _, order, _ = ek.sweep_cut_host(h, v)
    ids = np.arange(nodes)
    assert order.tolist() == ids[2::3].tolist() + ids[1::3].tolist() + ids[0::3].tolist()  # -0 < +0 < 1
    v = np.resize(np.array([np.nan, np.inf, 5e-324, -5e-324, -np.inf, -np.nan]), nodes)
    _, order, _ = ek.sweep_cut_host(h, v)
    want = [ids[j::6].tolist() for j in (5, 4, 3, 2, 1, 0)]  # -nan < -inf < -denormal < +denormal < +inf < +nan
    assert order.tolist() == sum(want, [])


def test_einval_guards_and_defaults(ek, graphs):
    h, nodes, _, _ = graphs["random"]
    v = np.zeros(nodes)
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.sweep_cut_host(h, v, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    one = ek.Hypergraph.from_pins(1, np.array([0, 1], np.int64), np.array([0], np.int32))
    with pytest.raises(ek.EKError) as e:
        ek.sweep_cut_host(one, np.zeros(1))
    assert e.value.code == ek.EK_EINVAL
    o = ek.SweepOpts()
    ek.lib.ek_sweep_default_opts(ctypes.byref(o))
    assert (o.objective, o.imbalance) == (0, 0.03)
    r = ek.SweepResult()
    for objective in (-1, 2):
        o.objective = objective
        rc = ek.lib.ek_sweep_cut_host(h._h, v.ctypes.data_as(ctypes.c_void_p), ctypes.byref(o), None, None,
                                      ctypes.byref(r))
        assert rc == ek.EK_EINVAL, objective
    # the outputs are optional
    o.objective = 1
    assert ek.lib.ek_sweep_cut_host(h._h, v.ctypes.data_as(ctypes.c_void_p), ctypes.byref(o), None, None, None) == 0
    assert ek.lib.ek_sweep_cut_host(h._h, v.ctypes.data_as(ctypes.c_void_p), None, None, None, ctypes.byref(r)) == 0
    assert r.max_part == sc.window(nodes, 0.03)[0]


def test_struct_layout_matches_python_mirror(ek, tmp_path):
    opts = [n for n, _ in ek.SweepOpts._fields_]
    res = [n for n, _ in ek.SweepResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(ek_sweep_opts), sizeof(ek_sweep_result));']
    lines += [f'  printf("%zu\\n", offsetof(ek_sweep_opts, {n}));' for n in opts]
    lines += [f'  printf("%zu\\n", offsetof(ek_sweep_result, {n}));' for n in res]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(ek.SweepOpts), ctypes.sizeof(ek.SweepResult)]
    want += [getattr(ek.SweepOpts, n).offset for n in opts]
    want += [getattr(ek.SweepResult, n).offset for n in res]
    assert got == want
    assert ek.ABI_VERSION == 4 and ek.lib.ek_abi_version() == 4  # new structs only: no existing layout changed
