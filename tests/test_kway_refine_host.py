"""ek_kway_refine_host (no GPU): against the plain-Python restatement of the
rule on the small cases, and the properties the rule promises: the
connectivity falls by exactly the logged gains, the cap holds (and binds), a
converged vector is a fixed point."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from conftest import REPO, circuit_path


@pytest.fixture(scope="module")
def graphs(ek):
    out = {}
    for name, (nodes, ptr, pins) in rc.small_hypergraphs().items():
        out[name] = (ek.Hypergraph.from_pins(nodes, ptr, pins), nodes, ptr, pins)
    for name in ("fract", "ibm01"):
        h = ek.Hypergraph.read(circuit_path(name))
        out[name] = (h, h.nodes, *h.pins())
    return out


@pytest.mark.parametrize("name,g,s,k,eps", rc.small_cases(), ids=[c[0] for c in rc.small_cases()])
def test_host_equals_restatement(ek, graphs, name, g, s, k, eps):
    h, nodes, ptr, pins = graphs[g]
    start = rc.starts(nodes, k)[s]
    # (the restatement takes a second a round on the 20,000 pins of "metrics" at large k: two rounds there)
    rounds = 2 if g == "metrics" and k >= 63 else 0
    want, want_log, lmax = rc.refine_ref(nodes, ptr, pins, start, k, eps, rounds)
    part, res, log = ek.kway_refine_host(h, start, k, eps, rounds)
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert np.array_equal(log, want_log)
    assert res["max_part"] == lmax
    rc.check_properties(ek, graphs[g], start, k, eps, part, res, log)


def test_fract_restatement_and_cap_binds(ek, graphs):
    h, nodes, ptr, pins = graphs["fract"]
    start = rc.starts(nodes, 4)["block"]
    want, want_log, lmax = rc.refine_ref(nodes, ptr, pins, start, 4, 0.05)
    assert lmax == 39 and np.any(want_log[:, 2] < want_log[:, 1])  # the cap binds in some round
    part, res, log = ek.kway_refine_host(h, start, 4, 0.05)
    assert np.array_equal(part, want) and np.array_equal(log, want_log)
    assert np.any(log[:, 2] < log[:, 1]) and res["part_max"] <= 39
    rc.check_properties(ek, graphs["fract"], start, 4, 0.05, part, res, log)
    assert res["connectivity"] < res["connectivity_before"]


@pytest.mark.parametrize("case", rc.circuit_cases(), ids=[c[0] for c in rc.circuit_cases()])
def test_circuit_properties(ek, graphs, case):
    _, g, s, k, eps, max_rounds = case
    h, nodes, ptr, pins = graphs[g]
    start = rc.starts(nodes, k)[s]
    part, res, log = ek.kway_refine_host(h, start, k, eps, max_rounds)
    rc.check_properties(ek, graphs[g], start, k, eps, part, res, log)
    if max_rounds:
        assert res["rounds"] <= max_rounds


def test_fixed_point_and_first_round(ek, graphs):
    for g, k, eps in (("random", 3, 0.05), ("metrics", 65, 0.5), ("fract", 4, 0.05)):
        h, nodes, ptr, pins = graphs[g]
        start = rc.starts(nodes, k)["perm"]
        part, res, log = ek.kway_refine_host(h, start, k, eps)
        assert res["rounds"] >= 2, g
        again, res2, log2 = ek.kway_refine_host(h, part, k, eps)
        assert np.array_equal(again, part) and res2["moves"] == 0 and res2["rounds"] == 0 and len(log2) == 0
        assert res2["connectivity_before"] == res2["connectivity"] == res["connectivity"]
        # max_rounds = 1: the first round of the unlimited run; 2 more from there: its first three
        one, res1, log1 = ek.kway_refine_host(h, start, k, eps, max_rounds=1)
        assert res1["rounds"] == 1 and np.array_equal(log1, log[:1])
        assert np.array_equal(one, rc.refine_ref(nodes, ptr, pins, start, k, eps, max_rounds=1)[0])
        three, _, log3 = ek.kway_refine_host(h, one, k, eps, max_rounds=2)
        assert np.array_equal(log3, log[1:3])
        if res["rounds"] <= 3:
            assert np.array_equal(three, part)


def test_zero_imbalance_equal_parts_is_fixed(ek, graphs):
    for g, k in (("random", 3), ("random", 2), ("metrics", 2)):
        h, nodes, _, _ = graphs[g]
        assert nodes % k == 0
        for s in ("block", "perm"):
            start = rc.starts(nodes, k)[s]
            part, res, log = ek.kway_refine_host(h, start, k, 0.0)
            assert np.array_equal(part, start) and res["moves"] == 0 and len(log) == 0
            assert res["max_part"] == nodes // k == res["part_min"] == res["part_max"]


def test_overfull_part_never_receives(ek, graphs):
    h, nodes, ptr, pins = graphs["random"]
    start = np.zeros(nodes, np.int32)
    start[200:] = np.arange(100) % 2 + 1  # part 0 holds 200 of 300, L_max = 105
    part, res, log = ek.kway_refine_host(h, start, 3, 0.05)
    assert res["max_part"] == 105
    assert not np.any((part == 0) & (start != 0))
    rc.check_properties(ek, graphs["random"], start, 3, 0.05, part, res, log)
    want, want_log, _ = rc.refine_ref(nodes, ptr, pins, start, 3, 0.05)
    assert np.array_equal(part, want) and np.array_equal(log, want_log)


def test_einval_guards(ek, graphs):
    h, nodes, _, _ = graphs["random"]
    good = rc.starts(nodes, 4)["block"]
    for k in (1, 257, 0):
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_host(h, np.zeros(nodes, np.int32), k)
        assert e.value.code == ek.EK_EINVAL, k
    for bad in (-1, 4):
        part = good.copy()
        part[17] = bad
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_host(h, part, 4)
        assert e.value.code == ek.EK_EINVAL, bad
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_host(h, good, 4, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    o = ek.KwayRefineOpts()
    ek.lib.ek_kway_refine_default_opts(ctypes.byref(o))
    assert (o.k, o.max_rounds, o.imbalance) == (2, 0, 0.03)


def test_struct_layout_matches_python_mirror(ek, tmp_path):
    opts = [n for n, _ in ek.KwayRefineOpts._fields_]
    res = [n for n, _ in ek.KwayRefineResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu %zu\\n", sizeof(ek_kway_refine_opts), sizeof(ek_kway_refine_result));']
    lines += [f'  printf("%zu\\n", offsetof(ek_kway_refine_opts, {n}));' for n in opts]
    lines += [f'  printf("%zu\\n", offsetof(ek_kway_refine_result, {n}));' for n in res]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    got = [int(x) for x in out]
    want = [ctypes.sizeof(ek.KwayRefineOpts), ctypes.sizeof(ek.KwayRefineResult)]
    want += [getattr(ek.KwayRefineOpts, n).offset for n in opts]
    want += [getattr(ek.KwayRefineResult, n).offset for n in res]
    assert got == want
    assert ek.ABI_VERSION == 4  # new structs only: no existing layout changed
