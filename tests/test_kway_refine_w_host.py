"""ek_kway_refine_w_host (no GPU): against the plain-Python restatement of the
rule of DESIGN.md §17 on every case, against ek_kway_refine_host under unit
weights, and the properties the rule promises: the weighted connectivity falls
by exactly the logged gains, no part ends above max(L_p, its initial weight),
the accepted set of a part is the longest prefix that fits."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_w_cases as wc
from conftest import PKG_DIR, REPO, circuit_path


@pytest.fixture(scope="module")
def circuits(ek):
    out = {}
    for name in ("fract", "ibm01"):
        plain = ek.Hypergraph.read(circuit_path(name))
        ptr, pins = plain.pins()
        node_w, net_w = wc.synthetic_weights(plain.nodes, len(ptr) - 1)
        weighted = ek.Hypergraph.read(circuit_path(name))
        weighted.set_weights(node_w, net_w)
        out[name] = {"ones": (plain, None, None), "synthetic": (weighted, node_w, net_w), "pins": (ptr, pins)}
    return out


def run_case(ek, case, h=None):
    h = wc.hypergraph(ek, case) if h is None else h
    want, want_log, L = wc.refine_w_ref(case["nodes"], case["ptr"], case["pins"], case["node_w"], case["net_w"],
                                        case["start"], case["k"], case["eps"], case["max_rounds"], case["bounds"])
    part, res, log = ek.kway_refine_w_host(h, case["start"], case["k"], case["eps"], case["max_rounds"], case["bounds"])
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert np.array_equal(log, want_log), (log[:4].tolist(), want_log[:4].tolist())
    wc.check_properties(ek, h, case["start"], case["k"], L, part, res, log)
    return part, res, log


def expected_moves(case):
    m = case["moved"]
    return m if isinstance(m, dict) else {v: 1 for v in m}


@pytest.mark.parametrize("name", list(wc.built_cases()))
def test_host_equals_restatement(ek, name):
    case = wc.built_cases()[name]
    part, res, log = run_case(ek, case)
    if case["moved"] is not None:  # the first round moves exactly these
        assert case["max_rounds"] == 1
        moved = {int(v): int(part[v]) for v in np.flatnonzero(part != case["start"])}
        assert moved == expected_moves(case)
        assert res["rounds"] == (1 if moved else 0)


def test_the_cases_cover_what_they_are_for(ek):
    cases = wc.built_cases()
    # k = 256: the node's own part and its target sit in each of the four mask words
    own, tgt = set(), set()
    for name in ("gain-k256-perm", "gain-k256-edge"):
        case = cases[name]
        part, _, _ = ek.kway_refine_w_host(wc.hypergraph(ek, case), case["start"], 256, case["eps"])
        for v in np.flatnonzero(part != case["start"]):
            own.add(int(case["start"][v]) >> 6)
            tgt.add(int(part[v]) >> 6)
    assert own == {0, 1, 2, 3} and tgt == {0, 1, 2, 3}
    # apply: every part both gives and receives in one round
    case = cases["apply-ring-k5"]
    assert {case["start"][v] for v in case["moved"]} == set(case["moved"].values()) == set(range(5))
    # the prefix rule leaves the light nodes to later rounds, which a greedy skip would have taken at once
    case = cases["select-prefix-later-rounds"]
    part, res, log = ek.kway_refine_w_host(wc.hypergraph(ek, case), case["start"], 2, 0.0, 0, case["bounds"])
    assert log[0].tolist() == [4, 4, 1, 9] and res["rounds"] >= 2 and part[2] == part[3] == 1 and part[1] == 0
    # zero-weight nodes: in front of the first rejected node only
    case = cases["select-zero-weights"]
    _, _, log = ek.kway_refine_w_host(wc.hypergraph(ek, case), case["start"], 2, 0.0, 1, case["bounds"])
    assert log[0, :3].tolist() == [7, 7, 4]
    # an over-full part receives nothing, not even a node of weight 0
    case = cases["select-overfull"]
    _, res, log = ek.kway_refine_w_host(wc.hypergraph(ek, case), case["start"], 2, 0.0, 0, case["bounds"])
    assert len(log) == 0 and res["parts_over_bound"] == 1 and res["moves"] == 0


def test_id_byte_3(ek):
    """The first rejected key parts from the last accepted one in key byte 3: ids past 2^24."""
    case = wc.id_byte3_case()
    part, res, log = run_case(ek, case)
    moved = set(np.flatnonzero(part != case["start"]).tolist())
    assert moved == case["moved"] and log.tolist() == [[4, 4, 2, 14]]


@pytest.mark.parametrize("case", wc.circuit_cases(), ids=[c[0] for c in wc.circuit_cases()])
def test_circuits_equal_restatement(ek, circuits, case):
    name, g, wt, s, k, eps, max_rounds = case
    h, node_w, net_w = circuits[g][wt]
    ptr, pins = circuits[g]["pins"]
    start = rc.starts(h.nodes, k)[s]
    c = dict(nodes=h.nodes, ptr=ptr, pins=pins, node_w=node_w, net_w=net_w, start=start, k=k, eps=eps,
             max_rounds=max_rounds, bounds=None)
    part, res, log = run_case(ek, c, h)
    if max_rounds:
        assert res["rounds"] <= max_rounds
    if name == wc.BINDING:
        assert np.any(log[:, 2] < log[:, 1])  # the bound binds: a prefix is cut short
    # bounds set to the uniform value: the same run
    L = np.full(k, wc.uniform_bound(res["total_weight"], k, eps), np.int64)
    again, res2, log2 = ek.kway_refine_w_host(h, start, k, 0.9, max_rounds, L)  # (the imbalance is then ignored)
    assert np.array_equal(again, part) and np.array_equal(log2, log)
    assert {f: res2[f] for f in wc.INTS} == {f: res[f] for f in wc.INTS}


def same_as_unweighted(got, want):
    part, res, log = got
    upart, ures, ulog = want
    assert np.array_equal(part, upart) and np.array_equal(log, ulog)
    assert {f: res[f] for f in wc.SHARED_WITH_UNWEIGHTED} == {f: ures[u] for f, u in wc.SHARED_WITH_UNWEIGHTED.items()}
    assert res["total_weight"] == len(part)
    assert res["parts_over_bound"] == int(np.count_nonzero(np.bincount(part, minlength=res["k"]) > ures["max_part"]))


@pytest.fixture(scope="module")
def plain_graphs(ek, circuits):
    out = {name: ek.Hypergraph.from_pins(nodes, ptr, pins) for name, (nodes, ptr, pins) in rc.small_hypergraphs().items()}
    out.update({name: circuits[name]["ones"][0] for name in ("fract", "ibm01")})
    return out


@pytest.mark.parametrize("name,g,s,k,eps", rc.small_cases(), ids=[c[0] for c in rc.small_cases()])
def test_unit_weights_are_the_unweighted_rule_small(ek, plain_graphs, name, g, s, k, eps):
    h = plain_graphs[g]
    start = rc.starts(h.nodes, k)[s]
    same_as_unweighted(ek.kway_refine_w_host(h, start, k, eps), ek.kway_refine_host(h, start, k, eps))


@pytest.mark.parametrize("case", rc.circuit_cases(), ids=[c[0] for c in rc.circuit_cases()])
def test_unit_weights_are_the_unweighted_rule_circuits(ek, plain_graphs, case):
    _, g, s, k, eps, max_rounds = case
    h = plain_graphs[g]
    start = rc.starts(h.nodes, k)[s]
    same_as_unweighted(ek.kway_refine_w_host(h, start, k, eps, max_rounds),
                       ek.kway_refine_host(h, start, k, eps, max_rounds))


def test_fixed_point_and_round_limit(ek, circuits):
    h, _, _ = circuits["fract"]["synthetic"]
    start = rc.starts(h.nodes, 4)["perm"]
    part, res, log = ek.kway_refine_w_host(h, start, 4, 0.05)
    assert res["rounds"] >= 2
    again, res2, log2 = ek.kway_refine_w_host(h, part, 4, 0.05)
    assert np.array_equal(again, part) and res2["moves"] == 0 and res2["rounds"] == 0 and len(log2) == 0
    assert res2["connectivity_w_before"] == res2["connectivity_w"] == res["connectivity_w"]
    one, res1, log1 = ek.kway_refine_w_host(h, start, 4, 0.05, max_rounds=1)
    assert res1["rounds"] == 1 and np.array_equal(log1, log[:1])
    rest, _, log3 = ek.kway_refine_w_host(h, one, 4, 0.05)
    assert np.array_equal(rest, part) and np.array_equal(log3, log[1:])


def test_einval_guards(ek):
    nodes, ptr, pins = rc.small_hypergraphs()["random"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    good = rc.starts(nodes, 4)["block"]
    for k in (1, 257, 0):
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_w_host(h, np.zeros(nodes, np.int32), k)
        assert e.value.code == ek.EK_EINVAL, k
    for bad in (-1, 4):
        part = good.copy()
        part[17] = bad
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_w_host(h, part, 4)
        assert e.value.code == ek.EK_EINVAL, bad
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_w_host(h, good, 4, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    for bounds in ([100, -1, 100, 100], [-5, 0, 0, 0]):
        with pytest.raises(ek.EKError) as e:
            ek.kway_refine_w_host(h, good, 4, bounds=bounds)
        assert e.value.code == ek.EK_EINVAL, bounds
    assert ek.kway_refine_w_host(h, good, 4, bounds=[0, 0, 0, 0])[1]["moves"] == 0  # a bound of 0 is a bound
    with pytest.raises(ValueError):
        ek.kway_refine_w_host(h, good, 4, bounds=[1, 2, 3])
    with pytest.raises(ValueError):
        ek.kway_refine_w_host(h, good[:-1], 4)
    # the nets on one node sum to 2^31: one more than a gain holds; 2^31 - 1 is the case gain-int32-max
    two = ek.Hypergraph.from_pins(3, np.array([0, 2, 4], np.int64), np.array([0, 1, 0, 2], np.int32))
    two.set_weights(None, [2 ** 30, 2 ** 30])
    with pytest.raises(ek.EKError) as e:
        ek.kway_refine_w_host(two, [0, 1, 1], 2)
    assert e.value.code == ek.EK_EINVAL


def test_symbols_struct_layout_and_abi(ek, tmp_path):
    hdr = open(os.path.join(REPO, "include", "eigkl.h")).read()
    for name in ("ek_kway_refine_w_host", "ek_kway_refine_w"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(ek.lib, name)
    res = [n for n, _ in ek.KwayRefineWResult._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%zu %d\\n", sizeof(ek_kway_refine_w_result), EIGKL_ABI_VERSION);']
    lines += [f'  printf("%zu\\n", offsetof(ek_kway_refine_w_result, {n}));' for n in res]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(ek.KwayRefineWResult), 4] + [getattr(ek.KwayRefineWResult, n).offset for n in res]
    assert ek.ABI_VERSION == 4 == ek.lib.ek_abi_version()  # a new struct only: no existing layout changed


def test_refine_weighted_cli_misuse_prints_usage(tmp_path):
    """Refused while the arguments are read: no GPU work, no results file.  --refine-weighted follows
    --kway-multilevel only and takes a finite imbalance >= 0; --refine with --kway-multilevel stays refused."""
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    for args in (("-EIG", "--k", "4", "--refine-weighted", "0.05"), ("-EIG", "--refine-weighted", "0.05"),
                 ("-EIG", "--k", "4", "--multilevel", "0.03", "--refine-weighted", "0.05"),
                 ("-EIG", "--k", "4", "--refine", "0.05", "--refine-weighted", "0.05"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "-0.1"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "nan"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "inf"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "x"),
                 ("-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "0.05", "--refine", "0.05")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--kway-multilevel" in r.stdout, args
        assert "--refine-weighted" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.4").exists()
