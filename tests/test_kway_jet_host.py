"""ek_kway_jet_host (no GPU): against the plain-Python restatement of the rule of
DESIGN.md §18 on every case, its stop rule and rollback, the start on which the
weighted pass ek_kway_refine_w_host is stuck and this one is not, and the
properties the rule promises: the result is the best state seen, no part ends
above max(L_p, its initial weight)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import jet_cases as jc
from conftest import PKG_DIR, REPO, circuit_path


def run_case(ek, case):
    h = jc.hypergraph(ek, case)
    want, want_log, _, best_iter, _ = jc.jet_ref(case["nodes"], case["ptr"], case["pins"], case["node_w"],
                                                 case["net_w"], case["start"], case["k"], case["eps"], case["bounds"],
                                                 case["max_iters"], case["patience"], case["neg"])
    part, res, log = jc.run(ek.kway_jet_host, h, case)
    assert np.array_equal(log, want_log), (log[:6].tolist(), want_log[:6].tolist())
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert res["best_iter"] == best_iter
    jc.check_properties(ek, h, case, part, res, log)
    jc.check_expect(case, part, res, log)
    return part, res, log


@pytest.mark.parametrize("name", list(jc.built_cases()))
def test_host_equals_restatement(ek, name):
    run_case(ek, jc.built_cases()[name])


def test_the_cases_cover_what_they_are_for(ek):
    cases = jc.built_cases()
    # k = 256: the node's own part and its target sit in each of the four mask words
    own, tgt = set(), set()
    for name in ("gain-k256-perm", "gain-k256-edge"):
        case = cases[name]
        part, _, _ = jc.run(ek.kway_jet_host, jc.hypergraph(ek, case), case)
        for v in np.flatnonzero(part != case["start"]):
            own.add(int(case["start"][v]) >> 6)
            tgt.add(int(part[v]) >> 6)
    assert own == {0, 1, 2, 3} and tgt == {0, 1, 2, 3}
    # negative-gain candidates, candidates the afterburner turns down, and a bound that cuts a prefix short
    saw_fail = saw_cut = False
    for name in ("gain-k3-edge", "nets-k4", "hubs-k3", "stop-rollback"):
        _, _, log = jc.run(ek.kway_jet_host, jc.hypergraph(ek, cases[name]), cases[name])
        saw_fail |= bool(np.any(log[:, 1] < log[:, 0]))
        saw_cut |= bool(np.any(log[:, 2] < log[:, 1]))
    assert saw_fail and saw_cut
    # a node that moved in iteration i is locked in i + 1 and moves again in i + 2
    case = cases["gain-int32-extremes"]
    *_, states = jc.jet_ref(case["nodes"], case["ptr"], case["pins"], case["node_w"], case["net_w"], case["start"], 2,
                            bounds=case["bounds"], max_iters=4, neg=case["neg"])
    assert [s.tolist() for s in states] == [[0, 1], [1, 1], [1, 1], [1, 0]]


@pytest.mark.parametrize("name", ["stop-patience-1", "stop-iters-1", "stop-iters-2", "stop-rollback",
                                  "stop-no-candidate"])
def test_stop_rule_and_rollback(ek, name):
    case = jc.built_cases()[name]
    h = jc.hypergraph(ek, case)
    part, res, log = run_case(ek, case)
    full, fres, flog = jc.run(ek.kway_jet_host, h, case, max_iters=0, patience=12)
    xs = [res["connectivity_w_before"]] + log[:, 3].tolist()
    if name == "stop-patience-1":  # the first iteration that brings no new best is the last
        assert xs[-1] >= min(xs[:-1]) and all(xs[i] < min(xs[:i]) for i in range(1, len(xs) - 1))
        assert len(log) < len(flog) and np.array_equal(log, flog[:len(log)])
    elif name.startswith("stop-iters"):
        assert res["iters"] == case["max_iters"] and np.array_equal(log, flog[:len(log)])
    elif name == "stop-no-candidate":  # the double-empty stop at i = 1
        assert res["iters"] == 1 and res["moves"] == 0 and np.array_equal(part, case["start"])
    else:  # the last iterations are worse than the best: the returned vector is the snapshot
        assert 0 < res["best_iter"] < res["iters"] and xs[-1] > min(xs)
        assert res["iters"] - res["best_iter"] == case["patience"]
    metrics, _ = ek.kway_metrics_w_host(h, part, case["k"])
    assert metrics[2] == min(xs) == res["connectivity_w"]


def test_it_leaves_a_minimum_the_weighted_pass_cannot(ek):
    case = jc.built_cases()["escape"]
    h = jc.hypergraph(ek, case)
    stuck, sres, slog = ek.kway_refine_w_host(h, case["start"], 2, bounds=case["bounds"])
    assert np.array_equal(stuck, case["start"]) and sres["moves"] == 0 and len(slog) == 0
    assert sres["connectivity_w"] == 14
    part, res, log = jc.run(ek.kway_jet_host, h, case)
    assert res["connectivity_w_before"] == 14 and res["connectivity_w"] == 0 and res["best_iter"] == 2
    assert log[:2].tolist() == [[2, 1, 1, 15], [1, 1, 1, 0]]  # up by 1, then down by 15
    assert part.tolist() == [1] * 6 and res["parts_over_bound"] == 0
    # with no negative-gain proposals the pass is stuck too
    part0, res0, _ = jc.run(ek.kway_jet_host, h, case, neg=(0, 1))
    assert np.array_equal(part0, case["start"]) and res0["moves"] == 0


@pytest.mark.parametrize("name", list(jc.random_cases()))
def test_promises_on_random_hypergraphs(ek, name):
    case = jc.random_cases()[name]
    h = jc.hypergraph(ek, case)
    part, res, log = run_case(ek, case)
    assert res["connectivity_w"] <= res["connectivity_w_before"]
    # the log's X_i against independent recounts of the intermediate vectors: after i iterations the state is the
    # snapshot whenever X_i is a new best; otherwise the recount of the restatement's state stands in
    *_, states = jc.jet_ref(case["nodes"], case["ptr"], case["pins"], case["node_w"], case["net_w"], case["start"],
                            case["k"], case["eps"], case["bounds"], case["max_iters"], case["patience"], case["neg"])
    best = res["connectivity_w_before"]
    for i in range(1, res["iters"] + 1):
        at, ares, alog = jc.run(ek.kway_jet_host, h, case, max_iters=i)
        assert np.array_equal(alog, log[:i])
        x = int(log[i - 1, 3])
        assert ek.kway_metrics_w_host(h, states[i - 1], case["k"])[0][2] == x
        if x < best:
            best = x
            assert ares["best_iter"] == i and np.array_equal(at, states[i - 1])
            assert ek.kway_metrics_w_host(h, at, case["k"])[0][2] == x
        assert ares["connectivity_w"] == best


def test_einval_guards(ek):
    case = jc.built_cases()["escape"]
    h = jc.hypergraph(ek, case)
    good = case["start"]
    for kw in (dict(neg=(-1, 4)), dict(neg=(1, 0)), dict(neg=(1, -2)), dict(patience=0), dict(patience=-3)):
        with pytest.raises(ek.EKError) as e:
            ek.kway_jet_host(h, good, 2, **kw)
        assert e.value.code == ek.EK_EINVAL, kw
    for k in (1, 257, 0):
        with pytest.raises(ek.EKError) as e:
            ek.kway_jet_host(h, np.zeros(6, np.int32), k)
        assert e.value.code == ek.EK_EINVAL, k
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.kway_jet_host(h, good, 2, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    bad = good.copy()
    bad[3] = 2
    with pytest.raises(ek.EKError) as e:
        ek.kway_jet_host(h, bad, 2)
    assert e.value.code == ek.EK_EINVAL
    with pytest.raises(ek.EKError) as e:
        ek.kway_jet_host(h, good, 2, bounds=[6, -1])
    assert e.value.code == ek.EK_EINVAL
    with pytest.raises(ValueError):
        ek.kway_jet_host(h, good, 2, bounds=[1, 2, 3])
    with pytest.raises(ValueError):
        ek.kway_jet_host(h, good[:-1], 2)
    # neg_num = 0 and max_iters <= 0 are values, not errors
    assert ek.kway_jet_host(h, good, 2, bounds=[6, 6], neg=(0, 1), max_iters=-1)[1]["iters"] == 1
    # no net of two distinct pins: the call returns at once
    lone = ek.Hypergraph.from_pins(4, np.array([0, 1, 3], np.int64), np.array([2, 1, 1], np.int32))
    lone.set_weights([3, 0, 2, 1], [4, 5])
    part, res, log = ek.kway_jet_host(lone, [0, 1, 0, 1], 2, 0.5)
    assert part.tolist() == [0, 1, 0, 1] and res["iters"] == 0 and len(log) == 0 and res["connectivity_w"] == 0
    assert (res["part_w_min"], res["part_w_max"], res["total_weight"]) == (1, 5, 6)


def test_symbols_struct_layout_and_abi(ek, tmp_path):
    hdr = open(os.path.join(REPO, "include", "eigkl.h")).read()
    for name in ("ek_kway_jet_host", "ek_kway_jet", "ek_kway_jet_default_opts"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(ek.lib, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%d\\n", EIGKL_ABI_VERSION);']
    want = [4]
    for c_name, cls in (("ek_kway_jet_result", ek.KwayJetResult), ("ek_kway_jet_opts", ek.KwayJetOpts)):
        fields = [n for n, _ in cls._fields_]
        lines += [f'  printf("%zu\\n", sizeof({c_name}));']
        lines += [f'  printf("%zu\\n", offsetof({c_name}, {n}));' for n in fields]
        want += [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ek.ABI_VERSION == 4 == ek.lib.ek_abi_version()  # new structs only: no existing layout changed
    o = ek.KwayJetOpts()
    ek.lib.ek_kway_jet_default_opts(ctypes.byref(o))
    assert (o.k, o.max_iters, o.patience, o.neg_num, o.neg_den, o.imbalance) == (2, 0, 12, 1, 4, 0.03)


def test_refine_jet_cli_misuse_prints_usage(tmp_path):
    """Refused while the arguments are read: no GPU work, no results file.  --refine-jet follows --kway-multilevel
    only, excludes --refine-weighted and takes a finite imbalance >= 0."""
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    ml = ("-EIG", "--k", "4", "--kway-multilevel", "0.03")
    for args in (("-EIG", "--k", "4", "--refine-jet", "0.05"), ("-EIG", "--refine-jet", "0.05"),
                 ("-EIG", "--k", "4", "--multilevel", "0.03", "--refine-jet", "0.05"),
                 (*ml, "--refine-weighted", "0.05", "--refine-jet", "0.05"),
                 (*ml, "--refine-jet", "0.05", "--refine-weighted", "0.05"),
                 (*ml, "--refine-jet"), (*ml, "--refine-jet", "-0.1"), (*ml, "--refine-jet", "nan"),
                 (*ml, "--refine-jet", "inf"), (*ml, "--refine-jet", "x"), (*ml, "--jet-iters", "3"),
                 (*ml, "--refine-jet", "0.05", "--jet-iters"), (*ml, "--refine-jet", "0.05", "--refine", "0.05")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--kway-multilevel" in r.stdout, (args, r.stdout)
        assert "--refine-jet" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.4").exists()
