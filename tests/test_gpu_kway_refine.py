"""The k-way refinement on the GPU (ek_kway_refine) against its host checker
(ek_kway_refine_host): the rule is integer and every tie is broken by ids, so
the part vector, the round log and every integer of the result must be
identical, whatever order the workgroups run in."""
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def graphs(ek):
    out = {}
    for name, (nodes, ptr, pins) in rc.small_hypergraphs().items():
        out[name] = (ek.Hypergraph.from_pins(nodes, ptr, pins), nodes, ptr, pins)
    for name in ("fract", "ibm01"):
        h = ek.Hypergraph.read(circuit_path(name))
        out[name] = (h, h.nodes, *h.pins())
    return out


def same_as_host(ek, ctx, g, start, k, eps, max_rounds=0):
    h, _, ptr, pins = g
    want, wres, wlog = ek.kway_refine_host(h, start, k, eps, max_rounds)
    part, res, log = ctx.kway_refine(h, start, k, eps, max_rounds)
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert np.array_equal(log, wlog), (log[:4].tolist(), wlog[:4].tolist())
    assert {f: res[f] for f in rc.INTS} == {f: wres[f] for f in rc.INTS}
    assert (res["cut_nets"], res["connectivity"], res["soed"]) == ctx.kway_metrics(ptr, pins, part, k)
    return part, res, log


@pytest.mark.parametrize("name,g,s,k,eps", rc.small_cases(), ids=[c[0] for c in rc.small_cases()])
def test_device_equals_host_small(ek, ctx, graphs, name, g, s, k, eps):
    start = rc.starts(graphs[g][1], k)[s]
    part, res, log = same_as_host(ek, ctx, graphs[g], start, k, eps)
    rc.check_properties(ek, graphs[g], start, k, eps, part, res, log)


@pytest.mark.parametrize("case", rc.circuit_cases(), ids=[c[0] for c in rc.circuit_cases()])
def test_device_equals_host_circuits(ek, ctx, graphs, case):
    _, g, s, k, eps, max_rounds = case
    start = rc.starts(graphs[g][1], k)[s]
    part, res, log = same_as_host(ek, ctx, graphs[g], start, k, eps, max_rounds)
    rc.check_properties(ek, graphs[g], start, k, eps, part, res, log)
    if case[0] == "fract-block-k4-e0.05":
        assert np.any(log[:, 2] < log[:, 1])  # the cap binds: the device selects a threshold key
    if max_rounds:
        assert res["rounds"] <= max_rounds


@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("k", [3, 4, 8])
def test_device_equals_host_after_partition(ek, ctx, graphs, name, k):
    start, _ = ctx.partition_kway(graphs[name][0], k)
    part, res, log = same_as_host(ek, ctx, graphs[name], start, k, 0.03)
    rc.check_properties(ek, graphs[name], start, k, 0.03, part, res, log)
    print(f"{name} k={k}: connectivity {res['connectivity_before']} -> {res['connectivity']} in {res['rounds']} rounds, "
          f"{res['moves']} moves, parts {res['part_min']}..{res['part_max']} (max {res['max_part']})")


def test_overfull_part_and_empty_inputs(ek, ctx, graphs):
    h, nodes, ptr, pins = graphs["random"]
    start = np.zeros(nodes, np.int32)
    start[200:] = np.arange(100) % 2 + 1
    part, _, _ = same_as_host(ek, ctx, graphs["random"], start, 3, 0.05)
    assert not np.any((part == 0) & (start != 0))
    # no net of two distinct pins: nothing to do, nothing cut
    lone = ek.Hypergraph.from_pins(4, np.array([0, 1, 3], np.int64), np.array([2, 1, 1], np.int32))
    g = (lone, 4, *lone.pins())
    part, res, log = same_as_host(ek, ctx, g, np.array([0, 1, 0, 1], np.int32), 2, 0.5)
    assert part.tolist() == [0, 1, 0, 1] and res["rounds"] == 0 and res["connectivity"] == 0


def test_two_calls_agree_and_fixed_point(ek, ctx, graphs):
    h, nodes, _, _ = graphs["ibm01"]
    start = rc.starts(nodes, 8)["perm"]
    a, ra, la = ctx.kway_refine(h, start, 8, 0.05, 6)
    b, rb, lb = ctx.kway_refine(h, start, 8, 0.05, 6)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and {f: ra[f] for f in rc.INTS} == {f: rb[f] for f in rc.INTS}
    h, nodes, _, _ = graphs["fract"]
    part, res, _ = ctx.kway_refine(h, rc.starts(nodes, 4)["block"], 4, 0.05)
    again, res2, log2 = ctx.kway_refine(h, part, 4, 0.05)
    assert np.array_equal(again, part) and res2["moves"] == 0 and len(log2) == 0


def _gkl2(*args, cwd):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def test_cli_refine(ek, ctx, graphs, tmp_path):
    fract = circuit_path("fract")
    h = graphs["fract"][0]
    start, kres = ctx.partition_kway(h, 4)
    part, res, _ = ctx.kway_refine(h, start, 4, 0.05)
    r = _gkl2(fract, "-EIG", "--k", "4", "--refine", "0.05", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "fract.hgr.part.4").read_text()
    assert [int(x) for x in text.split()] == part.tolist()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("refine:")]
    assert len(line) == 1
    assert f"connectivity {res['connectivity_before']} -> {res['connectivity']}," in line[0]
    assert f"{res['rounds']} rounds, {res['moves']} moves" in line[0]
    assert f"part sizes {res['part_min']}..{res['part_max']}" in line[0]
    kline = [ln for ln in r.stdout.splitlines() if ln.startswith("k-way:")]
    assert len(kline) == 1 and f"connectivity {kres['connectivity']}," in kline[0]
    # --refine-rounds 1: the first round only
    one, _, _ = ctx.kway_refine(h, start, 4, 0.05, 1)
    r = _gkl2(fract, "-EIG", "--k", "4", "--refine", "0.05", "--refine-rounds", "1", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in (tmp_path / "results" / "fract.hgr.part.4").read_text().split()] == one.tolist()
    # usage errors: before the GPU is touched
    for args in ((fract, "-EIG", "--refine", "0.05"), (fract, "-EIG", "--k", "4", "--refine", "-1"),
                 (fract, "-EIG", "--k", "4", "--refine")):
        r = _gkl2(*args, cwd=tmp_path)
        assert r.returncode != 0 and ("Usage" in r.stdout or "Error" in r.stderr), args


def test_refine_leaves_no_state_behind(ek, ctx, graphs):
    h, nodes, _, _ = graphs["ibm01"]
    ctx.kway_refine(h, rc.starts(nodes, 8)["block"], 8, 0.03, 4)
    ibm01 = circuit_path("ibm01")
    res, log = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    fresh = ek.Context(0)
    try:
        res0, log0 = fresh.solve_file(ibm01, write_results=False, log_cap=8192)
    finally:
        fresh.close()
    swap_fields_equal(log, log0)
    assert res["kl"]["net_cut_best"] == res0["kl"]["net_cut_best"] and res["lambda"] == res0["lambda"]
    a, _ = ctx.partition_kway(graphs["fract"][0], 3)
    ctx.kway_refine(graphs["fract"][0], a, 3, 0.03)
    b, _ = ctx.partition_kway(graphs["fract"][0], 3)
    assert np.array_equal(a, b)


def test_multirank_context_is_refused(ek, graphs):
    h, nodes, _, _ = graphs["fract"]
    start = rc.starts(nodes, 2)["block"]
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.kway_refine(h, start, 2)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()
