"""The weighted k-way refinement on the GPU (ek_kway_refine_w) against its host
checker (ek_kway_refine_w_host): the rule is integer and every tie is broken by
ids, so the part vector, the round log and every integer of the result must be
identical, whatever order the workgroups run in."""
import os
import re
import subprocess

import numpy as np
import pytest

import refine_cases as rc
import refine_w_cases as wc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def circuits(ek):
    out = {}
    for name in ("fract", "ibm01"):
        plain = ek.Hypergraph.read(circuit_path(name))
        ptr, _ = plain.pins()
        weighted = ek.Hypergraph.read(circuit_path(name))
        weighted.set_weights(*wc.synthetic_weights(plain.nodes, len(ptr) - 1))
        out[name] = {"ones": plain, "synthetic": weighted}
    return out


def same_as_host(ek, ctx, h, start, k, eps, max_rounds=0, bounds=None):
    want, wres, wlog = ek.kway_refine_w_host(h, start, k, eps, max_rounds, bounds)
    part, res, log = ctx.kway_refine_w(h, start, k, eps, max_rounds, bounds)
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert np.array_equal(log, wlog), (log[:4].tolist(), wlog[:4].tolist())
    assert {f: res[f] for f in wc.INTS} == {f: wres[f] for f in wc.INTS}
    metrics, weights = ctx.kway_metrics_w(h, part, k)
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == metrics
    assert (res["part_w_min"], res["part_w_max"]) == (int(weights.min()), int(weights.max()))
    L = np.full(k, wc.uniform_bound(res["total_weight"], k, eps), np.int64) if bounds is None else bounds
    wc.check_properties(ek, h, start, k, L, part, res, log)
    return part, res, log


@pytest.mark.parametrize("name", list(wc.built_cases()))
def test_device_equals_host_built(ek, ctx, name):
    case = wc.built_cases()[name]
    part, res, _ = same_as_host(ek, ctx, wc.hypergraph(ek, case), case["start"], case["k"], case["eps"],
                                case["max_rounds"], case["bounds"])
    if case["moved"] is not None:
        want = case["moved"] if isinstance(case["moved"], dict) else {v: 1 for v in case["moved"]}
        assert {int(v): int(part[v]) for v in np.flatnonzero(part != case["start"])} == want


def test_device_equals_host_id_byte_3(ek, ctx):
    """Ids past 2^24: the select's descent parts the first rejected key from the last accepted one in key byte 3."""
    case = wc.id_byte3_case()
    part, _, log = same_as_host(ek, ctx, wc.hypergraph(ek, case), case["start"], 2, 0.0, 1, case["bounds"])
    assert set(np.flatnonzero(part != case["start"]).tolist()) == case["moved"] and log.tolist() == [[4, 4, 2, 14]]


@pytest.mark.parametrize("case", wc.circuit_cases(), ids=[c[0] for c in wc.circuit_cases()])
def test_device_equals_host_circuits(ek, ctx, circuits, case):
    name, g, wt, s, k, eps, max_rounds = case
    h = circuits[g][wt]
    start = rc.starts(h.nodes, k)[s]
    part, res, log = same_as_host(ek, ctx, h, start, k, eps, max_rounds)
    if name == wc.BINDING:
        assert np.any(log[:, 2] < log[:, 1])  # the bound binds: the device selects a threshold key
    if max_rounds:
        assert res["rounds"] <= max_rounds
    if wt == "ones":  # unit weights on the device: ek_kway_refine's run
        upart, ures, ulog = ctx.kway_refine(h, start, k, eps, max_rounds)
        assert np.array_equal(part, upart) and np.array_equal(log, ulog)
        assert {f: res[f] for f in wc.SHARED_WITH_UNWEIGHTED} == {f: ures[u] for f, u in wc.SHARED_WITH_UNWEIGHTED.items()}


@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("wt", ["synthetic", "ones"])
def test_device_equals_host_after_multilevel_partition(ek, ctx, circuits, name, wt):
    h = circuits[name][wt]
    for k in (3, 4, 8):
        start, mres = ctx.partition_kway_ml(h, k, 0.03)
        part, res, _ = same_as_host(ek, ctx, h, start, k, 0.03)
        assert res["connectivity_w_before"] == mres["connectivity_w"] and res["bound_max"] == mres["part_bound"]
        print(f"{name}/{wt} k={k}: connectivity_w {res['connectivity_w_before']} -> {res['connectivity_w']} in "
              f"{res['rounds']} rounds, {res['moves']} moves, part weights {res['part_w_min']}..{res['part_w_max']} "
              f"(bound {res['bound_max']}), over bound {res['parts_over_bound']}")


def test_empty_inputs(ek, ctx):
    # no net of two distinct pins: nothing to do, nothing cut
    lone = ek.Hypergraph.from_pins(4, np.array([0, 1, 3], np.int64), np.array([2, 1, 1], np.int32))
    lone.set_weights([3, 0, 2, 1], [4, 5])
    start = np.array([0, 1, 0, 1], np.int32)
    part, res, _ = same_as_host(ek, ctx, lone, start, 2, 0.5)
    assert part.tolist() == [0, 1, 0, 1] and res["rounds"] == 0 and res["connectivity_w"] == 0
    assert (res["part_w_min"], res["part_w_max"], res["total_weight"]) == (1, 5, 6)


def test_two_calls_agree_and_fixed_point(ek, ctx, circuits):
    h = circuits["ibm01"]["synthetic"]
    start = rc.starts(h.nodes, 8)["perm"]
    a, ra, la = ctx.kway_refine_w(h, start, 8, 0.05, 4)
    b, rb, lb = ctx.kway_refine_w(h, start, 8, 0.05, 4)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and {f: ra[f] for f in wc.INTS} == {f: rb[f] for f in wc.INTS}
    h = circuits["fract"]["synthetic"]
    part, res, _ = ctx.kway_refine_w(h, rc.starts(h.nodes, 4)["block"], 4, 0.05)
    again, res2, log2 = ctx.kway_refine_w(h, part, 4, 0.05)
    assert np.array_equal(again, part) and res2["moves"] == 0 and len(log2) == 0
    assert res2["connectivity_w_before"] == res2["connectivity_w"] == res["connectivity_w"]


def test_refine_w_leaves_no_state_behind(ek, ctx, circuits):
    h = circuits["ibm01"]["synthetic"]
    ibm01 = circuit_path("ibm01")
    before, log_before = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    ctx.kway_refine_w(h, rc.starts(h.nodes, 8)["block"], 8, 0.03, 4)
    after, log_after = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    swap_fields_equal(log_before, log_after)
    assert before["kl"]["net_cut_best"] == after["kl"]["net_cut_best"] and before["lambda"] == after["lambda"]


def test_multirank_context_is_refused(ek, circuits):
    h = circuits["fract"]["ones"]
    start = rc.starts(h.nodes, 2)["block"]
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.kway_refine_w(h, start, 2)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def _gkl2(*args, cwd):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def test_cli_refine_weighted(ek, ctx, tmp_path):
    fract = circuit_path("fract")
    h = ek.Hypergraph.read_weighted(fract)
    start, _ = ctx.partition_kway_ml_file(fract, 4, 0.03, write_results=False)
    part, res, _ = ctx.kway_refine_w(h, start, 4, 0.05)
    r = _gkl2(fract, "-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "0.05", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "fract.hgr.part.4").read_text()
    assert [int(x) for x in text.split()] == part.tolist()
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("k-way-ml:")]) == 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("refine-w:")]
    assert len(line) == 1
    got = [int(x) for x in re.findall(r"-?\d+", line[0].split("bound", 1)[1].rsplit(",", 1)[0])]
    assert got == [res["bound_max"], res["rounds"], res["moves"], res["connectivity_w_before"], res["connectivity_w"],
                   res["cut_nets"], res["part_w_min"], res["part_w_max"], res["parts_over_bound"]], line[0]
    # --refine-rounds 1: the first round only
    one, res1, _ = ctx.kway_refine_w(h, start, 4, 0.05, 1)
    r = _gkl2(fract, "-EIG", "--k", "4", "--kway-multilevel", "0.03", "--refine-weighted", "0.05", "--refine-rounds",
              "1", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in (tmp_path / "results" / "fract.hgr.part.4").read_text().split()] == one.tolist()
    assert f" {res1['rounds']} rounds, {res1['moves']} moves," in r.stdout and res1["rounds"] <= 1
