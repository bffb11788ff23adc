"""The Jet refinement on the GPU (ek_kway_jet) against its host checker
(ek_kway_jet_host): the rule is integer and every tie is broken by ids, so the
part vector, the iteration log and every integer of the result must be
identical, whatever order the workgroups run in."""
import os
import re
import subprocess

import numpy as np
import pytest

import jet_cases as jc
import refine_w_cases as wc
from conftest import PKG_DIR, circuit_path

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


def same_as_host(ek, ctx, h, case):
    want, wres, wlog = jc.run(ek.kway_jet_host, h, case)
    part, res, log = jc.run(ctx.kway_jet, h, case)
    assert np.array_equal(log, wlog), (log[:6].tolist(), wlog[:6].tolist())
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert {f: res[f] for f in jc.INTS} == {f: wres[f] for f in jc.INTS}
    metrics, weights = ctx.kway_metrics_w(h, part, case["k"])
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == metrics
    assert (res["part_w_min"], res["part_w_max"]) == (int(weights.min()), int(weights.max()))
    jc.check_properties(ek, h, case, part, res, log)
    return part, res, log


@pytest.mark.parametrize("name", list(jc.built_cases()))
def test_device_equals_host_built(ek, ctx, name):
    case = jc.built_cases()[name]
    part, res, log = same_as_host(ek, ctx, jc.hypergraph(ek, case), case)
    jc.check_expect(case, part, res, log)


@pytest.mark.parametrize("name", list(jc.random_cases()))
def test_device_equals_host_random(ek, ctx, name):
    case = jc.random_cases()[name]
    same_as_host(ek, ctx, jc.hypergraph(ek, case), case)


def test_it_leaves_a_minimum_the_weighted_pass_cannot(ek, ctx):
    case = jc.built_cases()["escape"]
    h = jc.hypergraph(ek, case)
    stuck, sres, _ = ctx.kway_refine_w(h, case["start"], 2, bounds=case["bounds"])
    assert np.array_equal(stuck, case["start"]) and sres["moves"] == 0 and sres["connectivity_w"] == 14
    part, res, log = same_as_host(ek, ctx, h, case)
    assert res["connectivity_w"] == 0 and res["best_iter"] == 2 and log[:2].tolist() == [[2, 1, 1, 15], [1, 1, 1, 0]]


def circuit_case(h, start, k, eps=0.03, **kw):
    c = dict(k=k, start=np.ascontiguousarray(start, np.int32), eps=eps, bounds=None, max_iters=0, patience=12, neg=(1, 4))
    c.update(kw)
    return c


@pytest.mark.parametrize("name,wt,k,kw", [("fract", "synthetic", 4, dict()), ("fract", "ones", 3, dict(neg=(3, 4))),
                                           ("ibm01", "synthetic", 8, dict(max_iters=6)),
                                           ("ibm01", "ones", 256, dict(max_iters=2, eps=0.05)),
                                           ("ibm01", "synthetic", 65, dict(max_iters=3, eps=0.5, neg=(3, 4)))],
                         ids=["fract-k4", "fract-k3-3/4", "ibm01-k8", "ibm01-k256", "ibm01-k65-3/4"])
def test_device_equals_host_circuits(ek, ctx, circuits, name, wt, k, kw):
    import refine_cases as rc
    h = circuits[name][wt]
    same_as_host(ek, ctx, h, circuit_case(h, rc.starts(h.nodes, k)["perm"], k, **kw))


def test_device_equals_host_after_multilevel_partition(ek, ctx, circuits):
    h = circuits["ibm01"]["synthetic"]
    start, mres = ctx.partition_kway_ml(h, 4, 0.03)
    part, res, _ = same_as_host(ek, ctx, h, circuit_case(h, start, 4, max_iters=8))
    assert res["connectivity_w_before"] == mres["connectivity_w"] and res["bound_max"] == mres["part_bound"]
    print(f"ibm01/synthetic k=4: connectivity_w {res['connectivity_w_before']} -> {res['connectivity_w']} in "
          f"{res['iters']} iterations (best {res['best_iter']}), {res['moves']} moves")


def test_empty_inputs_and_two_calls_agree(ek, ctx, circuits):
    lone = ek.Hypergraph.from_pins(4, np.array([0, 1, 3], np.int64), np.array([2, 1, 1], np.int32))
    lone.set_weights([3, 0, 2, 1], [4, 5])
    part, res, log = ctx.kway_jet(lone, [0, 1, 0, 1], 2, 0.5)
    want, wres, _ = ek.kway_jet_host(lone, [0, 1, 0, 1], 2, 0.5)
    assert part.tolist() == want.tolist() == [0, 1, 0, 1] and res["iters"] == 0 and len(log) == 0
    assert {f: res[f] for f in jc.INTS} == {f: wres[f] for f in jc.INTS}
    case = jc.built_cases()["stop-rollback"]
    h = jc.hypergraph(ek, case)
    a, ra, la = jc.run(ctx.kway_jet, h, case)
    b, rb, lb = jc.run(ctx.kway_jet, h, case)
    assert np.array_equal(a, b) and np.array_equal(la, lb) and {f: ra[f] for f in jc.INTS} == {f: rb[f] for f in jc.INTS}


def test_bad_options_and_multirank_context_are_refused(ek, ctx):
    case = jc.built_cases()["escape"]
    h = jc.hypergraph(ek, case)
    for kw in (dict(neg=(-1, 4)), dict(neg=(1, 0)), dict(patience=0)):
        with pytest.raises(ek.EKError) as e:
            ctx.kway_jet(h, case["start"], 2, **kw)
        assert e.value.code == ek.EK_EINVAL, kw
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.kway_jet(h, case["start"], 2)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def test_cli_refine_jet(ek, ctx, tmp_path):
    ibm01 = circuit_path("ibm01")
    h = ek.Hypergraph.read_weighted(ibm01)
    start, _ = ctx.partition_kway_ml_file(ibm01, 4, 0.03, write_results=False)
    part, res, _ = ctx.kway_jet(h, start, 4, 0.05, max_iters=6)
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), ibm01, "-EIG", "--k", "4", "--kway-multilevel",
                        "0.03", "--refine-jet", "0.05", "--jet-iters", "6"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "ibm01.hgr.part.4").read_text()
    assert [int(x) for x in text.split()] == part.tolist()
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("k-way-ml:")]) == 1
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("refine-jet:")]
    assert len(line) == 1
    got = [int(x) for x in re.findall(r"-?\d+", line[0].split("bound", 1)[1].rsplit(",", 1)[0])]
    assert got == [res["bound_max"], res["iters"], res["best_iter"], res["moves"], res["connectivity_w_before"],
                   res["connectivity_w"], res["cut_nets"], res["part_w_min"], res["part_w_max"],
                   res["parts_over_bound"]], line[0]
