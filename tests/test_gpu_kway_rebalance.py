"""The k-way rebalancing on the GPU (ek_kway_rebalance) against its host checker
(ek_kway_rebalance_host): the rule is integer and every tie is broken by ids, so
the part vector, the round log and every integer of the result must be
identical, whatever order the workgroups run in."""
import os
import re
import subprocess

import numpy as np
import pytest

import rebalance_cases as bc
import refine_w_cases as wc
from conftest import PKG_DIR, circuit_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def same_as_host(ek, ctx, h, case, name=None):
    want, wres, wlog = bc.run(ek.kway_rebalance_host, h, case)
    part, res, log = bc.run(ctx.kway_rebalance, h, case)
    assert np.array_equal(log, wlog), (log[:6].tolist(), wlog[:6].tolist())
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert {f: res[f] for f in bc.INTS} == {f: wres[f] for f in bc.INTS}
    metrics, weights = ctx.kway_metrics_w(h, part, case["k"])
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == metrics
    assert (res["part_w_min"], res["part_w_max"]) == (int(weights.min()), int(weights.max()))
    if name is not None:
        ref = bc.reference(name, case)
        assert np.array_equal(part, ref[0]) and np.array_equal(log, ref[1])
        bc.check_properties(ek, h, case, ref, part, res, log)
    return part, res, log


@pytest.mark.parametrize("name", list(bc.built_cases()))
def test_device_equals_host_built(ek, ctx, name):
    case = bc.built_cases()[name]
    part, res, log = same_as_host(ek, ctx, bc.hypergraph(ek, case), case, name)
    bc.check_expect(case, part, res, log)


@pytest.mark.parametrize("name", list(bc.random_cases()))
def test_device_equals_host_random(ek, ctx, name):
    case = bc.random_cases()[name]
    same_as_host(ek, ctx, bc.hypergraph(ek, case), case, name)


def circuit_case(start, k, eps, **kw):
    c = dict(k=k, start=np.ascontiguousarray(start, np.int32), eps=eps, bounds=None, max_rounds=0)
    c.update(kw)
    return c


@pytest.mark.parametrize("name,weighted,k", [("fract", True, 4), ("ibm01", False, 8), ("ibm01", True, 65)],
                         ids=["fract-k4", "ibm01-k8", "ibm01-k65"])
def test_device_equals_host_circuits(ek, ctx, name, weighted, k):
    """A block start with a tenth of part 0's nodes handed to part 1, under the uniform bound at 0.01."""
    h = ek.Hypergraph.read(circuit_path(name))
    if weighted:
        h.set_weights(*wc.synthetic_weights(h.nodes, h.nets))
    start = (np.arange(h.nodes, dtype=np.int64) * k // h.nodes).astype(np.int32)
    mine = np.flatnonzero(start == 0)
    start[mine[:max(1, len(mine) // 10)]] = 1
    part, res, log = same_as_host(ek, ctx, h, circuit_case(start, k, 0.01))
    assert res["parts_over_before"] >= 1 and res["rounds"] >= 1 and res["excess"] < res["excess_before"]


def test_two_runs_agree_and_the_context_is_left_as_it_was(ek, ctx):
    case = bc.built_cases()["gain-k65-edge"]
    h = bc.hypergraph(ek, case)
    dims = ctx.spmv_dims()
    a, ra, la = bc.run(ctx.kway_rebalance, h, case)
    b, rb, lb = bc.run(ctx.kway_rebalance, h, case)
    assert np.array_equal(a, b) and np.array_equal(la, lb)
    assert {f: ra[f] for f in bc.INTS} == {f: rb[f] for f in bc.INTS}
    assert ctx.spmv_dims() == dims  # no SpMV, no graph, no partition appeared on the context
    fresh = ek.Context(0)
    try:
        c, rc_, lc = bc.run(fresh.kway_rebalance, h, case)
        assert np.array_equal(a, c) and np.array_equal(la, lc) and fresh.spmv_dims() == dims
    finally:
        fresh.close()


def test_bad_options_and_multirank_context_are_refused(ek, ctx):
    case = bc.built_cases()["accept-two-sources"]
    h = bc.hypergraph(ek, case)
    for kw in (dict(k=1), dict(k=257), dict(eps=-0.5), dict(eps=float("nan")), dict(bounds=[1, 1, -1, 10])):
        args = dict(k=4, eps=0.03, bounds=None)
        args.update(kw)
        with pytest.raises(ek.EKError) as e:
            ctx.kway_rebalance(h, case["start"], args["k"], args["eps"], args["bounds"])
        assert e.value.code == ek.EK_EINVAL, kw
    bad = case["start"].copy()
    bad[0] = 4
    with pytest.raises(ek.EKError) as e:
        ctx.kway_rebalance(h, bad, 4)
    assert e.value.code == ek.EK_EINVAL
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.kway_rebalance(h, case["start"], 4, bounds=case["bounds"])
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


@pytest.mark.parametrize("name", ["unit-weights", "gain-k129-edge"])
def test_jet_from_a_rebalanced_start_ends_in_bound(ek, ctx, name):
    """Jet alone never lets an overweight part give up weight on purpose: from the raw start a part stays over."""
    case = bc.built_cases()[name]
    h = bc.hypergraph(ek, case)
    _, raw, _ = ctx.kway_jet(h, case["start"], case["k"], case["eps"], case["bounds"])
    assert raw["parts_over_bound"] > 0
    start, res, _ = bc.run(ctx.kway_rebalance, h, case)
    assert res["parts_over_bound"] == 0
    _, jr, _ = ctx.kway_jet(h, start, case["k"], case["eps"], case["bounds"])
    assert jr["parts_over_bound"] == 0 and jr["connectivity_w"] <= res["connectivity_w"]


def test_cli_rebalance_to(ek, ctx, tmp_path):
    ibm01 = circuit_path("ibm01")
    h = ek.Hypergraph.read_weighted(ibm01)
    start, _ = ctx.partition_kway_ml_file(ibm01, 4, 0.03, write_results=False)
    part, res, _ = ctx.kway_rebalance(h, start, 4, 0.0)
    final, jres, _ = ctx.kway_jet(h, part, 4, 0.0, max_iters=6)
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), ibm01, "-EIG", "--k", "4", "--kway-multilevel",
                        "0.03", "--rebalance-to", "0", "--refine-jet", "0", "--jet-iters", "6"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "ibm01.hgr.part.4").read_text()
    assert [int(x) for x in text.split()] == final.tolist()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("rebalance:")]
    assert len(line) == 1 and len([ln for ln in r.stdout.splitlines() if ln.startswith("refine-jet:")]) == 1
    got = [int(x) for x in re.findall(r"-?\d+", line[0].split("bound", 1)[1].rsplit(",", 1)[0])]
    assert got == [res["bound_max"], int(res["parts_over_before"] > 0), res["rounds"], res["moves"],
                   res["excess_before"], res["excess"], res["parts_over_before"], res["parts_over_bound"],
                   res["connectivity_w_before"], res["connectivity_w"]], line[0]
