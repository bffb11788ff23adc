"""The matching on the GPU (ek_match) against its host checker (ek_match_host):
the rule is integer and every tie is broken by ids, so mate, cluster, the
round log and every integer of the result must be identical, whatever order
the workgroups run in."""
import numpy as np
import pytest

import match_cases as mc
from conftest import circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def same_as_host(ek, ctx, h, cap, max_net, max_rounds):
    want = ek.match_host(h, cap, max_net, max_rounds)
    got = ctx.match(h, cap, max_net, max_rounds)
    for a, b, what in zip(got[:3], want[:3], ("mate", "cluster", "round log")):
        assert np.array_equal(a, b), (what, max_rounds, int(np.count_nonzero(a != b)) if a.shape == b.shape else a.shape)
    assert mc.ints(got[3]) == mc.ints(want[3]), max_rounds
    return got


@pytest.mark.parametrize("name", mc.names())
def test_device_equals_host(ek, ctx, name):
    """Among the cases: nets of 8 | 9 and 64 | 65 pins (max_net's edge), 255 | 256 | 257 nodes and one wave less or
    more than a workgroup (192, 320), a hub of 32 | 33 entries (star32, star33: the thread / wave hand-over), every
    node its wave's (dense), a score of 51 bits (score_high_bits), no nets at all."""
    h, cap, max_net = mc.hypergraph(ek, name)
    for max_rounds in mc.ROUNDS:
        mate, _, _, res = same_as_host(ek, ctx, h, cap, max_net, max_rounds)
        assert mc.ints(res) + (mc.mate_sum(mate),) == mc.EXPECTED[name][max_rounds]


@pytest.mark.parametrize("name, weighted, cap", mc.CIRCUITS)
def test_device_equals_host_circuits(ek, ctx, name, weighted, cap):
    h = mc.circuit(ek, name, weighted)
    for max_rounds in mc.ROUNDS:
        mate, _, _, res = same_as_host(ek, ctx, h, cap, 64, max_rounds)
        assert mc.ints(res) + (mc.mate_sum(mate),) == mc.EXPECTED[name + ("-w" if weighted else "")][max_rounds]


def test_short_round_log_and_null_outputs(ek, ctx):
    """A log shorter than the run keeps its first rows; the result still counts every round."""
    import ctypes
    h, cap, max_net = mc.hypergraph(ek, "dense")
    full = ctx.match(h, cap, max_net, 0)
    o = ek.MatchOpts(max_net, 0, cap)
    log = np.full((2, 2), -7, np.int64)
    r = ek.MatchResult()
    rc = ek.lib.ek_match(ctx._c, h._h, ctypes.byref(o), None, None, log.ctypes.data, 2, ctypes.byref(r))
    assert rc == ek.EK_OK and r.rounds == full[3]["rounds"] > 2 and np.array_equal(log, full[2][:2])


def test_match_leaves_no_state_behind(ek, ctx):
    """An ek_solve_file step before and after a match gives the same bits, and the match the same result."""
    ibm01 = circuit_path("ibm01")
    res0, log0 = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    h = mc.circuit(ek, "ibm01", True)
    a = ctx.match(h, 8)
    res1, log1 = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    b = ctx.match(h, 8)
    swap_fields_equal(log0, log1)
    assert res0["kl"]["net_cut_best"] == res1["kl"]["net_cut_best"] and res0["lambda"] == res1["lambda"]
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and mc.ints(a[3]) == mc.ints(b[3])


def test_state_and_argument_errors(ek):
    h, cap, max_net = mc.hypergraph(ek, "path_rising")
    one = ek.Context(0)
    try:
        with pytest.raises(ek.EKError) as e:
            one.match(h, 0)
        assert e.value.code == ek.EK_EINVAL
        assert one.match(h, cap)[3]["pairs"] == 3

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:  # a multi-rank context
            one.match(h, cap)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()
