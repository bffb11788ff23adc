"""The contraction on the GPU (ek_hgr_contract_device) against the host's (ek_hgr_contract): the same hypergraph,
field by field and byte for byte, at every grouping width.  At hash_bits 1 and 4 almost every group of nets holds
different pin sets, so a merge that rested on the signature would show at once."""
import ctypes

import numpy as np
import pytest

import contract_cases as cc
from conftest import circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu

HASH_BITS = (64, 1, 4)


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", cc.names(error=False))
def test_device_equals_host(ek, ctx, name):
    case = cc.cases()[name]
    h = cc.hypergraph(ek, case)
    want = cc.fields(h.contract(case["cluster"], case["n_coarse"]))
    for bits in HASH_BITS:
        got = cc.fields(ctx.hgr_contract(h, case["cluster"], case["n_coarse"], hash_bits=bits))
        assert cc.same_fields(got, want) is None, bits


@pytest.mark.parametrize("name, weighted, cap", cc.CIRCUITS)
def test_device_equals_host_circuits(ek, ctx, name, weighted, cap):
    h, cluster, n_coarse = cc.circuit(ek, name, weighted, cap)
    want = cc.fields(h.contract(cluster, n_coarse))
    for bits in HASH_BITS:
        assert cc.same_fields(cc.fields(ctx.hgr_contract(h, cluster, n_coarse, hash_bits=bits)), want) is None, bits


@pytest.mark.parametrize("name", cc.names(error=True))
def test_device_refuses_what_the_host_refuses(ek, ctx, name):
    case = cc.cases()[name]
    h = cc.hypergraph(ek, case)
    for bits in HASH_BITS:
        with pytest.raises(ek.EKError) as e:
            ctx.hgr_contract(h, case["cluster"], case["n_coarse"], hash_bits=bits)
        assert e.value.code == ek.EK_EINVAL, bits
    # the context is as usable as before
    ok = cc.cases()["same3"]
    g = cc.hypergraph(ek, ok)
    assert cc.same_fields(cc.fields(ctx.hgr_contract(g, ok["cluster"])), cc.fields(g.contract(ok["cluster"]))) is None


def test_argument_and_state_errors(ek):
    case = cc.cases()["same3"]
    h = cc.hypergraph(ek, case)
    one = ek.Context(0)
    try:
        for bits in (0, 65, -1):
            with pytest.raises(ek.EKError) as e:
                one.hgr_contract(h, case["cluster"], hash_bits=bits)
            assert e.value.code == ek.EK_EINVAL
        out = ctypes.c_void_p()
        cl = np.ascontiguousarray(case["cluster"], np.int32)
        for args in ((None, cl.ctypes.data, 5, None, ctypes.byref(out)), (h._h, None, 5, None, ctypes.byref(out)),
                     (h._h, cl.ctypes.data, 5, None, None), (h._h, cl.ctypes.data, 6, None, ctypes.byref(out)),
                     (h._h, cl.ctypes.data, -1, None, ctypes.byref(out))):
            assert ek.lib.ek_hgr_contract_device(one._c, *args) == ek.EK_EINVAL
        # opts NULL: the default width
        assert ek.lib.ek_hgr_contract_device(one._c, h._h, cl.ctypes.data, 5, None, ctypes.byref(out)) == ek.EK_OK
        assert cc.same_fields(cc.fields(ek.Hypergraph(out)), cc.fields(h.contract(cl))) is None

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:  # a multi-rank context
            one.hgr_contract(h, case["cluster"])
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def test_two_runs_give_the_same_bytes(ek, ctx):
    h, cluster, n_coarse = cc.circuit(ek, "ibm01", True, 8)
    a = cc.fields(ctx.hgr_contract(h, cluster, n_coarse))
    b = cc.fields(ctx.hgr_contract(h, cluster, n_coarse))
    assert cc.same_fields(a, b) is None
    for x, y in zip(a[2:], b[2:]):
        assert x.tobytes() == y.tobytes()


def test_contract_leaves_no_state_behind(ek, ctx):
    """An ek_solve_file step before and after a contraction gives the same bits, and the contraction the same result."""
    ibm01 = circuit_path("ibm01")
    res0, log0 = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    h, cluster, n_coarse = cc.circuit(ek, "ibm01", True, 8)
    a = cc.fields(ctx.hgr_contract(h, cluster, n_coarse))
    res1, log1 = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    b = cc.fields(ctx.hgr_contract(h, cluster, n_coarse))
    swap_fields_equal(log0, log1)
    assert res0["kl"]["net_cut_best"] == res1["kl"]["net_cut_best"] and res0["lambda"] == res1["lambda"]
    assert cc.same_fields(a, b) is None
