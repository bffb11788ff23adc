"""The contraction's shared cases (contract_cases.py) against the host code: Hypergraph.contract (ek_hgr_contract) must
give what the plain-Python restatement of the five-step rule gives, field by field, and refuse what it refuses.  So
the cases the GPU test holds the device contraction to are themselves held to the rule.  No GPU."""
import numpy as np
import pytest

import contract_cases as cc


def ref_fields(case):
    node_w, net_ptr, pins, net_w = cc.contract_ref(case["nodes"], case["net_ptr"], case["pins"], case["node_w"],
                                                   case["net_w"], case["cluster"], case["n_coarse"])
    return case["n_coarse"], len(net_w), net_ptr, pins, node_w, net_w


@pytest.mark.parametrize("name", cc.names(error=False))
def test_host_equals_rule(ek, name):
    case = cc.cases()[name]
    got = cc.hypergraph(ek, case).contract(case["cluster"], case["n_coarse"])
    assert cc.same_fields(cc.fields(got), ref_fields(case)) is None


@pytest.mark.parametrize("name", cc.names(error=True))
def test_host_refuses_what_the_rule_refuses(ek, name):
    case = cc.cases()[name]
    with pytest.raises(ValueError):
        ref_fields(case)
    with pytest.raises(ek.EKError) as e:
        cc.hypergraph(ek, case).contract(case["cluster"], case["n_coarse"])
    assert e.value.code == ek.EK_EINVAL


@pytest.mark.parametrize("name, weighted, cap", cc.CIRCUITS)
def test_host_equals_rule_circuits(ek, name, weighted, cap):
    h, cluster, n_coarse = cc.circuit(ek, name, weighted, cap)
    net_ptr, pins = h.pins()
    node_w, net_w = h.weights()
    case = dict(nodes=h.nodes, net_ptr=net_ptr, pins=pins, node_w=node_w, net_w=net_w, cluster=cluster,
                n_coarse=n_coarse)
    assert cc.same_fields(cc.fields(h.contract(cluster, n_coarse)), ref_fields(case)) is None


def test_the_cases_cover_what_they_claim():
    c = cc.cases()
    assert sum(k.startswith("rand") for k in c) == 30
    assert {c[f"n{n}"]["nodes"] for n in (1, 2, 63, 64, 65, 257)} == {1, 2, 63, 64, 65, 257}
    assert [len(c[f"nets{m}"]["net_ptr"]) - 1 for m in (0, 1, 255, 256, 257)] == [0, 1, 255, 256, 257]
    for size in (2, 63, 64, 65, 300):
        case = c[f"size{size}"]
        assert int(np.diff(case["net_ptr"])[2]) == size
    one = ref_fields(c["one_cluster"])
    assert one[0] == 1 and one[1] == 0 and len(one[3]) == 0
    assert np.array_equal(c["identity"]["cluster"], np.arange(50))
    same40 = ref_fields(c["same40"])
    assert same40[1] == 2 and list(same40[5]) == [1 + 42, sum(range(2, 42))]  # merged into the first, c summed
    assert list(same40[3][2:]) == list(c["same40"]["pins"][2:7])              # with the first one's pin order
    assert ref_fields(c["eq_sum"])[1] == 4 and ref_fields(c["eq_xor"])[1] == 2 and ref_fields(c["superset"])[1] == 3
    assert list(ref_fields(c["netw_max"])[5]) == [2 ** 31 - 1, 1]
    assert list(ref_fields(c["nodew_max"])[4]) == [2 ** 31 - 1, 7]
    assert ref_fields(c["inside_one"])[1] == 1 and list(ref_fields(c["left_two"])[3]) == [0, 1]
