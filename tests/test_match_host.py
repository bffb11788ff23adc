"""The coarsening's host pieces, no GPU: ek_match_host (the checker of the
device matching) against the rule restated in match_cases and against the
properties the rule promises, and ek_hgr_contract against
ek_bipart_metrics_host: a coarse side vector must cut and weigh on the coarse
hypergraph exactly what its projection cuts and weighs on the fine one."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
from conftest import REPO

SMALL = [n for n in mc.names() if mc.cases()[n][0] <= 400]


def run(ek, name, max_rounds):
    h, cap, max_net = mc.hypergraph(ek, name)
    return ek.match_host(h, cap, max_net, max_rounds)


@pytest.mark.parametrize("name", mc.names())
def test_recorded_integers(ek, name):
    for max_rounds in mc.ROUNDS:
        mate, _, log, res = run(ek, name, max_rounds)
        assert mc.ints(res) + (mc.mate_sum(mate),) == mc.EXPECTED[name][max_rounds], max_rounds
        assert len(log) == res["rounds"] and int(log[:, 1].sum()) == res["pairs"] == res["n"] - res["n_coarse"]


@pytest.mark.parametrize("name, weighted, cap", mc.CIRCUITS)
def test_recorded_integers_circuits(ek, name, weighted, cap):
    h = mc.circuit(ek, name, weighted)
    for max_rounds in mc.ROUNDS:
        mate, cluster, log, res = ek.match_host(h, cap, 64, max_rounds)
        assert mc.ints(res) + (mc.mate_sum(mate),) == mc.EXPECTED[name + ("-w" if weighted else "")][max_rounds]
        check_properties(h, mate, cluster, cap, 64)


@pytest.mark.parametrize("name", sorted(mc.HAND))
def test_hand_worked(ek, name):
    mate, cluster, log, res = run(ek, name, 0)
    want_mate, want_cluster, want_log = mc.HAND[name]
    assert mate.tolist() == want_mate and cluster.tolist() == want_cluster
    assert [tuple(r) for r in log.tolist()] == want_log
    assert res["rounds"] == len(want_log) and res["n_coarse"] == max(want_cluster) + 1


def test_one_pair_a_round_on_the_rising_path(ek):
    """max_rounds stops the run where the log says: after one round only the pair of the greatest score exists."""
    mate, _, log, res = run(ek, "path_rising", 1)
    assert mate.tolist() == [-1, -1, -1, -1, 5, 4] and log.tolist() == [[6, 1]] and res["rounds"] == 1
    mate, _, log, _ = run(ek, "path_rising", 2)
    assert mate.tolist() == [-1, -1, 3, 2, 5, 4] and log.tolist() == [[6, 1], [4, 1]]


@pytest.mark.parametrize("name", SMALL)
def test_equals_the_rule_in_python(ek, name):
    for max_rounds in mc.ROUNDS:
        mate, cluster, log, _ = run(ek, name, max_rounds)
        want = mc.reference(name, max_rounds)
        assert np.array_equal(mate, want[0]) and np.array_equal(cluster, want[1]) and np.array_equal(log, want[2])


def eligible_pin_sets(h, max_net):
    ptr, pins = h.pins()
    sets = [set(pins[ptr[e]:ptr[e + 1]].tolist()) for e in range(len(ptr) - 1)]
    return [s for s in sets if 2 <= len(s) <= max(max_net, 2)]


def check_properties(h, mate, cluster, cap, max_net, maximal=False):
    n = h.nodes
    node_w = h.weights()[0]
    w = np.ones(n, np.int64) if node_w is None else node_w.astype(np.int64)
    matched = np.flatnonzero(mate >= 0)
    assert np.array_equal(mate[mate[matched]], matched)  # an involution
    assert not np.any(mate == np.arange(n))
    assert np.all(w[matched] + w[mate[matched]] <= cap)
    sets = eligible_pin_sets(h, max_net)
    shared = set()
    for s in sets:
        for u in s:
            if mate[u] in s:
                shared.add(u)
    assert shared == set(matched.tolist())  # every pair shares an eligible net
    leader = np.where(mate >= 0, np.minimum(mate, np.arange(n)), np.arange(n))
    leaders = np.unique(leader)
    assert np.array_equal(cluster, np.searchsorted(leaders, leader))  # the rank of the leader among the leaders
    if maximal:  # brute force: no eligible net holds two unmatched nodes that fit together
        for s in sets:
            free = sorted(u for u in s if mate[u] < 0)
            assert not any(w[a] + w[b] <= cap for i, a in enumerate(free) for b in free[i + 1:]), s


@pytest.mark.parametrize("name", SMALL)
def test_properties(ek, name):
    h, cap, max_net = mc.hypergraph(ek, name)
    for max_rounds in mc.ROUNDS:
        mate, cluster, _, _ = ek.match_host(h, cap, max_net, max_rounds)
        check_properties(h, mate, cluster, cap, max_net, maximal=max_rounds == 0)


def test_argument_errors(ek):
    h, _, _ = mc.hypergraph(ek, "path_end_ids")
    for cap in (0, -3):
        with pytest.raises(ek.EKError) as e:
            ek.match_host(h, cap)
        assert e.value.code == ek.EK_EINVAL
    # the weight range of ek_fm_refine_w: the nets on one node weigh at most 2^31 - 1
    h.set_weights(None, [mc.INT32_MAX, 1])
    with pytest.raises(ek.EKError) as e:
        ek.match_host(h, 2)
    assert e.value.code == ek.EK_EINVAL
    # max_net below 2 acts as 2
    h, _, _ = mc.hypergraph(ek, "path_rising")
    a, b = ek.match_host(h, 2, 0, 0), ek.match_host(h, 2, 2, 0)
    assert np.array_equal(a[0], b[0]) and a[3]["eligible_nets"] == b[3]["eligible_nets"] == 5


# ---------------------------------------------------------------------------
# ek_hgr_contract
CONTRACT = ["repeated_pin", "net9", "n257", "all_pins_net", "dense", "star33", "no_nets"]


def contracted(ek, name):
    h, cap, max_net = mc.hypergraph(ek, name)
    _, cluster, _, res = ek.match_host(h, cap, max_net, 0)
    return h, cluster, res["n_coarse"], h.contract(cluster, res["n_coarse"])


@pytest.mark.parametrize("name", CONTRACT)
def test_contract_preserves_cut_and_weights(ek, name):
    h, cluster, nc, coarse = contracted(ek, name)
    assert coarse.nodes == nc
    node_w, net_w = coarse.weights()
    fine_w = h.weights()[0]
    assert int(node_w.sum()) == (h.nodes if fine_w is None else int(fine_w.sum()))
    assert np.array_equal(node_w, np.bincount(cluster, None if fine_w is None else fine_w, nc).astype(np.int32))
    assert coarse.nets == 0 or net_w is not None
    ptr, pins = coarse.pins()
    sets = [tuple(sorted(pins[ptr[e]:ptr[e + 1]].tolist())) for e in range(coarse.nets)]
    assert all(len(s) >= 2 and len(set(s)) == len(s) for s in sets) and len(set(sets)) == len(sets)
    rng = np.random.default_rng(11)
    for _ in range(20):
        side = rng.integers(0, 2, nc).astype(np.uint8)
        a, b = ek.bipart_metrics_host(coarse, side), ek.bipart_metrics_host(h, side[cluster])
        assert (a[0], a[2], a[3]) == (b[0], b[2], b[3])
        assert a[1] <= b[1]  # merged nets count once


def test_contract_two_levels_of_a_circuit(ek):
    h = mc.circuit(ek, "ibm01", True)
    rng = np.random.default_rng(12)
    for _ in range(2):
        _, cluster, _, res = ek.match_host(h, 16, 64, 8)
        coarse = h.contract(cluster, res["n_coarse"])
        for _ in range(20):
            side = rng.integers(0, 2, coarse.nodes).astype(np.uint8)
            a, b = ek.bipart_metrics_host(coarse, side), ek.bipart_metrics_host(h, side[cluster])
            assert (a[0], a[2], a[3]) == (b[0], b[2], b[3])
        h = coarse


def test_contract_merges_parallel_nets_in_first_occurrence_order(ek):
    # clusters {0, 1} -> 0, {2} -> 1, {3} -> 2, {4} -> 3
    ptr, pins = mc.pack([[2, 0, 3], [0, 1], [3, 1, 2], [4, 3], [1, 1, 4], [3, 4, 4]])
    h = ek.Hypergraph.from_pins(5, ptr, pins)
    h.set_weights([1, 2, 3, 4, 5], [7, 1, 2, 3, 4, 5])
    c = h.contract([0, 0, 1, 2, 3])
    cptr, cpins = c.pins()
    # [2,0,3] -> (1,0,2) kept; [0,1] -> one pin, dropped; [3,1,2] -> (2,0,1): the first net's set, merged; [4,3] ->
    # (3,2) kept; [1,1,4] -> (0,3) kept; [3,4,4] -> (2,3): the set of (3,2), merged
    assert cptr.tolist() == [0, 3, 5, 7] and cpins.tolist() == [1, 0, 2, 3, 2, 0, 3]
    node_w, net_w = c.weights()
    assert node_w.tolist() == [3, 3, 4, 5] and net_w.tolist() == [7 + 2, 3 + 5, 4]


def test_contract_identity_returns_the_same_pins(ek):
    rng = np.random.default_rng(13)
    nets = {tuple(sorted(x)): x for x in mc.random_nets(rng, 60, 150, 2, 6)}  # no parallel, no single-pin nets
    ptr, pins = mc.pack(list(nets.values()))
    h = ek.Hypergraph.from_pins(60, ptr, pins)
    c = h.contract(np.arange(60))
    cptr, cpins = c.pins()
    assert np.array_equal(cptr, ptr) and np.array_equal(cpins, pins)
    node_w, net_w = c.weights()
    assert node_w.tolist() == [1] * 60 and net_w.tolist() == [1] * len(nets)


def test_contract_argument_errors(ek):
    ptr, pins = mc.pack([[0, 1], [1, 2]])
    h = ek.Hypergraph.from_pins(3, ptr, pins)
    for cluster, nc in (([0, 1, 2], 2), ([0, -1, 1], 2), ([0, 0, 2], 3), ([0, 0, 0], 4)):
        with pytest.raises(ek.EKError) as e:  # out of range (twice), an unhit id, more clusters than nodes
            h.contract(cluster, nc)
        assert e.value.code == ek.EK_EINVAL, cluster
    h.set_weights([mc.INT32_MAX, 1, 1], None)
    with pytest.raises(ek.EKError) as e:  # a summed node weight above INT32_MAX
        h.contract([0, 0, 1], 2)
    assert e.value.code == ek.EK_EINVAL
    ptr, pins = mc.pack([[0, 1], [1, 0]])
    h = ek.Hypergraph.from_pins(2, ptr, pins)
    h.set_weights(None, [mc.INT32_MAX, 1])
    with pytest.raises(ek.EKError) as e:  # a merged net weight above INT32_MAX
        h.contract([0, 1], 2)
    assert e.value.code == ek.EK_EINVAL


# ---------------------------------------------------------------------------
# the C-ABI conventions of test_capi.py, for the new symbols by themselves
NEW_SYMBOLS = ["ek_match_default_opts", "ek_match_host", "ek_match", "ek_hgr_contract", "ek_ml_default_opts",
               "ek_multilevel_bipartition", "ek_multilevel_bipartition_file"]


def test_new_symbols_are_declared_and_exported(ek):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "eigkl.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ek_[a-z0-9_]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(ek.lib, s), s
    assert re.search(r"#define EIGKL_ABI_VERSION 4\b", text)  # new structs only: no existing layout moved


def test_new_struct_layouts_match_python_mirror(ek, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "eigkl.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %d\\n", sizeof(ek_match_opts), sizeof(ek_match_result), sizeof(ek_ml_opts),'
        " sizeof(ek_ml_result), EK_ML_LEVELS);\n"
        '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(ek_match_opts, max_cluster), offsetof(ek_match_result, eligible_nets),'
        " offsetof(ek_ml_opts, match), offsetof(ek_ml_opts, lanczos), offsetof(ek_ml_result, fm_moves),"
        " offsetof(ek_ml_result, t_match));\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    a, b = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(x) for x in a.split()] == [ctypes.sizeof(ek.MatchOpts), ctypes.sizeof(ek.MatchResult),
                                           ctypes.sizeof(ek.MlOpts), ctypes.sizeof(ek.MlResult), ek.ML_LEVELS]
    assert [int(x) for x in b.split()] == [ek.MatchOpts.max_cluster.offset, ek.MatchResult.eligible_nets.offset,
                                           ek.MlOpts.match.offset, ek.MlOpts.lanczos.offset,
                                           ek.MlResult.fm_moves.offset, ek.MlResult.t_match.offset]


def test_default_opts(ek):
    m = ek.MatchOpts()
    ek.lib.ek_match_default_opts(ctypes.byref(m))
    assert (m.max_net, m.max_rounds, m.max_cluster) == (64, 8, 2)
    o = ek.MlOpts()
    ek.lib.ek_ml_default_opts(ctypes.byref(o))
    assert (o.imbalance, o.coarse_nodes, o.max_levels) == (0.03, 512, 32)
    assert (o.match.max_net, o.match.max_rounds, o.match.max_cluster) == (64, 8, 0)
    f, z = ek.FmOpts(), ek.LanczosOpts()
    ek.lib.ek_fm_default_opts(ctypes.byref(f))
    ek.lib.ek_lanczos_default_opts(ctypes.byref(z))
    assert bytes(o.fm) == bytes(f) and bytes(o.lanczos) == bytes(z)


def test_multilevel_cli_misuse_prints_usage(tmp_path):
    """Refused while the arguments are read: no GPU work."""
    from conftest import PKG_DIR, circuit_path
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    for args in (("--multilevel", "0.03"), ("-EIG", "--ml-coarse", "64"), ("-EIG", "--multilevel", "0.03", "--k", "4"),
                 ("-EIG", "--multilevel", "0.03", "--sweep", "0.03"), ("-EIG", "--multilevel", "0.03", "--fm", "0.03"),
                 ("-EIG", "--multilevel", "-1")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--multilevel" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.2").exists()
