"""The multi-node clustering of the coarsening without a GPU: ek_cluster_host (the checker of the device clustering)
against the rule restated in cluster_cases, against the hand-worked integers, and against what the rule promises
(DESIGN.md §20); the contraction along its cluster map against ek_bipart_metrics_host; the new struct, the defaults,
the EK_EINVAL cases and the CLI's refusals of --coarsen."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_cases as cc
import match_cases as mc
from conftest import PKG_DIR, REPO, circuit_path

GKL2 = os.path.join(PKG_DIR, "build", "bin", "gKL2")


def run(ek, name, max_rounds):
    h, cap, max_net = cc.hypergraph(ek, name)
    return ek.cluster_host(h, cap, max_net, max_rounds)


def same_as_rule(got, want, what):
    rep, cluster, log, res = got
    assert np.array_equal(rep, want[0]), what
    assert np.array_equal(cluster, want[1]), what
    assert np.array_equal(log, want[2]), what
    assert cc.ints(res) == want[3], what


@pytest.mark.parametrize("name", cc.names())
def test_equals_the_rule_in_python(ek, name):
    for max_rounds in cc.ROUNDS:
        same_as_rule(run(ek, name, max_rounds), cc.reference(name)[max_rounds], max_rounds)


@pytest.mark.parametrize("name, weighted, cap", cc.CIRCUITS)
def test_equals_the_rule_in_python_circuits(ek, name, weighted, cap):
    h = mc.circuit(ek, name, weighted)
    want = cc.circuit_reference(ek, name, weighted, cap)
    for max_rounds in cc.ROUNDS:
        got = ek.cluster_host(h, cap, 64, max_rounds)
        same_as_rule(got, want[max_rounds], max_rounds)
        check_promises(h, got, cap, 64, maximal=max_rounds == 0)


def test_ibm01_cross_check(ek):
    """The figures the rule was specified with: ibm01, unit weights, cap 95, 8 rounds at most: 12,752 -> 4,256 nodes in
    3 rounds, from the Python restatement and from the checker alike."""
    want = cc.circuit_reference(ek, "ibm01", False, 95)[8]
    assert want[3][:4] == (12752, 4256, 12752 - 4256, 3)
    _, _, log, res = ek.cluster_host(mc.circuit(ek, "ibm01", False), 95, 64, 8)
    assert (res["n_coarse"], res["rounds"], res["joins"]) == (4256, 3, 8496) and res["heaviest"] <= 95
    assert log[:, 2].tolist() == want[2][:, 2].tolist()


@pytest.mark.parametrize("name", sorted(cc.HAND))
def test_hand_worked(ek, name):
    rep, cluster, log, res = run(ek, name, 0)
    want_rep, want_cluster, want_log, heaviest = cc.HAND[name]
    assert rep.tolist() == want_rep and cluster.tolist() == want_cluster
    assert [tuple(r) for r in log.tolist()] == want_log
    assert res["rounds"] == len(want_log) and res["n_coarse"] == max(want_cluster) + 1
    assert res["joins"] == sum(r[2] for r in want_log) and res["heaviest"] == heaviest


def test_max_rounds_stops_where_the_log_says(ek):
    """After one round of the star whose hub is the greatest id only the mutual pair has merged: the leaves waited."""
    rep, cluster, log, res = run(ek, "star_hub_greatest", 1)
    assert rep.tolist() == [0, 1, 2, 3, 0] and cluster.tolist() == [0, 1, 2, 3, 0]
    assert log.tolist() == [[5, 1, 1]] and (res["rounds"], res["n_coarse"], res["heaviest"]) == (1, 4, 2)


def eligible_pin_sets(h, max_net):
    ptr, pins = h.pins()
    sets = [set(pins[ptr[e]:ptr[e + 1]].tolist()) for e in range(len(ptr) - 1)]
    return [s for s in sets if 2 <= len(s) <= max(max_net, 2)]


def check_promises(h, got, cap, max_net, maximal=False):
    rep, cluster, log, res = got
    n = h.nodes
    node_w = h.weights()[0]
    w = np.ones(n, np.int64) if node_w is None else node_w.astype(np.int64)
    ids = np.arange(n)
    assert np.array_equal(rep[rep], rep)  # every rep is a root
    S = np.bincount(rep, w, n).astype(np.int64)
    size = np.bincount(rep, None, n)
    assert np.all(S[size > 1] <= cap)  # every cluster of more than one node weighs at most the cap
    assert res["heaviest"] == (int(S[rep == ids].max()) if n else 0)
    roots = np.flatnonzero(rep == ids)
    assert np.array_equal(cluster, np.searchsorted(roots, rep)) and res["n_coarse"] == len(roots)
    assert res["joins"] == n - len(roots) == int(log[:, 2].sum()) and len(log) == res["rounds"]
    # a counted round joined; a round with a proposer joins; movers are proposers, joins are movers
    assert np.all(log[:, 2] >= 1) and np.all(log[:, 0] >= log[:, 1]) and np.all(log[:, 1] >= log[:, 2])
    sets = eligible_pin_sets(h, max_net)
    linked = set()  # every joiner shares an eligible net with a member of its cluster
    for s in sets:
        by_root = {}
        for v in s:
            by_root.setdefault(int(rep[v]), []).append(v)
        for members in by_root.values():
            if len(members) > 1:
                linked.update(members)
    assert set(np.flatnonzero(rep != ids).tolist()) <= linked
    if maximal:  # brute force: no single u and pin v != u of an eligible net of u fit together
        single = (rep == ids) & (size == 1)
        for s in sets:
            for u in s:
                if single[u]:
                    assert not any(S[rep[v]] + w[u] <= cap for v in s if v != u), (u, sorted(s))


@pytest.mark.parametrize("name", cc.names())
def test_promises(ek, name):
    h, cap, max_net = cc.hypergraph(ek, name)
    for max_rounds in cc.ROUNDS:
        check_promises(h, ek.cluster_host(h, cap, max_net, max_rounds), cap, max_net, maximal=max_rounds == 0)


def test_a_round_with_a_proposer_joins():
    """The progress argument by brute force on the restatement: in the run to the end, the round after the last
    counted one has no proposer at all (it would have joined), i.e. the end state admits no proposal."""
    for name in cc.names():
        nodes, nets, node_w, net_w, cap, max_net = cc.cases()[name]
        rep, _, log, _ = cc.reference(name)[0]
        w = np.ones(nodes, np.int64) if node_w is None else node_w.astype(np.int64)
        S = np.bincount(rep, w, nodes).astype(np.int64)
        size = np.bincount(rep, None, nodes)
        for net in nets:
            pins = set(net)
            if 2 <= len(pins) <= max(max_net, 2):
                for u in pins:
                    if rep[u] == u and size[u] == 1:
                        assert all(S[rep[v]] + w[u] > cap for v in pins if v != u), (name, u)
        assert np.all(log[:, 2] >= 1) if len(log) else True


CONTRACT = ["star_hub_greatest", "cap_zero_weights", "movers65_cap", "n257", "random7", "random22", "m4:dense",
            "m4:all_pins_net", "m:no_nets"]


@pytest.mark.parametrize("name", CONTRACT)
def test_contract_along_the_clusters_preserves_cut_and_weights(ek, name):
    h, cap, max_net = cc.hypergraph(ek, name)
    _, cluster, _, res = ek.cluster_host(h, cap, max_net, 0)
    nc = res["n_coarse"]
    coarse = h.contract(cluster, nc)
    fine_w = h.weights()[0]
    node_w = coarse.weights()[0]
    assert coarse.nodes == nc and int(node_w.sum()) == (h.nodes if fine_w is None else int(fine_w.sum()))
    assert int(node_w.max()) == res["heaviest"]
    rng = np.random.default_rng(21)
    for _ in range(20):
        side = rng.integers(0, 2, nc).astype(np.uint8)
        a, b = ek.bipart_metrics_host(coarse, side), ek.bipart_metrics_host(h, side[cluster])
        assert (a[0], a[2], a[3]) == (b[0], b[2], b[3])


def test_argument_errors(ek):
    h, _, _ = cc.hypergraph(ek, "chain_waits")
    for cap in (0, -3):
        with pytest.raises(ek.EKError) as e:
            ek.cluster_host(h, cap)
        assert e.value.code == ek.EK_EINVAL
    assert ek.lib.ek_cluster_host(None, None, None, None, None, 0, None) == ek.EK_EINVAL
    # the weight range of ek_fm_refine_w: the nets on one node weigh at most 2^31 - 1
    h.set_weights(None, [cc.INT32_MAX, 1])
    with pytest.raises(ek.EKError) as e:
        ek.cluster_host(h, 2)
    assert e.value.code == ek.EK_EINVAL
    # max_net below 2 acts as 2
    h, cap, _ = cc.hypergraph(ek, "path_rising")
    a, b = ek.cluster_host(h, cap, 0, 0), ek.cluster_host(h, cap, 2, 0)
    assert np.array_equal(a[0], b[0]) and a[3]["eligible_nets"] == b[3]["eligible_nets"] == 5
    # opts NULL: the matching's defaults (max_cluster 2), null outputs allowed
    r = ek.ClusterResult()
    assert ek.lib.ek_cluster_host(h._h, None, None, None, None, 0, ctypes.byref(r)) == ek.EK_OK
    assert (r.n, r.n_coarse, r.joins, r.heaviest) == (6, 3, 3, 2)


def test_short_round_log(ek):
    h, cap, max_net = cc.hypergraph(ek, "star_hub_greatest")
    o = ek.MatchOpts(max_net, 0, cap)
    log = np.full((1, 3), -7, np.int64)
    r = ek.ClusterResult()
    assert ek.lib.ek_cluster_host(h._h, ctypes.byref(o), None, None, log.ctypes.data, 1, ctypes.byref(r)) == ek.EK_OK
    assert r.rounds == 2 and log.tolist() == [[5, 1, 1]]


NEW_SYMBOLS = ["ek_cluster_host", "ek_cluster", "ek_partition_kway_direct_ex", "ek_partition_kway_direct_file_ex"]


def test_new_symbols_are_declared_and_exported(ek):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "eigkl.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ek_[a-z0-9_]+)\s*\(", text))
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(ek.lib, s), s
    assert re.search(r"#define EIGKL_ABI_VERSION 4\b", text)  # new structs and entries only


def test_struct_layout_matches_python_mirror(ek, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "eigkl.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu %zu %zu\\n", sizeof(ek_cluster_result), offsetof(ek_cluster_result, joins),'
        " offsetof(ek_cluster_result, rounds), offsetof(ek_cluster_result, heaviest), offsetof(ek_cluster_result, t_setup));\n"
        '  printf("%d %d %zu %zu\\n", EK_COARSEN_MATCH, EK_COARSEN_CLUSTER, sizeof(ek_kway_direct_opts),'
        " sizeof(ek_kway_direct_result));\n"
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    a, b = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(x) for x in a.split()] == [ctypes.sizeof(ek.ClusterResult), ek.ClusterResult.joins.offset,
                                           ek.ClusterResult.rounds.offset, ek.ClusterResult.heaviest.offset,
                                           ek.ClusterResult.t_setup.offset]
    assert [int(x) for x in b.split()] == [ek.COARSEN_MATCH, ek.COARSEN_CLUSTER, ctypes.sizeof(ek.KwayDirectOpts),
                                           ctypes.sizeof(ek.KwayDirectResult)]
    assert (ek.COARSEN_MATCH, ek.COARSEN_CLUSTER) == (0, 1) and ek.ABI_VERSION == 4


def test_python_refuses_an_unknown_coarsening(ek):
    with pytest.raises(ValueError):
        ek._coarsening("matching")
    assert ek._coarsening("match") == 0 and ek._coarsening("cluster") == 1


REFUSED = [
    ["--k", "4", "--coarsen", "cluster"],                                # without --kway-direct
    ["--k", "4", "--coarsen", "match"],
    ["--k", "4", "--kway-direct", "0.03", "--coarsen"],                  # without a value
    ["--k", "4", "--kway-direct", "0.03", "--coarsen", "matching"],      # another word
    ["--k", "4", "--kway-direct", "0.03", "--coarsen", "CLUSTER"],
    ["--k", "4", "--kway-multilevel", "0.03", "--coarsen", "cluster"],   # not the direct path
    ["--kway-direct", "0.03", "--coarsen", "cluster"],                   # without --k
]


@pytest.mark.parametrize("flags", REFUSED, ids=lambda f: " ".join(f))
def test_cli_refuses_with_the_usage_text(tmp_path, flags):
    r = subprocess.run([GKL2, circuit_path("fract"), "-EIG"] + flags, cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "Usage: gKL2 <input_file> -EIG --k <parts> --kway-direct <imbalance>" in r.stdout
    assert "[--coarsen match|cluster]" in r.stdout
    assert not any(ln.startswith("kway-direct:") for ln in r.stdout.splitlines())
    assert "HIP" not in r.stderr and "device" not in r.stderr  # refused before any GPU work
    assert not (tmp_path / "results").exists()
