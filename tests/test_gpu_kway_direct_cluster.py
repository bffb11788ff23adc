"""The direct k-way multilevel driver under EK_COARSEN_CLUSTER (ek_partition_kway_direct_ex) on the GPU.  The driver is
a composition of public entries, so the cycle that test_gpu_kway_direct.py composes, with ctx.cluster where it has
ctx.match, must give the same part vector and the same result integers; the four promises of DESIGN.md §19 must hold at
every level; EK_COARSEN_MATCH must be ek_partition_kway_direct itself; and the CLI's --coarsen must reach the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import match_cases as mc
import test_gpu_kway_direct as kd
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

CASES = [(name, weighted, k) for name in ("fract", "ibm01") for weighted in (False, True) for k in (2, 8)]
EPS = 0.03


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


class ClusterForMatch:
    """The context with `match` answering from `cluster`: what kd.compose needs to compose the clustering cycle.  The
    driver reports the clustering's rounds and joins where it reports the matching's rounds and pairs."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def match(self, h, max_cluster):
        rep, cluster, log, res = self._ctx.cluster(h, max_cluster)
        return rep, cluster, log, dict(res, pairs=res["joins"])


@pytest.mark.parametrize("name, weighted, k", CASES)
def test_driver_equals_its_composition_and_keeps_its_promises(ek, ctx, name, weighted, k):
    h = kd.circuit(ek, name, weighted)
    coarse = kd.COARSE[name]
    part, res = ctx.partition_kway_direct(h, k, EPS, coarse_nodes=coarse, coarsening="cluster")
    want, r, initial_w, projections = kd.compose(ek, ClusterForMatch(ctx), h, k, EPS, coarse)
    assert part.tobytes() == want.tobytes()
    assert kd.ints(res) == kd.ints(r)
    assert part.min() >= 0 and part.max() < k  # every node has a part
    L = res["levels"]
    for l in range(L):  # the weighted connectivity survives the projection
        assert res["conn_w_before"][l] == res["conn_w_after"][l + 1], l
        assert res["match_pairs"][l] == res["nodes"][l] - res["nodes"][l + 1]  # the joins of the level
    for l in range(L + 1):  # Jet never returns worse than it was given
        assert res["conn_w_after"][l] <= res["conn_w_before"][l], l
    assert res["connectivity_w"] == res["conn_w_after"][0]
    assert len(projections) == L
    for coarse_w, fine_w in projections:  # part weights are unchanged by projection
        assert list(coarse_w) == list(fine_w)
    final_w = kd.part_weights(ek, h, part, k)
    for p in range(k):  # no part ends above max(Lk, its weight after the initial partition)
        assert final_w[p] <= max(res["part_bound"], initial_w[p]), p
    assert res["parts_over_bound"] == sum(int(x) > res["part_bound"] for x in final_w)


def test_clustering_coarsens_ibm01_further_than_matching(ek, ctx):
    """Structure, not speed: under the driver's own defaults the clustering's first level has fewer nodes than the
    matching's can have (a matching at most halves), and it reaches coarse_nodes in fewer levels."""
    h = kd.circuit(ek, "ibm01", False)
    _, m = ctx.partition_kway_direct(h, 4, EPS)
    _, c = ctx.partition_kway_direct(h, 4, EPS, coarsening="cluster")
    assert 2 * m["nodes"][1] >= m["nodes"][0] > 2 * c["nodes"][1]
    assert 1 <= c["levels"] < m["levels"] and c["nodes"][-1] <= 512 and c["max_cluster"] == m["max_cluster"] == 95


def raw(ek, ctx, h, k, call, *extra):
    o = ek.KwayDirectOpts()
    ek.lib.ek_kway_direct_default_opts(ctypes.byref(o))
    o.k = k
    part = np.full(h.nodes, -1, np.int32)
    r = ek.KwayDirectResult()
    rc = call(ctx._c, h._h, ctypes.byref(o), *extra, part.ctypes.data, ctypes.byref(r))
    return rc, part, r


@pytest.mark.parametrize("name, weighted, k", [("fract", True, 3), ("ibm01", False, 2)])
def test_ex_with_match_is_the_plain_entry_byte_for_byte(ek, ctx, name, weighted, k):
    h = kd.circuit(ek, name, weighted)
    rc0, part0, r0 = raw(ek, ctx, h, k, ek.lib.ek_partition_kway_direct)
    rc1, part1, r1 = raw(ek, ctx, h, k, ek.lib.ek_partition_kway_direct_ex, ek.COARSEN_MATCH)
    assert rc0 == rc1 == ek.EK_OK and part0.tobytes() == part1.tobytes()
    times = len(ek._KWAY_DIRECT_TIMES) * 8  # the wall seconds at the struct's end differ run to run
    assert bytes(r0)[:-times] == bytes(r1)[:-times]
    part2, res2 = ctx.partition_kway_direct(h, k, coarsening="match")
    assert part2.tobytes() == part0.tobytes()


def test_an_unknown_coarsening_is_einval(ek, ctx, tmp_path):
    h = kd.circuit(ek, "fract", False)
    for coarsening in (2, -1):
        rc, part, _ = raw(ek, ctx, h, 2, ek.lib.ek_partition_kway_direct_ex, coarsening)
        assert rc == ek.EK_EINVAL and np.all(part == -1)
    src = tmp_path / "fract.hgr"
    h.write(src)
    o = ek.KwayDirectOpts()
    ek.lib.ek_kway_direct_default_opts(ctypes.byref(o))
    assert ek.lib.ek_partition_kway_direct_file_ex(ctx._c, os.fsencode(str(src)), ctypes.byref(o), 2, None,
                                                   None) == ek.EK_EINVAL
    assert ek.lib.ek_partition_kway_direct_ex(ctx._c, None, None, 1, None, None) == ek.EK_EINVAL


def test_cli_coarsen(ek, ctx, tmp_path):
    h = kd.circuit(ek, "ibm01", True)
    src = tmp_path / "ibm01w.hgr"
    h.write(src)  # fmt 11
    lines, parts = {}, {}
    for word in ("cluster", "match"):
        r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), str(src), "-EIG", "--k", "5", "--kway-direct",
                            "0.03", "--ml-coarse", "700", "--jet-iters", "40", "--coarsen", word],
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("kway-direct:")]
        assert len(line) == 1 and f"coarsen {word}," in line[0], r.stdout
        lines[word] = {k: int(v) for k, v in re.findall(rf"\b({kd.CLI_KEYS}) (-?\d+)", line[0])}
        parts[word] = np.array((tmp_path / "results" / "ibm01w.hgr.part.5").read_text().split(), np.int32)
    for word in ("cluster", "match"):
        want, res = ctx.partition_kway_direct(h, 5, 0.03, coarse_nodes=700, jet={"max_iters": 40}, coarsening=word)
        assert parts[word].tobytes() == want.tobytes()
        got = lines[word]
        assert (got["levels"], got["coarsest_nodes"], got["max_cluster"], got["connectivity_w"], got["cut nets"]) == \
               (res["levels"], res["nodes"][-1], res["max_cluster"], res["connectivity_w"], res["cut_nets"])
        assert (got["jet iterations"], got["jet moves"]) == (sum(res["jet_iters"]), sum(res["jet_moves"]))
    # the library's file entry writes the same file
    part_f, res_f = ctx.partition_kway_direct_file(str(src), 5, 0.03, coarse_nodes=700, jet={"max_iters": 40},
                                                   out_dir=str(tmp_path / "lib"), coarsening="cluster")
    assert part_f.tobytes() == parts["cluster"].tobytes()
    assert (tmp_path / "lib" / "results" / "ibm01w.hgr.part.5").read_text().split() == \
           [str(x) for x in parts["cluster"]]


def test_a_star_of_65_nodes(ek, ctx):
    """What the matching cannot do: the hub pairs with one leaf and 63 leaves stay; the clustering takes all 64."""
    h = ek.Hypergraph.from_pins(65, *mc.pack([[0, v] for v in range(1, 65)]))
    _, _, _, m = ctx.match(h, 65, 64, 0)
    rep, cluster, log, c = ctx.cluster(h, 65, 64, 0)
    assert m["n_coarse"] == 64 and c["n_coarse"] == 1
    assert not rep.any() and not cluster.any() and log.tolist() == [[65, 64, 64]] and c["heaviest"] == 65
