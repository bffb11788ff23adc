"""The sweep cut on the GPU (ek_sweep_cut, ek_kl_set_partition_fiedler_sweep)
against its host checker (ek_sweep_cut_host): the rule is integer and every
tie is broken by ids, so the order, the profile and every integer of the
result must be identical, whatever order the workgroups run in."""
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu

T = sc.TILE
# T - 1 | T | T + 1 and 2T + 1: one tile, its edge, more than one; the last n
# makes the (digit, tile) table's scan span two workgroups (sweep_cases.py)
SORT_NS = (2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, sc.N_TABLE_SCAN_SPANS_WORKGROUPS)


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def graphs(ek):
    out = {}
    for name, (nodes, ptr, pins) in sc.small_hypergraphs().items():
        out[name] = (ek.Hypergraph.from_pins(nodes, ptr, pins), nodes, ptr, pins)
    for name in ("fract", "ibm01"):
        h = ek.Hypergraph.read(circuit_path(name))
        out[name] = (h, h.nodes, *h.pins())
    return out


@pytest.fixture(scope="module")
def fiedler(ek, ctx, graphs):
    """name -> the Fiedler vector ctx.lanczos_fiedler returns (computed once, never changed)."""
    out = {}
    for name in ("fract", "ibm01"):
        ctx.spmv_setup_pins(graphs[name][0])
        _, v, st = ctx.lanczos_fiedler()
        assert st["converged"]
        v.setflags(write=False)
        out[name] = v
    return out


def same_as_host(ek, ctx, h, v, eps, ratio):
    want, worder, wprofile = ek.sweep_cut_host(h, v, eps, ratio)
    res, order, profile = ctx.sweep_cut(h, v, eps, ratio)
    assert np.array_equal(order, worder), int(np.count_nonzero(order != worder))
    assert np.array_equal(profile, wprofile), int(np.count_nonzero(profile != wprofile))
    assert sc.ints(res) == sc.ints(want)
    return res, order, profile


@pytest.mark.parametrize("n", SORT_NS)
def test_sort_shapes_and_value_families(ek, ctx, n):
    nodes, ptr, pins = sc.shape_hypergraph(n)
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    bare = ek.Hypergraph.from_pins(n, np.zeros(1, np.int64), np.zeros(0, np.int32))
    for fam, v in sc.value_families(n).items():
        res, order, _ = same_as_host(ek, ctx, h, v, 0.03, False)
        assert res["spanning_nets"] >= 1  # the net of all n pins
        same_as_host(ek, ctx, h, v, 0.5, True)
        # no nets: a zero profile and the most balanced split
        res, order0, profile = same_as_host(ek, ctx, bare, v, 0.5, False)
        assert np.array_equal(order0, order) and not profile.any()
        assert (res["n1"], res["cut"], res["cut_mid"], res["spanning_nets"]) == (n // 2, 0, 0, 0)


@pytest.mark.parametrize("name", sorted(sc.small_hypergraphs()))
def test_profile_and_choice_small(ek, ctx, graphs, name):
    h, nodes, _, _ = graphs[name]
    v = sc.value_families(nodes, 2)["normal"]
    for eps in sc.EPSILONS:
        for ratio in (False, True):
            same_as_host(ek, ctx, h, v, eps, ratio)
    same_as_host(ek, ctx, h, sc.value_families(nodes, 2)["three-values"], 0.5, True)


@pytest.mark.parametrize("name", ["fract", "ibm01"])
def test_profile_and_choice_circuits(ek, ctx, graphs, fiedler, name):
    h, nodes, ptr, pins = graphs[name]
    v = fiedler[name]
    for eps in sc.EPSILONS:
        for ratio in (False, True):
            res, _, _ = same_as_host(ek, ctx, h, v, eps, ratio)
            print(f"{name} eps={eps} ratio={ratio}: window {res['s_lo']}..{res['s_hi']}, n1 {res['n1']}, "
                  f"cut_mid {res['cut_mid']}, cut {res['cut']}")
    # a net that holds all n pins
    everyone = np.random.default_rng(8).permutation(nodes).astype(np.int32)
    big = ek.Hypergraph.from_pins(nodes, np.concatenate([ptr, [ptr[-1] + nodes]]).astype(np.int64),
                                  np.concatenate([pins, everyone]).astype(np.int32))
    res, _, profile = same_as_host(ek, ctx, big, v, 0.03, False)
    assert int(profile[1:nodes].min()) >= 1


@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("eps,ratio", [(0.0, False), (0.03, False), (0.5, True), (10.0, False)])
def test_context_path(ek, ctx, graphs, name, eps, ratio):
    h, nodes, ptr, pins = graphs[name]
    ctx.spmv_setup_pins(h)
    _, v, st = ctx.lanczos_fiedler()
    assert st["converged"]
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(ptr, pins)
    res = ctx.kl_set_partition_fiedler_sweep(h, eps, ratio)
    want, _, _ = ek.sweep_cut_host(h, v, eps, ratio)
    assert sc.ints(res) == sc.ints(want)
    assert np.array_equal(ctx.kl_sides(0), ek.rank_split(v, res["n1"]))
    _, kl = ctx.kl_run()
    # net_cut_initial comes from the existing k_net_cut, not from the sweep's kernels
    assert kl["net_cut_initial"] == res["cut"]
    assert kl["net_cut_best"] <= kl["net_cut_initial"]
    for which in (1, 2):  # KL swaps pairs: the side sizes survive
        assert int(ctx.kl_sides(which).sum()) == res["n1"]
    print(f"{name} eps={eps} ratio={ratio}: n1 {res['n1']}, cut_mid {res['cut_mid']}, cut {res['cut']}, "
          f"KL best {kl['net_cut_best']}")


def test_two_calls_agree(ek, ctx, graphs, fiedler):
    h = graphs["ibm01"][0]
    a, oa, pa = ctx.sweep_cut(h, fiedler["ibm01"], 0.1, True)
    b, ob, pb = ctx.sweep_cut(h, fiedler["ibm01"], 0.1, True)
    assert sc.ints(a) == sc.ints(b) and np.array_equal(oa, ob) and np.array_equal(pa, pb)


def test_sweep_leaves_no_state_behind(ek, ctx, graphs, fiedler):
    ctx.sweep_cut(graphs["ibm01"][0], fiedler["ibm01"], 0.03)
    ibm01 = circuit_path("ibm01")
    res, log = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    fresh = ek.Context(0)
    try:
        res0, log0 = fresh.solve_file(ibm01, write_results=False, log_cap=8192)
    finally:
        fresh.close()
    swap_fields_equal(log, log0)
    assert res["kl"]["net_cut_best"] == res0["kl"]["net_cut_best"] and res["lambda"] == res0["lambda"]


def test_state_and_argument_errors(ek, graphs):
    h, nodes, ptr, pins = graphs["fract"]
    one = ek.Context(0)
    try:
        with pytest.raises(ek.EKError) as e:  # before ek_kl_graph_setup
            one.kl_set_partition_fiedler_sweep(h)
        assert e.value.code == ek.EK_ESTATE
        one.kl_graph_setup(h.kl_graph())
        with pytest.raises(ek.EKError) as e:  # no Fiedler vector
            one.kl_set_partition_fiedler_sweep(h)
        assert e.value.code == ek.EK_ESTATE
        one.spmv_setup_pins(h)
        one.lanczos_fiedler()
        with pytest.raises(ek.EKError) as e:  # another hypergraph's node count
            one.kl_set_partition_fiedler_sweep(graphs["random"][0])
        assert e.value.code == ek.EK_EINVAL
        for eps in (-1.0, float("nan")):
            with pytest.raises(ek.EKError) as e:
                one.sweep_cut(h, np.zeros(nodes), eps)
            assert e.value.code == ek.EK_EINVAL
        assert one.kl_set_partition_fiedler_sweep(h)["n"] == nodes
    finally:
        one.close()


def test_multirank_context_is_refused(ek, graphs):
    h = graphs["fract"][0]
    one = ek.Context(0)
    try:
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.kl_set_partition_fiedler_sweep(h)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def _gkl2(*args, cwd, tool="gKL2"):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", tool), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def test_cli_sweep(ek, ctx, graphs, tmp_path):
    fract = circuit_path("fract")
    h, _, ptr, pins = graphs["fract"]
    ctx.spmv_setup_pins(h)
    ctx.lanczos_fiedler()
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(ptr, pins)
    res = ctx.kl_set_partition_fiedler_sweep(h, 0.1)
    _, kl = ctx.kl_run()
    sides = ctx.kl_sides(1)
    r = _gkl2(fract, "-EIG", "--sweep", "0.1", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    text = (tmp_path / "results" / "fract.hgr.part.2").read_text()
    assert [int(x) for x in text.split()] == sides.tolist()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("sweep:")]
    assert len(line) == 1
    got = re.search(r"imbalance 0\.1 .*window (\d+)\.\.(\d+) \(max part (\d+)\), n1 (\d+), cut_mid (\d+), cut (\d+), "
                    r"net_cut_best (\d+)", line[0])
    assert got, line[0]
    assert [int(x) for x in got.groups()] == [res["s_lo"], res["s_hi"], res["max_part"], res["n1"], res["cut_mid"],
                                              res["cut"], kl["net_cut_best"]]


def test_cli_sweep_usage_errors(tmp_path):
    """Refused while the arguments are read: no GPU work."""
    fract = circuit_path("fract")
    for args in ((fract, "--sweep", "0.1"), (fract, "-EIG", "--sweep", "0.1", "--k", "4"),
                 (fract, "-EIG", "--sweep", "-0.5"), (fract, "-EIG", "--sweep", "abc"), (fract, "-EIG", "--sweep", "nan"),
                 (fract, "-EIG", "--sweep"), (fract, "-EIG", "--sweep-ratio")):
        r = _gkl2(*args, cwd=tmp_path)
        assert r.returncode != 0 and ("Usage" in r.stdout or "Error" in r.stderr), args
        assert not (tmp_path / "results" / "fract.hgr.part.2").exists()
    for tool in ("cEIG", "cKL", "gKL"):
        r = _gkl2(fract, "-EIG", "--sweep", "0.1", cwd=tmp_path, tool=tool)
        assert r.returncode != 0 and "Usage" in r.stdout, tool
