"""The weighted sweep cut on the GPU (ek_sweep_cut_w,
ek_kl_set_partition_fiedler_sweep_w) against its host checker
(ek_sweep_cut_w_host): the rule is integer and every tie is broken by ids, so
the order, profile_w, P and every integer of the result must be identical,
whatever order the workgroups run in.  Then the context path, the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
import sweepw_cases as wc
from conftest import PKG_DIR, circuit_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def weighted_circuit(ek, name):
    h = ek.Hypergraph.read(circuit_path(name))
    h.set_weights(*wc.synthetic_weights(h.nodes, h.nets))
    return h


def same_as_host(ek, ctx, h, v, eps):
    want, worder, wprofw, wprefix = ek.sweep_cut_w_host(h, v, eps)
    res, order, profw, prefix = ctx.sweep_cut_w(h, v, eps)
    assert np.array_equal(order, worder), int(np.count_nonzero(order != worder))
    assert np.array_equal(profw, wprofw), int(np.count_nonzero(profw != wprofw))
    assert np.array_equal(prefix, wprefix), int(np.count_nonzero(prefix != wprefix))
    assert wc.ints(res) == wc.ints(want)
    return res, order, profw, prefix


@pytest.mark.parametrize("name", wc.names())
def test_device_equals_host(ek, ctx, name):
    """Among the cases: n + 1 = 2,047 | 2,048 | 2,049 words (n2046, n2047, n2048: the scans' block edge), nets
    of 8 | 9, 64 | 65 and n pins (metrics+all: thread / wave hand-over), 5,000 nets on one lo and one hi at weight
    2^31 - 1 (contended: carries into the high word), no feasible split (heavy_node)."""
    h, v, epsilons = wc.hypergraph(ek, name)
    for eps in epsilons:
        res, _, _, _ = same_as_host(ek, ctx, h, v, eps)
        assert wc.ints(res) == wc.reference(name, eps)[0]


def test_scan_of_block_sums_second_step(ek, ctx):
    """n = 524,288: the scans run over n + 1 = 256 * 2,048 + 1 words, 257 block sums, and k_scan_top takes 256 a
    step, so this is the smallest n at which its second step, with the carry of the first, runs: in its 64-bit
    instantiation (profile_w, P) and in its 32-bit one (the count profile)."""
    n, ptr, pins, node_w, net_w, v = wc.big_case()
    assert n == wc.N_TOP_SCAN_SECOND_STEP == 524288 and -(-(n + 1) // wc.SCAN_BLOCK) == wc.SCAN_TOP + 1
    h = ek.Hypergraph.from_pins(n, ptr, pins)
    h.set_weights(node_w, net_w)
    res, _, profw, prefix = same_as_host(ek, ctx, h, v, 0.03)
    assert res["feasible"] == 1 and int(profw[1:n].min()) >= 1 and int(prefix[-1]) == int(node_w.sum())


@pytest.mark.parametrize("name", sorted(sc.small_hypergraphs()))
def test_all_ones_is_the_unweighted_sweep(ek, ctx, name):
    nodes, ptr, pins = sc.small_hypergraphs()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    v = sc.value_families(nodes, 2)["normal"]
    for eps in sc.EPSILONS:
        want, worder, wprofile = ctx.sweep_cut(h, v, eps)
        res, order, profw, prefix = same_as_host(ek, ctx, h, v, eps)
        assert np.array_equal(order, worder) and np.array_equal(profw, wprofile)
        assert prefix.tolist() == list(range(nodes + 1))
        assert [res[k] for k in ("n1", "s_lo", "s_hi", "max_part", "cut", "cut_nets", "cut_half", "spanning_nets")] == \
               [want[k] for k in ("n1", "s_lo", "s_hi", "max_part", "cut", "cut", "cut_mid", "spanning_nets")]


@pytest.mark.parametrize("name", ["fract", "ibm01"])
@pytest.mark.parametrize("eps", wc.EPSILONS)
def test_context_path(ek, ctx, name, eps):
    h = weighted_circuit(ek, name)
    ptr, pins = h.pins()
    ctx.spmv_setup_pins(h)
    _, v, st = ctx.lanczos_fiedler()
    assert st["converged"]
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(ptr, pins)
    res = ctx.kl_set_partition_fiedler_sweep_w(h, eps)
    want, _, _, _ = ek.sweep_cut_w_host(h, v, eps)
    assert wc.ints(res) == wc.ints(want)
    sides = ek.rank_split(v, res["n1"])
    _, kl = ctx.kl_run()
    assert np.array_equal(ctx.kl_sides(0), sides)
    assert ek.bipart_metrics_host(h, sides) == (res["cut"], res["cut_nets"], res["w0"], res["w1"])
    if res["feasible"]:
        assert max(res["w0"], res["w1"]) <= res["max_part"]
    # the state ek_kl_set_partition_fiedler_rank leaves: the same KL run as after that call
    ctx.kl_set_partition_fiedler_rank(res["n1"])
    _, kl2 = ctx.kl_run()
    ints = ("iterations", "best_iter", "net_cut_initial", "net_cut_best", "net_cut_final")
    assert {k: kl[k] for k in ints} == {k: kl2[k] for k in ints}
    assert kl["net_cut_initial"] == res["cut_nets"]  # (from the existing k_net_cut, not from the sweep's kernels)
    for which in (1, 2):  # KL swaps pairs: the side sizes survive
        assert int(ctx.kl_sides(which).sum()) == res["n1"]
    print(f"{name} eps={eps}: window {res['s_lo']}..{res['s_hi']}, n1 {res['n1']}, w0 {res['w0']} | w1 {res['w1']}, "
          f"cut_half {res['cut_half']}, cut {res['cut']}, cut nets {res['cut_nets']}, KL best {kl['net_cut_best']}")


def test_sweepw_keeps_no_context_state(ek, ctx):
    h = weighted_circuit(ek, "ibm01")
    v = sc.value_families(h.nodes, 6)["normal"]
    before = ctx.sweep_cut(h, v, 0.1)
    a = ctx.sweep_cut_w(h, v, 0.1)
    after = ctx.sweep_cut(h, v, 0.1)
    b = ctx.sweep_cut_w(h, v, 0.1)
    assert sc.ints(before[0]) == sc.ints(after[0])
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert wc.ints(a[0]) == wc.ints(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_state_and_argument_errors(ek):
    h = weighted_circuit(ek, "fract")
    one = ek.Context(0)
    try:
        with pytest.raises(ek.EKError) as e:  # before ek_kl_graph_setup
            one.kl_set_partition_fiedler_sweep_w(h)
        assert e.value.code == ek.EK_ESTATE
        one.kl_graph_setup(h.kl_graph())
        with pytest.raises(ek.EKError) as e:  # no Fiedler vector
            one.kl_set_partition_fiedler_sweep_w(h)
        assert e.value.code == ek.EK_ESTATE
        one.spmv_setup_pins(h)
        one.lanczos_fiedler()
        with pytest.raises(ek.EKError) as e:  # another hypergraph's node count
            one.kl_set_partition_fiedler_sweep_w(wc.hypergraph(ek, "random")[0])
        assert e.value.code == ek.EK_EINVAL
        for eps in (-1.0, float("nan")):
            with pytest.raises(ek.EKError) as e:
                one.sweep_cut_w(h, np.zeros(h.nodes), eps)
            assert e.value.code == ek.EK_EINVAL
        assert one.kl_set_partition_fiedler_sweep_w(h)["n"] == h.nodes

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:  # a multi-rank context
            one.kl_set_partition_fiedler_sweep_w(h)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def _gkl2(*args, cwd, tool="gKL2"):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", tool), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def _line(stdout, tag, keys):
    line = [ln for ln in stdout.splitlines() if ln.startswith(tag)]
    assert len(line) == 1, stdout
    return {k: int(v) for k, v in re.findall(rf"\b({keys}) (-?\d+)", line[0])}


FMW_KEYS = "cut_before|cut|cut_nets_before|cut_nets|passes|w0|w1|total_weight|max_part|n0|n1"
SWEEPW_KEYS = "max_part|feasible|n1|w0|w1|total_weight|cut_half|cut|cut_nets"


@pytest.fixture(scope="module")
def ibm01w(ek, tmp_path_factory):
    h = weighted_circuit(ek, "ibm01")
    src = tmp_path_factory.mktemp("sweepw") / "ibm01w.hgr"
    h.write(src)  # fmt 11
    return h, str(src)


@pytest.mark.parametrize("no_kl", [False, True], ids=["kl", "no-kl"])
def test_cli_sweep_weighted(ek, ctx, ibm01w, tmp_path, no_kl):
    h, src = ibm01w
    r = _gkl2(src, "-EIG", "--sweep", "0.03", "--sweep-weighted", "--fm", "0.03", "--weighted",
              *(("--no-kl",) if no_kl else ()), cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert not any(ln.startswith(("sweep:", "fm:")) for ln in lines)
    assert sum(ln.startswith("kl:") for ln in lines) == (0 if no_kl else 1)
    got = _line(r.stdout, "sweepw:", SWEEPW_KEYS)
    window = re.search(r"^sweepw: imbalance 0\.03, window (\d+)\.\.(\d+) ", r.stdout, re.M)
    gotf = _line(r.stdout, "fmw:", FMW_KEYS)
    # the library, step by step
    ptr, pins = h.pins()
    ctx.spmv_setup_pins(h)
    _, v, _ = ctx.lanczos_fiedler()
    if no_kl:
        res, _, _, _ = ctx.sweep_cut_w(h, v, 0.03)
        start = ek.rank_split(v, res["n1"])
    else:
        ctx.kl_graph_setup(h.kl_graph())
        ctx.kl_nets_setup(ptr, pins)
        res = ctx.kl_set_partition_fiedler_sweep_w(h, 0.03)
        _, kl = ctx.kl_run()
        start = ctx.kl_sides(1)
        assert _line(r.stdout, "kl:", "net_cut_best")["net_cut_best"] == kl["net_cut_best"]
    assert {k: res[k] for k in got} == got and len(got) == 9
    assert [int(x) for x in window.groups()] == [res["s_lo"], res["s_hi"]]
    side, _, _, fres = ctx.fm_refine_w(h, start, 0.03)
    assert {k: fres[k] for k in gotf} == gotf and len(gotf) == 11
    part = np.array((tmp_path / "results" / "ibm01w.hgr.part.2").read_text().split(), np.uint8)
    assert np.array_equal(part, side)
    if no_kl:  # FM moves only within the bound, and the sweep started inside it
        assert res["feasible"] == 1 and max(gotf["w0"], gotf["w1"]) <= gotf["max_part"]


def test_cli_count_sweep_is_unchanged_without_the_flag(ek, ctx, ibm01w, tmp_path):
    """--weighted --sweep EPS keeps the count sweep: its line and the fmw line carry the library's integers."""
    h, src = ibm01w
    r = _gkl2(src, "-EIG", "--sweep", "0.03", "--fm", "0.03", "--weighted", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert not any(ln.startswith("sweepw:") for ln in r.stdout.splitlines())
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("sweep:")]
    assert len(line) == 1
    got = re.search(r"^sweep: imbalance 0\.03 \(minimum cut\), window (\d+)\.\.(\d+) \(max part (\d+)\), n1 (\d+), "
                    r"cut_mid (\d+), cut (\d+)$", line[0])
    assert got, line[0]
    ptr, pins = h.pins()
    ctx.spmv_setup_pins(h)
    ctx.lanczos_fiedler()
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(ptr, pins)
    res = ctx.kl_set_partition_fiedler_sweep(h, 0.03)
    assert [int(x) for x in got.groups()] == [res[k] for k in ("s_lo", "s_hi", "max_part", "n1", "cut_mid", "cut")]
    _, kl = ctx.kl_run()
    assert _line(r.stdout, "kl:", "net_cut_best")["net_cut_best"] == kl["net_cut_best"]
    gotf = _line(r.stdout, "fmw:", FMW_KEYS)
    side, _, _, fres = ctx.fm_refine_w(h, ctx.kl_sides(1), 0.03)
    assert {k: fres[k] for k in gotf} == gotf and len(gotf) == 11
    part = np.array((tmp_path / "results" / "ibm01w.hgr.part.2").read_text().split(), np.uint8)
    assert np.array_equal(part, side)


BASE = ("-EIG", "--sweep", "0.1", "--sweep-weighted", "--fm", "0.1", "--weighted")


@pytest.mark.parametrize("args", [
    ("-EIG", "--sweep-weighted", "--fm", "0.1", "--weighted"),  # no --sweep
    ("-EIG", "--sweep", "0.1", "--sweep-weighted", "--weighted"),  # no --fm
    ("-EIG", "--sweep", "0.1", "--sweep-weighted", "--fm", "0.1"),  # no --weighted
    BASE + ("--sweep-ratio",), BASE + ("--k", "4"), BASE[1:],  # the last: no -EIG
    ("-EIG", "--sweep", "0.1", "--fm", "0.1", "--weighted", "--no-kl"),  # --no-kl without --sweep-weighted
    ("-EIG", "--no-kl"), ("-EIG", "--sweep-weighted")], ids=lambda a: " ".join(a))
def test_cli_misuse_prints_usage(tmp_path, args):
    """Refused while the arguments are read: no GPU work."""
    r = _gkl2(circuit_path("fract"), *args, cwd=tmp_path)
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--sweep-weighted" in r.stdout and "--no-kl" in r.stdout
    assert not (tmp_path / "results" / "fract.hgr.part.2").exists()


def test_cli_misuse_other_tools(tmp_path):
    for tool in ("cEIG", "cKL", "gKL"):
        r = _gkl2(circuit_path("fract"), *BASE, cwd=tmp_path, tool=tool)
        assert r.returncode == 1 and "--sweep-weighted" in r.stdout, tool
