"""ek_fm_refine_w on the GPU: device = host bit for bit (sides, pass log, move
log, every result integer) on every weighted case, on every fm_cases case
under explicit all-ones weights and on the circuits under synthetic weights;
no context state, the multi-rank refusal, the EK_EINVAL cases, the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

import fm_cases as fc
import fmw_cases as wc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def synthetic_weights(h):
    """Node weight 1 + (id mod 5), net weight 1 + (e mod 3)."""
    return (1 + np.arange(h.nodes) % 5).astype(np.int32), (1 + np.arange(h.nets) % 3).astype(np.int32)


@pytest.mark.parametrize("name", wc.names())
def test_device_equals_host(ek, ctx, name):
    h, (side, eps, max_passes, stall) = wc.hypergraph(ek, name)
    want = ek.fm_refine_w_host(h, side, eps, max_passes, stall)
    wc.same(ctx.fm_refine_w(h, side, eps, max_passes, stall), want)


@pytest.mark.parametrize("name", fc.names())
def test_device_equals_host_under_all_ones(ek, ctx, name):
    nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    h.set_weights(np.ones(nodes, np.int32), np.ones(len(ptr) - 1, np.int32))
    want = ek.fm_refine_w_host(h, side, eps, max_passes, stall)
    wc.same(ctx.fm_refine_w(h, side, eps, max_passes, stall), want)


def test_key_sizes_are_the_lds_and_the_global_path():
    sizes = sorted(wc.cases()[x][0] for x in wc.names() if x.startswith("keys_"))
    assert sizes == [wc.LDS_CHUNKS * wc.C, wc.LDS_CHUNKS * wc.C + 1]
    for x in wc.names():
        if x.startswith("keys_"):
            _, _, _, node_w, net_w, *_ = wc.cases()[x]
            assert set(node_w.tolist()) == {1, 2, 3} and set(net_w.tolist()) == {1, 2}


def test_fract_and_ibm01_from_kl_best_prefix(ek, ctx):
    for name in ("fract", "ibm01"):
        path = circuit_path(name)
        h = ek.Hypergraph.read(path)
        h.set_weights(*synthetic_weights(h))
        ctx.solve_file(path, write_results=False)
        side = ctx.kl_sides(1)
        want = ek.fm_refine_w_host(h, side, 0.03)
        assert (want[3]["cut_before"], want[3]["cut_nets_before"]) == ek.bipart_metrics_host(h, side)[:2]
        wc.same(ctx.fm_refine_w(h, side, 0.03), want)
        assert want[3]["cut"] <= want[3]["cut_before"]


def test_fmw_leaves_no_state_behind(ek, ctx):
    ibm01 = circuit_path("ibm01")
    h = ek.Hypergraph.read(ibm01)
    h.set_weights(*synthetic_weights(h))
    ctx.fm_refine_w(h, (np.arange(h.nodes) % 2).astype(np.uint8), 0.03, 2, 50)
    res, log = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    fresh = ek.Context(0)
    try:
        res0, log0 = fresh.solve_file(ibm01, write_results=False, log_cap=8192)
    finally:
        fresh.close()
    swap_fields_equal(log, log0)
    assert res["kl"]["net_cut_best"] == res0["kl"]["net_cut_best"] and res["lambda"] == res0["lambda"]
    # ... and between a solve and its sides
    side = ctx.kl_sides(1)
    ctx.fm_refine_w(h, side, 0.03, 1, 10)
    assert np.array_equal(ctx.kl_sides(1), side)


def test_multirank_context_is_refused(ek):
    h, (side, eps, *_) = wc.hypergraph(ek, "hill_joins5")
    one = ek.Context(0)
    try:
        one.comm_init_host(1, 0, lambda send: send, lambda buf: None)  # one rank: a single context
        wc.same(one.fm_refine_w(h, side, eps), ek.fm_refine_w_host(h, side, eps))

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.fm_refine_w(h, side, eps)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def test_device_einval(ek, ctx):
    h, (side, *_) = wc.hypergraph(ek, "degenerate")
    bad = side.copy()
    bad[3] = 2
    for args in ((bad, 0.03), (side, -1.0), (side, float("nan"))):
        with pytest.raises(ek.EKError) as e:
            ctx.fm_refine_w(h, *args)
        assert e.value.code == ek.EK_EINVAL
    ptr, pins = fc.pack([[0, 1], [0, 2]])  # the nets on node 0 sum to 2^31
    h = ek.Hypergraph.from_pins(3, ptr, pins)
    h.set_weights(None, [2 ** 30, 2 ** 30])
    with pytest.raises(ek.EKError) as e:
        ctx.fm_refine_w(h, [0, 1, 1])
    assert e.value.code == ek.EK_EINVAL


def _gkl2(*args, cwd):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def _line(stdout, tag, keys):
    line = [ln for ln in stdout.splitlines() if ln.startswith(tag)]
    assert len(line) == 1, stdout
    return {k: int(v) for k, v in re.findall(rf"\b({keys}) (-?\d+)", line[0])}


FMW_KEYS = "cut_before|cut|cut_nets_before|cut_nets|passes|w0|w1|total_weight|max_part|n0|n1"


def test_cli_weighted(ek, ctx, tmp_path):
    h = ek.Hypergraph.read(circuit_path("fract"))
    h.set_weights(*synthetic_weights(h))
    src = tmp_path / "fractw.hgr"
    h.write(src)  # fmt 11
    assert src.read_text().splitlines()[0] == f"{h.nets} {h.nodes} 11"
    for extra in ((), ("--sweep", "0.1")):
        cwd = tmp_path / ("run" + str(len(extra)))
        cwd.mkdir()
        r = _gkl2(str(src), "-EIG", *extra, "--fm", "0.1", "--weighted", cwd=cwd)
        assert r.returncode == 0, r.stderr
        got = _line(r.stdout, "fmw:", FMW_KEYS)
        assert not any(ln.startswith("fm:") for ln in r.stdout.splitlines())
        part = np.array((cwd / "results" / "fractw.hgr.part.2").read_text().split(), np.uint8)
        assert len(part) == h.nodes and set(part.tolist()) <= {0, 1}
        assert (got["cut"], got["cut_nets"], got["w0"], got["w1"]) == ek.bipart_metrics_host(h, part)
        assert got["total_weight"] == got["w0"] + got["w1"] and got["max_part"] == wc.max_part(got["total_weight"], 0.1)
        assert (got["n0"], got["n1"]) == (int(np.count_nonzero(part == 0)), int(np.count_nonzero(part == 1)))
        assert got["cut"] <= got["cut_before"]
        if not extra:  # the library from the same start: the structure's KL best prefix, then the weighted FM
            ctx.solve_file(circuit_path("fract"), write_results=False)
            side, _, _, res = ctx.fm_refine_w(h, ctx.kl_sides(1), 0.1)
            assert np.array_equal(side, part) and {k: res[k] for k in got} == got


def test_cli_unweighted_is_unchanged(ek, ctx, tmp_path):
    fract = circuit_path("fract")
    h = ek.Hypergraph.read(fract)
    r = _gkl2(fract, "-EIG", "--fm", "0.1", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    got = _line(r.stdout, "fm:", "cut_before|cut|passes|n0|n1|max_part")
    assert not any(ln.startswith("fmw:") for ln in r.stdout.splitlines())
    ctx.solve_file(fract, write_results=False)
    side, _, _, res = ctx.fm_refine(h, ctx.kl_sides(1), 0.1)
    assert {k: res[k] for k in got} == got
    part = np.array((tmp_path / "results" / "fract.hgr.part.2").read_text().split(), np.uint8)
    assert np.array_equal(part, side)
    # --weighted on the same unweighted file: the unweighted rule's sides and cut
    cwd = tmp_path / "w"
    cwd.mkdir()
    r = _gkl2(fract, "-EIG", "--fm", "0.1", "--weighted", cwd=cwd)
    assert r.returncode == 0, r.stderr
    gotw = _line(r.stdout, "fmw:", FMW_KEYS)
    assert {k: gotw[k] for k in got} == got and gotw["cut_nets"] == got["cut"]
    assert np.array_equal(np.array((cwd / "results" / "fract.hgr.part.2").read_text().split(), np.uint8), side)


@pytest.mark.parametrize("args", [("--weighted",), ("--weighted", "--k", "4"), ("--weighted", "--fm", "0.1", "--k", "4"),
                                  ("--weighted", "--sweep", "0.1")], ids=lambda a: " ".join(a))
def test_cli_misuse_prints_usage(tmp_path, args):
    r = _gkl2(circuit_path("fract"), "-EIG", *args, cwd=tmp_path)
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--weighted" in r.stdout
    assert not (tmp_path / "results" / "fract.hgr.part.2").exists()
