"""ek_fm_refine on the GPU: device = host bit for bit (sides, pass log, move
log, result integers) on every shared case and on the circuits, no context
state, the multi-rank refusal, the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

import fm_cases as fc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", fc.names())
def test_device_equals_host(ek, ctx, name):
    nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    want = ek.fm_refine_host(h, side, eps, max_passes, stall)
    fc.same(ctx.fm_refine(h, side, eps, max_passes, stall), want)


def test_fract_and_ibm01_from_kl_best_prefix(ek, ctx):
    for name in ("fract", "ibm01"):
        path = circuit_path(name)
        h = ek.Hypergraph.read(path)
        res, _ = ctx.solve_file(path, write_results=False)
        side = ctx.kl_sides(1)
        for stall in (1000, 0) if name == "fract" else (1000,):
            want = ek.fm_refine_host(h, side, 0.03, 0, stall)
            assert want[3]["cut_before"] == res["kl"]["net_cut_best"]
            fc.same(ctx.fm_refine(h, side, 0.03, 0, stall), want)
            assert want[3]["cut"] <= want[3]["cut_before"]


def test_fm_leaves_no_state_behind(ek, ctx):
    ibm01 = circuit_path("ibm01")
    h = ek.Hypergraph.read(ibm01)
    ctx.fm_refine(h, (np.arange(h.nodes) % 2).astype(np.uint8), 0.03, 2, 50)
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
    ctx.fm_refine(h, side, 0.03, 1, 10)
    assert np.array_equal(ctx.kl_sides(1), side)


def test_multirank_context_is_refused(ek):
    nodes, ptr, pins, side, eps, _, _ = fc.cases()["hill"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    one = ek.Context(0)
    try:
        one.comm_init_host(1, 0, lambda send: send, lambda buf: None)  # one rank: a single context
        fc.same(one.fm_refine(h, side, eps), ek.fm_refine_host(h, side, eps))

        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.fm_refine(h, side, eps)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()


def test_device_einval(ek, ctx):
    nodes, ptr, pins, side, _, _, _ = fc.cases()["degenerate"]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    bad = side.copy()
    bad[3] = 2
    for args in ((bad, 0.03), (side, -1.0), (side, float("nan"))):
        with pytest.raises(ek.EKError) as e:
            ctx.fm_refine(h, *args)
        assert e.value.code == ek.EK_EINVAL


def _gkl2(*args, cwd):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def _fm_line(stdout):
    line = [ln for ln in stdout.splitlines() if ln.startswith("fm:")]
    assert len(line) == 1, stdout
    return {k: int(v) for k, v in re.findall(r"(cut_before|cut|passes|n0|n1|max_part) (-?\d+)", line[0])}


def test_cli(ek, tmp_path):
    fract = circuit_path("fract")
    h = ek.Hypergraph.read(fract)
    ptr, pins = h.pins()
    for extra in ((), ("--sweep", "0.1"), ("--fm-passes", "1", "--fm-stall", "5")):
        cwd = tmp_path / ("run" + str(len(extra)))
        cwd.mkdir()
        r = _gkl2(fract, "-EIG", *extra[:2 if extra[:1] == ("--sweep",) else 0], "--fm", "0.1",
                  *extra[2 if extra[:1] == ("--sweep",) else 0:], cwd=cwd)
        assert r.returncode == 0, r.stderr
        got = _fm_line(r.stdout)
        part = np.array((cwd / "results" / "fract.hgr.part.2").read_text().split(), np.int32)
        assert len(part) == h.nodes == 149 and set(part.tolist()) <= {0, 1}
        assert ek.kway_metrics_host(ptr, pins, part, 2)[0] == got["cut"] <= got["cut_before"]
        assert got["max_part"] == fc.max_part(149, 0.1) == 82
        assert (got["n0"], got["n1"]) == (int(np.count_nonzero(part == 0)), int(np.count_nonzero(part == 1)))
        assert max(got["n0"], got["n1"]) <= got["max_part"]
        if extra[:1] == ("--sweep",):
            assert any(ln.startswith("sweep:") for ln in r.stdout.splitlines())
        if extra[:1] == ("--fm-passes",):
            assert got["passes"] <= 1


@pytest.mark.parametrize("args", [
    ("--fm",), ("--fm", "x"), ("--fm", "-0.1"), ("--fm", "nan"), ("--fm", "0.1", "--k", "4"),
    ("--fm-passes", "2"), ("--fm-stall", "5"), ("--fm", "0.1", "--fm-passes"), ("--fm", "0.1", "--fm-stall", "y"),
    ("--fm", "0.1", "--fm-stall", "-1"), ("--fm", "0.1", "--sweep-ratio")], ids=lambda a: " ".join(a))
def test_cli_misuse_exits_1(tmp_path, args):
    r = _gkl2(circuit_path("fract"), "-EIG", *args, cwd=tmp_path)
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout and "--fm" in r.stdout
    assert not (tmp_path / "results" / "fract.hgr.part.2").exists()


def test_cli_fm_needs_gkl2_and_eig(tmp_path):
    fract = circuit_path("fract")
    r = _gkl2(fract, "--fm", "0.1", cwd=tmp_path)  # no -EIG
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "cKL"), fract, "-EIG", "--fm", "0.1"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Usage: gKL2" in r.stdout
