"""The k-way path on the GPU: the rank-split and metrics kernels against the
host entry points, and ek_partition_kway against a recursion written here from
the public pieces it is specified by (node for node: the solver is
deterministic)."""
import os
import subprocess

import numpy as np
import pytest

import kway_cases as kc
from conftest import PKG_DIR, circuit_path, swap_fields_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hgrs(ek):
    return {name: ek.Hypergraph.read(circuit_path(name)) for name in ("fract", "ibm01")}


# ---------------------------------------------------------------------------
# kernel parity
def test_rank_split_device_matches_host(ek, ctx):
    for name, v, n1 in kc.rank_split_cases() + [kc.rank_split_big_case()]:
        want = ek.rank_split(v, n1)
        got = ctx.rank_split_device(v, n1)
        assert np.array_equal(got, want), (name, int(got.sum()), n1)


@pytest.mark.parametrize("k", kc.METRIC_KS)
def test_kway_metrics_device_matches_host(ek, ctx, k):
    nodes, net_ptr, pins = kc.metrics_hypergraph()
    for part in kc.metrics_parts(nodes, k):
        assert ctx.kway_metrics(net_ptr, pins, part, k) == ek.kway_metrics_host(net_ptr, pins, part, k)
    assert ctx.kway_metrics(net_ptr, pins, np.zeros(nodes, np.int32), k) == (0, 0, 0)


def test_kway_metrics_ibm01(ek, ctx, hgrs):
    h = hgrs["ibm01"]
    net_ptr, pins = h.pins()
    rng = np.random.default_rng(5)
    for k in (2, 64, 65, 256):
        part = rng.integers(0, k, h.nodes).astype(np.int32)
        want = ek.kway_metrics_host(net_ptr, pins, part, k)
        assert want[0] > 0
        assert ctx.kway_metrics(net_ptr, pins, part, k) == want


# ---------------------------------------------------------------------------
# composition
def reference_recursion(ek, ctx, h, k, min_spectral=32):
    """ek_partition_kway restated with the public pieces: (part, fallbacks,
    the root bisection's KL result)."""
    part = np.full(h.nodes, -1, np.int32)
    info = {"fallbacks": 0, "root_kl": None}

    def rec(hg, ids, k, base):
        n = hg.nodes
        kl, kr = (k + 1) // 2, k // 2
        n1 = n * kr // k
        n0 = n - n1
        net_ptr, pins = hg.pins()
        edges = bool(np.any(np.diff(net_ptr) >= 2))
        spectral = edges and n >= min_spectral
        bits = None
        if spectral:
            ctx.spmv_setup_pins(hg)
            try:
                _, v, _ = ctx.lanczos_fiedler()
                bits = ek.rank_split(v, n1)
            except ek.EKError as e:
                if e.code != ek.EK_ENOCONV:
                    raise
                spectral = False
        if not spectral:
            info["fallbacks"] += 1
            bits = ek.rank_split(-np.arange(n, dtype=np.float64), n1)
            assert np.array_equal(bits, np.arange(n) >= n0)  # the first n0 nodes to side 0
        if edges:
            ctx.kl_graph_setup(hg.kl_graph())
            ctx.kl_nets_setup(net_ptr, pins)
            ctx.kl_set_partition_bits(bits)
            _, res = ctx.kl_run()
            if info["root_kl"] is None:
                info["root_kl"] = res
            sides = ctx.kl_sides(1)
        else:
            sides = bits
        for s, ks, bs in ((0, kl, base), (1, kr, base + kl)):
            sel = np.flatnonzero(sides == s)
            if ks == 1:
                part[ids[sel]] = bs
            else:
                sub, _ = hg.induce(sides == s)
                rec(sub, ids[sel], ks, bs)

    rec(h, np.arange(h.nodes), k, 0)
    return part, info["fallbacks"], info["root_kl"]


CASES = [("fract", 2, 32), ("fract", 3, 32), ("fract", 4, 32), ("fract", 8, 32), ("fract", 8, 64),
         ("ibm01", 2, 32), ("ibm01", 3, 32), ("ibm01", 4, 32)]


@pytest.mark.parametrize("name,k,min_spectral", CASES)
def test_partition_kway_equals_reference_recursion(ek, ctx, hgrs, name, k, min_spectral):
    h = hgrs[name]
    part, res = ctx.partition_kway(h, k, min_spectral=min_spectral)
    want, fallbacks, root_kl = reference_recursion(ek, ctx, h, k, min_spectral)
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    assert res["fallback_splits"] == fallbacks
    if min_spectral == 64:
        assert res["fallback_splits"] > 0  # fract's blocks of 37-38 nodes
    # properties
    assert np.array_equal(np.bincount(part, minlength=k), ek.kway_plan(h.nodes, k))
    assert set(part.tolist()) == set(range(k))
    assert res["part_min"] == h.nodes // k and res["part_max"] == -(-h.nodes // k)
    assert res["k"] == k and res["bisections"] == k - 1
    net_ptr, pins = h.pins()
    assert (res["cut_nets"], res["connectivity"], res["soed"]) == ek.kway_metrics_host(net_ptr, pins, part, k)
    if k == 2:  # the bipartition's own integer net cut (k_net_cut) of the same bisection
        assert res["cut_nets"] == root_kl["net_cut_best"]
        assert res["connectivity"] == res["cut_nets"] and res["soed"] == 2 * res["cut_nets"]
        assert res["kl_swaps"] == root_kl["iterations"]


def test_partition_kway_min_spectral_below_lanczos_minimum(ek, ctx, hgrs):
    """fract at k = 64 with min_spectral = 1: the last level bisects blocks of 4
    and 5 nodes (every part keeps >= 2 nodes, so no smaller block is bisected).
    ek_lanczos_fiedler takes them deflated (ncv = 2 > nev = 1) and refuses
    them undeflated (ncv = 2 <= nev = 2) with EK_EINVAL, which is no
    EK_ENOCONV and ended the whole call; such blocks now take the index split.
    Either way: a valid partition with the planned sizes."""
    h = hgrs["fract"]
    k = 64
    net_ptr, pins = h.pins()
    for lanczos in (None, {"deflate": 0}):
        part, res = ctx.partition_kway(h, k, min_spectral=1, lanczos=lanczos)
        assert np.array_equal(np.bincount(part, minlength=k), ek.kway_plan(h.nodes, k))
        assert part.min() == 0 and part.max() == k - 1
        assert res["part_min"] == h.nodes // k and res["part_max"] == -(-h.nodes // k)
        assert res["k"] == k and res["bisections"] == k - 1
        assert (res["cut_nets"], res["connectivity"], res["soed"]) == ek.kway_metrics_host(net_ptr, pins, part, k)
        if lanczos:
            assert res["fallback_splits"] > 0  # the 4- and 5-node blocks
            assert np.array_equal(part, ctx.partition_kway(h, k, min_spectral=6, lanczos=lanczos)[0])
        else:
            # min_spectral 1..3 act as 4, the smallest block the deflated solver takes
            assert np.array_equal(part, ctx.partition_kway(h, k, min_spectral=4)[0])


# ---------------------------------------------------------------------------
# file form and CLI
def _gkl2(*args, cwd):
    return subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=cwd, capture_output=True,
                          text=True, timeout=120)


def test_partition_kway_file_and_cli(ek, ctx, tmp_path):
    fract = circuit_path("fract")
    lib_dir, cli_dir = tmp_path / "lib", tmp_path / "cli"
    cli_dir.mkdir()
    part, res = ctx.partition_kway_file(fract, 4, out_dir=str(lib_dir))
    text = (lib_dir / "results" / "fract.hgr.part.4").read_text()
    assert text.endswith("\n") and [int(x) for x in text.split()] == part.tolist() and len(part) == 149
    assert not any(p.name != "fract.hgr.part.4" for p in (lib_dir / "results").iterdir())
    r = _gkl2(fract, "-EIG", "--k", "4", cwd=cli_dir)
    assert r.returncode == 0, r.stderr
    assert (cli_dir / "results" / "fract.hgr.part.4").read_text() == text
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("k-way:")]
    assert len(line) == 1 and f"cut nets {res['cut_nets']}," in line[0] and "part sizes 37..38" in line[0]


def test_cli_without_k_is_the_bipartition(ek, ctx, tmp_path):
    fract = circuit_path("fract")
    lib_dir, cli_dir = tmp_path / "lib", tmp_path / "cli"
    cli_dir.mkdir()
    ctx.solve_file(fract, out_dir=str(lib_dir))
    r = _gkl2(fract, "-EIG", cwd=cli_dir)
    assert r.returncode == 0, r.stderr
    names = sorted(p.name for p in (cli_dir / "results").iterdir())
    assert names == ["fract.hgr_KL_CutSize_EIG_output.txt"]
    assert (cli_dir / "results" / names[0]).read_bytes() == (lib_dir / "results" / names[0]).read_bytes()
    assert "k-way" not in r.stdout


# ---------------------------------------------------------------------------
# state
def test_kway_leaves_no_state_behind(ek, ctx, hgrs):
    h = hgrs["fract"]
    a, ra = ctx.partition_kway(h, 3)
    b, rb = ctx.partition_kway(h, 3)
    assert np.array_equal(a, b)
    assert (ra["matvecs"], ra["kl_swaps"], ra["cut_nets"]) == (rb["matvecs"], rb["kl_swaps"], rb["cut_nets"])
    ibm01 = circuit_path("ibm01")
    res, log = ctx.solve_file(ibm01, write_results=False, log_cap=8192)
    fresh = ek.Context(0)
    try:
        res0, log0 = fresh.solve_file(ibm01, write_results=False, log_cap=8192)
    finally:
        fresh.close()
    swap_fields_equal(log, log0)
    assert res["kl"]["net_cut_best"] == res0["kl"]["net_cut_best"] and res["lambda"] == res0["lambda"]


def test_kway_argument_and_rank_guards(ek, ctx, hgrs):
    h = hgrs["fract"]
    for k in (1, 257, 75):  # 149 nodes: at most 74 parts of >= 2
        with pytest.raises(ek.EKError) as e:
            ctx.partition_kway(h, k)
        assert e.value.code == ek.EK_EINVAL
    # a 1-rank host-staged communicator is a single context: allowed
    one = ek.Context(0)
    try:
        one.comm_init_host(1, 0, lambda send: send, lambda buf: None)
        part, _ = one.partition_kway(h, 2)
        assert np.array_equal(part, ctx.partition_kway(h, 2)[0])
        # rank 0 of 2: refused before anything is exchanged (the callbacks never run)
        def never(*_):
            raise AssertionError("a collective ran")
        one.comm_init_host(2, 0, never, never)
        with pytest.raises(ek.EKError) as e:
            one.partition_kway(h, 2)
        assert e.value.code == ek.EK_ESTATE
    finally:
        one.close()
