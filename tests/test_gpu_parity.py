"""GPU parity tests: the HIP path (through the C-ABI) against the oracle and the
reference's golden outputs.  Run on an MI355X: pytest -m gpu."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import (CIRCUITS, NET_CUTS, SWAP_MD5, PKG_DIR, circuit_path, compare_results_text, eig_path,
                      ref_results_path)
from spmv_cases import sequential_rows as _sequential_rows  # the left-to-right row sum, shared with the shape tests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def _swap_fields_equal(a, b):
    for f in ("iter", "node_left", "node_right"):
        assert np.array_equal(a[f], b[f]), f
    for f in ("max_gain", "min_gain", "gain", "cut"):  # bit-exact fp32
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f


# ---------------------------------------------------------------- SpMV seam
@pytest.mark.parametrize("which", ["ibm01", "industry2", "syn0.25"])
def test_spmv_matches_oracle(ek, oracle, ctx, which):
    if which.startswith("syn"):
        h = ek.Hypergraph.generate(float(which[3:]), 7)
        net_ptr, pins = h.pins()
        g = oracle.Graph.from_pins(h.nodes, net_ptr, pins)
    else:
        h = ek.Hypergraph.read(circuit_path(which))
        g = oracle.Graph.read(circuit_path(which))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(h.nodes)
    y = ctx.spmv_host(x)
    y_ref = g.spmv(x)
    # per-row bound: |y - y_ref| <= 1e-14 * sum_j |L_ij x_j| (fp64, different summation order)
    absrow = np.add.reduceat(np.abs(L.val * x[L.col]), L.rowptr[:-1]) if L.nnz else np.zeros(h.nodes)
    assert np.all(np.abs(y - y_ref) <= 1e-14 * absrow + 1e-300)
    # property at full size: L 1 = 0 exactly up to rounding
    y1 = ctx.spmv_host(np.ones(h.nodes))
    assert np.abs(y1).max() <= 1e-12


@pytest.mark.parametrize("which", ["ibm01", "industry2", "syn1"])
def test_spmv_dictionary_form_bit_identical(ek, ctx, monkeypatch, which):
    """The dictionary-coded entries (32-bit col|code words + exact fp64 table,
    per-block segments; industry2's 1,634 rows longer than a segment go to the
    overflow area) must give the plain CSR kernel's products in the same
    order: y and the whole Lanczos run bit for bit."""
    h = ek.Hypergraph.generate(1.0, 1) if which == "syn1" else ek.Hypergraph.read(circuit_path(which))
    L = h.laplacian()
    x = np.random.default_rng(11).standard_normal(h.nodes)
    out = {}
    for plain in (False, True):
        if plain:
            monkeypatch.setenv("EK_SPMV_PLAIN", "1")
        else:
            monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
        ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
        packed, stored = ctx.spmv_format()
        assert packed == (not plain)
        assert stored < ctx.spmv_bytes() if packed else stored == ctx.spmv_bytes()
        y = ctx.spmv_host(x)
        lam, v, st = ctx.lanczos_fiedler() if which != "syn1" else (0.0, np.zeros(1), {"matvecs": 0})
        out[plain] = (y, lam, v, st["matvecs"])
    monkeypatch.delenv("EK_SPMV_PLAIN", raising=False)
    assert np.array_equal(out[False][0].view(np.uint64), out[True][0].view(np.uint64))
    assert out[False][1] == out[True][1] and out[False][3] == out[True][3]
    assert np.array_equal(out[False][2], out[True][2])


@pytest.mark.parametrize("which", ["ibm01", "industry2", "syn0.25"])
@pytest.mark.parametrize("path", ["host_csr", "pins"])
def test_spmv_panel_form_is_the_sequential_row_sum(ek, ctx, monkeypatch, which, path):
    """The column-panel SpMV (kernels_panel.hip; chosen by default once x
    outgrows an XCD's L2, forced here on small graphs): each row summed
    strictly left to right in column order, bit for bit, through both setup
    paths (host CSR, device build from the pins)."""
    h = ek.Hypergraph.generate(0.25, 3) if which == "syn0.25" else ek.Hypergraph.read(circuit_path(which))
    L = h.laplacian()
    monkeypatch.setenv("EK_SPMV_PANEL", "1")
    if path == "pins":
        assert ctx.spmv_setup_pins(h) is True
    else:
        ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    x = np.random.default_rng(3).standard_normal(h.nodes)
    y = ctx.spmv_host(x)
    assert np.array_equal(y.view(np.uint64), _sequential_rows(L, x).view(np.uint64))


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2"])
def test_spmv_panel_form_lanczos_golden(ek, ctx, monkeypatch, name):
    monkeypatch.setenv("EK_SPMV_PANEL", "1")
    h = ek.Hypergraph.read(circuit_path(name))
    assert ctx.spmv_setup_pins(h) is True
    lam, v, st = ctx.lanczos_fiedler()
    assert st["converged"] and st["residual"] < 1e-9
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
    _fiedler_parity(name, lam, v, lam_ref, med_ref, bits_ref, v_ref, ek)


def test_spmv_dictionary_overflow_falls_back(ek, ctx):
    """More distinct values than the code bits hold -> plain CSR, same result."""
    n = 1 << 20  # colbits 20 -> 4096 codes; 6000 distinct values do not fit
    rng = np.random.default_rng(5)
    deg = 4
    rowptr = (np.arange(n + 1) * deg).astype(np.int32)
    col = rng.integers(0, n, n * deg).astype(np.int32)
    val = np.round(rng.integers(1, 6001, n * deg) * 1e-3, 3)
    ctx.spmv_setup(n, 0, rowptr, col, val)
    assert ctx.spmv_format()[0] is False
    x = rng.standard_normal(n)
    y = ctx.spmv_host(x)
    ref = np.add.reduceat(val * x[col], rowptr[:-1])
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


# ------------------------------------------------------- KL, bit-exact vs cKL
@pytest.mark.parametrize("name", CIRCUITS)
def test_kl_bitexact_golden(ek, oracle, ctx, name):
    h = ek.Hypergraph.read(circuit_path(name))
    G = h.kl_graph()
    lam, med, bits, v, o0, o1 = ek.eig_read(eig_path(name), h.nodes)
    ctx.kl_graph_setup(G)
    ctx.kl_nets_setup(*h.pins())
    ctx.kl_set_partition(o0, o1)
    log, res = ctx.kl_run()
    # oracle restatement: identical swap sequence and fp32 bits
    g = oracle.Graph.read(circuit_path(name))
    olog, ores = g.kl(o0, o1)
    assert res["iterations"] == ores["iterations"] == NET_CUTS[name]["iterations"]
    _swap_fields_equal(log, olog)
    assert np.float32(res["initial_cut"]).view(np.uint32) == np.float32(ores["initial_cut"]).view(np.uint32)
    assert res["best_iter"] == NET_CUTS[name]["best_iter"]
    assert res["net_cut_best"] == NET_CUTS[name]["net_cut_best"]
    assert res["net_cut_final"] == NET_CUTS[name]["net_cut_final"]
    # reference swap-log md5 and the reference cKL results file
    assert hashlib.md5(oracle.swap_log_text(log).encode()).hexdigest().startswith(SWAP_MD5[name])
    compare_results_text(oracle.format_results(log, res["initial_cut"]), open(ref_results_path(name)).read())
    # sides: best prefix replay and final
    sb = ctx.kl_sides(1)
    assert g.net_cut(sb) == NET_CUTS[name]["net_cut_best"]
    # run again on the resident graph: identical (state fully reset, deterministic)
    log2, res2 = ctx.kl_run()
    _swap_fields_equal(log, log2)


@pytest.mark.parametrize("mult,seed", [(0.05, 11), (0.25, 3)])
def test_kl_random_init_synthetic(ek, oracle, ctx, mult, seed):
    h = ek.Hypergraph.generate(mult, seed)
    n = h.nodes
    perm = np.random.default_rng(seed).permutation(n).astype(np.int32)  # seeded shuffle (cKL.cpp:176-192)
    o0, o1 = perm[: n // 2], perm[n // 2:]
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(*h.pins())
    ctx.kl_set_partition(o0, o1)
    log, res = ctx.kl_run()
    g = oracle.Graph.from_pins(n, *h.pins())
    olog, ores = g.kl(o0, o1)
    assert res["iterations"] == ores["iterations"] > 0
    _swap_fields_equal(log, olog)
    for k in ("best_iter", "net_cut_best", "net_cut_final", "net_cut_initial"):
        assert res[k] == ores[k], k


@pytest.mark.parametrize("mode", ["EK_KL_GLOBAL_STATE", "EK_KL_NOSEG", "EK_KL_NOSEGC", "EK_KL_PIPE",
                                  "EK_KL_PIPE+EK_KL_NOSEGC", "EK_KL_GBITS", "EK_KL_GBITS+EK_KL_NOSEGC",
                                  "EK_KL_FIXLDS=0", "EK_KL_FIXLDS=0+EK_KL_NOSEGC"])
@pytest.mark.parametrize("name", ["ibm01", "industry2"])
def test_kl_fallback_paths_bitexact(ek, oracle, ctx, monkeypatch, name, mode):
    # the global-state loop (graphs whose on-chip state does not fit LDS), the
    # LDS loop without inline neighbour rows (not enough memory for them) and
    # the plain (not weight-coded) inline rows (too many distinct weights) are
    # forced here on shipped circuits; industry2 has rows of 910 entries.
    # EK_KL_PIPE: the overlapped schedule (k_kl_swap_pipe, not the default:
    # profiles/r06/kl), coded and plain inline rows.  EK_KL_GBITS: the on-chip
    # loop with its side / locked bitmaps in global memory (the form graphs
    # above ~500k nodes take), coded and plain inline rows.  EK_KL_FIXLDS=0:
    # the carved (not fixed) LDS layout, the default from 131,073 positions a list
    for m in mode.split("+"):
        name_, _, value = m.partition("=")
        monkeypatch.setenv(name_, value or "1")
    h = ek.Hypergraph.read(circuit_path(name))
    _, _, _, _, o0, o1 = ek.eig_read(eig_path(name), h.nodes)
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(*h.pins())
    ctx.kl_set_partition(o0, o1)
    log, res = ctx.kl_run()
    olog, ores = oracle.Graph.read(circuit_path(name)).kl(o0, o1)
    assert res["iterations"] == ores["iterations"] == NET_CUTS[name]["iterations"]
    _swap_fields_equal(log, olog)
    assert res["net_cut_best"] == NET_CUTS[name]["net_cut_best"]


@pytest.mark.parametrize("name", ["fract", "ibm01"])
def test_kl_partition_from_bits(ek, oracle, ctx, name):
    # ek_kl_set_partition_bits is the -EIG branch of shuffleSparceMatrix
    # (cKL.cpp:155-174): the same lists as the EIG file's line order
    h = ek.Hypergraph.read(circuit_path(name))
    _, _, bits, _, o0, o1 = ek.eig_read(eig_path(name), h.nodes)
    assert np.array_equal(np.flatnonzero(bits == 0), o0) and np.array_equal(np.flatnonzero(bits == 1), o1)
    ctx.kl_graph_setup(h.kl_graph())
    ctx.kl_nets_setup(*h.pins())
    ctx.kl_set_partition_bits(bits)
    log, res = ctx.kl_run()
    olog, ores = oracle.Graph.read(circuit_path(name)).kl(o0, o1)
    assert res["iterations"] == ores["iterations"] == NET_CUTS[name]["iterations"]
    _swap_fields_equal(log, olog)
    with pytest.raises(ek.EKError):
        ctx.kl_set_partition_bits(np.full(h.nodes, 2, np.uint8))


def test_kl_edge_cases(ek, oracle, ctx):
    # tiny graph with repeated pins in a net, a 1-pin net, an empty net and an isolated node
    net_ptr = np.array([0, 3, 4, 4, 6, 9, 11], np.int64)
    pins = np.array([0, 1, 1, 2, 3, 4, 5, 6, 0, 6, 7], np.int32)
    h = ek.Hypergraph.from_pins(9, net_ptr, pins)
    g = oracle.Graph.from_pins(9, net_ptr, pins)
    G = h.kl_graph()
    rp, col, w, nf = g.kl_csr()
    assert np.array_equal(rp, G.rowptr) and np.array_equal(col, G.col)
    for o0, o1 in [([0, 1, 2, 3], [4, 5, 6, 7, 8]), ([8, 2, 4, 6, 1], [0, 3, 5, 7])]:
        ctx.kl_graph_setup(G)
        ctx.kl_nets_setup(net_ptr, pins)
        ctx.kl_set_partition(o0, o1)
        log, res = ctx.kl_run()
        olog, ores = g.kl(np.array(o0), np.array(o1))
        assert res["iterations"] == ores["iterations"]
        _swap_fields_equal(log, olog)
        assert res["net_cut_best"] == ores["net_cut_best"]


# --------------------------------------------------- Lanczos / Fiedler vector
def _fiedler_parity(name, lam, v, lam_ref, med_ref, bits_ref, v_ref, ek):
    v = v * np.sign(v @ v_ref)
    med, bits = ek.median_split(v)
    assert abs(lam - lam_ref) <= 1e-10, (lam, lam_ref)
    assert np.abs(v - v_ref).max() <= 1e-8
    mask = np.abs(v_ref - med_ref) > 1e-8
    assert np.array_equal(bits[mask], bits_ref[mask])


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2"])
@pytest.mark.parametrize("deflate,reorth", [(True, 1), (False, 1), (True, 2), (False, 2)])
def test_lanczos_golden(ek, ctx, name, deflate, reorth):
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam, v, st = ctx.lanczos_fiedler(deflate=deflate, reorth=reorth)
    assert st["converged"] and st["residual"] < 1e-9
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
    _fiedler_parity(name, lam, v, lam_ref, med_ref, bits_ref, v_ref, ek)
    assert abs(np.linalg.norm(v) - 1) < 1e-12 and abs(v.sum()) < 1e-8


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2", "ibm10"])
def test_lanczos_partial_reorth_vs_full(ek, ctx, monkeypatch, name):
    """Partial reorthogonalisation (reorth=3, the default; k_pro: Simon's
    omega recurrence) against the full Gram-Schmidt pass on every step
    (reorth=1, Spectra's rule, cEIG.cpp:195-198): fewer projected steps, the
    basis orthonormal to 1e-8 at every restart (max |[V u0]^T [V u0] - I|,
    EK_LANCZOS_ORTHO), lambda within 1e-10 of the full run, the matvec count
    within 5 %, and both held to the reference's pre_saved_EIG tolerances
    (ibm10's golden is unconverged: residual and the converged lambda)."""
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    monkeypatch.setenv("EK_LANCZOS_ORTHO", "1")
    lam_p, v_p, st_p = ctx.lanczos_fiedler()
    lam_f, v_f, st_f = ctx.lanczos_fiedler(reorth=1)
    print(name, {k: st_p[k] for k in ("matvecs", "projected_steps", "restarts", "ortho_max", "residual")},
          {k: st_f[k] for k in ("matvecs", "projected_steps", "ortho_max")})
    assert st_p["converged"] and st_p["residual"] < 1e-9 and st_f["residual"] < 1e-9
    assert st_f["projected_steps"] == st_f["matvecs"]
    assert st_p["projected_steps"] < st_p["matvecs"]
    assert st_p["ortho_max"] <= 1e-8 and st_f["ortho_max"] <= 1e-12
    assert abs(lam_p - lam_f) <= 1e-10
    assert st_p["matvecs"] <= 1.05 * st_f["matvecs"] + 8
    v_f = v_f * np.sign(v_p @ v_f)
    assert np.abs(v_p - v_f).max() <= 1e-8
    if name != "ibm10":
        lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
        _fiedler_parity(name, lam_p, v_p, lam_ref, med_ref, bits_ref, v_ref, ek)
    else:
        assert abs(lam_p - 0.0185035852) < 1e-9


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2", "ibm10"])
def test_lanczos_midcycle_check_same_split_as_end_of_cycle(ek, ctx, name):
    """The mid-cycle convergence test (check_every > 0) may stop a cycle early
    and take the Ritz pair from a j < ncv projection; check_every=0 is
    Spectra's end-of-cycle-only test.  Both must give the same median split
    wherever the entry is not within 1e-8 of the median, and both must meet
    the golden's tolerances (ibm10's golden is unconverged: residual only)."""
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam_a, v_a, st_a = ctx.lanczos_fiedler(check_every=8)
    lam_b, v_b, st_b = ctx.lanczos_fiedler(check_every=0)
    assert st_a["converged"] and st_b["converged"]
    assert st_a["residual"] < 1e-9 and st_b["residual"] < 1e-9
    assert abs(lam_a - lam_b) <= 1e-10
    v_b = v_b * np.sign(v_a @ v_b)
    assert np.abs(v_a - v_b).max() <= 1e-8
    med_a, bits_a = ek.median_split(v_a)
    med_b, bits_b = ek.median_split(v_b)
    mask = (np.abs(v_a - med_a) > 1e-8) & (np.abs(v_b - med_b) > 1e-8)
    assert np.array_equal(bits_a[mask], bits_b[mask])
    if name != "ibm10":
        lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
        _fiedler_parity(name, lam_b, v_b, lam_ref, med_ref, bits_ref, v_ref, ek)


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2", "ibm10"])
def test_lanczos_restart_floor_same_split_as_spectra_rule(ek, ctx, name):
    """The implicit restart keeps at least ncv/5 vectors (keep_min default)
    instead of Spectra's nev_adjusted alone (keep_min=0, which keeps 2-4 of
    100 on these Laplacians): a different restart sequence, the same Fiedler
    pair within the goldens' tolerances and the same median split."""
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam_a, v_a, st_a = ctx.lanczos_fiedler()
    lam_b, v_b, st_b = ctx.lanczos_fiedler(keep_min=0)
    assert st_a["converged"] and st_b["converged"] and st_a["residual"] < 1e-9 and st_b["residual"] < 1e-9
    assert abs(lam_a - lam_b) <= 1e-10
    v_b = v_b * np.sign(v_a @ v_b)
    assert np.abs(v_a - v_b).max() <= 1e-8
    med_a, bits_a = ek.median_split(v_a)
    med_b, bits_b = ek.median_split(v_b)
    mask = (np.abs(v_a - med_a) > 1e-8) & (np.abs(v_b - med_b) > 1e-8)
    assert np.array_equal(bits_a[mask], bits_b[mask])
    if name != "ibm10":
        lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
        for lam, v in ((lam_a, v_a), (lam_b, v_b)):
            _fiedler_parity(name, lam, v * np.sign(v @ v_ref), lam_ref, med_ref, bits_ref, v_ref, ek)


@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2"])
@pytest.mark.parametrize("deflate", [True, False])
def test_lanczos_basis32_update_golden(ek, ctx, name, deflate):
    """The update f = f' - V h reading the basis's fp32 shadow (basis32, the
    default) only where sum|h| <= 2^-29 ||f'||, so the shadow's rounding stays
    below the fp64 update's own: held to the reference's Fiedler tolerances
    like the fp64-basis run, and every regular step took the shadow."""
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    # (reorth=1: every step projects, h is the O(eps) loss of orthogonality;
    # under partial reorthogonalisation the projecting steps carry a loss of
    # up to the threshold and mostly take the fp64 basis)
    lam_a, v_a, st_a = ctx.lanczos_fiedler(deflate=deflate, basis32=True, reorth=1)
    lam_b, v_b, st_b = ctx.lanczos_fiedler(deflate=deflate, basis32=False, reorth=1)
    assert st_a["converged"] and st_a["residual"] < 1e-9 and st_b["residual"] < 1e-9
    assert st_a["update32_steps"] == st_a["matvecs"] and st_b["update32_steps"] == 0
    assert st_a["update32_fallbacks"] == 0, st_a
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), h.nodes)
    for lam, v in ((lam_a, v_a), (lam_b, v_b)):
        _fiedler_parity(name, lam, v * np.sign(v @ v_ref), lam_ref, med_ref, bits_ref, v_ref, ek)
    assert abs(lam_a - lam_b) <= 1e-11 and abs(st_a["matvecs"] - st_b["matvecs"]) <= 8 + 0.05 * st_b["matvecs"]


@pytest.mark.parametrize("which", ["syn0.25", "syn2", "syn1"])
def test_lanczos_basis32_synthetic_breakdowns(ek, ctx, which):
    """Disconnected synthetics (injected vectors, collapsed restart residuals):
    the shadow update converges to a null vector with the fp64 run's residual
    bar.  The accuracy test falls back to the fp64 basis only on the rare
    steps whose f' cancelled to near zero at an invariant subspace (a
    breakdown: sum|h| ~ eps ||w|| then exceeds 2^-29 ||f'||)."""
    mult, seed = {"syn0.25": (0.25, 3), "syn2": (2.0, 2), "syn1": (1.0, 1)}[which]
    h = ek.Hypergraph.generate(mult, seed)
    ctx.spmv_setup_pins(h)
    lam, v, st = ctx.lanczos_fiedler(reorth=1)
    assert st["converged"] and st["residual"] < 1e-8 and abs(lam) < 1e-8
    assert np.all(np.isfinite(v)) and abs(np.linalg.norm(v) - 1) < 1e-10
    assert st["update32_steps"] == st["matvecs"] and st["update32_fallbacks"] <= 0.01 * st["matvecs"], st
    # the default, partial reorthogonalisation, through the same breakdowns
    lam, v, st = ctx.lanczos_fiedler()
    assert st["converged"] and st["residual"] < 1e-8 and abs(lam) < 1e-8
    assert np.all(np.isfinite(v)) and abs(np.linalg.norm(v) - 1) < 1e-10
    assert 0 < st["projected_steps"] < st["matvecs"], st


@pytest.mark.parametrize("which", ["ibm01", "syn0.25", "syn2"])
@pytest.mark.parametrize("switch", ["EK_LANCZOS_TT=0", "EK_ALPHA_LAST=1", "plain:EK_ALPHA_LAST=1", "EK_UPD_RED=0",
                                    "EK_UPD_RED=1",
                                    "EK_UPD_RED=2", "EK_V_NT=1", "pro:EK_UPD_RED=0", "pro:EK_UPD_RED=2",
                                    "pro:EK_V_NT=1", "pro:EK_PRO_INLAUNCH=0", "pro:EK_PRO_MERGE=0",
                                    "pro:EK_PRO_CGW=0", "pro:EK_PRO_CGW=1", "pro:EK_VQ_IB=8",
                                    "pro:EK_CHK_FENCE=0", "pro:EK_CHK_POLL=0",
                                    "pro:EK_CHK_FOLD=1"])
def test_lanczos_device_paths_bit_identical(ek, tmp_path, which, switch):
    """Device-side restructurings give the bits of the forms they replace:
    * the single-GPU step without the three-term launch (alpha reduced by the
      SpMV's last block, f' formed inside the projection) vs EK_LANCZOS_TT=0;
    * alpha re-reduced by every projection workgroup (the default) vs by
      the SpMV's last block (EK_ALPHA_LAST=1);
    * the projection's column sums reduced by its last workgroup per column
      group (EK_UPD_RED=2, the default up to 256 row blocks), by every update
      workgroup (1) or by a k_reduce_cols launch (0, the default above);
    * the basis passes' non-temporal loads (EK_V_NT=1; the default above 768
      MB of basis) against plain ones;
    * the partial reorthogonalisation's decision taken inside the projection
      launch (the default with the projection's hand-off) against the k_pro
      launch (EK_PRO_INLAUNCH=0), and the update inside that launch (the
      default) against its own launch (EK_PRO_MERGE=0);
    * that launch's projection workgroups walking several column groups
      each (the default: ~850 projection workgroups, at least 3 per row
      block; EK_PRO_CGW=1: one per row block walking them all) against one
      workgroup per (row block, column group) tile (EK_PRO_CGW=0);
    * the restart's V Q with 8 basis rows in flight per trip (EK_VQ_IB=8)
      against 16, the mid-cycle check's chunk event with a system-scope
      fence (EK_CHK_FENCE=0) against the device-scope one, and that event
      path (EK_CHK_POLL=0) against the default polled completion word, and
      that word's copy folded into block 0 of the chunk's last SpMV
      (EK_CHK_FOLD=1, graph replays included) against its own launch.
    syn0.25 goes through breakdowns (injected vectors, beta = 0) and restarts,
    syn2 through restarts whose residual collapses.  These run the full
    reorthogonalisation (EK_REORTH=1); "plain:" runs both sides on the plain
    CSR SpMV (EK_SPMV_PLAIN=1, whose launcher must keep the alpha hand-off
    when the caller asks for it); "pro:" switches hold the partial one
    (the default) to the same rule: the skipped steps' paths (the projection's
    norm-only hand-off or its zeroed partials under k_reduce_cols, the
    update's early exit) give the same bits whichever form runs."""
    import subprocess
    import sys
    gen = {"ibm01": "ek.Hypergraph.read(circuit_path('ibm01'))", "syn0.25": "ek.Hypergraph.generate(0.25, 3)",
           "syn2": "ek.Hypergraph.generate(2.0, 2)"}[which]
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); from conftest import load_package, circuit_path; "
        "ek = load_package(); h = %s; c = ek.Context(0); c.spmv_setup_pins(h); lam, v, st = c.lanczos_fiedler(); "
        "np.save(sys.argv[1], np.concatenate([[lam, st['matvecs'], st['residual']], v]))"
    ) % (os.path.dirname(os.path.abspath(__file__)), gen)
    env = dict(os.environ)
    if switch.startswith("pro:"):
        switch = switch[4:]
        env["EK_REORTH"] = "3"
    else:
        env["EK_REORTH"] = "1"
    if switch.startswith("plain:"):
        switch = switch[6:]
        env["EK_SPMV_PLAIN"] = "1"
    a, b = str(tmp_path / "new.npy"), str(tmp_path / "old.npy")
    subprocess.run([sys.executable, "-c", code, a], check=True, timeout=180, env=env)
    k, v = switch.split("=")
    env[k] = v
    subprocess.run([sys.executable, "-c", code, b], check=True, timeout=180, env=env)
    x, y = np.load(a), np.load(b)
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert x[2] < 1e-8


@pytest.mark.parametrize("which", ["ibm01", "headline"])
def test_lanczos_inlaunch_waits_dispatch_order_free(ek, tmp_path, which):
    """VERDICT r5 next-6.  The in-launch waits of the partially
    reorthogonalised step (kernels_lanczos.hip gemvt_body, PROI): the
    projection's column groups and the merged update's workgroups poll the
    decider's words, the update's workgroups wait for the projection's done
    counter.  Each waits on a job of lower logical index.  Such a launch is
    free of any dispatch-order assumption when its whole grid is resident at
    once (the default sizes the workgroups per row block so that it is: the
    headline's 8 -> 2), and otherwise takes tickets: logical indices handed
    out in arrival order per residue class.  Here the physical index is
    reversed (EK_DISPATCH_REVERSE=1: job 0 would be the LAST workgroup
    dispatched), in the default form, with 8 workgroups per row block (a
    ~2,100-workgroup grid, twice what is resident, so its launches take
    tickets) and with tickets on every launch; the solve must give the bits of
    the plain launch every time, and so must the launch without tickets
    (EK_PRO_TICKETS=0: logical index = blockIdx)."""
    import subprocess
    import sys
    gen = {"ibm01": "ek.Hypergraph.read(circuit_path('ibm01'))",
           "headline": "ek.Hypergraph.generate(1.15, 1).largest_component()[0]"}[which]
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); from conftest import load_package, circuit_path; "
        "ek = load_package(); h = %s; c = ek.Context(0); c.spmv_setup_pins(h); lam, v, st = c.lanczos_fiedler(); "
        "np.save(sys.argv[1], np.concatenate([[lam, st['matvecs'], st['residual'], st['projected_steps']], v]))"
    ) % (os.path.dirname(os.path.abspath(__file__)), gen)
    out = {}
    rev = {"EK_DISPATCH_REVERSE": "1"}
    for name, extra in (("plain", {}), ("reversed", rev), ("reversed_cgw8", dict(rev, EK_PRO_CGW="8")),
                        ("reversed_tickets", dict(rev, EK_PRO_TICKETS="1")), ("no_tickets", {"EK_PRO_TICKETS": "0"})):
        env = dict(os.environ, **extra)
        f = str(tmp_path / f"{name}.npy")
        subprocess.run([sys.executable, "-c", code, f], check=True, timeout=180, env=env)
        out[name] = np.load(f)
    x = out["plain"]
    assert x[2] < 1e-8 and 0 < x[3] < x[1]
    for name in out:
        assert np.array_equal(out[name].view(np.uint64), x.view(np.uint64)), name


@pytest.mark.parametrize("which", ["ibm01", "syn0.25"])
def test_lanczos_pro_inlaunch_graph_replays(ek, tmp_path, which):
    """The in-launch decision (the projection's decider workgroup publishes
    to words the step's update re-arms) under the step-chunk graphs: three
    solves in one process (eager, captured, replayed) give the same bits, and
    the bits of eager launches with the k_pro launch (EK_PRO_INLAUNCH=0,
    EK_LANCZOS_GRAPH=0)."""
    import subprocess
    import sys
    gen = {"ibm01": "ek.Hypergraph.read(circuit_path('ibm01'))", "syn0.25": "ek.Hypergraph.generate(0.25, 3)"}[which]
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); from conftest import load_package, circuit_path; "
        "ek = load_package(); h = %s; c = ek.Context(0); c.spmv_setup_pins(h); out = []\n"
        "for _ in range(3):\n"
        "    lam, v, st = c.lanczos_fiedler(); out.append(np.concatenate([[lam, st['matvecs'], st['residual']], v]))\n"
        "np.save(sys.argv[1], np.stack(out))"
    ) % (os.path.dirname(os.path.abspath(__file__)), gen)
    env = dict(os.environ, EK_REORTH="3")
    a, b = str(tmp_path / "inl.npy"), str(tmp_path / "kpro.npy")
    subprocess.run([sys.executable, "-c", code, a], check=True, timeout=180, env=env)
    subprocess.run([sys.executable, "-c", code, b], check=True, timeout=180,
                   env=dict(env, EK_PRO_INLAUNCH="0", EK_LANCZOS_GRAPH="0"))
    x, y = np.load(a), np.load(b)
    for r in range(3):
        assert np.array_equal(x[r].view(np.uint64), y[0].view(np.uint64)), r
        assert np.array_equal(y[r].view(np.uint64), y[0].view(np.uint64)), r
    assert x[0][2] < 1e-8


@pytest.mark.parametrize("name", ["ibm01", "industry2", "fract"])
def test_lanczos_multirank_step_sequence_on_one_gpu(ek, tmp_path, name):
    """The step sequence the sharded path runs (ctx_lanczos.cpp factorize_mr: the
    rank's ||f||^2 through the all-gather slot, one sweep projecting w, v_i and
    v_{i-1}, alpha and the projection of f' from one all-reduce; the
    collectives are no-ops at one rank) against the fused single-GPU step:
    not the same rounding, so both are held to the reference's Fiedler
    tolerances and to each other's split."""
    import subprocess
    import sys
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); from conftest import load_package, circuit_path; "
        "ek = load_package(); h = ek.Hypergraph.read(circuit_path(%r)); L = h.laplacian(); "
        "c = ek.Context(0); c.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val); lam, v, st = c.lanczos_fiedler(); "
        "np.save(sys.argv[1], np.concatenate([[lam, st['matvecs'], st['residual']], v]))"
    ) % (os.path.dirname(os.path.abspath(__file__)), name)
    env = dict(os.environ)
    a, b = str(tmp_path / "fused.npy"), str(tmp_path / "unfused.npy")
    subprocess.run([sys.executable, "-c", code, a], check=True, timeout=120, env=env)
    env["EK_LANCZOS_UNFUSED"] = "1"
    subprocess.run([sys.executable, "-c", code, b], check=True, timeout=120, env=env)
    x, y = np.load(a), np.load(b)
    assert x[2] < 1e-9 and y[2] < 1e-9  # residuals
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), len(x) - 3)
    for z in (x, y):
        _fiedler_parity(name, z[0], z[3:], lam_ref, med_ref, bits_ref, v_ref, ek)
    assert abs(x[0] - y[0]) <= 1e-10 and abs(x[1] - y[1]) <= 0.1 * x[1]  # matvec counts within 10 %


def test_lanczos_ibm10_unconverged_golden(ek, ctx):
    # the shipped ibm10 golden is not converged (SURVEY §0 finding 5): pin by residual
    h = ek.Hypergraph.read(circuit_path("ibm10"))
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam, v, st = ctx.lanczos_fiedler()
    assert st["converged"] and st["residual"] < 1e-9
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path("ibm10"), h.nodes)
    assert abs(lam - 0.0185035852) < 1e-9  # converged value
    v = v * np.sign(v @ v_ref)
    _, bits = ek.median_split(v)
    assert (bits != bits_ref).sum() <= 100  # survey: a converged solver differs on 48 bits


def test_lanczos_synthetic_2x_restart_breakdown(ek, ctx):
    """2x synthetic (configs[3]): after an implicit restart the residual
    collapses to zero (the kept Ritz space is invariant); the run must
    continue from a fresh vector, not return a zero Ritz vector."""
    h = ek.Hypergraph.generate(2.0, 2)
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam, v, st = ctx.lanczos_fiedler()
    assert np.all(np.isfinite(v)) and abs(np.linalg.norm(v) - 1) < 1e-10  # host fp64 norm over 404K values
    assert st["converged"] and st["residual"] < 1e-8 and abs(lam) < 1e-8
    _, bits = ek.median_split(v)
    assert 0 < int(bits.sum()) < h.nodes


def test_lanczos_deterministic_and_synthetic(ek, ctx):
    h = ek.Hypergraph.generate(0.25, 5)
    L = h.laplacian()
    ctx.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
    lam1, v1, st1 = ctx.lanczos_fiedler()
    lam2, v2, st2 = ctx.lanczos_fiedler()
    assert lam1 == lam2 and np.array_equal(v1, v2)  # bitwise reproducible
    assert st1["residual"] < 1e-8


# ------------------------------------------------------- drop-in executables
def _tool(name):
    return os.path.join(PKG_DIR, "build", "bin", name)


@pytest.mark.parametrize("tool", ["cKL", "gKL"])
@pytest.mark.parametrize("name", ["fract", "ibm01", "industry2"])
def test_cli_kl_eig_matches_reference(tmp_path, tool, name):
    os.makedirs(tmp_path / "circuit")
    os.makedirs(tmp_path / "pre_saved_EIG")
    shutil.copy(circuit_path(name), tmp_path / "circuit")
    shutil.copy(eig_path(name), tmp_path / "pre_saved_EIG")
    subprocess.run([_tool(tool), f"circuit/{name}.hgr", "-EIG"], cwd=tmp_path, check=True, capture_output=True,
                   timeout=120)
    out = tmp_path / "results" / f"{name}.hgr_KL_CutSize_EIG_output.txt"
    compare_results_text(out.read_text(), open(ref_results_path(name)).read())


def test_cli_eig_then_kl(tmp_path, ek):
    shutil.copy(circuit_path("ibm01"), tmp_path)
    r = subprocess.run([_tool("cEIG"), "ibm01.hgr"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = 12752
    lam, med, bits, v, _, _ = ek.eig_read(str(tmp_path / "pre_saved_EIG" / "ibm01.hgr_out.txt"), n)
    lam_r, med_r, bits_r, v_r, _, _ = ek.eig_read(eig_path("ibm01"), n)
    assert abs(lam - lam_r) < 1e-10
    if v @ v_r < 0:  # even n: the opposite sign complements every bit
        bits = 1 - bits
    assert np.array_equal(bits, bits_r)
    r = subprocess.run([_tool("cKL"), "ibm01.hgr", "-EIG"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    compare_results_text((tmp_path / "results" / "ibm01.hgr_KL_CutSize_EIG_output.txt").read_text(),
                         open(ref_results_path("ibm01")).read())
    # gKL2 -EIG: in-process GPU EIG then KL; ibm01 has even n so the sign cannot matter
    r = subprocess.run([_tool("gKL2"), "ibm01.hgr", "-EIG"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    compare_results_text((tmp_path / "results" / "ibm01.hgr_KL_CutSize_EIG_output.txt").read_text(),
                         open(ref_results_path("ibm01")).read())


def test_cli_sign_ref_odd_n(tmp_path, ek):
    # industry2 has odd n: KL needs the golden sign (--sign-ref) for bit parity
    shutil.copy(circuit_path("industry2"), tmp_path)
    ref = eig_path("industry2")
    r = subprocess.run([_tool("cEIG"), "industry2.hgr", "--sign-ref", ref], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([_tool("cKL"), "industry2.hgr", "-EIG"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    compare_results_text((tmp_path / "results" / "industry2.hgr_KL_CutSize_EIG_output.txt").read_text(),
                         open(ref_results_path("industry2")).read())


def test_cli_errors(tmp_path):
    r = subprocess.run([_tool("cKL"), "missing.hgr", "-EIG"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1
    r = subprocess.run([_tool("cEIG")], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage" in r.stderr
