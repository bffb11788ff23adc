"""The library's own sharded Lanczos with 2 ranks, on one GPU.

Two processes each open a context on GPU 0 and join a 2-rank exchange through
ek_comm_init_host: every collective of the sharded path goes through the
library's comm seam, staged through host memory and carried by
torch.distributed gloo.  Per Lanczos step that is ONE all-gather (every
rank's padded f slice with its ||f||^2 partial) and ONE all-reduce (the
projections of w, v_i, v_{i-1}); the callbacks count them.  RCCL, the
production backend, refuses two ranks on one device; the device code, the
nnz-balanced shard map (unequal slices, remapped columns), the step sequence
and the global-index restart vectors are the same.

Checks: the 2-rank Fiedler pair against the reference's pre_saved_EIG files
(ibm01, industry2; the SURVEY §8c tolerances), the 2-rank SpMV against the
1-rank one per row, the sharded solve_file (parse -> results file) against the
reference cKL results, a disconnected synthetic whose solve goes through
breakdowns and injected restart vectors on both ranks, and configs[4] — the
10x synthetic (2,019,200 nodes), rows built on the device per shard — against
the 1-rank solve."""
import os
import socket

import numpy as np
import pytest

from conftest import circuit_path, compare_results_text, eig_path, ref_results_path

pytestmark = pytest.mark.gpu
WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fiedler_ok(ek, name, lam, v):
    lam_ref, med_ref, bits_ref, v_ref, _, _ = ek.eig_read(eig_path(name), len(v))
    v = v * np.sign(v @ v_ref)
    _, bits = ek.median_split(v)
    mask = np.abs(v_ref - med_ref) > 1e-8
    return {"dlam": abs(lam - lam_ref), "dv": float(np.abs(v - v_ref).max()),
            "bits_equal": bool(np.array_equal(bits[mask], bits_ref[mask]))}


def _comm(ctx, rank, counts):
    import torch
    import torch.distributed as dist

    def allgather(x):
        counts["allgather"] += 1
        parts = [torch.empty(len(x), dtype=torch.float64) for _ in range(WORLD)]
        dist.all_gather(parts, torch.from_numpy(x))
        return torch.cat(parts).numpy()

    def allreduce(x):
        counts["allreduce"] += 1
        dist.all_reduce(torch.from_numpy(x))  # in place (shared memory)

    ctx.comm_init_host(WORLD, rank, allgather, allreduce)


def _worker(rank, port, tmp, out):
    import datetime
    import faulthandler
    import sys
    import torch
    import torch.distributed as dist
    faulthandler.enable()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=90))
    from conftest import load_package
    ek = load_package()
    res = {}
    try:
        ctx = ek.Context(0)
        counts = {"allgather": 0, "allreduce": 0}
        _comm(ctx, rank, counts)
        one = ek.Context(0)  # an unsharded context for the 1-rank comparison
        for name in ("ibm01", "industry2"):
            h = ek.Hypergraph.read(circuit_path(name))
            n = h.nodes
            off = ek.shard_map(h, WORLD)
            row0, nrows = int(off[rank]), int(off[rank + 1] - off[rank])
            S = h.laplacian_rows(row0, row0 + nrows)
            ctx.spmv_setup(n, row0, S.rowptr, S.col, S.val)
            r = {}
            # reorth 3 (the default: partial reorthogonalisation, two all-reduces
            # a step) and 1 (the full pass by linearity, one all-reduce a step)
            for reorth in (3, 1):
                c0 = dict(counts)
                lam, v, st = ctx.lanczos_fiedler(reorth=reorth)
                q = _fiedler_ok(ek, name, lam, v)
                q.update(converged=bool(st["converged"]), residual=st["residual"], matvecs=st["matvecs"],
                         restarts=st["restarts"], row0=row0, nrows=nrows, comm_ms=st["comm_ms"],
                         allgathers=counts["allgather"] - c0["allgather"],
                         allreduces=counts["allreduce"] - c0["allreduce"], stat_ag=st["allgathers"],
                         stat_ar=st["allreduces"], v_bytes=v.tobytes(), lam=lam, projected=st["projected_steps"],
                         ortho_max=st["ortho_max"])
                r[reorth] = q
            # the default once more with the basis's orthogonality measured at
            # every restart (EK_LANCZOS_ORTHO: extra collectives, not counted above)
            os.environ["EK_LANCZOS_ORTHO"] = "1"
            try:
                lam_o, v_o, st_o = ctx.lanczos_fiedler()
            finally:
                del os.environ["EK_LANCZOS_ORTHO"]
            r[3]["ortho_max"] = st_o["ortho_max"]
            r[3]["same_bits_with_ortho_check"] = bool(lam_o == r[3]["lam"] and v_o.tobytes() == r[3]["v_bytes"])
            r.update(row0=row0, nrows=nrows)
            # SpMV: this rank's rows vs the same rows of a 1-rank SpMV
            x = np.random.default_rng(7).standard_normal(n)
            y = ctx.spmv_host(x)
            L = h.laplacian()
            one.spmv_setup(n, 0, L.rowptr, L.col, L.val)
            y1 = one.spmv_host(x)[row0: row0 + nrows]
            absrow = np.add.reduceat(np.abs(S.val * x[S.col]), S.rowptr[:-1])
            r["spmv_rows_ok"] = bool(np.all(np.abs(y - y1) <= 1e-14 * absrow + 1e-300))
            r["spmv_max_abs_diff"] = float(np.abs(y - y1).max())
            # the halo exchange (each rank receives only the rows its columns
            # read) against the all-gather of whole slots: the same bits
            hb = {}
            for mode in ("1", "0"):
                os.environ["EK_MR_HALO"] = mode
                try:
                    ctx.spmv_setup(n, row0, S.rowptr, S.col, S.val)
                    c0 = dict(counts)
                    lam_h, v_h, st_h = ctx.lanczos_fiedler()
                    ag = counts["allgather"] - c0["allgather"]
                    cs = ctx.comm_stats()  # (before spmv_host: its exchange is not a step's)
                    # the same solve with its collectives timed (exchange and all-reduce separately)
                    _, _, st_t = ctx.lanczos_fiedler(time_spmv=True)
                    ct = ctx.comm_stats()
                    hb[mode] = dict(lam=lam_h, v=v_h.tobytes(), ex=ctx.spmv_exchange(), matvecs=st_h["matvecs"],
                                    ag=ag, y=ctx.spmv_host(x).tobytes(),
                                    comm=cs, comm_t=ct, st_t={k: st_t[k] for k in ("matvecs", "allgathers",
                                                                                   "allreduces")})
                finally:
                    del os.environ["EK_MR_HALO"]
            r["halo"] = {"same_bits": hb["1"]["lam"] == hb["0"]["lam"] and hb["1"]["v"] == hb["0"]["v"],
                         "spmv_same": hb["1"]["y"] == hb["0"]["y"], "ex1": hb["1"]["ex"], "ex0": hb["0"]["ex"],
                         "ag": hb["1"]["ag"], "matvecs": hb["1"]["matvecs"], "comm": hb["1"]["comm"],
                         "comm_t": hb["1"]["comm_t"], "st_t": hb["1"]["st_t"], "comm_gather": hb["0"]["comm"]}
            res[name] = r
        # the whole file path, sharded: rank 0 writes the results file
        rr, _ = ctx.solve_file(circuit_path("ibm01"), eig=1, out_dir=os.path.join(tmp, f"r{rank}"))
        res["solve_file"] = {"iterations": rr["kl"]["iterations"], "net_cut_best": rr["kl"]["net_cut_best"]}
        # disconnected synthetic: breakdowns, injected vectors over global indices on both ranks
        h = ek.Hypergraph.generate(0.25, 3)
        n = h.nodes
        row0, nrows, _ = ek.shard_rows(n, WORLD, rank)  # (any tiling is accepted: here equal blocks)
        S = h.laplacian_rows(row0, row0 + nrows)
        ctx.spmv_setup(n, row0, S.rowptr, S.col, S.val)
        lam, v, st = ctx.lanczos_fiedler()
        res["syn0.25"] = {"lam": lam, "residual": st["residual"], "converged": bool(st["converged"]),
                          "finite": bool(np.all(np.isfinite(v))), "norm": float(np.linalg.norm(v)),
                          "v_head": v[:64].tolist()}
        one.close()
        ctx.close()
    except Exception:  # reported to the parent; the peer's next collective then fails too
        import traceback
        res["error"] = traceback.format_exc()
        print(f"[rank {rank}] {res['error']}", file=sys.stderr, flush=True)
    finally:
        out[rank] = res
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_lanczos_through_comm_seam(tmp_path):
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(_free_port(), str(tmp_path), out), nprocs=WORLD, join=True)
    r0, r1 = out[0], out[1]
    errors = {k: out[k]["error"] for k in (0, 1) if "error" in out[k]}
    assert not errors, errors
    for r in (r0, r1):
        for name in ("ibm01", "industry2"):
            assert r[name]["spmv_rows_ok"], r[name]
            for reorth, per_step in ((3, 2), (1, 1)):
                x = {k: v for k, v in r[name][reorth].items() if k != "v_bytes"}
                assert x["converged"] and x["residual"] < 1e-9, x
                assert x["dlam"] <= 1e-10 and x["dv"] <= 1e-8 and x["bits_equal"], x
                # ONE all-gather per Lanczos step (+ the final vector's) and
                # per_step all-reduces (reorth 3: alpha and ||w||^2, then the
                # projection; reorth 1: the three projections at once) + the
                # start vector's two norms, one per restart and cycle end, and
                # the residual's
                assert x["allgathers"] == x["stat_ag"] == x["matvecs"] + 1, x
                assert x["allreduces"] == x["stat_ar"], x
                lo = per_step * x["matvecs"]
                assert lo <= x["allreduces"] <= lo + 3 + 2 * (x["restarts"] + 1), x
            # partial reorthogonalisation runs on the sharded step: fewer
            # projected steps, the basis orthonormal to 1e-8 at every restart
            p = r[name][3]
            assert p["projected"] < 0.6 * p["matvecs"] and r[name][1]["projected"] == r[name][1]["matvecs"], p
            assert p["ortho_max"] <= 1e-8 and p["same_bits_with_ortho_check"], p
            assert p["matvecs"] <= 1.05 * r[name][1]["matvecs"], (p, r[name][1])
    for r in (r0, r1):
        for name in ("ibm01", "industry2"):
            hl = r[name]["halo"]
            print(name, "halo", hl)
            assert hl["same_bits"] and hl["spmv_same"], hl
            assert hl["ex1"][0] and not hl["ex0"][0] and hl["ex1"][1] <= hl["ex0"][1], hl
            assert hl["ag"] == hl["matvecs"] + 1, hl  # (one exchange a step + the final vector's all-gather)
            # ONE message to and ONE from every peer per exchange, one exchange a step
            # (the partial rides at the end of the rows: the block-end layout)
            cm = hl["comm"]
            assert cm["exchanges"] == hl["matvecs"], hl
            assert cm["sends"] == cm["recvs"] == (WORLD - 1) * cm["exchanges"], hl
            assert hl["comm_gather"]["exchanges"] == 0 and hl["comm_gather"]["sends"] == 0, hl
            assert hl["comm"]["exchanges_timed"] == 0, hl  # (untimed solve: nothing timed since the setup)
            # the timed solve: every all-gather (the steps' exchanges + the final
            # vector's) and every all-reduce timed, each kind on its own
            ct, stt = hl["comm_t"], hl["st_t"]
            assert ct["exchanges_timed"] == stt["allgathers"] and ct["allreduces_timed"] == stt["allreduces"], hl
            assert ct["exchange_ms"] > 0 and ct["allreduce_ms"] > 0, hl
    assert r1["ibm01"]["row0"] > 0 and r0["ibm01"]["nrows"] + r1["ibm01"]["nrows"] == 12752
    assert r0["industry2"]["nrows"] != r1["industry2"]["nrows"]  # nnz-balanced: unequal slices
    # every rank holds the same full vector: identical Ritz pairs
    for name in ("ibm01", "industry2"):
        for reorth in (3, 1):
            assert r0[name][reorth]["lam"] == r1[name][reorth]["lam"]
            assert r0[name][reorth]["v_bytes"] == r1[name][reorth]["v_bytes"]
    s0, s1 = r0["syn0.25"], r1["syn0.25"]
    for s in (s0, s1):
        assert s["converged"] and s["finite"] and abs(s["norm"] - 1) < 1e-10 and s["residual"] < 1e-8, s
        assert abs(s["lam"]) < 1e-8
    assert s0["v_head"] == s1["v_head"]
    # sharded file path == the reference cKL results (ibm01: even n, sign-independent)
    res = tmp_path / "r0" / "results" / "ibm01.hgr_KL_CutSize_EIG_output.txt"
    compare_results_text(res.read_text(), open(ref_results_path("ibm01")).read())
    assert r0["solve_file"]["net_cut_best"] == 367


def _worker10(rank, port, out):
    import datetime
    import faulthandler
    import sys
    import torch.distributed as dist
    faulthandler.enable()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=240))
    from conftest import load_package
    ek = load_package()
    res = {}
    try:
        h = ek.Hypergraph.generate(10.0, 10)  # configs[4]: 2,019,200 nodes
        n = h.nodes
        ctx = ek.Context(0)
        counts = {"allgather": 0, "allreduce": 0}
        _comm(ctx, rank, counts)
        assert ctx.spmv_setup_pins(h) is True  # this rank's rows built on the device
        _, row0, nrows = ctx.spmv_dims()
        c0 = dict(counts)
        lam, v, st = ctx.lanczos_fiedler()
        res.update(lam=lam, v_sha=__import__("hashlib").sha1(v.tobytes()).hexdigest(), residual=st["residual"],
                   converged=bool(st["converged"]), matvecs=st["matvecs"], restarts=st["restarts"], row0=row0,
                   nrows=nrows, allgathers=counts["allgather"] - c0["allgather"],
                   allreduces=counts["allreduce"] - c0["allreduce"], norm=float(np.linalg.norm(v)),
                   finite=bool(np.all(np.isfinite(v))))
        # this rank's SpMV rows vs the 1-rank SpMV
        x = np.random.default_rng(11).standard_normal(n)
        y = ctx.spmv_host(x)
        ctx.close()
        one = ek.Context(0)
        assert one.spmv_setup_pins(h) is True
        y1 = one.spmv_host(x)[row0: row0 + nrows]
        S = h.laplacian_rows(row0, row0 + nrows)
        absrow = np.add.reduceat(np.abs(S.val * x[S.col]), S.rowptr[:-1])
        res["spmv_rows_ok"] = bool(np.all(np.abs(y - y1) <= 1e-14 * absrow + 1e-300))
        res["spmv_max_abs_diff"] = float(np.abs(y - y1).max())
        if rank == 0:  # the 1-rank solve of the same problem
            lam1, v1, st1 = one.lanczos_fiedler()
            res.update(lam1=lam1, residual1=st1["residual"], matvecs1=st1["matvecs"])
        one.close()
    except Exception:
        import traceback
        res["error"] = traceback.format_exc()
        print(f"[rank {rank}] {res['error']}", file=sys.stderr, flush=True)
    finally:
        out[rank] = res
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_sharded_lanczos_syn10_config4():
    """configs[4]: the 10x synthetic, Lanczos rows
    sharded over 2 ranks (nnz-balanced map, rows built on the device per
    shard).  Converged residual, the same pair on both ranks, each rank's SpMV
    rows equal to the 1-rank SpMV's, lambda equal to the 1-rank solve's, and
    2 collectives per step.  (The synthetic is disconnected, so lambda1 = 0 and
    the null vector returned is not unique: v is compared across ranks, not
    with the 1-rank run.)"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker10, args=(_free_port(), out), nprocs=WORLD, join=True)
    r0, r1 = out[0], out[1]
    errors = {k: out[k]["error"] for k in (0, 1) if "error" in out[k]}
    assert not errors, errors
    for r in (r0, r1):
        assert r["converged"] and r["residual"] < 1e-8 and r["finite"] and abs(r["norm"] - 1) < 1e-10, r
        assert r["spmv_rows_ok"], r
        assert r["allgathers"] == r["matvecs"] + 1, r
        # (partial reorthogonalisation: two all-reduces a step; + up to 3 per injected vector)
        assert 2 * r["matvecs"] <= r["allreduces"] <= 2 * r["matvecs"] + 3 + 2 * (r["restarts"] + 1) + 3 * 64, r
    assert r0["nrows"] + r1["nrows"] == 2019200 and r1["row0"] == r0["nrows"]
    assert r0["lam"] == r1["lam"] and r0["v_sha"] == r1["v_sha"]
    assert abs(r0["lam"] - r0["lam1"]) <= 1e-10 and r0["residual1"] < 1e-8


@pytest.mark.parametrize("reorth", [3, 1])
@pytest.mark.parametrize("name", ["ibm01", "industry2"])
def test_rccl_one_rank_production_path(ek, monkeypatch, name, reorth):
    """The RCCL production path on the 1-GPU pool: under
    EK_COMM_FORCE a 1-rank context creates a real RCCL communicator
    (ncclCommInitRank, nranks 1) and runs the sharded step (ctx_lanczos.cpp
    factorize_mr: the slot layout with the ||f||^2 tail, ncclAllGather of the
    slots, ONE in-place ncclAllReduce of the projections, stream order).  The
    Fiedler pair must meet the pre_saved_EIG tolerances, the same forced path
    staged through the host (identity callbacks) must give the same bits, and
    every Lanczos step must issue one all-gather (+ the final vector's).
    reorth 3 (the default): the sharded partially reorthogonalised step
    (factorize_mr_pro: ncclAllReduce of alpha and ||w||^2, k_pro, then of the
    projection); reorth 1: the full pass by linearity (factorize_mr)."""
    monkeypatch.setenv("EK_COMM_FORCE", "1")
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    out = {}
    timed = {}
    for mode in ("rccl", "host"):
        c = ek.Context(0)
        try:
            if mode == "rccl":
                c.comm_init(1, 0, ek.comm_unique_id())
            else:
                c.comm_init_host(1, 0, lambda x: x.copy(), lambda x: None)
            c.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
            out[mode] = c.lanczos_fiedler(reorth=reorth)
            # the same solve with its collectives timed: RCCL by HIP events on
            # the stream, host-staged by the host's clock; the same bits
            lam_t, v_t, st_t = c.lanczos_fiedler(reorth=reorth, time_spmv=True)
            timed[mode] = (c.comm_stats(), st_t, lam_t == out[mode][0] and v_t.tobytes() == out[mode][1].tobytes())
        finally:
            c.close()
    for mode, (cs, st_t, same) in timed.items():
        assert same, mode
        assert cs["exchanges_timed"] == st_t["allgathers"] and cs["allreduces_timed"] == st_t["allreduces"], (mode, cs)
        assert cs["exchange_ms"] > 0 and cs["allreduce_ms"] > 0, (mode, cs)
    # the same path without the owned-slot / halo split of the SpMV (one SpMV
    # after the all-gather): other rounding, the same pair within tolerance
    monkeypatch.setenv("EK_MR_OVERLAP", "0")
    c = ek.Context(0)
    try:
        c.comm_init(1, 0, ek.comm_unique_id())
        c.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
        lam_n, v_n, st_n = c.lanczos_fiedler(reorth=reorth)
    finally:
        c.close()
    # the halo layout forced on (one rank: the own block alone, the pack kernel and the
    # compact column map): the same bits as the slot layout
    monkeypatch.setenv("EK_MR_HALO", "1")
    monkeypatch.delenv("EK_MR_OVERLAP")
    c = ek.Context(0)
    try:
        c.comm_init(1, 0, ek.comm_unique_id())
        c.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
        # the zero-row halo of one rank (the r05c failure):
        # no peer, so no message and an empty send list; the pack launch packs
        # zero message rows (the own block and partial only), and every step's
        # exchange posts nothing
        assert c.spmv_exchange() == (True, 0, 0)
        lam_x, v_x, st_x = c.lanczos_fiedler(reorth=reorth)
        cs_x = c.comm_stats()
        assert cs_x["exchanges"] == st_x["matvecs"] and cs_x["sends"] == cs_x["recvs"] == 0, cs_x
    finally:
        c.close()
    (lam, v, st), (lam_h, v_h, st_h) = out["rccl"], out["host"]
    assert lam_x == lam and v_x.tobytes() == v.tobytes() and st_x["allgathers"] == st["allgathers"]
    print(name, {k: st[k] for k in ("matvecs", "restarts", "allgathers", "allreduces", "reprojected", "residual")})
    assert abs(lam_n - lam) <= 1e-10 and st_n["residual"] < 1e-9
    assert _fiedler_ok(ek, name, lam_n, v_n)["bits_equal"]
    r = _fiedler_ok(ek, name, lam, v)
    assert st["converged"] and st["residual"] < 1e-9 and r["dlam"] <= 1e-10 and r["dv"] <= 1e-8 and r["bits_equal"], r
    assert st["allgathers"] == st["matvecs"] + 1
    per_step = 2 if reorth == 3 else 1
    assert per_step * st["matvecs"] <= st["allreduces"] <= per_step * st["matvecs"] + 3 + 2 * (st["restarts"] + 1)
    if reorth == 3:
        assert st["projected_steps"] < 0.6 * st["matvecs"], st
    assert lam_h == lam and v_h.tobytes() == v.tobytes()
    assert (st_h["allgathers"], st_h["allreduces"]) == (st["allgathers"], st["allreduces"])


@pytest.mark.parametrize("name", ["ibm01", "industry2"])
def test_sharded_step_reprojection(ek, monkeypatch, name):
    """the sharded step projects f' by linearity, exact to
    eps ||w|| rather than eps ||f'||; where f' cancels (||f'||^2 <
    2^-20 ||w||^2) the driver projects the next vector once more (ctx_lanczos.cpp
    Lanczos::repair).  The bar is raised (EK_MR_CANCEL=0.4) so the repair runs
    on many steps: the run must still meet the golden's tolerances with the
    basis orthonormal to 1e-12 at every restart (EK_LANCZOS_ORTHO), on the
    forced 1-rank RCCL path."""
    monkeypatch.setenv("EK_COMM_FORCE", "1")
    monkeypatch.setenv("EK_MR_CANCEL", "0.4")
    monkeypatch.setenv("EK_LANCZOS_ORTHO", "1")
    h = ek.Hypergraph.read(circuit_path(name))
    L = h.laplacian()
    c = ek.Context(0)
    try:
        c.comm_init(1, 0, ek.comm_unique_id())
        c.spmv_setup(h.nodes, 0, L.rowptr, L.col, L.val)
        lam, v, st = c.lanczos_fiedler(reorth=1)  # (the linearity step: the one that repairs)
    finally:
        c.close()
    print(name, {k: st[k] for k in ("matvecs", "restarts", "reprojected", "ortho_max", "residual")})
    r = _fiedler_ok(ek, name, lam, v)
    assert st["converged"] and st["residual"] < 1e-9 and r["dlam"] <= 1e-10 and r["dv"] <= 1e-8 and r["bits_equal"], r
    assert st["reprojected"] > 0
    assert st["ortho_max"] <= 1e-12


def _worker_head(rank, port, out):
    import datetime
    import faulthandler
    import sys
    import torch.distributed as dist
    faulthandler.enable()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=240))
    from conftest import load_package
    ek = load_package()
    res = {}
    try:
        h, _ = ek.Hypergraph.generate(1.15, 1).largest_component()
        ctx = ek.Context(0)
        counts = {"allgather": 0, "allreduce": 0}
        _comm(ctx, rank, counts)
        assert ctx.spmv_setup_pins(h) is True
        for reorth in (3, 1):
            lam, v, st = ctx.lanczos_fiedler(reorth=reorth)
            _, bits = ek.median_split(v)
            res[reorth] = dict(lam=lam, bits=np.packbits(bits).tobytes(), matvecs=st["matvecs"],
                               projected=st["projected_steps"], residual=st["residual"],
                               converged=bool(st["converged"]), v_sha=__import__("hashlib").sha1(v.tobytes()).hexdigest())
        os.environ["EK_LANCZOS_ORTHO"] = "1"
        try:
            _, _, st = ctx.lanczos_fiedler()
        finally:
            del os.environ["EK_LANCZOS_ORTHO"]
        res["ortho_max"] = st["ortho_max"]
        res["exchange_default"] = ctx.spmv_exchange()
        # the halo exchange forced on and off: the same pair, bit for bit
        for mode in ("1", "0"):
            os.environ["EK_MR_HALO"] = mode
            try:
                assert ctx.spmv_setup_pins(h) is True
                lam, v, st = ctx.lanczos_fiedler()
                res[f"halo{mode}"] = dict(lam=lam, v_sha=__import__("hashlib").sha1(v.tobytes()).hexdigest(),
                                          ex=ctx.spmv_exchange())
            finally:
                del os.environ["EK_MR_HALO"]
        ctx.close()
    except Exception:
        import traceback
        res["error"] = traceback.format_exc()
        print(f"[rank {rank}] {res['error']}", file=sys.stderr, flush=True)
    finally:
        out[rank] = res
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_headline_partial_reorth():
    """the bench's headline LCC (211,813 nodes) Lanczos
    sharded over 2 ranks under partial reorthogonalisation (the default) and
    under the full pass: fewer than half of the steps project, the basis stays
    orthonormal to 1e-8 at every restart, lambda1 within 1e-10 of the
    headline golden (tests/golden/syn115_lcc: the oracle restatement's
    converged pair) and the median split equal to the golden's on every node
    away from the median, the same pair on both ranks."""
    import json
    from conftest import GOLD
    import torch.multiprocessing as mp
    d = os.path.join(GOLD, "syn115_lcc")
    meta = json.load(open(os.path.join(d, "meta.json")))
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_head, args=(_free_port(), out), nprocs=WORLD, join=True)
    r0, r1 = out[0], out[1]
    errors = {k: out[k]["error"] for k in (0, 1) if "error" in out[k]}
    assert not errors, errors
    n = meta["nodes"]
    bits_ref = np.unpackbits(np.load(os.path.join(d, "split_bits.npy")))[:n]
    far = np.ones(n, bool)
    far[meta["near_median_nodes"]] = False
    print({k: {q: v for q, v in r0[k].items() if q != "bits"} for k in (3, 1)}, r0["ortho_max"])
    for r in (r0, r1):
        for reorth in (3, 1):
            x = r[reorth]
            assert x["converged"] and x["residual"] < 1e-8, x
            assert abs(x["lam"] - meta["lambda1"]) <= 1e-10, x
            bits = np.unpackbits(np.frombuffer(x["bits"], np.uint8))[:n]
            if np.mean(bits[far] != bits_ref[far]) > 0.5:  # (even split: the sign complements)
                bits = 1 - bits
            assert np.array_equal(bits[far], bits_ref[far])
        assert r[3]["projected"] < 0.5 * r[3]["matvecs"], r[3]
        assert r[3]["matvecs"] <= 1.05 * r[1]["matvecs"]
        assert r["ortho_max"] <= 1e-8
    for reorth in (3, 1):
        assert r0[reorth]["lam"] == r1[reorth]["lam"] and r0[reorth]["v_sha"] == r1[reorth]["v_sha"]
    for r in (r0, r1):
        print("exchange", r["exchange_default"], r["halo1"]["ex"], r["halo0"]["ex"])
        assert r["halo1"]["lam"] == r["halo0"]["lam"] == r[3]["lam"]
        assert r["halo1"]["v_sha"] == r["halo0"]["v_sha"] == r[3]["v_sha"]
        assert r["halo1"]["ex"][0] and not r["halo0"]["ex"][0] and r["halo1"]["ex"][1] < r["halo0"]["ex"][1]
