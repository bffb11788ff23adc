"""The row-sharded SpMV and Lanczos on small graphs at 2, 3 and 4 ranks (and 17,
past MAX_HALO_RANKS), every rank a thread of this process with a context of its
own on GPU 0, joined by mr_cases.LockstepComm through comm_init_host: set_shard,
halo_build and halo_exchange, the column remap and owned-slot rows of both
setup routes (the host rows under an explicit map, the device build under the
library's), the slot and halo branches of ek_spmv / ek_spmv_host, and the
sharded Lanczos steps with a non-zero row0.  The cases, the shard maps (one-row
and empty slices, slices at the GT_ROWS edge) and the numpy restatement of the
halo layout are mr_cases.py's; test_mr_cases_host.py proves them on the CPU and
that each edge is attained.

Bars: every SpMV row within (nnz_i + 1) eps sum_j |a_ij x_j| of the longdouble
product (mr_cases.spmv_reference); the device-pointer SpMV, the halo layout and
the device build give the same bits as the host-pointer SpMV, the slot layout
and the host rows; every rank's Fiedler pair passes lanczos_cases.check_pair
(the one-rank bars) and is bit-identical across ranks and layouts; the
collectives counted by the communicator are the library's own counts and
test_multirank_gpu.py's per-step bounds.

Tests whose id says "empty" run maps with a rank that owns no row.
Run on an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import lanczos_cases as lc
import mr_cases as mc

pytestmark = pytest.mark.gpu

SPLIT = (False, True)
SPLIT_IDS = ("rows", "empty")


def _entries(name, world, empty, with_lib=True):
    """[(map name, off, device route)] of `name` at `world` ranks: the explicit
    maps through the host rows, the library's map through both routes."""
    out = [(k, off, False) for k, off in mc.case_maps(name, world)]
    if with_lib:
        lib = mc.lib_map(name, world)
        out += [("lib", lib, False), ("lib/dev", lib, True)]
    return [e for e in out if mc.has_empty(e[1]) == empty]


def _setup(ctx, name, rank, off, dev):
    h = mc.hypergraph(name)
    n, row0, row1 = h.nodes, int(off[rank]), int(off[rank + 1])
    if dev:
        assert ctx.spmv_setup_pins(h) is True  # the device build ran (no host fallback)
    else:
        S = h.laplacian_rows(row0, row1)
        ctx.spmv_setup(n, row0, S.rowptr, S.col, S.val)
    assert ctx.spmv_dims() == (n, row0, row1 - row0)
    return n, row0, row1


def _hip():
    """hipMalloc / hipMemcpy / hipFree of the HIP runtime the library itself is
    linked to, resolved through the library's handle.  (torch's ROCm wheel
    brings a HIP and HSA runtime of its own; a second runtime in the process
    finds no GPU, so device memory for ek_spmv cannot come from torch here.)"""
    lib = mc.load_package()._lib
    lib.hipMalloc.argtypes, lib.hipMalloc.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t], ctypes.c_int
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemcpy.restype = ctypes.c_int
    lib.hipFree.argtypes, lib.hipFree.restype = [ctypes.c_void_p], ctypes.c_int
    return lib


def _device_spmv(ctx, x, nrows):
    """y = ek_spmv(x) through device pointers: x of n doubles, y of nrows (NaN before the call)."""
    hip = _hip()
    H2D, D2H = 1, 2
    x = np.ascontiguousarray(x, np.float64)
    y = np.full(max(nrows, 1), np.nan)
    xd, yd = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(xd), x.nbytes) == 0
    try:
        assert hip.hipMalloc(ctypes.byref(yd), y.nbytes) == 0
        try:
            assert hip.hipMemcpy(xd, x.ctypes.data, x.nbytes, H2D) == 0
            assert hip.hipMemcpy(yd, y.ctypes.data, y.nbytes, H2D) == 0
            ctx.spmv_device(xd.value, yd.value)
            ctx.synchronize()
            assert hip.hipMemcpy(y.ctypes.data, yd, y.nbytes, D2H) == 0
        finally:
            hip.hipFree(yd)
    finally:
        hip.hipFree(xd)
    assert nrows > 0 or np.isnan(y[0])  # (a rank of no rows writes nothing)
    return y[:nrows]


def _probe(ctx, name, rank, off, dev):
    """One rank's SpMV under one map: the host product against the reference, the
    device-pointer product against the host one; returns the bits and the exchange."""
    n, row0, row1 = _setup(ctx, name, rank, off, dev)
    x, yref, bound = mc.spmv_reference(name)
    y = ctx.spmv_host(x)
    assert y.shape == (row1 - row0,)
    err = np.abs(y - yref[row0:row1])
    worst = float(np.max(err / np.maximum(bound[row0:row1], np.finfo(np.longdouble).tiny), initial=0.0))
    print(f"{name} rank {rank} of {len(off) - 1} {[int(o) for o in off]} dev={dev}: max |y - yref| / bound = {worst:.3g}")
    assert np.all(err <= bound[row0:row1]), (name, rank, list(off), worst)
    yd = _device_spmv(ctx, x, row1 - row0)
    assert yd.tobytes() == y.tobytes(), (name, rank, list(off), "ek_spmv against ek_spmv_host")
    return {"y": y.tobytes(), "ex": ctx.spmv_exchange()}


def _plan(name, off):
    return mc.halo_plan(off, mc.rows_of(name, off), mc.slot_dims(off)[0])


def _spmv_case(name, world, entries):
    """3a and 3b for one graph and world: every entry under EK_MR_HALO 1, 0 and unset."""
    mc.spmv_reference(name)  # (computed once, before the threads)
    got = {}
    for mode in mc.HALO_MODES:
        def fn(rank, ctx, comm):
            return {key: _probe(ctx, name, rank, off, dev) for key, off, dev in entries}
        got[mode], _ = mc.run_ranks(world, fn, env={"EK_MR_HALO": mode})
    for key, off, dev in entries:
        plan = _plan(name, off)
        halo_of = {"1": world <= mc.MAX_HALO_RANKS, "0": False, None: plan["auto"] and world <= mc.MAX_HALO_RANKS}
        for r in range(world):
            for mode in mc.HALO_MODES:
                want = mc.exchange_doubles(plan, r, halo_of[mode])
                assert got[mode][r][key]["ex"] == want, (name, world, key, r, mode, got[mode][r][key]["ex"], want)
            # the halo layout gives the bits of the slot layout
            assert got["1"][r][key]["y"] == got["0"][r][key]["y"] == got[None][r][key]["y"], (name, world, key, r)
    if any(k == "lib/dev" for k, _, _ in entries):  # the device build gives the bits of the host rows
        for mode in mc.HALO_MODES:
            for r in range(world):
                assert got[mode][r]["lib/dev"] == got[mode][r]["lib"], (name, world, r, mode)


def _combos(pairs):
    """(name, world, empty) of `pairs` for which some map of that kind exists, so
    that every id runs something (2 ranks have no mid_empty / last_empty)."""
    return [pytest.param(n, w, e, id=f"{n}-{w}-{SPLIT_IDS[e]}") for n, w in pairs for e in SPLIT if _entries(n, w, e)]


@pytest.mark.parametrize("name,world,empty", _combos(mc.spmv_cases()))
def test_spmv_rows(name, world, empty):
    _spmv_case(name, world, _entries(name, world, empty))


def _krylov_can_run_out(name):
    """Whether a Lanczos cycle of `name` can meet an invariant subspace before its
    ncv steps (then the driver injects a fresh vector: 3 all-reduces each).  In
    exact arithmetic the Krylov space of the deflated start vector has at most
    one dimension per distinct non-zero eigenvalue, so it can when those are
    fewer than ncv = min(80, n / 2) (the star has 2, K_n 1, the barbell's two
    K_12 leave 13), and on a disconnected graph, whose second null vector the
    cycle converges on exactly.  Distinct: further apart than eigh's error."""
    ref = lc.reference(name)
    distinct = 1 + int(np.sum(np.diff(ref.w[1:]) > 2 * ref.eig_err))
    return ref.disconnected or distinct < min(80, ref.n // 2)


def _ar_bounds(name, st, per_step):
    """test_multirank_gpu.py's: per_step all-reduces a step, + the start vector's
    two, one per restart and cycle end and the residual's; + 3 per injected
    vector (as there, 64 allowed for) where the Krylov space can run out."""
    lo = per_step * st["matvecs"]
    inject = 3 * 64 if _krylov_can_run_out(name) else 0
    return lo, lo + 3 + 2 * (st["restarts"] + 1) + inject


def _solve(ctx, comm, rank, name, world, reorth, what, halo):
    ek = mc.load_package()
    c0, s0 = dict(comm.calls[rank]), ctx.comm_stats()
    lam, v, st = ctx.lanczos_fiedler(reorth=reorth)
    ag = comm.calls[rank]["allgather"] - c0["allgather"]
    ar = comm.calls[rank]["allreduce"] - c0["allreduce"]
    cs = ctx.comm_stats()
    lc.check_pair(ek, name, lam, v, st, f"{what} rank {rank}/{world} reorth {reorth}")
    assert ag == st["allgathers"] == st["matvecs"] + 1, (what, ag, st)
    lo, hi = _ar_bounds(name, st, 2 if reorth == 3 else 1)
    assert ar == st["allreduces"] and lo <= ar <= hi, (what, ar, lo, hi, st)
    ex = cs["exchanges"] - s0["exchanges"]
    sends, recvs = cs["sends"] - s0["sends"], cs["recvs"] - s0["recvs"]
    if halo:
        assert ex == st["matvecs"] and sends == recvs == (world - 1) * ex, (what, cs, s0, st)
    else:
        assert ex == sends == recvs == 0, (what, cs, s0)
    return {"lam": lam, "v": v.tobytes(), "matvecs": st["matvecs"], "restarts": st["restarts"]}


def _lanczos_case(name, world, entries, modes, reorths=(3, 1)):
    """3c for one graph and world: every entry under every EK_MR_HALO mode of
    `modes` and both reorth values; the same bits on every rank and in every layout."""
    lc.reference(name)
    got = {}
    for mode in modes:
        def fn(rank, ctx, comm):
            out = {}
            for key, off, dev in entries:
                _setup(ctx, name, rank, off, dev)
                halo = ctx.spmv_exchange()[0]
                assert mode is None or halo == (mode == "1" and world <= mc.MAX_HALO_RANKS)
                for reorth in reorths:
                    out[(key, reorth)] = _solve(ctx, comm, rank, name, world, reorth, f"{key} halo={mode}", halo)
            return out
        got[mode], _ = mc.run_ranks(world, fn, env={"EK_MR_HALO": mode})
    for mode in modes:
        for k, first in got[mode][0].items():
            for r in range(world):
                assert got[mode][r][k] == first, (name, world, mode, k, r, "the ranks' pairs differ")
            assert got[mode][0][k] == got[modes[0]][0][k], (name, world, mode, k, "the layouts' pairs differ")


@pytest.mark.parametrize("name,world,empty", _combos([(n, w) for n in mc.LANCZOS_ALL for w in mc.WORLDS]))
def test_lanczos_every_map_and_layout(name, world, empty):
    """star-65 at reorth 1 holds the breakdown test of the step that projects by
    linearity (factorize_mr) to the norm of the sound steps: every step after
    the second is a breakdown there (each injected vector lies in the star's
    63-dimensional lambda = 1 eigenspace), and the launches that run on past one
    must not raise the threshold of the steps before it (ctx_lanczos.cpp
    first_breakdown)."""
    _lanczos_case(name, world, _entries(name, world, empty), ("1", "0"))


@pytest.mark.parametrize("name", mc.LANCZOS_W3)
def test_lanczos_three_ranks_default_layout(name):
    """World 3, the layout the library picks, the device build under the library's map."""
    lib = mc.lib_map(name, 3)
    assert not mc.has_empty(lib)
    _lanczos_case(name, 3, [("lib/dev", lib, True)], (None,))


@pytest.mark.parametrize("off", mc.GT_MAPS["path-2049"], ids=lambda o: f"gt{o[1]}")
def test_lanczos_path_2049_at_the_row_block_edge(off):
    """Two ranks, 1,023 | 1,026, 1,024 | 1,025 and 1,025 | 1,024 rows: two row
    blocks of the basis, the second nearly all padding."""
    _lanczos_case("path-2049", 2, [(f"gt{off[1]}", np.array(off, np.int64), False)], (None,))


@pytest.mark.parametrize("name,world,key", [("path-65", 3, "first1"), ("random-300", 2, "last1")])
def test_lanczos_without_the_owned_slot_overlap(name, world, key):
    """EK_MR_OVERLAP=0: one SpMV after the all-gather.  Other rounding than the
    split SpMV, so no bits are compared: the pair passes the same bars."""
    off = dict(mc.case_maps(name, world))[key]
    ek = mc.load_package()
    lc.reference(name)

    def fn(rank, ctx, comm):
        _setup(ctx, name, rank, off, False)
        lam, v, st = ctx.lanczos_fiedler()
        lc.check_pair(ek, name, lam, v, st, f"no overlap rank {rank}")
        return lam, v.tobytes()

    got, _ = mc.run_ranks(world, fn, env={"EK_MR_OVERLAP": "0", "EK_MR_HALO": None})
    assert all(g == got[0] for g in got)


def test_seventeen_ranks_take_the_slot_layout():
    """17 > MAX_HALO_RANKS: the all-gather of whole slots even with EK_MR_HALO=1;
    the SpMV rows, the exchange accounting and the Lanczos pair as at any world."""
    name, off = mc.WORLD17
    world = len(off) - 1
    entries = [("w17", off, False)]
    _spmv_case(name, world, entries)
    _lanczos_case(name, world, entries, ("1",))


@pytest.mark.parametrize("world", mc.WORLDS)
def test_first_step_message_is_the_restated_pack(world):
    """star-65 with the hub alone on rank 0 (every rank reads it; it reads every
    row of every rank).  The start vector is deterministic from the global row
    index, so the slot-layout run's first step all-gathers every rank's whole f
    (rows, zero padding, its ||f||^2 partial at [ldv]); from that f the halo
    run's first block of every rank must be mr_cases.halo_message's bits: the
    send lists and k_halo_pack.  (The start vector is not restated on the host:
    its deflation's sums follow the device's reduction order.)  The setup's own
    all-gathers are checked on the way: (row0, nrows), the request counts, the
    padded request lists."""
    name = "star-65"
    off = mc.maps(65, world)["first1"]
    plan = _plan(name, off)
    blocks = {}
    for mode in ("0", "1"):
        def fn(rank, ctx, comm):
            _setup(ctx, name, rank, off, False)
            at = len(comm.sent[rank])
            ctx.lanczos_fiedler()
            return at
        at, comm = mc.run_ranks(world, fn, env={"EK_MR_HALO": mode}, record=True)
        for r in range(world):
            sent = comm.sent[r]
            assert list(sent[0]) == [off[r], off[r + 1] - off[r]]
            assert at[r] == (3 if mode == "1" else 1)  # (EK_MR_HALO=0 returns before halo_build's collectives)
            if mode == "1":
                assert list(sent[1]) == list(plan["C"][r]) and list(sent[2]) == list(plan["lists"][r])
        blocks[mode] = [comm.sent[r][at[r]] for r in range(world)]
    for r in range(world):
        f, nr = blocks["0"][r], int(off[r + 1] - off[r])
        assert f.shape == (plan["slot"],) and np.all(f[nr:plan["ldv"]] == 0.0) and np.all(f[plan["ldv"] + 1:] == 0.0)
        assert np.all(f[:nr] != 0.0) and abs(f[plan["ldv"]] - f[:nr] @ f[:nr]) <= 2 * (nr + 1) * mc.EPS * f[plan["ldv"]]
        assert f.tobytes() == mc.slot_block(plan, r, f[:nr], f[plan["ldv"]]).tobytes()
        assert blocks["1"][r].tobytes() == mc.halo_message(plan, r, f).tobytes(), (world, r)
