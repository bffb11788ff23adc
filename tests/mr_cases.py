"""The row-sharded SpMV and Lanczos at small shapes: what test_mr_cases_host.py
(CPU) and test_gpu_mr_small.py (GPU) share.

* LockstepComm / run_ranks: the ranks of one sharded context group as threads
  of this process, each with its own Context, joined through
  Context.comm_init_host by an in-process communicator (a threading.Barrier).
  The library is loaded with ctypes.CDLL, so a rank inside a library call does
  not hold the GIL and takes it again in its callbacks.  No processes, no
  torch.distributed.
* maps / lib_map / GT_MAPS: the shard maps (one-row and empty slices, slices at
  the GT_ROWS = 1,024 edge of the Lanczos vectors' leading dimension).
* halo_plan / halo_message / slot_block / sharded_spmv: ctx_comm.cpp halo_build
  and halo_exchange restated in numpy with every rank in one process, no
  collective (the logic test_distributed_cpu.py::_halo_worker runs per rank
  over gloo).
* the case lists of the GPU tests, so the host test can assert that each edge
  they are there for is attained.

Graphs: lanczos_cases.GRAPHS, and one of this module's (LADDER) for the one
edge none of those can reach: see there."""
import functools
import os
import threading
import traceback

import numpy as np

import lanczos_cases as lc
from conftest import load_package

GT_ROWS = 1024        # kernels_lanczos.hip: rows per projection block; ldv is a multiple
MAX_HALO_RANKS = 16   # ek_internal.hpp: more ranks take the all-gather of whole slots
EPS = lc.EPS

# The barrier's timeout is a deadlock guard, not a measurement.  Slowest case
# measured on the MI355X: star-65 over 4 ranks with every map, layout and reorth
# value, 4.5 s of wall for all its runs (a breakdown and an injected vector at
# nearly every step); then path-2049 over 2 ranks, 2.7 s, and the 17-rank case,
# 2.4 s.  60 s is more than ten times the slowest.
BARRIER_TIMEOUT = 60.0
JOIN_TIMEOUT = 4 * BARRIER_TIMEOUT


class RankAborted(RuntimeError):
    """A collective of this rank was abandoned because a peer failed or never came."""


class LockstepComm:
    """The collectives of `world` ranks living in threads of one process.

    allgather(rank, x) -> the ranks' blocks in rank order; allreduce(rank, buf)
    writes into buf the sum of the ranks' copies, added in rank order from rank
    0, computed by every rank itself from the same operands in the same order
    (the same bits everywhere).  calls / doubles count per rank and kind;
    record=True keeps every all-gather send block per rank (sent[rank]).  A
    rank that fails calls abort(): the barrier breaks and every other rank's
    pending or next collective raises RankAborted."""

    def __init__(self, world, timeout=BARRIER_TIMEOUT, record=False):
        self.world = int(world)
        self._bar = threading.Barrier(self.world, timeout=timeout)
        self._slot = [None] * self.world
        self.calls = [{"allgather": 0, "allreduce": 0} for _ in range(self.world)]
        self.doubles = [{"allgather": 0, "allreduce": 0} for _ in range(self.world)]
        self.sent = [[] for _ in range(self.world)] if record else None

    def abort(self):
        self._bar.abort()

    @property
    def broken(self):
        return self._bar.broken

    def _wait(self):
        try:
            self._bar.wait()
        except threading.BrokenBarrierError:
            raise RankAborted("a peer failed or did not reach this collective") from None

    def _exchange(self, rank, kind, x):
        x = np.array(x, np.float64)  # (a copy: the caller's buffer is the library's staging memory)
        self.calls[rank][kind] += 1
        self.doubles[rank][kind] += x.size
        self._slot[rank] = (kind, x)
        self._wait()
        blocks = list(self._slot)
        self._wait()  # every rank has taken the blocks before any rank posts its next one
        if any(k != kind or b.size != x.size for k, b in blocks):
            self.abort()
            raise AssertionError(f"rank {rank}: collectives paired wrongly: {[(k, b.size) for k, b in blocks]}")
        return [b for _, b in blocks]

    def allgather(self, rank, x):
        if self.sent is not None:
            self.sent[rank].append(np.array(x, np.float64))
        return np.concatenate(self._exchange(rank, "allgather", x))

    def allreduce(self, rank, buf):
        blocks = self._exchange(rank, "allreduce", buf)
        tot = blocks[0].copy()
        for b in blocks[1:]:
            tot += b
        buf[:] = tot


def run_ranks(world, fn, env=None, timeout=BARRIER_TIMEOUT, record=False):
    """fn(rank, ctx, comm) on `world` threads, each with a Context of its own
    joined to a LockstepComm by comm_init_host; returns (the ranks' results in
    rank order, the communicator with its counts and recorded blocks).  env:
    EK_* variables (None: unset) put in place before any thread starts and
    restored afterwards: they are process-wide and the library reads them at
    setup.  timeout is the barrier's; the join waits JOIN_TIMEOUT whatever it
    is.  The first failure, in time, is raised again with its traceback in the
    message; its peers' RankAborted / EK_ECOMM follow from it."""
    ek = load_package()
    comm = LockstepComm(world, timeout, record)
    results, errors, lock = [None] * world, [], threading.Lock()
    saved = {k: os.environ.get(k) for k in (env or {})}

    def put(k, v):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)

    def body(rank):
        ctx = None
        try:
            ctx = ek.Context(0)
            ctx.comm_init_host(world, rank, lambda x: comm.allgather(rank, x), lambda b: comm.allreduce(rank, b))
            results[rank] = fn(rank, ctx, comm)
        except BaseException as e:  # noqa: BLE001 (reported by the caller's thread)
            with lock:
                errors.append((rank, e, traceback.format_exc()))
            comm.abort()
        finally:
            if ctx is not None:
                ctx.close()

    for k, v in (env or {}).items():
        put(k, v)
    try:
        threads = [threading.Thread(target=body, args=(r,), name=f"rank{r}", daemon=True) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_TIMEOUT)
        stuck = [t.name for t in threads if t.is_alive()]
    finally:
        for k, v in saved.items():
            put(k, v)
    if stuck:
        comm.abort()
        raise AssertionError(f"ranks still running after {JOIN_TIMEOUT} s: {stuck}")
    if errors:
        rank, e, tb = errors[0]
        raise AssertionError(f"rank {rank} of {world} failed first ({len(errors)} in all):\n{tb}") from e
    assert not comm.broken
    return results, comm


# ---------------------------------------------------------------------------
# shard maps
def _even(n, parts):
    return [n * i // parts for i in range(parts + 1)]


def maps(n, world):
    """name -> off (world + 1 offsets tiling [0, n)).  equal: ek.shard_rows (64-row
    aligned blocks, so short graphs leave the last ranks empty); first1 / last1: one
    rank owns one row; mid_empty / last_empty (world >= 3): one rank owns no row."""
    ek = load_package()
    m = {"equal": [0] + [r0 + nr for r0, nr, _ in (ek.shard_rows(n, world, r) for r in range(world))],
         "first1": [0] + [1 + o for o in _even(n - 1, world - 1)],
         "last1": _even(n - 1, world - 1) + [n]}
    if world >= 3:
        e = _even(n, world - 1)
        m["mid_empty"] = e[:2] + e[1:]
        m["last_empty"] = e + [n]
    return {k: np.array(v, np.int64) for k, v in m.items()}


def lib_map(name, world):
    """The nnz-balanced map spmv_setup_pins takes by itself (ek.shard_map)."""
    return np.array(load_package().shard_map(hypergraph(name), world), np.int64)


def has_empty(off):
    return bool(np.any(np.diff(off) == 0))


# The Lanczos vectors' leading dimension is the largest slice rounded up to
# GT_ROWS: slices of 1,023 / 1,024 rows give ldv 1,024 (one row block), 1,025
# and 1,026 give 2,048 (two), and the slot is ldv + 64.  Beside path-2049's
# three maps, path-1025's leave the other rank 2 rows or 1: its padding is
# nearly the whole slot.
GT_MAPS = {"path-2049": ([0, 1023, 2049], [0, 1024, 2049], [0, 1025, 2049]),
           "path-1025": ([0, 1023, 1025], [0, 1024, 1025])}
LMAX0 = ("paths-40+60", [0, 40, 100])  # no rank reads a row of the other: lmax = 0


# With EK_MR_HALO unset the library takes the halo layout when the ranks' requests
# (+ 1 partial each) come to at most 3/4 of the whole slots.  A slot is at least
# 1,024 + 64 doubles whatever the graph, so at 2 ranks the slot layout wins only
# when the two ranks read more than 1,630 rows of each other: no graph of
# lanczos_cases that large has the edges (path-2049's are local), and a star or
# K_n of tens of nodes, which reads every row of its peers, stays far below.  A
# ladder of 2 x 850 nodes split between its rails does it: every row reads its
# rung's other end, 2 x (850 + 1) = 1,702 > 0.75 x 2 x 1,088 = 1,632.
LADDER = "ladder-1700"
LADDER_MAP = [0, 850, 1700]
EXTRA = {LADDER: (1700, [[i, i + 1] for i in range(849)] + [[850 + i, 851 + i] for i in range(849)] +
                  [[i, 850 + i] for i in range(850)])}


def graph(name):
    """(nodes, nets)"""
    return lc.GRAPHS[name][:2] if name in lc.GRAPHS else EXTRA[name]


@functools.lru_cache(maxsize=None)
def hypergraph(name):
    n, nets = graph(name)
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in nets])]).astype(np.int64)
    return load_package().Hypergraph.from_pins(n, ptr, np.array([p for e in nets for p in e], np.int32))


def dense_laplacian(name):
    if name in lc.GRAPHS:
        return lc.dense_laplacian(name)
    n, nets = graph(name)
    L = np.zeros((n, n))
    for a, b in nets:  # (2-pin nets: unit edges)
        L[a, b] -= 1.0
        L[b, a] -= 1.0
        L[a, a] += 1.0
        L[b, b] += 1.0
    return L


# ---------------------------------------------------------------------------
# the cases of test_gpu_mr_small.py
WORLDS = (2, 3, 4)
SPMV_GRAPHS = ("path-9", "path-65", "star-65", "complete-8", "barbell", "grid-7x11", "random-300", "paths-40+60",
               "cycle-1024")
HALO_MODES = ("1", "0", None)  # EK_MR_HALO: forced on, forced off, the library's decision
LANCZOS_ALL = ("path-9", "path-65", "star-65", "paths-40+60")  # every world, map, layout and reorth
LANCZOS_W3 = ("complete-8", "barbell", "grid-7x11", "random-300", "cycle-1024", "path-1025")  # world 3, default layout
WORLD17 = ("path-65", np.array(_even(65, 17), np.int64))  # 17 > MAX_HALO_RANKS; 3 or 4 rows a rank


def case_maps(name, world):
    """[(map name, off)] of the explicit maps the GPU tests run `name` under at
    `world` ranks (the library's own map comes on top, through spmv_setup_pins)."""
    if name == LADDER:
        return [("ladder", np.array(LADDER_MAP, np.int64))]
    n = graph(name)[0]
    out = list(maps(n, world).items()) if name not in GT_MAPS else []
    if world == 2:
        out += [(f"gt{o[1]}", np.array(o, np.int64)) for o in GT_MAPS.get(name, ())]
        if name == LMAX0[0]:
            out.append(("lmax0", np.array(LMAX0[1], np.int64)))
    return out


def spmv_cases():
    """(name, world) of test_spmv_rows."""
    return [(g, w) for g in SPMV_GRAPHS for w in WORLDS] + [(g, 2) for g in GT_MAPS] + [(LADDER, 2)]


def all_cases():
    """(name, world, map name, off) of every explicit map the GPU tests run, and the library's."""
    out = []
    for name, world in spmv_cases():
        out += [(name, world, k, off) for k, off in case_maps(name, world)]
        out.append((name, world, "lib", lib_map(name, world)))
    for name in LANCZOS_W3:
        out.append((name, 3, "lib", lib_map(name, 3)))
    return out


# ---------------------------------------------------------------------------
# the restatement
def slot_dims(off):
    """(ldv, slot) of ctx_comm.cpp set_shard."""
    mx = max(int(np.diff(off).max()), 1)
    ldv = -(-mx // GT_ROWS) * GT_ROWS
    return ldv, ldv + 64


def rows_of(name, off):
    """Every rank's Laplacian rows (global columns, rowptr from 0)."""
    h = hypergraph(name)
    return [h.laplacian_rows(int(off[r]), int(off[r + 1])) for r in range(len(off) - 1)]


def halo_plan(off, rows_of_rank, ldv):
    """ctx_comm.cpp halo_build for every rank at once.  Global: C (C[r, q] = rows
    rank r reads from rank q), lmax, lists (the padded request lists as all-gathered),
    tot_halo, full, auto (the library's decision with EK_MR_HALO unset), smax.
    Per rank (lists indexed by rank): colx (the slot-layout columns), req, sidx,
    soff, rcnt, base, pidx, src, colh (the compact column map), gidx (the global
    row behind every entry of the compact x; -1: a partial)."""
    off = np.asarray(off, np.int64)
    W, S = len(off) - 1, ldv + 64
    nrows = np.diff(off)
    owner, colx, req = [], [], []
    for r in range(W):
        col = np.asarray(rows_of_rank[r].col, np.int64)
        own = np.searchsorted(off[1:-1], col, side="right")  # the largest q with off[q] <= col
        owner.append(own)
        colx.append(own * S + (col - off[own]))
        req.append([np.unique(col[own == q]) - off[q] if q != r else np.zeros(0, np.int64) for q in range(W)])
    C = np.array([[len(req[r][q]) for q in range(W)] for r in range(W)], np.int64)
    lmax = int(C.sum(axis=1).max())
    lists = np.zeros((W, max(lmax, 1)), np.int64)
    for r in range(W):
        cat = np.concatenate(req[r])
        lists[r, :len(cat)] = cat
    tot_halo = int(sum(C[r, q] + 1 for r in range(W) for q in range(W) if q != r))
    full = W * (W - 1) * S
    p = {"world": W, "off": off, "ldv": ldv, "slot": S, "C": C, "lmax": lmax, "lists": lists, "tot_halo": tot_halo,
         "full": full, "auto": W > 1 and tot_halo <= 0.75 * full, "colx": colx, "req": req,
         "sidx": [], "soff": [], "rcnt": [], "base": [], "pidx": [], "src": [], "colh": [], "gidx": []}
    smax = 1
    for q in range(W):
        smax = max(smax, int(sum(C[r, q] + 1 for r in range(W) if r != q)))
    p["smax"] = smax
    for me in range(W):
        sidx, soff = [], np.zeros(W, np.int64)
        for r in range(W):
            if r == me:
                continue
            o = int(sum(C[r, q] for q in range(me) if q != r))  # where r's request from `me` starts in r's list
            soff[r] = len(sidx)
            sidx += list(lists[r, o:o + C[r, me]]) + [ldv]
        rcnt = np.array([nrows[me] if q == me else C[me, q] for q in range(W)], np.int64)
        base = np.concatenate([[0], np.cumsum(rcnt + 1)])
        # q's send buffer lists its messages to r = 0, 1, ... (r != q): where this rank's starts
        src = np.array([sum(C[r, q] + 1 for r in range(me) if r != q) if q != me else 0 for q in range(W)], np.int64)
        pos = [{int(l): k for k, l in enumerate(req[me][q])} for q in range(W)]
        loc = colx[me] - owner[me] * S
        colh = np.array([base[q] + (l if q == me else pos[q][int(l)]) for q, l in zip(owner[me], loc)], np.int64)
        gidx = np.full(base[-1], -1, np.int64)
        for q in range(W):
            rows = np.arange(nrows[me]) if q == me else req[me][q]
            gidx[base[q]:base[q] + len(rows)] = off[q] + rows
        for k, v in (("sidx", np.array(sidx, np.int64)), ("soff", soff), ("rcnt", rcnt), ("base", base),
                     ("pidx", base[:-1] + rcnt), ("src", src), ("colh", colh), ("gidx", gidx)):
            p[k].append(v)
    return p


def exchange_doubles(plan, rank, halo):
    """(halo, doubles received, doubles sent) per step: ek_spmv_exchange."""
    W, C = plan["world"], plan["C"]
    if not halo:
        return False, (W - 1) * plan["slot"], (W - 1) * plan["slot"]
    return (True, int(sum(C[rank, q] + 1 for q in range(W) if q != rank)),
            int(sum(C[r, rank] + 1 for r in range(W) if r != rank)))


def slot_block(plan, rank, f_rows, partial):
    """Rank `rank`'s all-gather block in the slot layout: its rows, zeros up to
    ldv, its ||f||^2 partial at [ldv], zeros after."""
    b = np.zeros(plan["slot"])
    b[:len(f_rows)] = f_rows
    b[plan["ldv"]] = partial
    return b


def halo_message(plan, rank, f):
    """Rank `rank`'s all-gather block in the halo layout (host-staged: its packed
    messages to the peers in rank order, each closed by its partial, padded with
    zeros to the longest rank's) from f, its slot_block."""
    b = np.zeros(plan["smax"])
    s = plan["sidx"][rank]
    b[:len(s)] = np.asarray(f)[s]
    return b


def halo_x(plan, rank, blocks):
    """The compact x rank `rank` holds after one exchange, from every rank's slot_block."""
    W = plan["world"]
    base, rcnt, src = plan["base"][rank], plan["rcnt"][rank], plan["src"][rank]
    X = np.zeros(base[-1])
    for q in range(W):
        if q == rank:
            X[base[q]:base[q] + rcnt[q]] = blocks[q][:rcnt[q]]
            X[base[q] + rcnt[q]] = blocks[q][plan["ldv"]]
        else:
            m = halo_message(plan, q, blocks[q])
            X[base[q]:base[q + 1]] = m[src[q]:src[q] + rcnt[q] + 1]
    return X


def csr_matvec(rowptr, col, val, x):
    """Row sums in storage order, one row at a time (the order is the row's)."""
    y = np.zeros(len(rowptr) - 1)
    for i in range(len(y)):
        s = 0.0
        for p in range(rowptr[i], rowptr[i + 1]):
            s += val[p] * x[col[p]]
        y[i] = s
    return y


def sharded_spmv(plan, rank, rows, x, halo):
    """Rank `rank`'s rows times the global x, read through the slot layout or the
    compact halo layout after one exchange."""
    off, W = plan["off"], plan["world"]
    blocks = [slot_block(plan, q, x[off[q]:off[q + 1]], 0.0) for q in range(W)]
    if halo:
        return csr_matvec(rows.rowptr, plan["colh"][rank], rows.val, halo_x(plan, rank, blocks))
    return csr_matvec(rows.rowptr, plan["colx"][rank], rows.val, np.concatenate(blocks))


# ---------------------------------------------------------------------------
# the SpMV reference and its bound
@functools.lru_cache(maxsize=None)
def spmv_reference(name):
    """(x, yref, bound): x standard normal (fixed seed), yref the product of
    Hypergraph.laplacian()'s CSR with x in np.longdouble, and per row
    (nnz_i + 1) eps sum_j |a_ij x_j|: the bound of a dot product of nnz_i terms
    summed in any order (Higham, Accuracy and Stability, section 3.1: gamma_n
    with n = nnz_i, here n + 1 for the rounding of yref to fp64)."""
    L = hypergraph(name).laplacian()
    n = L.nrows
    x = np.random.default_rng(20241).standard_normal(n)
    row = np.repeat(np.arange(n), np.diff(L.rowptr))
    prod = L.val.astype(np.longdouble) * x[L.col].astype(np.longdouble)
    yref = np.zeros(n, np.longdouble)
    np.add.at(yref, row, prod)
    absrow = np.zeros(n, np.longdouble)
    np.add.at(absrow, row, np.abs(prod))
    bound = (np.diff(L.rowptr) + 1) * np.longdouble(EPS) * absrow
    for a in (x, yref, bound):
        a.setflags(write=False)
    return x, yref, bound
