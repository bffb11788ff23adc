"""mr_cases.py on the CPU: the in-process communicator the sharded GPU tests run
their ranks through, the shard maps, the numpy restatement of the halo layout
against the dense Laplacian, and that each edge test_gpu_mr_small.py is there
for is attained by a case it runs (so a later edit cannot hollow it out)."""
import threading
import time

import numpy as np
import pytest

import lanczos_cases as lc
import mr_cases as mc


def _threads(world, body):
    out, err = [None] * world, [None] * world

    def run(r):
        try:
            out[r] = body(r)
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    ts = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(30)
    assert not any(t.is_alive() for t in ts)
    return out, err


@pytest.mark.parametrize("world", [1, 2, 3, 4, 17])
def test_lockstep_allgather_is_in_rank_order_and_counted(world):
    comm = mc.LockstepComm(world, timeout=20, record=True)

    def body(r):
        got = []
        for k in range(3):  # (back to back: a rank may not post its next block before all took this one)
            got.append(comm.allgather(r, np.array([10.0 * k + r, -1.0 - r])))
        return got

    out, err = _threads(world, body)
    assert err == [None] * world
    for r in range(world):
        for k in range(3):
            assert np.array_equal(out[r][k], np.array([[10.0 * k + q, -1.0 - q] for q in range(world)]).ravel())
        assert comm.calls[r] == {"allgather": 3, "allreduce": 0}
        assert comm.doubles[r] == {"allgather": 6, "allreduce": 0}
        assert [list(b) for b in comm.sent[r]] == [[10.0 * k + r, -1.0 - r] for k in range(3)]


def test_lockstep_allreduce_same_bits_on_every_rank():
    """Operands whose sum depends on the order: 1 + 2^-53 + 2^-53 - 1 is 0 from
    the left and 2^-52 when the small terms meet first.  Every rank must hold
    the left-to-right sum from rank 0."""
    world = 4
    vals = np.array([[1.0, 1e16, 0.1], [2.0 ** -53, 1.0, 0.2], [2.0 ** -53, -1e16, 0.3], [-1.0, 1.0, 0.4]])
    want = vals[0].copy()
    for r in range(1, world):
        want += vals[r]
    assert want[0] == 0.0 and (vals[1, 0] + vals[2, 0]) + (vals[0, 0] + vals[3, 0]) != 0.0  # order matters here
    comm = mc.LockstepComm(world, timeout=20)

    def body(r):
        buf = vals[r].copy()
        comm.allreduce(r, buf)
        return buf

    out, err = _threads(world, body)
    assert err == [None] * world
    for r in range(world):
        assert out[r].tobytes() == want.tobytes()
        assert comm.calls[r] == {"allgather": 0, "allreduce": 1} and comm.doubles[r]["allreduce"] == 3


def test_lockstep_failed_rank_releases_the_others():
    """Rank 1 raises instead of joining: ranks 0 and 2, already waiting, raise
    RankAborted at once (well inside the timeout), and so does any later call."""
    world = 3
    comm = mc.LockstepComm(world, timeout=20)
    t0 = time.monotonic()

    def body(r):
        if r == 1:
            comm.abort()  # what run_ranks does for a rank that raised
            raise ValueError("rank 1 failed")
        return comm.allgather(r, np.zeros(2))

    _, err = _threads(world, body)
    assert time.monotonic() - t0 < 10
    assert isinstance(err[1], ValueError)
    assert isinstance(err[0], mc.RankAborted) and isinstance(err[2], mc.RankAborted)
    with pytest.raises(mc.RankAborted):
        comm.allreduce(0, np.zeros(1))


def test_lockstep_missing_rank_times_out():
    """A rank that never comes (a deadlock in the code under test): the barrier's
    timeout breaks it for the ranks that wait."""
    comm = mc.LockstepComm(2, timeout=0.2)
    _, err = _threads(1, lambda r: comm.allgather(0, np.zeros(1)))
    assert isinstance(err[0], mc.RankAborted) and comm.broken


def test_lockstep_mismatched_collectives_fail():
    comm = mc.LockstepComm(2, timeout=20)
    _, err = _threads(2, lambda r: comm.allgather(r, np.zeros(1 + r)))
    assert all(isinstance(e, (AssertionError, mc.RankAborted)) for e in err) and any(
        isinstance(e, AssertionError) for e in err)


def test_every_map_tiles_the_rows():
    seen = set()
    for name, world, key, off in mc.all_cases():
        n = mc.graph(name)[0]
        assert len(off) == world + 1 and off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0), (name, key, off)
        seen.add(key)
    assert {"equal", "first1", "last1", "mid_empty", "last_empty", "lib", "lmax0", "gt1023", "gt1024",
            "gt1025"} <= seen
    for world in (3, 4):
        m = mc.maps(65, world)
        assert np.diff(m["mid_empty"])[1] == 0 and np.diff(m["last_empty"])[-1] == 0
        assert np.diff(m["first1"])[0] == 1 and np.diff(m["last1"])[-1] == 1
    assert np.all(np.diff(mc.WORLD17[1]) > 0) and len(mc.WORLD17[1]) == 18


@pytest.fixture(scope="module")
def plans():
    """(name, world, map name) -> (off, rows, plan) of every explicit and library map."""
    out = {}
    for name, world, key, off in mc.all_cases():
        rows = mc.rows_of(name, off)
        out[(name, world, key)] = (off, rows, mc.halo_plan(off, rows, mc.slot_dims(off)[0]))
    return out


def test_sharded_numpy_spmv_against_the_dense_laplacian(plans):
    """Both layouts of the restatement against the rows of dense_laplacian(name) @ x
    (taken in np.longdouble) within mr_cases.spmv_reference's bound; the halo
    layout gives the slot layout's bits."""
    for (name, world, key), (off, rows, plan) in plans.items():
        x, yref, bound = mc.spmv_reference(name)
        ydense = mc.dense_laplacian(name).astype(np.longdouble) @ x.astype(np.longdouble)
        assert np.all(np.abs(yref - ydense) <= bound), (name, "the CSR reference against the dense one")
        for r in range(world):
            lo, hi = int(off[r]), int(off[r + 1])
            y_slot = mc.sharded_spmv(plan, r, rows[r], x, halo=False)
            y_halo = mc.sharded_spmv(plan, r, rows[r], x, halo=True)
            assert y_slot.shape == (hi - lo,)
            assert y_halo.tobytes() == y_slot.tobytes(), (name, world, key, r)
            assert np.all(np.abs(y_slot - ydense[lo:hi]) <= bound[lo:hi]), (name, world, key, r)
            for seg in (plan["colh"][r][a:b] for a, b in zip(rows[r].rowptr[:-1], rows[r].rowptr[1:])):
                assert np.all(np.diff(seg) > 0)  # the compact map is monotone: rows stay sorted


def test_halo_plan_is_consistent(plans):
    """What one rank sends is what the other expects: message sizes, the place
    of each message in the sender's buffer, and every partial at its block end."""
    for (name, world, key), (off, rows, plan) in plans.items():
        C, ldv = plan["C"], plan["ldv"]
        assert plan["slot"] == ldv + 64 and ldv % mc.GT_ROWS == 0 and ldv >= np.diff(off).max() > ldv - mc.GT_ROWS
        rng = np.random.default_rng(3)
        blocks = [mc.slot_block(plan, q, rng.standard_normal(int(off[q + 1] - off[q])), 100.0 + q)
                  for q in range(world)]
        for r in range(world):
            assert len(plan["sidx"][r]) == sum(C[q, r] + 1 for q in range(world) if q != r) <= plan["smax"]
            X = mc.halo_x(plan, r, blocks)
            assert np.array_equal(X[plan["pidx"][r]], 100.0 + np.arange(world))
            g = plan["gidx"][r]
            xg = np.concatenate([b[:int(off[q + 1] - off[q])] for q, b in enumerate(blocks)])
            assert np.array_equal(X[g >= 0], xg[g[g >= 0]]) and np.array_equal(np.flatnonzero(g < 0), plan["pidx"][r])
            assert mc.exchange_doubles(plan, r, True)[1] == len(X) - (off[r + 1] - off[r]) - 1


def test_each_edge_is_attained(plans):
    """The edges the GPU cases are chosen for, over the cases the GPU tests run."""
    hit = {k: [] for k in ("C0", "lmax0", "reads_all", "src_nonzero", "req_offset_two_terms", "auto_halo",
                           "auto_slot", "max1023", "max1024", "max1025", "one_row", "empty", "soff_after_first",
                           "two_row_blocks")}
    for case, (off, rows, plan) in plans.items():
        W, C, nr = plan["world"], plan["C"], np.diff(off)
        if any(C[r, q] == 0 for r in range(W) for q in range(W) if r != q):
            hit["C0"].append(case)
        if plan["lmax"] == 0:
            hit["lmax0"].append(case)
        if any(C[r, q] == nr[q] > 0 for r in range(W) for q in range(W) if r != q):
            hit["reads_all"].append(case)
        if any(plan["src"][r][q] != 0 for r in range(W) for q in range(W)):
            hit["src_nonzero"].append(case)
        # the start of r's request from `me` inside r's list: sum over q < me, q != r, of C[r][q]
        if any(sum(1 for q in range(me) if q != r and C[r, q] > 0) >= 2 for me in range(W) for r in range(W)
               if r != me):
            hit["req_offset_two_terms"].append(case)
        if any(plan["soff"][me][r] > 1 for me in range(W) for r in range(W) if r != me):
            hit["soff_after_first"].append(case)  # (a first peer's message of at least one row before it)
        hit["auto_halo" if plan["auto"] else "auto_slot"].append(case)
        for m in (1023, 1024, 1025):
            if nr.max() == m:
                hit[f"max{m}"].append(case)
        if plan["ldv"] == 2 * mc.GT_ROWS:
            hit["two_row_blocks"].append(case)
        if np.any(nr == 1):
            hit["one_row"].append(case)
        if np.any(nr == 0):
            hit["empty"].append(case)
    for k, v in hit.items():
        print(k, len(v), v[:3])
    assert all(hit.values()), [k for k, v in hit.items() if not v]
    assert all(c[1] >= 3 for c in hit["src_nonzero"] + hit["req_offset_two_terms"])  # (zero at 2 ranks)
    # a star's hub row and K_n read every row of a peer
    assert any(c[0] == "star-65" for c in hit["reads_all"]) and any(c[0] == "complete-8" for c in hit["reads_all"])
    assert ("paths-40+60", 2, "lmax0") in hit["lmax0"]
    assert (mc.LADDER, 2, "ladder") in hit["auto_slot"]  # (see mr_cases.LADDER)


def test_world17_takes_the_slot_layout():
    name, off = mc.WORLD17
    assert len(off) - 1 > mc.MAX_HALO_RANKS
    rows = mc.rows_of(name, off)
    plan = mc.halo_plan(off, rows, mc.slot_dims(off)[0])
    assert plan["auto"]  # the counts alone would pick the halo layout: the rank limit decides
