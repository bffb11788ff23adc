"""Shared cases of the FM refinement tests (test_fm_host.py, test_gpu_fm.py):
small hypergraphs with a starting side vector and opts, and the plain-Python
restatement of the rule (eigkl.h) both entries are held to.

C is the device pass's chunk size (node ids per chunk key), T its workgroup's
threads, LDS_CHUNKS the chunk count above which its keys leave LDS: stated
here once, and test_fm_host.py holds them to the package's and the source's."""
import functools
import math

import numpy as np

C = 256
T = 512
LDS_CHUNKS = 2048


def pack(nets):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    pins = np.array([p for x in nets for p in x], np.int32)
    return ptr, pins


def random_nets(rng, nodes, count, lo=2, hi=12, among=None):
    """count nets of lo..hi distinct pins among `among` (default: all nodes)."""
    pool = np.arange(nodes) if among is None else np.asarray(among)
    return [rng.choice(pool, int(rng.integers(lo, min(hi, len(pool)) + 1)), replace=False).tolist()
            for _ in range(count)]


def planted_hill():
    """Nodes 0, 1 on side 0 joined by three parallel nets, each tied by two nets
    to two side-1 anchors (2, 3 and 4, 5) that a side-1 clique holds in place;
    6 .. 11 are side-0 padding on no net, so L_max = 6 leaves side 1 room for
    two more.  g(0) = g(1) = 2 - 3 = -1 and every anchor has g = 1 - 3 = -2:
    no single move gains, moving 0 and 1 takes the cut from 4 to 0."""
    nets = [[0, 1]] * 3 + [[0, 2], [0, 3], [1, 4], [1, 5]]
    nets += [[a, b] for a in range(2, 6) for b in range(a + 1, 6)]
    side = np.array([0, 0, 1, 1, 1, 1] + [0] * 6, np.uint8)
    return 12, nets, side


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (nodes, net_ptr, pins, side, eps, max_passes, stall)."""
    out = {}

    def add(name, nodes, nets, side, eps=0.03, max_passes=0, stall=1000):
        ptr, pins = pack(nets)
        side = np.ascontiguousarray(side, np.uint8)
        assert len(side) == nodes and name not in out
        out[name] = (nodes, ptr, pins, side, eps, max_passes, stall)

    # node counts
    add("n2_room", 2, [[0, 1]], [0, 1], eps=1.0)
    add("n2_full", 2, [[0, 1]], [0, 1], eps=0.0)
    add("n3", 3, [[0, 1], [1, 2], [0, 2]], [0, 1, 0], eps=0.0)
    for n in (C - 1, C, C + 1, 2 * C + 1):
        rng = np.random.default_rng(100 + n)
        nets = random_nets(rng, n, n, 2, 6) + [[0, n - 1], [n - 2, n - 1, 1]]  # (the last ids are on nets)
        add(f"n{n}", n, nets, rng.integers(0, 2, n), eps=0.1, stall=30)
    # net sizes 2, 8, 9, 63, 64, 65, 1025 and all n pins, over small nets that give the moves something to gain
    rng = np.random.default_rng(7)
    n = 1100
    nets = [rng.choice(n, k, replace=False).tolist() for k in (2, 8, 9, 63, 64, 65, 1025)] + [list(range(n))]
    nets += random_nets(rng, n, 500, 2, 4)
    add("netsizes", n, nets, (np.arange(n) * 7919 % 11 < 5), eps=0.1, stall=25)
    # the big nets almost on one side: their counts pass through 1 and 0
    side = np.zeros(n, np.uint8)
    side[rng.choice(n, 12, replace=False)] = 1
    add("netsizes_critical", n, nets, side, eps=1.0, max_passes=2, stall=25)
    # repeated pins, single-pin nets, empty nets
    rng = np.random.default_rng(8)
    nets = random_nets(rng, 90, 120, 2, 5)
    for e in range(0, 120, 7):
        nets[e] = nets[e] + [nets[e][0], nets[e][-1]]  # repeated pins: they count once
    nets[3] = [5, 5, 5]                                # one distinct pin: the net takes no part
    nets += [[17], [], [], [40], [41, 41]]
    nets.insert(10, [])
    add("degenerate", 90, nets, rng.integers(0, 2, 90), eps=0.1)
    add("nonets", 10, [], [0, 1] * 5, eps=0.5)
    add("onlydead", 6, [[1], [], [2, 2]], [0, 0, 0, 1, 1, 1], eps=0.5)
    # isolated nodes (every third id is on no net) and a hub on more nets than the workgroup has threads
    rng = np.random.default_rng(9)
    n = 3 * (T + 90)
    live = [v for v in range(n) if v % 3]
    hub = live[5]
    nets = [[hub] + rng.choice([v for v in live if v != hub], 2, replace=False).tolist() for _ in range(T + 88)]
    nets += random_nets(rng, n, 300, 2, 5, among=live)
    assert sum(hub in x for x in nets) > T
    add("hub", n, nets, rng.integers(0, 2, n), eps=0.05, stall=40)
    # all tied: a ring of 2-pin nets over contiguous halves; the even one at eps 0 has both sides full
    for n, eps in ((100, 0.0), (101, 0.0), (100, 0.1), (2 * C + 2, 0.05)):
        add(f"ring{n}_eps{eps}", n, [[i, (i + 1) % n] for i in range(n)], (np.arange(n) >= n // 2), eps=eps,
            stall=0 if n == 101 else 1000)
    # everything on one side; a start above L_max
    rng = np.random.default_rng(10)
    nets = random_nets(rng, 300, 320, 2, 8)
    add("all_side0", 300, nets, np.zeros(300), eps=0.03)
    add("all_side1", 300, nets, np.ones(300), eps=0.03, stall=0)
    add("over_limit", 300, nets, (np.arange(300) >= 250), eps=0.03, stall=50)
    # stall and pass limits
    side = rng.integers(0, 2, 300)
    for stall in (0, 1, 3):
        for max_passes in (0, 1):
            add(f"stall{stall}_passes{max_passes}", 300, nets, side, eps=0.1, max_passes=max_passes, stall=stall)
    # random hypergraphs
    for n, seed, stall in ((600, 21, 60), (2 * C + 5, 22, 60)):
        rng = np.random.default_rng(seed)
        nets = random_nets(rng, n, n, 2, 12)
        side = rng.integers(0, 2, n)
        if n % 2:  # (odd n: eps 0 leaves one node of slack whichever way the draw falls)
            side[:] = rng.permutation(np.arange(n) % 2)
        for eps in (0.0, 0.03, 0.25):
            add(f"random{n}_eps{eps}", n, nets, side, eps=eps, stall=stall)
    rng = np.random.default_rng(23)
    add("random350_default", 350, random_nets(rng, 350, 350, 2, 12), rng.integers(0, 2, 350))
    # the planted hill
    n, nets, side = planted_hill()
    add("hill", n, nets, side, eps=0.03)
    # the last size whose chunk keys are in LDS and the first whose keys are in global memory: a few hundred
    # live nodes spread over the id range (the first and the last chunk included), every other node on no net
    for n in (LDS_CHUNKS * C, LDS_CHUNKS * C + 1):
        rng = np.random.default_rng(31)
        live = np.unique(np.concatenate([rng.choice(n, 400, replace=False), [0, 1, C - 1, C, n - C - 1, n - 2, n - 1]]))
        nets = random_nets(rng, n, 450, 2, 5, among=live) + [[0, n - 1], [n - 2, n - 1, C]]
        add(f"keys_{'lds' if n == LDS_CHUNKS * C else 'global'}_n{n}", n, nets, (np.arange(n) * 31 % 7 < 3), eps=0.03,
            stall=40)
    return out


def names():
    return list(cases())


def max_part(nodes, eps):
    return math.floor((1.0 + eps) * float((nodes + 1) // 2))


def live_nets(ptr, pins):
    """The nets that take part: at least 2 distinct pins, each pin once (first occurrence)."""
    nets = []
    for e in range(len(ptr) - 1):
        s = list(dict.fromkeys(int(p) for p in pins[ptr[e]:ptr[e + 1]]))
        if len(s) >= 2:
            nets.append(s)
    return nets


@functools.lru_cache(maxsize=None)
def reference(name):
    """fm_ref of a case, computed once and shared (treat it as read-only)."""
    nodes, ptr, pins, side, eps, max_passes, stall = cases()[name]
    return fm_ref(nodes, ptr, pins, side, eps, max_passes, stall)


def fm_ref(nodes, ptr, pins, side, eps, max_passes=0, stall=1000):
    """The rule restated with dicts and sets: every count and every gain from scratch at every move, every choice
    a min over tuples.  Returns (side, pass_log rows, move_log rows, result integers)."""
    nets = live_nets(ptr, pins)
    on = {}
    for e, s in enumerate(nets):
        for v in s:
            on.setdefault(v, []).append(e)
    lmax = max_part(nodes, eps)
    side = [int(x) for x in side]
    size = [side.count(0), side.count(1)]

    def counts():
        out = []
        for s in nets:
            ones = sum(side[v] for v in s)
            out.append((len(s) - ones, ones))
        return out

    def cut_of(cnt):
        return sum(1 for c in cnt if c[0] and c[1])

    cut = cut_before = cut_of(counts())
    pass_log, move_log = [], []
    passes = 0
    while not (max_passes > 0 and passes >= max_passes):
        free = set(on)
        trail = [(cut, abs(size[0] - size[1]))]
        moved = []
        while True:
            cnt = counts()
            gain = {v: sum((cnt[e][side[v]] == 1) - (cnt[e][1 - side[v]] == 0) for e in on[v]) for v in free}
            cands = []
            for a in (0, 1):
                mine = [v for v in free if side[v] == a]
                if size[1 - a] < lmax and mine:
                    v = min(mine, key=lambda v: (-gain[v], v))
                    cands.append((-gain[v], -size[a], v))
            if not cands:
                break
            neg, _, v = min(cands)
            a = side[v]
            side[v] = 1 - a
            size[a] -= 1
            size[1 - a] += 1
            free.discard(v)
            moved.append(v)
            cut += neg
            trail.append((cut, abs(size[0] - size[1])))
            move_log.append((v, -neg, cut))
            if stall > 0 and len(moved) - trail.index(min(trail)) >= stall:
                break
        best = trail.index(min(trail))  # the least t of the least (c, d)
        for v in moved[best:]:
            size[side[v]] -= 1
            side[v] = 1 - side[v]
            size[side[v]] += 1
        cut = trail[best][0]
        assert cut == cut_of(counts())
        pass_log.append((len(moved), best, cut, trail[best][1]))
        if best == 0:
            break
        passes += 1
    res = {"n": nodes, "max_part": lmax, "passes": passes, "passes_run": len(pass_log),
           "moves_tried": len(move_log), "moves_kept": sum(r[1] for r in pass_log), "cut_before": cut_before,
           "cut": cut, "n0": size[0], "n1": size[1]}
    return (np.array(side, np.uint8), np.array(pass_log, np.int64).reshape(-1, 4), move_log, res)


RESULT_INTS = ("n", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut", "n0", "n1")


def same(got, want):
    """(side, pass_log, move_log, result) of two runs: equal sides, logs and result integers.  want's move log may
    be rows of tuples (the restatement's) or the structured array."""
    side, plog, mlog, res = got
    wside, wplog, wmlog, wres = want
    assert np.array_equal(side, wside), int(np.count_nonzero(side != wside))
    assert np.array_equal(plog, wplog), (plog.tolist()[:4], np.asarray(wplog).tolist()[:4])
    rows = [tuple(int(x) for x in r) for r in (wmlog.tolist() if hasattr(wmlog, "dtype") else wmlog)]
    assert [tuple(int(x) for x in r) for r in mlog.tolist()] == rows
    assert {k: res[k] for k in RESULT_INTS} == {k: wres[k] for k in RESULT_INTS}
