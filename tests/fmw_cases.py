"""Shared cases of the weighted FM refinement tests (test_fmw_host.py,
test_gpu_fmw.py): small weighted hypergraphs with a starting side vector and
opts, and the plain-Python restatement of the weighted rule (eigkl.h,
DESIGN.md §12) both entries are held to.  The structures, the chunk size C,
the workgroup's threads T and LDS_CHUNKS come from fm_cases, which is imported
and left as it is."""
import functools
import math

import numpy as np

import fm_cases as fc

C, T, LDS_CHUNKS = fc.C, fc.T, fc.LDS_CHUNKS
INT32_MAX = 2 ** 31 - 1


def rand_weights(rng, nodes, nets):
    """Node weights in 0..7 (zeros included), net weights in 1..9."""
    return rng.integers(0, 8, nodes).astype(np.int32), rng.integers(1, 10, nets).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (nodes, net_ptr, pins, node_w or None, net_w or None, side, eps, max_passes, stall)."""
    out = {}

    def add(name, nodes, nets, node_w, net_w, side, eps=0.03, max_passes=0, stall=1000):
        ptr, pins = fc.pack(nets)
        side = np.ascontiguousarray(side, np.uint8)
        node_w = None if node_w is None else np.ascontiguousarray(node_w, np.int32)
        net_w = None if net_w is None else np.ascontiguousarray(net_w, np.int32)
        assert len(side) == nodes and name not in out
        assert node_w is None or len(node_w) == nodes
        assert net_w is None or len(net_w) == len(nets)
        out[name] = (nodes, ptr, pins, node_w, net_w, side, eps, max_passes, stall)

    def reuse(name, new, seed, **kw):
        """The structure, the sides and the opts of an fm_cases case under random weights."""
        nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
        nets = [pins[ptr[e]:ptr[e + 1]].tolist() for e in range(len(ptr) - 1)]
        node_w, net_w = rand_weights(np.random.default_rng(seed), nodes, len(nets))
        opts = dict(eps=eps, max_passes=max_passes, stall=stall)
        opts.update(kw)
        add(new, nodes, nets, node_w, net_w, side, **opts)

    # node counts
    add("n2_room", 2, [[0, 1]], [3, 2], [4], [0, 1], eps=1.0)
    add("n2_full", 2, [[0, 1]], [3, 2], [4], [0, 1], eps=0.0)
    add("n3", 3, [[0, 1], [1, 2], [0, 2]], [2, 0, 1], [1, 5, 2], [0, 1, 0], eps=0.0)
    for n in (C - 1, C, C + 1, 2 * C + 1):
        reuse(f"n{n}", f"n{n}", 200 + n)
    # one node holds more than half of W: it never fits on the other side, and at a small eps its own side is
    # above L_max already, so that side never receives either
    rng = np.random.default_rng(41)
    n = 60
    nets = fc.random_nets(rng, n, 90, 2, 5)
    node_w = rng.integers(1, 4, n)
    node_w[7] = 10 * int(node_w.sum())
    side = rng.integers(0, 2, n)
    for s in nets:  # (node 7's nets are uncut, so its gain is the least: it is side 0's top only once the rest is locked)
        if 7 in s:
            side[s] = 0
    add("heavy",n, nets, node_w, rng.integers(1, 10, len(nets)), side, eps=0.03)
    # the top node of side 0 (node 0: g = 4, w = 5) does not fit while node 1 (g = 1, w = 1) would; the tops of
    # side 1 weigh 5 and do not fit either: W = 20, L_max = floor(1.1 * 10) = 11, S = 10 | 10, so nothing moves
    add("top_does_not_fit", 5, [[0, 3], [0, 4], [1, 3], [0, 2], [3, 4]], [5, 1, 4, 5, 5], [3, 2, 1, 1, 4],
        [0, 0, 0, 1, 1], eps=0.1)
    # node 1 (side 0) and node 0 (side 1) both have g = 2; side 0 is heavier (node 2 is padding on no net), so
    # node 1 moves first although its id is the greater one; with equal side weights the smaller id does
    add("tie_heavier_side", 3, [[0, 1]], [1, 1, 3], [2], [1, 0, 0], eps=1.0)
    add("tie_smaller_id", 4, [[0, 1]], [1, 1, 3, 3], [2], [1, 0, 0, 1], eps=1.0)
    # nets of 2, 8, 9, 63, 64, 65 and 1,025 pins at weights > 1; the same almost on one side
    for name in ("netsizes", "netsizes_critical"):
        nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
        nets = [pins[ptr[e]:ptr[e + 1]].tolist() for e in range(len(ptr) - 1)]
        rng = np.random.default_rng(43)
        node_w, net_w = rand_weights(rng, nodes, len(nets))
        net_w[:8] = [2, 3, 4, 5, 6, 7, 9, 8]  # (the seven sized nets and the all-pins net)
        add(name, nodes, nets, node_w, net_w, side, eps=eps, max_passes=max_passes, stall=stall)
    # repeated pins, single-pin nets and empty nets: the weights of the nets that take no part must not shift
    reuse("degenerate", "degenerate", 44)
    reuse("nonets", "nonets", 45)
    reuse("onlydead", "onlydead", 46)
    # a hub on more nets than the workgroup has threads, with mixed net weights
    reuse("hub", "hub", 47)
    # net weights at the int32 bound of the gains: node 0's nets sum to exactly 2^31 - 1
    # (and node 3's: 7 + (2^31 - 8))
    add("gain_bound", 6, [[0, 1], [0, 2], [3, 4], [3, 5]], [1, 2, 1, 0, 3, 1], [2 ** 30, 2 ** 30 - 1, 7, INT32_MAX - 7],
        [0, 1, 1, 0, 1, 1], eps=0.5)
    # a start above L_max; stall and pass limits; eps
    reuse("over_limit", "over_limit", 48)
    for stall in (0, 1, 3):
        for max_passes in (0, 1):
            reuse(f"stall{stall}_passes{max_passes}", f"stall{stall}_passes{max_passes}", 49)
    for eps in (0.0, 0.03, 0.25):
        reuse(f"random600_eps{eps}", f"random600_eps{eps}", 50)
    # node weights only, net weights only
    reuse("random350_default", "node_w_only", 51)
    reuse("random350_default", "net_w_only", 52)
    for name, drop in (("node_w_only", 4), ("net_w_only", 3)):
        row = list(out[name])
        row[drop] = None
        out[name] = tuple(row)
    # the planted hill of fm_cases: with the four nets that bridge the two sides at weight 5 a single move gains
    # (g(0) = 10 - 3); with the three nets that join 0 and 1 at weight 5 the hill is steeper (g(0) = 2 - 15)
    n, nets, side = fc.planted_hill()
    add("hill_bridges5", n, nets, None, [1] * 3 + [5] * 4 + [1] * 6, side)
    add("hill_joins5", n, nets, None, [5] * 3 + [1] * 4 + [1] * 6, side)
    # the last size with the chunk keys in LDS and the first with them in global memory
    for name in (x for x in fc.names() if x.startswith("keys_")):
        nodes, ptr, pins, side, eps, max_passes, stall = fc.cases()[name]
        nets = [pins[ptr[e]:ptr[e + 1]].tolist() for e in range(len(ptr) - 1)]
        rng = np.random.default_rng(53)
        add(name, nodes, nets, rng.integers(1, 4, nodes), rng.integers(1, 3, len(nets)), side, eps=eps,
            max_passes=max_passes, stall=stall)
    return out


def names():
    return list(cases())


def hypergraph(ek, name):
    """The case as a Hypergraph with its weights attached, and (side, eps, max_passes, stall)."""
    nodes, ptr, pins, node_w, net_w, side, eps, max_passes, stall = cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    h.set_weights(node_w, net_w)
    return h, (side, eps, max_passes, stall)


def max_part(total, eps):
    return math.floor((1.0 + eps) * float((total + 1) // 2))


def live_nets(ptr, pins, net_w):
    """The nets that take part with their weights: at least 2 distinct pins, each pin once."""
    nets = []
    for e in range(len(ptr) - 1):
        s = list(dict.fromkeys(int(p) for p in pins[ptr[e]:ptr[e + 1]]))
        if len(s) >= 2:
            nets.append((s, 1 if net_w is None else int(net_w[e])))
    return nets


def metrics(nodes, ptr, pins, node_w, net_w, side):
    """(weighted cut, cut nets, W0, W1), counted plainly."""
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    cut = [c for s, c in live_nets(ptr, pins, net_w) if len({int(side[v]) for v in s}) == 2]
    return (sum(cut), len(cut), sum(w[v] for v in range(nodes) if side[v] == 0),
            sum(w[v] for v in range(nodes) if side[v] == 1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """fmw_ref of a case, computed once and shared (treat it as read-only)."""
    return fmw_ref(*cases()[name])


def fmw_ref(nodes, ptr, pins, node_w, net_w, side, eps, max_passes=0, stall=1000):
    """The weighted rule restated with dicts and sets: every count and every gain from scratch at every move, every
    choice a min over tuples.  Returns (side, pass_log rows, move_log rows, result integers)."""
    nets = live_nets(ptr, pins, net_w)
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    on = {}
    for e, (s, _) in enumerate(nets):
        for v in s:
            on.setdefault(v, []).append(e)
    total = sum(w)
    lmax = max_part(total, eps)
    side = [int(x) for x in side]
    S = [sum(w[v] for v in range(nodes) if side[v] == a) for a in (0, 1)]

    def counts():
        out = []
        for s, _ in nets:
            ones = sum(side[v] for v in s)
            out.append((len(s) - ones, ones))
        return out

    def cut_of(cnt):
        return sum(nets[e][1] for e, c in enumerate(cnt) if c[0] and c[1])

    def cut_nets_of(cnt):
        return sum(1 for c in cnt if c[0] and c[1])

    cut = cut_before = cut_of(counts())
    cut_nets_before = cut_nets_of(counts())
    pass_log, move_log = [], []
    passes = 0
    while not (max_passes > 0 and passes >= max_passes):
        free = set(on)
        trail = [(cut, abs(S[0] - S[1]))]
        moved = []
        while True:
            cnt = counts()
            gain = {v: sum(nets[e][1] * ((cnt[e][side[v]] == 1) - (cnt[e][1 - side[v]] == 0)) for e in on[v])
                    for v in free}
            cands = []
            for a in (0, 1):
                mine = [v for v in free if side[v] == a]
                if mine:
                    top = min(mine, key=lambda v: (-gain[v], v))  # only the top node is tried
                    if S[1 - a] + w[top] <= lmax:
                        cands.append((-gain[top], -S[a], top))
            if not cands:
                break
            neg, _, v = min(cands)
            a = side[v]
            side[v] = 1 - a
            S[a] -= w[v]
            S[1 - a] += w[v]
            free.discard(v)
            moved.append(v)
            cut += neg
            trail.append((cut, abs(S[0] - S[1])))
            move_log.append((v, -neg, cut))
            if stall > 0 and len(moved) - trail.index(min(trail)) >= stall:
                break
        best = trail.index(min(trail))  # the least t of the least (c, d)
        for v in moved[best:]:
            S[side[v]] -= w[v]
            side[v] = 1 - side[v]
            S[side[v]] += w[v]
        cut = trail[best][0]
        assert cut == cut_of(counts())
        pass_log.append((len(moved), best, cut, trail[best][1]))
        if best == 0:
            break
        passes += 1
    res = {"n": nodes, "total_weight": total, "max_part": lmax, "passes": passes, "passes_run": len(pass_log),
           "moves_tried": len(move_log), "moves_kept": sum(r[1] for r in pass_log), "cut_before": cut_before,
           "cut": cut, "cut_nets_before": cut_nets_before, "cut_nets": cut_nets_of(counts()), "w0": S[0], "w1": S[1],
           "n0": side.count(0), "n1": side.count(1)}
    return (np.array(side, np.uint8), np.array(pass_log, np.int64).reshape(-1, 4), move_log, res)


RESULT_INTS = ("n", "total_weight", "max_part", "passes", "passes_run", "moves_tried", "moves_kept", "cut_before", "cut",
               "cut_nets_before", "cut_nets", "w0", "w1", "n0", "n1")


def same(got, want, ints=RESULT_INTS):
    """(side, pass_log, move_log, result) of two runs: equal sides, logs and the result integers named.  want's
    move log may be rows of tuples (the restatement's) or the structured array."""
    side, plog, mlog, res = got
    wside, wplog, wmlog, wres = want
    assert np.array_equal(side, wside), int(np.count_nonzero(side != wside))
    assert np.array_equal(plog, wplog), (plog.tolist()[:4], np.asarray(wplog).tolist()[:4])
    rows = [tuple(int(x) for x in r) for r in (wmlog.tolist() if hasattr(wmlog, "dtype") else wmlog)]
    assert [tuple(int(x) for x in r) for r in mlog.tolist()] == rows
    assert {k: res[k] for k in ints} == {k: wres[k] for k in ints}
