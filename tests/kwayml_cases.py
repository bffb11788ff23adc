"""Shared by test_kwayml_host.py and test_gpu_kwayml.py: the per-side bounds
the tests use, and the bounded sweep and FM rules (eigkl.h)
restated in plain Python.  The cases come from sweepw_cases and fmw_cases,
which are imported and left as they are."""
import math

import numpy as np

import fmw_cases as fw
import sweep_cases as sc
import sweepw_cases as sw

RATIOS = ((2, 1), (3, 2))
EPSILONS = (0.0, 0.03)
SWEEP_INTS = tuple("bound0" if k == "max_part" else k for k in sw.INTS) + ("bound1",)
FM_INTS = tuple("bound0" if k == "max_part" else k for k in fw.RESULT_INTS) + ("bound1",)


def symmetric(W, eps):
    """L0 = L1 = floor((1 + eps) ceil(W / 2)), clamped to W as the entries ask."""
    lmax = min(W, sw.max_part(W, eps))
    return lmax, lmax


def ratio_bounds(W, ratio, eps):
    """L_s = floor((1 + eps) ceil(W r_s / (r_0 + r_1))), clamped to W: r_0 : r_1 of W with slack eps."""
    tot = sum(ratio)
    return tuple(min(W, math.floor((1.0 + eps) * float(-(-W * r // tot)))) for r in ratio)


def all_bounds(W):
    """The unequal bounds the tests run every case under: 2 : 1 and 3 : 2 of W at eps 0 and 0.03."""
    return [ratio_bounds(W, r, eps) for r in RATIOS for eps in EPSILONS]


def total_weight(nodes, node_w):
    return nodes if node_w is None else int(np.asarray(node_w, np.int64).sum())


def sweepwb_ref(nodes, net_ptr, pins, node_w, net_w, v, bounds):
    """The bounded sweep by the rule: split s is feasible iff P[s] <= L1 and W - P[s] <= L0; the balance key is
    D = |(W - P[s] - L0) - (P[s] - L1)|; feasible: least (profile_w, D, s); none feasible: least (D, profile_w, s)."""
    n = nodes
    L0, L1 = (int(x) for x in bounds)
    key = sc.ord_keys(v)
    order = sorted(range(n), key=lambda i: (key[i], i))
    pos = {node: r for r, node in enumerate(order)}
    w = [1] * n if node_w is None else [int(x) for x in node_w]
    profw = [0] * (n + 1)
    prof = [0] * (n + 1)
    spanning = 0
    for e in range(len(net_ptr) - 1):
        ranks = {pos[int(p)] for p in pins[net_ptr[e]:net_ptr[e + 1]]}
        if len(ranks) < 2:
            continue
        spanning += 1
        for s in range(min(ranks) + 1, max(ranks) + 1):
            profw[s] += 1 if net_w is None else int(net_w[e])
            prof[s] += 1
    P = [0]
    for i in order:
        P.append(P[-1] + w[i])
    W = P[n]

    def D(s):
        return abs((W - P[s] - L0) - (P[s] - L1))
    window = [s for s in range(1, n) if P[s] <= L1 and W - P[s] <= L0]
    if window:
        best = min(window, key=lambda s: (profw[s], D(s), s))
    else:
        best = min(range(1, n), key=lambda s: (D(s), profw[s], s))
    res = {"n": n, "n0": n - best, "n1": best, "s_lo": window[0] if window else 0, "s_hi": window[-1] if window else 0,
           "feasible": 1 if window else 0, "total_weight": W, "bound0": L0, "bound1": L1, "w0": W - P[best],
           "w1": P[best], "cut": profw[best], "cut_nets": prof[best], "cut_half": profw[n // 2],
           "spanning_nets": spanning}
    return res, np.array(order, np.int32), np.array(profw, np.int64), np.array(P, np.int64)


def fmwb_ref(nodes, ptr, pins, node_w, net_w, side, bounds, max_passes=0, stall=1000):
    """The bounded FM by the rule, with dicts and sets, every count and gain from scratch at every move: side a's
    top node is a candidate iff S[1 - a] + w(top) <= L[1 - a]; of two, the greater g, then the side of less slack
    (greater S_a - L_a), then the smaller id; d = |(S0 - L0) - (S1 - L1)|.  Returns (side, pass_log, move_log,
    result integers)."""
    nets = fw.live_nets(ptr, pins, net_w)
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    L = [int(x) for x in bounds]
    on = {}
    for e, (s, _) in enumerate(nets):
        for v in s:
            on.setdefault(v, []).append(e)
    total = sum(w)
    side = [int(x) for x in side]
    S = [sum(w[v] for v in range(nodes) if side[v] == a) for a in (0, 1)]

    def D():
        return abs((S[0] - L[0]) - (S[1] - L[1]))

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
        trail = [(cut, D())]
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
                    if S[1 - a] + w[top] <= L[1 - a]:
                        cands.append((-gain[top], -(S[a] - L[a]), top))
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
            trail.append((cut, D()))
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
    res = {"n": nodes, "total_weight": total, "bound0": L[0], "bound1": L[1], "passes": passes,
           "passes_run": len(pass_log), "moves_tried": len(move_log), "moves_kept": sum(r[1] for r in pass_log),
           "cut_before": cut_before, "cut": cut, "cut_nets_before": cut_nets_before, "cut_nets": cut_nets_of(counts()),
           "w0": S[0], "w1": S[1], "n0": side.count(0), "n1": side.count(1)}
    return (np.array(side, np.uint8), np.array(pass_log, np.int64).reshape(-1, 4), move_log, res)


def same_sweep(got, want):
    res, order, profw, prefix = got
    wres, worder, wprofw, wprefix = want
    assert np.array_equal(order, worder) and np.array_equal(profw, wprofw) and np.array_equal(prefix, wprefix)
    assert {k: res[k] for k in SWEEP_INTS} == {k: wres[k] for k in SWEEP_INTS}


def same_fm(got, want):
    fw.same(got, want, FM_INTS)


def kway_metrics_w_ref(nodes, ptr, pins, node_w, net_w, part, k):
    """((cut nets, connectivity, weighted connectivity, SOED), part weights), counted plainly: lambda_e is the number
    of distinct parts among net e's pins (every net of the file, as ek_kway_metrics_host takes them)."""
    cut = conn = connw = soed = 0
    for e in range(len(ptr) - 1):
        lam = len({int(part[int(p)]) for p in pins[ptr[e]:ptr[e + 1]]})
        if lam >= 2:
            cut += 1
            conn += lam - 1
            connw += (1 if net_w is None else int(net_w[e])) * (lam - 1)
            soed += lam
    pw = [0] * k
    for v in range(nodes):
        pw[int(part[v])] += 1 if node_w is None else int(node_w[v])
    return (cut, conn, connw, soed), pw


def metrics_hypergraph(seed=7, nodes=700):
    """(nodes, net_ptr, pins, node_w, net_w): nets of 1, 2, 8 | 9 and 64 | 65 pins (the kernel's thread / wave
    hand-over at 8 and a wave's full stride at 64), a repeated pin, an empty net, and random nets between."""
    rng = np.random.default_rng(seed)
    nets = [rng.choice(nodes, s, replace=False).tolist() for s in (1, 2, 8, 9, 64, 65, 300)]
    nets += [[5, 5, 9], []]
    nets += [rng.choice(nodes, int(rng.integers(2, 12)), replace=False).tolist() for _ in range(600)]
    ptr, pin = sw.pack(nets)
    return nodes, ptr, pin, rng.integers(0, 8, nodes).astype(np.int32), rng.integers(1, 10, len(nets)).astype(np.int32)
