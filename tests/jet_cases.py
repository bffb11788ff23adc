"""The Jet refinement rule (eigkl.h) restated in plain Python, and
the inputs shared by test_kway_jet_host.py and test_gpu_kway_jet.py: the device
path must agree with the host entry point on the same cases, and the host entry
point with the restatement.  The hypergraphs, starts and select cases of
kway_cases, refine_cases and refine_w_cases are imported and left as they are."""
import functools

import numpy as np

import kway_cases as kc
import refine_cases as rc
import refine_w_cases as wc

INT32_MAX = 2 ** 31 - 1
KS = (2, 3, 63, 64, 65, 128, 129, 256)
INTS = ("k", "iters", "best_iter", "moves", "total_weight", "bound_min", "bound_max", "connectivity_w_before",
        "cut_nets", "connectivity", "connectivity_w", "soed", "part_w_min", "part_w_max", "parts_over_bound")


def prepared(nodes, net_ptr, pins, net_w):
    """The nets of >= 2 distinct pins, each pin once, with their weights; and the nets of every node on one."""
    nets, cw = [], []
    for e in range(len(net_ptr) - 1):
        distinct = sorted({int(p) for p in pins[net_ptr[e]:net_ptr[e + 1]]})
        if len(distinct) >= 2:
            nets.append(distinct)
            cw.append(1 if net_w is None else int(net_w[e]))
    on = {}
    for e, net in enumerate(nets):
        for v in net:
            on.setdefault(v, []).append(e)
    return nets, cw, on


def connectivity_w(nets, cw, part):
    return sum(c * (len({int(part[v]) for v in net}) - 1) for net, c in zip(nets, cw))


def jet_ref(nodes, net_ptr, pins, node_w, net_w, part, k, eps=0.03, bounds=None, max_iters=0, patience=12, neg=(1, 4)):
    """(snapshot, iteration log, bounds, best_iter, the states after every iteration) by the rule of §18, with sets
    and dicts; only the nodes on a net are walked."""
    part = [int(p) for p in part]
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    nets, cw, on = prepared(nodes, net_ptr, pins, net_w)
    W = sum(w)
    L = [wc.uniform_bound(W, k, eps)] * k if bounds is None else [int(x) for x in bounds]
    S = [0] * k
    for v in range(nodes):
        S[part[v]] += w[v]
    num, den = neg
    snapshot, best, best_iter, since, last = list(part), connectivity_w(nets, cw, part), 0, 0, 0
    locked, log, states = set(), [], []
    while nets:
        phi = []
        for net in nets:
            f = {}
            for v in net:
                f[part[v]] = f.get(part[v], 0) + 1
            phi.append(f)
        gain, target = {}, {}
        for v in sorted(on):
            if v in locked:
                continue
            a = part[v]
            D = sum(cw[e] for e in on[v])
            r = sum(cw[e] for e in on[v] if phi[e][a] == 1)
            c = {}
            for e in on[v]:
                for b in phi[e]:
                    c[b] = c.get(b, 0) + cw[e]
            open_parts = [b for b in range(k) if b != a and S[b] + w[v] <= L[b]]
            if not open_parts:
                continue
            g, b = max(((r - D) + c.get(b, 0), -b) for b in open_parts)
            if g >= 0 or -g * den < num * (D - r):
                gain[v], target[v] = g, -b
        rank = {v: (-gain[v], v) for v in gain}  # smaller is better
        passing = []
        for v in gain:
            a, t, g2 = part[v], target[v], 0
            for e in on[v]:
                held = [target[u] if u in rank and rank[u] < rank[v] else part[u] for u in nets[e] if u != v]
                g2 += cw[e] * (int(a not in held) - int(t not in held))
            if g2 >= 0:
                passing.append(v)
        accepted = []
        for b in range(k):
            acc = 0
            for v in sorted((v for v in passing if target[v] == b), key=rank.get):
                if acc + w[v] > L[b] - S[b]:  # the longest prefix that fits
                    break
                acc += w[v]
                accepted.append(v)
        for v in accepted:
            S[part[v]] -= w[v]
            S[target[v]] += w[v]
            part[v] = target[v]
        locked = set(accepted)
        X = connectivity_w(nets, cw, part)
        log.append((len(gain), len(passing), len(accepted), X))
        states.append(list(part))
        i = len(log)
        if X < best:
            best, best_iter, snapshot, since = X, i, list(part), 0
        else:
            since += 1
        idle = not accepted and last == 0
        last = len(accepted)
        if since == patience or i == max_iters or idle:
            break
    return (np.array(snapshot, np.int32), np.array(log, np.int64).reshape(-1, 4), L, best_iter,
            [np.array(s, np.int32) for s in states])


def _case(nodes, nets, node_w, net_w, start, k, eps=0.03, bounds=None, max_iters=0, patience=12, neg=(1, 4), **expect):
    """expect: first (node -> part: the moves of the only iteration, which must improve unless there are none), final
    (the returned vector), log (the whole log), best_iter, node0 (the returned part of node 0)."""
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    pins = np.array([p for x in nets for p in x], np.int32)
    return dict(nodes=nodes, ptr=ptr, pins=pins,
                node_w=None if node_w is None else np.ascontiguousarray(node_w, np.int32),
                net_w=None if net_w is None else np.ascontiguousarray(net_w, np.int32),
                start=np.ascontiguousarray(start, np.int32), k=k, eps=eps,
                bounds=None if bounds is None else np.ascontiguousarray(bounds, np.int64), max_iters=max_iters,
                patience=patience, neg=neg, expect=expect)


def _graph_case(g, start, k, seed, **kw):
    nodes, ptr, pins = g
    rng = np.random.default_rng(seed)
    out = _case(nodes, [], rng.integers(0, 8, nodes), rng.integers(1, 10, len(ptr) - 1), start, k, **kw)
    out["ptr"], out["pins"] = ptr, pins
    return out


def _from_w(c, **kw):
    """A case of refine_w_cases as a Jet case."""
    out = _case(c["nodes"], [], c["node_w"], c["net_w"], c["start"], c["k"], eps=c["eps"], bounds=c["bounds"], **kw)
    out["ptr"], out["pins"] = c["ptr"], c["pins"]
    return out


def escape_case(c_xy=8, c_out=7, **kw):
    """x = 0 and y = 1 in part 0 on a net of weight c_xy; nets {x, p} and {y, q} of weight c_out, p = 2 and q = 3
    held in part 1 by nets of weight 20 to 4 and 5.  With 8 and 7: g(x) = g(y) = -1 passes the 1/4 filter (4 < 8);
    x ranks first (the smaller id) and fails the afterburner (y stays: -8 + 7), y sees x moved (8 + 7 = 15) and moves
    alone, X rises from 14 to 15; iteration 2 moves x (g = 15), X = 0."""
    nets = [[0, 1], [0, 2], [1, 3], [2, 4], [3, 5]]
    return _case(6, nets, [1] * 6, [c_xy, c_out, c_out, 20, 20], [0, 0, 1, 1, 1, 1], 2, bounds=[6, 6], **kw)


def filter_case(A, B, neg, **kw):
    """v = 0 and y = 1 in part 0 on a net of weight A, v and p = 2 (part 1) on a net of weight B; part 0 is closed
    (its bound is its weight), so only v and y can propose: g(v) = B - A, D - r = A, and y (g = -A, D - r = A) is a
    candidate only when neg_num > neg_den."""
    return _case(3, [[0, 1], [0, 2]], [1, 1, 1], [A, B], [0, 0, 1], 2, bounds=[2, 9], neg=neg, max_iters=1, **kw)


def fit_case(slack, **kw):
    """One node of weight 5 with gain 3 towards part 1, whose bound is S(1) + 5 + slack."""
    return _case(2, [[0, 1]], [5, 2], [3], [0, 1], 2, bounds=[5, 2 + 5 + slack], max_iters=1, **kw)


@functools.lru_cache(maxsize=None)
def built_cases():
    """name -> case dict: the shapes at which the kernels of an iteration can go wrong."""
    out = {}
    small = rc.small_hypergraphs()
    # gain kernel: k at the lane and mask-word edges, every part id in use; 3/4 lets many negative gains through
    g = small["random"]
    for k in KS:
        out[f"gain-k{k}-perm"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 300 + k, eps=4.0, max_iters=4)
        out[f"gain-k{k}-edge"] = _graph_case(g, rc.starts(g[0], k)["edge"], k, 400 + k, eps=4.0, max_iters=3,
                                             neg=(3, 4))
    # node counts around a wave's 64, the last three nodes on no net; n = 2
    for n in (63, 64, 65, 129):
        nodes, ptr, pins = kc.random_hypergraph(20 + n, nodes=n - 3, nets=n + n // 2)
        out[f"gain-n{n}"] = _graph_case((n, ptr, pins), rc.starts(n, 3)["perm"], 3, 500 + n, eps=0.3)
    # ... and equal gains inside one net: node 0 (the smaller id) counts as moved for node 1, which then fails, not the
    # reverse
    out["gain-n2"] = _case(2, [[0, 1]], [1, 1], [3], [0, 1], 2, bounds=[2, 2], final=[1, 1],
                           log=[(2, 1, 1, 0), (0, 0, 0, 0), (0, 0, 0, 0)])
    # degrees 0, 1, 64, 65 and 130 (the incidence chunk of both node kernels)
    g = small["hubs"]
    for k in (2, 3, 64):
        out[f"hubs-k{k}"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 600 + k, eps=0.2, max_iters=6)
    # nets of 2, 63, 64, 65 and 300 pins (the afterburner's lane stride), repeated pins in the raw input
    rng = np.random.default_rng(8)
    nets = [rng.choice(320, s, replace=False).tolist() for s in (2, 63, 64, 65, 300, 64, 65)]
    nets[1] = nets[1] + nets[1][:5]  # 63 distinct pins, five of them twice
    nets += [[5, 5, 9], [7, 7], [11]]
    nets += [rng.choice(320, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(330)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    g = (321, ptr, np.array([p for x in nets for p in x], np.int32))  # node 320 is on no net
    for k, neg in ((2, (1, 4)), (4, (3, 4)), (65, (1, 1))):
        out[f"nets-k{k}"] = _graph_case(g, rc.starts(321, k)["perm"], k, 700 + k, eps=0.3, max_iters=4, neg=neg)
    g = small["metrics"]  # nets of 8 | 9, 64 | 65 and 300 pins, degrees around 50
    out["metrics-k3"] = _graph_case(g, rc.starts(g[0], 3)["perm"], 3, 453, eps=0.5, max_iters=2)
    # a better-ranked candidate that fails the afterburner itself still counts as moved (equal gains again: x by its id)
    out["escape"] = escape_case(final=[1, 1, 1, 1, 1, 1], log=[(2, 1, 1, 15), (1, 1, 1, 0), (0, 0, 0, 0), (0, 0, 0, 0)], best_iter=2)
    # neg_num = 0: g = 0 is still proposed (x: -5 + 5 = 0 passes, y: 5 + 5), g < 0 is not
    out["neg-zero-g0"] = escape_case(5, 5, neg=(0, 1), max_iters=1, first={0: 1, 1: 1}, log=[(2, 2, 2, 0)])
    out["neg-zero-g-1"] = escape_case(8, 7, neg=(0, 1), final=[0, 0, 1, 1, 1, 1], log=[(0, 0, 0, 14)])
    # the filter at -g den = num (D - r), where the node is no candidate, and one below it
    out["filter-1/4-at"] = filter_case(8, 6, (1, 4), first={}, log=[(0, 0, 0, 6)])
    out["filter-1/4-below"] = filter_case(9, 7, (1, 4), log=[(1, 0, 0, 7)])
    out["filter-3/7-at"] = filter_case(7, 4, (3, 7), first={}, log=[(0, 0, 0, 4)])
    out["filter-3/7-below"] = filter_case(5, 3, (3, 7), log=[(1, 0, 0, 3)])
    # the fit test at S + w = L and at L + 1
    out["fit-exact"] = fit_case(0, first={0: 1}, log=[(1, 1, 1, 0)])
    out["fit-one-over"] = fit_case(-1, first={}, log=[(0, 0, 0, 3)])
    # target ties across a mask word: the smaller b
    for lo, hi, k in ((1, 2, 3), (63, 64, 65), (127, 128, 129), (191, 192, 256)):
        c = _case(3, [[0, 1], [0, 2]], [1, 1, 1], [5, 5], [0, hi, lo], k, bounds=[1] + [9] * (k - 1), max_iters=1)
        c["expect"] = dict(node0=lo)
        out[f"tie-{lo}-{hi}"] = c
    # g = -(2^31 - 1): the biased key is 1, not 0; D = 2^31 - 1; then g = 2^31 - 1.  Node 1 moves in iteration 1 (it
    # sees node 0 moved), is locked in 2, where node 0 follows, and free again in 3
    out["gain-int32-extremes"] = _case(2, [[0, 1]], [1, 1], [INT32_MAX], [0, 0], 2, bounds=[2, 2], neg=(2, 1), max_iters=4,
                                       best_iter=0,
                                       log=[(2, 1, 1, INT32_MAX), (1, 1, 1, 0), (1, 0, 0, 0), (2, 1, 1, INT32_MAX)])
    # every select case of the weighted pass, reached through this entry: one iteration over disjoint 2-pin nets
    # accepts what a round of that pass accepts
    for name, c in wc.built_cases().items():
        if (name.startswith("select-") or name == "fit-heavy-light") and c["max_rounds"] == 1:
            moved = c["moved"]
            out[name] = _from_w(c, max_iters=1, first=moved if isinstance(moved, dict) else {v: 1 for v in moved})
    # the stop rule
    out["stop-no-candidate"] = _case(4, [[0, 1], [2, 3]], None, None, [0, 0, 1, 1], 2, log=[(0, 0, 0, 0)])
    g = small["random"]
    for name, kw in (("patience-1", dict(patience=1)), ("iters-1", dict(max_iters=1)), ("iters-2", dict(max_iters=2)),
                     ("rollback", dict(neg=(3, 4), patience=3))):
        out[f"stop-{name}"] = _graph_case(g, rc.starts(g[0], 4)["perm"], 4, 900, eps=0.1, **kw)
    return out


def random_cases():
    """A few dozen seeded hypergraphs, n <= 300, k <= 8, mixed weights, explicit bounds; every third start has a part
    above its bound."""
    out = {}
    for seed in range(30):
        rng = np.random.default_rng(4000 + seed)
        n, k = int(rng.integers(20, 301)), int(rng.integers(2, 9))
        g = kc.random_hypergraph(4100 + seed, nodes=n, nets=int(rng.integers(n // 2, 2 * n)))
        start = rng.integers(0, k, n).astype(np.int32)
        c = _graph_case(g, start, k, 4200 + seed, neg=[(1, 4), (3, 4), (0, 1)][seed % 3], patience=4)
        S = np.bincount(start, weights=c["node_w"], minlength=k).astype(np.int64)
        bounds = S + rng.integers(0, 12, k)
        if seed % 3 == 0:
            bounds[int(rng.integers(0, k))] //= 2
        c["bounds"] = bounds.astype(np.int64)
        out[f"random-{seed}"] = c
    return out


def hypergraph(ek, case):
    return wc.hypergraph(ek, case)


def run(call, h, case, **over):
    kw = dict(max_iters=case["max_iters"], patience=case["patience"], neg=case["neg"])
    kw.update(over)
    return call(h, case["start"], case["k"], case["eps"], case["bounds"], **kw)


def bounds_of(case, res):
    if case["bounds"] is not None:
        return case["bounds"]
    return np.full(case["k"], wc.uniform_bound(res["total_weight"], case["k"], case["eps"]), np.int64)


def check_expect(case, part, res, log):
    e = case["expect"]
    if "log" in e:
        assert log.tolist() == [list(x) for x in e["log"]], log.tolist()
    if "best_iter" in e:
        assert res["best_iter"] == e["best_iter"]
    if "node0" in e:
        assert part[0] == e["node0"]
    if "final" in e:
        assert part.tolist() == e["final"]
    if "first" in e:
        assert case["max_iters"] == 1
        assert {int(v): int(part[v]) for v in np.flatnonzero(part != case["start"])} == e["first"]


def check_properties(ek, h, case, part, res, log):
    """What every run must satisfy, host or device."""
    k, start = case["k"], case["start"]
    L = np.asarray(bounds_of(case, res), np.int64)
    before, w0 = ek.kway_metrics_w_host(h, start, k)
    after, w1 = ek.kway_metrics_w_host(h, part, k)
    assert res["connectivity_w_before"] == before[2]
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == after
    assert len(log) == res["iters"] and res["moves"] == int(log[:, 2].sum())
    assert np.all(log[:, 0] >= log[:, 1]) and np.all(log[:, 1] >= log[:, 2])
    # the result is the best state seen, the start among them; best_iter is the first iteration that reached it
    xs = [before[2]] + log[:, 3].tolist()
    assert after[2] == min(xs) <= before[2] and res["best_iter"] == xs.index(min(xs))
    assert np.all(w1 <= np.maximum(L, w0)), (w1.tolist(), L.tolist(), w0.tolist())
    assert res["parts_over_bound"] == int(np.count_nonzero(w1 > L))
    assert (res["part_w_min"], res["part_w_max"]) == (int(w1.min()), int(w1.max()))
    assert (res["bound_min"], res["bound_max"]) == (int(L.min()), int(L.max()))
    assert res["total_weight"] == int(w0.sum()) == int(w1.sum())
    if case["max_iters"] > 0:
        assert res["iters"] <= case["max_iters"]
    if res["best_iter"] == 0:
        assert np.array_equal(part, start)
