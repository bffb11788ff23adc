"""The k-way rebalancing rule (eigkl.h) restated in plain Python, and
the inputs shared by test_kway_rebalance_host.py and test_gpu_kway_rebalance.py:
the device path must agree with the host entry point on the same cases, and the
host entry point with the restatement.  The restatement uses per-net sets and
`sorted`, and nothing from the library; the hypergraph builders and starts of
kway_cases and refine_cases are imported and left as they are."""
import functools

import numpy as np

import kway_cases as kc
import refine_cases as rc
import refine_w_cases as wc

INT32_MAX = 2 ** 31 - 1
KS = (2, 3, 63, 64, 65, 128, 129, 256)
INTS = ("k", "rounds", "moves", "total_weight", "bound_min", "bound_max", "parts_over_before", "parts_over_bound",
        "excess_before", "excess", "connectivity_w_before", "connectivity_w", "cut_nets", "connectivity", "soed",
        "part_w_min", "part_w_max")


def prepared(net_ptr, pins, net_w):
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


def excess(S, L):
    return sum(max(0, s - l) for s, l in zip(S, L))


def rebal_ref(nodes, net_ptr, pins, node_w, net_w, part, k, eps=0.03, bounds=None, max_rounds=0):
    """(part, round log, bounds, rounds) by the rule of §21.  rounds: per logged round a dict with the part weights at
    its start (S), the evicted nodes per source (evicted), the moved nodes (moved) and the state after it (part)."""
    part = [int(p) for p in part]
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    nets, cw, on = prepared(net_ptr, pins, net_w)
    L = [wc.uniform_bound(sum(w), k, eps)] * k if bounds is None else [int(x) for x in bounds]
    S = [0] * k
    for v in range(nodes):
        S[part[v]] += w[v]
    log, rounds = [], []
    while excess(S, L) > 0:
        lam = [{part[v] for v in net} for net in nets]
        gain, target = {}, {}
        for v in range(nodes):
            a = part[v]
            if S[a] <= L[a] or w[v] <= 0:
                continue
            mine = on.get(v, [])
            D = sum(cw[e] for e in mine)
            r = sum(cw[e] for e in mine if sum(1 for u in nets[e] if part[u] == a) == 1)
            fits = [b for b in range(k) if b != a and S[b] + w[v] <= L[b]]
            if not fits:
                continue
            g, b = max(((r - D) + sum(cw[e] for e in mine if b in lam[e]), -b) for b in fits)
            gain[v], target[v] = g, -b
        rank = {v: (-gain[v], v) for v in gain}  # smaller is better
        evicted = {}
        for a in range(k):
            x, acc = S[a] - L[a], 0
            for v in sorted((v for v in gain if part[v] == a), key=rank.get):
                if acc >= x:  # the shortest prefix that reaches the excess
                    break
                acc += w[v]
                evicted.setdefault(a, []).append(v)
        out = [v for vs in evicted.values() for v in vs]
        moved = []
        for b in range(k):
            acc = 0
            for v in sorted((v for v in out if target[v] == b), key=rank.get):
                if acc + w[v] > L[b] - S[b]:  # the longest prefix that fits
                    break
                acc += w[v]
                moved.append(v)
        if not moved:
            break
        at_start = list(S)
        for v in moved:
            S[part[v]] -= w[v]
            S[target[v]] += w[v]
            part[v] = target[v]
        log.append((len(gain), len(out), len(moved), excess(S, L)))
        rounds.append(dict(S=at_start, evicted=evicted, moved=moved, part=np.array(part, np.int32)))
        if len(log) == max_rounds:
            break
    return np.array(part, np.int32), np.array(log, np.int64).reshape(-1, 4), L, rounds


def _case(nodes, nets, node_w, net_w, start, k, eps=0.03, bounds=None, max_rounds=0, **expect):
    """expect: log (the whole log), final (the returned vector), node0 (the returned part of node 0), over (the
    result's parts_over_bound)."""
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    pins = np.array([p for x in nets for p in x], np.int32)
    return dict(nodes=nodes, ptr=ptr, pins=pins,
                node_w=None if node_w is None else np.ascontiguousarray(node_w, np.int32),
                net_w=None if net_w is None else np.ascontiguousarray(net_w, np.int32),
                start=np.ascontiguousarray(start, np.int32), k=k, eps=eps,
                bounds=None if bounds is None else np.ascontiguousarray(bounds, np.int64), max_rounds=max_rounds,
                expect=expect)


def _graph_case(g, start, k, seed, over=1, unit=False, slack=12, **kw):
    """Random weights (node 0..7 or all 1, net 1..9) on a hypergraph, explicit bounds: `over` of the parts that weigh
    at least 2 get half their weight, the others a slack below `slack` (over = -1: all parts but the lightest)."""
    nodes, ptr, pins = g
    rng = np.random.default_rng(seed)
    node_w = np.ones(nodes, np.int64) if unit else rng.integers(0, 8, nodes)
    out = _case(nodes, [], node_w, rng.integers(1, 10, len(ptr) - 1), start, k, **kw)
    out["ptr"], out["pins"] = ptr, pins
    S = np.bincount(np.asarray(start), weights=node_w, minlength=k).astype(np.int64)
    bounds = S + rng.integers(0, slack, k)
    heavy = np.flatnonzero(S >= 2)
    if over < 0:
        chosen = [p for p in heavy if p != int(np.argmin(S))]
    else:
        chosen = rng.choice(heavy, min(over, len(heavy), k - 1), replace=False)  # (some part has to take weight)
    for p in chosen:
        bounds[p] = S[p] // 2
    rest = [p for p in range(k) if p not in set(int(c) for c in chosen)]
    if len(chosen) and rest:
        bounds[rest[int(np.argmin(S[rest]))]] += 8  # every node (w <= 7) fits the lightest of the others
    out["bounds"] = bounds.astype(np.int64)
    return out


def lone(weights, start, k, bounds, **kw):
    """Nodes on no net: every g is 0, the rank order is the id order and the target is the smallest part that fits."""
    return _case(len(weights), [], weights, None, start, k, bounds=bounds, **kw)


@functools.lru_cache(maxsize=None)
def built_cases():
    """name -> case dict: the shapes at which the kernels of a round can go wrong."""
    out = {}
    small = rc.small_hypergraphs()
    # gain kernel: k at the lane and mask-word edges, every part id in use; one to three parts over
    g = small["random"]
    for i, k in enumerate(KS):
        out[f"gain-k{k}-perm"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 300 + k, over=1 + i % 3)
        out[f"gain-k{k}-edge"] = _graph_case(g, rc.starts(g[0], k)["edge"], k, 400 + k, over=1 + (i + 1) % 3)
    # node counts around a wave's 64, the last three nodes on no net
    for n in (63, 64, 65, 129):
        _, ptr, pins = kc.random_hypergraph(20 + n, nodes=n - 3, nets=n + n // 2)
        out[f"gain-n{n}"] = _graph_case((n, ptr, pins), rc.starts(n, 3)["perm"], 3, 500 + n, over=2, slack=40)
    # degrees 0, 1, 64, 65 and 130 (the incidence chunk of the gain kernel)
    g = small["hubs"]
    for k in (2, 3, 64):
        out[f"hubs-k{k}"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 600 + k, over=1)
    # nets of 2, 63, 64, 65 and 300 pins (the masks kernel), repeated pins in the raw input
    rng = np.random.default_rng(8)
    nets = [rng.choice(320, s, replace=False).tolist() for s in (2, 63, 64, 65, 300, 64, 65)]
    nets[1] = nets[1] + nets[1][:5]  # 63 distinct pins, five of them twice
    nets += [[5, 5, 9], [7, 7], [11]]
    nets += [rng.choice(320, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(330)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    g = (321, ptr, np.array([p for x in nets for p in x], np.int32))  # node 320 is on no net
    for k, over in ((2, 1), (4, -1), (65, 3)):
        out[f"nets-k{k}"] = _graph_case(g, rc.starts(321, k)["perm"], k, 700 + k, over=over)
    # n = 2, and equal g inside one net: the smaller id ranks first.  g = -(2^31 - 1): the biased gain is 1, not 0
    out["gain-n2-min"] = _case(2, [[0, 1]], [1, 1], [INT32_MAX], [0, 0], 2, bounds=[1, 2], final=[1, 0],
                               log=[(2, 1, 1, 0)])
    # g = 2^31 - 1 at node 0: the key is 2^64 - 1
    out["gain-n2-max"] = _case(2, [[0, 1]], [1, 1], [INT32_MAX], [0, 1], 2, bounds=[0, 2], final=[1, 1],
                               log=[(1, 1, 1, 0)])
    # target ties across a mask word: the smaller b; part 0's bound is 0
    for lo, hi, k in ((1, 2, 3), (63, 64, 65), (127, 128, 129), (191, 192, 256)):
        out[f"tie-{lo}-{hi}"] = _case(3, [[0, 1], [0, 2]], [1, 1, 1], [5, 5], [0, hi, lo], k,
                                      bounds=[0] + [9] * (k - 1), max_rounds=1, node0=lo)
    # zero rounds: no part over (the vector comes back untouched); every part over (no proposer)
    g = small["random"]
    c = _graph_case(g, rc.starts(g[0], 4)["perm"], 4, 800, over=0)
    c["expect"] = dict(log=[], final=c["start"].tolist(), over=0)
    out["none-over"] = c
    out["all-over"] = lone([5, 5, 5], [0, 1, 2], 3, [1, 1, 1], log=[], final=[0, 1, 2], over=3)
    # no net at all, and no net of two distinct pins
    out["no-nets"] = lone([2, 2, 1, 1], [0, 1, 0, 1], 3, [1, 1, 10], log=[(4, 2, 2, 0)], final=[2, 2, 0, 1])
    out["no-real-nets"] = _case(5, [[2], [4, 4]], [1, 1, 1, 1, 1], [3, 3], [0, 0, 0, 0, 1], 3, bounds=[2, 1, 1],
                                log=[(4, 2, 1, 1)], final=[2, 0, 0, 0, 1], over=1)
    # all parts but one over
    out["all-but-one-over"] = out["no-nets"]
    # eviction: the running sum hits x exactly; overshoots by w - 1; the proposers weigh less than x (and node 2 fits
    # nowhere); a node of weight 0 in an overweight part never proposes
    out["evict-exact"] = lone([2, 3, 4, 1], [0, 0, 0, 0], 2, [5, 100], log=[(4, 2, 2, 0)], final=[1, 1, 0, 0])
    out["evict-overshoot"] = lone([4, 4, 1, 1], [0, 0, 0, 0], 2, [5, 100], log=[(4, 2, 2, 0)], final=[1, 1, 0, 0])
    out["evict-short"] = lone([3, 3, 9], [0, 0, 0], 2, [2, 7], log=[(2, 2, 2, 7)], final=[1, 1, 0], over=1)
    out["evict-zero-weight"] = lone([0, 2, 2], [0, 0, 0], 2, [2, 10], log=[(2, 1, 1, 0)], final=[0, 1, 0])
    # acceptance: room 0 at part 1; room equal to the first node's weight, the part full after round 1; two sources
    # compete for part 2, the lower-ranked source's node is turned down and goes to part 3 in round 2
    out["accept-room-0"] = lone([2, 2, 5, 1], [0, 0, 1, 2], 3, [2, 5, 10], log=[(2, 1, 1, 0)], final=[2, 0, 1, 2])
    out["accept-room-first"] = lone([3, 3, 1], [0, 0, 0], 2, [1, 3], log=[(3, 2, 1, 3)], final=[1, 0, 0], over=1)
    out["accept-two-sources"] = lone([2, 2, 1, 1], [0, 1, 0, 1], 4, [1, 1, 2, 10], log=[(4, 2, 1, 2), (2, 1, 1, 0)],
                                     final=[2, 3, 0, 1])
    out["max-rounds-1"] = lone([2, 2, 1, 1], [0, 1, 0, 1], 4, [1, 1, 2, 10], max_rounds=1, log=[(4, 2, 1, 2)],
                               final=[2, 1, 0, 1], over=1)
    # one heavy node alone above the bound: stuck
    out["stuck"] = lone([10, 1, 1], [0, 1, 1], 2, [5, 5], log=[], final=[0, 1, 1], over=1)
    # a bound of 0: the part empties
    out["bound-zero"] = lone([1, 1], [0, 0], 2, [0, 5], log=[(2, 2, 2, 0)], final=[1, 1])
    # unit weights under the uniform bound: a skewed start
    g = small["random"]
    skew = np.minimum(np.arange(g[0]) * 7 // g[0], 3).astype(np.int32)  # part 3 holds four sevenths
    c = _case(g[0], [], None, None, skew, 4, eps=0.0)
    c["ptr"], c["pins"] = g[1], g[2]
    out["unit-weights"] = c
    out["unit-weights-k64"] = _graph_case(g, rc.starts(g[0], 64)["perm"], 64, 900, over=3, unit=True)
    for name, c in out.items():
        if "log" not in c["expect"]:
            _, log, _, _ = reference(name, c)
            assert len(log) >= 1, f"{name}: the restatement logs no round"
    return out


@functools.lru_cache(maxsize=None)
def random_cases():
    """30 seeded hypergraphs, n <= 300, k <= 8, mixed weights, explicit bounds that put one to three parts over."""
    out = {}
    for seed in range(30):
        rng = np.random.default_rng(6000 + seed)
        n, k = int(rng.integers(20, 301)), int(rng.integers(2, 9))
        g = kc.random_hypergraph(6100 + seed, nodes=n, nets=int(rng.integers(n // 2, 2 * n)))
        start = rng.integers(0, k, n).astype(np.int32)
        c = _graph_case(g, start, k, 6200 + seed, over=1 + seed % 3)
        name = f"random-{seed}"
        _, log, _, _ = reference(name, c)
        assert len(log) >= 1, f"{name}: the restatement logs no round"  # a vacuous case fails collection
        out[name] = c
    return out


_REFS = {}


def reference(name, case):
    """rebal_ref of a case, computed once and shared (treat it as read-only)."""
    if name not in _REFS:
        _REFS[name] = rebal_ref(case["nodes"], case["ptr"], case["pins"], case["node_w"], case["net_w"], case["start"],
                                case["k"], case["eps"], case["bounds"], case["max_rounds"])
    return _REFS[name]


def all_cases():
    return {**built_cases(), **random_cases()}


def hypergraph(ek, case):
    return wc.hypergraph(ek, case)


def run(call, h, case, **over):
    kw = dict(max_rounds=case["max_rounds"])
    kw.update(over)
    return call(h, case["start"], case["k"], case["eps"], case["bounds"], **kw)


def check_expect(case, part, res, log):
    e = case["expect"]
    if "log" in e:
        assert log.tolist() == [list(x) for x in e["log"]], log.tolist()
    if "node0" in e:
        assert part[0] == e["node0"]
    if "final" in e:
        assert part.tolist() == e["final"]
    assert res["parts_over_bound"] == e.get("over", res["parts_over_bound"])


def check_properties(ek, h, case, ref, part, res, log):
    """The promises of §21, for a run (host or device) that agrees with the restatement `ref`."""
    k, start = case["k"], case["start"]
    _, _, L, rounds = ref
    L = np.asarray(L, np.int64)
    w = np.ones(case["nodes"], np.int64) if case["node_w"] is None else case["node_w"].astype(np.int64)
    before, w0 = ek.kway_metrics_w_host(h, start, k)
    after, w1 = ek.kway_metrics_w_host(h, part, k)
    # no quality promise: both values are reported as recounted
    assert res["connectivity_w_before"] == before[2]
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == after
    assert len(log) == res["rounds"] == len(rounds) and res["moves"] == int(log[:, 2].sum())
    # progress: a logged round has proposers >= evicted >= moved >= 1
    assert np.all(log[:, 0] >= log[:, 1]) and np.all(log[:, 1] >= log[:, 2]) and np.all(log[:, 2] >= 1)
    # X falls by at least 1 a round, so the run ends within X_0 rounds
    xs = [int(np.maximum(w0 - L, 0).sum())] + log[:, 3].tolist()
    assert res["excess_before"] == xs[0] and res["excess"] == xs[-1] == int(np.maximum(w1 - L, 0).sum())
    assert all(b < a for a, b in zip(xs, xs[1:])) and res["rounds"] <= xs[0]
    assert res["parts_over_before"] == int(np.count_nonzero(w0 > L))
    assert res["parts_over_bound"] == int(np.count_nonzero(w1 > L))
    assert (res["part_w_min"], res["part_w_max"]) == (int(w1.min()), int(w1.max()))
    assert (res["bound_min"], res["bound_max"]) == (int(L.min()), int(L.max()))
    assert res["total_weight"] == int(w0.sum()) == int(w1.sum())
    if res["rounds"] == 0:
        assert np.array_equal(part, start)
    if case["max_rounds"] > 0:
        assert res["rounds"] <= case["max_rounds"]
    for r in rounds:
        S0 = np.asarray(r["S"], np.int64)
        S1 = np.bincount(r["part"], weights=w, minlength=k).astype(np.int64)
        over = S0 > L
        assert np.all(S1[~over] <= L[~over])  # parts in bound stay there
        assert np.all(S1[over] <= S0[over])   # overweight parts only shrink
        for a, vs in r["evicted"].items():
            assert over[a]
            gone = [v for v in vs if v in r["moved"]]
            assert S1[a] == S0[a] - sum(int(w[v]) for v in gone)  # ... and never receive
            assert S1[a] > L[a] - max(int(w[v]) for v in vs)      # bounded overshoot
            if case["node_w"] is None or np.all(w == 1):          # unit weights
                assert len(vs) <= S0[a] - L[a] and S1[a] >= L[a]
    # stuck parts, by brute force over the final state
    if not (case["max_rounds"] > 0 and res["rounds"] == case["max_rounds"]):
        for v in range(case["nodes"]):
            a = int(part[v])
            if w1[a] > L[a] and w[v] > 0:
                assert not any(b != a and w1[b] + w[v] <= L[b] for b in range(k)), (v, a)
