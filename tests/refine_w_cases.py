"""The weighted k-way refinement rule (eigkl.h) restated in plain
Python, and the inputs shared by test_kway_refine_w_host.py and
test_gpu_kway_refine_w.py: the device path must agree with the host entry
point on the same cases, and the host entry point with the restatement.  The
hypergraphs and starts of refine_cases and kwayml_cases are imported and left
as they are."""
import functools

import numpy as np

import kway_cases as kc
import kwayml_cases as km
import refine_cases as rc

INT32_MAX = 2 ** 31 - 1
GAIN_KS = (2, 3, 64, 65, 128, 129, 192, 193, 256)
INTS = ("k", "rounds", "moves", "gain_total", "total_weight", "bound_min", "bound_max", "part_w_min", "part_w_max",
        "parts_over_bound", "connectivity_w_before", "cut_nets", "connectivity", "connectivity_w", "soed")
# what ek_kway_refine_w's result shares with ek_kway_refine's under unit weights and no bounds
SHARED_WITH_UNWEIGHTED = {"k": "k", "rounds": "rounds", "moves": "moves", "gain_total": "gain_total",
                          "bound_max": "max_part", "bound_min": "max_part", "part_w_min": "part_min",
                          "part_w_max": "part_max", "connectivity_w_before": "connectivity_before",
                          "cut_nets": "cut_nets", "connectivity": "connectivity", "connectivity_w": "connectivity",
                          "soed": "soed"}


def uniform_bound(W, k, eps):
    return rc.max_part(W, k, eps)


def synthetic_weights(nodes, nets):
    """§12's synthetic weights: node 1 + id mod 5, net 1 + e mod 3."""
    return (1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32)


def refine_w_ref(nodes, net_ptr, pins, node_w, net_w, part, k, eps=0.03, max_rounds=0, bounds=None):
    """(part, round log, bounds) by the rule of §17, with sets and dicts; only the nodes on a net are walked, so a
    case with millions of isolated nodes costs what its nets cost."""
    part = np.array(part, np.int64)
    w = np.ones(nodes, np.int64) if node_w is None else np.asarray(node_w, np.int64)
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
    W = int(w.sum())
    L = [uniform_bound(W, k, eps)] * k if bounds is None else [int(x) for x in bounds]
    S = [int(x) for x in np.bincount(part, weights=w.astype(np.float64), minlength=k)] if W < 2 ** 52 else None
    if S is None:  # (float sums would round)
        S = [0] * k
        for v in range(nodes):
            S[int(part[v])] += int(w[v])
    log = []
    while max_rounds <= 0 or len(log) < max_rounds:
        phi = []
        for net in nets:
            f = {}
            for v in net:
                f[int(part[v])] = f.get(int(part[v]), 0) + 1
            phi.append(f)
        gain, target = {}, {}
        for v in sorted(on):
            a = int(part[v])
            D = sum(cw[e] for e in on[v])
            r = sum(cw[e] for e in on[v] if phi[e][a] == 1)
            c = {}  # c[b] = the weight of v's nets with a pin in b
            for e in on[v]:
                for b in phi[e]:
                    c[b] = c.get(b, 0) + cw[e]
            best = None
            for b in range(k):
                if b == a or S[b] + int(w[v]) > L[b]:
                    continue
                g = (r - D) + c.get(b, 0)
                if best is None or g > best[0]:
                    best = (g, b)
            if best is not None and best[0] > 0:
                gain[v], target[v] = best
        winner = [min((v for v in net if v in gain), key=lambda v: (-gain[v], v), default=None) for net in nets]
        independent = [v for v in gain if all(winner[e] == v for e in on[v])]
        accepted = []
        for b in range(k):
            mine = sorted((v for v in independent if target[v] == b), key=lambda v: (-gain[v], v))
            acc = 0
            for v in mine:  # the longest prefix that fits: the first node that does not ends the part's intake
                if acc + int(w[v]) > L[b] - S[b]:
                    break
                acc += int(w[v])
                accepted.append(v)
        if not accepted:
            break
        for v in accepted:
            S[int(part[v])] -= int(w[v])
            S[target[v]] += int(w[v])
            part[v] = target[v]
        log.append((len(gain), len(independent), len(accepted), sum(gain[v] for v in accepted)))
    return part.astype(np.int32), np.array(log, np.int64).reshape(-1, 4), L


def _case(nodes, nets, node_w, net_w, start, k, eps=0.03, max_rounds=0, bounds=None, moved=None):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    pins = np.array([p for x in nets for p in x], np.int32)
    return dict(nodes=nodes, ptr=ptr, pins=pins,
                node_w=None if node_w is None else np.ascontiguousarray(node_w, np.int32),
                net_w=None if net_w is None else np.ascontiguousarray(net_w, np.int32),
                start=np.ascontiguousarray(start, np.int32), k=k, eps=eps, max_rounds=max_rounds,
                bounds=None if bounds is None else np.ascontiguousarray(bounds, np.int64), moved=moved)


def pairs(spec, room, max_rounds=1, moved=None, k=2):
    """m disjoint 2-pin nets (v_i, a_i), v_i in part 0, a_i in part 1 (ids after the last v), net weight g_i: every
    v_i that fits is an independent candidate for part 1 with gain g_i and weight w_i.  spec: (id, g, w) triples;
    the ids in between are isolated filler nodes of part 0.  bounds[0] = S(0) closes part 0 (every a_i weighs 1),
    bounds[1] = S(1) + room.  moved: the ids the first round must move."""
    ids = [s[0] for s in spec]
    assert ids == sorted(set(ids))
    m = len(spec)
    first_a = ids[-1] + 1
    nodes = first_a + m
    node_w = np.ones(nodes, np.int32)
    start = np.zeros(nodes, np.int32)
    start[first_a:] = 1
    nets, net_w = [], []
    for i, (v, g, wv) in enumerate(spec):
        node_w[v] = wv
        nets.append([v, first_a + i])
        net_w.append(g)
    S0 = int(node_w[:first_a].astype(np.int64).sum())
    bounds = [S0, m + room] + [0] * (k - 2)
    return _case(nodes, nets, node_w, net_w, start, k, max_rounds=max_rounds, bounds=bounds, moved=moved)


def _weighted(nodes, ptr, pins, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 8, nodes).astype(np.int32), rng.integers(1, 10, len(ptr) - 1).astype(np.int32)


def _graph_case(g, start, k, seed, **kw):
    nodes, ptr, pins = g
    node_w, net_w = _weighted(nodes, ptr, pins, seed)
    out = _case(nodes, [], node_w, net_w, start, k, **kw)
    out["ptr"], out["pins"] = ptr, pins
    return out


@functools.lru_cache(maxsize=None)
def built_cases():
    """name -> case dict: the shapes at which the kernels of a round can go wrong."""
    out = {}
    small = rc.small_hypergraphs()
    # gain kernel: k at the lane and mask-word edges, random weights, every part id in use
    for k in GAIN_KS:
        g = small["random"]
        out[f"gain-k{k}-perm"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 300 + k, eps=4.0)
        out[f"gain-k{k}-edge"] = _graph_case(g, rc.starts(g[0], k)["edge"], k, 400 + k, eps=4.0)
    # nets of 8 | 9, 64 | 65 and 300 pins, node degrees around 50 (one round: the restatement is slow there)
    g = small["metrics"]
    for k in (3, 65):
        out[f"metrics-k{k}"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 450 + k, eps=0.5, max_rounds=1)
    # node counts around a wave's 64
    for n in (63, 64, 65, 200):
        g = kc.random_hypergraph(20 + n, nodes=n, nets=n + n // 2)
        out[f"gain-n{n}"] = _graph_case(g, rc.starts(n, 3)["perm"], 3, 500 + n, eps=0.3)
    # degrees 0, 1, 64, 65 and 130 (the incidence chunk); nets of 2, 8, 9, 64, 65, 200 pins and a repeated pin
    g = small["hubs"]
    for k in (2, 3, 64):
        out[f"hubs-k{k}"] = _graph_case(g, rc.starts(g[0], k)["perm"], k, 600 + k, eps=0.2)
    rng = np.random.default_rng(8)
    nets = [rng.choice(260, s, replace=False).tolist() for s in (2, 8, 9, 64, 65, 200)]
    nets += [[5, 5, 9], [7, 7], [11]]
    nets += [rng.choice(260, int(rng.integers(2, 7)), replace=False).tolist() for _ in range(330)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    g = (261, ptr, np.array([p for x in nets for p in x], np.int32))  # node 260 is on no net
    for k in (2, 4, 65):
        out[f"nets-k{k}"] = _graph_case(g, rc.starts(261, k)["perm"], k, 700 + k, eps=0.3)
    g = km.metrics_hypergraph()
    c = _case(g[0], [], g[3], g[4], rc.starts(g[0], 4)["perm"], 4, eps=0.1)
    c["ptr"], c["pins"] = g[1], g[2]
    out["kwayml-metrics-k4"] = c
    # ties between two targets of equal g: the smaller b, also across a 64-part word
    for lo, hi, k in ((1, 2, 3), (63, 64, 65), (127, 128, 129), (191, 192, 256)):
        start = [0, hi, lo]  # node 1 in the greater part: the order of the nets must not decide
        out[f"tie-{lo}-{hi}"] = _case(3, [[0, 1], [0, 2]], [1, 1, 1], [5, 5], start, k, bounds=[1] + [9] * (k - 1),
                                      max_rounds=1, moved={0: lo})
    # the fit test closes part 1 for the heavy node and opens it for the light one in the same round
    out["fit-heavy-light"] = pairs([(0, 9, 10), (1, 4, 1)], room=5, moved={1})
    # D(v) = 2^31 - 1: (r - D) + c stays inside int32, r + c would not
    out["gain-int32-max"] = _case(3, [[0, 1], [0, 2]], [1, 1, 1], [2 ** 30, 2 ** 30 - 1], [0, 1, 1], 2,
                                  bounds=[1, 9], max_rounds=1, moved={0: 1})
    # select kernel: threshold and room
    five = [(i, 9 - i, i + 1) for i in range(5)]  # weights 1..5, gains 9..5
    out["select-all-fit"] = pairs(five, room=15, moved={0, 1, 2, 3, 4})
    out["select-room-exact"] = pairs(five, room=6, moved={0, 1, 2})
    out["select-room-one-short"] = pairs(five, room=5, moved={0, 1})
    B = 2 ** 30
    for j in (0, 8, 16, 24):  # the first rejected key parts from the last accepted one in key byte 4 + j / 8
        spec = [(0, B + 3 * 2 ** j, 1), (1, B + 2 * 2 ** j, 1), (2, B + 2 ** j, 1), (3, B, 1), (4, 3, 1)]
        out[f"select-gbit{j}"] = pairs(spec, room=2, moved={0, 1})
    for j in (0, 8, 16):  # ... and in key byte j / 8 (equal gains: the ids decide)
        ids = [1, 2, 2 + 2 ** j, 3 + 2 ** j]
        out[f"select-idbit{j}"] = pairs([(v, 7, 1) for v in ids], room=2, moved={1, 2})
    # select kernel: weights
    ws = [2, 3, 0, 0, 4, 0, 1]
    out["select-zero-weights"] = pairs([(i, 20 - i, x) for i, x in enumerate(ws)], room=5, moved={0, 1, 2, 3})
    heavy = [(0, 9, 3), (1, 8, 4), (2, 7, 1), (3, 6, 1)]  # node 1 fits by itself, not after node 0
    out["select-prefix-not-greedy"] = pairs(heavy, room=5, moved={0})
    out["select-prefix-later-rounds"] = pairs(heavy, room=5, max_rounds=0)
    big = [(i, 9 - i, INT32_MAX - i) for i in range(5)]
    out["select-sums-past-2^32"] = pairs(big, room=3 * INT32_MAX - 3, moved={0, 1, 2})
    out["select-sums-past-2^32-short"] = pairs(big, room=3 * INT32_MAX - 4, moved={0, 1})
    # select kernel: bounds
    out["select-room-zero"] = pairs([(0, 9, 0), (1, 8, 1), (2, 7, 0)], room=0, moved={0, 2})
    out["select-overfull"] = pairs([(0, 9, 0), (1, 8, 1)], room=-1, moved=set())
    g = small["random"]
    start = rc.starts(g[0], 4)["perm"]
    c = _graph_case(g, start, 4, 801)
    S = np.bincount(start, weights=c["node_w"], minlength=4).astype(np.int64)
    c["bounds"] = np.array([0, S[1] + 7, 10 ** 12, S[3]], np.int64)  # over-full, a little room, open, room 0
    out["bounds-distinct"] = c
    # apply kernel: every part gives and receives in one round.  Disjoint 2-pin nets (v, a), v in part p and a in part
    # p + 1 or p + 2 (mod k), every v before every a: each v wins its net (equal gains, the smaller id) and moves
    k, per = 5, 6
    m = k * per
    start = [i // per for i in range(m)] + [(i // per + 1 + i % 2) % k for i in range(m)]
    rng = np.random.default_rng(9)
    out["apply-ring-k5"] = _case(2 * m, [[i, m + i] for i in range(m)], rng.integers(0, 8, 2 * m),
                                 rng.integers(1, 10, m), start, k, eps=1.0, max_rounds=1,
                                 moved={i: (i // per + 1 + i % 2) % k for i in range(m)})
    return out


def id_byte3_case():
    """select-idbit24: the first rejected id differs from the last accepted one at bit 24, so the node count passes
    2^24 (isolated filler nodes in between).  Apart from built_cases: the tests that walk every node in Python leave
    it out."""
    ids = [1, 2, 2 + 2 ** 24, 3 + 2 ** 24]
    return pairs([(v, 7, 1) for v in ids], room=2, moved={1, 2})


def hypergraph(ek, case):
    h = ek.Hypergraph.from_pins(case["nodes"], case["ptr"], case["pins"])
    if case["node_w"] is not None or case["net_w"] is not None:
        h.set_weights(case["node_w"], case["net_w"])
    return h


def circuit_cases():
    """(id, circuit, weights, start name, k, eps, max_rounds)"""
    out = []
    for wt in ("synthetic", "ones"):
        out.append((f"fract-{wt}-block-k4-e0.05", "fract", wt, "block", 4, 0.05, 0))
        out.append((f"fract-{wt}-block-k4-e0.0", "fract", wt, "block", 4, 0.0, 0))
        out.append((f"fract-{wt}-perm-k3-e0.05", "fract", wt, "perm", 3, 0.05, 0))
        out.append((f"fract-{wt}-perm-k64-e0.5", "fract", wt, "perm", 64, 0.5, 0))
        out.append((f"fract-{wt}-edge-k65-e0.05", "fract", wt, "edge", 65, 0.05, 0))
        out.append((f"ibm01-{wt}-block-k8-e0.03-r4", "ibm01", wt, "block", 8, 0.03, 4))
        out.append((f"ibm01-{wt}-perm-k256-e0.05-r1", "ibm01", wt, "perm", 256, 0.05, 1))
        out.append((f"ibm01-{wt}-edge-k63-e0.5-r2", "ibm01", wt, "edge", 63, 0.5, 2))
    return out


BINDING = "fract-synthetic-block-k4-e0.05"  # the bound binds: accepted < independent in some round


def check_properties(ek, h, start, k, bounds, part, res, log):
    """What every run must satisfy, host or device.  bounds: the k values L_p the run was under."""
    L = np.asarray(bounds, np.int64)
    before, w0 = ek.kway_metrics_w_host(h, start, k)
    after, w1 = ek.kway_metrics_w_host(h, part, k)
    assert res["connectivity_w_before"] == before[2]
    assert (res["cut_nets"], res["connectivity"], res["connectivity_w"], res["soed"]) == after
    assert before[2] - after[2] == res["gain_total"] == int(log[:, 3].sum())
    assert len(log) == res["rounds"] and res["moves"] == int(log[:, 2].sum())
    assert np.all(log[:, 2] >= 1) and np.all(log[:, 3] >= log[:, 2])
    assert np.all(log[:, 0] >= log[:, 1]) and np.all(log[:, 1] >= log[:, 2])
    assert np.all(w1 <= np.maximum(L, w0)), (w1.tolist(), L.tolist(), w0.tolist())
    assert res["parts_over_bound"] == int(np.count_nonzero(w1 > L))
    assert (res["part_w_min"], res["part_w_max"]) == (int(w1.min()), int(w1.max()))
    assert (res["bound_min"], res["bound_max"]) == (int(L.min()), int(L.max()))
    assert res["total_weight"] == int(w0.sum()) == int(w1.sum())
    assert res["moves"] >= int(np.count_nonzero(np.asarray(part) != np.asarray(start)))
