"""The k-way refinement rule restated in plain Python, and the inputs shared by
test_kway_refine_host.py and test_gpu_kway_refine.py (the device path must
agree with the host entry point on the same cases)."""
import math

import numpy as np

import kway_cases as kc

KS = (2, 3, 63, 64, 65, 256)
EPSILONS = (0.0, 0.05, 0.5)


def max_part(n, k, eps):
    return math.floor((1.0 + eps) * float(-(-n // k)))


def refine_ref(nodes, net_ptr, pins, part, k, eps, max_rounds=0):
    """(part, round log, L_max) by the rule of DESIGN.md §9, sets and dicts only."""
    part = [int(p) for p in part]
    nets = []
    for e in range(len(net_ptr) - 1):
        distinct = sorted({int(p) for p in pins[net_ptr[e]:net_ptr[e + 1]]})
        if len(distinct) >= 2:
            nets.append(distinct)
    on = [[] for _ in range(nodes)]
    for e, net in enumerate(nets):
        for v in net:
            on[v].append(e)
    lmax = max_part(nodes, k, eps)
    log = []
    while max_rounds <= 0 or len(log) < max_rounds:
        size = [0] * k
        for p in part:
            size[p] += 1
        phi = []
        for net in nets:
            f = {}
            for v in net:
                f[part[v]] = f.get(part[v], 0) + 1
            phi.append(f)
        gain, target = {}, {}
        for v in range(nodes):
            if not on[v]:
                continue
            a = part[v]
            r = sum(1 for e in on[v] if phi[e][a] == 1)
            c = {}  # c[b] = #{e on v : b in Lambda(e)}
            for e in on[v]:
                for b in phi[e]:
                    c[b] = c.get(b, 0) + 1
            best = None
            for b in range(k):
                if b == a or size[b] >= lmax:
                    continue
                g = r + c.get(b, 0) - len(on[v])
                if best is None or g > best[0]:
                    best = (g, b)
            if best is not None and best[0] > 0:
                gain[v], target[v] = best
        winner = [min((v for v in net if v in gain), key=lambda v: (-gain[v], v), default=None) for net in nets]
        independent = [v for v in gain if all(winner[e] == v for e in on[v])]
        accepted = []
        for b in range(k):
            mine = sorted((v for v in independent if target[v] == b), key=lambda v: (-gain[v], v))
            accepted += mine[:max(lmax - size[b], 0)]
        if not accepted:
            break
        for v in accepted:
            part[v] = target[v]
        log.append((len(gain), len(independent), len(accepted), sum(gain[v] for v in accepted)))
    return np.array(part, np.int32), np.array(log, np.int64).reshape(-1, 4), lmax


def small_hypergraphs():
    """name -> (nodes, net_ptr, pins).  random: 300 nodes, 400 nets of 1..12 pins,
    one net with a repeated pin, one node on no net.  metrics: nets of 8 | 9,
    64 | 65 and 300 pins, node degrees around 50.  hubs: see below."""
    _, ptr, pins = kc.random_hypergraph(11, nodes=299)
    nodes = 300  # node 299 is on no net
    e = int(np.flatnonzero(np.diff(ptr) >= 3)[0])
    pins = pins.copy()
    pins[ptr[e] + 2] = pins[ptr[e]]  # a repeated pin: it counts once
    out = {"random": (nodes, ptr, pins)}
    nodes, ptr, pins = kc.metrics_hypergraph()
    out["metrics"] = (nodes, ptr, pins)
    # hubs: nodes 0, 1, 2 on exactly 64, 65 and 130 nets (one, two and three
    # strides of a wave over a node's nets); the metrics nodes stay below 64
    rng = np.random.default_rng(5)
    nets = [(3 + rng.choice(197, int(rng.integers(2, 7)), replace=False)).tolist() for _ in range(150)]
    for hub, count in ((0, 64), (1, 65), (2, 130)):
        for e in rng.choice(150, count, replace=False):
            nets[e].append(hub)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    pins = np.array([p for x in nets for p in x], np.int32)
    assert np.bincount(pins, minlength=200)[:3].tolist() == [64, 65, 130]
    out["hubs"] = (200, ptr, pins)
    return out


def starts(nodes, k):
    """name -> starting part vector."""
    block = (np.arange(nodes, dtype=np.int64) * k // nodes).astype(np.int32)
    out = {"block": block, "perm": np.random.default_rng(77 + k).permutation(block)}
    out["edge"] = list(kc.metrics_parts(nodes, k))[1]
    return out


def small_cases():
    """(id, hypergraph name, start name, k, eps): every k and start at eps 0.05,
    every eps on the block and permuted starts of k = 3 and 65."""
    out = []
    for g in ("random", "metrics", "hubs"):
        for k in KS if g != "hubs" else (2, 3, 64):
            for s in ("block", "perm", "edge"):
                out.append((f"{g}-{s}-k{k}-e0.05", g, s, k, 0.05))
        for k in (3, 65) if g != "metrics" else (3,):
            for eps in (0.0, 0.5):
                for s in ("block", "perm"):
                    out.append((f"{g}-{s}-k{k}-e{eps}", g, s, k, eps))
    return out


def circuit_cases():
    """(id, circuit, start name, k, eps, max_rounds)"""
    out = [("fract-block-k4-e0.05", "fract", "block", 4, 0.05, 0)]
    for k in (2, 3, 64):
        for eps in EPSILONS:
            out.append((f"fract-perm-k{k}-e{eps}", "fract", "perm", k, eps, 0))
    out.append(("fract-edge-k65-e0.05", "fract", "edge", 65, 0.05, 0))
    out.append(("ibm01-block-k8-e0.03-r8", "ibm01", "block", 8, 0.03, 8))
    out.append(("ibm01-perm-k256-e0.05-r3", "ibm01", "perm", 256, 0.05, 3))
    out.append(("ibm01-edge-k63-e0.5-r3", "ibm01", "edge", 63, 0.5, 3))
    return out


INTS = ("k", "rounds", "moves", "gain_total", "max_part", "part_min", "part_max", "connectivity_before", "cut_nets",
        "connectivity", "soed")


def check_properties(ek, g, start, k, eps, part, res, log):
    """What every run must satisfy, host or device."""
    _, nodes, ptr, pins = g
    before = ek.kway_metrics_host(ptr, pins, start, k)
    after = ek.kway_metrics_host(ptr, pins, part, k)
    assert res["connectivity_before"] == before[1]
    assert (res["cut_nets"], res["connectivity"], res["soed"]) == after
    assert len(log) == res["rounds"] and res["moves"] == int(log[:, 2].sum())
    assert before[1] - after[1] == res["gain_total"] == int(log[:, 3].sum())
    assert np.all(log[:, 3] > 0) and np.all(log[:, 2] > 0)
    assert np.all(log[:, 0] >= log[:, 1]) and np.all(log[:, 1] >= log[:, 2])
    assert res["max_part"] == max_part(nodes, k, eps)
    s0, s1 = np.bincount(start, minlength=k), np.bincount(part, minlength=k)
    assert np.all(s1 <= np.maximum(s0, res["max_part"]))
    assert (res["part_min"], res["part_max"]) == (int(s1.min()), int(s1.max()))
