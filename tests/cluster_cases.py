"""The multi-node clustering rule of the coarsening restated in plain Python, and the inputs shared by
test_cluster_host.py, test_gpu_cluster.py and test_gpu_kway_direct_cluster.py (the device path must agree with the
host entry point on the same cases).  The integers of the hand-worked cases are derived in HAND below, line by line,
from the rule alone."""
import functools

import numpy as np

import match_cases as mc

INT32_MAX = 2 ** 31 - 1
ROUNDS = (1, 8, 0)  # max_rounds: one round, the default, until a round joins nothing
INTS = ("n", "n_coarse", "joins", "rounds", "eligible_nets", "heaviest")
SHORT = 32  # CLUSTER_SHORT (ek_internal.hpp): above this many movers a destination's segment is its wave's


def cluster_ref(nodes, nets, node_w, net_w, max_cluster, max_net=64, stops=ROUNDS):
    """{max_rounds: (rep, cluster, round log, the result integers)} for every max_rounds of `stops`, from ONE run of
    the rule to its end: the state after round k is what max_rounds = k returns.  Every step of a round reads the
    state at the round's start.  Python ints throughout."""
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    max_net = max(max_net, 2)
    ent = [[] for _ in range(nodes)]  # per node: (score, v) over its eligible nets, itself excluded
    eligible = 0
    for e, net in enumerate(nets):
        pins = list(dict.fromkeys(int(p) for p in net))
        if 2 <= len(pins) <= max_net:
            eligible += 1
            score = (1 if net_w is None else int(net_w[e])) * 2 ** 20 // (len(pins) - 1)
            for u in pins:
                ent[u].extend((score, v) for v in pins if v != u)
    rep, S, grown = list(range(nodes)), list(w), [False] * nodes
    log, out = [], {}

    def snapshot():
        roots = [v for v in range(nodes) if rep[v] == v]
        rank = {v: i for i, v in enumerate(roots)}
        ints = (nodes, len(roots), sum(r[2] for r in log), len(log), eligible, max([S[v] for v in roots], default=0))
        return (np.array(rep, np.int32), np.array([rank[r] for r in rep], np.int32),
                np.array(log, np.int64).reshape(-1, 3), ints)

    while True:
        for k in stops:
            if k > 0 and k == len(log):
                out[k] = snapshot()
        if all(k in out for k in stops if k > 0) and 0 not in stops:
            break
        # 1. propose
        t, sigma = [-1] * nodes, [-1] * nodes
        for u in range(nodes):
            if rep[u] != u or grown[u]:
                continue
            best = None
            for s, v in ent[u]:
                r = rep[v]
                if S[r] + w[u] <= max_cluster and (best is None or (s, -r) > best):
                    best = (s, -r)
            if best is not None:
                sigma[u], t[u] = best[0], -best[1]
        # 2. incoming
        inc = [False] * nodes
        for u in range(nodes):
            if t[u] >= 0:
                inc[t[u]] = True

        # 3. resolve
        def ml(x):
            return t[x] >= 0 and t[t[x]] == x and x > t[x]
        movers = [u for u in range(nodes) if t[u] >= 0 and (not inc[u] or ml(u)) and not ml(t[u])]
        # 4. accept: the longest fitting prefix of every destination's order
        accepted = []
        for r in sorted(set(t[u] for u in movers)):
            total = 0
            for u in sorted((u for u in movers if t[u] == r), key=lambda u: (-sigma[u], u)):
                total += w[u]
                if total <= max_cluster - S[r]:
                    accepted.append(u)
        if not accepted:
            break
        # 5. apply
        for u in accepted:
            r = t[u]
            rep[u] = r
            S[r] += w[u]
            grown[u] = grown[r] = True
        log.append((sum(x >= 0 for x in t), len(movers), len(accepted)))
    end = snapshot()
    for k in stops:
        out.setdefault(k, end)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (nodes, nets as lists, node_w or None, net_w or None, max_cluster, max_net)."""
    out = {}

    def add(name, nodes, nets, node_w=None, net_w=None, max_cluster=2, max_net=64):
        assert name not in out
        assert node_w is None or len(node_w) == nodes
        assert net_w is None or len(net_w) == len(nets)
        out[name] = (nodes, [list(map(int, x)) for x in nets],
                     None if node_w is None else np.ascontiguousarray(node_w, np.int32),
                     None if net_w is None else np.ascontiguousarray(net_w, np.int32), max_cluster, max_net)

    def star(hub, leaves):
        return [[hub, v] for v in leaves]

    # --- hand-worked (HAND below): every branch of the resolve step ---
    add("star_hub_least", 5, star(0, range(1, 5)), max_cluster=5)
    add("star_hub_greatest", 5, star(4, range(4)), max_cluster=5)
    add("chain_waits", 3, [[0, 1], [1, 2]], net_w=[3, 1], max_cluster=3)
    add("path_rising", 6, [[i, i + 1] for i in range(5)], net_w=[1, 2, 3, 4, 5], max_cluster=3)
    add("ring_even", 4, [[0, 1], [1, 2], [2, 3], [3, 0]], max_cluster=4)
    # --- the cap (HAND below) ---
    add("cap_mid_order", 6, star(0, range(1, 6)), node_w=[1, 2, 2, 2, 2, 2], net_w=[1, 5, 3, 4, 2], max_cluster=6)
    add("cap_zero_weights", 6, star(0, range(1, 6)), node_w=[1, 2, 0, 2, 0, 1], net_w=[5, 4, 3, 2, 1], max_cluster=4)
    add("heavier_than_cap", 3, [[0, 1], [1, 2]], node_w=[1, 10, 1], max_cluster=4)
    add("weights_at_cap", 2, [[0, 1]], node_w=[3, 4], max_cluster=7)
    add("weights_above_cap", 2, [[0, 1]], node_w=[3, 4], max_cluster=6)
    # --- kernel edges ---
    for m in (1, 63, 64, 65, 300):  # m movers to one destination: the hub proposes to leaf 1, every leaf to the hub
        add(f"movers{m}", m + 1, star(0, range(1, m + 1)), max_cluster=m + 1)
        rng = np.random.default_rng(800 + m)
        wl = rng.integers(0, 4, m)
        add(f"movers{m}_cap", m + 1, star(0, range(1, m + 1)), node_w=[1] + wl.tolist(), net_w=rng.integers(1, 6, m),
            max_cluster=1 + int(wl.sum()) // 2)
    for n in (63, 64, 65, 255, 256, 257):
        rng = np.random.default_rng(900 + n)
        nets = mc.random_nets(rng, n, n)
        add(f"n{n}", n, nets, rng.integers(0, 4, n), rng.integers(1, 10, len(nets)), max_cluster=9)
    for i in range(30):  # seeded random hypergraphs
        rng = np.random.default_rng(1000 + i)
        n = int(rng.integers(20, 121))
        nets = mc.random_nets(rng, n, int(rng.integers(n // 2, 3 * n)), 2, int(rng.integers(2, 8)))
        add(f"random{i}", n, nets, rng.integers(0, 5, n) if i % 3 else None,
            rng.integers(1, 4, len(nets)) if i % 2 else None, max_cluster=int(rng.integers(2, 24)),
            max_net=64 if i % 5 else 4)
    # --- match_cases.py's cases as inputs: at their own cap, and at a cap that lets clusters grow.  Among them nets
    # of 64 | 65 pins (net64, net65), a hub of 32 | 33 entries (star32, star33), every node far above 32 entries
    # (dense), c = 2^31 - 1 (score_high_bits), no nets (no_nets) and no eligible net (no_eligible_net) ---
    for name, (nodes, nets, node_w, net_w, cap, max_net) in mc.cases().items():
        add("m:" + name, nodes, nets, node_w, net_w, cap, max_net)
        add("m4:" + name, nodes, nets, node_w, net_w, 4 * cap + 3, max_net)
    return out


def names():
    return list(cases())


CIRCUITS = [("fract", False, 6), ("fract", True, 16), ("ibm01", False, 95), ("ibm01", True, 285)]  # (name, weighted, cap)


def hypergraph(ek, name):
    """The case as a Hypergraph with its weights attached, and (max_cluster, max_net)."""
    nodes, nets, node_w, net_w, cap, max_net = cases()[name]
    ptr, pins = mc.pack(nets)
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    h.set_weights(node_w, net_w)
    return h, cap, max_net


@functools.lru_cache(maxsize=None)
def reference(name):
    """cluster_ref of a case at the three max_rounds, computed once and shared (treat it as read-only)."""
    nodes, nets, node_w, net_w, cap, max_net = cases()[name]
    return cluster_ref(nodes, nets, node_w, net_w, cap, max_net)


@functools.lru_cache(maxsize=None)
def circuit_reference(ek, name, weighted, cap):
    h = mc.circuit(ek, name, weighted)
    ptr, pins = h.pins()
    nets = [pins[ptr[e]:ptr[e + 1]].tolist() for e in range(len(ptr) - 1)]
    node_w, net_w = h.weights()
    return cluster_ref(h.nodes, nets, node_w, net_w, cap)


def ints(res):
    return tuple(int(res[f]) for f in INTS)


# The hand-worked cases: (rep, cluster, round log of (proposers, movers, joins), heaviest) at max_rounds 0.  t is the
# proposal, in the incoming flag, ml(x) "x is the larger id of a mutual pair".  Unless weights are given every node
# weighs 1 and every net here has 2 pins, so the score order is the order of c.
HAND = {
    # Equal scores.  t(0) = 1 (the smallest of its targets), t(1..4) = 0.  in = {0, 1}.  ml(1).  0 has incomers and is
    # not ml: it stays.  1 moves as the larger of the mutual pair, 2, 3, 4 move (in = 0, their target 0 stays).  All
    # four fit under 5 - 1.  One round, one cluster.
    "star_hub_least": ([0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [(5, 4, 4)], 5),
    # t(0..3) = 4, t(4) = 0.  in = {0, 4}.  ml(4): the hub moves to 0.  0 has an incomer and is not ml: stays.  1, 2, 3
    # target 4, which is leaving: they wait.  Round 2: 1, 2, 3 see pin 4 with rep 0, S(0) = 2, 2 + 1 <= 5; t = 0, in =
    # 0, 0 is no single so it proposes nothing: all three move and fit.
    "star_hub_greatest": ([0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [(5, 1, 1), (3, 3, 3)], 5),
    # c(01) = 3 > c(12) = 1.  t(0) = 1, t(1) = 0, t(2) = 1.  ml(1): 1 moves to 0.  2 targets 1, which is leaving: waits.
    # Round 2: t(2) = rep[1] = 0, S(0) + 1 = 3 <= 3.
    "chain_waits": ([0, 0, 0], [0, 0, 0], [(3, 1, 1), (1, 1, 1)], 3),
    # c rises along the path: t = 1, 2, 3, 4, 5, 4.  in = {1, .., 5}.  ml(5).  0 moves (in = 0; its target 1 is not ml);
    # 1, 2, 3, 4 have incomers; 5 moves to 4.  Round 2: the singles are 2 and 3.  2 sees 1 (S = 2, fits, score 2) and 3
    # (score 3): t(2) = 3.  3 sees 2 (score 3) and rep[4] = 4 (S = 2, fits, score 4): t(3) = 4.  2 moves (in = 0, 3 is
    # not ml: t(4) = -1); 3 has an incomer and stays.  Round 3: no single is left.  Roots 1, 3, 4.
    "path_rising": ([1, 1, 3, 3, 4, 4], [0, 0, 1, 1, 2, 2], [(6, 2, 2), (2, 1, 1)], 2),
    # The ring 0 - 1 - 2 - 3 - 0.  t(0) = 1, t(1) = 0, t(2) = 1, t(3) = 0.  in = {0, 1}.  ml(1): 1 moves to 0; 2 targets
    # 1 and waits; 3 moves to 0 (in = 0); 0 stays.  Round 2: 2 sees rep[1] = rep[3] = 0, S(0) + 1 = 4 <= 4.
    "ring_even": ([0, 0, 0, 0], [0, 0, 0, 0], [(4, 2, 2), (1, 1, 1)], 4),
    # Hub 0 (w 1), leaves of weight 2, c = 1, 5, 3, 4, 2 for leaves 1..5, cap 6.  t(0) = 2 (score 5), ml(2); every
    # leaf moves.  The order by score: 2, 4, 3, 5, 1; the sums 2, 4, 6 against 6 - 1 = 5: 2 and 4 are accepted.  Round
    # 2: S(0) = 5, 5 + 2 > 6, nobody proposes.
    "cap_mid_order": ([0, 1, 0, 3, 0, 5], [0, 1, 0, 2, 0, 3], [(6, 5, 2)], 5),
    # Hub 0 (w 1), leaves 1..5 of weight 2, 0, 2, 0, 1 and c = 5, 4, 3, 2, 1, cap 4: room 3.  All leaves move, in the
    # order 1, 2, 3, 4, 5 with the sums 2, 2, 4, 4, 5: 1 fits, the weightless 2 right behind it fits, 3 is the first
    # rejected, the weightless 4 behind it is rejected, 5 is rejected.  Round 2: S(0) = 3.  3 does not fit (5 > 4); 4
    # and 5 propose 0 and move, the sums 0, 1 against 4 - 3: both accepted.  Round 3: 3 cannot propose.
    "cap_zero_weights": ([0, 0, 0, 3, 0, 0], [0, 0, 0, 1, 0, 0], [(6, 5, 2), (2, 2, 2)], 4),
    # 1 weighs 10 > cap 4: it proposes nothing and nobody fits with it.  It stays a cluster of one, above the cap.
    "heavier_than_cap": ([0, 1, 2], [0, 1, 2], [], 10),
    "weights_at_cap": ([0, 0], [0, 0], [(2, 1, 1)], 7),      # 3 + 4 <= 7: mutual, 1 moves to 0
    "weights_above_cap": ([0, 1], [0, 1], [], 4),            # 3 + 4 > 6
}
