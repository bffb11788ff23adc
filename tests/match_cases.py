"""The matching rule of the coarsening restated in plain Python,
and the inputs shared by test_match_host.py, test_gpu_match.py and
test_gpu_multilevel.py (the device path must agree with the host entry point
on the same cases).  EXPECTED holds the integers ek_match_host gave when the
cases were written; those of the hand-worked cases are derived in HAND below,
line by line, from the rule alone."""
import functools

import numpy as np

from conftest import circuit_path

INT32_MAX = 2 ** 31 - 1
ROUNDS = (1, 8, 0)  # max_rounds: one round, the default, until nothing matches
INTS = ("n", "n_coarse", "pairs", "rounds", "eligible_nets")
THREADS = 256  # MATCH_THREADS (ek_internal.hpp): a workgroup of the node kernels
SHORT = 32  # MATCH_SHORT (ek_internal.hpp): above this many entries a node is its wave's


def pack(nets):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    return ptr, np.array([p for x in nets for p in x], np.int32)


def synthetic_weights(nodes, nets):
    """Node weight 1 + (id mod 5), net weight 1 + (e mod 3): the weighting DESIGN.md §12 measured with."""
    return (1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32)


def match_ref(nodes, nets, node_w, net_w, max_cluster, max_net=64, max_rounds=8):
    """(mate, cluster, round log) by the rule: every round from the state at its start, p(u) the partner of the
    greatest (score, -v) entry, mutual proposals matched.  Python ints throughout."""
    w = [1] * nodes if node_w is None else [int(x) for x in node_w]
    max_net = max(max_net, 2)
    part = []  # (score, distinct pins) of the eligible nets
    for e, net in enumerate(nets):
        pins = list(dict.fromkeys(int(p) for p in net))
        if 2 <= len(pins) <= max_net:
            part.append(((1 if net_w is None else int(net_w[e])) * 2 ** 20 // (len(pins) - 1), pins))
    on = [[] for _ in range(nodes)]
    for i, (_, pins) in enumerate(part):
        for v in pins:
            on[v].append(i)
    mate = [-1] * nodes
    log = []
    while max_rounds <= 0 or len(log) < max_rounds:
        p = [-1] * nodes
        for u in range(nodes):
            if mate[u] >= 0:
                continue
            keys = [(part[i][0], -v) for i in on[u] for v in part[i][1]
                    if v != u and mate[v] < 0 and w[u] + w[v] <= max_cluster]
            if keys:
                p[u] = -max(keys)[1]
        pairs = [(u, p[u]) for u in range(nodes) if p[u] > u and p[p[u]] == u]
        if not pairs:
            break
        for u, v in pairs:
            mate[u], mate[v] = v, u
        log.append((sum(x >= 0 for x in p), len(pairs)))
    leaders = [v for v in range(nodes) if mate[v] < 0 or v < mate[v]]
    rank = {v: i for i, v in enumerate(leaders)}
    cluster = [rank[min(v, mate[v]) if mate[v] >= 0 else v] for v in range(nodes)]
    return (np.array(mate, np.int32), np.array(cluster, np.int32), np.array(log, np.int64).reshape(-1, 2))


def random_nets(rng, n, count, lo=2, hi=5):
    return [rng.choice(n, int(rng.integers(lo, hi + 1)), replace=False).tolist() for _ in range(count)]


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

    # --- hand-worked (HAND below) ---
    add("path_end_ids", 3, [[0, 1], [1, 2]])
    add("path_mid_id_2", 3, [[0, 2], [2, 1]])
    add("cycle_rising", 3, [[0, 1], [1, 2], [0, 2]], net_w=[1, 2, 3])
    add("path_rising", 6, [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]], net_w=[1, 2, 3, 4, 5])
    add("weights_at_cap", 2, [[0, 1]], node_w=[3, 4], max_cluster=7)
    add("weights_above_cap", 2, [[0, 1]], node_w=[3, 4], max_cluster=6)
    add("zero_weights", 4, [[0, 1], [1, 2], [2, 3]], node_w=[0, 5, 0, 6], net_w=[1, 2, 3], max_cluster=5)
    add("repeated_pin", 4, [[0, 0, 1], [1, 2, 2, 3], [3]])
    add("no_eligible_net", 5, [[0, 1, 2], [3, 4]], max_net=2)
    # --- kernel edges ---
    for k in (8, 9, 64, 65):  # one net of k pins (65: above max_net) beside a few small ones
        rng = np.random.default_rng(500 + k)
        add(f"net{k}", k + 6, [list(range(k))] + random_nets(rng, k + 6, 6, 2, 3))
    for n in (THREADS - 64, THREADS - 1, THREADS, THREADS + 1, THREADS + 64):
        rng = np.random.default_rng(600 + n)
        nets = random_nets(rng, n, n)
        add(f"n{n}", n, nets, rng.integers(0, 4, n), rng.integers(1, 10, len(nets)), max_cluster=4)
    rng = np.random.default_rng(700)
    add("all_pins_net", 90, [list(range(90))] + random_nets(rng, 90, 60, 2, 2))
    add("score_high_bits", 5, [[0, 1], [2, 3], [3, 4]], net_w=[INT32_MAX, 5, 5])
    for leaves in (SHORT, SHORT + 1, 100):  # the hub's entries: the thread | wave hand-over
        add(f"star{leaves}", leaves + 1, [[0, v] for v in range(1, leaves + 1)])
    rng = np.random.default_rng(701)
    add("star_weighted", 201, [[0, v] for v in range(1, 201)], net_w=rng.integers(1, 10, 200))
    rng = np.random.default_rng(702)  # every node far above SHORT entries, nets of 2..9 pins
    nets = random_nets(rng, 300, 3000, 2, 9)
    add("dense", 300, nets, rng.integers(1, 6, 300), rng.integers(1, 10, len(nets)), max_cluster=7)
    add("no_nets", 7, [[3], [], [5, 5]])
    return out


def names():
    return list(cases())


def circuit(ek, name, weighted):
    """A golden circuit, with §12's synthetic weights or with none."""
    h = ek.Hypergraph.read(circuit_path(name))
    if weighted:
        h.set_weights(*synthetic_weights(h.nodes, h.nets))
    return h


CIRCUITS = [("fract", False, 2), ("fract", True, 8), ("ibm01", False, 2), ("ibm01", True, 8)]  # (name, weighted, cap)


def hypergraph(ek, name):
    """The case as a Hypergraph with its weights attached, and (max_cluster, max_net)."""
    nodes, nets, node_w, net_w, cap, max_net = cases()[name]
    ptr, pins = pack(nets)
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    h.set_weights(node_w, net_w)
    return h, cap, max_net


@functools.lru_cache(maxsize=None)
def reference(name, max_rounds):
    """match_ref of a case, computed once and shared (treat it as read-only)."""
    nodes, nets, node_w, net_w, cap, max_net = cases()[name]
    return match_ref(nodes, nets, node_w, net_w, cap, max_net, max_rounds)


def ints(res):
    return tuple(int(res[f]) for f in INTS)


def mate_sum(mate):
    """A checksum of a mate vector: the sum of mate[v] (v + 1)."""
    return int(np.dot(mate.astype(np.int64), np.arange(1, len(mate) + 1)))


# The hand-worked cases: (mate, cluster, round log) at max_rounds 0.  Scores are c 2^20 / (|e| - 1); but for
# repeated_pin every net here has 2 distinct pins, so the score order is the order of c.
HAND = {
    # equal scores.  p(0) = 1; p(1): entries 0 and 2 tie, the smaller id 0; p(2) = 1.  0 and 1 are mutual.  Round 2:
    # node 2 has no unmatched neighbour, nobody proposes: not counted.
    "path_end_ids": ([1, 0, -1], [0, 0, 1], [(3, 1)]),
    # the path 0 - 2 - 1.  p(2): entries 0 and 1 tie, so 0; p(0) = 2; p(1) = 2.  0 and 2 are mutual.  Leaders 0, 1.
    "path_mid_id_2": ([2, -1, 0], [0, 1, 0], [(3, 1)]),
    # c(01) = 1 < c(12) = 2 < c(02) = 3.  p(0) = 2, p(2) = 0, p(1) = 2: only the pair of the greatest score forms.
    "cycle_rising": ([2, -1, 0], [0, 1, 0], [(3, 1)]),
    # c rises along the path, so everyone proposes to its higher neighbour and only the last pair is mutual: (4, 5),
    # then (2, 3), then (0, 1), one pair a round with 6, 4, 2 proposers.
    "path_rising": ([1, 0, 3, 2, 5, 4], [0, 0, 1, 1, 2, 2], [(6, 1), (4, 1), (2, 1)]),
    "weights_at_cap": ([1, 0], [0, 0], [(2, 1)]),       # 3 + 4 <= 7
    "weights_above_cap": ([-1, -1], [0, 1], []),        # 3 + 4 > 6
    # w = 0, 5, 0, 6 under cap 5.  Feasible pairs: (0, 1) at 5, (1, 2) at 5; (2, 3) weighs 6.  p(0) = 1, p(1) = 2
    # (c = 2 beats 1), p(2) = 1, p(3) = -1: (1, 2) matches.  Round 2: 0 and 3 share no net.
    "zero_weights": ([-1, 2, 1, -1], [0, 1, 1, 2], [(3, 1)]),
    # [0, 0, 1] is the 2-pin net {0, 1} (score 2^20), [1, 2, 2, 3] the 3-pin net {1, 2, 3} (score 2^19), [3] takes no
    # part.  p(0) = 1, p(1) = 0, p(2) = 1, p(3) = 1.  Round 2: p(2) = 3, p(3) = 2.
    "repeated_pin": ([1, 0, 3, 2], [0, 0, 1, 1], [(4, 1), (2, 1)]),
    # max_net 2: {0, 1, 2} is not eligible, its nodes have no entry.
    "no_eligible_net": ([-1, -1, -1, 4, 3], [0, 1, 2, 3, 3], [(2, 1)]),
}

# name -> {max_rounds: (n, n_coarse, pairs, rounds, eligible_nets, mate_sum)}, as ek_match_host gave them
EXPECTED = {
    "path_end_ids": {1: (3, 2, 1, 1, 2, -2), 8: (3, 2, 1, 1, 2, -2), 0: (3, 2, 1, 1, 2, -2)},
    "path_mid_id_2": {1: (3, 2, 1, 1, 2, 0), 8: (3, 2, 1, 1, 2, 0), 0: (3, 2, 1, 1, 2, 0)},
    "cycle_rising": {1: (3, 2, 1, 1, 3, 0), 8: (3, 2, 1, 1, 3, 0), 0: (3, 2, 1, 1, 3, 0)},
    "path_rising": {1: (6, 5, 1, 1, 5, 39), 8: (6, 3, 3, 3, 5, 67), 0: (6, 3, 3, 3, 5, 67)},
    "weights_at_cap": {1: (2, 1, 1, 1, 1, 1), 8: (2, 1, 1, 1, 1, 1), 0: (2, 1, 1, 1, 1, 1)},
    "weights_above_cap": {1: (2, 2, 0, 0, 1, -3), 8: (2, 2, 0, 0, 1, -3), 0: (2, 2, 0, 0, 1, -3)},
    "zero_weights": {1: (4, 3, 1, 1, 3, 2), 8: (4, 3, 1, 1, 3, 2), 0: (4, 3, 1, 1, 3, 2)},
    "repeated_pin": {1: (4, 3, 1, 1, 2, -6), 8: (4, 2, 2, 2, 2, 18), 0: (4, 2, 2, 2, 2, 18)},
    "no_eligible_net": {1: (5, 4, 1, 1, 1, 25), 8: (5, 4, 1, 1, 1, 25), 0: (5, 4, 1, 1, 1, 25)},
    "net8": {1: (14, 12, 2, 1, 7, 73), 8: (14, 9, 5, 3, 7, 271), 0: (14, 9, 5, 3, 7, 271)},
    "net9": {1: (15, 12, 3, 1, 7, 82), 8: (15, 9, 6, 3, 7, 374), 0: (15, 9, 6, 3, 7, 374)},
    "net64": {1: (70, 63, 7, 1, 7, 9491), 8: (70, 56, 14, 8, 7, 11497), 0: (70, 38, 32, 26, 7, 85655)},
    "net65": {1: (71, 65, 6, 1, 6, 7818), 8: (71, 65, 6, 1, 6, 7818), 0: (71, 65, 6, 1, 6, 7818)},
    "n192": {1: (192, 156, 36, 1, 192, 585024), 8: (192, 120, 72, 6, 192, 1304454), 0: (192, 120, 72, 6, 192, 1304454)},
    "n255": {1: (255, 208, 47, 1, 255, 1435816), 8: (255, 153, 102, 6, 255, 2984172), 0: (255, 153, 102, 6, 255, 2984172)},
    "n256": {1: (256, 205, 51, 1, 256, 1182090), 8: (256, 152, 104, 5, 256, 3639808), 0: (256, 152, 104, 5, 256, 3639808)},
    "n257": {1: (257, 212, 45, 1, 257, 1300391), 8: (257, 159, 98, 5, 257, 3069715), 0: (257, 159, 98, 5, 257, 3069715)},
    "n320": {1: (320, 265, 55, 1, 320, 1807284), 8: (320, 188, 132, 7, 320, 6359132), 0: (320, 188, 132, 7, 320, 6359132)},
    "all_pins_net": {1: (90, 72, 18, 1, 60, 48501), 8: (90, 64, 26, 3, 60, 107835), 0: (90, 64, 26, 3, 60, 107835)},
    "score_high_bits": {1: (5, 3, 2, 1, 3, 13), 8: (5, 3, 2, 1, 3, 13), 0: (5, 3, 2, 1, 3, 13)},
    "star32": {1: (33, 32, 1, 1, 32, -557), 8: (33, 32, 1, 1, 32, -557), 0: (33, 32, 1, 1, 32, -557)},
    "star33": {1: (34, 33, 1, 1, 33, -591), 8: (34, 33, 1, 1, 33, -591), 0: (34, 33, 1, 1, 33, -591)},
    "star100": {1: (101, 100, 1, 1, 100, -5147), 8: (101, 100, 1, 1, 100, -5147), 0: (101, 100, 1, 1, 100, -5147)},
    "star_weighted": {1: (201, 200, 1, 1, 200, -20295), 8: (201, 200, 1, 1, 200, -20295), 0: (201, 200, 1, 1, 200, -20295)},
    "dense": {1: (300, 230, 70, 1, 3000, 2648614), 8: (300, 161, 139, 8, 3000, 6091420), 0: (300, 160, 140, 9, 3000, 6194092)},
    "no_nets": {1: (7, 7, 0, 0, 0, -28), 8: (7, 7, 0, 0, 0, -28), 0: (7, 7, 0, 0, 0, -28)},
    "fract": {1: (149, 124, 25, 1, 147, 60659), 8: (149, 86, 63, 5, 147, 503263), 0: (149, 86, 63, 5, 147, 503263)},
    "fract-w": {1: (149, 116, 33, 1, 147, 223009), 8: (149, 89, 60, 5, 147, 521281), 0: (149, 89, 60, 5, 147, 521281)},
    "ibm01": {1: (12752, 9665, 3087, 1, 14111, 163647737574), 8: (12752, 6935, 5817, 8, 14111, 468841010632), 0: (12752, 6922, 5830, 12, 14111, 470865058406)},
    "ibm01-w": {1: (12752, 9647, 3105, 1, 14111, 201337142934), 8: (12752, 7194, 5558, 8, 14111, 431513955556), 0: (12752, 7189, 5563, 10, 14111, 432233649214)},
}
