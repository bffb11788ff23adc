"""The weighted sweep-cut rule restated in plain Python, and
the inputs shared by test_sweepw_host.py and test_gpu_sweepw.py (the device
path must agree with the host entry point on the same cases).  The structures
and the value families come from sweep_cases, which is imported and left as it
is."""
import functools
import math

import numpy as np

import sweep_cases as sc

EPSILONS = (0.0, 0.03, 0.25)
INTS = ("n", "n0", "n1", "s_lo", "s_hi", "feasible", "total_weight", "max_part", "w0", "w1", "cut", "cut_nets",
        "cut_half", "spanning_nets")
INT32_MAX = 2 ** 31 - 1
SCAN_BLOCK = 2048  # words per workgroup of a scan, of either width (SWEEP_SCAN_BLOCK, ek_internal.hpp)
SCAN_TOP = 256  # block sums per step of the top scan's one workgroup (SC_THREADS, kernels_sweep.hip)
# k_scan_top, for both word widths, walks the block sums SCAN_TOP at a step and
# carries the running total between steps.  The scans run over n + 1 words, so up to n + 1 =
# SCAN_TOP * SCAN_BLOCK = 524,288 words there is one step and the carry is
# never used; n = 524,288 (524,289 words, 257 block sums) is the smallest n
# whose scan takes the second step.
N_TOP_SCAN_SECOND_STEP = SCAN_TOP * SCAN_BLOCK


def max_part(total, eps):
    return math.floor((1.0 + eps) * float((total + 1) // 2))


def rand_weights(rng, nodes, nets):
    """Node weights in 0..7 (zeros included), net weights in 1..9."""
    return rng.integers(0, 8, nodes).astype(np.int32), rng.integers(1, 10, nets).astype(np.int32)


def synthetic_weights(nodes, nets):
    """Node weight 1 + (id mod 5), net weight 1 + (e mod 3): the weighting DESIGN.md §12 measured with."""
    return (1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32)


def sweepw_ref(nodes, net_ptr, pins, node_w, net_w, v, eps):
    """(result ints, order, profile_w, P, count profile) by the rule: sorted on (key, id), profile_w[s] and the count
    profile summed over the nets with lo < s <= hi, P[s] summed over the ranks below s, the window and the choice by
    brute force over s = 1 .. n - 1.  Python ints and int64 sums (every sum here is below 2^62)."""
    n = nodes
    key = sc.ord_keys(v)
    order = sorted(range(n), key=lambda i: (key[i], i))
    pos = {node: r for r, node in enumerate(order)}
    w = [1] * n if node_w is None else [int(x) for x in node_w]
    profw = np.zeros(n + 1, np.int64)
    prof = np.zeros(n + 1, np.int64)
    spanning = 0
    for e in range(len(net_ptr) - 1):
        ranks = {pos[int(p)] for p in pins[net_ptr[e]:net_ptr[e + 1]]}
        if len(ranks) < 2:
            continue
        spanning += 1
        profw[min(ranks) + 1:max(ranks) + 1] += 1 if net_w is None else int(net_w[e])
        prof[min(ranks) + 1:max(ranks) + 1] += 1
    by_rank = np.array([w[i] for i in order], np.int64)
    P = [int(by_rank[:s].sum()) for s in range(n + 1)]
    W = sum(w)
    assert P[n] == W
    lmax = max_part(W, eps)
    window = [s for s in range(1, n) if P[s] <= lmax and W - P[s] <= lmax]
    if window:
        best = min(window, key=lambda s: (int(profw[s]), abs(2 * P[s] - W), s))
    else:
        best = min(range(1, n), key=lambda s: (abs(2 * P[s] - W), int(profw[s]), s))
    res = {"n": n, "n0": n - best, "n1": best, "s_lo": window[0] if window else 0, "s_hi": window[-1] if window else 0,
           "feasible": 1 if window else 0, "total_weight": W, "max_part": lmax, "w0": W - P[best], "w1": P[best],
           "cut": int(profw[best]), "cut_nets": int(prof[best]), "cut_half": int(profw[n // 2]),
           "spanning_nets": spanning}
    return res, np.array(order, np.int32), profw, np.array(P, np.int64), prof


def ints(res):
    return {f: res[f] for f in INTS}


def pack(nets):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    return ptr, np.array([p for x in nets for p in x], np.int32)


def zero_run_case(n=64, k=6, seed=9):
    """v = arange(n) (the order is the identity).  The 2k nodes of rank n/2 - k .. n/2 + k - 1 weigh 0 and the two
    flanks weigh the same, so P is flat at W / 2 over s = n/2 - k .. n/2 + k: at eps = 0 the window is exactly that
    run of 2k + 1 splits, every one of them perfectly balanced, and (profile_w, s) alone decides."""
    rng = np.random.default_rng(seed)
    left = rng.integers(1, 8, n // 2 - k)
    node_w = np.concatenate([left, np.zeros(2 * k, np.int64), left[::-1]]).astype(np.int32)
    nets = [rng.choice(n, int(rng.integers(2, 6)), replace=False).tolist() for _ in range(3 * n)]
    ptr, pins = pack(nets)
    return n, ptr, pins, node_w, rng.integers(1, 10, len(nets)).astype(np.int32), np.arange(n, dtype=np.float64)


def contended_case(n=300, nets=5000):
    """`nets` nets {3, n - 4} of weight 2^31 - 1 (v = arange): every add of the weighted difference array lands on
    one of two words, and their sum, 5,000 (2^31 - 1), carries far into the high word.  A few other nets beside."""
    rng = np.random.default_rng(12)
    rows = [[3, n - 4]] * nets + [rng.choice(n, 3, replace=False).tolist() for _ in range(40)]
    ptr, pins = pack(rows)
    net_w = np.concatenate([np.full(nets, INT32_MAX), rng.integers(1, 10, 40)]).astype(np.int32)
    return n, ptr, pins, rng.integers(0, 8, n).astype(np.int32), net_w, np.arange(n, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (nodes, net_ptr, pins, node_w or None, net_w or None, v, epsilons)."""
    out = {}

    def add(name, nodes, ptr, pins, node_w, net_w, v, eps=EPSILONS):
        node_w = None if node_w is None else np.ascontiguousarray(node_w, np.int32)
        net_w = None if net_w is None else np.ascontiguousarray(net_w, np.int32)
        v = np.ascontiguousarray(v, np.float64)
        assert name not in out and len(v) == nodes
        assert node_w is None or len(node_w) == nodes
        assert net_w is None or len(net_w) == len(ptr) - 1
        out[name] = (nodes, ptr, pins, node_w, net_w, v, tuple(eps))

    # node counts: the least, and n + 1 around one and two blocks of the 64-bit scan
    for n in (2, 3, SCAN_BLOCK - 2, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1):
        nodes, ptr, pins = sc.shape_hypergraph(n)
        rng = np.random.default_rng(300 + n)
        node_w, net_w = rand_weights(rng, n, len(ptr) - 1)
        add(f"n{n}", nodes, ptr, pins, node_w, net_w, rng.standard_normal(n), eps=(0.03,) if n > 3 else EPSILONS)
    # the structures of sweep_cases (a repeated pin, single-pin nets, an isolated node, nets of 8 | 9, 64 | 65, 300
    # and all n pins, no nets at all) under random weights, every eps
    for i, (name, (nodes, ptr, pins)) in enumerate(sorted(sc.small_hypergraphs().items())):
        rng = np.random.default_rng(400 + i)
        node_w, net_w = rand_weights(rng, nodes, len(ptr) - 1)
        add(name, nodes, ptr, pins, node_w, net_w, sc.value_families(nodes, 3)["normal"])
    # the value families that exercise every byte of the key, on one weighted structure
    nodes, ptr, pins = sc.small_hypergraphs()["random+all"]
    node_w, net_w = rand_weights(np.random.default_rng(420), nodes, len(ptr) - 1)
    for fam, v in sc.value_families(nodes, 4).items():
        add(f"family-{fam}", nodes, ptr, pins, node_w, net_w, v, eps=(0.03,))
    # node weights only, net weights only
    add("node_w_only", nodes, ptr, pins, node_w, None, sc.value_families(nodes, 5)["normal"])
    add("net_w_only", nodes, ptr, pins, None, net_w, sc.value_families(nodes, 5)["normal"])
    # a run of zero-weight nodes that is the whole window at eps = 0
    add("zero_run", *zero_run_case())
    # repeated pins, single-pin and empty nets, all of them carrying weights that must not shift onto other nets
    ptr, pins = pack([[0, 0, 1], [2], [], [3, 3], [1, 4, 4, 2], [], [5, 0], [6]])
    add("degenerate", 7, ptr, pins, [2, 0, 3, 1, 0, 4, 2], [9, 8, 7, 6, 5, 4, 3, 2], [0.5, -1.0, 2.0, 0.0, -0.0, 1.5, 0.5])
    # sums that cross 2^32: three nets of weight 2^31 - 1 over the same splits (profile_w = 3 (2^31 - 1)), three
    # nodes of weight 2^31 - 1 (P passes 2^32 at the second)
    ptr, pins = pack([[0, 5], [5, 0], [0, 2, 5], [1, 2], [3, 4]])
    add("cross_2_32", 6, ptr, pins, [INT32_MAX, 1, INT32_MAX, 5, INT32_MAX, 7],
        [INT32_MAX, INT32_MAX, INT32_MAX, 3, 2], np.arange(6))
    # one node heavier than L_max at every eps here: no feasible split, the fallback choice
    ptr, pins = pack([[0, 1], [1, 2], [2, 3], [3, 4], [0, 4]])
    add("heavy_node", 5, ptr, pins, [1, 2, 100, 1, 2], [4, 1, 2, 7, 3], [0.1, 0.2, 0.3, 0.4, 0.5])
    # W = 8, L_max = 4 at eps 0 and 0.03: only s = 2 (P = 4) is feasible; at 0.25 (L_max = 5) s = 1 is too
    ptr, pins = pack([[0, 1], [1, 2], [2, 3], [0, 3]])
    add("window_of_one", 4, ptr, pins, [3, 1, 2, 2], [2, 5, 1, 1], np.arange(4))
    # many nets on one lo and one hi
    add("contended", *contended_case(), eps=(0.03,))
    return out


def names():
    return list(cases())


def hypergraph(ek, name):
    """The case as a Hypergraph with its weights attached, and (v, epsilons)."""
    nodes, ptr, pins, node_w, net_w, v, eps = cases()[name]
    h = ek.Hypergraph.from_pins(nodes, ptr, pins)
    h.set_weights(node_w, net_w)
    return h, v, eps


@functools.lru_cache(maxsize=None)
def reference(name, eps):
    """sweepw_ref of a case, computed once and shared (treat it as read-only)."""
    nodes, ptr, pins, node_w, net_w, v, _ = cases()[name]
    return sweepw_ref(nodes, ptr, pins, node_w, net_w, v, eps)


def big_case(n=N_TOP_SCAN_SECOND_STEP, seed=21):
    """(nodes, net_ptr, pins, node_w, net_w, v) on n nodes, built with array operations only: n / 8 nets of 4 random
    pins and one net of all n pins."""
    rng = np.random.default_rng(seed)
    m = n // 8
    pins = np.concatenate([rng.integers(0, n, 4 * m), rng.permutation(n)]).astype(np.int32)
    ptr = np.concatenate([np.arange(0, 4 * m + 1, 4), [4 * m + n]]).astype(np.int64)
    node_w, net_w = rand_weights(rng, n, m + 1)
    return n, ptr, pins, node_w, net_w, rng.standard_normal(n)
