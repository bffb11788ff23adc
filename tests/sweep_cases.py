"""The sweep-cut rule restated in plain Python, and the inputs
shared by test_sweep_host.py and test_gpu_sweep.py (the device path must agree
with the host entry point on the same cases)."""
import math
from fractions import Fraction

import numpy as np

import refine_cases as rc

EPSILONS = (0.0, 0.03, 0.5, 10.0)
INTS = ("n", "n0", "n1", "s_lo", "s_hi", "max_part", "cut", "cut_mid", "spanning_nets")
TILE = 2048  # keys per workgroup of a sort pass (SWEEP_TILE, ek_internal.hpp)
# 10 tiles: the (digit, tile) table has 2,560 words, and its scan takes 2,048
# words a workgroup (SWEEP_SCAN_BLOCK, ek_internal.hpp), so the scan spans two workgroups
N_TABLE_SCAN_SPANS_WORKGROUPS = 20000


def ord_keys(v):
    """The radix order as Python ints: the fp64 bit pattern with the sign
    flipped and negatives inverted (-0 before +0)."""
    out = []
    for u in np.ascontiguousarray(v, np.float64).view(np.uint64).tolist():
        out.append((~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63))
    return out


def window(n, eps):
    lmax = math.floor((1.0 + eps) * float(-(-n // 2)))
    return lmax, max(1, n - lmax), min(n - 1, lmax)


def sweep_ref(nodes, net_ptr, pins, v, eps, ratio=False):
    """(result ints, order, profile) by the rule: sorted on (key, id), sets, and
    profile[s] counted from its definition #{e : lo_e < s <= hi_e}."""
    n = nodes
    key = ord_keys(v)
    order = sorted(range(n), key=lambda i: (key[i], i))
    pos = {node: r for r, node in enumerate(order)}
    profile = [0] * (n + 1)
    spanning = 0
    for e in range(len(net_ptr) - 1):
        ranks = {pos[int(p)] for p in pins[net_ptr[e]:net_ptr[e + 1]]}
        if len(ranks) < 2:
            continue
        spanning += 1
        for s in range(min(ranks) + 1, max(ranks) + 1):
            profile[s] += 1
    lmax, s_lo, s_hi = window(n, eps)
    if ratio:
        best = min(range(s_lo, s_hi + 1), key=lambda s: (Fraction(profile[s], s * (n - s)), abs(2 * s - n), s))
    else:
        best = min(range(s_lo, s_hi + 1), key=lambda s: (profile[s], abs(2 * s - n), s))
    res = {"n": n, "n0": n - best, "n1": best, "s_lo": s_lo, "s_hi": s_hi, "max_part": lmax, "cut": profile[best],
           "cut_mid": profile[n // 2], "spanning_nets": spanning}
    return res, np.array(order, np.int32), np.array(profile, np.int32)


def ints(res):
    return {f: res[f] for f in INTS}


def small_hypergraphs():
    """refine_cases' graphs (a repeated pin, an isolated node, nets of 8 | 9,
    64 | 65 and 300 pins), each with a net of all n pins added, and one with
    no nets."""
    out = {}
    for name, (nodes, ptr, pins) in rc.small_hypergraphs().items():
        out[name] = (nodes, ptr, pins)
        everyone = np.random.default_rng(3).permutation(nodes).astype(np.int32)
        out[name + "+all"] = (nodes, np.concatenate([ptr, [ptr[-1] + nodes]]).astype(np.int64),
                              np.concatenate([pins, everyone]).astype(np.int32))
    out["no-nets"] = (77, np.zeros(1, np.int64), np.zeros(0, np.int32))
    return out


def shape_hypergraph(n, seed=0):
    """(nodes, net_ptr, pins) on n nodes: about n / 2 nets of 2..12 pins (fewer
    on tiny n), one net of all n pins, one of a single pin."""
    rng = np.random.default_rng(1000 + n + seed)
    nets = [rng.choice(n, int(min(n, rng.integers(2, 13))), replace=False).tolist() for _ in range(max(2, n // 2))]
    nets.append(rng.permutation(n).tolist())
    nets.append([int(rng.integers(0, n))])
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    return n, ptr, np.array([p for x in nets for p in x], np.int32)


def value_families(n, seed=0):
    """name -> n doubles."""
    rng = np.random.default_rng(20240923 + n + seed)
    out = {"normal": rng.standard_normal(n), "all-equal": np.full(n, 0.25),
           "three-values": rng.choice(np.array([-0.0, 0.0, 1.0]), n),
           "ascending": np.arange(n, dtype=np.float64), "descending": -np.arange(n, dtype=np.float64)}
    # the same sign, exponent and upper mantissa: only the lowest byte differs
    low = np.full(n, 1.5).view(np.uint64) | rng.integers(0, 256, n).astype(np.uint64)
    out["low-byte"] = low.view(np.float64)
    # powers of two of either sign: the mantissa bytes are all zero
    out["sign-exponent"] = np.ldexp(rng.choice(np.array([-1.0, 1.0]), n), rng.integers(-40, 41, n))
    special = np.array([np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4, 0.0, -0.0, 1.0, -1.0, np.nan,
                        -np.nan])
    out["inf-denormal-nan"] = special[rng.integers(0, len(special), n)]
    return out


def path_hypergraph(n):
    """Nets {i, i + 1}: with v = arange every split cuts exactly one net."""
    pins = np.repeat(np.arange(n, dtype=np.int32), 2)[1:-1]
    return n, np.arange(0, 2 * (n - 1) + 1, 2, dtype=np.int64), pins


def ten_node_case():
    """v = arange(10): profile[1] = 1, profile[5] = 2, every other split 3."""
    nets = [[0, 1], [4, 5], [4, 5]]
    for a in (1, 2, 3, 5, 6, 7, 8):
        nets += [[a, a + 1]] * 3
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in nets])]).astype(np.int64)
    return 10, ptr, np.array([p for x in nets for p in x], np.int32)
