"""Inputs and a plain-numpy reference for the device median and rank splits,
shared by test_split_cases_host.py (the cases are what they claim, and the
reference agrees with the host entry points) and test_gpu_split.py (the
kernels agree with the reference, element for element).

Integers and exact doubles only: nothing here carries a tolerance.

The constants restate csrc/kernels_kl.hip and csrc/kernels_kway.hip (the
library exports none of them; test_split_cases_host.py holds them to the
sources as text):
  SEL_TILE    keys a block of the radix select's pass histograms
  SEL_SUB     first-level arrival counters of a select pass
  PART_BLOCK  nodes a block of the count / place kernels takes (both splits)
  PLACE_STRIDE  threads of a place block: the stride of its "blocks before me"
              loop, whose second trip starts at block 256"""
import functools

import numpy as np

from kway_cases import ord_key, rank_split_big_case, rank_split_cases, rank_split_ref

SEL_TILE = 2048
SEL_SUB = 16
PART_BLOCK = 1024
PLACE_STRIDE = 256
U64 = np.uint64
TOP = U64(1 << 63)


def key_value(k):
    """The inverse of ord_key: the doubles whose radix keys are k."""
    k = np.ascontiguousarray(k, U64)
    u = np.where(k >> U64(63) != 0, k & ~TOP, ~k)
    return np.ascontiguousarray(u, U64).view(np.float64)


def select_blocks(n):
    return (n + SEL_TILE - 1) // SEL_TILE


def place_blocks(n):
    return (n + PART_BLOCK - 1) // PART_BLOCK


def group_sizes(nb):
    """Blocks that arrive at each first-level counter of a select pass (block b
    at counter b % SEL_SUB), for the counters that have any."""
    return [(nb - g + SEL_SUB - 1) // SEL_SUB for g in range(min(nb, SEL_SUB))]


# ---------------------------------------------------------------------------
# reference
def median_ref(v):
    """(median, side): the two middle entries of a full sort, side = median > v."""
    v = np.ascontiguousarray(v, np.float64)
    n = len(v)
    s = np.sort(v)
    with np.errstate(invalid="ignore"):  # (-inf + inf: the NaN median of inf-halves)
        med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    return float(med), (med > v).astype(np.uint8)


def lists_ref(side):
    """order0, order1, plist, n0, n1 of a side vector: the lists in node order,
    plist[i] = i's position in its list, bit 31 set on side 1."""
    side = np.asarray(side, np.uint8)
    order0 = np.flatnonzero(side == 0).astype(np.int32)
    order1 = np.flatnonzero(side == 1).astype(np.int32)
    plist = np.empty(len(side), np.uint32)
    plist[order0] = np.arange(len(order0), dtype=np.uint32)
    plist[order1] = np.arange(len(order1), dtype=np.uint32) | np.uint32(1 << 31)
    return {"order0": order0, "order1": order1, "plist": plist, "side": side, "n0": len(order0), "n1": len(order1)}


def rank_ref(v, n1):
    """side 1 = the n1 smallest in (ord_key(v[i]), i)."""
    return rank_split_ref(v, n1)


def same_value(a, b):
    """a == b, and two NaNs count as the same value (the median of inf-halves)."""
    return a == b or (a != a and b != b)


# ---------------------------------------------------------------------------
# median cases
def _bytes_key(b):
    k = 0
    for x in b:
        k = (k << 8) | int(x)
    return k


def parting_keys(n, p, seed):
    """n distinct keys (even n) whose two middle ones share their top p bytes
    and first differ in byte p (byte 0 the most significant), in shuffled
    order.  Returns (keys, k_lo, k_hi).

    The middle keys' bytes after the shared prefix lie in 0x50..0x7f (lower)
    and 0x80..0xb0 (upper); p = 7 is 0x7f | 0x80, two neighbouring doubles.
    Around them a ladder of decoys: at every byte q, 64 keys that share the
    lower middle key's q-byte prefix and have a smaller byte q, and 64 that
    share the upper one's and have a larger byte q.  So every pass of either
    rank histograms keys into more than one bin, and at least 64 decoys a side
    share the p-byte prefix (those of the levels q >= p).  The rest of each
    half is filled at level 0.  Top bytes stay inside 0x01..0xfe: no NaN."""
    assert n % 2 == 0 and 0 <= p <= 7
    rng = np.random.default_rng(seed)
    pre = [int(x) for x in rng.integers(0x50, 0xb1, p)]
    lo = pre + [int(x) for x in rng.integers(0x50, 0x80, 8 - p)]
    hi = pre + [int(x) for x in rng.integers(0x80, 0xb1, 8 - p)]
    if p == 7:
        lo[7], hi[7] = 0x7f, 0x80
    half = n // 2 - 1
    assert half >= 8 * 64
    out = []
    for mid, below in ((lo, True), (hi, False)):
        keys = set()
        for q in range(8):
            want = len(keys) + (64 if q else half - 7 * 64)
            a, b = (1, mid[q]) if below else (mid[q] + 1, 0xff)
            while len(keys) < want:
                tail = [int(x) for x in rng.integers(0, 256, 7 - q)]
                keys.add(_bytes_key(mid[:q] + [int(rng.integers(a, b))] + tail))
        out.extend(sorted(keys))
    k_lo, k_hi = _bytes_key(lo), _bytes_key(hi)
    keys = np.array(out + [k_lo, k_hi], U64)
    rng.shuffle(keys)
    return keys, k_lo, k_hi


def tie_vector(n, r0, r1, seed, nodes=None):
    """n values whose sorted ranks r0..r1 (inclusive) are one equal run (0.25),
    distinct values below and above it.  nodes: the run sits at these node ids
    (a contiguous range of r1 - r0 + 1 ids); otherwise anywhere."""
    rng = np.random.default_rng(seed)
    run = r1 - r0 + 1
    below = 0.25 - np.arange(1, r0 + 1) / 4096.0
    above = 0.25 + np.arange(1, n - 1 - r1 + 1) / 4096.0
    rest = np.concatenate([below, above])
    rng.shuffle(rest)
    if nodes is None:
        v = np.concatenate([rest, np.full(run, 0.25)])
        rng.shuffle(v)
        return v
    a, b = nodes
    assert b - a == run
    return np.concatenate([rest[:a], np.full(run, 0.25), rest[a:]])


@functools.lru_cache(maxsize=None)
def median_cases():
    """name -> v.  (A dict built once: the tests share it and leave it unchanged.)"""
    rng = np.random.default_rng(20250301)
    out = {}
    # tiny
    for n in (1, 2, 3, 4):
        out[f"tiny-distinct-{n}"] = np.array([0.5, -1.25, 3.0, -0.125][:n])
        out[f"tiny-equal-{n}"] = np.full(n, -0.75)
    # place blocks (PART_BLOCK) and select tiles (SEL_TILE)
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4097):
        out[f"edge-{n}"] = rng.standard_normal(n)
    # the select's arrival counters: nb = 15, 16, 17, 32, 33, an even and an odd n each
    for n in (30719, 30720, 32767, 32768, 32769, 32770, 65535, 65536, 65537, 65538):
        out[f"ctr-nb{select_blocks(n)}-{n}"] = rng.standard_normal(n)
    # second trip of the blocks-before loops.  Ascending values put side 0 (the
    # large values) in the last blocks, so block 256 is all side 0 and a dropped
    # bcount[256] moves block 257's node by 1024; descending puts it all in the
    # first blocks; random gives every block about half.
    for n in (262144, 262145, 263169):
        r = rng.standard_normal(n)
        out[f"trip2-ascending-{n}"] = np.sort(r)
        out[f"trip2-descending-{n}"] = np.sort(r)[::-1].copy()
        out[f"trip2-random-{n}"] = r
    # the pass at which the two ranks part
    for n in (2050, 4098):
        for p in range(8):
            out[f"part-p{p}-{n}"] = key_value(parting_keys(n, p, 1000 * n + p)[0])
    # ties at the median
    for n in (2049, 2050, 4098):
        h = n // 2
        for name, (r0, r1) in tie_runs(n).items():
            out[f"tie-{name}-{n}"] = tie_vector(n, r0, r1, n + r0)
        # a run at the node ids crossing 1024 and 2048, holding the middle ranks
        a, b = 1000, min(2060, n)
        run = b - a
        r0 = h - run // 2
        out[f"tie-nodes-{n}"] = tie_vector(n, r0, r0 + run - 1, n, nodes=(a, b))
        out[f"tie-all-equal-{n}"] = np.full(n, 0.25)
    # value edges
    for n in (2049, 2050):
        out[f"val-signed-zeros-{n}"] = rng.choice(np.array([0.0, -0.0]), n)
        v = rng.standard_normal(n)
        v[[0, 5, n - 1]] = -np.inf
        v[[1, 1024, n - 2]] = np.inf
        out[f"val-inf-ends-{n}"] = v
        for s, inf in (("pos", np.inf), ("neg", -np.inf)):
            v = rng.standard_normal(n)
            v[rng.permutation(n)[: n // 2 + 40]] = inf
            v[[3, n - 4]] = -inf
            out[f"val-inf-most-{s}-{n}"] = v
        m = rng.integers(-(1 << 52) + 1, 1 << 52, n)
        out[f"val-denormals-{n}"] = m.astype(np.float64) * 2.0 ** -1074
        out[f"val-negative-{n}"] = -np.abs(rng.standard_normal(n)) - 0.125
        out[f"val-magnitudes-{n}"] = rng.choice(np.array([-1.0, 1.0]), n) * 10.0 ** rng.uniform(-300, 300, n)
    # the two middle entries are -inf and +inf: the median is NaN, `median > v`
    # is false everywhere and side 1 is empty
    v = np.full(2050, np.inf)
    v[rng.permutation(2050)[:1025]] = -np.inf
    out["val-inf-halves-2050"] = v
    for v in out.values():
        v.setflags(write=False)
    return out


def tie_runs(n):
    """name -> (r0, r1), the sorted ranks an equal run covers, around the median
    ranks lo = n/2 - 1 (even n) and hi = n/2."""
    h = n // 2
    runs = {
        "hi-only-starts": (h, h + 300),         # starts exactly at rank n/2
        "both-wide": (h - 400, h + 300),        # holds every median rank, well inside
        "ends-at-hi": (h - 400, h),             # ends exactly at rank n/2
    }
    if n % 2 == 0:
        runs["lo-only-ends"] = (h - 400, h - 1)   # ends exactly at rank n/2 - 1
        runs["starts-at-lo"] = (h - 1, h + 300)   # starts exactly at rank n/2 - 1
        runs["just-both"] = (h - 1, h)            # the two middle ranks and nothing else
    return runs


def median_ns():
    return sorted({len(v) for v in median_cases().values()})


def median_cases_of(n):
    return {k: v for k, v in median_cases().items() if len(v) == n}


@functools.lru_cache(maxsize=None)
def median_expected(name):
    """(median, lists_ref dict) of a median case, computed once."""
    med, side = median_ref(median_cases()[name])
    return med, lists_ref(side)


# ---------------------------------------------------------------------------
# rank cases
BIG_N = 263169
BIG_RUN = (261000, 263169)  # node ids [a, b) of the equal-key run
BIG_C = 0.125


def big_rank_vector():
    rng = np.random.default_rng(77)
    v = rng.standard_normal(BIG_N)
    v[BIG_RUN[0]:BIG_RUN[1]] = BIG_C
    return v


def big_rank_needs():
    """name -> need, the number of the run's keys side 1 takes: the last one
    taken is node BIG_RUN[0] + need - 1."""
    a, b = BIG_RUN
    return {
        "blk254-last": 261120 - a,          # the last key taken ends block 254
        "blk255-first": 261120 - a + 1,     # block 255's first node
        "blk255": 600,
        "blk256-first": 262144 - a + 1,
        "blk256": 1500,
        "blk256-last": 263168 - a,          # block 257's only node is the first one not taken
        "blk257": b - a,                    # the whole run: block 257's node is the last taken
    }


@functools.lru_cache(maxsize=None)
def rank_cases():
    """name -> (v, n1), 1 <= n1 < n."""
    out = {}
    for name, v, n1 in rank_split_cases() + [rank_split_big_case()]:
        if 1 <= n1 < len(v):
            out[name] = (v, n1)
    v = big_rank_vector()
    below = int((ord_key(v) < ord_key(np.array([BIG_C]))[0]).sum())
    for name, need in big_rank_needs().items():
        out[f"trip2-{name}"] = (v, below + need)
    out["trip2-n1-1"] = (v, 1)
    out["trip2-n1-last"] = (v, BIG_N - 1)
    for v, _ in out.values():
        v.setflags(write=False)
    return out


def rank_ns():
    return sorted({len(v) for v, _ in rank_cases().values()})


def rank_cases_of(n):
    return {k: c for k, c in rank_cases().items() if len(c[0]) == n}


@functools.lru_cache(maxsize=None)
def rank_expected(name):
    v, n1 = rank_cases()[name]
    return lists_ref(rank_ref(v, n1))


# ---------------------------------------------------------------------------
def ring_csr(n):
    """(rowptr, col, w) of the n-ring: two unit-weight neighbours a node (n >= 3;
    n = 2 has one, n = 1 none)."""
    i = np.arange(n, dtype=np.int64)
    if n >= 3:
        col = np.sort(np.stack([(i - 1) % n, (i + 1) % n], axis=1), axis=1).ravel()
        deg = 2
    elif n == 2:
        col, deg = np.array([1, 0]), 1
    else:
        col, deg = np.zeros(0, np.int64), 0
    return (np.arange(n + 1, dtype=np.int32) * deg), col.astype(np.int32), np.ones(len(col), np.float32)
