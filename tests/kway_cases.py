"""Inputs and plain-Python references shared by test_kway_host.py and
test_gpu_kway.py (the device kernels must agree with the host entry points on
the same cases)."""
import numpy as np


def ord_key(v):
    """The radix order of the device select: the fp64 bit patterns with the sign
    flipped and negatives inverted (-0 before +0)."""
    u = np.ascontiguousarray(v, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def rank_split_ref(v, n1):
    ids = np.arange(len(v))
    order = np.lexsort((ids, ord_key(v)))
    bits = np.zeros(len(v), np.uint8)
    bits[order[:n1]] = 1
    return bits


def rank_split_cases():
    """(name, v, n1) triples."""
    rng = np.random.default_rng(20240611)
    out = []
    for n in (2, 3, 2047, 2048, 2049):
        v = rng.standard_normal(n)
        for n1 in sorted({0, 1, n // 3, n - 1, n}):
            out.append((f"random-{n}-{n1}", v, n1))
    n = 2049
    for n1 in (0, 1, 700, n - 1, n):
        out.append((f"all-equal-{n1}", np.full(n, 0.25), n1))
    z = rng.choice(np.array([0.0, -0.0]), n)
    nneg = int(np.signbit(z).sum())
    for n1 in (0, 1, nneg - 1, nneg, nneg + 1, n - 1, n):
        out.append((f"signed-zeros-{n1}", z, n1))
    t = rng.integers(-2, 3, n).astype(np.float64) * 0.5  # five values, ~410 nodes each
    below = int((t < 0.0).sum())
    for n1 in (below, below + 1, below + 7, below + int((t == 0.0).sum()) - 1):
        out.append((f"ties-{n1}", t, n1))
    return out


def rank_split_big_case():
    """n = 20,000 (10 tiles of the select's 2,048 keys, 20 blocks of the split's
    1,024 nodes): an equal-key run over nodes 2000..2099 crosses the boundary at
    2048, and the rank falls inside it (50 of the run's 100 are taken)."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal(20000)
    c = float(np.median(v))
    v[2000:2100] = c
    n1 = int((ord_key(v) < ord_key(np.array([c]))[0]).sum()) + 50
    return "big-20000", v, n1


def induce_ref(nodes, net_ptr, pins, keep):
    """Plain restatement of ek_hgr_induce: (nodes, net_ptr, pins, node_map)."""
    node_map = np.full(nodes, -1, np.int32)
    kept = np.flatnonzero(np.asarray(keep) != 0)
    node_map[kept] = np.arange(len(kept), dtype=np.int32)
    ptr, out = [0], []
    for e in range(len(net_ptr) - 1):
        sub = [int(node_map[p]) for p in pins[net_ptr[e]:net_ptr[e + 1]] if node_map[p] >= 0]
        if len(sub) >= 2:
            out.extend(sub)
            ptr.append(len(out))
    return len(kept), np.array(ptr, np.int64), np.array(out, np.int32), node_map


def random_hypergraph(seed, nodes=300, nets=400):
    """(nodes, net_ptr, pins): net sizes 1..12, distinct pins in random order."""
    rng = np.random.default_rng(seed)
    ptr, pins = [0], []
    for _ in range(nets):
        pins.extend(rng.choice(nodes, int(rng.integers(1, 13)), replace=False).tolist())
        ptr.append(len(pins))
    return nodes, np.array(ptr, np.int64), np.array(pins, np.int32)


def metrics_ref(net_ptr, pins, part):
    cut = conn = soed = 0
    for e in range(len(net_ptr) - 1):
        lam = len({int(part[p]) for p in pins[net_ptr[e]:net_ptr[e + 1]]})
        if lam >= 2:
            cut += 1
            conn += lam - 1
            soed += lam
    return cut, conn, soed


METRIC_KS = (2, 63, 64, 65, 128, 256)


def metrics_hypergraph():
    """(nodes, net_ptr, pins): nets of 1, 2, 8, 9, 64, 65 and 300 pins, several
    of each in mixed order (8 | 9: one thread or one wave per net; 64 | 65: one
    or two strides of the wave), more than one 256-net workgroup."""
    rng = np.random.default_rng(99)
    nodes = 400
    sizes = np.array([1, 2, 8, 9, 64, 65, 300] * 45)
    rng.shuffle(sizes)
    ptr, pins = [0], []
    for s in sizes:
        pins.extend(rng.choice(nodes, int(s), replace=False).tolist())
        ptr.append(len(pins))
    return nodes, np.array(ptr, np.int64), np.array(pins, np.int32)


def metrics_parts(nodes, k):
    """Part vectors for k: random over all k ids, and random over the two ids
    either side of each 64-bit word of the mask."""
    rng = np.random.default_rng(1000 + k)
    yield rng.integers(0, k, nodes).astype(np.int32)
    edge = np.array(sorted({0, k - 1} | {q for q in (63, 64, 127, 128, 191, 192) if q < k}), np.int32)
    yield edge[rng.integers(0, len(edge), nodes)]
