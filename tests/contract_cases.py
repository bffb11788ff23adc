"""The shared cases of the contraction (ek_hgr_contract on the host, ek_hgr_contract_device on the GPU) and a
plain-Python restatement of the five-step rule of DESIGN.md §14 / §19 that holds the cases themselves to the host
code (test_contract_cases_host.py).  The GPU test (test_gpu_contract.py) expects Hypergraph.contract's result.

A case is a dict: nodes, net_ptr, pins (raw: a pin may repeat), node_w, net_w (None: all ones), cluster, n_coarse,
and error (True: the call must answer EK_EINVAL)."""
import functools

import numpy as np

from conftest import circuit_path

INT32_MAX = 2 ** 31 - 1


def contract_ref(nodes, net_ptr, pins, node_w, net_w, cluster, n_coarse):
    """(node_w, net_ptr, pins, net_w) of the contraction by the rule, Python ints throughout; ValueError where the
    entries answer EK_EINVAL."""
    if n_coarse < 0 or n_coarse > nodes:
        raise ValueError("n_coarse")
    w = [0] * n_coarse
    hit = [False] * n_coarse
    for v in range(nodes):  # 1. cluster weights are summed
        k = int(cluster[v])
        if k < 0 or k >= n_coarse:
            raise ValueError("id out of range")
        hit[k] = True
        w[k] += 1 if node_w is None else int(node_w[v])
    if not all(hit):
        raise ValueError("unhit cluster")
    if any(x > INT32_MAX for x in w):
        raise ValueError("cluster weight")
    kept = {}  # frozenset -> [least index, pins in its order, c]: dicts keep insertion order = ascending least index
    for e in range(len(net_ptr) - 1):
        seen, mapped = set(), []
        for p in pins[net_ptr[e]:net_ptr[e + 1]]:  # 2. mapped, distinct in first-occurrence order
            k = int(cluster[int(p)])
            if k not in seen:
                seen.add(k)
                mapped.append(k)
        if len(mapped) < 2:  # 3. dropped
            continue
        c = 1 if net_w is None else int(net_w[e])
        key = frozenset(mapped)
        if key in kept:  # 4. the same pin set: into the one of least index
            kept[key][2] += c
        else:
            kept[key] = [e, mapped, c]
    out_ptr, out_pins, out_w = [0], [], []
    for _, mapped, c in kept.values():  # 5. ascending least index, the first net's pin order
        if c > INT32_MAX:
            raise ValueError("merged net weight")
        out_pins += mapped
        out_ptr.append(len(out_pins))
        out_w.append(c)
    return (np.array(w, np.int32), np.array(out_ptr, np.int64), np.array(out_pins, np.int32),
            np.array(out_w, np.int32))


def _case(nodes, nets, cluster, n_coarse=None, node_w=None, net_w=None, error=False):
    """nets: a list of pin lists."""
    net_ptr = np.zeros(len(nets) + 1, np.int64)
    net_ptr[1:] = np.cumsum([len(x) for x in nets])
    pins = np.array([p for x in nets for p in x], np.int32)
    cluster = np.array(cluster, np.int32)
    if n_coarse is None:
        n_coarse = int(cluster.max()) + 1
    return dict(nodes=nodes, net_ptr=net_ptr, pins=pins, cluster=cluster, n_coarse=n_coarse,
                node_w=None if node_w is None else np.array(node_w, np.int32),
                net_w=None if net_w is None else np.array(net_w, np.int32), error=error)


def _surjective(rng, nodes, n_coarse):
    """A random map of the nodes onto [0, n_coarse) that hits every value."""
    cl = rng.integers(0, n_coarse, nodes)
    cl[rng.permutation(nodes)[:n_coarse]] = np.arange(n_coarse)
    return cl


def _random_nets(rng, nodes, count, lo, hi):
    return [list(rng.integers(0, nodes, int(rng.integers(lo, hi + 1)))) for _ in range(count)]


def _random(seed, nodes, count, lo=2, hi=12, n_coarse=None, weighted=True):
    rng = np.random.default_rng(seed)
    n_coarse = n_coarse or int(rng.integers(1, nodes + 1))
    return _case(nodes, _random_nets(rng, nodes, count, lo, min(hi, max(lo, nodes))), _surjective(rng, nodes, n_coarse),
                 n_coarse, rng.integers(0, 6, nodes) if weighted else None,
                 rng.integers(1, 4, count) if weighted else None)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in (1, 2, 63, 64, 65, 257):  # around a wave and a workgroup of nodes
        out[f"n{n}"] = _random(100 + n, n, 3 * n, 1, 6, max(1, n // 2))
    for m in (0, 1, 255, 256, 257):  # around a workgroup of nets; 20 clusters of 40 nodes, so many nets merge
        out[f"nets{m}"] = _random(200 + m, 40, m, 2, 4, 20)
    for size in (2, 63, 64, 65, 300):  # a net of that many raw pins, most of them repeats, among short ones
        rng = np.random.default_rng(300 + size)
        nets = _random_nets(rng, 200, 5, 2, 6)
        nets.insert(2, list(rng.integers(0, 200, size)))
        nets.append(list(reversed(nets[2])))  # the same set again, in another order
        out[f"size{size}"] = _case(200, nets, _surjective(rng, 200, 50), 50, net_w=rng.integers(1, 9, len(nets)))
    # a long net whose repeats sit in different 64-pin steps, and one of 130 distinct pins
    out["size_steps"] = _case(140, [list(range(70)) + list(range(70)), list(range(130)), [129, 3] + list(range(130))],
                              np.arange(140) // 1, 140)
    out["inside_one"] = _case(6, [[0, 1, 2], [0, 3], [1, 2, 1]], [0, 0, 0, 1, 2, 2])  # the first and last are dropped
    out["left_two"] = _case(6, [[0, 1, 3, 2, 0], [4, 5]], [0, 0, 0, 1, 2, 2])  # {0, 1} survives, {2} does not
    out["identity"] = _random(401, 50, 120, 2, 5, 50)
    out["identity"]["cluster"] = np.arange(50, dtype=np.int32)
    out["one_cluster"] = _random(402, 30, 40, 2, 5, 1)  # every net is dropped
    out["same2"] = _case(5, [[0, 1, 2], [3, 4], [2, 0, 1]], np.arange(5), net_w=[5, 1, 7])
    out["same3"] = _case(5, [[3, 1], [0, 1, 2], [1, 3], [3, 1, 3]], np.arange(5), net_w=[2, 1, 3, 4])
    rng = np.random.default_rng(403)
    out["same40"] = _case(12, [[7, 2]] + [list(rng.permutation([4, 9, 1, 6, 11])) for _ in range(40)] + [[2, 7]],
                          np.arange(12), net_w=np.arange(1, 43))
    # distinct sets a weak signature confuses: equal size and sum, equal size and XOR
    out["eq_sum"] = _case(8, [[0, 3], [1, 2], [0, 1, 5], [0, 2, 4], [2, 1], [4, 2, 0]], np.arange(8))
    out["eq_xor"] = _case(8, [[1, 2], [4, 7], [7, 4], [2, 1]], np.arange(8), net_w=[1, 2, 3, 4])
    out["superset"] = _case(6, [[0, 1, 2], [0, 1, 2, 3], [0, 1], [3, 2, 1, 0], [1, 0]], np.arange(6))
    out["netw_max"] = _case(4, [[0, 1], [2, 3], [1, 0]], np.arange(4), net_w=[2 ** 30, 1, 2 ** 30 - 1])
    out["netw_over"] = _case(4, [[0, 1], [2, 3], [1, 0]], np.arange(4), net_w=[2 ** 30, 1, 2 ** 30], error=True)
    out["nodew_max"] = _case(4, [[0, 2], [1, 3]], [0, 1, 0, 1], node_w=[2 ** 30, 3, 2 ** 30 - 1, 4])
    out["nodew_over"] = _case(4, [[0, 2], [1, 3]], [0, 1, 0, 1], node_w=[2 ** 30, 3, 2 ** 30, 4], error=True)
    out["id_too_large"] = _case(4, [[0, 1], [2, 3]], [0, 1, 2, 1], n_coarse=2, error=True)
    out["id_negative"] = _case(4, [[0, 1], [2, 3]], [0, -1, 1, 1], n_coarse=2, error=True)
    out["unhit"] = _case(4, [[0, 1], [2, 3]], [0, 2, 2, 0], n_coarse=3, error=True)
    for i in range(30):
        rng = np.random.default_rng(500 + i)
        nodes = int(rng.integers(2, 401))
        out[f"rand{i}"] = _random(600 + i, nodes, int(rng.integers(1, 3 * nodes)), 2, 12)
    return out


def names(error=None):
    return [k for k, c in cases().items() if error is None or c["error"] == error]


def hypergraph(ek, case):
    h = ek.Hypergraph.from_pins(case["nodes"], case["net_ptr"], case["pins"])
    h.set_weights(case["node_w"], case["net_w"])
    return h


def fields(h):
    """Every field of a hypergraph the contract covers: (nodes, nets, net_ptr, pins, node_w, net_w).  A weight array
    the hypergraph does not carry reads as the ones it stands for (an array of no entries is not carried)."""
    nets, nodes, _ = h.dims()
    net_ptr, pins = h.pins()
    node_w, net_w = h.weights()
    node_w = np.ones(nodes, np.int32) if node_w is None else node_w
    net_w = np.ones(nets, np.int32) if net_w is None else net_w
    return nodes, nets, net_ptr, pins, node_w, net_w


def same_fields(a, b):
    """None, or the name of the first field in which two fields() tuples differ (None arrays differ from real ones)."""
    for x, y, what in zip(a, b, ("nodes", "nets", "net_ptr", "pins", "node_w", "net_w")):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if x is None or y is None or x.dtype != y.dtype or not np.array_equal(x, y):
                return what
        elif x != y:
            return what
    return None


def synthetic_weights(nodes, nets):
    """Node weight 1 + (id mod 5), net weight 1 + (e mod 3): the weighting DESIGN.md §12 measured with."""
    return (1 + np.arange(nodes) % 5).astype(np.int32), (1 + np.arange(nets) % 3).astype(np.int32)


CIRCUITS = [("fract", False, 2), ("fract", True, 8), ("ibm01", False, 2), ("ibm01", True, 8)]  # (name, weighted, cap)


def circuit(ek, name, weighted, cap):
    """(a golden circuit with §12's synthetic weights or none, the first level's cluster map by ek.match_host)."""
    h = ek.Hypergraph.read(circuit_path(name))
    if weighted:
        h.set_weights(*synthetic_weights(h.nodes, h.nets))
    _, cluster, _, res = ek.match_host(h, cap)
    return h, cluster, res["n_coarse"]
