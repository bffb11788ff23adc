"""The host-only pieces of the k-way path (no GPU): the size plan, the rank
split, the induced sub-hypergraph and the k-way metrics, each against a plain
Python restatement."""
import os
import subprocess

import numpy as np
import pytest

import kway_cases as kc
from conftest import PKG_DIR, circuit_path


@pytest.mark.parametrize("n", [4, 7, 149, 12752, 1000003])
def test_kway_plan_sizes(ek, n):
    for k in (2, 3, 5, 7, 8, 64, 255, 256):
        if n < 2 * k:
            continue
        sizes = ek.kway_plan(n, k)
        assert len(sizes) == k and int(sizes.sum()) == n
        assert set(sizes.tolist()) <= {n // k, -(-n // k)}, (n, k)


def test_kway_plan_rejects(ek):
    for n, k in ((100, 1), (10000, 257), (5, 3), (511, 256), (3, 2)):
        with pytest.raises(ek.EKError) as e:
            ek.kway_plan(n, k)
        assert e.value.code == ek.EK_EINVAL, (n, k)
    assert ek.kway_plan(512, 256).tolist() == [2] * 256


@pytest.mark.parametrize("name,v,n1", kc.rank_split_cases() + [kc.rank_split_big_case()],
                         ids=lambda x: x if isinstance(x, str) else "")
def test_rank_split(ek, name, v, n1):
    bits = ek.rank_split(v, n1)
    assert int(bits.sum()) == n1
    assert np.array_equal(bits, kc.rank_split_ref(v, n1))


def test_rank_split_orientation_and_zeros(ek):
    # the median split's orientation: the smaller values get bit 1
    assert ek.rank_split([3.0, 1.0, 2.0, 0.0], 2).tolist() == [0, 1, 0, 1]
    # -0 sorts before +0, equal keys by ascending id
    assert ek.rank_split([0.0, -0.0, 0.0, -0.0], 1).tolist() == [0, 1, 0, 0]
    assert ek.rank_split([0.0, -0.0, 0.0, -0.0], 3).tolist() == [1, 1, 0, 1]
    with pytest.raises(ek.EKError):
        ek.rank_split([1.0, 2.0], 3)


def _check_induce(ek, h, keep):
    nets, nodes, _ = h.dims()
    net_ptr, pins = h.pins()
    sub, node_map = h.induce(keep)
    rn, rptr, rpins, rmap = kc.induce_ref(nodes, net_ptr, pins, keep)
    sptr, spins = sub.pins()
    assert sub.nodes == rn
    assert np.array_equal(node_map, rmap)
    assert np.array_equal(sptr, rptr) and np.array_equal(spins, rpins)
    assert np.all(np.diff(sptr) >= 2)
    return sub


def test_induce_fract(ek):
    h = ek.Hypergraph.read(circuit_path("fract"))
    rng = np.random.default_rng(3)
    for frac in (0.5, 0.1, 0.9):
        sub = _check_induce(ek, h, rng.random(h.nodes) < frac)
        assert sub.nets < h.nets  # some nets lose all but one pin
    # every node kept: the nets of >= 2 pins, unchanged
    net_ptr, pins = h.pins()
    sub = _check_induce(ek, h, np.ones(h.nodes, np.uint8))
    big = np.flatnonzero(np.diff(net_ptr) >= 2)
    sptr, spins = sub.pins()
    assert sub.nets == len(big)
    assert np.array_equal(spins, np.concatenate([pins[net_ptr[e]:net_ptr[e + 1]] for e in big]))
    with pytest.raises(ek.EKError) as e:
        h.induce(np.zeros(h.nodes, np.uint8))
    assert e.value.code == ek.EK_EINVAL


@pytest.mark.parametrize("seed", [1, 2])
def test_induce_random(ek, seed):
    nodes, net_ptr, pins = kc.random_hypergraph(seed)
    h = ek.Hypergraph.from_pins(nodes, net_ptr, pins)  # pins unsorted: their order must survive
    rng = np.random.default_rng(seed)
    for frac in (0.5, 0.03):
        _check_induce(ek, h, rng.random(nodes) < frac)
    _check_induce(ek, h, np.ones(nodes, np.uint8))
    one = np.zeros(nodes, np.uint8)
    one[17] = 1
    assert _check_induce(ek, h, one).dims() == (0, 1, 0)


@pytest.mark.parametrize("k", kc.METRIC_KS)
def test_kway_metrics_host(ek, k):
    nodes, net_ptr, pins = kc.metrics_hypergraph()
    for part in kc.metrics_parts(nodes, k):
        assert ek.kway_metrics_host(net_ptr, pins, part, k) == kc.metrics_ref(net_ptr, pins, part)
    assert ek.kway_metrics_host(net_ptr, pins, np.full(nodes, k - 1, np.int32), k) == (0, 0, 0)
    with pytest.raises(ek.EKError):
        ek.kway_metrics_host(net_ptr, pins, np.full(nodes, k, np.int32), k)


# --k is refused before the GPU is touched unless the tool is gKL2 and -EIG is given
def test_cli_k_usage_errors(tmp_path):
    fract = circuit_path("fract")
    for args in ((fract, "--k", "4"), (fract, "-EIG", "--k", "1"), (fract, "-EIG", "--k")):
        r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "gKL2"), *args], cwd=tmp_path, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode != 0 and ("Usage" in r.stdout or "Error" in r.stderr), args
    r = subprocess.run([os.path.join(PKG_DIR, "build", "bin", "cKL"), fract, "-EIG", "--k", "4"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Usage" in r.stdout
    assert not (tmp_path / "results").exists() or not list((tmp_path / "results").iterdir())
