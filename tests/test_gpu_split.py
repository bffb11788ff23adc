"""The device median and rank splits (k_select_*, k_split_*, k_rank_*) on
injected vectors at their edges (split_cases.py): ek_fiedler_set puts a chosen
vector where a Lanczos solve leaves its own, ek_kl_partition_copy reads back
the lists, plist and sides the kernels wrote, and every array is compared
element for element with a plain-numpy reference and with the host route
(ek_median_split / ek_rank_split + ek_kl_set_partition_bits).  No tolerance
anywhere: integers, and the median by value.

The graph under every case is the ring of its n nodes (the split kernels read
none of it; the partition's descriptors need one), set up once per n."""
import numpy as np
import pytest

import split_cases as sc
from conftest import swap_fields_equal

pytestmark = pytest.mark.gpu

ARRAYS = ("order0", "order1", "plist", "side")
NO_NETS = (np.zeros(1, np.int64), np.zeros(0, np.int32))


def _ring(ek, c, n):
    c.kl_graph_setup(ek.CSR(*sc.ring_csr(n)))
    c.kl_nets_setup(*NO_NETS)
    return c


@pytest.fixture(scope="module")
def rings(ek):
    """n -> a context holding the n-ring, built on first use and kept for the module."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = _ring(ek, ek.Context(0), n)
        return made[n]

    yield get
    for c in made.values():
        c.close()


def _same(got, exp, what):
    assert (got["n0"], got["n1"]) == (exp["n0"], exp["n1"]), (what, got["n0"], got["n1"], exp["n0"], exp["n1"])
    for k in ARRAYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k)
        bad = np.flatnonzero(got[k] != exp[k])
        assert bad.size == 0, (what, k, int(bad.size), int(bad[0]), int(got[k][bad[0]]), int(exp[k][bad[0]]))


def _lists_are_a_partition(got, n, what):
    o0, o1 = got["order0"].astype(np.int64), got["order1"].astype(np.int64)
    assert np.all(np.diff(o0) > 0) and np.all(np.diff(o1) > 0), what          # ascending
    both = np.concatenate([o0, o1])
    assert both.size == n and np.array_equal(np.sort(both), np.arange(n)), what  # disjoint, cover 0..n-1


def _median_route(c, v):
    c.fiedler_set(v)
    med, n0, n1 = c.kl_set_partition_fiedler()
    got = c.kl_partition_copy()
    assert (n0, n1) == (got["n0"], got["n1"])
    return med, got


def _rank_route(c, v, n1):
    c.fiedler_set(v)
    a, b = c.kl_set_partition_fiedler_rank(n1)
    got = c.kl_partition_copy()
    assert (a, b) == (got["n0"], got["n1"])
    return got


@pytest.mark.parametrize("n", sc.median_ns())
def test_median_split_equals_reference(ek, rings, n):
    c = rings(n)
    for name, v in sc.median_cases_of(n).items():
        want_med, exp = sc.median_expected(name)
        med, got = _median_route(c, v)
        if "signed-zeros" in name:  # == does not see a zero's sign, nor does the split: reported, not asserted
            print(f"{name}: median sign bit device {int(np.signbit(med))}, host "
                  f"{int(np.signbit(ek.median_split(v)[0]))}, reference {int(np.signbit(want_med))}")
        assert sc.same_value(med, want_med), (name, med, want_med)
        if want_med == want_med:
            assert med == want_med, (name, med, want_med)
        _same(got, exp, name + " (device)")
        # the host route: the same arrays, so the two routes agree
        host_med, bits = ek.median_split(v)
        assert sc.same_value(host_med, med), (name, host_med, med)
        c.kl_set_partition_bits(bits)
        host = c.kl_partition_copy()
        _same(host, exp, name + " (host)")
        _lists_are_a_partition(host, n, name)
        _lists_are_a_partition(got, n, name)


@pytest.mark.parametrize("n", sc.rank_ns())
def test_rank_split_equals_reference(ek, rings, n):
    c = rings(n)
    for name, (v, n1) in sc.rank_cases_of(n).items():
        exp = sc.rank_expected(name)
        assert exp["n1"] == n1
        got = _rank_route(c, v, n1)
        _same(got, exp, name + " (device)")
        c.kl_set_partition_bits(ek.rank_split(v, n1))
        host = c.kl_partition_copy()
        _same(host, exp, name + " (host)")
        _lists_are_a_partition(got, n, name)
        dev_bits = c.rank_split_device(v, n1)
        assert np.array_equal(dev_bits, exp["side"]), (name, int(dev_bits.sum()), n1)


def test_reuse_of_a_context_leaves_nothing_behind(ek, rings):
    """A large split, a small one, the large one again, median and rank routes
    mixed, on one context: each equals the same split on a context that ran
    nothing else (stale sp_tmp / rk_tmp contents would show)."""
    big_m, small_m = "trip2-random-263169", "tie-both-wide-2050"
    big_r, small_r = "trip2-blk256", next(k for k in sc.rank_cases() if k.startswith("ties-"))
    steps = [("m", big_m), ("r", small_r), ("r", big_r), ("m", small_m), ("m", big_m), ("r", big_r), ("m", small_m),
             ("r", small_r)]

    def run(c, kind, name):
        if kind == "m":
            v = sc.median_cases()[name]
            if getattr(c, "kl_n", 0) != len(v):
                _ring(ek, c, len(v))
            return _median_route(c, v)
        v, n1 = sc.rank_cases()[name]
        if getattr(c, "kl_n", 0) != len(v):
            _ring(ek, c, len(v))
        return None, _rank_route(c, v, n1)

    fresh = {}
    for kind, name in dict.fromkeys(steps):
        n = len(sc.median_cases()[name]) if kind == "m" else len(sc.rank_cases()[name][0])
        one = _ring(ek, ek.Context(0), n)
        try:
            fresh[kind, name] = run(one, kind, name)
        finally:
            one.close()
    c = ek.Context(0)
    try:
        for kind, name in steps:
            med, got = run(c, kind, name)
            fmed, fgot = fresh[kind, name]
            assert med == fmed, (kind, name)
            _same(got, fgot, f"{kind} {name} (reused context)")
            _same(got, sc.median_expected(name)[1] if kind == "m" else sc.rank_expected(name), name)
    finally:
        c.close()


@pytest.mark.parametrize("name", ("tie-both-wide-2050", "tie-lo-only-ends-2050"))
def test_kl_run_after_device_split_equals_host_route(ek, rings, name):
    c = rings(2050)
    v = sc.median_cases()[name]
    _median_route(c, v)
    log_d, res_d = c.kl_run()
    c.kl_set_partition_bits(ek.median_split(v)[1])
    log_h, res_h = c.kl_run()
    assert res_d["iterations"] > 0
    swap_fields_equal(log_d, log_h)
    for k in ("iterations", "best_iter", "net_cut_initial", "net_cut_best", "net_cut_final"):
        assert res_d[k] == res_h[k], (k, res_d[k], res_h[k])
    for k in ("initial_cut", "best_cut", "final_cut"):
        assert np.float32(res_d[k]).view(np.uint32) == np.float32(res_h[k]).view(np.uint32), (k, res_d[k], res_h[k])
    # the copy is of the partition as set: the run did not touch it
    _same(c.kl_partition_copy(), sc.median_expected(name)[1], name + " after kl_run")


def test_error_paths(ek):
    def code(call):
        with pytest.raises(ek.EKError) as e:
            call()
        return e.value.code

    c = ek.Context(0)
    try:
        v = np.arange(8, dtype=np.float64)
        bad = v.copy()
        bad[5] = np.nan
        assert code(lambda: c.fiedler_set(bad)) == ek.EK_EINVAL
        assert code(lambda: c.fiedler_set(None)) == ek.EK_EINVAL
        assert code(lambda: c.fiedler_set(np.zeros(0))) == ek.EK_EINVAL
        assert code(c.kl_partition_copy) == ek.EK_ESTATE            # no graph, no partition
        _ring(ek, c, 8)
        assert code(c.kl_partition_copy) == ek.EK_ESTATE            # a graph, no partition yet
        assert code(c.kl_set_partition_fiedler) == ek.EK_ESTATE     # the refused vectors left nothing behind
        c.fiedler_set(np.arange(7, dtype=np.float64))
        assert code(c.kl_set_partition_fiedler) == ek.EK_ESTATE     # 7 entries on a graph of 8
        assert code(lambda: c.kl_set_partition_fiedler_rank(3)) == ek.EK_ESTATE
        c.fiedler_set(v)
        for n1 in (0, 8):
            assert code(lambda: c.kl_set_partition_fiedler_rank(n1)) == ek.EK_EINVAL
        assert code(c.kl_partition_copy) == ek.EK_ESTATE            # the refused calls set none
        c.fiedler_set(np.array([3.0, -np.inf, 1.0, np.inf, 0.0, -0.0, 2.0, -1.0]))  # infinities are accepted
        assert c.kl_set_partition_fiedler() == (0.5, 4, 4)
        assert c.kl_partition_copy()["side"].tolist() == [0, 1, 0, 0, 1, 1, 0, 1]
        # a new graph voids the partition
        _ring(ek, c, 8)
        assert code(c.kl_partition_copy) == ek.EK_ESTATE

        def never(*_):
            raise AssertionError("a collective ran")
        c.comm_init_host(2, 0, never, never)
        assert code(lambda: c.fiedler_set(v)) == ek.EK_ESTATE       # a multi-rank context
    finally:
        c.close()
