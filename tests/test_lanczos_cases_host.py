"""The small-graph Lanczos cases (lanczos_cases.py) are what they claim, with no
GPU: the Laplacian the library builds from the pins is the dense one written
from the nets, L 1 = 0, numpy's eigenvalues match the analytic ones, each case
is classed by its computed gap, and the median-split comparison of the
non-degenerate cases cannot be vacuous."""
import numpy as np
import pytest

import lanczos_cases as lc


@pytest.mark.parametrize("name", lc.NAMES)
def test_case_reference(ek, name):
    ref = lc.reference(name)
    n, net_ptr, pins = lc.pins_of(name)
    h = ek.Hypergraph.from_pins(n, net_ptr, pins)
    assert h.nodes == n == ref.n
    Lh = lc.dense_of_csr(n, h.laplacian())
    round_off = 16 * lc.EPS * ref.norm2  # sums of at most a few dozen terms of at most ||L||
    assert np.abs(Lh - ref.L).max() <= round_off
    assert np.array_equal(ref.L, ref.L.T)
    assert np.abs(ref.L @ np.ones(n)).max() <= round_off and np.abs(Lh @ np.ones(n)).max() <= round_off
    assert abs(ref.w[0]) <= ref.eig_err
    if ref.analytic is not None:
        assert abs(ref.lam2 - ref.analytic) <= ref.eig_err, (ref.lam2, ref.analytic)
    print(name, ref.klass, "rel gap", ref.rel_gap, "gap'", ref.gap, "eigenspace dim", ref.space.shape[1])
    # the class comes from the number
    if ref.disconnected:
        assert ref.klass == "disconnected" and abs(ref.lam2) <= ref.eig_err and ref.space.shape[1] >= 2
        assert ref.space.shape[1] == {"paths-40+60": 2, "k5+k5+path-20": 3}[name]
    else:
        assert ref.w[1] > 1e3 * ref.eig_err  # connected
        assert ref.klass == ("nondegenerate" if ref.rel_gap >= 1e-4 else "degenerate")
        dims = {"cycle": 2, "grid-8x8": 2, "complete": n - 1, "star": n - 2}
        want = next((d for k, d in dims.items() if name.startswith(k)), 1)
        assert ref.space.shape[1] == want
        assert (want > 1) == (ref.rel_gap < 1e-12)
    assert ref.gap > 1e3 * ref.eig_err  # the next distinct eigenvalue is resolved


def test_classes():
    klass = {name: lc.reference(name).klass for name in lc.NAMES}
    nondeg = {k for k, v in klass.items() if v == "nondegenerate"}
    assert {f"path-{n}" for n in lc.PATHS if n <= 161} | {"barbell", "random-40", "random-300", "random-1500",
                                                         "grid-7x11"} <= nondeg
    # the long paths' gaps (3 (pi / n)^2 of a norm of 4) fall below 1e-4: classed by the number
    assert all(klass[f"path-{n}"] == "degenerate" for n in (1023, 1024, 1025, 2049))
    assert all(klass[k] == "degenerate" for k in klass if k.startswith(("cycle", "complete", "star", "grid-8x8")))


@pytest.mark.parametrize("name", [n for n in lc.NAMES if lc.reference(n).klass == "nondegenerate"])
def test_median_split_band_is_not_vacuous(ek, name):
    """With a residual of 1e-9 (the bar), at least 90 % of the nodes lie outside
    the Davis-Kahan band around the reference's median.  An odd path's middle
    node is the median itself (entry 0), always inside: below 10 nodes that one
    node is more than 10 %, so there every other node must lie outside."""
    ref = lc.reference(name)
    med, _ = ek.median_split(ref.U[:, 1])
    outside = ref.outside_band(1e-9, med)
    frac = float(outside.mean())
    print(name, "outside the band at r = 1e-9:", frac)
    if name in ("path-5", "path-7", "path-9"):
        assert int(outside.sum()) == ref.n - 1
    else:
        assert frac >= 0.9
