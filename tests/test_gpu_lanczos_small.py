"""The Lanczos solve on small graphs with known spectra (lanczos_cases.py; the
references are proved in test_lanczos_cases_host.py), through the route
ek_partition_kway takes (spmv_setup_pins on the pins), against
numpy.linalg.eigh of the dense Laplacian.  Paths of 4..2,049 nodes cross the
small-n branches (ncv = n/2 below 160, a basis that is mostly padding, one row
block); K_n and the star exhaust their Krylov space after one or two steps.

Bounds, with r = ||L v - lambda v||_2 computed here in extended precision from
the dense L, and e = 4 n eps ||L||_2 (eigh's own backward error):
  |lambda - lambda_2|         <= r + e      (a Ritz value lies within its residual of an eigenvalue)
  ||v - eigenspace||_2        <= 2 (r + e) / gap          (Davis-Kahan)
Run on an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import lanczos_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def _setup(ek, ctx, name):
    n, net_ptr, pins = lc.pins_of(name)
    h = ek.Hypergraph.from_pins(n, net_ptr, pins)
    ctx.spmv_setup_pins(h)
    return h


def _check(ek, name, lam, v, st, what=""):
    ref = lc.reference(name)
    assert st["converged"], st
    assert np.all(np.isfinite(v)) and np.isfinite(lam)
    r = ref.residual(lam, v)
    b = ref.bound(r)
    print(f"{name} {what}: {ref.klass}, matvecs {st['matvecs']}, restarts {st['restarts']}, residual {r:.3g}, "
          f"|lambda - ref| {abs(lam - ref.lam2):.3g} (bound {b:.3g})")
    if ref.klass == "disconnected":
        assert r <= 1e-8 and abs(lam) <= 1e-8
    else:
        assert r <= 1e-9
    assert abs(np.linalg.norm(v) - 1) <= 1e-12 and abs(v.sum()) <= 1e-8
    assert abs(lam - ref.lam2) <= b, (lam, ref.lam2)
    if ref.w[2] - ref.w[1] > 2 * b:  # the second eigenvalue, not just some eigenvalue
        assert abs(lam - ref.w[1]) < abs(lam - ref.w[2])
    if ref.klass == "nondegenerate":
        v_ref = ref.U[:, 1]
        v = v * np.sign(v @ v_ref)
        band = ref.angle(r)
        assert np.linalg.norm(v - v_ref) <= band, (np.linalg.norm(v - v_ref), band)
        med_ref, bits_ref = ek.median_split(v_ref)
        _, bits = ek.median_split(v)
        mask = ref.outside_band(r, med_ref)
        print(f"{name} {what}: outside the Davis-Kahan band {int(mask.sum())}/{ref.n} = {mask.mean():.4f}")
        assert np.array_equal(bits[mask], bits_ref[mask])
    elif np.isfinite(ref.gap):  # (K_n: every vector orthogonal to 1 is an eigenvector; |sum v| above)
        off = np.linalg.norm(v - ref.space @ (ref.space.T @ v))
        assert off <= ref.angle(r), (off, ref.angle(r))


@pytest.mark.parametrize("name", lc.NAMES)
def test_fiedler_pair_against_dense_eigensolver(ek, ctx, name):
    _setup(ek, ctx, name)
    lam, v, st = ctx.lanczos_fiedler()
    _check(ek, name, lam, v, st, "default")
    lam2, v2, st2 = ctx.lanczos_fiedler()  # the same bits on the resident matrix
    assert lam == lam2 and np.array_equal(v.view(np.uint64), v2.view(np.uint64)) and st["matvecs"] == st2["matvecs"]


def _mode_id(m):
    return ",".join(f"{k}={v}" for k, v in m.items())


@pytest.mark.parametrize("mode", lc.MODES, ids=_mode_id)
@pytest.mark.parametrize("name", lc.MODE_CASES)
def test_fiedler_pair_modes(ek, ctx, name, mode):
    """Full and CGS2 reorthogonalisation, the fp64 basis, end-of-cycle checks,
    Spectra's restart size and the undeflated solve: the same bars."""
    _setup(ek, ctx, name)
    n = lc.reference(name).n
    if mode.get("deflate") is False and min(n // 2, n) <= 2:
        with pytest.raises(ek.EKError) as e:  # ncv <= nev = 2 (ek_lanczos_fiedler, "graph too small")
            ctx.lanczos_fiedler(**mode)
        assert e.value.code == ek.EK_EINVAL
        return
    lam, v, st = ctx.lanczos_fiedler(**mode)
    _check(ek, name, lam, v, st, _mode_id(mode))
