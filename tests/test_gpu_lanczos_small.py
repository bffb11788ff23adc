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


@pytest.mark.parametrize("name", lc.NAMES)
def test_fiedler_pair_against_dense_eigensolver(ek, ctx, name):
    _setup(ek, ctx, name)
    lam, v, st = ctx.lanczos_fiedler()
    lc.check_pair(ek, name, lam, v, st, "default")
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
    lc.check_pair(ek, name, lam, v, st, _mode_id(mode))
