"""Small graphs with known spectra for the Lanczos solve, as hypergraphs (so the
same pins go to Hypergraph.laplacian(), to spmv_setup_pins and to the oracle),
with the dense-eigensolver reference and the bounds derived from it.  Shared by
test_lanczos_cases_host.py (the references against the analytic spectra, the
class of each case) and test_gpu_lanczos_small.py (the solver against them).

2-pin nets are unit edges, a repeated net an integer weight, and a net of k
pins adds 2/k to each pair of its clique (cEIG.cpp:86-133)."""
import functools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
PATHS = (4, 5, 6, 7, 8, 9, 31, 32, 33, 63, 64, 65, 159, 160, 161, 1023, 1024, 1025, 2049)
MODE_CASES = ("path-5", "path-33", "path-1025", "complete-8", "star-9", "barbell")
MODES = ({"reorth": 1}, {"reorth": 2}, {"basis32": False}, {"check_every": 0}, {"keep_min": 0}, {"deflate": False})


def _path(n, first=0):
    return [[first + i, first + i + 1] for i in range(n - 1)]


def _complete(n, first=0):
    return [[first + i, first + j] for i in range(n) for j in range(i + 1, n)]


def _grid(rows, cols):
    at = lambda r, c: r * cols + c
    return ([[at(r, c), at(r, c + 1)] for r in range(rows) for c in range(cols - 1)] +
            [[at(r, c), at(r + 1, c)] for r in range(rows - 1) for c in range(cols)])


def _random_connected(n, seed):
    """A random spanning tree, 1.5 n more edges (some repeated 2 or 3 times: integer
    weights) and n / 10 nets of 3 and 4 pins (weights 2/3 and 1/2)."""
    rng = np.random.default_rng(seed)
    nets = [[int(rng.integers(0, i)), i] for i in range(1, n)]
    for _ in range(3 * n // 2):
        a, b = rng.choice(n, 2, replace=False)
        nets.extend([[int(a), int(b)]] * int(rng.choice([1, 1, 1, 2, 3])))
    for _ in range(max(2, n // 10)):
        nets.append([int(p) for p in rng.choice(n, int(rng.integers(3, 5)), replace=False)])
    return nets


def _graphs():
    """name -> (nodes, nets, analytic lambda_2 or None, disconnected)."""
    g = {}
    for n in PATHS:
        g[f"path-{n}"] = (n, _path(n), 2 - 2 * math.cos(math.pi / n), False)
    # two K12 joined by a path through 8 more nodes
    g["barbell"] = (32, _complete(12) + _path(10, 11) + _complete(12, 20), None, False)
    for n in (40, 300, 1500):
        g[f"random-{n}"] = (n, _random_connected(n, n), None, False)
    g["grid-7x11"] = (77, _grid(7, 11), 2 - 2 * math.cos(math.pi / 11), False)
    for n in (6, 64, 1024):
        g[f"cycle-{n}"] = (n, _path(n) + [[n - 1, 0]], 2 - 2 * math.cos(2 * math.pi / n), False)
    g["grid-8x8"] = (64, _grid(8, 8), 2 - 2 * math.cos(math.pi / 8), False)
    for n in (4, 8, 64):
        g[f"complete-{n}"] = (n, _complete(n), float(n), False)
    for n in (9, 65):
        g[f"star-{n}"] = (n, [[0, i] for i in range(1, n)], 1.0, False)
    g["paths-40+60"] = (100, _path(40) + _path(60, 40), 0.0, True)
    g["k5+k5+path-20"] = (30, _complete(5) + _complete(5, 5) + _path(20, 10), 0.0, True)
    return g


GRAPHS = _graphs()
NAMES = tuple(GRAPHS)


def pins_of(name):
    """(nodes, net_ptr int64, pins int32)"""
    n, nets = GRAPHS[name][:2]
    ptr = np.concatenate([[0], np.cumsum([len(e) for e in nets])]).astype(np.int64)
    return n, ptr, np.array([p for e in nets for p in e], np.int32)


def dense_laplacian(name):
    """The clique Laplacian straight from the nets, in fp64."""
    n, nets = GRAPHS[name][:2]
    L = np.zeros((n, n))
    for e in nets:
        w = 2.0 / len(e)
        for i in e:
            for j in e:
                if i != j:
                    L[i, j] -= w
                    L[i, i] += w
    return L


def dense_of_csr(n, csr):
    L = np.zeros((n, n))
    np.add.at(L, (np.repeat(np.arange(n), np.diff(csr.rowptr)), csr.col), csr.val)
    return L


class Ref:
    """numpy.linalg.eigh of the dense Laplacian and what the bounds need."""

    def __init__(self, name, L):
        self.name, self.L, self.n = name, L, len(L)
        self.analytic, self.disconnected = GRAPHS[name][2:]
        self.w, self.U = np.linalg.eigh(L)
        self.norm2 = float(max(abs(self.w[0]), abs(self.w[-1])))
        # eigh's backward error: each computed eigenvalue is exact for L + E, ||E|| <= ~n eps ||L||
        self.eig_err = 4 * self.n * EPS * self.norm2
        self.lam2 = float(self.w[1])
        self.rel_gap = float((self.w[2] - self.w[1]) / self.w[-1])
        self.degenerate = self.rel_gap < 1e-4
        # the lambda_2 eigenspace: the eigenvalues eigh cannot tell from w[1] (equal in exact arithmetic)
        hi = 1
        while hi + 1 < self.n and self.w[hi + 1] - self.w[1] <= 2 * self.eig_err:
            hi += 1
        lo = 0 if self.w[1] - self.w[0] <= 2 * self.eig_err else 1  # disconnected: the null space
        self.space = self.U[:, lo:hi + 1]
        # to the next distinct eigenvalue (non-degenerate: w[2] - w[1]; the solver deflates the null vector)
        self.gap = float(self.w[hi + 1] - self.w[1]) if hi + 1 < self.n else float("inf")
        self.klass = "disconnected" if self.disconnected else "degenerate" if self.degenerate else "nondegenerate"

    def bound(self, r):
        """|lambda - lambda_2| <= r + 4 n eps ||L||: a Ritz value lies within its
        residual of an eigenvalue, and eigh's is that far from the true one."""
        return r + self.eig_err

    def angle(self, r):
        """Davis-Kahan: distance of a unit Ritz vector from the eigenspace."""
        return 2 * self.bound(r) / self.gap

    def residual(self, lam, v):
        """||L v - lam v||_2 in extended precision."""
        Lx = self.L.astype(np.longdouble)
        vx = np.asarray(v, np.longdouble)
        return float(np.sqrt(np.sum((Lx @ vx - np.longdouble(lam) * vx) ** 2)))

    def outside_band(self, r, median):
        """Nodes whose reference entry is further than the Davis-Kahan band from the
        reference's median (median_split's)."""
        return np.abs(self.U[:, 1] - median) > self.angle(r)


@functools.lru_cache(maxsize=None)
def reference(name):
    return Ref(name, dense_laplacian(name))


def check_pair(ek, name, lam, v, st, what=""):
    """The solver's pair (lam, v, stats) against the dense-eigensolver reference
    of `name`, with the bounds of this module (test_gpu_lanczos_small.py and,
    per rank, test_gpu_mr_small.py)."""
    ref = reference(name)
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
