"""NumPy float64 reference of one K-Means Lloyd pass (``ops.dense.kmeans_step``:
kmeans_mfma_kernel / kmeans_wave_kernel of ``csrc/kmeans_wave.hip``,
kmeans_kernel and the staged GEMM path of ``csrc/dense_kernels.hip``).

The operation: X feature-major [d][n] (NaN cells count as 0), C [k][d];

    dist[c][r] = ||c||^2 - 2 c . x_r        assign[r] = argmin_c, lowest c on ties
    sums[c]    = sum of the rows of c       counts[c] = their number
    sse[c]     = sum over them of max(dist[assign[r]][r] + ||x_r||^2, 0)

Two classes of test data:

* grid (:func:`grid_case`): every value of X and C is a multiple of 1/2 in
  [-1.5, 1.5] and ``36 d n < 2^24``.  A product is then a multiple of 1/4 of
  magnitude <= 2.25, a dot-product partial and ||c||^2, ||x||^2 are multiples of
  1/4 below 2.25 d, a distance and a row SSE (<= (1.5 + 1.5)^2 d = 9 d) too, and
  every partial sum of row SSEs or of cluster sums is a multiple of 1/4 below
  9 d n: all of them integers below 2^24 in units of 1/4, hence exactly
  representable in float32 whatever the order of accumulation, fused or not.
  A correct kernel of any design reproduces :func:`lloyd` bit for bit - the
  assignment with all its ties, the sums, the counts, the SSE.
* rounded (continuous data): an fp32 distance may differ from the float64 one
  and flip a near-tie.  :func:`flip_bound` bounds one fp32 evaluation of
  ``||c||^2 - 2 c . x`` to first order by four terms,

      dot product   gamma_(d+1) sum_f |c_f x_f|, any summation order, FMA or not,
                    one sum or an (even, odd) pair of partial sums: at most d
                    roundings on the path of a product, one more for the pair
      doubling      exact
      ||c||^2       one rounding of the float64 sum to float32
      subtraction   one rounding, of a result below ||c||^2 + 2 sum_f |c_f x_f|

  together at most ``(d + 4) 2^-24 (||c||^2 + 2 sum_f |c_f| |x_f|)``; the
  factor 1.01 absorbs the second-order terms ((d + 4) 2^-24 << 0.01).  A row
  on which a kernel and :func:`lloyd` disagree is justified only if

      dist[a_gpu][r] - dist[a_ref][r] <= B[a_gpu][r] + B[a_ref][r].

Plain NumPy float64; no code shared with ``h2omx.reference.dense.kmeans_step``
and no HIP code is called from here.
"""
from __future__ import annotations

import numpy as np

GRID_LIMIT = 1 << 24
GRID_VALUES = np.arange(-3, 4) / 2.0          # the multiples of 1/2 in [-1.5, 1.5]
U24 = 2.0 ** -24                              # unit roundoff of float32


def _x64(X) -> np.ndarray:
    X = np.asarray(X, dtype=np.float64)
    return np.where(np.isnan(X), 0.0, X)


def distances(X, C) -> np.ndarray:
    """dist[k][n] = ||c||^2 - 2 c . x in float64 (NaN cells of X as 0)"""
    X, C = _x64(X), np.asarray(C, dtype=np.float64)
    return (C * C).sum(1)[:, None] - 2.0 * (C @ X)


def given(X, C, assign):
    """(sums [k][d], counts [k], sse [k]) in float64 of the assignment ``assign``"""
    X, C = _x64(X), np.asarray(C, dtype=np.float64)
    assign = np.asarray(assign).astype(np.int64)
    k, n = C.shape[0], X.shape[1]
    if assign.shape != (n,) or (n and (assign.min() < 0 or assign.max() >= k)):
        raise ValueError("assign: one cluster id in [0, k) per row")
    onehot = np.zeros((k, n))
    onehot[assign, np.arange(n)] = 1.0
    sums = onehot @ X.T
    counts = np.bincount(assign, minlength=k).astype(np.float64)
    own = distances(X, C)[assign, np.arange(n)]
    row_sse = np.maximum(own + (X * X).sum(0), 0.0)
    sse = np.bincount(assign, weights=row_sse, minlength=k)
    return sums, counts, sse


def lloyd(X, C):
    """(assign int32 [n], sums [k][d], counts [k], sse [k]); lowest index on ties"""
    assign = np.argmin(distances(X, C), axis=0).astype(np.int32)   # first minimum = lowest index
    return (assign,) + given(X, C, assign)


def flip_bound(X, C) -> np.ndarray:
    """B[k][n]: bound on |fp32 dist - float64 dist| (module docstring)"""
    X, C = _x64(X), np.asarray(C, dtype=np.float64)
    d = X.shape[0]
    return 1.01 * (d + 4) * U24 * ((C * C).sum(1)[:, None] + 2.0 * (np.abs(C) @ np.abs(X)))


def flips(X, C, assign):
    """(rows on which ``assign`` differs from lloyd's, which of them flip_bound justifies)"""
    D = distances(X, C)
    ref = np.argmin(D, axis=0)
    assign = np.asarray(assign).astype(np.int64)
    rows = np.nonzero(assign != ref)[0]
    B = flip_bound(X, C)
    a, b = assign[rows], ref[rows]
    return rows, D[a, rows] - D[b, rows] <= B[a, rows] + B[b, rows]


def tied_rows(X, C, k_live=None) -> np.ndarray:
    """rows whose minimum distance is attained by two or more of the first ``k_live`` clusters"""
    D = distances(X, C)[:k_live]
    return np.nonzero((D == D.min(0)).sum(0) >= 2)[0]


def grid_case(d: int, k: int, n: int, seed: int, nan_cells: int = 0, dup: bool = False):
    """(X float32 [d][n], C float32 [k][d]) on the grid of the module docstring:
    uniform draws from the multiples of 1/2 in [-1.5, 1.5], ``nan_cells`` cells
    of X set to NaN, with ``dup`` the last centroid a copy of centroid 0 (it
    loses every tie, so it ends empty).

    Independent draws alone leave clusters empty once k is large for n (17 to
    25 of 150 at d = 520, n = 800), and an empty cluster's slab entries prove
    nothing.  So when ``n >= k`` each centroid is also planted as one row of X,
    at distinct random rows: a row equal to a centroid is at distance
    -||c||^2 from it and no closer to any other (||c - c'||^2 >= 0).  The
    values stay on the grid; a NaN cell may still land on a planted row."""
    if not 36 * d * n < GRID_LIMIT:
        raise ValueError(f"grid_case: 36 * {d} * {n} >= 2^24: fp32 sums would not be exact")
    if dup and k < 2:
        raise ValueError("grid_case: dup needs k >= 2")
    rng = np.random.default_rng(seed)
    X = rng.choice(GRID_VALUES, size=(d, n)).astype(np.float32)
    C = rng.choice(GRID_VALUES, size=(k, d)).astype(np.float32)
    if n >= k:
        X[:, rng.choice(n, size=k, replace=False)] = C.T
    if nan_cells:
        cells = rng.choice(d * n, size=min(nan_cells, d * n), replace=False)
        X.reshape(-1)[cells] = np.nan
    if dup:
        C[-1] = C[0]
    return X, C


def rounded_case(d: int, k: int, n: int, seed: int, nan_cells: int = 50):
    """(X, C) float32 of continuous data: standard normal X and C, ``nan_cells``
    NaN cells, the last centroid moved 50 away in every feature (empty cluster)"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(d, n)).astype(np.float32)
    C = rng.normal(size=(k, d)).astype(np.float32)
    X[rng.integers(0, d, nan_cells), rng.integers(0, n, nan_cells)] = np.nan
    C[-1] += 50.0
    return X, C


# ---------------------------------------------------------------------------
# The cases of tests/test_kmeans_oracle_gpu.py; tests/test_kmref.py proves on
# the CPU that each grid case is exact in float32 and has ties to break.
# ---------------------------------------------------------------------------
GRID_ROWS = (4099, 3001, 2051, 1500, 800)


def grid_rows(d: int) -> int:
    """the largest row count of GRID_ROWS that keeps d features on the exact grid"""
    return next(n for n in GRID_ROWS if 36 * d * n < GRID_LIMIT)


class GridCase:
    """One grid-class case: the route kmeans_step must take for (d, k) under the
    module flags KM_MFMA / KM_WAVE of h2omx.ops.dense, and its data."""

    def __init__(self, route: str, d: int, k: int, n: int | None = None, mfma: bool = True, wave: bool = True):
        self.route, self.d, self.k, self.mfma, self.wave = route, d, k, mfma, wave
        self.n = grid_rows(d) if n is None else n
        self.dup = k >= 2
        self.seed = 1000 * d + k + 7 * self.n + 1   # +1: (4, 3) draws two live centroids that can tie
        flags = "" if mfma and wave else ("-nomfma" if wave else "-nomfma-nowave")
        self.id = f"{route}{flags}-d{d}-k{k}-n{self.n}"

    def data(self):
        return grid_case(self.d, self.k, self.n, self.seed, nan_cells=max(1, self.d * self.n // 100), dup=self.dup)

    @property
    def k_live(self) -> int:
        return self.k - 1 if self.dup else self.k

    def __repr__(self):
        return self.id


def _cases(route, shapes, **flags):
    return [GridCase(route, d, k, **flags) for d, k in shapes]


MFMA_SHAPES = [(1, 1), (14, 4), (15, 5), (30, 12), (46, 17), (62, 32), (110, 13), (126, 16)]
# shapes that more than one fused kernel accepts, with those kernels.  d = 64 at
# k = 32 is one feature block past the MFMA kernel (d + 2 <= 64 above 16
# clusters); (62, 32) is its largest shape of that branch
SHARED_SHAPES = [(4, 3, ("mfma", "wave", "tile")), (33, 16, ("mfma", "wave", "tile")),
                 (62, 32, ("mfma", "wave", "tile")), (64, 32, ("wave", "tile"))]
GRID_TABLE = (
    _cases("mfma", MFMA_SHAPES)
    + _cases("wave", [(127, 8), (63, 20)])                                   # one past MFMA's nt limits
    + _cases("wave", [(4, 3), (33, 16), (100, 10), (64, 32)], mfma=False)
    + _cases("tile", [(20, 40), (20, 100), (50, 50), (64, 128), (100, 64), (200, 8), (256, 32)])
    + _cases("tile", [(4, 3), (64, 17), (128, 16)], mfma=False, wave=False)
    + _cases("large", [(65, 128), (129, 33), (257, 2), (10, 129), (520, 150)])
)
ROW_EDGES = [GridCase(route, d, k, n, **flags)
             for route, d, k, flags in [("mfma", 30, 12, {}), ("wave", 33, 16, dict(mfma=False)), ("tile", 20, 40, {}),
                                        ("large", 10, 129, {})]
             for n in (1, 63, 64, 65, 1025)] + [GridCase("tile", 32, 40, 8200)]   # three workgroups of 2752 rows
# (case, chunk rows): _kmeans_large in several chunks with a ragged last one
CHUNKED = [(GridCase("large", 40, 200, 2500), 1000), (GridCase("large", 300, 5, 1500), 640)]
# (route, d, k, flags) of the rounded class, n = ROUNDED_ROWS each
ROUNDED_ROWS = 20_011
ROUNDED = [("mfma", 28, 10, {}), ("wave", 100, 10, dict(mfma=False)), ("tile", 64, 40, {}), ("large", 300, 5, {})]
