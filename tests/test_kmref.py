"""CPU tests of the K-Means Lloyd-pass reference (tests/kmref.py): ``lloyd``
against a brute-force loop, the grid cases of the GPU table proved exact in
float32 under permuted accumulation orders (so the GPU test may ask for equal
bits), their ties and cluster sizes, and ``flip_bound`` against an fp32 NumPy
evaluation of the rounded-class shapes."""
import math

import numpy as np
import pytest

import kmref as KR

ALL_GRID = KR.GRID_TABLE + KR.ROW_EDGES + [c for c, _ in KR.CHUNKED]


def _brute(X, C):
    """the definition, one Python float operation at a time (math.fsum: exact sums)"""
    d, n = len(X), len(X[0])
    k = len(C)
    assign, sums, counts, sse = [], [[0.0] * d for _ in range(k)], [0.0] * k, [0.0] * k
    for r in range(n):
        x = [0.0 if math.isnan(X[f][r]) else float(X[f][r]) for f in range(d)]
        best, bi = math.inf, 0
        for c in range(k):
            dist = math.fsum(float(v) * float(v) for v in C[c]) - 2.0 * math.fsum(float(C[c][f]) * x[f] for f in range(d))
            if dist < best:
                best, bi = dist, c
        assign.append(bi)
        counts[bi] += 1.0
        sse[bi] += max(best + math.fsum(v * v for v in x), 0.0)
        for f in range(d):
            sums[bi][f] += x[f]
    return assign, sums, counts, sse


def test_lloyd_matches_brute_force_on_tiny_inputs():
    nan = float("nan")
    # features in rows; row 1 is equidistant from centroids 0 and 1 (exact tie),
    # row 2 has a NaN cell, centroid 3 duplicates centroid 0
    X = np.array([[0.0, 0.5, nan, 1.5, -1.0, 1.0],
                  [0.0, 0.5, 1.0, 1.0, 0.5, 1.0]], np.float32)
    C = np.array([[0.0, 0.0], [1.0, 1.0], [-1.0, 0.5], [0.0, 0.0]], np.float32)
    a, s, c, e = KR.lloyd(X, C)
    ab, sb, cb, eb = _brute(X.tolist(), C.tolist())
    assert a.dtype == np.int32 and a.tolist() == ab == [0, 0, 0, 1, 2, 1]
    assert s.tolist() == sb and c.tolist() == cb and e.tolist() == eb
    assert c[3] == 0 and 1 in KR.tied_rows(X, C, 3)
    assert s[0].tolist() == [0.5, 1.5]                    # the NaN cell counted as 0
    for seed, (d, k, n) in enumerate([(3, 4, 40), (1, 2, 9), (5, 7, 33)]):
        X, C = KR.grid_case(d, k, n, seed, nan_cells=3, dup=True)
        a, s, c, e = KR.lloyd(X, C)
        ab, sb, cb, eb = _brute(X.tolist(), C.tolist())
        assert a.tolist() == ab and s.tolist() == sb and c.tolist() == cb and e.tolist() == eb
        assert c[-1] == 0 and np.isnan(X).sum() == 3
        s2, c2, e2 = KR.given(X, C, a)
        assert np.array_equal(s2, s) and np.array_equal(c2, c) and np.array_equal(e2, e)
    # given() follows the supplied assignment, not the nearest centroid
    s3, c3, e3 = KR.given(X, C, np.zeros(33, np.int32))
    Xz = np.nan_to_num(X.astype(np.float64))
    assert c3[0] == 33 and np.array_equal(s3[0], Xz.sum(1))
    assert e3[0] == ((Xz - C[0].astype(np.float64)[:, None]) ** 2).sum()   # exact on the grid


def test_grid_case_rejects_sizes_off_the_exact_grid():
    KR.grid_case(126, 4, 3000, 0)
    with pytest.raises(ValueError):
        KR.grid_case(126, 4, 3700, 0)      # 36 * 126 * 3700 >= 2^24
    with pytest.raises(ValueError):
        KR.grid_case(4, 1, 10, 0, dup=True)
    X, C = KR.grid_case(7, 5, 100, 3, nan_cells=9, dup=True)
    assert X.dtype == C.dtype == np.float32 and np.isnan(X).sum() == 9 and np.array_equal(C[-1], C[0])
    assert set(np.unique(np.nan_to_num(X) * 2)) <= set(range(-3, 4)) and set(np.unique(C * 2)) <= set(range(-3, 4))
    assert [c.n for c in KR.GRID_TABLE if (c.d, c.k) in [(110, 13), (126, 16), (200, 8), (256, 32), (520, 150)]] \
        == [4099, 3001, 2051, 1500, 800]


def _fp32_pass(X, C, feat, rows):
    """One Lloyd pass evaluated in float32 only: features accumulated in the
    order ``feat``, rows in the order ``rows``, one rounding per operation."""
    f32 = np.float32
    Xz = np.where(np.isnan(X), f32(0), X).astype(f32)
    k, n = C.shape[0], X.shape[1]
    dot, cn, x2 = np.zeros((k, n), f32), np.zeros(k, f32), np.zeros(n, f32)
    for f in feat:
        dot += C[:, f, None] * Xz[f][None, :]
        cn += C[:, f] * C[:, f]
        x2 += Xz[f] * Xz[f]
    assert dot.dtype == cn.dtype == x2.dtype == f32
    dist = cn[:, None] - f32(2) * dot
    assign = np.argmin(dist, axis=0)
    row_sse = np.maximum(dist[assign, np.arange(n)] + x2, f32(0))
    sums, sse = np.zeros((k, X.shape[0]), f32), np.zeros(k, f32)
    np.add.at(sums, assign[rows], Xz.T[rows])           # unbuffered: one float32 addition per row, in order
    np.add.at(sse, assign[rows], row_sse[rows])
    return dist, assign, sums, sse


@pytest.mark.parametrize("case", ALL_GRID, ids=repr)
def test_grid_cases_are_exact_in_float32(case):
    """Distances, assignment, sums and SSE of every grid case come out of a
    float32-only evaluation equal to the float64 ones, in any order."""
    X, C = case.data()
    assert X.shape == (case.d, case.n) and C.shape == (case.k, case.d) and np.isnan(X).any()
    D64 = KR.distances(X, C)
    a, s, c, e = KR.lloyd(X, C)
    assert max(np.abs(s).max(), e.max(), np.abs(D64).max()) * 4 < KR.GRID_LIMIT
    for seed in range(3):
        rng = np.random.default_rng(seed)
        dist, a32, s32, e32 = _fp32_pass(X, C, rng.permutation(case.d), rng.permutation(case.n))
        assert np.array_equal(dist.astype(np.float64), D64)
        assert np.array_equal(a32, a)
        assert np.array_equal(s32.astype(np.float64), s) and np.array_equal(e32.astype(np.float64), e)
    if case.dup:
        assert c[-1] == 0                               # the copy of centroid 0 loses every tie


@pytest.mark.parametrize("case", KR.GRID_TABLE, ids=repr)
def test_grid_cases_have_ties_and_no_empty_cluster(case):
    X, C = case.data()
    _, _, c, _ = KR.lloyd(X, C)
    assert (c[: case.k_live] > 0).all()
    if case.k_live >= 2:
        assert len(KR.tied_rows(X, C, case.k_live)) >= 1       # a tie between two distinct centroids
    elif case.dup:
        assert len(KR.tied_rows(X, C)) == case.n               # k = 2: every row ties with the copy


@pytest.mark.parametrize("route,d,k,flags", KR.ROUNDED, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_reference_stays_within_the_flip_cap(route, d, k, flags):
    """An fp32 evaluation of the rounded-class shapes disagrees with float64
    on at most 0.1 % of the rows, each within flip_bound; so does one whose
    distances are pushed to the edge of the bound, and one pushed past it is
    not justified."""
    X, C = KR.rounded_case(d, k, KR.ROUNDED_ROWS, seed=100 + d + k)
    n = KR.ROUNDED_ROWS
    assert np.isnan(X).any()
    a, _, c, _ = KR.lloyd(X, C)
    assert c[-1] == 0
    dist, a32, _, _ = _fp32_pass(X, C, np.arange(d), np.arange(n))
    D64, B = KR.distances(X, C), KR.flip_bound(X, C)
    assert (np.abs(dist.astype(np.float64) - D64) <= B).all()
    rows, ok = KR.flips(X, C, a32)
    assert len(rows) <= n // 1000 and ok.all()
    # the worst evaluation the bound admits: every distance but the best one lowered by B
    sign = np.where(np.arange(k)[:, None] == a[None, :], 1.0, -1.0)
    worst = np.argmin(D64 + sign * B, axis=0)
    rows, ok = KR.flips(X, C, worst)
    assert ok.all()
    # an outright misassignment (the runner-up by far more than the bound) is not justified
    second = np.argsort(D64, axis=0)[1]
    rows, ok = KR.flips(X, C, second)
    assert len(rows) == n and ok.mean() < 0.01
