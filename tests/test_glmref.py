"""CPU self-test of the GLM oracle (tests/glmref.py): runs anywhere.

* the oracle is internally consistent: its gradient is the central finite
  difference of deviance / 2, and the IRLS Gram and the gradient satisfy
  G[:p+1, p+1] - G[:p+1, :p+1] beta = -g on all 17 family x link combinations;
* it agrees entry-wise with the NumPy mirror ``h2omx.reference.dense`` where no
  floor is active (the current contract is the textbook there);
* the split-piece design has teeth: a float32 model of the kernel's bf16 split
  reproduces the designated entries exactly, and loses at least one of them
  when any one of the six kept products is dropped;
* the exact designs satisfy the precondition under which fp32 accumulation in
  any order is exact.
"""
import numpy as np
import pytest
import torch

import glmref as R
from h2omx.reference import dense as M

IDS = [R.combo_id(c) for c in R.COMBOS]


def _kw(c):
    return dict(var_power=c[2], link_power=c[3])


@pytest.mark.parametrize("combo", R.COMBOS, ids=IDS)
def test_gradient_is_finite_difference_of_half_deviance(combo):
    f, l, vp, lp = combo
    X, y, w, off, beta = R.dense_design(11, combo, 5, 200)
    r = R.irls(X, y, w, off, beta, f, l, **_kw(combo))
    R.check_unclamped(f, l, r.eta, r.mu, y, lp)
    g = R.grad(X, y, w, off, beta, f, l, **_kw(combo))
    h = 2.0 ** -17
    fd = np.zeros(6)
    for j in range(6):
        bp, bm = beta.copy(), beta.copy()
        bp[0, j] += h
        bm[0, j] -= h
        fd[j] = (R.deviance_at(X, y, w, off, bp, f, l, vp, lp) - R.deviance_at(X, y, w, off, bm, f, l, vp, lp)) / (4 * h)
    # central difference: O(h^2) truncation + deviance rounding / h; prototype saw <= 8e-9 of absg
    assert (np.abs(fd - g.g[0]) <= 1e-7 * g.absg[0]).all(), np.abs(fd - g.g[0]) / g.absg[0]


@pytest.mark.parametrize("combo", R.COMBOS, ids=IDS)
@pytest.mark.parametrize("p", [5, 37])
def test_gram_and_gradient_identity(combo, p):
    """X W z - X W X^T beta = X W (y - mu) / mu' = -g: the two passes are tied."""
    f, l, vp, lp = combo
    X, y, w, off, beta = R.dense_design(12 + p, combo, p, 300)
    r = R.irls(X, y, w, off, beta, f, l, **_kw(combo))
    g = R.grad(X, y, w, off, beta, f, l, **_kw(combo))
    lhs = r.G[:p + 1, p + 1] - r.G[:p + 1, :p + 1] @ beta[0]
    bound = r.absG[:p + 1, p + 1] + r.absG[:p + 1, :p + 1] @ np.abs(beta[0]) + g.absg[0]
    assert (np.abs(lhs + g.g[0]) <= 1e-13 * bound).all()
    assert g.dev == pytest.approx(r.dev, rel=1e-14)


def test_multinomial_gradient_is_finite_difference():
    X, y, w, _, beta = R.multinomial_design(5, 4, 150, 3)
    g = R.grad(X, y, w, None, beta, "multinomial", "logit")
    h = 2.0 ** -17
    for k in range(3):
        for j in range(5):
            bp, bm = beta.copy(), beta.copy()
            bp[k, j] += h
            bm[k, j] -= h
            fd = (R.deviance_at(X, y, w, None, bp, "multinomial", "logit")
                  - R.deviance_at(X, y, w, None, bm, "multinomial", "logit")) / (4 * h)
            assert abs(fd - g.g[k, j]) <= 1e-7 * g.absg[k, j]


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float32))


@pytest.mark.parametrize("combo", R.COMBOS, ids=IDS)
def test_oracle_agrees_with_mirror_where_no_floor_is_active(combo):
    f, l, vp, lp = combo
    for X, y, w, off, beta in (R.dense_design(21, combo, 37, 300), R.diag_design(22, combo, 30)):
        r = R.irls(X, y, w, off, beta, f, l, **_kw(combo))
        R.check_unclamped(f, l, r.eta, r.mu, y, lp)
        Gm, dm = M.glm_irls_pass(_t(X), _t(y), _t(w), _t(off), beta, f, l, **_kw(combo))
        assert (np.abs(Gm - r.G) <= 1e-13 * r.absG).all(), (np.abs(Gm - r.G) / np.maximum(r.absG, 1e-300)).max()
        assert abs(dm - r.dev) <= 1e-13 * r.absdev
        g = R.grad(X, y, w, off, beta, f, l, **_kw(combo))
        gm, dgm = M.glm_grad_pass(_t(X), _t(y), _t(w), _t(off), beta, f, l, **_kw(combo))
        assert (np.abs(gm - g.g) <= 1e-13 * g.absg).all()
        assert abs(dgm - g.dev) <= 1e-13 * g.absdev


@pytest.mark.parametrize("K", [2, 3, 16])
def test_oracle_agrees_with_mirror_multinomial(K):
    X, y, w, _, beta = R.multinomial_design(23 + K, 9, 200, K)
    for cls in range(K):
        r = R.irls(X, y, w, None, beta, "multinomial", "logit", cls=cls)
        R.check_unclamped("multinomial", "logit", r.eta, r.mu, y)
        Gm, dm = M.glm_irls_pass(_t(X), _t(y), _t(w), None, beta, "multinomial", "logit", cls=cls)
        assert (np.abs(Gm - r.G) <= 1e-13 * r.absG).all()
        assert abs(dm - r.dev) <= 1e-13 * r.absdev
    g = R.grad(X, y, w, None, beta, "multinomial", "logit")
    gm, dgm = M.glm_grad_pass(_t(X), _t(y), _t(w), None, beta, "multinomial", "logit")
    assert (np.abs(gm - g.g) <= 1e-13 * g.absg).all() and abs(dgm - g.dev) <= 1e-13 * g.absdev


def test_stable_binomial_deviance_of_saturated_rows():
    """log(1 - mu) from a rounded mu loses the deviance of a confidently wrong
    row (60.002 instead of 60 at eta = 30, y = 0); the oracle and the mirror
    take the logs from eta."""
    eta = np.array([20.0, 25.0, 30.0, 33.0, -30.0])
    y = np.array([0.0, 0.0, 0.0, 0.0, 1.0])
    X = np.ones((1, 5))
    for fam in R.BINOMIAL:
        for i in range(5):
            beta = np.array([[0.0, eta[i]]])
            r = R.irls(X[:, :1], y[i:i + 1], None, None, beta, fam, "logit", floors=True)
            exact = 2.0 * (abs(eta[i]) + np.log1p(np.exp(-abs(eta[i]))))
            assert r.dev == pytest.approx(exact, rel=1e-15)
            _, dm = M.glm_irls_pass(_t(X[:, :1]), _t(y[i:i + 1]), None, None, beta, fam, "logit")
            _, dg = M.glm_grad_pass(_t(X[:, :1]), _t(y[i:i + 1]), None, None, beta, fam, "logit")
            assert dm == pytest.approx(exact, rel=1e-14) and dg == pytest.approx(exact, rel=1e-14)


# ---------------------------------------------------------------------------
# the split-piece design
# ---------------------------------------------------------------------------
def test_split3_is_exact_and_pieces_are_bf16():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(size=1000) * 10.0 ** rng.integers(-6, 7, 1000), [0.0, 1.0, 16777215.0]]).astype(
        np.float32)
    hi, mid, lo = R.split3(x)
    assert (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) == x.astype(np.float64)).all()
    for pc in (hi, mid, lo):
        assert (pc.view(np.uint32) & np.uint32(0xFFFF) == 0).all()


@pytest.mark.parametrize("place", list(R.PIECE_PLACEMENTS))
def test_piece_design_has_teeth(place):
    p, cols = R.PIECE_PLACEMENTS[place]
    X, y, w, beta, pairs = R.piece_design(31, p, cols)
    r = R.irls(X, y, w, None, beta, "gaussian", "identity")
    A = (np.vstack([X, np.ones((1, X.shape[1])), r.z[None, :]]) * np.sqrt(r.W)[None, :]).astype(np.float32)
    ii, jj = np.array(pairs).T
    full = R.gram_split(A).astype(np.float64)
    assert (r.G[ii, jj] != 0).all() and (np.abs(r.G[ii, jj]) < 2.0 ** 48).all()
    assert (full[ii, jj] == r.G[ii, jj]).all()
    for k in range(6):
        dropped = R.gram_split(A, drop=k).astype(np.float64)
        assert (dropped[ii, jj] != r.G[ii, jj]).any(), f"dropping product {R.KEPT[k]} goes unnoticed"


# ---------------------------------------------------------------------------
# the exact designs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("setting", R.EXACT_SETTINGS)
@pytest.mark.parametrize("p,n", [(1, 20), (30, 101), (126, 1000), (126, 4093), (254, 4097), (255, 4097)])
def test_exact_designs_satisfy_their_precondition(setting, p, n):
    X, y, w, off, beta, f, l, quantum = R.exact_design(41, setting, p, n)
    r = R.irls(X, y, w, off, beta, f, l)
    assert n * r.absG.max() / quantum < 2.0 ** 24
    A = np.vstack([X, np.ones((1, n)), r.z[None, :]]) * np.sqrt(r.W)[None, :]
    assert (A / np.sqrt(quantum) == np.round(A / np.sqrt(quantum))).all()       # every entry a multiple of the quantum's root
    assert (w > 0).sum() >= min(n // 2, 100)       # the thinning leaves live rows all over the range
