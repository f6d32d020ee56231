"""Independent float64 oracle for the GLM passes (IRLS Gram pass, gradient pass).

Plain NumPy, written from the textbook definitions of the exponential-family
GLM (McCullagh & Nelder): inverse link mu = g^-1(eta), its derivative, the
variance function V(mu) and the unit deviance d(y, mu).  It shares no code
with ``h2omx.reference.dense`` (the mirror of the HIP pass) or ``h2omx.ops``.

By default NOTHING is floored or clamped: the tests choose inputs on which the
kernel's floors are inactive (``check_unclamped``) and then expect the kernel
to agree with the textbook.  ``floors=True`` applies the documented floors of
the pass contract (docs/ALGORITHMS.md, "GLM pass contract") for the saturation
tests only.

Conventions of the pass that the oracle follows:

* the design is feature-major, X [p][n]; beta is [K][p + 1], coefficients then
  the intercept; the augmented matrix is A = [x | 1 | z] ([p + 2][n]);
* the binomial family (binomial, quasibinomial, fractionalbinomial) reports
  -2 (y log mu + (1 - y) log(1 - mu)), i.e. -2 log-likelihood without the
  saturated term (the two agree for y in {0, 1});
* a multinomial IRLS pass updates one class ``cls``: W = w p (1 - p),
  z = eta_cls + ([y = cls] - p) / (p (1 - p)), and its deviance is the sum of
  -2 w log p_cls over the rows of that class; offsets do not enter.

``split3`` / ``gram_split`` model the split kernel's three-way bf16 split in
NumPy float32 (CPU self-test of the piece design only).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

BINOMIAL = ("binomial", "quasibinomial", "fractionalbinomial")
FAMILIES = ("gaussian",) + BINOMIAL + ("poisson", "gamma", "tweedie", "negativebinomial", "multinomial")
LINKS = ("identity", "logit", "log", "inverse", "tweedie")
LOG_FLOOR = np.log(1e-15)

# (family, link, var_power, link_power): every non-multinomial combination the passes serve.
# var_power carries theta for negativebinomial.
COMBOS = [
    ("gaussian", "identity", 0.0, 0.0), ("gaussian", "log", 0.0, 0.0), ("gaussian", "inverse", 0.0, 0.0),
    ("binomial", "logit", 0.0, 0.0), ("quasibinomial", "logit", 0.0, 0.0), ("fractionalbinomial", "logit", 0.0, 0.0),
    ("poisson", "log", 0.0, 0.0), ("poisson", "identity", 0.0, 0.0),
    ("gamma", "inverse", 0.0, 0.0), ("gamma", "log", 0.0, 0.0), ("gamma", "identity", 0.0, 0.0),
    ("tweedie", "tweedie", 1.5, 0.0), ("tweedie", "tweedie", 1.2, 1.0), ("tweedie", "tweedie", 1.9, -0.5),
    ("tweedie", "tweedie", 1.5, 0.5),
    ("negativebinomial", "log", 0.5, 0.0), ("negativebinomial", "identity", 2.0, 0.0),
]


def combo_id(c) -> str:
    f, l, vp, lp = c
    if f == "tweedie":
        return f"tweedie-v{vp:g}-l{lp:g}"
    if f == "negativebinomial":
        return f"negbin-{l}-th{vp:g}"
    return f"{f}-{l}"


def _is_log(link, link_power):
    return link == "log" or (link == "tweedie" and link_power == 0.0)


def linkinv(eta, link, link_power=0.0, floors=False):
    """mu = g^-1(eta) and dmu/deta."""
    eta = np.asarray(eta, np.float64)
    if link == "identity":
        return eta.copy(), np.ones_like(eta)
    if link == "logit":
        e = np.exp(-np.abs(eta))
        mu = np.where(eta >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        if floors:
            return mu, np.maximum(mu * (1.0 - mu), 1e-10)
        return mu, e / ((1.0 + e) * (1.0 + e))
    if _is_log(link, link_power):
        if floors:
            mu = np.exp(np.minimum(eta, 700.0))
            return mu, np.maximum(mu, 1e-10)
        mu = np.exp(eta)
        return mu, mu.copy()
    if link == "inverse":
        e = np.where(np.abs(eta) < 1e-10, np.copysign(1e-10, eta), eta) if floors else eta
        return 1.0 / e, -1.0 / (e * e)
    if link == "tweedie":
        e = np.maximum(eta, 1e-10) if floors else eta
        mu = e ** (1.0 / link_power)
        return mu, mu / (link_power * e)
    raise ValueError(link)


def variance(family, mu, var_power=1.5, floors=False):
    """V(mu)."""
    if family == "gaussian":
        return np.ones_like(mu)
    if family in BINOMIAL:
        v = mu * (1.0 - mu)
        return np.maximum(v, 1e-10) if floors else v
    if family == "poisson":
        return np.maximum(mu, 1e-10) if floors else mu.copy()
    if family == "gamma":
        return np.maximum(mu * mu, 1e-20) if floors else mu * mu
    if family == "tweedie":
        return np.maximum(np.maximum(mu, 1e-10) ** var_power, 1e-20) if floors else mu ** var_power
    if family == "negativebinomial":
        v = mu + var_power * mu * mu
        return np.maximum(v, 1e-10) if floors else v
    raise ValueError(family)


def _ylogy_over(y, m):
    """y log(y / m) with 0 log 0 = 0."""
    pos = y > 0
    return np.where(pos, y * np.log(np.where(pos, y, 1.0) / m), 0.0)


def unit_deviance(family, link, y, mu, eta, var_power=1.5, floors=False):
    """d(y, mu).  The binomial family under the logit link takes its logs from
    eta (log mu = min(eta, 0) - log1p(e), log(1 - mu) = -max(eta, 0) - log1p(e),
    e = exp(-|eta|)), never from a rounded mu."""
    if family == "gaussian":
        return (y - mu) ** 2
    if family in BINOMIAL:
        if link == "logit":
            l1p = np.log1p(np.exp(-np.abs(eta)))
            lm, l1m = np.minimum(eta, 0.0) - l1p, -np.maximum(eta, 0.0) - l1p
            if floors:
                lm, l1m = np.maximum(lm, LOG_FLOOR), np.maximum(l1m, LOG_FLOOR)
        else:
            m = np.clip(mu, 1e-15, 1.0 - 1e-15) if floors else mu
            lm, l1m = np.log(m), np.log1p(-m)
        return -2.0 * (y * lm + (1.0 - y) * l1m)
    m = np.maximum(mu, 1e-15) if floors else mu
    if family == "poisson":
        return 2.0 * (_ylogy_over(y, m) - (y - m))
    if family == "gamma":
        yy = np.maximum(y, 1e-15) if floors else y
        return 2.0 * (-np.log(yy / m) + (y - m) / m)
    if family == "tweedie":
        r = var_power
        a = np.where(y > 0, np.where(y > 0, y, 1.0) ** (2.0 - r) / ((1.0 - r) * (2.0 - r)), 0.0)
        return 2.0 * (a - y * m ** (1.0 - r) / (1.0 - r) + m ** (2.0 - r) / (2.0 - r))
    if family == "negativebinomial":
        th = var_power
        return 2.0 * (_ylogy_over(y, m) - (y + 1.0 / th) * np.log((1.0 + th * y) / (1.0 + th * m)))
    raise ValueError(family)


def _inputs(X, y, w, off, beta):
    X = np.asarray(X, np.float64)
    p, n = X.shape
    y = np.asarray(y, np.float64)
    w = np.ones(n) if w is None else np.asarray(w, np.float64)
    off = np.zeros(n) if off is None else np.asarray(off, np.float64)
    beta = np.atleast_2d(np.asarray(beta, np.float64))
    assert beta.shape[1] == p + 1 and y.shape == (n,) and w.shape == (n,) and off.shape == (n,)
    return X, y, w, off, beta, p, n


def softmax(beta, X, floors=False):
    """class probabilities [K][n] and their logs (log-sum-exp form)."""
    p = X.shape[0]
    eta = beta[:, :p] @ X + beta[:, p:p + 1]
    m = eta.max(axis=0, keepdims=True)
    lse = m + np.log(np.exp(eta - m).sum(axis=0, keepdims=True))
    logp = eta - lse
    return eta, np.exp(logp), logp


def _gram(A, W):
    """A W A^T and |A| W |A|^T, A [p + 2][n]."""
    AW = A * W[None, :]
    aA = np.abs(A)
    return AW @ A.T, (aA * np.abs(W)[None, :]) @ aA.T


def irls(X, y, w, off, beta, family, link, cls=0, var_power=1.5, link_power=0.0, floors=False):
    """One IRLS pass.  Returns a namespace with G, absG ([p + 2][p + 2]), dev,
    absdev, and the per-row W, z, eta, mu (multinomial: mu = p_cls)."""
    X, y, w, off, beta, p, n = _inputs(X, y, w, off, beta)
    if family == "multinomial":
        etas, pr, logp = softmax(beta, X)
        eta, pk, lpk = etas[cls], pr[cls], logp[cls]
        if floors:
            pk = np.clip(pk, 1e-10, 1.0 - 1e-10)
            lpk = np.log(pk)
        yk = (y.astype(np.int64) == cls).astype(np.float64)
        v = pk * (1.0 - pk)
        W = w * v
        z = eta + (yk - pk) / v
        d = np.where(yk > 0, -2.0 * lpk, 0.0)
        mu = pk
    else:
        eta = beta[0, :p] @ X + beta[0, p] + off
        mu, dmu = linkinv(eta, link, link_power, floors)
        W = w * dmu * dmu / variance(family, mu, var_power, floors)
        z = eta - off + (y - mu) / dmu
        d = unit_deviance(family, link, y, mu, eta, var_power, floors)
    A = np.vstack([X, np.ones((1, n)), z[None, :]])
    G, absG = _gram(A, W)
    return SimpleNamespace(G=G, absG=absG, dev=float((w * d).sum()), absdev=float((w * np.abs(d)).sum()),
                           W=W, z=z, eta=eta, mu=mu)


def grad(X, y, w, off, beta, family, link, var_power=1.5, link_power=0.0, floors=False):
    """Gradient pass: g [K][p + 1] = sum_i r_ki [x_i | 1] (= d(deviance / 2) /
    d beta), absg = sum_i |r_ki| |[x_i | 1]|, and the deviance."""
    X, y, w, off, beta, p, n = _inputs(X, y, w, off, beta)
    if family == "multinomial":
        K = beta.shape[0]
        etas, pr, logp = softmax(beta, X)
        yi = y.astype(np.int64)
        R = w[None, :] * (pr - (yi[None, :] == np.arange(K)[:, None]))
        d = -2.0 * logp[yi, np.arange(n)]
        eta, mu = etas, pr
    else:
        eta = beta[0, :p] @ X + beta[0, p] + off
        mu, dmu = linkinv(eta, link, link_power, floors)
        R = (w * (mu - y) * dmu / variance(family, mu, var_power, floors))[None, :]
        d = unit_deviance(family, link, y, mu, eta, var_power, floors)
    A1 = np.vstack([X, np.ones((1, n))])
    return SimpleNamespace(g=R @ A1.T, absg=np.abs(R) @ np.abs(A1).T, dev=float((w * d).sum()),
                           absdev=float((w * np.abs(d)).sum()), R=R, eta=eta, mu=mu)


def deviance_at(X, y, w, off, beta, family, link, var_power=1.5, link_power=0.0):
    return grad(X, y, w, off, beta, family, link, var_power, link_power).dev


def check_unclamped(family, link, eta, mu, y, link_power=0.0):
    """Assert the oracle's own values stay clear of every floor of the kernel,
    with a wide margin (1e-6 against floors of 1e-10 and below), so that the
    unfloored textbook formulas ARE the contract on these inputs."""
    eta, mu, y = np.asarray(eta), np.asarray(mu), np.asarray(y)
    assert np.isfinite(eta).all() and np.isfinite(mu).all()
    if family == "multinomial":
        assert (mu > 1e-6).all() and (mu < 1.0 - 1e-6).all(), "softmax probability near a floor"
        return
    if family in BINOMIAL or link == "logit":
        assert (mu * (1.0 - mu) > 1e-6).all(), "mu (1 - mu) near its floor"
    if family != "gaussian" or _is_log(link, link_power):
        assert (mu > 1e-6).all(), "mu near its floor"
    if link == "inverse":
        assert (np.abs(eta) > 1e-3).all(), "inverse link: eta near 0"
    if link == "tweedie" and link_power != 0.0:
        assert (eta > 1e-3).all(), "tweedie power link: eta near 0"
    if _is_log(link, link_power):
        assert (eta < 80.0).all(), "log link: eta beyond the fp32 range of the weights"
    if family == "gamma":
        assert (y > 0).all(), "gamma response must be positive"
    if family in ("poisson", "tweedie", "negativebinomial"):
        assert (y >= 0).all()


# ---------------------------------------------------------------------------
# NumPy float32 model of the split kernel's three-way bf16 split
# ---------------------------------------------------------------------------
def _trunc16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(x):
    """x (float32) = hi + mid + lo exactly; every piece is a bf16 value."""
    x = np.ascontiguousarray(x, np.float32)
    hi = _trunc16(x)
    r = (x - hi).astype(np.float32)
    mid = _trunc16(r)
    lo = (r - mid).astype(np.float32)
    return hi, mid, lo


# the six kept partial products in the kernel's issue order: (piece of a, piece of b), 0 = hi, 1 = mid, 2 = lo
KEPT = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))   # mm, lh, hl, mh, hm, hh


def gram_split(A, drop=None):
    """fp32 Gram of the already scaled augmented design A [cols][rows] (float32)
    from its bf16 pieces: six kept products per entry, each an MFMA that adds
    its (exact) bf16 x bf16 products into an fp32 accumulator.  ``drop`` omits
    kept product number ``drop`` (index into KEPT).  Upper triangle is
    meaningful: entry (i, j), i <= j, pairs a = column i with b = column j."""
    pieces = split3(np.ascontiguousarray(A, np.float32))
    acc = np.zeros((A.shape[0], A.shape[0]), np.float32)
    for k, (ia, ib) in enumerate(KEPT):
        if k == drop:
            continue
        acc = (acc.astype(np.float64) + pieces[ia].astype(np.float64) @ pieces[ib].astype(np.float64).T).astype(
            np.float32)
    return acc


# ---------------------------------------------------------------------------
# Test designs (shared by the CPU self-test and the GPU tests).  Every value is
# a small dyadic rational, exactly representable in fp32.
# ---------------------------------------------------------------------------
def eta_range(family, link, link_power=0.0):
    """(lo, hi) of the linear predictor on which no floor of the pass is near."""
    if link == "logit" or _is_log(link, link_power):
        return -6.0, 6.0
    if link == "identity" and family == "gaussian":
        return -6.0, 6.0
    if link == "inverse":
        return 0.25, 4.0
    return 0.25, 6.0          # identity on a positive mean, tweedie power links


def draw_response(rng, family, mu):
    """A response on the family's support, multiples of 1/4 (exact in fp32)."""
    n = mu.shape[0]
    if family == "gaussian":
        return np.round(2.0 * (mu + rng.normal(size=n))) / 2.0
    if family == "binomial":
        return (rng.random(n) < mu).astype(np.float64)
    if family in BINOMIAL:
        return rng.integers(0, 5, n) / 4.0
    if family in ("poisson", "negativebinomial"):
        return np.minimum(rng.poisson(np.minimum(mu, 50.0)), 60).astype(np.float64)
    g = np.ceil(4.0 * rng.gamma(2.0, np.minimum(mu, 50.0) / 2.0)) / 4.0
    if family == "gamma":
        return np.maximum(g, 0.25)
    return np.where(rng.random(n) < 0.3, 0.0, g)      # tweedie: a point mass at zero


def draw_conditioned_response(rng, family, link, link_power, eta, off):
    """draw_response, redrawing rows whose working response z = (eta - off) +
    (y - mu) / mu' cancels to less than 1/8 of its two terms: there the fp64
    rounding of the terms is amplified in z, and |z| (which every entry-wise
    bound here is relative to) says nothing about it."""
    mu, dmu = linkinv(eta, link, link_power)
    y = draw_response(rng, family, mu)
    for _ in range(50):
        a, b = eta - off, (y - mu) / dmu
        bad = np.abs(a + b) * 8.0 < np.abs(a) + np.abs(b)
        if not bad.any():
            break
        y = np.where(bad, draw_response(rng, family, mu), y)
    return y


def dense_design(seed, combo, p, n):
    """Moderate dense design of 3d: X multiples of 1/2 in [-2, 2], beta_j in
    {-1, 0, 1} 2^-s with s chosen so that |beta . x| <= 2, offsets multiples of
    1/4 in [-1/2, 1/2], prior weights in {0, 1/4, 1/2, 1, 2}; the intercept
    centres eta in the link's unclamped range."""
    family, link, vp, lp = combo
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, (p, n)) / 2.0
    s = int(np.ceil(np.log2(max(p, 1)))) if p else 0      # p 2^-s 2 <= 2
    beta = np.zeros((1, p + 1))
    beta[0, :p] = rng.choice([-1.0, 1.0, 1.0, 0.0], p) * 2.0 ** -s
    lo, hi = eta_range(family, link, lp)
    beta[0, p] = 0.25 if lo < 0 else 3.0
    off = rng.integers(-2, 3, n) / 4.0
    w = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0], n)
    eta = beta[0, :p] @ X + beta[0, p] + off
    y = draw_conditioned_response(rng, family, link, lp, eta, off)
    return X, y, w, off, beta


def multinomial_design(seed, p, n, K):
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, (p, n)) / 2.0
    s = int(np.ceil(np.log2(max(p, 1)))) if p else 0
    beta = np.zeros((K, p + 1))
    beta[:, :p] = rng.choice([-1.0, 1.0, 0.0], (K, p)) * 2.0 ** -s
    beta[:, p] = rng.integers(-4, 5, K) / 4.0
    y = rng.integers(0, K, n).astype(np.float64)
    w = rng.choice([0.0, 0.25, 0.5, 1.0, 2.0], n)
    return X, y, w, None, beta


def diag_design(seed, combo, p):
    """3c: n = p, X = diag(c) with c a signed power of two, eta spread over the
    link's unclamped range in steps of 1/32 (exact in fp32 through
    eta_j = beta_j c_j + b0 + off_j)."""
    family, link, vp, lp = combo
    rng = np.random.default_rng(seed)
    lo, hi = eta_range(family, link, lp)
    eta = np.round(32.0 * rng.permutation(np.linspace(lo, hi, p))) / 32.0
    if family == "gaussian" and link == "inverse":
        eta *= rng.choice([-1.0, 1.0], p)
    c = rng.choice([0.5, 1.0, 2.0], p) * rng.choice([-1.0, 1.0], p)
    off = rng.integers(-2, 3, p) / 4.0
    b0 = 0.25
    beta = np.zeros((1, p + 1))
    beta[0, :p] = (eta - b0 - off) / c
    beta[0, p] = b0
    w = rng.choice([0.25, 0.5, 1.0, 2.0], p)
    y = draw_conditioned_response(rng, family, link, lp, eta, off)
    return np.diag(c), y, w, off, beta


def diag_multinomial(seed, p, K):
    rng = np.random.default_rng(seed)
    c = rng.choice([0.5, 1.0, 2.0], p) * rng.choice([-1.0, 1.0], p)
    b0 = rng.integers(-2, 3, K) / 4.0
    eta = rng.integers(-16, 17, (K, p)) / 8.0            # [-2, 2] around the intercepts
    beta = np.zeros((K, p + 1))
    beta[:, :p] = eta / c[None, :]
    beta[:, p] = b0
    y = rng.integers(0, K, p).astype(np.float64)
    w = rng.choice([0.25, 0.5, 1.0, 2.0], p)
    return np.diag(c), y, w, None, beta


EXACT_SETTINGS = ("gaussian", "binomial", "poisson", "multinomial2")


def exact_design(seed, setting, p, n, use_w=True, use_off=True, zero_frac=None):
    """3a: dyadic inputs on which every quantity of the pass is exactly
    representable at every step.  n <= 128: X, y, offset multiples of 1/2 in
    [-2, 2], prior weights in {0, 1/4, 1, 4}; larger n: the value range shrinks
    to integers in [-1, 1] and weights in {0, 1}, and live rows are thinned
    (halving) until n max|G| < 2^24 quanta.  Returns (X, y, w, off, beta,
    family, link, quantum) with quantum the smallest product of two entries of
    sqrt(W) [x | 1 | z]."""
    rng = np.random.default_rng(seed)
    small = n <= 128
    draw = (lambda size: rng.integers(-4, 5, size) / 2.0) if small else (
        lambda size: rng.integers(-1, 2, size).astype(np.float64))
    X = draw((p, n))
    K = 2 if setting == "multinomial2" else 1
    beta = np.zeros((K, p + 1))
    off = None
    if setting == "gaussian":
        family, link = "gaussian", "identity"
        beta[0] = rng.integers(-4, 5, p + 1) / 4.0
        y = draw(n)
        off = draw(n) if use_off else None
        q = 0.25 if small else 1.0        # sqrt(w) x: multiples of 1/2 * 1/2, or integers
    elif setting == "poisson":
        family, link = "poisson", "log"
        y = rng.integers(0, 4, n).astype(np.float64)
        q = 0.25 if small else 1.0
    else:
        family, link = ("binomial", "logit") if setting == "binomial" else ("multinomial", "logit")
        y = rng.integers(0, 2, n).astype(np.float64)
        q = 0.125 if small else 0.5       # sqrt(W) = sqrt(w) / 2
    w = None
    if use_w:
        w = rng.choice([0.0, 0.25, 1.0, 4.0], n) if small else np.ones(n)
        live = 1.0 if small else 0.75
        if zero_frac is not None:
            live = 1.0 - zero_frac
        keep = rng.random(n)
        for _ in range(12):
            wt = np.where(keep < live, w, 0.0)
            r = irls(X, y, wt, off, beta, family, link)
            if n * r.absG.max() / (q * q) < 2.0 ** 24:
                break
            live *= 0.5
        w = wt
    return X, y, w, off, beta, family, link, q * q


def piece_design(seed, p, cols, n=64, live_row=37):
    """3b: one live row (weight 1, every other row weight 0 and filled with
    junk), gaussian at beta = 0, so the Gram is the outer product of that row
    of [x | 1 | y].  cols = the five column indices of [wide0, 2.0, wide1, m0,
    m1]: wide* odd 24-bit integers whose three bf16 pieces are all nonzero, m*
    odd 12-bit integers (hi and mid pieces).  Every designated entry is one
    product with at most 24 significant bits.  Returns (X, y, w, beta,
    designated index pairs (i <= j))."""
    rng = np.random.default_rng(seed)

    def wide():
        return float((1 << 23) | (int(rng.integers(1, 128)) << 16) | (int(rng.integers(1, 256)) << 8)
                     | (int(rng.integers(0, 128)) << 1) | 1)

    def narrow():
        return float((1 << 11) | (int(rng.integers(0, 512)) << 1) | 1)

    X = rng.integers(-1000, 1000, (p, n)).astype(np.float64)
    X[:, live_row] = 0.0
    i0, i2, i1, j0, j1 = cols
    X[i0, live_row], X[i2, live_row], X[i1, live_row] = wide(), 2.0, wide()
    X[j0, live_row], X[j1, live_row] = narrow(), narrow()
    y = rng.integers(-8, 9, n).astype(np.float64)
    y[live_row] = 1.0
    w = np.zeros(n)
    w[live_row] = 1.0
    pairs = [(i0, i2), (i0, p), (i2, i1), (i1, p), (j0, j1), (j0, p), (j1, p), (i2, p), (p, p), (i2, i2)]
    pairs = [(min(a, b), max(a, b)) for a, b in pairs]
    return X, y, w, np.zeros((1, p + 1)), pairs


# column placements of the five piece columns: p = 5 (one block), p = 40 at the
# start of block 0, at the end of the last data block, and spread over three
# blocks so that every designated pair sits in an off-diagonal tile
PIECE_PLACEMENTS = {
    "p5": (5, (0, 1, 2, 3, 4)),
    "p40-start": (40, (0, 1, 2, 3, 4)),
    "p40-end": (40, (35, 36, 37, 38, 39)),
    "p40-spread": (40, (0, 17, 36, 1, 37)),
}
