"""np.longdouble oracle of the GLRM losses, their derivatives, both sampled gradients and
the objective, with the entrywise error bounds the tests assert (derivation: the
docstring of tests/test_glrm_loss_gpu.py)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
Q, ABS, HUB, POI, HIN, LOG, PER = range(7)
# evaluation constant C of every loss: 2 for the algebraic ones; for Poisson, Logistic and
# Periodic the next power of two above twice the worst err / bound measured at C = 1 on the
# device (0.252, 0.113, 0.666: docs/ROADMAP.md, round 23)
C_EVAL = {Q: 2, ABS: 2, HUB: 2, HIN: 2, POI: 1, LOG: 0.25, PER: 2}
MIXED = [j % 7 for j in range(37)]


def loss_ref(c, w, u, a):
    """L, dL/du, |L''| and the sum of the magnitudes of L's terms, of loss c."""
    x, s, one = u - a, 2 * a - 1, np.ones_like(u)
    if c == Q:
        return x * x, 2 * x, 2 * one, x * x
    if c == ABS:
        return np.abs(x), np.sign(x), 0 * one, np.abs(x)
    if c == HUB:
        L = np.where(np.abs(x) <= 1, x * x / 2, np.abs(x) - LD(0.5))
        return L, np.clip(x, -1, 1), one, L
    if c == POI:
        e, ca = np.exp(u), np.where(a > 0, a * np.log(np.where(a > 0, a, 1)) - a, 0)
        return e - a * u + ca, e - a, e, e + np.abs(a * u) + np.abs(ca)
    if c == HIN:
        t = 1 - s * u
        return np.maximum(t, 0), np.where(t > 0, -s, 0), 0 * one, np.maximum(t, 0)
    if c == LOG:
        L = np.log1p(np.exp(-s * u))
        return L, -s / (1 + np.exp(s * u)), one / 4, L
    return 1 - np.cos(w * x), w * np.sin(w * x), w * w * one, 1 + np.abs(np.cos(w * x))


def inputs(n, p, k, codes):
    """A [p][n] (zeros where missing), mask, X [k][n], Y [k][p] and the parameters [p]:
    30 % missing, row 0 all missing, row 1 all present, column p - 1 all missing."""
    rng = np.random.default_rng(1000 * n + 10 * p + k)
    A = rng.normal(size=(p, n))
    X = (rng.normal(size=(k, n)) / np.sqrt(k)).astype(np.float32)
    Y = rng.normal(size=(k, p)).astype(np.float32)
    mask = rng.random((p, n)) >= 0.3
    binary, counts = rng.random((p, n)) < 0.5, rng.poisson(2, (p, n))
    codes = np.asarray(codes)
    A[(codes == HIN) | (codes == LOG)] = binary[(codes == HIN) | (codes == LOG)]
    A[codes == POI] = counts[codes == POI]
    mask[:, 0] = False
    mask[:, 1] = True
    if p > 1:
        mask[p - 1] = False
    pars = np.where(codes == PER, 2 * np.pi / 3, 0.0)
    return np.where(mask, A, 0).astype(np.float32), mask, X, Y, pars


def grads_ref(A, mask, X, Y, codes, pars, C=C_EVAL):
    """gx [k][n], gy [k][p], obj, their bounds bx, by, bobj, and the smallest distance of an
    observed entry to a kink of its loss (Absolute: u = a, Hinge: s u = 1)."""
    Xl, Yl, Al = (t.astype(LD) for t in (X, Y, A))
    (k, n), p = X.shape, A.shape[0]
    U = Yl.T @ Xl
    du = (k + 2) * EPS * (np.abs(Yl).T @ np.abs(Xl))
    L, G, H, M = (np.zeros((p, n), LD) for _ in range(4))
    kink = np.inf
    for j in range(p):
        L[j], G[j], H[j], M[j] = loss_ref(codes[j], LD(pars[j]), U[j], Al[j])
        if codes[j] in (ABS, HIN) and mask[j].any():
            d = U[j] - Al[j] if codes[j] == ABS else 1 - (2 * Al[j] - 1) * U[j]
            kink = min(kink, float(np.abs(d[mask[j]]).min()))
    Cj = np.asarray([C[c] for c in codes], LD)[:, None]
    L, G, H, M = (np.where(mask, t, 0) for t in (L, G, H, M))
    dG = H * du + Cj * EPS * np.abs(G)
    dL = np.abs(G) * du + Cj * EPS * M
    return dict(gx=Yl @ G, gy=Xl @ G.T, obj=L.sum(), kink=kink,
                bx=np.abs(Yl) @ dG + (p + 2) * EPS * (np.abs(Yl) @ np.abs(G)),
                by=np.abs(Xl) @ dG.T + (n + 2) * EPS * (np.abs(Xl) @ np.abs(G).T),
                bobj=dL.sum() + (mask.sum() + 2) * EPS * np.abs(L).sum(),
                # first-order change of obj when every x moves by its fp32 rounding, 2^-24 |x|
                bstore=2.0 ** -24 * (np.abs(G) * (np.abs(Yl).T @ np.abs(Xl))).sum())
