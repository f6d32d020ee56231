"""NumPy reference of the tree gradient pass (dist_grad, boost_update_kernel,
softmax_grad_kernel of ``csrc/tree_kernels.hip``): the (g, h, w) a tree is
built from, given the margins, the response, observation weights and the bag.

Two classes of distribution:

* exact (gaussian, laplace, quantile, huber, drf): no transcendental, so the
  reference evaluates in ``np.float32`` in the kernel's operation order and the
  GPU result must equal it bit for bit.  ``quantile_alpha`` / ``huber_delta``
  are rounded to float32 first, as ``GradParams`` stores them; ``g * w`` and
  ``h * w`` are one rounding each.
* toleranced (bernoulli, poisson, gamma, tweedie, softmax): float64 values of
  the same expressions on the float32 inputs, with ``tol = C * M * w`` where
  ``C = (|a| + 4) * 2^-22`` (softmax: ``|a| + 4 + K``), ``a`` the largest
  exponent argument of the row and ``M`` the magnitude before cancellation:

      bernoulli   a = f                      g: p + y          h: 2 p
      poisson     a = f                      g: mu + |y|       h: mu
      gamma       a = -f, e = y exp(-f)      g: 1 + e          h: e
      tweedie     a = max(|(1-rho) f|, |(2-rho) f|), A = y exp((1-rho) f), B = exp((2-rho) f)
                                             g: A + B          h: |1-rho| A + (2-rho) B
      softmax     a = max_k (mx - F_k)       g: p_k + y        h: 2 p_k

  ``__expf(a)`` is a hardware exp2 (1 ulp) of ``a * log2(e)`` rounded to fp32:
  relative error about ``(|a| + 1.5) * 2^-23``; every later operation adds
  ``2^-24`` of an operand; ``C`` is twice that.  The h floor ``1e-16f`` applies
  on both sides, and it is an operand of the last multiplication (by ``w``)
  like any other h, so M of h is never below it.

  bernoulli beyond |f| = 89 saturates in fp32 (exp overflows to inf, or
  vanishes against 1): p is exactly 0 or 1 there and so is the reference.

Plain NumPy; no HIP code is called from here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from h2omx.reference.tree import bag_weights

EXACT = ("gaussian", "laplace", "quantile", "huber", "drf")
TOLERANCED = ("bernoulli", "poisson", "gamma", "tweedie")
DISTS = ("gaussian", "bernoulli", "poisson", "gamma", "tweedie", "laplace", "quantile", "huber", "drf")
H_FLOOR = np.float32(1e-16)
BERNOULLI_SATURATED = 89.0
_EPS = 2.0 ** -22


def params32(params: dict | None) -> dict:
    """tweedie_power, quantile_alpha, huber_delta as GradParams stores them (float32; the defaults of make_grad_params)"""
    p = dict(tweedie_power=1.5, quantile_alpha=0.5, huber_delta=1.0)
    p.update(params or {})
    return {k: np.float32(v) for k, v in p.items()}


def row_weights(n: int, wobs, sample_rate: float, seed: int, tree_index: int, row_base: int = 0):
    """observation weight x bag weight per row (float32; exact: the bag weight is 0 or 1)"""
    w = np.ones(n, np.float32) if wobs is None else np.asarray(wobs, np.float32)
    return w * bag_weights(n, sample_rate, seed, tree_index, row_base)


def exact_gh(dist: str, f, y, params=None):
    """(g, h) of the exact class before weighting, float32 in the kernel's operation order"""
    f, y = np.asarray(f, np.float32), np.asarray(y, np.float32)
    p = params32(params)
    one = np.float32(1.0)
    if dist == "gaussian":
        g = f - y
    elif dist == "laplace":
        g = np.where(f > y, one, np.where(f < y, -one, np.float32(0.0)))
    elif dist == "quantile":
        a = p["quantile_alpha"]
        g = np.where(y > f, -a, one - a)
    elif dist == "huber":
        d = p["huber_delta"]
        r = f - y
        g = np.where(np.abs(r) <= d, r, np.copysign(d, r))
    elif dist == "drf":
        g = -y
    else:
        raise ValueError(dist)
    g = g.astype(np.float32)
    return g, np.ones_like(g)


def float_gh(dist: str, f, y, params=None):
    """(g, h, a, Mg, Mh) of the toleranced class before weighting, float64 on the float32 inputs"""
    f = np.asarray(f, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    floor = float(H_FLOOR)
    with np.errstate(over="ignore", under="ignore"):
        if dist == "bernoulli":
            pr = 1.0 / (1.0 + np.exp(-f))
            pr = np.where(f >= BERNOULLI_SATURATED, 1.0, np.where(f <= -BERNOULLI_SATURATED, 0.0, pr))
            g, h, a, mg, mh = pr - y, pr * (1.0 - pr), f, pr + y, 2.0 * pr
        elif dist == "poisson":
            mu = np.exp(f)
            g, h, a, mg, mh = mu - y, mu, f, mu + np.abs(y), mu
        elif dist == "gamma":
            e = y * np.exp(-f)
            g, h, a, mg, mh = 1.0 - e, e, -f, 1.0 + np.abs(e), np.abs(e)
        elif dist == "tweedie":
            rho = float(params32(params)["tweedie_power"])
            A, B = y * np.exp((1.0 - rho) * f), np.exp((2.0 - rho) * f)
            g, h = -A + B, -(1.0 - rho) * A + (2.0 - rho) * B
            a = np.maximum(np.abs((1.0 - rho) * f), np.abs((2.0 - rho) * f))
            mg, mh = np.abs(A) + B, abs(1.0 - rho) * np.abs(A) + (2.0 - rho) * B
        else:
            raise ValueError(dist)
    return g, np.maximum(h, floor), np.abs(a), mg, np.maximum(mh, floor)


@dataclass
class GradRef:
    exact: bool
    g: np.ndarray          # float32 (exact) / float64 (toleranced), weighted
    h: np.ndarray
    w: np.ndarray          # float32, observation weight x bag weight
    tol_g: np.ndarray | None = None
    tol_h: np.ndarray | None = None

    def compare(self, g, h, w=None, what: str = "") -> float:
        """Assert (g, h[, w]) of a kernel against the reference: bit for bit
        (exact class, and w always) or within tol.  Returns the worst err / tol
        over g and h (0 for the exact class)."""
        g, h = np.asarray(g, np.float32), np.asarray(h, np.float32)
        if w is not None:
            bad = np.asarray(w, np.float32).view(np.int32) != self.w.view(np.int32)
            assert not bad.any(), f"{what}: w differs at rows {np.nonzero(bad)[0][:8]}"
        if self.exact:
            for name, got, ref in (("g", g, self.g), ("h", h, self.h)):
                bad = got.view(np.int32) != ref.view(np.int32)
                assert not bad.any(), (f"{what}: {name} differs at rows {np.nonzero(bad)[0][:8]}: "
                                       f"{got[bad][:8]} != {ref[bad][:8]}")
            return 0.0
        worst = 0.0
        for name, got, ref, tol in (("g", g, self.g, self.tol_g), ("h", h, self.h, self.tol_h)):
            err = np.abs(got.astype(np.float64) - ref)
            bad = ~(err <= tol)
            assert not bad.any(), (f"{what}: {name} beyond tol at rows {np.nonzero(bad)[0][:8]}: got {got[bad][:8]}, "
                                   f"want {ref[bad][:8]}, err / tol {(err[bad] / tol[bad])[:8]}")
            live = tol > 0
            if live.any():
                worst = max(worst, float((err[live] / tol[live]).max()))
        return worst


def grad_pass(F, y, wobs, dist: str, params=None, sample_rate: float = 1.0, seed: int = 0, tree_index: int = 0,
              row_base: int = 0) -> GradRef:
    """Reference (g, h, w) of boost_update_kernel for rows 0 .. n - 1 (F: the margins dist_grad sees)"""
    n = len(F)
    w = row_weights(n, wobs, sample_rate, seed, tree_index, row_base)
    if dist in EXACT:
        g, h = exact_gh(dist, F, y, params)
        return GradRef(True, g * w, h * w, w)
    g, h, a, mg, mh = float_gh(dist, F, y, params)
    w64 = w.astype(np.float64)
    c = (a + 4.0) * _EPS
    return GradRef(False, g * w64, h * w64, w, c * mg * w64, c * mh * w64)


def softmax_pass(Fm, yk, wobs, cls: int, sample_rate: float = 1.0, seed: int = 0, tree_index: int = 0,
                 row_base: int = 0) -> GradRef:
    """Reference (g, h, w) of softmax_grad_kernel for class ``cls``; Fm [K][n] margins, yk class index per row"""
    Fm = np.asarray(Fm, np.float32).astype(np.float64)
    K, n = Fm.shape
    w = row_weights(n, wobs, sample_rate, seed, tree_index, row_base)
    mx = Fm.max(axis=0)
    with np.errstate(under="ignore"):
        z = np.exp(Fm - mx)
    pk = z[cls] / z.sum(axis=0)
    yv = (np.asarray(yk) == cls).astype(np.float64)
    floor = float(H_FLOOR)
    a = (mx - Fm).max(axis=0)
    c = (a + 4.0 + K) * _EPS
    w64 = w.astype(np.float64)
    g, h = pk - yv, np.maximum(pk * (1.0 - pk), floor)
    return GradRef(False, g * w64, h * w64, w, c * (pk + yv) * w64, c * np.maximum(2.0 * pk, floor) * w64)


# ---------------------------------------------------------------------------
# fp32 emulation of the toleranced kernels (CPU test of the bound itself)
# ---------------------------------------------------------------------------
def expf_emulated(a, push: int):
    """__expf in fp32: exp2 of the fp32 product a * log2(e), rounded to fp32 and
    pushed ``push`` ulps (the hardware exp2 is good to 1 ulp)"""
    a = np.asarray(a, np.float32)
    t = (a * np.float32(1.4426950408889634)).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(t.astype(np.float64)).astype(np.float32)
    for _ in range(abs(push)):
        e = np.nextafter(e, np.float32(np.inf if push > 0 else 0.0), dtype=np.float32)
    return e


def emulate_gh(dist: str, f, y, w, params=None, push: int = 0):
    """(g, h) weighted, every step of dist_grad + the weighting rounded to fp32"""
    f, y, w = (np.asarray(v, np.float32) for v in (f, y, w))
    one = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        if dist == "bernoulli":
            pr = one / (one + expf_emulated(-f, push))
            g, h = pr - y, pr * (one - pr)
        elif dist == "poisson":
            mu = expf_emulated(f, push)
            g, h = mu - y, mu
        elif dist == "gamma":
            e = y * expf_emulated(-f, push)
            g, h = one - e, e
        elif dist == "tweedie":
            rho = params32(params)["tweedie_power"]
            A = y * expf_emulated((one - rho) * f, push)
            B = expf_emulated((np.float32(2.0) - rho) * f, -push)
            g = -A + B
            h = (-(one - rho) * A).astype(np.float32) + ((np.float32(2.0) - rho) * B).astype(np.float32)
        else:
            raise ValueError(dist)
    h = np.maximum(h.astype(np.float32), H_FLOOR)
    return (g.astype(np.float32) * w).astype(np.float32), (h * w).astype(np.float32)


def emulate_softmax(Fm, yk, w, cls: int, push: int = 0):
    Fm = np.asarray(Fm, np.float32)
    w = np.asarray(w, np.float32)
    one = np.float32(1.0)
    mx = Fm.max(axis=0)
    den = np.zeros(Fm.shape[1], np.float32)
    fk = None
    for k in range(Fm.shape[0]):
        e = expf_emulated(Fm[k] - mx, push if k == cls else -push)
        den = (den + e).astype(np.float32)
        if k == cls:
            fk = e
    pk = (fk / den).astype(np.float32)
    yv = (np.asarray(yk) == cls).astype(np.float32)
    h = np.maximum((pk * (one - pk)).astype(np.float32), H_FLOOR)
    return ((pk - yv) * w).astype(np.float32), (h * w).astype(np.float32)
