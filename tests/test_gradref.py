"""CPU tests of the gradient-pass reference (tests/gradref.py): its exact
class against the float64 ``h2omx.reference.tree.dist_grad`` where rounding
that to float32 is well defined, and its tolerance against an fp32 emulation
of the kernels whose exp result is pushed a full ulp either way."""
import numpy as np
import pytest

import gradref as GR
from h2omx.reference.tree import dist_grad

PARAMS = dict(tweedie_power=1.2, quantile_alpha=0.3, huber_delta=0.8)


def _eighths(rng, n, lim):
    """multiples of 1/8 below ``lim``: their differences are exact in float32 and float64 alike"""
    return (rng.integers(-8 * lim, 8 * lim + 1, n) / 8.0).astype(np.float32)


@pytest.mark.parametrize("dist", GR.EXACT)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_exact_class_matches_float64_reference(dist, weighted):
    rng = np.random.default_rng(11)
    n = 5000
    f, y = _eighths(rng, n, 40), _eighths(rng, n, 40)
    y[:500] = f[:500]                                   # f == y: laplace 0, quantile 1 - alpha, huber / gaussian 0
    f[500:520], y[500:520] = -0.0, 0.0
    wobs = rng.uniform(0.5, 2.0, n).astype(np.float32) if weighted else None
    p32 = {k: float(v) for k, v in GR.params32(PARAMS).items()}
    ref = GR.grad_pass(f, y, wobs, dist, PARAMS, sample_rate=0.632, seed=0x80000003, tree_index=70001,
                       row_base=2 ** 32 - 700)
    assert ref.exact and 0.2 < (ref.w == 0).mean() < 0.6
    g64, h64 = dist_grad(dist, f, y, **p32)
    # the unweighted float64 values are exact here (1 - alpha: one rounding), the weighting is one fp32 product
    assert np.array_equal(g64.astype(np.float32) * ref.w, ref.g)
    assert np.array_equal(h64.astype(np.float32) * ref.w, ref.h)
    if dist == "laplace":
        assert (ref.g[:500] == 0).all()
    if dist == "quantile":
        live = ref.w[:500] != 0
        assert np.array_equal(ref.g[:500][live], ((np.float32(1) - np.float32(0.3)) * ref.w[:500])[live])
    if dist == "huber":
        # |f - y| == delta takes the linear branch, the next float32 the clipped one
        d = np.float32(0.8)
        g, _ = GR.exact_gh("huber", np.array([d, np.nextafter(d, np.float32(2)), -d], np.float32),
                           np.zeros(3, np.float32), PARAMS)
        assert g.tolist() == [d, d, -d]
    # the reference reads its parameters as float32: float64 0.3 and float32 0.3 give the same gradients
    again = GR.grad_pass(f, y, wobs, dist, {k: np.float32(v) for k, v in PARAMS.items()}, 0.632, 0x80000003, 70001,
                         2 ** 32 - 700)
    assert again.g.tobytes() == ref.g.tobytes()


def _inputs(dist, rng, n):
    lim = 30.0 if dist == "bernoulli" else 10.0
    f = rng.uniform(-lim, lim, n).astype(np.float32)
    if dist == "bernoulli":
        y = (rng.random(n) < 0.5).astype(np.float32)
    elif dist == "poisson":
        y = rng.poisson(np.exp(np.clip(f, -3, 3))).astype(np.float32)
    else:
        y = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)
        if dist == "tweedie":
            y[rng.random(n) < 0.3] = 0.0
    return f, y


@pytest.mark.parametrize("dist,rho", [("bernoulli", None), ("poisson", None), ("gamma", None), ("tweedie", 1.2),
                                      ("tweedie", 1.5), ("tweedie", 1.9)])
def test_tolerance_holds_for_fp32_emulation(dist, rho):
    """every fp32 step of dist_grad rounded, the exp2 result one ulp off in
    either direction: the error stays inside tol (observed worst err / tol:
    bernoulli 0.28, poisson 0.27, gamma 0.28, tweedie 0.37 / 0.30 / 0.38 at
    power 1.2 / 1.5 / 1.9; softmax below, 0.44)"""
    rng = np.random.default_rng(17)
    n = 400_000
    f, y = _inputs(dist, rng, n)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    params = {"tweedie_power": rho} if rho else None
    ref = GR.grad_pass(f, y, w, dist, params)
    assert not ref.exact
    worst = 0.0
    for push in (-1, 0, 1):
        g, h = GR.emulate_gh(dist, f, y, w, params, push)
        worst = max(worst, ref.compare(g, h, w, f"{dist} push {push}"))
    print(f"{dist} rho {rho}: worst err / tol {worst:.3f}")
    assert 0.0 < worst <= 1.0
    # the bound is not slack by orders of magnitude: a relative error of 2^-14 is caught
    g, h = GR.emulate_gh(dist, f, y, w, params, 0)
    with pytest.raises(AssertionError, match="beyond tol"):
        ref.compare(g * np.float32(1 + 2.0 ** -14), h, None, "scaled g")
    with pytest.raises(AssertionError, match="beyond tol"):
        ref.compare(g, h * np.float32(1 + 2.0 ** -14), None, "scaled h")


@pytest.mark.parametrize("K", [2, 3, 7])
def test_softmax_tolerance_holds_for_fp32_emulation(K):
    rng = np.random.default_rng(19)
    n = 100_000
    Fm = rng.uniform(-40, 40, (K, n)).astype(np.float32)
    Fm[:, : n // 2] *= 0.05                                # half the rows with comparable classes
    yk = rng.integers(0, K, n)
    w = rng.uniform(0.5, 2.0, n).astype(np.float32)
    worst = 0.0
    for cls in range(K):
        ref = GR.softmax_pass(Fm, yk, w, cls)
        for push in (-1, 0, 1):
            g, h = GR.emulate_softmax(Fm, yk, w, cls, push)
            worst = max(worst, ref.compare(g, h, w, f"K {K} class {cls} push {push}"))
        assert (ref.h == float(GR.H_FLOOR) * w.astype(np.float64)).any(), "no row at the h floor"
    print(f"softmax K {K}: worst err / tol {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_bernoulli_saturates_exactly():
    f = np.array([100, 100, -100, -100], np.float32)
    y = np.array([0, 1, 0, 1], np.float32)
    w = np.array([1.5, 0.75, 1.25, 2.0], np.float32)
    ref = GR.grad_pass(f, y, w, "bernoulli")
    g, h = GR.emulate_gh("bernoulli", f, y, w)
    assert np.array_equal(g, np.array([1, 0, 0, -1], np.float32) * w) and np.array_equal(h, GR.H_FLOOR * w)
    assert np.array_equal(ref.g, g.astype(np.float64))
    ref.compare(g, h, w)
