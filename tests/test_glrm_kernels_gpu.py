"""ops.glrm (masked ALS kernels) against the np.longdouble oracle of glrm_ref, and
the public fit with missing entries on the kernel route against the CPU-frame fit.

Bounds.  Every term of the products is exact in fp64 (a product of two fp32
numbers, a 0 / 1 mask, a widened fp32), so an n-term sum in any order is within
(n + 2) 2^-52 sum |term| of the exact one.  x is stored as fp32 (2^-23 |x|)
after a Cholesky solve whose forward error is bounded by 64 k kappa_i 2^-52
max_a |x[a][i]|.  Measured figures: the Round 19 section of docs/ROADMAP.md."""
import numpy as np
import pandas as pd
import pytest
import torch

import glrm_ref as R
from h2omx.frame.frame import Frame
from h2omx.models import glrm as M
from h2omx.models.glrm import H2OGeneralizedLowRankEstimator
from h2omx.ops import glrm

pytestmark = pytest.mark.gpu
SHAPES = [(333, 5, 1), (333, 37, 3), (333, 37, 10), (130, 130, 16), (130, 70, 17), (70, 40, 32)]
LAM = 0.5 + 1e-8


def _inputs(n, p, k, factor_cols):
    """A [p][n] (zeros where missing), mask, and a standard-normal factor [k][factor_cols]."""
    rng = np.random.default_rng(1000 * n + 10 * p + k)
    A = rng.normal(size=(p, n)).astype(np.float32)
    F = rng.normal(size=(k, factor_cols)).astype(np.float32)
    mask = rng.random((p, n)) >= 0.3
    mask[:, 0] = False
    mask[:, 1] = True
    if p > 1:
        mask[p - 1] = False
    return np.where(mask, A, np.float32(0)), mask, F


@pytest.mark.parametrize("n,p,k,slab", [s + (None,) for s in SHAPES] + [(333, 37, 10, 128)])
def test_masked_y_terms(cuda_dev, n, p, k, slab):
    A, mask, X = _inputs(n, p, k, n)
    dev = [torch.from_numpy(t).to(cuda_dev) for t in (A, mask, X)]
    S = glrm.masked_y_terms(*dev, slab_rows=slab)
    ref, mag = R.y_terms_ref(A, mask, X)
    err = np.abs(S.cpu().numpy().astype(R.LD) - ref)
    print(f"y_terms {n} x {p}, k {k}: max err / bound {float((err / np.maximum((n + 2) * R.EPS * mag, 1e-300)).max()):.3g}")
    assert (err <= (n + 2) * R.EPS * mag).all()
    assert torch.equal(S[:, :, :k], S[:, :, :k].transpose(1, 2))
    assert not S[p - 1].any()
    assert torch.equal(S, glrm.masked_y_terms(*dev, slab_rows=slab))


@pytest.mark.parametrize("n,p,k", SHAPES)
def test_masked_x(cuda_dev, n, p, k):
    A, mask, Y = _inputs(n, p, k, p)
    dev = [torch.from_numpy(t).to(cuda_dev) for t in (A, mask, Y)]
    X, bad = glrm.masked_x(*dev, LAM)
    ref, kappa = R.x_ref(A, mask, Y, LAM)
    bound = 2.0 ** -23 * np.abs(ref) + 64 * k * kappa * R.EPS * np.abs(ref).max(0)
    err = np.abs(X.cpu().numpy().astype(np.float64) - ref)
    e_torch = np.abs(M._solve_x_torch(*(torch.from_numpy(t) for t in (A, mask, Y)), LAM).numpy() - ref).max()
    print(f"masked_x {n} x {p}, k {k}: kappa {kappa.max():.3g}, relative to max|x| kernel "
          f"{err.max() / np.abs(ref).max():.3g} torch {e_torch / np.abs(ref).max():.3g}, "
          f"max err / bound {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert bad == 0
    assert not X[:, 0].any()
    assert (err <= bound).all()
    X2, _ = glrm.masked_x(*dev, LAM)
    assert torch.equal(X, X2)


def test_refusals(cuda_dev):
    A, mask, Y = (torch.from_numpy(t) for t in _inputs(40, 34, 33, 34))
    with pytest.raises(ValueError, match="32"):
        glrm.masked_x(A.to(cuda_dev), mask.to(cuda_dev), Y.to(cuda_dev), LAM)
    with pytest.raises(ValueError, match="32"):
        glrm.masked_y_terms(A.to(cuda_dev), mask.to(cuda_dev), torch.zeros((33, 40), device=cuda_dev))
    with pytest.raises(ValueError, match="device"):
        glrm.masked_x(A, mask, Y[:3], LAM)
    with pytest.raises(ValueError, match="device"):
        glrm.masked_y_terms(A, mask, torch.zeros((3, 40)))


@pytest.mark.parametrize("nonneg", [False, True])
def test_public_fit(cuda_dev, nonneg):
    rng = np.random.default_rng(2)
    full = rng.normal(size=(1500, 3)) @ rng.normal(size=(3, 8)) + 0.01 * rng.normal(size=(1500, 8))
    full = (np.abs(full) if nonneg else full).astype(np.float32)
    miss = np.random.default_rng(9).random(full.shape) < 0.15
    df = pd.DataFrame(full, columns=[f"c{i}" for i in range(8)]).mask(miss)
    kw = dict(regularization_x="NonNegative", regularization_y="NonNegative") if nonneg else {}
    fits = []
    for dev in ("cpu", "cuda"):
        fr = Frame.from_pandas(df, device=dev)
        m = H2OGeneralizedLowRankEstimator(k=3, init="SVD", max_iterations=40, min_step_size=0, **kw).train(
            training_frame=fr)
        fits.append((m, m.predict(fr).to_pandas().to_numpy()))
    (mc, _), (mg, Rg) = fits
    assert mc.timings["als_engine"] == "torch" and mg.timings["als_engine"] == "hip"
    print(f"public fit nonneg={nonneg}: objective cpu {mc.objective:.6g} device {mg.objective:.6g}")
    np.testing.assert_allclose(mg.objective, mc.objective, rtol=1e-3)
    if nonneg:
        assert (mg.Y >= 0).all() and float(mg.representation.to_pandas().to_numpy().min()) >= 0
    else:
        assert np.abs(Rg[miss] - full[miss]).mean() < 0.1 * np.abs(full).mean()
