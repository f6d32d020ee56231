"""ops.anomaly.eif_mean_length (Extended Isolation Forest scoring on the walk kernels)
against the tree walk in np.longdouble on the model's stored fp32 arrays, and the
public fit through it.

The kernels take every product exactly and round only the additions of a projection
(at most p of them, in fp64), so they decide as the oracle does wherever
|proj - offs| > (p + 1) 2^-52 sum_k |x_k n_k|; the oracle asserts that for every
decision of every row.  The leaf values then add exactly, which leaves one fp64
division and one fp32 store: |ml - ref| <= (2^-24 + 2^-52) |ref|.  Largest error /
tolerance and smallest margin ratio measured on MI355X: Round 21 of docs/ROADMAP.md."""
import numpy as np
import pytest
import torch

from h2omx import _native
from h2omx.frame import Frame
from h2omx.models import H2OExtendedIsolationForestEstimator
from h2omx.models.isolation_forest import avg_path
from h2omx.ops import anomaly

pytestmark = pytest.mark.gpu
LD = np.longdouble
TOL = LD(2.0) ** -24 + LD(2.0) ** -52


def _oracle(m, X):
    """Mean path value, np.longdouble [n], of the rows of fp32 X [n][p] (NaN -> training mean)."""
    X = np.where(np.isnan(X), m.design.means.astype(np.float32)[None, :], X).astype(LD)
    (T, cap, p), n = m.normals.shape, X.shape[0]
    leaf = m.sizes >= 0
    hval = (np.floor(np.log2(np.arange(cap) + 1.0)).astype(np.float32)[None, :]
            + avg_path(np.maximum(m.sizes, 0)).astype(np.float32))
    total, ratio = np.zeros(n, LD), LD(np.inf)
    for t in range(T):
        node = np.zeros(n, np.int64)
        for _ in range(m.limit):
            inner = ~leaf[t][node]
            terms = X * m.normals[t][node].astype(LD)
            proj, offs, mass = terms.sum(1), m.offs[t][node].astype(LD), np.abs(terms).sum(1)
            assert (np.abs(proj - offs)[inner] > (p + 1) * LD(2.0) ** -52 * mass[inner]).all()
            if (inner & (mass > 0)).any():
                ratio = min(ratio, (np.abs(proj - offs) / np.where(mass > 0, mass, 1))[inner & (mass > 0)].min())
            node = np.where(inner, 2 * node + 1 + (proj > offs), node)
        assert leaf[t][node].all()
        total += hval[t][node].astype(LD)
    print(f"oracle n={n} p={p} T={T}: smallest margin ratio {float(ratio):.3g}")
    return total / T


# (n, p, extension_level, T, sample_size), NaN share of the scored entries, forced EIF_SPARSE_MAX_K, dense walk
@pytest.mark.parametrize("case,nan,max_k,dense", [
    ((1, 1, 0, 3, 2), 0.0, None, False),            # limit 1, cap 3, one row
    ((333, 1, 0, 5, 256), 0.0, None, False),        # ragged row block, K = 1
    ((333, 5, 0, 7, 256), 0.0, None, False),        # axis-parallel
    ((333, 5, 2, 7, 256), 0.0, None, False),        # K = 3 with padded nodes
    ((333, 5, 4, 7, 64), 0.0, None, False),         # K = p, limit 6
    ((130, 33, 32, 5, 256), 0.0, None, True),       # dense, U = 64, ragged unit
    ((67, 65, 3, 5, 300), 0.0, None, False),        # x from global memory, limit 9, cap 1023
    ((67, 130, 129, 3, 256), 0.0, None, True),      # dense, three values per lane
    ((333, 5, 2, 7, 256), 0.05, None, False),       # NaN -> training mean
    ((333, 5, 2, 7, 256), 0.0, 0, True),            # both walks forced onto one forest
    ((333, 5, 2, 7, 256), 0.0, 32, False)])
def test_mean_length(cuda_dev, monkeypatch, case, nan, max_k, dense):
    n, p, ext, T, ss = case
    rng = np.random.default_rng(1000 * n + p)
    data = rng.normal(size=(max(n, ss), p)).astype(np.float32)
    m = H2OExtendedIsolationForestEstimator(ntrees=T, sample_size=ss, extension_level=ext, seed=2).train(
        training_frame=Frame.from_numpy(data, names=[f"x{j}" for j in range(p)]))
    X = data[:n].copy()
    X[rng.random(X.shape) < nan] = np.nan
    ref = _oracle(m, X)
    if max_k is not None:
        monkeypatch.setattr(anomaly, "EIF_SPARSE_MAX_K", max_k)
    plan = anomaly.eif_pack(m.normals, m.offs, m.sizes, m.design.means, cuda_dev)
    assert anomaly.eif_dense(plan) == dense and plan.limit == m.limit
    Xraw = torch.from_numpy(np.ascontiguousarray(X.T)).to(cuda_dev)
    ml = anomaly.eif_mean_length(Xraw, plan)
    assert ml.dtype == torch.float32 and ml.shape == (n,)
    err = np.abs(ml.cpu().numpy().astype(LD) - ref) / (TOL * np.abs(ref))
    print(f"eif_mean_length {case} nan={nan} K={plan.K} dense={dense}: largest error / tolerance {float(err.max()):.3g}")
    assert (err <= 1).all()
    for slab in (None, 1, 3, 7):                    # exact sum over the trees: any split, any call, the same bits
        assert torch.equal(ml, anomaly.eif_mean_length(Xraw, plan, slab_trees=slab))


def test_public_fit_scores_on_kernel(cuda_dev):
    data = np.random.default_rng(0).normal(size=(1500, 5)).astype(np.float32)
    fr = Frame.from_numpy(data, names=list("abcde"), device=cuda_dev)
    m = H2OExtendedIsolationForestEstimator(ntrees=20, extension_level=2, seed=2).train(training_frame=fr)
    assert m.score_engine(fr) == "hip" and m.timings["score_engine"] == "hip"
    ml = m.predict(fr).to_pandas()["mean_length"].to_numpy()
    assert "eif" in " ".join(_native.loaded_libraries())
    ref = _oracle(m, data)
    err = np.abs(ml.astype(LD) - ref) / (TOL * np.abs(ref))
    print(f"public fit: largest error / tolerance {float(err.max()):.3g}")
    assert (err <= 1).all()
    cpu = fr.to("cpu")
    assert m.score_engine(cpu) == "torch"
    assert np.isfinite(m.predict(cpu).to_pandas()["mean_length"].to_numpy()).all()
