"""Interventional SHAP HIP kernels (csrc/explain_kernels.hip:
shap_bg_mask_kernel, tree_shap_bg_kernel, shap_slab_mean_kernel) vs the
float64 NumPy closed form on the same path table, in both output modes, on
every accumulator path and MAXM bucket; additivity on the device, run-to-run
determinism, and the unchanged path-dependent kernel."""
import numpy as np
import pytest
import torch

from h2omx import _native
from h2omx.explain import (_bucket, _shap_background_device, _shap_background_numpy, _shap_numpy,
                           predict_contributions, tree_paths)
from h2omx.frame import Frame
from h2omx.models import H2OGradientBoostingEstimator, H2ORandomForestEstimator, H2OXGBoostEstimator

pytestmark = pytest.mark.gpu

N_TRAIN, N_SCORE, N_BG, BG0 = 5000, 300, 37, 1001     # 300 rows: one full + one partial workgroup

CASES = {
    # name: (estimator, parameters, F, MAXM bucket, accumulators in LDS)
    "gbm_d5_f6": (H2OGradientBoostingEstimator, dict(ntrees=10, max_depth=5), 6, 8, True),
    "xgb_d8_f70": (H2OXGBoostEstimator, dict(ntrees=5, max_depth=8), 70, 8, False),      # 70*256*4 > 64 KB
    "drf_d12_f10": (H2ORandomForestEstimator, dict(ntrees=5, max_depth=12), 10, 16, True),
}


def _stack(fr, cols):
    return torch.stack([fr.vec(c).data for c in cols]).cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, cuda_dev):
    cls, kw, F, bucket, lds = CASES[request.param]
    rng = np.random.default_rng(F)
    X = rng.normal(size=(N_TRAIN, F)).astype(np.float32)
    X[::13, 0] = np.nan                                 # scored rows 0, 13, ...; background rows 1001, 1014, 1027
    y = (np.nan_to_num(X[:, 0]) + X[:, 1] * X[:, 2] + rng.normal(size=N_TRAIN) > 0).astype(np.float32)
    names = [f"f{i}" for i in range(F)]
    fr = Frame.from_numpy(np.c_[X, y], names=names + ["y"], device=cuda_dev)
    m = cls(seed=1, **kw).train(y="y", training_frame=fr)
    Xs, Xb = X[:N_SCORE], X[BG0: BG0 + N_BG]
    assert np.isnan(Xs[:, 0]).any() and np.isnan(Xb[:, 0]).any()
    nt = m.ens.ntrees
    lv, el, _, maxm, sets = tree_paths(m.ens.trees[:nt], 1.0 / nt if m.ens.average else 1.0)
    ref = _shap_background_numpy(Xs.T.astype(np.float64), Xb.T.astype(np.float64), lv, el, maxm, sets,
                                 per_reference=True)                     # [F][n][nb], computed once
    ref.setflags(write=False)
    return dict(m=m, names=names, F=F, bucket=bucket, lds=lds, maxm=maxm, ref=ref, train=fr,
                xs=Frame.from_numpy(Xs, names=names, device=cuda_dev),
                xb=Frame.from_numpy(Xb, names=names, device=cuda_dev))


def _tol(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


def test_kernel_path_exercised(case):
    assert _bucket(case["maxm"]) == case["bucket"], case["maxm"]
    assert (case["F"] * 256 * 4 <= 64 * 1024) == case["lds"]


def test_averaged_matches_numpy_and_margin(case):
    m, F, ref = case["m"], case["F"], case["ref"]
    C = predict_contributions(m, case["xs"], background_frame=case["xb"])
    assert C.names == case["names"] + ["BiasTerm"] and C.nrows == N_SCORE
    assert all(v.data.is_cuda for v in C.vecs)
    got = _stack(C, case["names"])
    want = ref.mean(2)
    print("averaged: max |kernel - numpy| =", np.abs(got - want).max(), "tol", _tol(want))
    np.testing.assert_allclose(got, want, atol=_tol(want))
    margin = m.ens.raw_margin(case["xs"].feature_matrix(m.x))[0]
    mb = m.ens.raw_margin(case["xb"].feature_matrix(m.x))[0]
    total = torch.stack([v.data for v in C.vecs]).sum(0)
    assert torch.allclose(total, margin, atol=5e-4 * max(1.0, float(margin.abs().max())))
    assert torch.allclose(C.vec("BiasTerm").data, mb.double().mean().float().expand(N_SCORE), atol=1e-6)
    assert "explain" in " ".join(_native.loaded_libraries())


def test_per_reference_matches_numpy_and_margin(case):
    m, F, ref = case["m"], case["F"], case["ref"]
    C = predict_contributions(m, case["xs"], background_frame=case["xb"], output_per_reference=True)
    assert C.names == ["RowIdx", "BackgroundRowIdx"] + case["names"] + ["BiasTerm"] and C.nrows == N_SCORE * N_BG
    np.testing.assert_array_equal(C.vec("RowIdx").data.cpu().numpy(), np.repeat(np.arange(N_SCORE), N_BG))
    np.testing.assert_array_equal(C.vec("BackgroundRowIdx").data.cpu().numpy(), np.tile(np.arange(N_BG), N_SCORE))
    got = _stack(C, case["names"]).reshape(F, N_SCORE, N_BG)
    print("per reference: max |kernel - numpy| =", np.abs(got - ref).max(), "tol", _tol(ref))
    np.testing.assert_allclose(got, ref, atol=_tol(ref))
    margin = m.ens.raw_margin(case["xs"].feature_matrix(m.x))[0]
    mb = m.ens.raw_margin(case["xb"].feature_matrix(m.x))[0]
    phi = torch.stack([C.vec(c).data for c in case["names"]]).sum(0).reshape(N_SCORE, N_BG)
    tol = 5e-4 * max(1.0, float(margin.abs().max()))
    assert torch.allclose(phi, margin[:, None] - mb[None, :], atol=tol)
    assert torch.allclose(phi + C.vec("BiasTerm").data.reshape(N_SCORE, N_BG), margin[:, None].expand(-1, N_BG),
                          atol=tol)


def test_single_background_row_and_single_scored_row(case, cuda_dev):
    m, ref = case["m"], case["ref"]
    one = torch.arange(1, device=cuda_dev)
    C = predict_contributions(m, case["xs"], background_frame=case["xb"].rows(one))           # nb = 1
    np.testing.assert_allclose(_stack(C, case["names"]), ref[:, :, 0], atol=_tol(ref))
    P = predict_contributions(m, case["xs"], background_frame=case["xb"].rows(one), output_per_reference=True)
    assert torch.equal(torch.stack([P.vec(c).data for c in case["names"]]),
                       torch.stack([C.vec(c).data for c in case["names"]]))
    C = predict_contributions(m, case["xs"].rows(one), background_frame=case["xb"])           # 1 scored row
    assert C.nrows == 1
    np.testing.assert_allclose(_stack(C, case["names"]), ref[:, :1].mean(2), atol=_tol(ref))
    P = predict_contributions(m, case["xs"].rows(one), background_frame=case["xb"], output_per_reference=True)
    np.testing.assert_allclose(_stack(P, case["names"]), ref[:, 0], atol=_tol(ref))


def test_two_calls_are_bit_identical(case):
    for per in (False, True):
        a = predict_contributions(case["m"], case["xs"], background_frame=case["xb"], output_per_reference=per)
        b = predict_contributions(case["m"], case["xs"], background_frame=case["xb"], output_per_reference=per)
        for u, v in zip(a.vecs, b.vecs):
            assert torch.equal(u.data, v.data), u.name


def test_path_dependent_kernel_unchanged(case):
    m, F = case["m"], case["F"]
    C = predict_contributions(m, case["xs"])
    assert C.names == case["names"] + ["BiasTerm"]
    out = torch.stack([v.data for v in C.vecs])
    assert out.is_cuda
    margin = m.ens.raw_margin(case["xs"].feature_matrix(m.x))[0]
    assert torch.allclose(out.sum(0), margin, atol=5e-4 * max(1.0, float(margin.abs().max())))
    nt = m.ens.ntrees
    lv, el, _, maxm, sets = tree_paths(m.ens.trees[:nt], 1.0 / nt if m.ens.average else 1.0)
    ref = _shap_numpy(_stack(case["xs"], case["names"]), lv, el, maxm, sets)
    np.testing.assert_allclose(out[:F].cpu().numpy(), ref, atol=2e-4 * max(1.0, np.abs(ref).max()))
    same = predict_contributions(m, case["xs"], background_frame=None, output_per_reference=False)
    assert all(torch.equal(u.data, v.data) for u, v in zip(C.vecs, same.vecs))


@pytest.mark.parametrize("F,mmax,bucket", [(40, 32, 32), (70, 32, 32), (40, 16, 16)])
def test_wide_paths_on_a_synthetic_table(cuda_dev, F, mmax, bucket):
    """Trained trees rarely split on more than 16 distinct features along one
    path, so the MAXM = 32 instantiation (and a full 16) runs on a hand-made
    path table: leaves of 1..mmax elements with one-sided intervals that a row
    satisfies with probability ~0.85, so that about half the pairs are alive."""
    rng = np.random.default_rng(100 * F + mmax)
    ms = [mmax, mmax, 1, 2, bucket // 2 + 1] + list(rng.integers(1, mmax + 1, 25))
    lv, el = [], []
    for m in ms:
        feats = rng.choice(F, m, replace=False)
        lv.append((len(el), m, int(np.float32(rng.normal()).view(np.int32)), 0))
        for f in feats:
            na_ok = int(rng.random() < 0.5)
            lo, hi = (-np.inf, 1.04) if rng.random() < 0.5 else (-1.04, np.inf)
            el.append((np.int32(int(f) | (na_ok << 30)).view(np.float32), 1.0, lo, hi))
    lv = np.asarray(lv, np.int32).reshape(-1, 4)
    feat_bits = np.asarray([e[0] for e in el], np.float32)
    el = np.asarray(el, np.float32).reshape(-1, 4)
    el[:, 0] = feat_bits
    sets = np.zeros((1, 8), np.uint32)
    maxm = int(lv[:, 1].max())
    assert _bucket(maxm) == bucket
    X = rng.normal(size=(F, N_SCORE)).astype(np.float32)
    B = rng.normal(size=(F, N_BG)).astype(np.float32)
    X[3, ::13] = np.nan
    B[3, ::13] = np.nan
    ref = _shap_background_numpy(X.astype(np.float64), B.astype(np.float64), lv, el, maxm, sets, per_reference=True)
    assert (np.abs(ref).sum(0) > 0).mean() > 0.2          # enough live pairs to mean something
    Xd, Bd = torch.from_numpy(X).to(cuda_dev), torch.from_numpy(B).to(cuda_dev)
    per = _shap_background_device(Xd, Bd, lv, el, maxm, sets, 1, True).cpu().numpy().reshape(F, N_SCORE, N_BG)
    print("synthetic per reference: max err", np.abs(per - ref).max(), "tol", _tol(ref))
    np.testing.assert_allclose(per, ref, atol=_tol(ref))
    for chunk in (5, N_BG):                               # 8 slabs with a short last one; one slab
        avg = _shap_background_device(Xd, Bd, lv, el, maxm, sets, chunk, False).cpu().numpy()
        np.testing.assert_allclose(avg, ref.mean(2), atol=_tol(ref.mean(2)))
