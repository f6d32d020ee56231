"""The path-dependent TreeSHAP kernel (csrc/explain_kernels.hip
tree_shap_kernel) against the division-free float64 reference of
tests/shapref.py, on hand-made path tables that reach every MAXM instantiation
(8, 16, 32) on both accumulator routes (LDS for F = 40, global for F = 70)
with zero fractions from balanced to near one, NaN cells, categorical level
sets and levels outside them; additivity on the device, a single scored row,
run-to-run determinism, the 32-feature limit, and one trained forest whose
chain-shaped paths reach the 32 bucket.  tests/test_shapref.py pins the
reference and the tables on the CPU."""
import numpy as np
import pytest
import torch

import shapref as SR
from h2omx import _native
from h2omx.explain import _bucket, _shap_device, predict_contributions, tree_paths
from h2omx.frame import Frame
from h2omx.models import H2ORandomForestEstimator

pytestmark = pytest.mark.gpu

TABLES = SR.table_ids()


def _ids(t):
    return f"m{t[0]}-{t[1]}-F{t[2]}"


def _tol(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


_OUT = {}


def _score(t, dev) -> torch.Tensor:
    # copies: the shared tables are read-only
    X = torch.tensor(t["X"], device=dev)
    return _shap_device(X, t["lv"].copy(), t["el"].copy(), t["maxm"], t["sets"].copy())


def _device_out(table, dev) -> torch.Tensor:
    """[F][300] of one table, scored once"""
    if table not in _OUT:
        _OUT[table] = _score(SR.reference(*table)[0], dev)
    return _OUT[table]


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_kernel_matches_the_reference(cuda_dev, table):
    bucket, regime, F = table
    t, ref, tot = SR.reference(*table)
    assert _bucket(t["maxm"]) == bucket
    out = _device_out(table, cuda_dev)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (F, SR.N_ROWS)
    got = out.cpu().numpy().astype(np.float64)
    print(f"{_ids(table)}: max |kernel - shapref| = {np.abs(got - ref).max():.3e}  tol {_tol(ref):.3e}  "
          f"max |ref| = {np.abs(ref).max():.3f}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=_tol(ref))
    assert "explain" in " ".join(_native.loaded_libraries())


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_additivity_on_the_device(cuda_dev, table):
    t, ref, tot = SR.reference(*table)
    got = _device_out(table, cuda_dev).sum(0).cpu().numpy().astype(np.float64)
    print(f"{_ids(table)}: max |sum of contributions - total| = {np.abs(got - tot).max():.3e}  tol {_tol(ref):.3e}")
    np.testing.assert_allclose(got, tot, rtol=0, atol=_tol(ref))


@pytest.mark.parametrize("table", TABLES, ids=_ids)
def test_one_row_and_a_second_call_give_the_same_bits(cuda_dev, table):
    t = SR.reference(*table)[0]
    out = _device_out(table, cuda_dev)
    assert torch.equal(_score(t, cuda_dev), out)
    one = SR.tables(*table, n=1)
    assert one["X"].shape == (table[2], 1) and np.array_equal(one["X"][:, 0], t["X"][:, 0], equal_nan=True)
    first = _score(one, cuda_dev)
    assert tuple(first.shape) == (table[2], 1) and torch.equal(first[:, 0], out[:, 0])


def test_more_than_32_features_on_a_path_is_an_argument_error(cuda_dev):
    F, m = 40, 33
    lv = np.array([[0, m, int(np.array([1.0], np.float32).view(np.int32)[0]), 0]], np.int32)
    el = np.zeros((m, 4), np.float32)
    el[:, 0] = np.arange(m, dtype=np.int32).view(np.float32)
    el[:, 1], el[:, 2], el[:, 3] = 0.5, -np.inf, 0.0
    X = torch.zeros((F, 5), device=cuda_dev)
    with pytest.raises(RuntimeError, match="more than 32 distinct features are unsupported on the device"):
        _shap_device(X, lv, el, m, np.zeros((1, 8), np.uint32))


def test_trained_forest_reaches_the_widest_bucket(cuda_dev):
    """Sparse binary features, each 5 % ones, make chain-shaped trees: every
    split peels a few percent of the rows off, so a deep path splits on many
    distinct features and its zero fractions are near one."""
    F, n_train, n_score = 40, 3000, 64
    rng = np.random.default_rng(11)
    X = (rng.random((n_train, F)) < 0.05).astype(np.float32)
    y = (X @ rng.normal(size=F) + 0.1 * rng.normal(size=n_train)).astype(np.float32)
    names = [f"f{i}" for i in range(F)]
    fr = Frame.from_numpy(np.c_[X, y], names=names + ["y"], device=cuda_dev)
    m = H2ORandomForestEstimator(ntrees=2, max_depth=26, min_rows=2.0, mtries=-2, seed=1).train(
        y="y", training_frame=fr)
    nt = m.ens.ntrees
    lv, el, _, maxm, sets = tree_paths(m.ens.trees[:nt], 1.0 / nt)
    assert maxm > 16 and _bucket(maxm) == 32, maxm
    ref = SR.contributions(X[:n_score].T, lv, el, sets)
    xs = Frame.from_numpy(X[:n_score], names=names, device=cuda_dev)
    C = predict_contributions(m, xs)
    got = torch.stack([C.vec(c).data for c in names]).cpu().numpy().astype(np.float64)
    print(f"trained forest: {len(lv)} leaves, up to {maxm} features on a path; max |kernel - shapref| = "
          f"{np.abs(got - ref).max():.3e}  tol {_tol(ref):.3e}")
    np.testing.assert_allclose(got, ref, rtol=0, atol=_tol(ref))
    margin = m.ens.raw_margin(xs.feature_matrix(m.x))[0]
    total = torch.stack([v.data for v in C.vecs]).sum(0)
    assert torch.allclose(total, margin, atol=5e-4 * max(1.0, float(margin.abs().max())))
