"""The H statistic's HIP kernel (csrc/explain_kernels.hip:
friedman_h_pd_kernel<K>, h_slab_sum_kernel) against the float64 NumPy form on
the same leaf table for every K bucket end and ragged row counts, leaf
chunking and its determinism, the public ``model.h`` on a device frame
against the CPU path, and the device-side refusals."""
import math

import numpy as np
import pytest
import torch

import h2omx.explain as ex
from h2omx import _native
from h2omx.explain import (H_MAX_VARS_DEVICE, _h_leaf_table, _h_pd_device, _h_pd_numpy, friedman_h,
                           tree_paths)
from h2omx.frame import Frame
from h2omx.models import H2OGradientBoostingEstimator, H2ORandomForestEstimator

pytestmark = pytest.mark.gpu

N_TRAIN, N_SCORE, F = 3000, 1000, 6
NAMES = [f"f{i}" for i in range(F)]
CASES = {"gbm_d5": (H2OGradientBoostingEstimator, dict(ntrees=20, max_depth=5)),
         "drf_d10": (H2ORandomForestEstimator, dict(ntrees=5, max_depth=10))}
# the variables of each K (bit j of a subset is the j-th name); f0 and f2 hold the NaNs
VARS = {2: ["f0", "f2"], 3: ["f2", "f1", "f0"], H_MAX_VARS_DEVICE: ["f3", "f0", "f5", "f2", "f1", "f4"]}
ROWS = (1, 257, 1000)          # a single thread, one row past a workgroup, a ragged tail of four workgroups


def _xy(seed=11):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_TRAIN, F)).astype(np.float32)
    y = X[:, 0] * X[:, 1] + X[:, 2] + 0.5 * X[:, 3] + 0.1 * rng.normal(size=N_TRAIN)
    X[::11, 0] = np.nan
    X[3::17, 2] = np.nan
    return X, y.astype(np.float32)


@pytest.fixture(scope="module")
def data(cuda_dev):
    X, y = _xy()
    return X, y, Frame.from_numpy(np.c_[X, y], names=NAMES + ["y"], device=cuda_dev)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, data, cuda_dev):
    cls, kw = CASES[request.param]
    X, _, fr = data
    m = cls(seed=1, **kw).train(y="y", training_frame=fr)
    nt = m.ens.ntrees
    lv, el, _, maxm, _ = tree_paths(m.ens.trees[:nt], 1.0 / nt if m.ens.average else 1.0)
    Xs = np.ascontiguousarray(X[:N_SCORE].T)
    assert np.isnan(Xs[0]).any() and np.isnan(Xs[2]).any() and np.isnan(Xs[0, 0])
    tables, refs = {}, {}
    for k, names in VARS.items():
        tables[k] = _h_leaf_table(lv, el, [NAMES.index(v) for v in names])
        refs[k] = _h_pd_numpy(Xs.astype(np.float64), tables[k])          # [2^k - 1][1000], computed once
        refs[k].setflags(write=False)
    return dict(m=m, maxm=maxm, tables=tables, refs=refs, Xd=torch.from_numpy(Xs).to(cuda_dev),
                score=Frame.from_numpy(X[:N_SCORE], names=NAMES, device=cuda_dev),
                score_cpu=Frame.from_numpy(X[:N_SCORE], names=NAMES))


def _bound(case, k):
    """fp64 summation order only (the comparisons are exact on float32): the
    kept leaves' terms, each a product of at most maxm + 2 factors."""
    w = case["tables"][k]["w"]
    return w.shape[0] * (case["maxm"] + 2) * 2.0 ** -52 * float(np.abs(w).max())


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("k", list(VARS))
def test_kernel_matches_numpy(case, k, n):
    table, ref = case["tables"][k], case["refs"][k][:, :n]
    assert table["hdr"].shape[0] > 0 and table["w"].shape == (table["hdr"].shape[0], 1 << k)
    got = _h_pd_device(case["Xd"][:, :n].contiguous(), table)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == ((1 << k) - 1, n)
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print(f"k={k} n={n} leaves={table['hdr'].shape[0]}: max |kernel - numpy| = {err:.3e}, bound {_bound(case, k):.3e}")
    assert err <= _bound(case, k)
    assert "explain" in " ".join(_native.loaded_libraries())


@pytest.mark.parametrize("k", list(VARS))
def test_leaf_chunks_agree_and_repeat(case, k):
    table, X = case["tables"][k], case["Xd"]
    one = _h_pd_device(X, table, nchunks=1)
    a = _h_pd_device(X, table, nchunks=7)
    b = _h_pd_device(X, table, nchunks=7)
    err = float((one - a).abs().max())
    print(f"k={k}: max |1 chunk - 7 chunks| = {err:.3e}, bound {_bound(case, k):.3e}")
    assert err <= _bound(case, k)
    assert torch.equal(a, b)
    assert float(np.abs(one.cpu().numpy() - case["refs"][k]).max()) <= _bound(case, k)


def test_public_h_matches_cpu_path(case):
    m = case["m"]
    for names in VARS.values():
        got = m.h(case["score"], names)
        want = friedman_h(m, case["score_cpu"], names)
        print(m.algo, names, got, want)
        # depth-5 paths hold at most 5 features: the 6-variable H of the GBM is rounding noise around 0
        assert isinstance(got, float) and 0.0 <= want < 1.0
        assert got == pytest.approx(want, rel=1e-9)


def test_stumps_on_device(data):
    _, _, fr = data
    m = H2OGradientBoostingEstimator(ntrees=120, max_depth=1, seed=1).train(y="y", training_frame=fr)
    used = {int(tr["feat"][0]) for tr in m.ens.trees[:m.ens.ntrees]}
    assert {2, 3} <= used
    h = m.h(fr, ["f2", "f3"])
    print("stumps on the device", h)
    assert h < 1e-6


def test_unused_variables_on_device(cuda_dev):
    X, y = _xy(5)
    X[:, 4] = 1.5
    X[:, 5] = -2.0
    fr = Frame.from_numpy(np.c_[X, y], names=NAMES + ["y"], device=cuda_dev)
    m = H2OGradientBoostingEstimator(ntrees=10, max_depth=3, seed=1).train(y="y", training_frame=fr)
    used = {int(f) for tr in m.ens.trees[:m.ens.ntrees] for f in tr["feat"] if f >= 0}
    assert 2 in used and not used & {4, 5}
    assert m.h(fr, ["f2", "f4"]) == 0.0
    assert m.h(fr, ["f5", "f2"]) == 0.0
    assert math.isnan(m.h(fr, ["f4", "f5"]))


def test_device_refusals_launch_nothing(cuda_dev, monkeypatch):
    rng = np.random.default_rng(2)
    names = [f"c{i}" for i in range(H_MAX_VARS_DEVICE + 1)]
    X = rng.normal(size=(500, len(names))).astype(np.float32)
    y = X[:, 0] * X[:, 1] + X[:, 2]
    fr = Frame.from_numpy(np.c_[X, y], names=names + ["y"], device=cuda_dev)
    m = H2OGradientBoostingEstimator(ntrees=3, max_depth=3, seed=1).train(y="y", training_frame=fr)
    pair = [names[2], names[0]]                     # c2 is a main effect: some tree uses it
    assert 0.0 <= m.h(fr, pair) < 1.0

    def no_launch(*a, **k):
        raise AssertionError("the kernel path was entered")

    monkeypatch.setattr(ex, "_h_pd_device", no_launch)
    with pytest.raises(ValueError, match=f"at most {H_MAX_VARS_DEVICE} variables on the device"):
        m.h(fr, names)
    total = torch.cuda.mem_get_info(cuda_dev)[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (2000, total))
    # 3 subsets x 500 rows x 8 bytes = 12000 bytes against half of 2000
    with pytest.raises(ValueError, match=r"500 rows needs 12000 bytes.*limit is 1000 bytes.*sample"):
        m.h(fr, pair)
