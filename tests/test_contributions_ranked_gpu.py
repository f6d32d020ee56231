"""contrib_rank_kernel (csrc/explain_kernels.hip) on the device: the entry point
on synthetic planes against ``_rank_numpy`` on both sides of the LDS-staging
boundary (F = 64 / 65), with heavy ties, signed zeros, a ragged last workgroup
and a strided view; the public ranked call on a device frame in the three SHAP
forms; repeatability; the unchanged default call; refused arguments.  Ranking
moves floats and computes none, so every comparison is exact."""
import numpy as np
import pandas as pd
import pytest
import torch

import h2omx.explain as ex
from h2omx import _native
from h2omx.explain import _rank_device, _rank_numpy, _rank_spec, predict_contributions
from h2omx.frame import Frame
from h2omx.frame.frame import ENUM
from h2omx.models import H2OGradientBoostingEstimator, H2ORandomForestEstimator

pytestmark = pytest.mark.gpu

K_BAD_ARG = 1


def specs(F):
    out = [(1, 0), (0, 1), (F, 0), (0, F), (min(3, F), 0)]
    return out + ([(3, 2)] if F >= 6 else [])


def planes(kind, F, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        # small integers, most comparisons are ties; a third of the zeros are negative
        phi = rng.integers(-2, 3, size=(F, n)).astype(np.float32)
        phi[(phi == 0) & (rng.random((F, n)) < 0.33)] = -0.0
        return phi
    phi = rng.normal(size=(F, n)).astype(np.float32)
    phi[rng.random((F, n)) < 0.05] *= -1.0
    return phi


def assert_ranked(phi_dev, phi_np, kt, kb, ca):
    idx, val = _rank_device(phi_dev, kt, kb, ca)
    ridx, rval = _rank_numpy(phi_np, kt, kb, ca)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and idx.is_cuda and val.is_cuda
    assert torch.equal(idx.cpu(), torch.from_numpy(ridx)), (kt, kb, ca)
    # bit for bit: a reported zero keeps its sign
    assert torch.equal(val.cpu().view(torch.int32), torch.from_numpy(rval).view(torch.int32)), (kt, kb, ca)
    return idx, val


@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("F", [1, 2, 7, 64, 65, 100])
def test_entry_point_matches_rank_numpy(cuda_dev, F, n):
    for kind in ("ties", "normal"):
        phi = planes(kind, F, n, seed=1000 * F + n)
        if kind == "ties" and F * n >= 64:
            assert np.signbit(phi[phi == 0]).any() and not np.signbit(phi[phi == 0]).all()
        dev = torch.from_numpy(phi).to(cuda_dev)
        for ca in (False, True):
            for kt, kb in specs(F):
                assert_ranked(dev, phi, kt, kb, ca)
    assert "explain" in " ".join(_native.loaded_libraries())


@pytest.mark.parametrize("F", [7, 65])
def test_strided_view_never_reads_past_n(cuda_dev, F):
    n, ld, sentinel = 300, 337, np.float32(1e30)
    wide = np.full((F, ld), sentinel, np.float32)
    wide[:, :n] = planes("normal", F, n, seed=F)
    dev = torch.from_numpy(wide).to(cuda_dev)[:, :n]
    assert dev.stride(0) == ld and not dev.is_contiguous()
    for ca in (False, True):
        for kt, kb in specs(F):
            _, val = assert_ranked(dev, wide[:, :n], kt, kb, ca)
            assert bool((val.abs() < 1e29).all())


def test_bad_arguments_are_refused_without_a_launch(cuda_dev):
    from h2omx.ops import P, explain_lib, stream

    F, n = 5, 10
    phi = torch.zeros((F, n), dtype=torch.float32, device=cuda_dev)
    idx = torch.full((2 * F, n), -7, dtype=torch.int32, device=cuda_dev)
    val = torch.full((2 * F, n), -7.0, dtype=torch.float32, device=cuda_dev)
    call = lambda ld, n_, F_, kt, kb: explain_lib().h2omx_contrib_rank(       # noqa: E731
        P(phi), ld, n_, F_, kt, kb, 0, P(idx), P(val), stream(cuda_dev))
    assert call(n, n, F, F + 1, 0) == K_BAD_ARG          # kt > F
    assert call(n, n, F, 0, F + 1) == K_BAD_ARG          # kb > F
    assert call(n, n, F, 0, 0) == K_BAD_ARG              # nothing asked for
    assert call(n, n, 0, 0, 0) == K_BAD_ARG              # F = 0
    assert call(n, n, 0, 1, 0) == K_BAD_ARG
    assert call(n, n, F, -1, 1) == K_BAD_ARG
    assert call(n, n, F, 1, -1) == K_BAD_ARG
    assert call(n - 1, n, F, 1, 0) == K_BAD_ARG          # ld < n
    assert call(n, 0, F, 1, 0) == 0                      # no rows: nothing to do
    torch.cuda.synchronize(cuda_dev)
    assert bool((idx == -7).all()) and bool((val == -7.0).all())


# ---------------------------------------------------------------------------
# public call on a device frame
# ---------------------------------------------------------------------------
N_TRAIN, N_SCORE, N_BG = 2000, 300, 11     # 300 rows: one full + one partial workgroup; 3300 pairs


def _mixed(n, seed=0):
    """a, b, c numeric with NaNs, k constant (never split: its zeros tie), e enum."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 3)).astype(np.float32)
    X[::17, 1] = np.nan
    X[5::29, 2] = np.nan
    e = rng.choice(["u", "v", "w", "x"], n)
    f = X[:, 0] - np.nan_to_num(X[:, 1]) * np.nan_to_num(X[:, 2]) + np.where(e == "w", 1.5, 0.0)
    df = pd.DataFrame(X, columns=list("abc"))
    df["k"] = np.float32(2.5)
    df["e"] = pd.Categorical(e)
    df["yreg"] = (f + 0.1 * rng.normal(size=n)).astype(np.float32)
    df["ycls"] = pd.Categorical(np.where(f + 0.3 * rng.normal(size=n) > 0, "p", "q"))
    return df


def _wide(n, F=70, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[::13, 0] = np.nan
    df = pd.DataFrame(X, columns=[f"f{i}" for i in range(F)])
    df["yreg"] = (np.nan_to_num(X[:, 0]) + X[:, 1] * X[:, 2] + X[:, 60] + 0.1 * rng.normal(size=n)).astype(np.float32)
    return df


CASES = {
    # name: (data, estimator, parameters, response, predictors)
    "gbm_regression": (_mixed, H2OGradientBoostingEstimator, dict(ntrees=8, max_depth=4), "yreg", list("abcke")),
    "drf_binomial": (_mixed, H2ORandomForestEstimator, dict(ntrees=5, max_depth=5), "ycls", list("abcke")),
    # 70 planes: past the LDS-staging boundary of the rank kernel
    "gbm_wide": (_wide, H2OGradientBoostingEstimator, dict(ntrees=5, max_depth=4), "yreg",
                 [f"f{i}" for i in range(70)]),
}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, cuda_dev):
    data, cls, kw, y, x = CASES[request.param]
    df = data(N_TRAIN)
    fr = Frame.from_pandas(df, device=cuda_dev)
    m = cls(seed=1, **kw).train(x=x, y=y, training_frame=fr)
    assert m.x == x
    xs = fr.rows(torch.arange(0, N_SCORE))
    xb = fr.rows(torch.arange(1001, 1001 + N_BG))
    kws = {"path": {}, "averaged": dict(background_frame=xb),
           "per_reference": dict(background_frame=xb, output_per_reference=True)}
    plain = {form: predict_contributions(m, xs, **kw) for form, kw in kws.items()}       # computed once
    return dict(m=m, x=x, xs=xs, kws=kws, plain=plain)


def _requests(F):
    return [(3, None, False), (None, 2, True), (2, 2, False), (-1, None, True), (0, -1, False)] + \
        ([(F - 2, 2, False)] if F < 10 else [])


@pytest.mark.parametrize("form", ["path", "averaged", "per_reference"])
def test_public_ranked_call(case, form):
    m, names, xs = case["m"], case["x"], case["xs"]
    F = len(names)
    plain = case["plain"][form]
    nlead = 2 if form == "per_reference" else 0
    lead = ["RowIdx", "BackgroundRowIdx"][:nlead]
    assert plain.names == lead + names + ["BiasTerm"]
    assert plain.nrows == (N_SCORE * N_BG if nlead else N_SCORE)
    phi = torch.stack([plain.vec(c).data for c in names]).cpu().numpy()
    if "k" in names:
        assert (phi[names.index("k")] == 0).all()
    for top_n, bottom_n, ca in _requests(F):
        kt, kb = _rank_spec(top_n, bottom_n, F)
        got = m.predict_contributions(xs, top_n=top_n, bottom_n=bottom_n, compare_abs=ca, **case["kws"][form])
        want = lead[:]
        for side, k in (("top", kt), ("bottom", kb)):
            for i in range(1, k + 1):
                want += [f"{side}_feature_{i}", f"{side}_value_{i}"]
        assert got.names == want + ["BiasTerm"] and got.nrows == plain.nrows
        assert all(v.data.is_cuda for v in got.vecs)
        idx, val = _rank_numpy(phi, kt, kb, ca)
        for s in range(kt + kb):
            fv, vv = got.vecs[nlead + 2 * s], got.vecs[nlead + 2 * s + 1]
            assert fv.vtype == ENUM and list(fv.domain) == names
            assert torch.equal(fv.data.cpu(), torch.from_numpy(idx[s])), fv.name
            assert torch.equal(vv.data.cpu().view(torch.int32), torch.from_numpy(val[s]).view(torch.int32)), vv.name
        for c in lead + ["BiasTerm"]:
            assert torch.equal(got.vec(c).data, plain.vec(c).data), c


@pytest.mark.parametrize("form", ["path", "averaged", "per_reference"])
def test_two_ranked_calls_are_bit_identical(case, form):
    kw = dict(top_n=2, bottom_n=2, compare_abs=True, **case["kws"][form])
    a = predict_contributions(case["m"], case["xs"], **kw)
    b = predict_contributions(case["m"], case["xs"], **kw)
    assert a.names == b.names
    for u, v in zip(a.vecs, b.vecs):
        assert torch.equal(u.data, v.data), u.name


@pytest.mark.parametrize("form", ["path", "averaged", "per_reference"])
def test_default_call_is_the_input_of_the_ranked_call(case, form, monkeypatch):
    """The guard that the unsorted path did not change: what the default call
    returns is, plane by plane, the tensor that the ranked call hands to the
    rank kernel."""
    seen = []
    real = ex._rank_device

    def spy(phi, kt, kb, compare_abs):
        seen.append(phi)
        return real(phi, kt, kb, compare_abs)

    monkeypatch.setattr(ex, "_rank_device", spy)
    predict_contributions(case["m"], case["xs"], top_n=1, **case["kws"][form])
    assert len(seen) == 1 and seen[0].is_cuda and seen[0].shape[0] == len(case["x"])
    monkeypatch.undo()
    default = predict_contributions(case["m"], case["xs"], **case["kws"][form])
    nlead = 2 if form == "per_reference" else 0
    assert default.names == case["plain"][form].names
    for j, c in enumerate(case["x"]):
        assert default.vecs[nlead + j].name == c
        assert torch.equal(default.vecs[nlead + j].data, seen[0][j]), c
    for u, v in zip(default.vecs, case["plain"][form].vecs):
        assert torch.equal(u.data, v.data), u.name
