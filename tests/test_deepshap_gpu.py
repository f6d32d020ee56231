"""DeepSHAP on the device (csrc/explain_kernels.hip: deepshap_rescale_kernel,
deepshap_fold_kernel, and the project's GEMM between them) against the
float64 pair-by-pair oracle of tests/deepshap_ref.py: both output forms, all
three activations, hidden widths that leave tail lanes, span several waves
and are no multiple of 4, a folded categorical predictor, nb = 1 and n = 1,
several row blocks with a ragged last one, near ties, completeness against
the device margin, run-to-run determinism and the ranked form."""
import numpy as np
import pytest
import torch

import deepshap_ref as DR
from h2omx import _native
from h2omx.explain import _contributions_deeplearning, _rank_numpy, _rank_spec, predict_contributions
from h2omx.frame import Frame
from h2omx.frame.frame import Vec

pytestmark = pytest.mark.gpu

N_TRAIN, N_SCORE, N_BG = 500, 300, 37
PRED = ["x0", "x1", "g", "x2", "x3"]
HIDDEN = [(7,), (33, 65), (64, 5, 130)]
# every activation on every width list; regression and binomial alternate
CASES = [(a, h, ("regression", "binomial")[(i + j) % 2]) for i, a in enumerate(DR.ACTS) for j, h in enumerate(HIDDEN)]


def _tol(ref):
    return 2e-4 * max(1.0, float(np.abs(ref).max()))


def _split(kind, dev, seed=11):
    df = DR.make_df(N_TRAIN + N_SCORE + N_BG, seed, kind=kind)
    cut = N_TRAIN + N_SCORE
    train = Frame.from_pandas(df.iloc[:N_TRAIN].reset_index(drop=True), device=dev)
    x = Frame.from_pandas(df.iloc[N_TRAIN:cut].drop(columns="y").reset_index(drop=True), device=dev)
    b = Frame.from_pandas(df.iloc[cut:].drop(columns="y").reset_index(drop=True), device=dev)
    return train, x, b


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2]}")
def case(request, cuda_dev):
    act, hidden, kind = request.param
    train, x, b = _split(kind, cuda_dev)
    m = DR.fit(train, act, hidden)
    xs, bs = DR.design_rows(m, x), DR.design_rows(m, b)
    assert xs.shape == (N_SCORE, 7) and np.isnan(x.vec("x1").data.cpu().numpy()).any()
    DR.condition(m, xs, bs)                       # reseeds the weights until the oracle's inputs are conditioned
    assert DR.min_gap(m, xs, bs) >= 1e-6          # the oracle's naive quotient keeps >= 9 digits
    phi, mx, mb = DR.oracle(m, xs, bs)            # [n][nb][C], computed once
    phi.setflags(write=False)
    return dict(m=m, x=x, b=b, phi=phi, mx=mx, mb=mb, id="-".join(map(str, request.param)))


def _planes(C, n, nb=None):
    a = DR.stack(C, PRED).T
    return a if nb is None else a.reshape(n, nb, -1)


def _device_margin(m, fr):
    P = m.predict_raw(m.adapt_frame(fr))
    return (torch.log(P[1]) - torch.log(P[0])) if P.shape[0] == 2 else P[0]


def test_both_forms_match_the_oracle_and_the_margin(case):
    m, phi = case["m"], case["phi"]
    avg = predict_contributions(m, case["x"], background_frame=case["b"])
    assert avg.names == PRED + ["BiasTerm"] and avg.nrows == N_SCORE
    assert all(v.data.is_cuda for v in avg.vecs)
    want = phi.mean(1)
    print(f"{case['id']} averaged: max |kernel - oracle| = {np.abs(_planes(avg, N_SCORE) - want).max():.3e} "
          f"tol {_tol(want):.3e}")
    np.testing.assert_allclose(_planes(avg, N_SCORE), want, atol=_tol(want))
    per = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=True)
    assert per.names == ["RowIdx", "BackgroundRowIdx"] + PRED + ["BiasTerm"] and per.nrows == N_SCORE * N_BG
    np.testing.assert_array_equal(per.vec("RowIdx").data.cpu().numpy(), np.repeat(np.arange(N_SCORE), N_BG))
    np.testing.assert_array_equal(per.vec("BackgroundRowIdx").data.cpu().numpy(), np.tile(np.arange(N_BG), N_SCORE))
    got = _planes(per, N_SCORE, N_BG)
    print(f"{case['id']} per reference: max |kernel - oracle| = {np.abs(got - phi).max():.3e} tol {_tol(phi):.3e}")
    np.testing.assert_allclose(got, phi, atol=_tol(phi))
    # completeness against the device margin
    margin, mb = _device_margin(m, case["x"]), _device_margin(m, case["b"])
    tol = 5e-4 * max(1.0, float(margin.abs().max()))
    total = torch.stack([v.data for v in avg.vecs]).sum(0)
    assert torch.allclose(total, margin, atol=tol)
    ps = torch.stack([per.vec(c).data for c in PRED]).sum(0).reshape(N_SCORE, N_BG)
    assert torch.allclose(ps, margin[:, None] - mb[None, :], atol=tol)
    assert torch.allclose(ps + per.vec("BiasTerm").data.reshape(N_SCORE, N_BG), margin[:, None].expand(-1, N_BG),
                          atol=tol)
    assert "explain" in " ".join(_native.loaded_libraries())


def test_single_background_row_and_single_scored_row(case, cuda_dev):
    m, phi = case["m"], case["phi"]
    one = torch.arange(1, device=cuda_dev)
    C = predict_contributions(m, case["x"], background_frame=case["b"].rows(one))             # nb = 1
    np.testing.assert_allclose(_planes(C, N_SCORE), phi[:, 0], atol=_tol(phi))
    C = predict_contributions(m, case["x"].rows(one), background_frame=case["b"])             # 1 scored row
    assert C.nrows == 1
    np.testing.assert_allclose(_planes(C, 1), phi[:1].mean(1), atol=_tol(phi))
    P = predict_contributions(m, case["x"].rows(one), background_frame=case["b"], output_per_reference=True)
    np.testing.assert_allclose(_planes(P, 1, N_BG), phi[:1], atol=_tol(phi))


def test_row_blocks_with_a_ragged_last_one(case):
    """A work-space budget of 120 scored rows: blocks of 120, 120 and 60."""
    m, phi = case["m"], case["phi"]
    width = max([7] + [w for _, w, _ in m.net.layers[:-1]])
    budget = 2 * 4 * N_BG * width * 120 + 64
    for per in (False, True):
        C = _contributions_deeplearning(m, case["x"], case["b"], per, None, None, False, _budget=budget)
        want = phi if per else phi.mean(1)
        got = _planes(C, N_SCORE, N_BG if per else None)
        np.testing.assert_allclose(got, want, atol=_tol(want))
        whole = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=per)
        np.testing.assert_allclose(got, _planes(whole, N_SCORE, N_BG if per else None), atol=_tol(want))
    with pytest.raises(ValueError, match=rf"one row against {N_BG} background rows needs {2 * 4 * N_BG * width} bytes"
                                         r".*limit is 100 bytes"):
        _contributions_deeplearning(m, case["x"], case["b"], False, None, None, False, _budget=100)


def test_two_calls_are_bit_identical(case):
    for per in (False, True):
        a = predict_contributions(case["m"], case["x"], background_frame=case["b"], output_per_reference=per)
        b = predict_contributions(case["m"], case["x"], background_frame=case["b"], output_per_reference=per)
        for u, v in zip(a.vecs, b.vecs):
            assert torch.equal(u.data, v.data), u.name


@pytest.mark.parametrize("kw", [dict(top_n=2, bottom_n=1), dict(bottom_n=-1, compare_abs=True)])
def test_ranked_call_equals_rank_numpy_on_the_plane(case, kw):
    m = case["m"]
    for per in (False, True):
        plain = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=per)
        plane = torch.stack([plain.vec(c).data for c in PRED]).cpu().numpy()
        kt, kb = _rank_spec(kw.get("top_n"), kw.get("bottom_n"), len(PRED))
        idx, val = _rank_numpy(plane, kt, kb, kw.get("compare_abs", False))
        got = predict_contributions(m, case["x"], background_frame=case["b"], output_per_reference=per, **kw)
        lead = 2 if per else 0
        assert len(got.names) == lead + 2 * (kt + kb) + 1
        for s in range(kt + kb):
            np.testing.assert_array_equal(got.vecs[lead + 2 * s].data.cpu().numpy(), idx[s])
            np.testing.assert_array_equal(got.vecs[lead + 2 * s + 1].data.cpu().numpy(), val[s])
        assert torch.equal(got.vec("BiasTerm").data, plain.vec("BiasTerm").data)


def test_a_net_without_hidden_layers(cuda_dev):
    """No rescale stage and no GEMM: the output row is every pair's G_0."""
    train, x, b = _split("binomial", cuda_dev, seed=17)
    m = DR.fit(train, "Rectifier", ())
    phi, _, _ = DR.oracle(m, DR.design_rows(m, x), DR.design_rows(m, b))
    for per in (False, True):
        C = predict_contributions(m, x, background_frame=b, output_per_reference=per)
        want = phi if per else phi.mean(1)
        np.testing.assert_allclose(_planes(C, N_SCORE, N_BG if per else None), want, atol=_tol(want))


@pytest.mark.parametrize("act", ["Tanh", "ExpRectifier"])
@pytest.mark.parametrize("hidden", [(33, 65)])
def test_near_ties_keep_their_digits(cuda_dev, act, hidden):
    """Scored row k is background row k moved by 1e-4 in the standardised x2,
    so every pre-activation of pair (k, k) differs by about 1e-4 times a weight:
    a float32 (f(a) - f(b)) / (a - b) has lost three or four digits there.  The
    pairs (k, k) are compared on their own scale (no floor of 1 under the
    tolerance), then every pair on the scale of all of them.  Rectifier is left
    out: at its kink the multiplier itself is ill-conditioned."""
    train, _, b = _split("regression", cuda_dev, seed=13)
    m = DR.fit(train, act, hidden)
    j2 = m.design.names.index("x2")
    moved = b.vec("x2").data + float(1e-4 * m.design.sds[j2])
    x = Frame([v if v.name != "x2" else Vec("x2", moved, v.vtype, v.domain) for v in b.vecs])
    xs, bs = DR.design_rows(m, x), DR.design_rows(m, b)
    gap = xs[:, j2] - bs[:, j2]
    assert np.all((gap > 5e-5) & (gap < 2e-4)) and np.array_equal(np.delete(xs, j2, 1), np.delete(bs, j2, 1))
    phi, _, _ = DR.oracle(m, xs, bs)
    per = predict_contributions(m, x, background_frame=b, output_per_reference=True)
    got = DR.stack(per, PRED).T.reshape(N_BG, N_BG, -1)
    assert np.isfinite(got).all()
    k = np.arange(N_BG)
    near, near_ref = got[k, k], phi[k, k]
    assert np.abs(near_ref).max() > 0
    print(f"{act} near ties: max |kernel - oracle| = {np.abs(near - near_ref).max():.3e} on the pairs (k, k), "
          f"tol {2e-4 * np.abs(near_ref).max():.3e}; {np.abs(got - phi).max():.3e} on all, "
          f"tol {2e-4 * np.abs(phi).max():.3e}")
    np.testing.assert_allclose(near, near_ref, rtol=0, atol=2e-4 * np.abs(near_ref).max())
    np.testing.assert_allclose(got, phi, rtol=0, atol=2e-4 * np.abs(phi).max())
