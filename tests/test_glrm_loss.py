"""GLRM with generalized losses: the tensor route against the np.longdouble oracle, the
refusals of the estimator, and the public fit on CPU and device frames."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

import glrm_loss_ref as R
from h2omx.frame.frame import Frame
from h2omx.models import glrm as M
from h2omx.models.glrm import H2OGeneralizedLowRankEstimator as GLRM
from h2omx.mojo import import_mojo

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
ENGINE = {"cpu": "proxgrad-torch", "cuda": "proxgrad-hip"}
COLS = [f"c{i}" for i in range(8)]


def test_loss_grad_torch_against_oracle():
    A, mask, X, Y, pars = R.inputs(333, 37, 10, R.MIXED)
    ref = R.grads_ref(A, mask, X, Y, R.MIXED, pars)
    t = [torch.from_numpy(v) for v in (A, mask, X, Y)]
    for wrt, g, b in (("x", "gx", "bx"), ("y", "gy", "by")):
        got, obj = M._loss_grad_torch(*t, np.asarray(R.MIXED), pars, wrt)
        assert (np.abs(got.numpy().astype(R.LD) - ref[g]) <= ref[b]).all()
        assert abs(R.LD(float(obj)) - ref["obj"]) <= ref["bobj"]


@pytest.mark.parametrize("kw,col,match", [
    (dict(loss="Logistic"), "c0", "c0"), (dict(loss_by_col=["Poisson"], loss_by_col_idx=[2]), "c2", "c2"),
    (dict(loss="Periodic", period=0), None, "period"), (dict(loss="Cubic"), None, "unknown loss"),
    (dict(loss_by_col=["Absolute", "Nope"], loss_by_col_idx=[0, 1]), None, "unknown loss")])
def test_validation(kw, col, match):
    df = pd.DataFrame(np.random.default_rng(0).integers(0, 2, (50, 8)).astype(np.float32), columns=COLS)
    if col:
        df.loc[3, col] = -2.0
    with pytest.raises(ValueError, match=match):
        GLRM(k=2, init="SVD", **kw).train(training_frame=Frame.from_pandas(df))


def test_all_quadratic_by_col_is_the_quadratic_fit():
    df = pd.DataFrame(np.random.default_rng(1).normal(size=(300, 8)).astype(np.float32), columns=COLS)
    df = df.mask(np.random.default_rng(2).random(df.shape) < 0.1)
    fits = [GLRM(k=3, init="SVD", max_iterations=15, **kw).train(training_frame=Frame.from_pandas(df))
            for kw in ({}, dict(loss_by_col=["Quadratic"] * 8))]
    assert fits[0].objective == fits[1].objective and np.array_equal(fits[0].Y, fits[1].Y)


@functools.lru_cache(None)
def _outliers():
    """1500 x 8 of rank 3, 15 % missing, 5 % of the observed entries replaced by +-20 x the scale."""
    rng = np.random.default_rng(2)
    clean = (rng.normal(size=(1500, 3)) @ rng.normal(size=(3, 8))).astype(np.float32)
    miss, hit = rng.random(clean.shape) < 0.15, rng.random(clean.shape) < 0.05
    data = np.where(hit, (20 * clean.std() * rng.choice([-1.0, 1.0], clean.shape)).astype(np.float32), clean)
    return clean, ~miss & ~hit, pd.DataFrame(data, columns=COLS).mask(miss)


@functools.lru_cache(None)
def _quadratic_mae(dev):
    clean, keep, df = _outliers()
    fr = Frame.from_pandas(df, device=dev)
    m = GLRM(k=3, init="SVD", max_iterations=100).train(training_frame=fr)
    return float(np.abs(m.predict(fr).to_pandas().to_numpy() - clean)[keep].mean())


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kw,code", [(dict(loss="Absolute"), R.ABS), (dict(loss_by_col=["Huber"] * 8), R.HUB)])
def test_robust_fit(dev, kw, code, tmp_path):
    clean, keep, df = _outliers()
    fr = Frame.from_pandas(df, device=dev)
    m = GLRM(k=3, init="SVD", max_iterations=300, min_step_size=1e-6, **kw).train(training_frame=fr)
    pred = m.predict(fr).to_pandas().to_numpy()
    mae = float(np.abs(pred - clean)[keep].mean())
    print(f"{kw} on {dev}: mae {mae:.4g} against Quadratic {_quadratic_mae(dev):.4g}, {m.iterations} iterations")
    assert mae < _quadratic_mae(dev)
    assert m.timings["als_engine"] == ENGINE[dev]
    objs = [h["objective"] for h in m.scoring_history]
    assert all(b < a for a, b in zip(objs, objs[1:])) and all("step_size" in h for h in m.scoring_history)
    # the reported objective against the oracle at the returned factors (fp32, so exactly those)
    mask = df.notna().to_numpy().T
    A = np.where(mask, df.to_numpy().T, 0).astype(np.float32)
    X = m.representation.to_pandas().to_numpy().T.astype(np.float32)
    ref = R.grads_ref(A, mask, X, m.Y.astype(np.float32), [code] * 8, np.zeros(8))
    assert abs(R.LD(m.objective) - ref["obj"]) <= ref["bobj"] + ref["bstore"]
    if dev == "cpu":
        g = import_mojo(m.download_mojo(str(tmp_path)))
        assert np.array_equal(g.predict(fr).to_pandas().to_numpy(), pred)


@pytest.mark.parametrize("dev", DEVICES)
def test_logistic_fit(dev):
    rng = np.random.default_rng(3)
    logit = 2.0 * rng.normal(size=(1500, 2)) @ rng.normal(size=(2, 8))
    data = (rng.random(logit.shape) < 1 / (1 + np.exp(-logit))).astype(np.float32)
    miss = rng.random(data.shape) < 0.15
    fr = Frame.from_pandas(pd.DataFrame(data, columns=COLS).mask(miss), device=dev)
    m = GLRM(k=2, init="SVD", loss="Logistic", max_iterations=200, min_step_size=1e-6).train(training_frame=fr)
    pred = m.predict(fr).to_pandas().to_numpy()
    assert set(np.unique(pred)) <= {0.0, 1.0} and m.timings["als_engine"] == ENGINE[dev]
    majority = np.where(np.nanmean(np.where(miss, np.nan, data), 0) > 0.5, 1.0, 0.0)[None, :]
    agree, guess = (pred == data)[~miss].mean(), (majority == data)[~miss].mean()
    print(f"logistic on {dev}: agreement {agree:.4f} against the majority guess {guess:.4f}")
    assert agree > guess
