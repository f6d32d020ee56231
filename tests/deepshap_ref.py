"""Shared pieces of the DeepSHAP tests (tests/test_deepshap.py on the CPU,
tests/test_deepshap_gpu.py on the HIP kernels): seeded data, briefly fitted
Deep Learning models whose weights are then overwritten with seeded values,
and an independent float64 oracle of DeepLIFT's rescale rule.

The oracle walks pair by pair and layer by layer with the naive multiplier
(f(a) - f(b)) / (a - b), f'(a) at an exact tie.  From the code under test it
takes the model's weights and its ``design`` (the standardised design rows)
and nothing else, so it shares no formula with h2omx.explain.  In float64 the
naive quotient loses about 2^-52 / |a - b| of its digits, which is why
:func:`min_gap` must hold for the data it is run on."""
import numpy as np
import pandas as pd
import torch

from h2omx.frame import Frame
from h2omx.models import H2ODeepLearningEstimator
from h2omx.models.base import ModelCategory

ACTS = ("Rectifier", "Tanh", "ExpRectifier")
NUM = ["x0", "x1", "x2", "x3"]


def make_df(n: int, seed: int, enum: bool = True, kind: str = "regression") -> pd.DataFrame:
    """Four numerical predictors (x1 with a few NAs) and, between them, one
    3-level categorical ``g``; ``y`` numerical, 2-class or 3-class."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 4)).astype(np.float32)
    X[3::41, 1] = np.nan
    g = rng.choice(["a", "b", "c"], n)
    df = pd.DataFrame({"x0": X[:, 0], "x1": X[:, 1]})
    if enum:
        df["g"] = pd.Categorical(g)
    df["x2"], df["x3"] = X[:, 2], X[:, 3]
    s = X[:, 0] - np.nan_to_num(X[:, 1]) * X[:, 2] + 0.5 * (g == "b") + 0.3 * rng.normal(size=n)
    if kind == "regression":
        df["y"] = (3.0 * s + 1.0).astype(np.float32)
    elif kind == "binomial":
        df["y"] = pd.Categorical(np.where(s > 0, "pos", "neg"))
    else:
        df["y"] = pd.Categorical(np.where(s > 0.7, "hi", np.where(s > -0.7, "mid", "lo")))
    return df


def seed_weights(model, seed: int) -> None:
    """Overwrite ``model.net.flat``: weights uniform in +-1.5 / sqrt(fan-in)
    and biases uniform in +-0.5, so that pre-activations are O(1) with both signs."""
    gen = torch.Generator().manual_seed(seed)
    net = model.net
    flat = torch.empty(net.flat.numel(), dtype=torch.float32)
    for off, w, f in net.layers:
        flat[off: off + w * f].uniform_(-1.0, 1.0, generator=gen).mul_(1.5 / np.sqrt(f))
        flat[off + w * f: off + w * f + w].uniform_(-0.5, 0.5, generator=gen)
    net.flat.copy_(flat.to(net.flat.device))


def fit(train: Frame, activation: str, hidden, seed: int = 7, **kw):
    """A short fit, only to obtain the model object, then seeded weights."""
    m = H2ODeepLearningEstimator(hidden=list(hidden), epochs=0.1, activation=activation, seed=1, **kw).train(
        y="y", training_frame=train)
    seed_weights(m, seed)
    return m


def design_rows(model, frame: Frame) -> np.ndarray:
    """The standardised, mean-imputed, one-hot design rows [rows][p] as float64
    (of the float32 values the model scores)."""
    d = model.design
    return d.transform(d.raw_matrix(model.adapt_frame(frame))).T.cpu().numpy().astype(np.float64)


def _weights(model):
    net = model.net
    L = len(net.layers)
    W = [net.W(i).detach().cpu().numpy().astype(np.float64) for i in range(L)]
    b = [net.b(i).detach().cpu().numpy().astype(np.float64) for i in range(L)]
    return W, b


_F = {1: (lambda z: np.maximum(z, 0.0), lambda z: (z > 0).astype(np.float64)),
      2: (np.tanh, lambda z: 1.0 - np.tanh(z) ** 2),
      4: (lambda z: np.where(z > 0, z, np.expm1(np.minimum(z, 0.0))),
          lambda z: np.where(z > 0, 1.0, np.exp(np.minimum(z, 0.0))))}


def _forward(model, rows: np.ndarray):
    """(hidden pre-activations [L][rows][h], margins [rows]) in float64."""
    W, b = _weights(model)
    f = _F[model.act][0]
    H, Zs = rows, []
    for l in range(len(W) - 1):
        Zs.append(H @ W[l].T + b[l])
        H = f(Zs[-1])
    out = H @ W[-1].T + b[-1]
    if model.category == ModelCategory.BINOMIAL:
        return Zs, out[:, 1] - out[:, 0]
    return Zs, out[:, 0] * model.y_sd + model.y_mean


def groups(model):
    """(predictor names, their design column lists) in ``design.x`` order."""
    d = model.design
    cols = [c for c in d.x if any(col == c for col, _ in d.spec)]
    return cols, [[j for j, (col, _) in enumerate(d.spec) if col == c] for c in cols]


def min_gap(model, xs: np.ndarray, bs: np.ndarray) -> float:
    """The smallest non-zero |zx - zb| over every (pair, hidden unit)."""
    Zx, _ = _forward(model, xs)
    Zb, _ = _forward(model, bs)
    lo = np.inf
    for zx, zb in zip(Zx, Zb):
        d = np.abs(zx[:, None, :] - zb[None, :, :])
        d = d[d > 0]
        if d.size:
            lo = min(lo, float(d.min()))
    return lo


def condition(model, xs: np.ndarray, bs: np.ndarray, first: int = 7, tries: int = 64) -> int:
    """Seed the weights with the first seed from ``first`` on for which no
    (pair, hidden unit) has 0 < |zx - zb| < 1e-6 (with millions of them a
    given seed leaves one or two that close); returns the seed."""
    for seed in range(first, first + tries):
        seed_weights(model, seed)
        if min_gap(model, xs, bs) >= 1e-6:
            return seed
    raise AssertionError(f"no seed in {first} .. {first + tries - 1} keeps every |zx - zb| above 1e-6")


def oracle(model, xs: np.ndarray, bs: np.ndarray):
    """(phi [n][nb][C], margin of xs [n], margin of bs [nb]) in float64."""
    W, _ = _weights(model)
    f, df = _F[model.act]
    L = len(W) - 1
    binomial = model.category == ModelCategory.BINOMIAL
    w_out = W[L][1] - W[L][0] if binomial else W[L][0]
    scale = 1.0 if binomial else float(model.y_sd)
    Zx, mx = _forward(model, xs)
    Zb, mb = _forward(model, bs)
    _, grp = groups(model)
    n, nb = xs.shape[0], bs.shape[0]
    phi = np.zeros((n, nb, len(grp)))
    for i in range(n):
        for j in range(nb):
            g = w_out
            for l in range(L - 1, -1, -1):
                a, b = Zx[l][i], Zb[l][j]
                d = a - b
                tie = d == 0
                r = np.where(tie, df(a), (f(a) - f(b)) / np.where(tie, 1.0, d))
                g = (g * r) @ W[l]
            col = scale * g * (xs[i] - bs[j])
            for c, js in enumerate(grp):
                phi[i, j, c] = sum(col[k] for k in js)
    return phi, mx, mb


def stack(frame: Frame, cols) -> np.ndarray:
    return torch.stack([frame.vec(c).data for c in cols]).cpu().numpy().astype(np.float64)
