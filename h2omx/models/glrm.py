"""Generalized Low Rank Model (H2O ``H2OGeneralizedLowRankEstimator``).

Factorises the (transformed, one-hot expanded) n×p data A ≈ X Y with X n×k
(rows, kept on the rank that owns them) and Y k×p (archetypes, replicated),
minimising the quadratic loss over the OBSERVED entries plus
``gamma_x r_x(X) + gamma_y r_y(Y)``.

Alternating minimisation, every product on the fp32 matrix cores
(ops.dense.gemm, feature-major A [p][n]):

* X-step (local to each rank): X = (Y Yᵀ + γx I)⁻¹ Y A;
* Y-step: Y = (X Xᵀ + γy I)⁻¹ X Aᵀ, with X Xᵀ (k×k) and X Aᵀ (k×p) summed over
  ranks in ONE all-reduce per iteration (the only communication);
* with missing entries each row (X-step) / column (Y-step) has its own
  normal equations over its observed entries: batched k×k solves of
  Y diag(m_i) Yᵀ and X diag(m_j) Xᵀ (exact masked ALS), the column systems
  all-reduced as one p×k×(k+1) tensor.  On a device frame with k ≤ 32 both
  come from ``ops.glrm`` (fp64 matrix-unit kernels, O(n p) memory, the row
  systems solved inside the kernel); CPU frames and larger k build them as
  torch expressions (:func:`als_engine`);
* ``NonNegative`` projects onto X, Y ≥ 0 after each half-step and ``L1``
  soft-thresholds (proximal step); ``Quadratic`` / ``L2`` are the ridge
  terms above; ``None`` uses γ = 0.

Stops after ``max_iterations`` or when the relative objective change drops
below ``min_step_size``.

Generalized losses.  ``loss`` (Quadratic, Absolute, Poisson, Hinge, Logistic,
Periodic) or a loss per predictor column (``loss_by_col`` /
``loss_by_col_idx``, which also serves Huber) replace the squared error of an
observed entry by ``L_j(u_ji, a_ji)``, ``u = Y^T X``.  If any column's loss is
not Quadratic the fit is alternating proximal gradient (:func:`_fit_proxgrad`):
its two sampled products come from ``ops.glrm.loss_grad_x`` / ``loss_grad_y``
on a device frame with k <= 32 (``"proxgrad-hip"``) and from
:func:`_loss_grad_torch` otherwise (``"proxgrad-torch"``); an all-Quadratic fit
takes the ALS code above, untouched.  One-hot columns of categorical
predictors keep the Quadratic loss (``multi_loss`` is ignored).

``init``: ``SVD`` (top-k right singular vectors of the Gram, scaled),
``PlusPlus`` (k-means++ row seeding), ``Random``.  Scoring a frame solves its
X with Y fixed and returns the reconstruction ``reconstr_<col>`` (H2O
``predict``); ``transform_frame`` returns X (``Arch1 … Archk``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..frame.frame import DKV, Frame, Vec
from ..backend import dense as D
from ..ops import glrm as K
from .base import Model, ModelBuilder, ModelCategory
from .glm import DesignInfo
from .pca import TRANSFORMS
from .svd import transform_params


class GLRMModel(Model):
    algo = "glrm"
    algo_full_name = "Generalized Low Rank Modeling"

    def __init__(self, builder, model_id, design, center, scale, Y, objective, iterations):
        super().__init__(builder, model_id)
        self.design, self.center, self.scale = design, center, scale
        self.Y = Y                  # [k][p] archetypes (transformed scale)
        self.objective = objective
        self.iterations = iterations
        self.representation_key = None
        self.loss_codes = None      # per expanded column (ops.glrm.LOSSES); None: every column Quadratic

    def _cols(self, dev):
        return None if self.loss_codes is None else LossCols(self.loss_codes, self.params.get("period", 1), dev)

    def _A(self, frame: Frame):
        Xraw = self.design.raw_matrix(frame)
        dev = Xraw.device
        c = torch.from_numpy(np.asarray(self.center, np.float32)).to(dev)[:, None]
        s = torch.from_numpy(np.asarray(self.scale, np.float32)).to(dev)[:, None]
        A = (Xraw - c) / s
        mask = ~torch.isnan(A)
        return torch.where(mask, A, torch.zeros_like(A)).contiguous(), mask

    def transform_frame(self, frame: Frame) -> Frame:
        """X (n×k) of a frame with the archetypes fixed (H2O ``transform_frame``)."""
        A, mask = self._A(frame)
        Xk = _solve_x(A, mask, torch.from_numpy(self.Y.astype(np.float32)).to(A.device), self.params,
                      self._cols(A.device))
        return Frame([Vec(f"Arch{i + 1}", Xk[i].float(), "real") for i in range(Xk.shape[0])])

    def predict_raw(self, frame: Frame) -> torch.Tensor:
        A, mask = self._A(frame)
        Yt = torch.from_numpy(self.Y.astype(np.float32)).to(A.device)
        Xk = _solve_x(A, mask, Yt, self.params, self._cols(A.device))
        R = _impute(D.gemm(Yt, Xk, ta=True), self.loss_codes)             # [p][n]
        s = torch.from_numpy(np.asarray(self.scale, np.float32)).to(R.device)[:, None]
        c = torch.from_numpy(np.asarray(self.center, np.float32)).to(R.device)[:, None]
        return R * s + c

    def predict(self, frame: Frame) -> Frame:
        R = self.predict_raw(frame)
        return Frame([Vec(f"reconstr_{n}", R[j].float(), "real") for j, n in enumerate(self.design.names)])

    def model_performance(self, frame=None):
        return self.training_metrics

    def archetypes(self):
        return self.Y.copy()

    def summary(self):
        return {"model_id": self.model_id, "k": int(self.Y.shape[0]), "objective": self.objective,
                "iterations": self.iterations}

    def to_json(self):
        j = super().to_json()
        out = j["output"]
        out["archetypes"] = {"names": self.design.names, "data": self.Y.tolist()}
        out["objective"] = self.objective
        out["iterations"] = self.iterations
        out["representation_name"] = self.representation_key
        return j


def _prox(M: torch.Tensor, reg: str, gamma: float, step=1.0):
    """``step``: the gradient step in front of the regulariser (proximal gradient), a float or a 0-d tensor."""
    reg = reg.lower()
    if reg == "nonnegative":
        return M.clamp_min(0.0)
    if reg == "l1" and gamma > 0:
        return torch.sign(M) * (M.abs() - gamma * step).clamp_min(0.0)
    return M


def _ridge(reg: str, gamma: float) -> float:
    return gamma if reg.lower() in ("quadratic", "l2") else 0.0


# ------------------------------------------------------------ generalized losses

_LOSS_NAMES = {name.lower(): name for name in K.LOSSES}
_Q, _ABS, _HUB, _POI, _HIN, _LOG, _PER = (K.LOSSES[n] for n in ("Quadratic", "Absolute", "Huber", "Poisson", "Hinge",
                                                                 "Logistic", "Periodic"))


def _loss_name(name) -> str:
    got = _LOSS_NAMES.get(str(name).lower())
    if got is None:
        raise ValueError(f"glrm: unknown loss {name!r} ({', '.join(K.LOSSES)})")
    return got


def column_losses(p_, design) -> list[str]:
    """The loss name of every predictor column (``design.x`` order): ``loss`` unless
    ``loss_by_col`` names another, at ``loss_by_col_idx`` or in order."""
    per = [_loss_name(p_["loss"])] * len(design.x)
    by, idx = p_.get("loss_by_col"), p_.get("loss_by_col_idx")
    if by:
        names = [_loss_name(n) for n in by]
        if idx is None:
            if len(names) != len(per):
                raise ValueError(f"glrm: loss_by_col has {len(names)} entries for {len(per)} predictors; "
                                 "give loss_by_col_idx")
            idx = range(len(per))
        if len(list(idx)) != len(names):
            raise ValueError("glrm: loss_by_col and loss_by_col_idx differ in length")
        for i, nm in zip(idx, names):
            if not 0 <= int(i) < len(per):
                raise ValueError(f"glrm: loss_by_col_idx {i} outside the {len(per)} predictors")
            per[int(i)] = nm
    elif idx is not None:
        raise ValueError("glrm: loss_by_col_idx without loss_by_col")
    return per


def expanded_codes(losses, design) -> np.ndarray:
    """One code per expanded column; the one-hot columns of a categorical keep Quadratic."""
    per = dict(zip(design.x, losses))
    return np.asarray([_Q if lvl is not None else K.LOSSES[per[c]] for c, lvl in design.spec], np.int32)


class LossCols:
    """The per-column losses of a fit: codes and parameters (Periodic: 2 pi / period)
    on the host, and on a device as ``ops.glrm`` reads them."""

    def __init__(self, codes, period, dev):
        self.codes = np.asarray(codes, np.int32)
        if (self.codes == _PER).any() and not float(period) > 0:
            raise ValueError(f"glrm: period={period!r} must be positive")
        self.pars = np.where(self.codes == _PER, 2.0 * math.pi / float(period) if float(period) > 0 else 0.0, 0.0)
        self.quadratic = not self.codes.any()
        self.dev = K.loss_columns(self.codes, self.pars, dev) if torch.device(dev).type == "cuda" else None


def loss_engine(A: torch.Tensor, k: int) -> str:
    """Who forms the two sampled products of proximal gradient: ``ops.glrm`` or torch."""
    return "proxgrad-hip" if A.is_cuda and k <= K.MAX_K else "proxgrad-torch"


def _loss_planes(U: torch.Tensor, A: torch.Tensor, codes: np.ndarray, pars: np.ndarray):
    """L(u, a) and dL/du of every entry, [p][n] fp64, row j under the loss ``codes[j]``."""
    L, G = torch.empty_like(U), torch.empty_like(U)
    for c in np.unique(codes):
        rows = torch.from_numpy(np.nonzero(codes == c)[0]).to(U.device)
        u, a = U[rows], A[rows]
        x = u - a
        if c == _Q:
            l, g = x * x, 2.0 * x
        elif c == _ABS:
            l, g = x.abs(), torch.sign(x)
        elif c == _HUB:
            l, g = torch.where(x.abs() <= 1.0, 0.5 * x * x, x.abs() - 0.5), x.clamp(-1.0, 1.0)
        elif c == _POI:
            e = torch.exp(u)
            l, g = e - a * u + torch.xlogy(a, a) - a, e - a
        elif c == _HIN:
            s = 2.0 * a - 1.0
            t = 1.0 - s * u
            l, g = t.clamp_min(0.0), torch.where(t > 0, -s, torch.zeros_like(s))
        elif c == _LOG:
            s = 2.0 * a - 1.0
            z = s * u
            e = torch.exp(-z.abs())
            l, g = (-z).clamp_min(0.0) + torch.log1p(e), -s * torch.where(z < 0, torch.ones_like(e), e) / (1.0 + e)
        else:
            w = torch.from_numpy(pars[codes == c]).to(U.device)[:, None]
            l, g = 1.0 - torch.cos(w * x), w * torch.sin(w * x)
        L[rows], G[rows] = l, g
    return L, G


def _loss_grad_torch(A, mask, X, Y, codes: np.ndarray, pars: np.ndarray, wrt: str):
    """The tensor route of ``ops.glrm.loss_grad_x`` (``wrt="x"``) / ``loss_grad_y`` (``"y"``):
    fp64, materialises the [p][n] reconstruction and derivative planes."""
    Xd, Yd = X.double(), Y.double()
    L, G = _loss_planes(Yd.T @ Xd, A.double(), codes, pars)
    G = torch.where(mask, G, torch.zeros_like(G))
    obj = torch.where(mask, L, torch.zeros_like(L)).sum()
    return (Yd @ G if wrt == "x" else Xd @ G.T), obj


def _loss_grad(A, mask, X, Y, cols: LossCols, wrt: str):
    if loss_engine(A, X.shape[0]) == "proxgrad-hip":
        return (K.loss_grad_x if wrt == "x" else K.loss_grad_y)(A, mask, X, Y, *cols.dev)
    return _loss_grad_torch(A, mask, X, Y, cols.codes, cols.pars, wrt)


def _reg_value(M: torch.Tensor, reg: str, gamma: float) -> torch.Tensor:
    if reg.lower() == "l1":
        return M.double().abs().sum() * gamma
    return M.double().pow(2).sum() * _ridge(reg, gamma)


def _prox_step(M: torch.Tensor, G: torch.Tensor, step, reg: str, gamma: float) -> torch.Tensor:
    """``prox_{step r}(M - step G)`` in fp64, stored fp32: Quadratic / L2 in closed form
    (division by ``1 + 2 step gamma``), L1 by soft threshold, NonNegative by projection."""
    V = M.double() - step * G
    if _ridge(reg, gamma) > 0:
        V = V / (1.0 + 2.0 * step * gamma)
    return _prox(V, reg, gamma, step).float().contiguous()


def _step(alpha: float, other: torch.Tensor):
    """alpha over the squared Frobenius norm of the other factor, which bounds its
    largest squared singular value: at alpha = 1 the step is within 2 / Lipschitz for
    every loss with |L''| <= 2 (Quadratic, Huber, Logistic, Periodic up to w^2 <= 2)."""
    return alpha / (other.clamp_min(1e-12) if torch.is_tensor(other) else max(float(other), 1e-12))


def _impute(U: torch.Tensor, codes) -> torch.Tensor:
    """H2O's impute per column: u itself, exp(u) for Poisson, u > 0 as 0 / 1 for Logistic and Hinge."""
    if codes is None:
        return U
    codes = np.asarray(codes)
    poi, binary = np.nonzero(codes == _POI)[0], np.nonzero((codes == _LOG) | (codes == _HIN))[0]
    if poi.size:
        U[torch.from_numpy(poi).to(U.device)] = torch.exp(U[torch.from_numpy(poi).to(U.device)])
    if binary.size:
        U[torch.from_numpy(binary).to(U.device)] = (U[torch.from_numpy(binary).to(U.device)] > 0).to(U.dtype)
    return U


def _solve_x_proxgrad(A, mask, Y, p_, cols: LossCols) -> torch.Tensor:
    """X [k][n] by the X half-steps of proximal gradient alone, Y fixed, from X = 0, with
    the accept / halve rule of the fit.  Rows are independent, so no communication."""
    rx, gx = str(p_["regularization_x"]), float(p_["gamma_x"])
    alpha, tol = float(p_.get("init_step_size", 1.0)), float(p_.get("min_step_size", 1e-4))
    ynorm = Y.double().pow(2).sum()
    X = torch.zeros((Y.shape[0], A.shape[1]), dtype=torch.float32, device=A.device)
    gX, loss = _loss_grad(A, mask, X, Y, cols, "x")
    obj = float(loss + _reg_value(X, rx, gx))
    for _ in range(int(p_.get("max_iterations", 1000))):
        Xn = _prox_step(X, gX, _step(alpha, ynorm), rx, gx)
        gn, loss = _loss_grad(A, mask, Xn, Y, cols, "x")
        objn = float(loss + _reg_value(Xn, rx, gx))
        if math.isfinite(objn) and objn < obj:
            rel = (obj - objn) / max(abs(obj), 1e-12)
            X, gX, obj = Xn, gn, objn
            alpha *= 1.05
            if rel < tol:
                break
        else:
            alpha *= 0.5
            if alpha < tol:
                break
    return X


def als_engine(A: torch.Tensor, k: int) -> str:
    """Who builds the masked normal equations: the ``ops.glrm`` kernels or torch."""
    return "hip" if A.is_cuda and k <= K.MAX_K else "torch"


def _solve_x_torch(A: torch.Tensor, mask: torch.Tensor, Y: torch.Tensor, lam: float) -> torch.Tensor:
    """Per-row normal equations over the observed columns, G_i = Y diag(m_i) Y^T, in chunks of rows."""
    k = Y.shape[0]
    m = mask.float()
    out = torch.empty((k, A.shape[1]), dtype=torch.float32, device=A.device)
    eye = lam * torch.eye(k, dtype=torch.float64, device=A.device)
    for s0 in range(0, A.shape[1], 1 << 16):
        s1 = min(A.shape[1], s0 + (1 << 16))
        mb = m[:, s0:s1]
        G = torch.einsum("jn,aj,bj->nab", mb, Y, Y).double() + eye
        r = (Y @ (A[:, s0:s1] * mb)).T.double()                           # [n][k]
        out[:, s0:s1] = torch.linalg.solve(G, r.unsqueeze(-1)).squeeze(-1).T.float()
    return out


def _solve_x(A: torch.Tensor, mask: torch.Tensor, Y: torch.Tensor, p_, cols: "LossCols | None" = None) -> torch.Tensor:
    """X [k][n] minimising the masked loss (+ x regulariser) with Y fixed: the normal
    equations when every column's loss is Quadratic, else :func:`_solve_x_proxgrad`."""
    if cols is not None and not cols.quadratic:
        return _solve_x_proxgrad(A, mask, Y, p_, cols)
    k = Y.shape[0]
    rx, gx = str(p_["regularization_x"]), float(p_["gamma_x"])
    lam = _ridge(rx, gx) + 1e-8
    if bool(mask.all()):
        Gy = D.gemm(Y, Y, tb=True).double() + lam * torch.eye(k, dtype=torch.float64, device=Y.device)
        return _prox(torch.linalg.inv(Gy.cpu()).to(Y.device, torch.float32) @ D.gemm(Y, A), rx, gx)
    if als_engine(A, k) == "hip":
        out, bad = K.masked_x(A, mask, Y, lam)
        if bad > 0:             # a singular row system: whatever the torch route makes of it
            out = _solve_x_torch(A, mask, Y, lam)
    else:
        out = _solve_x_torch(A, mask, Y, lam)
    return _prox(out, rx, gx)


def _solve_y_terms_torch(A: torch.Tensor, mask: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """S [p][k][k + 1] fp64, S[j] = [X diag(m_j) X^T | X (a_j m_j)]."""
    m = mask.float()
    G = torch.einsum("jn,an,bn->jab", m, X, X).double()                    # [p][k][k]
    r = (X @ (A * m).T).T.double()                                         # [p][k]
    return torch.cat([G, r.unsqueeze(-1)], -1)


def _solve_y(A: torch.Tensor, mask: torch.Tensor, X: torch.Tensor, p_, comm, full: bool) -> torch.Tensor:
    """Y [k][p] with X fixed; one all-reduce of the (summed) normal equations.
    ``full`` (no missing entry on ANY rank) must agree across ranks."""
    k = X.shape[0]
    ry, gy = str(p_["regularization_y"]), float(p_["gamma_y"])
    lam = _ridge(ry, gy) + 1e-8
    world = comm.world_size if comm is not None else 1
    dev = A.device
    if full:
        S = torch.cat([D.gemm(X, X, tb=True), D.gemm(X, A, tb=True)], 1).double()
        if world > 1:
            comm.all_reduce_(S)
        Gx = S[:, :k] + lam * torch.eye(k, dtype=torch.float64, device=dev)
        return _prox(torch.linalg.solve(Gx.cpu(), S[:, k:].cpu()).to(dev, torch.float32), ry, gy)
    S = K.masked_y_terms(A, mask, X) if als_engine(A, k) == "hip" else _solve_y_terms_torch(A, mask, X)
    if world > 1:
        comm.all_reduce_(S)
    G = S[..., :k] + lam * torch.eye(k, dtype=torch.float64, device=dev)
    Y = torch.linalg.solve(G, S[..., k:]).squeeze(-1).T                    # [k][p]
    return _prox(Y.float().contiguous(), ry, gy)


class H2OGeneralizedLowRankEstimator(ModelBuilder):
    algo = "glrm"
    UNSUPERVISED_CATEGORY = ModelCategory.DIMREDUCTION
    DEFAULTS = dict(k=1, transform="NONE", loss="Quadratic", multi_loss="Categorical", regularization_x="None",
                    regularization_y="None", gamma_x=0.0, gamma_y=0.0, max_iterations=1000, max_updates=2000,
                    init_step_size=1.0, min_step_size=1e-4, init="PlusPlus", svd_method="Randomized",
                    user_y=None, user_x=None, expand_user_y=True, impute_original=False, recover_svd=False,
                    representation_name=None, period=1, max_runtime_secs=0.0, loss_by_col=None,
                    loss_by_col_idx=None)

    def train(self, x=None, y=None, training_frame=None, validation_frame=None, comm=None, **kw):
        return super().train(x=x, y=None, training_frame=training_frame, validation_frame=validation_frame,
                             comm=comm, **kw)

    def _fit(self, train: Frame, valid, model_id):
        p_ = self.params
        if _loss_name(p_["loss"]) == "Huber":
            raise ValueError("glrm: loss='Huber' is not accepted as the scalar loss; name it per column through "
                             "loss_by_col, which serves it")
        tr = str(p_["transform"]).upper()
        if tr not in TRANSFORMS:
            raise ValueError(f"glrm: unknown transform {p_['transform']!r}")
        for r in ("regularization_x", "regularization_y"):
            if str(p_[r]).lower() not in ("none", "quadratic", "l2", "l1", "nonnegative"):
                raise ValueError(f"glrm: {r}={p_[r]!r} (None, Quadratic, L2, L1, NonNegative)")
        comm = self.comm
        world = comm.world_size if comm is not None else 1
        design = DesignInfo(self.x, self.feature_types, self.feature_domains, use_all_levels=True)
        Xraw = design.raw_matrix(train)
        design.fit_standardization(Xraw, True, comm)
        center, scale = transform_params(design, Xraw, tr, comm)
        del Xraw
        model = GLRMModel(self, model_id, design, center, scale, np.zeros((1, 1)), float("nan"), 0)
        A, mask = model._A(train)
        p, n = A.shape
        k = int(p_["k"])
        if not 1 <= k <= p:
            raise ValueError(f"glrm: k={k} must be in [1, {p}]")
        dev = A.device
        seed = self._seed()
        g = torch.Generator().manual_seed(seed)
        # missing entries start at the column means (0 on the transformed scale when demeaned)
        colmean = (A.double().sum(1) / mask.double().sum(1).clamp_min(1))
        cm = torch.stack([A.double().sum(1), mask.double().sum(1)])
        if world > 1:
            comm.all_reduce_(cm)
        colmean = (cm[0] / cm[1].clamp_min(1)).float()
        Af = torch.where(mask, A, colmean[:, None].expand_as(A)).contiguous()
        Y = self._init_y(Af, k, str(p_["init"]), g, comm).to(dev)
        rx, ry = str(p_["regularization_x"]), str(p_["regularization_y"])
        gx, gy = float(p_["gamma_x"]), float(p_["gamma_y"])
        nobs = mask.double().sum()
        anymiss = torch.tensor([0.0 if bool(mask.all()) else 1.0], dtype=torch.float64, device=dev)
        if world > 1:
            comm.all_reduce_(anymiss, "max")
        full = float(anymiss) == 0.0
        if world > 1:
            comm.all_reduce_(nobs)
        losses = column_losses(p_, design)
        cols = LossCols(expanded_codes(losses, design), p_["period"], dev)
        if not cols.quadratic:
            return self._fit_proxgrad(model, A, mask, Y, cols, float(nobs))
        prev = math.inf
        obj = math.inf
        it = 0
        X = None
        hist = []
        for it in range(1, int(p_["max_iterations"]) + 1):
            X = _solve_x(A, mask, Y, p_)                                   # rows are local
            Y = _solve_y(A, mask, X, p_, comm, full)
            R = D.gemm(Y, X, ta=True)                                     # reconstruction [p][n]
            err = torch.where(mask, A - R, torch.zeros_like(R)).double().pow(2).sum()
            regx = (X.double().pow(2).sum() * _ridge(rx, gx) + (X.double().abs().sum() * gx if rx.lower() == "l1"
                                                                 else 0.0))
            parts = torch.stack([err, torch.as_tensor(regx, dtype=torch.float64, device=dev)])
            if world > 1:
                comm.all_reduce_(parts)
            regy = float(Y.double().pow(2).sum()) * _ridge(ry, gy) + (float(Y.double().abs().sum()) * gy
                                                                      if ry.lower() == "l1" else 0.0)
            obj = float(parts[0] + parts[1]) + regy
            hist.append({"iterations": it, "objective": obj})
            if abs(prev - obj) <= float(p_["min_step_size"]) * max(abs(prev), 1e-12):
                break
            prev = obj
        model = GLRMModel(self, model_id, design, center, scale, Y.double().cpu().numpy(), obj, it)
        model.scoring_history = hist
        model.training_metrics = {"objective": obj, "iterations": it, "numerr": float(parts[0]),
                                  "nobs": float(nobs), "caterr": 0.0}
        model.timings["als_engine"] = "gemm" if full else als_engine(A, k)
        rep = Frame([Vec(f"Arch{i + 1}", X[i].float(), "real") for i in range(k)],
                    key=p_["representation_name"] or None)
        DKV.put(rep.key, rep)
        model.representation_key = rep.key
        model.representation = rep
        return model

    def _check_loss_data(self, A, mask, cols: LossCols, names):
        """Logistic / Hinge columns hold 0 / 1, Poisson columns no negative value (observed,
        transformed scale); every rank raises alike."""
        binary = torch.from_numpy((cols.codes == _LOG) | (cols.codes == _HIN)).to(A.device)[:, None]
        poisson = torch.from_numpy(cols.codes == _POI).to(A.device)[:, None]
        bad = torch.stack([(mask & binary & (A != 0) & (A != 1)).any(1), (mask & poisson & (A < 0)).any(1)]).double()
        if self.comm is not None and self.comm.world_size > 1:
            self.comm.all_reduce_(bad, "max")
        bad = bad.cpu().numpy() > 0
        for j in np.nonzero(bad[0])[0]:
            raise ValueError(f"glrm: column {names[j]!r} has a Logistic or Hinge loss but observed values "
                             "(after the transform) outside {0, 1}")
        for j in np.nonzero(bad[1])[0]:
            raise ValueError(f"glrm: column {names[j]!r} has a Poisson loss but negative observed values "
                             "(after the transform)")

    def _fit_proxgrad(self, proto: GLRMModel, A, mask, Y, cols: LossCols, nobs: float):
        """Alternating proximal gradient on ``sum m L + gamma_x r_x(X) + gamma_y r_y(Y)``.

        One update: gradX and the loss at the candidate (X, Y); X' = prox(X - step_x gradX);
        gradY at (X', Y); one all-reduce carries gradY, the candidate's loss and x
        regulariser, and |X'|_F^2.  The candidate is then accepted (its objective is
        below the last accepted one: alpha grows by 5 %) or rejected (back to the
        accepted point and its gradient, alpha halved, gradY formed again), and
        Y' = prox(Y - step_y gradY) gives the next candidate (X', Y').  ``step_x`` =
        alpha / |Y|_F^2 and ``step_y`` = alpha / |X'|_F^2 (:func:`_step`).  X starts at the
        Quadratic X-step of the initial Y, or at 0 if the loss is not finite there."""
        p_, comm = self.params, self.comm
        world = comm.world_size if comm is not None else 1
        rx, ry = str(p_["regularization_x"]), str(p_["regularization_y"])
        gx, gy = float(p_["gamma_x"]), float(p_["gamma_y"])
        tol, max_it, max_up = float(p_["min_step_size"]), int(p_["max_iterations"]), int(p_["max_updates"])
        self._check_loss_data(A, mask, cols, proto.design.names)
        k, p = Y.shape
        Y = Y.float().contiguous()
        X = _solve_x(A, mask, Y, p_)
        alpha = float(p_["init_step_size"])
        good, hist, updates = None, [], 0          # good: the accepted (X, Y, gradX, objective, loss)

        def y_pass(Xc, Xn, Yc, loss):
            gY, _ = _loss_grad(A, mask, Xn, Yc, cols, "y")
            tail = torch.stack([loss, _reg_value(Xc, rx, gx), Xn.double().pow(2).sum()])
            pack = torch.cat([gY.reshape(-1), tail])
            if world > 1:
                comm.all_reduce_(pack)
            return pack[:k * p].reshape(k, p), pack[k * p:].cpu().numpy()

        while len(hist) < max_it and updates < max_up and alpha >= tol:
            updates += 1
            gX, loss = _loss_grad(A, mask, X, Y, cols, "x")
            Xn = _prox_step(X, gX, _step(alpha, Y.double().pow(2).sum()), rx, gx)
            gY, (lsum, regx, xnorm) = y_pass(X, Xn, Y, loss)
            obj = float(lsum + regx + float(_reg_value(Y, ry, gy)))
            if good is None and not math.isfinite(obj) and bool(X.any()):
                X = torch.zeros_like(X)             # the Quadratic start overflows this loss
                continue
            if math.isfinite(obj) and (good is None or obj < good[3]):
                rel = math.inf if good is None else (good[3] - obj) / max(abs(good[3]), 1e-12)
                good = (X, Y, gX, obj, float(lsum))
                hist.append({"iterations": len(hist) + 1, "objective": obj, "step_size": alpha})
                if rel < tol:
                    break
                alpha *= 1.05
            else:
                if good is None:
                    raise ValueError("glrm: the loss is not finite at the initial factors")
                alpha *= 0.5
                if alpha < tol:
                    break
                X, Y, gX = good[:3]
                Xn = _prox_step(X, gX, _step(alpha, Y.double().pow(2).sum()), rx, gx)
                gY, (_, _, xnorm) = y_pass(X, Xn, Y, loss)
            Y = _prox_step(Y, gY, _step(alpha, xnorm), ry, gy)
            X = Xn
        if good is None:
            raise ValueError("glrm: no iteration ran (max_iterations, max_updates, init_step_size)")
        X, Y, _, obj, lsum = good
        model = GLRMModel(self, proto.model_id, proto.design, proto.center, proto.scale, Y.double().cpu().numpy(), obj,
                          len(hist))
        model.loss_codes = cols.codes
        model.scoring_history = hist
        model.training_metrics = {"objective": obj, "iterations": len(hist), "numerr": lsum, "nobs": nobs,
                                  "caterr": 0.0}
        model.timings["als_engine"] = loss_engine(A, k)
        model.timings["updates"] = updates
        rep = Frame([Vec(f"Arch{i + 1}", X[i].float(), "real") for i in range(k)],
                    key=p_["representation_name"] or None)
        DKV.put(rep.key, rep)
        model.representation_key = rep.key
        model.representation = rep
        return model

    def _init_y(self, Af: torch.Tensor, k: int, init: str, g, comm) -> torch.Tensor:
        p, n = Af.shape
        world = comm.world_size if comm is not None else 1
        init = init.lower()
        if init == "svd":
            G = D.gemm(Af, Af, tb=True).double()
            if world > 1:
                comm.all_reduce_(G)
            w, V = np.linalg.eigh(G.cpu().numpy())
            order = np.argsort(w)[::-1][:k]
            nrows = float(n) * world
            Y = (V[:, order] * np.sqrt(np.maximum(w[order], 0) / max(nrows, 1.0))).T
            return torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32))
        if init == "random":
            return torch.randn((k, p), generator=g)
        if init in ("plusplus", "user"):
            # k-means++ seeding over a sample of the rank's rows, gathered to every rank
            m = min(n, 20000)
            idx = torch.randperm(n, generator=g)[:m].to(Af.device)
            S = Af[:, idx].T.contiguous().float()                        # [m][p]
            if world > 1:
                S = comm.all_gather_cat(S)
            S = S.cpu()
            rows = [int(torch.randint(0, S.shape[0], (1,), generator=g))]
            d2 = ((S - S[rows[0]]) ** 2).sum(1)
            for _ in range(1, k):
                pr = d2 / d2.sum().clamp_min(1e-30)
                j = int(torch.multinomial(pr, 1, generator=g)) if float(d2.sum()) > 0 else int(
                    torch.randint(0, S.shape[0], (1,), generator=g))
                rows.append(j)
                d2 = torch.minimum(d2, ((S - S[j]) ** 2).sum(1))
            return S[rows].contiguous()
        raise ValueError(f"glrm: init {init!r} (SVD, PlusPlus, Random)")
