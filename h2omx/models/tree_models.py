"""GBM, XGBoost and DRF estimators on the shared histogram tree engine.

Parameter names and defaults follow H2O-3's GBM / XGBoost / DRF model
builders (the algorithms the reference's h2o.jar image serves; SURVEY.md
§2.7).  Differences that come from the MI355X design are documented in
docs/ALGORITHMS.md: features are binned once into <= 255 global quantile
bins (``nbins``; H2O re-bins adaptively per node), categorical levels are
binned as ordinal codes, and trees grow level-wise entirely on the GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..frame.frame import ENUM, Frame, Vec
from .base import Model, ModelBuilder, ModelCategory
from .tree import TreeParams, bin_matrix, compute_edges, train_ensemble
from .tree.binning import PER_NODE_MODES, adaptive_ranges, categorical_bins, resolve_histogram_type
from .tree.boost import concat_catbits, concat_trees


class TreeModel(Model):
    algo = "tree"

    def __init__(self, builder, model_id, ens, dist):
        super().__init__(builder, model_id)
        self.ens = ens
        self.dist = dist

    def _link(self, margin: torch.Tensor) -> torch.Tensor:
        cat = self.category
        if self.dist == "drf":
            if cat == ModelCategory.BINOMIAL:
                p1 = margin[0].clamp(0, 1)
                return torch.stack([1 - p1, p1])
            if cat == ModelCategory.MULTINOMIAL:
                m = margin.clamp_min(0)
                s = m.sum(0, keepdim=True)
                return torch.where(s > 0, m / s.clamp_min(1e-30), torch.full_like(m, 1.0 / m.shape[0]))
            return margin
        if cat == ModelCategory.BINOMIAL:
            p1 = torch.sigmoid(margin[0])
            return torch.stack([1 - p1, p1])
        if cat == ModelCategory.MULTINOMIAL:
            return torch.softmax(margin, dim=0)
        if self.dist in ("poisson", "gamma", "tweedie"):
            return torch.exp(margin)
        return margin

    def predict_raw(self, frame: Frame) -> torch.Tensor:
        X = frame.feature_matrix(self.x)
        dev = X.device
        m = self.ens.raw_margin(X)
        off = frame.vec(self.params["offset_column"]).as_float() if self.params.get("offset_column") else None
        return self.scores_from_margin(m, off, dev)

    def scores_from_margin(self, m: torch.Tensor, offset: torch.Tensor | None = None, dev=None) -> torch.Tensor:
        """The tail of ``predict_raw``: margins [K][n] of the ensemble (plus the
        rows' ``offset``) through the link and the class-balance correction."""
        if offset is not None:
            m = m + offset[None, :].to(m.device)
        P = self._link(m if dev is None else m.to(dev))
        cd = getattr(self, "class_dist", None)
        return P if cd is None else correct_probabilities(P, *cd)

    def predict(self, frame: Frame) -> Frame:
        fr = super().predict(frame)
        cal = getattr(self, "calibration", None)
        if cal is None:
            return fr
        p1 = fr.vec(self.response_domain[1]).data.double()
        c1 = _apply_calibration(cal, p1).float()
        return Frame(list(fr.vecs) + [Vec("cal_p0", 1.0 - c1, "real"), Vec("cal_p1", c1, "real")])

    def varimp(self):
        gains = np.zeros(len(self.x))
        for t in range(self.ens.trees.shape[0]):
            tr = self.ens.trees[t]
            for i in _reachable(tr):
                if tr[i]["feat"] >= 0:
                    gains[tr[i]["feat"]] += max(float(tr[i]["gain"]), 0.0)
        if gains.max() <= 0:
            return [(c, 0.0, 0.0, 0.0) for c in self.x]
        order = np.argsort(-gains, kind="stable")
        mx, tot = gains.max(), gains.sum()
        return [(self.x[i], float(gains[i]), float(gains[i] / mx), float(gains[i] / tot)) for i in order]

    def summary(self):
        depths, leaves = [], []
        for t in range(self.ens.trees.shape[0]):
            nodes = _reachable(self.ens.trees[t])
            lv = [i for i in nodes if self.ens.trees[t][i]["feat"] < 0]
            leaves.append(len(lv))
            depths.append(int(math.floor(math.log2(max(nodes) + 1))) if nodes else 0)
        return {"model_id": self.model_id, "algo": self.algo, "number_of_trees": int(self.ens.trees.shape[0]),
                "number_of_internal_trees": int(self.ens.trees.shape[0]),
                "min_depth": int(min(depths) if depths else 0), "max_depth": int(max(depths) if depths else 0),
                "mean_depth": float(np.mean(depths)) if depths else 0.0,
                "min_leaves": int(min(leaves) if leaves else 0), "max_leaves": int(max(leaves) if leaves else 0),
                "mean_leaves": float(np.mean(leaves)) if leaves else 0.0}


def _reachable(tr):
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        out.append(i)
        if tr[i]["feat"] >= 0:
            stack += [int(tr[i]["left"]), int(tr[i]["left"]) + 1]
    return out


class _TreeBuilder(ModelBuilder):
    model_cls = TreeModel
    mode = 0
    default_nbins = 255
    # histogram_type AUTO and the per-node rules (H2O GBM / DRF: AUTO =
    # UniformAdaptive re-binned per node; XGBoost 'hist' bins globally)
    auto_histogram = "quantilesglobal"
    per_node_histograms = False
    # fine-grid cap of the per-node rules for trees deeper than deep_depth
    deep_depth = 12
    deep_fine_bins = 63

    def _warn(self, msg: str, loud: bool = True) -> None:
        """A deviation from H2O's semantics, surfaced in the model output
        (``output.warnings``, H2O's model warnings) and, for a value the user
        set, as a Python warning."""
        import warnings

        self._warnings.append(msg)
        if loud:
            warnings.warn(f"h2omx {self.algo}: {msg}", stacklevel=3)

    def _dist(self) -> str:
        d = str(self.params.get("distribution", "AUTO")).lower()
        if d in ("auto", ""):
            return {ModelCategory.BINOMIAL: "bernoulli", ModelCategory.MULTINOMIAL: "multinomial"}.get(
                self.category, "gaussian")
        return d

    def _tree_params(self, nfeat: int) -> TreeParams:
        raise NotImplementedError

    # categorical group splits for enum predictors (GBM / DRF under
    # categorical_encoding AUTO / Enum; H2O's XGBoost one-hot encodes instead)
    group_splits = True

    def _group_splits(self, enc: str) -> bool:
        return self.group_splits and enc in ("auto", "enum", "enumlimited")

    # SortByResponse is applied by the tree builder itself (_sort_levels_by_response)
    NATIVE_ENCODINGS = ("auto", "enum", "sortbyresponse")

    def _encoding_scheme(self) -> str:
        s = super()._encoding_scheme()
        if s == "onehotinternal":
            raise ValueError(f"{self.algo}: categorical_encoding OneHotInternal is not supported by tree algorithms "
                             "(as in H2O); use OneHotExplicit")
        return s

    def _monotone(self):
        """H2O ``monotone_constraints`` ({column: +1 / -1}, or the REST form
        [{"key": column, "value": sign}]) as one sign per predictor; None if
        unconstrained.  Numeric predictors only; not for multinomial models
        (hex/tree/gbm/GBMModel.java monotone checks)."""
        mc = self.params.get("monotone_constraints")
        if not mc:
            return None
        if isinstance(mc, dict):
            items = list(mc.items())
        else:
            items = [(e["key"], e["value"]) if isinstance(e, dict) else tuple(e) for e in mc]
        signs = [0] * len(self.x)
        for col, v in items:
            if col not in self.x:
                raise ValueError(f"monotone_constraints: column {col!r} is not a predictor")
            if self.feature_types.get(col) == ENUM:
                raise ValueError(f"monotone_constraints: column {col!r} is categorical (numeric columns only)")
            v = int(float(v))
            if v not in (-1, 0, 1):
                raise ValueError(f"monotone_constraints: {col!r} must be -1, 0 or 1, got {v}")
            signs[self.x.index(col)] = v
        if not any(signs):
            return None
        if self.category == ModelCategory.MULTINOMIAL:
            raise ValueError("monotone_constraints are not supported for multinomial models")
        return tuple(signs)

    def _interactions(self):
        """H2O ``interaction_constraints`` (a list of lists of column names whose
        columns may appear together on a root path) as feature-index tuples;
        None if unset.  Columns outside every list only combine with
        themselves (hex/tree/GlobalInteractionConstraints)."""
        ic = self.params.get("interaction_constraints")
        if not ic:
            return None
        sets = []
        for grp in ic:
            idx = []
            for col in ([grp] if isinstance(grp, str) else grp):
                if col not in self.x:
                    raise ValueError(f"interaction_constraints: column {col!r} is not a predictor")
                idx.append(self.x.index(col))
            sets.append(tuple(sorted(set(idx))))
        return tuple(sets)

    def _fit(self, train: Frame, valid: Frame | None, model_id: str) -> Model:
        enc = self._encoding_scheme()
        if enc == "sortbyresponse":
            train, valid = self._sort_levels_by_response(train, valid)
        X = train.feature_matrix(self.x)
        dist = self._dist()
        yv = train.vec(self.y)
        if self.category == ModelCategory.REGRESSION:
            y = yv.as_float()
        else:
            y = yv.data.float()
        w = train.vec(self.params["weights_column"]).as_float() if self.params.get("weights_column") else None
        ok = (y >= 0) if self.category != ModelCategory.REGRESSION else ~torch.isnan(y)
        if not bool(ok.all()):
            X, y = X[:, ok], y[ok]
            w = None if w is None else w[ok]
        balance = None
        if self.params.get("balance_classes") and self.category in (ModelCategory.BINOMIAL,
                                                                     ModelCategory.MULTINOMIAL):
            w, balance = _balance_weights(y, w, len(self.response_domain), self.params, self.comm)
        nbins = int(self.params.get("nbins") or self.params.get("max_bins") or self.default_nbins)
        htype = resolve_histogram_type(self.params.get("histogram_type"), auto=self.auto_histogram)
        top = int(self.params.get("nbins_top_level") or 1024)
        per_node = self.per_node_histograms and htype in PER_NODE_MODES
        self._warnings = []
        if per_node:
            # H2O's per-node rules on fine quantile bins (root resolution
            # nbins_top_level, at most 255: uint8 codes); every node then keeps the
            # fine edges nearest its own equal-width / random cuts (binning.py)
            fine = min(255, max(nbins, top))
            if (int(self.params.get("max_depth") or 0) > self.deep_depth and fine > self.deep_fine_bins
                    and "nbins_top_level" not in getattr(self, "_explicit_params", ())):
                # deep trees (DRF depth 20) with the default nbins_top_level: 63 fine bins
                # keep the direct levels' per-node histograms small - 10M x 100 DRF 13.7 vs
                # 19.4 ms/tree for 255, OOB AUC 0.791 vs 0.794 (profiles/r6/drf_fine255_r6bg.txt;
                # round 5: 27 vs 43 ms, profiles/r5/hist/hist_rule_ab_r5y.jsonl).  An explicit
                # nbins_top_level keeps the 255-bin grid.
                fine = self.deep_fine_bins
                self._warn(f"max_depth > {self.deep_depth} with the default nbins_top_level: per-node cut points "
                           f"snap to {fine} fine quantile bins per column (faster: on 10M x 100 13.7 vs 19.4 ms/tree, "
                           f"OOB AUC 0.791 vs 0.794 for 255 bins) - pass nbins_top_level explicitly for the "
                           f"255-bin grid")
            edges, nvb, nbt = compute_edges(X, fine, seed=self._seed(), comm=self.comm,
                                            histogram_type="QuantilesGlobal")
            if max(nbins, top) > 255 and fine == 255:
                # (H2O's defaults hit this: recorded in the model, not raised as a Python warning)
                self._warn(f"histogram_type {self.params.get('histogram_type') or 'AUTO'}: node cut points snap to "
                           f"255 fine quantile bins per column (nbins_top_level={top} finer than the uint8 codes)",
                           loud=max(nbins, top) != 1024)
        else:
            if htype in PER_NODE_MODES or htype == "uniformrobust":
                self._warn(f"histogram_type {self.params.get('histogram_type')}: {self.algo} bins every column "
                           "with one global grid (no per-node re-binning)")
            if nbins > 256:      # (XGBoost's max_bins=256 default: 255 value bins + the NA bin)
                self._warn(f"nbins={nbins} capped at 255 bins per column (uint8 codes)")
            edges, nvb, nbt = compute_edges(X, min(nbins, 255), seed=self._seed(), comm=self.comm,
                                            histogram_type=htype)
        cat = None
        if self._group_splits(enc):
            # H2O's default for enum predictors (categorical_encoding AUTO / Enum):
            # identity level bins + group splits (sets of levels) in GBM / DRF
            levels = {i: len(self.feature_domains.get(c) or []) for i, c in enumerate(self.x)
                      if self.feature_types.get(c) == ENUM}
            edges, nvb, nbt, cat = categorical_bins(edges, nvb, nbt, levels)
        bm = bin_matrix(X, edges, nvb, nbt, names=self.x, cat=cat)
        tp = self._tree_params(len(self.x))
        if per_node:
            tp.hist_mode, tp.hist_top, tp.hist_nbins = PER_NODE_MODES[htype], top, nbins
            bm.frange = adaptive_ranges(X, bm, self.comm, seed=self._seed())
        nclass = len(self.response_domain) if self.response_domain else 1
        ens_dist = self._engine_dist(dist)
        init_f = None
        offset = None
        if self.params.get("offset_column"):
            # H2O: margin = init_f + offset + trees; init_f fitted with the offset held fixed
            if ens_dist in ("drf", "multinomial"):
                raise ValueError(f"offset_column is not supported for {self.algo} / {ens_dist} (as in H2O)")
            offset = train.vec(self.params["offset_column"]).as_float().to(X.device)
            if not bool(ok.all()):
                offset = offset[ok]
        ntrees = int(self.params["ntrees"])
        ckpt = self._checkpoint_ensemble()
        base_margin = None if ckpt is None else ckpt.raw_margin(X)
        if ckpt is not None:
            # H2O checkpoint: continue a previous model up to `ntrees` total trees
            init_f = None
            ntrees = max(0, ntrees - ckpt.ntrees)
        if offset is not None:
            if base_margin is None:
                init_f = np.array([_offset_init(ens_dist, y, w, offset, self.params, self.comm)], np.float64)
                base_margin = torch.full((1, offset.numel()), float(init_f[0]), device=offset.device)
            base_margin = base_margin.to(offset.device) + offset[None, :]
        scorer = _TreeScoring(self, train, valid, X, y, w, ens_dist, nclass, ckpt)
        ens = train_ensemble(bm, y, w, dist=ens_dist, ntrees=ntrees, tparams=tp,
                             sample_rate=float(self.params.get("sample_rate", 1.0)), nclass=nclass,
                             seed=self._seed(), comm=self.comm, init_f=init_f,
                             callback=scorer if scorer.active else None,
                             base_margin=base_margin, tree_offset=0 if ckpt is None else ckpt.ntrees,
                             dist_kw={"tweedie_power": float(self.params.get("tweedie_power", 1.5)),
                                      "quantile_alpha": float(self.params.get("quantile_alpha", 0.5)),
                                      "huber_delta": float(self.params.get("huber_alpha", 0.9))})
        if ckpt is not None:
            if ckpt.catbits is not None or ens.catbits is not None:
                ens.catbits = concat_catbits(ckpt, ens)
            ens.trees = concat_trees(ckpt.trees, ens.trees) if len(ens.trees) else ckpt.trees
            ens.init_f = ckpt.init_f
        model = self.model_cls(self, model_id, ens, ens_dist)
        model.warnings = list(self._warnings)
        model.class_dist = balance      # (prior, modelled) class fractions for correctProbabilities
        model.calibration = None
        if self.params.get("calibrate_model"):
            model.calibration = _fit_calibration(model, self.params.get("calibration_frame"),
                                                 str(self.params.get("calibration_method") or "AUTO"))
        model.timings = dict(ens.timings)
        model.scoring_history = scorer.history
        oob = getattr(ens, "_oob", None)
        if oob is not None and ckpt is None and not self.params.get("offset_column"):
            model.training_metrics = _oob_metrics(model, train, y, w, oob, ens_dist)
        return model

    def _sort_levels_by_response(self, train: Frame, valid: Frame | None):
        """H2O ``categorical_encoding="SortByResponse"``: every categorical
        predictor's levels are reordered by their mean response (lowest -> code
        0; levels without training rows last), so ordinal bin splits separate
        low- from high-response levels.  The reordered domain is the model's
        (scoring frames and MOJOs map level names onto it)."""
        yv = train.vec(self.y)
        yval = yv.as_float().double() if self.category == ModelCategory.REGRESSION else yv.data.double()
        ok = ~torch.isnan(yval) & (yval >= 0 if self.category != ModelCategory.REGRESSION else True)
        for c in self.x:
            if self.feature_types.get(c) != ENUM:
                continue
            dom = list(self.feature_domains.get(c) or [])
            L = len(dom)
            if L < 2:
                continue
            codes = train.vec(c).data.long().to(yval.device)
            m = ok & (codes >= 0) & (codes < L)
            sums = torch.bincount(codes[m], weights=yval[m], minlength=L).cpu().numpy()
            cnt = torch.bincount(codes[m], minlength=L).cpu().numpy()
            if self.comm is not None and self.comm.world_size > 1:
                sums = self.comm.all_reduce_numpy(sums.astype(np.float64))
                cnt = self.comm.all_reduce_numpy(cnt.astype(np.float64))
            key = [(sums[i] / cnt[i] if cnt[i] > 0 else float("inf"), i) for i in range(L)]
            self.feature_domains[c] = [dom[i] for _, i in sorted(key)]
        adapt = Model.adapt_frame.__get__(self)
        return adapt(train), (adapt(valid) if valid is not None else None)

    def _checkpoint_ensemble(self):
        ck = self.params.get("checkpoint")
        if not ck:
            return None
        from ..frame.frame import DKV

        m = DKV.get(ck) if isinstance(ck, str) else ck
        if m is None or not hasattr(m, "ens"):
            raise ValueError(f"checkpoint model {ck!r} not found or not a tree model")
        if list(m.x) != list(self.x):
            raise ValueError("checkpoint model was trained on different predictors")
        if int(m.params.get("max_depth", -1)) != int(self.params["max_depth"]):
            raise ValueError("checkpoint continuation requires the same max_depth")
        return m.ens

    def _engine_dist(self, dist: str) -> str:
        return dist


def _oob_metrics(model, train, y, w, oob, dist) -> dict:
    """H2O DRF training metrics: every row scored by the trees whose bag left
    it out only (average of their leaf values); rows no tree left out are not
    scored.  ``oob_rows`` = the scored count (all ranks)."""
    from .base import compute_metrics
    from .scoring import margins_to_scores

    s, cnt = oob
    dev = y.device
    s, cnt = s.to(dev), cnt.to(dev)
    ok = cnt > 0
    P = margins_to_scores(s[:, ok] / cnt[ok][None, :], dist, model.category, 1)
    yv = train.vec(model.y)
    yy = Vec(model.y, (y.to(torch.int32) if model.category in ("Binomial", "Multinomial") else y.float())[ok],
             ENUM if model.category in ("Binomial", "Multinomial") else "real",
             list(yv.domain) if yv.domain else None)
    m = compute_metrics(model.category, P, yy, None if w is None else w.to(dev)[ok], model.comm, dist)
    n_ok = float(ok.sum())
    if model.comm is not None and model.comm.world_size > 1:
        n_ok = float(model.comm.all_reduce_numpy(np.array([n_ok]))[0])
    m["oob_rows"] = int(n_ok)
    m["description"] = "Metrics reported on Out-Of-Bag training samples"
    return m


def _fit_calibration(model, cal, method: str) -> dict:
    """H2O ``calibrate_model``: map the binomial p1 on ``calibration_frame`` to
    calibrated probabilities - Platt scaling (logistic regression of y on p1,
    Newton in fp64; method AUTO / PlattScaling) or isotonic regression
    (pool-adjacent-violators, clipped to the fitted range)."""
    from ..frame.frame import DKV

    if model.category != ModelCategory.BINOMIAL:
        raise ValueError("calibrate_model: binomial models only (as in H2O)")
    cal = DKV.get(cal) if isinstance(cal, str) else cal
    if cal is None:
        raise ValueError("calibrate_model requires calibration_frame")
    p1 = model.predict_raw(cal)[-1].double()
    y = model.adapt_frame(cal).vec(model.y).data.long().to(p1.device)
    ok = y >= 0
    p1, y = p1[ok], (y[ok] == 1).double()
    comm = getattr(model, "comm", None)
    multi = comm is not None and comm.world_size > 1
    m = method.lower()
    if m in ("auto", "plattscaling", "platt_scaling"):
        # Newton on the row-sharded calibration frame: the 2-vector gradient and
        # 2x2 Hessian are all-reduced every iteration, so all ranks take the
        # same steps and end with the coefficients of the whole frame
        a = np.zeros(2)
        Xd = torch.stack([torch.ones_like(p1), p1], 1)
        for _ in range(100):
            mu = torch.sigmoid(Xd @ torch.from_numpy(a).to(p1.device))
            g = Xd.T @ (y - mu)
            H = (Xd * (mu * (1 - mu))[:, None]).T @ Xd
            gh = torch.cat([g, H.reshape(-1)]).cpu().numpy()
            if multi:
                gh = comm.all_reduce_numpy(gh)
            step = np.linalg.solve(gh[2:].reshape(2, 2) + 1e-10 * np.eye(2), gh[:2])
            a = a + step
            if float(np.abs(step).max()) < 1e-12:
                break
        return {"method": "PlattScaling", "intercept": float(a[0]), "slope": float(a[1])}
    if m in ("isotonicregression", "isotonic_regression"):
        if multi:
            # PAV needs the globally sorted pairs: every rank gathers them and fits
            # the same step function
            p1, y = comm.all_gather_cat(p1.contiguous()), comm.all_gather_cat(y.contiguous())
        # ties ordered by y too, so the fit does not depend on the row order / sharding
        pn, yn = p1.cpu().numpy(), y.cpu().numpy()
        order = np.lexsort((yn, pn))
        xs, ys = pn[order], yn[order]
        vals, wts, xs_hi = [], [], []
        for xv, yv in zip(xs, ys):            # pool adjacent violators
            vals.append(yv); wts.append(1.0); xs_hi.append(xv)
            while len(vals) > 1 and vals[-2] > vals[-1]:
                v = (vals[-2] * wts[-2] + vals[-1] * wts[-1]) / (wts[-2] + wts[-1])
                w = wts[-2] + wts[-1]
                vals[-2:], wts[-2:], xs_hi[-2:] = [v], [w], [xs_hi[-1]]
        return {"method": "IsotonicRegression", "x": [float(v) for v in xs_hi], "y": [float(v) for v in vals],
                "x_min": float(xs[0])}
    raise ValueError(f"calibration_method {method!r}: AUTO, PlattScaling or IsotonicRegression")


def _apply_calibration(cal: dict, p1: torch.Tensor) -> torch.Tensor:
    if cal["method"] == "PlattScaling":
        return torch.sigmoid(cal["intercept"] + cal["slope"] * p1)
    xs = torch.tensor(cal["x"], dtype=torch.float64, device=p1.device)
    ys = torch.tensor(cal["y"], dtype=torch.float64, device=p1.device)
    i = torch.searchsorted(xs, p1.clamp(cal["x_min"], float(xs[-1]))).clamp_max(xs.numel() - 1)
    return ys[i]


def correct_probabilities(P: torch.Tensor, prior, modelled) -> torch.Tensor:
    """H2O ModelUtils.correctProbabilities: class probabilities [K][n] of a
    model trained on a rebalanced class mix, mapped back to the original
    class priors (p_k * prior_k / modelled_k, renormalised)."""
    pr = torch.as_tensor(np.asarray(prior, np.float64), dtype=P.dtype, device=P.device)[:, None]
    md = torch.as_tensor(np.asarray(modelled, np.float64), dtype=P.dtype, device=P.device)[:, None]
    P = P * torch.where((pr > 0) & (md > 0), pr / md.clamp_min(1e-300), torch.ones_like(pr))
    s = P.sum(0, keepdim=True)
    return torch.where(s > 0, P / s.clamp_min(1e-300), P)


def _balance_weights(y, w, K: int, params, comm=None):
    """H2O ``balance_classes`` as row weights: class k's rows carry
    t_k / n_k where t_k is the majority count (or n_k x
    ``class_sampling_factors[k]``), all t_k scaled down so that sum t_k <=
    ``max_after_balance_size`` x N.  Returns the weights and the (prior,
    modelled) class fractions used to correct predicted probabilities."""
    codes = y.long().clamp(0, K - 1)
    n = torch.bincount(codes, weights=None if w is None else w.double().to(codes.device), minlength=K).double().cpu()
    if comm is not None and comm.world_size > 1:
        n = torch.from_numpy(comm.all_reduce_numpy(n.numpy()))
    N = float(n.sum())
    f = params.get("class_sampling_factors")
    t = n * torch.tensor([float(v) for v in f], dtype=torch.float64) if f else torch.where(
        n > 0, torch.full_like(n, float(n.max())), n)
    cap = float(params.get("max_after_balance_size") or 5.0) * N
    if float(t.sum()) > cap:
        t = t * (cap / float(t.sum()))
    ratio = torch.where(n > 0, t / n.clamp_min(1e-300), torch.zeros_like(n)).float().to(y.device)
    rw = ratio[codes]
    w = rw if w is None else w.float().to(y.device) * rw
    return w, ((n / N).numpy(), (t / float(t.sum())).numpy())


def _offset_init(dist: str, y, w, off, params, comm=None) -> float:
    """Initial margin c minimising the loss of ``c + offset`` (H2O GBM with an
    offset column): closed forms where they exist, Newton steps for bernoulli.
    Sums are all-reduced over the ranks; laplace / quantile take the weighted
    quantile of y - offset over all ranks (boost.weighted_quantile)."""
    multi = comm is not None and comm.world_size > 1

    def red(*v):
        a = np.array(v, np.float64)
        return comm.all_reduce_numpy(a) if multi else a

    y = y.double().to(off.device)
    o = off.double()
    wt = torch.ones_like(y) if w is None else w.double().to(off.device)
    if dist == "bernoulli":
        c = 0.0
        for _ in range(50):
            p = torch.sigmoid(c + o)
            g, h = red(float((wt * (y - p)).sum()), float((wt * p * (1 - p)).sum()))
            if h <= 0:
                break
            c += g / h
            if abs(g / h) < 1e-12:
                break
        return c
    if dist == "poisson":
        a, b = red(float((wt * y).sum()), float((wt * torch.exp(o)).sum()))
        return float(np.log(a / b))
    if dist == "tweedie":
        # H2O Tweedie initF: log(sum w y e^{o (1-p)} / sum w e^{o (2-p)})
        pw = float(params.get("tweedie_power", 1.5))
        a, b = red(float((wt * y * torch.exp(o * (1 - pw))).sum()), float((wt * torch.exp(o * (2 - pw))).sum()))
        return float(np.log(a / b))
    if dist == "gamma":
        a, b = red(float((wt * y * torch.exp(-o)).sum()), float(wt.sum()))
        return float(np.log(a / b))
    r = y - o
    if dist in ("laplace", "quantile"):
        from .tree.boost import weighted_quantile

        q = 0.5 if dist == "laplace" else float(params.get("quantile_alpha", 0.5))
        return weighted_quantile(r, None if w is None else wt, q, comm)
    a, b = red(float((wt * r).sum()), float(wt.sum()))
    return float(a / b)      # gaussian / huber


# ---------------------------------------------------------------------------
class _TreeScoring:
    """Training callback: scoring history every ``score_tree_interval`` trees
    (training metrics from the device margins, validation metrics from the
    new trees scored on the validation frame), early stopping, job cancel."""

    def __init__(self, builder, train, valid, X, y, w, dist, nclass, ckpt):
        from .scoring import ScoreKeeper

        p = builder.params
        self.b, self.dist, self.valid = builder, dist, valid
        self.category = builder.category
        self.k = int(p.get("stopping_rounds") or 0)
        iv = int(p.get("score_tree_interval") or 0)
        self.interval = iv if iv > 0 else (5 if (self.k > 0 or valid is not None) else 0)
        self.keeper = ScoreKeeper(p.get("stopping_metric", "AUTO"), self.category, self.k,
                                  float(p.get("stopping_tolerance", 1e-3)))
        self.w = w
        yv = train.vec(builder.y)
        if self.category in ("Binomial", "Multinomial"):
            self.yv = Vec(builder.y, y.to(torch.int32), ENUM, list(yv.domain))
        else:
            self.yv = Vec(builder.y, y.float(), "real")
        self.n_ckpt = ckpt.ntrees if ckpt is not None else 0
        self.vmargin = None
        self.done = 0
        if valid is not None and self.interval:
            Xv = valid.feature_matrix(builder.x)
            self.Xv = Xv
            K = ckpt.K if ckpt is not None else (nclass if dist == "multinomial" or (dist == "drf" and nclass > 2) else 1)
            ocol = p.get("offset_column")
            self.voff = valid.vec(ocol).as_float().to(Xv.device)[None, :] if ocol else 0.0
            self.vmargin = ckpt.raw_margin(Xv).to(Xv.device) + self.voff if ckpt is not None else None
            self.K = K
        from ..runtime.jobs import current_job

        self.job = current_job()
        comm = builder.comm
        self.multi = comm is not None and comm.world_size > 1
        # cancellation is decided collectively so every rank stops on the same tree
        self.cancel_every = 10 if self.multi else 1
        # H2O max_runtime_secs: stop adding trees once the budget is spent (decided
        # collectively with the cancellation flag)
        import time as _time

        self.t_start = _time.time()
        self.max_rt = float(builder.params.get("max_runtime_secs") or 0.0)
        self.active = bool(self.interval) or self.job is not None or self.multi or self.max_rt > 0

    @property
    def history(self):
        return self.keeper.history

    def __call__(self, t, view):
        from ..metrics import binomial_metrics, multinomial_metrics, regression_metrics  # noqa: F401
        from .base import compute_metrics
        from .scoring import margins_to_scores

        if self.job is not None:
            self.job.progress = (t + 1) / max(1, int(self.b.params["ntrees"]))
        if (t + 1) % self.cancel_every == 0:
            import time as _time

            flag = 1.0 if (self.job is not None and self.job.cancel_requested) else 0.0
            if self.max_rt > 0 and _time.time() - self.t_start > self.max_rt:
                flag = 1.0
            if self.multi:
                flag = float(self.b.comm.all_reduce_numpy(np.array([flag]), "max")[0])
            if flag > 0:
                return True
        if not self.interval or (t + 1) % self.interval:
            return False
        ntot = self.n_ckpt + t + 1
        comm = self.b.comm
        cat = self.category
        P = margins_to_scores(view.margin.to(self.yv.data.device).float(), self.dist, cat, ntot)
        tm = compute_metrics(cat, P, self.yv, self.w, comm, self.dist)
        entry = {"number_of_trees": ntot}
        entry.update({f"training_{k.lower()}": v for k, v in tm.items() if isinstance(v, float)})
        metrics = tm
        if self.vmargin is not None or (self.valid is not None and hasattr(self, "Xv")):
            from .tree.boost import TreeEnsemble

            new = view.trees(self.done, t + 1)
            part = TreeEnsemble(new, self.K, self.dist, np.zeros(self.K), average=False)
            part.catbits = view.catbits(self.done, t + 1) if hasattr(view, "catbits") else None
            m = part.raw_margin(self.Xv).to(self.Xv.device) if len(new) else 0.0
            if self.vmargin is None:
                init = 0.0 if self.dist == "drf" else torch.from_numpy(
                    np.asarray(view.init_f, np.float32)).to(self.Xv.device)[:, None]
                self.vmargin = init + m + self.voff
            else:
                self.vmargin = self.vmargin + m
            self.done = t + 1
            Pv = margins_to_scores(self.vmargin, self.dist, cat, ntot)
            vm = compute_metrics(cat, Pv, self.valid.vec(self.b.y), None, comm, self.dist)
            entry.update({f"validation_{k.lower()}": v for k, v in vm.items() if isinstance(v, float)})
            metrics = vm
        return self.keeper.record(entry, metrics)


class GBMModel(TreeModel):
    algo = "gbm"
    algo_full_name = "Gradient Boosting Machine"


class H2OGradientBoostingEstimator(_TreeBuilder):
    """H2O GBM: squared-error splits on pseudo-residuals, Newton leaf steps."""
    algo = "gbm"
    model_cls = GBMModel
    auto_histogram = "uniformadaptive"
    per_node_histograms = True
    default_nbins = 20
    DEFAULTS = dict(ntrees=50, max_depth=5, min_rows=10.0, nbins=20, nbins_top_level=1024, nbins_cats=1024,
                    learn_rate=0.1, learn_rate_annealing=1.0, sample_rate=1.0, col_sample_rate=1.0,
                    col_sample_rate_per_tree=1.0, min_split_improvement=1e-5, histogram_type="AUTO",
                    max_abs_leafnode_pred=0.0, tweedie_power=1.5, quantile_alpha=0.5, huber_alpha=0.9,
                    stopping_rounds=0, stopping_metric="AUTO", stopping_tolerance=1e-3, score_tree_interval=0,
                    offset_column=None, balance_classes=False, class_sampling_factors=None,
                    max_after_balance_size=5.0, categorical_encoding="AUTO", checkpoint=None,
                    calibrate_model=False, calibration_frame=None, calibration_method="AUTO",
                    monotone_constraints=None, interaction_constraints=None)

    def _tree_params(self, nfeat):
        p = self.params
        return TreeParams(max_depth=int(p["max_depth"]), min_rows=float(p["min_rows"]), learn_rate=float(p["learn_rate"]),
                          learn_rate_annealing=float(p.get("learn_rate_annealing") or 1.0),
                          min_split_improvement=float(p["min_split_improvement"]), mode=0, leaf_mode=0,
                          col_sample_rate=float(p["col_sample_rate"]),
                          col_sample_rate_per_tree=float(p["col_sample_rate_per_tree"]),
                          max_abs_leaf=float(p["max_abs_leafnode_pred"] or 0.0), seed=self._seed(),
                          monotone=self._monotone(), interactions=self._interactions())


# ---------------------------------------------------------------------------
class XGBoostModel(TreeModel):
    algo = "xgboost"
    algo_full_name = "XGBoost"


class H2OXGBoostEstimator(_TreeBuilder):
    """XGBoost 'hist' semantics: second-order gain with L1/L2 leaf penalties,
    min_child_weight on hessian mass, eta-scaled leaves."""
    algo = "xgboost"
    model_cls = XGBoostModel
    group_splits = False

    def _encoding_scheme(self) -> str:
        """H2O XGBoost: AUTO / OneHotInternal one-hot encode the levels; Enum
        feeds the level codes (ordinal)."""
        from ..frame.encoding import normalize_scheme

        s = normalize_scheme(self.params.get("categorical_encoding"))
        return {"auto": "onehotexplicit", "onehotinternal": "onehotexplicit", "enum": "labelencoder"}.get(s, s)
    mode = 1
    default_nbins = 255
    DEFAULTS = dict(ntrees=50, max_depth=6, min_rows=1.0, min_child_weight=None, learn_rate=0.3, eta=None,
                    sample_rate=1.0, subsample=None, col_sample_rate=1.0, colsample_bylevel=None,
                    col_sample_rate_per_tree=1.0, colsample_bytree=None, colsample_bynode=1.0, reg_lambda=1.0,
                    reg_alpha=0.0, gamma=0.0, min_split_improvement=None, max_bins=256, tree_method="hist",
                    booster="gbtree", grow_policy="depthwise", max_abs_leafnode_pred=0.0, tweedie_power=1.5,
                    stopping_rounds=0, stopping_metric="AUTO", stopping_tolerance=1e-3, score_tree_interval=0,
                    offset_column=None, backend="gpu", nbins=None, categorical_encoding="AUTO", checkpoint=None,
                    calibrate_model=False, calibration_frame=None, calibration_method="AUTO",
                    monotone_constraints=None, interaction_constraints=None)

    def _tree_params(self, nfeat):
        p = self.params
        mcw = p["min_child_weight"] if p["min_child_weight"] is not None else p["min_rows"]
        eta = p["eta"] if p["eta"] is not None else p["learn_rate"]
        gamma = p["min_split_improvement"] if p["min_split_improvement"] is not None else p["gamma"]
        if p.get("subsample") is not None:
            p["sample_rate"] = p["subsample"]
        csr = p["colsample_bylevel"] if p["colsample_bylevel"] is not None else p["col_sample_rate"]
        csr = float(csr) * float(p.get("colsample_bynode") or 1.0)
        cst = p["colsample_bytree"] if p["colsample_bytree"] is not None else p["col_sample_rate_per_tree"]
        return TreeParams(max_depth=int(p["max_depth"]), min_rows=0.0, min_child_weight=float(mcw),
                          reg_lambda=float(p["reg_lambda"]), reg_alpha=float(p["reg_alpha"]), gamma=float(gamma),
                          min_split_improvement=0.0, learn_rate=float(eta), mode=1, leaf_mode=0,
                          col_sample_rate=csr, col_sample_rate_per_tree=float(cst),
                          max_abs_leaf=float(p["max_abs_leafnode_pred"] or 0.0), seed=self._seed(),
                          monotone=self._monotone(), interactions=self._interactions())


# ---------------------------------------------------------------------------
class DRFModel(TreeModel):
    algo = "drf"
    algo_full_name = "Distributed Random Forest"


class H2ORandomForestEstimator(_TreeBuilder):
    """Random forest: bagged (sample_rate) trees with per-node feature
    sampling (mtries), leaves = mean response (class-indicator means for
    classification), predictions averaged over trees.

    Histograms: H2O's AUTO = per-node UniformAdaptive with nbins=20 on fine
    quantile bins (``binning.py``).  With max_depth > 12 (the default 20) and
    the default nbins_top_level, the fine grid has 63 bins per column instead
    of 255: 1.4x faster (10M x 100: 13.7 vs 19.4 ms/tree) at a small accuracy
    cost (out-of-bag AUC 0.791 vs 0.794 there); the fit warns.  Passing
    ``nbins_top_level`` (e.g. H2O's 1024) keeps 255 bins."""
    algo = "drf"
    model_cls = DRFModel
    auto_histogram = "uniformadaptive"
    per_node_histograms = True
    default_nbins = 20
    DEFAULTS = dict(ntrees=50, max_depth=20, min_rows=1.0, nbins=20, nbins_top_level=1024, nbins_cats=1024,
                    mtries=-1, sample_rate=0.632, col_sample_rate_per_tree=1.0, min_split_improvement=1e-5,
                    binomial_double_trees=False, histogram_type="AUTO", stopping_rounds=0,
                    stopping_metric="AUTO", stopping_tolerance=1e-3, score_tree_interval=0, balance_classes=False,
                    class_sampling_factors=None, max_after_balance_size=5.0,
                    categorical_encoding="AUTO", offset_column=None, checkpoint=None,
                    calibrate_model=False, calibration_frame=None, calibration_method="AUTO")

    def _engine_dist(self, dist):
        return "drf"

    def _tree_params(self, nfeat):
        p = self.params
        mt = int(p["mtries"])
        if mt == -1:
            mt = max(1, int(math.sqrt(nfeat))) if self.category != ModelCategory.REGRESSION else max(1, nfeat // 3)
        elif mt == -2 or mt >= nfeat:
            mt = 0
        return TreeParams(max_depth=int(p["max_depth"]), min_rows=float(p["min_rows"]), learn_rate=1.0,
                          min_split_improvement=float(p["min_split_improvement"]), mode=0, leaf_mode=1, mtries=mt,
                          col_sample_rate_per_tree=float(p["col_sample_rate_per_tree"]), seed=self._seed())

    def _fit(self, train, valid, model_id):
        if self.category == ModelCategory.BINOMIAL:
            # one regression tree per iteration on the class-1 indicator (H2O
            # DRF binomial without binomial_double_trees)
            return super()._fit(train, valid, model_id)
        return super()._fit(train, valid, model_id)
