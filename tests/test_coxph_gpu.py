"""CoxPH on the gfx950 kernels (ops.survival): one Newton pass against a naive
per-time oracle, concordance against the torch pair tables, and the public fit
against the CPU-frame fit."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from h2omx.frame import Frame
from h2omx.models import H2OCoxProportionalHazardsEstimator
from h2omx.models.coxph import _concordance_torch, _event_sums
from h2omx.ops import survival

pytestmark = pytest.mark.gpu

N = 1500


def _oracle(beta, X, t, d, w, start, strata, dtype):
    """Textbook partial likelihood: per stratum and distinct event time the risk set by
    comparison, the tied events, and phi2/phi0 - mu mu^T.  Returns {ties: [ll, grad, hess, sum of
    phi2/phi0]}; the last is the larger of the two sums whose difference the kernels form."""
    X, t, d, w, beta = (np.asarray(a, dtype) for a in (X, t, d, w, beta))
    p = X.shape[1]
    eta = X @ beta
    r = w * np.exp(eta)
    out = {k: [dtype(0), np.zeros(p, dtype), np.zeros((p, p), dtype), np.zeros((p, p), dtype)]
           for k in ("efron", "breslow")}
    for s in np.unique(strata):
        idx = np.nonzero(strata == s)[0]
        for tau in np.unique(t[idx][d[idx] > 0]):
            R = idx[(t[idx] >= tau) & ((np.asarray(start, dtype)[idx] < tau) if start is not None else True)]
            D = idx[(t[idx] == tau) & (d[idx] > 0)]
            S = [r[R].sum(), r[R] @ X[R], (X[R] * r[R, None]).T @ X[R]]
            A = [r[D].sum(), r[D] @ X[D], (X[D] * r[D, None]).T @ X[D]]
            m = len(D)
            for ties, terms in (("efron", [(dtype(k) / m, w[D].sum() / m) for k in range(m)]),
                                ("breslow", [(dtype(0), w[D].sum())])):
                o = out[ties]
                o[0] += w[D] @ eta[D]
                o[1] += w[D] @ X[D]
                for f, sc in terms:
                    phi0, phi1, phi2 = (S[q] - f * A[q] for q in range(3))
                    mu = phi1 / phi0
                    o[0] -= sc * np.log(phi0)
                    o[1] -= sc * mu
                    o[2] -= sc * (phi2 / phi0 - np.outer(mu, mu))
                    o[3] += sc * phi2 / phi0
    return out


@functools.lru_cache(maxsize=None)
def _case(variant, p):
    rng = np.random.default_rng(100 * p + ord(variant))
    X = rng.normal(size=(N, p))
    c = dict(w=np.ones(N), strata=np.zeros(N, np.int64), start=None)
    T = rng.exponential(np.exp(-0.5 * X[:, 0]))
    C = rng.exponential(1.0, N)
    t, d = np.minimum(T, C), (T <= C).astype(float)              # about half events
    if variant == "b":     # 3 distinct times: buckets of ~500 rows, and x0 follows time
        t = np.ceil(np.clip(t, 0.01, 1.4) * 2)
        X[:, 0] += t
    if variant == "c":     # weights, unequal strata, stratum 2 has no event, late censoring
        c["w"] = rng.uniform(0.5, 2.0, N)
        c["strata"] = np.repeat([0, 1, 2], [900, 450, 150])
        d[c["strata"] == 2] = 0.0
        t[:40] = t.max() + rng.uniform(0.1, 1.0, 40)
        d[:40] = 0.0
    if variant == "d":     # start times, some at or above other rows' event times, some after the last event
        t = np.round(t, 2) + 0.01
        c["start"] = np.maximum(0.0, t - rng.uniform(0.05, 1.0, N))
        late = np.arange(20)
        t[late], d[late] = t.max() + 1.0 + rng.uniform(0, 1, 20), 0.0
        c["start"][late] = t[late] - 0.5
        odd = np.arange(20, 40)
        c["start"][odd] = t[odd]                                  # start >= stop
    wm = (X * c["w"][:, None]).sum(0) / c["w"].sum()
    beta = rng.normal(size=p)
    c.update(X=X - wm, t=t, d=d, beta=beta / np.linalg.norm(beta))
    args = (c["beta"], c["X"], t, d, c["w"], c["start"], c["strata"])
    c["ref"] = _oracle(*args, np.longdouble)
    tt = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v))) for k, v in c.items()
          if k in ("X", "t", "d", "w", "start", "strata", "beta")}
    c["torch"] = tt
    c["cpu"] = {ties: _event_sums(tt["t"], tt["start"], tt["d"], tt["w"], tt["X"] @ tt["beta"], tt["X"],
                                  tt["strata"], ties == "efron") for ties in ("efron", "breslow")}
    return c


def _rel_err(got, ref):
    """Largest error of ll, grad, hess, each relative to its largest absolute entry."""
    return max(float(np.max(np.abs(np.asarray(g, np.longdouble) - r)) / np.max(np.abs(r)))
               for g, r in zip(got, ref))


@pytest.mark.parametrize("ties", ["efron", "breslow"])
@pytest.mark.parametrize("p", [1, 5, 17, 33])
@pytest.mark.parametrize("variant", ["a", "b", "c", "d"])
def test_newton_pass_matches_oracle(cuda_dev, variant, p, ties):
    c = _case(variant, p)
    ref = c["ref"][ties]
    e_ref = _rel_err([v.numpy() for v in c["cpu"][ties]], ref)
    dev = {k: (None if v is None else v.to(cuda_dev)) for k, v in c["torch"].items()}
    plan = survival.cox_prepare(dev["t"], dev["start"], dev["d"], dev["w"], dev["strata"], dev["X"])
    got = [v.cpu().numpy() for v in survival.cox_newton_pass(plan, dev["beta"], ties == "efron")]
    err = _rel_err(got, ref)
    again = [v.cpu().numpy() for v in survival.cox_newton_pass(plan, dev["beta"], ties == "efron")]
    print(f"cox {variant} p={p} {ties}: e_ref={e_ref:.2e} kernel={err:.2e} nb={plan.nb} "
          f"cancellation={float(np.max(np.abs(ref[3])) / np.max(np.abs(ref[2]))):.2f}")
    assert all(np.array_equal(a, b) for a, b in zip(got, again))          # bit-identical between calls
    assert err <= max(100 * e_ref, 64 * N * 2.0 ** -52)


@pytest.mark.parametrize("events", [True, False])
def test_concordance_equals_torch(cuda_dev, events):
    rng = np.random.default_rng(7)
    n = 3000
    t = torch.from_numpy(np.round(rng.exponential(1.0, n), 1)).to(cuda_dev)
    lp = torch.from_numpy(np.round(rng.normal(size=n), 2)).to(cuda_dev)
    d = torch.from_numpy((rng.random(n) < 0.6).astype(float) * events).to(cuda_dev)
    got, want = survival.concordance(t, d, lp), _concordance_torch(t, d, lp)
    assert got == want or (np.isnan(got) and np.isnan(want) and not events)


def _frame_case(variant, ncol):
    c = _case(variant, 5)
    rng = np.random.default_rng(3)
    X = c["X"] if ncol == 5 else np.hstack([c["X"], rng.normal(size=(N, ncol - 5))])
    df = pd.DataFrame(X, columns=[f"x{j}" for j in range(ncol)])
    df["t"], df["ev"], df["w"], df["g"] = c["t"], c["d"], c["w"], c["strata"].astype(float)
    kw = dict(stop_column="t", weights_column="w", stratify_by=["g"])
    if c["start"] is not None:
        df["s"] = c["start"]
        kw["start_column"] = "s"
    return df, kw, [f"x{j}" for j in range(ncol)]


@pytest.mark.parametrize("variant,ncol,engine", [("c", 5, "hip"), ("d", 5, "hip"), ("c", 65, "torch")])
def test_public_fit_matches_cpu_frame(cuda_dev, variant, ncol, engine):
    df, kw, x = _frame_case(variant, ncol)
    mc = H2OCoxProportionalHazardsEstimator(**kw).train(x=x, y="ev", training_frame=Frame.from_pandas(df))
    mg = H2OCoxProportionalHazardsEstimator(**kw).train(x=x, y="ev",
                                                        training_frame=Frame.from_pandas(df, device="cuda"))
    assert mg.newton_engine == engine and mc.newton_engine == "torch"
    np.testing.assert_allclose(mg.beta, mc.beta, rtol=1e-5)
    assert mg.stats["iter"] == mc.stats["iter"]
