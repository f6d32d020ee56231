"""The partial dependence sweep kernel (csrc/explain_kernels.hip:
pd_sweep_kernel) against one ``predict_raw_kernel`` launch per cell on the
same device matrix, bit for bit: every (cell, row) margin receives the same
fp32 additions in the same tree order.  Then row chunking, the public tables
on a device frame and ICE.

Public tables are compared with the general frame-substitution path on the
same device frame (the CPU scorer adds the leaf values in float64, so its
float32 margins are not those of the device kernels bit for bit; the distance
to the CPU table is printed).  Both paths score identical margins and differ
in summation order only.  With u = 2**-52, n rows, weights <= W and |r| <= R
(R from the node table: |init_f| plus every tree's largest |leaf|, 1 for
probabilities) each float64 sum is within n u W R (``sum w r``) or n u W R^2
(``sum w r^2``) of the exact one, so two tables differ by at most
    |mean_a - mean_b| <= 2 n u W R / sw,
and with dvar0 = 2 (n u W R^2 + 2 R n u W R) / sw + 8 u R^2 the bound on the
uncorrected variance s2 / sw - mean^2 (its own roundings included),
    |sd_a - sd_b| <= sqrt(dvar0 m / (m - 1))       (|sqrt a - sqrt b| <= sqrt |a - b|),
and the standard error by that over sqrt m.
"""
import math

import numpy as np
import pytest
import torch

import h2omx.explain as ex
from h2omx import _native
from h2omx.explain import _pd_margins_device, _pd_margins_loop, _response
from h2omx.frame import Frame
from h2omx.frame.frame import ENUM, Vec
from h2omx.models import H2OGradientBoostingEstimator, H2ORandomForestEstimator

pytestmark = pytest.mark.gpu

N_TRAIN, N_SCORE, U = 3000, 1000, 2.0 ** -52
NUM = ["f0", "f1", "f2", "f3", "f4", "flat"]
LEVELS = ["a", "b", "c", "d", "e"]
X_COLS = NUM + ["e"]
FS, FLAT, FE = 0, 5, 6                 # f0 holds NaNs, flat is constant (never split), e is the enum
ROWS = (1, 257, 1000)                  # a single thread, one row past a workgroup, a ragged tail of four workgroups
CASES = {"gbm_d5": (H2OGradientBoostingEstimator, dict(ntrees=20, max_depth=5), "y"),
         "drf_d10": (H2ORandomForestEstimator, dict(ntrees=5, max_depth=10), "y"),
         "gbm_k3": (H2OGradientBoostingEstimator, dict(ntrees=20, max_depth=5), "cls")}
NAN = float("nan")


def _data(seed=7):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_TRAIN, 5)).astype(np.float32)
    e = rng.integers(0, 5, N_TRAIN)
    y = X[:, 0] * X[:, 1] + X[:, 2] + 0.5 * X[:, 3] + 1.5 * np.isin(e, (1, 3)) + 0.1 * rng.normal(size=N_TRAIN)
    X[::11, 0] = np.nan
    X[3::17, 2] = np.nan
    d = {c: X[:, j] for j, c in enumerate(NUM[:5])}
    d["flat"] = np.full(N_TRAIN, 1.5, np.float32)
    d["e"] = np.array(LEVELS, dtype=object)[e]
    d["y"] = y.astype(np.float32)
    d["cls"] = np.array(["lo", "mid", "hi"], dtype=object)[np.digitize(y, np.quantile(y, [0.33, 0.66]))]
    d["w"] = rng.integers(0, 4, N_TRAIN).astype(np.float32)
    return d


@pytest.fixture(scope="module")
def frames(cuda_dev):
    d = _data()
    score = {k: v[:N_SCORE] for k, v in d.items()}
    return Frame.from_numpy(d, device=cuda_dev), Frame.from_numpy(score, device=cuda_dev), Frame.from_numpy(score)


def _reachable(tr):
    """The records of one tree that a path reaches (the others hold whatever the build left)."""
    found, stack = [], [0]
    while stack:
        nd = tr[stack.pop()]
        found.append(nd)
        if nd["feat"] >= 0:
            stack += [int(nd["left"]), int(nd["left"]) + 1]
    return np.array(found, dtype=tr.dtype)


def _split_nodes(ens, f):
    nodes = np.concatenate([_reachable(tr) for tr in ens.trees[:ens.ntrees * ens.K]])
    return nodes[nodes["feat"] == f]


def _grids(ens):
    thr = np.unique(_split_nodes(ens, FS)["thr"])[:20].astype(np.float32)
    edge = np.concatenate([thr, np.nextafter(thr, np.float32(-np.inf)), np.nextafter(thr, np.float32(np.inf)), thr[:5]])
    np.random.default_rng(3).shuffle(edge)
    return {"one": np.array([0.3], np.float32), "two": np.array([0.5, -0.5], np.float32),
            "lin20": np.linspace(-3.0, 3.0, 20).astype(np.float32),
            "lin65": np.linspace(-3.0, 3.0, 65).astype(np.float32), "edges": edge}


@pytest.fixture(scope="module", params=list(CASES))
def case(request, frames, cuda_dev):
    cls, kw, y = CASES[request.param]
    train, score, score_cpu = frames
    m = cls(seed=1, **kw).train(x=X_COLS, y=y, training_frame=train)
    ens = m.ens
    assert m.x == X_COLS and ens.K == (3 if y == "cls" else 1)
    # the run logic needs splits on the swept column in every model; flat has none; e splits by level sets
    assert len(_split_nodes(ens, FS)) > 0 and len(_split_nodes(ens, 1)) > 0
    assert len(_split_nodes(ens, FLAT)) == 0
    assert ens.catbits is not None and (_split_nodes(ens, FE)["na_left"] & 2).any()
    Xd = score.feature_matrix(m.x)
    assert Xd.is_cuda and bool(torch.isnan(Xd[FS]).any()) and bool(torch.isnan(Xd[FS, 0]))
    grids = _grids(ens)
    # one oracle per grid at 1000 rows with the NaN cell last (rows and cells are independent: slices are oracles too)
    refs = {k: _pd_margins_loop(m, Xd, FS, np.r_[g, np.float32(NAN)]) for k, g in grids.items()}
    leaf = sum(float(np.abs(nd["value"][nd["feat"] < 0]).max())
               for nd in map(_reachable, ens.trees[:ens.ntrees * ens.K]))
    R = 1.0 if y == "cls" else (leaf / ens.ntrees if ens.average else float(np.abs(ens.init_f).max()) + leaf)
    return dict(m=m, Xd=Xd, grids=grids, refs=refs, score=score, score_cpu=score_cpu, R=float(R),
                target="mid" if y == "cls" else None)


@pytest.mark.parametrize("gname", ["one", "two", "lin20", "lin65", "edges"])
def test_kernel_equals_one_launch_per_cell(case, gname):
    m, Xd, g, ref = case["m"], case["Xd"], case["grids"][gname], case["refs"][gname]
    G = len(g)
    assert tuple(ref.shape) == (1, G + 1, m.ens.K, N_SCORE)
    if gname == "edges":
        assert G >= 3 * 5 + 5 and len(np.unique(g)) < G          # thresholds, their neighbours, duplicates
    walks = torch.zeros(1, dtype=torch.int64, device=Xd.device)
    for n in ROWS:
        X = Xd[:, :n].contiguous()
        for with_nan in (False, True):
            grid = np.r_[g, np.float32(NAN)] if with_nan else g
            got = _pd_margins_device(m, X, FS, grid, walks=walks if n == N_SCORE and with_nan else None)
            want = ref[:, :len(grid), :, :n]
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape)
            assert torch.equal(got, want), (gname, n, with_nan, float((got - want).abs().max()))
    per = float(walks) / (N_SCORE * m.ens.ntrees * m.ens.K)
    print(f"{m.algo} {gname}: G={G} + NaN, {per:.2f} walks per (row, tree) against {G + 1} cells")
    assert 1.0 <= per <= G + 1
    # with and without the walk counter the margins are the same
    assert torch.equal(_pd_margins_device(m, Xd, FS, np.r_[g, np.float32(NAN)]), ref)
    assert "explain" in " ".join(_native.loaded_libraries())


def test_unsplit_column_gives_equal_cells(case):
    m, Xd = case["m"], case["Xd"]
    grid = np.r_[np.linspace(-2.0, 4.0, 7).astype(np.float32), np.float32(NAN)]
    got = _pd_margins_device(m, Xd, FLAT, grid)
    assert torch.equal(got, _pd_margins_loop(m, Xd, FLAT, grid))
    assert torch.equal(got, got[:, :1].expand_as(got))


def test_enum_sweep_with_unseen_level(case):
    m, Xd = case["m"], case["Xd"]
    for grid in ([0, 1, 2, 3, 4, 300], [0, 1, 2, 3, 4, 300, NAN], [3, 300, 0, NAN, 4, 1, 2, -7]):
        for n in ROWS:
            X = Xd[:, :n].contiguous()
            got = _pd_margins_device(m, X, FE, grid)
            assert torch.equal(got, _pd_margins_loop(m, X, FE, grid)), (grid, n)
    full = _pd_margins_device(m, Xd, FE, [0, 1, 2, 3, 4])
    assert not torch.equal(full[:, 0], full[:, 1]) or not torch.equal(full[:, 0], full[:, 3])     # the levels matter


@pytest.mark.parametrize("fs,ff", [(0, 1), (1, 0), (FE, 0), (0, FE)])
def test_pair_with_a_fixed_column(case, fs, ff):
    m, Xd = case["m"], case["Xd"]
    enum_grid = [0.0, 2.0, NAN, 4.0]
    num_grid = np.r_[np.linspace(-2.0, 2.0, 9).astype(np.float32), np.float32(NAN)]
    grid = enum_grid if fs == FE else num_grid
    fixed = [1.0, NAN, 3.0] if ff == FE else [0.25, NAN, -1.0]
    for n in ROWS:
        X = Xd[:, :n].contiguous()
        got = _pd_margins_device(m, X, fs, grid, ff, fixed)
        assert tuple(got.shape) == (3, len(grid), m.ens.K, n)
        assert torch.equal(got, _pd_margins_loop(m, X, fs, grid, ff, fixed)), (fs, ff, n)


def test_row_chunks(case, monkeypatch):
    m, Xd = case["m"], case["Xd"]
    g = case["grids"]["two"]                                     # not ascending: the budget covers the reordered copy
    K = m.ens.K
    per_row = 4 * 2 * K * 2
    chunks = list(ex._pd_margin_chunks(m, Xd, FS, g, budget=per_row * 400))
    assert [(a, b) for a, b, _ in chunks] == [(0, 400), (400, 800), (800, 1000)]
    got = _pd_margins_device(m, Xd, FS, g, budget=per_row * 400)
    assert torch.equal(got, case["refs"]["two"][:, :2])
    g65 = case["grids"]["lin65"]
    assert torch.equal(_pd_margins_device(m, Xd, FS, g65, budget=4 * 65 * K * 333), case["refs"]["lin65"][:, :65])

    # the refusal comes before any launch
    def no_launch(*a, **k):
        raise AssertionError("a kernel library was opened")

    import h2omx.ops as ops

    monkeypatch.setattr(ops, "explain_lib", no_launch)
    msg = rf"one row \(1 x 65 cells, {K} classes\) need {260 * K} bytes.*limit is 259 bytes"
    with pytest.raises(ValueError, match=msg):
        _pd_margins_device(m, Xd, FS, g65, budget=259)


def _compare_tables(a, b, n, sw, mk, R, W=1.0):
    dmean = 2 * n * U * W * R / sw
    dvar = 2 * (n * U * W * R * R + 2 * R * n * U * W * R) / sw + 8 * U * R * R
    dsd = math.sqrt(dvar * mk / max(mk - 1, 1))
    assert len(a["data"]) == len(b["data"])
    worst = [0.0, 0.0]
    for ra, rb in zip(a["data"], b["data"]):
        assert list(ra) == list(rb)
        for k in ra:
            if not k.endswith("_response"):
                assert ra[k] == rb[k] or (ra[k] != ra[k] and rb[k] != rb[k])
        worst[0] = max(worst[0], abs(ra["mean_response"] - rb["mean_response"]))
        worst[1] = max(worst[1], abs(ra["stddev_response"] - rb["stddev_response"]))
        assert abs(ra["mean_response"] - rb["mean_response"]) <= dmean
        assert abs(ra["stddev_response"] - rb["stddev_response"]) <= dsd
        assert abs(ra["std_error_mean_response"] - rb["std_error_mean_response"]) <= dsd / math.sqrt(max(mk, 1))
    print(f"  max |mean diff| {worst[0]:.3e} (bound {dmean:.3e}), max |sd diff| {worst[1]:.3e} (bound {dsd:.3e})")


def test_public_tables_match_the_general_path(case, monkeypatch):
    m, fr, R, target = case["m"], case["score"], case["R"], case["target"]
    w = fr.vec("w").data.double()
    calls = dict(cols=["f0", "e"], nbins=7, target=target)
    variants = {"1-D": {}, "pair": dict(cols=None, col_pairs_2dpdp=[("f0", "f1"), ("e", "f2")]),
                "weights": dict(weight_column="w"), "include_na": dict(include_na=True),
                "pair with NA": dict(cols=None, col_pairs_2dpdp=[("f2", "e")], include_na=True),
                "row_index": dict(row_index=0, user_splits={"f0": [-1.0, 0.0, 1.0]})}
    fast = {}
    launches = []
    real = ex._pd_margin_chunks

    def spy(*a, **k):
        launches.append(a[2])
        return real(*a, **k)

    monkeypatch.setattr(ex, "_pd_margin_chunks", spy)
    for name, kw in variants.items():
        fast[name] = m.partial_dependence(fr, **{**calls, **kw})
    assert len(launches) == sum(len(t) for t in fast.values())           # every table came from the kernel
    monkeypatch.setattr(ex, "_pd_device_matrix", lambda *a, **k: None)
    n0 = len(launches)
    for name, kw in variants.items():
        slow = m.partial_dependence(fr, **{**calls, **kw})
        print(m.algo, name)
        for a, b in zip(fast[name], slow):
            if name == "weights":
                _compare_tables(a, b, N_SCORE, float(w.sum()), int((w > 0).sum()), R, 3.0)
            elif name == "row_index":
                _compare_tables(a, b, 1, 1.0, 1, R)
                assert all(r["stddev_response"] == 0.0 for r in a["data"])
            else:
                _compare_tables(a, b, N_SCORE, float(N_SCORE), N_SCORE, R)
    assert len(launches) == n0
    cpu = m.partial_dependence(case["score_cpu"], cols=["f0"], nbins=7, target=target)[0]
    d = max(abs(a["mean_response"] - b["mean_response"]) for a, b in zip(fast["1-D"][0]["data"], cpu["data"]))
    print(f"{m.algo}: max |device mean - CPU frame mean| = {d:.3e} (float64 leaf sums on the CPU)")
    assert d <= 1e-5 * max(R, 1.0)


def _parent_ice(model, frame, col, nbins=20, target=None, max_rows=1000):
    """``ice`` as it stood before the sweep kernel: one predict_raw per grid value."""
    frame = model.adapt_frame(frame)
    n = min(frame.nrows, int(max_rows))
    sub = frame.rows(torch.arange(n, device=frame.device))
    v = sub.vec(col)
    if v.vtype == ENUM:
        dom = list(model.feature_domains.get(col) or v.domain or [])
        grid = list(range(len(dom)))
        labels = dom
    else:
        x = v.as_float()
        ok = ~torch.isnan(x)
        lo, hi = (float(x[ok].min()), float(x[ok].max())) if bool(ok.any()) else (0.0, 0.0)
        grid = list(np.linspace(lo, hi, nbins)) if hi > lo else [lo]
        labels = grid
    curves = []
    for g in grid:
        if v.vtype == ENUM:
            nv = Vec(col, torch.full((n,), int(g), dtype=torch.int32, device=v.data.device), ENUM, list(dom))
        else:
            nv = Vec(col, torch.full((n,), float(g), dtype=torch.float32, device=v.data.device), v.vtype)
        fr = Frame([nv if u.name == col else u for u in sub.vecs])
        curves.append(_response(model, model.predict_raw(fr), target).double().cpu())
    C = torch.stack(curves, 1).numpy()
    return {"column": col, "grid": labels, "curves": C.tolist(), "mean": C.mean(0).tolist()}


def test_ice_is_unchanged(case, monkeypatch):
    m, fr, target = case["m"], case["score"], case["target"]
    launches = []
    real = ex._pd_margins_device

    def spy(*a, **k):
        launches.append(a[2])
        return real(*a, **k)

    monkeypatch.setattr(ex, "_pd_margins_device", spy)
    for col in ("f0", "e"):
        got = m.ice(fr, col, nbins=9, target=target)
        want = _parent_ice(m, fr, col, 9, target)
        assert got["grid"] == want["grid"] and got["curves"] == want["curves"] and got["mean"] == want["mean"]
    assert launches == [FS, FE]
