"""ops.uplift kernels against plain numpy references: histogram, split scan, routing and
scoring are exact; the split scan's gain is compared with a np.longdouble scan."""
import numpy as np
import pytest
import torch

from h2omx.frame.frame import ENUM, Frame, Vec
from h2omx.models import H2OUpliftRandomForestEstimator
from h2omx.ops import uplift as uplift_ops

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _codes(rng, n, F, nbt):
    c = rng.integers(0, nbt, (F, -(-n // 64) * 64)).astype(np.uint8)
    c[:, ::7] = nbt - 1                                   # NA codes
    return c


@pytest.mark.parametrize("n,F,nbt,S,lds", [(1, 1, 3, 1, True), (333, 5, 22, 3, True), (4097, 33, 256, 1, True),
                                           (4097, 5, 256, 40, False), (4097, 5, 256, 16, True)])   # last: 64 KB of LDS
def test_category_hist(cuda_dev, n, F, nbt, S, lds):
    rng = np.random.default_rng(n + S)
    codes = _codes(rng, n, F, nbt)
    slot = rng.integers(0, max(S - 1, 1), n)              # S > 1: the last slot has no rows
    key = np.where(rng.random(n) < 0.3, -1, slot * 4 + rng.integers(0, 4, n)).astype(np.int32)
    key[0] = 1
    on = key >= 0
    ref = np.zeros((S, F, nbt, 4), np.int64)
    for f in range(F):
        idx = ((key[on] // 4 * F + f) * nbt + codes[f, :n][on]) * 4 + key[on] % 4
        ref += np.bincount(idx, minlength=ref.size).reshape(ref.shape)
    assert uplift_ops.hist_lds(S, nbt) == lds
    H = uplift_ops.category_hist(_dev(codes, cuda_dev), _dev(key, cuda_dev), S, nbt)
    H2 = uplift_ops.category_hist(_dev(codes, cuda_dev), _dev(key, cuda_dev), S, nbt)
    assert H.dtype == torch.int32 and np.array_equal(H.cpu().numpy(), ref) and torch.equal(H, H2)


def _amp(p, q, metric):
    """Divergence in longdouble and the size of its terms taken without cancellation."""
    lo, hi = LD(1e-6), LD(1.0 - 1e-6)
    p_, q_ = np.clip(p, lo, hi), np.clip(q, lo, hi)
    if metric == "KL":
        a, b = np.log(p_ / q_), np.log((1 - p_) / (1 - q_))
        return p_ * a + (1 - p_) * b, p_ * abs(a) + (1 - p_) * abs(b) + 1 + (1 - p_) / (1 - q_)
    if metric == "Euclidean":
        return 2 * (p - q) ** 2, 2 * (p + q) ** 2
    return (p - q) ** 2 / q_ + (p - q) ** 2 / (1 - q_), (p + q) ** 2 * (1 / q_ + 1 / (1 - q_) ** 2)


def _scan(H, fmask, nvb, metric, min_rows):
    """One node H [F][nbt][4]: gains, error bounds and left counts over [2 na_left][F][bin]."""
    st = np.stack([H[..., 0] + H[..., 1], H[..., 1], H[..., 2] + H[..., 3], H[..., 3]])     # [4][F][nbt]
    nb = H.shape[1] - 1
    T = st[:, 0, :].sum(-1)
    cum = np.cumsum(st[..., :nb], -1)
    L = np.stack([cum, cum + st[..., nb:]], 1)                                              # [4][2][F][nb]
    R = T[:, None, None, None] - L
    nL, nR = L[0] + L[2], R[0] + R[2]
    ok = ((nL >= min_rows) & (nR >= min_rows) & (L[0] > 0) & (L[2] > 0) & (R[0] > 0) & (R[2] > 0)
          & (np.arange(nb) < nvb[:, None] - 1) & fmask[:, None])
    rat = lambda y, n, fb: np.where(n > 0, y.astype(LD) / np.maximum(n, 1), fb)
    pn, qn = rat(T[1], T[0], LD(0)), rat(T[3], T[2], LD(0))
    (dn, an), ntot = _amp(pn, qn, metric), LD(max(T[0] + T[2], 1))
    dL, aL = _amp(rat(L[1], L[0], pn), rat(L[3], L[2], qn), metric)
    dR, aR = _amp(rat(R[1], R[0], pn), rat(R[3], R[2], qn), metric)
    G = np.where(ok, (nL * dL + nR * dR) / ntot - dn, -np.inf)
    return G, 64 * U * (1 + (nL * aL + nR * aR) / ntot + an), L.transpose(1, 2, 3, 0), T


@pytest.mark.parametrize("metric", ["KL", "Euclidean", "ChiSquared"])
@pytest.mark.parametrize("nb", [2, 21, 255])
@pytest.mark.parametrize("F", [1, 5, 33])
@pytest.mark.parametrize("K", [1, 7])
def test_best_splits(cuda_dev, K, F, nb, metric):
    """Bound on |gain - oracle| at one candidate.  With u = 2^-53: a ratio carries u; p - q
    carries 2 u (p + q), its square 5 u (p + q)^2; 1 - q_ carries u absolutely, so a quotient
    by it u / (1 - q_) relatively; a log's argument carries up to u (3 + 1 / (1 - p_) +
    1 / (1 - q_)), which the log turns into an absolute error, plus one ulp of the library
    log.  Each divergence is therefore within 11 u of its `amplitude` (_amp: its terms
    without cancellation, the clamped denominators squared where they are differences), and
    the two products, the sum, the quotient and the difference of the gain add 5 u of the
    same size.  The test allows 64 u (1 + weighted amplitudes).  A split has to be the
    oracle's where the oracle's best gain leads every other partition by twice the largest
    bound of the node, which the test asserts for every node."""
    rng = np.random.default_rng(1000 * K + 10 * F + nb)
    min_rows = 5.0
    H = np.zeros((K, F, nb + 1, 4), np.int64)
    for k in range(K):
        m = (400, 12, 400, 400, 3, 400, 25)[k]            # 12: only min_rows decides; 3: no valid split
        cat = rng.integers(0, 4, m)
        for f in range(F):
            c = np.where(rng.random(m) < 0.1, nb, rng.integers(0, nb, m))
            if k == 3:                                    # no treated rows right of the middle
                c = np.where(cat < 2, rng.integers(0, max(nb // 2, 1), m), c)
            H[k, f] = np.bincount(c * 4 + cat, minlength=(nb + 1) * 4).reshape(nb + 1, 4)
    nvb = rng.integers(1, nb + 2, F)
    nvb[0] = nb + 1
    fmask = rng.random((K, F)) < 0.7
    fmask[np.arange(K), rng.integers(0, F, K)] = True
    if F >= 5:                                            # a duplicated feature: the tie goes to feature 1
        H[:, 3], nvb[3] = H[:, 1], nvb[1]
        fmask[:, [1, 3]] = True
        fmask[0 if K == 1 else 5] = np.isin(np.arange(F), [1, 3])
        nvb[[1, 3]] = nb + 1                              # that node: only the twins are on, the tie decides
    rec = uplift_ops.split_records(uplift_ops.best_splits(
        _dev(H.astype(np.int32), cuda_dev), _dev(fmask, cuda_dev), _dev(nvb.astype(np.int32), cuda_dev), metric, min_rows))
    for k in range(K):
        G, bound, L, T = _scan(H[k], fmask[k], nvb, metric, min_rows)
        got = (int(rec["na_left"][k]), int(rec["feat"][k]), int(rec["bin"][k]))
        assert np.array_equal(rec["node"][k], T) and np.array_equal(rec["left"][k], L[got])
        if not np.isfinite(G).any():
            assert rec["gain"][k] == -np.inf and got == (0, 0, 0)
            continue
        best = np.unravel_index(np.argmax(G), G.shape)    # the first maximum: lowest (na_left, feature, bin)
        other = (L != L[best]).any(-1) & (L != T - L[best]).any(-1)
        lead = G[best] - np.max(np.where(other, G, -np.inf))
        assert lead > 2 * bound[np.isfinite(G)].max(), (k, lead)
        assert got == best and (F < 5 or k != (0 if K == 1 else 5) or best[1] == 1)
        assert abs(LD(rec["gain"][k]) - G[got]) <= bound[got]
    assert K == 1 or rec["gain"][4] == -np.inf


@pytest.mark.parametrize("n", [1, 333, 4097])
def test_route(cuda_dev, n):
    rng = np.random.default_rng(n)
    F, nbt, K = 5, 22, 6
    codes = _codes(rng, n, F, nbt)
    nid = np.where(rng.random(n) < 0.2, -1, rng.integers(0, K, n)).astype(np.int32)
    nid[0] = 0
    cat = np.where(nid >= 0, rng.integers(0, 4, n), -1).astype(np.int32)
    remap = np.array([0, -1, 1, 2, -1, 3], np.int32)      # nodes 1 and 4 did not split
    br = np.array([0, 1, 1, 0], np.int32)
    feat, binv, nal = rng.integers(0, F, K), rng.integers(0, nbt - 1, K), np.array([0, 1, 1, 0, 1, 0])
    rec = np.zeros((K, uplift_ops.REC_INTS), np.int32)
    rec[:, 2], rec[:, 3], rec[:, 4] = feat, binv, nal
    k = np.maximum(nid, 0)
    c = codes[feat[k], np.arange(n)].astype(np.int64)
    right = np.where(c == nbt - 1, nal[k] == 0, c > binv[k])
    new = np.where((nid >= 0) & (remap[k] >= 0), 2 * remap[k] + right, -1)
    slot = np.where((new >= 0) & ((new & 1) == br[np.maximum(new >> 1, 0)]), new >> 1, -1)
    nid_d = _dev(nid, cuda_dev)
    key = uplift_ops.route(_dev(codes, cuda_dev), nid_d, _dev(cat, cuda_dev), _dev(rec, cuda_dev), _dev(remap, cuda_dev),
                           _dev(br, cuda_dev), nbt)
    assert np.array_equal(nid_d.cpu().numpy(), new) and np.array_equal(key.cpu().numpy(), np.where(slot >= 0, slot * 4 + cat, -1))


def _tree(rng, F, nbt, depth):
    """A random tree of exactly `depth` levels of splits, children behind their parent."""
    t = {k: [] for k in ("feat", "bin", "na_left", "left", "pt", "pc")}
    level = [0]
    for d in range(depth + 1):
        nxt = []
        for j, _ in enumerate(level):
            inner = d < depth and (j == 0 or rng.random() < 0.45)
            left = len(level) - j + len(t["feat"]) + len(nxt) if inner else -1
            for key, v in zip(t, (rng.integers(0, F) if inner else -1, rng.integers(0, nbt - 1), rng.integers(0, 2), left,
                                  rng.random(), rng.random())):
                t[key].append(v)
            nxt += [left, left + 1] if inner else []
        level = nxt
    return {k: np.array(v, np.float64 if k in ("pt", "pc") else np.int32) for k, v in t.items()}


@pytest.mark.parametrize("n,F,ntrees,depth", [(1, 1, 1, 0), (333, 5, 7, 4), (4097, 5, 50, 20), (333, 300, 3, 6),
                                                (333, 256, 3, 6)])   # last: 64 KB of LDS
def test_forest_predict(cuda_dev, n, F, ntrees, depth):
    rng = np.random.default_rng(n + F)
    nbt = 22
    codes = _codes(rng, n, F, nbt)
    trees = [_tree(rng, F, nbt, depth if i % 3 == 0 else depth // 2) for i in range(ntrees)]
    ref, rows = np.zeros((2, n)), np.arange(n)
    for t in trees:
        nid = np.zeros(n, np.int64)
        for _ in range(depth):
            f = t["feat"][nid]
            c = codes[np.maximum(f, 0), rows]
            right = np.where(c == nbt - 1, t["na_left"][nid] == 0, c > t["bin"][nid])
            nid = np.where(f >= 0, t["left"][nid] + right, nid)
        ref[0] += t["pt"][nid]
        ref[1] += t["pc"][nid]
    pt, pc = uplift_ops.forest_predict(_dev(codes, cuda_dev), uplift_ops.pack_forest(trees, cuda_dev, nbt), n)
    assert np.array_equal(pt.cpu().numpy(), ref[0]) and np.array_equal(pc.cpu().numpy(), ref[1])


@pytest.mark.parametrize("metric", ["Euclidean", "ChiSquared", "KL"])
def test_fit_matches_tensor_route(cuda_dev, monkeypatch, metric):
    """Node for node the trees of _grow_torch, and predict_raw equal to _predict_raw_torch.
    Euclidean and ChiSquared gains are the same IEEE operations on both routes.  KL: exact
    equality is the contract here too, with no gap precondition: both routes call the device
    library's log on equal arguments, so equal bits are expected; a failure for KL alone
    means the two logs differ, or differ at a near-tie of two partitions."""
    g = torch.Generator().manual_seed(0)
    n = 3000
    X = torch.randn((4, n), generator=g)
    t = (torch.rand(n, generator=g) < 0.5).float()
    p = (torch.sigmoid(X[1] * 0.5) * 0.6 + t * torch.where(X[0] > 0, 0.3, -0.1)).clamp(0.02, 0.98)
    y = (torch.rand(n, generator=g) < p).int()
    fr = Frame([Vec(f"x{i}", X[i].to(cuda_dev), "real") for i in range(4)]
               + [Vec("treatment", t.int().to(cuda_dev), ENUM, ["control", "treatment"]),
                  Vec("y", y.to(cuda_dev), ENUM, ["0", "1"])])
    kw = dict(ntrees=3, max_depth=4, seed=1, treatment_column="treatment", sample_rate=0.632, mtries=2,
              uplift_metric=metric)
    m = H2OUpliftRandomForestEstimator(**kw).train(y="y", training_frame=fr)
    assert m.timings["tree_engine"] == "hip" and m.timings["score_engine"] == "hip"
    monkeypatch.setattr(H2OUpliftRandomForestEstimator, "tree_engine", lambda self, codes: "torch")
    ref = H2OUpliftRandomForestEstimator(**kw).train(y="y", training_frame=fr)
    assert ref.timings["tree_engine"] == "torch" and len(m.trees) == len(ref.trees) == 3
    for a, b in zip(m.trees, ref.trees):
        assert max(len(a["feat"]), len(b["feat"])) > 1
        for k in ("feat", "bin", "na_left", "left", "pt", "pc"):
            assert np.array_equal(a[k], b[k]), k
    assert torch.equal(m.predict_raw(fr), m._predict_raw_torch(fr))
