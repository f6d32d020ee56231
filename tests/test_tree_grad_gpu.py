"""The gradient-pass kernels called directly, against tests/gradref.py:
``h2omx_boost_update`` (dist_grad for all nine distributions, tree apply,
bagging, node-id reset, per-block maxima + ``h2omx_stat_reduce``, the next
tree's packed rows, the tree archive ring), ``h2omx_softmax_grad``,
``h2omx_apply_tree`` and ``h2omx_oob_accumulate``.

The tests own every buffer.  Each output buffer carries 64 sentinel elements
past ``npad`` (n rounded up to 64) that must come back untouched.  The exact
class (gaussian, laplace, quantile, huber, drf) must match the float32
reference bit for bit, the others the float64 reference within
``tol = C * M * w`` (see gradref).  Bag weights use a seed with the top bit
set, a tree index above 2^16 and a row base of 2^32 - 500, so the 32-bit wrap
of the row id falls inside the rows.

Worst err / tol on the MI355X (the assertion is err <= tol):

    boost_update, n = 1027     bernoulli 0.250, poisson 0.183, gamma 0.161, tweedie (power 1.2) 0.215
    boost_update, n = 4195331  bernoulli 0.276
    softmax_grad, n = 1027     K = 2: 0.354, K = 3: 0.407, K = 7: 0.377
    softmax_grad, n = 1049603  K = 3: 0.431

and 0 for gaussian, laplace, quantile, huber and drf, which match bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import gradref as GR
import quantref as Q
from h2omx.models.tree.engine import make_grad_params
from h2omx.models.tree.structs import TREE_NODE_DTYPE
from h2omx.reference.tree import bag_weights

pytestmark = pytest.mark.gpu

SENT = 64
F_SENT = np.float32(-1.2345e30)
I_SENT = 0x5A5A5A5A
B_SENT = 0xA5
INT32_MIN = -(2 ** 31)
SEED, TREE_INDEX, ROW_BASE, RATE, SALT = 0x9E3779B5, 70001, 2 ** 32 - 500, 0.632, 123457
PARAMS = dict(tweedie_power=1.2, quantile_alpha=0.3, huber_delta=0.8)
CAP = 37
F_PAD, W_PAD = np.float32(3.5), np.float32(0.25)     # what the padding rows of the inputs hold
N_SMALL = 1027                                       # tail inside a float4, 61 padding rows
N_STRIDE = 4 * 4096 * 256 + 1027                     # boost_update's grid-stride loop takes a second trip


def _npad(n):
    return -(-n // 64) * 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _tree():
    """leaves with distinct values (multiples of 1/64: sums with such margins are exact)"""
    t = np.zeros(CAP, TREE_NODE_DTYPE)
    t["feat"], t["left"] = -1, -1
    t["value"] = (np.arange(CAP) - CAP // 2) / 64.0
    t["weight"] = np.arange(CAP) + 1
    return t


def _guarded(dev, a, sent):
    """device copy of ``a`` followed by 64 sentinel elements"""
    return torch.from_numpy(np.concatenate([a, np.full(SENT, sent, a.dtype)])).to(dev)


def _filled(dev, size, dtype, sent):
    return _guarded(dev, np.full(size, sent, dtype), sent)


def _margins(dist, rng, n, npad):
    F = np.full(npad, F_PAD, np.float32)
    if dist == "bernoulli":
        F[:n] = rng.uniform(-30, 30, n)
        F[:8] = [100, 100, -100, -100] * 2          # saturated: p is exactly 1 / 0
    elif dist == "poisson":
        F[:n] = rng.uniform(-6, 6, n)
    elif dist in ("gamma", "tweedie"):
        F[:n] = rng.uniform(-5, 5, n)
    else:
        F[:n] = 2 * rng.normal(size=n)
        F[:96] = rng.integers(-8, 9, 96) / 64.0     # rows whose comparisons hit equality
        F[96:100] = -0.0
    return F


def _response(dist, fa, rng):
    """y per row of margins ``fa`` (what dist_grad sees), with the edges of each distribution"""
    n = fa.size
    if dist in ("gaussian", "laplace", "quantile"):
        y = (fa + rng.normal(size=n)).astype(np.float32)
        y[:32] = fa[:32]                            # f == y: gaussian 0, laplace 0, quantile 1 - alpha
        y[96:100] = 0.0
    elif dist == "huber":
        d = np.float32(PARAMS["huber_delta"])
        y = (fa + 2 * rng.normal(size=n)).astype(np.float32)
        y[:32], y[32:64], y[64:96] = fa[:32] - d, fa[32:64] + d, fa[64:96]
    elif dist == "drf":
        y = (rng.random(n) < 0.5).astype(np.float32)
        y[:2] = -0.0
    elif dist == "bernoulli":
        y = (rng.random(n) < 0.5).astype(np.float32)
        y[:8] = [0, 1] * 4
    elif dist == "poisson":
        y = rng.poisson(np.exp(np.clip(fa, -3, 3))).astype(np.float32)
    elif dist == "gamma":
        y = (10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)      # four decades
    else:
        y = rng.gamma(2, np.exp(np.clip(0.5 * fa, -3, 3)) / 2).astype(np.float32)
        y[rng.random(n) < 0.3] = 0.0
    return y


def _qs(ref, s_is_h):
    """power-of-two scales that keep the packed fields inside 16 bits, row base and salt where tree_begin puts them"""
    qs = np.zeros(16, np.float64)
    gmax = max(float(np.abs(ref.g).max()), 1e-30)
    smax = max(float((ref.h if s_is_h else ref.w).max()), 1e-30)
    qs[0], qs[1] = Q._pow2_floor(8192.0 / gmax), Q._pow2_floor(16384.0 / smax)
    qs[2], qs[3], qs[7], qs[9] = 1.0 / qs[0], 1.0 / qs[1], ROW_BASE, SALT
    return qs


def _boost(dev, F, y, wobs, n, dist, *, apply=0, leaf=None, rate=1.0, skip_nid=0, store_gh=1, y8=False, nid16=False,
           nid_in=None, slab=None, qs=None, s_is_h=0, ring=False, row_base=ROW_BASE):
    """One h2omx_boost_update + h2omx_stat_reduce on buffers of our own; every buffer back as a host array."""
    from h2omx import ops

    lib, P, npad = ops.tree_lib(), ops.P, F.size
    gp = make_grad_params(dist, bool(apply), rate, SEED, TREE_INDEX, row_base=row_base, **PARAMS)
    gp.skip_nid = skip_nid
    tree = _tree()
    tree_d = torch.from_numpy(tree.view(np.uint8).copy()).to(dev)
    nid_h = np.full(npad, INT32_MIN, np.int32) if nid_in is None else nid_in.copy()
    if leaf is not None and nid_in is None:
        nid_h[:n] = ~leaf
    t = dict(F=_guarded(dev, F, F_SENT), nid=_guarded(dev, nid_h, I_SENT),
             g=_filled(dev, npad, np.float32, F_SENT), h=_filled(dev, npad, np.float32, F_SENT),
             wout=_filled(dev, npad, np.float32, F_SENT), stat=_filled(dev, 4, np.int32, I_SENT),
             slab=slab if slab is not None else _guarded(dev, np.zeros(4096 * 4, np.int32), I_SENT))
    assert lib.h2omx_stat_blocks() == 4096
    yd = torch.from_numpy(y).to(dev)
    wd = None if wobs is None else torch.from_numpy(wobs).to(dev)
    y8d = torch.from_numpy(y.astype(np.uint8)).to(dev) if y8 else None
    n16 = None
    if nid16:
        h16 = np.full(npad, -32768, np.int16)
        h16[:n] = ~leaf
        n16 = torch.from_numpy(h16).to(dev)
    qd = None
    if qs is not None:
        qd = torch.from_numpy(qs).to(dev)
        t["pk"] = _filled(dev, npad, np.int32, I_SENT)
    ctr = None
    if ring:
        t["ring"] = _filled(dev, 3 * tree.nbytes, np.uint8, B_SENT)
        ctr = torch.tensor([13], dtype=torch.int32, device=dev)      # (13 - 2) mod 3: slot 2, wrapped
    s = ops.stream(dev)
    ops.check(lib.h2omx_boost_update(P(t["F"]), P(yd), P(wd), n, npad, P(t["nid"]), P(tree_d), ctypes.addressof(gp),
                                     P(t["g"]), P(t["h"]), P(t["wout"]), P(t["slab"]), tree.nbytes, P(t.get("ring")),
                                     3 if ring else 0, P(ctr), 2 if ring else 0, P(t.get("pk")), P(qd), s_is_h,
                                     store_gh, P(y8d), P(n16), s), "boost_update")
    ops.check(lib.h2omx_stat_reduce(P(t["slab"]), P(t["stat"]), s), "stat_reduce")
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["slab_dev"], out["tree"] = t["slab"], tree
    return out


def _check_tails(o, npad):
    for k, sent in (("F", F_SENT), ("g", F_SENT), ("h", F_SENT), ("wout", F_SENT), ("nid", I_SENT), ("pk", I_SENT)):
        if k in o:
            assert o[k].size == npad + SENT and (o[k][npad:] == sent).all(), f"{k}: wrote past npad"
    assert (o["stat"][4:] == I_SENT).all() and (o["slab"][4096 * 4:] == I_SENT).all()
    if "ring" in o:
        assert (o["ring"][3 * o["tree"].nbytes:] == B_SENT).all()


def _check_maxima(o, npad):
    """stat_max holds the float bits of the maxima of the kernel's own outputs"""
    mx = np.array([np.abs(o["g"][:npad]).max(), o["h"][:npad].max(), o["wout"][:npad].max()], np.float32)
    assert o["stat"][:3].tolist() == _bits(mx).tolist() and o["stat"][3] == 0, (o["stat"][:4], _bits(mx))


def _check_pk(o, n, npad, qs, s_is_h):
    """the packed rows are the quantisation model's, from the kernel's own (g, h, w)"""
    gq, sq = Q.quantised_rows(o["g"][:n], o["h"][:n], o["wout"][:n], s_is_h, qs, ROW_BASE, SALT)
    assert np.abs(gq).max() < 2 ** 15 and 0 <= sq.min() and sq.max() < 2 ** 16
    assert np.array_equal(o["pk"][:n].view(np.uint32), Q.packed_rows(gq, sq, True)), "packed rows"
    assert (o["pk"][n:npad] == 0).all(), "packed padding rows"
    x = o["g"][:n].astype(np.float64) * qs[0]
    if (x != np.floor(x)).sum() > 64:       # (laplace / quantile / drf without weights: integers, nothing to dither)
        assert (gq != np.floor(x)).any(), "dither had no effect"


def _check_rows(o, n, npad, F_in, fa, ref, what):
    """F, g, h, wout, nid of live and padding rows; returns the worst err / tol"""
    _check_tails(o, npad)
    assert np.array_equal(_bits(o["F"][:n]), _bits(fa)), f"{what}: margins"
    assert np.array_equal(_bits(o["F"][n:npad]), _bits(F_in[n:])), f"{what}: padding margins"
    for k in ("g", "h", "wout"):
        assert (_bits(o[k][n:npad]) == 0).all(), f"{what}: padding {k}"
    assert (o["nid"][:n] == 0).all() and (o["nid"][n:npad] == INT32_MIN).all(), f"{what}: nid"
    return ref.compare(o["g"][:n], o["h"][:n], o["wout"][:n], what)


def _check_saturated(o, fa, y, w):
    """bernoulli beyond |f| = 89: g is -y or 1 - y, h the floor, times w, exactly"""
    sat = np.abs(fa) >= GR.BERNOULLI_SATURATED
    assert sat.sum() >= 8
    pr = (fa[sat] > 0).astype(np.float32)
    assert np.array_equal(_bits(o["g"][: fa.size][sat]), _bits((pr - y[sat]) * w[sat]))
    assert np.array_equal(_bits(o["h"][: fa.size][sat]), _bits(GR.H_FLOOR * w[sat]))


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dist", GR.DISTS)
def test_boost_update(cuda_dev, dist, weighted):
    """Two launches per case.  A: apply_tree 0, no bag, packed rows with s = w.
    B: apply_tree 1, bag of 63.2 % across the 2^32 row-id wrap, packed rows
    with s = h, the tree archived to slot (13 - 2) mod 3 of a 3-slot ring."""
    n, npad = N_SMALL, _npad(N_SMALL)
    rng = np.random.default_rng(100 + GR.DISTS.index(dist))
    F = _margins(dist, rng, n, npad)
    leaf = rng.integers(0, CAP, n)
    wobs = None
    if weighted:
        wobs = np.full(npad, W_PAD, np.float32)
        wobs[:n] = rng.uniform(0.5, 2.0, n)
    tree = _tree()
    worst = 0.0
    for apply in (0, 1):
        fa = F[:n] + tree["value"][leaf] if apply else F[:n].copy()
        assert fa.dtype == np.float32
        y = np.zeros(npad, np.float32)
        y[:n] = _response(dist, fa, rng)
        rate = RATE if apply else 1.0
        ref = GR.grad_pass(fa, y[:n], None if wobs is None else wobs[:n], dist, PARAMS, rate, SEED, TREE_INDEX,
                           ROW_BASE)
        assert ref.exact == (dist in GR.EXACT)
        if dist == "huber":
            d = np.float32(PARAMS["huber_delta"])
            assert ((fa - y[:n]) == d).sum() >= 4 and ((fa - y[:n]) == -d).sum() >= 4, "no |f - y| == delta rows"
        qs = _qs(ref, apply)
        o = _boost(cuda_dev, F, y, wobs, n, dist, apply=apply, leaf=leaf, rate=rate, qs=qs, s_is_h=apply,
                   ring=bool(apply))
        what = f"{dist} apply {apply}"
        worst = max(worst, _check_rows(o, n, npad, F, fa, ref, what))
        if apply:
            # bagging: exactly the hash's rows, on both sides of the 32-bit wrap of the row id
            bag = bag_weights(n, RATE, SEED, TREE_INDEX, ROW_BASE)
            assert 0.3 < (bag[:500] == 0).mean() < 0.45 and 0.3 < (bag[500:] == 0).mean() < 0.45
            assert np.array_equal(o["wout"][:n], bag if wobs is None else wobs[:n] * bag)
            assert not np.array_equal(bag, bag_weights(n, RATE, SEED, TREE_INDEX, 0))
            ring = o["ring"][: 3 * tree.nbytes].reshape(3, -1)
            assert ring[2].tobytes() == tree.tobytes() and (ring[:2] == B_SENT).all(), "tree archive"
        else:
            assert np.array_equal(o["wout"][:n], np.ones(n, np.float32) if wobs is None else wobs[:n])
        if dist == "bernoulli":
            _check_saturated(o, fa, y[:n], ref.w)
        _check_maxima(o, npad)
        _check_pk(o, n, npad, qs, apply)
    print(f"boost_update {dist} {'weighted' if weighted else 'unweighted'}: worst err / tol {worst:.3f}")


def test_boost_update_switches(cuda_dev):
    """skip_nid, store_gh 0, byte labels and int16 leaf ids against the plain launch"""
    n, npad, dist = N_SMALL, _npad(N_SMALL), "bernoulli"
    rng = np.random.default_rng(7)
    F = _margins(dist, rng, n, npad)
    leaf = rng.integers(0, CAP, n)
    fa = F[:n] + _tree()["value"][leaf]
    y = np.zeros(npad, np.float32)
    y[:n] = _response(dist, fa, rng)
    ref = GR.grad_pass(fa, y[:n], None, dist, PARAMS, RATE, SEED, TREE_INDEX, ROW_BASE)
    qs = _qs(ref, 1)
    kw = dict(apply=1, leaf=leaf, rate=RATE, qs=qs, s_is_h=1)
    base = _boost(cuda_dev, F, y, None, n, dist, **kw)
    _check_rows(base, n, npad, F, fa, ref, "plain")
    _check_pk(base, n, npad, qs, 1)
    same = ("F", "g", "h", "wout", "nid", "stat", "pk")
    for name, extra in (("y8", dict(y8=True)), ("nid16", dict(nid16=True))):
        o = _boost(cuda_dev, F, y, None, n, dist, **kw, **extra)
        for k in same:
            assert o[k].tobytes() == base[k].tobytes(), (name, k)
    o = _boost(cuda_dev, F, y, None, n, dist, **kw, skip_nid=1)
    assert o["nid"][:n].tolist() == (~leaf).tolist() and (o["nid"][n:npad] == INT32_MIN).all(), "skip_nid wrote nid"
    for k in ("F", "g", "h", "wout", "stat", "pk"):
        assert o[k].tobytes() == base[k].tobytes(), ("skip_nid", k)
    o = _boost(cuda_dev, F, y, None, n, dist, **kw, store_gh=0)
    assert (o["g"] == F_SENT).all() and (o["h"] == F_SENT).all(), "store_gh 0 stored (g, h)"
    for k in ("F", "wout", "nid", "stat", "pk"):
        assert o[k].tobytes() == base[k].tobytes(), ("store_gh 0", k)


def test_maxima_of_a_second_launch(cuda_dev):
    """every block rewrites its slot of the maxima slab: a launch of few rows
    with small gradients after one of many rows with large gradients reports
    its own maxima"""
    dist = "gaussian"
    rng = np.random.default_rng(9)
    n1, n2 = 300_001, N_SMALL
    slab = None
    for n, scale in ((n1, 64.0), (n2, 2.0 ** -6)):
        npad = _npad(n)
        F = np.full(npad, F_PAD, np.float32)
        F[:n] = scale * rng.normal(size=n)
        y = np.zeros(npad, np.float32)
        wobs = np.full(npad, W_PAD, np.float32)
        wobs[:n] = scale * rng.uniform(0.5, 2.0, n)
        o = _boost(cuda_dev, F, y, wobs, n, dist, slab=slab)
        slab = o["slab_dev"]
        ref = GR.grad_pass(F[:n], y[:n], wobs[:n], dist, PARAMS)
        _check_rows(o, n, npad, F, F[:n], ref, f"launch of {n}")
        _check_maxima(o, npad)
        assert (o["slab"][: 4096 * 4].reshape(4096, 4)[:, 0] != 0).sum() == -(-npad // 1024)
    assert o["stat"][:3].view(np.float32)[0] < 1.0


@pytest.mark.parametrize("dist", ["gaussian", "bernoulli"])
def test_boost_update_grid_stride(cuda_dev, dist):
    """more than 4096 x 256 x 4 rows: the lanes' second trip, every row checked"""
    n, npad = N_STRIDE, _npad(N_STRIDE)
    rng = np.random.default_rng(13)
    F = np.full(npad, F_PAD, np.float32)
    F[:n] = rng.uniform(-30, 30, n) if dist == "bernoulli" else 2 * rng.normal(size=n)
    leaf = rng.integers(0, CAP, n)
    fa = F[:n] + _tree()["value"][leaf]
    y = np.zeros(npad, np.float32)
    y[:n] = (rng.random(n) < 0.5) if dist == "bernoulli" else fa + rng.normal(size=n).astype(np.float32)
    wobs = np.full(npad, W_PAD, np.float32)
    wobs[:n] = rng.uniform(0.5, 2.0, n)
    ref = GR.grad_pass(fa, y[:n], wobs[:n], dist, PARAMS, RATE, SEED, TREE_INDEX, ROW_BASE - n)
    qs = _qs(ref, 1)
    o = _boost(cuda_dev, F, y, wobs, n, dist, apply=1, leaf=leaf, rate=RATE, qs=qs, s_is_h=1, row_base=ROW_BASE - n)
    ratio = _check_rows(o, n, npad, F, fa, ref, dist)
    _check_maxima(o, npad)
    _check_pk(o, n, npad, qs, 1)
    assert (o["slab"][: 4096 * 4].reshape(4096, 4)[:, 2] != 0).all(), "idle blocks"
    print(f"boost_update {dist} n {n}: worst err / tol {ratio:.3f}")


# ---- softmax -------------------------------------------------------------------

def _softmax_case(cuda_dev, K, n, weighted):
    from h2omx import ops

    lib, P, dev = ops.tree_lib(), ops.P, cuda_dev
    npad = _npad(n)
    ldF = npad + 192
    rng = np.random.default_rng(20 + K)
    Fm = np.full((K, ldF), F_PAD, np.float32)
    Fm[:, :n] = rng.uniform(-40, 40, (K, n))
    Fm[:, n // 2: n] *= 0.03                       # half the rows with comparable classes
    Fm[:, 5] = 1.25                                # all classes equal
    yk = np.zeros(npad, np.int32)
    yk[:n] = rng.integers(0, K, n)
    wobs, rate = None, 1.0
    if weighted:
        wobs = np.full(npad, W_PAD, np.float32)
        wobs[:n] = rng.uniform(0.5, 2.0, n)
        rate = RATE
    gp = make_grad_params("bernoulli", False, rate, SEED, TREE_INDEX, row_base=ROW_BASE, **PARAMS)
    Fd, ykd = torch.from_numpy(Fm).to(dev), torch.from_numpy(yk).to(dev)
    wd = None if wobs is None else torch.from_numpy(wobs).to(dev)
    slab = _guarded(dev, np.zeros(4096 * 4, np.int32), I_SENT)
    worst, floored = 0.0, 0
    for cls in range(K):
        t = dict(nid=_filled(dev, npad, np.int32, I_SENT), g=_filled(dev, npad, np.float32, F_SENT),
                 h=_filled(dev, npad, np.float32, F_SENT), wout=_filled(dev, npad, np.float32, F_SENT),
                 stat=_filled(dev, 4, np.int32, I_SENT), slab=slab)
        s = ops.stream(dev)
        ops.check(lib.h2omx_softmax_grad(P(Fd), K, ldF, P(ykd), P(wd), n, npad, cls, ctypes.addressof(gp),
                                         P(t["nid"]), P(t["g"]), P(t["h"]), P(t["wout"]), P(slab), s), "softmax_grad")
        ops.check(lib.h2omx_stat_reduce(P(slab), P(t["stat"]), s), "stat_reduce")
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in t.items()}
        _check_tails(o, npad)
        for k in ("g", "h", "wout"):
            assert (_bits(o[k][n:npad]) == 0).all(), f"class {cls}: padding {k}"
        assert (o["nid"][:n] == 0).all() and (o["nid"][n:npad] == INT32_MIN).all()
        ref = GR.softmax_pass(Fm[:, :n], yk[:n], None if wobs is None else wobs[:n], cls, rate, SEED, TREE_INDEX,
                              ROW_BASE)
        worst = max(worst, ref.compare(o["g"][:n], o["h"][:n], o["wout"][:n], f"K {K} class {cls}"))
        _check_maxima(o, npad)
        floored += int((ref.h == float(GR.H_FLOOR) * ref.w.astype(np.float64))[ref.w > 0].sum())
    assert np.array_equal(Fd.cpu().numpy(), Fm)
    assert floored > 0, "no row at the h floor"
    return worst


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted_bagged"])
@pytest.mark.parametrize("K", [2, 3, 7])
def test_softmax_grad(cuda_dev, K, weighted):
    """every class of K, margins spanning +-40 (p underflows, the h floor
    applies), ldF > npad, one maxima slab reused by the classes' launches"""
    worst = _softmax_case(cuda_dev, K, N_SMALL, weighted)
    print(f"softmax_grad K {K} {'weighted + bagged' if weighted else 'plain'}: worst err / tol {worst:.3f}")


def test_softmax_grad_grid_stride(cuda_dev):
    """more than 4096 x 256 rows (one row per lane): the second trip"""
    worst = _softmax_case(cuda_dev, 3, 4096 * 256 + 1027, True)
    print(f"softmax_grad K 3 n {4096 * 256 + 1027}: worst err / tol {worst:.3f}")


# ---- apply_tree, oob_accumulate ------------------------------------------------

def test_apply_tree(cuda_dev):
    from h2omx import ops

    lib, P, dev = ops.tree_lib(), ops.P, cuda_dev
    n = 70_001
    rng = np.random.default_rng(31)
    tree = _tree()
    tree["value"] = rng.normal(size=CAP)
    F = rng.normal(size=n).astype(np.float32)
    leaf = rng.integers(0, CAP, n)
    Fd = _guarded(dev, F, F_SENT)
    nid = torch.from_numpy((~leaf).astype(np.int32)).to(dev)
    tree_d = torch.from_numpy(tree.view(np.uint8).copy()).to(dev)
    ops.check(lib.h2omx_apply_tree(P(Fd), n, P(nid), P(tree_d), ops.stream(dev)), "apply_tree")
    torch.cuda.synchronize()
    got = Fd.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(F + tree["value"][leaf])) and (got[n:] == F_SENT).all()


@pytest.mark.parametrize("n", [70_001, 4096 * 256 + 1027])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_oob_accumulate(cuda_dev, n, weighted):
    """only rows the bag left out, of non-zero observation weight, that sit in
    a leaf, add the leaf's value; the count moves only when asked"""
    from h2omx import ops

    lib, P, dev = ops.tree_lib(), ops.P, cuda_dev
    rng = np.random.default_rng(37)
    tree = _tree()
    tree["value"] = rng.normal(size=CAP)
    leaf = rng.integers(0, CAP, n)
    nid = (~leaf).astype(np.int32)
    inner = rng.random(n) < 0.1
    nid[inner] = rng.integers(0, CAP, int(inner.sum()))          # not a leaf id: skipped
    wobs = None
    if weighted:
        wobs = rng.uniform(0.5, 2.0, n).astype(np.float32)
        wobs[rng.random(n) < 0.2] = 0.0
    sum0, cnt0 = rng.normal(size=n).astype(np.float32), rng.integers(0, 5, n).astype(np.float32)
    bag = bag_weights(n, RATE, SEED, TREE_INDEX, ROW_BASE - n // 2)
    add = (bag == 0) & ~inner
    if weighted:
        add &= wobs != 0
    assert 0.2 < add.mean() < 0.4
    want_sum = np.where(add, sum0 + tree["value"][np.where(inner, 0, leaf)], sum0).astype(np.float32)
    nd, tree_d = torch.from_numpy(nid).to(dev), torch.from_numpy(tree.view(np.uint8).copy()).to(dev)
    wd = None if wobs is None else torch.from_numpy(wobs).to(dev)
    for count in (0, 1):
        sd, cd = _guarded(dev, sum0, F_SENT), _guarded(dev, cnt0, F_SENT)
        ops.check(lib.h2omx_oob_accumulate(P(sd), P(cd), n, P(nd), P(tree_d), P(wd), SEED, TREE_INDEX, RATE,
                                           ROW_BASE - n // 2, count, ops.stream(dev)), "oob_accumulate")
        torch.cuda.synchronize()
        gs, gc = sd.cpu().numpy(), cd.cpu().numpy()
        assert (gs[n:] == F_SENT).all() and (gc[n:] == F_SENT).all()
        assert np.array_equal(_bits(gs[:n]), _bits(want_sum)), f"count {count}: sums"
        assert np.array_equal(gc[:n], cnt0 + add if count else cnt0), f"count {count}: counts"
