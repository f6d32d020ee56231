"""NumPy oracle of the tree engine's arithmetic on the kernels' own integers.

``h2omx/reference/tree.py`` sums unquantised float64 gradients; the kernels of
``csrc/tree_kernels.hip`` sum stochastically rounded fixed-point integers, so
the two break honest near-ties differently and can only be compared loosely.
This helper quantises the rows exactly as the kernels do (same scales, same
dither hash, same fp32 rounding) and repeats everything after that in int64 /
float64, so a GPU-built tree can be checked for EQUALITY node by node:

* scales              tree_begin / tree_begin_scales
* row quantisation    hist_build_kernel and its twins (floorf(fmaf(g, sg, d)))
* split scan          feat_scan_wave + split_gain_pt, node_best_wave
* categorical scan    feat_best_cat_wave: levels ordered by (G_int / S_int,
                      bin), every prefix a candidate, 256-bit left sets
* constraints         mono_ok in the threshold scan (the categorical scan
                      applies none); inter_ok / inter_children with istate
* finalisation        lf_decide + lf_write_node (child numbering, thr, weight,
                      the gbound intervals and clamp_bound, treecat)
* routing             part_right (a retired row carries ~gid; a categorical
                      split tests its bitset, the NA bin follows na_left)
* leaves              leaf_stats / the partitions' leaf sums + leaf_finalize,
                      and mono_newton_kernel (mode 0, Newton leaves, monotone)

Out of scope (not modelled, the tests do not use them): ``hist_mode != 0``,
N-rank runs, and levels wide enough for the host to read node counts back (the
capacity guard of lf_write_node).

Plain NumPy; no HIP code is called from here.
"""
from __future__ import annotations

import math

import numpy as np

from h2omx.models.tree.hashing import M32, _mix32
from h2omx.models.tree.structs import TREE_NODE_DTYPE, interaction_masks
from h2omx.reference.tree import feature_allowed, leaf_value

QG, QS = 32768.0, 65536.0      # per-row fixed-point ranges (QG / QS of the kernels)
LEAF_RANGE = 1073741823.0
TIE_REL = 1e-12                # candidates this close to the best gain form a near-tie


# ---------------------------------------------------------------------------
# scales
# ---------------------------------------------------------------------------
def _pow2_floor(x: float) -> float:
    """2^floor(log2 x), from the exponent (no libm rounding at powers of two)"""
    m, e = math.frexp(x)
    return math.ldexp(1.0, e - 1)


def row_ranges(max_rows_per_wg: int) -> tuple[float, float]:
    """(qg, qsr) of h2omx_tree_begin: per-row ranges that keep a workgroup
    chunk's sums below 2^30 / 2^31"""
    return _pow2_floor(1073741824.0 / max_rows_per_wg), _pow2_floor(2147483648.0 / max_rows_per_wg)


def scales(stat_bits, mode: int, max_rows_per_wg: int) -> np.ndarray:
    """qscale[0..6] from the stat_max image (float bits of max|g|, max h, max w)"""
    st = np.asarray(stat_bits).astype(np.int32).view(np.float32).astype(np.float64)
    gmax, hmax, wmax = (max(float(v), 1e-30) for v in st[:3])
    smax = wmax if mode == 0 else hmax
    qg, qsr = row_ranges(max_rows_per_wg)
    sg = _pow2_floor(min(qg, QG) / gmax)
    ss = _pow2_floor(min(qsr, QS) / smax)
    return np.array([sg, ss, 1.0 / sg, 1.0 / ss, _pow2_floor(LEAF_RANGE / gmax), _pow2_floor(LEAF_RANGE / hmax),
                     _pow2_floor(LEAF_RANGE / wmax)], np.float64)


def unit_scales() -> np.ndarray:
    """every scale 1: integer inputs stay themselves (CPU tests)"""
    return np.ones(7, np.float64)


def host_max_rows_per_wg(n: int, F: int, nbt: int, segmented: bool = False, cls=None) -> int:
    """HipTreeBuilder.max_rows_per_wg of a one-rank builder, from the host-side
    level plans alone (no device): the constructor's rule on a bare instance"""
    from h2omx.models.tree.engine import HipTreeBuilder

    cls = cls or HipTreeBuilder
    b = cls.__new__(cls)
    b.F, b.nbt, b.max_rows_per_wg = F, nbt, None
    units = max(1, -(-n // 64) * 64) // b.ROWS_PER_LANE
    cands = [b._choose(1 << k, units) for k in range(0, 13)] + [b._choose(1 << 20, units)]
    m = max(b.ROWS_PER_LANE * math.ceil(units / c["wgpg"]) for c in cands)
    if segmented:
        hc = -(-n // b.SEG_TARGET_CHUNKS)
        m = max(m, min(b.ROWS_CAP, max(2048, -(-hc // 256) * 256)))
    return m


# ---------------------------------------------------------------------------
# row quantisation
# ---------------------------------------------------------------------------
def row_hash(rows, salt: int) -> np.ndarray:
    """row_hash(r, salt) = mix32(uint32(r) * 0x9E3779B1 ^ mix32(salt + uint32(r >> 32)))"""
    r = np.asarray(rows, np.int64)
    lo = r.astype(np.uint64) & M32
    hi = (r >> 32).astype(np.uint64) & M32
    inner = _mix32((np.uint64(salt & 0xFFFFFFFF) + hi) & M32)
    return _mix32(((lo * np.uint64(0x9E3779B1)) & M32) ^ inner)


def quantise(g, s, sg: float, ss: float, rows, salt: int, dither: bool = True):
    """(G_q, S_q) int64 per row: floor(fmaf(g, sg, d1)), floor(fmaf(s, ss, d2))
    in fp32.  The scales are powers of two, so the fp32 product is exact and
    the sum rounds once, as the fused multiply-add does."""
    g = np.asarray(g, np.float32)
    s = np.asarray(s, np.float32)
    if dither:
        hsh = row_hash(rows, salt)
        d1 = (hsh & np.uint64(0xFFFF)).astype(np.float32) * np.float32(1.0 / 65536.0)
        d2 = (hsh >> np.uint64(16)).astype(np.float32) * np.float32(1.0 / 65536.0)
    else:
        d1 = d2 = np.zeros(g.shape, np.float32)
    gq = np.floor(g * np.float32(sg) + d1).astype(np.int64)
    sq = np.floor(s * np.float32(ss) + d2).astype(np.int64)
    return gq, sq


def packed_rows(gq, sq, pk32: bool) -> np.ndarray:
    """The level-0 packed rows as hist_build stores them: 64-bit (PKM 1)
    uint32(G_q) << 32 | S_q, or 32-bit (PKM 3) uint32(G_q) << 16 | (S_q & 0xFFFF)"""
    gu = np.asarray(gq, np.int64).astype(np.uint64) & M32
    su = np.asarray(sq, np.int64).astype(np.uint64) & M32
    if pk32:
        return (((gu << np.uint64(16)) & M32) | (su & np.uint64(0xFFFF))).astype(np.uint32)
    return (gu << np.uint64(32)) | su


def quantised_rows(g, h, w, mode: int, qs, row_base: int, salt: int, dither: bool = True):
    """(G_q, S_q) of rows 0 .. n - 1 of a rank whose first row has the global
    id ``row_base``; s is w (1 without weights) in mode 0 and h in mode 1"""
    g = np.asarray(g, np.float32)
    s = (np.ones(g.size, np.float32) if w is None else w) if mode == 0 else h
    rows = np.arange(g.size, dtype=np.int64) + int(row_base)
    return quantise(g, s, qs[0], qs[1], rows, salt, dither)


def leaf_ints(x, scale: float) -> np.ndarray:
    """rint(fp32(x) * fp32(scale)) as int64 (__float2int_rn)"""
    return np.rint(np.asarray(x, np.float32) * np.float32(scale)).astype(np.int64)


# ---------------------------------------------------------------------------
# level scan
# ---------------------------------------------------------------------------
def _l1(x, a):
    if a <= 0.0:
        return x
    return np.where(x > a, x - a, np.where(x < -a, x + a, 0.0))


def _gain(GL, SL, G, S, p):
    """split_gain_pt on float64 arrays (G, S broadcast); -inf where inadmissible"""
    GR, SR = G - GL, S - SL
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if p.mode == 0:
            bad = (SL < p.min_rows) | (SR < p.min_rows) | (SL <= 0.0) | (SR <= 0.0)
            pt = G * G / S
            gain = GL * GL / SL + GR * GR / SR - pt
        else:
            bad = (SL < p.min_child_weight) | (SR < p.min_child_weight) | (SL <= 0.0) | (SR <= 0.0)
            lam = p.reg_lambda
            tt = _l1(G, p.reg_alpha)
            pt = tt * tt / (S + lam)
            tl, tr = _l1(GL, p.reg_alpha), _l1(GR, p.reg_alpha)
            gain = 0.5 * (tl * tl / (SL + lam) + tr * tr / (SR + lam) - pt) - p.gamma
    return np.where(bad | ~(gain > -np.inf), -np.inf, gain)


def _bincount_i64(key, wts, size):
    """exact integer bincount (float64 accumulation of integers below 2^53)"""
    if np.abs(wts).sum() >= 2 ** 53:
        raise OverflowError("integer histogram outside the exact float64 range")
    return np.rint(np.bincount(key, wts.astype(np.float64), size)).astype(np.int64)


def level_hist(codes, nbt, node, gq, sq, n_nodes):
    """exact int64 histograms [n_nodes][F][nbt] of (G_q, S_q) over the rows with node >= 0"""
    F = codes.shape[0]
    act = np.nonzero(node >= 0)[0]
    nn = node[act] * nbt
    ga, sa = gq[act], sq[act]
    Gh = np.zeros((n_nodes, F, nbt), np.int64)
    Sh = np.zeros((n_nodes, F, nbt), np.int64)
    for f in range(F):
        key = nn + codes[f, act].astype(np.int64)
        Gh[:, f, :] = _bincount_i64(key, ga, n_nodes * nbt).reshape(n_nodes, nbt)
        Sh[:, f, :] = _bincount_i64(key, sa, n_nodes * nbt).reshape(n_nodes, nbt)
    return Gh, Sh


def allowed_features(p, F, n_nodes, tree_index, depth, fmask) -> np.ndarray:
    """bool [n_nodes][F]: the tree's column mask and the per-node mtries / column sample"""
    if p.mtries > 0 or p.col_sample_rate < 1.0:
        return np.stack([feature_allowed(p, F, tree_index, depth, i, fmask) for i in range(n_nodes)])
    return np.broadcast_to(np.ones(F, bool) if fmask is None else np.asarray(fmask, bool), (n_nodes, F))


def _lv(G, S, p):
    """leaf_value(G, S, S, p) on float64 arrays: the child value mono_ok and the
    interval cuts compare (S stands for both H and W)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if p.leaf_mode == 1:
            v = np.where(S > 0.0, -G / S, 0.0)
        else:
            den = S + p.reg_lambda
            v = np.where(den > 1e-12, -_l1(G, p.reg_alpha) / den, 0.0)
    v = v * p.learn_rate
    if p.max_abs_leaf > 0.0:
        v = np.minimum(np.maximum(v, -p.max_abs_leaf), p.max_abs_leaf)
    return v


def mono_signs(p, F):
    """int [F] of SplitParams::mono, or None when no feature is constrained (the
    engine then allocates no gbound and nothing is clamped)"""
    if p.monotone is None or not any(int(m) != 0 for m in p.monotone):
        return None
    if len(p.monotone) != F:
        raise ValueError("monotone needs one entry per feature")
    return np.sign(np.asarray(p.monotone, np.int64))


def bitset(mask) -> np.ndarray:
    """8 uint32 words of a bool vector over bins (bit b of word b >> 5)"""
    bits = np.zeros(256, np.uint8)
    bits[: len(mask)] = np.asarray(mask, bool)
    return np.packbits(bits, bitorder="little").view("<u4").copy()


class LevelScan:
    """Split candidates of one level from its histograms ``Gh`` / ``Sh``
    int64 [n_nodes][F][nbt] (feat_scan_wave, then node_best_wave).

    Per (node, feature) - ``f_gain`` (-inf: none), ``f_code``, ``f_GL`` /
    ``f_SL`` and the row's totals ``f_G`` / ``f_S`` (the FeatBest record): the
    best gain, then the smaller code, over the thresholds t < min(nvb[f],
    nbt - 1) with the NA bin nbt - 1 kept out of the prefix; code 2t sends NA
    right, 2t + 1 left (only with NA mass).  Per node - ``G_int`` / ``S_int``
    totals (feature 0's row) and the best candidate (``gain`` -inf / ``feat``
    -1: none): the best gain, then the smaller (feature, code), with its
    integer left totals, and ``ntie``: the number of distinct (GL_int, SL_int)
    among the candidates within relative TIE_REL of the best gain (see
    :meth:`near`).

    ``catf`` bool [F]: categorical rows (feat_best_cat_wave).  A bin t <
    min(nvb[f], nbt - 1) with S_int > 0 is a level; the levels are ordered by
    (float64(G_int) / float64(S_int), t) and every prefix of that order is a
    candidate, stored AT THE BIN ID t OF ITS LAST LEVEL (not its rank), so codes,
    ties and the FeatBest fields read as for thresholds.  Its integer left
    totals are the prefix's; :meth:`left_set` gives the members.  ``mono`` int
    [F]: a threshold candidate whose child values leaf_value(GL, SL, SL) /
    (G - GL, S - SL, S - SL) break the feature's sign is -inf (mono_ok); the
    categorical scan applies no such test, whatever mono[f] says."""

    def __init__(self, Gh, Sh, nvb, p, ig, is_, allowed, catf=None, mono=None):
        n_nodes, F, nbt = Gh.shape
        self.F, self.nbt, self.n_nodes, self.p, self.ig, self.is_ = F, nbt, n_nodes, p, ig, is_
        self.Gh, self.Sh, self.allowed = Gh, Sh, allowed
        T = nbt - 1
        # the NA bin (nbt - 1) stays out of the prefix
        pg, ps = np.cumsum(Gh[:, :, :T], axis=2), np.cumsum(Sh[:, :, :T], axis=2)
        nag, nas = Gh[:, :, T], Sh[:, :, T]
        tg, ts = pg[:, :, -1] + nag, ps[:, :, -1] + nas                 # [nodes][F] totals of each row
        self.G_int, self.S_int = tg[:, 0], ts[:, 0]
        m = np.minimum(np.asarray(nvb, np.int64), T)
        inrange = np.arange(T)[None, :] < m[:, None]                                       # [F][T]
        cand = np.repeat(inrange[None, :, :], n_nodes, 0) & allowed[:, :, None]            # [nodes][F][T]
        self.catf = np.zeros(F, bool) if catf is None else np.asarray(catf, bool)
        self.cat_key = {}
        for f in np.nonzero(self.catf)[0]:
            # levels in (key, bin) order; the prefix ending at level t lands at index t
            gl, sl = Gh[:, f, :T], Sh[:, f, :T]
            ne = inrange[f][None, :] & (sl > 0)
            key = np.where(ne, gl.astype(np.float64) / np.where(ne, sl, 1).astype(np.float64), np.inf)
            order = np.argsort(key, axis=1, kind="stable")
            cg = np.cumsum(np.take_along_axis(np.where(ne, gl, 0), order, 1), axis=1)
            cs = np.cumsum(np.take_along_axis(np.where(ne, sl, 0), order, 1), axis=1)
            np.put_along_axis(pg[:, f, :], order, cg, 1)
            np.put_along_axis(ps[:, f, :], order, cs, 1)
            cand[:, f, :] = ne & allowed[:, f, None]
            self.cat_key[int(f)] = key
        # integer left totals of code 2t (NA right) and 2t + 1 (NA left)
        GLi = np.stack([pg, pg + nag[:, :, None]], axis=3)                # [nodes][F][T][2]
        SLi = np.stack([ps, ps + nas[:, :, None]], axis=3)
        self.f_G, self.f_S = tg.astype(np.float64) * ig, ts.astype(np.float64) * is_
        ng, ns = nag.astype(np.float64) * ig, nas.astype(np.float64) * is_
        # decoded as the kernel does: the prefix and the NA sums separately, then added
        GLd = np.stack([pg.astype(np.float64) * ig, pg.astype(np.float64) * ig + ng[:, :, None]], axis=3)
        SLd = np.stack([ps.astype(np.float64) * is_, ps.astype(np.float64) * is_ + ns[:, :, None]], axis=3)
        gain = _gain(GLd, SLd, self.f_G[:, :, None, None], self.f_S[:, :, None, None], p)
        ok = np.stack([cand, cand & (ns > 0.0)[:, :, None]], axis=3)
        gain = np.where(ok, gain, -np.inf)
        if mono is not None:
            Gt, St = self.f_G[:, :, None, None], self.f_S[:, :, None, None]
            for f in np.nonzero((np.asarray(mono) != 0) & ~self.catf)[0]:
                wl, wr = _lv(GLd[:, f], SLd[:, f], p), _lv(Gt[:, f] - GLd[:, f], St[:, f] - SLd[:, f], p)
                gain[:, f] = np.where((wl <= wr) if mono[f] > 0 else (wl >= wr), gain[:, f], -np.inf)
        self.gains, self.GLi, self.SLi, self.GLd, self.SLd = gain, GLi, SLi, GLd, SLd
        # per feature: first maximum = smallest code
        pf = gain.reshape(n_nodes, F, 2 * T)
        fa = pf.argmax(axis=2)
        take = lambda a: np.take_along_axis(a.reshape(n_nodes, F, 2 * T), fa[:, :, None], axis=2)[:, :, 0]
        self.f_gain = take(gain)
        fhas = self.f_gain > -np.inf
        self.f_code = np.where(fhas, fa, 0x7FFFFFFF)
        self.f_GL, self.f_SL = np.where(fhas, take(GLd), 0.0), np.where(fhas, take(SLd), 0.0)
        # per node: first maximum = smallest (feature, code)
        flat = gain.reshape(n_nodes, -1)
        arg = flat.argmax(axis=1)
        best = flat[np.arange(n_nodes), arg]
        has = best > -np.inf
        f, rem = np.divmod(arg, 2 * T)
        pick = lambda a: a.reshape(n_nodes, -1)[np.arange(n_nodes), arg]
        self.gain = np.where(has, best, -np.inf)
        self.feat = np.where(has, f, -1)
        self.code = np.where(has, rem, 0)
        self.GL_int, self.SL_int = np.where(has, pick(GLi), 0), np.where(has, pick(SLi), 0)
        self.GL, self.SL = np.where(has, pick(GLd), 0.0), np.where(has, pick(SLd), 0.0)
        self.G = self.G_int.astype(np.float64) * ig
        self.S = self.S_int.astype(np.float64) * is_
        self.ntie = np.zeros(n_nodes, np.int64)
        for i in np.nonzero(has)[0]:
            self.ntie[i] = len(self.near(i))

    def near(self, i: int) -> set:
        """distinct (GL_int, SL_int) of node i's candidates within TIE_REL of its best gain.
        A candidate and its mirror image (G - GL, S - SL) - the same two row sets
        with left and right exchanged, e.g. "NA right" of one threshold and "NA
        left" of another - count once: the gain adds the two children's terms, so
        it is the same to the bit, an exact tie that the (feature, code) order
        resolves, not a near-tie."""
        b = self.gain[i]
        sel = self.gains[i] >= b - TIE_REL * abs(b)
        G, S = int(self.G_int[i]), int(self.S_int[i])
        return {min((gl, sl), (G - gl, S - sl)) for gl, sl in zip(self.GLi[i][sel].tolist(), self.SLi[i][sel].tolist())}

    def left_set(self, i: int, f: int, t: int) -> np.ndarray:
        """bool [nbt - 1]: the levels of node i's categorical feature f at or before
        level t in (key, bin) order - the NA bin is never a member"""
        key = self.cat_key[f][i]
        return (key < np.inf) & ((key < key[t]) | ((key == key[t]) & (np.arange(key.size) <= t)))

    def candidate(self, i: int, f: int, t: int, na_left: int):
        """(gain, GL_int, SL_int, GL, SL) of one candidate of node i"""
        return (float(self.gains[i, f, t, na_left]), int(self.GLi[i, f, t, na_left]), int(self.SLi[i, f, t, na_left]),
                float(self.GLd[i, f, t, na_left]), float(self.SLd[i, f, t, na_left]))

    def top(self, i: int, k: int = 3) -> list:
        """the k best candidates of node i: (gain, feat, bin, na_left, GL_int, SL_int)"""
        flat = self.gains[i].reshape(-1)
        order = np.lexsort((np.arange(flat.size), -flat))[:k]
        T = self.nbt - 1
        out = []
        for a in order:
            if not flat[a] > -np.inf:
                break
            f, rem = divmod(int(a), 2 * T)
            out.append((float(flat[a]), f, rem >> 1, rem & 1, int(self.GLi[i].reshape(-1)[a]),
                        int(self.SLi[i].reshape(-1)[a])))
        return out


def decide(gain, feat, G, W, p) -> bool:
    """lf_decide: gain > 0 and H2O's relative min_split_improvement (mode 0)"""
    do = feat >= 0 and np.isfinite(gain) and gain > 0.0
    if do and p.mode == 0 and p.min_split_improvement > 0.0:
        base_term = G * G / W if W > 0.0 else 0.0
        do = gain > p.min_split_improvement * max(base_term, 1e-12)
    return bool(do)


def f32(x) -> np.float32:
    with np.errstate(over="ignore"):
        return np.float32(x)


def ulps(a, b) -> int:
    """distance of two fp32 values in representable steps (0 = same bits or both zero)"""
    def key(v):
        i = int(np.float32(v).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return 0 if (np.isnan(a) and np.isnan(b)) else 1 << 31
    return abs(key(a) - key(b))


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------
# the walk: grow (follow = None) and verify (follow = the GPU tree)
# ---------------------------------------------------------------------------
def _fclamp(v, lo, hi):
    """fmin(fmax(v, lo), hi)"""
    return min(max(v, lo), hi)


def _cut(mf, wl, wr, lo, hi):
    """the children's intervals (llo, lhi, rlo, rhi) of a split on a feature of
    sign mf inside [lo, hi]: cut at the midpoint of the clipped child values"""
    llo, lhi, rlo, rhi = lo, hi, lo, hi
    if mf != 0:
        mid = 0.5 * (_fclamp(wl, lo, hi) + _fclamp(wr, lo, hi))
        if mf > 0:
            lhi = rlo = mid
        else:
            llo = rhi = mid
    return llo, lhi, rlo, rhi


def _mono_newton(tree, total, mono, p, SG, SH, SW):
    """mono_newton_kernel on the oracle's tree: depths top-down, subtree (G, H)
    bottom-up from the exact leaf sums (each parent SG[left] + SG[left + 1] in
    float64), the intervals cut again on the Newton scale, every leaf clamped.
    Returns (LO, HI) by node id."""
    dep = np.full(total, -1, np.int64)
    dep[0] = 0
    levels = [[0]]
    while True:
        nxt = []
        for i in levels[-1]:
            l = int(tree[i]["left"])
            if tree[i]["feat"] >= 0 and l > 0 and l + 1 < total:
                dep[l] = dep[l + 1] = len(levels)
                nxt += [l, l + 1]
        if not nxt:
            break
        levels.append(nxt)
    SG, SH = SG.astype(np.float64).copy(), SH.astype(np.float64).copy()
    for lev in reversed(levels[:-1]):
        for i in lev:
            if tree[i]["feat"] >= 0:
                l = int(tree[i]["left"])
                SG[i], SH[i] = SG[l] + SG[l + 1], SH[l] + SH[l + 1]
    LO, HI = np.full(total, -np.inf), np.full(total, np.inf)
    for lev in levels:
        for i in lev:
            lo, hi = float(LO[i]), float(HI[i])
            if tree[i]["feat"] < 0:
                tree[i]["value"] = f32(_fclamp(leaf_value(float(SG[i]), float(SH[i]), float(SW[i]), p), lo, hi))
                continue
            l = int(tree[i]["left"])
            mf = int(mono[int(tree[i]["feat"])])
            wl = leaf_value(float(SG[l]), float(SH[l]), float(SH[l]), p) if mf else 0.0
            wr = leaf_value(float(SG[l + 1]), float(SH[l + 1]), float(SH[l + 1]), p) if mf else 0.0
            LO[l], HI[l], LO[l + 1], HI[l + 1] = _cut(mf, wl, wr, lo, hi)
    return LO, HI


def _walk(codes, nvb, edges, g, h, w, p, qs, row_base, salt, fmask, tree_index, dither, follow, catf=None,
          follow_cat=None, info=None):
    codes = np.asarray(codes)
    F, n = codes.shape
    catf = None if catf is None or not np.any(catf) else np.asarray(catf, bool)
    mono = mono_signs(p, F)
    ifsets = None
    if p.interactions:
        ifsets = [int(v) for v in interaction_masks(p.interactions, F)]
    edges = np.asarray(edges, np.float32)
    nbt = edges.shape[1]
    nvb = np.asarray(nvb, np.int64)
    g = np.asarray(g, np.float32)[:n]
    h = None if h is None else np.asarray(h, np.float32)[:n]
    w = None if w is None else np.asarray(w, np.float32)[:n]
    ones = np.ones(n, np.float32)
    gq, sq = quantised_rows(g, h, w, p.mode, qs, row_base, salt, dither)
    ig, is_ = float(qs[2]), float(qs[3])
    cap = (1 << (p.max_depth + 1)) - 1
    tree = np.zeros(cap, TREE_NODE_DTYPE)
    node = np.zeros(n, np.int64)
    leaf = np.full(n, -1, np.int64)
    records, ties = [], 0
    base, n_nodes = 0, 1
    # gbound: [lo, hi] of every node's value, written by its parent's split (the root has none)
    LO, HI = np.full(cap, -np.inf), np.full(cap, np.inf)
    # istate: (compatible-set mask, solo feature) of every node; root: every set, empty path
    imask, isolo = [0] * cap, [-1] * cap
    imask[0], isolo[0] = (1 << 64) - 1, -2
    bitsets = np.zeros((cap, 8), np.uint32)

    def clamp(v, gid):
        """clamp_bound"""
        return v if mono is None or gid <= 0 or gid >= cap else _fclamp(v, float(LO[gid]), float(HI[gid]))

    def inter_ok(gid, f):
        if isolo[gid] == -2:
            return True
        if isolo[gid] >= 0:
            return f == isolo[gid]
        return (ifsets[f] & imask[gid]) != 0

    def fail(d, i, field, sc, msg):
        gid = base + i
        lines = [f"level {d} node {i} (gid {gid}) field {field}: {msg}",
                 f"  totals G_int {int(sc.G_int[i])} S_int {int(sc.S_int[i])} near-tie candidates {int(sc.ntie[i])}",
                 "  oracle top candidates (gain, feat, bin, na_left, GL_int, SL_int):"]
        lines += [f"    {c}" for c in sc.top(i)]
        lines.append(f"  GPU record: {follow[gid] if follow is not None and gid < len(follow) else None}")
        text = "\n".join(lines)
        print(text)
        raise Mismatch(text)

    for d in range(p.max_depth):
        last = d == p.max_depth - 1
        Gh, Sh = level_hist(codes, nbt, node, gq, sq, n_nodes)
        listed = allowed = allowed_features(p, F, n_nodes, tree_index, d, fmask)
        if ifsets is not None:
            allowed = allowed & np.array([[inter_ok(base + i, f) for f in range(F)] for i in range(n_nodes)], bool)
        sc = LevelScan(Gh, Sh, nvb, p, ig, is_, allowed, catf, mono)
        # for the tests' witnesses only (``info``): the level with neither constraint applied
        free = None
        if info is not None and (mono is not None or ifsets is not None):
            free = LevelScan(Gh, Sh, nvb, p, ig, is_, listed, catf)
        next_base = base + n_nodes
        k = 0
        child = np.full(n_nodes, -1, np.int64)
        sfeat = np.zeros(n_nodes, np.int64)
        sbin = np.zeros(n_nodes, np.int64)
        snal = np.zeros(n_nodes, np.int64)
        sleft = np.zeros((n_nodes, nbt), bool)      # left sets of the level's categorical splits
        scat = np.zeros(n_nodes, bool)
        for i in range(n_nodes):
            gid = base + i
            G, S = float(sc.G[i]), float(sc.S[i])
            o_gain, o_feat, o_code = float(sc.gain[i]), int(sc.feat[i]), int(sc.code[i])
            do = decide(o_gain, o_feat, G, S, p)
            f_, t_, nal = o_feat, o_code >> 1, o_code & 1
            gain, GLi, SLi, GL, SL = o_gain, int(sc.GL_int[i]), int(sc.SL_int[i]), float(sc.GL[i]), float(sc.SL[i])
            tie = bool(do and sc.ntie[i] > 1)
            if follow is not None:
                gt = follow[gid]
                if int(gt["feat"]) < 0:
                    if do:
                        fail(d, i, "feat", sc, "GPU made a leaf, the oracle's best candidate passes lf_decide")
                    if int(gt["left"]) != -1:
                        fail(d, i, "left", sc, "leaf record with a child link")
                else:
                    gf, gb, gn = int(gt["feat"]), int(gt["bin"]), int(gt["na_left"])
                    if not do:
                        fail(d, i, "feat", sc, "GPU split, the oracle has no admissible candidate passing lf_decide")
                    if not (0 <= gf < F and 0 <= gb < min(int(nvb[gf]), nbt - 1) and 0 <= gn <= 3):
                        fail(d, i, "bin", sc, "GPU split outside the candidate range")
                    # bit 1 of na_left: a categorical split, of a categorical feature only
                    if (gn >> 1) != int(catf is not None and catf[gf]):
                        fail(d, i, "na_left", sc, f"categorical bit {gn >> 1} on feature {gf}")
                    gn &= 1
                    if (gf, gb, gn) != (f_, t_, nal):
                        cg = sc.candidate(i, gf, gb, gn)
                        excused = (tie and sc.allowed[i, gf] and cg[0] >= o_gain - TIE_REL * abs(o_gain)
                                   and decide(cg[0], gf, G, S, p))
                        if not excused:
                            fail(d, i, "feat/bin/na_left", sc,
                                 f"GPU picked {(gf, gb, gn)} (gain {cg[0]!r}, GL_int {cg[1]}, SL_int {cg[2]}), "
                                 f"oracle {(f_, t_, nal)} (gain {o_gain!r})")
                        f_, t_, nal = gf, gb, gn
                        gain, GLi, SLi, GL, SL = cg
                    if int(gt["left"]) != next_base + 2 * k:
                        fail(d, i, "left", sc, f"child numbering: GPU {int(gt['left'])}, oracle {next_base + 2 * k}")
                    if catf is not None and catf[f_]:
                        if not np.isnan(gt["thr"]):
                            fail(d, i, "thr", sc, f"GPU {gt['thr']!r}, a categorical split carries NaN")
                        want_bits = bitset(sc.left_set(i, f_, t_))
                        got_bits = np.asarray(follow_cat[gid], np.uint32)
                        if not np.array_equal(got_bits, want_bits):
                            fail(d, i, "bitset", sc, "left set words GPU " + " ".join(f"{int(v):08x}" for v in got_bits)
                                 + ", oracle " + " ".join(f"{int(v):08x}" for v in want_bits))
                    else:
                        thr = edges[f_, t_] if t_ < int(nvb[f_]) - 1 else np.float32(np.inf)
                        if np.float32(gt["thr"]).tobytes() != np.float32(thr).tobytes():
                            fail(d, i, "thr", sc, f"GPU {gt['thr']!r}, oracle {thr!r}")
                    if ulps(gt["gain"], f32(gain)) > 1:
                        fail(d, i, "gain", sc, f"GPU {gt['gain']!r}, oracle {f32(gain)!r} ({gain!r})")
                    if ulps(gt["weight"], f32(S)) > 1:
                        fail(d, i, "weight", sc, f"GPU {gt['weight']!r}, oracle {f32(S)!r}")
            ties += tie
            rec = tree[gid]
            rec["weight"] = f32(S)
            rec["value"] = f32(clamp(leaf_value(G, S, S, p), gid))
            if follow is not None and do and ulps(follow[gid]["value"], rec["value"]) > 1:
                fail(d, i, "value", sc, f"GPU {follow[gid]['value']!r}, oracle {rec['value']!r} "
                     f"(interval [{LO[gid]!r}, {HI[gid]!r}])")
            r = dict(level=d, node=i, gid=gid, gain=o_gain, ntie=int(sc.ntie[i]), split=do,
                     G_int=int(sc.G_int[i]), S_int=int(sc.S_int[i]), GL_int=GLi, SL_int=SLi,
                     feat=f_ if do else -1, bin=t_, na_left=nal)
            if free is not None:
                # the best candidate with neither mono_ok nor inter_ok applied
                r.update(free_feat=int(free.feat[i]), free_code=int(free.code[i]),
                         free_barred=bool(free.feat[i] >= 0 and not allowed[i, free.feat[i]]))
            if ifsets is not None:
                r.update(imask=imask[gid], isolo=isolo[gid])
            records.append(r)
            if do:
                cg = next_base + 2 * k
                is_cat = bool(catf is not None and catf[f_])
                rec["feat"], rec["bin"], rec["na_left"], rec["left"] = f_, t_, nal | (2 if is_cat else 0), cg
                rec["gain"] = f32(gain)
                rec["thr"] = np.nan if is_cat else (edges[f_, t_] if t_ < int(nvb[f_]) - 1 else np.inf)
                child[i], sfeat[i], sbin[i], snal[i] = 2 * k, f_, t_, nal
                r.update(left=cg, cat=False)
                if is_cat:
                    scat[i] = True
                    sleft[i, : nbt - 1] = sc.left_set(i, f_, t_)
                    bitsets[gid] = bitset(sleft[i])
                    in_f = Sh[i, f_, : min(int(nvb[f_]), nbt - 1)]
                    r.update(cat=True, left_levels=np.nonzero(sleft[i])[0].tolist(), empty_levels=int((in_f == 0).sum()))
                if mono is not None:
                    # the intervals follow mono[feat], whatever the kind of the split
                    mf = int(mono[f_])
                    lo, hi = (float(LO[gid]), float(HI[gid])) if gid > 0 else (-np.inf, np.inf)
                    cut = _cut(mf, leaf_value(GL, SL, SL, p), leaf_value(G - GL, S - SL, S - SL, p), lo, hi)
                    LO[cg], HI[cg], LO[cg + 1], HI[cg + 1] = cut
                    r.update(cut=mf != 0, interval=(lo, hi), child_intervals=cut)
                if ifsets is not None:
                    # inter_children: both children get the same state
                    fs = ifsets[f_]
                    if fs != 0:
                        comp = (1 << 64) - 1 if isolo[gid] == -2 else imask[gid]
                        st = (comp & fs, -1)
                    else:
                        st = (0, f_)
                    for c in (cg, cg + 1):
                        imask[c], isolo[c] = st
                if last:
                    # children are final: totals from the split's left / right sums
                    # (leaf_finalize then overwrites value and weight from the leaf sums)
                    for c, (Gc, Sc) in enumerate(((GL, SL), (G - GL, S - SL))):
                        cr = tree[cg + c]
                        cr["feat"], cr["left"] = -1, -1
                        cr["value"], cr["weight"] = f32(clamp(leaf_value(Gc, Sc, Sc, p), cg + c)), f32(Sc)
                k += 1
            else:
                rec["feat"], rec["left"] = -1, -1
        # part_right: NA follows na_left, other bins go right when above the split bin
        act = np.nonzero(node >= 0)[0]
        nn = node[act]
        ch = child[nn]
        ret = ch < 0
        leaf[act[ret]] = base + nn[ret]
        node[act[ret]] = -1
        a_sp, n_sp = act[~ret], nn[~ret]
        b = codes[sfeat[n_sp], a_sp].astype(np.int64)
        above = np.where(scat[n_sp], ~sleft[n_sp, b], b > sbin[n_sp])     # a categorical split tests its set
        right = np.where(b == nbt - 1, 1 - snal[n_sp], above.astype(np.int64))
        nxt = ch[~ret] + right
        if last:
            leaf[a_sp] = next_base + nxt
            node[a_sp] = -1
        else:
            node[a_sp] = nxt
        base, n_nodes = next_base, 2 * k
        if n_nodes == 0:
            break
    total = base + n_nodes
    # exact leaf sums: rint(fp32(x) * fp32(scale)) per row of nonzero weight
    live = np.ones(n, bool) if w is None else (w != 0)
    lg, lh, lw = float(qs[4]), float(qs[5]), float(qs[6])
    lf = leaf[live]
    Gs = _bincount_i64(lf, leaf_ints(g[live], lg), cap)
    Hs = _bincount_i64(lf, leaf_ints(h[live], lh), cap) if h is not None else np.zeros(cap, np.int64)
    Ws = _bincount_i64(lf, leaf_ints((ones if w is None else w)[live], lw), cap)
    clamps = []
    for gid in range(min(total, cap)):
        if tree[gid]["feat"] < 0:
            Gv, Hv, Wv = Gs[gid] / lg, Hs[gid] / lh, Ws[gid] / lw
            raw = leaf_value(Gv, Hv, Wv, p)
            tree[gid]["value"] = f32(clamp(raw, gid))
            tree[gid]["weight"] = f32(Wv)
            clamps.append([gid, raw, clamp(raw, gid), None])
    newton = mono is not None and p.mode == 0 and p.leaf_mode == 0
    if newton:
        # squared-error splits with Newton leaves: the level's intervals are on the
        # -G/W scale, mono_newton_kernel re-derives them from the leaf sums
        NLO, NHI = _mono_newton(tree, min(total, cap), mono, p, Gs / lg, Hs / lh, Ws / lw)
        for c in clamps:
            c[3] = _fclamp(c[1], float(NLO[c[0]]), float(NHI[c[0]]))
    if info is not None:
        info.update(records=records, cap=cap, total=total, catbits=bitsets[:max(total, 1)], lo=LO, hi=HI, newton=newton,
                    leaf_clamps=clamps,
                    istate=list(zip(imask, isolo)))
    return tree[:max(total, 1)], leaf, records, ties, (gq, sq)


def grow(codes, nvb, edges, g, h, w, params, scales, row_base, salt, fmask=None, *, tree_index=None, dither=True,
         catf=None, info=None):
    """Grow one tree.  ``codes`` uint8 [F][n], ``edges`` float32 [F][nbt],
    ``scales`` = qscale[0..6]; ``salt``: the tree's dither salt (its index,
    which also keys the per-node column sample unless ``tree_index`` differs).
    Returns (tree, per-row leaf id, per-node records); a record holds the
    best gain, ``ntie`` (distinct (GL_int, SL_int) within TIE_REL of it) and
    the integer totals.  ``catf`` bool [F] flags the categorical features;
    ``params.monotone`` / ``params.interactions`` switch the constraints on.  A
    dict passed as ``info`` receives ``catbits`` uint32 [nodes][8] (the left
    sets by node id), the level intervals ``lo`` / ``hi``, ``istate``,
    ``newton`` (the leaves went through the mono_newton re-derivation) and
    ``leaf_clamps``: [gid, raw value, clamped by the level's interval, clamped
    by the re-derived one or None] of every leaf."""
    ti = salt if tree_index is None else tree_index
    tree, leaf, records, _, _ = _walk(codes, nvb, edges, g, h, w, params, scales, row_base, salt, fmask, ti,
                                      dither, None, catf, None, info)
    return tree, leaf, records


def near_tie_nodes(records) -> int:
    """splitting nodes with more than one distinct candidate within TIE_REL of the best"""
    return sum(1 for r in records if r["split"] and r["ntie"] > 1)


def verify(codes, nvb, edges, g, h, w, params, scales, row_base, salt, fmask, gpu_tree, gpu_nid, gpu_qscale, *,
           tree_index=None, catf=None, gpu_cat=None, info=None) -> int:
    """Check one GPU-built tree against the oracle, level by level: at each
    node the oracle recomputes the node from the rows the GPU tree routes
    there.  Raises Mismatch (after printing the level, node, field, the
    oracle's top three candidates with integer totals and the GPU record) at
    the first difference; only a near-tie node - more than one distinct
    candidate within TIE_REL of the best - may hold another of those
    candidates, and the walk then follows the GPU's pick.  With categorical
    features (``catf``) ``gpu_cat`` uint32 [nodes][8] holds the GPU tree's
    bitsets, which must equal the oracle's word for word at every categorical
    split.  Returns the number of near-tie nodes."""
    ti = salt if tree_index is None else tree_index
    qs = np.asarray(gpu_qscale, np.float64)
    want = np.asarray(scales, np.float64)
    names = ("sg", "ss", "1/sg", "1/ss", "leaf g", "leaf h", "leaf w")
    for j in range(7):
        if qs[j].tobytes() != want[j].tobytes():
            raise Mismatch(f"qscale[{j}] ({names[j]}): GPU {qs[j]!r}, formula {want[j]!r}")
    if qs[7] != float(row_base):
        raise Mismatch(f"qscale[7] (row_base): GPU {qs[7]!r}, expected {row_base}")
    if qs[9] != float(salt & 0x7FFFFFFF):
        raise Mismatch(f"qscale[9] (tree index): GPU {qs[9]!r}, expected {salt & 0x7FFFFFFF}")
    gpu_tree = np.asarray(gpu_tree)
    if catf is not None and np.any(catf):
        gpu_cat = np.asarray(gpu_cat, np.uint32).reshape(-1, 8)
    tree, leaf, records, ties, _ = _walk(codes, nvb, edges, g, h, w, params, want, row_base, salt, fmask, ti, True,
                                         gpu_tree, catf, gpu_cat, info)
    # leaves: value and weight from the fixed-point leaf sums
    for gid in range(len(tree)):
        if tree[gid]["feat"] < 0:
            gt = gpu_tree[gid]
            for fld in ("value", "weight"):
                if int(gt["feat"]) >= 0 or ulps(gt[fld], tree[gid][fld]) > 1:
                    text = (f"leaf gid {gid} field {fld}: GPU {gt[fld]!r}, oracle {tree[gid][fld]!r}\n"
                            f"  GPU record: {gt}\n  oracle record: {tree[gid]}")
                    print(text)
                    raise Mismatch(text)
    # routing: every row, zero-weight rows included, carries ~leaf
    nid = np.asarray(gpu_nid, np.int64)[: leaf.size]
    bad = np.nonzero(nid != ~leaf)[0]
    if bad.size:
        r = int(bad[0])
        text = (f"row routing: {bad.size} rows differ, first row {r}: GPU nid {int(nid[r])} (leaf {~int(nid[r])}), "
                f"oracle leaf {int(leaf[r])}")
        print(text)
        raise Mismatch(text)
    return ties
