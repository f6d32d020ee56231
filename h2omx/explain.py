"""Model explanations: SHAP contributions and partial dependence.

``predict_contributions(model, frame)`` (H2O ``predict_contributions``):
path-dependent TreeSHAP for GBM / DRF / XGBoost / Isolation-Forest-free
tree ensembles with one tree per iteration (regression and binomial, like
H2O).  Output columns are the predictors plus ``BiasTerm``; each row sums
to the model's raw margin (link space).  On the GPU the contributions come
from csrc/explain_kernels.hip (one thread per row over a flattened path
table); on CPU frames the same path formula runs vectorised in NumPy.
With ``background_frame=`` the same path table gives interventional
(baseline) SHAP against every background row, averaged over the background
or, with ``output_per_reference=True``, one row per (row, background row).
``top_n=`` / ``bottom_n=`` / ``compare_abs=`` return, for any of these forms,
each row's strongest features by name and value instead of every column; on
the device contrib_rank_kernel ranks the contribution planes where the SHAP
kernels left them.  For a Deep Learning model ``background_frame=`` gives
DeepSHAP (DeepLIFT's rescale rule per pair) in the same forms: on the device
deepshap_rescale_kernel and deepshap_fold_kernel around the project's GEMM,
on CPU frames the same closed forms in float64.

``friedman_h(model, frame, variables)`` (H2O ``model.h``): Friedman and
Popescu's H statistic of 2 or more numerical variables, from the partial
dependence of every subset of them by the weighted tree traversal, summed
over the same path table in float64 (friedman_h_pd_kernel on the GPU).

``partial_dependence(model, frame, col, nbins)`` (H2O PartialDependence):
mean / sd / standard error of the model response with ``col`` forced to
each grid value (``nbins`` equally spaced values between the column's min
and max, every level for categorical columns), scored on the device; with
``col2`` the 2-D table of a pair, with ``weight_column`` / ``include_na`` /
``row_index`` H2O's options of the same names.  Tree models on a device frame
get every cell's margins from one pass of pd_sweep_kernel
(csrc/explain_kernels.hip), bit-identical to scoring the frame with the
columns overwritten; every other model and frame takes that loop.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .frame.frame import ENUM, INT, Frame, Vec
from .models.base import ModelCategory


# ---------------------------------------------------------------------------
# TreeSHAP
# ---------------------------------------------------------------------------
def tree_paths(trees: np.ndarray, scale: float = 1.0, catbits: np.ndarray | None = None):
    """Flatten every root-to-leaf path: returns (leaves [L][4] int32 =
    {first element, m, value bits, tree}, elems [E][4] float32 = {feature |
    na_ok << 30 | categorical << 29, z, lo, hi}, expected value, max unique
    features, sets [S][8] uint32).  A categorical feature's element keeps the
    set of levels the path allows (intersection of its group splits' sides)
    in ``sets[lo]``."""
    leaves, elems, sets = [], [], []
    expected = 0.0
    maxm = 1
    full = np.full(8, 0xFFFFFFFF, np.uint32)
    for t in range(trees.shape[0]):
        tr = trees[t]
        cb = None if catbits is None else catbits[t]
        # stack entries: (node, {feature: [z, lo, hi, na_ok, level set or None]})
        stack = [(0, {})]
        while stack:
            i, path = stack.pop()
            nd = tr[i]
            if nd["feat"] < 0:
                v = float(nd["value"]) * scale
                m = len(path)
                zprod = 1.0
                start = len(elems)
                for f, (z, lo, hi, na, st) in path.items():
                    if st is not None:
                        elems.append((np.int32(f | (int(na) << 30) | (1 << 29)).view(np.float32), z,
                                      float(len(sets)), 0.0))
                        sets.append(st)
                    else:
                        elems.append((np.int32(f | (int(na) << 30)).view(np.float32), z, lo, hi))
                    zprod *= z
                leaves.append((start, m, np.float32(v).view(np.int32), t))
                expected += v * zprod
                maxm = max(maxm, m)
                continue
            f, thr, left = int(nd["feat"]), float(nd["thr"]), int(nd["left"])
            is_cat = cb is not None and (int(nd["na_left"]) & 2) != 0
            w = float(nd["weight"])
            for child, go_left in ((left, True), (left + 1, False)):
                cw = float(tr[child]["weight"])
                r = cw / w if w > 0 else 0.0
                z, lo, hi, na, st = path.get(f, (1.0, -np.inf, np.inf, True, None))
                if is_cat:
                    side = cb[i] if go_left else ~cb[i]
                    st = (full if st is None else st) & side
                elif go_left:
                    hi = min(hi, thr)
                else:
                    lo = max(lo, thr)
                na = na and (bool(int(nd["na_left"]) & 1) == go_left)
                p2 = dict(path)
                p2[f] = (z * r, lo, hi, na, st)
                stack.append((child, p2))
    lv = np.asarray(leaves, np.int32).reshape(-1, 4)
    el = np.asarray([(e[0], e[1], e[2], e[3]) for e in elems], np.float32).reshape(-1, 4) if elems else \
        np.zeros((0, 4), np.float32)
    if elems:
        el[:, 0] = np.asarray([e[0] for e in elems], np.float32)
    st = np.asarray(sets, np.uint32).reshape(-1, 8) if sets else np.zeros((1, 8), np.uint32)
    return lv, el, expected, maxm, st


def shapley_weights(M: int) -> np.ndarray:
    """w[m][k] = k! (m-1-k)! / m! for 1 <= m <= M, 0 <= k < m (row/col M+1)."""
    w = np.zeros((M + 1, M + 1), np.float64)
    for m in range(1, M + 1):
        for k in range(m):
            w[m, k] = math.exp(math.lgamma(k + 1) + math.lgamma(m - k) - math.lgamma(m + 1))
    return w


def _bucket(maxm: int) -> int:
    return 8 if maxm <= 8 else (16 if maxm <= 16 else 32)


def _follows(X: np.ndarray, E: np.ndarray, sets=None):
    """The follow rule of one leaf's elements E [m][4] on rows X [F][n]:
    (features [m], o [m][n] float64 with o = 1 where the row satisfies the
    element: lo < x <= hi, NA by na_ok, categorical levels by the path's level
    set, out-of-range levels in the NA direction)."""
    feats = E[:, 0].view(np.int32)
    f = feats & 0x1FFFFFFF
    na_ok = (feats >> 30) & 1
    iscat = (feats >> 29) & 1
    x = X[f]                                       # [m][n]
    with np.errstate(invalid="ignore"):
        o = np.where(np.isnan(x), na_ok[:, None].astype(np.float64),
                     ((x > E[:, 2:3]) & (x <= E[:, 3:4])).astype(np.float64))
    if sets is not None and iscat.any():
        from .models.tree.structs import bitset_has

        for j in np.nonzero(iscat)[0]:
            c = np.where(np.isnan(x[j]), -1, x[j]).astype(np.int64)
            oor = (c < 0) | (c > 255)
            inside = bitset_has(sets[int(E[j, 2])], c).astype(np.float64)
            o[j] = np.where(np.isnan(x[j]) | oor, float(na_ok[j]), inside)
    return f, o


def _shap_numpy(X: np.ndarray, lv, el, maxm, sets=None) -> np.ndarray:
    F, n = X.shape
    out = np.zeros((F, n), np.float64)
    W = shapley_weights(maxm)
    for start, m, vbits, _ in lv:
        v = float(np.int32(vbits).view(np.float32))
        if m == 0:
            continue
        E = el[start: start + m]
        z = E[:, 1].astype(np.float64)
        f, o = _follows(X, E, sets)
        P = np.zeros((m + 1, n))
        P[0] = 1.0
        for j in range(m):
            P[1:] = z[j] * P[1:] + o[j] * P[:-1]
            P[0] *= z[j]
        for i in range(m):
            s = np.zeros(n)
            carry = np.zeros(n)
            s1 = np.zeros(n)
            for k in range(m, 0, -1):
                q = P[k] - z[i] * carry
                s1 += q * W[m, k - 1]
                carry = q
            if z[i] > 0:
                s0 = (P[:m] * W[m, :m, None]).sum(0) / z[i]
            else:
                s0 = np.zeros(n)
            s = np.where(o[i] != 0, s1, s0)
            out[f[i]] += v * (o[i] - z[i]) * s
    return out


def _shap_device(X: torch.Tensor, lv, el, maxm, sets) -> torch.Tensor:
    """The HIP path (csrc/explain_kernels.hip tree_shap_kernel): [F][n] float32
    contributions of the device rows X [F][n] over the path table."""
    from .ops import P, check, explain_lib, stream

    F, n = X.shape
    dev = X.device
    Xc = X.float().contiguous()
    M = _bucket(maxm)
    wt = torch.from_numpy(shapley_weights(M).astype(np.float32)).to(dev)
    lvd = torch.from_numpy(lv).to(dev)
    eld = torch.from_numpy(el if el.size else np.zeros((1, 4), np.float32)).to(dev)
    out = torch.zeros((F, n), dtype=torch.float32, device=dev)
    setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
    rc = explain_lib().h2omx_tree_shap(P(Xc), Xc.stride(0), n, F, P(lvd), int(lv.shape[0]), P(eld), P(wt),
                                       maxm, P(out), P(setd), stream(dev))
    if rc != 0 and maxm > 32:
        raise RuntimeError(f"h2omx native call tree_shap failed with status {rc}: a path of this model splits on "
                           f"{maxm} distinct features; paths with more than 32 distinct features are unsupported "
                           "on the device")
    check(rc, "tree_shap")
    return out


def baseline_weights(M: int = 32) -> np.ndarray:
    """T[a][c] = (a-1)! c! / (a+c)! for 1 <= a <= M, 0 <= c <= M (row 0 is
    zero).  For a leaf whose elements split into a followed only by the scored
    row and c followed only by the background row, T[a][c] is the Shapley
    weight of the former and T[c][a] (negated) that of the latter."""
    T = np.zeros((M + 1, M + 1), np.float64)
    for a in range(1, M + 1):
        for c in range(M + 1):
            T[a, c] = math.factorial(a - 1) * math.factorial(c) / math.factorial(a + c)
    return T


def _shap_background_numpy(X: np.ndarray, B: np.ndarray, lv, el, maxm, sets=None,
                           per_reference: bool = False) -> np.ndarray:
    """Interventional SHAP of rows X [F][n] against background rows B [F][nb]
    in float64: phi(x, b) per pair [F][n][nb] with ``per_reference``, else its
    mean over the background [F][n]."""
    F, n = X.shape
    nb = B.shape[1]
    T = baseline_weights(max(32, int(maxm)))
    out = np.zeros((F, n, nb) if per_reference else (F, n), np.float64)
    step = max(1, (1 << 22) // max(1, nb * max(1, int(maxm))))      # bounds the [m][rows][nb] temporaries
    for start, m, vbits, _ in lv:
        if m == 0:
            continue
        v = float(np.int32(vbits).view(np.float32))
        E = el[start: start + m]
        _, ob = _follows(B, E, sets)
        ob = ob != 0
        for r0 in range(0, n, step):
            f, ox = _follows(X[:, r0: r0 + step], E, sets)
            ox = ox != 0
            only_x = ox[:, :, None] & ~ob[:, None, :]            # [m][rows][nb]
            only_b = ~ox[:, :, None] & ob[:, None, :]
            alive = (ox[:, :, None] | ob[:, None, :]).all(0)
            a, c = only_x.sum(0), only_b.sum(0)
            ws = np.where(alive, T[a, c], 0.0)
            wb = np.where(alive, T[c, a], 0.0)
            for j in range(m):
                phi = v * (only_x[j] * ws - only_b[j] * wb)
                if per_reference:
                    out[f[j], r0: r0 + step] += phi
                else:
                    out[f[j], r0: r0 + step] += phi.sum(1)
    return out if per_reference else out / nb


_CPU_CONTRIB_LIMIT = 2 << 30


def _background_chunk(n: int, nb: int, F: int, limit: int) -> int:
    """Background rows per slab of the averaged form: enough chunks to give a
    small scored frame ~1024 workgroups, as few slabs as that needs and as fit
    in ``limit`` bytes."""
    want = -(-1024 // max(1, -(-n // 256)))
    fit = max(1, limit // max(1, F * n * 4))
    return -(-nb // max(1, min(nb, want, fit)))


def _shap_background_device(X: torch.Tensor, Bm: torch.Tensor, lv, el, maxm, sets, chunk: int,
                            per_reference: bool) -> torch.Tensor:
    """The HIP path: [F][n] mean over the background (slabs of ``chunk``
    background rows, added in order), or [F][n * nb] x-major pairs."""
    from .ops import P, check, explain_lib, stream

    F, n = X.shape
    nb = int(Bm.shape[1])
    L = int(lv.shape[0])
    chunk = 1 if per_reference else int(chunk)
    nslabs = -(-nb // chunk)
    dev = X.device
    Xc = X.float().contiguous()
    Bc = Bm.float().contiguous()
    wt = torch.from_numpy(baseline_weights().astype(np.float32)).to(dev)
    lvd = torch.from_numpy(np.ascontiguousarray(lv, np.int32) if L else np.zeros((1, 4), np.int32)).to(dev)
    eld = torch.from_numpy(el if el.size else np.zeros((1, 4), np.float32)).to(dev)
    setd = torch.from_numpy(sets.view(np.int32).copy()).to(dev)
    bmask = torch.empty((max(L, 1), nb), dtype=torch.int32, device=dev)
    slabs = torch.zeros((nslabs, F, n), dtype=torch.float32, device=dev)
    out = None if per_reference else torch.empty((F, n), dtype=torch.float32, device=dev)
    check(explain_lib().h2omx_tree_shap_background(
        P(Xc), Xc.stride(0), n, F, P(Bc), Bc.stride(0), nb, P(lvd), L, P(eld), P(wt), maxm, P(setd), P(bmask),
        chunk, P(slabs), P(out), stream(dev)), "tree_shap_background")
    if per_reference:
        return slabs.permute(1, 2, 0).reshape(F, n * nb)      # [b][f][r] -> x-major pairs
    return out


# ---------------------------------------------------------------------------
# Ranked contributions (top_n / bottom_n / compare_abs)
# ---------------------------------------------------------------------------
def _rank_count(v, name: str) -> int:
    if v is None:
        return 0
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be an integer, got {v!r}")
    if not math.isfinite(v) or int(v) != v:
        raise ValueError(f"{name} must be an integer, got {v!r}")
    return int(v)


def _rank_spec(top_n, bottom_n, F: int) -> tuple[int, int]:
    """(kt, kb): how many features of the descending and of the ascending
    order H2O's ``top_n`` / ``bottom_n`` ask for among F; (0, 0) is the
    unsorted frame.  A negative count means all of them."""
    t, b = _rank_count(top_n, "top_n"), _rank_count(bottom_n, "bottom_n")
    if t == 0 and b == 0:
        return 0, 0
    if t != 0 and (t < 0 or b < 0):
        return F, 0
    if t == 0:
        return (0, F) if b < 0 else (0, min(b, F))
    if b == 0:
        return min(t, F), 0
    return (F, 0) if t + b >= F else (t, b)


def _output_format(output_format) -> None:
    # "Original" and "Compact" name the same frame here: no model one-hot expands a contribution column
    if str(output_format).lower() not in ("original", "compact"):
        raise ValueError(f"output_format must be 'Original' or 'Compact', got {output_format!r}")


def _rank_numpy(phi: np.ndarray, kt: int, kb: int, compare_abs: bool):
    """The oracle of :func:`_rank_device` on phi [F][n] float32: (idx int32,
    val float32), both [kt + kb][n].  Descending sorts (-key, index) and
    ascending (key, index), each a stable argsort, so ties go to the lower
    index in both and the ascending order is not the descending one reversed."""
    phi = np.asarray(phi, np.float32)
    key = np.abs(phi) if compare_abs else phi
    desc = np.argsort(-key, axis=0, kind="stable")[:kt]
    asc = np.argsort(key, axis=0, kind="stable")[:kb]
    idx = np.concatenate([desc, asc], 0)
    return idx.astype(np.int32), np.take_along_axis(phi, idx, 0)


def _rank_device(phi: torch.Tensor, kt: int, kb: int, compare_abs: bool):
    """The HIP path (csrc/explain_kernels.hip contrib_rank_kernel) on a device
    tensor phi [F][n] float32 whose rows are contiguous."""
    from .ops import P, check, explain_lib, stream

    F, n = (int(a) for a in phi.shape)
    if phi.dtype != torch.float32 or (n > 1 and phi.stride(1) != 1) or (F > 1 and phi.stride(0) < n):
        phi = phi.float().contiguous()
    ld = max(int(phi.stride(0)), n) if F > 1 else n
    idx = torch.empty((kt + kb, n), dtype=torch.int32, device=phi.device)
    val = torch.empty((kt + kb, n), dtype=torch.float32, device=phi.device)
    check(explain_lib().h2omx_contrib_rank(P(phi), ld, n, F, kt, kb, int(bool(compare_abs)), P(idx), P(val),
                                           stream(phi.device)), "contrib_rank")
    return idx, val


def _rank(phi: torch.Tensor, kt: int, kb: int, compare_abs: bool):
    if phi.is_cuda:
        return _rank_device(phi, kt, kb, compare_abs)
    idx, val = _rank_numpy(phi.float().numpy(), kt, kb, compare_abs)
    return torch.from_numpy(idx), torch.from_numpy(val)


def _ranked_frame(names, idx: torch.Tensor, val: torch.Tensor, lead_vecs, bias: Vec, *, kt: int) -> Frame:
    """``lead_vecs``, then top_feature_i / top_value_i for the kt first slots
    of idx / val and bottom_feature_i / bottom_value_i for the rest, then
    ``bias``.  The feature columns are categorical over ``names``."""
    dom = list(names)
    vecs = list(lead_vecs)
    for s in range(idx.shape[0]):
        side, i = ("top", s + 1) if s < kt else ("bottom", s - kt + 1)
        vecs.append(Vec(f"{side}_feature_{i}", idx[s], ENUM, dom))
        vecs.append(Vec(f"{side}_value_{i}", val[s], "real"))
    vecs.append(bias)
    return Frame(vecs)


def rank_contributions(frame: Frame, top_n, bottom_n, compare_abs: bool, nlead: int = 0) -> Frame:
    """The ranked form of an unsorted contribution frame: ``nlead`` leading
    index columns, the contribution columns, ``BiasTerm``.  Shared by the models
    whose contributions are not [F][n] planes to begin with (GLM / GAM)."""
    cols = frame.vecs[nlead:-1]
    kt, kb = _rank_spec(top_n, bottom_n, len(cols))
    if kt + kb == 0:
        return frame
    idx, val = _rank(torch.stack([v.data.float() for v in cols]), kt, kb, bool(compare_abs))
    return _ranked_frame([v.name for v in cols], idx, val, frame.vecs[:nlead], frame.vecs[-1], kt=kt)


def _contributions_background(model, ens, X, Bm, lv, el, maxm, sets, per_reference: bool, kt: int = 0, kb: int = 0,
                              compare_abs: bool = False) -> Frame:
    F, n = X.shape
    nb = int(Bm.shape[1])
    if nb == 0:
        raise ValueError("background_frame has no rows")
    Bm = Bm.to(X.device)
    L = int(lv.shape[0])
    result = 4 * n * (nb * (F + 3) if per_reference else F + 1)
    if per_reference:
        result += 8 * (kt + kb) * n * nb
    if X.is_cuda:
        if maxm > 32:
            raise ValueError(f"a path of this model splits on {maxm} distinct features; the device kernel takes 32")
        limit = torch.cuda.mem_get_info(X.device)[0] // 2
        chunk = 1 if per_reference else _background_chunk(n, nb, F, limit)
        nslabs = -(-nb // chunk)
        slab = 4 * (nslabs * F * n + L * nb)
    else:
        limit, chunk, nslabs, slab = _CPU_CONTRIB_LIMIT, nb, 1, 0
    if max(result, slab) > limit:
        raise ValueError(f"predict_contributions of {n} rows against {nb} background rows needs {result} bytes for "
                         f"the result and {slab} bytes of work space; the limit is {limit} bytes: use fewer "
                         "background rows or score the frame in parts")
    margin_b = ens.raw_margin(Bm)[0].float()
    if X.is_cuda:
        if nslabs > 65535:
            raise ValueError(f"output_per_reference takes at most 65535 background rows on the device, got {nb}")
        out = _shap_background_device(X, Bm, lv, el, maxm, sets, chunk, per_reference)
    else:
        ref = _shap_background_numpy(X.double().numpy(), Bm.double().numpy(), lv, el, maxm, sets, per_reference)
        out = torch.from_numpy(ref.reshape(F, -1).astype(np.float32))
    dev = out.device
    vecs = []
    if per_reference:
        rows = torch.arange(n, dtype=torch.float32, device=dev)
        refs = torch.arange(nb, dtype=torch.float32, device=dev)
        vecs += [Vec("RowIdx", rows.repeat_interleave(nb), INT), Vec("BackgroundRowIdx", refs.repeat(n), INT)]
        bias = margin_b.to(dev).repeat(n)
    else:
        bias = torch.full((n,), float(margin_b.double().mean()), dtype=torch.float32, device=dev)
    if kt + kb:
        idx, val = _rank(out, kt, kb, compare_abs)
        return _ranked_frame(model.x, idx, val, vecs, Vec("BiasTerm", bias, "real"), kt=kt)
    vecs += [Vec(c, out[j], "real") for j, c in enumerate(model.x)]
    vecs.append(Vec("BiasTerm", bias, "real"))
    return Frame(vecs)


# ---------------------------------------------------------------------------
# DeepSHAP (Deep Learning models)
# ---------------------------------------------------------------------------
# pairs per block on the device: one GEMM launch takes 65535 row tiles of at least 64 rows
_DEEPSHAP_MAX_PAIRS = 65535 * 64
_DEEPSHAP_CPU_BLOCK = 1 << 24        # float64 elements of one [rows][nb][width] temporary on the CPU


def _deepshap_multiplier(act: int, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The rescale rule's multiplier r(a, b) = (f(a) - f(b)) / (a - b) of the
    activation ``act`` (1 Rectifier, 2 Tanh, 4 ExpRectifier) in the
    cancellation-free closed forms of csrc/explain_kernels.hip
    (deepshap_rescale_kernel), on broadcastable float64 tensors."""
    d = a - b
    one = torch.ones_like(d)
    if act == 2:
        nz = d != 0
        s = torch.where(nz, torch.tanh(d) / torch.where(nz, d, one), one)
        return s * (1.0 - torch.tanh(a) * torch.tanh(b))
    pa, pb = (a > 0).expand_as(d), (b > 0).expand_as(d)
    mixed = pa != pb
    den = torch.where(mixed, d, one).abs()                      # a - b or b - a, whichever is positive
    if act == 1:
        return torch.where(mixed, torch.where(pa, a, b) / den, (pa & pb).to(d.dtype))
    if act != 4:
        raise ValueError(f"no DeepSHAP multiplier for activation code {act}")
    a0, b0 = a.clamp(max=0.0), b.clamp(max=0.0)                 # the branches that read them have a, b <= 0
    up = torch.where(pa, a - torch.expm1(b0), b - torch.expm1(a0)) / den
    ad = d.abs()
    low = torch.where(ad == 0, torch.exp(a0),
                      torch.exp(torch.maximum(a0, b0)) * -torch.expm1(-ad) / torch.where(ad == 0, one, ad))
    return torch.where(mixed, up, torch.where(pa, one, low))


def _deepshap_pre64(act: int, Ws, biases, X: torch.Tensor) -> list:
    """float64 pre-activations [Z_1, ..., Z_L, Z_out] of the design rows X."""
    f = {1: torch.relu, 2: torch.tanh, 4: torch.nn.functional.elu}[act]
    Zs = []
    for W, b in zip(Ws, biases):
        Zs.append((f(Zs[-1]) if Zs else X.double()) @ W.T + b)
    return Zs


def _deepshap_host(act: int, Ws, w_out, xs: torch.Tensor, bs: torch.Tensor, Zx, Zb, scale: float, col_start,
                   per_reference: bool) -> torch.Tensor:
    """DeepSHAP in float64 on the CPU, block by block of scored rows: [C][n * nb]
    x-major pairs or the [C][n] mean over the background of the design rows xs
    [n][p] against bs [nb][p].  ``Ws`` are the hidden layers' weights, ``w_out``
    [h_L] the output row, ``Zx`` / ``Zb`` the hidden pre-activations."""
    n, p = xs.shape
    nb = int(bs.shape[0])
    C = len(col_start) - 1
    xs, bs = xs.double(), bs.double()
    out = torch.zeros((C, n * nb if per_reference else n), dtype=torch.float64)
    width = max([p] + [int(W.shape[0]) for W in Ws])
    step = max(1, _DEEPSHAP_CPU_BLOCK // max(1, nb * width))
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        G = w_out.expand(i1 - i0, nb, -1)
        for l in range(len(Ws) - 1, -1, -1):
            U = G * _deepshap_multiplier(act, Zx[l][i0:i1, None, :], Zb[l][None, :, :])
            G = U @ Ws[l]
        phi = scale * G * (xs[i0:i1, None, :] - bs[None, :, :])                        # [rows][nb][p]
        fold = torch.stack([phi[..., col_start[c]: col_start[c + 1]].sum(-1) for c in range(C)])
        if per_reference:
            out[:, i0 * nb: i1 * nb] = fold.reshape(C, -1)
        else:
            out[:, i0:i1] = fold.sum(2) / nb
    return out


def _deepshap_rows(nb: int, width: int, budget: int) -> int:
    """Scored rows per block of the device path: the two [rows * nb][width]
    float32 work buffers within ``budget`` bytes and one GEMM launch."""
    one = 2 * 4 * nb * width
    rows = min(int(budget) // one, _DEEPSHAP_MAX_PAIRS // nb, (2 ** 31 - 1) // (nb * width))
    if rows < 1:
        raise ValueError(f"predict_contributions of one row against {nb} background rows needs {one} bytes of work "
                         f"space; the limit is {int(budget)} bytes and {_DEEPSHAP_MAX_PAIRS} pairs per block: use "
                         "fewer background rows")
    return rows


def _deepshap_device(act: int, Ws, w_out: torch.Tensor, xs: torch.Tensor, bs: torch.Tensor, Zx, Zb, scale: float,
                     col_start, per_reference: bool, *, _budget: int | None = None) -> torch.Tensor:
    """The HIP path (csrc/explain_kernels.hip deepshap_rescale_kernel,
    deepshap_fold_kernel and the project's GEMM between them): float32
    [C][n * nb] x-major pairs or the [C][n] background mean.  ``Zx`` / ``Zb``
    are the hidden pre-activations of xs [n][p] / bs [nb][p].  Scored rows go
    in blocks whose two work buffers fit ``_budget`` bytes (half of the free
    device memory by default)."""
    from .ops import P, check, explain_lib, stream
    from .ops import dense as OD

    n, p = (int(a) for a in xs.shape)
    nb = int(bs.shape[0])
    C = len(col_start) - 1
    dev = xs.device
    L = len(Ws)
    width = max([p] + [int(W.shape[0]) for W in Ws])
    if _budget is None:
        _budget = torch.cuda.mem_get_info(dev)[0] // 2
    rows = min(_deepshap_rows(nb, width, _budget), max(n, 1))
    out = torch.empty((C, n * nb if per_reference else n), dtype=torch.float32, device=dev)
    ldo = int(out.shape[1])
    if n == 0:
        return out
    bufs = [torch.empty((rows * nb * width,), dtype=torch.float32, device=dev) for _ in range(2 if L else 1)]
    cs = torch.tensor(list(col_start), dtype=torch.int32, device=dev)
    lib, st = explain_lib(), stream(dev)
    xs, bs = xs.float().contiguous(), bs.float().contiguous()
    Ws = [W.float().contiguous() for W in Ws]
    Zx = [Z.float().contiguous() for Z in Zx]
    Zb = [Z.float().contiguous() for Z in Zb]
    w_out = w_out.float().contiguous()
    for i0 in range(0, n, rows):
        ni = min(rows, n - i0)
        pairs = ni * nb
        cur = 0
        if L == 0:
            bufs[0][: pairs * p].view(pairs, p).copy_(w_out.expand(pairs, p))
        for l in range(L - 1, -1, -1):
            h = int(Ws[l].shape[0])
            U = bufs[cur][: pairs * h].view(pairs, h)
            # the top layer's multipliers are the output row itself, passed as a vector
            check(lib.h2omx_deepshap_rescale(P(w_out if l == L - 1 else U), int(l == L - 1), P(Zx[l][i0: i0 + ni]),
                                             P(Zb[l]), P(U), ni, nb, h, act, st), "deepshap_rescale")
            k = int(Ws[l].shape[1])
            OD.gemm(U, Ws[l], out=bufs[1 - cur][: pairs * k].view(pairs, k))
            cur = 1 - cur
        dst = out[:, i0 * nb if per_reference else i0:]
        check(lib.h2omx_deepshap_fold(P(bufs[cur]), P(xs[i0: i0 + ni]), P(bs), P(cs), float(scale), ni, nb, p, C,
                                      int(not per_reference), ldo, P(dst), st), "deepshap_fold")
    return out


def _contributions_deeplearning(model, frame: Frame, background_frame: Frame | None, per_reference: bool, top_n,
                                bottom_n, compare_abs: bool, *, _budget: int | None = None) -> Frame:
    """DeepSHAP (DeepLIFT's rescale rule) of a Deep Learning model against the
    rows of ``background_frame``: docs/ALGORITHMS.md, "Explanations"."""
    if model.autoencoder:
        raise ValueError("predict_contributions does not support autoencoders: there is no single output to explain")
    if model.category not in (ModelCategory.REGRESSION, ModelCategory.BINOMIAL):
        raise ValueError("predict_contributions supports regression and binomial Deep Learning models, not "
                         f"multinomial ones ({len(model.response_domain or [])} classes)")
    if model.act == 3:
        raise ValueError("predict_contributions does not support the Maxout activation: the rescale rule needs an "
                         "elementwise activation")
    if model.params.get("offset_column"):
        raise ValueError("predict_contributions does not support Deep Learning models fitted with an offset_column")
    if background_frame is None:
        raise ValueError("predict_contributions of a Deep Learning model needs a background_frame: DeepSHAP "
                         "explains a row against reference rows")
    design = model.design
    cols, col_start = [], [0]
    for c in design.x:
        k = sum(1 for col, _ in design.spec if col == c)
        if k:
            cols.append(c)
            col_start.append(col_start[-1] + k)
    # a predictor's design columns are adjacent (DesignInfo.spec), so a column range per predictor is enough
    owner = [c for j, c in enumerate(cols) for _ in range(col_start[j], col_start[j + 1])]
    assert owner == [col for col, _ in design.spec]
    C = len(cols)
    kt, kb = _rank_spec(top_n, bottom_n, C)
    xs = model._rows(model.adapt_frame(frame))                                        # [n][p]
    bs = model._rows(model.adapt_frame(background_frame)).to(xs.device)
    n, p = (int(a) for a in xs.shape)
    nb = int(bs.shape[0])
    if nb == 0:
        raise ValueError("background_frame has no rows")
    dev = xs.device
    result = 4 * n * (nb * (C + 3) if per_reference else C + 1)
    if per_reference:
        result += 8 * (kt + kb) * n * nb
    limit = torch.cuda.mem_get_info(dev)[0] // 2 if xs.is_cuda else _CPU_CONTRIB_LIMIT
    if result > limit:
        raise ValueError(f"predict_contributions of {n} rows against {nb} background rows needs {result} bytes for "
                         f"the result; the limit is {limit} bytes: use fewer background rows or score the frame in "
                         "parts")
    net = model.net
    L = len(net.layers) - 1
    binomial = model.category == ModelCategory.BINOMIAL
    scale = 1.0 if binomial else float(model.y_sd)
    Wo = net.W(L).to(dev)
    w_out = (Wo[1] - Wo[0]) if binomial else Wo[0]
    Ws = [net.W(i).to(dev) for i in range(L)]
    if xs.is_cuda:
        Zx, Zb = model.preactivations(xs), model.preactivations(bs)
        zb = Zb[-1]
        out = _deepshap_device(model.act, Ws, w_out, xs, bs, Zx[:-1], Zb[:-1], scale, col_start, per_reference,
                               _budget=_budget)
    else:
        Wd = [net.W(i).double() for i in range(L + 1)]
        bd = [net.b(i).double() for i in range(L + 1)]
        Zx, Zb = _deepshap_pre64(model.act, Wd, bd, xs), _deepshap_pre64(model.act, Wd, bd, bs)
        zb = Zb[-1]
        out = _deepshap_host(model.act, Wd[:L], w_out.double(), xs, bs, Zx[:-1], Zb[:-1], scale, col_start,
                             per_reference).float()
    margin_b = ((zb[:, 1] - zb[:, 0]) if binomial else zb[:, 0] * model.y_sd + model.y_mean).float()
    vecs = []
    if per_reference:
        rows = torch.arange(n, dtype=torch.float32, device=dev)
        refs = torch.arange(nb, dtype=torch.float32, device=dev)
        vecs += [Vec("RowIdx", rows.repeat_interleave(nb), INT), Vec("BackgroundRowIdx", refs.repeat(n), INT)]
        bias = margin_b.repeat(n)
    else:
        bias = torch.full((n,), float(margin_b.double().mean()), dtype=torch.float32, device=dev)
    if kt + kb:
        idx, val = _rank(out, kt, kb, compare_abs)
        return _ranked_frame(cols, idx, val, vecs, Vec("BiasTerm", bias, "real"), kt=kt)
    vecs += [Vec(c, out[j], "real") for j, c in enumerate(cols)]
    vecs.append(Vec("BiasTerm", bias, "real"))
    return Frame(vecs)


def predict_contributions(model, frame: Frame, *, background_frame: Frame | None = None,
                          output_per_reference: bool = False, top_n=None, bottom_n=None, compare_abs: bool = False,
                          output_format: str = "Original") -> Frame:
    """Path-dependent TreeSHAP, or with ``background_frame`` interventional
    (baseline) SHAP: every scored row x is explained against every background
    row b by the Shapley values of the game "coalition features from x, the
    rest from b".  The default averages over the background (one row per
    scored row, ``BiasTerm`` = mean background margin);
    ``output_per_reference`` returns one row per pair, x-major, led by
    ``RowIdx`` and ``BackgroundRowIdx``, with ``BiasTerm`` = margin(b).

    ``top_n`` / ``bottom_n`` give the ranked form of any of the three: per row
    (per pair) the strongest features of the descending and of the ascending
    order as ``top_feature_i`` / ``top_value_i`` and ``bottom_feature_i`` /
    ``bottom_value_i`` (see :func:`_rank_spec`); ``compare_abs`` orders by
    magnitude, the values keep their sign.  Ties go to the lower column index
    in both orders.

    A Deep Learning model needs ``background_frame`` and is explained by
    DeepSHAP (:func:`_contributions_deeplearning`), in the same forms."""
    _output_format(output_format)
    if model.algo == "deeplearning":
        return _contributions_deeplearning(model, frame, background_frame, bool(output_per_reference), top_n, bottom_n,
                                           bool(compare_abs))
    ens = getattr(model, "ens", None)
    if ens is None or model.algo not in ("gbm", "drf", "xgboost", "generic"):
        raise NotImplementedError(f"predict_contributions is available for tree models, not {model.algo}")
    if ens.K != 1:
        raise NotImplementedError("predict_contributions supports regression and binomial tree models (as in H2O)")
    if output_per_reference and background_frame is None:
        raise ValueError("output_per_reference=True needs a background_frame")
    frame = model.adapt_frame(frame)
    X = model._matrix(frame) if hasattr(model, "_matrix") else frame.feature_matrix(model.x)
    F, n = X.shape
    kt, kb = _rank_spec(top_n, bottom_n, F)
    nt = ens.ntrees
    scale = 1.0 / nt if (ens.average and nt > 0) else 1.0
    cb = getattr(ens, "catbits", None)
    lv, el, expected, maxm, sets = tree_paths(ens.trees[:nt], scale, None if cb is None else cb[:nt])
    if background_frame is not None:
        bg = model.adapt_frame(background_frame)
        Bm = model._matrix(bg) if hasattr(model, "_matrix") else bg.feature_matrix(model.x)
        return _contributions_background(model, ens, X, Bm, lv, el, maxm, sets, bool(output_per_reference), kt, kb,
                                         bool(compare_abs))
    bias = expected + (0.0 if ens.average else float(ens.init_f[0]))
    if X.is_cuda:
        out = _shap_device(X, lv, el, maxm, sets)
    else:
        out = torch.from_numpy(_shap_numpy(X.double().numpy(), lv, el, maxm, sets).astype(np.float32))
    if kt + kb:
        idx, val = _rank(out, kt, kb, bool(compare_abs))
        bias_vec = Vec("BiasTerm", torch.full((n,), float(bias), dtype=torch.float32, device=out.device), "real")
        return _ranked_frame(model.x, idx, val, [], bias_vec, kt=kt)
    vecs = [Vec(c, out[j], "real") for j, c in enumerate(model.x)]
    vecs.append(Vec("BiasTerm", torch.full((n,), float(bias), dtype=torch.float32, device=out.device), "real"))
    return Frame(vecs)


# ---------------------------------------------------------------------------
# Friedman-Popescu H statistic
# ---------------------------------------------------------------------------
H_MAX_VARS = 10          # NumPy path
H_MAX_VARS_DEVICE = 6    # friedman_h_pd_kernel<K> is instantiated for K = 2 .. 6


def _h_leaf_table(lv, el, var_idx) -> dict:
    """Host records of the H statistic's partial dependence on the variables
    ``var_idx`` (feature rows, bit j of a subset mask S stands for
    ``var_idx[j]``), from the path table of :func:`tree_paths`.  Leaves whose
    path touches a variable are kept: ``hdr`` [L][2k + 2] float32 = {lo_j, hi_j
    per variable (-inf, +inf where untouched), na_ok mask, untouched mask (both
    as bits)} and ``w`` [L][2^k] float64 with w[S] = v prod_{e not in S} z_e
    (float64 products of the table's float32 z; w[0] pads).  A term that no
    row can switch off, S without a touched variable or a leaf that touches
    none, is the same for every row: it is left out of ``w`` (zero) and summed
    into ``const`` [2^k - 1]."""
    k = len(var_idx)
    nsub1 = 1 << k
    S = np.arange(nsub1)
    inS = ((S[:, None] >> np.arange(k)) & 1).astype(bool)                # [2^k][k]
    pos = {int(f): j for j, f in enumerate(var_idx)}
    hdr, w = [], []
    const = np.zeros(nsub1, np.float64)
    for start, m, vbits, _ in lv:
        v = float(np.int32(vbits).view(np.float32))
        E = el[start: start + m]
        feats = E[:, 0].view(np.int32)
        h = np.empty(2 * k + 2, np.float32)
        h[0:2 * k:2], h[1:2 * k:2] = -np.inf, np.inf
        z = np.ones(k, np.float64)
        touched = na = 0
        other = 1.0
        for e, fi in zip(E, feats):
            j = pos.get(int(fi) & 0x1FFFFFFF)
            if j is None:
                other *= float(e[1])
                continue
            h[2 * j], h[2 * j + 1] = e[2], e[3]
            z[j] = float(e[1])
            touched |= 1 << j
            na |= ((int(fi) >> 30) & 1) << j
        ws = v * other * np.where(inS, 1.0, z).prod(1)
        fold = (S & touched) == 0
        const += np.where(fold, ws, 0.0)
        if touched:
            untouched = (nsub1 - 1) & ~touched
            h[2 * k:] = np.array([na | untouched, untouched], np.uint32).view(np.float32)
            hdr.append(h)
            w.append(np.where(fold, 0.0, ws))
    return {"k": k, "vars": [int(f) for f in var_idx], "const": const[1:].copy(),
            "hdr": np.asarray(hdr, np.float32).reshape(-1, 2 * k + 2),
            "w": np.asarray(w, np.float64).reshape(-1, nsub1)}


def _h_pd_numpy(X: np.ndarray, table: dict, const: bool = True) -> np.ndarray:
    """Partial dependence [2^k - 1][n] of rows X [F][n] on every non-empty
    subset of the table's variables, in float64 (row S - 1 is subset S; the
    model's link space without ``init_f``).  ``const=False`` leaves the
    row-independent part out."""
    k, hdr, w = table["k"], table["hdr"], table["w"]
    nsub = (1 << k) - 1
    n = X.shape[1]
    L = hdr.shape[0]
    out = np.zeros((nsub, n), np.float64)
    x = X[table["vars"]]                                                 # [k][n]
    words = hdr[:, 2 * k:].view(np.uint32).astype(np.int64)              # [L][2] = na_ok, untouched
    step = max(1, (1 << 22) // max(1, L))                                # bounds the [L][rows] temporaries
    for r0 in range(0, n if L else 0, step):
        xs = x[:, r0: r0 + step]
        mk = np.repeat(words[:, 1:2], xs.shape[1], 1)
        for j in range(k):
            with np.errstate(invalid="ignore"):
                o = np.where(np.isnan(xs[j])[None, :], ((words[:, 0:1] >> j) & 1) != 0,
                             (xs[j][None, :] > hdr[:, 2 * j, None]) & (xs[j][None, :] <= hdr[:, 2 * j + 1, None]))
            mk |= o.astype(np.int64) << j
        for s in range(1, nsub + 1):
            out[s - 1, r0: r0 + step] = (((mk & s) == s) * w[:, s, None]).sum(0)
    if const:
        out += table["const"][:, None]
    return out


def _h_chunks(n: int, L: int, nsub: int, limit: int) -> int:
    """Leaf chunks of the device path: enough to give a small frame ~1024
    workgroups (as ``_background_chunk``), as many as fit in ``limit`` bytes
    next to the result; the sized ValueError when one does not fit."""
    one = 8 * nsub * n
    if one > limit:
        raise ValueError(f"the H statistic of {nsub} variable subsets on {n} rows needs {one} bytes of work space; "
                         f"the limit is {limit} bytes: use a sample of the rows")
    want = -(-1024 // max(1, -(-n // 256)))
    fit = max(1, limit // max(1, one) - 1)
    return max(1, min(L, want, fit, 65535))


def _h_pd_device(X: torch.Tensor, table: dict, nchunks: int | None = None, const: bool = True) -> torch.Tensor:
    """The HIP path of :func:`_h_pd_numpy`: [2^k - 1][n] float64 on X's device.
    Leaves go to ``nchunks`` slabs that are added in order."""
    from .ops import P, check, explain_lib, stream

    k, hdr, w = table["k"], table["hdr"], table["w"]
    if not 2 <= k <= H_MAX_VARS_DEVICE:
        raise ValueError(f"the device kernel takes 2 to {H_MAX_VARS_DEVICE} variables, got {k}")
    nsub = (1 << k) - 1
    F, n = X.shape
    L = int(hdr.shape[0])
    dev = X.device
    if nchunks is None:
        nchunks = _h_chunks(n, L, nsub, torch.cuda.mem_get_info(dev)[0] // 2)
    out = torch.zeros((nsub, n), dtype=torch.float64, device=dev)
    if L and n:
        chunk = -(-L // max(1, min(int(nchunks), L)))
        nchunks = -(-L // chunk)
        Xc = X.float().contiguous()
        hd = torch.from_numpy(np.ascontiguousarray(hdr)).to(dev)
        wd = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
        slabs = torch.empty((nchunks, nsub, n), dtype=torch.float64, device=dev) if nchunks > 1 else None
        v = table["vars"] + [0] * (H_MAX_VARS_DEVICE - k)
        check(explain_lib().h2omx_friedman_h_pd(P(Xc), max(int(Xc.stride(0)), n), n, F, k, *v, P(hd), P(wd), L, chunk,
                                                P(slabs), P(out), stream(dev)), "friedman_h_pd")
    if const:
        out += torch.from_numpy(table["const"]).to(dev)[:, None]
    return out


def _h_sums(Fd: torch.Tensor) -> torch.Tensor:
    """[nsub + 1] float64: the sum of every subset's partial dependence over
    the rows, then the row count (additive over row shards)."""
    cnt = torch.tensor([float(Fd.shape[1])], dtype=torch.float64, device=Fd.device)
    return torch.cat([Fd.double().sum(1), cnt])


def _h_moments(Fd: torch.Tensor, means: torch.Tensor) -> torch.Tensor:
    """[2] float64 = {num, den} of H^2 over the rows of Fd [2^k - 1][n], the
    partial dependences centred by ``means`` [2^k - 1] (additive over row
    shards): num = sum_i (sum_S (-1)^(k - |S|) F~_S(x_i))^2, den = sum_i
    F~_full(x_i)^2."""
    nsub = Fd.shape[0]
    k = nsub.bit_length()
    sign = torch.tensor([(-1.0) ** (k - bin(s).count("1")) for s in range(1, nsub + 1)], dtype=torch.float64,
                        device=Fd.device)
    C = Fd.double() - means.to(Fd.device)[:, None]
    comb = (sign[:, None] * C).sum(0)
    return torch.stack([(comb * comb).sum(), (C[-1] * C[-1]).sum()])


def friedman_h(model, frame: Frame, variables, *, comm=None) -> float:
    """Friedman and Popescu's H statistic of ``variables`` (H2O ``model.h``):
    the share of the variance of their joint partial dependence that no
    proper subset explains, 0 for variables that do not interact.  The
    partial dependence is the weighted tree traversal evaluated on every row
    of ``frame``; NaN when the joint partial dependence does not vary or the
    ratio is not below one."""
    ens = getattr(model, "ens", None)
    if ens is None or model.algo not in ("gbm", "drf", "xgboost", "generic"):
        raise NotImplementedError(f"the H statistic is available for tree models, not {model.algo}")
    if ens.K != 1:
        raise NotImplementedError("the H statistic supports regression and binomial tree models (as in H2O)")
    variables = [variables] if isinstance(variables, str) else list(variables)
    if len(variables) < 2:
        raise ValueError(f"the H statistic needs at least 2 variables, got {variables}")
    for i, v in enumerate(variables):
        if v in variables[:i]:
            raise ValueError(f"variable {v!r} is listed twice")
        if v not in model.x:
            raise ValueError(f"variable {v!r} is not a predictor of the model")
        if model.feature_types.get(v) == ENUM:
            raise ValueError(f"variable {v!r} is categorical: the H statistic takes numerical variables only")
    frame = model.adapt_frame(frame)
    X = model._matrix(frame) if hasattr(model, "_matrix") else frame.feature_matrix(model.x)
    k = len(variables)
    kmax = H_MAX_VARS_DEVICE if X.is_cuda else H_MAX_VARS
    if k > kmax:
        raise ValueError(f"the H statistic takes at most {kmax} variables on "
                         f"{'the device' if X.is_cuda else 'the CPU'}, got {k}: {variables[kmax]!r} is one too many")
    n = int(X.shape[1])
    nsub = (1 << k) - 1
    nt = ens.ntrees
    scale = 1.0 / nt if (ens.average and nt > 0) else 1.0
    cb = getattr(ens, "catbits", None)
    lv, el, _, _, _ = tree_paths(ens.trees[:nt], scale, None if cb is None else cb[:nt])
    table = _h_leaf_table(lv, el, [model.x.index(v) for v in variables])
    # the row-independent part cancels in the centring and stays out: a variable that no tree uses
    # then has an exactly zero partial dependence
    if X.is_cuda:
        nchunks = _h_chunks(n, int(table["hdr"].shape[0]), nsub, torch.cuda.mem_get_info(X.device)[0] // 2)
        Fd = _h_pd_device(X, table, nchunks, const=False)
    else:
        _h_chunks(n, 1, nsub, _CPU_CONTRIB_LIMIT)
        Fd = torch.from_numpy(_h_pd_numpy(X.double().numpy(), table, const=False))
    sums = _h_sums(Fd)
    if comm is not None and comm.world_size > 1:
        comm.all_reduce_(sums)
    mom = _h_moments(Fd, sums[:-1] / sums[-1].clamp(min=1.0))
    if comm is not None and comm.world_size > 1:
        comm.all_reduce_(mom)
    num, den = (float(a) for a in mom)
    return math.sqrt(num / den) if num < den else float("nan")


# ---------------------------------------------------------------------------
# Partial dependence
# ---------------------------------------------------------------------------
def _response(model, P: torch.Tensor, target: str | None) -> torch.Tensor:
    if model.category == ModelCategory.BINOMIAL:
        return P[-1]
    if model.category == ModelCategory.MULTINOMIAL:
        dom = list(model.response_domain)
        return P[dom.index(target) if target is not None else 0]
    return P[0]


NA_LABEL = ".missing(NA)"
_PD_TREE_ALGOS = ("gbm", "drf", "xgboost", "generic")


def _pd_sorted(grid):
    """(cells ascending with the NaN cells last, the sorting permutation, the
    number of non-NaN cells) of a grid of float32 cell values."""
    g = np.asarray(grid, np.float32).reshape(-1)
    order = np.argsort(g, kind="stable")
    gs = np.ascontiguousarray(g[order])
    return gs, order, int((~np.isnan(gs)).sum())


def _pd_margin_chunks(model, X: torch.Tensor, fs: int, grid, ff: int | None = None, fixed=None, *,
                      budget: int | None = None, walks: torch.Tensor | None = None):
    """The HIP path (csrc/explain_kernels.hip pd_sweep_kernel): yields (r0, r1,
    margins [NY][G][K][r1 - r0]) over row ranges of the device matrix X [F][n],
    each margin buffer (and its copy in the caller's cell order, where the grid
    was not ascending) within ``budget`` bytes, half of the free device memory
    by default.  Cell g of slice y is ``ens.raw_margin`` of X with row ``fs``
    set to grid[g] and row ``ff`` to fixed[y], bit for bit.  ``walks`` (int64
    [1] on the device) is a debug output: the root-to-leaf walks made."""
    from .ops import P, check, explain_lib, stream

    ens = model.ens
    F, n = (int(a) for a in X.shape)
    dev = X.device
    gs, order, gn = _pd_sorted(grid)
    G = int(gs.shape[0])
    fx = None if ff is None else np.ascontiguousarray(np.asarray(fixed, np.float32).reshape(-1))
    NY = 1 if fx is None else int(fx.shape[0])
    K, nt = int(ens.K), int(ens.ntrees)
    T = nt * K
    if not 0 <= fs < F or (ff is not None and (not 0 <= ff < F or ff == fs)):
        raise ValueError(f"swept feature {fs} and fixed feature {ff} must be two different rows of the {F}-row matrix")
    if NY > 65535 or -(-G // 64) * K > 65535:
        raise ValueError(f"a partial dependence table of {NY} x {G} cells and {K} classes exceeds the launch grid")
    permuted = not np.array_equal(order, np.arange(G))
    per_row = 4 * NY * G * K * (2 if permuted else 1)
    if budget is None:
        budget = torch.cuda.mem_get_info(dev)[0] // 2
    rows = int(budget) // max(per_row, 1)
    if rows < 1:
        raise ValueError(f"the partial dependence margins of one row ({NY} x {G} cells, {K} classes) need {per_row} "
                         f"bytes; the limit is {int(budget)} bytes: use a smaller grid")
    rows = min(rows, 1 << 30)
    if G == 0 or NY == 0 or n == 0:
        yield 0, n, torch.empty((NY, G, K, n), dtype=torch.float32, device=dev)
        return
    Xc = X.float().contiguous()
    nodes, cbits, roots = ens.device_nodes(dev, T)
    # per node: how many of the ascending cells are <= thr (read at the nodes that split on fs)
    thr = np.ascontiguousarray(ens.trees[:T]["thr"]).reshape(-1)
    ub = torch.from_numpy(np.searchsorted(gs[:gn], thr, side="right").astype(np.int32)).to(dev)
    gd = torch.from_numpy(gs).to(dev)
    fd = None if fx is None else torch.from_numpy(fx).to(dev)
    init = None if ens.average else torch.from_numpy(ens.init_f.astype(np.float32)).to(dev)
    inv = torch.from_numpy(np.argsort(order)).to(dev) if permuted else None
    for r0 in range(0, n, rows):
        nc = min(rows, n - r0)
        out = torch.empty((NY, G, K, nc), dtype=torch.float32, device=dev)
        if ens.average:
            out.zero_()
        else:
            out.copy_(init[None, None, :, None].expand(NY, G, K, nc))
        if T:
            Xv = Xc[:, r0: r0 + nc]
            check(explain_lib().h2omx_pd_sweep(P(Xv), max(int(Xc.stride(0)), nc), nc, F, P(nodes), P(roots), T, K,
                                               P(cbits), fs, P(gd), P(ub), G, gn, -1 if ff is None else ff, P(fd), NY,
                                               P(out), P(walks), stream(dev)), "pd_sweep")
        if ens.average and nt > 0:
            out /= nt
        yield r0, r0 + nc, (out if inv is None else out.index_select(1, inv))


def _pd_margins_device(model, X: torch.Tensor, fs: int, grid, ff: int | None = None, fixed=None, *,
                       budget: int | None = None, walks: torch.Tensor | None = None) -> torch.Tensor:
    """Margins [NY][G][K][n] of every (fixed value, grid cell) by the sweep
    kernel; see :func:`_pd_margin_chunks`."""
    parts = [M for _, _, M in _pd_margin_chunks(model, X, fs, grid, ff, fixed, budget=budget, walks=walks)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 3)


def _pd_margins_loop(model, X: torch.Tensor, fs: int, grid, ff: int | None = None, fixed=None) -> torch.Tensor:
    """The oracle of :func:`_pd_margins_device`: the rows of the matrix
    overwritten and one ``ens.raw_margin`` call per cell (CPU or device X)."""
    ens = model.ens
    Xw = X.float().clone()
    g = np.asarray(grid, np.float32).reshape(-1)
    fx = [None] if ff is None else list(np.asarray(fixed, np.float32).reshape(-1))
    out = torch.empty((len(fx), len(g), int(ens.K), int(X.shape[1])), dtype=torch.float32, device=X.device)
    for y, fv in enumerate(fx):
        if ff is not None:
            Xw[ff] = float(fv)
        for c, gv in enumerate(g):
            Xw[fs] = float(gv)
            out[y, c] = ens.raw_margin(Xw)
    return out


def _pd_device_matrix(model, frame: Frame, cols) -> torch.Tensor | None:
    """The model's feature matrix of the adapted ``frame`` when the sweep kernel
    can answer for ``cols``: a tree ensemble scored by ``TreeModel.predict_raw``
    alone on a device matrix of which every column of ``cols`` is a row."""
    from .models.tree_models import TreeModel

    if getattr(model, "ens", None) is None or model.algo not in _PD_TREE_ALGOS or not isinstance(model, TreeModel):
        return None
    if type(model).predict_raw is not TreeModel.predict_raw or model.preprocessors or model.cat_encoder is not None:
        return None
    if any(c not in model.x for c in cols) or any(c not in frame.names for c in model.x):
        return None
    X = frame.feature_matrix(model.x)
    return X if X.is_cuda else None


def _pd_grid(model, frame: Frame, col: str, nbins: int, user_splits, include_na: bool, comm):
    """(cell values, labels) of one column: every level code of a categorical
    column, else ``user_splits`` or ``nbins`` equally spaced values over the
    column's global min .. max; with ``include_na`` one NA cell comes last."""
    v = frame.vec(col)
    if v.vtype == ENUM:
        dom = list(model.feature_domains.get(col) or v.domain or [])
        grid = list(range(len(dom)))
        labels = list(dom)
    else:
        if user_splits is not None:
            grid = [float(a) for a in user_splits]
        else:
            x = v.as_float()
            ok = ~torch.isnan(x)
            lo = x[ok].min() if bool(ok.any()) else torch.tensor(0.0)
            hi = x[ok].max() if bool(ok.any()) else torch.tensor(0.0)
            mm = torch.stack([lo.float(), -hi.float()]).to(x.device)
            if comm is not None and comm.world_size > 1:
                comm.all_reduce_(mm, "min")
            lo_v, hi_v = float(mm[0]), float(-mm[1])
            grid = list(np.linspace(lo_v, hi_v, nbins)) if hi_v > lo_v else [lo_v]
        labels = list(grid)
    if include_na:
        grid = grid + [float("nan")]
        labels = labels + [NA_LABEL if v.vtype == ENUM else float("nan")]
    return grid, labels


def _pd_vec(model, v: Vec, g, n: int) -> Vec:
    """Column ``v`` forced to the cell value ``g`` (NaN: NA) on ``n`` rows."""
    if v.vtype == ENUM:
        code = -1 if g != g else int(g)
        dom = list(model.feature_domains.get(v.name) or v.domain or [])
        return Vec(v.name, torch.full((n,), code, dtype=torch.int32, device=v.data.device), ENUM, dom)
    return Vec(v.name, torch.full((n,), float(g), dtype=torch.float32, device=v.data.device), v.vtype)


def _pd_responses_loop(model, frame: Frame, cols, grids, target):
    """The general path: per cell (the first column slowest) the response of
    ``model.predict_raw`` on the frame with the columns overwritten."""
    n = frame.nrows
    for g0 in grids[0]:
        v0 = _pd_vec(model, frame.vec(cols[0]), g0, n)
        for g1 in (grids[1] if len(cols) > 1 else [None]):
            repl = {cols[0]: v0}
            if len(cols) > 1:
                repl[cols[1]] = _pd_vec(model, frame.vec(cols[1]), g1, n)
            fr = Frame([repl.get(u.name, u) for u in frame.vecs])
            yield _response(model, model.predict_raw(fr), target).double()


def _pd_responses_device(model, frame: Frame, X: torch.Tensor, target, r0: int, r1: int, M):
    """The responses of one row range from its margins M [NY][G][K][rows]: the
    tail of ``TreeModel.predict_raw`` per cell."""
    off = None
    if model.params.get("offset_column"):
        off = frame.vec(model.params["offset_column"]).as_float()[r0:r1]
    for y in range(M.shape[0]):
        for c in range(M.shape[1]):
            yield _response(model, model.scores_from_margin(M[y, c], off, X.device), target).double()


def _pd_moments(responses, w) -> torch.Tensor | None:
    """[cells][2] float64 = {sum(w r), sum(w r^2)} of the cells' responses."""
    pairs = []
    for r in responses:
        wr = r if w is None else w.to(r.device) * r
        pairs.append(torch.stack([wr.sum(), (wr * r).sum()]))
    return torch.stack(pairs) if pairs else None


def partial_dependence(model, frame: Frame, col: str, nbins: int = 20, target: str | None = None,
                       user_splits=None, comm=None, *, col2: str | None = None, user_splits2=None,
                       weight_column: str | None = None, include_na: bool = False, row_index: int = -1) -> dict:
    """H2O PartialDependence for one column: {col, mean_response,
    stddev_response, std_error_mean_response} per grid value, or with ``col2``
    for the pair (``col`` varies slowest; each column keeps its 1-D grid).
    ``weight_column`` weights the rows (NaN or <= 0: left out), ``include_na``
    adds one NA cell per column, ``row_index >= 0`` gives the table of that one
    row of the whole frame.  Tree models on a device frame take the sweep
    kernel; everything else overwrites the columns and scores every cell."""
    cols = [col] if col2 is None else [col, col2]
    if col2 is not None and col2 == col:
        raise ValueError(f"a 2-D partial dependence pair names column {col!r} twice")
    for c in cols:
        if c not in frame.names:
            raise ValueError(f"partial dependence column {c!r} is not in the frame")
        if c == model.y:
            raise ValueError(f"partial dependence column {c!r} is the response column")
    if weight_column is not None:
        if weight_column in cols:
            raise ValueError(f"weight column {weight_column!r} is a partial dependence column")
        if weight_column not in frame.names:
            raise ValueError(f"weight column {weight_column!r} is not in the frame")
    frame = model.adapt_frame(frame)
    n = frame.nrows
    splits = [user_splits, user_splits2]
    grids, labels = zip(*[_pd_grid(model, frame, c, nbins, splits[j], include_na, comm) for j, c in enumerate(cols)])
    ncells = len(grids[0]) * (len(grids[1]) if len(cols) > 1 else 1)
    multi = comm is not None and comm.world_size > 1
    dev = frame.device
    single = row_index is not None and int(row_index) >= 0
    w = None
    if single:
        # the index counts rows of the whole frame: the owning shard alone contributes
        counts = [n]
        if multi:
            counts = [int(a) for a in comm.all_gather_cat(torch.tensor([n], dtype=torch.int64, device=dev)).tolist()]
        if int(row_index) >= sum(counts):
            raise ValueError(f"row_index {int(row_index)} is outside the frame of {sum(counts)} rows")
        local = int(row_index) - (sum(counts[:comm.rank]) if multi else 0)
        own = 0 <= local < n
        if own:
            frame = frame.rows(torch.tensor([local], dtype=torch.int64))
        sw = m = 1.0 if own else 0.0
    elif weight_column is not None:
        wv = frame.vec(weight_column).as_float().double()
        keep = ~torch.isnan(wv) & (wv > 0)
        w = torch.where(keep, wv, torch.zeros_like(wv))
        sw, m = float(w.sum()), float(keep.sum())
    else:
        sw = m = float(n)
    mom = None
    if not single or own:
        X = _pd_device_matrix(model, frame, cols)
        if X is not None:
            # sweep the last column; a pair pins the first one per slice
            ix = [model.x.index(c) for c in cols]
            g32 = [np.asarray(g, np.float32) for g in grids]
            chunks = _pd_margin_chunks(model, X, ix[-1], g32[-1], ix[0] if len(cols) > 1 else None,
                                       g32[0] if len(cols) > 1 else None)
            for r0, r1, M in chunks:
                part = _pd_moments(_pd_responses_device(model, frame, X, target, r0, r1, M),
                                   None if w is None else w[r0:r1])
                mom = part if mom is None else mom + part
        else:
            mom = _pd_moments(_pd_responses_loop(model, frame, cols, grids, target), w)
    if mom is None:
        mom = torch.zeros((ncells, 2), dtype=torch.float64, device=dev)
    # every cell's moments, sum(w) and the rows kept travel in one reduction
    st = torch.cat([mom.reshape(-1), torch.tensor([sw, m], dtype=torch.float64, device=mom.device)])
    if multi:
        comm.all_reduce_(st)
    st = [float(a) for a in st.cpu()]
    sw, cnt = st[-2], st[-1]
    den = sw if sw > 0 else 1.0
    rows = []
    for i in range(ncells):
        s, s2 = st[2 * i], st[2 * i + 1]
        mean = s / den
        sd = 0.0 if single else math.sqrt(max(s2 / den - mean * mean, 0.0) * cnt / max(cnt - 1.0, 1.0))
        se = sd / math.sqrt(max(cnt, 1.0))
        if len(cols) == 1:
            row = {col: labels[0][i]}
        else:
            row = {col: labels[0][i // len(grids[1])], col2: labels[1][i % len(grids[1])]}
        row.update(mean_response=mean, stddev_response=sd, std_error_mean_response=se)
        rows.append(row)
    if len(cols) == 1:
        return {"column": col, "target": target, "data": rows}
    return {"columns": [col, col2], "target": target, "data": rows}
