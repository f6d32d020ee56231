"""Python entry points of csrc/uplift_kernels.hip (Uplift DRF: level histograms, split
scan, row routing and forest scoring).

Device tensors only, on the current stream.  ``codes`` is the uint8 binned matrix
``[F][ld]`` of ``BinnedMatrix`` (``ld`` a multiple of 4, NA code ``nbt - 1``); a view of
its first ``n`` columns is taken as it is.  A row's category is ``2 (1 - treated) + y``.
All counts are int32 and added with integer atomics, the split scan's cumulative counts
are integer prefix sums, and the scoring sums are added in tree order: every result is
bit-identical between calls.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import P, _bind, check, stream

UPLIFT_SIGS = {
    # codes, ld, key, n, F, nbt, S, slab_rows, lds, H
    "h2omx_uplift_hist": "PLPLIIILIPS",
    # H, fmask, nvb, K, F, nbt, metric, min_rows, out
    "h2omx_uplift_splits": "PPPIIIIDPS",
    # codes, ld, n, nid, cat, rec, remap, built_right, K, P, F, nbt, key
    "h2omx_uplift_route": "PLLPPPPPIIIIPS",
    # codes, ld, n, F, nodes, leaves, T, M, nbt, pt, pc
    "h2omx_uplift_score": "PLLIPPIIIPPS",
}

MAX_NBT = 256                 # bins of a feature with the NA bin: four per lane of a wave
MAX_F = 32767                 # feat is an int16 of a packed node
MAX_ROWS = (1 << 31) - 1      # int32 counts
MAX_DEPTH = 64                # rounds of the tensor walk the kernel reproduces
# LDS a histogram workgroup may take: the whole 64 KB.  The size is set per launch, so shallow levels take a few
# hundred bytes; the budget only decides where the global path begins, and at the limit two workgroups still share a
# compute unit's 160 KB.
HIST_LDS_BYTES = 65536
HIST_STEP_ROWS = 1024         # rows of one step of a histogram workgroup
HIST_FILL = 4                 # (features x row slabs) fills the compute units this many times
REC_INTS = 16                 # int32 of a split record
METRICS = {"auto": 0, "kl": 0, "euclidean": 1, "chisquared": 2, "chi_squared": 2}


def uplift_lib() -> ctypes.CDLL:
    return _bind("uplift", UPLIFT_SIGS)


def _codes(codes: torch.Tensor, n: int, what: str) -> int:
    """The row stride of ``codes`` after the checks every entry makes."""
    if not (codes.is_cuda and codes.dtype == torch.uint8 and codes.dim() == 2 and codes.stride(1) == 1):
        raise ValueError(f"ops.uplift.{what}: codes is a uint8 device tensor [F][ld] with unit row stride")
    ld = codes.stride(0) if codes.shape[0] > 1 else max(codes.stride(0), codes.shape[1])
    if ld % 4 or ld < -(-n // 4) * 4 or codes.shape[1] < n or codes.data_ptr() % 4 or not 1 <= codes.shape[0] <= MAX_F:
        raise ValueError(f"ops.uplift.{what}: codes [F][ld] with ld % 4 == 0, ld >= n rounded up to 4, F <= {MAX_F}")
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(f"ops.uplift.{what}: 1 <= n <= {MAX_ROWS}")
    return ld


def hist_lds(S: int, nbt: int) -> bool:
    """True where the level's histogram [S][nbt][4] int32 fits the LDS budget, False
    where the rows add straight into global memory."""
    return S * nbt * 16 <= HIST_LDS_BYTES


def hist_slab_rows(n: int, F: int, cus: int) -> int:
    """Rows of a slab: features x slabs fills the compute units HIST_FILL times."""
    slabs = max(1, -(-HIST_FILL * cus // F))
    return max(1, -(-n // slabs // HIST_STEP_ROWS)) * HIST_STEP_ROWS


def category_hist(codes: torch.Tensor, key: torch.Tensor, S: int, nbt: int, lds: bool | None = None) -> torch.Tensor:
    """Counts int32 ``[S][F][nbt][4]`` of (slot, feature, bin, category) over the rows of
    ``key [n]`` int32 = slot * 4 + category, -1 for a row that does not count."""
    n = key.numel()
    ld = _codes(codes, n, "category_hist")
    F = codes.shape[0]
    if not (key.is_cuda and key.dtype == torch.int32 and key.is_contiguous() and key.device == codes.device):
        raise ValueError("ops.uplift.category_hist: key is a contiguous int32 tensor on the device of codes")
    if not (2 <= nbt <= MAX_NBT and 1 <= S and S * F * nbt * 4 < 1 << 31):
        raise ValueError(f"ops.uplift.category_hist: S={S} F={F} nbt={nbt}")
    if lds is None:
        lds = hist_lds(S, nbt)
    dev = codes.device
    H = torch.zeros((S, F, nbt, 4), dtype=torch.int32, device=dev)
    slab = hist_slab_rows(n, F, torch.cuda.get_device_properties(dev).multi_processor_count)
    check(uplift_lib().h2omx_uplift_hist(P(codes), ld, P(key), n, F, nbt, S, slab, int(lds), P(H), stream(dev)),
          "uplift_hist")
    return H


def best_splits(H: torch.Tensor, fmask: torch.Tensor, nvb: torch.Tensor, metric: str, min_rows: float) -> torch.Tensor:
    """Best split of every node of ``H [K][F][nbt][4]`` int32 over the features of
    ``fmask [K][F]`` (bool) and the bins below ``nvb [F] - 1`` (int32): one record of 16
    int32 per node, on the device (``split_records`` reads it)."""
    if not (H.is_cuda and H.dtype == torch.int32 and H.dim() == 4 and H.shape[3] == 4 and H.is_contiguous()):
        raise ValueError("ops.uplift.best_splits: H is a contiguous int32 device tensor [K][F][nbt][4]")
    K, F, nbt, _ = H.shape
    m = METRICS.get(str(metric).lower())
    if m is None:
        raise ValueError(f"uplift_metric {metric!r} (AUTO, KL, Euclidean, ChiSquared)")
    if not (K >= 1 and 1 <= F <= MAX_F and 2 <= nbt <= MAX_NBT and fmask.shape == (K, F) and fmask.dtype == torch.bool
            and nvb.shape == (F,) and nvb.dtype == torch.int32 and fmask.device == H.device == nvb.device):
        raise ValueError(f"ops.uplift.best_splits: K={K} F={F} nbt={nbt}, fmask bool [K][F], nvb int32 [F]")
    dev = H.device
    out = torch.empty((K, REC_INTS), dtype=torch.int32, device=dev)
    check(uplift_lib().h2omx_uplift_splits(P(H), P(fmask.contiguous()), P(nvb.contiguous()), K, F, nbt, m,
                                           float(min_rows), P(out), stream(dev)), "uplift_splits")
    return out


def split_records(rec: torch.Tensor) -> dict:
    """The records of ``best_splits`` on the host: gain fp64 [K], feat / bin / na_left
    int32 [K], left and node int32 [K][4] (nt, yt, nc, yc)."""
    r = rec.cpu().numpy()
    return {"gain": r[:, :2].copy().view(np.float64)[:, 0], "feat": r[:, 2], "bin": r[:, 3], "na_left": r[:, 4],
            "left": r[:, 6:10], "node": r[:, 10:14]}


def route(codes: torch.Tensor, nid: torch.Tensor, cat: torch.Tensor, rec: torch.Tensor, remap: torch.Tensor,
          built_right: torch.Tensor, nbt: int) -> torch.Tensor:
    """One level's routing.  ``nid [n]`` int32 (level-local node, -1 done) becomes
    ``2 remap[nid] + right`` or -1 in place; returns the next level's histogram key
    int32 ``[n]``: ``remap[nid] * 4 + cat`` where the row went to the child that
    ``built_right [P]`` names, else -1.  ``rec``: the device records of ``best_splits``."""
    n = nid.numel()
    ld = _codes(codes, n, "route")
    K, Pn = remap.numel(), built_right.numel()
    dev = codes.device
    for t in (nid, cat, remap, built_right, rec):
        if not (t.dtype == torch.int32 and t.is_contiguous() and t.device == dev):
            raise ValueError("ops.uplift.route: nid, cat, rec, remap and built_right are contiguous int32 on one device")
    if not (cat.numel() == n and rec.shape == (K, REC_INTS) and K >= 1 and Pn >= 1 and 2 <= nbt <= MAX_NBT):
        raise ValueError(f"ops.uplift.route: n={n} K={K} P={Pn} nbt={nbt}")
    key = torch.empty(n, dtype=torch.int32, device=dev)
    check(uplift_lib().h2omx_uplift_route(P(codes), ld, n, P(nid), P(cat), P(rec), P(remap), P(built_right), K, Pn,
                                          codes.shape[0], nbt, P(key), stream(dev)), "uplift_route")
    return key


@dataclass
class UpliftPlan:
    """A forest on one device: ``nodes [T][M]`` of 8 bytes {feat int16 (-1 leaf), bin
    uint8, na_left uint8, left int32} (as int64), ``leaves [T][M][2]`` = {pt, pc}."""
    nodes: torch.Tensor
    leaves: torch.Tensor
    nbt: int
    max_feat: int


NODE_DTYPE = np.dtype([("feat", "<i2"), ("bin", "u1"), ("na_left", "u1"), ("left", "<i4")])


def pack_forest(trees: list, device, nbt: int) -> UpliftPlan:
    """Pack the trees' flat arrays for ``forest_predict``.  Host work, once per (model,
    device).  Every inner node's children have to lie behind it and inside its tree:
    a walk then ends and stays in bounds."""
    T = len(trees)
    M = max((len(t["feat"]) for t in trees), default=0)
    if T < 1 or M < 1 or not 2 <= nbt <= MAX_NBT:
        raise ValueError("ops.uplift.pack_forest: at least one tree of at least one node, 2 <= nbt <= 256")
    nodes = np.zeros((T, M), NODE_DTYPE)
    nodes["feat"] = -1
    leaves = np.zeros((T, M, 2), np.float64)
    max_feat = -1
    for i, t in enumerate(trees):
        feat, left = np.asarray(t["feat"], np.int64), np.asarray(t["left"], np.int64)
        binv = np.asarray(t["bin"], np.int64)
        m = len(feat)
        inner = feat >= 0
        if m < 1 or feat.max() > MAX_F or (inner & ((left <= np.arange(m)) | (left + 1 >= m))).any() or \
                (inner & ((binv < 0) | (binv > 255))).any():
            raise ValueError(f"ops.uplift.pack_forest: tree {i} is not a forward-linked tree of 8-bit bins")
        nodes["feat"][i, :m] = np.where(inner, feat, -1)
        nodes["bin"][i, :m] = np.where(inner, binv, 0)
        nodes["na_left"][i, :m] = np.asarray(t["na_left"]) != 0
        nodes["left"][i, :m] = np.where(inner, left, 0)
        leaves[i, :m, 0], leaves[i, :m, 1] = t["pt"], t["pc"]
        max_feat = max(max_feat, int(feat.max()))
    return UpliftPlan(torch.from_numpy(nodes.view(np.int64)).to(device), torch.from_numpy(leaves).to(device), int(nbt),
                      max_feat)


def forest_predict(codes: torch.Tensor, plan: UpliftPlan, n: int | None = None):
    """Sums over the trees, in tree order, of the leaf ``(pt, pc)`` every row of ``codes``
    reaches -> two fp64 ``[n]``."""
    n = codes.shape[1] if n is None else int(n)
    dev = codes.device
    pt = torch.empty(n, dtype=torch.float64, device=dev)
    pc = torch.empty_like(pt)
    if n == 0:
        return pt, pc
    ld = _codes(codes, n, "forest_predict")
    if plan.nodes.device != dev or plan.max_feat >= codes.shape[0]:
        raise ValueError("ops.uplift.forest_predict: plan and codes on one device, every split feature a row of codes")
    T, M = plan.nodes.shape
    check(uplift_lib().h2omx_uplift_score(P(codes), ld, n, codes.shape[0], P(plan.nodes), P(plan.leaves), T, M,
                                          plan.nbt, P(pt), P(pc), stream(dev)), "uplift_score")
    return pt, pc
