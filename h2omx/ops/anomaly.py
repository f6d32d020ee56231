"""Python entry points of csrc/eif_kernels.hip (Extended Isolation Forest scoring).

Device tensors only: the scored matrix is the feature-major fp32 design
``Xraw [p][n]`` (NaN allowed, replaced by the training means as it is loaded),
the result fp32 ``[n]`` on the current stream.  The result is bit-identical
between calls and does not depend on the slab split: no floating-point atomics,
and the fp64 sum of the leaf values over the trees is exact.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import P, _bind, check, stream

ANOMALY_SIGS = {
    # Xraw, means, meta, ent, normals, n, p, T, cap, K, limit, slab_trees, dense, part, out
    "h2omx_eif_mean_length": "PPPPPLIIIIIIIPPS",
}

# the sparse walk (lane per row) serves forests with at most this many non-zeros per
# normal, the dense walk (unit of lanes per row) the others: the largest K of the sweep
# of scripts/eif_timing.py (p = 32, K 4 .. 32) at which the sparse walk was the faster
# one, which it was at every K measured (docs/ROADMAP.md, Round 21)
EIF_SPARSE_MAX_K = 32
EIF_DENSE_MAX_P = 256        # four values per lane in a unit of 64
EIF_MAX_LIMIT = 24
EIF_MAX_TREES = 1 << 20      # the fp64 sum of the leaf values stays exact
EIF_SPARSE_ROWS = 256        # rows of a workgroup
EIF_DENSE_ROWS = 64
# (row blocks x slabs) fills the compute units this many times over ...
EIF_FILL = 4
# ... unless the slab partials would pass the bytes of the scored matrix
EIF_PART_SHARE = 1
MAX_SLABS = 65535


def anomaly_lib() -> ctypes.CDLL:
    return _bind("eif", ANOMALY_SIGS)


@dataclass
class EifPlan:
    """A forest on one device.  ``meta [T][cap][2]`` = {offs, hval}; ``ent [T][cap][K][2]``
    = {dim as uint32 bits, val}, dims ascending, padded entries val = 0 at the node's first
    dim; ``normals [T][cap][p]``; ``hval [T][cap]`` (-1: inner node); ``means [p]``."""
    meta: torch.Tensor
    ent: torch.Tensor
    K: int
    normals: torch.Tensor
    hval: torch.Tensor
    means: torch.Tensor
    limit: int


def eif_pack(normals: np.ndarray, offs: np.ndarray, sizes: np.ndarray, means: np.ndarray, device) -> EifPlan:
    """Pack the heap-indexed forest ``normals [T][cap][p]``, ``offs [T][cap]``, ``sizes
    [T][cap]`` (leaf sizes, -1 inner) for the walk kernels.  Host work, once per (model,
    device)."""
    from ..models.isolation_forest import avg_path

    normals = np.ascontiguousarray(normals, np.float32)
    T, cap, p = normals.shape
    limit = (cap + 1).bit_length() - 2
    if T < 1 or p < 1 or cap != (2 << max(limit, 0)) - 1 or offs.shape != (T, cap) or sizes.shape != (T, cap):
        raise ValueError("ops.anomaly.eif_pack: normals [T][cap][p], offs and sizes [T][cap], cap = 2^(limit + 1) - 1")
    leaf = sizes >= 0
    # path value of a leaf: floor(log2(node + 1)) + c(size), both fp32, added in fp32
    depth = np.array([(v + 1).bit_length() - 1 for v in range(cap)], np.float32)
    cpath = np.where(leaf, avg_path(np.maximum(sizes, 0)), 0.0).astype(np.float32)
    hval = np.where(leaf, depth[None, :] + cpath, np.float32(-1.0)).astype(np.float32)
    # a walk is over after `limit` steps: the nodes it can stand on then have to be leaves
    reach = np.zeros((T, cap), bool)
    reach[:, 0] = True
    for v in range(cap // 2):
        reach[:, 2 * v + 1] = reach[:, 2 * v + 2] = reach[:, v] & ~leaf[:, v]
    if (reach[:, cap // 2:] & ~leaf[:, cap // 2:]).any():
        raise ValueError("ops.anomaly.eif_pack: an inner node at depth `limit` is reachable")
    nz = normals != 0
    cnt = nz.sum(-1)
    K = max(1, int(cnt.max()))
    idx = np.argsort(~nz, axis=-1, kind="stable")[..., :K]               # non-zero dims first, ascending
    valid = np.arange(K)[None, None, :] < cnt[..., None]
    ent = np.empty((T, cap, K, 2), np.uint32)
    ent[..., 0] = np.where(valid, idx, idx[..., :1])
    ent[..., 1] = np.where(valid, np.take_along_axis(normals, idx, -1), np.float32(0.0)).astype(np.float32).view(np.uint32)
    meta = np.stack([np.asarray(offs, np.float32), hval], -1)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)

    return EifPlan(dev(meta), dev(ent.view(np.int32)), K, dev(normals), dev(hval),
                   dev(np.asarray(means, np.float32)), limit)


def eif_dense(plan: EifPlan) -> bool:
    """True where the dense walk takes the forest, False for the sparse walk."""
    return plan.K > EIF_SPARSE_MAX_K


def eif_slab_trees(n: int, T: int, p: int, cus: int, block_rows: int = EIF_SPARSE_ROWS) -> int:
    """Trees per slab: enough slabs for row blocks x slabs to fill the machine EIF_FILL
    times over, capped so the [slab][n] fp64 partials stay within 1 / EIF_PART_SHARE of
    the bytes of the scored matrix."""
    blocks = -(-n // block_rows)
    slabs = -(-EIF_FILL * cus // blocks)
    cap = 4 * n * p // EIF_PART_SHARE // (8 * n)
    slabs = max(1, min(slabs, cap, T, MAX_SLABS))
    return -(-T // slabs)


def eif_mean_length(Xraw: torch.Tensor, plan: EifPlan, slab_trees: int | None = None) -> torch.Tensor:
    """Mean path value over the forest for every column of the feature-major design
    ``Xraw [p][n]`` -> fp32 [n].  Only the hyperplane products on a row's own paths are
    formed; the memory beyond the result is the [slabs][n] fp64 partials."""
    if not (Xraw.is_cuda and plan.meta.is_cuda and plan.meta.device == Xraw.device):
        raise ValueError("ops.anomaly.eif_mean_length: device tensors only, plan and matrix on one device")
    T, cap, p = plan.normals.shape
    dense = eif_dense(plan)
    if Xraw.dim() != 2 or Xraw.shape[0] != p:
        raise ValueError(f"ops.anomaly.eif_mean_length: Xraw [p][n] with p = {p}")
    if plan.limit > EIF_MAX_LIMIT or T > EIF_MAX_TREES or (dense and p > EIF_DENSE_MAX_P):
        raise ValueError(f"ops.anomaly.eif_mean_length: limit={plan.limit} T={T} p={p} K={plan.K}, the kernels take "
                         f"limit <= {EIF_MAX_LIMIT}, T <= {EIF_MAX_TREES} and p <= {EIF_DENSE_MAX_P} on the dense walk")
    Xraw = Xraw.to(torch.float32).contiguous()
    n = Xraw.shape[1]
    dev = Xraw.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if slab_trees is None:
        slab_trees = eif_slab_trees(n, T, p, torch.cuda.get_device_properties(dev).multi_processor_count,
                                    EIF_DENSE_ROWS if dense else EIF_SPARSE_ROWS)
    if not 1 <= slab_trees or -(-T // slab_trees) > MAX_SLABS:
        raise ValueError(f"ops.anomaly.eif_mean_length: slab_trees={slab_trees}")
    slabs = -(-T // slab_trees)
    part = torch.empty((slabs, n), dtype=torch.float64, device=dev) if slabs > 1 else None
    check(anomaly_lib().h2omx_eif_mean_length(P(Xraw), P(plan.means), P(plan.meta), P(plan.ent), P(plan.normals), n, p,
                                              T, cap, plan.K, plan.limit, int(slab_trees), int(dense), P(part), P(out),
                                              stream(dev)), "eif_mean_length")
    return out
