"""Python entry points of csrc/walk_kernels.hip (leaf ids, staged margins, feature counts).

Device tensors only: the walked matrix is the feature-major fp32 ``X [F][n]`` (NaN
allowed), every result lives on the current stream.  No call synchronises with the
host, and the results are bit-identical between calls and do not depend on the slab
split: ids and counts are integers, the staged margins a fixed sequence of fp64
additions per row.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import P, _bind, check, stream

WALK_SIGS = {
    "h2omx_walk_limits": "P",
    # X, ld, n, F, nodes, roots, catbits, T, cap, slab_trees, ids, reached
    "h2omx_walk_leaf": "PLLIPPPIIIPPS",
    # X, ld, n, F, nodes, roots, catbits, nt, K, cap, init_f, average, out
    "h2omx_walk_staged": "PLLIPPPIIIPIPS",
    # X, ld, n, F, nodes, roots, catbits, T, cap, slab_trees, part, cnt
    "h2omx_walk_counts": "PLLIPPPIIIPPS",
}

WALK_XLDS_MAX_F = 32         # widest matrix, and widest counter block, a workgroup keeps in LDS
WALK_ROWS = 256              # rows of a workgroup
WALK_MAX_STEPS = 64
WALK_MAX_CAP = 1 << 29       # left << 2 | flags is an int32
# (row blocks x slabs) fills the compute units this many times over ...
WALK_FILL = 4
# ... unless the int32 count partials [slabs][F][n] would pass this many bytes
WALK_PART_BYTES = 256 << 20
MAX_SLABS = 65535


def walk_lib() -> ctypes.CDLL:
    lib = _bind("walk", WALK_SIGS)
    lim = (ctypes.c_int * 2)()
    lib.h2omx_walk_limits(lim)
    if list(lim) != [WALK_XLDS_MAX_F, WALK_ROWS]:
        raise RuntimeError(f"walk kernel limits {list(lim)} differ from ops.walk")
    return lib


@dataclass
class WalkPlan:
    """An ensemble on one device.  ``nodes [T][cap][4]`` int32 = {feat (< 0: leaf), thr bits,
    left << 2 | categorical << 1 | na_left, value bits}; ``roots [T]`` = t * cap; ``used [T]``
    = largest reachable index + 1 (the kernels do not read it: the tree stage it was packed
    for lost its measurement); ``catbits`` as ``TreeEnsemble.device_nodes`` gives them.
    Host side: ``depth [T][cap]`` (-1: unreachable) and ``bits [T][cap]`` (bit d = went right
    at depth d) of every node's path, and ``paths``, the "LRRL" strings of the trees that
    ``path_strings`` has been asked for."""
    nodes: torch.Tensor
    roots: torch.Tensor
    used: torch.Tensor
    catbits: torch.Tensor | None
    T: int
    cap: int
    max_feat: int
    max_depth: int
    depth: np.ndarray
    bits: np.ndarray
    paths: dict = field(default_factory=dict)

    def path_strings(self, t: int) -> np.ndarray:
        """Object array [cap] of tree t's path strings (None at unreachable nodes), built once."""
        out = self.paths.get(t)
        if out is None:
            out = np.full(self.cap, None, object)
            for i in np.flatnonzero(self.depth[t] >= 0):
                b = int(self.bits[t, i])
                out[i] = "".join("R" if (b >> k) & 1 else "L" for k in range(int(self.depth[t, i])))
            self.paths[t] = out
        return out


def pack_walk(ens, dev) -> WalkPlan:
    """Pack the first ``ntrees * K`` trees of a ``TreeEnsemble`` for the walk kernels, cached
    on the ensemble.  Host work, once per (ensemble, device).  The children of every
    reachable inner node have to lie behind it and inside its tree, and no node may have two
    parents: a walk then ends and stays in bounds."""
    from ..models.tree.structs import CAT_SPLIT_BIT, NA_LEFT_BIT

    trees = ens.trees
    T = ens.ntrees * ens.K
    key = (T, str(dev), trees.shape, id(trees), id(ens.catbits))
    cache = getattr(ens, "_walk_plan", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    if trees.ndim != 2 or T < 1 or not 1 <= trees.shape[1] <= WALK_MAX_CAP:
        raise ValueError("ops.walk.pack_walk: trees [T][cap] with at least one tree")
    cap = trees.shape[1]
    cb = ens.catbits
    if cb is not None and (cb.ndim != 3 or cb.shape[0] < T or cb.shape[1:] != (cap, 8)):
        raise ValueError("ops.walk.pack_walk: catbits [T][cap][8]")
    feat = trees["feat"][:T].astype(np.int64)
    left = trees["left"][:T].astype(np.int64)
    depth = np.full((T, cap), -1, np.int8)
    bits = np.zeros((T, cap), np.int64)
    ft, fi, fb = np.arange(T), np.zeros(T, np.int64), np.zeros(T, np.int64)
    for d in range(WALK_MAX_STEPS + 1):
        if (depth[ft, fi] >= 0).any() or len(np.unique(ft * cap + fi)) != len(ft):
            raise ValueError("ops.walk.pack_walk: a node has two parents")
        depth[ft, fi], bits[ft, fi] = d, fb
        inner = feat[ft, fi] >= 0
        if d == WALK_MAX_STEPS or not inner.any():
            break
        ft, fi, fb = ft[inner], fi[inner], fb[inner]
        lc = left[ft, fi]
        if ((lc <= fi) | (lc + 1 >= cap)).any():
            raise ValueError("ops.walk.pack_walk: a child lies before its parent or outside its tree")
        ft, fi, fb = np.concatenate([ft, ft]), np.concatenate([lc, lc + 1]), \
            np.concatenate([fb, fb | (1 << min(d, 62))])
    reach = depth >= 0
    inner = reach & (feat >= 0)
    used = (np.where(reach, np.arange(cap)[None, :], 0).max(1) + 1).astype(np.int32)
    nl = trees["na_left"][:T].astype(np.int64)
    flags = (nl & NA_LEFT_BIT) | ((nl & CAT_SPLIT_BIT) if cb is not None else 0)
    rec = np.zeros((T, cap, 4), np.int32)
    rec[..., 0] = np.where(inner, feat, -1)
    rec[..., 1] = np.ascontiguousarray(trees["thr"][:T], np.float32).view(np.int32)
    rec[..., 2] = np.where(inner, (left << 2) | flags, 0)
    rec[..., 3] = np.ascontiguousarray(trees["value"][:T], np.float32).view(np.int32)
    plan = WalkPlan(torch.from_numpy(rec).to(dev), torch.arange(T, dtype=torch.int32, device=dev) * cap,
                    torch.from_numpy(used).to(dev), ens.device_nodes(dev, T)[1] if cb is not None else None, T, cap,
                    int(feat[inner].max()) if inner.any() else -1, int(depth.max()), depth, bits)
    ens._walk_plan = (key, plan)
    return plan


def walk_slab_trees(n: int, T: int, cus: int, slab_bytes: int = 0) -> int:
    """Trees per slab: enough slabs for row blocks x slabs to fill the machine WALK_FILL
    times over, capped so partials of ``slab_bytes`` per slab stay within WALK_PART_BYTES."""
    blocks = -(-n // WALK_ROWS)
    slabs = min(-(-WALK_FILL * cus // blocks), T, MAX_SLABS)
    if slab_bytes:
        slabs = min(slabs, WALK_PART_BYTES // slab_bytes)
    return -(-T // max(1, slabs))


def _args(X: torch.Tensor, plan: WalkPlan, what: str) -> torch.Tensor:
    if not (torch.is_tensor(X) and X.is_cuda and plan.nodes.device == X.device):
        raise ValueError(f"ops.walk.{what}: device tensors only, plan and matrix on one device")
    if X.dim() != 2 or X.shape[0] < 1 or plan.max_feat >= X.shape[0]:
        raise ValueError(f"ops.walk.{what}: X [F][n] with a row for every split feature (largest: {plan.max_feat})")
    return X.to(torch.float32).contiguous()


def _slabs(slab_trees, n: int, T: int, dev, what: str, slab_bytes: int = 0) -> int:
    if slab_trees is None:
        slab_trees = walk_slab_trees(n, T, torch.cuda.get_device_properties(dev).multi_processor_count, slab_bytes)
    slab_trees = min(int(slab_trees), T)
    if slab_trees < 1 or -(-T // slab_trees) > MAX_SLABS:
        raise ValueError(f"ops.walk.{what}: slab_trees={slab_trees}")
    return slab_trees


def leaf_ids(X: torch.Tensor, plan: WalkPlan, reached: bool = False, slab_trees: int | None = None):
    """Tree-local index of the node every column of ``X [F][n]`` ends on -> int32 ``[T][n]``;
    with ``reached`` also uint8 ``[T][cap]``, 1 at every node some column ended on."""
    X = _args(X, plan, "leaf_ids")
    n, dev = X.shape[1], X.device
    ids = torch.empty((plan.T, n), dtype=torch.int32, device=dev)
    hit = torch.zeros((plan.T, plan.cap), dtype=torch.uint8, device=dev) if reached else None
    if n:
        slab_trees = _slabs(slab_trees, n, plan.T, dev, "leaf_ids")
        check(walk_lib().h2omx_walk_leaf(P(X), X.stride(0), n, X.shape[0], P(plan.nodes), P(plan.roots),
                                         P(plan.catbits), plan.T, plan.cap, slab_trees, P(ids), P(hit), stream(dev)),
              "walk_leaf")
    return (ids, hit) if reached else ids


def staged_margins(X: torch.Tensor, plan: WalkPlan, init_f, K: int, average: bool) -> torch.Tensor:
    """Margins after every iteration -> fp32 ``[nt][K][n]``: per row and class an fp64 sum of
    the leaf values in tree order, from ``init_f [K]`` (boosted) or from 0 and divided by the
    iteration count (``average``), rounded to fp32 once."""
    X = _args(X, plan, "staged_margins")
    K = int(K)
    if K < 1 or plan.T % K or len(init_f) != K:
        raise ValueError(f"ops.walk.staged_margins: K={K} has to divide the {plan.T} trees, init_f [K]")
    n, dev = X.shape[1], X.device
    nt = plan.T // K
    out = torch.empty((nt, K, n), dtype=torch.float32, device=dev)
    if n:
        f0 = torch.from_numpy(np.asarray(init_f, np.float64).copy()).to(dev)
        check(walk_lib().h2omx_walk_staged(P(X), X.stride(0), n, X.shape[0], P(plan.nodes), P(plan.roots),
                                           P(plan.catbits), nt, K, plan.cap, P(f0), int(bool(average)), P(out),
                                           stream(dev)), "walk_staged")
    return out


def feature_counts(X: torch.Tensor, plan: WalkPlan, F: int, slab_trees: int | None = None) -> torch.Tensor:
    """How often feature f is tested on the paths of column r, over all trees -> fp32
    ``[F][n]``.  Work: int32 partials ``[slabs][F][n]`` when F > WALK_XLDS_MAX_F or with
    more than one slab."""
    X = _args(X, plan, "feature_counts")
    if int(F) != X.shape[0]:
        raise ValueError(f"ops.walk.feature_counts: F={F} but X has {X.shape[0]} rows")
    n, dev = X.shape[1], X.device
    cnt = torch.empty((F, n), dtype=torch.float32, device=dev)
    if n:
        slab_trees = _slabs(slab_trees, n, plan.T, dev, "feature_counts", 4 * F * n)
        slabs = -(-plan.T // slab_trees)
        part = torch.zeros((slabs, F, n), dtype=torch.int32, device=dev) if slabs > 1 or F > WALK_XLDS_MAX_F else None
        check(walk_lib().h2omx_walk_counts(P(X), X.stride(0), n, F, P(plan.nodes), P(plan.roots), P(plan.catbits),
                                           plan.T, plan.cap, slab_trees, P(part), P(cnt), stream(dev)), "walk_counts")
    return cnt
