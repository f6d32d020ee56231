"""Python entry points of csrc/glrm_kernels.hip (GLRM with missing entries).

Device tensors only; A [p][n] fp32 feature-major with a bool mask of the same
shape (False = missing), factors fp32, all arithmetic fp64.  Every launch goes
to the current stream.  Every result is bit-identical between two calls: no
floating-point atomics, slab partials added in slab order.
"""
from __future__ import annotations

import ctypes

import torch

from . import P, _bind, check, stream

GLRM_SIGS = {
    # A, mask, Y, n, p, k, lam, X, bad_part, bad
    "h2omx_glrm_masked_x": "PPPLIIDPPPS",
    # A, mask, X, n, p, k, slab_rows, part, S
    "h2omx_glrm_masked_y_terms": "PPPLIILPPS",
}

MAX_K = 32                   # rank: a row's system is solved by a unit of at most 32 lanes
X_MIN_BLOCK_ROWS = 16        # smallest row block of the x-step (sizes its work array)
Y_COLS = 16                  # y-terms: data columns per workgroup
Y_STAGE_ROWS = 32            # y-terms: rows per LDS stage; slabs are whole stages
# y-terms: (column tiles x slabs) fills the compute units this many times over ...
Y_FILL = 4
# ... unless the fp64 slab partials would pass 1 / 4 of the bytes of the n p floats of A
Y_PART_SHARE = 4
MAX_SLABS = 65535


def glrm_lib() -> ctypes.CDLL:
    return _bind("glrm", GLRM_SIGS)


def _args(what: str, A: torch.Tensor, mask: torch.Tensor, F: torch.Tensor):
    """A, mask and the factor F [k][p or n] as the kernels read them."""
    if not (A.is_cuda and mask.is_cuda and F.is_cuda):
        raise ValueError(f"ops.glrm.{what}: device tensors only")
    if A.dim() != 2 or mask.shape != A.shape or mask.dtype != torch.bool or F.dim() != 2:
        raise ValueError(f"ops.glrm.{what}: A [p][n] with a bool mask of the same shape and a factor [k][.]")
    k = F.shape[0]
    if not 1 <= k <= MAX_K:
        raise ValueError(f"ops.glrm.{what}: k={k}, the kernels take k 1..{MAX_K}")
    if A.shape[0] < 1:
        raise ValueError(f"ops.glrm.{what}: p >= 1")
    return A.float().contiguous(), mask.contiguous(), F.float().contiguous()


def masked_x(A: torch.Tensor, mask: torch.Tensor, Y: torch.Tensor, lam: float):
    """X [k][n] fp32, ``x_i = (sum_j m_ji y_j y_j^T + lam I)^-1 sum_j a_ji y_j`` for
    every row, and the number of rows whose Cholesky factorisation met a pivot
    that was not positive and finite (their x is then meaningless).  A row with
    no observed entry gets exactly 0."""
    A, mask, Y = _args("masked_x", A, mask, Y)
    (p, n), k = A.shape, Y.shape[0]
    if Y.shape[1] != p:
        raise ValueError(f"ops.glrm.masked_x: Y {tuple(Y.shape)} against A [{p}][{n}]")
    dev = A.device
    X = torch.empty((k, n), dtype=torch.float32, device=dev)
    if n == 0:
        return X, 0
    bad_part = torch.empty(-(-n // X_MIN_BLOCK_ROWS), dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    check(glrm_lib().h2omx_glrm_masked_x(P(A), P(mask), P(Y), n, p, k, float(lam), P(X), P(bad_part), P(bad),
                                         stream(dev)), "glrm_masked_x")
    return X, int(bad)


def y_slab_rows(n: int, p: int, k: int, cus: int) -> int:
    """Rows per slab: enough slabs to fill the machine Y_FILL times over, capped
    so the fp64 partials [slabs][p][Tc] stay within 1 / Y_PART_SHARE of the
    bytes of A (4 n p): slabs <= n / (2 Y_PART_SHARE Tc)."""
    tc = k * (k + 1) // 2 + k
    slabs = -(-Y_FILL * cus // -(-p // Y_COLS))
    cap = n // (2 * Y_PART_SHARE * tc)
    slabs = max(1, min(slabs, cap, -(-n // Y_STAGE_ROWS), MAX_SLABS))
    return -(-(-(-n // slabs)) // Y_STAGE_ROWS) * Y_STAGE_ROWS


def masked_y_terms(A: torch.Tensor, mask: torch.Tensor, X: torch.Tensor, slab_rows: int | None = None) -> torch.Tensor:
    """S [p][k][k + 1] fp64, ``S[j] = [sum_i m_ji x_i x_i^T | sum_i a_ji x_i]``,
    every ``S[j][:, :k]`` exactly symmetric; no ridge term."""
    A, mask, X = _args("masked_y_terms", A, mask, X)
    (p, n), k = A.shape, X.shape[0]
    if X.shape[1] != n:
        raise ValueError(f"ops.glrm.masked_y_terms: X {tuple(X.shape)} against A [{p}][{n}]")
    dev = A.device
    if n == 0:
        return torch.zeros((p, k, k + 1), dtype=torch.float64, device=dev)
    if slab_rows is None:
        slab_rows = y_slab_rows(n, p, k, torch.cuda.get_device_properties(dev).multi_processor_count)
    if slab_rows < 1 or -(-n // slab_rows) > MAX_SLABS:
        raise ValueError(f"ops.glrm.masked_y_terms: slab_rows={slab_rows}, at least 1 and at most {MAX_SLABS} slabs")
    slabs = -(-n // slab_rows)
    part = torch.empty((slabs, p, k * (k + 1) // 2 + k), dtype=torch.float64, device=dev)
    S = torch.empty((p, k, k + 1), dtype=torch.float64, device=dev)
    check(glrm_lib().h2omx_glrm_masked_y_terms(P(A), P(mask), P(X), n, p, k, slab_rows, P(part), P(S), stream(dev)),
          "glrm_masked_y_terms")
    return S
