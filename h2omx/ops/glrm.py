"""Python entry points of csrc/glrm_kernels.hip (masked ALS) and
csrc/glrm_loss_kernels.hip (generalized losses by proximal gradient).

Device tensors only; A [p][n] fp32 feature-major with a bool mask of the same
shape (False = missing), factors fp32, all arithmetic fp64.  Every launch goes
to the current stream.  Every result is bit-identical between two calls: no
floating-point atomics, slab partials added in slab order.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import P, _bind, check, stream

GLRM_SIGS = {
    # A, mask, Y, n, p, k, lam, X, bad_part, bad
    "h2omx_glrm_masked_x": "PPPLIIDPPPS",
    # A, mask, X, n, p, k, slab_rows, part, S
    "h2omx_glrm_masked_y_terms": "PPPLIILPPS",
    # A, mask, X, Y, codes, pars, n, p, k, gradX, obj_part, obj
    "h2omx_glrm_loss_grad_x": "PPPPPPLIIPPPS",
    # A, mask, X, Y, codes, pars, n, p, k, slab_rows, part, obj_part, gradY, obj
    "h2omx_glrm_loss_grad_y": "PPPPPPLIILPPPPS",
}

# loss name -> code of csrc/glrm_loss_kernels.hip (enum Loss)
LOSSES = {"Quadratic": 0, "Absolute": 1, "Huber": 2, "Poisson": 3, "Hinge": 4, "Logistic": 5, "Periodic": 6}
LOSS_X_BLOCK_ROWS = 64       # loss_grad_x: rows per workgroup (sizes its objective partials)

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


def y_slab_rows(n: int, p: int, k: int, cus: int, tc: int | None = None) -> int:
    """Rows per slab: enough slabs to fill the machine Y_FILL times over, capped
    so the fp64 partials [slabs][p][Tc] stay within 1 / Y_PART_SHARE of the
    bytes of A (4 n p): slabs <= n / (2 Y_PART_SHARE Tc).  Tc is the y-terms'
    k (k + 1) / 2 + k unless given (loss_grad_y: k)."""
    if tc is None:
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


def loss_columns(codes, pars, device):
    """The per-column loss codes [p] and parameters [p] (host sequences) as the
    device tensors the kernels read, refused if a code is outside LOSSES."""
    c = np.asarray(codes.cpu() if torch.is_tensor(codes) else codes)
    w = np.asarray(pars.cpu() if torch.is_tensor(pars) else pars, dtype=np.float64)
    if c.ndim != 1 or w.shape != c.shape or c.dtype.kind not in "iu":
        raise ValueError("ops.glrm.loss_columns: integer codes [p] and parameters [p]")
    if c.size and not np.isin(c, list(LOSSES.values())).all():
        raise ValueError(f"ops.glrm.loss_columns: loss codes {sorted(set(c.tolist()) - set(LOSSES.values()))} "
                         f"are not in {LOSSES}")
    return (torch.from_numpy(c.astype(np.int32)).to(device), torch.from_numpy(w.copy()).to(device))


def _loss_args(what: str, A, mask, X, Y, codes, pars):
    A, mask, X = _args(what, A, mask, X)
    (p, n), k = A.shape, X.shape[0]
    if not (torch.is_tensor(Y) and Y.is_cuda):
        raise ValueError(f"ops.glrm.{what}: device tensors only")
    if X.shape[1] != n or Y.dim() != 2 or tuple(Y.shape) != (k, p):
        raise ValueError(f"ops.glrm.{what}: X {tuple(X.shape)} and Y {tuple(Y.shape)} against A [{p}][{n}]")
    if not (torch.is_tensor(codes) and codes.is_cuda):      # host codes: checked against the table here
        codes, pars = loss_columns(codes, pars, A.device)
    if codes.dtype != torch.int32 or pars.dtype != torch.float64 or codes.shape != (p,) or pars.shape != (p,):
        raise ValueError(f"ops.glrm.{what}: int32 codes [{p}] and fp64 parameters [{p}]")
    return A, mask, X, Y.float().contiguous(), codes.contiguous(), pars.contiguous()


def loss_grad_x(A: torch.Tensor, mask: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, codes, pars):
    """``gradX [k][n]`` fp64, ``gradX[a][i] = sum_j Y[a][j] m_ji L_j'(u_ji, a_ji)`` with
    ``u = Y^T X``, and the 0-d fp64 device tensor ``sum m L``; no host synchronisation.
    ``codes`` / ``pars``: one LOSSES code and one parameter (Periodic: 2 pi / period)
    per data column, as host sequences (validated) or as the device tensors of
    :func:`loss_columns` (then an unknown code yields NaN)."""
    A, mask, X, Y, codes, pars = _loss_args("loss_grad_x", A, mask, X, Y, codes, pars)
    (p, n), k = A.shape, X.shape[0]
    dev = A.device
    grad = torch.empty((k, n), dtype=torch.float64, device=dev)
    if n == 0:
        return grad, torch.zeros((), dtype=torch.float64, device=dev)
    obj_part = torch.empty(-(-n // LOSS_X_BLOCK_ROWS), dtype=torch.float64, device=dev)
    obj = torch.empty((), dtype=torch.float64, device=dev)
    check(glrm_lib().h2omx_glrm_loss_grad_x(P(A), P(mask), P(X), P(Y), P(codes), P(pars), n, p, k, P(grad),
                                            P(obj_part), P(obj), stream(dev)), "glrm_loss_grad_x")
    return grad, obj


def loss_grad_y(A: torch.Tensor, mask: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, codes, pars,
                slab_rows: int | None = None):
    """``gradY [k][p]`` fp64, ``gradY[a][j] = sum_i X[a][i] m_ji L_j'(u_ji, a_ji)``, and the
    0-d fp64 device tensor ``sum m L``; arguments as :func:`loss_grad_x`."""
    A, mask, X, Y, codes, pars = _loss_args("loss_grad_y", A, mask, X, Y, codes, pars)
    (p, n), k = A.shape, X.shape[0]
    dev = A.device
    if n == 0:
        return torch.zeros((k, p), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    if slab_rows is None:
        slab_rows = y_slab_rows(n, p, k, torch.cuda.get_device_properties(dev).multi_processor_count, tc=k)
    if slab_rows < 1 or -(-n // slab_rows) > MAX_SLABS:
        raise ValueError(f"ops.glrm.loss_grad_y: slab_rows={slab_rows}, at least 1 and at most {MAX_SLABS} slabs")
    slabs = -(-n // slab_rows)
    part = torch.empty((slabs, p, k), dtype=torch.float64, device=dev)
    obj_part = torch.empty(slabs * -(-p // Y_COLS), dtype=torch.float64, device=dev)
    grad = torch.empty((k, p), dtype=torch.float64, device=dev)
    obj = torch.empty((), dtype=torch.float64, device=dev)
    check(glrm_lib().h2omx_glrm_loss_grad_y(P(A), P(mask), P(X), P(Y), P(codes), P(pars), n, p, k, slab_rows, P(part),
                                            P(obj_part), P(grad), P(obj), stream(dev)), "glrm_loss_grad_y")
    return grad, obj
