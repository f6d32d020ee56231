"""Python entry points of csrc/svm_kernels.hip (PSVM: ICF, interior-point products,
decision function).

Device tensors only, all fp64 (rbf_decision: fp32 points, fp64 coefficients and
result); every launch goes to the current stream.  Every result is
bit-identical between two calls: no floating-point atomics, slab partials added
in slab order.
"""
from __future__ import annotations

import ctypes

import torch

from . import P, _bind, check, stream

SVM_SIGS = {
    # X, xsq, n, d, p, gamma, thresh, H, diag, part_v, part_i, rec_i, rec_v, xp, hp
    "h2omx_svm_icf": "PPLIIDDPPPPPPPPS",
    # A, w, n, k, slab_rows, part, C
    "h2omx_svm_wsyrk": "PPLILPPS",
    # A, s, V, n, k, r, slab_rows, part, out
    "h2omx_svm_tall_tv": "PPPLIILPPS",
    # A, s, T, n, k, r, out
    "h2omx_svm_tall_v": "PPPLIIPS",
    # X, S, coef, n, nsv, d, gamma, slab_svs, xsq, ssq, part, out
    "h2omx_svm_rbf_decision": "PPPLLIDLPPPPS",
}

# limits of the ICF kernels (LDS stage of the pivot row: 8 KB of x, 32 KB of H)
ICF_MAX_P = 4096
ICF_MAX_D = 1024
ICF_MIN_BLOCK_ROWS = 64      # 4 units of 64 lanes, 16 rows each
MAX_RHS = 4
WSYRK_BLOCK = 64
# wsyrk: (blocks x slabs) fills the compute units this many times over ...
WSYRK_FILL = 4
# ... unless the slab partials would pass 1 / 8 of the n k doubles of A
WSYRK_PART_SHARE = 8
TALL_TV_BLOCKS = 2048
RBF_BLOCK = 64               # scored rows of a workgroup, SVs of a tile
# rbf_decision: (row blocks x slabs) fills the compute units this many times over ...
RBF_FILL = 4
# ... unless the slab partials would pass the bytes of X, S and coef
RBF_PART_SHARE = 1
MAX_SLABS = 65535


def svm_lib() -> ctypes.CDLL:
    return _bind("svm", SVM_SIGS)


def _f64(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"ops.svm.{what}: device tensors only")
    return t.to(torch.float64).contiguous()


def _empty(shape, dev, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device=dev)


def icf(X: torch.Tensor, gamma: float, p: int, thresh: float, return_pivots: bool = False):
    """Pivoted incomplete Cholesky of the Gaussian kernel over the rows of X
    [n][d] -> H [n][k_used], K ~ H H^T.  The pivot is the largest residual
    diagonal, the lowest row index among equals; the factorisation stops at the
    first pivot below ``thresh``.  One host read, after the last launch.
    ``return_pivots``: also the pivot row of every column, int64 [k_used]."""
    X = _f64(X, "icf")
    n, d = X.shape
    if n < 1 or not 1 <= d <= ICF_MAX_D or not 1 <= p <= ICF_MAX_P:
        raise ValueError(f"ops.svm.icf: n={n} d={d} p={p}, the kernels take n >= 1, d 1..{ICF_MAX_D}, "
                         f"p 1..{ICF_MAX_P}")
    dev = X.device
    lib = svm_lib()
    H = _empty((n, p), dev)
    xsq = (X * X).sum(1)
    diag = _empty(n, dev)
    nparts = -(-n // ICF_MIN_BLOCK_ROWS)
    part_v, part_i = _empty(nparts, dev), _empty(nparts, dev, torch.int64)
    rec_i, rec_v = _empty(3 + p, dev, torch.int64), _empty(2, dev)
    xp, hp = _empty(d, dev), _empty(p, dev)
    check(lib.h2omx_svm_icf(P(X), P(xsq), n, d, p, float(gamma), float(thresh), P(H), P(diag), P(part_v), P(part_i),
                            P(rec_i), P(rec_v), P(xp), P(hp), stream(dev)), "svm_icf")
    k_used = int(rec_i[2])
    H = H[:, :k_used].contiguous()
    return (H, rec_i[3:3 + k_used]) if return_pivots else H


def wsyrk_slab_rows(n: int, k: int, cus: int) -> int:
    """Rows per slab: enough slabs to fill the machine WSYRK_FILL times over,
    capped so the partials stay within 1 / WSYRK_PART_SHARE of n k doubles."""
    nbc = -(-k // WSYRK_BLOCK)
    pairs = nbc * (nbc + 1) // 2
    slabs = -(-WSYRK_FILL * cus // pairs)
    cap = (n * k // WSYRK_PART_SHARE) // (pairs * WSYRK_BLOCK * WSYRK_BLOCK)
    slabs = max(1, min(slabs, cap, -(-n // 16), MAX_SLABS))
    return -(-(-(-n // slabs)) // 16) * 16


def wsyrk(A: torch.Tensor, w: torch.Tensor, slab_rows: int | None = None) -> torch.Tensor:
    """``A^T diag(w) A`` [k][k] on the fp64 matrix units, exactly symmetric."""
    A, w = _f64(A, "wsyrk"), _f64(w, "wsyrk")
    n, k = A.shape
    dev = A.device
    if k < 1 or w.shape != (n,):
        raise ValueError("ops.svm.wsyrk: A [n][k] with k >= 1 and w [n]")
    if n == 0:
        return torch.zeros((k, k), dtype=torch.float64, device=dev)
    if slab_rows is None:
        slab_rows = wsyrk_slab_rows(n, k, torch.cuda.get_device_properties(dev).multi_processor_count)
    slabs = -(-n // slab_rows)
    nbc = -(-k // WSYRK_BLOCK)
    part = _empty((slabs, nbc * (nbc + 1) // 2, WSYRK_BLOCK * WSYRK_BLOCK), dev)
    C = _empty((k, k), dev)
    check(svm_lib().h2omx_svm_wsyrk(P(A), P(w), n, k, slab_rows, P(part), P(C), stream(dev)), "svm_wsyrk")
    return C


def tall_tv(A: torch.Tensor, s: torch.Tensor | None, V: torch.Tensor) -> torch.Tensor:
    """``A^T diag(s) V`` [k][r] for V [n][r], r <= 4 (``s`` None: ones)."""
    A, V = _f64(A, "tall_tv"), _f64(V, "tall_tv")
    s = None if s is None else _f64(s, "tall_tv")
    n, k = A.shape
    r = V.shape[1]
    dev = A.device
    if k < 1 or not 1 <= r <= MAX_RHS or V.shape[0] != n:
        raise ValueError(f"ops.svm.tall_tv: A [n][k], V [n][r] with r 1..{MAX_RHS}")
    if n == 0:
        return torch.zeros((k, r), dtype=torch.float64, device=dev)
    col_tiles = -(-k // 64)
    slabs = max(1, min(-(-TALL_TV_BLOCKS // col_tiles), -(-n // 256), MAX_SLABS))
    slab_rows = -(-n // slabs)
    slabs = -(-n // slab_rows)
    part = _empty((slabs, k, r), dev)
    out = _empty((k, r), dev)
    check(svm_lib().h2omx_svm_tall_tv(P(A), P(s), P(V), n, k, r, slab_rows, P(part), P(out), stream(dev)),
          "svm_tall_tv")
    return out


def tall_v(A: torch.Tensor, s: torch.Tensor | None, T: torch.Tensor) -> torch.Tensor:
    """``diag(s) A T`` [n][r] for T [k][r], r <= 4 (``s`` None: ones)."""
    A, T = _f64(A, "tall_v"), _f64(T, "tall_v")
    s = None if s is None else _f64(s, "tall_v")
    n, k = A.shape
    r = T.shape[1]
    dev = A.device
    if k < 1 or not 1 <= r <= MAX_RHS or T.shape[0] != k:
        raise ValueError(f"ops.svm.tall_v: A [n][k], T [k][r] with r 1..{MAX_RHS}")
    out = _empty((n, r), dev)
    if n == 0:
        return out
    check(svm_lib().h2omx_svm_tall_v(P(A), P(s), P(T), n, k, r, P(out), stream(dev)), "svm_tall_v")
    return out


def rbf_slab_svs(n: int, nsv: int, d: int, cus: int) -> int:
    """Support vectors per slab, a multiple of 64: enough slabs for row blocks
    x slabs to fill the machine RBF_FILL times over, capped so the [slab][n]
    fp64 partials stay within 1 / RBF_PART_SHARE of the bytes of X, S and coef."""
    blocks = -(-n // RBF_BLOCK)
    slabs = -(-RBF_FILL * cus // blocks)
    cap = (4 * (n + nsv) * d + 8 * nsv) // RBF_PART_SHARE // (8 * n)
    slabs = max(1, min(slabs, cap, -(-nsv // RBF_BLOCK), MAX_SLABS))
    return -(-(-(-nsv // slabs)) // RBF_BLOCK) * RBF_BLOCK


def rbf_decision(X: torch.Tensor, S: torch.Tensor, coef: torch.Tensor, gamma: float,
                 slab_svs: int | None = None) -> torch.Tensor:
    """``f_i = sum_j coef_j exp(-gamma |x_i - s_j|^2)`` -> fp64 [n] for fp32 points
    X [n][d] and S [nsv][d] and fp64 coef [nsv]: the cross term on the fp64
    matrix units, exp and the sum over j in registers.  No [n][nsv] tensor
    exists; the memory beyond the result is the row norms (n + nsv doubles) and
    the [slabs][n] partials."""
    if not (X.is_cuda and S.is_cuda and coef.is_cuda):
        raise ValueError("ops.svm.rbf_decision: device tensors only")
    if X.dim() != 2 or S.dim() != 2 or X.shape[1] < 1 or S.shape[1] != X.shape[1] or coef.shape != (S.shape[0],):
        raise ValueError("ops.svm.rbf_decision: X [n][d], S [nsv][d] with d >= 1 and coef [nsv]")
    n, d = X.shape
    nsv = S.shape[0]
    if nsv < 1 or not gamma > 0:
        raise ValueError(f"ops.svm.rbf_decision: nsv={nsv} gamma={gamma}, the kernel takes nsv >= 1 and gamma > 0")
    X, S = X.to(torch.float32).contiguous(), S.to(torch.float32).contiguous()
    coef = coef.to(torch.float64).contiguous()
    dev = X.device
    out = _empty(n, dev)
    if n == 0:
        return out
    if slab_svs is None:
        slab_svs = rbf_slab_svs(n, nsv, d, torch.cuda.get_device_properties(dev).multi_processor_count)
    slabs = -(-nsv // slab_svs)
    xsq, ssq = _empty(n, dev), _empty(nsv, dev)
    part = _empty((slabs, n), dev) if slabs > 1 else None
    check(svm_lib().h2omx_svm_rbf_decision(P(X), P(S), P(coef), n, nsv, d, float(gamma), slab_svs, P(xsq), P(ssq),
                                           P(part), P(out), stream(dev)), "svm_rbf_decision")
    return out
