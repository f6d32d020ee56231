"""Python entry points of csrc/cox_kernels.hip (CoxPH Newton pass, concordance).

Device tensors only; every launch goes to the current stream.  The plan of a
fit (:func:`cox_prepare`) is torch plumbing and runs once; a Newton pass
(:func:`cox_newton_pass`) is kernels only and holds O(n p) memory.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import P, _bind, check, stream

SURVIVAL_SIGS = {
    # X, n, p, unit_rows, perm, key, beta, w, ev, eta, r, B1, A1, sc, nb, rec_key, rec
    "h2omx_cox_row_sums": "PLIIPPPPPPPPPPLPPS",
    # B1, sc, Bp1, Bp0, A1, sstart, send, nb, p, chunk, efron, gw, work, S1, scal, ll, grad
    "h2omx_cox_bucket_stage": "PPPPPPPLIIIPPPPPPS",
    # r, ev, b, bp, scal, nb, n, omega
    "h2omx_cox_row_weight": "PPPPPLLPS",
    # Y, Z, omega, n, p, slab_rows, part, C
    "h2omx_cox_wxty": "PPPLILPPS",
    # te, lpe, ne, t, lp, n, ysplit, part, counts
    "h2omx_cox_concordance": "PPLPPLIPPS",
}

MAX_P = 64
# rows per unit of the row pass (two carry records per unit)
ROW_UNIT = 256
# buckets per workgroup of the bucket scans: small tables still span several
# chunks, large ones keep the single-workgroup offset pass short
SCAN_CHUNK_SMALL, SCAN_CHUNK_LARGE, SCAN_LARGE_FROM = 256, 1024, 1 << 16
WXTY_MAX_SLABS = 1024


def survival_lib() -> ctypes.CDLL:
    return _bind("survival", SURVIVAL_SIGS)


@dataclass
class CoxPlan:
    """Rows sorted by (stratum, stop descending) and their bucket indices."""
    Xs: torch.Tensor            # [n][p] fp64, centred
    w: torch.Tensor             # [n]
    ev: torch.Tensor            # [n] 1.0 for an event row
    b: torch.Tensor             # [n] int32, non-decreasing
    bp: torch.Tensor | None     # [n] int32 (start times)
    perm: torch.Tensor | None   # [n] int32: rows in order of bp
    bp_sorted: torch.Tensor | None
    sstart: torch.Tensor        # [nb] int32 first bucket of the bucket's stratum
    send: torch.Tensor          # [nb] int32 last bucket (the one without events)
    gw: torch.Tensor            # [p] sum over the event rows of w x
    nb: int


def _first_bucket_at_or_below(bkey, s, rank, R):
    # buckets are ordered by (stratum, time descending): count those before (s, time rank)
    return torch.searchsorted(bkey, s * (R + 1) + (R - rank), right=False)


def cox_prepare(t, start, d, w, strata, Xc) -> CoxPlan:
    """Sort once per fit and number the distinct event times of every stratum."""
    if not Xc.is_cuda:
        raise ValueError("ops.survival.cox_prepare: device tensors only")
    n, p = Xc.shape
    if not 1 <= p <= MAX_P:
        raise ValueError(f"ops.survival: {p} design columns, the kernels take 1..{MAX_P}")
    s = torch.unique(strata, return_inverse=True)[1]
    o = torch.argsort(t, descending=True, stable=True)
    o = o[torch.argsort(s[o], stable=True)]
    t, s, w, Xs = t[o], s[o], w[o].contiguous(), Xc[o].contiguous()
    ev = (d[o] > 0)
    ns = int(s[-1]) + 1
    times = torch.cat([t, start[o]]) if start is not None else t
    rank = torch.unique(times, return_inverse=True)[1]
    R = int(rank.max())
    # distinct (stratum, event time) pairs in sorted order
    es, er = s[ev], rank[:n][ev]
    new = torch.ones_like(es, dtype=torch.bool)
    new[1:] = (es[1:] != es[:-1]) | (er[1:] != er[:-1])
    bs, br = es[new], er[new]
    bkey = bs * (R + 1) + (R - br)
    # + s: every stratum before this one has one closing bucket without events
    b = _first_bucket_at_or_below(bkey, s, rank[:n], R) + s
    nreal = torch.bincount(bs, minlength=ns)
    send_s = torch.cumsum(nreal, 0) + torch.arange(ns, device=s.device)
    sstart_s = send_s - nreal
    nb = int(send_s[-1]) + 1
    per = nreal + 1
    plan = CoxPlan(Xs=Xs, w=w, ev=ev.double(), b=b.int(), bp=None, perm=None, bp_sorted=None,
                   sstart=torch.repeat_interleave(sstart_s, per).int(),
                   send=torch.repeat_interleave(send_s, per).int(),
                   gw=(w[ev][:, None] * Xs[ev]).sum(0), nb=nb)
    if start is not None:
        bp = _first_bucket_at_or_below(bkey, s, rank[n:], R) + s
        q = torch.argsort(bp, stable=True)
        plan.bp, plan.perm, plan.bp_sorted = bp.int(), q.int(), bp[q].int()
    return plan


def _zeros(shape, dev):
    return torch.zeros(shape, dtype=torch.float64, device=dev)


def _row_sums(lib, plan, perm, key, beta, eta, r, main):
    dev = plan.Xs.device
    n, p = plan.Xs.shape
    units = -(-n // ROW_UNIT)
    B1 = _zeros((plan.nb, p), dev)
    A1 = _zeros((plan.nb, p), dev) if main else None
    sc = _zeros((5 if main else 1, plan.nb), dev)
    rec_key = torch.empty(2 * units, dtype=torch.int32, device=dev)
    rec = torch.empty((2 * units, 2 * p + 5), dtype=torch.float64, device=dev)
    check(lib.h2omx_cox_row_sums(P(plan.Xs), n, p, ROW_UNIT, P(perm), P(key), P(beta), P(plan.w), P(plan.ev),
                                 P(eta), P(r), P(B1), P(A1), P(sc), plan.nb, P(rec_key), P(rec), stream(dev)),
          "cox_row_sums")
    return B1, A1, sc


def wxty(Y, Z, omega):
    """``sum_i omega_i y_i z_i^T`` in fp64 on the matrix units (``Y is Z``: symmetric)."""
    lib = survival_lib()
    n, p = Y.shape
    dev = Y.device
    slab = max(64, -(-n // (16 * WXTY_MAX_SLABS)) * 16)   # rows per slab, a multiple of 16
    slabs = -(-n // slab)
    T = -(-p // 16)
    tiles = T * (T + 1) // 2 if Y is Z else T * T
    part = torch.empty((slabs, tiles, 256), dtype=torch.float64, device=dev)
    C = torch.empty((p, p), dtype=torch.float64, device=dev)
    check(lib.h2omx_cox_wxty(P(Y), P(Y if Y is Z else Z), P(omega), n, p, slab, P(part), P(C), stream(dev)),
          "cox_wxty")
    return C


def cox_newton_pass(plan: CoxPlan, beta: torch.Tensor, efron: bool):
    """Partial log-likelihood, gradient and Hessian at ``beta`` (fp64 device tensors)."""
    lib = survival_lib()
    dev = plan.Xs.device
    n, p = plan.Xs.shape
    nb = plan.nb
    beta = beta.to(dev, torch.float64).contiguous()
    eta = torch.empty(n, dtype=torch.float64, device=dev)
    r = torch.empty(n, dtype=torch.float64, device=dev)
    B1, A1, sc = _row_sums(lib, plan, None, plan.b, beta, eta, r, True)
    Bp1 = Bp0 = None
    if plan.bp is not None:
        Bp1, _, Bp0 = _row_sums(lib, plan, plan.perm, plan.bp_sorted, beta, eta, r, False)
    chunk = SCAN_CHUNK_LARGE if nb >= SCAN_LARGE_FROM else SCAN_CHUNK_SMALL
    chunks = -(-nb // chunk)
    work = torch.empty(chunks * (3 * (p + 1) + 3), dtype=torch.float64, device=dev)
    S1 = torch.empty((nb, p), dtype=torch.float64, device=dev)
    scal = torch.empty((7, nb), dtype=torch.float64, device=dev)
    ll = torch.empty(1, dtype=torch.float64, device=dev)
    grad = torch.empty(p, dtype=torch.float64, device=dev)
    check(lib.h2omx_cox_bucket_stage(P(B1), P(sc), P(Bp1), P(Bp0), P(A1), P(plan.sstart), P(plan.send), nb, p,
                                     chunk, int(efron), P(plan.gw), P(work), P(S1), P(scal), P(ll), P(grad),
                                     stream(dev)), "cox_bucket_stage")
    omega = torch.empty(n, dtype=torch.float64, device=dev)
    check(lib.h2omx_cox_row_weight(P(r), P(plan.ev), P(plan.b), P(plan.bp), P(scal), nb, n, P(omega), stream(dev)),
          "cox_row_weight")
    cross = wxty(S1, A1, -scal[4])
    neg_hess = wxty(plan.Xs, plan.Xs, omega) - (wxty(S1, S1, scal[3]) + wxty(A1, A1, scal[5]) + cross + cross.T)
    return ll[0], grad, -neg_hess


def concordance(t, d, lp) -> float:
    """Harrell's C, the pair counts of ``models.coxph.concordance`` in 64-bit integers."""
    if not t.is_cuda:
        raise ValueError("ops.survival.concordance: device tensors only")
    lib = survival_lib()
    dev = t.device
    t = t.double().contiguous()
    lp = lp.double().contiguous()
    e = torch.nonzero(d > 0).flatten()
    ne, n = e.numel(), t.numel()
    if ne == 0 or n == 0:
        return float("nan")
    te, lpe = t[e].contiguous(), lp[e].contiguous()
    eb = -(-ne // 256)
    ysplit = max(1, min(-(-n // 256), -(-4096 // eb)))
    part = torch.empty((ysplit * eb, 3), dtype=torch.int64, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    check(lib.h2omx_cox_concordance(P(te), P(lpe), ne, P(t), P(lp), n, ysplit, P(part), P(counts), stream(dev)),
          "cox_concordance")
    gt, eq, tot = counts.tolist()
    return (gt + 0.5 * eq) / tot if tot > 0 else float("nan")
