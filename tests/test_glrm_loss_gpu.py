"""ops.glrm.loss_grad_x / loss_grad_y against the np.longdouble oracle of glrm_loss_ref.

Bounds.  x and y are fp32 widened to fp64, so every product x_ai y_aj is exact and
u_ji, a sum of k terms (K padded with exact zeros) in any order, is within
du_ji = (k + 2) 2^-52 sum_a |x_ai y_aj| of the exact one.  To first order the derivative
g_ji = L_j'(u_ji, a_ji) moves by |L_j''| du_ji (Quadratic 2, Huber 1, Logistic 1 / 4,
Poisson exp(u), Periodic w^2, Absolute and Hinge 0 away from their kinks), and its own
evaluation adds C 2^-52 |g_ji|: dg_ji = |L''| du_ji + C 2^-52 |g_ji|.  g times a widened
fp32 factor rounds once inside the fused multiply-add of the matrix unit, so an outer sum
of T terms is within sum |factor| dg + (T + 2) 2^-52 sum |factor g| (T = p for gradX, n for
gradY, any order: slabs, waves, K steps).  The objective likewise: every L_ji is within
|g_ji| du_ji + C 2^-52 M_ji, M the sum of the magnitudes of the terms L is made of (L
itself except Poisson: exp(u) + |a u| + |a log a - a|, and Periodic: 1 + |cos|), and the sum
of the observed entries adds (count + 2) 2^-52 sum |L|.  C = 2 for the algebraic losses (a
subtraction and a product); for Poisson, Logistic and Periodic see glrm_loss_ref.C_EVAL.
A missing entry is a select, not a product: it contributes exactly 0.

Kinks.  The derivatives of Absolute and Hinge jump at u = a and s u = 1; the oracle's
smallest distance of an observed entry to a kink is asserted to be above 1e-6, nine
orders above du, and no entry is excluded."""
import numpy as np
import pytest
import torch

import glrm_loss_ref as R
from h2omx.ops import glrm

pytestmark = pytest.mark.gpu
SHAPES = [(333, 5, 1), (333, 37, 3), (333, 37, 10), (130, 130, 16), (130, 70, 17), (70, 40, 32)]
CASES = [s + (c, None) for s in SHAPES for c in range(7)] + [(333, 37, 10, "mixed", None), (333, 37, 10, "mixed", 128)]


@pytest.mark.parametrize("n,p,k,loss,slab", CASES)
def test_loss_gradients(cuda_dev, n, p, k, loss, slab):
    codes = R.MIXED if loss == "mixed" else [loss] * p
    A, mask, X, Y, pars = R.inputs(n, p, k, codes)
    ref = R.grads_ref(A, mask, X, Y, codes, pars)
    unit = R.grads_ref(A, mask, X, Y, codes, pars, C={c: 1 for c in range(7)})
    assert ref["kink"] >= 1e-6
    dev = [torch.from_numpy(t).to(cuda_dev) for t in (A, mask, X, Y)]
    gx, ox = glrm.loss_grad_x(*dev, codes, pars)
    gy, oy = glrm.loss_grad_y(*dev, codes, pars, slab_rows=slab)
    ex = np.abs(gx.cpu().numpy().astype(R.LD) - ref["gx"])
    ey = np.abs(gy.cpu().numpy().astype(R.LD) - ref["gy"])
    eo = max(abs(R.LD(float(ox)) - ref["obj"]), abs(R.LD(float(oy)) - ref["obj"]))
    worst = [float((e / np.maximum(b, 1e-300)).max()) for e, b in ((ex, unit["bx"]), (ey, unit["by"]))]
    print(f"loss {loss} {n} x {p}, k {k}: err / bound at C = 1: gradX {worst[0]:.3g} gradY {worst[1]:.3g} "
          f"objective {float(eo / unit['bobj']):.3g}, kink {ref['kink']:.3g}")
    assert (ex <= ref["bx"]).all() and (ey <= ref["by"]).all() and eo <= ref["bobj"]
    assert ox.dim() == 0 and ox.dtype == torch.float64 and ox.is_cuda
    assert not gx[:, 0].any() and not gy[:, p - 1].any()
    gx2, ox2 = glrm.loss_grad_x(*dev, codes, pars)
    gy2, oy2 = glrm.loss_grad_y(*dev, codes, pars, slab_rows=slab)
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2) and torch.equal(ox, ox2) and torch.equal(oy, oy2)


def test_refusals(cuda_dev):
    A, mask, X, Y, pars = (torch.from_numpy(t) for t in R.inputs(40, 34, 33, [0] * 34))
    codes = [0] * 34
    d = [t.to(cuda_dev) for t in (A, mask, X, Y)]
    for f in (glrm.loss_grad_x, glrm.loss_grad_y):
        with pytest.raises(ValueError, match="32"):
            f(*d, codes, pars)
        with pytest.raises(ValueError, match="device"):
            f(A, mask, X[:3], Y[:3], codes, pars)
        with pytest.raises(ValueError, match="loss codes"):
            f(d[0], d[1], d[2][:3], d[3][:3], [7] + codes[1:], pars)
        with pytest.raises(ValueError, match="against"):
            f(d[0], d[1], d[2][:3], d[3][:4], codes, pars)
