"""ops.svm (PSVM kernels) against the np.longdouble oracle of psvm_ref, and the
public fit on the kernel route against the CPU-frame fit.

Entrywise bounds of the products: an n-term sum of three-factor products has
error at most (n + 2) u |A|^T |w| |A| with u = 2^-53 in any order of addition;
the tests allow twice that, (n + 2) 2^-52 (sum length k + 2 for tall_v)."""
import numpy as np
import pytest
import torch

import psvm_ref as R
from h2omx.frame.frame import ENUM, Frame, Vec
from h2omx.models import H2OSupportVectorMachineEstimator
from h2omx.models import psvm
from h2omx.ops import svm

pytestmark = pytest.mark.gpu
N = 1037


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _within(got, ref, mag, terms):
    err = np.abs(got.cpu().numpy().astype(R.LD) - ref)
    assert (err <= (terms + 2) * R.EPS * mag).all(), float((err / np.maximum(mag, 1e-300)).max())


@pytest.mark.parametrize("n,k,slab", [(N, k, 256) for k in (1, 5, 16, 17, 33, 64, 65, 130)] + [(1, 5, None), (67, 64, None)])
def test_wsyrk(cuda_dev, n, k, slab):
    A = _rand((n, k), k)
    w = torch.rand(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64) + 0.1
    w[::7] = 0.0
    C = svm.wsyrk(A.to(cuda_dev), w.to(cuda_dev), slab_rows=slab)
    ref, mag = R.wsyrk_ref(A.numpy(), w.numpy())
    _within(C, ref, mag, n)
    assert torch.equal(C, C.T)
    assert torch.equal(C, svm.wsyrk(A.to(cuda_dev), w.to(cuda_dev), slab_rows=slab))


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("k", [1, 17, 64, 130])
def test_thin_products(cuda_dev, k, r):
    A, s, V, T = _rand((N, k), k), _rand(N, 1), _rand((N, r), 2), _rand((k, r), 3)
    Ad, sd, Vd, Td = (t.to(cuda_dev) for t in (A, s, V, T))
    tv = svm.tall_tv(Ad, sd, Vd)
    _within(tv, *R.tall_tv_ref(A.numpy(), s.numpy(), V.numpy()), N)
    assert torch.equal(tv, svm.tall_tv(Ad, sd, Vd))
    v = svm.tall_v(Ad, sd, Td)
    _within(v, *R.tall_v_ref(A.numpy(), s.numpy(), T.numpy()), k)
    assert torch.equal(v, svm.tall_v(Ad, sd, Td))
    ones = torch.ones(N, dtype=torch.float64)
    _within(svm.tall_v(Ad, None, Td), *R.tall_v_ref(A.numpy(), ones.numpy(), T.numpy()), k)


def _icf_case(name):
    g = torch.Generator().manual_seed({"full": 2, "wide": 1, "stop": 3}[name])
    if name == "full":       # every row becomes a pivot; row 0, the first pivot, at the centre of the cube
        X = torch.rand((300, 3), generator=g, dtype=torch.float64)
        X[0] = 0.5
        return X, 12.0, 300, 1e-10
    if name == "wide":
        return torch.randn((300, 20), generator=g, dtype=torch.float64), 0.05, 17, 1e-10
    return torch.randn((40, 3), generator=g, dtype=torch.float64).repeat(3, 1), 0.5, 120, 1e-5


@pytest.mark.parametrize("name", ["full", "wide", "stop"])
def test_icf(cuda_dev, name):
    """Measured on MI355X, relative to max|H| (e_ref is today's psvm.icf on the CPU):
    see the Round 18 section of docs/ROADMAP.md."""
    X, gamma, p, thresh = _icf_case(name)
    Href, pivots, gaps, margin = R.icf_ref(X.numpy(), gamma, p, thresh)
    # the comparison of pivot sequences means something only where rounding cannot reorder them
    assert len(gaps) == len(pivots) - 1 and min(gaps) > 1e-9 and margin > 1e-9
    if name == "stop":
        assert len(pivots) == 40
    scale = float(np.abs(Href).max())
    e_ref = float(np.abs(psvm.icf(X, gamma, p, thresh).numpy() - Href).max()) / scale
    H, piv = svm.icf(X.to(cuda_dev), gamma, p, thresh, return_pivots=True)
    assert piv.tolist() == pivots
    assert H.shape == Href.shape
    err = float(np.abs(H.cpu().numpy() - Href).max()) / scale
    print(f"icf {name}: k_used {H.shape[1]} e_ref {e_ref:.3g} kernel {err:.3g}")
    assert err <= max(100 * e_ref, 64 * p * R.EPS)
    assert torch.equal(H, psvm.icf(X.to(cuda_dev), gamma, p, thresh))     # the public route, bit-identical


def _frame(n, d, device):
    g = torch.Generator().manual_seed(0)
    X = torch.randn((d, n), generator=g)
    y = ((X[:2] ** 2).sum(0) < 1.4).int()
    return Frame([Vec(f"x{j}", X[j].to(device), "real") for j in range(d)] + [Vec("y", y.to(device), ENUM, ["0", "1"])])


@pytest.mark.parametrize("d,kw", [(2, {}), (5, {"positive_weight": 2.0})])
def test_public_fit(cuda_dev, d, kw):
    fits = []
    for dev in ("cpu", cuda_dev):
        fr = _frame(1500, d, dev)
        m = H2OSupportVectorMachineEstimator(gamma=0.5, **kw).train(y="y", training_frame=fr)
        fits.append((m, m.decision_function(fr).cpu().numpy()))
    (mc, fc), (mg, fg) = fits
    assert mc.timings["icf_engine"] == "torch" and mc.timings["ipm_engine"] == "torch"
    assert mg.timings["icf_engine"] == "hip" and mg.timings["ipm_engine"] == "hip"
    assert mg.timings["icf_rank"] == mc.timings["icf_rank"]
    print(f"public fit d={d}: max |f_gpu - f_cpu| {np.abs(fg - fc).max():.3g}")
    np.testing.assert_allclose(fg, fc, atol=2e-3)
