"""ops.svm.rbf_decision (the PSVM decision function in one kernel) against an
np.longdouble oracle that takes every pair in the difference form
sum_k (x_k - s_k)^2, which has no cancellation, and the public fit through it.

Bound, inputs exact in fp64, u = 2^-53, every factor doubled:
    |f_i - ref_i| <= 2^-52 sum_j |coef_j| K_ij (nsv + 8 + 2 (d + 4) gamma (|x_i|^2 + |s_j|^2))
(the sum over nsv terms, product and exp at one ulp each, the (d + 4)-term error
of d2 relative to |x|^2 + |s|^2 carried through the exponent, and gamma d2 <=
2 gamma (|x|^2 + |s|^2) for the rounding of the argument).  Largest error /
bound measured on MI355X: see the Round 20 section of docs/ROADMAP.md."""
import numpy as np
import pytest
import torch

from psvm_ref import EPS, LD
from test_psvm_kernels_gpu import _frame
from h2omx.models import H2OSupportVectorMachineEstimator
from h2omx.models import psvm
from h2omx.ops import svm

pytestmark = pytest.mark.gpu


def _oracle(X, S, coef, gamma):
    """f and the bound, np.longdouble [n], from fp32 X [n][d], S [nsv][d] and fp64 coef."""
    X, S, coef = X.numpy().astype(LD), S.numpy().astype(LD), coef.numpy().astype(LD)
    d2 = ((X[:, None, :] - S[None, :, :]) ** 2).sum(2)
    assert float(gamma * d2.max()) < 700.0                 # no subnormal term: the relative bound means something
    T = np.abs(coef)[None, :] * np.exp(-LD(gamma) * d2)
    nrm = (X * X).sum(1)[:, None] + (S * S).sum(1)[None, :]
    bound = EPS * (T * (S.shape[0] + 8 + 2 * (X.shape[1] + 4) * LD(gamma) * nrm)).sum(1)
    return (np.sign(coef)[None, :] * T).sum(1), bound


# d = 32 is the last width with the X block resident in LDS, 33 the first that stages it per SV tile
@pytest.mark.parametrize("n,nsv,d,slab,same", [
    (1, 1, 1, None, 0), (333, 1, 1, None, 0), (67, 63, 3, None, 0), (333, 65, 1, None, 0), (67, 65, 16, None, 5),
    (1, 200, 17, None, 0), (333, 200, 17, 64, 0), (333, 200, 20, None, 0), (67, 200, 32, None, 0),
    (67, 65, 33, None, 0), (333, 63, 20, None, 5), (67, 200, 50, 128, 5)])
def test_rbf_decision(cuda_dev, n, nsv, d, slab, same):
    g = torch.Generator().manual_seed(1000 * n + 10 * nsv + d)
    X, S = torch.randn((n, d), generator=g), torch.randn((nsv, d), generator=g)
    coef = torch.randn(nsv, generator=g, dtype=torch.float64)
    if same:                      # true d2 = 0: the clamp is on the path; a few coefficients exactly 0
        X[3:3 + same] = S[7:7 + same]
        coef[[0, 8, nsv - 1]] = 0.0
    ref, bound = _oracle(X, S, coef, 1.0 / d)
    args = (X.to(cuda_dev), S.to(cuda_dev), coef.to(cuda_dev), 1.0 / d)
    f = svm.rbf_decision(*args, slab_svs=slab)
    assert f.dtype == torch.float64 and f.shape == (n,)
    ratio = np.abs(f.cpu().numpy().astype(LD) - ref) / bound
    print(f"rbf_decision n={n} nsv={nsv} d={d} slab={slab}: largest error / bound {float(ratio.max()):.3g}")
    assert (ratio <= 1).all()
    assert torch.equal(f, svm.rbf_decision(*args, slab_svs=slab))


@pytest.mark.parametrize("d", [2, 5])
def test_public_fit_scores_on_kernel(cuda_dev, d):
    fr = _frame(1500, d, cuda_dev)
    m = H2OSupportVectorMachineEstimator(gamma=0.5).train(y="y", training_frame=fr)
    assert m.timings["score_engine"] == "hip"
    X = psvm._design(fr, m.x, m.means, m.scales).float()
    ref, bound = _oracle(X.cpu(), m.sv, m.coef, m.gamma)
    ref = ref + LD(m.b)
    f = m.decision_function(fr)
    assert f.dtype == torch.float32
    err = np.abs(f.cpu().numpy().astype(LD) - ref)
    e_torch = np.abs((m._decision_torch(X) + m.b).float().cpu().numpy().astype(LD) - ref)
    print(f"public fit d={d}: nsv {m.sv.shape[0]}, max error kernel {float(err.max()):.3g}, "
          f"torch route {float(e_torch.max()):.3g}, largest error / bound "
          f"{float((err / (bound + 2.0 ** -23 * np.abs(ref))).max()):.3g}")
    assert (err <= bound + 2.0 ** -23 * np.abs(ref)).all()


def test_memory_is_linear_in_rows(cuda_dev):
    n, nsv, d = 65536, 4096, 8
    g = torch.Generator(device=cuda_dev).manual_seed(0)
    X, S = (torch.randn((r, d), generator=g, device=cuda_dev) for r in (n, nsv))
    coef = torch.randn(nsv, generator=g, dtype=torch.float64, device=cuda_dev)
    cus = torch.cuda.get_device_properties(cuda_dev).multi_processor_count
    slabs = -(-nsv // svm.rbf_slab_svs(n, nsv, d, cus))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda_dev)
    base = torch.cuda.memory_allocated(cuda_dev)
    f = svm.rbf_decision(X, S, coef, 1.0 / d)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(cuda_dev) - base
    print(f"rbf_decision {n} x {nsv}: {slabs} slab(s), peak {peak} B over the inputs")
    assert bool(torch.isfinite(f).all())
    assert peak <= 8 * n * (slabs + 2) + (4 << 20)       # one [n][nsv] fp64 plane would be 2 GiB
