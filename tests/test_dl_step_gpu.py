"""One fp32 DeepLearning training step on the GPU against autograd.

The reference is the same update computed by torch autograd in float64 on the
CPU (forward, softmax cross-entropy / squared loss averaged over the batch,
backward) followed by H2O's ADADELTA (``reference/dense.py adadelta_``).
The reference (``tests/dlref.py``) is whole-step autograd, which is only
valid while no Rectifier pre-activation sits within fp32 rounding of zero, so
the batches here are small (M <= 256).  At these sizes both GPU paths of
``models/deeplearning._DLTrainer`` are pinned:

* the fused small-batch chain (``ops/mlp.py`` / ``csrc/mlp_kernels.hip``:
  forward, loss gradient, backward and ADADELTA in 2 L - 1 launches);
* the per-op path (GEMM kernels, fused activation backward, the bias /
  output-layer gradient folds inside the ADADELTA kernel); with M <= 256
  ``ops/dense.py`` routes every product to the small-batch kernels (split-K
  ``gemm``, ``act_backward_bias``).

The large-batch routes that ``bench.py --model dl-mlp`` runs (x3 forward and
data-gradient GEMMs, ``gemm_dact``, ``gemm_wgrad_bias``, the bf16 step at
split-K 8) are pinned stage by stage in ``tests/test_dl_large_step_gpu.py``.

Gradients, updated weights and both ADADELTA accumulators must match at
rtol 1e-4 (fp32 MFMA accumulation vs float64)."""
import numpy as np
import pytest
import torch

from dlref import close as _close, reference as _reference

pytestmark = pytest.mark.gpu

CASES = [
    # sizes, act (1 relu, 2 tanh), M, regression, l2
    ([200, 512, 512, 512, 512, 2], 1, 256, False, 0.0),     # estimator-default shape of the DL bench
    ([37, 48, 40, 3], 2, 50, False, 1e-4),                  # ragged dims, tanh, 3 classes, L2
    ([21, 64, 1], 1, 100, True, 0.0),                       # one hidden layer (ADADELTA tail launch), regression
    ([16, 32, 32, 8], 1, 7, False, 0.0),                    # 8 classes, a batch smaller than one MFMA block
]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_one_training_step_matches_autograd(case, fused, monkeypatch):
    from h2omx.models.deeplearning import H2ODeepLearningEstimator, _DLTrainer, _Net

    sizes, act, M, regression, l2 = CASES[case]
    monkeypatch.setattr(_DLTrainer, "FUSED", fused)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(case)
    X = rng.normal(size=(M * 3, sizes[0])).astype(np.float32)
    y = (rng.normal(size=M * 3).astype(np.float32) if regression
         else rng.integers(0, sizes[-1], size=M * 3).astype(np.int32))
    gen = torch.Generator().manual_seed(case)
    net = _Net(sizes, act, dev, gen)
    p = dict(H2ODeepLearningEstimator.DEFAULTS)
    p.update(l2=l2, loss="Automatic")
    Xd = torch.from_numpy(X).to(dev)
    Yd = torch.from_numpy(y).to(dev)
    tr = _DLTrainer(p, net, Xd, Yd, act, not regression, False, 0.0, [0.0] * 8, M, 3, None,
                    torch.Generator().manual_seed(1), None, len(sizes) - 2, backward=H2ODeepLearningEstimator._backward)
    assert (tr.fused is not None) == fused
    # non-trivial ADADELTA state (as after a few steps)
    P = net.flat.numel()
    Eg2_0 = (rng.random(P) * 1e-4).astype(np.float32)
    Edx2_0 = (rng.random(P) * 1e-6).astype(np.float32)
    tr.Eg2.copy_(torch.from_numpy(Eg2_0))
    tr.Edx2.copy_(torch.from_numpy(Edx2_0))
    W0 = net.flat.cpu().numpy().copy()
    idx = torch.arange(M, 2 * M, device=dev)
    tr._body(idx)
    torch.cuda.synchronize()
    G, Wn, E1, E2 = _reference(sizes, act, W0, X[M:2 * M], y[M:2 * M], regression, float(p["rho"]),
                               float(p["epsilon"]), l2, Eg2_0, Edx2_0, net.layers)
    _close("grad", net.grad.cpu().numpy(), G)
    _close("weights", net.flat.cpu().numpy(), Wn)
    _close("Eg2", tr.Eg2.cpu().numpy(), E1)
    _close("Edx2", tr.Edx2.cpu().numpy(), E2)


def test_two_fused_steps_on_different_batch_tensors_match_autograd():
    """The second call of FusedMlpStep._set_batch re-points F_0's A operand and the dW_0
    job of Q_0 at a new batch tensor: a stale pointer in either would train on the first
    batch again.  Two steps on two live tensors against two reference steps."""
    from h2omx.models.deeplearning import H2ODeepLearningEstimator, _DLTrainer, _Net

    sizes, act, M, l2 = [37, 48, 40, 3], 2, 50, 1e-4
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    Xs = [rng.normal(size=(M, sizes[0])).astype(np.float32) for _ in range(2)]
    ys = [rng.integers(0, sizes[-1], size=M).astype(np.int32) for _ in range(2)]
    net = _Net(sizes, act, dev, torch.Generator().manual_seed(7))
    p = dict(H2ODeepLearningEstimator.DEFAULTS)
    p.update(l2=l2, loss="Automatic")
    Xd = [torch.from_numpy(x).to(dev) for x in Xs]      # two live tensors: two different pointers
    Yd = [torch.from_numpy(y).to(dev) for y in ys]
    assert Xd[0].data_ptr() != Xd[1].data_ptr() and Yd[0].data_ptr() != Yd[1].data_ptr()
    tr = _DLTrainer(p, net, Xd[0], Yd[0], act, True, False, 0.0, [0.0] * 8, M, 1, None,
                    torch.Generator().manual_seed(1), None, len(sizes) - 2, backward=H2ODeepLearningEstimator._backward)
    assert tr.fused is not None
    P = net.flat.numel()
    E1 = (rng.random(P) * 1e-4).astype(np.float32)
    E2 = (rng.random(P) * 1e-6).astype(np.float32)
    tr.Eg2.copy_(torch.from_numpy(E1))
    tr.Edx2.copy_(torch.from_numpy(E2))
    W = net.flat.cpu().numpy().copy()
    for k in range(2):
        tr._body(None, xb=Xd[k], yb=Yd[k])
        G, W, E1, E2 = _reference(sizes, act, W, Xs[k], ys[k], False, float(p["rho"]), float(p["epsilon"]), l2,
                                  E1, E2, net.layers)
    torch.cuda.synchronize()
    _close("grad", net.grad.cpu().numpy(), G)
    _close("weights", net.flat.cpu().numpy(), W)
    _close("Eg2", tr.Eg2.cpu().numpy(), E1)
    _close("Edx2", tr.Edx2.cpu().numpy(), E2)


def test_fused_chain_is_the_estimator_default_path():
    """The estimator's defaults (Rectifier, ADADELTA, 256-row batches) train on the
    fused chain: 2 L - 1 launches per update (L = 3 layers here)."""
    from h2omx.frame import Frame
    from h2omx.models import H2ODeepLearningEstimator
    from h2omx.frame.synthetic import higgs_like

    dev = torch.device("cuda", 0)
    X, y = higgs_like(40000, seed=3, device=dev)
    fr = Frame.from_tensor(X.contiguous(), y=y, y_categorical=True)
    est = H2ODeepLearningEstimator(hidden=[64, 64], epochs=1, seed=1)
    m = est.train(y="response", training_frame=fr)
    tr = getattr(est, "_last_trainer", None)
    assert tr is not None and tr.fused is not None and tr.fused.launches == 5
    assert m.training_metrics["AUC"] > 0.7
