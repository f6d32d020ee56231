"""The large-batch DeepLearning step on the GPU, verified stage by stage.

``tests/test_dl_step_gpu.py`` compares whole updates with float64 autograd at
M <= 256, where ``ops/dense.py`` routes every product to the small-batch
kernels.  Here the batches are the size at which the routes of
``bench.py --model dl-mlp`` are taken (x3 forward GEMM, ``transpose_weights``
+ ``gemm_x3_dact``, fp32 ``gemm_dact``, ``gemm_wgrad_bias`` with the bias
slices riding on the split-K reduce, ``out_backward`` / ``out_wgrad`` +
``thin_dact``, ``adadelta_fix`` with its deferred folds, the bf16 step at
split-K 8), and every stage is checked from the stage's own device inputs
against float64 with the derived single-GEMM bound of ``tests/dlref.py``.

Intermediate tensors are recorded by wrapping the Python entry points
(``_forward``, ``_dgrad``, ``out_backward``, the softmax gradient); route
witnesses count the native entry points, and every case asserts that the ones
it names ran - a shape that silently falls back to another kernel fails."""
import numpy as np
import pytest
import torch

import dlref as DR

pytestmark = pytest.mark.gpu

RHO, EPS = 0.99, 1e-8

DENSE_NAMES = ("h2omx_gemm", "h2omx_gemm_skinny_nt", "h2omx_gemm_skinny_softmax", "h2omx_softmax_xent",
               "h2omx_out_backward", "h2omx_out_wgrad", "h2omx_out_wgrad_partial", "h2omx_thin_dact",
               "h2omx_gemm_dact", "h2omx_act_backward_bias", "h2omx_act_backward", "h2omx_gemm_wgrad_bias",
               "h2omx_bias_grad", "h2omx_slab_sum_f32", "h2omx_adadelta", "h2omx_adadelta_fix", "h2omx_gemm_bf16",
               "h2omx_cvt_bf16", "h2omx_cvt_bf16_multi", "h2omx_softmax_xent_bf16")
MLP_NAMES = ("h2omx_gemm_x3", "h2omx_gemm_x3_dact", "h2omx_x3_transpose", "h2omx_mlp_phase", "h2omx_mlp_out")


class _Calls:
    """route witnesses: the argument tuples of every native launch, by entry point"""

    def __init__(self, monkeypatch):
        from h2omx import ops
        from h2omx.ops import mlp as OM

        self.args = {}
        for lib, names in ((ops.dense_lib(), DENSE_NAMES), (OM.lib(), MLP_NAMES)):
            for name in names:
                monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))

    def _wrap(self, name, fn):
        def call(*a):
            self.args.setdefault(name, []).append(a)
            return fn(*a)
        return call

    def take(self):
        out, self.args = self.args, {}
        return out


def _counts(args):
    return {k: len(v) for k, v in sorted(args.items())}


class _Tensors:
    """the intermediate tensors of one fp32 step (references kept, so nothing is reused)"""

    def __init__(self, monkeypatch):
        import h2omx.models.deeplearning as DL
        from h2omx.ops import dense as OD

        self.Hs = self.Z = self.dZ_out = None
        self.dgrad = {}      # layer i -> (dZ_i, dZ_{i-1}, bias slices of dZ_{i-1})
        fwd, dgrad = DL._forward, DL.H2ODeepLearningEstimator._dgrad
        outb, gsx, sx = OD.out_backward, OD.gemm_softmax_xent, OD.softmax_xent

        def forward(*a, **k):
            Hs, aux = fwd(*a, **k)
            self.Hs = list(Hs)
            return Hs, aux

        def _dgrad(Hs, aux, dZ, W, act, i, L, Wt=None):
            out = dgrad(Hs, aux, dZ, W, act, i, L, Wt)
            self.dgrad[i] = (dZ, out[0], out[1])
            return out

        def out_backward(dZ, H, W, dW, db, act):
            out = outb(dZ, H, W, dW, db, act)
            self.dgrad["out"] = (dZ, out[0], out[1])
            return out

        def gemm_softmax_xent(H, W, b, y):
            self.Z, self.dZ_out = gsx(H, W, b, y)
            return self.Z, self.dZ_out

        def softmax_xent(Z, y, with_loss=True):
            dZ, loss = sx(Z, y, with_loss)
            self.Z, self.dZ_out = Z, dZ
            return dZ, loss

        monkeypatch.setattr(DL, "_forward", forward)
        monkeypatch.setattr(DL.H2ODeepLearningEstimator, "_dgrad", staticmethod(_dgrad))
        monkeypatch.setattr(OD, "out_backward", out_backward)
        monkeypatch.setattr(OD, "gemm_softmax_xent", gemm_softmax_xent)
        monkeypatch.setattr(OD, "softmax_xent", softmax_xent)   # backend.dense dispatches to it by name


def _setup(sizes, act, M, dev, seed):
    from h2omx.models.deeplearning import _Net

    rng = np.random.default_rng(seed)
    net = _Net(sizes, act, dev, torch.Generator().manual_seed(seed))
    for i in range(len(net.layers)):   # _Net starts with zero biases: a dropped bias would not show
        net.b(i).copy_(torch.from_numpy((0.1 * rng.normal(size=net.b(i).numel())).astype(np.float32)))
    X = torch.from_numpy(rng.normal(size=(2 * M, sizes[0])).astype(np.float32)).to(dev)
    y = torch.from_numpy(rng.integers(0, sizes[-1], size=2 * M).astype(np.int32)).to(dev)
    P = net.flat.numel()
    # non-trivial ADADELTA state (as after a few steps)
    Eg2 = torch.from_numpy((rng.random(P) * 1e-4).astype(np.float32)).to(dev)
    Edx2 = torch.from_numpy((rng.random(P) * 1e-6).astype(np.float32)).to(dev)
    net.grad.fill_(7.0)                # every entry of the gradient must be written by the step
    return net, X, y, Eg2, Edx2


def _check_fp32_stages(rep, net, act, W0, rec, yb, M):
    """every stage of the recorded step from its own device inputs"""
    from h2omx.ops import dense as OD

    L = len(net.layers)
    shapes = [(w, f) for (_, w, f) in net.layers]
    Ws = [net.W(i, W0) for i in range(L)]
    bs = [net.b(i, W0) for i in range(L)]
    Hs = rec.Hs[:L]
    assert len(Hs) == L and rec.Z is not None
    for i in range(L - 1):
        w, f = shapes[i]
        x3 = M * w * f >= OD.X3_MIN_MNK and f % 4 == 0
        DR.check_forward(rep, f"H[{i + 1}]", Hs[i], Ws[i], bs[i], act, Hs[i + 1], 1 if x3 else OD._splitk(M, w, f))
    DR.check_forward(rep, "logits", Hs[L - 1], Ws[L - 1], bs[L - 1], 0, rec.Z)
    DR.check_softmax_grad(rep, f"dZ[{L - 1}]", rec.Z, yb, rec.dZ_out)
    dZ, slices = rec.dZ_out, None
    for i in range(L - 1, -1, -1):
        w, f = shapes[i]
        if i == L - 1:
            S = Sb = OD._row_splits(M, f)
        else:
            S, Sb = OD._splitk(w, f, M), slices[1]
        DR.check_wgrad(rep, f"[{i}]", dZ, Hs[i], net.W(i, net.grad), net.b(i, net.grad), S, Sb)
        if i == 0:
            break
        din, dprev, slices = rec.dgrad["out"] if (i == L - 1 and "out" in rec.dgrad) else rec.dgrad[i]
        assert torch.equal(din, dZ), f"layer {i}: the data gradient did not read the recorded dZ"
        fused = i == L - 1 or OD.dact_ok(dZ, Ws[i])
        DR.check_dgrad(rep, f"dZ[{i - 1}]", dZ, Ws[i], Hs[i], act, dprev, 1 if fused else OD._splitk(M, f, w))
        dZ = dprev


def _expect(got, want):
    for name, n in want.items():
        assert got.get(name, 0) == n, f"route witness {name}: {got.get(name, 0)} launches, expected {n}; all: {got}"


def _run_fp32(monkeypatch, dev, sizes, act, M, l2, mode, seed):
    """one update through the named call sequence; returns (report, witnesses, argument tuples)"""
    import h2omx.models.deeplearning as DL
    from h2omx.backend import dense as D

    Est = DL.H2ODeepLearningEstimator
    net, X, y, Eg2, Edx2 = _setup(sizes, act, M, dev, seed)
    xb, yb = X[M:], y[M:]
    tr = None
    if mode != "bench":
        monkeypatch.setattr(DL._DLTrainer, "FUSED", False)
        monkeypatch.setattr(DL._DLTrainer, "FOLD", mode == "fold")
        p = dict(Est.DEFAULTS)
        p.update(l2=l2, loss="Automatic")
        tr = DL._DLTrainer(p, net, X, y, act, True, False, 0.0, [0.0] * 8, M, 2, None, torch.Generator().manual_seed(1),
                           None, len(sizes) - 2, backward=Est._backward)
        assert tr.fused is None and tr.mlp is None
        tr.Eg2.copy_(Eg2)
        tr.Edx2.copy_(Edx2)
        Eg2, Edx2 = tr.Eg2, tr.Edx2
    W0, E1, E2 = net.flat.clone(), Eg2.clone(), Edx2.clone()
    calls, rec = _Calls(monkeypatch), _Tensors(monkeypatch)
    if tr is None:
        # bench.py _mlp.step
        Hs, aux = DL._forward(net, xb, act, True, 0.0, [0.0] * 8, None)
        dZ, _ = D.softmax_xent(Hs[-1], yb, with_loss=False)
        Est._backward(net, Hs, aux, dZ, act, None, 1)
        D.adadelta_(net.flat, net.grad, Eg2, Edx2, RHO, EPS, l2)
    else:
        tr._body(torch.arange(M, 2 * M, device=dev))
    torch.cuda.synchronize()
    args = calls.take()
    got = _counts(args)
    print(f"\n{sizes} M={M} act={act} {mode}: route witnesses {got}")
    rep = DR.Report(f"{mode}: ")
    _check_fp32_stages(rep, net, act, W0, rec, yb, M)
    rep.assert_ok()
    DR.check_update(f"{mode}: ", W0, net.grad, E1, E2, RHO, EPS, l2, net.flat, Eg2, Edx2)
    return rep, got, args


@pytest.mark.parametrize("mode", ["bench", "fold", "nofold"])
def test_case_a_every_large_route_in_one_net(cuda_dev, monkeypatch, mode):
    """Rectifier, M = 2048, [200, 512, 256, 512, 64, 2]: x3 forward on layers 0-2, split-K fp32 GEMM on
    layer 3, skinny output layer, gemm_wgrad_bias at S = 8, fp32 gemm_dact through W_3 (128 blocks =
    DACT_MIN_BLOCKS, MNK = 2^26), gemm + act_backward_bias through W_2 (64 blocks), x3_transpose +
    gemm_x3_dact through W_1; the bench call sequence and _DLTrainer._body with and without folds"""
    _, got, args = _run_fp32(monkeypatch, cuda_dev, [200, 512, 256, 512, 64, 2], 1, 2048, 0.0, mode, seed=11)
    _expect(got, {"h2omx_gemm_x3": 3, "h2omx_gemm": 2, "h2omx_gemm_wgrad_bias": 4, "h2omx_gemm_dact": 1,
                  "h2omx_act_backward_bias": 1, "h2omx_x3_transpose": 1, "h2omx_gemm_x3_dact": 1,
                  "h2omx_mlp_phase": 0, "h2omx_mlp_out": 0, "h2omx_gemm_bf16": 0})
    assert [a[6] for a in args["h2omx_gemm_wgrad_bias"]] == [8, 8, 8, 8]
    assert [a[11] for a in args["h2omx_gemm"]] == [8, 1]    # layer 3 forward split-K 8; dZ_2 W_2 unsplit
    if mode == "bench":
        _expect(got, {"h2omx_gemm_skinny_nt": 1, "h2omx_softmax_xent": 1, "h2omx_out_wgrad": 1, "h2omx_thin_dact": 1,
                      "h2omx_adadelta": 1, "h2omx_adadelta_fix": 0, "h2omx_out_backward": 0})
    elif mode == "fold":
        _expect(got, {"h2omx_gemm_skinny_softmax": 1, "h2omx_out_backward": 1, "h2omx_adadelta_fix": 1,
                      "h2omx_adadelta": 0, "h2omx_out_wgrad": 0, "h2omx_thin_dact": 0})
    else:
        _expect(got, {"h2omx_gemm_skinny_softmax": 1, "h2omx_out_wgrad": 1, "h2omx_thin_dact": 1, "h2omx_adadelta": 1,
                      "h2omx_adadelta_fix": 0, "h2omx_out_backward": 0})


def test_case_b_ragged_tanh(cuda_dev, monkeypatch):
    """Tanh, M = 2000 (a multiple of 8, not of 64 or 128), [200, 384, 300, 3], l2 = 1e-4: x3 forward with a
    partial row block and a partial column block, no gemm_dact (M % 128), 3 classes, split-K 7"""
    _, got, args = _run_fp32(monkeypatch, cuda_dev, [200, 384, 300, 3], 2, 2000, 1e-4, "fold", seed=12)
    _expect(got, {"h2omx_gemm_x3": 2, "h2omx_gemm_skinny_softmax": 1, "h2omx_out_backward": 1,
                  "h2omx_gemm_wgrad_bias": 2, "h2omx_gemm": 1, "h2omx_act_backward_bias": 1, "h2omx_gemm_dact": 0,
                  "h2omx_gemm_x3_dact": 0, "h2omx_x3_transpose": 0, "h2omx_adadelta_fix": 1, "h2omx_adadelta": 0,
                  "h2omx_mlp_phase": 0})
    assert [a[6] for a in args["h2omx_gemm_wgrad_bias"]] == [7, 7]


def _run_bf16(monkeypatch, dev, sizes, act, B, seed):
    """the benchmark's bf16 body(): load_batch, forward, loss_grad, backward(None, ...), adadelta_, refresh"""
    from h2omx.backend import dense as D
    from h2omx.models.deeplearning import _Bf16Mlp

    net, X, y, Eg2, Edx2 = _setup(sizes, act, B, dev, seed)
    X, y = X[:B].contiguous(), y[:B].contiguous()
    m = _Bf16Mlp(net, act, B, dev)
    L = m.L
    calls = _Calls(monkeypatch)
    m.load_batch(X)
    m.forward(m.Xb)
    m.loss_grad(y)
    m.backward(None, m.Xbt)
    torch.cuda.synchronize()
    args = calls.take()
    # the weight-gradient GEMMs are the ones with c_last; they run from the output layer down
    splits = [a[18] for a in args["h2omx_gemm_bf16"] if a[20]][::-1]
    assert len(splits) == L
    s = DR.bf16_snapshot(m, X, y, splits=splits)
    W0, G, E1, E2 = net.flat.clone(), net.grad.clone(), Eg2.clone(), Edx2.clone()
    D.adadelta_(net.flat, net.grad, Eg2, Edx2, RHO, EPS, 0.0)
    m.refresh()
    torch.cuda.synchronize()
    got = _counts(args)
    got.update(_counts(calls.take()))
    print(f"\nbf16 {sizes} B={B} act={act}: route witnesses {got}, weight-gradient split-K {splits}")
    _expect(got, {"h2omx_cvt_bf16": 1, "h2omx_gemm_bf16": 3 * L - 1, "h2omx_softmax_xent_bf16": 1, "h2omx_adadelta": 1,
                  "h2omx_cvt_bf16_multi": 1, "h2omx_gemm": 0, "h2omx_gemm_x3": 0})
    rep = DR.Report("bf16: ")
    DR.check_bf16_step(s, rep)
    # after the update, Wb / Wbt are the rounded NEW weights
    DR.check_bf16_weights(DR.bf16_snapshot(m, X, y, splits=splits), rep, tag="refreshed ")
    rep.assert_ok()
    assert not torch.equal(s["Wb"][0], m.Wb[0].cpu())
    DR.check_update("bf16: ", W0, G, E1, E2, RHO, EPS, 0.0, net.flat, Eg2, Edx2)
    return splits


def test_case_c_bf16_benchmark_like(cuda_dev, monkeypatch):
    """Rectifier, B = 2048, [200, 512, 512, 2]: split-K 8 in every weight gradient"""
    splits = _run_bf16(monkeypatch, cuda_dev, [200, 512, 512, 2], 1, 2048, seed=13)
    assert splits == [8, 8, 8]


def test_case_d_bf16_ragged(cuda_dev, monkeypatch):
    """Tanh, B = 1000, [203, 520, 70, 3]: kp padding, 204-column weight gradients with c_last, S = 3,
    partial 4-row groups of the transposed store"""
    splits = _run_bf16(monkeypatch, cuda_dev, [203, 520, 70, 3], 2, 1000, seed=14)
    assert splits == [3, 3, 3]
