"""CPU audit of the DeepLearning stage oracle (tests/dlref.py).

* the stage references chained end to end are the same function as float64
  autograd (so verifying every stage verifies the gradient);
* the checkers accept the bf16 step's CPU contract (``reference/dense.py``
  under ``_Bf16Mlp``) and an fp32 CPU step;
* power: each way a kernel goes subtly wrong is rejected, and by the check
  that is meant to see it."""
import numpy as np
import pytest
import torch

import dlref as DR
from h2omx.backend import dense as D
from h2omx.models.deeplearning import _Bf16Mlp, _Net

BF16 = torch.bfloat16


def _net(sizes, act, seed=0):
    net = _Net(sizes, act, "cpu", torch.Generator().manual_seed(seed))
    g = torch.Generator().manual_seed(seed + 100)
    for i in range(len(net.layers)):       # _Net starts with zero biases: a dropped bias would not show
        net.b(i).copy_(0.2 * torch.randn(net.b(i).shape, generator=g))
    return net


# ---------------------------------------------------------------------------
# fp32: the stage decomposition is the gradient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,M,l2", [([7, 12, 9, 3], 33, 0.0), ([20, 48, 24, 3], 64, 1e-4), ([5, 16, 2], 10, 0.0)])
def test_chained_stage_references_are_the_autograd_gradient(sizes, M, l2):
    act = 2
    net = _net(sizes, act, seed=M)
    L = len(net.layers)
    rng = np.random.default_rng(M)
    X = rng.normal(size=(M, sizes[0])).astype(np.float32)
    y = rng.integers(0, sizes[-1], size=M).astype(np.int32)
    W0 = net.flat.numpy().copy()
    P = W0.size
    E1, E2 = (rng.random(P) * 1e-4).astype(np.float32), (rng.random(P) * 1e-6).astype(np.float32)
    G, Wn, Eg2, Edx2 = DR.reference(sizes, act, W0, X, y, False, 0.99, 1e-8, l2, E1, E2, net.layers)
    flat = DR.f64(W0)
    Ws = [net.W(i, flat) for i in range(L)]
    bs = [net.b(i, flat) for i in range(L)]
    Hs = [DR.f64(X)]
    for i in range(L):
        Hs.append(DR.ref_forward(Hs[-1], Ws[i], bs[i], act if i < L - 1 else 0))
    dZ = DR.ref_softmax_grad(Hs[-1], torch.from_numpy(y))
    grad = torch.zeros_like(flat)
    for i in range(L - 1, -1, -1):
        net.W(i, grad).copy_(DR.ref_wgrad(dZ, Hs[i]))
        net.b(i, grad).copy_(DR.ref_bgrad(dZ))
        if i:
            dZ = DR.ref_dgrad(dZ, Ws[i], Hs[i], act)
    assert np.abs(grad.numpy() - G).max() <= 1e-12 * np.abs(G).max()
    Wc, E1c, E2c = DR.adadelta(W0, grad, E1, E2, 0.99, 1e-8, l2)
    for got, want in ((Wc, Wn), (E1c, Eg2), (E2c, Edx2)):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("act", [1, 2])
def test_fp32_checkers_accept_a_cpu_step_and_reject_a_dropped_term(act):
    """the fp32 stage checkers on torch's own float32 products (K = 200: a dropped k-term, a
    missing bias and a derivative read from the wrong unit are all far outside t)"""
    g = torch.Generator().manual_seed(act)
    M, K, N = 96, 200, 40
    H = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = 0.2 * torch.randn(N, generator=g)
    Y = D.gemm(H, W, bias=b, act=act, tb=True)
    dZn = torch.randn(M, N, generator=g) / M
    dH = D.gemm(dZn, W)
    Yin = D.gemm(torch.randn(M, 30, generator=g), torch.randn(K, 30, generator=g) / 5, act=act, tb=True)
    D.act_backward(Yin, dH, act)
    dW, db = D.gemm(dZn, H, ta=True), D.bias_grad(dZn)
    rep = DR.Report("cpu fp32: ")
    DR.check_forward(rep, "H", H, W, b, act, Y)
    DR.check_dgrad(rep, "dZ", dZn, W, Yin, act, dH)
    DR.check_wgrad(rep, "", dZn, H, dW, db)
    rep.assert_ok()
    assert max(r[2] for r in rep.rows) < 1
    bad = DR.Report()
    Hd = H.clone()
    Hd[:, 17] = 0
    DR.check_forward(bad, "H-k", H, W, b, act, D.gemm(Hd, W, bias=b, act=act, tb=True))
    DR.check_forward(bad, "H-bias", H, W, b, act, D.gemm(H, W, act=act, tb=True))
    DR.check_dgrad(bad, "dZ-unit", dZn, W, Yin, act, D.act_backward(Yin.roll(1, 1), D.gemm(dZn, W), act))
    DR.check_wgrad(bad, "-row", dZn, H, D.gemm(dZn[1:], H[1:], ta=True), D.bias_grad(dZn[1:]))
    print("\n".join(bad.lines()))
    assert bad.failed() == ["H-k", "H-bias", "dZ-unit", "dW-row", "db-row"]


# ---------------------------------------------------------------------------
# bf16: pass cases on the CPU contract
# ---------------------------------------------------------------------------
def _bf16_step(sizes, act, B, seed=0):
    """one CPU step of _Bf16Mlp as the benchmark runs it; returns (mlp, snapshot before the update)"""
    net = _net(sizes, act, seed)
    g = torch.Generator().manual_seed(seed + 1)
    X = torch.randn(B, sizes[0], generator=g)
    y = torch.randint(0, sizes[-1], (B,), generator=g, dtype=torch.int32)
    m = _Bf16Mlp(net, act, B, "cpu")
    xb, xbt = m.load_batch(X)
    m.forward(xb)
    m.loss_grad(y)
    net.grad.zero_()
    m.backward(None, xbt)
    return m, DR.bf16_snapshot(m, X, y)


_steps = {}


def _step(sizes, act, B):
    """computed once per shape; tests take copies (``_copy``) and leave it unchanged"""
    key = (tuple(sizes), act, B)
    if key not in _steps:
        _steps[key] = _bf16_step(sizes, act, B, seed=B)
    return _steps[key]


def _copy(s):
    c = lambda v: v.clone() if torch.is_tensor(v) else [c(u) for u in v] if isinstance(v, list) else v
    return {k: c(v) for k, v in s.items()}


SIZES = [20, 48, 24, 3]
RAGGED = [19, 50, 21, 3]    # every width off the 8-element row padding


@pytest.mark.parametrize("sizes,B", [(SIZES, 64), (RAGGED, 72)], ids=["even", "ragged"])
@pytest.mark.parametrize("act", [1, 2])
def test_bf16_checkers_accept_the_cpu_contract(sizes, B, act):
    m, s = _step(sizes, act, B)
    rep = DR.Report(f"cpu bf16 {sizes} B={B} act={act}: ")
    DR.check_bf16_step(s, rep)
    rep.assert_ok()
    ratios = [r[2] for r in rep.rows if r[1] == "fp32"]
    print(f"max |v-r|/t = {max(ratios):.4g}")
    assert max(ratios) < 1
    # the update and the refreshed bf16 weights
    net = m.net
    W0, G = net.flat.clone(), net.grad.clone()
    g = torch.Generator().manual_seed(3)
    Eg2 = torch.rand(W0.shape, generator=g) * 1e-4
    Edx2 = torch.rand(W0.shape, generator=g) * 1e-6
    E1, E2 = Eg2.clone(), Edx2.clone()
    D.adadelta_(net.flat, net.grad, Eg2, Edx2, 0.99, 1e-8, 0.0)
    m.refresh()
    DR.check_update("", W0, G, E1, E2, 0.99, 1e-8, 0.0, net.flat, Eg2, Edx2)
    after = DR.Report("after refresh: ")
    DR.check_bf16_weights(DR.bf16_snapshot(m, s["X"], s["y"]), after)
    after.assert_ok()
    assert not torch.equal(s["Wb"][0], m.Wb[0])
    net.flat.copy_(W0)   # the cached step stays as it was
    m.refresh()


# ---------------------------------------------------------------------------
# power: every mutation is rejected, by the check named here
# ---------------------------------------------------------------------------
def _failed(s):
    rep = DR.Report()
    DR.check_bf16_step(s, rep)
    return rep


def _trunc_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits (what a kernel without rounding stores)"""
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def _fwd32(s, i, bias=True, drop_k=None):
    """layer i's fp32 output of the CPU contract, optionally without its bias / without one k-term"""
    A = (s["Xb"] if i == 0 else s["H"][i]).float()
    if drop_k is not None:
        A = A.clone()
        A[:, drop_k] = 0
    w, f = s["shapes"][i]
    c = A @ s["Wb"][i].float().T
    if bias:
        c = c + DR.span(s, i, s["flat"])[1]
    if i < s["L"] - 1:
        c = torch.relu(c) if s["act"] == 1 else torch.tanh(c)
    return c


def _set_h(s, i, c):
    """store layer i's output consistently (row-major and transposed)"""
    w = c.shape[1]
    s["H"][i + 1][:, :w] = c
    s["Ht"][i + 1][:w, :] = c.T


@pytest.mark.parametrize("act", [1, 2])
def test_bf16_checkers_reject_each_mutation(act):
    _, base = _step(SIZES, act, 64)
    L = base["L"]
    seen = {}

    def run(name, s, must, readers=()):
        """``must`` rejects; besides it only the stages that READ the mutated buffer may (their
        reference is then computed from the mutated input, the recorded output is not)"""
        rep = _failed(s)
        seen[name] = rep.failed()
        print(f"{name}: rejected by {must}; readers that notice: {[n for n in rep.failed() if n != must]}")
        assert must in rep.failed(), (name, rep.failed())
        assert set(rep.failed()) <= {must, *readers}, (name, rep.failed())
        return rep

    r_logits = (f"dZ[{L - 1}]",)
    r_h1 = ("H[2]", "dZ[0]", "dW[1]", "db[1]")
    r_h2 = ("logits", "dZ[1]", "dW[2]", "db[2]")

    # one k-term dropped from one product: an fp32 output (logits) and a bf16 one (H[1])
    s = _copy(base)
    s["logits"] = _fwd32(s, L - 1, drop_k=5)
    run("k-term dropped (logits)", s, "logits", r_logits)
    s = _copy(base)
    _set_h(s, 0, _fwd32(s, 0, drop_k=3).to(BF16))
    run("k-term dropped (H[1])", s, "H[1]", r_h1)
    # bias omitted
    s = _copy(base)
    _set_h(s, 1, _fwd32(s, 1, bias=False).to(BF16))
    run("bias omitted (H[2])", s, "H[2]", r_h2)
    s = _copy(base)
    s["logits"] = _fwd32(s, L - 1, bias=False)
    run("bias omitted (logits)", s, "logits", r_logits)
    # truncation instead of round-to-nearest on a bf16 output
    s = _copy(base)
    c = _fwd32(s, 0)
    _set_h(s, 0, _trunc_bf16(c))
    rep = run("truncated (H[1])", s, "H[1]", r_h1)
    differs = float((_trunc_bf16(c) != c.to(BF16)).double().mean())
    print(f"  truncation differs from rne on {differs:.3f} of H[1], rejected on {rep.share('H[1]'):.3f}")
    assert rep.share("H[1]") >= 0.95 * differs > 0.2
    # the softmax gradient truncated as well (the interval rule with t = 3e-4 / B)
    s = _copy(base)
    g32 = DR.ref_softmax_grad(DR.f64(s["logits"]), s["y"]).float()
    C = g32.shape[1]
    s["dZ"][L - 1][:, :C] = _trunc_bf16(g32)
    s["dZt"][L - 1][:, :] = _trunc_bf16(g32).T
    run(f"truncated (dZ[{L - 1}])", s, f"dZ[{L - 1}]", (f"dZ[{L - 2}]", f"dW[{L - 1}]", f"db[{L - 1}]"))
    # one pad column non-zero
    s = _copy(base)
    s["Xb"][5, 21] = 1.0
    run("pad column (Xb)", s, "Xb.pad")
    s = _copy(base)
    s["dZ"][L - 1][7, 5] = 1e-3
    run(f"pad column (dZ[{L - 1}])", s, f"dZ[{L - 1}].pad")
    # the ones row shifted by one
    s = _copy(base)
    s["Ht"][1] = s["Ht"][1].roll(-1, 0)
    run("ones row shifted (Ht[1])", s, "Ht[1].ones", ("Ht[1]", "dW[1]", "db[1]"))
    s = _copy(base)
    s["Xbt"][-1, :-1] = s["Xbt"][-1, 1:].clone()
    s["Xbt"][-1, -1] = 0
    run("ones row shifted along the batch (Xbt)", s, "Xbt.ones", ("db[0]",))
    # Ht holding a different rounding than H
    s = _copy(base)
    up = (s["H"][2].view(torch.int16) + 1).view(BF16)   # the next bf16: what rounding the other way stores
    s["Ht"][2][:-1, 9] = up[9, : s["shapes"][1][0]]
    run("Ht != H^T (Ht[2])", s, "Ht[2]", ("dW[2]",))
    # the bias gradient taken from the wrong column (the last weight column, not the ones row)
    s = _copy(base)
    gW, gb = DR.span(s, 1, s["grad"])
    gb.copy_(gW[:, -1])
    run("db from the wrong column", s, "db[1]")
    assert len(seen) == 12


def test_wgrad_bound_sees_one_dropped_batch_row_at_2048():
    """B = 2048: t = 2 (2048 + 8 + 8) 2^-24 sum |dz| |h| is about half a mean term, so a single
    dropped row is visible wherever its term is at least of average size; demanded on at least
    half of the layer's entries"""
    _, base = _step(SIZES, 2, 2048)
    ok = _failed(base)
    assert ok.failed() == []
    s = _copy(base)
    i, row = 0, 0
    assert s["splits"][i] == 8
    gW, _ = DR.span(s, i, s["grad"])
    w, f = s["shapes"][i]
    gW.sub_(s["dZt"][i][:, row].float()[:, None] * s["Xbt"][:f, row].float()[None, :])
    rep = _failed(s)
    share = rep.share(f"dW[{i}]")
    print(f"dropped row {row} of dW[{i}] at B = 2048: rejected on {share:.3f} of {w * f} entries by dW[{i}]")
    assert rep.failed() == [f"dW[{i}]"]
    assert share >= 0.5
