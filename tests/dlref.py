"""Float64 reference of the DeepLearning training step, whole and stage by stage.

No GPU and no kernel code in here: plain torch float64 on the CPU.

* :func:`reference` is one whole update (autograd + H2O's ADADELTA); it is what
  ``tests/test_dl_step_gpu.py`` compares small-batch steps with.
* The stage checkers verify every product of a step from that stage's OWN
  device inputs (the activations, gradients and weights the GPU actually
  held), so a Rectifier unit whose pre-activation sits within fp32 rounding of
  zero cannot flip between the GPU and the reference, and every bound is the
  bound of a single GEMM.  The chain closes because each stage's verified
  output is the next stage's input.

Stage bound (derived, not measured).  For ``C = A B^T`` of inner length K,
reduced over S split-K partials, with an optional bias, the device's fp32 value
``v`` must satisfy

    |v_ij - r_ij| <= t_ij = 2 (K + S + 8) 2^-24 ((|A| |B|^T)_ij + |bias_j|)

with ``r`` the float64 result from the same operand values: the worst-case fp32
summation bound for any order, times 2 for the non-IEEE rounding inside MFMA
accumulation; ``+ 8`` covers bias, activation, output rounding and the three
dropped cross terms of the x3 operand split.  Rectifier and the derivative
epilogues are contractions, so ``t`` holds after them; ``tanhf`` adds
``4 * 2^-24`` absolute (2 ulp on outputs in [-1, 1], an assumption).

bf16 outputs.  A stored bf16 ``b`` is accepted iff
``rne_bf16(r - t') <= b <= rne_bf16(r + t')`` with ``t' = t + 2^-24 |r|`` (the
float64 -> float32 -> bf16 double rounding of the end points).  The row-major
and transposed copies of one output must be bit-identical transposes, pad
columns zero, ones rows ones, conversions equal to ``x.to(torch.bfloat16)``.

Softmax gradient: ``|M dZ - (softmax - onehot)| <= 3e-4`` (the bound of
``test_mlp_elementwise``, ``atol=1e-6`` at M = 300, without its 1 / M).

Every check adds a row to a :class:`Report`; fp32 rows carry ``max |v - r| / t``.
"""
import numpy as np
import torch

U = 2.0 ** -24
TANH_ABS = 4 * U
SOFTMAX_TOL = 3e-4
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------
# the whole step
# ---------------------------------------------------------------------------
def adadelta(W, G, Eg2, Edx2, rho, eps, l2):
    """H2O's ADADELTA in float64: (new W, Eg2, Edx2)."""
    W, G, Eg2, Edx2 = (f64(t) for t in (W, G, Eg2, Edx2))
    g = G + l2 * W
    Eg2 = rho * Eg2 + (1 - rho) * g * g
    dx = -torch.sqrt(Edx2 + eps) / torch.sqrt(Eg2 + eps) * g
    Edx2 = rho * Edx2 + (1 - rho) * dx * dx
    return W + dx, Eg2, Edx2


def reference(sizes, act, W0, X, y, regression, rho, eps, l2, Eg2_0, Edx2_0, layers):
    """float64 autograd step: returns (grad, new flat, Eg2, Edx2)."""
    flat = torch.from_numpy(W0).double().requires_grad_(True)
    H = torch.from_numpy(X).double()
    L = len(layers)
    for i, (off, w, f) in enumerate(layers):
        Wl = flat[off: off + w * f].view(w, f)
        bl = flat[off + w * f: off + w * f + w]
        Z = H @ Wl.T + bl
        if i < L - 1:
            H = torch.relu(Z) if act == 1 else torch.tanh(Z)
        else:
            H = Z
    if regression:
        loss = 0.5 * ((H[:, 0] - torch.from_numpy(y).double()) ** 2).mean()
    else:
        loss = torch.nn.functional.cross_entropy(H, torch.from_numpy(y).long())
    loss.backward()
    G = flat.grad.detach().clone()
    Wn = flat.detach().clone()
    g = G + l2 * Wn
    Eg2 = rho * torch.from_numpy(Eg2_0).double() + (1 - rho) * g * g
    Edx2 = torch.from_numpy(Edx2_0).double()
    dx = -torch.sqrt(Edx2 + eps) / torch.sqrt(Eg2 + eps) * g
    Edx2 = rho * Edx2 + (1 - rho) * dx * dx
    return G.numpy(), (Wn + dx).numpy(), Eg2.numpy(), Edx2.numpy()


def close(name, got, want, rtol=1e-4):
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want) / (np.abs(want) + 1e-3 * scale)
    assert err.max() <= rtol, f"{name}: max rel err {err.max():.3g} at {int(err.argmax())}"


# ---------------------------------------------------------------------------
# stage references (float64 in, float64 out)
# ---------------------------------------------------------------------------
def f64(x) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    return x.detach().cpu().double()


def act_fn(Z, act):
    return torch.relu(Z) if act == 1 else torch.tanh(Z) if act == 2 else Z


def act_prime(H, act):
    """act' as a function of the layer's OUTPUT (what the kernels read)."""
    return (H > 0).double() if act == 1 else 1 - H * H if act == 2 else torch.ones_like(H)


def ref_forward(H, W, b, act):
    return act_fn(H @ W.T + b, act)


def ref_softmax_grad(Z, y):
    M, C = Z.shape
    oh = torch.nn.functional.one_hot(y.long(), C).double()
    return (torch.softmax(Z, 1) - oh) / M


def ref_dgrad(dZ, W, H, act):
    return (dZ @ W) * act_prime(H, act)


def ref_wgrad(dZ, H):
    return dZ.T @ H


def ref_bgrad(dZ):
    return dZ.sum(0)


def bound(A, B, S=1, bias=None):
    """t of the stage bound for A [M][K] B [N][K]^T (float64 operands)."""
    K = A.shape[1]
    m = A.abs() @ B.abs().T
    if bias is not None:
        m = m + bias.abs()
    return 2.0 * (K + S + 8) * U * m


def rne_bf16(x):
    """float64 -> float32 -> bf16, round to nearest even, back as float64."""
    return x.float().to(BF16).double()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------
class Report:
    """rows of (check name, kind, figure, entries out of bounds, entries)"""

    def __init__(self, label=""):
        self.label = label
        self.rows = []
        self.bad = {}

    def _add(self, name, kind, figure, bad):
        self.rows.append((name, kind, figure, int(bad.sum()), bad.numel()))
        self.bad[name] = bad

    def fp32(self, name, v, r, t, abs_extra=0.0):
        """|v - r| <= t (+ abs_extra); figure = max |v - r| / t"""
        v = f64(v)
        assert v.shape == r.shape, (name, v.shape, r.shape)
        tt = t + abs_extra
        err = (v - r).abs()
        ratio = torch.where(tt > 0, err / tt.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        self._add(name, "fp32", float(ratio.max()) if ratio.numel() else 0.0, ratio > 1)

    def bf16(self, name, b, r, t):
        """rne(r - t') <= b <= rne(r + t'); figure = share of entries that are not rne(r)"""
        assert b.dtype == BF16 and b.shape == r.shape, (name, b.dtype, b.shape, r.shape)
        b = b.detach().cpu().double()
        tp = t + U * r.abs()
        bad = ~((rne_bf16(r - tp) <= b) & (b <= rne_bf16(r + tp)))
        self._add(name, "bf16", float((b != rne_bf16(r)).double().mean()) if b.numel() else 0.0, bad)

    def same_bits(self, name, got, want):
        assert got.dtype == BF16 and want.dtype == BF16 and got.shape == want.shape, (name, got.shape, want.shape)
        self._add(name, "bits", 0.0, _bits(got.detach().cpu()) != _bits(want.detach().cpu()))

    def equals(self, name, got, value):
        self._add(name, "const", 0.0, got.detach().cpu().double() != value)

    def failed(self):
        return [r[0] for r in self.rows if r[3]]

    def share(self, name):
        return float(self.bad[name].double().mean())

    def lines(self):
        out = []
        for name, kind, fig, nbad, n in self.rows:
            if kind == "fp32":
                out.append(f"{self.label}{name}: max |v-r|/t = {fig:.4g} ({nbad} of {n} over)")
            elif kind == "bf16":
                out.append(f"{self.label}{name}: {nbad} of {n} outside [rne(r-t'), rne(r+t')], "
                           f"{100 * fig:.3g}% != rne(r)")
            else:
                out.append(f"{self.label}{name}: {nbad} of {n} differ")
        return out

    def summary(self):
        """one line per check"""
        return "\n".join(self.lines())

    def assert_ok(self):
        print(self.summary())
        bad = self.failed()
        assert not bad, "stages out of bounds: " + "; ".join(
            ln for ln, r in zip(self.lines(), self.rows) if r[3])


# ---------------------------------------------------------------------------
# fp32 stage checkers (device values in, one report row each)
# ---------------------------------------------------------------------------
def check_forward(rep, name, H, W, b, act, v, S=1):
    """v = act(H W^T + b)"""
    H, W, b = f64(H), f64(W), f64(b)
    rep.fp32(name, v, ref_forward(H, W, b, act), bound(H, W, S, b), TANH_ABS if act == 2 else 0.0)


def check_softmax_grad(rep, name, Z, y, dZ):
    """|M dZ - (softmax(Z) - onehot)| <= 3e-4 from the device logits Z"""
    Z = f64(Z)
    M = Z.shape[0]
    r = ref_softmax_grad(Z, y.detach().cpu()) * M
    rep.fp32(name, f64(dZ) * M, r, torch.full_like(r, SOFTMAX_TOL))


def check_dgrad(rep, name, dZ, W, H, act, v, S=1):
    """v = (dZ W) * act'(H), act' from the device H"""
    dZ, W, H = f64(dZ), f64(W), f64(H)
    rep.fp32(name, v, ref_dgrad(dZ, W, H, act), bound(dZ, W.T, S))


def check_wgrad(rep, name, dZ, H, vW, vb, S=1, Sb=1):
    """vW = dZ^T H, vb = column sums of dZ (K = rows in the bound)"""
    dZ, H = f64(dZ), f64(H)
    rep.fp32("dW" + name, vW, ref_wgrad(dZ, H), bound(dZ.T, H.T, S))
    ones = torch.ones((1, dZ.shape[0]), dtype=torch.float64)
    rep.fp32("db" + name, vb, ref_bgrad(dZ), bound(dZ.T, ones, Sb)[:, 0])


def check_update(tag, W0, G, Eg2_0, Edx2_0, rho, eps, l2, W1, Eg2_1, Edx2_1):
    """ADADELTA in float64 from the device's own (W, G, Eg2, Edx2) before the update"""
    Wn, E1, E2 = adadelta(W0, G, Eg2_0, Edx2_0, rho, eps, l2)
    close(tag + "weights", f64(W1).numpy(), Wn.numpy())
    close(tag + "Eg2", f64(Eg2_1).numpy(), E1.numpy())
    close(tag + "Edx2", f64(Edx2_1).numpy(), E2.numpy())


# ---------------------------------------------------------------------------
# _Bf16Mlp: every buffer it keeps is a stage boundary
# ---------------------------------------------------------------------------
def bf16_wgrad_splits(w, f, B):
    """split-K of the weight-gradient GEMM [w][f + 1] over B rows (as _Bf16Mlp.backward chooses it)"""
    tiles = -(-w // 128) * -(-(f + 1) // 128)
    return max(1, min(64, 256 // tiles, B // 256))


def bf16_snapshot(m, X, y, splits=None):
    """CPU copies of everything a _Bf16Mlp step read and wrote (take it before the update)"""
    def c(t):
        return None if t is None else t.detach().cpu().clone()

    net = m.net
    L = m.L
    return dict(act=m.act, B=m.B, L=L, shapes=list(m.shapes), kp=list(m.kp), wp=list(m.wp), layers=list(net.layers),
                X=c(X), y=c(y), flat=c(net.flat), grad=c(net.grad), Xb=c(m.Xb), Xbt=c(m.Xbt),
                Wb=[c(t) for t in m.Wb], Wbt=[c(t) for t in m.Wbt], H=[c(t) for t in m.H], Ht=[c(t) for t in m.Ht],
                logits=c(m.logits), dZ=[c(t) for t in m.dZ], dZt=[c(t) for t in m.dZt],
                splits=splits or [bf16_wgrad_splits(w, f, m.B) for (w, f) in m.shapes])


def span(s, i, buf):
    """layer i's (W, b) views of a flat parameter / gradient buffer of the snapshot"""
    off, w, f = s["layers"][i]
    return buf[off: off + w * f].view(w, f), buf[off + w * f: off + w * f + w]


def _pair(rep, name, tname, row, col, R, C, ones=False):
    """row [R][>=C] and its transposed copy col [C (+1)][>=R]: same bits, zero pads, ones row"""
    rep.same_bits(tname, col[:C, :R], row[:R, :C].T.contiguous())
    if row.shape[1] > C:
        rep.equals(name + ".pad", row[:R, C:], 0.0)
    if ones:
        assert col.shape[0] == C + 1, (name, col.shape)
        rep.equals(tname + ".ones", col[C], 1.0)


def check_bf16_weights(s, rep, flat=None, tag=""):
    """Wb / Wbt = the rounded fp32 master weights (``flat``: the weights they must hold)"""
    flat = s["flat"] if flat is None else flat.detach().cpu()
    for i, (w, f) in enumerate(s["shapes"]):
        W, _ = span(s, i, flat)
        rep.same_bits(f"{tag}Wb[{i}]", s["Wb"][i][:, :f], W.to(BF16))
        if s["kp"][i] > f:
            rep.equals(f"{tag}Wb[{i}].pad", s["Wb"][i][:, f:], 0.0)
        rep.same_bits(f"{tag}Wbt[{i}]", s["Wbt"][i][:, :w], W.T.contiguous().to(BF16))
        if s["wp"][i] > w:
            rep.equals(f"{tag}Wbt[{i}].pad", s["Wbt"][i][:, w:], 0.0)


def check_bf16_step(s, rep):
    """load_batch, forward, loss_grad, backward of one _Bf16Mlp step, buffer by buffer"""
    act, B, L = s["act"], s["B"], s["L"]
    f0 = s["shapes"][0][1]
    # conversions
    rep.same_bits("Xb", s["Xb"][:, :f0], s["X"].to(BF16))
    _pair(rep, "Xb", "Xbt", s["Xb"], s["Xbt"], B, f0, ones=True)
    check_bf16_weights(s, rep)
    # forward
    Hin = s["Xb"]
    for i, (w, f) in enumerate(s["shapes"]):
        A, Wb = f64(Hin), f64(s["Wb"][i])
        b = f64(span(s, i, s["flat"])[1])
        r, t = ref_forward(A, Wb, b, act if i < L - 1 else 0), bound(A, Wb, 1, b)
        if i == L - 1:
            rep.fp32("logits", s["logits"], r, t)
            break
        rep.bf16(f"H[{i + 1}]", s["H"][i + 1][:, :w], r, t + (TANH_ABS if act == 2 else 0.0))
        _pair(rep, f"H[{i + 1}]", f"Ht[{i + 1}]", s["H"][i + 1], s["Ht"][i + 1], B, w, ones=True)
        Hin = s["H"][i + 1]
    # loss gradient from the device logits
    C = s["shapes"][-1][0]
    r = ref_softmax_grad(f64(s["logits"]), s["y"])
    rep.bf16(f"dZ[{L - 1}]", s["dZ"][L - 1][:, :C], r, torch.full_like(r, SOFTMAX_TOL / B))
    # backward
    for i in range(L - 1, -1, -1):
        w, f = s["shapes"][i]
        _pair(rep, f"dZ[{i}]", f"dZt[{i}]", s["dZ"][i], s["dZt"][i], B, w)
        Hin_t = s["Xbt"] if i == 0 else s["Ht"][i]
        A, Bm = f64(s["dZt"][i][:, :B]), f64(Hin_t[:, :B])
        r, t = A @ Bm.T, bound(A, Bm, s["splits"][i])
        gW, gb = span(s, i, s["grad"])
        rep.fp32(f"dW[{i}]", gW, r[:, :f], t[:, :f])
        rep.fp32(f"db[{i}]", gb, r[:, f], t[:, f])
        if i == 0:
            break
        A, Bm = f64(s["dZ"][i]), f64(s["Wbt"][i])
        r = (A @ Bm.T) * act_prime(f64(s["H"][i][:, :f]), act)
        rep.bf16(f"dZ[{i - 1}]", s["dZ"][i - 1][:, :f], r, bound(A, Bm, 1))
