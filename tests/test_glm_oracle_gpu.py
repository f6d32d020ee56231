"""GLM passes on the GPU against the independent float64 oracle (tests/glmref.py),
on every kernel route.

Routes are pinned with the module flags of ``h2omx.ops.dense``:

  split   glm_irls_split_kernel   GLM_WAVE, GLM_GRAM = "split"; 1 <= p <= 126.  LDS-DMA staging
                                  when ld % 4 == 0 and the base is 16-byte aligned, else
                                  register prefetch with scalar loads; FAM 1 = binomial / logit
  wave    glm_irls_wave_kernel    GLM_GRAM = "f32"; 0 <= p <= 126; 16-byte or scalar loads
  wg      glm_irls_kernel<TP>     GLM_WAVE = False (or multinomial); p <= 254
  wide    glm_wz -> glm_aug -> Gram GEMM   p = 255 through glm_irls_pass; narrower designs call
                                  the same chain (_glm_irls_wide) directly
  grad    glm_resid / glm_xtr     glm_grad_pass

Layers: (a) exact structural tests on dyadic inputs (==, any accumulation
order), (b) the bf16 split's six kept products (==), (c) per-row family math on
diagonal designs (8 * 2^-24 per entry), (d) dense designs (entry-wise bounds
relative to |A| W |A|^T), the gradient pass and the identity that ties the two
passes, (e) floors and saturation.

Not covered: the multi-chunk wide path (n > 2^27 / (p + 2), over 500k rows at
p = 255; too large for a seconds-long test and its chunk size is not a module
constant), solver behaviour, NaN imputation inside the pass, multi-rank runs.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import glmref as R

gpu = pytest.mark.gpu
EPS = 2.0 ** -24
IDS = [R.combo_id(c) for c in R.COMBOS]
ROUTE_FLAGS = {"split": (True, "split"), "wave": (True, "f32"), "wg": (False, "split"), "wide": (True, "split")}
WORST = {}      # route -> largest observed |G - Gref| / (2^-24 absG) in layer (d)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    if WORST:
        print("\nGLM oracle, layer (d): largest |err| / (2^-24 absG) per route:",
              ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items())))


@contextlib.contextmanager
def pinned(route):
    from h2omx.ops import dense as DD

    old = DD.GLM_WAVE, DD.GLM_GRAM
    DD.GLM_WAVE, DD.GLM_GRAM = ROUTE_FLAGS[route]
    try:
        yield DD
    finally:
        DD.GLM_WAVE, DD.GLM_GRAM = old


def f32(a):
    a32 = np.asarray(a, np.float32)
    assert (a32.astype(np.float64) == np.asarray(a, np.float64)).all(), "test input is not exact in fp32"
    return a32


def layout_ld_offset(n, layout):
    """(leading dimension, first column) of the design inside its parent buffer."""
    if layout == "plain":
        return n, 0
    if layout == "view4":                     # aligned base, ld > n, ld % 4 == 0
        return (n + 8 + 3) // 4 * 4, 4
    if layout == "view3":                     # ld % 4 == 0 but the base is 12 bytes off
        return (n + 8 + 3) // 4 * 4, 3
    if layout == "ldodd":                     # ld % 4 != 0
        return (n + 8) // 4 * 4 + 1, 0
    raise ValueError(layout)


def place(X, layout, dev):
    """The design as a device tensor in the given memory layout; everything of
    the parent buffer outside the view is NaN, so a read outside it shows."""
    X = f32(X)
    p, n = X.shape
    ld, c0 = layout_ld_offset(n, layout)
    if layout == "plain":
        return torch.from_numpy(X).to(dev)
    big = torch.full((p, ld), float("nan"), dtype=torch.float32, device=dev)
    v = big[:, c0:c0 + n]
    v.copy_(torch.from_numpy(X))
    assert v.stride(1) == 1 and v.stride(0) == ld
    return v


def instance(route, p, n, layout="plain", family="gaussian", link="identity"):
    """The template instance a call lands on (for the coverage check)."""
    if route in ("split", "wave"):
        ld, c0 = layout_ld_offset(n, layout)
        vec = ld % 4 == 0 and c0 % 4 == 0
        nb = (p + 2 + 15) // 16
        if route == "split":
            return "split", nb, vec, int(family == "binomial" and link == "logit")
        return "wave", nb, vec
    if route == "wg":
        return "wg", next(tp for tp in (1, 2, 4, 8) if p + 2 <= 32 * tp)
    return (route,)


def dt(a, dev):
    return None if a is None else torch.from_numpy(f32(a)).to(dev)


def run_irls(dev, route, X, y, w, off, beta, family, link, layout="plain", **kw):
    p, n = X.shape
    if route in ("split", "wave"):
        assert family != "multinomial" and p + 2 <= 128
    if route == "wg":
        assert p + 2 <= 256
    beta = f32(beta).astype(np.float64)
    with pinned(route) as DD:
        args = (place(X, layout, dev), dt(y, dev), dt(w, dev), dt(off, dev), beta, family, link)
        if route == "wide" and p + 2 <= 256:
            return DD._glm_irls_wide(*args, kw.get("cls", 0), kw.get("var_power", 1.5), kw.get("link_power", 0.0))
        return DD.glm_irls_pass(*args, **kw)


def run_grad(dev, X, y, w, off, beta, family, link, **kw):
    from h2omx.ops import dense as DD

    return DD.glm_grad_pass(place(X, "plain", dev), dt(y, dev), dt(w, dev), dt(off, dev),
                            f32(beta).astype(np.float64), family, link, **kw)


# ---------------------------------------------------------------------------
# (a) exact structural layer
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(setting, p, n, wmode):
    """Design and oracle of one exact case (shared by every route that runs it)."""
    use_w = wmode in ("w", "w+off", "zero90", "tail0")
    use_off = wmode in ("off", "w+off", "zero90", "tail0")
    X, y, w, off, beta, family, link, quantum = R.exact_design(
        1000 * p + n, setting, p, n, use_w, use_off, 0.9 if wmode == "zero90" else None)
    if wmode == "tail0":                      # a zero-weight tail: stale rows of the last chunk must not count
        w = w.copy()
        w[n - max(1, n // 50):] = 0.0
    r = R.irls(X, y, w, off, beta, family, link)
    assert n * r.absG.max() / quantum < 2.0 ** 24, "precondition of exactness"
    return X, y, w, off, beta, family, link, r


def check_exact(dev, route, setting, p, n, wmode="w+off", layout="plain"):
    X, y, w, off, beta, family, link, r = exact_case(setting, p, n, wmode)
    classes = (0, 1) if setting == "multinomial2" else (0,)
    for cls in classes:
        rc = r if cls == 0 else R.irls(X, y, w, off, beta, family, link, cls=1)
        G, dev_ = run_irls(dev, route, X, y, w, off, beta, family, link, layout, cls=cls)
        bad = np.argwhere(G != rc.G)
        assert bad.size == 0, f"{len(bad)} entries differ, first {bad[0]}: {G[tuple(bad[0])]} != {rc.G[tuple(bad[0])]}"
        if setting == "gaussian":
            assert dev_ == rc.dev
        else:
            assert abs(dev_ - rc.dev) <= 1e-12 * rc.absdev
        if setting in ("binomial", "multinomial2"):      # mu = 1/2 on every row
            wv = np.ones(n) if w is None else w
            wsum = wv[y == cls].sum() if setting == "multinomial2" else wv.sum()
            assert abs(dev_ - 2.0 * np.log(2.0) * wsum) <= 1e-12 * 2.0 * np.log(2.0) * wsum


WAVE_P = [1, 13, 14, 15, 16, 30, 31, 46, 47, 62, 63, 78, 94, 110, 111, 126]
N_ALIGNED, N_SCALAR, N_UNITS = [20, 40, 64, 100], [21, 41, 65, 101], [1000, 1025, 2049, 4093]


def _wave_exact_cases():
    out = []
    for route in ("split", "wave"):
        for i, p in enumerate(WAVE_P):
            for n in N_ALIGNED + N_SCALAR + N_UNITS:
                out.append((route, "gaussian", p, n))
            # the FAM 1 instance and the FAM 0 null model: alternate halves of the row counts,
            # all of them where a block count has a single p (94, 110)
            for ns in (N_ALIGNED, N_SCALAR, N_UNITS):
                for n in (ns if p in (94, 110) else ns[i % 2::2]):
                    out.append((route, "binomial", p, n))
                    out.append((route, "poisson", p, n))
    return out


WAVE_EXACT = _wave_exact_cases()


@gpu
@pytest.mark.parametrize("route,setting,p,n", WAVE_EXACT, ids=[f"{r}-{s}-p{p}-n{n}" for r, s, p, n in WAVE_EXACT])
def test_exact_wave_routes(cuda_dev, route, setting, p, n):
    check_exact(cuda_dev, route, setting, p, n)


VARIANTS = [(route, setting, p, n, wm)
            for route in ("split", "wave", "wg") for p in (14, 30) for n in (100, 1000)
            for setting, wms in (("gaussian", ("none", "w", "off", "w+off")), ("binomial", ("none", "w")),
                                 ("poisson", ("none", "w")))
            for wm in wms]
VARIANTS += [(route, setting, p, 1000, "zero90") for route in ("split", "wave", "wg", "wide") for p in (14, 30)
             for setting in ("gaussian", "binomial")]


@gpu
@pytest.mark.parametrize("route,setting,p,n,wmode", VARIANTS,
                         ids=[f"{r}-{s}-p{p}-n{n}-{wm}" for r, s, p, n, wm in VARIANTS])
def test_exact_prior_weight_and_offset_variants(cuda_dev, route, setting, p, n, wmode):
    """wprior = None / offset = None alias y in the LDS-DMA path; 90 % zero weights."""
    check_exact(cuda_dev, route, setting, p, n, wmode)


VIEWS = [(route, setting, p, layout) for route in ("split", "wave", "wg") for setting in ("gaussian", "binomial")
         for p in (30, 100) for layout in ("view4", "view3", "ldodd")]


@gpu
@pytest.mark.parametrize("route,setting,p,layout", VIEWS, ids=[f"{r}-{s}-p{p}-{l}" for r, s, p, l in VIEWS])
def test_exact_row_range_views(cuda_dev, route, setting, p, layout):
    """A design passed as a row-range view of a wider buffer: ld > n on the
    LDS-DMA path, a misaligned base with ld % 4 == 0 (must fall back to scalar
    loads), ld % 4 != 0.  Everything outside the view is NaN."""
    check_exact(cuda_dev, route, setting, p, 1000, "w+off", layout)


WG_EXACT = [(setting, p, n, wm) for setting in R.EXACT_SETTINGS for p in (30, 31, 62, 63, 126, 127, 254)
            for n in (1, 63, 64, 65, 4096, 4097) for wm in (("w+off", "tail0") if n in (65, 4097) else ("w+off",))]


@gpu
@pytest.mark.parametrize("setting,p,n,wmode", WG_EXACT, ids=[f"{s}-p{p}-n{n}-{wm}" for s, p, n, wm in WG_EXACT])
def test_exact_workgroup_route(cuda_dev, setting, p, n, wmode):
    check_exact(cuda_dev, "wg", setting, p, n, wmode)


@gpu
@pytest.mark.parametrize("setting", R.EXACT_SETTINGS)
@pytest.mark.parametrize("n", [100, 4096, 4097])
def test_exact_wide_route(cuda_dev, setting, n):
    """n = 4096 (n % 4 == 0 and 257^2 n >= 2^27) sends the Gram GEMM to the x3 bf16-split kernel."""
    check_exact(cuda_dev, "wide", setting, 255, n)


@gpu
@pytest.mark.parametrize("setting", ["gaussian", "binomial", "poisson"])
@pytest.mark.parametrize("n", [20, 21, 1000, 2049])
def test_exact_intercept_only(cuda_dev, setting, n):
    """p = 0 (the null-model pass) runs on the fp32 wave kernel whatever GLM_GRAM says."""
    check_exact(cuda_dev, "wave", setting, 0, n)
    check_exact(cuda_dev, "split", setting, 0, n)


def test_case_lists_reach_every_instance():
    """Every NB x load path x FAM of the split kernel, every NB x load path of
    the fp32 wave kernel, every TP of the workgroup kernel (no GPU needed)."""
    fam = {"gaussian": ("gaussian", "identity"), "binomial": ("binomial", "logit"), "poisson": ("poisson", "log")}
    seen = {instance(r, p, n, "plain", *fam[s]) for r, s, p, n in WAVE_EXACT}
    seen |= {instance(r, p, 1000, l, *fam[s]) for r, s, p, l in VIEWS}
    seen |= {instance("wg", p, n) for _, p, n, _ in WG_EXACT}
    for nb in range(1, 9):
        for vec in (True, False):
            assert ("wave", nb, vec) in seen
            for f in (0, 1):
                assert ("split", nb, vec, f) in seen
    for tp in (1, 2, 4, 8):
        assert ("wg", tp) in seen
    # every block count meets every count of full 32-row chunks (0, 1, 2, 3+) on the LDS-DMA path
    # and a multi-unit row count, for both FAM instances
    for f, s in ((0, "gaussian"), (0, "poisson"), (1, "binomial")):
        for nb in range(1, 9):
            ns = {n for r, ss, p, n in WAVE_EXACT if r == "split" and ss == s and (p + 2 + 15) // 16 == nb}
            assert set(N_ALIGNED) <= ns and set(N_SCALAR) <= ns and len(ns & set(N_UNITS)) >= 2, (s, nb, ns)


# ---------------------------------------------------------------------------
# (b) the six kept products of the bf16 split
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("place_", list(R.PIECE_PLACEMENTS))
@pytest.mark.parametrize("n", [64, 65])
def test_split_pieces_exact(cuda_dev, place_, n):
    """One live row; each designated entry is a single product with at most 24
    significant bits, and the CPU self-test shows that dropping any one of the
    six kept products (mm, lh, hl, mh, hm, hh) breaks at least one of them."""
    p, cols = R.PIECE_PLACEMENTS[place_]
    X, y, w, beta, pairs = R.piece_design(31, p, cols, n=n)
    r = R.irls(X, y, w, None, beta, "gaussian", "identity")
    ii, jj = np.array(pairs).T
    for route in ("split", "wave"):
        G, _ = run_irls(cuda_dev, route, X, y, w, None, beta, "gaussian", "identity")
        assert (G[ii, jj] == r.G[ii, jj]).all(), (route, G[ii, jj] - r.G[ii, jj])
        assert np.isfinite(G).all()


# ---------------------------------------------------------------------------
# (c) per-row family math on diagonal designs
# ---------------------------------------------------------------------------
def check_diag(G, r, p, tol=8 * EPS):
    """X = diag(c): G[j, j], G[j, p], G[j, p + 1] isolate row j; the data block
    is otherwise exactly zero; the three intercept / z entries sum all rows."""
    j = np.arange(p)
    assert (G[:p, :p][~np.eye(p, dtype=bool)] == 0).all()
    for name, got, ref in (("W c^2", G[j, j], r.G[j, j]), ("W c", G[j, p], r.G[j, p]),
                           ("W c z", G[j, p + 1], r.G[j, p + 1])):
        err = np.abs(got - ref)
        bad = np.flatnonzero(~(err <= tol * np.abs(ref)))
        assert bad.size == 0, f"{name}: row {bad[0]}: {got[bad[0]]!r} vs {ref[bad[0]]!r}"
    tail = np.abs(G[p:, p:] - r.G[p:, p:])
    assert (tail <= (p + 8) * EPS * r.absG[p:, p:]).all()
    assert (G == G.T).all()


DIAG = [(route, p) for route, ps in (("split", (30, 64)), ("wave", (30, 64)), ("wg", (30, 62)), ("wide", (255,)))
        for p in ps]


@gpu
@pytest.mark.parametrize("route,p", DIAG, ids=[f"{r}-p{p}" for r, p in DIAG])
@pytest.mark.parametrize("combo", R.COMBOS, ids=IDS)
def test_row_math_on_diagonal_designs(cuda_dev, combo, route, p):
    f, l, vp, lp = combo
    X, y, w, off, beta = R.diag_design(7 * p + 1, combo, p)
    r = R.irls(X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    R.check_unclamped(f, l, r.eta, r.mu, y, lp)
    G, d = run_irls(cuda_dev, route, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    check_diag(G, r, p)
    assert abs(d - r.dev) <= 1e-11 * r.absdev


@gpu
@pytest.mark.parametrize("route,p", [("wg", 30), ("wg", 62), ("wide", 255)])
@pytest.mark.parametrize("K", [2, 3, 16])
def test_row_math_multinomial(cuda_dev, route, p, K):
    X, y, w, _, beta = R.diag_multinomial(13 * p + K, p, K)
    for cls in range(K):
        r = R.irls(X, y, w, None, beta, "multinomial", "logit", cls=cls)
        R.check_unclamped("multinomial", "logit", r.eta, r.mu, y)
        G, d = run_irls(cuda_dev, route, X, y, w, None, beta, "multinomial", "logit", cls=cls)
        check_diag(G, r, p)
        assert abs(d - r.dev) <= 1e-11 * r.absdev


# ---------------------------------------------------------------------------
# (d) dense moderate designs, the gradient pass, the identity between them
# ---------------------------------------------------------------------------
N_DENSE = 500


@functools.lru_cache(maxsize=None)
def dense_case(ci, p):
    combo = R.COMBOS[ci]
    f, l, vp, lp = combo
    X, y, w, off, beta = R.dense_design(100 * ci + p, combo, p, N_DENSE)
    r = R.irls(X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    R.check_unclamped(f, l, r.eta, r.mu, y, lp)
    g = R.grad(X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    return X, y, w, off, beta, r, g


def check_gram(route, G, r, n):
    ratio = np.abs(G - r.G) / (EPS * np.maximum(r.absG, 1e-300))
    WORST[route] = max(WORST.get(route, 0.0), float(ratio.max()))
    print(f"{route}: max |G - Gref| / (2^-24 absG) = {ratio.max():.3f} (bound {n + 8})")
    assert (np.abs(G - r.G) <= (n + 8) * EPS * r.absG).all(), ratio.max()


def check_grad(g, ref):
    assert (np.abs(g - ref.g) <= (2 * EPS + 1e-12) * ref.absg).all(), (
        np.abs(g - ref.g) / np.maximum(ref.absg, 1e-300)).max() / EPS


@gpu
@pytest.mark.parametrize("route", ["split", "wave", "wg", "wide"])
@pytest.mark.parametrize("p", [5, 37, 100])
@pytest.mark.parametrize("ci", range(len(R.COMBOS)), ids=IDS)
def test_dense_designs(cuda_dev, ci, p, route):
    f, l, vp, lp = R.COMBOS[ci]
    X, y, w, off, beta, r, gr = dense_case(ci, p)
    G, d = run_irls(cuda_dev, route, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    check_gram(route, G, r, N_DENSE)
    assert abs(d - r.dev) <= 1e-11 * r.absdev
    # the identity X W z - X W X^T beta = -g on the GPU results themselves
    g, dg = run_grad(cuda_dev, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    b = beta[0]
    lhs = G[:p + 1, p + 1] - G[:p + 1, :p + 1] @ b
    bound = (N_DENSE + 8) * EPS * (r.absG[:p + 1, p + 1] + r.absG[:p + 1, :p + 1] @ np.abs(b)) + (
        2 * EPS + 1e-12) * gr.absg[0]
    # the oracle's own residual of the identity (fp64 rounding of its cancelling terms)
    bound += 1e-13 * (r.absG[:p + 1, p + 1] + r.absG[:p + 1, :p + 1] @ np.abs(b) + gr.absg[0])
    assert (np.abs(lhs + g[0]) <= bound).all()


@gpu
@pytest.mark.parametrize("p", [0, 5, 37, 100])
@pytest.mark.parametrize("ci", range(len(R.COMBOS)), ids=IDS)
def test_gradient_pass(cuda_dev, ci, p):
    f, l, vp, lp = R.COMBOS[ci]
    X, y, w, off, beta, r, gr = dense_case(ci, p)
    g, d = run_grad(cuda_dev, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    check_grad(g, gr)
    assert abs(d - gr.dev) <= 1e-11 * gr.absdev


@gpu
@pytest.mark.parametrize("K", [1, 2, 3, 16])
@pytest.mark.parametrize("p", [0, 5, 37])
def test_gradient_pass_multinomial(cuda_dev, K, p):
    X, y, w, _, beta = R.multinomial_design(17 * p + K, p, N_DENSE, K)
    gr = R.grad(X, y, w, None, beta, "multinomial", "logit")
    if K > 1:          # K = 1 is the degenerate p_0 = 1: zero gradient, zero deviance
        R.check_unclamped("multinomial", "logit", gr.eta, gr.mu, y)
    g, d = run_grad(cuda_dev, X, y, w, None, beta, "multinomial", "logit")
    check_grad(g, gr)
    assert abs(d - gr.dev) <= 1e-11 * gr.absdev


@gpu
def test_gradient_pass_row_splits(cuda_dev):
    """n = 70001: glm_xtr_kernel splits the rows (splits = 2) and the host sums the partials."""
    combo = R.COMBOS[3]
    f, l, vp, lp = combo
    X, y, w, off, beta = R.dense_design(99, combo, 5, 70001)
    gr = R.grad(X, y, w, off, beta, f, l)
    g, d = run_grad(cuda_dev, X, y, w, off, beta, f, l)
    check_grad(g, gr)
    assert abs(d - gr.dev) <= 1e-11 * gr.absdev


@gpu
@pytest.mark.parametrize("route", ["wg", "wide"])
@pytest.mark.parametrize("p", [5, 37, 100])
def test_dense_designs_multinomial(cuda_dev, route, p):
    K = 3
    X, y, w, _, beta = R.multinomial_design(5 * p, p, N_DENSE, K)
    for cls in range(K):
        r = R.irls(X, y, w, None, beta, "multinomial", "logit", cls=cls)
        R.check_unclamped("multinomial", "logit", r.eta, r.mu, y)
        G, d = run_irls(cuda_dev, route, X, y, w, None, beta, "multinomial", "logit", cls=cls)
        check_gram(route, G, r, N_DENSE)
        assert abs(d - r.dev) <= 1e-11 * r.absdev


# ---------------------------------------------------------------------------
# (e) floors and saturation
# ---------------------------------------------------------------------------
LOGIT_ETAS = [s * e for e in (20.0, 25.0, 30.0, 34.0, 40.0, 745.0) for s in (1.0, -1.0)]
E12 = float(np.float32(1e-12))
# name -> (combo, [(eta, y, offset)]).  Log link: the row at eta = 80 (a case of its own: its deviance would
# drown the others') carries an offset of 32, because
# z = eta - offset - 1 + y / mu and the Gram's (z, z) entry W z^2 = e^80 79^2 = 3.46e38 would leave the
# fp32 range of the slab by itself (a range limit like the weight's own at eta ~ 88; docs/ALGORITHMS.md).
# The families whose weight grows faster than mu (gaussian / log: mu^2; gaussian / inverse: eta^-4) hit
# that limit long before these rows and are not saturated here.
SATURATED = {
    "binomial": (R.COMBOS[3], [(e, y, 0.0) for e in LOGIT_ETAS for y in (0.0, 1.0)]),
    "quasibinomial": (R.COMBOS[4], [(e, y, 0.0) for e in LOGIT_ETAS for y in (0.0, 1.0)]),
    "fractionalbinomial": (R.COMBOS[5], [(e, y, 0.0) for e in LOGIT_ETAS for y in (0.0, 1.0)]),
    "poisson-log": (R.COMBOS[6], [(-745.0, 0.0, 0.0), (-745.0, 2.0, 0.0), (-80.0, 1.0, 0.0)]),
    "poisson-log-80": (R.COMBOS[6], [(80.0, 3.0, 32.0)]),
    "gamma-log": (R.COMBOS[9], [(-745.0, 1.0, 0.0), (-80.0, 1.0, 0.0), (1.0, 0.0, 0.0)]),
    "gamma-log-80": (R.COMBOS[9], [(80.0, 1.0, 32.0)]),
    "tweedie-log": (R.COMBOS[11], [(-745.0, 1.0, 0.0), (-80.0, 0.0, 0.0), (1.0, 0.0, 0.0)]),
    "tweedie-log-80": (R.COMBOS[11], [(80.0, 1.0, 32.0)]),
    "negbin-log": (R.COMBOS[15], [(-745.0, 1.0, 0.0), (-80.0, 0.0, 0.0)]),
    "negbin-log-80": (R.COMBOS[15], [(80.0, 2.0, 32.0)]),
    "gamma-inverse": (R.COMBOS[8], [(0.0, 1.0, 0.0), (E12, 1.0, 0.0), (-E12, 1.0, 0.0), (1.0, 0.0, 0.0)]),
    "tweedie-l1": (R.COMBOS[12], [(0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]),
    "tweedie-l-0.5": (R.COMBOS[13], [(0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]),
    "tweedie-l0.5": (R.COMBOS[14], [(0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]),
}


@functools.lru_cache(maxsize=None)
def saturated_case(name, p):
    """Diagonal design (c = 1) whose first rows sit at the saturated values; the
    rest are benign rows at eta = 1 (logit: 0.5)."""
    combo, rows = SATURATED[name]
    f, l, vp, lp = combo
    assert p >= len(rows)
    eta = np.full(p, 0.5 if l == "logit" else 1.0)
    y = np.ones(p)
    off = np.zeros(p)
    for i, (e, yy, o) in enumerate(rows):
        eta[i], y[i], off[i] = e, yy, o
    beta = np.zeros((1, p + 1))
    beta[0, :p] = eta - off
    X, w = np.eye(p), np.ones(p)
    r = R.irls(X, y, w, off, beta, f, l, var_power=vp, link_power=lp, floors=True)
    g = R.grad(X, y, w, off, beta, f, l, var_power=vp, link_power=lp, floors=True)
    assert np.isfinite(r.G).all() and np.isfinite(g.g).all() and np.isfinite(r.dev)
    return X, y, w, off, beta, r, g


SAT_ROUTES = [("split", 32), ("wave", 32), ("wg", 30), ("wide", 255)]


@gpu
@pytest.mark.parametrize("route,p", SAT_ROUTES, ids=[r for r, _ in SAT_ROUTES])
@pytest.mark.parametrize("name", list(SATURATED))
def test_floors_and_saturation(cuda_dev, name, route, p):
    """The floors are the contract: finite outputs, the Gram of the floored
    oracle, and the deviance of the STABLE oracle (binomial family under the
    logit link: logs from eta, floored at log(1e-15)).  Before the deviance fix
    the last assertion failed on the fp32 wave, workgroup, wide and gradient
    routes for binomial and on every route for quasi / fractionalbinomial
    (e.g. 60.00204 instead of 60.0 for the row at eta = 30, y = 0)."""
    f, l, vp, lp = SATURATED[name][0]
    X, y, w, off, beta, r, gr = saturated_case(name, p)
    G, d = run_irls(cuda_dev, route, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    assert np.isfinite(G).all() and np.isfinite(d)
    check_diag(G, r, p)
    print(f"{name} {route}: deviance {d!r}, oracle {r.dev!r}, rel {abs(d - r.dev) / r.absdev:.2e}")
    assert abs(d - r.dev) <= 1e-11 * r.absdev


@gpu
@pytest.mark.parametrize("name", list(SATURATED))
def test_floors_and_saturation_gradient(cuda_dev, name):
    f, l, vp, lp = SATURATED[name][0]
    X, y, w, off, beta, r, gr = saturated_case(name, 30)
    g, d = run_grad(cuda_dev, X, y, w, off, beta, f, l, var_power=vp, link_power=lp)
    assert np.isfinite(g).all() and np.isfinite(d)
    check_grad(g, gr)
    print(f"{name} grad: deviance {d!r}, oracle {gr.dev!r}, rel {abs(d - gr.dev) / gr.absdev:.2e}")
    assert abs(d - gr.dev) <= 1e-11 * gr.absdev
