"""Plain float64 reference of path-dependent TreeSHAP over a flattened path
table (``csrc/explain_kernels.hip`` tree_shap_kernel, ``explain._shap_numpy``).

The operation.  A leaf record is {first element, m, leaf value bits, tree}; its
m elements are {feature | na_ok << 30 | categorical << 29, z, lo, hi}, one per
distinct feature of the root-to-leaf path.  A row follows element j (o_j = 1,
else 0) when ``lo < x <= hi``; a NaN follows when the ``na_ok`` bit is set; a
categorical element tests level ``int(x)`` (truncation) against the 256-bit set
``sets[int(lo)]``, and a level below 0 or above 255 goes the NaN way.  z_j is
the fraction of the training cover that follows the path on feature j.  The
leaf plays the game

    val(S) = v * prod_{j in S} o_j * prod_{j not in S} z_j

over its m elements and element i's Shapley value goes to its feature.

How it is computed here, and why it shares no weakness with the code under
test: both the kernel and ``_shap_numpy`` build P(t) = prod_j (z_j + o_j t)
once and take element i out again by synthetic division, which subtracts.
:func:`leaf_phi` never divides and never subtracts: for each i it multiplies
out prod_{j != i} (z_j + o_j t) from scratch.  Every factor has non-negative
coefficients, so every product and every sum has non-negative terms and the
relative error of each coefficient c_k is at most ``(2m) 2^-53`` at any width;

    phi_i = v (o_i - z_i) sum_k w(m, k) c_k,      w(m, k) = 1 / (m C(m-1, k)),

with the weights from exact integer binomials.  :func:`exact` is the same in
rational arithmetic and :func:`brute` is the Shapley definition by subset
enumeration; tests/test_shapref.py holds the three against each other.

Nothing is imported from ``h2omx``; no HIP code is called from here.
"""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import numpy as np

FEAT_MASK = 0x1FFFFFFF
N_ROWS = 300                         # one full and one partial 256-row workgroup

WIDTHS = {8: (1, 2, 8), 16: (9, 16), 32: (17, 24, 28, 32)}          # leaf widths per MAXM bucket
REGIMES = {"balanced": (0.3, 0.7), "high_cover": (0.8, 1.0), "near_one": (0.95, 1.0)}
FEATURES = (40, 70)                  # 40 * 256 * 4 B fits the 64 KiB LDS accumulator, 70 does not

# a standard normal cell lies in each of these intervals with probability 0.93
ONE_SIDED = float(np.float32(1.4758))
TWO_SIDED = float(np.float32(1.8119))
NAN_FEATURE = 3
BASE_LEVELS = (0, 31, 32, 255)       # in every level set: first / last bit of a word, last bit of the set
OTHER_LEVELS = (3, 5, 63, 64, 100, 200, 224, 254)                   # each in a set with probability 0.8


def weights(m: int) -> np.ndarray:
    """w[k] = k! (m-1-k)! / m! = 1 / (m C(m-1, k)), 0 <= k < m"""
    return np.array([1.0 / (m * math.comb(m - 1, k)) for k in range(m)], np.float64)


def decode(E):
    """(feature [m], na_ok [m], categorical [m], z [m], lo [m], hi [m]) of elements E [m][4] float32"""
    E = np.ascontiguousarray(E, np.float32).reshape(-1, 4)
    bits = E[:, 0].copy().view(np.int32).astype(np.int64)
    return (bits & FEAT_MASK, ((bits >> 30) & 1).astype(bool), ((bits >> 29) & 1).astype(bool),
            E[:, 1].astype(np.float64), E[:, 2].astype(np.float64), E[:, 3].astype(np.float64))


def follows(X, E, sets) -> np.ndarray:
    """o [m][n] bool: row r of X [F][n] follows element j of E [m][4]"""
    X = np.asarray(X, np.float64)
    f, na_ok, cat, _, lo, hi = decode(E)
    o = np.zeros((len(f), X.shape[1]), bool)
    for j in range(len(f)):
        x = X[f[j]]
        nan = np.isnan(x)
        if cat[j]:
            level = np.trunc(np.where(nan, -1.0, x)).astype(np.int64)     # toward zero, as a C cast does
            words = [int(w) for w in sets[int(lo[j])]]
            member = [0 <= b <= 255 and bool((words[b // 32] >> (b % 32)) & 1) for b in level.tolist()]
            inside = np.where((level < 0) | (level > 255), na_ok[j], member)
        else:
            with np.errstate(invalid="ignore"):
                inside = (lo[j] < x) & (x <= hi[j])
        o[j] = np.where(nan, na_ok[j], inside)
    return o


def leaf_phi(z, o, v: float) -> np.ndarray:
    """phi [m][n] of one leaf: z [m], o [m][n] (or [m]), without division or
    subtraction.  C[i] holds the coefficients of prod_{j != i} (z_j + o_j t)."""
    z = np.asarray(z, np.float64)
    o = np.asarray(o, np.float64)
    single = o.ndim == 1
    o = o.reshape(len(z), -1)
    m, n = o.shape
    if m == 0:
        return np.zeros((0,) if single else (0, n))
    C = np.zeros((m, m, n))                                      # [i][k][row]
    C[:, 0] = 1.0
    others = ~np.eye(m, dtype=bool)
    for j in range(m):
        grown = z[j] * C
        grown[:, 1:] += o[j] * C[:, :-1]
        C = np.where(others[:, j, None, None], grown, C)         # element i skips its own factor
    w = weights(m)
    s = np.zeros((m, n))
    for k in range(m):                                           # in this order whatever the number of rows
        s += w[k] * C[:, k]
    phi = v * (o - z[:, None]) * s
    return phi[:, 0] if single else phi


def brute(z, o, v: float) -> np.ndarray:
    """phi [m] of one row by the Shapley definition (m <= 10)"""
    m = len(z)
    assert m <= 10

    def val(S):
        p = v
        for j in range(m):
            p *= o[j] if j in S else z[j]
        return p

    phi = np.zeros(m)
    for i in range(m):
        rest = [j for j in range(m) if j != i]
        for k in range(m):
            wk = math.factorial(k) * math.factorial(m - 1 - k) / math.factorial(m)
            for S in itertools.combinations(rest, k):
                phi[i] += wk * (val(set(S) | {i}) - val(set(S)))
    return phi


def exact(z, o, v: float) -> list:
    """phi [m] of one row as Fractions: leaf_phi in rational arithmetic"""
    zq = [Fraction(float(a)) for a in z]
    oq = [Fraction(int(a)) for a in o]
    m = len(zq)
    phi = []
    for i in range(m):
        c = [Fraction(1)] + [Fraction(0)] * (m - 1)
        for j in range(m):
            if j != i:
                c = [zq[j] * c[k] + (oq[j] * c[k - 1] if k else 0) for k in range(m)]
        s = sum(Fraction(1, m * math.comb(m - 1, k)) * c[k] for k in range(m))
        phi.append(Fraction(float(v)) * (oq[i] - zq[i]) * s)
    return phi


def leaf_value(vbits) -> float:
    return float(np.array([vbits], np.int32).view(np.float32)[0])


def leaf_total(z, o, v: float) -> np.ndarray:
    """sum_i phi_i = val(all) - val(none) = v (prod o - prod z), per row"""
    o = np.asarray(o, np.float64)
    return v * (np.prod(o, axis=0) - np.prod(np.asarray(z, np.float64)))


def contributions(X, lv, el, sets) -> np.ndarray:
    """phi [F][n] float64 of rows X [F][n] over the whole path table"""
    X = np.asarray(X, np.float64)
    out = np.zeros(X.shape)
    for start, m, vbits, _ in np.asarray(lv).reshape(-1, 4):
        if m == 0:
            continue
        E = el[start: start + m]
        f, _, _, z, _, _ = decode(E)
        phi = leaf_phi(z, follows(X, E, sets), leaf_value(vbits))
        for i in range(m):
            out[f[i]] += phi[i]
    return out


def totals(X, lv, el, sets) -> np.ndarray:
    """[n]: what each row's contributions add up to, from the game's two ends"""
    X = np.asarray(X, np.float64)
    out = np.zeros(X.shape[1])
    for start, m, vbits, _ in np.asarray(lv).reshape(-1, 4):
        if m == 0:
            continue
        E = el[start: start + m]
        out += leaf_total(decode(E)[3], follows(X, E, sets), leaf_value(vbits))
    return out


# ---------------------------------------------------------------------------
# The synthetic path tables
# ---------------------------------------------------------------------------
def level_set(levels) -> np.ndarray:
    st = np.zeros(8, np.uint32)
    for b in levels:
        st[b // 32] |= np.uint32(1 << (b % 32))
    return st


def tables(bucket: int, regime: str, F: int, n: int = N_ROWS) -> dict:
    """One seeded hand-made path table and the rows to score on it:
    dict(X [F][n] float32, lv [L][4] int32, el [E][4] float32, sets [S][8]
    uint32, maxm).  About 30 leaves of the widths of ``bucket`` (features
    distinct within a leaf) and one of width 0; z from ``regime``, rounded to
    float32, one in twenty exactly 1.0 and one exactly 0.0; every numeric
    element an interval that a standard normal cell meets with probability
    0.93.  Feature NAN_FEATURE is NaN in 8 % of the rows; features 1 and F - 1
    are categorical."""
    widths = WIDTHS[bucket]
    a, b = REGIMES[regime]
    rng = np.random.default_rng(1000 * bucket + 10 * F + list(REGIMES).index(regime))
    cats = (1, F - 1)
    special = [NAN_FEATURE, *cats]
    ms = [widths[i % len(widths)] for i in range(30)]
    lv, el, sets = [], [], []
    zero_leaf = next(i for i, m in enumerate(ms) if m == max(widths))
    for li, m in enumerate(ms):
        if m >= 3 and (li < len(widths) or rng.random() < 0.5):      # the special features, and the rest at random
            rest = [f for f in range(F) if f not in special]
            feats = special + list(rng.choice(rest, m - 3, replace=False))
            feats = [feats[p] for p in rng.permutation(m)]
        else:
            feats = list(rng.choice(F, m, replace=False))
        v = np.float32(rng.normal())
        lv.append((len(el), m, int(np.array([v]).view(np.int32)[0]), 0))
        for pos, f in enumerate(feats):
            na_ok = int(rng.random() < 0.5)
            z = np.float32(rng.uniform(a, b))
            if rng.random() < 0.05:
                z = np.float32(1.0)
            if li == zero_leaf and pos == m // 2:
                z = np.float32(0.0)
            if f in cats:
                levels = list(BASE_LEVELS) + [c for c in OTHER_LEVELS if rng.random() < 0.8]
                bits = int(f) | (na_ok << 30) | (1 << 29)
                el.append((bits, z, np.float32(len(sets)), np.float32(0.0)))
                sets.append(level_set(levels))
            else:
                kind = rng.integers(3)
                lo, hi = ((-np.inf, ONE_SIDED), (-ONE_SIDED, np.inf), (-TWO_SIDED, TWO_SIDED))[kind]
                el.append((int(f) | (na_ok << 30), z, np.float32(lo), np.float32(hi)))
    lv.insert(len(lv) // 2, (len(el), 0, int(np.array([np.float32(0.75)]).view(np.int32)[0]), 0))   # a stump's leaf
    lv = np.asarray(lv, np.int32).reshape(-1, 4)
    E = np.zeros((len(el), 4), np.float32)
    E[:, 0] = np.asarray([e[0] for e in el], np.int32).view(np.float32)
    E[:, 1:] = np.asarray([e[1:] for e in el], np.float32)
    X = rng.normal(size=(F, N_ROWS)).astype(np.float32)
    X[NAN_FEATURE, rng.random(N_ROWS) < 0.08] = np.nan
    X[NAN_FEATURE, 0] = np.nan                                     # the n = 1 call sees a NaN too
    edges = np.float32([ONE_SIDED, -ONE_SIDED, TWO_SIDED, -TWO_SIDED])
    for f in range(F):                                             # cells exactly on an interval's end
        if f not in special:
            X[f, rng.integers(4, N_ROWS, 4)] = edges
    for f in cats:
        base = rng.choice(BASE_LEVELS, N_ROWS)
        other = rng.choice(OTHER_LEVELS, N_ROWS)
        X[f] = np.where(rng.random(N_ROWS) < 0.6, base, other).astype(np.float32)
    # levels at the set's last bit, past it, below it, and a non-integral one (3.7 is level 3, not 4)
    X[cats[0], :4] = (255.0, -1.0, 3.7, 256.0)
    X[cats[1], :4] = (256.0, 3.7, 255.0, -1.0)
    X[cats[0], 4] = np.nan
    return dict(X=np.ascontiguousarray(X[:, :n]), lv=lv, el=E, sets=np.asarray(sets, np.uint32).reshape(-1, 8),
                maxm=int(lv[:, 1].max()))


def table_ids():
    return [(bucket, regime, F) for bucket in WIDTHS for regime in REGIMES for F in FEATURES]


_REF = {}


def reference(bucket: int, regime: str, F: int):
    """(table, phi [F][n] float64, totals [n]) of one table, computed once and read-only"""
    key = (bucket, regime, F)
    if key not in _REF:
        t = tables(bucket, regime, F)
        phi = contributions(t["X"], t["lv"], t["el"], t["sets"])
        tot = totals(t["X"], t["lv"], t["el"], t["sets"])
        for arr in (phi, tot, *[v for v in t.values() if isinstance(v, np.ndarray)]):
            arr.setflags(write=False)
        _REF[key] = (t, phi, tot)
    return _REF[key]
