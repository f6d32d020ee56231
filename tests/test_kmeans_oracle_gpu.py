"""One K-Means Lloyd pass of every kernel route against the float64 oracle
tests/kmref.py: kmeans_mfma_kernel and kmeans_wave_kernel (csrc/kmeans_wave.hip),
the workgroup-tile kmeans_kernel and the staged GEMM path _kmeans_large
(csrc/dense_kernels.hip).

Grid class: data on which float32 arithmetic is exact in any order (proved on
the CPU by tests/test_kmref.py), so assignment - exact ties to the lowest
index included - sums, counts and SSE must equal ``kmref.lloyd`` bit for bit.
Rounded class: Gaussian data; a row may differ from the oracle only within
``kmref.flip_bound``, and sums / counts / SSE are checked unconditionally
against ``kmref.given`` of the GPU's own assignment.

Every case names its route and the test observes it (a recording proxy around
``ops.dense.dense_lib`` and a spy on ``_kmeans_large``), so a routing change
cannot move a case onto another kernel unnoticed."""
import functools

import numpy as np
import pytest
import torch

import kmref as KR
from h2omx.ops import dense as OD

pytestmark = pytest.mark.gpu

KERNELS = {"mfma": ["h2omx_kmeans_mfma"], "wave": ["h2omx_kmeans_wave"], "tile": ["h2omx_kmeans"],
           "large": ["h2omx_kmeans", "_kmeans_large"]}    # large: the tile launcher's kBadArg, then the GEMM path
WATCHED = {"h2omx_kmeans_mfma", "h2omx_kmeans_wave", "h2omx_kmeans", "_kmeans_large"}


class _Recorder:
    """ops.dense.dense_lib() stand-in: the real library, every symbol looked up noted"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._lib, name)


@pytest.fixture
def step(cuda_dev, monkeypatch):
    """step(route, X, C, mfma=, wave=, na_free=, host_c=) -> numpy (assign, sums,
    counts, sse) of one ops.dense.kmeans_step that took ``route``; step.calls
    lists the library entry points of the last call"""
    calls: list = []
    rec = _Recorder(OD.dense_lib(), calls)
    monkeypatch.setattr(OD, "dense_lib", lambda: rec)
    large = OD._kmeans_large

    def spy(*a, **kw):
        calls.append("_kmeans_large")
        return large(*a, **kw)

    monkeypatch.setattr(OD, "_kmeans_large", spy)

    def run(route, X, C, mfma=True, wave=True, na_free=False, host_c=False):
        monkeypatch.setattr(OD, "KM_MFMA", mfma)
        monkeypatch.setattr(OD, "KM_WAVE", wave)
        del calls[:]
        Cin = np.array(C) if host_c else torch.from_numpy(np.array(C)).to(cuda_dev)
        a, s, c, e = OD.kmeans_step(torch.from_numpy(np.array(X)).to(cuda_dev), Cin, na_free=na_free)
        assert [name for name in calls if name in WATCHED] == KERNELS[route], (route, calls)
        assert a.dtype == torch.int32 and s.dtype == c.dtype == e.dtype == np.float64
        return a.cpu().numpy(), s, c, e

    run.calls = calls
    return run


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """(X, C, lloyd(X, C)) of a grid case, computed once and read-only"""
    X, C = case.data()
    ref = KR.lloyd(X, C)
    for arr in (X, C) + ref:
        arr.setflags(write=False)
    return X, C, ref


def _same(got, want, what):
    for name, g, w in zip(("assign", "sums", "counts", "sse"), got, want):
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert not len(bad), (what, name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("case", KR.GRID_TABLE + KR.ROW_EDGES, ids=repr)
def test_grid_case_is_bit_exact_on_its_route(step, case):
    """Tables: every instantiation family of each route, the shapes on both
    sides of each routing boundary, row counts 1 / 63 / 64 / 65 / 1025 (second
    workgroup) and 8200 on the tile kernel (three workgroups); 1 % NaN cells,
    the last centroid a copy of centroid 0 that must stay empty."""
    X, C, ref = _oracle(case)
    got = step(case.route, X, C, mfma=case.mfma, wave=case.wave)
    _same(got, ref, "oracle")
    if case.dup:
        assert got[2][-1] == 0
    _same(step(case.route, X, C, mfma=case.mfma, wave=case.wave), got, "second call")


@pytest.mark.parametrize("case", [c for c in KR.GRID_TABLE if c.route == "mfma"], ids=repr)
def test_mfma_entry_variants_are_bit_identical(step, case):
    """C as a host array (the model's call: tables built on the host) or a
    device tensor, na_free=True on the imputed design (the NA = false kernel
    variant) or na_free=False on the design with its NaN cells."""
    X, C, ref = _oracle(case)
    Xz = np.nan_to_num(X, nan=0.0)
    for host_c in (False, True):
        _same(step("mfma", X, C, host_c=host_c), ref, f"NaN design, host_c={host_c}")
        _same(step("mfma", Xz, C, host_c=host_c, na_free=True), ref, f"na_free, host_c={host_c}")


@pytest.mark.parametrize("case,rows", KR.CHUNKED, ids=repr)
def test_large_path_in_chunks_is_bit_identical(step, monkeypatch, case, rows):
    """_kmeans_large over several row chunks with a ragged last one (row0 of
    kmeans_stage_kernel, the per-chunk stat / sums slabs) equals the
    single-chunk run and the oracle."""
    X, C, ref = _oracle(case)
    whole = step("large", X, C)
    assert step.calls.count("h2omx_kmeans_stage") == 1
    _same(whole, ref, "one chunk")
    monkeypatch.setattr(OD, "KM_LARGE_MIN_ROWS", rows)
    monkeypatch.setattr(OD, "KM_LARGE_ELEMS", rows * max(case.d, case.k))
    parts = step("large", X, C)
    assert step.calls.count("h2omx_kmeans_stage") == -(-case.n // rows) >= 3 and case.n % rows
    _same(parts, whole, "chunked against whole")
    _same(parts, ref, "chunked against the oracle")


FLAGS = {"mfma": {}, "wave": dict(mfma=False), "tile": dict(mfma=False, wave=False)}


@pytest.mark.parametrize("d,k,routes", KR.SHARED_SHAPES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_routes_agree_bit_for_bit(step, d, k, routes):
    """shapes that more than one of the MFMA, the wave and the tile kernel accept"""
    X, C, ref = _oracle(KR.GridCase(routes[0], d, k))
    outs = {route: step(route, X, C, **FLAGS[route]) for route in routes}
    for route, got in outs.items():
        _same(got, outs[routes[0]], f"{route} against {routes[0]}")
        _same(got, ref, route)


@pytest.mark.parametrize("route,d,k,flags", KR.ROUNDED, ids=lambda v: str(v) if not isinstance(v, dict) else "")
def test_rounded_case_flips_only_within_the_bound(step, route, d, k, flags):
    """Gaussian data, NaN cells, one far-away empty cluster: at most 0.1 % of
    the rows differ from the oracle, every one of them within flip_bound;
    counts are those of the GPU's assignment; sums and SSE match the float64
    statistics of that assignment - unconditionally."""
    n = KR.ROUNDED_ROWS
    X, C = KR.rounded_case(d, k, n, seed=100 + d + k)
    a, s, c, e = step(route, X, C, **flags)
    rows, ok = KR.flips(X, C, a)
    assert len(rows) <= n // 1000, len(rows)
    assert ok.all(), (rows[~ok][:5].tolist(), len(rows))
    assert np.array_equal(c, np.bincount(a, minlength=k)) and c[-1] == 0
    sr, _, er = KR.given(X, C, a)
    np.testing.assert_allclose(s, sr, rtol=1e-4, atol=2e-3)
    np.testing.assert_allclose(e, er, rtol=1e-4)
    # _kmeans_large adds the row SSEs of a block's four waves through LDS float
    # atomics (kmeans_argmin_kernel), in no fixed order: on rounded data its SSE
    # repeats only up to that rounding, everything else bit for bit
    keep = 3 if route == "large" else 4
    _same(step(route, X, C, **flags)[:keep], (a, s, c, e)[:keep], "second call")
