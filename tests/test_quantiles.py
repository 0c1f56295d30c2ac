"""Ensemble quantiles on the device: umpcBatchEnsembleQuantiles turns a step history and its reference into the order
statistics of a term over the robots of each group, per step; umpcBatchScoreQuantiles does the same once over a per-robot
score. The answer is an element of the cell (nearest rank), so wherever the terms are exact the comparison is bit for bit.
CPU: the numpy mirrors (robobee3d_amd/score.py) by hand, against ensemble_reference and against sorted(), exports, refusals
without a handle, the resource record of the build.
GPU: exact integer tables on both sides of the 64-member switch and at the sizes of the block path, the noise tables of
test_score within the rounding of one term, the ensemble kernel's own minimum and maximum, independence of a row from
everything but its member set, a score's quantiles, one end-to-end sweep, refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_ensemble import G_, SIZES, TAULIM, _ensemble, _groups, _index
from test_score import B_, COUNT, FIRST, INF_AT, NAN_AT, REF_FIRST, STEP0, TOL, U, _dev, _mpc, _rel, _score, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
TERMS = {"ep": 0, "es": 1, "tau": 2}


def _same(a, b):
    """equal as doubles, a NaN equal to a NaN"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _exact_tables(dtype, B, steps, seed, extra=()):
    """p = (x, 0, 0) against a reference at the origin, s = sdes = e3: e_p = x^2 with x drawn from a pool of 12 integers in
    [0, 2047] (0 and 2047 among them: many duplicates), exact in fp32 and fp64 with or without contraction. `extra`:
    (step, robot, (px, py)) entries written afterwards. Returns state [steps + 1, 18, B], the constant reference [9, B]."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([[0, 2047], rng.integers(1, 2047, 10)]).astype(np.float64)
    state = np.zeros((steps + 1, 18, B))
    state[:, 0] = rng.choice(pool, size=(steps + 1, B))
    state[:, 11] = 1.0
    for i, b, (px, py) in extra:
        state[i, 0, b], state[i, 1, b] = px, py
    assert (state[:steps, 0] == 0).any()
    ref = np.zeros((9, B))
    ref[8] = 1.0
    return state.astype(dtype), ref.astype(dtype)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_quantile_mirror_semantics_by_hand():
    """9 robots, 3 steps: group 0 = robots 0..7, group 1 empty, group 2 = robot 8; p = (x, 0, 0) against the origin: e_p = x^2"""
    from robobee3d_amd import score as S
    x = np.array([[3.0, 1.0, 2.0, 1.0, 0.0, 2.0, 1.0, 5.0, 4.0],          # duplicates; n = 8
                  [3.0, np.nan, 2.0, 1.0, 0.0, 2.0, 1.0, 5.0, np.inf],    # a NaN member: n = 7; the singleton not finite: n = 0
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]])
    state = np.zeros((4, 18, 9))
    state[:3, 0] = x
    state[:, 11] = 1.0
    ref = np.zeros((9, 9))
    ref[8] = 1.0
    order, offset = S.group_index_reference(np.array([0] * 8 + [2], np.int32), 3)
    probs = (0.0, 0.25, 0.5, 1.0, 0.126, 0.125)
    q = S.ensemble_quantiles_reference(state, None, ref, 0, 3, 0, False, 3.5, order, offset, probs)
    assert q.shape == (3, 3, 8) and (S.Q_N, S.Q_SKIPPED, S.Q_FIRST) == (0, 1, 2)
    # step 0, sorted e_p = 0 1 1 1 4 4 9 25: p = 0.25 and 0.125 land on integers (k = 2 - 1, 1 - 1), 0.126 just above (k = 1)
    assert q[0, 0].tolist() == [8, 0, 0.0, 1.0, 1.0, 25.0, 1.0, 0.0]
    # step 1, n = 7: 0 1 1 4 4 9 25: ceil(1.75) - 1 = 1, ceil(3.5) - 1 = 3, ceil(0.882) - 1 = 0
    assert q[1, 0].tolist() == [7, 1, 0.0, 1.0, 4.0, 25.0, 0.0, 0.0]
    assert q[2, 0].tolist() == [8, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    for i in range(3):                                                  # the empty group: nothing scored, nothing skipped, NaN
        assert q[i, 1, :2].tolist() == [0, 0] and np.isnan(q[i, 1, 2:]).all()
    assert q[0, 2].tolist() == [1, 0] + [16.0] * 6                      # a singleton is every quantile
    assert q[1, 2, :2].tolist() == [0, 1] and np.isnan(q[1, 2, 2:]).all()
    assert q[2, 2].tolist() == [1, 0] + [4.0] * 6
    # the rank expression itself
    assert [S.quantile_rank(p, 8) for p in (0.0, 0.125, 0.25, 0.5, 0.51, 1.0)] == [0, 0, 1, 3, 4, 7]
    assert [S.quantile_rank(p, 1) for p in (0.0, 0.5, 1.0)] == [0, 0, 0] and S.quantile_rank(0.5, 7) == 3
    # the other terms: e_s = |s - sdes|^2 and the moments (3, 4) clipped at 3.5 -> 9 + 12.25; a non-finite moment skips
    state[0, 9, 2] = 2.0
    out = np.zeros((3, 9, 9))
    out[:, 1], out[:, 2] = 3.0, 4.0
    out[0, 2, 1] = np.inf
    es = S.ensemble_quantiles_reference(state, None, ref, 0, 1, 0, False, 3.5, order, offset, (0.5, 1.0), term=S.TERM_ES)
    assert es[0, 0].tolist() == [8, 0, 0.0, 4.0]
    tau = S.ensemble_quantiles_reference(state, out, ref, 0, 1, 0, False, 3.5, order, offset, (0.0, 1.0), term=S.TERM_TAU)
    assert tau[0, 0].tolist() == [7, 1, 21.25, 21.25]
    ep = S.ensemble_quantiles_reference(state, out, ref, 0, 1, 0, False, 3.5, order, offset, (0.0, 1.0))
    assert ep[0, 0].tolist() == [7, 1, 0.0, 25.0]                        # out enters the finiteness test whatever the term
    # after = 1 on the table moved by one slice, a table of references, count = 0, refusals
    tab = np.repeat(ref[None], 5, 0)
    assert _same(S.ensemble_quantiles_reference(state, None, tab, 0, 2, 2, True, 3.5, order, offset, probs), q[1:3])
    assert S.ensemble_quantiles_reference(state, None, ref, 1, 0, 0, False, 3.5, order, offset, probs).shape == (0, 3, 8)
    for bad in (dict(probs=()), dict(probs=(0.5,) * 9), dict(probs=(1.5,)), dict(probs=(-0.1,)), dict(probs=(np.nan,)),
                dict(term=3), dict(term=S.TERM_TAU), dict(count=-1), dict(first=-1), dict(ref_first=-1)):
        kw = dict(first=0, count=3, ref_first=0, after=False, taulim=3.5, order=order, offset=offset, probs=probs)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.ensemble_quantiles_reference(state, None, ref, **kw)


def test_extreme_probabilities_are_the_ensemble_mirrors_envelope():
    """on the tables of test_ensemble: p = 0 and p = 1 are ensemble_reference rows 5 and 4 where row 0 > 0, rows 0 and 1 are
    its rows 0 and 1 -- all exact"""
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.float64)
    for layout in ("contiguous", "permuted"):
        order, offset = S.group_index_reference(_groups(layout), G_)
        for after in (0, 1):
            for with_out in (True, False):
                o = out if with_out else None
                ens = S.ensemble_reference(state, o, status, ref, FIRST, COUNT, REF_FIRST, TOL, after, TAULIM, order, offset)
                q = S.ensemble_quantiles_reference(state, o, ref, FIRST, COUNT, REF_FIRST, after, TAULIM, order, offset, (0.0, 1.0))
                assert np.array_equal(q[..., 0], ens[..., S.E_N]) and np.array_equal(q[..., 1], ens[..., S.E_SKIPPED])
                some = ens[..., S.E_N] > 0
                assert np.array_equal(q[..., 2][some], ens[..., S.E_MIN_EP][some])
                assert np.array_equal(q[..., 3][some], ens[..., S.E_MAX_EP][some])
                assert np.isnan(q[..., 2:][~some]).all() and (~some).sum() >= COUNT
                if with_out:
                    t = S.ensemble_quantiles_reference(state, o, ref, FIRST, COUNT, REF_FIRST, after, TAULIM, order, offset, (1.0,),
                                                       term=S.TERM_TAU)
                    assert np.array_equal(t[..., 2][some], ens[..., S.E_MAX_TAU2][some])


def test_score_quantiles_reference_against_sorted():
    from robobee3d_amd import score as S
    rng = np.random.default_rng(11)
    B = 150
    sc = S.score_identity(B)
    sc[S.STEPS] = rng.integers(0, 5, B)
    sc[S.SUM_EP] = rng.integers(0, 9, B) * 0.5
    sc[S.MAX_EP] = rng.normal(size=B)
    sc[S.FIRST_OVER] = np.where(rng.random(B) < 0.5, -1.0, rng.integers(0, 30, B))
    sc[S.LAST_OVER] = np.where(sc[S.FIRST_OVER] < 0, -1.0, sc[S.FIRST_OVER] + 3)
    assert (sc[S.STEPS] == 0).any() and (sc[S.FIRST_OVER] == -1).any()
    group = rng.integers(-1, 4, B).astype(np.int32)
    order, offset = S.group_index_reference(group, 5)                      # group 4 stays empty
    for num, den in ((S.SUM_EP, S.STEPS), (S.MAX_EP, None), (S.FIRST_OVER, -1), (S.SUM_EP, S.SUM_EP)):
        q = S.score_quantiles_reference(sc, order, offset, PROBS, num, den)
        assert q.shape == (5, 9)
        for g in range(5):
            robots = [b for b in range(B) if group[b] == g]
            with np.errstate(invalid="ignore", divide="ignore"):
                vals = [(sc[num, b] / sc[den, b]) if den not in (None, -1) else sc[num, b] for b in robots if sc[S.STEPS, b] > 0]
            vals = sorted(v for v in vals if np.isfinite(v))
            assert q[g, 0] == len(vals) and q[g, 1] == len(robots) - len(vals)
            for j, p in enumerate(PROBS):
                want = vals[min(len(vals) - 1, max(0, int(np.ceil(p * len(vals))) - 1))] if vals else np.nan
                assert _same(q[g, 2 + j], want), (num, den, g, p)
    assert (S.score_quantiles_reference(sc, order, offset, (0.0,), S.FIRST_OVER)[:4, 2] == -1).all()      # negative values
    assert np.isnan(S.score_quantiles_reference(sc, order, offset, (0.5,), S.SUM_EP, S.SUM_EP)[4, 2])
    for bad in (dict(num=12), dict(num=-1), dict(den=12), dict(den=-2), dict(probs=())):
        kw = dict(probs=PROBS, num=1, den=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.score_quantiles_reference(sc, order, offset, **kw)


def test_quantile_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    decls = ("#define UMPC_QUANT_MAX_PROBS 8", "#define UMPC_TERM_EP 0 /* e_p = |p - pdes|^2 */",
             "#define UMPC_TERM_ES 1 /* e_s = |s - sdes|^2 */",
             "#define UMPC_TERM_TAU 2 /* tau1^2 + tau2^2, clipped at +-taulim; needs out_hist */",
             "int umpcBatchEnsembleQuantiles(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *ref_tab, "
             "const void *ref, long long first, long long count, long long ref_first, int after, "
             "const int32_t *order, const int32_t *offset, int G, int term, const double *probs, "
             "int nq, double *quant, void *stream);",
             "int umpcBatchScoreQuantiles(umpc_batch_t *h, const void *score, int num, int den, const int32_t *order, "
             "const int32_t *offset, int G, const double *probs, int nq, double *quant, void *stream);")
    at = [flat.index(d) for d in decls]
    assert at == sorted(at)
    assert flat.index("int umpcBatchEnsemble(") < at[0] and at[-1] < flat.index("int umpcBatchSetStepKernel")
    assert (_lib.QUANT_MAX_PROBS, _lib.TERM_EP, _lib.TERM_ES, _lib.TERM_TAU) == (8, 0, 1, 2)
    assert (S.QUANT_MAX_PROBS, S.TERM_EP, S.TERM_ES, S.TERM_TAU) == (8, 0, 1, 2) and S.TERM_NAMES == ("ep", "es", "tau")
    L = _lib.lib()
    for sym in ("umpcBatchEnsembleQuantiles", "umpcBatchScoreQuantiles"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    dp = C.POINTER(C.c_double)
    assert L.umpcBatchEnsembleQuantiles.argtypes == [C.c_void_p] * 5 + [C.c_longlong] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                                                         C.c_int, dp, C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchScoreQuantiles.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, dp,
                                                  C.c_int, C.c_void_p, C.c_void_p]
    # argument checks come before any HIP call: no device needed
    p = (C.c_double * 2)(0.5, 1.0)
    assert L.umpcBatchEnsembleQuantiles(None, None, None, None, None, 0, 1, 0, 0, None, None, 1, 0, p, 2, None, None) == -1
    assert b"umpcBatchEnsembleQuantiles" in L.umpcLastError()
    assert L.umpcBatchScoreQuantiles(None, None, 1, 0, None, None, 1, p, 2, None, None) == -1
    assert b"umpcBatchScoreQuantiles" in L.umpcLastError()


def test_quantile_kernels_use_no_scratch():
    """the resource remarks of the build: every form of the three quantile kernels has no private frame, and the block
    kernels have the one static LDS block"""
    import json
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    for pat, n, lds in (("umpc_ens_quantile_kernel", 20, 0), ("umpc_ens_quantile_block_kernel", 20, 8360),
                        ("umpc_score_quantile_kernel", 2, 8360)):
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == lds, (k, res[k])
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds}
        with pytest.raises(RuntimeError, match=pat):
            _lib._validate_resources(dict(res, **{"a_form_of_%s_with_a_frame" % pat: {"ScratchSize": 8, "LDS": lds}}))
    assert len([k for k in limits if "quantile" in k and "boot" not in k]) == 3


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _quant(m, state, out, reftab, ref, first, count, ref_first, after, index, term, probs, quant=None):
    """umpcBatchEnsembleQuantiles on device tensors through the C ABI; a fresh `quant` is filled with NaN first: a row the
    call did not write shows (rows 0 and 1 are never NaN)"""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    if quant is None:
        quant = torch.full((count, G, 2 + len(probs)), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchEnsembleQuantiles(m.h, _ptr(state), _ptr(out), _ptr(reftab), _ptr(ref), first, count, ref_first, int(after),
                                        _ptr(order), _ptr(offset), G, TERMS[term], (C.c_double * len(probs))(*probs), len(probs),
                                        _ptr(quant), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return quant


def _score_quant(m, score, num, den, index, probs):
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    quant = torch.full((G, 2 + len(probs)), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchScoreQuantiles(m.h, _ptr(score), num, den, _ptr(order), _ptr(offset), G, (C.c_double * len(probs))(*probs),
                                     len(probs), _ptr(quant), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return quant


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


def _device_alone(m, state, out, reftab, ref, first, count, ref_first, after, index, tag):
    """p = 0 and p = 1 of e_p against rows 5 and 4 of umpcBatchEnsemble on the same arguments, rows 0 and 1 against its rows 0
    and 1: bit for bit, both from the same score_terms"""
    import torch
    q = _quant(m, state, out, reftab, ref, first, count, ref_first, after, index, "ep", (0.0, 1.0))
    ens = _ensemble(m, state, out, None, reftab, ref, first, count, ref_first, 1.0, after, index)
    assert torch.equal(q[..., 0], ens[..., 0]) and torch.equal(q[..., 1], ens[..., 1]), tag
    some = ens[..., 0] > 0
    assert torch.equal(q[..., 2][some], ens[..., 5][some]) and torch.equal(q[..., 3][some], ens[..., 4][some]), tag
    assert torch.isnan(q[..., 2:][~some]).all(), tag
    if out is not None:
        t = _quant(m, state, out, reftab, ref, first, count, ref_first, after, index, "tau", (1.0,))
        assert torch.equal(t[..., 2][some], ens[..., 9][some]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_exact_tables_bit_for_bit(dtype):
    """B = 200 as groups of 64, 1, 0, 65, 63 and 5 (both sides of the switch at 64), contiguous and permuted, 7 steps of
    integer positions: the kernel's rows are the mirror's rows"""
    from robobee3d_amd import score as S
    steps = 7
    state, ref = _exact_tables(np.dtype(dtype), B_, steps, 3, extra=[(2, 9, (np.nan, 0.0))])
    m = _mpc(B_, dtype)
    dstate, dref = _dev(m, state), _dev(m, ref)
    for layout in ("contiguous", "permuted"):
        ids = _groups(layout)
        order, offset = S.group_index_reference(ids, G_)
        index = _index(m, ids, G_)
        for after in (0, 1):
            for probs in (PROBS, (0.3,)):
                got = _quant(m, dstate, None, None, dref, 0, steps - after, 0, after, index, "ep", probs).cpu().numpy()
                want = S.ensemble_quantiles_reference(state, None, ref, 0, steps - after, 0, after, TAULIM, order, offset, probs)
                assert _same(got, want), (layout, after, probs, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
                assert (want[..., 0] == 0).sum() >= steps - after and want[..., 1].sum() == int(0 <= ids[9] < G_)
            _device_alone(m, dstate, None, None, dref, 0, steps - after, 0, after, index, (layout, after))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_block_path_sizes_bit_for_bit(dtype):
    """B = 1 400 as groups of 257, 256, 700, 65 and 122: the block's thread count on both sides, several trips per thread, the
    first size above a wavefront; fp64 adds e_p = 2^52, 2^52 + 1 and (2^26 + 1)^2 (keys apart in the lowest digits only)
    beside 0 (apart in the highest)"""
    from robobee3d_amd import score as S
    sizes, steps, B = (257, 256, 700, 65, 122), 3, 1400
    big = 2.0 ** 26
    extra = [(i, b, v) for i in range(steps) for b, v in ((3, (big, 0.0)), (4, (big, 1.0)), (5, (big + 1, 0.0)), (6, (big, 1.0)),
                                                         (300, (big, 1.0)), (301, (big, 0.0)), (600, (big, 0.0)), (601, (0.0, 0.0)))] \
        if dtype == "float64" else []
    state, ref = _exact_tables(np.dtype(dtype), B, steps, 5, extra=extra + [(1, 700, (np.inf, 0.0))])
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(sizes)])
    assert ids.shape == (B,)
    m = _mpc(B, dtype)
    dstate, dref = _dev(m, state), _dev(m, ref)
    for layout in ("contiguous", "permuted"):
        if layout == "permuted":
            ids = ids[np.random.default_rng(9).permutation(B)]
        order, offset = S.group_index_reference(ids, len(sizes))
        index = _index(m, ids, len(sizes))
        top = (253.5 / 257, 254.5 / 257, 255.5 / 257, 1.0)                  # ranks 253 .. 256 of the group of 257
        for probs in (PROBS, (0.999,), top):
            got = _quant(m, dstate, None, None, dref, 0, steps, 0, 0, index, "ep", probs).cpu().numpy()
            want = S.ensemble_quantiles_reference(state, None, ref, 0, steps, 0, 0, TAULIM, order, offset, probs)
            assert _same(got, want), (layout, probs, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
            assert want[..., 1].sum() == 1
        if dtype == "float64" and layout == "contiguous":
            assert want[0, 0].tolist() == [257, 0, big * big, big * big + 1, big * big + 1, (big + 1) ** 2]
        _device_alone(m, dstate, None, None, dref, 0, steps, 0, 0, index, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_noise_tables_within_the_rounding_of_a_term(dtype, margin):
    """the tables of test_score with their planted NaN and inf: both layouts x after 0 / 1 x table / constant reference x with /
    without out_hist x all terms. Rows 0 and 1 exact; an order statistic is monotone in every member, so it inherits the
    bound of one term (six roundings: 8 u relative) with no condition on ties"""
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    taulim = float(m.prm.taulim)
    d = [_dev(m, a) for a in (state, out, ref)]
    cref = np.ascontiguousarray(ref[REF_FIRST])
    dcref = _dev(m, cref)
    inside = lambda ids, b: int(0 <= ids[b] < G_)
    for layout in ("contiguous", "permuted"):
        ids = _groups(layout)
        order, offset = S.group_index_reference(ids, G_)
        index = _index(m, ids, G_)
        for after in (0, 1):
            for table in (True, False):
                for with_out in (True, False):
                    args = (d[0], d[1] if with_out else None, d[2] if table else None, None if table else dcref, FIRST, COUNT,
                            REF_FIRST if table else 0, after, index)
                    worst = 0.0
                    for term in ("ep", "es", "tau") if with_out else ("ep", "es"):
                        got = _quant(m, *args, term, PROBS).cpu().numpy()
                        want = S.ensemble_quantiles_reference(state, out if with_out else None, ref if table else cref, FIRST, COUNT,
                                                              REF_FIRST if table else 0, after, taulim, order, offset, PROBS,
                                                              term=TERMS[term])
                        assert np.array_equal(got[..., :2], want[..., :2]), (layout, after, table, with_out, term)
                        some = want[..., 0] > 0
                        assert np.isnan(got[..., 2:][~some]).all() and not np.isnan(got[..., 2:][some]).any()
                        worst = max(worst, _rel(got[..., 2:][some], want[..., 2:][some]))
                        assert want[..., 1].sum() == inside(ids, NAN_AT[2]) + (inside(ids, INF_AT[2]) if with_out else 0)
                    margin("%s after%d %s%s quantile rows rel" % (layout[:4], after, "tab" if table else "const", "" if with_out else " -out"),
                           worst, 8 * U[dtype])
                    _device_alone(m, *args, (layout, after, table, with_out))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_quantile_row_depends_on_its_member_set_alone(dtype):
    """the same bits: run to run, with the other groups' ids changed, with another G, with the step range cut into two calls
    that write slices of one table; count = 0 writes nothing"""
    import torch
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    d = [_dev(m, a) for a in (state, out, ref)]
    ids = _groups("contiguous")
    index = _index(m, ids, G_)
    one = _quant(m, d[0], d[1], d[2], None, FIRST, COUNT, REF_FIRST, 1, index, "ep", PROBS)
    assert not torch.isnan(one[..., :2]).any() and not torch.isnan(one[:, 0]).any()
    assert torch.equal(_bits(one), _bits(_quant(m, d[0], d[1], d[2], None, FIRST, COUNT, REF_FIRST, 1, index, "ep", PROBS)))
    two = torch.full_like(one, float("nan"))
    _quant(m, d[0], d[1], d[2], None, FIRST, 20, REF_FIRST, 1, index, "ep", PROBS, quant=two[:20])
    _quant(m, d[0], d[1], d[2], None, FIRST + 20, 17, REF_FIRST + 20, 1, index, "ep", PROBS, quant=two[20:])
    assert torch.equal(_bits(one), _bits(two))
    keep = two.clone()
    _quant(m, d[0], d[1], d[2], None, FIRST, 0, REF_FIRST, 1, index, "ep", PROBS, quant=two)
    torch.cuda.synchronize()
    assert torch.equal(_bits(two), _bits(keep))
    # groups 3 (65 members: the block path) and 4 (63: a wavefront) alone, the others' robots relabelled, G = 5 and 9
    for G, relabel in ((5, lambda g: np.where((g == 3) | (g == 4), g, (g + 1) % 3)), (9, lambda g: np.where((g == 3) | (g == 4), g, 8 - g % 3))):
        other = _quant(m, d[0], d[1], d[2], None, FIRST, COUNT, REF_FIRST, 1, _index(m, relabel(ids).astype(np.int32), G), "ep", PROBS)
        assert tuple(other.shape) == (COUNT, G, 9)
        for g in (3, 4):
            assert torch.equal(one[:, g], other[:, g]), (G, g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_score_quantiles_bit_for_bit(dtype):
    """a score from umpcBatchScore on the noise tables; per-robot mean e_p (row 1 / row 0), max e_p (row 2) and the first step
    outside the tube (row 9, -1 where none): every operation is an IEEE double operation on both sides"""
    import torch
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    d = [_dev(m, a) for a in (state, out, status, ref)]
    # (a tube of 4 instead of TOL = 2: a dozen robots never leave it in 37 steps, so row 9 holds -1 beside step numbers)
    score = _score(m, d[0], d[1], d[2], d[3], None, FIRST, COUNT, REF_FIRST, STEP0, 4.0, 1)
    # robot 20 scored nothing: it is a member that does not enter
    score[:, 20] = torch.as_tensor(S.score_identity(1)[:, 0]).to(score)
    sc = score.cpu().numpy()
    rest = np.arange(B_) != 20
    assert (sc[S.FIRST_OVER][rest] == -1).sum() >= 5 and (sc[S.FIRST_OVER][rest] >= 0).sum() >= 100
    for layout in ("contiguous", "permuted"):
        ids = _groups(layout)
        order, offset = S.group_index_reference(ids, G_)
        index = _index(m, ids, G_)
        for num, den in ((1, 0), (2, -1), (9, -1)):
            for probs in (PROBS, (0.5,)):
                got = _score_quant(m, score, num, den, index, probs)
                want = S.score_quantiles_reference(sc, order, offset, probs, num, den)
                assert _same(got.cpu().numpy(), want), (layout, num, den, probs)
                assert want[..., 1].sum() == int(0 <= ids[20] < G_) and np.isnan(want[2, 2:]).all()
                q = m.score_quantiles(score, index, probs, num, None if den < 0 else den)
                assert torch.equal(_bits(q), _bits(got))


@pytest.mark.gpu
def test_end_to_end_sweep_has_a_median_its_pushed_draw_does_not_own(margin):
    """B = 256 as 4 cells of 64 draws, 8 steps, one draw per cell pushed after step 2 (fp32): ensemble_quantiles and
    score_quantiles against the mirrors on the recorded history; where the pushed draw is the cell's maximum the median
    stays below it"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, push = 256, 8, 2
    m = _mpc(B, "float32")
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    m.record_history(K, status=True)
    pushed = [5, 64 + 17, 128 + 63, 192]
    m.set_impulses(m.impulse_table(K, [(push, pushed, (0, 4, 0, 0, 0, 0))]))
    m.rollout(K)
    cell = (np.arange(B) // 64).astype(np.int32)
    index = m.group_index(cell, 4)
    order, offset = S.group_index_reference(cell, 4)
    h = m.history()
    state, out, cref = h["state"].cpu().numpy(), h["out"].cpu().numpy(), m.ref.cpu().numpy()
    taulim = float(m.prm.taulim)
    probs = (0.05, 0.5, 0.95, 1.0)
    for term in S.TERM_NAMES:
        got = m.ensemble_quantiles(index, probs, term=term, after=True)
        assert got.dtype == torch.float64 and tuple(got.shape) == (K, 4, 6)
        want = S.ensemble_quantiles_reference(state, out, cref, 0, K, 0, True, taulim, order, offset, probs, term=S.TERM_NAMES.index(term))
        got = got.cpu().numpy()
        assert np.array_equal(got[..., :2], want[..., :2]) and np.all(want[..., 0] == 64)
        margin("end to end %s quantile rows rel" % term, _rel(got[..., 2:], want[..., 2:]), 8 * U["float32"])
    ep = m.ensemble_quantiles(index, probs, after=True)
    ens = m.ensemble(index, after=True)
    assert torch.equal(ep[..., 5], ens[..., S.E_MAX_EP])
    owns = torch.as_tensor(pushed, dtype=torch.float64, device=m.device)[None] == ens[..., S.E_ARGMAX_EP]
    print("steps x cells where the pushed draw is the maximum:\n", owns.cpu().numpy().astype(int))
    assert owns[K - 1].all() and torch.all(ep[..., 3][owns] < ep[..., 5][owns])
    # chunks into one table through `out`, the checks of the wrapper
    both = torch.empty_like(ep)
    m.ensemble_quantiles(index, probs, first=0, count=3, after=True, out=both[:3])
    m.ensemble_quantiles(index, probs, first=3, after=True, out=both[3:])
    assert torch.equal(both, ep)
    for bad in (dict(probs=()), dict(probs=(1.1,)), dict(probs=(0.5,) * 9), dict(term="p2"), dict(count=K + 1),
                dict(out=torch.empty((K, 4, 5), dtype=torch.float64, device=m.device))):
        with pytest.raises(ValueError):
            m.ensemble_quantiles(index, **dict(dict(probs=probs), **bad))
    # the median cost of a cell: the per-robot mean e_p, which the pushed draw's does not own
    sc = m.score(after=True)
    q = m.score_quantiles(sc, index, (0.5, 1.0), S.SUM_EP, S.STEPS)
    assert _same(q.cpu().numpy(), S.score_quantiles_reference(sc.cpu().numpy(), order, offset, (0.5, 1.0), S.SUM_EP, S.STEPS))
    assert torch.all(q[:, 0] == 64) and torch.all(q[:, 2] < q[:, 3])
    with pytest.raises(ValueError):
        m.score_quantiles(sc[:, :-1], index, (0.5,), 1)


@pytest.mark.gpu
def test_quantile_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((4, 18, 64), device=m.device)
    out = torch.zeros((3, 9, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((3, 9, 64), device=m.device)
    score = torch.ones((12, 64), device=m.device)
    order = torch.arange(64, dtype=torch.int32, device=m.device)
    offset = torch.tensor([0, 64], dtype=torch.int32, device=m.device)
    quant = torch.full((3, 1, 4), 3.0, dtype=torch.float64, device=m.device)
    keep = quant.clone()
    arr = lambda *p: (C.c_double * len(p))(*p)
    ok = dict(state=P(state), out=None, tab=None, ref=P(ref), first=0, count=3, ref_first=0, order=P(order), offset=P(offset), G=1,
              term=0, probs=arr(0.5, 1.0), nq=2, quant=P(quant))
    for bad in (dict(state=None), dict(order=None), dict(offset=None), dict(probs=None), dict(quant=None), dict(tab=P(tab)),
                dict(ref=None), dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(count=1 << 31), dict(G=0), dict(G=-3),
                dict(nq=0), dict(nq=9, probs=arr(*[0.5] * 9)), dict(probs=arr(0.5, 1.5)), dict(probs=arr(-0.25, 1.0)),
                dict(probs=arr(0.5, float("nan"))), dict(term=-1), dict(term=3), dict(term=2)):
        a = dict(ok, **bad)
        rc = L.umpcBatchEnsembleQuantiles(h, a["state"], a["out"], a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], 0,
                                          a["order"], a["offset"], a["G"], a["term"], a["probs"], a["nq"], a["quant"], s)
        assert rc == -1 and b"umpcBatchEnsembleQuantiles" in L.umpcLastError(), bad
    oks = dict(score=P(score), num=1, den=0, order=P(order), offset=P(offset), G=1, probs=arr(0.5, 1.0), nq=2, quant=P(quant))
    for bad in (dict(score=None), dict(order=None), dict(offset=None), dict(probs=None), dict(quant=None), dict(G=0), dict(nq=0),
                dict(nq=9, probs=arr(*[0.5] * 9)), dict(probs=arr(2.0, 1.0)), dict(probs=arr(float("nan"), 1.0)), dict(num=-1),
                dict(num=12), dict(den=-2), dict(den=12)):
        a = dict(oks, **bad)
        rc = L.umpcBatchScoreQuantiles(h, a["score"], a["num"], a["den"], a["order"], a["offset"], a["G"], a["probs"], a["nq"], a["quant"], s)
        assert rc == -1 and b"umpcBatchScoreQuantiles" in L.umpcLastError(), bad
    # count = 0 is a successful no-op; nothing above has written anything
    a = ok
    assert L.umpcBatchEnsembleQuantiles(h, a["state"], None, None, a["ref"], 0, 0, 0, 0, a["order"], a["offset"], 1, 0, a["probs"], 2,
                                        a["quant"], s) == 0
    torch.cuda.synchronize()
    assert torch.equal(quant, keep)
    # the same calls with good arguments go through: every member at the origin, term 2 with an out table
    for term, o in ((0, None), (2, P(out))):
        assert L.umpcBatchEnsembleQuantiles(h, a["state"], o, None, a["ref"], 0, 3, 0, 0, a["order"], a["offset"], 1, term, a["probs"], 2,
                                            a["quant"], s) == 0, L.umpcLastError()
        torch.cuda.synchronize()
        assert torch.all(quant[..., 0] == 64) and torch.all(quant[..., 1:] == 0)
    sq = torch.full((1, 4), 3.0, dtype=torch.float64, device=m.device)
    assert L.umpcBatchScoreQuantiles(h, P(score), 1, 0, P(order), P(offset), 1, a["probs"], 2, P(sq), s) == 0
    torch.cuda.synchronize()
    assert sq.tolist() == [[64.0, 0.0, 1.0, 1.0]]
