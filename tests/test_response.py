"""Frequency response of recorded rollouts on the device: umpcBatchResponse adds the sums of a three-parameter sine fit
a0 + a1 cos + a2 sin of p and of pdes, per robot and position axis at the robot's own frequency, in one pass over the step
history; umpcBatchResponseFit solves them into gain, phase, offsets, residual and the error amplitude (rows: score.RESP_*).
CPU: the numpy mirror (robobee3d_amd/score.py) on planted sinusoids and against an independent least-squares solve, its
semantics on small tables, exports, refusals and the build's resource record.
GPU: the accumulation kernel against the mirror on the same arrays -- both dtypes, both alignments, table / constant reference,
chunked calls, a late step0, column blocks --, the fit kernel against the mirror on the mirror's sums, one end-to-end run,
refusals."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
# fit kernel against the mirror, rows 2..11: the largest relative deviation (the phase against 1 rad) measured on the first
# GPU run; asserted at 16 x that value and never looser than the cap (4 u of fp32; 1e-10 in fp64)
FIT_MEASURED = {"float32": 1.179e-7, "float64": 4.441e-16}
FIT_CAP = {"float32": 4 * 2.0 ** -24, "float64": 1e-10}
FIT_BOUND = {k: min(16 * FIT_MEASURED[k], FIT_CAP[k]) for k in FIT_CAP}


def _planted(B, n, seed, step0=0):
    """y_k = off + A cos(2 pi k nu + psi) per robot and axis, for p (state rows 0..2) and pdes (reference rows 0..2), in fp64:
    (state [n + 1, 18, B], ref [n, 9, B], nu [B], truth) with windows that are no whole number of periods"""
    rng = np.random.default_rng(seed)
    nu = rng.uniform(0.05, 0.45, B)
    k = (step0 + np.arange(n + 1))[:, None, None]
    tr = {key: rng.uniform(lo, hi, (3, B)) for key, lo, hi in (("y_off", -30, 30), ("y_amp", 1, 25), ("y_psi", -3, 3),
                                                                 ("r_off", -30, 30), ("r_amp", 1, 25), ("r_psi", -3, 3))}
    ang = 2 * np.pi * (k * nu[None, None, :])
    state = rng.normal(size=(n + 1, 18, B))
    ref = rng.normal(size=(n, 9, B))
    state[:, 0:3] = tr["y_off"] + tr["y_amp"] * np.cos(ang + tr["y_psi"])
    ref[:, 0:3] = (tr["r_off"] + tr["r_amp"] * np.cos(ang + tr["r_psi"]))[:n]
    return state, ref, nu, tr


def _wrap(a):
    return a - 2 * np.pi * np.ceil((a - np.pi) / (2 * np.pi))          # into (-pi, pi]


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,step0", [(41, 0), (57, 12)])
def test_mirror_recovers_planted_sinusoids(n, step0):
    from robobee3d_amd import score as S
    B = 24
    state, ref, nu, tr = _planted(B, n, 3, step0)
    frac = n * nu - np.floor(n * nu)
    assert np.all((frac > 1e-3) & (frac < 1 - 1e-3))                         # no window is a whole number of periods
    sm = S.response_sums_reference(state, ref, nu, 0, n, 0, step0, False)
    assert sm.shape == (33, B) and np.all(sm[S.RSUM_N] == n) and np.all(sm[S.RSUM_SKIPPED] == 0)
    assert np.all(S.response_pivots(sm) >= n / 8)                            # well conditioned
    resp = S.response_fit_reference(sm)
    assert resp.shape == (3, 12, B)
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    Y = tr["y_amp"] * np.exp(1j * tr["y_psi"])
    R = tr["r_amp"] * np.exp(1j * tr["r_psi"])
    H = Y / R
    assert np.all(resp[:, S.RESP_STEPS] == n) and np.all(resp[:, S.RESP_SKIPPED] == 0)
    for row, want in ((S.RESP_Y_AMP2, tr["y_amp"] ** 2), (S.RESP_R_AMP2, tr["r_amp"] ** 2), (S.RESP_GAIN, tr["y_amp"] / tr["r_amp"]),
                      (S.RESP_H_RE, H.real), (S.RESP_H_IM, H.imag), (S.RESP_Y_DC, tr["y_off"]), (S.RESP_R_DC, tr["r_off"]),
                      (S.RESP_E_AMP2, np.abs(Y - R) ** 2)):
        assert np.abs(resp[:, row] - want).max() <= 1e-10 * np.abs(want).max(), S.RESP_ROW_NAMES[row]
    dphi = _wrap(resp[:, S.RESP_PHASE] - (tr["y_psi"] - tr["r_psi"]))
    assert np.abs(dphi).max() <= 1e-10
    assert np.all(resp[:, S.RESP_Y_RES] <= 1e-10 * (tr["y_off"] ** 2 + tr["y_amp"] ** 2))
    # a lag is a negative phase: y = r delayed by a quarter period
    lag_s, lag_r = state.copy(), ref.copy()
    k = (step0 + np.arange(n + 1))[:, None, None]
    lag_s[:, 0:3] = np.cos(2 * np.pi * (k * nu[None, None, :]) - np.pi / 2)
    lag_r[:, 0:3] = np.cos(2 * np.pi * (k * nu[None, None, :]))[:n]
    lag = S.response_fit_reference(S.response_sums_reference(lag_s, lag_r, nu, 0, n, 0, step0, False))
    assert np.abs(lag[:, S.RESP_PHASE] + np.pi / 2).max() <= 1e-10 and np.abs(lag[:, S.RESP_GAIN] - 1).max() <= 1e-10
    # an independent least-squares solve on the design matrix [1, c, s]
    for b in range(B):
        cs = np.array([S.response_phase(step0 + i, nu[b:b + 1])[:2] for i in range(n)])[:, :, 0]       # [n, 2]
        A = np.column_stack([np.ones(n), cs[:, 0], cs[:, 1]])
        for j in range(3):
            ay = np.linalg.lstsq(A, state[:n, j, b], rcond=None)[0]
            ar = np.linalg.lstsq(A, ref[:, j, b], rcond=None)[0]
            h = (ay[1] - 1j * ay[2]) / (ar[1] - 1j * ar[2])
            want = {S.RESP_Y_AMP2: ay[1] ** 2 + ay[2] ** 2, S.RESP_R_AMP2: ar[1] ** 2 + ar[2] ** 2, S.RESP_H_RE: h.real,
                    S.RESP_H_IM: h.imag, S.RESP_Y_DC: ay[0], S.RESP_R_DC: ar[0], S.RESP_GAIN: abs(h),
                    S.RESP_E_AMP2: (ay[1] - ar[1]) ** 2 + (ay[2] - ar[2]) ** 2}
            scale = max(abs(ay).max(), abs(ar).max(), abs(h), 1.0) ** 2
            for row, w in want.items():
                assert abs(resp[j, row, b] - w) <= 1e-10 * scale, (b, j, S.RESP_ROW_NAMES[row], resp[j, row, b], w)
            assert abs(_wrap(resp[j, S.RESP_PHASE, b] - np.angle(h))) <= 1e-10


def test_phase_is_exact_at_the_quarter_points_and_late_steps():
    from robobee3d_amd import score as S
    c, s, u = S.response_phase(3, np.array([0.0, 0.25, 0.5, 0.75, 0.125]))
    assert u.tolist() == [0.0, 0.75, 0.5, 0.25, 0.375]
    assert c[:4].tolist() == [1.0, 0.0, -1.0, 0.0] and s[:4].tolist() == [0.0, -1.0, 0.0, 1.0]
    assert abs(c[4] + np.sqrt(0.5)) < 2e-16 and abs(s[4] - np.sqrt(0.5)) < 2e-16
    # k = 10^6 + 3: the phase is that of the fractional part of the one double product, to a few ulp
    nu = np.array([0.123456789])
    c, s, u = S.response_phase(10 ** 6 + 3, nu)
    x = float(10 ** 6 + 3) * nu
    assert u[0] == (x - np.floor(x))[0]
    import math
    assert abs(c[0] - math.cos(2 * math.pi * u[0])) < 4e-16 and abs(s[0] - math.sin(2 * math.pi * u[0])) < 4e-16
    assert S.response_nu(5.0, 25, 0.2) == 5.0 * 1e-3 * 25.0 * 0.2 and abs(S.response_nu(5.0, 25, 0.2) - 0.025) < 1e-16


def _small_tables(seed=5, B=5, n=41):
    rng = np.random.default_rng(seed)
    state = rng.normal(size=(n + 1, 18, B))
    ref = state[:n, 0:9].copy() + rng.normal(size=(n, 9, B))
    nu = rng.uniform(0.05, 0.45, B)
    return state, ref, nu


def test_mirror_semantics_on_small_tables():
    from robobee3d_amd import score as S
    state, ref, nu = _small_tables()
    n, B = 41, 5
    full = S.response_sums_reference(state, ref, nu, 0, n, 0, 0, False)
    assert np.all(full[S.RSUM_N] == n) and np.all(full[S.RSUM_SKIPPED] == 0)
    cs = np.array([S.response_phase(k, nu)[:2] for k in range(n)])                      # [n, 2, B]
    assert np.allclose(full[S.RSUM_C], cs[:, 0].sum(0), rtol=0, atol=1e-13) and np.allclose(full[S.RSUM_CS], (cs[:, 0] * cs[:, 1]).sum(0), rtol=0, atol=1e-13)
    for j in range(3):
        a = S.RSUM_AXIS + 9 * j
        assert np.allclose(full[a + S.RSUM_YC], (state[:n, j] * cs[:, 0]).sum(0), rtol=1e-13, atol=1e-13)
        assert np.allclose(full[a + S.RSUM_RS], (ref[:, j] * cs[:, 1]).sum(0), rtol=1e-13, atol=1e-13)
        assert np.allclose(full[a + S.RSUM_YR], (state[:n, j] * ref[:, j]).sum(0), rtol=1e-13, atol=1e-13)
        assert np.allclose(full[a + S.RSUM_YY], (state[:n, j] ** 2).sum(0), rtol=1e-13) and np.allclose(full[a + S.RSUM_RR], (ref[:, j] ** 2).sum(0), rtol=1e-13)
    # after = 1 is after = 0 on the table moved by one state slice, and differs from it
    a1 = S.response_sums_reference(state, ref, nu, 0, n, 0, 0, True)
    assert np.array_equal(a1, S.response_sums_reference(state[1:], ref, nu, 0, n, 0, 0, False))
    assert not np.array_equal(a1[S.RSUM_AXIS], full[S.RSUM_AXIS])
    # two chunked calls = one call, exactly (the mirror is sequential); first / ref_first / step0 move together
    part = S.response_sums_reference(state, ref, nu, 0, 17, 0, 0, False)
    part = S.response_sums_reference(state, ref, nu, 17, 24, 17, 17, False, sums=part)
    assert np.array_equal(part, full)
    # ... and step0 is the phase origin: moving it alone changes the sums, not the amplitudes
    moved = S.response_sums_reference(state, ref, nu, 0, n, 0, 1000, False)
    assert not np.array_equal(moved[S.RSUM_C], full[S.RSUM_C])
    f0, f1 = S.response_fit_reference(full), S.response_fit_reference(moved)
    for row in (S.RESP_Y_AMP2, S.RESP_R_AMP2, S.RESP_GAIN, S.RESP_PHASE, S.RESP_Y_DC, S.RESP_Y_RES, S.RESP_E_AMP2):
        assert np.allclose(f0[:, row], f1[:, row], rtol=1e-9, atol=1e-9), row
    # a constant reference [9, B]: the table that repeats it; a ZERO constant has R_AMP2 = 0 exactly and no gain, a non-zero
    # one has R_AMP2 = 0 to rounding only
    cst = S.response_sums_reference(state, ref[3], nu, 0, n, 0, 0, False)
    assert np.array_equal(cst, S.response_sums_reference(state, np.repeat(ref[3:4], n, 0), nu, 0, n, 0, 0, False))
    fc = S.response_fit_reference(cst)
    assert np.all(fc[:, S.RESP_R_AMP2] <= (64 * n * U64 * np.abs(ref[3, 0:3])) ** 2)
    assert np.allclose(fc[:, S.RESP_R_DC], ref[3, 0:3], rtol=1e-12) and np.all(fc[:, S.RESP_STEPS] == n)
    zero = np.zeros((9, B)); zero[8] = 1.0
    fz = S.response_fit_reference(S.response_sums_reference(state, zero, nu, 0, n, 0, 0, False))
    assert np.all(fz[:, S.RESP_R_AMP2] == 0) and np.all(fz[:, S.RESP_R_DC] == 0) and np.all(fz[:, S.RESP_STEPS] == n)
    for row in (S.RESP_GAIN, S.RESP_PHASE, S.RESP_H_RE, S.RESP_H_IM):
        assert np.all(np.isnan(fz[:, row])), row
    for row in (S.RESP_Y_AMP2, S.RESP_Y_DC, S.RESP_Y_RES):
        assert np.array_equal(fz[:, row], f0[:, row]), row
    assert np.array_equal(fz[:, S.RESP_E_AMP2], fz[:, S.RESP_Y_AMP2])
    # a NaN / an Inf in one robot's step: `skipped` counts it, no other row sees it
    bad_s, bad_r = state.copy(), ref.copy()
    bad_s[6, 1, 2] = np.nan
    bad_r[20, 2, 4] = np.inf
    got = S.response_sums_reference(bad_s, bad_r, nu, 0, n, 0, 0, False)
    assert got[S.RSUM_SKIPPED].tolist() == [0, 0, 1, 0, 1] and got[S.RSUM_N].tolist() == [n, n, n - 1, n, n - 1]
    assert np.all(np.isfinite(got)) and np.array_equal(got[:, [0, 1, 3]], full[:, [0, 1, 3]])
    keep = np.ones((n, B)); keep[6, 2] = keep[20, 4] = 0
    assert np.allclose(got[S.RSUM_C], (cs[:, 0] * keep).sum(0), rtol=0, atol=1e-13)
    assert np.allclose(got[S.RSUM_AXIS + S.RSUM_YC], (state[:n, 0] * cs[:, 0] * keep).sum(0), rtol=1e-13, atol=1e-13)
    fb = S.response_fit_reference(got)
    assert fb[0, S.RESP_SKIPPED].tolist() == [0, 0, 1, 0, 1] and np.all(np.isfinite(fb))
    # a frequency that is not finite skips every step of its robot
    nu_bad = nu.copy(); nu_bad[1] = np.nan
    gb = S.response_sums_reference(state, ref, nu_bad, 0, n, 0, 0, False)
    assert gb[S.RSUM_SKIPPED, 1] == n and np.all(gb[[0] + list(range(2, 33)), 1] == 0) and np.array_equal(gb[:, [0, 2, 3, 4]], full[:, [0, 2, 3, 4]])
    # an unread word may be anything: state rows 3..17, reference rows 3..8
    junk_s, junk_r = state.copy(), ref.copy()
    junk_s[:, 3:] = np.nan; junk_r[:, 3:] = np.inf
    assert np.array_equal(S.response_sums_reference(junk_s, junk_r, nu, 0, n, 0, 0, False), full)
    # refused fits: nu = 0 and nu = 0.5 (s = 0 at every step), and a window of two steps
    nu_r = nu.copy(); nu_r[0], nu_r[3] = 0.0, 0.5
    fr = S.response_fit_reference(S.response_sums_reference(state, ref, nu_r, 0, n, 0, 0, False))
    for b in (0, 3):
        assert np.all(fr[:, S.RESP_STEPS, b] == 0) and np.all(fr[:, S.RESP_SKIPPED, b] == 0) and np.all(np.isnan(fr[:, 2:, b]))
    for b in (1, 2, 4):
        assert np.array_equal(fr[:, :, b], f0[:, :, b])
    f2 = S.response_fit_reference(S.response_sums_reference(state, ref, nu, 0, 2, 0, 0, False))
    assert np.all(f2[:, S.RESP_STEPS] == 0) and np.all(np.isnan(f2[:, 2:]))
    f3 = S.response_fit_reference(S.response_sums_reference(state, ref, nu, 0, 3, 0, 0, False))
    assert np.all(f3[:, S.RESP_STEPS] == 3) and np.all(f3[:, S.RESP_Y_RES] <= 1e-10)         # three steps, three parameters
    # count = 0 is the identity
    assert np.array_equal(S.response_sums_reference(state, ref, nu, 2, 0, 0, 0, False), S.response_identity(B))
    assert np.array_equal(S.response_sums_reference(state, ref, nu, 2, 0, 0, 0, False, sums=full), full)
    fi = S.response_fit_reference(S.response_identity(B))
    assert np.all(fi[:, 0:2] == 0) and np.all(np.isnan(fi[:, 2:]))
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(step0=-1), dict(step0=1 << 53)):
        kw = dict(first=0, count=n, ref_first=0, step0=0, after=False)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.response_sums_reference(state, ref, nu, **kw)


def test_new_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    decls = ("#define UMPC_RSUM_ROWS 33", "#define UMPC_RESP_ROWS 12",
             "int umpcBatchResponseInit(umpc_batch_t *h, double *sums, void *stream);",
             "int umpcBatchResponse(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, const double *nu, "
             "long long first, long long count, long long ref_first, long long step0, int after, double *sums, void *stream);",
             "int umpcBatchResponseFit(umpc_batch_t *h, const double *sums, void *resp, void *stream);")
    for decl in decls:
        assert decl in flat, decl
    at = [flat.index(d) for d in decls]
    assert at == sorted(at) and flat.index("int umpcBatchEnsembleBootstrap(") < at[0] and at[-1] < flat.index("int umpcBatchSetStepKernel")
    assert (_lib.RSUM_ROWS, _lib.RESP_ROWS) == (S.RSUM_ROWS, S.RESP_ROWS) == (33, 12)
    assert len(S.RESP_ROW_NAMES) == 12 and S.RSUM_AXIS + 3 * S.RSUM_AXIS_ROWS == 33
    assert (S.RESP_STEPS, S.RESP_SKIPPED, S.RESP_Y_AMP2, S.RESP_R_AMP2, S.RESP_GAIN, S.RESP_PHASE, S.RESP_H_RE, S.RESP_H_IM,
            S.RESP_Y_DC, S.RESP_R_DC, S.RESP_Y_RES, S.RESP_E_AMP2) == tuple(range(12))
    L = _lib.lib()
    for sym in ("umpcBatchResponseInit", "umpcBatchResponse", "umpcBatchResponseFit"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchResponseInit.argtypes == [C.c_void_p] * 3
    assert L.umpcBatchResponse.argtypes == [C.c_void_p] * 5 + [C.c_longlong] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchResponseFit.argtypes == [C.c_void_p] * 4
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchResponseInit(None, None, None) == -1 and b"umpcBatchResponseInit" in L.umpcLastError()
    assert L.umpcBatchResponse(None, None, None, None, None, 0, 1, 0, 0, 0, None, None) == -1
    assert b"umpcBatchResponse:" in L.umpcLastError()
    assert L.umpcBatchResponseFit(None, None, None, None) == -1 and b"umpcBatchResponseFit" in L.umpcLastError()


def test_response_kernels_use_no_scratch():
    """the resource remarks of the build: the accumulation kernel (reference table / constant x plain / non-temporal x 2
    dtypes) and the fit kernel (2 dtypes) spill nothing, and their LDS is what csrc/resource_limits.json states"""
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    assert sorted(k for k in limits if "response" in k) == ["umpc_response_fit_kernel", "umpc_response_kernel"]
    for pat, n, lds in (("umpc_response_kernel", 8, 3 * 33 * 64 * 8), ("umpc_response_fit_kernel", 2, 0)):
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == lds, (k, res[k])
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds}
    assert 2 * 3 * 33 * 64 * 8 <= 160 * 1024                                     # at least two blocks fit a CU
    # no older substring pattern counts the new kernels
    for pat in limits:
        if "response" not in pat:
            assert not [k for k in res if pat in k and "response" in k], pat


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
B_, COUNT, FIRST, REF_FIRST, STEP0 = 200, 37, 3, 5, 1000
NAN_AT = (12, 1, 7)          # (state slice, row, robot): a scored step for after = 0 and 1
_CACHE = {}


def _tables(dtype, seed=20250117):
    """Seeded tables for B = 200 (three full wavefronts and a partial one): per robot and axis the reference is an offset plus a
    sinusoid at the robot's nu in [0.05, 0.45] plus noise, the state the same with its own amplitude and phase, one NaN in
    robot 7's position. Returned in `dtype`, with nu [B] float64."""
    key = (np.dtype(dtype).name, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        ns = FIRST + COUNT + 2
        nu = rng.uniform(0.05, 0.45, B_)
        kk = np.arange(REF_FIRST - FIRST + ns + 1)[:, None, None]
        ref = rng.normal(size=(len(kk), 9, B_))
        ang = 2 * np.pi * kk * nu[None, None, :]
        ref[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, B_)) + rng.uniform(2, 20, (1, 3, B_)) * np.cos(ang + rng.uniform(-3, 3, (1, 3, B_))) \
            + 0.3 * rng.normal(size=(len(kk), 3, B_))
        state = rng.normal(size=(ns + 1, 18, B_))
        state[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, B_)) + rng.uniform(2, 20, (1, 3, B_)) * np.cos(ang[:ns + 1] + rng.uniform(-3, 3, (1, 3, B_))) \
            + 0.5 * rng.normal(size=(ns + 1, 3, B_))
        state[NAN_AT] = np.nan
        _CACHE[key] = (state.astype(dtype), ref.astype(dtype), nu)
    return _CACHE[key]


def _mirror(dtype, table, after, first=FIRST, count=COUNT, step0=STEP0):
    """the mirror's sums on the seeded tables, computed once per case and left unchanged"""
    from robobee3d_amd import score as S
    key = ("mirror", dtype, table, after, first, count, step0)
    if key not in _CACHE:
        state, ref, nu = _tables(np.dtype(dtype))
        r = ref if table else np.ascontiguousarray(ref[REF_FIRST])
        sm = S.response_sums_reference(state, r, nu, first, count, (REF_FIRST + first - FIRST) if table else 0, step0, after)
        sm.setflags(write=False)
        _CACHE[key] = sm
    return _CACHE[key]


def _sum_bounds(dtype, table, after, first=FIRST, count=COUNT):
    """[33, B]: (count + 16) 2^-53 sum_k |term bound| over the steps that enter, with |y|, |r|, |y r|, y^2, r^2 or 1 as the
    term bound; 0 for the two count rows"""
    from robobee3d_amd import score as S
    state, ref, _ = _tables(np.dtype(dtype))
    st = state.astype(np.float64)[first + after:first + after + count, 0:3]
    rf = ref.astype(np.float64)
    rf = rf[REF_FIRST + first - FIRST:REF_FIRST + first - FIRST + count, 0:3] if table else np.repeat(rf[REF_FIRST][None, 0:3], count, 0)
    ok = np.isfinite(st).all(1) & np.isfinite(rf).all(1)                                  # [count, B]
    y, r = np.where(ok[:, None], np.abs(st), 0.0), np.where(ok[:, None], np.abs(rf), 0.0)
    tb = np.zeros((33, B_))
    tb[2:6] = ok.sum(0)
    for j in range(3):
        a = S.RSUM_AXIS + 9 * j
        tb[a + S.RSUM_Y] = tb[a + S.RSUM_YC] = tb[a + S.RSUM_YS] = y[:, j].sum(0)
        tb[a + S.RSUM_R] = tb[a + S.RSUM_RC] = tb[a + S.RSUM_RS] = r[:, j].sum(0)
        tb[a + S.RSUM_YY], tb[a + S.RSUM_RR], tb[a + S.RSUM_YR] = (y[:, j] ** 2).sum(0), (r[:, j] ** 2).sum(0), (y[:, j] * r[:, j]).sum(0)
    return (count + 16) * U64 * tb


def _check_sums(got, want, bound, margin, tag):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape
    for r in (0, 1):
        assert np.array_equal(got[r], want[r]), (tag, r, got[r], want[r])
    d = np.abs(got[2:] - want[2:])
    assert np.all(np.isfinite(got))
    margin("%s sum rows / bound" % tag, float((d / bound[2:]).max()), 1.0)


def _dev(m, a):
    import torch
    return None if a is None else torch.as_tensor(a).to(m.device).contiguous()


def _mpc(B, dtype):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    return BatchUprightMPC(B, getattr(torch, dtype))


def _sums(m, state, reftab, ref, nu, first, count, ref_first, step0, after, sums=None):
    """umpcBatchResponseInit + umpcBatchResponse on device tensors through the C ABI"""
    import torch
    from robobee3d_amd.batch import _ptr
    if sums is None:
        sums = torch.full((33, m.B), 7.0, dtype=torch.float64, device=m.device)
        assert m.L.umpcBatchResponseInit(m.h, _ptr(sums), m._stream()) == 0
    rc = m.L.umpcBatchResponse(m.h, _ptr(state), _ptr(reftab), _ptr(ref), _ptr(nu), first, count, ref_first, step0, int(after),
                               _ptr(sums), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return sums


def _fit(m, sums):
    import torch
    from robobee3d_amd.batch import _ptr
    resp = torch.full((3, 12, m.B), 7.0, dtype=m.dtype, device=m.device)
    assert m.L.umpcBatchResponseFit(m.h, _ptr(sums), _ptr(resp), m._stream()) == 0, m.L.umpcLastError()
    return resp


def _conditions_on_the_inputs(sm):
    """asserted on the mirror alone -- if one fires, choose another seed: every Cholesky pivot >= n / 8, no phase within 1e-6
    of +-pi, a reference amplitude above zero"""
    from robobee3d_amd import score as S
    assert np.all(S.response_pivots(sm) >= sm[S.RSUM_N] / 8)
    f = S.response_fit_reference(sm)
    assert np.all(f[:, S.RESP_R_AMP2] > 0) and np.all(np.abs(np.abs(f[:, S.RESP_PHASE]) - np.pi) > 1e-6)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_accumulation_kernel_against_the_mirror(dtype, margin):
    """after 0 / 1 x table / constant reference on one set of tables; 20 + 17 steps against 37 in one call; count 0, 1, 9;
    step0 = 10^6; run to run; columns [64, 200) on a handle of their own"""
    import torch
    state, ref, nu = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    ds, dr, dnu = _dev(m, state), _dev(m, ref), _dev(m, nu)
    dc = _dev(m, np.ascontiguousarray(ref[REF_FIRST]))
    zero = torch.zeros((33, B_), dtype=torch.float64, device=m.device)
    run = lambda table, after, first=FIRST, count=COUNT, step0=STEP0, sums=None: _sums(
        m, ds, dr if table else None, None if table else dc, dnu, first, count, (REF_FIRST + first - FIRST) if table else 0, step0, after, sums)
    for after in (0, 1):
        for table in (True, False):
            want = _mirror(dtype, table, after)
            if table:
                _conditions_on_the_inputs(want)
            assert want[1, NAN_AT[2]] == 1 and want[1].sum() == 1 and want[0, NAN_AT[2]] == COUNT - 1     # the planted NaN is scored
            _check_sums(run(table, after), want, _sum_bounds(dtype, table, after), margin, "after%d %s" % (after, "tab" if table else "const"))
    # chunks: 20 + 17 steps accumulate to what one call of 37 gives
    bound = _sum_bounds(dtype, True, 1)
    one = run(True, 1)
    two = run(True, 1, FIRST, 20, STEP0)
    two = run(True, 1, FIRST + 20, 17, STEP0 + 20, sums=two)
    assert torch.equal(one[0:2], two[0:2])
    margin("chunked against one call / bound", float(((one[2:] - two[2:]).abs().cpu().numpy() / bound[2:]).max()), 1.0)
    _check_sums(two, _mirror(dtype, True, 1), bound, margin, "chunked")
    assert torch.equal(one, run(True, 1))                                                    # run to run
    # count = 0 changes nothing; 1 and 9 steps: the tail alone, and one full trip of every slice plus a tail
    assert torch.equal(run(True, 1, count=0), zero) and torch.equal(run(True, 1, count=0, sums=one.clone()), one)
    for count in (1, 9):
        _check_sums(run(True, 0, count=count), _mirror(dtype, True, 0, count=count), _sum_bounds(dtype, True, 0, count=count), margin,
                    "count %d" % count)
    # a late phase origin: k = 10^6 .. 10^6 + 36
    _check_sums(run(True, 0, step0=10 ** 6), _mirror(dtype, True, 0, step0=10 ** 6), _sum_bounds(dtype, True, 0), margin, "step0 1e6")
    # blocks: columns [64, 200) from column-sliced tables on a B = 136 handle
    mb = _mpc(B_ - 64, dtype)
    part = _sums(mb, _dev(mb, np.ascontiguousarray(state[..., 64:])), _dev(mb, np.ascontiguousarray(ref[..., 64:])), None,
                 _dev(mb, np.ascontiguousarray(nu[64:])), FIRST, COUNT, REF_FIRST, STEP0, 1)
    assert torch.equal(part, one[:, 64:])


def _fit_deviation(got, want):
    """(rows 0 and 1 equal, the largest relative deviation over rows 2..11 with the phase against 1 rad); NaN must meet NaN"""
    from robobee3d_amd import score as S
    got = got.cpu().numpy().astype(np.float64) if hasattr(got, "cpu") else np.asarray(got, np.float64)
    exact = np.array_equal(got[:, 0:2], want[:, 0:2])
    g, w = got[:, 2:], want[:, 2:]
    assert np.array_equal(np.isnan(g), np.isnan(w))
    den = np.where(w == 0, np.finfo(float).tiny, np.abs(w))
    den[:, S.RESP_PHASE - 2] = 1.0
    d = np.abs(g - w) / den
    return exact, float(np.nanmax(d, initial=0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fit_kernel_against_the_mirror_on_the_mirrors_sums(dtype, margin):
    import torch
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    sm = np.array(_mirror(dtype, True, 1))
    want = _conditions_on_the_inputs(sm)
    exact, dev = _fit_deviation(_fit(m, _dev(m, sm)), want)
    assert exact
    margin("fit rows 2..11 rel (phase: rad)", dev, FIT_BOUND[dtype], "16 x measured %.2e, cap %.2e" % (FIT_MEASURED[dtype], FIT_CAP[dtype]))
    # refused robots: nu = 0.5 planted in one robot (s = 0 at every step), and n < 3 in a separate call
    state, ref, nu = _tables(np.dtype(dtype))
    nu2 = nu.copy(); nu2[9] = 0.5
    sm2 = S.response_sums_reference(state, ref, nu2, FIRST, COUNT, REF_FIRST, STEP0, True)
    want2 = S.response_fit_reference(sm2)
    got2 = _fit(m, _dev(m, sm2))
    assert np.all(want2[:, 0, 9] == 0) and np.all(np.isnan(want2[:, 2:, 9])) and np.all(want2[:, 0, 10] == COUNT)
    assert torch.all(got2[:, 0, 9] == 0) and torch.all(got2[:, 1, 9] == 0) and torch.all(torch.isnan(got2[:, 2:, 9]))
    exact, dev = _fit_deviation(got2, want2)
    assert exact and dev <= FIT_BOUND[dtype]
    sm3 = S.response_sums_reference(state, ref, nu, FIRST, 2, REF_FIRST, STEP0, True)
    got3 = _fit(m, _dev(m, sm3)).cpu().numpy()
    want3 = S.response_fit_reference(sm3)
    assert np.all(want3[:, 0] == 0) and np.all(np.isnan(want3[:, 2:]))
    assert np.all(got3[:, 0] == 0) and np.array_equal(got3[:, 1], want3[:, 1]) and np.all(np.isnan(got3[:, 2:]))
    # the accumulation kernel's own sums of the same call fit to the same rows, robot 9 refused on the device too
    ds = _sums(m, _dev(m, state), _dev(m, ref), None, _dev(m, nu2), FIRST, COUNT, REF_FIRST, STEP0, 1)
    got4 = _fit(m, ds)
    assert torch.all(got4[:, 0, 9] == 0) and torch.all(torch.isnan(got4[:, 2:, 9])) and torch.all(got4[:, 0, 10] == COUNT)


@pytest.mark.gpu
def test_end_to_end_frequency_sweep(margin):
    """helix(trajAmp = 20, useY = False) at 5 Hz (cell 0) and 10 Hz (cell 1) over B = 128 as two contiguous cells of 64, 200
    recorded steps in fp32: frequency_response against the mirror on the downloaded history -- the sums within the bounds
    of the accumulation test, the rows against the mirror's fit of those sums --, the reference's amplitude, the cells'
    median gain^2 through score_quantiles, and a chunked run. Which cell tracks better is not asserted."""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, dtype = 128, 200, "float32"
    m = _mpc(B, dtype)
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    freq = np.repeat([5.0, 10.0], 64)
    nu = S.response_nu(freq, int(m.prm.nsub), float(m.prm.dtsim))
    assert np.abs(nu - np.repeat([0.025, 0.05], 64)).max() < 1e-16
    tab = m.task_table(K, "helix", trajAmp=20.0, trajFreq=freq, useY=False)
    m.set_reference_trajectory(tab)
    m.record_history(K)
    m.rollout(K)
    hs, ht = m.history()["state"].cpu().numpy(), tab.cpu().numpy()
    for after in (False, True):
        want = S.response_sums_reference(hs, ht, nu, 0, K, 0, 0, after)
        assert np.all(want[S.RSUM_N] == K) and np.all(want[S.RSUM_SKIPPED] == 0)
        assert np.all(S.response_pivots(want) >= K / 8)                                   # conditions on the inputs, axis 0
        fw = S.response_fit_reference(want)
        assert np.all(fw[0, S.RESP_R_AMP2] > 0) and np.all(np.abs(np.abs(fw[0, S.RESP_PHASE]) - np.pi) > 1e-6)
        resp, sums = m.frequency_response(freq, after=after)
        assert tuple(resp.shape) == (3, 12, B) and resp.dtype == torch.float32 and tuple(sums.shape) == (33, B) and sums.dtype == torch.float64
        y = np.abs(hs[int(after):K + int(after), 0:3].astype(np.float64))
        r = np.abs(ht[:, 0:3].astype(np.float64))
        tb = np.zeros((33, B))
        tb[2:6] = K
        for j in range(3):
            a = S.RSUM_AXIS + 9 * j
            tb[a + S.RSUM_Y] = tb[a + S.RSUM_YC] = tb[a + S.RSUM_YS] = y[:, j].sum(0)
            tb[a + S.RSUM_R] = tb[a + S.RSUM_RC] = tb[a + S.RSUM_RS] = r[:, j].sum(0)
            tb[a + S.RSUM_YY], tb[a + S.RSUM_RR], tb[a + S.RSUM_YR] = (y[:, j] ** 2).sum(0), (r[:, j] ** 2).sum(0), (y[:, j] * r[:, j]).sum(0)
        bound = (K + 16) * U64 * tb
        bound[bound == 0] = np.finfo(float).tiny                  # (the y axis of the reference is 0 at every step: exact zeros)
        _check_sums(sums, want, bound, margin, "end to end after%d" % after)
        exact, dev = _fit_deviation(resp, S.response_fit_reference(sums.cpu().numpy()))
        assert exact
        margin("end to end after%d fit rows rel" % after, dev, FIT_BOUND[dtype])
        got = resp.cpu().numpy().astype(np.float64)
        margin("end to end after%d |sqrt(R_AMP2) - 20| axis 0" % after, float(np.abs(np.sqrt(got[0, S.RESP_R_AMP2]) - 20.0).max()), 1e-3)
        assert np.all(got[1, S.RESP_R_AMP2] == 0) and np.all(np.isnan(got[1, S.RESP_GAIN]))         # useY = False: pdes_y = 0
        print("after=%d cell medians: gain %s phase %s |S| %s" % (after, np.median(got[0, S.RESP_GAIN].reshape(2, 64), 1),
              np.median(got[0, S.RESP_PHASE].reshape(2, 64), 1), np.median(np.sqrt(got[0, S.RESP_E_AMP2] / got[0, S.RESP_R_AMP2]).reshape(2, 64), 1)))
    # resp[axis] is shaped as a score: the cells' median gain^2, unchanged score_quantiles
    resp, sums = m.frequency_response(freq, after=True)
    index = m.group_index(np.repeat(np.arange(2, dtype=np.int32), 64), 2)
    q = m.score_quantiles(resp[0], index, [0.5], S.RESP_Y_AMP2, S.RESP_R_AMP2).cpu().numpy()
    wq = S.score_quantiles_reference(resp[0].cpu().numpy(), index[0].cpu().numpy(), index[1].cpu().numpy(), [0.5], S.RESP_Y_AMP2, S.RESP_R_AMP2)
    assert np.array_equal(q, wq) and np.all(q[:, 0] == 64) and np.all(np.isfinite(q[:, 2]))
    # chunks: steps 0..79, then 80..199 with the sums passed back and no fit in between
    none, part = m.frequency_response(freq, 0, 80, after=True, fit=False)
    assert none is None
    resp2, part = m.frequency_response(freq, 80, 120, after=True, sums=part)
    assert torch.equal(part[0:2], sums[0:2])
    margin("end to end chunked against one call / bound", float(((part[2:] - sums[2:]).abs().cpu().numpy() / bound[2:]).max()), 1.0)
    # a scalar frequency is every robot's
    r5, s5 = m.frequency_response(5.0, after=True)
    assert torch.equal(s5[:, :64], sums[:, :64])
    assert torch.allclose(r5[:, :, :64], resp[:, :, :64], rtol=0, atol=0, equal_nan=True)      # (axis 1 holds NaN rows)
    with pytest.raises(ValueError):
        m.frequency_response(freq, 0, K + 1)
    with pytest.raises(ValueError):
        m.frequency_response(freq, sums=torch.zeros((33, B), device=m.device))          # not float64


@pytest.mark.gpu
def test_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((5, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((4, 9, 64), device=m.device)
    nu = torch.full((64,), 0.1, dtype=torch.float64, device=m.device)
    sums = torch.full((33, 64), 3.0, dtype=torch.float64, device=m.device)
    keep = sums.clone()
    ok = dict(state=P(state), tab=None, ref=P(ref), nu=P(nu), first=0, count=4, ref_first=0, step0=0, sums=P(sums))
    for bad in (dict(count=-1), dict(count=(1 << 31) - 8), dict(first=-1), dict(ref_first=-1), dict(step0=-1), dict(step0=1 << 53),
                dict(tab=P(tab)), dict(ref=None), dict(nu=None), dict(sums=None), dict(state=None)):
        a = dict(ok, **bad)
        rc = L.umpcBatchResponse(h, a["state"], a["tab"], a["ref"], a["nu"], a["first"], a["count"], a["ref_first"], a["step0"], 0,
                                 a["sums"], s)
        assert rc == -1 and b"umpcBatchResponse:" in L.umpcLastError(), bad
    assert L.umpcBatchResponseInit(h, None, s) == -1 and b"umpcBatchResponseInit" in L.umpcLastError()
    resp = torch.zeros((3, 12, 64), device=m.device)
    assert L.umpcBatchResponseFit(h, None, P(resp), s) == -1 and b"umpcBatchResponseFit" in L.umpcLastError()
    assert L.umpcBatchResponseFit(h, P(sums), None, s) == -1
    torch.cuda.synchronize()
    assert torch.equal(sums, keep)
    # the same call with good arguments goes through, count = 0 changes nothing, and the call adds into the sums
    assert L.umpcBatchResponse(h, P(state), None, P(ref), P(nu), 0, 0, 0, 0, 0, P(sums), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, keep)
    assert L.umpcBatchResponse(h, P(state), None, P(ref), P(nu), 0, 4, 0, 0, 0, P(sums), s) == 0
    torch.cuda.synchronize()
    assert torch.all(sums[0] == 7.0) and torch.all(sums[1] == 3.0) and torch.all(sums[6] == 3.0)
