"""Error spectra of recorded rollouts on the device: umpcBatchSpectrum projects the tracking error, the attitude error or the
command of every robot onto K windowed cosine / sine pairs in one pass over the step history (a host-made basis table, no
sincos on the device), umpcBatchSpectrumPower turns the raw sums into a periodogram and a chatter score per robot (rows:
score.SPEC_*), umpcBatchSpectrumGroups sums the periodograms over the draws of each grid cell.
CPU: the numpy mirrors (robobee3d_amd/score.py) on planted sinusoids, against numpy.fft.rfft, Parseval, a Hann window off the
grid, the high share, refusals and semantics, the group mirror by hand, exports and the build's resource record.
GPU: the sums kernel against the mirror BIT FOR BIT -- both dtypes, both alignments, K across the tile boundaries, table /
constant reference, after 0 / 1, the three signals, planted NaN / Inf, column blocks, chunks --, the power kernel on the
mirror's sums, the groups kernel on group sizes around the wavefront, one end-to-end run, refusals.

The bound used throughout: a sum of n products y_k b_jk, each basis word within 3 u of its real value (2 ulp of the cosine,
one rounding of w c), one rounding per product and n - 1 per sum, lies within (n + 4) u sum_k |y_k b_jk| of the exact sum,
u = 2^-53."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def _tables_from_signal(y, offset_rows=0):
    """state [W + 1, 18, B] whose rows 0..2 are y [W, 3, B] (the last slice repeats) and a zero constant reference [9, B]"""
    W, _, B = y.shape
    state = np.zeros((W + 1, 18, B))
    state[:W, offset_rows:offset_rows + 3] = y
    state[W, offset_rows:offset_rows + 3] = y[-1]
    return state, np.zeros((9, B))


def _sums_of(y, basis, dtype=np.float64):
    from robobee3d_amd import score as S
    state, ref = _tables_from_signal(y)
    return S.spectrum_sums_reference("ep", state, None, ref, basis, 0, 0, y.shape[0], 0, False, dtype)


def _ab(sm, wsum, K):
    """(m [3, B], A [3, K, B], Bq [3, K, B]) from the sums, in the mirror's operation order"""
    chan = 2 + 2 * K
    m, A, Bq = [], [], []
    for c in range(3):
        ch = sm[2 + c * chan:2 + (c + 1) * chan]
        mc = ch[0] / wsum[0]
        m.append(mc)
        A.append(np.stack([ch[2 + 2 * j] - mc * wsum[1 + 2 * j] for j in range(K)]))
        Bq.append(np.stack([ch[3 + 2 * j] - mc * wsum[2 + 2 * j] for j in range(K)]))
    return np.stack(m), np.stack(A), np.stack(Bq)


def _ab_bounds(y, basis, wsum):
    """[3, K, B] bounds on A_j and on B_j: the bound of the sum C_j (S_j), the bound of sum w y carried through m Wc_j (m Ws_j),
    and four roundings of the final operations"""
    n, K = y.shape[0], (basis.shape[1] - 1) // 2
    ay = np.abs(y)                                                                     # [n, 3, B]
    bwy = (n + 4) * U64 * np.einsum("k,kcb->cb", np.abs(basis[:n, 0]), ay) / abs(wsum[0])       # bound on m
    m = np.einsum("k,kcb->cb", basis[:n, 0], y) / wsum[0]
    out = []
    for part in (1, 2):
        col = np.abs(basis[:n, part::2])                                               # [n, K]
        s = (n + 4) * U64 * np.einsum("kj,kcb->cjb", col, ay)
        ws = np.abs(wsum[part::2])[None, :, None]
        out.append(s + ws * bwy[:, None, :] + 4 * U64 * (np.einsum("kj,kcb->cjb", col, ay) + ws * np.abs(m)[:, None, :]))
    return out


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_planted_on_grid_sinusoids():
    from robobee3d_amd import score as S
    B, W = 24, 48
    rng = np.random.default_rng(11)
    nu = np.arange(1, 24) / 48.0
    freq = nu * 200.0                                                  # 5 ms steps
    K = len(nu)
    jp = rng.integers(1, 24, (3, B))                                   # the planted bin of each robot and channel
    amp, off, psi = rng.uniform(0.5, 2.0, (3, B)), rng.uniform(-3, 3, (3, B)), rng.uniform(-3, 3, (3, B))
    k = np.arange(W)[:, None, None]
    y = off + amp * np.cos(2 * np.pi * k * jp / 48.0 + psi)
    basis = S.spectrum_basis(nu, W, "rect")
    assert basis.shape == (W, 1 + 2 * K) and np.all(basis[:, 0] == 1.0)
    wsum = S.spectrum_wsum(basis)
    sm = _sums_of(y, basis)
    assert sm.shape == (2 + 3 * (2 + 2 * K), B) and np.all(sm[0] == W) and np.all(sm[1] == 0)
    spec, power = S.spectrum_power_reference(sm, wsum, freq, W, K)
    assert spec.shape == (3, 12, B) and power.shape == (3, K, B)
    at = np.zeros((3, K, B), bool)
    np.put_along_axis(at, (jp - 1)[:, None, :], True, 1)
    peak = np.take_along_axis(power, (jp - 1)[:, None, :], 1)[:, 0]
    assert np.abs(peak - amp ** 2).max() <= 1e-12 * (amp ** 2).max()
    others = np.where(at, 0.0, power)
    print("largest off-peak bin / a^2: %.3e" % (others / (amp ** 2)[:, None, :]).max())
    assert np.all(others <= 1e-20 * (amp ** 2)[:, None, :])
    assert np.abs(spec[:, S.SPEC_MEAN] - off).max() <= 1e-13 * 8
    assert np.array_equal(spec[:, S.SPEC_PEAK_BIN], jp - 1) and np.array_equal(spec[:, S.SPEC_PEAK_HZ], freq[jp - 1])
    assert np.array_equal(spec[:, S.SPEC_PEAK_POWER], peak)
    assert np.abs(spec[:, S.SPEC_PEAK_SHARE] - 1).max() <= 1e-12 and np.abs(spec[:, S.SPEC_CENTROID_HZ] - freq[jp - 1]).max() <= 1e-9
    assert np.all(spec[:, S.SPEC_BANDWIDTH_HZ] <= 1e-6) and np.all(spec[:, S.SPEC_HIGH_SHARE] == 0)
    assert np.abs(spec[:, S.SPEC_VAR] - amp ** 2 / 2).max() <= 1e-12 * (amp ** 2 + off ** 2).max()
    assert np.all(spec[:, S.SPEC_STEPS] == W) and np.all(spec[:, S.SPEC_SKIPPED] == 0)
    # the quarter points of the phase are exact: bin 12 of 48 at step 1 is (0, 1), at step 2 (-1, 0)
    assert basis[1, 1 + 2 * 11] == 0.0 and basis[1, 2 + 2 * 11] == 1.0 and basis[2, 1 + 2 * 11] == -1.0 and basis[2, 2 + 2 * 11] == 0.0


@pytest.mark.parametrize("W", [48, 37])
def test_against_numpy_rfft(W, margin):
    """A_j - i B_j against numpy.fft.rfft(y - mean) on noise with an offset, full grid, rect window"""
    from robobee3d_amd import score as S
    B = 24
    rng = np.random.default_rng(W)
    y = rng.normal(size=(W, 3, B)) + rng.normal(scale=2.0, size=(1, 3, B))
    nu = np.arange(1, (W - 1) // 2 + 1) / float(W)
    nu = nu[nu < 0.5]
    K = len(nu)
    basis = S.spectrum_basis(nu, W, "rect")
    wsum = S.spectrum_wsum(basis)
    m, A, Bq = _ab(_sums_of(y, basis), wsum, K)
    F = np.fft.rfft(y - y.mean(0), axis=0)[1:K + 1]                                     # [K, 3, B]
    bA, bB = _ab_bounds(y, basis, wsum)
    margin("A_j against Re rfft / bound", float((np.abs(A - F.real.transpose(1, 0, 2)) / bA).max()), 1.0)
    margin("B_j against -Im rfft / bound", float((np.abs(Bq + F.imag.transpose(1, 0, 2)) / bB).max()), 1.0)
    # the bare operation-count bound (n + 4) u sum |y b| of the sums themselves, against the exact products in long double
    chan = 2 + 2 * K
    sm = _sums_of(y, basis)
    lb, ly = basis.astype(np.longdouble), y.astype(np.longdouble)
    for c in range(3):
        exact = np.einsum("kj,kb->jb", lb[:, 1:], ly[:, c])
        bound = (W + 4) * U64 * np.einsum("kj,kb->jb", np.abs(basis[:, 1:]), np.abs(y[:, c]))
        got = sm[2 + c * chan + 2:2 + (c + 1) * chan]
        margin("sums against long double / (n + 4) u sum |y b|, channel %d" % c, float((np.abs(got - exact) / bound).max()), 1.0)


def test_parseval_rect_full_grid():
    """W odd (no Nyquist bin), every bin 1 .. (W - 1) / 2: sum_j P_j / 2 is the variance"""
    from robobee3d_amd import score as S
    B, W = 24, 47
    rng = np.random.default_rng(2)
    y = rng.normal(size=(W, 3, B)) + rng.normal(scale=2.0, size=(1, 3, B))
    nu = np.arange(1, 24) / 47.0
    K = len(nu)
    basis = S.spectrum_basis(nu, W, "rect")
    wsum = S.spectrum_wsum(basis)
    sm = _sums_of(y, basis)
    spec, power = S.spectrum_power_reference(sm, wsum, nu, W, K)
    m, A, Bq = _ab(sm, wsum, K)
    bA, bB = _ab_bounds(y, basis, wsum)
    # what the bounds on A_j, B_j leave of P_j = 4 (A^2 + B^2) / W^2, summed and halved, plus the variance's own sums:
    # (n + 4) u sum y^2 / W for sum w y y / W0 and 2 |m| times the bound on m, plus a few roundings of the results
    tol = (4 * (2 * np.abs(A) * bA + bA ** 2 + 2 * np.abs(Bq) * bB + bB ** 2) / W ** 2).sum(1) / 2
    ay2 = (y ** 2).sum(0) / W
    bm = (W + 4) * U64 * np.abs(y).sum(0) / W
    tol = tol + (W + 4) * U64 * ay2 + 2 * np.abs(m) * bm + bm ** 2 + 8 * U64 * (ay2 + m * m) + 4 * K * U64 * spec[:, S.SPEC_TOTAL]
    d = np.abs(spec[:, S.SPEC_TOTAL] / 2 - spec[:, S.SPEC_VAR])
    print("Parseval: worst |sum P / 2 - var| / tolerance %.3f" % (d / tol).max())
    assert np.all(d <= tol)
    assert np.abs(spec[:, S.SPEC_VAR] - y.var(0)).max() <= 1e-13 * (y ** 2).mean(0).max()
    assert np.abs(spec[:, S.SPEC_TOTAL] - power.sum(1)).max() <= 1e-14 * power.sum(1).max()


def test_hann_off_grid_and_offset_removal(margin):
    from robobee3d_amd import score as S
    B, W = 24, 64
    rng = np.random.default_rng(3)
    nu = np.arange(1, 32) / 64.0
    K = len(nu)
    # in bins, off the grid by 0.1 to 0.4 of a bin either way (at 0.4 the Hann main lobe leaves the nearest bin 0.54 of the total)
    tone = rng.integers(3, 30, (3, B)) + rng.uniform(0.1, 0.4, (3, B)) * rng.choice([-1.0, 1.0], (3, B))
    amp, psi = rng.uniform(0.5, 2.0, (3, B)), rng.uniform(-3, 3, (3, B))
    k = np.arange(W)[:, None, None]
    y = amp * np.cos(2 * np.pi * k * tone / 64.0 + psi)
    basis = S.spectrum_basis(nu, W, "hann")
    assert basis[0, 0] == 0.0 and basis[32, 0] == 1.0 and np.allclose(basis[:, 0], 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(W) / W), rtol=0, atol=1e-15)
    wsum = S.spectrum_wsum(basis)
    assert abs(wsum[0] - W / 2) <= 1e-13 * W
    spec, power = S.spectrum_power_reference(_sums_of(y, basis), wsum, nu * 200.0, W, K)
    assert np.array_equal(spec[:, S.SPEC_PEAK_BIN], np.rint(tone) - 1)          # the bin nearest the tone
    assert np.all(spec[:, S.SPEC_PEAK_SHARE] > 0.5) and np.all(np.abs(spec[:, S.SPEC_CENTROID_HZ] - tone * 200.0 / 64) < 200.0 / 64)
    # a constant offset 1e3 times the amplitude: the mean is removed through the window's own transform, exactly in real
    # arithmetic, so every P_j moves by rounding alone -- by what the bounds of both runs leave of 4 (A^2 + B^2) / W0^2
    y2 = y + 1e3 * amp
    sm2 = _sums_of(y2, basis)
    spec2, power2 = S.spectrum_power_reference(sm2, wsum, nu * 200.0, W, K)
    _, A, Bq = _ab(sm2, wsum, K)
    bA, bB = [a + b for a, b in zip(_ab_bounds(y, basis, wsum), _ab_bounds(y2, basis, wsum))]
    tol = 4 * (2 * np.abs(A) * bA + bA ** 2 + 2 * np.abs(Bq) * bB + bB ** 2) / wsum[0] ** 2 + 8 * U64 * power
    margin("P_j with an offset of 1e3 a / bound", float((np.abs(power2 - power) / tol).max()), 1.0)
    assert np.array_equal(spec2[:, S.SPEC_PEAK_BIN], spec[:, S.SPEC_PEAK_BIN])
    assert np.abs(spec2[:, S.SPEC_MEAN] / (1e3 * amp) - 1).max() < 0.05          # (a Hann-weighted mean of offset + tone)


def test_high_share_of_two_tones():
    from robobee3d_amd import score as S
    B, W = 24, 48
    rng = np.random.default_rng(4)
    nu = np.arange(1, 24) / 48.0
    freq = nu * 200.0
    a1, a2 = rng.uniform(0.5, 2.0, (3, B)), rng.uniform(0.5, 2.0, (3, B))
    k = np.arange(W)[:, None, None]
    y = 0.7 + a1 * np.cos(2 * np.pi * k * 5 / 48.0 + 0.3) + a2 * np.cos(2 * np.pi * k * 17 / 48.0 - 1.1)
    basis = S.spectrum_basis(nu, W, "rect")
    sm = _sums_of(y, basis)
    for jsplit in (5, 11, 16):                                           # bins 5 .. 16 lie between the tones (bin j is index j - 1)
        spec, _ = S.spectrum_power_reference(sm, S.spectrum_wsum(basis), freq, W, jsplit)
        assert np.abs(spec[:, S.SPEC_HIGH_SHARE] - a2 ** 2 / (a1 ** 2 + a2 ** 2)).max() <= 1e-12
    lo, _ = S.spectrum_power_reference(sm, S.spectrum_wsum(basis), freq, W, 0)
    hi, _ = S.spectrum_power_reference(sm, S.spectrum_wsum(basis), freq, W, 23)
    assert np.abs(lo[:, S.SPEC_HIGH_SHARE] - 1).max() <= 1e-12 and np.all(hi[:, S.SPEC_HIGH_SHARE] == 0)
    assert np.array_equal(lo[:, :S.SPEC_HIGH_SHARE], hi[:, :S.SPEC_HIGH_SHARE])
    want = (freq[4] * a1 ** 2 + freq[16] * a2 ** 2) / (a1 ** 2 + a2 ** 2)
    assert np.abs(lo[:, S.SPEC_CENTROID_HZ] - want).max() <= 1e-9
    bw = np.sqrt(((freq[4] - want) ** 2 * a1 ** 2 + (freq[16] - want) ** 2 * a2 ** 2) / (a1 ** 2 + a2 ** 2))
    assert np.abs(lo[:, S.SPEC_BANDWIDTH_HZ] - bw).max() <= 1e-9


def _noise_tables(B, dtype, seed=20250301, attitude=False):
    """Seeded noise tables for the semantics and the GPU tests: state [44, 18, B], out [43, 9, B], ref [46, 9, B] in `dtype`,
    with a NaN in robot 7's position, an Inf in robot 70's reference attitude, a NaN in robot 130's command and, with
    `attitude`, an Inf in robot 33's attitude (so that a constant reference has a skipped step too)"""
    rng = np.random.default_rng(seed + B)
    state = rng.normal(size=(44, 18, B))
    out = rng.normal(size=(43, 9, B))
    ref = rng.normal(size=(46, 9, B))
    state[12, 1, 7] = np.nan
    ref[20, 7, 70] = np.inf
    out[9, 2, 130] = np.nan
    if attitude:
        state[15, 10, 33] = np.inf
    return state.astype(dtype), out.astype(dtype), ref.astype(dtype)


FIRST, COUNT, REF_FIRST, BASIS_FIRST = 3, 37, 5, 2


def _basis(K, window="hann"):
    from robobee3d_amd import score as S
    nu = (np.arange(K) + 0.7) / (2.0 * K + 1.0)                         # K frequencies inside (0, 0.5)
    return S.spectrum_basis(nu, BASIS_FIRST + COUNT + 3, window, step0=1000), nu


def _mirror(signal, tables, table, after, K, dtype, first=FIRST, count=COUNT, basis_first=BASIS_FIRST, sums=None):
    from robobee3d_amd import score as S
    state, out, ref = tables
    r = ref if table else np.ascontiguousarray(ref[REF_FIRST])
    return S.spectrum_sums_reference(signal, state, out, r, _basis(K)[0], basis_first, first, count,
                                     (REF_FIRST + first - FIRST) if table else 0, after, dtype, sums)


def _term_bounds(signal, tables, table, after, K, dtype, first=FIRST, count=COUNT, basis_first=BASIS_FIRST):
    """[rows, B]: (count + 4) u sum_k |term| over the steps that enter; 0 for the two count rows"""
    state, out, ref = [np.asarray(t, np.float64) for t in tables]
    if signal == "u":
        y = out[first:first + count, 0:3]
        ok = np.isfinite(y).all(1)
    else:
        y0, r0 = (0, 0) if signal == "ep" else (9, 6)
        y = state[first + after:first + after + count, y0:y0 + 3]
        r = ref[REF_FIRST + first - FIRST:REF_FIRST + first - FIRST + count, r0:r0 + 3] if table else ref[REF_FIRST][None, r0:r0 + 3]
        ok = np.isfinite(y).all(1) & np.isfinite(y - r).all(1)
        y = (np.asarray(tables[0])[first + after:first + after + count, y0:y0 + 3] - (np.asarray(tables[2])[
            REF_FIRST + first - FIRST:REF_FIRST + first - FIRST + count, r0:r0 + 3] if table else np.asarray(tables[2])[REF_FIRST][None, r0:r0 + 3])).astype(np.float64)
    v = np.where(ok[:, None], np.abs(y), 0.0)                                        # [count, 3, B]
    b = np.abs(_basis(K)[0][basis_first:basis_first + count])
    rows = 2 + 3 * (2 + 2 * K)
    tb = np.zeros((rows, v.shape[2]))
    for c in range(3):
        at = 2 + c * (2 + 2 * K)
        tb[at] = np.einsum("k,kb->b", b[:, 0], v[:, c])
        tb[at + 1] = np.einsum("k,kb->b", b[:, 0], v[:, c] ** 2)
        tb[at + 2:at + 2 + 2 * K] = np.einsum("kj,kb->jb", b[:, 1:], v[:, c])
    return (count + 4) * U64 * tb


def test_refusals_and_semantics():
    from robobee3d_amd import score as S
    B, K = 140, 5
    tables = _noise_tables(B, np.float64)
    state, out, ref = tables
    basis, nu = _basis(K)
    rows = 2 + 3 * (2 + 2 * K)
    assert S.spectrum_sum_rows(K) == rows and S.spectrum_identity(K, B).shape == (rows, B)
    wsum = S.spectrum_wsum(basis, BASIS_FIRST, COUNT)
    assert np.array_equal(wsum, np.add.reduce(basis[BASIS_FIRST:BASIS_FIRST + COUNT], 0)) or np.allclose(wsum, basis[BASIS_FIRST:BASIS_FIRST + COUNT].sum(0), rtol=0, atol=1e-13)
    clean = [t.copy() for t in tables]
    clean[0][12, 1, 7] = 0.25; clean[2][20, 7, 70] = -0.5; clean[1][9, 2, 130] = 0.125
    # a planted NaN / Inf step: `skipped` counts it and the fit is refused; the other robots are bit-unchanged
    for signal, robot, after in (("ep", 7, 0), ("es", 70, 0), ("u", 130, 0), ("ep", 7, 1)):
        got = _mirror(signal, tables, True, after, K, np.float64)
        want = _mirror(signal, clean, True, after, K, np.float64)
        others = np.arange(B) != robot
        assert got[1].tolist() == [float(b == robot) for b in range(B)] and got[0, robot] == COUNT - 1, signal
        assert np.all(np.isfinite(got)) and np.array_equal(got[:, others], want[:, others])
        spec, power = S.spectrum_power_reference(got, wsum, nu * 200.0, COUNT, 3)
        swant, pwant = S.spectrum_power_reference(want, wsum, nu * 200.0, COUNT, 3)
        assert np.all(spec[:, S.SPEC_STEPS, robot] == 0) and np.all(spec[:, S.SPEC_SKIPPED, robot] == 1)
        assert np.all(np.isnan(spec[:, 2:, robot])) and np.all(np.isnan(power[:, :, robot]))
        assert np.array_equal(spec[:, :, others], swant[:, :, others]) and np.array_equal(power[:, :, others], pwant[:, :, others])
        assert np.all(swant[:, S.SPEC_STEPS] == COUNT) and np.all(np.isfinite(swant)) and np.all(np.isfinite(pwant))
    # what a signal does not read may be anything
    junk = [t.copy() for t in clean]
    junk[0][:, 3:9] = np.nan; junk[0][:, 12:] = np.inf; junk[2][:, 3:6] = np.nan; junk[1][:] = np.nan
    for signal in ("ep", "es"):
        assert np.array_equal(_mirror(signal, junk, True, 1, K, np.float64), _mirror(signal, clean, True, 1, K, np.float64))
    assert np.array_equal(S.spectrum_sums_reference("u", None, clean[1], None, basis, BASIS_FIRST, FIRST, COUNT, 0, True),
                          _mirror("u", clean, False, 0, K, np.float64))
    # after = 1 is after = 0 on the table moved by one state slice; the two signals differ; a constant reference is its table
    a1 = _mirror("ep", clean, True, 1, K, np.float64)
    assert np.array_equal(a1, _mirror("ep", [clean[0][1:], clean[1], clean[2]], True, 0, K, np.float64))
    assert not np.array_equal(a1, _mirror("ep", clean, True, 0, K, np.float64)) and not np.array_equal(a1, _mirror("es", clean, True, 1, K, np.float64))
    rep = [clean[0], clean[1], np.repeat(clean[2][REF_FIRST:REF_FIRST + 1], 46, 0)]
    assert np.array_equal(_mirror("ep", clean, False, 0, K, np.float64), _mirror("ep", rep, True, 0, K, np.float64))
    # the difference is formed in the handle's dtype: fp32 tables give what their rounded difference gives
    t32 = [t.astype(np.float32) for t in clean]
    d32 = [np.zeros_like(clean[0]), clean[1], np.zeros_like(clean[2])]
    d32[0][FIRST:FIRST + COUNT, 0:3] = (t32[0][FIRST:FIRST + COUNT, 0:3] - t32[2][REF_FIRST:REF_FIRST + COUNT, 0:3]).astype(np.float64)
    assert np.array_equal(_mirror("ep", t32, True, 0, K, np.float32), _mirror("ep", d32, True, 0, K, np.float64))
    # nrows that is not the number of steps: refused everywhere; n < 2 likewise; zero power likewise
    full = _mirror("ep", clean, True, 0, K, np.float64)
    s_bad, p_bad = S.spectrum_power_reference(full, wsum, nu * 200.0, COUNT + 1, 3)
    assert np.all(s_bad[:, 0] == 0) and np.all(np.isnan(s_bad[:, 2:])) and np.all(np.isnan(p_bad)) and np.all(s_bad[:, 1] == 0)
    one = _mirror("ep", clean, True, 0, K, np.float64, count=1)
    s1, _ = S.spectrum_power_reference(one, S.spectrum_wsum(basis, BASIS_FIRST, 1), nu * 200.0, 1, 3)
    assert np.all(s1[:, 0] == 0) and np.all(np.isnan(s1[:, 2:]))
    flat = [np.zeros_like(clean[0]), clean[1], np.zeros_like(clean[2])]
    s0, p0 = S.spectrum_power_reference(_mirror("ep", flat, True, 0, K, np.float64), wsum, nu * 200.0, COUNT, 3)
    assert np.all(s0[:, 0] == 0) and np.all(np.isnan(s0[:, 2:])) and np.all(np.isnan(p0))
    # chunks of 20 + 17 steps against 37 undivided: the counts equal, the other rows within the bound
    part = _mirror("ep", tables, True, 1, K, np.float64, count=20)
    part = _mirror("ep", tables, True, 1, K, np.float64, first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=part)
    whole = _mirror("ep", tables, True, 1, K, np.float64)
    bound = _term_bounds("ep", tables, True, 1, K, np.float64)
    assert np.array_equal(part[0:2], whole[0:2]) and np.all(np.abs(part[2:] - whole[2:]) <= 2 * bound[2:])
    assert not np.array_equal(part, whole)                                           # (the order of summation differs)
    assert np.array_equal(_mirror("ep", tables, True, 1, K, np.float64, count=0), S.spectrum_identity(K, B))
    assert np.array_equal(_mirror("ep", tables, True, 1, K, np.float64, count=0, sums=whole), whole)
    # refused arguments
    for bad_nu in ([0.0, 0.1], [0.1, 0.5], [-0.1], [0.6], [np.nan]):
        with pytest.raises(ValueError):
            S.spectrum_basis(bad_nu, 16)
    for bad_k in (np.zeros(0), np.full(65, 0.25)):
        with pytest.raises(ValueError):
            S.spectrum_basis(bad_k, 16)
    for k in (0, 65):
        with pytest.raises(ValueError):
            S.spectrum_sum_rows(k)
    assert S.spectrum_basis(np.full(64, 0.25), 4).shape == (4, 129)
    with pytest.raises(ValueError):
        S.spectrum_basis([0.1], 16, "blackman")
    with pytest.raises(ValueError):
        _mirror("ep", tables, True, 1, K, np.float64, sums=np.zeros((rows + 2, B)))
    with pytest.raises(ValueError):
        _mirror("ep", tables, True, 1, K, np.float64, sums=np.zeros((rows, B + 1)))
    with pytest.raises(ValueError):
        _mirror("ep", tables, True, 1, K, np.float64, basis_first=BASIS_FIRST + 4)          # the basis ends before the call
    with pytest.raises(ValueError):
        _mirror("tau", tables, True, 1, K, np.float64)
    with pytest.raises(ValueError):
        S.spectrum_power_reference(full, wsum[:-2], nu * 200.0, COUNT, 3)
    with pytest.raises(ValueError):
        S.spectrum_power_reference(full, wsum, nu * 200.0, COUNT, K + 1)
    with pytest.raises(ValueError):
        S.spectrum_sums_reference("u", state, None, ref, basis, 0, 0, 4, 0, False)


GROUP_SIZES = (1, 3, 64, 65, 130)


def _group_tables(dtype, K, seed=9):
    """B = 268: groups of 1, 3, 64, 65 and 130 members scattered over the batch, 5 robots in no group; power [3, K, B] dyadic
    (multiples of 1/8 below 64: every order of summation is exact), a few members refused"""
    rng = np.random.default_rng(seed + K)
    B = sum(GROUP_SIZES) + 5
    group = np.concatenate([np.full(n, g) for g, n in enumerate(GROUP_SIZES)] + [np.array([-1, 5, 7, -3, 99])]).astype(np.int32)
    group = group[rng.permutation(B)]
    power = (rng.integers(0, 512, (3, K, B)) / 8.0).astype(dtype)
    spec = rng.normal(size=(3, 12, B)).astype(dtype)
    spec[:, 0] = 37
    refused = rng.random((3, B)) < 0.1
    spec[:, 0][refused] = 0
    power[np.repeat(refused[:, None, :], K, 1)] = np.nan
    return group, power, spec


@pytest.mark.parametrize("K", [1, 33])
def test_group_mirror_by_hand_and_combine(K):
    from robobee3d_amd import score as S
    group, power, spec = _group_tables(np.float64, K)
    G = len(GROUP_SIZES)
    order, offset = S.group_index_reference(group, G)
    got = S.spectrum_groups_reference(power, spec, order, offset)
    assert got.shape == (G, 3, 2 + K)
    for g, n in enumerate(GROUP_SIZES):
        mem = np.flatnonzero(group == g)
        assert len(mem) == n
        for c in range(3):
            ok = spec[c, 0, mem] > 0
            assert got[g, c, 0] == ok.sum() and got[g, c, 1] == n - ok.sum()
            assert np.array_equal(got[g, c, 2:], power[c][:, mem[ok]].sum(1))               # dyadic: exact in any order
    assert np.all(np.isfinite(got))                                                       # a refused member's NaN never enters
    # non-dyadic powers: the mirror's tree against a plain sum, to rounding
    rough = np.abs(np.random.default_rng(1).normal(size=power.shape))
    spec1 = spec.copy(); spec1[:, 0] = 1
    g2 = S.spectrum_groups_reference(rough, spec1, order, offset)
    for g in range(G):
        mem = np.flatnonzero(group == g)
        assert np.allclose(g2[g, :, 2:], rough[:, :, mem].sum(2), rtol=64 * U64 * len(mem), atol=0)
    # the column blocks of a cell add up: exactly on the dyadic tables
    half = len(group) // 2
    parts = []
    for lo, hi in ((0, half), (half, len(group))):
        o, f = S.group_index_reference(group[lo:hi], G)
        parts.append(S.spectrum_groups_reference(power[:, :, lo:hi], spec[:, :, lo:hi], o, f))
    assert np.array_equal(S.combine_spectra(parts), got) and np.array_equal(S.combine_spectra([got]), got)
    with pytest.raises(ValueError):
        S.combine_spectra([])


def test_new_exports_constants_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    decls = ("#define UMPC_SPEC_EP 0", "#define UMPC_SPEC_ES 1", "#define UMPC_SPEC_U 2", "#define UMPC_SPEC_ROWS 12", "#define UMPC_SPEC_MAX_K 64",
             "int umpcBatchSpectrumInit(umpc_batch_t *h, int K, double *sums, void *stream);",
             "int umpcBatchSpectrum(umpc_batch_t *h, int signal, const void *state_hist, const void *out_hist, const void *ref_tab, "
             "const void *ref, const double *basis, long long basis_first, int K, long long first, long long count, "
             "long long ref_first, int after, double *sums, void *stream);",
             "int umpcBatchSpectrumPower(umpc_batch_t *h, const double *sums, const double *wsum, const double *freq_hz, int K, "
             "long long nrows, int jsplit, void *power, void *spec, void *stream);",
             "int umpcBatchSpectrumGroups(umpc_batch_t *h, const void *power, const void *spec, const int32_t *order, "
             "const int32_t *offset, int G, int K, double *gspec, void *stream);")
    for decl in decls:
        assert decl in flat, decl
    # the slice count is part of the order of summation: one value in the kernel's header, the loader and the mirror
    src = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_spectrum.h")).read()
    slices = int(re.search(r"^#define UMPC_SPEC_SLICES (\d+)$", src, re.M).group(1))
    assert slices == _lib.SPEC_SLICES == S.SPEC_SLICES and slices >= 2
    assert (_lib.SPEC_EP, _lib.SPEC_ES, _lib.SPEC_U) == (S.SPEC_EP, S.SPEC_ES, S.SPEC_U) == (0, 1, 2)
    assert (_lib.SPEC_ROWS, _lib.SPEC_MAX_K) == (S.SPEC_ROWS, S.SPEC_MAX_K) == (12, 64) and len(S.SPEC_ROW_NAMES) == 12
    assert (S.SPEC_STEPS, S.SPEC_SKIPPED, S.SPEC_MEAN, S.SPEC_VAR, S.SPEC_TOTAL, S.SPEC_PEAK_BIN, S.SPEC_PEAK_HZ, S.SPEC_PEAK_POWER,
            S.SPEC_PEAK_SHARE, S.SPEC_CENTROID_HZ, S.SPEC_BANDWIDTH_HZ, S.SPEC_HIGH_SHARE) == tuple(range(12))
    scoring = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_scoring.hip")).read()
    assert '#include "umpc_spectrum.h"' in scoring
    L = _lib.lib()
    for sym in ("umpcBatchSpectrumInit", "umpcBatchSpectrum", "umpcBatchSpectrumPower", "umpcBatchSpectrumGroups"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchSpectrumInit.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchSpectrum.argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_int] + [C.c_longlong] * 3 + \
        [C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchSpectrumGroups.argtypes == [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchSpectrumInit(None, 4, None, None) == -1 and b"umpcBatchSpectrumInit" in L.umpcLastError()
    assert L.umpcBatchSpectrum(None, 0, None, None, None, None, None, 0, 4, 0, 1, 0, 0, None, None) == -1
    assert b"umpcBatchSpectrum:" in L.umpcLastError()
    assert L.umpcBatchSpectrumPower(None, None, None, None, 4, 1, 0, None, None, None) == -1 and b"umpcBatchSpectrumPower" in L.umpcLastError()
    assert L.umpcBatchSpectrumGroups(None, None, None, None, None, 1, 4, None, None) == -1 and b"umpcBatchSpectrumGroups" in L.umpcLastError()


def test_spectrum_kernels_use_no_scratch():
    """the resource remarks of the build: the sums kernel (2 dtypes x no / constant / table reference x tiles of 8 and 16), the
    power kernel (2 dtypes) and the groups kernel (2 dtypes x one or two trees) spill nothing, and their LDS is what
    csrc/resource_limits.json states: the parking of one slice, (8 + 6 KT) x 64 doubles"""
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    lds = {kt: (_lib.SPEC_SLICES - 1) * (8 + 6 * kt) * 64 * 8 for kt in (8, 16)}
    assert lds[16] == 53248 and 3 * lds[16] <= 160 * 1024                        # three blocks fit a CU
    pats = {"umpc_spectrum_kernelIfLi": 6, "umpc_spectrum_kernelIdLi": 6, "umpc_spectrum_power_kernel": 2, "umpc_spectrum_groups_kernel": 4}
    assert sorted(k for k in limits if "spectrum" in k) == sorted(["umpc_spectrum_kernel", "umpc_spectrum_power_kernel", "umpc_spectrum_groups_kernel"])
    for pat, n in pats.items():
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            want = 0 if "kernelI" not in pat else lds[16] if re.search(r"Li[012]ELi16E", k) else lds[8]
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == want, (k, res[k])
            if "kernelI" in pat:                                                 # two waves per SIMD at KT = 16, three at KT = 8
                assert res[k]["VGPRs"] + res[k]["AGPRs"] <= (256 if want == lds[16] else 168), (k, res[k])
    assert {f: x for f, x in limits["umpc_spectrum_kernel"].items() if f != "_note"} == {"ScratchSize": 0}
    for kt in (8, 16):
        pat = "Li%dEEEvNS_8SpecArgs" % kt
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds[kt]}
        assert len([k for k in res if pat in k]) == 6 and all("umpc_spectrum_kernel" in k for k in res if pat in k)
    for pat in ("umpc_spectrum_power_kernel", "umpc_spectrum_groups_kernel"):
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": 0}
    assert "53248" in limits["umpc_spectrum_kernel"]["_note"] and "28672" in limits["umpc_spectrum_kernel"]["_note"]
    # no older substring pattern counts the new kernels
    for pat in limits:
        if "spectrum" not in pat and "SpecArgs" not in pat:
            assert not [k for k in res if pat in k and "spectrum" in k], pat


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
KS = (1, 5, 8, 9, 16, 17, 33)      # across the tile boundaries of both tile sizes (8: the default, and 16)
_CACHE = {}


def _cached_tables(B, dtype):
    key = (B, dtype)
    if key not in _CACHE:
        _CACHE[key] = tuple(_noise_tables(B, np.dtype(dtype), attitude=True))
        for t in _CACHE[key]:
            t.setflags(write=False)
    return _CACHE[key]


def _dev(m, a):
    import torch
    return None if a is None else torch.as_tensor(np.array(a)).to(m.device).contiguous()


def _mpc(B, dtype):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    return BatchUprightMPC(B, getattr(torch, dtype))


def _run(m, signal, dstate, dout, dtab, dconst, dbasis, K, table, after, first=FIRST, count=COUNT, basis_first=BASIS_FIRST, sums=None):
    """umpcBatchSpectrumInit + umpcBatchSpectrum on device tensors through the C ABI"""
    import torch
    from robobee3d_amd.batch import _ptr
    rows = 2 + 3 * (2 + 2 * K)
    if sums is None:
        sums = torch.full((rows, m.B), 7.0, dtype=torch.float64, device=m.device)
        assert m.L.umpcBatchSpectrumInit(m.h, K, _ptr(sums), m._stream()) == 0
    cmd = signal == "u"
    rc = m.L.umpcBatchSpectrum(m.h, ("ep", "es", "u").index(signal), None if cmd else _ptr(dstate), _ptr(dout) if cmd else None,
                               _ptr(dtab) if table and not cmd else None, _ptr(dconst) if not table and not cmd else None,
                               _ptr(dbasis), basis_first, K, first, count, (REF_FIRST + first - FIRST) if table else 0, int(after),
                               _ptr(sums), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return sums


@pytest.mark.gpu
@pytest.mark.parametrize("B", [200, 197])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sums_kernel_bit_for_bit(dtype, B, margin):
    """every K across the tile boundaries x the three signals x table / constant reference x after 0 / 1 on one set of noise
    tables with planted NaN / Inf: the kernel's sums ARE the mirror's; columns [64, B) on a handle of their own are the same
    columns of the whole batch; 20 + 17 steps against 37 in one call; count 0, 1, 5; run to run"""
    import torch
    tables = _cached_tables(B, dtype)
    m = _mpc(B, dtype)
    ds, do, dr = [_dev(m, t) for t in tables]
    dc = _dev(m, tables[2][REF_FIRST])
    mb = _mpc(B - 64, dtype)
    bs, bo, br = [_dev(mb, t[..., 64:]) for t in tables]
    for K in KS:
        db = _dev(m, _basis(K)[0])
        for signal in ("ep", "es", "u"):
            for table, after in ((True, 0), (True, 1), (False, 0), (False, 1)) if signal != "u" else ((True, 0),):
                want = _mirror(signal, tables, table, after, K, np.dtype(dtype))
                got = _run(m, signal, ds, do, dr, dc, db, K, table, after).cpu().numpy()
                assert 1 <= want[1].sum() <= 2 and np.all(np.isfinite(want))                # the planted values are scored
                assert np.array_equal(got, want), (K, signal, table, after, np.abs(got - want).max())
        # a column block on a handle of its own
        one = _run(m, "ep", ds, do, dr, dc, db, K, True, 1)
        part = _run(mb, "ep", bs, bo, br, None, _dev(mb, _basis(K)[0]), K, True, 1)
        assert torch.equal(part, one[:, 64:]), K
        assert torch.equal(one, _run(m, "ep", ds, do, dr, dc, db, K, True, 1))               # run to run
        # chunks: the counts exact, the other rows within the bound of either order of summation
        two = _run(m, "ep", ds, do, dr, dc, db, K, True, 1, count=20)
        two = _run(m, "ep", ds, do, dr, dc, db, K, True, 1, first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=two)
        assert torch.equal(one[0:2], two[0:2])
        bound = _term_bounds("ep", tables, True, 1, K, np.dtype(dtype))
        bound[bound == 0] = np.finfo(float).tiny
        margin("K %d chunked against one call / bound" % K, float(((one[2:] - two[2:]).abs().cpu().numpy() / (2 * bound[2:])).max()), 1.0)
        chunked = _mirror("ep", tables, True, 1, K, np.dtype(dtype), count=20)
        chunked = _mirror("ep", tables, True, 1, K, np.dtype(dtype), first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=chunked)
        assert np.array_equal(two.cpu().numpy(), chunked), K
    # count = 0 changes nothing; 1 step: slice 0's tail alone; 5 steps: one full trip of both slices and a tail
    K = 17
    db = _dev(m, _basis(K)[0])
    zero = torch.zeros((2 + 3 * (2 + 2 * K), B), dtype=torch.float64, device=m.device)
    assert torch.equal(_run(m, "es", ds, do, dr, dc, db, K, True, 0, count=0), zero)
    for count in (1, 5):
        got = _run(m, "es", ds, do, dr, dc, db, K, False, 1, count=count).cpu().numpy()
        assert np.array_equal(got, _mirror("es", tables, False, 1, K, np.dtype(dtype), count=count)), count


def _power(m, sums, wsum, freq, nrows, jsplit):
    import torch
    from robobee3d_amd.batch import _ptr
    K = len(freq)
    power = torch.full((3, K, m.B), 7.0, dtype=m.dtype, device=m.device)
    spec = torch.full((3, 12, m.B), 7.0, dtype=m.dtype, device=m.device)
    wsum, freq = np.ascontiguousarray(wsum, np.float64), np.ascontiguousarray(freq, np.float64)
    rc = m.L.umpcBatchSpectrumPower(m.h, _ptr(sums), wsum.ctypes.data_as(C.POINTER(C.c_double)), freq.ctypes.data_as(C.POINTER(C.c_double)),
                                    K, nrows, jsplit, _ptr(power), _ptr(spec), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return spec.cpu().numpy(), power.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_power_kernel_on_the_mirrors_sums(dtype):
    """fp64: rows and power bit for bit, NaN meeting NaN; fp32: the mirror's rows rounded to the dtype"""
    from robobee3d_amd import score as S
    B = 197
    tables = _cached_tables(B, dtype)
    m = _mpc(B, dtype)
    for K in KS:
        basis, nu = _basis(K)
        freq = nu * 200.0
        wsum = S.spectrum_wsum(basis, BASIS_FIRST, COUNT)
        for signal, jsplit in (("ep", K // 2), ("u", K), ("es", 0)):
            sm = _mirror(signal, tables, True, 1, K, np.dtype(dtype))
            for nrows in (COUNT, COUNT - 1):                                  # (COUNT - 1: the robot with a skipped step has n = nrows)
                wspec, wpower = S.spectrum_power_reference(sm, wsum, freq, nrows, jsplit)
                gspec, gpower = _power(m, _dev(m, sm), wsum, freq, nrows, jsplit)
                assert gspec.dtype == np.dtype(dtype) and gpower.dtype == np.dtype(dtype)
                refused = wspec[:, 0] == 0
                assert refused.sum() == (3 * int((sm[1] > 0).sum()) if nrows == COUNT else 3 * B)     # still refused at COUNT - 1: skipped > 0
                assert np.array_equal(np.isnan(gpower), np.isnan(wpower)) and np.all(np.isnan(wpower) == np.repeat(refused[:, None], K, 1))
                with np.errstate(over="ignore"):
                    assert np.array_equal(gspec, wspec.astype(dtype), equal_nan=True), (K, signal, nrows)
                    assert np.array_equal(gpower, wpower.astype(dtype), equal_nan=True), (K, signal, nrows)
    # the sums kernel's own sums give the same rows
    from robobee3d_amd.batch import _ptr  # noqa: F401
    K = 16
    basis, nu = _basis(K)
    ds, do, dr = [_dev(m, t) for t in tables]
    sums = _run(m, "ep", ds, do, dr, None, _dev(m, basis), K, True, 1)
    wsum = S.spectrum_wsum(basis, BASIS_FIRST, COUNT)
    gspec, gpower = _power(m, sums, wsum, nu * 200.0, COUNT, 8)
    wspec, wpower = S.spectrum_power_reference(_mirror("ep", tables, True, 1, K, np.dtype(dtype)), wsum, nu * 200.0, COUNT, 8)
    assert np.array_equal(gspec, wspec.astype(dtype), equal_nan=True) and np.array_equal(gpower, wpower.astype(dtype), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 32, 33, 64])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_groups_kernel_bit_for_bit(dtype, K):
    """groups of 1, 3, 64, 65 and 130 scattered members and robots in no group; dyadic and rough powers"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import _ptr
    group, power, spec = _group_tables(np.dtype(dtype), K)
    G = len(GROUP_SIZES)
    m = _mpc(len(group), dtype)
    index = m.group_index(group, G)
    order, offset = index[0].cpu().numpy(), index[1].cpu().numpy()
    rough = np.where(np.isnan(power), np.nan, np.abs(np.random.default_rng(K).normal(size=power.shape))).astype(dtype)
    for pw in (power, rough):
        want = S.spectrum_groups_reference(pw, spec, order, offset)
        gspec = torch.full((G, 3, 2 + K), 7.0, dtype=torch.float64, device=m.device)
        dpw, dspec = _dev(m, pw), _dev(m, spec)
        rc = m.L.umpcBatchSpectrumGroups(m.h, _ptr(dpw), _ptr(dspec), _ptr(index[0]), _ptr(index[1]), G, K, _ptr(gspec), m._stream())
        assert rc == 0, m.L.umpcLastError()
        assert np.array_equal(gspec.cpu().numpy(), want)
        assert torch.equal(m.spectrum_groups(dpw, dspec, index), gspec)
    assert want[:, :, 0].sum() + want[:, :, 1].sum() == 3 * sum(GROUP_SIZES)


@pytest.mark.gpu
def test_end_to_end_spectrum_of_a_rollout():
    """helix at 5 Hz over B = 128 as two contiguous cells of 64, 48 recorded steps in fp32: spectrum() and spectrum_groups()
    against the mirrors on the downloaded history, for the three signals; a chunked run; argument errors"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, W, dtype = 128, 48, "float32"
    m = _mpc(B, dtype)
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    tab = m.task_table(W, "helix", trajAmp=20.0, trajFreq=np.full(B, 5.0), useY=False)
    m.set_reference_trajectory(tab)
    m.record_history(W)
    m.rollout(W)
    hist = m.history()
    hs, ho, ht = hist["state"].cpu().numpy(), hist["out"].cpu().numpy(), tab.cpu().numpy()
    freq = np.array([5.0, 10.0, 20.0, 35.0, 50.0, 80.0])
    nu = S.response_nu(freq, int(m.prm.nsub), float(m.prm.dtsim))
    basis = S.spectrum_basis(nu, W, "hann")
    wsum = S.spectrum_wsum(basis)
    index = m.group_index(np.repeat(np.arange(2, dtype=np.int32), 64), 2)
    order, offset = index[0].cpu().numpy(), index[1].cpu().numpy()
    for signal in ("ep", "es", "u"):
        spec, power, sums = m.spectrum(freq, signal, after=True, split_hz=30.0)
        assert tuple(spec.shape) == (3, 12, B) and spec.dtype == torch.float32 and tuple(power.shape) == (3, 6, B)
        assert tuple(sums.shape) == (2 + 3 * 14, B) and sums.dtype == torch.float64
        want = S.spectrum_sums_reference(signal, hs, ho, ht, basis, 0, 0, W, 0, True, np.float32)
        assert np.all(want[0] == W) and np.array_equal(sums.cpu().numpy(), want), signal
        wspec, wpower = S.spectrum_power_reference(want, wsum, freq, W, 3)
        with np.errstate(over="ignore"):
            assert np.array_equal(spec.cpu().numpy(), wspec.astype(np.float32), equal_nan=True), signal
            assert np.array_equal(power.cpu().numpy(), wpower.astype(np.float32), equal_nan=True), signal
        gs = m.spectrum_groups(power, spec, index)
        assert np.array_equal(gs.cpu().numpy(), S.spectrum_groups_reference(power.cpu().numpy(), spec.cpu().numpy(), order, offset))
        print("%s: cell-averaged periodogram, channel 0: %s" % (signal, (gs[:, 0, 2:] / gs[:, 0, 0:1]).cpu().numpy()))
    # spec[c] is shaped as a score: a cell's median chatter score through score_quantiles, unchanged
    spec, power, sums = m.spectrum(freq, "ep", after=True, split_hz=30.0)
    q = m.score_quantiles(spec[0], index, [0.5], S.SPEC_HIGH_SHARE).cpu().numpy()
    assert np.array_equal(q, S.score_quantiles_reference(spec[0].cpu().numpy(), order, offset, [0.5], S.SPEC_HIGH_SHARE))
    # chunks: steps 0..19, then 20..47 on the basis of the whole window
    db = torch.as_tensor(basis).to(m.device)
    none, nopow, part = m.spectrum(freq, "ep", first=0, count=20, after=True, basis=db, power=False)
    assert none is None and nopow is None
    spec2, power2, part = m.spectrum(freq, "ep", first=20, count=28, after=True, basis=db, basis_first=20, sums=part, split_hz=30.0)
    assert torch.equal(part[0:2], sums[0:2]) and torch.all(spec2[:, 0] == W)
    assert torch.allclose(power2, power, rtol=1e-5, atol=1e-6 * float(power.max()))
    for bad in (dict(freq_hz=[0.0]), dict(freq_hz=[100.0]), dict(freq_hz=np.arange(65) + 1.0), dict(count=W + 1), dict(signal="tau"),
                dict(sums=torch.zeros((44, B), device=m.device)), dict(basis=db, basis_first=1), dict(freq_hz=[20.0, 5.0], split_hz=10.0),
                dict(basis_first=3), dict(window="blackman")):
        kw = dict(freq_hz=freq, signal="ep")
        kw.update(bad)
        with pytest.raises(ValueError):
            m.spectrum(**kw)


@pytest.mark.gpu
def test_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    K = 4
    state = torch.zeros((5, 18, 64), device=m.device)
    out = torch.zeros((4, 9, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((4, 9, 64), device=m.device)
    basis = torch.ones((4, 1 + 2 * K), dtype=torch.float64, device=m.device)
    sums = torch.full((2 + 3 * (2 + 2 * K), 64), 3.0, dtype=torch.float64, device=m.device)
    keep = sums.clone()
    ok = dict(signal=0, state=P(state), out=P(out), tab=None, ref=P(ref), basis=P(basis), basis_first=0, K=K, first=0, count=4,
              ref_first=0, sums=P(sums))
    call = lambda a: L.umpcBatchSpectrum(h, a["signal"], a["state"], a["out"], a["tab"], a["ref"], a["basis"], a["basis_first"], a["K"],
                                         a["first"], a["count"], a["ref_first"], 0, a["sums"], s)
    for bad in (dict(count=-1), dict(count=(1 << 31) - 4), dict(first=-1), dict(ref_first=-1), dict(basis_first=-1), dict(K=0), dict(K=65),
                dict(signal=3), dict(signal=-1), dict(tab=P(tab)), dict(ref=None), dict(basis=None), dict(sums=None), dict(state=None),
                dict(signal=2, out=None)):
        assert call(dict(ok, **bad)) == -1 and b"umpcBatchSpectrum:" in L.umpcLastError(), bad
    assert L.umpcBatchSpectrumInit(h, K, None, s) == -1 and L.umpcBatchSpectrumInit(h, 0, P(sums), s) == -1
    assert L.umpcBatchSpectrumInit(h, 65, P(sums), s) == -1 and b"umpcBatchSpectrumInit" in L.umpcLastError()
    power = torch.zeros((3, K, 64), device=m.device)
    spec = torch.zeros((3, 12, 64), device=m.device)
    wsum = (C.c_double * (1 + 2 * K))(*([4.0] + [0.0] * (2 * K)))
    freq = (C.c_double * K)(1.0, 2.0, 3.0, 4.0)
    pw = lambda su=P(sums), ws=wsum, fr=freq, k=K, nrows=4, jsplit=2, po=P(power), sp=P(spec): L.umpcBatchSpectrumPower(h, su, ws, fr, k, nrows, jsplit, po, sp, s)
    for bad in (dict(su=None), dict(ws=None), dict(fr=None), dict(po=None), dict(sp=None), dict(k=0), dict(k=65), dict(nrows=-1), dict(jsplit=-1),
                dict(jsplit=K + 1)):
        assert pw(**bad) == -1 and b"umpcBatchSpectrumPower" in L.umpcLastError(), bad
    index = m.group_index(np.zeros(64, np.int32), 1)
    gspec = torch.full((1, 3, 2 + K), 5.0, dtype=torch.float64, device=m.device)
    gr = lambda po=P(power), sp=P(spec), o=P(index[0]), f=P(index[1]), G=1, k=K, gs=P(gspec): L.umpcBatchSpectrumGroups(h, po, sp, o, f, G, k, gs, s)
    for bad in (dict(po=None), dict(sp=None), dict(o=None), dict(f=None), dict(gs=None), dict(G=0), dict(k=0), dict(k=65)):
        assert gr(**bad) == -1 and b"umpcBatchSpectrumGroups" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert torch.equal(sums, keep) and torch.all(power == 0) and torch.all(spec == 0) and torch.all(gspec == 5.0)      # nothing was launched
    # the same calls with good arguments go through: count = 0 changes nothing, a call adds into the sums; the command
    # needs neither state nor reference
    assert call(dict(ok, count=0)) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, keep)
    assert call(ok) == 0 and call(dict(ok, signal=2, state=None, ref=None)) == 0
    torch.cuda.synchronize()
    assert torch.all(sums[0] == 11.0) and torch.all(sums[1] == 3.0) and torch.all(sums[2] == 3.0)
    assert pw() == 0 and gr() == 0
    torch.cuda.synchronize()
    assert torch.all(spec[:, 0] == 0) and torch.all(torch.isnan(power)) and torch.all(gspec[:, :, 0] == 0) and torch.all(gspec[:, :, 1] == 64)
