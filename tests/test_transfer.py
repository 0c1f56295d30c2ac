"""Transfer estimates (umpcBatchCrossSpectrumInit / umpcBatchCrossSpectrum / umpcBatchCrossSpectrumGroups / umpcBatchTransfer;
csrc/umpc_transfer.h, score.py cross_spectrum_* / transfer_rows_reference, BatchUprightMPC.transfer).

CPU: the numpy mirrors against planted systems -- a FIR filter, a pure delay, independent signals --, the identities between
the rows, the refusals, the group order by hand, the existing spectrum mirror, the exports and the resource record of the
build. GPU: the three kernels against the mirrors bit for bit (the phase within PHASE_BOUND), one closed-loop run end to
end, every argument rule of the header."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
# rows kernel against the mirror, the phase row: the largest deviation in rad measured on the first GPU run; asserted at
# 16 x that value and never looser than the fp64 cap of test_response.py
PHASE_MEASURED = 4.441e-16
PHASE_CAP = 1e-10
PHASE_BOUND = min(16 * PHASE_MEASURED, PHASE_CAP)

FIR_BINS = (1, 2, 3, 5, 8, 13, 21, 23)


def _track_tables(x, y):
    """state [W + 1, 18, B] and reference table [W, 9, B] whose tracking pair is (x, y) [W, 3, B] with after = 0"""
    W, _, B = x.shape
    state, ref = np.zeros((W + 1, 18, B)), np.zeros((W, 9, B))
    ref[:, 0:3], state[:W, 0:3] = x, y
    return state, ref


def _transfer_of(x, y, nu, window="rect", group=None, G=1):
    """(tf, gx, sums) of the mirrors for the tracking pair (x, y) [W, 3, B]; one cell of all draws unless `group` says else"""
    from robobee3d_amd import score as S
    W, _, B = x.shape
    state, ref = _track_tables(x, y)
    basis = S.spectrum_basis(nu, W, window)
    sums = S.cross_spectrum_sums_reference("track", state, ref, None, basis, 0, 0, W, 0, 0, False)
    order, offset = S.group_index_reference(np.zeros(B, np.int32) if group is None else group, G)
    gx = S.cross_spectrum_groups_reference(sums, S.spectrum_wsum(basis), W, order, offset)
    return S.transfer_rows_reference(gx), gx, sums


def _angle_between(a, b):
    """|a - b| in rad on the circle"""
    return np.abs(np.angle(np.exp(1j * (np.asarray(a) - np.asarray(b)))))


def _white(W, B, seed):
    return np.random.default_rng(seed).normal(size=(W, 3, B))


def test_planted_fir_filter():
    """y = h * x circularly on on-grid frequencies of a rect window: H1 is the filter's frequency response and coh is 1, both
    within 1e-12 relative; the offsets of x and y do not enter"""
    from robobee3d_amd import score as S
    W, B = 48, 64
    nu = np.array(FIR_BINS) / W
    h = (0.5, 0.3, -0.2, 0.1)
    x = _white(W, B, 11)
    y = sum(hl * np.roll(x, l, 0) for l, hl in enumerate(h))
    tf, gx, _ = _transfer_of(x + 3.0, y - 2.0, nu)
    want = sum(hl * np.exp(-2j * np.pi * nu * l) for l, hl in enumerate(h))                  # [K]
    got = tf[0, :, :, S.TF_H_RE] + 1j * tf[0, :, :, S.TF_H_IM]                               # [3, K]
    assert np.all(tf[..., S.TF_N] == B) and np.all(tf[..., S.TF_SKIPPED] == 0)
    assert (np.abs(got - want) / np.abs(want)).max() <= 1e-12
    assert np.abs(tf[..., S.TF_COH] - 1).max() <= 1e-12
    assert (np.abs(tf[0, :, :, S.TF_GAIN] - np.abs(want)) / np.abs(want)).max() <= 1e-12
    assert _angle_between(tf[0, :, :, S.TF_PHASE], np.angle(want)).max() <= 1e-12
    # the same system without the offsets: the same rows to rounding
    tf0, _, _ = _transfer_of(x, y, nu)
    assert (np.abs(tf0[0, :, :, S.TF_H_RE] + 1j * tf0[0, :, :, S.TF_H_IM] - got) / np.abs(want)).max() <= 1e-12
    # Pxx is the averaged periodogram of x in spectrum()'s units
    X = np.fft.fft(x, axis=0)[list(FIR_BINS)]                                                # [K, 3, B]
    pxx = (4.0 * np.abs(X) ** 2 / W ** 2).mean(2).T
    assert np.allclose(tf0[0, :, :, S.TF_PXX], pxx, rtol=1e-12, atol=0)


def test_pure_delay_has_gain_one_and_negative_phase():
    from robobee3d_amd import score as S
    W, B = 48, 64
    nu = np.array(FIR_BINS) / W
    x = _white(W, B, 12)
    tf, _, _ = _transfer_of(x, np.roll(x, 3, 0), nu)
    want = -2 * np.pi * nu * 3                                                              # (compared on the circle: bin 8 sits at -pi)
    assert np.abs(tf[0, :, :, S.TF_GAIN] - 1).max() <= 1e-12 and np.abs(tf[0, :, :, S.TF_GAIN_H2] - 1).max() <= 1e-12
    assert _angle_between(tf[0, :, :, S.TF_PHASE], want).max() <= 1e-12
    assert np.array_equal(tf[0, :, :3, S.TF_PHASE] < 0, np.ones((3, 3), bool)) and np.abs(tf[0, :, :3, S.TF_PHASE] - want[:3]).max() <= 1e-12                                              # a lag is a negative phase
    assert np.all(tf[0, :, :, S.TF_H_IM][:, :3] < 0)


def test_independent_signals_have_low_coherence():
    """coh of independent x and y follows Beta(1, n - 1): P(coh > 0.2) = 0.8^63 = 8e-7 per bin with 64 draws"""
    from robobee3d_amd import score as S
    W, B = 48, 64
    nu = np.array(FIR_BINS) / W
    tf, _, _ = _transfer_of(_white(W, B, 13), _white(W, B, 14), nu)
    assert np.all(tf[..., S.TF_N] == B)
    assert tf[..., S.TF_COH].max() < 0.2 and tf[..., S.TF_COH].min() >= 0
    assert np.all(tf[..., S.TF_REL_ERR] > 0.1) and np.all(np.isfinite(tf))


def test_identities_between_the_rows():
    """gain <= gain_h2 and coh = gain / gain_h2; noise = Pyy (1 - coh); a filter with output noise on a Hann window"""
    from robobee3d_amd import score as S
    W, B = 48, 64
    nu = (np.arange(8) + 0.7) / 17.0
    x = _white(W, B, 15)
    y = 0.7 * np.roll(x, 1, 0) - 0.2 * np.roll(x, 2, 0) + 0.5 * _white(W, B, 16)
    tf, gx, _ = _transfer_of(x + 1.0, y, nu, "hann")
    g1, g2, coh = tf[..., S.TF_GAIN], tf[..., S.TF_GAIN_H2], tf[..., S.TF_COH]
    assert np.all(g1 <= g2) and np.all(coh > 0) and np.all(coh < 1)
    assert (np.abs(coh - g1 / g2) / coh).max() <= 16 * U64                                   # (seven roundings between the two)
    assert np.allclose(tf[..., S.TF_GAIN], np.hypot(tf[..., S.TF_H_RE], tf[..., S.TF_H_IM]), rtol=16 * U64, atol=0)
    assert np.array_equal(tf[..., S.TF_NOISE], tf[..., S.TF_PYY] * (1.0 - coh))
    assert np.array_equal(tf[..., S.TF_REL_ERR], np.sqrt((1.0 - coh) / ((2.0 * B) * coh)))
    four = gx[:, :, 2:].reshape(1, 3, 8, 4)
    assert np.array_equal(tf[..., S.TF_PXX], four[..., S.GX_SXX] / B) and np.array_equal(tf[..., S.TF_PYY], four[..., S.GX_SYY] / B)
    assert np.array_equal(tf[..., S.TF_PHASE], np.arctan2(four[..., S.GX_QXY], four[..., S.GX_CXY]))


def test_a_cell_of_one_member_is_refused():
    """one record's coherence is identically 1: there is nothing to estimate"""
    from robobee3d_amd import score as S
    W, B = 48, 65
    nu = np.array(FIR_BINS) / W
    x, y = _white(W, B, 17), _white(W, B, 18)
    group = np.zeros(B, np.int32)
    group[64] = 1
    tf, gx, _ = _transfer_of(x, y, nu, group=group, G=2)
    assert np.all(gx[0, :, 0] == 64) and np.all(gx[1, :, 0] == 1) and np.all(gx[:, :, 1] == 0)
    assert np.all(tf[0, ..., S.TF_N] == 64) and np.all(np.isfinite(tf[0]))
    assert np.all(tf[1, ..., S.TF_N] == 0) and np.all(tf[1, ..., S.TF_SKIPPED] == 0) and np.all(np.isnan(tf[1, ..., 2:]))
    # the one record alone WOULD have coherence 1: the refusal is what keeps that number out of a table
    four = gx[1, :, 2:].reshape(3, len(nu), 4)
    m2 = four[..., 2] ** 2 + four[..., 3] ** 2
    assert np.allclose(m2 / (four[..., 0] * four[..., 1]), 1.0, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------------------------
# tables for the semantics and the GPU tests
# ------------------------------------------------------------------------------------------------------------------
FIRST, COUNT, REF_FIRST, IMP_FIRST, BASIS_FIRST = 3, 37, 5, 4, 2
# (pair, reference table?) -> robots with one skipped step in _noise_tables
PLANTED = {("track", True): (7, 71), ("att", True): (33, 70), ("push", True): (7, 71, 130), ("push", False): (7, 130)}


def _noise_tables(B, dtype, seed=20250607, clean=False):
    """Seeded noise tables: state [44, 18, B], ref [46, 9, B], impulses [45, 6, B] in `dtype`, with a NaN in robot 7's position,
    an Inf in robot 33's attitude, an Inf in robot 70's reference attitude and in robot 71's reference position, and a NaN in
    robot 130's push (none with `clean`)"""
    rng = np.random.default_rng(seed + B)
    state = rng.normal(size=(44, 18, B))
    ref = rng.normal(size=(46, 9, B))
    imp = rng.normal(size=(45, 6, B))
    if not clean:
        state[12, 1, 7] = np.nan
        state[15, 10, 33] = np.inf
        ref[20, 7, 70] = np.inf
        ref[21, 1, 71] = -np.inf
        imp[15, 2, 130] = np.nan
    return state.astype(dtype), ref.astype(dtype), imp.astype(dtype)


def _basis(K, window="hann"):
    from robobee3d_amd import score as S
    nu = (np.arange(K) + 0.7) / (2.0 * K + 1.0)                         # K frequencies inside (0, 0.5)
    return S.spectrum_basis(nu, BASIS_FIRST + COUNT + 3, window, step0=1000), nu


def _mirror(pair, tables, table, after, K, dtype, first=FIRST, count=COUNT, basis_first=BASIS_FIRST, sums=None):
    from robobee3d_amd import score as S
    state, ref, imp = tables
    r = ref if table else np.ascontiguousarray(ref[REF_FIRST])
    return S.cross_spectrum_sums_reference(pair, state, r, imp, _basis(K)[0], basis_first, first, count,
                                           (REF_FIRST + first - FIRST) if table else 0, IMP_FIRST + first - FIRST, after, dtype, sums)


def test_semantics_of_the_sums_mirror():
    from robobee3d_amd import score as S
    B, K = 140, 5
    tables = _noise_tables(B, np.float64)
    clean = [t.copy() for t in tables]
    clean[0][12, 1, 7] = 0.25; clean[0][15, 10, 33] = -0.75; clean[1][20, 7, 70] = -0.5; clean[1][21, 1, 71] = 0.5; clean[2][15, 2, 130] = 0.125
    basis, nu = _basis(K)
    rows = 2 + 6 * (2 + 2 * K)
    assert S.cross_spectrum_sum_rows(K) == rows and S.cross_spectrum_identity(K, B).shape == (rows, B)
    wsum = S.spectrum_wsum(basis, BASIS_FIRST, COUNT)
    group = np.arange(B, dtype=np.int32) % 2
    order, offset = S.group_index_reference(group, 2)
    # a planted NaN / Inf step in each of the three tables: `skipped` counts it, BOTH signals receive +0 for it, the member
    # does not enter its cell; the other robots are bit-unchanged
    for (pair, table), robots in PLANTED.items():
        for after in (0, 1):
            got = _mirror(pair, tables, table, after, K, np.float64)
            want = _mirror(pair, clean, table, after, K, np.float64)
            others = ~np.isin(np.arange(B), robots)
            assert got[1].tolist() == [float(b in robots) for b in range(B)], (pair, table)
            assert np.all(got[0] + got[1] == COUNT) and np.all(np.isfinite(got)) and np.array_equal(got[:, others], want[:, others])
            gx = S.cross_spectrum_groups_reference(got, wsum, COUNT, order, offset)
            gw = S.cross_spectrum_groups_reference(want, wsum, COUNT, order, offset)
            for g in range(2):
                out = sum(1 for b in robots if b % 2 == g)
                assert np.all(gx[g, :, 0] == B // 2 - out) and np.all(gx[g, :, 1] == out) and np.all(gw[g, :, 0] == B // 2)
            # the skipped member's value is +0 in the products of BOTH signals: its x blocks differ from the clean ones too
            for b in robots:
                assert not np.array_equal(got[2:2 + 3 * (2 + 2 * K), b], want[2:2 + 3 * (2 + 2 * K), b])
                assert not np.array_equal(got[2 + 3 * (2 + 2 * K):, b], want[2 + 3 * (2 + 2 * K):, b])
    # what a pair does not read may be anything
    junk = [t.copy() for t in clean]
    junk[0][:, 3:9] = np.nan; junk[0][:, 12:] = np.inf; junk[1][:, 3:6] = np.nan; junk[2][:, 3:6] = np.nan
    for pair, table in PLANTED:
        assert np.array_equal(_mirror(pair, junk, table, 1, K, np.float64), _mirror(pair, clean, table, 1, K, np.float64))
    assert np.array_equal(S.cross_spectrum_sums_reference("track", clean[0], clean[1], None, basis, BASIS_FIRST, FIRST, COUNT, REF_FIRST, 0, True),
                          _mirror("track", clean, True, 1, K, np.float64))
    # after = 1 is after = 0 on the state moved by one slice; a constant reference is its table; the pairs differ
    a1 = _mirror("push", clean, True, 1, K, np.float64)
    assert np.array_equal(a1, _mirror("push", [clean[0][1:], clean[1], clean[2]], True, 0, K, np.float64))
    rep = [clean[0], np.repeat(clean[1][REF_FIRST:REF_FIRST + 1], 46, 0), clean[2]]
    assert np.array_equal(_mirror("push", clean, False, 0, K, np.float64), _mirror("push", rep, True, 0, K, np.float64))
    assert not np.array_equal(a1, _mirror("track", clean, True, 1, K, np.float64))
    assert not np.array_equal(_mirror("att", clean, True, 1, K, np.float64), _mirror("track", clean, True, 1, K, np.float64))
    # the difference of the push pair is formed in the handle's dtype
    t32 = [t.astype(np.float32) for t in clean]
    d32 = [np.zeros_like(clean[0]), np.zeros_like(clean[1]), t32[2].astype(np.float64)]
    d32[0][FIRST:FIRST + COUNT, 0:3] = (t32[0][FIRST:FIRST + COUNT, 0:3] - t32[1][REF_FIRST:REF_FIRST + COUNT, 0:3]).astype(np.float64)
    assert np.array_equal(_mirror("push", t32, True, 0, K, np.float32), _mirror("push", d32, True, 0, K, np.float64))
    # n != nrows: nobody enters, every row is refused; n < 2 likewise
    full = _mirror("track", clean, True, 0, K, np.float64)
    gbad = S.cross_spectrum_groups_reference(full, wsum, COUNT + 1, order, offset)
    assert np.all(gbad[:, :, 0] == 0) and np.all(gbad[:, :, 1] == B // 2) and np.all(gbad[:, :, 2:] == 0)
    tbad = S.transfer_rows_reference(gbad)
    assert np.all(tbad[..., 0] == 0) and np.all(tbad[..., 1] == B // 2) and np.all(np.isnan(tbad[..., 2:]))
    one = _mirror("track", clean, True, 0, K, np.float64, count=1)
    g1 = S.cross_spectrum_groups_reference(one, S.spectrum_wsum(basis, BASIS_FIRST, 1), 1, order, offset)
    assert np.all(g1[:, :, 0] == 0) and np.all(g1[:, :, 1] == B // 2)
    # an input without power in one channel: Sxx = 0 there, the row is refused; the other channels are bit-unchanged
    flat = [clean[0], clean[1].copy(), clean[2]]
    flat[1][:, 1] = 0.25                                                                  # a constant: its mean is removed
    flat[1][:, 2] = 0.0
    tf_flat = S.transfer_rows_reference(S.cross_spectrum_groups_reference(_mirror("track", flat, True, 0, K, np.float64), wsum, COUNT, order, offset))
    tf_full = S.transfer_rows_reference(S.cross_spectrum_groups_reference(full, wsum, COUNT, order, offset))
    assert np.all(tf_flat[:, 2, :, 0] == 0) and np.all(np.isnan(tf_flat[:, 2, :, 2:])) and np.all(tf_flat[:, 2, :, 1] == 0)
    assert np.array_equal(tf_flat[:, 0], tf_full[:, 0]) and np.all(tf_full[..., 0] == B // 2) and np.all(np.isfinite(tf_full))
    assert np.all(~(tf_flat[:, 1, :, S.TF_PXX] > 1e-28))                                   # rounding dust at the most: Pxx reveals it
    # an output without power: H1 stands (zero), rows 8..11 are NaN
    quiet = [clean[0].copy(), clean[1], clean[2]]
    quiet[0][:, 0] = 0.0
    tf_q = S.transfer_rows_reference(S.cross_spectrum_groups_reference(_mirror("track", quiet, True, 0, K, np.float64), wsum, COUNT, order, offset))
    assert np.all(tf_q[:, 0, :, 0] == B // 2) and np.all(tf_q[:, 0, :, S.TF_GAIN] == 0) and np.all(np.isnan(tf_q[:, 0, :, 8:]))
    # a sum that is not finite refuses its row alone
    ginf = S.cross_spectrum_groups_reference(full, wsum, COUNT, order, offset)
    ginf[1, 2, 2 + 4 * 3 + 2] = np.inf
    tinf = S.transfer_rows_reference(ginf)
    assert tinf[1, 2, 3, 0] == 0 and np.all(np.isnan(tinf[1, 2, 3, 2:])) and np.all(np.isfinite(np.delete(tinf[1, 2], 3, 0)))
    # chunks of 20 + 17 steps against 37 undivided: the counts equal, the other rows to rounding
    part = _mirror("push", tables, True, 1, K, np.float64, count=20)
    part = _mirror("push", tables, True, 1, K, np.float64, first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=part)
    whole = _mirror("push", tables, True, 1, K, np.float64)
    assert np.array_equal(part[0:2], whole[0:2]) and not np.array_equal(part, whole)
    amax = max(np.abs(t[np.isfinite(t)]).max() for t in tables)                               # |v| <= 2 amax, a term <= 4 amax^2
    assert np.allclose(part, whole, rtol=0, atol=2 * (COUNT + 4) * U64 * COUNT * 4 * amax ** 2)
    assert np.array_equal(_mirror("push", tables, True, 1, K, np.float64, count=0), S.cross_spectrum_identity(K, B))
    assert np.array_equal(_mirror("push", tables, True, 1, K, np.float64, count=0, sums=whole), whole)
    # refused arguments
    state, ref, imp = clean
    with pytest.raises(ValueError):
        S.cross_spectrum_sums_reference("track", state, ref[REF_FIRST], None, basis, 0, 0, 4, 0, 0, False)   # a constant reference has no spectrum
    with pytest.raises(ValueError):
        S.cross_spectrum_sums_reference("att", state, ref[REF_FIRST], None, basis, 0, 0, 4, 0, 0, False)
    with pytest.raises(ValueError):
        S.cross_spectrum_sums_reference("push", state, ref, None, basis, 0, 0, 4, 0, 0, False)             # no impulse table
    with pytest.raises(ValueError):
        S.cross_spectrum_sums_reference("push", state, None, imp, basis, 0, 0, 4, 0, 0, False)
    with pytest.raises(ValueError):
        S.cross_spectrum_sums_reference("ep", state, ref, imp, basis, 0, 0, 4, 0, 0, False)
    with pytest.raises(ValueError):
        _mirror("track", clean, True, 1, K, np.float64, sums=np.zeros((rows + 2, B)))
    with pytest.raises(ValueError):
        _mirror("track", clean, True, 1, K, np.float64, basis_first=BASIS_FIRST + 4)           # the basis ends before the call
    for k in (0, 65):
        with pytest.raises(ValueError):
            S.cross_spectrum_sum_rows(k)
    with pytest.raises(ValueError):
        S.cross_spectrum_groups_reference(full, wsum[:-2], COUNT, order, offset)
    with pytest.raises(ValueError):
        S.transfer_rows_reference(np.zeros((2, 3, 2 + 4 * K + 1)))
    with pytest.raises(ValueError):
        S.transfer_rows_reference(np.zeros((2, 2, 2 + 4 * K)))
    with pytest.raises(ValueError):
        S.combine_cross_spectra([])


def test_track_y_blocks_are_the_spectrum_mirrors_channels():
    """on tables without a hole the y blocks of the tracking pair equal spectrum_sums_reference("ep") against a zero reference,
    and the x blocks the same mirror on the reference table against zero, bit for bit"""
    from robobee3d_amd import score as S
    B = 70
    for dtype in (np.float64, np.float32):
        state, ref, imp = _noise_tables(B, dtype, clean=True)
        for K in (1, 5, 9):
            basis = _basis(K)[0]
            chan = 2 + 2 * K
            for after in (0, 1):
                xs = _mirror("track", (state, ref, imp), True, after, K, dtype)
                sp = S.spectrum_sums_reference("ep", state, None, np.zeros((9, B), dtype), basis, BASIS_FIRST, FIRST, COUNT, 0, after, dtype)
                assert np.array_equal(xs[2 + 3 * chan:], sp[2:]) and np.array_equal(xs[0:2], sp[0:2])
                asx = np.zeros((46, 18, B), dtype)
                asx[:, 0:3] = ref[:, 0:3]
                sx = S.spectrum_sums_reference("ep", asx, None, np.zeros((9, B), dtype), basis, BASIS_FIRST, REF_FIRST, COUNT, 0, 0, dtype)
                assert np.array_equal(xs[2:2 + 3 * chan], sx[2:])


GROUP_SIZES = (1, 3, 64, 65, 130)


def _group_sums(K, seed=9, exact=True):
    """B = 268: groups of 1, 3, 64, 65 and 130 members scattered over the batch, 5 robots in no group; sums [2 + 6 (2 + 2 K), B]
    of small integers with W0 = 2 and integer Wc, Ws (`exact`: every mean, product and partial sum is an integer, every
    order of summation exact) or of noise; nrows = 8; about a tenth of the members do not enter (a skipped step, or another n)"""
    rng = np.random.default_rng(seed + K)
    B = sum(GROUP_SIZES) + 5
    group = np.concatenate([np.full(n, g) for g, n in enumerate(GROUP_SIZES)] + [np.array([-1, 5, 7, -3, 99])]).astype(np.int32)
    group = group[rng.permutation(B)]
    rows = 2 + 6 * (2 + 2 * K)
    if exact:
        sums = rng.integers(-6, 7, (rows, B)).astype(np.float64)
        for c in range(6):
            sums[2 + c * (2 + 2 * K)] *= 2.0                                                 # sum w v even: m = sum w v / 2 is an integer
        wsum = np.concatenate(([2.0], rng.integers(-2, 3, 2 * K).astype(np.float64)))
    else:
        sums = rng.normal(size=(rows, B))
        wsum = np.concatenate(([3.7], 0.1 * rng.normal(size=2 * K)))
    sums[0], sums[1] = 8.0, 0.0
    out = rng.random(B)
    sums[1, out < 0.05] = 1.0
    sums[0, (out >= 0.05) & (out < 0.1)] = 7.0
    return group, sums, wsum, 8


@pytest.mark.parametrize("K", [1, 9])
def test_group_mirror_by_hand_and_combine(K):
    from robobee3d_amd import score as S
    group, sums, wsum, nrows = _group_sums(K)
    G = len(GROUP_SIZES)
    order, offset = S.group_index_reference(group, G)
    got = S.cross_spectrum_groups_reference(sums, wsum, nrows, order, offset)
    assert got.shape == (G, 3, 2 + 4 * K)
    chan = 2 + 2 * K
    enters = (sums[1] == 0) & (sums[0] == nrows)
    assert 0 < (~enters).sum() < len(group) // 4
    for g, n in enumerate(GROUP_SIZES):
        mem = np.flatnonzero(group == g)
        assert len(mem) == n
        ok = mem[enters[mem]]
        for c in range(3):
            xs, ys = sums[2 + c * chan:2 + (c + 1) * chan, ok], sums[2 + (3 + c) * chan:2 + (4 + c) * chan, ok]
            assert got[g, c, 0] == len(ok) and got[g, c, 1] == n - len(ok)
            for j in range(K):
                ax, bx = xs[2 + 2 * j] - xs[0] / 2 * wsum[1 + 2 * j], xs[3 + 2 * j] - xs[0] / 2 * wsum[2 + 2 * j]
                ay, by = ys[2 + 2 * j] - ys[0] / 2 * wsum[1 + 2 * j], ys[3 + 2 * j] - ys[0] / 2 * wsum[2 + 2 * j]
                hand = [(ax * ax + bx * bx).sum(), (ay * ay + by * by).sum(), (ax * ay + bx * by).sum(), (bx * ay - ax * by).sum()]
                assert got[g, c, 2 + 4 * j:6 + 4 * j].tolist() == hand, (g, c, j)               # integers: exact in any order
    assert np.all(np.isfinite(got))
    # noise: the mirror's tree against a plain sum of the same terms, to rounding
    group2, rough, wsum2, _ = _group_sums(K, exact=False)
    g2 = S.cross_spectrum_groups_reference(rough, wsum2, nrows, order, offset)
    ent2 = (rough[1] == 0) & (rough[0] == nrows)
    for g in range(G):
        mem = np.flatnonzero(group2 == g)
        ok = mem[ent2[mem]]
        for c in range(3):
            xs, ys = rough[2 + c * chan:2 + (c + 1) * chan, ok], rough[2 + (3 + c) * chan:2 + (4 + c) * chan, ok]
            X = (xs[2::2] - xs[0] / wsum2[0] * wsum2[1::2, None]) - 1j * (xs[3::2] - xs[0] / wsum2[0] * wsum2[2::2, None])
            Y = (ys[2::2] - ys[0] / wsum2[0] * wsum2[1::2, None]) - 1j * (ys[3::2] - ys[0] / wsum2[0] * wsum2[2::2, None])
            s = 4.0 / wsum2[0] ** 2
            cross = (np.conj(X) * Y).sum(1) * s
            want = np.stack(((np.abs(X) ** 2).sum(1) * s, (np.abs(Y) ** 2).sum(1) * s, cross.real, cross.imag), 1).reshape(-1)
            scale = np.repeat(np.sqrt((np.abs(X) ** 2).sum(1) * (np.abs(Y) ** 2).sum(1)) * s + want.reshape(K, 4)[:, :2].max(1), 4)
            assert np.all(np.abs(g2[g, c, 2:] - want) <= 64 * U64 * (len(ok) + 8) * scale)
    # the column blocks of a cell add up: exactly on the integer tables; members outside every group are ignored
    half = len(group) // 2
    parts = []
    for lo, hi in ((0, half), (half, len(group))):
        o, f = S.group_index_reference(group[lo:hi], G)
        parts.append(S.cross_spectrum_groups_reference(sums[:, lo:hi], wsum, nrows, o, f))
    assert np.array_equal(S.combine_cross_spectra(parts), got) and np.array_equal(S.combine_cross_spectra([got]), got)
    inside = (group >= 0) & (group < G)
    o, f = S.group_index_reference(group[inside], G)
    assert np.array_equal(S.cross_spectrum_groups_reference(sums[:, inside], wsum, nrows, o, f), got)
    tf = S.transfer_rows_reference(got)
    assert np.all(tf[0, ..., 0] == 0) and np.all(np.isnan(tf[0, ..., 2:]))                   # the cell of one member
    assert np.all((tf[2:, ..., 0] > 0) | np.isnan(tf[2:, ..., 2]))


def test_new_exports_constants_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    decls = ("#define UMPC_XS_TRACK 0", "#define UMPC_XS_ATT 1", "#define UMPC_XS_PUSH 2", "#define UMPC_TF_ROWS 12",
             "int umpcBatchCrossSpectrumInit(umpc_batch_t *h, int K, double *xsums, void *stream);",
             "int umpcBatchCrossSpectrum(umpc_batch_t *h, int pair, const void *state_hist, const void *ref_tab, const void *ref, "
             "const void *imp_tab, const double *basis, long long basis_first, int K, long long first, long long count, "
             "long long ref_first, long long imp_first, int after, double *xsums, void *stream);",
             "int umpcBatchCrossSpectrumGroups(umpc_batch_t *h, const double *xsums, const double *wsum /* host, [1 + 2 K] */, int K, "
             "long long nrows, const int32_t *order, const int32_t *offset, int G, double *gx, void *stream);",
             "int umpcBatchTransfer(umpc_batch_t *h, const double *gx, int G, int K, double *tf, void *stream);")
    for decl in decls:
        assert decl in flat, decl
    assert "cross-spectra and coherence;" not in flat                                      # no longer in a "Not built" list
    assert "cross-spectra and coherence;" not in re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert (_lib.XS_TRACK, _lib.XS_ATT, _lib.XS_PUSH) == (S.XS_TRACK, S.XS_ATT, S.XS_PUSH) == (0, 1, 2)
    assert _lib.TF_ROWS == S.TF_ROWS == len(S.TF_ROW_NAMES) == 12 and S.XS_PAIRS == ("track", "att", "push")
    assert (S.TF_N, S.TF_SKIPPED, S.TF_PXX, S.TF_PYY, S.TF_H_RE, S.TF_H_IM, S.TF_GAIN, S.TF_PHASE, S.TF_COH, S.TF_GAIN_H2,
            S.TF_REL_ERR, S.TF_NOISE) == tuple(range(12))
    scoring = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_scoring.hip")).read()
    assert '#include "umpc_transfer.h"' in scoring
    L = _lib.lib()
    for sym in ("umpcBatchCrossSpectrumInit", "umpcBatchCrossSpectrum", "umpcBatchCrossSpectrumGroups", "umpcBatchTransfer"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchCrossSpectrumInit.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchCrossSpectrum.argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_longlong, C.c_int] + [C.c_longlong] * 4 + \
        [C.c_int, C.c_void_p, C.c_void_p]
    assert L.umpcBatchTransfer.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchCrossSpectrumInit(None, 4, None, None) == -1 and b"umpcBatchCrossSpectrumInit" in L.umpcLastError()
    assert L.umpcBatchCrossSpectrum(None, 0, None, None, None, None, None, 0, 4, 0, 1, 0, 0, 0, None, None) == -1
    assert b"umpcBatchCrossSpectrum:" in L.umpcLastError()
    assert L.umpcBatchCrossSpectrumGroups(None, None, None, 4, 1, None, None, 1, None, None) == -1
    assert b"umpcBatchCrossSpectrumGroups" in L.umpcLastError()
    assert L.umpcBatchTransfer(None, None, 1, 4, None, None) == -1 and b"umpcBatchTransfer" in L.umpcLastError()


def test_transfer_kernels_use_no_scratch():
    """the resource remarks of the build: the sums kernel (2 dtypes x two tables / push against a table / push against a
    constant x tiles of 8 and 4), the groups kernel and the rows kernel spill nothing, and their LDS is what
    csrc/resource_limits.json states: the parking of one slice, (14 + 12 KT) x 64 doubles, and none"""
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    lds = {kt: (_lib.SPEC_SLICES - 1) * (14 + 12 * kt) * 64 * 8 for kt in (8, 4)}
    assert lds == {8: 56320, 4: 31744} and 2 * lds[8] <= 160 * 1024 < 3 * lds[8]             # two blocks per CU at KT = 8
    pats = {"umpc_xspec_kernelIfLi": 6, "umpc_xspec_kernelIdLi": 6, "umpc_xspec_groups_kernel": 1, "umpc_transfer_kernel": 1}
    for pat, n in pats.items():
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            want = 0 if "kernelI" not in pat else lds[8] if re.search(r"Li[012]ELi8E", k) else lds[4]
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == want, (k, res[k])
            if "kernelI" in pat:
                # tiles of 8: the parked sums admit two blocks per CU = one wave per SIMD, the whole unified file of 512; tiles
                # of 4: two waves per SIMD at the least
                assert res[k]["VGPRs"] + res[k]["AGPRs"] <= (512 if want == lds[8] else 256), (k, res[k])
    assert {f: x for f, x in limits["umpc_xspec_kernel"].items() if f != "_note"} == {"ScratchSize": 0}
    for kt in (8, 4):
        pat = "Li%dEEEvNS_6XsArgs" % kt
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds[kt]}
        assert len([k for k in res if pat in k]) == 6 and all("umpc_xspec_kernel" in k for k in res if pat in k)
    for pat in ("umpc_xspec_groups_kernel", "umpc_transfer_kernel"):
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": 0}
    # no older substring pattern counts the new kernels, and no new key is counted among the spectrum's
    new = ("umpc_xspec_kernel", "Li8EEEvNS_6XsArgs", "Li4EEEvNS_6XsArgs", "umpc_xspec_groups_kernel", "umpc_transfer_kernel")
    assert all(k in limits and "spectrum" not in k for k in new)
    for pat in limits:
        if pat not in new:
            assert not [k for k in res if pat in k and ("xspec" in k or "umpc_transfer_kernel" in k)], pat
    for pat in new:
        assert all("xspec" in k or "umpc_transfer_kernel" in k for k in res if pat in k), pat


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
KS = (1, 3, 4, 5, 8, 9, 17, 33)      # across the tile boundaries of both tile sizes (8 and 4)
FORMS = (("track", True), ("att", True), ("push", True), ("push", False))
_CACHE = {}


def _cached_tables(B, dtype, clean=False):
    key = (B, dtype, clean)
    if key not in _CACHE:
        _CACHE[key] = tuple(_noise_tables(B, np.dtype(dtype), clean=clean))
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


def _tile(kt):
    """the tile size of the sums kernel for the calls that follow (read by the library at every call; the sums do not depend on it)"""
    if kt is None:
        os.environ.pop("UMPC_XS_KT", None)
    else:
        os.environ["UMPC_XS_KT"] = str(kt)


def _run(m, pair, dstate, dtab, dconst, dimp, dbasis, K, table, after, first=FIRST, count=COUNT, basis_first=BASIS_FIRST, sums=None):
    """umpcBatchCrossSpectrumInit + umpcBatchCrossSpectrum on device tensors through the C ABI"""
    import torch
    from robobee3d_amd.batch import _ptr
    rows = 2 + 6 * (2 + 2 * K)
    if sums is None:
        sums = torch.full((rows, m.B), 7.0, dtype=torch.float64, device=m.device)
        assert m.L.umpcBatchCrossSpectrumInit(m.h, K, _ptr(sums), m._stream()) == 0
    push = pair == "push"
    rc = m.L.umpcBatchCrossSpectrum(m.h, ("track", "att", "push").index(pair), _ptr(dstate), _ptr(dtab) if table else None,
                                    _ptr(dconst) if not table else None, _ptr(dimp) if push else None, _ptr(dbasis), basis_first, K,
                                    first, count, (REF_FIRST + first - FIRST) if table else 0, IMP_FIRST + first - FIRST, int(after),
                                    _ptr(sums), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return sums


@pytest.fixture
def default_tile():
    yield
    _tile(None)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [200, 197])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_sums_kernel_bit_for_bit(dtype, B, default_tile):
    """every K across the tile boundaries of both tile sizes x both tile sizes forced x the three pairs (push against a table
    and against a constant reference) x after 0 / 1 on one set of noise tables with a NaN / Inf planted in each of the three
    tables: the kernel's sums ARE the mirror's; columns [64, B) on a handle of their own are the same columns of the whole
    batch; run to run; 20 + 17 steps against 37 in one call; count 0, 1, 5; the y blocks of the tracking pair against
    umpcBatchSpectrum(ep) with a zero reference on the device"""
    import torch
    from robobee3d_amd.batch import _ptr
    tables = _cached_tables(B, dtype)
    m = _mpc(B, dtype)
    ds, dr, di = [_dev(m, t) for t in tables]
    dc = _dev(m, tables[1][REF_FIRST])
    mb = _mpc(B - 64, dtype)
    bs, br, bi = [_dev(mb, t[..., 64:]) for t in tables]
    ctab = _cached_tables(B, dtype, clean=True)
    cs, cr = _dev(m, ctab[0]), _dev(m, ctab[1])
    zero_ref = torch.zeros((9, B), dtype=m.dtype, device=m.device)
    for K in KS:
        db = _dev(m, _basis(K)[0])
        chan = 2 + 2 * K
        want = {(pair, table, after): _mirror(pair, tables, table, after, K, np.dtype(dtype)) for pair, table in FORMS for after in (0, 1)}
        for key, w in want.items():
            assert sorted(np.flatnonzero(w[1]).tolist()) == sorted(PLANTED[key[:2]]) and np.all(np.isfinite(w))   # the planted values are read
        chunked = _mirror("push", tables, True, 1, K, np.dtype(dtype), count=20)
        chunked = _mirror("push", tables, True, 1, K, np.dtype(dtype), first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=chunked)
        for kt in (8, 4):
            _tile(kt)
            for (pair, table, after), w in want.items():
                got = _run(m, pair, ds, dr, dc, di, db, K, table, after).cpu().numpy()
                assert np.array_equal(got, w), (K, kt, pair, table, after, np.abs(got - w).max())
            # a column block on a handle of its own; run to run
            one = _run(m, "push", ds, dr, dc, di, db, K, True, 1)
            part = _run(mb, "push", bs, br, None, bi, _dev(mb, _basis(K)[0]), K, True, 1)
            assert torch.equal(part, one[:, 64:]), (K, kt)
            assert torch.equal(one, _run(m, "push", ds, dr, dc, di, db, K, True, 1))
            # chunks: the counts exact, the chunked run bit-equal to the chunked mirror
            two = _run(m, "push", ds, dr, dc, di, db, K, True, 1, count=20)
            two = _run(m, "push", ds, dr, dc, di, db, K, True, 1, first=FIRST + 20, count=17, basis_first=BASIS_FIRST + 20, sums=two)
            assert torch.equal(one[0:2], two[0:2]) and np.array_equal(two.cpu().numpy(), chunked), (K, kt)
            # tables without a hole: the y blocks of the tracking pair are the channel blocks of umpcBatchSpectrum(ep, ref = 0)
            xs = _run(m, "track", cs, cr, None, None, db, K, True, 1)
            sp = torch.full((2 + 3 * chan, B), 7.0, dtype=torch.float64, device=m.device)
            assert m.L.umpcBatchSpectrumInit(m.h, K, _ptr(sp), m._stream()) == 0
            assert m.L.umpcBatchSpectrum(m.h, 0, _ptr(cs), None, None, _ptr(zero_ref), _ptr(db), BASIS_FIRST, K, FIRST, COUNT, 0, 1,
                                         _ptr(sp), m._stream()) == 0, m.L.umpcLastError()
            assert torch.equal(xs[2 + 3 * chan:], sp[2:]) and torch.equal(xs[0:2], sp[0:2]) and torch.all(sp[0] == COUNT), (K, kt)
    # count = 0 changes nothing; 1 step: slice 0's tail alone; 5 steps: one full trip of both slices and a tail
    K = 17
    db = _dev(m, _basis(K)[0])
    zero = torch.zeros((2 + 6 * (2 + 2 * K), B), dtype=torch.float64, device=m.device)
    for kt in (8, 4):
        _tile(kt)
        assert torch.equal(_run(m, "att", ds, dr, dc, di, db, K, True, 0, count=0), zero)
        for count in (1, 5):
            got = _run(m, "push", ds, dr, dc, di, db, K, False, 1, count=count).cpu().numpy()
            assert np.array_equal(got, _mirror("push", tables, False, 1, K, np.dtype(dtype), count=count)), (kt, count)


def _groups(m, dsums, wsum, K, nrows, index, G):
    import torch
    from robobee3d_amd.batch import _ptr
    gx = torch.full((G, 3, 2 + 4 * K), 7.0, dtype=torch.float64, device=m.device)
    wsum = np.ascontiguousarray(wsum, np.float64)
    rc = m.L.umpcBatchCrossSpectrumGroups(m.h, _ptr(dsums), wsum.ctypes.data_as(C.POINTER(C.c_double)), K, nrows, _ptr(index[0]),
                                          _ptr(index[1]), G, _ptr(gx), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return gx


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 8, 9, 64])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_groups_kernel_bit_for_bit(dtype, K):
    """groups of 1, 3, 64, 65 and 130 scattered members, robots in no group and members that do not enter; integer and noise sums"""
    from robobee3d_amd import score as S
    G = len(GROUP_SIZES)
    for exact in (True, False):
        group, sums, wsum, nrows = _group_sums(K, exact=exact)
        m = _mpc(len(group), dtype)
        index = m.group_index(group, G)
        order, offset = index[0].cpu().numpy(), index[1].cpu().numpy()
        want = S.cross_spectrum_groups_reference(sums, wsum, nrows, order, offset)
        got = _groups(m, _dev(m, sums), wsum, K, nrows, index, G).cpu().numpy()
        assert np.array_equal(got, want), (exact, np.abs(got - want).max())
        assert want[:, :, 0].sum() + want[:, :, 1].sum() == 3 * sum(GROUP_SIZES) and want[:, :, 1].sum() > 0
        # another nrows: nobody enters, zeros
        none = _groups(m, _dev(m, sums), wsum, K, nrows + 1, index, G).cpu().numpy()
        assert np.array_equal(none, S.cross_spectrum_groups_reference(sums, wsum, nrows + 1, order, offset)) and np.all(none[:, :, 2:] == 0)


def _rows(m, dgx):
    import torch
    from robobee3d_amd.batch import _ptr
    G, K = int(dgx.shape[0]), (int(dgx.shape[2]) - 2) // 4
    tf = torch.full((G, 3, K, 12), 7.0, dtype=torch.float64, device=m.device)
    assert m.L.umpcBatchTransfer(m.h, _ptr(dgx), G, K, _ptr(tf), m._stream()) == 0, m.L.umpcLastError()
    return tf


def _rows_deviation(got, want):
    """(every row but the phase bit-equal, NaN meeting NaN; the largest phase deviation in rad)"""
    from robobee3d_amd import score as S
    others = [r for r in range(12) if r != S.TF_PHASE]
    exact = np.array_equal(got[..., others], want[..., others], equal_nan=True)
    exact = exact and np.array_equal(np.isnan(got[..., S.TF_PHASE]), np.isnan(want[..., S.TF_PHASE]))
    live = ~np.isnan(want[..., S.TF_PHASE])
    dev = float(np.abs(got[..., S.TF_PHASE][live] - want[..., S.TF_PHASE][live]).max()) if live.any() else 0.0
    return exact, dev


@pytest.mark.gpu
def test_rows_kernel_on_the_mirrors_gx(margin):
    """every row but the phase bit for bit on the mirror's gx, refused rows included; the phase within PHASE_BOUND"""
    import torch
    from robobee3d_amd import score as S
    G = len(GROUP_SIZES)
    m = _mpc(64, "float64")
    worst = 0.0
    for K in (1, 9, 64):
        group, sums, wsum, nrows = _group_sums(K, exact=False)
        order, offset = S.group_index_reference(group, G)
        gx = S.cross_spectrum_groups_reference(sums, wsum, nrows, order, offset)
        gx[1, 0, 2 + 4 * (K - 1)] = 0.0                       # Sxx = 0
        gx[2, 1, 3 + 4 * (K - 1)] = 0.0                       # Syy = 0
        gx[3, 2, 4] = np.inf                                  # a sum that is not finite
        gx[4, 0, 5] = np.nan
        gx[3, 1, 0] = 1.0                                     # n < 2
        want = S.transfer_rows_reference(gx)
        assert np.isnan(want[1, 0, K - 1, 2]) and np.isnan(want[3, 2, 0, 2]) and np.isnan(want[4, 0, 0, 2]) and np.all(np.isnan(want[3, 1, :, 2]))
        assert np.all(np.isnan(want[0, ..., 2])) and np.isnan(want[2, 1, K - 1, 8]) and np.isfinite(want[2, 1, K - 1, 6])
        assert np.isfinite(want[..., 2]).sum() >= 3 * 4 * K - K - 3
        got = _rows(m, _dev(m, gx))
        exact, dev = _rows_deviation(got.cpu().numpy(), want)
        print("K %d: rows kernel against the mirror, largest phase deviation %.3e rad" % (K, dev))
        assert exact, K
        worst = max(worst, dev)
        assert np.array_equal(m.transfer_rows(_dev(m, gx)).cpu().numpy(), got.cpu().numpy(), equal_nan=True)
    margin("phase row (rad)", worst, PHASE_BOUND, "16 x measured %.2e, cap %.2e" % (PHASE_MEASURED, PHASE_CAP))


@pytest.mark.gpu
def test_end_to_end_transfer_of_a_rollout(margin):
    """B = 128 as two cells of 64 draws with different gains, a per-draw random-phase multisine in pdes at 8 on-grid frequencies
    of a 64-step window, one launch: transfer() against the mirrors on the downloaded history. The controller's response is
    printed, not asserted: nobody has measured it."""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, W, dtype = 128, 64, "float32"
    m = _mpc(B, dtype)
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    wts = np.tile(np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])[:, None], (1, B))
    wts[2:4, 64:] *= 4.0                                                                    # the second cell holds its position harder
    m.set_weights(wts.astype(np.float32))
    bins = np.array([1, 2, 3, 5, 8, 13, 21, 27])
    step_s = 1e-3 * int(m.prm.nsub) * float(m.prm.dtsim)
    freq = bins / (W * step_s)
    rng = np.random.default_rng(5)
    phase = rng.uniform(0, 2 * np.pi, (len(bins), 3, B))
    k = np.arange(W)[:, None, None, None]
    tab = np.zeros((W, 9, B))
    tab[:, 0:3] = (2.0 * np.cos(2 * np.pi * bins[None, :, None, None] * k / W + phase[None])).sum(1)
    tab[:, 8] = 1.0
    m.set_reference_trajectory(torch.as_tensor(tab.astype(np.float32)))
    m.record_history(W)
    m.rollout(W)
    hs, ht = m.history()["state"].cpu().numpy(), m._reftab.cpu().numpy()
    index = m.group_index(np.repeat(np.arange(2, dtype=np.int32), 64), 2)
    order, offset = index[0].cpu().numpy(), index[1].cpu().numpy()
    nu = S.response_nu(freq, int(m.prm.nsub), float(m.prm.dtsim))
    basis = S.spectrum_basis(nu, W, "hann")
    tf, gx, sums = m.transfer(freq, index, "track", after=True)
    assert tuple(tf.shape) == (2, 3, 8, 12) and tuple(gx.shape) == (2, 3, 34) and tuple(sums.shape) == (2 + 6 * 18, B)
    assert tf.dtype == gx.dtype == sums.dtype == torch.float64
    wsums = S.cross_spectrum_sums_reference("track", hs, ht, None, basis, 0, 0, W, 0, 0, True, np.float32)
    assert np.all(wsums[0] == W) and np.array_equal(sums.cpu().numpy(), wsums)
    wgx = S.cross_spectrum_groups_reference(wsums, S.spectrum_wsum(basis), W, order, offset)
    assert np.array_equal(gx.cpu().numpy(), wgx)
    got = tf.cpu().numpy()
    exact, dev = _rows_deviation(got, S.transfer_rows_reference(wgx))
    assert exact
    margin("end to end phase row (rad)", dev, PHASE_BOUND)
    assert np.all(got[..., S.TF_N] == 64) and np.all(got[..., S.TF_SKIPPED] == 0) and np.all(np.isfinite(got))
    assert np.all(got[..., S.TF_COH] >= 0) and np.all(got[..., S.TF_COH] <= 1 + 1e-12)
    assert np.all(got[..., S.TF_GAIN] <= got[..., S.TF_GAIN_H2])
    for g in range(2):
        for c in range(3):
            for j in range(len(bins)):
                r = got[g, c, j]
                print("cell %d channel %d %7.2f Hz: gain %.4f phase %+.4f rad coh %.4f rel_err %.4f" % (g, c, freq[j], r[S.TF_GAIN], r[S.TF_PHASE],
                                                                                                 r[S.TF_COH], r[S.TF_REL_ERR]))
    # the attitude pair and the push pair (no pushes were made: a table of noise stands in) through the same method
    tfa, gxa, sa = m.transfer(freq, index, "att", after=True)
    assert np.array_equal(sa.cpu().numpy(), S.cross_spectrum_sums_reference("att", hs, ht, None, basis, 0, 0, W, 0, 0, True, np.float32))
    # sdes = e3 is constant: channels 0 and 1 have no input power at all and are refused; channel 2 keeps the rounding dust
    # of the mean removal, which Pxx reveals
    assert torch.all(tfa[:, 0:2, :, 0] == 0) and torch.all(torch.isnan(tfa[:, 0:2, :, 2:])) and not torch.any(tfa[:, 2, :, S.TF_PXX] > 1e-28)
    imp = torch.as_tensor(rng.normal(size=(W + 2, 6, B)).astype(np.float32)).to(m.device)
    tfp, gxp, sp = m.transfer(freq, index, "push", after=True, impulses=imp, imp_first=2)
    wp = S.cross_spectrum_sums_reference("push", hs, ht, imp.cpu().numpy(), basis, 0, 0, W, 0, 2, True, np.float32)
    assert np.array_equal(sp.cpu().numpy(), wp) and torch.all(tfp[..., 0] == 64)
    # chunks: steps 0..19, then 20..63 on the basis of the whole window; the rows of a table combined over column blocks
    db = torch.as_tensor(basis).to(m.device)
    none, nogx, part = m.transfer(freq, index, "track", first=0, count=20, after=True, basis=db, rows=False)
    assert none is None and nogx is None
    tf2, gx2, part = m.transfer(freq, index, "track", first=20, count=44, after=True, basis=db, basis_first=20, sums=part)
    assert torch.equal(part[0:2], sums[0:2]) and torch.all(tf2[..., 0] == 64)
    assert torch.allclose(tf2[..., S.TF_GAIN], tf[..., S.TF_GAIN], rtol=1e-9, atol=0)
    halves = []
    for lo in (0, 32):
        grp = np.full(B, -1, np.int32)
        grp[lo:lo + 32], grp[64 + lo:96 + lo] = 0, 1
        halves.append(m.transfer(freq, m.group_index(grp, 2), "track", after=True)[1])
    both = m.transfer_rows(S.combine_cross_spectra(halves))
    assert torch.all(both[..., 0] == 64) and torch.allclose(both[..., S.TF_GAIN], tf[..., S.TF_GAIN], rtol=1e-12, atol=0)
    # the impulse cursor at the start of the record is remembered beside the reference's
    assert m._hist_imp0 == 0 and m._hist_ref0 == 0
    for bad in (dict(freq_hz=[0.0]), dict(freq_hz=np.arange(65) + 1.0), dict(count=W + 1), dict(pair="ep"),
                dict(sums=torch.zeros((44, B), device=m.device)), dict(basis=db, basis_first=1), dict(basis_first=3), dict(window="blackman"),
                dict(pair="push", impulses=imp, imp_first=3), dict(pair="push", impulses=imp[:, :3])):
        kw = dict(freq_hz=freq, index=index, pair="track")
        kw.update(bad)
        with pytest.raises(ValueError):
            m.transfer(**kw)
    with pytest.raises(RuntimeError):
        m.transfer(freq, index, "push")                                                     # no impulse table is set
    with pytest.raises(ValueError):
        m.transfer_rows(gx[:, :2])


@pytest.mark.gpu
def test_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    K = 4
    state = torch.zeros((5, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((4, 9, 64), device=m.device)
    imp = torch.zeros((4, 6, 64), device=m.device)
    basis = torch.ones((4, 1 + 2 * K), dtype=torch.float64, device=m.device)
    sums = torch.full((2 + 6 * (2 + 2 * K), 64), 3.0, dtype=torch.float64, device=m.device)
    keep = sums.clone()
    ok = dict(pair=0, state=P(state), tab=P(tab), ref=None, imp=None, basis=P(basis), basis_first=0, K=K, first=0, count=4, ref_first=0,
              imp_first=0, sums=P(sums))
    call = lambda a: L.umpcBatchCrossSpectrum(h, a["pair"], a["state"], a["tab"], a["ref"], a["imp"], a["basis"], a["basis_first"], a["K"],
                                              a["first"], a["count"], a["ref_first"], a["imp_first"], 0, a["sums"], s)
    push = dict(ok, pair=2, imp=P(imp))
    for bad in (dict(count=-1), dict(count=(1 << 31) - 4), dict(first=-1), dict(ref_first=-1), dict(imp_first=-1), dict(basis_first=-1),
                dict(K=0), dict(K=65), dict(pair=3), dict(pair=-1), dict(basis=None), dict(sums=None), dict(state=None),
                dict(tab=None), dict(tab=None, ref=P(ref)), dict(ref=P(ref)), dict(pair=1, tab=None, ref=P(ref)), dict(pair=1, ref=P(ref)),
                dict(push, imp=None), dict(push, ref=P(ref)), dict(push, tab=None)):
        assert call(dict(ok, **bad)) == -1 and b"umpcBatchCrossSpectrum:" in L.umpcLastError(), bad
    assert L.umpcBatchCrossSpectrumInit(h, K, None, s) == -1 and L.umpcBatchCrossSpectrumInit(h, 0, P(sums), s) == -1
    assert L.umpcBatchCrossSpectrumInit(h, 65, P(sums), s) == -1 and b"umpcBatchCrossSpectrumInit" in L.umpcLastError()
    index = m.group_index(np.zeros(64, np.int32), 1)
    gx = torch.full((1, 3, 2 + 4 * K), 5.0, dtype=torch.float64, device=m.device)
    tf = torch.full((1, 3, K, 12), 5.0, dtype=torch.float64, device=m.device)
    wsum = (C.c_double * (1 + 2 * K))(*([4.0] + [0.0] * (2 * K)))
    gr = lambda su=P(sums), ws=wsum, k=K, nrows=4, o=P(index[0]), f=P(index[1]), G=1, g=P(gx): L.umpcBatchCrossSpectrumGroups(h, su, ws, k, nrows, o, f, G, g, s)
    for bad in (dict(su=None), dict(ws=None), dict(o=None), dict(f=None), dict(g=None), dict(G=0), dict(k=0), dict(k=65), dict(nrows=-1),
                dict(nrows=(1 << 53) + 1)):
        assert gr(**bad) == -1 and b"umpcBatchCrossSpectrumGroups" in L.umpcLastError(), bad
    ro = lambda g=P(gx), G=1, k=K, t=P(tf): L.umpcBatchTransfer(h, g, G, k, t, s)
    for bad in (dict(g=None), dict(t=None), dict(G=0), dict(k=0), dict(k=65)):
        assert ro(**bad) == -1 and b"umpcBatchTransfer" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert torch.equal(sums, keep) and torch.all(gx == 5.0) and torch.all(tf == 5.0)          # nothing was launched
    # the same calls with good arguments go through: count = 0 changes nothing, a call adds into the sums; the push pair
    # takes a table or a constant reference
    assert call(dict(ok, count=0)) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums, keep)
    assert call(ok) == 0 and call(push) == 0 and call(dict(push, tab=None, ref=P(ref))) == 0 and call(dict(ok, pair=1)) == 0
    torch.cuda.synchronize()
    assert torch.all(sums[0] == 19.0) and torch.all(sums[1] == 3.0) and torch.all(sums[2] == 3.0)
    assert gr() == 0 and ro() == 0
    torch.cuda.synchronize()
    assert torch.all(gx[:, :, 0] == 0) and torch.all(gx[:, :, 1] == 64) and torch.all(gx[:, :, 2:] == 0)
    assert torch.all(tf[..., 0] == 0) and torch.all(tf[..., 1] == 64) and torch.all(torch.isnan(tf[..., 2:]))
