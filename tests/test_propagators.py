"""Error propagators on the device: umpcBatchLagMoments turns a step history and its reference into the raw cross moments [96]
of the error state z = (p - pdes, v - dpdes) between step k and step k + L per (step, group); umpcBatchPropagators turns them
into the affine map z_b ~ Phi z_a + c, the unexplained covariance Q, r2 and growth [80].
CPU: the numpy mirrors (robobee3d_amd/score.py) by hand on a tiny table, against two-pass numpy, against numpy.linalg.lstsq,
exact recovery of a planted linear recursion and its poles, the status rows, the combination over column blocks, exports,
refusals, the resource record.
GPU: the kernels against the mirrors on the same arrays -- both dtypes, contiguous and scattered groups, after 0 / 1, table /
constant reference, lags 1 and 3 --, independence of a row from everything but its member list and the lag, agreement with the
dispersion kernel bit for bit, exact recovery, one end-to-end sweep, refusals."""
import json
import os
import re

import numpy as np
import pytest

from test_dispersion import B_, G_, SIZES, U64, _disp, _groups, _index
from test_score import U, _dev, _mpc, _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, COUNT, REF_FIRST = 1, 11, 2
LAGS, LMAX = (1, 3), 3
NAN_AT, INF_AT = (5, 1, 140), (6, 13, 10)        # (state slice, row, robot): a p word and a v word of different members
# the planted recursion z_{k+1} = A z_k + C0 in the order (p, v): three position-velocity pairs with the poles 0.875 +- 0.125i,
# 0.875 +- 0.25i and 0.8125 +- 0.108i (moduli 0.884, 0.910, 0.820: spectral radius 0.910), coupled upwards so that the
# characteristic polynomial stays the product of the pairs'; every entry a multiple of 1/8
A = np.array([[1.0, 0.125, 0.0, 0.125, 0.0, 0.0],
              [0.0, 0.875, 0.125, 0.0, 0.25, 0.0],
              [0.0, 0.0, 0.875, 0.0, 0.0, 0.125],
              [-0.25, 0.0, 0.125, 0.75, 0.125, 0.0],
              [0.0, -0.25, 0.0, 0.0, 0.875, 0.125],
              [0.0, 0.0, -0.125, 0.0, 0.0, 0.75]])
C0 = np.array([0.03, -0.02, 0.01, 0.0, 0.02, -0.01])


def _xtables(dtype, kind, seed=20240611, planted=True):
    """state [15, 18, 320] and reference [16, 9, 320] in `dtype`, built as test_dispersion._tables builds them but LMAX slices
    longer. "noise": an anisotropic, correlated cloud around the reference. "dyadic": multiples of 2^-6 of magnitude <= 1/4 so
    that every difference, product and sum is exact in both dtypes, and at state slices 1 and 2 every robot sits at the same
    offset from its reference: cells on one point. planted: one NaN in a p word and one Inf in a v word of different members;
    rows that no kernel reads hold NaN."""
    rng = np.random.default_rng(seed)
    ns = FIRST + COUNT + 1 + LMAX
    state = np.full((ns, 18, B_), np.nan)
    ref = np.full((REF_FIRST + COUNT + 1 + LMAX, 9, B_), np.nan)
    if kind == "noise":
        ref[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, B_)) + 0.7 * rng.normal(size=(len(ref), 3, B_))
        ref[:, 3:6] = rng.normal(size=(len(ref), 3, B_))
        mix = np.array([[1.5, 0.0, 0.0], [0.4, 0.7, 0.0], [-0.2, 0.1, 0.3]])
        near = slice(REF_FIRST - FIRST, REF_FIRST - FIRST + ns)
        state[:, 0:3] = ref[near, 0:3] + np.einsum("ij,sjb->sib", mix, rng.normal(size=(ns, 3, B_)))
        state[:, 12:15] = ref[near, 3:6] + 0.5 * rng.normal(size=(ns, 3, B_)) + 0.3 * (state[:, 0:3] - ref[near, 0:3])
    else:
        ref[:, 0:6] = rng.integers(-16, 17, size=(len(ref), 6, B_)) / 64.0
        state[:, 0:3] = rng.integers(-16, 17, size=(ns, 3, B_)) / 64.0
        state[:, 12:15] = rng.integers(-16, 17, size=(ns, 3, B_)) / 64.0
        for s in (1, 2):                      # slice a of the first row, after = 0 and 1, table and constant reference
            state[s, 0:3] = ref[REF_FIRST, 0:3] + np.array([0.25, -0.125, 0.5])[:, None]
            state[s, 12:15] = ref[REF_FIRST, 3:6] + np.array([0.0, 0.125, -0.25])[:, None]
    if planted:
        state[NAN_AT] = np.nan
        state[INF_AT] = np.inf
    return state.astype(dtype), ref.astype(dtype)


def _recursion_tables(seed=7):
    """fp64 tables with a zero reference table and z_{k+1} = A z_k + C0 from a unit Gaussian cloud at slice 0"""
    rng = np.random.default_rng(seed)
    ns = FIRST + COUNT + 1 + LMAX
    z = np.zeros((ns, 6, B_))
    z[0] = rng.normal(size=(6, B_))
    for k in range(1, ns):
        z[k] = A @ z[k - 1] + C0[:, None]
    state = np.full((ns, 18, B_), np.nan)
    state[:, 0:3], state[:, 12:15] = z[:, 0:3], z[:, 3:6]
    ref = np.zeros((REF_FIRST + COUNT + 1 + LMAX, 9, B_))
    return state, ref


def _pairs(state, ref, table, after, lag, dtype, first=FIRST, count=COUNT, ref_first=REF_FIRST):
    """(ok [count, B], za, zb [count, 6, B] float64) of the window: the differences formed in `dtype`, zero where not scored"""
    def z(st, rf):
        a, b = np.concatenate([st[:, 0:3], st[:, 12:15]], 1), rf[:, 0:6]
        with np.errstate(invalid="ignore", over="ignore"):
            d = (a - b).astype(np.float64)
        return np.isfinite(a).all(1) & np.isfinite(b).all(1), d
    st, rf = np.asarray(state, dtype), np.asarray(ref, dtype)
    sa, sb = st[first + after:first + after + count], st[first + after + lag:first + after + lag + count]
    if table:
        ra, rb = rf[ref_first:ref_first + count], rf[ref_first + lag:ref_first + lag + count]
    else:
        ra = rb = np.repeat(rf[None], count, 0)
    oka, za = z(sa, ra)
    okb, zb = z(sb, rb)
    ok = oka & okb
    return ok, np.where(ok[:, None], za, 0.0), np.where(ok[:, None], zb, 0.0)


def _terms(za, zb):
    """[count, 90, B]: the terms of rows 2..91"""
    from robobee3d_amd import score as S
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([za, zb, np.stack([za[:, a] * za[:, b] for a, b in S.DISP_PAIRS], 1),
                               np.stack([zb[:, a] * zb[:, b] for a, b in S.DISP_PAIRS], 1),
                               np.stack([zb[:, a] * za[:, b] for a in range(6) for b in range(6)], 1)], 1)


def _sum_abs(za, zb, order, offset):
    """[count, G, 90]: sum |term| of every entry over the group's members (the scale of its rounding error)"""
    t = np.abs(_terms(za, zb))
    res = np.zeros((t.shape[0], len(offset) - 1, 90))
    for g in range(len(offset) - 1):
        res[:, g] = t[:, :, order[offset[g]:offset[g + 1]]].sum(2)
    return res


def _check_xmom(got, want, sabs, margin, tag, parts=1):
    """counts exact, rows 92..95 zero, |got - want| <= (n + 9) 2^-53 sum |term| per entry (n the members of the group; one more
    rounding per part beyond the first and both sides' bounds when `want` is a sum of parts); an entry without a nonzero term is
    exactly 0. Returns whether the bits agree."""
    got = got.to("cpu").numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (tag, got.dtype, got.shape)
    assert np.array_equal(got[..., 0:2], want[..., 0:2]) and np.all(got[..., 92:96] == 0), tag
    n = want[..., 0:1] + want[..., 1:2]
    bound = (n + 9) * U64 * sabs if parts == 1 else 2 * (n + 9 + parts) * U64 * sabs
    err = np.abs(got[..., 2:92] - want[..., 2:92])
    assert np.all(err[bound == 0] == 0), tag
    margin("%s |xmom - mirror| / bound" % tag, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)), 1.0)
    return bool(np.array_equal(got, want))


def _full(tri):
    """[.., 6, 6] symmetric from an upper triangle [.., 21] in DISP_PAIRS order"""
    from robobee3d_amd import score as S
    m = np.zeros(tri.shape[:-1] + (6, 6))
    for k, (i, j) in enumerate(S.DISP_PAIRS):
        m[..., i, j] = m[..., j, i] = tri[..., k]
    return m


def _covs(x):
    """(n, m_a, m_b, C_a, C_b, C_ba, raw) of lag-moment rows [.., 96] in plain numpy; raw = max_i S2a_ii / ((n - 1) C_a,ii)"""
    from robobee3d_amd import score as S
    with np.errstate(invalid="ignore", divide="ignore"):
        n = x[..., S.X_N]
        nn, n1 = n[..., None, None], (n - 1.0)[..., None, None]
        s1a, s1b = x[..., S.X_S1A:S.X_S1A + 6], x[..., S.X_S1B:S.X_S1B + 6]
        s2a, s2b = _full(x[..., S.X_S2A:S.X_S2A + 21]), _full(x[..., S.X_S2B:S.X_S2B + 21])
        sba = x[..., S.X_SBA:S.X_SBA + 36].reshape(x.shape[:-1] + (6, 6))
        ca = (s2a - s1a[..., :, None] * s1a[..., None, :] / nn) / n1
        cb = (s2b - s1b[..., :, None] * s1b[..., None, :] / nn) / n1
        cba = (sba - s1b[..., :, None] * s1a[..., None, :] / nn) / n1
        d = np.arange(6)
        raw = np.max(s2a[..., d, d] / (n1[..., 0] * ca[..., d, d]), -1)
        ma, mb = s1a / n[..., None], s1b / n[..., None]
    return n, ma, mb, ca, cb, cba, raw


def _bound3(x):
    """the bound of the issue's test 3 without its last factor, per usable row [..]: 16 cond2(C_a) 2^-53 raw; and cond2(C_a)"""
    from robobee3d_amd import score as S
    n, _, _, ca, _, _, raw = _covs(x)
    cond = np.full(n.shape, np.nan)
    use = S.propagator_reference(x)[..., S.P_STATUS] == S.PROP_OK
    cond[use] = np.linalg.cond(ca[use])
    return 16.0 * cond * U64 * raw, cond


def _phi(p):
    from robobee3d_amd import score as S
    return p[..., S.P_PHI:S.P_C].reshape(p.shape[:-1] + (6, 6))


NAN_ROWS = [3, 4, 5] + list(range(8, 71))


def _check_pattern(p, tag):
    """what every propagator table obeys: rows 6, 7, 71..79 zero; status != 0 <=> exactly rows 3..5 and 8..70 NaN (an r2 may be
    NaN on a usable row whose denominator is 0; nothing else)"""
    from robobee3d_amd import score as S
    assert np.all(p[..., 6:8] == 0) and np.all(p[..., 71:80] == 0), tag
    un = p[..., S.P_STATUS] != S.PROP_OK
    assert np.isnan(p[un][:, NAN_ROWS]).all() and not np.isnan(p[un][:, [0, 1, 2, 6, 7] + list(range(71, 80))]).any(), tag
    ok = p[~un]
    assert not np.isnan(ok[:, [5] + list(range(8, 71))]).any(), tag
    assert np.all((p[..., S.P_STATUS] == S.PROP_FEW) == (p[..., S.P_N] < 8)), tag


def _check_props(got, want, x, margin, tag):
    """the propagator kernel (or any other route) against the mirror on the same moments: status, counts and NaN pattern exact;
    Phi, c, r2 and growth within bound3 x max(1, max |Phi|), Q within that x max |C_b|. Returns whether the bits agree."""
    from robobee3d_amd import score as S
    assert got.shape == want.shape and np.array_equal(got[..., 0:3], want[..., 0:3]), tag
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    _check_pattern(got, tag)
    b3, _ = _bound3(x)
    use = want[..., S.P_STATUS] == S.PROP_OK
    cb = _covs(x)[4][use]
    g, w = got[use], want[use]
    bnd = b3[use] * np.maximum(1.0, np.abs(_phi(w)).max((-1, -2)))
    worst = lambda rows: float(np.max(np.nan_to_num(np.abs(g[:, rows] - w[:, rows]), nan=0.0) / bnd[:, None], initial=0.0))
    margin("%s Phi, c / bound" % tag, worst(list(range(8, 50))), 1.0)
    margin("%s r2, growth / bound" % tag, worst([3, 4, 5]), 1.0)
    qb = bnd * np.abs(cb).max((-1, -2))
    margin("%s Q / bound" % tag, float(np.max(np.abs(g[:, 50:71] - w[:, 50:71]) / qb[:, None], initial=0.0)), 1.0)
    return bool(np.array_equal(got.view(np.int64), want.view(np.int64)))


def _match(got, want):
    """the largest distance after pairing two multisets of complex numbers greedily, nearest first"""
    got, worst = list(got), 0.0
    for w in want:
        j = int(np.argmin([abs(g - w) for g in got]))
        worst = max(worst, abs(got.pop(j) - w))
    return worst


def _check_recovery(prop, x, lag, margin, tag):
    """the assertions of the issue's test 4 on a propagator table of the planted recursion at `lag`: for every row with
    n >= 8, Phi = A^lag and the c row = (A^(lag-1) + .. + I) C0 within bound3 x max(1, max |Phi|), Q within that x max |C_b| of
    zero, r2 >= 1 - 1e-9, cond2(C_a) < 1e6; the poles"""
    from robobee3d_amd import score as S
    Al = np.linalg.matrix_power(A, lag)
    cl = sum(np.linalg.matrix_power(A, j) for j in range(lag)) @ C0
    b3, cond = _bound3(x)
    big = x[..., S.X_N] >= 8
    assert big.sum() == COUNT * 4 and np.all(prop[..., S.P_STATUS][big] == S.PROP_OK) and np.all(prop[..., S.P_STATUS][~big] == S.PROP_FEW), tag
    assert np.all(cond[big] < 1e6), (tag, cond[big].max())
    p, bnd = prop[big], b3[big]
    bnd = bnd * np.maximum(1.0, np.abs(_phi(p)).max((-1, -2)))
    margin("%s |Phi - A^%d| / bound" % (tag, lag), float(np.max(np.abs(_phi(p) - Al).max((-1, -2)) / bnd)), 1.0)
    margin("%s |c - c_%d| / bound" % (tag, lag), float(np.max(np.abs(p[:, S.P_C:S.P_Q] - cl).max(-1) / bnd)), 1.0)
    cbmax = np.abs(_covs(x)[4][big]).max((-1, -2))
    margin("%s |Q| / (bound max |C_b|)" % (tag,), float(np.max(np.abs(p[:, S.P_Q:S.P_END]).max(-1) / (bnd * cbmax))), 1.0)
    assert np.all(p[:, S.P_R2_P] >= 1 - 1e-9) and np.all(p[:, S.P_R2_V] >= 1 - 1e-9), tag
    # eigenvalues of Phi against those of A^lag (before the root), and after the principal root those of A again: the poles of A
    # turn less than a quarter revolution per step
    raw = S.propagator_poles(prop, 1)
    root = S.propagator_poles(prop, lag)
    assert np.isnan(raw[~big]).all() and np.isnan(root[~big]).all() and raw.shape == prop.shape[:2] + (6,)
    want = np.linalg.eigvals(Al)
    margin("%s eigenvalues of Phi against eigvals(A^%d)" % (tag, lag), max(_match(r, want) for r in raw[big]), 1e-8)
    margin("%s poles against eigvals(A)" % tag, max(_match(r, np.linalg.eigvals(A)) for r in root[big]), 1e-8)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_mirror_semantics_by_hand():
    """a cell of three members and two rows at lag 1 (three slices): p = (x, y, 0), v = (w, 0, 0) against a reference at the
    origin, so z = (x, y, 0, w, 0, 0). Robot 3 is a cell of its own, robot 4 is ignored."""
    from robobee3d_amd import score as S
    assert (S.XMOM_ROWS, S.PROP_ROWS, S.PROP_PIVOT_TOL) == (96, 80, 1e-10)
    assert (S.X_N, S.X_SKIPPED, S.X_S1A, S.X_S1B, S.X_S2A, S.X_S2B, S.X_SBA) == (0, 1, 2, 8, 14, 35, 56)
    assert (S.P_N, S.P_SKIPPED, S.P_STATUS, S.P_R2_P, S.P_R2_V, S.P_GROWTH, S.P_PHI, S.P_C, S.P_Q) == (0, 1, 2, 3, 4, 5, 8, 44, 50)
    nan, inf = np.nan, np.inf
    x = np.array([[2.0, -2.0, 3.0, 3.0, 100.0], [3.0, 1.0, 1.0, nan, 100.0], [1.0, nan, 2.0, 1.0, nan]])
    y = np.array([[0.0, 1.0, 2.0, 0.0, 0.0], [2.0, 0.0, 1.0, 0.0, 0.0], [0.5, 0.5, 4.0, 0.0, 0.0]])
    w = np.array([[1.0, 1.0, -2.0, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0, 0.0], [0.25, 0.25, inf, 0.0, 0.0]])
    state = np.zeros((3, 18, 5))
    state[:, 0], state[:, 1], state[:, 12] = x, y, w
    state[:, 3:12] = nan                                 # the attitude is not read
    ref = np.zeros((9, 5))
    ref[6:9] = nan                                       # sdes is not read
    order, offset = S.group_index_reference(np.array([0, 0, 0, 2, -1], np.int32), 3)
    xm = S.lag_moments_reference(state, ref, 0, 2, 0, False, 1, order, offset)
    assert xm.shape == (2, 3, 96)

    def row(n, skipped, members):
        """the 96 rows from a list of (z_a, z_b) of the scored members, summed by hand in plain Python"""
        r = [0.0] * 96
        r[0], r[1] = float(n), float(skipped)
        for za, zb in members:
            for j in range(6):
                r[2 + j] += za[j]
                r[8 + j] += zb[j]
            for k, (i, j) in enumerate(S.DISP_PAIRS):
                r[14 + k] += za[i] * za[j]
                r[35 + k] += zb[i] * zb[j]
            for i in range(6):
                for j in range(6):
                    r[56 + 6 * i + j] += zb[i] * za[j]
        return r
    zz = lambda s, b: [x[s, b], y[s, b], 0.0, w[s, b], 0.0, 0.0]
    # row 0 (slices 0 and 1): all three of group 0 scored; group 2's member is not finite at b: skipped
    assert xm[0, 0].tolist() == row(3, 0, [(zz(0, b), zz(1, b)) for b in (0, 1, 2)])
    assert xm[0, 2].tolist() == row(0, 1, [])
    # row 1 (slices 1 and 2): robot 1 has a NaN and robot 2 an Inf at b: one member left; group 2's member is not finite at a
    assert xm[1, 0].tolist() == row(1, 2, [(zz(1, 0), zz(2, 0))])
    assert xm[1, 2].tolist() == row(0, 1, [])
    assert np.all(xm[:, 1] == 0) and np.all(xm[..., 92:] == 0)          # the empty group; rows 92..95
    # spot values, written out: Sba[0][0] = 3*2 + 1*(-2) + 1*3 = 7, Sba[3][0] = 0*2 + .5*(-2) + 0*3 = -1, S1b = (5, 3, 0, .5, 0, 0)
    assert xm[0, 0, 56] == 7 and xm[0, 0, 56 + 18] == -1 and xm[0, 0, 8:14].tolist() == [5, 3, 0, 0.5, 0, 0]
    assert xm[0, 0, 2:8].tolist() == [3, 3, 0, 0, 0, 0] and xm[0, 0, 14] == 17 and xm[0, 0, 35] == 11
    # lag 2 pairs slices 0 and 2; fp32 handles give the same numbers on dyadic tables; a table; after = 1
    x2 = S.lag_moments_reference(state, ref, 0, 1, 0, False, 2, order, offset)
    assert x2[0, 0].tolist() == row(1, 2, [(zz(0, 0), zz(2, 0))]) and x2[0, 2].tolist() == row(1, 0, [(zz(0, 3), zz(2, 3))])
    assert np.array_equal(S.lag_moments_reference(state, ref, 0, 2, 0, False, 1, order, offset, dtype=np.float32), xm)
    tab = np.repeat(ref[None], 6, 0)
    assert np.array_equal(S.lag_moments_reference(state, tab, 0, 1, 3, True, 1, order, offset), xm[1:2])
    assert S.lag_moments_reference(state, ref, 1, 0, 0, False, 1, order, offset).shape == (0, 3, 96)
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(lag=0), dict(lag=-1), dict(lag=(1 << 20) + 1)):
        kw = dict(first=0, count=2, ref_first=0, after=False, lag=1, order=order, offset=offset)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.lag_moments_reference(state, ref, **kw)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lag", LAGS)
def test_mirror_against_two_pass_numpy(dtype, lag, margin):
    """The raw moments of the mirror (one pass, the device's order) against the two-pass route on the same z: centre first, then
    np.cov-style products of the centred members, and the raw moment put back together as sum (dz dz^T) + n m m^T (S1 as n m).
    Bound per entry: (n + 9) 2^-53 sum |term|, that of test_dispersion._check_moments for an fp64 handle. The two-pass value
    carries a handful of roundings of its own at the scale |n m_i m_j| + sum |dz_i dz_j| <= 2 sqrt(T_ii T_jj), which for these
    clouds (every axis of comparable spread, offsets below a sigma) is of the order of T_ij: far inside (n + 9) of them."""
    from robobee3d_amd import score as S
    state, ref = _xtables(np.dtype(dtype), "noise")
    order, offset = S.group_index_reference(_groups("contiguous"), G_)
    xm = S.lag_moments_reference(state, ref, FIRST, COUNT, REF_FIRST, True, lag, order, offset, dtype=np.dtype(dtype))
    ok, za, zb = _pairs(state, ref, True, 1, lag, np.dtype(dtype))
    two = np.zeros_like(xm)
    for i in range(COUNT):
        for g in range(G_):
            mem = order[offset[g]:offset[g + 1]]
            mem = mem[ok[i, mem]]
            n = len(mem)
            two[i, g, 0], two[i, g, 1] = n, offset[g + 1] - offset[g] - n
            if n == 0:
                continue
            a, b = za[i][:, mem], zb[i][:, mem]
            ma, mb = a.mean(1), b.mean(1)
            da, db = a - ma[:, None], b - mb[:, None]
            saa, sbb, sba = da @ da.T + n * np.outer(ma, ma), db @ db.T + n * np.outer(mb, mb), db @ da.T + n * np.outer(mb, ma)
            two[i, g, 2:8], two[i, g, 8:14] = n * ma, n * mb
            two[i, g, 14:35] = [saa[p] for p in S.DISP_PAIRS]
            two[i, g, 35:56] = [sbb[p] for p in S.DISP_PAIRS]
            two[i, g, 56:92] = sba.reshape(-1)
    assert two[..., 1].sum() > 0
    _check_xmom(xm, two, _sum_abs(za, zb, order, offset), margin, "%s lag %d" % (dtype, lag))


def _lstsq_case(state, ref, ids, G, lag, dtype):
    from robobee3d_amd import score as S
    order, offset = S.group_index_reference(ids, G)
    x = S.lag_moments_reference(state, ref, FIRST, COUNT, REF_FIRST, False, lag, order, offset, dtype=dtype)
    ok, za, zb = _pairs(state, ref, True, 0, lag, dtype)
    return order, offset, x, ok, za, zb


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_propagator_mirror_against_lapack(dtype, margin):
    """Phi and c of propagator_reference (normal equations from raw moments) against numpy.linalg.lstsq on the centred members,
    Q against the residual covariance of that fit: cells of n = 8, 9, 64, 65, 100 of the noise cloud shifted by a mean of 3
    sigma per axis, 11 steps, lags 1 and 3. Bound: 16 cond2(C_a) 2^-53 raw max(1, max |Phi|), raw = max_i S2a_ii / ((n - 1)
    C_a,ii) the magnification raw moments bring; Q at the same bound times max |C_b| (the issue's test 3)."""
    from robobee3d_amd import score as S
    dt = np.dtype(dtype)
    state, ref = _xtables(np.float64, "noise", planted=False)
    # after = 0 pairs state slice s with reference slice s + 1, the one the cloud was drawn around: z is the cloud itself
    sig = _pairs(state, ref, True, 0, 1, np.float64)[1].std((0, 2))
    state[:, 0:3] += 3.0 * sig[0:3, None]
    state[:, 12:15] += 3.0 * sig[3:6, None]
    state, ref = state.astype(dt), ref.astype(dt)
    sizes = (8, 9, 64, 65, 100)
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(sizes)] + [np.full(B_ - sum(sizes), -1, np.int32)])
    worst = np.zeros(3)
    seen = 0
    for lag in LAGS:
        order, offset, x, ok, za, zb = _lstsq_case(state, ref, ids, len(sizes), lag, dt)
        prop = S.propagator_reference(x)
        _check_pattern(prop, dtype)
        assert np.all(prop[..., S.P_STATUS] == S.PROP_OK) and np.all(x[..., 0] == sizes)
        b3, cond = _bound3(x)
        cbm = np.abs(_covs(x)[4]).max((-1, -2))
        for i in range(COUNT):
            for g, n in enumerate(sizes):
                mem = order[offset[g]:offset[g + 1]]
                a, b = za[i][:, mem].T, zb[i][:, mem].T                      # [n, 6]
                ma, mb = a.mean(0), b.mean(0)
                assert np.abs(ma / a.std(0, ddof=1)).min() > 1.5              # (input check: the planted offset is there)
                sol = np.linalg.lstsq(a - ma, b - mb, rcond=None)[0]          # [6, 6] = Phi^T
                res = (b - mb) - (a - ma) @ sol
                phi, c, q = sol.T, mb - sol.T @ ma, res.T @ res / (n - 1)
                p = prop[i, g]
                bnd = b3[i, g] * max(1.0, np.abs(phi).max())
                worst = np.maximum(worst, [np.abs(_phi(p) - phi).max() / bnd, np.abs(p[S.P_C:S.P_Q] - c).max() / bnd,
                                           np.abs(_full(p[S.P_Q:S.P_END]) - q).max() / (bnd * cbm[i, g])])
                seen += 1
        r2 = prop[..., S.P_R2_P:S.P_R2_V + 1]
        assert np.all(r2 >= 0) and np.all(r2 <= 1 + 1e-12) and np.all(prop[..., S.P_GROWTH] >= 0)
    assert seen == 2 * COUNT * len(sizes)
    for k, name in enumerate(("Phi", "c", "Q")):
        margin("%s |%s - lstsq| / bound" % (dtype, name), float(worst[k]), 1.0)


@pytest.mark.parametrize("lag", (1, 2))
def test_exact_recovery_of_a_planted_recursion(lag, margin):
    from robobee3d_amd import score as S
    lam = np.linalg.eigvals(A)
    assert 0.8 <= np.abs(lam).max() <= 1.0 and np.all(A * 8 == np.round(A * 8)) and np.abs(A[0:3, 3:6]).max() > 0 and np.abs(A[3:6, 0:3]).max() > 0
    state, ref = _recursion_tables()
    order, offset = S.group_index_reference(_groups("contiguous"), G_)
    x = S.lag_moments_reference(state, ref, FIRST, COUNT, REF_FIRST, True, lag, order, offset)
    _check_recovery(S.propagator_reference(x), x, lag, margin, "mirror")


def test_status_rows():
    """cells of 2, 1 and 0 members: status 1; the cells of the dyadic tables all sit on one point at state slices 1 and 2:
    status 2 on the row whose slice a that is; the NaN pattern is exactly rows 3..5 and 8..70"""
    from robobee3d_amd import score as S
    state, ref = _xtables(np.float64, "dyadic")
    order, offset = S.group_index_reference(_groups("contiguous"), G_)
    for after in (0, 1):
        prop = S.propagator_reference(S.lag_moments_reference(state, ref, FIRST, COUNT, REF_FIRST, after, 1, order, offset))
        st = prop[..., S.P_STATUS]
        assert np.all(st[:, (3, 4, 5)] == S.PROP_FEW) and np.all(st[0, (0, 1, 2, 6)] == S.PROP_NOT_PD)
        assert np.all(st[1:, (0, 1, 2, 6)] == S.PROP_OK)
        _check_pattern(prop, "after%d" % after)
        for row in prop[st != S.PROP_OK]:
            assert np.nonzero(np.isnan(row))[0].tolist() == NAN_ROWS
        assert not np.isnan(prop[st == S.PROP_OK]).any()
    # a pivot that is NaN, and one below the relative floor, in units a trace-based floor would misjudge: scaled by 1e-9 and 1e9
    x = S.lag_moments_reference(state, ref, FIRST + 2, 1, REF_FIRST + 2, 0, 1, order, offset)[:, :1]
    for scale in (1e-9, 1.0, 1e9):
        y = x.copy()
        y[..., 2:14] *= scale
        y[..., 14:92] *= scale * scale
        assert S.propagator_reference(y)[0, 0, S.P_STATUS] == S.PROP_OK
    y = x.copy()
    y[..., S.X_S2A] = np.nan
    assert S.propagator_reference(y)[0, 0, S.P_STATUS] == S.PROP_NOT_PD
    with pytest.raises(ValueError):
        S.propagator_reference(x[..., :80])
    with pytest.raises(ValueError):
        S.propagator_poles(np.zeros((2, 3, 96)))


def test_combination_over_column_blocks(margin):
    """two and three column blocks of a dyadic table equal the undivided batch bit for bit (every sum is exact); of a noise
    table counts exactly and sums within the entry bound of both sides; torch tensors combine like arrays"""
    import torch
    from robobee3d_amd import score as S
    ids = _groups("contiguous")
    order, offset = S.group_index_reference(ids, G_)
    for kind in ("dyadic", "noise"):
        state, ref = _xtables(np.float64, kind)
        whole = S.lag_moments_reference(state, ref, FIRST, COUNT, REF_FIRST, True, 3, order, offset)
        _, za, zb = _pairs(state, ref, True, 1, 3, np.float64)
        sabs = _sum_abs(za, zb, order, offset)
        for cuts in ((0, 100, 320), (0, 64, 137, 320)):          # cut inside groups 1, 2 and at a group's edge
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                o, f = S.group_index_reference(ids[lo:hi], G_)
                parts.append(S.lag_moments_reference(state[..., lo:hi], ref[..., lo:hi], FIRST, COUNT, REF_FIRST, True, 3, o, f))
            keep = [p.copy() for p in parts]
            tot = S.combine_lag_moments(parts)
            if kind == "dyadic":
                assert np.array_equal(tot, whole), cuts
            _check_xmom(tot, whole, sabs, margin, "%s %d blocks" % (kind, len(parts)), parts=len(parts))
            assert all(np.array_equal(p, k) for p, k in zip(parts, keep))
            tt = S.combine_lag_moments([torch.as_tensor(p) for p in parts])
            assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), tot)
    assert np.array_equal(S.combine_lag_moments([whole]), whole)
    with pytest.raises(ValueError):
        S.combine_lag_moments([])


def test_propagator_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    for decl in ("#define UMPC_XMOM_ROWS 96", "#define UMPC_PROP_ROWS 80",
                 "int umpcBatchLagMoments(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, "
                 "long long first, long long count, long long ref_first, int after, int lag, const int32_t *order, "
                 "const int32_t *offset, int G, double *xmom, void *stream);",
                 "int umpcBatchPropagators(umpc_batch_t *h, const double *xmom, long long count, int G, double *prop, void *stream);"):
        assert decl in flat, decl
    assert (_lib.XMOM_ROWS, _lib.PROP_ROWS) == (S.XMOM_ROWS, S.PROP_ROWS) == (96, 80)
    L = _lib.lib()
    for sym in ("umpcBatchLagMoments", "umpcBatchPropagators"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    # argument checks come before any HIP call: no device needed; the message names the call
    for lag in (1, 0, -1, (1 << 20) + 1):
        assert L.umpcBatchLagMoments(None, None, None, None, 0, 1, 0, 0, lag, None, None, 1, None, None) == -1
        assert b"umpcBatchLagMoments:" in L.umpcLastError() and b"no handle" in L.umpcLastError()
    assert L.umpcBatchPropagators(None, None, 1, 1, None, None) == -1
    assert b"umpcBatchPropagators:" in L.umpcLastError() and b"no handle" in L.umpcLastError()


def test_propagator_kernels_use_no_scratch():
    """the resource remarks of the build: the lag-moments kernel (2 dtypes x table / constant) and the propagator kernel spill
    nothing, and their LDS is what resource_limits.json records"""
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    for pat, forms in (("umpc_lagmom_kernel", 4), ("umpc_propagator_kernel", 1)):
        hits = [k for k in res if pat in k]
        assert len(hits) == forms, (pat, hits)
        assert limits[pat]["ScratchSize"] == 0 and limits[pat]["_note"]
        assert not any((pat in k or k in pat) and k != pat for k in limits), pat
        for k in hits:
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == limits[pat]["LDS"], (k, res[k])
    assert limits["umpc_propagator_kernel"]["LDS"] == 0
    for pat in ("umpc_lagmom_kernel", "umpc_propagator_kernel"):
        with pytest.raises(RuntimeError, match=pat):
            _lib._validate_resources(dict(res, **{"a_form_of_%s_with_a_frame" % pat: {"ScratchSize": 8, "LDS": limits[pat]["LDS"]}}))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _lagm(m, state, reftab, ref, first, count, ref_first, after, lag, index, xmom=None):
    """umpcBatchLagMoments on device tensors through the C ABI; a fresh `xmom` is filled with NaN first: the call has to
    overwrite every row"""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    if xmom is None:
        xmom = torch.full((count, G, 96), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchLagMoments(m.h, _ptr(state), _ptr(reftab), _ptr(ref), first, count, ref_first, int(after), int(lag), _ptr(order),
                                 _ptr(offset), G, _ptr(xmom), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return xmom


def _props(m, xmom):
    import torch
    from robobee3d_amd.batch import _ptr
    prop = torch.full((xmom.shape[0], xmom.shape[1], 80), 7.0, dtype=torch.float64, device=m.device)
    assert m.L.umpcBatchPropagators(m.h, _ptr(xmom), xmom.shape[0], xmom.shape[1], _ptr(prop), m._stream()) == 0, m.L.umpcLastError()
    return prop


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_moments_against_the_mirror(dtype, margin):
    """both layouts x dyadic / noise tables x after 0 / 1 x table / constant reference x lags 1 / 3. Dyadic: bit for bit, rows
    0..95. Noise: within the bound of _check_xmom (how often the bits agree as well is printed, not asserted)."""
    from robobee3d_amd import score as S
    dt = np.dtype(dtype)
    m = _mpc(B_, dtype)
    same = []
    for kind in ("dyadic", "noise"):
        state, ref = _xtables(dt, kind)
        d_state, d_ref = _dev(m, state), _dev(m, ref)
        cref = np.ascontiguousarray(ref[REF_FIRST])
        d_cref = _dev(m, cref)
        for layout in ("contiguous", "scattered"):
            ids = _groups(layout)
            order, offset = S.group_index_reference(ids, G_)
            index = _index(m, ids, G_)
            for after in (0, 1):
                for table in (True, False):
                    for lag in LAGS:
                        tag = "%s %s after%d %s lag%d" % (kind[:3], layout[:4], after, "tab" if table else "const", lag)
                        rf = REF_FIRST if table else 0
                        got = _lagm(m, d_state, d_ref if table else None, None if table else d_cref, FIRST, COUNT, rf, after, lag, index)
                        want = S.lag_moments_reference(state, ref if table else cref, FIRST, COUNT, rf, after, lag, order, offset, dtype=dt)
                        _, za, zb = _pairs(state, ref if table else cref, table, after, lag, dt)
                        bits = _check_xmom(got, want, _sum_abs(za, zb, order, offset), margin, tag)
                        same.append(bits)
                        if kind == "dyadic":
                            assert bits, tag
                        # the planted values spoil the rows where they are a and the rows where they are b, in groups 2 and 0
                        sk = want[..., S.X_SKIPPED]
                        assert sk.sum() == 4 and np.all(sk[[NAN_AT[0] - after - FIRST, NAN_AT[0] - after - FIRST - lag], 2] == 1)
                        assert np.all(sk[[INF_AT[0] - after - FIRST, INF_AT[0] - after - FIRST - lag], 0] == 1) and np.all(want[:, 5] == 0)
    print("lag moments bit-identical to the mirror in %d of %d comparisons" % (sum(same), len(same)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_row_depends_on_its_member_list_and_lag_alone(dtype):
    """all torch.equal on the bits: run to run, the step range cut at 5 and at 9 into two calls writing slices of one table,
    count = 0, another G with the other groups relabelled"""
    import torch
    state, ref = _xtables(np.dtype(dtype), "noise")
    m = _mpc(B_, dtype)
    d_state, d_ref = _dev(m, state), _dev(m, ref)
    bits = lambda t: t.view(torch.int64)
    for layout in ("contiguous", "scattered"):
        ids = _groups(layout)
        index = _index(m, ids, G_)
        for lag in LAGS:
            one = _lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, lag, index)
            assert not torch.isnan(one).any()
            assert torch.equal(bits(one), bits(_lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, lag, index)))
            for cut in (5, 9):
                two = torch.full_like(one, float("nan"))
                _lagm(m, d_state, d_ref, None, FIRST, cut, REF_FIRST, 1, lag, index, xmom=two[:cut])
                _lagm(m, d_state, d_ref, None, FIRST + cut, COUNT - cut, REF_FIRST + cut, 1, lag, index, xmom=two[cut:])
                assert torch.equal(bits(one), bits(two)), cut
            keep = two.clone()
            _lagm(m, d_state, d_ref, None, FIRST, 0, REF_FIRST, 1, lag, index, xmom=two)
            torch.cuda.synchronize()
            assert torch.equal(bits(two), bits(keep))
            # group 2's robots alone as group 4 of 9, every other robot relabelled
            other = np.where(ids == 2, 4, np.where(ids == 0, 7, np.where(ids == 1, 0, -1))).astype(np.int32)
            alone = _lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, lag, _index(m, other, 9))
            assert tuple(alone.shape) == (COUNT, 9, 96)
            assert torch.equal(bits(alone[:, 4]), bits(one[:, 2])) and torch.equal(bits(alone[:, 7]), bits(one[:, 0]))
            assert torch.equal(bits(alone[:, 0]), bits(one[:, 1])) and torch.all(alone[:, (1, 2, 3, 5, 6, 8)] == 0)
        assert not torch.equal(bits(_lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, 1, index)), bits(one))      # lag 1 is not lag 3


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_agreement_with_the_dispersion_kernel(dtype, margin):
    """tables without the planted NaN and Inf (the two kernels skip by different rules): rows 2..7 and 14..34 are the bits of
    umpcBatchDispersion's S1 and S2 of steps k, rows 8..13 and 35..55 those of steps k + L; for lag 1, Sba is the transpose of the
    Sba of the host mirror with the roles of a and b exchanged (the tables reversed in time), within the entry bound"""
    import torch
    from robobee3d_amd import score as S
    dt = np.dtype(dtype)
    state, ref = _xtables(dt, "noise", planted=False)
    m = _mpc(B_, dtype)
    d_state, d_ref = _dev(m, state), _dev(m, ref)
    bits = lambda t: t.contiguous().view(torch.int64)
    for layout in ("contiguous", "scattered"):
        ids = _groups(layout)
        index = _index(m, ids, G_)
        order, offset = S.group_index_reference(ids, G_)
        for lag in LAGS:
            for after in (0, 1):
                x = _lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, after, lag, index)
                da = _disp(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, after, index)
                db = _disp(m, d_state, d_ref, None, FIRST + lag, COUNT, REF_FIRST + lag, after, index)
                assert torch.equal(x[..., 0:2], da[..., 0:2]) and torch.all(x[..., 1] == 0)
                assert torch.equal(bits(x[..., 2:8]), bits(da[..., 2:8])) and torch.equal(bits(x[..., 14:35]), bits(da[..., 8:29]))
                assert torch.equal(bits(x[..., 8:14]), bits(db[..., 2:8])) and torch.equal(bits(x[..., 35:56]), bits(db[..., 8:29]))
        # time reversed: slice t of the reversed tables is slice S - 1 - t; row i' = COUNT - 1 - i pairs (t + 1, t) for row i's (t, t + 1)
        x = _lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 0, 1, index).cpu().numpy()
        rstate, rref = state[::-1], ref[::-1]
        rev = S.lag_moments_reference(rstate, rref, len(state) - 2 - FIRST - (COUNT - 1), COUNT, len(ref) - 2 - REF_FIRST - (COUNT - 1),
                                      0, 1, order, offset, dtype=dt)[::-1]
        assert np.array_equal(rev[..., 0:2], x[..., 0:2])
        want = x.copy()
        want[..., 56:92] = rev[..., 56:92].reshape(COUNT, G_, 6, 6).transpose(0, 1, 3, 2).reshape(COUNT, G_, 36)
        _, za, zb = _pairs(state, ref, True, 0, 1, dt)
        _check_xmom(x, want, _sum_abs(za, zb, order, offset), margin, "%s Sba against the exchanged roles" % layout[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_propagator_kernel_against_the_mirror(dtype, margin):
    """the propagator kernel on the device's own moments against the mirror on the same moments: status, counts and the NaN
    pattern exact, Phi, c, Q, r2 and growth within the bound of the lstsq test. The kernel performs the mirror's operations in
    the mirror's order, so bit equality is expected: printed, not asserted."""
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    same = []
    for kind in ("noise", "dyadic"):
        state, ref = _xtables(np.dtype(dtype), kind)
        d_state, d_ref = _dev(m, state), _dev(m, ref)
        for layout in ("contiguous", "scattered"):
            index = _index(m, _groups(layout), G_)
            for lag in LAGS:
                tag = "%s %s lag%d" % (kind[:3], layout[:4], lag)
                x_t = _lagm(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 0, lag, index)
                got = _props(m, x_t).cpu().numpy()
                x = x_t.cpu().numpy()
                want = S.propagator_reference(x)
                same.append(_check_props(got, want, x, margin, tag))
                st = want[..., S.P_STATUS]
                assert np.all(st[:, (3, 4, 5)] == S.PROP_FEW) and (st == S.PROP_OK).sum() >= (COUNT - 2) * 4
                if kind == "dyadic":                           # every cell of eight or more starts on one point
                    assert np.all(st[0, (0, 1, 2, 6)] == S.PROP_NOT_PD)
    print("propagators bit-identical to the mirror in %d of %d comparisons" % (sum(same), len(same)))


@pytest.mark.gpu
@pytest.mark.parametrize("lag", (1, 2))
def test_exact_recovery_on_the_device(lag, margin):
    import torch
    state, ref = _recursion_tables()
    m = _mpc(B_, "float64")
    x = _lagm(m, _dev(m, state), _dev(m, ref), None, FIRST, COUNT, REF_FIRST, 1, lag, _index(m, _groups("contiguous"), G_))
    prop = _props(m, x)
    torch.cuda.synchronize()
    _check_recovery(prop.cpu().numpy(), x.cpu().numpy(), lag, margin, "device")


@pytest.mark.gpu
def test_end_to_end_sweep_gives_the_propagators_of_its_cells(margin):
    """B = 256 as 4 cells x 64 draws of monte_carlo_draws, 12 recorded steps (fp32), set up as
    test_dispersion.test_end_to_end_sweep_gives_the_ellipsoids_of_its_cells: group_index, lag_moments, propagators through the
    Python API against the mirrors on the downloaded history"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions, monte_carlo_draws
    B, K, push = 256, 12, 3
    m = _mpc(B, "float32")
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    Ib, gain = monte_carlo_draws(B, 9, np.float32)
    m.Ib, m.gain = torch.as_tensor(Ib).to(m.device), torch.as_tensor(gain).to(m.device)
    cell = (np.arange(B) // 64).astype(np.int32)
    m.set_impulses(m.impulse_table(K, [(push, np.nonzero((cell == 1) | (cell == 3))[0], (0.0, 2.0, 0.0, 0.0, 0.0, 0.0))]))
    m.record_history(K)
    m.rollout(K)
    index = m.group_index(cell, 4)
    order, offset = S.group_index_reference(cell, 4)
    state = m.history()["state"].cpu().numpy()
    cref = m.ref.cpu().numpy()
    first, cnt = 2, K - 2 - 1
    x_t = m.lag_moments(index, lag=1, first=first, after=True)
    assert x_t.dtype == torch.float64 and tuple(x_t.shape) == (cnt, 4, 96)
    want = S.lag_moments_reference(state, cref, first, cnt, 0, True, 1, order, offset, dtype=np.float32)
    ok, za, zb = _pairs(state, cref, False, 1, 1, np.float32, first=first, count=cnt)
    assert ok.all() and np.all(want[..., 0] == 64) and np.all(want[..., 1] == 0)
    _check_xmom(x_t, want, _sum_abs(za, zb, order, offset), margin, "end to end")
    p_t = m.propagators(x_t)
    prop, x = p_t.cpu().numpy(), x_t.cpu().numpy()
    assert tuple(prop.shape) == (cnt, 4, 80) and np.all(prop[..., 0] == 64) and np.all(prop[..., 1] == 0)
    _check_props(prop, S.propagator_reference(x), x, margin, "end to end")
    usable = prop[..., S.P_STATUS] == S.PROP_OK
    assert usable.any()
    with np.errstate(invalid="ignore"):
        print("status per step and cell:\n", prop[..., S.P_STATUS], "\ngrowth:\n", prop[..., S.P_GROWTH], "\nr2_p:\n", prop[..., S.P_R2_P],
              "\nlargest |pole|:\n", np.abs(S.propagator_poles(prop, 1)).max(-1))
    # chunks into one table through `out`; lag 2 ends one step earlier
    both = torch.empty_like(x_t)
    m.lag_moments(index, 1, first, 4, after=True, out=both[:4])
    m.lag_moments(index, 1, first + 4, after=True, out=both[4:])
    assert torch.equal(both.view(torch.int64), x_t.view(torch.int64))
    pboth = torch.empty_like(p_t)
    m.propagators(both[:4], out=pboth[:4])
    m.propagators(both[4:], out=pboth[4:])
    assert torch.equal(pboth.view(torch.int64), p_t.view(torch.int64))
    assert tuple(m.lag_moments(index, lag=2, first=first, after=True).shape) == (cnt - 1, 4, 96)
    for bad in (lambda: m.lag_moments(index, 1, 0, K), lambda: m.lag_moments(index, 3, first, K - first - 2),
                lambda: m.lag_moments(index, lag=K + 1), lambda: m.lag_moments(index, lag=0), lambda: m.lag_moments(index, 1, 0, -1),
                lambda: m.lag_moments((index[0][:-1], index[1])),
                lambda: m.lag_moments(index, out=torch.empty((K - 1, 4, 32), dtype=torch.float64, device=m.device)),
                lambda: m.propagators(x_t[..., :32]), lambda: m.propagators(x_t.to(torch.float32)),
                lambda: m.propagators(x_t, out=torch.empty((cnt, 4, 48), dtype=torch.float64, device=m.device))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.gpu
def test_propagator_refusals_with_a_handle():
    """each refusal is -1 with a message naming the call, before anything is launched: the outputs are unchanged"""
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((5, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((4, 9, 64), device=m.device)
    order = torch.arange(64, dtype=torch.int32, device=m.device)
    offset = torch.tensor([0, 64], dtype=torch.int32, device=m.device)
    xmom = torch.full((3, 1, 96), 3.0, dtype=torch.float64, device=m.device)
    prop = torch.full((3, 1, 80), 5.0, dtype=torch.float64, device=m.device)
    keep = [t.clone() for t in (xmom, prop)]
    ok = dict(state=P(state), tab=None, ref=P(ref), first=0, count=3, ref_first=0, lag=1, order=P(order), offset=P(offset), G=1, xmom=P(xmom))
    for bad in (dict(state=None), dict(order=None), dict(offset=None), dict(xmom=None), dict(tab=P(tab)), dict(ref=None),
                dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(count=1 << 31), dict(G=0), dict(G=-3),
                dict(lag=0), dict(lag=-1), dict(lag=(1 << 20) + 1)):
        a = dict(ok, **bad)
        rc = L.umpcBatchLagMoments(h, a["state"], a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], 0, a["lag"], a["order"],
                                   a["offset"], a["G"], a["xmom"], s)
        assert rc == -1 and b"umpcBatchLagMoments:" in L.umpcLastError(), bad
    for bad in (dict(xmom=None), dict(prop=None), dict(count=-1), dict(count=1 << 31), dict(G=0)):
        a = dict(dict(xmom=P(xmom), prop=P(prop), count=3, G=1), **bad)
        assert L.umpcBatchPropagators(h, a["xmom"], a["count"], a["G"], a["prop"], s) == -1, bad
        assert b"umpcBatchPropagators:" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((xmom, prop), keep))
    # the same calls with good arguments go through; count = 0 changes nothing
    assert L.umpcBatchLagMoments(h, P(state), None, P(ref), 0, 0, 0, 0, 1, P(order), P(offset), 1, P(xmom), s) == 0
    assert L.umpcBatchPropagators(h, P(xmom), 0, 1, P(prop), s) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((xmom, prop), keep))
    assert L.umpcBatchLagMoments(h, P(state), None, P(ref), 0, 3, 0, 0, 2, P(order), P(offset), 1, P(xmom), s) == 0
    assert L.umpcBatchPropagators(h, P(xmom), 3, 1, P(prop), s) == 0
    torch.cuda.synchronize()
    # 64 members on the reference at both steps: n = 64, every moment 0, a cloud on one point (status 2)
    assert torch.all(xmom[..., 0] == 64) and torch.all(xmom[..., 1:] == 0) and torch.all(prop[..., 2] == 2) and torch.all(prop[..., 0] == 64)
    # a window plus lag past the history is refused by the wrapper, which knows the cursor (nothing is recorded yet)
    m.record_history(3)
    with pytest.raises(ValueError, match="lag_moments"):
        m.lag_moments(m.group_index(torch.zeros(64, dtype=torch.int32), 1), 1, 0, 3)
