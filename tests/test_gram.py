"""Trajectory modes on the device: umpcBatchGram turns a step history and its reference into the Gram matrix [66, 64] of the error
trajectories of each group's draws (fp64 MFMA), umpcBatchProject into weighted sums of the error state over each group's draws
[32] per step; trajectory_modes / trajectory_table (robobee3d_amd/score.py) turn the Gram tables into the modes of a cell and a
score-shaped table per robot.
CPU: the numpy mirrors by hand on a tiny table, against a long-double evaluation, the combination of windows, a planted rank-2
cell, the invariants of the per-robot table, the projection against two-pass numpy, exports, refusals, the resource record.
GPU: the kernels against the mirrors on the same arrays -- both dtypes, contiguous and scattered groups, windows of 1, 2, 3 and 11
steps, after 0 / 1, table / constant reference, two sets of scales --, independence of a cell's table from everything but its
member list, accumulation, one identity through both kernels and the host layer, one end-to-end sweep, refusals.
The order of accumulation inside an MFMA is not documented: on exactly representable ("dyadic") data the Gram table must equal
the mirror bit for bit, on noise it must be inside (2 N + 2) 2^-53 S_ij, N = 6 x steps, S_ij = sum |y_i y_j| -- the dot-product
bound for any order, once for the kernel and once for the mirror."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from test_score import _dev, _mpc
from test_dispersion import _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
B_, G_ = 384, 9
SIZES = (64, 63, 17, 16, 15, 1, 0, 65, 100)       # a full cell, both sides of a 16-row tile edge, one member, none, two oversized
FIRST, COUNT, REF_FIRST = 1, 11, 2
COUNTS = (1, 2, 3, 11)                            # one step is 1 1/2 MFMAs: the k tail is padded; 11 = a full stage and an odd tail
NAN_AT, INF_AT = (3, 1, 10), (2, 13, 130)         # (state slice, row, robot): a p word of a member of cell 0, a v word of one of cell 2
SCALES = ((1.0, 1.0, 1.0, 0.0, 0.0, 0.0), (1.0, 0.5, 2.0, 0.25, 0.0, 1.0))


def _groups(layout):
    """[384] ids: the cells in order and 43 ignored ids behind them, or the same array permuted ("scattered") with robots 10 and
    130 (the NaN and the Inf of the tables) put back into cells 0 and 2"""
    rest = B_ - sum(SIZES)
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(SIZES)]
                         + [np.resize(np.array([-1, G_, -5, G_ + 3], np.int32), rest)])
    assert ids.shape == (B_,)
    if layout == "scattered":
        ids = ids[np.random.default_rng(17).permutation(B_)]
        for b, g in ((10, 0), (130, 2)):
            j = int(np.nonzero((ids == g) & (np.arange(B_) != 10) & (np.arange(B_) != 130))[0][0])
            ids[j], ids[b] = ids[b], ids[j]
    assert [(ids == g).sum() for g in range(G_)] == list(SIZES) and ids[10] == 0 and ids[130] == 2
    return ids


_TABLES = {}


def _tables(dtype, kind):
    """state [13, 18, 384] and reference [14, 9, 384] in `dtype`, computed once per (dtype, kind) and never modified. "noise":
    order-one clouds around an order-ten reference, far from subnormals. "dyadic": multiples of 2^-6 of magnitude <= 1/2, so
    that with scales that are powers of two every difference, product and partial sum is exact in both dtypes. One NaN in a
    p word and one Inf in a v word of different members of different cells; rows that no kernel reads hold NaN."""
    key = (np.dtype(dtype).name, kind)
    if key not in _TABLES:
        rng = np.random.default_rng(20250307)
        ns = FIRST + COUNT + 1
        state = np.full((ns, 18, B_), np.nan)
        ref = np.full((REF_FIRST + COUNT + 1, 9, B_), np.nan)
        if kind == "noise":
            ref[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, B_)) + 0.7 * rng.normal(size=(len(ref), 3, B_))
            ref[:, 3:6] = rng.normal(size=(len(ref), 3, B_))
            drift = rng.normal(size=(1, 3, B_)) * np.linspace(0.5, 2.0, ns)[:, None, None]      # a way the draws differ over time
            state[:, 0:3] = ref[REF_FIRST - FIRST:REF_FIRST - FIRST + ns, 0:3] + drift + 0.4 * rng.normal(size=(ns, 3, B_))
            state[:, 12:15] = ref[REF_FIRST - FIRST:REF_FIRST - FIRST + ns, 3:6] + 0.5 * rng.normal(size=(ns, 3, B_))
        else:
            ref[:, 0:6] = rng.integers(-16, 17, size=(len(ref), 6, B_)) / 64.0
            state[:, 0:3] = rng.integers(-16, 17, size=(ns, 3, B_)) / 64.0
            state[:, 12:15] = rng.integers(-16, 17, size=(ns, 3, B_)) / 64.0
        state[NAN_AT] = np.nan
        state[INF_AT] = np.inf
        _TABLES[key] = (state.astype(dtype), ref.astype(dtype))
    return _TABLES[key]


def _y(state, ref, first, count, ref_first, after, scale, dtype):
    """(ok [count, B], y [count, 6, B] float64) of a window: the differences formed in `dtype`, what is not scored is 0"""
    st = np.asarray(state, dtype)[first + after:first + after + count]
    r = np.asarray(ref, dtype)
    r = r[ref_first:ref_first + count] if r.ndim == 3 else np.repeat(r[None], count, 0)
    a, b = np.concatenate([st[:, 0:3], st[:, 12:15]], 1), r[:, 0:6]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (a - b).astype(np.float64)
    ok = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    return ok, np.asarray(scale, np.float64)[None, :, None] * np.where(ok[:, None], z, 0.0)


def _sabs(y, order, offset):
    """[G, 64, 64]: S_ij = sum over steps and components of |y_i y_j| over the member slots of every cell of up to 64 (0 elsewhere)"""
    G = len(offset) - 1
    s = np.zeros((G, 64, 64))
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        if 0 < len(mem) <= 64:
            a = np.abs(y[:, :, mem]).reshape(-1, len(mem))
            s[g, :len(mem), :len(mem)] = a.T @ a
    return s


def _check_gram(got, want, sabs, nsteps, sides, margin, tag):
    """counts and row 65 exact; the NaN pattern (the flag of n > 64) that of the mirror; the matrix symmetric bit for bit and
    within sides * (N + 1) 2^-53 S_ij of the mirror, N = 6 nsteps, exactly 0 where S_ij = 0. Returns whether all bits agree."""
    got = got.to("cpu").numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (tag, got.dtype, got.shape)
    assert np.array_equal(got[:, 64:], want[:, 64:]), (tag, got[:, 64:, :8], want[:, 64:, :8])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isinf(got).any(), tag
    assert np.array_equal(got[:, :64].view(np.int64), np.ascontiguousarray(np.swapaxes(got[:, :64], 1, 2)).view(np.int64)), tag
    big = np.isnan(want[:, 0, 0])
    bound = sides * (6 * nsteps + 1) * U64 * sabs[~big]
    err = np.abs(got[~big, :64] - want[~big, :64])
    assert np.all(err[bound == 0] == 0), tag
    if margin is not None:
        margin("%s |gram - mirror| / bound" % tag, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)), 1.0)
    else:
        assert np.all(err <= bound), tag
    return bool(np.array_equal(got.view(np.int64), want.view(np.int64)))


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_gram_mirror_by_hand():
    """3 members, 2 steps, p = (x, y, 0), v = (w, 0, 0) against a reference at the origin, scale (1, 2, 1, 1/2, 0, 0); member 1 is
    not finite at step 1; a second cell of 67 members is flagged"""
    from robobee3d_amd import score as S
    B = 70
    state = np.zeros((3, 18, B))
    state[:, 3:12] = np.nan                              # the attitude is not read
    state[2] = np.nan                                    # slice 2 is read by no step (after = 0)
    state[0, 0, :3], state[0, 1, :3], state[0, 12, :3] = [1, 2, 3], [0, 1, 0], [1, 0, -1]
    state[1, 0, :3], state[1, 1, :3], state[1, 12, :3] = [2, np.nan, 1], [1, 5, 1], [0, 0, 2]
    ref = np.zeros((9, B))
    ref[6:9] = np.nan
    group = np.array([0, 0, 0] + [1] * 67, np.int32)
    order, offset = S.group_index_reference(group, 2)
    scale = (1, 2, 1, 0.5, 0, 0)
    g = S.gram_reference(state, ref, 0, 2, 0, False, order, offset, scale=scale)
    assert g.shape == (2, 66, 64) and (S.GRAM_ROWS, S.GRAM_COLS, S.PROJ_ROWS, S.PROJ_MAX) == (66, 64, 32, 4)
    # y: step 0: (1, 0, 0, .5) (2, 2, 0, 0) (3, 0, 0, -.5); step 1: (2, 2, 0, 0), not scored, (1, 2, 0, 1)
    want = np.zeros((66, 64))
    want[:3, :3] = [[9.25, 2.0, 8.75], [2.0, 8.0, 6.0], [8.75, 6.0, 15.25]]
    want[64, :3] = [2, 1, 2]
    want[65, :8] = [2, 3, 1, 2, 1, 0.5, 0, 0]
    assert np.array_equal(g[0], want), g[0, :4, :4]
    assert np.isnan(g[1, :64]).all() and np.all(g[1, 64] == 0) and g[1, 65, :8].tolist() == [2, 67, 1, 2, 1, 0.5, 0, 0] and np.all(g[1, 65, 8:] == 0)
    # fp32 handles give the same numbers on dyadic tables; after = 1 is after = 0 on the table moved by one slice; a table
    assert np.array_equal(S.gram_reference(state, ref, 0, 2, 0, False, order, offset, scale=scale, dtype=np.float32), g, equal_nan=True)
    assert np.array_equal(S.gram_reference(state, np.repeat(ref[None], 4, 0), 0, 1, 2, True, order, offset, scale=scale)[0, :3, :3],
                          [[8, 0, 6], [0, 0, 0], [6, 0, 6]])
    # accumulation: step 0, then step 1 added to it; count = 0 changes nothing; an empty window without accumulate holds zeros
    a = S.gram_reference(state, ref, 0, 1, 0, False, order, offset, scale=scale)
    assert a[0, 64, :3].tolist() == [1, 1, 1] and a[0, 65, 0] == 1 and a[0, 1, 1] == 8
    b = S.gram_reference(state, ref, 1, 1, 0, False, order, offset, scale=scale, accumulate=True, gram=a)
    assert np.array_equal(b, g, equal_nan=True) and a[0, 65, 0] == 1
    assert np.array_equal(S.gram_reference(state, ref, 1, 0, 0, False, order, offset, scale=scale, accumulate=True, gram=g), g, equal_nan=True)
    e = S.gram_reference(state, ref, 1, 0, 0, False, order, offset, scale=scale)
    assert np.all(e[0, :65] == 0) and e[0, 65, :8].tolist() == [0, 3, 1, 2, 1, 0.5, 0, 0]
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(scale=(1, 1, 1, 1, 1, -1)), dict(scale=(1, 1, 1, np.nan, 0, 0)),
                dict(scale=(1, 1, 1)), dict(accumulate=True)):
        kw = dict(first=0, count=2, ref_first=0, after=False, order=order, offset=offset)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.gram_reference(state, ref, **kw)


def test_gram_mirror_against_long_double(margin):
    """the mirror's half of the bound: |mirror - sum in long double| <= (N + 1) 2^-53 S_ij on the noise table, 11 steps, both
    scales (the long-double sum of N <= 66 products carries N 2^-64 S_ij, 2000 times less)"""
    from robobee3d_amd import score as S
    assert np.finfo(np.longdouble).nmant >= 63
    state, ref = _tables(np.float64, "noise")
    order, offset = S.group_index_reference(_groups("contiguous"), G_)
    for scale in SCALES:
        got = S.gram_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, scale=scale)
        _, y = _y(state, ref, FIRST, COUNT, REF_FIRST, 1, scale, np.float64)
        sabs = _sabs(y, order, offset)
        worst = 0.0
        for g in range(G_):
            mem = order[offset[g]:offset[g + 1]]
            if not 0 < len(mem) <= 64:
                continue
            a = y[:, :, mem].reshape(-1, len(mem)).astype(np.longdouble)
            exact = np.zeros((len(mem), len(mem)), np.longdouble)
            for row in a:
                exact += np.multiply.outer(row, row)
            err = np.abs(got[g, :len(mem), :len(mem)].astype(np.longdouble) - exact).astype(np.float64)
            bound = (6 * COUNT + 1) * U64 * sabs[g, :len(mem), :len(mem)]
            assert np.all(err[bound == 0] == 0)
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
        margin("scale %s |mirror - long double| / ((N + 1) u S)" % (scale,), worst, 1.0)


def test_combine_grams_of_two_windows(margin):
    """the 11 steps as 4 + 7 and as 5 + 6: dyadic equal bits, noise inside (2 N + 2) u S; n or scales that differ are refused;
    torch tensors combine like arrays"""
    import torch
    from robobee3d_amd import score as S
    order, offset = S.group_index_reference(_groups("contiguous"), G_)
    scale = SCALES[1]
    for kind in ("dyadic", "noise"):
        state, ref = _tables(np.float64, kind)
        whole = S.gram_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, scale=scale)
        _, y = _y(state, ref, FIRST, COUNT, REF_FIRST, 1, scale, np.float64)
        for cut in (4, 5):
            parts = [S.gram_reference(state, ref, FIRST, cut, REF_FIRST, True, order, offset, scale=scale),
                     S.gram_reference(state, ref, FIRST + cut, COUNT - cut, REF_FIRST + cut, True, order, offset, scale=scale)]
            keep = [p.copy() for p in parts]
            tot = S.combine_grams(parts)
            same = _check_gram(tot, whole, _sabs(y, order, offset), COUNT, 2, margin if kind == "noise" else None, "%s cut %d" % (kind[:3], cut))
            assert same or kind == "noise"
            assert all(np.array_equal(p, k, equal_nan=True) for p, k in zip(parts, keep))
            tt = S.combine_grams([torch.as_tensor(p) for p in parts])
            assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), tot, equal_nan=True)
    assert np.array_equal(S.combine_grams([whole]), whole, equal_nan=True)
    other = S.gram_reference(state, ref, FIRST, 2, REF_FIRST, True, order, offset, scale=SCALES[0])
    o2, f2 = S.group_index_reference(np.roll(_groups("contiguous"), 1), G_)
    for bad in ([], [whole, other], [whole, S.gram_reference(state, ref, FIRST, 2, REF_FIRST, True, o2, f2[:-1], scale=scale)]):
        with pytest.raises(ValueError):
            S.combine_grams(bad)


def test_planted_rank_two_cell():
    """n = 64, 11 steps, z_x(i, k) = a_i (k - 5) / 8 + 1/4, z_y(i, k) = b_i / 4 with a_i = i - 31.5 and b = +1 on the outer
    quarters, -1 inside: a and b sum to 0 and a . b = 0, everything exact in doubles. Gc = |t|^2 a a^T + (11 / 16) b b^T with
    |t|^2 = sum ((k - 5) / 8)^2 = 110 / 64: lam = (21840 * 110 / 64, 64 * 11 / 16) = (37537.5, 44); the offset 1/4 must go."""
    from robobee3d_amd import score as S
    n, K = 64, 11
    a = np.arange(n) - 31.5
    b = np.where((np.arange(n) < 16) | (np.arange(n) >= 48), 1.0, -1.0)
    assert a.sum() == 0 and b.sum() == 0 and a @ b == 0
    state = np.zeros((K, 18, n))
    state[:, 0] = a[None] * ((np.arange(K) - 5) / 8)[:, None] + 0.25
    state[:, 1] = b[None] / 4
    order, offset = S.group_index_reference(np.zeros(n, np.int32), 1)
    gram = S.gram_reference(state, np.zeros((9, n)), 0, K, 0, False, order, offset)
    md = S.trajectory_modes(gram, M=3)
    assert md["status"].tolist() == [S.MODES_OK] and md["nvalid"].tolist() == [64]
    lam = md["lam"][0]
    assert abs(lam[0] - 37537.5) <= 1e-10 * lam[0] and abs(lam[1] - 44.0) <= 1e-10 * lam[0] and abs(lam[2]) <= 1e-10 * lam[0]
    W = md["W"][0]
    # up to the fixed sign: the component of largest magnitude is positive (the magnitudes of a and of b tie in exact
    # arithmetic -- a_0 = -a_63, |b_i| = 1 --, so which slot decides is left to the rounding of eigh)
    for k, v in ((0, a / np.linalg.norm(a)), (1, b / 8.0)):
        assert min(np.abs(W[:, k] - v).max(), np.abs(W[:, k] + v).max()) <= 1e-9, k
        assert W[int(np.argmax(np.abs(W[:, k]))), k] > 0 and abs(W[:, k].sum()) <= 1e-9, k
    want_neff = (37537.5 + 44) ** 2 / (37537.5 ** 2 + 44 ** 2)
    assert abs(md["neff"][0] - want_neff) <= 1e-9 and abs(md["share"][0].sum() - 1.0) <= 1e-10 and abs(md["trace"][0] - 37581.5) <= 1e-7
    tab = S.trajectory_table(gram, md, order, offset, n)
    assert np.all(tab[S.T_VALID] == 1) and np.abs(tab[S.T_MODE0] - np.sqrt(lam[0]) * W[:, 0]).max() == 0
    assert np.abs(tab[S.T_GCII] - (110 / 64 * a * a + 11 / 16)).max() <= 1e-9 and tab[S.T_MEDOID].sum() == 1
    assert tab[S.T_MEDOID, 31] + tab[S.T_MEDOID, 32] == 1        # the two draws next to the mean path
    # a cell on one path, a cell of one: not usable, rows NaN
    flat = S.gram_reference(np.full((K, 18, n), 0.5), np.zeros((9, n)), 0, K, 0, False, order, offset)
    md = S.trajectory_modes(np.concatenate([flat, gram[:, :, :]]), M=2)
    assert md["status"].tolist() == [S.MODES_FLAT, S.MODES_OK] and np.isnan(md["lam"][0]).all() and np.isnan(md["W"][0]).all()
    with pytest.raises(ValueError):
        S.trajectory_modes(gram[0])


def test_trajectory_table_invariants_on_the_noise_gram():
    from robobee3d_amd import score as S
    state, ref = _tables(np.float64, "noise")
    ids = _groups("contiguous")
    order, offset = S.group_index_reference(ids, G_)
    scale = SCALES[1]
    gram = S.gram_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, scale=scale)
    md = S.trajectory_modes(gram)
    assert md["status"].tolist() == [0, 0, 0, 0, 0, S.MODES_FEW, S.MODES_FEW, S.MODES_BIG, S.MODES_BIG]
    assert md["nvalid"].tolist() == [63, 63, 16, 16, 15, 1, 0, 0, 0]
    tab = S.trajectory_table(gram, md, order, offset, B_)
    assert tab.shape == (12, B_) and tab.dtype == np.float64
    _, y = _y(state, ref, FIRST, COUNT, REF_FIRST, 1, scale, np.float64)
    sabs = _sabs(y, order, offset)
    for g in range(5):
        mem = order[offset[g]:offset[g + 1]]
        n = len(mem)
        valid = gram[g, 64, :n] == COUNT
        rob = mem[valid]
        assert np.all(tab[S.T_VALID, rob] == 1) and np.all(tab[:, mem[~valid]] == 0)
        d = np.diag(gram[g])[:n]
        d2 = (d[:, None] + d[None, :]) - 2 * gram[g, :n, :n]
        sd = np.diag(sabs[g])[:n]
        bound = (6 * COUNT + 4) * U64 * (sd[:, None] + sd[None, :] + 2 * sabs[g, :n, :n])
        assert np.array_equal(d2, d2.T) and np.all(d2 >= -bound) and np.all(np.diag(d2) == 0)
        assert np.all(tab[S.T_MIN_D2, rob] > 0) and np.all(tab[S.T_MEAN_D2, rob] >= tab[S.T_MIN_D2, rob])
        med = rob[tab[S.T_MEDOID, rob] == 1]
        assert len(med) == 1 and tab[S.T_MEAN_D2, med[0]] == tab[S.T_MEAN_D2, rob].min() and tab[S.T_RANK, med[0]] == 0
        assert sorted(tab[S.T_RANK, rob].tolist()) == list(range(len(rob)))
        assert np.all(np.diff(tab[S.T_MEAN_D2, rob][np.argsort(tab[S.T_RANK, rob])]) >= 0)
        assert abs(tab[S.T_SHARE, rob].sum() - 1.0) <= 1e-12 and np.all(np.isin(tab[S.T_NEAREST, rob], rob))
        assert np.all(tab[S.T_NEAREST, rob] != rob) and np.all(tab[S.T_GII, rob] == d[valid])
        for k in range(3):       # a mode score is sqrt(lam) W: its square sums to lam over the cell
            assert abs((tab[S.T_MODE0 + k, rob] ** 2).sum() - md["lam"][g, k]) <= 1e-12 * md["trace"][g]
    assert np.all(tab[:, ids >= 5] == 0) and np.all(tab[:, ids < 0] == 0)
    assert tab[S.T_VALID, NAN_AT[2]] == 0 and tab[S.T_VALID, INF_AT[2]] == 0
    # other non-finite words in the same member-steps: nobody else's row moves
    st2 = state.copy()
    st2[NAN_AT], st2[INF_AT] = -np.inf, np.nan
    st2[NAN_AT[0], 12, NAN_AT[2]] = np.nan
    gram2 = S.gram_reference(st2, ref, FIRST, COUNT, REF_FIRST, True, order, offset, scale=scale)
    assert np.array_equal(S.trajectory_table(gram2, S.trajectory_modes(gram2), order, offset, B_), tab)
    # the weights of the projection: W scattered to the robots, 0 outside the usable cells
    w = S.mode_weights(md, order, offset, B_)
    assert w.shape == (3, B_) and np.all(w[:, ids >= 5] == 0) and np.all(w[:, ids < 0] == 0) and np.all(w[:, NAN_AT[2]] == 0)
    assert np.array_equal(w[:, order[offset[2]:offset[3]]], md["W"][2, :17].T) and S.mode_weights(md, order, offset, B_, M=1).shape == (1, B_)
    with pytest.raises(ValueError):
        S.mode_weights(md, order, offset, B_, M=4)


def test_projection_mirror_against_two_pass_numpy(margin):
    """project_reference against numpy's own sum of the same terms within twice the dispersion bound ((n + 9) 2^-53 sum |term| for
    each side: n - 1 additions in any order, one product, the tree's padding); with weights 1 / n it reproduces
    dispersion_reference's S1 / n within (2 n + 20) 2^-53 sum |z| / n (the bound of each side and the division)"""
    from robobee3d_amd import score as S
    state, ref = _tables(np.float64, "noise")
    ids = _groups("scattered")
    order, offset = S.group_index_reference(ids, G_)
    rng = np.random.default_rng(3)
    w = rng.normal(size=(3, B_))
    bnan = int(order[offset[8] + 3])                            # a member of the cell of 100
    w[1, bnan] = np.nan
    proj = S.project_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, w)
    assert proj.shape == (COUNT, G_, 32) and np.all(proj[..., 2 + 18:] == 0)
    ok, z = _y(state, ref, FIRST, COUNT, REF_FIRST, 1, (1,) * 6, np.float64)
    ok = ok & np.isfinite(w).all(0)[None]
    worst = 0.0
    for g in range(G_):
        mem = order[offset[g]:offset[g + 1]]
        assert np.array_equal(proj[:, g, 0], ok[:, mem].sum(1)) and np.array_equal(proj[:, g, 1], len(mem) - ok[:, mem].sum(1))
        t = np.where(ok[:, None, None, mem], w[None, :, None, mem] * z[:, None, :, mem], 0.0).reshape(COUNT, 18, len(mem))
        err, bound = np.abs(proj[:, g, 2:20] - t.sum(2)), 2 * (len(mem) + 9) * U64 * np.abs(t).sum(2)
        assert np.all(err[bound == 0] == 0)
        worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    margin("|project - numpy sum| / bound", worst, 1.0)
    assert proj[:, 8, 1].min() >= 1                             # the robot with a NaN weight is skipped at every step
    mom = S.dispersion_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset)
    nmem = np.diff(offset)[ids.clip(0, G_ - 1)].astype(np.float64)
    mean = S.project_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, (1.0 / np.maximum(nmem, 1.0))[None])
    assert np.array_equal(mean[..., 0:2], mom[..., 0:2]) and np.all(mean[..., 8:] == 0)
    worst = 0.0
    for g in range(G_):
        mem = order[offset[g]:offset[g + 1]]
        if len(mem):
            sz = np.abs(z[:, :, mem]).sum(2) / len(mem)
            err, bound = np.abs(mean[:, g, 2:8] - mom[:, g, 2:8] / len(mem)), (2 * len(mem) + 20) * U64 * sz
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
    margin("|project(1 / n) - S1 / n| / bound", worst, 1.0)
    for bad in (np.zeros((5, B_)), np.zeros((0, B_)), np.zeros(B_), np.zeros((2, B_ - 1))):
        with pytest.raises(ValueError):
            S.project_reference(state, ref, FIRST, COUNT, REF_FIRST, True, order, offset, bad)


def test_gram_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    for decl in ("#define UMPC_GRAM_ROWS 66", "#define UMPC_GRAM_COLS 64", "#define UMPC_PROJ_ROWS 32", "#define UMPC_PROJ_MAX 4",
                 "int umpcBatchGram(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, "
                 "long long first, long long count, long long ref_first, int after, const int32_t *order, const int32_t *offset, int G, "
                 "const double *scale /* host, [6] */, int accumulate, double *gram, void *stream);",
                 "int umpcBatchProject(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, "
                 "long long first, long long count, long long ref_first, int after, const int32_t *order, const int32_t *offset, int G, "
                 "const double *weights /* device, [M][B] */, int M, double *proj, void *stream);"):
        assert decl in flat, decl
    assert (_lib.GRAM_ROWS, _lib.GRAM_COLS, _lib.PROJ_ROWS, _lib.PROJ_MAX) == (S.GRAM_ROWS, S.GRAM_COLS, S.PROJ_ROWS, S.PROJ_MAX) == (66, 64, 32, 4)
    L = _lib.lib()
    for sym in ("umpcBatchGram", "umpcBatchProject"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    # argument checks come before any HIP call: no device needed; the message names the function and what is missing
    sc = (C.c_double * 6)(1, 1, 1, 0, 0, 0)
    assert L.umpcBatchGram(None, None, None, None, 0, 1, 0, 0, None, None, 1, sc, 0, None, None) == -1
    assert b"umpcBatchGram:" in L.umpcLastError() and b"no handle" in L.umpcLastError()
    assert L.umpcBatchProject(None, None, None, None, 0, 1, 0, 0, None, None, 1, None, 1, None, None) == -1
    assert b"umpcBatchProject:" in L.umpcLastError() and b"no handle" in L.umpcLastError()


def test_gram_kernels_resource_record():
    """the resource remarks of the build: both kernels (2 dtypes x table / constant) spill nothing, and their LDS is what
    resource_limits.json records -- the Gram kernel's one stage of y (48 rows at a pitch of 80 doubles) and its step counts"""
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    for pat, forms, lds in (("umpc_gram_kernel", 4, 48 * 80 * 8 + 4 * 64 * 4), ("umpc_project_kernel", 4, 0)):
        hits = [k for k in res if pat in k]
        assert len(hits) == forms, (pat, hits)
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds}
        for k in hits:
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == lds, (k, res[k])
        with pytest.raises(RuntimeError, match=pat):
            _lib._validate_resources(dict(res, **{"a_form_of_%s_with_a_frame" % pat: {"ScratchSize": 8, "LDS": lds}}))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _gram(m, state, reftab, ref, first, count, ref_first, after, index, scale, gram=None):
    """umpcBatchGram on device tensors through the C ABI; a fresh table is filled with NaN first and overwritten (accumulate = 0),
    a given one is accumulated into"""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    acc = gram is not None
    if gram is None:
        gram = torch.full((G, 66, 64), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchGram(m.h, _ptr(state), _ptr(reftab), _ptr(ref), first, count, ref_first, int(after), _ptr(order), _ptr(offset), G,
                           (C.c_double * 6)(*scale), int(acc), _ptr(gram), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return gram


def _project(m, state, reftab, ref, first, count, ref_first, after, index, weights):
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    proj = torch.full((count, G, 32), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchProject(m.h, _ptr(state), _ptr(reftab), _ptr(ref), first, count, ref_first, int(after), _ptr(order), _ptr(offset), G,
                              _ptr(weights), int(weights.shape[0]), _ptr(proj), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return proj


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gram_against_the_mirror(dtype, margin):
    """dyadic / noise x both layouts x windows of 1, 2, 3, 11 steps x after 0 / 1 x table / constant reference x both scales.
    Dyadic: all 66 rows bit for bit. Noise: _check_gram with both sides of the bound (whether the bits agree as well is printed)."""
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    dt = np.dtype(dtype)
    same, worst = [], {}
    for kind in ("dyadic", "noise"):
        state, ref = _tables(dt, kind)
        d_state, d_ref = _dev(m, state), _dev(m, ref)
        cref = np.ascontiguousarray(ref[REF_FIRST])
        d_cref = _dev(m, cref)
        for layout in ("contiguous", "scattered"):
            ids = _groups(layout)
            order, offset = S.group_index_reference(ids, G_)
            index = _index(m, ids, G_)
            for count in COUNTS:
                for after in (0, 1):
                    for table in (True, False):
                        for si, scale in enumerate(SCALES):
                            tag = "%s %s n%d after%d %s s%d" % (kind[:3], layout[:4], count, after, "tab" if table else "const", si)
                            r, rf = (ref, REF_FIRST) if table else (cref, 0)
                            got = _gram(m, d_state, d_ref if table else None, None if table else d_cref, FIRST, count, rf, after, index, scale)
                            want = S.gram_reference(state, r, FIRST, count, rf, after, order, offset, scale=scale, dtype=dt)
                            _, y = _y(state, r, FIRST, count, rf, after, scale, dt)
                            got = got.cpu().numpy()
                            bits = _check_gram(got, want, _sabs(y, order, offset), count, 2, None, tag)
                            same.append(bits)
                            if kind == "dyadic":
                                assert bits, tag
                            else:
                                sab = _sabs(y, order, offset)[:7]
                                bound = 2 * (6 * count + 1) * U64 * sab
                                err = np.abs(got[:7, :64] - want[:7, :64])
                                worst[count] = max(worst.get(count, 0.0), float(np.max(err[bound > 0] / bound[bound > 0], initial=0.0)))
                            # cells 7 and 8 carry the flag, no other cell holds a NaN or an Inf despite the planted ones
                            assert np.isnan(got[7:, :64]).all() and np.all(got[7:, 64] == 0) and got[7, 65, 1] == 65 and got[8, 65, 1] == 100
                            assert np.isfinite(got[:7]).all() and np.all(got[6, :65] == 0) and np.all(got[:, 65, 0] == count)
                            if count == COUNT:      # the planted values did what they are there for
                                for g, b, n in ((0, NAN_AT[2], 64), (2, INF_AT[2], 17)):
                                    slot = int(np.nonzero(order[offset[g]:offset[g + 1]] == b)[0][0])
                                    assert want[g, 64, slot] == COUNT - 1 and (want[g, 64, :n] == COUNT).sum() == n - 1, (tag, g)
    for count, w in sorted(worst.items()):
        margin("noise %d steps |gram - mirror| / ((2 N + 2) u S)" % count, w, 1.0)
    print("Gram tables bit-identical to the mirror in %d of %d comparisons" % (sum(same), len(same)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_gram_table_depends_on_its_member_list_alone(dtype):
    """all torch.equal on the bits: run to run; a cell computed alone (G = 1) against its rows in the full call; the same cells
    listed in another order"""
    import torch
    state, ref = _tables(np.dtype(dtype), "noise")
    m = _mpc(B_, dtype)
    d_state, d_ref = _dev(m, state), _dev(m, ref)
    bits = lambda t: t.view(torch.int64)
    scale = SCALES[1]
    for layout in ("contiguous", "scattered"):
        ids = _groups(layout)
        one = _gram(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, _index(m, ids, G_), scale)
        assert torch.equal(bits(one), bits(_gram(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, _index(m, ids, G_), scale)))
        for g in (0, 2, 4, 5, 7):
            alone = _gram(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, _index(m, np.where(ids == g, 0, -1).astype(np.int32), 1), scale)
            assert tuple(alone.shape) == (1, 66, 64) and torch.equal(bits(alone[0]), bits(one[g])), (layout, g)
        perm = np.array([4, 0, 7, 8, 2, 6, 1, 3, 5])
        other = np.where((ids >= 0) & (ids < G_), perm[ids.clip(0, G_ - 1)], -1).astype(np.int32)
        moved = _gram(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, _index(m, other, G_), scale)
        for g in range(G_):
            assert torch.equal(bits(moved[perm[g]]), bits(one[g])), (layout, g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_gram_accumulates_windows(dtype, margin):
    """the 11 steps as 4 + 7 and 5 + 6 (overwrite, then accumulate) against the one call: dyadic equal bits, noise inside the bound
    with N of the whole window (both sides are the kernel: two sides of the bound); count = 0 with accumulate changes nothing"""
    import torch
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    dt = np.dtype(dtype)
    scale = SCALES[1]
    for kind in ("dyadic", "noise"):
        state, ref = _tables(dt, kind)
        d_state, d_ref = _dev(m, state), _dev(m, ref)
        for layout in ("contiguous", "scattered"):
            ids = _groups(layout)
            order, offset = S.group_index_reference(ids, G_)
            index = _index(m, ids, G_)
            one = _gram(m, d_state, d_ref, None, FIRST, COUNT, REF_FIRST, 1, index, scale).cpu().numpy()
            _, y = _y(state, ref, FIRST, COUNT, REF_FIRST, 1, scale, dt)
            for cut in (4, 5):
                two = _gram(m, d_state, d_ref, None, FIRST, cut, REF_FIRST, 1, index, scale)
                _gram(m, d_state, d_ref, None, FIRST + cut, COUNT - cut, REF_FIRST + cut, 1, index, scale, gram=two)
                tag = "%s %s cut %d" % (kind[:3], layout[:4], cut)
                same = _check_gram(two, one, _sabs(y, order, offset), COUNT, 2, margin if kind == "noise" else None, tag)
                assert same or kind == "noise", tag
            keep = two.clone()
            _gram(m, d_state, d_ref, None, FIRST, 0, REF_FIRST, 1, index, scale, gram=two)
            torch.cuda.synchronize()
            assert torch.equal(two.view(torch.int64), keep.view(torch.int64))
            # an empty window without accumulate writes the table of an empty window
            empty = _gram(m, d_state, d_ref, None, FIRST, 0, REF_FIRST, 1, index, scale).cpu().numpy()
            assert np.array_equal(empty, S.gram_reference(state, ref, FIRST, 0, REF_FIRST, 1, order, offset, scale=scale, dtype=dt), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_projection_against_the_mirror(dtype):
    """bit for bit on both kinds of data, both layouts, M = 1, 3, 4, after 0 / 1, table / constant reference: the cells of 65 and
    100 take two trips, one robot has a NaN weight and one an Inf, the tables hold their NaN and Inf; rows beyond 2 + 6 M are +0"""
    import torch
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    dt = np.dtype(dtype)
    rng = np.random.default_rng(5)
    for kind in ("dyadic", "noise"):
        state, ref = _tables(dt, kind)
        d_state, d_ref = _dev(m, state), _dev(m, ref)
        cref = np.ascontiguousarray(ref[REF_FIRST])
        d_cref = _dev(m, cref)
        w = rng.normal(size=(4, B_)) if kind == "noise" else rng.integers(-8, 9, size=(4, B_)) / 8.0
        w[0, 300], w[2, 5] = np.nan, np.inf          # a member of the cell of 100 (contiguous layout), a member of cell 0
        for layout in ("contiguous", "scattered"):
            ids = _groups(layout)
            order, offset = S.group_index_reference(ids, G_)
            index = _index(m, ids, G_)
            for M in (1, 3, 4):
                d_w = _dev(m, np.ascontiguousarray(w[:M]))
                for after, table, count in ((1, True, COUNT), (0, False, COUNT), (1, False, 3), (0, True, 1)):
                    r, rf = (ref, REF_FIRST) if table else (cref, 0)
                    got = _project(m, d_state, d_ref if table else None, None if table else d_cref, FIRST, count, rf, after, index, d_w)
                    want = S.project_reference(state, r, FIRST, count, rf, after, order, offset, w[:M], dtype=dt)
                    got = got.cpu().numpy()
                    tag = (kind, layout, M, after, table, count)
                    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (tag, np.argwhere(got != want)[:5])
                    assert np.all(got[..., 2 + 6 * M:].view(np.int64) == 0) and np.isfinite(got).all(), tag
                    if layout == "contiguous":      # the robots with the Inf (row 2 of the weights) and the NaN weight are skipped
                        assert np.all(got[:, 0, 1] >= (1 if M >= 3 else 0)) and np.all(got[:, 8, 1] >= 1), tag


@pytest.mark.gpu
def test_mode_energy_through_both_kernels():
    """cell 0 of the noise table: with W from trajectory_modes of the device's Gram table as the weights of umpcBatchProject,
    sum_k sum_c (scale_c proj[k, 0, 2 + 6 m + c])^2 = lam_m to 1e-10 of trace(Gc): W^T Gram W = W^T Gc W when sum W = 0 (the
    member that is not finite at one step is not valid: its weight is 0, so the projection leaves it out as the modes do)"""
    from robobee3d_amd import score as S
    m = _mpc(B_, "float32")
    state, ref = _tables(np.float32, "noise")
    ids = _groups("contiguous")
    order, offset = S.group_index_reference(ids, G_)
    index = _index(m, ids, G_)
    scale = SCALES[1]
    gram = _gram(m, _dev(m, state), _dev(m, ref), None, FIRST, COUNT, REF_FIRST, 1, index, scale).cpu().numpy()
    md = S.trajectory_modes(gram, M=3)
    assert md["status"][0] == S.MODES_OK and md["nvalid"][0] == 63 and np.abs(md["W"][0].sum(0)).max() <= 1e-12
    w = S.mode_weights(md, order, offset, B_)
    proj = _project(m, _dev(m, state), _dev(m, ref), None, FIRST, COUNT, REF_FIRST, 1, index, _dev(m, w)).cpu().numpy()
    for k in range(3):
        e = ((np.asarray(scale)[None] * proj[:, 0, 2 + 6 * k:8 + 6 * k]) ** 2).sum()
        assert abs(e - md["lam"][0, k]) <= 1e-10 * md["trace"][0], (k, e, md["lam"][0, k])
    assert md["lam"][0, 0] > md["lam"][0, 1] > md["lam"][0, 2] > 0 and 1.0 < md["neff"][0] < 63.0


@pytest.mark.gpu
def test_end_to_end_sweep_gives_the_modes_of_its_cells(margin):
    """B = 256 as 4 cells x 64 draws of monte_carlo_draws from drawn initial offsets, 12 recorded steps (fp32): trajectory_gram in
    two chunks through out=, trajectory_modes, trajectory_table, ensemble_projection and score_quantiles through the Python API
    against the mirrors on the downloaded history, inside the bounds of the kernel tests; every cell has exactly one medoid"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions, monte_carlo_draws
    B, K = 256, 12
    m = _mpc(B, "float32")
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    Ib, gain = monte_carlo_draws(B, 9, np.float32)
    m.Ib, m.gain = torch.as_tensor(Ib).to(m.device), torch.as_tensor(gain).to(m.device)
    cell = (np.arange(B) // 64).astype(np.int32)
    m.record_history(K)
    m.rollout(K)
    index = m.group_index(cell, 4)
    order, offset = S.group_index_reference(cell, 4)
    state = m.history()["state"].cpu().numpy()
    cref = m.ref.cpu().numpy()
    scale = (1, 1, 1, 0.25, 0.25, 0.25)
    gram_t = m.trajectory_gram(index, 0, 5, after=True, scale=scale)
    assert gram_t.dtype == torch.float64 and tuple(gram_t.shape) == (4, 66, 64)
    assert m.trajectory_gram(index, 5, after=True, scale=scale, out=gram_t) is gram_t
    want = S.gram_reference(state, cref, 0, K, 0, True, order, offset, scale=scale, dtype=np.float32)
    _, y = _y(state, cref, 0, K, 0, 1, scale, np.float32)
    _check_gram(gram_t, want, _sabs(y, order, offset), K, 2, margin, "end to end")
    gram = gram_t.cpu().numpy()
    assert np.all(gram[:, 64] == K) and np.all(gram[:, 65, 0] == K) and np.all(gram[:, 65, 1] == 64)
    md = m.trajectory_modes(gram_t)
    assert np.all(md["status"] == S.MODES_OK) and np.all(md["nvalid"] == 64) and np.all(md["lam"][:, 0] > 0)
    assert np.all(np.abs(md["share"].sum(1)) <= 1 + 1e-12) and np.all(md["neff"] >= 1 - 1e-12)
    print("share of the first three modes per cell:\n", md["share"], "\nneff:", md["neff"])
    tab_t = m.trajectory_table(gram_t, md, index)
    assert tab_t.dtype == torch.float32 and tuple(tab_t.shape) == (12, B) and tab_t.device == m.state.device
    tab = S.trajectory_table(gram, md, order, offset, B)
    assert np.array_equal(tab_t.cpu().numpy(), tab.astype(np.float32))
    assert np.all(tab[S.T_VALID] == 1) and [tab[S.T_MEDOID, cell == g].sum() for g in range(4)] == [1, 1, 1, 1]
    w_t = m.mode_weights(md, index)
    assert tuple(w_t.shape) == (3, B) and w_t.dtype == torch.float64
    proj = m.ensemble_projection(index, w_t, after=True).cpu().numpy()
    wantp = S.project_reference(state, cref, 0, K, 0, True, order, offset, w_t.cpu().numpy(), dtype=np.float32)
    assert np.array_equal(proj.view(np.int64), wantp.view(np.int64))
    sc = np.asarray(scale)
    for g in range(4):
        e = ((sc[None] * proj[:, g, 2:8]) ** 2).sum()
        assert abs(e - md["lam"][g, 0]) <= 1e-10 * md["trace"][g]
    q = m.score_quantiles(tab_t, index, (0.5,), 3).cpu().numpy()
    assert np.array_equal(q, S.score_quantiles_reference(tab_t.cpu().numpy(), order, offset, (0.5,), 3))
    # the checks of the wrappers
    for bad in (lambda: m.trajectory_gram(index, 0, K + 1), lambda: m.trajectory_gram((index[0][:-1], index[1])),
                lambda: m.trajectory_gram(index, out=torch.empty((4, 66, 32), dtype=torch.float64, device=m.device)),
                lambda: m.trajectory_gram(index, scale=(1, 1, 1)), lambda: m.trajectory_modes(gram_t[:, :64]),
                lambda: m.trajectory_table(gram_t[:2].contiguous(), md, index),
                lambda: m.ensemble_projection(index, w_t[:, :-1].contiguous()), lambda: m.ensemble_projection(index, w_t.float()),
                lambda: m.ensemble_projection(index, w_t.cpu()), lambda: m.ensemble_projection(index, w_t, 0, K + 1)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="umpcBatchGram"):
        m.trajectory_gram(index, scale=(1, 1, 1, 0, 0, -1))


@pytest.mark.gpu
def test_gram_refusals_with_a_handle():
    """each refusal is -1 with a message naming the call, before anything is launched: the outputs are unchanged"""
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((4, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((3, 9, 64), device=m.device)
    order = torch.arange(64, dtype=torch.int32, device=m.device)
    offset = torch.tensor([0, 64], dtype=torch.int32, device=m.device)
    gram = torch.full((1, 66, 64), 3.0, dtype=torch.float64, device=m.device)
    proj = torch.full((3, 1, 32), 5.0, dtype=torch.float64, device=m.device)
    w = torch.ones((4, 64), dtype=torch.float64, device=m.device)
    keep = [t.clone() for t in (gram, proj)]
    sc = lambda *v: (C.c_double * 6)(*v)
    ok = dict(state=P(state), tab=None, ref=P(ref), first=0, count=3, ref_first=0, order=P(order), offset=P(offset), G=1,
              scale=sc(1, 1, 1, 0, 0, 0), acc=0, gram=P(gram))
    for bad in (dict(state=None), dict(order=None), dict(offset=None), dict(gram=None), dict(scale=None), dict(tab=P(tab)), dict(ref=None),
                dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(count=1 << 31), dict(G=0), dict(G=-3),
                dict(scale=sc(1, 1, 1, 0, 0, -1)), dict(scale=sc(1, float("nan"), 1, 0, 0, 0)), dict(scale=sc(float("inf"), 1, 1, 0, 0, 0)),
                dict(acc=2), dict(acc=-1)):
        a = dict(ok, **bad)
        rc = L.umpcBatchGram(h, a["state"], a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], 0, a["order"], a["offset"],
                             a["G"], a["scale"], a["acc"], a["gram"], s)
        assert rc == -1 and b"umpcBatchGram:" in L.umpcLastError(), bad
    ok = dict(state=P(state), tab=None, ref=P(ref), first=0, count=3, ref_first=0, order=P(order), offset=P(offset), G=1,
              w=P(w), M=3, proj=P(proj))
    for bad in (dict(state=None), dict(order=None), dict(offset=None), dict(proj=None), dict(w=None), dict(tab=P(tab)), dict(ref=None),
                dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(count=1 << 31), dict(G=0), dict(M=0), dict(M=5), dict(M=-1)):
        a = dict(ok, **bad)
        rc = L.umpcBatchProject(h, a["state"], a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], 0, a["order"], a["offset"],
                                a["G"], a["w"], a["M"], a["proj"], s)
        assert rc == -1 and b"umpcBatchProject:" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((gram, proj), keep))
    # count = 0: the projection and the accumulating Gram call change nothing
    assert L.umpcBatchGram(h, P(state), None, P(ref), 0, 0, 0, 0, P(order), P(offset), 1, sc(1, 1, 1, 0, 0, 0), 1, P(gram), s) == 0
    assert L.umpcBatchProject(h, P(state), None, P(ref), 0, 0, 0, 0, P(order), P(offset), 1, P(w), 3, P(proj), s) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip((gram, proj), keep))
    # the same calls with good arguments go through: 64 members on the reference
    assert L.umpcBatchGram(h, P(state), None, P(ref), 0, 3, 0, 0, P(order), P(offset), 1, sc(1, 1, 1, 0, 0, 0), 0, P(gram), s) == 0
    assert L.umpcBatchProject(h, P(state), None, P(ref), 0, 3, 0, 0, P(order), P(offset), 1, P(w), 4, P(proj), s) == 0
    torch.cuda.synchronize()
    assert torch.all(gram[0, :64] == 0) and torch.all(gram[0, 64] == 3) and gram[0, 65, :8].tolist() == [3, 64, 1, 1, 1, 0, 0, 0]
    assert torch.all(proj[..., 0] == 64) and torch.all(proj[..., 1:] == 0)
    # a window outside the history, tensors of the wrong shape, dtype or device: refused by the wrappers before a launch
    m.record_history(2)
    index = (order, offset)
    with pytest.raises(ValueError, match="trajectory_gram"):
        m.trajectory_gram(index, 0, 3)
    with pytest.raises(ValueError, match="ensemble_projection"):
        m.ensemble_projection(index, w, 0, 3)
    for bad in (torch.zeros((1, 66, 64), device=m.device), torch.zeros((1, 66, 64), dtype=torch.float64), torch.zeros((2, 66, 64), dtype=torch.float64, device=m.device)):
        with pytest.raises(ValueError):
            m.trajectory_gram(index, 0, 0, out=bad)
    for bad in (torch.zeros((5, 64), dtype=torch.float64, device=m.device), torch.zeros((2, 64), device=m.device), torch.zeros((2, 64), dtype=torch.float64)):
        with pytest.raises(ValueError):
            m.ensemble_projection(index, bad, 0, 0)
