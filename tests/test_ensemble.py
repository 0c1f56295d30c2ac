"""Ensemble curves on the device: umpcBatchGroupIndex sorts the robots by group, umpcBatchEnsemble turns a step history and
its reference into one row [16] per (step, group) -- reduced over the robots of a group and not over time.
CPU: the numpy mirrors (robobee3d_amd/score.py) by hand on a tiny table, against score_reference on the tables of
test_score, against the reference's own log, their combination over column blocks, exports, refusals, scratch.
GPU: the kernels against the mirrors on the same arrays -- both dtypes, contiguous and permuted groups, after 0 / 1, table /
constant reference, NULL records --, independence of a row from everything but its member list, one end-to-end sweep,
refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_score import (B_, COUNT, FIRST, INF_AT, NAN_AT, REF_FIRST, STEP0, TOL, U, _dev, _golden_tables, _mpc,
                        _no_step_on_the_threshold, _rel, _tables)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_, SIZES = 6, (64, 1, 0, 65, 63, 5)      # a full wavefront, a singleton, an empty group, a second lane trip, partial ones
EXACT = (0, 1, 10, 11, 15)
EXTREME, SUMS, SUM_SQ, SIGNED = (4, 5, 7, 9), (2, 6, 8), 3, (12, 13, 14)
TAULIM = 100.0


def _groups(layout):
    """[200] ids. "contiguous": the groups in order with the ignored ids -1 and G at robots 70 and 199; "permuted": the same
    array permuted, then ids swapped so that robot 7 (the NaN of the tables) is the singleton group's only member."""
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(SIZES)])
    ids = np.append(np.insert(ids, 70, -1), G_).astype(np.int32)
    assert ids.shape == (B_,) and ids[70] == -1 and ids[199] == G_
    if layout == "permuted":
        ids = ids[np.random.default_rng(7).permutation(B_)]
        j = int(np.nonzero(ids == 1)[0][0])
        ids[j], ids[7] = ids[7], ids[j]
        assert ids[7] == 1 and (ids == 1).sum() == 1
    assert [(ids == g).sum() for g in range(G_)] == list(SIZES)
    return ids


def _ref_steps(ref, table):
    """the reference of the COUNT steps of a call as a table [COUNT, 9, B] (the constant reference repeated)"""
    return ref[REF_FIRST:REF_FIRST + COUNT] if table else np.repeat(ref[REF_FIRST][None], COUNT, 0)


def _terms(state, out, ref_steps, after, with_out):
    """per (step, robot), in the mirror's arithmetic: scored, e_p, |d| summed over the three axes"""
    st = np.asarray(state, np.float64)[FIRST + after:FIRST + after + COUNT]
    rs = np.asarray(ref_steps, np.float64)
    with np.errstate(invalid="ignore"):
        d = st[:, 0:3] - rs[:, 0:3]
        ep = (d ** 2).sum(1)
    ok = np.isfinite(st[:, 0:3]).all(1) & np.isfinite(st[:, 9:12]).all(1) & np.isfinite(rs[:, 0:3]).all(1) & np.isfinite(rs[:, 6:9]).all(1)
    if with_out:
        ok &= np.isfinite(np.asarray(out, np.float64)[FIRST:FIRST + COUNT, 1:3]).all(1)
    return ok, ep, np.abs(d).sum(1)


def _input_conditions(ok, ep, order, offset, u):
    """conditions on the INPUTS, on the mirror's arithmetic (if one fires, change the seed, not a bound): row 15 is
    comparable only where the two largest e_p of a row differ by more than 64 u relative -- or are both exactly 0 (a start on the
    reference: differences of equal numbers are 0 in every arithmetic, and a tie goes to the lowest index on both sides)"""
    for g in range(len(offset) - 1):
        mem = order[offset[g]:offset[g + 1]]
        for i in range(ep.shape[0]):
            x = np.sort(ep[i, mem[ok[i, mem]]])
            if len(x) >= 2 and x[-1] > 0:
                assert x[-1] - x[-2] > 64 * u * x[-1], (i, g, x[-2:])


def _check(got, want, sum_abs_d, dtype, margin, tag):
    """the bounds of the issue: rows 0, 1, 10, 11, 15 exact; rows 4, 5 (where finite), 7, 9 (one term: six roundings)
    relative <= 8 u; rows 2, 6, 8 (non-negative terms within 8 u each, summed in fp64) <= 9 u; row 3 (the square of such a
    term) <= 17 u; rows 12..14 |got - want| <= 2 u sum |d| over the row's members (one rounding per difference)"""
    u = U[dtype]
    got = got.to("cpu").numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (tag, got.dtype, got.shape)
    for r in EXACT:
        assert np.array_equal(got[..., r], want[..., r]), (tag, r, np.argwhere(got[..., r] != want[..., r])[:5])
    fin = np.isfinite(want[..., 5])
    assert np.array_equal(got[..., 5][~fin], want[..., 5][~fin]), tag              # +inf where nothing is scored
    margin("%s extreme rows rel" % tag, max(_rel(got[..., r][fin], want[..., r][fin]) for r in EXTREME), 8 * u)
    assert all(np.all(got[..., r][~fin] == 0) for r in (4, 7, 9)), tag
    margin("%s sum rows rel" % tag, max(_rel(got[..., r], want[..., r]) for r in SUMS), 9 * u)
    margin("%s sum e_p^2 rel" % tag, _rel(got[..., SUM_SQ], want[..., SUM_SQ]), 17 * u)
    err = np.max(np.abs(got[..., 12:15] - want[..., 12:15]), axis=-1)
    assert np.all(err[sum_abs_d == 0] == 0), tag
    margin("%s signed sums / sum|d|" % tag, float(np.max(err[sum_abs_d > 0] / sum_abs_d[sum_abs_d > 0], initial=0.0)), 2 * u)


def _group_sum(x, order, offset, ok):
    """[COUNT, G]: x [COUNT, B] summed over the scored members of each group"""
    res = np.zeros((x.shape[0], len(offset) - 1))
    for g in range(len(offset) - 1):
        mem = order[offset[g]:offset[g + 1]]
        res[:, g] = np.where(ok[:, mem], x[:, mem], 0.0).sum(1)
    return res


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_mirror_semantics_by_hand():
    """5 robots, 4 steps: group 0 = robots 0, 1, 2, group 1 empty, group 2 = robot 3, robot 4 ignored; p = (x, 0, 0) against a
    reference at the origin, so e_p = x^2 and d = (x, 0, 0); s = sdes, so e_s = 0"""
    from robobee3d_amd import score as S
    x = np.array([[2.0, -2.0, 1.0, 3.0, 100.0],          # robots 0 and 1 tie at e_p = 4: row 15 names the lower index
                  [0.5, 1.0, 2.0, np.nan, 100.0],        # group 2's only member is not finite: a row with a member and n = 0
                  [0.0, 0.0, 0.0, 1.0, 100.0],           # every e_p = 0: the maximum is 0 and still has an owner
                  [1.0, np.inf, 3.0, 2.0, np.nan]])      # one member of three skipped; robot 4 is ignored whatever it holds
    state = np.zeros((5, 18, 5))
    state[:4, 0] = x
    state[4] = np.nan                                    # slice 4 is read by no step (after = 0)
    state[:, 11] = 1.0
    ref = np.zeros((9, 5))
    ref[8] = 1.0
    group = np.array([0, 0, 0, 2, -1], np.int32)
    order, offset = S.group_index_reference(group, 3)
    assert order.tolist() == [0, 1, 2, 3, 4] and offset.tolist() == [0, 3, 3, 4]
    ens = S.ensemble_reference(state, None, None, ref, 0, 4, 0, 1.5, False, 3.5, order, offset)
    assert ens.shape == (4, 3, 16) and S.ENS_ROWS == 16 and len(S.ENS_ROW_NAMES) == 16
    inf = np.inf
    #            n  skip sum  sum2 max  min  ses mes  tau mtau over bad  dx   dy dz arg
    want = {(0, 0): [3, 0, 9.0, 33.0, 4.0, 1.0, 0, 0, 0, 0, 2, 0, 1.0, 0, 0, 0],
            (1, 0): [3, 0, 5.25, 17.0625, 4.0, 0.25, 0, 0, 0, 0, 1, 0, 3.5, 0, 0, 2],
            (2, 0): [3, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0],
            (3, 0): [2, 1, 10.0, 82.0, 9.0, 1.0, 0, 0, 0, 0, 1, 0, 4.0, 0, 0, 2],
            (0, 2): [1, 0, 9.0, 81.0, 9.0, 9.0, 0, 0, 0, 0, 1, 0, 3.0, 0, 0, 3],
            (1, 2): [0, 1, 0.0, 0.0, 0.0, inf, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, -1],
            (2, 2): [1, 0, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 3],
            (3, 2): [1, 0, 4.0, 16.0, 4.0, 4.0, 0, 0, 0, 0, 1, 0, 2.0, 0, 0, 3]}
    for i in range(4):
        want[(i, 1)] = [0, 0, 0, 0, 0, inf, 0, 0, 0, 0, 0, 0, 0, 0, 0, -1]      # the empty group
    for (i, g), row in want.items():
        assert ens[i, g].tolist() == [float(v) for v in row], (i, g, ens[i, g])
    # out and status: moments (3, 4) clipped at taulim = 3.5 -> 9 + 12.25; a non-finite moment skips the member
    out = np.zeros((4, 9, 5))
    out[:, 1], out[:, 2] = 3.0, 4.0
    out[:, 0] = np.nan                                   # the thrust row is not read
    out[0, 2, 1] = np.inf
    status = np.ones((4, 5), np.int32)
    status[0, 0], status[0, 1], status[2, 3] = 2, -2, 2
    full = S.ensemble_reference(state, out, status, ref, 0, 4, 0, 1.5, False, 3.5, order, offset)
    assert full[0, 0].tolist() == [2, 1, 5.0, 17.0, 4.0, 1.0, 0, 0, 42.5, 21.25, 1, 1, 3.0, 0, 0, 0]   # robot 1 skipped: its status too
    assert full[2, 2, S.E_NOT_SOLVED] == 1 and full[2, 2, S.E_SUM_TAU2] == 21.25 and full[1, 2, S.E_SUM_TAU2] == 0
    rest = [r for r in range(16) if r not in (S.E_SUM_TAU2, S.E_MAX_TAU2, S.E_NOT_SOLVED)]
    assert np.array_equal(full[1:, :, rest], ens[1:, :, rest])
    # after = 1 is after = 0 on the table moved by one slice; first / ref_first move the window; a table of references
    tab = np.repeat(ref[None], 6, 0)
    a1 = S.ensemble_reference(state, None, None, tab, 1, 2, 3, 1.5, True, 3.5, order, offset)
    assert np.array_equal(a1, ens[2:4])
    assert S.ensemble_reference(state, None, None, ref, 2, 0, 0, 1.5, False, 3.5, order, offset).shape == (0, 3, 16)
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(tol_p=-1.0), dict(tol_p=np.nan), dict(tol_p=np.inf)):
        kw = dict(first=0, count=4, ref_first=0, tol_p=1.5, after=False, taulim=3.5, order=order, offset=offset)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.ensemble_reference(state, None, None, ref, **kw)


def test_group_index_reference_is_the_stable_sort():
    from robobee3d_amd import score as S
    for ids, G in ((_groups("contiguous"), G_), (_groups("permuted"), G_), (np.zeros(9, np.int32), 1),
                   (np.random.default_rng(3).integers(-3, 12, 500).astype(np.int32), 7)):
        order, offset = S.group_index_reference(ids, G)
        assert order.dtype == np.int32 and offset.dtype == np.int32 and offset.shape == (G + 1,) and offset[0] == 0
        assert np.array_equal(order, np.argsort(np.where((ids >= 0) & (ids < G), ids, G), kind="stable"))
        assert np.array_equal(np.sort(order), np.arange(len(ids)))
        for g in range(G):
            assert np.array_equal(order[offset[g]:offset[g + 1]], np.nonzero(ids == g)[0])
        assert np.array_equal(order[offset[G]:], np.nonzero((ids < 0) | (ids >= G))[0])


def test_combination_over_column_blocks():
    """blocks [0, 64) + [64, 200) (whole groups) and [0, 100) + [100, 137) + [137, 200) (cut inside groups 3 and 4) of the
    contiguous layout combine to the undivided mirror; torch tensors combine like arrays"""
    import torch
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.float64)
    ids = _groups("contiguous")
    order, offset = S.group_index_reference(ids, G_)
    whole = S.ensemble_reference(state, out, status, ref, FIRST, COUNT, REF_FIRST, TOL, True, TAULIM, order, offset)
    for cuts in ((0, 64, 200), (0, 100, 137, 200)):
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            o, f = S.group_index_reference(ids[lo:hi], G_)
            parts.append(S.ensemble_reference(state[..., lo:hi], out[..., lo:hi], status[..., lo:hi], ref[..., lo:hi], FIRST, COUNT,
                                              REF_FIRST, TOL, True, TAULIM, o, f))
        keep = [p.copy() for p in parts]
        tot = S.combine_ensembles(parts, cuts[:-1])
        for r in (0, 1, 4, 5, 7, 9, 10, 11, 15):
            assert np.array_equal(tot[..., r], whole[..., r]), (cuts, r)
        for r in (2, 3, 6, 8) + SIGNED:
            assert np.allclose(tot[..., r], whole[..., r], rtol=1e-13, atol=0), (cuts, r)
        assert all(np.array_equal(p, k) for p, k in zip(parts, keep))             # the parts are not modified
        tt = S.combine_ensembles([torch.as_tensor(p) for p in parts], cuts[:-1])
        assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), tot)
    assert np.array_equal(S.combine_ensembles([whole]), whole)
    with pytest.raises(ValueError):
        S.combine_ensembles([])


def test_mirror_against_score_reference():
    """the same tables reduced the other way: what an ensemble sums over the steps is what the scores sum over the members"""
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.float64)
    for layout in ("contiguous", "permuted"):
        order, offset = S.group_index_reference(_groups(layout), G_)
        for after in (0, 1):
            sc = S.score_reference(state, out, status, ref, FIRST, COUNT, REF_FIRST, STEP0, TOL, after, TAULIM)
            ens = S.ensemble_reference(state, out, status, ref, FIRST, COUNT, REF_FIRST, TOL, after, TAULIM, order, offset)
            for g in range(G_):
                mem = order[offset[g]:offset[g + 1]]
                assert ens[:, g, S.E_N].sum() == sc[S.STEPS, mem].sum()
                assert ens[:, g, S.E_SKIPPED].sum() == sc[S.SKIPPED, mem].sum()
                assert ens[:, g, S.E_NOT_SOLVED].sum() == sc[S.NOT_SOLVED, mem].sum()
                assert ens[:, g, S.E_MAX_EP].max() == sc[S.MAX_EP, mem].max(initial=0.0)
                assert np.isclose(ens[:, g, S.E_SUM_EP].sum(), sc[S.SUM_EP, mem].sum(), rtol=1e-12, atol=0)
            assert ens[..., S.E_SKIPPED].sum() == 2 and (ens[..., S.E_N] + ens[..., S.E_SKIPPED] == 0).sum() == COUNT


def test_mirror_on_the_references_own_log():
    """the kick run of tests/golden/impulse_log.npz (the tables of test_score._golden_tables) replicated 8 times in one group:
    every row is 8 identical members"""
    from robobee3d_amd import score as S
    g, state, out, status, ref = _golden_tables()
    n = len(g["t"])
    rep = lambda a: np.repeat(a[..., :1], 8, -1)
    order, offset = S.group_index_reference(np.zeros(8, np.int32), 1)
    ens = S.ensemble_reference(rep(state), rep(out), rep(status), rep(ref), 0, n, 0, 10.0, True, 100.0, order, offset)
    ep = ((g["kick_y"][:, 0:3] - g["kick_pdes"]) ** 2).sum(1)
    assert ens.shape == (n, 1, 16) and np.all(ens[:, 0, S.E_N] == 8) and np.all(ens[:, 0, S.E_SKIPPED] == 0)
    assert np.array_equal(ens[:, 0, S.E_SUM_EP], 8 * ep)
    assert np.array_equal(ens[:, 0, S.E_MAX_EP], ens[:, 0, S.E_MIN_EP]) and np.array_equal(ens[:, 0, S.E_MAX_EP], ep)
    assert np.array_equal(ens[:, 0, S.E_SUM_EP2], 8 * (ep * ep))
    assert np.array_equal(ens[:, 0, S.E_OVER], 8.0 * (ep > 100.0)) and np.all(ens[:, 0, S.E_ARGMAX_EP] == 0)
    assert np.array_equal(ens[:, 0, S.E_NOT_SOLVED], 8.0 * (g["kick_status"] != 1))


def test_ensemble_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    for decl in ("#define UMPC_ENS_ROWS 16",
                 "int umpcBatchGroupIndex(umpc_batch_t *h, const int32_t *group, int G, int32_t *order, int32_t *offset, void *stream);",
                 "int umpcBatchEnsemble(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist, "
                 "const void *ref_tab, const void *ref, long long first, long long count, long long ref_first, "
                 "double tol_p, int after, const int32_t *order, const int32_t *offset, int G, double *ens, void *stream);"):
        assert decl in flat, decl
    assert flat.index("int umpcBatchScoreGroups(") < flat.index("#define UMPC_ENS_ROWS") < flat.index("int umpcBatchSetStepKernel")
    assert _lib.ENS_ROWS == S.ENS_ROWS == 16
    L = _lib.lib()
    for sym in ("umpcBatchGroupIndex", "umpcBatchEnsemble"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchGroupIndex.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.umpcBatchEnsemble.argtypes == [C.c_void_p] * 6 + [C.c_longlong] * 3 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p,
                                                                                  C.c_int, C.c_void_p, C.c_void_p]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchGroupIndex(None, None, 1, None, None, None) == -1 and b"umpcBatchGroupIndex" in L.umpcLastError()
    assert L.umpcBatchEnsemble(None, None, None, None, None, None, 0, 1, 0, 1.0, 0, None, None, 1, None, None) == -1
    assert b"umpcBatchEnsemble" in L.umpcLastError()


def test_ensemble_kernels_use_no_scratch():
    """the resource remarks of the build: the ensemble kernel (8 forms by which tables there are x 2 dtypes) and the
    group-index kernel spill nothing"""
    import json
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    for pat in ("umpc_ensemble_kernel", "umpc_group_index_kernel"):
        hits = [k for k in res if pat in k]
        assert len(hits) >= 1, (pat, sorted(res))
        for k in hits:
            assert res[k]["ScratchSize"] == 0, (k, res[k])
    # the build itself refuses a frame: the two entries of resource_limits.json, checked by _validate_resources
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    for pat in ("umpc_ensemble_kernel", "umpc_group_index_kernel"):
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0}
    with pytest.raises(RuntimeError, match="umpc_ensemble_kernel"):
        _lib._validate_resources(dict(res, **{"a_form_of_umpc_ensemble_kernel_with_a_frame": {"ScratchSize": 8}}))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _index(m, ids, G):
    """umpcBatchGroupIndex through the C ABI on a device array of ids"""
    import torch
    from robobee3d_amd.batch import _ptr
    d = _dev(m, np.asarray(ids, np.int32))
    order = torch.full((m.B,), -7, dtype=torch.int32, device=m.device)
    offset = torch.full((G + 1,), -7, dtype=torch.int32, device=m.device)
    assert m.L.umpcBatchGroupIndex(m.h, _ptr(d), G, _ptr(order), _ptr(offset), m._stream()) == 0, m.L.umpcLastError()
    return order, offset


def _ensemble(m, state, out, status, reftab, ref, first, count, ref_first, tol, after, index, ens=None):
    """umpcBatchEnsemble on device tensors through the C ABI (BatchUprightMPC.ensemble works on the handle's own history);
    a fresh `ens` is filled with NaN first: the call has to overwrite every row"""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    if ens is None:
        ens = torch.full((count, G, 16), float("nan"), dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchEnsemble(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(reftab), _ptr(ref), first, count, ref_first,
                               float(tol), int(after), _ptr(order), _ptr(offset), G, _ptr(ens), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return ens


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_group_index_against_the_mirror(dtype):
    import torch
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    for ids, G in ((_groups("contiguous"), G_), (_groups("permuted"), G_), (np.zeros(B_, np.int32), 1)):
        want = S.group_index_reference(ids, G)
        got = _index(m, ids, G)
        for a, b in zip(got, want):
            assert a.dtype == torch.int32 and torch.equal(a.cpu(), torch.as_tensor(b)), (G, a, b)
        o, f = m.group_index(ids, G)
        assert torch.equal(o, got[0]) and torch.equal(f, got[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ensemble_kernel_against_the_mirror(dtype, margin):
    """both layouts x after 0 / 1 x table / constant reference x all records / no out / no status on one set of tables"""
    import torch
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    taulim = float(m.prm.taulim)
    d = [_dev(m, a) for a in (state, out, status, ref)]
    cref = np.ascontiguousarray(ref[REF_FIRST])
    dcref = _dev(m, cref)
    for layout in ("contiguous", "permuted"):
        ids = _groups(layout)
        order, offset = S.group_index_reference(ids, G_)
        index = _index(m, ids, G_)
        inside = lambda b: int(0 <= ids[b] < G_)
        for after in (0, 1):
            for table in (True, False):
                rsteps = _ref_steps(ref, table)
                _no_step_on_the_threshold(state, rsteps, after, TOL)
                for with_out, with_status in ((True, True), (False, True), (True, False)):
                    tag = "%s after%d %s%s%s" % (layout[:4], after, "tab" if table else "const", "" if with_out else " -out",
                                                 "" if with_status else " -status")
                    ok, ep, absd = _terms(state, out, rsteps, after, with_out)
                    _input_conditions(ok, ep, order, offset, U[dtype])
                    got = _ensemble(m, d[0], d[1] if with_out else None, d[2] if with_status else None, d[3] if table else None,
                                    None if table else dcref, FIRST, COUNT, REF_FIRST if table else 0, TOL, after, index)
                    want = S.ensemble_reference(state, out if with_out else None, status if with_status else None,
                                                ref if table else cref, FIRST, COUNT, REF_FIRST if table else 0, TOL, after,
                                                taulim, order, offset)
                    _check(got, want, _group_sum(absd, order, offset, ok), dtype, margin, tag)
                    # the planted values did what they are there for: 2 skipped member-steps, 37 empty rows, and in the
                    # permuted layout one row that has a member and nobody scored
                    assert want[..., S.E_SKIPPED].sum() == inside(NAN_AT[2]) + (inside(INF_AT[2]) if with_out else 0)
                    assert inside(NAN_AT[2]) and inside(INF_AT[2])
                    assert (want[..., S.E_N] + want[..., S.E_SKIPPED] == 0).sum() == COUNT
                    if layout == "permuted":
                        assert want[NAN_AT[0] - after - FIRST, 1, :2].tolist() == [0, 1]
                    if not with_out:
                        assert torch.all(got[..., S.E_SUM_TAU2] == 0) and torch.all(got[..., S.E_MAX_TAU2] == 0)
                    if not with_status:
                        assert torch.all(got[..., S.E_NOT_SOLVED] == 0)
                    else:
                        assert want[..., S.E_NOT_SOLVED].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_row_depends_on_its_member_list_alone(dtype):
    """all torch.equal: run to run, the step range cut into two calls, count = 0, another G and other groups around,
    a column block on a handle of its own"""
    import torch
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    d = [_dev(m, a) for a in (state, out, status, ref)]
    ids = _groups("contiguous")
    index = _index(m, ids, G_)
    one = _ensemble(m, *d, None, FIRST, COUNT, REF_FIRST, TOL, 1, index)
    assert not torch.isnan(one).any()
    assert torch.equal(one, _ensemble(m, *d, None, FIRST, COUNT, REF_FIRST, TOL, 1, index))
    # steps 3..22 then 23..39 into the two slices of one table
    two = torch.full_like(one, float("nan"))
    _ensemble(m, *d, None, FIRST, 20, REF_FIRST, TOL, 1, index, ens=two[:20])
    _ensemble(m, *d, None, FIRST + 20, 17, REF_FIRST + 20, TOL, 1, index, ens=two[20:])
    assert torch.equal(one, two)
    # count = 0 writes nothing
    keep = two.clone()
    _ensemble(m, *d, None, FIRST, 0, REF_FIRST, TOL, 1, index, ens=two)
    torch.cuda.synchronize()
    assert torch.equal(two, keep)
    # only group 3's robots labelled, G = 4
    only3 = _ensemble(m, *d, None, FIRST, COUNT, REF_FIRST, TOL, 1, _index(m, np.where(ids == 3, 3, -1), 4))
    assert tuple(only3.shape) == (COUNT, 4, 16) and torch.equal(only3[:, 3], one[:, 3])
    assert torch.all(only3[:, :3, 0] == 0) and torch.all(only3[:, :3, 15] == -1)
    # columns [64, 200) on a B = 136 handle: groups 1, 3, 4, 5 lie wholly inside (0 lies outside, 2 is empty)
    mb = _mpc(B_ - 64, dtype)
    blk = [_dev(mb, np.ascontiguousarray(a[..., 64:])) for a in (state, out, status, ref)]
    part = _ensemble(mb, *blk, None, FIRST, COUNT, REF_FIRST, TOL, 1, _index(mb, ids[64:], G_))
    shifted = part.clone()
    shifted[..., 15] = torch.where(part[..., 15] >= 0, part[..., 15] + 64, part[..., 15])
    assert (ids[:64] == 0).all() and not (ids[64:] == 0).any()
    for g in (1, 2, 3, 4, 5):
        assert torch.equal(shifted[:, g], one[:, g]), g
    assert torch.all(part[:, 0, 0] == 0)


@pytest.mark.gpu
def test_end_to_end_sweep_gives_the_curves_of_its_cells(margin):
    """the sweep of test_score's end-to-end test (B = 128 as 8 cells x 16 draws, 12 steps, every second robot pushed after
    step 4, fp32): m.ensemble(m.group_index(cell, 8)) against the mirror on the downloaded tables; the push shows in the
    count of draws outside the tube; the step sums are the scores' sums"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, tol, push = 128, 12, 10.0, 4
    m = _mpc(B, "float32")
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    amp = np.repeat(np.linspace(20, 80, 8), 16)
    tab = m.task_table(K, "helix", trajAmp=amp, trajFreq=np.tile(np.linspace(0.5, 2, 16), 8), dz=0.05)
    m.set_reference_trajectory(tab)
    m.record_history(K, status=True)
    m.set_impulses(m.impulse_table(K, [(push, slice(0, B, 2), (0, 2, 0, 0, 0, 0))]))
    m.rollout(K)
    cell = np.repeat(np.arange(8, dtype=np.int32), 16)
    index = m.group_index(cell, 8)
    order, offset = S.group_index_reference(cell, 8)
    assert torch.equal(index[0].cpu(), torch.as_tensor(order)) and torch.equal(index[1].cpu(), torch.as_tensor(offset))
    h = m.history()
    tabs = [h["state"].cpu().numpy(), h["out"].cpu().numpy(), h["status"].cpu().numpy(), tab.cpu().numpy()]
    u = U["float32"]
    for after in (False, True):
        want = S.ensemble_reference(*tabs, 0, K, 0, tol, after, float(m.prm.taulim), order, offset)
        s64 = tabs[0][int(after):K + int(after)].astype(np.float64)
        d = s64[:, 0:3] - tabs[3][:, 0:3]
        ep = (d ** 2).sum(1)
        assert np.abs(ep - tol * tol).min() > 1e-5 * tol * tol                       # conditions on the inputs, as above
        ok = np.ones(ep.shape, bool)
        _input_conditions(ok, ep, order, offset, u)
        assert np.all(want[..., S.E_N] == 16) and np.all(want[..., S.E_SKIPPED] == 0)
        got = m.ensemble(index, tol=tol, after=after)
        assert got.dtype == torch.float64 and tuple(got.shape) == (K, 8, 16)
        _check(got, want, _group_sum(np.abs(d).sum(1), order, offset, ok), "float32", margin, "end to end after%d" % after)
        # the step sum of row 0 is score() row 0 summed per cell
        sc = m.score(tol=tol, after=after)
        assert torch.equal(got[..., S.E_N].sum(0), sc[S.STEPS].to(torch.float64).reshape(8, 16).sum(1))
    # after = True: row i is the state step i produced. The kick is added to the VELOCITY after the last substep of step
    # `push`, so the positions of rows push - 1 and push are those before the push acts and every later row is after it.
    # Every cell holds 8 pushed draws: the draws outside the 10 mm tube in the two rows before are no more than in the last
    # row after, and there are some there
    over = got[..., S.E_OVER].cpu().numpy()
    print("outside the tube per cell and step (rows = steps, the push after step %d):\n" % push, over)
    assert np.all(over[push - 1] <= over[K - 1]) and np.all(over[push] <= over[K - 1]) and np.all(over[K - 1] > 0)
    # chunks into one table through `out`, and the checks of the wrapper
    both = torch.empty_like(got)
    m.ensemble(index, 0, 5, tol=tol, after=True, out=both[:5])
    m.ensemble(index, 5, tol=tol, after=True, out=both[5:])
    assert torch.equal(both, got)
    with pytest.raises(ValueError):
        m.ensemble(index, 0, K + 1)
    with pytest.raises(ValueError):
        m.ensemble((index[0][:-1], index[1]))
    with pytest.raises(ValueError):
        m.ensemble(index, out=torch.empty((K, 8, 12), dtype=torch.float64, device=m.device))
    m2 = _mpc(B, "float32")
    m2.set_state(st, ref)
    m2.set_task("helix")
    m2.record_history(2)
    m2.rollout(2)
    with pytest.raises(RuntimeError, match="ensemble: .*task_table"):
        m2.ensemble(m2.group_index(cell, 8))
    e2 = m2.ensemble(m2.group_index(cell, 8), ref_table=m2.task_table(2, t_ms=0.0))
    assert tuple(e2.shape) == (2, 8, 16) and torch.all(e2[..., S.E_N] == 16) and torch.all(e2[..., S.E_NOT_SOLVED] == 0)


@pytest.mark.gpu
def test_ensemble_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr as P
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((4, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((3, 9, 64), device=m.device)
    group = torch.zeros(64, dtype=torch.int32, device=m.device)
    order = torch.arange(64, dtype=torch.int32, device=m.device)
    offset = torch.tensor([0, 64], dtype=torch.int32, device=m.device)
    ens = torch.full((3, 1, 16), 3.0, dtype=torch.float64, device=m.device)
    keep, keep_o, keep_f = ens.clone(), order.clone(), offset.clone()
    ok = dict(state=P(state), tab=None, ref=P(ref), first=0, count=3, ref_first=0, tol=1.0, order=P(order), offset=P(offset),
              G=1, ens=P(ens))
    for bad in (dict(state=None), dict(order=None), dict(offset=None), dict(ens=None), dict(tab=P(tab)), dict(ref=None),
                dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(count=1 << 31), dict(tol=-1.0), dict(tol=float("nan")),
                dict(tol=float("inf")), dict(G=0), dict(G=-3)):
        a = dict(ok, **bad)
        rc = L.umpcBatchEnsemble(h, a["state"], None, None, a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], a["tol"], 0,
                                 a["order"], a["offset"], a["G"], a["ens"], s)
        assert rc == -1 and b"umpcBatchEnsemble" in L.umpcLastError(), bad
    for bad in (dict(group=None), dict(order=None), dict(offset=None), dict(G=0)):
        a = dict(dict(group=P(group), order=P(order), offset=P(offset), G=1), **bad)
        assert L.umpcBatchGroupIndex(h, a["group"], a["G"], a["order"], a["offset"], s) == -1, bad
        assert b"umpcBatchGroupIndex" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert torch.equal(ens, keep) and torch.equal(order, keep_o) and torch.equal(offset, keep_f)
    # the same calls with good arguments go through; count = 0 changes nothing
    a = ok
    assert L.umpcBatchEnsemble(h, a["state"], None, None, None, a["ref"], 0, 0, 0, 1.0, 0, a["order"], a["offset"], 1, a["ens"], s) == 0
    torch.cuda.synchronize()
    assert torch.equal(ens, keep)
    assert L.umpcBatchGroupIndex(h, P(group), 1, P(order), P(offset), s) == 0
    assert L.umpcBatchEnsemble(h, a["state"], None, None, None, a["ref"], 0, 3, 0, 1.0, 0, a["order"], a["offset"], 1, a["ens"], s) == 0
    torch.cuda.synchronize()
    assert torch.equal(order, keep_o) and torch.equal(offset, keep_f)
    assert torch.all(ens[..., 0] == 64) and torch.all(ens[..., 2] == 0) and torch.all(ens[..., 15] == 0)
