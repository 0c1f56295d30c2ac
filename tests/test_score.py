"""Scoring of recorded rollouts on the device: umpcBatchScore turns a step history and its reference into a score [12, B] per
robot in one pass, umpcBatchScoreGroups turns the scores into one row [8] per group of robots (a grid cell of a sweep).
CPU: the numpy mirror (robobee3d_amd/score.py) against the reference's own log and logMetric, its semantics on small synthetic
tables, the group reduction and its combination over blocks, exports and refusals.
GPU: the kernels against the mirror on the same arrays -- both dtypes, both alignments, table / constant reference, NULL
records, chunked calls, column blocks, the reference's log, the groups, one end-to-end run, refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
EXACT_ROWS, MAX_ROWS, SUM_ROWS = (0, 8, 9, 10, 11), (2, 3, 5), (1, 4, 6, 7)
ORDER_FREE_ROWS = (0, 2, 3, 5, 8, 9, 10, 11)
# the reference's own numbers for tests/golden/impulse_log.npz (recorded from the reference; computed from the fixture, not by
# the code under test): logMetric err / eff, mean and max tracking error with the step of the max, steps not solved
GOLD = {"kick": (173.61782059975266, 2727.073978517893, 188.13614464484516, 880.3254981783109, 199, 100),
        "plain": (5.488304315210562, 66.77819036132387, 29.334686687494024, 83.95312008977392, 193, 62)}


def _golden_tables():
    """impulse_log.npz as a two-robot history (robot 0 = kick, 1 = plain) in the reference log's convention: log['y'][ti] is
    the state AFTER the plant of iteration ti = state slice ti + 1 (after=True); slice 0 is never read and holds NaN."""
    g = golden("impulse_log.npz")
    n = len(g["t"])
    state = np.full((n + 1, 18, 2), np.nan)
    out = np.zeros((n, 9, 2))
    ref = np.zeros((n, 9, 2))
    status = np.zeros((n, 2), np.int32)
    for b, name in enumerate(("kick", "plain")):
        y = g[name + "_y"]
        state[1:, :, b] = 0.0
        state[1:, 0:3, b] = y[:, 0:3]
        state[1:, 9:12, b] = y[:, 3:6]
        out[:, 0:3, b] = g[name + "_u"]
        ref[:, 0:3, b] = g[name + "_pdes"]
        ref[:, 8, b] = 1.0
        status[:, b] = g[name + "_status"]
    return g, state, out, status, ref


def _log_metric(g, name):
    """logMetric of the reference restated (template/uprightmpc2.py:161-175): mean |p|^2 and mean |tau|^2 over the log"""
    y, u = g[name + "_y"], g[name + "_u"]
    return (y[:, 0:3] ** 2).sum() / len(y), (u[:, 1:3] ** 2).sum() / len(y)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_mirror_on_the_references_own_log():
    from robobee3d_amd import score as S
    g, state, out, status, ref = _golden_tables()
    n = len(g["t"])
    for name in ("kick", "plain"):                     # `u` is logged after the clip: taulim = 100 leaves it alone
        assert np.abs(g[name + "_u"][:, 1:3]).max() <= 100.0
    sc = S.score_reference(state, out, status, ref, 0, n, 0, 0, 10.0, True, 100.0)
    assert sc.shape == (12, 2) and np.all(sc[S.STEPS] == n) and np.all(sc[S.SKIPPED] == 0)
    for b, name in enumerate(("kick", "plain")):
        err, eff, mean_ep, max_ep, at, bad = GOLD[name]
        lm = _log_metric(g, name)
        assert np.isclose(lm[0], err, rtol=1e-12, atol=0) and np.isclose(lm[1], eff, rtol=1e-12, atol=0)
        assert np.isclose(sc[S.SUM_P2, b] / sc[S.STEPS, b], err, rtol=1e-12, atol=0)
        assert np.isclose(sc[S.SUM_TAU2, b] / sc[S.STEPS, b], eff, rtol=1e-12, atol=0)
        assert np.isclose(sc[S.SUM_EP, b] / sc[S.STEPS, b], mean_ep, rtol=1e-12, atol=0)
        ep = ((g[name + "_y"][:, 0:3] - g[name + "_pdes"]) ** 2).sum(1)
        assert np.isclose(sc[S.MAX_EP, b], max_ep, rtol=1e-12, atol=0) and int(ep.argmax()) == at
        assert sc[S.LAST_EP, b] == ep[-1]
        assert sc[S.NOT_SOLVED, b] == bad
        over = np.nonzero(ep > 100.0)[0]
        assert (len(over) > 0) == (name == "kick")       # the plain run stays inside 10 mm (max e_p 83.95): -1, -1
        assert sc[S.FIRST_OVER, b] == (over[0] if len(over) else -1) and sc[S.LAST_OVER, b] == (over[-1] if len(over) else -1)


def _small_tables(seed=5, B=5, n=11):
    rng = np.random.default_rng(seed)
    state = rng.normal(size=(n + 1, 18, B))
    out = rng.normal(scale=80.0, size=(n, 9, B))
    status = rng.choice(np.array([1, 2, -2], np.int32), size=(n, B))
    ref = state[:n, 0:9].copy() + rng.normal(size=(n, 9, B))
    return state, out, status, ref


def test_mirror_semantics_on_small_tables():
    from robobee3d_amd import score as S
    state, out, status, ref = _small_tables()
    n, B = 11, 5
    full = S.score_reference(state, out, status, ref, 0, n, 0, 0, 1.5, False, 100.0)
    assert np.all(full[S.STEPS] == n) and np.all(full[S.SKIPPED] == 0)
    ep = ((state[:n, 0:3] - ref[:, 0:3]) ** 2).sum(1)                               # [n, B]
    assert np.array_equal(full[S.MAX_EP], ep.max(0)) and np.array_equal(full[S.LAST_EP], ep[-1])
    assert np.array_equal(full[S.NOT_SOLVED], (status != 1).sum(0))
    tau = np.clip(out[:, 1:3], -100, 100)
    assert np.abs(out[:, 1:3]).max() > 100 and np.allclose(full[S.SUM_TAU2], (tau ** 2).sum((0, 1)), rtol=1e-13)
    # after = 1 is after = 0 on the table moved by one state slice, and differs from it
    a1 = S.score_reference(state, out, status, ref, 0, n, 0, 0, 1.5, True, 100.0)
    assert np.array_equal(a1, S.score_reference(state[1:], out, status, ref, 0, n, 0, 0, 1.5, False, 100.0))
    assert not np.array_equal(a1[S.SUM_EP], full[S.SUM_EP])
    # two chunked calls = one call, exactly (the mirror is sequential); first / ref_first / step0 move together
    part = S.score_reference(state, out, status, ref, 0, 4, 0, 0, 1.5, False, 100.0)
    part = S.score_reference(state, out, status, ref, 4, 7, 4, 4, 1.5, False, 100.0, score=part)
    assert np.array_equal(part, full)
    # a constant reference [9, B]
    cst = S.score_reference(state, out, status, ref[3], 0, n, 0, 0, 1.5, False, 100.0)
    assert np.array_equal(cst, S.score_reference(state, out, status, np.repeat(ref[3:4], n, 0), 0, n, 0, 0, 1.5, False, 100.0))
    # a NaN / an Inf in one robot's step: row 11 counts it, no other row sees it
    bad_s, bad_o = state.copy(), out.copy()
    bad_s[6, 10, 2] = np.nan
    bad_o[2, 2, 4] = np.inf
    got = S.score_reference(bad_s, bad_o, status, ref, 0, n, 0, 0, 1.5, False, 100.0)
    assert got[S.SKIPPED].tolist() == [0, 0, 1, 0, 1] and got[S.STEPS].tolist() == [n, n, n - 1, n, n - 1]
    assert np.all(np.isfinite(got))
    keep = np.ones((n, B), bool)
    keep[6, 2] = keep[2, 4] = False
    assert np.allclose(got[S.SUM_EP], (ep * keep).sum(0), rtol=1e-13) and np.array_equal(got[S.MAX_EP], (ep * keep).max(0))
    assert np.array_equal(got[:, [0, 1, 3]], full[:, [0, 1, 3]])
    # an unread value may be anything: out row 0, state rows 3..8 and 12..17, reference rows 3..5
    junk_s, junk_o, junk_r = state.copy(), out.copy(), ref.copy()
    junk_s[:, 3:9] = np.nan; junk_s[:, 12:18] = np.inf; junk_o[:, 0] = np.nan; junk_o[:, 3:] = np.nan; junk_r[:, 3:6] = np.nan
    assert np.array_equal(S.score_reference(junk_s, junk_o, status, junk_r, 0, n, 0, 0, 1.5, False, 100.0), full)
    # NULL out / NULL status: rows 6 / 8 stay at the identity, and a bad `out` value no longer skips a step
    no = S.score_reference(state, None, None, ref, 0, n, 0, 0, 1.5, False, 100.0)
    assert np.all(no[S.SUM_TAU2] == 0) and np.all(no[S.NOT_SOLVED] == 0)
    rest = [r for r in range(12) if r not in (S.SUM_TAU2, S.NOT_SOLVED)]
    assert np.array_equal(no[rest], full[rest])
    assert np.all(S.score_reference(state, None, status, ref, 0, n, 0, 0, 1.5, False, 100.0)[S.SKIPPED] == 0)
    keep6 = S.score_reference(state, None, None, ref, 0, n, 0, 0, 1.5, False, 100.0, score=full)
    assert np.array_equal(keep6[S.SUM_TAU2], full[S.SUM_TAU2]) and np.array_equal(keep6[S.NOT_SOLVED], full[S.NOT_SOLVED])
    # rows 9 and 10 carry the caller's step numbers; -1 where the threshold is never passed
    over = ep > 1.5 ** 2
    assert over.any() and not over.all()
    s0 = S.score_reference(state, out, status, ref, 0, n, 0, 1000, 1.5, False, 100.0)
    for b in range(B):
        k = np.nonzero(over[:, b])[0]
        assert s0[S.FIRST_OVER, b] == (1000 + k[0] if len(k) else -1) and s0[S.LAST_OVER, b] == (1000 + k[-1] if len(k) else -1)
    never = S.score_reference(state, out, status, ref, 0, n, 0, 1000, 1e3, False, 100.0)
    assert np.all(never[S.FIRST_OVER] == -1) and np.all(never[S.LAST_OVER] == -1)
    assert np.array_equal(S.score_reference(state, out, status, ref, 2, 0, 0, 0, 1.5, False, 100.0), S.score_identity(B))
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(tol_p=-1.0), dict(tol_p=np.nan), dict(tol_p=np.inf)):
        kw = dict(first=0, count=n, ref_first=0, step0=0, tol_p=1.5, after=False, taulim=100.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.score_reference(state, out, status, ref, **kw)


def _random_score(B, seed):
    """a score as the kernel leaves one: integer counts, -1 markers, some robots with no step scored"""
    rng = np.random.default_rng(seed)
    sc = np.abs(rng.normal(size=(12, B))) * 10
    sc[0] = rng.integers(0, 40, B)
    sc[0, ::9] = 0
    sc[8] = rng.integers(0, 5, B)
    sc[9] = np.where(rng.random(B) < 0.4, -1, rng.integers(0, 30, B))
    sc[10] = np.where(sc[9] < 0, -1, sc[9] + rng.integers(0, 9, B))
    sc[11] = rng.integers(0, 3, B)
    return sc


def test_group_reference_and_combination_over_blocks():
    from robobee3d_amd import score as S
    B, G = 200, 7
    sc = _random_score(B, 11)
    group = np.random.default_rng(12).integers(-1, G + 1, B).astype(np.int32)          # ids in [-1, 7]: -1 and 7 are outside
    assert (group == -1).any() and (group == G).any()
    gs = S.group_reference(sc, group, G)
    assert gs.shape == (G, 8)
    inside = (group >= 0) & (group < G)
    assert gs[:, S.G_ROBOTS].sum() == inside.sum() and gs[:, S.G_SCORED].sum() == (inside & (sc[0] > 0)).sum()
    for g in range(G):
        sel = (group == g) & (sc[0] > 0)
        assert np.isclose(gs[g, S.G_SUM_MEAN_EP], (sc[1, sel] / sc[0, sel]).sum(), rtol=1e-13)
        assert np.isclose(gs[g, S.G_SUM_MEAN_TAU2], (sc[6, sel] / sc[0, sel]).sum(), rtol=1e-13)
        assert np.isclose(gs[g, S.G_SUM_MEAN_P2], (sc[7, sel] / sc[0, sel]).sum(), rtol=1e-13)
        assert gs[g, S.G_MAX_EP] == sc[2, sel].max()
        assert gs[g, S.G_LEFT] == (sc[9, group == g] >= 0).sum() and gs[g, S.G_NOT_SOLVED] == sc[8, group == g].sum()
    # robots outside [0, G) change nothing
    assert np.array_equal(S.group_reference(sc[:, inside], group[inside], G), gs)
    # column blocks combine to the undivided table: counts and the max exactly, the sums to rounding
    cuts = (0, 64, 137, 200)
    parts = [S.group_reference(sc[:, a:b], group[a:b], G) for a, b in zip(cuts[:-1], cuts[1:])]
    tot = S.combine_groups(parts)
    for r in (S.G_ROBOTS, S.G_SCORED, S.G_MAX_EP, S.G_LEFT, S.G_NOT_SOLVED):
        assert np.array_equal(tot[:, r], gs[:, r]), r
    for r in (S.G_SUM_MEAN_EP, S.G_SUM_MEAN_TAU2, S.G_SUM_MEAN_P2):
        assert np.allclose(tot[:, r], gs[:, r], rtol=1e-13, atol=0), r
    import torch
    tt = S.combine_groups([torch.as_tensor(p) for p in parts])
    assert isinstance(tt, torch.Tensor) and np.array_equal(tt.numpy(), tot)
    assert np.array_equal(parts[0], S.group_reference(sc[:, 0:64], group[0:64], G))      # the parts are not modified


def test_score_block_is_a_column_slice():
    import torch
    from robobee3d_amd import shard
    sc = torch.arange(12 * 9).reshape(12, 9)
    blk = shard.score_block(sc, 2, 7)
    assert blk.is_contiguous() and blk.shape == (12, 5) and torch.equal(blk, sc[:, 2:7])


def test_new_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("#define UMPC_SCORE_ROWS 12", "#define UMPC_GSCORE_ROWS 8",
                 "int umpcBatchScoreInit(umpc_batch_t *h, void *score, void *stream);",
                 "int umpcBatchScore(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist, "
                 "const void *ref_tab, const void *ref, long long first, long long count, long long ref_first, "
                 "long long step0, double tol_p, int after, void *score, void *stream);",
                 "int umpcBatchScoreGroups(umpc_batch_t *h, const void *score, const int32_t *group, int G, double *gstat, "
                 "void *stream);"):
        assert decl in flat, decl
    assert flat.index("umpcBatchImpulseCursor(const") < flat.index("#define UMPC_SCORE_ROWS") < flat.index("int umpcBatchSetStepKernel")
    assert (_lib.SCORE_ROWS, _lib.GSCORE_ROWS) == (S.SCORE_ROWS, S.GSCORE_ROWS) == (12, 8)
    assert len(S.SCORE_ROW_NAMES) == 12 and len(S.GSCORE_ROW_NAMES) == 8
    L = _lib.lib()
    for sym in ("umpcBatchScoreInit", "umpcBatchScore", "umpcBatchScoreGroups"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchScore.argtypes == [C.c_void_p] * 6 + [C.c_longlong] * 4 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchScoreInit(None, None, None) == -1 and b"umpcBatchScoreInit" in L.umpcLastError()
    assert L.umpcBatchScore(None, None, None, None, None, None, 0, 1, 0, 0, 1.0, 0, None, None) == -1
    assert b"umpcBatchScore" in L.umpcLastError()
    assert L.umpcBatchScoreGroups(None, None, None, 1, None, None) == -1 and b"umpcBatchScoreGroups" in L.umpcLastError()


def test_score_kernels_use_no_scratch():
    """the resource remarks of the build: the scoring kernel (8 forms by which tables there are x plain / non-temporal x 2
    dtypes), the group kernel and the init kernel spill nothing"""
    import json
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    for pat, n in (("umpc_score_kernel", 32), ("umpc_score_groups_kernel", 2), ("umpc_score_init_kernel", 2)):
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            assert res[k]["ScratchSize"] == 0, (k, res[k])


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
B_, COUNT, FIRST, REF_FIRST, STEP0, TOL = 200, 37, 3, 5, 1000, 2.0
NAN_AT, INF_AT = (12, 1, 7), (20, 2, 130)          # (state slice, row, robot), (out slice, row, robot)


def _tables(dtype, seed=20240531):
    """Seeded tables for B = 200 (three full wavefronts and a partial one): the state follows the reference with an error whose
    square is spread around TOL^2 = 4, the moments pass taulim = 100 here and there, one NaN in robot 7's position (a scored
    step for after = 0 and 1) and one Inf in robot 130's moment, statuses from {1, 2, -2}. Returned in `dtype`."""
    rng = np.random.default_rng(seed)
    ns = FIRST + COUNT + 2
    ref = np.zeros((REF_FIRST - FIRST + ns + 1, 9, B_))
    ref[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, B_)) + 0.7 * rng.normal(size=(len(ref), 3, B_))
    ref[:, 3:6] = rng.normal(size=(len(ref), 3, B_))
    ref[:, 6:9] = np.array([0, 0, 1.0])[None, :, None] + 0.05 * rng.normal(size=(len(ref), 3, B_))
    state = rng.normal(size=(ns + 1, 18, B_))
    state[:, 0:3] = ref[REF_FIRST - FIRST:REF_FIRST - FIRST + ns + 1, 0:3] + rng.normal(scale=1.1, size=(ns + 1, 3, B_))
    state[:, 9:12] = np.array([0, 0, 1.0])[None, :, None] + 0.2 * rng.normal(size=(ns + 1, 3, B_))
    out = rng.normal(scale=70.0, size=(ns, 9, B_))
    status = rng.choice(np.array([1, 2, -2], np.int32), size=(ns, B_))
    state[NAN_AT] = np.nan
    out[INF_AT] = np.inf
    return state.astype(dtype), out.astype(dtype), status, ref.astype(dtype)


def _no_step_on_the_threshold(state, ref_steps, after, tol):
    """a condition on the INPUTS (checked on the mirror's arithmetic): rows 9 and 10 are comparable only if no e_p lies within
    relative 1e-5 of tol^2 -- if this fires, choose another seed"""
    st = np.asarray(state, np.float64)[FIRST + after:FIRST + after + COUNT]
    with np.errstate(invalid="ignore"):
        ep = ((st[:, 0:3] - np.asarray(ref_steps, np.float64)[:, 0:3]) ** 2).sum(1)
    ep = ep[np.isfinite(ep)]
    assert np.abs(ep - tol * tol).min() > 1e-5 * tol * tol
    assert (ep > tol * tol).mean() > 0.2 and (ep < tol * tol).mean() > 0.2              # spread around the threshold


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want)
    return float(np.max(np.where(d == 0, 0.0, d / np.where(want == 0, np.finfo(float).tiny, np.abs(want))), initial=0.0))


def _check(got, want, nsteps, dtype, margin, tag):
    """the bounds of the issue: rows 0, 8..11 exact; rows 2, 3, 5 (one e: six roundings) relative <= 8 u; the sum rows
    (non-negative terms, any order adds at most (n - 1) u) relative <= (n + 8) u"""
    u = U[dtype]
    got = got.to("cpu").numpy().astype(np.float64) if hasattr(got, "cpu") else np.asarray(got, np.float64)
    for r in EXACT_ROWS:
        assert np.array_equal(got[r], want[r]), (tag, r, got[r], want[r])
    margin("%s max rows rel" % tag, max(_rel(got[r], want[r]) for r in MAX_ROWS), 8 * u)
    margin("%s sum rows rel" % tag, max(_rel(got[r], want[r]) for r in SUM_ROWS), (nsteps + 8) * u)


def _dev(m, a):
    import torch
    return None if a is None else torch.as_tensor(a).to(m.device).contiguous()


def _score(m, state, out, status, reftab, ref, first, count, ref_first, step0, tol, after, score=None):
    """umpcBatchScore on device tensors through the C ABI (BatchUprightMPC.score works on the handle's own history)"""
    import torch
    from robobee3d_amd.batch import _ptr
    if score is None:
        score = torch.empty((12, m.B), dtype=m.dtype, device=m.device)
        assert m.L.umpcBatchScoreInit(m.h, _ptr(score), m._stream()) == 0
    rc = m.L.umpcBatchScore(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(reftab), _ptr(ref), first, count, ref_first, step0,
                            float(tol), int(after), _ptr(score), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return score


def _mpc(B, dtype):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    return BatchUprightMPC(B, getattr(torch, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_kernel_against_the_mirror(dtype, margin):
    """after 0 / 1 x table / constant reference x all records / NULL out / NULL status / both NULL on one set of tables; then
    20 + 17 steps against 37 in one call, and columns [64, 200) on a handle of their own"""
    import torch
    from robobee3d_amd import score as S
    state, out, status, ref = _tables(np.dtype(dtype))
    m = _mpc(B_, dtype)
    taulim = float(m.prm.taulim)
    d = [_dev(m, a) for a in (state, out, status, ref)]
    cref = np.ascontiguousarray(ref[REF_FIRST])
    ident = torch.as_tensor(S.score_identity(B_)).to(m.dtype).to(m.device)
    sc0 = torch.empty((12, B_), dtype=m.dtype, device=m.device)
    assert m.L.umpcBatchScoreInit(m.h, C.c_void_p(sc0.data_ptr()), m._stream()) == 0 and torch.equal(sc0, ident)
    for after in (0, 1):
        _no_step_on_the_threshold(state, ref[REF_FIRST:REF_FIRST + COUNT], after, TOL)
        _no_step_on_the_threshold(state, np.repeat(cref[None], COUNT, 0), after, TOL)
        for table in (True, False):
            for with_out, with_status in ((True, True), (False, True), (True, False), (False, False)):
                tag = "after%d %s%s%s" % (after, "tab" if table else "const", "" if with_out else " -out", "" if with_status else " -status")
                got = _score(m, d[0], d[1] if with_out else None, d[2] if with_status else None, d[3] if table else None,
                             None if table else _dev(m, cref), FIRST, COUNT, REF_FIRST if table else 0, STEP0, TOL, after)
                want = S.score_reference(state, out if with_out else None, status if with_status else None,
                                         ref if table else cref, FIRST, COUNT, REF_FIRST if table else 0, STEP0, TOL, after, taulim)
                _check(got, want, COUNT, dtype, margin, tag)
                # the planted values did what they are there for
                assert want[S.SKIPPED, NAN_AT[2]] == 1 and want[S.SKIPPED, INF_AT[2]] == (1 if with_out else 0)
                assert want[S.SKIPPED].sum() == (2 if with_out else 1)
                if not with_out:
                    assert torch.all(got[S.SUM_TAU2] == 0)
                if not with_status:
                    assert torch.all(got[S.NOT_SOLVED] == 0)
    # chunks: 20 + 17 steps accumulate to what one call of 37 gives
    one = _score(m, d[0], d[1], d[2], d[3], None, FIRST, COUNT, REF_FIRST, STEP0, TOL, 1)
    two = _score(m, d[0], d[1], d[2], d[3], None, FIRST, 20, REF_FIRST, STEP0, TOL, 1)
    two = _score(m, d[0], d[1], d[2], d[3], None, FIRST + 20, 17, REF_FIRST + 20, STEP0 + 20, TOL, 1, score=two)
    for r in ORDER_FREE_ROWS:
        assert torch.equal(one[r], two[r]), r
    margin("chunked sum rows rel", max(_rel(two[r].cpu().numpy(), one[r].cpu().numpy()) for r in SUM_ROWS), (COUNT + 8) * U[dtype])
    _check(two, S.score_reference(state, out, status, ref, FIRST, COUNT, REF_FIRST, STEP0, TOL, 1, taulim), COUNT, dtype, margin, "chunked")
    assert torch.equal(one, _score(m, d[0], d[1], d[2], d[3], None, FIRST, COUNT, REF_FIRST, STEP0, TOL, 1))    # run to run
    assert torch.equal(_score(m, d[0], d[1], d[2], d[3], None, FIRST, 0, REF_FIRST, STEP0, TOL, 1), ident)      # count = 0
    # blocks: columns [64, 200) from column-sliced tables on a B = 136 handle
    mb = _mpc(B_ - 64, dtype)
    blk = [_dev(mb, np.ascontiguousarray(a[..., 64:])) for a in (state, out, status, ref)]
    part = _score(mb, blk[0], blk[1], blk[2], blk[3], None, FIRST, COUNT, REF_FIRST, STEP0, TOL, 1)
    assert torch.equal(part, one[:, 64:])


@pytest.mark.gpu
def test_the_references_log_through_the_kernel(margin):
    from robobee3d_amd import score as S
    g, state, out, status, ref = _golden_tables()
    n = len(g["t"])
    m = _mpc(2, "float64")
    sc = _score(m, _dev(m, state), _dev(m, out), _dev(m, status), _dev(m, ref), None, 0, n, 0, 0, 10.0, 1).cpu().numpy()
    bound = (n + 8) * U["float64"]
    for b, name in enumerate(("kick", "plain")):
        err, eff, _, max_ep, _, bad = GOLD[name]
        margin("%s logMetric err rel" % name, abs(sc[S.SUM_P2, b] / sc[S.STEPS, b] - err) / err, bound)
        margin("%s logMetric eff rel" % name, abs(sc[S.SUM_TAU2, b] / sc[S.STEPS, b] - eff) / eff, bound)
        margin("%s max e_p rel" % name, abs(sc[S.MAX_EP, b] - max_ep) / max_ep, 8 * U["float64"])
        assert sc[S.STEPS, b] == n and sc[S.NOT_SOLVED, b] == bad and sc[S.SKIPPED, b] == 0
    _check(sc, S.score_reference(state, out, status, ref, 0, n, 0, 0, 10.0, True, 100.0), n, "float64", margin, "golden")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_groups_against_the_mirror(dtype, margin):
    import torch
    from robobee3d_amd import score as S
    G = 7
    m = _mpc(B_, dtype)
    sc = _random_score(B_, 21).astype(np.dtype(dtype))
    group = np.random.default_rng(22).integers(-1, G + 1, B_).astype(np.int32)
    assert (group == -1).any() and (group == G).any()
    dsc = _dev(m, sc)
    gs = m.score_groups(dsc, group, G)
    assert gs.dtype == torch.float64 and tuple(gs.shape) == (G, 8)
    want = S.group_reference(sc, group, G)
    got = gs.cpu().numpy()
    for r in (S.G_ROBOTS, S.G_SCORED, S.G_MAX_EP, S.G_LEFT, S.G_NOT_SOLVED):
        assert np.array_equal(got[:, r], want[:, r]), r
    margin("group sums rel", max(_rel(got[:, r], want[:, r]) for r in (S.G_SUM_MEAN_EP, S.G_SUM_MEAN_TAU2, S.G_SUM_MEAN_P2)),
           (B_ + 8) * U["float64"])
    assert torch.equal(gs, m.score_groups(dsc, group, G))


@pytest.mark.gpu
def test_end_to_end_sweep_is_scored_on_the_device(margin):
    """task_table + set_reference_trajectory + record_history(status) + one push (of every second robot: 2 mm / ms carry a robot
    out of the 10 mm tube, the slow small helices without a push stay inside), 12 steps at B = 128 in fp32: m.score() against
    the mirror on the downloaded tables, in one call and as steps 0..5 then 6..11 with the score passed back"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, tol = 128, 12, 10.0     # 10 mm: the slow, small helices of the grid stay inside it, the fast ones leave within 60 ms
    m = _mpc(B, "float32")
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    m.set_state(st, ref)
    amp = np.repeat(np.linspace(20, 80, 8), 16)
    tab = m.task_table(K, "helix", trajAmp=amp, trajFreq=np.tile(np.linspace(0.5, 2, 16), 8), dz=0.05)
    m.set_reference_trajectory(tab)
    m.record_history(K, status=True)
    m.set_impulses(m.impulse_table(K, [(4, slice(0, B, 2), (0, 2, 0, 0, 0, 0))]))      # every second robot is pushed
    m.rollout(K)
    h = m.history()
    tabs = [h["state"].cpu().numpy(), h["out"].cpu().numpy(), h["status"].cpu().numpy(), tab.cpu().numpy()]
    taulim = float(m.prm.taulim)
    for after in (False, True):
        want = S.score_reference(*tabs, 0, K, 0, 0, tol, after, taulim)
        ep = ((tabs[0][int(after):K + int(after), 0:3].astype(np.float64) - tabs[3][:, 0:3]) ** 2).sum(1)
        print("e_p quantiles (after=%d):" % after, np.quantile(ep, [0, 0.25, 0.5, 0.75, 1]))
        assert np.abs(ep - tol * tol).min() > 1e-5 * tol * tol                       # a condition on the inputs, as above
        assert np.all(want[S.STEPS] == K) and (want[S.FIRST_OVER] >= 0).any() and (want[S.FIRST_OVER] < 0).any()
        _check(m.score(tol=tol, after=after), want, K, "float32", margin, "end to end after%d" % after)
    one = m.score(tol=tol)
    two = m.score(0, 6, tol=tol)
    two = m.score(6, 6, tol=tol, score=two)
    for r in ORDER_FREE_ROWS:
        assert torch.equal(one[r], two[r]), r
    margin("end to end chunked sum rows rel", max(_rel(two[r].cpu().numpy(), one[r].cpu().numpy()) for r in SUM_ROWS), (K + 8) * U["float32"])
    # cells: 8 amplitudes x 16 robots each
    cells = m.score_groups(one, np.repeat(np.arange(8, dtype=np.int32), 16), 8).cpu().numpy()
    wantg = S.group_reference(one.cpu().numpy(), np.repeat(np.arange(8), 16), 8)
    assert np.array_equal(cells[:, 0], np.full(8, 16.0)) and np.allclose(cells, wantg, rtol=(16 + 8) * U["float64"], atol=0)
    # no table set, task 0: the constant `m.ref` is the reference of every step
    m3 = _mpc(B, "float32")
    m3.set_state(st, ref)
    m3.record_history(4, status=True)
    m3.rollout(4)
    h3 = m3.history()
    tabs3 = [h3["state"].cpu().numpy(), h3["out"].cpu().numpy(), h3["status"].cpu().numpy(), m3.ref.cpu().numpy()]
    ep3 = ((tabs3[0][1:5, 0:3].astype(np.float64) - tabs3[3][None, 0:3]) ** 2).sum(1)
    print("e_p quantiles (constant reference):", np.quantile(ep3, [0, 0.25, 0.5, 0.75, 1]))
    assert np.abs(ep3 - 0.25).min() > 1e-5 * 0.25                                    # a condition on the inputs, as above
    _check(m3.score(tol=0.5, after=True, step0=7), S.score_reference(*tabs3, 0, 4, 0, 7, 0.5, True, taulim), 4, "float32", margin,
           "end to end constant reference")
    # a handle that follows a task generator has no table to score against
    m2 = _mpc(B, "float32")
    m2.set_state(st, ref)
    m2.set_task("helix")
    m2.record_history(2)
    m2.rollout(2)
    with pytest.raises(RuntimeError, match="task_table"):
        m2.score()
    with pytest.raises(ValueError):
        m.score(0, K + 1)


@pytest.mark.gpu
def test_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import _ptr
    m = _mpc(64, "float32")
    L, h, s = m.L, m.h, m._stream()
    state = torch.zeros((4, 18, 64), device=m.device)
    ref = torch.zeros((9, 64), device=m.device)
    tab = torch.zeros((3, 9, 64), device=m.device)
    score = torch.full((12, 64), 3.0, device=m.device)
    keep = score.clone()
    P = _ptr
    ok = dict(state=P(state), tab=None, ref=P(ref), first=0, count=3, ref_first=0, step0=0, tol=1.0, score=P(score))
    for bad in (dict(count=-1), dict(first=-1), dict(ref_first=-1), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
                dict(score=None), dict(state=None), dict(tab=P(tab)), dict(ref=None), dict(step0=(1 << 24) - 2),
                dict(count=(1 << 24) + 1), dict(step0=-1), dict(count=(1 << 31) - 16)):
        a = dict(ok, **bad)
        rc = L.umpcBatchScore(h, a["state"], None, None, a["tab"], a["ref"], a["first"], a["count"], a["ref_first"], a["step0"],
                              a["tol"], 0, a["score"], s)
        assert rc == -1 and b"umpcBatchScore" in L.umpcLastError(), bad
    torch.cuda.synchronize()
    assert torch.equal(score, keep)
    assert L.umpcBatchScoreGroups(h, P(score), None, 4, None, s) == -1 and b"umpcBatchScoreGroups" in L.umpcLastError()
    assert L.umpcBatchScoreGroups(h, P(score), P(torch.zeros(64, dtype=torch.int32, device=m.device)), 0,
                                  P(torch.zeros((1, 8), dtype=torch.float64, device=m.device)), s) == -1
    # the same call with good arguments goes through, and count = 0 changes nothing
    assert L.umpcBatchScore(h, P(state), None, None, None, P(ref), 0, 0, 0, 0, 1.0, 0, P(score), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(score, keep)
    assert L.umpcBatchScore(h, P(state), None, None, None, P(ref), 0, 3, 0, 0, 1.0, 0, P(score), s) == 0
    torch.cuda.synchronize()
    assert torch.all(score[0] == 6.0) and torch.all(score[11] == 3.0)
