"""Bootstrap confidence bands of ensemble curves on the device: umpcBatchEnsembleBootstrap resamples the draws of every group at
every recorded step R times, takes a statistic of each resample and gives the step its point estimate, the mean, standard error
and percentile band of the replicates; over the window every replicate keeps its largest studentised distance (sup), whose
quantiles (crit) are the critical values of a simultaneous band. The numpy mirror (robobee3d_amd/score.py:
ensemble_bootstrap_reference) is the definition.
CPU: the mirror by hand, common random numbers, the statistical sense of the two bands, exports, refusals without a handle, the
resource record of the build.
GPU: exact tables bit for bit on both sides of the 64-value switch, the per-step path of umpcBatchScore + umpcBatchScoreBootstrap on the device alone, noise
tables within the rounding of a sum, independence of a row from everything but its cell, one end-to-end MPC-against-reactive
sweep, refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
TERMS = {"ep": 0, "es": 1, "tau": 2}
STATS = ("mean", "quantile")
PROBS = (0.05, 0.5, 0.95)
LEVELS = (0.5, 0.9)


def _same(a, b):
    """equal as doubles bit for bit, but any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _curve_tables(x, other=None):
    """a history whose e_p is a given table: x [K, B] >= 0 becomes p = (sqrt(x), 0, 0) against a reference at the origin, s =
    sdes = e3; only for x whose square roots square back exactly (squares of small integers, NaN). Returns (state [K + 1, 18, B],
    ref [9, B]) or, with `other`, the second state too."""
    def state_of(v):
        v = np.asarray(v, np.float64)
        st = np.zeros((v.shape[0] + 1, 18, v.shape[1]))
        st[:-1, 0] = np.sqrt(v)
        st[:, 11] = 1.0
        assert np.array_equal(st[:-1, 0] ** 2, v, equal_nan=True)
        return st
    ref = np.zeros((9, np.asarray(x).shape[1]))
    ref[8] = 1.0
    return (state_of(x), ref) if other is None else (state_of(x), ref, state_of(other))


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_band_mirror_by_hand():
    from robobee3d_amd import score as S
    assert (S.BAND_N, S.BAND_SKIPPED, S.BAND_POINT, S.BAND_MEAN, S.BAND_SE, S.BAND_ENTERS, S.BAND_FIRST) == (0, 1, 2, 3, 4, 5, 6)
    R = 9
    # nsc = 1: every replicate is the value, the step does not enter, sup and crit are NaN
    state, ref = _curve_tables([[4.0], [9.0]])
    order, offset = np.array([0], np.int32), np.array([0, 1], np.int32)
    for stat in STATS:
        band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, 2, 0, False, 100.0, order, offset, stat=stat, reps=R,
                                                         probs=(0.0, 1.0), levels=(0.9,))
        assert band[:, 0].tolist() == [[1, 0, 4.0, 4.0, 0.0, 0.0, 4.0, 4.0], [1, 0, 9.0, 9.0, 0.0, 0.0, 9.0, 9.0]]
        assert crit[0, 0] == 0 and np.isnan(crit[0, 1]) and np.isnan(sup).all() and sup.shape == (1, R)
    # a constant cell: the replicates are all the same double, se is 0 (or an ulp had they differed): excluded by the all-equal rule
    for n in (2, 3, 7, 64):
        c = float(np.float32(0.1 * n + 0.3)) ** 2
        state, ref = np.zeros((2, 18, n)), np.zeros((9, n))
        state[:, 0], state[:, 11], ref[8] = float(np.float32(0.1 * n + 0.3)), 1.0, 1.0
        order, offset = np.arange(n, dtype=np.int32), np.array([0, n], np.int32)
        band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, 1, 0, False, 100.0, order, offset, reps=50, seed=n)
        assert band[0, 0, :3].tolist() == [n, 0, c] and band[0, 0, S.BAND_ENTERS] == 0.0 and band[0, 0, S.BAND_SE] <= 2 * U53 * c
        assert crit[0, 0] == 0 and np.isnan(crit[0, 1:]).all() and np.isnan(sup).all()
    # two steps of three draws, R = 9, sup and crit written out from the index table (small dyadic values: every sum is exact)
    x = np.array([[1.0, 4.0, 16.0], [9.0, 0.0, 36.0]])
    state, ref = _curve_tables(x)
    order, offset = np.arange(3, dtype=np.int32), np.array([0, 3], np.int32)
    J = S.bootstrap_indices(3, R, 5).tolist()
    assert len({tuple(j) for j in J}) > 1
    for stat in STATS:
        def statistic(v):
            return sum(v) / 3 if stat == "mean" else sorted(v)[S.quantile_rank(0.5, 3)]
        t = [[statistic([x[i][j] for j in row]) for row in J] for i in range(2)]
        point = [statistic(list(x[i])) for i in range(2)]
        mean = [math.fsum(ti) / R for ti in t]
        se = [math.sqrt(math.fsum((v - m) ** 2 for v in ti) / (R - 1)) for ti, m in zip(t, mean)]
        want_sup = [max(abs(t[i][r] - point[i]) / se[i] for i in range(2)) for r in range(R)]
        band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, 2, 0, False, 100.0, order, offset, stat=stat, p=0.5,
                                                         reps=R, seed=5, probs=(0.0, 0.5, 1.0), levels=(0.0, 0.5, 1.0))
        for i in range(2):
            assert band[i, 0].tolist() == [3, 0, point[i], mean[i], se[i], 1.0, min(t[i]), sorted(t[i])[4], max(t[i])]
        assert sup[0].tolist() == want_sup
        assert crit[0].tolist() == [2, min(want_sup), sorted(want_sup)[4], max(want_sup)]
        # the same replicate draws the same members at both steps: whole trajectories
        for r, row in enumerate(J):
            assert [t[i][r] for i in range(2)] == [statistic([x[i][j] for j in row]) for i in range(2)]
    # other= subtracts, and skips a member missing in either table; a step of one pair does not enter
    a = np.array([[25.0, 36.0, 49.0, 64.0], [1.0, np.nan, 9.0, 16.0]])
    b = np.array([[1.0, 4.0, np.nan, 16.0], [4.0, 4.0, np.nan, 0.0]])
    state, ref, ostate = _curve_tables(a, b)
    order, offset = np.arange(4, dtype=np.int32), np.array([0, 4], np.int32)
    band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, 2, 0, False, 100.0, order, offset, other=(ostate, None),
                                                     reps=R, probs=(0.0, 1.0))
    assert band[0, 0, :3].tolist() == [3, 1, (24.0 + 32.0 + 48.0) / 3]              # 25 - 1, 36 - 4, 64 - 16
    assert band[1, 0, :3].tolist() == [2, 2, (-3.0 + 16.0) / 2]                      # 1 - 4 and 16 - 0: a difference may be negative
    assert set(band[1, 0, 6:].tolist()) <= {-3.0, 6.5, 16.0} and crit[0, 0] == 2
    # an empty group and a step where nobody is scored: NaN rows, column 5 = 0
    state, ref = _curve_tables([[4.0, 9.0], [np.nan, np.nan]])
    order, offset = S.group_index_reference(np.array([0, 0], np.int32), 2)
    band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, 2, 0, False, 100.0, order, offset, reps=R)
    assert band[1, 0, :2].tolist() == [0, 2] and np.isnan(band[1, 0, [2, 3, 4, 6, 7]]).all() and band[1, 0, 5] == 0 and crit[0, 0] == 1
    assert band[:, 1, :2].tolist() == [[0, 0], [0, 0]] and np.isnan(sup[1]).all() and crit[1, 0] == 0 and not np.isnan(sup[0]).any()
    # the terms in the tables' dtype: fp32 terms widened, not fp64 terms
    st32 = np.random.default_rng(0).normal(size=(3, 18, 4)).astype(np.float32)
    r32 = np.random.default_rng(1).normal(size=(9, 4)).astype(np.float32)
    order, offset = np.arange(4, dtype=np.int32), np.array([0, 4], np.int32)
    b32 = S.ensemble_bootstrap_reference(st32, None, r32, 0, 2, 0, False, 100.0, order, offset, stat="quantile", p=1.0, reps=R,
                                         dtype=np.float32)[0]
    d = st32[:2, 0:3] - r32[0:3]
    assert b32[:, 0, 2].tolist() == ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max(1).astype(np.float64).tolist()
    for bad in (dict(stat="median"), dict(p=1.5), dict(reps=1), dict(reps=4097), dict(probs=()), dict(levels=(1.5,)),
                dict(levels=()), dict(term=3), dict(term=S.TERM_TAU), dict(count=-1), dict(other=(st32[:, :, :2], None))):
        kw = dict(first=0, count=2, ref_first=0, after=False, taulim=100.0, order=order, offset=offset)
        kw.update(bad)
        with pytest.raises(ValueError):
            S.ensemble_bootstrap_reference(st32, None, r32, **kw)


def test_equal_cells_share_draws_and_sup_ignores_the_order_of_steps():
    from robobee3d_amd import score as S
    rng = np.random.default_rng(4)
    K, n, R = 6, 17, 60
    x = rng.integers(0, 40, size=(K, n)).astype(np.float64) ** 2
    state, ref = _curve_tables(np.concatenate([x, x, rng.integers(0, 40, size=(K, n)).astype(np.float64) ** 2], 1))
    order, offset = S.group_index_reference(np.repeat(np.arange(3, dtype=np.int32), n), 3)
    for stat in STATS:
        band, crit, sup = S.ensemble_bootstrap_reference(state, None, ref, 0, K, 0, False, 100.0, order, offset, stat=stat, reps=R,
                                                         seed=3, probs=PROBS, levels=LEVELS)
        assert np.all(band[..., 0] == n) and np.all(band[..., 5] == 1)
        # two cells holding the same values get the same rows: common random numbers
        assert _same(band[:, 0], band[:, 1]) and _same(sup[0], sup[1]) and _same(crit[0], crit[1])
        assert not _same(sup[0], sup[2])
        # permuting the steps of a window in which nsc is constant permutes the rows and leaves sup and crit alone
        perm = rng.permutation(K)
        pstate = state.copy()
        pstate[:K] = state[perm]
        pband, pcrit, psup = S.ensemble_bootstrap_reference(pstate, None, ref, 0, K, 0, False, 100.0, order, offset, stat=stat,
                                                            reps=R, seed=3, probs=PROBS, levels=LEVELS)
        assert _same(pband, band[perm]) and _same(psup, sup) and _same(pcrit, crit)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_simultaneous_band_covers_the_curve_and_the_pointwise_band_does_not(seed):
    """n = 64 draws of a K = 20 step curve 0.3 cumsum(N(0, 1)) + N(0, 1), true mean 0; statistic mean, R = 400, level 0.9,
    pointwise probs (0.05, 0.95), 300 experiments from default_rng(seed) with the indices bootstrap_indices(64, 400, seed).
    The replicates are formed vectorised (a float64 mean per resample); everything behind them is the mirror's band_rows.
    Conditions of the definition, not tuned targets: the sup-t band holds the whole true curve in >= 0.78 of the experiments
    (nominal 0.9 less the bootstrap's known small-sample under-coverage, binomial sigma 0.021), the pointwise band in <= 0.35."""
    from robobee3d_amd import score as S
    n, K, R, E = 64, 20, 400, 300
    rng = np.random.default_rng(seed)
    J = S.bootstrap_indices(n, R, seed)
    simul = point = 0
    for _ in range(E):
        x = 0.3 * np.cumsum(rng.normal(size=(K, n)), 0) + rng.normal(size=(K, n))
        t = x[:, J].mean(2)                                                        # [K, R]
        est = x.mean(1)
        rows, sup, crit = S.band_rows(t, est, np.full(K, n), (0.05, 0.95), (0.9,))
        assert crit[0] == K and np.all(rows[:, 2] == 1)
        simul += bool(np.all(np.abs(est) <= crit[1] * rows[:, 1]))
        point += bool(np.all((rows[:, 3] <= 0.0) & (0.0 <= rows[:, 4])))
    print("seed %d: simultaneous band holds the curve in %.3f of %d experiments, pointwise band in %.3f" % (seed, simul / E, E, point / E))
    assert simul / E >= 0.78
    assert point / E <= 0.35


def _fake(n=64):
    """an address that is never read: the refusals come before any HIP call"""
    buf = (C.c_double * n)()
    return buf, C.c_void_p(C.addressof(buf))


def test_band_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    decls = ("#define UMPC_BAND_ROWS 6 /* columns ahead of the percentile columns */", "#define UMPC_BAND_MAX_REPS 4096",
             "int umpcBatchEnsembleBootstrap(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *other_state, "
             "const void *other_out, const void *ref_tab, const void *ref, long long first, long long count, long long ref_first, "
             "int after, const int32_t *order, const int32_t *offset, int G, int term, int stat, double stat_p, int R, "
             "unsigned long long seed, const double *probs, int nq, const double *levels, int nl, "
             "double *band, double *crit, double *sup, double *work, void *stream);")
    at = [flat.index(d) for d in decls]
    assert at == sorted(at) and flat.index("int umpcBatchScoreBootstrap(") < at[0]
    assert (_lib.BAND_ROWS, _lib.BAND_MAX_REPS) == (6, 4096) and S.BAND_MAX_REPS == 4096 and S.BAND_FIRST == 6
    L = _lib.lib()
    assert "umpcBatchEnsembleBootstrap" in _lib.EXPORTS and L.umpcBatchEnsembleBootstrap
    vp, ll, dp = C.c_void_p, C.c_longlong, C.POINTER(C.c_double)
    assert L.umpcBatchEnsembleBootstrap.argtypes == [vp] * 7 + [ll] * 3 + [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                                                          C.c_ulonglong, dp, C.c_int, dp, C.c_int, vp, vp, vp, vp, vp]
    keepalive, p = _fake()
    arr = lambda *v: (C.c_double * len(v))(*v)
    ok = dict(state=p, out=None, ostate=None, oout=None, reftab=None, ref=p, first=0, count=5, ref_first=0, after=0, order=p, offset=p,
              G=1, term=0, stat=0, stat_p=0.5, R=100, seed=3, probs=arr(0.025, 0.975), nq=2, levels=arr(0.9), nl=1, band=p, crit=p,
              sup=p, work=p)

    def call(**bad):
        a = dict(ok, **bad)
        rc = L.umpcBatchEnsembleBootstrap(None, a["state"], a["out"], a["ostate"], a["oout"], a["reftab"], a["ref"], a["first"], a["count"],
                                          a["ref_first"], a["after"], a["order"], a["offset"], a["G"], a["term"], a["stat"], a["stat_p"],
                                          a["R"], a["seed"], a["probs"], a["nq"], a["levels"], a["nl"], a["band"], a["crit"], a["sup"],
                                          a["work"], None)
        return rc, L.umpcLastError()
    rc, err = call()
    assert rc == -1 and b"umpcBatchEnsembleBootstrap" in err and b"handle" in err                # all good but the handle
    rc, err = call(crit=None, sup=None, levels=None, nl=0)
    assert rc == -1 and b"handle" in err                                                          # the pointwise rows alone
    rc, err = call(count=0)
    assert rc == -1 and b"handle" in err                                                          # the handle comes before the no-op
    for bad, word in ((dict(R=1), b"R"), (dict(R=0), b"R"), (dict(R=4097), b"R"), (dict(stat=2), b"stat"), (dict(stat=-1), b"stat"),
                      (dict(stat_p=1.5), b"stat_p"), (dict(stat_p=float("nan")), b"stat_p"), (dict(nq=0), b"probabilities"),
                      (dict(nq=9, probs=arr(*[0.5] * 9)), b"probabilities"), (dict(probs=arr(0.5, 1.5)), b"probabilities"),
                      (dict(probs=arr(float("nan"), 0.5)), b"probabilities"), (dict(probs=None), b"probs"), (dict(nl=0), b"levels"),
                      (dict(nl=9, levels=arr(*[0.5] * 9)), b"levels"), (dict(levels=arr(1.5)), b"levels"), (dict(levels=arr(float("nan"))), b"levels"),
                      (dict(levels=None), b"levels"), (dict(crit=None), b"crit"), (dict(sup=None), b"sup"),
                      (dict(crit=None, sup=None), b"levels"), (dict(term=3), b"term"), (dict(term=-1), b"term"), (dict(term=2), b"out_hist"),
                      (dict(ostate=p, oout=p), b"other_out"), (dict(oout=p), b"other_out"), (dict(ostate=p, out=p), b"other_out"),
                      (dict(band=None), b"band"), (dict(work=None), b"work"), (dict(state=None), b"state_hist"), (dict(order=None), b"order"),
                      (dict(offset=None), b"offset"), (dict(G=0), b"G"), (dict(count=-1), b"count"), (dict(first=-1), b"first"),
                      (dict(ref_first=-1), b"ref_first"), (dict(count=1 << 31), b"count"), (dict(reftab=p), b"ref_tab"), (dict(ref=None), b"ref_tab")):
        rc, err = call(**bad)
        assert rc == -1 and b"umpcBatchEnsembleBootstrap" in err and word in err and b"handle" not in err, (bad, err)
    del keepalive


def test_band_kernels_use_no_scratch():
    """the resource remarks of the build: every form of the band kernel has no private frame and the static LDS that its entry of
    csrc/resource_limits.json states; a form with a frame is refused"""
    import json
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    pat, n, lds = "umpc_band_kernel", 12, 12928
    assert [k for k in limits if "band" in k] == [pat]
    hits = [k for k in res if pat in k]
    assert len(hits) == n and len([k for k in res if "umpc_band" in k]) == n, hits
    for k in hits:
        assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == lds, (k, res[k])
    assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds}
    # the static block and the most replicates a call may ask for stay under the 64 KB a block gets without asking
    assert lds + 8 * _lib.BAND_MAX_REPS <= 65536
    with pytest.raises(RuntimeError, match=pat):
        _lib._validate_resources(dict(res, **{"a_form_of_%s_with_a_frame" % pat: {"ScratchSize": 8, "LDS": lds}}))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _mpc(B, dtype):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    return BatchUprightMPC(B, getattr(torch, dtype))


def _dev(m, a):
    import torch
    return None if a is None else torch.as_tensor(a).to(m.device).contiguous()


def _band(m, state, out, ostate, oout, reftab, ref, first, count, ref_first, after, index, term, stat, p, R, seed, probs, levels,
          band=None, simul=True):
    """umpcBatchEnsembleBootstrap on device tensors through the C ABI; fresh outputs are filled with NaN first (and work with a
    canary): a row the call did not write shows (columns 0, 1 and 5 are never NaN). Returns numpy (band, crit, sup)."""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    nan = float("nan")
    if band is None:
        band = torch.full((count, G, 6 + len(probs)), nan, dtype=torch.float64, device=m.device)
    crit = torch.full((G, 1 + len(levels)), nan, dtype=torch.float64, device=m.device) if simul else None
    sup = torch.full((G, R), nan, dtype=torch.float64, device=m.device) if simul else None
    work = torch.full((m.B + G,), -77.0, dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchEnsembleBootstrap(m.h, _ptr(state), _ptr(out), _ptr(ostate), _ptr(oout), _ptr(reftab), _ptr(ref), first, count,
                                        ref_first, int(after), _ptr(order), _ptr(offset), G, TERMS[term], STATS.index(stat), p, R, seed,
                                        (C.c_double * len(probs))(*probs), len(probs),
                                        (C.c_double * len(levels))(*levels) if simul else None, len(levels) if simul else 0,
                                        _ptr(band), _ptr(crit), _ptr(sup), _ptr(work), m._stream())
    assert rc == 0, m.L.umpcLastError()
    return band.cpu().numpy(), (crit.cpu().numpy() if simul else None), (sup.cpu().numpy() if simul else None)


def _values(state, out, ref, first, count, ref_first, after, taulim, term, other, dtype):
    """(x [count, B] float64, ok [count, B]): the value of every robot at every step of the window as the mirror forms it, terms
    in `dtype` -- for the bounds of the noise tests"""
    from robobee3d_amd import score as S
    dt = np.dtype(dtype)
    x, ok = np.zeros((count, state.shape[-1])), np.zeros((count, state.shape[-1]), bool)
    for i in range(count):
        r = (ref[ref_first + i] if ref.ndim == 3 else ref).astype(dt)
        def terms(st, o):
            t = S._step_terms(st[first + i + after].astype(dt), None if o is None else o[first + i].astype(dt), r, dt.type(taulim))
            return (t[2 + term] if term < 2 else t[5]).astype(np.float64), t[0]
        x[i], ok[i] = terms(state, out)
        if other is not None:
            y, ok2 = terms(*other)
            with np.errstate(invalid="ignore", over="ignore"):
                x[i] = x[i] - y
            ok[i] &= ok2 & np.isfinite(x[i])
    return x, ok


_INDICES = {}


def _bounds(x, ok, order, offset, wband, wsup, R, seed, stat):
    """What the rounding of the device's sums may move, from the mirror's own numbers (never from the device's):
    a mean replicate t within b_t = (nsc + 1) u sum|sample| / nsc of the fsum mirror (any order of summation and the one
    division, test_bootstrap), the point estimate within b_p (the cell's own sum); a quantile replicate is an element: 0.
    Percentile columns within c = max_r b_t (an order statistic is 1-Lipschitz in the sup norm); the mean of the replicates
    within c + (R + 1) u mean|t| (test_bootstrap), mean|t| <= |mean| + se (the mean distance from the mean is at most the
    root mean square one); the standard error within dse = c sqrt(R / (R - 1)) + 1e-9 se (the norm of the centred
    replicates moves by no more than the norm of their change; 1e-9 for its own two-pass sums, as test_bootstrap).
    A studentised distance d = |t - point| / se: the error of t and of the point estimate over se, plus d times the relative
    error of se, both over the smaller se' >= se - dse, plus 4 u d for its own three operations; sup and crit (a max and an
    order statistic of maxima: 1-Lipschitz again) within the largest such bound over the entering steps.
    Returns dict of arrays: point [K, G], cols [K, G], mean [K, G], se [K, G], sup [G] (one figure per group)."""
    from robobee3d_amd import score as S
    K, G = wband.shape[:2]
    b = {k: np.zeros((K, G)) for k in ("point", "cols", "mean", "se")}
    b["sup"] = np.zeros(G)
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        for i in range(K):
            v = x[i, mem[ok[i, mem]]]
            nsc = len(v)
            assert nsc == wband[i, g, 0]
            if nsc == 0:
                continue
            bt = np.zeros(R)
            if stat == "mean":
                if (nsc, R, seed) not in _INDICES:
                    _INDICES[(nsc, R, seed)] = S.bootstrap_indices(nsc, R, seed)
                bt = (nsc + 1) * U53 * np.abs(v)[_INDICES[(nsc, R, seed)]].sum(1) / nsc
                b["point"][i, g] = (nsc + 1) * U53 * np.abs(v).sum() / nsc
            c = bt.max()
            se = wband[i, g, 4]
            b["cols"][i, g] = c
            b["mean"][i, g] = c + (R + 1) * U53 * (abs(wband[i, g, 3]) + se)
            b["se"][i, g] = dse = c * math.sqrt(R / (R - 1.0)) + 1e-9 * se
            if wband[i, g, 5]:
                # d is not kept by the mirror: sup bounds it from above
                d = wsup[g]
                b["sup"][g] = max(b["sup"][g], float(np.max((bt + b["point"][i, g]) / (se - dse) + d * (dse / (se - dse)) + 4 * U53 * d)))
    return b


def _compare(got, want, b, tag, margin=None, exact_values=False):
    """band, crit, sup of the device against the mirror's: counts and column 5 and crit column 0 exact, NaN where the mirror has
    NaN, the rest within the bounds `b` (_bounds); exact_values: the point and percentile columns bit for bit"""
    (band, crit, sup), (wband, wcrit, wsup) = got, want
    assert np.array_equal(band[..., [0, 1, 5]], wband[..., [0, 1, 5]]), tag
    assert np.array_equal(np.isnan(band), np.isnan(wband)) and np.array_equal(np.isnan(sup), np.isnan(wsup)), tag
    assert np.array_equal(crit[:, 0], wcrit[:, 0]) and np.array_equal(np.isnan(crit), np.isnan(wcrit)), tag
    live = wband[..., 0] > 0
    if exact_values:
        assert _same(band[..., 2], wband[..., 2]) and _same(band[..., 6:], wband[..., 6:]), tag
    tiny = np.finfo(float).tiny
    ratio = {"point": np.abs(band[..., 2] - wband[..., 2])[live] / np.maximum(b["point"][live], tiny),
             "percentile columns": (np.abs(band[..., 6:] - wband[..., 6:]).max(-1))[live] / np.maximum(b["cols"][live], tiny),
             "mean of the replicates": np.abs(band[..., 3] - wband[..., 3])[live] / np.maximum(b["mean"][live], tiny),
             "standard error": np.abs(band[..., 4] - wband[..., 4])[live] / np.maximum(b["se"][live], tiny)}
    some = wcrit[:, 0] > 0
    if some.any():
        ratio["sup"] = np.abs(sup - wsup)[some].max(1) / np.maximum(b["sup"][some], tiny)
        ratio["crit"] = np.abs(crit[:, 1:] - wcrit[:, 1:])[some].max(1) / np.maximum(b["sup"][some], tiny)
    for what, r in ratio.items():
        worst = float(np.max(r, initial=0.0))
        print("%s: %s / bound = %.3g" % (tag, what, worst))
        if margin is not None:
            margin("%s %s / bound" % (tag, what), worst, 1.0)
        else:
            assert worst <= 1.0, (tag, what, worst)


# cells of the exact test: nothing, the smallest, both sides of a half and of a whole wavefront (cell 9 holds the values of cell
# 8 in the same member order), the block path at its first size, across one and across the block's 256 threads
SCORED = (0, 1, 2, 3, 31, 32, 33, 63, 64, 64, 65, 129, 257)
NEVER = {1: 1, 4: 2, 8: 3, 9: 3, 10: 1, 12: 2}         # members of a cell that never enter (a NaN position at every step)
XG = len(SCORED)
XB = sum(SCORED) + sum(NEVER.values())
XSTEPS = 5
_MIRROR = {}


def _exact_layout():
    """(ids [XB], members): the robots of every cell scattered over the batch"""
    ids = np.concatenate([np.full(n + NEVER.get(g, 0), g, np.int32) for g, n in enumerate(SCORED)])
    ids = ids[np.random.default_rng(3).permutation(XB)]
    return ids, [np.nonzero(ids == g)[0] for g in range(XG)]


def _exact_tables(dtype, seed):
    """p = (x, 0, 0) against a reference at the origin, s = sdes = e3: e_p = x^2, x from a pool of 12 integers in [0, 2047]
    (many ties), exact in fp32 and fp64: every sum of at most 257 of them is exact. XSTEPS + 1 state slices. The members of
    NEVER hold a NaN at every step; one more member of the cell of 33 goes NaN at step 2 (state slice 2), so that nsc changes
    mid-window; cell 9 repeats cell 8 member by member."""
    rng = np.random.default_rng(seed)
    ids, members = _exact_layout()
    pool = np.concatenate([[0, 2047], rng.integers(1, 2047, 10)]).astype(np.float64)
    state = np.zeros((XSTEPS + 1, 18, XB))
    state[:, 0] = rng.choice(pool, size=(XSTEPS + 1, XB))
    state[:, 11] = 1.0
    for g, k in NEVER.items():
        state[:, 0, members[g][np.linspace(0, len(members[g]) - 1, k).astype(int)]] = np.nan
    state[:, 0, members[9]] = state[:, 0, members[8]]
    state[2, 0, members[6][5]] = np.nan
    ref = np.zeros((9, XB))
    ref[8] = 1.0
    return ids, state.astype(dtype), ref.astype(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 65, 257, 1000, 1024, 1025])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_exact_tables_bit_for_bit(dtype, R):
    """13 cells of 0 .. 257 scored members scattered over the batch, some members never entering, one going NaN mid-window;
    integer positions: every sum of values is exact, so every replicate is the mirror's bit for bit, and with it the counts,
    the point estimate, column 5, the percentile columns and the number of entering steps. The mean of the replicates
    (rounded quotients: not exact) equals the fsum mirror or is within the double-double bound; se, sup and crit within the
    bounds of _bounds with nothing for the replicates (b_t = b_p = 0). Both statistics, after 0 and 1, with and without a
    second history; R: one short chunk, a chunk and one, the block's stride and one, several trips, and both sides of the switch
    between the form with 4 and the form with 16 running maxima per thread."""
    from robobee3d_amd import score as S
    ids, state, ref = _exact_tables(np.dtype(dtype), 3)
    _, ostate, _ = _exact_tables(np.dtype(dtype), 4)
    ostate[3, 0, np.nonzero(ids == 7)[0][2]] = np.nan            # a member missing in the other table alone, at one step
    m = _mpc(XB, dtype)
    order, offset = S.group_index_reference(ids, XG)
    index = m.group_index(_dev(m, ids), XG)
    dstate, dostate, dref = _dev(m, state), _dev(m, ostate), _dev(m, ref)
    for stat, p, after, pair in (("mean", 0.5, 0, False), ("quantile", 0.0, 0, False), ("quantile", 0.5, 0, False),
                                 ("quantile", 1.0, 0, False), ("mean", 0.5, 1, False), ("quantile", 0.5, 1, True), ("mean", 0.5, 0, True),
                                 ("mean", 0.5, 1, True)):
        count = XSTEPS - after
        got = _band(m, dstate, None, dostate if pair else None, None, None, dref, 0, count, 0, after, index, "ep", stat, p, R, 11,
                    PROBS, LEVELS)
        key = (R, stat, p, after, pair)
        if key not in _MIRROR:                                    # (the same values in both dtypes: one mirror run serves both)
            _MIRROR[key] = S.ensemble_bootstrap_reference(state, None, ref, 0, count, 0, after, 100.0, order, offset, other=(ostate, None)
                                                          if pair else None, stat=stat, p=p, reps=R, seed=11, probs=PROBS, levels=LEVELS)
        want = _MIRROR[key]
        wband = want[0]
        if not pair:
            assert wband[0, :, 0].tolist() == list(SCORED) and wband[0, :, 1].tolist() == [NEVER.get(g, 0) for g in range(XG)]
            assert wband[2 - after, 6, 0] == 32 and wband[2 - after, 6, 1] == 1
        x, ok = _values(state, None, ref, 0, count, 0, after, 100.0, 0, (ostate, None) if pair else None, dtype)
        b = _bounds(x, ok, order, offset, wband, want[2], R, 11, "exact")
        # (the double-double mean: two roundings, and R u^2 of the sum of the magnitudes)
        b["mean"] = 2 * U53 * np.abs(wband[..., 3]) + 4 * R * U53 * U53 * (np.abs(wband[..., 3]) + wband[..., 4])
        _compare(got, want, b, "%s %s%g after%d%s R%d" % (dtype, stat[:4], p, after, " pair" if pair else "", R), exact_values=True)
        band = got[0]
        assert np.all(band[:, 1, 5] == 0) and np.all(band[:, 0, 5] == 0)            # a cell of one, an empty cell
        if not pair:
            assert _same(band[:, 8, 2:], band[:, 9, 2:]) and _same(got[2][8], got[2][9]) and _same(got[1][8], got[1][9])
    # the pointwise rows alone: the same band, nothing else written
    alone = _band(m, dstate, None, None, None, None, dref, 0, XSTEPS, 0, 0, index, "ep", "mean", 0.5, R, 11, PROBS, LEVELS, simul=False)
    both = _band(m, dstate, None, None, None, None, dref, 0, XSTEPS, 0, 0, index, "ep", "mean", 0.5, R, 11, PROBS, LEVELS)
    assert _same(alone[0], both[0])


# cells of at most 64 for the comparison with the per-step path of umpcBatchScore + umpcBatchScoreBootstrap
SMALL = (64, 1, 0, 63, 5, 33, 34)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_against_the_per_step_path_on_the_device_alone(dtype):
    """the noise tables, cells of at most 64, term e_p, statistic mean, no second history: step i of the band equals
    umpcBatchScore(first = i, count = 1) into a fresh score followed by umpcBatchScoreBootstrap(SUM_EP / STEPS, the same seed,
    R and probs) BIT FOR BIT -- counts, point, mean, se and percentile columns: the order of summation and the row code are
    those kernels' --, and sup is the torch composition of that call's replicates over the steps that column 5 marks"""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import _ptr
    state, out, ref = _noise_tables(np.dtype(dtype))
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(SMALL)])
    assert ids.shape == (NB,)
    G, R, count, seed = len(SMALL), 257, 12, 6
    m = _mpc(NB, dtype)
    index = m.group_index(_dev(m, ids), G)
    d = [_dev(m, a) for a in (state, out, ref)]
    for after in (0, 1):
        band, crit, sup = _band(m, d[0], d[1], None, None, d[2], None, NFIRST, count, NREF_FIRST, after, index, "ep", "mean", 0.5, R, seed,
                                PROBS, LEVELS)
        want_sup = torch.zeros((G, R), dtype=torch.float64, device=m.device)
        entered = np.zeros(G)
        for i in range(count):
            score = torch.empty((12, NB), dtype=m.dtype, device=m.device)
            assert m.L.umpcBatchScoreInit(m.h, _ptr(score), m._stream()) == 0
            rc = m.L.umpcBatchScore(m.h, _ptr(d[0]), _ptr(d[1]), None, _ptr(d[2]), None, NFIRST + i, 1, NREF_FIRST + i, 0, 1.0, after,
                                    _ptr(score), m._stream())
            assert rc == 0, m.L.umpcLastError()
            boot, reps = m.score_bootstrap(score, index, S.SUM_EP, S.STEPS, reps=R, seed=seed, probs=PROBS, return_reps=True)
            nboot = boot.cpu().numpy()
            assert _same(nboot[:, :5], band[i][:, :5]) and _same(nboot[:, 5:], band[i][:, 6:]), (after, i, nboot - band[i][:, [0, 1, 2, 3, 4, 6, 7, 8]])
            mark = torch.as_tensor(band[i][:, 5] == 1.0, device=m.device)
            dist = (reps - boot[:, 2:3]).abs() / boot[:, 4:5]
            want_sup = torch.where(mark[:, None] & (dist > want_sup), dist, want_sup)
            entered += band[i][:, 5]
        assert entered.tolist() == crit[:, 0].tolist() and (entered > 0).sum() == 5 and entered[0] == count
        want_sup = want_sup.cpu().numpy()
        want_sup[entered == 0] = np.nan
        assert _same(sup, want_sup), after
        ss = np.sort(sup, axis=1)
        assert _same(crit[:, 1:], np.stack([ss[:, S.quantile_rank(q, R)] for q in LEVELS], 1))


NB, NCOUNT, NFIRST, NREF_FIRST = 200, 8, 3, 5
# (state slice, row, robot), (out slice, row, robot), (state slice of the second history, row, robot): inside the window of
# NCOUNT steps from NFIRST for after = 0 and 1
NAN_AT, INF_AT, ONAN_AT = (7, 1, 7), (8, 2, 130), (6, 9, 41)
NSIZES = (64, 1, 0, 65, 63, 5)


def _noise_tables(dtype, seed=20240531):
    """the seeded tables of test_score.py (its generator, copied): B = 200, the state follows the reference with an error whose
    square is spread around 4, the moments pass taulim = 100 here and there, one NaN in robot 7's position and one Inf in robot
    130's moment. Returned in `dtype`: (state, out, ref)."""
    rng = np.random.default_rng(seed)
    ns = NFIRST + 37 + 2
    ref = np.zeros((NREF_FIRST - NFIRST + ns + 1, 9, NB))
    ref[:, 0:3] = rng.normal(scale=10.0, size=(1, 3, NB)) + 0.7 * rng.normal(size=(len(ref), 3, NB))
    ref[:, 3:6] = rng.normal(size=(len(ref), 3, NB))
    ref[:, 6:9] = np.array([0, 0, 1.0])[None, :, None] + 0.05 * rng.normal(size=(len(ref), 3, NB))
    state = rng.normal(size=(ns + 1, 18, NB))
    state[:, 0:3] = ref[NREF_FIRST - NFIRST:NREF_FIRST - NFIRST + ns + 1, 0:3] + rng.normal(scale=1.1, size=(ns + 1, 3, NB))
    state[:, 9:12] = np.array([0, 0, 1.0])[None, :, None] + 0.2 * rng.normal(size=(ns + 1, 3, NB))
    out = rng.normal(scale=70.0, size=(ns, 9, NB))
    rng.choice(np.array([1, 2, -2], np.int32), size=(ns, NB))                      # (the status record of the original: the same stream)
    state[NAN_AT] = np.nan
    out[INF_AT] = np.inf
    return state.astype(dtype), out.astype(dtype), ref.astype(dtype)


def _noise_groups(layout):
    """[200] ids of test_ensemble.py: the groups in order with the ignored ids -1 and G at robots 70 and 199; "permuted": the
    same array permuted, then ids swapped so that robot 7 (the NaN of the tables) is the singleton group's only member"""
    G = len(NSIZES)
    ids = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(NSIZES)])
    ids = np.append(np.insert(ids, 70, -1), G).astype(np.int32)
    if layout == "permuted":
        ids = ids[np.random.default_rng(7).permutation(NB)]
        j = int(np.nonzero(ids == 1)[0][0])
        ids[j], ids[7] = ids[7], ids[j]
    assert ids.shape == (NB,) and [(ids == g).sum() for g in range(G)] == list(NSIZES)
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_noise_tables_within_the_rounding_of_a_sum(dtype, margin):
    """the planted-NaN/inf tables: both layouts x table / constant reference x with / without out_hist x all terms, with and
    without a second history (another seed, a NaN of its own). The mirror forms the terms in the tables' dtype, as the device
    does, so what is left is the rounding of the sums: counts, column 5 and the entering steps exact; the quantile statistic
    an element, bit for bit; the mean statistic within the bounds of _bounds, every achieved-to-bound ratio recorded."""
    from robobee3d_amd import score as S
    dt = np.dtype(dtype)
    state, out, ref = _noise_tables(dt)
    ostate, oout, _ = _noise_tables(dt, seed=77)
    ostate[ONAN_AT] = np.nan
    m = _mpc(NB, dtype)
    taulim = float(m.prm.taulim)
    d = [_dev(m, a) for a in (state, out, ref, ostate, oout)]
    cref = np.ascontiguousarray(ref[NREF_FIRST])
    dcref = _dev(m, cref)
    G, R, seed = len(NSIZES), 130, 8
    for layout in ("contiguous", "permuted"):
        ids = _noise_groups(layout)
        order, offset = S.group_index_reference(ids, G)
        index = m.group_index(_dev(m, ids), G)
        for table in (True, False):
            for with_out in (True, False):
                for pair in (False, True):
                    after = int(table != with_out)                                  # (both conventions, spread over the forms)
                    for term in ("ep", "es", "tau") if with_out else ("ep", "es"):
                        tag = "%s %s%s%s %s" % (layout[:4], "tab" if table else "const", "" if with_out else " -out", " pair" if pair else "", term)
                        targs = (state, out if with_out else None, ref if table else cref, NFIRST, NCOUNT, NREF_FIRST if table else 0, after, taulim)
                        other = (ostate, oout if with_out else None) if pair else None
                        dargs = (d[0], d[1] if with_out else None, d[3] if pair else None, d[4] if pair and with_out else None,
                                 d[2] if table else None, None if table else dcref, NFIRST, NCOUNT, NREF_FIRST if table else 0, after, index, term)
                        x, ok = _values(*targs, TERMS[term], other, dt)
                        for stat, p in (("mean", 0.5),) + ((("quantile", 0.5),) if term == "ep" else ()):
                            got = _band(m, *dargs, stat, p, R, seed, PROBS, LEVELS)
                            want = S.ensemble_bootstrap_reference(*targs, order, offset, term=TERMS[term], other=other, stat=stat, p=p,
                                                                  reps=R, seed=seed, probs=PROBS, levels=LEVELS, dtype=dt)
                            b = _bounds(x, ok, order, offset, want[0], want[2], R, seed, stat)
                            _compare(got, want, b, "%s %s" % (tag, stat[:4]), margin if stat == "mean" else None, exact_values=stat == "quantile")
                    inside = lambda b_: int(0 <= ids[b_] < G)
                    skipped = inside(NAN_AT[2]) + (inside(INF_AT[2]) if with_out else 0) + (inside(ONAN_AT[2]) if pair else 0)
                    assert want[0][..., 1].sum() == skipped, (tag, want[0][..., 1].sum(), skipped)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_band_depends_on_its_cell_alone(dtype):
    """cells 0 (64 members), 3 (65: through `work`), 4 (63) and 5 (5) keep the bits of their band, crit and sup when the groups
    are re-numbered, cells are appended (G grows) and the other cells' robots are dealt out differently or ignored; two calls
    with the same arguments are bit-identical; a window cut into two calls that write slices of one band gives the same rows;
    count = 0 writes nothing. Last, the most replicates a call takes (R = 4096, 32 KB of dynamic LDS) against the mirror."""
    from robobee3d_amd import score as S
    state, out, ref = _noise_tables(np.dtype(dtype))
    ostate, oout, _ = _noise_tables(np.dtype(dtype), seed=77)
    m = _mpc(NB, dtype)
    d = [_dev(m, a) for a in (state, out, ref, ostate, oout)]
    ids = _noise_groups("permuted")
    index = m.group_index(_dev(m, ids), len(NSIZES))
    to = {0: 7, 3: 0, 4: 11, 5: 2}
    rng = np.random.default_rng(2)
    rest = ~np.isin(ids, list(to))
    ids2 = ids.copy()
    ids2[rest] = rng.choice([1, 3, 4, 5, 6, 8, -1, 12], int(rest.sum()))
    for g, h in to.items():
        ids2[ids == g] = h
    index2 = m.group_index(_dev(m, ids2), 12)
    R = 200
    for stat, p, pair in (("mean", 0.5, True), ("quantile", 0.5, False)):
        args = (d[0], d[1], d[3] if pair else None, d[4] if pair else None, d[2], None)
        one = _band(m, *args, NFIRST, NCOUNT, NREF_FIRST, 1, index, "ep", stat, p, R, 9, PROBS, LEVELS)
        again = _band(m, *args, NFIRST, NCOUNT, NREF_FIRST, 1, index, "ep", stat, p, R, 9, PROBS, LEVELS)
        assert all(_same(a, b) for a, b in zip(one, again))
        assert not np.isnan(one[0][..., [0, 1, 5]]).any() and not np.isnan(one[1][:, 0]).any()
        two = _band(m, *args, NFIRST, NCOUNT, NREF_FIRST, 1, index2, "ep", stat, p, R, 9, PROBS, LEVELS)
        assert two[0].shape == (NCOUNT, 12, 9) and two[2].shape == (12, R)
        for g, h in to.items():
            assert _same(one[0][:, g], two[0][:, h]) and _same(one[1][g], two[1][h]) and _same(one[2][g], two[2][h]), (stat, g)
        # another seed is another band
        assert not _same(one[2][0], _band(m, *args, NFIRST, NCOUNT, NREF_FIRST, 1, index, "ep", stat, p, R, 10, PROBS, LEVELS)[2][0])
        # the window in two calls, written into slices of one band
        import torch
        whole = torch.full((NCOUNT, len(NSIZES), 9), float("nan"), dtype=torch.float64, device=m.device)
        _band(m, *args, NFIRST, 5, NREF_FIRST, 1, index, "ep", stat, p, R, 9, PROBS, LEVELS, band=whole[:5])
        _band(m, *args, NFIRST + 5, NCOUNT - 5, NREF_FIRST + 5, 1, index, "ep", stat, p, R, 9, PROBS, LEVELS, band=whole[5:])
        assert _same(whole.cpu().numpy(), one[0])
        keep = whole.clone()
        nothing = _band(m, *args, NFIRST, 0, NREF_FIRST, 1, index, "ep", stat, p, R, 9, PROBS, LEVELS, band=whole)
        assert _same(nothing[0], keep.cpu().numpy()) and np.isnan(nothing[1]).all() and np.isnan(nothing[2]).all()
    order, offset = S.group_index_reference(ids, len(NSIZES))
    got = _band(m, d[0], d[1], None, None, d[2], None, NFIRST, 3, NREF_FIRST, 0, index, "es", "mean", 0.5, 4096, 5, PROBS, LEVELS)
    want = S.ensemble_bootstrap_reference(state, out, ref, NFIRST, 3, NREF_FIRST, 0, float(m.prm.taulim), order, offset, term=1, reps=4096,
                                          seed=5, probs=PROBS, levels=LEVELS, dtype=np.dtype(dtype))
    x, ok = _values(state, out, ref, NFIRST, 3, NREF_FIRST, 0, float(m.prm.taulim), 1, None, dtype)
    _compare(got, want, _bounds(x, ok, order, offset, want[0], want[2], 4096, 5, "mean"), "%s R 4096" % dtype)


@pytest.mark.gpu
def test_end_to_end_mpc_minus_reactive_with_a_band(margin):
    """B = 256 as 4 contiguous cells of 64 draws, 12 closed-loop steps of rollout() and of reactive_steps() from the same start
    on the same tables, a push at step 3 in cells 1 and 3; ensemble_bootstrap(other=reactive) on the MPC handle against the
    mirror on the downloaded histories, at the bounds of the noise test. Nothing is asserted about which controller wins."""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, R = 256, 12, 200
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    cell = (np.arange(B) // 64).astype(np.int32)
    handles = []
    for use_mpc in (True, False):
        m = _mpc(B, "float32")
        m.set_state(st, ref)
        m.set_impulses(m.impulse_table(K, [(3, np.nonzero((cell == 1) | (cell == 3))[0], (0.0, 2.0, 0.0, 0.0, 0.0, 0.0))]))
        m.record_history(K)
        m.rollout(K) if use_mpc else m.reactive_steps(K)
        handles.append(m)
    mpc, rea = handles
    index = mpc.group_index(cell, 4)
    order, offset = S.group_index_reference(cell, 4)
    hm, hr = mpc.history(), rea.history()
    tabs = [h[k].cpu().numpy() for h in (hm, hr) for k in ("state", "out")]
    cref = mpc.ref.cpu().numpy()
    taulim = float(mpc.prm.taulim)
    for stat, term in (("mean", "ep"), ("quantile", "ep"), ("mean", "tau")):
        band, crit, sup = mpc.ensemble_bootstrap(index, term=term, stat=stat, reps=R, seed=1, probs=PROBS, levels=LEVELS, other=rea, after=True)
        assert band.dtype == torch.float64 and tuple(band.shape) == (K, 4, 9) and tuple(crit.shape) == (4, 3) and tuple(sup.shape) == (4, R)
        only = mpc.ensemble_bootstrap(index, term=term, stat=stat, reps=R, seed=1, probs=PROBS, other=rea, after=True, simultaneous=False)
        assert torch.equal(only.view(torch.int64), band.view(torch.int64))
        got = tuple(t.cpu().numpy() for t in (band, crit, sup))
        want = S.ensemble_bootstrap_reference(tabs[0], tabs[1], cref, 0, K, 0, True, taulim, order, offset, term=TERMS[term],
                                              other=(tabs[2], tabs[3]), stat=stat, reps=R, seed=1, probs=PROBS, levels=LEVELS, dtype=np.float32)
        assert np.all(want[0][..., 0] == 64) and np.all(want[0][..., 5] == 1) and np.all(want[1][:, 0] == K)
        x, ok = _values(tabs[0], tabs[1], cref, 0, K, 0, True, taulim, TERMS[term], (tabs[2], tabs[3]), np.float32)
        b = _bounds(x, ok, order, offset, want[0], want[2], R, 1, stat)
        _compare(got, want, b, "end to end %s %s" % (stat[:4], term), margin if stat == "mean" else None, exact_values=stat == "quantile")
        lo, hi = (got[0][..., 2] + s * got[1][None, :, 2] * got[0][..., 4] for s in (-1.0, 1.0))
        print(stat, term, "MPC - reactive, cell 1 (pushed at step 3): point, simultaneous 90 % band\n",
              np.stack([got[0][:, 1, 2], lo[:, 1], hi[:, 1]], 1))
        assert np.all(lo <= got[0][..., 2]) and np.all(got[0][..., 2] <= hi) and np.all(got[0][..., 6] <= got[0][..., 8])
    # the band of one run alone, from the first step of the push on
    alone = mpc.ensemble_bootstrap(index, reps=R, first=3, after=True, simultaneous=False)
    assert tuple(alone.shape) == (K - 3, 4, 8) and bool((alone[..., 0] == 64).all())


@pytest.mark.gpu
def test_band_refusals_with_a_handle():
    """each refusal leaves the outputs untouched"""
    import torch
    from robobee3d_amd.batch import _ptr
    B, K = 128, 4
    m, small = _mpc(B, "float32"), _mpc(64, "float32")
    for h in (m, small):
        h.record_history(K)
        h.reactive_steps(K)
    index = m.group_index(torch.arange(B, device=m.device, dtype=torch.int32) // 64, 2)
    foreign = small.group_index(torch.zeros(64, device=m.device, dtype=torch.int32), 1)
    twin = _mpc(B, "float32")
    twin.record_history(K, out=False)
    twin.reactive_steps(K)
    short = _mpc(B, "float32")
    short.record_history(K)
    short.reactive_steps(K - 1)
    good = m.ensemble_bootstrap(index, reps=10)
    torch.cuda.synchronize()
    assert tuple(good[0].shape) == (K, 2, 8) and good[0][..., 0].tolist() == [[64.0, 64.0]] * K
    for bad, exc in ((dict(index=foreign), ValueError), (dict(index=(index[0], index[1].long())), ValueError), (dict(reps=1), ValueError),
                     (dict(reps=4097), ValueError), (dict(p=1.5), ValueError), (dict(stat="median"), ValueError), (dict(term="e"), ValueError),
                     (dict(probs=()), ValueError), (dict(probs=(1.1,)), ValueError), (dict(levels=()), ValueError), (dict(levels=(-0.1,)), ValueError),
                     (dict(other=small), ValueError), (dict(other=twin), ValueError), (dict(other=short), ValueError), (dict(other=3), ValueError),
                     (dict(first=2, count=3), ValueError), (dict(out=torch.zeros((K, 2, 7), dtype=torch.float64, device=m.device)), ValueError)):
        with pytest.raises(exc):
            m.ensemble_bootstrap(**dict(dict(index=index), **bad))
    with pytest.raises(RuntimeError, match="tau"):
        twin.ensemble_bootstrap(index, term="tau")
    # through the C ABI with a handle: refused, and band, crit, sup and work stay as they were
    hist = m.history()
    canary = lambda *s: torch.full(s, -77.0, dtype=torch.float64, device=m.device)
    band, crit, sup, work = canary(K, 2, 8), canary(2, 2), canary(2, 10), canary(B + 2)
    arr = lambda *v: (C.c_double * len(v))(*v)
    ok = dict(out=_ptr(hist["out"]), ostate=None, oout=None, reftab=None, ref=_ptr(m.ref), count=K, term=0, stat=0, stat_p=0.5, R=10,
              probs=arr(0.05, 0.95), nq=2, levels=arr(0.9), nl=1, crit=_ptr(crit), sup=_ptr(sup), G=2)
    for bad, word in ((dict(R=1), b"R"), (dict(R=4097), b"R"), (dict(stat=3), b"stat"), (dict(stat_p=2.0), b"stat_p"), (dict(nq=0), b"probabilities"),
                      (dict(levels=arr(2.0)), b"levels"), (dict(nl=0), b"levels"), (dict(crit=None), b"crit"), (dict(term=2, out=None), b"out_hist"),
                      (dict(ostate=_ptr(hist["state"])), b"other_out"), (dict(ref=None), b"ref_tab"), (dict(count=-1), b"count"), (dict(G=0), b"G")):
        a = dict(ok, **bad)
        rc = m.L.umpcBatchEnsembleBootstrap(m.h, _ptr(hist["state"]), a["out"], a["ostate"], a["oout"], a["reftab"], a["ref"], 0, a["count"], 0, 0,
                                            _ptr(index[0]), _ptr(index[1]), a["G"], a["term"], a["stat"], a["stat_p"], a["R"], 1, a["probs"],
                                            a["nq"], a["levels"], a["nl"], _ptr(band), a["crit"], a["sup"], _ptr(work), m._stream())
        assert rc == -1 and word in m.L.umpcLastError(), (bad, m.L.umpcLastError())
    torch.cuda.synchronize()
    for t in (band, crit, sup, work):
        assert bool((t == -77.0).all())
