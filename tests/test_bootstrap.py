"""Bootstrap intervals on the device: umpcBatchScoreBootstrap resamples the scored values of every group of a per-robot score R
times, takes a statistic of each resample and condenses the replicates into a point estimate, a standard error and a
percentile interval per group. The numpy mirror (robobee3d_amd/score.py: score_bootstrap_reference) is the definition.
CPU: the hash against batch._u01, the index rule, the mirror by hand, constant cells, the statistical sense of the definition,
exports, refusals without a handle, the resource record of the build.
GPU: exact tables bit for bit on both sides of the 64-value switch, noise tables within the rounding of a sum, independence of
a row from everything but its cell, common random numbers, two calls, one end-to-end MPC-against-reactive sweep, refusals."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U53 = 2.0 ** -53
# scored values per cell: nothing, the smallest cells, both sides of a half and of a whole wavefront (two cells of 64 with the
# SAME values in the same order), the block path at its first size, across one and across the block's 256 threads; then
# the values of cell 8 and of cell 12 once more in another robot order
SCORED = (0, 1, 2, 3, 31, 32, 33, 63, 64, 64, 65, 129, 257, 300, 64, 257)
EXTRA = {1: 1, 4: 2, 8: 3, 10: 1, 13: 2, 15: 1}      # members of a cell that do not enter, on top of the scored ones
G_ = len(SCORED)
B_ = sum(SCORED) + sum(EXTRA.values())
STATS = (("mean", 0.5), ("quantile", 0.0), ("quantile", 0.5), ("quantile", 1.0))
PROBS = (0.025, 0.5, 0.975)


def _same(a, b):
    """equal as doubles bit for bit, but any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def _layout(seed=3):
    """ids [B_]: the robots of every cell scattered over the batch; (ids, members): members[g] = the robots of cell g in
    ascending order -- the member list of group_index"""
    ids = np.concatenate([np.full(n + EXTRA.get(g, 0), g, np.int32) for g, n in enumerate(SCORED)])
    ids = ids[np.random.default_rng(seed).permutation(B_)]
    return ids, [np.nonzero(ids == g)[0] for g in range(G_)]


def _tables(dtype, kind, pair, seed=5):
    """(score, other or None) [12, B_] in `dtype`, with num = 1, den = 0. kind "exact": values k / 8, 0 < |k| < 2^20, a third
    of them from a pool of 12 (ties), row 0 in {1, 2, 4} and row 1 = value * row 0, so that the quotient is the value again and
    every sum of values is exact; kind "noise": signed normal values over row 0 = 1. The members of EXTRA do not enter: row 0
    = 0, a NaN in row 1, and the third either an inf in row 1 or, with `pair`, row 0 = 0 in the OTHER table alone -- the
    same robots with and without `pair`. Cells 9, 14 and 15 hold the values of cells 8, 8 and 12: in the same list order,
    reversed, permuted."""
    from robobee3d_amd import score as S
    rng = np.random.default_rng(seed)
    ids, members = _layout()

    def values(n):
        if kind == "noise":
            return rng.normal(size=n).astype(dtype).astype(np.float64)
        k = rng.integers(1, 1 << 20, n) * rng.choice([-1, 1], n)
        pool = rng.integers(1, 1 << 20, 12) * rng.choice([-1, 1], 12)
        return np.where(rng.random(n) < 1 / 3, rng.choice(pool, n), k) / 8.0

    def table():
        vals = [values(n) for n in SCORED]
        vals[9], vals[14], vals[15] = vals[8].copy(), vals[8][::-1].copy(), vals[12][np.random.default_rng(1).permutation(257)]
        sc = S.score_identity(B_)
        sc[S.STEPS] = 1.0 if kind == "noise" else rng.choice([1.0, 2.0, 4.0], B_)
        drop = []
        for g, mem in enumerate(members):
            out = mem[np.linspace(0, len(mem) - 1, EXTRA.get(g, 0)).astype(int)] if g in EXTRA else mem[:0]
            drop.append(out)
            keep = np.setdiff1d(mem, out)
            assert len(keep) == SCORED[g]
            sc[S.SUM_EP, keep] = vals[g] * sc[S.STEPS, keep]
        return sc, drop
    sc, drop = table()
    ot = table()[0] if pair else None
    for g, out in enumerate(drop):
        for i, b in enumerate(out):
            if i % 3 == 0:
                sc[S.STEPS, b] = 0.0
            elif i % 3 == 1:
                sc[S.SUM_EP, b] = np.nan
            elif pair:
                ot[S.STEPS, b] = 0.0
            else:
                sc[S.SUM_EP, b] = np.inf
    return ids, sc.astype(dtype), (None if ot is None else ot.astype(dtype))


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_bootstrap_hash_is_the_monte_carlo_hash():
    from robobee3d_amd import batch, score as S
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(50000, dtype=np.uint64), (rng.integers(0, 1 << 20, 50000).astype(np.uint64) << np.uint64(32))
                          + rng.integers(0, 1 << 31, 50000).astype(np.uint64)])
    for seed, salt in ((0, 41), (7, 41), (2 ** 63 + 12345, 3), (123456789, 14)):
        a, b = S.bootstrap_u01(seed, idx, salt), batch._u01(seed, idx, salt)
        assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert a.min() >= 0.0 and a.max() < 1.0
    assert S.BOOT_SALT == 41


def test_bootstrap_indices_stay_in_range_and_cover_the_cell():
    from robobee3d_amd import score as S
    for nsc in (1, 2, 3, 63, 64, 65, 200):
        for seed in (0, 1, 99):
            j = S.bootstrap_indices(nsc, 1000, seed)
            assert j.shape == (1000, nsc) and j.min() >= 0 and j.max() <= nsc - 1
            idx = (np.arange(1000, dtype=np.uint64)[:, None] << np.uint64(32)) + np.arange(nsc, dtype=np.uint64)[None]
            u = S.bootstrap_u01(seed, idx, 41)
            assert np.floor(u * nsc).max() < nsc                       # the clamp never acts on these; it is there for u -> 1
            assert np.array_equal(j, np.floor(u * nsc).astype(np.int64))
    # the draw is a function of (seed, r, m, nsc): more replicates only append rows
    assert np.array_equal(S.bootstrap_indices(64, 1000, 0)[:10], S.bootstrap_indices(64, 10, 0))
    counts = np.bincount(S.bootstrap_indices(64, 1000, 0).ravel(), minlength=64)
    print("draws per member, R = 1000, nsc = 64, seed 0: min %d max %d" % (counts.min(), counts.max()))
    # 1000 expected, binomial sigma 31.4: five sigma either way
    assert counts.sum() == 64000 and counts.min() > 1000 - 157 and counts.max() < 1000 + 157


def _one_cell(values, steps=None, other=None, other_steps=None):
    """a score [12, n] with row 1 = values and row 0 = steps (1 where not given), one group of all robots"""
    from robobee3d_amd import score as S
    n = len(values)
    sc = S.score_identity(n)
    sc[S.SUM_EP], sc[S.STEPS] = values, 1.0 if steps is None else steps
    ot = None
    if other is not None:
        ot = S.score_identity(n)
        ot[S.SUM_EP], ot[S.STEPS] = other, 1.0 if other_steps is None else other_steps
    return sc, ot, np.arange(n, dtype=np.int32), np.array([0, n], np.int32)


def test_bootstrap_mirror_by_hand():
    from robobee3d_amd import score as S
    assert (S.BOOT_N, S.BOOT_SKIPPED, S.BOOT_POINT, S.BOOT_MEAN, S.BOOT_SE, S.BOOT_FIRST) == (0, 1, 2, 3, 4, 5)
    R = 9
    # nsc = 1: every replicate is the value, whatever the statistic
    sc, _, order, offset = _one_cell([2.5])
    for stat in ("mean", "quantile"):
        boot, reps = S.score_bootstrap_reference(sc, order, offset, 1, stat=stat, reps=R, probs=(0.0, 1.0))
        assert reps.tolist() == [[2.5] * R] and boot.tolist() == [[1, 0, 2.5, 2.5, 0.0, 2.5, 2.5]]
    # nsc = 2 and 3: the replicate table written out from the index table
    for vals in ([1.0, 4.0], [1.0, -2.0, 4.0]):
        n = len(vals)
        sc, _, order, offset = _one_cell(vals)
        J = S.bootstrap_indices(n, R, 5)
        assert J.shape == (R, n) and len({tuple(j) for j in J.tolist()}) > 1
        means = [sum(vals[j] for j in row) / n for row in J.tolist()]            # (small dyadic values: the sums are exact)
        lows = [sorted(vals[j] for j in row)[S.quantile_rank(0.5, n)] for row in J.tolist()]
        for stat, want, point in (("mean", means, sum(vals) / n), ("quantile", lows, sorted(vals)[S.quantile_rank(0.5, n)])):
            boot, reps = S.score_bootstrap_reference(sc, order, offset, 1, stat=stat, p=0.5, reps=R, seed=5, probs=(0.0, 0.5, 1.0))
            assert reps.tolist() == [want]
            mean = math.fsum(want) / R
            assert boot[0, :4].tolist() == [n, 0, point, mean]
            assert boot[0, 4] == math.sqrt(math.fsum((t - mean) ** 2 for t in want) / (R - 1))
            assert boot[0, 5:].tolist() == [min(want), sorted(want)[4], max(want)]
    # the quotient, an empty cell, members that do not enter: row 0 = 0, a NaN value, an inf quotient's numerator
    sc = S.score_identity(7)
    sc[S.STEPS] = [2, 0, 2, 2, 4, 2, 2]
    sc[S.SUM_EP] = [3.0, 1.0, np.nan, np.inf, 2.0, 5.0, 7.0]
    order, offset = S.group_index_reference(np.array([0, 0, 0, 0, 0, 2, 2], np.int32), 3)
    boot, reps = S.score_bootstrap_reference(sc, order, offset, S.SUM_EP, S.STEPS, reps=4, probs=(0.5,))
    assert boot.shape == (3, 6) and reps.shape == (3, 4)
    assert boot[0, :3].tolist() == [2, 3, 1.0] and boot[2, :3].tolist() == [2, 0, 3.0]          # (1.5 + 0.5) / 2, (2.5 + 3.5) / 2
    assert set(reps[0].tolist()) <= {0.5, 1.0, 1.5} and set(reps[2].tolist()) <= {2.5, 3.0, 3.5}
    assert boot[1, :2].tolist() == [0, 0] and np.isnan(boot[1, 2:]).all() and np.isnan(reps[1]).all()
    # with other=: a robot missing in either table is skipped in the pair, and the value is the difference
    sc, ot, order, offset = _one_cell([5.0, 6.0, 7.0, 8.0], [1, 1, 0, 1], other=[1.0, 1.0, 1.0, 4.0], other_steps=[1, 0, 1, 1])
    boot, reps = S.score_bootstrap_reference(sc, order, offset, 1, other=ot, reps=6, probs=(0.0, 1.0))
    assert boot[0, :3].tolist() == [2, 2, 4.0] and set(reps[0].tolist()) <= {4.0}               # 5 - 1 and 8 - 4
    x, ok = S.score_bootstrap_values(sc, 1, None, ot)
    assert ok.tolist() == [True, False, False, True] and x[[0, 3]].tolist() == [4.0, 4.0]
    # the total order: -0 sorts before +0
    sc, _, order, offset = _one_cell([0.0, -0.0, 0.0])
    boot, _ = S.score_bootstrap_reference(sc, order, offset, 1, stat="quantile", p=0.0, reps=2)
    assert math.copysign(1.0, boot[0, 2]) == -1.0
    boot, _ = S.score_bootstrap_reference(sc, order, offset, 1, stat="quantile", p=0.5, reps=2)
    assert math.copysign(1.0, boot[0, 2]) == 1.0
    for bad in (dict(stat="median"), dict(p=1.5), dict(p=-0.1), dict(reps=1), dict(reps=(1 << 20) + 1), dict(probs=()),
                dict(probs=(0.5,) * 9), dict(probs=(1.5,)), dict(num=12), dict(den=-2)):
        with pytest.raises(ValueError):
            S.score_bootstrap_reference(sc, order, offset, **dict(dict(num=1), **bad))


def test_a_constant_cell_has_constant_replicates():
    """n x c is exact for an fp32-representable c and n <= 64 (24 + 6 <= 53 bits), and so is the division"""
    from robobee3d_amd import score as S
    for n in range(1, 65):
        c = float(np.float32(0.1 * n - 3.3))
        sc, _, order, offset = _one_cell([c] * n)
        boot, reps = S.score_bootstrap_reference(sc, order, offset, 1, reps=50, seed=n)
        assert np.all(reps == c) and boot[0].tolist() == [n, 0, c, c, 0.0, c, c]


def test_the_standard_error_of_the_mean_is_the_textbook_one():
    """the mirror's SE of the mean against s / sqrt(n) * sqrt((n - 1) / n) (the plug-in variance the bootstrap estimates) within
    10 %, and the mean of the replicates within 4 SE / sqrt(R) of the sample mean: R = 2000, seeds 0..11, n in {16, 64, 200},
    three distributions rounded to fp32, all as cells of one call per seed"""
    from robobee3d_amd import score as S
    R, sizes = 2000, (16, 64, 200)
    worst = 0.0
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        vals = [d(n).astype(np.float32).astype(np.float64) for n in sizes
                for d in (lambda n: rng.normal(size=n), lambda n: rng.lognormal(size=n), lambda n: rng.uniform(size=n))]
        sc, _, _, _ = _one_cell(np.concatenate(vals))
        offset = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int32)
        boot, _ = S.score_bootstrap_reference(sc, np.arange(offset[-1], dtype=np.int32), offset, 1, reps=R, seed=seed)
        for g, v in enumerate(vals):
            n = len(v)
            se = v.std(ddof=1) / math.sqrt(n) * math.sqrt((n - 1) / n)
            worst = max(worst, abs(boot[g, S.BOOT_SE] / se - 1))
            assert abs(boot[g, S.BOOT_SE] / se - 1) < 0.10, (seed, g, boot[g, S.BOOT_SE], se)
            assert abs(boot[g, S.BOOT_MEAN] - boot[g, S.BOOT_POINT]) < 4 * boot[g, S.BOOT_SE] / math.sqrt(R), (seed, g)
            assert boot[g, S.BOOT_POINT] == math.fsum(v.tolist()) / n
            assert boot[g, 5] < boot[g, S.BOOT_POINT] < boot[g, 6]
    print("worst SE against the textbook figure: %.1f %%" % (100 * worst))


def _fake(n=64):
    """an address that is never read: the refusals come before any HIP call"""
    buf = (C.c_double * n)()
    return buf, C.c_void_p(C.addressof(buf))


def test_bootstrap_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib, score as S
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read())
    decls = ("#define UMPC_BOOT_MEAN 0", "#define UMPC_BOOT_QUANTILE 1",
             "#define UMPC_BOOT_ROWS 5 /* columns ahead of the percentile columns */", "#define UMPC_BOOT_MAX_REPS 1048576",
             "int umpcBatchScoreBootstrap(umpc_batch_t *h, const void *score, const void *other, int num, int den, "
             "const int32_t *order, const int32_t *offset, int G, int stat, double stat_p, "
             "int R, unsigned long long seed, const double *probs, int nq, "
             "double *boot, double *reps, double *work, void *stream);")
    at = [flat.index(d) for d in decls]
    assert at == sorted(at)
    assert flat.index("int umpcBatchScoreQuantiles(") < at[0] and at[-1] < flat.index("int umpcBatchSetStepKernel")
    assert (_lib.BOOT_MEAN, _lib.BOOT_QUANTILE, _lib.BOOT_ROWS, _lib.BOOT_MAX_REPS) == (0, 1, 5, 1 << 20)
    assert S.BOOT_STATS == ("mean", "quantile") and S.BOOT_MAX_REPS == 1 << 20
    L = _lib.lib()
    assert "umpcBatchScoreBootstrap" in _lib.EXPORTS and L.umpcBatchScoreBootstrap
    vp = C.c_void_p
    assert L.umpcBatchScoreBootstrap.argtypes == [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int,
                                                  C.c_ulonglong, C.POINTER(C.c_double), C.c_int, vp, vp, vp, vp]
    # argument checks come before any HIP call and the handle is looked at last: every refusal is met without a device
    keepalive, p = _fake()
    arr = lambda *v: (C.c_double * len(v))(*v)
    ok = dict(score=p, other=None, num=1, den=0, order=p, offset=p, G=1, stat=0, stat_p=0.5, R=100, seed=3, probs=arr(0.025, 0.975),
              nq=2, boot=p, reps=p, work=p)

    def call(**bad):
        a = dict(ok, **bad)
        rc = L.umpcBatchScoreBootstrap(None, a["score"], a["other"], a["num"], a["den"], a["order"], a["offset"], a["G"], a["stat"],
                                       a["stat_p"], a["R"], a["seed"], a["probs"], a["nq"], a["boot"], a["reps"], a["work"], None)
        return rc, L.umpcLastError()
    rc, err = call()
    assert rc == -1 and b"umpcBatchScoreBootstrap" in err and b"handle" in err                    # all good but the handle
    for bad, word in ((dict(R=1), b"R"), (dict(R=0), b"R"), (dict(R=-5), b"R"), (dict(R=(1 << 20) + 1), b"R"), (dict(stat=2), b"stat"),
                      (dict(stat=-1), b"stat"), (dict(stat_p=1.5), b"stat_p"), (dict(stat_p=-0.1), b"stat_p"),
                      (dict(stat_p=float("nan")), b"stat_p"), (dict(nq=0), b"probabilities"), (dict(nq=9, probs=arr(*[0.5] * 9)), b"probabilities"),
                      (dict(probs=arr(0.5, 1.5)), b"probabilities"), (dict(probs=arr(float("nan"), 0.5)), b"probabilities"),
                      (dict(probs=None), b"probs"), (dict(num=-1), b"num"), (dict(num=12), b"num"), (dict(den=-2), b"den"),
                      (dict(den=12), b"den"), (dict(boot=None), b"boot"), (dict(reps=None), b"reps"), (dict(work=None), b"work"),
                      (dict(score=None), b"score"), (dict(order=None), b"order"), (dict(offset=None), b"offset"), (dict(G=0), b"G")):
        rc, err = call(**bad)
        assert rc == -1 and b"umpcBatchScoreBootstrap" in err and word in err and b"handle" not in err, (bad, err)
    assert L.umpcBatchScoreBootstrap(None, *([None] * 2), 1, 0, None, None, 1, 0, 0.5, 100, 0, None, 2, None, None, None, None) == -1
    assert b"umpcBatchScoreBootstrap" in L.umpcLastError()
    del keepalive


def test_bootstrap_kernels_use_no_scratch():
    """the resource remarks of the build: every form of the five bootstrap kernels has no private frame and the static LDS that
    its entry of csrc/resource_limits.json states; a form with a frame is refused"""
    import json
    from robobee3d_amd import _lib
    _lib.build()
    res = json.load(open(_lib.RESOURCES_JSON))
    limits = json.load(open(_lib.RESOURCE_LIMITS))
    forms = {"umpc_boot_compact_kernel": (4, 0), "umpc_boot_rep_kernel": (2, 0), "umpc_boot_mean_block_kernel": (1, 2048),
             "umpc_boot_quantile_block_kernel": (1, 8440), "umpc_boot_row_kernel": (1, 12536)}
    assert {k for k in limits if "boot" in k} == set(forms)
    for pat, (n, lds) in forms.items():
        hits = [k for k in res if pat in k]
        assert len(hits) == n, (pat, hits)
        for k in hits:
            assert res[k]["ScratchSize"] == 0 and res[k]["LDS"] == lds, (k, res[k])
        assert {f: x for f, x in limits[pat].items() if f != "_note"} == {"ScratchSize": 0, "LDS": lds}
        with pytest.raises(RuntimeError, match=pat):
            _lib._validate_resources(dict(res, **{"a_form_of_%s_with_a_frame" % pat: {"ScratchSize": 8, "LDS": lds}}))
    assert len([k for k in res if "umpc_boot" in k]) == 9
    for older in ("umpc_score_quantile_kernel", "umpc_ens_quantile", "umpc_ensemble_kernel"):
        assert not [k for k in res if "umpc_boot" in k and older in k]


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


def _boot(m, score, other, num, den, index, stat, p, R, seed, probs):
    """umpcBatchScoreBootstrap through the C ABI; boot, reps and work are filled with a canary first: what the call did not
    write shows"""
    import torch
    from robobee3d_amd.batch import _ptr
    order, offset = index
    G = offset.numel() - 1
    boot = torch.full((G, 5 + len(probs)), -77.0, dtype=torch.float64, device=m.device)
    reps = torch.full((G, R), -77.0, dtype=torch.float64, device=m.device)
    work = torch.full((m.B + G,), -77.0, dtype=torch.float64, device=m.device)
    rc = m.L.umpcBatchScoreBootstrap(m.h, _ptr(score), _ptr(other), num, den, _ptr(order), _ptr(offset), G, ("mean", "quantile").index(stat),
                                     p, R, seed, (C.c_double * len(probs))(*probs), len(probs), _ptr(boot), _ptr(reps), _ptr(work),
                                     m._stream())
    assert rc == 0, m.L.umpcLastError()
    return boot.cpu().numpy(), reps.cpu().numpy()


def _sample_abs_sums(x, ok, order, offset, R, seed):
    """per cell [R]: sum |v[j]| over the slots of every replicate (NaN row for an empty cell), and sum |v| of the cell"""
    from robobee3d_amd import score as S
    G = len(offset) - 1
    sums, own = np.full((G, R), np.nan), np.full(G, np.nan)
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        v = np.abs(x[mem[ok[mem]]])
        if len(v):
            sums[g], own[g] = v[S.bootstrap_indices(len(v), R, seed)].sum(1), v.sum()
    return sums, own


@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 64, 65, 1000])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_exact_tables_bit_for_bit(dtype, R):
    """16 cells with 0 .. 300 scored values k / 8 (|k| < 2^20, no zero) as a quotient over row 0 in {1, 2, 4}: every sum of
    values is exact, so reps and boot are the mirror's bit for bit in both statistics and both cell-size paths, with and
    without a second table. The replicates of the MEAN of a cell whose count is no power of two are rounded quotients, their
    sum is not exact in general: the kernel accumulates it in double-double and the test holds it to the fsum of the mirror
    all the same. The standard error (squares: not exact) at 1e-9 relative."""
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    for pair, stats in ((False, STATS), (True, STATS[:1] + STATS[2:3])):
        ids, sc, ot = _tables(np.dtype(dtype), "exact", pair)
        x, ok = S.score_bootstrap_values(sc, 1, 0, ot)
        assert np.all(x[ok] * 8 == np.round(x[ok] * 8)) and (pair or not np.any(x[ok] == 0))
        order, offset = S.group_index_reference(ids, G_)
        index = m.group_index(_dev(m, ids), G_)
        dsc, dot = _dev(m, sc), _dev(m, ot)
        for stat, p in stats:
            boot, reps = _boot(m, dsc, dot, 1, 0, index, stat, p, R, 11, PROBS)
            wboot, wreps = S.score_bootstrap_reference(sc, order, offset, 1, 0, other=ot, stat=stat, p=p, reps=R, seed=11, probs=PROBS)
            assert wboot[:, 0].tolist() == list(SCORED) and wboot[:, 1].tolist() == [EXTRA.get(g, 0) for g in range(G_)]
            tag = (pair, stat, p)
            assert _same(reps, wreps), (tag, np.argwhere(reps != wreps)[:5])
            cols = [c for c in range(boot.shape[1]) if c != S.BOOT_SE]
            assert _same(boot[:, cols], wboot[:, cols]), (tag, boot[:, cols] - wboot[:, cols])
            se, wse = boot[1:, S.BOOT_SE], wboot[1:, S.BOOT_SE]
            assert np.isnan(boot[0, S.BOOT_SE]) and np.all(np.abs(se - wse) <= 1e-9 * wse), (tag, se, wse)
            assert se[0] == 0.0                                                        # the cell of one value
            # the same values in another robot order: the same point estimate (exact sums), other replicates
            assert boot[14, 2] == boot[8, 2] and boot[15, 2] == boot[12, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("R", [64, 1000])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_noise_tables_within_the_rounding_of_a_sum(dtype, R, margin):
    """signed normal values (as an other= difference gives them). Quantile statistic: an element, bit for bit. Mean: a replicate
    within (nsc + 1) 2^-53 sum|sample| / nsc of the fsum mirror (any order of summation, and the one division); the
    percentile columns within that bound taken over the cell (an order statistic is 1-Lipschitz in the sup norm); the mean of
    the replicates within it plus the (R + 1) 2^-53 mean|t| of its own sum; the standard error within it times sqrt(R / (R -
    1)) (the norm of the centred replicates moves by no more than the norm of their change) plus 1e-9 relative."""
    from robobee3d_amd import score as S
    m = _mpc(B_, dtype)
    for pair in (False, True):
        ids, sc, ot = _tables(np.dtype(dtype), "noise", pair)
        order, offset = S.group_index_reference(ids, G_)
        index = m.group_index(_dev(m, ids), G_)
        dsc, dot = _dev(m, sc), _dev(m, ot)
        den = None if pair else 0                                                     # (row 0 = 1: the quotient changes nothing)
        for stat, p in (("quantile", 0.5), ("quantile", 0.9)):
            boot, reps = _boot(m, dsc, dot, 1, -1 if den is None else den, index, stat, p, R, 4, PROBS)
            wboot, wreps = S.score_bootstrap_reference(sc, order, offset, 1, den, other=ot, stat=stat, p=p, reps=R, seed=4, probs=PROBS)
            cols = [c for c in range(boot.shape[1]) if c != S.BOOT_SE]
            assert _same(reps, wreps) and _same(boot[:, cols], wboot[:, cols]), (pair, stat, p)
            assert np.all(np.abs(boot[1:, 4] - wboot[1:, 4]) <= 1e-9 * wboot[1:, 4])
        boot, reps = _boot(m, dsc, dot, 1, -1 if den is None else den, index, "mean", 0.5, R, 4, PROBS)
        wboot, wreps = S.score_bootstrap_reference(sc, order, offset, 1, den, other=ot, reps=R, seed=4, probs=PROBS)
        x, ok = S.score_bootstrap_values(sc, 1, den, ot)
        sums, own = _sample_abs_sums(x, ok, order, offset, R, 4)
        nsc = wboot[:, 0]
        assert np.array_equal(boot[:, :2], wboot[:, :2]) and np.isnan(boot[0, 2:]).all() and np.isnan(reps[0]).all()
        live = nsc > 0
        assert not np.isnan(reps[live]).any() and not np.isnan(boot[live]).any()
        bound = (nsc[:, None] + 1) * U53 * sums / np.maximum(nsc[:, None], 1)         # [G, R]
        cell = bound.max(1)
        worst = {"replicates": np.nanmax(np.abs(reps - wreps)[live] / bound[live]),
                 "point estimate": np.max(np.abs(boot[live, 2] - wboot[live, 2]) / ((nsc + 1) * U53 * own / np.maximum(nsc, 1))[live]),
                 "percentile columns": np.max(np.abs(boot[live, 5:] - wboot[live, 5:]) / cell[live, None]),
                 "mean of the replicates": np.max(np.abs(boot[live, 3] - wboot[live, 3])
                                                  / (cell + (R + 1) * U53 * np.abs(wreps).mean(1))[live]),
                 "standard error": np.max(np.abs(boot[live, 4] - wboot[live, 4])
                                          / (cell * math.sqrt(R / (R - 1.0)) + 1e-9 * wboot[:, 4])[live])}
        for what, ratio in worst.items():
            margin("%s%s %s / bound" % ("pair " if pair else "", dtype, what), float(ratio), 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_row_depends_on_its_cell_alone_and_equal_cells_share_their_draws(dtype):
    """cells 3 (3 values), 8 (64 scored of 67 members), 11 (129) and 13 (300 of 302) keep the bits of their boot and reps rows
    when the groups are re-numbered, G grows and the other cells' robots are dealt out differently or ignored; two calls with
    the same arguments are bit-identical; cells 8 and 9 (the same values in the same list order) have bit-identical
    replicates, and cell 14 (the same values reversed) has not"""
    from robobee3d_amd import score as S
    ids, sc, ot = _tables(np.dtype(dtype), "noise", True)
    m = _mpc(B_, dtype)
    dsc, dot = _dev(m, sc), _dev(m, ot)
    index = m.group_index(_dev(m, ids), G_)
    watch = (3, 8, 11, 13)
    to = {3: 0, 8: 19, 11: 7, 13: 4}
    rng = np.random.default_rng(2)
    rest = ~np.isin(ids, watch)
    ids2 = ids.copy()
    ids2[rest] = rng.choice([1, 2, 3, 5, 6, 8, -1, 20], int(rest.sum()))
    for g, h in to.items():
        ids2[ids == g] = h
    index2 = m.group_index(_dev(m, ids2), 20)
    for stat, p in (("mean", 0.5), ("quantile", 0.5)):
        for R in (65, 1000):
            boot, reps = _boot(m, dsc, dot, 1, -1, index, stat, p, R, 9, PROBS)
            again = _boot(m, dsc, dot, 1, -1, index, stat, p, R, 9, PROBS)
            assert _same(boot, again[0]) and _same(reps, again[1])
            assert not np.any(boot == -77.0) and not np.any(reps == -77.0)
            boot2, reps2 = _boot(m, dsc, dot, 1, -1, index2, stat, p, R, 9, PROBS)
            assert boot2.shape == (20, 8) and reps2.shape == (20, R)
            for g, h in to.items():
                assert _same(boot[g], boot2[h]) and _same(reps[g], reps2[h]), (stat, R, g)
            assert boot[8, 0] == 64 and boot[8, 1] == 3 and _same(reps[8], reps[9]) and _same(boot[8, 2:], boot[9, 2:])
            assert not _same(reps[8], reps[14])
            # another seed is another table
            assert not _same(reps[8], _boot(m, dsc, dot, 1, -1, index, stat, p, R, 10, PROBS)[1][8])


@pytest.mark.gpu
def test_end_to_end_mpc_minus_reactive_per_cell(margin):
    """B = 256 as 4 contiguous cells of 64 Monte-Carlo draws, 20 closed-loop steps of rollout() and of reactive_steps() from the
    same start, each scored on the device; score_bootstrap(mpc_score, index, num=1, den=0, other=reactive_score) against the
    mirror on the downloaded scores: bit for bit in the quantile statistic, within the bound of a sum in the mean. Nothing is
    asserted about which controller wins."""
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import hover_initial_conditions
    B, K, R = 256, 20, 200
    st, ref = hover_initial_conditions(B, 7, np.float32, tilt=0.3)
    scores = []
    for use_mpc in (True, False):
        m = _mpc(B, "float32")
        m.set_state(st, ref)
        m.record_history(K, status=True)
        m.rollout(K) if use_mpc else m.reactive_steps(K)
        scores.append(m.score(after=True))
    cell = (np.arange(B) // 64).astype(np.int32)
    index = m.group_index(cell, 4)
    order, offset = S.group_index_reference(cell, 4)
    sm, sr = (s.cpu().numpy() for s in scores)
    for stat in S.BOOT_STATS:
        boot, reps = m.score_bootstrap(scores[0], index, num=1, den=0, other=scores[1], stat=stat, reps=R, seed=1, return_reps=True)
        assert boot.dtype == torch.float64 and tuple(boot.shape) == (4, 7) and tuple(reps.shape) == (4, R)
        only = m.score_bootstrap(scores[0], index, num=1, den=0, other=scores[1], stat=stat, reps=R, seed=1)
        assert torch.equal(only.view(torch.int64), boot.view(torch.int64))
        boot, reps = boot.cpu().numpy(), reps.cpu().numpy()
        wboot, wreps = S.score_bootstrap_reference(sm, order, offset, 1, 0, other=sr, stat=stat, reps=R, seed=1)
        assert np.all(wboot[:, 0] == 64) and np.all(wboot[:, 1] == 0)
        print(stat, "MPC - reactive per cell: point, interval\n", boot[:, [2, 5, 6]])
        if stat == "quantile":
            assert _same(boot[:, :4], wboot[:, :4]) and _same(boot[:, 5:], wboot[:, 5:]) and _same(reps, wreps)
            assert np.all(np.abs(boot[:, 4] - wboot[:, 4]) <= 1e-9 * wboot[:, 4])
        else:
            x, ok = S.score_bootstrap_values(sm, 1, 0, sr)
            sums, own = _sample_abs_sums(x, ok, order, offset, R, 1)
            bound = 65 * U53 * sums / 64
            cellb = bound.max(1)
            margin("end to end replicates / bound", float(np.max(np.abs(reps - wreps) / bound)), 1.0)
            margin("end to end point / bound", float(np.max(np.abs(boot[:, 2] - wboot[:, 2]) / (65 * U53 * own / 64))), 1.0)
            margin("end to end percentiles / bound", float(np.max(np.abs(boot[:, 5:] - wboot[:, 5:]) / cellb[:, None])), 1.0)
            margin("end to end mean / bound", float(np.max(np.abs(boot[:, 3] - wboot[:, 3])
                                                          / (cellb + (R + 1) * U53 * np.abs(wreps).mean(1)))), 1.0)
            margin("end to end SE / bound", float(np.max(np.abs(boot[:, 4] - wboot[:, 4])
                                                        / (cellb * math.sqrt(R / (R - 1.0)) + 1e-9 * wboot[:, 4]))), 1.0)
        assert np.all(boot[:, 5] <= boot[:, 6])


@pytest.mark.gpu
def test_bootstrap_refusals_with_a_handle():
    import torch
    m, other_handle = _mpc(128, "float32"), _mpc(64, "float32")
    score = torch.ones((12, 128), device=m.device)
    index = m.group_index(torch.arange(128, device=m.device, dtype=torch.int32) // 64, 2)
    foreign = other_handle.group_index(torch.zeros(64, device=m.device, dtype=torch.int32), 1)
    good = m.score_bootstrap(score, index, 1, 0, other=score.clone(), reps=10)
    torch.cuda.synchronize()
    assert good[:, :5].tolist() == [[64.0, 0.0, 0.0, 0.0, 0.0]] * 2                  # 1 / 1 - 1 / 1 in every draw
    for bad in (dict(score=score[:, :-1]), dict(score=score[:11]), dict(score=score.double()), dict(score=score.cpu()),
                dict(score=score.t().contiguous().t()), dict(other=score[:, :-1]), dict(other=score.double()), dict(other=score.cpu()),
                dict(index=foreign), dict(index=(index[0], index[1].long())), dict(reps=1), dict(reps=(1 << 20) + 1), dict(p=1.5),
                dict(p=-0.5), dict(stat="median"), dict(probs=()), dict(probs=(0.5,) * 9), dict(probs=(1.1,)), dict(probs=(-0.1, 0.5))):
        kw = dict(dict(score=score, index=index, num=1, den=0), **bad)
        with pytest.raises(ValueError):
            m.score_bootstrap(**kw)
    with pytest.raises(RuntimeError, match="umpcBatchScoreBootstrap"):
        m.score_bootstrap(score, index, 12)
