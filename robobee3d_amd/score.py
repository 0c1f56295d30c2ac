"""Scores of recorded rollouts: the row names of umpcBatchScore / umpcBatchScoreGroups (include/umpc_mi355x.h) and their
numpy fp64 mirrors. The device path is BatchUprightMPC.score / score_groups (batch.py); nothing here touches a device, and
the mirrors are the definition the kernels are tested against, not a fallback. The same holds for the ensemble rows of
umpcBatchGroupIndex / umpcBatchEnsemble (BatchUprightMPC.group_index / ensemble) and for the order statistics of
umpcBatchEnsembleQuantiles / umpcBatchScoreQuantiles (ensemble_quantiles / score_quantiles), the bootstrap of
umpcBatchScoreBootstrap (score_bootstrap) and the bootstrap bands of umpcBatchEnsembleBootstrap (ensemble_bootstrap) further down,
and for the moments, ellipsoids and Mahalanobis scores of umpcBatchDispersion / umpcBatchDispersionEllipsoids /
umpcBatchMahalanobis (dispersion / dispersion_ellipsoids / mahalanobis), the propagators, the binned sums and
correlation ratios of umpcBatchFactorBins / umpcBatchSensitivity / umpcBatchSensitivityIndices / umpcBatchScoreSensitivity
(factor_bins / sensitivity / sensitivity_indices / score_sensitivity) and, at the end, the projections, periodograms and
per-group spectra of umpcBatchSpectrum / umpcBatchSpectrumPower / umpcBatchSpectrumGroups (spectrum / spectrum_groups), and
the Gram matrices, trajectory modes and weighted sums of umpcBatchGram / umpcBatchProject (trajectory_gram / trajectory_modes /
trajectory_table / ensemble_projection).

A score [12, B] condenses what every closed-loop step of a run did against its reference; a group table [G, 8] condenses the
scores of the robots of each group -- the draws of one grid cell of a gain sweep, the end of the reference's gainTuningSims
(costs[i,j], efforts[i,j] = logMetric(log), template/uprightmpc2.py:272-303). An ensemble [count, G, 16] keeps the steps
apart instead and reduces over the robots of each group: the cell's y(t) against pdes(t) figure (uprightmpc2.py:177-269) as
mean, spread, envelope and the share of draws outside the tube, per step."""
import math

import numpy as np

SCORE_ROWS, GSCORE_ROWS = 12, 8
# score rows
(STEPS, SUM_EP, MAX_EP, LAST_EP, SUM_ES, MAX_ES, SUM_TAU2, SUM_P2, NOT_SOLVED, FIRST_OVER, LAST_OVER, SKIPPED) = range(12)
SCORE_ROW_NAMES = ("steps", "sum_ep", "max_ep", "last_ep", "sum_es", "max_es", "sum_tau2", "sum_p2", "not_solved",
                   "first_over", "last_over", "skipped")
# group rows
(G_ROBOTS, G_SCORED, G_SUM_MEAN_EP, G_MAX_EP, G_SUM_MEAN_TAU2, G_SUM_MEAN_P2, G_LEFT, G_NOT_SOLVED) = range(8)
GSCORE_ROW_NAMES = ("robots", "scored", "sum_mean_ep", "max_ep", "sum_mean_tau2", "sum_mean_p2", "left", "not_solved")
OSQP_SOLVED = 1
# ensemble rows, per (step, group)
ENS_ROWS = 16
(E_N, E_SKIPPED, E_SUM_EP, E_SUM_EP2, E_MAX_EP, E_MIN_EP, E_SUM_ES, E_MAX_ES, E_SUM_TAU2, E_MAX_TAU2, E_OVER, E_NOT_SOLVED,
 E_SUM_DX, E_SUM_DY, E_SUM_DZ, E_ARGMAX_EP) = range(16)
ENS_ROW_NAMES = ("n", "skipped", "sum_ep", "sum_ep2", "max_ep", "min_ep", "sum_es", "max_es", "sum_tau2", "max_tau2", "over",
                 "not_solved", "sum_dx", "sum_dy", "sum_dz", "argmax_ep")
ENS_ADD_ROWS = (E_N, E_SKIPPED, E_SUM_EP, E_SUM_EP2, E_SUM_ES, E_SUM_TAU2, E_OVER, E_NOT_SOLVED, E_SUM_DX, E_SUM_DY, E_SUM_DZ)
ENS_MAX_ROWS = (E_MAX_EP, E_MAX_ES, E_MAX_TAU2)
# quantile rows, per (step, group) or per group: members that enter, members that do not, then one row per probability
Q_N, Q_SKIPPED, Q_FIRST = 0, 1, 2
QUANT_MAX_PROBS = 8
TERM_EP, TERM_ES, TERM_TAU = 0, 1, 2
TERM_NAMES = ("ep", "es", "tau")
# bootstrap rows, per group: members that enter, members that do not, the statistic of the cell's own values, the mean and
# the standard error of the replicates, then one row per probability (the percentile interval)
BOOT_N, BOOT_SKIPPED, BOOT_POINT, BOOT_MEAN, BOOT_SE, BOOT_FIRST = 0, 1, 2, 3, 4, 5
BOOT_STATS = ("mean", "quantile")      # UMPC_BOOT_MEAN, UMPC_BOOT_QUANTILE
BOOT_MAX_REPS = 1 << 20
BOOT_SALT = 41


def score_identity(B, dtype=np.float64):
    """The score no step has entered (umpcBatchScoreInit): rows 9 and 10 = -1, all others 0."""
    s = np.zeros((SCORE_ROWS, int(B)), dtype)
    s[FIRST_OVER] = s[LAST_OVER] = -1
    return s


def _step_terms(y, o, r, tl):
    """What one step contributes, per robot: (ok, d, ep, es, p2, tau2) from the state slice y [18, B], the out slice o [9, B] or
    None, the reference slice r [9, B] and taulim. ok: every word the step reads is finite; d = p - pdes [3, B], ep = |d|^2,
    es = |s - sdes|^2, p2 = |p|^2, tau2 = the moments squared, clipped at +-taulim (zeros without an out slice)."""
    p, s, pdes, sdes = y[0:3], y[9:12], r[0:3], r[6:9]
    ok = np.isfinite(p).all(0) & np.isfinite(s).all(0) & np.isfinite(pdes).all(0) & np.isfinite(sdes).all(0)
    if o is not None:
        ok &= np.isfinite(o[1:3]).all(0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - pdes
        ep = (d ** 2).sum(0)
        es = ((s - sdes) ** 2).sum(0)
        p2 = (p ** 2).sum(0)
        tau2 = (np.clip(o[1:3], -tl, tl) ** 2).sum(0) if o is not None else np.zeros_like(ep)
    return ok, d, ep, es, p2, tau2


def score_reference(state_hist, out_hist, status_hist, ref, first, count, ref_first, step0, tol_p, after, taulim, score=None):
    """umpcBatchScore in numpy fp64, step by step in order. state_hist [.., 18, B], out_hist [.., 9, B] or None, status_hist
    [.., B] or None are taken as given; ref is a table [.., 9, B] (slice ref_first + i) or one constant reference [9, B].
    Step c = first + i reads state slice c + after, out / status slice c, and carries the step number k = step0 + i.
    Returns the score [12, B] (float64); passing one back in accumulates."""
    st = np.asarray(state_hist, np.float64)
    B = st.shape[-1]
    out = None if out_hist is None else np.asarray(out_hist, np.float64)
    stat = None if status_hist is None else np.asarray(status_hist)
    ref = np.asarray(ref, np.float64)
    first, count, ref_first, step0, after = int(first), int(count), int(ref_first), int(step0), int(bool(after))
    if count < 0 or first < 0 or ref_first < 0 or not (tol_p >= 0 and np.isfinite(tol_p)):
        raise ValueError("score_reference: bad argument")
    sc = score_identity(B) if score is None else np.array(score, np.float64)
    tol2, tl = float(tol_p) ** 2, float(taulim)
    for i in range(count):
        c, k = first + i, step0 + i
        ok, _, ep, es, p2, tau2 = _step_terms(st[c + after], None if out is None else out[c],
                                              ref[ref_first + i] if ref.ndim == 3 else ref, tl)
        sc[SKIPPED] += ~ok
        sc[STEPS] += ok
        sc[SUM_EP, ok] += ep[ok]
        sc[MAX_EP, ok] = np.maximum(sc[MAX_EP, ok], ep[ok])
        sc[LAST_EP, ok] = ep[ok]
        sc[SUM_ES, ok] += es[ok]
        sc[MAX_ES, ok] = np.maximum(sc[MAX_ES, ok], es[ok])
        if out is not None:
            sc[SUM_TAU2, ok] += tau2[ok]
        sc[SUM_P2, ok] += p2[ok]
        if stat is not None:
            sc[NOT_SOLVED] += ok & (stat[c] != OSQP_SOLVED)
        with np.errstate(invalid="ignore"):
            over = ok & (ep > tol2)
        sc[FIRST_OVER, over] = np.where(sc[FIRST_OVER, over] < 0, k, np.minimum(sc[FIRST_OVER, over], k))
        sc[LAST_OVER, over] = np.maximum(sc[LAST_OVER, over], k)
    return sc


def group_reference(score, group, G):
    """umpcBatchScoreGroups in numpy fp64: [G, 8] raw sums over the robots of each group; ids outside [0, G) are ignored."""
    sc = np.asarray(score, np.float64)
    group = np.asarray(group)
    gs = np.zeros((int(G), GSCORE_ROWS))
    for b in range(sc.shape[1]):
        g = int(group[b])
        if not 0 <= g < G:
            continue
        n = sc[STEPS, b]
        gs[g, G_ROBOTS] += 1
        if n > 0:
            gs[g, G_SCORED] += 1
            gs[g, G_SUM_MEAN_EP] += sc[SUM_EP, b] / n
            gs[g, G_MAX_EP] = max(gs[g, G_MAX_EP], sc[MAX_EP, b])
            gs[g, G_SUM_MEAN_TAU2] += sc[SUM_TAU2, b] / n
            gs[g, G_SUM_MEAN_P2] += sc[SUM_P2, b] / n
        gs[g, G_LEFT] += sc[FIRST_OVER, b] >= 0
        gs[g, G_NOT_SOLVED] += sc[NOT_SOLVED, b]
    return gs


def combine_groups(parts):
    """The group table of a whole job from the tables [G, 8] of its blocks of robots (shard.score_block, one
    score_groups per block): the tables hold raw sums, so rows 0, 1, 2, 4, 5, 6, 7 add and row 3 takes the max.
    numpy arrays or torch tensors; the result is of the first part's kind."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_groups: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        mx = np.maximum(total[:, G_MAX_EP], p[:, G_MAX_EP]) if isinstance(total, np.ndarray) else \
            total[:, G_MAX_EP].maximum(p[:, G_MAX_EP])
        total += p
        total[:, G_MAX_EP] = mx
    return total


def group_index_reference(group, G):
    """umpcBatchGroupIndex in numpy: (order [B], offset [G + 1]) int32. order is a stable sort of the robots by group with
    every id outside [0, G) last: positions offset[g] .. offset[g + 1] - 1 hold group g in ascending robot index, positions
    offset[G] .. B - 1 the ignored robots."""
    group, G = np.asarray(group), int(G)
    if G < 1 or group.ndim != 1:
        raise ValueError("group_index_reference: bad argument")
    key = np.where((group >= 0) & (group < G), group, G)
    order = np.argsort(key, kind="stable").astype(np.int32)
    offset = np.zeros(G + 1, np.int32)
    for g in range(1, G + 1):
        offset[g] = offset[g - 1] + int((key == g - 1).sum())
    return order, offset


def ensemble_reference(state_hist, out_hist, status_hist, ref, first, count, ref_first, tol_p, after, taulim, order, offset):
    """umpcBatchEnsemble in numpy fp64, step by step and group by group: [count, G, 16] with G = len(offset) - 1. The tables,
    first, count, ref_first, tol_p and after are those of score_reference; order / offset are a group index
    (group_index_reference). The members of group g are order[offset[g]:offset[g + 1]]; a member is scored at a step when
    every value it reads there is finite. The sums are the correctly rounded sums of their terms (math.fsum): the mirror has no
    order of summation of its own."""
    st = np.asarray(state_hist, np.float64)
    out = None if out_hist is None else np.asarray(out_hist, np.float64)
    stat = None if status_hist is None else np.asarray(status_hist)
    ref = np.asarray(ref, np.float64)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after = int(first), int(count), int(ref_first), int(bool(after))
    G = len(offset) - 1
    if count < 0 or first < 0 or ref_first < 0 or not (tol_p >= 0 and np.isfinite(tol_p)) or G < 1:
        raise ValueError("ensemble_reference: bad argument")
    tol2, tl = float(tol_p) ** 2, float(taulim)
    ens = np.zeros((count, G, ENS_ROWS))
    for i in range(count):
        c = first + i
        ok, d, ep, es, _, tau2 = _step_terms(st[c + after], None if out is None else out[c],
                                             ref[ref_first + i] if ref.ndim == 3 else ref, tl)
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            sel = mem[ok[mem]]                                  # the scored members, in list order
            e = ens[i, g]
            e[E_N], e[E_SKIPPED] = len(sel), len(mem) - len(sel)
            e[E_MIN_EP], e[E_ARGMAX_EP] = np.inf, -1
            if len(sel) == 0:
                continue
            x = ep[sel]
            e[E_SUM_EP], e[E_SUM_EP2] = math.fsum(x), math.fsum(x * x)
            e[E_MAX_EP], e[E_MIN_EP] = x.max(), x.min()
            e[E_SUM_ES], e[E_MAX_ES] = math.fsum(es[sel]), es[sel].max()
            if out is not None:
                e[E_SUM_TAU2], e[E_MAX_TAU2] = math.fsum(tau2[sel]), tau2[sel].max()
            e[E_OVER] = (x > tol2).sum()
            if stat is not None:
                e[E_NOT_SOLVED] = (stat[c][sel] != OSQP_SOLVED).sum()
            for j in range(3):
                e[E_SUM_DX + j] = math.fsum(d[j][sel])
            e[E_ARGMAX_EP] = sel[x == x.max()].min()              # ties: the lowest robot index
    return ens


def combine_ensembles(parts, los=None):
    """The ensemble of a whole job from the ensembles [count, G, 16] of its blocks of robots (each block: its own columns
    and ids, BatchUprightMPC.group_index + ensemble): rows 0-3, 6, 8, 10-14 add, rows 4, 7, 9 take the max, row 5 the min,
    and row 15 comes from the part with the larger row 4 (the first such part on a tie), shifted by that block's first robot
    los[k] (None: no shift) -- the blocks in ascending robot order give the lowest index on a tie, as the undivided call
    does. numpy arrays or torch tensors; the result is of the first part's kind and the parts are not modified."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_ensembles: no parts")
    los = [0] * len(parts) if los is None else [int(v) for v in los]
    if len(los) != len(parts):
        raise ValueError("combine_ensembles: one lo per part")
    if hasattr(parts[0], "clone"):
        import torch as xp
        total = parts[0].clone()
    else:
        xp = np
        total = np.array(parts[0], np.float64)
    arg = total[..., E_ARGMAX_EP]
    total[..., E_ARGMAX_EP] = xp.where(arg >= 0, arg + los[0], arg)
    add, mx = list(ENS_ADD_ROWS), list(ENS_MAX_ROWS)
    for p, lo in zip(parts[1:], los[1:]):
        take = (p[..., E_ARGMAX_EP] >= 0) & ((total[..., E_ARGMAX_EP] < 0) | (p[..., E_MAX_EP] > total[..., E_MAX_EP]))
        total[..., E_ARGMAX_EP] = xp.where(take, p[..., E_ARGMAX_EP] + lo, total[..., E_ARGMAX_EP])
        total[..., add] = total[..., add] + p[..., add]
        total[..., mx] = xp.maximum(total[..., mx], p[..., mx])
        total[..., E_MIN_EP] = xp.minimum(total[..., E_MIN_EP], p[..., E_MIN_EP])
    return total


def quantile_rank(p, n):
    """The index k of the order statistic for probability p among n >= 1 values in ascending order (inverted CDF / nearest
    rank): k = min(n - 1, max(0, ceil(p * n) - 1)), the product one IEEE double multiply. p = 0 the minimum, p = 1 the
    maximum, p = 0.5 the lower median."""
    return min(int(n) - 1, max(0, int(math.ceil(float(p) * float(n))) - 1))


def _check_probs(probs, what):
    probs = [float(p) for p in np.atleast_1d(np.asarray(probs, np.float64))]
    if not 1 <= len(probs) <= QUANT_MAX_PROBS or not all(0.0 <= p <= 1.0 for p in probs):
        raise ValueError("%s: 1 to %d probabilities, each in [0, 1]" % (what, QUANT_MAX_PROBS))
    return probs


def _quantile_row(values, members, probs):
    """[2 + nq]: values = the members' values that enter (any order), members = the size of the group"""
    v = sorted(float(x) for x in values)
    row = [float(len(v)), float(members - len(v))]
    row += [v[quantile_rank(p, len(v))] if v else float("nan") for p in probs]
    return row


def ensemble_quantiles_reference(state_hist, out_hist, ref, first, count, ref_first, after, taulim, order, offset, probs,
                                 term=TERM_EP):
    """umpcBatchEnsembleQuantiles in numpy, step by step and group by group: [count, G, 2 + nq]. The tables, first, count,
    ref_first, after, order and offset are those of ensemble_reference; a member is scored at a step exactly when
    ensemble_reference with the same out_hist scores it. term: TERM_EP |p - pdes|^2, TERM_ES |s - sdes|^2, TERM_TAU the
    moments squared, clipped at +-taulim (needs out_hist), in the mirror's fp64. Row 0 = members scored (n), row 1 = members
    skipped, row 2 + j = v[quantile_rank(probs[j], n)] over the scored members' terms v in ascending order -- an explicit
    sort and an explicit rank --, NaN when n = 0.
    Quantiles do NOT combine across the blocks of a sharded job (there is no combine_quantiles): keep a cell inside one
    block. Cells of 64 in contiguous blocks are."""
    st = np.asarray(state_hist, np.float64)
    out = None if out_hist is None else np.asarray(out_hist, np.float64)
    ref = np.asarray(ref, np.float64)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after, term = int(first), int(count), int(ref_first), int(bool(after)), int(term)
    G = len(offset) - 1
    probs = _check_probs(probs, "ensemble_quantiles_reference")
    if count < 0 or first < 0 or ref_first < 0 or G < 1 or term not in (TERM_EP, TERM_ES, TERM_TAU) or (term == TERM_TAU and out is None):
        raise ValueError("ensemble_quantiles_reference: bad argument")
    tl = float(taulim)
    quant = np.zeros((count, G, 2 + len(probs)))
    for i in range(count):
        c = first + i
        ok, _, ep, es, _, tau2 = _step_terms(st[c + after], None if out is None else out[c],
                                             ref[ref_first + i] if ref.ndim == 3 else ref, tl)
        x = ep if term == TERM_EP else es if term == TERM_ES else tau2
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            quant[i, g] = _quantile_row(x[mem[ok[mem]]], len(mem), probs)
    return quant


def _table_value(sc, num, den):
    """(value [B] float64, enters [B] bool) of a score table [12, B]: sc[num], or the IEEE double quotient sc[num] / sc[den]
    when den >= 0; a robot enters when its row 0 > 0 and the value is finite"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = sc[num].astype(np.float64)
        if den >= 0:
            x = x / sc[den].astype(np.float64)
    return x, (sc[STEPS] > 0) & np.isfinite(x)


def score_quantiles_reference(score, order, offset, probs, num, den=None):
    """umpcBatchScoreQuantiles in numpy: [G, 2 + nq] over the robots of each group of a per-robot score [12, B]. The value of
    robot b is score[num, b], or the IEEE double quotient score[num, b] / score[den, b] (den None or -1: no division;
    SUM_EP / STEPS is the per-robot mean tracking error). A robot enters when its row 0 > 0 and the value is finite (the
    rule of group_reference); the other members of the group are counted in row 1. Values may be negative."""
    sc = np.asarray(score)
    order, offset = np.asarray(order), np.asarray(offset)
    num, den = int(num), -1 if den is None else int(den)
    G = len(offset) - 1
    probs = _check_probs(probs, "score_quantiles_reference")
    if G < 1 or not 0 <= num < SCORE_ROWS or not -1 <= den < SCORE_ROWS:
        raise ValueError("score_quantiles_reference: bad argument")
    x, ok = _table_value(sc, num, den)
    quant = np.zeros((G, 2 + len(probs)))
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        quant[g] = _quantile_row(x[mem[ok[mem]]], len(mem), probs)
    return quant


def u01(seed, idx, salt):
    """The counter hash of the library's Monte-Carlo draws, the one numpy definition (batch._u01 is this function; the kernels'
    boot_u01 and batch._u01_device restate it): idx + seed * 0x9E3779B97F4A7C15 + salt modulo 2^64, two multiply-xorshift
    rounds, the top 53 bits as a double in [0, 1). idx: an array of counters, any integer dtype."""
    with np.errstate(over="ignore"):
        v = np.asarray(idx).astype(np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15 + int(salt)) & 0xFFFFFFFFFFFFFFFF)
        v ^= v >> np.uint64(30); v *= np.uint64(0xBF58476D1CE4E5B9)
        v ^= v >> np.uint64(27); v *= np.uint64(0x94D049BB133111EB)
        v ^= v >> np.uint64(31)
    return (v >> np.uint64(11)).astype(np.float64) / float(1 << 53)


bootstrap_u01 = u01


def bootstrap_indices(nsc, R, seed):
    """[R, nsc] int64: the member slot m of replicate r takes, j = min(nsc - 1, floor(u * nsc)) in double with
    u = bootstrap_u01(seed, (r << 32) + m, 41). A function of (seed, r, m, nsc) alone -- not of the cell, the number of cells
    or anything else: cells with equal nsc are resampled with the same indices (common random numbers)."""
    nsc, R = int(nsc), int(R)
    idx = (np.arange(R, dtype=np.uint64)[:, None] << np.uint64(32)) + np.arange(nsc, dtype=np.uint64)[None, :]
    u = bootstrap_u01(seed, idx, BOOT_SALT)
    return np.minimum(nsc - 1, np.floor(u * float(nsc)).astype(np.int64))


def _total_order_image(v):
    """the unsigned image whose integer order is the total order of the doubles (-0 before +0): the kernels' quant_image"""
    b = np.ascontiguousarray(v, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def _boot_statistic(sample, stat, p):
    """of one sample (a 1-d float64 array, at least one value): fsum / n, or the element at quantile_rank(p, n) of the sample
    sorted by its total-order image"""
    n = len(sample)
    if stat == 0:
        return math.fsum(sample.tolist()) / n
    return float(sample[np.argsort(_total_order_image(sample), kind="stable")[quantile_rank(p, n)]])


def score_bootstrap_values(score, num, den=None, other=None):
    """(value [B] float64, enters [B] bool) of umpcBatchScoreBootstrap: x_b = score[num, b] or the IEEE double quotient
    score[num, b] / score[den, b]; with `other` the same expression of the second table is subtracted in double. A robot
    enters when row 0 > 0 in score (and in other, if given) and the value is finite."""
    num, den = int(num), -1 if den is None else int(den)
    if not 0 <= num < SCORE_ROWS or not -1 <= den < SCORE_ROWS:
        raise ValueError("score_bootstrap_values: bad argument (num in 0..11, den in -1..11)")
    sc = np.asarray(score)
    x, ok = _table_value(sc, num, den)
    if other is not None:
        ot = np.asarray(other)
        if ot.shape != sc.shape or ot.dtype != sc.dtype:
            raise ValueError("score_bootstrap_values: other must have the shape and dtype of score")
        y, ok2 = _table_value(ot, num, den)
        with np.errstate(invalid="ignore", over="ignore"):
            x = x - y               # (finite only when both values are)
        ok = ok & ok2 & np.isfinite(x)
    return x, ok


def score_bootstrap_reference(score, order, offset, num, den=None, other=None, stat="mean", p=0.5, reps=1000, seed=0,
                              probs=(0.025, 0.975)):
    """umpcBatchScoreBootstrap in numpy, cell by cell and replicate by replicate: (boot [G, 5 + nq], reps [G, R]).
    The scored values of cell g in member-list order, v[0 .. nsc), are resampled R = reps times with bootstrap_indices(nsc,
    R, seed); the statistic of a sample is its math.fsum divided by nsc (stat "mean") or the element at quantile_rank(p, nsc)
    of the sample sorted in the total order of the values, -0 before +0 (stat "quantile"): an element, never an
    interpolation. boot rows: BOOT_N scored, BOOT_SKIPPED the cell's other members, BOOT_POINT the statistic of v itself,
    BOOT_MEAN fsum(t) / R over the replicates t, BOOT_SE sqrt(fsum((t - mean)^2) / (R - 1)), BOOT_FIRST + k the element
    at quantile_rank(probs[k], R) of the sorted replicates (the percentile interval). nsc = 0: NaN from BOOT_POINT on and a NaN
    row of reps. Every sum is an fsum: the mirror has no order of summation of its own.
    Cells with equal nsc share their indices. Lay a sweep out so that draw m of every cell carries the same perturbation (the
    task_table examples of INTEGRATION.md do): then reps[g1] - reps[g2] is a paired bootstrap of the difference between two
    cells. With other= (the reactive run of the same sweep on the same tables) the values are differences paired by draw.
    Like quantiles, the rows of the blocks of a sharded job do not combine: keep a cell inside one block."""
    order, offset = np.asarray(order), np.asarray(offset)
    G, R = len(offset) - 1, int(reps)
    probs = _check_probs(probs, "score_bootstrap_reference")
    if stat not in BOOT_STATS or not 0.0 <= float(p) <= 1.0 or not 2 <= R <= BOOT_MAX_REPS or G < 1:
        raise ValueError("score_bootstrap_reference: bad argument (stat 'mean' or 'quantile', p in [0, 1], 2 <= reps <= 2^20)")
    st, p = BOOT_STATS.index(stat), float(p)
    x, ok = score_bootstrap_values(score, num, den, other)
    boot = np.full((G, BOOT_FIRST + len(probs)), np.nan)
    out = np.full((G, R), np.nan)
    tables = {}
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        v = x[mem[ok[mem]]]
        nsc = len(v)
        boot[g, BOOT_N], boot[g, BOOT_SKIPPED] = nsc, len(mem) - nsc
        if nsc == 0:
            continue
        if nsc not in tables:
            tables[nsc] = bootstrap_indices(nsc, R, seed)
        t = out[g]
        for r in range(R):
            t[r] = _boot_statistic(v[tables[nsc][r]], st, p)
        boot[g, BOOT_POINT] = _boot_statistic(v, st, p)
        mean = math.fsum(t.tolist()) / R
        boot[g, BOOT_MEAN] = mean
        boot[g, BOOT_SE] = math.sqrt(math.fsum(((t - mean) ** 2).tolist()) / (R - 1))
        ts = t[np.argsort(_total_order_image(t), kind="stable")]
        for k, q in enumerate(probs):
            boot[g, BOOT_FIRST + k] = ts[quantile_rank(q, R)]
    return boot, out


def _boot_replicates(v, J, stat, p):
    """[R]: _boot_statistic of every resample v[J[r]], J [R, nsc] from bootstrap_indices -- the same values row by row, formed
    once for all rows: an fsum per row, or one sort of the total-order images along the rows (equal images are equal doubles)"""
    S = v[J]
    n = S.shape[1]
    if stat == 0:
        return np.array([math.fsum(row) / n for row in S.tolist()])
    img = np.sort(_total_order_image(S), axis=1)[:, quantile_rank(p, n)]
    return np.where(img >> np.uint64(63) != 0, img & np.uint64((1 << 63) - 1), ~img).view(np.float64)


def band_rows(t, point, nsc, probs, levels):
    """The band of ONE group from its replicates, the second half of ensemble_bootstrap_reference: t [K, R] the replicates of
    every step (rows with nsc = 0 are not read), point [K], nsc [K]. Returns (rows [K, 3 + nq] = mean, standard error, enters,
    the percentile columns; NaN and enters = 0 where nsc = 0), sup [R], crit [1 + nl]. A step enters when nsc >= 2 and its R
    replicates are not all the same double (total-order images: -0 is not +0); sup[r] is the largest |t[i, r] - point[i]| /
    se[i] over the entering steps, found by comparisons that a NaN never wins, from 0; crit[0] the number of entering steps,
    crit[1 + j] the element at quantile_rank(levels[j], R) of sup sorted; NaN when no step enters. Every sum is an fsum."""
    t = np.asarray(t, np.float64)
    K, R = t.shape
    rows = np.full((K, 3 + len(probs)), np.nan)
    rows[:, 2] = 0.0
    sup, entered = np.zeros(R), 0
    for i in range(K):
        if nsc[i] == 0:
            continue
        ti = t[i]
        mean = math.fsum(ti.tolist()) / R
        se = math.sqrt(math.fsum(((ti - mean) ** 2).tolist()) / (R - 1))
        img = _total_order_image(ti)
        ts = ti[np.argsort(img, kind="stable")]
        rows[i, 0], rows[i, 1] = mean, se
        rows[i, 3:] = [ts[quantile_rank(q, R)] for q in probs]
        if nsc[i] >= 2 and img.min() != img.max():
            rows[i, 2] = 1.0
            entered += 1
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                d = np.abs(ti - point[i]) / se
                sup = np.where(d > sup, d, sup)
    crit = np.full(1 + len(levels), np.nan)
    crit[0] = entered
    if entered == 0:
        return rows, np.full(R, np.nan), crit
    ss = np.sort(sup)
    crit[1:] = [ss[quantile_rank(q, R)] for q in levels]
    return rows, sup, crit


BAND_N, BAND_SKIPPED, BAND_POINT, BAND_MEAN, BAND_SE, BAND_ENTERS, BAND_FIRST = 0, 1, 2, 3, 4, 5, 6
BAND_MAX_REPS = 4096


def ensemble_bootstrap_reference(state_hist, out_hist, ref, first, count, ref_first, after, taulim, order, offset, term=TERM_EP,
                                 other=None, stat="mean", p=0.5, reps=1000, seed=0, probs=(0.025, 0.975), levels=(0.95,),
                                 dtype=np.float64):
    """umpcBatchEnsembleBootstrap in numpy, group by group, step by step and replicate by replicate: (band [count, G, 6 + nq],
    crit [G, 1 + nl], sup [G, R]). The tables, first, count, ref_first, after, order, offset and term are those of
    ensemble_quantiles_reference. At step i of the window the values of group g are the terms of its members scored at
    that step (the rule of ensemble_quantiles_reference with the same out_hist) in member-list order, v_i[0 .. nsc_i). With
    other = (state_hist, out_hist or None) of a second run of the same shape, read against the SAME reference, a member
    enters when both runs score it and x - x_other, subtracted in double, is finite; that difference is the value.
    Replicate t[i, r] = the statistic of v_i[bootstrap_indices(nsc_i, R, seed)[r]]: its fsum / nsc_i (stat "mean") or its
    element at quantile_rank(p, nsc_i) in the total order (stat "quantile"), exactly as score_bootstrap_reference. The
    indices do not depend on the step: while nsc does not change, replicate r resamples the same members at every step --
    whole trajectories. When a draw drops out mid-window its steps are resampled with the indices of the new count.
    band columns: BAND_N scored, BAND_SKIPPED, BAND_POINT the statistic of v_i, BAND_MEAN fsum(t_i) / R, BAND_SE
    sqrt(fsum((t_i - mean)^2) / (R - 1)), BAND_ENTERS 1.0 when the step enters the simultaneous statistic (nsc_i >= 2 and the
    R replicates are not all the same double -- a test on replicates, not on se > 0), BAND_FIRST + k the element at
    quantile_rank(probs[k], R) of the sorted replicates: the pointwise percentile band. nsc_i = 0: NaN from BAND_POINT on and
    BAND_ENTERS = 0. sup[g, r] = max over the entering steps of |t[i, r] - point_i| / se_i, crit[g, 0] = the number of entering
    steps, crit[g, 1 + j] = the element at quantile_rank(levels[j], R) of sup[g] sorted; NaN when no step enters (band_rows).
    The simultaneous band of group g is band[:, g, BAND_POINT] +- crit[g, 1 + j] * band[:, g, BAND_SE].
    dtype: the terms are evaluated in it (the same operations in the same order as the kernels' score_terms) and then widened
    to double: np.float32 gives the values the device forms from fp32 tables bit for bit, so that what is left between the
    mirror and the device is the rounding of the sums alone. Everything behind the values is fp64 either way.
    Like quantiles, the rows of the blocks of a sharded job do not combine: keep a cell inside one block."""
    dtype = np.dtype(dtype)
    st = np.asarray(state_hist).astype(dtype)
    out = None if out_hist is None else np.asarray(out_hist).astype(dtype)
    ref = np.asarray(ref).astype(dtype)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after, term = int(first), int(count), int(ref_first), int(bool(after)), int(term)
    G, R = len(offset) - 1, int(reps)
    probs = _check_probs(probs, "ensemble_bootstrap_reference")
    levels = _check_probs(levels, "ensemble_bootstrap_reference")
    if (count < 0 or first < 0 or ref_first < 0 or G < 1 or term not in (TERM_EP, TERM_ES, TERM_TAU)
            or (term == TERM_TAU and out is None) or stat not in BOOT_STATS or not 0.0 <= float(p) <= 1.0
            or not 2 <= R <= BAND_MAX_REPS):
        raise ValueError("ensemble_bootstrap_reference: bad argument (term, stat 'mean' or 'quantile', p in [0, 1], 2 <= reps <= 4096)")
    ost = oout = None
    if other is not None:
        ost = np.asarray(other[0]).astype(dtype)
        oout = None if other[1] is None else np.asarray(other[1]).astype(dtype)
        if ost.shape != st.shape or (oout is None) != (out is None):
            raise ValueError("ensemble_bootstrap_reference: other must be (state_hist, out_hist) of the shape of the first run")
    sti, p, tl = BOOT_STATS.index(stat), float(p), dtype.type(taulim)
    x, ok = np.zeros((count, st.shape[-1])), np.zeros((count, st.shape[-1]), bool)
    for i in range(count):
        c = first + i
        r = ref[ref_first + i] if ref.ndim == 3 else ref
        terms = _step_terms(st[c + after], None if out is None else out[c], r, tl)
        x[i], ok[i] = (terms[2 + term] if term < 2 else terms[5]).astype(np.float64), terms[0]
        if ost is not None:
            oterms = _step_terms(ost[c + after], None if oout is None else oout[c], r, tl)
            with np.errstate(invalid="ignore", over="ignore"):
                x[i] = x[i] - (oterms[2 + term] if term < 2 else oterms[5]).astype(np.float64)
            ok[i] &= oterms[0] & np.isfinite(x[i])
    nq = len(probs)
    band = np.full((count, G, BAND_FIRST + nq), np.nan)
    crit, sup = np.full((G, 1 + len(levels)), np.nan), np.full((G, R), np.nan)
    tables = {}
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        t, point, nsc = np.full((count, R), np.nan), np.full(count, np.nan), np.zeros(count, np.int64)
        for i in range(count):
            v = x[i, mem[ok[i, mem]]]
            nsc[i] = len(v)
            if len(v) == 0:
                continue
            if len(v) not in tables:
                tables[len(v)] = bootstrap_indices(len(v), R, seed)
            t[i] = _boot_replicates(v, tables[len(v)], sti, p)
            point[i] = _boot_statistic(v, sti, p)
        rows, sup[g], crit[g] = band_rows(t, point, nsc, probs, levels)
        band[:, g, BAND_N], band[:, g, BAND_SKIPPED], band[:, g, BAND_POINT] = nsc, len(mem) - nsc, point
        band[:, g, BAND_MEAN:] = rows
    return band, crit, sup


# ----------------------------------------------------------------------------------------------------------------------
# Frequency response (umpcBatchResponseInit / umpcBatchResponse / umpcBatchResponseFit): a three-parameter sine fit
# y_k ~ a0 + a1 cos(phi_k) + a2 sin(phi_k) per robot and position axis, of p and of pdes, at the robot's own frequency
# ----------------------------------------------------------------------------------------------------------------------
RSUM_ROWS, RESP_ROWS = 33, 12
# sum rows: common, then 9 per axis j at RSUM_AXIS + 9 j
RSUM_N, RSUM_SKIPPED, RSUM_C, RSUM_S, RSUM_CC, RSUM_CS, RSUM_AXIS = 0, 1, 2, 3, 4, 5, 6
(RSUM_Y, RSUM_YC, RSUM_YS, RSUM_YY, RSUM_R, RSUM_RC, RSUM_RS, RSUM_RR, RSUM_YR) = range(9)
RSUM_AXIS_ROWS = 9
# response rows, per axis (row 0 > 0 means "enters", as in a score: score_quantiles / score_bootstrap take resp[axis] as it is)
(RESP_STEPS, RESP_SKIPPED, RESP_Y_AMP2, RESP_R_AMP2, RESP_GAIN, RESP_PHASE, RESP_H_RE, RESP_H_IM, RESP_Y_DC, RESP_R_DC,
 RESP_Y_RES, RESP_E_AMP2) = range(12)
RESP_ROW_NAMES = ("steps", "skipped", "y_amp2", "r_amp2", "gain", "phase", "h_re", "h_im", "y_dc", "r_dc", "y_res", "e_amp2")
RESP_PIVOT_TOL = 1e-9       # the fit is refused when a Cholesky pivot is <= RESP_PIVOT_TOL * n


def response_nu(freq_hz, nsub, dtsim):
    """The frequency of a task in revolutions per closed-loop step, float64: freq_hz * 1e-3 * nsub * dtsim, multiplied in that
    order (dtsim in ms: 5 Hz at the default 25 x 0.2 ms step is 0.025)."""
    return np.asarray(freq_hz, np.float64) * 1e-3 * float(nsub) * float(dtsim)


def response_identity(B):
    """The sums no step has entered (umpcBatchResponseInit): zeros [33, B] float64."""
    return np.zeros((RSUM_ROWS, int(B)))


def response_phase(k, nu):
    """(c, s) = (cos, sin)(2 pi u), u = k nu - floor(k nu) with ONE double multiply of float(k) and nu [B], and u itself. The
    quadrant is taken out exactly first (u - j / 4 is exact), so the argument of cos / sin is at most pi / 4 and the results
    are within ~2 ulp of the true values, exactly 0 and +-1 at the quarter points, whatever k is."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = float(k) * np.asarray(nu, np.float64)
        u = x - np.floor(x)
        j = np.rint(4.0 * u)
        a = (2.0 * np.pi) * (u - 0.25 * j)
        ca, sa = np.cos(a), np.sin(a)
        jj = np.where(np.isfinite(j), j, 0).astype(np.int64) & 3
    c = np.choose(jj, [ca, -sa, -ca, sa])
    s = np.choose(jj, [sa, ca, -sa, -ca])
    return c, s, u


def response_sums_reference(state_hist, ref, nu, first, count, ref_first, step0, after, sums=None):
    """umpcBatchResponse in numpy fp64, step by step in order. state_hist [.., 18, B] and ref -- a table [.., 9, B] (slice
    ref_first + i) or one constant reference [9, B] -- are taken as given and widened; nu [B] float64 is the frequency of each
    robot in revolutions per step. Step c = first + i reads rows 0..2 of state slice c + after and of its reference slice and
    carries k = step0 + i, phase response_phase(k, nu). A step where any of the six words, or the phase, is not finite is
    counted in RSUM_SKIPPED and in no other row. Returns the sums [33, B] (float64); passing one back in accumulates."""
    st = np.asarray(state_hist, np.float64)
    ref = np.asarray(ref, np.float64)
    B = st.shape[-1]
    nu = np.asarray(nu, np.float64)
    first, count, ref_first, step0, after = int(first), int(count), int(ref_first), int(step0), int(bool(after))
    if count < 0 or first < 0 or ref_first < 0 or step0 < 0 or step0 + count > 1 << 53 or nu.shape != (B,):
        raise ValueError("response_sums_reference: bad argument")
    sm = response_identity(B) if sums is None else np.array(sums, np.float64)
    for i in range(count):
        y = st[first + i + after, 0:3]
        r = (ref[ref_first + i] if ref.ndim == 3 else ref)[0:3]
        c, s, u = response_phase(step0 + i, nu)
        ok = np.isfinite(u) & np.isfinite(y).all(0) & np.isfinite(r).all(0)
        sm[RSUM_SKIPPED] += ~ok
        sm[RSUM_N] += ok
        c, s = c[ok], s[ok]
        sm[RSUM_C, ok] += c
        sm[RSUM_S, ok] += s
        sm[RSUM_CC, ok] += c * c
        sm[RSUM_CS, ok] += c * s
        for j in range(3):
            yj, rj, a = y[j, ok], r[j, ok], RSUM_AXIS + RSUM_AXIS_ROWS * j
            for row, term in ((RSUM_Y, yj), (RSUM_YC, yj * c), (RSUM_YS, yj * s), (RSUM_YY, yj * yj), (RSUM_R, rj),
                              (RSUM_RC, rj * c), (RSUM_RS, rj * s), (RSUM_RR, rj * rj), (RSUM_YR, yj * rj)):
                sm[a + row, ok] += term
    return sm


def _response_factor(sm):
    """the Cholesky factor of the normal matrix [[n, Sc, Ss], [Sc, Scc, Scs], [Ss, Scs, n - Scc]] in that variable order, in
    the kernel's operation order: ((l11, l21, l31, l22, l32, l33), pivots [3, B], fit [B] bool)"""
    n, Sc, Ss, Scc, Scs = sm[RSUM_N], sm[RSUM_C], sm[RSUM_S], sm[RSUM_CC], sm[RSUM_CS]
    Sss, tol = n - Scc, RESP_PIVOT_TOL * n
    d1 = n
    l11 = np.sqrt(d1)
    l21, l31 = Sc / l11, Ss / l11
    d2 = Scc - l21 * l21
    l22 = np.sqrt(d2)
    l32 = (Scs - l21 * l31) / l22
    d3 = (Sss - l31 * l31) - l32 * l32
    l33 = np.sqrt(d3)
    fit = (n >= 3.0) & (d1 > tol) & (d2 > tol) & (d3 > tol)
    return (l11, l21, l31, l22, l32, l33), np.stack([d1, d2, d3]), fit


def response_pivots(sums):
    """[3, B]: the Cholesky pivots d1 = n, d2, d3 of every robot's normal matrix (the squares of the factor's diagonal); the
    fit is refused when n < 3 or one of them is <= 1e-9 n. For a window of whole periods they are n, n / 2, n / 2."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return _response_factor(np.asarray(sums, np.float64))[1]


def response_fit_reference(sums):
    """umpcBatchResponseFit in numpy fp64, in the kernel's operation order: [3, 12, B] float64 from the sums [33, B]. Rows per
    axis (RESP_*), with Y = a1 - i a2 of y = p_axis and R likewise of r = pdes_axis: STEPS n, or 0 when the fit is refused (n < 3
    or a pivot <= 1e-9 n: rows 2..11 are then NaN); SKIPPED; Y_AMP2 |Y|^2; R_AMP2 |R|^2; GAIN sqrt(Y_AMP2 / R_AMP2); PHASE arg Y -
    arg R in (-pi, pi], negative = a lag; H_RE, H_IM the parts of Y / R (GAIN, PHASE, H_RE, H_IM are NaN when R_AMP2 is 0); Y_DC,
    R_DC the offsets a0; Y_RES = max(0, (sum yy - a . rhs) / n), the mean squared residual of y's fit; E_AMP2 |Y - R|^2."""
    sm = np.asarray(sums, np.float64)
    if sm.ndim != 2 or sm.shape[0] != RSUM_ROWS:
        raise ValueError("response_fit_reference: sums must be [33, B]")
    B = sm.shape[1]
    resp = np.full((3, RESP_ROWS, B), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        (l11, l21, l31, l22, l32, l33), _, fit = _response_factor(sm)

        def solve(b0, b1, b2):
            z0 = b0 / l11
            z1 = (b1 - l21 * z0) / l22
            z2 = ((b2 - l31 * z0) - l32 * z1) / l33
            a2 = z2 / l33
            a1 = (z1 - l32 * a2) / l22
            a0 = ((z0 - l21 * a1) - l31 * a2) / l11
            return a0, a1, a2

        n = sm[RSUM_N]
        for j in range(3):
            x = sm[RSUM_AXIS + RSUM_AXIS_ROWS * j:RSUM_AXIS + RSUM_AXIS_ROWS * (j + 1)]
            ay, ar = solve(x[RSUM_Y], x[RSUM_YC], x[RSUM_YS]), solve(x[RSUM_R], x[RSUM_RC], x[RSUM_RS])
            yamp2, ramp2 = ay[1] * ay[1] + ay[2] * ay[2], ar[1] * ar[1] + ar[2] * ar[2]
            re, im = ay[1] * ar[1] + ay[2] * ar[2], ay[1] * ar[2] - ay[2] * ar[1]
            href = ramp2 > 0.0
            res = (x[RSUM_YY] - ((ay[0] * x[RSUM_Y] + ay[1] * x[RSUM_YC]) + ay[2] * x[RSUM_YS])) / n
            e1, e2 = ay[1] - ar[1], ay[2] - ar[2]
            at = np.arctan2(im, re)
            o = resp[j]
            o[RESP_STEPS] = n
            o[RESP_Y_AMP2], o[RESP_R_AMP2] = yamp2, ramp2
            o[RESP_GAIN] = np.where(href, np.sqrt(yamp2 / ramp2), np.nan)
            o[RESP_PHASE] = np.where(href, np.where(at == -np.pi, np.pi, at), np.nan)
            o[RESP_H_RE], o[RESP_H_IM] = np.where(href, re / ramp2, np.nan), np.where(href, im / ramp2, np.nan)
            o[RESP_Y_DC], o[RESP_R_DC] = ay[0], ar[0]
            o[RESP_Y_RES] = np.where(res > 0.0, res, 0.0)
            o[RESP_E_AMP2] = e1 * e1 + e2 * e2
            o[2:, ~fit] = np.nan
            o[RESP_STEPS, ~fit] = 0.0
            o[RESP_SKIPPED] = sm[RSUM_SKIPPED]
    return resp


# ---- dispersion ellipsoids (umpcBatchDispersion / umpcBatchDispersionEllipsoids / umpcBatchMahalanobis) ------------------------
DISP_ROWS, ELL_ROWS, MAHA_ROWS = 32, 48, 12
# moment rows, per (step, group): members scored / skipped, S1 = sum z [6], S2 = sum z_i z_j [21] (upper triangle row by row)
D_N, D_SKIPPED, D_S1, D_S2 = 0, 1, 2, 8
DISP_PAIRS = tuple((i, j) for i in range(6) for j in range(i, 6))      # the (i, j) of S2 entry k, and of covariance entry k
DISP_PP = (0, 1, 2, 6, 7, 11)                                          # the entries of the 3 x 3 position block: 00 01 02 11 12 22
# ellipsoid rows: n, skipped, mean [6], covariance [21], eigenvalues of C_pp descending [3], V [3, 3] row by row (column c =
# eigenvector c), status, Linv [6] (lower triangle row by row: 00 10 11 20 21 22)
L_N, L_SKIPPED, L_MEAN, L_COV, L_EIGVAL, L_EIGVEC, L_STATUS, L_LINV = 0, 1, 2, 8, 29, 32, 41, 42
ELL_OK, ELL_FEW, ELL_NOT_PD = 0, 1, 2
ELL_SWEEPS = 8              # cyclic Jacobi sweeps of the 3 x 3 block, fixed
ELL_PIVOT_TOL = 1e-12       # a Cholesky pivot fails when it is <= ELL_PIVOT_TOL * trace(C_pp)
# Mahalanobis score rows, per robot
(M_STEPS, M_SUM_D2, M_MAX_D2, M_STEP_MAX, M_OVER, M_FIRST_OVER, M_LAST_OVER, M_LAST_D2, M_SKIPPED) = range(9)
MAHA_ROW_NAMES = ("steps", "sum_d2", "max_d2", "step_max", "over", "first_over", "last_over", "last_d2", "skipped", "", "", "")


def _error_state(y, r, dtype):
    """(ok [B], z [6, B] float64): z = (p - pdes, v - dpdes) of one step, each difference formed in `dtype` with one rounding
    and then widened; ok: all 12 words are finite"""
    y, r = np.asarray(y, dtype), np.asarray(r, dtype)
    a, b = np.concatenate([y[0:3], y[12:15]]), r[0:6]
    with np.errstate(invalid="ignore", over="ignore"):
        z = (a - b).astype(np.float64)
    return np.isfinite(a).all(0) & np.isfinite(b).all(0), z


def _lane_fold(terms):
    """[rows] from terms [rows, n] of the n members of a group in list order, IN THE DEVICE'S ORDER (disp_store,
    csrc/umpc_dispersion.h): lane l of 64 starts at +0 and adds the terms of members l, l + 64, ..; then for w = 32, 16, .., 1
    lane l becomes (lane l) + (lane l ^ w)"""
    lanes = np.arange(64)
    part = np.zeros((terms.shape[0], 64))
    with np.errstate(over="ignore", invalid="ignore"):
        for m0 in range(0, terms.shape[1], 64):
            t = terms[:, m0:m0 + 64]
            part[:, :t.shape[1]] = part[:, :t.shape[1]] + t
        for w in (32, 16, 8, 4, 2, 1):
            part = part + part[:, lanes ^ w]
    return part[:, 0]


def dispersion_reference(state_hist, ref, first, count, ref_first, after, order, offset, dtype=np.float64):
    """umpcBatchDispersion in numpy, IN THE DEVICE'S ORDER OF SUMMATION: [count, G, 32] float64. The tables, first, count,
    ref_first and after are those of ensemble_reference (no out, no status); dtype is the handle's: the differences are
    formed in it, everything after is float64. Per (step, group) row, lane l of 64 starts at +0 and adds the terms of members
    l, l + 64, .. of the list in order (+0 for a member that is not scored); then for w = 32, 16, .., 1 lane l becomes
    (lane l) + (lane l ^ w). Elementwise IEEE additions in that order: the kernel's bits (the kernel evaluates this tree for the
    one lane that stores the entry)."""
    st = np.asarray(state_hist)
    ref = np.asarray(ref)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after = int(first), int(count), int(ref_first), int(bool(after))
    G = len(offset) - 1
    if count < 0 or first < 0 or ref_first < 0 or G < 1:
        raise ValueError("dispersion_reference: bad argument")
    mom = np.zeros((count, G, DISP_ROWS))
    for i in range(count):
        ok, z = _error_state(st[first + i + after], ref[ref_first + i] if ref.ndim == 3 else ref, dtype)
        z = np.where(ok, z, 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            terms = np.concatenate([z, np.stack([z[a] * z[b] for a, b in DISP_PAIRS])])       # [27, B]
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            scored = int(ok[mem].sum())
            mom[i, g, D_N], mom[i, g, D_SKIPPED] = scored, len(mem) - scored
            mom[i, g, D_S1:D_S1 + 27] = _lane_fold(terms[:, mem])
    return mom


def combine_dispersions(parts):
    """The moments of a whole job from the moments [count, G, 32] of its blocks of robots, or of the column blocks a cell is
    split over: raw moments add, so rows 0..28 are sums (counts exactly; S1 and S2 to the rounding of one more addition per
    part) -- what order statistics cannot do. numpy arrays or torch tensors; the result is of the first part's kind and the
    parts are not modified. dispersion_ellipsoids / ellipsoid_reference of the result is the ellipsoid of the whole cell."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_dispersions: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        total[..., :D_S2 + 21] = total[..., :D_S2 + 21] + p[..., :D_S2 + 21]
    return total


def _jacobi_rotate(app, aqq, apq, arp, arq, vp, vq):
    """one rotation of ell_rotate (csrc/umpc_dispersion.h), elementwise over arrays, same operations in the same order"""
    theta = (aqq - app) / (2.0 * apq)
    t = np.copysign(1.0, theta) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(apq != 0.0, t, 0.0)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    app, aqq = app - t * apq, aqq + t * apq
    arp, arq = c * arp - s * arq, s * arp + c * arq
    vp, vq = c * vp - s * vq, s * vp + c * vq
    return app, aqq, np.zeros_like(apq), arp, arq, vp, vq


def ellipsoid_reference(mom):
    """umpcBatchDispersionEllipsoids in numpy fp64, in the kernel's operation order: [.., 48] from the moments [.., 32]. Mean
    S1 / n; covariance (S2 - S1 S1^T / n) / (n - 1); the 3 x 3 position block by cyclic Jacobi, pairs (0,1), (0,2), (1,2),
    ELL_SWEEPS sweeps whatever the data; eigenvalues descending, eigenvectors the columns of V with the component of largest
    magnitude positive (ties: the lowest index); status ELL_FEW when n < 2 (rows 8..47 NaN but the status), ELL_NOT_PD when a
    Cholesky pivot of the position block is <= ELL_PIVOT_TOL * trace or NaN (rows 42..47 NaN); Linv = inverse of the lower
    Cholesky factor."""
    mom = np.asarray(mom, np.float64)
    if mom.shape[-1] != DISP_ROWS:
        raise ValueError("ellipsoid_reference: mom must be [.., 32]")
    ell = np.full(mom.shape[:-1] + (ELL_ROWS,), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = mom[..., D_N]
        s1 = [mom[..., D_S1 + j] for j in range(6)]
        ell[..., L_N], ell[..., L_SKIPPED] = n, mom[..., D_SKIPPED]
        for j in range(6):
            ell[..., L_MEAN + j] = s1[j] / n
        few = ~(n >= 2.0)
        c = [(mom[..., D_S2 + k] - s1[i] * s1[j] / n) / (n - 1.0) for k, (i, j) in enumerate(DISP_PAIRS)]
        for k in range(21):
            ell[..., L_COV + k] = c[k]
        c00, c01, c02, c11, c12, c22 = (c[k] for k in DISP_PP)
        a00, a01, a02, a11, a12, a22 = c00, c01, c02, c11, c12, c22
        one, zero = np.ones_like(n), np.zeros_like(n)
        v = [np.stack([one, zero, zero]), np.stack([zero, one, zero]), np.stack([zero, zero, one])]     # v[c][k]: column c
        for _ in range(ELL_SWEEPS):
            a00, a11, a01, a02, a12, v[0], v[1] = _jacobi_rotate(a00, a11, a01, a02, a12, v[0], v[1])
            a00, a22, a02, a01, a12, v[0], v[2] = _jacobi_rotate(a00, a22, a02, a01, a12, v[0], v[2])
            a11, a22, a12, a01, a02, v[1], v[2] = _jacobi_rotate(a11, a22, a12, a01, a02, v[1], v[2])
        lam = [a00, a11, a22]
        for i, j in ((0, 1), (1, 2), (0, 1)):
            sw = lam[i] < lam[j]
            lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
            v[i], v[j] = np.where(sw, v[j], v[i]), np.where(sw, v[i], v[j])
        for cidx in range(3):
            big = v[cidx][0]
            big = np.where(np.abs(v[cidx][1]) > np.abs(big), v[cidx][1], big)
            big = np.where(np.abs(v[cidx][2]) > np.abs(big), v[cidx][2], big)
            v[cidx] = np.where(big < 0.0, -v[cidx], v[cidx])
            ell[..., L_EIGVAL + cidx] = lam[cidx]
            for k in range(3):
                ell[..., L_EIGVEC + 3 * k + cidx] = v[cidx][k]
        floor = ELL_PIVOT_TOL * ((c00 + c11) + c22)
        l00 = np.sqrt(c00)
        l10, l20 = c01 / l00, c02 / l00
        p1 = c11 - l10 * l10
        l11 = np.sqrt(p1)
        l21 = (c12 - l20 * l10) / l11
        p2 = (c22 - l20 * l20) - l21 * l21
        l22 = np.sqrt(p2)
        bad = ~(c00 > floor) | ~(p1 > floor) | ~(p2 > floor)
        i00, i11, i22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
        i10, i21 = -(l10 * i00) * i11, -(l21 * i11) * i22
        i20 = -(l20 * i00 + l21 * i10) * i22
        for k, x in enumerate((i00, i10, i11, i20, i21, i22)):
            ell[..., L_LINV + k] = np.where(few | bad, np.nan, x)
        ell[..., L_COV:L_STATUS][few] = np.nan
        ell[..., L_STATUS] = np.where(few, ELL_FEW, np.where(bad, ELL_NOT_PD, ELL_OK))
    return ell


def mahalanobis_terms(state_hist, ref, ell, group, G, first, count, ref_first, after, dtype=np.float64):
    """(ok [count, B], d2 [count, B], A [count, B]) of umpcBatchMahalanobis: per step and robot whether the step is scored
    (p and pdes finite, the id inside [0, G), the row's status 0), d2 = |Linv (d - m_p)|^2 with d = p - pdes formed in `dtype`
    and widened, evaluated in float64 in the kernel's operation order and rounded once to `dtype` (returned as float64), and
    A = (sum_jk |Linv_jk| |d_k - m_k|)^2, the scale of d2's own rounding error. d2 and A are 0 where the step is not scored."""
    st, ref, ell = np.asarray(state_hist), np.asarray(ref), np.asarray(ell, np.float64)
    group, G = np.asarray(group), int(G)
    first, count, ref_first, after = int(first), int(count), int(ref_first), int(bool(after))
    B = st.shape[-1]
    gok = (group >= 0) & (group < G)
    gc = np.where(gok, group, 0)
    ok, d2, A = np.zeros((count, B), bool), np.zeros((count, B)), np.zeros((count, B))
    for i in range(count):
        y = np.asarray(st[first + i + after][0:3], dtype)
        r = np.asarray((ref[ref_first + i] if ref.ndim == 3 else ref)[0:3], dtype)
        row = ell[i][gc]                                   # [B, 48]
        with np.errstate(invalid="ignore", over="ignore"):
            e = (y - r).astype(np.float64) - row[:, L_MEAN:L_MEAN + 3].T
            li = row[:, L_LINV:L_LINV + 6].T
            y0, y1, y2 = li[0] * e[0], li[1] * e[0] + li[2] * e[1], (li[3] * e[0] + li[4] * e[1]) + li[5] * e[2]
            v = ((y0 * y0 + y1 * y1) + y2 * y2).astype(dtype).astype(np.float64)
            ae = np.abs(e)
            a = (np.abs(li[0]) * ae[0] + np.abs(li[1]) * ae[0] + np.abs(li[2]) * ae[1] + np.abs(li[3]) * ae[0] + np.abs(li[4]) * ae[1]
                 + np.abs(li[5]) * ae[2]) ** 2
        ok[i] = gok & (row[:, L_STATUS] == ELL_OK) & np.isfinite(y).all(0) & np.isfinite(r).all(0)
        d2[i], A[i] = np.where(ok[i], v, 0.0), np.where(ok[i], a, 0.0)
    return ok, d2, A


def mahalanobis_identity(B, dtype=np.float64):
    """The score no step has entered (umpcBatchMahalanobisInit): rows 3, 5 and 6 = -1, all others 0."""
    s = np.zeros((MAHA_ROWS, int(B)), dtype)
    s[M_STEP_MAX] = s[M_FIRST_OVER] = s[M_LAST_OVER] = -1
    return s


def mahalanobis_reference(state_hist, ref, ell, group, G, first, count, ref_first, step0, after, limit, dtype=np.float64, score=None):
    """umpcBatchMahalanobis in numpy, step by step in order: the score [12, B] float64 (rows M_*) of the steps first ..
    first + count - 1 against the ellipsoids ell [count, G, 48] of exactly those steps; step i carries the number step0 + i;
    `limit` is compared after rounding to `dtype`, as d2 is. Passing a score back in accumulates. The sum row is summed in
    float64 in step order: the mirror has no slices."""
    if not (limit > 0 and np.isfinite(limit)) or int(count) < 0 or int(first) < 0 or int(ref_first) < 0 or int(step0) < 0 or int(G) < 1:
        raise ValueError("mahalanobis_reference: bad argument")
    ok, d2, _ = mahalanobis_terms(state_hist, ref, ell, group, G, first, count, ref_first, after, dtype)
    B = ok.shape[1]
    sc = mahalanobis_identity(B) if score is None else np.array(score, np.float64)
    lim = float(np.asarray(limit, dtype))
    for i in range(int(count)):
        k, o, v = int(step0) + i, ok[i], d2[i]
        sc[M_SKIPPED] += ~o
        sc[M_STEPS] += o
        sc[M_SUM_D2, o] += v[o]
        take = o & ((sc[M_STEP_MAX] < 0) | (v > sc[M_MAX_D2]) | ((v == sc[M_MAX_D2]) & (k < sc[M_STEP_MAX])))
        sc[M_MAX_D2, take], sc[M_STEP_MAX, take] = v[take], k
        sc[M_LAST_D2, o] = v[o]
        over = o & (v > lim)
        sc[M_OVER] += over
        sc[M_FIRST_OVER, over] = np.where(sc[M_FIRST_OVER, over] < 0, k, np.minimum(sc[M_FIRST_OVER, over], k))
        sc[M_LAST_OVER, over] = np.maximum(sc[M_LAST_OVER, over], k)
    return sc


def chi2_3_cdf(x):
    """P(chi^2 with 3 degrees of freedom <= x) in closed form: erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2)"""
    x = float(x)
    return 0.0 if x <= 0 else math.erf(math.sqrt(0.5 * x)) - math.sqrt(2.0 * x / math.pi) * math.exp(-0.5 * x)


def chi2_3_quantile(p):
    """The x with chi2_3_cdf(x) = p, by bisection (no scipy): the squared Mahalanobis radius that holds a share p of a Gaussian
    cloud in three dimensions -- chi2_3_quantile(0.99) = 11.345 is a `limit` for BatchUprightMPC.mahalanobis. 0 <= p < 1."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("chi2_3_quantile: 0 <= p < 1")
    if p == 0.0:
        return 0.0
    lo, hi = 0.0, 1.0
    while chi2_3_cdf(hi) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if chi2_3_cdf(mid) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ---- error propagators (umpcBatchLagMoments / umpcBatchPropagators) ---------------------------------------------------------
XMOM_ROWS, PROP_ROWS = 96, 80
# lag-moment rows, per (step, group): members scored / skipped, S1a = sum z_a [6], S1b = sum z_b [6], S2a and S2b [21] (upper
# triangles in DISP_PAIRS order), Sba[i][j] = sum z_b,i z_a,j [36] row-major; a = step k, b = step k + lag
X_N, X_SKIPPED, X_S1A, X_S1B, X_S2A, X_S2B, X_SBA, X_END = 0, 1, 2, 8, 14, 35, 56, 92
# propagator rows: n, skipped, status, r2 of the position and of the velocity block, growth, Phi [6, 6] row-major, c [6],
# Q [21] (upper triangle in DISP_PAIRS order)
P_N, P_SKIPPED, P_STATUS, P_R2_P, P_R2_V, P_GROWTH, P_PHI, P_C, P_Q, P_END = 0, 1, 2, 3, 4, 5, 8, 44, 50, 71
PROP_OK, PROP_FEW, PROP_NOT_PD = 0, 1, 2
PROP_MIN_MEMBERS = 8        # one more than the seven coefficients of a row of the fit z_b,i ~ Phi[i] z_a + c_i
PROP_PIVOT_TOL = 1e-10      # a Cholesky pivot of C_a fails when it is <= PROP_PIVOT_TOL * C_a[j][j]
LAG_MAX = 1 << 20


def lag_moments_reference(state_hist, ref, first, count, ref_first, after, lag, order, offset, dtype=np.float64):
    """umpcBatchLagMoments in numpy, IN THE DEVICE'S ORDER OF SUMMATION: [count, G, 96] float64. Row i pairs state slice
    first + after + i (a) with first + after + i + lag (b), reference slice ref_first + i with ref_first + i + lag (a constant
    reference [9, B] serves both). A member is scored when all 24 words are finite (_error_state's rule at a and at b); the
    order of a row is dispersion_reference's: lane l of 64 starts at +0 and adds the terms of members l, l + 64, .. in order,
    then for w = 32, 16, .., 1 lane l becomes (lane l) + (lane l ^ w)."""
    st = np.asarray(state_hist)
    ref = np.asarray(ref)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after, lag = int(first), int(count), int(ref_first), int(bool(after)), int(lag)
    G = len(offset) - 1
    if count < 0 or first < 0 or ref_first < 0 or G < 1 or not 1 <= lag <= LAG_MAX:
        raise ValueError("lag_moments_reference: bad argument")
    xmom = np.zeros((count, G, XMOM_ROWS))
    lanes = np.arange(64)
    nt = X_END - X_S1A
    for i in range(count):
        oka, za = _error_state(st[first + i + after], ref[ref_first + i] if ref.ndim == 3 else ref, dtype)
        okb, zb = _error_state(st[first + i + after + lag], ref[ref_first + i + lag] if ref.ndim == 3 else ref, dtype)
        ok = oka & okb
        za, zb = np.where(ok, za, 0.0), np.where(ok, zb, 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            terms = np.concatenate([za, zb, np.stack([za[a] * za[b] for a, b in DISP_PAIRS]),
                                    np.stack([zb[a] * zb[b] for a, b in DISP_PAIRS]),
                                    np.stack([zb[a] * za[b] for a in range(6) for b in range(6)])])       # [90, B]
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            part = np.zeros((nt, 64))
            for m0 in range(0, len(mem), 64):
                t = terms[:, mem[m0:m0 + 64]]
                part[:, :t.shape[1]] = part[:, :t.shape[1]] + t
            with np.errstate(over="ignore", invalid="ignore"):
                for w in (32, 16, 8, 4, 2, 1):
                    part = part + part[:, lanes ^ w]
            scored = int(ok[mem].sum())
            xmom[i, g, X_N], xmom[i, g, X_SKIPPED] = scored, len(mem) - scored
            xmom[i, g, X_S1A:X_END] = part[:, 0]
    return xmom


def combine_lag_moments(parts):
    """The lag moments of a whole job from the moments [count, G, 96] of its blocks of robots, or of the column blocks a cell
    is split over, all at the same lag: raw moments add, so rows 0..91 are sums (counts exactly; the others to the rounding of
    one more addition per part), as in combine_dispersions. numpy arrays or torch tensors; the result is of the first part's
    kind and the parts are not modified. propagators() / propagator_reference of the result is the map of the whole cell."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_lag_moments: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        total[..., :X_END] = total[..., :X_END] + p[..., :X_END]
    return total


def _pair(i, j):
    """the entry of an upper triangle in DISP_PAIRS order that holds (i, j) or (j, i)"""
    i, j = min(i, j), max(i, j)
    return i * 6 - i * (i - 1) // 2 + (j - i)


def propagator_reference(xmom):
    """umpcBatchPropagators in numpy fp64, THE DEFINITION OF THE KERNEL'S OPERATION ORDER: [.., 80] from the lag moments
    [.., 96]. m_a = S1a / n, m_b = S1b / n; every covariance entry (S - S1_i S1_j / n) / (n - 1) as ellipsoid_reference forms
    it. C_a = L L^T row by row (s = C_a[j][j]; s -= L[j][k]^2, k ascending; pivot_j = s; L[j][j] = sqrt(s); L[i][j] =
    (C_a[i][j] - sum_k L[i][k] L[j][k]) / L[j][j]); Y = L^-1 C_ba^T and W = L^-1 Y^T by forward substitution column by column,
    growth = sum W^2 / 6 row by row; X = L^-T Y by back substitution (k = i + 1 .. 5 ascending), Phi = X^T = C_ba C_a^-1;
    c = m_b - Phi m_a; Q = C_b - Phi C_ba^T; r2 = 1 - trace(Q block) / trace(C_b block), NaN where that trace is 0. Status
    PROP_FEW when n < 8, PROP_NOT_PD when a pivot is <= PROP_PIVOT_TOL * C_a[j][j] or NaN; then rows 3..5 and 8..70 are NaN.
    The affine model is z_b ~ Phi z_a + c and Q the covariance it leaves unexplained."""
    xmom = np.asarray(xmom, np.float64)
    if xmom.shape[-1] != XMOM_ROWS:
        raise ValueError("propagator_reference: xmom must be [.., 96]")
    prop = np.zeros(xmom.shape[:-1] + (PROP_ROWS,))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = xmom[..., X_N]
        n1 = n - 1.0
        few = ~(n >= float(PROP_MIN_MEMBERS))
        s1a = [xmom[..., X_S1A + j] for j in range(6)]
        s1b = [xmom[..., X_S1B + j] for j in range(6)]
        ma, mb = [s / n for s in s1a], [s / n for s in s1b]
        ca = [(xmom[..., X_S2A + k] - s1a[i] * s1a[j] / n) / n1 for k, (i, j) in enumerate(DISP_PAIRS)]
        cb = [(xmom[..., X_S2B + k] - s1b[i] * s1b[j] / n) / n1 for k, (i, j) in enumerate(DISP_PAIRS)]
        cba = [[(xmom[..., X_SBA + 6 * i + j] - s1b[i] * s1a[j] / n) / n1 for j in range(6)] for i in range(6)]
        L = [[None] * 6 for _ in range(6)]
        bad = np.zeros(n.shape, bool)
        for j in range(6):
            s = ca[_pair(j, j)]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            bad = bad | ~(s > PROP_PIVOT_TOL * ca[_pair(j, j)])
            L[j][j] = np.sqrt(s)
            for i in range(j + 1, 6):
                t = ca[_pair(j, i)]
                for k in range(j):
                    t = t - L[i][k] * L[j][k]
                L[i][j] = t / L[j][j]
        y = [[None] * 6 for _ in range(6)]
        w = [[None] * 6 for _ in range(6)]
        for c in range(6):
            for i in range(6):
                s = cba[c][i]
                for k in range(i):
                    s = s - L[i][k] * y[k][c]
                y[i][c] = s / L[i][i]
        for c in range(6):
            for i in range(6):
                s = y[c][i]
                for k in range(i):
                    s = s - L[i][k] * w[k][c]
                w[i][c] = s / L[i][i]
        gsum = np.zeros_like(n)
        for i in range(6):
            for c in range(6):
                gsum = gsum + w[i][c] * w[i][c]
        growth = gsum / 6.0
        for c in range(6):
            for i in range(5, -1, -1):
                s = y[i][c]
                for k in range(i + 1, 6):
                    s = s - L[k][i] * y[k][c]
                y[i][c] = s / L[i][i]
        phi = [[y[j][i] for j in range(6)] for i in range(6)]
        prop[..., P_N], prop[..., P_SKIPPED] = n, xmom[..., X_SKIPPED]
        prop[..., P_STATUS] = np.where(few, PROP_FEW, np.where(bad, PROP_NOT_PD, PROP_OK))
        prop[..., P_GROWTH] = growth
        for i in range(6):
            s = mb[i]
            for j in range(6):
                prop[..., P_PHI + 6 * i + j] = phi[i][j]
                s = s - phi[i][j] * ma[j]
            prop[..., P_C + i] = s
        q = []
        for k, (i, j) in enumerate(DISP_PAIRS):
            s = cb[k]
            for t in range(6):
                s = s - phi[i][t] * cba[j][t]
            q.append(s)
            prop[..., P_Q + k] = s
        for row, blk in ((P_R2_P, (0, 1, 2)), (P_R2_V, (3, 4, 5))):
            d = [_pair(t, t) for t in blk]
            den = (cb[d[0]] + cb[d[1]]) + cb[d[2]]
            prop[..., row] = np.where(den == 0.0, np.nan, 1.0 - ((q[d[0]] + q[d[1]]) + q[d[2]]) / den)
        none = few | bad
        prop[..., P_R2_P:P_GROWTH + 1][none] = np.nan
        prop[..., P_PHI:P_END][none] = np.nan
    return prop


def propagator_poles(prop, lag=1):
    """The poles of each usable row of prop [count, G, 80] (propagators() downloaded, or propagator_reference): [count, G, 6]
    complex, numpy.linalg.eigvals of Phi, and for lag > 1 the principal lag-th root of each (Phi carries a deviation over
    `lag` steps, so its eigenvalues are the lag-th powers of the per-step poles; which of the lag roots the plant has is not in
    the data: the principal one is right while a pole turns less than half a revolution in `lag` steps). NaN where the status
    is not PROP_OK. The decay rate per step of a mode is log|lambda| (negative: it contracts; the slowest mode is the largest)
    and its frequency angle(lambda) / (2 pi) cycles per step. No order is imposed on the six. CPU only: eigenvalues of a
    6 x 6 non-symmetric matrix are not hot-path work."""
    prop = np.asarray(prop, np.float64)
    lag = int(lag)
    if prop.ndim != 3 or prop.shape[-1] != PROP_ROWS or lag < 1:
        raise ValueError("propagator_poles: prop must be [count, G, 80] and lag >= 1")
    poles = np.full(prop.shape[:2] + (6,), np.nan + 0j, np.complex128)
    use = prop[..., P_STATUS] == PROP_OK
    if use.any():
        lam = np.linalg.eigvals(prop[..., P_PHI:P_C][use].reshape(-1, 6, 6)).astype(np.complex128)
        poles[use] = lam if lag == 1 else np.abs(lam) ** (1.0 / lag) * np.exp(1j * np.angle(lam) / lag)
    return poles


# ---- sensitivity indices (umpcBatchFactorBins / umpcBatchSensitivity / umpcBatchSensitivityIndices / umpcBatchScoreSensitivity) --
SENS_MAX_FACTORS, SENS_MAX_BINS = 6, 8
# sum rows, per (step, group): members scored / skipped, S1 = sum y, S2 = sum y^2, then N_fm at S_BINS + f M + m (the scored
# members of bin m of factor f) and S_fm = sum y over them at S_BINS + F M + f M + m
S_N, S_SKIPPED, S_S1, S_S2, S_BINS = 0, 1, 2, 3, 4
# index rows: n, skipped, status, mean, variance, SST, two zeros, then per factor f at I_FIRST + f (4 + M): eta2, eps2, F, M_f and
# the M bin means
I_N, I_SKIPPED, I_STATUS, I_MEAN, I_VAR, I_SST, I_FIRST = 0, 1, 2, 3, 4, 5, 8
I_ETA2, I_EPS2, I_F, I_MF, I_BINMEAN = 0, 1, 2, 3, 4
SENS_OK, SENS_FEW, SENS_FLAT = 0, 1, 2


def sens_cols(F, nbins):
    """the length 4 + 2 F M of a row of sums"""
    return S_BINS + 2 * int(F) * int(nbins)


def sens_index_cols(F, nbins):
    """the length 8 + F (4 + M) of a row of indices"""
    return I_FIRST + int(F) * (4 + int(nbins))


def _check_factors(what, F, M):
    if not 1 <= F <= SENS_MAX_FACTORS or not 2 <= M <= SENS_MAX_BINS:
        raise ValueError("%s: 1 to %d factors, 2 to %d bins" % (what, SENS_MAX_FACTORS, SENS_MAX_BINS))


def factor_bins_reference(factors, order, offset, nbins=8):
    """umpcBatchFactorBins in numpy: bins [F, B] int32 from factors [F, B] (any float dtype) and a group index. Per group and
    factor the members with a finite value are ranked by numpy.argsort(kind="stable") over the member list (ties, -0 against +0
    among them, go to the earlier position); bin = rank * M // n_f with n_f the finite members. -1 for a value that is not
    finite and for a robot outside every group. Bins of equal count by rank inside the cell: the given-data estimator of the
    correlation ratio. A categorical factor needs no ranking: write its bins by hand."""
    fac = np.atleast_2d(np.asarray(factors))
    order, offset = np.asarray(order), np.asarray(offset)
    F, M, G = fac.shape[0], int(nbins), len(offset) - 1
    _check_factors("factor_bins_reference", F, M)
    if G < 1 or fac.ndim != 2 or fac.shape[1] != len(order):
        raise ValueError("factor_bins_reference: bad argument")
    bins = np.full(fac.shape, -1, np.int32)
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        for f in range(F):
            v = fac[f, mem]
            at = np.nonzero(np.isfinite(v))[0]
            rank = np.empty(len(at), np.int64)
            rank[np.argsort(v[at], kind="stable")] = np.arange(len(at))
            bins[f, mem[at]] = rank * M // max(len(at), 1)
    return bins


def _dtype_terms(y, o, r, tl, dtype):
    """(ok [B], ep, es, tau2 [B] in `dtype`) of one step IN THE DEVICE'S ARITHMETIC (score_terms, csrc/umpc_score.h): every
    difference, product and sum formed in `dtype` in the order (d0 d0 + d1 d1) + d2 d2; the moments clipped at +-taulim rounded
    to `dtype`; ok as _step_terms has it"""
    y, r = np.asarray(y, dtype), np.asarray(r, dtype)
    p, s, pdes, sdes = y[0:3], y[9:12], r[0:3], r[6:9]
    ok = np.isfinite(p).all(0) & np.isfinite(s).all(0) & np.isfinite(pdes).all(0) & np.isfinite(sdes).all(0)
    with np.errstate(invalid="ignore", over="ignore"):
        d, c = p - pdes, s - sdes
        ep = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        es = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        if o is not None:
            o = np.asarray(o, dtype)
            ok &= np.isfinite(o[1:3]).all(0)
            lim = np.dtype(dtype).type(tl)
            t = np.minimum(np.maximum(o[1:3], -lim), lim)
            tau2 = t[0] * t[0] + t[1] * t[1]
        else:
            tau2 = np.zeros_like(ep)
    return ok, ep, es, tau2


def _sens_rows(y, fin, order, offset, bins, M):
    """[G, 4 + 2 F M]: the rows of one table of values y [B] float64 (fin [B]: the value enters) IN THE DEVICE'S ORDER OF
    SUMMATION: lane l of 64 starts at +0 and adds the terms of members l, l + 64, .. in list order (+0 for a member that is not
    scored or not in the bin), then for w = 32, 16, .., 1 lane l becomes (lane l) + (lane l ^ w)"""
    F, G = bins.shape[0], len(offset) - 1
    ok = fin & ((bins >= 0) & (bins < M)).all(0)
    lanes = np.arange(64)
    with np.errstate(over="ignore", invalid="ignore"):
        yz = np.where(ok, y, 0.0)
        hit = [ok & (bins[f] == m) for f in range(F) for m in range(M)]
        terms = np.stack([yz, np.where(ok, y * y, 0.0)] + [np.where(h, yz, 0.0) for h in hit])       # [2 + F M, B]
    rows = np.zeros((G, sens_cols(F, M)))
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        part = np.zeros((terms.shape[0], 64))
        for m0 in range(0, len(mem), 64):
            t = terms[:, mem[m0:m0 + 64]]
            part[:, :t.shape[1]] = part[:, :t.shape[1]] + t
        with np.errstate(over="ignore", invalid="ignore"):
            for w in (32, 16, 8, 4, 2, 1):
                part = part + part[:, lanes ^ w]
        scored = int(ok[mem].sum())
        rows[g, S_N], rows[g, S_SKIPPED] = scored, len(mem) - scored
        rows[g, S_S1], rows[g, S_S2] = part[0, 0], part[1, 0]
        rows[g, S_BINS:S_BINS + F * M] = [int(h[mem].sum()) for h in hit]
        rows[g, S_BINS + F * M:] = part[2:, 0]
    return rows


def sensitivity_reference(state_hist, out_hist, ref, first, count, ref_first, after, taulim, order, offset, bins, nbins,
                          term=TERM_EP, dtype=np.float64):
    """umpcBatchSensitivity in numpy, IN THE DEVICE'S ARITHMETIC AND ORDER OF SUMMATION: [count, G, 4 + 2 F M] float64. The
    tables, first, count, ref_first, after, order, offset and term are those of ensemble_quantiles_reference, bins [F, B]
    int32 and nbins = M those of factor_bins_reference (or written by hand); dtype is the handle's: the term y of a member is
    formed in it by the expressions of the scoring kernel and widened, y^2 and every sum are float64. A member is scored at a
    step when ensemble_quantiles_reference with the same out_hist scores it and all F of its bins lie in [0, M). Rows: S_*."""
    st, ref = np.asarray(state_hist), np.asarray(ref)
    out = None if out_hist is None else np.asarray(out_hist)
    order, offset, bins = np.asarray(order), np.asarray(offset), np.atleast_2d(np.asarray(bins))
    first, count, ref_first, after, term, M = int(first), int(count), int(ref_first), int(bool(after)), int(term), int(nbins)
    F, G = bins.shape[0], len(offset) - 1
    _check_factors("sensitivity_reference", F, M)
    if (count < 0 or first < 0 or ref_first < 0 or G < 1 or term not in (TERM_EP, TERM_ES, TERM_TAU)
            or (term == TERM_TAU and out is None) or bins.shape[1] != st.shape[-1]):
        raise ValueError("sensitivity_reference: bad argument")
    sens = np.zeros((count, G, sens_cols(F, M)))
    for i in range(count):
        c = first + i
        fin, ep, es, tau2 = _dtype_terms(st[c + after], None if out is None else out[c],
                                         ref[ref_first + i] if ref.ndim == 3 else ref, float(taulim), dtype)
        y = (ep if term == TERM_EP else es if term == TERM_ES else tau2).astype(np.float64)
        sens[i] = _sens_rows(y, fin, order, offset, bins, M)
    return sens


def score_sensitivity_reference(score, order, offset, bins, nbins, num, den=None):
    """umpcBatchScoreSensitivity in numpy: [G, 4 + 2 F M], the sums of sensitivity_reference over one column of a per-robot
    score [12, B]. The value of robot b and whether it enters are those of score_quantiles_reference (score[num, b], or the
    IEEE double quotient by score[den, b]; row 0 > 0 and the value finite); all F of its bins must lie in [0, M) as well."""
    sc = np.asarray(score)
    order, offset, bins = np.asarray(order), np.asarray(offset), np.atleast_2d(np.asarray(bins))
    num, den, M = int(num), -1 if den is None else int(den), int(nbins)
    _check_factors("score_sensitivity_reference", bins.shape[0], M)
    if len(offset) < 2 or not 0 <= num < SCORE_ROWS or not -1 <= den < SCORE_ROWS or bins.shape[1] != sc.shape[1]:
        raise ValueError("score_sensitivity_reference: bad argument")
    x, fin = _table_value(sc, num, den)
    return _sens_rows(x, fin, order, offset, bins, M)


def sensitivity_indices_reference(sens, F, nbins):
    """umpcBatchSensitivityIndices in numpy fp64, THE DEFINITION OF THE KERNEL'S OPERATION ORDER: [.., 8 + F (4 + M)] from the
    sums [.., 4 + 2 F M]. mean = S1 / n; c = S1 * S1 / n; SST = S2 - c; variance = SST / (n - 1). Per factor: a = +0 and, over
    the non-empty bins with m ascending, a = a + S_fm * S_fm / N_fm; SSB = a - c; eta2 = SSB / SST, the correlation ratio: the
    share of the variance of y that the bin means of the factor explain; eps2 = 1 - ((1 - eta2) * (n - 1)) / (n - M_f), its
    bias-adjusted form (with no effect eta2 averages (M_f - 1) / (n - 1), eps2 zero); F = (SSB / (M_f - 1)) / ((SST - SSB) /
    (n - M_f)), the one-way ANOVA statistic; M_f the non-empty bins; the bin means S_fm / N_fm, NaN for an empty bin. Status
    SENS_FEW when n < 2 M, SENS_FLAT when not SST > 0 or S1 or S2 is not finite: eta2, eps2 and F of every factor are then NaN,
    as they are for a factor with M_f < 2 or n <= M_f. Nothing is clamped."""
    sens = np.asarray(sens, np.float64)
    F, M = int(F), int(nbins)
    _check_factors("sensitivity_indices_reference", F, M)
    if sens.shape[-1] != sens_cols(F, M):
        raise ValueError("sensitivity_indices_reference: sens must be [.., %d]" % sens_cols(F, M))
    idx = np.zeros(sens.shape[:-1] + (sens_index_cols(F, M),))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n, s1, s2 = sens[..., S_N], sens[..., S_S1], sens[..., S_S2]
        c = s1 * s1 / n
        sst, n1 = s2 - c, n - 1.0
        few = ~(n >= 2.0 * M)
        bad = ~(sst > 0.0) | ~np.isfinite(s1) | ~np.isfinite(s2)
        none = few | bad
        idx[..., I_N], idx[..., I_SKIPPED] = n, sens[..., S_SKIPPED]
        idx[..., I_STATUS] = np.where(few, SENS_FEW, np.where(bad, SENS_FLAT, SENS_OK))
        idx[..., I_MEAN], idx[..., I_VAR], idx[..., I_SST] = s1 / n, sst / n1, sst
        for f in range(F):
            at = I_FIRST + f * (4 + M)
            acc, mf = np.zeros_like(n), np.zeros_like(n)
            for m in range(M):
                nm, sm = sens[..., S_BINS + f * M + m], sens[..., S_BINS + F * M + f * M + m]
                has = nm > 0.0
                acc = np.where(has, acc + sm * sm / nm, acc)
                mf = np.where(has, mf + 1.0, mf)
                idx[..., at + I_BINMEAN + m] = np.where(has, sm / nm, np.nan)
            ssb = acc - c
            eta = ssb / sst
            eps = 1.0 - ((1.0 - eta) * n1) / (n - mf)
            fst = (ssb / (mf - 1.0)) / ((sst - ssb) / (n - mf))
            nof = none | ~(mf >= 2.0) | ~(n > mf)
            idx[..., at + I_ETA2] = np.where(nof, np.nan, eta)
            idx[..., at + I_EPS2] = np.where(nof, np.nan, eps)
            idx[..., at + I_F] = np.where(nof, np.nan, fst)
            idx[..., at + I_MF] = mf
    return idx


def combine_sensitivities(parts):
    """The sums of a whole job from the sums [.., 4 + 2 F M] of its blocks of robots, or of the column blocks a cell is split
    over: every row is a raw sum, so the rows add (counts exactly; the others to the rounding of one more addition per part) --
    PROVIDED THE BINS WERE ASSIGNED ON THE WHOLE JOB: factor_bins of a block ranks inside the block and cuts other bins. numpy
    arrays or torch tensors; the result is of the first part's kind and the parts are not modified.
    sensitivity_indices / sensitivity_indices_reference of the result are the indices of the whole cell."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_sensitivities: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        total = total + p
    return total


# ----------------------------------------------------------------------------------------------------------------------
# Error spectra (umpcBatchSpectrumInit / umpcBatchSpectrum / umpcBatchSpectrumPower / umpcBatchSpectrumGroups): per robot
# the projection of a 3-channel signal onto K windowed cosine / sine pairs, its periodogram and chatter score; per group the
# periodogram summed over the members
# ----------------------------------------------------------------------------------------------------------------------
SPEC_ROWS, SPEC_MAX_K = 12, 64
SPEC_SLICES = 2             # UMPC_SPEC_SLICES (csrc/umpc_spectrum.h): wavefronts a call's step range is split over
SPEC_EP, SPEC_ES, SPEC_U = 0, 1, 2
SPEC_SIGNALS = ("ep", "es", "u")      # p - pdes, s - sdes, the recorded command (out rows 0..2)
SPEC_WINDOWS = ("hann", "rect")
# sum rows: n, skipped, then per channel c at SSUM_CHANNEL + c (2 + 2 K): sum w y, sum w y y, then (C_j, S_j) per frequency
SSUM_N, SSUM_SKIPPED, SSUM_CHANNEL = 0, 1, 2
SSUM_WY, SSUM_WYY, SSUM_BINS = 0, 1, 2
# spectrum rows, per channel (row 0 > 0 means "enters", as in a score)
(SPEC_STEPS, SPEC_SKIPPED, SPEC_MEAN, SPEC_VAR, SPEC_TOTAL, SPEC_PEAK_BIN, SPEC_PEAK_HZ, SPEC_PEAK_POWER, SPEC_PEAK_SHARE,
 SPEC_CENTROID_HZ, SPEC_BANDWIDTH_HZ, SPEC_HIGH_SHARE) = range(12)
SPEC_ROW_NAMES = ("steps", "skipped", "mean", "var", "total", "peak_bin", "peak_hz", "peak_power", "peak_share", "centroid_hz",
                  "bandwidth_hz", "high_share")
# group rows, per (group, channel): members that enter, members that do not, then the sum of P_j per frequency
GSPEC_N, GSPEC_SKIPPED, GSPEC_FIRST = 0, 1, 2


def spectrum_sum_rows(K):
    """rows of the sums of umpcBatchSpectrum for K frequencies: 2 + 3 (2 + 2 K)"""
    K = int(K)
    if not 1 <= K <= SPEC_MAX_K:
        raise ValueError("1 <= K <= %d frequencies" % SPEC_MAX_K)
    return 2 + 3 * (2 + 2 * K)


def spectrum_identity(K, B):
    """The sums no step has entered (umpcBatchSpectrumInit): zeros [2 + 3 (2 + 2 K), B] float64."""
    return np.zeros((spectrum_sum_rows(K), int(B)))


def spectrum_basis(nu, W, window="hann", step0=0):
    """The basis table of umpcBatchSpectrum, float64 [W, 1 + 2 K]: row k holds the window weight w_k, then per frequency j
    w_k cos(2 pi u_jk) and w_k sin(2 pi u_jk) with the phase of response_phase(step0 + k, nu) -- one double multiply, exact
    zeros and ones at the quarter points, the same whatever step0 is. nu [K]: revolutions per step, each strictly inside
    (0, 0.5): the power kernel reads a bin with the factor 4 / W0^2 of a frequency between 0 and half the step rate; at 0
    and 0.5 the sine column is zero and the factor is another one. window: "rect" (w = 1) or "hann" (the periodic Hann
    window w_k = 0.5 - 0.5 cos(2 pi k / W)); the window counts rows from 0, step0 moves the phase origin only."""
    nu = np.atleast_1d(np.asarray(nu, np.float64))
    W, step0 = int(W), int(step0)
    if nu.ndim != 1 or not 1 <= len(nu) <= SPEC_MAX_K:
        raise ValueError("spectrum_basis: 1 <= K <= %d frequencies" % SPEC_MAX_K)
    if not np.all((nu > 0.0) & (nu < 0.5)):
        raise ValueError("spectrum_basis: every nu must lie strictly inside (0, 0.5) revolutions per step")
    if W < 1 or step0 < 0 or step0 + W > 1 << 53 or window not in SPEC_WINDOWS:
        raise ValueError("spectrum_basis: bad argument (W >= 1, 0 <= step0, window is 'hann' or 'rect')")
    basis = np.empty((W, 1 + 2 * len(nu)))
    inv = np.array([1.0 / W])
    for k in range(W):
        w = 1.0 if window == "rect" else 0.5 - 0.5 * response_phase(k, inv)[0][0]
        c, s, _ = response_phase(step0 + k, nu)
        basis[k, 0] = w
        basis[k, 1::2] = w * c
        basis[k, 2::2] = w * s
    return basis


def spectrum_wsum(basis, basis_first=0, count=None):
    """wsum [1 + 2 K] of umpcBatchSpectrumPower: the column sums of rows basis_first .. basis_first + count - 1 of the basis,
    added sequentially in row order from +0."""
    basis = np.asarray(basis, np.float64)
    first = int(basis_first)
    count = basis.shape[0] - first if count is None else int(count)
    if basis.ndim != 2 or first < 0 or count < 0 or first + count > basis.shape[0]:
        raise ValueError("spectrum_wsum: the rows asked for are not inside the basis")
    total = np.zeros(basis.shape[1])
    for k in range(first, first + count):
        total = total + basis[k]
    return total


def _spectrum_signal(signal):
    if signal in SPEC_SIGNALS:
        return SPEC_SIGNALS.index(signal)
    if signal in (SPEC_EP, SPEC_ES, SPEC_U):
        return int(signal)
    raise ValueError("signal is one of %s" % (SPEC_SIGNALS,))


def spectrum_sums_reference(signal, state_hist, out_hist, ref, basis, basis_first, first, count, ref_first, after,
                            dtype=np.float64, sums=None):
    """umpcBatchSpectrum in numpy, IN THE DEVICE'S ORDER OF SUMMATION: the sums [2 + 3 (2 + 2 K), B] float64. signal "ep" / "es"
    / "u"; state_hist [.., 18, B], ref -- a table [.., 9, B] (slice ref_first + i) or one constant reference [9, B] --, first,
    count, ref_first and after are those of response_sums_reference; "u" reads rows 0..2 of out_hist [.., 9, B], slice first
    + i, and neither state_hist nor ref. dtype is the handle's: a difference is formed in it with one rounding, everything
    after is float64. basis [W, 1 + 2 K]: step i reads row basis_first + i. A step enters for a robot when every word it reads
    is finite; otherwise it is counted in row 1 and its value is +0 in every product. Slice s of SPEC_SLICES adds steps s,
    s + SPEC_SLICES, .. in order from +0, the partial sums are added in the order 0, 1, .. and the total is added to `sums`
    (passing one back in accumulates). Elementwise IEEE operations in that order: the kernel's bits."""
    sig = _spectrum_signal(signal)
    basis = np.asarray(basis, np.float64)
    first, count, ref_first, after, basis_first = int(first), int(count), int(ref_first), int(bool(after)), int(basis_first)
    if basis.ndim != 2 or basis.shape[1] < 3 or basis.shape[1] % 2 != 1:
        raise ValueError("spectrum_sums_reference: basis must be [W, 1 + 2 K]")
    K = (basis.shape[1] - 1) // 2
    rows = spectrum_sum_rows(K)
    if count < 0 or first < 0 or ref_first < 0 or basis_first < 0 or basis_first + count > basis.shape[0]:
        raise ValueError("spectrum_sums_reference: bad argument")
    if sig == SPEC_U:
        if out_hist is None:
            raise ValueError("spectrum_sums_reference: signal 'u' needs out_hist")
        src = np.asarray(out_hist, dtype)
    else:
        src = np.asarray(state_hist, dtype)
        ref = np.asarray(ref, dtype)
    B = src.shape[-1]
    sm = spectrum_identity(K, B) if sums is None else np.array(sums, np.float64)
    if sm.shape != (rows, B):
        raise ValueError("spectrum_sums_reference: sums must be [%d, %d]" % (rows, B))
    chan = 2 + 2 * K
    total = None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(SPEC_SLICES):
            part = np.zeros((rows, B))
            for i in range(s, count, SPEC_SLICES):
                if sig == SPEC_U:
                    y = src[first + i, 0:3]
                    ok, d = np.isfinite(y).all(0), y
                else:
                    y0, r0 = (0, 0) if sig == SPEC_EP else (9, 6)
                    y = src[first + i + after, y0:y0 + 3]
                    r = (ref[ref_first + i] if ref.ndim == 3 else ref)[r0:r0 + 3]
                    ok, d = np.isfinite(y).all(0) & np.isfinite(r).all(0), y - r
                v = np.where(ok, d.astype(np.float64), 0.0)                    # [3, B]
                row = basis[basis_first + i]
                part[SSUM_N] += ok
                part[SSUM_SKIPPED] += ~ok
                for c in range(3):
                    at = SSUM_CHANNEL + c * chan
                    t = row[0] * v[c]
                    part[at + SSUM_WY] += t
                    part[at + SSUM_WYY] += t * v[c]
                    part[at + SSUM_BINS:at + chan] += v[c][None, :] * row[1:, None]
            total = part if total is None else total + part
        sm = sm + total
    return sm


def spectrum_power_reference(sums, wsum, freq_hz, nrows, jsplit):
    """umpcBatchSpectrumPower in numpy fp64, in the kernel's operation order: (spec [3, 12, B], power [3, K, B]) float64 from
    the sums [2 + 3 (2 + 2 K), B], the window's column sums wsum [1 + 2 K] (spectrum_wsum), the frequencies freq_hz [K], the
    number of basis rows wsum was taken over and the first bin of the high band. Per channel: m = sum wy / W0, var = sum wyy /
    W0 - m m, A_j = C_j - m Wc_j, B_j = S_j - m Ws_j, P_j = (4 (A_j A_j + B_j B_j)) / (W0 W0); total, the centroid's numerator
    sum f_j P_j and the high band's sum are added with j ascending from +0, the peak is the first maximum; then the bandwidth's
    numerator sum ((f_j - centroid) (f_j - centroid)) P_j. Refused (row 0 = 0, rows 2..11 and the channel's power NaN) when
    skipped > 0, n != nrows, n < 2 or total is not > 0 and finite. The device rounds to the handle's dtype at the store."""
    sm = np.asarray(sums, np.float64)
    wsum, f = np.asarray(wsum, np.float64), np.atleast_1d(np.asarray(freq_hz, np.float64))
    K = len(f)
    nrows, jsplit = int(nrows), int(jsplit)
    if sm.ndim != 2 or f.ndim != 1 or sm.shape[0] != spectrum_sum_rows(K) or wsum.shape != (1 + 2 * K,):
        raise ValueError("spectrum_power_reference: sums must be [2 + 3 (2 + 2 K), B], wsum [1 + 2 K], freq_hz [K]")
    if nrows < 0 or not 0 <= jsplit <= K:
        raise ValueError("spectrum_power_reference: bad argument (nrows >= 0, 0 <= jsplit <= K)")
    B = sm.shape[1]
    spec, power = np.full((3, SPEC_ROWS, B), np.nan), np.full((3, K, B), np.nan)
    n, skipped = sm[SSUM_N], sm[SSUM_SKIPPED]
    w0 = wsum[0]
    w02 = w0 * w0
    counts = (skipped > 0.0) | (n != float(nrows)) | ~(n >= 2.0)
    chan = 2 + 2 * K
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(3):
            ch = sm[SSUM_CHANNEL + c * chan:SSUM_CHANNEL + (c + 1) * chan]
            m = ch[SSUM_WY] / w0
            var = ch[SSUM_WYY] / w0 - m * m
            P = np.empty((K, B))
            total, peak, cnum, high = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
            jpeak = np.zeros(B, np.int64)
            for j in range(K):
                A = ch[SSUM_BINS + 2 * j] - m * wsum[1 + 2 * j]
                Bq = ch[SSUM_BINS + 2 * j + 1] - m * wsum[2 + 2 * j]
                P[j] = (4.0 * (A * A + Bq * Bq)) / w02
                total = total + P[j]
                better = (P[j] > peak) if j else np.ones(B, bool)
                peak = np.where(better, P[j], peak)
                jpeak = np.where(better, j, jpeak)
                cnum = cnum + f[j] * P[j]
                high = high + (P[j] if j >= jsplit else 0.0)
            cen = cnum / total
            refused = counts | ~(total > 0.0) | ~np.isfinite(total)
            bnum = np.zeros(B)
            for j in range(K):
                d = f[j] - cen
                bnum = bnum + (d * d) * P[j]
            o = spec[c]
            o[SPEC_STEPS] = n
            o[SPEC_MEAN], o[SPEC_VAR], o[SPEC_TOTAL] = m, var, total
            o[SPEC_PEAK_BIN], o[SPEC_PEAK_HZ], o[SPEC_PEAK_POWER] = jpeak, f[jpeak], peak
            o[SPEC_PEAK_SHARE], o[SPEC_CENTROID_HZ] = peak / total, cen
            o[SPEC_BANDWIDTH_HZ], o[SPEC_HIGH_SHARE] = np.sqrt(bnum / total), high / total
            o[2:, refused] = np.nan
            o[SPEC_STEPS, refused] = 0.0
            o[SPEC_SKIPPED] = skipped
            power[c] = np.where(refused, np.nan, P)
    return spec, power


def spectrum_groups_reference(power, spec, order, offset):
    """umpcBatchSpectrumGroups in numpy, IN THE DEVICE'S ORDER OF SUMMATION: [G, 3, 2 + K] float64 from power [3, K, B] and
    spec [3, 12, B] as the device holds them (in the handle's dtype; widened here) and the tables of group_index. Per group
    and channel: the members that enter (row 0 of spec[c] > 0), the members that do not, and per frequency the sum of P_j over
    the members that enter, in dispersion_reference's order: lane l of 64 starts at +0 and adds members l, l + 64, .. of the
    list in order (+0 for a member that does not enter), then for w = 32, 16, .., 1 lane l becomes (lane l) + (lane l ^ w)."""
    power, spec = np.asarray(power), np.asarray(spec)
    order, offset = np.asarray(order), np.asarray(offset)
    G, K = len(offset) - 1, power.shape[1]
    if G < 1 or power.ndim != 3 or spec.shape != (3, SPEC_ROWS, power.shape[2]) or not 1 <= K <= SPEC_MAX_K:
        raise ValueError("spectrum_groups_reference: bad argument")
    out = np.zeros((G, 3, 2 + K))
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            for c in range(3):
                ok = spec[c, SPEC_STEPS, mem] > 0
                terms = np.where(ok[None, :], power[c][:, mem].astype(np.float64), 0.0)          # [K, members]
                part = np.zeros((K, 64))
                for m0 in range(0, len(mem), 64):
                    t = terms[:, m0:m0 + 64]
                    part[:, :t.shape[1]] = part[:, :t.shape[1]] + t
                for w in (32, 16, 8, 4, 2, 1):
                    part = part + part[:, lanes ^ w]
                out[g, c, GSPEC_N], out[g, c, GSPEC_SKIPPED] = ok.sum(), len(mem) - ok.sum()
                out[g, c, GSPEC_FIRST:] = part[:, 0]
    return out


def combine_spectra(parts):
    """The group table of a whole job from the tables [G, 3, 2 + K] of its blocks of robots, or of the column blocks a cell
    is split over: every column is a raw sum, so the tables add (counts exactly; the powers to the rounding of one more
    addition per part). numpy arrays or torch tensors; the result is of the first part's kind and the parts are not modified.
    Column 2 + j divided by column 0 is the cell's averaged periodogram."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_spectra: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        total = total + p
    return total


# ----------------------------------------------------------------------------------------------------------------------
# Transfer estimates (umpcBatchCrossSpectrumInit / umpcBatchCrossSpectrum / umpcBatchCrossSpectrumGroups / umpcBatchTransfer):
# per robot the projections of an input x and an output y onto the basis of the spectrum; per group the auto- and
# cross-periodograms summed over the draws; from those the H1 transfer function, the coherence and the random error
# ----------------------------------------------------------------------------------------------------------------------
XS_TRACK, XS_ATT, XS_PUSH = 0, 1, 2
XS_PAIRS = ("track", "att", "push")       # pdes -> p, sdes -> s, dv_world of the impulse table -> p - pdes
XS_CHANNELS = 6                           # blocks of the sums: x0 x1 x2 y0 y1 y2, each in the layout of a spectrum channel
# group rows, per (group, channel): members that enter, members that do not, then (Sxx, Syy, Cxy, Qxy) per frequency
GX_N, GX_SKIPPED, GX_FIRST = 0, 1, 2
GX_SXX, GX_SYY, GX_CXY, GX_QXY = range(4)
TF_ROWS = 12
(TF_N, TF_SKIPPED, TF_PXX, TF_PYY, TF_H_RE, TF_H_IM, TF_GAIN, TF_PHASE, TF_COH, TF_GAIN_H2, TF_REL_ERR, TF_NOISE) = range(12)
TF_ROW_NAMES = ("n", "skipped", "pxx", "pyy", "h_re", "h_im", "gain", "phase", "coh", "gain_h2", "rel_err", "noise")


def cross_spectrum_sum_rows(K):
    """rows of the sums of umpcBatchCrossSpectrum for K frequencies: 2 + 6 (2 + 2 K)"""
    K = int(K)
    if not 1 <= K <= SPEC_MAX_K:
        raise ValueError("1 <= K <= %d frequencies" % SPEC_MAX_K)
    return 2 + XS_CHANNELS * (2 + 2 * K)


def cross_spectrum_identity(K, B):
    """The sums no step has entered (umpcBatchCrossSpectrumInit): zeros [2 + 6 (2 + 2 K), B] float64."""
    return np.zeros((cross_spectrum_sum_rows(K), int(B)))


def _cross_pair(pair):
    if pair in XS_PAIRS:
        return XS_PAIRS.index(pair)
    if pair in (XS_TRACK, XS_ATT, XS_PUSH):
        return int(pair)
    raise ValueError("pair is one of %s" % (XS_PAIRS,))


def cross_spectrum_sums_reference(pair, state_hist, ref, impulses, basis, basis_first, first, count, ref_first, imp_first, after,
                                  dtype=np.float64, sums=None):
    """umpcBatchCrossSpectrum in numpy, IN THE DEVICE'S ORDER OF SUMMATION: the sums [2 + 6 (2 + 2 K), B] float64. pair "track"
    (x = pdes, reference rows 0..2; y = p, state rows 0..2), "att" (x = sdes, reference rows 6..8; y = s, state rows 9..11) or
    "push" (x = dv_world, rows 0..2 of impulses [.., 6, B], slice imp_first + i; y = p - pdes formed in `dtype` with one
    rounding). state_hist [.., 18, B] is read at slice first + i + after; ref is a table [.., 9, B] read at slice ref_first +
    i -- "track" and "att" take nothing else: a constant reference has no spectrum -- or, for "push" alone, one constant
    reference [9, B]. basis, basis_first and the order of summation are spectrum_sums_reference's; the blocks of the sums
    are x0 x1 x2 y0 y1 y2, each in the layout of a spectrum channel. A step enters for a robot when every word it reads for
    BOTH signals is finite; otherwise row 1 counts it and its value is +0 in every product of both signals. Passing `sums`
    back in accumulates. Elementwise IEEE operations in the kernel's order: the kernel's bits."""
    pr = _cross_pair(pair)
    basis = np.asarray(basis, np.float64)
    first, count, ref_first, imp_first = int(first), int(count), int(ref_first), int(imp_first)
    after, basis_first = int(bool(after)), int(basis_first)
    if basis.ndim != 2 or basis.shape[1] < 3 or basis.shape[1] % 2 != 1:
        raise ValueError("cross_spectrum_sums_reference: basis must be [W, 1 + 2 K]")
    K = (basis.shape[1] - 1) // 2
    rows = cross_spectrum_sum_rows(K)
    if count < 0 or first < 0 or ref_first < 0 or imp_first < 0 or basis_first < 0 or basis_first + count > basis.shape[0]:
        raise ValueError("cross_spectrum_sums_reference: bad argument")
    if ref is None:
        raise ValueError("cross_spectrum_sums_reference: a reference must be given")
    src, ref = np.asarray(state_hist, dtype), np.asarray(ref, dtype)
    if pr == XS_PUSH:
        if impulses is None:
            raise ValueError("cross_spectrum_sums_reference: pair 'push' needs the impulse table")
        imp = np.asarray(impulses, dtype)
    elif ref.ndim != 3:
        raise ValueError("cross_spectrum_sums_reference: pairs 'track' and 'att' need a reference table (a constant reference has no spectrum)")
    B = src.shape[-1]
    sm = cross_spectrum_identity(K, B) if sums is None else np.array(sums, np.float64)
    if sm.shape != (rows, B):
        raise ValueError("cross_spectrum_sums_reference: sums must be [%d, %d]" % (rows, B))
    chan = 2 + 2 * K
    total = None
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(SPEC_SLICES):
            part = np.zeros((rows, B))
            for i in range(s, count, SPEC_SLICES):
                if pr == XS_PUSH:
                    x = imp[imp_first + i, 0:3]
                    y = src[first + i + after, 0:3]
                    r = (ref[ref_first + i] if ref.ndim == 3 else ref)[0:3]
                    ok, d = np.isfinite(x).all(0) & np.isfinite(y).all(0) & np.isfinite(r).all(0), y - r
                else:
                    y0, r0 = (0, 0) if pr == XS_TRACK else (9, 6)
                    x = ref[ref_first + i, r0:r0 + 3]
                    d = src[first + i + after, y0:y0 + 3]
                    ok = np.isfinite(x).all(0) & np.isfinite(d).all(0)
                v = np.where(ok, np.concatenate((x, d)).astype(np.float64), 0.0)            # [6, B]
                row = basis[basis_first + i]
                part[SSUM_N] += ok
                part[SSUM_SKIPPED] += ~ok
                for c in range(XS_CHANNELS):
                    at = SSUM_CHANNEL + c * chan
                    t = row[0] * v[c]
                    part[at + SSUM_WY] += t
                    part[at + SSUM_WYY] += t * v[c]
                    part[at + SSUM_BINS:at + chan] += v[c][None, :] * row[1:, None]
            total = part if total is None else total + part
        sm = sm + total
    return sm


def cross_spectrum_groups_reference(xsums, wsum, nrows, order, offset):
    """umpcBatchCrossSpectrumGroups in numpy, IN THE DEVICE'S ORDER OF OPERATIONS: gx [G, 3, 2 + 4 K] float64 from the sums
    [2 + 6 (2 + 2 K), B], the window's column sums wsum [1 + 2 K] (spectrum_wsum), the number of basis rows they were taken
    over and the tables of group_index. A member enters when skipped == 0, n == nrows and n >= 2 -- one rule for all
    channels. Per member and signal channel the mean removal of spectrum_power_reference: m = sum wv / W0, A_j = C_j - m Wc_j,
    B_j = S_j - m Ws_j. Per group and channel c: the members that enter, those that do not, then at 2 + 4 j the sums over the
    members that enter of (4 (Ax Ax + Bx Bx)) / W0^2, (4 (Ay Ay + By By)) / W0^2, (4 (Ax Ay + Bx By)) / W0^2 and
    (4 (Bx Ay - Ax By)) / W0^2: Sxx, Syy, Cxy, Qxy -- (Cxy, Qxy) is conj(X) Y with X = A - iB, so a y that lags x has Qxy < 0.
    Order of summation: spectrum_groups_reference's (lane l of 64 adds members l, l + 64, .. from +0, then the tree)."""
    sm, wsum = np.asarray(xsums, np.float64), np.asarray(wsum, np.float64)
    order, offset = np.asarray(order), np.asarray(offset)
    G, nrows = len(offset) - 1, int(nrows)
    if sm.ndim != 2 or wsum.ndim != 1 or wsum.shape[0] < 3 or wsum.shape[0] % 2 != 1:
        raise ValueError("cross_spectrum_groups_reference: sums must be [2 + 6 (2 + 2 K), B] and wsum [1 + 2 K]")
    K = (wsum.shape[0] - 1) // 2
    if G < 1 or nrows < 0 or sm.shape[0] != cross_spectrum_sum_rows(K):
        raise ValueError("cross_spectrum_groups_reference: bad argument")
    chan = 2 + 2 * K
    w0 = wsum[0]
    w02 = w0 * w0
    n, skipped = sm[SSUM_N], sm[SSUM_SKIPPED]
    enters = (skipped == 0.0) & (n == float(nrows)) & (n >= 2.0)
    out = np.zeros((G, 3, 2 + 4 * K))
    lanes = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(3):
            xs = sm[SSUM_CHANNEL + c * chan:SSUM_CHANNEL + (c + 1) * chan]
            ys = sm[SSUM_CHANNEL + (3 + c) * chan:SSUM_CHANNEL + (4 + c) * chan]
            mx, my = xs[SSUM_WY] / w0, ys[SSUM_WY] / w0
            wc, ws = wsum[1::2][:, None], wsum[2::2][:, None]
            ax, bx = xs[SSUM_BINS::2] - mx * wc, xs[SSUM_BINS + 1::2] - mx * ws                 # [K, B]
            ay, by = ys[SSUM_BINS::2] - my * wc, ys[SSUM_BINS + 1::2] - my * ws
            four = np.stack(((4.0 * (ax * ax + bx * bx)) / w02, (4.0 * (ay * ay + by * by)) / w02,
                             (4.0 * (ax * ay + bx * by)) / w02, (4.0 * (bx * ay - ax * by)) / w02), 1)   # [K, 4, B]
            for g in range(G):
                mem = order[offset[g]:offset[g + 1]]
                ok = enters[mem]
                terms = np.where(ok[None, None, :], four[:, :, mem], 0.0).reshape(4 * K, len(mem))
                part = np.zeros((4 * K, 64))
                for m0 in range(0, len(mem), 64):
                    t = terms[:, m0:m0 + 64]
                    part[:, :t.shape[1]] = part[:, :t.shape[1]] + t
                for w in (32, 16, 8, 4, 2, 1):
                    part = part + part[:, lanes ^ w]
                out[g, c, GX_N], out[g, c, GX_SKIPPED] = ok.sum(), len(mem) - ok.sum()
                out[g, c, GX_FIRST:] = part[:, 0]
    return out


def combine_cross_spectra(parts):
    """The group table of a whole job from the tables gx [G, 3, 2 + 4 K] of its blocks of robots, or of the column blocks a
    cell is split over: every column is a raw sum, so the tables add (counts exactly; the sums to the rounding of one more
    addition per part). numpy arrays or torch tensors; the result is of the first part's kind and the parts are not
    modified. transfer_rows_reference / BatchUprightMPC.transfer_rows turn the combined table into rows."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_cross_spectra: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        total = total + p
    return total


def transfer_rows_reference(gx):
    """umpcBatchTransfer in numpy fp64, in the kernel's operation order: tf [G, 3, K, 12] (rows TF_*) from gx [G, 3, 2 + 4 K].
    With M2 = Cxy Cxy + Qxy Qxy: Pxx = Sxx / n, Pyy = Syy / n, the H1 estimate h = (Cxy / Sxx, Qxy / Sxx), gain = sqrt(M2) /
    Sxx, phase = atan2(Qxy, Cxy) (negative: y lags x), coh = M2 / (Sxx Syy), gain_h2 = Syy / sqrt(M2), rel_err = sqrt((1 -
    coh) / ((2 n) coh)), noise = Pyy (1 - coh). Refused (row 0 = 0, rows 2..11 NaN) when n < 2, a sum is not finite or Sxx is
    not > 0; rows 8..11 are NaN when Syy is not > 0. Nothing else is clamped: rounding may leave coh a hair above 1. Every
    row but the phase is the kernel's bit for bit; the phase to the rounding of atan2."""
    gx = np.asarray(gx, np.float64)
    if gx.ndim != 3 or gx.shape[1] != 3 or gx.shape[2] < 6 or (gx.shape[2] - 2) % 4 != 0 or (gx.shape[2] - 2) // 4 > SPEC_MAX_K:
        raise ValueError("transfer_rows_reference: gx must be [G, 3, 2 + 4 K] with 1 <= K <= %d" % SPEC_MAX_K)
    G, K = gx.shape[0], (gx.shape[2] - 2) // 4
    n = np.repeat(gx[:, :, GX_N, None], K, 2)                                                    # [G, 3, K]
    four = gx[:, :, GX_FIRST:].reshape(G, 3, K, 4)
    sxx, syy, cxy, qxy = (four[..., k] for k in range(4))
    tf = np.full((G, 3, K, TF_ROWS), np.nan)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        refused = ~(n >= 2.0) | ~np.isfinite(four).all(-1) | ~(sxx > 0.0)
        noy = refused | ~(syy > 0.0)
        m2 = cxy * cxy + qxy * qxy
        mag = np.sqrt(m2)
        pyy, coh = syy / n, m2 / (sxx * syy)
        rest = 1.0 - coh
        tf[..., TF_N] = np.where(refused, 0.0, n)
        tf[..., TF_SKIPPED] = gx[:, :, GX_SKIPPED, None]
        for row, val in ((TF_PXX, sxx / n), (TF_PYY, pyy), (TF_H_RE, cxy / sxx), (TF_H_IM, qxy / sxx), (TF_GAIN, mag / sxx),
                         (TF_PHASE, np.arctan2(qxy, cxy))):
            tf[..., row] = np.where(refused, np.nan, val)
        for row, val in ((TF_COH, coh), (TF_GAIN_H2, syy / mag), (TF_REL_ERR, np.sqrt(rest / ((2.0 * n) * coh))), (TF_NOISE, pyy * rest)):
            tf[..., row] = np.where(noy, np.nan, val)
    return tf


# ---- trajectory modes (umpcBatchGram / umpcBatchProject) ------------------------------------------------------------------------
GRAM_ROWS, GRAM_COLS, PROJ_ROWS, PROJ_MAX = 66, 64, 32, 4
# Gram table, per group [66, 64]: rows 0..63 the matrix over member slots (slot i = order[offset[g] + i]); row GR_COUNTS the steps
# at which each slot was scored; row GR_TAIL: the steps accumulated, n, the six scales, zeros
GR_COUNTS, GR_TAIL = 64, 65
GT_STEPS, GT_N, GT_SCALE = 0, 1, 2
GRAM_DEFAULT_SCALE = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)      # the position error alone
# projection rows, per (step, group): members scored / skipped, then row P_FIRST + 6 m + c = sum_b weights[m][b] z_c(b)
P_N, P_SKIPPED, P_FIRST = 0, 1, 2
# status of a cell in trajectory_modes: usable; fewer than two valid members; trace(Gc) <= 0 (all valid draws on one path); n > 64
MODES_OK, MODES_FEW, MODES_FLAT, MODES_BIG = 0, 1, 2, 3
# trajectory table rows, per robot [12, B] (score-shaped: score_quantiles / score_bootstrap / score_sensitivity take it unchanged):
#   0  1 when the robot is a valid member of a usable cell (the "enters" convention of a score), else 0 and rows 1..11 are 0
#   1  Gram_ii, the squared length of the robot's error path        2  Gc_ii, its squared distance from the cell's mean path
#   3  the mean of D2_ij = Gram_ii + Gram_jj - 2 Gram_ij over the other valid members        4  the smallest such D2
#   5  the robot index of that nearest neighbour (ties: the lowest slot)
#   6  1 for the cell's medoid: the minimum of row 3, ties to the lowest slot
#   7  the rank of row 3 inside the cell, 0 = the most typical (ties: the lowest slot first)
#   8  Gc_ii / trace(Gc), the robot's share of the cell's variation
#   9..11  the mode scores sqrt(lam_m) W_im, m = 0..2 (0 beyond M)
(T_VALID, T_GII, T_GCII, T_MEAN_D2, T_MIN_D2, T_NEAREST, T_MEDOID, T_RANK, T_SHARE, T_MODE0, T_MODE1, T_MODE2) = range(12)
TRAJ_ROW_NAMES = ("valid", "gram_ii", "gc_ii", "mean_d2", "min_d2", "nearest", "medoid", "rank", "share", "mode0", "mode1", "mode2")


def _check_scale(what, scale):
    scale = np.asarray(scale, np.float64)
    if scale.shape != (6,) or not np.all(np.isfinite(scale)) or np.any(scale < 0):
        raise ValueError("%s: scale is six finite numbers >= 0" % what)
    return scale


def gram_reference(state_hist, ref, first, count, ref_first, after, order, offset, scale=GRAM_DEFAULT_SCALE, accumulate=False,
                   gram=None, dtype=np.float64):
    """umpcBatchGram in numpy: [G, 66, 64] float64. The tables, first, count, ref_first, after, order, offset and dtype are
    those of dispersion_reference, and so is the data rule: a (member, step) is scored when its 12 words are finite, each
    difference is formed in `dtype` and widened, y_c = scale[c] * z_c is one fp64 product, and what is not scored is y = +0.
    Gram[i][j] is summed over k = (step ascending, component 0..5 ascending) in that order, one rounded product and one rounded
    addition per term, from +0 or -- accumulate=True -- from the matrix of `gram`, whose counts and steps add. THE KERNEL'S ORDER
    INSIDE ONE MFMA IS NOT DOCUMENTED AND NOT FOLLOWED: kernel and mirror agree bit for bit on exactly representable data and
    within (2 N + 2) 2^-53 sum |y_i y_j|, N = 6 x steps accumulated, otherwise (each side is within (N + 1) 2^-53 of the exact
    sum). A cell of n > 64 members is flagged: rows 0..63 NaN, row 64 zero."""
    st = np.asarray(state_hist)
    ref = np.asarray(ref)
    order, offset = np.asarray(order), np.asarray(offset)
    first, count, ref_first, after = int(first), int(count), int(ref_first), int(bool(after))
    G = len(offset) - 1
    if count < 0 or first < 0 or ref_first < 0 or G < 1:
        raise ValueError("gram_reference: bad argument")
    scale = _check_scale("gram_reference", scale)
    if accumulate:
        if gram is None or np.shape(gram) != (G, GRAM_ROWS, GRAM_COLS):
            raise ValueError("gram_reference: accumulate needs gram [G, 66, 64]")
        out = np.array(gram, np.float64)
        if count == 0:
            return out
    else:
        out = np.zeros((G, GRAM_ROWS, GRAM_COLS))
    B = st.shape[-1]
    oks, ys = np.zeros((count, B), bool), np.zeros((count, 6, B))
    for i in range(count):
        ok, z = _error_state(st[first + i + after], ref[ref_first + i] if ref.ndim == 3 else ref, dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            oks[i], ys[i] = ok, scale[:, None] * np.where(ok, z, 0.0)
    for g in range(G):
        mem = order[offset[g]:offset[g + 1]]
        n = len(mem)
        t = out[g]
        t[GR_TAIL, GT_STEPS] += count
        t[GR_TAIL, GT_N] = n
        t[GR_TAIL, GT_SCALE:GT_SCALE + 6] = scale
        t[GR_TAIL, GT_SCALE + 6:] = 0.0
        if n > GRAM_COLS:
            t[:GRAM_COLS], t[GR_COUNTS] = np.nan, 0.0
            continue
        acc = t[:n, :n].copy()
        yg = ys[:, :, mem]
        with np.errstate(over="ignore", invalid="ignore"):
            for i in range(count):
                for c in range(6):
                    acc = acc + np.multiply.outer(yg[i, c], yg[i, c])
        t[:n, :n] = acc
        t[GR_COUNTS, :n] += oks[:, mem].sum(0)
    return out


def combine_grams(parts):
    """The Gram table of a whole window from the tables [G, 66, 64] of the pieces it is cut into (the same cells, the same
    scales): the matrices, the counts and the steps add, as they do on the device with accumulate = 1 -- bit for bit on exactly
    representable data, else to the rounding of one more addition per part. n and the scales of the parts must agree:
    ValueError otherwise. numpy arrays or torch tensors; the result is of the first part's kind and the parts are not modified."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_grams: no parts")
    total = parts[0].clone() if hasattr(parts[0], "clone") else np.array(parts[0], np.float64)
    for p in parts[1:]:
        if tuple(p.shape) != tuple(total.shape) or not bool((p[:, GR_TAIL, GT_N:GT_SCALE + 6] == total[:, GR_TAIL, GT_N:GT_SCALE + 6]).all()):
            raise ValueError("combine_grams: the parts are tables of different cells or scales (n and the six scales must agree)")
        total[:, :GR_TAIL] = total[:, :GR_TAIL] + p[:, :GR_TAIL]
        total[:, GR_TAIL, GT_STEPS] = total[:, GR_TAIL, GT_STEPS] + p[:, GR_TAIL, GT_STEPS]
    return total


def project_reference(state_hist, ref, first, count, ref_first, after, order, offset, weights, dtype=np.float64):
    """umpcBatchProject in numpy, IN THE DEVICE'S ORDER OF SUMMATION: [count, G, 32] float64. weights [M, B], 1 <= M <= 4, by robot.
    The dispersion mirror with S1 weighted and S2 dropped: a member is scored when its 12 words AND its M weights are finite;
    its term for row 2 + 6 m + c is the one fp64 product weights[m] * z_c, and (+0) * (+0) when it is not scored; the fold is
    dispersion_reference's (_lane_fold). The kernel's bits, for every cell size."""
    st = np.asarray(state_hist)
    ref = np.asarray(ref)
    order, offset = np.asarray(order), np.asarray(offset)
    weights = np.asarray(weights, np.float64)
    first, count, ref_first, after = int(first), int(count), int(ref_first), int(bool(after))
    G = len(offset) - 1
    if count < 0 or first < 0 or ref_first < 0 or G < 1:
        raise ValueError("project_reference: bad argument")
    if weights.ndim != 2 or not 1 <= weights.shape[0] <= PROJ_MAX or weights.shape[1] != st.shape[-1]:
        raise ValueError("project_reference: weights is [M, B] with 1 <= M <= 4")
    M = weights.shape[0]
    wfin = np.isfinite(weights).all(0)
    proj = np.zeros((count, G, PROJ_ROWS))
    for i in range(count):
        ok, z = _error_state(st[first + i + after], ref[ref_first + i] if ref.ndim == 3 else ref, dtype)
        ok = ok & wfin
        z = np.where(ok, z, 0.0)
        w = np.where(ok, weights, 0.0)
        with np.errstate(over="ignore", invalid="ignore"):
            terms = (w[:, None, :] * z[None, :, :]).reshape(6 * M, -1)       # [6 M, B], row 6 m + c
        for g in range(G):
            mem = order[offset[g]:offset[g + 1]]
            scored = int(ok[mem].sum())
            proj[i, g, P_N], proj[i, g, P_SKIPPED] = scored, len(mem) - scored
            proj[i, g, P_FIRST:P_FIRST + 6 * M] = _lane_fold(terms[:, mem])
    return proj


def _valid_slots(t):
    """the member slots of one Gram table [66, 64] that were scored at every accumulated step"""
    n = int(t[GR_TAIL, GT_N])
    return np.nonzero((np.arange(GRAM_COLS) < n) & (t[GR_COUNTS] == t[GR_TAIL, GT_STEPS]))[0]


def _centred(gv):
    """H gv H with H = I - 11^T / n, symmetric by construction"""
    gc = gv - gv.mean(0)[None, :]
    gc = gc - gc.mean(1)[:, None]
    return 0.5 * (gc + gc.T)


def trajectory_modes(gram, M=3):
    """The ways the draws of each cell differ AS WHOLE TRAJECTORIES, from the Gram tables [G, 66, 64] of umpcBatchGram /
    gram_reference (numpy; the small dense algebra stays on the host, as propagator_poles does). Per cell, on its VALID slots
    only -- slot i < n with gram[g][64][i] == gram[g][65][0]: a draw that was not finite at any step is left out, not zero-filled
    --: Gc = H Gram H, the doubly centred matrix (H = I - 11^T / nvalid: the cell's mean path is removed), and its
    eigen-decomposition by numpy.linalg.eigh. Returns a dict of
      lam [G, M]      the M largest eigenvalues, descending (0 beyond nvalid)      share [G, M]   lam / trace(Gc)
      W [G, 64, M]    their eigenvectors over the member slots, 0 on slots that are not valid; the component of largest
                      magnitude is positive, ties to the lowest slot (the rule of the ellipsoids' eigenvectors)
      neff [G]        trace(Gc)^2 / sum of all lambda^2: the number of ways the cell really varies (1: one drift direction)
      trace [G], nvalid [G], status [G]: 0 usable, 1 fewer than two valid members, 2 trace(Gc) <= 0, 3 the cell had n > 64.
    lam, share, W, neff and trace of a cell that is not usable are NaN. sqrt(lam_m) W_im is draw i's score on mode m
    (trajectory_table); umpcBatchProject with W[:, :, m] as weights is the mode's time course."""
    gram = np.asarray(gram, np.float64)
    M = int(M)
    if gram.ndim != 3 or gram.shape[1:] != (GRAM_ROWS, GRAM_COLS) or not 1 <= M <= GRAM_COLS:
        raise ValueError("trajectory_modes: gram is [G, 66, 64] and 1 <= M <= 64")
    G = gram.shape[0]
    res = dict(lam=np.full((G, M), np.nan), share=np.full((G, M), np.nan), W=np.full((G, GRAM_COLS, M), np.nan),
               neff=np.full(G, np.nan), trace=np.full(G, np.nan), nvalid=np.zeros(G, np.int64), status=np.zeros(G, np.int64))
    for g in range(G):
        t = gram[g]
        if t[GR_TAIL, GT_N] > GRAM_COLS:
            res["status"][g] = MODES_BIG
            continue
        v = _valid_slots(t)
        res["nvalid"][g] = len(v)
        if len(v) < 2:
            res["status"][g] = MODES_FEW
            continue
        gc = _centred(t[np.ix_(v, v)])
        tr = float(np.trace(gc))
        if not tr > 0:
            res["status"][g] = MODES_FLAT
            continue
        lam, vec = np.linalg.eigh(gc)
        lam, vec = lam[::-1], vec[:, ::-1]
        m = min(M, len(v))
        W = np.zeros((GRAM_COLS, M))
        for k in range(m):
            w = vec[:, k]
            big = w[int(np.argmax(np.abs(w)))]          # (argmax takes the lowest slot on a tie)
            W[v, k] = -w if big < 0 else w
        res["lam"][g], res["share"][g] = 0.0, 0.0
        res["lam"][g, :m] = lam[:m]
        res["share"][g, :m] = lam[:m] / tr
        res["W"][g] = W
        res["neff"][g] = tr * tr / float(np.sum(lam * lam))
        res["trace"][g] = tr
    return res


def trajectory_table(gram, modes, order, offset, B):
    """The score-shaped table [12, B] float64 of the Gram tables [G, 66, 64] and their trajectory_modes (rows: T_* above): per
    robot that is a valid member of a usable cell, how long its error path is, how far it is from the cell's mean path and
    from the other draws (D2_ij = Gram_ii + Gram_jj - 2 Gram_ij), its nearest neighbour, whether it is the cell's medoid --
    the flight to plot as "the typical one" --, its rank from the most typical to the oddest, and its scores on the first
    three modes. Every other robot has zeros. order, offset: the index the Gram tables were computed with."""
    gram = np.asarray(gram, np.float64)
    order, offset = np.asarray(order), np.asarray(offset)
    G = len(offset) - 1
    if gram.shape != (G, GRAM_ROWS, GRAM_COLS) or len(modes["status"]) != G:
        raise ValueError("trajectory_table: gram, modes and the index are of different numbers of cells")
    tab = np.zeros((12, int(B)))
    for g in range(G):
        if modes["status"][g] != MODES_OK:
            continue
        t = gram[g]
        v = _valid_slots(t)
        rob = order[offset[g] + v]
        gv = t[np.ix_(v, v)]
        d = np.diag(gv)
        d2 = (d[:, None] + d[None, :]) - 2.0 * gv
        gc = np.diag(_centred(gv))
        nv = len(v)
        mean_d2 = (d2.sum(1) - np.diag(d2)) / (nv - 1)
        off = d2 + np.where(np.eye(nv, dtype=bool), np.inf, 0.0)
        near = np.argmin(off, 1)                      # (argmin takes the lowest slot on a tie)
        by = np.argsort(mean_d2, kind="stable")
        rank = np.empty(nv)
        rank[by] = np.arange(nv)
        tab[T_VALID, rob] = 1.0
        tab[T_GII, rob], tab[T_GCII, rob] = d, gc
        tab[T_MEAN_D2, rob], tab[T_MIN_D2, rob] = mean_d2, off[np.arange(nv), near]
        tab[T_NEAREST, rob] = rob[near]
        tab[T_MEDOID, rob[by[0]]] = 1.0
        tab[T_RANK, rob] = rank
        tab[T_SHARE, rob] = gc / modes["trace"][g]
        lam, W = modes["lam"][g], modes["W"][g]
        for k in range(min(3, W.shape[1])):
            tab[T_MODE0 + k, rob] = np.sqrt(max(lam[k], 0.0)) * W[v, k]
    return tab


def mode_weights(modes, order, offset, B, M=None):
    """weights [M, B] float64 for umpcBatchProject / project_reference from the eigenvectors W [G, 64, M'] of trajectory_modes:
    weights[m][order[offset[g] + i]] = W[g][i][m] for the member slots of every usable cell, 0 for every other robot. M None =
    all the modes there are, 4 at the most."""
    order, offset = np.asarray(order), np.asarray(offset)
    W = modes["W"]
    M = min(W.shape[2], PROJ_MAX) if M is None else int(M)
    if not 1 <= M <= min(W.shape[2], PROJ_MAX):
        raise ValueError("mode_weights: 1 <= M <= min(the modes computed, 4)")
    out = np.zeros((M, int(B)))
    for g in range(len(offset) - 1):
        n = int(offset[g + 1] - offset[g])
        if modes["status"][g] == MODES_OK and n <= GRAM_COLS:
            out[:, order[offset[g]:offset[g + 1]]] = W[g, :n, :M].T
    return out
