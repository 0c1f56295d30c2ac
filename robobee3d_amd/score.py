"""Scores of recorded rollouts: the row names of umpcBatchScore / umpcBatchScoreGroups (include/umpc_mi355x.h) and their
numpy fp64 mirrors. The device path is BatchUprightMPC.score / score_groups (batch.py); nothing here touches a device, and
the mirrors are the definition the kernels are tested against, not a fallback.

A score [12, B] condenses what every closed-loop step of a run did against its reference; a group table [G, 8] condenses the
scores of the robots of each group -- the draws of one grid cell of a gain sweep, the end of the reference's gainTuningSims
(costs[i,j], efforts[i,j] = logMetric(log), template/uprightmpc2.py:272-303)."""
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


def score_identity(B, dtype=np.float64):
    """The score no step has entered (umpcBatchScoreInit): rows 9 and 10 = -1, all others 0."""
    s = np.zeros((SCORE_ROWS, int(B)), dtype)
    s[FIRST_OVER] = s[LAST_OVER] = -1
    return s


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
        y = st[c + after]
        r = ref[ref_first + i] if ref.ndim == 3 else ref
        p, s, pdes, sdes = y[0:3], y[9:12], r[0:3], r[6:9]
        ok = np.isfinite(p).all(0) & np.isfinite(s).all(0) & np.isfinite(pdes).all(0) & np.isfinite(sdes).all(0)
        if out is not None:
            ok &= np.isfinite(out[c, 1:3]).all(0)
        with np.errstate(invalid="ignore", over="ignore"):
            ep = ((p - pdes) ** 2).sum(0)
            es = ((s - sdes) ** 2).sum(0)
            p2 = (p ** 2).sum(0)
            if out is not None:
                tau2 = (np.clip(out[c, 1:3], -tl, tl) ** 2).sum(0)
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
