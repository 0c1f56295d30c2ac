#!/usr/bin/env python3
"""Times umpcBatchEnsembleBootstrap against what the library could do for the same result before it: a loop over the steps of
umpcBatchScore(first = i, count = 1) into a fresh score and umpcBatchScoreBootstrap with the replicates of every step kept as
[K, G, R], then the studentised maximum over the steps and its quantiles in torch. Same tables, one process.

    python tools/time_bands.py [--B 65536] [--K 200] [--R 1000] [--reps 7] [--out profiles/band_timing.txt]

Shape of record, that of the neighbouring profiles: B = 65 536 as 1 024 contiguous cells of 64, K = 200 recorded steps, fp32
tables (state record and a constant reference), term e_p, R = 1000 replicates, probabilities (0.025, 0.975), level 0.95; the
mean and the median statistic, with and without a second history. Device events around each route after warm calls of both;
the routes alternate inside the loop, so that both see the same clock state. The group index and every result and work
tensor of both routes are made once, before the loop; "extra memory" is what a route holds beyond the tables and the band,
crit and sup it returns. The two routes are compared first: the band columns bit for bit, sup and crit bit for bit.
The bar is the loop: the new call has to be faster."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402

PROBS, LEVELS = (0.025, 0.975), (0.95,)
STATS = (("mean", 0.5), ("quantile", 0.5))


def rank(p, n):
    return min(n - 1, max(0, int(-(-(p * n) // 1)) - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--R", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bands.py needs the MI355X: a timing taken anywhere else says nothing")
    B, K, R, nq, nl = a.B, a.K, a.R, len(PROBS), len(LEVELS)
    if B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    G = B // 64
    probs, levels = (C.c_double * nq)(*PROBS), (C.c_double * nl)(*LEVELS)
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    gen = torch.Generator(device=dev).manual_seed(1)

    def history(drift):
        """a random walk of the position about the origin: a curve per draw, as a sweep records one"""
        st = torch.zeros((K + 1, 18, B), device=dev)
        st[:, 0:3] = torch.cumsum(drift * torch.randn((K + 1, 3, B), device=dev, generator=gen), 0) + torch.randn((K + 1, 3, B), device=dev,
                                                                                                                generator=gen)
        st[:, 11] = 1.0
        return st
    state, ostate = history(0.3), history(0.4)
    ref = torch.zeros((9, B), device=dev)
    ref[8] = 1.0
    index = m.group_index(torch.arange(B, device=dev, dtype=torch.int32) // 64, G)
    held0 = torch.cuda.memory_allocated(dev)
    # the new call: band, crit, sup and work
    band = torch.empty((K, G, 6 + nq), dtype=torch.float64, device=dev)
    crit = torch.empty((G, 1 + nl), dtype=torch.float64, device=dev)
    sup = torch.empty((G, R), dtype=torch.float64, device=dev)
    work = torch.empty((B + G,), dtype=torch.float64, device=dev)
    held_new = torch.cuda.memory_allocated(dev) - held0 - (band.numel() + crit.numel() + sup.numel()) * 8
    # the loop: two scores, the rows and the replicates of every step
    score, oscore = (torch.empty((12, B), device=dev) for _ in range(2))
    boots = torch.empty((K, G, 5 + nq), dtype=torch.float64, device=dev)
    reps = torch.empty((K, G, R), dtype=torch.float64, device=dev)

    def new(stat, p, pair):
        m._check(m.L.umpcBatchEnsembleBootstrap(m.h, _ptr(state), None, _ptr(ostate) if pair else None, None, None, _ptr(ref), 0, K, 0, 1,
                                                _ptr(index[0]), _ptr(index[1]), G, 0, ("mean", "quantile").index(stat), p, R, 7, probs,
                                                nq, levels, nl, _ptr(band), _ptr(crit), _ptr(sup), _ptr(work), m._stream()))
        return band, crit, sup

    def loop(stat, p, pair):
        s = m._stream()
        for i in range(K):
            for tab, sc in ((state, score), (ostate, oscore))[:2 if pair else 1]:
                m._check(m.L.umpcBatchScoreInit(m.h, _ptr(sc), s))
                m._check(m.L.umpcBatchScore(m.h, _ptr(tab), None, None, None, _ptr(ref), i, 1, 0, 0, 1.0, 1, _ptr(sc), s))
            m._check(m.L.umpcBatchScoreBootstrap(m.h, _ptr(score), _ptr(oscore) if pair else None, 1, 0, _ptr(index[0]), _ptr(index[1]), G,
                                                 ("mean", "quantile").index(stat), p, R, 7, probs, nq, _ptr(boots[i]), _ptr(reps[i]),
                                                 _ptr(work), s))
        enters = (boots[..., 0] >= 2) & (reps.amax(2) != reps.amin(2))                 # [K, G]
        d = (reps - boots[..., 2:3]).abs() / boots[..., 4:5]
        d = torch.where(enters[..., None] & (d == d), d, torch.zeros((), dtype=torch.float64, device=dev))
        lsup = d.amax(0)                                                               # [G, R]
        lcrit = torch.cat([enters.sum(0, dtype=torch.float64)[:, None], lsup.sort(1).values[:, [rank(q, R) for q in LEVELS]]], 1)
        return torch.cat([boots[..., :5], enters.double()[..., None], boots[..., 5:]], 2), lcrit, lsup

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    med = lambda v: v[len(v) // 2]
    lines = ["umpcBatchEnsembleBootstrap vs the per-step loop umpcBatchScore(count = 1) + umpcBatchScoreBootstrap with the replicates kept "
             "[K, G, R] and sup / crit in torch (tools/time_bands.py)",
             "B = %d as %d contiguous cells of 64, K = %d steps, fp32 state record, constant reference, term e_p, after = 1, R = %d, "
             "probabilities %s, level %s; %d repetitions, routes alternating, device events"
             % (B, G, K, R, PROBS, LEVELS, a.reps)]
    slower = []
    for stat, p in STATS:
        for pair in (False, True):
            name = "%s%s" % ("mean" if stat == "mean" else "median", ", MPC minus a second history" if pair else "")
            for _ in range(2):
                route(lambda: new(stat, p, pair))
            got = [t.clone() for t in new(stat, p, pair)]
            route(lambda: loop(stat, p, pair))
            torch.cuda.reset_peak_memory_stats(dev)
            held = torch.cuda.memory_allocated(dev)
            _, want = route(lambda: loop(stat, p, pair))
            peak = torch.cuda.max_memory_allocated(dev) - held + (score.numel() * (2 if pair else 1)) * 4 + (boots.numel() + reps.numel()) * 8
            for g_, w_, what in zip(got, want, ("band", "crit", "sup")):
                assert torch.equal(g_.view(torch.int64), w_.contiguous().view(torch.int64)), "%s differs from the loop's (%s)" % (what, name)
            del want
            tn, tl = [], []
            for _ in range(a.reps):
                tn.append(route(lambda: new(stat, p, pair))[0])
                tl.append(route(lambda: loop(stat, p, pair))[0])
            tn, tl = sorted(tn), sorted(tl)
            lines += ["%s" % name,
                      "  one call   min %.3f ms   median %.3f ms   max %.3f ms; memory beyond the tables and band, crit, sup: %.1f MB (work)"
                      % (tn[0], med(tn), tn[-1], held_new / 1e6),
                      "  the loop   min %.3f ms   median %.3f ms   max %.3f ms; %d launches of the library and torch's kernels; memory beyond the "
                      "tables and its results: %.1f MB" % (tl[0], med(tl), tl[-1], K * (5 + (4 if pair else 2)), peak / 1e6),
                      "  ratio loop / one call %.2f (median); %.2f replicate-values per ns" % (med(tl) / med(tn), K * G * R * 64 / med(tn) / 1e6)]
            if not med(tn) < med(tl):
                slower.append(name)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if slower:
        raise SystemExit("the one call's median is not below the loop's: %s" % ", ".join(slower))


if __name__ == "__main__":
    main()
