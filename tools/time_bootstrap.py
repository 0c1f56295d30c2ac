#!/usr/bin/env python3
"""Times umpcBatchScoreBootstrap against the torch route a user would otherwise write (the resample indices from the counter
hash, a gather [cells, R, 64], a mean or a sort along the cell, a sort over the replicates), on the same score, in one process.

    python tools/time_bootstrap.py [--B 65536] [--R 1000] [--reps 20] [--out profiles/bootstrap_timing.txt]

Shape of record, that of the neighbouring profiles: B = 65 536 as 1 024 contiguous cells of 64, fp32 scores, the per-robot
mean tracking error (row 1 / row 0), R = 1000 replicates, probabilities (0.025, 0.975), the mean and the median statistic.
Device events around each call after warm calls of each route; the routes alternate inside the loop, so that both see the
same clock state. The group index and the kernel's work and result tensors are made once, before the loop. Written out per
statistic: min, median and max of both routes over the repetitions, their ratio, and the peak memory the torch route
allocates beyond the score. The bar is the torch route. One more line is written down and not judged: 100 cells of 640, the
block path, kernels only."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr, _u01_device  # noqa: E402

PROBS = (0.025, 0.975)
STATS = (("mean", 0.5), ("quantile", 0.5))


def rank(p, n):
    return min(n - 1, max(0, int(-(-(p * n) // 1)) - 1))


def torch_bootstrap(score, cells, R, seed, stat, p, probs):
    """[cells, 5 + nq] and [cells, R] as array expressions (every robot scored: nothing is compacted)"""
    size = score.shape[1] // cells
    x = (score[1].double() / score[0].double()).reshape(cells, size)
    idx = (torch.arange(R, dtype=torch.int64, device=score.device)[:, None] << 32) + torch.arange(size, dtype=torch.int64,
                                                                                                   device=score.device)[None]
    j = (_u01_device(seed, idx, 41) * size).floor().long().clamp_max(size - 1)
    sample = x[:, j]                                                                  # the gather: [cells, R, size]
    if stat == "mean":
        t, point = sample.sum(2) / size, x.sum(1) / size
    else:
        t, point = sample.sort(2).values[..., rank(p, size)], x.sort(1).values[:, rank(p, size)]
    ts = t.sort(1).values
    n = torch.full_like(point, float(size))
    return torch.cat([n[:, None], torch.zeros_like(n)[:, None], point[:, None], t.mean(1, keepdim=True), t.std(1, keepdim=True),
                      ts[:, [rank(q, R) for q in probs]]], 1), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--R", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bootstrap.py needs the MI355X: a timing taken anywhere else says nothing")
    B, R, nq = a.B, a.R, len(PROBS)
    if B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    probs = (C.c_double * nq)(*PROBS)

    def setup(B, size):
        G = B // size
        m = BatchUprightMPC(B, torch.float32)
        g = torch.Generator(device=m.device).manual_seed(1)
        score = torch.zeros((12, B), device=m.device)
        score[0] = 200.0
        score[1] = 200.0 * torch.randn(B, device=m.device, generator=g).square()
        index = m.group_index(torch.arange(B, device=m.device, dtype=torch.int32) // size, G)
        boot = torch.empty((G, 5 + nq), dtype=torch.float64, device=m.device)
        reps = torch.empty((G, R), dtype=torch.float64, device=m.device)
        work = torch.empty((B + G,), dtype=torch.float64, device=m.device)

        def kernel(stat, p):
            m._check(m.L.umpcBatchScoreBootstrap(m.h, _ptr(score), None, 1, 0, _ptr(index[0]), _ptr(index[1]), G,
                                                 ("mean", "quantile").index(stat), p, R, 7, probs, nq, _ptr(boot), _ptr(reps),
                                                 _ptr(work), m._stream()))
            return boot, reps
        return m, G, score, kernel

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    med = lambda v: v[len(v) // 2]
    m, G, score, kernel = setup(B, 64)
    dev = m.device
    lines = ["umpcBatchScoreBootstrap vs the torch route (hash indices, gather [cells, R, 64], mean or sort, sort over the replicates) "
             "(tools/time_bootstrap.py)",
             "B = %d as %d contiguous cells of 64, fp32 score, value row 1 / row 0, R = %d, probabilities %s; %d repetitions, "
             "routes alternating, device events" % (B, G, R, PROBS, a.reps)]
    slower = []
    for stat, p in STATS:
        for _ in range(3):                                                           # warm calls, and the two results agree
            _, (bk, rk) = route(lambda: kernel(stat, p))
        bk, rk = bk.clone(), rk.clone()
        route(lambda: torch_bootstrap(score, G, R, 7, stat, p, PROBS))
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        _, (bt, rt) = route(lambda: torch_bootstrap(score, G, R, 7, stat, p, PROBS))
        peak = torch.cuda.max_memory_allocated(dev) - held
        if stat == "quantile":
            assert torch.equal(rk, rt) and torch.equal(bk[:, :3], bt[:, :3]) and torch.equal(bk[:, 5:], bt[:, 5:]), "elements differ"
        assert float(((rk - rt).abs() / rt.abs().clamp_min(1e-300)).max()) < 1e-12, "replicates differ"
        assert float(((bk - bt).abs() / bt.abs().clamp_min(1e-300))[:, 2:].max()) < 1e-9, "rows differ"
        del bt, rt
        tk, tt = [], []
        for _ in range(a.reps):
            tk.append(route(lambda: kernel(stat, p))[0])
            tt.append(route(lambda: torch_bootstrap(score, G, R, 7, stat, p, PROBS))[0])
        tk, tt = sorted(tk), sorted(tt)
        name = "mean" if stat == "mean" else "median"
        lines += ["%-6s kernels       min %.3f ms   median %.3f ms   max %.3f ms" % (name, tk[0], med(tk), tk[-1]),
                  "%-6s torch route   min %.3f ms   median %.3f ms   max %.3f ms" % (name, tt[0], med(tt), tt[-1]),
                  "%-6s ratio torch / kernels %.2f (median); %.1f replicate-values per ns; torch route, peak memory allocated beyond "
                  "the score (its results of %.1f MB included): %.1f MB"
                  % (name, med(tt) / med(tk), G * R * 64 / med(tk) / 1e6, (G * R + G * (5 + nq)) * 8 / 1e6, peak / 1e6)]
        if not med(tk) < med(tt):
            slower.append(name)
    del m, score, kernel
    m, G, score, kernel = setup(64000, 640)
    row = []
    for stat, p in STATS:
        for _ in range(2):
            route(lambda: kernel(stat, p))
        t = sorted(route(lambda: kernel(stat, p))[0] for _ in range(5))
        row.append("%s median %.3f ms" % ("mean" if stat == "mean" else "median", med(t)))
    lines.append("block path, 64000 robots as 100 cells of 640, R = %d, 5 repetitions, kernels only: %s" % (R, ", ".join(row)))
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if slower:
        raise SystemExit("the kernels' median is not below the torch route's: %s" % ", ".join(slower))


if __name__ == "__main__":
    main()
