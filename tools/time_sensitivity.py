#!/usr/bin/env python3
"""Times umpcBatchSensitivity against the torch composition of the same numbers and against umpcBatchDispersion over the same
window, on the same tables, in one process; then umpcBatchSensitivityIndices and umpcBatchFactorBins once each.

    python tools/time_sensitivity.py [--B 65536] [--steps 200] [--F 4] [--M 8] [--reps 20] [--commit ID] [--out profiles/sensitivity_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, state record and a reference table, term e_p,
F = 4 factors in M = 8 bins. Device events around each call after warm calls of each route; the three routes alternate inside the
loop, so that all see the same clock state. The group index and the bins are built once, before the loop: they belong to the
sweep, not to a call. Written out: the three times (min, median and max over the repetitions), the ratios torch / kernel and
kernel / dispersion, the achieved GB/s of the kernel over the ALGORITHMIC bytes (48 B read per robot-step -- p, s, pdes, sdes --,
8 (4 + 2 F M) B written per step and group), the peak memory the torch route allocates on top of the tables
(torch.cuda.max_memory_allocated), and the single times of the index and the bin kernels. No time is fixed in advance: ratios
and GB/s are recorded, not asserted."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_sensitivity(state, ref, n, bins, M, cells):
    """n, skipped, S1, S2, N_fm and S_fm as array expressions: e_p [steps, B] in the dtype, widened; the bins as a one-hot
    [cells, 64, F M] in fp64 and one batched product per table of sums (finite inputs and valid bins: nothing is skipped)"""
    B, F = ref.shape[2], bins.shape[0]
    d = state[:n, 0:3] - ref[:n, 0:3]
    ep = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]                                  # [steps, B]
    fin = torch.isfinite(state[:n, 0:3]).all(1) & torch.isfinite(state[:n, 9:12]).all(1) & torch.isfinite(ref[:n, 0:3]).all(1) \
        & torch.isfinite(ref[:n, 6:9]).all(1)
    ok = (fin & ((bins >= 0) & (bins < M)).all(0)).reshape(n, cells, B // cells)
    okd = ok.to(torch.float64)
    y = ep.to(torch.float64).reshape(n, cells, B // cells) * okd
    hot = torch.nn.functional.one_hot(bins.clamp(0, M - 1).to(torch.int64), M).to(torch.float64)    # [F, B, M]
    hot = hot.permute(1, 0, 2).reshape(cells, B // cells, F * M)
    sfm = torch.einsum("ncj,cjk->nck", y, hot)
    nfm = torch.einsum("ncj,cjk->nck", okd, hot)
    count = okd.sum(2)
    return torch.cat([count[..., None], (~ok).to(torch.float64).sum(2)[..., None], y.sum(2)[..., None], (y * y).sum(2)[..., None],
                      nfm, sfm], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--F", type=int, default=4)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensitivity_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sensitivity.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n, F, M = a.B, a.steps, a.F, a.M
    if B % 64 or not 1 <= F <= 6 or not 2 <= M <= 8:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots), 1 <= F <= 6, 2 <= M <= 8")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    G, cols, icols = B // 64, 4 + 2 * F * M, 8 + F * (4 + M)
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    factors = torch.randn((F, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3] + 0.5 * factors[0].abs()           # (an effect of the first factor)
    state[:n, 12:15] += ref[:, 3:6]
    group = torch.arange(B, device=dev, dtype=torch.int32) // 64
    index = m.group_index(group, G)
    order, offset = index
    bins = m.factor_bins(factors, index, M)
    sens = torch.empty((n, G, cols), dtype=torch.float64, device=dev)
    mom = torch.empty((n, G, 32), dtype=torch.float64, device=dev)
    idx = torch.empty((n, G, icols), dtype=torch.float64, device=dev)

    def kernel():
        m._check(m.L.umpcBatchSensitivity(m.h, _ptr(state), None, _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, 0,
                                          _ptr(bins), F, M, _ptr(sens), m._stream()))
        return sens

    def torch_route():
        return torch_sensitivity(state, ref, n, bins, M, G)

    def dispersion():
        m._check(m.L.umpcBatchDispersion(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, _ptr(mom),
                                         m._stream()))
        return mom

    def indices():
        m._check(m.L.umpcBatchSensitivityIndices(m.h, _ptr(sens), n, G, F, M, _ptr(idx), m._stream()))
        return idx

    def binning():
        return m.factor_bins(factors, index, M)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the results agree
        _, sk = route(kernel)
        route(dispersion)
        route(indices)
        route(binning)
    sk = sk.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, st = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    nc = 4 + F * M
    assert torch.equal(sk[..., 0:2], st[..., 0:2]) and torch.equal(sk[..., 4:nc], st[..., 4:nc]), "counts differ"
    scale = float(sk[..., 3].abs().max())
    assert float((sk[..., 2:4] - st[..., 2:4]).abs().max()) < 1e-12 * scale and float((sk[..., nc:] - st[..., nc:]).abs().max()) < 1e-12 * scale, \
        "sums differ"
    del st
    tk, tt, td = [], [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
        td.append(route(dispersion)[0])
    tk, tt, td = sorted(tk), sorted(tt), sorted(td)
    ti, tb = route(indices)[0], route(binning)[0]
    usable = int((idx[..., 2] == 0).sum())
    eta0 = float(idx[..., 8][idx[..., 2] == 0].mean())
    med = lambda v: v[len(v) // 2]
    nbytes = 48.0 * B * n + 8.0 * cols * n * G
    lines = ["umpcBatchSensitivity vs the torch composition of the same %d numbers and vs umpcBatchDispersion "
             "(tools/time_sensitivity.py), commit %s" % (cols, commit),
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, reference table, term e_p, F = %d, M = %d; %d repetitions, routes "
             "alternating, device events" % (B, G, n, F, M, a.reps),
             "kernel (binned sums)   min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "dispersion kernel      min %.3f ms   median %.3f ms   max %.3f ms   (same window, same run: 12 words and 27 sums)"
             % (td[0], med(td), td[-1]),
             "ratio torch / kernel   %.2f (median)" % (med(tt) / med(tk)),
             "ratio kernel / dispersion kernel   %.2f (median)" % (med(tk) / med(td)),
             "kernel, algorithmic bytes (48 B per robot-step read, %d B per step and group written): %.1f MB -> %.0f GB/s (median)"
             % (8 * cols, nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB)"
             % (n * G * cols * 8 / 1e6, peak / 1e6, tables / 1e6),
             "indices, once          %.3f ms (%d rows, %d usable, mean eta2 of factor 0: %.3f)" % (ti, n * G, usable, eta0),
             "factor bins, once      %.3f ms (%d factors x %d cells)" % (tb, F, G)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
