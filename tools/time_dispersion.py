#!/usr/bin/env python3
"""Times umpcBatchDispersion against the torch composition of the same 29 numbers, on the same tables, in one process; then
umpcBatchDispersionEllipsoids and umpcBatchMahalanobis once each.

    python tools/time_dispersion.py [--B 65536] [--steps 200] [--reps 20] [--commit ID] [--out profiles/dispersion_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, state record and a reference table. Device events
around each call after warm calls of each route; the two routes alternate inside the loop, so that both see the same clock
state. The group index is built once, before the loop: it belongs to the sweep, not to a call. Written out: the two times (min,
median and max over the repetitions), the ratio torch / kernel, the achieved GB/s of the kernel over the ALGORITHMIC bytes (48 B
read per robot-step, 256 B written per step and group), the peak memory the torch route allocates on top of the tables
(torch.cuda.max_memory_allocated), and the single times of the ellipsoid and the Mahalanobis kernels. The only bar is the torch
route: that is what a user would otherwise write. Ratios and GB/s are recorded, not asserted."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_dispersion(state, ref, after, cells):
    """n, skipped, S1 [6] and S2 [21] as array expressions: z [steps, B, 6] in the dtype, then fp64 and an einsum over the members
    of a cell into the full [6, 6] matrix, of which the upper triangle is kept (finite inputs: nothing is skipped)"""
    n, B = ref.shape[0], ref.shape[2]
    st = state[int(after):int(after) + n]
    z = torch.cat([st[:, 0:3] - ref[:, 0:3], st[:, 12:15] - ref[:, 3:6]], 1)             # [steps, 6, B]
    ok = torch.isfinite(z).all(1).reshape(n, cells, B // cells)
    zd = z.to(torch.float64).reshape(n, 6, cells, B // cells)
    s1 = zd.sum(3).permute(0, 2, 1)                                                      # [steps, cells, 6]
    s2 = torch.einsum("sicm,sjcm->scij", zd, zd)
    iu = torch.triu_indices(6, 6, device=z.device)
    count = ok.to(torch.float64).sum(2)
    return torch.cat([count[..., None], (~ok).to(torch.float64).sum(2)[..., None], s1, s2[..., iu[0], iu[1]]], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dispersion_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dispersion.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n = a.B, a.steps
    if B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    G = B // 64
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    state[:n, 12:15] += ref[:, 3:6]
    group = torch.arange(B, device=dev, dtype=torch.int32) // 64
    order, offset = m.group_index(group, G)
    mom = torch.empty((n, G, 32), dtype=torch.float64, device=dev)
    ell = torch.empty((n, G, 48), dtype=torch.float64, device=dev)
    msc = torch.empty((12, B), device=dev)

    def kernel():
        m._check(m.L.umpcBatchDispersion(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, _ptr(mom),
                                         m._stream()))
        return mom

    def torch_route():
        return torch_dispersion(state, ref, 0, G)

    def ellipsoids():
        m._check(m.L.umpcBatchDispersionEllipsoids(m.h, _ptr(mom), n, G, _ptr(ell), m._stream()))
        return ell

    def mahalanobis():
        m._check(m.L.umpcBatchMahalanobisInit(m.h, _ptr(msc), m._stream()))
        m._check(m.L.umpcBatchMahalanobis(m.h, _ptr(state), _ptr(ref), None, _ptr(ell), _ptr(group), G, 0, n, 0, 0, 0, 7.8, _ptr(msc),
                                          m._stream()))
        return msc

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        _, mk = route(kernel)
        route(ellipsoids)
        route(mahalanobis)
    mk = mk.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, mt = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    assert torch.equal(mk[..., 0:2], mt[..., 0:2]), "counts differ"
    assert float((mk[..., 2:29] - mt[..., 2:]).abs().max()) < 1e-9, "moments differ"
    del mt
    tk, tt = [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
    tk, tt = sorted(tk), sorted(tt)
    te, tm = route(ellipsoids)[0], route(mahalanobis)[0]
    usable = int((ell[..., 41] == 0).sum())
    med = lambda v: v[len(v) // 2]
    nbytes = 48.0 * B * n + 256.0 * n * G
    lines = ["umpcBatchDispersion vs the torch composition of the same 29 numbers (tools/time_dispersion.py), commit %s" % commit,
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, reference table; %d repetitions, routes alternating, device "
             "events" % (B, G, n, a.reps),
             "kernel (moments)       min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "ratio torch / kernel   %.2f (median)" % (med(tt) / med(tk)),
             "kernel, algorithmic bytes (48 B per robot-step read, 256 B per step and group written): %.1f MB -> %.0f GB/s (median)"
             % (nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB)"
             % (n * G * 29 * 8 / 1e6, peak / 1e6, tables / 1e6),
             "ellipsoids, once       %.3f ms (%d rows, %d usable)" % (te, n * G, usable),
             "Mahalanobis, once      %.3f ms (init + score; 24 B per robot-step and 80 B of its cell's row from cache)" % tm]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(tk) < med(tt):
        raise SystemExit("the kernel's median is not below the torch route's")


if __name__ == "__main__":
    main()
