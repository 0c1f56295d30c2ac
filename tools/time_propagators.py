#!/usr/bin/env python3
"""Times umpcBatchLagMoments against the torch composition of the same 92 numbers and against umpcBatchDispersion over the same
window, on the same tables, in one process; then umpcBatchPropagators once.

    python tools/time_propagators.py [--B 65536] [--steps 200] [--lag 1] [--reps 20] [--commit ID] [--out profiles/propagator_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, state record and a reference table, lag 1. Device
events around each call after warm calls of each route; the three routes alternate inside the loop, so that all see the same
clock state. The group index is built once, before the loop: it belongs to the sweep, not to a call. Written out: the three times
(min, median and max over the repetitions), the ratios torch / kernel and kernel / dispersion, the achieved GB/s of the kernel
over the ALGORITHMIC bytes (96 B read per robot-step, 768 B written per step and group), the peak memory the torch route allocates
on top of the tables (torch.cuda.max_memory_allocated), and the single time of the propagator kernel. No time is fixed in
advance: ratios and GB/s are recorded, not asserted."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_lag_moments(state, ref, n, lag, cells):
    """n, skipped, S1a, S1b [6], S2a, S2b [21] and Sba [36] as array expressions: z [steps + lag, 6, B] in the dtype, then fp64
    and einsums over the members of a cell into full [6, 6] matrices, of which S2 keeps the upper triangle (finite inputs:
    nothing is skipped)"""
    B = ref.shape[2]
    z = torch.cat([state[:n + lag, 0:3] - ref[:, 0:3], state[:n + lag, 12:15] - ref[:, 3:6]], 1)      # [steps + lag, 6, B]
    fin = torch.isfinite(z).all(1)
    ok = (fin[:n] & fin[lag:]).reshape(n, cells, B // cells)
    zd = z.to(torch.float64).reshape(n + lag, 6, cells, B // cells)
    za, zb = zd[:n], zd[lag:]
    s1a, s1b = za.sum(3).permute(0, 2, 1), zb.sum(3).permute(0, 2, 1)                                  # [steps, cells, 6]
    s2a = torch.einsum("sicm,sjcm->scij", za, za)
    s2b = torch.einsum("sicm,sjcm->scij", zb, zb)
    sba = torch.einsum("sicm,sjcm->scij", zb, za)
    iu = torch.triu_indices(6, 6, device=z.device)
    count = ok.to(torch.float64).sum(2)
    return torch.cat([count[..., None], (~ok).to(torch.float64).sum(2)[..., None], s1a, s1b, s2a[..., iu[0], iu[1]],
                      s2b[..., iu[0], iu[1]], sba.reshape(n, cells, 36)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "propagator_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_propagators.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n, lag = a.B, a.steps, a.lag
    if B % 64 or lag < 1:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots) and lag >= 1")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    G = B // 64
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n + lag, 9, B), device=dev, generator=g)
    state = torch.randn((n + lag + 1, 18, B), device=dev, generator=g)
    state[:n + lag, 0:3] += ref[:, 0:3]
    state[:n + lag, 12:15] += ref[:, 3:6]
    state[1:n + lag, 0:3] += 0.5 * (state[:n + lag - 1, 0:3] - ref[:n + lag - 1, 0:3])     # (some correlation between the steps)
    group = torch.arange(B, device=dev, dtype=torch.int32) // 64
    order, offset = m.group_index(group, G)
    xmom = torch.empty((n, G, 96), dtype=torch.float64, device=dev)
    mom = torch.empty((n, G, 32), dtype=torch.float64, device=dev)
    prop = torch.empty((n, G, 80), dtype=torch.float64, device=dev)

    def kernel():
        m._check(m.L.umpcBatchLagMoments(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, lag, _ptr(order), _ptr(offset), G, _ptr(xmom),
                                         m._stream()))
        return xmom

    def torch_route():
        return torch_lag_moments(state, ref, n, lag, G)

    def dispersion():
        m._check(m.L.umpcBatchDispersion(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, _ptr(mom),
                                         m._stream()))
        return mom

    def propagators():
        m._check(m.L.umpcBatchPropagators(m.h, _ptr(xmom), n, G, _ptr(prop), m._stream()))
        return prop

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the results agree
        _, xk = route(kernel)
        _, dk = route(dispersion)
        route(propagators)
    xk = xk.clone()
    assert torch.equal(xk[..., 2:8].view(torch.int64), dk[..., 2:8].view(torch.int64)), "S1a is not the dispersion kernel's S1"
    assert torch.equal(xk[..., 14:35].view(torch.int64), dk[..., 8:29].view(torch.int64)), "S2a is not the dispersion kernel's S2"
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, xt = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    assert torch.equal(xk[..., 0:2], xt[..., 0:2]), "counts differ"
    assert float((xk[..., 2:92] - xt[..., 2:]).abs().max()) < 1e-9, "moments differ"
    del xt
    tk, tt, td = [], [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
        td.append(route(dispersion)[0])
    tk, tt, td = sorted(tk), sorted(tt), sorted(td)
    tp = route(propagators)[0]
    usable = int((prop[..., 2] == 0).sum())
    med = lambda v: v[len(v) // 2]
    nbytes = 96.0 * B * n + 768.0 * n * G
    lines = ["umpcBatchLagMoments vs the torch composition of the same 92 numbers and vs umpcBatchDispersion "
             "(tools/time_propagators.py), commit %s" % commit,
             "B = %d as %d contiguous cells of 64, steps = %d, lag = %d, fp32, reference table; %d repetitions, routes alternating, "
             "device events" % (B, G, n, lag, a.reps),
             "kernel (lag moments)   min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "dispersion kernel      min %.3f ms   median %.3f ms   max %.3f ms   (same window, same run: 12 words and 27 sums)"
             % (td[0], med(td), td[-1]),
             "ratio torch / kernel   %.2f (median)" % (med(tt) / med(tk)),
             "ratio kernel / dispersion kernel   %.2f (median; twice the words, three times the folded doubles)" % (med(tk) / med(td)),
             "kernel, algorithmic bytes (96 B per robot-step read, 768 B per step and group written): %.1f MB -> %.0f GB/s (median)"
             % (nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB)"
             % (n * G * 92 * 8 / 1e6, peak / 1e6, tables / 1e6),
             "propagators, once      %.3f ms (%d rows, %d usable)" % (tp, n * G, usable)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
