#!/usr/bin/env python3
"""Times umpcBatchCrossSpectrum at both tile sizes against umpcBatchSpectrum("ep") at the same shape in the same process and
against the torch composition of the same sums; then umpcBatchCrossSpectrumGroups and umpcBatchTransfer once each.

    python tools/time_transfer.py [--B 65536] [--steps 200] [--K 32] [--reps 20] [--commit ID] [--out profiles/transfer_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, the tracking pair (x = pdes, y = p), K = 32,
Hann window. The tile size of the sums kernel (8 or 4 frequencies per block, UMPC_XS_KT) is read at every call, so one process
runs both; the routes alternate inside one loop, so that all see the same clock state; device events around each call after
warm calls of each route; min, median and max over the repetitions. The sums of the two tile sizes must be equal bit for bit.
The pass issues exactly twice the fp64 products and sums of umpcBatchSpectrum over the same loads, so the expectation printed
at the end is: at most 2.2 x that call's time as measured beside it, and below the torch route. The tool reports; it fails
only when sums differ."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_cross_spectrum(torch, state, ref, basis, K):
    """the same numbers as array expressions: both signals widened into one fp64 [steps, 6, B] temporary, one matrix product
    with the basis (sum w v, C_j, S_j), a second reduction for sum w v v, and the counts"""
    n, B = ref.shape[0], ref.shape[2]
    x, y = ref[:, 0:3], state[:n, 0:3]
    ok = torch.isfinite(x).all(1) & torch.isfinite(y).all(1)                           # [steps, B]
    v = torch.cat((x, y), 1).double()                                                  # the fp64 [steps, 6, B] temporary
    proj = (basis.t() @ v.reshape(n, 6 * B)).reshape(1 + 2 * K, 6, B)
    wvv = basis[:, 0].reshape(n, 1, 1) * v * v
    cnt = ok.to(torch.float64).sum(0)
    return cnt, n - cnt, proj, wvv.sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer_timing.txt"))
    a = ap.parse_args()
    if a.B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    import numpy as np
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import BatchUprightMPC, _ptr
    B, n, K, G = a.B, a.steps, a.K, a.B // 64
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    tables = torch.cuda.memory_allocated(dev)
    nu = (np.arange(K) + 0.7) / (2.0 * K + 1.0)
    host = S.spectrum_basis(nu, n, "hann")
    basis = torch.as_tensor(host).to(dev)
    xsums = torch.empty((S.cross_spectrum_sum_rows(K), B), dtype=torch.float64, device=dev)
    ssums = torch.empty((S.spectrum_sum_rows(K), B), dtype=torch.float64, device=dev)

    def xs(kt):
        def call():
            os.environ["UMPC_XS_KT"] = str(kt)
            m._check(m.L.umpcBatchCrossSpectrumInit(m.h, K, _ptr(xsums), m._stream()))
            m._check(m.L.umpcBatchCrossSpectrum(m.h, 0, _ptr(state), _ptr(ref), None, None, _ptr(basis), 0, K, 0, n, 0, 0, 0,
                                                _ptr(xsums), m._stream()))
            return xsums
        return call

    def spectrum():
        m._check(m.L.umpcBatchSpectrumInit(m.h, K, _ptr(ssums), m._stream()))
        m._check(m.L.umpcBatchSpectrum(m.h, 0, _ptr(state), None, _ptr(ref), None, _ptr(basis), 0, K, 0, n, 0, 0, _ptr(ssums), m._stream()))
        return ssums

    def torch_route():
        return torch_cross_spectrum(torch, state, ref, basis, K)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(3):
        route(xs(8)), route(xs(4)), route(spectrum)
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, (cnt, skip, proj, wvv) = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    s8 = xs(8)().clone()
    s4 = xs(4)().clone()
    torch.cuda.synchronize()
    if not torch.equal(s8, s4):
        raise SystemExit("the sums of the two tile sizes differ")
    chan = 2 + 2 * K
    if not (torch.equal(s8[0], cnt) and torch.equal(s8[1], skip)):
        raise SystemExit("counts differ from the torch route")
    dev_max = 0.0
    for c in range(6):
        at = 2 + c * chan
        dev_max = max(dev_max, float((s8[at] - proj[0, c]).abs().max()), float((s8[at + 1] - wvv[c]).abs().max()),
                      float((s8[at + 2:at + chan] - proj[1:, c]).abs().max()))
    if not dev_max < 1e-9:
        raise SystemExit("sums differ from the torch route: %g" % dev_max)
    del cnt, skip, proj, wvv
    t = {"xs8": [], "xs4": [], "spectrum": [], "torch": []}
    for _ in range(a.reps):
        t["xs8"].append(route(xs(8))[0])
        t["xs4"].append(route(xs(4))[0])
        t["spectrum"].append(route(spectrum)[0])
        t["torch"].append(route(torch_route)[0])
    t = {k: sorted(v) for k, v in t.items()}
    # groups and rows, once each (after a warm call)
    wsum = S.spectrum_wsum(host)
    index = m.group_index(torch.arange(B, device=dev, dtype=torch.int32) // 64, G)
    gx = torch.empty((G, 3, 2 + 4 * K), dtype=torch.float64, device=dev)
    tf = torch.empty((G, 3, K, 12), dtype=torch.float64, device=dev)

    def groups_call():
        m._check(m.L.umpcBatchCrossSpectrumGroups(m.h, _ptr(s8), wsum.ctypes.data_as(C.POINTER(C.c_double)), K, n, _ptr(index[0]),
                                                  _ptr(index[1]), G, _ptr(gx), m._stream()))

    def rows_call():
        m._check(m.L.umpcBatchTransfer(m.h, _ptr(gx), G, K, _ptr(tf), m._stream()))

    route(groups_call), route(rows_call)
    tg, tr = route(groups_call)[0], route(rows_call)[0]
    entered = int((tf[..., 0] > 0).sum())
    med = lambda v: v[len(v) // 2]
    rows = 2 + 6 * chan
    lines = ["umpcBatchCrossSpectrum vs umpcBatchSpectrum(ep) beside it and vs the torch composition of the same sums (tools/time_transfer.py), commit %s" % commit,
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, the tracking pair (x = pdes, y = p), K = %d, Hann; %d repetitions, "
             "routes alternating in one process, device events; UMPC_SPEC_SLICES = 2" % (B, G, n, K, a.reps),
             "the sums of the two tile sizes are equal bit for bit; largest |kernel - torch| over the sums %.2e" % dev_max]
    for name, key in (("sums kernel, tiles of 8", "xs8"), ("sums kernel, tiles of 4", "xs4"), ("umpcBatchSpectrum(ep)", "spectrum"),
                      ("torch route", "torch")):
        lines.append("%-26s min %.3f ms   median %.3f ms   max %.3f ms" % (name, t[key][0], med(t[key]), t[key][-1]))
    for kt, key in ((8, "xs8"), (4, "xs4")):
        tiles = (K + kt - 1) // kt
        ops = (24.0 * K + 26.0 * tiles) * B * n
        nbytes = 24.0 * B * n * tiles + 16.0 * rows * B
        lines.append("tiles of %d: %d tiles per block of 64 robots; %.1f MB moved (24 B per robot-step and tile, 16 B per sum) -> %.0f GB/s; "
                     "%.2f G fp64 operations -> %.1f Tops/s; %.2f x umpcBatchSpectrum(ep); torch / kernel %.2f (medians)"
                     % (kt, tiles, nbytes / 1e6, nbytes / med(t[key]) / 1e6, ops / 1e9, ops / med(t[key]) / 1e9,
                        med(t[key]) / med(t["spectrum"]), med(t["torch"]) / med(t[key])))
    best = 8 if med(t["xs8"]) <= med(t["xs4"]) else 4
    tb = med(t["xs%d" % best])
    lines += ["torch route, peak memory allocated beyond the tables (its results of %.1f MB included): %.1f MB (the tables: %.1f MB)"
              % ((1 + 2 * K + 1) * 6 * B * 8 / 1e6, peak / 1e6, tables / 1e6),
              "groups, once              %.3f ms (%d groups x 3 channels x %d frequencies, %d tiles of 8)" % (tg, G, K, (K + 7) // 8),
              "rows, once                %.3f ms (%d of %d rows entered)" % (tr, entered, G * 3 * K),
              "faster tile size at this shape: %d (the library launches tiles of 4; UMPC_XS_KT=8 selects tiles of 8)" % best,
              "expectation, at most 2.2 x umpcBatchSpectrum(ep): %.2f x -- %s" % (tb / med(t["spectrum"]), "met" if tb <= 2.2 * med(t["spectrum"]) else "NOT met"),
              "expectation, below the torch route: %.3f ms against %.3f ms -- %s" % (tb, med(t["torch"]), "met" if tb < med(t["torch"]) else "NOT met")]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
