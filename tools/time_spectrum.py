#!/usr/bin/env python3
"""Times umpcBatchSpectrum against the torch composition of the same numbers and against umpcBatchResponse over the same
window, on the same tables; then umpcBatchSpectrumPower and umpcBatchSpectrumGroups once each.

    python tools/time_spectrum.py [--B 65536] [--steps 200] [--K 32] [--reps 20] [--commit ID] [--out profiles/spectrum_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, reference table, signal ep, K = 32, Hann window.
The tile size of the sums kernel (8 or 16 frequencies per block, UMPC_SPEC_KT) is read once per process, so each candidate
runs in a child process of its own (started fresh, one after the other; this process never opens the device). In a child the
three routes alternate inside one loop, so that all see the same clock state; device events around each call after warm
calls of each route; min, median and max over the repetitions. Each child also times the sums kernel at K = 8 and K = 16 on the
same tables: with tiles of 8, K = 8 is one tile per block, and with tiles of 16, K = 16 is one tile per block over exactly the
same loads with twice the arithmetic -- the pair says whether the loads or the arithmetic set the pace. The sums of the two
tile sizes must be equal bit for bit (a digest is compared).
The one pass condition: at the tile size the library runs by default, the kernel's median is below the torch route's."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_spectrum(torch, state, ref, basis, K):
    """the same numbers as array expressions: the difference in the dtype, widened, one matrix product with the basis (sum w y,
    C_j, S_j), a second reduction for sum w y y, and the counts"""
    n, B = ref.shape[0], ref.shape[2]
    d = state[:n, 0:3] - ref[:, 0:3]                                                  # [steps, 3, B] in the dtype
    ok = torch.isfinite(state[:n, 0:3]).all(1) & torch.isfinite(ref[:, 0:3]).all(1)      # [steps, B]
    dd = d.double()                                                                   # the fp64 [steps, 3, B] temporary
    proj = (basis.t() @ dd.reshape(n, 3 * B)).reshape(1 + 2 * K, 3, B)
    wyy = basis[:, 0].reshape(n, 1, 1) * dd * dd
    cnt = ok.to(torch.float64).sum(0)
    return cnt, n - cnt, proj, wyy.sum(0)


def child(a):
    import numpy as np
    import torch
    from robobee3d_amd import score as S
    from robobee3d_amd.batch import BatchUprightMPC, _ptr
    B, n, K = a.B, a.steps, a.K
    G = B // 64
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    tables = torch.cuda.memory_allocated(dev)
    bases, sums = {}, {}
    for k in sorted({8, 16, K}):
        nu = (np.arange(k) + 0.7) / (2.0 * k + 1.0)
        bases[k] = (torch.as_tensor(S.spectrum_basis(nu, n, "hann")).to(dev), nu)
        sums[k] = torch.empty((S.spectrum_sum_rows(k), B), dtype=torch.float64, device=dev)
    nu_r = torch.full((B,), 0.025, dtype=torch.float64, device=dev)
    rsums = torch.empty((33, B), dtype=torch.float64, device=dev)

    def kernel(k=K):
        m._check(m.L.umpcBatchSpectrumInit(m.h, k, _ptr(sums[k]), m._stream()))
        m._check(m.L.umpcBatchSpectrum(m.h, 0, _ptr(state), None, _ptr(ref), None, _ptr(bases[k][0]), 0, k, 0, n, 0, 0,
                                       _ptr(sums[k]), m._stream()))
        return sums[k]

    def torch_route():
        return torch_spectrum(torch, state, ref, bases[K][0], K)

    def response():
        m._check(m.L.umpcBatchResponseInit(m.h, _ptr(rsums), m._stream()))
        m._check(m.L.umpcBatchResponse(m.h, _ptr(state), _ptr(ref), None, _ptr(nu_r), 0, n, 0, 0, 0, _ptr(rsums), m._stream()))
        return rsums

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    for _ in range(3):
        route(kernel), route(response), route(lambda: kernel(8)), route(lambda: kernel(16))
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, (cnt, skip, proj, wyy) = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    sk = kernel().clone()
    torch.cuda.synchronize()
    chan = 2 + 2 * K
    assert torch.equal(sk[0], cnt) and torch.equal(sk[1], skip), "counts differ"
    dev_max = 0.0
    for c in range(3):
        at = 2 + c * chan
        dev_max = max(dev_max, float((sk[at] - proj[0, c]).abs().max()), float((sk[at + 1] - wyy[c]).abs().max()),
                      float((sk[at + 2:at + chan] - proj[1:, c]).abs().max()))
    assert dev_max < 1e-9, "sums differ from the torch route: %g" % dev_max
    del cnt, skip, proj, wyy
    t = {"kernel": [], "torch": [], "response": [], "k8": [], "k16": []}
    for _ in range(a.reps):
        t["kernel"].append(route(kernel)[0])
        t["torch"].append(route(torch_route)[0])
        t["response"].append(route(response)[0])
        t["k8"].append(route(lambda: kernel(8))[0])
        t["k16"].append(route(lambda: kernel(16))[0])
    # power and groups, once each (after a warm call)
    wsum = S.spectrum_wsum(bases[K][0].cpu().numpy())
    freq = np.ascontiguousarray(bases[K][1] * 200.0)
    import ctypes as C
    spec = torch.empty((3, 12, B), device=dev)
    power = torch.empty((3, K, B), device=dev)
    index = m.group_index(torch.arange(B, device=dev, dtype=torch.int32) // 64, G)
    gspec = torch.empty((G, 3, 2 + K), dtype=torch.float64, device=dev)

    def power_call():
        m._check(m.L.umpcBatchSpectrumPower(m.h, _ptr(sk), wsum.ctypes.data_as(C.POINTER(C.c_double)),
                                            freq.ctypes.data_as(C.POINTER(C.c_double)), K, n, K // 2, _ptr(power), _ptr(spec), m._stream()))

    def groups_call():
        m._check(m.L.umpcBatchSpectrumGroups(m.h, _ptr(power), _ptr(spec), _ptr(index[0]), _ptr(index[1]), G, K, _ptr(gspec), m._stream()))

    route(power_call), route(groups_call)
    tp, tg = route(power_call)[0], route(groups_call)[0]
    entered = int((spec[:, 0] > 0).sum())
    digest = hashlib.sha256(sk.cpu().numpy().tobytes()).hexdigest()
    print("RESULT " + json.dumps(dict(kt=a.child, times={k: sorted(v) for k, v in t.items()}, peak=peak, tables=tables, power=tp, groups=tg,
                                      entered=entered, digest=digest, torch_dev=dev_max)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_timing.txt"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    if a.child:
        return child(a)
    commit = a.commit
    if commit is None:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    res = {}
    for kt in (8, 16):
        env = dict(os.environ, UMPC_SPEC_KT=str(kt))
        cmd = [sys.executable, os.path.abspath(__file__), "--B", str(a.B), "--steps", str(a.steps), "--K", str(a.K), "--reps", str(a.reps),
               "--child", str(kt)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:
            # (a child that failed may have faulted the device: nothing more is started on it)
            raise SystemExit("the run with tiles of %d failed (exit %d):\n%s" % (kt, p.returncode, (p.stdout + p.stderr)[-3000:]))
        res[kt] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    if res[8]["digest"] != res[16]["digest"]:
        raise SystemExit("the sums of the two tile sizes differ")
    med = lambda v: v[len(v) // 2]
    B, n, K, G = a.B, a.steps, a.K, a.B // 64
    rows = 2 + 3 * (2 + 2 * K)
    lines = ["umpcBatchSpectrum vs the torch composition of the same numbers and vs umpcBatchResponse (tools/time_spectrum.py), commit %s" % commit,
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, reference table, signal ep, K = %d, Hann; %d repetitions, routes "
             "alternating, device events; UMPC_SPEC_SLICES = 2" % (B, G, n, K, a.reps),
             "the sums of the two tile sizes are equal bit for bit (sha256 %s..); largest |kernel - torch| over the sums %.2e"
             % (res[16]["digest"][:12], max(res[8]["torch_dev"], res[16]["torch_dev"]))]
    for kt in (8, 16):
        t = res[kt]["times"]
        tiles = (K + kt - 1) // kt
        nbytes = 24.0 * B * n * tiles + 16.0 * rows * B
        lines += ["-- tiles of %d frequencies (%d tiles per block of 64 robots) --" % (kt, tiles)]
        for name, key in (("kernel (sums, K = %d)" % K, "kernel"), ("torch route", "torch"), ("umpcBatchResponse", "response"),
                          ("kernel, K = 8", "k8"), ("kernel, K = 16", "k16")):
            lines.append("%-24s min %.3f ms   median %.3f ms   max %.3f ms" % (name, t[key][0], med(t[key]), t[key][-1]))
        lines += ["ratio torch / kernel     %.2f (median)" % (med(t["torch"]) / med(t["kernel"])),
                  "kernel, bytes moved (24 B per robot-step and tile read, 16 B per sum read and written): %.1f MB -> %.0f GB/s; "
                  "%.2f G fp64 operations -> %.1f Tops/s (median)"
                  % (nbytes / 1e6, nbytes / med(t["kernel"]) / 1e6, (12.0 * K + 14.0 * tiles) * B * n / 1e9,
                     (12.0 * K + 14.0 * tiles) * B * n / med(t["kernel"]) / 1e9)]
    t16, t8 = res[16]["times"], res[8]["times"]
    lines += ["same loads, twice the arithmetic: one tile of 16 at K = 16 %.3f ms against one tile of 8 at K = 8 %.3f ms (medians): ratio %.2f"
              % (med(t16["k16"]), med(t8["k8"]), med(t16["k16"]) / med(t8["k8"])),
              "torch route, peak memory allocated beyond the tables (its results of %.1f MB included): %.1f MB (the tables: %.1f MB)"
              % ((1 + 2 * K + 1) * 3 * B * 8 / 1e6, res[8]["peak"] / 1e6, res[8]["tables"] / 1e6),
              "power, once             %.3f ms (%d of %d channel fits entered)" % (res[8]["power"], res[8]["entered"], 3 * B),
              "groups, once            %.3f ms (%d groups x 3 channels x %d frequencies)" % (res[8]["groups"], G, K)]
    best = 16 if med(t16["kernel"]) <= med(t8["kernel"]) else 8
    lines.append("faster tile size at this shape: %d (the library's default is 8; UMPC_SPEC_KT=16 selects the other)" % best)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(t8["kernel"]) < med(t8["torch"]):
        raise SystemExit("the kernel's median is not below the torch route's")


if __name__ == "__main__":
    main()
