#!/usr/bin/env python3
"""Times umpcBatchGram and umpcBatchProject (M = 3) against the torch composition of the Gram matrices and against
umpcBatchDispersion over the same window, on the same tables, in one process.

    python tools/time_gram.py [--B 65536] [--steps 200] [--reps 20] [--commit ID] [--out profiles/gram_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, state record and a reference table. Device events
around each call after warm calls of each route; the routes alternate inside the loop, so that all see the same clock state. The
group index is built once, before the loop: it belongs to the sweep, not to a call. The torch route is what a user would
otherwise write: the differences, the finiteness select and the scales into Y [cells, 64, 6 steps] in fp64, then torch.bmm(Y,
Y^T) -- rocBLAS behind a temporary of the size of the tables. Written out: the times (min, median and max over the repetitions),
the ratios, the achieved GB/s over the ALGORITHMIC bytes (48 B read per robot-step), the fp64 MFMA rate of the Gram kernel (issued:
12 tiles per block and k-block, of which 10 are stored), the peak memory the torch route allocates on top of the tables, and one
probe of what sets the Gram kernel's pace: the same launch on an index whose every cell lists robots 0..63, so that the loads are
served from cache and the staging, the LDS traffic and the MFMAs remain. The only bar is the torch route including the construction
of its operand. Ratios, GB/s and GFLOP/s are recorded, not asserted."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402

SCALE = (1.0, 1.0, 1.0, 0.5, 0.5, 0.5)


def torch_gram(state, ref, after, cells, scale):
    """Gram [cells, 64, 64] as array expressions: z [steps, 6, B] in the dtype, the select and the scales in fp64, Y [cells, 64,
    6 steps] made contiguous, torch.bmm"""
    n, B = ref.shape[0], ref.shape[2]
    st = state[int(after):int(after) + n]
    z = torch.cat([st[:, 0:3] - ref[:, 0:3], st[:, 12:15] - ref[:, 3:6]], 1)             # [steps, 6, B]
    ok = torch.isfinite(st[:, 0:3]).all(1) & torch.isfinite(st[:, 12:15]).all(1) & torch.isfinite(ref[:, 0:6]).all(1)
    y = torch.where(ok[:, None], z.to(torch.float64), 0.0) * scale[None, :, None]
    Y = y.reshape(n, 6, cells, B // cells).permute(2, 3, 0, 1).reshape(cells, B // cells, 6 * n).contiguous()
    return torch.bmm(Y, Y.transpose(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gram.py needs the MI355X: a timing taken anywhere else says nothing")
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
    order_hot = (torch.arange(B, device=dev, dtype=torch.int32) % 64).contiguous()      # every cell lists robots 0..63
    gram = torch.empty((G, 66, 64), dtype=torch.float64, device=dev)
    gram_hot = torch.empty_like(gram)
    proj = torch.empty((n, G, 32), dtype=torch.float64, device=dev)
    mom = torch.empty((n, G, 32), dtype=torch.float64, device=dev)
    weights = torch.randn((3, B), dtype=torch.float64, device=dev, generator=g)
    sc = (C.c_double * 6)(*SCALE)
    scale_t = torch.tensor(SCALE, dtype=torch.float64, device=dev)

    def kernel():
        m._check(m.L.umpcBatchGram(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, sc, 0, _ptr(gram),
                                   m._stream()))
        return gram

    def kernel_hot():
        m._check(m.L.umpcBatchGram(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order_hot), _ptr(offset), G, sc, 0,
                                   _ptr(gram_hot), m._stream()))
        return gram_hot

    def project():
        m._check(m.L.umpcBatchProject(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, _ptr(weights), 3,
                                      _ptr(proj), m._stream()))
        return proj

    def dispersion():
        m._check(m.L.umpcBatchDispersion(m.h, _ptr(state), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset), G, _ptr(mom),
                                         m._stream()))
        return mom

    def torch_route():
        return torch_gram(state, ref, 0, G, scale_t)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        _, gk = route(kernel)
        route(kernel_hot)
        route(project)
        route(dispersion)
    gk = gk.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, gt = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    assert bool((gk[:, 64] == n).all()) and bool((gk[:, 65, 0] == n).all()), "counts differ"
    rel = float(((gk[:, :64] - gt).abs() / (gk[:, :64].diagonal(dim1=1, dim2=2).max(1).values[:, None, None])).max())
    assert rel < 1e-12, "Gram matrices differ (%.3e of the largest diagonal entry)" % rel
    del gt
    tk, th, tp, td, tt = [], [], [], [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
        tp.append(route(project)[0])
        td.append(route(dispersion)[0])
        th.append(route(kernel_hot)[0])
    tk, th, tp, td, tt = sorted(tk), sorted(th), sorted(tp), sorted(td), sorted(tt)
    med = lambda v: v[len(v) // 2]
    row = lambda name, v: "%-26s min %.3f ms   median %.3f ms   max %.3f ms" % (name, v[0], med(v), v[-1])
    nbytes = 48.0 * B * n
    kblocks = (6 * n + 3) // 4
    issued, stored = G * 12.0 * kblocks * 2048, G * 10.0 * kblocks * 2048
    lines = ["umpcBatchGram and umpcBatchProject vs the torch composition and umpcBatchDispersion (tools/time_gram.py), commit %s" % commit,
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, reference table, scales %s; %d repetitions, routes alternating, "
             "device events" % (B, G, n, SCALE, a.reps),
             row("Gram kernel", tk),
             row("torch route (Y + bmm)", tt),
             row("projection kernel, M = 3", tp),
             row("dispersion kernel", td),
             row("Gram kernel, cached loads", th),
             "ratio torch / Gram kernel        %.2f (median)" % (med(tt) / med(tk)),
             "ratio Gram / dispersion kernel   %.2f   projection / dispersion %.2f (median)" % (med(tk) / med(td), med(tp) / med(td)),
             "algorithmic bytes (48 B per robot-step read): %.1f MB -> Gram %.0f GB/s, projection %.0f GB/s, dispersion %.0f GB/s (median)"
             % (nbytes / 1e6, nbytes / med(tk) / 1e6, nbytes / med(tp) / 1e6, nbytes / med(td) / 1e6),
             "fp64 MFMA (v_mfma_f64_16x16x4_f64, 2048 flop each): %.2f GFLOP issued (12 tile slots per block), %.2f stored (10 tiles) -> "
             "%.1f TFLOP/s issued over the whole kernel, %.1f TFLOP/s with the loads served from cache"
             % (issued / 1e9, stored / 1e9, issued / med(tk) / 1e9, issued / med(th) / 1e9),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB); "
             "the Gram kernel allocates nothing" % (G * 64 * 64 * 8 / 1e6, peak / 1e6, tables / 1e6)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(tk) < med(tt):
        raise SystemExit("the Gram kernel's median is not below the torch route's")


if __name__ == "__main__":
    main()
