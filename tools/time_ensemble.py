#!/usr/bin/env python3
"""Times umpcBatchEnsemble against the torch composition of the same sixteen rows and against umpcBatchScore, on the same
tables, in one process.

    python tools/time_ensemble.py [--B 65536] [--steps 200] [--reps 20] [--out profiles/ensemble_timing.txt]

Shape of record: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, all records on (state, out, status) and a
reference table. Device events around each call after warm calls of each route; the three routes alternate inside the loop,
so that all see the same clock state. The group index is built once, before the loop: it belongs to the sweep, not to a call.
Written out: the three times (min, median and max over the repetitions), the ratios torch / kernel and kernel / score, the
achieved GB/s of the kernel over the ALGORITHMIC bytes (60 B read per robot-step, 128 B written per step and group), and the
peak memory the torch route allocates on top of the tables (torch.cuda.max_memory_allocated). The bar is the torch route:
that is what a user would otherwise write. The score kernel reads the same 60 B per robot-step and reduces over the steps
instead of over the robots: its time is what the stream alone costs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_ensemble(state, out, status, ref, tol, after, taulim, cells):
    """the sixteen rows as array expressions over [steps, B] temporaries seen as [steps, cells, B / cells] (finite inputs:
    nothing is skipped); everything that crosses robots in fp64, as the kernel has it"""
    n, B = out.shape[0], out.shape[2]
    st = state[int(after):int(after) + n]
    d = st[:, 0:3] - ref[:n, 0:3]
    ep = d.square().sum(1)
    es = (st[:, 9:12] - ref[:n, 6:9]).square().sum(1)
    tau2 = out[:, 1:3].clamp(-taulim, taulim).square().sum(1)
    ok = torch.isfinite(ep) & torch.isfinite(es) & torch.isfinite(out[:, 1:3]).all(1)
    c = lambda x: x.reshape(n, cells, B // cells)
    f = lambda x: c(x).to(torch.float64)
    epd, esd, taud = f(ep), f(es), f(tau2)
    arg = c(ep).argmax(2) + torch.arange(cells, device=ep.device)[None] * (B // cells)
    rows = [f(ok).sum(2), f(~ok).sum(2), epd.sum(2), epd.square().sum(2), epd.amax(2), epd.amin(2), esd.sum(2), esd.amax(2),
            taud.sum(2), taud.amax(2), f(ep > tol * tol).sum(2), f(status != 1).sum(2), f(d[:, 0]).sum(2), f(d[:, 1]).sum(2),
            f(d[:, 2]).sum(2), arg.to(torch.float64)]
    return torch.stack(rows, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ensemble.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n, tol = a.B, a.steps, 2.0
    if B % 64:
        raise SystemExit("B must be a multiple of 64 (cells of 64 contiguous robots)")
    G = B // 64
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    out = 70.0 * torch.randn((n, 9, B), device=dev, generator=g)
    status = torch.randint(1, 3, (n, B), device=dev, generator=g, dtype=torch.int32)
    score = torch.empty((12, B), device=dev)
    ens = torch.empty((n, G, 16), dtype=torch.float64, device=dev)
    order, offset = m.group_index(torch.arange(B, device=dev, dtype=torch.int32) // 64, G)
    taulim = float(m.prm.taulim)

    def kernel():
        m._check(m.L.umpcBatchEnsemble(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(ref), None, 0, n, 0, tol, 0, _ptr(order),
                                       _ptr(offset), G, _ptr(ens), m._stream()))
        return ens

    def score_kernel():
        m._check(m.L.umpcBatchScoreInit(m.h, _ptr(score), m._stream()))
        m._check(m.L.umpcBatchScore(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(ref), None, 0, n, 0, 0, tol, 0,
                                    _ptr(score), m._stream()))
        return score

    def torch_route():
        return torch_ensemble(state, out, status, ref, tol, 0, taulim, G)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        _, ek = route(kernel)
        route(score_kernel)
    ek = ek.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, et = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    exact = [0, 1, 10, 11, 15]
    assert torch.equal(ek[..., exact], et[..., exact]), "exact rows differ"
    pos = [2, 3, 4, 5, 6, 7, 8, 9]
    rel = ((ek[..., pos] - et[..., pos]).abs() / et[..., pos].abs().clamp_min(1e-30)).amax((0, 1))
    assert float(rel.max()) < 1e-5, rel
    assert float((ek[..., 12:15] - et[..., 12:15]).abs().max()) < 1e-3
    del et
    tk, tt, ts = [], [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
        ts.append(route(score_kernel)[0])
    tk, tt, ts = sorted(tk), sorted(tt), sorted(ts)
    med = lambda v: v[len(v) // 2]
    nbytes = 60.0 * B * n + 128.0 * n * G
    lines = ["umpcBatchEnsemble vs the torch composition of the same sixteen rows and vs umpcBatchScore (tools/time_ensemble.py)",
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, all records on, reference table; %d repetitions, routes "
             "alternating, device events" % (B, G, n, a.reps),
             "kernel (ensemble)      min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "score (init + score)   min %.3f ms   median %.3f ms   max %.3f ms" % (ts[0], med(ts), ts[-1]),
             "ratio torch / kernel   %.2f (median)" % (med(tt) / med(tk)),
             "ratio kernel / score   %.2f (median)" % (med(tk) / med(ts)),
             "kernel, algorithmic bytes (60 B per robot-step read, 128 B per step and group written): %.1f MB -> %.0f GB/s (median)"
             % (nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB)"
             % (n * G * 128 / 1e6, peak / 1e6, tables / 1e6)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(tk) < med(tt):
        raise SystemExit("the kernel's median is not below the torch route's")


if __name__ == "__main__":
    main()
