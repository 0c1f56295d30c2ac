#!/usr/bin/env python3
"""Times umpcBatchEnsembleQuantiles against umpcBatchEnsemble and against the torch route (e_p over [steps, B], reshaped to
[steps, cells, 64], sorted), on the same tables, in one process.

    python tools/time_quantiles.py [--B 65536] [--steps 200] [--reps 20] [--out profiles/quantile_timing.txt]

Shape of record, that of profiles/ensemble_timing.txt: B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, the state
and out records and a reference table, seven probabilities (0, 0.05, 0.25, 0.5, 0.75, 0.95, 1) of e_p. Device events around
each call after warm calls of each route; the three routes alternate inside the loop, so that all see the same clock state.
The group index is built once, before the loop: it belongs to the sweep, not to a call. Written out: the three times (min,
median and max over the repetitions), the ratios torch / kernel and kernel / ensemble, the achieved GB/s of the kernel over
the ALGORITHMIC bytes (56 B read per robot-step: the ensemble's 60 without the status word; 72 B written per step and
group), and the peak memory the torch route allocates on top of the tables. The bar is the torch route: that is what a user
would otherwise write. The ratio to the ensemble kernel is written down, not judged: it reads the same words and folds
where this one sorts."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402

PROBS = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


def torch_quantiles(state, out, ref, after, cells, probs):
    """the rows as array expressions: e_p over [steps, B], seen as [steps, cells, B / cells], sorted along the cell (finite
    inputs: nothing is skipped, so every cell has n = B / cells and one rank per probability serves all of them)"""
    n, B = out.shape[0], out.shape[2]
    st = state[int(after):int(after) + n]
    ep = (st[:, 0:3] - ref[:n, 0:3]).square().sum(1)
    es = (st[:, 9:12] - ref[:n, 6:9]).square().sum(1)
    ok = torch.isfinite(ep) & torch.isfinite(es) & torch.isfinite(out[:, 1:3]).all(1)
    size = B // cells
    v = ep.reshape(n, cells, size).sort(2).values
    ks = [min(size - 1, max(0, int(-(-(p * size) // 1)) - 1)) for p in probs]
    scored = ok.reshape(n, cells, size).sum(2).to(torch.float64)
    return torch.cat([scored[..., None], (size - scored)[..., None], v[..., ks].to(torch.float64)], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_quantiles.py needs the MI355X: a timing taken anywhere else says nothing")
    import ctypes as C
    B, n, nq = a.B, a.steps, len(PROBS)
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
    ens = torch.empty((n, G, 16), dtype=torch.float64, device=dev)
    quant = torch.empty((n, G, 2 + nq), dtype=torch.float64, device=dev)
    order, offset = m.group_index(torch.arange(B, device=dev, dtype=torch.int32) // 64, G)
    probs = (C.c_double * nq)(*PROBS)

    def kernel():
        m._check(m.L.umpcBatchEnsembleQuantiles(m.h, _ptr(state), _ptr(out), _ptr(ref), None, 0, n, 0, 0, _ptr(order), _ptr(offset),
                                                G, 0, probs, nq, _ptr(quant), m._stream()))
        return quant

    def ensemble_kernel():
        m._check(m.L.umpcBatchEnsemble(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(ref), None, 0, n, 0, 2.0, 0, _ptr(order),
                                       _ptr(offset), G, _ptr(ens), m._stream()))
        return ens

    def torch_route():
        return torch_quantiles(state, out, ref, 0, G, PROBS)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        _, qk = route(kernel)
        _, ek = route(ensemble_kernel)
    qk = qk.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, qt = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    assert torch.equal(qk[..., :2], qt[..., :2]), "count rows differ"
    rel = ((qk[..., 2:] - qt[..., 2:]).abs() / qt[..., 2:].abs().clamp_min(1e-30)).amax((0, 1))
    assert float(rel.max()) < 1e-5, rel
    assert torch.equal(qk[..., 2], ek[..., 5]) and torch.equal(qk[..., 1 + nq], ek[..., 4]), "p = 0 / 1 are not the ensemble's min / max"
    del qt
    tk, tt, te = [], [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
        te.append(route(ensemble_kernel)[0])
    tk, tt, te = sorted(tk), sorted(tt), sorted(te)
    med = lambda v: v[len(v) // 2]
    nbytes = 56.0 * B * n + 8.0 * (2 + nq) * n * G
    lines = ["umpcBatchEnsembleQuantiles vs the torch route (e_p over [steps, B], sorted per cell) and vs umpcBatchEnsemble (tools/time_quantiles.py)",
             "B = %d as %d contiguous cells of 64, steps = %d, fp32, state and out records, reference table, %d probabilities of "
             "e_p; %d repetitions, routes alternating, device events" % (B, G, n, nq, a.reps),
             "kernel (quantiles)     min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "ensemble kernel        min %.3f ms   median %.3f ms   max %.3f ms" % (te[0], med(te), te[-1]),
             "ratio torch / kernel      %.2f (median)" % (med(tt) / med(tk)),
             "ratio kernel / ensemble   %.2f (median)" % (med(tk) / med(te)),
             "kernel, algorithmic bytes (56 B per robot-step read, %d B per step and group written): %.1f MB -> %.0f GB/s (median)"
             % (8 * (2 + nq), nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (its result of %.1f MB included): %.1f MB (the tables: %.1f MB)"
             % (n * G * 8 * (2 + nq) / 1e6, peak / 1e6, tables / 1e6)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(tk) < med(tt):
        raise SystemExit("the kernel's median is not below the torch route's")


if __name__ == "__main__":
    main()
