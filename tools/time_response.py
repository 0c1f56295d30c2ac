#!/usr/bin/env python3
"""Times umpcBatchResponse + umpcBatchResponseFit against the torch composition of the same rows, on the same tables, in one
process.

    python tools/time_response.py [--B 65536] [--steps 200] [--reps 20] [--out profiles/response_timing.txt]

Shape of record: B = 65 536, 200 steps, fp32, a reference table, one frequency per robot in [0.05, 0.45] revolutions per step.
Device events around each call after warm calls of each route; the two routes alternate inside the loop, so that both see
the same clock state. The torch route is what a user would otherwise write: the phase, cosine and sine as [steps, B] fp64
tables, the 33 sums as products and sums over them, the fit as [B] expressions. Written out: both times (min, median and max
over the repetitions), their ratio, the achieved GB/s of the kernel pair over the ALGORITHMIC bytes (24 B read per
robot-step, 8 B of nu and 2 x 264 B of sums per robot, 144 B of rows written per robot), and the peak memory the torch
route allocates on top of the tables (torch.cuda.max_memory_allocated). The one pass condition is that the kernel pair's
median is below the torch route's. UMPC_SCORE_NT=1 in the environment times the kernel's non-temporal variant."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_sums(state, ref, nu, step0, after):
    """the 33 sums as array expressions over [steps, B] fp64 tables (finite inputs: nothing is skipped)"""
    n, B = ref.shape[0], ref.shape[2]
    k = torch.arange(step0, step0 + n, device=nu.device, dtype=torch.float64)[:, None]
    x = k * nu[None]
    u = x - x.floor()
    c, s = torch.cos(2 * math.pi * u), torch.sin(2 * math.pi * u)
    rows = [torch.full((B,), float(n), device=nu.device, dtype=torch.float64), torch.zeros(B, device=nu.device, dtype=torch.float64),
            c.sum(0), s.sum(0), (c * c).sum(0), (c * s).sum(0)]
    for j in range(3):
        y, r = state[int(after):int(after) + n, j].to(torch.float64), ref[:, j].to(torch.float64)
        rows += [y.sum(0), (y * c).sum(0), (y * s).sum(0), (y * y).sum(0), r.sum(0), (r * c).sum(0), (r * s).sum(0), (r * r).sum(0),
                 (y * r).sum(0)]
    return torch.stack(rows)


def torch_fit(sm, dtype):
    """the twelve rows per axis from the sums, the expressions of score.response_fit_reference on [B] tensors"""
    n, Sc, Ss, Scc, Scs = sm[0], sm[2], sm[3], sm[4], sm[5]
    l11 = n.sqrt()
    l21, l31 = Sc / l11, Ss / l11
    d2 = Scc - l21 * l21
    l22 = d2.sqrt()
    l32 = (Scs - l21 * l31) / l22
    d3 = ((n - Scc) - l31 * l31) - l32 * l32
    l33 = d3.sqrt()
    fit = (n >= 3) & (n > 1e-9 * n) & (d2 > 1e-9 * n) & (d3 > 1e-9 * n)

    def solve(b0, b1, b2):
        z0 = b0 / l11
        z1 = (b1 - l21 * z0) / l22
        z2 = ((b2 - l31 * z0) - l32 * z1) / l33
        a2 = z2 / l33
        a1 = (z1 - l32 * a2) / l22
        return ((z0 - l21 * a1) - l31 * a2) / l11, a1, a2

    nan = torch.full_like(n, float("nan"))
    out = []
    for j in range(3):
        x = sm[6 + 9 * j:15 + 9 * j]
        ay, ar = solve(x[0], x[1], x[2]), solve(x[4], x[5], x[6])
        yamp2, ramp2 = ay[1] * ay[1] + ay[2] * ay[2], ar[1] * ar[1] + ar[2] * ar[2]
        re, im = ay[1] * ar[1] + ay[2] * ar[2], ay[1] * ar[2] - ay[2] * ar[1]
        res = (x[3] - ((ay[0] * x[0] + ay[1] * x[1]) + ay[2] * x[2])) / n
        rows = [n, sm[1], yamp2, ramp2, (yamp2 / ramp2).sqrt(), torch.atan2(im, re), re / ramp2, im / ramp2, ay[0], ar[0],
                res.clamp_min(0), (ay[1] - ar[1]).square() + (ay[2] - ar[2]).square()]
        rows = [rows[0] * fit, rows[1]] + [torch.where(fit, v, nan) for v in rows[2:]]
        out.append(torch.stack(rows))
    return torch.stack(out).to(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "response_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_response.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n = a.B, a.steps
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    nu = 0.05 + 0.4 * torch.rand((B,), device=dev, generator=g, dtype=torch.float64)
    k = torch.arange(n + 1, device=dev, dtype=torch.float64)[:, None]
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    ref[:, 0] += (20.0 * torch.sin(2 * math.pi * k[:n] * nu[None])).float()
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    del k
    sums = torch.empty((33, B), dtype=torch.float64, device=dev)
    resp = torch.empty((3, 12, B), device=dev)

    def kernel():
        m._check(m.L.umpcBatchResponseInit(m.h, _ptr(sums), m._stream()))
        m._check(m.L.umpcBatchResponse(m.h, _ptr(state), _ptr(ref), None, _ptr(nu), 0, n, 0, 0, 0, _ptr(sums), m._stream()))
        m._check(m.L.umpcBatchResponseFit(m.h, _ptr(sums), _ptr(resp), m._stream()))
        return resp

    def torch_route():
        return torch_fit(torch_sums(state, ref, nu, 0, 0), torch.float32)

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        route(kernel)
    sk, rk = sums.clone(), resp.clone()
    route(torch_route)
    torch.cuda.reset_peak_memory_stats(dev)
    held = torch.cuda.memory_allocated(dev)
    _, rt = route(torch_route)
    peak = torch.cuda.max_memory_allocated(dev) - held
    st = torch_sums(state, ref, nu, 0, 0)
    assert torch.equal(sk[0:2], st[0:2]), "count rows differ"
    assert float((sk - st).abs().max()) < 1e-9 * n * float(state[:, 0:3].abs().max()) ** 2, "sum rows differ"
    amp = [2, 3, 8, 9]
    rel = ((rk[:, amp] - rt[:, amp]).abs() / rt[:, amp].abs().clamp_min(1e-3)).amax()
    assert float(rel) < 1e-4, rel
    assert float((torch.sqrt(rk[0, 3]) - 20.0).abs().median()) < 0.5, "the planted amplitude is not found"
    del st, rt
    tk, tt = [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(torch_route)[0])
    tk, tt = sorted(tk), sorted(tt)
    med = lambda v: v[len(v) // 2]
    nbytes = 24.0 * B * n + (8.0 + 3 * 264.0 + 144.0) * B
    lines = ["umpcBatchResponse + umpcBatchResponseFit vs the torch composition of the same rows (tools/time_response.py)",
             "B = %d, steps = %d, fp32, reference table, nu per robot in [0.05, 0.45]; %d repetitions, routes alternating, device events"
             % (B, n, a.reps),
             "non-temporal loads: %s" % ("on" if os.environ.get("UMPC_SCORE_NT", "0") not in ("", "0") else "off"),
             "kernels (init + sums + fit)  min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route                  min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "ratio torch / kernels        %.2f (median)" % (med(tt) / med(tk)),
             "kernels, algorithmic bytes (24 B per robot-step read; per robot 8 B of nu, 3 x 264 B of sums zeroed, added to and "
             "read, 144 B of rows written): %.1f MB -> %.0f GB/s (median)" % (nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables (temporaries): %.1f MB (the tables: %.1f MB)" % (peak / 1e6, tables / 1e6)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not med(tk) < med(tt):
        raise SystemExit("the kernels' median is not below the torch route's")


if __name__ == "__main__":
    main()
