#!/usr/bin/env python3
"""Times umpcBatchScore against the torch composition of the same twelve rows, on the same tables, in one process.

    python tools/time_score.py [--B 65536] [--steps 200] [--reps 20] [--out profiles/score_timing.txt]

Shape of record: B = 65 536, 200 steps, fp32, all records on (state, out, status) and a reference table. Device events
around each call after a warm call of each route; the two routes alternate inside the loop, so that both see the same clock
state. Written out: both times (min, median and max over the repetitions, so that the spread is on record), their ratio, the achieved GB/s of the kernel over the
ALGORITHMIC bytes (60 B read per robot-step, 48 B written per robot), and the peak memory the torch route allocates on top
of the tables (torch.cuda.max_memory_allocated). The bar is the torch route: that is what a user would otherwise write.
UMPC_SCORE_NT=1 in the environment times the kernel's non-temporal variant."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from robobee3d_amd.batch import BatchUprightMPC, _ptr  # noqa: E402


def torch_score(state, out, status, ref, tol, after, taulim, step0):
    """the twelve rows as array expressions (finite inputs: nothing is skipped)"""
    n = out.shape[0]
    st = state[int(after):int(after) + n]
    ep = (st[:, 0:3] - ref[:n, 0:3]).square().sum(1)
    es = (st[:, 9:12] - ref[:n, 6:9]).square().sum(1)
    ok = torch.isfinite(ep) & torch.isfinite(es) & torch.isfinite(out[:, 1:3]).all(1)
    k = torch.arange(step0, step0 + n, device=ep.device, dtype=ep.dtype)[:, None]
    over = ep > tol * tol
    big = torch.full_like(ep, float("inf"))
    first = torch.where(over, k, big).amin(0)
    rows = [ok.sum(0).to(ep.dtype), ep.sum(0), ep.amax(0), ep[-1], es.sum(0), es.amax(0),
            out[:, 1:3].clamp(-taulim, taulim).square().sum((0, 1)), st[:, 0:3].square().sum((0, 1)),
            (status != 1).sum(0).to(ep.dtype), torch.where(torch.isinf(first), -torch.ones_like(first), first),
            torch.where(over, k, -torch.ones_like(ep)).amax(0), (~ok).sum(0).to(ep.dtype)]
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_score.py needs the MI355X: a timing taken anywhere else says nothing")
    B, n, tol = a.B, a.steps, 2.0
    m = BatchUprightMPC(B, torch.float32)
    dev = m.device
    g = torch.Generator(device=dev).manual_seed(1)
    ref = torch.randn((n, 9, B), device=dev, generator=g)
    state = torch.randn((n + 1, 18, B), device=dev, generator=g)
    state[:n, 0:3] += ref[:, 0:3]
    out = 70.0 * torch.randn((n, 9, B), device=dev, generator=g)
    status = torch.randint(1, 3, (n, B), device=dev, generator=g, dtype=torch.int32)
    score = torch.empty((12, B), device=dev)
    taulim = float(m.prm.taulim)

    def kernel():
        m._check(m.L.umpcBatchScoreInit(m.h, _ptr(score), m._stream()))
        m._check(m.L.umpcBatchScore(m.h, _ptr(state), _ptr(out), _ptr(status), _ptr(ref), None, 0, n, 0, 0, tol, 0,
                                    _ptr(score), m._stream()))
        return score

    def route(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    tables = torch.cuda.memory_allocated(dev)
    for _ in range(3):                                                           # warm calls, and the two results agree
        _, sk = route(kernel)
    sk = sk.clone()
    route(lambda: torch_score(state, out, status, ref, tol, 0, taulim, 0))
    torch.cuda.reset_peak_memory_stats(dev)
    _, stt = route(lambda: torch_score(state, out, status, ref, tol, 0, taulim, 0))
    peak = torch.cuda.max_memory_allocated(dev) - tables
    rel = ((sk - stt).abs() / stt.abs().clamp_min(1e-30)).amax(1)
    assert torch.equal(sk[[0, 8, 9, 10, 11]], stt[[0, 8, 9, 10, 11]]) and float(rel.max()) < 1e-3, rel
    del stt
    tk, tt = [], []
    for _ in range(a.reps):
        tk.append(route(kernel)[0])
        tt.append(route(lambda: torch_score(state, out, status, ref, tol, 0, taulim, 0))[0])
    tk, tt = sorted(tk), sorted(tt)
    med = lambda v: v[len(v) // 2]
    nbytes = 60.0 * B * n + 48.0 * B
    lines = ["umpcBatchScore vs the torch composition of the same twelve rows (tools/time_score.py)",
             "B = %d, steps = %d, fp32, all records on, reference table; %d repetitions, routes alternating, device events"
             % (B, n, a.reps),
             "non-temporal loads: %s" % ("on" if os.environ.get("UMPC_SCORE_NT", "0") not in ("", "0") else "off"),
             "kernel (init + score)  min %.3f ms   median %.3f ms   max %.3f ms" % (tk[0], med(tk), tk[-1]),
             "torch route            min %.3f ms   median %.3f ms   max %.3f ms" % (tt[0], med(tt), tt[-1]),
             "ratio torch / kernel   %.2f (median)" % (med(tt) / med(tk)),
             "kernel, algorithmic bytes (60 B per robot-step read, 48 B per robot written): %.1f MB -> %.0f GB/s (median)"
             % (nbytes / 1e6, nbytes / med(tk) / 1e6),
             "torch route, peak memory allocated beyond the tables: %.1f MB (the tables: %.1f MB)" % (peak / 1e6, tables / 1e6)]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
