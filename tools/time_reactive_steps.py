"""Cost of the reactive baseline on the tables (BatchUprightMPC.reactive_steps = umpcBatchReactiveRollout) in fp32: one launch
of K closed-loop steps with every record on (state / out / status / info history, impulse table) and with all of them off,
against the only route to a state table without the entry: K x (reactive_rollout(nsub) + a device copy of `state` into a
table slice). Device events, the routes alternating, min / median / max over the repetitions.
usage (GPU box): python tools/time_reactive_steps.py [--steps 40] [--batches 65536 4096] [--reps 20] [--commit ID] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions_device  # noqa: E402


def _commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown"


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reactive_steps_timing.txt"))
    a = ap.parse_args()
    K = a.steps
    lines = ["umpcBatchReactiveRollout vs K x (umpcBatchReactive(nsub) + state copy) (tools/time_reactive_steps.py)",
             "commit %s; fp32, K = %d steps of nsub = 25, handle task helix, default gains; %d repetitions, routes alternating, "
             "device events" % (a.commit or _commit(), K, a.reps)]
    for B in a.batches:
        st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
        imp = torch.zeros((K, 6, B), dtype=torch.float32, device="cuda")
        imp[K // 2, 1] = 2.0
        table = torch.empty((K + 1, 18, B), dtype=torch.float32, device="cuda")      # the copy route's state table

        def handle():
            m = BatchUprightMPC(B, torch.float32, taulim=10.0)
            m.set_task("helix", trajAmp=50, trajFreq=1, dz=0.1, useY=False)
            return m
        rec, bare, old = handle(), handle(), handle()
        rec.record_history(K, state=True, out=True, status=True, info=True)
        rec.set_impulses(imp)
        nsub = int(old.prm.nsub)

        def reset(m):
            m.set_state(st, ref)
            m.set_task("helix", trajAmp=50, trajFreq=1, dz=0.1, useY=False)          # (the clock back to 0)

        def records_on():
            rec.reactive_steps(K)

        def records_off():
            bare.reactive_steps(K)

        def k_launches_with_copies():
            table[0].copy_(old.state)
            for k in range(K):
                old.reactive_rollout(nsub)
                table[k + 1].copy_(old.state)
        routes = (("one launch, all records on", rec, records_on), ("one launch, records off", bare, records_off),
                  ("K launches + K state copies", old, k_launches_with_copies))
        ts = {name: [] for name, _, _ in routes}
        for rep in range(a.reps + 1):                                          # (repetition 0 is the warm-up)
            for name, m, fn in routes:
                reset(m)
                if m is rec:
                    m.rewind_history(0)
                    m.rewind_impulses(0)
                t = _event_ms(fn)
                if rep:
                    ts[name].append(t)
        lines.append("B = %d" % B)
        for name, _, _ in routes:
            v = ts[name]
            lines.append("  %-30s min %.3f ms   median %.3f ms   max %.3f ms   (%.4f ms per step, median)"
                         % (name, min(v), statistics.median(v), max(v), statistics.median(v) / K))
        med = {n: statistics.median(v) for n, v in ts.items()}
        lines.append("  ratio K launches / one launch with records  %.2f (median);  records on / off  %.3f (median)"
                     % (med["K launches + K state copies"] / med["one launch, all records on"],
                        med["one launch, all records on"] / med["one launch, records off"]))
        # the three routes ran the same closed loop
        torch.cuda.synchronize()
        same = bool(torch.equal(rec.history()["state"][K], rec.state))
        lines.append("  history slice K == state: %s" % same)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
