"""Cost of velocity impulses (BatchUprightMPC.set_impulses) in fp32: one K-step launch with a table against (a) the same
launch without one and (b) K single-step launches with `state[12:18] += tab[k]` in between, what a user without the feature
needs. usage (GPU box): python tools/time_impulses.py [--steps 20] [--batches 65536 4096] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions_device  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    K = a.steps
    for B in a.batches:
        st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
        tab = torch.zeros((K, 6, B), dtype=torch.float32, device="cuda")
        tab[K // 2, 1] = 2.0
        m = BatchUprightMPC(B, torch.float32, plant_mode=1)

        def reset():
            m.set_state(st, ref)
            m.reset_controller()

        def with_table():
            m.set_impulses(tab)
            m.rollout(K)

        def without():
            m.set_impulses(None)
            m.rollout(K)

        def launches():
            m.set_impulses(None)
            for k in range(K):
                m.rollout(1)
                m.state[12:18] += tab[k]
        res = {}
        for name, fn in (("table", with_table), ("no_table", without), ("k_launches_with_adds", launches)):
            reset()
            fn()                                          # warm-up
            ts = []
            for _ in range(a.reps):
                reset()
                ts.append(_timed(fn) / K)
            res[name] = dict(ms_per_step_min=min(ts), ms_per_step_max=max(ts))
        print(json.dumps(dict(B=B, K=K, kernel=m.kernel_name, **res)))


if __name__ == "__main__":
    main()
