"""Cost of the step history (BatchUprightMPC.record_history) in fp32: one K-step launch with state + out recorded against
(a) the same launch with history off and (b) K single-step launches with the device copies a user without the feature
needs (state and out into slices of their own tables after every step). The first recording launch writes fresh pages
(first touch); it is timed apart from the repeats, which reuse the tables with the cursor reset.
usage (GPU box): python tools/time_step_history.py [--steps 500] [--batches 65536 4096] [--reps 3]"""
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
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    K = a.steps
    for B in a.batches:
        st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
        m = BatchUprightMPC(B, torch.float32, plant_mode=1)

        def reset():
            m.set_state(st, ref)
            m.reset_controller()
        reset()
        m.rollout(K)                                        # warm-up: clocks, code objects
        off, on, singles = [], [], []
        reset()
        m.record_history(K)
        first = _timed(lambda: m.rollout(K))                # fresh pages
        for _ in range(a.reps):
            m.record_history(None)
            reset()
            off.append(_timed(lambda: m.rollout(K)))
        m.record_history(K)
        m.rollout(K)                                        # touch the new tables once
        for _ in range(a.reps):
            reset()
            m.rewind_history()
            on.append(_timed(lambda: m.rollout(K)))
        tabs = m.history()
        m.record_history(None)
        s_tab, o_tab = tabs["state"], tabs["out"]

        def k_launches():
            s_tab[0].copy_(m.state)
            for k in range(K):
                m.rollout(1)
                s_tab[k + 1].copy_(m.state)
                o_tab[k].copy_(m.out)
        for _ in range(a.reps):
            reset()
            singles.append(_timed(k_launches))
        print(json.dumps({"B": B, "K": K, "kernel": m.kernel_name, "ms_per_step_history_off": [x / K for x in off],
                          "ms_per_step_history_on": [x / K for x in on], "ms_per_step_history_on_first_touch": first / K,
                          "ms_per_step_k_single_launches_with_copies": [x / K for x in singles],
                          "table_GB": (s_tab.numel() + o_tab.numel()) * 4 / 1e9}))


if __name__ == "__main__":
    main()
