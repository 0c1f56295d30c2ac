"""The Ruiz speculation of the fp32 lane step on the MI355X (asmstep.StepGen.ruiz; the CPU side is
tests/test_ruiz_fast_path.py): two wavefronts of the lane form, one of which restarts its steps through the exact body."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEFAULT_W = np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])          # rows ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom
B, K, GLOBAL = 128, 3, 65536
EXTREME, RESTART = 70, 100       # robots of wavefront 1: the weights of test_limit_scaling_exact_path; wvf = 1e14
TOL_T, TOL_A = 3e-5, 3e-5        # tests/test_gpu_parity.py


def tol_tau(ref):
    return np.maximum(2e-2, 1e-3 * np.abs(ref))


def _weights(restart=True):
    W = np.tile(DEFAULT_W[:, None], (1, B))
    W[5, EXTREME], W[7, EXTREME] = 5e5, 2e-5
    if restart:
        W[5, RESTART] = 1e14     # still out of limit_scaling's range in pass 2: wavefront 1 restarts every step
    return W


def _rollout(torch, st, ref, W, lo, n, launches=1):
    from robobee3d_amd.batch import BatchUprightMPC
    m = BatchUprightMPC(n, torch.float32, global_batch=GLOBAL, plant_mode=1)
    m.set_state(st[:, lo:lo + n].copy(), ref[:, lo:lo + n].copy())
    m.set_weights(W[:, lo:lo + n].copy())
    for _ in range(launches):
        m.rollout(K // launches)
    torch.cuda.synchronize()
    assert "asm" in m.kernel_name and "quad" not in m.kernel_name
    return m


WORDS = ("state", "ctrl", "out", "stats", "status", "info")


def test_two_wavefronts_one_restarting(oracle_built):
    """B = 128 as a block of a 65 536-robot job (lane form), K = 3 in one launch, per-robot weights: wavefront 0 default,
    wavefront 1 with robot 70 at (wvf=5e5, wmom=2e-5) and robot 100 at wvf = 1e14, which forces the restart.
      * every robot with ordinary weights against the fp64 oracle's 3-step rollout: the fp32 closed-loop band of
        tests/test_gpu_parity.py (1.5e-3 mm, 3e-4; thrust 3e-5, moments max(2e-2, 1e-3 |u|), accdes 3e-5);
      * robot 70 at the tolerances of test_limit_scaling_exact_path. Those are the tolerances of ONE controller step from
        given inputs (after three closed-loop steps with these weights the fp32 and fp64 trajectories already solve
        different QPs: the CPU interpreter of the exact-only stream is 0.32 away in the moment against a bound of 0.05,
        7.7e-4 in the state), so every one of the three steps is compared with the oracle's step from the SAME state and
        controller record; robot 100 likewise;
      * the restart is per wavefront and leaks nowhere: the same batch in two calls of 64 robots is bit-identical, and with
        robot 100 back at the default weights (no restart) every other robot of its wavefront is bit-identical too."""
    import torch
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import hover_initial_conditions
    assert torch.cuda.is_available(), "this test needs the MI355X"
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    W = _weights()
    full = _rollout(torch, st, ref, W, 0, B)
    # fp64 oracle, ordinary robots
    s_o = st.astype(np.float64)
    c_o = np.zeros((127, B)); c_o[124:] = 1
    out_o, _, _ = oracle_built.batch_rollout(s_o, c_o, ref.astype(np.float64), K, dtype=np.float64, perm=perm, plant_mode=1,
                                             weights=W)
    s = full.state.cpu().numpy().astype(np.float64)
    out = full.out.cpu().numpy().astype(np.float64)
    assert np.isfinite(s).all() and np.isfinite(out).all()
    ordinary = np.array([b for b in range(B) if b not in (EXTREME, RESTART)])
    dp = np.abs(s[0:3, ordinary] - s_o[0:3, ordinary]).max()
    ds = np.abs(s[3:, ordinary] - s_o[3:, ordinary]).max()
    print("ordinary robots: |dp| %.3e mm, |dR|,|ddq| %.3e, |d thrust| %.3e, |d accdes| %.3e" % (
        dp, ds, np.abs(out[0, ordinary] - out_o[0, ordinary]).max(), np.abs(out[3:, ordinary] - out_o[3:, ordinary]).max()))
    assert dp <= 1.5e-3 and ds <= 3e-4
    assert np.abs(out[0, ordinary] - out_o[0, ordinary]).max() <= TOL_T
    assert np.all(np.abs(out[1:3, ordinary] - out_o[1:3, ordinary]) <= tol_tau(out_o[1:3, ordinary]))
    assert np.abs(out[3:, ordinary] - out_o[3:, ordinary]).max() <= TOL_A
    # the two extreme robots, step by step (K launches of one step == one launch of K steps, bit for bit)
    from robobee3d_amd.batch import BatchUprightMPC
    one = BatchUprightMPC(B, torch.float32, global_batch=GLOBAL, plant_mode=1)
    one.set_state(st.copy(), ref.copy())
    one.set_weights(W.copy())
    sel = [EXTREME, RESTART]
    for k in range(K):
        s64 = np.ascontiguousarray(one.state.cpu().numpy()[:, sel]).astype(np.float64)
        c64 = np.ascontiguousarray(one.ctrl.cpu().numpy()[:, sel]).astype(np.float64)
        one.rollout(1)
        o = one.out.cpu().numpy().astype(np.float64)[:, sel]
        uq, _, _ = oracle_built.batch_rollout(s64, c64, np.ascontiguousarray(ref[:, sel]).astype(np.float64), 1,
                                              dtype=np.float64, perm=perm, plant_mode=1, weights=np.ascontiguousarray(W[:, sel]))
        print("step %d, robots 70 / 100: |d thrust| %s |d accdes| %s |d moment| %s" % (
            k, np.abs(o[0] - uq[0]), np.abs(o[3:] - uq[3:]).max(axis=0), np.abs(o[1:3] - uq[1:3]).max(axis=0)))
        assert np.abs(o[0] - uq[0]).max() < 1e-4 and np.abs(o[3:] - uq[3:]).max() < 1e-4
        assert np.all(np.abs(o[1:3] - uq[1:3]) <= np.maximum(5e-2, 2e-3 * np.abs(uq[1:3])))
    for n in WORDS:
        assert torch.equal(getattr(one, n), getattr(full, n)), n
    # the same batch in two calls of 64
    for lo in (0, 64):
        half = _rollout(torch, st, ref, W, lo, 64)
        for n in WORDS:
            a, b = getattr(half, n), getattr(full, n)
            assert torch.equal(a, b[lo:lo + 64] if n == "status" else b[:, lo:lo + 64]), (n, lo)
    # without the restart: every other robot of wavefront 1 is what it was
    calm = _rollout(torch, st, ref, _weights(restart=False), 0, B)
    keep = torch.as_tensor([b for b in range(B) if b != RESTART], device=full.state.device)
    for n in WORDS:
        a, b = getattr(calm, n), getattr(full, n)
        assert torch.equal(a.index_select(a.dim() - 1, keep), b.index_select(b.dim() - 1, keep)), n
