"""The reactive baseline on the tables of the MPC rollout (umpcBatchReactiveRollout / BatchUprightMPC.reactive_steps): K
closed-loop steps of nsub substeps in one launch with a reference per robot (the handle's task, per-robot tasks, or the table
of set_reference_trajectory held over each step), the impulse table and the step history, so that the reactive half of the
reference's MPC-versus-reactive comparisons (template/uprightmpc2.py:214-246, :272-303) is scored like the MPC half.
CPU: the declaration and the export, the refusal of a NULL handle before any HIP call, no scratch in any form of the kernel,
task_arrays (the task-name parsing factored out of task_table).
GPU (B = 70: two wavefronts, the second partial; K <= 4; both dtypes; taulim = 10 like test_reactive.py): equality with
umpcBatchReactive bit for bit, one launch = K launches bit for bit on the table path, oracle parity with six per-robot
(task, parameters) combinations under a gain grid and two pushes, the history's semantics, scoring against task_table through
score(ref_table=...), the refusals, partition invariance."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from conftest import record_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NSUB, DTS, TAULIM = 70, 25, 0.2, 10.0
DTYPES = ["float64", "float32"]
TOL = {"float64": 1e-9, "float32": 2e-3}          # tests/test_reactive.py: max |d| / max(1, |s|)
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from robobee3d_amd import _lib
    _lib.build()
    return _lib


def test_header_declares_and_library_exports_the_entry(lib):
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+umpcBatchReactiveRollout\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/umpc_mi355x.h does not declare umpcBatchReactiveRollout"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 13 and args[0] == "umpc_batch_t *h" and args[1] == "int K" and args[2] == "int every"
    assert "const int32_t *task" in args and args[-1] == "void *stream"
    assert "umpcBatchReactiveRollout" in lib.EXPORTS
    assert hasattr(C.CDLL(lib.SO_PATH), "umpcBatchReactiveRollout")


def test_null_handle_is_refused_before_any_hip_call(lib):
    L = lib.lib()
    assert L.umpcBatchReactiveRollout(None, 1, 1, *([None] * 10)) == -1
    assert b"umpcBatchReactiveRollout" in L.umpcLastError()


def test_no_form_of_the_kernel_has_a_scratch_frame(lib):
    """3 reference sources x 2 dtypes, each with ScratchSize 0 in the compiler's own resource remarks; the recorded limits
    of the other kernels are the parent's, byte for byte."""
    res = json.load(open(lib.RESOURCES_JSON))
    mine = {k: v for k, v in res.items() if "umpc_reactive_steps_kernel" in k}
    assert len(mine) >= 6, sorted(mine)
    for k, v in mine.items():
        assert v["ScratchSize"] == 0, (k, v)
    lim = json.load(open(lib.RESOURCE_LIMITS))
    assert hashlib.sha256(json.dumps({k: lim[k] for k in STEP_PATH_LIMITS}, sort_keys=True).encode()).hexdigest() == STEP_PATH_LIMITS_SHA256


# the entries the file had when this kernel came, limits and notes, in their canonical dump: entries of later kernels do not enter
STEP_PATH_LIMITS = ("umpc_dropin_quad_kernel", "umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel", "umpc_rollout_kernelIdLb1ELb1E",
                    "umpc_rollout_kernelIdLb1ELb1ELb1E", "umpc_rollout_kernelIfLb0E", "umpc_task_table_kernel")
STEP_PATH_LIMITS_SHA256 = "7435920afaa15d095fab3ea386384aa98e277f30d7fe2dd65e3d802365232e4b"


def test_task_arrays_one_name_and_the_default_task():
    from robobee3d_amd.batch import task_arrays
    ids, P = task_arrays(5, "helix", {}, "ref")
    assert ids.dtype == np.int32 and ids.tolist() == [1] * 5 and P.dtype == np.float64 and P.shape == (4, 5)
    assert np.array_equal(P, np.tile(np.array([[80.0], [1.0], [0.15], [1.0]]), (1, 5)))
    # tasks None = the default task for every robot, keywords still apply
    ids, P = task_arrays(3, None, {"vdes": 3.0}, "straightAcc")
    assert ids.tolist() == [2] * 3 and np.array_equal(P, np.tile(np.array([[500.0], [3.0], [0.0], [0.0]]), (1, 3)))
    ids, P = task_arrays(2, None, {}, "ref")
    assert ids.tolist() == [0, 0] and not P.any()


def test_task_arrays_names_per_robot_and_task_dependent_defaults():
    """B names; vdes and tend default per task (straightAcc 2 / perch 0.2; flip 200 / perch 500), as set_task does"""
    from robobee3d_amd.batch import task_arrays
    ids, P = task_arrays(5, ["ref", "helix", "straightAcc", "flip", "perch"], {}, "ref")
    assert ids.tolist() == [0, 1, 2, 3, 4]
    want = np.array([[0, 0, 0, 0], [80, 1, 0.15, 1], [500, 2, 0, 0], [100, 200, 0, 0], [500, 100, 450, 0.2]], np.float64).T
    assert np.array_equal(P, want)
    with pytest.raises(ValueError):
        task_arrays(4, ["helix"] * 5, {}, "ref")


def test_task_arrays_per_robot_parameter_arrays_and_unknown_keywords():
    from robobee3d_amd.batch import task_arrays
    names = ["helix", "perch", "helix", "ref"]
    amp, freq = np.array([10.0, 20.0, 30.0, 40.0]), np.array([0.5, 1.5, 2.5, 3.5])
    ids, P = task_arrays(4, names, {"trajAmp": amp, "trajFreq": freq, "useY": False, "trotend": 400}, "ref")
    assert ids.tolist() == [1, 4, 1, 0]
    # a keyword fills the slot of the robots whose task has it, and of no other robot
    want = np.array([[10, 0.5, 0.15, 0], [500, 100, 400, 0.2], [30, 2.5, 0.15, 0], [0, 0, 0, 0]], np.float64).T
    assert np.array_equal(P, want)
    with pytest.raises(TypeError, match="trajAmplitude"):
        task_arrays(4, names, {"trajAmplitude": 1.0}, "ref")


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _tdt(dtype):
    import torch
    return getattr(torch, dtype)


def _ndt(dtype):
    return np.float32 if dtype == "float32" else np.float64


def _gains(nb, dtype, lo=0):
    """a (ks0, ks1) grid over the robots like gainTuningSims(useMPC=False), keyed by the GLOBAL robot index"""
    b = np.arange(lo, lo + nb)
    g = np.tile(np.array([[5e-3], [5e-1], [1e-1], [1e0], [0], [0]]), (1, nb))
    g[4], g[5] = 5 + 15 * (b % 7) / 6.0, 50 + 150 * (b % 10) / 9.0
    return g.astype(_ndt(dtype))


def _handle(dtype, nb=B, **kw):
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    st, ref = hover_initial_conditions(B, 7, _ndt(dtype))
    m = BatchUprightMPC(nb, _tdt(dtype), taulim=TAULIM, **kw)
    if nb == B:
        m.set_state(st, ref)
    return m, st, ref


def _eq(a, b):
    import torch
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def _cursors(m):
    return (m.ref_cursor, m.history_cursor, m.impulse_cursor)


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_handle_task_equals_the_substep_entry_bit_for_bit(dtype, every):
    """no table, no per-robot task, the handle follows a helix: reactive_steps(3) against reactive_rollout(75) on a second
    handle, and one more call each so that a non-zero clock enters too"""
    import torch
    gains = _gains(B, dtype)
    ms = []
    for _ in range(2):
        m, _, _ = _handle(dtype)
        m.set_task("helix", trajAmp=50, trajFreq=2, dz=0.1, useY=True)
        ms.append(m)
    new, old = ms
    for K in (3, 1):
        new.reactive_steps(K, gains, every=every)
        old.reactive_rollout(K * NSUB, gains, every=every)
        torch.cuda.synchronize()
        assert _eq(new.state, old.state) and _eq(new.out[0:3], old.out[0:3]) and _eq(new.stats, old.stats)
        assert new.time_ms == old.time_ms
    assert new.time_ms == pytest.approx(4 * NSUB * DTS) and float(new.stats.abs().min()) > 0


def _table_handle(dtype, K, seed):
    """a handle with a reference table of K random slices, an impulse table of K non-zero slices and all four records"""
    import torch
    rng = np.random.default_rng(seed)
    m, _, _ = _handle(dtype)
    tab = rng.normal(scale=3.0, size=(K, 9, B))
    kick = rng.uniform(0.25, 1.0, size=(K, 6, B)) * rng.choice([-1.0, 1.0], size=(K, 6, B)) * np.array([2.0] * 3 + [0.02] * 3)[None, :, None]
    m.set_reference_trajectory(torch.as_tensor(tab))
    m.set_impulses(torch.as_tensor(kick))
    m.record_history(K, state=True, out=True, status=True, info=True)
    for v in m._hist.values():
        v.fill_(7)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_launch_equals_k_launches_bit_for_bit(dtype):
    """the time-free path (a reference table): reactive_steps(4) against four reactive_steps(1) -- state, out, stats, the whole
    history and the three cursors"""
    import torch
    K = 4
    gains = _gains(B, dtype)
    one, many = _table_handle(dtype, K, 11), _table_handle(dtype, K, 11)
    one.reactive_steps(K, gains, every=5)
    for _ in range(K):
        many.reactive_steps(1, gains, every=5)
    torch.cuda.synchronize()
    assert _cursors(one) == _cursors(many) == (K, K, K) and one.time_ms == many.time_ms
    assert _eq(one.state, many.state) and _eq(one.out, many.out) and _eq(one.stats, many.stats)
    h1, h2 = one.history(), many.history()
    for k in ("state", "out", "status", "info"):
        assert h1[k].shape[0] == K + (k == "state") and _eq(h1[k], h2[k]), k
    # the table is what the controller followed: another table gives another run
    other = _table_handle(dtype, K, 12)
    other.reactive_steps(K, gains, every=5)
    assert not _eq(other.state, one.state)


# --- the run the parity, scoring and partition tests share: six (task, parameters) combinations over the 70 robots ---------
K3 = 4
COMBOS = (("helix", 1, (80.0, 1.0, 0.15, 1.0)), ("helix", 1, (30.0, 2.5, 0.15, 1.0)), ("helix", 1, (80.0, 1.0, 0.15, 0.0)),
          ("straightAcc", 2, (500.0, 2.0)), ("perch", 4, (500.0, 100.0, 450.0, 0.2)), ("ref", 0, ()))
GROUP = np.repeat(np.arange(6, dtype=np.int32), [12, 12, 12, 12, 11, 11])     # robots of one task adjacent


def _inputs3(dtype):
    from robobee3d_amd.batch import hover_initial_conditions
    ndt = _ndt(dtype)
    st, ref = hover_initial_conditions(B, 7, ndt)
    ref[0:3] = np.random.default_rng(3).normal(scale=2.0, size=(3, B)).astype(ndt)       # initialPos / the "ref" robots' pdes
    names = [COMBOS[g][0] for g in GROUP]
    params = {"trajAmp": np.where(GROUP == 1, 30.0, 80.0), "trajFreq": np.where(GROUP == 1, 2.5, 1.0), "useY": GROUP != 2}
    kick = np.zeros((K3, 6, B))
    kick[1, 1] = 2.0                                                       # the reference's push, dq[1] += 2
    kick[2, :, ::2] = np.array([0.5, 0.0, -0.3, 0.01, 0.0, -0.02])[:, None]
    return st, ref, names, params, kick.astype(ndt)


def _run3(dtype, lo=0, hi=B):
    """the robots [lo, hi) of the run as a handle of their own, inputs sliced column-wise"""
    import torch
    from robobee3d_amd import shard
    st, ref, names, params, kick = _inputs3(dtype)
    m, _, _ = _handle(dtype, hi - lo, global_batch=B)
    m.set_state(shard.table_block(torch.as_tensor(st), lo, hi), shard.table_block(torch.as_tensor(ref), lo, hi))
    m.set_impulses(shard.impulse_block(torch.as_tensor(kick), lo, hi))
    m.record_history(K3, state=True, out=True, status=True, info=True)
    for v in m._hist.values():
        v.fill_(7)
    tasks = dict(tasks=names[lo:hi], **{k: v[lo:hi] for k, v in params.items()})
    m.reactive_steps(K3, _gains(hi - lo, dtype, lo), **tasks)
    torch.cuda.synchronize()
    return m, tasks


@pytest.fixture(scope="module", params=DTYPES)
def run3(request):
    m, tasks = _run3(request.param)
    return request.param, m, tasks


@pytest.mark.gpu
def test_per_robot_tasks_match_the_oracle_chain(run3, oracle_built):
    """oraclebind.reactive_rollout per combination on its columns, chained in blocks of nsub with t0 advanced and the add in
    between (the method of test_impulses.py::test_reactive_rollout_honours_the_table): every state slice, the final out and
    stats, at the margins of tests/test_reactive.py"""
    dtype, m, _ = run3
    tol = TOL[dtype]
    st, ref, _, _, kick = _inputs3(dtype)
    gains = _gains(B, dtype).astype(np.float64)
    want = np.zeros((K3 + 1, 18, B))
    want[0] = st
    out_o, stats_o = np.zeros((3, B)), np.zeros((2, B))
    for g, (_, tid, tp) in enumerate(COMBOS):
        cols = np.where(GROUP == g)[0]
        so = np.ascontiguousarray(st[:, cols], np.float64)
        ro = np.ascontiguousarray(ref[:, cols], np.float64)
        tp = np.asarray(tp, _ndt(dtype)).astype(np.float64)          # the parameters as the device holds them
        for k in range(K3):
            o_k, s_k, _ = oracle_built.reactive_rollout(so, ro, NSUB, 1, np.ascontiguousarray(gains[:, cols]), taulim=TAULIM,
                                                        task=tid, task_p=tp, t0=k * NSUB * DTS)
            stats_o[:, cols] += s_k
            so[12:18] += kick[k][:, cols]
            want[k + 1][:, cols] = so
        out_o[:, cols] = o_k
    assert m.history_cursor == K3 and m.impulse_cursor == K3 and m.time_ms == pytest.approx(K3 * NSUB * DTS)
    got = m.history()["state"].cpu().numpy().astype(np.float64)
    assert np.array_equal(got[0], st.astype(np.float64)) and np.array_equal(got[K3], m.state.cpu().numpy().astype(np.float64))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    for g, (name, _, _) in enumerate(COMBOS):
        print("REACTIVE-STEPS %s combo %d (%s): max |d state| / max(1, |s|) = %.3e" % (dtype, g, name, err[:, :, GROUP == g].max()))
    record_margin("reactive steps, per-robot tasks " + dtype, "max |d state| / max(1, |s|)", err.max(), tol)
    out = m.out[:3].cpu().numpy().astype(np.float64)
    stats = m.stats.cpu().numpy().astype(np.float64)
    record_margin("reactive steps, per-robot tasks " + dtype, "max |d out|", np.abs(out - out_o).max(), tol)
    record_margin("reactive steps, per-robot tasks " + dtype, "max rel d stats", (np.abs(stats - stats_o) / np.abs(stats_o)).max(),
                  max(tol, 1e-8) * 10)
    assert err.max() < tol
    assert np.allclose(out, out_o, rtol=max(tol, 1e-8) * 10, atol=tol)
    assert np.allclose(stats, stats_o, rtol=max(tol, 1e-8) * 10)
    # the tasks were followed: the combinations ended in different places although their robots started alike
    assert np.abs(got[K3][0:3]).max() > 1e-2


@pytest.mark.gpu
def test_scores_against_the_task_table(run3):
    """score(after=True, ref_table=task_table(...)) of the per-robot task run: the counts, and the sum / max rows against the
    float64 numpy composition of the same tables (bound: the header's (steps + 8) u, times 2 for the numpy side's conversions);
    score_groups over the six combinations"""
    from robobee3d_amd import score as S
    dtype, m, tasks = run3
    tab = m.task_table(K3, t_ms=0.0, **tasks)
    sc = m.score(after=True, ref_table=tab)
    h = m.history()
    want = S.score_reference(h["state"].cpu().numpy(), h["out"].cpu().numpy(), h["status"].cpu().numpy(), tab.cpu().numpy(),
                             0, K3, 0, 0, 10.0, True, TAULIM)
    got = sc.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[0], np.full(B, float(K3))) and not got[8].any() and not got[11].any()
    bound = 2 * (K3 + 8) * U[dtype]
    for r in (1, 2, 4, 6):
        rel = np.max(np.abs(got[r] - want[r]) / np.where(want[r] == 0, 1.0, np.abs(want[r])))
        print("REACTIVE-STEPS score %s row %d: rel %.3e, bound %.3e" % (dtype, r, rel, bound))
        record_margin("reactive steps score " + dtype, "row %d rel" % r, rel, bound)
        assert rel <= bound, (dtype, r, rel)
        assert want[r].max() > 0
    # a part of the run, from another slice of the table on
    part = m.score(first=1, count=2, after=True, ref_table=tab).cpu().numpy().astype(np.float64)
    wantp = S.score_reference(h["state"].cpu().numpy(), h["out"].cpu().numpy(), h["status"].cpu().numpy(), tab.cpu().numpy(),
                              1, 2, 1, 1, 10.0, True, TAULIM)
    assert np.array_equal(part[0], np.full(B, 2.0)) and np.allclose(part[1], wantp[1], rtol=bound, atol=0)
    gs = m.score_groups(sc, GROUP, 6).cpu().numpy()
    assert gs.shape == (6, 8) and gs[:, 0].tolist() == [12, 12, 12, 12, 11, 11] and gs[:, 1].tolist() == gs[:, 0].tolist()
    assert np.allclose(gs, S.group_reference(got, GROUP, 6), rtol=(12 + 8) * U["float64"], atol=0)


@pytest.mark.gpu
def test_a_block_of_robots_equals_its_columns(run3):
    """robots 13..50 as a B = 38 handle on column-sliced inputs (shard.table_block / impulse_block): state, out, stats and the
    whole history bit for bit"""
    from robobee3d_amd import shard
    dtype, m, _ = run3
    lo, hi = 13, 51
    blk, _ = _run3(dtype, lo, hi)
    assert blk.B == 38
    assert _eq(blk.state, shard.table_block(m.state, lo, hi)) and _eq(blk.out, shard.table_block(m.out, lo, hi))
    assert _eq(blk.stats, shard.table_block(m.stats, lo, hi))
    want = shard.history_block(m.history(), lo, hi)
    for k, v in blk.history().items():
        assert _eq(v, want[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_history_semantics(dtype):
    """slice c = the state passed, slice c + K = the state afterwards; out rows 0..2 = the last command, rows 3..8 = 0;
    status 1, info 0; a second call continues the tables"""
    import torch
    m, st, _ = _handle(dtype)
    m.set_task("helix", trajAmp=50, trajFreq=2, dz=0.1, useY=True)
    m.record_history(6, state=True, out=True, status=True, info=True)
    for v in m._hist.values():
        v.fill_(7)
    m.reactive_steps(2, _gains(B, dtype))
    torch.cuda.synchronize()
    h = m.history()
    mid, out_mid = m.state.clone(), m.out.clone()
    assert m.history_cursor == 2 and h["state"].shape[0] == 3 and h["out"].shape[0] == 2
    assert _eq(h["state"][0], torch.as_tensor(st).to(m.device)) and _eq(h["state"][2], mid)
    assert not _eq(h["state"][1], h["state"][0]) and not _eq(h["state"][1], h["state"][2])
    assert _eq(h["out"][1, 0:3], out_mid[0:3]) and not _eq(h["out"][0, 0:3], h["out"][1, 0:3])
    assert not h["out"][:, 3:9].any() and bool((h["status"] == 1).all()) and not h["info"].any()
    assert float(m._hist["state"][3:].min()) == 7 and float(m._hist["out"][2:].min()) == 7       # nothing past the cursor
    m.reactive_steps(3, _gains(B, dtype), every=5)
    torch.cuda.synchronize()
    h = m.history()
    assert m.history_cursor == 5 and _eq(h["state"][2], mid) and _eq(h["state"][5], m.state) and _eq(h["out"][1, 0:3], out_mid[0:3])
    assert _eq(h["out"][4, 0:3], m.out[0:3]) and not h["out"][:, 3:9].any()
    assert bool((h["status"] == 1).all()) and not h["info"].any()
    assert float(m._hist["state"][6:].min()) == 7 and float(m._hist["out"][5:].min()) == 7
    assert float(m._hist["status"][5:].min()) == 7 and float(m._hist["info"][5:].min()) == 7
    # any record may be off
    m2, _, _ = _handle(dtype)
    m2.record_history(2, state=False, out=True)
    m2.reactive_steps(2)
    torch.cuda.synchronize()
    assert m2.history()["state"] is None and _eq(m2.history()["out"][1, 0:3], m2.out[0:3])


@pytest.mark.gpu
def test_refusals_leave_the_handle_and_the_state_alone():
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    m, st, _ = _handle("float32")
    before = m.state.clone()

    def refused(match, *a, **kw):
        t, c = m.time_ms, _cursors(m)
        with pytest.raises(RuntimeError, match=match):
            m.reactive_steps(*a, **kw)
        torch.cuda.synchronize()
        assert m.time_ms == t and _cursors(m) == c and _eq(m.state, before)

    refused("umpcBatchReactiveRollout.*every", 1, every=4)              # 4 does not divide nsub = 25
    refused("umpcBatchReactiveRollout", 0)
    refused("umpcBatchReactiveRollout", 1, every=0)
    z = BatchUprightMPC(B, torch.float32, taulim=TAULIM, nsub=0)
    z.set_state(st)
    with pytest.raises(RuntimeError, match="umpcBatchReactiveRollout.*nsub"):
        z.reactive_steps(1)
    assert z.time_ms == 0 and _eq(z.state, before)
    # K past the end of the history, then of the impulse table, then of the trajectory: each is checked before the launch
    m.record_history(2)
    refused("step history", 3)
    m.record_history(8)
    m.set_impulses(torch.zeros((2, 6, B)))
    refused("impulse table", 3)
    m.set_impulses(torch.zeros((8, 6, B)))
    m.set_reference_trajectory(torch.zeros((2, 9, B)))
    refused("reference trajectory", 3)
    # per-robot tasks and a table exclude each other; the substep entry still refuses a table
    refused("umpcBatchReactiveRollout.*exclude", 1, tasks="helix")
    with pytest.raises(RuntimeError, match="umpcBatchReactive:"):
        m.reactive_rollout(NSUB)
    torch.cuda.synchronize()
    assert _eq(m.state, before) and m.time_ms == 0 and _cursors(m) == (0, 0, 0)
    # ... and inside every table the same handle runs
    m.reactive_steps(2)
    torch.cuda.synchronize()
    assert _cursors(m) == (2, 2, 2) and m.time_ms == pytest.approx(2 * NSUB * DTS) and not _eq(m.state, before)
