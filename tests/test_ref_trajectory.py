"""Reference trajectories: a different (pdes, dpdes, sdes) at every closed-loop step of ONE rollout launch, per robot
(umpcBatchSetRefTrajectory), and per-robot task tables (umpcBatchTaskTable).
CPU: the regenerated lane and quad instruction streams advance their `ref` pointer per step (interpreted, bit for bit
against chained single steps); the new exports and their refusals. GPU: one launch = K launches, the oracle step by step,
the task table against the generators, a task sweep over the batch, the options of the stream, partition invariance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import golden, record_margin
from test_asm_step import _arrays
from test_tasks_weights import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {1: "helix", 2: "straightAcc", 3: "flip", 4: "perch"}
OUTPUTS = ("state", "ctrl", "out", "stats", "status", "info")


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def _slices(n, seed):
    """n different, plausible reference slices [9] (small offsets around hover, unit sdes)"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 9), np.float32)
    r[:, 0:3] = rng.normal(size=(n, 3)) * 2.0
    r[:, 3:6] = rng.normal(size=(n, 3)) * 0.05
    s = np.array([0.0, 0.0, 1.0]) + rng.normal(size=(n, 3)) * 0.1
    r[:, 6:9] = s / np.linalg.norm(s, axis=1, keepdims=True)
    return r


@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_stream_advances_ref_per_step_bit_for_bit(quad):
    """K = 3 with refstep = one slice and three DIFFERENT slices against three chained K = 1 runs of the same stream with
    ref = slice k: every output array equal bit for bit -- so both ref loads of a step (phase A: assembly, phase C:
    extraction / statistics) read the step's own slice and the pointer moves exactly once per step. With refstep = 0 the
    same table reproduces the frozen-reference run (slice 0 for all steps)."""
    from robobee3d_amd import asmstep
    from robobee3d_amd.batch import hover_initial_conditions
    ins = asmstep.StepGen(quad=quad).program()
    fl = asmstep.host_floats()
    st, ref = hover_initial_conditions(1, 20201118, np.float32)
    K = 3
    tab = _slices(K, 5)
    ints = dict(maxIter=50, nsub=25, plant=1)
    one = _arrays(st, ref, 0)
    one["ref"] = tab.ravel().copy()                      # rows 9k .. 9k+8 = slice k
    asmstep.simulate(ins, one, dict(ints, K=K, refstep=9 * asmstep.STRIDE), fl)
    assert np.array_equal(one["ref"], tab.ravel())       # read only
    chained = _arrays(st, ref, 0)
    for k in range(K):
        chained["ref"] = tab[k].copy()
        asmstep.simulate(ins, chained, dict(ints, K=1), fl)
    for key in OUTPUTS:
        assert np.array_equal(one[key], chained[key]), key
    # the slices do differ in effect: the frozen reference (stride 0) gives another trajectory, equal to a plain run on slice 0
    frozen = _arrays(st, ref, 0)
    frozen["ref"] = tab.ravel().copy()
    asmstep.simulate(ins, frozen, dict(ints, K=K, refstep=0), fl)
    plain = _arrays(st, ref, 0)
    plain["ref"] = tab[0].copy()
    asmstep.simulate(ins, plain, dict(ints, K=K), fl)
    for key in OUTPUTS:
        assert np.array_equal(frozen[key], plain[key]), key
    assert not np.array_equal(frozen["state"], one["state"])


def test_ref_pointer_add_carries_into_the_high_word():
    """the 64-bit pointer add of the stream, s_add_u32 / s_addc_u32 on the `ref` pair: interpreted with a low word that wraps
    (the byte offset passes 4 GB over a long launch at a large batch)"""
    from robobee3d_amd import asmstep, isasim
    prog = asmstep.StepGen().program()
    lo, hi = asmstep.S_PTR["ref"], asmstep.S_PTR["ref"] + 1
    add = [t for t in prog if t[0] in ("s_add_u32", "s_addc_u32")]
    assert add == [("s_add_u32", "s%d" % lo, "s%d" % lo, "s%d" % asmstep.S_TMP), ("s_addc_u32", "s%d" % hi, "s%d" % hi, 0)]
    m = isasim.Machine(add, sgpr={lo: 0xFFF00000, hi: 0x7F00, asmstep.S_TMP: 9 * 65536 * 4})
    isasim.run(m)
    assert m.S[lo] | (m.S[hi] << 32) == 0x7F00FFF00000 + 9 * 65536 * 4 and m.S[hi] == 0x7F01
    assert asmstep.OFF["refstep"] == asmstep.PARAM_BYTES - 4 and asmstep.OFF["mbg"] == asmstep.PARAM_BYTES - 8   # appended: older offsets stay


def test_new_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int umpcBatchSetRefTrajectory(umpc_batch_t *h, const void *tab, long long steps, long long cursor0);",
                 "long long umpcBatchRefCursor(const umpc_batch_t *h);",
                 "int umpcBatchTaskTable(umpc_batch_t *h, long long steps, double t_ms, const int32_t *task, const void *params, "
                 "const void *ref, void *tab, void *stream);"):
        assert decl in flat, decl
    L = _lib.lib()
    for sym in ("umpcBatchSetRefTrajectory", "umpcBatchRefCursor", "umpcBatchTaskTable"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchRefCursor.restype is C.c_longlong
    assert L.umpcBatchSetRefTrajectory.argtypes == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchSetRefTrajectory(None, None, 0, 0) == -1 and b"umpcBatchSetRefTrajectory" in L.umpcLastError()
    assert L.umpcBatchTaskTable(None, 1, 0.0, None, None, None, None, None) == -1 and b"umpcBatchTaskTable" in L.umpcLastError()
    assert L.umpcBatchRefCursor(None) == 0
    # the stale scope sentence is gone from the header
    assert "no task generator, batch-constant weights, no WL coupling" not in flat.replace("* ", "")


def test_resource_limits_cover_the_new_kernel_and_keep_the_old_ones():
    import json
    lim = json.load(open(os.path.join(ROOT, "robobee3d_amd", "csrc", "resource_limits.json")))
    assert lim["umpc_task_table_kernel"]["ScratchSize"] == 0
    assert lim["umpc_rollout_kernelIdLb1ELb1ELb1E"]["ScratchSize"] == 600 and lim["umpc_rollout_kernelIdLb1ELb1E"]["ScratchSize"] == 950
    assert lim["umpc_rollout_kernelIfLb0E"]["ScratchSize"] == 1376
    for k in ("umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel", "umpc_dropin_quad_kernel"):
        assert lim[k]["ScratchSize"] == 0 and lim[k]["VGPRs"] == 256 and lim[k]["AGPRs"] == 256


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
MODES = [("f32-lane", "float32", "lane"), ("f32-quad", "float32", "quad"), ("f32-cpp", "float32", "cpp"), ("f64", "float64", "auto")]
MODE_IDS = [m[0] for m in MODES]


def _handle(B, dtype, mode, **kw):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    m = BatchUprightMPC(B, getattr(torch, dtype), **kw)
    m.set_step_kernel(mode)
    return m


def _smooth_table(B, steps, seed, p0=None, dt_ms=5.0):
    """random smooth per-robot path [steps, 9, B] (fp64): pdes = p0 + A sin(w t + phi) per axis, dpdes its derivative
    (mm/ms), sdes a slowly tilting unit vector"""
    rng = np.random.default_rng(seed)
    t = (np.arange(steps) * dt_ms)[:, None, None]
    A = rng.uniform(1.0, 6.0, size=(1, 3, B))
    w = rng.uniform(0.002, 0.02, size=(1, 3, B))
    ph = rng.uniform(0, 2 * np.pi, size=(1, 3, B))
    p0 = np.zeros((3, B)) if p0 is None else p0
    tab = np.zeros((steps, 9, B))
    tab[:, 0:3] = p0[None] + A * (np.sin(w * t + ph) - np.sin(ph))
    tab[:, 3:6] = A * w * np.cos(w * t + ph)
    tilt = 0.15 * np.sin(rng.uniform(0.002, 0.01, size=(1, 2, B)) * t + rng.uniform(0, 2 * np.pi, size=(1, 2, B)))
    s = np.concatenate((tilt, np.ones((steps, 1, B))), axis=1)
    tab[:, 6:9] = s / np.linalg.norm(s, axis=1, keepdims=True)
    return tab


def _equal(a, b, what=""):
    import torch
    for k in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


def _np_dtype(dtype):
    return np.float32 if dtype == "float32" else np.float64


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode", MODES, ids=MODE_IDS)
def test_table_of_equal_slices_is_the_frozen_reference(name, dtype, mode):
    """identity: a table whose slices all equal `ref`, K = 8, against the plain rollout(8) of a second handle"""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    B, K = 128, 8
    st, ref = hover_initial_conditions(B, 20201118, _np_dtype(dtype))
    ref[0:3] = np.random.default_rng(1).normal(size=(3, B))
    a, b = _handle(B, dtype, mode), _handle(B, dtype, mode)
    a.set_state(st, ref)
    b.set_state(st, ref)
    a.set_reference_trajectory(torch.as_tensor(ref)[None].repeat(K, 1, 1))
    a.ref.fill_(float("nan"))                      # not read while a table is set
    a.rollout(K)
    b.rollout(K)
    assert a.kernel_name == b.kernel_name and a.ref_cursor == K
    _equal(a, b, name)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [128, 100])
@pytest.mark.parametrize("name,dtype,mode", MODES, ids=MODE_IDS)
def test_one_launch_equals_k_launches(name, dtype, mode, B):
    """rollout(8) with a random smooth per-robot table == eight rollout(1) of a second handle whose `ref` is overwritten with
    slice k each time; also split as rollout(3) + rollout(5) (the cursor carries over) and with a non-zero cursor0"""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    K = 8
    st, ref = hover_initial_conditions(B, 7, _np_dtype(dtype), tilt=0.3)
    tab = torch.as_tensor(_smooth_table(B, K, 3).astype(_np_dtype(dtype))).cuda()
    one, many, split, off = (_handle(B, dtype, mode) for _ in range(4))
    for h in (one, many, split, off):
        h.set_state(st, ref)
    one.set_reference_trajectory(tab)
    one.rollout(K)
    for k in range(K):
        many.ref.copy_(tab[k])
        many.rollout(1)
    assert one.kernel_name == many.kernel_name
    _equal(one, many, name)
    assert one.time_ms == many.time_ms
    split.set_reference_trajectory(tab)
    split.rollout(3)
    assert split.ref_cursor == 3
    split.rollout(5)
    assert split.ref_cursor == 8
    _equal(split, many, name + " 3+5")
    junk = torch.full((2, 9, B), 1e3, dtype=tab.dtype, device=tab.device)
    off.set_reference_trajectory(torch.cat((junk, tab)), cursor=2)
    off.rollout(K)
    assert off.ref_cursor == 10
    _equal(off, many, name + " cursor0")
    assert not torch.equal(one.state[0:3], torch.as_tensor(st[0:3]).cuda())


def _oracle_steps(oracle_built, perm, st, tab, dtype, **kw):
    """the table through the oracle, one call per step (it carries state / ctrl in place); returns state, out of the last step"""
    B = st.shape[1]
    s = st.astype(dtype).copy()
    c = np.zeros((127, B), dtype)
    c[124:] = 1
    out = None
    for k in range(tab.shape[0]):
        out, _, _ = oracle_built.batch_rollout(s, c, np.ascontiguousarray(tab[k].astype(dtype)), 1, dtype=dtype, perm=perm, **kw)
    return s, out


def _check_against_oracle(label, m, s_o, out_o, s_o32):
    """fp64: the margins tests/test_tasks_weights.py asserts for this loop; fp32: its self-calibrating band (at most 4x the
    distance of the fp32 CPU oracle from the fp64 one, floors 2e-3 mm / 3e-4)"""
    import torch
    s = m.state.cpu().numpy().astype(np.float64)
    if m.dtype == torch.float64:
        out = m.out.cpu().numpy()
        record_margin(label, "max |d state| / (1e-9 + 1e-7 |s|)", (np.abs(s - s_o) / (1e-9 + 1e-7 * np.abs(s_o))).max(), 1.0)
        record_margin(label, "max |d out| / (1e-8 + 1e-6 |o|)", (np.abs(out - out_o) / (1e-8 + 1e-6 * np.abs(out_o))).max(), 1.0)
        np.testing.assert_allclose(s, s_o, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(out, out_o, rtol=1e-6, atol=1e-8)
        return
    band_p = max(2e-3, 4 * np.abs(s_o32[0:3].astype(np.float64) - s_o[0:3]).max())
    band_r = max(3e-4, 4 * np.abs(s_o32[3:].astype(np.float64) - s_o[3:]).max())
    dp, dr = np.abs(s[0:3] - s_o[0:3]).max(), np.abs(s[3:] - s_o[3:]).max()
    record_margin(label, "|dp| mm vs fp64 oracle", dp, band_p)
    record_margin(label, "|dR|,|ddq| vs fp64 oracle", dr, band_r)
    assert dp <= band_p and dr <= band_r, (label, dp, band_p, dr, band_r)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode", MODES, ids=MODE_IDS)
def test_table_rollout_matches_the_oracle_step_by_step(oracle_built, name, dtype, mode):
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import hover_initial_conditions
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    B, K = 128, 8
    st, _ = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    tab = _smooth_table(B, K, 17)
    s_o, out_o = _oracle_steps(oracle_built, perm, st, tab, np.float64)
    s_o32, _ = _oracle_steps(oracle_built, perm, st, tab, np.float32)
    m = _handle(B, dtype, mode)
    m.set_state(st.astype(_np_dtype(dtype)), tab[0].astype(_np_dtype(dtype)))
    m.set_reference_trajectory(tab.astype(_np_dtype(dtype)))
    m.rollout(K)
    _check_against_oracle("reference trajectory K=8 " + name, m, s_o, out_o, s_o32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[2] for c in CASES])
def test_task_table_is_the_generators(case):
    """task_table with batch-constant parameters at the fixture's times (0, 25, ... 1200 ms = every fifth fire time of a 241-step
    table from t = 0; 25 * 0.2 rounds to exactly 5 in fp32 and fp64, so the fire times are exact): fp64 against the vectors
    the reference's flight_tasks.py produced, at the 1e-13 the oracle's own test uses, and -- fp64 and fp32 -- bit-equal to
    task_reference(t) of a handle with set_task (the same device function)."""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    task, tp, key = case
    g = golden("flight_tasks.npz")
    kw = dict(zip(BatchUprightMPC.TASKS[NAMES[task]][1], tp))
    B = 70
    assert np.array_equal(g["t"], 25.0 * np.arange(49))
    for dtype in (torch.float64, torch.float32):
        m = BatchUprightMPC(B, dtype)
        m.ref[0:3] = torch.as_tensor(g["p0"], dtype=dtype, device=m.device)[:, None]
        tab = m.task_table(241, NAMES[task], t_ms=0.0, **kw)
        assert tab.shape == (241, 9, B) and bool((tab == tab[:, :, :1]).all())
        if dtype == torch.float64:
            got = tab[::5, :, 0].cpu().numpy()
            d = np.abs(got - g[key]) / (1e-13 + 1e-13 * np.abs(g[key]))
            record_margin("task_table fp64 vs flight_tasks.py: " + key, "max |d| / (1e-13 + 1e-13 |r|)", d.max(), 1.0)
            np.testing.assert_allclose(got, g[key], rtol=1e-13, atol=1e-13)
        h = BatchUprightMPC(B, dtype)
        h.ref.copy_(m.ref)
        h.set_task(NAMES[task], t_ms=0.0, **kw)
        for k in (0, 1, 7, 100, 240):
            assert torch.equal(tab[k], h.task_reference(5.0 * k)), (key, dtype, k)
        # the handle's own task and parameters (NULL, NULL) give the same table
        assert torch.equal(h.task_table(241, t_ms=0.0), tab)


def _sweep_setup(B=128):
    rng = np.random.default_rng(5)
    names = np.repeat(["helix", "straightAcc", "flip", "perch"], B // 4)
    by = {c[2]: c for c in CASES}
    vdes = np.where(names == "straightAcc", 2.0, 0.2)
    tend = np.where(names == "flip", 200.0, 500.0)
    kw = dict(trajAmp=80.0, trajFreq=1.0, dz=0.15, useY=True, tduration=500.0, vdes=vdes, tstart=100.0, tend=tend,
              trotstart=100.0, trotend=450.0)
    p0 = rng.normal(size=(3, B))
    return names, by, kw, p0


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode", MODES, ids=MODE_IDS)
def test_task_sweep_over_the_batch_matches_the_oracle(oracle_built, name, dtype, mode):
    """B = 128 in four groups of 32 robots -- helix / straightAcc / flip / perch with the CASES parameters, per-robot initialPos --
    as task_table + set_reference_trajectory + rollout(8), against four oracle runs on the column groups"""
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import hover_initial_conditions
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    B, K, t0 = 128, 8, 35.0
    names, by, kw, p0 = _sweep_setup(B)
    st, ref = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    ref[:] = 0
    ref[0:3] = p0
    st[0:3] = p0
    s_o, s_o32, out_o = st.copy(), st.astype(np.float32), np.zeros((9, B))
    for gi, nm in enumerate(["helix", "straightAcc", "flip", "perch"]):
        sl = slice(32 * gi, 32 * gi + 32)
        task, tp, _ = by[nm]
        for dt_, dst in ((np.float64, s_o), (np.float32, s_o32)):
            s = np.ascontiguousarray(st[:, sl].astype(dt_))
            c = np.zeros((127, 32), dt_); c[124:] = 1
            o, _, _ = oracle_built.batch_rollout(s, c, np.ascontiguousarray(ref[:, sl].astype(dt_)), K, dtype=dt_, perm=perm,
                                                 task=task, task_p=tp, t0=t0)
            dst[:, sl] = s
            if dt_ == np.float64:
                out_o[:, sl] = o
    m = _handle(B, dtype, mode)
    m.set_state(st.astype(_np_dtype(dtype)), ref.astype(_np_dtype(dtype)))
    tab = m.task_table(K, list(names), t_ms=t0, **kw)
    m.set_reference_trajectory(tab)
    m.rollout(K)
    _check_against_oracle("task sweep 4 x 32 K=8 " + name, m, s_o, out_o, s_o32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[1:], ids=[c[2] for c in CASES[1:]])
@pytest.mark.parametrize("name,dtype,mode", MODES, ids=MODE_IDS)
def test_one_task_through_a_table_against_set_task(oracle_built, name, dtype, mode, case):
    """ONE task for all robots: the table route against a handle using set_task. fp64 and fp32 "cpp" evaluate the same device
    function at the same times in the same type: bit-equal. The fp32 assembly forms add a float table entry to initialPos
    inside the stream on the set_task route (equal only up to rounding): both are held to the fp64 oracle's band instead."""
    import torch
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    task, tp, key = case
    kw = dict(zip(BatchUprightMPC.TASKS[NAMES[task]][1], tp))
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    B, K, t0 = 128, 8, 35.0
    st, ref = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    ref[:] = 0
    ref[0:3] = np.random.default_rng(5).normal(size=(3, B))
    st[0:3] = ref[0:3]
    nd = _np_dtype(dtype)
    a, b = _handle(B, dtype, mode), _handle(B, dtype, mode)
    for h in (a, b):
        h.set_state(st.astype(nd), ref.astype(nd))
    a.set_reference_trajectory(a.task_table(K, NAMES[task], t_ms=t0, **kw))
    b.set_task(NAMES[task], t_ms=t0, **kw)
    a.rollout(K)
    b.rollout(K)
    if mode in ("cpp", "auto"):
        _equal(a, b, name + " " + key)
        return
    assert a.kernel_name == b.kernel_name and a.kernel_name.startswith("umpc_rollout_asm")
    s_o, s_o32 = st.copy(), st.astype(np.float32)
    c = np.zeros((127, B)); c[124:] = 1
    out_o, _, _ = oracle_built.batch_rollout(s_o, c, ref, K, dtype=np.float64, perm=perm, task=task, task_p=tp, t0=t0)
    c32 = np.zeros((127, B), np.float32); c32[124:] = 1
    oracle_built.batch_rollout(s_o32, c32, ref.astype(np.float32), K, dtype=np.float32, perm=perm, task=task, task_p=tp, t0=t0)
    _check_against_oracle("one task via table K=8 %s %s" % (name, key), a, s_o, out_o, s_o32)
    _check_against_oracle("one task via set_task K=8 %s %s" % (name, key), b, s_o, out_o, s_o32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "lane", "quad"])
def test_options_still_combine_with_a_table(mode):
    """table + per-robot weights + fused WL + per-robot Ib / gain in one fp32 launch == K single-step launches"""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, BatchWLCon, hover_initial_conditions, monte_carlo_draws
    from test_wl_step import _args
    g = golden("mpc_wl_loop.npz")
    B, K = 128, 6
    st, ref = hover_initial_conditions(B, 3, np.float32, tilt=0.3)
    tab = torch.as_tensor(_smooth_table(B, K, 23).astype(np.float32)).cuda()
    rng = np.random.default_rng(2)
    W = np.tile(np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])[:, None], (1, B)) * rng.uniform(0.5, 2.0, size=(8, B))
    Ib, gain = monte_carlo_draws(B, 9, np.float32)
    hs = []
    for _ in range(2):
        m = BatchUprightMPC(B, torch.float32)
        m.set_step_kernel(mode)
        m.set_state(st, ref)
        m.set_weights(W.astype(np.float32))
        m.Ib, m.gain = torch.as_tensor(Ib).cuda(), torch.as_tensor(gain).cuda()
        wl = BatchWLCon(B, *_args(g), dtype=torch.float32)
        m.set_wl(wl)
        hs.append((m, wl))
    (a, wa), (b, wb) = hs
    a.set_reference_trajectory(tab)
    a.rollout(K)
    assert a.kernel_name in ("umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel")
    for k in range(K):
        b.ref.copy_(tab[k])
        b.rollout(1)
    assert a.kernel_name == b.kernel_name
    _equal(a, b, mode)
    assert torch.equal(wa.u, wb.u) and torch.equal(wa.w0, wb.w0)


@pytest.mark.gpu
def test_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B = 64
    st, ref = hover_initial_conditions(B, 1, np.float32)
    m = BatchUprightMPC(B, torch.float32)
    m.set_state(st, ref)
    tab = torch.as_tensor(ref)[None].repeat(4, 1, 1)
    m.set_reference_trajectory(tab, cursor=1)
    before = m.state.clone()
    with pytest.raises(RuntimeError, match="reference trajectory ends"):
        m.rollout(4)                                    # 1 + 4 > 4: refused before anything is launched
    torch.cuda.synchronize()
    assert torch.equal(m.state, before) and m.ref_cursor == 1 and m.time_ms == 0.0
    m.rollout(3)
    assert m.ref_cursor == 4
    with pytest.raises(RuntimeError):
        m.update()                                      # slice 4 does not exist
    with pytest.raises(RuntimeError, match="umpcBatchSetTask"):
        m.set_task("helix")
    with pytest.raises(RuntimeError, match="umpcBatchReactive"):
        m.reactive_rollout(1)
    with pytest.raises(RuntimeError, match="umpcBatchTaskReference"):
        m.task_reference(0.0)
    with pytest.raises(ValueError):
        m.set_reference_trajectory(torch.zeros((4, 9, B + 1)))
    with pytest.raises(RuntimeError):
        m.set_reference_trajectory(tab, cursor=5)
    m.set_reference_trajectory(tab, cursor=2)
    m.update()                                          # reads slice 2, does not advance
    assert m.ref_cursor == 2
    m.set_reference_trajectory(None)
    m.set_task("helix")
    with pytest.raises(RuntimeError, match="umpcBatchSetRefTrajectory"):
        m.set_reference_trajectory(tab)
    m.set_task("ref")
    m.set_reference_trajectory(tab)
    with pytest.raises(TypeError):
        m.task_table(2, "helix", amplitude=3)


@pytest.mark.gpu
def test_blocks_with_column_sliced_tables_equal_the_undivided_run():
    """partition invariance: 16 384 robots whole (fp32: quad form) and as 2 blocks of 8 192 with global_batch = 16 384; 32 768
    robots (above the quad threshold: lane form) whole and as 4 blocks of 8 192 -- every block on the column slice of the
    job's table (shard.table_block)"""
    import torch
    from robobee3d_amd import shard
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions_device
    K = 4
    for B, W, kernel in ((16384, 2, "umpc_rollout_asm_quad_kernel"), (32768, 4, "umpc_rollout_asm_kernel")):
        whole = BatchUprightMPC(B, torch.float32, plant_mode=1)
        st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
        whole.set_state(st, ref)
        whole.ref[0:3] = 0.01 * torch.arange(B, device="cuda", dtype=torch.float32)[None] % 3.0
        tab = whole.task_table(K, ["helix", "perch"] * (B // 2), t_ms=10.0, trajFreq=torch.linspace(0.5, 2.0, B).numpy())
        whole.set_reference_trajectory(tab)
        whole.rollout(K)
        assert whole.kernel_name == kernel
        for rank in range(W):
            lo, hi = shard.split_range(B, rank, W)
            blk = BatchUprightMPC(hi - lo, torch.float32, plant_mode=1, global_batch=B)
            blk.set_state(st[:, lo:hi], ref[:, lo:hi])
            blk.set_reference_trajectory(shard.table_block(tab, lo, hi))
            blk.rollout(K)
            assert blk.kernel_name == kernel
            for a, b in ((blk.state, whole.state), (blk.ctrl, whole.ctrl), (blk.out, whole.out), (blk.stats, whole.stats),
                         (blk.info, whole.info)):
                assert torch.equal(a, b[:, lo:hi])
            assert torch.equal(blk.status, whole.status[lo:hi])
