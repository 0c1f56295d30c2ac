"""Step history: the state before / after and the command, status and residuals of EVERY closed-loop step of one rollout
launch, for the whole batch (umpcBatchSetHistory): each step's own stores land one slice further on.
CPU: the regenerated lane and quad streams interpreted with the strides set, bit for bit against chained single steps, guard
words, the 64-bit advances with a wrapping low word, the layout of the second parameter block, exports and refusals.
GPU: one launch = K launches in every step-kernel form, the options of the stream, the oracle step by step, refusals,
partition invariance, the log against control_test_log."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from conftest import golden
from test_asm_step import _arrays
from test_ref_trajectory import (MODES, MODE_IDS, OUTPUTS, _check_against_oracle, _handle, _np_dtype, _oracle_steps, _slices,
                                 _smooth_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 3                      # guard rows behind every table
ROWS = {"state": 18, "out": 9, "status": 1, "info": 2}
GUARD_F, GUARD_I = np.float32(-12345.5), np.int32(-77)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def _tables(base, K):
    """the arrays of one interpreted run with room for K slices (K + 1 of state) and GUARD rows of guard words behind them;
    slice 0 of state is the initial state"""
    a = {n: None if x is None else x.copy() for n, x in base.items()}
    for n, rows in ROWS.items():
        nsl = K + 1 if n == "state" else K
        t = np.full(rows * nsl + GUARD, GUARD_I if n == "status" else GUARD_F, base[n].dtype)
        if n == "state":
            t[:rows] = base[n]
        a[n] = t
    return a


def _strides():
    from robobee3d_amd import asmstep
    return dict(statestep=18 * asmstep.STRIDE, outstep=9 * asmstep.STRIDE, statusstep=asmstep.STRIDE, infostep=2 * asmstep.STRIDE)


@pytest.mark.parametrize("with_ref", [False, True], ids=["frozen-ref", "ref-table"])
@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_stream_writes_one_slice_per_step_bit_for_bit(quad, with_ref):
    """K = 3 with the four strides set (and, ref-table, `refstep` too: all five pointers move in one stream) against three
    chained K = 1 runs: slice k + 1 of state and slice k of out / status / info are what the chain leaves after step k, ctrl
    and stats are equal, slice 0 of state is only read, the guard words behind every table are untouched. With all strides 0
    the same stream equals a plain run in every array."""
    from robobee3d_amd import asmstep
    from robobee3d_amd.batch import hover_initial_conditions
    ins = asmstep.StepGen(quad=quad).program()
    fl = asmstep.host_floats()
    st, ref = hover_initial_conditions(1, 20201118, np.float32, tilt=0.3)
    K = 3
    tab = _slices(K, 5)
    ints = dict(maxIter=50, nsub=25, plant=1)
    base = _arrays(st, ref, 0)
    one = _tables(base, K)
    if with_ref:
        one["ref"] = tab.ravel().copy()
    asmstep.simulate(ins, one, dict(ints, K=K, refstep=9 * asmstep.STRIDE if with_ref else 0, **_strides()), fl)
    chained = _arrays(st, ref, 0)
    assert np.array_equal(one["state"][:18], chained["state"])                  # slice 0: read, never written
    for k in range(K):
        if with_ref:
            chained["ref"] = tab[k].copy()
        asmstep.simulate(ins, chained, dict(ints, K=1), fl)
        for n, rows in ROWS.items():
            sl = k + 1 if n == "state" else k
            assert np.array_equal(one[n][rows * sl:rows * (sl + 1)].view(np.uint32), chained[n].view(np.uint32)), (n, k)
    for n in ("ctrl", "stats"):
        assert np.array_equal(one[n].view(np.uint32), chained[n].view(np.uint32)), n
    for n in ROWS:
        assert np.all(one[n][-GUARD:] == (GUARD_I if n == "status" else GUARD_F)), n
    assert not np.array_equal(one["state"][18:36], one["state"][36:54])         # the steps do differ
    # all strides 0: a plain run, also on the large arrays (nothing beyond slice 0 is touched)
    zero = _tables(base, K)
    plain = _arrays(st, ref, 0)
    if with_ref:
        zero["ref"] = tab[0].copy()
        plain["ref"] = tab[0].copy()
    asmstep.simulate(ins, zero, dict(ints, K=K, **{n: 0 for n in asmstep.HIST_INTS}), fl)
    asmstep.simulate(ins, plain, dict(ints, K=K), fl)
    for n in OUTPUTS:
        rows = len(plain[n])
        assert np.array_equal(zero[n][:rows].view(np.uint32), plain[n].view(np.uint32)), n
    for n, rows in ROWS.items():
        assert np.all(zero[n][rows:] == (GUARD_I if n == "status" else GUARD_F)), n


@pytest.mark.parametrize("ptr", ["state", "out", "status", "info"])
@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_history_pointer_adds_carry_into_the_high_word(quad, ptr):
    """the 64-bit advance of every moved pointer, extracted from the program (the four scalar instructions from the s_add_i32
    on the pointer's low word) and interpreted with a low word that wraps: the high word is incremented exactly once (the
    state offset passes 4 GB after 455 steps at B = 65 536); without a wrap it stays. Each pointer is advanced exactly once
    per step, and by no s_add_u32 / s_addc_u32: those stay the `ref` pair alone."""
    from robobee3d_amd import asmstep, isasim
    prog = asmstep.StepGen(quad=quad).program()
    lo, hi = asmstep.S_PTR[ptr], asmstep.S_PTR[ptr] + 1
    at = [k for k, t in enumerate(prog) if t[0] == "s_add_i32" and t[1] == "s%d" % lo]
    assert len(at) == 1
    seq = prog[at[0]:at[0] + 4]
    assert [t[0] for t in seq] == ["s_add_i32", "s_cmp_lt_u32", "s_cselect_b32", "s_add_i32"] and seq[3][1] == "s%d" % hi
    sstep = int(seq[0][3][1:])
    step = 18 * 65536 * 4
    m = isasim.Machine(seq, sgpr={lo: 0xFFF00000, hi: 0x7F00, sstep: step})
    isasim.run(m)
    assert m.S[lo] | (m.S[hi] << 32) == 0x7F00FFF00000 + step and m.S[hi] == 0x7F01
    m = isasim.Machine(seq, sgpr={lo: 0x80000000, hi: 0x7F00, sstep: step})
    isasim.run(m)
    assert (m.S[lo], m.S[hi]) == (0x80000000 + step, 0x7F00)
    m = isasim.Machine(seq, sgpr={lo: 0xFFFFFFFF, hi: 0x7F00, sstep: 0})              # stride 0 never carries
    isasim.run(m)
    assert (m.S[lo], m.S[hi]) == (0xFFFFFFFF, 0x7F00)
    # the word is read from the second block, once per step, by a scalar load just ahead
    loads = [t for t in prog[:at[0]] if t[0].startswith("s_load_dword") and t[2] == "s[%d:%d]" % (asmstep.S_PBLK, asmstep.S_PBLK + 1)]
    last = loads[-1]
    first = int(re.match(r"s\[?(\d+)", last[1]).group(1))
    assert last[3] + 4 * (sstep - first) == asmstep.OFF[ptr + "step"]
    add = [t for t in prog if t[0] in ("s_add_u32", "s_addc_u32")]
    assert [t[1] for t in add] == ["s%d" % asmstep.S_PTR["ref"], "s%d" % (asmstep.S_PTR["ref"] + 1)]


def test_the_advances_add_no_vector_or_memory_instruction():
    """per step the history costs two scalar loads of the second block and SALU instructions, nothing else: the words of a
    moved pointer are named by scalar instructions and by the loads / stores through it, which were there before"""
    from robobee3d_amd import asmstep
    for quad in (False, True):
        prog = asmstep.StepGen(quad=quad).program()
        new = [t for t in prog if t[0] in ("s_cmp_lt_u32", "s_cselect_b32")]
        assert len(new) == 8
        hist = [t for t in prog if t[0].startswith("s_load") and isinstance(t[3], int) and t[3] >= asmstep.HIST_OFF]
        assert [t[0] for t in hist] == ["s_load_dword", "s_load_dwordx4"]
        # nothing but scalar instructions names a moved pointer's words apart from the loads / stores through it
        for ptr in ROWS:
            lo = asmstep.S_PTR[ptr]
            for t in prog:
                if "s%d" % lo in t[1:] or "s%d" % (lo + 1) in t[1:]:
                    assert t[0].startswith("s_"), t
        vmem = [t for t in prog if t[0].startswith("global_") and "s[%d:%d]" % (asmstep.S_PTR["state"], asmstep.S_PTR["state"] + 1) in t]
        assert len(vmem) == 2 * 18 + 18                     # two loads and one store of the 18 state rows, as before


def test_second_block_layout_and_old_offsets():
    """PARAM_BYTES and every older offset are what they were; the new block starts at the padded size of StepParams, which is
    what the generated header asserts; simulate() packs both blocks"""
    from robobee3d_amd import asmstep
    assert asmstep.PARAM_BYTES == 292 and asmstep.HIST_OFF == 296 and asmstep.HIST_BYTES == 16
    assert asmstep.OFF["refstep"] == 288 and asmstep.OFF["mbg"] == 284 and asmstep.OFF["state"] == 0 and asmstep.OFF["done"] == 128
    assert asmstep.OFF["stride"] == 136 and asmstep.OFF["seq"] == 156 and asmstep.OFF["dt"] == 160
    assert [asmstep.OFF[n] for n in asmstep.HIST_INTS] == [296, 300, 304, 308]
    assert asmstep.HIST_INTS == ["statestep", "outstep", "statusstep", "infostep"]
    hdr = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_step_asm.h")).read()
    assert "static_assert(sizeof(StepParams) == 296, \"StepParams layout\");" in hdr
    assert "static_assert(offsetof(StepArgs, h) == 296 && sizeof(StepHist) == 16, \"StepHist layout\");" in hdr
    src = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_mi355x.hip")).read()
    for k in ("umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel", "umpc_dropin_quad_kernel"):
        assert re.search(r"void %s\(const umpcasm::StepArgs prm\b" % k, src), k


def test_new_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int umpcBatchSetHistory(umpc_batch_t *h, void *state_hist, void *out_hist, int32_t *status_hist, "
                 "void *info_hist, long long steps, long long cursor0);",
                 "long long umpcBatchHistoryCursor(const umpc_batch_t *h);"):
        assert decl in flat, decl
    L = _lib.lib()
    for sym in ("umpcBatchSetHistory", "umpcBatchHistoryCursor"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchHistoryCursor.restype is C.c_longlong
    assert L.umpcBatchSetHistory.argtypes == [C.c_void_p] * 5 + [C.c_longlong, C.c_longlong]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchSetHistory(None, None, None, None, None, 4, 0) == -1 and b"umpcBatchSetHistory" in L.umpcLastError()
    assert L.umpcBatchHistoryCursor(None) == 0


def test_resource_limits_are_unchanged():
    """csrc/resource_limits.json holds the parent's figures for the seven kernels of the step path: no frame, register or LDS
    limit moved (build() checks the compiled kernels against it). Every other entry -- the kernels that came after them, and
    whichever come next -- allows no scratch frame at all."""
    lim = json.load(open(os.path.join(ROOT, "robobee3d_amd", "csrc", "resource_limits.json")))
    got = {k: {f: x for f, x in v.items() if f != "_note"} for k, v in lim.items()}
    full = lambda lds, scratch: {"VGPRs": 256, "AGPRs": 256, "LDS": lds, "ScratchSize": scratch}
    step = {"umpc_dropin_quad_kernel": full(40960, 0), "umpc_rollout_kernelIfLb0E": full(40960, 1376),
            "umpc_rollout_asm_kernel": full(40960, 0), "umpc_rollout_kernelIdLb1ELb1E": full(163840, 950),
            "umpc_rollout_asm_quad_kernel": full(40960, 0), "umpc_rollout_kernelIdLb1ELb1ELb1E": full(163840, 600),
            "umpc_task_table_kernel": {"ScratchSize": 0}}
    assert {k: got[k] for k in step} == step
    for k in set(got) - set(step):
        assert got[k].get("ScratchSize") == 0 and set(got[k]) <= {"VGPRs", "AGPRs", "LDS", "ScratchSize"}, (k, got[k])


def test_history_block_is_a_column_slice():
    import torch
    from robobee3d_amd import shard
    hist = {"state": torch.arange(5 * 18 * 6).reshape(5, 18, 6), "status": torch.arange(4 * 6).reshape(4, 6), "out": None, "info": None}
    blk = shard.history_block(hist, 2, 5)
    assert blk["out"] is None and blk["info"] is None and blk["state"].is_contiguous()
    assert torch.equal(blk["state"], hist["state"][:, :, 2:5]) and torch.equal(blk["status"], hist["status"][:, 2:5])


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
RECORDS = ("state", "out", "status", "info")
# the modes of tests/test_ref_trajectory.py, plus the two fp64 forms that advance their pointers IN the kernel ("auto" takes
# the fp64 quad form at these batch sizes, whose steps the library issues one per launch)
HIST_MODES = MODES + [("f64-lane", "float64", "lane"), ("f64-cpp", "float64", "cpp")]
HIST_MODE_IDS = [m[0] for m in HIST_MODES]
KERNEL = {"f32-lane": "umpc_rollout_asm_kernel", "f32-quad": "umpc_rollout_asm_quad_kernel", "f32-cpp": "umpc_rollout_kernel<float>",
          "f64": "umpc_rollout_kernel<double, LDSF, ASM64, QUAD>", "f64-lane": "umpc_rollout_kernel<double, LDSF, ASM64>",
          "f64-cpp": "umpc_rollout_kernel<double, LDSF>"}


def _hist_equal(hist, k, m, what=""):
    """slice k + 1 of state and slice k of the other records against the arrays of handle m after its step k"""
    import torch
    for n in RECORDS:
        assert torch.equal(hist[n][k + 1 if n == "state" else k], getattr(m, n)), (what, n, k)


def _final_equal(a, b, what=""):
    import torch
    for k in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [128, 100])
@pytest.mark.parametrize("name,dtype,mode", HIST_MODES, ids=HIST_MODE_IDS)
def test_history_of_one_launch_equals_k_launches(name, dtype, mode, B):
    """rollout(8) with all four records on == what a second handle holds after each of eight rollout(1); the final arrays
    equal a history-free rollout(8) of a third handle; rollout(3) + rollout(5) continue one table"""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    K = 8
    st, ref = hover_initial_conditions(B, 7, _np_dtype(dtype), tilt=0.3)
    ref[0:3] = np.random.default_rng(1).normal(size=(3, B))
    one, many, plain, split = (_handle(B, dtype, mode) for _ in range(4))
    for h in (one, many, plain, split):
        h.set_state(st, ref)
    one.record_history(K, status=True, info=True)
    assert one.history_cursor == 0 and one.history()["state"].shape == (1, 18, B) and one.history()["out"].shape == (0, 9, B)
    one.rollout(K)
    assert one.history_cursor == K
    hist = one.history()
    assert hist["state"].shape == (K + 1, 18, B) and hist["out"].shape == (K, 9, B) and hist["status"].shape == (K, B) and \
        hist["info"].shape == (K, 2, B)
    assert torch.equal(hist["state"][0], torch.as_tensor(st).cuda())
    for k in range(K):
        many.rollout(1)
        _hist_equal(hist, k, many, name)
    assert one.kernel_name == many.kernel_name == KERNEL[name]
    plain.rollout(K)
    assert plain.kernel_name == one.kernel_name
    _final_equal(one, plain, name)
    assert one.time_ms == plain.time_ms
    assert not torch.equal(hist["state"][1], hist["state"][2]) and not torch.equal(hist["out"][0], hist["out"][1])
    split.record_history(K, status=True, info=True)
    split.rollout(3)
    assert split.history_cursor == 3 and split.history()["state"].shape[0] == 4
    split.rollout(5)
    assert split.history_cursor == 8
    hs = split.history()
    for n in RECORDS:
        assert torch.equal(hs[n], hist[n]), (name, "3+5", n)
    _final_equal(split, plain, name + " 3+5")
    # a record that is off leaves the others what they are; history off again = the plain run
    part = _handle(B, dtype, mode)
    part.set_state(st, ref)
    part.record_history(K, state=False, out=True, status=True)
    part.rollout(K)
    hp = part.history()
    assert hp["state"] is None and hp["info"] is None and torch.equal(hp["out"], hist["out"]) and torch.equal(hp["status"], hist["status"])
    _final_equal(part, plain, name + " out+status only")
    part.record_history(None)
    plain.rollout(2)
    part.rollout(2)
    _final_equal(part, plain, name + " off again")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "lane", "quad"])
def test_history_combines_with_the_options_of_the_stream(mode):
    """history + reference trajectory + per-robot weights + fused WL + per-robot Ib / gain in one fp32 launch == K
    single-step launches"""
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
    a.record_history(K, status=True, info=True)
    a.rollout(K)
    assert a.kernel_name in ("umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel")
    hist = a.history()
    for k in range(K):
        b.ref.copy_(tab[k])
        b.rollout(1)
        _hist_equal(hist, k, b, mode)
    assert a.kernel_name == b.kernel_name and a.ref_cursor == K and a.history_cursor == K
    _final_equal(a, b, mode)
    assert torch.equal(wa.u, wb.u) and torch.equal(wa.w0, wb.w0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode", [MODES[0], MODES[3]], ids=[MODE_IDS[0], MODE_IDS[3]])
def test_history_matches_the_oracle_step_by_step(oracle_built, name, dtype, mode):
    """every recorded step -- state slice k + 1, out slice k -- against the oracle stepped k + 1 times along the same
    reference trajectory, with the helpers and bands of tests/test_ref_trajectory.py"""
    from types import SimpleNamespace
    import torch
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import hover_initial_conditions
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    B, K = 128, 8
    st, _ = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    tab = _smooth_table(B, K, 17)
    m = _handle(B, dtype, mode)
    m.set_state(st.astype(_np_dtype(dtype)), tab[0].astype(_np_dtype(dtype)))
    m.set_reference_trajectory(tab.astype(_np_dtype(dtype)))
    m.record_history(K)
    m.rollout(K)
    hist = m.history()
    for k in range(K):
        s_o, out_o = _oracle_steps(oracle_built, perm, st, tab[:k + 1], np.float64)
        s_o32, _ = _oracle_steps(oracle_built, perm, st, tab[:k + 1], np.float32)
        rec = SimpleNamespace(state=hist["state"][k + 1], out=hist["out"][k], dtype=m.dtype)
        _check_against_oracle("step history, step %d of 8 %s" % (k, name), rec, s_o, out_o, s_o32)


@pytest.mark.gpu
def test_history_refusals_with_a_handle():
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B = 64
    st, ref = hover_initial_conditions(B, 1, np.float32)
    m = BatchUprightMPC(B, torch.float32)
    m.set_state(st, ref)
    m.record_history(4, status=True, info=True)
    m.rollout(1)
    torch.cuda.synchronize()
    for t in m._hist.values():
        t[2 if t is m._hist["state"] else 1:].fill_(-7)      # what no step has written yet
    before = {k: v.clone() for k, v in m._hist.items()}
    state, t_ms = m.state.clone(), m.time_ms
    with pytest.raises(RuntimeError, match="step history ends"):
        m.rollout(4)                                    # 1 + 4 > 4: refused before anything is launched or copied
    torch.cuda.synchronize()
    assert m.history_cursor == 1 and m.time_ms == t_ms and torch.equal(m.state, state)
    for k, v in m._hist.items():
        assert torch.equal(v, before[k]), k
    # update(), plant() and a reactive rollout record nothing and leave the cursor
    m.update()
    m.plant(m.out[0:3].clone(), 1)
    m.reactive_rollout(1)
    torch.cuda.synchronize()
    assert m.history_cursor == 1
    for k, v in m._hist.items():
        assert torch.equal(v, before[k]), k
    m.rollout(3)
    assert m.history_cursor == 4
    with pytest.raises(RuntimeError, match="step history ends"):
        m.rollout(1)
    # bad arguments: steps < 1, a cursor outside [0, steps]; the handle keeps its history
    L, p = m.L, m._hist["out"].data_ptr()
    for steps, cur in ((0, 0), (4, -1), (4, 5)):
        assert L.umpcBatchSetHistory(m.h, None, C.c_void_p(p), None, None, steps, cur) == -1
        assert b"umpcBatchSetHistory" in L.umpcLastError()
    assert m.history_cursor == 4
    assert L.umpcBatchSetHistory(m.h, None, C.c_void_p(p), None, None, 4, 4) == 0 and m.history_cursor == 4
    m.record_history(None)
    assert m.history_cursor == 0
    m.rollout(2)                                        # history off: nothing to overrun
    # a handle without a plant has no trajectory
    n0 = BatchUprightMPC(B, torch.float32, nsub=0)
    with pytest.raises(RuntimeError):
        n0.record_history(4)
    assert L.umpcBatchSetHistory(n0.h, None, C.c_void_p(p), None, None, 4, 0) == -1 and b"nsub" in L.umpcLastError()


@pytest.mark.gpu
def test_history_blocks_equal_the_columns_of_the_undivided_run():
    """partition invariance: 128 robots whole and as 2 blocks of 64 with global_batch = 128, the form pinned (fp32 lane and
    quad): shard.history_block of the whole run's history == the block's own history"""
    import torch
    from robobee3d_amd import shard
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B, K = 128, 4
    st, ref = hover_initial_conditions(B, 5, np.float32, tilt=0.3)
    ref[0:3] = np.random.default_rng(3).normal(size=(3, B))
    st, ref = torch.as_tensor(st).cuda(), torch.as_tensor(ref).cuda()
    for mode, kernel in (("lane", "umpc_rollout_asm_kernel"), ("quad", "umpc_rollout_asm_quad_kernel")):
        whole = BatchUprightMPC(B, torch.float32, plant_mode=1)
        whole.set_step_kernel(mode)
        whole.set_state(st, ref)
        whole.record_history(K, status=True, info=True)
        whole.rollout(K)
        assert whole.kernel_name == kernel
        for rank in range(2):
            lo, hi = shard.split_range(B, rank, 2)
            blk = BatchUprightMPC(hi - lo, torch.float32, plant_mode=1, global_batch=B)
            blk.set_step_kernel(mode)
            blk.set_state(shard.table_block(st, lo, hi), shard.table_block(ref, lo, hi))
            blk.record_history(K, status=True, info=True)
            blk.rollout(K)
            assert blk.kernel_name == kernel
            want, got = shard.history_block(whole.history(), lo, hi), blk.history()
            for n in RECORDS:
                assert torch.equal(got[n], want[n]), (mode, rank, n)


@pytest.mark.gpu
def test_history_log_agrees_with_control_test_log_and_metrics():
    """fp64, helix task, 12 MPC steps on the fixed schedule. control_test_log logs row ti AFTER plant substep ti and fires
    at ti = 25 k on the state row 25 k - 1 shows; history_log row k holds the state step k fired on. So: y / R of row k == row
    25 k - 1 of the substep log (k >= 1; row 0 is the initial state), u / accdes / pdes / t of row k == row 25 k. Both paths
    run the same fp64 kernels step by step; the margins are the ones the fp64 kernel is held to against the oracle in
    tests/test_ref_trajectory.py (state rtol 1e-7 atol 1e-9, out rtol 1e-6 atol 1e-8). `metric` == metrics()."""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B, K, nsub = 4, 12, 25
    st, ref = hover_initial_conditions(B, 2, np.float64, tilt=0.2)
    ref[:] = 0
    a, b = BatchUprightMPC(B, torch.float64), BatchUprightMPC(B, torch.float64)
    for m in (a, b):
        m.set_state(st, ref)
        m.set_task("helix", trajAmp=20, trajFreq=2, dz=0.1, useY=False)
    a.record_history(K)
    a.rollout(K)
    lg = a.history_log(robots=(1,))[1]
    ct = b.control_test_log(K * nsub * 0.2, robots=(1,))[1]
    assert lg["y"].shape == (K, 12) and lg["u"].shape == (K, 3) and lg["accdes"].shape == (K, 6) and lg["pdes"].shape == (K, 3)
    assert set(lg) >= set(ct)
    rows = nsub * np.arange(K)
    np.testing.assert_allclose(lg["t"], ct["t"][rows], rtol=0, atol=1e-9)
    np.testing.assert_allclose(lg["y"][0], np.concatenate((st[0:3, 1], st[9:12, 1], st[12:18, 1])), rtol=0, atol=0)
    np.testing.assert_allclose(lg["y"][1:], ct["y"][rows[1:] - 1], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(lg["R"][1:], ct["R"][rows[1:] - 1], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(lg["u"], ct["u"][rows], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(lg["accdes"], ct["accdes"][rows], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(lg["pdes"], ct["pdes"][rows], rtol=1e-12, atol=1e-12)
    assert np.all(np.abs(lg["u"][:, 1:3]) <= 100.0)
    met = a.metrics(K)[:, 1].cpu().numpy()
    assert lg["metric"] == (float(met[0]), float(met[1]))
    np.testing.assert_allclose(lg["metric"], ct["metric"], rtol=1e-7)
