"""Velocity impulses: a kick (dv_world, domega_body) per closed-loop step and per robot INSIDE one rollout launch
(umpcBatchSetImpulses), added to rows 12..17 of the state after the step's last plant substep and ahead of its state store.
CPU: the regenerated lane and quad streams interpreted with a table, bit for bit against chained single steps with the numpy
add in between, guard words, the 64-bit slice offset with a wrapping low word and a product above 2^32, the layout of the third
parameter block, the instruction budget, the oracle chain, the reference's own controlTest(tpert=...) log through the oracle,
exports and refusals, the helpers.
GPU: one launch = K launches + add in every step-kernel form and both plant modes, the options of the stream, all three tables
(reference trajectory, full history, impulses) with non-zero cursors on one handle in every form, the oracle chain,
refusals, partition invariance, the reactive controller under the table, the reference's log through one nsub = 1 launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import golden, record_margin
from test_asm_step import _arrays
from test_ref_trajectory import OUTPUTS, _check_against_oracle, _handle, _np_dtype, _slices, _smooth_table
from test_step_history import GUARD, GUARD_F, GUARD_I, HIST_MODES, HIST_MODE_IDS, KERNEL, ROWS, _strides, _tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kick sizes: the reference's own push is 2 (mm / ms) on one velocity component (template/uprightmpc2.py:132); body rates up to
# 0.02 rad / ms. test_oracle_chain_stays_finite_for_these_kicks checks on the CPU that the oracle chain alone stays finite and
# inside the margins of _check_against_oracle with them, so that no case needs excluding.
DV, DW = 2.0, 0.02


def _kicks(K, B, seed, dtype=np.float64):
    """[K, 6, B], the shape of the reference's experiment: every robot gets ONE velocity push (uniform in +-DV on one world axis,
    at one step) and ONE body-rate push (+-DW on one body axis, at another or the same step); every fourth robot is never
    pushed. Slices differ, most entries are zero."""
    rng = np.random.default_rng(seed)
    tab = np.zeros((K, 6, B))
    b = np.arange(B)
    tab[rng.integers(0, K, B), rng.integers(0, 3, B), b] = rng.uniform(-DV, DV, B)
    tab[rng.integers(0, K, B), 3 + rng.integers(0, 3, B), b] = rng.uniform(-DW, DW, B)
    tab[:, :, ::4] = 0.0
    return tab.astype(dtype)


def _dense(K, seed, dtype=np.float64):
    """[K, 6] for one robot: every component of every slice non-zero"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.25, 1.0, size=(K, 6)) * rng.choice([-1.0, 1.0], size=(K, 6))
    return (u * np.array([DV] * 3 + [DW] * 3)).astype(dtype)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def _imp_array(tab):
    """the table of one interpreted run (rows 6k .. 6k + 5 = slice k) with GUARD rows of guard words behind it"""
    return np.concatenate((tab.astype(np.float32).ravel(), np.full(GUARD, GUARD_F, np.float32)))


@pytest.mark.parametrize("plant", [0, 1], ids=["plant0", "rk4"])
@pytest.mark.parametrize("moved", [False, True], ids=["in-place", "refstep+history"])
@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_stream_adds_one_slice_per_step_bit_for_bit(quad, moved, plant):
    """K = 3 with a table of three DIFFERENT slices against three chained K = 1 runs of the same stream with the numpy fp32 add
    `state[12:18] += tab[k]` in between: state, ctrl, out, status, info and stats equal as uint32 -- in place, and with
    `refstep` and the four history strides set (then state slice k + 1 holds the kicked state, and all six pointers of the
    stream move). The table is only read; the guard words behind it and behind every table are untouched."""
    from robobee3d_amd import asmstep
    from robobee3d_amd.batch import hover_initial_conditions
    ins = asmstep.StepGen(quad=quad).program()
    fl = asmstep.host_floats()
    st, ref = hover_initial_conditions(1, 20201118, np.float32, tilt=0.3)
    K = 3
    kick = _dense(K, 9, np.float32)
    kick[1, 3:] = 0.0                                    # mixed slices: one without a rate kick ...
    kick[2, 0] = -0.0                                    # ... and a signed zero
    rtab = _slices(K, 5)
    ints = dict(maxIter=50, nsub=25, plant=plant)
    base = _arrays(st, ref, 0)
    one = _tables(base, K) if moved else {n: None if x is None else x.copy() for n, x in base.items()}
    if moved:
        one["ref"] = rtab.ravel().copy()
    one["impulse"] = _imp_array(kick)
    moves = dict(refstep=9 * asmstep.STRIDE, **_strides()) if moved else {}
    asmstep.simulate(ins, one, dict(ints, K=K, **moves), fl)
    assert np.array_equal(one["impulse"][:6 * K], kick.ravel()) and np.all(one["impulse"][6 * K:] == GUARD_F)
    chained = _arrays(st, ref, 0)
    for k in range(K):
        if moved:
            chained["ref"] = rtab[k].copy()
        asmstep.simulate(ins, chained, dict(ints, K=1), fl)
        chained["state"][12:18] += kick[k]
        if moved:
            for n, rows in ROWS.items():
                sl = k + 1 if n == "state" else k
                assert np.array_equal(one[n][rows * sl:rows * (sl + 1)].view(np.uint32), chained[n].view(np.uint32)), (n, k)
    if moved:
        for n in ROWS:
            assert np.all(one[n][-GUARD:] == (GUARD_I if n == "status" else GUARD_F)), n
        assert np.array_equal(one["state"][:18], base["state"])                # slice 0: read, never written
    for n in OUTPUTS if not moved else ("ctrl", "stats"):
        assert np.array_equal(one[n].view(np.uint32), chained[n].view(np.uint32)), n
    if not moved:                                        # the kicks do act: the same run without a table ends elsewhere
        plain = _arrays(st, ref, 0)
        asmstep.simulate(ins, plain, dict(ints, K=K), fl)
        assert not np.array_equal(one["state"], plain["state"])


@pytest.mark.parametrize("plant", [0, 1], ids=["plant0", "rk4"])
@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_null_table_is_a_plain_run_and_a_zero_table_equals_it_by_value(quad, plant):
    """with a null table pointer every array equals the run of a program without the impulse block, bit for bit (the block is
    cut out of the instruction list: nothing else of the stream depends on it); an all-zero table is six adds of +0.0 -- equal
    by VALUE (-0.0 + 0.0 = +0.0 is not a skipped add)"""
    from robobee3d_amd import asmstep
    from robobee3d_amd.batch import hover_initial_conditions
    ins = asmstep.StepGen(quad=quad).program()
    lo, hi = _impulse_block(ins)
    cut = ins[:lo] + ins[hi:]
    fl = asmstep.host_floats()
    st, ref = hover_initial_conditions(1, 20201118, np.float32, tilt=0.3)
    ints = dict(maxIter=50, nsub=25, plant=plant, K=2)
    null, without, zero = _arrays(st, ref, 0), _arrays(st, ref, 0), _arrays(st, ref, 0)
    n_null = asmstep.simulate(ins, null, ints, fl)
    n_cut = asmstep.simulate(cut, without, ints, fl)
    zero["impulse"] = _imp_array(np.zeros((2, 6)))
    asmstep.simulate(ins, zero, ints, fl)
    for n in OUTPUTS:
        assert np.array_equal(null[n].view(np.uint32), without[n].view(np.uint32)), n
        assert np.array_equal(zero[n], null[n]), n
    assert n_null - n_cut == 2 * 5                       # five scalar instructions per step, nothing else


def _impulse_block(prog):
    """[lo, hi) of the impulse block in a program: from the s_mov_b32 of the block's offset to the label its null test jumps to"""
    from robobee3d_amd import asmstep
    at = [k for k, t in enumerate(prog) if t[0] == "s_mov_b32" and t[1] == "s%d" % asmstep.S_TMP and t[2] == asmstep.IMP_OFF]
    assert len(at) == 1
    lo = at[0]
    br = next(t for t in prog[lo:] if t[0] == "s_cbranch_scc1")
    hi = next(k for k in range(lo, len(prog)) if prog[k] == ("label", br[1][:-1]))
    return lo, hi + 1


@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_slice_offset_carries_into_the_high_word(quad):
    """the 64-bit address of row 0 of slice `step`, extracted from the program (the scalar instructions from the first
    s_mul_hi_u32 to the first global_load_dword of the block) and interpreted: a base whose low word wraps, and a step x
    stride product above 2^32 (step 3 000 at B = 65 536: 4.7 GB) -- the high word is right in both, and stays without a wrap.
    Then the five row advances by `stride`, with a low word that wraps in the middle of the slice."""
    from robobee3d_amd import asmstep, isasim
    prog = asmstep.StepGen(quad=quad).program()
    lo, hi = _impulse_block(prog)
    blk = prog[lo:hi]
    first = next(k for k, t in enumerate(blk) if t[0] == "s_mul_hi_u32")
    loads = [k for k, t in enumerate(blk) if t[0] == "global_load_dword"]
    assert len(loads) == 6
    S = asmstep.S_IMP
    stride = 6 * 65536 * 4
    for base, step in ((0x7F00FFF00000, 1), (0x7F0080000000, 3000), (0x7F00FFFFFFF0, 3000), (0x7F0000000010, 0), (0x7F0080000000, 1)):
        m = isasim.Machine(blk[first:loads[0]], sgpr={S: base & 0xFFFFFFFF, S + 1: base >> 32, S + 2: stride, asmstep.S_STEP: step})
        isasim.run(m)
        assert m.S[S] | (m.S[S + 1] << 32) == base + step * stride, (hex(base), step)
    rows = [t for t in blk[loads[0]:loads[5] + 1] if t[0] != "global_load_dword"]
    m = isasim.Machine(rows, sgpr={S: 0xFFF80000, S + 1: 0x7F00, asmstep.S_INT["stride"]: 65536 * 4})
    isasim.run(m)
    assert m.S[S] | (m.S[S + 1] << 32) == 0x7F00FFF80000 + 5 * 65536 * 4 and m.S[S + 1] == 0x7F01
    # every load of the block goes through that pair with the lanes' own offset v0, and nothing else does
    pair = "s[%d:%d]" % (S, S + 1)
    assert all(blk[k][2:4] == ("v0", pair) for k in loads)
    assert [t[0] for t in blk if t[0] in ("s_add_u32", "s_addc_u32", "s_cmp_lt_u32", "s_cselect_b32")] == []


def test_third_block_layout_and_old_offsets():
    """the block lies at byte 312 = HIST_OFF + HIST_BYTES, 8-aligned, behind StepHist; PARAM_BYTES and every older offset are
    what they were; the generated header asserts the layout; simulate() packs three blocks and knows an `impulse` region"""
    from robobee3d_amd import asmstep
    assert asmstep.IMP_OFF == 312 == asmstep.HIST_OFF + asmstep.HIST_BYTES and asmstep.IMP_OFF % 8 == 0
    assert asmstep.OFF["imp"] == 312 and asmstep.OFF["impstep"] == 320
    assert asmstep.PARAM_BYTES == 292 and asmstep.HIST_OFF == 296 and asmstep.HIST_BYTES == 16
    assert asmstep.OFF["refstep"] == 288 and asmstep.OFF["state"] == 0 and asmstep.OFF["done"] == 128 and asmstep.OFF["dt"] == 160
    assert [asmstep.OFF[n] for n in asmstep.HIST_INTS] == [296, 300, 304, 308]
    hdr = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_step_asm.h")).read()
    assert "static_assert(offsetof(StepArgs, h) == 296 && sizeof(StepHist) == 16, \"StepHist layout\");" in hdr
    assert "static_assert(offsetof(StepArgs, i) == 312 && sizeof(StepImp) == 16 && offsetof(StepImp, impstep) == 8, \"StepImp layout\");" in hdr
    assert re.search(r"struct StepArgs \{\s*StepParams p;\s*StepHist h;\s*StepImp i;\s*\};", hdr)
    src = open(os.path.join(ROOT, "robobee3d_amd", "csrc", "umpc_mi355x.hip")).read()
    assert "pa.i = umpcasm::StepImp{nullptr, 0, 0};" in src               # the B = 1 drop-in passes a null table
    # the stream reads the block through an SGPR offset, once per step
    for quad in (False, True):
        prog = asmstep.StepGen(quad=quad).program()
        lo, hi = _impulse_block(prog)
        assert prog[lo + 1] == ("s_load_dwordx4", "s[%d:%d]" % (asmstep.S_IMP, asmstep.S_IMP + 3), "s[%d:%d]" % (asmstep.S_PBLK, asmstep.S_PBLK + 1),
                                "s%d" % asmstep.S_TMP)


def test_instruction_budget_of_the_impulse_block():
    """per step the table adds exactly six global_load_dword, six v_add_f32 and scalar instructions, in each form; with a null
    table five scalar instructions are executed (see test_null_table_...)"""
    from robobee3d_amd import asmstep
    for quad in (False, True):
        prog = asmstep.StepGen(quad=quad).program()
        lo, hi = _impulse_block(prog)
        blk = [t for t in prog[lo:hi] if t[0] != "label"]
        vec = [t[0] for t in blk if not t[0].startswith("s_")]
        assert sorted(vec) == ["global_load_dword"] * 6 + ["v_add_f32"] * 6, vec
        assert len(blk) - len(vec) <= 40
        adds = [t for t in blk if t[0] == "v_add_f32"]
        assert sorted(int(t[1][1:]) for t in adds) == sorted(int(t[2][1:]) for t in adds)       # dq += slice, in place
        # the block sits between the plant's last substep and the state store
        store = next(k for k in range(hi, len(prog)) if prog[k][0] == "global_store_dword")
        assert "s[%d:%d]" % (asmstep.S_PTR["state"], asmstep.S_PTR["state"] + 1) in prog[store]


def _oracle_chain(ob, perm, st, ref, kick, dtype, nsub=25, dtsim=0.2, reftab=None, **kw):
    """the closed loop through the oracle, one batch_rollout(K = 1) per step with t0 advanced and the add in `dtype` in between
    (it carries state / ctrl in place); returns state, out of the last step and the state after every step [K + 1, 18, B]"""
    B = st.shape[1]
    s = st.astype(dtype).copy()
    c = np.zeros((127, B), dtype)
    c[124:] = 1
    out, hist = None, [s.copy()]
    for k in range(kick.shape[0]):
        r = np.ascontiguousarray((ref if reftab is None else reftab[k]).astype(dtype))
        out, _, _ = ob.batch_rollout(s, c, r, 1, dtype=dtype, perm=perm, nsub=nsub, dtsim=dtsim, t0=k * nsub * dtsim, **kw)
        s[12:18] += kick[k].astype(dtype)
        hist.append(s.copy())
    return s, out, np.stack(hist)


def _bands(s_o, s_o32):
    """the self-calibrating fp32 band of _check_against_oracle: at most 4x the distance of the fp32 CPU oracle from the fp64 one,
    floors 2e-3 mm / 3e-4"""
    return (max(2e-3, 4 * np.abs(s_o32[0:3].astype(np.float64) - s_o[0:3]).max()),
            max(3e-4, 4 * np.abs(s_o32[3:].astype(np.float64) - s_o[3:]).max()))


def test_oracle_chain_stays_finite_for_these_kicks(oracle_built, structure):
    """the kick sizes of this file through the oracle chain ALONE, fp64 and fp32, both plant modes, K = 8, 128 robots: finite,
    every status solved-or-max-iter as without kicks, and the fp32 oracle within 0.05 mm / 5e-3 of the fp64 one -- so the bands of
    _check_against_oracle (4x that distance) stay tight bands and no robot needs excluding in the GPU tests"""
    from robobee3d_amd.batch import hover_initial_conditions
    perm = structure["perm"]
    B, K = 128, 8
    st, ref = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    kick = _kicks(K, B, 4)
    for pm in (0, 1):
        s_o, out_o, _ = _oracle_chain(oracle_built, perm, st, ref, kick, np.float64, plant_mode=pm)
        s_o32, _, _ = _oracle_chain(oracle_built, perm, st, ref, kick, np.float32, plant_mode=pm)
        assert np.all(np.isfinite(s_o)) and np.all(np.isfinite(out_o)) and np.all(np.isfinite(s_o32))
        dp, dr = np.abs(s_o32[0:3] - s_o[0:3]).max(), np.abs(s_o32[3:] - s_o[3:]).max()
        print("plant %d: fp32 oracle vs fp64 oracle |dp| %.3e mm, |dR|,|ddq| %.3e" % (pm, dp, dr))
        assert dp < 0.05 and dr < 5e-3


@pytest.mark.parametrize("quad", [False, True], ids=["lane", "quad"])
def test_interpreted_stream_with_a_table_matches_the_oracle_chain(oracle_built, structure, quad):
    """fp32: the interpreted stream, K = 3 with a table, against oraclebind.batch_rollout(K = 1) chained with t0 advanced and
    the add in between, inside the margins of _check_against_oracle (4x the fp32 oracle's own distance from the fp64 oracle,
    floors 2e-3 mm / 3e-4). fp64 has no interpreted stream of the whole step: its oracle chain is checked against the
    reference's own log in test_reference_push_log_through_the_oracle_chain."""
    from robobee3d_amd import asmstep
    from robobee3d_amd.batch import hover_initial_conditions
    from robobee3d_amd import _lib
    lperm = np.array(_lib.lib().umpcKKTPerm().contents)
    ins = asmstep.StepGen(quad=quad).program()
    fl = asmstep.host_floats()
    K = 3
    st, ref = hover_initial_conditions(1, 20201118, np.float32, tilt=0.3)
    kick = _dense(K, 6)[:, :, None]
    for pm in (0, 1):
        a = _arrays(st, ref, 0)
        a["impulse"] = _imp_array(kick[:, :, 0])
        asmstep.simulate(ins, a, dict(maxIter=50, nsub=25, plant=pm, K=K), fl)
        s_o, out_o, _ = _oracle_chain(oracle_built, lperm, st.astype(np.float64), ref.astype(np.float64), kick, np.float64, plant_mode=pm)
        s_o32, _, _ = _oracle_chain(oracle_built, lperm, st.astype(np.float64), ref.astype(np.float64), kick, np.float32, plant_mode=pm)
        band_p, band_r = _bands(s_o, s_o32)
        s = a["state"].astype(np.float64)[:, None]
        dp, dr = np.abs(s[0:3] - s_o[0:3]).max(), np.abs(s[3:] - s_o[3:]).max()
        record_margin("interpreted %s plant %d + kicks" % ("quad" if quad else "lane", pm), "|dp| mm vs fp64 oracle chain", dp, band_p)
        record_margin("interpreted %s plant %d + kicks" % ("quad" if quad else "lane", pm), "|dR|,|ddq| vs fp64 oracle chain", dr, band_r)
        assert dp <= band_p and dr <= band_r, (pm, dp, band_p, dr, band_r)


def _fixture_setup():
    """the start of controlTest (template/uprightmpc2.py:101-103), the task of the S trajectory and the dense kick table of the
    recorded run: the reference kicks ahead of the MPC call of loop iteration kick_ti, which is the end of step kick_ti - 1"""
    from scipy.spatial.transform import Rotation
    g = golden("impulse_log.npz")
    n, kt = len(g["t"]), int(g["kick_ti"])
    st = np.zeros((18, 1))
    st[3:12, 0] = Rotation.from_euler("xyz", [0.5, -0.5, 0]).as_matrix().T.ravel()       # column-major
    st[12, 0] = 0.1
    ref = np.zeros((9, 1))
    ref[8] = 1.0
    kick = np.zeros((n, 6, 1))
    kick[kt - 1, :, 0] = g["kick"]
    task_p = (float(g["trajAmp"]), float(g["trajFreq"]), float(g["dz"]), float(g["useY"]))
    return g, n, kt, st, ref, kick, task_p


def _log_y(hist, kick=None):
    """[K + 1, 18, 1] states -> the reference log's y rows (p, Rb[:, 2], dq) after every substep. State slice c + 1 holds the
    kick of slice c, which the reference adds AFTER it has written log row c (at the top of iteration c + 1): the kick is taken
    off that row again."""
    y = np.concatenate((hist[1:, 0:3, 0], hist[1:, 9:12, 0], hist[1:, 12:18, 0]), axis=1)
    if kick is not None:
        y[:, 6:12] -= kick[:, :, 0]
    return y


def test_reference_push_log_through_the_oracle_chain(oracle_built, structure):
    """the same two logs through the fp64 oracle CHAIN -- batch_rollout(K = 1) with nsub = 1 (MPC at every substep = the
    reference loop), plant mode 0, the helix task at the fire time, t0 advanced and ONE non-zero slice added in between: the
    statement the GPU kernels are checked against. It carries between steps what the product carries (iterates, thrust
    accumulator, the last scaling rows), not the reference's whole solver workspace, so it leaves the reference's log by more
    than round-off even without a push (measured: 0.314 on z after 200 steps; the fp32 and the fp64 chain agree to 5e-5). The
    un-kicked replay is therefore the yardstick, as in the GPU test of the same fixture: the kicked replay may deviate from its
    log four times as far (measured: 0.217). Before the kick both replays are the same numbers, and the kick is in the state
    slice that the controller of iteration kick_ti reads."""
    g, n, kt, st, ref, kick, task_p = _fixture_setup()
    perm = structure["perm"]
    kw = dict(nsub=1, plant_mode=0, task=1, task_p=task_p)
    _, _, h_plain = _oracle_chain(oracle_built, perm, st, ref, np.zeros_like(kick), np.float64, **kw)
    _, _, h_kick = _oracle_chain(oracle_built, perm, st, ref, kick, np.float64, **kw)
    y_plain, y_kick = _log_y(h_plain), _log_y(h_kick, kick)
    assert np.array_equal(y_plain[:kt - 1], y_kick[:kt - 1])
    assert np.allclose(h_kick[kt, 12:18, 0] - h_plain[kt, 12:18, 0], g["kick"], atol=1e-12)
    d0 = np.abs(y_plain - g["plain_y"]).max()
    d1 = np.abs(y_kick - g["kick_y"]).max()
    print("fp64 oracle chain vs reference log: un-kicked %.3e, kicked %.3e (bound %.3e)" % (d0, d1, 4 * d0))
    record_margin("push log, oracle chain fp64", "kicked max |dy| vs reference", d1, 4 * d0, "un-kicked %.3e" % d0)
    assert d1 <= 4 * d0
    # the fixture itself: the runs are the same numbers up to the row the kick precedes, and the push moves the robot by millimetres
    assert np.array_equal(g["kick_y"][:kt], g["plain_y"][:kt]) and not np.array_equal(g["kick_y"][kt], g["plain_y"][kt])
    assert np.abs(g["kick_y"] - g["plain_y"]).max() > 1.0


def test_new_exports_and_refusals_without_a_handle():
    from robobee3d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "umpc_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    for decl in ("int umpcBatchSetImpulses(umpc_batch_t *h, const void *tab, long long steps, long long cursor0);",
                 "long long umpcBatchImpulseCursor(const umpc_batch_t *h);"):
        assert decl in flat, decl
    assert "786 MB" in flat and "6 x B x steps" in flat
    L = _lib.lib()
    for sym in ("umpcBatchSetImpulses", "umpcBatchImpulseCursor"):
        assert sym in _lib.EXPORTS and getattr(L, sym)
    assert L.umpcBatchImpulseCursor.restype is C.c_longlong
    assert L.umpcBatchSetImpulses.argtypes == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong]
    # argument checks come before any HIP call: no device needed
    assert L.umpcBatchSetImpulses(None, None, 4, 0) == -1 and b"umpcBatchSetImpulses" in L.umpcLastError()
    assert L.umpcBatchImpulseCursor(None) == 0


def test_impulse_block_is_a_column_slice():
    import torch
    from robobee3d_amd import shard
    tab = torch.arange(5 * 6 * 7).reshape(5, 6, 7)
    blk = shard.impulse_block(tab, 2, 6)
    assert blk.is_contiguous() and blk.shape == (5, 6, 4) and torch.equal(blk, tab[:, :, 2:6])


def test_impulse_table_against_a_numpy_loop():
    import torch
    from robobee3d_amd.batch import impulse_table
    steps, B = 7, 10
    rng = np.random.default_rng(3)
    events = [(3, None, (0, 2, 0, 0, 0, 0)),                                   # the reference's push, every robot
              (0, 4, rng.normal(size=6)), (6, [1, 5, 9], rng.normal(size=(6, 3))), (3, slice(2, 5), rng.normal(size=6)),
              (3, [4, 2], rng.normal(size=(6, 2)))]
    for dt, ndt in ((torch.float32, np.float32), (torch.float64, np.float64)):
        want = np.zeros((steps, 6, B), ndt)
        for step, robots, vec in events:
            vec = np.asarray(vec, np.float64).astype(ndt)
            idx = range(B) if robots is None else range(B)[robots] if isinstance(robots, slice) else np.atleast_1d(robots)
            for c, b in enumerate(idx):
                want[step, :, b] += vec if vec.ndim == 1 else vec[:, c]
        got = impulse_table(steps, B, events, dt)
        assert got.dtype == dt and got.shape == (steps, 6, B) and got.is_contiguous()
        assert np.array_equal(got.numpy(), want)
    with pytest.raises(ValueError):
        impulse_table(steps, B, [(7, None, np.zeros(6))])
    with pytest.raises(ValueError):
        impulse_table(steps, B, [(0, [1, 1], np.zeros(6))])
    with pytest.raises(ValueError):
        impulse_table(steps, B, [(0, None, np.zeros(5))])


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
RECORDS = ("state", "out", "status", "info")


def _final_equal(a, b, what=""):
    import torch
    for k in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


def _step_and_add(m, tab, k):
    m.rollout(1)
    m.state[12:18] += tab[k]


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [0, 1], ids=["plant0", "rk4"])
@pytest.mark.parametrize("name,dtype,mode", HIST_MODES, ids=HIST_MODE_IDS)
def test_one_launch_equals_k_launches_with_adds(name, dtype, mode, plant):
    """rollout(6) with a table == six rollout(1) of a second handle with `state[12:18] += tab[k]` in between, torch.equal on
    every array, in all six step-kernel forms and both plant modes (B = 100: a partly filled wavefront). With a history the
    state slice k + 1 holds the kicked state and the other records are the chain's; rollout(2) + rollout(4) continue one table;
    a non-zero cursor0 starts in the middle of one."""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    B, K = 100, 6
    st, ref = hover_initial_conditions(B, 7, _np_dtype(dtype), tilt=0.3)
    ref[0:3] = np.random.default_rng(1).normal(size=(3, B))
    tab = torch.as_tensor(_kicks(K, B, 5, _np_dtype(dtype))).cuda()
    one, many, hist, split, off = (_handle(B, dtype, mode, plant_mode=plant) for _ in range(5))
    for h in (one, many, hist, split, off):
        h.set_state(st, ref)
    one.set_impulses(tab)
    assert one.impulse_cursor == 0
    one.rollout(K)
    assert one.impulse_cursor == K and one.kernel_name == KERNEL[name]
    hist.set_impulses(tab)
    hist.record_history(K, status=True, info=True)
    hist.rollout(K)
    rec = hist.history()
    assert torch.equal(rec["state"][0], torch.as_tensor(st).cuda())
    for k in range(K):
        _step_and_add(many, tab, k)
        for n in RECORDS:
            assert torch.equal(rec[n][k + 1 if n == "state" else k], getattr(many, n)), (name, n, k)
    assert many.kernel_name == one.kernel_name == hist.kernel_name
    _final_equal(one, many, name)
    _final_equal(hist, many, name + " history")
    assert one.time_ms == many.time_ms
    split.set_impulses(tab)
    split.rollout(2)
    assert split.impulse_cursor == 2
    split.rollout(4)
    assert split.impulse_cursor == 6
    _final_equal(split, many, name + " 2+4")
    junk = torch.full((3, 6, B), 1e3, dtype=tab.dtype, device=tab.device)
    off.set_impulses(torch.cat((junk, tab)), cursor0=3)
    off.rollout(K)
    assert off.impulse_cursor == 9
    _final_equal(off, many, name + " cursor0")
    # the kicks act, and a zero table equals no table by value
    plain, zero = _handle(B, dtype, mode, plant_mode=plant), _handle(B, dtype, mode, plant_mode=plant)
    for h in (plain, zero):
        h.set_state(st, ref)
    zero.set_impulses(torch.zeros_like(tab))
    plain.rollout(K)
    zero.rollout(K)
    assert not torch.equal(plain.state, one.state)
    for k in OUTPUTS:
        assert bool((getattr(zero, k) == getattr(plain, k)).all()), k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "lane", "quad"])
def test_impulses_combine_with_the_options_of_the_stream(mode):
    """impulses + a reference table + per-robot weights + fused WL + per-robot Ib / gain + a history in one fp32 launch == K
    single-step launches with adds"""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, BatchWLCon, hover_initial_conditions, monte_carlo_draws
    from test_wl_step import _args
    g = golden("mpc_wl_loop.npz")
    B, K = 128, 6
    st, ref = hover_initial_conditions(B, 3, np.float32, tilt=0.3)
    rtab = torch.as_tensor(_smooth_table(B, K, 23).astype(np.float32)).cuda()
    tab = torch.as_tensor(_kicks(K, B, 8, np.float32)).cuda()
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
    a.set_reference_trajectory(rtab)
    a.set_impulses(tab)
    a.record_history(K)
    a.rollout(K)
    assert a.kernel_name in ("umpc_rollout_asm_kernel", "umpc_rollout_asm_quad_kernel")
    assert (a.ref_cursor, a.impulse_cursor, a.history_cursor) == (K, K, K)
    rec = a.history()
    for k in range(K):
        b.ref.copy_(rtab[k])
        _step_and_add(b, tab, k)
        assert torch.equal(rec["state"][k + 1], b.state) and torch.equal(rec["out"][k], b.out), k
    assert a.kernel_name == b.kernel_name
    _final_equal(a, b, mode)
    assert torch.equal(wa.u, wb.u) and torch.equal(wa.w0, wb.w0)


# all six step-kernel forms: one full wavefront for the lane and C++ forms, one full and one ragged wave of quads for the two
# quad forms ("f64" = automatic = the fp64 quad form, whose steps the library issues one per launch)
ALL_TABLES_CASES = [(n, d, m, B) for n, d, m in HIST_MODES for B in ((16, 20) if n in ("f32-quad", "f64") else (64,))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode,B", ALL_TABLES_CASES, ids=["%s-B%d" % (c[0], c[3]) for c in ALL_TABLES_CASES])
def test_all_tables_at_once_one_launch_equals_k_launches(name, dtype, mode, B):
    """a reference trajectory, the full history (state, out, status, info) and an impulse table on ONE handle, each of 5 slices
    with its cursor starting at 1 (a wrong offset reads or writes another slice): rollout(3) == three rollout(1) of a second
    handle set up the same way, torch.equal on every array, on the WHOLE of every history table (pre-filled, so the slices no
    step may touch count too) and on the three cursors and the clock. A rollout(0) in the middle of the chain changes nothing."""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    K, S, C0 = 3, 5, 1
    ndt = _np_dtype(dtype)
    st, ref = hover_initial_conditions(B, 7, ndt, tilt=0.3)
    rtab = torch.as_tensor(_smooth_table(B, S, 23).astype(ndt)).cuda()
    tab = torch.as_tensor(_kicks(S, B, 5, ndt)).cuda()
    one, many = _handle(B, dtype, mode), _handle(B, dtype, mode)
    for h in (one, many):
        h.set_state(st, ref)
        h.set_reference_trajectory(rtab, cursor=C0)
        h.set_impulses(tab, cursor0=C0)
        h.record_history(S, status=True, info=True)
        for t in h._hist.values():
            t.fill_(-77)
        h.rewind_history(C0)

    def snapshot(h):
        return ([getattr(h, k).clone() for k in OUTPUTS] + [h._hist[n].clone() for n in RECORDS],
                (h.ref_cursor, h.history_cursor, h.impulse_cursor, h.time_ms))

    one.rollout(K)
    assert one.kernel_name == KERNEL[name]
    many.rollout(1)
    arrays0, scalars0 = snapshot(many)
    many.rollout(0)
    arrays1, scalars1 = snapshot(many)
    assert scalars1 == scalars0 and scalars0[:3] == (C0 + 1,) * 3 and scalars0[3] > 0, (name, scalars0, scalars1)
    for x, y in zip(arrays0, arrays1):
        assert torch.equal(x, y), (name, "rollout(0)")
    many.rollout(1)
    many.rollout(1)
    assert many.kernel_name == KERNEL[name]
    _final_equal(one, many, name)
    for n in RECORDS:
        assert torch.equal(one._hist[n], many._hist[n]), (name, n)
        assert bool((one._hist[n][C0 + K + (n == "state"):] == -77).all()) and bool((one._hist[n][:C0] == -77).all()), (name, n)
        assert not bool((one._hist[n][C0 + (n == "state"):C0 + K + (n == "state")] == -77).any()), (name, n)
    assert torch.equal(one._hist["state"][C0], torch.as_tensor(st).cuda())
    assert (one.ref_cursor, one.history_cursor, one.impulse_cursor) == (C0 + K,) * 3
    assert (many.ref_cursor, many.history_cursor, many.impulse_cursor, many.time_ms) == (C0 + K,) * 3 + (one.time_ms,)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype,mode", HIST_MODES, ids=HIST_MODE_IDS)
def test_impulses_with_a_task(name, dtype, mode):
    """the S trajectory of the reference's push experiment (helix, trajAmp 50, trajFreq 1) as the handle's task, with a table"""
    import torch
    from robobee3d_amd.batch import hover_initial_conditions
    B, K = 128, 5
    st, ref = hover_initial_conditions(B, 5, _np_dtype(dtype), tilt=0.3)
    tab = torch.as_tensor(_kicks(K, B, 12, _np_dtype(dtype))).cuda()
    one, many = _handle(B, dtype, mode), _handle(B, dtype, mode)
    for h in (one, many):
        h.set_state(st, ref)
        h.set_task("helix", trajAmp=50, trajFreq=1, dz=0.1, useY=False)
    one.set_impulses(tab)
    one.rollout(K)
    for k in range(K):
        _step_and_add(many, tab, k)
    _final_equal(one, many, name)


@pytest.mark.gpu
def test_large_batch_on_the_default_form():
    """B = 65 536 at K = 20 on the default lane form: one launch == 20 launches + adds"""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions_device
    B, K = 65536, 20
    st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
    gen = torch.Generator(device="cuda").manual_seed(3)
    tab = (torch.rand((K, 6, B), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1)
    tab[:, 0:3] *= DV
    tab[:, 3:6] *= DW
    one, many = BatchUprightMPC(B, torch.float32, plant_mode=1), BatchUprightMPC(B, torch.float32, plant_mode=1)
    for h in (one, many):
        h.set_state(st, ref)
    one.set_impulses(tab)
    one.rollout(K)
    assert one.kernel_name == "umpc_rollout_asm_kernel" and one.impulse_cursor == K
    for k in range(K):
        _step_and_add(many, tab, k)
    _final_equal(one, many, "B = 65536")


@pytest.mark.gpu
@pytest.mark.parametrize("plant", [0, 1], ids=["plant0", "rk4"])
@pytest.mark.parametrize("name,dtype,mode", HIST_MODES, ids=HIST_MODE_IDS)
def test_table_rollout_matches_the_oracle_chain(oracle_built, name, dtype, mode, plant):
    """the same launch against oraclebind.batch_rollout(K = 1) chained with t0 advanced and the add in between, all 128 robots,
    with the margins of _check_against_oracle"""
    import torch
    from robobee3d_amd import _lib
    from robobee3d_amd.batch import hover_initial_conditions
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    B, K = 128, 8
    st, ref = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    kick = _kicks(K, B, 4)
    s_o, out_o, _ = _oracle_chain(oracle_built, perm, st, ref, kick, np.float64, plant_mode=plant)
    s_o32, _, _ = _oracle_chain(oracle_built, perm, st, ref, kick, np.float32, plant_mode=plant)
    m = _handle(B, dtype, mode, plant_mode=plant)
    m.set_state(st.astype(_np_dtype(dtype)), ref.astype(_np_dtype(dtype)))
    m.set_impulses(torch.as_tensor(kick.astype(_np_dtype(dtype))))
    m.rollout(K)
    _check_against_oracle("impulses K=8 plant %d %s" % (plant, name), m, s_o, out_o, s_o32)


@pytest.mark.gpu
def test_refusals_and_cursors_with_a_handle():
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B = 64
    st, ref = hover_initial_conditions(B, 1, np.float32)
    m = BatchUprightMPC(B, torch.float32)
    m.set_state(st, ref)
    tab = torch.as_tensor(_kicks(4, B, 1, np.float32)).cuda()
    rtab = torch.as_tensor(ref)[None].repeat(8, 1, 1)
    m.set_reference_trajectory(rtab)
    m.record_history(8)
    m.set_impulses(tab, cursor0=1)
    before = m.state.clone()
    with pytest.raises(RuntimeError, match="impulse table ends"):
        m.rollout(4)                                    # 1 + 4 > 4: refused before anything is launched or copied
    torch.cuda.synchronize()
    assert torch.equal(m.state, before) and m.time_ms == 0.0
    assert (m.impulse_cursor, m.ref_cursor, m.history_cursor) == (1, 0, 0)
    m.rollout(3)
    assert (m.impulse_cursor, m.ref_cursor, m.history_cursor) == (4, 3, 3)         # three cursors, each its own
    with pytest.raises(RuntimeError, match="impulse table ends"):
        m.rollout(1)
    assert (m.impulse_cursor, m.ref_cursor, m.history_cursor) == (4, 3, 3)
    s0 = m.state.clone()
    m.update()                                          # no plant: neither applies a slice nor moves the cursor
    m.plant(m.out[0:3].clone(), 1)
    assert m.impulse_cursor == 4
    m.rewind_impulses(2)
    assert m.impulse_cursor == 2
    assert not torch.equal(m.state, s0)
    with pytest.raises(ValueError):
        m.set_impulses(torch.zeros((4, 6, B + 1)))
    with pytest.raises(ValueError):
        m.set_impulses(torch.zeros((4, 5, B)))
    with pytest.raises(RuntimeError, match="umpcBatchSetImpulses"):
        m.set_impulses(tab, cursor0=5)
    with pytest.raises(RuntimeError, match="umpcBatchSetImpulses"):
        m.set_impulses(tab, cursor0=-1)
    assert m.impulse_cursor == 2                        # a refused set leaves the table that was set
    m.set_impulses(None)
    assert m.impulse_cursor == 0
    with pytest.raises(RuntimeError):
        m.rewind_impulses()
    m.set_reference_trajectory(None)
    m.record_history(None)
    m.rollout(2)                                        # off: rollouts are free again
    n0 = BatchUprightMPC(B, torch.float32, nsub=0)
    with pytest.raises(RuntimeError, match="nsub = 0"):
        n0.set_impulses(tab)
    # the reactive controller: whole closed-loop steps only, and inside the table
    r = BatchUprightMPC(B, torch.float32)
    r.set_state(st, ref)
    r.set_impulses(tab, cursor0=2)
    with pytest.raises(RuntimeError, match="multiple of nsub"):
        r.reactive_rollout(30)
    with pytest.raises(RuntimeError, match="impulse table ends"):
        r.reactive_rollout(75)
    assert r.impulse_cursor == 2 and r.time_ms == 0.0
    r.reactive_rollout(50)
    assert r.impulse_cursor == 4 and r.time_ms == pytest.approx(10.0)
    with pytest.raises(RuntimeError, match="set_impulses"):
        r.control_test_log(1.0)


@pytest.mark.gpu
def test_blocks_with_column_sliced_tables_equal_the_undivided_run():
    """partition invariance: 16 384 robots whole (fp32: quad form) and as 2 blocks of 8 192 with global_batch = 16 384; 32 768
    robots (lane form) whole and as 4 blocks -- every block kicked with its columns of the job's table (shard.impulse_block)"""
    import torch
    from robobee3d_amd import shard
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions_device
    K = 4
    for B, W, kernel in ((16384, 2, "umpc_rollout_asm_quad_kernel"), (32768, 4, "umpc_rollout_asm_kernel")):
        whole = BatchUprightMPC(B, torch.float32, plant_mode=1)
        st, ref, _ = hover_initial_conditions_device(B, 20201118, torch.float32)
        whole.set_state(st, ref)
        # a push-time x push-direction sweep: robot b is pushed once, at step b % K, along direction (b // K) % 3
        b = np.arange(B)
        ev = [(k, b[(b % K == k) & ((b // K) % 3 == d)], np.eye(6)[d] * DV) for k in range(K) for d in range(3)]
        tab = whole.impulse_table(K, ev)
        assert int((tab != 0).sum()) == B
        whole.set_impulses(tab)
        whole.rollout(K)
        assert whole.kernel_name == kernel
        for rank in range(W):
            lo, hi = shard.split_range(B, rank, W)
            blk = BatchUprightMPC(hi - lo, torch.float32, plant_mode=1, global_batch=B)
            blk.set_state(st[:, lo:hi], ref[:, lo:hi])
            blk.set_impulses(shard.impulse_block(tab, lo, hi))
            blk.rollout(K)
            assert blk.kernel_name == kernel
            for x, y in ((blk.state, whole.state), (blk.ctrl, whole.ctrl), (blk.out, whole.out), (blk.stats, whole.stats),
                         (blk.info, whole.info)):
                assert torch.equal(x, y[:, lo:hi])
            assert torch.equal(blk.status, whole.status[lo:hi])


@pytest.mark.gpu
def test_reactive_rollout_honours_the_table(oracle_built):
    """umpcBatchReactive with a table against oraclebind.reactive_rollout chained in blocks of nsub with t0 advanced and the add
    in between: slice cursor + j lands after substep (j + 1) * nsub - 1. Margins of tests/test_reactive.py."""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    B, K, nsub = 100, 8, 25
    kick = _kicks(K, B, 21)
    gains = np.tile(np.array([[5e-3], [5e-1], [1e-1], [1e0], [10e0], [1e2]]), (1, B))
    for tdt, ndt, tol in ((torch.float64, np.float64, 1e-9), (torch.float32, np.float32, 2e-3)):
        st, ref = hover_initial_conditions(B, 7, ndt)
        mpc = BatchUprightMPC(B, tdt, taulim=10.0)
        mpc.set_state(st, ref)
        mpc.set_impulses(torch.as_tensor(kick.astype(ndt)))
        mpc.reactive_rollout(3 * nsub, gains)
        mpc.reactive_rollout(5 * nsub, gains)
        torch.cuda.synchronize()
        assert mpc.impulse_cursor == K and mpc.time_ms == pytest.approx(K * nsub * 0.2)
        so = st.astype(np.float64)
        ro = np.ascontiguousarray(ref, np.float64)
        stats = np.zeros((2, B))
        for j in range(K):
            _, s_j, _ = oracle_built.reactive_rollout(so, ro, nsub, 1, gains, taulim=10.0, t0=j * nsub * 0.2)
            stats += s_j
            so[12:18] += kick[j]
        got = mpc.state.cpu().numpy().astype(np.float64)
        scale = np.maximum(1.0, np.abs(so))
        err = np.max(np.abs(got - so) / scale)
        record_margin("reactive + impulses %s" % str(tdt)[6:], "max |d state| / max(1, |s|)", err, tol)
        assert err < tol, tdt
        assert np.allclose(mpc.stats.cpu().numpy(), stats, rtol=max(tol, 1e-8) * 10)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_reference_push_log_through_one_launch(dtype):
    """tests/golden/impulse_log.npz through ONE nsub = 1 launch of 200 steps with a one-slice-non-zero table and a state history
    (plant mode 0, helix task: the reference loop), compared with the reference log's y. The reference's controller is fp32 C, so
    the tolerance is not fixed in advance: the un-kicked run of the same launch (the parent can produce it) is measured against
    the un-kicked log, and the kicked run may deviate FOUR times as far -- after the push the trajectories separate at the
    solver's 50-iteration sensitivity, not at round-off.
    The test prints both figures and the bound ("PUSH-LOG ..."). They have NOT been measured on an MI355X yet, and
    profiles/impulses_parity.txt is not written; on the CPU the fp64 oracle chain gives 0.314 un-kicked and 0.217 kicked."""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    g, n, kt, st, ref, kick, task_p = _fixture_setup()
    tdt, ndt = getattr(torch, dtype), _np_dtype(dtype)
    ys = {}
    for what, tab in (("plain", None), ("kick", kick)):
        m = BatchUprightMPC(1, tdt, nsub=1, plant_mode=0)
        m.set_state(st.astype(ndt), ref.astype(ndt))
        m.set_task("helix", trajAmp=task_p[0], trajFreq=task_p[1], dz=task_p[2], useY=bool(task_p[3]))
        if tab is not None:
            m.set_impulses(torch.as_tensor(tab.astype(ndt)))
        m.record_history(n, out=False)
        m.rollout(n)
        ys[what] = _log_y(m.history()["state"].to(torch.float64).cpu().numpy(), None if tab is None else tab.astype(ndt))
    d0 = np.abs(ys["plain"] - g["plain_y"]).max()
    d1 = np.abs(ys["kick"] - g["kick_y"]).max()
    print("PUSH-LOG %s: un-kicked max |dy| %.6e, kicked max |dy| %.6e, bound 4 x un-kicked = %.6e" % (dtype, d0, d1, 4 * d0))
    record_margin("push log, one launch " + dtype, "kicked max |dy| vs reference", d1, 4 * d0, "un-kicked %.3e" % d0)
    assert np.array_equal(ys["plain"][:kt - 1], ys["kick"][:kt - 1])
    assert d1 <= 4 * d0, (dtype, d0, d1)


@pytest.mark.gpu
def test_control_test_log_applies_impulses_ahead_of_the_fire():
    """the logging path on the fixed schedule with nsub = 1 and impulses={kick_ti: kick} is the reference's loop too: it equals
    the history of the one-launch run (fp64: the same kernels' arithmetic per substep, to round-off of the separate plant launch)"""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    g, n, kt, st, ref, kick, task_p = _fixture_setup()
    m = BatchUprightMPC(1, torch.float64, nsub=1, plant_mode=0)
    m.set_state(st, ref)
    m.set_task("helix", trajAmp=task_p[0], trajFreq=task_p[1], dz=task_p[2], useY=bool(task_p[3]))
    lg = m.control_test_log(n * 0.2, impulses={kt: g["kick"]})[0]
    a = BatchUprightMPC(1, torch.float64, nsub=1, plant_mode=0)
    a.set_state(st, ref)
    a.set_task("helix", trajAmp=task_p[0], trajFreq=task_p[1], dz=task_p[2], useY=bool(task_p[3]))
    a.set_impulses(torch.as_tensor(kick))
    a.record_history(n, out=False)
    a.rollout(n)
    y = _log_y(a.history()["state"].cpu().numpy(), kick)
    np.testing.assert_allclose(lg["y"], y, rtol=1e-7, atol=1e-9)
