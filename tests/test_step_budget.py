"""The instruction budget of the two fp32 step streams, and the bit-identity of what was cut (CPU, interpreter only).

A lone wavefront pays per EXECUTED instruction, so a step's time is a count, and the counts are pinned here:
the lane stream with the RK4 substep on the paired register layout (asmstep.StepGen.plant, _rk4_packed), the quad stream with
Ruiz passes that never switch EXEC and speculate like the lane form's (ruiz_quad). tests/test_asm_quad.py holds the quad stream
under 0.55 of the lane stream, so a cut in the lane stream needs its share in the quad stream: for a lane cut of d1 and a
quad-only cut of q per step, q > 0.55 d1 - 47. The ratio asserted here is the one both streams had before these cuts.

Every cut must leave every bit: the lane stream is compared with StepGen(scalar_rk4=True), the quad stream with
StepGen(quad=True, exact_ruiz=True) -- the streams before the cuts, which the generator still emits."""
import numpy as np
import pytest

from robobee3d_amd import asmgen, asmstep, isasim
from robobee3d_amd.batch import hover_initial_conditions, monte_carlo_draws
from conftest import golden
from test_asm_step import _arrays

WORDS = ("state", "ctrl", "out", "stats", "status", "info", "ws")
RUN = dict(maxIter=50, nsub=25, plant=1)


@pytest.fixture(scope="module")
def lane():
    new, old = asmstep.StepGen(), asmstep.StepGen(scalar_rk4=True)
    return (new, new.program()), (old, old.program())


@pytest.fixture(scope="module")
def quad():
    new, old = asmstep.StepGen(quad=True), asmstep.StepGen(quad=True, exact_ruiz=True)
    return (new, new.program()), (old, old.program())


def _same_bits(a, b, what=""):
    for n in a:
        if a[n] is not None:
            assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), (what, n)


# ---- executed counts --------------------------------------------------------------------------------------------------
def test_executed_counts_per_step(lane, quad):
    """K = 1, robot 0 of the hover draw, 50 iterations, 25 substeps. Bounds: the lane stream 1 000 below the 55 874 it
    executed with the scalar substep; the quad stream below the 30 636 of the EXEC-masked, exact-only passes by the selects
    (330) and the speculation (another 406); the ratio no higher than those two had, 0.5483; a substep at most 186."""
    (g1, ins1), (g4, ins4) = lane[0], quad[0]
    st, ref = hover_initial_conditions(4, 20201118, np.float32)
    fl = asmstep.host_floats()
    n1 = asmstep.simulate(ins1, _arrays(st, ref, 0), dict(K=1, **RUN), fl, hits=True)
    h = asmstep.simulate.last_hits
    n4 = asmstep.simulate(ins4, _arrays(st, ref, 0), dict(K=1, **RUN), fl)
    sub = int(h[g1.rk4_span[0]:g1.rk4_span[1]].sum())
    print("lane %d, quad %d, ratio %.4f, substep %.1f" % (n1, n4, n4 / n1, sub / RUN["nsub"]))
    assert n1 <= 54874, n1
    assert n4 <= 29900, n4
    assert n4 / n1 <= 0.5483, (n1, n4)
    assert sub % RUN["nsub"] == 0 and sub // RUN["nsub"] <= 186, sub
    # the streams before the cuts are still what they were
    assert asmstep.simulate(lane[1][1], _arrays(st, ref, 0), dict(K=1, **RUN), fl) == 55874
    assert asmstep.simulate(quad[1][1], _arrays(st, ref, 0), dict(K=1, **RUN), fl) == 30636


def test_the_restart_flag_is_dead_where_the_quad_stream_uses_it(quad):
    """S_EXACT is s14, the ADMM counter and half of a phase C mask: from the top of a step to the end of the Ruiz section
    no instruction of the quad stream names it but the ones that set and test the flag."""
    g, ins = quad[0]
    top = ins.index(("label", g.lab_restart))
    end = next(k for k in range(ins.index(("quad_begin", "ruiz")), len(ins)) if ins[k][0] == "quad_end")
    assert ins[top - 1] == ("s_mov_b32", "s%d" % asmstep.S_EXACT, 0)
    named = [t for t in ins[top:end] if any(("s", asmstep.S_EXACT) in isasim._regs(x) for x in t[1:] if isinstance(x, str))]
    flag = "s%d" % asmstep.S_EXACT
    assert named and all(t in (("s_mov_b32", flag, 1), ("s_cmp_eq_u32", flag, 0)) for t in named), named
    assert sum(1 for t in named if t[0] == "s_mov_b32") == 2          # the finite guard and the failed range test


def test_the_comparison_streams_are_the_ones_before_the_cuts(lane, quad):
    """a guard against a cut leaking into the streams the shipped ones are compared with: the text lines the two headers
    held before (labels included), a scalar substep of 226 instructions, and EXEC-masked maxima in the quad passes"""
    (g1, ins1), (g4, ins4) = lane[1], quad[1]
    assert len([t for t in ins1 if t[0] not in asmstep.PSEUDO]) == 10037
    assert len([t for t in ins4 if t[0] not in asmstep.PSEUDO]) == 10529
    span = [t for t in ins1[g1.rk4_span[0]:g1.rk4_span[1]] if t[0] != "label"]
    assert len(span) == 226 and sum(1 for t in span if t[0].startswith("v_pk_")) == 63
    qb = ins4.index(("quad_begin", "ruiz"))
    lab = next(k for k in range(qb, len(ins4)) if ins4[k][0] == "label")
    end = next(k for k in range(lab, len(ins4)) if ins4[k][0] == "s_cbranch_scc1")
    assert sum(1 for t in ins4[lab:end] if t[0] == "s_mov_b64" and t[1] == "exec") == 20 and end - lab == 386


# ---- lane form: the packed substep against the scalar one ---------------------------------------------------------------
def _wave(st, ref, n, **opt):
    f = np.float32
    a = dict(state=np.array(st[:, :n], f, order="C"), ctrl=np.zeros((127, n), f), ref=np.array(ref[:, :n], f, order="C"),
             ws=np.zeros((asmgen.WS_ROWS, n), f), out=np.zeros((9, n), f), stats=np.zeros((2, n), f),
             status=np.zeros((1, n), np.int32), info=np.zeros((2, n), f))
    a["ctrl"][124:] = 1
    a.update(opt)
    return a


def _lane_case(name):
    B = 64
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    opt, ints = {}, dict(K=3, **RUN)
    if name == "monte-carlo":
        Ib, gain = monte_carlo_draws(B, 7, np.float32)
        opt = dict(Ib=np.array(Ib, np.float32, order="C"), gain=np.array(gain, np.float32).reshape(1, B))
    elif name == "impulses":
        rng = np.random.default_rng(11)
        kick = rng.normal(size=(3, 6, B)) * np.array([0.05, 0.05, 0.05, 1e-3, 1e-3, 1e-3])[None, :, None]
        opt = dict(impulse=np.ascontiguousarray(kick.reshape(18, B), np.float32))
    elif name == "nsub1":
        ints["nsub"] = 1
    elif name == "euler":
        ints["plant"] = 0
    return st, ref, opt, ints


@pytest.mark.parametrize("name", ["hover", "monte-carlo", "impulses", "nsub1", "euler"])
def test_lane_stream_equals_the_scalar_substep_bit_for_bit(lane, name):
    """64 lanes of one wavefront, K = 3: the hover tilts; per-robot Ib and thrust gain (the packed Ib w and Ib^-1 products
    read them as pairs); an impulse table (added to dq through the layout's map); one substep per step; and plant mode 0,
    the Euler + expm step, which shares the layout's registers and must keep its bits. Every public array and the
    workspace, raw bits."""
    st, ref, opt, ints = _lane_case(name)
    got = []
    for g, ins in lane:
        a = _wave(st, ref, 64, **{k: x.copy() for k, x in opt.items()})
        asmstep.simulate(ins, a, ints, asmstep.host_floats(), lanes=64, max_exec=10 ** 7)
        got.append(a)
    _same_bits(got[0], got[1], name)
    assert np.isfinite(got[0]["state"]).all() and got[0]["state"].any()


def test_paired_layout_is_a_permutation_and_wide_data_stays_even(lane):
    """the substep's packed instructions name aligned pairs only (an odd base does not assemble), and the pool's peak holds"""
    g, ins = lane[0]
    assert g.pool.peak <= 254
    span = ins[g.rk4_span[0]:g.rk4_span[1]]
    packed = [t for t in span if t[0].startswith("v_pk_")]
    assert len(packed) >= 63 + 4 * 9
    for t in packed:
        for x in t[1:-1]:
            kind, lo, n = isasim._decode(x)[:3]
            assert n == 2 and lo % 2 == 0, t
    real = [t for t in ins if t[0] not in asmstep.PSEUDO and t[0] != "label"]
    assert len(real) < 12000


# ---- quad form: selects and speculation against the EXEC-masked, exact-only passes ---------------------------------------
def _quad_pair(quad, a_of, ints, fl=None):
    got = []
    for g, ins in quad:
        a = a_of()
        n = asmstep.simulate(ins, a, ints, fl or asmstep.host_floats(), max_exec=10 ** 7)
        got.append((a, n, dict(asmstep.simulate.last_quad_sections)))
    return got


def test_quad_stream_equals_the_exact_masked_passes_bit_for_bit(quad):
    """4 robots x K = 2 (50 iterations, 25 substeps): all arrays, NaN payloads included; no restart (the stream is shorter
    than the exact-only one by more than 1 400 executed instructions per robot), and EXEC is never switched inside a pass"""
    st, ref = hover_initial_conditions(4, 20201118, np.float32)
    for b in range(4):
        (a, n, sec), (ax, nx, secx) = _quad_pair(quad, lambda: _arrays(st, ref, b), dict(K=2, **RUN))
        _same_bits(a, ax, b)
        assert nx - n > 1400 and sec["ruiz"] > 2 * 3000, (n, nx, sec)
    g, ins = quad[0]
    qb = ins.index(("quad_begin", "ruiz"))
    qe = next(k for k in range(qb, len(ins)) if ins[k][0] == "quad_end")
    first = next(k for k in range(qb, qe) if ins[k][0] == "label")
    last = max(k for k in range(qb, qe) if ins[k][0].startswith("s_cbranch") and ins[k][1].endswith("b"))
    assert not any(t[0] == "s_mov_b64" and t[1] == "exec" for t in ins[first:last])


@pytest.mark.parametrize("kw,restart", [(dict(wvf=5e5, wmom=2e-5), False), (dict(wvf=1e14), True)], ids=["pass1", "pass2"])
def test_quad_out_of_range_weights(quad, kw, restart):
    """The weights of test_limit_scaling_exact_path are out of limit_scaling's range in pass 1 only, which is always exact:
    no restart. wvf = 1e14 is still out of range in pass 2: the step is run again through ten exact passes, which shows in
    the executed count (a restarted step executes its phase A and its passes twice). Equal bits either way."""
    st, ref = hover_initial_conditions(1, 3, np.float32)
    (a, n, _), (ax, nx, _) = _quad_pair(quad, lambda: _arrays(st, ref, 0), dict(K=2, **RUN), asmstep.host_floats(**kw))
    _same_bits(a, ax, kw)
    assert (n > nx + 2 * 2000) if restart else (n < nx), (n, nx)
    assert np.isfinite(a["out"]).all()


def test_quad_restart_from_the_per_robot_weights_table(quad):
    """the same through the weights table (the gain-sweep option), one step"""
    st, ref = hover_initial_conditions(1, 3, np.float32)
    W = np.array([[1e1], [1e3], [1], [5], [1e3], [1e14], [1e-1], [1e-2]], np.float32)
    (a, n, _), (ax, nx, _) = _quad_pair(quad, lambda: _arrays(st, ref, 0, weights=W), dict(K=1, **RUN))
    _same_bits(a, ax)
    assert n > nx + 2000, (n, nx)


def test_quad_nan_branch_inputs(quad):
    """the twelve calls of tests/golden/nan_branch.npz, one controller step each (no plant): calls 4 and 9 see a state of 1e33
    and end with status -7; every word of every call equals the exact-only stream's, NaN payloads included (whichever of
    the guard, the restart or the fast body a call takes)."""
    seq = golden("nan_branch.npz")
    n, maxIter = len(seq["p0"]), int(seq["maxIter"])
    f = np.float32
    state = np.zeros((18, n), f)
    state[0:3], state[12:18] = seq["p0"].T, seq["dq0"].T
    state[3:12] = seq["R0"].transpose(2, 1, 0).reshape(9, n)
    ref = np.vstack((seq["pdes"].T, seq["dpdes"].T, seq["sdes"].T)).astype(f)
    ctrl = np.vstack((seq["pre_x"].T, seq["pre_y"].T, seq["pre_z"].T, seq["pre_T0"][None, :], seq["pre_E3"].T)).astype(f)
    aT0 = seq["actualT0"].astype(f)
    status = []
    for b in range(n):
        def a_of():
            a = _arrays(state, ref, b, aT0=aT0)
            a["ctrl"] = ctrl[:, b].copy()
            return a
        (a, cnt, _), (ax, cntx, _) = _quad_pair(quad, a_of, dict(K=1, maxIter=maxIter, nsub=0, plant=1))
        _same_bits(a, ax, b)
        status.append(int(a["status"][0]))
    assert [k for k, s_ in enumerate(status) if s_ == -7] == [4, 9], status
