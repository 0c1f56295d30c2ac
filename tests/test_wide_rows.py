"""WIDE ROWS of the fp32 lane step (asmstep.py): x, y, z between the steps of one launch -- words only the stream itself reads
back -- live in `ws` in groups of four words per lane, one four-word access per group.

CPU: the interpreter (asmstep.simulate) runs the shipped stream and StepGen(narrow_rows=True), the stream with x, y, z on their
public rows on every step, on the same inputs: raw bits of every public word. A K-step launch against K chained one-step launches is the check that the
private hand-off of the iterates is complete. Instruction counts come from the executed-instruction counters of a middle step.
GPU: K steps in one launch against K launches of one step (bits) and against the fp32 oracle (the margins of
tests/test_gpu_parity.py for the same quantities), lane form forced at small B."""
import functools

import numpy as np
import pytest

from robobee3d_amd import asmgen, asmstep
from robobee3d_amd.batch import hover_initial_conditions, monte_carlo_draws

PUBLIC = ("state", "ctrl", "out", "stats", "status", "info")
DEFAULT_W = np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])          # rows ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom
# short steps for the option matrix: the accesses under test do not depend on the iteration or substep count
SHORT = dict(maxIter=12, nsub=3)


@pytest.fixture(scope="module")
def streams():
    wide, narrow = asmstep.StepGen(), asmstep.StepGen(narrow_rows=True)
    return (wide, wide.program()), (narrow, narrow.program())


def _wave(st, ref, n=1, **opt):
    """the arrays of robots 0 .. n - 1 as the lanes of one wavefront ([rows][lanes]); opt: per-robot tables [rows][B] / flat"""
    f = np.float32
    a = dict(state=np.array(st[:, :n], f, order="C"), ctrl=np.zeros((127, n), f), ref=np.array(ref[:, :n], f, order="C"),
             ws=np.zeros((asmgen.WS_ROWS, n), f), out=np.zeros((9, n), f), stats=np.zeros((2, n), f),
             status=np.zeros((1, n), np.int32), info=np.zeros((2, n), f))
    a["ctrl"][124:] = 1
    for k, t in opt.items():
        t = np.asarray(t, f)
        a[k] = np.ascontiguousarray(t) if k in asmstep.FLAT else np.array(t.reshape(t.shape[0], -1)[:, :n], f, order="C")
    return a


def _run(stream, a, K, fl=None, plant=1, maxIter=50, nsub=25):
    g, ins = stream
    asmstep.simulate(ins, a, dict(K=K, maxIter=maxIter, nsub=nsub, plant=plant), fl or asmstep.host_floats(),
                     lanes=a["state"].shape[1], hits=True, max_exec=10 ** 7)
    return asmstep.simulate.last_hits.copy()


def _same_public_bits(a, b, what):
    for n in PUBLIC + tuple(k for k in ("wlu", "wlw") if k in a):
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), (what, n)


def _copy(a):
    return {k: v.copy() for k, v in a.items()}


def _options():
    """name -> (arrays of one robot, simulate keywords): the options tests/test_asm_step.py covers"""
    from conftest import golden
    from test_asm_step import _wldev_words
    from test_wl_step import _args, _loop_inputs
    st, ref = hover_initial_conditions(2, 20201118, np.float32)
    Ib, gain = monte_carlo_draws(2, 20201120, np.float64)
    W = np.tile(DEFAULT_W[:, None], (1, 2))
    W[2], W[4] = [0.02, 7.0], [30.0, 8e3]
    # a task table of 4 steps: (dp[3], dpdes[3], sdes_x, sdes_z) per step, any smooth values (both streams read the same)
    tab = np.array([[0.1 * k, -0.05 * k, 0.02 * k, 0.01, -0.005, 0.002, 0.05 * np.sin(k), 1.0] for k in range(4)], np.float32)
    gl = golden("mpc_wl_loop.npz")
    stw, refw, _, u4 = _loop_inputs(gl, np.float64, 1)
    wl = _wldev_words(_args(gl), (100.0, 100.0, 100.0, 3333.0, 3333.0, 1000.0))
    return {
        "plain": (_wave(st, ref), {}),
        "monte_carlo": (_wave(st, ref, Ib=Ib, gain=gain[None, :]), {}),
        "weights": (_wave(st, ref, weights=W), {}),
        "task_table": (_wave(st, ref, taskf=tab), {}),
        "fused_wl": (_wave(stw, refw, wl=wl, wlu=u4, wlw=np.zeros((6, 1))), {}),
        "euler_plant": (_wave(st, ref), dict(plant=0)),
        "controller_only": (_wave(st, ref, aT0=np.array([[0.0123]])), dict(nsub=0)),
    }


OPTIONS = ("plain", "monte_carlo", "weights", "task_table", "fused_wl", "euler_plant", "controller_only")


@pytest.fixture(scope="module")
def options():
    return _options()


@pytest.mark.parametrize("name", OPTIONS)
def test_public_words_equal_the_narrow_stream(streams, options, name):
    """K = 1, 2, 3, 4, every option: state, ctrl (all 127 rows), out, stats, status, info (and the WL state rows) bit for bit"""
    a0, kw = options[name]
    kw = dict(SHORT, **kw)
    for K in (1, 2, 3, 4):
        got = []
        for stream in streams:
            a = _copy(a0)
            _run(stream, a, K, **kw)
            got.append(a)
        _same_public_bits(got[0], got[1], (name, K))
        assert np.isfinite(got[0]["out"]).all() and int(got[0]["status"][0, 0]) != 0


def test_full_length_steps_and_the_chain_of_single_steps(streams):
    """50 iterations, 25 substeps, two lanes of one wavefront. K = 3 in one launch == the narrow stream == three chained
    launches of one step, `ctrl` included: what step k + 1 reads from the groups is what step k would have left on the
    public rows."""
    st, ref = hover_initial_conditions(2, 20201118, np.float32)
    wide, narrow = streams
    a, b, c = (_wave(st, ref, 2) for _ in range(3))
    _run(wide, a, 3)
    _run(narrow, b, 3)
    for _ in range(3):
        _run(wide, c, 1)
    _same_public_bits(a, b, "wide vs narrow")
    _same_public_bits(a, c, "one launch vs chain")


@pytest.mark.parametrize("name", ["plain", "fused_wl", "euler_plant"])
def test_chain_of_single_steps_with_options(streams, options, name):
    a0, kw = options[name]
    kw = dict(SHORT, **kw)
    a, c = _copy(a0), _copy(a0)
    _run(streams[0], a, 3, **kw)
    for _ in range(3):
        _run(streams[0], c, 1, **kw)
    _same_public_bits(a, c, name)


def test_ruiz_restart_inside_a_launch(streams):
    """wvf = 1e14 (tests/test_ruiz_fast_path.py) fails the Ruiz speculation, so every step of the launch -- step 2 of 3 among
    them -- starts again through the exact body. The restart lies ahead of the load of the iterates: the restarted step
    reads the groups step 1 left, and the launch equals the narrow stream and the chain bit for bit."""
    st, ref = hover_initial_conditions(1, 3, np.float32)
    fl = asmstep.host_floats(wvf=1e14)
    wide, narrow = streams
    a, b, c = (_wave(st, ref) for _ in range(3))
    h = _run(wide, a, 3, fl, **SHORT)
    assert int(h[wide[0].restart_at]) == 3
    _run(narrow, b, 3, fl, **SHORT)
    for _ in range(3):
        _run(wide, c, 1, fl, **SHORT)
    _same_public_bits(a, b, "wide vs narrow")
    _same_public_bits(a, c, "one launch vs chain")


def test_cold_start_inside_a_launch(streams):
    """A NaN in the angular rate of lane 1: no solution, the lane's x, y, z are zeroed -- in the groups on steps 1 and 2, on the
    public rows on step 3 -- while lane 0 runs on untouched. Raw bits, NaN payloads included."""
    st, ref = hover_initial_conditions(2, 3, np.float32)
    wide, narrow = streams
    a, b, c = (_wave(st, ref, 2) for _ in range(3))
    for x in (a, b, c):
        x["state"][16, 1] = np.nan
    _run(wide, a, 3, **SHORT)
    _run(narrow, b, 3, **SHORT)
    for _ in range(3):
        _run(wide, c, 1, **SHORT)
    _same_public_bits(a, b, "wide vs narrow")
    _same_public_bits(a, c, "one launch vs chain")
    assert int(a["status"][0, 1]) == -7 and not a["ctrl"][:123, 1].any()
    assert int(a["status"][0, 0]) != -7 and a["ctrl"][:123, 0].any() and np.isfinite(a["state"][:, 0]).all()


def test_hazards_budget_and_size(streams):
    (g, ins), _ = streams
    real = [t for t in ins if t[0] not in asmstep.PSEUDO and t[0] != "label"]
    # with and without the interpreter's markers between the instructions
    assert asmgen.wide_store_hazards(ins) == [] and asmgen.wide_store_hazards([t for t in ins if t[0] not in asmstep.PSEUDO]) == []
    assert g.pool.peak <= 254 and len(real) < 12000                       # tests/test_asm_step.py test_register_budget_and_size
    for t in real:
        if t[0].startswith("global_") and t[0].endswith(("x2", "x4")):
            data = t[1] if t[0].startswith("global_load") else t[2]
            assert min(asmgen._vgprs(data)) % 2 == 0, t                  # wide VMEM data starts on an even register


def _is_ptr(t, name):
    return t[0].startswith("global_") and t[3] == asmstep.sp(asmstep.S_PTR[name])


def test_instruction_counts_of_a_middle_step(streams):
    """executed instructions of step 2 of 3 = counters of a K = 3 launch minus those of a K = 2 launch (first and last step
    take the same paths in both)"""
    st, ref = hover_initial_conditions(1, 20201118, np.float32)
    mid = {}
    for key, stream in zip(("wide", "narrow"), streams):
        h3 = _run(stream, _wave(st, ref), 3, **SHORT)
        h2 = _run(stream, _wave(st, ref), 2, **SHORT)
        mid[key] = h3 - h2
    (g, ins), (_, ins_n) = streams
    in_spans = lambda k, spans: any(lo <= k < hi for lo, hi in spans)
    ws = [k for k, t in enumerate(ins) if _is_ptr(t, "ws")]
    iterates = sum(int(mid["wide"][k]) for k in ws if in_spans(k, g.group_spans))
    assert iterates == 2 * len(asmstep.WIDE_ITER) == 64
    # the parked D, E rows are what they were: 66 + 66 one-word accesses (nine D words and c sit in spare AGPRs)
    assert sum(int(mid["wide"][k]) for k in ws if not in_spans(k, g.group_spans)) == 2 * (45 - asmstep.N_SPARE_D + 39)
    # the public x, y, z rows of ctrl: every access lies in a recorded span, and a middle step executes none of them
    ctrl = [k for k, t in enumerate(ins) if _is_ptr(t, "ctrl")]
    assert sum(1 for k in ctrl if in_spans(k, g.public_spans)) == 3 * 123                 # load, store, cold start
    assert sum(int(mid["wide"][k]) for k in ctrl if in_spans(k, g.public_spans)) == 0
    # ... what is left on ctrl per step: T0 (read twice, written twice) and the three thrust-row E words (read, written)
    assert sum(int(mid["wide"][k]) for k in ctrl) == 10
    vmem = {key: sum(int(mid[key][k]) for k, t in enumerate(i_) if t[0].startswith("global_"))
            for key, i_ in (("wide", ins), ("narrow", ins_n))}
    print("VMEM instructions of a middle step: narrow %d, wide %d" % (vmem["narrow"], vmem["wide"]))
    assert vmem["narrow"] - vmem["wide"] == (123 - 32) * 2


def test_first_and_only_step_issues_the_public_accesses(streams):
    """K = 1: the x, y, z rows are read and written on their public rows, no group of the iterates is touched"""
    st, ref = hover_initial_conditions(1, 20201118, np.float32)
    g, ins = streams[0]
    h = _run(streams[0], _wave(st, ref), 1, **SHORT)
    in_spans = lambda k, spans: any(lo <= k < hi for lo, hi in spans)
    assert sum(int(h[k]) for k, t in enumerate(ins) if _is_ptr(t, "ctrl") and in_spans(k, g.public_spans)) == 2 * 123
    assert sum(int(h[k]) for k, t in enumerate(ins) if _is_ptr(t, "ws") and in_spans(k, g.group_spans)) == 0


def test_the_parked_rows_keep_their_layout(streams):
    """one lane: D (columns 9..44) and E stay on rows 9..83 behind the `ws` pointer, as tests/test_asm_quad.py compares them
    with the quad stream's; the groups of the iterates start behind row 84"""
    st, ref = hover_initial_conditions(1, 20201118, np.float32)
    a, b = _wave(st, ref), _wave(st, ref)
    _run(streams[0], a, 3, **SHORT)
    _run(streams[1], b, 3, **SHORT)
    assert np.array_equal(a["ws"].view(np.uint32), b["ws"].view(np.uint32))
    assert a["ws"][asmstep.N_SPARE_D:asmgen.WS_C - asmgen.WS_DS].all() and not a["ws"][asmgen.WS_C - asmgen.WS_DS:].any()
    assert 4 * asmstep.WIDE_FIRST > asmgen.WS_C - asmgen.WS_DS
    # two lanes: the array is contiguous and the groups land in it, behind the rows
    st, ref = hover_initial_conditions(2, 20201118, np.float32)
    c = _wave(st, ref, 2)
    _run(streams[0], c, 2, **SHORT)
    assert c["ws"][4 * asmstep.WIDE_FIRST:asmstep.WIDE_ROWS].any() and not c["ws"][asmstep.WIDE_ROWS:].any()
    assert not c["ws"][asmgen.WS_C - asmgen.WS_DS:4 * asmstep.WIDE_FIRST].any()


# ----------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------
TOL_T, TOL_A = 3e-5, 3e-5          # tests/test_gpu_parity.py


@functools.lru_cache(maxsize=None)
def _oracle(B, K):
    """the fp32 oracle's K closed-loop steps of the B robots (same elimination order, RK4 plant): state, out, stats"""
    import oraclebind
    from robobee3d_amd import _lib
    oraclebind.build()
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    s, c = st.copy(), np.zeros((127, B), np.float32)
    c[124:] = 1
    out, stats, status = oraclebind.batch_rollout(s, c, ref.copy(), K, dtype=np.float32, perm=perm, plant_mode=1)
    return s, out, stats


@pytest.mark.gpu
@pytest.mark.parametrize("hist", [False, True], ids=["inplace", "history"])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("B", [64, 100, 192])
def test_gpu_one_launch_equals_single_step_launches_and_the_oracle(B, K, hist, margin):
    """lane form forced by global_batch = 65 536: one K-step launch against K one-step launches, bit for bit in every public
    array (and in the recorded history), then against the fp32 oracle"""
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    assert torch.cuda.is_available(), "these tests need the MI355X"
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    runs = []
    for launches in ((K,), (1,) * K):
        m = BatchUprightMPC(B, torch.float32, global_batch=65536, plant_mode=1)
        m.set_state(st, ref)
        if hist:
            m.record_history(K, state=True, out=True, status=True, info=True)
        for k in launches:
            m.rollout(k)
        torch.cuda.synchronize()
        assert m.kernel_name == "umpc_rollout_asm_kernel"
        got = {n: getattr(m, n).cpu().numpy() for n in PUBLIC}
        if hist:
            got.update({"hist_" + n: t.cpu().numpy() for n, t in m.history().items()})
        runs.append(got)
    for n in runs[0]:
        assert np.array_equal(runs[0][n].view(np.uint32), runs[1][n].view(np.uint32)), n
    s_o, out_o, stats_o = _oracle(B, K)
    s, out = runs[0]["state"].astype(np.float64), runs[0]["out"].astype(np.float64)
    assert np.isfinite(s).all()
    margin("|dp| mm", np.abs(s[0:3] - s_o[0:3]).max(), 1.5e-3)
    margin("|dR|, |ddq|", np.abs(s[3:] - s_o[3:]).max(), 3e-4)
    margin("|d thrust|", np.abs(out[0] - out_o[0]).max(), TOL_T)
    margin("|d moment| / max(2e-2, 1e-3 |u|)", (np.abs(out[1:3] - out_o[1:3]) / np.maximum(2e-2, 1e-3 * np.abs(out_o[1:3]))).max(), 1.0)
    margin("|d accdes|", np.abs(out[3:] - out_o[3:]).max(), TOL_A)
    np.testing.assert_allclose(runs[0]["stats"], stats_o, rtol=1e-3)
