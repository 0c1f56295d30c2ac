"""The Ruiz speculation of the fp32 lane step (asmstep.StepGen.ruiz): passes 2..10 without limit_scaling's compare / select /
min, one wave-wide range test per step, and a restart of the step through the exact body when it fails. Everything here is the
interpreter's (asmstep.simulate) comparison of the shipped stream with the exact-only stream, StepGen(exact_ruiz=True): raw
bits of every word the kernel writes."""
import numpy as np
import pytest

from robobee3d_amd import asmgen, asmstep
from robobee3d_amd.batch import hover_initial_conditions

DEFAULT_W = np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])          # rows ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom
WORDS = ("state", "ctrl", "out", "stats", "status", "info", "ws")


@pytest.fixture(scope="module")
def streams():
    fast, exact = asmstep.StepGen(), asmstep.StepGen(exact_ruiz=True)
    return (fast, fast.program()), (exact, exact.program())


def _wave(st, ref, lo, n, weights=None):
    """the arrays of robots lo .. lo + n - 1 as the lanes of one wavefront ([rows][lanes])"""
    f = np.float32
    a = dict(state=np.array(st[:, lo:lo + n], f, order="C"), ctrl=np.zeros((127, n), f),
             ref=np.array(ref[:, lo:lo + n], f, order="C"), ws=np.zeros((asmgen.WS_ROWS, n), f), out=np.zeros((9, n), f),
             stats=np.zeros((2, n), f), status=np.zeros((1, n), np.int32), info=np.zeros((2, n), f))
    a["ctrl"][124:] = 1
    if weights is not None:
        a["weights"] = np.array(weights[:, lo:lo + n], f, order="C")
    return a


def _run(stream, a, K, fl=None, maxIter=50, nsub=25):
    """-> (restarts taken, executed instructions inside the Ruiz phase)"""
    g, ins = stream
    lanes = a["state"].shape[1]
    asmstep.simulate(ins, a, dict(K=K, maxIter=maxIter, nsub=nsub, plant=1), fl or asmstep.host_floats(), lanes=lanes,
                     hits=True, max_exec=10 ** 7)
    h = asmstep.simulate.last_hits
    return (int(h[g.restart_at]) if g.restart_at is not None else 0), int(h[g.ruiz_span[0]:g.ruiz_span[1]].sum())


def _same_bits(a, b):
    for n in WORDS:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


def test_bit_identity_with_the_exact_only_stream(streams):
    """8 robots x 2 closed-loop steps (50 iterations, 25 substeps): every word of state, ctrl, out, stats, status, info
    and the workspace equals the exact-only stream's, and no restart is taken."""
    st, ref = hover_initial_conditions(8, 20201118, np.float32)
    got = []
    for stream in streams:
        a = _wave(st, ref, 0, 8)
        got.append((a, _run(stream, a, 2)))
    _same_bits(got[0][0], got[1][0])
    assert got[0][1][0] == 0
    assert np.isfinite(got[0][0]["out"]).all()


@pytest.mark.parametrize("kw,restarts", [(dict(wvf=5e5, wmom=2e-5), 0), (dict(wvf=1e14), 2)], ids=["pass1", "pass2"])
def test_out_of_range_weights(streams, kw, restarts):
    """Weights outside limit_scaling's range, K = 2. (wvf=5e5, wmom=2e-5), the set of test_limit_scaling_exact_path, is out
    of range in pass 1 ONLY: the clamp of that pass (always the exact body) brings every later norm into (1e-4, 1e4], so
    the speculation holds and no restart is taken -- measured: 0 restarts, which is what this asserts; the weights are
    kept as a case because pass 1's clamp is the reason that pass stays exact. wvf = 1e14 is still out of range in pass 2
    (1e14 * 1e-4 (pass 1's clamped D^2) * 1e-4 (clamped c) = 1e6 > 1e4): the restart is taken once per step. Both equal
    the exact-only stream bit for bit."""
    st, ref = hover_initial_conditions(1, 3, np.float32)
    fl = asmstep.host_floats(**kw)
    got = []
    for stream in streams:
        a = _wave(st, ref, 0, 1)
        got.append((a, _run(stream, a, 2, fl)))
    _same_bits(got[0][0], got[1][0])
    assert got[0][1][0] == restarts
    assert np.isfinite(got[0][0]["out"]).all()


def test_restart_is_the_identity_on_the_clean_lanes_of_the_wavefront(streams):
    """Four lanes of one wavefront, lane 2 with wvf = 1e14 through the per-robot weights table: the whole wavefront
    restarts (once per step), and every lane, clean or not, equals the exact-only stream bit for bit."""
    st, ref = hover_initial_conditions(4, 20201118, np.float32)
    W = np.tile(DEFAULT_W[:, None], (1, 4))
    W[5, 2] = 1e14
    got = []
    for stream in streams:
        a = _wave(st, ref, 0, 4, W)
        got.append((a, _run(stream, a, 2)))
    _same_bits(got[0][0], got[1][0])
    assert got[0][1][0] == 2


@pytest.mark.parametrize("bad,word,guarded", [(np.nan, 4, True), (np.inf, 4, True), (np.nan, 16, False)],
                         ids=["nan-R", "inf-R", "nan-w"])
def test_non_finite_state(streams, bad, word, guarded):
    """A NaN, then an infinity, in one state word: raw bits equal the exact-only stream's, NaN payloads included. In a
    rotation entry (state word 4) it reaches A: the finite guard sends the step through ten exact passes, without a
    restart. In the angular rate (word 16) it reaches only the bounds, which the equilibration never reads: the fast
    body runs, and the result is the exact-only stream's all the same."""
    st, ref = hover_initial_conditions(1, 3, np.float32)
    got = []
    for stream in streams:
        a = _wave(st, ref, 0, 1)
        a["state"][word, 0] = bad
        got.append((a, _run(stream, a, 1)))
    _same_bits(got[0][0], got[1][0])
    (r_fast, n_fast), (_, n_exact) = got[0][1], got[1][1]
    assert r_fast == 0 and (n_fast > n_exact) == guarded      # guarded: the guard's instructions on top of ten exact passes
    assert int(got[0][0]["status"][0, 0]) == -7


def _gain_grid_weights(B):
    """bench.gain_grid_weights: the 10 x 10 (wpr, wvr) grid of template/uprightmpc2.py:272-303"""
    g1, g2 = np.meshgrid(np.logspace(-2, 1, 10), np.logspace(1, 4, 10))
    W = np.tile(DEFAULT_W[:, None], (1, B))
    W[2], W[4] = np.resize(g1.ravel(), B), np.resize(g2.ravel(), B)
    return W


def test_the_benchmark_never_pays_for_the_fallback(streams):
    """256 robots of the benchmark's seed, K = 3, as four wavefronts of 64 lanes: no restart. 100 robots carrying the
    gain-sweep grid (two wavefronts): the count found on the CPU is 0 as well, so the f3_gain_sweep configuration runs the
    fast body too."""
    fast = streams[0]
    st, ref = hover_initial_conditions(256, 20201118, np.float32)
    assert sum(_run(fast, _wave(st, ref, lo, 64), 3)[0] for lo in range(0, 256, 64)) == 0
    st, ref = hover_initial_conditions(100, 20201118, np.float32)
    W = _gain_grid_weights(100)
    assert sum(_run(fast, _wave(st, ref, lo, n, W), 3)[0] for lo, n in ((0, 64), (64, 36))) == 0


def test_instruction_budget(streams):
    """Executed instructions of the Ruiz phase per step on a clean robot: at least 1 400 fewer than the exact-only stream
    (9 passes x (258 limit - 86 tracking) = 1 548, less the finite guard and the range test)."""
    st, ref = hover_initial_conditions(1, 20201118, np.float32)
    n = [_run(stream, _wave(st, ref, 0, 1), 1, maxIter=2, nsub=1)[1] for stream in streams]
    assert n[1] - n[0] >= 1400, n
    g = streams[0][0]
    assert g.pool.peak <= 254
