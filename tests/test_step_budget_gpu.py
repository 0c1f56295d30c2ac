"""The shortened fp32 step streams on the device (GPU): the lane stream with the packed RK4 substep and the quad stream with
select-based, speculating Ruiz passes, replayed in the interpreter word for word by the method of tests/test_stream_replay.py
(the approximate instructions take the device's own results, everything else is the interpreter's model: EQUAL, not close).

What the CPU cannot see and this file can: the packed instructions' operand selects and negations as the hardware decodes
them, the wait states the DPP reads of the new Ruiz body rely on, and the restart of a step from inside the quad section.

Shapes: the batch sizes and K are the two-wavefront ones the streams branch per wave on; ten ADMM iterations instead of fifty
(the iterations are untouched code and are most of what the interpreter would spend), the default 25 substeps."""
import numpy as np
import pytest

from robobee3d_amd import asmgen, asmstep
from robobee3d_amd.batch import hover_initial_conditions, monte_carlo_draws

pytestmark = pytest.mark.gpu
PUBLIC = ("state", "ctrl", "out", "stats", "status", "info")
KERNELS = {"lane": "umpc_rollout_asm_kernel", "quad": "umpc_rollout_asm_quad_kernel"}
K, MAXITER, NSUB = 3, 10, 25
DEFAULT_W = np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2], np.float32)      # rows ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom


@pytest.fixture(scope="module")
def device():
    import torch
    from robobee3d_amd import isaprobe
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return isaprobe.Device()


@pytest.fixture(scope="module")
def streams():
    return {"lane": asmstep.StepGen().program(), "quad-exact": asmstep.StepGen(quad=True, exact_ruiz=True).program()}


def _handle(B, form):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    m = BatchUprightMPC(B, torch.float32, plant_mode=1, maxIter=MAXITER, nsub=NSUB)
    m.set_step_kernel(form)
    return m


def _public(m):
    import torch
    torch.cuda.synchronize()
    return {n: getattr(m, n).cpu().numpy().reshape(-1, m.B) for n in PUBLIC}


def _wave(pub, ref, cols, **opt):
    a = {n: np.array(pub[n][:, cols], order="C") for n in PUBLIC}
    a["ref"] = np.array(ref[:, cols], np.float32, order="C")
    a["ws"] = np.zeros((asmgen.WS_ROWS, a["state"].shape[1]), np.float32)
    a.update({n: np.array(x[:, cols], order="C") for n, x in opt.items()})
    return a


def _differences(got, want, cols, what):
    bad = []
    for n in PUBLIC:
        g = np.ascontiguousarray(got[n][:, cols]).view(np.uint32).reshape(-1)
        w = np.ascontiguousarray(want[n]).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        d = np.nonzero(g != w)[0]
        if len(d):
            bad.append("%s, %s: %d of %d words differ, first at flat index %d: device 0x%08x, interpreter 0x%08x"
                       % (what, n, len(d), len(g), d[0], g[d[0]], w[d[0]]))
    return bad


@pytest.mark.parametrize("monte_carlo", [False, True], ids=["nominal", "monte-carlo"])
def test_lane_form_two_wavefronts(device, streams, monte_carlo):
    """B = 128, K = 3 in one launch, with and without per-robot inertia and thrust gain (the packed Ib w and Ib^-1 products
    read those as register pairs): state, ctrl, out, stats, status, info of both wavefronts equal the interpretation of the
    shipped lane stream bit for bit."""
    import torch
    B = 128
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    m = _handle(B, "lane")
    m.set_state(st, ref)
    opt = {}
    if monte_carlo:
        Ib, gain = monte_carlo_draws(B, 7, np.float32)
        m.Ib, m.gain = torch.as_tensor(Ib).to(m.device), torch.as_tensor(gain).to(m.device)
        opt = dict(Ib=np.asarray(Ib, np.float32), gain=np.asarray(gain, np.float32).reshape(1, B))
    pub = _public(m)
    m.rollout(K)
    got = _public(m)
    assert m.kernel_name == KERNELS["lane"]
    bad = []
    for lo in (0, 64):
        cols = slice(lo, lo + 64)
        a = _wave(pub, ref, cols, **opt)
        asmstep.simulate(streams["lane"], a, dict(K=K, maxIter=MAXITER, nsub=NSUB, plant=1), asmstep.host_floats(), lanes=64,
                         max_exec=10 ** 7, approx=device.approx)
        bad += _differences(got, a, cols, "lane form, robots %d..%d" % (lo, lo + 63))
    assert not bad, "\n  ".join(bad)
    assert np.isfinite(got["state"]).all() and device.calls > 1000


def test_quad_form_restart_inside_a_clean_wavefront(device, streams):
    """B = 32 (two wavefronts of 16 quads), K = 3. Robot 5 carries wvf = 1e14, out of limit_scaling's range in pass 2: its
    wavefront runs every step again through ten exact passes, the other wavefront never does. Robot 5, three clean robots of
    its wavefront and two of the other equal the interpretation of the exact-only quad stream (StepGen(quad=True,
    exact_ruiz=True): what the restart must reproduce, and the identity on a clean robot) bit for bit; and with robot 5 back
    at the default weights every OTHER robot's words are the same as before -- the restart leaks nowhere."""
    B, BAD = 32, 5
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    W = np.tile(DEFAULT_W[:, None], (1, B))
    runs = []
    for wvf in (1e14, DEFAULT_W[5]):
        W[5, BAD] = wvf
        m = _handle(B, "quad")
        m.set_state(st, ref)
        m.set_weights(W.copy())
        pub = _public(m)
        m.rollout(K)
        runs.append(_public(m))
        assert m.kernel_name == KERNELS["quad"]
    W[5, BAD] = 1e14
    got, clean = runs
    bad = []
    for r in (BAD, 0, 4, 15, 16, 31):
        a = _wave(pub, ref, slice(r, r + 1), weights=W)
        a = {n: np.ascontiguousarray(x[:, 0]) for n, x in a.items()}
        asmstep.simulate(streams["quad-exact"], a, dict(K=K, maxIter=MAXITER, nsub=NSUB, plant=1), asmstep.host_floats(),
                         lanes=1, max_exec=10 ** 7, approx=device.approx)
        bad += _differences(got, {n: a[n].reshape(-1, 1) for n in PUBLIC}, slice(r, r + 1), "quad form, robot %d" % r)
    assert not bad, "\n  ".join(bad)
    others = [r for r in range(B) if r != BAD]
    for n in PUBLIC:
        assert np.array_equal(got[n][:, others].view(np.uint32), clean[n][:, others].view(np.uint32)), n
    assert not np.array_equal(got["out"][:, BAD], clean["out"][:, BAD])
