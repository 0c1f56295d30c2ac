"""The shipped fp32 step kernels replayed in the interpreter, word for word (GPU).

A handle runs K closed-loop steps on the device; robobee3d_amd.asmstep.simulate runs the stream the kernel was generated
from on the same arrays, with the float parameters of asmstep.host_floats(). The five approximate instructions (v_rcp_f32,
v_rsq_f32, v_sqrt_f32; the fp32 streams hold no fp64 ones) take the device's own result through isasim.Machine's `approx`:
one probe launch of robobee3d_amd.isaprobe per executed instruction. Everything else is the interpreter's model, which
tests/test_isa_probe.py holds to the device instruction by instruction -- so every public word must be EQUAL, not close.

A difference is a bug in the interpreter, in host_floats() or in the generator (an address or a row): find the first
differing word and narrow it with the probes; it must never become a tolerance.

The fp64 step and the p5f kernel have no whole-kernel interpretation to replay against: the probes alone cover them."""
import numpy as np
import pytest

from robobee3d_amd import asmgen, asmstep
from robobee3d_amd.batch import hover_initial_conditions

pytestmark = pytest.mark.gpu
PUBLIC = ("state", "ctrl", "out", "stats", "status", "info")
KERNELS = {"lane": "umpc_rollout_asm_kernel", "quad": "umpc_rollout_asm_quad_kernel"}


@pytest.fixture(scope="module")
def device():
    import torch
    from robobee3d_amd import isaprobe
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return isaprobe.Device()


@pytest.fixture(scope="module")
def streams():
    return {"lane": asmstep.StepGen().program(), "quad": asmstep.StepGen(quad=True).program()}


def _handle(B, form, **prm):
    import torch
    from robobee3d_amd.batch import BatchUprightMPC
    m = BatchUprightMPC(B, torch.float32, plant_mode=1, **prm)
    m.set_step_kernel(form)
    return m


def _public(m):
    import torch
    torch.cuda.synchronize()
    return {n: getattr(m, n).cpu().numpy().reshape(-1, m.B) for n in PUBLIC}


def _wave(pub, ref, cols=slice(None), **opt):
    """the interpreter's arrays for the robots `cols` of a handle's public arrays (as read BEFORE the launch), [rows][lanes]"""
    a = {n: np.array(pub[n][:, cols], order="C") for n in PUBLIC}
    a["ref"] = np.array(ref[:, cols], np.float32, order="C")
    a["ws"] = np.zeros((asmgen.WS_ROWS, a["state"].shape[1]), np.float32)
    a.update(opt)
    return a


def _one(a):
    """the same for the one-lane machine: vectors indexed by row"""
    return {n: None if x is None else np.ascontiguousarray(x[:, 0]) for n, x in a.items()}


def _equal_bits(got, want, names, what):
    bad = []
    for n in names:
        g, w = np.asarray(got[n]).view(np.uint32).reshape(-1), np.asarray(want[n]).view(np.uint32).reshape(-1)
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        d = np.nonzero(g != w)[0]
        if len(d):
            bad.append("%s: %d of %d words differ, first at flat index %d: device 0x%08x, interpreter 0x%08x"
                       % (n, len(d), len(g), d[0], g[d[0]], w[d[0]]))
    assert not bad, "%s\n  " % what + "\n  ".join(bad)


def test_lane_form_full_wave(device, streams):
    """B = 64, 50 iterations, 25 substeps, K = 2 in one launch: one whole wavefront, status 1 and status 2 robots in it"""
    B, K = 64, 2
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    m = _handle(B, "lane")
    m.set_state(st, ref)
    a = _wave(_public(m), ref)
    m.rollout(K)
    got = _public(m)
    assert m.kernel_name == KERNELS["lane"]
    asmstep.simulate(streams["lane"], a, dict(K=K, maxIter=50, nsub=25, plant=1), asmstep.host_floats(), lanes=B,
                     max_exec=10 ** 7, approx=device.approx)
    _equal_bits(got, a, PUBLIC, "lane form, B = 64, K = 2")
    status = got["status"].reshape(-1)
    assert set(np.unique(status)) == {1, 2}, np.unique(status, return_counts=True)
    assert device.calls > 1000           # the replay did take the device's values


def _partial_wave_with_tables(device, streams, source):
    """B = 5 (a partial wave) with per-robot weights, an impulse table and the step history, K = 2 in one launch, history
    slices included. A handle takes a task or a reference table, not both, so the reference comes from `source`:
    "table": set_reference_trajectory (the `ref` pointer moves per step; the table is the helix generator's, so both
             runs fly the same trajectory);
    "task":  set_task("helix"): the stream's taskf branch (asmstep.load_taskf) on the entries umpc_taskf_kernel fills in,
             8 floats per step. The interpreter takes them from rows 0..6 and 8 of task_table on a handle with a zero
             `ref` and the same task: the same device function and the same fire-time expression (csrc/umpc_sim.hip,
             umpc_task_table_kernel), read back as data."""
    B, K = 5, 2
    st, ref = hover_initial_conditions(B, 20201118, np.float32)
    rng = np.random.default_rng(7)
    W = np.tile(np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2], np.float32)[:, None], (1, B))
    W[2], W[4] = rng.uniform(0.5, 2.0, B), rng.uniform(500, 2000, B)
    kick = (rng.normal(size=(K, 6, B)) * np.array([0.05, 0.05, 0.05, 1e-3, 1e-3, 1e-3])[None, :, None]).astype(np.float32)
    task = dict(trajAmp=60.0, trajFreq=1.5, dz=0.2)
    m = _handle(B, "lane")
    m.set_state(st, ref)
    m.set_weights(W)
    opt, moves = {}, {}
    stride = 4 * B
    if source == "table":
        tab = m.task_table(K, "helix", t_ms=0.0, **task)
        m.set_reference_trajectory(tab)
        ref_rows = np.ascontiguousarray(tab.cpu().numpy().reshape(K * 9, B))
        moves["refstep"] = 9 * stride
    else:
        m.set_task("helix", **task)
        z = _handle(1, "lane")
        z.set_task("helix", **task)
        assert z.time_ms == m.time_ms == 0.0 and not z.ref.any()
        t9 = z.task_table(K).cpu().numpy()[:, :, 0]                     # [K, 9] on a zero ref: the task's own part
        opt["taskf"] = np.ascontiguousarray(t9[:, [0, 1, 2, 3, 4, 5, 6, 8]].reshape(-1))
        assert opt["taskf"].any() and not t9[:, 7].any()               # (sdes_y is 0 in every task)
        ref_rows = np.array(ref, np.float32, order="C")                 # rows 0..2: the robots' initialPos
    m.set_impulses(kick)
    m.record_history(K, state=True, out=True, status=True, info=True)
    pub = _public(m)
    m.rollout(K)
    got = _public(m)
    assert m.kernel_name == KERNELS["lane"]
    hist = {n: t.cpu().numpy().reshape(-1, B) for n, t in m.history().items()}
    a = _wave(pub, ref, weights=W.copy(), impulse=np.ascontiguousarray(kick.reshape(K * 6, B)), **opt)
    a["ref"] = ref_rows
    rows = {"state": 18, "out": 9, "status": 1, "info": 2}
    for n, r in rows.items():                 # tables of slices; slice 0 of state is the initial state
        t = np.zeros((r * (K + (n == "state")), B), a[n].dtype)
        if n == "state":
            t[:r] = a[n]
        a[n] = t
    asmstep.simulate(streams["lane"], a, dict(K=K, maxIter=50, nsub=25, plant=1, statestep=18 * stride, outstep=9 * stride,
                                              statusstep=stride, infostep=2 * stride, **moves),
                     asmstep.host_floats(), lanes=B, max_exec=10 ** 7, approx=device.approx)
    _equal_bits(hist, a, tuple(rows), "lane form, B = 5, %s: history tables" % source)
    last = {n: a[n][-r:] for n, r in rows.items()}
    last.update(ctrl=a["ctrl"], stats=a["stats"])
    _equal_bits(got, last, PUBLIC, "lane form, B = 5, %s: the public arrays hold the last slices" % source)
    return got


def test_lane_form_partial_wave_with_every_table(device, streams):
    """weights, the reference table, an impulse table and history"""
    _partial_wave_with_tables(device, streams, "table")


def test_lane_form_partial_wave_with_a_task(device, streams):
    """weights, the task generator inside the launch, an impulse table and history"""
    _partial_wave_with_tables(device, streams, "task")


def test_quad_form_single_robots(device, streams):
    """three robots, each a B = 1 handle on the quad form (the wave-wide decisions are then the one robot's), K = 2"""
    K = 2
    st, ref = hover_initial_conditions(3, 20201118, np.float32)
    for r in range(3):
        m = _handle(1, "quad")
        m.set_state(st[:, r:r + 1], ref[:, r:r + 1])
        a = _one(_wave(_public(m), ref[:, r:r + 1]))
        m.rollout(K)
        got = _public(m)
        assert m.kernel_name == KERNELS["quad"]
        asmstep.simulate(streams["quad"], a, dict(K=K, maxIter=50, nsub=25, plant=1), asmstep.host_floats(), lanes=1,
                         max_exec=10 ** 7, approx=device.approx)
        _equal_bits(got, a, PUBLIC, "quad form, robot %d" % r)


def test_lane_form_nan_branch(device, streams):
    """the twelve calls of tests/golden/nan_branch.npz as one partial wave of the lane form (one controller step, no plant):
    calls 4 and 9 fail (status -7); their stored words, the OSQP_NAN number among them, and everybody's are equal"""
    import torch
    from conftest import golden
    from test_gpu_parity import _load_seq_into
    from robobee3d_amd.batch import BatchUprightMPC
    seq = golden("nan_branch.npz")
    n, maxIter = len(seq["p0"]), int(seq["maxIter"])
    m = BatchUprightMPC(n, torch.float32, maxIter=maxIter)
    m.set_step_kernel("lane")
    _, ref, _ = _load_seq_into(m, seq, torch, n)
    pub = _public(m)
    aT0 = m.actualT0.cpu().numpy().reshape(1, n).copy()
    m.update()
    got = _public(m)
    assert m.kernel_name == KERNELS["lane"]
    a = _wave(pub, ref, aT0=aT0)
    a["stats"] = None                         # update() passes none
    asmstep.simulate(streams["lane"], a, dict(K=1, maxIter=maxIter, nsub=0, plant=int(m.prm.plant_mode)), asmstep.host_floats(),
                     lanes=n, max_exec=10 ** 7, approx=device.approx)
    names = tuple(k for k in PUBLIC if k != "stats")
    _equal_bits(got, a, names, "lane form, NaN branch")
    status = got["status"].reshape(-1)
    assert list(np.nonzero(status == -7)[0]) == [4, 9]
    assert (got["out"][1:3][:, [4, 9]] == np.float32(2143289344.0)).all()            # OSQP_NAN (constants.h:96), stored as a number
