"""Step-kernel parity pinned PER FORM. `set_step_kernel` can pin six kernels:

    fp32  lane  umpc_rollout_asm_kernel                          fp64  quad  umpc_rollout_kernel<double, LDSF, ASM64, QUAD>
    fp32  quad  umpc_rollout_asm_quad_kernel                     fp64  lane  umpc_rollout_kernel<double, LDSF, ASM64>
    fp32  cpp   umpc_rollout_kernel<float>                       fp64  cpp   umpc_rollout_kernel<double, LDSF>

The reference-fixture and oracle tests of tests/test_gpu_parity.py, tests/test_tasks_weights.py and
tests/test_r3_parity_evidence.py run "auto", which is the quad form at their batch sizes (B <= 16 384 in fp32, B <= 4 096 in
fp64). This file replays the same fixtures and closed loops on every form, and every test asserts BY NAME which kernel it ran
(`expect_kernel`), so a later dispatch change cannot move a test to another kernel unnoticed.

Bounds. The per-form tests assert the stated fp32 tolerance of the path, TOL_T = TOL_A = 3e-5 (about 3x the reference's own
rounding error against fp64: tests/test_oracle_golden.py) and the moment band max(2e-2, 1e-3 |u|) at scale 1, not the 1e-5 of
the "auto" test: on seq_iter50 the CPU oracle itself gives 0.89e-5 / 0.92e-5 (thrust / accdes) in the natural elimination order
and 1.27e-5 / 1.20e-5 in the fixture's order, so a second, equally correct summation order already crosses 1e-5. Every other
bound is the table of tests/test_gpu_parity.py, unchanged. `test_cpu_orders_inside_form_bounds` (no GPU) shows that
both CPU orders of the reference arithmetic sit inside every bound the GPU tests assert; nothing here is calibrated on what a
kernel form returns. fp64 forms: the bounds of test_fp64_kernel_matches_fp64_oracle (1e-9 relative on the outputs, 1e-8 on x,
status words equal).
"""
import numpy as np
import pytest

from conftest import golden
from test_gpu_parity import (DUA_RATIO, FIXTURE_SCALE, FLIP_FACTOR, ITERATE_TOL, PRI_REL, STATUS_FLIPS, TOL_T,
                             _check_outputs, _load_seq_into, tol_tau)

FORMS = ("lane", "quad", "cpp")
SEQS = ("seq_iter50.npz", "seq_iter10.npz", "seq_iter2.npz", "seq_iter1.npz")
OSQP_NAN = 2143289344.0        # constants.h:96: the NUMBER the reference stores into a failed solution

KERNELS = {
    ("fp32", "lane"): "umpc_rollout_asm_kernel",
    ("fp32", "quad"): "umpc_rollout_asm_quad_kernel",
    ("fp32", "cpp"): "umpc_rollout_kernel<float>",
    ("fp64", "quad"): "umpc_rollout_kernel<double, LDSF, ASM64, QUAD>",
    ("fp64", "lane"): "umpc_rollout_kernel<double, LDSF, ASM64>",
    ("fp64", "cpp"): "umpc_rollout_kernel<double, LDSF>",
}


def expect_kernel(dtype, form, maxIter=50):
    """The kernel `set_step_kernel(form)` must dispatch (launch_steps, csrc/umpc_mi355x.hip). The fp64 quad stream has no
    single-iteration path: with maxIter == 1 it falls to the fp64 lane kernel."""
    assert maxIter >= 1
    if dtype == "fp64" and form == "quad" and maxIter < 2:
        form = "lane"
    return KERNELS[dtype, form]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def test_expect_kernel_table():
    assert len(set(KERNELS.values())) == 6
    assert expect_kernel("fp64", "quad", 1) == expect_kernel("fp64", "lane", 1) == KERNELS["fp64", "lane"]
    assert expect_kernel("fp64", "quad", 2) == KERNELS["fp64", "quad"]
    assert expect_kernel("fp32", "quad", 1) == KERNELS["fp32", "quad"]


# ---------------------------------------------------------------------------
# The CPU oracle on a fixture, every call from the fixture's pre-call state. Computed once per (fixture, precision, order).
# ---------------------------------------------------------------------------
_ORACLE = {}


def _oracle_replay(oracle_built, fname, dtype, perm, n=None):
    """(out [9,n], ctrl [127,n], status [n], info [2,n]) of the canonical oracle in the layout of BatchUprightMPC."""
    key = (fname, np.dtype(dtype).name, None if perm is None else tuple(int(p) for p in perm), n)
    if key not in _ORACLE:
        seq = golden(fname)
        n_ = n or len(seq["p0"])
        o = oracle_built.Oracle(dtype, perm=perm, maxIter=int(seq["maxIter"]))
        out, ctrl = np.zeros((9, n_), dtype), np.zeros((127, n_), dtype)
        status, info = np.zeros(n_, np.int32), np.zeros((2, n_), dtype)
        for k in range(n_):
            o.set_canonical(True, seq["pre_E3"][k].astype(dtype))
            o.set_iterates(seq["pre_x"][k], seq["pre_y"][k], seq["pre_z"][k])
            o.set_T0(float(seq["pre_T0"][k]))
            uq, ac = o.update(seq["p0"][k], seq["R0"][k], seq["dq0"][k], seq["pdes"][k], seq["dpdes"][k], seq["sdes"][k],
                              float(seq["actualT0"][k]))
            out[:3, k], out[3:, k] = uq, ac
            ctrl[0:45, k], ctrl[45:84, k], ctrl[84:123, k] = o.get("x"), o.get("y"), o.get("z")
            ctrl[123, k] = o.get("T0")[0]
            ctrl[124:127, k] = o.get("E")[36:39]
            status[k] = o.get("status_val")[0]
            info[0, k], info[1, k] = o.get("pri_res")[0], o.get("dua_res")[0]
        for a in (out, ctrl, status, info):
            a.setflags(write=False)
        _ORACLE[key] = (out, ctrl, status, info)
    return _ORACLE[key]


# ---------------------------------------------------------------------------
# What a single step of a fixture is held to: the body of test_gpu_parity.test_single_step_matches_reference_golden with the
# stated tolerance of the path on the outputs. `rec` is the `margin` fixture.
# ---------------------------------------------------------------------------
def _assert_fixture_step(rec, label, fname, seq, structure, out, ctrl, status, info):
    import status_boundary
    n = len(seq["p0"])
    out, ctrl, info = (np.asarray(a, np.float64) for a in (out, ctrl, info))
    sc = FIXTURE_SCALE.get(fname, 1.0)
    _check_outputs(out, seq, n, label, sc, tau_scale=1.0)            # TOL_T = TOL_A = 3e-5, moment band at scale 1
    for name, sl in (("x", slice(0, 45)), ("y", slice(45, 84)), ("z", slice(84, 123))):
        ref = seq[name].T
        err = np.abs(ctrl[sl] - ref) / (1e-3 + np.abs(ref).max(axis=0, keepdims=True))
        rec("iterate %s: |d| / (1e-3 + max|ref|)" % name, err.max(), ITERATE_TOL[fname])
        assert err.max() < ITERATE_TOL[fname], (name, err.max())
    np.testing.assert_allclose(ctrl[123], seq["T0"], rtol=0, atol=TOL_T * sc)
    np.testing.assert_allclose(ctrl[124:127].T, seq["E"][:, 36:39], rtol=1e-5)
    mismatch = int(np.sum(status != seq["status"]))
    assert set(np.unique(status)).issubset({1, 2, -2}), np.unique(status)
    rec("status flips of %d" % n, mismatch, STATUS_FLIPS[fname])
    nflip, worst, arg = status_boundary.worst_flip(structure, seq, status)
    assert nflip == mismatch
    rec("worst flip: reference residual vs its eps (factor)", worst, FLIP_FACTOR[fname], "robot %d" % arg if arg >= 0 else "no flip")
    rel_pri = np.abs(info[0] - seq["pri_res"]) / seq["pri_res"]
    rec("median rel. error of pri_res", np.median(rel_pri), PRI_REL[fname])
    assert np.median(rel_pri) < PRI_REL[fname], np.median(rel_pri)
    med = float(np.median(info[1] / seq["dua_res"]))
    rec("median dua_res ratio (max of r, 1/r)", max(med, 1 / med), DUA_RATIO[fname])
    assert 1 / DUA_RATIO[fname] < med < DUA_RATIO[fname], med


def _assert_nan_branch(label, seq, out, ctrl, status):
    """The body of test_gpu_parity.test_nan_and_cold_start_branch_matches_reference (fp32)."""
    n = len(seq["p0"])
    out = np.asarray(out, np.float64)
    bad = np.nonzero(seq["status"] == -7)[0]
    assert list(bad) == [4, 9]
    assert list(np.nonzero(status == -7)[0]) == [4, 9]
    nanv = np.float32(OSQP_NAN)
    for k in bad:
        np.testing.assert_array_equal(out[1:3, k], nanv)                           # moments: the number itself
        np.testing.assert_array_equal(out[:3, k].astype(np.float32), seq["uquad"][k])
        np.testing.assert_allclose(out[3:, k], seq["accdes"][k], rtol=1e-6)        # (OSQP_NAN - dq0) / dt
        np.testing.assert_array_equal(ctrl[:123, k], 0)                            # cold start (auxil.c:563)
        np.testing.assert_array_equal(ctrl[123, k], seq["T0"][k])                  # T0 += OSQP_NAN, as the reference
    good = np.setdiff1d(np.arange(n), bad)
    assert set(np.unique(status[good])).issubset({1, 2, -2})
    _check_outputs(out, seq, n, label, sel=good)


@pytest.mark.parametrize("order", ["perm", "natural"])
@pytest.mark.parametrize("fname", SEQS + ("nan_branch.npz",))
def test_cpu_orders_inside_form_bounds(oracle_built, structure, margin, request, fname, order):
    """The bounds of the per-form GPU tests hold for the reference arithmetic alone: the canonical fp32 oracle under two
    elimination orders of the KKT factorisation (the fixture's `perm`, and none), every call from the fixture's pre-call
    state, held to exactly what `test_fp32_form_replays_fixture` / `..._nan_and_cold_start_branch` hold a kernel to.
    Two summation orders of the same algorithm meet them, so a form that sums differently can too."""
    seq = golden(fname)
    perm = structure["perm"] if order == "perm" else None
    out, ctrl, status, info = _oracle_replay(oracle_built, fname, np.float32, perm)
    if fname == "nan_branch.npz":
        _assert_nan_branch(request.node.name, seq, out, ctrl, status)
    else:
        _assert_fixture_step(margin, request.node.name, fname, seq, structure, out, ctrl, status, info)


def _fp64_bound_units(got, ref, rtol, atol):
    """assert_allclose's criterion as a number: max |got - ref| / (atol + rtol |ref|); <= 1 passes"""
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _assert_fp64_against_oracle(rec, got, want, sel=None):
    """The bounds of test_gpu_parity.test_fp64_kernel_matches_fp64_oracle; got / want = (out, ctrl, status[, info])."""
    sel = slice(None) if sel is None else sel
    rec("out[:3] |d| / (1e-10 + 1e-9|ref|)",
        _fp64_bound_units(got[0][:3, sel], want[0][:3, sel], 1e-9, 1e-10), 1.0)
    rec("accdes |d| / (1e-12 + 1e-9|ref|)",
        _fp64_bound_units(got[0][3:, sel], want[0][3:, sel], 1e-9, 1e-12), 1.0)
    rec("x |d| / (1e-10 + 1e-8|ref|)",
        _fp64_bound_units(got[1][:45, sel], want[1][:45, sel], 1e-8, 1e-10), 1.0)
    np.testing.assert_array_equal(got[2][sel], want[2][sel])


def test_cpu_fp64_orders_inside_fp64_bounds(oracle_built, structure, margin):
    """The fp64 bounds have room for any summation order: the fp64 oracle's two elimination orders, held to each other by the
    bounds the fp64 forms are held to the oracle by, differ by well under 1 % of them on the calls the GPU tests replay (see
    the margin lines), status words equal."""
    for fname in SEQS + ("nan_branch.npz",):
        n = min(64, len(golden(fname)["p0"]))
        a = _oracle_replay(oracle_built, fname, np.float64, structure["perm"], n)
        b = _oracle_replay(oracle_built, fname, np.float64, None, n)
        good = np.nonzero(a[2] != -7)[0]
        assert np.all(np.isfinite(a[0][:, good])) and np.all(np.isfinite(a[1][:, good]))
        for q, lo, hi, rtol, atol in (("out[:3]", 0, 3, 1e-9, 1e-10), ("accdes", 3, 9, 1e-9, 1e-12)):
            margin("%s %s: natural vs perm order, bound units" % (fname, q),
                   _fp64_bound_units(b[0][lo:hi, good], a[0][lo:hi, good], rtol, atol), 1.0)
        margin("%s x: natural vs perm order, bound units" % fname, _fp64_bound_units(b[1][:45, good], a[1][:45, good], 1e-8, 1e-10), 1.0)
        np.testing.assert_array_equal(a[2], b[2])


# ---------------------------------------------------------------------------
# a. / c. Reference fixtures, one step, on every form
# ---------------------------------------------------------------------------
def _run_fixture(torch, dtype, form, seq, n):
    from robobee3d_amd.batch import BatchUprightMPC
    maxIter = int(seq["maxIter"])
    mpc = BatchUprightMPC(n, dtype, maxIter=maxIter)
    mpc.set_step_kernel(form)
    _load_seq_into(mpc, seq, torch, n)
    mpc.update()
    torch.cuda.synchronize()
    assert mpc.kernel_name == expect_kernel("fp32" if dtype == torch.float32 else "fp64", form, maxIter)
    return mpc.out.cpu().numpy(), mpc.ctrl.cpu().numpy(), mpc.status.cpu().numpy(), mpc.info.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SEQS)
@pytest.mark.parametrize("form", FORMS)
def test_fp32_form_replays_fixture(torch_cuda, structure, margin, request, form, fname):
    """Every call of a reference sequence as one batch (robot k starts from the reference's state before call k: warm start
    x, y, z, T0, E), on the pinned form. maxIter = 1, 2 and >= 3 take different paths through each stream."""
    seq = golden(fname)
    n = len(seq["p0"])
    out, ctrl, status, info = _run_fixture(torch_cuda, torch_cuda.float32, form, seq, n)
    _assert_fixture_step(margin, request.node.name, fname, seq, structure, out, ctrl, status, info)


@pytest.mark.gpu
@pytest.mark.parametrize("fname", SEQS)
@pytest.mark.parametrize("form", FORMS)
def test_fp64_form_replays_fixture(torch_cuda, oracle_built, margin, form, fname):
    """The first 64 calls (or all 24) of a reference sequence on the pinned fp64 form against the fp64 oracle started from
    the same pre-call state. With maxIter == 1 the quad form is the lane kernel (expect_kernel)."""
    from robobee3d_amd import _lib
    seq = golden(fname)
    n = min(64, len(seq["p0"]))
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    got = _run_fixture(torch_cuda, torch_cuda.float64, form, seq, n)
    _assert_fp64_against_oracle(margin, got, _oracle_replay(oracle_built, fname, np.float64, perm, n))


# ---------------------------------------------------------------------------
# b. NaN / cold-start branch
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fp32_form_nan_and_cold_start_branch(torch_cuda, request, form):
    """SURVEY a14 on the pinned form: calls 4 and 9 of tests/golden/nan_branch.npz see a state of 1e33 (status -7, OSQP_NAN
    stored as a number, iterates cold-started), the calls after them restart from zero iterates with actualT0 overriding the
    thrust accumulator. Bit-exact where test_nan_and_cold_start_branch_matches_reference is."""
    seq = golden("nan_branch.npz")
    out, ctrl, status, _ = _run_fixture(torch_cuda, torch_cuda.float32, form, seq, len(seq["p0"]))
    _assert_nan_branch(request.node.name, seq, out, ctrl, status)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fp64_form_nan_and_cold_start_branch(torch_cuda, oracle_built, margin, form):
    """The same twelve calls in fp64 against the fp64 oracle: -7 at calls 4 and 9 with zeroed iterates, every other call
    inside the fp64 bounds."""
    from robobee3d_amd import _lib
    seq = golden("nan_branch.npz")
    n = len(seq["p0"])
    perm = np.array(_lib.lib().umpcKKTPerm().contents)
    got = _run_fixture(torch_cuda, torch_cuda.float64, form, seq, n)
    want = _oracle_replay(oracle_built, "nan_branch.npz", np.float64, perm, n)
    assert list(np.nonzero(want[2] == -7)[0]) == [4, 9]
    assert list(np.nonzero(got[2] == -7)[0]) == [4, 9]
    for k in (4, 9):
        np.testing.assert_array_equal(got[1][:123, k], 0)
        np.testing.assert_array_equal(got[0][1:3, k], OSQP_NAN)
    good = np.setdiff1d(np.arange(n), [4, 9])
    assert set(np.unique(got[2][good])).issubset({1, 2, -2})
    _assert_fp64_against_oracle(margin, got, want, sel=good)


# ---------------------------------------------------------------------------
# d. Partial waves
# ---------------------------------------------------------------------------
def _results(m):
    return [t.cpu().numpy() for t in (m.state, m.out, m.ctrl, m.status, m.stats)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", ["fp32", "fp64"])
def test_form_partial_waves_are_bit_identical_slices(torch_cuda, dtype, form):
    """B = 1, 63, 65, each alone, against the same columns of B = 131 (the last wave of every one of them is partial; B = 1
    and 63 have no full wave at all), K = 3 closed-loop steps; one launch of three steps == three launches of one. fp32 with
    the RK4 plant, fp64 with the Euler/expm plant. For the lane forms a wave whose EXEC mask is partial from the first
    instruction runs on the GPU only here."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    tdt, npdt, plant_mode = (torch.float32, np.float32, 1) if dtype == "fp32" else (torch.float64, np.float64, 0)
    st, ref = hover_initial_conditions(131, 7, npdt)

    def run(n, launches):
        m = BatchUprightMPC(n, tdt, plant_mode=plant_mode)
        m.set_step_kernel(form)
        m.set_state(st[:, :n].copy(), ref[:, :n].copy())
        for k in launches:
            m.rollout(k)
            assert m.kernel_name == expect_kernel(dtype, form)
        return _results(m)
    big = run(131, (3,))
    assert np.all(np.isfinite(big[0])) and set(np.unique(big[3])).issubset({1, 2, -2})
    for a, b in zip(run(131, (1, 1, 1)), big):
        np.testing.assert_array_equal(a, b)
    for n in (1, 63, 65):
        for launches in ((3,), (1, 1, 1)):
            for a, b in zip(run(n, launches), big):
                np.testing.assert_array_equal(a, b[..., :n])


@pytest.mark.gpu
def test_a_shard_of_a_large_job_runs_the_lane_form(torch_cuda):
    """A block of 100 robots of a 65 536-robot job runs the form the whole job runs (the lane form), without
    `set_step_kernel`: bit for bit what the pinned lane form computes."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    st, ref = hover_initial_conditions(100, 7, np.float32)
    res = []
    for kw, form in ((dict(global_batch=65536), None), ({}, "lane")):
        m = BatchUprightMPC(100, torch.float32, plant_mode=1, **kw)
        if form:
            m.set_step_kernel(form)
        m.set_state(st, ref)
        m.rollout(3)
        assert m.kernel_name == expect_kernel("fp32", "lane")
        res.append(_results(m))
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# e. Closed loops with per-robot inputs against the oracle, fp32, every form
# ---------------------------------------------------------------------------
_CLOSED = {}


def _closed_loop_oracle(oracle_built, key, st, ref, K, dtype, **kw):
    """batch_rollout from (st, ref) once per case and precision: (final state, out, stats)"""
    key = (key, np.dtype(dtype).name)
    if key not in _CLOSED:
        from robobee3d_amd import _lib
        perm = np.array(_lib.lib().umpcKKTPerm().contents)
        B = st.shape[1]
        s = st.astype(dtype)
        ctrl = np.zeros((127, B), dtype); ctrl[124:] = 1
        kw = {k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        out, stats, _ = oracle_built.batch_rollout(s, ctrl, ref.astype(dtype), K, dtype=dtype, perm=perm, **kw)
        _CLOSED[key] = (s, out, stats)
    return _CLOSED[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fp32_form_config5_inputs_match_oracle(torch_cuda, oracle_built, margin, form):
    """Per-robot inertia and thrust gain (config 5 inputs), RK4 plant, B = 320, K = 8 on the pinned form against the fp64
    oracle: the fp32 closed-loop band of test_assembly_kernel_ragged_batches_and_monte_carlo."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions, monte_carlo_draws
    B, K = 320, 8
    st, ref = hover_initial_conditions(B, 20201120, np.float64)
    Ib, gain = monte_carlo_draws(B, 20201120, np.float64)
    s_o, _, stats_o = _closed_loop_oracle(oracle_built, "config5", st, ref, K, np.float64, Ib=Ib, gain=gain, plant_mode=1)
    m = BatchUprightMPC(B, torch.float32, plant_mode=1)
    m.set_step_kernel(form)
    m.set_state(st.astype(np.float32), ref.astype(np.float32))
    m.Ib = torch.as_tensor(Ib.astype(np.float32)).cuda()
    m.gain = torch.as_tensor(gain.astype(np.float32)).cuda()
    m.rollout(K)
    assert m.kernel_name == expect_kernel("fp32", form)
    s = m.state.cpu().numpy().astype(np.float64)
    margin("|dp| mm vs fp64 oracle", np.abs(s[0:3] - s_o[0:3]).max(), 1.5e-3)
    margin("|dR|,|ddq| vs fp64 oracle", np.abs(s[3:] - s_o[3:]).max(), 3e-4)
    np.testing.assert_allclose(m.stats.cpu().numpy(), stats_o, rtol=1e-3)


def _self_calibrating_band(oracle_built, key, st, ref, K, **kw):
    """tests/test_tasks_weights.py: the kernel may be at most 4x as far from the fp64 trajectory as the fp32 CPU oracle (the
    reference's arithmetic) itself is; floors 2e-3 mm / 3e-4. Measured against the reference, not the kernel."""
    s_o, _, stats_o = _closed_loop_oracle(oracle_built, key, st, ref, K, np.float64, **kw)
    s_o32 = _closed_loop_oracle(oracle_built, key, st, ref, K, np.float32, **kw)[0].astype(np.float64)
    return s_o, stats_o, max(2e-3, 4 * np.abs(s_o32[0:3] - s_o[0:3]).max()), max(3e-4, 4 * np.abs(s_o32[3:] - s_o[3:]).max())


TASK_CASES = [(1, (80.0, 1.0, 0.15, 1.0), "helix"), (2, (500.0, 2.0), "straightAcc"), (3, (100.0, 200.0), "flip"),
              (4, (500.0, 100.0, 450.0, 0.2), "perch")]          # tests/test_tasks_weights.py CASES[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TASK_CASES, ids=[c[2] for c in TASK_CASES])
@pytest.mark.parametrize("form", FORMS)
def test_fp32_form_closed_loop_with_task_matches_oracle(torch_cuda, oracle_built, margin, form, case):
    """The reference generators of template/flight_tasks.py evaluated at every MPC fire, B = 128, K = 8 in two launches (the
    task clock carries over), on the pinned form against the fp64 oracle."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    task, tp, name = case
    kwn = BatchUprightMPC.TASKS[name][1]
    B, K, t0 = 128, 8, 35.0
    st, ref = hover_initial_conditions(B, 11, np.float64, tilt=0.2)
    ref[:] = 0
    ref[0:3] = np.random.default_rng(5).normal(size=(3, B))           # initialPos per robot
    st[0:3] = ref[0:3]
    s_o, _, band_p, band_r = _self_calibrating_band(oracle_built, "task " + name, st, ref, K, task=task, task_p=tp, t0=t0)
    m = BatchUprightMPC(B, torch.float32)
    m.set_step_kernel(form)
    m.set_state(st.astype(np.float32), ref.astype(np.float32))
    m.set_task(name, t_ms=t0, **dict(zip(kwn, tp)))
    m.rollout(K // 2)
    assert m.kernel_name == expect_kernel("fp32", form)
    assert m.time_ms == t0 + (K // 2) * 25 * 0.2
    m.rollout(K - K // 2)
    s = m.state.cpu().numpy().astype(np.float64)
    margin("|dp| mm vs fp64 oracle", np.abs(s[0:3] - s_o[0:3]).max(), band_p)
    margin("|dR|,|ddq| vs fp64 oracle", np.abs(s[3:] - s_o[3:]).max(), band_r)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fp32_form_gain_sweep_matches_oracle(torch_cuda, oracle_built, margin, form):
    """The 10 x 10 (wpr, wvr) grid of gainTuningSims as one batch of per-robot weights, K = 6, on the pinned form against
    the fp64 oracle."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, hover_initial_conditions
    g1, g2 = np.meshgrid(np.logspace(-2, 1, 10), np.logspace(1, 4, 10))
    B, K = g1.size, 6
    W = np.tile(np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2])[:, None], (1, B))
    W[2], W[4] = g1.ravel(), g2.ravel()
    st, ref = hover_initial_conditions(B, 3, np.float64)
    st[:, :] = st[:, :1]
    s_o, stats_o, band_p, band_r = _self_calibrating_band(oracle_built, "gain sweep", st, ref, K, weights=W)
    m = BatchUprightMPC(B, torch.float32)
    m.set_step_kernel(form)
    m.set_state(st.astype(np.float32), ref.astype(np.float32))
    m.set_weights(W.astype(np.float32))
    m.rollout(K)
    assert m.kernel_name == expect_kernel("fp32", form)
    s = m.state.cpu().numpy().astype(np.float64)
    margin("|dp| mm vs fp64 oracle", np.abs(s[0:3] - s_o[0:3]).max(), band_p)
    margin("|dR|,|ddq| vs fp64 oracle", np.abs(s[3:] - s_o[3:]).max(), band_r)
    np.testing.assert_allclose(m.stats.cpu().numpy(), stats_o, rtol=2e-3)


# ---------------------------------------------------------------------------
# f. Options together: the lane form beside "auto", against the C++ kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("opts", [("task",), ("weights",), ("wl",), ("task", "weights", "wl")], ids="+".join)
def test_lane_form_options_agree_with_the_cpp_kernel(torch_cuda, margin, opts):
    """The loop of test_r3_parity_evidence.test_assembly_kernel_options_agree_with_the_cpp_kernel (task table, per-robot
    weights, fused WL step, alone and together, B = 200) with the lane form beside "auto" (the quad form at this size), same
    bounds, both against the C++ kernel around the assembly loop."""
    torch = torch_cuda
    from robobee3d_amd.batch import BatchUprightMPC, BatchWLCon, hover_initial_conditions
    from test_wl_step import _args
    gl = golden("mpc_wl_loop.npz")
    B, K = 200, 6
    st, ref = hover_initial_conditions(B, 11, np.float32, tilt=0.2)
    rng = np.random.default_rng(5)
    W = np.tile(np.array([1e1, 1e3, 1, 5, 1e3, 2e3, 1e-1, 1e-2], np.float32)[:, None], (1, B))
    W[2] = rng.uniform(0.05, 8.0, B)
    W[4] = rng.uniform(50.0, 5e3, B)
    names = {"lane": expect_kernel("fp32", "lane"), "auto": expect_kernel("fp32", "quad"), "cpp": expect_kernel("fp32", "cpp")}
    res = {}
    for mode in ("lane", "auto", "cpp"):
        m = BatchUprightMPC(B, torch.float32, plant_mode=1)
        m.set_step_kernel(mode)
        r = ref.copy()
        s0 = st.copy()
        if "task" in opts:
            r[:] = 0
            r[0:3] = np.random.default_rng(6).normal(size=(3, B))
            s0[0:3] = r[0:3]
            m.set_task("helix", t_ms=35.0, trajAmp=40, trajFreq=2, dz=0.1, useY=True)
        m.set_state(s0, r)
        if "weights" in opts:
            m.set_weights(W)
        wl = None
        if "wl" in opts:
            wl = BatchWLCon(B, *_args(gl), dtype=torch.float32)
            m.set_wl(wl)
        m.rollout(K // 2)
        assert m.kernel_name == names[mode]
        m.rollout(K - K // 2)               # the task clock and the WL state carry over between launches
        assert m.kernel_name == names[mode]
        res[mode] = [t.cpu().numpy().astype(np.float64) for t in (m.state, m.out, m.stats, m.ctrl[123:124])] + \
                    ([wl.u.cpu().numpy().astype(np.float64), wl.w0.cpu().numpy().astype(np.float64)] if wl else [])
    c = res["cpp"]
    for mode in ("lane", "auto"):
        a = res[mode]
        lab = "%s vs cpp: " % mode
        margin(lab + "|dp| mm", float(np.abs(a[0][0:3] - c[0][0:3]).max()), 5e-4)
        margin(lab + "|dR|, |ddq|", float(np.abs(a[0][3:] - c[0][3:]).max()), 6e-5)
        margin(lab + "|d thrust|", float(np.abs(a[1][0] - c[1][0]).max()), 1e-5)
        margin(lab + "|d moment| / max(2e-2, 1e-3|u|)", float((np.abs(a[1][1:3] - c[1][1:3]) / tol_tau(c[1][1:3])).max()), 0.6)
        margin(lab + "stats relative", float(np.max(np.abs(a[2] - c[2]) / (1e-6 + np.abs(c[2])))), 3e-4)
        margin(lab + "|d T0 accumulator|", float(np.abs(a[3] - c[3]).max()), 4e-6)
        if "wl" in opts:
            margin(lab + "|d u4| / rate limit", float((np.abs(a[4] - c[4]) / np.array([5.0, 0.01, 0.01, 0.01])[:, None]).max()), 1.2e-3)
            margin(lab + "|d w0|", float(np.abs(a[5] - c[5]).max()), 2.5e-4)
