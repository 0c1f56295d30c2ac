"""Batched uprightmpc2 controller + plant on one MI355X (host side, Python).

torch is used only for device memory, streams and (elsewhere) torch.distributed;
all compute is in libumpc_mi355x.so, reached through the C ABI with raw device
pointers. Array convention: SoA [rows, B] contiguous, robot index fastest
(include/umpc_mi355x.h).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .score import u01 as _u01      # counter-based uniform in [0, 1): a hash of (seed, global robot index, salt)

_DT = {torch.float32: _lib.UMPC_F32, torch.float64: _lib.UMPC_F64}


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def hover_initial_conditions(B, seed, dtype=np.float32, tilt=0.5, index_offset=0):
    """Random-tilt hover start (reference single IC at
    template/uprightmpc2.py:101-103 is a=0.5, b=-0.5): p=0, Rb = Rx(a) Ry(b),
    a,b ~ U(-tilt, tilt), dq = (0.1,0,0,0,0,0). Streams are keyed by the GLOBAL
    robot index so a sharded run draws the same numbers as a single-GPU run.
    Returns state[18,B] (R column-major) and ref[9,B] (pdes=0, dpdes=0, sdes=e3)."""
    idx = np.arange(index_offset, index_offset + B, dtype=np.uint64)
    # counter-based: two uniforms per robot from a hash of (seed, index)
    a = (2 * _u01(seed, idx, 1) - 1) * tilt
    b = (2 * _u01(seed, idx, 2) - 1) * tilt
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    # R = Rx(a) @ Ry(b)
    R = np.empty((B, 3, 3))
    R[:, 0, 0] = cb; R[:, 0, 1] = 0; R[:, 0, 2] = sb
    R[:, 1, 0] = sa * sb; R[:, 1, 1] = ca; R[:, 1, 2] = -sa * cb
    R[:, 2, 0] = -ca * sb; R[:, 2, 1] = sa; R[:, 2, 2] = ca * cb
    state = np.zeros((18, B), dtype)
    state[3:12] = R.transpose(2, 1, 0).reshape(9, B)  # column-major: row r + 3*col c
    state[12] = 0.1
    ref = np.zeros((9, B), dtype)
    ref[8] = 1.0
    return state, ref


def monte_carlo_draws(B, seed, dtype=np.float32, spread=0.2, index_offset=0):
    """BASELINE configs[4] inputs: Ib = Ib0 (1 + d), d ~ U(-spread, spread)^3 for controller and
    plant, plant thrust gain 1 + U(-spread, spread); keyed by the GLOBAL robot index like hover_initial_conditions, so
    a sharded run draws exactly what the single-GPU run draws. Returns Ib [3, B], gain [B]."""
    idx = np.arange(index_offset, index_offset + B, dtype=np.uint64)
    Ib0 = np.array([3333.0, 3333.0, 1000.0])   # template/genqp.py:22
    Ib = np.stack([Ib0[i] * (1 + (2 * _u01(seed, idx, 11 + i) - 1) * spread) for i in range(3)])
    gain = 1 + (2 * _u01(seed, idx, 14) - 1) * spread
    return Ib.astype(dtype), gain.astype(dtype)


def _u01_device(seed, idx, salt):
    """_u01 on the device: the same counter hash in int64 two's-complement arithmetic (wrap-around multiplies, logical
    right shifts spelled as arithmetic shift + mask), bit-identical to the numpy uint64 version."""
    def c(v):        # 64-bit constant as a signed int
        v &= 0xFFFFFFFFFFFFFFFF
        return v - (1 << 64) if v >> 63 else v

    def lsr(v, k):
        return (v >> k) & ((1 << (64 - k)) - 1)
    v = idx + c(int(seed) * 0x9E3779B97F4A7C15) + int(salt)
    v = v ^ lsr(v, 30)
    v = v * c(0xBF58476D1CE4E5B9)
    v = v ^ lsr(v, 27)
    v = v * c(0x94D049BB133111EB)
    v = v ^ lsr(v, 31)
    return lsr(v, 11).to(torch.float64) / float(1 << 53)


def monte_carlo_draws_device(B, seed, dtype=torch.float32, spread=0.2, index_offset=0, device="cuda"):
    """monte_carlo_draws generated ON the device (an 8-rank config-5 start is then 8 tiny kernels, not 8
    host-side numpy passes over 2^17 x 4 draws + 8 uploads): same hash, same fp64 arithmetic, bit-identical values.
    Returns Ib [3, B], gain [B] as device tensors."""
    idx = torch.arange(index_offset, index_offset + B, dtype=torch.int64, device=device)
    Ib0 = (3333.0, 3333.0, 1000.0)   # template/genqp.py:22
    Ib = torch.stack([Ib0[i] * (1 + (2 * _u01_device(seed, idx, 11 + i) - 1) * spread) for i in range(3)])
    gain = 1 + (2 * _u01_device(seed, idx, 14) - 1) * spread
    return Ib.to(dtype).contiguous(), gain.to(dtype).contiguous()


def hover_initial_conditions_device(B, seed, dtype=torch.float32, tilt=0.5, index_offset=0, device="cuda"):
    """hover_initial_conditions generated ON the device: identical tilt angles (same hash, bit for bit); the rotation
    entries come from the device's fp64 sin / cos, which may differ from numpy's in the last fp64 bit before the cast."""
    idx = torch.arange(index_offset, index_offset + B, dtype=torch.int64, device=device)
    a = (2 * _u01_device(seed, idx, 1) - 1) * tilt
    b = (2 * _u01_device(seed, idx, 2) - 1) * tilt
    ca, sa, cb, sb = torch.cos(a), torch.sin(a), torch.cos(b), torch.sin(b)
    z = torch.zeros_like(a)
    state = torch.zeros((18, B), dtype=torch.float64, device=device)
    # R = Rx(a) Ry(b), column-major rows 3..11: entry r + 3 c
    cols = ((cb, sa * sb, -ca * sb), (z, ca, sa), (sb, -sa * cb, ca * cb))
    for cidx, col in enumerate(cols):
        for r in range(3):
            state[3 + r + 3 * cidx] = col[r]
    state[12] = 0.1
    ref = torch.zeros((9, B), dtype=torch.float64, device=device)
    ref[8] = 1.0
    return state.to(dtype).contiguous(), ref.to(dtype).contiguous(), (a, b)


def impulse_table(steps, B, events, dtype=torch.float32, device="cpu"):
    """Dense impulse table [steps, 6, B] for BatchUprightMPC.set_impulses from sparse events (step, robots, vec6): at the end
    of closed-loop step `step` the robots `robots` (None = all, an index, a slice or a sequence of indices) get
    (dv_world[3], domega_body[3]) = vec6, a [6] vector for all of them or [6, n] with one column per robot. Events that meet
    on one (step, robot) add up, in the order given and in `dtype`. The reference's experiment, controlTest(tpert=t)
    (template/uprightmpc2.py:130-133), is the single event (step of t, None, (0, 2, 0, 0, 0, 0))."""
    tab = torch.zeros((int(steps), 6, int(B)), dtype=dtype, device=device)
    for step, robots, vec in events:
        step = int(step)
        if not 0 <= step < int(steps):
            raise ValueError("impulse_table: step %d is outside the table of %d steps" % (step, int(steps)))
        vec = torch.as_tensor(np.asarray(vec, np.float64)).to(dtype).to(device)
        if vec.shape[0] != 6 or vec.dim() > 2:
            raise ValueError("impulse_table: an impulse is [6] or [6, n], got %r" % (tuple(vec.shape),))
        if robots is None:
            sel = slice(None)
        elif isinstance(robots, slice):
            sel = robots
        else:
            sel = torch.as_tensor(np.atleast_1d(np.asarray(robots, np.int64)), device=device)
            if len(torch.unique(sel)) != len(sel):
                raise ValueError("impulse_table: a robot is named twice in one event")
        tab[step, :, sel] += vec[:, None] if vec.dim() == 1 else vec
    return tab


# the generators of template/flight_tasks.py: name -> (UMPC_TASK_* id, the keywords that fill the parameter slots in order)
TASKS = {"ref": (0, ()), "helix": (1, ("trajAmp", "trajFreq", "dz", "useY")),
         "straightAcc": (2, ("tduration", "vdes")), "flip": (3, ("tstart", "tend")),
         "perch": (4, ("tend", "trotstart", "trotend", "vdes"))}
TASK_DEFAULTS = {"trajAmp": 80, "trajFreq": 1, "dz": 0.15, "useY": True, "tduration": 500, "vdes": None,
                 "tstart": 100, "tend": None, "trotstart": 100, "trotend": 450}


def task_arrays(B, tasks, params, default_task):
    """Per-robot task ids [B] int32 and parameters [4, B] float64 (the layout of umpcBatchTaskTable / umpcBatchReactiveRollout)
    from names and keywords. tasks: a name of TASKS, a length-B sequence of names, or None (= `default_task` for every
    robot); params: {keyword of TASK_DEFAULTS: a scalar or a [B] array}, defaults as set_task for each robot's task (vdes and
    tend depend on it). Pure numpy, no device. Raises TypeError on an unknown keyword."""
    B = int(B)
    bad = sorted(set(params) - set(TASK_DEFAULTS))
    if bad:
        raise TypeError("unknown task parameter(s) %r" % bad)
    names = [default_task] * B if tasks is None else [tasks] * B if isinstance(tasks, str) else list(tasks)
    if len(names) != B:
        raise ValueError("tasks must be one name or %d names" % B)
    names = np.asarray(names)
    ids = np.zeros(B, np.int32)
    P = np.zeros((4, B), np.float64)
    for name in sorted(set(names.tolist())):
        t_id, slots = TASKS[name]
        sel = names == name
        ids[sel] = t_id
        dflt = dict(TASK_DEFAULTS)
        dflt["vdes"] = {"straightAcc": 2, "perch": 0.2}.get(name, 0)
        dflt["tend"] = {"flip": 200, "perch": 500}.get(name, 0)
        for i, n in enumerate(slots):
            val = np.broadcast_to(np.asarray(params.get(n, dflt[n]), np.float64), (B,))
            P[i, sel] = val[sel]
    return ids, P


class BatchUprightMPC:
    """B independent uprightmpc2 controllers (+ plants), one GPU lane each."""

    def __init__(self, B, dtype=torch.float32, device="cuda", global_batch=None, **params):
        """global_batch: the size of the whole job when this object holds one block of a sharded batch (shard.py,
        SURVEY 8e). The automatic lane / quad choice of the step kernel is made from it, so every block runs the
        instruction stream the undivided batch would and the partition cannot change a bit of the result."""
        if not torch.cuda.is_available():
            raise RuntimeError("BatchUprightMPC needs a HIP device; there is no CPU path")
        self.L = _lib.lib()
        self.B, self.dtype, self.device = int(B), dtype, torch.device(device)
        self.prm = _lib.default_params()
        for k, v in params.items():
            if k == "Ib":
                for i in range(3):
                    self.prm.Ib[i] = float(v[i])
            else:
                if not hasattr(self.prm, k):
                    raise TypeError("unknown parameter %r" % k)
                setattr(self.prm, k, v)
        with torch.cuda.device(self.device):
            self.h = self.L.umpcBatchCreate(C.byref(self.prm), self.B, _DT[dtype])
        if not self.h:
            raise RuntimeError(self.L.umpcLastError().decode())
        if global_batch is not None:
            self._check(self.L.umpcBatchSetGlobalBatch(self.h, int(global_batch)))
        z = lambda r, dt=dtype: torch.zeros((r, self.B), dtype=dt, device=self.device)
        self.state, self.ctrl, self.ref = z(_lib.STATE_ROWS), z(_lib.CTRL_ROWS), z(_lib.REF_ROWS)
        self.out, self.stats, self.info = z(_lib.OUT_ROWS), z(_lib.STAT_ROWS), z(2)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.Ib = None
        self.gain = None
        self.actualT0 = None
        self.reset_controller()

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.umpcBatchDestroy(self.h)
                self.h = None
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        if rc:
            raise RuntimeError(self.L.umpcLastError().decode())

    def reset_controller(self):
        self._check(self.L.umpcBatchInitCtrl(self.h, _ptr(self.ctrl), self._stream()))
        self.stats.zero_()

    def set_state(self, state, ref=None):
        self.state.copy_(torch.as_tensor(state, dtype=self.dtype))
        if ref is not None:
            self.ref.copy_(torch.as_tensor(ref, dtype=self.dtype))

    TASKS, TASK_DEFAULTS = TASKS, TASK_DEFAULTS

    def set_task(self, name, t_ms=0.0, **kw):
        """On-device reference generator (template/flight_tasks.py, same keyword names and defaults).
        With a task other than "ref", rows 0..2 of `self.ref` are the robots' initialPos."""
        tid, names = self.TASKS[name]
        dflt = dict(self.TASK_DEFAULTS)
        dflt["vdes"] = {"straightAcc": 2, "perch": 0.2}.get(name, 0)
        dflt["tend"] = {"flip": 200, "perch": 500}.get(name, 0)
        vals = [float(kw.pop(n, dflt[n])) for n in names] + [0.0] * (4 - len(names))
        if kw:
            raise TypeError("unknown task parameter(s) %r" % sorted(kw))
        arr = (C.c_double * 4)(*vals)
        self._task = (tid, arr)
        self._check(self.L.umpcBatchSetTask(self.h, tid, arr, float(t_ms)))

    def set_reference_trajectory(self, tab, cursor=0):
        """A reference per closed-loop step and per robot (umpcBatchSetRefTrajectory): tab [steps, 9, B] holds the rows
        (pdes, dpdes, sdes) of every step; step k of a rollout reads slice ref_cursor + k and `self.ref` is not read. The
        cursor starts at `cursor` and advances with every rollout(); a rollout that would run past the table raises before
        anything is launched. None switches back to `self.ref`. Excludes set_task (either call raises after the other) and
        reactive_rollout / task_reference (reactive_steps reads the table, one slice held over each step); combines with
        everything else. Memory: 36 B x B x steps in fp32 -- chunk long runs."""
        if tab is None:
            self._check(self.L.umpcBatchSetRefTrajectory(self.h, None, 0, 0))
            self._reftab = None
            return
        t = torch.as_tensor(tab, dtype=self.dtype).to(self.device).contiguous()
        if t.dim() != 3 or tuple(t.shape[1:]) != (_lib.REF_ROWS, self.B):
            raise ValueError("reference trajectory must be [steps, 9, %d], got %r" % (self.B, tuple(t.shape)))
        self._check(self.L.umpcBatchSetRefTrajectory(self.h, _ptr(t), int(t.shape[0]), int(cursor)))
        self._reftab = t  # keep alive: the library stores the pointer

    @property
    def ref_cursor(self):
        """The slice of the reference trajectory the next closed-loop step reads (umpcBatchRefCursor)."""
        return int(self.L.umpcBatchRefCursor(self.h))

    def record_history(self, steps, state=True, out=True, status=False, info=False):
        """Record every closed-loop step of the following rollout() calls for the whole batch (umpcBatchSetHistory):
        allocates the chosen tables for `steps` steps -- state [steps + 1, 18, B] (slice k = the state before step k, slice
        k + 1 after it), out [steps, 9, B], status [steps, B] int32, info [steps, 2, B] -- and sets them with the cursor at 0.
        The kernels' own per-step stores go to the tables, so a K-step launch stays one launch with no store more (the fp64
        quad form alone -- fp64 at B <= 4 096, or set_step_kernel("quad") -- runs K single-step launches with a state copy each);
        self.state / out / status / info end every rollout holding what they hold without a history. Consecutive rollouts
        continue the tables; one that would pass `steps` raises before anything is launched. update(), plant() and
        reactive_rollout() record nothing; reactive_steps() records like rollout() (status 1, info 0, out rows 3..8 = 0).
        record_history(None) switches history off. Memory: 72 B x B x steps for the state and 36 B x B x steps for out in
        fp32 -- chunk long runs with rewind_history()."""
        if steps is None:
            self._check(self.L.umpcBatchSetHistory(self.h, None, None, None, None, 0, 0))
            self._hist = None
            return
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if int(self.prm.nsub) == 0:
            raise RuntimeError("record_history: the handle has no plant (nsub = 0), there is no trajectory to record")
        e = lambda shape, dt=self.dtype: torch.empty(shape, dtype=dt, device=self.device)
        hist = {"state": e((steps + 1, _lib.STATE_ROWS, self.B)) if state else None,
                "out": e((steps, _lib.OUT_ROWS, self.B)) if out else None,
                "status": e((steps, self.B), torch.int32) if status else None,
                "info": e((steps, 2, self.B)) if info else None}
        if all(v is None for v in hist.values()):
            raise ValueError("record_history: every record is off (record_history(None) switches history off)")
        self._check(self.L.umpcBatchSetHistory(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(hist["status"]),
                                               _ptr(hist["info"]), steps, 0))
        self._hist = hist  # keep alive: the library stores the pointers
        # where the record starts: the clock, the slice of a reference trajectory, the statistics accumulated before it
        self._hist_t0, self._hist_ref0, self._hist_stats0 = self.time_ms, self.ref_cursor, self.stats.clone()
        self._hist_imp0 = self.impulse_cursor      # (the slice of the table of set_impulses the first recorded step adds)

    def rewind_history(self, cursor=0):
        """Reuse the tables of record_history from step `cursor` on (a chunked long run: read the full tables out, rewind,
        roll on): no allocation, the records that are on stay on; what lies behind `cursor` is overwritten as the run goes."""
        hist = getattr(self, "_hist", None)
        if hist is None:
            raise RuntimeError("no history is set (record_history)")
        steps = next(int(v.shape[0]) - (k == "state") for k, v in hist.items() if v is not None)
        self._check(self.L.umpcBatchSetHistory(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(hist["status"]),
                                               _ptr(hist["info"]), steps, int(cursor)))
        step_ms = int(self.prm.nsub) * float(self.prm.dtsim)
        self._hist_t0, self._hist_ref0 = self.time_ms - int(cursor) * step_ms, self.ref_cursor - int(cursor)
        self._hist_imp0 = self.impulse_cursor - int(cursor)
        self._hist_stats0 = self.stats.clone()

    @property
    def history_cursor(self):
        """Closed-loop steps recorded so far = the step the next rollout records first (umpcBatchHistoryCursor)."""
        return int(self.L.umpcBatchHistoryCursor(self.h))

    def history(self):
        """The recorded part of the tables as views: {"state": [cursor + 1, 18, B], "out": [cursor, 9, B], "status":
        [cursor, B], "info": [cursor, 2, B]}, None for a record that is off."""
        hist = getattr(self, "_hist", None)
        if hist is None:
            raise RuntimeError("no history is set (record_history)")
        c = self.history_cursor
        return {k: None if v is None else v[:c + 1 if k == "state" else c] for k, v in hist.items()}

    def history_log(self, robots=(0,)):
        """The recorded steps of the selected robots in the layout of control_test_log / the reference's controlTest log
        (template/uprightmpc2.py:113,152-154), at MPC-step granularity: one row per closed-loop step k --
        't' the fire time, 'y' = (p, Rb[:, 2], dq) and 'R' the state the step fired on (before it), 'u' the command with
        the moments clipped at +-taulim as the plant saw them, 'accdes', 'pdes' from the reference trajectory, the task
        or `ref` -- plus 'metric' = the logMetric pair over the recorded substeps (from the statistics the step kernel
        accumulates per substep). Needs the state and out records. save_viewlog takes a log as is. Returns {robot: log}."""
        h = self.history()
        if h["state"] is None or h["out"] is None:
            raise RuntimeError("history_log needs the state and out records")
        n = self.history_cursor
        nsub, dts, tl = int(self.prm.nsub), float(self.prm.dtsim), float(self.prm.taulim)
        idx = torch.as_tensor(list(robots), device=self.device)
        tt = self._hist_t0 + np.arange(n) * (nsub * dts)
        st = h["state"][:n][:, :, idx].to(torch.float64).cpu().numpy()            # [n, 18, r]
        out = h["out"][:, :, idx].to(torch.float64).cpu().numpy()
        if getattr(self, "_reftab", None) is not None:
            pdes = self._reftab[self._hist_ref0:self._hist_ref0 + n, 0:3][:, :, idx].to(torch.float64).cpu().numpy()
        elif self._task_id() != 0:
            pdes = np.stack([self.task_reference(t)[0:3][:, idx].to(torch.float64).cpu().numpy() for t in tt]) if n else np.zeros((0, 3, len(idx)))
        else:
            pdes = np.repeat(self.ref[0:3][:, idx].to(torch.float64).cpu().numpy()[None], n, 0)
        met = ((self.stats - self._hist_stats0)[:, idx] / max(1, n * nsub)).to(torch.float64).cpu().numpy()
        logs = {}
        for c, r in enumerate(robots):
            u = out[:, 0:3, c].copy()
            u[:, 1:3] = np.clip(u[:, 1:3], -tl, tl)
            logs[r] = {"t": tt.copy(), "y": np.concatenate((st[:, 0:3, c], st[:, 9:12, c], st[:, 12:18, c]), 1), "u": u,
                       "pdes": pdes[:, :, c].copy(), "accdes": out[:, 3:9, c].copy(), "R": st[:, 3:12, c].copy(),
                       "metric": (float(met[0, c]), float(met[1, c]))}
        return logs

    def set_impulses(self, tab, cursor0=0):
        """A velocity kick per closed-loop step and per robot inside the rollout launch (umpcBatchSetImpulses): tab
        [steps, 6, B] holds (dv_world[3], domega_body[3]); slice impulse_cursor + k is added to self.state[12:18] after the last
        plant substep of step k of a rollout and before its state store -- the next step's controller, the state history's
        slice k + 1 and self.state after the launch see the kicked state (the placement of controlTest(tpert=...),
        template/uprightmpc2.py:130-133). One IEEE add per component: rollout(K) equals K times rollout(1) with
        `state[12:18] += tab[c]` in between, bit for bit. The cursor starts at `cursor0` and advances with every rollout();
        a rollout that would run past the table raises before anything is launched. reactive_rollout() honours the table
        too (one slice per nsub substeps; nsteps must then be a multiple of nsub), reactive_steps() like rollout(); update() and
        plant() do not. None
        switches impulses off. impulse_table() builds a table from sparse events. Memory: 24 B x B x steps in fp32 -- chunk
        long runs."""
        if tab is None:
            self._check(self.L.umpcBatchSetImpulses(self.h, None, 0, 0))
            self._imptab = None
            return
        t = torch.as_tensor(tab, dtype=self.dtype).to(self.device).contiguous()
        if t.dim() != 3 or tuple(t.shape[1:]) != (6, self.B):
            raise ValueError("impulse table must be [steps, 6, %d], got %r" % (self.B, tuple(t.shape)))
        self._check(self.L.umpcBatchSetImpulses(self.h, _ptr(t), int(t.shape[0]), int(cursor0)))
        self._imptab = t  # keep alive: the library stores the pointer

    def rewind_impulses(self, cursor=0):
        """Apply the table of set_impulses again from slice `cursor` on (a repeated experiment, or a chunked run whose table was
        refilled in place): no copy, no allocation."""
        t = getattr(self, "_imptab", None)
        if t is None:
            raise RuntimeError("no impulses are set (set_impulses)")
        self._check(self.L.umpcBatchSetImpulses(self.h, _ptr(t), int(t.shape[0]), int(cursor)))

    @property
    def impulse_cursor(self):
        """The slice of the impulse table the next closed-loop step adds (umpcBatchImpulseCursor)."""
        return int(self.L.umpcBatchImpulseCursor(self.h))

    def impulse_table(self, steps, events):
        """impulse_table() for this handle: [steps, 6, B] in its dtype, on its device."""
        return impulse_table(steps, self.B, events, self.dtype, self.device)

    def _history_window(self, what, first, count):
        """(hist, first, count) for a method `what` that reads the recorded steps first .. first + count - 1 of the step history;
        count None = up to the history cursor"""
        hist = getattr(self, "_hist", None)
        if hist is None or hist["state"] is None:
            raise RuntimeError("%s needs a step history with the state record (record_history)" % what)
        cur = self.history_cursor
        first = int(first)
        count = cur - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > cur:
            raise ValueError("%s: steps [%d, %d) are not inside the %d recorded steps" % (what, first, first + count, cur))
        return hist, first, count

    def _score_arg(self, name, t):
        if (tuple(t.shape) != (_lib.SCORE_ROWS, self.B) or t.dtype != self.dtype or t.device != self.state.device
                or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous [12, %d] tensor of the handle's dtype on its device" % (name, self.B))

    def _out_arg(self, out, shape):
        """`out` checked against `shape` [count, G, rows], or a new tensor of that shape"""
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device=self.device)
        if tuple(out.shape) != shape or out.dtype != torch.float64 or out.device != self.state.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous [%d, %d, %d] float64 tensor on the handle's device" % shape)
        return out

    def _group_index_arg(self, what, index):
        order, offset = index
        G = int(offset.numel()) - 1
        for t, n, name in ((order, self.B, "order"), (offset, G + 1, "offset")):
            if tuple(t.shape) != (n,) or t.dtype != torch.int32 or t.device != self.state.device or not t.is_contiguous():
                raise ValueError("%s: index must be the (order, offset) pair of group_index() of this handle (%s)" % (what, name))
        return order, offset, G

    def _scoring_reference(self, what, first, count, ref_table, ref_first):
        """What the recorded steps first .. first + count - 1 are scored against (score, ensemble): (table, its first slice) --
        `ref_table` when given, else the table of set_reference_trajectory -- or (None, 0) for the constant `self.ref`; a
        handle that follows a task generator has no table to read and raises."""
        reftab, rfirst = getattr(self, "_reftab", None), 0
        if ref_table is not None:
            reftab, rfirst = ref_table, int(ref_first) + first
            if (reftab.dim() != 3 or tuple(reftab.shape[1:]) != (_lib.REF_ROWS, self.B) or reftab.dtype != self.dtype
                    or reftab.device != self.state.device or not reftab.is_contiguous()):
                raise ValueError("ref_table must be a contiguous [steps, 9, %d] tensor of the handle's dtype on its device" % self.B)
            if rfirst < 0 or rfirst + count > int(reftab.shape[0]):
                raise ValueError("%s: ref_table does not cover the steps asked for" % what)
        elif reftab is not None:
            rfirst = self._hist_ref0 + first
            if rfirst < 0 or rfirst + count > int(reftab.shape[0]):
                raise ValueError("%s: the reference trajectory does not cover the steps asked for" % what)
        elif self._task_id() != 0:
            raise RuntimeError("%s: the handle follows a task generator, there is no reference table to read; build the "
                               "table with task_table() and pass it as ref_table (or set it with set_reference_trajectory() "
                               "before the run)" % what)
        return reftab, rfirst

    def score(self, first=0, count=None, tol=10.0, after=False, score=None, step0=None, ref_table=None, ref_first=0):
        """The recorded steps first .. first + count - 1 of the step history as a per-robot score [12, B] (umpcBatchScore; rows:
        robobee3d_amd/score.py -- steps, sum / max / last of e_p = |p - pdes|^2, sum / max of e_s = |s - sdes|^2, sum of
        the clipped moments squared, sum |p|^2, steps not solved, first / last step with e_p > tol^2, steps skipped as not
        finite), in ONE pass over the tables on the device: no temporary, nothing of the tables' size allocated.
        count None = up to the history cursor. The reference of step c is slice `history start + c` of the table of
        set_reference_trajectory, else the constant `self.ref`; a handle task has no table to read: build one with
        task_table and set it with set_reference_trajectory before the run. after=False scores the state each step fired
        on, after=True the state it produced (the convention of the reference's log). step0 (default `first`) is the step
        number rows 9 and 10 report for step `first`. Passing a score back in accumulates: a chunked run is scored chunk by
        chunk (rewind_history() in between, step0 = the steps already run). The out and status records enter when they are
        on; without them rows 6 / 8 stay as they are. ref_table [steps, 9, B], when given, is read IN PLACE of the set
        trajectory / `self.ref` / the task: recorded step c is scored against its slice ref_first + c -- a run that followed
        per-robot tasks or the handle's task (reactive_steps, rollout) is scored against task_table(...) without switching
        the controller to step-held references."""
        hist, first, count = self._history_window("score", first, count)
        reftab, rfirst = self._scoring_reference("score", first, count, ref_table, ref_first)
        with torch.cuda.device(self.device):
            if score is None:
                score = torch.empty((_lib.SCORE_ROWS, self.B), dtype=self.dtype, device=self.device)
                self._check(self.L.umpcBatchScoreInit(self.h, _ptr(score), self._stream()))
            else:
                self._score_arg("score", score)
            self._check(self.L.umpcBatchScore(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(hist["status"]),
                                              _ptr(reftab), None if reftab is not None else _ptr(self.ref), first, count,
                                              rfirst, first if step0 is None else int(step0), float(tol), int(bool(after)),
                                              _ptr(score), self._stream()))
        return score

    def score_groups(self, score, group, G):
        """[G, 8] float64 table of the scores of the robots of each group (umpcBatchScoreGroups; rows: robobee3d_amd/score.py):
        group [B] int32 names each robot's group -- the grid cell of a gain sweep, ids outside [0, G) are ignored. Raw sums
        (robots, robots scored, sum of the per-robot means of e_p / tau^2 / |p|^2, max e_p, robots that left the path, steps
        not solved), so the tables of the blocks of a sharded job add up (score.combine_groups). Bit-identical from run to
        run."""
        group = torch.as_tensor(group).to(torch.int32).to(self.device).contiguous()
        if tuple(group.shape) != (self.B,):
            raise ValueError("group must be [%d]" % self.B)
        self._score_arg("score", score)
        gstat = torch.empty((int(G), _lib.GSCORE_ROWS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchScoreGroups(self.h, _ptr(score), _ptr(group), int(G), _ptr(gstat), self._stream()))
        return gstat

    def group_index(self, group, G):
        """(order [B], offset [G + 1]) int32 on the device (umpcBatchGroupIndex): the robots sorted by group, once per sweep,
        for ensemble(). group [B] int32 is the array score_groups takes; order[offset[g]:offset[g + 1]] are the robots of
        group g in ascending index, order[offset[G]:] the robots whose id is outside [0, G)."""
        group = torch.as_tensor(group).to(torch.int32).to(self.device).contiguous()
        if tuple(group.shape) != (self.B,):
            raise ValueError("group must be [%d]" % self.B)
        order = torch.empty(self.B, dtype=torch.int32, device=self.device)
        offset = torch.empty(int(G) + 1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchGroupIndex(self.h, _ptr(group), int(G), _ptr(order), _ptr(offset), self._stream()))
        return order, offset

    def ensemble(self, index, first=0, count=None, tol=10.0, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history as per-step, per-group statistics [count, G, 16]
        float64 on the device (umpcBatchEnsemble; rows: robobee3d_amd/score.py -- members scored / skipped, sum, sum of
        squares, max and min of e_p, sum and max of e_s and of the clipped moments squared, members outside the tube
        e_p > tol^2, members not solved, the signed sums of p - pdes, the robot with the largest e_p): the curve of a grid cell
        over time, reduced over its draws and not over the steps, in ONE pass over the tables. index = group_index(group, G).
        first, count, tol, after, ref_table and ref_first are those of score(), and the reference is resolved as there. Every
        (step, group) row is independent and bit-reproducible; `out` [count, G, 16], when given, is overwritten and returned
        (a slice of a larger tensor serves a chunked run). Keep the cells contiguous in the batch (cell = b // 64): scattered
        ids are correct and an order of magnitude slower per load."""
        hist, first, count = self._history_window("ensemble", first, count)
        order, offset, G = self._group_index_arg("ensemble", index)
        reftab, rfirst = self._scoring_reference("ensemble", first, count, ref_table, ref_first)
        out = self._out_arg(out, (count, G, _lib.ENS_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchEnsemble(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(hist["status"]),
                                                 _ptr(reftab), None if reftab is not None else _ptr(self.ref), first, count,
                                                 rfirst, float(tol), int(bool(after)), _ptr(order), _ptr(offset), G, _ptr(out),
                                                 self._stream()))
        return out

    @staticmethod
    def _probs_arg(what, probs):
        from .score import QUANT_MAX_PROBS
        probs = [float(p) for p in (probs if hasattr(probs, "__len__") else [probs])]
        if not 1 <= len(probs) <= QUANT_MAX_PROBS or not all(0.0 <= p <= 1.0 for p in probs):
            raise ValueError("%s: 1 to %d probabilities, each in [0, 1]" % (what, QUANT_MAX_PROBS))
        return (C.c_double * len(probs))(*probs), len(probs)

    def ensemble_quantiles(self, index, probs, term="ep", first=0, count=None, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history as per-step, per-group order statistics
        [count, G, 2 + len(probs)] float64 on the device (umpcBatchEnsembleQuantiles; rows: robobee3d_amd/score.py -- members
        scored, members skipped, then for each probability p the element v[min(n - 1, max(0, ceil(p n) - 1))] of the scored
        members' terms in ascending order: 0 the minimum, 0.5 the lower median, 1 the maximum, NaN when nobody is scored): the
        median curve and percentile band of a grid cell, which one diverged draw does not own as it owns the mean and the max
        of ensemble(). term: "ep" |p - pdes|^2, "es" |s - sdes|^2, "tau" the clipped moments squared (needs the out record).
        index = group_index(group, G); probs: 1 to 8 numbers in [0, 1], passed in the launch arguments (no copy to the
        device, no synchronisation). first, count, after, ref_table, ref_first and out are those of ensemble(), and the
        reference is resolved as there. An element of the cell, never an interpolation: bit-reproducible and independent of
        everything but the member set. Quantiles of the blocks of a sharded job do not combine: keep a cell inside one block."""
        from .score import TERM_NAMES
        hist, first, count = self._history_window("ensemble_quantiles", first, count)
        order, offset, G = self._group_index_arg("ensemble_quantiles", index)
        if term not in TERM_NAMES:
            raise ValueError("ensemble_quantiles: term is one of %s" % (TERM_NAMES,))
        if term == "tau" and hist["out"] is None:
            raise RuntimeError("ensemble_quantiles: term 'tau' needs the out record of the step history")
        cprobs, nq = self._probs_arg("ensemble_quantiles", probs)
        reftab, rfirst = self._scoring_reference("ensemble_quantiles", first, count, ref_table, ref_first)
        out = self._out_arg(out, (count, G, 2 + nq))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchEnsembleQuantiles(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(reftab),
                                                          None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                                          int(bool(after)), _ptr(order), _ptr(offset), G, TERM_NAMES.index(term),
                                                          cprobs, nq, _ptr(out), self._stream()))
        return out

    def score_quantiles(self, score, index, probs, num, den=None):
        """[G, 2 + len(probs)] float64 order statistics of a per-robot score over the robots of each group
        (umpcBatchScoreQuantiles; rows as ensemble_quantiles): the value of robot b is score[num, b], or score[num, b] /
        score[den, b] in double (num = 1, den = 0: the per-robot mean tracking error, whose median over a cell is a cost
        table that one crashed draw does not own, as it owns the sums of score_groups). A robot enters when its row 0 > 0
        and its value is finite; the group's other members are counted in row 1. index = group_index(group, G)."""
        order, offset, G = self._group_index_arg("score_quantiles", index)
        self._score_arg("score", score)
        cprobs, nq = self._probs_arg("score_quantiles", probs)
        quant = torch.empty((G, 2 + nq), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchScoreQuantiles(self.h, _ptr(score), int(num), -1 if den is None else int(den), _ptr(order),
                                                       _ptr(offset), G, cprobs, nq, _ptr(quant), self._stream()))
        return quant

    def score_bootstrap(self, score, index, num, den=None, other=None, stat="mean", p=0.5, reps=1000, seed=0,
                        probs=(0.025, 0.975), return_reps=False):
        """[G, 5 + len(probs)] float64 bootstrap table of a per-robot score over the draws of each group
        (umpcBatchScoreBootstrap; rows: robobee3d_amd/score.py BOOT_N scored, BOOT_SKIPPED, BOOT_POINT the statistic of the
        cell, BOOT_MEAN and BOOT_SE of the replicates, then their nearest-rank element for each probability: (0.025, 0.975)
        is a 95 % percentile interval). The value of robot b is that of score_quantiles (score[num, b], or score[num, b] /
        score[den, b] in double); with other= (a second score of the same shape and dtype: the reactive run of the same
        sweep on the same tables) the same expression of `other` is subtracted, a comparison paired by draw, and a robot
        missing in either table is skipped. stat: "mean", or "quantile" with p (0.5 the lower median): an element of the
        resample, never an interpolation. The cell's scored values are resampled with replacement `reps` times by the
        counter hash of the Monte-Carlo draws; the indices depend on (seed, replicate, slot, members scored) alone, so cells
        with equal counts share them (common random numbers): with return_reps=True the replicates [G, reps] come back
        too, and reps[g1] - reps[g2] is a paired bootstrap of the difference between two cells when draw m of every cell
        carries the same perturbation. index = group_index(group, G). No host synchronisation; bit-reproducible. The rows of
        the blocks of a sharded job do not combine: keep a cell inside one block."""
        from .score import BOOT_FIRST, BOOT_MAX_REPS, BOOT_STATS
        order, offset, G = self._group_index_arg("score_bootstrap", index)
        self._score_arg("score", score)
        if other is not None:
            self._score_arg("other", other)
        if stat not in BOOT_STATS or not 0.0 <= float(p) <= 1.0:
            raise ValueError("score_bootstrap: stat is one of %s, p in [0, 1]" % (BOOT_STATS,))
        R = int(reps)
        if not 2 <= R <= BOOT_MAX_REPS:
            raise ValueError("score_bootstrap: 2 <= reps <= %d" % BOOT_MAX_REPS)
        cprobs, nq = self._probs_arg("score_bootstrap", probs)
        boot = torch.empty((G, BOOT_FIRST + nq), dtype=torch.float64, device=self.device)
        rep = torch.empty((G, R), dtype=torch.float64, device=self.device)
        work = torch.empty((self.B + G,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchScoreBootstrap(self.h, _ptr(score), _ptr(other), int(num), -1 if den is None else int(den),
                                                       _ptr(order), _ptr(offset), G, BOOT_STATS.index(stat), float(p), R,
                                                       int(seed) & 0xFFFFFFFFFFFFFFFF, cprobs, nq, _ptr(boot), _ptr(rep),
                                                       _ptr(work), self._stream()))
        return (boot, rep) if return_reps else boot

    def ensemble_bootstrap(self, index, term="ep", stat="mean", p=0.5, reps=1000, seed=0, probs=(0.025, 0.975), levels=(0.95,),
                           other=None, first=0, count=None, after=False, ref_table=None, ref_first=0, simultaneous=True, out=None):
        """Bootstrap confidence bands of the per-step curve of each group over the recorded steps first .. first + count - 1
        (umpcBatchEnsembleBootstrap; columns: robobee3d_amd/score.py BAND_N scored, BAND_SKIPPED, BAND_POINT the statistic of
        the cell at that step, BAND_MEAN and BAND_SE of its replicates, BAND_ENTERS, then the nearest-rank element of the
        replicates for each of `probs`: the POINTWISE percentile band): band [count, G, 6 + len(probs)] float64, in ONE launch
        and one pass over the tables, the replicates never stored. term, first, count, after, ref_table, ref_first and out are
        those of ensemble_quantiles() and the reference is resolved as there; stat, p, reps (2 .. 4096) and seed those of
        score_bootstrap(). other: another handle of the same B, dtype and device whose recorded history is read at the same
        window against the SAME reference -- in practice the reactive run of the same sweep: the value of a draw is then its
        term minus the other run's, a comparison paired by draw, and a draw missing in either run is skipped.
        The resample indices depend on (seed, replicate, slot, members scored) alone, so a replicate draws the same members at
        every step: it resamples whole trajectories. simultaneous=True returns (band, crit, sup): sup [G, reps] is every
        replicate's largest |t - point| / se over the steps that enter (BAND_ENTERS: at least two members scored and
        replicates that are not all the same double), crit [G, 1 + len(levels)] the number of entering steps and the
        nearest-rank element of sup[g] at each level. The simultaneous band of group g at levels[j] is
            band[:, g, BAND_POINT, None] + crit[g, 1 + j] * band[:, g, BAND_SE, None] * torch.tensor([-1.0, 1.0])
        -- one expression, left to the caller: it contains the whole curve with about that probability, which the pointwise
        band does not (a 90 % pointwise band around 20 steps holds the whole curve 15-20 % of the time). When a draw drops
        out mid-window its later steps are resampled with the indices of the new count. No host synchronisation;
        bit-reproducible. Rows of the blocks of a sharded job do not combine: keep a cell inside one block."""
        from .score import BAND_FIRST, BAND_MAX_REPS, BOOT_STATS, TERM_NAMES
        hist, first, count = self._history_window("ensemble_bootstrap", first, count)
        order, offset, G = self._group_index_arg("ensemble_bootstrap", index)
        if term not in TERM_NAMES:
            raise ValueError("ensemble_bootstrap: term is one of %s" % (TERM_NAMES,))
        if term == "tau" and hist["out"] is None:
            raise RuntimeError("ensemble_bootstrap: term 'tau' needs the out record of the step history")
        if stat not in BOOT_STATS or not 0.0 <= float(p) <= 1.0:
            raise ValueError("ensemble_bootstrap: stat is one of %s, p in [0, 1]" % (BOOT_STATS,))
        R = int(reps)
        if not 2 <= R <= BAND_MAX_REPS:
            raise ValueError("ensemble_bootstrap: 2 <= reps <= %d" % BAND_MAX_REPS)
        cprobs, nq = self._probs_arg("ensemble_bootstrap", probs)
        clevels, nl = self._probs_arg("ensemble_bootstrap", levels) if simultaneous else (None, 0)
        ostate = oout = None
        if other is not None:
            if not isinstance(other, BatchUprightMPC) or other.B != self.B or other.dtype != self.dtype or other.state.device != self.state.device:
                raise ValueError("ensemble_bootstrap: other must be a handle of the same B, dtype and device")
            ohist, _, _ = other._history_window("ensemble_bootstrap (other)", first, count)
            if (ohist["out"] is None) != (hist["out"] is None):
                raise ValueError("ensemble_bootstrap: both histories must have the out record, or neither")
            ostate, oout = ohist["state"], ohist["out"]
        reftab, rfirst = self._scoring_reference("ensemble_bootstrap", first, count, ref_table, ref_first)
        band = self._out_arg(out, (count, G, BAND_FIRST + nq))
        crit = sup = None
        if simultaneous:
            crit = torch.empty((G, 1 + nl), dtype=torch.float64, device=self.device)
            sup = torch.empty((G, R), dtype=torch.float64, device=self.device)
        work = torch.empty((self.B + G,), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchEnsembleBootstrap(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(ostate), _ptr(oout),
                                                          _ptr(reftab), None if reftab is not None else _ptr(self.ref), first,
                                                          count, rfirst, int(bool(after)), _ptr(order), _ptr(offset), G,
                                                          TERM_NAMES.index(term), BOOT_STATS.index(stat), float(p), R,
                                                          int(seed) & 0xFFFFFFFFFFFFFFFF, cprobs, nq, clevels, nl, _ptr(band),
                                                          _ptr(crit), _ptr(sup), _ptr(work), self._stream()))
        if simultaneous and count == 0:
            crit.fill_(float("nan")); sup.fill_(float("nan")); crit[:, 0] = 0.0      # (a no-op of the library: no step enters)
        return (band, crit, sup) if simultaneous else band

    def frequency_response(self, freq_hz, first=0, count=None, after=False, ref_table=None, ref_first=0, step0=None, sums=None,
                           fit=True):
        """The Bode point of every robot from the recorded steps first .. first + count - 1 of the step history
        (umpcBatchResponse / umpcBatchResponseFit; rows: robobee3d_amd/score.py RESP_* and RSUM_*): a three-parameter
        least-squares sine fit a0 + a1 cos + a2 sin of p and of pdes, per position axis, at the robot's own frequency, in
        ONE pass over the tables on the device -- no sine or cosine table, nothing of the tables' size allocated. freq_hz: a
        scalar or [B], the trajFreq a robot's task was built with; nu = freq_hz * 1e-3 * nsub * dtsim revolutions per step
        in float64 (score.response_nu). Returns (resp, sums): resp [3, 12, B] in the handle's dtype -- per axis the steps
        that entered (0 when the fit is refused: fewer than three steps, or nu = 0 or 0.5 where the sine is zero at every
        step; the rows behind are then NaN), the steps skipped as not finite, |Y|^2, |R|^2, gain, phase (negative = p
        lags pdes), Re and Im of Y / R, the two offsets, the mean squared residual of p's fit (distortion and everything
        off the fundamental) and |Y - R|^2, the squared amplitude of the tracking error at the fundamental; sums [33, B]
        float64, the raw sums of the normal equations. first, count, after, ref_table and ref_first are those of score()
        and the reference is resolved as there. step0 (default `first`) is the step number of step `first`: it sets the
        phase origin. Passing `sums` back in accumulates, and fit=False accumulates only (resp is None): a chunked run
        calls this once per chunk with rewind_history() in between, step0 = the steps already run, and fits at the end.
        resp[axis] is shaped as a score: score_quantiles(resp[0], index, [0.5], num=RESP_Y_AMP2, den=RESP_R_AMP2) is a cell's
        median gain^2, score_bootstrap(..., other=resp_reactive[0]) its interval and MPC minus reactive paired by draw.
        One frequency per call: a harmonic is a second call with 2 * freq_hz."""
        from .score import response_nu
        hist, first, count = self._history_window("frequency_response", first, count)
        reftab, rfirst = self._scoring_reference("frequency_response", first, count, ref_table, ref_first)
        nu = np.broadcast_to(response_nu(freq_hz, int(self.prm.nsub), float(self.prm.dtsim)), (self.B,))
        nu = torch.as_tensor(np.array(nu)).to(self.device)
        with torch.cuda.device(self.device):
            if sums is None:
                sums = torch.empty((_lib.RSUM_ROWS, self.B), dtype=torch.float64, device=self.device)
                self._check(self.L.umpcBatchResponseInit(self.h, _ptr(sums), self._stream()))
            elif (tuple(sums.shape) != (_lib.RSUM_ROWS, self.B) or sums.dtype != torch.float64 or sums.device != self.state.device
                  or not sums.is_contiguous()):
                raise ValueError("sums must be a contiguous [33, %d] float64 tensor on the handle's device" % self.B)
            self._check(self.L.umpcBatchResponse(self.h, _ptr(hist["state"]), _ptr(reftab),
                                                 None if reftab is not None else _ptr(self.ref), _ptr(nu), first, count, rfirst,
                                                 first if step0 is None else int(step0), int(bool(after)), _ptr(sums),
                                                 self._stream()))
            resp = None
            if fit:
                resp = torch.empty((3, _lib.RESP_ROWS, self.B), dtype=self.dtype, device=self.device)
                self._check(self.L.umpcBatchResponseFit(self.h, _ptr(sums), _ptr(resp), self._stream()))
        return resp, sums

    def dispersion(self, index, first=0, count=None, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history as the raw moments of the error state
        z = (p - pdes, v - dpdes) of each group [count, G, 32] float64 on the device (umpcBatchDispersion; rows:
        robobee3d_amd/score.py -- members scored / skipped, S1 = sum z [6], S2 = sum z_i z_j [21], the upper triangle row by
        row), in ONE pass over the tables: what dispersion_ellipsoids() turns into the mean, the covariance and the ellipsoid
        of a cell's cloud at every step. index = group_index(group, G). first, count, after, ref_table, ref_first and out are
        those of ensemble(), and the reference is resolved as there. A member is scored when p, v, pdes and dpdes are finite
        (not ensemble()'s rule: v is read, s, out and the status are not). Every (step, group) row is independent and
        bit-reproducible, and raw moments ADD: the rows of the blocks of a sharded job combine exactly in their counts and to
        rounding in their sums (score.combine_dispersions). Keep the cells contiguous in the batch (cell = b // 64)."""
        hist, first, count = self._history_window("dispersion", first, count)
        order, offset, G = self._group_index_arg("dispersion", index)
        reftab, rfirst = self._scoring_reference("dispersion", first, count, ref_table, ref_first)
        out = self._out_arg(out, (count, G, _lib.DISP_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchDispersion(self.h, _ptr(hist["state"]), _ptr(reftab),
                                                   None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                                   int(bool(after)), _ptr(order), _ptr(offset), G, _ptr(out), self._stream()))
        return out

    def dispersion_ellipsoids(self, mom, out=None):
        """[count, G, 48] float64 from the moments [count, G, 32] of dispersion() (umpcBatchDispersionEllipsoids; rows:
        robobee3d_amd/score.py -- n, skipped, the mean [6], the covariance [21] (upper triangle), the eigenvalues of its 3 x 3
        position block descending, their eigenvectors as the columns of V [3, 3], the status (0 usable, 1 fewer than two
        members, 2 the position block is not positive definite -- a cell whose draws start on one point) and Linv [6], the
        inverse of the lower Cholesky factor of the position block: |Linv (d - m_p)|^2 is a squared Mahalanobis distance.
        The k-sigma ellipsoid of a cell at a step has the semi-axes k sqrt(eigenvalue) along the columns of V. The
        covariance comes from raw moments: fine while |mean| / sigma stays below about 1e4 (fp32 tables) or 1e3 (fp64)."""
        if (mom.dim() != 3 or int(mom.shape[2]) != _lib.DISP_ROWS or mom.dtype != torch.float64 or mom.device != self.state.device
                or not mom.is_contiguous()):
            raise ValueError("mom must be a contiguous [count, G, 32] float64 tensor on the handle's device (dispersion())")
        count, G = int(mom.shape[0]), int(mom.shape[1])
        if G < 1:
            raise ValueError("dispersion_ellipsoids: G >= 1")
        out = self._out_arg(out, (count, G, _lib.ELL_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchDispersionEllipsoids(self.h, _ptr(mom), count, G, _ptr(out), self._stream()))
        return out

    def mahalanobis(self, ell, group, G, first=0, count=None, limit=None, after=False, ref_table=None, ref_first=0, score=None,
                    step0=None):
        """How far every robot sits from its own cell's cloud over the recorded steps first .. first + count - 1: a score
        [12, B] in the handle's dtype (umpcBatchMahalanobis; rows: robobee3d_amd/score.py -- steps scored, sum and max of
        d2 = |Linv (d - m_p)|^2 with d = p - pdes, the step of the maximum, the steps with d2 > limit and the first / last of
        them, the last d2, the steps skipped). ell [count, G, 48] = dispersion_ellipsoids() of exactly these steps; group [B]
        is the array group_index() took (ids outside [0, G) are skipped). limit None = score.chi2_3_quantile(0.99), the 99 %
        point of a Gaussian cloud in three dimensions; the covariance includes the robot itself, so d2 <= (n - 1)^2 / n and a
        larger limit never fires in a small cell. first, count, after, ref_table, ref_first, score and step0 are those of
        score(): passing a score back in accumulates a chunked run. Row 0 > 0 means "enters", as in score(): score_quantiles
        and score_bootstrap take the table unchanged (num=1, den=0 or num=2). A draw that sits 5 sigma out in a direction
        where its cell is tight is inside the isotropic tube of score() and shows here."""
        from .score import chi2_3_quantile
        hist, first, count = self._history_window("mahalanobis", first, count)
        reftab, rfirst = self._scoring_reference("mahalanobis", first, count, ref_table, ref_first)
        G = int(G)
        group = torch.as_tensor(group).to(torch.int32).to(self.device).contiguous()
        if tuple(group.shape) != (self.B,):
            raise ValueError("group must be [%d]" % self.B)
        if (tuple(ell.shape) != (count, G, _lib.ELL_ROWS) or ell.dtype != torch.float64 or ell.device != self.state.device
                or not ell.is_contiguous()):
            raise ValueError("ell must be a contiguous [%d, %d, 48] float64 tensor on the handle's device: the ellipsoids of "
                             "exactly the steps asked for" % (count, G))
        limit = chi2_3_quantile(0.99) if limit is None else float(limit)
        with torch.cuda.device(self.device):
            if score is None:
                score = torch.empty((_lib.MAHA_ROWS, self.B), dtype=self.dtype, device=self.device)
                self._check(self.L.umpcBatchMahalanobisInit(self.h, _ptr(score), self._stream()))
            else:
                self._score_arg("score", score)
            self._check(self.L.umpcBatchMahalanobis(self.h, _ptr(hist["state"]), _ptr(reftab),
                                                    None if reftab is not None else _ptr(self.ref), _ptr(ell), _ptr(group), G,
                                                    first, count, rfirst, first if step0 is None else int(step0),
                                                    int(bool(after)), limit, _ptr(score), self._stream()))
        return score

    def lag_moments(self, index, lag=1, first=0, count=None, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history, each PAIRED WITH THE STEP `lag` LATER, as the raw
        cross moments of the error state z = (p - pdes, v - dpdes) of each group [count, G, 96] float64 on the device
        (umpcBatchLagMoments; rows: robobee3d_amd/score.py X_* -- members scored / skipped, S1 and S2 of step k (a) and of
        step k + lag (b) as dispersion() gives them, and Sba = sum z_b z_a^T [6, 6]), in ONE pass over the tables: what
        propagators() turns into the linear map that carries a draw's deviation at step k to its deviation at step k + lag.
        count None = up to the history cursor minus lag: the steps [first, first + count + lag) must be recorded, and the
        reference table must cover them. index, after, ref_table, ref_first and out are those of dispersion(), and the
        reference is resolved as there. A member is scored when p, v, pdes and dpdes are finite at BOTH steps. Every (step,
        group) row is independent and bit-reproducible, and raw moments add across the blocks of a sharded job
        (score.combine_lag_moments). Keep the cells contiguous in the batch (cell = b // 64)."""
        from .score import LAG_MAX
        lag = int(lag)
        if not 1 <= lag <= LAG_MAX:
            raise ValueError("lag_moments: 1 <= lag <= %d" % LAG_MAX)
        if count is None:
            count = self.history_cursor - int(first) - lag
        hist, first, span = self._history_window("lag_moments", first, int(count) + lag if int(count) >= 0 else -1)
        count = span - lag
        order, offset, G = self._group_index_arg("lag_moments", index)
        reftab, rfirst = self._scoring_reference("lag_moments", first, span, ref_table, ref_first)
        out = self._out_arg(out, (count, G, _lib.XMOM_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchLagMoments(self.h, _ptr(hist["state"]), _ptr(reftab),
                                                   None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                                   int(bool(after)), lag, _ptr(order), _ptr(offset), G, _ptr(out), self._stream()))
        return out

    def propagators(self, xmom, out=None):
        """[count, G, 80] float64 from the lag moments [count, G, 96] of lag_moments() (umpcBatchPropagators; rows:
        robobee3d_amd/score.py P_* -- n, skipped, the status (0 usable, 1 fewer than eight members, 2 the cloud at step k is
        flat in some direction), r2 of the position and of the velocity block, growth, Phi [6, 6], c [6] and Q [21], upper
        triangle): the affine model z_{k + lag} ~ Phi z_k + c of the cell's draws, the closed-loop dynamics of that cell as
        the data show them. Q is the covariance the model leaves unexplained -- nonlinearity, saturation, unsolved steps --
        and r2 = 1 - trace(Q) / trace(C_b) per block the share it explains; growth = |L_a^-1 Phi L_a|_F^2 / 6 is the mean
        squared amplification in the cloud's own metric (below 1: the cloud contracts on average). The ellipsoid at k + lag
        predicted from the one at k is Phi C_a Phi^T + Q around Phi m_a + c. The poles are host work:
        score.propagator_poles(prop.cpu().numpy(), lag)."""
        if (xmom.dim() != 3 or int(xmom.shape[2]) != _lib.XMOM_ROWS or xmom.dtype != torch.float64 or xmom.device != self.state.device
                or not xmom.is_contiguous()):
            raise ValueError("xmom must be a contiguous [count, G, 96] float64 tensor on the handle's device (lag_moments())")
        count, G = int(xmom.shape[0]), int(xmom.shape[1])
        if G < 1:
            raise ValueError("propagators: G >= 1")
        out = self._out_arg(out, (count, G, _lib.PROP_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchPropagators(self.h, _ptr(xmom), count, G, _ptr(out), self._stream()))
        return out

    def trajectory_gram(self, index, first=0, count=None, after=False, ref_table=None, ref_first=0, scale=(1, 1, 1, 0, 0, 0),
                        out=None):
        """The recorded steps first .. first + count - 1 of the step history as the Gram matrix of the error trajectories of each
        group's draws [G, 66, 64] float64 on the device (umpcBatchGram; layout: robobee3d_amd/score.py GR_* / GT_* -- rows 0..63
        Gram[i][j] = sum over the steps and the components of y_i y_j with y = scale * (p - pdes, v - dpdes), member slot i being
        robot order[offset[g] + i]; row 64 the steps at which each slot was scored; row 65 the steps accumulated, n and the six
        scales), in ONE pass over the tables on the matrix cores (fp64 MFMA): what relates draw i of a cell to draw j as WHOLE
        flights, where every other table here is a marginal. trajectory_modes() / trajectory_table() turn it into the cell's
        medoid flight, the number of ways its draws differ and each draw's score on them. index = group_index(group, G).
        first, count, after, ref_table and ref_first are those of dispersion(), the reference is resolved as there, and the
        member rule is dispersion()'s (p, v, pdes and dpdes finite; what is not scored enters as 0 and is counted out in row
        64). scale: six finite numbers >= 0, the default is the position error alone. A cell of more than 64 members is
        flagged (rows 0..63 NaN), not computed. `out`, WHEN GIVEN, IS ACCUMULATED INTO: a chunked run passes the table of the
        first chunk back in (rewind_history() in between) -- with the same index and the same scale, which nobody checks.
        The matrix is symmetric bit for bit and bit-identical from run to run; against the numpy mirror (score.gram_reference)
        it is exact on exactly representable data and within (2 N + 2) 2^-53 sum |y_i y_j|, N = 6 x steps, otherwise: the
        order of accumulation inside an MFMA is not documented. Keep the cells contiguous in the batch (cell = b // 64)."""
        hist, first, count = self._history_window("trajectory_gram", first, count)
        order, offset, G = self._group_index_arg("trajectory_gram", index)
        reftab, rfirst = self._scoring_reference("trajectory_gram", first, count, ref_table, ref_first)
        accumulate = out is not None
        out = self._out_arg(out, (G, _lib.GRAM_ROWS, _lib.GRAM_COLS))
        scale = [float(x) for x in scale]
        if len(scale) != 6:
            raise ValueError("trajectory_gram: scale is six numbers")
        sc = (C.c_double * 6)(*scale)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchGram(self.h, _ptr(hist["state"]), _ptr(reftab),
                                             None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                             int(bool(after)), _ptr(order), _ptr(offset), G, sc, int(accumulate), _ptr(out),
                                             self._stream()))
        return out

    def _gram_arg(self, what, gram):
        if (gram.dim() != 3 or tuple(gram.shape[1:]) != (_lib.GRAM_ROWS, _lib.GRAM_COLS) or gram.dtype != torch.float64
                or gram.device != self.state.device or not gram.is_contiguous()):
            raise ValueError("%s: gram must be a contiguous [G, 66, 64] float64 tensor on the handle's device (trajectory_gram())" % what)
        return gram.cpu().numpy()

    def trajectory_modes(self, gram, M=3):
        """The ways the draws of each cell differ as whole trajectories, from the table of trajectory_gram(): a dict of numpy
        arrays (score.trajectory_modes, which documents them -- lam [G, M], share, W [G, 64, M], neff, trace, nvalid, status).
        The tables are G x 33 KB, so the small dense algebra (centring, numpy.linalg.eigh) is host work, as the poles of the
        propagators are. A draw that was not finite at any step is left out of its cell."""
        from .score import trajectory_modes
        return trajectory_modes(self._gram_arg("trajectory_modes", gram), M)

    def trajectory_table(self, gram, modes, index):
        """The score-shaped table [12, B] in the handle's dtype on the device of trajectory_gram()'s table and its
        trajectory_modes() (rows: robobee3d_amd/score.py T_* -- valid, Gram_ii, the squared distance from the cell's mean path,
        the mean and the smallest squared distance to the other draws, the nearest neighbour, the medoid flag, the rank from
        the most typical draw to the oddest, the share of the cell's variation, the scores on the first three modes). Row 0
        is the score's "enters": score_quantiles / score_bootstrap / score_sensitivity take the table unchanged, e.g.
        score_sensitivity(table, index, bins, nbins, num=9) asks which drawn input explains mode 0. (Robot indices in row 5
        are exact in fp32 up to 2^24.)"""
        from .score import trajectory_table
        order, offset, G = self._group_index_arg("trajectory_table", index)
        g = self._gram_arg("trajectory_table", gram)
        if g.shape[0] != G:
            raise ValueError("trajectory_table: gram has %d cells, the index %d" % (g.shape[0], G))
        tab = trajectory_table(g, modes, order.cpu().numpy(), offset.cpu().numpy(), self.B)
        return torch.as_tensor(tab).to(self.dtype).to(self.device).contiguous()

    def mode_weights(self, modes, index, M=None):
        """weights [M, B] float64 on the device for ensemble_projection() from the eigenvectors of trajectory_modes(): robot
        order[offset[g] + i] gets W[g][i][m], a robot outside every usable cell 0 (score.mode_weights)."""
        from .score import mode_weights
        order, offset, _ = self._group_index_arg("mode_weights", index)
        return torch.as_tensor(mode_weights(modes, order.cpu().numpy(), offset.cpu().numpy(), self.B, M)).to(self.device).contiguous()

    def ensemble_projection(self, index, weights, first=0, count=None, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history as weighted sums of the error state over each group's
        draws [count, G, 32] float64 on the device (umpcBatchProject; rows: robobee3d_amd/score.py P_* -- members scored /
        skipped, then row 2 + 6 m + c = sum_b weights[m][b] z_c(b) for the M <= 4 weight vectors): dispersion() with S1 weighted
        and S2 dropped. weights [M, B] float64 by robot -- mode_weights() of a cell's eigenvectors gives the time course of its
        modes, 1 / n the mean path, +-1 on two clusters their contrast. A member is scored when p, v, pdes, dpdes and its M
        weights are finite. index, first, count, after, ref_table, ref_first and out are those of dispersion(). Bit-identical to
        score.project_reference, for every cell size."""
        hist, first, count = self._history_window("ensemble_projection", first, count)
        order, offset, G = self._group_index_arg("ensemble_projection", index)
        reftab, rfirst = self._scoring_reference("ensemble_projection", first, count, ref_table, ref_first)
        if not torch.is_tensor(weights):
            weights = torch.as_tensor(np.asarray(weights, np.float64)).to(self.device)
        if (weights.dim() != 2 or not 1 <= int(weights.shape[0]) <= _lib.PROJ_MAX or int(weights.shape[1]) != self.B
                or weights.dtype != torch.float64 or weights.device != self.state.device or not weights.is_contiguous()):
            raise ValueError("weights must be a contiguous [M, %d] float64 tensor on the handle's device, 1 <= M <= 4" % self.B)
        out = self._out_arg(out, (count, G, _lib.PROJ_ROWS))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchProject(self.h, _ptr(hist["state"]), _ptr(reftab),
                                                None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                                int(bool(after)), _ptr(order), _ptr(offset), G, _ptr(weights),
                                                int(weights.shape[0]), _ptr(out), self._stream()))
        return out

    def _bins_arg(self, what, bins, nbins):
        from .score import SENS_MAX_BINS, SENS_MAX_FACTORS
        M = int(nbins)
        if (bins.dim() != 2 or int(bins.shape[1]) != self.B or bins.dtype != torch.int32 or bins.device != self.state.device
                or not bins.is_contiguous()):
            raise ValueError("%s: bins must be a contiguous [F, %d] int32 tensor on the handle's device (factor_bins())" % (what, self.B))
        F = int(bins.shape[0])
        if not 1 <= F <= SENS_MAX_FACTORS or not 2 <= M <= SENS_MAX_BINS:
            raise ValueError("%s: 1 to %d factors, 2 to %d bins" % (what, SENS_MAX_FACTORS, SENS_MAX_BINS))
        return F, M

    def factor_bins(self, factors, index, nbins=8):
        """bins [F, B] int32 on the device (umpcBatchFactorBins), once per sweep: each of the F drawn inputs `factors` [F, B] --
        initial offsets, tilts, push sizes, a task parameter, a weight: whatever the sweep drew per robot -- cut into `nbins`
        bins of equal count INSIDE each cell of index = group_index(group, G), by rank (numpy.argsort(kind="stable") over the
        cell's member list; bin = rank * nbins // finite members). -1 for a value that is not finite and for a robot outside
        every group. What sensitivity() and score_sensitivity() take. A categorical factor (a push direction index) is its own
        bin: write that row by hand. 1 to 6 factors, 2 to 8 bins."""
        from .score import SENS_MAX_BINS, SENS_MAX_FACTORS
        order, offset, G = self._group_index_arg("factor_bins", index)
        factors = torch.as_tensor(factors).to(self.dtype).to(self.device).contiguous()
        if factors.dim() == 1:
            factors = factors[None]
        F, M = int(factors.shape[0]), int(nbins)
        if factors.dim() != 2 or int(factors.shape[1]) != self.B:
            raise ValueError("factors must be [F, %d]" % self.B)
        if not 1 <= F <= SENS_MAX_FACTORS or not 2 <= M <= SENS_MAX_BINS:
            raise ValueError("factor_bins: 1 to %d factors, 2 to %d bins" % (SENS_MAX_FACTORS, SENS_MAX_BINS))
        bins = torch.empty((F, self.B), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchFactorBins(self.h, _ptr(factors), F, _ptr(order), _ptr(offset), G, M, _ptr(bins), self._stream()))
        return bins

    def sensitivity(self, index, bins, nbins, term="ep", first=0, count=None, after=False, ref_table=None, ref_first=0, out=None):
        """The recorded steps first .. first + count - 1 of the step history as the binned sums of a term over the drawn inputs
        [count, G, 4 + 2 F nbins] float64 on the device (umpcBatchSensitivity; rows: robobee3d_amd/score.py S_* -- members
        scored / skipped, S1 = sum y, S2 = sum y^2, then per factor f and bin m the scored members N_fm and S_fm = sum y over
        them), in ONE pass over the tables: what sensitivity_indices() turns into the share of a cell's error variance that
        each drawn input explains. bins = factor_bins(factors, index, nbins) (or written by hand); term, index, first, count,
        after, ref_table, ref_first and out are those of ensemble_quantiles(), and the reference is resolved as there. A member
        is scored when ensemble_quantiles() scores it and all its bins lie in [0, nbins). Every (step, group) row is independent
        and bit-reproducible, and raw sums ADD across the blocks of a sharded job when the bins were assigned on the whole job
        (score.combine_sensitivities). Keep the cells contiguous in the batch (cell = b // 64)."""
        from .score import TERM_NAMES, sens_cols
        hist, first, count = self._history_window("sensitivity", first, count)
        order, offset, G = self._group_index_arg("sensitivity", index)
        F, M = self._bins_arg("sensitivity", bins, nbins)
        if term not in TERM_NAMES:
            raise ValueError("sensitivity: term is one of %s" % (TERM_NAMES,))
        if term == "tau" and hist["out"] is None:
            raise RuntimeError("sensitivity: term 'tau' needs the out record of the step history")
        reftab, rfirst = self._scoring_reference("sensitivity", first, count, ref_table, ref_first)
        out = self._out_arg(out, (count, G, sens_cols(F, M)))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchSensitivity(self.h, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(reftab),
                                                    None if reftab is not None else _ptr(self.ref), first, count, rfirst,
                                                    int(bool(after)), _ptr(order), _ptr(offset), G, TERM_NAMES.index(term),
                                                    _ptr(bins), F, M, _ptr(out), self._stream()))
        return out

    def sensitivity_indices(self, sens, F, nbins, out=None):
        """[count, G, 8 + F (4 + nbins)] float64 from the sums [count, G, 4 + 2 F nbins] of sensitivity(), or [G, ..] from the
        [G, ..] of score_sensitivity() (umpcBatchSensitivityIndices; rows: robobee3d_amd/score.py I_* -- n, skipped, the
        status (0 usable, 1 fewer than 2 nbins members, 2 the term does not vary in the cell), mean, variance and SST of the
        term, then per factor eta2 = SSB / SST, the correlation ratio: the share of the cell's variance that goes away when
        that input is known; eps2, the same adjusted for the (M_f - 1) / (n - 1) that eta2 shows with no effect at all; the
        one-way ANOVA F; the non-empty bins M_f; and the bin means, the main-effect curve E[y | bin]). First-order indices:
        they need not add up to 1, the rest is interaction and noise. Nothing is clamped."""
        from .score import SENS_MAX_BINS, SENS_MAX_FACTORS, sens_cols, sens_index_cols
        F, M = int(F), int(nbins)
        if not 1 <= F <= SENS_MAX_FACTORS or not 2 <= M <= SENS_MAX_BINS:
            raise ValueError("sensitivity_indices: 1 to %d factors, 2 to %d bins" % (SENS_MAX_FACTORS, SENS_MAX_BINS))
        if (sens.dim() not in (2, 3) or int(sens.shape[-1]) != sens_cols(F, M) or sens.dtype != torch.float64
                or sens.device != self.state.device or not sens.is_contiguous()):
            raise ValueError("sens must be a contiguous [count, G, %d] (or [G, %d]) float64 tensor on the handle's device "
                             "(sensitivity(), score_sensitivity())" % (sens_cols(F, M), sens_cols(F, M)))
        flat = sens.dim() == 2
        count, G = (1, int(sens.shape[0])) if flat else (int(sens.shape[0]), int(sens.shape[1]))
        if G < 1:
            raise ValueError("sensitivity_indices: G >= 1")
        if flat and out is not None:
            out = out[None]
        out = self._out_arg(out, (count, G, sens_index_cols(F, M)))
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchSensitivityIndices(self.h, _ptr(sens), count, G, F, M, _ptr(out), self._stream()))
        return out[0] if flat else out

    def score_sensitivity(self, score, index, bins, nbins, num, den=None):
        """[G, 4 + 2 F nbins] float64: the sums of sensitivity() over one column of a per-robot score over the robots of each
        group (umpcBatchScoreSensitivity). The value of robot b is that of score_quantiles() (score[num, b], or score[num, b] /
        score[den, b] in double: num = 1, den = 0 is the per-robot mean tracking error); it enters when its row 0 > 0, the
        value is finite and all its bins lie in [0, nbins). sensitivity_indices(result, F, nbins) says which drawn input
        explains the spread of a cell's cost."""
        from .score import sens_cols
        order, offset, G = self._group_index_arg("score_sensitivity", index)
        self._score_arg("score", score)
        F, M = self._bins_arg("score_sensitivity", bins, nbins)
        sens = torch.empty((G, sens_cols(F, M)), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchScoreSensitivity(self.h, _ptr(score), _ptr(order), _ptr(offset), G, int(num),
                                                         -1 if den is None else int(den), _ptr(bins), F, M, _ptr(sens), self._stream()))
        return sens

    def spectrum(self, freq_hz, signal="ep", window="hann", first=0, count=None, after=False, ref_table=None, ref_first=0,
                 sums=None, basis=None, basis_first=0, split_hz=None, power=True):
        """The spectrum of every robot's tracking error ("ep": p - pdes), attitude error ("es": s - sdes) or command ("u": out
        rows 0..2 as recorded) over the recorded steps first .. first + count - 1 of the step history, at the K <= 64
        frequencies freq_hz [K] in Hz, in ONE pass over the tables on the device (umpcBatchSpectrum / umpcBatchSpectrumPower;
        rows: robobee3d_amd/score.py SPEC_* and SSUM_*) -- the oscillation nobody asked for, where frequency_response() fits
        one frequency known in advance. Returns (spec, power, sums): spec [3, 12, B] in the handle's dtype -- per channel the
        steps that entered (0 when the fit is refused: a skipped step, fewer than two steps, or no power at all; the rows
        behind and the channel's power are then NaN), the steps skipped as not finite, the windowed mean and variance, the
        total power over the K bins, the peak bin, its frequency, power and share of the total, the spectral centroid and
        bandwidth in Hz, and the share of the power at or above split_hz (the chatter score; split_hz None: 0) --, power
        [3, K, B] the periodogram P_j (an on-grid sinusoid of amplitude a gives a^2), sums [2 + 3 (2 + 2 K), B] float64 the
        raw projections. Every frequency must lie strictly between 0 and half the step rate (nu = freq_hz * 1e-3 * nsub *
        dtsim revolutions per step, score.response_nu). first, count, after, ref_table and ref_first are those of score()
        and the reference is resolved as there; "u" needs the out record and reads no reference. The cosines and sines
        come from a host-made table (score.spectrum_basis: window "hann" or "rect" over the count steps of the call):
        nothing of the tables' size is allocated. A chunked run makes the table of the WHOLE window once, uploads it and
        passes it as `basis` [W, 1 + 2 K] with basis_first = the steps already run, the sums passed back in and power=False
        (spec and power are None) until the last chunk: with `sums` given the mean is removed over the basis rows 0 ..
        basis_first + count - 1, which must be the steps the sums hold. spec[c] is shaped as a score: score_quantiles(spec[0],
        index, [0.5], SPEC_HIGH_SHARE) is a cell's median chatter score; spectrum_groups() averages the periodograms."""
        from . import score as S
        sig = S._spectrum_signal(signal)
        hist, first, count = self._history_window("spectrum", first, count)
        freq = np.ascontiguousarray(np.atleast_1d(np.asarray(freq_hz, np.float64)))
        if freq.ndim != 1 or not 1 <= len(freq) <= _lib.SPEC_MAX_K:
            raise ValueError("spectrum: freq_hz must hold 1 to %d frequencies" % _lib.SPEC_MAX_K)
        K = len(freq)
        nu = S.response_nu(freq, int(self.prm.nsub), float(self.prm.dtsim))
        if not np.all((nu > 0.0) & (nu < 0.5)):
            raise ValueError("spectrum: every frequency must lie strictly between 0 and half the step rate")
        reftab, rfirst = None, 0
        if sig == _lib.SPEC_U:
            if hist["out"] is None:
                raise RuntimeError("spectrum: signal 'u' needs a step history with the out record (record_history)")
        else:
            reftab, rfirst = self._scoring_reference("spectrum", first, count, ref_table, ref_first)
        basis_first = int(basis_first)
        if basis is None:
            if basis_first != 0 or sums is not None:
                raise ValueError("spectrum: a chunked run (sums or basis_first given) needs the basis of the whole window")
            host = S.spectrum_basis(nu, max(count, 1), window)
            basis = torch.as_tensor(host).to(self.device)
        else:
            if (basis.dim() != 2 or int(basis.shape[1]) != 1 + 2 * K or basis.dtype != torch.float64
                    or basis.device != self.state.device or not basis.is_contiguous()):
                raise ValueError("basis must be a contiguous [W, %d] float64 tensor on the handle's device" % (1 + 2 * K))
            if basis_first < 0 or basis_first + count > int(basis.shape[0]):
                raise ValueError("spectrum: the basis does not cover the steps asked for")
            host = None
        rows = S.spectrum_sum_rows(K)
        fresh = sums is None
        jsplit = K
        if split_hz is not None:
            if np.any(np.diff(freq) <= 0):
                raise ValueError("spectrum: split_hz needs ascending frequencies")
            jsplit = int(np.searchsorted(freq, float(split_hz), side="left"))
        with torch.cuda.device(self.device):
            if fresh:
                sums = torch.empty((rows, self.B), dtype=torch.float64, device=self.device)
                self._check(self.L.umpcBatchSpectrumInit(self.h, K, _ptr(sums), self._stream()))
            elif (tuple(sums.shape) != (rows, self.B) or sums.dtype != torch.float64 or sums.device != self.state.device
                  or not sums.is_contiguous()):
                raise ValueError("sums must be a contiguous [%d, %d] float64 tensor on the handle's device" % (rows, self.B))
            self._check(self.L.umpcBatchSpectrum(self.h, sig, _ptr(hist["state"]), _ptr(hist["out"]), _ptr(reftab),
                                                 None if reftab is not None or sig == _lib.SPEC_U else _ptr(self.ref),
                                                 _ptr(basis), basis_first, K, first, count, rfirst, int(bool(after)),
                                                 _ptr(sums), self._stream()))
            spec = pw = None
            if power:
                # the rows the sums hold: this call's alone, or with `sums` passed in everything from row 0
                lo, n = (basis_first, count) if fresh else (0, basis_first + count)
                wsum = S.spectrum_wsum(basis.cpu().numpy() if host is None else host, lo, n)
                spec = torch.empty((3, _lib.SPEC_ROWS, self.B), dtype=self.dtype, device=self.device)
                pw = torch.empty((3, K, self.B), dtype=self.dtype, device=self.device)
                self._check(self.L.umpcBatchSpectrumPower(self.h, _ptr(sums), wsum.ctypes.data_as(C.POINTER(C.c_double)),
                                                          freq.ctypes.data_as(C.POINTER(C.c_double)), K, n, jsplit, _ptr(pw),
                                                          _ptr(spec), self._stream()))
        return spec, pw, sums

    def spectrum_groups(self, power, spec, index):
        """[G, 3, 2 + K] float64: per group and channel the members that enter (row 0 of spec[c] > 0), the members that do
        not, and the periodogram of spectrum() summed over the members that enter (umpcBatchSpectrumGroups) -- column 2 + j
        divided by column 0 is the cell's averaged periodogram, the consistent estimate of the cell's spectrum that a
        Monte-Carlo sweep provides for free. index = group_index(group, G). A row is a function of the group's member list
        alone and bit-reproducible; raw sums ADD over the blocks of a sharded job (score.combine_spectra)."""
        order, offset, G = self._group_index_arg("spectrum_groups", index)
        if G < 1:
            raise ValueError("spectrum_groups: G >= 1")
        for t, name in ((power, "power"), (spec, "spec")):
            if t.dim() != 3 or t.dtype != self.dtype or t.device != self.state.device or not t.is_contiguous():
                raise ValueError("%s must be a contiguous tensor of the handle's dtype on its device (spectrum())" % name)
        K = int(power.shape[1])
        if tuple(power.shape) != (3, K, self.B) or not 1 <= K <= _lib.SPEC_MAX_K or tuple(spec.shape) != (3, _lib.SPEC_ROWS, self.B):
            raise ValueError("power must be [3, K, %d] with 1 <= K <= 64 and spec [3, 12, %d]" % (self.B, self.B))
        gspec = torch.empty((G, 3, 2 + K), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchSpectrumGroups(self.h, _ptr(power), _ptr(spec), _ptr(order), _ptr(offset), G, K,
                                                       _ptr(gspec), self._stream()))
        return gspec

    def transfer(self, freq_hz, index, pair="track", window="hann", first=0, count=None, after=False, ref_table=None, ref_first=0,
                 impulses=None, imp_first=None, sums=None, basis=None, basis_first=0, rows=True):
        """The transfer function of every grid cell from an input x to an output y over the recorded steps first .. first +
        count - 1 of the step history, at the K <= 64 frequencies freq_hz [K] in Hz: the H1 estimate, the coherence and the
        random error per frequency, from the cell's draws as independent records of one closed loop (umpcBatchCrossSpectrum /
        umpcBatchCrossSpectrumGroups / umpcBatchTransfer; rows: robobee3d_amd/score.py TF_*, GX_*). pair "track": x = pdes, y = p;
        "att": x = sdes, y = s -- both read the reference TABLE (ref_table, else that of set_reference_trajectory): a constant
        reference has no spectrum --; "push": x = dv_world of the impulse table (`impulses` [steps, 6, B], default the table of
        set_impulses, read at slice imp_first + step; imp_first defaults to the impulse cursor at the start of the record plus
        `first`), y = p - pdes against the reference resolved as score() does. index = group_index(group, G). Returns (tf, gx,
        sums): tf [G, 3, K, 12] float64 -- per cell, channel and frequency the draws that entered (0 when the row is refused:
        fewer than two, or no input power), the draws that did not (a skipped step), Pxx, Pyy, h_re, h_im, gain, phase
        (negative: y lags x, as in frequency_response), coh, gain_h2 (gain <= |H| <= gain_h2), rel_err (the normalised random
        error of the gain = the standard deviation of the phase in rad) and the unexplained output power --, gx [G, 3, 2 + 4 K]
        the raw cell sums (they add over shards: score.combine_cross_spectra, then transfer_rows), sums [2 + 6 (2 + 2 K), B]
        float64 the raw projections. freq_hz, window, first, count, after, ref_table, ref_first, basis, basis_first and sums
        are those of spectrum(): a chunked run passes the basis of the WHOLE window, basis_first = the steps already run, the
        sums back in and rows=False (tf and gx are None) until the last chunk. Nothing of the tables' size is allocated."""
        from . import score as S
        pr = S._cross_pair(pair)
        order, offset, G = self._group_index_arg("transfer", index)
        if G < 1:
            raise ValueError("transfer: G >= 1")
        hist, first, count = self._history_window("transfer", first, count)
        freq = np.ascontiguousarray(np.atleast_1d(np.asarray(freq_hz, np.float64)))
        if freq.ndim != 1 or not 1 <= len(freq) <= _lib.SPEC_MAX_K:
            raise ValueError("transfer: freq_hz must hold 1 to %d frequencies" % _lib.SPEC_MAX_K)
        K = len(freq)
        nu = S.response_nu(freq, int(self.prm.nsub), float(self.prm.dtsim))
        if not np.all((nu > 0.0) & (nu < 0.5)):
            raise ValueError("transfer: every frequency must lie strictly between 0 and half the step rate")
        reftab, rfirst = self._scoring_reference("transfer", first, count, ref_table, ref_first)
        imptab, ifirst = None, 0
        if pr == _lib.XS_PUSH:
            imptab = getattr(self, "_imptab", None) if impulses is None else impulses
            if imptab is None:
                raise RuntimeError("transfer: pair 'push' needs an impulse table (set_impulses, or impulses=)")
            if (imptab.dim() != 3 or tuple(imptab.shape[1:]) != (6, self.B) or imptab.dtype != self.dtype
                    or imptab.device != self.state.device or not imptab.is_contiguous()):
                raise ValueError("impulses must be a contiguous [steps, 6, %d] tensor of the handle's dtype on its device" % self.B)
            ifirst = self._hist_imp0 + first if imp_first is None else int(imp_first)
            if ifirst < 0 or ifirst + count > int(imptab.shape[0]):
                raise ValueError("transfer: the impulse table does not cover the steps asked for")
        elif reftab is None:
            raise RuntimeError("transfer: pair '%s' needs a reference table (set_reference_trajectory, or ref_table=): a constant "
                               "reference has no spectrum" % S.XS_PAIRS[pr])
        basis_first = int(basis_first)
        if basis is None:
            if basis_first != 0 or sums is not None:
                raise ValueError("transfer: a chunked run (sums or basis_first given) needs the basis of the whole window")
            host = S.spectrum_basis(nu, max(count, 1), window)
            basis = torch.as_tensor(host).to(self.device)
        else:
            if (basis.dim() != 2 or int(basis.shape[1]) != 1 + 2 * K or basis.dtype != torch.float64
                    or basis.device != self.state.device or not basis.is_contiguous()):
                raise ValueError("basis must be a contiguous [W, %d] float64 tensor on the handle's device" % (1 + 2 * K))
            if basis_first < 0 or basis_first + count > int(basis.shape[0]):
                raise ValueError("transfer: the basis does not cover the steps asked for")
            host = None
        nsum = S.cross_spectrum_sum_rows(K)
        fresh = sums is None
        with torch.cuda.device(self.device):
            if fresh:
                sums = torch.empty((nsum, self.B), dtype=torch.float64, device=self.device)
                self._check(self.L.umpcBatchCrossSpectrumInit(self.h, K, _ptr(sums), self._stream()))
            elif (tuple(sums.shape) != (nsum, self.B) or sums.dtype != torch.float64 or sums.device != self.state.device
                  or not sums.is_contiguous()):
                raise ValueError("sums must be a contiguous [%d, %d] float64 tensor on the handle's device" % (nsum, self.B))
            self._check(self.L.umpcBatchCrossSpectrum(self.h, pr, _ptr(hist["state"]), _ptr(reftab),
                                                      _ptr(self.ref) if pr == _lib.XS_PUSH and reftab is None else None,
                                                      _ptr(imptab), _ptr(basis), basis_first, K, first, count, rfirst, ifirst,
                                                      int(bool(after)), _ptr(sums), self._stream()))
            tf = gx = None
            if rows:
                # the rows the sums hold: this call's alone, or with `sums` passed in everything from row 0
                lo, n = (basis_first, count) if fresh else (0, basis_first + count)
                wsum = S.spectrum_wsum(basis.cpu().numpy() if host is None else host, lo, n)
                gx = torch.empty((G, 3, 2 + 4 * K), dtype=torch.float64, device=self.device)
                self._check(self.L.umpcBatchCrossSpectrumGroups(self.h, _ptr(sums), wsum.ctypes.data_as(C.POINTER(C.c_double)), K, n,
                                                                _ptr(order), _ptr(offset), G, _ptr(gx), self._stream()))
                tf = self.transfer_rows(gx)
        return tf, gx, sums

    def transfer_rows(self, gx):
        """tf [G, 3, K, 12] float64 from the cell sums gx [G, 3, 2 + 4 K] of transfer() (umpcBatchTransfer alone): for tables
        combined over the shards of a job or the column blocks of a cell (score.combine_cross_spectra)."""
        if (gx.dim() != 3 or int(gx.shape[1]) != 3 or gx.dtype != torch.float64 or gx.device != self.state.device
                or not gx.is_contiguous() or int(gx.shape[0]) < 1 or int(gx.shape[2]) < 6 or (int(gx.shape[2]) - 2) % 4 != 0
                or (int(gx.shape[2]) - 2) // 4 > _lib.SPEC_MAX_K):
            raise ValueError("gx must be a contiguous [G, 3, 2 + 4 K] float64 tensor on the handle's device, 1 <= K <= 64 (transfer())")
        G, K = int(gx.shape[0]), (int(gx.shape[2]) - 2) // 4
        tf = torch.empty((G, 3, K, _lib.TF_ROWS), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchTransfer(self.h, _ptr(gx), G, K, _ptr(tf), self._stream()))
        return tf

    def task_table(self, steps, tasks=None, t_ms=None, **params):
        """[steps, 9, B] tensor for set_reference_trajectory: the generators of set_task evaluated PER ROBOT on the device
        at the fire times t_ms + k * nsub * dtsim (umpcBatchTaskTable; t_ms None = the handle's clock). tasks: a name of
        TASKS, a length-B sequence of names, or None (= the handle's task); every keyword of TASKS (trajAmp, trajFreq, dz,
        useY, tduration, vdes, tstart, tend, trotstart, trotend) a scalar or a [B] array, defaults as set_task for the
        robot's task. Rows 0..2 of `self.ref` are the robots' initialPos ("ref" robots copy their whole column)."""
        steps = int(steps)
        tid, prm = self._task_tensors(tasks, params)
        tab = torch.empty((steps, _lib.REF_ROWS, self.B), dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchTaskTable(self.h, steps, self.time_ms if t_ms is None else float(t_ms), _ptr(tid),
                                                  _ptr(prm), _ptr(self.ref), _ptr(tab), self._stream()))
        return tab

    def _task_tensors(self, tasks, params):
        """task_arrays on the device, in the handle's dtype: (ids [B] int32, params [4, B]), or (None, None) when neither names
        nor keywords are given (= the handle's task)."""
        if tasks is None and not params:
            return None, None
        by_id = {v[0]: k for k, v in TASKS.items()}
        ids, P = task_arrays(self.B, tasks, params, by_id[self._task_id()])
        return torch.as_tensor(ids).to(self.device), torch.as_tensor(P).to(self.dtype).to(self.device).contiguous()

    def set_weights(self, weights):
        """Per-robot objective weights [8, B] = (ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom), or None."""
        if weights is None:
            self._weights = None
            self._check(self.L.umpcBatchSetWeights(self.h, None))
            return
        w = torch.as_tensor(weights, dtype=self.dtype).to(self.device).contiguous()
        assert w.shape == (8, self.B)
        self._weights = w  # keep alive: the library stores the pointer
        self._check(self.L.umpcBatchSetWeights(self.h, _ptr(w)))

    def set_step_kernel(self, mode):
        """"auto" (default: the all-assembly fp32 kernel / the fp64 kernel with the assembly ADMM loop where they apply)
        or "cpp" (fp32: the C++ kernel around the assembly ADMM loop; fp64: the C++ loop): ablation and cross-checks.
        "lane" / "quad" pin the form of the assembly path (one lane / one lane quad per robot; "auto" takes the quad form for
        B <= 16 384 in fp32, B <= 4 096 in fp64, counted on `global_batch`, the size of the WHOLE job, so that a shard takes the
        form the undivided batch takes): equal up to rounding, not bit for bit."""
        self._check(self.L.umpcBatchSetStepKernel(self.h, {"auto": 0, "cpp": 1, "lane": 2, "quad": 3}[mode]))

    M0_CA6 = (100.0, 100.0, 100.0, 3333.0, 3333.0, 1000.0)   # dynamicsTerms, template/ca6dynamics.py:5-10

    def set_wl(self, wl, Mdiag=M0_CA6):
        """Fuse the wrench-linearisation step into every MPC step (robobee_test_controllers.py:162-171):
        accdes -> (u4, w0) = wlConUpdate(h0, M0 accdes) -> actualT0 = w0[2] / M0[2,2] for the next step.
        wl: a BatchWLCon of the same B / dtype / device (its `u` [4,B] is the per-robot WL state, its `w0` [6,B]
        receives the wrench), or None to switch the coupling off."""
        if wl is None:
            self._wl = None
            self._check(self.L.umpcBatchSetWL(self.h, None, None, None, None))
            return
        assert wl.B == self.B and wl.dtype == self.dtype and wl.u.is_contiguous() and wl.w0.is_contiguous()
        self._wl = wl   # keeps u / w0 alive: the library stores the pointers
        md = (C.c_double * 6)(*[float(v) for v in Mdiag])
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchSetWL(self.h, C.byref(wl.wl), md, _ptr(wl.u), _ptr(wl.w0)))

    @property
    def kernel_name(self):
        """The kernel the last rollout() / update() of this handle dispatched (umpcBatchKernelName)."""
        return self.L.umpcBatchKernelName(self.h).decode()

    @property
    def time_ms(self):
        return float(self.L.umpcBatchTime(self.h))

    def rollout(self, K=1):
        """K closed-loop MPC steps (QP + nsub plant substeps each) in one launch."""
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchRollout(self.h, int(K), _ptr(self.state), _ptr(self.ctrl), _ptr(self.ref),
                                                _ptr(self.actualT0), _ptr(self.Ib), _ptr(self.gain), _ptr(self.out),
                                                _ptr(self.stats), _ptr(self.status), _ptr(self.info), self._stream()))

    def reactive_rollout(self, nsteps, gains=None, every=1):
        """controlTest(useMPC=False) (template/uprightmpc2.py:121-151) for every robot: `nsteps` plant substeps with
        reactiveController (template/template_controllers.py:282-296) evaluated every `every` substeps. gains:
        [6, B] tensor (kpos0, kpos1, kz0, kz1, ks0, ks1) or None for the reference's defaults. Last command in
        self.out[0:3]; statistics accumulate in self.stats."""
        if gains is not None:
            gains = torch.as_tensor(gains, dtype=self.dtype, device=self.device).contiguous()
            assert gains.shape == (6, self.B)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchReactive(self.h, int(nsteps), int(every), _ptr(self.state), _ptr(self.ref),
                                                 _ptr(gains), _ptr(self.Ib), _ptr(self.gain), _ptr(self.out),
                                                 _ptr(self.stats), self._stream()))

    def reactive_steps(self, K, gains=None, every=1, tasks=None, **params):
        """The reactive baseline on the tables of rollout() (umpcBatchReactiveRollout): K closed-loop steps of nsub plant
        substeps in one launch, reactiveController fired at the substeps j of a step with j % every == 0 (`every` divides
        nsub). It reads what rollout() reads and records what rollout() records, so an MPC-versus-reactive sweep over tasks x
        gains x pushes is two launches scored the same way:
        the reference is the table of set_reference_trajectory when one is set (pdes of slice ref_cursor + k, held over the
        step), else per-robot tasks when `tasks` / task keywords are given (as in task_table: a name, B names, keywords as
        scalars or [B] arrays; rows 0..2 of self.ref are initialPos, "ref" robots follow their column), else the handle's
        task -- then the call equals reactive_rollout(K * nsub, gains, every) bit for bit; the table of set_impulses kicks
        after the last substep of every step; record_history tables take the state before / after every step, the last
        command of the step in rows 0..2 of `out` (rows 3..8 = 0: there is no accdes), status 1 and info 0, so score() and
        score_groups() apply as they are (score a per-robot task run with ref_table=task_table(...)). Robots of different
        tasks inside one wavefront (64 consecutive robots) take turns in the generators: keep the robots of one task adjacent.
        gains: [6, B] (kpos0, kpos1, kz0, kz1, ks0, ks1) or None. Raises before anything is launched when a table would be
        overrun; the clock and the cursors then stay where they were."""
        if gains is not None:
            gains = torch.as_tensor(gains, dtype=self.dtype, device=self.device).contiguous()
            assert gains.shape == (6, self.B)
        tid, prm = self._task_tensors(tasks, params)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchReactiveRollout(self.h, int(K), int(every), _ptr(self.state), _ptr(self.ref), _ptr(gains),
                                                        _ptr(tid), _ptr(prm), _ptr(self.Ib), _ptr(self.gain), _ptr(self.out),
                                                        _ptr(self.stats), self._stream()))

    def task_reference(self, t_ms):
        """(pdes, dpdes, sdes) [9, B] of the current task at time t_ms (template/flight_tasks.py:6-49)."""
        out = torch.empty((9, self.B), dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchTaskReference(self.h, float(t_ms), _ptr(self.ref), _ptr(out), self._stream()))
        return out

    def control_test_log(self, tend, robots=(0,), use_mpc=True, gains=None, fire=None, impulses=None):
        """The log of controlTest (template/uprightmpc2.py:113,150-159) for the selected robots, in the reference's
        layout -- a dict {'t' [Nt], 'y' [Nt, 12] = (p, Rb[:, 2], dq), 'u' [Nt, 3], 'pdes' [Nt, 3], 'accdes' [Nt, 6]}
        per robot that viewControlTestLog / logMetric (:14-84, :161-175) take as is -- plus 'metric'. The loop runs
        from the current state, one launch per substep: this is the logging path, not the throughput path.
        fire: None = the fixed schedule (an MPC step every nsub substeps, the first at substep 0), or the substep
        indices at which the MPC fires -- the reference fires when `tt[ti] - thlPrev > hlInterval` (:136), which in
        floating point gives gaps of 25 / 26 substeps starting at substep 26; before the first fire the command is
        zero (:118) and between fires it is held.
        impulses: {substep: [6] or [6, B]} -- (dv_world, domega_body) added to the state AHEAD of that substep's fire and
        plant, where the reference kicks (`dq[1] += 2` at the first substep past tpert, :130-133, is {ti: (0, 2, 0, 0, 0, 0)}).
        This loop applies them itself; a table of set_impulses is for rollout() and must not be set on the handle here.
        Returns {robot: log}."""
        nsub, dts = int(self.prm.nsub), float(self.prm.dtsim)
        if getattr(self, "_imptab", None) is not None:
            raise RuntimeError("control_test_log applies its own `impulses`; switch the table off first (set_impulses(None))")
        kicks = {}
        for k, vec in (impulses or {}).items():
            vec = torch.as_tensor(np.asarray(vec, np.float64)).to(self.dtype).to(self.device)
            if vec.shape not in ((6,), (6, self.B)):
                raise ValueError("an impulse is [6] or [6, %d], got %r" % (self.B, tuple(vec.shape)))
            kicks[int(k)] = vec[:, None] if vec.dim() == 1 else vec
        Nt = int(np.ceil(tend / dts - 1e-9))
        idx = torch.as_tensor(list(robots), device=self.device)
        rec = {k: [] for k in ("y", "u", "pdes", "accdes", "R")}
        t_start = self.time_ms
        acc_now = torch.zeros((6, len(robots)), dtype=self.dtype, device=self.device)
        tl = float(self.prm.taulim)
        fire_at = None if fire is None else {int(i) for i in np.asarray(fire).ravel()}
        u = torch.zeros((3, self.B), dtype=self.dtype, device=self.device)      # uquad = np.zeros(3), :118
        for ti in range(Nt):
            t = t_start + ti * dts
            fire = (ti % nsub == 0) if fire_at is None else (ti in fire_at)
            if ti in kicks:
                self.state[12:18] += kicks[ti]
            if use_mpc and fire:
                self._check(self.L.umpcBatchSetTask(self.h, self._task_id(), self._task_params(), t))
                self.update()
                u = self.out[0:3].clone()
                acc_now = self.out[3:9][:, idx].clone()
            pd = self.task_reference(t)[0:3][:, idx]
            if use_mpc:
                u[1:3].clamp_(-tl, tl)
                self.plant(u, 1)
                ulog = u[:, idx]
            else:
                self.reactive_rollout(1, gains)
                ulog = self.out[0:3][:, idx]
            st = self.state[:, idx]
            rec["y"].append(torch.cat((st[0:3], st[9:12], st[12:18]), 0).T.cpu().numpy().copy())
            rec["R"].append(st[3:12].T.cpu().numpy().copy())          # column-major Rb (for save_viewlog's quaternion)
            rec["u"].append(ulog.T.cpu().numpy().copy())
            rec["pdes"].append(pd.T.cpu().numpy().copy())
            rec["accdes"].append((acc_now if (use_mpc and fire) else torch.zeros_like(acc_now)).T.cpu().numpy().copy())
        if use_mpc:   # leave the handle's clock where the loop ended
            self._check(self.L.umpcBatchSetTask(self.h, self._task_id(), self._task_params(), t_start + Nt * dts))
        logs = {}
        tt = np.arange(Nt) * dts
        for c, r in enumerate(robots):
            lg = {"t": tt.copy()}
            for k in rec:
                lg[k] = np.stack([a[c] for a in rec[k]]).astype(np.float64)
            perr, tau = lg["y"][:, :3], lg["u"][:, 1:3]
            lg["metric"] = (float((perr ** 2).sum() / Nt), float((tau ** 2).sum() / Nt))
            logs[r] = lg
        return logs

    def _task_id(self):
        return getattr(self, "_task", (0, (C.c_double * 4)()))[0]

    def _task_params(self):
        return getattr(self, "_task", (0, (C.c_double * 4)()))[1]

    def update(self):
        """One controller step on the current state (= umpcUpdate for every robot); no plant."""
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchUpdate(self.h, _ptr(self.state), _ptr(self.ctrl), _ptr(self.ref),
                                               _ptr(self.actualT0), _ptr(self.Ib), _ptr(self.out), _ptr(self.status),
                                               _ptr(self.info), self._stream()))

    def plant(self, u, nsub=1):
        u = torch.as_tensor(u, dtype=self.dtype, device=self.device).contiguous()
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchPlant(self.h, int(nsub), _ptr(self.state), _ptr(u), _ptr(self.Ib),
                                              _ptr(self.gain), self._stream()))

    def assemble(self):
        """Raw QP data (l, u, q, Px, Ax) for the current state; parity/debug."""
        z = lambda r: torch.empty((r, self.B), dtype=self.dtype, device=self.device)
        l, u, q, Px, Ax = z(39), z(39), z(45), z(45), z(48)
        with torch.cuda.device(self.device):
            self._check(self.L.umpcBatchAssemble(self.h, _ptr(self.state), _ptr(self.ctrl), _ptr(self.ref),
                                                 _ptr(self.Ib), _ptr(l), _ptr(u), _ptr(q), _ptr(Px), _ptr(Ax),
                                                 self._stream()))
        return l, u, q, Px, Ax

    def metrics(self, nsteps):
        """logMetric pair per robot (template/uprightmpc2.py:161-175): mean |p|^2, mean |tau|^2
        over the nsteps*nsub plant substeps accumulated so far."""
        n = max(1, int(nsteps) * int(self.prm.nsub))
        return self.stats / n


def save_viewlog(f1, log, timestamp=None):
    """Writes one robot's control_test_log() as the file template/viewlog.py reads (saveLog :24-33, readFile :50-56):
    gzip-pickled dict {'t','q','dq','u','accdes','posdes'} of arrays, one row per >= 0.999 ms like appendLog (:11-22),
    q = (p, quaternion xyzw of Rb), named `<f1>_<YYYYmmddHHMMSS>.zip`. Returns the file name."""
    import gzip
    import pickle
    import time
    from scipy.spatial.transform import Rotation
    t = np.asarray(log["t"], np.float64)
    keep, last = [], -np.inf
    for i, ti in enumerate(t):
        if ti - last >= 0.999:
            keep.append(i)
            last = ti
    keep = np.array(keep, int)
    Rb = np.asarray(log["R"])[keep].reshape(-1, 3, 3).transpose(0, 2, 1)          # stored column-major
    y = np.asarray(log["y"])[keep]
    data = {"t": t[keep], "q": np.hstack((y[:, 0:3], Rotation.from_matrix(Rb).as_quat())), "dq": y[:, 6:12],
            "u": np.asarray(log["u"])[keep], "accdes": np.asarray(log["accdes"])[keep],
            "posdes": np.asarray(log["pdes"])[keep]}
    fname = "%s_%s.zip" % (f1, timestamp or time.strftime("%Y%m%d%H%M%S", time.localtime()))
    with gzip.GzipFile(fname, "wb") as zf:
        pickle.dump(data, zf)
    return fname


MODELS = {"ca6": (0, 18, 6, 30), "ThrustStrokeDev": (1, 12, 4, 12)}  # id, state rows, input rows, vf output rows


def model_vector_field(model, y, u):
    """ydot of the reference's ca6 / ThrustStrokeDev models (template/ca6dynamics.py:35-50,
    template/FlappingModels3D.py:19-38) for a batch: y [ny,B], u [nu,B] CUDA tensors. ca6 also returns the
    wrench and the bias h: rows [ydot 18 | w 6 | h 6]."""
    mid, ny, nu, nout = MODELS[model]
    L = _lib.lib()
    B = y.shape[1]
    assert y.shape == (ny, B) and u.shape == (nu, B) and y.is_cuda and y.dtype == u.dtype
    y, u = y.contiguous(), u.contiguous()
    aux = torch.empty((nout, B), dtype=y.dtype, device=y.device)
    with torch.cuda.device(y.device):
        rc = L.umpcBatchModel(mid, B, _DT[y.dtype], 0, 0.0, _ptr(y), _ptr(u), _ptr(aux),
                              C.c_void_p(torch.cuda.current_stream(y.device).cuda_stream))
    if rc:
        raise RuntimeError(L.umpcLastError().decode())
    return aux


def model_rk4(model, y, u, dt, nsub=1):
    """Advance y in place by nsub RK4 steps of dt under constant u (build-defined integrator)."""
    mid, ny, nu, _ = MODELS[model]
    L = _lib.lib()
    B = y.shape[1]
    assert y.shape == (ny, B) and u.shape == (nu, B) and y.is_cuda and y.is_contiguous() and nsub >= 1
    u = u.contiguous()
    with torch.cuda.device(y.device):
        rc = L.umpcBatchModel(mid, B, _DT[y.dtype], int(nsub), float(dt), _ptr(y), _ptr(u), None,
                              C.c_void_p(torch.cuda.current_stream(y.device).cuda_stream))
    if rc:
        raise RuntimeError(L.umpcLastError().decode())
    return y


class BatchWLCon:
    """B wrench-linearisation controllers (the step that consumes accdes, SURVEY 8f-1;
    template/uprightmpc2/funapprox.c:118-165), one lane each. `u` [4,B] is the input state."""

    def __init__(self, B, u0, umin, umax, dumax, Qw, controlRate, popts, dtype=torch.float32, device="cuda"):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchWLCon needs a HIP device; there is no CPU path")
        self.L = _lib.lib()
        self.B, self.dtype, self.device = int(B), dtype, torch.device(device)
        self.wl = _lib.WLCon_t()
        f = lambda a, n: np.ascontiguousarray(np.asarray(a, np.float32).reshape(n))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        self.L.wlConInit(C.byref(self.wl), fp(f(u0, 4)), fp(f(umin, 4)), fp(f(umax, 4)), fp(f(dumax, 4)),
                         fp(f(Qw, 6)), C.c_float(controlRate), fp(f(popts, 90)))
        self.u = torch.as_tensor(np.asarray(u0, np.float64)).to(dtype).to(self.device)[:, None].repeat(1, self.B).contiguous()
        self.w0 = torch.zeros((6, self.B), dtype=dtype, device=self.device)

    def update(self, h0, pdotdes):
        h0 = torch.as_tensor(h0, dtype=self.dtype, device=self.device).contiguous()
        pd = torch.as_tensor(pdotdes, dtype=self.dtype, device=self.device).contiguous()
        assert h0.shape == (6, self.B) and pd.shape == (6, self.B)
        with torch.cuda.device(self.device):
            rc = self.L.umpcBatchWLUpdate(C.byref(self.wl), self.B, _DT[self.dtype], _ptr(self.u), _ptr(h0), _ptr(pd),
                                          _ptr(self.w0), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc:
            raise RuntimeError(self.L.umpcLastError().decode())
        return self.u, self.w0
