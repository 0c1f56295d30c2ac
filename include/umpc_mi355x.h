/*
 * libumpc_mi355x.so -- C ABI of the MI355X-native uprightmpc2 path.
 *
 * Part 1 re-exports the reference's own three entry points with identical
 * signatures and semantics (avikde/robobee3d,
 * template/uprightmpc2/uprightmpc2.h:27-49), so every existing host of the
 * reference (pybind module py/uprightmpc2py.cpp:30-52, Simulink S-function
 * legacy_code_gen.m:6, MCU loop g4bee/app/loop_update.cpp:36,54) links
 * unchanged. Unlike the reference this library does NOT import `matMult`
 * (matmult.h:35) and keeps no global solver workspace: any number of
 * UprightMPC_t controllers may coexist (the reference allows one per process,
 * workspace.c:2620).
 *
 * Part 2 is additive: batched controllers (one GPU lane per robot) that run
 * the same step for B independent robots, optionally fused with the
 * rigid-body plant (template/genqp.py:24-41) into a closed loop
 * (template/uprightmpc2.py:120-154).
 *
 * Plain C types only; device buffers are raw HIP device pointers; `stream` is a
 * hipStream_t passed as void* (NULL = default stream). No call allocates or
 * synchronises except where stated.
 */
#ifndef UMPC_MI355X_H
#define UMPC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Part 1: the reference ABI (template/uprightmpc2/uprightmpc2.h)      */
/* ------------------------------------------------------------------ */
#define UMPC_N 3
#define UMPC_NY 6
#define UMPC_NU 3
#define UMPC_NX (UMPC_N * (2 * UMPC_NY + UMPC_NU))
#define UMPC_NC (2 * UMPC_N * UMPC_NY + UMPC_N)
#define UMPC_nAdata 48

/* Caller-allocated POD, same field layout as uprightmpc2.h:27-43 (1308 B):
 * the reference's pybind `vectors()/matrices()` read l,u,q,Px_data,Ax_data,
 * Ax_idx straight out of it (py/uprightmpc2py.cpp:46-51), so umpcUpdate keeps
 * them filled. The two words of `smin` -- which no reference source reads or
 * writes -- carry an opaque controller id set by umpcInit, so the POD may be
 * copied or moved by its host (the pybind class holds it by value) without
 * losing the warm start kept on the device. `T0` is the thrust accumulator of
 * record, as in the reference: a host edit between calls is honoured. */
typedef struct {
  float dt, g, Tmax;
  float Qyr[6], Qyf[6], Qdyr[6], Qdyf[6], R[3];
  float smin[3], smax[3];
  float e3h[3 * 3];
  float e3hIbi[3 * 3];
  float l[UMPC_NC], u[UMPC_NC], q[UMPC_NX];
  float Px_data[UMPC_NX];
  float Ax_data[UMPC_nAdata];
  int Ax_idx[UMPC_nAdata], nAxT0dt, nAxdt;
  float c0[UMPC_NY];
  float T0;
} UprightMPC_t;

/* uprightmpc2.h:45 / uprightmpc2.c:19-118 */
void umpcInit(UprightMPC_t *up, float dt, float g, float TtoWmax, float ws, float wds,
              float wpr, float wpf, float wvr, float wvf, float wthrust, float wmom,
              const float Ib[/* 3 */], int maxIter);

/* uprightmpc2.h:47 / uprightmpc2.c:209-272. R0 column-major. actualT0 >= 0
 * overrides the internal thrust accumulator. Returns 0 (the reference returns
 * osqp_solve's exit flag, which is 0 on every reachable path). Synchronous. */
int umpcUpdate(UprightMPC_t *up, float uquad[/* 3 */], float accdes[/* 6 */],
               const float p0[/* 3 */], const float R0[/* 9 */], const float dq0[/* 6 */],
               const float pdes[/* 3 */], const float dpdes[/* 3 */],
               const float sdes[/* 3 */], float actualT0);

/* uprightmpc2.h:49 / uprightmpc2.c:275-284: lazily initialised singleton. */
void umpcS(float uquad_y1[/* 3 */], float accdes_y2[/* 6 */], const float p0_u1[/* 3 */],
           const float R0_u2[/* 9 */], const float dq0_u3[/* 6 */], const float pdes_u4[/* 3 */],
           const float dpdes_u5[/* 3 */], const float sdes_u6[/* 3 */], float dt_u7, float g_u8,
           float TtoWmax_u9, float ws_u10, float wds_u11, float wpr_u12, float wpf_u13,
           float wvr_u14, float wvf_u15, float wthrust_u16, float wmom_u17,
           const float Ib_u18[/* 3 */], int maxIter_u19, float actualT0_u20);

/* OSQP status of the most recent umpcUpdate on `up` (the reference leaves it
 * in its global workspace.info->status_val; constants.h:18-30). */
int umpcLastStatus(const UprightMPC_t *up);
/* Releases the device-side state attached to `up` (optional: umpcInit on a POD that already carries a live
 * controller releases the previous one first, so re-initialising in a gain sweep or at a Simulink / MCU restart does
 * not accumulate device memory or streams). */
void umpcRelease(UprightMPC_t *up);
/* Number of drop-in controllers currently holding device state (diagnostics / tests). */
int umpcLiveControllers(void);
/* Opt-in reference compatibility switches of ONE controller (flags OR-ed; returns the previous flags, -1 when `up`
 * carries no live controller). A controller starts with the flags of the environment variable UMPC_COMPAT (decimal)
 * at umpcInit time, 0 when it is unset.
 *   UMPC_COMPAT_BOUNDS_REJECT  reproduce osqp_update_bounds' early return (template/uprightmpc2/osqp.c:801-808) whose
 *     value umpcUpdate drops (uprightmpc2.c:246): when ANY assembled l[i] > u[i] (reachable with TtoWmax < 0) NO bound
 *     of that call is applied and the step solves with the bounds the reference's workspace still holds -- Tmax is fixed
 *     by umpcInit in this library, so every call of such a controller is rejected and those are the generated
 *     workspace's placeholder l = 0, u = 1e30 on all 39 rows (workspace.c:476-557), every row an inequality at
 *     rho = 0.1 -- while q, P and A are the new ones; up->l / up->u still show the assembled
 *     (crossed) pair, as in the reference. Such a call runs on the general-structure solver (Part 5), not on the
 *     specialised stream (its dynamics rows are hard-wired equalities): milliseconds, not 0.1 ms. Without the flag the
 *     crossed pair is applied as assembled. tests/golden/bounds_reject.npz pins both behaviours. */
#define UMPC_COMPAT_BOUNDS_REJECT 1
int umpcSetCompat(UprightMPC_t *up, int flags);

/* ------------------------------------------------------------------ */
/* Part 2: batched controllers                                         */
/* ------------------------------------------------------------------ */
#define UMPC_F32 0
#define UMPC_F64 1

/* rows of the SoA device arrays (every array is [rows][B], robot index fastest) */
#define UMPC_STATE_ROWS 18 /* p(3), R column-major (9), dq = (v_world, omega_body) (6) */
#define UMPC_CTRL_ROWS 127 /* x(45) y(39) z(39) T0(1) Eprev(3): warm start of the solver */
#define UMPC_REF_ROWS 9    /* pdes(3) dpdes(3) sdes(3) */
#define UMPC_OUT_ROWS 9    /* uquad(3) = (specific thrust, 2 moments), accdes(6) */
#define UMPC_STAT_ROWS 2   /* sum |p|^2, sum |tau|^2 over plant substeps (logMetric, uprightmpc2.py:161-175) */

typedef struct {
  /* createMPC / umpcInit arguments (template_controllers.py:260-279) */
  double dt, g, TtoWmax, ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom;
  double Ib[3];
  int maxIter; /* fixed ADMM iteration count (50 in the reference) */
  /* closed loop (template/uprightmpc2.py:87, 148-151) */
  double dtsim;   /* plant substep (0.2) */
  double taulim;  /* moment clip (100) */
  int nsub;       /* plant substeps per MPC step (25); 0 = controller only */
  int plant_mode; /* 0 = reference Euler + expm step, 1 = RK4 on the same vector field */
} umpc_batch_params_t;

typedef struct umpc_batch umpc_batch_t;

/* Fills `prm` with the reference defaults (createMPC + controlTest). */
void umpcBatchDefaultParams(umpc_batch_params_t *prm);

/* Creates a batched controller for B robots of scalar type dtype on the
 * current HIP device. Returns NULL on error (umpcLastError()). The handle owns
 * one scratch workspace of 559 rows x B scalars (hipMalloc here, hipFree in
 * umpcBatchDestroy); every other array is caller-provided. */
umpc_batch_t *umpcBatchCreate(const umpc_batch_params_t *prm, int B, int dtype);
void umpcBatchDestroy(umpc_batch_t *h);

/* Writes the cold-start controller record (x=y=z=0, T0=0, Eprev=1) for B robots. */
int umpcBatchInitCtrl(umpc_batch_t *h, void *ctrl, void *stream);

/* K closed-loop MPC steps for every robot in ONE launch. Each step = QP
 * assembly + 10 Ruiz passes + LDL' + maxIter ADMM iterations + status +
 * extraction (= one umpcUpdate), then nsub plant substeps with the moments
 * clipped. Device pointers, SoA [rows][B]:
 *   state   in/out (not written when nsub == 0)
 *   ctrl    in/out
 *   ref     in
 *   actualT0 in, [B] or NULL (values >= 0 override T0 before the first step)
 *   Ib      in, [3][B] or NULL (per-robot inertia for controller and plant)
 *   gain    in, [B] or NULL (per-robot plant thrust gain, Monte-Carlo mass sweep)
 *   out     out
 *   stats   in/out or NULL (accumulated)
 *   status  out int32 [B] or NULL (OSQP status of the last step)
 *   info    out [2][B] or NULL (pri_res, dua_res of the last step)
 * Asynchronous on `stream`. Returns 0 or a hipError_t. */
int umpcBatchRollout(umpc_batch_t *h, int K, void *state, void *ctrl, const void *ref,
                     const void *actualT0, const void *Ib, const void *gain, void *out,
                     void *stats, int32_t *status, void *info, void *stream);

/* One controller step without plant (= umpcUpdate for B robots): `state` is
 * only read. */
int umpcBatchUpdate(umpc_batch_t *h, const void *state, void *ctrl, const void *ref,
                    const void *actualT0, const void *Ib, void *out, int32_t *status,
                    void *info, void *stream);

/* Plant only: nsub substeps of the rigid-body model under inputs u[3][B]. */
int umpcBatchPlant(umpc_batch_t *h, int nsub, void *state, const void *u, const void *Ib,
                   const void *gain, void *stream);

/* Debug/parity: QP assembly for B robots, raw l[39],u[39],q[45],Px[45],Ax[48] rows. */
int umpcBatchAssemble(umpc_batch_t *h, const void *state, const void *ctrl, const void *ref,
                      const void *Ib, void *l, void *u, void *q, void *Px, void *Ax, void *stream);

/* Reference generators evaluated on device at every MPC fire (template/flight_tasks.py:6-49,
 * called at template/uprightmpc2.py:124-131). task 0 (default): `ref` rows are (pdes, dpdes, sdes).
 * task != 0: `ref` rows 0..2 hold initialPos and the reference is generated at time
 *   t = t_ms + step * nsub * dtsim   (umpcBatchTime() advances with every rollout):
 *   1 helix       params (trajAmp, trajFreq [Hz], dz, useY)
 *   2 straightAcc params (tduration, vdes)
 *   3 flip        params (tstart, tend)
 *   4 perch       params (tend, trotstart, trotend, vdes) */
#define UMPC_TASK_REF 0
#define UMPC_TASK_HELIX 1
#define UMPC_TASK_STRAIGHTACC 2
#define UMPC_TASK_FLIP 3
#define UMPC_TASK_PERCH 4
int umpcBatchSetTask(umpc_batch_t *h, int task, const double params[/* 4 */], double t_ms);
double umpcBatchTime(const umpc_batch_t *h);
/* Per-robot objective weights for gain sweeps (template/uprightmpc2.py:272-303): device table
 * [8][B] = (ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom) in the handle's dtype, or NULL for the
 * batch-constant createMPC weights. The pointer is kept, not copied: the table must stay allocated (and may be
 * rewritten between launches) until it is replaced or the handle destroyed. Every weight must be > 0 (the step
 * recovers the Ruiz scaling from the equilibrated diagonal of P); the table is checked once here (synchronous
 * copy), umpcBatchCreate checks the batch-constant ones. Returns 0, -1 (bad weights) or a hipError_t. */
int umpcBatchSetWeights(umpc_batch_t *h, const void *weights);

/* Reference trajectories: a different reference at every closed-loop step of ONE launch, per robot (waypoints, a
 * recorded flight, a planner's output, a task / parameter sweep over the batch).
 * tab: device [steps][9][B] in the handle's dtype -- slice k = the `ref` rows (pdes, dpdes, sdes) of step k, robot index
 * fastest -- kept by pointer, not copied (like the weights table: it must stay allocated, and may be rewritten between
 * launches, until it is replaced or the handle destroyed); NULL = off. While a table is set the `ref` argument of
 * umpcBatchRollout / umpcBatchUpdate is not read (it may be NULL): step k of a rollout reads slice cursor + k. The cursor
 * starts at `cursor0` and advances by K with every umpcBatchRollout whose nsub > 0 (like umpcBatchTime). A rollout that
 * would read past `steps` is refused (-1, umpcLastError) BEFORE anything is launched. umpcBatchUpdate reads slice `cursor`
 * and does not advance it.
 * A table and a handle task != 0 exclude each other: whichever of umpcBatchSetRefTrajectory / umpcBatchSetTask comes
 * second is refused (-1). umpcBatchReactive and umpcBatchTaskReference are refused (-1) while a table is set: they
 * evaluate the reference per plant substep / at a free time, and a table has one slice per MPC step (substep-granular
 * references are not built); umpcBatchReactiveRollout is the reactive baseline that reads a table, one slice held over
 * the substeps of each step. The WL coupling, per-robot weights, Ib, gain, actualT0, both plant modes and
 * umpcBatchSetStepKernel 0..3 all combine with a table. Memory: 9 x B x steps scalars (fp32, B = 65 536, 500 steps:
 * 1.2 GB) -- long runs are chunked: fill the next table while one runs, then set it with cursor0 = 0. */
int umpcBatchSetRefTrajectory(umpc_batch_t *h, const void *tab, long long steps, long long cursor0);
long long umpcBatchRefCursor(const umpc_batch_t *h);
/* Fills tab [steps][9][B] with the task generators evaluated PER ROBOT at the fire times t_k = t_ms + k * nsub * dtsim
 * (the step kernel's own device function and time expression, in the handle's dtype: a table with batch-constant
 * parameters holds what umpcBatchSetTask would generate). task: int32 [B] device array of UMPC_TASK_* ids, or NULL (= the
 * handle's task); params: [4][B] in the handle's dtype, rows in the order listed at umpcBatchSetTask, or NULL (= the
 * handle's); ref [9][B] as in umpcBatchRollout (rows 0..2 = initialPos for a task != 0; task 0 copies the column).
 * Asynchronous on `stream`. Does not set the table: pass it to umpcBatchSetRefTrajectory. */
int umpcBatchTaskTable(umpc_batch_t *h, long long steps, double t_ms, const int32_t *task, const void *params,
                       const void *ref, void *tab, void *stream);

/* Step history: what EVERY closed-loop step of a rollout launch read and produced, for the whole batch (the output side of
 * a reference trajectory: which robots left the path, when, with what command).
 * Device tables in the handle's dtype, robot index fastest, kept by pointer, not copied (they must stay allocated until
 * replaced or the handle destroyed); any one may be NULL = that record is off, all NULL = history off:
 *   state_hist  [steps+1][18][B]   slice c = the state BEFORE step c, slice c + 1 = the state after it
 *   out_hist    [steps][9][B]      (T0 + u0, u1, u2, accdes[6]) of step c
 *   status_hist [steps][B] int32   OSQP status of step c
 *   info_hist   [steps][2][B]      (pri_res, dua_res) of step c
 * While a history is set, a umpcBatchRollout of K steps at cursor c leaves state slice c = its `state` argument as passed,
 * slices c + 1 .. c + K and slices c .. c + K - 1 of the other tables as above, and its `state`, `out`, `status`, `info`
 * arguments exactly what they are without a history. The kernels' own per-step stores go to the tables (the destination
 * moves on one slice per step: the step kernel issues no store more than without a history); stream-ordered device copies
 * around the launch serve the arguments -- five per launch at the most.
 * One form is an exception: the fp64 kernel with one robot per lane quad (the automatic choice for fp64 at B <= 4 096, or
 * umpcBatchSetStepKernel 3) cannot move its pointers inside its register / scratch budget, so with a history set the
 * library issues its K steps as K single-step launches on moved pointers, each preceded by a device copy of state slice
 * k into slice k + 1 (18 x B scalars per step more, K launches instead of one; the results are the same). Every other
 * form -- fp32 lane / quad / C++, fp64 lane / C++ -- stays one launch with no copy per step.
 * A HIP error in the middle of a rollout with a history leaves both cursors and umpcBatchTime where they were. The cursor starts at `cursor0` and
 * advances by K per rollout, so consecutive rollouts continue one table; a rollout that would pass `steps` is refused
 * (-1, umpcLastError) BEFORE anything is launched or copied. Refused (-1): a handle with nsub = 0 (its rollouts never
 * write the state), steps < 1, cursor0 outside [0, steps]. umpcBatchUpdate, umpcBatchPlant, umpcBatchReactive and the
 * B = 1 drop-in neither record nor move the cursor; umpcBatchReactiveRollout, the reactive baseline in closed-loop steps,
 * records into the same tables (see there).
 * Combines with a reference trajectory, the tasks, per-robot weights, Ib, gain, actualT0, the WL coupling, both plant
 * modes, both dtypes and umpcBatchSetStepKernel 0..3. Memory: (18 (steps + 1) + 9 steps + steps + 2 steps) x B scalars
 * when all four are on -- fp32, B = 65 536, 500 steps: state 2.4 GB, out 1.2 GB -- long runs are chunked: read a full table
 * out, then set it again with cursor0 = 0. */
int umpcBatchSetHistory(umpc_batch_t *h, void *state_hist, void *out_hist, int32_t *status_hist, void *info_hist,
                        long long steps, long long cursor0);
long long umpcBatchHistoryCursor(const umpc_batch_t *h);

/* Velocity impulses: a push per closed-loop step and per robot INSIDE a rollout launch (the disturbance experiment of the
 * reference's harness, controlTest(..., tpert=t): dq[1] += 2 once, template/uprightmpc2.py:130-133; a Monte-Carlo sweep of
 * push time x direction x size is one batch). The input side of the step history, with the conventions of its two
 * neighbours: a device table in the handle's dtype, robot index fastest, kept by pointer, not copied (it must stay
 * allocated until replaced or the handle destroyed); tab == NULL switches impulses off:
 *   tab [steps][6][B]   slice c = (dv_world[3], domega_body[3]), added to rows 12..17 of the state
 *                       AFTER the last plant substep of closed-loop step c and BEFORE that step's state store.
 * So the `state` argument holds the kicked state after the launch, step c + 1's controller reads it, and with a step
 * history state slice c + 1 holds it. This is the reference's placement (there the kick precedes the MPC call of the same
 * loop iteration, which is the end of the previous step here); a push before the first step stays the caller's job, by
 * editing `state`. The addition is ONE IEEE add per component in the handle's dtype: a launch of K steps with a table equals
 * K single-step launches with state[12:18] += tab[c] done in between in that dtype, bit for bit, in every kernel form. An
 * all-zero slice is an add like any other (-0.0 + 0.0 = +0.0): "zero table" equals "no table" by value, not by bit pattern.
 * The cursor starts at `cursor0` and advances by K with every umpcBatchRollout whose nsub > 0, independently of the
 * reference and history cursors; a rollout that would read past `steps` is refused (-1, umpcLastError) BEFORE anything is
 * launched or copied, and cursors and umpcBatchTime stay where they were -- as they do after a HIP error in the middle of
 * a rollout. Refused at set time (-1): a handle with nsub = 0, steps < 1, cursor0 outside [0, steps]. umpcBatchUpdate,
 * umpcBatchPlant and the B = 1 drop-in neither apply a slice nor move the cursor. umpcBatchReactive honours the table (the
 * reference's MPC-vs-reactive comparison under one push): it adds slice cursor + j after substep (j + 1) * nsub - 1 and
 * advances the cursor by nsteps / nsub; with a table set it is refused when nsteps % nsub != 0 or the table would be overrun.
 * umpcBatchReactiveRollout adds slice cursor + k after step k like umpcBatchRollout.
 * The fp32 assembly kernels (lane and quad) and the C++ kernels fp32, fp64 lane and fp64 C++ add the slice in the kernel:
 * one launch, six loads and six adds per robot-step; without a table a step costs a few scalar instructions more. One form
 * is an exception, as for the history: the fp64 kernel with one robot per lane quad (the automatic choice for fp64 at
 * B <= 4 096, or umpcBatchSetStepKernel 3) takes no member more inside its scratch budget, so with impulses set the library
 * issues its K steps as K single-step launches with a small add kernel (dq += slice, one lane per robot) after each; the
 * results are the same.
 * Combines with a reference trajectory, the tasks, per-robot weights, Ib, gain, actualT0, the WL coupling, both plant
 * modes, both dtypes, a step history and umpcBatchSetStepKernel 0..3. Memory: 6 x B x steps scalars -- fp32, B = 65 536,
 * 500 steps: 786 MB -- long runs are chunked: set the next part of the table with cursor0 = 0. */
int umpcBatchSetImpulses(umpc_batch_t *h, const void *tab, long long steps, long long cursor0);
long long umpcBatchImpulseCursor(const umpc_batch_t *h);

/* Scoring: from the tables of a rollout (step history, reference trajectory) to one small score per robot and one row per
 * group of robots, on the device -- the last stage of the reference's gainTuningSims, which ends in one cost and one effort
 * per grid cell (costs[i,j], efforts[i,j] = logMetric(log), template/uprightmpc2.py:272-303). UMPC_STAT_ROWS measures
 * sum |p|^2, the distance from the ORIGIN (the reference's logMetric, uprightmpc2.py:161-175); on a reference trajectory
 * that is the path, not the tracking error, and the tables are too large to be scored with array expressions that
 * materialise temporaries of their size.
 * umpcBatchScore is a pure function of its arguments: it reads none of the handle's cursors and takes only B, the dtype and
 * taulim from the handle. All tables are device arrays in the handle's dtype, robot index fastest, in the layouts of
 * umpcBatchSetHistory and umpcBatchSetRefTrajectory:
 *   state_hist  [..][18][B]        must be given
 *   out_hist    [..][9][B]         or NULL: row 6 is left alone and `out` does not enter the finiteness test
 *   status_hist [..][B] int32      or NULL: row 8 is left alone
 *   ref_tab     [..][9][B]         a reference per step, or
 *   ref         [9][B]             one constant reference; exactly ONE of the two is given
 * The call scores steps c = first .. first + count - 1. after = 0: the state of step c is state slice c, the state the
 * step fired on (when its reference slice was evaluated); after = 1: slice c + 1, the state the step produced -- the
 * reference log's convention (log['y'][ti] after the plant, log['pdes'][ti] before it). The reference slice of step c is
 * ref_first + (c - first), its out / status slice is c, and k = step0 + (c - first) is the caller's absolute step number.
 * The caller keeps every slice inside its table.
 * score [UMPC_SCORE_ROWS][B] is in/out and accumulates over calls (a long chunked run is scored chunk by chunk, in any
 * order); umpcBatchScoreInit writes the identity (rows 9 and 10 = -1, all others 0). Per robot, with
 * e_p = |p - pdes|^2 (state rows 0..2, reference rows 0..2), e_s = |s - sdes|^2 (s = state rows 9..11, reference rows 6..8),
 * tau = out rows 1 and 2 clipped at +-taulim, as the plant saw them:
 *   0  steps scored                 1  sum e_p           2  max e_p        3  e_p of the last scored step of the latest call
 *   4  sum e_s                      5  max e_s           6  sum (tau1^2 + tau2^2)
 *   7  sum |p|^2   (rows 7 / 0 and 6 / 0 are the reference's logMetric pair at step granularity)
 *   8  steps with status != 1 (OSQP solved)
 *   9  first k with e_p > tol_p^2, -1 if none ("left the path")
 *  10  last k with e_p > tol_p^2, -1 if none (settled from k + 1 on)
 *  11  steps skipped
 * A step is skipped when any of the up to 14 values it reads is not finite; it is counted in row 11 and in no other row, so
 * a robot that went to NaN stays visible and does not poison its group. Counts and step numbers are scalars of the dtype:
 * a call whose step0 + count passes 2^24 in fp32 is refused. Row 0 lives on the device and the call does not synchronise, so
 * the library cannot see it: it stays exact as long as step0 counts the steps of the run (row 0 <= step0 + count then, as in
 * every use here); a caller who accumulates with another step0 keeps row 0 + count below 2^24 in fp32 themselves. Rows 0, 2, 3, 5, 8..11 do not depend on how a step range is cut into calls; the sum rows
 * 1, 4, 6, 7 are sums of non-negative terms whose order depends on the cut (relative difference <= (steps + 8) u). Nothing
 * crosses robots: a block of robots scored from column-sliced tables equals the same columns of the undivided batch bit for
 * bit, and so do two runs.
 * One pass: 15 words (60 B in fp32) read per robot-step, each once, 12 words written per robot; no temporaries, no atomics.
 * Refused (-1, umpcLastError) BEFORE any launch: count, first, ref_first or step0 < 0 (a negative step number would collide with
 * the -1 of rows 9 and 10); count > 2^31 - 17; tol_p < 0 or not
 * finite; score or state_hist NULL; both or neither of ref_tab and ref. count == 0 is a successful no-op.
 * Asynchronous on `stream`.
 * umpcBatchScoreGroups: group [B] int32 names each robot's group (a grid cell); ids outside [0, G) are ignored. gstat
 * [G][UMPC_GSCORE_ROWS] is DOUBLE whatever the handle's dtype and is overwritten. It holds raw sums, so the tables of the
 * blocks of a sharded job combine by adding (row 3: by max):
 *   0  robots in the group          1  of these, robots with score row 0 > 0; only they enter rows 2..5
 *   2  sum row 1 / row 0            3  max row 2         4  sum row 6 / row 0     5  sum row 7 / row 0
 *   6  robots with row 9 >= 0       7  sum row 8
 * (rows 2 / 1, 5 / 1 and 4 / 1 are a cell's mean tracking cost, logMetric cost and effort). The result is the same bit for
 * bit from run to run: a fixed reduction order, no floating-point atomics. One workgroup per group scans `group`: G x B id
 * reads. */
#define UMPC_SCORE_ROWS 12
#define UMPC_GSCORE_ROWS 8
int umpcBatchScoreInit(umpc_batch_t *h, void *score, void *stream);
int umpcBatchScore(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist,
                   const void *ref_tab, const void *ref, long long first, long long count, long long ref_first,
                   long long step0, double tol_p, int after, void *score, void *stream);
int umpcBatchScoreGroups(umpc_batch_t *h, const void *score, const int32_t *group, int G, double *gstat, void *stream);

/* Ensemble curves: the statistics of each group of robots at every step -- a quantity over time, the view every figure of
 * the reference's harness draws (y(t) against pdes(t), template/uprightmpc2.py:177-269), for a cell of a sweep: reduced over
 * the cell's draws and NOT over time. It is the transpose of the score's reduction over the same words (60 B per robot-step in
 * fp32), which a score cannot give any more (it has summed over the steps) and array expressions cannot give without
 * [steps][B] temporaries. Both calls are pure functions of their arguments, as umpcBatchScore is: they read no cursor of
 * the handle, take only B, the dtype and taulim from it, are asynchronous on `stream` and allocate nothing.
 * umpcBatchGroupIndex sorts the robots by group, once per sweep: group [B] is the array umpcBatchScoreGroups takes;
 * offset [G + 1] with offset[0] = 0; order [B] is a full permutation of 0 .. B - 1: positions offset[g] .. offset[g + 1] - 1
 * hold the robots of group g in ascending robot index, positions offset[G] .. B - 1 the robots whose id is outside [0, G),
 * ascending too (a stable sort by group with the ignored ids last). Integers only, exact. One wavefront per group scans
 * `group` twice: 2 (G + 1) x B id reads. Refused (-1, umpcLastError): h, group, order or offset NULL, G < 1.
 * umpcBatchEnsemble takes the tables, first, count, ref_first, tol_p and after exactly as umpcBatchScore does (layouts, the
 * meaning of `after`, exactly one of ref_tab / ref). order and offset are trusted as umpcBatchGroupIndex left them: the
 * library does not validate device data. ens [count][G][UMPC_ENS_ROWS] is DOUBLE whatever the dtype and is OVERWRITTEN; row
 * i belongs to step first + i, and every (step, group) row is independent of every other: a chunked run writes its chunks
 * into disjoint slices of one `ens` by moving the pointer. A member is scored at a step when all the up to 14 values it
 * reads there are finite. The per-member terms e_p, e_s, the clipped moments and d = p - pdes are formed in the handle's
 * dtype by the expressions of umpcBatchScore, then widened; everything that crosses robots is fp64. Per (step, group):
 *   0  members scored               1  members skipped (not finite); they enter no other row
 *   2  sum e_p                      3  sum e_p^2 (the square formed in double)
 *   4  max e_p                      5  min e_p, +inf when row 0 is 0
 *   6  sum e_s                      7  max e_s
 *   8  sum (tau1^2 + tau2^2), clipped at +-taulim              9  max of that term
 *  10  members with e_p > tol_p^2 (outside the tube at this step)      11  members with status != 1
 *  12..14  sum d_x, d_y, d_z (signed: the cell's bias)
 *  15  robot index of the member with the largest e_p (ties: the lowest index), -1 when row 0 is 0
 * (2 / 0 is the cell's mean tracking error at the step, 3 / 0 - (2 / 0)^2 its variance, 10 / 0 the share of draws outside the
 * tube: a survival curve after a push.) out_hist NULL: rows 8 and 9 are 0 and `out` does not enter the finiteness test;
 * status_hist NULL: row 11 is 0. An empty group has rows 0 and 1 = 0, row 5 = +inf, row 15 = -1 and 0 elsewhere.
 * Order of summation: lane l of a wavefront folds members l, l + 64, .. of the group's list in order, then a fixed butterfly
 * over the 64 lanes. The order of a (step, group) row is a function of that group's member list alone: it does not depend
 * on G, on the other groups, on how the step range is cut into calls, or on the run -- the same bits every time, no
 * floating-point atomics. The rows hold raw sums, maxima and minima, so the blocks of a sharded job combine (score.py,
 * combine_ensembles).
 * Lay the sweep out with CONTIGUOUS cells (cell = b / 64): the 64 lanes then read one 256-B segment per word. Scattered ids
 * are correct but gather one word per row segment and lane, an order of magnitude slower per load; there is no second path.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; state_hist, order, offset or ens NULL; both or neither of ref_tab
 * and ref; count, first or ref_first < 0; count > 2^31 - 1; tol_p < 0 or not finite; G < 1. count == 0 is a successful
 * no-op. */
#define UMPC_ENS_ROWS 16
int umpcBatchGroupIndex(umpc_batch_t *h, const int32_t *group, int G, int32_t *order, int32_t *offset, void *stream);
int umpcBatchEnsemble(umpc_batch_t *h, const void *state_hist, const void *out_hist, const int32_t *status_hist,
                      const void *ref_tab, const void *ref, long long first, long long count, long long ref_first,
                      double tol_p, int after, const int32_t *order, const int32_t *offset, int G,
                      double *ens, void *stream);

/* Ensemble quantiles: the order statistics of each group of robots -- the median curve with a percentile band of a
 * Monte-Carlo cell, which the rows of umpcBatchEnsemble cannot give (one diverged draw owns the mean and the maximum of its
 * cell at every later step; it moves a median by one rank), and the robust counterpart of umpcBatchScoreGroups' cost table.
 * Both calls are pure functions of their arguments: they read no cursor of the handle, take only B, the dtype and taulim
 * from it, are asynchronous on `stream` and allocate nothing. `probs` is a HOST array of nq doubles, 1 <= nq <=
 * UMPC_QUANT_MAX_PROBS, each in [0, 1]: it is copied into the launch arguments -- no device memory, no synchronisation.
 * The order statistic for probs[j] over the n values of a cell that enter, v[0] <= .. <= v[n - 1]:
 *   v[k],  k = min(n - 1, max(0, (long long)ceil(probs[j] * (double)n) - 1))    (one IEEE double multiply)
 * the inverted-CDF / nearest-rank rule: p = 0 the minimum, p = 1 the maximum, p = 0.5 the lower median; NaN when n = 0. The
 * result is an ELEMENT of the cell, widened exactly, never an interpolation (ask for the two neighbouring ranks): it
 * depends on the member set alone -- not on the algorithm, the grid, G, the other groups, how the step range is cut into
 * calls, or the run. Quantiles do NOT combine across the blocks of a sharded job: keep a cell inside one block (cells of 64
 * in contiguous blocks are).
 * umpcBatchEnsembleQuantiles takes the tables, first, count, ref_first, after, order, offset and G exactly as
 * umpcBatchEnsemble does. term chooses the per-member value, formed in the handle's dtype by the expressions of
 * umpcBatchScore and used as it is: UMPC_TERM_EP e_p = |p - pdes|^2, UMPC_TERM_ES e_s = |s - sdes|^2, UMPC_TERM_TAU
 * tau1^2 + tau2^2 clipped at +-taulim (needs out_hist). A member is scored at a step exactly when umpcBatchEnsemble with the
 * same out_hist scores it: with out_hist given, out rows 1 and 2 enter the finiteness test whatever term is. quant
 * [count][G][2 + nq] is DOUBLE whatever the dtype and is OVERWRITTEN; row i belongs to step first + i and every (step,
 * group) row is independent of every other: a chunked run writes its chunks into disjoint slices of one `quant`.
 *   0  members scored (n)           1  members skipped (not finite)          2 + j  the order statistic for probs[j]
 * Rows 0 and 1 are rows 0 and 1 of umpcBatchEnsemble; p = 0 and p = 1 of UMPC_TERM_EP are its rows 5 and 4 bit for bit where
 * row 0 > 0. A group of up to 64 members (cell = b / 64, contiguous: the fast case, as for umpcBatchEnsemble) is sorted in
 * the registers of one wavefront; a larger group of any size is selected by radix in 8 KB of LDS, a path that is correct
 * and not tuned.
 * umpcBatchScoreQuantiles is the same selection over the robots of each group on a per-robot score [UMPC_SCORE_ROWS][B] in
 * the handle's dtype: the value of robot b is (double)score[num][b] (den = -1) or (double)score[num][b] /
 * (double)score[den][b] (den in 0..11, one IEEE double division: 1 / 0 is the per-robot mean tracking error). A robot enters
 * when its score row 0 > 0 and the value is finite -- the rule of umpcBatchScoreGroups; the group's other members are
 * counted in row 1. Values may be negative (rows 9 and 10 hold -1): the order is the total order of the values. quant
 * [G][2 + nq], rows as above.
 * Refused (-1, umpcLastError) BEFORE any HIP call: h, state_hist, score, order, offset, probs or quant NULL; both or neither
 * of ref_tab and ref; count, first or ref_first < 0; count > 2^31 - 1; G < 1; nq outside 1..8; a probability outside [0, 1]
 * or NaN; term outside 0..2; UMPC_TERM_TAU without out_hist; num outside 0..11, den outside -1..11. count == 0 is a
 * successful no-op. */
#define UMPC_QUANT_MAX_PROBS 8
#define UMPC_TERM_EP 0   /* e_p = |p - pdes|^2 */
#define UMPC_TERM_ES 1   /* e_s = |s - sdes|^2 */
#define UMPC_TERM_TAU 2  /* tau1^2 + tau2^2, clipped at +-taulim; needs out_hist */
int umpcBatchEnsembleQuantiles(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *ref_tab,
                               const void *ref, long long first, long long count, long long ref_first, int after,
                               const int32_t *order, const int32_t *offset, int G, int term, const double *probs,
                               int nq, double *quant, void *stream);
int umpcBatchScoreQuantiles(umpc_batch_t *h, const void *score, int num, int den, const int32_t *order,
                            const int32_t *offset, int G, const double *probs, int nq, double *quant, void *stream);

/* Bootstrap intervals of a per-group cost table: how far to trust a number that is an estimate from the draws of one grid
 * cell. The scored values of each group are resampled with replacement R times on the device, a statistic is taken of
 * every resample, and each group gets its point estimate, the mean and standard error of the R replicates and their
 * percentile interval. A pure function of its arguments like umpcBatchScoreQuantiles: it reads no cursor of the handle,
 * takes only B and the dtype from it, is asynchronous on `stream` and allocates nothing; probs is a HOST array as there.
 * Value of robot b: x_b = (double)score[num][b] (den = -1) or (double)score[num][b] / (double)score[den][b] (den in 0..11,
 * one IEEE double division), the rule of umpcBatchScoreQuantiles. With `other` (a second score [UMPC_SCORE_ROWS][B] of the
 * same dtype, e.g. the reactive run of the same sweep on the same tables; may be NULL) y_b is formed the same way from it
 * and the value is x_b - y_b in double: a comparison PAIRED by draw. A robot enters when score[0][b] > 0, other[0][b] > 0
 * if other is given, and the value is finite; the group's other members are counted as skipped. The scored values of group
 * g in the order of its member list order[offset[g] .. offset[g + 1]) are v[0 .. nsc).
 * Replicate r (0 <= r < R), slot m (0 <= m < nsc): u = u01(seed, (r << 32) + m, salt 41) -- the counter hash of the
 * library's Monte-Carlo draws: idx + seed * 0x9E3779B97F4A7C15 + salt, two multiply-xorshift rounds, the top 53 bits --,
 * j = min(nsc - 1, floor(u * nsc)) in double; the resample is v[j(r, 0)], .., v[j(r, nsc - 1)]. The draw depends on
 * (seed, r, m, nsc) and on NOTHING else: not on g, G, the grid or the other groups. Groups with equal nsc are therefore
 * resampled with the same indices -- common random numbers: when draw m of every cell carries the same perturbation,
 * reps[g1] - reps[g2] is a paired bootstrap of the difference between two cells.
 * Statistic of a resample: UMPC_BOOT_MEAN its sum in fp64 (in an order that is a function of nsc alone) divided by nsc;
 * UMPC_BOOT_QUANTILE the element at rank min(nsc - 1, max(0, ceil(stat_p * nsc) - 1)) of the resample in the total order of
 * the values (-0 before +0): an element, never an interpolation. stat_p is ignored by UMPC_BOOT_MEAN but must be in [0, 1].
 * boot [G][UMPC_BOOT_ROWS + nq], DOUBLE, overwritten:
 *   0  members scored (nsc)     1  members skipped     2  the statistic of v itself (the point estimate)
 *   3  mean of the R replicates t_r     4  their standard error sqrt(sum (t_r - mean)^2 / (R - 1)), two passes, fixed order
 *   5 + k  the nearest-rank element of the R replicates at probs[k] (rank as above with R for nsc): the percentile interval
 * nsc = 0 gives NaN in columns 2 and up. reps [G][R], DOUBLE, overwritten: every replicate t_r of every group, NaN rows for
 * empty groups -- what a caller differences between groups. work: DOUBLE [B + G], scratch of the call (the compacted
 * values and nsc per group); the caller owns it, and two calls in flight need two. Bit-reproducible: no atomics, every order
 * of summation fixed. A group of up to 64 scored values is resampled in the registers of one wavefront; a larger one of any
 * size through L2 by a block, a path that is correct and not tuned. Like quantiles, the rows of the blocks of a sharded
 * job do NOT combine: keep a cell inside one block.
 * Refused (-1, umpcLastError) BEFORE any HIP call: score, order, offset, probs, boot, reps or work NULL; G < 1; R outside
 * 2..UMPC_BOOT_MAX_REPS; stat neither of the two; stat_p outside [0, 1] or NaN; nq outside 1..8; a probability outside
 * [0, 1] or NaN; num outside 0..11, den outside -1..11; h NULL. */
#define UMPC_BOOT_MEAN 0
#define UMPC_BOOT_QUANTILE 1
#define UMPC_BOOT_ROWS 5   /* columns ahead of the percentile columns */
#define UMPC_BOOT_MAX_REPS 1048576
int umpcBatchScoreBootstrap(umpc_batch_t *h, const void *score, const void *other, int num, int den,
                            const int32_t *order, const int32_t *offset, int G, int stat, double stat_p,
                            int R, unsigned long long seed, const double *probs, int nq,
                            double *boot, double *reps, double *work, void *stream);

/* Bootstrap confidence bands of ensemble curves: the error bar of the per-step curve of a group (the mean or a quantile of a
 * term over the draws of a grid cell, or of MPC minus reactive), pointwise and SIMULTANEOUS over the window. A pure function
 * of its arguments like umpcBatchEnsembleQuantiles, whose tables, window (first, count, ref_first, after), reference
 * (exactly one of ref_tab, ref), group index and term it takes: it reads no cursor of the handle, takes only B, the dtype
 * and taulim from it, is asynchronous on `stream` and allocates nothing; probs and levels are HOST arrays.
 * Step i of the window, group g: v_i[0 .. nsc_i) is the term of the members scored at that step -- the rule of
 * umpcBatchEnsembleQuantiles with the same out_hist -- in member-list order, as a double. With other_state (a second
 * history of the same shape and dtype, e.g. the reactive run of the same sweep; other_out given exactly when out_hist is)
 * a member enters when BOTH histories score it against the SAME reference and x - x_other, subtracted in double, is finite:
 * that difference is the value, a comparison paired by draw. Replicate r of the step is the statistic (stat, stat_p: those
 * of umpcBatchScoreBootstrap) of v_i resampled with the indices of that call for (seed, r, slot, nsc_i): they do not depend
 * on the step, so while nsc does not change replicate r draws the same members at every step -- it resamples whole
 * trajectories. When a draw drops out mid-window its later steps are resampled with the indices of the new count.
 * band [count][G][UMPC_BAND_ROWS + nq], DOUBLE, overwritten:
 *   0  members scored (nsc)     1  members skipped     2  the statistic of v_i itself (the point estimate)
 *   3  mean of the R replicates     4  their standard error, two passes, R - 1 in the divisor
 *   5  1.0 when the step ENTERS the simultaneous statistic -- nsc >= 2 and the R replicates are not all the same double
 *      (a test on the replicates, not on se > 0) --, else 0.0
 *   6 + k  the nearest-rank element of the R replicates at probs[k]: the pointwise percentile band
 * nsc = 0 gives NaN from column 2 on and 0 in column 5.
 * sup [G][R], DOUBLE: sup[g][r] = the largest |t_{i,r} - point_i| / se_i over the entering steps i (a comparison that a NaN
 * never wins), a NaN row when no step enters. crit [G][1 + nl], DOUBLE: column 0 = the number of entering steps, column
 * 1 + j = the nearest-rank element of sup[g] at levels[j], NaN when no step enters. The simultaneous band of group g at
 * level j is point_i +- crit[g][1 + j] * se_i over its entering steps: it contains the whole curve with about that
 * probability, which a pointwise band does not. crit == NULL && sup == NULL (with nl == 0) asks for band alone.
 * work: DOUBLE [B + G], scratch of the call (the compacted values of groups above 64 members); the caller owns it, and two
 * calls in flight need two. One launch, one pass over the tables; the replicates are never stored (nothing of size R * B
 * or count * G * R exists). Bit-reproducible: no atomics, every order of summation fixed and that of
 * umpcBatchScoreBootstrap: a step equals umpcBatchScore(count = 1) + umpcBatchScoreBootstrap on it bit for bit. A group of
 * up to 64 scored values is resampled in the registers of a wavefront; a larger one through L2, correct and not tuned.
 * Rows of the blocks of a sharded job do NOT combine: keep a cell inside one block.
 * Refused (-1, umpcLastError) BEFORE any HIP call: state_hist, order, offset, probs, band or work NULL; one of crit and sup
 * without the other; both or neither of ref_tab and ref; count, first or ref_first < 0; count > 2^31 - 1; G < 1; R outside
 * 2..UMPC_BAND_MAX_REPS; stat neither of the two; stat_p outside [0, 1] or NaN; nq outside 1..8 or a probability outside
 * [0, 1] or NaN; with crit, nl outside 1..8 or a level outside [0, 1] or NaN or levels NULL; without crit, nl != 0; term
 * outside 0..2; UMPC_TERM_TAU without out_hist; other_out without other_state, or other_state with other_out given and
 * out_hist not (or the reverse); h NULL. count == 0 is a successful no-op. */
#define UMPC_BAND_ROWS 6   /* columns ahead of the percentile columns */
#define UMPC_BAND_MAX_REPS 4096
int umpcBatchEnsembleBootstrap(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *other_state,
                               const void *other_out, const void *ref_tab, const void *ref, long long first,
                               long long count, long long ref_first, int after, const int32_t *order,
                               const int32_t *offset, int G, int term, int stat, double stat_p, int R,
                               unsigned long long seed, const double *probs, int nq, const double *levels, int nl,
                               double *band, double *crit, double *sup, double *work, void *stream);

/* Frequency response: how fast a reference the controller still follows. Scores, ensembles and their bootstraps measure how
 * LARGE the tracking error is; this block gives the Bode point of every robot of a (trajFreq x draws) sweep -- gain and
 * phase of p against pdes at the robot's own task frequency, the amplitude of the tracking error there, and how much of
 * the motion is not at that frequency at all -- by a three-parameter least-squares sine fit (IEEE 1057 style)
 *   y_k ~ a0 + a1 cos(phi_k) + a2 sin(phi_k),   phi_k = 2 pi k nu[b]
 * per robot and per position axis j = 0..2, of y = p_j (state row j) and of r = pdes_j (reference row j). A least-squares
 * fit and not a DFT bin: it is exact for a window that is not a whole number of periods, and indifferent to the constant
 * offset (initialPos, the 1 - cos of useY). Two stages, as a score holds raw sums before means: umpcBatchResponse adds the
 * sums of the normal equations in one pass over the step history, once per chunk of a chunked run; umpcBatchResponseFit
 * solves them once. Array expressions over the history would need [steps][B] sine and cosine tables.
 * umpcBatchResponse is a pure function of its arguments, as umpcBatchScore is: it reads none of the handle's cursors and
 * takes only B and the dtype from the handle. state_hist, ref_tab / ref (exactly ONE of the two), first, count, ref_first
 * and after are those of umpcBatchScore; there is no out or status record. nu [B] DOUBLE on the device: the robot's
 * frequency in revolutions per closed-loop step (f [Hz] x 1e-3 x nsub x dtsim). Step i of the call (c = first + i) carries
 * k = step0 + i. Its phase is u = k nu - floor(k nu) with ONE IEEE double multiply of (double)k and nu, and c = cos(2 pi u),
 * s = sin(2 pi u) in fp64 to a few ulp (sincospi(2 u): exactly 0 and +-1 at the quarter points): the phase of a step does
 * not depend on how the run is cut into calls, and stays accurate at a step0 of 10^6.
 * A step reads 6 words per robot: state rows 0..2 of slice c + after, reference rows 0..2 of table slice ref_first + i or of
 * the constant ref. A step where any of the six, or the phase (a nu that is not finite), is not finite is counted in
 * `skipped` and adds nothing else. The words are widened exactly; every product and every sum is fp64.
 * sums [UMPC_RSUM_ROWS][B] DOUBLE, in/out: the call ADDS into it; umpcBatchResponseInit writes zeros. Per robot:
 *   0  n, steps that entered        1  skipped steps
 *   2  sum c      3  sum s      4  sum c c      5  sum c s          (sum s s = n - sum c c)
 *   6 + 9 j + 0..8, axis j:  sum y,  sum y c,  sum y s,  sum y y,  sum r,  sum r c,  sum r s,  sum r r,  sum y r
 * Order of summation: a block of 64 robots is 4 wavefronts; wavefront w folds steps w, w + 4, w + 8, .. of the call in
 * order, the four partial sums are added in the order 0, 1, 2, 3 and the total is added to `sums`. Nothing crosses robots:
 * bit-equal from run to run, and between a column block on a handle of its own and the same columns of the whole batch; no
 * atomics, no temporaries. Rows 0 and 1 do not depend on how a step range is cut into calls; the other rows to rounding
 * (each within (n + 16) u times the sum of its terms' magnitudes of the exact sum).
 * umpcBatchResponseFit: one lane per robot, fp64 throughout, rounded to the handle's dtype at the store. Normal matrix
 * M = [[n, sum c, sum s], [sum c, sum cc, sum cs], [sum s, sum cs, sum ss]], Cholesky in that variable order with the
 * pivots d1 = n, d2, d3 (the squares of the factor's diagonal). The fit is REFUSED when n < 3 or a pivot is <= 1e-9 n (or
 * NaN): nu = 0 and nu = 0.5, where s = 0 at every step, and windows of fewer than three steps. With Y = a1 - i a2 of y
 * and R likewise of r, resp [3][UMPC_RESP_ROWS][B] in the handle's dtype, overwritten; per axis:
 *   0  n, or 0 when the fit is refused (rows 2..11 are then NaN)        1  skipped steps
 *   2  |Y|^2                        3  |R|^2
 *   4  gain sqrt(row 2 / row 3), NaN when row 3 is 0
 *   5  phase arg Y - arg R in (-pi, pi], negative = p lags pdes; NaN when row 3 is 0
 *   6  Re (Y / R)                   7  Im (Y / R); both NaN when row 3 is 0
 *   8  a0 of y                      9  a0 of r
 *  10  mean squared residual of y's fit, max(0, (sum y y - a . rhs) / n): distortion and everything off the fundamental
 *  11  |Y - R|^2, the squared amplitude of the tracking error at the fundamental; sqrt(row 11 / row 3) is |S|
 * A constant reference has |R|^2 = 0 only to rounding unless it is zero: rows 4..7 then mean nothing; rows 2, 8, 10 stand.
 * resp[axis] is shaped as a score on purpose -- [12][B], contiguous, row 0 > 0 meaning "enters" -- so
 * umpcBatchScoreQuantiles(resp[0], num = 2, den = 3) is a cell's median gain^2 and umpcBatchScoreBootstrap(.., other = the
 * reactive run's resp[0]) its interval and MPC minus reactive paired by draw, unchanged. Rows 0 and 1 are exact in fp32 up
 * to 2^24 steps.
 * Not built: more than one frequency per call (a harmonic is a second call with 2 nu); the attitude and effort signals;
 * a per-cell reduction of the complex H beyond what the quantile and bootstrap calls give.
 * Refused (-1, umpcLastError) BEFORE any HIP call: h NULL; state_hist, nu, sums or resp NULL; both or neither of ref_tab and
 * ref; count, first, ref_first or step0 < 0; count > 2^31 - 9; step0 + count > 2^53. count == 0 is a successful no-op.
 * Asynchronous on `stream`. */
#define UMPC_RSUM_ROWS 33
#define UMPC_RESP_ROWS 12
int umpcBatchResponseInit(umpc_batch_t *h, double *sums, void *stream);
int umpcBatchResponse(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref, const double *nu,
                      long long first, long long count, long long ref_first, long long step0, int after, double *sums,
                      void *stream);
int umpcBatchResponseFit(umpc_batch_t *h, const double *sums, void *resp, void *stream);

/* Dispersion ellipsoids: the mean vector, the covariance and the k-sigma ellipsoid of the error state of each group of
 * robots at every step -- the standard product of a Monte-Carlo dispersion study -- and the Mahalanobis distance of every
 * robot from its own cell's ellipsoid. Every other table here works on a scalar norm (e_p, e_s, the clipped moments); the
 * direction of the error and the correlation between axes are kept only here. Array expressions would need a
 * [steps][B][21] temporary. All four calls are pure functions of their arguments, as umpcBatchScore is: they read no
 * cursor of the handle, take only B and the dtype from it, are asynchronous on `stream` and allocate nothing.
 * Error state of robot b at a step: z = (p - pdes, v - dpdes) in R^6; p = state rows 0..2, v = state rows 12..14 (world
 * frame), pdes = reference rows 0..2, dpdes = reference rows 3..5: 12 words (48 B in fp32) per robot-step, each read once.
 * Each difference is formed in the handle's dtype with one rounding, then widened to double.
 * umpcBatchDispersion takes state_hist, ref_tab / ref (exactly ONE of the two), first, count, ref_first, after, order, offset
 * and G exactly as umpcBatchEnsemble does; there is no out or status record and no tube. A member is scored at a step when
 * all 12 words it reads there are finite, and skipped otherwise. THIS IS NOT umpcBatchEnsemble's RULE: that call reads s, out
 * and the status and not v, this one reads v and dpdes and none of them. mom [count][G][UMPC_DISP_ROWS] is DOUBLE whatever
 * the dtype and is OVERWRITTEN; row i belongs to step first + i. Per (step, group):
 *   0  members scored               1  members skipped (not finite); they enter no other row
 *   2..7   S1 = sum z
 *   8..28  S2 = sum z_i z_j for i <= j, the upper triangle row by row: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
 *  29..31  0, reserved
 * The products are formed in double: exact for an fp32 handle, one rounding for an fp64 one (no contraction).
 * Order of summation: lane l of a wavefront starts at +0 and adds the terms of members l, l + 64, .. of the group's list in
 * that order; then for w = 32, 16, 8, 4, 2, 1 every lane l replaces its value by (value of l) + (value of l ^ w) (the kernel
 * evaluates this tree of pairwise sums only in the lanes that store: 32 doubles cross lanes per row, not 27 x 6). The order
 * of a (step, group) row is a function of that group's member list alone: it does not depend on G, on the other groups, on
 * how the step range is cut into calls, or on the run -- the same bits every time, no floating-point atomics. Each entry
 * is within (n + 8) 2^-53 sum |term| of the exact sum of its terms for an fp32 handle ((n + 9) for fp64, whose products
 * round). RAW MOMENTS ADD: the rows 0..28 of the blocks of a sharded job, or of a cell split over column blocks, sum to the
 * undivided rows (score.py, combine_dispersions) -- which the order statistics do not.
 * umpcBatchDispersionEllipsoids: one row of ell [count][G][UMPC_ELL_ROWS] DOUBLE per row of mom, fp64 throughout:
 *   0, 1   n scored, skipped        2..7  mean m = S1 / n (NaN when n = 0)
 *   8..28  covariance C = (S2 - S1 S1^T / n) / (n - 1), upper triangle in the order of mom
 *  29..31  eigenvalues of the 3 x 3 position block C_pp, descending
 *  32..40  V [3][3] row by row: COLUMN c is the eigenvector of eigenvalue c; its component of largest magnitude is positive
 *          (ties: the lowest index). Cyclic Jacobi, pairs (0,1), (0,2), (1,2), 8 sweeps whatever the data.
 *  41      status. 0: usable. 1: n < 2 -- rows 8..47 are NaN except this one. 2: C_pp is not positive definite: a pivot
 *          of its Cholesky factorisation is <= 1e-12 trace(C_pp) (or NaN) -- rows 42..47 are NaN, the rest is filled.
 *          A cell whose draws all start on one point has status 2 at its first steps: a normal case, not an error.
 *  42..47  Linv, the inverse of the lower Cholesky factor of C_pp, its lower triangle row by row: (0,0) (1,0) (1,1) (2,0)
 *          (2,1) (2,2). d2 = |Linv (d - m_p)|^2 is the squared Mahalanobis distance of a position error d.
 * The covariance is formed from raw moments: its entries carry the summation error above amplified by about
 * (|m|^2 + sigma^2) / sigma^2. Derived, not measured: fine while |m| / sigma stays below about 1e4 for an fp32 handle's
 * tables and 1e3 for an fp64 handle's.
 * umpcBatchMahalanobis: a per-robot score msc [UMPC_MAHA_ROWS][B] in the handle's dtype, in/out, over the steps of the call.
 * ell covers exactly the steps first .. first + count - 1 of THIS call (row i = step first + i); group [B] is the array
 * umpcBatchGroupIndex took. Per step a robot reads p and pdes (6 words) and the row of its own cell: d = p - pdes in the
 * dtype, widened; d2 in fp64; rounded once to the dtype. The step is skipped when a word is not finite, the id is outside
 * [0, G), or the row's status is not 0. Step i of the call carries the number k = step0 + i.
 *   0  steps scored                 1  sum d2
 *   2  max d2                       3  step of the maximum (the first on a tie), -1 when row 0 is 0
 *   4  steps with d2 > limit        5, 6  first / last step over the limit, -1 if none
 *   7  last d2                      8  steps skipped               9..11  0, reserved
 * (`limit` is compared after rounding to the dtype.) Row 0 is the score's "enters when row 0 > 0", so
 * umpcBatchScoreQuantiles and umpcBatchScoreBootstrap take this table unchanged (num = 1, den = 0: the mean d2; num = 2:
 * the worst). umpcBatchMahalanobisInit writes the identity (rows 3, 5, 6 = -1, the others 0); a chunked run accumulates as
 * umpcBatchScore does: rows 0, 2..8 do not depend on how a range is cut into calls, row 1 to rounding ((steps + 8) u).
 * The covariance includes the robot itself, so d2 <= (n - 1)^2 / n: a limit above that never fires in a small cell.
 * Not built: a 6 x 6 distance or eigen-decomposition; attitude components in z; leave-one-out distances and calibrated
 * limits; bootstrap bands of covariance entries; a DPP fold; shifted or two-pass accumulation for |m| / sigma beyond the
 * range above; combining across GPUs inside the library.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; a table pointer, order, offset, group, mom, ell or msc NULL; both
 * or neither of ref_tab and ref; count, first, ref_first or step0 < 0; count > 2^31 - 1 (Mahalanobis: 2^31 - 17); G < 1;
 * limit <= 0 or not finite; an fp32 handle with step0 + count > 2^24. count == 0 is a successful no-op. */
#define UMPC_DISP_ROWS 32
#define UMPC_ELL_ROWS 48
#define UMPC_MAHA_ROWS 12
int umpcBatchDispersion(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref,
                        long long first, long long count, long long ref_first, int after,
                        const int32_t *order, const int32_t *offset, int G, double *mom, void *stream);
int umpcBatchDispersionEllipsoids(umpc_batch_t *h, const double *mom, long long count, int G, double *ell, void *stream);
int umpcBatchMahalanobisInit(umpc_batch_t *h, void *msc, void *stream);
int umpcBatchMahalanobis(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref,
                         const double *ell, const int32_t *group, int G, long long first, long long count,
                         long long ref_first, long long step0, int after, double limit, void *msc, void *stream);

/* Error propagators: what relates the cloud of a group at step k to its cloud at step k + L. Every table above looks at one
 * step at a time; these two calls give the cross moments of the error state z = (p - pdes, v - dpdes) between two steps and
 * the affine map z_b ~ Phi z_a + c they determine -- the closed-loop dynamics of a gain cell as its Monte-Carlo draws show
 * them: poles and decay rate (eigenvalues of Phi, on the host: robobee3d_amd/score.py propagator_poles), how much of the
 * spread at k + L the linear model leaves unexplained (Q, r2), and growth, the mean squared amplification in the cloud's
 * own metric.
 *
 * umpcBatchLagMoments takes the tables, the window and the group index of umpcBatchDispersion and a lag L >= 1. Row i of
 * xmom [count][G][UMPC_XMOM_ROWS] DOUBLE pairs slice a (state first + after + i, reference ref_first + i) with slice b
 * (state first + after + i + L, reference ref_first + i + L; a constant `ref` serves both): THE TABLES MUST HOLD
 * count + L SLICES from the first one. A member is scored when all 24 words -- p, v, pdes, dpdes at a and at b, the rows
 * umpcBatchDispersion reads -- are finite; differences in the handle's dtype with one rounding, every product and sum fp64.
 *   row  0        n, the members scored
 *        1        members skipped (some word at a or at b is not finite)
 *        2..7     S1a = sum z_a          8..13   S1b = sum z_b
 *        14..34   S2a = sum z_a,i z_a,j, i <= j, upper triangle row by row (the order of umpcBatchDispersion's S2)
 *        35..55   S2b likewise
 *        56..91   Sba[i][j] = sum z_b,i z_a,j, row-major 6 x 6
 *        92..95   +0
 * The order of summation of a row is umpcBatchDispersion's (lane partials in member order, then the butterfly w = 32 .. 1):
 * a function of the group's member list and L alone, bit-reproducible; on tables where no member is skipped rows 2..7 and
 * 14..34 are the bits of umpcBatchDispersion's row of step k, rows 8..13 and 35..55 those of step k + L. Raw moments add
 * across the blocks of a sharded job (score.py combine_lag_moments). No atomics, no temporaries.
 *
 * umpcBatchPropagators: one row of prop [count][G][UMPC_PROP_ROWS] DOUBLE per row of xmom, fp64 throughout. With the means
 * m = S1 / n and the covariances C_a, C_b, C_ba formed from the raw moments as umpcBatchDispersionEllipsoids forms C,
 * C_a = L_a L_a^T (Cholesky): Phi = C_ba C_a^-1, c = m_b - Phi m_a, Q = C_b - Phi C_ba^T.
 *   row  0, 1     n, skipped (copied)
 *        2        status: 0 usable; 1 n < 8 (one more member than the seven coefficients of a row of the fit); 2 a pivot of
 *                 the Cholesky factorisation of C_a is <= 1e-10 x C_a[j][j] or NaN (the cloud at a is flat in a direction)
 *        3, 4     r2_p = 1 - (Q00 + Q11 + Q22) / (Cb00 + Cb11 + Cb22), r2_v likewise on the velocity block; NaN where
 *                 the denominator is 0
 *        5        growth = |L_a^-1 Phi L_a|_F^2 / 6; below 1: the cloud contracts on average over L steps
 *        6, 7     0
 *        8..43    Phi, row-major 6 x 6
 *        44..49   c
 *        50..70   Q, upper triangle row by row
 *        71..79   0
 * With status != 0 rows 3..5 and 8..70 are NaN. No eigen-solver on the device: the poles are host work.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; a table pointer, order, offset, xmom or prop NULL; both or neither
 * of ref_tab and ref; count, first or ref_first < 0; count > 2^31 - 1; G < 1; lag < 1 or lag > 2^20. count == 0 is a
 * successful no-op. */
#define UMPC_XMOM_ROWS 96
#define UMPC_PROP_ROWS 80
int umpcBatchLagMoments(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref,
                        long long first, long long count, long long ref_first, int after, int lag,
                        const int32_t *order, const int32_t *offset, int G, double *xmom, void *stream);
int umpcBatchPropagators(umpc_batch_t *h, const double *xmom, long long count, int G, double *prop, void *stream);

/* Sensitivity indices: which of the inputs DRAWN for a sweep explains the error of a cell. The user drew per-robot inputs --
 * initial offset and tilt per axis, push size, direction and time, a task parameter, a weight --; the first-order index
 * (correlation ratio) of input j is eta2_j = Var(E[y | x_j]) / Var(y), the share of a cell's error variance that goes away
 * when x_j is known. The estimator is the given-data, binned one: the range of a factor is cut into M bins of equal count
 * inside the cell, by rank, and eta2 = SSB / SST, the between-bin sum of squares over the total. The error terms are even
 * functions of a signed offset, so the linear fit of umpcBatchPropagators finds a coefficient of 0 where eta2 is 1. All four
 * calls are pure functions of their arguments, asynchronous on `stream`, and allocate nothing; from the handle they take B and
 * the dtype (umpcBatchSensitivity also taulim). 1 <= F <= UMPC_SENS_MAX_FACTORS, 2 <= M <= UMPC_SENS_MAX_BINS.
 *
 * umpcBatchFactorBins, once per sweep: factors [F][B] in the handle's dtype, order / offset / G a group index
 * (umpcBatchGroupIndex), bins [F][B] int32 OVERWRITTEN. For every group and factor the members with a finite value are
 * ranked by value with <, ties broken by position in the member list (-0 and +0 are equal): numpy.argsort(kind="stable").
 * bin = (rank * M) / n_f in integers, n_f the members of the group with a finite value. A value that is not finite gets -1,
 * and so does every robot outside every group. Integers only and exact. n^2 comparisons per (group, factor): meant for
 * cells of tens to thousands. `bins` may as well be written by hand: a categorical factor is its own bin.
 *
 * umpcBatchSensitivity: the tables, the window, the reference (exactly ONE of ref_tab / ref), the group index and `term` are
 * exactly those of umpcBatchEnsembleQuantiles. The value y of a member is formed in the handle's dtype by the expressions of
 * umpcBatchScore and widened; y^2 and every sum are fp64. A member is scored at a step when umpcBatchEnsembleQuantiles with
 * the same out_hist scores it AND all F of its bins lie in [0, M); it is skipped otherwise. sens [count][G][4 + 2 F M] is
 * DOUBLE and OVERWRITTEN; row i belongs to step first + i and rows are independent (chunked runs write disjoint slices):
 *   0  n scored          1  skipped          2  S1 = sum y          3  S2 = sum y^2
 *   4 + f M + m          N_fm, the scored members of bin m of factor f (sum_m N_fm = n for every f)
 *   4 + F M + f M + m    S_fm = sum y over them
 * Order of summation: umpcBatchDispersion's -- lane l of a wavefront starts at +0 and adds the terms of members l, l + 64, ..
 * in list order (+0 for a member that is not scored or not in the bin), then for w = 32, 16, 8, 4, 2, 1 every lane l replaces
 * its value by (value of l) + (value of l ^ w). A row is a function of the member list and the bins alone: the same bits
 * every time, no atomics, no temporaries (score.py, sensitivity_reference, follows it operation by operation). Rows 0 and 1
 * with valid bins are rows 0 and 1 of umpcBatchEnsemble. RAW SUMS ADD across the blocks of a sharded job when the bins were
 * assigned on the whole job (score.py, combine_sensitivities).
 *
 * umpcBatchSensitivityIndices: one row of idx [count][G][8 + F (4 + M)] DOUBLE per row of sens, fp64 throughout:
 *   0  n      1  skipped      2  status      3  mean = S1 / n      4  variance = SST / (n - 1)
 *   5  SST = S2 - S1 S1 / n   6, 7  0
 *   per factor f at 8 + f (4 + M):
 *     +0  eta2 = SSB / SST, SSB = sum over the non-empty bins, m ascending, of S_fm S_fm / N_fm, minus S1 S1 / n
 *     +1  eps2 = 1 - (1 - eta2)(n - 1) / (n - M_f), the bias-adjusted index (with no effect E eta2 ~ (M_f - 1) / (n - 1))
 *     +2  F = (SSB / (M_f - 1)) / ((SST - SSB) / (n - M_f))
 *     +3  M_f, the non-empty bins
 *     +4 .. +3 + M  the bin means S_fm / N_fm, the main-effect curve E[y | bin]; NaN for an empty bin
 * status 1: n < 2 M. status 2: !(SST > 0), or S1 or S2 is not finite. With either, +0 .. +2 of every factor are NaN (the
 * other rows are filled as the formulas give them). A factor with M_f < 2 or n <= M_f has NaN in +0 .. +2. Nothing is
 * clamped: rounding may put eta2 a hair outside [0, 1]. SST comes from raw moments: eta2 carries the summation error
 * amplified by about S2 / SST.
 *
 * umpcBatchScoreSensitivity: the same sums over one column of a per-robot score [UMPC_SCORE_ROWS][B] in the handle's dtype,
 * sens [G][4 + 2 F M]. The value of robot b is that of umpcBatchScoreQuantiles (score[num][b], or score[num][b] /
 * score[den][b] in double; den = -1: no division); it enters when row 0 > 0, the value is finite and all F bins lie in
 * [0, M). umpcBatchSensitivityIndices takes the result with count = 1.
 * Not built: total-effect or interaction indices (two-factor bins); a permutation null on the device; p-values.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; a table pointer, factors, order, offset, bins, sens or idx NULL; both
 * or neither of ref_tab and ref; count, first or ref_first < 0; count > 2^31 - 1; G < 1; F outside 1..6 or M outside 2..8;
 * term outside 0..2; UMPC_TERM_TAU without out_hist; num outside 0..11, den outside -1..11. count == 0 is a successful
 * no-op. */
#define UMPC_SENS_MAX_FACTORS 6
#define UMPC_SENS_MAX_BINS 8
int umpcBatchFactorBins(umpc_batch_t *h, const void *factors, int F, const int32_t *order, const int32_t *offset, int G,
                        int M, int32_t *bins, void *stream);
int umpcBatchSensitivity(umpc_batch_t *h, const void *state_hist, const void *out_hist, const void *ref_tab,
                         const void *ref, long long first, long long count, long long ref_first, int after,
                         const int32_t *order, const int32_t *offset, int G, int term, const int32_t *bins, int F, int M,
                         double *sens, void *stream);
int umpcBatchSensitivityIndices(umpc_batch_t *h, const double *sens, long long count, int G, int F, int M, double *idx,
                                void *stream);
int umpcBatchScoreSensitivity(umpc_batch_t *h, const void *score, const int32_t *order, const int32_t *offset, int G,
                              int num, int den, const int32_t *bins, int F, int M, double *sens, void *stream);

/* Error spectra: the oscillation nobody asked for. A gain cell whose position error rings at 30 Hz has the sum_ep of a cell
 * with a steady offset, and a cell whose moments chatter at the step rate the sum_tau2 of one that pushes smoothly;
 * umpcBatchResponse fits ONE frequency the caller knows in advance. This block projects a 3-channel signal of every robot
 * onto K windowed cosine / sine pairs over a window of the step history in one pass, turns the raw sums into a periodogram
 * and a chatter score per robot, and sums the periodograms over the draws of each grid cell -- the average over draws is
 * the consistent spectral estimate, and a Monte-Carlo sweep provides it for free. Array expressions would need the signal
 * as an fp64 [steps][3][B] temporary in front of a matrix product. All four calls are pure functions of their arguments,
 * take only B and the dtype from the handle, are asynchronous on `stream` and allocate nothing.
 *
 * Signals, 3 channels each:
 *   UMPC_SPEC_EP  p - pdes: state rows 0..2 minus reference rows 0..2
 *   UMPC_SPEC_ES  s - sdes: state rows 9..11 minus reference rows 6..8
 *   UMPC_SPEC_U   out rows 0..2 as recorded (specific thrust and the two moments, unclipped); state_hist, ref_tab and ref
 *                 are not read and may be NULL, out_hist is required and `after` does not enter
 * A difference is formed in the handle's dtype with one rounding and then widened exactly. state_hist, ref_tab / ref (exactly
 * ONE of the two), first, count, ref_first and after are those of umpcBatchResponse.
 *
 * basis [W][1 + 2 K] DOUBLE on the device, made on the host (robobee3d_amd/score.py spectrum_basis): column 0 is the window
 * weight w_k, columns 1 + 2 j and 2 + 2 j are w_k cos(2 pi u_jk) and w_k sin(2 pi u_jk) of frequency j. Step i of the call
 * reads row basis_first + i: the caller makes sure the table holds basis_first + count rows. There is no sincos on the
 * device: the sums are bit-identical to the numpy mirror, and the call is a projection onto ANY temporal basis -- the
 * spectrum is its first user. Every entry must be finite. 1 <= K <= UMPC_SPEC_MAX_K.
 *
 * sums [2 + 3 (2 + 2 K)][B] DOUBLE, in/out: umpcBatchSpectrum ADDS into it; umpcBatchSpectrumInit writes zeros. A step
 * enters for a robot when every word it reads for the three channels is finite; otherwise row 1 counts it and every other
 * row receives +0. With y the channel's value, w, bc_j, bs_j the step's basis row and t = w y:
 *   0  n, steps that entered        1  skipped steps
 *   2 + c (2 + 2 K) + 0, channel c:  sum t            + 1:  sum t y
 *   2 + c (2 + 2 K) + 2 + 2 j:       C_j = sum y bc_j     + 3 + 2 j:  S_j = sum y bs_j
 * Every product and every sum is a separate IEEE fp64 operation (no fused multiply-add).
 * Order of summation: a block of 64 robots is UMPC_SPEC_SLICES = 2 wavefronts; wavefront s folds steps s, s + 2, s + 4, ..
 * of the call in order from +0, the partial sums are added in the order 0, 1 and the total is added to `sums`. Nothing
 * crosses robots, and how the K frequencies are cut into tiles on the device does not enter: a robot's sums depend on its
 * own columns, the basis rows and count alone -- bit-equal from run to run and between a column block on a handle of its
 * own and the same columns of the whole batch; no atomics, no temporaries. A chunked run calls umpcBatchSpectrum once per
 * chunk with basis_first advanced: rows 0 and 1 are exact across the cut, the other rows agree to rounding (each within
 * (n + 4) 2^-53 times the sum of its terms' magnitudes of the exact sum).
 *
 * umpcBatchSpectrumPower: one lane per robot, fp64 throughout, rounded to the handle's dtype at the store. wsum [1 + 2 K]
 * and freq_hz [K] are HOST arrays (they travel in the launch arguments): wsum the column sums of the basis rows that were
 * used, added sequentially in row order -- W0 = wsum[0], Wc_j = wsum[1 + 2 j], Ws_j = wsum[2 + 2 j] --, freq_hz the frequency
 * of each column pair in Hz (any unit: rows 6, 9 and 10 are in it). Per channel:
 *   m = sum t / W0,  var = sum t y / W0 - m m
 *   A_j = C_j - m Wc_j,  B_j = S_j - m Ws_j          (the mean is removed through the window's own transform)
 *   P_j = 4 (A_j^2 + B_j^2) / W0^2                   (an on-grid sinusoid of amplitude a gives a^2, as row 2 of a response)
 * power [3][K][B] and spec [3][UMPC_SPEC_ROWS][B] in the handle's dtype, overwritten; per channel the rows of spec:
 *   0  n, or 0 when the fit is refused            1  skipped steps
 *   2  m                                          3  var
 *   4  total = sum_j P_j, j ascending             5  peak bin, the first maximum of P_j
 *   6  freq_hz of the peak bin                    7  P of the peak bin
 *   8  peak share, row 7 / row 4                  9  centroid sum_j f_j P_j / total
 *  10  bandwidth sqrt(sum_j (f_j - centroid)^2 P_j / total)
 *  11  high share sum_{j >= jsplit} P_j / total: the chatter score (jsplit = K: 0)
 * The fit is REFUSED when skipped > 0 (the window has a hole), n != nrows (the sums are not those of the nrows basis rows
 * wsum was taken over), n < 2, or total is not > 0 and finite: row 0 is then 0 and rows 2..11 and the channel's power are
 * NaN. Nothing is clamped: rounding may put var a hair below 0. spec[c] is shaped as a score on purpose -- row 0 > 0
 * meaning "enters" -- so umpcBatchScoreQuantiles, umpcBatchScoreBootstrap and umpcBatchScoreSensitivity take it unchanged.
 * The bins are read with the factor of a frequency strictly between 0 and half the step rate; the caller keeps them there.
 *
 * umpcBatchSpectrumGroups: the cell-summed periodogram on the tables of umpcBatchGroupIndex, gspec [G][3][2 + K] DOUBLE,
 * overwritten; per group and channel: the members that enter (row 0 of spec[c] > 0), the members that do not, and per
 * frequency the sum of P_j over the members that enter (divide by column 0 for the cell's averaged periodogram). Order of
 * summation: that of umpcBatchDispersion -- lane l of 64 adds members l, l + 64, .. of the list in order from +0, then for
 * w = 32, 16, 8, 4, 2, 1 every lane becomes (itself) + (lane ^ w). A row is a function of the group's member list alone;
 * raw sums ADD over the blocks of a sharded job.
 * Not built: an MFMA Gram product (its order of accumulation is undocumented: no mirror could follow it); Welch averaging
 * over time segments; peak interpolation between bins (cross-spectra and coherence: umpcBatchCrossSpectrum, below).
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; basis, sums, wsum, freq_hz, power, spec, order, offset or gspec
 * NULL; K outside 1..64; signal outside 0..2; state_hist NULL for UMPC_SPEC_EP / ES, out_hist NULL for UMPC_SPEC_U; both or
 * neither of ref_tab and ref (UMPC_SPEC_EP / ES); count, first, ref_first or basis_first < 0; count > 2^31 - 5; nrows < 0;
 * jsplit outside 0..K; G < 1. count == 0 is a successful no-op. */
#define UMPC_SPEC_EP 0
#define UMPC_SPEC_ES 1
#define UMPC_SPEC_U 2
#define UMPC_SPEC_ROWS 12
#define UMPC_SPEC_MAX_K 64
int umpcBatchSpectrumInit(umpc_batch_t *h, int K, double *sums, void *stream);
int umpcBatchSpectrum(umpc_batch_t *h, int signal, const void *state_hist, const void *out_hist, const void *ref_tab,
                      const void *ref, const double *basis, long long basis_first, int K, long long first, long long count,
                      long long ref_first, int after, double *sums, void *stream);
int umpcBatchSpectrumPower(umpc_batch_t *h, const double *sums, const double *wsum, const double *freq_hz, int K,
                           long long nrows, int jsplit, void *power, void *spec, void *stream);
int umpcBatchSpectrumGroups(umpc_batch_t *h, const void *power, const void *spec, const int32_t *order, const int32_t *offset,
                            int G, int K, double *gspec, void *stream);

/* Trajectory modes: the Gram matrix of the error trajectories of the draws of a group, and weighted sums over the draws of a
 * group at every step. Every table above is a marginal -- one robot condensed over time, or one (step, group) condensed
 * over its draws; these two calls relate draw i of a cell to draw j of the same cell AS WHOLE TRAJECTORIES: which flight is
 * the typical one (the medoid), in how many ways the draws differ (the eigenvalues of the doubly centred Gram matrix), what
 * those ways look like over time (umpcBatchProject with the eigenvectors as weights) -- the host part is
 * robobee3d_amd/score.py, trajectory_modes / trajectory_table. Both calls are pure functions of their arguments, as
 * umpcBatchDispersion is, are asynchronous on `stream` and allocate nothing.
 * umpcBatchGram takes state_hist, ref_tab / ref (exactly ONE of the two), first, count, ref_first, after, order, offset and G
 * exactly as umpcBatchDispersion does; member slot i of group g is robot order[offset[g] + i]. The data rule is
 * umpcBatchDispersion's: a step reads 12 words per member (state rows 0..2 and 12..14, reference rows 0..5); a (member,
 * step) is SCORED when all 12 are finite; each difference is formed in the handle's dtype with one rounding, then widened;
 * y_c = scale[c] * z_c is one fp64 product; a (member, step) that is not scored contributes y = +0, selected before the
 * product. scale [6] is read on the HOST; a scale may be 0 (the default of the Python layer, (1, 1, 1, 0, 0, 0), is the
 * position error alone), and the finiteness rule does not depend on the scales.
 * gram [G][UMPC_GRAM_ROWS][UMPC_GRAM_COLS] is DOUBLE whatever the dtype. Per group of n members:
 *   [i][j], i, j < 64   Gram[i][j] = sum over the steps k and the components c of y_i,c(k) y_j,c(k); +0 where i or j >= n
 *   [64][i]             the number of steps at which slot i was scored (0 for i >= n)
 *   [65][0]             the steps accumulated        [65][1]  n        [65][2..7]  the six scales        [65][8..63]  +0
 * A group with n > 64 is FLAGGED, not computed and not an error: rows 0..63 are NaN, row 64 is 0, row 65 is as for any
 * group. A group with n = 0 holds zeros. accumulate = 0 OVERWRITES every word; accumulate = 1 ADDS this window to what the
 * table holds (the old matrix is the C operand of the first product, the counts add, [65][0] += count), so a chunked run
 * is accumulated chunk by chunk as `score` is for umpcBatchScore. IT IS THE CALLER'S DUTY TO PASS THE SAME INDEX AND THE SAME
 * SCALES to every call that accumulates into one table: the kernel does not compare them.
 * The products run on the matrix cores (v_mfma_f64_16x16x4_f64): one block of four wavefronts per group stages 8 steps of
 * y in LDS and computes the 10 upper 16 x 16 tiles; the lower triangle is their mirror image, so the stored matrix is
 * SYMMETRIC BIT FOR BIT. The k index runs over (step ascending, component 0..5 ascending), four per product, a tail padded
 * with +0. No atomics: a group's table is a function of its member list, the window and the scales alone -- not of G, the
 * other groups or the run -- and bit-identical from run to run. The order of accumulation INSIDE one product is not
 * documented, so the contract is a bound and not bit-identity with the numpy mirror (score.py, gram_reference): on data
 * whose every difference, product and partial sum is exactly representable every word equals the mirror's; otherwise
 * |gram - mirror| <= (2 N + 2) 2^-53 S_ij with N = 6 x (steps accumulated) and S_ij = sum |y_i,c(k) y_j,c(k)| (the
 * dot-product bound for any order of N products and N - 1 additions, once for each side; an entry with S_ij = 0 is exactly
 * 0). Counts and row 65 are exact.
 * umpcBatchProject: proj [count][G][UMPC_PROJ_ROWS] DOUBLE, overwritten, row i = step first + i. weights [M][B] DOUBLE on the
 * DEVICE, indexed by robot, 1 <= M <= UMPC_PROJ_MAX. Per (step, group):
 *   0  members scored          1  members skipped          2 + 6 m + c  sum_b weights[m][b] z_c(b), m < M, c = 0..5
 * and +0 in every other row. It is umpcBatchDispersion with S1 weighted and S2 dropped: the same 12 words, the same member
 * rule (a member one of whose M weights is not finite is skipped too), each term one fp64 product, the same order of
 * summation (lane l adds members l, l + 64, .. from +0, then the tree w = 32 .. 1): BIT-IDENTICAL to the mirror that follows
 * that order (score.py, project_reference), for every group size -- there is no 64-member limit here. With an eigenvector
 * of the centred Gram matrix as weights it is the time course of a mode, with 1 / n the mean path, with +-1 on two
 * clusters their contrast.
 * Not built: groups larger than 64 in umpcBatchGram; an eigensolver on the device; clustering beyond medoid and rank; a
 * split of one group's window over several blocks when G is small; attitude components in y.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; state_hist, order, offset, scale, gram, weights or proj NULL; both
 * or neither of ref_tab and ref; count, first or ref_first < 0; count > 2^31 - 1; G < 1; M outside 1..4; a scale that is
 * negative or not finite; accumulate other than 0 or 1. count == 0 is a successful no-op, except that umpcBatchGram with
 * accumulate = 0 writes the table of an empty window (zeros, n, the scales). */
#define UMPC_GRAM_ROWS 66
#define UMPC_GRAM_COLS 64
#define UMPC_PROJ_ROWS 32
#define UMPC_PROJ_MAX 4
int umpcBatchGram(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref,
                  long long first, long long count, long long ref_first, int after,
                  const int32_t *order, const int32_t *offset, int G,
                  const double *scale /* host, [6] */, int accumulate, double *gram, void *stream);
int umpcBatchProject(umpc_batch_t *h, const void *state_hist, const void *ref_tab, const void *ref,
                     long long first, long long count, long long ref_first, int after,
                     const int32_t *order, const int32_t *offset, int G,
                     const double *weights /* device, [M][B] */, int M, double *proj, void *stream);

/* Transfer estimates: how the closed loop maps an input onto an output across a band, per grid cell. umpcBatchResponse fits
 * ONE frequency the caller knows on a pure sine task; umpcBatchSpectrum keeps the power of one signal. A cell's draws are
 * independent records of the same closed loop: averaged over them, the cross-periodogram of an input x and an output y
 * gives the H1 estimate of the transfer function at every frequency of the basis, and the coherence, which says where that
 * estimate can be trusted -- a single record has coherence 1 identically, so only the cell can provide it. A broadband
 * reference per draw (a random-phase multisine or noise in the table of umpcBatchSetRefTrajectory), random pushes per step
 * (umpcBatchSetImpulses) or an attitude reference each yield the whole Bode curve of every cell, with an error bar per
 * frequency, from ONE launch and one scoring pass. All four calls are pure functions of their arguments, take only B and the
 * dtype from the handle, are asynchronous on `stream` and allocate nothing; everything is fp64 on the device except the
 * loads; every product, sum, quotient and root is a separate IEEE operation (no fused multiply-add); no atomics.
 *
 * Pairs, 3 channels each, channel c of x against channel c of y:
 *   UMPC_XS_TRACK  x = pdes, reference-table rows 0..2, slice ref_first + i;  y = p, state rows 0..2, slice first + i + after
 *   UMPC_XS_ATT    x = sdes, reference-table rows 6..8;                        y = s, state rows 9..11
 *   UMPC_XS_PUSH   x = dv_world, rows 0..2 of imp_tab [..][6][B] (the table of umpcBatchSetImpulses), slice imp_first + i;
 *                  y = p - pdes as UMPC_SPEC_EP forms it: against ref_tab, or against the constant ref (exactly ONE of the two),
 *                  the difference in the handle's dtype with one rounding, then widened exactly
 * UMPC_XS_TRACK and UMPC_XS_ATT need ref_tab and refuse ref: a constant reference has no spectrum. imp_tab is read by
 * UMPC_XS_PUSH alone. basis [W][1 + 2 K] DOUBLE on the device is umpcBatchSpectrum's (score.py spectrum_basis), step i reads
 * row basis_first + i, 1 <= K <= UMPC_SPEC_MAX_K.
 *
 * xsums [2 + 6 (2 + 2 K)][B] DOUBLE, in/out: umpcBatchCrossSpectrum ADDS into it; umpcBatchCrossSpectrumInit writes zeros.
 *   0  n, steps that entered        1  skipped steps
 *   then six blocks of 2 + 2 K rows in the layout of umpcBatchSpectrum's channels (sum w v, sum w v v, then C_j, S_j per
 *   frequency), in the order x0, x1, x2, y0, y1, y2
 * A step enters for a robot when every word it reads for BOTH signals is finite (6 words; 9 for UMPC_XS_PUSH against a table;
 * the constant reference counts); otherwise row 1 counts it and its value is +0 in every product of both signals. The order
 * of summation is umpcBatchSpectrum's: UMPC_SPEC_SLICES = 2 wavefronts per 64 robots, wavefront s folds steps s, s + 2, .. in
 * order from +0, the partial sums are added in the order 0, 1 and the total is added to `xsums`. A robot's sums depend on its
 * own columns, the basis rows and count alone -- not on how the frequencies are cut into tiles --: bit-equal from run to run,
 * between a column block on a handle of its own and the same columns of the whole batch, and with the numpy mirror
 * (score.py, cross_spectrum_sums_reference). On tables without a hole the y blocks of UMPC_XS_TRACK equal the channel blocks
 * of umpcBatchSpectrum(UMPC_SPEC_EP) against a zero reference bit for bit. A chunked run calls umpcBatchCrossSpectrum once
 * per chunk with basis_first advanced, as there.
 *
 * umpcBatchCrossSpectrumGroups: gx [G][3][2 + 4 K] DOUBLE, overwritten, on the tables of umpcBatchGroupIndex. wsum [1 + 2 K] is
 * a HOST array (it travels in the launch arguments), the column sums of the nrows basis rows that were used, as for
 * umpcBatchSpectrumPower. A member ENTERS when skipped == 0, n == nrows and n >= 2: one rule for all channels. Per member
 * and signal channel the power kernel's mean removal: m = sum w v / W0, A_j = C_j - m Wc_j, B_j = S_j - m Ws_j. Per group and
 * channel c: the members that enter, the members that do not, then per frequency j at 2 + 4 j the four sums over the members
 * that enter, each term (4 (..)) / W0^2 so that Sxx / n is the averaged periodogram in umpcBatchSpectrumPower's units:
 *   Sxx = sum (Ax Ax + Bx Bx)    Syy = sum (Ay Ay + By By)    Cxy = sum (Ax Ay + Bx By)    Qxy = sum (Bx Ay - Ax By)
 * (Cxy, Qxy) is conj(X) Y with X = A - i B: a y that LAGS x has Qxy < 0, the sign convention of umpcBatchResponseFit's phase.
 * Order of summation: umpcBatchSpectrumGroups' -- lane l of 64 adds members l, l + 64, .. of the list in order from +0, then
 * for w = 32, 16, 8, 4, 2, 1 every lane becomes (itself) + (lane ^ w). A row is a function of the group's member list alone
 * and bit-reproducible; raw sums ADD over the blocks of a sharded job (score.py, combine_cross_spectra).
 *
 * umpcBatchTransfer: tf [G][3][K][UMPC_TF_ROWS] DOUBLE from gx, overwritten; with M2 = Cxy Cxy + Qxy Qxy:
 *   0  n, members that entered, or 0 when the row is refused     1  members that did not enter
 *   2  Pxx = Sxx / n                                             3  Pyy = Syy / n
 *   4  h_re = Cxy / Sxx                                          5  h_im = Qxy / Sxx                  (the H1 estimate)
 *   6  gain = sqrt(M2) / Sxx                                     7  phase = atan2(Qxy, Cxy), negative: y lags x
 *   8  coh = M2 / (Sxx Syy)                                      9  gain_h2 = Syy / sqrt(M2)
 *  10  rel_err = sqrt((1 - coh) / ((2 n) coh))                  11  noise = Pyy (1 - coh)
 * gain <= |H| <= gain_h2 brackets the bias of noise on the input and of noise on the output; rel_err is the normalised
 * random error of the gain and the standard deviation of the phase in rad; noise is the output power the linear map leaves
 * unexplained. A row is REFUSED when n < 2 (one record's coherence is identically 1), when one of the four sums is not
 * finite, or when Sxx is not > 0: row 0 is then 0 and rows 2..11 are NaN. Rows 8..11 are NaN when Syy is not > 0. Nothing
 * else is clamped: rounding may leave coh a hair above 1 (rel_err is then NaN), and an input with no power at a bin beyond
 * rounding dust gives a meaningless row that Pxx reveals -- compare row 2 with the power the experiment put there. Every row
 * but the phase is bit-identical to the mirror (score.py, transfer_rows_reference); the phase agrees to the rounding of atan2.
 * Not built: the off-diagonal terms of the 3 x 3 (MIMO) transfer matrix; Welch averaging over time segments; a per-robot H
 * shaped as a score; the pair from the error to the command.
 * Refused (-1, umpcLastError) BEFORE any launch: h NULL; state_hist, basis, xsums, wsum, order, offset, gx or tf NULL; K
 * outside 1..64; pair outside 0..2; UMPC_XS_TRACK / ATT without ref_tab or with ref; UMPC_XS_PUSH without imp_tab, or with both
 * or neither of ref_tab and ref; count, first, ref_first, imp_first or basis_first < 0; count > 2^31 - 5; nrows < 0 or
 * > 2^53; G < 1. count == 0 is a successful no-op. */
#define UMPC_XS_TRACK 0
#define UMPC_XS_ATT 1
#define UMPC_XS_PUSH 2
#define UMPC_TF_ROWS 12
int umpcBatchCrossSpectrumInit(umpc_batch_t *h, int K, double *xsums, void *stream);
int umpcBatchCrossSpectrum(umpc_batch_t *h, int pair, const void *state_hist, const void *ref_tab, const void *ref,
                           const void *imp_tab, const double *basis, long long basis_first, int K, long long first,
                           long long count, long long ref_first, long long imp_first, int after, double *xsums, void *stream);
int umpcBatchCrossSpectrumGroups(umpc_batch_t *h, const double *xsums, const double *wsum /* host, [1 + 2 K] */, int K,
                                 long long nrows, const int32_t *order, const int32_t *offset, int G, double *gx, void *stream);
int umpcBatchTransfer(umpc_batch_t *h, const double *gx, int G, int K, double *tf, void *stream);

/* Step-kernel choice. 0 (default): automatic. fp32: the all-assembly kernel (robobee3d_amd/asmstep.py: phase A, ADMM
 * loop, phase C and the plant as one generated gfx950 stream) whenever the call is inside its scope (maxIter >= 1 and
 * row offsets within 31 bits; the task generators, per-robot weights, the fused WL step and a reference trajectory are
 * options of that stream), else the C++ kernel with the assembly ADMM loop.
 * fp64: the C++ kernel with L and 1/D in LDS and the Ruiz passes and the ADMM phase as generated fp64 assembly
 * (robobee3d_amd/asmgen64.py; one workgroup per CU at a time, maxIter >= 1, batches up to ~4.8e5 robots), else the all-C++
 * kernel.
 * In its scope the fp32 all-assembly stream exists in two forms with equal results up to rounding: one LANE per robot
 * (64 robots per wavefront: throughput; B = 65 536 is one wave per SIMD) and one lane QUAD per robot (robobee3d_amd/
 * asmquad.py: 16 robots per wavefront, ADMM iterations 2.. split over three lanes, ~0.6x the instructions per step:
 * latency). Automatic = the quad form for B <= 16 384 (and for the B = 1 drop-in of Part 1), the lane form above.
 * 1: always the C++ kernel -- fp32 around the assembly ADMM loop, fp64 with the C++ loop (ablation / cross-check).
 * 2 / 3: the assembly path in its lane / quad form whatever the batch size (a run that must equal another batch size's
 * run bit for bit -- a shard against the whole -- pins the form). fp64 has the same two forms of its assembly ADMM phase
 * (robobee3d_amd/asmquad64.py; automatic = the quad form for B <= 4 096, one workgroup per CU in one round). */
int umpcBatchSetStepKernel(umpc_batch_t *h, int mode);
/* The size of the WHOLE job this handle's batch is a block of (contiguous blocks of robots per rank; default
 * = the handle's own B). The automatic choice between the lane and the quad form is made from THIS number, so that a
 * shard runs the instruction stream the undivided batch would run and a sharded job equals the single-GPU job bit for
 * bit whatever the partition (65 536 robots as 8 blocks of 8 192 stay on the lane form). global_B < B is refused. */
int umpcBatchSetGlobalBatch(umpc_batch_t *h, long long global_B);
long long umpcBatchGlobalBatch(const umpc_batch_t *h);

/* Static facts */
int umpcBatchSize(const umpc_batch_t *h);
int umpcBatchDtype(const umpc_batch_t *h);
const int *umpcAxIdx(void);    /* 48 entries, uprightmpc2.c:65-113 */
const int *umpcKKTPerm(void);  /* 84 entries, the build's own elimination order */
int umpcNnzL(void);
const char *umpcLastError(void);
/* name of the kernel a DEFAULT rollout of this dtype dispatches (environment overrides included), and of the kernel
 * the handle's last umpcBatchRollout / umpcBatchUpdate actually dispatched ("" before the first launch): bench.py and
 * the tests attribute timings and profiles through the second one */
const char *umpcKernelName(int dtype, int plant_mode);
const char *umpcBatchKernelName(const umpc_batch_t *h);

/* The reactive baseline of the reference's gain sweeps: reactiveController (template/template_controllers.py:
 * 282-296) inside controlTest(useMPC=False) (template/uprightmpc2.py:121-151): `nsteps` plant substeps of dtsim,
 * the controller evaluated every `every` substeps (reference: 1), moments clipped at +-taulim, the handle's task
 * generator / plant mode / time. gains [6][B] = (kpos0, kpos1, kz0, kz1, ks0, ks1) or NULL (the reference's
 * defaults); out [3][B] last command or NULL; stats as in umpcBatchRollout. */
int umpcBatchReactive(umpc_batch_t *h, int nsteps, int every, void *state, const void *ref, const void *gains,
                      const void *Ib, const void *thrust_gain, void *out, void *stats, void *stream);
/* The reactive baseline on the tables of the MPC rollout: the other half of the reference's comparisons (hoverTask, sTask:
 * controlTest(useMPC=True) against controlTest(useMPC=False) on one task under one push, template/uprightmpc2.py:214-246;
 * gainTuningSims(useMPC=False), :272-303) as ONE launch that reads and writes what umpcBatchRollout reads and writes.
 * K closed-loop steps of nsub substeps of dtsim each -- the granularity of umpcBatchRollout, so every table keeps its shape
 * and meaning. The controller fires at the substeps j of a step with j % every == 0; `every` must divide nsub (a run cut
 * into several launches then fires at the same substeps). Moments are clipped at +-taulim; gains, Ib, thrust_gain, out
 * [3][B] or NULL and stats (accumulated per substep) are those of umpcBatchReactive.
 * The reference of substep j of step k is one of three, chosen once per call:
 *   handle task      task == NULL and no reference trajectory set: the handle's task at t = t0 + T(k nsub + j) dtsim, the
 *                    expression of umpcBatchReactive. With nothing else set the call equals umpcBatchReactive(h, K nsub,
 *                    every, ...) bit for bit in state, out, stats and umpcBatchTime.
 *   per-robot task   task [B] int32 of UMPC_TASK_* ids, task_params [4][B] in the handle's dtype or NULL (= the handle's),
 *                    layout as in umpcBatchTaskTable; rows 0..2 of ref are initialPos, task 0 follows its ref column.
 *                    Evaluated per substep at the same t. Refused while a reference trajectory is set. Robots of different
 *                    tasks in one wavefront (64 consecutive robots) run their generators one after the other: a sweep
 *                    keeps the robots of one task adjacent.
 *   reference table  umpcBatchSetRefTrajectory set: pdes = rows 0..2 of slice ref_cursor + k, held over the substeps of
 *                    step k; ref may be NULL; the cursor advances by K. No time expression enters.
 * Impulses (umpcBatchSetImpulses): slice imp_cursor + k is added to dq after the last substep of step k and before anything
 * of that step is stored -- the placement and the single IEEE add of umpcBatchRollout.
 * Step history (umpcBatchSetHistory; any record may be off): state slice c = `state` as passed (the kernel stores the words
 * it loaded: no copy), slice c + k + 1 = the state after step k, kick included; out slice c + k = (thrust, clipped moments)
 * of the last fire of the step in rows 0..2 and 0 in rows 3..8 (a reactive controller has no accdes); status = 1; info = 0.
 * The tables stay fully defined -- umpcBatchScore takes them as they are, its row 8 counts nothing -- and `state` / `out`
 * hold after the call what they hold without a history.
 * Every range check (trajectory, history, impulses) is made BEFORE the launch; the clock and the three cursors move after
 * the launch has been accepted and nowhere else. Refused (-1, umpcLastError): h NULL, K < 1, every < 1, nsub % every != 0,
 * a handle with nsub = 0, state NULL, ref NULL without a table, task_params without task, task with a table set, K * nsub
 * > 2^31 - 1. Slice offsets are 64-bit: a table may pass 4 GB (the state history does after 455 steps at B = 65 536 in
 * fp32). Both dtypes, both plant modes. Asynchronous on `stream`. */
int umpcBatchReactiveRollout(umpc_batch_t *h, int K, int every, void *state, const void *ref, const void *gains,
                             const int32_t *task, const void *task_params, const void *Ib, const void *thrust_gain, void *out,
                             void *stats, void *stream);
/* out [9][B] = (pdes, dpdes, sdes) of the handle's task (template/flight_tasks.py:6-49) at time t_ms, what the
 * step kernel evaluates at an MPC fire; ref as in umpcBatchRollout (rows 0..2 = initialPos for a task). */
int umpcBatchTaskReference(umpc_batch_t *h, double t_ms, const void *ref, void *out, void *stream);

/* ------------------------------------------------------------------ */
/* Part 3: wrench-linearisation step (the consumer of accdes)          */
/* template/uprightmpc2/funapprox.h:18-54, funapprox.c:102-176          */
/* ------------------------------------------------------------------ */
#define NDELU 4
typedef struct {
  int k;
  float a0;
  float a1[NDELU];
  float A2[NDELU * NDELU];
} FunApprox_t; /* funapprox.h:18-23 */

typedef struct {
  float u0[NDELU], umin[NDELU], umax[NDELU], dumax[NDELU];
  float Qw[6 * 6];
  FunApprox_t fa[6];
} WLCon_t; /* funapprox.h:37-41; caller-allocated, holds ALL state (u0) like the reference */

/* funapprox.h:43 / funapprox.c:102-116. popts: 6 x (a0, a1[4], upper-triangular A2 row-major [10]). */
void wlConInit(WLCon_t *wl, const float u0[/* 4 */], const float umin[/* 4 */], const float umax[/* 4 */],
               const float dumax[/* 4 */], const float Qw[/* 6 */], float controlRate,
               const float popts[/* 90 */]);
/* funapprox.h:45 / funapprox.c:118-165: w0 = w(u0); one projected-gradient step of
 * |w(u) - h0 - pdotdes|^2_Qw with step 1e3, clipped to the rate limit and frozen at the box. */
void wlConUpdate(WLCon_t *wl, float u1[/* 4 */], float w0[/* 6 */], const float h0[/* 6 */],
                 const float pdotdes[/* 6 */]);
/* funapprox.h:48 / funapprox.c:171-176 */
void wlconS(float u1_y1[/* 4 */], float w0_y2[/* 6 */], const float u0init_u1[/* 4 */],
            const float umin_u2[/* 4 */], const float umax_u3[/* 4 */], const float dumax_u4[/* 4 */],
            const float Qw_u5[/* 6 */], float controlRate_u6, const float popts_u7[/* 90 */],
            const float h0_u8[/* 6 */], const float pdotdes_u9[/* 6 */]);

/* Batched: `wl` supplies limits, weights and wrench-map coefficients for every robot (its u0 is
 * ignored); u [4][B] is the per-robot input state (in: u0, out: u1), h0 / pdotdes [6][B] in,
 * w0 [6][B] out. fp32 (UMPC_F32) or fp64 device arrays. Asynchronous on `stream`. */
int umpcBatchWLUpdate(const WLCon_t *wl, int B, int dtype, void *u, const void *h0, const void *pdotdes,
                      void *w0, void *stream);

/* The coupling of the two steps as every real caller of the reference wires them
 * (template/robobee_test_controllers.py:162-171, template/uprightmpc2/conn_MPC_WL.m:2-10), FUSED into the step
 * kernel: after each MPC step of umpcBatchRollout / umpcBatchUpdate
 *     h0 = (Rb' (0, 0, mb g), 0, 0, 0),  pdotdes = M0 accdes,  (u4, w0) = wlConUpdate(h0, pdotdes),
 *     actualT0 = w0[2] / M0[2,2]  -> overrides the thrust accumulator of the NEXT step when >= 0
 * with M0 = diag(Mdiag) (dynamicsTerms, template/ca6dynamics.py:5-10,44-50: (100,100,100,3333,3333,1000)) and g
 * the handle's g. wl: parameters (umin, umax, dumax, Qw, fa; its u0 is ignored), copied to the device here
 * (synchronous); NULL switches the coupling off. u4 [4][B]: per-robot WL input state, in/out, kept by pointer;
 * w0 [6][B] or NULL: wrench w(u4) evaluated by the last step. */
int umpcBatchSetWL(umpc_batch_t *h, const WLCon_t *wl, const double Mdiag[/* 6 */], void *u4, void *w0);

/* ------------------------------------------------------------------ */
/* Part 4: the reference's other rigid-body vector fields */
/* ------------------------------------------------------------------ */
/* UMPC_MODEL_CA6: template/ca6dynamics.py:35-50. y [18][B] = (p, R column-major, dq = (v_world, omega_body)),
 *   u [6][B] = (u1L,u2L,u3L,u1R,u2R,u3R); wrenchMap + M ddq = w - h (h = (R'(0,0,mb g), 0), body frame).
 * UMPC_MODEL_TSD: ThrustStrokeDev.dynamics, template/FlappingModels3D.py:19-38. y [12][B] = (p, rotvec, v, omega),
 *   u [4][B] = (FzL, dxL, FzR, dxR), restated as written.
 * nsub == 0: aux receives ydot ([18] or [12] rows; CA6 appends wrench [6] and h [6] -> 30 rows), y unchanged.
 * nsub  > 0: y advances by nsub classical RK4 steps of dt with u held (build-defined integrator: the
 *            reference has none for these models); aux unused. */
#define UMPC_MODEL_CA6 0
#define UMPC_MODEL_TSD 1
int umpcBatchModel(int model, int B, int dtype, int nsub, double dt, void *y, const void *u, void *aux,
                   void *stream);

/* ------------------------------------------------------------------ */
/* Part 5: general-structure batch QP            */
/* ------------------------------------------------------------------ */
/* The embedded-OSQP step of Part 1/2 for an ARBITRARY structure: min 1/2 x'Px + q'x s.t. l <= Ax <= u with
 * P diagonal on a subset of the columns and A sparse. This is what the reference's other MPC formulations hand
 * to `osqp.OSQP().setup / update / solve`: planar/mpc_osqp_p5f.py:87-147,172 (n = 87, m = 164 at N = 10),
 * template/genqp.py:43-168 (v1 UprightMPC, n = m = 9N), template/template_controllers.py:170-258 (UprightMPC2 at
 * any horizon N). The sparsity is analysed on the host (robobee3d_amd/qpstruct.py: KKT ordering, elimination
 * tree, LDL' schedule = what OSQP's code generator bakes into workspace.c:743-2467) and handed over as one int32
 * table blob. Per call and per robot: 10 Ruiz passes, row classification, numeric LDL', max_iter ADMM
 * iterations (no early exit), residuals / status / solution -- the call sequence of
 * template/uprightmpc2/osqp.c:288-641,752-833,1158-1266 in canonical-restart form. */
typedef struct {
  double rho, sigma, alpha, eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
  int max_iter, scaling;
  /* 0 (default, the embedded reference: uprightmpc2.c:116-117): exactly max_iter iterations, no early exit.
   * k > 0: the pip-osqp semantics of the reference's Python twin (template_controllers.py:190-191, 216-219;
   * osqp.c:411-450): every k-th iteration update_info + check_termination at the exact tolerances, a robot that
   * meets a criterion stops iterating (per-lane mask; osqp's default k = 25, max_iter = 4000). Runs on the
   * table-driven kernel. */
  int check_termination;
  /* 0 (default; the embedded reference has none): fixed rho. k > 0: adapt_rho (auxil.c:12-82, osqp.c:482-520,
   * 1268-1330) every k iterations: rho <- rho sqrt(rel. primal / rel. dual residual) when it changes by more than
   * 5x, rho_vec by constraint type, numeric refactorisation. pip osqp derives its interval from wall-clock timings
   * (osqp.c:455-480: a multiple of check_termination), so any multiple of 25 is a behaviour the reference's
   * Python twin can show; the twin here uses 25. */
  int adaptive_rho_interval;
} umpcQPSettings;
/* the reference's generated settings (workspace.c) with umpcInit's max_iter = 50 (uprightmpc2.c:116-117) */
void umpcQPDefaultSettings(umpcQPSettings *s);
/* blob: robobee3d_amd/qpstruct.py layout (64-word header, 18 index tables); validated here. NULL on error. */
void *umpcQPCreate(const int32_t *blob, int nwords, int B, int dtype, const umpcQPSettings *settings);
void umpcQPDestroy(void *h);
int umpcQPSetMaxIter(void *h, int max_iter);
int umpcQPSetCheckTermination(void *h, int every);
int umpcQPSetAdaptiveRho(void *h, int interval);
/* For the structures known at build time (robobee3d_amd/codegen_qp.py: planar p5f N = 10, v1 N = 3, UprightMPC2
 * N = 5) umpcQPCreate selects a generated straight-line kernel (same arithmetic, literal indices). UseTables(1)
 * forces the table-driven kernel; returns the index of the specialisation or -1. KernelName: its name or "tables". */
int umpcQPUseTables(void *h, int on);
/* Kernel choice. 1 (default): one LANE per robot (the build-time specialisation if there is one, else the
 * table-driven kernel). 2: lane per robot, tables. 0: one WAVEFRONT per robot, working set in LDS, level-scheduled
 * solves (needs the working set to fit a CU's LDS; faster for the planar p5f structure at B = 16 384, slower on
 * the others measured -- DESIGN.md 10). 3: as 1 but without the assembly loop some specialisations carry (fp32 planar
 * p5f: the middle ADMM iterations as generated gfx950 assembly, robobee3d_amd/asmqp.py; results equal to rounding). */
int umpcQPSetKernel(void *h, int mode);
/* "wave", the specialisation's name ("+asm" appended when its assembly loop will run), or "tables" */
const char *umpcQPKernelName(void *h);
/* All arrays are DEVICE pointers, SoA [rows][B] of the handle's dtype:
 *   Pv [nnzP], Av [nnzA] (CSC order), q [n], l, u [m]   raw problem data                     in
 *   x [n], y [m], z [m]   OSQP's (scaled) iterates, warm start                                in/out
 *   Eprev [m]             E of the previous call (1 before the first), osqp.c:812-820          in/out
 *   sol_x [n], sol_y [m]  unscaled solution (NaN on an infeasibility status) or NULL           out
 *   status [B] int32 (OSQP codes) or NULL; info [6][B] = pri_res, dua_res, c, zero-pivot flag, iterations run,
 *                         rho updates, or NULL
 * Asynchronous on `stream`. */
int umpcQPSolve(void *h, const void *Pv, const void *Av, const void *q, const void *l, const void *u, void *x,
                void *y, void *z, void *Eprev, void *sol_x, void *sol_y, int32_t *status, void *info, void *stream);
/* out[k][b] = src[k] < 0 ? cst[k] : cst[k] * par[src[k]][b]  (k < nnz): fills a value array whose entries are
 * constants or scaled per-robot parameters, e.g. A <- kron(I,-I) + kron(eye(k=-1), Ad) | kron(.., Bd) of
 * planar/mpc_osqp_p5f.py:168-170. cst, src are device arrays of length nnz. */
int umpcQPGather(int B, int dtype, int nnz, const void *cst, const int32_t *src, const void *par, void *out,
                 void *stream);
/* The same for the entries with src[k] >= 0 only: `out` already holds the constant entries from an earlier umpcQPGather
 * with the same cst / src (the reference rewrites only the Ad / Bd blocks of its A every tick, mpc_osqp_p5f.py:168-170). */
int umpcQPGatherUpdate(int B, int dtype, int nnz, const void *cst, const int32_t *src, const void *par, void *out,
                       void *stream);
/* planar/mpc_osqp_p5f.py: getLin (:45-85) at (u[b], sigma = y[0][b], phi = y[3][b]) -> lin [5][B] =
 * (Ad[4][3], Ad[5][3], Bd[4], Bd[5], Bd[6]); mode 1 additionally applies the reference's plant tick
 * y <- y + (Ad y + Bd u) dt (:176). y [7][B], u [B]; lin may be NULL in mode 1. */
int umpcP5fStep(int B, int dtype, int mode, double dt, const void *u, void *y, void *lin, void *stream);
/* The same with ONE nominal input for the whole batch, as the reference's loop has it (unom = 15 sin(2 pi 170 t) is a
 * scalar, planar/mpc_osqp_p5f.py:157): no [B] array to fill per tick. */
int umpcP5fStepU(int B, int dtype, int mode, double dt, double u, void *y, void *lin, void *stream);
/* getLin and the A update of one tick (mpc_osqp_p5f.py:165-170) in ONE launch: umpcP5fStep[U] mode 0 followed by
 * umpcQPGather (update = 0) or umpcQPGatherUpdate (update != 0) with par = lin; the entries of the structure refer to lin
 * rows (src[k] in 0..4). u [B] or NULL (then u_all is every robot's input); lin [5][B], Av [nnz][B] as above. */
int umpcP5fLinearise(int B, int dtype, const void *u, double u_all, const void *y, void *lin, int nnz, const void *cst,
                     const int32_t *src, void *Av, int update, void *stream);
/* One tick of planar/mpc_osqp_p5f.py:157-176 in ONE launch (round 5): umpcP5fLinearise (getLin at (unom, y[0], y[3]) -> lin and
 * the state-dependent entries of Av) + umpcQPSolve + umpcP5fStepU(mode 1) (the plant tick y += (Ad y + Bd unom) dt), with the
 * first and the last folded into the prologue of the QP kernel (they depend on the previous state only). Same arguments as
 * umpcQPSolve, then the tick's: Av is rewritten in place where src[k] >= 0 (its constant entries must be there already: a
 * first tick goes through umpcP5fLinearise), ystate [7][B] is advanced, lin [5][B] may be null. Only for a handle that
 * dispatches the fp32 p5f10 assembly kernel; returns -2 (and does nothing) otherwise, so that a caller can fall back to the
 * three calls. Results are the three calls' bit for bit. */
int umpcP5fTick(void *h, const void *Pv, void *Av, const void *q, const void *l, const void *u, void *x, void *y, void *z,
                void *Eprev, void *sol_x, void *sol_y, int32_t *status, void *info, double unom, double dt, void *ystate,
                void *lin, int nnz, const void *cst, const int32_t *src, void *stream);
/* UprightMPC2 at any horizon N (template/template_controllers.py:170-258; N = 3 is Parts 1-2's specialised path):
 * assembly (updateConstraint :65-125, updateObjective :127-143 = uprightmpc2.c:121-207) and extraction (update2 /
 * getAccDes :232-250 = uprightmpc2.c:253-269) around umpcQPSolve on the structure of initConstraint (:28-63).
 *   state [18][B] (p, R column-major, dq), ref [9][B] (pdes, dpdes, sdes), T0 [B] in/out, actualT0 [B] or NULL
 *   Pv [nx], q [nx], l, u [nc]  (nx = 15 N, nc = 13 N);  par [10][B] = (dt T0, dt s0[3], dt Btau[6]) for umpcQPGather
 *   out [9][B] = (uquad[3], accdes[6]); T0 <- T0 + x[12 N]. */
typedef struct {
  double dt, g, TtoWmax, ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom, Ib[3];
} umpcNParams;
int umpcNAssemble(int B, int dtype, int N, const umpcNParams *p, const void *state, const void *ref, void *T0,
                  const void *actualT0, void *Pv, void *q, void *l, void *u, void *par, void *stream);
int umpcNExtract(int B, int dtype, int N, double dt, const void *state, const void *sol_x, void *T0, void *out,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UMPC_MI355X_H */
