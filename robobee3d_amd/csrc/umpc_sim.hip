// libumpc_mi355x.so, simulation without the solver: the plant, the reactive baseline, the task references and tables, the
// wrench-linearisation step and the other rigid-body models, each with its entry points. Everything here is built on
// umpc_plant.h and umpc_models.h: no QP, no generated header.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "umpc_handle.h"
#include "umpc_models.h"

namespace {

using umpc::DevParams;
using umpc::WLDev;

template <typename T>
__global__ __launch_bounds__(kBlock) void umpc_plant_kernel(DevParams<T> prm, int B_, int nsub, T *state,
                                                            const T *u, const T *IbA, const T *gainA) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  T p[3], R[9], dq[6], uq[3], Ib[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { p[i] = state[(size_t)i * B + b]; uq[i] = u[(size_t)i * B + b]; }
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = state[(size_t)(3 + i) * B + b];
#pragma unroll
  for (int i = 0; i < 6; ++i) dq[i] = state[(size_t)(12 + i) * B + b];
#pragma unroll
  for (int i = 0; i < 3; ++i) Ib[i] = IbA ? IbA[(size_t)i * B + b] : prm.Ib[i];
  const T gain = gainA ? gainA[b] : T(1);
  const T Ibinv[3] = {T(1) / Ib[0], T(1) / Ib[1], T(1) / Ib[2]};
#pragma nounroll
  for (int s = 0; s < nsub; ++s) umpc::plant_step(p, R, dq, uq, prm.dtsim, Ib, Ibinv, gain, prm.plant_mode);
#pragma unroll
  for (int i = 0; i < 3; ++i) state[(size_t)i * B + b] = p[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) state[(size_t)(3 + i) * B + b] = R[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) state[(size_t)(12 + i) * B + b] = dq[i];
}

// reactiveController (template/template_controllers.py:282-296) in the closed loop of controlTest with
// useMPC=False (template/uprightmpc2.py:121-151): the reference evaluates it at every plant substep
// (hlInterval=None); `every` > 1 holds the command for that many substeps (fixed schedule).
// gains rows: kpos[2], kz[2], ks[2] (defaults 5e-3, 5e-1 | 1e-1, 1 | 10, 1e2).
template <typename T>
__device__ __forceinline__ void reactive_controller(const T (&p)[3], const T (&R)[9], const T (&dq)[6],
                                                    const T (&pdes)[3], const T (&k)[6], T (&u)[3]) {
  T sdes[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    sdes[i] = umpc::umpc_min(umpc::umpc_max(k[0] * (pdes[i] - p[i]) - k[1] * dq[i], T(-0.5)), T(0.5));
  sdes[2] = T(1);
  T ds[3], fT[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    ds[r] = -(R[r] * (-dq[4]) + R[r + 3] * dq[3]);      // -Rb e3h omega
    fT[r] = k[4] * (R[6 + r] - sdes[r]) + k[5] * ds[r];
  }
  fT[2] = T(0);
  // fAorn = -e3h Rb' fTorn = ((Rb' f)_y, -(Rb' f)_x, 0)
  const T wx = (R[0] * fT[0] + R[1] * fT[1]) + R[2] * fT[2];
  const T wy = (R[3] * fT[0] + R[4] * fT[1]) + R[5] * fT[2];
  u[0] = k[2] * (pdes[2] - p[2]) - k[3] * dq[2];
  u[1] = wy;
  u[2] = -wx;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void umpc_reactive_kernel(DevParams<T> prm, int B_, int nsteps, int every, T t0,
                                                              T *state, const T *ref, const T *gains, const T *IbA,
                                                              const T *gainA, T *out, T *stats, const T *imp, int nsub) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  T p[3], R[9], dq[6], Ib[3], rf0[9], k[6] = {T(5e-3), T(5e-1), T(1e-1), T(1e0), T(10e0), T(1e2)}, u[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = state[(size_t)i * B + b];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = state[(size_t)(3 + i) * B + b];
#pragma unroll
  for (int i = 0; i < 6; ++i) dq[i] = state[(size_t)(12 + i) * B + b];
#pragma unroll
  for (int i = 0; i < 9; ++i) rf0[i] = ref[(size_t)i * B + b];
#pragma unroll
  for (int i = 0; i < 3; ++i) Ib[i] = IbA ? IbA[(size_t)i * B + b] : prm.Ib[i];
  if (gains) {
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = gains[(size_t)i * B + b];
  }
  const T gain = gainA ? gainA[b] : T(1);
  const T Ibinv[3] = {T(1) / Ib[0], T(1) / Ib[1], T(1) / Ib[2]};
  T s_err = stats ? stats[b] : T(0), s_eff = stats ? stats[B + b] : T(0);
#pragma nounroll
  for (int ti = 0; ti < nsteps; ++ti) {
    if (ti % every == 0) {
      T rf[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) rf[i] = rf0[i];
      umpc::task_reference(prm.task, prm.task_p, t0 + T(ti) * prm.dtsim, rf);
      const T pdes[3] = {rf[0], rf[1], rf[2]};
      reactive_controller(p, R, dq, pdes, k, u);
      u[1] = umpc::umpc_min(umpc::umpc_max(u[1], -prm.taulim), prm.taulim);
      u[2] = umpc::umpc_min(umpc::umpc_max(u[2], -prm.taulim), prm.taulim);
    }
    umpc::plant_step(p, R, dq, u, prm.dtsim, Ib, Ibinv, gain, prm.plant_mode);
    s_err += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    s_eff += u[1] * u[1] + u[2] * u[2];
    // velocity impulses (umpcBatchSetImpulses): slice j of `imp` after substep (j + 1) * nsub - 1, where the rollout adds it
    if (imp && (ti + 1) % nsub == 0) {
      const T *const imp_j = imp + (size_t)((ti + 1) / nsub - 1) * 6 * B;
#pragma unroll
      for (int i = 0; i < 6; ++i) dq[i] += imp_j[(size_t)i * B + b];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) state[(size_t)i * B + b] = p[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) state[(size_t)(3 + i) * B + b] = R[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) state[(size_t)(12 + i) * B + b] = dq[i];
  if (out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[(size_t)i * B + b] = u[i];
  }
  if (stats) { stats[b] = s_err; stats[B + b] = s_eff; }
}

// The reactive baseline on the tables of the MPC rollout (umpcBatchReactiveRollout): K closed-loop steps of nsub substeps,
// with a reference per robot, the impulse table and the step history. Where pdes comes from is decided on the host, once
// per call, and is a template parameter: the substep loop holds no test of a table pointer and no load.
//   kRefHandle  the handle's task at t = t0 + T(k nsub + j) dtsim -- the expression of umpc_reactive_kernel, so with no
//               table set the two kernels run the same arithmetic on the same values
//   kRefRobot   the same expression with the robot's own task id and parameters (lanes of different tasks diverge inside
//               task_reference: a sweep keeps the robots of one task adjacent)
//   kRefTable   rows 0..2 of one slice of the reference trajectory per step, held over its substeps: no time expression
// One lane per robot, robot index fastest: every access below is one coalesced row segment, nothing crosses robots. The
// table pointers move on one slice per step as 64-bit pointers, so a table may pass 4 GB.
enum { kRefHandle = 0, kRefRobot = 1, kRefTable = 2 };

template <typename T>
struct ReactiveSteps {
  DevParams<T> prm;
  int B, K, nsub, every;
  T t0;
  T *state;
  const T *ref, *gains, *Ib, *gain;
  T *out, *stats;
  const int32_t *task;     // kRefRobot: [B] ids
  const T *task_params;    // kRefRobot: [4][B] or null (= the handle's)
  const T *reftab;         // kRefTable: the slice of step 0
  const T *imp;            // the impulse slice of step 0, or null
  T *h_state;              // the history slices of step 0 (state: the slice BEFORE it), each may be null
  T *h_out;
  int32_t *h_status;
  T *h_info;
};

template <typename T, int SRC>
__global__ __launch_bounds__(kBlock) void umpc_reactive_steps_kernel(ReactiveSteps<T> a) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= a.B) return;
  const size_t B = (size_t)a.B;
  const DevParams<T> &prm = a.prm;
  T p[3], R[9], dq[6], Ib[3], ip[3] = {T(0), T(0), T(0)}, tp[4];
  T k[6] = {T(5e-3), T(5e-1), T(1e-1), T(1e0), T(10e0), T(1e2)}, u[3] = {T(0), T(0), T(0)};
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = a.state[(size_t)i * B + b];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = a.state[(size_t)(3 + i) * B + b];
#pragma unroll
  for (int i = 0; i < 6; ++i) dq[i] = a.state[(size_t)(12 + i) * B + b];
  // state slice c of the history: the registers just loaded
  T *hs = a.h_state;
  if (hs) {
#pragma unroll
    for (int i = 0; i < 3; ++i) hs[(size_t)i * B + b] = p[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) hs[(size_t)(3 + i) * B + b] = R[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) hs[(size_t)(12 + i) * B + b] = dq[i];
    hs += 18 * B;
  }
  int tk = prm.task;
#pragma unroll
  for (int i = 0; i < 4; ++i) tp[i] = prm.task_p[i];
  if constexpr (SRC != kRefTable) {
    // (the reactive controller reads pdes only, and every generator takes rows 0..2 = initialPos and nothing else)
#pragma unroll
    for (int i = 0; i < 3; ++i) ip[i] = a.ref[(size_t)i * B + b];
  }
  if constexpr (SRC == kRefRobot) {
    tk = a.task[b];
    if (a.task_params) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tp[i] = a.task_params[(size_t)i * B + b];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) Ib[i] = a.Ib ? a.Ib[(size_t)i * B + b] : prm.Ib[i];
  if (a.gains) {
#pragma unroll
    for (int i = 0; i < 6; ++i) k[i] = a.gains[(size_t)i * B + b];
  }
  const T gain = a.gain ? a.gain[b] : T(1);
  const T Ibinv[3] = {T(1) / Ib[0], T(1) / Ib[1], T(1) / Ib[2]};
  T s_err = a.stats ? a.stats[b] : T(0), s_eff = a.stats ? a.stats[B + b] : T(0);
  const T *imp = a.imp, *rt = a.reftab;
  T *ho = a.h_out, *hi = a.h_info;
  int32_t *hst = a.h_status;
  int ti = 0;
#pragma nounroll
  for (int ks = 0; ks < a.K; ++ks) {
    // the words of this step that come from tables, ahead of its substeps (which hide the miss); used after the last one
    T kick[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, pdes[3] = {ip[0], ip[1], ip[2]};
    if (imp) {
#pragma unroll
      for (int i = 0; i < 6; ++i) kick[i] = imp[(size_t)i * B + b];
      imp += 6 * B;
    }
    if constexpr (SRC == kRefTable) {
#pragma unroll
      for (int i = 0; i < 3; ++i) pdes[i] = rt[(size_t)i * B + b];
      rt += 9 * B;
    }
    int hold = 0;      // substeps until the controller fires again: j % every == 0, counted down
#pragma nounroll
    for (int j = 0; j < a.nsub; ++j, ++ti) {
      if (hold == 0) {
        hold = a.every;
        if constexpr (SRC != kRefTable) {
          T rf[9] = {ip[0], ip[1], ip[2], T(0), T(0), T(0), T(0), T(0), T(0)};
          umpc::task_reference(tk, tp, a.t0 + T(ti) * prm.dtsim, rf);
          pdes[0] = rf[0]; pdes[1] = rf[1]; pdes[2] = rf[2];
        }
        reactive_controller(p, R, dq, pdes, k, u);
        u[1] = umpc::umpc_min(umpc::umpc_max(u[1], -prm.taulim), prm.taulim);
        u[2] = umpc::umpc_min(umpc::umpc_max(u[2], -prm.taulim), prm.taulim);
      }
      --hold;
      umpc::plant_step(p, R, dq, u, prm.dtsim, Ib, Ibinv, gain, prm.plant_mode);
      s_err += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
      s_eff += u[1] * u[1] + u[2] * u[2];
    }
    // velocity impulse of the step (umpcBatchSetImpulses): after its last substep, ahead of everything it stores
    if (imp) {
#pragma unroll
      for (int i = 0; i < 6; ++i) dq[i] += kick[i];
    }
    // the records of the step (wave-uniform tests, once per step; the stores are issued and not waited for)
    if (hs) {
#pragma unroll
      for (int i = 0; i < 3; ++i) hs[(size_t)i * B + b] = p[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) hs[(size_t)(3 + i) * B + b] = R[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) hs[(size_t)(12 + i) * B + b] = dq[i];
      hs += 18 * B;
    }
    if (ho) {      // (thrust, clipped moments, accdes = 0: a reactive controller has none)
#pragma unroll
      for (int i = 0; i < 3; ++i) ho[(size_t)i * B + b] = u[i];
#pragma unroll
      for (int i = 3; i < 9; ++i) ho[(size_t)i * B + b] = T(0);
      ho += 9 * B;
    }
    if (hst) { hst[b] = 1; hst += B; }      // OSQP_SOLVED: the step counts as solved in a score
    if (hi) { hi[b] = T(0); hi[B + b] = T(0); hi += 2 * B; }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) a.state[(size_t)i * B + b] = p[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) a.state[(size_t)(3 + i) * B + b] = R[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) a.state[(size_t)(12 + i) * B + b] = dq[i];
  if (a.out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.out[(size_t)i * B + b] = u[i];
  }
  if (a.stats) { a.stats[b] = s_err; a.stats[B + b] = s_eff; }
}

// (pdes, dpdes, sdes) of the handle's task at time t for every robot (what the step kernel evaluates at a fire)
template <typename T>
__global__ void umpc_taskref_kernel(DevParams<T> prm, int B_, T t, const T *ref, T *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  T r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = ref[(size_t)i * B + b];
  umpc::task_reference(prm.task, prm.task_p, t, r);
#pragma unroll
  for (int i = 0; i < 9; ++i) out[(size_t)i * B + b] = r[i];
}

// Per-robot task tables (umpcBatchTaskTable): slice k of tab [steps][9][B] = task_reference(task[b], params[.][b], t_k, ref
// column b) at the fire time t_k of closed-loop step k -- the SAME device function and the SAME expression for t_k, in the
// same scalar type, as closed_loop_step (umpc_step.h) and umpc_taskf_kernel, so a table with batch-constant parameters holds
// exactly what the step kernel would generate. 2-D grid: x = robots (robot index fastest: every store of a warp is one
// coalesced row segment), y = a grid stride over the steps; a thread loads its robot's task, parameters and ref column once
// and reuses them for all its steps. task 0 copies the ref column.
template <typename T>
__global__ void umpc_task_table_kernel(DevParams<T> prm, int B_, long long steps, T t0, const int32_t *task, const T *params,
                                       const T *ref, T *tab) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  const int tk = task ? task[b] : prm.task;
  T tp[4], r0[9];
#pragma unroll
  for (int i = 0; i < 4; ++i) tp[i] = params ? params[(size_t)i * B + b] : prm.task_p[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) r0[i] = ref[(size_t)i * B + b];
  for (long long k = blockIdx.y; k < steps; k += gridDim.y) {
    T r[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) r[i] = r0[i];
    const T tnow = t0 + T(k) * (T(prm.nsub) * prm.dtsim);
    umpc::task_reference(tk, tp, tnow, r);
    T *o = tab + (size_t)k * 9 * B;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[(size_t)i * B + b] = r[i];
  }
}

// ---------------------------------------------------------------------------
// Part 3: wrench-linearisation step, funapprox.c
// ---------------------------------------------------------------------------
// one lane = one robot: w0 = w(u0), A1 = dw/du(u0), one clipped gradient step (funapprox.c:118-165)
template <typename T>
__global__ __launch_bounds__(256) void umpc_wl_kernel(WLDev p, int B_, T *u, const T *h0, const T *pd, T *w0out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  T u0[4], h[6], d[6], w[6];
#pragma unroll
  for (int j = 0; j < 4; ++j) u0[j] = u[(size_t)j * B + b];
#pragma unroll
  for (int i = 0; i < 6; ++i) { h[i] = h0[(size_t)i * B + b]; d[i] = pd[(size_t)i * B + b]; }
  umpc::wl_step(p, u0, h, d, w);
#pragma unroll
  for (int i = 0; i < 6; ++i) w0out[(size_t)i * B + b] = w[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) u[(size_t)j * B + b] = u0[j];
}

// a19 / a20 vector fields: nsub == 0 evaluates ydot (ca6 also appends wrench and bias h), nsub > 0
// advances y by nsub RK4 steps of dt with u held
template <typename T, int MODEL>
__global__ __launch_bounds__(256) void umpc_model_kernel(int B_, int nsub, T dt, T *y, const T *u, T *aux) {
  constexpr int NYV = MODEL == 0 ? 18 : 12, NUV = MODEL == 0 ? 6 : 4;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B_) return;
  const size_t B = (size_t)B_;
  T yv[NYV], uv[NUV];
#pragma unroll
  for (int i = 0; i < NYV; ++i) yv[i] = y[(size_t)i * B + b];
#pragma unroll
  for (int i = 0; i < NUV; ++i) uv[i] = u[(size_t)i * B + b];
  auto vf = [&](const T (&ys)[NYV], T (&k)[NYV]) {
    if constexpr (MODEL == 0) {
      T w[6], h[6];
      umpc::ca6_vf(ys, uv, k, w, h);
    } else {
      umpc::tsd_vf(ys, uv, k);
    }
  };
  if (nsub == 0) {
    T k[NYV];
    vf(yv, k);
#pragma unroll
    for (int i = 0; i < NYV; ++i) aux[(size_t)i * B + b] = k[i];
    if constexpr (MODEL == 0) {
      T w[6], h[6], kk[NYV];
      umpc::ca6_vf(yv, uv, kk, w, h);
#pragma unroll
      for (int i = 0; i < 6; ++i) { aux[(size_t)(18 + i) * B + b] = w[i]; aux[(size_t)(24 + i) * B + b] = h[i]; }
    }
    return;
  }
#pragma nounroll
  for (int s = 0; s < nsub; ++s) umpc::rk4_step<T, NYV>(yv, dt, vf);
#pragma unroll
  for (int i = 0; i < NYV; ++i) y[(size_t)i * B + b] = yv[i];
}

WLDev make_wl(const WLCon_t *wl) {
  WLDev d;
  for (int j = 0; j < 4; ++j) { d.umin[j] = wl->umin[j]; d.umax[j] = wl->umax[j]; d.dumax[j] = wl->dumax[j]; }
  for (int i = 0; i < 6; ++i) {
    d.Qw[i] = wl->Qw[i + 6 * i];
    d.a0[i] = wl->fa[i].a0;
    for (int j = 0; j < 4; ++j) d.a1[i][j] = wl->fa[i].a1[j];
    for (int j = 0; j < 16; ++j) d.A2[i][j] = wl->fa[i].A2[j];
    d.Md[i] = 0.f;
  }
  return d;
}
std::mutex g_wl_mu;         // guards g_wl_dev
float *g_wl_dev = nullptr;  // 4 + 6 + 6 + 6 floats for the B = 1 entry point

}  // namespace

template <typename T>
static int launch_reactive(umpc_batch_t *h, int nsteps, int every, void *state, const void *ref, const void *gains,
                           const void *Ib, const void *gain, void *out, void *stats, void *stream) {
  const int grid = (h->B + kBlock - 1) / kBlock;
  // velocity impulses: slice cursor + j after substep (j + 1) * nsub - 1 (umpcBatchReactive has made the range checks)
  const int nsub = h->prm.nsub;
  const T *imp = h->imptab ? (const T *)h->imptab + (size_t)h->imp_c.cursor * 6 * (size_t)h->B : nullptr;
  hipLaunchKernelGGL(umpc_reactive_kernel<T>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, make_dev_task<T>(h), h->B, nsteps, every,
                     (T)h->t_ms, (T *)state, (const T *)ref, (const T *)gains, (const T *)Ib, (const T *)gain, (T *)out,
                     (T *)stats, imp, nsub > 0 ? nsub : 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, "umpcBatchReactive");      // (the clock and the cursor stay where they were)
  h->advance((double)nsteps * h->prm.dtsim, 0, 0, imp ? nsteps / nsub : 0);
  return 0;
}

// umpcBatchReactiveRollout has made every check; the slices of the three tables are taken from the cursors here, the form of
// the kernel is chosen from where the reference comes from, and the clock and the cursors move last
template <typename T>
static int launch_reactive_steps(umpc_batch_t *h, int K, int every, void *state, const void *ref, const void *gains,
                                 const int32_t *task, const void *task_params, const void *Ib, const void *gain, void *out,
                                 void *stats, void *stream) {
  const int nsub = h->prm.nsub;
  const bool hist = h->hist_on(K, nsub), imp = h->imp_on(K, nsub);
  const size_t B = (size_t)h->B, c = (size_t)h->hist_c.cursor;
  ReactiveSteps<T> a;
  a.prm = make_dev_task<T>(h);
  a.B = h->B; a.K = K; a.nsub = nsub; a.every = every; a.t0 = (T)h->t_ms;
  a.state = (T *)state; a.ref = (const T *)ref; a.gains = (const T *)gains; a.Ib = (const T *)Ib; a.gain = (const T *)gain;
  a.out = (T *)out; a.stats = (T *)stats;
  a.task = task; a.task_params = (const T *)task_params;
  a.reftab = h->reftab ? (const T *)h->reftab + (size_t)h->ref_c.cursor * 9 * B : nullptr;
  a.imp = imp ? (const T *)h->imptab + (size_t)h->imp_c.cursor * 6 * B : nullptr;
  a.h_state = hist && h->hist_state ? (T *)h->hist_state + c * 18 * B : nullptr;
  a.h_out = hist && h->hist_out ? (T *)h->hist_out + c * 9 * B : nullptr;
  a.h_status = hist && h->hist_status ? h->hist_status + c * B : nullptr;
  a.h_info = hist && h->hist_info ? (T *)h->hist_info + c * 2 * B : nullptr;
  const dim3 grid((unsigned)((h->B + kBlock - 1) / kBlock)), block(kBlock);
  const hipStream_t s = (hipStream_t)stream;
  if (h->reftab) hipLaunchKernelGGL((umpc_reactive_steps_kernel<T, kRefTable>), grid, block, 0, s, a);
  else if (task) hipLaunchKernelGGL((umpc_reactive_steps_kernel<T, kRefRobot>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((umpc_reactive_steps_kernel<T, kRefHandle>), grid, block, 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(e, "umpcBatchReactiveRollout");      // (the clock and the cursors stay where they were)
  h->advance((double)((long long)K * nsub) * h->prm.dtsim, h->reftab ? K : 0, hist ? K : 0, imp ? K : 0);
  return 0;
}

template <typename T>
static int launch_task_table(umpc_batch_t *h, long long steps, double t_ms, const int32_t *task, const void *params,
                             const void *ref, void *tab, void *stream) {
  // enough blocks in y to fill the device when B is small, never more than the steps there are (or the grid limit)
  const unsigned gx = (unsigned)((h->B + 255) / 256);
  long long gy = (2048 + gx - 1) / gx;
  if (gy > steps) gy = steps;
  if (gy > 65535) gy = 65535;
  hipLaunchKernelGGL(umpc_task_table_kernel<T>, dim3(gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, make_dev_task<T>(h), h->B, steps,
                     (T)t_ms, task, (const T *)params, (const T *)ref, (T *)tab);
  return launch_status("umpcBatchTaskTable");
}

extern "C" {

int umpcBatchTaskTable(umpc_batch_t *h, long long steps, double t_ms, const int32_t *task, const void *params,
                       const void *ref, void *tab, void *stream) {
  if (!h || steps < 1 || !ref || !tab) return refuse("umpcBatchTaskTable", "bad argument");
  return h->dtype == UMPC_F32 ? launch_task_table<float>(h, steps, t_ms, task, params, ref, tab, stream)
                              : launch_task_table<double>(h, steps, t_ms, task, params, ref, tab, stream);
}

int umpcBatchTaskReference(umpc_batch_t *h, double t_ms, const void *ref, void *out, void *stream) {
  if (!h || !ref || !out) return refuse("umpcBatchTaskReference", "bad argument");
  if (h->reftab) return refuse("umpcBatchTaskReference", "a reference trajectory is set (its slices ARE the reference)");
  const int grid = (h->B + 255) / 256;
  if (h->dtype == UMPC_F32)
    hipLaunchKernelGGL(umpc_taskref_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, make_dev_task<float>(h), h->B,
                       (float)t_ms, (const float *)ref, (float *)out);
  else
    hipLaunchKernelGGL(umpc_taskref_kernel<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, make_dev_task<double>(h), h->B,
                       t_ms, (const double *)ref, (double *)out);
  return launch_status("umpcBatchTaskReference");
}

int umpcBatchReactive(umpc_batch_t *h, int nsteps, int every, void *state, const void *ref, const void *gains,
                      const void *Ib, const void *gain, void *out, void *stats, void *stream) {
  const char *const me = "umpcBatchReactive";
  if (!h || nsteps < 0 || every < 1 || !state || !ref) return refuse(me, "bad argument");
  if (h->reftab) return refuse(me, "a reference trajectory is set (it has one slice per MPC step, not per substep)");
  if (h->imptab) {      // (set only on handles with nsub >= 1)
    const int nsub = h->prm.nsub;
    if (nsteps % nsub != 0)
      return refuse(me, ("impulses are set (one slice per nsub = " + std::to_string(nsub) + " substeps): nsteps must be a multiple of nsub").c_str());
    if (!h->imp_c.fits(me, "impulse table", "", nsteps / nsub)) return -1;
  }
  return h->dtype == UMPC_F32 ? launch_reactive<float>(h, nsteps, every, state, ref, gains, Ib, gain, out, stats, stream)
                              : launch_reactive<double>(h, nsteps, every, state, ref, gains, Ib, gain, out, stats, stream);
}

int umpcBatchReactiveRollout(umpc_batch_t *h, int K, int every, void *state, const void *ref, const void *gains,
                             const int32_t *task, const void *task_params, const void *Ib, const void *thrust_gain, void *out,
                             void *stats, void *stream) {
  const char *const me = "umpcBatchReactiveRollout";
  if (!h) return refuse(me, "bad argument (no handle)");
  const int nsub = h->prm.nsub;
  if (K < 1 || every < 1 || !state) return refuse(me, "bad argument (K >= 1, every >= 1, state must be given)");
  if (nsub == 0) return refuse(me, "the handle has no plant (nsub = 0): there is no closed-loop step to run");
  if (nsub % every != 0)
    return refuse(me, ("every = " + std::to_string(every) + " does not divide nsub = " + std::to_string(nsub) +
                       " (a run cut into several launches must fire at the same substeps)").c_str());
  if ((long long)K * nsub > 0x7fffffffLL) return refuse(me, "K * nsub passes 2^31 - 1 substeps");
  if (!ref && !h->reftab) return refuse(me, "bad argument (ref must be given when no reference trajectory is set)");
  if (task_params && !task) return refuse(me, "task_params without task");
  if (task && h->reftab) return refuse(me, "per-robot tasks and a reference trajectory (umpcBatchSetRefTrajectory) exclude each other");
  if (h->reftab && !h->ref_c.fits(me, "reference trajectory", "K ", K)) return -1;
  if (h->hist_on(K, nsub) && !h->hist_c.fits(me, "step history", "K ", K)) return -1;
  if (h->imp_on(K, nsub) && !h->imp_c.fits(me, "impulse table", "K ", K)) return -1;
  return h->dtype == UMPC_F32
             ? launch_reactive_steps<float>(h, K, every, state, ref, gains, task, task_params, Ib, thrust_gain, out, stats, stream)
             : launch_reactive_steps<double>(h, K, every, state, ref, gains, task, task_params, Ib, thrust_gain, out, stats, stream);
}

int umpcBatchPlant(umpc_batch_t *h, int nsub, void *state, const void *u, const void *Ib, const void *gain,
                   void *stream) {
  const int grid = (h->B + kBlock - 1) / kBlock;
  if (h->dtype == UMPC_F32)
    hipLaunchKernelGGL(umpc_plant_kernel<float>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                       make_dev<float>(h->prm), h->B, nsub, (float *)state, (const float *)u, (const float *)Ib,
                       (const float *)gain);
  else
    hipLaunchKernelGGL(umpc_plant_kernel<double>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                       make_dev<double>(h->prm), h->B, nsub, (double *)state, (const double *)u, (const double *)Ib,
                       (const double *)gain);
  return launch_status("umpcBatchPlant");
}

int umpcBatchWLUpdate(const WLCon_t *wl, int B, int dtype, void *u, const void *h0, const void *pdotdes, void *w0,
                      void *stream) {
  if (!wl || B <= 0 || !u || !h0 || !pdotdes || !w0) return refuse("umpcBatchWLUpdate", "bad argument");
  const WLDev d = make_wl(wl);
  const int grid = (B + 255) / 256;
  if (dtype == UMPC_F32)
    hipLaunchKernelGGL(umpc_wl_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, d, B, (float *)u,
                       (const float *)h0, (const float *)pdotdes, (float *)w0);
  else
    hipLaunchKernelGGL(umpc_wl_kernel<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, d, B, (double *)u,
                       (const double *)h0, (const double *)pdotdes, (double *)w0);
  return launch_status("umpcBatchWLUpdate");
}

int umpcBatchSetWL(umpc_batch_t *h, const WLCon_t *wl, const double Mdiag[6], void *u4, void *w0) {
  if (!h) return -1;
  if (!wl) {
    h->wlu = h->wlw = nullptr;
    if (h->wl) { (void)hipDeviceSynchronize(); (void)hipFree(h->wl); h->wl = nullptr; }
    return 0;
  }
  if (!Mdiag || !u4 || !(Mdiag[2] > 0)) return refuse("umpcBatchSetWL", "bad argument");
  WLDev d = make_wl(wl);
  for (int i = 0; i < 6; ++i) d.Md[i] = (float)Mdiag[i];
  h->wl_md2 = d.Md[2];
  hipError_t e = hipSuccess;
  if (!h->wl) e = hipMalloc((void **)&h->wl, sizeof(WLDev));
  if (e == hipSuccess) e = hipMemcpy(h->wl, &d, sizeof(WLDev), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(e, "umpcBatchSetWL");
  h->wlu = u4; h->wlw = w0;
  return 0;
}

int umpcBatchModel(int model, int B, int dtype, int nsub, double dt, void *y, const void *u, void *aux, void *stream) {
  if ((model != UMPC_MODEL_CA6 && model != UMPC_MODEL_TSD) || B <= 0 || nsub < 0 || !y || !u || (nsub == 0 && !aux))
    return refuse("umpcBatchModel", "bad argument");
  const dim3 grid((B + 255) / 256), blk(256);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == UMPC_F32) {
    if (model == UMPC_MODEL_CA6)
      hipLaunchKernelGGL((umpc_model_kernel<float, 0>), grid, blk, 0, s, B, nsub, (float)dt, (float *)y, (const float *)u, (float *)aux);
    else
      hipLaunchKernelGGL((umpc_model_kernel<float, 1>), grid, blk, 0, s, B, nsub, (float)dt, (float *)y, (const float *)u, (float *)aux);
  } else {
    if (model == UMPC_MODEL_CA6)
      hipLaunchKernelGGL((umpc_model_kernel<double, 0>), grid, blk, 0, s, B, nsub, dt, (double *)y, (const double *)u, (double *)aux);
    else
      hipLaunchKernelGGL((umpc_model_kernel<double, 1>), grid, blk, 0, s, B, nsub, dt, (double *)y, (const double *)u, (double *)aux);
  }
  return launch_status("umpcBatchModel");
}

void wlConInit(WLCon_t *wl, const float u0[4], const float umin[4], const float umax[4], const float dumax[4],
               const float Qw[6], float controlRate, const float popts[90]) {
  // funapprox.c:102-116 + funApproxInit :35-51 (host-side unpacking; the struct carries all state)
  memset(wl, 0, sizeof(*wl));
  for (int i = 0; i < 4; ++i) {
    wl->u0[i] = u0[i]; wl->umin[i] = umin[i]; wl->umax[i] = umax[i];
    wl->dumax[i] = dumax[i] / controlRate;
  }
  for (int i = 0; i < 6; ++i) {
    const float *p = &popts[15 * i];
    wl->fa[i].k = NDELU;
    wl->fa[i].a0 = p[0];
    memcpy(wl->fa[i].a1, &p[1], 4 * sizeof(float));
    int kk = 0;
    for (int r = 0; r < 4; ++r)
      for (int c = r; c < 4; ++c) wl->fa[i].A2[r + 4 * c] = wl->fa[i].A2[c + 4 * r] = p[5 + kk++];
    wl->Qw[i + 6 * i] = Qw[i];
  }
}

void wlConUpdate(WLCon_t *wl, float u1[4], float w0[6], const float h0[6], const float pdotdes[6]) {
  std::lock_guard<std::mutex> lk(g_wl_mu);
  if (!g_wl_dev && hipMalloc((void **)&g_wl_dev, 22 * sizeof(float)) != hipSuccess) {
    fprintf(stderr, "wlConUpdate: no GPU (no CPU path exists)\n");
    return;
  }
  float hin[16];
  memcpy(hin, wl->u0, 16); memcpy(hin + 4, h0, 24); memcpy(hin + 10, pdotdes, 24);
  (void)hipMemcpy(g_wl_dev, hin, sizeof(hin), hipMemcpyHostToDevice);
  if (umpcBatchWLUpdate(wl, 1, UMPC_F32, g_wl_dev, g_wl_dev + 4, g_wl_dev + 10, g_wl_dev + 16, nullptr)) return;
  float hout[22];
  if (hipMemcpy(hout, g_wl_dev, sizeof(hout), hipMemcpyDeviceToHost) != hipSuccess) return;
  memcpy(wl->u0, hout, 16); memcpy(u1, hout, 16); memcpy(w0, hout + 16, 24);
}

namespace { WLCon_t g_wl; int g_wl_inited = 0; }
void wlconS(float u1[4], float w0[6], const float u0init[4], const float umin[4], const float umax[4],
            const float dumax[4], const float Qw[6], float controlRate, const float popts[90], const float h0[6],
            const float pdotdes[6]) {
  if (!g_wl_inited) {  // funapprox.c:172-175
    wlConInit(&g_wl, u0init, umin, umax, dumax, Qw, controlRate, popts);
    g_wl_inited = 1;
  }
  wlConUpdate(&g_wl, u1, w0, h0, pdotdes);
}

}  // extern "C"
