// The simulation side of a closed-loop step, without the solver: the parameter block, the task generators, the plant
// integrator and the wrench-linearisation step. One lane = one robot, SoA [rows][B] like everything else. No generated
// code: the step path (umpc_step.h) and the kernels that simulate without a QP (umpc_sim.hip) both start from here.
#pragma once
#include <hip/hip_runtime.h>

#include "umpc_scalar.h"

namespace umpc {

template <typename T>
struct DevParams {
  T dt, g, Tmax;
  T wpr, wpf, ws, wvr, wvf, wds, wthrust, wmom;
  T Ib[3];
  T dtsim, taulim;
  int maxIter, nsub, plant_mode;
  int task;       // 0: ref rows are (pdes, dpdes, sdes); 1 helix, 2 straightAcc, 3 flip, 4 perch (flight_tasks.py)
  T task_p[4];    // task parameters, see task_reference()
};

// objective weights of one robot (createMPC arguments, template_controllers.py:260); batch-constant unless
// the caller supplies a per-robot table (gain-tuning sweeps, uprightmpc2.py:272-303)
template <typename T>
struct Weights {
  T ws, wds, wpr, wpf, wvr, wvf, wthrust, wmom;
};

// Reference generators of template/flight_tasks.py:6-49, evaluated on device at the MPC fire time t (ms).
// `r` holds (initialPos, -, -) on entry for task != 0 and (pdes, dpdes, sdes) on exit.
//   1 helix(trajAmp, trajFreq[Hz], dz, useY)   :6-20     2 straightAcc(tduration, vdes)            :22-29
//   3 flip(tstart, tend)                       :31-36    4 perch(tend, trotstart, trotend, vdes)   :38-49
template <typename T>
__device__ __forceinline__ void task_reference(int task, const T (&tp)[4], T t, T (&r)[9]) {
  if (task == 0) return;
  const T ip[3] = {r[0], r[1], r[2]};
  const T twopi = T(6.283185307179586476925286766559);
  const T pi = T(3.1415926535897932384626433832795);
#pragma unroll
  for (int i = 0; i < 3; ++i) { r[3 + i] = T(0); r[6 + i] = i == 2 ? T(1) : T(0); }
  if (task == 1) {
    const T amp = tp[0], omg = twopi * tp[1] * T(1e-3);
    r[0] = ip[0] + amp * umpc_sin(omg * t);
    r[3] = amp * omg * umpc_cos(omg * t);
    if (tp[3] != T(0)) {
      r[1] = ip[1] + amp * (T(1) - umpc_cos(omg * t));
      r[4] = amp * omg * umpc_sin(omg * t);
    }
    if (amp > T(1e-3)) { r[2] = ip[2] + tp[2] * t; r[5] = tp[2]; }
  } else if (task == 2) {
    const T tdur = tp[0], vdes = tp[1];
    r[3] = t < tdur ? vdes : T(0);
    r[0] = ip[0] + vdes * umpc_min(umpc_max(t, T(0)), tdur);
  } else if (task == 3) {
    const T ph = umpc_min(umpc_max((t - tp[0]) / tp[1], T(0)), T(1));
    r[6] = -umpc_sin(ph * twopi); r[7] = T(0); r[8] = umpc_cos(ph * twopi);
  } else if (task == 4) {
    const T tend = tp[0], trotstart = tp[1], trotend = tp[2], vdes = tp[3];
    r[0] = ip[0] + vdes * umpc_min(umpc_max(t, T(0)), tend);
    r[3] = t < tend ? vdes : T(0);
    if (t < tend) {
      const T ph = umpc_min(umpc_max((t - trotend) / trotstart, T(0)), T(1));
      r[6] = -umpc_sin(ph * pi); r[7] = T(0); r[8] = umpc_cos(ph * pi);
    } else {
      r[6] = T(-1); r[7] = T(0); r[8] = T(0);
    }
  }
}

// ---------------------------------------------------------------------------
// plant: template/genqp.py:24-41 (R column-major, dq = (v_world, omega_body))
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void plant_vf(const T (&R)[9], const T (&dq)[6], const T (&u)[3],
                                         const T (&Ib)[3], const T (&Ibinv)[3], T gain, T (&ddq)[6]) {
  // the library is built with -ffp-contract=off (the QP phases place their FMAs explicitly); the plant is plain
  // arithmetic where a fused multiply-add only removes a rounding
#pragma clang fp contract(fast)
  const T wx = dq[3], wy = dq[4], wz = dq[5];
  const T Th = gain * u[0];
  ddq[0] = Th * R[6];
  ddq[1] = Th * R[7];
  ddq[2] = Th * R[8] - T(9.81e-3);
  const T hx = Ib[0] * wx, hy = Ib[1] * wy, hz = Ib[2] * wz;
  const T cx = wy * hz - wz * hy;
  const T cy = wz * hx - wx * hz;
  const T cz = wx * hy - wy * hx;
  // np.linalg.inv(Ib) @ (...), genqp.py:28: the reference multiplies by the inverse too
  ddq[3] = (-cx + u[1]) * Ibinv[0];
  ddq[4] = (-cy + u[2]) * Ibinv[1];
  ddq[5] = (-cz) * Ibinv[2];
}

// R <- R expm(skew(w) h): Rodrigues form of scipy.linalg.expm(skew(w) dt), genqp.py:39
template <typename T>
__device__ __forceinline__ void plant_rot(T (&R)[9], T w0, T w1, T w2, T h) {
  // the library is built with -ffp-contract=off (the QP phases place their FMAs explicitly); the plant is plain
  // arithmetic where a fused multiply-add only removes a rounding
#pragma clang fp contract(fast)
  const T ax = w0 * h, ay = w1 * h, az = w2 * h;
  const T t = ax * ax + ay * ay + az * az;
  T a, b;
  if (t < T(1e-2)) {
    a = T(1) - t * (T(1) / 6 - t * (T(1) / 120 - t * (T(1) / 5040 - t * (T(1) / 362880))));
    b = T(0.5) - t * (T(1) / 24 - t * (T(1) / 720 - t * (T(1) / 40320 - t * (T(1) / 3628800))));
  } else {
    const T th = umpc_sqrt(t);
    a = umpc_sin(th) / th;
    b = (T(1) - umpc_cos(th)) / t;
  }
  T e[3][3];
  e[0][0] = T(1) - b * (ay * ay + az * az);
  e[1][1] = T(1) - b * (ax * ax + az * az);
  e[2][2] = T(1) - b * (ax * ax + ay * ay);
  e[0][1] = -a * az + b * ax * ay;
  e[1][0] = a * az + b * ax * ay;
  e[0][2] = a * ay + b * ax * az;
  e[2][0] = -a * ay + b * ax * az;
  e[1][2] = -a * ax + b * ay * az;
  e[2][1] = a * ax + b * ay * az;
  T Rn[9];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) Rn[r + 3 * c] = R[r] * e[0][c] + R[r + 3] * e[1][c] + R[r + 6] * e[2][c];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rn[i];
}

template <typename T>
__device__ __forceinline__ void plant_step(T (&p)[3], T (&R)[9], T (&dq)[6], const T (&u)[3], T dt,
                                           const T (&Ib)[3], const T (&Ibinv)[3], T gain, int mode) {
  // the library is built with -ffp-contract=off (the QP phases place their FMAs explicitly); the plant is plain
  // arithmetic where a fused multiply-add only removes a rounding
#pragma clang fp contract(fast)
  if (mode == 0) {
    T ddq[6];
    plant_vf(R, dq, u, Ib, Ibinv, gain, ddq);
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = p[i] + dt * dq[i];
    plant_rot(R, dq[3], dq[4], dq[5], dt);
#pragma unroll
    for (int i = 0; i < 6; ++i) dq[i] = dq[i] + dt * ddq[i];
  } else {
    // build-defined classical RK4 on y = (p, R, dq), dR/dt = R skew(w)
    T yv0[18], ys[18], acc[18], k[18];
#pragma unroll
    for (int i = 0; i < 3; ++i) yv0[i] = p[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) yv0[3 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) yv0[12 + i] = dq[i];
    const T cs[4] = {T(0), T(0.5), T(0.5), T(1)};
    const T wt[4] = {T(1), T(2), T(2), T(1)};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < 18; ++i) ys[i] = s ? yv0[i] + cs[s] * dt * k[i] : yv0[i];
      T Rs[9], dqs[6], dd[6];
#pragma unroll
      for (int i = 0; i < 9; ++i) Rs[i] = ys[3 + i];
#pragma unroll
      for (int i = 0; i < 6; ++i) dqs[i] = ys[12 + i];
#pragma unroll
      for (int i = 0; i < 3; ++i) k[i] = dqs[i];
      const T wx = dqs[3], wy = dqs[4], wz = dqs[5];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        k[3 + r + 0] = Rs[r + 3] * wz - Rs[r + 6] * wy;
        k[3 + r + 3] = -Rs[r + 0] * wz + Rs[r + 6] * wx;
        k[3 + r + 6] = Rs[r + 0] * wy - Rs[r + 3] * wx;
      }
      plant_vf(Rs, dqs, u, Ib, Ibinv, gain, dd);
#pragma unroll
      for (int i = 0; i < 6; ++i) k[12 + i] = dd[i];
#pragma unroll
      for (int i = 0; i < 18; ++i) acc[i] = s ? acc[i] + wt[s] * k[i] : k[i];
    }
    // (k1 + 2 k2 + 2 k3 + k4) associated as in the oracle; the final dt/6 is one multiply (no per-word division)
    const T dt6 = dt / T(6);
#pragma unroll
    for (int i = 0; i < 18; ++i) ys[i] = yv0[i] + dt6 * acc[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = ys[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ys[3 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) dq[i] = ys[12 + i];
  }
}

// ---------------------------------------------------------------------------
// Wrench-linearisation step, template/uprightmpc2/funapprox.c:118-165: w0 = w(u0), A1 = dw/du(u0),
// one clipped gradient step on |A1 du + (w0 - h0 - pdotdes)|^2_Qw. Parameters are batch-constant.
// ---------------------------------------------------------------------------
struct WLDev {
  float umin[4], umax[4], dumax[4], Qw[6];
  float a0[6], a1[6][4], A2[6][16];
  float Md[6];   // M0 = diag(mb, mb, mb, ixx, iyy, izz) of dynamicsTerms (template/ca6dynamics.py:5-10, 44-50)
};

// P may live in kernarg (by value) or in global memory (wave-uniform loads): u0 is updated in place.
template <typename T>
__device__ __forceinline__ void wl_step(const WLDev &P, T (&u0)[4], const T (&h0)[6], const T (&pd)[6], T (&w0)[6]) {
  T A1[6][4], a0v[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    // funApproxF: a0 + u.a1 + 0.5 u'(A2 u), accumulated like the reference's matMult (funapprox.c:53-65)
    T dot = T(0), vout[4], quad = T(0);
#pragma unroll
    for (int l = 0; l < 4; ++l) dot += u0[l] * T(P.a1[i][l]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T acc = T(0);
#pragma unroll
      for (int l = 0; l < 4; ++l) acc += T(P.A2[i][r + 4 * l]) * u0[l];
      vout[r] = acc;
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) quad += u0[l] * vout[l];
    const T w = (T(P.a0[i]) + dot) + T(0.5) * quad;
    w0[i] = w;
    a0v[i] = w - h0[i] - pd[i];
    // funApproxDf: a1 + A2 u  (funapprox.c:67-76)
#pragma unroll
    for (int j = 0; j < 4; ++j) A1[i][j] = T(P.a1[i][j]) + vout[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    T Lb = -T(P.dumax[j]), Ub = T(P.dumax[j]);
    if (u0[j] < T(P.umin[j])) Lb = T(0);
    else if (u0[j] > T(P.umax[j])) Ub = T(0);
    T acc = T(0);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc += A1[i][j] * (T(P.Qw[i]) * a0v[i]);
    T d = T(-1e3) * acc;
    if (d < Lb) d = Lb;
    else if (d > Ub) d = Ub;
    u0[j] = u0[j] + d;
  }
}

}  // namespace umpc
