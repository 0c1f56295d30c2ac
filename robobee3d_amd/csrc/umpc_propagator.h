// Error propagators of recorded rollouts (umpcBatchLagMoments / umpcBatchPropagators, include/umpc_mi355x.h): the cross
// moments of the error state z = (p - pdes, v - dpdes) of a group of robots between step k (a) and step k + L (b), and the
// affine map z_b ~ Phi z_a + c they determine. umpc_dispersion.h looks at one step at a time; the sums sum z_b z_a^T are the
// one second moment its kernel cannot give.
//
// Lag-moments kernel. The shape, the member walk and the load helper of the dispersion kernel: one block per (group, slice of
// the step range), blockDim (64, kLagWaves); a wavefront owns whole rows, ONE at a time; its lanes walk
// order[offset[g] .. offset[g + 1]), lane l taking members l, l + 64, .. in that order; the next trip's robot index travels
// with this trip's words; reference table or constant is a template parameter; nothing branches around a load.
// A row reads 24 words per member, each once: the 12 of disp_load at slice i and the 12 at slice i + lag, every one a
// coalesced row segment for contiguous cells. (A wavefront that owned consecutive rows could keep z_b of row i as z_a of row
// i + lag and read 12; not done: the rows of a wavefront are `stride` apart so that the slices of a call cut the range evenly,
// and the fold below, not the loads, is what a row costs.)
// A member is scored when all 24 words are finite -- disp_fold's rule on both slices; the differences are formed in the
// handle's dtype with one rounding each and widened, every product and sum is fp64 (the library is built without
// contraction). A member that is not scored adds +0 everywhere. Per lane and row 90 doubles: S1a[6], S1b[6], S2a[21], S2b[21]
// (upper triangles, row by row) and Sba[36] = sum z_b,i z_a,j.
// REGISTERS: 90 fp64 accumulators are 180 registers and the 24 words, the robot indices and the fold's temporaries come on
// top: more than the 128 that four waves per SIMD leave and close to the 256 of two. On gfx950 the VGPR and AGPR files are one
// budget of 512 per SIMD lane, so the kernel is built for TWO WAVES PER SIMD (256 each: the block is four wavefronts, one per
// SIMD, and two blocks share a CU) rather than one with two rows in flight (2 x 180 accumulators do not fit 512 with the
// words of both), and rather than more waves with accumulators in scratch: ScratchSize is 0 for every form
// (resource_limits.json). Two waves per SIMD is what hides a row's load latency behind the other wave's fold.
// Cross-lane fold: the 96 rows of `xmom` are three groups of 32 slots, each folded by the halving tree of disp_store
// (umpc_dispersion.h): 3 x 32 doubles cross lanes per row where a full butterfly would move 90 x 6; after tree t lane l holds
// row 32 t + (l >> 1) and the even lanes store 256 B. The stages w = 32 and w = 16, three quarters of the exchanged doubles, are
// v_permlane32_swap / v_permlane16_swap (lag_swap_add: VALU, no select); w = 8 .. 1 are disp_halve's __shfl_xor. With all six
// stages on __shfl_xor the same kernel took 0.567 ms at the shape of record. No LDS, no barrier: a wavefront shares nothing with
// the others.
// ORDER OF SUMMATION of a row (score.lag_moments_reference follows it operation by operation): the dispersion kernel's.
//   1. lane l starts at +0 and adds the terms of members l, l + 64, .. of the group's list in that order (+0 for a member
//      that is not scored, +0 in every lane without a member);
//   2. for w = 32, 16, 8, 4, 2, 1 in that order every lane l replaces its value by (value of l) + (value of l ^ w).
// A function of the group's member list and the lag alone -- not of G, the other groups, the grid, how the step range is cut
// into calls, or the run. Where no member is skipped, S1a, S2a (S1b, S2b) are the bits of the dispersion kernel's row of step
// k (k + L): same terms, same order.
// CONTIGUOUS CELLS ARE THE FAST CASE, as in the dispersion kernel: scattered ids are correct and gather one word per lane.
// Measured (profiles/propagator_timing.txt; B = 65 536 as 1 024 cells of 64, 200 steps, lag 1, fp32, reference table): 0.419 ms
// = 3.4 TB/s over the algorithmic bytes, 18.6x faster than the torch composition of the same 92 numbers and 2.03x the time of
// the dispersion kernel over the same window in the same run, for twice the words and three times the folded doubles.
//
// Propagator kernel. One lane per (step, group) row of `xmom`, registers only, fp64 throughout, in the shape of
// umpc_dispersion_ellipsoid_kernel. The operation order is that of score.propagator_reference:
//   m_a = S1a / n, m_b = S1b / n; every covariance entry (S - S1_i S1_j / n) / (n - 1): one product, one division, one
//   subtraction, one division;
//   C_a = L L^T row by row: s = C_a[j][j], s -= L[j][k]^2 for k = 0 .. j - 1, pivot_j = s, L[j][j] = sqrt(s);
//     L[i][j] = (C_a[i][j] - sum_k L[i][k] L[j][k]) / L[j][j], the subtractions in the order k = 0 .. j - 1;
//   Y = L^-1 C_ba^T column by column (forward substitution, k ascending); W = L^-1 Y^T likewise; growth = sum W^2 / 6 summed
//   row by row; X = L^-T Y (back substitution, k = i + 1 .. 5 ascending), Phi = X^T;
//   c_i = m_b,i - sum_j Phi[i][j] m_a,j and Q[i][j] = C_b[i][j] - sum_k Phi[i][k] C_ba[j][k], each as s -= product, in order.
// A pivot fails when it is <= kPropPivotTol * C_a[j][j] (or NaN): relative to its own diagonal entry, so unit-free.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_dispersion.h"

namespace umpc {

constexpr int kXmomRows = 96, kPropRows = 80;
constexpr int kLagWaves = 4;        // wavefronts per block; they share nothing
constexpr int kLagSba = 36;
constexpr double kPropPivotTol = 1e-10;   // a Cholesky pivot of C_a fails when it is <= kPropPivotTol * C_a[j][j]
constexpr int kPropBlock = 256;

// the tables of DispArgs (t.mom = xmom [count][G][96]) and the lag; the tables hold t.count + lag slices
template <typename T>
struct LagArgs {
  DispArgs<T> t;
  int lag;
};

// one lane's share of one (step, group) row
struct LagAcc {
  double s1a[kDispS1] = {0, 0, 0, 0, 0, 0}, s1b[kDispS1] = {0, 0, 0, 0, 0, 0};
  double s2a[kDispS2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double s2b[kDispS2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double sba[kLagSba] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int cnt[2] = {0, 0};    // scored, skipped: wave-uniform
};

template <typename T>
__device__ __forceinline__ bool lag_finite(const DispStep<T> &s) {
  bool fin = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    fin = fin & __builtin_isfinite(s.p[j]) & __builtin_isfinite(s.v[j]) & __builtin_isfinite(s.rp[j]) & __builtin_isfinite(s.rv[j]);
  return fin;
}

// `live`: this lane has a member in this trip. Branch-free; the rule and the roundings of disp_fold on both slices.
template <typename T>
__device__ __forceinline__ void lag_fold(const DispStep<T> &sa, const DispStep<T> &sb, bool live, LagAcc &q) {
  const bool fin = lag_finite(sa) & lag_finite(sb);
  const bool ok = live & fin;
  q.cnt[0] += __popcll(__ballot(ok));
  q.cnt[1] += __popcll(__ballot(live & !fin));
  double za[6], zb[6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T dpa = sa.p[j] - sa.rp[j], dva = sa.v[j] - sa.rv[j], dpb = sb.p[j] - sb.rp[j], dvb = sb.v[j] - sb.rv[j];
    za[j] = ok ? (double)dpa : 0.0;
    za[3 + j] = ok ? (double)dva : 0.0;
    zb[j] = ok ? (double)dpb : 0.0;
    zb[3 + j] = ok ? (double)dvb : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) { q.s1a[j] += za[j]; q.s1b[j] += zb[j]; }
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j, ++k) { q.s2a[k] += za[i] * za[j]; q.s2b[k] += zb[i] * zb[j]; }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) q.sba[6 * i + j] += zb[i] * za[j];
}

// what row r of `xmom` sums (r is a constant after unrolling); the count rows and rows 92..95 fold +0
__device__ __forceinline__ double lag_slot(const LagAcc &q, int r) {
  return r < 2 ? 0.0 : r < 8 ? q.s1a[r - 2] : r < 14 ? q.s1b[r - 8] : r < 35 ? q.s2a[r - 14] : r < 56 ? q.s2b[r - 35]
       : r < 92 ? q.sba[r - 56] : 0.0;
}

// disp_halve for w = 32 and w = 16 without ds_bpermute and without selects: v_permlane32_swap / v_permlane16_swap (gfx950) swap
// the odd rows of 32 / 16 lanes of one register with the even rows of another. With a = x[j] (what the lanes without bit w keep
// and the lanes with it send) and b = x[H + j] (the other way round), after the swap the first register holds a of the lane itself
// where bit w is clear and b of the partner where it is set, the second a of the partner where it is clear and b of the lane
// itself where it is set: their sum is keep + received in every lane, the same IEEE addition as disp_halve's.
template <int W>
__device__ __forceinline__ double lag_swap_add(double a, double b) {
  const unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
  const unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
  const auto lo = W == 32 ? __builtin_amdgcn_permlane32_swap(alo, blo, false, false) : __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
  const auto hi = W == 32 ? __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false) : __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
template <int H, int W>
__device__ __forceinline__ void lag_halve_swap(const double (&x)[2 * H], double (&y)[H]) {
#pragma unroll
  for (int j = 0; j < H; ++j) y[j] = lag_swap_add<W>(x[j], x[H + j]);
}

// rows 32 t .. 32 t + 31 by the halving tree of disp_store: lane l ends with row 32 t + (l >> 1)
template <int TREE>
__device__ __forceinline__ double lag_tree(const LagAcc &q, int lane) {
  double x32[32], x16[16], x8[8], x4[4], x2[2], x1[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) x32[j] = lag_slot(q, 32 * TREE + j);
  lag_halve_swap<16, 32>(x32, x16);
  lag_halve_swap<8, 16>(x16, x8);
  disp_halve<4>(x8, x4, (lane & 8) != 0, 8);
  disp_halve<2>(x4, x2, (lane & 4) != 0, 4);
  disp_halve<1>(x2, x1, (lane & 2) != 0, 2);
  return x1[0] + __shfl_xor(x1[0], 1);
}

__device__ __forceinline__ void lag_store(const LagAcc &q, int lane, double *row) {
  const int r = lane >> 1;
  double t0 = lag_tree<0>(q, lane);
  t0 = r == 0 ? (double)q.cnt[0] : r == 1 ? (double)q.cnt[1] : t0;
  const double t1 = lag_tree<1>(q, lane), t2 = lag_tree<2>(q, lane);
  if ((lane & 1) == 0) { row[r] = t0; row[32 + r] = t1; row[64 + r] = t2; }
}

template <typename T, bool TAB>
__global__ __launch_bounds__(64 * kLagWaves) void umpc_lagmom_kernel(const LagArgs<T> a) {
  // (blockDim = (64, kLagWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(a.t.offset, g);
  const long long stride = (long long)gridDim.y * kLagWaves, count = a.t.count, lag = a.lag;
  const size_t B = (size_t)a.t.B;
  const int32_t *mem = a.t.order + lo;
  // the first trip's robot is the same for every row of this wavefront (n == 0: no trip, nothing is read)
  const int b_first = n > 0 ? mem[lane < n ? lane : n - 1] : 0;
  for (long long i = (long long)blockIdx.y * kLagWaves + wave; i < count; i += stride) {
    LagAcc q;
    int b = b_first;
    for (int m0 = 0; m0 < n; m0 += 64) {
      const int m = m0 + lane, mn = m + 64;
      const int b_next = mem[mn < n ? mn : n - 1];      // the next trip's robot travels with this trip's words
      T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
      if (!TAB) {
#pragma unroll
        for (int j = 0; j < 6; ++j) rc[j] = a.t.ref[(size_t)j * B + b];
      }
      DispStep<T> sa, sb;
      disp_load<T, TAB>(a.t, B, (unsigned)b, i, rc, sa);
      disp_load<T, TAB>(a.t, B, (unsigned)b, i + lag, rc, sb);
      lag_fold(sa, sb, m < n, q);
      b = b_next;
    }
    lag_store(q, lane, a.t.mom + ((size_t)i * a.t.G + g) * kXmomRows);
  }
}

// ---- propagators -----------------------------------------------------------------------------------------------------
// entry k of an upper triangle stored row by row (DISP_PAIRS), for i <= j
__device__ __forceinline__ constexpr int prop_pair(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

__global__ __launch_bounds__(kPropBlock) void umpc_propagator_kernel(const double *xmom, long long rows, double *prop) {
  const long long r = (long long)blockIdx.x * kPropBlock + threadIdx.x;
  if (r >= rows) return;
  const double *m = xmom + (size_t)r * kXmomRows;
  double *o = prop + (size_t)r * kPropRows;
  const double nan = __builtin_nan("");
  const double n = m[0], n1 = n - 1.0;
  const bool few = !(n >= 8.0);
  double s1a[6], s1b[6], ma[6], mb[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) { s1a[j] = m[2 + j]; s1b[j] = m[8 + j]; ma[j] = s1a[j] / n; mb[j] = s1b[j] / n; }
  double ca[kDispS2], cba[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) ca[prop_pair(i, j)] = (m[14 + prop_pair(i, j)] - s1a[i] * s1a[j] / n) / n1;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) cba[i][j] = (m[56 + 6 * i + j] - s1b[i] * s1a[j] / n) / n1;
  // C_a = L L^T, row by row; `!(pivot > floor)` also catches a NaN
  double l[6][6];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = ca[prop_pair(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - l[j][k] * l[j][k];
    bad = bad | !(s > kPropPivotTol * ca[prop_pair(j, j)]);
    l[j][j] = __dsqrt_rn(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = ca[prop_pair(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) t = t - l[i][k] * l[j][k];
      l[i][j] = t / l[j][j];
    }
  }
  const bool none = few | bad;
  // Y = L^-1 C_ba^T: column c solves L y = row c of C_ba
  double y[6][6];
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = cba[c][i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - l[i][k] * y[k][c];
      y[i][c] = s / l[i][i];
    }
  // W = L^-1 Y^T (= L^-1 Phi L): column c solves L w = row c of Y; growth = |W|_F^2 / 6, summed row by row
  double growth;
  {
    double w[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s = y[c][i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - l[i][k] * w[k][c];
        w[i][c] = s / l[i][i];
      }
    double gsum = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int c = 0; c < 6; ++c) gsum = gsum + w[i][c] * w[i][c];
    growth = gsum / 6.0;
  }
  // X = L^-T Y in place of Y (back substitution); Phi = X^T: phi[c][i] = x[i][c]
#pragma unroll
  for (int c = 0; c < 6; ++c)
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double s = y[i][c];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) s = s - l[k][i] * y[k][c];
      y[i][c] = s / l[i][i];
    }
  o[0] = n; o[1] = m[1];
  o[2] = few ? 1.0 : bad ? 2.0 : 0.0;
  o[5] = none ? nan : growth;
  o[6] = 0.0; o[7] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) o[8 + 6 * i + j] = none ? nan : y[j][i];
    double s = mb[i];
#pragma unroll
    for (int j = 0; j < 6; ++j) s = s - y[j][i] * ma[j];
    o[44 + i] = none ? nan : s;
  }
  // Q = C_b - Phi C_ba^T, upper triangle; the traces of the position and velocity blocks of Q and of C_b on the way
  double qd[6], cbd[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      const double cb = (m[35 + prop_pair(i, j)] - s1b[i] * s1b[j] / n) / n1;
      double s = cb;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = s - y[k][i] * cba[j][k];
      o[50 + prop_pair(i, j)] = none ? nan : s;
      if (i == j) { qd[i] = s; cbd[i] = cb; }
    }
  const double dp = (cbd[0] + cbd[1]) + cbd[2], dv = (cbd[3] + cbd[4]) + cbd[5];
  const double r2p = 1.0 - ((qd[0] + qd[1]) + qd[2]) / dp, r2v = 1.0 - ((qd[3] + qd[4]) + qd[5]) / dv;
  o[3] = none ? nan : dp == 0.0 ? nan : r2p;
  o[4] = none ? nan : dv == 0.0 ? nan : r2v;
#pragma unroll
  for (int j = 71; j < kPropRows; ++j) o[j] = 0.0;
}

}  // namespace umpc
