// Dispersion ellipsoids of recorded rollouts (umpcBatchDispersion / umpcBatchDispersionEllipsoids / umpcBatchMahalanobis,
// include/umpc_mi355x.h): the first and second moments of the 6-vector error state z = (p - pdes, v - dpdes) of a group of
// robots (the draws of one grid cell of a sweep) at every step, the mean, covariance and position ellipsoid they give, and
// how far each robot sits from its own cell's ellipsoid over a window. Every other table of the sweep toolbox works on a
// scalar norm (e_p, e_s, the clipped moments); these keep the direction of the error and the correlation between axes.
//
// Moments kernel. The shape of the ensemble kernel (umpc_ensemble.h): one block per (group, slice of the step range),
// blockDim (64, kDispWaves); a wavefront owns whole steps, two per trip where there are two, so that the loads of both are
// issued before the first word is used; its lanes walk order[offset[g] .. offset[g + 1]), lane l taking members l, l + 64,
// .. in that order; the robot index of the next trip travels with this trip's words and the first trip's index is kept in a
// register for every step; whether a reference table exists is a template parameter and the fold is written with selects:
// nothing branches around a load. A lane past the end of the list reads the last member again and folds nothing.
// A step reads 12 words per member (48 B in fp32), each once: state rows 0..2 (p) and 12..14 (v, world frame), reference
// rows 0..2 (pdes) and 3..5 (dpdes). A member is scored when all 12 are finite. THIS IS NOT THE ENSEMBLE'S RULE: the ensemble
// reads s, out and the status and not v; this kernel reads v and dpdes and none of s, out or the status. A member can be
// scored here and skipped there, and the other way round.
// Each difference is formed in the handle's dtype with one rounding, as score_terms forms d, then widened; the products
// z_i z_j are fp64 (exact for an fp32 handle, one rounding for an fp64 one: the library is built without contraction).
// Per lane and step 27 doubles: S1[6] = sum z and S2[21] = sum z_i z_j, i <= j, row-major upper triangle. A member that is
// not scored adds +0 to all of them. The two counts are popcounts of the wavefront's ballots.
// Cross-lane fold: __shfl_xor as in ens_store, but a lane does not carry all 27 values through all six stages. The sums sit
// in 32 slots (slot = row of `mom`); at stage w = 32, 16, 8, 4, 2 a lane keeps the half of its slots its bit w selects, sends
// the other half to lane ^ w and adds what it receives: 16 + 8 + 4 + 2 + 1 exchanged doubles, and a last stage w = 1 in which
// both partners add the same two values. 32 doubles = 64 ds_bpermute_b32 per row where the full butterfly would move 27 x 6
// = 324, and the row ends up spread over the lanes as it is stored: lane l holds row l >> 1, the even lanes store 256 B.
// Chosen over parking 27 x 64 partials in LDS because it needs no LDS, no barrier and no second shape of the kernel: a
// wavefront shares nothing with the others of its block, exactly as in the ensemble kernel.
// ORDER OF SUMMATION of a (step, group) row, for the mirror to follow operation by operation (score.dispersion_reference):
//   1. lane l starts at +0 and adds the terms of members l, l + 64, l + 128, .. of the group's list in that order (+0 for a
//      member that is not scored, +0 in every lane without a member);
//   2. for w = 32, 16, 8, 4, 2, 1 in that order: every lane l replaces its value by (value of l) + (value of l ^ w).
//      (A full butterfly in that order, written for all lanes. The kernel evaluates, for each entry, only the lanes of this
//      tree that lead to the lane that stores it; IEEE addition commutes, so which partner of a pair adds does not matter.)
// It is a function of the group's member list alone -- not of G, the other groups, the grid, how the step range is cut
// into calls, or the run. No atomics, no LDS, no barrier, no temporaries: bit-reproducible.
// CONTIGUOUS CELLS ARE THE FAST CASE, as in the ensemble kernel: scattered ids are correct and gather one word per lane.
// Measured (profiles/dispersion_timing.txt; B = 65 536 as 1 024 cells of 64, 200 steps, fp32, reference table): 0.192 ms =
// 3.5 TB/s over the algorithmic bytes, 17.8x faster than the torch composition of the same 29 numbers. With the full
// butterfly over all 27 values (324 ds_bpermute_b32 per row) the same kernel took 0.709 ms: the fold, not HBM, set the pace.
//
// Ellipsoid kernel. One lane per (step, group) row of `mom`, registers only, fp64 throughout: the mean S1 / n, the
// covariance C = (S2 - S1 S1^T / n) / (n - 1) (each entry: one product, one division, one subtraction, one division), the
// eigen-decomposition of the 3 x 3 position block C_pp by cyclic Jacobi -- pairs (0, 1), (0, 2), (1, 2), kEllSweeps = 8
// sweeps whatever the data: no data-dependent exit --, eigenvalues descending with their eigenvectors as columns (the
// component of largest magnitude positive, ties to the lowest index), and the inverse of the lower Cholesky factor of C_pp.
// A pivot fails when it is <= kEllPivotTol * trace(C_pp) (or NaN): status 2, a normal outcome for a cell whose draws all
// start on one point.
//
// Mahalanobis kernel. The shape of the scoring kernel (umpc_score.h): one lane per robot, a block of 64 robots is
// kMahaSlices wavefronts, slice s takes steps s, s + 8, .. of the call, two per trip; the slices meet once in LDS and slice 0
// adds them in the fixed order 1, 2, .., 7. A step reads the robot's 6 words (p and pdes) and 10 doubles of the row of its
// own cell g = group[b] (m_p, the status, Linv): wave-uniform for contiguous cells, served from cache. d = p - pdes is
// formed in the dtype and widened, d2 = |Linv (d - m_p)|^2 in fp64, rounded once to the dtype. The LDS parking is fp64 for
// both dtypes (the widening is exact), so the block has one size: 7 x 64 x (3 doubles + 7 ints).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_score.h"

namespace umpc {

constexpr int kDispRows = 32, kEllRows = 48, kMahaRows = 12;
constexpr int kDispWaves = 4;       // wavefronts per block; they share nothing
constexpr int kDispS1 = 6, kDispS2 = 21;
constexpr int kEllSweeps = 8;       // cyclic Jacobi sweeps of the 3 x 3 block, fixed
constexpr double kEllPivotTol = 1e-12;   // a Cholesky pivot fails when it is <= kEllPivotTol * trace(C_pp)
constexpr int kMahaSlices = 8;      // wavefronts per block of 64 robots = ways a call's step range is split
constexpr int kMahaNF = 3, kMahaNI = 7;   // floating-point / integer partial values per robot and slice

// pointers as the kernel reads them: the host has moved them to the first slice of the call (state: slice first + after)
template <typename T>
struct DispArgs {
  const T *state;         // [..][18][B]
  const T *reftab;        // [..][9][B] or null
  const T *ref;           // [9][B], read when reftab is null
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  double *mom;            // [count][G][32]
  int B, count, G;
};

template <typename T>
struct DispStep {
  T p[3], v[3], rp[3], rv[3];
};

// one lane's share of one (step, group) row
struct DispAcc {
  double s1[kDispS1] = {0, 0, 0, 0, 0, 0};
  double s2[kDispS2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int cnt[2] = {0, 0};    // scored, skipped: wave-uniform
};

// rc = the six words robot b reads of a constant reference (rows 0..5); zeros, and never read, with a reference table
template <typename T, bool TAB>
__device__ __forceinline__ void disp_load(const DispArgs<T> &a, size_t B, unsigned b, long long i, const T (&rc)[6], DispStep<T> &s) {
  const T *st = a.state + (size_t)i * 18 * B;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s.p[j] = st[(size_t)j * B + b];
    s.v[j] = st[(size_t)(12 + j) * B + b];
  }
  if (TAB) {
    const T *r = a.reftab + (size_t)i * 9 * B;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s.rp[j] = r[(size_t)j * B + b];
      s.rv[j] = r[(size_t)(3 + j) * B + b];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) { s.rp[j] = rc[j]; s.rv[j] = rc[3 + j]; }
  }
}

// `live`: this lane has a member in this trip. Branch-free, as score_terms is.
template <typename T>
__device__ __forceinline__ void disp_fold(const DispStep<T> &s, bool live, DispAcc &q) {
  bool fin = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    fin = fin & __builtin_isfinite(s.p[j]) & __builtin_isfinite(s.v[j]) & __builtin_isfinite(s.rp[j]) & __builtin_isfinite(s.rv[j]);
  const bool ok = live & fin;
  q.cnt[0] += __popcll(__ballot(ok));
  q.cnt[1] += __popcll(__ballot(live & !fin));
  // the differences in the dtype, one rounding each; a member that is not scored has z = +0 and adds +0 everywhere
  double z[6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T dp = s.p[j] - s.rp[j], dv = s.v[j] - s.rv[j];
    z[j] = ok ? (double)dp : 0.0;
    z[3 + j] = ok ? (double)dv : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) q.s1[j] += z[j];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) q.s2[k++] += z[i] * z[j];
}

// one stage of the fold: the 2 H values a lane holds become H. A lane whose bit `w` is set keeps the upper half and sends the
// lower one to its partner lane ^ w, which keeps the lower half and sends the upper one; each adds what it receives to what it
// keeps. Selects on constant indices: the values stay in registers.
template <int H>
__device__ __forceinline__ void disp_halve(const double (&x)[2 * H], double (&y)[H], bool up, int w) {
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const double keep = up ? x[H + j] : x[j], send = up ? x[j] : x[H + j];
    y[j] = keep + __shfl_xor(send, w);
  }
}

// the lanes of a wavefront into one row. The 27 sums sit in slots 2..28 of 32 (slot = row of `mom`; the others hold +0). Five
// halving stages w = 32, 16, 8, 4, 2 leave lane l with the one slot l >> 1, summed over the 32 lanes that differ from l in the
// bits 1..5; the last stage w = 1 adds the two halves in both partners. 32 doubles cross lanes per row where the full
// butterfly moves 27 x 6. The even lanes store the row.
__device__ __forceinline__ void disp_store(const DispAcc &q, int lane, double *row) {
  double x32[32], x16[16], x8[8], x4[4], x2[2], x1[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) x32[j] = 0.0;
#pragma unroll
  for (int j = 0; j < kDispS1; ++j) x32[2 + j] = q.s1[j];
#pragma unroll
  for (int j = 0; j < kDispS2; ++j) x32[8 + j] = q.s2[j];
  disp_halve<16>(x32, x16, (lane & 32) != 0, 32);
  disp_halve<8>(x16, x8, (lane & 16) != 0, 16);
  disp_halve<4>(x8, x4, (lane & 8) != 0, 8);
  disp_halve<2>(x4, x2, (lane & 4) != 0, 4);
  disp_halve<1>(x2, x1, (lane & 2) != 0, 2);
  double mine = x1[0] + __shfl_xor(x1[0], 1);
  const int r = lane >> 1;
  mine = r == 0 ? (double)q.cnt[0] : r == 1 ? (double)q.cnt[1] : mine;      // (rows 29..31: sums of +0)
  if ((lane & 1) == 0) row[r] = mine;
}

// NS steps (i, i + stride, ..) of one group by one wavefront: the loads of all NS are issued before the first is used
template <typename T, bool TAB, int NS>
__device__ __forceinline__ void disp_steps(const DispArgs<T> &a, const int32_t *mem, int n, int b_first, int lane, int g, long long i,
                                           long long stride) {
  const size_t B = (size_t)a.B;
  DispAcc q[NS];
  int b = b_first;
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane, mn = m + 64;
    const int b_next = mem[mn < n ? mn : n - 1];      // the next trip's robot travels with this trip's words
    T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    if (!TAB) {
#pragma unroll
      for (int j = 0; j < 6; ++j) rc[j] = a.ref[(size_t)j * B + b];
    }
    DispStep<T> v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) disp_load<T, TAB>(a, B, (unsigned)b, i + s * stride, rc, v[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s) disp_fold(v[s], m < n, q[s]);
    b = b_next;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) disp_store(q[s], lane, a.mom + ((size_t)(i + s * stride) * a.G + g) * kDispRows);
}

template <typename T, bool TAB>
__global__ __launch_bounds__(64 * kDispWaves) void umpc_dispersion_kernel(const DispArgs<T> a) {
  // (blockDim = (64, kDispWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(a.offset, g);
  const long long stride = (long long)gridDim.y * kDispWaves, count = a.count;
  const int32_t *mem = a.order + lo;
  // the first trip's robot is the same for every step of this wavefront (n == 0: no trip, nothing is read)
  const int b_first = n > 0 ? mem[lane < n ? lane : n - 1] : 0;
  long long i = (long long)blockIdx.y * kDispWaves + wave;
  // (fp64: one step at a time, 88 VGPRs and 5 waves per SIMD. Two steps compile to 166 VGPRs and 3 waves per SIMD, still
  // without scratch: about the same bytes in flight per SIMD either way; not measured, so the smaller form stays.)
  if (sizeof(T) == 4)
    for (; i + stride < count; i += 2 * stride) disp_steps<T, TAB, 2>(a, mem, n, b_first, lane, g, i, stride);
  for (; i < count; i += stride) disp_steps<T, TAB, 1>(a, mem, n, b_first, lane, g, i, stride);
}

// ---- ellipsoids ------------------------------------------------------------------------------------------------------
// one Jacobi rotation of the symmetric 3 x 3 matrix on the pair (p, q); r is the third index: app, aqq, apq, arp, arq are
// its entries, vp and vq the columns p and q of the accumulated rotations. Written with a select: apq == 0 rotates nothing.
__device__ __forceinline__ void ell_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double (&vp)[3], double (&vq)[3]) {
  const double theta = (aqq - app) / (2.0 * apq);
  double t = __builtin_copysign(1.0, theta) / (__builtin_fabs(theta) + __dsqrt_rn(theta * theta + 1.0));
  t = apq != 0.0 ? t : 0.0;
  const double c = 1.0 / __dsqrt_rn(t * t + 1.0), s = t * c;
  app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp; arq = rq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = c * vp[k] - s * vq[k], b = s * vp[k] + c * vq[k];
    vp[k] = a; vq[k] = b;
  }
}

// eigenvalue i before eigenvalue j: the larger first
__device__ __forceinline__ void ell_order(double &li, double &lj, double (&vi)[3], double (&vj)[3]) {
  const bool sw = li < lj;
  const double a = li, b = lj;
  li = sw ? b : a; lj = sw ? a : b;
#pragma unroll
  for (int k = 0; k < 3; ++k) { const double x = vi[k], y = vj[k]; vi[k] = sw ? y : x; vj[k] = sw ? x : y; }
}

// the component of largest magnitude positive, ties to the lowest index
__device__ __forceinline__ void ell_sign(double (&v)[3]) {
  double big = v[0];
  big = __builtin_fabs(v[1]) > __builtin_fabs(big) ? v[1] : big;
  big = __builtin_fabs(v[2]) > __builtin_fabs(big) ? v[2] : big;
  const bool flip = big < 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = flip ? -v[k] : v[k];
}

__global__ __launch_bounds__(256) void umpc_dispersion_ellipsoid_kernel(const double *mom, long long rows, double *ell) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double *m = mom + (size_t)r * kDispRows;
  double *e = ell + (size_t)r * kEllRows;
  const double nan = __builtin_nan("");
  const double n = m[0];
  double s1[kDispS1], c[kDispS2];
#pragma unroll
  for (int j = 0; j < kDispS1; ++j) s1[j] = m[2 + j];
  e[0] = n; e[1] = m[1];
#pragma unroll
  for (int j = 0; j < kDispS1; ++j) e[2 + j] = s1[j] / n;
  const bool few = !(n >= 2.0);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j, ++k) {
      c[k] = (m[8 + k] - s1[i] * s1[j] / n) / (n - 1.0);
      e[8 + k] = few ? nan : c[k];
    }
  // C_pp: entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) of the upper triangle = k 0, 1, 2, 6, 7, 11
  const double c00 = c[0], c01 = c[1], c02 = c[2], c11 = c[6], c12 = c[7], c22 = c[11];
  double a00 = c00, a01 = c01, a02 = c02, a11 = c11, a12 = c12, a22 = c22;
  double v0[3] = {1, 0, 0}, v1[3] = {0, 1, 0}, v2[3] = {0, 0, 1};
  for (int sweep = 0; sweep < kEllSweeps; ++sweep) {
    ell_rotate(a00, a11, a01, a02, a12, v0, v1);     // (0, 1), third index 2
    ell_rotate(a00, a22, a02, a01, a12, v0, v2);     // (0, 2), third index 1
    ell_rotate(a11, a22, a12, a01, a02, v1, v2);     // (1, 2), third index 0
  }
  ell_order(a00, a11, v0, v1); ell_order(a11, a22, v1, v2); ell_order(a00, a11, v0, v1);
  ell_sign(v0); ell_sign(v1); ell_sign(v2);
  e[29] = few ? nan : a00; e[30] = few ? nan : a11; e[31] = few ? nan : a22;
#pragma unroll
  for (int j = 0; j < 3; ++j) {      // row j of V = [v0 v1 v2]
    e[32 + 3 * j] = few ? nan : v0[j]; e[33 + 3 * j] = few ? nan : v1[j]; e[34 + 3 * j] = few ? nan : v2[j];
  }
  // lower Cholesky factor of C_pp and its inverse; `!(pivot > floor)` also catches a NaN
  const double floor_ = kEllPivotTol * ((c00 + c11) + c22);
  const double l00 = __dsqrt_rn(c00), l10 = c01 / l00, l20 = c02 / l00;
  const double p1 = c11 - l10 * l10, l11 = __dsqrt_rn(p1), l21 = (c12 - l20 * l10) / l11;
  const double p2 = (c22 - l20 * l20) - l21 * l21, l22 = __dsqrt_rn(p2);
  const bool bad = !(c00 > floor_) | !(p1 > floor_) | !(p2 > floor_);
  const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
  const double i10 = -(l10 * i00) * i11, i21 = -(l21 * i11) * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
  e[41] = few ? 1.0 : bad ? 2.0 : 0.0;
  const bool none = few | bad;
  e[42] = none ? nan : i00; e[43] = none ? nan : i10; e[44] = none ? nan : i11;
  e[45] = none ? nan : i20; e[46] = none ? nan : i21; e[47] = none ? nan : i22;
}

// ---- Mahalanobis score -----------------------------------------------------------------------------------------------
template <typename T>
struct MahaArgs {
  const T *state;         // [..][18][B]
  const T *reftab;        // [..][9][B] or null
  const T *ref;           // [9][B], read when reftab is null
  const double *ell;      // [count][G][48]
  const int32_t *group;   // [B]
  T *msc;                 // [12][B] in/out
  int B, count, G;
  long long step0;
  T limit;
};

template <typename T>
struct MahaStep {
  T p[3], rp[3];
  double m[3], li[6], st;
};

template <typename T>
struct MahaPart {
  T sum = T(0), mx = T(0), last = T(0);
  int n = 0, nskip = 0, nover = 0, imax = -1, ilast = -1, ifirst_over = -1, ilast_over = -1;   // i = step index inside the call
};

// gc = the robot's group, moved into [0, G) for the address (a robot outside is skipped, its row 0 of the step read and unused)
template <typename T, bool TAB>
__device__ __forceinline__ void maha_load(const MahaArgs<T> &a, size_t B, size_t b, int gc, long long i, const T (&rc)[3], MahaStep<T> &s) {
  const T *st = a.state + (size_t)i * 18 * B + b;
#pragma unroll
  for (int j = 0; j < 3; ++j) s.p[j] = st[(size_t)j * B];
  if (TAB) {
    const T *r = a.reftab + (size_t)i * 9 * B + b;
#pragma unroll
    for (int j = 0; j < 3; ++j) s.rp[j] = r[(size_t)j * B];
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) s.rp[j] = rc[j];
  }
  const double *e = a.ell + ((size_t)i * a.G + gc) * kEllRows;
#pragma unroll
  for (int j = 0; j < 3; ++j) s.m[j] = e[2 + j];
  s.st = e[41];
#pragma unroll
  for (int j = 0; j < 6; ++j) s.li[j] = e[42 + j];
}

template <typename T>
__device__ __forceinline__ void maha_step(const MahaArgs<T> &a, bool gok, int i, const MahaStep<T> &s, MahaPart<T> &q) {
  bool ok = gok & (s.st == 0.0);
#pragma unroll
  for (int j = 0; j < 3; ++j) ok = ok & __builtin_isfinite(s.p[j]) & __builtin_isfinite(s.rp[j]);
  double e[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { const T d = s.p[j] - s.rp[j]; e[j] = (double)d - s.m[j]; }
  const double y0 = s.li[0] * e[0], y1 = s.li[1] * e[0] + s.li[2] * e[1], y2 = (s.li[3] * e[0] + s.li[4] * e[1]) + s.li[5] * e[2];
  const T d2 = (T)((y0 * y0 + y1 * y1) + y2 * y2);
  const bool over = ok & (d2 > a.limit);
  q.n += ok; q.nskip += !ok;
  q.sum += ok ? d2 : T(0);
  const bool better = ok & ((q.imax < 0) | (d2 > q.mx));     // steps ascend inside a wavefront: the first on a tie stays
  q.imax = better ? i : q.imax;
  q.mx = umpc_max(q.mx, ok ? d2 : T(0));
  q.last = ok ? d2 : q.last; q.ilast = ok ? i : q.ilast;
  q.nover += over;
  q.ifirst_over = (over & (q.ifirst_over < 0)) ? i : q.ifirst_over;
  q.ilast_over = over ? i : q.ilast_over;
}

template <typename T, bool TAB>
__global__ __launch_bounds__(64 * kMahaSlices) void umpc_mahalanobis_kernel(const MahaArgs<T> a) {
  __shared__ double ldsf[kMahaSlices - 1][kMahaNF][64];
  __shared__ int ldsi[kMahaSlices - 1][kMahaNI][64];
  // (blockDim = (64, kMahaSlices): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const size_t B = (size_t)a.B, b = (size_t)blockIdx.x * 64 + lane;
  const bool live = b < B;                 // (a lane past the batch loads nothing, but meets the barrier)
  MahaPart<T> q;
  if (live) {
    const int g = a.group[b];
    const bool gok = (g >= 0) & (g < a.G);
    const int gc = gok ? g : 0;
    T rc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) rc[j] = TAB ? T(0) : a.ref[(size_t)j * B + b];
    // two steps per trip: the loads of both are issued before the first is used
    int i = slice;                         // (count <= 2^31 - 1 - 2 kMahaSlices, umpcBatchMahalanobis: no sum here wraps)
    for (; i + kMahaSlices < a.count; i += 2 * kMahaSlices) {
      MahaStep<T> v0, v1;
      maha_load<T, TAB>(a, B, b, gc, i, rc, v0);
      maha_load<T, TAB>(a, B, b, gc, i + kMahaSlices, rc, v1);
      maha_step(a, gok, i, v0, q);
      maha_step(a, gok, i + kMahaSlices, v1, q);
    }
    if (i < a.count) {
      MahaStep<T> v0;
      maha_load<T, TAB>(a, B, b, gc, i, rc, v0);
      maha_step(a, gok, i, v0, q);
    }
  }
  if (slice > 0) {
    double(*f)[64] = ldsf[slice - 1];
    int(*n)[64] = ldsi[slice - 1];
    f[0][lane] = (double)q.sum; f[1][lane] = (double)q.mx; f[2][lane] = (double)q.last;
    n[0][lane] = q.n; n[1][lane] = q.nskip; n[2][lane] = q.nover; n[3][lane] = q.imax; n[4][lane] = q.ilast;
    n[5][lane] = q.ifirst_over; n[6][lane] = q.ilast_over;
  }
  __syncthreads();
  if (slice > 0 || !live) return;
  // the slices in the fixed order 0, 1, .., 7; the maximum of a tie belongs to the earlier step
#pragma unroll
  for (int s = 0; s < kMahaSlices - 1; ++s) {
    const double(*f)[64] = ldsf[s];
    const int(*n)[64] = ldsi[s];
    q.sum += (T)f[0][lane];
    const T mx = (T)f[1][lane];
    const int im = n[3][lane];
    if (im >= 0 && (q.imax < 0 || mx > q.mx || (mx == q.mx && im < q.imax))) { q.mx = mx; q.imax = im; }
    q.n += n[0][lane]; q.nskip += n[1][lane]; q.nover += n[2][lane];
    if (n[4][lane] > q.ilast) { q.ilast = n[4][lane]; q.last = (T)f[2][lane]; }
    const int fo = n[5][lane], lo = n[6][lane];
    if (fo >= 0 && (q.ifirst_over < 0 || fo < q.ifirst_over)) q.ifirst_over = fo;
    if (lo > q.ilast_over) q.ilast_over = lo;
  }
  T *sc = a.msc + b;
  sc[0] += T(q.n);
  sc[1 * B] += q.sum;
  if (q.imax >= 0) {
    const T km = T(a.step0 + q.imax), old = sc[2 * B], oldk = sc[3 * B];
    if (oldk < T(0) || q.mx > old || (q.mx == old && km < oldk)) { sc[2 * B] = q.mx; sc[3 * B] = km; }
  }
  sc[4 * B] += T(q.nover);
  if (q.ifirst_over >= 0) {
    const T kf = T(a.step0 + q.ifirst_over), kl = T(a.step0 + q.ilast_over);
    const T of = sc[5 * B];
    sc[5 * B] = of < T(0) ? kf : umpc_min(of, kf);
    sc[6 * B] = umpc_max(sc[6 * B], kl);
  }
  if (q.ilast >= 0) sc[7 * B] = q.last;
  sc[8 * B] += T(q.nskip);
}

template <typename T>
__global__ __launch_bounds__(256) void umpc_mahalanobis_init_kernel(T *msc, int B_) {
  const size_t B = (size_t)B_, b = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
#pragma unroll
  for (int r = 0; r < kMahaRows; ++r) msc[(size_t)r * B + b] = (r == 3 || r == 5 || r == 6) ? T(-1) : T(0);
}

}  // namespace umpc
