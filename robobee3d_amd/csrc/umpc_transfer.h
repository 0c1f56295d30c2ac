// Transfer estimates of recorded rollouts (umpcBatchCrossSpectrumInit / umpcBatchCrossSpectrum / umpcBatchCrossSpectrumGroups /
// umpcBatchTransfer, include/umpc_mi355x.h): per robot the projection of TWO 3-channel signals -- an input x and an output y --
// onto the K windowed cosine / sine pairs of umpc_spectrum.h in one pass; per group of robots (the draws of one grid cell) the
// auto- and cross-periodograms summed over its members; from those the H1 estimate of the transfer function from x to y, the
// coherence and the random error of the estimate per frequency. umpc_spectrum.h keeps the power of ONE signal; a single record
// has coherence 1 identically, so only the cell's draws -- independent records of the same closed loop -- can say how the loop
// maps an input onto an output, and where that statement can be trusted.
//
// Sums kernel. The spectrum kernel with six channels x0 x1 x2 y0 y1 y2: one lane per robot, robot index fastest, every load of
// a wavefront one coalesced row segment, two steps per trip with the loads of both issued before the first is used, the
// step's basis row fetched with uniform loads, the frequency tile as blockIdx.y. A step reads 6 words per robot (x from the
// reference table, y from the state: the tracking and the attitude pair) or 9 (x from the impulse table, y = p - pdes with the
// reference from its table; 6 with a constant reference, fetched once). A lane carries 14 + 12 KT fp64 accumulators (n,
// skipped, sum w v and sum w v v per channel; C_j and S_j per channel and frequency of the tile): 110 at KT = 8, 62 at KT = 4,
// the faster one at the shape of record and the one the library launches.
// Every tile folds the 14 common sums; tile 0 alone writes them. A tile that K cuts short reads frequency K - 1 again in the
// slots past it and stores nothing from them. A step enters for a robot when every word it reads for BOTH signals is finite;
// otherwise `skipped` counts it and its value is +0 in every product of both signals. Selects, no branches.
// The order of summation is the spectrum kernel's: UMPC_SPEC_SLICES = 2 wavefronts per block of 64 robots, slice s folds steps
// s, s + 2, .. in order from +0; slice 1 parks its accumulators in LDS ((14 + 12 KT) x 64 doubles: 56 320 B at KT = 8 -- two
// blocks per CU --, 31 744 B at KT = 4), slice 0 adds them and then adds the total into `xsums`: partials in the order 0, 1, then
// xsums += total. Nothing crosses robots and neither the tile size nor the number of tiles enters a sum: a robot's sums depend
// on its own columns, the basis rows and `count` alone. Every product and every sum is one IEEE fp64 operation; no atomics,
// no temporaries. On tables without a hole the y blocks of the tracking pair ARE the channel blocks of umpcBatchSpectrum(ep)
// against a zero reference.
//
// Groups kernel. One wavefront per (group, channel, tile of 8 frequencies) on the tables of umpcBatchGroupIndex: per member the
// power kernel's mean removal for x and for y, then the four products Sxx, Syy, Cxy, Qxy per frequency -- 32 accumulators a lane
// --, the member walk of umpc_spectrum_groups_kernel (lane l takes members l, l + 64, ..) and one tree of spec_tree. A row is a
// function of the group's member list alone.
//
// Rows kernel. One lane per (group, channel, frequency), registers only: the twelve rows of score.TF_*.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_spectrum.h"

namespace umpc {

constexpr int kXsChannels = 6;                       // x0 x1 x2 y0 y1 y2
constexpr int kXsCommon = 2 + 2 * kXsChannels;       // n, skipped, then (sum w v, sum w v v) per channel
// what a step reads: x and y from two tables as they are; x from the impulse table and y = p - pdes against the reference
// table; the same against a constant reference
constexpr int kXsTwoTables = 0, kXsPushTable = 1, kXsPushConst = 2;
constexpr int kXsGroupTile = 8, kXsGroupSums = 4;    // frequencies per wavefront of the groups kernel; Sxx Syy Cxy Qxy
constexpr int kTfRows = 12;

// pointers as the kernel reads them: the host has moved them to the first slice AND the first row of the call (x: slice
// ref_first, row 0 or 6 of the reference table, or slice imp_first, row 0 of the impulse table; y: slice first + after, row 0
// or 9 of the state; reftab: slice ref_first, row 0; basis: row basis_first)
template <typename T>
struct XsArgs {
  const T *x;             // [..][xstride][B]
  const T *y;             // [..][18][B]
  const T *reftab;        // [..][9][B], kXsPushTable
  const T *ref;           // [3][B] of the constant reference, kXsPushConst
  const double *basis;    // [..][1 + 2 K]
  double *sums;           // [2 + 6 (2 + 2 K)][B] in/out
  int B, count, K, xstride;
};

// col = the block's first robot, the same in every lane, i = the wavefront's step
template <typename T, int FORM>
__device__ __forceinline__ void xs_load(const XsArgs<T> &a, size_t B, size_t col, unsigned lane, long long i, const T (&rc)[3],
                                        T (&x)[3], T (&y)[3], T (&r)[3]) {
  const T *xt = a.x + ((size_t)i * a.xstride * B + col);
  const T *st = a.y + ((size_t)i * 18 * B + col);
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = xt[(size_t)c * B + lane];
#pragma unroll
  for (int c = 0; c < 3; ++c) y[c] = st[(size_t)c * B + lane];
  if (FORM == kXsPushTable) {
    const T *rt = a.reftab + ((size_t)i * 9 * B + col);
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = rt[(size_t)c * B + lane];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = rc[c];      // (zeros, never used, with two tables)
  }
}

// what one step adds to the 14 + 12 KT sums of a robot. row = the step's basis row (wave-uniform), j0 = the tile's first
// frequency. FULL: the tile lies inside K; otherwise the slots past K read frequency K - 1 again (never stored).
template <typename T, int FORM, int KT, bool FULL>
__device__ __forceinline__ void xs_step(const double *row, int j0, int K, const T (&xv)[3], const T (&yv)[3], const T (&rv)[3],
                                        double (&q)[kXsCommon + 2 * kXsChannels * KT]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    ok = ok & __builtin_isfinite(xv[c]) & __builtin_isfinite(yv[c]) & (FORM == kXsTwoTables ? true : __builtin_isfinite(rv[c]));
  q[0] = __dadd_rn(q[0], ok ? 1.0 : 0.0);
  q[1] = __dadd_rn(q[1], ok ? 0.0 : 1.0);
  const double w = row[0];
  double v[kXsChannels];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // the difference in the dtype, one rounding, then widened exactly; a step that does not enter has v = +0 in both signals
    const T d = FORM == kXsTwoTables ? yv[c] : yv[c] - rv[c];
    v[c] = ok ? (double)xv[c] : 0.0;
    v[3 + c] = ok ? (double)d : 0.0;
  }
#pragma unroll
  for (int ch = 0; ch < kXsChannels; ++ch) {
    const double t = __dmul_rn(w, v[ch]);
    q[2 + 2 * ch] = __dadd_rn(q[2 + 2 * ch], t);
    q[3 + 2 * ch] = __dadd_rn(q[3 + 2 * ch], __dmul_rn(t, v[ch]));
  }
#pragma unroll
  for (int jj = 0; jj < KT; ++jj) {
    const int j = FULL ? j0 + jj : (j0 + jj < K ? j0 + jj : K - 1);
    const double bc = row[1 + 2 * j], bs = row[2 + 2 * j];
#pragma unroll
    for (int ch = 0; ch < kXsChannels; ++ch) {
      const int at = kXsCommon + (ch * KT + jj) * 2;
      q[at] = __dadd_rn(q[at], __dmul_rn(v[ch], bc));
      q[at + 1] = __dadd_rn(q[at + 1], __dmul_rn(v[ch], bs));
    }
  }
}

// the steps slice, slice + S, .. of the call, two per trip: the loads of both are issued before the first is used
template <typename T, int FORM, int KT, bool FULL>
__device__ __forceinline__ void xs_walk(const XsArgs<T> &a, size_t B, size_t col, unsigned lane, int slice, int j0, const T (&rc)[3],
                                        double (&q)[kXsCommon + 2 * kXsChannels * KT]) {
  const int K = a.K;
  const size_t bstride = 1 + 2 * (size_t)K;
  int i = slice;                           // (count <= 2^31 - 1 - 2 kSpecSlices, umpcBatchCrossSpectrum: no sum here wraps)
  for (; i + kSpecSlices < a.count; i += 2 * kSpecSlices) {
    T x0[3], y0[3], r0[3], x1[3], y1[3], r1[3];
    xs_load<T, FORM>(a, B, col, lane, i, rc, x0, y0, r0);
    xs_load<T, FORM>(a, B, col, lane, i + kSpecSlices, rc, x1, y1, r1);
    xs_step<T, FORM, KT, FULL>(a.basis + (size_t)i * bstride, j0, K, x0, y0, r0, q);
    xs_step<T, FORM, KT, FULL>(a.basis + (size_t)(i + kSpecSlices) * bstride, j0, K, x1, y1, r1, q);
  }
  if (i < a.count) {
    T x0[3], y0[3], r0[3];
    xs_load<T, FORM>(a, B, col, lane, i, rc, x0, y0, r0);
    xs_step<T, FORM, KT, FULL>(a.basis + (size_t)i * bstride, j0, K, x0, y0, r0, q);
  }
}

// (two waves per SIMD asked for; at KT = 8 the parked sums admit two blocks per CU = one wave per SIMD, and 220 registers hold sums)
template <typename T, int FORM, int KT>
__global__ __launch_bounds__(64 * kSpecSlices, 2) void umpc_xspec_kernel(const XsArgs<T> a) {
  constexpr int NQ = kXsCommon + 2 * kXsChannels * KT;
  static_assert(KT % 4 == 0, "the final fold takes four frequencies at a time");
  __shared__ double lds[kSpecSlices - 1][NQ][64];
  // (blockDim = (64, kSpecSlices): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int tile = blockIdx.y, j0 = tile * KT, K = a.K;
  const size_t B = (size_t)a.B, col = (size_t)blockIdx.x * 64, b = col + lane;
  const bool live = b < B;                 // (a lane past the batch loads nothing, but meets the barrier)
  double q[NQ];
#pragma unroll
  for (int r = 0; r < NQ; ++r) q[r] = 0.0;
  if (live) {
    T rc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rc[c] = FORM == kXsPushConst ? a.ref[(size_t)c * B + b] : T(0);
    if (j0 + KT <= K) xs_walk<T, FORM, KT, true>(a, B, col, (unsigned)lane, slice, j0, rc, q);
    else xs_walk<T, FORM, KT, false>(a, B, col, (unsigned)lane, slice, j0, rc, q);
  }
  if (slice > 0) {
#pragma unroll
    for (int r = 0; r < NQ; ++r) lds[slice - 1][r][lane] = q[r];
  }
  __syncthreads();
  if (slice > 0 || !live) return;
  // the slices in the fixed order 0, 1, .., then the call's total into the sums, eight rows at a time: their old values are
  // requested before the fold and stored after it, as in the spectrum kernel
  double *sm = a.sums + b;
  const size_t chan = 2 + 2 * (size_t)K;       // rows per channel
  if (tile == 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {              // seven common rows at a time
      double old[kXsCommon / 2];
#pragma unroll
      for (int e = 0; e < kXsCommon / 2; ++e) {
        const int r = h * (kXsCommon / 2) + e;
        const size_t row = r < 2 ? (size_t)r : 2 + (size_t)((r - 2) >> 1) * chan + ((r - 2) & 1);
        old[e] = sm[row * B];
      }
#pragma unroll
      for (int e = 0; e < kXsCommon / 2; ++e) {
        const int r = h * (kXsCommon / 2) + e;
#pragma unroll
        for (int s = 0; s < kSpecSlices - 1; ++s) q[r] = __dadd_rn(q[r], lds[s][r][lane]);
      }
#pragma unroll
      for (int e = 0; e < kXsCommon / 2; ++e) {
        const int r = h * (kXsCommon / 2) + e;
        const size_t row = r < 2 ? (size_t)r : 2 + (size_t)((r - 2) >> 1) * chan + ((r - 2) & 1);
        sm[row * B] = __dadd_rn(old[e], q[r]);
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < kXsChannels; ++ch) {
#pragma unroll
    for (int g = 0; g < KT / 4; ++g) {
      // frequencies j0 + 4 g .. j0 + 4 g + 3 of channel ch: eight consecutive rows of `sums`, eight consecutive accumulators
      const int at = kXsCommon + ch * 2 * KT + 8 * g;
      double *rows = sm + (2 + (size_t)ch * chan + 2 + 2 * (size_t)(j0 + 4 * g)) * B;
      double old[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) old[e] = j0 + 4 * g + (e >> 1) < K ? rows[(size_t)e * B] : 0.0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
#pragma unroll
        for (int s = 0; s < kSpecSlices - 1; ++s) q[at + e] = __dadd_rn(q[at + e], lds[s][at + e][lane]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (j0 + 4 * g + (e >> 1) < K) rows[(size_t)e * B] = __dadd_rn(old[e], q[at + e]);
    }
  }
}

// ---- groups ----------------------------------------------------------------------------------------------------------
// the window's column sums travel in the launch arguments
struct XsGroupArgs {
  double wsum[1 + 2 * kSpecMaxK];
  const double *sums;     // [2 + 6 (2 + 2 K)][B]
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  double *gx;             // [G][3][2 + 4 K]
  double nrows;
  int B, K;
};

// one term of a member: (4 (a b + c d)) / W0^2, the power kernel's scaling of a periodogram
__device__ __forceinline__ double xs_term(double a, double b, double c, double d, double w02) {
  return __ddiv_rn(__dmul_rn(4.0, __dadd_rn(__dmul_rn(a, b), __dmul_rn(c, d))), w02);
}

// grid (G, 3, tiles of 8 frequencies). A slot past K reads frequency K - 1 and folds +0.
__global__ __launch_bounds__(64) void umpc_xspec_groups_kernel(const XsGroupArgs a) {
  const int lane = threadIdx.x, g = blockIdx.x, c = blockIdx.y, j0 = blockIdx.z * kXsGroupTile, K = a.K;
  const auto [lo, n] = group_window(a.offset, g);
  const size_t B = (size_t)a.B, chan = 2 + 2 * (size_t)K;
  const int32_t *mem = a.order + lo;
  const double *xs = a.sums + (2 + (size_t)c * chan) * B, *ys = a.sums + (2 + (size_t)(3 + c) * chan) * B;
  const double w0 = a.wsum[0], w02 = __dmul_rn(w0, w0);
  double q[kXsGroupSums * kXsGroupTile];
#pragma unroll
  for (int s = 0; s < kXsGroupSums * kXsGroupTile; ++s) q[s] = 0.0;
  int cnt[2] = {0, 0};
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane;
    const bool live = m < n;
    const size_t b = (size_t)mem[live ? m : n - 1];
    const double nb = a.sums[b], skipped = a.sums[B + b];
    // the same rule for all channels: no hole in the window, the sums of exactly the nrows basis rows, two steps at least
    const bool ok = live & (skipped == 0.0) & (nb == a.nrows) & (nb >= 2.0);
    cnt[0] += __popcll(__ballot(ok));
    cnt[1] += __popcll(__ballot(live & !ok));
    const double mx = __ddiv_rn(xs[b], w0), my = __ddiv_rn(ys[b], w0);
#pragma unroll
    for (int jj = 0; jj < kXsGroupTile; ++jj) {
      const bool in = j0 + jj < K;
      const int j = in ? j0 + jj : K - 1;
      const double wc = a.wsum[1 + 2 * j], ws = a.wsum[2 + 2 * j];
      const double ax = __dsub_rn(xs[(size_t)(2 + 2 * j) * B + b], __dmul_rn(mx, wc));
      const double bx = __dsub_rn(xs[(size_t)(3 + 2 * j) * B + b], __dmul_rn(mx, ws));
      const double ay = __dsub_rn(ys[(size_t)(2 + 2 * j) * B + b], __dmul_rn(my, wc));
      const double by = __dsub_rn(ys[(size_t)(3 + 2 * j) * B + b], __dmul_rn(my, ws));
      const bool use = ok & in;
      const int at = kXsGroupSums * jj;
      q[at] = __dadd_rn(q[at], use ? xs_term(ax, ax, bx, bx, w02) : 0.0);
      q[at + 1] = __dadd_rn(q[at + 1], use ? xs_term(ay, ay, by, by, w02) : 0.0);
      q[at + 2] = __dadd_rn(q[at + 2], use ? xs_term(ax, ay, bx, by, w02) : 0.0);
      // conj(X) Y with X = A - i B: the imaginary part is Bx Ay - Ax By, negative for a y that lags x
      q[at + 3] = __dadd_rn(q[at + 3], use ? xs_term(bx, ay, -ax, by, w02) : 0.0);
    }
  }
  double *row = a.gx + ((size_t)g * 3 + c) * (2 + kXsGroupSums * (size_t)K);
  const int r = lane >> 1;
  const double t = spec_tree<1, 0>(q, lane);      // lane l ends with slot l >> 1 = sum (l >> 1) & 3 of frequency j0 + (l >> 3)
  if (((lane & 1) == 0) & (j0 + (r >> 2) < K)) row[2 + kXsGroupSums * j0 + r] = t;
  if ((lane < 2) & (j0 == 0)) row[lane] = (double)(lane == 0 ? cnt[0] : cnt[1]);
}

// ---- rows ------------------------------------------------------------------------------------------------------------
// one lane per (group, channel, frequency): rows = G x 3 x K
__global__ __launch_bounds__(256) void umpc_transfer_kernel(const double *gx, long long rows, int K, double *tf) {
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  if (at >= rows) return;
  const long long gc = at / K;
  const int j = (int)(at - gc * K);
  const double *r = gx + gc * (2 + kXsGroupSums * (long long)K);
  const double n = r[0], out = r[1], nan = __builtin_nan("");
  const double sxx = r[2 + kXsGroupSums * j], syy = r[3 + kXsGroupSums * j], cxy = r[4 + kXsGroupSums * j], qxy = r[5 + kXsGroupSums * j];
  const bool finite = __builtin_isfinite(sxx) & __builtin_isfinite(syy) & __builtin_isfinite(cxy) & __builtin_isfinite(qxy);
  const bool refused = !(n >= 2.0) | !finite | !(sxx > 0.0);
  const bool noy = refused | !(syy > 0.0);
  const double m2 = __dadd_rn(__dmul_rn(cxy, cxy), __dmul_rn(qxy, qxy)), mag = __dsqrt_rn(m2);
  const double pyy = __ddiv_rn(syy, n), coh = __ddiv_rn(m2, __dmul_rn(sxx, syy)), rest = __dsub_rn(1.0, coh);
  double *o = tf + at * kTfRows;
  o[0] = refused ? 0.0 : n;
  o[1] = out;
  o[2] = refused ? nan : __ddiv_rn(sxx, n);
  o[3] = refused ? nan : pyy;
  o[4] = refused ? nan : __ddiv_rn(cxy, sxx);
  o[5] = refused ? nan : __ddiv_rn(qxy, sxx);
  o[6] = refused ? nan : __ddiv_rn(mag, sxx);
  o[7] = refused ? nan : atan2(qxy, cxy);
  o[8] = noy ? nan : coh;
  o[9] = noy ? nan : __ddiv_rn(syy, mag);
  o[10] = noy ? nan : __dsqrt_rn(__ddiv_rn(rest, __dmul_rn(__dmul_rn(2.0, n), coh)));
  o[11] = noy ? nan : __dmul_rn(pyy, rest);
}

}  // namespace umpc
