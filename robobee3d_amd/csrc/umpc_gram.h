// Trajectory modes of recorded rollouts (umpcBatchGram / umpcBatchProject, include/umpc_mi355x.h): the Gram matrix of the error
// trajectories of the draws of a cell, Gram[i][j] = sum_k sum_c y_i,c(k) y_j,c(k) with y = scale (.) (p - pdes, v - dpdes), and
// weighted sums over the draws of a cell at every step. Every other table of the sweep toolbox is a marginal -- one robot
// condensed over time, or one (step, cell) condensed over its draws; this one relates draw i to draw j as whole trajectories:
// the medoid flight, the number of ways the draws differ and the time course of each way (score.py, trajectory_modes) come
// from it. It is the project's first dense contraction and its first use of the matrix cores.
//
// Gram kernel. One block of kGramWaves = 4 wavefronts per cell, cells of up to 64 members (a larger cell is FLAGGED: rows
// 0..63 NaN). The block walks the window in stages of kGramStage = 8 steps. Staging: lane l = member slot l, wavefront w takes
// the steps w and w + 4 of the stage with the dispersion kernel's loads (disp_load: 12 words per member and step, coalesced
// for a contiguous cell) and its member rule -- scored when all 12 words are finite; each difference in the handle's dtype
// with one rounding, widened; y_c = scale[c] * z_c, one fp64 product; a (member, step) that is not scored, a slot past n and a
// step past the window give y = +0, selected BEFORE the product: a NaN never reaches an accumulator -- and writes the 6 values
// to row (step in stage) * 6 + c of the stage in LDS, 48 rows of 64 doubles at a pitch of kGramLd = 80 doubles (so that the two
// rows a 32-lane group of ds_read_b64 touches sit on different banks). The loads of the NEXT stage are issued before the
// products of this one: they fly under the MFMAs.
// Products: v_mfma_f64_16x16x4_f64 (__builtin_amdgcn_mfma_f64_16x16x4f64), D = A B + C with A [16][4], B [4][16], one double
// per lane: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15] -- for Y Y^T both are the same fragment of the stage, lane l
// reads Y[16 T + (l & 15)][4 kb + (l >> 4)] of tile row T; C / D: 4 doubles per lane, col = l & 15, row = (l >> 4) + 4 reg.
// ONLY THE 10 UPPER TILES (I <= J) of the 4 x 4 tile grid are computed, tile q = 0..9 (row by row) by wavefront q & 3: 3, 3,
// 2, 2 tiles; every wavefront runs three independent accumulators (12 doubles per lane) through a loop without a branch, the
// third of wavefronts 2 and 3 being tile 9 once more, dropped at the end. The k index runs over (step ascending, component 0..5 ascending),
// four per MFMA, 1 1/2 MFMAs per step; a tail that is no multiple of 4 is padded with rows of +0. The stored matrix is the
// upper triangle and its mirror image: symmetric bit for bit by construction (of a diagonal tile the entries col >= row).
// accumulate = 1: the old matrix is the C operand of the first MFMA, the counts and the steps add.
// CONTRACT. No atomics; a cell's table is a function of its member list, the window and the scales alone -- not of G, the other
// cells, the grid or the run: the same bits every time. The order of the four products inside one MFMA and of their sum with
// C is not documented, so the numpy mirror (score.gram_reference) cannot follow it: on data whose every difference, product
// and partial sum is exactly representable every word equals the mirror's; otherwise |gram - mirror| <= (2 N + 2) 2^-53 S_ij,
// N = 6 x (steps accumulated), S_ij = sum |y_i,c(k) y_j,c(k)| -- the dot-product bound gamma_N S for ANY order of N products
// and N - 1 additions each rounded at most once (fused multiply-adds only remove roundings), once for the kernel and once for
// the mirror. Counts and row 65 are exact. THE CALLER OF accumulate = 1 PASSES THE SAME INDEX AND SCALES AS FOR THE TABLE IT
// ADDS TO: the kernel does not check it (score.combine_grams does, on the host).
// Measured (profiles/gram_timing.txt; B = 65 536 as 1 024 contiguous cells of 64, 200 steps, fp32, reference table): Gram 0.193
// ms = 3.3 TB/s over the algorithmic bytes, 14.2x the torch composition (the operand Y [1024, 64, 1200] in fp64, then torch.bmm:
// 2.73 ms and 1.6 GB of temporaries), the time of umpcBatchDispersion over the same window (0.189 ms); projection (M = 3) 0.199
// ms. 7.55 GFLOP of fp64 MFMA issued = 39 TFLOP/s, about half of the part's fp64 matrix rate; with the loads served from cache
// the launch takes 0.186 ms: the compute side (staging, barriers, LDS reads, MFMAs), not HBM, sets the pace. Not measured: how
// that divides; the fp64 handle's form. DESIGN.md, "Trajectory modes".
//
// Projection kernel. The dispersion kernel (umpc_dispersion.h) with S1 weighted and S2 dropped: per (step, cell) the M <= 4
// weighted sums sum_b weights[m][b] z_c(b) of the six components over the scored members, 24 sums in rows 2..25 of 32. Same
// grid, same loads, same member rule; a member one of whose M weights is not finite is skipped too. Each term is one fp64
// product (no contraction); a skipped member adds (+0) * (+0). Per-lane order members l, l + 64, ..; cross-lane fold: disp_store's
// halving tree over 32 slots (disp_halve). BIT-IDENTICAL to a numpy mirror that follows that order (score.project_reference),
// for every cell size. No LDS, no scratch, no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_dispersion.h"

namespace umpc {

constexpr int kGramRows = 66, kGramCols = 64;
constexpr int kGramWaves = 4;                 // wavefronts per block = per cell
constexpr int kGramStage = 8;                 // steps staged per trip: two per wavefront
constexpr int kGramK = 6 * kGramStage;        // rows of a stage: 12 MFMAs deep
constexpr int kGramLd = 80;                   // doubles between two rows of the stage
constexpr int kGramTiles = 10;                // upper tiles of the 4 x 4 grid
constexpr int kGramHold = 3;                  // tiles a wavefront holds at the most
constexpr int kProjRows = 32, kProjMax = 4, kProjSums = 6 * kProjMax;

typedef double gram_v4 __attribute__((ext_vector_type(4)));

template <typename T>
struct GramArgs {
  DispArgs<T> t;          // the tables, the window and the index (mom is not used)
  double scale[6];
  double *gram;           // [G][66][64]
  int accumulate;
};

// y = scale (.) z of one (member, step), +0 when it is not scored; returns whether it is
template <typename T>
__device__ __forceinline__ bool gram_y(const DispStep<T> &s, bool live, const double (&scale)[6], double (&y)[6]) {
  bool fin = true;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    fin = fin & __builtin_isfinite(s.p[j]) & __builtin_isfinite(s.v[j]) & __builtin_isfinite(s.rp[j]) & __builtin_isfinite(s.rv[j]);
  const bool ok = live & fin;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T dp = s.p[j] - s.rp[j], dv = s.v[j] - s.rv[j];
    y[j] = scale[j] * (ok ? (double)dp : 0.0);
    y[3 + j] = scale[3 + j] * (ok ? (double)dv : 0.0);
  }
  return ok;
}

// word `lane` of row 65: the steps accumulated, n, the six scales, +0 (selects: the scales are not indexed by the lane)
__device__ __forceinline__ double gram_tail(int lane, double steps, int n, const double (&scale)[6]) {
  double x = lane == 0 ? steps : lane == 1 ? (double)n : 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) x = lane == 2 + c ? scale[c] : x;
  return x;
}

// a wavefront's two steps of a stage, i0 and i0 + 4: the loads are issued, nothing waits for them here. A step past the window
// reads the last step of the window again (no branch around a load; steps >= 1) and is not used: its y is selected to +0.
template <typename T, bool TAB>
__device__ __forceinline__ void gram_issue(const DispArgs<T> &t, size_t B, unsigned b, const T (&rc)[6], long long steps, long long i0,
                                           DispStep<T> (&v)[2]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const long long i = i0 + kGramWaves * u;
    disp_load<T, TAB>(t, B, b, i < steps ? i : steps - 1, rc, v[u]);
  }
}

// (four waves per SIMD asked for: one block per SIMD quarter of each of four cells at the shape of record, and a register
// budget of 128, inside the 256 architectural VGPRs -- with which the compiler keeps the MFMA accumulators in VGPRs for the
// whole loop instead of moving them to AGPRs and back around every k-block)
template <typename T, bool TAB>
__global__ __launch_bounds__(64 * kGramWaves) __attribute__((amdgpu_waves_per_eu(4))) void umpc_gram_kernel(const GramArgs<T> a) {
  __shared__ double ys[kGramK * kGramLd];
  __shared__ int cs[kGramWaves][64];
  // (blockDim = (64, kGramWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(a.t.offset, g);
  double *out = a.gram + (size_t)g * kGramRows * kGramCols;
  const long long count = a.t.count;
  if (n > kGramCols) {      // flagged, not computed: NaN matrix, no counts, row 65 as for any cell (the whole block leaves here)
    const int tid = wave * 64 + lane;
    for (int j = tid; j < 64 * kGramCols; j += 64 * kGramWaves) out[j] = __builtin_nan("");
    if (wave == 0) {
      // (the old number of steps is read by the one lane that overwrites it)
      const double old_steps = a.accumulate && lane == 0 ? out[65 * kGramCols] : 0.0;
      out[64 * kGramCols + lane] = 0.0;
      out[65 * kGramCols + lane] = gram_tail(lane, old_steps + (double)count, n, a.scale);
    }
    return;
  }
  const size_t B = (size_t)a.t.B;
  const bool live = lane < n;
  const unsigned b = n > 0 ? (unsigned)a.t.order[lo + (live ? lane : n - 1)] : 0u;      // a slot past n reads the last member and folds nothing
  const long long steps = n > 0 ? count : 0;                                            // an empty cell reads nothing
  T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  if (!TAB && n > 0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) rc[j] = a.t.ref[(size_t)j * B + b];
  }
  // tile q = wave, wave + 4, wave + 8 of the upper tiles row by row: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
  int ti[kGramHold], tj[kGramHold];
  bool has[kGramHold];
  gram_v4 acc[kGramHold];
  const int r0 = lane >> 4, c0 = lane & 15;
#pragma unroll
  for (int t = 0; t < kGramHold; ++t) {
    const int qq = wave + kGramWaves * t;
    has[t] = qq < kGramTiles;
    const int q = has[t] ? qq : kGramTiles - 1;      // (wavefronts 2 and 3 compute tile 9 once more and drop it: no branch in the loop)
    const int i = (q >= 4) + (q >= 7) + (q >= 9);
    ti[t] = i; tj[t] = i + (q - (4 * i - i * (i - 1) / 2));
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
    if (has[t] && a.accumulate) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] = out[(size_t)(16 * ti[t] + r0 + 4 * r) * kGramCols + 16 * tj[t] + c0];
    }
  }
  int cnt = 0;
  DispStep<T> v[2];
  if (steps > 0) gram_issue<T, TAB>(a.t, B, b, rc, steps, wave, v);
  for (long long s0 = 0; s0 < steps; s0 += kGramStage) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int slot = wave + kGramWaves * u;
      double y[6];
      cnt += gram_y(v[u], live & (s0 + slot < steps), a.scale, y);
#pragma unroll
      for (int c = 0; c < 6; ++c) ys[(slot * 6 + c) * kGramLd + lane] = y[c];
    }
    __syncthreads();
    if (s0 + kGramStage < steps) gram_issue<T, TAB>(a.t, B, b, rc, steps, s0 + kGramStage + wave, v);        // the next stage's loads fly under this stage's products
    const int ns = steps - s0 < kGramStage ? (int)(steps - s0) : kGramStage;
    const int nkb = (6 * ns + 3) / 4;      // (the rows of the slots past ns hold +0: the padding of the tail)
    for (int kb = 0; kb < nkb; ++kb) {
      const double *row = ys + (4 * kb + r0) * kGramLd + c0;
#pragma unroll
      for (int t = 0; t < kGramHold; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ti[t]], row[16 * tj[t]], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  cs[wave][lane] = cnt;
  __syncthreads();      // (also: every read of the old table is behind, the stores below may begin)
#pragma unroll
  for (int t = 0; t < kGramHold; ++t) {
    if (!has[t]) continue;
    const bool diag = ti[t] == tj[t];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ti[t] + r0 + 4 * r, col = 16 * tj[t] + c0;
      const double x = acc[t][r];
      if (!diag || col >= row) out[(size_t)row * kGramCols + col] = x;
      if (!diag || col > row) out[(size_t)col * kGramCols + row] = x;
    }
  }
  if (wave == 0) {
    const double scored = (double)(((cs[0][lane] + cs[1][lane]) + cs[2][lane]) + cs[3][lane]);
    const double old_scored = a.accumulate ? out[64 * kGramCols + lane] : 0.0;
    const double old_steps = a.accumulate && lane == 0 ? out[65 * kGramCols] : 0.0;      // (read by the one lane that overwrites it)
    out[64 * kGramCols + lane] = old_scored + scored;
    out[65 * kGramCols + lane] = gram_tail(lane, old_steps + (double)count, n, a.scale);
  }
}

// ---- weighted sums over the draws of a cell ----------------------------------------------------------------------------
template <typename T>
struct ProjArgs {
  DispArgs<T> t;           // the tables, the window and the index (mom is not used)
  const double *weights;   // [M][B]
  double *proj;            // [count][G][32]
  int M;
};

// one lane's share of one (step, group) row
struct ProjAcc {
  double s[kProjSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int cnt[2] = {0, 0};     // scored, skipped: wave-uniform
};

// `live`: this lane has a member in this trip; `wfin`: its M weights are finite. Branch-free, as disp_fold is.
template <typename T>
__device__ __forceinline__ void proj_fold(const DispStep<T> &s, bool live, bool wfin, const double (&w)[kProjMax], ProjAcc &q) {
  bool fin = wfin;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    fin = fin & __builtin_isfinite(s.p[j]) & __builtin_isfinite(s.v[j]) & __builtin_isfinite(s.rp[j]) & __builtin_isfinite(s.rv[j]);
  const bool ok = live & fin;
  q.cnt[0] += __popcll(__ballot(ok));
  q.cnt[1] += __popcll(__ballot(live & !fin));
  double z[6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T dp = s.p[j] - s.rp[j], dv = s.v[j] - s.rv[j];
    z[j] = ok ? (double)dp : 0.0;
    z[3 + j] = ok ? (double)dv : 0.0;
  }
#pragma unroll
  for (int m = 0; m < kProjMax; ++m) {
    const double wm = ok ? w[m] : 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) q.s[6 * m + c] += wm * z[c];
  }
}

// disp_store's tree: the 24 sums sit in slots 2..25 of 32 (slot = row of `proj`; the others hold +0)
__device__ __forceinline__ void proj_store(const ProjAcc &q, int lane, double *row) {
  double x32[32], x16[16], x8[8], x4[4], x2[2], x1[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) x32[j] = 0.0;
#pragma unroll
  for (int j = 0; j < kProjSums; ++j) x32[2 + j] = q.s[j];
  disp_halve<16>(x32, x16, (lane & 32) != 0, 32);
  disp_halve<8>(x16, x8, (lane & 16) != 0, 16);
  disp_halve<4>(x8, x4, (lane & 8) != 0, 8);
  disp_halve<2>(x4, x2, (lane & 4) != 0, 4);
  disp_halve<1>(x2, x1, (lane & 2) != 0, 2);
  double mine = x1[0] + __shfl_xor(x1[0], 1);
  const int r = lane >> 1;
  mine = r == 0 ? (double)q.cnt[0] : r == 1 ? (double)q.cnt[1] : mine;      // (rows 26..31: sums of +0)
  if ((lane & 1) == 0) row[r] = mine;
}

// NS steps (i, i + stride, ..) of one group by one wavefront, as disp_steps; the weights of a trip's member serve all NS
template <typename T, bool TAB, int NS>
__device__ __forceinline__ void proj_steps(const ProjArgs<T> &a, const int32_t *mem, int n, int b_first, int lane, int g, long long i,
                                           long long stride) {
  const size_t B = (size_t)a.t.B;
  ProjAcc q[NS];
  int b = b_first;
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane, mn = m + 64;
    const int b_next = mem[mn < n ? mn : n - 1];
    T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    if (!TAB) {
#pragma unroll
      for (int j = 0; j < 6; ++j) rc[j] = a.t.ref[(size_t)j * B + b];
    }
    double w[kProjMax];
    bool wfin = true;
#pragma unroll
    for (int k = 0; k < kProjMax; ++k) {
      w[k] = k < a.M ? a.weights[(size_t)k * B + b] : 0.0;
      wfin = wfin & __builtin_isfinite(w[k]);
    }
    DispStep<T> v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) disp_load<T, TAB>(a.t, B, (unsigned)b, i + s * stride, rc, v[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s) proj_fold(v[s], m < n, wfin, w, q[s]);
    b = b_next;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) proj_store(q[s], lane, a.proj + ((size_t)(i + s * stride) * a.t.G + g) * kProjRows);
}

template <typename T, bool TAB>
__global__ __launch_bounds__(64 * kDispWaves) void umpc_project_kernel(const ProjArgs<T> a) {
  // (blockDim = (64, kDispWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(a.t.offset, g);
  const long long stride = (long long)gridDim.y * kDispWaves, count = a.t.count;
  const int32_t *mem = a.t.order + lo;
  const int b_first = n > 0 ? mem[lane < n ? lane : n - 1] : 0;
  long long i = (long long)blockIdx.y * kDispWaves + wave;
  if (sizeof(T) == 4)
    for (; i + stride < count; i += 2 * stride) proj_steps<T, TAB, 2>(a, mem, n, b_first, lane, g, i, stride);
  for (; i < count; i += stride) proj_steps<T, TAB, 1>(a, mem, n, b_first, lane, g, i, stride);
}

}  // namespace umpc
