// Sensitivity indices of recorded rollouts (umpcBatchFactorBins / umpcBatchSensitivity / umpcBatchSensitivityIndices /
// umpcBatchScoreSensitivity, include/umpc_mi355x.h): which of the inputs the user DREW for a sweep -- initial offset and tilt,
// push size and time, a task parameter, a weight -- explains the error of a grid cell. The first-order index (correlation
// ratio) of input j is eta2_j = Var(E[y | x_j]) / Var(y), estimated from the given draws by cutting x_j into M bins of equal
// count inside the cell: eta2 = SSB / SST, the between-bin sum of squares over the total. The error terms scored here are even
// functions of a signed offset: a regression coefficient on the offset (umpc_propagator.h) is 0 where the offset explains
// everything, the correlation ratio is 1.
//
// Bin kernel (once per sweep, not hot). One block of kBinThreads per (group, factor) and one row of blocks for the robots
// outside every group. A member's rank among the members of its group with a finite value is counted: the members before it
// in the order (value, position in the member list), compared with < and == on the values, so -0 and +0 tie and the tie goes
// to the position -- numpy.argsort(kind="stable"). The values of 256 members at a time are parked in LDS (as doubles: the
// widening is exact and keeps the order, so the block has one size for both dtypes) and every thread compares its own member
// against them: n^2 comparisons per (group, factor), meant for cells of tens to thousands. bin = (rank * M) / n_f in 64-bit
// integers; -1 for a value that is not finite and for a robot outside every group. Integers only: exact.
//
// Sums kernel (the hot one). The shape, the member walk and the loader of the ensemble kernel (umpc_ensemble.h): one block per
// (group, slice of the step range), blockDim (64, kSensWaves); a wavefront owns whole rows, ONE at a time; its lanes walk
// order[offset[g] .. offset[g + 1]), lane l taking members l, l + 64, .. in that order. score_load and score_terms of
// umpc_score.h are used as they are, so a member is scored exactly when umpcBatchEnsembleQuantiles with the same out_hist
// scores it -- and all F of its bins lie in [0, M) -- and its term y has the ensemble's bits. The robot, its F bins and its
// constant reference do not depend on the step: the first trip's are fetched once, before the row loop; a later trip's robot
// travels with the trip before and its bins are fetched at the trip (a cell of up to 64 never issues them).
// Per lane and row 2 + 8 NF doubles, NF = 3 for F <= 3 and 6 above: S1 = sum y, S2 = sum y^2 and S_fm = sum y over the members
// of bin m of factor f, each accumulator a register with a static index: s_fm += (bin_f == m) ? y : +0, a compare, a select
// and an add per (f, m). A member that is not scored adds +0 everywhere. The counts are never per lane: n, skipped and every
// N_fm are popcounts of the wavefront's ballots, and a select puts N_fm into lane 8 f + m of one integer register.
// REGISTERS: 50 fp64 accumulators (NF = 6) are 100 registers, the 14 words of a step, the bins and the fold's temporaries come
// on top. One row in flight. Built for THREE WAVES PER SIMD at NF = 6 in fp32 (149 .. 158 registers of the 168 that three
// waves leave), two in fp64 (163 .. 180), and four at NF = 3 in both dtypes (100 .. 125 of 128), always with ScratchSize 0
// (resource_limits.json): a row's load latency hides behind the other waves' folds. The first trip is peeled off the member
// loop: with the next trip's bins and constant reference carried through the loop the same kernel needed 232 .. 256
// registers at NF = 6 and spilled in one form.
// Cross-lane fold: the halving tree of disp_store / lag_tree -- 32 slots per tree, one tree for NF = 3 (26 sums) and two for
// NF = 6 (50), the stages w = 32 and w = 16 by v_permlane32_swap / v_permlane16_swap, w = 8 .. 1 by __shfl_xor. After a tree
// lane l holds slot l >> 1 and the even lanes store. No LDS, no barrier, no atomics: a wavefront shares nothing.
// ORDER OF SUMMATION of a row (score.sensitivity_reference follows it operation by operation): the dispersion kernel's.
//   1. lane l starts at +0 and adds the terms of members l, l + 64, .. of the group's list in that order (+0 for a member that
//      is not scored or not in the bin, +0 in every lane without a member);
//   2. for w = 32, 16, 8, 4, 2, 1 in that order every lane l replaces its value by (value of l) + (value of l ^ w).
// A function of the group's member list and the bins alone -- not of G, the other groups, the grid, how the step range is cut
// into calls, or the run.
// CONTIGUOUS CELLS ARE THE FAST CASE, as in the ensemble kernel: scattered ids are correct and gather one word per lane.
// Measured (profiles/sensitivity_timing.txt; B = 65 536 as 1 024 cells of 64, 200 steps, fp32, reference table, e_p, F = 4,
// M = 8): 0.396 ms = 1.9 TB/s over the algorithmic bytes, 4.0x faster than the torch composition of the same 68 numbers (a
// one-hot of the bins and two batched products) and 2.09x the time of the dispersion kernel over the same window in the same
// run. The VALU sets the pace, not the loads: the same window with F = 3 (24 select-adds and one tree per row instead of 48 and
// two, the same 12 words per member) takes 0.210 ms, 1.10x the dispersion kernel -- the time follows the select-adds and the
// fold, which double together between the two forms, so which of the two weighs more is not established.
//
// Index kernel. One lane per (step, group) row of `sens`, registers only, fp64 throughout; it reads N_fm and S_fm from the row
// as it goes, so nothing is indexed in private memory. The operation order is that of score.sensitivity_indices_reference:
//   mean = S1 / n; c = S1 * S1 / n (product, division); SST = S2 - c; variance = SST / (n - 1);
//   per factor: a = +0; for m ascending over the non-empty bins a = a + S_fm * S_fm / N_fm; SSB = a - c; eta2 = SSB / SST;
//   eps2 = 1 - ((1 - eta2) * (n - 1)) / (n - M_f); F = (SSB / (M_f - 1)) / ((SST - SSB) / (n - M_f)); bin mean S_fm / N_fm.
//
// Score kernel. The same sums over one column of a per-robot score (the value rule of umpcBatchScoreQuantiles: score[num][b] or
// the IEEE double quotient score[num][b] / score[den][b], entering when row 0 > 0 and the value is finite): one wavefront per
// group, the fold and the store of the sums kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_propagator.h"
#include "umpc_quantile.h"

namespace umpc {

constexpr int kSensMaxFactors = 6, kSensMaxBins = 8;
constexpr int kSensWaves = 4;       // wavefronts per block; they share nothing
constexpr int kBinThreads = 256;
constexpr int kSensIdxBlock = 256;

// ---- bins ------------------------------------------------------------------------------------------------------------
template <typename T>
struct BinArgs {
  const T *factors;       // [F][B]
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  int32_t *bins;          // [F][B]
  int B, G, M;
};

template <typename T>
__global__ __launch_bounds__(kBinThreads) void umpc_factor_bins_kernel(const BinArgs<T> a) {
  __shared__ double tile[kBinThreads];
  const int tid = threadIdx.x, g = blockIdx.x;            // g in [0, G]: block G takes the robots outside every group
  const size_t B = (size_t)a.B;
  const T *fac = a.factors + (size_t)blockIdx.y * B;
  int32_t *out = a.bins + (size_t)blockIdx.y * B;
  const int lo = a.offset[g];
  if (g == a.G) {
    for (int i = lo + tid; i < a.B; i += kBinThreads) out[a.order[i]] = -1;
    return;
  }
  const int n = a.offset[g + 1] - lo;
  const int32_t *mem = a.order + lo;
  // (both loops run the same number of trips in every thread of the block: they hold barriers)
  for (int i0 = 0; i0 < n; i0 += kBinThreads) {
    const int i = i0 + tid;
    const bool live = i < n;
    const int b = mem[live ? i : n - 1];
    const double v = (double)fac[b];
    long long rank = 0, nf = 0;
    for (int j0 = 0; j0 < n; j0 += kBinThreads) {
      const int j = j0 + tid;
      __syncthreads();                                    // the tile of the trip before has been read
      tile[tid] = j < n ? (double)fac[mem[j]] : __builtin_nan("");
      __syncthreads();
      const int nj = n - j0 < kBinThreads ? n - j0 : kBinThreads;
      for (int k = 0; k < nj; ++k) {
        const double u = tile[k];
        const bool fin = __builtin_isfinite(u);
        nf += fin;
        rank += fin & ((u < v) | ((u == v) & (j0 + k < i)));
      }
    }
    // (a finite member counts itself in nf: nf >= 1)
    if (live) out[b] = __builtin_isfinite(v) ? (int32_t)((rank * a.M) / nf) : -1;
  }
}

// ---- sums ------------------------------------------------------------------------------------------------------------
template <typename T>
struct SensArgs {
  ScoreArgs<T> t;         // the tables as the scoring kernel reads them (score, status, tol2 unused); t.count = steps
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  const int32_t *bins;    // [F][B]
  double *sens;           // [count][G][4 + 2 F M]
  int G, F, M, term;
};

template <typename T>
struct ScoreSensArgs {
  const T *score;         // [12][B]
  const int32_t *order, *offset, *bins;
  double *sens;           // [G][4 + 2 F M]
  int B, num, den, F, M;
};

// one lane's share of one row: s[0] = S1, s[1] = S2, s[2 + 8 f + m] = S_fm
template <int NF>
struct SensAcc {
  double s[2 + 8 * NF];
  int cv;                 // lane 8 f + m: N_fm
  int cnt[2];             // scored, skipped: wave-uniform
};

template <int NF>
__device__ __forceinline__ void sens_clear(SensAcc<NF> &q) {
#pragma unroll
  for (int j = 0; j < 2 + 8 * NF; ++j) q.s[j] = 0.0;
  q.cv = 0; q.cnt[0] = 0; q.cnt[1] = 0;
}

// the F bins of robot b (the slots f >= F read factor 0 again: nothing branches around a load)
template <int NF>
__device__ __forceinline__ void sens_bins(const int32_t *bins, size_t B, int F, int b, int (&bf)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) bf[f] = bins[(size_t)(f < F ? f : 0) * B + b];
}

// `live`: this lane has a member in this trip; `fin`: its value y enters by the rule of the table it comes from. Branch-free.
template <int NF>
__device__ __forceinline__ void sens_fold(double y, bool fin, bool live, const int (&bf)[NF], int F, int M, SensAcc<NF> &q) {
  bool valid = true;
  int bb[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    valid = valid & ((f >= F) | ((unsigned)bf[f] < (unsigned)M));
    bb[f] = f < F ? bf[f] : -1;
  }
  const bool ok = live & fin & valid;
  q.cnt[0] += __popcll(__ballot(ok));
  q.cnt[1] += __popcll(__ballot(live & !ok));
  // a member that is not scored has y = +0 and adds +0 everywhere
  const double yz = ok ? y : 0.0;
  q.s[0] += yz;
  q.s[1] += ok ? y * y : 0.0;
  const int lane = threadIdx.x;
  int cv = 0;
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int m = 0; m < kSensMaxBins; ++m) {
      const bool hit = ok & (bb[f] == m);
      q.s[2 + 8 * f + m] += hit ? yz : 0.0;
      const int c = __popcll(__ballot(hit));              // (wave-uniform: a scalar, selected into its lane)
      cv = lane == 8 * f + m ? c : cv;
    }
  q.cv += cv;
}

// what slot r of the fold sums (r is a constant after unrolling); the slots past the sums fold +0
template <int NF>
__device__ __forceinline__ double sens_slot(const SensAcc<NF> &q, int r) {
  return r < 2 + 8 * NF ? q.s[r < 2 + 8 * NF ? r : 0] : 0.0;
}

// slots 32 t .. 32 t + 31 by the halving tree of lag_tree: lane l ends with slot 32 t + (l >> 1)
template <int NF, int TREE>
__device__ __forceinline__ double sens_tree(const SensAcc<NF> &q, int lane) {
  double x32[32], x16[16], x8[8], x4[4], x2[2], x1[1];
#pragma unroll
  for (int j = 0; j < 32; ++j) x32[j] = sens_slot<NF>(q, 32 * TREE + j);
  lag_halve_swap<16, 32>(x32, x16);
  lag_halve_swap<8, 16>(x16, x8);
  disp_halve<4>(x8, x4, (lane & 8) != 0, 8);
  disp_halve<2>(x4, x2, (lane & 4) != 0, 4);
  disp_halve<1>(x2, x1, (lane & 2) != 0, 2);
  return x1[0] + __shfl_xor(x1[0], 1);
}

// slot s of the fold goes to: row 2 + s for s < 2, row 4 + F M + f M + m for s = 2 + 8 f + m with f < F and m < M, nowhere else
__device__ __forceinline__ void sens_store_slot(double v, int s, bool writer, double *row, int F, int M) {
  const int f = (s - 2) >> 3, m = (s - 2) & 7;
  const bool head = s < 2, body = (s >= 2) & (f < F) & (m < M);
  const int at = head ? 2 + s : 4 + F * M + f * M + m;
  if (writer & (head | body)) row[at] = v;
}

template <int NF>
__device__ __forceinline__ void sens_store(const SensAcc<NF> &q, int lane, double *row, int F, int M) {
  const double t0 = sens_tree<NF, 0>(q, lane);
  double t1 = 0.0;
  if (NF > 3) t1 = sens_tree<NF, 1>(q, lane);
  const bool even = (lane & 1) == 0;
  sens_store_slot(t0, lane >> 1, even, row, F, M);
  if (NF > 3) sens_store_slot(t1, 32 + (lane >> 1), even, row, F, M);
  {
    const int f = lane >> 3, m = lane & 7;
    if ((lane < 8 * NF) & (f < F) & (m < M)) row[4 + f * M + m] = (double)q.cv;
  }
  if (lane < 2) row[lane] = (double)(lane == 0 ? q.cnt[0] : q.cnt[1]);
}

// one trip of one row: the lane's member b, its bins and its constant reference are in registers
template <typename T, bool TAB, bool OUT, int NF>
__device__ __forceinline__ void sens_trip(const SensArgs<T> &e, size_t B, int b, const int (&bf)[NF], const T (&rc)[6], bool live,
                                          long long i, SensAcc<NF> &q) {
  ScoreStep<T> v;
  score_load<T, false, TAB, OUT, false>(e.t, B, 0, (unsigned)b, i, rc, v);
  const ScoreTerms<T> t = score_terms(e.t.taulim, v);
  const T y = e.term == 0 ? t.ep : e.term == 1 ? t.es : t.tt;
  sens_fold<NF>((double)y, t.ok, live, bf, e.F, e.M, q);
}

template <typename T, bool TAB, bool OUT, int NF>
__global__ __launch_bounds__(64 * kSensWaves, NF > 3 ? 2 : 3) void umpc_sensitivity_kernel(const SensArgs<T> e) {
  // (blockDim = (64, kSensWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  const ScoreArgs<T> &a = e.t;
  const long long stride = (long long)gridDim.y * kSensWaves, count = a.count;
  const size_t B = (size_t)a.B;
  const int F = e.F, M = e.M, cols = 4 + 2 * F * M;
  const int32_t *mem = e.order + lo;
  // the first trip's robot, bins and constant reference are the same for every row of this wavefront (n == 0: no trip,
  // nothing is read)
  const int b_first = n > 0 ? mem[lane < n ? lane : n - 1] : 0;
  int bf_first[NF];
  T rc_first[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
#pragma unroll
  for (int f = 0; f < NF; ++f) bf_first[f] = -1;
  if (n > 0) {
    sens_bins<NF>(e.bins, B, F, b_first, bf_first);
    score_const_ref<T, TAB>(a, B, b_first, rc_first);
  }
  for (long long i = (long long)blockIdx.y * kSensWaves + wave; i < count; i += stride) {
    SensAcc<NF> q;
    sens_clear(q);
    if (n > 0) sens_trip<T, TAB, OUT, NF>(e, B, b_first, bf_first, rc_first, lane < n, i, q);
    // the later trips of a cell of more than 64: the robot travels with the words of the trip before, its bins and its
    // constant reference are fetched here
    int b = n > 64 ? mem[lane + 64 < n ? lane + 64 : n - 1] : 0;
    for (int m0 = 64; m0 < n; m0 += 64) {
      const int m = m0 + lane, mn = m + 64;
      const int b_next = mem[mn < n ? mn : n - 1];
      int bf[NF];
      T rc[6];
      sens_bins<NF>(e.bins, B, F, b, bf);
      score_const_ref<T, TAB>(a, B, b, rc);
      sens_trip<T, TAB, OUT, NF>(e, B, b, bf, rc, m < n, i, q);
      b = b_next;
    }
    sens_store<NF>(q, lane, e.sens + ((size_t)i * e.G + g) * cols, F, M);
  }
}

template <typename T, int NF>
__global__ __launch_bounds__(64) void umpc_score_sensitivity_kernel(const ScoreSensArgs<T> e) {
  const int lane = threadIdx.x, g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  const size_t B = (size_t)e.B;
  const int32_t *mem = e.order + lo;
  SensAcc<NF> q;
  sens_clear(q);
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane;
    const int b = mem[m < n ? m : n - 1];
    int bf[NF];
    sens_bins<NF>(e.bins, B, e.F, b, bf);
    bool ok;
    const double x = score_table_value(e.score, B, e.num, e.den, b, ok);
    sens_fold<NF>(x, ok & __builtin_isfinite(x), m < n, bf, e.F, e.M, q);
  }
  sens_store<NF>(q, lane, e.sens + (size_t)g * (4 + 2 * e.F * e.M), e.F, e.M);
}

// ---- indices ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSensIdxBlock) void umpc_sensitivity_indices_kernel(const double *sens, long long rows, int F, int M,
                                                                                 double *idx) {
  const long long r = (long long)blockIdx.x * kSensIdxBlock + threadIdx.x;
  if (r >= rows) return;
  const int FM = F * M;
  const double *s = sens + (size_t)r * (4 + 2 * FM);
  double *o = idx + (size_t)r * (8 + F * (4 + M));
  const double nan = __builtin_nan("");
  const double n = s[0], s1 = s[2], s2 = s[3];
  const double c = s1 * s1 / n, sst = s2 - c, n1 = n - 1.0;
  const bool few = !(n >= 2.0 * M);
  const bool bad = !(sst > 0.0) | !__builtin_isfinite(s1) | !__builtin_isfinite(s2);
  const bool none = few | bad;
  o[0] = n; o[1] = s[1];
  o[2] = few ? 1.0 : bad ? 2.0 : 0.0;
  o[3] = s1 / n; o[4] = sst / n1; o[5] = sst;
  o[6] = 0.0; o[7] = 0.0;
  for (int f = 0; f < F; ++f) {
    const double *nf = s + 4 + f * M, *sf = s + 4 + FM + f * M;
    double *of = o + 8 + f * (4 + M);
    double acc = 0.0, mf = 0.0;
    for (int m = 0; m < M; ++m) {
      const double nm = nf[m], sm = sf[m];
      const bool has = nm > 0.0;
      const double term = sm * sm / nm;
      acc = has ? acc + term : acc;
      mf = has ? mf + 1.0 : mf;
      of[4 + m] = has ? sm / nm : nan;
    }
    const double ssb = acc - c, eta = ssb / sst;
    const double eps = 1.0 - ((1.0 - eta) * n1) / (n - mf);
    const double fst = (ssb / (mf - 1.0)) / ((sst - ssb) / (n - mf));
    const bool nof = none | !(mf >= 2.0) | !(n > mf);
    of[0] = nof ? nan : eta; of[1] = nof ? nan : eps; of[2] = nof ? nan : fst;
    of[3] = mf;
  }
}

}  // namespace umpc
