// Ensemble curves of recorded rollouts (umpcBatchGroupIndex / umpcBatchEnsemble, include/umpc_mi355x.h): the statistics of
// a group of robots (the draws of one grid cell of a sweep) at every step -- the transpose of the scoring kernel's
// reduction (umpc_score.h), over the same 15 words (60 B in fp32) per robot-step. A score has summed over the steps and
// keeps the robots apart; a row of `ens` has reduced over the robots of a cell and keeps the steps apart: mean, spread and
// envelope of the tracking error over time, the share of draws outside the tube after a push.
//
// Ensemble kernel. One block per (group, slice of the step range), blockDim (64, kEnsWaves). A wavefront owns whole steps:
// wavefront w of slice y takes steps y * kEnsWaves + w, + gridDim.y * kEnsWaves, .., two per trip, so that the loads of
// both are issued before the first word is used (30 per lane in flight with every record, as in the scoring kernel, whose
// loader score_load and per-robot-step expressions score_terms are used as they are: the terms are formed in the dtype and
// then widened). The wavefront's lanes walk the group's member list order[offset[g] .. offset[g + 1]): lane l takes members
// l, l + 64, .. in that order. The robot index of the next trip is fetched with the table words of this one, and the first
// trip's index is kept in a register for every step, so no table load waits for an index. Which tables there are is a
// template parameter and the fold is written with selects: nothing branches around a load. A lane past the end of the
// list reads the last member again (a valid address, an L1 hit) and folds nothing.
// Everything that crosses robots is fp64. Per step a lane holds 11 doubles (seven sums, three maxima, one minimum:
// EnsAcc) and the index of its largest e_p; the four counts are never per lane: they are popcounts of the wavefront's
// ballots. After the last trip the lanes meet in a butterfly (__shfl_xor 1, 2, 4, .., 32: both partners of a stage add the
// same two values, IEEE addition commutes, so all 64 lanes end with the same bits), then lanes 0..15 store one row of 128 B.
// Order of summation of a (step, group) row: lane l folds its members in list order, then the fixed butterfly over the 64
// lanes. It is a function of the group's member list alone -- not of G, the other groups, the grid, how the step range
// is cut into calls, or the run. No atomics, no LDS, no barrier, no temporaries.
// CONTIGUOUS CELLS ARE THE FAST CASE. A cell of 64 consecutive robots (cell = b // 64) makes every load of
// a wavefront one coalesced 256-B segment per word, as in the scoring kernel. Scattered ids are correct but every lane
// then gathers its word from another row segment: the hardware notes put 64 lanes in 64 different rows at about 17x slower
// per instruction. There is no second path for scattered ids: lay the sweep out with its cells contiguous.
// Measured (profiles/ensemble_timing.txt; B = 65 536 as 1 024 cells of 64, 200 steps, fp32, every record): 0.304 ms = 2.7 TB/s
// over the algorithmic bytes, 7.2x faster than the torch composition of the same rows, 1.69x the scoring kernel's time on the
// same tables: the butterfly (about 140 ds_bpermute_b32 per row of 3.8 KB) runs once per step also for n <= 64.
//
// Group-index kernel. One wavefront per group (and one for the ignored tail, key G) scans group[] twice, 256 ids per trip:
// first it counts the robots with a smaller key -- its offset --, then it writes its own robots at offset + rank, the rank
// from the ballot of the trip and a running count: ascending robot index by construction. Integers only; (G + 1) x 2 B id
// reads, served by L2 after the first group, once per sweep.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "umpc_score.h"

namespace umpc {

constexpr int kEnsRows = 16;
constexpr int kEnsWaves = 4;        // wavefronts per block; they share nothing
constexpr int kEnsInts = 4;         // ballot counts: scored, skipped, outside the tube, not solved

template <typename T>
struct EnsArgs {
  ScoreArgs<T> t;         // the tables as the scoring kernel reads them (score unused); t.count = steps of the call
  const int32_t *order;   // [B]
  const int32_t *offset;  // [G + 1]
  double *ens;            // [count][G][16]
  int G;
};

// one lane's share of one (step, group) row
struct EnsAcc {
  double sum_ep = 0, sum_ep2 = 0, max_ep = 0, min_ep = __builtin_inf(), sum_es = 0, max_es = 0, sum_tau = 0, max_tau = 0;
  double sd[3] = {0, 0, 0};
  int arg = -1;           // robot of max_ep among this lane's scored members (ties: lowest index), -1: none scored
  int cnt[kEnsInts] = {0, 0, 0, 0};   // wave-uniform
};

// `live`: this lane has a member in this trip (b its robot)
template <typename T>
__device__ __forceinline__ void ens_fold(const ScoreArgs<T> &a, const ScoreStep<T> &v, bool live, int b, EnsAcc &q) {
  const ScoreTerms<T> t = score_terms(a.taulim, v);
  const bool ok = live & t.ok;
  const double ep = (double)t.ep, es = (double)t.es, tt = (double)t.tt;
  q.cnt[0] += __popcll(__ballot(ok));
  q.cnt[1] += __popcll(__ballot(live & !t.ok));
  q.cnt[2] += __popcll(__ballot(ok & (t.ep > a.tol2)));
  q.cnt[3] += __popcll(__ballot(ok & (v.st != 1)));
  // a member that is not scored adds +0 to the sums and takes no part in a maximum of non-negative terms or in the minimum
  q.sum_ep += ok ? ep : 0.0; q.sum_ep2 += ok ? ep * ep : 0.0;
  const bool better = ok & ((q.arg < 0) | (ep > q.max_ep) | ((ep == q.max_ep) & (b < q.arg)));
  q.arg = better ? b : q.arg;
  q.max_ep = umpc_max(q.max_ep, ok ? ep : 0.0); q.min_ep = ok ? umpc_min(q.min_ep, ep) : q.min_ep;
  q.sum_es += ok ? es : 0.0; q.max_es = umpc_max(q.max_es, ok ? es : 0.0);
  q.sum_tau += ok ? tt : 0.0; q.max_tau = umpc_max(q.max_tau, ok ? tt : 0.0);
#pragma unroll
  for (int j = 0; j < 3; ++j) q.sd[j] += ok ? (double)t.d[j] : 0.0;
}

// the lanes of a wavefront into one row: every lane ends with the same values; lanes 0..15 store them
template <bool OUT, bool STAT>
__device__ __forceinline__ void ens_store(EnsAcc &q, int lane, double *row) {
  const double own_max = q.max_ep;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) {
    q.sum_ep += __shfl_xor(q.sum_ep, w); q.sum_ep2 += __shfl_xor(q.sum_ep2, w);
    q.max_ep = umpc_max(q.max_ep, __shfl_xor(q.max_ep, w)); q.min_ep = umpc_min(q.min_ep, __shfl_xor(q.min_ep, w));
    q.sum_es += __shfl_xor(q.sum_es, w); q.max_es = umpc_max(q.max_es, __shfl_xor(q.max_es, w));
    if (OUT) { q.sum_tau += __shfl_xor(q.sum_tau, w); q.max_tau = umpc_max(q.max_tau, __shfl_xor(q.max_tau, w)); }
#pragma unroll
    for (int j = 0; j < 3; ++j) q.sd[j] += __shfl_xor(q.sd[j], w);
  }
  // the lanes whose own maximum is the row's: the lowest robot index among them
  int arg = ((q.arg >= 0) & (own_max == q.max_ep)) ? q.arg : 0x7fffffff;
#pragma unroll
  for (int w = 1; w < 64; w <<= 1) { const int o = __shfl_xor(arg, w); arg = o < arg ? o : arg; }
  const double vals[kEnsRows] = {(double)q.cnt[0], (double)q.cnt[1], q.sum_ep, q.sum_ep2, q.max_ep, q.min_ep, q.sum_es, q.max_es,
                                 OUT ? q.sum_tau : 0.0, OUT ? q.max_tau : 0.0, (double)q.cnt[2], STAT ? (double)q.cnt[3] : 0.0,
                                 q.sd[0], q.sd[1], q.sd[2], arg == 0x7fffffff ? -1.0 : (double)arg};
  double mine = vals[0];
#pragma unroll
  for (int r = 1; r < kEnsRows; ++r) mine = lane == r ? vals[r] : mine;
  if (lane < kEnsRows) row[lane] = mine;
}

// NS steps (i, i + stride, ..) of one group by one wavefront: the loads of all NS are issued before the first is used
template <typename T, bool TAB, bool OUT, bool STAT, int NS>
__device__ __forceinline__ void ens_steps(const EnsArgs<T> &e, const int32_t *mem, int n, int b_first, int lane, int g, long long i,
                                          long long stride) {
  const ScoreArgs<T> &a = e.t;
  const size_t B = (size_t)a.B;
  EnsAcc q[NS];
  int b = b_first;
  for (int m0 = 0; m0 < n; m0 += 64) {
    const int m = m0 + lane, mn = m + 64;
    const int b_next = mem[mn < n ? mn : n - 1];      // the next trip's robot travels with this trip's words
    T rc[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
    if (!TAB) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { rc[j] = a.ref[(size_t)j * B + b]; rc[3 + j] = a.ref[(size_t)(6 + j) * B + b]; }
    }
    ScoreStep<T> v[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) score_load<T, false, TAB, OUT, STAT>(a, B, 0, (unsigned)b, i + s * stride, rc, v[s]);
#pragma unroll
    for (int s = 0; s < NS; ++s) ens_fold(a, v[s], m < n, b, q[s]);
    b = b_next;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) ens_store<OUT, STAT>(q[s], lane, e.ens + ((size_t)(i + s * stride) * e.G + g) * kEnsRows);
}

template <typename T, bool TAB, bool OUT, bool STAT>
__global__ __launch_bounds__(64 * kEnsWaves) void umpc_ensemble_kernel(const EnsArgs<T> e) {
  // (blockDim = (64, kEnsWaves): threadIdx.y is the same in every lane of a wavefront -- said to the compiler)
  const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
  const int g = blockIdx.x;
  const auto [lo, n] = group_window(e.offset, g);
  const long long stride = (long long)gridDim.y * kEnsWaves, count = e.t.count;
  const int32_t *mem = e.order + lo;
  // the first trip's robot is the same for every step of this wavefront (n == 0: no trip, nothing is read)
  const int b_first = n > 0 ? mem[lane < n ? lane : n - 1] : 0;
  long long i = (long long)blockIdx.y * kEnsWaves + wave;
  for (; i + stride < count; i += 2 * stride) ens_steps<T, TAB, OUT, STAT, 2>(e, mem, n, b_first, lane, g, i, stride);
  if (i < count) ens_steps<T, TAB, OUT, STAT, 1>(e, mem, n, b_first, lane, g, i, stride);
}

// key of a robot: its group id, or G for every id outside [0, G)
__device__ __forceinline__ int ens_key(int id, int G) { return ((id >= 0) & (id < G)) ? id : G; }

constexpr int kIndexUnroll = 4;     // trips of 64 ids whose loads are issued together

__global__ __launch_bounds__(64) void umpc_group_index_kernel(const int32_t *group, int B, int G, int32_t *order, int32_t *offset) {
  const int g = blockIdx.x, lane = threadIdx.x;             // g in [0, G]
  // pass 1: robots with a smaller key
  int less = 0;
  for (long long base = 0; base < B; base += 64 * kIndexUnroll) {
    int id[kIndexUnroll];
#pragma unroll
    for (int u = 0; u < kIndexUnroll; ++u) { const long long b = base + 64 * u + lane; id[u] = b < B ? group[b] : -1; }
#pragma unroll
    for (int u = 0; u < kIndexUnroll; ++u) {
      const long long b = base + 64 * u + lane;
      less += __popcll(__ballot((b < B) & (ens_key(id[u], G) < g)));
    }
  }
  if (lane == 0) offset[g] = less;
  // pass 2: this key's robots in ascending index
  int at = less;
  for (long long base = 0; base < B; base += 64 * kIndexUnroll) {
    int id[kIndexUnroll];
#pragma unroll
    for (int u = 0; u < kIndexUnroll; ++u) { const long long b = base + 64 * u + lane; id[u] = b < B ? group[b] : -1; }
#pragma unroll
    for (int u = 0; u < kIndexUnroll; ++u) {
      const long long b = base + 64 * u + lane;
      const bool mine = (b < B) & (ens_key(id[u], G) == g);
      const unsigned long long bal = __ballot(mine);
      const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
      if (mine) order[at + rank] = (int32_t)b;       // at + rank < B: the keys partition the robots
      at += __popcll(bal);
    }
  }
}

}  // namespace umpc
