// The store side of tools/microbench_vmem.hip: what does it cost ONE wave per SIMD (the step kernel's occupancy) to WRITE 16
// (or 4) words per 64 VALU instructions with global_store_dword (lane-contiguous rows of 256 B) or global_store_dwordx4
// (16 B per lane, 1 KiB per instruction), plain and with the `nt` hint the lane stream puts on its workspace rows?
// The body is the same 64 v_fmac (4 chains); stores are never waited for inside the loop (vmcnt only at the end), so what
// shows is the ISSUE cost and the throughput of the memory pipe. Each wave writes its own 16 KiB window (1 024 waves:
// 16 MiB, 2 MiB per XCD), four 4-KiB quarters in turn.
// Build: hipcc --offload-arch=gfx950 -O3 -o tools/microbench_vmem_store tools/microbench_vmem_store.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float f4 __attribute__((ext_vector_type(4)));
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("err %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)

// four one-word stores of rows O .. O + 768 (256 B apart); NT: " nt" or ""
#define ST1B(O, NT) "global_store_dword %0, %1, %5 offset:" #O "+0" NT "\n global_store_dword %0, %2, %5 offset:" #O "+256" NT "\n global_store_dword %0, %3, %5 offset:" #O "+512" NT "\n global_store_dword %0, %4, %5 offset:" #O "+768" NT
// four one-word stores of words 0 .. 3 of the 1-KiB group at O (lane stride 16 B: where a four-word access finds them)
#define ST1S(O, NT) "global_store_dword %0, %1, %5 offset:" #O "+0" NT "\n global_store_dword %0, %2, %5 offset:" #O "+4" NT "\n global_store_dword %0, %3, %5 offset:" #O "+8" NT "\n global_store_dword %0, %4, %5 offset:" #O "+12" NT

template <int MODE>
__global__ __launch_bounds__(256) void k(float *out, float *dst, long long *cyc, int iters) {
  extern __shared__ float dyn[];
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float a[4], b[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = out[i * 256 + threadIdx.x];
#pragma unroll
  for (int i = 0; i < 16; ++i) b[i] = out[(4 + i) * 256 + threadIdx.x];
  if (iters < 0) dyn[threadIdx.x] = a[0];
  float *base = dst + (size_t)wave * 4096;          // 16 KiB window per wave
  const f4 r0 = {b[0], b[1], b[2], b[3]}, r1 = {b[4], b[5], b[6], b[7]}, r2 = {b[8], b[9], b[10], b[11]}, r3 = {b[12], b[13], b[14], b[15]};
  constexpr bool NT = MODE >= 6;
  // 1: 16 x dword, 2: 4 x dwordx4, 3: 1 x dwordx4, 4: 4 x dword, 5: 16 x dword into the layout of the dwordx4 (16-B lane stride)
  constexpr int KIND = MODE == 0 ? 0 : (MODE - 1) % 5 + 1;
  long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; ++it) {
    const unsigned long long pa = (unsigned long long)(base + ((it & 3) * 1024));
    float *p = (float *)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(pa >> 32)) << 32) |
                         (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)pa));
    if (KIND == 1 || KIND == 4) {
      if (NT) asm volatile(ST1B(0, " nt") : : "v"(lane * 4), "v"(r0.x), "v"(r0.y), "v"(r0.z), "v"(r0.w), "s"(p) : "memory");
      else asm volatile(ST1B(0, "") : : "v"(lane * 4), "v"(r0.x), "v"(r0.y), "v"(r0.z), "v"(r0.w), "s"(p) : "memory");
    }
    if (KIND == 1) {
      if (NT) {
        asm volatile(ST1B(1024, " nt") : : "v"(lane * 4), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "s"(p) : "memory");
        asm volatile(ST1B(2048, " nt") : : "v"(lane * 4), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w), "s"(p) : "memory");
        asm volatile(ST1B(3072, " nt") : : "v"(lane * 4), "v"(r3.x), "v"(r3.y), "v"(r3.z), "v"(r3.w), "s"(p) : "memory");
      } else {
        asm volatile(ST1B(1024, "") : : "v"(lane * 4), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "s"(p) : "memory");
        asm volatile(ST1B(2048, "") : : "v"(lane * 4), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w), "s"(p) : "memory");
        asm volatile(ST1B(3072, "") : : "v"(lane * 4), "v"(r3.x), "v"(r3.y), "v"(r3.z), "v"(r3.w), "s"(p) : "memory");
      }
    }
    if (KIND == 2 || KIND == 3) {
      if (NT) asm volatile("global_store_dwordx4 %0, %1, %2 nt" : : "v"(lane * 16), "v"(r0), "s"(p) : "memory");
      else asm volatile("global_store_dwordx4 %0, %1, %2" : : "v"(lane * 16), "v"(r0), "s"(p) : "memory");
    }
    if (KIND == 2) {
      if (NT) asm volatile("global_store_dwordx4 %0, %1, %4 offset:1024 nt\n global_store_dwordx4 %0, %2, %4 offset:2048 nt\n global_store_dwordx4 %0, %3, %4 offset:3072 nt"
                           : : "v"(lane * 16), "v"(r1), "v"(r2), "v"(r3), "s"(p) : "memory");
      else asm volatile("global_store_dwordx4 %0, %1, %4 offset:1024\n global_store_dwordx4 %0, %2, %4 offset:2048\n global_store_dwordx4 %0, %3, %4 offset:3072"
                        : : "v"(lane * 16), "v"(r1), "v"(r2), "v"(r3), "s"(p) : "memory");
    }
    if (KIND == 5) {
      if (NT) {
        asm volatile(ST1S(0, " nt") : : "v"(lane * 16), "v"(r0.x), "v"(r0.y), "v"(r0.z), "v"(r0.w), "s"(p) : "memory");
        asm volatile(ST1S(1024, " nt") : : "v"(lane * 16), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "s"(p) : "memory");
        asm volatile(ST1S(2048, " nt") : : "v"(lane * 16), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w), "s"(p) : "memory");
        asm volatile(ST1S(3072, " nt") : : "v"(lane * 16), "v"(r3.x), "v"(r3.y), "v"(r3.z), "v"(r3.w), "s"(p) : "memory");
      } else {
        asm volatile(ST1S(0, "") : : "v"(lane * 16), "v"(r0.x), "v"(r0.y), "v"(r0.z), "v"(r0.w), "s"(p) : "memory");
        asm volatile(ST1S(1024, "") : : "v"(lane * 16), "v"(r1.x), "v"(r1.y), "v"(r1.z), "v"(r1.w), "s"(p) : "memory");
        asm volatile(ST1S(2048, "") : : "v"(lane * 16), "v"(r2.x), "v"(r2.y), "v"(r2.z), "v"(r2.w), "s"(p) : "memory");
        asm volatile(ST1S(3072, "") : : "v"(lane * 16), "v"(r3.x), "v"(r3.y), "v"(r3.z), "v"(r3.w), "s"(p) : "memory");
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(a[i & 3]) : "v"(b[i]), "v"(b[(i + 1) & 15]));
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += a[i];
  out[(blockIdx.x * 256 + threadIdx.x) % (32 * 256)] = s;
  if (lane == 0) cyc[wave] = t1 - t0;
}

template <int M> void launch(int blocks, int lds, float *d, float *s, long long *c, int iters) {
  hipFuncSetAttribute((const void *)k<M>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(k<M>, dim3(blocks), dim3(256), lds, 0, d, s, c, iters);
}

int main() {
  float *d, *s; long long *c;
  const int iters = 4000, blocks = 256, lds = 160 * 1024;      // 160 KiB of LDS: one workgroup per CU, one wave per SIMD
  CHECK(hipMalloc(&d, 32 * 256 * sizeof(float)));
  CHECK(hipMemset(d, 0, 32 * 256 * sizeof(float)));
  CHECK(hipMalloc(&s, (size_t)blocks * 4 * 4096 * sizeof(float)));
  CHECK(hipMemset(s, 0, (size_t)blocks * 4 * 4096 * sizeof(float)));
  CHECK(hipMalloc(&c, blocks * 4 * sizeof(long long)));
  const char *names[] = {"64 fmac (4 chains) alone", "+ 16 global_store_dword", "+ 4 global_store_dwordx4", "+ 1 global_store_dwordx4 (4 words)",
                         "+ 4 global_store_dword (4 words)", "+ 16 global_store_dword, 16-B lane stride",
                         "+ 16 global_store_dword nt", "+ 4 global_store_dwordx4 nt", "+ 1 global_store_dwordx4 nt (4 words)",
                         "+ 4 global_store_dword nt (4 words)", "+ 16 global_store_dword nt, 16-B lane stride"};
  const int words[] = {16, 16, 16, 4, 4, 16, 16, 16, 4, 4, 16};
  double base = 0;
  for (int m = 0; m < 11; ++m) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int rep = 0; rep < 2; ++rep) {
      hipEventRecord(e0);
      switch (m) {
#define CASE(M) case M: launch<M>(blocks, lds, d, s, c, iters); break;
        CASE(0) CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10)
      }
      hipEventRecord(e1); CHECK(hipEventSynchronize(e1));
    }
    float ms; hipEventElapsedTime(&ms, e0, e1);
    if (m == 0) base = ms;
    printf("%-46s : wall %.3f ms, %.1f ns per body, +%.1f ns for the %d words (%.2f ns per word)\n", names[m], ms, ms * 1e6 / iters,
           (ms - base) * 1e6 / iters, words[m], (ms - base) * 1e6 / iters / words[m]);
  }
  return 0;
}
