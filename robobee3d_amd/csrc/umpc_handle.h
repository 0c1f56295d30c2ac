// Private to libumpc_mi355x.so: what every translation unit of the batch API needs of a handle -- the handle itself, the
// cursor rule of its tables, the parameter block the kernels take, and the error helpers. The message umpcLastError() returns
// lives in umpc_mi355x.hip; everything here writes it through umpc_set_error (umpc_err.h). Nothing in this header has
// external linkage that the public header does not declare.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/umpc_mi355x.h"
#include "umpc_err.h"
#include "umpc_plant.h"

constexpr int kBlock = 64;  // one wavefront per workgroup: 64 robots, no barriers anywhere

static inline int fail(hipError_t e, const char *what) {
  umpc_set_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
  return (int)e;
}
// after a kernel launch: 0, or the launch error under the entry point's name
static inline int launch_status(const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(e, what);
}
// A refusal: "<entry point>: <reason>" for umpcLastError, -1 for the caller to return.
static inline int refuse(const char *fn, const char *why) {
  umpc_set_error((std::string(fn) + ": " + why).c_str());
  return -1;
}

// A table the handle keeps by pointer and walks with a cursor (reference trajectory, step history, impulses): `steps` slices,
// the next closed-loop step uses slice `cursor`. One rule for all of them: a setter takes 0 <= cursor0 <= steps, and a launch
// that would pass the end is refused before anything is launched or copied.
struct CursorTable {
  long long steps = 0, cursor = 0;
  static bool valid(const char *setter, long long steps, long long cursor0) {
    if (steps >= 1 && cursor0 >= 0 && cursor0 <= steps) return true;
    umpc_set_error((std::string(setter) + ": bad argument (steps >= 1, 0 <= cursor0 <= steps)").c_str());
    return false;
  }
  // do the n slices of a launch fit? `n_name` is what the message calls n ("K " in a rollout)
  bool fits(const char *who, const char *table, const char *n_name, long long n) const {
    if (cursor + n <= steps) return true;
    umpc_set_error((std::string(who) + ": the " + table + " ends before the launch does (cursor " + std::to_string(cursor) + " + " + n_name +
                    std::to_string(n) + " > steps " + std::to_string(steps) + ")").c_str());
    return false;
  }
};

struct umpc_batch {
  umpc_batch_params_t prm;
  int B, dtype;
  long long global_B = 0;        // size of the whole (sharded) job, umpcBatchSetGlobalBatch; the lane / quad choice is made from it
  int task = 0;
  double task_p[4] = {0, 0, 0, 0};
  double t_ms = 0;               // time of the next MPC step
  const void *weights = nullptr;  // [8][B] device table or null
  void *ws;  // [WS_ROWS][B] scratch the step parks Ruiz scalings / x_prev / delta_y in; fp32: at least WS_WIDE_ROWS rows and
             // 1 KB behind row WS_DS, where the lane stream keeps its four-word groups (umpcBatchCreate sizes it)
  int step_kernel = 0;            // 0 = automatic, 1 = always the C++ / loop-assembly kernel, 2 / 3 = the all-assembly stream with one lane / one lane quad per robot
  umpc::WLDev *wl = nullptr;      // device copy of the WL parameters (umpcBatchSetWL), null = no coupling
  void *wlu = nullptr, *wlw = nullptr;
  float wl_md2 = 0.f;             // M0[2,2] of the WL coupling (host copy, for the kernel's mb g)
  const char *last_kernel = "";   // the kernel the last umpcBatchRollout / umpcBatchUpdate dispatched (umpcBatchKernelName)
  float *taskf = nullptr;         // task table of the all-assembly kernel: 8 floats per step of a launch
  int taskf_cap = 0;              // ... steps it holds
  const void *reftab = nullptr;   // reference trajectory [steps][9][B] (umpcBatchSetRefTrajectory), kept by pointer; null = off
  CursorTable ref_c;              // ... its slices; the cursor is the slice the next closed-loop step reads
  // step history (umpcBatchSetHistory), kept by pointer; each may be null = that record is off
  void *hist_state = nullptr;     // [steps+1][18][B]
  void *hist_out = nullptr;       // [steps][9][B]
  int32_t *hist_status = nullptr; // [steps][B]
  void *hist_info = nullptr;      // [steps][2][B]
  CursorTable hist_c;             // ... the steps the tables hold; the cursor is the step the next rollout records first
  const void *imptab = nullptr;   // velocity impulses [steps][6][B] (umpcBatchSetImpulses), kept by pointer; null = off
  CursorTable imp_c;              // ... its slices; the cursor is the slice the next closed-loop step adds
  // the history and the impulses belong to closed-loop steps with a plant: only those are recorded, kicked and range-checked,
  // and only they advance the two cursors (the reference trajectory is read, and checked, by every call)
  bool hist_on(int K, int nsub) const { return (hist_state || hist_out || hist_status || hist_info) && nsub > 0 && K >= 1; }
  bool imp_on(int K, int nsub) const { return imptab && nsub > 0 && K >= 1; }
  // THE place the clock and the cursors advance: callers come here after every launch and copy of their call has returned
  // hipSuccess, so a refused or failed call leaves the handle where it was
  void advance(double ms, long long ref_n, long long hist_n, long long imp_n) {
    t_ms += ms; ref_c.cursor += ref_n; hist_c.cursor += hist_n; imp_c.cursor += imp_n;
  }
};

template <typename T>
static umpc::DevParams<T> make_dev(const umpc_batch_params_t &p) {
  umpc::DevParams<T> d;
  d.dt = (T)p.dt; d.g = (T)p.g;
  d.Tmax = (T)p.TtoWmax * (T)p.g;  // uprightmpc2.c:25
  d.wpr = (T)p.wpr; d.wpf = (T)p.wpf; d.ws = (T)p.ws; d.wvr = (T)p.wvr; d.wvf = (T)p.wvf;
  d.wds = (T)p.wds; d.wthrust = (T)p.wthrust; d.wmom = (T)p.wmom;
  for (int i = 0; i < 3; ++i) d.Ib[i] = (T)p.Ib[i];
  d.dtsim = (T)p.dtsim; d.taulim = (T)p.taulim;
  d.maxIter = p.maxIter; d.nsub = p.nsub; d.plant_mode = p.plant_mode;
  d.task = 0;
  for (int i = 0; i < 4; ++i) d.task_p[i] = T(0);
  return d;
}

// DevParams of a handle, its task included
template <typename T>
static umpc::DevParams<T> make_dev_task(const umpc_batch_t *h) {
  umpc::DevParams<T> d = make_dev<T>(h->prm);
  d.task = h->task;
  for (int i = 0; i < 4; ++i) d.task_p[i] = (T)h->task_p[i];
  return d;
}
