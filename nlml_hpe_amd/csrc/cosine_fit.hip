// cosine_fit.hip -- K8: a batch of independent cosine fits a cos(b w + c) + d, each a whole Powell minimisation, in one launch.
//
// Replaces TD_Trainer.Train's nine calls of scipy.optimize.minimize(objective, guess, method='Powell') (TD_Trainer.py:70-93,320-322;
// 476..4,000 evaluations of an interpreted loop each).  One WAVE owns one fit for the whole minimisation:
//
//   repeat:  lane i < n evaluates the squared residual q_i of row i at the machine's trial point (cosine_fit_ref.h: one correctly
//            rounded cos per lane, all rows at once); the wave forms the sequential sum ((q_0 + q_1) + ...) + q_{n-1} in the
//            reference's order from the lanes' values; lane 0 resumes the fit's Powell/Brent machine (powell.h) with sum / 2
//   until the machine has finished.
//
// The machine is powell.h's, instantiated for four parameters; it lives in LDS and is reached through a real call with an LDS
// pointer, as in tucker_powell.hip and for the same reasons (the switch inlined would set the register demand of the whole kernel;
// through a generic pointer every access would be a flat_ one).  A workgroup is four waves that share nothing: no barrier, no
// atomics, no grid-level synchronisation; a wave ends when its fit does (at most maxfev = 4000 evaluations).  Fits may have
// different row counts n[f] <= 64 in one launch.
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "cosine_fit_ref.h"

namespace nlml {

constexpr int CF_WAVES = 4;                 // fits per workgroup
constexpr int CF_NT = 64 * CF_WAVES;

typedef __attribute__((address_space(3))) PowellState4 LdsState4;

__device__ __attribute__((noinline)) bool cf_powell_step_call(LdsState4* s, double f) { return powell_step(*(PowellState4*)s, f); }

// the value lane `src` (wave-uniform) holds
__device__ __forceinline__ double cf_lane_value(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// The objective at (a, b, c, d), the same value in every lane: lane i < n holds row i (y, wr = cf_radians(w_deg)); n is wave-uniform.
__device__ __forceinline__ double cf_wave_objective(double y, double wr, int n, int lane, double a, double b, double c, double d) {
  NLML_FP_STRICT
  const double q = lane < n ? cf_term(y, wr, a, b, c, d) : 0.0;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = s + cf_lane_value(q, i);
  return s / 2.0;
}

// row count of a fit as the kernels use it: whatever the device array holds, no lane reads beyond the row (the entry point has
// checked the caller's host copy: 1 <= n <= min(64, ld))
__device__ __forceinline__ int cf_rows(int n, int64_t ld) {
  const int cap = ld < CF_ROWS_MAX ? (int)ld : CF_ROWS_MAX;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

__global__ __launch_bounds__(CF_NT) void cosine_fit_kernel(const double* __restrict__ y, const double* __restrict__ w_deg, int64_t ld,
                                                           const int32_t* __restrict__ nrows, int64_t C, const double* __restrict__ x0,
                                                           double xtol, double ftol, double* __restrict__ x, double* __restrict__ fun,
                                                           int32_t* __restrict__ nfev, int32_t* __restrict__ nit,
                                                           int32_t* __restrict__ status) {
  __shared__ PowellState4 st[CF_WAVES];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t f = (int64_t)blockIdx.x * CF_WAVES + wave;
  if (f >= C) return;   // the waves of a workgroup never meet at a barrier
  const int n = __builtin_amdgcn_readfirstlane(cf_rows(nrows[f], ld));
  const double yl = lane < n ? y[f * ld + lane] : 0.0;
  const double wr = lane < n ? cf_radians(w_deg[f * ld + lane]) : 0.0;

  LdsState4* s = (LdsState4*)&st[wave];
  int need = 0;
  if (lane == 0) {
    for (int k = 0; k < CF_NPAR; ++k) st[wave].xeval[k] = x0[f * CF_NPAR + k];   // the start, by way of the trial-point slot
    powell_init(st[wave], st[wave].xeval, xtol, ftol);
    need = cf_powell_step_call(s, 0.0) ? 1 : 0;
  }
  need = __builtin_amdgcn_readfirstlane(need);
  // every evaluation is counted by the machine and refused beyond maxfun = 4000: the bound only states that the loop ends
  for (int round = 0; need && round < CF_NPAR * 1000 + 16; ++round) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // lane 0's trial point, written in the call, is read by all lanes
    const double a = s->xeval[0], b = s->xeval[1], c = s->xeval[2], d = s->xeval[3];
    const double fe = cf_wave_objective(yl, wr, n, lane, a, b, c, d);
    int nd = 0;
    if (lane == 0) nd = cf_powell_step_call(s, fe) ? 1 : 0;
    need = __builtin_amdgcn_readfirstlane(nd);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane < CF_NPAR) x[f * CF_NPAR + lane] = s->x[lane];
  if (lane == 0) {
    if (fun) fun[f] = s->fval;
    if (nfev) nfev[f] = s->nfev;
    if (nit) nit[f] = s->iter;
    if (status) status[f] = need ? PW_RUNNING : s->status;
  }
}

// one wave per parameter point, against one fit's rows: the kernel above's evaluation, read out
__global__ __launch_bounds__(CF_NT) void cosine_fit_objective_kernel(const double* __restrict__ y, const double* __restrict__ w_deg, int n,
                                                                     const double* __restrict__ params, int64_t N,
                                                                     double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t e = (int64_t)blockIdx.x * CF_WAVES + wave;
  if (e >= N) return;
  n = __builtin_amdgcn_readfirstlane(cf_rows(n, CF_ROWS_MAX));
  const double yl = lane < n ? y[lane] : 0.0;
  const double wr = lane < n ? cf_radians(w_deg[lane]) : 0.0;
  const double* p = params + e * CF_NPAR;
  const double fe = cf_wave_objective(yl, wr, n, lane, p[0], p[1], p[2], p[3]);
  if (lane == 0) out[e] = fe;
}

int launch_cosine_fit(const double* y, const double* w_deg, int64_t ld, const int32_t* n, int64_t C, const double* x0, double xtol,
                      double ftol, double* x, double* fun, int32_t* nfev, int32_t* nit, int32_t* status, void* stream) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(cosine_fit_kernel, dim3((unsigned)((C + CF_WAVES - 1) / CF_WAVES)), dim3(CF_NT), 0, reinterpret_cast<hipStream_t>(stream),
                     y, w_deg, ld, n, C, x0, xtol, ftol, x, fun, nfev, nit, status);
  return hip_launch_status();
}

int launch_cosine_fit_objective(const double* y, const double* w_deg, int n, const double* params, int64_t N, double* out, void* stream) {
  if (N == 0) return 0;
  hipLaunchKernelGGL(cosine_fit_objective_kernel, dim3((unsigned)((N + CF_WAVES - 1) / CF_WAVES)), dim3(CF_NT), 0,
                     reinterpret_cast<hipStream_t>(stream), y, w_deg, n, params, N, out);
  return hip_launch_status();
}

}  // namespace nlml
