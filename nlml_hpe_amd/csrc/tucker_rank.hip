// tucker_rank.hip -- K3 and the device-side Powell minimiser for any Tucker identity rank R = 1..16 (nlml_tucker_objective_r,
// nlml_tucker_powell_r): Wm f32[27 R, 1404], 3 + R parameters per evaluation.  The arithmetic is tucker_ref.h's (reference order, the
// parity mode) and tucker_common.h's (matrix cores) with the rank as a run-time value: tucker_rank.h.  R = 5 is handed on by the launchers
// below to the kernels of tucker_objective.hip / tucker_powell.hip, so the shipped artefacts run the code they always ran.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "abi_internal.h"
#include "powell.h"
#include "tucker_rank.h"

namespace nlml {

struct GlobalParR {
  const double* p;   // params of this block's first evaluation
  int64_t left;      // evaluations available from there (>= 1)
  int n;             // parameters per evaluation, 3 + R
  __device__ __forceinline__ double operator()(int e, int k) const {
    return gload<double>(p + (e < left ? e : left - 1) * n + k);
  }
};

// row functors of the reference-order pass (passed by value into the non-inlined pass); slots beyond N read the last row
struct RankXRow {
  const float* x;
  const int32_t* x_index;
  int64_t ldx, e0, N;
  __device__ __forceinline__ const float* operator()(int slot) const {
    int64_t n = e0 + slot;
    n = n < N ? n : N - 1;
    return x + (x_index ? (int64_t)x_index[n] : n) * ldx;
  }
};
struct RankXhRow {
  double* x_hat;
  int64_t e0;
  __device__ __forceinline__ double* operator()(int slot) const { return x_hat ? x_hat + (e0 + slot) * TM : (double*)nullptr; }
};
struct RankNoXhRow {
  static constexpr double* x_hat = nullptr;
  __device__ __forceinline__ double* operator()(int) const { return nullptr; }
};

__device__ __forceinline__ void load_cos_rows(const double* __restrict__ cosp, int tid, double (&cp4)[4]) {
  cp4[0] = cp4[1] = cp4[2] = cp4[3] = 0.0;
  if (tid < EV * 9) {
    const double* c4 = cosp + ((tid % 9) / 3 * 3 + tid % 3) * 4;     // (a,b,c,d) row, TD_Tester.py:26
    cp4[0] = c4[0]; cp4[1] = c4[1]; cp4[2] = c4[2]; cp4[3] = c4[3];
  }
}

// this lane's x values of its four evaluations, then the residual norms of all 16 into sh.red (tucker_err)
__device__ __forceinline__ void rank_residual(TuckerSharedR& sh, const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ x_index,
                                              int64_t e0, int64_t N, const f64x4 (&acc)[MBW], int tid) {
  float xv[MBW][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int64_t n = e0 + ((tid & 63) >> 4) + 4 * r;
    n = n < N ? n : N - 1;
    float v[MBW];
    tucker_load_x(x + (x_index ? (int64_t)x_index[n] : n) * ldx, tid, v);
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb) xv[mb][r] = v[mb];
  }
  tucker_residual(sh, xv, acc, tid);
}

// ---- K3 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TNT, 2) void tucker_objective_r_kernel(
    const float* __restrict__ Wm, const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ x_index,
    const double* __restrict__ params, const double* __restrict__ cosp, int64_t N, double* __restrict__ err,
    double* __restrict__ x_hat, int rid) {
  __shared__ __attribute__((aligned(16))) TuckerSharedR sh;
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * EV;
  double cp4[4];
  load_cos_rows(cosp, tid, cp4);
  GlobalParR par{params + e0 * (3 + rid), N - e0, 3 + rid};
  tucker_coef_r(sh, par, cp4, tid, rid);
  f64x4 acc[MBW];
  tucker_mfma_r(sh, Wm, tid, rid, acc);
  const int lane = tid & 63, wv = tid >> 6, col = lane & 15;
  if (x_hat) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = e0 + (lane >> 4) + 4 * r;
#pragma unroll
      for (int mb = 0; mb < MBW; ++mb)
        if (n < N && tcol_live(wv, col, mb)) x_hat[n * TM + tcol0(wv) + tlcol(col, mb)] = acc[mb][r];
    }
  }
  rank_residual(sh, x, ldx, x_index, e0, N, acc, tid);
  if (tid < EV && e0 + tid < N) err[e0 + tid] = tucker_err(sh, tid);
}

__global__ __launch_bounds__(TR_NT, 1) void tucker_objective_ref_r_kernel(
    const float* __restrict__ Wm, const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ x_index,
    const double* __restrict__ params, const double* __restrict__ cosp, int64_t N, double* __restrict__ err,
    double* __restrict__ x_hat, int rid) {
  __shared__ __attribute__((aligned(16))) TuckerFvecShared sh;
  __shared__ __attribute__((aligned(16))) TuckerRefSharedR<8> rs;
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * EV;
  double cp4[4];
  load_cos_rows(cosp, tid, cp4);
  GlobalParR par{params + e0 * (3 + rid), N - e0, 3 + rid};
  tucker_fvec(sh, par, cp4, tid);
  const int64_t left = N - e0;
  const int mask = left >= EV ? 0xffff : ((1 << (int)left) - 1);
  tucker_ref_eval_r(sh, rs, Wm, par, mask, RankXRow{x, x_index, ldx, e0, N}, RankXhRow{x_hat, e0}, tid, rid);
  if (tid < EV && e0 + tid < N) err[e0 + tid] = rs.err[tid];
}

// ---- device Powell -------------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) PowellStateN LdsPowellStateN;
__device__ __attribute__((noinline)) bool powell_step_call_n(LdsPowellStateN* s, double f) { return powell_step(*(PowellStateN*)s, f); }

struct LdsParN {
  const PowellStateN* st;
  __device__ __forceinline__ double operator()(int e, int k) const {
    return ((const __attribute__((address_space(3))) PowellStateN*)st)[e].xeval[k];
  }
};

// a matrix-core round: all 16 evaluations (tucker_powell.hip's tucker_round16 for a run-time rank)
__device__ __attribute__((noinline)) void tucker_round16_r(TuckerSharedR& sh, const float* __restrict__ Wm, const float* __restrict__ x,
                                                           int64_t ldx, int64_t e0, int64_t N, int tid, int rid) {
  rid = __builtin_amdgcn_readfirstlane(rid);   // (arguments of a non-inlined function arrive in vector registers)
  f64x4 acc[MBW];
  tucker_mfma_r(sh, Wm, tid, rid, acc);
  rank_residual(sh, x, ldx, nullptr, e0, N, acc, tid);
}

// tucker_powell_kernel (tucker_powell.hip) with n = 3 + R parameters per machine.  LDS of the workgroup, which still owns 16 faces:
//   machines   16 x sizeof(PowellStateN) = 16 x 4,192 B = 65.5 KB: the direction set is n x n, and the state is laid out for the
//              largest n = 19 whatever the rank (one kernel, static offsets);
//   reference order   + the pass tables for SEVEN evaluations (86.5 KB; eight would need 98.8 KB) + the f-vectors = 153.2 of 160 KB:
//              16 live machines go as three passes (6 + 5 + 5) where the rank-5 kernel, whose machines take 21 KB, makes two of 8;
//   matrix cores      + the coefficient table of the largest rank (54 KB) = 122 KB, one workgroup per CU.
template <int ORDER>
__global__ __launch_bounds__(ORDER == NLML_TD_ORDER_REFERENCE ? TR_NT : TNT, 1) void tucker_powell_r_kernel(
    const float* __restrict__ Wm, const float* __restrict__ x, int64_t ldx, const double* __restrict__ cosp,
    int64_t N, const double* __restrict__ x0, double* __restrict__ result, double* __restrict__ fval,
    int32_t* __restrict__ nfev, int32_t* __restrict__ nit, int32_t* __restrict__ status, int rid) {
  constexpr bool REF = ORDER == NLML_TD_ORDER_REFERENCE;
  __shared__ __attribute__((aligned(16))) std::conditional_t<REF, TuckerFvecShared, TuckerSharedR> sh;
  __shared__ PowellStateN st[EV];
  __shared__ int need[EV];
  __shared__ int livew[2];

  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * EV;
  const int n = 3 + rid;
  double cp4[4];
  load_cos_rows(cosp, tid, cp4);

  // machine e on lane e&1 of wave e>>1, as in the rank-5 kernel
  const int me = ((tid & 63) < 2 && tid < 64 * (EV / 2)) ? 2 * (tid >> 6) + (tid & 63) : -1;
  if (me >= 0) {
    const bool live = e0 + me < N;
    st[me].set_dim(n);
    for (int k = 0; k < n; ++k) st[me].xeval[k] = (x0 && live) ? x0[(e0 + me) * n + k] : 0.0;   // the start, by way of the trial-point slot
    powell_init(st[me], st[me].xeval);
    for (int k = 0; k < PW_NMAX; ++k) st[me].xeval[k] = 0.0;   // slots beyond N are evaluated too (and ignored): defined parameters
    const bool nd = live && powell_step_call_n((LdsPowellStateN*)&st[me], 0.0);
    need[me] = nd ? 1 : 0;
  }
  __syncthreads();

  const LdsParN lp{st};
  if (tid == 0) {
    int m0 = 0;
    for (int e = 0; e < EV; ++e) m0 |= need[e] << e;
    livew[0] = m0;
    livew[1] = 0;
  }
  __syncthreads();
  for (int round = 0; round < n * 1000 + 16; ++round) {
    const int live_mask = livew[round & 1];
    if (!live_mask) break;
    if (tid == 0) livew[(round + 1) & 1] = 0;     // last read a round ago; the barriers of the evaluation order this before the ORs below

    double fe = 0.0;
    if constexpr (REF) {
      __shared__ __attribute__((aligned(16))) TuckerRefSharedR<7> rs;
      tucker_fvec(sh, lp, cp4, tid);
      tucker_ref_eval_r(sh, rs, Wm, lp, live_mask, RankXRow{x, nullptr, ldx, e0, N}, RankNoXhRow{}, tid, rid);
      if (me >= 0) fe = rs.err[me];
    } else {
      tucker_coef_r(sh, lp, cp4, tid, rid);
      tucker_round16_r(sh, Wm, x, ldx, e0, N, tid, rid);
      if (me >= 0) fe = tucker_err(sh, me);
    }
    if (me >= 0 && need[me]) {   // resume the state machines with their objective values
      const bool nd = powell_step_call_n((LdsPowellStateN*)&st[me], fe);
      need[me] = nd ? 1 : 0;
      if (nd) atomicOr(&livew[(round + 1) & 1], 1 << me);
    }
    __syncthreads();
  }

  if (tid < EV && e0 + tid < N) {
    const int64_t f = e0 + tid;
    for (int k = 0; k < n; ++k) result[f * n + k] = st[tid].x[k];
    if (fval) fval[f] = st[tid].fval;
    if (nfev) nfev[f] = st[tid].nfev;
    if (nit) nit[f] = st[tid].iter;
    if (status) status[f] = need[tid] ? PW_RUNNING : st[tid].status;
  }
}

int launch_tucker_objective_r(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                              const double* cos_params, int64_t N, double* err, double* x_hat, int r_id, int order, void* stream) {
  if (r_id == 5) return launch_tucker_objective(Wm, x, ldx, x_index, params, cos_params, N, err, x_hat, order, stream);   // the shipped artefacts' kernels
  if (N == 0) return 0;
  const dim3 grid((unsigned)((N + EV - 1) / EV));
  if (order == NLML_TD_ORDER_REFERENCE)
    hipLaunchKernelGGL(tucker_objective_ref_r_kernel, grid, dim3(TR_NT), 0, reinterpret_cast<hipStream_t>(stream), Wm, x, ldx,
                       x_index, params, cos_params, N, err, x_hat, r_id);
  else
    hipLaunchKernelGGL(tucker_objective_r_kernel, grid, dim3(TNT), 0, reinterpret_cast<hipStream_t>(stream), Wm, x, ldx,
                       x_index, params, cos_params, N, err, x_hat, r_id);
  return hip_launch_status();
}

int launch_tucker_powell_r(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                           double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int r_id, int order,
                           void* stream) {
  if (r_id == 5) return launch_tucker_powell(Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, order, stream);
  if (N == 0) return 0;
  const dim3 grid((unsigned)((N + EV - 1) / EV));
  if (order == NLML_TD_ORDER_REFERENCE)
    hipLaunchKernelGGL((tucker_powell_r_kernel<NLML_TD_ORDER_REFERENCE>), grid, dim3(TR_NT), 0, reinterpret_cast<hipStream_t>(stream),
                       Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, r_id);
  else
    hipLaunchKernelGGL((tucker_powell_r_kernel<NLML_TD_ORDER_FAST>), grid, dim3(TNT), 0, reinterpret_cast<hipStream_t>(stream),
                       Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, r_id);
  return hip_launch_status();
}

}  // namespace nlml
