// tucker_powell.hip -- TD end-to-end on device: lock-step Powell minimisation of the Tucker objective.
//
// Replaces Test() (TD_Tester.py:162-199) = scipy Powell over objective() (:31-58), 2-4 s per face on
// the reference's CPU path.  One workgroup owns EV = 16 faces for the whole minimisation:
//
//   repeat:  lanes 0..15 each resume their face's Powell/Brent state machine (powell.h) with the
//            objective value of the previous round and publish the next trial point (8 doubles);
//            all 512 threads then evaluate the 16 objectives together exactly as K3 does
//            (tucker_common.h: one pass over Wm from L2 shared by the 16 evaluations, f64 MFMA);
//   until all 16 machines have finished.
//
// Faces are independent, so there is no grid-level synchronisation: a workgroup runs as many
// rounds as its slowest face needs (1.4k-7k).  The machine state lives in LDS.  Every round costs one Wm pass (758 KB from L2) per 8
// faces: ~383.7 kFLOP (f64) per face-evaluation, the same roofline as K3.  Rounds with at most PW_FEW live machines take
// the vector-ALU pass tucker_few (tucker_common.h): same bits, one Wm stream, no 16-wide MFMA work for dead machines.
// (Figures for the shipped artefacts' identity rank 5, 8 parameters per face; the kernel is written once over the rank traits of
// tucker_rank.h and serves any rank R = 1..16 with 3 + R parameters.)
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "powell.h"
#include "tucker_rank.h"

namespace nlml {

// The state machine is a large switch; inlined into the kernel it inflates the register demand of the
// whole function (spills in the MFMA loop).  As a real call its registers are its own.
// The state is passed as an LDS pointer: through a generic one every access to it would be a flat_load / flat_store.
template <typename State>
__device__ __attribute__((noinline)) bool powell_step_call(__attribute__((address_space(3))) State* s, double f) {
  return powell_step(*(State*)s, f);
}

// at most this many live machines: a few-machine pass instead of the 16-wide one -- 13 us (one machine, vector ALUs) or 15 us
// (2..4, 4x4x4 matrix instruction) a round against 30 us; BASELINE config 3 end to end: 0.117 s, 16-wide rounds only 0.24 s
#ifndef PW_FEW_N
#define PW_FEW_N 4
#endif
constexpr int PW_FEW = PW_FEW_N;
static_assert(PW_FEW >= 1 && PW_FEW <= 4, "the few-machine passes take one to four evaluations");

// A round with many live machines: all 16 evaluations on the 16x16x4 matrix cores, exactly K3's body.  Not inlined, like the
// few-machine passes: its 150 registers are then allocated on their own instead of across the state-machine code (inlined, the
// fully unrolled MFMA loop spilled).  The lane's 4 evaluations x 11 columns of the feature rows are re-read from L2 every round
// (44 dwords per lane against 374 of Wm).
// (K3 fetches its x rows with the loads of one of the last K steps; here the 44 extra live registers spill: measured slower)
template <typename Rank>
__device__ __attribute__((noinline)) void tucker_round16(typename Rank::Shared& sh, const float* __restrict__ Wm, const float* __restrict__ x,
                                                         int64_t ldx, int64_t e0, int64_t N, int tid, const Rank rk) {
  f64x4 acc[MBW];
  // (called directly: behind a forwarding member of the traits, or with the loop below in a helper, the rank-5 body is inlined in
  // another order and comes out as other code -- profiles/td_rank_fold_ab.md)
  if constexpr (Rank::kFixed) tucker_mfma(sh, Wm, tid, acc);
  else tucker_mfma_r(sh, Wm, tid, __builtin_amdgcn_readfirstlane(rk.rid), acc);   // (arguments of a non-inlined function arrive in vector registers)
  float xv[MBW][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int64_t n = e0 + ((tid & 63) >> 4) + 4 * r;
    n = n < N ? n : N - 1;
    float v[MBW];
    tucker_load_x(x + n * ldx, tid, v);
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb) xv[mb][r] = v[mb];
  }
  tucker_residual(sh, xv, acc, tid);
}

// The trial point of machine e IS its state's xeval field: the evaluation passes read the parameters straight from the machines
// (a separate copy per round cost ~450 cycles of one lane's LDS round trips).
template <typename State>
struct LdsPar {
  const State* st;
  __device__ __forceinline__ double operator()(int e, int k) const {
    return ((const __attribute__((address_space(3))) State*)st)[e].xeval[k];   // a ds_ read, not a flat_ one
  }
};

// ORDER = NLML_TD_ORDER_FAST: the objective as a GEMM on the f64 matrix cores (tucker_common.h); NLML_TD_ORDER_REFERENCE: in the
// reference's own operation order (tucker_ref.h) -- then the machines receive the reference's objective values bit for bit and
// walk scipy's trajectory (FX5: same evaluation counts, same final angles).
// Rank (tucker_rank.h) = TdRank5: n = 8 parameters per machine, 16 machines 21 KB of LDS, reference-order rounds of up to eight
// evaluations per pass, matrix-core rounds with the few-machine passes, two workgroups per CU.  TdRankDyn: n = 3 + R; LDS of the
// workgroup, which still owns 16 faces:
//   machines   16 x sizeof(PowellStateN) = 16 x 4,192 B = 65.5 KB: the direction set is n x n, and the state is laid out for the
//              largest n = 19 whatever the rank (one kernel, static offsets);
//   reference order   + the pass tables for SEVEN evaluations (86.5 KB; eight would need 98.8 KB) + the f-vectors = 153.2 of 160 KB:
//              16 live machines go as three passes (6 + 5 + 5) where rank 5 makes two of 8;
//   matrix cores      + the coefficient table of the largest rank (54 KB) = 122 KB, one workgroup per CU, 16-wide rounds only.
// The skeleton -- machine placement, start, the live words, the round loop, the resume, the write-out -- is one; the rank chooses
// how a round is evaluated.
template <int ORDER, typename Rank>
__global__ __launch_bounds__(ORDER == NLML_TD_ORDER_REFERENCE ? TR_NT : TNT, ORDER == NLML_TD_ORDER_REFERENCE ? 1 : Rank::kFastWorkgroups) void tucker_powell_kernel(
    const float* __restrict__ Wm, const float* __restrict__ x, int64_t ldx, const double* __restrict__ cosp,
    int64_t N, const double* __restrict__ x0, double* __restrict__ result, double* __restrict__ fval,
    int32_t* __restrict__ nfev, int32_t* __restrict__ nit, int32_t* __restrict__ status, int rid) {
  constexpr bool REF = ORDER == NLML_TD_ORDER_REFERENCE;
  typedef typename Rank::State State;
  typedef __attribute__((address_space(3))) State LdsState;
  __shared__ __attribute__((aligned(16))) std::conditional_t<REF, typename Rank::FvecShared, typename Rank::Shared> sh;
  __shared__ State st[EV];
  __shared__ int need[EV];

  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * EV;
  const Rank rk = Rank::make(rid);
  const int n = rk.npar();
  double cp4[4];
  load_cos_rows(cosp, tid, cp4);

  // machine e runs on lane e&1 of wave e>>1: two machines per wave, so the divergent state-machine code is at
  // most 2-way serialised and the 8 waves step their machines concurrently (16 machines on the lanes of one
  // wave would serialise up to 16 paths per round)
  const int me = ((tid & 63) < 2 && tid < 64 * (EV / 2)) ? 2 * (tid >> 6) + (tid & 63) : -1;   // (the reference-order workgroup has 12 waves)
  if (me >= 0) {
    const bool live = e0 + me < N;
    st[me].set_dim(n);
    for (int k = 0; k < n; ++k) st[me].xeval[k] = (x0 && live) ? x0[(e0 + me) * n + k] : 0.0;   // the start, by way of the trial-point slot
    powell_init(st[me], st[me].xeval);
    for (int k = 0; k < State::kMax; ++k) st[me].xeval[k] = 0.0;   // slots beyond N are evaluated too (and ignored): defined parameters
    const bool nd = live && powell_step_call((LdsState*)&st[me], 0.0);
    need[me] = nd ? 1 : 0;
  }
  __syncthreads();

  const LdsPar<State> lp{st};
  const typename Rank::FaceRow xrow{x, nullptr, ldx, e0, N};   // the faces' rows; machine slots beyond N read the last one
  // live machines as one word per round parity: the machines that want another evaluation OR their bit into the next round's
  // word (sixteen LDS reads per thread and round before)
  __shared__ int livew[2];
  if (tid == 0) {
    int m0 = 0;
    for (int e = 0; e < EV; ++e) m0 |= need[e] << e;
    livew[0] = m0;
    livew[1] = 0;
  }
  __syncthreads();
#ifdef PW_STAMPS   // timing-only diagnostic: cycles per phase summed over the rounds, written over fval[e0 .. e0+3] at the end
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp = __builtin_amdgcn_s_memtime();
#define PWS(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph[i] += t_ - tp; tp = t_; } while (0)
#else
#define PWS(i) do { } while (0)
#endif
  for (int round = 0; round < n * 1000 + 16; ++round) {
    const int live_mask = livew[round & 1];
    if (!live_mask) break;
    if (tid == 0) livew[(round + 1) & 1] = 0;     // last read a round ago; the barriers of the evaluation order this before the ORs below

    // the round's evaluation: fe = the objective value of this thread's machine, where that machine waits for one
    double fe = 0.0;
    PWS(0);
    if constexpr (REF) {
      __shared__ __attribute__((aligned(16))) typename Rank::PowellRefShared rs;
      tucker_fvec(sh, lp, cp4, tid);
      PWS(1);
      tucker_ref_eval(sh, rs, Wm, lp, live_mask, xrow, NoXhRow{}, tid, rk.pass_rank());
      PWS(2);
      if (me >= 0 && need[me]) fe = rs.err[me];
    } else {   // NLML_TD_ORDER_FAST (discarded in the other instantiation: its LDS is the reference pass's)
    if constexpr (Rank::kFixed) tucker_coef(sh, lp, cp4, tid);
    else tucker_coef_r(sh, lp, cp4, tid, rid);
    PWS(1);
    bool wide = true;
    if constexpr (Rank::kFixed) {
    __shared__ __attribute__((aligned(16))) TuckerFewShared few;
    if (__popc(live_mask) <= PW_FEW) {
      wide = false;
      // the tail of a workgroup's run: one to a few machines left (a face that needs 6,000 evaluations next to fifteen
      // that needed 1,500).  Their evaluations share ONE pass over Wm on the vector ALUs, bit-identical to the MFMA pass.
      int ev[PW_FEW];
      const float* xe[PW_FEW];
      int ne = 0;
      for (int mleft = live_mask; mleft; mleft &= mleft - 1) {
        const int e = __ffs(mleft) - 1;
        ev[ne] = e;
        xe[ne++] = xrow(e);
      }
      // the count is a compile-time parameter of the pass: its accumulators live in registers
#define NLML_FEW_CASE(K)                                                  \
  case K: {                                                               \
    int ek[K];                                                            \
    const float* xk[K];                                                   \
    for (int i = 0; i < K; ++i) { ek[i] = ev[i]; xk[i] = xe[i]; }         \
    tucker_few<K>(sh, few, Wm, xk, ek, tid);                              \
    break;                                                                \
  }
#ifndef PW_MFMA4_FROM
#define PW_MFMA4_FROM 2          // rounds with this many live machines or more (up to 4) take the 4x4x4 matrix pass
#endif
      if (ne >= PW_MFMA4_FROM) {
        int e4[4];
        const float* x4[4];
        for (int i = 0; i < 4; ++i) { e4[i] = ev[i < ne ? i : 0]; x4[i] = xe[i < ne ? i : 0]; }
        tucker_mfma4(sh, Wm, x4, e4, ne, tid);
      } else {
      switch (ne) {
        NLML_FEW_CASE(1) NLML_FEW_CASE(2) NLML_FEW_CASE(3) NLML_FEW_CASE(4)
        default: break;   // unreachable: ne <= PW_FEW
      }
      }
#undef NLML_FEW_CASE
      __syncthreads();
    }
    }
    if (wide) tucker_round16(sh, Wm, x, ldx, e0, N, tid, rk);
    PWS(2);
    if (me >= 0 && need[me]) fe = tucker_err(sh, me);
    }   // order
    if (me >= 0 && need[me]) {   // resume the state machines with their objective values
      PWS(4);
      const bool nd = powell_step_call((LdsState*)&st[me], fe);
      PWS(5);
      need[me] = nd ? 1 : 0;
      if (nd) atomicOr(&livew[(round + 1) & 1], 1 << me);
      PWS(6);
    }
    __syncthreads();
    PWS(3);
  }

  if (tid < EV && e0 + tid < N) {
    const int64_t f = e0 + tid;
    for (int k = 0; k < n; ++k) result[f * n + k] = st[tid].x[k];
    if (fval) fval[f] = st[tid].fval;
#ifdef PW_STAMPS
    for (int i = 0; i < 8; ++i) {   // lane 0 (machine 0) holds all eight sums
      const unsigned long long v = __shfl(ph[i], 0, 64);
      if (fval && tid == i) fval[f] = (double)v;
    }
#endif
    if (nfev) nfev[f] = st[tid].nfev;
    if (nit) nit[f] = st[tid].iter;
    if (status) status[f] = need[tid] ? PW_RUNNING : st[tid].status;
  }
}

// r_id == 5: the kernels of the shipped artefacts (the rank a constant); every other rank: the rank a run-time value
int launch_tucker_powell(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                         double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int r_id, int order,
                         void* stream) {
  if (N == 0) return 0;
  const bool ref = order == NLML_TD_ORDER_REFERENCE;
  auto* kernel = ref ? (r_id == 5 ? tucker_powell_kernel<NLML_TD_ORDER_REFERENCE, TdRank5> : tucker_powell_kernel<NLML_TD_ORDER_REFERENCE, TdRankDyn>)
                     : (r_id == 5 ? tucker_powell_kernel<NLML_TD_ORDER_FAST, TdRank5> : tucker_powell_kernel<NLML_TD_ORDER_FAST, TdRankDyn>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((N + EV - 1) / EV)), dim3(ref ? TR_NT : TNT), 0, reinterpret_cast<hipStream_t>(stream),
                     Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, r_id);
  return hip_launch_status();
}

}  // namespace nlml
