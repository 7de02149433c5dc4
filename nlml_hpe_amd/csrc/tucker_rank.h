// tucker_rank.h -- the TD path for ANY Tucker identity rank R = 1..NLML_TUCKER_RANK_MAX: Wm has 27 R rows, an evaluation 3 + R parameters.
//
// The identity rank is a knob of the reference's model (configs/config_TD_main.yaml tensor_decom_ranks.R_identity; the reference
// reads it from the artefact, TD_Inference.py:51, and runs objective / Test with 3 + R parameters whatever it is).  The kernels of
// tucker_common.h / tucker_ref.h are tuned for the shipped artefacts' R = 5 and stay the code they are; the pieces here take R at
// run time and share their arithmetic:
//   reference order  tucker_ref_pass itself (tucker_ref.h) with a run-time rank: np.einsum keeps its operation order when only the
//                    first extent changes, and the pairwise sum over the 1,404 residuals does not depend on R.  Bit-correct for every
//                    R; its shape (768 threads x 2 columns, three-slot ring) is the one tuned for 135 rows;
//   matrix cores     tucker_coef_r / tucker_mfma_r: x_hat = c^T Wm on v_mfma_f64_16x16x4_f64 with K = 27 R padded to a multiple of 4
//                    by zero coefficient rows, the same columns per lane and the same q-ascending chains as tucker_mfma (at R = 5 the
//                    same bits); no few-machine passes: every round of the Powell kernel is a 16-wide pass.
// The largest tables bound the workgroup: see the LDS budget at tucker_powell_kernel (tucker_powell.hip).
// Below them: the rank traits and the functors over which tucker_objective.hip and tucker_powell.hip write every kernel once.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "powell.h"
#include "tucker_common.h"
#include "tucker_ref.h"

namespace nlml {

constexpr int TRK_RMAX = NLML_TUCKER_RANK_MAX;   // 16
constexpr int TRK_QMAX = 27 * TRK_RMAX;          // 432 rows of Wm, a multiple of 4
static_assert(TRK_QMAX % 4 == 0, "K of the largest rank needs no padding row");
static_assert(PW_NMAX == 3 + TRK_RMAX, "powell.h's largest state and the largest rank go together");

typedef TuckerSharedT<TRK_QMAX> TuckerSharedR;   // matrix-core order: coefficient table of the largest rank (54 KB), f-vectors, partial sums
struct TuckerFvecShared {                        // reference order: the f-vectors alone (its passes keep their own tables)
  double fvec[EV][3][3];
};
template <int MAXE>
using TuckerRefSharedR = TuckerRefSharedT<MAXE, TRK_RMAX + 9>;   // factor rows for up to 16 + 9 factors

// tucker_coef for 27 R rows (same expressions: at R = 5 the same table)
template <typename ParT>
__device__ __forceinline__ void tucker_coef_r(TuckerSharedR& sh, const ParT& par, const double (&cp4)[4], int tid, int rid) {
#pragma clang fp contract(off)   // the coefficient products are rounded one by one
  tucker_coef_fvec(sh, par, cp4, tid);
  const int tq = 27 * rid, rows = (tq + 3) & ~3;
  for (int i = tid; i < rows * EV; i += TNT) {
    const int q = i / EV, e = i % EV;
    const int ui = q < tq ? tucker_q_i(q) : rid - 1, j = tucker_q_j(q), k = tucker_q_k(q), l = tucker_q_l(q);   // (a padding row reads a parameter that exists)
    const double c = ((par(e, 3 + ui) * sh.fvec[e][0][j]) * sh.fvec[e][1][k]) * sh.fvec[e][2][l];
    sh.coef[q][e] = q < tq ? c : 0.0;
  }
  __syncthreads();
}

// tucker_mfma for 27 R rows: (27 R + 3) / 4 K steps through a three-slot ring.  Every load stays inside Wm: steps past the end re-read
// the last one, the padding rows re-read row 27 R - 1 (their coefficients are zero).
__device__ __forceinline__ void tucker_mfma_r(TuckerSharedR& sh, const float* __restrict__ Wm, int tid, int rid, f64x4 (&acc)[MBW]) {
  const int lane = tid & 63, wv = tid >> 6;
  const int kq = lane >> 4, col = lane & 15;
  const int tq = 27 * rid, tqs = (tq + 3) >> 2;
  const float* wbase = Wm + tcol0(wv);
#pragma unroll
  for (int mb = 0; mb < MBW; ++mb) acc[mb] = f64x4{0.0, 0.0, 0.0, 0.0};
  auto row_off = [&](int qs) {
    const int q = 4 * (qs < tqs ? qs : tqs - 1) + kq;
    return (size_t)(q < tq ? q : tq - 1) * TM;
  };
  float wr[3][MBW];
  load11(wbase + row_off(0), col, wr[0]);
  load11(wbase + row_off(1), col, wr[1]);
  auto step = [&](int qs, int slot) {
    load11(wbase + row_off(qs + 2), col, wr[(slot + 2) % 3]);
    const double a = sh.coef[4 * qs + kq][col];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb)
      acc[mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)wr[slot][mb], acc[mb], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
#pragma unroll 1
  for (int qs0 = 0; qs0 < tqs; qs0 += 3) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (qs0 + r < tqs) step(qs0 + r, r);
  }
}

// ---- rank traits: what the TD kernels (tucker_objective.hip, tucker_powell.hip) let the rank choose -------------------------------
// TdRank5: the shipped artefacts' identity rank, a constant of the type -- the tuned code above and below it is instantiated as it
// always was.  TdRankDyn: a run-time rank 1..16.  Each names its Powell state, its LDS tables and its matrix-core bodies.
template <bool INDEXED, bool CLAMPED>
struct XRow;   // (below)
struct TdRank5 {
  static constexpr bool kFixed = true;          // matrix cores: tucker_coef + tucker_mfma, and the Powell kernel's few-machine passes
  static constexpr int kFastWorkgroups = 2;     // __launch_bounds__ of the matrix-core Powell kernel: two workgroups per CU
  typedef PowellState State;
  typedef TuckerShared Shared;                  // matrix-core order
  typedef TuckerShared FvecShared;              // reference order: only fvec is used; the type stays (LDS offsets inside the tuned pass)
  typedef TuckerRefShared ObjRefShared;
  typedef TuckerRefShared PowellRefShared;
  typedef XRow<false, true> FaceRow;            // the Powell kernel's x rows: one per face, no index
  static __device__ __forceinline__ TdRank5 make(int) { return {}; }
  typedef std::integral_constant<int, PW_N> NPar;   // parameters per evaluation: a constant (reads as an int)
  __device__ __forceinline__ constexpr NPar npar() const { return {}; }
  __device__ __forceinline__ TrFixedRank<5> pass_rank() const { return {}; }
};
struct TdRankDyn {
  static constexpr bool kFixed = false;         // matrix cores: tucker_coef_r + tucker_mfma_r, every round of the Powell kernel 16 wide
  static constexpr int kFastWorkgroups = 1;
  typedef PowellStateN State;
  typedef TuckerSharedR Shared;
  typedef TuckerFvecShared FvecShared;
  typedef TuckerRefSharedR<8> ObjRefShared;
  typedef TuckerRefSharedR<7> PowellRefShared;  // next to 16 machines of 19 parameters eight evaluations do not fit: tucker_powell_kernel
  typedef XRow<true, true> FaceRow;             // with the (null) index member: the registers the run-time-rank passes were allocated with; without it passes of 6 and 7 spill
  int rid;
  static __device__ __forceinline__ TdRankDyn make(int rid) { return {rid}; }
  typedef int NPar;
  __device__ __forceinline__ int npar() const { return 3 + rid; }
  __device__ __forceinline__ TrDynRank pass_rank() const { return {rid}; }
};

// this thread's cosine row (a,b,c,d), TD_Tester.py:26 (threads < 144; zeros beyond).  Row (tid % 9) / 3 * 3 + tid % 3 is row tid % 9;
// the long spelling stays until these kernels may change: the short one takes eleven instructions out of every prologue
// (profiles/np_sum_one_definition.md).
__device__ __forceinline__ void load_cos_rows(const double* __restrict__ cosp, int tid, double (&cp4)[4]) {
  cp4[0] = cp4[1] = cp4[2] = cp4[3] = 0.0;
  if (tid < EV * 9) {
    const double* c4 = cosp + ((tid % 9) / 3 * 3 + tid % 3) * 4;
    cp4[0] = c4[0]; cp4[1] = c4[1]; cp4[2] = c4[2]; cp4[3] = c4[3];
  }
}

// par(e, k) from global memory: evaluations beyond the batch repeat the last one
template <typename Rank>
struct GlobalPar {
  const double* p;   // params of this block's first evaluation
  int64_t left;      // evaluations available from there (>= 1)
  [[no_unique_address]] typename Rank::NPar n;   // parameters per evaluation
  __device__ __forceinline__ double operator()(int e, int k) const {
    return gload<double>(p + (e < left ? e : left - 1) * n + k);
  }
};

// Row functors of the reference-order pass (passed by value into the non-inlined pass).  A member a variant does not use is Absent:
// each instantiation carries the members, and evaluates the expression, it needs -- a run-time test here lands in the tuned pass.
struct Absent {
  template <typename T>
  constexpr Absent(T) {}   // (takes and drops what the member would have held: one brace list builds every variant)
};
// x row of machine slot `slot`.  INDEXED: through x_index where given; CLAMPED: slots beyond N read the last row
template <bool INDEXED, bool CLAMPED>
struct XRow {
  const float* x;
  [[no_unique_address]] std::conditional_t<INDEXED, const int32_t*, Absent> x_index;
  int64_t ldx, e0;
  [[no_unique_address]] std::conditional_t<CLAMPED, int64_t, Absent> N;
  __device__ __forceinline__ const float* operator()(int slot) const {
    int64_t n = e0 + slot;
    if constexpr (CLAMPED) n = n < N ? n : N - 1;
    if constexpr (INDEXED) return x + (x_index ? (int64_t)x_index[n] : n) * ldx;
    else return x + n * ldx;
  }
};
struct XhRow {
  double* x_hat;
  int64_t e0;
  __device__ __forceinline__ double* operator()(int slot) const { return x_hat ? x_hat + (e0 + slot) * TM : (double*)nullptr; }
};
struct NoXhRow {
  static constexpr double* x_hat = nullptr;   // (the stamp build of the pass looks for this member)
  __device__ __forceinline__ double* operator()(int) const { return nullptr; }
};

}  // namespace nlml
