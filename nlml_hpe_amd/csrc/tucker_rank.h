// tucker_rank.h -- the TD path for ANY Tucker identity rank R = 1..NLML_TUCKER_RANK_MAX: Wm has 27 R rows, an evaluation 3 + R parameters.
//
// The identity rank is a knob of the reference's model (configs/config_TD_main.yaml tensor_decom_ranks.R_identity; the reference
// reads it from the artefact, TD_Inference.py:51, and runs objective / Test with 3 + R parameters whatever it is).  The kernels of
// tucker_common.h / tucker_ref.h / tucker_powell.hip are tuned for the shipped artefacts' R = 5 and stay the code they are; the
// pieces here take R at run time and share their arithmetic:
//   reference order  tucker_ref_pass itself (tucker_ref.h) with a run-time rank: np.einsum keeps its operation order when only the
//                    first extent changes, and the pairwise sum over the 1,404 residuals does not depend on R.  Bit-correct for every
//                    R; its shape (768 threads x 2 columns, three-slot ring) is the one tuned for 135 rows;
//   matrix cores     tucker_coef_r / tucker_mfma_r: x_hat = c^T Wm on v_mfma_f64_16x16x4_f64 with K = 27 R padded to a multiple of 4
//                    by zero coefficient rows, the same columns per lane and the same q-ascending chains as tucker_mfma (at R = 5 the
//                    same bits); no few-machine passes: every round of the Powell kernel is a 16-wide pass.
// The largest tables bound the workgroup: see the LDS budget at tucker_powell_r_kernel (tucker_rank.hip).
#pragma once
#include <hip/hip_runtime.h>

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
#pragma clang fp contract(off)   // numpy rounds b*w, + c, a*cos, + d separately (TD_Tester.py:25-28); the coefficient products too
  if (tid < EV * 9) {
    const int e = tid / 9, a = (tid % 9) / 3;
    const double v = cp4[0] * cr_cos(cp4[1] * par(e, a) + cp4[2]) + cp4[3];
    sh.fvec[e][a][tid % 3] = (double)(float)v;
  }
  __syncthreads();
  const int tq = 27 * rid, rows = (tq + 3) & ~3;
  for (int i = tid; i < rows * EV; i += TNT) {
    const int q = i / EV, e = i % EV;
    const int ui = q < tq ? q / 27 : rid - 1, j = (q / 9) % 3, k = (q / 3) % 3, l = q % 3;   // (a padding row reads a parameter that exists)
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

// tucker_ref_eval for a run-time rank and a table of RS::kMaxE evaluations per pass: the live machines go as the fewest passes that
// hold them, of about the same size (16 live, 7 per pass: 6 + 5 + 5).
template <typename SH, typename RS, typename ParT, typename XRow, typename XhRow>
__device__ __forceinline__ void tucker_ref_eval_r(const SH& sh, RS& rs, const float* __restrict__ Wm, const ParT par, int mask,
                                                  const XRow xrow, const XhRow xhrow, int tid, int rid) {
  const TrDynRank rank{rid};
  while (mask) {
    const int cnt = __popc(mask);
    const int passes = (cnt + RS::kMaxE - 1) / RS::kMaxE;
    const int take = (cnt + passes - 1) / passes;
    unsigned slots = 0;
    for (int i = 0; i < take; ++i) {
      slots |= (unsigned)(__ffs(mask) - 1) << (4 * i);
      mask &= mask - 1;
    }
#define NLML_RANK_PASS(K)                                                                                 \
  case K:                                                                                                 \
    if constexpr (K <= RS::kMaxE) tucker_ref_pass<K>(sh, rs, Wm, par, slots, xrow, xhrow, tid, rank);     \
    break;
    switch (take) {
      NLML_RANK_PASS(8) NLML_RANK_PASS(7) NLML_RANK_PASS(6) NLML_RANK_PASS(5)
      NLML_RANK_PASS(4) NLML_RANK_PASS(3) NLML_RANK_PASS(2) NLML_RANK_PASS(1)
      default: break;
    }
#undef NLML_RANK_PASS
  }
}

}  // namespace nlml
