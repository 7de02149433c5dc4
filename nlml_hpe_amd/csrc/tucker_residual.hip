// tucker_residual.hip -- K11: expand a Tucker model and compare it with the tensor in ONE pass (tensorly's tucker_to_tensor and the
// reconstruction error of TD_main.py:221-224).  X f32[I,ny,np,nr,M] is read once; nothing of its size is written unless X_hat is asked
// for.  The operation order, per element and for the sums, is tucker_residual_ref.h's; the lane body is that header's, so the host form
// (nlml_tucker_residual_host) returns the same bits.
//
// A wave owns one identity and one group of 64 columns: a lane per column, so the 64 lanes read 256 consecutive bytes of every cell's
// row.  The lane first builds v = W x_1 U_id[i] for its column (ry rp rr f64 values, 27 at the shipped ranks, in registers; W and the
// factors are small and stay in cache), then walks the cells in row-major order with the yaw, pitch and roll contractions nested: about
// rr + 3 + rp rr / nr + ry rp rr / (np nr) f64 operations per element of X.  The walk issues the loads of eight cells together into
// one of two register buffers while the other buffer's cells are computed: with one load in flight per wave the kernel waited on
// memory latency at a third of the HBM rate (profiles/tucker_residual.md).  A workgroup is one wave (nothing is shared between waves),
// so the identity, the group and every factor entry are scalar values.  No floating-point atomics: the wave's two sums go to the
// caller's workspace and a second launch of one workgroup adds them (tucker_residual_ref.h, steps 1 and 2).  Every offset is int64_t.
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"
#include "tucker_residual_ref.h"

namespace nlml {

constexpr unsigned TR_MAX_GRID = 0x7fffffffu;

template <int RY, int RP, int RR, bool HAS_X, bool HAS_XHAT>
__global__ __launch_bounds__(TR_LANES) void tucker_residual_kernel(TrArgs a, int64_t G, int64_t items, double* __restrict__ P) {
  const int lane = threadIdx.x;
  for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int64_t i = w / G, g = w - i * G;
    const int64_t m = g * TR_LANES + lane;
    double s = 0.0, q = 0.0;
    if (m < a.M) tr_lane<RY, RP, RR, HAS_X, HAS_XHAT>(a, i, m, s, q);
    if (HAS_X) {
#pragma unroll
      for (int h = TR_LANES / 2; h >= 1; h /= 2) {
        s = s + __shfl_down(s, h, TR_LANES);
        q = q + __shfl_down(q, h, TR_LANES);
      }
      if (lane == 0) {
        P[2 * w] = s;
        P[2 * w + 1] = q;
      }
    }
  }
}

__global__ __launch_bounds__(TR_RED_THREADS) void tucker_residual_reduce_kernel(const double* __restrict__ P, int64_t I, int64_t G,
                                                                                double* __restrict__ res_id, double* __restrict__ sums) {
  __shared__ double ts[TR_RED_THREADS], tq[TR_RED_THREADS];
  const int t = threadIdx.x;
  double as, aq;
  tr_reduce_thread(P, I, G, t, res_id, as, aq);
  ts[t] = as;
  tq[t] = aq;
  __syncthreads();
  for (int h = TR_RED_THREADS / 2; h >= 1; h /= 2) {
    if (t < h) {
      ts[t] = ts[t] + ts[t + h];
      tq[t] = tq[t] + tq[t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    sums[0] = ts[0];
    sums[1] = tq[0];
  }
}

namespace {
struct TrLaunch {
  const TrArgs& a;
  int64_t G, items;
  double* P;
  dim3 grid;
  hipStream_t st;
  template <int RY, int RP, int RR> void run() {
    if (a.X && a.xhat)
      hipLaunchKernelGGL((tucker_residual_kernel<RY, RP, RR, true, true>), grid, dim3(TR_LANES), 0, st, a, G, items, P);
    else if (a.X)
      hipLaunchKernelGGL((tucker_residual_kernel<RY, RP, RR, true, false>), grid, dim3(TR_LANES), 0, st, a, G, items, P);
    else
      hipLaunchKernelGGL((tucker_residual_kernel<RY, RP, RR, false, true>), grid, dim3(TR_LANES), 0, st, a, G, items, P);
  }
};
}  // namespace

size_t tucker_residual_workspace_bytes(int64_t I, int64_t M) { return tr_workspace_bytes(I, M); }

int launch_tucker_residual(const TrArgs& a, int ry, int rp, int rr, double* sums, double* res_id, void* ws, void* stream) {
  const int64_t G = tr_groups(a.M), items = a.I * G;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(items < (int64_t)TR_MAX_GRID ? (unsigned)items : TR_MAX_GRID);
  tr_dispatch(ry, rp, rr, TrLaunch{a, G, items, static_cast<double*>(ws), grid, st});
  if (const int rc = hip_launch_status()) return rc;
  if (!a.X) return 0;
  hipLaunchKernelGGL(tucker_residual_reduce_kernel, dim3(1), dim3(TR_RED_THREADS), 0, st, static_cast<const double*>(ws), a.I, G, res_id, sums);
  return hip_launch_status();
}

}  // namespace nlml
