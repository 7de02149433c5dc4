// encoder_heads_f16x2_tailws.hip -- the strict-fast mode's streamed tail (encoder_heads_f16x2_tailws_dev.h: what it is, its measurements
// and its bits) as a launch of its own behind the trunk-only launch of the eight-wave kernel: workgroup g takes the 32-face blocks
// 8g .. 8g + 7 of the hand-over buffer.
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"
#include "encoder_heads_f16x2_tailws_dev.h"

namespace nlml {
namespace hx {

__global__ __launch_bounds__(512) void tail_ws_kernel(TwArgs a) {
  __shared__ __attribute__((aligned(1024))) char lds[TW_LDS];
  tail_ws_body(a, (int64_t)blockIdx.x * 8, lds);
}

}  // namespace hx

int launch_tail_ws(const void* blob, const void* h3, int64_t nfb, int64_t B, float* out, float* latent, void* stream) {
  hx::TwArgs a;
  a.blob = blob; a.h3 = reinterpret_cast<const hx::u4*>(h3); a.out = out; a.latent = latent; a.B = B; a.nfb = nfb;
  hipLaunchKernelGGL(hx::tail_ws_kernel, dim3((unsigned)((nfb + 7) / 8)), dim3(512), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hip_launch_status();
}

}  // namespace nlml
