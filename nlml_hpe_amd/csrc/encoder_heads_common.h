// encoder_heads_common.h -- the pieces of the K2 kernels that do not depend on the operand precision, shared by the f32 kernel
// (encoder_heads.hip), the split-f16 kernels (encoder_heads_f16x2_dev.h) and the bf16 kernel (encoder_heads_bf16_dev.h): f32 vector
// types, the activation codes, the activation itself, the bias as the accumulators' initial value and the "no face" mask write.
#pragma once
#include <hip/hip_runtime.h>

namespace nlml {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2 };

template <int ACT>
__device__ __forceinline__ float activate(float v) {
  if (ACT == ACT_RELU) return v < 0.0f ? 0.0f : v;   // NaN propagates like torch.relu (fmaxf would swallow it)
  if (ACT == ACT_TANH) return tanhf(v);
  return v;
}

// acc[nb][fb]: neuron block nb x face block fb.  The bias depends on the neuron only.
template <int NB, int NFB>
__device__ __forceinline__ void load_bias(f32x16 (&acc)[NB][NFB], const f32x4* __restrict__ b, int h) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const f32x4* p = b + (nb * 2 + h) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 v = p[q];
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        acc[nb][fb][4 * q + 0] = v[0];
        acc[nb][fb][4 * q + 1] = v[1];
        acc[nb][fb][4 * q + 2] = v[2];
        acc[nb][fb][4 * q + 3] = v[3];
      }
    }
  }
}

// The "no face" mask of layer 0's staging: an all-zero feature row == no face (FeatureExtractor.py:105-106).  LANES consecutive
// threads stage one row (`nzbits`: the OR of the magnitude bits of what this thread staged; `part` = tid % LANES: which part of the
// row, passed in because the callers hold it for their column already); the first of them, if the row is `live` (inside the
// batch), writes valid[row].  Every lane of the wave calls it (the ballot).
template <int LANES>
__device__ __forceinline__ void write_valid(uint8_t* valid, unsigned nzbits, int part, int lane, bool live, int64_t row) {
  static_assert(LANES > 0 && LANES < 64 && (LANES & (LANES - 1)) == 0, "a power-of-two group of lanes inside one wave");
  const unsigned long long m = __ballot(nzbits != 0u);
  if (part == 0 && live) valid[row] = ((m >> (lane & (64 - LANES))) & ((1ull << LANES) - 1)) ? 1 : 0;
}

}  // namespace nlml
