// encoder_train_dev.h -- the device pieces of THE GEMM ORDER (encoder_train_ref.h) that K9 (encoder_train.hip) and K10
// (heads_train.hip) share: the operand loads, a wave's MFMA chain, the partial tiles' meeting in LDS and the halving tree.
#pragma once
#include <hip/hip_runtime.h>

#include "encoder_train_ref.h"

namespace nlml {

typedef float et_f32x16 __attribute__((ext_vector_type(16)));
typedef float et_f32x4 __attribute__((ext_vector_type(4)));

constexpr int ET_RS = 40;   // LDS row stride of a partial tile: the two half-waves of a store land on disjoint banks

// four consecutive k of a k-contiguous operand row (NULL: a row beyond the matrix); vec: row + k is 16-byte aligned
__device__ __forceinline__ et_f32x4 et_ld_kc(const float* row, int k, int K, bool vec) {
  et_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!row) return v;
  if (vec && k + 3 < K) return *reinterpret_cast<const et_f32x4*>(row + k);
  if (k < K) v.x = row[k];
  if (k + 1 < K) v.y = row[k + 1];
  if (k + 2 < K) v.z = row[k + 2];
  if (k + 3 < K) v.w = row[k + 3];
  return v;
}
// four consecutive k of one column of a k-outer operand (col = base + column, NULL: beyond the matrix); rows: the gather of k
__device__ __forceinline__ et_f32x4 et_ld_ko(const float* col, int64_t ld, const int32_t* rows, int k, int K) {
  et_f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (!col) return v;
  if (k < K) v.x = col[(int64_t)(rows ? rows[k] : k) * ld];
  if (k + 1 < K) v.y = col[(int64_t)(rows ? rows[k + 1] : k + 1) * ld];
  if (k + 2 < K) v.z = col[(int64_t)(rows ? rows[k + 2] : k + 2) * ld];
  if (k + 3 < K) v.w = col[(int64_t)(rows ? rows[k + 3] : k + 3) * ld];
  return v;
}

struct EtOperand { const float* p; int64_t ld; const int32_t* rows; bool vec; };   // p: this lane's row (k-contiguous) or column (k-outer)

template <bool KC> __device__ __forceinline__ et_f32x4 et_ld(const EtOperand& o, int k, int K) {
  if constexpr (KC) return et_ld_kc(o.p, k, K, o.vec);
  else return et_ld_ko(o.p, o.ld, o.rows, k, K);
}

// this wave's share of a tile's chains: acc += sum over its super-chunks, in the order of encoder_train_ref.h
template <bool A_KC, bool B_KC>
__device__ __forceinline__ void et_chain(et_f32x16& acc, const EtOperand& a, const EtOperand& b, int K, int wave, int h) {
  int s0, s1;
  et_wave_range(K, wave, &s0, &s1);
  if (s0 >= s1) return;
  et_f32x4 av[2], bv[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    av[u] = et_ld<A_KC>(a, ET_SUPER * s0 + 8 * u + 4 * h, K);
    bv[u] = et_ld<B_KC>(b, ET_SUPER * s0 + 8 * u + 4 * h, K);
  }
  for (int s = s0; s < s1; ++s) {
    et_f32x4 an[2], bn[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {   // the next super-chunk (beyond K: zeros, nothing is read)
      an[u] = et_ld<A_KC>(a, ET_SUPER * (s + 1) + 8 * u + 4 * h, K);
      bn[u] = et_ld<B_KC>(b, ET_SUPER * (s + 1) + 8 * u + 4 * h, K);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][j], bv[u][j], acc, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 2; ++u) { av[u] = an[u]; bv[u] = bn[u]; }
  }
}

// the waves' partial tiles -> LDS; after the barrier et_tile_total(red, e) is element e = 32 i + j of the tile
__device__ __forceinline__ void et_store_partial(float (*red)[ET_TILE * ET_RS], const et_f32x16& acc, int wave, int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int q = 0; q < 16; ++q) red[wave][((q & 3) + 8 * (q >> 2) + 4 * h) * ET_RS + j] = acc[q];
  __syncthreads();
}
__device__ __forceinline__ float et_tile_total(float (*red)[ET_TILE * ET_RS], int e) {
  const int at = (e >> 5) * ET_RS + (e & 31);
  float t = red[0][at];
#pragma unroll
  for (int w = 1; w < ET_WAVES; ++w) t = t + red[w][at];
  return t;
}
// halving tree over the workgroup's slots (every thread has written s[threadIdx.x]); the total is s[0] after it
template <class T, int SLOTS> __device__ __forceinline__ T et_tree(T* s) {
  __syncthreads();
  for (int stride = SLOTS / 2; stride >= 1; stride >>= 1) {
    if ((int)threadIdx.x < stride) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + stride];
    __syncthreads();
  }
  return s[0];
}

}  // namespace nlml
