// normalize_centroid.hip -- K1c: landmark normalisation by centroid and RMS radius (streaming kernel).
//
// Replaces Normalization_using_Centroid (helpers/FeatureExtractor.py:17-28) and the f32 cast of its callers (:101), in numpy's own
// operation order (centroid_ref.h), so the result is the reference's bit for bit.
//
// Unlike the IPD form, no output can be written before the whole face has been read, and the three centroid sums are chains of 468
// dependent f64 additions whose order is fixed.  A workgroup therefore takes a tile of 8 faces through LDS:
//   P0  the tile (8 x 5,616 B, contiguous in memory) -> LDS with coalesced 16-byte loads, all in flight together
//   P1  24 lanes of wave 0, one per (face, coordinate): the sequential centroid sum, reading LDS words f*1404 + 3i + c -- 28 f + c mod 32
//       is distinct for the 24 lanes, so the reads are conflict-free; the same lanes OR the magnitude bits for the "no face" test
//   P2  all lanes: n[i] = |a[i] - centroid|^2 of four faces at a time -> LDS (stride-3 word reads: conflict-free)
//   P3  16 lanes, one per (face, leaf): a leaf of numpy's pairwise sum (eight independent accumulators per lane); then one lane per
//       face: the two tree levels, / 468, sqrt
//   P4  all lanes: out = f32((a - centroid) / scale), an IEEE f64 divide per element, coalesced 16-byte non-temporal stores
// 60 KB of LDS per workgroup: two workgroups per CU, so one tile's chains run under the other's loads and stores.
// Algorithmic bytes per face: 5,616 read + 5,616 written = 11,232 B, as K1.
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"
#include "centroid_ref.h"

namespace nlml {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CN_F = NLML_F_REFERENCE;    // 1404 floats per face
constexpr int CN_F4 = CN_F / 4;           // 351 float4 per face: a float4 never straddles two faces
constexpr int CN_TILE = 8;                // faces per workgroup
constexpr int CN_PART = 4;                // faces whose n[] are in LDS at a time
constexpr int CN_THREADS = 256;
constexpr int CN_LOADS = (CN_TILE * CN_F4 + CN_THREADS - 1) / CN_THREADS;   // 11 float4 per lane
static_assert(CN_F == 3 * CN_LM && CN_F % 4 == 0 && CN_TILE % CN_PART == 0, "tile geometry");
static_assert(3 * CN_TILE <= 32, "P1's lanes are one 32-lane LDS group: the bank argument above");

__global__ __launch_bounds__(CN_THREADS) void normalize_centroid_kernel(const float* __restrict__ raw, int64_t B,
                                                                        float* __restrict__ out, uint8_t* __restrict__ valid,
                                                                        double* __restrict__ stats) {
  __shared__ __attribute__((aligned(16))) float s_raw[CN_TILE * CN_F];
  __shared__ double s_n[CN_PART * CN_LM];
  __shared__ double s_cen[CN_TILE * 3];
  __shared__ double s_leaf[CN_TILE * CN_LEAVES];
  __shared__ double s_scale[CN_TILE];
  __shared__ unsigned s_bits[CN_TILE * 3];
  __shared__ unsigned s_nz[CN_TILE];

  const int t = threadIdx.x;
  const int64_t face0 = (int64_t)blockIdx.x * CN_TILE;
  const int nf = B - face0 < CN_TILE ? (int)(B - face0) : CN_TILE;   // faces of this tile, >= 1 by the grid size
  const int n4 = nf * CN_F4;
  f32x4* const s_raw4 = reinterpret_cast<f32x4*>(s_raw);

  // P0: every load first, then the LDS writes
  {
    const f32x4* g = reinterpret_cast<const f32x4*>(raw + face0 * CN_F);
    f32x4 v[CN_LOADS];
#pragma unroll
    for (int k = 0; k < CN_LOADS; ++k) {
      const int i = k * CN_THREADS + t;
      v[k] = __builtin_nontemporal_load(g + (i < n4 ? i : n4 - 1));
    }
#pragma unroll
    for (int k = 0; k < CN_LOADS; ++k) {
      const int i = k * CN_THREADS + t;
      if (i < n4) s_raw4[i] = v[k];
    }
  }
  __syncthreads();

  // P1: one lane per (face, coordinate)
  if (t < 3 * nf) {
    const int f = t / 3, c = t - 3 * f;
    const float* p = s_raw + f * CN_F + c;
    double sum = 0.0;
    unsigned bits = 0u;
#pragma unroll 12
    for (int i = 0; i < CN_LM; ++i) {
      const float v = p[3 * i];
      bits |= __float_as_uint(v);
      sum += (double)v;
    }
    s_cen[t] = sum / (double)CN_LM;
    s_bits[t] = bits & 0x7fffffffu;
  }
  __syncthreads();

  for (int part = 0; part * CN_PART < nf; ++part) {   // (nf is the same for the whole workgroup: the barriers below are uniform)
    const int fbase = part * CN_PART;
    // P2
    for (int idx = t; idx < CN_PART * CN_LM; idx += CN_THREADS) {
      const int fl = idx / CN_LM, i = idx - fl * CN_LM, f = fbase + fl;
      if (f < nf) {
        const float* p = s_raw + f * CN_F + 3 * i;
        s_n[idx] = cn_sqnorm((double)p[0] - s_cen[3 * f], (double)p[1] - s_cen[3 * f + 1], (double)p[2] - s_cen[3 * f + 2]);
      }
    }
    __syncthreads();
    // P3: the leaves
    if (t < CN_PART * CN_LEAVES) {
      const int fl = t / CN_LEAVES, leaf = t - fl * CN_LEAVES;
      if (fbase + fl < nf) s_leaf[(fbase + fl) * CN_LEAVES + leaf] = np_leaf_sum(s_n + fl * CN_LM + CnTree::off(leaf), CnTree::len(leaf));
    }
    __syncthreads();
  }

  // P3: the tree above the leaves; the per-face outputs
  if (t < nf) {
    const double s = cn_scale(s_leaf + t * CN_LEAVES);
    const unsigned nz = s_bits[3 * t] | s_bits[3 * t + 1] | s_bits[3 * t + 2];
    s_scale[t] = s;
    s_nz[t] = nz;
    if (valid) valid[face0 + t] = nz ? 1 : 0;
    if (stats) {
      double* st = stats + (face0 + t) * 4;
      st[0] = s_cen[3 * t]; st[1] = s_cen[3 * t + 1]; st[2] = s_cen[3 * t + 2]; st[3] = s;
    }
  }
  __syncthreads();

  // P4: float4 j of a face holds columns 4j..4j+3, coordinates (j + e) % 3
  f32x4* o = reinterpret_cast<f32x4*>(out + face0 * CN_F);
#pragma unroll 2
  for (int i = t; i < n4; i += CN_THREADS) {
    const int f = i / CN_F4, j = i - f * CN_F4, ph = j % 3;
    const f32x4 v = s_raw4[i];
    const double s = s_scale[f];
    const double c0 = s_cen[3 * f + ph], c1 = s_cen[3 * f + (ph == 2 ? 0 : ph + 1)], c2 = s_cen[3 * f + (ph == 0 ? 2 : ph - 1)];
    f32x4 r;
    r[0] = (float)(((double)v[0] - c0) / s);
    r[1] = (float)(((double)v[1] - c1) / s);
    r[2] = (float)(((double)v[2] - c2) / s);
    r[3] = (float)(((double)v[3] - c0) / s);
    if (!s_nz[f]) r = f32x4{0.f, 0.f, 0.f, 0.f};   // the "no face" row stays all zero
    __builtin_nontemporal_store(r, o + i);
  }
}

int launch_normalize_centroid(const float* raw, int64_t B, float* out, uint8_t* valid, double* stats, void* stream) {
  if (B == 0) return 0;
  const dim3 grid((unsigned)((B + CN_TILE - 1) / CN_TILE)), block(CN_THREADS);
  hipLaunchKernelGGL(normalize_centroid_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), raw, B, out, valid, stats);
  return hip_launch_status();
}

}  // namespace nlml
