// centroid_ref.h -- the operation order of Normalization_using_Centroid (helpers/FeatureExtractor.py:17-28) as numpy evaluates it,
// shared by the device kernel (normalize_centroid.hip) and the host restatement (nlml_normalize_centroid_host, abi.cpp).
//
//   centroid = np.mean(a, axis=0)            0.0 + a[0][c] + a[1][c] + ... row by row (axis 0 of a C-ordered array: no pairwise routine),
//                                            then / 468.0
//   d = a - centroid;  q = d ** 2            each product rounded on its own
//   n = np.sum(q, axis=1)                    (q0 + q1) + q2
//   m = np.mean(n)                           numpy's pairwise sum over 468 elements, then / 468.0:
//                                            468 -> 232 + 236 -> (112 + 120) + (112 + 124); a leaf: eight accumulators seeded from its
//                                            first eight elements, stride 8, ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), remainder in sequence
//   out = f32(d / sqrt(m))                   IEEE f64 square root and divide, one rounding to f32 (:101)
//
// Nothing here may be contracted into an fma: the functions that multiply switch contraction off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_CN_HD __host__ __device__
#else
#define NLML_CN_HD
#endif

namespace nlml {

constexpr int CN_LM = 468;       // landmarks per face
constexpr int CN_LEAVES = 4;     // leaves of numpy's pairwise tree for 468 elements

// numpy's pairwise sum splits a range of more than 128 elements at n/2 rounded down to a multiple of 8
constexpr int cn_split(int n) { return n / 2 - (n / 2) % 8; }
// first element of leaf 0..3 (4: one past the last); constexpr functions, so device code may index them at run time
constexpr int cn_leaf_off(int leaf) {
  return leaf == 0 ? 0
       : leaf == 1 ? cn_split(cn_split(CN_LM))
       : leaf == 2 ? cn_split(CN_LM)
       : leaf == 3 ? cn_split(CN_LM) + cn_split(CN_LM - cn_split(CN_LM))
                   : CN_LM;
}
constexpr int cn_leaf_len(int leaf) { return cn_leaf_off(leaf + 1) - cn_leaf_off(leaf); }
static_assert(cn_leaf_off(1) == 112 && cn_leaf_off(2) == 232 && cn_leaf_off(3) == 344, "468 -> (112 + 120) + (112 + 124)");
static_assert(cn_leaf_len(0) == 112 && cn_leaf_len(1) == 120 && cn_leaf_len(2) == 112 && cn_leaf_len(3) == 124, "leaf lengths");
static_assert(cn_split(CN_LM) > 128 && CN_LM - cn_split(CN_LM) > 128, "both halves split once more");
static_assert(cn_leaf_len(1) <= 128 && cn_leaf_len(3) <= 128 && cn_leaf_len(0) >= 8, "a leaf: 8..128 elements, not split further");

// one leaf of numpy's pairwise sum, 8 <= n <= 128
NLML_CN_HD inline double cn_pairwise_leaf(const double* a, int n) {
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i + 0]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

// np.sum(d ** 2, axis=1) of one landmark: three products rounded on their own, then (q0 + q1) + q2
NLML_CN_HD inline double cn_sqnorm(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  const double q0 = dx * dx, q1 = dy * dy, q2 = dz * dz;
  return (q0 + q1) + q2;
}

// the four leaf sums -> the RMS radius: sqrt(pairwise / 468.0)
NLML_CN_HD inline double cn_scale(const double* leaf_sums) {
  const double m = ((leaf_sums[0] + leaf_sums[1]) + (leaf_sums[2] + leaf_sums[3])) / (double)CN_LM;
  return sqrt(m);
}

// "no face": every landmark coordinate is +0 or -0 (the extractor's sentinel row, FeatureExtractor.py:105-106)
inline bool cn_all_zero(const float* raw) {
  uint32_t bits = 0;
  for (int e = 0; e < 3 * CN_LM; ++e) {
    uint32_t u;
    memcpy(&u, raw + e, 4);
    bits |= u;
  }
  return (bits & 0x7fffffffu) == 0;
}

// One face on the host: raw f32[468*3] -> out f32[468*3], stats (centroid x, y, z, scale); returns valid (0: the sentinel row, out = 0).
inline int cn_face_host(const float* raw, float* out, double* stats) {
  double cen[3];
  for (int c = 0; c < 3; ++c) {
    double sum = 0.0;
    for (int i = 0; i < CN_LM; ++i) sum += (double)raw[3 * i + c];
    cen[c] = sum / (double)CN_LM;
  }
  double n[CN_LM], leaf[CN_LEAVES];
  for (int i = 0; i < CN_LM; ++i)
    n[i] = cn_sqnorm((double)raw[3 * i] - cen[0], (double)raw[3 * i + 1] - cen[1], (double)raw[3 * i + 2] - cen[2]);
  for (int l = 0; l < CN_LEAVES; ++l) leaf[l] = cn_pairwise_leaf(n + cn_leaf_off(l), cn_leaf_len(l));
  const double s = cn_scale(leaf);
  const int valid = cn_all_zero(raw) ? 0 : 1;
  for (int i = 0; i < CN_LM; ++i)
    for (int c = 0; c < 3; ++c) out[3 * i + c] = valid ? (float)(((double)raw[3 * i + c] - cen[c]) / s) : 0.0f;
  if (stats) { stats[0] = cen[0]; stats[1] = cen[1]; stats[2] = cen[2]; stats[3] = s; }
  return valid;
}

}  // namespace nlml
