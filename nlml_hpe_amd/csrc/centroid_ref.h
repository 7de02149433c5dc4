// centroid_ref.h -- the operation order of Normalization_using_Centroid (helpers/FeatureExtractor.py:17-28) as numpy evaluates it,
// shared by the device kernel (normalize_centroid.hip) and the host restatement (nlml_normalize_centroid_host, abi.cpp).
//
//   centroid = np.mean(a, axis=0)            0.0 + a[0][c] + a[1][c] + ... row by row (axis 0 of a C-ordered array: no pairwise routine),
//                                            then / 468.0
//   d = a - centroid;  q = d ** 2            each product rounded on its own
//   n = np.sum(q, axis=1)                    (q0 + q1) + q2
//   m = np.mean(n)                           numpy's pairwise sum over 468 elements (np_sum.h: four leaves, (112 + 120) + (112 + 124)),
//                                            then / 468.0
//   out = f32(d / sqrt(m))                   IEEE f64 square root and divide, one rounding to f32 (:101)
//
// Nothing here may be contracted into an fma: the functions that multiply switch contraction off.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "np_sum.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_CN_HD __host__ __device__
#else
#define NLML_CN_HD
#endif

namespace nlml {

constexpr int CN_LM = 468;       // landmarks per face
typedef NpTree<CN_LM> CnTree;    // numpy's pairwise tree for 468 elements (np_sum.h): 4 leaves, (112 + 120) + (112 + 124)
constexpr int CN_LEAVES = CnTree::leaves;
static_assert(CnTree::balanced, "np_tree_sum adds the leaves as a balanced tree");

// np.sum(d ** 2, axis=1) of one landmark: three products rounded on their own, then (q0 + q1) + q2
NLML_CN_HD inline double cn_sqnorm(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  const double q0 = dx * dx, q1 = dy * dy, q2 = dz * dz;
  return (q0 + q1) + q2;
}

// the leaf sums -> the RMS radius: sqrt(pairwise / 468.0)
NLML_CN_HD inline double cn_scale(const double* leaf_sums) {
  const double m = np_tree_sum<CN_LEAVES>(leaf_sums) / (double)CN_LM;
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
  for (int l = 0; l < CN_LEAVES; ++l) leaf[l] = np_leaf_sum(n + CnTree::off(l), CnTree::len(l));
  const double s = cn_scale(leaf);
  const int valid = cn_all_zero(raw) ? 0 : 1;
  for (int i = 0; i < CN_LM; ++i)
    for (int c = 0; c < 3; ++c) out[3 * i + c] = valid ? (float)(((double)raw[3 * i + c] - cen[c]) / s) : 0.0f;
  if (stats) { stats[0] = cen[0]; stats[1] = cen[1]; stats[2] = cen[2]; stats[3] = s; }
  return valid;
}

}  // namespace nlml
