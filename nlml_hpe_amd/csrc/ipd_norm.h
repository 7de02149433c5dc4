// ipd_norm.h -- the arithmetic of Read_Landmarks_and_Normalizing_using_IPD (helpers/FeatureExtractor.py:30-66) and the f32 cast of its
// callers (:101), stated ONCE: out = f32((f64(v) - f64(lm[1][c])) / ipd), ipd = ||lm[33] - lm[263]||_2 in f64, 1e-6 when exactly 0.
// Shared by K1 (normalize_ipd.hip), by every K2 kernel that normalises while it stages x (encoder_heads.hip, encoder_heads_f16x2.hip,
// encoder_heads_f16x2_w8.hip, encoder_heads_f16x2_small.hip, encoder_heads_f16x2_rescue.h, encoder_heads_bf16_w8.hip) and by a host
// program (tests/native/ipd_norm_host.cpp): fused == K2(K1(raw)) bit for bit because all of them run these functions.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_IPD_HD __host__ __device__ __forceinline__
#else
#define NLML_IPD_HD inline
#endif

namespace nlml {

constexpr int IPD_LM_REF = 1;      // nose tip: the origin of the normalised coordinates (:85-86)
constexpr int IPD_LM_EYE_A = 33;   // outer eye corners: ipd is their distance (:38-46)
constexpr int IPD_LM_EYE_B = 263;
constexpr int ipd_col(int l, int c) { return 3 * l + c; }   // column of landmark l, coordinate c (0 x, 1 y, 2 z) in a face row

// n / d correctly rounded in f64 from y = RN(1/d) (Markstein): q = n*y, r = n - q*d exactly by fma, q' = q + r*y -- three multiply-adds
// per element instead of a ~35-instruction IEEE division sequence, equal to IEEE n / d for these operands (tests/test_ipd_exact_host.py).
// The residual is taken NEGATED, r = -(n - q d), and subtracted: same value, same instructions, but a zero numerator keeps its sign --
// fma(-q, d, n) is +0 for n = -0 and fma(+0, y, -0) = +0, where IEEE division gives -0 (family E of the exact tests).
// The three links are functions of their own for the kernel that issues one link per MFMA slot (lw_norm2, encoder_heads_f16x2.hip).
NLML_IPD_HD double div_ipd_quotient(double n, double y) { return n * y; }
NLML_IPD_HD double div_ipd_residual(double q, double d, double n) { return fma(q, d, -n); }
NLML_IPD_HD double div_ipd_correct(double q, double r, double y) { return fma(-r, y, q); }
NLML_IPD_HD double div_ipd(double n, double d, double y) {
  const double q = div_ipd_quotient(n, y);
  return div_ipd_correct(q, div_ipd_residual(q, d, n), y);
}

// ipd of the face row p (== np.linalg.norm: sqrt of an fma-chained ddot, as the reference's BLAS evaluates it)
NLML_IPD_HD double ipd_length(const float* p) {
  const double dx = (double)p[ipd_col(IPD_LM_EYE_A, 0)] - (double)p[ipd_col(IPD_LM_EYE_B, 0)];
  const double dy = (double)p[ipd_col(IPD_LM_EYE_A, 1)] - (double)p[ipd_col(IPD_LM_EYE_B, 1)];
  const double dz = (double)p[ipd_col(IPD_LM_EYE_A, 2)] - (double)p[ipd_col(IPD_LM_EYE_B, 2)];
  const double d = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
  return d == 0.0 ? 1e-6 : d;   // (:47-48)
}
// div_ipd's third argument: RN(1 / ipd), an IEEE division, once per face
NLML_IPD_HD double ipd_reciprocal(double ipd) { return 1.0 / ipd; }
// coordinate c of the reference point of the face row p
NLML_IPD_HD double ipd_origin(const float* p, int c) { return (double)p[ipd_col(IPD_LM_REF, c)]; }
// Everything a face row contributes: element k of the row becomes f32(div_ipd(f64(p[k]) - (x0, y0, z0)[k % 3], ipd, rcp)).
// (A kernel whose constants have other values on a path that does not normalise, joined at run time, composes the three pieces above
// itself -- normalize_ipd.hip, encoder_heads_f16x2_small.hip: out-parameters change the order in which hipcc 7.2 promotes such variables
// to registers, and with it the register allocation of the whole kernel.)
NLML_IPD_HD void ipd_setup(const float* p, double& ipd, double& rcp, double& x0, double& y0, double& z0) {
  ipd = ipd_length(p);
  rcp = ipd_reciprocal(ipd);
  x0 = ipd_origin(p, 0);
  y0 = ipd_origin(p, 1);
  z0 = ipd_origin(p, 2);
}

// the reference coordinates in the order a thread needs them whose FIRST column has coordinate ph = column % 3: its columns
// + 0, + 1, + 2 (and + 3, + 4, ... again) subtract ra, rb, rc
NLML_IPD_HD void ipd_phase(int ph, double x0, double y0, double z0, double& ra, double& rb, double& rc) {
  ra = ph == 0 ? x0 : (ph == 1 ? y0 : z0);
  rb = ph == 0 ? y0 : (ph == 1 ? z0 : x0);
  rc = ph == 0 ? z0 : (ph == 1 ? x0 : y0);
}

}  // namespace nlml
