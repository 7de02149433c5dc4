// rotate_ref.h -- the operation order of helpers/IntrinsicRotation.py:108-120 (apply_rotations) and of the rotation branch of
// CreateTensor.Compose_Tensor (CreateTensor.py:96-114) as numpy evaluates them, shared by the device kernel (rotate_landmarks.hip)
// and the host restatement (nlml_compose_rotation_tensor_host, nlml_rotate_landmarks_host, abi.cpp).
//
//   landmarks @ M                 the [468,3] float32 block promoted to f64, times a [3,3] f64 matrix, through numpy's BLAS:
//                                 b[j] = fma(a[2], M[2][j], fma(a[1], M[1][j], fma(a[0], M[0][j], +0.0)))
//                                 The accumulator STARTS at +0.0: fma(a0, m0, +0.0) is not a0 * m0 -- a product that is -0.0 becomes +0.0.
//   (L @ M0) @ M1 @ M2            three such stages, every stage's outputs rounded to f64 before the next
//       intrinsic                 M0, M1, M2 = Rx(pitch), Ry(yaw), Rz(roll)
//       extrinsic                 M0, M1, M2 = Rz(roll)^T, Ry(yaw)^T, Rx(pitch)^T        (:113-118)
//   torch.tensor(.., float32)     one rounding of the third stage's f64 (CreateTensor.py:110)
//   yaw == pitch == roll == 0     Compose_Tensor copies the base landmarks (:97-98): no rotation by identity matrices, which would turn
//                                 a -0.0 coordinate into +0.0
//
// No trigonometry here: the matrices are inputs (the host layer builds them with numpy, in the reference's expressions).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_RT_HD __host__ __device__
#else
#define NLML_RT_HD
#endif

namespace nlml {

constexpr int RT_LM = 468;          // landmarks per face
constexpr int RT_F = 3 * RT_LM;     // 1404 coordinates per face, x,y,z interleaved
constexpr int RT_INTRINSIC = 0;     // NLML_ROT_INTRINSIC
constexpr int RT_EXTRINSIC = 1;     // NLML_ROT_EXTRINSIC

// one stage: b = a @ M, M row-major [3][3].  fma(a, m, +0.0) must stay an fma: it is what makes (-0.0 product) + 0.0 = +0.0.
NLML_RT_HD inline void rt_stage(const double* a, const double* M, double* b) {
  for (int j = 0; j < 3; ++j) {
    double acc = 0.0;
    acc = fma(a[0], M[0 + j], acc);
    acc = fma(a[1], M[3 + j], acc);
    acc = fma(a[2], M[6 + j], acc);
    b[j] = acc;
  }
}

// one point at one pose: the three matrices in application order
NLML_RT_HD inline void rt_pose(const double* a, const double* M0, const double* M1, const double* M2, double* out) {
  double b[3], c[3];
  rt_stage(a, M0, b);
  rt_stage(b, M1, c);
  rt_stage(c, M2, out);
}

// the application order of a grid cell's matrices: which of (yaw, pitch, roll) is stage 0, 1, 2
NLML_RT_HD inline void rt_cell_order(int order, const double* yaw, const double* pitch, const double* roll, const double*& M0,
                                     const double*& M1, const double*& M2) {
  M1 = yaw;
  if (order == RT_INTRINSIC) { M0 = pitch; M2 = roll; } else { M0 = roll; M2 = pitch; }
}

// One face on the host: lm f32[1404] at the pose (M0, M1, M2) -> out f32[1404] and / or out64 f64[1404] (either may be null).
inline void rt_face_host(const float* lm, const double* M0, const double* M1, const double* M2, float* out, double* out64) {
  for (int i = 0; i < RT_LM; ++i) {
    const double a[3] = {(double)lm[3 * i], (double)lm[3 * i + 1], (double)lm[3 * i + 2]};
    double o[3];
    rt_pose(a, M0, M1, M2, o);
    for (int c = 0; c < 3; ++c) {
      if (out) out[3 * i + c] = (float)o[c];
      if (out64) out64[3 * i + c] = o[c];
    }
  }
}

// The copied cell: the base landmarks bit for bit; its f64 form is the same values widened.
inline void rt_copy_host(const float* lm, float* out, double* out64) {
  if (out) memcpy(out, lm, RT_F * sizeof(float));
  if (out64)
    for (int e = 0; e < RT_F; ++e) out64[e] = (double)lm[e];
}

// The whole tensor on the host: out[id, yaw, pitch, roll, :], zero_* = the bin whose value is 0 on that axis or -1.
inline void rt_grid_host(const float* base, int64_t I, const double* rot_yaw, int ny, const double* rot_pitch, int np, const double* rot_roll,
                         int nr, int order, int zero_yaw, int zero_pitch, int zero_roll, float* out, double* out64) {
  int64_t row = 0;
  for (int64_t id = 0; id < I; ++id)
    for (int y = 0; y < ny; ++y)
      for (int p = 0; p < np; ++p)
        for (int r = 0; r < nr; ++r, ++row) {
          const float* lm = base + id * RT_F;
          float* o = out ? out + row * RT_F : nullptr;
          double* o64 = out64 ? out64 + row * RT_F : nullptr;
          if (y == zero_yaw && p == zero_pitch && r == zero_roll) {
            rt_copy_host(lm, o, o64);
            continue;
          }
          const double *M0, *M1, *M2;
          rt_cell_order(order, rot_yaw + 9 * y, rot_pitch + 9 * p, rot_roll + 9 * r, M0, M1, M2);
          rt_face_host(lm, M0, M1, M2, o, o64);
        }
}

}  // namespace nlml
