// rotate_landmarks.hip -- K6: landmarks at a known pose (write-streaming kernel), one body behind two entry points.
//
// Replaces helpers/IntrinsicRotation.apply_rotations (IntrinsicRotation.py:108-120) and the rotation branch of
// CreateTensor.Compose_Tensor (CreateTensor.py:96-114), in numpy's own operation order (rotate_ref.h), so the result is the
// reference's bit for bit.  No trigonometry runs here: the 3x3 matrices are inputs.
//
// The unit of work is a ROW: the 468 points of one face at one pose = 1,404 outputs = 5,616 B = 351 x 16 B.
//   grid mode   row = ((id * ny + yaw) * np + pitch) * nr + roll, the reference's composition_tensor[id, yaw, pitch, roll, :]; the
//               landmarks are base[id], the three matrices come from the per-axis tables, and the cell whose three bins are the
//               zero bins is the base copied bit for bit
//   face mode   row = face; the landmarks are lm[face], the matrices rot[face][0..2] in application order; no copy rule
// A workgroup takes RT_ROWS consecutive rows per step of a grid-stride loop.  Per row:
//   P0  234 lanes, two points each (t and t + 234): three f32 loads per point (the 9 MB of landmarks stay in L2; HBM sees the writes),
//       27 f64 fma per point, the results to LDS as f32 (word 3 i + c: stride-3, conflict-free) and, where out64 is asked for, as f64
//   P1  all lanes: the row from LDS to memory with 16-byte non-temporal stores, lane i at byte 16 i -- a wave's stores cover whole
//       lines although x,y,z are interleaved and a float4 straddles points; out64 with 8-byte stores (f64 buffers are 8-byte aligned)
// The LDS row is double-buffered, so a row costs one barrier.  A row's matrices are wave-uniform: the indices derive from blockIdx and
// loop counters alone, the loads are scalar loads and the 27 doubles live in scalar registers.
// Every row and byte offset is int64_t: the reference's own shape (1620, 11, 9, 7, 1404) has byte offsets beyond 4 GiB, and
// TD_main.py:108's other configurations have element offsets beyond 2^31.
// out64 is a template parameter: the instance without it has neither its LDS nor its stores.
// Algorithmic bytes per row: 5,616 written (+ 11,232 with out64); 14.2 G fma for the reference's grid against 6.30 GB of stores.
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"
#include "rotate_ref.h"

namespace nlml {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RT_F4 = RT_F / 4;            // 351 float4 per row: a float4 never straddles two rows
constexpr int RT_THREADS = 256;
constexpr int RT_HALF = RT_LM / 2;         // 234 lanes compute, points t and t + 234
constexpr int RT_ROWS = 8;                 // consecutive rows per workgroup and loop step
constexpr unsigned RT_MAX_GRID = 0x7fffffffu;
static_assert(RT_F % 4 == 0 && 2 * RT_HALF == RT_LM && RT_HALF <= RT_THREADS, "row geometry");

template <bool GRID, bool W32, bool W64>
__global__ __launch_bounds__(RT_THREADS) void rotate_kernel(const float* __restrict__ lm, const double* __restrict__ rot_yaw,
                                                            const double* __restrict__ rot_pitch, const double* __restrict__ rot_roll,
                                                            int ny, int np, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll,
                                                            int64_t rows, float* __restrict__ out, double* __restrict__ out64) {
  __shared__ __attribute__((aligned(16))) float s_row[2][RT_F];
  __shared__ double s_row64[W64 ? 2 : 1][W64 ? RT_F : 1];

  const int t = threadIdx.x;
  const int64_t groups = (rows + RT_ROWS - 1) / RT_ROWS;
  int buf = 0;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    int64_t row = g * RT_ROWS;
    // grid mode: the cell of the group's first row, then an odometer (the divisions once per group, not per row)
    int64_t id = 0;
    int y = 0, p = 0, r = 0;
    if (GRID) {
      int64_t q = row;
      r = (int)(q % nr); q /= nr;
      p = (int)(q % np); q /= np;
      y = (int)(q % ny);
      id = q / ny;
    }
    for (int j = 0; j < RT_ROWS && row < rows; ++j, ++row) {
      const float* src = lm + (GRID ? id : row) * (int64_t)RT_F;
      const double *M0, *M1, *M2;
      bool copy = false;
      if (GRID) {
        rt_cell_order(order, rot_yaw + 9 * y, rot_pitch + 9 * p, rot_roll + 9 * r, M0, M1, M2);
        copy = y == zero_yaw && p == zero_pitch && r == zero_roll;
      } else {
        M0 = rot_yaw + row * 27;   // face mode: rot[face][0..2]
        M1 = M0 + 9;
        M2 = M0 + 18;
      }
      float* const sb = s_row[buf];
      double* const sb64 = s_row64[W64 ? buf : 0];

      // P0
      if (t < RT_HALF) {
        if (copy) {   // (uniform) the base landmarks themselves
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int e = 3 * (t + h * RT_HALF);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float v = src[e + c];
              sb[e + c] = v;
              if (W64) sb64[e + c] = (double)v;
            }
          }
        } else {
          double m0[9], m1[9], m2[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) { m0[k] = M0[k]; m1[k] = M1[k]; m2[k] = M2[k]; }
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int e = 3 * (t + h * RT_HALF);
            const double a[3] = {(double)src[e], (double)src[e + 1], (double)src[e + 2]};
            double o[3];
            rt_pose(a, m0, m1, m2, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              sb[e + c] = (float)o[c];
              if (W64) sb64[e + c] = o[c];
            }
          }
        }
      }
      __syncthreads();   // the one barrier of a row: the next row goes to the other buffer

      // P1
      const int64_t off = row * (int64_t)RT_F;
      if (W32) {
        f32x4* const o4 = reinterpret_cast<f32x4*>(out + off);
        const f32x4* const s4 = reinterpret_cast<const f32x4*>(sb);
        for (int i = t; i < RT_F4; i += RT_THREADS) __builtin_nontemporal_store(s4[i], o4 + i);
      }
      if (W64) {
        double* const o = out64 + off;
        for (int i = t; i < RT_F; i += RT_THREADS) __builtin_nontemporal_store(sb64[i], o + i);
      }
      buf ^= 1;

      if (GRID && ++r == nr) {
        r = 0;
        if (++p == np) {
          p = 0;
          if (++y == ny) { y = 0; ++id; }
        }
      }
    }
  }
}

template <bool GRID, bool W32, bool W64>
static int launch_instance(const float* lm, const double* rot_yaw, const double* rot_pitch, const double* rot_roll, int ny, int np, int nr,
                           int order, int zy, int zp, int zr, int64_t rows, float* out, double* out64, void* stream) {
  const int64_t groups = (rows + RT_ROWS - 1) / RT_ROWS;
  const dim3 grid(groups < (int64_t)RT_MAX_GRID ? (unsigned)groups : RT_MAX_GRID), block(RT_THREADS);
  hipLaunchKernelGGL((rotate_kernel<GRID, W32, W64>), grid, block, 0, reinterpret_cast<hipStream_t>(stream), lm, rot_yaw, rot_pitch, rot_roll,
                     ny, np, nr, order, zy, zp, zr, rows, out, out64);
  return hip_launch_status();
}

int launch_compose_rotation_tensor(const float* base, int64_t rows, const double* rot_yaw, int ny, const double* rot_pitch, int np,
                                   const double* rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll, float* out,
                                   double* out64, void* stream) {
  if (rows == 0) return 0;
  return out64 ? launch_instance<true, true, true>(base, rot_yaw, rot_pitch, rot_roll, ny, np, nr, order, zero_yaw, zero_pitch, zero_roll,
                                                   rows, out, out64, stream)
               : launch_instance<true, true, false>(base, rot_yaw, rot_pitch, rot_roll, ny, np, nr, order, zero_yaw, zero_pitch, zero_roll,
                                                    rows, out, nullptr, stream);
}

int launch_rotate_landmarks(const float* lm, const double* rot, float* out, double* out64, int64_t B, void* stream) {
  if (B == 0) return 0;
  if (out && out64) return launch_instance<false, true, true>(lm, rot, nullptr, nullptr, 1, 1, 1, 0, -1, -1, -1, B, out, out64, stream);
  if (out) return launch_instance<false, true, false>(lm, rot, nullptr, nullptr, 1, 1, 1, 0, -1, -1, -1, B, out, nullptr, stream);
  return launch_instance<false, false, true>(lm, rot, nullptr, nullptr, 1, 1, 1, 0, -1, -1, -1, B, nullptr, out64, stream);
}

}  // namespace nlml
