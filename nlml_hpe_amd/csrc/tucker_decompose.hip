// tucker_decompose.hip -- K7a..K7d: the four device primitives of the Tucker decomposition of the rotation training tensor
// (TD_main.py:181, `core, factors = tucker(tensor, rank=[5, 3, 3, 3, 1404])`); the driver is nlml_hpe_amd/tucker_decompose.py.
//
// The tensor X is f32[I, ny, np, nr, M] (the reference's: 1620 x 11 x 9 x 7 x 1404 = 6.3 GB); every sum and every Gram is f64; factors
// are f64.  No floating-point atomics anywhere: partial sums go to the caller's workspace and are added in a fixed order, so two runs
// give the same bits.  Every element offset is int64_t.
//
// K7a  mode_gram         G = A A^T of A f32[I, K] (the mode-1 unfolding) on v_mfma_f64_16x16x4_f64.
//        A workgroup owns one 128 x 128 tile of the UPPER triangle and one K slice (split-K); its four waves own a 64 x 64 quarter each:
//        16 accumulator tiles per wave, and per K step of 4 eight operand fragments feed sixteen matrix instructions.  The f32 -> f64
//        conversion happens ONCE per element and workgroup, on the way into LDS (nothing issues in the shadow of an f64 MFMA,
//        tucker_common.h tucker_mfma4, so a conversion inside the K loop would be paid in full): the K loop is LDS reads and MFMAs only.
//        The next 32 columns are fetched into registers while the current ones are multiplied.  A second launch adds the K slices in
//        ascending order and writes the tile and its mirror image.
// K7b  pose_grams        the three small mode Grams (ny x ny, np x np, nr x nr) in ONE pass over X.
//        A workgroup loads a slab -- all ny np nr cells of one identity by 32 columns -- into LDS and its four waves run the three
//        Gram updates on the f64 matrix cores straight from it (operand rows beyond n are zero).  The accumulators live in registers
//        over all slabs of the workgroup; at the end the four waves are added in LDS and one partial per workgroup goes to the
//        workspace.  A second launch adds the workgroups' partials in ascending order.
// K7c  project_identity  out[r, k] = sum_i U[i, r] A[i, k]: a lane per column, i ascending, R f64 accumulators in registers.
// K7d  project_pose      X x_2 Uy^T x_3 Up^T x_4 Ur^T with any factor left out: a lane per (identity, kept cells, column), the
//        contraction nested roll-inside-pitch-inside-yaw so that an element costs rr + rp rr / nr + ry rp rr / (np nr) fma instead of
//        the ry rp rr of the Kronecker form; ranks are template parameters (<= 3 each), the accumulators registers.
// The kernels are templates on the tensors' element types: the *_ex entry points take or give f64 where the driver keeps a projected
// tensor unrounded between two steps (K7a, K7b, K7d in; K7c, K7d out); the sums and their order are the f32 forms' -- except K7b's,
// whose f64 slab is 16 columns wide (the same 128 bytes of a row), so that it has other slabs, other partials and, on inputs that
// are not exactly summable, other bits.
//
// The orders, as include/nlml_hpe.h states them and oracle/csrc/oracle.c ("K7") restates them on the host; tests/test_tucker_order_gpu.py
// holds the kernels to those models bit for bit:
//   K7a  slice = max(NLML_GRAM_KCHUNK, ceil(K / max(1, 1024 / pairs)) rounded up to 32 columns), pairs = the upper triangle of
//        ceil(I / 128) tile rows; per slice ONE fma chain per entry, k ascending (the matrix instruction adds its four k in ascending
//        order to its accumulator, and zero columns past the slice change nothing); slices added ascending from 0.0.
//   K7b  partial b of min(slabs, 1024) takes slabs b, b + partials, ...; wave w the pairs (o, j) = w, w + 4, ... of each mode's outer
//        and inner cells, columns ascending inside a pair, one chain per entry over all slabs of the workgroup; then
//        0.0 + w0 + w1 + w2 + w3 and the partials ascending from 0.0.
//   K7c  i ascending.     K7d  roll inside pitch inside yaw, each ascending; a kept mode is one step with coefficient 1.0.
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"

namespace nlml {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- K7a ------------------------------------------------------------------------------------------------------------------------
constexpr int MG_TILE = 128;                      // rows / columns of G per workgroup
constexpr int MG_KC = 32;                         // columns of A per LDS stage
constexpr int MG_LD = MG_KC + 2;                  // LDS row stride in doubles: 68 dwords, so the 16 rows of a fragment read hit 16 bank groups
constexpr int MG_THREADS = 256;
constexpr int MG_TARGET_WGS = 1024;               // split K until about this many workgroups exist
constexpr int MG_TILE_ELEMS = MG_TILE * MG_TILE;
static_assert(NLML_GRAM_KCHUNK % MG_KC == 0, "a K slice is whole LDS stages");

struct MgPlan {
  int tiles, pairs, splits;
  int64_t slice;                                  // columns per K slice (a multiple of MG_KC)
};
static MgPlan mg_plan(int64_t I, int64_t K) {
  MgPlan p;
  p.tiles = (int)((I + MG_TILE - 1) / MG_TILE);
  p.pairs = p.tiles * (p.tiles + 1) / 2;
  const int64_t smax = MG_TARGET_WGS / p.pairs > 1 ? MG_TARGET_WGS / p.pairs : 1;
  int64_t slice = (K + smax - 1) / smax;
  slice = (slice + MG_KC - 1) / MG_KC * MG_KC;
  p.slice = slice < NLML_GRAM_KCHUNK ? NLML_GRAM_KCHUNK : slice;
  p.splits = (int)((K + p.slice - 1) / p.slice);
  return p;
}
size_t mode_gram_workspace_bytes(int64_t I, int64_t K) {
  const MgPlan p = mg_plan(I, K);
  return (size_t)p.splits * p.pairs * MG_TILE_ELEMS * sizeof(double);
}

// pair index -> tile row ti <= tile column tj (row-major over the upper triangle)
__device__ __forceinline__ void mg_pair(int pair, int tiles, int& ti, int& tj) {
  ti = 0;
  while (pair >= tiles - ti) { pair -= tiles - ti; ++ti; }
  tj = ti + pair;
}

template <bool VEC4, class T>   // T: float (VEC4 where rows allow 16-byte loads) or double (a projected tensor kept in f64; VEC4 = false)
__global__ __launch_bounds__(MG_THREADS) void mode_gram_kernel(const T* __restrict__ A, int64_t I, int64_t K, int tiles, int pairs,
                                                               int64_t slice, double* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) double s_ab[2 * MG_TILE][MG_LD];   // rows 0..127: the tile's rows of A; 128..255: its columns' rows
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int pair = (int)(blockIdx.x % (unsigned)pairs), split = (int)(blockIdx.x / (unsigned)pairs);
  int ti, tj;
  mg_pair(pair, tiles, ti, tj);
  const int64_t kbeg = (int64_t)split * slice;
  const int64_t kend = kbeg + slice < K ? kbeg + slice : K;
  const bool active = ti != tj || wr <= wc;       // the lower quarter of a diagonal tile is never read

  T pre[8][4];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = t + MG_THREADS * j, row = f >> 3, c4 = (f & 7) * 4;
      const int64_t src = row < MG_TILE ? (int64_t)ti * MG_TILE + row : (int64_t)tj * MG_TILE + (row - MG_TILE);
      const int64_t k = k0 + c4;
      T v[4] = {0, 0, 0, 0};
      if (src < I) {
        const T* p = A + src * K + k;
        if (VEC4) {                               // K % 4 == 0 and kend % 4 == 0: a float4 is inside the slice or outside it
          if (k < kend) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = q[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k + e < kend) v[e] = p[e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) pre[j][e] = v[e];
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = t + MG_THREADS * j, row = f >> 3, c4 = (f & 7) * 4;
      f64x2* d = reinterpret_cast<f64x2*>(&s_ab[row][c4]);
      d[0] = f64x2{(double)pre[j][0], (double)pre[j][1]};
      d[1] = f64x2{(double)pre[j][2], (double)pre[j][3]};
    }
  };

  f64x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int frow = lane & 15, kq = lane >> 4;
  fetch(kbeg);
  for (int64_t k0 = kbeg; k0 < kend; k0 += MG_KC) {
    stash();
    __syncthreads();
    if (k0 + MG_KC < kend) fetch(k0 + MG_KC);
    if (active) {
#pragma unroll
      for (int kk = 0; kk < MG_KC / 4; ++kk) {
        double a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          a[q] = s_ab[wr * 64 + 16 * q + frow][4 * kk + kq];
          b[q] = s_ab[MG_TILE + wc * 64 + 16 * q + frow][4 * kk + kq];
        }
#pragma unroll
        for (int qa = 0; qa < 4; ++qa)
#pragma unroll
          for (int qb = 0; qb < 4; ++qb) acc[qa][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[qa], b[qb], acc[qa][qb], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (!active) return;
  double* dst = ws + ((int64_t)split * pairs + pair) * MG_TILE_ELEMS;
#pragma unroll
  for (int qa = 0; qa < 4; ++qa)
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wr * 64 + 16 * qa + kq + 4 * r, col = wc * 64 + 16 * qb + frow;
        dst[row * MG_TILE + col] = acc[qa][qb][r];
      }
}

// adds the K slices in ascending order; writes G[i][j] and its mirror G[j][i] from the same sum
__global__ __launch_bounds__(256) void mode_gram_reduce_kernel(const double* __restrict__ ws, int64_t I, int tiles, int pairs, int splits,
                                                               double* __restrict__ G) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int pair = (int)(idx / MG_TILE_ELEMS), e = (int)(idx % MG_TILE_ELEMS);
  if (pair >= pairs) return;
  const int r = e / MG_TILE, c = e % MG_TILE;
  int ti, tj;
  mg_pair(pair, tiles, ti, tj);
  const int64_t gi = (int64_t)ti * MG_TILE + r, gj = (int64_t)tj * MG_TILE + c;
  if (gi >= I || gj >= I || (ti == tj && r > c)) return;
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s += ws[((int64_t)sp * pairs + pair) * MG_TILE_ELEMS + e];
  G[gi * I + gj] = s;
  G[gj * I + gi] = s;
}

int launch_mode_gram(const void* A_, int a_f64, int64_t I, int64_t K, double* G, void* ws, void* stream) {
  const MgPlan p = mg_plan(I, K);
  const float* A = static_cast<const float*>(A_);
  const bool vec4 = !a_f64 && K % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const dim3 grid((unsigned)(p.pairs * p.splits)), block(MG_THREADS);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a_f64)
    hipLaunchKernelGGL((mode_gram_kernel<false, double>), grid, block, 0, st, static_cast<const double*>(A_), I, K, p.tiles, p.pairs, p.slice,
                       static_cast<double*>(ws));
  else if (vec4)
    hipLaunchKernelGGL((mode_gram_kernel<true, float>), grid, block, 0, st, A, I, K, p.tiles, p.pairs, p.slice, static_cast<double*>(ws));
  else
    hipLaunchKernelGGL((mode_gram_kernel<false, float>), grid, block, 0, st, A, I, K, p.tiles, p.pairs, p.slice, static_cast<double*>(ws));
  if (const int rc = hip_launch_status()) return rc;
  const dim3 rgrid((unsigned)((int64_t)p.pairs * MG_TILE_ELEMS / 256));
  hipLaunchKernelGGL(mode_gram_reduce_kernel, rgrid, dim3(256), 0, st, static_cast<const double*>(ws), I, p.tiles, p.pairs, p.splits, G);
  return hip_launch_status();
}

// ---- K7b ------------------------------------------------------------------------------------------------------------------------
// a slab row is 128 bytes of columns (32 f32 or 16 f64) + 16 bytes of padding: 36 dwords, and 36 r mod 64 are 16 distinct bank groups
template <class T> struct PgGeom {
  static constexpr int TC = 128 / (int)sizeof(T);          // columns of a slab
  static constexpr int TCP = TC + 16 / (int)sizeof(T);     // LDS row stride in elements
};
constexpr int PG_TC_MIN = PgGeom<double>::TC;
constexpr int PG_THREADS = 256;
constexpr int PG_MAX_GRID = 1024;                  // workgroups (and partials); depends on the shape alone, never on the device
constexpr int PG_N = NLML_POSE_BINS_MAX;           // 32: a Gram is at most 2 x 2 matrix-core tiles
constexpr int PG_SLAB_BYTES = NLML_POSE_GRAMS_MAX_CELLS * 144;
static_assert(PG_SLAB_BYTES >= 4 * 3 * PG_N * PG_N * (int)sizeof(double), "the waves' accumulators are added in the slab's LDS");
static_assert(PG_SLAB_BYTES <= 112 * 1024, "slab within the 160 KB of LDS");

static int64_t pg_grid(int64_t I, int64_t M, int tc) {
  const int64_t slabs = I * ((M + tc - 1) / tc);
  return slabs < PG_MAX_GRID ? slabs : PG_MAX_GRID;
}
// one size for both element types: the f64 form's partial count (its slabs are half as wide), which is never the smaller
size_t pose_grams_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M) {
  return (size_t)pg_grid(I, M, PG_TC_MIN) * (size_t)(ny * ny + np * np + nr * nr) * sizeof(double);
}

// One mode's Gram update from the slab: the mode has extent n, `O` cells outside it and `J` inside (cell = (o n + a) J + j).  The K
// index of the product runs over (o, j, column); this wave takes every fourth (o, j).  acc[0]: rows/columns 0..15, acc[1]: rows 0..15 x
// columns 16..31, acc[2]: rows/columns 16..31.
template <class T>
__device__ __forceinline__ void pg_mode(const T* slab, int O, int n, int J, int lane, int wv, f64x4 (&acc)[3]) {
  constexpr int PG_TC = PgGeom<T>::TC, PG_TCP = PgGeom<T>::TCP;
  const int row = lane & 15, kq = lane >> 4;
  const bool v0 = row < n, v1 = row + 16 < n, big = n > 16;
  const int off0 = (v0 ? row : 0) * J * PG_TCP + kq, off1 = (v1 ? row + 16 : 0) * J * PG_TCP + kq;
  const int OJ = O * J;
  for (int oj = wv; oj < OJ; oj += 4) {
    const int o = oj / J, j = oj - o * J;
    const T* p = slab + (o * n * J + j) * PG_TCP;
#pragma unroll
    for (int s = 0; s < PG_TC / 4; ++s) {
      const double a0 = v0 ? (double)p[off0 + 4 * s] : 0.0;
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, acc[0], 0, 0, 0);
      if (big) {
        const double a1 = v1 ? (double)p[off1 + 4 * s] : 0.0;
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a1, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, acc[2], 0, 0, 0);
      }
    }
  }
}

template <bool VEC4, class T>
__global__ __launch_bounds__(PG_THREADS) void pose_grams_kernel(const T* __restrict__ X, int ny, int np, int nr, int64_t M, int64_t mtiles,
                                                                int64_t slabs, int do_y, int do_p, int do_r, double* __restrict__ ws) {
  constexpr int PG_TC = PgGeom<T>::TC, PG_TCP = PgGeom<T>::TCP, GPR = PG_TC / 4;   // GPR: groups of four columns per slab row
  __shared__ __attribute__((aligned(16))) T s_slab[PG_SLAB_BYTES / sizeof(T)];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int cells = ny * np * nr;
  f64x4 acc[3][3];
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[m][q] = f64x4{0.0, 0.0, 0.0, 0.0};

  for (int64_t sl = blockIdx.x; sl < slabs; sl += gridDim.x) {
    const int64_t i = sl / mtiles, m0 = (sl - i * mtiles) * PG_TC;
    const T* base = X + i * cells * M + m0;
    for (int f = t; f < cells * GPR; f += PG_THREADS) {
      const int cell = f / GPR, c4 = (f - cell * GPR) * 4;
      const T* p = base + (int64_t)cell * M + c4;
      T v[4] = {0, 0, 0, 0};
      if (VEC4) {                                  // M % 4 == 0: a float4 is inside the row or outside it
        if (m0 + c4 < M) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = q[e];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m0 + c4 + e < M) v[e] = p[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) s_slab[cell * PG_TCP + c4 + e] = v[e];
    }
    __syncthreads();
    if (do_y) pg_mode(s_slab, 1, ny, np * nr, lane, wv, acc[0]);
    if (do_p) pg_mode(s_slab, ny, np, nr, lane, wv, acc[1]);
    if (do_r) pg_mode(s_slab, ny * np, nr, 1, lane, wv, acc[2]);
    __syncthreads();
  }

  // the four waves' accumulators, added in wave order; red[wave][mode][32][32]
  double* red = reinterpret_cast<double*>(s_slab);
  const int col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = (q == 2 ? 16 : 0) + kq + 4 * r, cc = (q == 0 ? 0 : 16) + col;
        red[((wv * 3 + m) * PG_N + rr) * PG_N + cc] = acc[m][q][r];
      }
  __syncthreads();
  const int ey = ny * ny, ep = np * np, er = nr * nr;
  double* dst = ws + (int64_t)blockIdx.x * (ey + ep + er);
  for (int e = t; e < ey + ep + er; e += PG_THREADS) {
    const int m = e < ey ? 0 : (e < ey + ep ? 1 : 2);
    const int n = m == 0 ? ny : (m == 1 ? np : nr);
    const int le = e - (m == 0 ? 0 : (m == 1 ? ey : ey + ep));
    const int a = le / n, b = le - a * n;
    double s = 0.0;
    if (a <= b) {
#pragma unroll
      for (int w = 0; w < 4; ++w) s += red[((w * 3 + m) * PG_N + a) * PG_N + b];
    }
    dst[e] = s;
  }
}

// adds the workgroups' partials in ascending order; entry (a, b) and its mirror come from the upper one
__global__ __launch_bounds__(256) void pose_grams_reduce_kernel(const double* __restrict__ ws, int parts, int ny, int np, int nr,
                                                                double* __restrict__ Gy, double* __restrict__ Gp, double* __restrict__ Gr) {
  const int ey = ny * ny, ep = np * np, er = nr * nr;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= ey + ep + er) return;
  const int m = e < ey ? 0 : (e < ey + ep ? 1 : 2);
  const int n = m == 0 ? ny : (m == 1 ? np : nr);
  double* G = m == 0 ? Gy : (m == 1 ? Gp : Gr);
  if (!G) return;
  const int off = m == 0 ? 0 : (m == 1 ? ey : ey + ep);
  const int le = e - off;
  const int a = le / n, b = le - a * n;
  const int src = off + (a <= b ? a * n + b : b * n + a);
  double s = 0.0;
  for (int g = 0; g < parts; ++g) s += ws[(int64_t)g * (ey + ep + er) + src];
  G[le] = s;
}

int launch_pose_grams(const void* X_, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr, void* ws,
                      void* stream) {
  const int tc = x_f64 ? PgGeom<double>::TC : PgGeom<float>::TC;
  const int64_t mtiles = (M + tc - 1) / tc, slabs = I * mtiles;
  const int parts = (int)pg_grid(I, M, tc);
  const float* X = static_cast<const float*>(X_);
  const bool vec4 = !x_f64 && M % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* w = static_cast<double*>(ws);
  if (x_f64)
    hipLaunchKernelGGL((pose_grams_kernel<false, double>), dim3(parts), dim3(PG_THREADS), 0, st, static_cast<const double*>(X_), ny, np, nr, M,
                       mtiles, slabs, Gy != nullptr, Gp != nullptr, Gr != nullptr, w);
  else if (vec4)
    hipLaunchKernelGGL((pose_grams_kernel<true, float>), dim3(parts), dim3(PG_THREADS), 0, st, X, ny, np, nr, M, mtiles, slabs, Gy != nullptr,
                       Gp != nullptr, Gr != nullptr, w);
  else
    hipLaunchKernelGGL((pose_grams_kernel<false, float>), dim3(parts), dim3(PG_THREADS), 0, st, X, ny, np, nr, M, mtiles, slabs, Gy != nullptr,
                       Gp != nullptr, Gr != nullptr, w);
  if (const int rc = hip_launch_status()) return rc;
  const int entries = ny * ny + np * np + nr * nr;
  hipLaunchKernelGGL(pose_grams_reduce_kernel, dim3((entries + 255) / 256), dim3(256), 0, st, static_cast<const double*>(ws), parts, ny, np, nr,
                     Gy, Gp, Gr);
  return hip_launch_status();
}

// ---- K7c ------------------------------------------------------------------------------------------------------------------------
constexpr int PI_THREADS = 256;
constexpr unsigned PJ_MAX_GRID = 0x7fffffffu;

template <int R, class TOut>
__global__ __launch_bounds__(PI_THREADS) void project_identity_kernel(const float* __restrict__ A, int64_t I, int64_t K,
                                                                      const double* __restrict__ U, TOut* __restrict__ out) {
  for (int64_t k = (int64_t)blockIdx.x * PI_THREADS + threadIdx.x; k < K; k += (int64_t)gridDim.x * PI_THREADS) {
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    const float* p = A + k;
#pragma unroll 4
    for (int64_t i = 0; i < I; ++i) {
      const double x = (double)p[i * K];
      const double* u = U + i * R;                 // wave-uniform: scalar loads
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fma(u[r], x, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) out[(int64_t)r * K + k] = (TOut)acc[r];
  }
}

template <int R>
static void pi_launch(const float* A, int64_t I, int64_t K, const double* U, void* out, int out_f64, dim3 grid, hipStream_t st) {
  if (out_f64)
    hipLaunchKernelGGL((project_identity_kernel<R, double>), grid, dim3(PI_THREADS), 0, st, A, I, K, U, static_cast<double*>(out));
  else
    hipLaunchKernelGGL((project_identity_kernel<R, float>), grid, dim3(PI_THREADS), 0, st, A, I, K, U, static_cast<float*>(out));
}

int launch_project_identity(const float* A, int64_t I, int64_t K, const double* U, int R, void* out, int out_f64, void* stream) {
  const int64_t groups = (K + PI_THREADS - 1) / PI_THREADS;
  const dim3 grid(groups < (int64_t)PJ_MAX_GRID ? (unsigned)groups : PJ_MAX_GRID);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (R) {
#define NLML_PI_CASE(n) case n: pi_launch<n>(A, I, K, U, out, out_f64, grid, st); break;
    NLML_PI_CASE(1) NLML_PI_CASE(2) NLML_PI_CASE(3) NLML_PI_CASE(4) NLML_PI_CASE(5) NLML_PI_CASE(6) NLML_PI_CASE(7) NLML_PI_CASE(8)
    NLML_PI_CASE(9) NLML_PI_CASE(10) NLML_PI_CASE(11) NLML_PI_CASE(12) NLML_PI_CASE(13) NLML_PI_CASE(14) NLML_PI_CASE(15) NLML_PI_CASE(16)
#undef NLML_PI_CASE
    default: return fail(NLML_E_BADARG, "project_identity: R outside 1..16");
  }
  return hip_launch_status();
}

// ---- K7d ------------------------------------------------------------------------------------------------------------------------
// A mode with a factor is contracted (its output extent is the template rank); a mode without one is kept: the lane's own index of
// it comes out of the lane number (by / bp / br = its extent, else 1), the loop over it has one step and the coefficient is 1.
struct PpArgs {
  const void* X;           // TIn
  const double *Uy, *Up, *Ur;
  void* out;               // TOut
  int64_t I, M, total;     // total = lanes = I by bp br M
  int ny, np, nr;
};

template <int RY, int RP, int RR, class TIn, class TOut>
__global__ __launch_bounds__(256) void project_pose_kernel(PpArgs a) {
  const bool cy = a.Uy != nullptr, cp = a.Up != nullptr, cr = a.Ur != nullptr;
  const int by = cy ? 1 : a.ny, bp = cp ? 1 : a.np, br = cr ? 1 : a.nr;
  const int oy = cy ? RY : a.ny, op = cp ? RP : a.np, orr = cr ? RR : a.nr;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (int64_t)gridDim.x * 256) {
    int64_t q = idx / a.M;
    const int64_t m = idx - q * a.M;
    const int rb = (int)(q % br); q /= br;
    const int pb = (int)(q % bp); q /= bp;
    const int yb = (int)(q % by);
    const int64_t i = q / by;
    const int y0 = cy ? 0 : yb, y1 = cy ? a.ny : yb + 1;
    const int p0 = cp ? 0 : pb, p1 = cp ? a.np : pb + 1;
    const int r0 = cr ? 0 : rb, r1 = cr ? a.nr : rb + 1;
    double acc[RY][RP][RR];
#pragma unroll
    for (int ia = 0; ia < RY; ++ia)
#pragma unroll
      for (int ib = 0; ib < RP; ++ib)
#pragma unroll
        for (int ic = 0; ic < RR; ++ic) acc[ia][ib][ic] = 0.0;
    const TIn* xi = static_cast<const TIn*>(a.X) + i * a.ny * a.np * a.nr * a.M + m;
    for (int y = y0; y < y1; ++y) {
      double tp[RP][RR];
#pragma unroll
      for (int ib = 0; ib < RP; ++ib)
#pragma unroll
        for (int ic = 0; ic < RR; ++ic) tp[ib][ic] = 0.0;
      for (int p = p0; p < p1; ++p) {
        double tr[RR];
#pragma unroll
        for (int ic = 0; ic < RR; ++ic) tr[ic] = 0.0;
        const TIn* xr = xi + (int64_t)((y * a.np + p) * a.nr) * a.M;
        // a plain loop: issuing the roll bins' loads in groups of eight ahead of their fma was measured SLOWER (8.0 against 5.6 ms
        // at the reference's shape, profiles/tucker_decompose.md)
        for (int r = r0; r < r1; ++r) {
          const double x = (double)xr[(int64_t)r * a.M];
#pragma unroll
          for (int ic = 0; ic < RR; ++ic) tr[ic] = fma(cr ? a.Ur[r * RR + ic] : 1.0, x, tr[ic]);
        }
#pragma unroll
        for (int ib = 0; ib < RP; ++ib)
#pragma unroll
          for (int ic = 0; ic < RR; ++ic) tp[ib][ic] = fma(cp ? a.Up[p * RP + ib] : 1.0, tr[ic], tp[ib][ic]);
      }
#pragma unroll
      for (int ia = 0; ia < RY; ++ia)
#pragma unroll
        for (int ib = 0; ib < RP; ++ib)
#pragma unroll
          for (int ic = 0; ic < RR; ++ic) acc[ia][ib][ic] = fma(cy ? a.Uy[y * RY + ia] : 1.0, tp[ib][ic], acc[ia][ib][ic]);
    }
    TOut* oi = static_cast<TOut*>(a.out) + i * oy * op * orr * a.M + m;
#pragma unroll
    for (int ia = 0; ia < RY; ++ia)
#pragma unroll
      for (int ib = 0; ib < RP; ++ib)
#pragma unroll
        for (int ic = 0; ic < RR; ++ic) {
          const int cell = ((cy ? ia : yb) * op + (cp ? ib : pb)) * orr + (cr ? ic : rb);
          oi[(int64_t)cell * a.M] = (TOut)acc[ia][ib][ic];
        }
  }
}

template <int RY, int RP, int RR>
static void pp_launch_type(const PpArgs& a, int x_f64, int out_f64, dim3 grid, hipStream_t st) {
  if (x_f64 && out_f64) hipLaunchKernelGGL((project_pose_kernel<RY, RP, RR, double, double>), grid, dim3(256), 0, st, a);
  else if (x_f64) hipLaunchKernelGGL((project_pose_kernel<RY, RP, RR, double, float>), grid, dim3(256), 0, st, a);
  else if (out_f64) hipLaunchKernelGGL((project_pose_kernel<RY, RP, RR, float, double>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((project_pose_kernel<RY, RP, RR, float, float>), grid, dim3(256), 0, st, a);
}
template <int RY, int RP>
static void pp_launch_rr(const PpArgs& a, int rr, int x_f64, int out_f64, dim3 grid, hipStream_t st) {
  switch (rr) {
    case 1: pp_launch_type<RY, RP, 1>(a, x_f64, out_f64, grid, st); break;
    case 2: pp_launch_type<RY, RP, 2>(a, x_f64, out_f64, grid, st); break;
    default: pp_launch_type<RY, RP, 3>(a, x_f64, out_f64, grid, st); break;
  }
}
template <int RY>
static void pp_launch_rp(const PpArgs& a, int rp, int rr, int x_f64, int out_f64, dim3 grid, hipStream_t st) {
  switch (rp) {
    case 1: pp_launch_rr<RY, 1>(a, rr, x_f64, out_f64, grid, st); break;
    case 2: pp_launch_rr<RY, 2>(a, rr, x_f64, out_f64, grid, st); break;
    default: pp_launch_rr<RY, 3>(a, rr, x_f64, out_f64, grid, st); break;
  }
}

// ry / rp / rr: 1..NLML_POSE_RANK_MAX where the factor is given (checked by the caller); ignored where it is NULL
int launch_project_pose(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up,
                        int rp, const double* Ur, int rr, void* out, int out_f64, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!Uy && !Up && !Ur && x_f64 == out_f64) {     // nothing to contract, nothing to convert: the tensor itself
    const hipError_t e = hipMemcpyAsync(out, X, (size_t)(I * ny * np * nr * M) * (x_f64 ? sizeof(double) : sizeof(float)), hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? 0 : fail((int)e, hipGetErrorString(e));
  }
  PpArgs a;
  a.X = X; a.Uy = Uy; a.Up = Up; a.Ur = Ur; a.out = out;
  a.I = I; a.M = M; a.ny = ny; a.np = np; a.nr = nr;
  a.total = I * (Uy ? 1 : ny) * (Up ? 1 : np) * (Ur ? 1 : nr) * M;
  const int64_t groups = (a.total + 255) / 256;
  const dim3 grid(groups < (int64_t)PJ_MAX_GRID ? (unsigned)groups : PJ_MAX_GRID);
  const int ty = Uy ? ry : 1, tp = Up ? rp : 1, tr = Ur ? rr : 1;
  switch (ty) {
    case 1: pp_launch_rp<1>(a, tp, tr, x_f64, out_f64, grid, st); break;
    case 2: pp_launch_rp<2>(a, tp, tr, x_f64, out_f64, grid, st); break;
    default: pp_launch_rp<3>(a, tp, tr, x_f64, out_f64, grid, st); break;
  }
  return hip_launch_status();
}

}  // namespace nlml
