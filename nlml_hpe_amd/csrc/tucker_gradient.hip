// tucker_gradient.hip -- K3g: objective value and analytic gradient (TD_Tester.py:60-102) in the reference's operation order, for any
// identity rank R = 1..16 (nlml_tucker_gradient_r).  The order itself is written down in tucker_grad_ref.h.  Two launches:
//
//   tucker_gradient_kernel      one workgroup of 768 threads per FOUR gradients.  A gradient is four evaluations of the reference-order
//       pass (tucker_ref_pass, untouched): the chains x_hat, e_y, e_p, e_r differ only in one factor triple, so the workgroup's 16
//       machine slots are 4 gradients x 4 chains with a factor table of f and df entries -- one gradient a 4-evaluation pass, two an
//       8-evaluation pass.  The pass leaves the chains' rows in the caller's workspace (16 rows per workgroup, read back by the threads
//       of the same workgroup after its barrier) and err = 0.5 sum(r^2) of the x_hat slots.  Then: one sweep over Wm for the f32 chain
//       v of all four gradients; r = x - x_hat, t = r f64(v) into the workspace, TRANSPOSED ([1404, N], so the second kernel reads 64
//       evaluations of one column with one load); the three angle components by numpy's pairwise tree over r e_a.
//   tucker_gradient_uid_kernel  grad_u[i] = -einsum('ijklm,m->i', W, t) in numpy's buffered two-lane order: 10 sequential chains per
//       (evaluation, i).  A workgroup of 10 waves takes one i and 64 evaluations: wave = chain, lane = evaluation, so the element of W
//       is the same for the whole wave (scalar loads) and only t is per lane.
//
// Bound: the f64 vector issue rate, as for K3: 20 f64 operations per (q, m) in the four chains, 4 f32 operations for v and 2 f64 for the
// identity term (DESIGN.md section 3 has the measured times).
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "tucker_grad_ref.h"
#include "tucker_rank.h"

namespace nlml {

constexpr int TG_GPB = 4;                   // gradients per workgroup: 4 chains each = the 16 machine slots
static_assert(TG_GPB * 4 == EV && TG_M == TM, "a workgroup's chains are the pass's machine slots");
constexpr int TG_WS_ROWS = EV;              // f64[1404] chain rows per workgroup
constexpr int TG_UID_NT = 64 * TG_CHAINS;   // second kernel: one wave per chain
constexpr int TG_UID_B = 16;                // multiply-adds per register batch (the next batch's loads fly under this one's adds)

// slot s = 4 g + c: gradient g of the workgroup, chain c (0: x_hat, 1..3: e_y, e_p, e_r)
struct GradPar {
  const double* p;   // params of the workgroup's first gradient
  int64_t left;      // gradients available from there (>= 1)
  int n;             // parameters per evaluation, 3 + R
  __device__ __forceinline__ double operator()(int slot, int k) const {
    const int g = slot >> 2;
    return gload<double>(p + (g < left ? g : left - 1) * n + k);
  }
};
struct GradXRow {
  const float* x;
  const int32_t* x_index;
  int64_t ldx, g0, N;
  __device__ __forceinline__ const float* operator()(int slot) const {
    int64_t n = g0 + (slot >> 2);
    n = n < N ? n : N - 1;
    return x + (x_index ? (int64_t)x_index[n] : n) * ldx;
  }
};
struct GradChainRow {
  double* x_hat;     // the workgroup's 16 rows
  __device__ __forceinline__ double* operator()(int slot) const { return x_hat + slot * TM; }
};

// numpy's pairwise sums of rs.d2[0 .. nrows), nrows <= TG_SUM_ROWS (np_sum.h over the pass's tree, TrTree): a lane per (row, leaf), then
// thread t < nrows returns row t's.  Eight lanes of every wave take leaves: neighbouring leaves of a row start 48 words apart modulo the
// 64 LDS banks (a row: a multiple of 64), so a wave's reads meet two or three to a bank; the sixteen leaves of four rows in one wave
// would meet sixteen.
constexpr int TG_SUM_ROWS = 6;              // r e_y, r e_p, r e_r of two gradients
static_assert(TG_SUM_ROWS * TR_LEAVES <= TR_NT / 64 * 8, "eight leaves per wave");
template <typename RS>
__device__ __forceinline__ double tg_block_pairwise(RS& rs, int nrows, int tid) {
  const int task = (tid >> 6) * 8 + (tid & 63);
  if ((tid & 63) < 8 && task < nrows * TR_LEAVES) {
    const int n = task / TR_LEAVES, L = task % TR_LEAVES;
    rs.leaf[n][L] = np_leaf_sum(rs.d2[n] + tr_leaf_start(L), tr_leaf_len(L));
  }
  __syncthreads();
  return tid < nrows ? np_tree_sum<TR_LEAVES>(rs.leaf[tid]) : 0.0;
}

__global__ __launch_bounds__(TR_NT, 1) void tucker_gradient_kernel(
    const float* __restrict__ Wm, const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ x_index,
    const double* __restrict__ params, const double* __restrict__ cosp, int64_t N, double* __restrict__ err,
    double* __restrict__ grad, double* __restrict__ chains, double* __restrict__ tT, int rid) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) TuckerFvecShared sh;
  __shared__ __attribute__((aligned(16))) TuckerRefSharedR<8> rs;
  __shared__ float ff[TG_GPB][2][3][3];     // [gradient][f, df][angle][row]
  const int tid = threadIdx.x;
  const int64_t g0 = (int64_t)blockIdx.x * TG_GPB;
  const int64_t left = N - g0;
  const int ng = left < TG_GPB ? (int)left : TG_GPB;
  const int np = 3 + rid;
  const GradPar par{params + g0 * np, left, np};

  // f and df of the workgroup's gradients (a gradient beyond N repeats the last one: defined values, never stored)
  if (tid < TG_GPB * 9) {
    const int g = tid / 9, a = (tid % 9) / 3, j = tid % 3;
    const double* row = cosp + (a * 3 + j) * 4;                   // (a,b,c,d) row, TD_Tester.py:26
    ff[g][0][a][j] = cr_fvec(row, par(4 * g, a));
    ff[g][1][a][j] = cr_dfvec(row, par(4 * g, a));
  }
  __syncthreads();
  if (tid < EV * 9) {
    const int slot = tid / 9, a = (tid % 9) / 3, j = tid % 3;
    sh.fvec[slot][a][j] = (double)ff[slot >> 2][(slot & 3) == a + 1 ? 1 : 0][a][j];
  }
  __syncthreads();

  // the four chains of every gradient: two gradients per pass over Wm
  double* const rows = chains + (size_t)blockIdx.x * TG_WS_ROWS * TM;
  const GradXRow xrow{x, x_index, ldx, g0, N};
  const GradChainRow chrow{rows};
  const TrDynRank rank{rid};
  for (int g = 0; g < ng; g += 2) {
    unsigned slots = 0;
    for (int i = 0; i < 8; ++i) slots |= (unsigned)(4 * g + i) << (4 * i);
    if (ng - g >= 2) tucker_ref_pass<8>(sh, rs, Wm, par, slots, xrow, chrow, tid, rank);
    else tucker_ref_pass<4>(sh, rs, Wm, par, slots & 0xffffu, xrow, chrow, tid, rank);
  }
  // (the pass ends with a barrier: the rows it wrote are visible to the whole workgroup)
  if (err && tid < ng) err[g0 + tid] = rs.err[4 * tid];

  // v = einsum('ijklm,j,k,l->m') in f32, all four gradients on one sweep over Wm; thread t on columns t and t + 768
  const int m0 = tid, m1 = tid + TR_NT;
  const bool live1 = m1 < TM;
  float v[TG_GPB][2];
#pragma unroll
  for (int g = 0; g < TG_GPB; ++g) v[g][0] = v[g][1] = 0.0f;
  const int tq = 27 * rid;
  int j = 0, k = 0, l = 0;
  for (int q = 0; q < tq; ++q) {
    const float w0 = Wm[(size_t)q * TM + m0], w1 = Wm[(size_t)q * TM + (live1 ? m1 : 0)];
#pragma unroll
    for (int g = 0; g < TG_GPB; ++g) {
      const float fy = ff[g][0][0][j], fp = ff[g][0][1][k], fr = ff[g][0][2][l];
      v[g][0] = ((w0 * fy) * fp) * fr + v[g][0];
      v[g][1] = ((w1 * fy) * fp) * fr + v[g][1];
    }
    if (++l == 3) {
      l = 0;
      if (++k == 3) {
        k = 0;
        if (++j == 3) j = 0;
      }
    }
  }

  // r, t = r f64(v) (transposed out), and the angle components two gradients at a time: rows (g & 1) * 3 + a of rs.d2 hold r e_a
  for (int gb = 0; gb < ng; gb += 2) {
    const int nb = ng - gb < 2 ? ng - gb : 2;
#pragma unroll
    for (int gi = 0; gi < 2; ++gi) {
      const int g = gb + gi;
      if (gi < nb) {
        const float* xr = xrow(4 * g);
        const double* ch = rows + (size_t)4 * g * TM;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int m = c ? m1 : m0;
          if (c == 0 || live1) {
            const double r = (double)xr[m] - ch[m];
            const float vv = (g == 0 ? v[0][c] : g == 1 ? v[1][c] : g == 2 ? v[2][c] : v[3][c]);
            tT[(size_t)m * N + (g0 + g)] = r * (double)vv;
#pragma unroll
            for (int a = 0; a < 3; ++a) rs.d2[gi * 3 + a][m] = r * ch[(1 + a) * TM + m];
          }
        }
      }
    }
    __syncthreads();
    const double sum = tg_block_pairwise(rs, 3 * nb, tid);
    if (tid < 3 * nb) grad[(g0 + gb + tid / 3) * np + tid % 3] = -sum;
    __syncthreads();
  }
}

// grad_u[i] of 64 evaluations: wave w = chunk * 2 + lane of numpy's two-lane loop, thread lane = evaluation
__global__ __launch_bounds__(TG_UID_NT) void tucker_gradient_uid_kernel(const float* __restrict__ Wm, const double* __restrict__ tT,
                                                                        int64_t N, double* __restrict__ grad, int rid) {
#pragma clang fp contract(off)
  __shared__ double accs[TG_CHAINS][64];
  const int i = blockIdx.y, ln = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int chunk = wv >> 1, lane2 = wv & 1;
  const int64_t n = (int64_t)blockIdx.x * 64 + ln;
  const double* tn = tT + (n < N ? n : N - 1);
  const float* wi = Wm + (size_t)i * TG_ROW;
  const int start = chunk * TG_CHUNK, count = tg_chunk_count(chunk), steps = tg_uid_steps(count);

  float wb[2][TG_UID_B];
  double tb[2][TG_UID_B];
  auto load = [&](int s0, float (&w)[TG_UID_B], double (&t)[TG_UID_B]) {   // steps past the end re-read the last one (inside W and tT)
#pragma unroll
    for (int q = 0; q < TG_UID_B; ++q) {
      const int s = s0 + q < steps ? s0 + q : steps - 1;
      const int e = start + tg_uid_elem(count, s, lane2);
      w[q] = wi[e];
      t[q] = tn[(size_t)((unsigned)e % (unsigned)TG_M) * N];
    }
  };
  double acc = 0.0;
  auto run = [&](int s0, const float (&w)[TG_UID_B], const double (&t)[TG_UID_B]) {
#pragma unroll
    for (int q = 0; q < TG_UID_B; ++q) {
      const double a1 = (double)w[q] * t[q] + acc;
      acc = s0 + q < steps ? a1 : acc;
    }
  };
  load(0, wb[0], tb[0]);
  for (int s0 = 0; s0 < steps; s0 += 2 * TG_UID_B) {
    load(s0 + TG_UID_B, wb[1], tb[1]);
    run(s0, wb[0], tb[0]);
    load(s0 + 2 * TG_UID_B, wb[0], tb[0]);
    run(s0 + TG_UID_B, wb[1], tb[1]);
  }
  accs[wv][ln] = acc;
  __syncthreads();
  if (threadIdx.x < 64 && n < N) grad[n * (3 + rid) + 3 + i] = tg_uid_combine([&](int c) { return accs[c][ln]; });
}

size_t tucker_gradient_workspace_bytes(int64_t N) {
  if (N <= 0) return 0;
  const size_t groups = (size_t)((N + TG_GPB - 1) / TG_GPB);
  return (groups * TG_WS_ROWS * TM + (size_t)N * TM) * sizeof(double);
}

int launch_tucker_gradient(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                           const double* cos_params, int64_t N, double* err, double* grad, int r_id, void* workspace, void* stream) {
  if (N == 0) return 0;
  const unsigned groups = (unsigned)((N + TG_GPB - 1) / TG_GPB);
  double* chains = static_cast<double*>(workspace);
  double* tT = chains + (size_t)groups * TG_WS_ROWS * TM;
  hipLaunchKernelGGL(tucker_gradient_kernel, dim3(groups), dim3(TR_NT), 0, reinterpret_cast<hipStream_t>(stream), Wm, x, ldx, x_index,
                     params, cos_params, N, err, grad, chains, tT, r_id);
  if (int rc = hip_launch_status()) return rc;
  hipLaunchKernelGGL(tucker_gradient_uid_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)r_id), dim3(TG_UID_NT), 0,
                     reinterpret_cast<hipStream_t>(stream), Wm, tT, N, grad, r_id);
  return hip_launch_status();
}

}  // namespace nlml
