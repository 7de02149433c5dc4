// encoder_train_dev.h -- the device pieces of THE GEMM ORDER and THE OTHER SUMS (encoder_train_ref.h) that K9 (encoder_train.hip) and
// K10 (heads_train.hip) share: the operand loads, a wave's MFMA chain, the partial tiles' meeting in LDS and the halving tree; on them
// the forward tile and the backward tile (mlp_forward_tile, mlp_backward_tile: one network's view of a launch plus the launch's shared
// fields; the kernels around them and the loops that launch them are encoder_train.hip's, declared in abi_internal.h), the loss kernels' tail (et_loss_tail) and
// the update kernels' prologue (et_clip_prologue).  K9 is the launch of one network (gridDim.y = 1); K10 passes
// zero_grad = 1 and has no Tanh.  The bits depend on the tile bodies' order: the bias start on wave 0 only, then
// et_chain, the bias runs, et_store_partial, the tile totals, sq[], et_tree; et_tile_total * et_act_grad is one multiply.
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

// ---- forward tile: out[b][o] = act(sum_k A[b][k] W[o][k] + bias[o]) ---------------------------------------------------------------------
struct MlpFwdNet {
  const float* A; int64_t lda;
  const int32_t* order; int64_t N;      // layer 0: the rows come from the dataset through order
  int32_t* rows;                        // layer 0 writes the batch's resolved rows here
  const float* W; const float* bias; float* out;
  int B, avec;
};
struct MlpFwdShared {
  int64_t slot0;
  int K, Nout, ldo, act, gather, wvec;  // act: MLP_ACT_*
};
struct MlpFwd { MlpFwdNet net[MLP_NETS_MAX]; MlpFwdShared s; };   // a launch's arguments: blockIdx.y is the network

// ragged: a network of the launch may have fewer rows than the grid was sized for (B < Bmax, or B = 0: exhausted).  A launch of one
// network never is, and its kernel says so at compile time: the test would put the argument loads behind a first load and a branch.
__device__ __forceinline__ void mlp_forward_tile(const MlpFwdNet& q, const MlpFwdShared& p, const bool ragged) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tn_n = et_tiles(p.Nout);
  const int tm = blockIdx.x / tn_n, tn = blockIdx.x % tn_n;
  if (ragged && tm * ET_TILE >= q.B) return;
  const int m = tm * ET_TILE + r, n = tn * ET_TILE + r;
  EtOperand a = {nullptr, q.lda, nullptr, q.avec != 0}, b = {nullptr, p.K, nullptr, p.wvec != 0};
  if (m < q.B) {
    int64_t row = m;
    if (p.gather) {
      bool clamped;
      row = et_resolve_row(q.order, p.slot0 + m, q.N, &clamped);
      if (tn == 0 && wave == 0 && h == 0) q.rows[m] = (int32_t)row;
    }
    a.p = q.A + row * q.lda;
  }
  if (n < p.Nout) b.p = q.W + (int64_t)n * p.K;
  const float start = (wave == 0 && n < p.Nout) ? q.bias[n] : 0.0f;
  et_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = start;
  et_chain<true, true>(acc, a, b, p.K, wave, h);
  et_store_partial(red, acc, wave, lane);
  for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
    const int mm = tm * ET_TILE + (e >> 5), nn = tn * ET_TILE + (e & 31);
    if (mm >= q.B || nn >= p.Nout) continue;
    float z = et_tile_total(red, e);
    if (p.act == MLP_ACT_RELU) z = z > 0.0f ? z : 0.0f;
    else if (p.act == MLP_ACT_TANH) z = tanhf(z);
    q.out[(int64_t)mm * p.ldo + nn] = z;
  }
}

// ---- backward tile of one layer: wgrad tiles [0, n_wgrad), then dgrad tiles -------------------------------------------------------------
struct MlpBwdNet {
  const float* delta;                                    // delta_l [B, out]
  const float* aprev; int64_t lda; const int32_t* rows;  // A_{l-1} [B, in]; rows: layer 0's gather of the dataset
  const float* W; float* gW; float* gb;
  float* dprev;                                          // delta_{l-1} [B, in], NULL for layer 0
  double* partials;                                      // this layer's norm partials, one per wgrad tile
  int B;
};
struct MlpBwdShared { int ldd, ldp, in, out, zero_grad, tanh_prev, n_wgrad, dvec; };
struct MlpBwd { MlpBwdNet net[MLP_NETS_MAX]; MlpBwdShared s; };

__device__ __forceinline__ void mlp_backward_tile(const MlpBwdNet& q, const MlpBwdShared& p, const bool ragged) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  __shared__ float runs[ET_BIAS_RUNS][ET_TILE];
  __shared__ double sq[ET_NT];
  if (ragged && q.B == 0) return;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tn_n = et_tiles(p.in);
  et_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
  if ((int)blockIdx.x < p.n_wgrad) {
    // dW[o][i] = sum_b delta[b][o] aprev[b][i]: both operands k-outer
    const int tm = blockIdx.x / tn_n, tn = blockIdx.x % tn_n;
    const int o = tm * ET_TILE + r, i = tn * ET_TILE + r;
    const EtOperand a = {o < p.out ? q.delta + o : nullptr, p.ldd, nullptr, false};
    const EtOperand b = {i < p.in ? q.aprev + i : nullptr, q.lda, q.rows, false};
    et_chain<false, false>(acc, a, b, q.B, wave, h);
    if (tn == 0) {   // this tile's bias rows: run `wave*2 + h` of column o
      const int run = threadIdx.x >> 5, rp = (q.B + ET_BIAS_RUNS - 1) / ET_BIAS_RUNS;
      float s = 0.0f;
      if (o < p.out)
        for (int bb = run * rp; bb < q.B && bb < (run + 1) * rp; ++bb) s = s + q.delta[(int64_t)bb * p.ldd + o];
      runs[run][r] = s;
    }
    et_store_partial(red, acc, wave, lane);
    double s = 0.0;
    for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
      const int oo = tm * ET_TILE + (e >> 5), ii = tn * ET_TILE + (e & 31);
      if (oo >= p.out || ii >= p.in) continue;
      float* g = q.gW + (int64_t)oo * p.in + ii;
      const float dw = et_tile_total(red, e);
      const float gn = p.zero_grad ? dw : *g + dw;
      *g = gn;
      s = fma((double)gn, (double)gn, s);
    }
    if (tn == 0 && (int)threadIdx.x < ET_TILE && tm * ET_TILE + (int)threadIdx.x < p.out) {
      const int oo = tm * ET_TILE + threadIdx.x;
      float total = runs[0][threadIdx.x];
#pragma unroll
      for (int i = 1; i < ET_BIAS_RUNS; ++i) total = total + runs[i][threadIdx.x];
      const float gn = p.zero_grad ? total : q.gb[oo] + total;
      q.gb[oo] = gn;
      s = fma((double)gn, (double)gn, s);
    }
    sq[threadIdx.x] = s;
    const double total = et_tree<double, ET_NT>(sq);
    if (threadIdx.x == 0) q.partials[blockIdx.x] = total;
  } else {
    // delta_{l-1}[b][i] = (sum_o delta[b][o] W[o][i]) act'(aprev[b][i]): delta k-contiguous, W k-outer
    const int t = blockIdx.x - p.n_wgrad;
    const int tm = t / tn_n, tn = t % tn_n;
    if (ragged && tm * ET_TILE >= q.B) return;
    const int m = tm * ET_TILE + r, i = tn * ET_TILE + r;
    const EtOperand a = {m < q.B ? q.delta + (int64_t)m * p.ldd : nullptr, p.ldd, nullptr, p.dvec != 0};
    const EtOperand b = {i < p.in ? q.W + i : nullptr, p.in, nullptr, false};
    et_chain<true, false>(acc, a, b, p.out, wave, h);
    et_store_partial(red, acc, wave, lane);
    for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
      const int mm = tm * ET_TILE + (e >> 5), ii = tn * ET_TILE + (e & 31);
      if (mm >= q.B || ii >= p.in) continue;
      const float av = q.aprev[(int64_t)mm * q.lda + ii];
      q.dprev[(int64_t)mm * p.ldp + ii] = et_tile_total(red, e) * et_act_grad(av, p.tanh_prev != 0);
    }
  }
}

// ---- the loss kernels' tail: every thread brings its row's q and flags; thread 0 writes total / denom and the status word ---------------
__device__ __forceinline__ void et_loss_tail(float q, int flags, float denom, float* loss_out, int32_t* status, int first) {
  __shared__ float q_s[ET_BATCH_MAX];
  __shared__ int f_s[ET_BATCH_MAX];
  const int b = threadIdx.x;
  q_s[b] = q;
  f_s[b] = flags;
  __syncthreads();
  for (int stride = ET_BATCH_MAX / 2; stride >= 1; stride >>= 1) {
    if (b < stride) {
      q_s[b] = q_s[b] + q_s[b + stride];
      f_s[b] |= f_s[b + stride];
    }
    __syncthreads();
  }
  if (b == 0) {
    if (loss_out) *loss_out = q_s[0] / denom;
    if (status) *status = (first ? 0 : *status) | f_s[0];
  }
}

// ---- the update kernels' prologue: the norm from the partials -> the clip coefficient; workgroup 0 writes the norm ----------------------
__device__ __forceinline__ float et_clip_prologue(const double* __restrict__ partials, int n_partials, double max_norm, float* norm_out) {
  __shared__ double sq[ET_NT];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += ET_NT) s = s + partials[i];
  sq[threadIdx.x] = s;
  double norm;
  const float c = (float)et_clip_coefficient(et_tree<double, ET_NT>(sq), max_norm, &norm);
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = (float)norm;
  return c;
}

}  // namespace nlml
