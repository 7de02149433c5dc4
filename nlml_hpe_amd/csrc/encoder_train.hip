// encoder_train.hip -- K9: training steps of the landmark encoder (NLML_HPE_EncoderTrainer.py:393-456), a whole epoch enqueued at once.
//
// A step is fourteen launches ordered by the stream, nothing else: six forward layers (activations kept in the workspace), the
// residual and loss, six backward layers (a layer's wgrad tiles and its dgrad tiles are disjoint workgroup ranges of ONE launch: both
// consume delta_l), and the update (every workgroup reduces the norm partials itself, in the same order, so the clip coefficient
// needs no launch and no broadcast).  No atomics, no grid-wide barrier, no workgroup waits for another; losses, norms and the clip
// coefficient never leave the device.  The operation order is encoder_train_ref.h's; this file is its MFMA form:
//
//   one workgroup = one 32 x 32 output tile = ET_WAVES waves that split K (a tile's chain is up to 702 dependent MFMAs of 64 cycles:
//   on one wave it would leave three SIMDs idle, and the small layers have fewer tiles than the device has CUs); every wave reads its
//   own operands straight from global memory (a k-contiguous operand as one 16-byte load per four MFMAs, a k-outer operand as four
//   row-coalesced loads), one super-chunk ahead; the partial tiles meet in LDS and are added in wave order.
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "encoder_train_dev.h"   // the GEMM order's device pieces (et_ld_*, et_chain, et_store_partial, et_tile_total, et_tree), shared with K10
#include "encoder_train_ref.h"

namespace nlml {

// ---- forward: out[b][o] = act(sum_k A[b][k] W[o][k] + bias[o]) ------------------------------------------------------------------------
struct EtFwd {
  const float* A; int64_t lda;
  const int32_t* order; int64_t slot0, N; int gather;   // layer 0: the rows come from the dataset through order
  int32_t* rows;                                        // layer 0 writes the batch's resolved rows here
  const float* W; const float* bias; float* out; int ldo;
  int B, K, Nout, act;                                  // act: 0 none, 1 ReLU, 2 Tanh
  int avec, wvec;
};

__global__ __launch_bounds__(ET_NT) void et_forward_kernel(EtFwd p) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tn_n = et_tiles(p.Nout);
  const int tm = blockIdx.x / tn_n, tn = blockIdx.x % tn_n;
  const int m = tm * ET_TILE + r, n = tn * ET_TILE + r;
  EtOperand a = {nullptr, p.lda, nullptr, p.avec != 0}, b = {nullptr, p.K, nullptr, p.wvec != 0};
  if (m < p.B) {
    int64_t row = m;
    if (p.gather) {
      bool clamped;
      row = et_resolve_row(p.order, p.slot0 + m, p.N, &clamped);
      if (tn == 0 && wave == 0 && h == 0) p.rows[m] = (int32_t)row;
    }
    a.p = p.A + row * p.lda;
  }
  if (n < p.Nout) b.p = p.W + (int64_t)n * p.K;
  const float start = (wave == 0 && n < p.Nout) ? p.bias[n] : 0.0f;
  et_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = start;
  et_chain<true, true>(acc, a, b, p.K, wave, h);
  et_store_partial(red, acc, wave, lane);
  for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
    const int mm = tm * ET_TILE + (e >> 5), nn = tn * ET_TILE + (e & 31);
    if (mm >= p.B || nn >= p.Nout) continue;
    float z = et_tile_total(red, e);
    if (p.act == 1) z = z > 0.0f ? z : 0.0f;
    else if (p.act == 2) z = tanhf(z);
    p.out[(int64_t)mm * p.ldo + nn] = z;
  }
}

// ---- residual and loss: one workgroup, one thread per row -----------------------------------------------------------------------------
struct EtLoss {
  const float* pred; const int32_t* rows;
  const int32_t* order; int64_t slot0, N;
  const int32_t* labels; int64_t ld_lab;
  const float* table[3]; int nrows[3];
  float* delta;          // NULL: the validation pass
  float* loss_out;       // this step's slot, or NULL
  int32_t* status; int first;
  int B; float scale;
};

__global__ __launch_bounds__(ET_BATCH_MAX) void et_loss_kernel(EtLoss p) {
  __shared__ float q_s[ET_BATCH_MAX];
  __shared__ int f_s[ET_BATCH_MAX];
  const int b = threadIdx.x;
  float q = 0.0f;
  int flags = 0;
  if (b < p.B) {
    bool cl;
    et_resolve_row(p.order, p.slot0 + b, p.N, &cl);
    if (cl) flags |= ET_STATUS_ORDER;
    const int64_t row = p.rows[b];
    cl = false;
#pragma unroll
    for (int j = 0; j < ET_LATENT; ++j) {
      const int t = j / 3;
      const int tr = et_clamp_label(p.labels[row * p.ld_lab + t], p.nrows[t], &cl);
      const float d = p.pred[b * ET_LATENT_LD + j] - p.table[t][tr * 3 + j % 3];
      if (p.delta) p.delta[b * ET_LATENT_LD + j] = d * p.scale;
      q = fmaf(d, d, q);
    }
    if (cl) flags |= ET_STATUS_LABEL;
  }
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
    if (p.loss_out) *p.loss_out = q_s[0] / (float)(3 * p.B);
    if (p.status) *p.status = (p.first ? 0 : *p.status) | f_s[0];
  }
}

// ---- backward of one layer: wgrad tiles [0, n_wgrad), then dgrad tiles ----------------------------------------------------------------
struct EtBwd {
  const float* delta; int ldd;                           // delta_l [B, out]
  const float* aprev; int64_t lda; const int32_t* rows;  // A_{l-1} [B, in]; rows: layer 0's gather of the dataset
  const float* W; float* gW; float* gb;
  float* dprev; int ldp;                                 // delta_{l-1} [B, in], NULL for layer 0
  double* partials;                                      // this layer's norm partials, one per wgrad tile
  int B, in, out, zero_grad, tanh_prev, n_wgrad, dvec;
};

__global__ __launch_bounds__(ET_NT) void et_backward_kernel(EtBwd p) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  __shared__ float runs[ET_BIAS_RUNS][ET_TILE];
  __shared__ double sq[ET_NT];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tn_n = et_tiles(p.in);
  et_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
  if ((int)blockIdx.x < p.n_wgrad) {
    // dW[o][i] = sum_b delta[b][o] aprev[b][i]: both operands k-outer
    const int tm = blockIdx.x / tn_n, tn = blockIdx.x % tn_n;
    const int o = tm * ET_TILE + r, i = tn * ET_TILE + r;
    const EtOperand a = {o < p.out ? p.delta + o : nullptr, p.ldd, nullptr, false};
    const EtOperand b = {i < p.in ? p.aprev + i : nullptr, p.lda, p.rows, false};
    et_chain<false, false>(acc, a, b, p.B, wave, h);
    if (tn == 0) {   // this tile's bias rows: run `wave*2 + h` of column o
      const int run = threadIdx.x >> 5, rp = (p.B + ET_BIAS_RUNS - 1) / ET_BIAS_RUNS;
      float s = 0.0f;
      if (o < p.out)
        for (int bb = run * rp; bb < p.B && bb < (run + 1) * rp; ++bb) s = s + p.delta[(int64_t)bb * p.ldd + o];
      runs[run][r] = s;
    }
    et_store_partial(red, acc, wave, lane);
    double s = 0.0;
    for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
      const int oo = tm * ET_TILE + (e >> 5), ii = tn * ET_TILE + (e & 31);
      if (oo >= p.out || ii >= p.in) continue;
      float* g = p.gW + (int64_t)oo * p.in + ii;
      const float dw = et_tile_total(red, e);
      const float gn = p.zero_grad ? dw : *g + dw;
      *g = gn;
      s = fma((double)gn, (double)gn, s);
    }
    if (tn == 0 && (int)threadIdx.x < ET_TILE && tm * ET_TILE + (int)threadIdx.x < p.out) {
      const int oo = tm * ET_TILE + threadIdx.x;
      float total = runs[0][threadIdx.x];
#pragma unroll
      for (int q = 1; q < ET_BIAS_RUNS; ++q) total = total + runs[q][threadIdx.x];
      const float gn = p.zero_grad ? total : p.gb[oo] + total;
      p.gb[oo] = gn;
      s = fma((double)gn, (double)gn, s);
    }
    sq[threadIdx.x] = s;
    const double total = et_tree<double, ET_NT>(sq);
    if (threadIdx.x == 0) p.partials[blockIdx.x] = total;
  } else {
    // delta_{l-1}[b][i] = (sum_o delta[b][o] W[o][i]) act'(aprev[b][i]): delta k-contiguous, W k-outer
    const int t = blockIdx.x - p.n_wgrad;
    const int tm = t / tn_n, tn = t % tn_n;
    const int m = tm * ET_TILE + r, i = tn * ET_TILE + r;
    const EtOperand a = {m < p.B ? p.delta + (int64_t)m * p.ldd : nullptr, p.ldd, nullptr, p.dvec != 0};
    const EtOperand b = {i < p.in ? p.W + i : nullptr, p.in, nullptr, false};
    et_chain<true, false>(acc, a, b, p.out, wave, h);
    et_store_partial(red, acc, wave, lane);
    for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
      const int mm = tm * ET_TILE + (e >> 5), ii = tn * ET_TILE + (e & 31);
      if (mm >= p.B || ii >= p.in) continue;
      const float av = p.aprev[(int64_t)mm * p.lda + ii];
      p.dprev[(int64_t)mm * p.ldp + ii] = et_tile_total(red, e) * et_act_grad(av, p.tanh_prev != 0);
    }
  }
}

// ---- norm, clip and update ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ET_NT) void et_update_kernel(float* __restrict__ params, float* __restrict__ grads, int64_t total,
                                                          const double* __restrict__ partials, int n_partials, float lr, float wd,
                                                          double max_norm, float* norm_out) {
  __shared__ double sq[ET_NT];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += ET_NT) s = s + partials[i];
  sq[threadIdx.x] = s;
  double norm;
  const float c = (float)et_clip_coefficient(et_tree<double, ET_NT>(sq), max_norm, &norm);
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = (float)norm;
  const int64_t e0 = (int64_t)blockIdx.x * ET_UPDATE_PER_WG;
  for (int i = 0; i < ET_UPDATE_PER_WG / ET_NT; ++i) {
    const int64_t e = e0 + (int64_t)i * ET_NT + threadIdx.x;
    if (e < total) et_update(params + e, grads + e, c, lr, wd);
  }
}

static bool et_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ceil(n / batch) steps (c.grads == NULL: forward and loss only), all enqueued on `stream`; nothing is read back
int launch_encoder_train(const EtCall& c, void* workspace, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const EtDims d = et_dims(c.F);
  const EtWorkspace ws = et_workspace(c.F, c.batch);
  char* base = static_cast<char*>(workspace);
  double* partials = reinterpret_cast<double*>(base + ws.partials);
  int32_t* rows = reinterpret_cast<int32_t*>(base + ws.rows);
  float* act[ET_LAYERS];
  float* delta[ET_LAYERS];
  for (int l = 0; l < ET_LAYERS; ++l) {
    act[l] = reinterpret_cast<float*>(base + ws.act[l]);
    delta[l] = reinterpret_cast<float*>(base + ws.delta[l]);
  }
  const bool xvec = c.ldx % 4 == 0 && c.F % 4 == 0 && et_aligned16(c.x);
  int64_t step = 0;
  for (int64_t s0 = 0; s0 < c.n; s0 += c.batch, ++step) {
    const int B = (int)(c.n - s0 < c.batch ? c.n - s0 : c.batch);
    for (int l = 0; l < ET_LAYERS; ++l) {
      EtFwd f{};
      f.A = l == 0 ? c.x : act[l - 1]; f.lda = l == 0 ? c.ldx : ws.ld[l - 1];
      f.order = c.order; f.slot0 = s0; f.N = c.N; f.gather = l == 0; f.rows = rows;
      f.W = c.params + d.w_off[l]; f.bias = c.params + d.b_off[l]; f.out = act[l]; f.ldo = ws.ld[l];
      f.B = B; f.K = d.in[l]; f.Nout = d.out[l]; f.act = l < 4 ? 1 : (l == 4 ? 2 : 0);
      f.avec = l == 0 ? xvec : 1; f.wvec = d.in[l] % 4 == 0 && et_aligned16(f.W);
      hipLaunchKernelGGL(et_forward_kernel, dim3((unsigned)(et_tiles(B) * et_tiles(d.out[l]))), dim3(ET_NT), 0, st, f);
    }
    EtLoss q{};
    q.pred = act[5]; q.rows = rows; q.order = c.order; q.slot0 = s0; q.N = c.N; q.labels = c.labels; q.ld_lab = c.ld_lab;
    for (int t = 0; t < 3; ++t) { q.table[t] = c.table[t]; q.nrows[t] = c.rows[t]; }
    q.delta = c.grads ? delta[5] : nullptr;
    q.loss_out = c.loss_out ? c.loss_out + step : nullptr;
    q.status = c.status; q.first = step == 0; q.B = B; q.scale = (float)(2.0 / (3.0 * B));
    hipLaunchKernelGGL(et_loss_kernel, dim3(1), dim3(ET_BATCH_MAX), 0, st, q);
    if (c.grads) {
      for (int l = ET_LAYERS - 1; l >= 0; --l) {
        EtBwd b{};
        b.delta = delta[l]; b.ldd = ws.ld[l];
        b.aprev = l == 0 ? c.x : act[l - 1]; b.lda = l == 0 ? c.ldx : ws.ld[l - 1]; b.rows = l == 0 ? rows : nullptr;
        b.W = c.params + d.w_off[l]; b.gW = c.grads + d.w_off[l]; b.gb = c.grads + d.b_off[l];
        b.dprev = l == 0 ? nullptr : delta[l - 1]; b.ldp = l == 0 ? 0 : ws.ld[l - 1];
        b.partials = partials + d.part_off[l];
        b.B = B; b.in = d.in[l]; b.out = d.out[l]; b.zero_grad = c.zero_grad; b.tanh_prev = l - 1 == 4;
        b.n_wgrad = et_tiles(d.out[l]) * et_tiles(d.in[l]); b.dvec = 1;
        const int n_dgrad = l == 0 ? 0 : et_tiles(B) * et_tiles(d.in[l]);
        hipLaunchKernelGGL(et_backward_kernel, dim3((unsigned)(b.n_wgrad + n_dgrad)), dim3(ET_NT), 0, st, b);
      }
      hipLaunchKernelGGL(et_update_kernel, dim3((unsigned)((d.total + ET_UPDATE_PER_WG - 1) / ET_UPDATE_PER_WG)), dim3(ET_NT), 0, st,
                         c.params, c.grads, d.total, partials, d.n_partials, c.lr, c.wd, c.max_norm,
                         c.norm_out ? c.norm_out + step : nullptr);
    }
    if (int rc = hip_launch_status()) return rc;
  }
  return 0;
}

}  // namespace nlml
