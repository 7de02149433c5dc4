// heads_train.hip -- K10: training steps of the yaw, pitch and roll heads (NLML_HPE_MLPHeadsTrainer.py:83-126), a whole epoch of all
// networks enqueued at once.
//
// K9's shape (encoder_train.hip): a step is twelve launches ordered by the stream, nothing else -- five forward layers, the residual
// and loss, five backward layers (wgrad tiles and dgrad tiles are disjoint workgroup ranges of one launch; no dgrad for layer 0) and
// the norm/clip/Adam launch (every workgroup reduces the network's 78 norm partials itself, in the same order).  No atomics, no
// grid-wide barrier, no workgroup waits for another, nothing is read back.  What is new is the second grid dimension: blockIdx.y is
// the NETWORK.  No launch of this size runs under ~4.8 us whatever it computes (profiles/encoder_train.md), so the up to three
// independent networks of a call share every launch, each through its own row of the launch's argument table; a network whose rows
// are used up has B = 0 there, and its workgroups return before touching memory.  The operation order is heads_train_ref.h's; the
// GEMMs are K9's device pieces (encoder_train_dev.h), unchanged.
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "encoder_train_dev.h"
#include "heads_train_ref.h"

namespace nlml {

// ---- forward: out[b][o] = act(sum_k A[b][k] W[o][k] + bias[o]) ------------------------------------------------------------------------
struct HtFwdNet {
  const float* A; int64_t lda;
  const int32_t* order; int64_t N;      // layer 0: the rows come from the table through order
  int32_t* rows;                        // layer 0 writes the batch's resolved rows here
  const float* W; const float* bias; float* out;
  int B, avec;
};
struct HtFwd {
  HtFwdNet net[HT_NETS_MAX];
  int64_t slot0;
  int K, Nout, ldo, relu, gather, wvec;
};

__global__ __launch_bounds__(ET_NT) void ht_forward_kernel(HtFwd p) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  const HtFwdNet& q = p.net[blockIdx.y];
  const int tn_n = et_tiles(p.Nout);
  const int tm = blockIdx.x / tn_n, tn = blockIdx.x % tn_n;
  if (tm * ET_TILE >= q.B) return;   // a smaller batch than the launch's largest, or an exhausted network
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
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
    if (p.relu) z = z > 0.0f ? z : 0.0f;
    q.out[(int64_t)mm * p.ldo + nn] = z;
  }
}

// ---- residual and loss: one workgroup per network, one thread per row -------------------------------------------------------------------
struct HtLossNet {
  const float* pred; const int32_t* rows;
  const int32_t* order; int64_t N;
  const float* y;
  float* delta;          // NULL: the evaluation pass
  float* loss_out;       // this step's slot, or NULL
  int32_t* status;
  int B; float scale;
};
struct HtLoss {
  HtLossNet net[HT_NETS_MAX];
  int64_t slot0;
  int first;
};

__global__ __launch_bounds__(ET_BATCH_MAX) void ht_loss_kernel(HtLoss p) {
  __shared__ float q_s[ET_BATCH_MAX];
  __shared__ int f_s[ET_BATCH_MAX];
  const HtLossNet& n = p.net[blockIdx.y];
  if (n.B == 0) return;
  const int b = threadIdx.x;
  float q = 0.0f;
  int flags = 0;
  if (b < n.B) {
    bool cl;
    et_resolve_row(n.order, p.slot0 + b, n.N, &cl);
    if (cl) flags |= HT_STATUS_ORDER;
    float d;
    q = ht_loss_q(n.pred[b], n.y[n.rows[b]], &d);
    if (n.delta) n.delta[b] = ht_mul(d, n.scale);
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
    if (n.loss_out) *n.loss_out = ht_div(q_s[0], (float)n.B);
    if (n.status) *n.status = (p.first ? 0 : *n.status) | f_s[0];
  }
}

// ---- backward of one layer: wgrad tiles [0, n_wgrad), then dgrad tiles ----------------------------------------------------------------
struct HtBwdNet {
  const float* delta;                                    // delta_l [B, out]
  const float* aprev; int64_t lda; const int32_t* rows;  // A_{l-1} [B, in]; rows: layer 0's gather of the table
  const float* W; float* gW; float* gb;
  float* dprev;                                          // delta_{l-1} [B, in], NULL for layer 0
  double* partials;                                      // this layer's norm partials, one per wgrad tile
  int B;
};
struct HtBwd {
  HtBwdNet net[HT_NETS_MAX];
  int ldd, ldp, in, out, n_wgrad, dvec;
};

__global__ __launch_bounds__(ET_NT) void ht_backward_kernel(HtBwd p) {
  __shared__ float red[ET_WAVES][ET_TILE * ET_RS];
  __shared__ float runs[ET_BIAS_RUNS][ET_TILE];
  __shared__ double sq[ET_NT];
  const HtBwdNet& q = p.net[blockIdx.y];
  if (q.B == 0) return;
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
      const float gn = et_tile_total(red, e);
      q.gW[(int64_t)oo * p.in + ii] = gn;
      s = s + (double)gn * (double)gn;
    }
    if (tn == 0 && (int)threadIdx.x < ET_TILE && tm * ET_TILE + (int)threadIdx.x < p.out) {
      const int oo = tm * ET_TILE + threadIdx.x;
      float total = runs[0][threadIdx.x];
#pragma unroll
      for (int i = 1; i < ET_BIAS_RUNS; ++i) total = total + runs[i][threadIdx.x];
      q.gb[oo] = total;
      s = s + (double)total * (double)total;
    }
    sq[threadIdx.x] = s;
    const double total = et_tree<double, ET_NT>(sq);
    if (threadIdx.x == 0) q.partials[blockIdx.x] = total;
  } else {
    // delta_{l-1}[b][i] = (sum_o delta[b][o] W[o][i]) (aprev[b][i] > 0): delta k-contiguous, W k-outer
    const int t = blockIdx.x - p.n_wgrad;
    const int tm = t / tn_n, tn = t % tn_n;
    if (tm * ET_TILE >= q.B) return;
    const int m = tm * ET_TILE + r, i = tn * ET_TILE + r;
    const EtOperand a = {m < q.B ? q.delta + (int64_t)m * p.ldd : nullptr, p.ldd, nullptr, p.dvec != 0};
    const EtOperand b = {i < p.in ? q.W + i : nullptr, p.in, nullptr, false};
    et_chain<true, false>(acc, a, b, p.out, wave, h);
    et_store_partial(red, acc, wave, lane);
    for (int e = threadIdx.x; e < ET_TILE * ET_TILE; e += ET_NT) {
      const int mm = tm * ET_TILE + (e >> 5), ii = tn * ET_TILE + (e & 31);
      if (mm >= q.B || ii >= p.in) continue;
      const float av = q.aprev[(int64_t)mm * q.lda + ii];
      q.dprev[(int64_t)mm * p.ldp + ii] = et_tile_total(red, e) * et_act_grad(av, false);
    }
  }
}

// ---- norm, clip and Adam ----------------------------------------------------------------------------------------------------------------
struct HtAdamNet {
  float* p; float* g; float* m; float* v;
  const double* partials;
  float* norm_out;       // this step's slot, or NULL
  float ss, s2;          // float(lr / (1 - beta1^t)), float(sqrt(1 - beta2^t)) of this network's t
  int active;            // 0: exhausted, nothing of it is touched and its step count stays
};
struct HtAdamArgs {
  HtAdamNet net[HT_NETS_MAX];
  HtAdam k;
  int64_t total;
  int n_partials;
  double max_norm;
};

__global__ __launch_bounds__(ET_NT) void ht_adam_kernel(HtAdamArgs p) {
  __shared__ double sq[ET_NT];
  const HtAdamNet& n = p.net[blockIdx.y];
  if (!n.active) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < p.n_partials; i += ET_NT) s = s + n.partials[i];
  sq[threadIdx.x] = s;
  double norm;
  const float c = (float)et_clip_coefficient(et_tree<double, ET_NT>(sq), p.max_norm, &norm);
  if (blockIdx.x == 0 && threadIdx.x == 0 && n.norm_out) *n.norm_out = (float)norm;
  const int64_t e0 = (int64_t)blockIdx.x * ET_UPDATE_PER_WG;
  for (int i = 0; i < ET_UPDATE_PER_WG / ET_NT; ++i) {
    const int64_t e = e0 + (int64_t)i * ET_NT + threadIdx.x;
    if (e < p.total) ht_adam_update(n.p + e, n.g + e, n.m + e, n.v + e, c, n.ss, n.s2, p.k);
  }
}

static bool ht_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ht_steps(c) steps of every network (c.train == 0: forward and loss only), all enqueued on `stream`; nothing is read back
int launch_heads_train(const HtCall& c, void* workspace, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const HtDims d = ht_dims(c.R);
  const HtWorkspace ws = ht_workspace(c.R, c.batch);
  const HtAdam k = ht_adam_constants(c.weight_decay);
  const unsigned nets = (unsigned)c.n_nets;
  char* base[HT_NETS_MAX];
  for (int i = 0; i < c.n_nets; ++i) base[i] = static_cast<char*>(workspace) + (size_t)i * ws.net_bytes;
  const auto fbuf = [&](int i, size_t off) { return reinterpret_cast<float*>(base[i] + off); };
  const int64_t steps = ht_steps(c);
  for (int64_t step = 0; step < steps; ++step) {
    int B[HT_NETS_MAX], Bmax = 0;
    for (int i = 0; i < c.n_nets; ++i) {
      B[i] = ht_batch_rows(c, i, step);
      Bmax = B[i] > Bmax ? B[i] : Bmax;
    }
    const int64_t s0 = step * c.batch;
    for (int l = 0; l < HT_LAYERS; ++l) {
      HtFwd f{};
      f.slot0 = s0; f.K = d.in[l]; f.Nout = d.out[l]; f.ldo = ws.ld[l]; f.relu = l < HT_LAYERS - 1; f.gather = l == 0;
      f.wvec = d.in[l] % 4 == 0;   // params is 16-byte aligned and every w_off is a multiple of four floats
      for (int i = 0; i < c.n_nets; ++i) {
        const HtNet& a = c.net[i];
        HtFwdNet& q = f.net[i];
        q.A = l == 0 ? a.x : fbuf(i, ws.act[l - 1]); q.lda = l == 0 ? a.ldx : ws.ld[l - 1];
        q.order = a.order; q.N = a.N; q.rows = reinterpret_cast<int32_t*>(base[i] + ws.rows);
        q.W = a.params + d.w_off[l]; q.bias = a.params + d.b_off[l]; q.out = fbuf(i, ws.act[l]);
        q.B = B[i];
        q.avec = l == 0 ? (a.ldx % 4 == 0 && c.R % 4 == 0 && ht_aligned16(a.x)) : 1;
      }
      hipLaunchKernelGGL(ht_forward_kernel, dim3((unsigned)(et_tiles(Bmax) * et_tiles(d.out[l])), nets), dim3(ET_NT), 0, st, f);
    }
    HtLoss q{};
    q.slot0 = s0; q.first = step == 0;
    for (int i = 0; i < c.n_nets; ++i) {
      const HtNet& a = c.net[i];
      HtLossNet& n = q.net[i];
      n.pred = fbuf(i, ws.act[HT_LAYERS - 1]); n.rows = reinterpret_cast<const int32_t*>(base[i] + ws.rows);
      n.order = a.order; n.N = a.N; n.y = a.y;
      n.delta = c.train ? fbuf(i, ws.delta[HT_LAYERS - 1]) : nullptr;
      n.loss_out = a.loss_out ? a.loss_out + step : nullptr;
      n.status = a.status; n.B = B[i]; n.scale = B[i] ? (float)(2.0 / B[i]) : 0.0f;
    }
    hipLaunchKernelGGL(ht_loss_kernel, dim3(1, nets), dim3(ET_BATCH_MAX), 0, st, q);
    if (c.train) {
      for (int l = HT_LAYERS - 1; l >= 0; --l) {
        HtBwd b{};
        b.ldd = ws.ld[l]; b.ldp = l == 0 ? 0 : ws.ld[l - 1]; b.in = d.in[l]; b.out = d.out[l];
        b.n_wgrad = et_tiles(d.out[l]) * et_tiles(d.in[l]); b.dvec = ws.ld[l] % 4 == 0;
        for (int i = 0; i < c.n_nets; ++i) {
          const HtNet& a = c.net[i];
          HtBwdNet& n = b.net[i];
          n.delta = fbuf(i, ws.delta[l]);
          n.aprev = l == 0 ? a.x : fbuf(i, ws.act[l - 1]); n.lda = l == 0 ? a.ldx : ws.ld[l - 1];
          n.rows = l == 0 ? reinterpret_cast<const int32_t*>(base[i] + ws.rows) : nullptr;
          n.W = a.params + d.w_off[l]; n.gW = a.grads + d.w_off[l]; n.gb = a.grads + d.b_off[l];
          n.dprev = l == 0 ? nullptr : fbuf(i, ws.delta[l - 1]);
          n.partials = reinterpret_cast<double*>(base[i] + ws.partials) + d.part_off[l];
          n.B = B[i];
        }
        const int n_dgrad = l == 0 ? 0 : et_tiles(Bmax) * et_tiles(d.in[l]);
        hipLaunchKernelGGL(ht_backward_kernel, dim3((unsigned)(b.n_wgrad + n_dgrad), nets), dim3(ET_NT), 0, st, b);
      }
      HtAdamArgs u{};
      u.k = k; u.total = d.total; u.n_partials = d.n_partials; u.max_norm = c.max_norm;
      for (int i = 0; i < c.n_nets; ++i) {
        const HtNet& a = c.net[i];
        HtAdamNet& n = u.net[i];
        n.p = a.params; n.g = a.grads; n.m = a.m; n.v = a.v;
        n.partials = reinterpret_cast<const double*>(base[i] + ws.partials);
        n.norm_out = a.norm_out ? a.norm_out + step : nullptr;
        n.active = B[i] > 0;
        if (n.active) ht_adam_step_scales(c.lr, a.step0 + step + 1, &n.ss, &n.s2);
      }
      hipLaunchKernelGGL(ht_adam_kernel, dim3((unsigned)((d.total + ET_UPDATE_PER_WG - 1) / ET_UPDATE_PER_WG), nets), dim3(ET_NT), 0, st, u);
    }
    if (int rc = hip_launch_status()) return rc;
  }
  return 0;
}

}  // namespace nlml
