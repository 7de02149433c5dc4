// heads_train.hip -- K10: training steps of the yaw, pitch and roll heads (NLML_HPE_MLPHeadsTrainer.py:83-126), a whole epoch of all
// networks enqueued at once.
//
// K9's shape (encoder_train.hip): a step is twelve launches ordered by the stream, nothing else -- five forward layers, the residual
// and loss, five backward layers (wgrad tiles and dgrad tiles are disjoint workgroup ranges of one launch; no dgrad for layer 0) and
// the norm/clip/Adam launch (every workgroup reduces the network's 78 norm partials itself, in the same order).  No atomics, no
// grid-wide barrier, no workgroup waits for another, nothing is read back.  The second grid dimension is used: blockIdx.y is
// the NETWORK.  No launch of this size runs under ~4.8 us whatever it computes (profiles/encoder_train.md), so the up to three
// independent networks of a call share every launch, each through its own row of the launch's argument table; a network whose rows
// are used up has B = 0 there, and its workgroups return before touching memory.  The operation order is heads_train_ref.h's.
// The forward and backward launches are K9's own kernels and launch loops (mlp_launch_forward, mlp_launch_backward: encoder_train.hip)
// with zero_grad = 1 and no Tanh; this file holds what differs: the residual and loss, Adam, and the steps' bookkeeping.
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "encoder_train_dev.h"
#include "heads_train_ref.h"

namespace nlml {

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
  et_loss_tail(q, flags, (float)n.B, n.loss_out, n.status, p.first);
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
  const HtAdamNet& n = p.net[blockIdx.y];
  if (!n.active) return;
  const float c = et_clip_prologue(n.partials, p.n_partials, p.max_norm, n.norm_out);
  const int64_t e0 = (int64_t)blockIdx.x * ET_UPDATE_PER_WG;
  for (int i = 0; i < ET_UPDATE_PER_WG / ET_NT; ++i) {
    const int64_t e = e0 + (int64_t)i * ET_NT + threadIdx.x;
    if (e < p.total) ht_adam_update(n.p + e, n.g + e, n.m + e, n.v + e, c, n.ss, n.s2, p.k);
  }
}

// ht_steps(c) steps of every network (c.train == 0: forward and loss only), all enqueued on `stream`; nothing is read back
int launch_heads_train(const HtCall& c, void* workspace, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const MlpDims d = ht_dims(c.R);
  const MlpWorkspace ws = ht_workspace(c.R, c.batch);
  const HtAdam k = ht_adam_constants(c.weight_decay);
  const unsigned nets = (unsigned)c.n_nets;
  MlpLaunchNet net[HT_NETS_MAX];
  for (int i = 0; i < c.n_nets; ++i) {
    const HtNet& a = c.net[i];
    net[i] = MlpLaunchNet{a.x, a.ldx, a.N, a.order, a.params, a.grads, static_cast<char*>(workspace) + (size_t)i * ws.net_bytes, 0};
  }
  const int64_t steps = ht_steps(c);
  for (int64_t step = 0; step < steps; ++step) {
    for (int i = 0; i < c.n_nets; ++i) net[i].B = ht_batch_rows(c, i, step);
    const int64_t s0 = step * c.batch;
    mlp_launch_forward(d, ws, net, c.n_nets, s0, stream);
    HtLoss q{};
    q.slot0 = s0; q.first = step == 0;
    for (int i = 0; i < c.n_nets; ++i) {
      const HtNet& a = c.net[i];
      HtLossNet& n = q.net[i];
      n.pred = reinterpret_cast<const float*>(net[i].block + ws.act[HT_LAYERS - 1]);
      n.rows = reinterpret_cast<const int32_t*>(net[i].block + ws.rows);
      n.order = a.order; n.N = a.N; n.y = a.y;
      n.delta = c.train ? reinterpret_cast<float*>(net[i].block + ws.delta[HT_LAYERS - 1]) : nullptr;
      n.loss_out = a.loss_out ? a.loss_out + step : nullptr;
      n.status = a.status; n.B = net[i].B; n.scale = n.B ? (float)(2.0 / n.B) : 0.0f;
    }
    hipLaunchKernelGGL(ht_loss_kernel, dim3(1, nets), dim3(ET_BATCH_MAX), 0, st, q);
    if (c.train) {
      mlp_launch_backward(d, ws, net, c.n_nets, 1, stream);
      HtAdamArgs u{};
      u.k = k; u.total = d.total; u.n_partials = d.n_partials; u.max_norm = c.max_norm;
      for (int i = 0; i < c.n_nets; ++i) {
        const HtNet& a = c.net[i];
        HtAdamNet& n = u.net[i];
        n.p = a.params; n.g = a.grads; n.m = a.m; n.v = a.v;
        n.partials = reinterpret_cast<const double*>(net[i].block + ws.partials);
        n.norm_out = a.norm_out ? a.norm_out + step : nullptr;
        n.active = net[i].B > 0;
        if (n.active) ht_adam_step_scales(c.lr, a.step0 + step + 1, &n.ss, &n.s2);
      }
      hipLaunchKernelGGL(ht_adam_kernel, dim3((unsigned)((d.total + ET_UPDATE_PER_WG - 1) / ET_UPDATE_PER_WG), nets), dim3(ET_NT), 0, st, u);
    }
    if (int rc = hip_launch_status()) return rc;
  }
  return 0;
}

}  // namespace nlml
