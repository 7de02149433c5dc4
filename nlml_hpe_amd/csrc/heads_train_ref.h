// heads_train_ref.h -- K10: one training step of the yaw, pitch and roll heads, its operation order stated once for host and device.
//
// The reference trains three independent networks (NLML_HPE_MLPHeadsTrainer.py:26-126), each
//   Linear(R,128) ReLU Linear(128,256) ReLU Linear(256,128) ReLU Linear(128,64) ReLU Linear(64,1)
// on (row of the cosine table, angle in radians): zero_grad, forward, MSELoss (the mean over the B outputs), backward,
// clip_grad_norm_(max_norm 1), Adam(weight_decay as L2 added to the gradient, not AdamW).  Up to HT_NETS_MAX networks share every
// launch of a call (blockIdx.y is the network); each has its own data, parameters, Adam state, visiting order and row count, and
// nothing of one network enters another.  Everything below is f32 unless it says f64.
//
// THE GEMM ORDER is K9's, unchanged (encoder_train_ref.h): 32 x 32 tiles, eight waves over super-chunks of 16, k = 16 s + 8 u + 4 h + j,
//   p_w = fmaf(a_k, b_k, p_w) from +0 (wave 0 of a forward tile: from the bias), the partial tiles added in wave order; an index
//   k >= K of a visited super-chunk, a row or a column beyond the matrix is an exact ZERO OPERAND (fmaf(0, 0, p)), a wave without a
//   super-chunk contributes +0.  Layer 0 has K = R <= 16: one super-chunk, waves 1..7 empty.  The three products of layer l:
//       forward   Z_l[b][o]         = sum_k A_{l-1}[b][k] W_l[o][k] + b_l[o]             K = in;   A_l = max(Z_l, 0) for l < 4, A_5 = Z_4 = pred
//       wgrad     dW_l[o][i]        = sum_b delta_l[b][o] A_{l-1}[b][i]                  K = B
//       dgrad     delta_{l-1}[b][i] = (sum_o delta_l[b][o] W_l[o][i]) * (A_{l-1}[b][i] > 0)   K = out (layer 4: K = 1); none for layer 0
//   G = dW: the gradient is always overwritten (the reference zeroes it before every step).
// THE OTHER ORDERS -- every operation below is rounded on its own (no fused multiply-add anywhere: ht_mul, ht_add, .. below), so
// separately rounded numpy float32 / float64 scalars reproduce them:
//   bias     K9's: db_l[o] in ET_BIAS_RUNS = 16 runs of ceil(B/16) rows, a run summed b ascending from +0, the runs added in order.
//   loss     row b: d = pred_b - y_b, q_b = d * d; the q_b (slots b >= B hold +0) through K9's halving tree over 256 slots
//            (slot t += slot t + stride, stride 128, 64, .. 1); loss = total / float(B); delta_5[b] = d * float(2.0 / B).
//   norm     f64, K9's way.  A wgrad tile's 512 threads each take the squares of their G (elements t and t + 512 of the tile,
//            row-major; thread o < 32 of a first-column tile then its G_b) as K9's s = fma(g, g, s) (the product of two f32 is exact in
//            f64, so s + g * g rounded separately is the same number);
//            a halving tree over the 512 slots gives the tile's partial.  The 78 partials (layer 0's tiles first, row-major: 4, 32, 32,
//            8, 2 tiles) are summed by 512 strided chains (i = t, t + 512, ..) and the same tree; n = sqrt(total),
//            c = min(1, max_norm / (n + 1e-6))  (et_clip_coefficient).
//   Adam     torch's single-tensor order.  With w1 = float(1 - beta1), b2 = float(beta2), w2 = float(1 - beta2), wd = float(weight_decay),
//            eps = float(1e-8) and, computed by the launcher on the host in double for the network's step count t (its steps so far + 1),
//            ss = float(lr / (1 - beta1^t)), s2 = float(sqrt(1 - beta2^t)):
//                g1 = float(c) * g;   g2 = g1 + wd * p;   m' = m + w1 * (g2 - m);   v' = b2 * v + w2 * (g2 * g2);
//                den = sqrt(v') / s2 + eps;   p' = p - ss * (m' / den)
//            and g is stored as g1 (clip_grad_norm_ scales in place).  beta1 = 0.9, beta2 = 0.999.
//
// The host form (ht_host_*, below; nlml_heads_train_steps_host) runs this order in plain C++ and, with no tanhf in this network, IS
// claimed to return the device's bits: every word of the parameters, the state, the losses and the workspace.
//
// What is written here is what differs from K9: the network (HT_SHAPE), the loss, Adam and the steps of a call.  The dims and the
// workspace layout, the forward, wgrad, dgrad and norm of the host form (mlp_host_*, called with pad = true and zero_grad = 1) and of
// the device (mlp_forward_kernel, mlp_backward_kernel, the loss tail, the clip prologue) are encoder_train_ref.h's, encoder_train_dev.h's
// and encoder_train.hip's.
#pragma once
#include "encoder_train_ref.h"

namespace nlml {

constexpr int HT_LAYERS = 5;
constexpr int HT_NETS_MAX = MLP_NETS_MAX; // NLML_HEADS_TRAIN_NETS_MAX
constexpr int HT_R_MAX = 16;             // NLML_HEADS_TRAIN_R_MAX
constexpr int HT_STATUS_ORDER = 1;       // NLML_HEADS_TRAIN_CLAMPED_ORDER
constexpr double HT_BETA1 = 0.9, HT_BETA2 = 0.999, HT_EPS = 1e-8;

// the network, its dims and its workspace are K9's structs (encoder_train_ref.h); network i of a call owns the workspace block
// [i net_bytes, (i + 1) net_bytes), every A_l and delta_l dense
constexpr MlpShape HT_SHAPE = {HT_LAYERS, {128, 256, 128, 64, 1}, -1, 1};
ET_HD MlpDims ht_dims(int R) { return mlp_dims(HT_SHAPE, R); }
ET_HD MlpWorkspace ht_workspace(int R, int batch) { return mlp_workspace(ht_dims(R), batch); }

// ---- separately rounded f32 operations, the same text for both compilers.  The device's *_rn intrinsics are NOT used: without
// OCML_BASIC_ROUNDED_OPERATIONS the HIP headers define __fmul_rn(x, y) as x * y, which the device compiler's default
// -ffp-contract=fast-honor-pragmas may fuse with a following add, and __fsqrt_rn as the native (1 ulp) square root.  What holds on
// both sides is the pragma, which takes the `contract` flag off the operation, and sqrtf and /, which hipcc rounds correctly by
// default (-fhip-fp32-correctly-rounded-divide-sqrt) as x86 does.
ET_HD float ht_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
ET_HD float ht_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
ET_HD float ht_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
ET_HD float ht_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}
ET_HD float ht_sqrt(float a) { return sqrtf(a); }

// the constants of Adam as the kernels take them, and the two that depend on a network's step count t >= 1
struct HtAdam { float w1, b2, w2, wd, eps; };
ET_HD HtAdam ht_adam_constants(double weight_decay) {
  HtAdam k;
  k.w1 = (float)(1.0 - HT_BETA1); k.b2 = (float)HT_BETA2; k.w2 = (float)(1.0 - HT_BETA2); k.wd = (float)weight_decay; k.eps = (float)HT_EPS;
  return k;
}
static inline void ht_adam_step_scales(double lr, int64_t t, float* ss, float* s2) {
  *ss = (float)(lr / (1.0 - pow(HT_BETA1, (double)t)));
  *s2 = (float)sqrt(1.0 - pow(HT_BETA2, (double)t));
}
ET_HD float ht_loss_q(float pred, float y, float* d) {
  *d = ht_sub(pred, y);
  return ht_mul(*d, *d);
}
ET_HD void ht_adam_update(float* p, float* g, float* m, float* v, float c, float ss, float s2, const HtAdam& k) {
  const float g1 = ht_mul(c, *g);
  const float g2 = ht_add(g1, ht_mul(k.wd, *p));
  const float mn = ht_add(*m, ht_mul(k.w1, ht_sub(g2, *m)));
  const float vn = ht_add(ht_mul(k.b2, *v), ht_mul(k.w2, ht_mul(g2, g2)));
  const float den = ht_add(ht_div(ht_sqrt(vn), s2), k.eps);
  *p = ht_sub(*p, ht_mul(ss, ht_div(mn, den)));
  *g = g1; *m = mn; *v = vn;
}

// one network of a call (the layout of include/nlml_hpe.h's nlml_heads_net) and the call, already checked (abi.cpp, "K10 argument checks")
struct HtNet {
  const float* x; int64_t ldx, N;       // the table's rows f32[N,ldx], R columns used
  const float* y;                       // the targets f32[N]
  float* params; float* grads; float* m; float* v;   // f32[ht_dims(R).total] each; the last three unused by the evaluation pass
  const int32_t* order; int64_t n;      // the rows in visiting order (NULL: 0..n-1)
  int64_t step0;                        // Adam steps this network has taken before the call
  float* loss_out; float* norm_out; int32_t* status;
};
struct HtCall {
  HtNet net[HT_NETS_MAX];
  int n_nets, R, batch, train;
  double lr, weight_decay, max_norm;
};
// the steps of a call: the most any network needs; network i takes part in the first ceil(n_i / batch) of them
static inline int64_t ht_steps(const HtCall& c) {
  int64_t steps = 0;
  for (int i = 0; i < c.n_nets; ++i) {
    const int64_t s = (c.net[i].n + c.batch - 1) / c.batch;
    steps = s > steps ? s : steps;
  }
  return steps;
}
// rows of network i's batch at step s (0: the network is exhausted)
static inline int ht_batch_rows(const HtCall& c, int i, int64_t s) {
  const int64_t left = c.net[i].n - s * c.batch;
  return (int)(left < 0 ? 0 : (left < c.batch ? left : c.batch));
}

}  // namespace nlml

// ---- the host form ---------------------------------------------------------------------------------------------------------------
namespace nlml {

// one batch of one network into its workspace block `wsb`: forward, loss, and (c.train) backward, norm and Adam with step count t.
// The shared part (mlp_host_*, encoder_train_ref.h) with pad = true: the device's zero operands.
static inline void ht_host_step(const HtCall& c, int i, int64_t slot0, int B, int64_t t, char* wsb, float* loss, float* norm_out, int* status) {
  const HtNet& a = c.net[i];
  const MlpDims d = ht_dims(c.R);
  const MlpHostWs v = mlp_host_ws(d, c.batch, wsb);
  const bool clamped = mlp_host_rows(v, a.order, slot0, a.N, B);
  if (status && clamped) *status |= HT_STATUS_ORDER;
  const EtHostMat X = {a.x, a.ldx, v.rows};
  mlp_host_forward(d, v, X, a.params, B, true);
  // residual and loss
  const float scale = (float)(2.0 / B);
  float slots[ET_BATCH_MAX];
  for (int b = 0; b < ET_BATCH_MAX; ++b) slots[b] = 0.0f;
  for (int b = 0; b < B; ++b) {
    float dd;
    slots[b] = ht_loss_q(v.act[HT_LAYERS - 1][b], a.y[v.rows[b]], &dd);
    if (c.train) v.delta[HT_LAYERS - 1][b] = ht_mul(dd, scale);
  }
  *loss = ht_div(et_host_tree<float, ET_BATCH_MAX>(slots), (float)B);
  if (!c.train) return;
  mlp_host_dgrad(d, v, a.params, B, true);
  mlp_host_wgrad(d, v, X, a.grads, B, 1, true);
  double norm;
  const float cc = mlp_host_clip(d, v, c.max_norm, &norm);
  if (norm_out) *norm_out = (float)norm;
  const HtAdam k = ht_adam_constants(c.weight_decay);
  float ss, s2;
  ht_adam_step_scales(c.lr, t, &ss, &s2);
  for (int64_t e = 0; e < d.total; ++e) ht_adam_update(a.params + e, a.grads + e, a.m + e, a.v + e, cc, ss, s2, k);
}

// every step of a call, network after network; workspace: the caller's (the layout above) or NULL
static inline void ht_host_run(const HtCall& c, void* workspace) {
  const MlpWorkspace ws = ht_workspace(c.R, c.batch);
  std::vector<char> own;
  if (!workspace) {
    own.assign(ws.net_bytes * c.n_nets, 0);
    workspace = own.data();
  }
  for (int i = 0; i < c.n_nets; ++i)
    if (c.net[i].status) *c.net[i].status = 0;
  const int64_t steps = ht_steps(c);
  for (int64_t s = 0; s < steps; ++s)
    for (int i = 0; i < c.n_nets; ++i) {
      const int B = ht_batch_rows(c, i, s);
      if (B == 0) continue;
      float loss = 0.0f, norm = 0.0f;
      ht_host_step(c, i, s * c.batch, B, c.net[i].step0 + s + 1, static_cast<char*>(workspace) + (size_t)i * ws.net_bytes, &loss, &norm,
                   c.net[i].status);
      if (c.net[i].loss_out) c.net[i].loss_out[s] = loss;
      if (c.train && c.net[i].norm_out) c.net[i].norm_out[s] = norm;
    }
}

}  // namespace nlml
