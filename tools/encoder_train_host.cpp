// Stand-alone host program for tests/test_encoder_train_host.py: the host forms of the two trainers' steps, which share their
// forward, backward and norm (csrc/encoder_train_ref.h, mlp_host_*), on tiny cases, built with -fsanitize=address,undefined and
// run directly.  Every buffer is a heap block of exactly its size, so a read or write past an end is reported.
//   K9  (et_host_run, the code behind nlml_encoder_train_steps_host / nlml_encoder_eval_losses_host): five rows of F = 136 with a
//       padded row stride, batches of three (so the second is partial), an order and a label out of range (clamped and flagged), a
//       gathered order, then the validation pass.
//   K10 (ht_host_run, csrc/heads_train_ref.h, behind nlml_heads_*_host): R = 3, two networks of 5 and 2 rows at batch 4 (a partial
//       second step for the first, the second exhausted in it), one training and one evaluation call, in the caller's workspace of
//       exactly workspace_bytes, so an overrun of a network's block is reported.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/encoder_train_host.cpp
#include <cmath>
#include <cstdio>
#include <vector>

#include "../nlml_hpe_amd/csrc/heads_train_ref.h"

using namespace nlml;

static unsigned g_state = 12345u;
static float uniform(float lo, float hi) {
  g_state = g_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * (float)(g_state >> 8) / 16777216.0f;
}
static std::vector<float> initial_params(const MlpDims& d) {
  std::vector<float> params(d.total);
  for (int l = 0; l < d.layers; ++l) {
    const float bound = 1.0f / std::sqrt((float)d.in[l]);
    for (int64_t e = d.w_off[l]; e < d.b_off[l] + d.out[l]; ++e) params[e] = uniform(-bound, bound);
  }
  return params;
}

static int encoder_case() {
  const int F = 136, N = 5, batch = 3, ld_lab = 3;
  const int64_t ldx = F + 3;
  const MlpDims d = et_dims(F);
  std::vector<float> x((size_t)(N - 1) * ldx + F), params = initial_params(d), grads(d.total, 0.0f);
  for (float& v : x) v = uniform(-2.0f, 2.0f);
  const int rows[3] = {11, 9, 7};
  std::vector<float> ty(11 * 3), tp(9 * 3), tr(7 * 3);
  for (std::vector<float>* t : {&ty, &tp, &tr})
    for (float& v : *t) v = uniform(-0.5f, 0.5f);
  std::vector<int32_t> labels = {0, 0, 0, 10, 8, 6, 5, 4, 3, 11 /* beyond the yaw table */, 2, 1, 3, -1 /* below */, 2};
  std::vector<int32_t> order = {4, 2, 7 /* beyond N */, 0, 1};
  std::vector<float> loss(2, -1.0f), norm(2, -1.0f);
  int32_t status = -1;

  EtCall c;
  c.x = x.data(); c.ldx = ldx; c.N = N; c.labels = labels.data(); c.ld_lab = ld_lab;
  c.table[0] = ty.data(); c.table[1] = tp.data(); c.table[2] = tr.data();
  for (int t = 0; t < 3; ++t) c.rows[t] = rows[t];
  c.params = params.data(); c.grads = grads.data(); c.F = F; c.batch = batch; c.order = order.data(); c.n = N;
  c.lr = 1e-3f; c.wd = 1e-5f; c.max_norm = 0.3; c.zero_grad = 0;
  c.loss_out = loss.data(); c.norm_out = norm.data(); c.status = &status;
  et_host_run(c);
  if (status != (ET_STATUS_ORDER | ET_STATUS_LABEL)) { std::printf("status %d\n", status); return 1; }
  for (int s = 0; s < 2; ++s)
    if (!(std::isfinite(loss[s]) && loss[s] > 0.0f && std::isfinite(norm[s]) && norm[s] > 0.0f)) { std::printf("step %d: %g %g\n", s, loss[s], norm[s]); return 1; }
  double sumsq = 0.0;
  for (float g : grads) sumsq += (double)g * g;
  if (!(std::sqrt(sumsq) <= 0.3 * (1.0 + 1e-5))) { std::printf("the accumulator is not clipped: %g\n", std::sqrt(sumsq)); return 1; }
  for (float p : params)
    if (!std::isfinite(p)) { std::printf("a parameter is not finite\n"); return 1; }

  // the validation pass: no order (the rows in turn), no gradients
  std::vector<float> vloss(2, -1.0f);
  c.grads = nullptr; c.order = nullptr; c.loss_out = vloss.data(); c.norm_out = nullptr;
  et_host_run(c);
  if (status != ET_STATUS_LABEL || !(vloss[0] > 0.0f && vloss[1] > 0.0f)) { std::printf("validation: status %d, %g %g\n", status, vloss[0], vloss[1]); return 1; }
  std::printf("losses %a %a norms %a %a validation %a %a\nencoder train host ok\n", loss[0], loss[1], norm[0], norm[1], vloss[0], vloss[1]);
  return 0;
}

static int heads_case() {
  const int R = 3, batch = 4, n_nets = 2, rows[2] = {5, 2};
  const MlpDims d = ht_dims(R);
  std::vector<float> x[2], y[2], params[2], grads[2], m[2], v[2], loss[2], norm[2];
  std::vector<int32_t> order0 = {3, 0, 9 /* beyond N */, 1, 4};
  int32_t status[2] = {-1, -1};
  HtCall c = {};
  c.n_nets = n_nets; c.R = R; c.batch = batch; c.train = 1; c.lr = 5e-3; c.weight_decay = 1e-5; c.max_norm = 1.0;
  for (int i = 0; i < n_nets; ++i) {
    x[i].resize((size_t)rows[i] * R); y[i].resize(rows[i]);
    for (float& e : x[i]) e = uniform(-1.0f, 1.0f);
    for (float& e : y[i]) e = uniform(-1.0f, 1.0f);
    params[i] = initial_params(d);
    grads[i].assign(d.total, 0.0f); m[i].assign(d.total, 0.0f); v[i].assign(d.total, 0.0f);
    loss[i].assign(i == 0 ? 2 : 1, -1.0f); norm[i].assign(i == 0 ? 2 : 1, -1.0f);
    c.net[i] = HtNet{x[i].data(), R, rows[i], y[i].data(), params[i].data(), grads[i].data(), m[i].data(), v[i].data(),
                     i == 0 ? order0.data() : nullptr, rows[i], 0, loss[i].data(), norm[i].data(), &status[i]};
  }
  std::vector<char> workspace(ht_workspace(R, batch).net_bytes * n_nets);   // workspace_bytes and not one byte more
  ht_host_run(c, workspace.data());
  if (status[0] != HT_STATUS_ORDER || status[1] != 0) { std::printf("heads status %d %d\n", status[0], status[1]); return 1; }
  for (int i = 0; i < n_nets; ++i) {
    for (size_t s = 0; s < loss[i].size(); ++s)
      if (!(std::isfinite(loss[i][s]) && loss[i][s] > 0.0f && std::isfinite(norm[i][s]) && norm[i][s] > 0.0f)) {
        std::printf("heads network %d step %zu: %g %g\n", i, s, loss[i][s], norm[i][s]);
        return 1;
      }
    for (float p : params[i])
      if (!std::isfinite(p)) { std::printf("heads: a parameter is not finite\n"); return 1; }
  }
  // the evaluation pass: no gradients, no state
  std::vector<float> eloss[2];
  c.train = 0;
  for (int i = 0; i < n_nets; ++i) {
    eloss[i].assign(i == 0 ? 2 : 1, -1.0f);
    c.net[i].grads = c.net[i].m = c.net[i].v = nullptr;
    c.net[i].order = nullptr; c.net[i].loss_out = eloss[i].data(); c.net[i].norm_out = nullptr;
  }
  ht_host_run(c, workspace.data());
  if (status[0] != 0 || status[1] != 0 || !(eloss[0][0] > 0.0f && eloss[0][1] > 0.0f && eloss[1][0] > 0.0f)) {
    std::printf("heads evaluation: status %d %d, %g %g %g\n", status[0], status[1], eloss[0][0], eloss[0][1], eloss[1][0]);
    return 1;
  }
  std::printf("heads losses %a %a %a evaluation %a %a %a\nheads train host ok\n", loss[0][0], loss[0][1], loss[1][0], eloss[0][0], eloss[0][1], eloss[1][0]);
  return 0;
}

int main() {
  if (int rc = encoder_case()) return rc;
  return heads_case();
}
