// Stand-alone host program for tests/test_encoder_train_host.py: the host form of the encoder's training steps
// (csrc/encoder_train_ref.h, the code behind nlml_encoder_train_steps_host / nlml_encoder_eval_losses_host) on a tiny case, built
// with -fsanitize=address,undefined and run directly.  Every buffer is a heap block of exactly its size, so a read or write past
// an end is reported: five rows of F = 136 with a padded row stride, batches of three (so the second is partial), an order and a
// label out of range (clamped and flagged), a gathered order, then the validation pass.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off tools/encoder_train_host.cpp
#include <cmath>
#include <cstdio>
#include <vector>

#include "../nlml_hpe_amd/csrc/encoder_train_ref.h"

using namespace nlml;

static unsigned g_state = 12345u;
static float uniform(float lo, float hi) {
  g_state = g_state * 1664525u + 1013904223u;
  return lo + (hi - lo) * (float)(g_state >> 8) / 16777216.0f;
}

int main() {
  const int F = 136, N = 5, batch = 3, ld_lab = 3;
  const int64_t ldx = F + 3;
  const EtDims d = et_dims(F);
  std::vector<float> x((size_t)(N - 1) * ldx + F), params(d.total), grads(d.total, 0.0f);
  for (float& v : x) v = uniform(-2.0f, 2.0f);
  for (int l = 0; l < ET_LAYERS; ++l) {
    const float bound = 1.0f / std::sqrt((float)d.in[l]);
    for (int64_t e = d.w_off[l]; e < d.b_off[l] + d.out[l]; ++e) params[e] = uniform(-bound, bound);
  }
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
