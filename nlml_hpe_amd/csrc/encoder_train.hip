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
//
// The forward and the backward kernels and the loops that launch them (mlp_launch_forward, mlp_launch_backward) serve K10
// (heads_train.hip) as well: there blockIdx.y is the network, each with its own row of the launch's argument table; K9 is the case of
// one network, whose kernels take the same fields flat.  The tile bodies, the loss kernels' tail and the update kernels' prologue are encoder_train_dev.h's.
#include <hip/hip_runtime.h>

#include "abi_internal.h"
#include "encoder_train_dev.h"
#include "encoder_train_ref.h"

namespace nlml {

// One body, two thin kernels each.  The table kernels take up to MLP_NETS_MAX views, indexed by blockIdx.y.  The kernels of a launch
// of ONE network (K9, and a K10 call of one network) take the same fields flat, in the order K9's kernels had them before the body was
// shared, so that they compile to that code: one kernel over the table for both, or the view and the shared fields as they lie in
// the table, left the kernel's argument loads scattered over later waits and cost K9 0.6-3 % of a step (profiles/mlp_train_one_body.md).
struct EtFwd {
  const float* A; int64_t lda; const int32_t* order; int64_t slot0, N; int gather; int32_t* rows;
  const float* W; const float* bias; float* out; int ldo, B, K, Nout, act, avec, wvec;
};
struct EtBwd {
  const float* delta; int ldd; const float* aprev; int64_t lda; const int32_t* rows; const float* W; float* gW; float* gb;
  float* dprev; int ldp; double* partials; int B, in, out, zero_grad, tanh_prev, n_wgrad, dvec;
};
static EtFwd et_flat(const MlpFwdNet& q, const MlpFwdShared& s) {
  return {q.A, q.lda, q.order, s.slot0, q.N, s.gather, q.rows, q.W, q.bias, q.out, s.ldo, q.B, s.K, s.Nout, s.act, q.avec, s.wvec};
}
static EtBwd et_flat(const MlpBwdNet& q, const MlpBwdShared& s) {
  return {q.delta, s.ldd, q.aprev, q.lda, q.rows, q.W, q.gW, q.gb, q.dprev, s.ldp, q.partials, q.B, s.in, s.out, s.zero_grad, s.tanh_prev,
          s.n_wgrad, s.dvec};
}
__global__ __launch_bounds__(ET_NT) void et_forward_kernel(EtFwd p) {
  mlp_forward_tile(MlpFwdNet{p.A, p.lda, p.order, p.N, p.rows, p.W, p.bias, p.out, p.B, p.avec},
                   MlpFwdShared{p.slot0, p.K, p.Nout, p.ldo, p.act, p.gather, p.wvec}, false);
}
__global__ __launch_bounds__(ET_NT) void et_backward_kernel(EtBwd p) {
  mlp_backward_tile(MlpBwdNet{p.delta, p.aprev, p.lda, p.rows, p.W, p.gW, p.gb, p.dprev, p.partials, p.B},
                    MlpBwdShared{p.ldd, p.ldp, p.in, p.out, p.zero_grad, p.tanh_prev, p.n_wgrad, p.dvec}, false);
}
__global__ __launch_bounds__(ET_NT) void mlp_forward_kernel(MlpFwd p) { mlp_forward_tile(p.net[blockIdx.y], p.s, true); }
__global__ __launch_bounds__(ET_NT) void mlp_backward_kernel(MlpBwd p) { mlp_backward_tile(p.net[blockIdx.y], p.s, true); }

// the vector flags only pick the load width: a row stride of whole 16 bytes from a 16-byte aligned base (params, grads and the
// workspace are aligned by the ABI's checks, and every w_off and workspace offset is a multiple of four floats)
static bool mlp_vec(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }
static float* mlp_f32(const MlpLaunchNet& a, size_t off) { return reinterpret_cast<float*>(a.block + off); }
static int mlp_bmax(const MlpLaunchNet* nets, int n_nets) {
  int Bmax = 0;
  for (int i = 0; i < n_nets; ++i) Bmax = nets[i].B > Bmax ? nets[i].B : Bmax;
  return Bmax;
}

// one launch per layer, the grid sized for the largest batch of the step
void mlp_launch_forward(const MlpDims& d, const MlpWorkspace& ws, const MlpLaunchNet* nets, int n_nets, int64_t slot0, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Bmax = mlp_bmax(nets, n_nets);
  for (int l = 0; l < d.layers; ++l) {
    MlpFwd f{};
    f.s.slot0 = slot0; f.s.K = d.in[l]; f.s.Nout = d.out[l]; f.s.ldo = ws.ld[l]; f.s.act = mlp_act(d, l); f.s.gather = l == 0;
    f.s.wvec = d.in[l] % 4 == 0;
    for (int i = 0; i < n_nets; ++i) {
      const MlpLaunchNet& a = nets[i];
      MlpFwdNet& q = f.net[i];
      q.A = l == 0 ? a.x : mlp_f32(a, ws.act[l - 1]); q.lda = l == 0 ? a.ldx : ws.ld[l - 1];
      q.order = a.order; q.N = a.N; q.rows = reinterpret_cast<int32_t*>(a.block + ws.rows);
      q.W = a.params + d.w_off[l]; q.bias = a.params + d.b_off[l]; q.out = mlp_f32(a, ws.act[l]);
      q.B = a.B; q.avec = mlp_vec(q.A, q.lda);
    }
    const dim3 grid((unsigned)(et_tiles(Bmax) * et_tiles(d.out[l])), (unsigned)n_nets);
    if (n_nets == 1) hipLaunchKernelGGL(et_forward_kernel, grid, dim3(ET_NT), 0, st, et_flat(f.net[0], f.s));
    else hipLaunchKernelGGL(mlp_forward_kernel, grid, dim3(ET_NT), 0, st, f);
  }
}

void mlp_launch_backward(const MlpDims& d, const MlpWorkspace& ws, const MlpLaunchNet* nets, int n_nets, int zero_grad, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int Bmax = mlp_bmax(nets, n_nets);
  for (int l = d.layers - 1; l >= 0; --l) {
    MlpBwd b{};
    b.s.ldd = ws.ld[l]; b.s.ldp = l == 0 ? 0 : ws.ld[l - 1]; b.s.in = d.in[l]; b.s.out = d.out[l];
    b.s.zero_grad = zero_grad; b.s.tanh_prev = l - 1 == d.tanh_layer;
    b.s.n_wgrad = et_tiles(d.out[l]) * et_tiles(d.in[l]); b.s.dvec = ws.ld[l] % 4 == 0;
    for (int i = 0; i < n_nets; ++i) {
      const MlpLaunchNet& a = nets[i];
      MlpBwdNet& n = b.net[i];
      n.delta = mlp_f32(a, ws.delta[l]);
      n.aprev = l == 0 ? a.x : mlp_f32(a, ws.act[l - 1]); n.lda = l == 0 ? a.ldx : ws.ld[l - 1];
      n.rows = l == 0 ? reinterpret_cast<const int32_t*>(a.block + ws.rows) : nullptr;
      n.W = a.params + d.w_off[l]; n.gW = a.grads + d.w_off[l]; n.gb = a.grads + d.b_off[l];
      n.dprev = l == 0 ? nullptr : mlp_f32(a, ws.delta[l - 1]);
      n.partials = reinterpret_cast<double*>(a.block + ws.partials) + d.part_off[l];
      n.B = a.B;
    }
    const int n_dgrad = l == 0 ? 0 : et_tiles(Bmax) * et_tiles(d.in[l]);
    const dim3 grid((unsigned)(b.s.n_wgrad + n_dgrad), (unsigned)n_nets);
    if (n_nets == 1) hipLaunchKernelGGL(et_backward_kernel, grid, dim3(ET_NT), 0, st, et_flat(b.net[0], b.s));
    else hipLaunchKernelGGL(mlp_backward_kernel, grid, dim3(ET_NT), 0, st, b);
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
  et_loss_tail(q, flags, (float)(3 * p.B), p.loss_out, p.status, p.first);
}

// ---- norm, clip and update ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ET_NT) void et_update_kernel(float* __restrict__ params, float* __restrict__ grads, int64_t total,
                                                          const double* __restrict__ partials, int n_partials, float lr, float wd,
                                                          double max_norm, float* norm_out) {
  const float c = et_clip_prologue(partials, n_partials, max_norm, norm_out);
  const int64_t e0 = (int64_t)blockIdx.x * ET_UPDATE_PER_WG;
  for (int i = 0; i < ET_UPDATE_PER_WG / ET_NT; ++i) {
    const int64_t e = e0 + (int64_t)i * ET_NT + threadIdx.x;
    if (e < total) et_update(params + e, grads + e, c, lr, wd);
  }
}

// ceil(n / batch) steps (c.grads == NULL: forward and loss only), all enqueued on `stream`; nothing is read back
int launch_encoder_train(const EtCall& c, void* workspace, void* stream) {
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const MlpDims d = et_dims(c.F);
  const MlpWorkspace ws = et_workspace(c.F, c.batch);
  MlpLaunchNet net = {c.x, c.ldx, c.N, c.order, c.params, c.grads, static_cast<char*>(workspace), 0};
  double* partials = reinterpret_cast<double*>(net.block + ws.partials);
  int64_t step = 0;
  for (int64_t s0 = 0; s0 < c.n; s0 += c.batch, ++step) {
    net.B = (int)(c.n - s0 < c.batch ? c.n - s0 : c.batch);
    mlp_launch_forward(d, ws, &net, 1, s0, stream);
    EtLoss q{};
    q.pred = mlp_f32(net, ws.act[5]); q.rows = reinterpret_cast<const int32_t*>(net.block + ws.rows);
    q.order = c.order; q.slot0 = s0; q.N = c.N; q.labels = c.labels; q.ld_lab = c.ld_lab;
    for (int t = 0; t < 3; ++t) { q.table[t] = c.table[t]; q.nrows[t] = c.rows[t]; }
    q.delta = c.grads ? mlp_f32(net, ws.delta[5]) : nullptr;
    q.loss_out = c.loss_out ? c.loss_out + step : nullptr;
    q.status = c.status; q.first = step == 0; q.B = net.B; q.scale = (float)(2.0 / (3.0 * net.B));
    hipLaunchKernelGGL(et_loss_kernel, dim3(1), dim3(ET_BATCH_MAX), 0, st, q);
    if (c.grads) {
      mlp_launch_backward(d, ws, &net, 1, c.zero_grad, stream);
      hipLaunchKernelGGL(et_update_kernel, dim3((unsigned)((d.total + ET_UPDATE_PER_WG - 1) / ET_UPDATE_PER_WG)), dim3(ET_NT), 0, st,
                         c.params, c.grads, d.total, partials, d.n_partials, c.lr, c.wd, c.max_norm,
                         c.norm_out ? c.norm_out + step : nullptr);
    }
    if (int rc = hip_launch_status()) return rc;
  }
  return 0;
}

}  // namespace nlml
