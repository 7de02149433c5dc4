// encoder_train_ref.h -- K9: one training step of the landmark encoder, its operation order stated once for host and device.
//
// The reference trains the encoder K2 runs (NLML_HPE_EncoderTrainer.py:294-539):
//   Linear(F,1024) ReLU Linear(1024,512) ReLU Linear(512,256) ReLU Linear(256,128) ReLU Linear(128,64) Tanh Linear(64,9)
// by SGD on  loss = sum (pred - t)^2 / (3B)  (three MSELoss means over B x 3 elements each), with NO zero_grad in its loop: the
// gradient accumulator G persists, G <- G + grad, is clipped IN PLACE (clip_grad_norm_, max_norm 20: c = min(1, 20 / (||G|| + 1e-6)),
// G <- c G) and p <- p - lr (G + wd p).  Everything below is f32 unless it says f64.
//
// THE GEMM ORDER (every matrix product of a step; encoder_train.hip runs it on v_mfma_f32_32x32x2_f32, which is an fmaf chain):
//   The output is cut into 32 x 32 tiles, one workgroup of ET_WAVES waves each.  The reduction index k = 0..K-1 is cut into
//   super-chunks of 16; wave w owns the super-chunks [w spw, (w+1) spw), spw = ceil(ceil(K/16) / ET_WAVES).  Inside a super-chunk s
//   the wave visits
//       k = 16 s + 8 u + 4 h + j      for u = 0, 1;  j = 0..3;  h = 0, 1   (h innermost: one MFMA takes the pair h = 0, 1)
//   i.e. 0,4,1,5,2,6,3,7, 8,12,9,13,... and forms  p_w = fmaf(a_k, b_k, p_w)  from p_w = +0 (wave 0 of a forward tile: from the bias).
//   An index k >= K, a row or a column beyond the matrix is an exact zero operand.  The tile's value is ((p_0 + p_1) + p_2) + ... in
//   wave order, through LDS.  The three products of layer l (A_0 = the gathered batch rows, A_l its post-activation output):
//       forward   Z_l[b][o]        = sum_k A_{l-1}[b][k] W_l[o][k] + b_l[o]                  K = in
//       wgrad     dW_l[o][i]       = sum_b delta_l[b][o] A_{l-1}[b][i]                       K = B (the batch)
//       dgrad     delta_{l-1}[b][i] = (sum_o delta_l[b][o] W_l[o][i]) * act'(A_{l-1}[b][i])  K = out;  ReLU: a > 0, Tanh: 1 - a a
//   then G (+)= dW: G_new = G_old + dW (zero_grad: G_new = dW).
// THE OTHER SUMS
//   bias     db_l[o]: the batch is cut into ET_NT/32 = 16 runs of ceil(B/16) rows; a run is summed b ascending from +0, the runs are
//            added in order; G_b (+)= db as above.
//   loss     row b: q_b = fmaf(d, d, q_b) over its nine d = pred - t, j ascending; the rows through a halving tree over 256 slots
//            (slot t += slot t + stride, stride 128, 64, .. 1); loss = total / float(3B); delta_6 = d * float(2 / (3B)).
//   norm     f64.  A wgrad tile's 512 threads each take the squares of their G_new (elements t and t + 512 of the tile, row-major;
//            thread o < 32 of a first-column tile then its G_b) as s = fma(g, g, s); a halving tree over the 512 slots gives the
//            tile's partial.  All partials (layer 0's tiles first, row-major) are summed by 512 strided chains (i = t, t + 512, ..)
//            and the same tree; n = sqrt(total), c = min(1, max_norm / (n + 1e-6)).
//   update   g = float(c) * g;  d = fmaf(wd, p, g);  p = fmaf(-lr, d, p).
//
// The host form (et_host_*, below; nlml_encoder_train_steps_host) runs this order in plain C++.  It is NOT claimed to return the
// device's bits: tanhf is ocml's on the device and glibc's on the host, and a skipped k >= K differs from fmaf(0, 0, p) in the sign
// of a zero.  The device IS held to this prose bit for bit, launch by launch: the C oracle restates the order apart from this file
// (oracle/csrc/oracle.c "K9", k >= K as a zero operand), tests/test_encoder_train_order_host.py holds that model to the host form's
// values, to float64 and to deliberately wrong orders, and tests/test_encoder_train_order_gpu.py holds every launch of a step to it on
// the device's own inputs (A_5 alone to 5 ulp of float64 tanh).
//
// K10 (heads_train_ref.h, the yaw, pitch and roll heads) is the same design on another network, so what the two share is written here
// once, over a description of the network (MlpShape: layer count, widths, which layer's output goes through Tanh, the last layer's row
// stride in the workspace): the dims and the workspace layout (mlp_dims, mlp_workspace), and the host form's row resolution, forward,
// dgrad, wgrad + bias + norm partials and norm (mlp_host_*), which write into a workspace block in the device's layout.  K9 is
// ET_SHAPE, one network, pad = false, zero_grad from the call; its own part is the residual and loss, and the SGD update.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ET_HD __host__ __device__ __forceinline__
#else
#define ET_HD inline
#endif

namespace nlml {

constexpr int ET_LAYERS = 6;             // K9's layers, and the most a network may have
constexpr int MLP_NETS_MAX = 3;          // networks that may share a launch (blockIdx.y); K9 is the case of one
constexpr int ET_TILE = 32;
constexpr int ET_WAVES = 8;              // waves of a workgroup = the split of K
constexpr int ET_NT = 64 * ET_WAVES;
constexpr int ET_SUPER = 16;             // k per super-chunk
constexpr int ET_BATCH_MAX = 256;        // NLML_ENCODER_TRAIN_BATCH_MAX
constexpr int ET_LATENT = 9;
constexpr int ET_LATENT_LD = 12;         // row stride of pred and delta_6 in the workspace
constexpr int ET_BIAS_RUNS = ET_NT / 32;
constexpr int ET_UPDATE_PER_WG = 16 * ET_NT;
constexpr int ET_STATUS_ORDER = 1;       // NLML_ENCODER_TRAIN_CLAMPED_ORDER
constexpr int ET_STATUS_LABEL = 2;       // NLML_ENCODER_TRAIN_CLAMPED_LABEL

ET_HD int et_tiles(int n) { return (n + ET_TILE - 1) / ET_TILE; }

// a network both trainers can run: Linear(fan_in, widths[0]) .. Linear(widths[layers-2], widths[layers-1]), ReLU after every layer but
// the last, except Tanh after layer `tanh_layer` (-1: none); last_ld: the row stride of the last layer's output in the workspace.
// K9 is ET_SHAPE with fan_in = F; K10 is HT_SHAPE (heads_train_ref.h) with fan_in = R.
struct MlpShape { int layers, widths[ET_LAYERS], tanh_layer, last_ld; };
constexpr MlpShape ET_SHAPE = {ET_LAYERS, {1024, 512, 256, 128, 64, ET_LATENT}, 4, ET_LATENT_LD};
constexpr int MLP_ACT_NONE = 0, MLP_ACT_RELU = 1, MLP_ACT_TANH = 2;

// widths and the offsets (in floats) of W_l [out,in] and b_l [out] inside the contiguous params / grads buffers, state-dict order
struct MlpDims {
  int layers, tanh_layer, last_ld;
  int in[ET_LAYERS], out[ET_LAYERS];
  int64_t w_off[ET_LAYERS], b_off[ET_LAYERS];
  int64_t total;
  int part_off[ET_LAYERS];   // first norm partial of layer l's wgrad tiles
  int n_partials;
};
ET_HD MlpDims mlp_dims(const MlpShape& s, int fan_in) {
  MlpDims d = {};
  d.layers = s.layers; d.tanh_layer = s.tanh_layer; d.last_ld = s.last_ld;
  int64_t off = 0;
  int parts = 0;
  for (int l = 0; l < s.layers; ++l) {
    d.in[l] = fan_in; d.out[l] = s.widths[l];
    d.w_off[l] = off; off += (int64_t)s.widths[l] * fan_in;
    d.b_off[l] = off; off += s.widths[l];
    d.part_off[l] = parts; parts += et_tiles(s.widths[l]) * et_tiles(fan_in);
    fan_in = s.widths[l];
  }
  d.total = off;
  d.n_partials = parts;
  return d;
}
ET_HD int mlp_act(const MlpDims& d, int l) { return l == d.layers - 1 ? MLP_ACT_NONE : (l == d.tanh_layer ? MLP_ACT_TANH : MLP_ACT_RELU); }

// the workspace of one network's batch, byte offsets: the norm partials (f64), the batch's resolved dataset rows (i32[256]), A_1..A_L
// and delta_1..delta_L (index l - 1; A_L = pred), each [batch, ld[l-1]] and padded to 16 bytes; ld is the layer's width (last_ld for
// the last).  It holds the network's LAST step; words outside these ranges, and rows b >= B of that step, are never written.
struct MlpWorkspace {
  size_t partials, rows, act[ET_LAYERS], delta[ET_LAYERS], net_bytes;
  int ld[ET_LAYERS];
};
ET_HD MlpWorkspace mlp_workspace(const MlpDims& d, int batch) {
  MlpWorkspace w = {};
  size_t off = 0;
  w.partials = off; off += (size_t)((d.n_partials + 1) / 2 * 2) * 8;
  w.rows = off; off += (size_t)ET_BATCH_MAX * 4;
  for (int l = 0; l < d.layers; ++l) {
    w.ld[l] = l == d.layers - 1 ? d.last_ld : d.out[l];
    w.act[l] = off; off += (size_t)batch * w.ld[l] * 4;
    off = (off + 15) / 16 * 16;
  }
  for (int l = 0; l < d.layers; ++l) {
    w.delta[l] = off; off += (size_t)batch * w.ld[l] * 4;
    off = (off + 15) / 16 * 16;
  }
  w.net_bytes = off;
  return w;
}
ET_HD MlpDims et_dims(int F) { return mlp_dims(ET_SHAPE, F); }
ET_HD MlpWorkspace et_workspace(int F, int batch) { return mlp_workspace(et_dims(F), batch); }

// the dataset row of batch slot `slot`: order[slot] (order == NULL: slot itself) clamped into [0, N); *clamped: it was outside
ET_HD int32_t et_resolve_row(const int32_t* order, int64_t slot, int64_t N, bool* clamped) {
  const int64_t v = order ? (int64_t)order[slot] : slot;
  const int64_t c = v < 0 ? 0 : (v >= N ? N - 1 : v);
  *clamped = c != v;
  return (int32_t)c;
}
ET_HD int et_clamp_label(int32_t v, int n, bool* clamped) {
  const int c = v < 0 ? 0 : (v >= n ? n - 1 : v);
  if (c != v) *clamped = true;
  return c;
}
// wave w's super-chunks [*s0, *s1) of a reduction of length K
ET_HD void et_wave_range(int K, int wave, int* s0, int* s1) {
  const int nsc = (K + ET_SUPER - 1) / ET_SUPER, spw = (nsc + ET_WAVES - 1) / ET_WAVES;
  *s0 = wave * spw < nsc ? wave * spw : nsc;
  *s1 = *s0 + spw < nsc ? *s0 + spw : nsc;
}
ET_HD float et_act_grad(float a, bool tanh_layer) { return tanh_layer ? fmaf(-a, a, 1.0f) : (a > 0.0f ? 1.0f : 0.0f); }
ET_HD double et_clip_coefficient(double sumsq, double max_norm, double* norm) {
  *norm = sqrt(sumsq);
  const double c = max_norm / (*norm + 1e-6);
  return c < 1.0 ? c : 1.0;
}
ET_HD void et_update(float* p, float* g, float c, float lr, float wd) {
  const float gc = c * *g;
  const float d = fmaf(wd, *p, gc);
  *g = gc;
  *p = fmaf(-lr, d, *p);
}

// the arguments every form shares, already checked (abi.cpp, "K9 argument checks")
struct EtCall {
  const float* x; int64_t ldx, N;
  const int32_t* labels; int64_t ld_lab;
  const float* table[3]; int rows[3];
  float* params; float* grads;          // grads NULL: forward and loss only (the validation pass)
  int F, batch;
  const int32_t* order; int64_t n;
  float lr, wd; double max_norm; int zero_grad;
  float* loss_out; float* norm_out; int32_t* status;
};

}  // namespace nlml

// ---- the host form ---------------------------------------------------------------------------------------------------------------
#include <vector>

namespace nlml {

// an operand of a host GEMM: element (r, c) = base[row(r) * ld + c], row(r) = rows ? rows[r] : r
struct EtHostMat { const float* base; int64_t ld; const int32_t* rows; };
static inline const float* et_host_row(const EtHostMat& m, int r) { return m.base + (int64_t)(m.rows ? m.rows[r] : r) * m.ld; }

// C[m][n] (row stride N) = the GEMM order above.  B is k-outer: element (k, n) = Bm(k, n); A is k-contiguous (a_kc: element (m, k) =
// Am(m, k)) or k-outer (element (m, k) = Am(k, m)).  init [N] or NULL: wave 0's start.  pad: an index k >= K of a visited super-chunk is
// the zero operand the device feeds its matrix cores (fmaf(0, 0, p): a -0 becomes +0) instead of a skipped one -- K10's host form,
// which is claimed to return the device's bits (heads_train_ref.h); K9's stays as it was.
static inline __attribute__((always_inline)) void et_host_gemm_body(int M, int N, int K, const EtHostMat& Am, bool a_kc, const EtHostMat& Bm,
                                                                    const float* init, float* __restrict C, float* __restrict part,
                                                                    const bool pad) {
  for (int m = 0; m < M; ++m) {
    for (int w = 0; w < ET_WAVES; ++w) {
      float* __restrict p = part + (size_t)w * N;
      for (int n = 0; n < N; ++n) p[n] = (w == 0 && init) ? init[n] : 0.0f;
      int s0, s1;
      et_wave_range(K, w, &s0, &s1);
      for (int s = s0; s < s1; ++s)
        for (int u = 0; u < 2; ++u)
          for (int j = 0; j < 4; ++j)
            for (int h = 0; h < 2; ++h) {
              const int k = ET_SUPER * s + 8 * u + 4 * h + j;
              if (k >= K) {
                if (pad)
                  for (int n = 0; n < N; ++n) p[n] = fmaf(0.0f, 0.0f, p[n]);
                continue;
              }
              const float av = a_kc ? et_host_row(Am, m)[k] : et_host_row(Am, k)[m];
              const float* __restrict br = et_host_row(Bm, k);
              for (int n = 0; n < N; ++n) p[n] = fmaf(av, br[n], p[n]);
            }
    }
    float* __restrict c = C + (size_t)m * N;
    for (int n = 0; n < N; ++n) {
      float t = part[n];
      for (int w = 1; w < ET_WAVES; ++w) t = t + part[(size_t)w * N + n];
      c[n] = t;
    }
  }
}
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
__attribute__((target("avx2,fma"))) static void et_host_gemm_fma(int M, int N, int K, const EtHostMat& Am, bool a_kc, const EtHostMat& Bm,
                                                                 const float* init, float* C, float* part, bool pad) {
  if (pad) et_host_gemm_body(M, N, K, Am, a_kc, Bm, init, C, part, true);
  else et_host_gemm_body(M, N, K, Am, a_kc, Bm, init, C, part, false);
}
#endif
static void et_host_gemm_plain(int M, int N, int K, const EtHostMat& Am, bool a_kc, const EtHostMat& Bm, const float* init, float* C,
                               float* part, bool pad) {
  if (pad) et_host_gemm_body(M, N, K, Am, a_kc, Bm, init, C, part, true);
  else et_host_gemm_body(M, N, K, Am, a_kc, Bm, init, C, part, false);
}
// the same values either way (fmaf is fmaf); the first is the second with the machine's own fused multiply-add and vectors
static inline void et_host_gemm(int M, int N, int K, const EtHostMat& Am, bool a_kc, const EtHostMat& Bm, const float* init, float* C,
                                bool pad = false) {
  std::vector<float> part((size_t)ET_WAVES * N);
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
  if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma")) return et_host_gemm_fma(M, N, K, Am, a_kc, Bm, init, C, part.data(), pad);
#endif
  et_host_gemm_plain(M, N, K, Am, a_kc, Bm, init, C, part.data(), pad);
}

template <class T, int SLOTS> static inline T et_host_tree(T* s) {
  for (int stride = SLOTS / 2; stride >= 1; stride /= 2)
    for (int t = 0; t < stride; ++t) s[t] = s[t] + s[t + stride];
  return s[0];
}

// ---- the part of a step K9 and K10 share, into one network's workspace block (the device's layout, mlp_workspace) ---------------------
struct MlpHostWs {
  MlpWorkspace ws;
  int32_t* rows; double* partials;
  float* act[ET_LAYERS]; float* delta[ET_LAYERS];
};
static inline MlpHostWs mlp_host_ws(const MlpDims& d, int batch, char* block) {
  MlpHostWs v = {};
  v.ws = mlp_workspace(d, batch);
  v.rows = reinterpret_cast<int32_t*>(block + v.ws.rows);
  v.partials = reinterpret_cast<double*>(block + v.ws.partials);
  for (int l = 0; l < d.layers; ++l) {
    v.act[l] = reinterpret_cast<float*>(block + v.ws.act[l]);
    v.delta[l] = reinterpret_cast<float*>(block + v.ws.delta[l]);
  }
  return v;
}
// the batch's dataset rows -> v.rows; true: an entry of order was outside [0, N)
static inline bool mlp_host_rows(const MlpHostWs& v, const int32_t* order, int64_t slot0, int64_t N, int B) {
  bool any = false;
  for (int b = 0; b < B; ++b) {
    bool cl;
    v.rows[b] = et_resolve_row(order, slot0 + b, N, &cl);
    any = any || cl;
  }
  return any;
}
// A_{l-1} as a GEMM operand: the gathered rows of x for l = 0
static inline EtHostMat mlp_host_input(const MlpHostWs& v, const EtHostMat& X, int l) {
  return l == 0 ? X : EtHostMat{v.act[l - 1], v.ws.ld[l - 1], nullptr};
}
// A_1 .. A_L
static inline void mlp_host_forward(const MlpDims& d, const MlpHostWs& v, const EtHostMat& X, const float* params, int B, bool pad) {
  std::vector<float> wt, c;
  for (int l = 0; l < d.layers; ++l) {
    const int K = d.in[l], N = d.out[l], ld = v.ws.ld[l], act = mlp_act(d, l);
    const float* W = params + d.w_off[l];
    wt.resize((size_t)K * N);
    for (int o = 0; o < N; ++o)
      for (int k = 0; k < K; ++k) wt[(size_t)k * N + o] = W[(size_t)o * K + k];
    c.resize((size_t)B * N);
    et_host_gemm(B, N, K, mlp_host_input(v, X, l), true, EtHostMat{wt.data(), N, nullptr}, params + d.b_off[l], c.data(), pad);
    for (int b = 0; b < B; ++b)
      for (int o = 0; o < N; ++o) {
        const float z = c[(size_t)b * N + o];
        v.act[l][(size_t)b * ld + o] = act == MLP_ACT_RELU ? (z > 0.0f ? z : 0.0f) : (act == MLP_ACT_TANH ? tanhf(z) : z);
      }
  }
}
// delta_{L-1} .. delta_1 from delta_L
static inline void mlp_host_dgrad(const MlpDims& d, const MlpHostWs& v, const float* params, int B, bool pad) {
  std::vector<float> c;
  for (int l = d.layers - 1; l >= 1; --l) {
    const int in = d.in[l], out = d.out[l], ldp = v.ws.ld[l - 1];
    c.resize((size_t)B * in);
    et_host_gemm(B, in, out, EtHostMat{v.delta[l], v.ws.ld[l], nullptr}, true, EtHostMat{params + d.w_off[l], in, nullptr}, nullptr, c.data(), pad);
    for (int b = 0; b < B; ++b)
      for (int i = 0; i < in; ++i)
        v.delta[l - 1][(size_t)b * ldp + i] = c[(size_t)b * in + i] * et_act_grad(v.act[l - 1][(size_t)b * ldp + i], l - 1 == d.tanh_layer);
  }
}
// G (+)= dW, G_b (+)= db and every wgrad tile's norm partial
static inline void mlp_host_wgrad(const MlpDims& d, const MlpHostWs& v, const EtHostMat& X, float* grads, int B, int zero_grad, bool pad) {
  std::vector<float> c;
  for (int l = 0; l < d.layers; ++l) {
    const int in = d.in[l], out = d.out[l], ldd = v.ws.ld[l];
    float* gW = grads + d.w_off[l];
    float* gb = grads + d.b_off[l];
    c.resize((size_t)out * in);
    et_host_gemm(out, in, B, EtHostMat{v.delta[l], ldd, nullptr}, false, mlp_host_input(v, X, l), nullptr, c.data(), pad);
    const int tn_n = et_tiles(in);
    const int rp = (B + ET_BIAS_RUNS - 1) / ET_BIAS_RUNS;
    for (int tm = 0; tm < et_tiles(out); ++tm)
      for (int tn = 0; tn < tn_n; ++tn) {
        double s[ET_NT];
        for (int t = 0; t < ET_NT; ++t) {
          s[t] = 0.0;
          for (int e = t; e < ET_TILE * ET_TILE; e += ET_NT) {
            const int o = tm * ET_TILE + (e >> 5), i = tn * ET_TILE + (e & 31);
            if (o >= out || i >= in) continue;
            float* g = gW + (size_t)o * in + i;
            *g = zero_grad ? c[(size_t)o * in + i] : *g + c[(size_t)o * in + i];
            s[t] = fma((double)*g, (double)*g, s[t]);
          }
        }
        if (tn == 0)
          for (int t = 0; t < ET_TILE; ++t) {
            const int o = tm * ET_TILE + t;
            if (o >= out) continue;
            float total = 0.0f;
            for (int r = 0; r < ET_BIAS_RUNS; ++r) {
              float run = 0.0f;
              for (int b = r * rp; b < B && b < (r + 1) * rp; ++b) run = run + v.delta[l][(size_t)b * ldd + o];
              total = r == 0 ? run : total + run;
            }
            gb[o] = zero_grad ? total : gb[o] + total;
            s[t] = fma((double)gb[o], (double)gb[o], s[t]);
          }
        v.partials[d.part_off[l] + tm * tn_n + tn] = et_host_tree<double, ET_NT>(s);
      }
  }
}
// the clip coefficient from the norm partials; *norm: the norm
static inline float mlp_host_clip(const MlpDims& d, const MlpHostWs& v, double max_norm, double* norm) {
  double s[ET_NT];
  for (int t = 0; t < ET_NT; ++t) {
    s[t] = 0.0;
    for (int i = t; i < d.n_partials; i += ET_NT) s[t] = s[t] + v.partials[i];
  }
  return (float)et_clip_coefficient(et_host_tree<double, ET_NT>(s), max_norm, norm);
}

// ---- K9's own part ---------------------------------------------------------------------------------------------------------------------
// one batch: forward, loss (-> *loss, status bits OR-ed into *status), and with grads the backward pass, the norm and the update
static inline void et_host_step(const EtCall& a, int64_t slot0, int B, char* block, float* loss, float* norm_out, int* status) {
  const MlpDims d = et_dims(a.F);
  const MlpHostWs v = mlp_host_ws(d, a.batch, block);
  int flags = mlp_host_rows(v, a.order, slot0, a.N, B) ? ET_STATUS_ORDER : 0;
  const EtHostMat X = {a.x, a.ldx, v.rows};
  mlp_host_forward(d, v, X, a.params, B, false);
  // residual and loss
  const float scale = (float)(2.0 / (3.0 * B));
  float slots[ET_BATCH_MAX];
  for (int b = 0; b < ET_BATCH_MAX; ++b) slots[b] = 0.0f;
  for (int b = 0; b < B; ++b) {
    bool cl = false;
    float q = 0.0f;
    for (int j = 0; j < ET_LATENT; ++j) {
      const int t = j / 3;
      const int row = et_clamp_label(a.labels[(int64_t)v.rows[b] * a.ld_lab + t], a.rows[t], &cl);
      const float dd = v.act[5][b * ET_LATENT_LD + j] - a.table[t][row * 3 + j % 3];
      v.delta[5][b * ET_LATENT_LD + j] = dd * scale;
      q = fmaf(dd, dd, q);
    }
    if (cl) flags |= ET_STATUS_LABEL;
    slots[b] = q;
  }
  *loss = et_host_tree<float, ET_BATCH_MAX>(slots) / (float)(3 * B);
  if (status) *status |= flags;
  if (!a.grads) return;
  mlp_host_dgrad(d, v, a.params, B, false);
  mlp_host_wgrad(d, v, X, a.grads, B, a.zero_grad, false);
  double norm;
  const float c = mlp_host_clip(d, v, a.max_norm, &norm);
  if (norm_out) *norm_out = (float)norm;
  for (int64_t e = 0; e < d.total; ++e) et_update(a.params + e, a.grads + e, c, a.lr, a.wd);
}

// ceil(n / batch) consecutive batches, in a workspace of its own
static inline void et_host_run(const EtCall& a) {
  std::vector<char> block(et_workspace(a.F, a.batch).net_bytes, 0);
  if (a.status) *a.status = 0;
  int64_t step = 0;
  for (int64_t s0 = 0; s0 < a.n; s0 += a.batch, ++step) {
    const int B = (int)(a.n - s0 < a.batch ? a.n - s0 : a.batch);
    float loss = 0.0f, norm = 0.0f;
    et_host_step(a, s0, B, block.data(), &loss, &norm, a.status);
    if (a.loss_out) a.loss_out[step] = loss;
    if (a.grads && a.norm_out) a.norm_out[step] = norm;
  }
}

}  // namespace nlml
