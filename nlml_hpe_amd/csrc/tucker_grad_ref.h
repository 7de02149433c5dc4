// tucker_grad_ref.h -- the analytic gradient of the Tucker objective in the REFERENCE'S OWN OPERATION ORDER (K3g): what the gfx950
// kernels (tucker_gradient.hip) and the host restatement (nlml_tucker_gradient_host) share.  Plain C++ on the host side.
//
// The reference (TD_Tester.py:60-102) forms, for params = (w_y, w_p, w_r, u[R]) and one face x:
//   f_a  = float32(a cos(b w_a + c) + d)                       as the objective does (cr_cos.h)
//   df_a = float32(((-a) b) sin(b w_a + c))                    :82,87,92, the sin correctly rounded (cr_cos.h, cr_f32_nab_sin)
//   x_hat = einsum('ijklm,i,j,k,l->m', W, u, f_y, f_p, f_r)    numpy's generic loop (tucker_ref.h), r = x - x_hat, err = 0.5 sum(r^2)
//   e_y   = the same einsum with df_y in f_y's place (e_p, e_r likewise);  grad_w_a = -np.sum(r * e_a)   numpy's pairwise tree (np_sum.h)
//   v     = einsum('ijklm,j,k,l->m', W, f_y, f_p, f_r)         all operands f32: numpy runs it IN F32, and it sums over i as well
//           (the reference's quirk, kept): for q = (i,j,k,l) in nesting order, v[m] = f32(f32(f32(W f_yj) f_pk) f_rl) + v[m]
//   grad_u[i] = -einsum('ijklm,m->i', W, t),  t = r * f64(v)
// The order of the last, two-operand reduction is numpy's buffered iterator and its contiguous / output-stride-0 inner loop
// (einsum_sumprod.c.src, *_sum_of_products_contig_contig_outstride0_two), established against numpy 2.2.6 bit for bit:
//   * W needs a cast to f64, so the iterator buffers: for every i the 27 * 1404 = 37,908 (j,k,l,m) elements go through the inner loop
//     in chunks of the iterator's buffer, 8192 elements (4 x 8192 + 5140); m is the fast index, so a chunk starts in mid row;
//   * the inner loop (baseline build: 128-bit vectors, two f64 lanes, no fma) takes 8 elements per round as four lane pairs and adds
//     their products to the lane accumulator LAST PAIR FIRST: acc = a0 b0 + (a1 b1 + (a2 b2 + (a3 b3 + acc))); what is left of the
//     chunk goes pair by pair; then the chunk's sum is acc[0] + acc[1] and the output becomes sum + output.
// So grad_u[i] is 10 sequential chains (5 chunks x 2 lanes) of up to 4,096 multiply-adds; tg_uid_elem below is that order.
#pragma once
#include <stdint.h>

#include "cr_cos.h"
#include "np_sum.h"

namespace nlml {

constexpr int TG_M = 1404;                 // features of a face
constexpr int TG_ROW = 27 * TG_M;          // elements of W under one identity index i
constexpr int TG_CHUNK = 8192;             // numpy's iterator buffer (NPY_BUFSIZE), in elements
constexpr int TG_NCHUNK = (TG_ROW + TG_CHUNK - 1) / TG_CHUNK;   // 5
constexpr int TG_CHAINS = 2 * TG_NCHUNK;   // sequential chains of one grad_u[i]: (chunk, lane)

NLML_CR_HD int tg_chunk_count(int chunk) { return chunk < TG_NCHUNK - 1 ? TG_CHUNK : TG_ROW - (TG_NCHUNK - 1) * TG_CHUNK; }
// multiply-adds of one lane over a chunk of `count` elements (count is even here: 8192 or 5140)
NLML_CR_HD int tg_uid_steps(int count) { return 4 * (count / 8) + (count % 8 + 1) / 2; }
// the element (offset inside its chunk) of a lane's s-th multiply-add
NLML_CR_HD int tg_uid_elem(int count, int s, int lane) {
  const int body = 4 * (count / 8);
  return s < body ? 8 * (s / 4) + 2 * (3 - s % 4) + lane : 8 * (count / 8) + 2 * (s - body) + lane;
}
// -(the chunks' sums added to the output in turn); acc[chunk * 2 + lane]
template <typename AccAt>
NLML_CR_HD double tg_uid_combine(const AccAt acc) {
  NLML_CR_STRICT
  double o = 0.0;
  for (int c = 0; c < TG_NCHUNK; ++c) o = (acc(2 * c) + acc(2 * c + 1)) + o;
  return -o;
}

// One gradient on the host: Wm f32[27 R, 1404], x f32[1404], par f64[3 + R], cosp f64[3,3,4] -> *err (if given), grad f64[3 + R],
// v f32[1404] (if given: the f32 einsum of the identity term, for tests).
inline void tg_gradient_host(const float* Wm, const float* x, const double* par, const double* cosp, int rid, double* err, double* grad,
                             float* v_out) {
  NLML_CR_STRICT
  float f[3][3], df[3][3];
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 3; ++j) {
      const double* row = cosp + (a * 3 + j) * 4;
      f[a][j] = cr_fvec(row, par[a]);
      df[a][j] = cr_dfvec(row, par[a]);
    }
  // chain 0: x_hat; chains 1..3: e_y, e_p, e_r (one factor triple swapped)
  static thread_local double ch[4][TG_M], r[TG_M], prod[TG_M], t[TG_M];
  static thread_local float v[TG_M];
  for (int c = 0; c < 4; ++c)
    for (int m = 0; m < TG_M; ++m) ch[c][m] = 0.0;
  for (int m = 0; m < TG_M; ++m) v[m] = 0.0f;
  for (int q = 0; q < 27 * rid; ++q) {
    const int i = tucker_q_i(q), j = tucker_q_j(q), k = tucker_q_k(q), l = tucker_q_l(q);
    const float* w = Wm + (int64_t)q * TG_M;
    for (int c = 0; c < 4; ++c) {
      const double u = par[3 + i], fy = (double)(c == 1 ? df[0][j] : f[0][j]), fp = (double)(c == 2 ? df[1][k] : f[1][k]),
                   fr = (double)(c == 3 ? df[2][l] : f[2][l]);
      for (int m = 0; m < TG_M; ++m) ch[c][m] = ((((double)w[m] * u) * fy) * fp) * fr + ch[c][m];
    }
    const float fy = f[0][j], fp = f[1][k], fr = f[2][l];
    for (int m = 0; m < TG_M; ++m) v[m] = ((w[m] * fy) * fp) * fr + v[m];
  }
  for (int m = 0; m < TG_M; ++m) r[m] = (double)x[m] - ch[0][m];
  if (err) {
    for (int m = 0; m < TG_M; ++m) prod[m] = r[m] * r[m];
    *err = 0.5 * np_pairwise_sum(prod, TG_M);
  }
  for (int a = 0; a < 3; ++a) {
    for (int m = 0; m < TG_M; ++m) prod[m] = r[m] * ch[1 + a][m];
    grad[a] = -np_pairwise_sum(prod, TG_M);
  }
  for (int m = 0; m < TG_M; ++m) t[m] = r[m] * (double)v[m];
  if (v_out)
    for (int m = 0; m < TG_M; ++m) v_out[m] = v[m];
  for (int i = 0; i < rid; ++i) {
    const float* wi = Wm + (int64_t)i * TG_ROW;
    double acc[TG_CHAINS];
    for (int c = 0; c < TG_NCHUNK; ++c)
      for (int lane = 0; lane < 2; ++lane) {
        const int start = c * TG_CHUNK, count = tg_chunk_count(c), steps = tg_uid_steps(count);
        double s = 0.0;
        for (int st = 0; st < steps; ++st) {
          const int e = start + tg_uid_elem(count, st, lane);
          s = (double)wi[e] * t[e % TG_M] + s;
        }
        acc[2 * c + lane] = s;
      }
    grad[3 + i] = tg_uid_combine([&](int k) { return acc[k]; });
  }
}

}  // namespace nlml
