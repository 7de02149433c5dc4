/* oracle.c -- plain-C CPU restatement of the NLML_HPE hot path.  TEST INFRASTRUCTURE ONLY
 * (see oracle/__init__.py): loaded by tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg, never by the product package.
 *
 * Each function cites the reference lines it follows (paths under /root/reference).
 * Unlike the numpy oracle, summation ORDER is fixed here, and selectable to equal the order the
 * HIP kernel's MFMA chains use, so GPU results can be compared bit for bit wherever the
 * arithmetic is pure fma (everything up to the Tanh).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ---- helpers/FeatureExtractor.py:30-66 + the .float() at :101 ---------------------------- */
/* ipd[b] of raw [B,1404] as oracle_normalize_ipd below computes it (the 1e-6 branch included) */
void oracle_ipd(const float* raw, int64_t B, double* ipd_out) {
  for (int64_t b = 0; b < B; ++b) {
    const float* p = raw + b * 1404;
    const double dx = (double)p[99] - (double)p[789];
    const double dy = (double)p[100] - (double)p[790];
    const double dz = (double)p[101] - (double)p[791];
    const double ipd = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
    ipd_out[b] = ipd == 0.0 ? 1e-6 : ipd;
  }
}

void oracle_normalize_ipd(const float* raw, int64_t B, int normalize, float* out) {
  for (int64_t b = 0; b < B; ++b) {
    const float* p = raw + b * 1404;
    float* o = out + b * 1404;
    if (!normalize) { memcpy(o, p, 1404 * sizeof(float)); continue; }
    const double ref[3] = {p[3], p[4], p[5]};                                /* landmark 1, :85-86 */
    const double dx = (double)p[99] - (double)p[789];                        /* 33 vs 263, :38-43 */
    const double dy = (double)p[100] - (double)p[790];
    const double dz = (double)p[101] - (double)p[791];
    double ipd = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));  /* np.linalg.norm == sqrt(ddot): fma chain on this BLAS */
    if (ipd == 0.0) ipd = 1e-6;                                              /* :47-48 */
    for (int k = 0; k < 1404; ++k) o[k] = (float)(((double)p[k] - ref[k % 3]) / ipd);   /* :55-61 */
  }
}

/* One Linear layer for one row.  order 0: k ascending; order 1: the HIP kernels' MFMA chain order -- within each group of 8:
 * k, k+4, k+1, k+5, k+2, k+6, k+3, k+7 (layout.h).  blk > 0 (a multiple of 8): the K-BLOCKED sum of the f32 kernel's layers 0
 * to 3 (encoder_heads.hip fold_block): one chain per block of blk k-values in the order above, the first from the bias, the
 * others from +0.0, and the block sums added up in block order starting from +0.0: ((0 + s_0) + s_1) + ... */
static float chain8(const float* w, const float* x, int k0, int k1, int K, float acc) {
  for (; k0 + 8 <= k1; k0 += 8)
    for (int j = 0; j < 4; ++j) {
      acc = fmaf(w[k0 + j], x[k0 + j], acc);
      acc = fmaf(w[k0 + 4 + j], x[k0 + 4 + j], acc);
    }
  if (k0 < k1) /* zero-padded tail step: padded products are exact zeros and change nothing */
    for (int j = 0; j < 4; ++j) {
      if (k0 + j < K) acc = fmaf(w[k0 + j], x[k0 + j], acc);
      if (k0 + 4 + j < K) acc = fmaf(w[k0 + 4 + j], x[k0 + 4 + j], acc);
    }
  return acc;
}

static void linear_row(const float* x, const float* W, const float* b, int K, int N, float* y, int order, int blk) {
  for (int n = 0; n < N; ++n) {
    const float* w = W + (size_t)n * K;
    if (order == 0) {
      float acc = b[n];
      for (int k = 0; k < K; ++k) acc = fmaf(w[k], x[k], acc);
      y[n] = acc;
    } else if (blk <= 0) {
      y[n] = chain8(w, x, 0, K, K, b[n]);
    } else {
      float tot = 0.0f;
      for (int k0 = 0; k0 < K; k0 += blk) {
        const int k1 = k0 + blk < K ? k0 + blk : K;
        tot += chain8(w, x, k0, k1, K, k0 == 0 ? b[n] : 0.0f);
      }
      y[n] = tot;
    }
  }
}

/* ---- NLML_HPE_Model_Builder.py:55-68 (encoder), :104-105 (heads), :115-126 (combined) -----
 * enc_w[i] [out,in] for widths F->1024->512->256->128->64->9; head_w[3*5] in (yaw,pitch,roll) x
 * layer order with widths 3->128->256->128->64->1.  out [B,3] radians; latent [B,9] and
 * pre_tanh [B,64] optional (NULL to skip). */
void oracle_encoder_heads_f32(const float* x, int64_t B, int F, const float* const* enc_w,
                              const float* const* enc_b, const float* const* head_w,
                              const float* const* head_b, int order, float* out, float* latent,
                              float* pre_tanh) {
  static const int EN[7] = {0, 1024, 512, 256, 128, 64, 9};
  static const int HN[6] = {3, 128, 256, 128, 64, 1};
#pragma omp parallel
  {
    float* a = (float*)malloc(sizeof(float) * (F > 1024 ? F : 1024));
    float* c = (float*)malloc(sizeof(float) * 1024);
#pragma omp for schedule(static)
    for (int64_t r = 0; r < B; ++r) {
      memcpy(a, x + r * F, sizeof(float) * F);
      int K = F;
      for (int l = 0; l < 6; ++l) {
        const int N = EN[l + 1];
        linear_row(a, enc_w[l], enc_b[l], K, N, c, order, (order == 2 && l < 4) ? 128 : 0);   /* order 2: layers 0..3 K-blocked */
        if (l == 4 && pre_tanh) memcpy(pre_tanh + r * 64, c, sizeof(float) * 64);
        for (int n = 0; n < N; ++n)
          a[n] = (l < 4) ? (c[n] < 0.0f ? 0.0f : c[n]) : (l == 4 ? tanhf(c[n]) : c[n]);   /* ReLU x4 (NaN propagates, like torch.relu), Tanh, none */
        K = N;
      }
      float lat[9];
      memcpy(lat, a, sizeof lat);
      if (latent) memcpy(latent + r * 9, lat, sizeof lat);
      for (int g = 0; g < 3; ++g) {                          /* latent[:, 3g:3g+3] -> head g, :118-124 */
        memcpy(a, lat + 3 * g, 3 * sizeof(float));
        int Kh = 3;
        for (int l = 0; l < 5; ++l) {
          const int N = HN[l + 1];
          linear_row(a, head_w[g * 5 + l], head_b[g * 5 + l], Kh, N, c, order, 0);
          for (int n = 0; n < N; ++n) a[n] = (l < 4) ? (c[n] < 0.0f ? 0.0f : c[n]) : c[n];
          Kh = N;
        }
        out[r * 3 + g] = a[0];
      }
    }
    free(a);
    free(c);
  }
}

/* ---- TD_Tester.py:25-28 (func), :31-58 (objective) ---------------------------------------
 * Wm f32[135,1404]; x f32[N,1404]; params f64[N,8]; cosp f64[3,3,4]; err f64[N]; xhat f64[N,1404]|NULL.
 * x_hat[m] = sum_q c[q]*Wm[q][m], q ascending in one fma chain (the HIP kernel's order). */
/* device_order != 0: the residual is summed in the HIP kernel's order (tucker_objective.hip /
 * tucker_powell.hip): the MFMA tiling's order, see residual_device_order; the result is then bit-identical to the
 * GPU's, which lets the device-side Powell run be replayed exactly on the CPU. */
static double residual_device_order(const float* xrow, const double* acc) {
  /* tucker_common.h: 8 waves x 176 columns from tcol0(w) = 176 w (the last wave: 1228; its first 4 columns belong to wave 6 and
   * are skipped); lane column c of wave w sums its 11 columns tcol0 + tlcol(c, mb) (fma chain, mb ascending), where
   * tlcol(c, mb) = 64 (mb/4) + 4 c + mb%4 for mb < 8 and 128 + 3 c + (mb - 8) above; xor butterfly over the 16 lanes (offsets
   * 1,2,4,8), then the 8 waves. */
  double red[8];
  for (int w = 0; w < 8; ++w) {
    const int base = w < 7 ? 176 * w : 1404 - 176;
    double v[16], n[16];
    for (int c = 0; c < 16; ++c) {
      double s = 0.0;
      for (int mb = 0; mb < 11; ++mb) {
        const int lc = mb < 8 ? 64 * (mb >> 2) + 4 * c + (mb & 3) : 128 + 3 * c + (mb - 8);
        const int m = base + lc;
        if (w < 7 || lc >= 8 * 176 - 1404) { const double r = (double)xrow[m] - acc[m]; s = fma(r, r, s); }
      }
      v[c] = s;
    }
    for (int off = 1; off < 16; off <<= 1) {
      for (int c = 0; c < 16; ++c) n[c] = v[c] + v[c ^ off];
      memcpy(v, n, sizeof v);
    }
    red[w] = v[0];
  }
  return 0.5 * (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7])));
}

/* numpy's pairwise summation (numpy/_core/src/umath/loops_utils.h.src, DOUBLE_pairwise_sum; what np.sum at TD_Tester.py:49 runs on
 * a contiguous f64 vector): blocks of at most 128 elements are summed in eight strided partial sums, combined as
 * ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the remainder added one by one; longer ranges split at n/2 rounded down to a multiple of 8. */
static double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    int i;
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

/* The objective in the REFERENCE's own operation order (TD_Tester.py:46,49): np.einsum('ijklm,i,j,k,l->m') with five operands
 * runs numpy's generic sum-of-products loop -- for every (i,j,k,l), in that nesting order, and every m:
 *     x_hat[m] = ((((W[i,j,k,l,m] * u_i) * f_yj) * f_pk) * f_rl) + x_hat[m]
 * every operation rounded to f64 on its own (no fused multiply-add) -- then 0.5 * np.sum((x - x_hat)**2) with the pairwise sum
 * above.  Bit-identical to FX4's err and x_hat (tests/test_oracle_golden.py). */
void oracle_tucker_objective_reforder(const float* Wm, const float* x, const double* params, const double* cosp,
                                      int64_t N, double* err, double* xhat) {
#pragma omp parallel for schedule(static)
  for (int64_t n = 0; n < N; ++n) {
    const double* p = params + n * 8;
    double f[3][3];
    for (int a = 0; a < 3; ++a)
      for (int j = 0; j < 3; ++j) {
        const double* cp = cosp + (a * 3 + j) * 4;
        f[a][j] = (double)(float)(cp[0] * cos(cp[1] * p[a] + cp[2]) + cp[3]);
      }
    double acc[1404], d2[1404];
    for (int m = 0; m < 1404; ++m) acc[m] = 0.0;
    for (int q = 0; q < 135; ++q) {
      const double u = p[3 + q / 27], fy = f[0][(q / 9) % 3], fp = f[1][(q / 3) % 3], fr = f[2][q % 3];
      const float* w = Wm + (size_t)q * 1404;
      for (int m = 0; m < 1404; ++m) {
        double t = (double)w[m] * u;
        t = t * fy;
        t = t * fp;
        t = t * fr;
        acc[m] = t + acc[m];
      }
    }
    for (int m = 0; m < 1404; ++m) {
      const double d = (double)x[n * 1404 + m] - acc[m];
      d2[m] = d * d;
      if (xhat) xhat[n * 1404 + m] = acc[m];
    }
    err[n] = 0.5 * np_pairwise_sum(d2, 1404);
  }
}

/* The MATRIX-CORE ("fast") order for any identity rank R, written from the prose of nlml_hpe_amd/csrc/tucker_common.h (its header
 * comment) and tucker_rank.h; no kernel header is included.
 *   Wm f32[27 R,1404]; x f32 rows of stride ldx (>= 1404; the pad columns are never read); x_index i32[N] or NULL: evaluation n reads
 *   row x_index[n] (row n without); params f64[N,3+R]; fvec f64[N,3,3] holding f32 values (f_y, f_p, f_r: an INPUT, so that libm does
 *   not enter here and the caller decides whose cos it is); err f64[N]; xhat f64[N,1404] or NULL.
 *   c[q]      = ((u_i * f_y[j]) * f_p[k]) * f_r[l], q = ((i*3+j)*3+k)*3+l < 27 R, every product rounded on its own;
 *   x_hat[m]  = one fma(c[q], (double)Wm[q][m], acc) chain, q ascending from +0.0 (what one matrix-core output accumulates; the zero
 *               coefficient rows that pad 27 R to a multiple of 4 multiply a finite Wm entry and add +0.0 or -0.0 to a chain that is
 *               not -0.0: no change, and they are left out here);
 *   err       = residual_device_order.
 * variant 0 is that order.  The others are deliberately WRONG orders with which tests/test_td_fast_order_host.py shows that its inputs
 * tell them apart: 1 q descending; 2 multiply and add rounded separately instead of fused; 3 the residual summed left to right over
 * m (x_hat is the model's); 4 wave 7's four repeated columns 1228..1231 counted twice (x_hat is the model's); 5 the coefficient
 * rounded to f32 before the product. */
void oracle_tucker_objective_fast(const float* Wm, int R, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                                  const double* fvec, int64_t N, double* err, double* xhat, int variant) {
  const int Q = 27 * R, npar = 3 + R;
#pragma omp parallel for schedule(static)
  for (int64_t n = 0; n < N; ++n) {
    const double* p = params + n * npar;
    const double* f = fvec + n * 9;
    const float* xrow = x + (x_index ? (int64_t)x_index[n] : n) * ldx;
    double c[27 * 16];
    for (int q = 0; q < Q; ++q) {
      c[q] = ((p[3 + q / 27] * f[(q / 9) % 3]) * f[3 + (q / 3) % 3]) * f[6 + q % 3];
      if (variant == 5) c[q] = (double)(float)c[q];
    }
    double accv[1404];
    for (int m = 0; m < 1404; ++m) accv[m] = 0.0;
    for (int s = 0; s < Q; ++s) {   /* row by row: each column's chain still takes its q in this order */
      const int q = variant == 1 ? Q - 1 - s : s;
      const float* w = Wm + (size_t)q * 1404;
      if (variant == 2)
        for (int m = 0; m < 1404; ++m) { const double t = c[q] * (double)w[m]; accv[m] = t + accv[m]; }   /* (-ffp-contract=off: two roundings) */
      else
        for (int m = 0; m < 1404; ++m) accv[m] = fma(c[q], (double)w[m], accv[m]);
    }
    if (xhat) memcpy(xhat + n * 1404, accv, sizeof accv);
    if (variant == 3) {
      double s = 0.0;
      for (int m = 0; m < 1404; ++m) { const double r = (double)xrow[m] - accv[m]; s = fma(r, r, s); }
      err[n] = 0.5 * s;
    } else if (variant == 4) {
      /* the model's tree, but wave 7 also sums its first four columns: lanes 0 (mb 0..3) of the segment from 1228.  Same chain
       * positions, so only those four extra terms differ. */
      double red[8];
      for (int w = 0; w < 8; ++w) {
        const int base = w < 7 ? 176 * w : 1404 - 176;
        double v[16], t[16];
        for (int cl = 0; cl < 16; ++cl) {
          double s = 0.0;
          for (int mb = 0; mb < 11; ++mb) {
            const int lc = mb < 8 ? 64 * (mb >> 2) + 4 * cl + (mb & 3) : 128 + 3 * cl + (mb - 8);
            const double r = (double)xrow[base + lc] - accv[base + lc];
            s = fma(r, r, s);
          }
          v[cl] = s;
        }
        for (int off = 1; off < 16; off <<= 1) {
          for (int cl = 0; cl < 16; ++cl) t[cl] = v[cl] + v[cl ^ off];
          memcpy(v, t, sizeof v);
        }
        red[w] = v[0];
      }
      err[n] = 0.5 * (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7])));
    } else {
      err[n] = residual_device_order(xrow, accv);
    }
  }
}

void oracle_tucker_objective(const float* Wm, const float* x, const double* params, const double* cosp,
                             int64_t N, double* err, double* xhat, int device_order) {
#pragma omp parallel for schedule(static)
  for (int64_t n = 0; n < N; ++n) {
    const double* p = params + n * 8;
    double f[3][3];
    for (int a = 0; a < 3; ++a)
      for (int j = 0; j < 3; ++j) {
        const double* cp = cosp + (a * 3 + j) * 4;
        f[a][j] = (double)(float)(cp[0] * cos(cp[1] * p[a] + cp[2]) + cp[3]);   /* :26, .astype(f32) :37 */
      }
    double c[135];
    for (int q = 0; q < 135; ++q)
      c[q] = ((p[3 + q / 27] * f[0][(q / 9) % 3]) * f[1][(q / 3) % 3]) * f[2][q % 3];
    double s = 0.0;
    double accv[1404];
    for (int m = 0; m < 1404; ++m) {
      double acc = 0.0;
      for (int q = 0; q < 135; ++q) acc = fma(c[q], (double)Wm[(size_t)q * 1404 + m], acc);
      if (xhat) xhat[n * 1404 + m] = acc;
      accv[m] = acc;
      const double r = (double)x[n * 1404 + m] - acc;
      s += r * r;
    }
    err[n] = device_order ? residual_device_order(x + n * 1404, accv) : 0.5 * s;   /* :49 */
  }
}

/* ---- K7: the four primitives of the Tucker decomposition (TD_main.py:181) ------------------
 * The SUMMATION ORDERS of nlml_mode_gram, nlml_pose_grams, nlml_project_identity and nlml_project_pose, written from the prose of
 * include/nlml_hpe.h (its K7 paragraph) and of the header comment of nlml_hpe_amd/csrc/tucker_decompose.hip; no kernel header is
 * included and libm enters through fma alone.  A tensor argument is f32, or f64 where its flag is nonzero.  variant 0 is the order;
 * the others are deliberately WRONG orders with which tests/test_tucker_order_host.py shows that the inputs of
 * tests/test_tucker_order_gpu.py tell them apart. */
static inline double k7_load(const void* p, int f64, int64_t idx) {
  return f64 ? ((const double*)p)[idx] : (double)((const float*)p)[idx];
}
/* one step of a chain: fused, or (the wrong order "multiply and add rounded separately"; -ffp-contract=off) in two roundings */
static inline double k7_step(double u, double x, double acc, int split) {
  if (split) { const double t = u * x; return t + acc; }
  return fma(u, x, acc);
}

/* K7a's slice rule: ceil(I / 128) tile rows, the pairs of the upper triangle, K cut into max(1, 1024 / pairs) slices at most, a
 * slice rounded up to 32 columns and never below 4,096. */
void oracle_mode_gram_plan(int64_t I, int64_t K, int64_t* pairs, int64_t* slice, int64_t* splits) {
  const int64_t tiles = (I + 127) / 128;
  *pairs = tiles * (tiles + 1) / 2;
  const int64_t smax = 1024 / *pairs > 1 ? 1024 / *pairs : 1;
  int64_t s = (K + smax - 1) / smax;
  s = (s + 31) / 32 * 32;
  *slice = s < 4096 ? 4096 : s;
  *splits = (K + *slice - 1) / *slice;
}

/* G f64[I,I] = A A^T.  Per slice every entry is one chain fma(A[i][k], A[j][k], acc), k ascending from +0.0 (what the f64 matrix
 * instruction accumulates over its steps of four k); the slices are added s = 0.0; s += part, ascending; i <= j is computed once and
 * mirrored.  Wrong orders: 1 k descending inside a slice; 2 multiply and add rounded separately; 3 one chain over the whole K, no
 * slices; 4 the slices added descending. */
void oracle_mode_gram(const void* A, int a_f64, int64_t I, int64_t K, double* G, int variant) {
  int64_t pairs, slice, splits;
  oracle_mode_gram_plan(I, K, &pairs, &slice, &splits);
  if (variant == 3) { slice = K; splits = 1; }
  double* D = (double*)malloc((size_t)I * (size_t)K * sizeof(double));   /* the one conversion per element */
  for (int64_t e = 0; e < I * K; ++e) D[e] = k7_load(A, a_f64, e);
#pragma omp parallel for schedule(dynamic)
  for (int64_t i = 0; i < I; ++i)
    for (int64_t j = i; j < I; ++j) {
      const double *a = D + i * K, *b = D + j * K;
      double s = 0.0;
      for (int64_t t = 0; t < splits; ++t) {
        const int64_t sp = variant == 4 ? splits - 1 - t : t;
        const int64_t kbeg = sp * slice, kend = kbeg + slice < K ? kbeg + slice : K;
        double acc = 0.0;
        if (variant == 1)
          for (int64_t k = kend - 1; k >= kbeg; --k) acc = fma(a[k], b[k], acc);
        else if (variant == 2)
          for (int64_t k = kbeg; k < kend; ++k) acc = k7_step(a[k], b[k], acc, 1);
        else
          for (int64_t k = kbeg; k < kend; ++k) acc = fma(a[k], b[k], acc);
        s += acc;
      }
      G[i * I + j] = s;
      G[j * I + i] = s;
    }
  free(D);
}

/* One pose mode's Gram: the mode has extent n, O cells outside it and J inside (cell = (o n + a) J + j).  A slab is one identity by
 * tc columns; partial b of parts = min(slabs, 1024) takes the slabs b, b + parts, ...; within a slab wave w of 4 takes the (o, j)
 * pairs w, w + 4, ... (o j = o J + j) and for each runs the slab's columns ascending, one fma chain per entry that goes on over
 * the wave's pairs and the partial's slabs (the columns beyond M are zero and change nothing).  The four waves are added
 * 0.0 + w0 + w1 + w2 + w3, then the partials ascending from 0.0; the upper triangle is computed and mirrored. */
static void k7_pose_gram(const void* X, int x_f64, int64_t I, int cells, int64_t M, int O, int n, int J, int tc, int variant, double* G) {
  const int64_t mtiles = (M + tc - 1) / tc, slabs = I * mtiles;
  const int parts = (int)(slabs < 1024 ? slabs : 1024);
  const int OJ = O * J, quarter = (OJ + 3) / 4;
  double* part = (double*)malloc((size_t)parts * n * n * sizeof(double));
#pragma omp parallel for schedule(dynamic)
  for (int b = 0; b < parts; ++b) {
    double acc[4][32][32];
    memset(acc, 0, sizeof acc);
    for (int w = 0; w < 4; ++w)
      for (int64_t sl = b; sl < slabs; sl += parts) {
        const int64_t i = sl / mtiles, m0 = (sl - i * mtiles) * tc;
        const int first = variant == 1 ? w * quarter : w, step = variant == 1 ? 1 : 4;
        const int last = variant == 1 ? ((w + 1) * quarter < OJ ? (w + 1) * quarter : OJ) : OJ;
        for (int oj = first; oj < last; oj += step) {
          const int o = oj / J, j = oj - o * J;
          for (int c = 0; c < tc && m0 + c < M; ++c) {
            double x[32];
            for (int a = 0; a < n; ++a) x[a] = k7_load(X, x_f64, (i * cells + (int64_t)((o * n + a) * J + j)) * M + m0 + c);
            for (int a = 0; a < n; ++a)
              for (int a2 = a; a2 < n; ++a2) acc[w][a][a2] = fma(x[a], x[a2], acc[w][a][a2]);
          }
        }
      }
    for (int a = 0; a < n; ++a)
      for (int a2 = a; a2 < n; ++a2) {
        double s = 0.0;
        for (int w = 0; w < 4; ++w) s += acc[w][a][a2];
        part[((size_t)b * n + a) * n + a2] = s;
      }
  }
  for (int a = 0; a < n; ++a)
    for (int a2 = a; a2 < n; ++a2) {
      double s = 0.0;
      for (int t = 0; t < parts; ++t) s += part[((size_t)(variant == 3 ? parts - 1 - t : t) * n + a) * n + a2];
      G[a * n + a2] = s;
      G[a2 * n + a] = s;
    }
  free(part);
}

/* Gy f64[ny,ny], Gp f64[np,np], Gr f64[nr,nr] of X [I,ny,np,nr,M]; a NULL output is skipped.  A slab is 32 columns wide for f32
 * input and 16 for f64 input.  Wrong orders: 1 each wave takes a contiguous quarter of the (o, j) pairs; 2 32-column slabs for
 * f64 input too; 3 the partials added descending. */
void oracle_pose_grams(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr,
                       int variant) {
  const int tc = x_f64 && variant != 2 ? 16 : 32, cells = ny * np * nr;
  if (Gy) k7_pose_gram(X, x_f64, I, cells, M, 1, ny, np * nr, tc, variant, Gy);
  if (Gp) k7_pose_gram(X, x_f64, I, cells, M, ny, np, nr, tc, variant, Gp);
  if (Gr) k7_pose_gram(X, x_f64, I, cells, M, ny * np, nr, 1, tc, variant, Gr);
}

/* out[r][k] = sum_i U[i][r] A[i][k], A f32[I,K], U f64[I,R], R <= 16: one chain fma(U[i][r], (double)A[i][k], acc), i ascending
 * from +0.0; an f32 output is that sum cast once.  Wrong orders: 1 i descending; 2 multiply and add rounded separately; 3 U
 * rounded to f32. */
void oracle_project_identity(const float* A, int64_t I, int64_t K, const double* U, int R, void* out, int out_f64, int variant) {
#pragma omp parallel for schedule(static)
  for (int64_t k = 0; k < K; ++k) {
    double acc[16];
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (int64_t t = 0; t < I; ++t) {
      const int64_t i = variant == 1 ? I - 1 - t : t;
      const double x = (double)A[i * K + k];
      for (int r = 0; r < R; ++r) {
        const double u = variant == 3 ? (double)(float)U[i * R + r] : U[i * R + r];
        acc[r] = k7_step(u, x, acc[r], variant == 2);
      }
    }
    for (int r = 0; r < R; ++r) {
      if (out_f64) ((double*)out)[(int64_t)r * K + k] = acc[r];
      else ((float*)out)[(int64_t)r * K + k] = (float)acc[r];
    }
  }
}

/* out [I,ny',np',nr',M] = X x_2 Uy^T x_3 Up^T x_4 Ur^T, Uy f64[ny,ry] etc. (ranks <= 3).  Three nested fma chains, each ascending
 * from +0.0: over roll tr[c] = fma(Ur[r][c], x, tr[c]); over pitch tp[b][c] = fma(Up[p][b], tr[c], tp[b][c]); over yaw
 * acc[a][b][c] = fma(Uy[y][a], tp[b][c], acc[a][b][c]).  A NULL factor keeps its mode (n' = n): its chain has the one step of the
 * output's own index, with coefficient 1.0.  An f32 output is the sum cast once.  Wrong orders: 1 every chain descending;
 * 2 multiply and add rounded separately; 3 the Kronecker form, coefficient (Uy Up) Ur and one chain over (y, p, r); 4 yaw innermost
 * (yaw inside pitch inside roll). */
void oracle_project_pose(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up,
                         int rp, const double* Ur, int rr, void* out, int out_f64, int variant) {
  const int RY = Uy ? ry : 1, RP = Up ? rp : 1, RR = Ur ? rr : 1;
  const int by = Uy ? 1 : ny, bp = Up ? 1 : np, br = Ur ? 1 : nr;
  const int oy = Uy ? ry : ny, op = Up ? rp : np, orr = Ur ? rr : nr;
  const int64_t total = I * by * bp * br * M;
  const int split = variant == 2, desc = variant == 1;
#pragma omp parallel for schedule(static)
  for (int64_t idx = 0; idx < total; ++idx) {
    int64_t q = idx / M;
    const int64_t m = idx - q * M;
    const int rb = (int)(q % br); q /= br;
    const int pb = (int)(q % bp); q /= bp;
    const int yb = (int)(q % by);
    const int64_t i = q / by;
    const int y0 = Uy ? 0 : yb, y1 = Uy ? ny : yb + 1, p0 = Up ? 0 : pb, p1 = Up ? np : pb + 1, r0 = Ur ? 0 : rb, r1 = Ur ? nr : rb + 1;
    const int64_t xi = i * ny * np * nr * M + m;
#define K7_X(y, p, r) k7_load(X, x_f64, xi + (int64_t)(((y) * np + (p)) * nr + (r)) * M)
#define K7_UY(y, a) (Uy ? Uy[(y) * RY + (a)] : 1.0)
#define K7_UP(p, b) (Up ? Up[(p) * RP + (b)] : 1.0)
#define K7_UR(r, c) (Ur ? Ur[(r) * RR + (c)] : 1.0)
    double acc[3][3][3];
    memset(acc, 0, sizeof acc);
    if (variant == 3) {
      for (int y = y0; y < y1; ++y)
        for (int p = p0; p < p1; ++p)
          for (int r = r0; r < r1; ++r) {
            const double x = K7_X(y, p, r);
            for (int a = 0; a < RY; ++a)
              for (int b = 0; b < RP; ++b)
                for (int c = 0; c < RR; ++c) acc[a][b][c] = fma((K7_UY(y, a) * K7_UP(p, b)) * K7_UR(r, c), x, acc[a][b][c]);
          }
    } else if (variant == 4) {
      for (int r = r0; r < r1; ++r) {
        double tp[3][3];
        memset(tp, 0, sizeof tp);
        for (int p = p0; p < p1; ++p) {
          double ty[3] = {0.0, 0.0, 0.0};
          for (int y = y0; y < y1; ++y) {
            const double x = K7_X(y, p, r);
            for (int a = 0; a < RY; ++a) ty[a] = fma(K7_UY(y, a), x, ty[a]);
          }
          for (int a = 0; a < RY; ++a)
            for (int b = 0; b < RP; ++b) tp[a][b] = fma(K7_UP(p, b), ty[a], tp[a][b]);
        }
        for (int a = 0; a < RY; ++a)
          for (int b = 0; b < RP; ++b)
            for (int c = 0; c < RR; ++c) acc[a][b][c] = fma(K7_UR(r, c), tp[a][b], acc[a][b][c]);
      }
    } else {
      for (int ty_ = 0; ty_ < y1 - y0; ++ty_) {
        const int y = desc ? y1 - 1 - ty_ : y0 + ty_;
        double tp[3][3];
        memset(tp, 0, sizeof tp);
        for (int tp_ = 0; tp_ < p1 - p0; ++tp_) {
          const int p = desc ? p1 - 1 - tp_ : p0 + tp_;
          double tr[3] = {0.0, 0.0, 0.0};
          for (int tr_ = 0; tr_ < r1 - r0; ++tr_) {
            const int r = desc ? r1 - 1 - tr_ : r0 + tr_;
            const double x = K7_X(y, p, r);
            for (int c = 0; c < RR; ++c) tr[c] = k7_step(K7_UR(r, c), x, tr[c], split);
          }
          for (int b = 0; b < RP; ++b)
            for (int c = 0; c < RR; ++c) tp[b][c] = k7_step(K7_UP(p, b), tr[c], tp[b][c], split);
        }
        for (int a = 0; a < RY; ++a)
          for (int b = 0; b < RP; ++b)
            for (int c = 0; c < RR; ++c) acc[a][b][c] = k7_step(K7_UY(y, a), tp[b][c], acc[a][b][c], split);
      }
    }
#undef K7_X
#undef K7_UY
#undef K7_UP
#undef K7_UR
    const int64_t oi = i * oy * op * orr * M + m;
    for (int a = 0; a < RY; ++a)
      for (int b = 0; b < RP; ++b)
        for (int c = 0; c < RR; ++c) {
          const int64_t at = oi + (int64_t)(((Uy ? a : yb) * op + (Up ? b : pb)) * orr + (Ur ? c : rb)) * M;
          if (out_f64) ((double*)out)[at] = acc[a][b][c];
          else ((float*)out)[at] = (float)acc[a][b][c];
        }
  }
}

/* ---- K9: one training step of the landmark encoder, launch by launch ------------------------
 * The OPERATION ORDERS of nlml_encoder_train_steps, written from the prose at the top of nlml_hpe_amd/csrc/encoder_train_ref.h
 * ("THE GEMM ORDER", "THE OTHER SUMS"); no kernel header is included, nothing is shared with that file's et_host_* functions, and
 * libm enters through fmaf, fma, sqrt and (oracle_et_tanhf alone) tanhf.  Unlike the host form an index k >= K is NOT skipped: it is
 * a +0 operand of an fmaf, as on the matrix core, so the sign of a zero is the device's.  (A row or a column of a tile beyond the
 * matrix is such an operand too; its chains end in elements nobody stores, so the model does not form them.)  variant 0 is the
 * order; the others are deliberately WRONG orders with which tests/test_encoder_train_order_host.py shows that the inputs of
 * tests/test_encoder_train_order_gpu.py tell them apart:
 *   1 natural k order inside a super-chunk          5 bias runs of a fixed 16 rows
 *   2 the wave partials added as a halving tree     6 the loss tree over B slots instead of 256
 *   3 spw = floor(nsc / 8), the rest on wave 7      7 a tile's norm partial accumulated in f32
 *   4 the start vector added after the wave sum     8 the update with c g contracted into the following fmaf
 * A function ignores the variants that are not its own. */
enum { ET9_WAVES = 8, ET9_SUPER = 16, ET9_TILE = 32, ET9_THREADS = 512, ET9_RUNS = 16, ET9_LOSS_SLOTS = 256, ET9_LATENT = 9 };
static const int et9_widths[6] = {1024, 512, 256, 128, 64, 9};

static inline int64_t et9_row(const int32_t* rows, int64_t r) { return rows ? (int64_t)rows[r] : r; }

/* C[m][n] (row stride ldc) = sum_k a(m, k) b(k, n), M x N x K.  An operand is k-contiguous (kc != 0: a(m, k) = A[row(m) lda + k],
 * b(k, n) = Bm[row(n) ldb + k]) or k-outer (a(m, k) = A[row(k) lda + m], b(k, n) = Bm[row(k) ldb + n]); row(r) = rows ? rows[r] : r
 * gathers the STORAGE row.  start [N] or NULL: wave 0 begins its chain of column n from start[n] instead of +0.
 * The order: k is cut into nsc = ceil(K / 16) super-chunks; wave w of 8 owns [w spw, (w + 1) spw) cut at nsc, spw = ceil(nsc / 8);
 * inside super-chunk s it visits k = 16 s + 8 u + 4 h + j for u = 0, 1; j = 0..3; h = 0, 1 (h innermost) as p = fmaf(a, b, p); a wave
 * without super-chunks keeps its start; the element is ((p_0 + p_1) + p_2) + ... + p_7. */
void oracle_et_gemm(const float* A, int64_t lda, int a_kc, const int32_t* a_rows, const float* Bm, int64_t ldb, int b_kc,
                    const int32_t* b_rows, const float* start, int M, int N, int K, float* C, int64_t ldc, int variant) {
  const int nsc = (K + ET9_SUPER - 1) / ET9_SUPER;
  const int spw = variant == 3 ? nsc / ET9_WAVES : (nsc + ET9_WAVES - 1) / ET9_WAVES;
  const int Kp = ET9_SUPER * nsc;
  int* ks = (int*)malloc((size_t)(Kp + 1) * sizeof(int));
  int wbeg[ET9_WAVES + 1], cnt = 0;
  for (int w = 0; w < ET9_WAVES; ++w) {
    const int s0 = w * spw < nsc ? w * spw : nsc;
    int s1 = s0 + spw < nsc ? s0 + spw : nsc;
    if (variant == 3 && w == ET9_WAVES - 1) s1 = nsc;
    wbeg[w] = cnt;
    for (int s = s0; s < s1; ++s) {
      if (variant == 1) {
        for (int i = 0; i < ET9_SUPER; ++i) ks[cnt++] = ET9_SUPER * s + i;
      } else {
        for (int u = 0; u < 2; ++u)
          for (int j = 0; j < 4; ++j)
            for (int h = 0; h < 2; ++h) ks[cnt++] = ET9_SUPER * s + 8 * u + 4 * h + j;
      }
    }
  }
  wbeg[ET9_WAVES] = cnt;
  /* both operands in visiting order, one vector per output row / column; k >= K stays the +0.0f of calloc */
  float* Pa = (float*)calloc((size_t)M * (size_t)(cnt + 1), sizeof(float));
  float* Pb = (float*)calloc((size_t)N * (size_t)(cnt + 1), sizeof(float));
  for (int m = 0; m < M; ++m)
    for (int i = 0; i < cnt; ++i) {
      const int k = ks[i];
      if (k < K) Pa[(size_t)m * cnt + i] = a_kc ? A[et9_row(a_rows, m) * lda + k] : A[et9_row(a_rows, k) * lda + m];
    }
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < cnt; ++i) {
      const int k = ks[i];
      if (k < K) Pb[(size_t)n * cnt + i] = b_kc ? Bm[et9_row(b_rows, n) * ldb + k] : Bm[et9_row(b_rows, k) * ldb + n];
    }
#pragma omp parallel for schedule(static)
  for (int64_t e = 0; e < (int64_t)M * N; ++e) {
    const int m = (int)(e / N), n = (int)(e % N);
    const float *a = Pa + (size_t)m * cnt, *b = Pb + (size_t)n * cnt;
    float p[ET9_WAVES];
    for (int w = 0; w < ET9_WAVES; ++w) {
      float acc = (w == 0 && start && variant != 4) ? start[n] : 0.0f;
      for (int i = wbeg[w]; i < wbeg[w + 1]; ++i) acc = fmaf(a[i], b[i], acc);
      p[w] = acc;
    }
    float t;
    if (variant == 2) {
      for (int stride = ET9_WAVES / 2; stride >= 1; stride /= 2)
        for (int w = 0; w < stride; ++w) p[w] = p[w] + p[w + stride];
      t = p[0];
    } else {
      t = p[0];
      for (int w = 1; w < ET9_WAVES; ++w) t = t + p[w];
    }
    if (variant == 4 && start) t = t + start[n];
    C[(int64_t)m * ldc + n] = t;
  }
  free(Pa);
  free(Pb);
  free(ks);
}

/* db[o] of delta [B, out] (row stride ldd): sixteen runs of ceil(B / 16) rows, a run summed b ascending from +0, the runs added in
 * order beginning with run 0 (the runs beyond the batch are +0). */
void oracle_et_bias_grad(const float* delta, int64_t ldd, int B, int out, float* db, int variant) {
  const int rp = variant == 5 ? 16 : (B + ET9_RUNS - 1) / ET9_RUNS;
  for (int o = 0; o < out; ++o) {
    float run[ET9_RUNS];
    for (int r = 0; r < ET9_RUNS; ++r) {
      float s = 0.0f;
      const int hi = (r + 1) * rp < B ? (r + 1) * rp : B;
      for (int b = r * rp; b < hi; ++b) s = s + delta[(int64_t)b * ldd + o];
      run[r] = s;
    }
    float total = run[0];
    for (int r = 1; r < ET9_RUNS; ++r) total = total + run[r];
    db[o] = total;
  }
}

/* pred [B, 9] (row stride ldp) against target [B, 9] (tight): q[b] = the fmaf chain of the nine squared residuals, j ascending from
 * +0; slots [256]: q then zeros, after the halving tree (slot t += slot t + stride; stride 128, 64, .., 1), so slots[0] is the total;
 * *loss = total / float(3B); delta6 [B, 9] (tight) = residual * float(2 / (3B)). */
void oracle_et_loss(const float* pred, int64_t ldp, const float* target, int B, float* q, float* slots, float* loss, float* delta6,
                    int variant) {
  const float scale = (float)(2.0 / (3.0 * (double)B));
  for (int t = 0; t < ET9_LOSS_SLOTS; ++t) slots[t] = 0.0f;
  for (int b = 0; b < B; ++b) {
    float s = 0.0f;
    for (int j = 0; j < ET9_LATENT; ++j) {
      const float d = pred[(int64_t)b * ldp + j] - target[b * ET9_LATENT + j];
      delta6[b * ET9_LATENT + j] = d * scale;
      s = fmaf(d, d, s);
    }
    q[b] = s;
    slots[b] = s;
  }
  if (variant == 6) {   /* a tree over the B slots in use: the upper half folded onto the lower until one is left */
    for (int n = B; n > 1;) {
      const int half = (n + 1) / 2;
      for (int t = 0; t + half < n; ++t) slots[t] = slots[t] + slots[t + half];
      n = half;
    }
  } else {
    for (int stride = ET9_LOSS_SLOTS / 2; stride >= 1; stride /= 2)
      for (int t = 0; t < stride; ++t) slots[t] = slots[t] + slots[t + stride];
  }
  *loss = slots[0] / (float)(3 * B);
}

/* the number of wgrad tiles (= norm partials) of an encoder with F inputs */
int oracle_et_n_partials(int F) {
  int n = 0, fan_in = F;
  for (int l = 0; l < 6; ++l) {
    n += ((et9_widths[l] + ET9_TILE - 1) / ET9_TILE) * ((fan_in + ET9_TILE - 1) / ET9_TILE);
    fan_in = et9_widths[l];
  }
  return n;
}

static double et9_tree512(double* s) {
  for (int stride = ET9_THREADS / 2; stride >= 1; stride /= 2)
    for (int t = 0; t < stride; ++t) s[t] = s[t] + s[t + stride];
  return s[0];
}

/* The norm of the accumulator G (the flat gradient buffer: W_0 [1024, F], b_0, W_1 [512, 1024], b_1, ...), f64.
 * G != NULL: partials [n_partials] are formed from it -- layer 0's 32 x 32 tiles first, row-major within a layer; thread t of 512
 * takes elements t and t + 512 of its tile (element e = row e / 32, column e % 32; those beyond the matrix are skipped) as
 * s = fma(g, g, s) from +0, thread o < 32 of a tile in the first tile column then the bias gradient of the tile's row o, and a
 * halving tree over the 512 slots gives the partial.  G == NULL: the partials are taken from partials_in.
 * Then chains [512]: chain t = partials t, t + 512, .. added ascending from +0; tree [512]: the chains after the same halving tree;
 * *norm = sqrt(tree[0]); *c = min(1, max_norm / (norm + 1e-6)). */
void oracle_et_norm(const float* G, int F, const double* partials_in, double max_norm, double* partials, double* chains, double* tree,
                    double* norm, double* c, int variant) {
  const int n_partials = oracle_et_n_partials(F);
  if (G) {
    int fan_in = F, part = 0;
    int64_t off = 0;
    for (int l = 0; l < 6; ++l) {
      const int out = et9_widths[l], in = fan_in;
      const float *gW = G + off, *gb = G + off + (int64_t)out * in;
      const int tn_n = (in + ET9_TILE - 1) / ET9_TILE;
      for (int tm = 0; tm < (out + ET9_TILE - 1) / ET9_TILE; ++tm)
        for (int tn = 0; tn < tn_n; ++tn) {
          double s[ET9_THREADS];
          float sf[ET9_THREADS];
          for (int t = 0; t < ET9_THREADS; ++t) {
            double acc = 0.0;
            float accf = 0.0f;
            for (int half = 0; half < 2; ++half) {
              const int e = t + ET9_THREADS * half;
              const int o = tm * ET9_TILE + e / ET9_TILE, i = tn * ET9_TILE + e % ET9_TILE;
              if (o >= out || i >= in) continue;
              const float g = gW[(int64_t)o * in + i];
              acc = fma((double)g, (double)g, acc);
              accf = fmaf(g, g, accf);
            }
            if (tn == 0 && t < ET9_TILE && tm * ET9_TILE + t < out) {
              const float g = gb[tm * ET9_TILE + t];
              acc = fma((double)g, (double)g, acc);
              accf = fmaf(g, g, accf);
            }
            s[t] = acc;
            sf[t] = accf;
          }
          if (variant == 7) {
            for (int stride = ET9_THREADS / 2; stride >= 1; stride /= 2)
              for (int t = 0; t < stride; ++t) sf[t] = sf[t] + sf[t + stride];
            partials[part++] = (double)sf[0];
          } else {
            partials[part++] = et9_tree512(s);
          }
        }
      off += (int64_t)out * in + out;
      fan_in = out;
    }
  } else {
    for (int i = 0; i < n_partials; ++i) partials[i] = partials_in[i];
  }
  for (int t = 0; t < ET9_THREADS; ++t) {
    double s = 0.0;
    for (int i = t; i < n_partials; i += ET9_THREADS) s = s + partials[i];
    chains[t] = s;
    tree[t] = s;
  }
  et9_tree512(tree);
  *norm = sqrt(tree[0]);
  const double r = max_norm / (*norm + 1e-6);
  *c = r < 1.0 ? r : 1.0;
}

/* n elements in place: g <- c g (one rounding); d = fmaf(wd, p, g); p <- fmaf(-lr, d, p) */
void oracle_et_update(float* p, float* g, int64_t n, float c, float lr, float wd, int variant) {
  for (int64_t e = 0; e < n; ++e) {
    const float gc = c * g[e];
    float d = fmaf(wd, p[e], gc);
    if (variant == 8) { const float t = wd * p[e]; d = fmaf(c, g[e], t); }   /* c g never rounded on its way into d */
    g[e] = gc;
    p[e] = fmaf(-lr, d, p[e]);
  }
}

/* out = s * act'(a), element by element: ReLU (a > 0 ? 1 : 0) or, tanh_layer != 0, fmaf(-a, a, 1) */
void oracle_et_act_grad(const float* s, const float* a, int64_t n, int tanh_layer, float* out) {
  for (int64_t e = 0; e < n; ++e) out[e] = s[e] * (tanh_layer ? fmaf(-a[e], a[e], 1.0f) : (a[e] > 0.0f ? 1.0f : 0.0f));
}

/* this machine's libm tanhf: the host form's layer 4, NOT the device's */
void oracle_et_tanhf(const float* z, int64_t n, float* out) {
  for (int64_t e = 0; e < n; ++e) out[e] = tanhf(z[e]);
}
