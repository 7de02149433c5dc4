// tucker_residual_ref.h -- K11: the operation order of the Tucker expansion X_hat = W x_1 U_id x_2 Uy x_3 Up x_4 Ur (tensorly's
// tucker_to_tensor, TD_main.py:221) and of the true reconstruction error |X - X_hat| / |X| (:224), shared by the device kernel
// (tucker_residual.hip) and the host form (nlml_tucker_residual_host, abi.cpp): one body, the same bits.
//
//   X f32[I,ny,np,nr,M], W f32[R,ry,rp,rr,M], U_id f64[I,R], Uy f64[ny,ry], Up f64[np,rp], Ur f64[nr,rr], all row-major.
//
// One LANE owns one (identity i, column m).  Every chain below is ascending from +0.0 and every fma is f64:
//   v[b][c][d] = fma(U_id[i][a], (double)W[a][b][c][d][m], v[b][c][d])   over a                  (ry rp rr values, in registers)
//   ty[c][d]   = fma(Uy[y][b],  v[b][c][d], ty[c][d])                    over b   per yaw bin y
//   tp[d]      = fma(Up[p][c],  ty[c][d],   tp[d])                       over c   per pitch bin p
//   xhat       = fma(Ur[r][d],  tp[d],      xhat)                        over d   per roll bin r
//   X_hat[i][y][p][r][m] = (float)xhat                                   one rounding, where X_hat is asked for
//   x = (double)X[i][y][p][r][m],  e = x - xhat,  s = fma(e, e, s),  q = fma(x, x, q)    over the cells (y, p, r) in row-major order
// so a lane ends with s[i][m] = sum of squared residuals and q[i][m] = sum of squares of its column of identity i.
//
// The sums, without floating-point atomics, in an order that depends on the shape alone:
//   1. Column GROUP g of G = ceil(M / 64) holds the columns 64 g .. 64 g + 63, lane l the column 64 g + l; a lane past M holds
//      s = q = +0.0.  The group's 64 lanes are added by the halving tree  t[l] = t[l] + t[l + h]  for l < h,  h = 32, 16, 8, 4, 2, 1;
//      t[0] is the partial P[i][g] (s and q apart), which goes to the workspace: f64[I][G][2].
//   2. (second launch, one workgroup of TR_RED_THREADS = 256 threads)  thread t takes the identities i = t, t + 256, ...
//      ascending; for each,  res_id[i] = (..((0.0 + P[i][0]) + P[i][1]) + ..) + P[i][G-1]  (the same chain over the q partials),
//      and the thread's own totals a[t] = a[t] + res_id[i] from +0.0.  The 256 totals (0.0 for a thread without an identity) are
//      added by the same halving tree, h = 128 .. 1;  sums = {a_s[0], a_q[0]}.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_TR_HD __host__ __device__
#else
#define NLML_TR_HD
#endif

namespace nlml {

constexpr int TR_LANES = 64;          // columns of a group: one wave
constexpr int TR_RED_THREADS = 256;   // threads of the second launch
constexpr int TR_CHUNK = 8;           // cells whose loads are issued together

struct TrArgs {
  const float* X;        // NULL: expand only
  const float* W;
  const double *Uid, *Uy, *Up, *Ur;
  float* xhat;           // NULL: not asked for
  int64_t I, M;
  int R, ny, np, nr;
};

inline int64_t tr_groups(int64_t M) { return (M + TR_LANES - 1) / TR_LANES; }
inline size_t tr_workspace_bytes(int64_t I, int64_t M) { return (size_t)I * (size_t)tr_groups(M) * 2 * sizeof(double); }

// One lane: identity i, column m < M.  HAS_X: read X and accumulate s, q; HAS_XHAT: write X_hat.
template <int RY, int RP, int RR, bool HAS_X, bool HAS_XHAT>
NLML_TR_HD inline void tr_lane(const TrArgs& a, int64_t i, int64_t m, double& s, double& q) {
  double v[RY][RP][RR];
#pragma unroll
  for (int b = 0; b < RY; ++b)
#pragma unroll
    for (int c = 0; c < RP; ++c)
#pragma unroll
      for (int d = 0; d < RR; ++d) v[b][c][d] = 0.0;
  const double* uid = a.Uid + i * a.R;
  for (int r = 0; r < a.R; ++r) {
    const double u = uid[r];
    const float* w = a.W + (int64_t)r * (RY * RP * RR) * a.M + m;
#pragma unroll
    for (int b = 0; b < RY; ++b)
#pragma unroll
      for (int c = 0; c < RP; ++c)
#pragma unroll
        for (int d = 0; d < RR; ++d) v[b][c][d] = fma(u, (double)w[(int64_t)((b * RP + c) * RR + d) * a.M], v[b][c][d]);
  }
  const int64_t base = i * ((int64_t)a.ny * a.np * a.nr) * a.M + m;
  const int cells = a.ny * a.np * a.nr;
  s = 0.0;
  q = 0.0;
  // The cells in row-major order, TR_CHUNK at a time through two register buffers: the loads of the chunk after the next are in
  // flight while a chunk is computed (one load at a time leaves the device waiting on memory latency, profiles/tucker_residual.md).
  // A load past the last cell reads the last cell again and is not used.  (y, p, r) is the cell about to be computed; ty and tp are
  // rebuilt where p and r return to 0, which is the nesting of the order stated above.
  double ty[RP][RR], tp[RR];
  int y = 0, p = 0, r = 0;
  float bufA[TR_CHUNK], bufB[TR_CHUNK];
  auto fetch = [&](float (&buf)[TR_CHUNK], int c0) {
    if (HAS_X) {
#pragma unroll
      for (int k = 0; k < TR_CHUNK; ++k) {
        const int c = c0 + k < cells ? c0 + k : cells - 1;
        buf[k] = a.X[base + (int64_t)c * a.M];
      }
    }
  };
  auto compute = [&](const float (&buf)[TR_CHUNK], int c0) {
#pragma unroll
    for (int k = 0; k < TR_CHUNK; ++k) {
      if (c0 + k >= cells) break;
      if (r == 0) {
        if (p == 0) {
#pragma unroll
          for (int c = 0; c < RP; ++c)
#pragma unroll
            for (int d = 0; d < RR; ++d) {
              double t = 0.0;
#pragma unroll
              for (int b = 0; b < RY; ++b) t = fma(a.Uy[y * RY + b], v[b][c][d], t);
              ty[c][d] = t;
            }
        }
#pragma unroll
        for (int d = 0; d < RR; ++d) {
          double t = 0.0;
#pragma unroll
          for (int c = 0; c < RP; ++c) t = fma(a.Up[p * RP + c], ty[c][d], t);
          tp[d] = t;
        }
      }
      double xh = 0.0;
#pragma unroll
      for (int d = 0; d < RR; ++d) xh = fma(a.Ur[r * RR + d], tp[d], xh);
      const int64_t off = base + (int64_t)(c0 + k) * a.M;
      if (HAS_XHAT) a.xhat[off] = (float)xh;
      if (HAS_X) {
        const double x = (double)buf[k];
        const double e = x - xh;
        s = fma(e, e, s);
        q = fma(x, x, q);
      }
      if (++r == a.nr) {
        r = 0;
        if (++p == a.np) {
          p = 0;
          ++y;
        }
      }
    }
  };
  fetch(bufA, 0);
  for (int c0 = 0; c0 < cells; c0 += 2 * TR_CHUNK) {
    fetch(bufB, c0 + TR_CHUNK);
    compute(bufA, c0);
    fetch(bufA, c0 + 2 * TR_CHUNK);
    compute(bufB, c0 + TR_CHUNK);
  }
}

// The second launch's work of thread t: its identities' chains over the partials; -> its own totals.
NLML_TR_HD inline void tr_reduce_thread(const double* P, int64_t I, int64_t G, int t, double* res_id, double& as, double& aq) {
  as = 0.0;
  aq = 0.0;
  for (int64_t i = t; i < I; i += TR_RED_THREADS) {
    double rs = 0.0, rq = 0.0;
    const double* p = P + i * G * 2;
    for (int64_t g = 0; g < G; ++g) {
      rs += p[2 * g];
      rq += p[2 * g + 1];
    }
    if (res_id) res_id[i] = rs;
    as += rs;
    aq += rq;
  }
}

// The halving tree over n = 64 or 256 values, in place; the sum is t[0].
inline void tr_tree_host(double* t, int n) {
  for (int h = n / 2; h >= 1; h /= 2)
    for (int l = 0; l < h; ++l) t[l] = t[l] + t[l + h];
}

template <int RY, int RP, int RR>
inline void tr_host_ranks(const TrArgs& a, double* P) {
  const int64_t G = tr_groups(a.M);
  for (int64_t i = 0; i < a.I; ++i)
    for (int64_t g = 0; g < G; ++g) {
      double ts[TR_LANES], tq[TR_LANES];
      for (int l = 0; l < TR_LANES; ++l) {
        const int64_t m = g * TR_LANES + l;
        ts[l] = tq[l] = 0.0;
        if (m >= a.M) continue;
        if (a.X && a.xhat) tr_lane<RY, RP, RR, true, true>(a, i, m, ts[l], tq[l]);
        else if (a.X) tr_lane<RY, RP, RR, true, false>(a, i, m, ts[l], tq[l]);
        else tr_lane<RY, RP, RR, false, true>(a, i, m, ts[l], tq[l]);
      }
      if (!a.X) continue;
      tr_tree_host(ts, TR_LANES);
      tr_tree_host(tq, TR_LANES);
      P[(i * G + g) * 2] = ts[0];
      P[(i * G + g) * 2 + 1] = tq[0];
    }
}

// Dispatch on the pose ranks (each 1..3, checked by the caller): F is called as F.template run<RY, RP, RR>().
template <class F>
inline void tr_dispatch(int ry, int rp, int rr, F&& f) {
#define NLML_TR_RR(RY, RP) \
  switch (rr) { case 1: f.template run<RY, RP, 1>(); break; case 2: f.template run<RY, RP, 2>(); break; default: f.template run<RY, RP, 3>(); break; }
#define NLML_TR_RP(RY) \
  switch (rp) { case 1: NLML_TR_RR(RY, 1) break; case 2: NLML_TR_RR(RY, 2) break; default: NLML_TR_RR(RY, 3) break; }
  switch (ry) { case 1: NLML_TR_RP(1) break; case 2: NLML_TR_RP(2) break; default: NLML_TR_RP(3) break; }
#undef NLML_TR_RP
#undef NLML_TR_RR
}

struct TrHostRun {
  const TrArgs& a;
  double* P;
  template <int RY, int RP, int RR> void run() { tr_host_ranks<RY, RP, RR>(a, P); }
};

// The whole call on the host.  P: the workspace (tr_workspace_bytes), unused when a.X is NULL; sums f64[2] and res_id f64[I] as the
// device writes them (res_id may be NULL; neither is touched when a.X is NULL).
inline void tr_host(const TrArgs& a, int ry, int rp, int rr, double* P, double* sums, double* res_id) {
  tr_dispatch(ry, rp, rr, TrHostRun{a, P});
  if (!a.X) return;
  double as[TR_RED_THREADS], aq[TR_RED_THREADS];
  for (int t = 0; t < TR_RED_THREADS; ++t) tr_reduce_thread(P, a.I, tr_groups(a.M), t, res_id, as[t], aq[t]);
  tr_tree_host(as, TR_RED_THREADS);
  tr_tree_host(aq, TR_RED_THREADS);
  sums[0] = as[0];
  sums[1] = aq[0];
}

}  // namespace nlml
