// pose_eval.hip -- K5: the evaluation block of the test entry point (NLML_HPE_Test.py:95-152 of the reference, the
// numpy post-processing of this repository's NLML_HPE_Test.py) in one pass over the predictions.
//
// Per face, all in f64:
//   pred  = rint(deg(pose) * 10^d) / 10^d          np.round(np.degrees(pose.astype(f64)), d); no rounding when d < 0
//   keep  = valid && all(lo <= gt <= hi)            the GT range filter and the no-face filter
//   e     = |gt - pred|                             per axis
//   v     = acos(clamp(dot(c_gt, c_pred), -1, 1)) * 180/pi over the l/b/f columns c of R = Rx(pitch) Ry(-yaw) Rz(roll)
// Reduced over the kept faces: count, mean and M2 of e per axis, the sums of the three vector errors, and per interval k
// (axis a_k, [low_k, high_k) on the GT angle) the count and the sum of e[a_k]; counted over all rows: no face, out of range.
//
// Launch 1 (one workgroup per FACES_PER_RECORD faces, a constant) writes one record per workgroup; launch 2 (one workgroup)
// merges the records in index order: Chan's pairwise merge for (count, mean, M2), plain sums for everything else.  No atomics and
// no hand-off inside a launch, and the grid does not depend on the CU count, so the result depends only on the inputs.
//
// Record (doubles, record_len(K) = 12 + 2K):
//   0 kept   1 no face   2 out of range   3..5 mean e   6..8 M2 e   9..11 sum v (left, down, front)   12+2k count_k   13+2k sum_k
// Result (result_len(K) = 14 + 2K):
//   0..2 mae yaw/pitch/roll  3 mae total  4 maev  5..7 v left/down/front  8..10 std yaw/pitch/roll (ddof 1)
//   11 kept  12 no face  13 out of range  14+2k count_k  15+2k mae_k (NaN where count_k = 0)
#include <hip/hip_runtime.h>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"

namespace nlml {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFacesPerThread = NLML_POSE_EVAL_FACES_PER_RECORD / kThreads;
static_assert(kFacesPerThread * kThreads == NLML_POSE_EVAL_FACES_PER_RECORD, "faces per record");
constexpr int kMaxK = NLML_POSE_EVAL_MAX_INTERVALS;
constexpr int kMaxL = 12 + 2 * kMaxK;

constexpr double kDeg = 57.29577951308232;        // np.degrees: x * (180/pi)
constexpr double kRad = 0.017453292519943295;     // np.radians: x * (pi/180)

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;                                        // lane 0 holds the wave's sum
}

__device__ inline double pick(int a, const double* v) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// clamp that lets a NaN through, as np.clip / torch.clamp do
__device__ inline double clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

// the l / b / f columns of Rx(rx) Ry(ry) Rz(rz), rx = pitch, ry = -yaw, rz = roll (radians)
__device__ inline void columns(double yaw, double pitch, double roll, double c[9]) {
  double sx, cx, sy, cy, sz, cz;
  sincos(pitch * kRad, &sx, &cx);
  sincos(-(yaw * kRad), &sy, &cy);
  sincos(roll * kRad, &sz, &cz);
  c[0] = cy * cz;            c[1] = sx * sy * cz + cx * sz;    c[2] = -cx * sy * cz + sx * sz;   // l
  c[3] = -cy * sz;           c[4] = -sx * sy * sz + cx * cz;   c[5] = cx * sy * sz + sx * cz;    // b
  c[6] = sy;                 c[7] = -sx * cy;                  c[8] = cx * cy;                   // f
}

// (n, mean, M2) <- (n, mean, M2) merged with (nb, mb, Mb), Chan et al.; an empty side leaves the other as it is
__device__ inline void chan(double& n, double& m, double& M, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (n == 0.0) { n = nb; m = mb; M = Mb; return; }
  const double t = n + nb, d = mb - m;
  m = m + d * (nb / t);
  M = M + Mb + d * d * (n * (nb / t));
  n = t;
}

__global__ void __launch_bounds__(kThreads) pose_eval_records(const float* __restrict__ pose_rad, const double* __restrict__ pred_deg,
                                                              const uint8_t* __restrict__ valid, const double* __restrict__ gt_deg,
                                                              int64_t B, PoseEvalArgs args, double* __restrict__ records,
                                                              double* __restrict__ pred_out, uint8_t* __restrict__ keep_out) {
  __shared__ double lds[kWaves * kMaxL + kMaxL];
  double* red = lds;                               // [kWaves][L] wave partials
  double* tot = lds + kWaves * kMaxL;              // [L] the workgroup's sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = args.K, L = 12 + 2 * K;
  const int64_t base = (int64_t)blockIdx.x * NLML_POSE_EVAL_FACES_PER_RECORD;
  const double scale = args.decimals >= 0 ? args.scale : 1.0;

  double g[kFacesPerThread][3], e[kFacesPerThread][3];
  bool kp[kFacesPerThread];
  double cnt[3] = {0.0, 0.0, 0.0}, se[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < kFacesPerThread; ++i) {
    const int64_t f = base + i * kThreads + tid;
    kp[i] = false;
    e[i][0] = e[i][1] = e[i][2] = 0.0;
    g[i][0] = g[i][1] = g[i][2] = 0.0;
    if (f >= B) continue;
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      g[i][a] = gt_deg[f * 3 + a];
      double x = pose_rad ? (double)pose_rad[f * 3 + a] * kDeg : pred_deg[f * 3 + a];
      if (args.decimals >= 0) x = rint(x * scale) / scale;
      p[a] = x;
      if (pred_out) pred_out[f * 3 + a] = x;
    }
    const bool v = valid ? valid[f] != 0 : true;
    bool in_range = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) in_range = in_range && (g[i][a] >= args.lo[a]) && (g[i][a] <= args.hi[a]);
    kp[i] = v && in_range;
    if (keep_out) keep_out[f] = kp[i] ? 1 : 0;
    cnt[1] += v ? 0.0 : 1.0;
    cnt[2] += in_range ? 0.0 : 1.0;
    if (!kp[i]) continue;
    cnt[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      e[i][a] = fabs(g[i][a] - p[a]);
      se[a] += e[i][a];
    }
    double cg[9], cp[9];
    columns(g[i][0], g[i][1], g[i][2], cg);
    columns(p[0], p[1], p[2], cp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double dot = cg[3 * c] * cp[3 * c] + cg[3 * c + 1] * cp[3 * c + 1] + cg[3 * c + 2] * cp[3 * c + 2];
      sv[c] += acos(clamp1(dot)) * (180.0 / 3.141592653589793);
    }
  }

  // pass 1: counts, sums of e, sums of v, interval counts and sums -> wave sums -> LDS
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double r0 = wave_sum(cnt[a]), r1 = wave_sum(se[a]), r2 = wave_sum(sv[a]);
    if (lane == 0) { red[wave * kMaxL + a] = r0; red[wave * kMaxL + 3 + a] = r1; red[wave * kMaxL + 9 + a] = r2; }
  }
  for (int k = 0; k < K; ++k) {
    const int ax = args.axes[k];
    const double lo = args.ivl[k][0], hi = args.ivl[k][1];
    double c = 0.0, s = 0.0;
#pragma unroll
    for (int i = 0; i < kFacesPerThread; ++i) {
      const double gv = pick(ax, g[i]);
      if (kp[i] && gv >= lo && gv < hi) { c += 1.0; s += pick(ax, e[i]); }
    }
    c = wave_sum(c);
    s = wave_sum(s);
    if (lane == 0) { red[wave * kMaxL + 12 + 2 * k] = c; red[wave * kMaxL + 13 + 2 * k] = s; }
  }
  __syncthreads();
  for (int j = tid; j < L; j += kThreads) {
    if (j >= 6 && j < 9) continue;                 // M2: pass 2
    double t = red[j];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += red[w * kMaxL + j];
    tot[j] = t;
  }
  __syncthreads();

  // pass 2: M2 about the workgroup's mean
  const double n = tot[0];
  double mean[3], m2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { mean[a] = n > 0.0 ? tot[3 + a] / n : 0.0; m2[a] = 0.0; }
#pragma unroll
  for (int i = 0; i < kFacesPerThread; ++i)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double d = e[i][a] - mean[a];
      m2[a] += kp[i] ? d * d : 0.0;
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double r = wave_sum(m2[a]);
    if (lane == 0) red[wave * kMaxL + 6 + a] = r;
  }
  __syncthreads();
  double* rec = records + (int64_t)blockIdx.x * L;
  for (int j = tid; j < L; j += kThreads) {
    double v;
    if (j >= 3 && j < 6) {
      v = mean[j - 3];
    } else if (j >= 6 && j < 9) {
      v = red[j];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += red[w * kMaxL + j];
    } else {
      v = tot[j];
    }
    rec[j] = v;
  }
}

// Launch 2.  Items: 0..2 = the (n, mean, M2) triple of axis i; i >= 3 = a plain sum of record field sum_field(i) (the counts, the
// vector sums, the interval counts and sums).  The records stream through LDS in tiles of whole records; inside a tile, lane p of
// kLanes takes a contiguous run of records, and after the tile the lanes are folded in order into the running value: a left fold
// of contiguous blocks, i.e. index order.
constexpr int kLanes = 16;
constexpr int kMaxItems = kMaxL - 3;
constexpr int kTile = 12288;                       // doubles (96 KB)
constexpr int kLoadUnroll = 16;

__device__ inline int sum_field(int i) { return i < 6 ? i - 3 : i + 3; }   // 3,4,5 -> 0,1,2 ; 6.. -> 9..

__global__ void __launch_bounds__(kThreads) pose_eval_merge_kernel(const double* __restrict__ records, int64_t n_rec, int K,
                                                                   double* __restrict__ record_out, double* __restrict__ result_out) {
  __shared__ double lds[kTile + kLanes * kMaxItems * 3 + kMaxL];
  double* tile = lds;
  double* part = lds + kTile;                      // [kLanes][items][3]
  double* fin = part + kLanes * kMaxItems * 3;     // [L] the merged record
  const int tid = threadIdx.x;
  const int L = 12 + 2 * K, NI = L - 3;
  const int64_t per_tile = kTile / L;
  double rn = 0.0, rm = 0.0, rM = 0.0;             // thread i < NI: item i's running value (rn only for a sum)

  for (int64_t r0 = 0; r0 < n_rec; r0 += per_tile) {
    const int tr = (int)min<int64_t>(per_tile, n_rec - r0);
    const int cnt = tr * L;
    const double* src = records + r0 * L;
    for (int b = 0; b < cnt; b += kThreads * kLoadUnroll) {       // all loads of a round in flight, then the LDS stores
      double v[kLoadUnroll];
#pragma unroll
      for (int u = 0; u < kLoadUnroll; ++u) {
        const int idx = b + u * kThreads + tid;
        v[u] = idx < cnt ? src[idx] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kLoadUnroll; ++u) {
        const int idx = b + u * kThreads + tid;
        if (idx < cnt) tile[idx] = v[u];
      }
    }
    __syncthreads();
    const int per_lane = (tr + kLanes - 1) / kLanes;
    for (int it = tid; it < kLanes * NI; it += kThreads) {
      const int p = it / NI, i = it - p * NI;
      const int lo = min(p * per_lane, tr), hi = min(lo + per_lane, tr);
      double n = 0.0, m = 0.0, M = 0.0;
      if (i < 3) {
        for (int r = lo; r < hi; ++r) chan(n, m, M, tile[r * L], tile[r * L + 3 + i], tile[r * L + 6 + i]);
      } else {
        const int j = sum_field(i);
        for (int r = lo; r < hi; ++r) n += tile[r * L + j];
      }
      double* q = part + (p * kMaxItems + i) * 3;
      q[0] = n; q[1] = m; q[2] = M;
    }
    __syncthreads();
    if (tid < NI) {
      for (int p = 0; p < kLanes; ++p) {
        const double* q = part + (p * kMaxItems + tid) * 3;
        if (tid < 3) chan(rn, rm, rM, q[0], q[1], q[2]);
        else rn += q[0];
      }
    }
    __syncthreads();                               // the next tile overwrites tile and part
  }

  if (tid < NI) {
    if (tid < 3) { fin[3 + tid] = rm; fin[6 + tid] = rM; }
    else fin[sum_field(tid)] = rn;
  }
  __syncthreads();
  if (record_out)
    for (int j = tid; j < L; j += kThreads) record_out[j] = fin[j];
  const double nan = __builtin_nan("");
  const double n = fin[0];
  if (tid == 0) {
    double* o = result_out;
    const double m0 = n > 0.0 ? fin[3] : nan, m1 = n > 0.0 ? fin[4] : nan, m2 = n > 0.0 ? fin[5] : nan;
    o[0] = m0; o[1] = m1; o[2] = m2;
    o[3] = (m0 + m1 + m2) / 3.0;
    o[4] = (fin[9] + fin[10] + fin[11]) / (3.0 * n);
    o[5] = fin[9] / n; o[6] = fin[10] / n; o[7] = fin[11] / n;
    for (int a = 0; a < 3; ++a) o[8 + a] = n > 1.0 ? sqrt(fin[6 + a] / (n - 1.0)) : nan;
    o[11] = fin[0]; o[12] = fin[1]; o[13] = fin[2];
  }
  for (int k = tid; k < K; k += kThreads) {
    const double c = fin[12 + 2 * k];
    result_out[14 + 2 * k] = c;
    result_out[15 + 2 * k] = c > 0.0 ? fin[13 + 2 * k] / c : nan;
  }
}

}  // namespace

int launch_pose_eval(const float* pose_rad, const double* pred_deg, const uint8_t* valid, const double* gt_deg, int64_t B,
                     const PoseEvalArgs& args, double* workspace, double* record_out, double* result_out, double* pred_out,
                     uint8_t* keep_out, void* stream) {
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nrec = (B + NLML_POSE_EVAL_FACES_PER_RECORD - 1) / NLML_POSE_EVAL_FACES_PER_RECORD;
  if (nrec > 0) {
    hipLaunchKernelGGL(pose_eval_records, dim3((unsigned)nrec), dim3(kThreads), 0, s, pose_rad, pred_deg, valid, gt_deg, B, args,
                       workspace, pred_out, keep_out);
    if (int rc = hip_launch_status()) return rc;
  }
  return launch_pose_eval_merge(workspace, nrec, args.K, record_out, result_out, stream);
}

int launch_pose_eval_merge(const double* records, int64_t n, int K, double* record_out, double* result_out, void* stream) {
  hipLaunchKernelGGL(pose_eval_merge_kernel, dim3(1), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), records, n, K,
                     record_out, result_out);
  return hip_launch_status();
}

}  // namespace nlml
