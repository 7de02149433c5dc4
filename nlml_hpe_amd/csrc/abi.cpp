// abi.cpp -- the extern "C" surface declared in include/nlml_hpe.h: ALL the argument checks, in the order that header states, then the
// launchers in the .hip files, which refuse nothing.  A refusal is fail(code, text) or, where the text names its caller, refuse(code,
// who, what); every alignment test is aligned().  K2: k2_forward checks a call once, hands it on as one K2Call (abi_internal.h) and
// chains the strict-fast mode's re-evaluation launch behind whichever form ran.  No allocation, no synchronisation, no global mutable
// state beyond values read once and kept (the NLML_K2_* environment variables, a device's compute-unit count).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nlml_hpe.h"
#include "abi_internal.h"
#include "centroid_ref.h"
#include "cosine_fit_ref.h"
#include "encoder_train_ref.h"
#include "heads_train_ref.h"
#include "layout.h"
#include "powell.h"
#include "rotate_ref.h"
#include "tucker_grad_ref.h"
#include "tucker_residual_ref.h"

namespace nlml {
static thread_local char g_err[256] = "";
int fail(int code, const char* msg) {
  std::snprintf(g_err, sizeof g_err, "%s", msg ? msg : "unknown error");
  return code ? code : NLML_E_BADARG;
}
int hip_launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail((int)e, hipGetErrorString(e));
}
// the dispatcher's split of a strict-fast batch (abi_internal.h; nlml_k2_quad_split)
int64_t k2_quad_faces(int64_t B, int cus) {
  if (B <= 0 || cus <= 0) return 0;
  return (B / TILE_FACES) / (4 * (int64_t)cus) * cus * (4 * TILE_FACES);
}
}  // namespace nlml

using namespace nlml;

// The one place a refusal's text is put together: "<who>: <what>", `what` a printf format for the values behind it (a literal '%' is "%%")
__attribute__((format(printf, 3, 4))) static int refuse(int code, const char* who, const char* what, ...) {
  char msg[sizeof g_err];
  const int n = std::snprintf(msg, sizeof msg, "%s: ", who);
  va_list ap;
  va_start(ap, what);
  if (n >= 0 && (size_t)n < sizeof msg) std::vsnprintf(msg + n, sizeof msg - n, what, ap);
  va_end(ap);
  return fail(code, msg);
}
// p may be read or written `bytes` (a power of two) at a time; NULL is aligned
static bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

static bool known_mode(int mode) { return mode == NLML_MODE_F32 || mode == NLML_MODE_BF16 || mode == NLML_MODE_F16X2 || mode == NLML_MODE_F16X2S; }
static bool split_f16(int mode) { return mode == NLML_MODE_F16X2 || mode == NLML_MODE_F16X2S; }

extern "C" {

int nlml_abi_version(void) { return NLML_ABI_VERSION; }
const char* nlml_last_error(void) { return g_err; }

int nlml_normalize_ipd(const float* raw, int64_t B, int normalize, float* out, uint8_t* valid, void* stream) {
  if (B < 0 || (B > 0 && (!raw || !out))) return fail(NLML_E_BADARG, "normalize_ipd: null buffer or negative B");
  if (!aligned(raw, 16) || !aligned(out, 16)) return fail(NLML_E_BADARG, "normalize_ipd: raw/out must be 16-byte aligned");
  return launch_normalize_ipd(raw, B, normalize, out, valid, stream);
}

int nlml_normalize_centroid(const float* raw, int64_t B, float* out, uint8_t* valid, double* stats, void* stream) {
  if (B < 0 || (B > 0 && (!raw || !out))) return fail(NLML_E_BADARG, "normalize_centroid: null buffer or negative B");
  if (!aligned(raw, 16) || !aligned(out, 16)) return fail(NLML_E_BADARG, "normalize_centroid: raw/out must be 16-byte aligned");
  if (!aligned(stats, 8)) return fail(NLML_E_BADARG, "normalize_centroid: stats must be 8-byte aligned");
  return launch_normalize_centroid(raw, B, out, valid, stats, stream);
}

// the same operation order (centroid_ref.h) on host buffers: plain C++, no HIP call
int nlml_normalize_centroid_host(const float* h_raw, int64_t B, float* h_out, uint8_t* h_valid, double* h_stats) {
  if (B < 0 || (B > 0 && (!h_raw || !h_out))) return fail(NLML_E_BADARG, "normalize_centroid_host: null buffer or negative B");
  for (int64_t b = 0; b < B; ++b) {
    const int v = cn_face_host(h_raw + b * NLML_F_REFERENCE, h_out + b * NLML_F_REFERENCE, h_stats ? h_stats + 4 * b : nullptr);
    if (h_valid) h_valid[b] = (uint8_t)v;
  }
  return 0;
}

// K6: the checks of include/nlml_hpe.h in their stated order, shared by the device and the host forms.  -> 0 with *rows = the number
// of rows to write (0: nothing to do), or the error.
static int check_rotation_grid(const char* who, bool have_buffers, int64_t I, int ny, int np, int nr, int order, int zy, int zp, int zr,
                               int64_t* rows) {
  const bool empty = I == 0 || ny == 0 || np == 0 || nr == 0;
  if (!empty && !have_buffers) return refuse(NLML_E_BADARG, who, "null buffer");
  if (I < 0 || ny < 0 || np < 0 || nr < 0) return refuse(NLML_E_BADARG, who, "negative extent");
  if (order != NLML_ROT_INTRINSIC && order != NLML_ROT_EXTRINSIC) return refuse(NLML_E_BADARG, who, "unknown order");
  if (zy < -1 || zy >= ny || zp < -1 || zp >= np || zr < -1 || zr >= nr) return refuse(NLML_E_BADARG, who, "zero index outside -1..n-1");
  *rows = 0;
  if (empty) return 0;
  int64_t n = 0;
  if (__builtin_mul_overflow(I, (int64_t)ny, &n) || __builtin_mul_overflow(n, (int64_t)np, &n) || __builtin_mul_overflow(n, (int64_t)nr, &n) ||
      n > INT64_MAX / (NLML_F_REFERENCE * 8))
    return refuse(NLML_E_BADARG, who, "tensor too large for 64-bit byte offsets");
  *rows = n;
  return 0;
}

int nlml_compose_rotation_tensor(const float* base, int64_t I, const double* rot_yaw, int ny, const double* rot_pitch, int np,
                                 const double* rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll, float* out,
                                 double* out64, void* stream) {
  int64_t rows;
  if (const int rc = check_rotation_grid("compose_rotation_tensor", base && rot_yaw && rot_pitch && rot_roll && out, I, ny, np, nr, order,
                                         zero_yaw, zero_pitch, zero_roll, &rows))
    return rc;
  if (rows == 0) return 0;
  if (!aligned(base, 16) || !aligned(out, 16)) return fail(NLML_E_BADARG, "compose_rotation_tensor: base/out must be 16-byte aligned");
  if (!aligned(rot_yaw, 8) || !aligned(rot_pitch, 8) || !aligned(rot_roll, 8) || !aligned(out64, 8))
    return fail(NLML_E_BADARG, "compose_rotation_tensor: the matrices and out64 must be 8-byte aligned");
  return launch_compose_rotation_tensor(base, rows, rot_yaw, ny, rot_pitch, np, rot_roll, nr, order, zero_yaw, zero_pitch, zero_roll, out,
                                        out64, stream);
}

int nlml_compose_rotation_tensor_host(const float* h_base, int64_t I, const double* h_rot_yaw, int ny, const double* h_rot_pitch, int np,
                                      const double* h_rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll,
                                      float* h_out, double* h_out64) {
  int64_t rows;
  if (const int rc = check_rotation_grid("compose_rotation_tensor_host", h_base && h_rot_yaw && h_rot_pitch && h_rot_roll && (h_out || h_out64),
                                         I, ny, np, nr, order, zero_yaw, zero_pitch, zero_roll, &rows))
    return rc;
  if (rows) rt_grid_host(h_base, I, h_rot_yaw, ny, h_rot_pitch, np, h_rot_roll, nr, order, zero_yaw, zero_pitch, zero_roll, h_out, h_out64);
  return 0;
}

int nlml_rotate_landmarks(const float* lm, const double* rot, float* out, double* out64, int64_t B, void* stream) {
  if (B != 0 && (!lm || !rot || (!out && !out64))) return fail(NLML_E_BADARG, "rotate_landmarks: null buffer (lm, rot, and out or out64)");
  if (B < 0) return fail(NLML_E_BADARG, "rotate_landmarks: negative extent");
  if (B == 0) return 0;
  if (B > INT64_MAX / (NLML_F_REFERENCE * 8)) return fail(NLML_E_BADARG, "rotate_landmarks: too many faces for 64-bit byte offsets");
  if (!aligned(lm, 16) || !aligned(out, 16)) return fail(NLML_E_BADARG, "rotate_landmarks: lm/out must be 16-byte aligned");
  if (!aligned(rot, 8) || !aligned(out64, 8)) return fail(NLML_E_BADARG, "rotate_landmarks: rot/out64 must be 8-byte aligned");
  return launch_rotate_landmarks(lm, rot, out, out64, B, stream);
}

int nlml_rotate_landmarks_host(const float* h_lm, const double* h_rot, float* h_out, double* h_out64, int64_t B) {
  if (B != 0 && (!h_lm || !h_rot || (!h_out && !h_out64))) return fail(NLML_E_BADARG, "rotate_landmarks_host: null buffer (lm, rot, and out or out64)");
  if (B < 0) return fail(NLML_E_BADARG, "rotate_landmarks_host: negative extent");
  for (int64_t b = 0; b < B; ++b)
    rt_face_host(h_lm + b * NLML_F_REFERENCE, h_rot + b * 27, h_rot + b * 27 + 9, h_rot + b * 27 + 18,
                 h_out ? h_out + b * NLML_F_REFERENCE : nullptr, h_out64 ? h_out64 + b * NLML_F_REFERENCE : nullptr);
  return 0;
}

size_t nlml_encoder_heads_packed_bytes(int F, int mode) {
  if (F <= 0 || !known_mode(mode)) return 0;
  return blob_bytes_for(F, mode);
}

int nlml_encoder_heads_pack(int F, int mode, const float* const h_enc_w[6], const float* const h_enc_b[6],
                            const float* const h_head_w[3][5], const float* const h_head_b[3][5], void* h_blob,
                            size_t blob_bytes) {
  if (!known_mode(mode)) return fail(NLML_E_BADARG, "pack: unsupported mode");
  if (!h_enc_w || !h_enc_b || !h_head_w || !h_head_b) return fail(NLML_E_BADARG, "pack: null table");
  return pack_blob(F, mode, h_enc_w, h_enc_b, h_head_w, h_head_b, h_blob, blob_bytes);
}

// The blob lives in device memory; its mode is recognised by its size (the sizes of the modes never coincide:
// the latent and head-input stages are padded differently in each).
static int check_blob_args(int64_t B, int F, const void* blob, size_t blob_bytes, const float* out, int* mode) {
  if (B < 0 || F <= 0) return fail(NLML_E_BADARG, "encoder_heads: negative B or bad F");
  if (B > 0 && (!blob || !out)) return fail(NLML_E_BADARG, "encoder_heads: null buffer");
  if (!aligned(blob, 16)) return fail(NLML_E_BADARG, "encoder_heads: blob must be 16-byte aligned");
  if (blob_bytes == blob_bytes_for(F, NLML_MODE_F32)) *mode = NLML_MODE_F32;
  else if (blob_bytes == blob_bytes_for(F, NLML_MODE_BF16)) *mode = NLML_MODE_BF16;
  else if (blob_bytes == blob_bytes_for(F, NLML_MODE_F16X2)) *mode = NLML_MODE_F16X2;
  else if (blob_bytes == blob_bytes_for(F, NLML_MODE_F16X2S)) *mode = NLML_MODE_F16X2S;
  else return fail(NLML_E_BADBLOB, "encoder_heads: blob size does not match F in any mode");
  return 0;
}

// ---- the K2 forward: one core behind the eight entry points --------------------------------------------------------------------
// (crossovers measured with tools/k2_crossover.py and bench.py extra.k2_batch_sweep)
// Split-f16 modes: up to here the layer-per-launch path over 64-face tiles, above it the fused kernel wins.  NLML_MODE_F16X2: 5,120 faces
// 0.140 against 0.159 ms layered.  NLML_MODE_F16X2S: with the eight-wave fused kernel the same crossover (5,120 faces: 0.152 against 0.159 ms
// layered; 4,096: 0.152 against 0.123; round 3's four-wave kernel lost up to 8,192).  The one place the figure is written: hosts ask
// nlml_k2_small_batch_max.
static const int64_t kSmallMax = 4096;
// The trunk + streamed-tail path (encoder_heads_f16x2_tailws.hip) is bit-identical to the fused kernel and measured 1.4-2.2 % faster at 65,536
// faces (0.801 against 0.815 ms, same box, alternating) -- inside the box-to-box spread, for a 64 MB workspace and a
// second big launch -- so the dispatcher does not pick it by itself.  NLML_K2_STREAMED_MIN=<faces> routes batches from that size
// on through it (the explicit _streamed entry points always do).
static int64_t streamed_min() {
  static const int64_t v = [] { const char* e = getenv("NLML_K2_STREAMED_MIN"); return e && e[0] ? (int64_t)atoll(e) : (int64_t)-1; }();
  return v;
}

// The four-tile kernel (encoder_heads_f16x2_w8.hip, encoder_heads_f16x2_w8q_kernel: a workgroup runs the trunk over four tiles and the
// streamed tail once) pays where every compute unit gets a whole workgroup of it: AUTO sends whole rounds of one workgroup per unit
// through it and the rest of the batch through the fused kernel (k2_quad_faces), if the caller's workspace holds the quad part's
// hand-over.  NLML_K2_QUAD_MIN=<faces>: negative switches the path off, otherwise batches from that size on go through it whole.
// NLML_K2_QUAD_CUS=<n> stands in for the device's compute-unit count (tests: a split at a small batch).
static int64_t env_i64(const char* name, int64_t unset) {
  const char* e = getenv(name);
  return e && e[0] ? (int64_t)atoll(e) : unset;
}
static const int64_t kQuadMinUnset = INT64_MIN;
static int64_t quad_min() {
  static const int64_t v = env_i64("NLML_K2_QUAD_MIN", kQuadMinUnset);
  return v;
}
static int device_cus() {   // of the calling thread's current device, asked once per device
  static const int64_t forced = env_i64("NLML_K2_QUAD_CUS", 0);
  if (forced > 0) return (int)forced;
  constexpr int kMaxDev = 64;
  static int cus[kMaxDev];   // 0: not asked yet (a race writes the same value twice)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 0;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = -1;
    cus[dev] = n;
  }
  return cus[dev] > 0 ? cus[dev] : 0;
}

// The part of a strict-fast batch of B faces with 16-byte readable rows that AUTO sends through the four-tile kernel on the current device
static int64_t auto_quad_faces(int64_t B) {
  if (B <= 0) return 0;
  if (B > kSmallMax && streamed_min() >= 0 && B >= streamed_min()) return 0;   // the streamed path was asked for: it wins
  if (quad_min() != kQuadMinUnset) return quad_min() >= 0 && B >= quad_min() ? B : 0;
  return B > kSmallMax ? k2_quad_faces(B, device_cus()) : 0;                   // (the layer-per-launch path's sizes stay its own)
}
// What the streamed and the quad path take: a strict-fast blob and rows that may be read 16 bytes at a time
static bool k2_wide(bool strict_fast, const K2Input& in) { return strict_fast && in.vec4; }
// The same part for a given input and blob: AUTO's rule for the four-tile kernel, whole.  k2_forward and the hosts (nlml_k2_quad_part) ask here.
static int64_t auto_quad_part(bool strict_fast, const K2Input& in, int64_t B) { return k2_wide(strict_fast, in) ? auto_quad_faces(B) : 0; }

// The call forms: the fused kernel of the blob's mode; the split-f16 modes' layer-per-launch path (small batches); the strict-fast
// mode's trunk + streamed tail (encoder_heads_f16x2_w8.hip TRUNK, encoder_heads_f16x2_tailws.hip); the strict-fast mode's four-tile
// kernel over the whole batch; AUTO = the fastest of them for the batch size and the blob's mode, through a caller-provided workspace.
enum K2Form { K2_FUSED, K2_SMALL, K2_STREAMED, K2_QUAD, K2_AUTO };

// What a path other than the fused kernels needs of a call (B > 0), the last of the "K2 argument checks" (include/nlml_hpe.h): the
// workspace's presence and size, its alignment, and for the streamed and the quad path rows readable 16 bytes at a time.
static int check_k2_path(K2Form form, const K2Call& c, int64_t quad_faces) {
  if (form == K2_FUSED) return 0;
  const char* who = form == K2_SMALL ? "small-batch path" : form == K2_STREAMED ? "streamed-tail path" : "quad path";
  // (k2_forward's own arithmetic, k2_quad_faces or the whole batch: held to the launcher's contract here, where every refusal is)
  if (form == K2_QUAD && (quad_faces < 0 || quad_faces > c.B || (quad_faces < c.B && quad_faces % (4 * TILE_FACES))))
    return refuse(NLML_E_BADARG, who, "the quad part is whole workgroups of 256 faces, or the whole batch");
  if (form == K2_QUAD && quad_faces == 0) return 0;   // (no quad part: all of it through the fused kernel, which needs no workspace)
  const size_t need = form == K2_SMALL ? small_workspace_bytes(c.B, c.F) : form == K2_STREAMED ? tailws_workspace_bytes(c.B, c.F)
                                                                                               : quad_workspace_bytes(quad_faces);
  if (!c.ws || c.ws_bytes < need) return refuse(NLML_E_BADARG, who, "workspace too small");
  if (!aligned(c.ws, 16)) return refuse(NLML_E_BADARG, who, "workspace must be 16-byte aligned");
  if (form != K2_SMALL && !c.in.vec4) return refuse(NLML_E_BADARG, who, "x must be 16-byte aligned with F and ldx multiples of 4");
  return 0;
}

// landmarks: the input is raw [B,468,3] (x, ldx unused), else the feature rows x / ldx (raw null).  workspace / ws_bytes are read by the
// forms that need one.  The checks and their order: include/nlml_hpe.h, "K2 argument checks".
static int k2_forward(K2Form form, bool landmarks, const float* x, int64_t ldx, const float* raw, int normalize, int64_t B, int F,
                      const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes,
                      void* stream) {
  const char* no_input = nullptr;
  if (B > 0 && landmarks && !raw) no_input = "landmarks_to_pose: null raw";
  if (B > 0 && !landmarks && (!x || ldx < F)) no_input = "encoder_heads: null x or ldx < F";
  // nlml_landmarks_to_pose_ws alone looks at raw before the blob; hosts may match on which of two errors they get
  if (no_input && form == K2_AUTO && landmarks) return fail(NLML_E_BADARG, no_input);
  int mode = 0;
  if (int rc = check_blob_args(B, F, blob, blob_bytes, out, &mode)) return rc;
  if (form == K2_SMALL && !split_f16(mode)) return fail(NLML_E_BADARG, "small-batch path: NLML_MODE_F16X2 / NLML_MODE_F16X2S blob only");
  if (form == K2_STREAMED && mode != NLML_MODE_F16X2S) return fail(NLML_E_BADARG, "streamed-tail path: NLML_MODE_F16X2S blob only");
  if (form == K2_QUAD && mode != NLML_MODE_F16X2S) return fail(NLML_E_BADARG, "quad path: NLML_MODE_F16X2S blob only");
  if (no_input) return fail(NLML_E_BADARG, no_input);
  if (B == 0) return 0;
  const K2Call c{k2_input(x, ldx, raw, normalize, F), B, F, blob, out, latent, valid, workspace, ws_bytes};
  const int split = mode == NLML_MODE_F16X2S;
  int64_t quad_faces = B;   // K2_QUAD: the whole batch
  if (form == K2_AUTO) {
    quad_faces = auto_quad_part(split, c.in, B);
    // whole rounds only if the workspace takes them -- never a failure the fused kernel would not have; asked for by the environment, always
    const bool fits = workspace && ws_bytes >= quad_workspace_bytes(quad_faces) && aligned(workspace, 16);
    if (quad_faces > 0 && (fits || quad_min() != kQuadMinUnset)) form = K2_QUAD;
    else if (split_f16(mode) && B <= kSmallMax) form = K2_SMALL;
    else if (k2_wide(split, c.in) && streamed_min() >= 0 && B >= streamed_min()) form = K2_STREAMED;
    else form = K2_FUSED;
  }
  if (int rc = check_k2_path(form, c, quad_faces)) return rc;
  int rc;
  if (form == K2_SMALL) rc = launch_encoder_heads_f16x2_small(c, split, stream);
  else if (form == K2_STREAMED) rc = launch_encoder_heads_f16x2_tailws(c, stream);
  else if (form == K2_QUAD) rc = launch_encoder_heads_f16x2_w8_mixed(c, quad_faces, stream);
  else if (mode == NLML_MODE_BF16) rc = launch_encoder_heads_bf16(c, stream);
  else if (mode == NLML_MODE_F16X2) rc = launch_encoder_heads_f16x2(c, stream);
  else if (split) rc = launch_encoder_heads_f16x2_w8(c, stream);
  else rc = launch_encoder_heads_f32(c, nullptr, nullptr, stream);
  // a strict-fast forward is its split-f16 launch(es) followed by the f32 re-evaluation launch over all B, whichever form ran
  return rc || !split ? rc : launch_strict_reeval(c, stream);
}

int nlml_encoder_heads_fwd(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                           float* out, float* latent, uint8_t* valid, void* stream) {
  return k2_forward(K2_FUSED, false, x, ldx, nullptr, 0, B, F, blob, blob_bytes, out, latent, valid, nullptr, 0, stream);
}

int nlml_encoder_heads_fwd_debug(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                                 float* out, float* latent, float* pre_tanh, unsigned long long* stamps, void* stream) {
  int mode = 0;
  if (int rc = check_blob_args(B, F, blob, blob_bytes, out, &mode)) return rc;
  if (mode != NLML_MODE_F32) return fail(NLML_E_BADARG, "debug build: f32 blob only");
  if (B > 0 && (!x || ldx < F)) return fail(NLML_E_BADARG, "encoder_heads: null x or ldx < F");
  if (B == 0) return 0;
  const K2Call c{k2_input(x, ldx, nullptr, 0, F), B, F, blob, out, latent, nullptr, nullptr, 0};
  if ((pre_tanh || stamps) && !c.in.vec4) return fail(NLML_E_BADARG, "debug build: features input, F % 4 == 0 only");
  return launch_encoder_heads_f32(c, pre_tanh, stamps, stream);
}

int nlml_landmarks_to_pose(const float* raw, int64_t B, int normalize, const void* blob, size_t blob_bytes,
                           float* out, float* latent, uint8_t* valid, void* stream) {
  return k2_forward(K2_FUSED, true, nullptr, 0, raw, normalize, B, NLML_F_REFERENCE, blob, blob_bytes, out, latent, valid, nullptr, 0, stream);
}

size_t nlml_encoder_heads_small_workspace_bytes(int64_t B, int F) { return small_workspace_bytes(B, F); }

int nlml_encoder_heads_fwd_small(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                                 float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_SMALL, false, x, ldx, nullptr, 0, B, F, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_landmarks_to_pose_small(const float* raw, int64_t B, int normalize, const void* blob, size_t blob_bytes,
                                 float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_SMALL, true, nullptr, 0, raw, normalize, B, NLML_F_REFERENCE, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_encoder_heads_fwd_streamed(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                                    float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_STREAMED, false, x, ldx, nullptr, 0, B, F, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_landmarks_to_pose_streamed(const float* raw, int64_t B, int normalize, const void* blob, size_t blob_bytes,
                                    float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_STREAMED, true, nullptr, 0, raw, normalize, B, NLML_F_REFERENCE, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_encoder_heads_fwd_quad(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                                float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_QUAD, false, x, ldx, nullptr, 0, B, F, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_landmarks_to_pose_quad(const float* raw, int64_t B, int normalize, const void* blob, size_t blob_bytes,
                                float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_QUAD, true, nullptr, 0, raw, normalize, B, NLML_F_REFERENCE, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_k2_quad_split(int64_t B, int cus, int64_t* quad_faces) {
  if (!quad_faces) return fail(NLML_E_BADARG, "k2_quad_split: null quad_faces");
  *quad_faces = 0;
  if (B < 0 || cus <= 0) return fail(NLML_E_BADARG, "k2_quad_split: negative B or cus <= 0");
  *quad_faces = k2_quad_faces(B, cus);
  return 0;
}

// nlml_k2_quad_part / nlml_k2_quad_faces (who: the one that was called)
static int k2_quad_part(const char* who, const float* rows, int64_t ld, int64_t B, int F, size_t blob_bytes, int64_t* quad_faces,
                        size_t* ws_bytes) {
  if (quad_faces) *quad_faces = 0;
  if (ws_bytes) *ws_bytes = 0;
  if (B < 0 || F <= 0 || !quad_faces) return refuse(NLML_E_BADARG, who, "negative B, F <= 0 or null quad_faces");
  *quad_faces = auto_quad_part(blob_bytes == blob_bytes_for(F, NLML_MODE_F16X2S), k2_input(rows, ld, nullptr, 0, F), B);
  if (ws_bytes) *ws_bytes = quad_workspace_bytes(*quad_faces);
  return 0;
}

int nlml_k2_quad_part(const float* rows, int64_t ld, int64_t B, int F, size_t blob_bytes, int64_t* quad_faces, size_t* ws_bytes) {
  return k2_quad_part("k2_quad_part", rows, ld, B, F, blob_bytes, quad_faces, ws_bytes);
}

// the same rule for aligned rows of the reference width and a strict-fast blob
int nlml_k2_quad_faces(int64_t B, int64_t* quad_faces, size_t* ws_bytes) {
  return k2_quad_part("k2_quad_faces", nullptr, NLML_F_REFERENCE, B, NLML_F_REFERENCE, blob_bytes_for(NLML_F_REFERENCE, NLML_MODE_F16X2S), quad_faces,
                      ws_bytes);
}

int64_t nlml_k2_small_batch_max(int mode) { return split_f16(mode) ? kSmallMax : 0; }

size_t nlml_encoder_heads_workspace_bytes(int64_t B, int F) {
  const size_t a = small_workspace_bytes(B, F), b = tailws_workspace_bytes(B, F);
  return a > b ? a : b;
}

int nlml_encoder_heads_fwd_ws(const float* x, int64_t ldx, int64_t B, int F, const void* blob, size_t blob_bytes,
                              float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_AUTO, false, x, ldx, nullptr, 0, B, F, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_landmarks_to_pose_ws(const float* raw, int64_t B, int normalize, const void* blob, size_t blob_bytes,
                              float* out, float* latent, uint8_t* valid, void* workspace, size_t ws_bytes, void* stream) {
  return k2_forward(K2_AUTO, true, nullptr, 0, raw, normalize, B, NLML_F_REFERENCE, blob, blob_bytes, out, latent, valid, workspace, ws_bytes, stream);
}

int nlml_video_post_ex(const float* pose_rad, const float* raw, const uint8_t* valid, int64_t S, double frame_w,
                       double frame_h, double alpha, double max_jump, double size, double* state, double* smoothed,
                       double* centre, double* endpoints, uint8_t* updated, void* stream) {
  if (S < 0) return fail(NLML_E_BADARG, "video_post: negative S");
  if (S > 0 && (!pose_rad || !raw || !state || !smoothed || !centre || !endpoints))
    return fail(NLML_E_BADARG, "video_post: null buffer");
  return launch_video_post(pose_rad, raw, valid, S, frame_w, frame_h, alpha, max_jump, size, state, smoothed, centre,
                           endpoints, updated, stream);
}

int nlml_video_post(const float* pose_rad, const float* raw, const uint8_t* valid, int64_t S, double frame_w,
                    double frame_h, double alpha, double max_jump, double size, double* state, double* smoothed,
                    double* centre, double* endpoints, void* stream) {
  return nlml_video_post_ex(pose_rad, raw, valid, S, frame_w, frame_h, alpha, max_jump, size, state, smoothed, centre, endpoints,
                            nullptr, stream);
}

int nlml_cosine_table(const float* angles_rad, int64_t n, const double* cos_params, int R, double* out, void* stream) {
  if (n < 0 || R < 0) return fail(NLML_E_BADARG, "cosine_table: negative size");
  if (n > 0 && R > 0 && (!angles_rad || !cos_params || !out)) return fail(NLML_E_BADARG, "cosine_table: null buffer");
  return launch_cosine_table(angles_rad, n, cos_params, R, out, stream);
}

int nlml_mode5_product(const float* core, const float* U_feat, int Q, int R5, int M, float* W, void* stream) {
  if (Q < 0 || R5 < 0 || M < 0) return fail(NLML_E_BADARG, "mode5_product: negative size");
  if (Q > 0 && M > 0 && (!W || (R5 > 0 && (!core || !U_feat)))) return fail(NLML_E_BADARG, "mode5_product: null buffer");
  return launch_mode5_product(core, U_feat, Q, R5, M, W, stream);
}

// ---- K7: the Tucker decomposition's primitives (tucker_decompose.hip) ----------------------------------
// I x K within 64-bit byte offsets of f64 partials (I <= 4096 keeps every product below 2^63)
static bool k7_matrix_ok(int64_t I, int64_t K) { return I >= 1 && I <= NLML_GRAM_I_MAX && K >= 1 && K <= INT64_MAX / (8 * NLML_GRAM_I_MAX); }
static bool k7_bins_ok(int ny, int np, int nr) {
  return ny >= 1 && np >= 1 && nr >= 1 && ny <= NLML_POSE_BINS_MAX && np <= NLML_POSE_BINS_MAX && nr <= NLML_POSE_BINS_MAX;
}
// I x (ny np nr) x M elements within 64-bit byte offsets
static bool k7_tensor_ok(int64_t I, int ny, int np, int nr, int64_t M) {
  int64_t n = 0;
  return I >= 1 && M >= 1 && !__builtin_mul_overflow(I, (int64_t)ny * np * nr, &n) && !__builtin_mul_overflow(n, M, &n) && n <= INT64_MAX / 8;
}

size_t nlml_mode_gram_workspace_bytes(int64_t I, int64_t K) { return k7_matrix_ok(I, K) ? mode_gram_workspace_bytes(I, K) : 0; }

int nlml_mode_gram(const float* A, int64_t I, int64_t K, double* G, void* workspace, size_t workspace_bytes, void* stream) {
  return nlml_mode_gram_ex(A, 0, I, K, G, workspace, workspace_bytes, stream);
}

int nlml_mode_gram_ex(const void* A, int a_f64, int64_t I, int64_t K, double* G, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "mode_gram";
  if (!A || !G || !workspace) return refuse(NLML_E_BADARG, who, "null buffer (A, G, workspace)");
  if (I < 1 || I > NLML_GRAM_I_MAX) return refuse(NLML_E_BADARG, who, "I outside 1..NLML_GRAM_I_MAX (4096)");
  if (!k7_matrix_ok(I, K)) return refuse(NLML_E_BADARG, who, "K < 1 or too large for 64-bit byte offsets");
  if (!aligned(A, a_f64 ? 8 : 4) || !aligned(G, 8) || !aligned(workspace, 8))
    return refuse(NLML_E_BADARG, who, "A must be aligned to its element (4 bytes f32, 8 bytes f64), G and the workspace 8-byte aligned");
  if (workspace_bytes < mode_gram_workspace_bytes(I, K)) return refuse(NLML_E_BADARG, who, "workspace too small (nlml_mode_gram_workspace_bytes)");
  return launch_mode_gram(A, a_f64 != 0, I, K, G, workspace, stream);
}

static bool k7_pose_grams_ok(int64_t I, int ny, int np, int nr, int64_t M) {
  return k7_bins_ok(ny, np, nr) && ny * np * nr <= NLML_POSE_GRAMS_MAX_CELLS && k7_tensor_ok(I, ny, np, nr, M);
}
size_t nlml_pose_grams_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M) {
  return k7_pose_grams_ok(I, ny, np, nr, M) ? pose_grams_workspace_bytes(I, ny, np, nr, M) : 0;
}

int nlml_pose_grams(const float* X, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr, void* workspace,
                    size_t workspace_bytes, void* stream) {
  return nlml_pose_grams_ex(X, 0, I, ny, np, nr, M, Gy, Gp, Gr, workspace, workspace_bytes, stream);
}

int nlml_pose_grams_ex(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "pose_grams";
  if (!X || !workspace || (!Gy && !Gp && !Gr)) return refuse(NLML_E_BADARG, who, "null buffer (X, workspace, and at least one of Gy, Gp, Gr)");
  if (I < 1 || M < 1) return refuse(NLML_E_BADARG, who, "I < 1 or M < 1");
  if (!k7_bins_ok(ny, np, nr)) return refuse(NLML_E_BADARG, who, "ny, np, nr outside 1..NLML_POSE_BINS_MAX (32)");
  if (ny * np * nr > NLML_POSE_GRAMS_MAX_CELLS) return refuse(NLML_E_BADARG, who, "ny np nr beyond NLML_POSE_GRAMS_MAX_CELLS (768): the slab does not fit in LDS");
  if (!k7_tensor_ok(I, ny, np, nr, M)) return refuse(NLML_E_BADARG, who, "tensor too large for 64-bit byte offsets");
  if (!aligned(X, x_f64 ? 8 : 4) || !aligned(Gy, 8) || !aligned(Gp, 8) || !aligned(Gr, 8) || !aligned(workspace, 8))
    return refuse(NLML_E_BADARG, who, "X must be aligned to its element (4 bytes f32, 8 bytes f64), the Grams and the workspace 8-byte aligned");
  if (workspace_bytes < pose_grams_workspace_bytes(I, ny, np, nr, M)) return refuse(NLML_E_BADARG, who, "workspace too small (nlml_pose_grams_workspace_bytes)");
  return launch_pose_grams(X, x_f64 != 0, I, ny, np, nr, M, Gy, Gp, Gr, workspace, stream);
}

int nlml_project_identity(const float* A, int64_t I, int64_t K, const double* U, int R, float* out, void* stream) {
  return nlml_project_identity_ex(A, I, K, U, R, out, 0, stream);
}

int nlml_project_identity_ex(const float* A, int64_t I, int64_t K, const double* U, int R, void* out, int out_f64, void* stream) {
  const char* who = "project_identity";
  if (!A || !U || !out) return refuse(NLML_E_BADARG, who, "null buffer (A, U, out)");
  if (I < 1 || K < 1) return refuse(NLML_E_BADARG, who, "I < 1 or K < 1");
  if (R < NLML_TUCKER_RANK_MIN || R > NLML_TUCKER_RANK_MAX) return refuse(NLML_E_BADARG, who, "R outside 1..NLML_TUCKER_RANK_MAX (16)");
  int64_t n = 0;
  if (__builtin_mul_overflow(I, K, &n) || n > INT64_MAX / 8) return refuse(NLML_E_BADARG, who, "A too large for 64-bit byte offsets");
  if (!aligned(A, 4) || !aligned(out, out_f64 ? 8 : 4) || !aligned(U, 8))
    return refuse(NLML_E_BADARG, who, "A and out must be aligned to their element (4 bytes f32, 8 bytes f64), U 8-byte aligned");
  return launch_project_identity(A, I, K, U, R, out, out_f64 != 0, stream);
}

int nlml_project_pose(const float* X, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up, int rp,
                      const double* Ur, int rr, float* out, void* stream) {
  return nlml_project_pose_ex(X, 0, I, ny, np, nr, M, Uy, ry, Up, rp, Ur, rr, out, 0, stream);
}

int nlml_project_pose_ex(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up,
                         int rp, const double* Ur, int rr, void* out, int out_f64, void* stream) {
  const char* who = "project_pose";
  if (!X || !out) return refuse(NLML_E_BADARG, who, "null buffer (X, out)");
  if (I < 1 || M < 1) return refuse(NLML_E_BADARG, who, "I < 1 or M < 1");
  if (!k7_bins_ok(ny, np, nr)) return refuse(NLML_E_BADARG, who, "ny, np, nr outside 1..NLML_POSE_BINS_MAX (32)");
  if ((Uy && (ry < 1 || ry > NLML_POSE_RANK_MAX)) || (Up && (rp < 1 || rp > NLML_POSE_RANK_MAX)) || (Ur && (rr < 1 || rr > NLML_POSE_RANK_MAX)))
    return refuse(NLML_E_BADARG, who, "rank of a given factor outside 1..NLML_POSE_RANK_MAX (3)");
  if (!k7_tensor_ok(I, ny, np, nr, M)) return refuse(NLML_E_BADARG, who, "tensor too large for 64-bit byte offsets");
  if (!aligned(X, x_f64 ? 8 : 4) || !aligned(out, out_f64 ? 8 : 4) || !aligned(Uy, 8) || !aligned(Up, 8) || !aligned(Ur, 8))
    return refuse(NLML_E_BADARG, who, "X and out must be aligned to their element (4 bytes f32, 8 bytes f64), the factors 8-byte aligned");
  return launch_project_pose(X, x_f64 != 0, I, ny, np, nr, M, Uy, ry, Up, rp, Ur, rr, out, out_f64 != 0, stream);
}

// ---- K11: expand and compare in one pass (tucker_residual.hip) -----------------------------------------
static bool k11_shape_ok(int64_t I, int ny, int np, int nr, int64_t M) {
  return k7_bins_ok(ny, np, nr) && k7_tensor_ok(I, ny, np, nr, M) && M <= INT64_MAX / (8 * 27 * NLML_TUCKER_RANK_MAX);
}
size_t nlml_tucker_residual_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M) {
  return k11_shape_ok(I, ny, np, nr, M) ? tucker_residual_workspace_bytes(I, M) : 0;
}

// the checks of include/nlml_hpe.h in their stated order, shared by the device and the host forms
static int check_tucker_residual(const char* who, const TrArgs& a, int ry, int rp, int rr, const double* sums, const double* res_id,
                                 const void* workspace, size_t workspace_bytes) {
  if (!a.W || !a.Uid || !a.Uy || !a.Up || !a.Ur || (!a.X && !a.xhat) || (a.X && (!sums || !workspace)))
    return refuse(NLML_E_BADARG, who, "null buffer (W, the four factors, X or xhat; with X: sums and the workspace)");
  if (a.I < 1 || a.M < 1) return refuse(NLML_E_BADARG, who, "I < 1 or M < 1");
  if (!k7_bins_ok(a.ny, a.np, a.nr)) return refuse(NLML_E_BADARG, who, "ny, np, nr outside 1..NLML_POSE_BINS_MAX (32)");
  if (a.R < NLML_TUCKER_RANK_MIN || a.R > NLML_TUCKER_RANK_MAX) return refuse(NLML_E_BADARG, who, "R outside 1..NLML_TUCKER_RANK_MAX (16)");
  if (ry < 1 || ry > NLML_POSE_RANK_MAX || rp < 1 || rp > NLML_POSE_RANK_MAX || rr < 1 || rr > NLML_POSE_RANK_MAX)
    return refuse(NLML_E_BADARG, who, "ry, rp, rr outside 1..NLML_POSE_RANK_MAX (3)");
  if (!k11_shape_ok(a.I, a.ny, a.np, a.nr, a.M)) return refuse(NLML_E_BADARG, who, "tensor too large for 64-bit byte offsets");
  if (!aligned(a.X, 4) || !aligned(a.W, 4) || !aligned(a.xhat, 4) || !aligned(a.Uid, 8) || !aligned(a.Uy, 8) || !aligned(a.Up, 8) ||
      !aligned(a.Ur, 8) || !aligned(sums, 8) || !aligned(res_id, 8) || !aligned(workspace, 8))
    return refuse(NLML_E_BADARG, who, "X, W and xhat must be 4-byte aligned, the factors, sums, res_id and the workspace 8-byte aligned");
  if (a.X && workspace_bytes < tucker_residual_workspace_bytes(a.I, a.M))
    return refuse(NLML_E_BADARG, who, "workspace too small (nlml_tucker_residual_workspace_bytes)");
  return 0;
}

int nlml_tucker_residual(const float* X, const float* W, const double* U_id, const double* Uy, const double* Up, const double* Ur,
                         int64_t I, int ny, int np, int nr, int64_t M, int R, int ry, int rp, int rr, double* sums, double* res_id,
                         float* xhat, void* workspace, size_t workspace_bytes, void* stream) {
  const TrArgs a{X, W, U_id, Uy, Up, Ur, xhat, I, M, R, ny, np, nr};
  if (const int rc = check_tucker_residual("tucker_residual", a, ry, rp, rr, sums, res_id, workspace, workspace_bytes)) return rc;
  return launch_tucker_residual(a, ry, rp, rr, sums, res_id, workspace, stream);
}

// the same operation order (tucker_residual_ref.h) on host buffers: plain C++, no HIP call
int nlml_tucker_residual_host(const float* h_X, const float* h_W, const double* h_U_id, const double* h_Uy, const double* h_Up,
                              const double* h_Ur, int64_t I, int ny, int np, int nr, int64_t M, int R, int ry, int rp, int rr,
                              double* h_sums, double* h_res_id, float* h_xhat, void* h_workspace, size_t workspace_bytes) {
  const TrArgs a{h_X, h_W, h_U_id, h_Uy, h_Up, h_Ur, h_xhat, I, M, R, ny, np, nr};
  if (const int rc = check_tucker_residual("tucker_residual_host", a, ry, rp, rr, h_sums, h_res_id, h_workspace, workspace_bytes)) return rc;
  tr_host(a, ry, rp, rr, static_cast<double*>(h_workspace), h_sums, h_res_id);
  return 0;
}

// ---- K5 evaluation ---------------------------------------------------------------------------------
static bool eval_k_ok(int K) { return K >= 0 && K <= NLML_POSE_EVAL_MAX_INTERVALS; }
static int64_t eval_records(int64_t B) { return (B + NLML_POSE_EVAL_FACES_PER_RECORD - 1) / NLML_POSE_EVAL_FACES_PER_RECORD; }

size_t nlml_pose_eval_record_len(int n_intervals) { return eval_k_ok(n_intervals) ? (size_t)(12 + 2 * n_intervals) : 0; }
size_t nlml_pose_eval_result_len(int n_intervals) { return eval_k_ok(n_intervals) ? (size_t)(14 + 2 * n_intervals) : 0; }
size_t nlml_pose_eval_workspace_bytes(int64_t B, int n_intervals) {
  if (B < 0 || !eval_k_ok(n_intervals)) return 0;
  return (size_t)eval_records(B) * nlml_pose_eval_record_len(n_intervals) * sizeof(double);
}

int nlml_pose_eval(const float* pose_rad, const double* pred_deg, const uint8_t* valid, const double* gt_deg, int64_t B,
                   const double* h_lo, const double* h_hi, int decimals, const double* h_intervals, const int32_t* h_axes,
                   int n_intervals, void* workspace, size_t workspace_bytes, double* record_out, double* result_out,
                   double* pred_out, uint8_t* keep_out, void* stream) {
  if (B < 0) return fail(NLML_E_BADARG, "pose_eval: negative B");
  // an empty tensor's data pointer may be NULL: with B == 0 "neither" is accepted
  if ((pose_rad && pred_deg) || (B > 0 && !pose_rad && !pred_deg))
    return fail(NLML_E_BADARG, "pose_eval: give exactly one of pose_rad and pred_deg");
  if (B > 0 && !gt_deg) return fail(NLML_E_BADARG, "pose_eval: null gt_deg");
  if (!h_lo || !h_hi || !result_out) return fail(NLML_E_BADARG, "pose_eval: null lo / hi / result_out");
  if (!eval_k_ok(n_intervals)) return fail(NLML_E_BADARG, "pose_eval: number of intervals outside [0, NLML_POSE_EVAL_MAX_INTERVALS]");
  if (n_intervals > 0 && (!h_intervals || !h_axes)) return fail(NLML_E_BADARG, "pose_eval: null intervals / axes");
  if (decimals > 15) return fail(NLML_E_BADARG, "pose_eval: decimals > 15");
  const size_t need = nlml_pose_eval_workspace_bytes(B, n_intervals);
  if (workspace_bytes < need || (need > 0 && !workspace)) return fail(NLML_E_BADARG, "pose_eval: workspace too small");
  if (!aligned(pred_deg, 8) || !aligned(gt_deg, 8) || !aligned(workspace, 8) || !aligned(record_out, 8) || !aligned(result_out, 8) ||
      !aligned(pred_out, 8) || !aligned(pose_rad, 4))
    return fail(NLML_E_BADARG, "pose_eval: f64 buffers must be 8-byte aligned, pose_rad 4-byte aligned");
  PoseEvalArgs a{};
  for (int i = 0; i < 3; ++i) { a.lo[i] = h_lo[i]; a.hi[i] = h_hi[i]; }
  for (int k = 0; k < n_intervals; ++k) {
    if (h_axes[k] < 0 || h_axes[k] > 2) return fail(NLML_E_BADARG, "pose_eval: interval axis outside {0, 1, 2}");
    a.axes[k] = h_axes[k];
    a.ivl[k][0] = h_intervals[2 * k];
    a.ivl[k][1] = h_intervals[2 * k + 1];
  }
  a.scale = 1.0;
  for (int i = 0; i < decimals; ++i) a.scale *= 10.0;   // exact: every 10^d, d <= 15, is an integer below 2^53
  a.K = n_intervals;
  a.decimals = decimals;
  return launch_pose_eval(pose_rad, pred_deg, valid, gt_deg, B, a, static_cast<double*>(workspace), record_out, result_out, pred_out,
                          keep_out, stream);
}

int nlml_pose_eval_merge(const double* records, int64_t n, int n_intervals, double* record_out, double* result_out, void* stream) {
  if (n < 0) return fail(NLML_E_BADARG, "pose_eval_merge: negative record count");
  if (!eval_k_ok(n_intervals)) return fail(NLML_E_BADARG, "pose_eval_merge: number of intervals outside [0, NLML_POSE_EVAL_MAX_INTERVALS]");
  if ((n > 0 && !records) || !result_out) return fail(NLML_E_BADARG, "pose_eval_merge: null records / result_out");
  if (!aligned(records, 8) || !aligned(record_out, 8) || !aligned(result_out, 8))
    return fail(NLML_E_BADARG, "pose_eval_merge: buffers must be 8-byte aligned");
  return launch_pose_eval_merge(records, n, n_intervals, record_out, result_out, stream);
}

// ---- the TD path (K3 objective, device Powell, K3g gradient): one argument check, one core per operation -----------------------
static_assert(PW_NMAX == 3 + NLML_TUCKER_RANK_MAX && PW_N == 3 + 5, "powell.h's state sizes follow the ranks");
static bool rank_ok(int r_id) { return r_id >= NLML_TUCKER_RANK_MIN && r_id <= NLML_TUCKER_RANK_MAX; }
static int bad_rank(const char* who, int r_id) {
  return refuse(NLML_E_SHAPE, who, "identity rank %d outside [%d, %d]", r_id, NLML_TUCKER_RANK_MIN, NLML_TUCKER_RANK_MAX);
}

// The checks of every TD entry point, in the order include/nlml_hpe.h promises ("TD argument checks": hosts may match on which of two
// errors they get).  who: the entry point family that was called.  An entry point without a rank passes the shipped artefacts' 5, one
// without an order the reference order -- what they run.  null_buffer: one of the operation's required buffers is NULL.  N == 0 with
// rank and order in range needs nothing else: the launchers return at once.
static int check_td_args(const char* who, int r_id, int order, int64_t N, int64_t ldx, bool null_buffer, const float* Wm, const float* x) {
  if (!rank_ok(r_id)) return bad_rank(who, r_id);
  if (order != NLML_TD_ORDER_FAST && order != NLML_TD_ORDER_REFERENCE) return refuse(NLML_E_BADARG, who, "unknown order");
  if (N < 0) return refuse(NLML_E_BADARG, who, "negative N");
  if (N == 0) return 0;
  if (null_buffer) return refuse(NLML_E_BADARG, who, "null buffer");
  if (ldx < NLML_F_REFERENCE) return refuse(NLML_E_BADARG, who, "ldx < 1404");
  // the matrix-core order reads Wm and the x rows with 16-byte vector loads (tucker_common.h load11 / tucker_few)
  if (order == NLML_TD_ORDER_FAST && (!aligned(Wm, 16) || !aligned(x, 16) || ldx % 4 != 0))
    return refuse(NLML_E_BADARG, who, "NLML_TD_ORDER_FAST needs Wm and x 16-byte aligned and ldx %% 4 == 0");
  return 0;
}

static int td_objective(const char* who, const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                        const double* cos_params, int64_t N, double* err, double* x_hat, int r_id, int order, void* stream) {
  if (int rc = check_td_args(who, r_id, order, N, ldx, !Wm || !x || !params || !cos_params || !err, Wm, x)) return rc;
  return launch_tucker_objective(Wm, x, ldx, x_index, params, cos_params, N, err, x_hat, r_id, order, stream);
}

int nlml_tucker_objective(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                          const double* cos_params, int64_t N, double* err, double* x_hat, void* stream) {
  return td_objective("tucker_objective", Wm, x, ldx, x_index, params, cos_params, N, err, x_hat, 5, NLML_TD_ORDER_REFERENCE, stream);
}

int nlml_tucker_objective_ex(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                             const double* cos_params, int64_t N, double* err, double* x_hat, int order, void* stream) {
  return td_objective("tucker_objective", Wm, x, ldx, x_index, params, cos_params, N, err, x_hat, 5, order, stream);
}

int nlml_tucker_objective_r(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                            const double* cos_params, int64_t N, double* err, double* x_hat, int r_id, int order, void* stream) {
  return td_objective("tucker_objective_r", Wm, x, ldx, x_index, params, cos_params, N, err, x_hat, r_id, order, stream);
}

static int td_powell(const char* who, const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                     double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int r_id, int order, void* stream) {
  if (int rc = check_td_args(who, r_id, order, N, ldx, !Wm || !x || !cos_params || !result, Wm, x)) return rc;
  return launch_tucker_powell(Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, r_id, order, stream);
}

int nlml_tucker_powell(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                       double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, void* stream) {
  return td_powell("tucker_powell", Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, 5, NLML_TD_ORDER_REFERENCE, stream);
}

int nlml_tucker_powell_ex(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                          double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int order, void* stream) {
  return td_powell("tucker_powell", Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, 5, order, stream);
}

int nlml_tucker_powell_r(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                         double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int r_id, int order,
                         void* stream) {
  return td_powell("tucker_powell_r", Wm, x, ldx, cos_params, N, x0, result, fval, nfev, nit, status, r_id, order, stream);
}

// K3g: objective value + analytic gradient, reference order
size_t nlml_tucker_gradient_workspace_bytes(int64_t N, int r_id) { return rank_ok(r_id) ? tucker_gradient_workspace_bytes(N) : 0; }

int nlml_tucker_gradient_r(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                           const double* cos_params, int64_t N, double* err, double* grad, int r_id, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (int rc = check_td_args("tucker_gradient_r", r_id, NLML_TD_ORDER_REFERENCE, N, ldx, !Wm || !x || !params || !cos_params || !grad, Wm, x))
    return rc;
  const size_t need = tucker_gradient_workspace_bytes(N);
  if (workspace_bytes < need || (need > 0 && !workspace)) return fail(NLML_E_BADARG, "tucker_gradient_r: workspace too small");
  if (!aligned(workspace, 8) || !aligned(err, 8) || !aligned(grad, 8) || !aligned(params, 8))
    return fail(NLML_E_BADARG, "tucker_gradient_r: f64 buffers and the workspace must be 8-byte aligned");
  return launch_tucker_gradient(Wm, x, ldx, x_index, params, cos_params, N, err, grad, r_id, workspace, stream);
}

// the same operation order (tucker_grad_ref.h) on host buffers: plain C++, no HIP call
int nlml_tucker_gradient_host(const float* h_Wm, const float* h_x, int64_t ldx, const int32_t* h_x_index, const double* h_params,
                              const double* h_cos_params, int64_t N, double* h_err, double* h_grad, int r_id, float* h_v) {
  if (int rc = check_td_args("tucker_gradient_host", r_id, NLML_TD_ORDER_REFERENCE, N, ldx,
                             !h_Wm || !h_x || !h_params || !h_cos_params || !h_grad, h_Wm, h_x))
    return rc;
  for (int64_t n = 0; n < N; ++n)
    tg_gradient_host(h_Wm, h_x + (h_x_index ? (int64_t)h_x_index[n] : n) * ldx, h_params + n * (3 + r_id), h_cos_params, r_id,
                     h_err ? h_err + n : nullptr, h_grad + n * (3 + r_id), h_v ? h_v + n * NLML_F_REFERENCE : nullptr);
  return 0;
}

// ---- K8: the cosine fit of the pose factors (cosine_fit_ref.h, cosine_fit.hip) -----------------------------------------------
static_assert(CF_ROWS_MAX == NLML_COSINE_FIT_ROWS_MAX, "one row per lane");
// The checks of include/nlml_hpe.h ("K8") in their stated order; -> 0 with *run = whether there is anything to do.
static int check_cosine_fit(const char* who, bool null_buffer, int64_t C, int64_t ld, const int32_t* h_n, bool* run) {
  *run = false;
  if (C != 0 && null_buffer) return refuse(NLML_E_BADARG, who, "null buffer");
  if (C < 0) return refuse(NLML_E_BADARG, who, "negative C");
  if (C == 0) return 0;
  for (int64_t f = 0; f < C; ++f)
    if (h_n[f] < 1 || h_n[f] > NLML_COSINE_FIT_ROWS_MAX)
      return refuse(NLML_E_BADARG, who, "n[%lld] = %d outside [1, %d]", (long long)f, (int)h_n[f], NLML_COSINE_FIT_ROWS_MAX);
  for (int64_t f = 0; f < C; ++f)
    if (ld < h_n[f]) return refuse(NLML_E_BADARG, who, "ld = %lld < n[%lld] = %d", (long long)ld, (long long)f, (int)h_n[f]);
  if (C > (int64_t)INT32_MAX || ld > INT64_MAX / 8 / C) return refuse(NLML_E_BADARG, who, "batch too large for 64-bit byte offsets");
  *run = true;
  return 0;
}
static int check_cosine_objective(const char* who, bool null_buffer, int n, int64_t N, bool* run) {
  *run = false;
  if (N != 0 && null_buffer) return refuse(NLML_E_BADARG, who, "null buffer");
  if (N < 0) return refuse(NLML_E_BADARG, who, "negative N");
  if (n < 1 || n > NLML_COSINE_FIT_ROWS_MAX) return refuse(NLML_E_BADARG, who, "n = %d outside [1, %d]", n, NLML_COSINE_FIT_ROWS_MAX);
  if (N > (int64_t)INT32_MAX) return refuse(NLML_E_BADARG, who, "too many points for one launch");
  *run = N != 0;
  return 0;
}

int nlml_cosine_fit(const double* y, const double* w_deg, int64_t ld, const int32_t* n, const int32_t* h_n, int64_t C, const double* x0,
                    double xtol, double ftol, double* x, double* fun, int32_t* nfev, int32_t* nit, int32_t* status, void* stream) {
  bool run;
  if (int rc = check_cosine_fit("cosine_fit", !y || !w_deg || !n || !h_n || !x0 || !x, C, ld, h_n, &run)) return rc;
  if (!run) return 0;
  if (!aligned(y, 8) || !aligned(w_deg, 8) || !aligned(x0, 8) || !aligned(x, 8) || !aligned(fun, 8))
    return fail(NLML_E_BADARG, "cosine_fit: f64 buffers must be 8-byte aligned");
  if (!aligned(n, 4) || !aligned(nfev, 4) || !aligned(nit, 4) || !aligned(status, 4))
    return fail(NLML_E_BADARG, "cosine_fit: i32 buffers must be 4-byte aligned");
  return launch_cosine_fit(y, w_deg, ld, n, C, x0, xtol, ftol, x, fun, nfev, nit, status, stream);
}

// the same fits (cosine_fit_ref.h) on host buffers: plain C++, no HIP call
int nlml_cosine_fit_host(const double* h_y, const double* h_w_deg, int64_t ld, const int32_t* h_n, int64_t C, const double* h_x0,
                         double xtol, double ftol, double* h_x, double* h_fun, int32_t* h_nfev, int32_t* h_nit, int32_t* h_status) {
  bool run;
  if (int rc = check_cosine_fit("cosine_fit_host", !h_y || !h_w_deg || !h_n || !h_x0 || !h_x, C, ld, h_n, &run)) return rc;
  if (!run) return 0;
  for (int64_t f = 0; f < C; ++f)
    cf_fit_host(h_y + f * ld, h_w_deg + f * ld, h_n[f], h_x0 + f * CF_NPAR, xtol, ftol, h_x + f * CF_NPAR, h_fun ? h_fun + f : nullptr,
                h_nfev ? h_nfev + f : nullptr, h_nit ? h_nit + f : nullptr, h_status ? h_status + f : nullptr);
  return 0;
}

int nlml_cosine_fit_objective(const double* y, const double* w_deg, int n, const double* params, int64_t N, double* out, void* stream) {
  bool run;
  if (int rc = check_cosine_objective("cosine_fit_objective", !y || !w_deg || !params || !out, n, N, &run)) return rc;
  if (!run) return 0;
  if (!aligned(y, 8) || !aligned(w_deg, 8) || !aligned(params, 8) || !aligned(out, 8))
    return fail(NLML_E_BADARG, "cosine_fit_objective: f64 buffers must be 8-byte aligned");
  return launch_cosine_fit_objective(y, w_deg, n, params, N, out, stream);
}

int nlml_cosine_fit_objective_host(const double* h_y, const double* h_w_deg, int n, const double* h_params, int64_t N, double* h_out) {
  bool run;
  if (int rc = check_cosine_objective("cosine_fit_objective_host", !h_y || !h_w_deg || !h_params || !h_out, n, N, &run)) return rc;
  for (int64_t e = 0; run && e < N; ++e) h_out[e] = cf_objective(h_y, h_w_deg, n, h_params + e * CF_NPAR);
  return 0;
}

// ---- K9: training steps of the landmark encoder (encoder_train_ref.h, encoder_train.hip) --------------------------------------
static_assert(ET_BATCH_MAX == NLML_ENCODER_TRAIN_BATCH_MAX && ET_STATUS_ORDER == NLML_ENCODER_TRAIN_CLAMPED_ORDER &&
              ET_STATUS_LABEL == NLML_ENCODER_TRAIN_CLAMPED_LABEL, "the header's constants are the kernels'");
// The checks of include/nlml_hpe.h ("K9 argument checks") in their stated order, shared by the four forms: train (grads wanted) or
// validation, device (workspace, alignment) or host.  -> 0 with *run = whether there is anything to do.
static int check_encoder_train(const char* who, bool train, bool device, const EtCall& c, const void* workspace, size_t workspace_bytes,
                               double lr, double weight_decay, bool* run) {
  *run = false;
  if (c.F != 136 && c.F != NLML_F_REFERENCE) return refuse(NLML_E_BADARG, who, "F = %d: expected 136 or %d", c.F, NLML_F_REFERENCE);
  if (c.batch < 1 || c.batch > NLML_ENCODER_TRAIN_BATCH_MAX)
    return refuse(NLML_E_BADARG, who, "batch = %d outside [1, %d]", c.batch, NLML_ENCODER_TRAIN_BATCH_MAX);
  if (c.n < 0) return refuse(NLML_E_BADARG, who, "negative n");
  if (c.n == 0) return 0;
  if (!c.x || !c.labels || !c.table[0] || !c.table[1] || !c.table[2] || !c.params || (train && !c.grads) || (device && !workspace))
    return refuse(NLML_E_BADARG, who, "null buffer");
  if (c.N < 1 || c.N > (int64_t)INT32_MAX) return refuse(NLML_E_BADARG, who, "N = %lld outside [1, 2^31 - 1]", (long long)c.N);
  if (c.ld_lab < 3) return refuse(NLML_E_BADARG, who, "ld_lab = %lld < 3", (long long)c.ld_lab);
  for (int t = 0; t < 3; ++t)
    if (c.rows[t] < 1) return refuse(NLML_E_BADARG, who, "target table %d has %d rows", t, c.rows[t]);
  if (c.ldx < c.F) return refuse(NLML_E_BADARG, who, "ldx = %lld < F = %d", (long long)c.ldx, c.F);
  if (c.ldx > INT64_MAX / 4 / c.N || c.ld_lab > INT64_MAX / 4 / c.N)
    return refuse(NLML_E_BADARG, who, "dataset too large for 64-bit byte offsets");
  if (train && !(std::isfinite(lr) && std::isfinite(weight_decay) && std::isfinite(c.max_norm) && c.max_norm >= 0.0))
    return refuse(NLML_E_BADARG, who, "lr, weight_decay and max_norm must be finite, max_norm not negative");
  if (device) {
    const size_t need = et_workspace(c.F, c.batch).net_bytes;
    if (workspace_bytes < need) return refuse(NLML_E_BADARG, who, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (!aligned(c.params, 16) || !aligned(c.grads, 16) || !aligned(workspace, 16))
      return refuse(NLML_E_BADARG, who, "params, grads and workspace must be 16-byte aligned");
    if (!aligned(c.x, 4) || !aligned(c.labels, 4) || !aligned(c.table[0], 4) || !aligned(c.table[1], 4) || !aligned(c.table[2], 4) ||
        !aligned(c.order, 4) || !aligned(c.loss_out, 4) || !aligned(c.norm_out, 4) || !aligned(c.status, 4))
      return refuse(NLML_E_BADARG, who, "f32 and i32 buffers must be 4-byte aligned");
  }
  *run = true;
  return 0;
}
static EtCall encoder_call(const float* x, int64_t ldx, int64_t N, const int32_t* labels, int64_t ld_lab, const float* t_yaw, int n_yaw,
                           const float* t_pitch, int n_pitch, const float* t_roll, int n_roll, float* params, float* grads, int F, int batch,
                           const int32_t* order, int64_t n, double lr, double weight_decay, double max_norm, int zero_grad, float* loss_out,
                           float* norm_out, int32_t* status) {
  EtCall c;
  c.x = x; c.ldx = ldx; c.N = N; c.labels = labels; c.ld_lab = ld_lab;
  c.table[0] = t_yaw; c.table[1] = t_pitch; c.table[2] = t_roll;
  c.rows[0] = n_yaw; c.rows[1] = n_pitch; c.rows[2] = n_roll;
  c.params = params; c.grads = grads; c.F = F; c.batch = batch; c.order = order; c.n = n;
  c.lr = (float)lr; c.wd = (float)weight_decay; c.max_norm = max_norm; c.zero_grad = zero_grad ? 1 : 0;
  c.loss_out = loss_out; c.norm_out = norm_out; c.status = status;
  return c;
}

size_t nlml_encoder_train_workspace_bytes(int F, int batch) {
  if ((F != 136 && F != NLML_F_REFERENCE) || batch < 1 || batch > NLML_ENCODER_TRAIN_BATCH_MAX) return 0;
  return et_workspace(F, batch).net_bytes;
}

int nlml_encoder_train_steps(const float* x, int64_t ldx, int64_t N, const int32_t* labels, int64_t ld_lab, const float* t_yaw, int n_yaw,
                             const float* t_pitch, int n_pitch, const float* t_roll, int n_roll, float* params, float* grads, int F,
                             int batch, const int32_t* order, int64_t n, double lr, double weight_decay, double max_norm, int zero_grad,
                             float* loss_out, float* norm_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const EtCall c = encoder_call(x, ldx, N, labels, ld_lab, t_yaw, n_yaw, t_pitch, n_pitch, t_roll, n_roll, params, grads, F, batch, order, n,
                                lr, weight_decay, max_norm, zero_grad, loss_out, norm_out, status);
  bool run;
  if (int rc = check_encoder_train("encoder_train_steps", true, true, c, workspace, workspace_bytes, lr, weight_decay, &run)) return rc;
  return run ? launch_encoder_train(c, workspace, stream) : 0;
}

int nlml_encoder_eval_losses(const float* x, int64_t ldx, int64_t N, const int32_t* labels, int64_t ld_lab, const float* t_yaw, int n_yaw,
                             const float* t_pitch, int n_pitch, const float* t_roll, int n_roll, const float* params, int F, int batch,
                             const int32_t* order, int64_t n, float* loss_out, int32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream) {
  const EtCall c = encoder_call(x, ldx, N, labels, ld_lab, t_yaw, n_yaw, t_pitch, n_pitch, t_roll, n_roll, const_cast<float*>(params), nullptr,
                                F, batch, order, n, 0.0, 0.0, 0.0, 0, loss_out, nullptr, status);
  bool run;
  if (int rc = check_encoder_train("encoder_eval_losses", false, true, c, workspace, workspace_bytes, 0.0, 0.0, &run)) return rc;
  return run ? launch_encoder_train(c, workspace, stream) : 0;
}

// the same order (encoder_train_ref.h) on host buffers: plain C++, no HIP call
int nlml_encoder_train_steps_host(const float* h_x, int64_t ldx, int64_t N, const int32_t* h_labels, int64_t ld_lab, const float* h_t_yaw,
                                  int n_yaw, const float* h_t_pitch, int n_pitch, const float* h_t_roll, int n_roll, float* h_params,
                                  float* h_grads, int F, int batch, const int32_t* h_order, int64_t n, double lr, double weight_decay,
                                  double max_norm, int zero_grad, float* h_loss_out, float* h_norm_out, int32_t* h_status) {
  const EtCall c = encoder_call(h_x, ldx, N, h_labels, ld_lab, h_t_yaw, n_yaw, h_t_pitch, n_pitch, h_t_roll, n_roll, h_params, h_grads, F, batch,
                                h_order, n, lr, weight_decay, max_norm, zero_grad, h_loss_out, h_norm_out, h_status);
  bool run;
  if (int rc = check_encoder_train("encoder_train_steps_host", true, false, c, nullptr, 0, lr, weight_decay, &run)) return rc;
  if (run) et_host_run(c);
  return 0;
}

int nlml_encoder_eval_losses_host(const float* h_x, int64_t ldx, int64_t N, const int32_t* h_labels, int64_t ld_lab, const float* h_t_yaw,
                                  int n_yaw, const float* h_t_pitch, int n_pitch, const float* h_t_roll, int n_roll, const float* h_params,
                                  int F, int batch, const int32_t* h_order, int64_t n, float* h_loss_out, int32_t* h_status) {
  const EtCall c = encoder_call(h_x, ldx, N, h_labels, ld_lab, h_t_yaw, n_yaw, h_t_pitch, n_pitch, h_t_roll, n_roll,
                                const_cast<float*>(h_params), nullptr, F, batch, h_order, n, 0.0, 0.0, 0.0, 0, h_loss_out, nullptr, h_status);
  bool run;
  if (int rc = check_encoder_train("encoder_eval_losses_host", false, false, c, nullptr, 0, 0.0, 0.0, &run)) return rc;
  if (run) et_host_run(c);
  return 0;
}

// ---- K10: training steps of the yaw, pitch and roll heads (heads_train_ref.h, heads_train.hip) --------------------------------
static_assert(HT_NETS_MAX == NLML_HEADS_TRAIN_NETS_MAX && HT_R_MAX == NLML_HEADS_TRAIN_R_MAX &&
              HT_STATUS_ORDER == NLML_HEADS_TRAIN_CLAMPED_ORDER, "the header's constants are the kernels'");
static_assert(sizeof(HtNet) == sizeof(nlml_heads_net) && offsetof(HtNet, y) == offsetof(nlml_heads_net, y) &&
              offsetof(HtNet, v) == offsetof(nlml_heads_net, v) && offsetof(HtNet, step0) == offsetof(nlml_heads_net, step0) &&
              offsetof(HtNet, status) == offsetof(nlml_heads_net, status), "HtNet is the header's nlml_heads_net");
// The checks of include/nlml_hpe.h ("K10 argument checks") in their stated order, shared by the four forms; fills *c.
static int check_heads_train(const char* who, bool train, bool device, const nlml_heads_net* nets, int n_nets, int R, int batch, double lr,
                             double weight_decay, double max_norm, const void* workspace, size_t workspace_bytes, HtCall* c) {
  if (n_nets < 1 || n_nets > NLML_HEADS_TRAIN_NETS_MAX)
    return refuse(NLML_E_BADARG, who, "n_nets = %d outside [1, %d]", n_nets, NLML_HEADS_TRAIN_NETS_MAX);
  if (R < 1 || R > NLML_HEADS_TRAIN_R_MAX) return refuse(NLML_E_BADARG, who, "R = %d outside [1, %d]", R, NLML_HEADS_TRAIN_R_MAX);
  if (batch < 1 || batch > NLML_ENCODER_TRAIN_BATCH_MAX)
    return refuse(NLML_E_BADARG, who, "batch = %d outside [1, %d]", batch, NLML_ENCODER_TRAIN_BATCH_MAX);
  if (!nets || (device && !workspace)) return refuse(NLML_E_BADARG, who, "null buffer");
  for (int i = 0; i < n_nets; ++i)
    if (!nets[i].x || !nets[i].y || !nets[i].params || (train && (!nets[i].grads || !nets[i].m || !nets[i].v)))
      return refuse(NLML_E_BADARG, who, "network %d: null buffer", i);
  for (int i = 0; i < n_nets; ++i)
    if (nets[i].n <= 0) return refuse(NLML_E_BADARG, who, "network %d: n = %lld, expected at least 1", i, (long long)nets[i].n);
  const size_t need = ht_workspace(R, batch).net_bytes * (size_t)n_nets;
  if ((device || workspace) && workspace_bytes < need)
    return refuse(NLML_E_BADARG, who, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  for (int i = 0; i < n_nets; ++i)
    if (nets[i].step0 < 0) return refuse(NLML_E_BADARG, who, "network %d: step0 = %lld is negative", i, (long long)nets[i].step0);
  for (int i = 0; i < n_nets; ++i) {
    const nlml_heads_net& a = nets[i];
    if (a.N < 1 || a.N > (int64_t)INT32_MAX) return refuse(NLML_E_BADARG, who, "network %d: N = %lld outside [1, 2^31 - 1]", i, (long long)a.N);
    if (a.ldx < R) return refuse(NLML_E_BADARG, who, "network %d: ldx = %lld < R = %d", i, (long long)a.ldx, R);
    if (a.ldx > INT64_MAX / 4 / a.N) return refuse(NLML_E_BADARG, who, "network %d: table too large for 64-bit byte offsets", i);
  }
  if (train && !(std::isfinite(lr) && std::isfinite(weight_decay) && std::isfinite(max_norm) && max_norm >= 0.0))
    return refuse(NLML_E_BADARG, who, "lr, weight_decay and max_norm must be finite, max_norm not negative");
  if (device) {
    if (!aligned(workspace, 16)) return refuse(NLML_E_BADARG, who, "params, grads, m, v and workspace must be 16-byte aligned");
    for (int i = 0; i < n_nets; ++i) {
      const nlml_heads_net& a = nets[i];
      if (!aligned(a.params, 16) || (train && (!aligned(a.grads, 16) || !aligned(a.m, 16) || !aligned(a.v, 16))))
        return refuse(NLML_E_BADARG, who, "params, grads, m, v and workspace must be 16-byte aligned");
      if (!aligned(a.x, 4) || !aligned(a.y, 4) || !aligned(a.order, 4) || !aligned(a.loss_out, 4) || !aligned(a.norm_out, 4) ||
          !aligned(a.status, 4))
        return refuse(NLML_E_BADARG, who, "f32 and i32 buffers must be 4-byte aligned");
    }
  }
  *c = HtCall{};
  for (int i = 0; i < n_nets; ++i) {
    const nlml_heads_net& a = nets[i];
    c->net[i] = HtNet{a.x, a.ldx, a.N, a.y, a.params, train ? a.grads : nullptr, train ? a.m : nullptr, train ? a.v : nullptr,
                      a.order, a.n, a.step0, a.loss_out, train ? a.norm_out : nullptr, a.status};
  }
  c->n_nets = n_nets; c->R = R; c->batch = batch; c->train = train ? 1 : 0;
  c->lr = lr; c->weight_decay = weight_decay; c->max_norm = max_norm;
  return 0;
}

size_t nlml_heads_train_workspace_bytes(int R, int batch, int n_nets) {
  if (R < 1 || R > NLML_HEADS_TRAIN_R_MAX || batch < 1 || batch > NLML_ENCODER_TRAIN_BATCH_MAX || n_nets < 1 ||
      n_nets > NLML_HEADS_TRAIN_NETS_MAX)
    return 0;
  return ht_workspace(R, batch).net_bytes * (size_t)n_nets;
}

int nlml_heads_train_steps(const nlml_heads_net* nets, int n_nets, int R, int batch, double lr, double weight_decay, double max_norm,
                           void* workspace, size_t workspace_bytes, void* stream) {
  HtCall c;
  if (int rc = check_heads_train("heads_train_steps", true, true, nets, n_nets, R, batch, lr, weight_decay, max_norm, workspace,
                                 workspace_bytes, &c))
    return rc;
  return launch_heads_train(c, workspace, stream);
}

int nlml_heads_eval_losses(const nlml_heads_net* nets, int n_nets, int R, int batch, void* workspace, size_t workspace_bytes, void* stream) {
  HtCall c;
  if (int rc = check_heads_train("heads_eval_losses", false, true, nets, n_nets, R, batch, 0.0, 0.0, 0.0, workspace, workspace_bytes, &c))
    return rc;
  return launch_heads_train(c, workspace, stream);
}

// the same order (heads_train_ref.h) on host buffers: plain C++, no HIP call
int nlml_heads_train_steps_host(const nlml_heads_net* h_nets, int n_nets, int R, int batch, double lr, double weight_decay, double max_norm,
                                void* h_workspace, size_t workspace_bytes) {
  HtCall c;
  if (int rc = check_heads_train("heads_train_steps_host", true, false, h_nets, n_nets, R, batch, lr, weight_decay, max_norm, h_workspace,
                                 workspace_bytes, &c))
    return rc;
  ht_host_run(c, h_workspace);
  return 0;
}

int nlml_heads_eval_losses_host(const nlml_heads_net* h_nets, int n_nets, int R, int batch, void* h_workspace, size_t workspace_bytes) {
  HtCall c;
  if (int rc = check_heads_train("heads_eval_losses_host", false, false, h_nets, n_nets, R, batch, 0.0, 0.0, 0.0, h_workspace,
                                 workspace_bytes, &c))
    return rc;
  ht_host_run(c, h_workspace);
  return 0;
}

// ---- host-side stepping of the Powell state machine (powell.h) --------------------------------
// S = PowellState (the shipped artefacts' 8 parameters, a constant of the type: nlml_powell_*) or PowellStateN (n = 3 + r_id
// parameters, remembered in the state the rank-aware device kernel runs: nlml_powell_*_n)
static bool dim_ok(int n) { return n >= 3 + NLML_TUCKER_RANK_MIN && n <= 3 + NLML_TUCKER_RANK_MAX; }

extern "C++" {   // templates have no C linkage
template <class S> static int powell_host_init(const char* who, void* h_state, int n, const double* h_x0, double xtol, double ftol) {
  if (!dim_ok(n)) return bad_rank(who, n - 3);
  if (!h_state || !h_x0) return refuse(NLML_E_BADARG, who, "null pointer");
  S& s = *static_cast<S*>(h_state);
  if (S::kDyn) std::memset(h_state, 0, sizeof(S));
  s.set_dim(n);
  powell_init(s, h_x0, xtol, ftol);
  return 0;
}

template <class S> static int powell_host_step(const char* who, void* h_state, double fin, double* h_xeval) {
  if (!h_state || !h_xeval) return refuse(NLML_E_BADARG, who, "null pointer");
  S& s = *static_cast<S*>(h_state);
  if (!dim_ok(s.dim())) return bad_rank(who, s.dim() - 3);
  const bool need = powell_step(s, fin);
  if (need) std::memcpy(h_xeval, s.xeval, sizeof(double) * s.dim());
  return need ? 1 : 0;
}

template <class S>
static int powell_host_result(const char* who, const void* h_state, double* h_x, double* h_fval, int* h_nfev, int* h_nit, int* h_status) {
  if (!h_state || !h_x) return refuse(NLML_E_BADARG, who, "null pointer");
  const S& s = *static_cast<const S*>(h_state);
  if (!dim_ok(s.dim())) return bad_rank(who, s.dim() - 3);
  std::memcpy(h_x, s.x, sizeof(double) * s.dim());
  if (h_fval) *h_fval = s.fval;
  if (h_nfev) *h_nfev = s.nfev;
  if (h_nit) *h_nit = s.iter;
  if (h_status) *h_status = s.status;
  return 0;
}
}  // extern "C++"

size_t nlml_powell_state_bytes(void) { return sizeof(PowellState); }
int nlml_powell_init(void* h_state, const double* h_x0, double xtol, double ftol) {
  return powell_host_init<PowellState>("powell_init", h_state, PW_N, h_x0, xtol, ftol);
}
int nlml_powell_step(void* h_state, double fin, double* h_xeval) { return powell_host_step<PowellState>("powell_step", h_state, fin, h_xeval); }
int nlml_powell_result(const void* h_state, double* h_x, double* h_fval, int* h_nfev, int* h_nit, int* h_status) {
  return powell_host_result<PowellState>("powell_result", h_state, h_x, h_fval, h_nfev, h_nit, h_status);
}

size_t nlml_powell_state_bytes_n(int n) { return dim_ok(n) ? sizeof(PowellStateN) : 0; }
int nlml_powell_init_n(void* h_state, int n, const double* h_x0, double xtol, double ftol) {
  return powell_host_init<PowellStateN>("powell_init_n", h_state, n, h_x0, xtol, ftol);
}
int nlml_powell_step_n(void* h_state, double fin, double* h_xeval) { return powell_host_step<PowellStateN>("powell_step_n", h_state, fin, h_xeval); }
int nlml_powell_result_n(const void* h_state, double* h_x, double* h_fval, int* h_nfev, int* h_nit, int* h_status) {
  return powell_host_result<PowellStateN>("powell_result_n", h_state, h_x, h_fval, h_nfev, h_nit, h_status);
}

}  // extern "C"
