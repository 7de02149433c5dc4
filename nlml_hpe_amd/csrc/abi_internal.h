// abi_internal.h -- error plumbing and cross-file declarations behind include/nlml_hpe.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nlml_hpe.h"

namespace nlml {

// Records msg in the thread-local error slot and returns code (never 0).
int fail(int code, const char* msg);
// The tail of every launcher: 0, or the pending HIP launch error recorded through fail() (abi.cpp).
int hip_launch_status();

// ---- K2 (encoder + heads): what every launcher shares --------------------------------------------------------------------
// The rows a K2 kernel reads.  `raw` given: the landmarks [B,468,3] themselves, row stride 1404 (without normalisation they ARE the
// feature rows); else x with row stride ldx.  vec4: rows may be read with 16-byte loads.
struct K2Input { const float* src; int64_t ld; int norm; bool vec4; };
inline K2Input k2_input(const float* x, int64_t ldx, const float* raw, int normalize, int F) {
  K2Input a;
  if (raw) {
    a.src = raw; a.ld = NLML_F_REFERENCE; a.norm = normalize ? 1 : 0;
  } else {
    a.src = x; a.ld = ldx; a.norm = 0;
  }
  a.vec4 = (F % 4 == 0) && (a.ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(a.src) & 15) == 0);
  return a;
}
// One K2 forward as every launcher gets it: the input, the batch, the blob, the outputs and the caller's workspace, already checked
// (abi.cpp, "K2 argument checks": B > 0, and whatever the form needs of ws / ws_bytes and of in.vec4 holds).  Host side only: the
// kernels take their own argument structs (k2_args).
struct K2Call {
  K2Input in;
  int64_t B;
  int F;
  const void* blob;
  float* out;
  float* latent;
  uint8_t* valid;
  void* ws;
  size_t ws_bytes;
};
// The arguments every K2 kernel takes (Args: hx::Args, bf::w8::Args or the f32 kernel's EncArgs) from a call; whatever else an Args
// holds keeps its default or is the launcher's to fill.
template <class Args> Args k2_args(const K2Call& c) {
  Args a{};
  a.B = c.B; a.F = c.F; a.blob = c.blob; a.out = c.out; a.latent = c.latent; a.valid = c.valid;
  a.x = c.in.src; a.ldx = c.in.ld; a.norm = c.in.norm;
  return a;
}
// The <VEC4, NORM> kernel instance of an input: calls fn(std::bool_constant<VEC4>{}, std::bool_constant<NORM>{}).
template <class Fn> void k2_with_variant(const K2Input& in, Fn&& fn) {
  if (in.norm) {
    if (in.vec4) fn(std::true_type{}, std::true_type{}); else fn(std::false_type{}, std::true_type{});
  } else {
    if (in.vec4) fn(std::true_type{}, std::false_type{}); else fn(std::false_type{}, std::false_type{});
  }
}

// pack.cpp
size_t blob_bytes_for(int F, int mode);
int pack_blob(int F, int mode, const float* const enc_w[6], const float* const enc_b[6],
              const float* const head_w[3][5], const float* const head_b[3][5],
              void* blob, size_t blob_bytes);

// The K2 launchers: a checked call, the launcher's own extras, the stream.  None of them refuses anything.
// encoder_heads.hip; reeval_over >= 0: the re-evaluation launch behind a split-f16 one
int launch_encoder_heads_f32(const K2Call& c, float* pre_tanh, unsigned long long* stamps, void* stream, int reeval_over = -1);
// the f32 image inside an NLML_MODE_F16X2S blob (layout.h, layout_strict_f32_image16): byte offset from the blob's start
size_t strict_f32_image_offset(int F);
// the strict-fast mode's re-evaluation launch behind its split-f16 kernels (fused, streamed, quad, layer-per-launch): the f32 kernel on
// that image, no mask.  Every strict-fast forward ends with it; abi.cpp's k2_forward is the one caller.
int launch_strict_reeval(const K2Call& c, void* stream);
// faces of a tile the strict-fast kernels re-evaluate themselves on the vector ALUs (as NLML_MODE_F16X2 does); a tile with more goes
// to the f32 re-evaluation launch.  0: every face beyond f16's range is re-evaluated on the f32 matrix cores -- one rule, one
// accuracy class (the strict parity kernel's bits), and no slow-path code inside the strict kernels.
constexpr int STRICT_INKERNEL_RESCUE_MAX = 0;
// encoder_heads_bf16_w8.hip (throughput mode, eight waves per workgroup)
int launch_encoder_heads_bf16(const K2Call& c, void* stream);
// encoder_heads_f16x2.hip (NLML_MODE_F16X2, the split-f16 parity mode's fused kernel)
int launch_encoder_heads_f16x2(const K2Call& c, void* stream);
// encoder_heads_f16x2_w8.hip (NLML_MODE_F16X2S, eight waves per workgroup: the strict-fast mode's fused kernel)
int launch_encoder_heads_f16x2_w8(const K2Call& c, void* stream);
// the same forward as TWO launches: the trunk (layers 0-2, the eight-wave kernel ending with layer 2's output in c.ws) and the streamed
// tail (encoder_heads_f16x2_tailws.hip: layers E3.. and the heads with the weights through LDS once per 256 faces); bit-identical to the
// fused kernel
size_t tailws_workspace_bytes(int64_t B, int F);
int launch_encoder_heads_f16x2_tailws(const K2Call& c, void* stream);
// the same forward with FOUR tiles per workgroup and the streamed tail inside the launch (encoder_heads_f16x2_w8.hip,
// encoder_heads_f16x2_w8q_kernel): bit-identical to the fused kernel.  The first quad_faces faces (a multiple of 256, or all B) go that
// way and the others through the fused kernel.
// c.ws holds the quad part's hand-over, quad_workspace_bytes(quad_faces) (1 KiB per face of whole 64-face tiles).
size_t quad_workspace_bytes(int64_t quad_faces);
int launch_encoder_heads_f16x2_w8_mixed(const K2Call& c, int64_t quad_faces, void* stream);
// The dispatcher's split (abi.cpp; exported as nlml_k2_quad_split): how many of B faces go through the four-tile kernel on a device of
// `cus` compute units -- whole rounds of one workgroup per unit, ((B / 64) / (4 cus)) * cus workgroups of 256 faces; 0 for cus <= 0
int64_t k2_quad_faces(int64_t B, int cus);
// encoder_heads_f16x2_tailws.hip: h3 = layer 2's output as operand fragments, nfb 32-face blocks of it -> poses (and the latent)
int launch_tail_ws(const void* blob, const void* h3, int64_t nfb, int64_t B, float* out, float* latent, void* stream);
// encoder_heads_f16x2_small.hip (split-f16 modes, big layers as separate launches + the tail's, for small batches; split: NLML_MODE_F16X2S)
size_t small_workspace_bytes(int64_t B, int F);
int launch_encoder_heads_f16x2_small(const K2Call& c, int split, void* stream);
// artefacts.hip
int launch_cosine_table(const float* angles, int64_t n, const double* cos_params, int R, double* out, void* stream);
int launch_mode5_product(const float* core, const float* U, int Q, int R5, int M, float* W, void* stream);
// normalize_ipd.hip
int launch_normalize_ipd(const float* raw, int64_t B, int normalize, float* out, uint8_t* valid,
                         void* stream);
// normalize_centroid.hip
int launch_normalize_centroid(const float* raw, int64_t B, float* out, uint8_t* valid, double* stats, void* stream);
// rotate_landmarks.hip (K6): rows = I * ny * np * nr of the grid, one face and pose each
int launch_compose_rotation_tensor(const float* base, int64_t rows, const double* rot_yaw, int ny, const double* rot_pitch, int np,
                                   const double* rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll, float* out,
                                   double* out64, void* stream);
int launch_rotate_landmarks(const float* lm, const double* rot, float* out, double* out64, int64_t B, void* stream);
// tucker_objective.hip, tucker_powell.hip: K3 and the device-side Powell minimiser for an identity rank r_id = 1..NLML_TUCKER_RANK_MAX
// (Wm [27 r_id, 1404], 3 + r_id parameters).  r_id == 5 runs the kernels with the rank as a constant, the shipped artefacts' code.
int launch_tucker_objective(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                            const double* cos_params, int64_t N, double* err, double* x_hat, int r_id, int order, void* stream);
int launch_tucker_powell(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N, const double* x0,
                         double* result, double* fval, int32_t* nfev, int32_t* nit, int32_t* status, int r_id, int order,
                         void* stream);

// tucker_gradient.hip (K3g): objective value and analytic gradient in the reference's operation order; workspace = the chains' rows + t
size_t tucker_gradient_workspace_bytes(int64_t N);
int launch_tucker_gradient(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index, const double* params,
                           const double* cos_params, int64_t N, double* err, double* grad, int r_id, void* workspace, void* stream);

// tucker_decompose.hip (K7a..K7d): the arguments are checked by the caller (abi.cpp); the workspace sizes are 0-free for checked shapes
size_t mode_gram_workspace_bytes(int64_t I, int64_t K);
// a_f64 / x_f64 / out_f64: that tensor is f64 instead of f32 (a projected tensor the decomposition keeps unrounded between two steps)
int launch_mode_gram(const void* A, int a_f64, int64_t I, int64_t K, double* G, void* ws, void* stream);
size_t pose_grams_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M);
int launch_pose_grams(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr, void* ws,
                      void* stream);
int launch_project_identity(const float* A, int64_t I, int64_t K, const double* U, int R, void* out, int out_f64, void* stream);
int launch_project_pose(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up,
                        int rp, const double* Ur, int rr, void* out, int out_f64, void* stream);

// tucker_residual.hip (K11): the call is checked by the caller (abi.cpp); TrArgs is tucker_residual_ref.h's.  ws unused when a.X is NULL.
struct TrArgs;
size_t tucker_residual_workspace_bytes(int64_t I, int64_t M);
int launch_tucker_residual(const TrArgs& a, int ry, int rp, int rr, double* sums, double* res_id, void* ws, void* stream);

// cosine_fit.hip (K8): C fits, one wave each; n i32[C] on the device.  The arguments are checked by the caller (abi.cpp).
int launch_cosine_fit(const double* y, const double* w_deg, int64_t ld, const int32_t* n, int64_t C, const double* x0, double xtol,
                      double ftol, double* x, double* fun, int32_t* nfev, int32_t* nit, int32_t* status, void* stream);
int launch_cosine_fit_objective(const double* y, const double* w_deg, int n, const double* params, int64_t N, double* out, void* stream);

// encoder_train.hip (K9): ceil(n / batch) training steps (c.grads == NULL: forward and loss only), all enqueued on the stream.  The
// call is checked by the caller (abi.cpp); EtCall is encoder_train_ref.h's.
struct EtCall;
int launch_encoder_train(const EtCall& c, void* workspace, void* stream);
// The launches K9 shares with K10: a step's forward layers and its backward layers over the 1..3 networks of a call, one launch per
// layer, the grid sized for the largest batch (MlpDims, MlpWorkspace: encoder_train_ref.h's).
struct MlpDims;
struct MlpWorkspace;
struct MlpLaunchNet {
  const float* x; int64_t ldx, N;       // the dataset rows
  const int32_t* order;
  const float* params; float* grads;    // grads unused by the forward launches
  char* block;                          // the network's workspace block (mlp_workspace)
  int B;                                // rows of this step's batch; 0: the network is exhausted
};
void mlp_launch_forward(const MlpDims& d, const MlpWorkspace& ws, const MlpLaunchNet* nets, int n_nets, int64_t slot0, void* stream);
void mlp_launch_backward(const MlpDims& d, const MlpWorkspace& ws, const MlpLaunchNet* nets, int n_nets, int zero_grad, void* stream);

// heads_train.hip (K10): the steps of up to three head networks (c.train == 0: forward and loss only), every launch shared by all of
// them, all enqueued on the stream.  The call is checked by the caller (abi.cpp); HtCall is heads_train_ref.h's.
struct HtCall;
int launch_heads_train(const HtCall& c, void* workspace, void* stream);

// video_post.hip
int launch_video_post(const float* pose_rad, const float* raw, const uint8_t* valid, int64_t S, double frame_w,
                      double frame_h, double alpha, double max_jump, double size, double* state, double* smoothed,
                      double* centre, double* endpoints, uint8_t* updated, void* stream);

// pose_eval.hip: everything of a call that is not a pointer, passed by value in the kernel arguments
struct PoseEvalArgs {
  double lo[3], hi[3];
  double scale;                                      // 10^decimals (exact for decimals <= 15)
  double ivl[NLML_POSE_EVAL_MAX_INTERVALS][2];
  int32_t axes[NLML_POSE_EVAL_MAX_INTERVALS];
  int K, decimals;
};
int launch_pose_eval(const float* pose_rad, const double* pred_deg, const uint8_t* valid, const double* gt_deg, int64_t B,
                     const PoseEvalArgs& args, double* workspace, double* record_out, double* result_out, double* pred_out,
                     uint8_t* keep_out, void* stream);
int launch_pose_eval_merge(const double* records, int64_t n, int K, double* record_out, double* result_out, void* stream);

}  // namespace nlml
