// torch_ops.cpp -- torch.ops.nlml_hpe.* registered from COMPILED code (SURVEY.md 7 "Design stance", 8b "Underlying op").
//
// A TORCH_LIBRARY shim over the C ABI of include/nlml_hpe.h, nothing else: it checks shapes and dtypes (a wrong shape must never
// reach a hand-written kernel), allocates the outputs with torch's allocator, takes torch's CURRENT HIP stream of the operand's
// device and calls the same nlml_* entry point the ctypes binding calls -- so the results are the same bits, and the host side of a
// call is one dispatcher hop instead of a Python wrapper (measured at a 64-face tick, tools/host_hop.py: 15.4 us per call through the
// round-3 Python-registered op, 11.1 us through the Python wrapper, 4.0 us for the bare C call).  Kernels are registered for the GPU
// backend only (ROCm tensors carry torch's CUDA dispatch key): a CPU tensor has no kernel to land on and the dispatcher raises --
// there is no CPU fallback.  Meta kernels give the output shapes for tracing.
//
// Built by csrc/Makefile into nlml_hpe_amd/libnlml_torch_ops.so (links libnlml_hpe_hip.so next to it) and loaded by ops.py with
// torch.ops.load_library; a missing library raises at import.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <string>
#include <tuple>
#include <vector>

#include "../../include/nlml_hpe.h"

namespace {

constexpr int64_t F_REF = NLML_F_REFERENCE;

void need(const at::Tensor& t, const char* name, at::ScalarType dt) {
  TORCH_CHECK(t.is_cuda(), name, ": expected a GPU tensor (there is no CPU fallback), got ", t.device());
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected ", dt, ", got ", t.scalar_type());
}

// a buffer whose data_ptr() / numel() are handed to the C ABI as (pointer, size): it must be one dense run of bytes
void need_dense(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_contiguous(), name, ": expected a contiguous tensor (its data_ptr() and numel() go to the kernel as pointer and size)");
}

void same_device(const at::Tensor& a, const at::Tensor& b, const char* nb) {
  TORCH_CHECK(a.device() == b.device(), nb, " is on ", b.device(), " but the first operand is on ", a.device(),
              ": all operands must share one GPU");
}

void check(int rc, const char* what) {
  if (rc != 0) {
    const char* msg = nlml_last_error();
    TORCH_CHECK(false, what, " failed (code ", rc, "): ", msg ? msg : "");
  }
}

// the launch goes to the operand's device, on torch's current stream of THAT device
struct OnDevice {
  c10::hip::HIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit OnDevice(const at::Tensor& t)
      : guard(t.device()), stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream()) {}
};

int td_order(const std::string& order) {
  if (order == "reference") return NLML_TD_ORDER_REFERENCE;
  if (order == "fast") return NLML_TD_ORDER_FAST;
  TORCH_CHECK(false, "unknown TD order '", order, "'; expected 'fast' or 'reference'");
}

at::Tensor normalize_ipd(const at::Tensor& raw_, bool normalize) {
  need(raw_, "raw", at::kFloat);
  TORCH_CHECK(raw_.dim() == 3 && raw_.size(1) == 468 && raw_.size(2) == 3, "raw: expected [B,468,3], got ", raw_.sizes());
  const at::Tensor raw = raw_.contiguous();
  const int64_t B = raw.size(0);
  at::Tensor out = at::empty({B, F_REF}, raw.options());
  OnDevice dev(raw);
  check(nlml_normalize_ipd(raw.data_ptr<float>(), B, normalize ? 1 : 0, out.data_ptr<float>(), nullptr, dev.stream), "nlml_normalize_ipd");
  return out;
}

// the reference's other normalisation (centroid and RMS radius): features only -- the face mask and the statistics come from the Python
// wrapper, ops.normalize_centroid
at::Tensor normalize_centroid(const at::Tensor& raw_) {
  need(raw_, "raw", at::kFloat);
  TORCH_CHECK(raw_.dim() == 3 && raw_.size(1) == 468 && raw_.size(2) == 3, "raw: expected [B,468,3], got ", raw_.sizes());
  const at::Tensor raw = raw_.contiguous();
  const int64_t B = raw.size(0);
  at::Tensor out = at::empty({B, F_REF}, raw.options());
  OnDevice dev(raw);
  check(nlml_normalize_centroid(raw.data_ptr<float>(), B, out.data_ptr<float>(), nullptr, nullptr, dev.stream), "nlml_normalize_centroid");
  return out;
}

// K6, grid mode: base f32[I,468,3], one f64[n,3,3] table per axis -> (out f32[I,ny,np,nr,1404], out64 f64[same] or an empty f64[0]).
// zero_index: the three zero bins (yaw, pitch, roll), -1 = none.
std::tuple<at::Tensor, at::Tensor> compose_rotation_tensor(const at::Tensor& base_, const at::Tensor& ry_, const at::Tensor& rp_,
                                                           const at::Tensor& rr_, int64_t order, at::IntArrayRef zero_index, bool return_f64) {
  need(base_, "base", at::kFloat);
  TORCH_CHECK(base_.dim() == 3 && base_.size(1) == 468 && base_.size(2) == 3, "base: expected [I,468,3], got ", base_.sizes());
  const at::Tensor* const tabs[] = {&ry_, &rp_, &rr_};
  const char* const names[] = {"rot_yaw", "rot_pitch", "rot_roll"};
  for (int k = 0; k < 3; ++k) {
    need(*tabs[k], names[k], at::kDouble);
    same_device(base_, *tabs[k], names[k]);
    TORCH_CHECK(tabs[k]->dim() == 3 && tabs[k]->size(1) == 3 && tabs[k]->size(2) == 3, names[k], ": expected [n,3,3], got ", tabs[k]->sizes());
  }
  TORCH_CHECK(zero_index.size() == 3, "zero_index: expected 3 values (yaw, pitch, roll)");
  const at::Tensor base = base_.contiguous(), ry = ry_.contiguous(), rp = rp_.contiguous(), rr = rr_.contiguous();
  const int64_t I = base.size(0), ny = ry.size(0), np = rp.size(0), nr = rr.size(0);
  TORCH_CHECK(ny <= INT32_MAX && np <= INT32_MAX && nr <= INT32_MAX, "more than 2^31 - 1 bins on an axis");
  for (int k = 0; k < 3; ++k)
    TORCH_CHECK(zero_index[k] >= -1 && zero_index[k] < tabs[k]->size(0), "zero_index[", k, "] = ", zero_index[k], " is outside -1..n-1");
  at::Tensor out = at::empty({I, ny, np, nr, F_REF}, base.options());
  at::Tensor out64 = return_f64 ? at::empty({I, ny, np, nr, F_REF}, ry.options()) : at::empty({0}, ry.options());
  OnDevice dev(base);
  check(nlml_compose_rotation_tensor(base.data_ptr<float>(), I, ry.data_ptr<double>(), (int)ny, rp.data_ptr<double>(), (int)np,
                                     rr.data_ptr<double>(), (int)nr, (int)order, (int)zero_index[0], (int)zero_index[1], (int)zero_index[2],
                                     out.data_ptr<float>(), return_f64 ? out64.data_ptr<double>() : nullptr, dev.stream),
        "nlml_compose_rotation_tensor");
  return {out, out64};
}

// K6, one pose per face: lm f32[B,468,3], rot f64[B,3,3,3] (application order) -> (f32[B,468,3], f64[B,468,3]); the one not asked for
// is an empty [0]
std::tuple<at::Tensor, at::Tensor> rotate_landmarks(const at::Tensor& lm_, const at::Tensor& rot_, bool return_f32, bool return_f64) {
  need(lm_, "lm", at::kFloat);
  need(rot_, "rot", at::kDouble);
  same_device(lm_, rot_, "rot");
  TORCH_CHECK(lm_.dim() == 3 && lm_.size(1) == 468 && lm_.size(2) == 3, "lm: expected [B,468,3], got ", lm_.sizes());
  const int64_t B = lm_.size(0);
  TORCH_CHECK(rot_.dim() == 4 && rot_.size(0) == B && rot_.size(1) == 3 && rot_.size(2) == 3 && rot_.size(3) == 3, "rot: expected [", B,
              ",3,3,3], got ", rot_.sizes());
  TORCH_CHECK(return_f32 || return_f64, "rotate_landmarks: at least one of return_f32, return_f64");
  const at::Tensor lm = lm_.contiguous(), rot = rot_.contiguous();
  at::Tensor out = return_f32 ? at::empty({B, 468, 3}, lm.options()) : at::empty({0}, lm.options());
  at::Tensor out64 = return_f64 ? at::empty({B, 468, 3}, rot.options()) : at::empty({0}, rot.options());
  OnDevice dev(lm);
  check(nlml_rotate_landmarks(lm.data_ptr<float>(), rot.data_ptr<double>(), return_f32 ? out.data_ptr<float>() : nullptr,
                              return_f64 ? out64.data_ptr<double>() : nullptr, B, dev.stream), "nlml_rotate_landmarks");
  return {out, out64};
}

// The K2 forwards: the checks, the allocation and the call behind the five forward ops and landmarks_to_pose_valid.  in_ is the raw
// landmarks [B,468,3] (landmarks) or the feature rows [B,F]; ws given = the layer-per-launch path through that workspace, else the fused
// launch; want_valid adds the "a face was found" mask u8[B] (row not all-zero).
struct K2Out { at::Tensor pose, valid; };
K2Out k2_forward(const at::Tensor& in_, bool landmarks, const at::Tensor& blob, int64_t F, bool normalize, const at::Tensor* ws,
                 bool want_valid) {
  need(in_, landmarks ? "raw" : "x", at::kFloat);
  need(blob, "packed_w", at::kByte);
  need_dense(blob, "packed_w");
  if (ws) {
    need(*ws, "workspace", at::kByte);
    need_dense(*ws, "workspace");
  }
  same_device(in_, blob, "packed_w");
  if (ws) same_device(in_, *ws, "workspace");
  if (landmarks) {
    TORCH_CHECK(in_.dim() == 3 && in_.size(1) == 468 && in_.size(2) == 3, "raw: expected [B,468,3], got ", in_.sizes());
  } else {
    TORCH_CHECK(in_.dim() == 2 && in_.size(1) == F, "x: expected [B,", F, "], got ", in_.sizes());
  }
  const at::Tensor in = !landmarks && in_.stride(1) == 1 ? in_ : in_.contiguous();
  const int64_t B = in.size(0);
  K2Out r{at::empty({B, 3}, in.options()), want_valid ? at::empty({B}, in.options().dtype(at::kByte)) : at::Tensor()};
  uint8_t* const valid = want_valid ? r.valid.data_ptr<uint8_t>() : nullptr;
  float* const out = r.pose.data_ptr<float>();
  const size_t blob_bytes = (size_t)blob.numel();
  const float* const src = in.data_ptr<float>();
  const int64_t ldx = B > 1 ? in.stride(0) : F;   // of feature rows
  const int norm = normalize ? 1 : 0;
  OnDevice dev(in);
  // No workspace given: where the library says its _ws dispatcher would send a part of this batch through the four-tile strict-fast
  // kernel, give it that part's scratch from torch's allocator (stream-ordered: freed at return, reused only behind this launch).
  at::Tensor quad_ws;
  int64_t quad_faces = 0;
  size_t quad_bytes = 0;
  if (!ws && nlml_k2_quad_part(src, landmarks ? F_REF : ldx, B, (int)F, blob_bytes, &quad_faces, &quad_bytes) == 0 && quad_faces > 0)
    quad_ws = at::empty({(int64_t)quad_bytes}, in.options().dtype(at::kByte));
  // the entry point, chosen once: plain, _small through the caller's workspace, or _ws through the quad part's
  static const char* const names[2][3] = {{"nlml_encoder_heads_fwd", "nlml_encoder_heads_fwd_small", "nlml_encoder_heads_fwd_ws"},
                                          {"nlml_landmarks_to_pose", "nlml_landmarks_to_pose_small", "nlml_landmarks_to_pose_ws"}};
  const int form = quad_ws.defined() ? 2 : ws ? 1 : 0;
  const at::Tensor* const scratch = form == 2 ? &quad_ws : ws;
  void* const wsp = scratch ? scratch->data_ptr() : nullptr;
  const size_t wsn = scratch ? (size_t)scratch->numel() : 0;
  int rc;
  if (landmarks) {
    const auto with_ws = form == 2 ? nlml_landmarks_to_pose_ws : nlml_landmarks_to_pose_small;
    rc = form ? with_ws(src, B, norm, blob.data_ptr(), blob_bytes, out, nullptr, valid, wsp, wsn, dev.stream)
              : nlml_landmarks_to_pose(src, B, norm, blob.data_ptr(), blob_bytes, out, nullptr, valid, dev.stream);
  } else {
    const auto with_ws = form == 2 ? nlml_encoder_heads_fwd_ws : nlml_encoder_heads_fwd_small;
    rc = form ? with_ws(src, ldx, B, (int)F, blob.data_ptr(), blob_bytes, out, nullptr, valid, wsp, wsn, dev.stream)
              : nlml_encoder_heads_fwd(src, ldx, B, (int)F, blob.data_ptr(), blob_bytes, out, nullptr, valid, dev.stream);
  }
  check(rc, names[landmarks][form]);
  return r;
}

at::Tensor encoder_heads_fwd(const at::Tensor& x, const at::Tensor& blob, int64_t F) {
  return k2_forward(x, false, blob, F, false, nullptr, false).pose;
}
at::Tensor landmarks_to_pose(const at::Tensor& raw, const at::Tensor& blob, bool normalize) {
  return k2_forward(raw, true, blob, F_REF, normalize, nullptr, false).pose;
}
at::Tensor encoder_heads_fwd_small(const at::Tensor& x, const at::Tensor& blob, int64_t F, const at::Tensor& ws) {
  return k2_forward(x, false, blob, F, false, &ws, false).pose;
}
at::Tensor landmarks_to_pose_small(const at::Tensor& raw, const at::Tensor& blob, bool normalize, const at::Tensor& ws) {
  return k2_forward(raw, true, blob, F_REF, normalize, &ws, false).pose;
}
// the video tick's forward: pose AND the face mask in one call; `ws` empty = the fused launch
std::tuple<at::Tensor, at::Tensor> landmarks_to_pose_valid(const at::Tensor& raw, const at::Tensor& blob, bool normalize,
                                                           const std::optional<at::Tensor>& ws) {
  K2Out r = k2_forward(raw, true, blob, F_REF, normalize, ws.has_value() ? &*ws : nullptr, true);
  return {r.pose, r.valid};
}

// -> the identity rank R of Wm [27 R, 1404]; params (objective, gradient): f64[N, 3 + R], one row of x per row of it
int check_td(const at::Tensor& Wm, const at::Tensor& x, const at::Tensor& cosp, const at::Tensor* params = nullptr) {
  need(Wm, "Wm", at::kFloat);
  need(x, "x", at::kFloat);
  need(cosp, "cos_params", at::kDouble);
  same_device(x, Wm, "Wm");
  same_device(x, cosp, "cos_params");
  TORCH_CHECK(Wm.dim() == 2 && Wm.size(1) == F_REF && Wm.size(0) % 27 == 0 && Wm.size(0) >= 27 * NLML_TUCKER_RANK_MIN &&
                  Wm.size(0) <= 27 * NLML_TUCKER_RANK_MAX,
              "Wm: expected [27*R,1404] for an identity rank R in [", NLML_TUCKER_RANK_MIN, ", ", NLML_TUCKER_RANK_MAX, "], got ", Wm.sizes());
  TORCH_CHECK(x.dim() == 2 && x.size(1) == F_REF, "x: expected [N,1404], got ", x.sizes());
  TORCH_CHECK(cosp.dim() == 3 && cosp.size(0) == 3 && cosp.size(1) == 3 && cosp.size(2) == 4, "cos_params: expected [3,3,4], got ", cosp.sizes());
  const int r_id = (int)(Wm.size(0) / 27);
  if (params) {
    need(*params, "params", at::kDouble);
    same_device(x, *params, "params");
    TORCH_CHECK(params->dim() == 2 && params->size(1) == 3 + r_id, "params: expected [N,", 3 + r_id, "], got ", params->sizes());
    TORCH_CHECK(x.size(0) == params->size(0), "x has ", x.size(0), " rows but params has ", params->size(0));
  }
  return r_id;
}

at::Tensor tucker_objective(const at::Tensor& Wm_, const at::Tensor& x_, const at::Tensor& params_, const at::Tensor& cosp_,
                            std::string order) {
  const int r_id = check_td(Wm_, x_, cosp_, &params_);
  const at::Tensor Wm = Wm_.contiguous(), x = x_.contiguous(), params = params_.contiguous(), cosp = cosp_.contiguous();
  const int64_t N = params.size(0);
  at::Tensor err = at::empty({N}, params.options());
  OnDevice dev(x);
  check(nlml_tucker_objective_r(Wm.data_ptr<float>(), x.data_ptr<float>(), F_REF, nullptr, params.data_ptr<double>(),
                                cosp.data_ptr<double>(), N, err.data_ptr<double>(), nullptr, r_id, td_order(order), dev.stream),
        "nlml_tucker_objective_r");
  return err;
}

// K3g: objective value and analytic gradient in the reference's operation order -> (err f64[N], grad f64[N,3+R])
std::tuple<at::Tensor, at::Tensor> tucker_gradient(const at::Tensor& Wm_, const at::Tensor& x_, const at::Tensor& params_,
                                                   const at::Tensor& cosp_) {
  const int r_id = check_td(Wm_, x_, cosp_, &params_);
  const at::Tensor Wm = Wm_.contiguous(), x = x_.contiguous(), params = params_.contiguous(), cosp = cosp_.contiguous();
  const int64_t N = params.size(0);
  at::Tensor err = at::empty({N}, params.options()), grad = at::empty({N, 3 + r_id}, params.options());
  const size_t ws_bytes = nlml_tucker_gradient_workspace_bytes(N, r_id);
  at::Tensor ws = at::empty({(int64_t)(ws_bytes / sizeof(double))}, params.options());
  OnDevice dev(x);
  check(nlml_tucker_gradient_r(Wm.data_ptr<float>(), x.data_ptr<float>(), F_REF, nullptr, params.data_ptr<double>(),
                               cosp.data_ptr<double>(), N, err.data_ptr<double>(), grad.data_ptr<double>(), r_id, ws.data_ptr(), ws_bytes,
                               dev.stream),
        "nlml_tucker_gradient_r");
  return {err, grad};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> tucker_powell(const at::Tensor& Wm_, const at::Tensor& x_,
                                                                                      const at::Tensor& cosp_, std::string order) {
  const int r_id = check_td(Wm_, x_, cosp_);
  const at::Tensor Wm = Wm_.contiguous(), x = x_.contiguous(), cosp = cosp_.contiguous();
  const int64_t N = x.size(0);
  const auto f64 = x.options().dtype(at::kDouble), i32 = x.options().dtype(at::kInt);
  at::Tensor res = at::empty({N, 3 + r_id}, f64), fun = at::empty({N}, f64), nfev = at::empty({N}, i32), nit = at::empty({N}, i32),
             status = at::empty({N}, i32);
  OnDevice dev(x);
  check(nlml_tucker_powell_r(Wm.data_ptr<float>(), x.data_ptr<float>(), F_REF, cosp.data_ptr<double>(), N, nullptr,
                             res.data_ptr<double>(), fun.data_ptr<double>(), nfev.data_ptr<int32_t>(), nit.data_ptr<int32_t>(),
                             status.data_ptr<int32_t>(), r_id, td_order(order), dev.stream), "nlml_tucker_powell_r");
  return {res, fun, nfev, nit, status};
}

// one video tick, everything in place: `state` f64[S,6] and the caller's output buffers smoothed f64[S,3] (degrees), centre f64[S,2],
// endpoints f64[S,3,2], updated u8[S] -- a stream that is skipped (no face / non-finite pose) keeps its previous outputs, as the
// C entry point specifies
void video_post(const at::Tensor& pose_, const at::Tensor& raw_, const std::optional<at::Tensor>& valid_, double frame_w, double frame_h,
                double alpha, double max_jump, double size, at::Tensor state, at::Tensor sm, at::Tensor centre, at::Tensor ep,
                at::Tensor upd) {
  need(pose_, "pose_rad", at::kFloat);
  need(raw_, "raw", at::kFloat);
  need(state, "state", at::kDouble);
  need(sm, "smoothed", at::kDouble);
  need(centre, "centre", at::kDouble);
  need(ep, "endpoints", at::kDouble);
  need(upd, "updated", at::kByte);
  const at::Tensor* const others[] = {&raw_, &state, &sm, &centre, &ep, &upd};
  for (const at::Tensor* t : others) same_device(pose_, *t, "video_post operand");
  const int64_t S = pose_.size(0);
  TORCH_CHECK(pose_.dim() == 2 && pose_.size(1) == 3, "pose_rad: expected [S,3], got ", pose_.sizes());
  TORCH_CHECK(raw_.dim() == 3 && raw_.size(0) == S && raw_.size(1) == 468 && raw_.size(2) == 3, "raw: expected [S,468,3], got ", raw_.sizes());
  TORCH_CHECK(state.is_contiguous() && state.numel() == S * 6 && sm.is_contiguous() && sm.numel() == S * 3 && centre.is_contiguous() &&
                  centre.numel() == S * 2 && ep.is_contiguous() && ep.numel() == S * 6 && upd.is_contiguous() && upd.numel() == S,
              "video_post: state [S,6], smoothed [S,3], centre [S,2], endpoints [S,3,2], updated [S], all contiguous");
  const at::Tensor pose = pose_.contiguous(), raw = raw_.contiguous();
  at::Tensor valid;
  if (valid_.has_value()) {
    need(*valid_, "valid", at::kByte);
    same_device(pose_, *valid_, "valid");
    TORCH_CHECK(valid_->dim() == 1 && valid_->size(0) == S, "valid: expected [S]");
    valid = valid_->contiguous();
  }
  OnDevice dev(pose);
  check(nlml_video_post_ex(pose.data_ptr<float>(), raw.data_ptr<float>(), valid.defined() ? valid.data_ptr<uint8_t>() : nullptr, S,
                           frame_w, frame_h, alpha, max_jump, size, state.data_ptr<double>(), sm.data_ptr<double>(),
                           centre.data_ptr<double>(), ep.data_ptr<double>(), upd.data_ptr<uint8_t>(), dev.stream), "nlml_video_post_ex");
}

at::Tensor cosine_table(const at::Tensor& angles_, const at::Tensor& cosp_) {
  need(angles_, "angles_rad", at::kFloat);
  need(cosp_, "cos_params", at::kDouble);
  same_device(angles_, cosp_, "cos_params");
  TORCH_CHECK(angles_.dim() == 1 && cosp_.dim() == 2 && cosp_.size(1) == 4, "expected angles [n] and cos_params [R,4]");
  const at::Tensor angles = angles_.contiguous(), cosp = cosp_.contiguous();
  at::Tensor out = at::empty({angles.size(0), cosp.size(0)}, cosp.options());
  OnDevice dev(angles);
  check(nlml_cosine_table(angles.data_ptr<float>(), angles.size(0), cosp.data_ptr<double>(), (int)cosp.size(0), out.data_ptr<double>(),
                          dev.stream), "nlml_cosine_table");
  return out;
}

// K8: C cosine fits in one launch.  y, w_deg f64[C,ld], n the row counts (host integers: the entry point checks them; their device copy
// is made here), x0 f64[C,4] -> (x f64[C,4], fun f64[C], nfev, nit, status i32[C])
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> cosine_fit(const at::Tensor& y_, const at::Tensor& w_, at::IntArrayRef n,
                                                                                   const at::Tensor& x0_, double xtol, double ftol) {
  need(y_, "y", at::kDouble);
  need(w_, "w_deg", at::kDouble);
  need(x0_, "x0", at::kDouble);
  same_device(y_, w_, "w_deg");
  same_device(y_, x0_, "x0");
  TORCH_CHECK(y_.dim() == 2 && w_.sizes() == y_.sizes(), "y and w_deg: expected two [C,ld] tensors of one shape, got ", y_.sizes(), ", ", w_.sizes());
  const int64_t C = y_.size(0), ld = y_.size(1);
  TORCH_CHECK(x0_.dim() == 2 && x0_.size(0) == C && x0_.size(1) == 4, "x0: expected [", C, ",4], got ", x0_.sizes());
  TORCH_CHECK((int64_t)n.size() == C, "n: expected ", C, " row counts, got ", n.size());
  std::vector<int32_t> h_n(n.size());
  for (size_t f = 0; f < n.size(); ++f) {
    TORCH_CHECK(n[f] >= 1 && n[f] <= NLML_COSINE_FIT_ROWS_MAX && n[f] <= ld, "n[", f, "] = ", n[f], " outside [1, min(", NLML_COSINE_FIT_ROWS_MAX,
                ", ld = ", ld, ")]");
    h_n[f] = (int32_t)n[f];
  }
  const at::Tensor y = y_.contiguous(), w = w_.contiguous(), x0 = x0_.contiguous();
  const auto f64 = y.options(), i32 = y.options().dtype(at::kInt);
  at::Tensor d_n = at::empty({C}, i32);
  if (C) d_n.copy_(at::from_blob(h_n.data(), {C}, at::TensorOptions().dtype(at::kInt)));   // pageable source: the copy is complete on return
  at::Tensor res = at::empty({C, 4}, f64), fun = at::empty({C}, f64), nfev = at::empty({C}, i32), nit = at::empty({C}, i32),
             status = at::empty({C}, i32);
  OnDevice dev(y);
  check(nlml_cosine_fit(y.data_ptr<double>(), w.data_ptr<double>(), ld, d_n.data_ptr<int32_t>(), h_n.data(), C, x0.data_ptr<double>(), xtol,
                        ftol, res.data_ptr<double>(), fun.data_ptr<double>(), nfev.data_ptr<int32_t>(), nit.data_ptr<int32_t>(),
                        status.data_ptr<int32_t>(), dev.stream), "nlml_cosine_fit");
  return {res, fun, nfev, nit, status};
}

// K9: ceil(n / batch) training steps of the encoder, params and grads f32[P] updated in place.  x f32[N,>=F] with unit column stride
// (a padded row stride is passed on as ldx), labels i32[N,>=3], the tables f32[.,3], order i32[n] or None (the rows in turn)
// -> (loss f32[steps], norm f32[steps], status i32[1]); the workspace comes from torch's allocator
std::tuple<at::Tensor, at::Tensor, at::Tensor> encoder_train_steps(const at::Tensor& x, const at::Tensor& labels_, const at::Tensor& ty_,
                                                                   const at::Tensor& tp_, const at::Tensor& tr_, at::Tensor params,
                                                                   at::Tensor grads, const std::optional<at::Tensor>& order_, int64_t n,
                                                                   int64_t batch, double lr, double weight_decay, double max_norm,
                                                                   bool zero_grad) {
  need(x, "x", at::kFloat);
  need(labels_, "labels", at::kInt);
  need(ty_, "t_yaw", at::kFloat);
  need(tp_, "t_pitch", at::kFloat);
  need(tr_, "t_roll", at::kFloat);
  need(params, "params", at::kFloat);
  need(grads, "grads", at::kFloat);
  need_dense(params, "params");
  need_dense(grads, "grads");
  const at::Tensor* operands[] = {&labels_, &ty_, &tp_, &tr_, &params, &grads};
  for (const at::Tensor* t : operands) same_device(x, *t, "an operand");
  TORCH_CHECK(x.dim() == 2 && x.size(0) >= 1 && (x.size(1) == 136 || x.size(1) == F_REF) && x.stride(1) == 1 && x.stride(0) >= x.size(1),
              "x: expected [N,136] or [N,1404] with unit column stride, got ", x.sizes(), " strides ", x.strides());
  const int64_t N = x.size(0), F = x.size(1);
  TORCH_CHECK(labels_.dim() == 2 && labels_.size(0) == N && labels_.size(1) >= 3, "labels: expected [", N, ",>=3], got ", labels_.sizes());
  for (const at::Tensor* t : {&ty_, &tp_, &tr_})
    TORCH_CHECK(t->dim() == 2 && t->size(0) >= 1 && t->size(1) == 3, "a target table: expected [rows,3], got ", t->sizes());
  TORCH_CHECK(batch >= 1 && batch <= NLML_ENCODER_TRAIN_BATCH_MAX, "batch = ", batch, " outside [1, ", NLML_ENCODER_TRAIN_BATCH_MAX, "]");
  TORCH_CHECK(n >= 0, "negative n");
  const at::Tensor labels = labels_.contiguous(), ty = ty_.contiguous(), tp = tp_.contiguous(), tr = tr_.contiguous();
  const size_t ws_bytes = nlml_encoder_train_workspace_bytes((int)F, (int)batch);
  // P from the workspace-independent rule of the header
  const int64_t P = 1024 * F + 1024 + 512 * 1024 + 512 + 256 * 512 + 256 + 128 * 256 + 128 + 64 * 128 + 64 + 9 * 64 + 9;
  TORCH_CHECK(params.numel() == P && grads.numel() == P, "params and grads: expected ", P, " elements each, got ", params.numel(), ", ", grads.numel());
  at::Tensor order;
  if (order_.has_value()) {
    need(*order_, "order", at::kInt);
    same_device(x, *order_, "order");
    TORCH_CHECK(order_->dim() == 1 && order_->size(0) >= n, "order: expected at least n = ", n, " entries, got ", order_->sizes());
    order = order_->contiguous();
  }
  const int64_t steps = (n + batch - 1) / batch;
  const auto f32 = x.options(), i32 = x.options().dtype(at::kInt);
  at::Tensor loss = at::empty({steps}, f32), norm = at::empty({steps}, f32), status = at::zeros({1}, i32);
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, x.options().dtype(at::kByte));
  OnDevice dev(x);
  check(nlml_encoder_train_steps(x.data_ptr<float>(), x.stride(0), N, labels.data_ptr<int32_t>(), labels.size(1), ty.data_ptr<float>(),
                                 (int)ty.size(0), tp.data_ptr<float>(), (int)tp.size(0), tr.data_ptr<float>(), (int)tr.size(0),
                                 params.data_ptr<float>(), grads.data_ptr<float>(), (int)F, (int)batch,
                                 order.defined() ? order.data_ptr<int32_t>() : nullptr, n, lr, weight_decay, max_norm, zero_grad ? 1 : 0,
                                 loss.data_ptr<float>(), norm.data_ptr<float>(), status.data_ptr<int32_t>(), ws.data_ptr(), ws_bytes,
                                 dev.stream), "nlml_encoder_train_steps");
  return {loss, norm, status};
}

// K10: the training steps of up to three head networks, params / grads / m / v f32[P] each updated in place.  x[i] f32[N_i,R] with unit
// column stride (a padded row stride is passed on as ldx), y[i] f32[N_i], order[i] i32[>= n_i] or None (the rows in turn), n[i] rows
// visited, step0[i] Adam steps taken before -> (loss f32[steps_i] per network, norm likewise, status i32[n_nets]); the workspace comes
// from torch's allocator
std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>, at::Tensor> heads_train_steps(
    at::TensorList x, at::TensorList y_, at::TensorList params, at::TensorList grads, at::TensorList m, at::TensorList v,
    const c10::List<std::optional<at::Tensor>>& order_, at::IntArrayRef n, at::IntArrayRef step0, int64_t batch, double lr,
    double weight_decay, double max_norm) {
  const int64_t nets = (int64_t)x.size();
  TORCH_CHECK(nets >= 1 && nets <= NLML_HEADS_TRAIN_NETS_MAX, "expected 1..", NLML_HEADS_TRAIN_NETS_MAX, " networks, got ", nets);
  TORCH_CHECK((int64_t)y_.size() == nets && (int64_t)params.size() == nets && (int64_t)grads.size() == nets && (int64_t)m.size() == nets &&
              (int64_t)v.size() == nets && (int64_t)order_.size() == nets && (int64_t)n.size() == nets && (int64_t)step0.size() == nets,
              "every per-network list must have ", nets, " entries");
  TORCH_CHECK(batch >= 1 && batch <= NLML_ENCODER_TRAIN_BATCH_MAX, "batch = ", batch, " outside [1, ", NLML_ENCODER_TRAIN_BATCH_MAX, "]");
  need(x[0], "x", at::kFloat);
  const int64_t R = x[0].dim() == 2 ? x[0].size(1) : 0;
  TORCH_CHECK(R >= 1 && R <= NLML_HEADS_TRAIN_R_MAX, "x: expected [N,R] with R in [1, ", NLML_HEADS_TRAIN_R_MAX, "], got ", x[0].sizes());
  int64_t P = 0, fan_in = R;
  for (int64_t w : {128, 256, 128, 64, 1}) { P += w * fan_in + w; fan_in = w; }
  const auto f32 = x[0].options(), i32 = x[0].options().dtype(at::kInt);
  std::vector<at::Tensor> keep, loss, norm;
  at::Tensor status = at::zeros({nets}, i32);
  nlml_heads_net call[NLML_HEADS_TRAIN_NETS_MAX] = {};
  for (int64_t i = 0; i < nets; ++i) {
    need(x[i], "x", at::kFloat);
    need(y_[i], "y", at::kFloat);
    same_device(x[0], x[i], "x");
    same_device(x[0], y_[i], "y");
    TORCH_CHECK(x[i].dim() == 2 && x[i].size(0) >= 1 && x[i].size(1) == R && x[i].stride(1) == 1 && x[i].stride(0) >= R,
                "x: expected [N,", R, "] with unit column stride, got ", x[i].sizes(), " strides ", x[i].strides());
    TORCH_CHECK(y_[i].dim() == 1 && y_[i].size(0) == x[i].size(0), "y: expected [", x[i].size(0), "], got ", y_[i].sizes());
    for (const at::Tensor* t : {&params[i], &grads[i], &m[i], &v[i]}) {
      need(*t, "params, grads, m, v", at::kFloat);
      need_dense(*t, "params, grads, m, v");
      same_device(x[0], *t, "params, grads, m, v");
      TORCH_CHECK(t->numel() == P, "params, grads, m, v: expected ", P, " elements each, got ", t->numel());
    }
    TORCH_CHECK(n[i] >= 1 && step0[i] >= 0, "n must be at least 1 and step0 not negative");
    const at::Tensor y = y_[i].contiguous();
    keep.push_back(y);
    const std::optional<at::Tensor> order_i = order_.get(i);
    const int32_t* order = nullptr;
    if (order_i.has_value()) {
      need(*order_i, "order", at::kInt);
      same_device(x[0], *order_i, "order");
      TORCH_CHECK(order_i->dim() == 1 && order_i->size(0) >= n[i], "order: expected at least n = ", n[i], " entries, got ", order_i->sizes());
      keep.push_back(order_i->contiguous());
      order = keep.back().data_ptr<int32_t>();
    } else {
      TORCH_CHECK(n[i] <= x[i].size(0), "n = ", n[i], " beyond the ", x[i].size(0), " rows of x");
    }
    const int64_t steps = (n[i] + batch - 1) / batch;
    loss.push_back(at::empty({steps}, f32));
    norm.push_back(at::empty({steps}, f32));
    call[i] = nlml_heads_net{x[i].data_ptr<float>(), x[i].stride(0), x[i].size(0), y.data_ptr<float>(), params[i].data_ptr<float>(),
                             grads[i].data_ptr<float>(), m[i].data_ptr<float>(), v[i].data_ptr<float>(), order, n[i], step0[i],
                             loss[i].data_ptr<float>(), norm[i].data_ptr<float>(), status.data_ptr<int32_t>() + i};
  }
  const size_t ws_bytes = nlml_heads_train_workspace_bytes((int)R, (int)batch, (int)nets);
  at::Tensor ws = at::empty({(int64_t)ws_bytes}, x[0].options().dtype(at::kByte));
  OnDevice dev(x[0]);
  check(nlml_heads_train_steps(call, (int)nets, (int)R, (int)batch, lr, weight_decay, max_norm, ws.data_ptr(), ws_bytes, dev.stream),
        "nlml_heads_train_steps");
  return {loss, norm, status};
}

// K5: the evaluation block in one native pass.  pose f32[B,3] radians or f64[B,3] degrees (by dtype), valid bool/u8[B] or None,
// gt f64[B,3]; lo / hi the inclusive GT range, intervals [K*2] (low, high) with their axes [K]; the records' workspace comes from
// torch's allocator -> (record f64[12+2K], result f64[14+2K])
std::tuple<at::Tensor, at::Tensor> pose_eval(const at::Tensor& pose_, const std::optional<at::Tensor>& valid_, const at::Tensor& gt_,
                                             at::ArrayRef<double> lo, at::ArrayRef<double> hi, int64_t decimals,
                                             at::ArrayRef<double> intervals, at::ArrayRef<int64_t> axes) {
  TORCH_CHECK(pose_.is_cuda(), "pose: expected a GPU tensor (there is no CPU fallback), got ", pose_.device());
  TORCH_CHECK(pose_.scalar_type() == at::kFloat || pose_.scalar_type() == at::kDouble, "pose: expected float32 radians or float64 degrees");
  need(gt_, "gt", at::kDouble);
  same_device(pose_, gt_, "gt");
  const int64_t B = pose_.size(0);
  TORCH_CHECK(pose_.dim() == 2 && pose_.size(1) == 3 && gt_.dim() == 2 && gt_.size(0) == B && gt_.size(1) == 3,
              "pose and gt: expected [B,3] each, got ", pose_.sizes(), " and ", gt_.sizes());
  TORCH_CHECK(lo.size() == 3 && hi.size() == 3, "lo / hi: expected 3 values each");
  const int64_t K = (int64_t)axes.size();
  TORCH_CHECK((int64_t)intervals.size() == 2 * K, "intervals: expected 2 values per axis entry");
  TORCH_CHECK(K <= NLML_POSE_EVAL_MAX_INTERVALS, "at most ", NLML_POSE_EVAL_MAX_INTERVALS, " intervals");
  std::vector<int32_t> ax(axes.begin(), axes.end());
  const at::Tensor pose = pose_.contiguous(), gt = gt_.contiguous();
  at::Tensor valid;
  if (valid_.has_value()) {
    TORCH_CHECK(valid_->scalar_type() == at::kBool || valid_->scalar_type() == at::kByte, "valid: expected bool or uint8");
    same_device(pose_, *valid_, "valid");
    TORCH_CHECK(valid_->dim() == 1 && valid_->size(0) == B, "valid: expected [B]");
    valid = valid_->contiguous();
  }
  const auto f64 = gt.options();
  at::Tensor ws = at::empty({std::max<int64_t>(1, (int64_t)nlml_pose_eval_workspace_bytes(B, (int)K) / 8)}, f64);
  at::Tensor record = at::empty({12 + 2 * K}, f64), result = at::empty({14 + 2 * K}, f64);
  const bool f32 = pose.scalar_type() == at::kFloat;
  OnDevice dev(pose);
  check(nlml_pose_eval(f32 ? pose.data_ptr<float>() : nullptr, f32 ? nullptr : pose.data_ptr<double>(),
                       valid.defined() ? static_cast<const uint8_t*>(valid.data_ptr()) : nullptr, gt.data_ptr<double>(), B, lo.data(),
                       hi.data(), (int)decimals, intervals.data(), ax.data(), (int)K, ws.data_ptr(), (size_t)ws.numel() * 8,
                       record.data_ptr<double>(), result.data_ptr<double>(), nullptr, nullptr, dev.stream), "nlml_pose_eval");
  return {record, result};
}

std::tuple<at::Tensor, at::Tensor> pose_eval_merge(const at::Tensor& records_, int64_t K) {
  need(records_, "records", at::kDouble);
  TORCH_CHECK(K >= 0 && K <= NLML_POSE_EVAL_MAX_INTERVALS, "K: at most ", NLML_POSE_EVAL_MAX_INTERVALS, " intervals");
  TORCH_CHECK(records_.dim() == 2 && records_.size(1) == 12 + 2 * K, "records: expected [n,", 12 + 2 * K, "], got ", records_.sizes());
  const at::Tensor records = records_.contiguous();
  at::Tensor record = at::empty({12 + 2 * K}, records.options()), result = at::empty({14 + 2 * K}, records.options());
  OnDevice dev(records);
  check(nlml_pose_eval_merge(records.data_ptr<double>(), records.size(0), (int)K, record.data_ptr<double>(), result.data_ptr<double>(),
                             dev.stream), "nlml_pose_eval_merge");
  return {record, result};
}

// ---- K7: the Tucker decomposition's primitives; workspaces come from torch's allocator ----------------------------------
int64_t ws_doubles(size_t bytes) { return std::max<int64_t>(1, (int64_t)((bytes + 7) / 8)); }

const at::Tensor need_tensor5(const at::Tensor& X_, const char* name) {
  need(X_, name, at::kFloat);
  TORCH_CHECK(X_.dim() == 5, name, ": expected [I,ny,np,nr,M], got ", X_.sizes());
  TORCH_CHECK(X_.size(1) <= NLML_POSE_BINS_MAX && X_.size(2) <= NLML_POSE_BINS_MAX && X_.size(3) <= NLML_POSE_BINS_MAX, name,
              ": at most ", NLML_POSE_BINS_MAX, " bins per pose mode, got ", X_.sizes());
  return X_.contiguous();
}

// A f32[I,K] -> G f64[I,I] = A A^T
at::Tensor mode_gram(const at::Tensor& A_) {
  need(A_, "A", at::kFloat);
  TORCH_CHECK(A_.dim() == 2, "A: expected [I,K], got ", A_.sizes());
  const at::Tensor A = A_.contiguous();
  const int64_t I = A.size(0), K = A.size(1);
  const auto f64 = A.options().dtype(at::kDouble);
  at::Tensor G = at::empty({I, I}, f64), ws = at::empty({ws_doubles(nlml_mode_gram_workspace_bytes(I, K))}, f64);
  OnDevice dev(A);
  check(nlml_mode_gram(A.data_ptr<float>(), I, K, G.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel() * 8, dev.stream), "nlml_mode_gram");
  return G;
}

// X f32[I,ny,np,nr,M] -> (Gy f64[ny,ny], Gp f64[np,np], Gr f64[nr,nr])
std::tuple<at::Tensor, at::Tensor, at::Tensor> pose_grams(const at::Tensor& X_) {
  const at::Tensor X = need_tensor5(X_, "X");
  const int64_t I = X.size(0), ny = X.size(1), np = X.size(2), nr = X.size(3), M = X.size(4);
  const auto f64 = X.options().dtype(at::kDouble);
  at::Tensor Gy = at::empty({ny, ny}, f64), Gp = at::empty({np, np}, f64), Gr = at::empty({nr, nr}, f64);
  at::Tensor ws = at::empty({ws_doubles(nlml_pose_grams_workspace_bytes(I, (int)ny, (int)np, (int)nr, M))}, f64);
  OnDevice dev(X);
  check(nlml_pose_grams(X.data_ptr<float>(), I, (int)ny, (int)np, (int)nr, M, Gy.data_ptr<double>(), Gp.data_ptr<double>(),
                        Gr.data_ptr<double>(), ws.data_ptr(), (size_t)ws.numel() * 8, dev.stream), "nlml_pose_grams");
  return {Gy, Gp, Gr};
}

// A f32[I,K], U f64[I,R] -> f32[R,K] = U^T A
at::Tensor project_identity(const at::Tensor& A_, const at::Tensor& U_) {
  need(A_, "A", at::kFloat);
  need(U_, "U", at::kDouble);
  same_device(A_, U_, "U");
  TORCH_CHECK(A_.dim() == 2 && U_.dim() == 2 && U_.size(0) == A_.size(0), "A [I,K] and U [I,R] disagree: ", A_.sizes(), ", ", U_.sizes());
  TORCH_CHECK(U_.size(1) >= NLML_TUCKER_RANK_MIN && U_.size(1) <= NLML_TUCKER_RANK_MAX, "U: R outside 1..", NLML_TUCKER_RANK_MAX);
  const at::Tensor A = A_.contiguous(), U = U_.contiguous();
  at::Tensor out = at::empty({U.size(1), A.size(1)}, A.options());
  OnDevice dev(A);
  check(nlml_project_identity(A.data_ptr<float>(), A.size(0), A.size(1), U.data_ptr<double>(), (int)U.size(1), out.data_ptr<float>(),
                              dev.stream), "nlml_project_identity");
  return out;
}

// X f32[I,ny,np,nr,M], each factor f64[n,r] or None (the mode stays) -> f32[I,ny',np',nr',M]
at::Tensor project_pose(const at::Tensor& X_, const std::optional<at::Tensor>& Uy_, const std::optional<at::Tensor>& Up_,
                        const std::optional<at::Tensor>& Ur_) {
  const at::Tensor X = need_tensor5(X_, "X");
  const std::optional<at::Tensor>* const opt[] = {&Uy_, &Up_, &Ur_};
  const char* const names[] = {"U_yaw", "U_pitch", "U_roll"};
  at::Tensor U[3];
  std::vector<int64_t> shape = {X.size(0), X.size(1), X.size(2), X.size(3), X.size(4)};
  for (int k = 0; k < 3; ++k) {
    if (!opt[k]->has_value()) continue;
    const at::Tensor& u = **opt[k];
    need(u, names[k], at::kDouble);
    same_device(X, u, names[k]);
    TORCH_CHECK(u.dim() == 2 && u.size(0) == X.size(1 + k), names[k], ": expected [", X.size(1 + k), ",r], got ", u.sizes());
    TORCH_CHECK(u.size(1) >= 1 && u.size(1) <= NLML_POSE_RANK_MAX, names[k], ": rank outside 1..", NLML_POSE_RANK_MAX);
    U[k] = u.contiguous();
    shape[1 + k] = u.size(1);
  }
  at::Tensor out = at::empty(shape, X.options());
  auto ptr = [&](int k) { return U[k].defined() ? U[k].data_ptr<double>() : nullptr; };
  auto rank = [&](int k) { return U[k].defined() ? (int)U[k].size(1) : 0; };
  OnDevice dev(X);
  check(nlml_project_pose(X.data_ptr<float>(), X.size(0), (int)X.size(1), (int)X.size(2), (int)X.size(3), X.size(4), ptr(0), rank(0), ptr(1),
                          rank(1), ptr(2), rank(2), out.data_ptr<float>(), dev.stream), "nlml_project_pose");
  return out;
}

// K11: X f32[I,ny,np,nr,M] or None (expand only), W f32[R,ry,rp,rr,M], the four factors f64[n,r] -> (sums f64[2], res_id f64[I],
// xhat f32[I,ny,np,nr,M]); an output that is not asked for (or, without X, not computed) is an empty tensor
std::tuple<at::Tensor, at::Tensor, at::Tensor> tucker_residual(const std::optional<at::Tensor>& X_, const at::Tensor& W_, const at::Tensor& Uid_,
                                                               const at::Tensor& Uy_, const at::Tensor& Up_, const at::Tensor& Ur_,
                                                               bool want_res_id, bool want_xhat) {
  need(W_, "W", at::kFloat);
  TORCH_CHECK(W_.dim() == 5, "W: expected [R,ry,rp,rr,M], got ", W_.sizes());
  TORCH_CHECK(W_.size(0) >= NLML_TUCKER_RANK_MIN && W_.size(0) <= NLML_TUCKER_RANK_MAX, "W: identity rank outside 1..", NLML_TUCKER_RANK_MAX);
  const at::Tensor* const in[] = {&Uid_, &Uy_, &Up_, &Ur_};
  const char* const names[] = {"U_id", "U_yaw", "U_pitch", "U_roll"};
  at::Tensor U[4];
  for (int k = 0; k < 4; ++k) {
    need(*in[k], names[k], at::kDouble);
    same_device(W_, *in[k], names[k]);
    TORCH_CHECK(in[k]->dim() == 2 && in[k]->size(0) >= 1 && in[k]->size(1) == W_.size(k), names[k], ": expected [n,", W_.size(k), "], got ",
                in[k]->sizes());
    TORCH_CHECK(k == 0 || (in[k]->size(1) <= NLML_POSE_RANK_MAX && in[k]->size(0) <= NLML_POSE_BINS_MAX), names[k], ": at most ",
                NLML_POSE_BINS_MAX, " bins and rank ", NLML_POSE_RANK_MAX, ", got ", in[k]->sizes());
    U[k] = in[k]->contiguous();
  }
  const at::Tensor W = W_.contiguous();
  const int64_t I = U[0].size(0), ny = U[1].size(0), np = U[2].size(0), nr = U[3].size(0), M = W.size(4);
  TORCH_CHECK(M >= 1, "W: no columns");
  at::Tensor X;
  if (X_.has_value()) {
    X = need_tensor5(*X_, "X");
    same_device(W, X, "X");
    TORCH_CHECK(X.size(0) == I && X.size(1) == ny && X.size(2) == np && X.size(3) == nr && X.size(4) == M,
                "X: expected the factors' rows by W's columns, got ", X.sizes());
  } else {
    want_xhat = true;
    want_res_id = false;
  }
  const auto f64 = W.options().dtype(at::kDouble);
  at::Tensor sums = at::empty({X.defined() ? 2 : 0}, f64), res_id = at::empty({want_res_id ? I : 0}, f64);
  at::Tensor xhat = want_xhat ? at::empty({I, ny, np, nr, M}, W.options()) : at::empty({0}, W.options());
  at::Tensor ws = at::empty({ws_doubles(X.defined() ? nlml_tucker_residual_workspace_bytes(I, (int)ny, (int)np, (int)nr, M) : 0)}, f64);
  OnDevice dev(W);
  check(nlml_tucker_residual(X.defined() ? X.data_ptr<float>() : nullptr, W.data_ptr<float>(), U[0].data_ptr<double>(), U[1].data_ptr<double>(),
                             U[2].data_ptr<double>(), U[3].data_ptr<double>(), I, (int)ny, (int)np, (int)nr, M, (int)W.size(0), (int)W.size(1),
                             (int)W.size(2), (int)W.size(3), X.defined() ? sums.data_ptr<double>() : nullptr,
                             want_res_id ? res_id.data_ptr<double>() : nullptr, want_xhat ? xhat.data_ptr<float>() : nullptr, ws.data_ptr(),
                             (size_t)ws.numel() * 8, dev.stream), "nlml_tucker_residual");
  return {sums, res_id, xhat};
}

// ---- shapes only (Meta backend: tracing / fake tensors) -------------------------------------------------------------
at::Tensor mode_gram_meta(const at::Tensor& A) { return at::empty({A.size(0), A.size(0)}, A.options().dtype(at::kDouble)); }
std::tuple<at::Tensor, at::Tensor, at::Tensor> pose_grams_meta(const at::Tensor& X) {
  const auto f64 = X.options().dtype(at::kDouble);
  return {at::empty({X.size(1), X.size(1)}, f64), at::empty({X.size(2), X.size(2)}, f64), at::empty({X.size(3), X.size(3)}, f64)};
}
at::Tensor project_identity_meta(const at::Tensor& A, const at::Tensor& U) { return at::empty({U.size(1), A.size(1)}, A.options()); }
at::Tensor project_pose_meta(const at::Tensor& X, const std::optional<at::Tensor>& Uy, const std::optional<at::Tensor>& Up,
                             const std::optional<at::Tensor>& Ur) {
  return at::empty({X.size(0), Uy.has_value() ? Uy->size(1) : X.size(1), Up.has_value() ? Up->size(1) : X.size(2),
                    Ur.has_value() ? Ur->size(1) : X.size(3), X.size(4)}, X.options());
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> tucker_residual_meta(const std::optional<at::Tensor>& X, const at::Tensor& W, const at::Tensor& Uid,
                                                                    const at::Tensor& Uy, const at::Tensor& Up, const at::Tensor& Ur,
                                                                    bool want_res_id, bool want_xhat) {
  const auto f64 = W.options().dtype(at::kDouble);
  const bool x = X.has_value();
  return {at::empty({x ? 2 : 0}, f64), at::empty({x && want_res_id ? Uid.size(0) : 0}, f64),
          want_xhat || !x ? at::empty({Uid.size(0), Uy.size(0), Up.size(0), Ur.size(0), W.size(4)}, W.options()) : at::empty({0}, W.options())};
}
at::Tensor normalize_ipd_meta(const at::Tensor& raw, bool) { return at::empty({raw.size(0), F_REF}, raw.options()); }
at::Tensor normalize_centroid_meta(const at::Tensor& raw) { return at::empty({raw.size(0), F_REF}, raw.options()); }
std::tuple<at::Tensor, at::Tensor> compose_rotation_tensor_meta(const at::Tensor& base, const at::Tensor& ry, const at::Tensor& rp,
                                                                const at::Tensor& rr, int64_t, at::IntArrayRef, bool return_f64) {
  const std::vector<int64_t> shape = {base.size(0), ry.size(0), rp.size(0), rr.size(0), F_REF};
  return {at::empty(shape, base.options()), return_f64 ? at::empty(shape, ry.options()) : at::empty({0}, ry.options())};
}
std::tuple<at::Tensor, at::Tensor> rotate_landmarks_meta(const at::Tensor& lm, const at::Tensor& rot, bool return_f32, bool return_f64) {
  return {return_f32 ? at::empty({lm.size(0), 468, 3}, lm.options()) : at::empty({0}, lm.options()),
          return_f64 ? at::empty({lm.size(0), 468, 3}, rot.options()) : at::empty({0}, rot.options())};
}
template <class... Rest> at::Tensor pose_meta(const at::Tensor& x, const at::Tensor&, Rest...) { return at::empty({x.size(0), 3}, x.options()); }
at::Tensor tucker_objective_meta(const at::Tensor&, const at::Tensor&, const at::Tensor& params, const at::Tensor&, std::string) {
  return at::empty({params.size(0)}, params.options());
}
std::tuple<at::Tensor, at::Tensor> tucker_gradient_meta(const at::Tensor&, const at::Tensor&, const at::Tensor& params, const at::Tensor&) {
  return {at::empty({params.size(0)}, params.options()), at::empty({params.size(0), params.size(1)}, params.options())};
}
std::tuple<at::Tensor, at::Tensor> pose_valid_meta(const at::Tensor& raw, const at::Tensor&, bool, const std::optional<at::Tensor>&) {
  return {at::empty({raw.size(0), 3}, raw.options()), at::empty({raw.size(0)}, raw.options().dtype(at::kByte))};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> tucker_powell_meta(const at::Tensor& Wm, const at::Tensor& x, const at::Tensor&,
                                                                                           std::string) {
  const int64_t N = x.size(0), n_par = 3 + Wm.size(0) / 27;   // Wm [27 R, 1404] -> 3 + R parameters per face
  const auto f64 = x.options().dtype(at::kDouble), i32 = x.options().dtype(at::kInt);
  return {at::empty({N, n_par}, f64), at::empty({N}, f64), at::empty({N}, i32), at::empty({N}, i32), at::empty({N}, i32)};
}
void video_post_meta(const at::Tensor&, const at::Tensor&, const std::optional<at::Tensor>&, double, double, double, double, double, at::Tensor,
                     at::Tensor, at::Tensor, at::Tensor, at::Tensor) {}   // everything in place: nothing to shape
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> cosine_fit_meta(const at::Tensor& y, const at::Tensor&, at::IntArrayRef,
                                                                                        const at::Tensor&, double, double) {
  const int64_t C = y.size(0);
  const auto i32 = y.options().dtype(at::kInt);
  return {at::empty({C, 4}, y.options()), at::empty({C}, y.options()), at::empty({C}, i32), at::empty({C}, i32), at::empty({C}, i32)};
}
std::tuple<at::Tensor, at::Tensor, at::Tensor> encoder_train_steps_meta(const at::Tensor& x, const at::Tensor&, const at::Tensor&, const at::Tensor&,
                                                                        const at::Tensor&, at::Tensor, at::Tensor, const std::optional<at::Tensor>&,
                                                                        int64_t n, int64_t batch, double, double, double, bool) {
  const int64_t steps = batch > 0 ? (n + batch - 1) / batch : 0;
  return {at::empty({steps}, x.options()), at::empty({steps}, x.options()), at::empty({1}, x.options().dtype(at::kInt))};
}
std::tuple<std::vector<at::Tensor>, std::vector<at::Tensor>, at::Tensor> heads_train_steps_meta(
    at::TensorList x, at::TensorList, at::TensorList, at::TensorList, at::TensorList, at::TensorList, const c10::List<std::optional<at::Tensor>>&,
    at::IntArrayRef n, at::IntArrayRef, int64_t batch, double, double, double) {
  std::vector<at::Tensor> loss, norm;
  for (size_t i = 0; i < x.size(); ++i) {
    const int64_t steps = batch > 0 && i < n.size() ? (n[i] + batch - 1) / batch : 0;
    loss.push_back(at::empty({steps}, x[i].options()));
    norm.push_back(at::empty({steps}, x[i].options()));
  }
  return {loss, norm, at::empty({(int64_t)x.size()}, x[0].options().dtype(at::kInt))};
}
at::Tensor cosine_table_meta(const at::Tensor& angles, const at::Tensor& cosp) { return at::empty({angles.size(0), cosp.size(0)}, cosp.options()); }

std::tuple<at::Tensor, at::Tensor> pose_eval_meta(const at::Tensor& pose, const std::optional<at::Tensor>&, const at::Tensor& gt,
                                                  at::ArrayRef<double>, at::ArrayRef<double>, int64_t, at::ArrayRef<double>,
                                                  at::ArrayRef<int64_t> axes) {
  const int64_t K = (int64_t)axes.size();
  return {at::empty({12 + 2 * K}, gt.options()), at::empty({14 + 2 * K}, gt.options())};
}
std::tuple<at::Tensor, at::Tensor> pose_eval_merge_meta(const at::Tensor& records, int64_t K) {
  return {at::empty({12 + 2 * K}, records.options()), at::empty({14 + 2 * K}, records.options())};
}

}  // namespace

TORCH_LIBRARY(nlml_hpe, m) {
  m.def("normalize_ipd(Tensor raw, bool normalize) -> Tensor");
  m.def("normalize_centroid(Tensor raw) -> Tensor");
  m.def("compose_rotation_tensor(Tensor base, Tensor rot_yaw, Tensor rot_pitch, Tensor rot_roll, int order, int[] zero_index, "
        "bool return_f64=False) -> (Tensor, Tensor)");
  m.def("rotate_landmarks(Tensor lm, Tensor rot, bool return_f32=True, bool return_f64=False) -> (Tensor, Tensor)");
  m.def("encoder_heads_fwd(Tensor x, Tensor packed_w, int F) -> Tensor");
  m.def("landmarks_to_pose(Tensor raw, Tensor packed_w, bool normalize) -> Tensor");
  m.def("encoder_heads_fwd_small(Tensor x, Tensor packed_w, int F, Tensor workspace) -> Tensor");
  m.def("landmarks_to_pose_small(Tensor raw, Tensor packed_w, bool normalize, Tensor workspace) -> Tensor");
  m.def("landmarks_to_pose_valid(Tensor raw, Tensor packed_w, bool normalize, Tensor? workspace) -> (Tensor, Tensor)");
  m.def("tucker_objective(Tensor Wm, Tensor x, Tensor params, Tensor cos_params, str order=\"reference\") -> Tensor");
  m.def("tucker_gradient(Tensor Wm, Tensor x, Tensor params, Tensor cos_params) -> (Tensor, Tensor)");
  m.def("tucker_powell(Tensor Wm, Tensor x, Tensor cos_params, str order=\"reference\") -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("video_post(Tensor pose_rad, Tensor raw, Tensor? valid, float frame_w, float frame_h, float alpha, float max_jump, float size, "
        "Tensor(a!) state, Tensor(b!) smoothed, Tensor(c!) centre, Tensor(d!) endpoints, Tensor(e!) updated) -> ()");
  m.def("cosine_table(Tensor angles_rad, Tensor cos_params) -> Tensor");
  m.def("cosine_fit(Tensor y, Tensor w_deg, int[] n, Tensor x0, float xtol=1e-4, float ftol=1e-4) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("encoder_train_steps(Tensor x, Tensor labels, Tensor t_yaw, Tensor t_pitch, Tensor t_roll, Tensor(a!) params, Tensor(b!) grads, "
        "Tensor? order, int n, int batch, float lr, float weight_decay, float max_norm, bool zero_grad) -> (Tensor, Tensor, Tensor)");
  m.def("heads_train_steps(Tensor[] x, Tensor[] y, Tensor(a!)[] params, Tensor(b!)[] grads, Tensor(c!)[] m, Tensor(d!)[] v, Tensor?[] order, "
        "int[] n, int[] step0, int batch, float lr, float weight_decay, float max_norm) -> (Tensor[], Tensor[], Tensor)");
  m.def("pose_eval(Tensor pose, Tensor? valid, Tensor gt, float[] lo, float[] hi, int decimals, float[] intervals, int[] axes) "
        "-> (Tensor, Tensor)");
  m.def("pose_eval_merge(Tensor records, int K) -> (Tensor, Tensor)");
  m.def("mode_gram(Tensor A) -> Tensor");
  m.def("pose_grams(Tensor X) -> (Tensor, Tensor, Tensor)");
  m.def("project_identity(Tensor A, Tensor U) -> Tensor");
  m.def("project_pose(Tensor X, Tensor? U_yaw, Tensor? U_pitch, Tensor? U_roll) -> Tensor");
  m.def("tucker_residual(Tensor? X, Tensor W, Tensor U_id, Tensor U_yaw, Tensor U_pitch, Tensor U_roll, bool want_res_id=False, "
        "bool want_xhat=False) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(nlml_hpe, CUDA, m) {   // ROCm tensors dispatch on torch's CUDA key
  m.impl("normalize_ipd", &normalize_ipd);
  m.impl("normalize_centroid", &normalize_centroid);
  m.impl("compose_rotation_tensor", &compose_rotation_tensor);
  m.impl("rotate_landmarks", &rotate_landmarks);
  m.impl("encoder_heads_fwd", &encoder_heads_fwd);
  m.impl("landmarks_to_pose", &landmarks_to_pose);
  m.impl("encoder_heads_fwd_small", &encoder_heads_fwd_small);
  m.impl("landmarks_to_pose_small", &landmarks_to_pose_small);
  m.impl("landmarks_to_pose_valid", &landmarks_to_pose_valid);
  m.impl("tucker_objective", &tucker_objective);
  m.impl("tucker_gradient", &tucker_gradient);
  m.impl("tucker_powell", &tucker_powell);
  m.impl("video_post", &video_post);
  m.impl("cosine_table", &cosine_table);
  m.impl("cosine_fit", &cosine_fit);
  m.impl("encoder_train_steps", &encoder_train_steps);
  m.impl("heads_train_steps", &heads_train_steps);
  m.impl("pose_eval", &pose_eval);
  m.impl("pose_eval_merge", &pose_eval_merge);
  m.impl("mode_gram", &mode_gram);
  m.impl("pose_grams", &pose_grams);
  m.impl("project_identity", &project_identity);
  m.impl("project_pose", &project_pose);
  m.impl("tucker_residual", &tucker_residual);
}

TORCH_LIBRARY_IMPL(nlml_hpe, Meta, m) {
  m.impl("normalize_ipd", &normalize_ipd_meta);
  m.impl("normalize_centroid", &normalize_centroid_meta);
  m.impl("compose_rotation_tensor", &compose_rotation_tensor_meta);
  m.impl("rotate_landmarks", &rotate_landmarks_meta);
  m.impl("encoder_heads_fwd", &pose_meta<int64_t>);
  m.impl("landmarks_to_pose", &pose_meta<bool>);
  m.impl("encoder_heads_fwd_small", &pose_meta<int64_t, const at::Tensor&>);
  m.impl("landmarks_to_pose_small", &pose_meta<bool, const at::Tensor&>);
  m.impl("tucker_objective", &tucker_objective_meta);
  m.impl("landmarks_to_pose_valid", &pose_valid_meta);
  m.impl("tucker_gradient", &tucker_gradient_meta);
  m.impl("tucker_powell", &tucker_powell_meta);
  m.impl("video_post", &video_post_meta);
  m.impl("cosine_table", &cosine_table_meta);
  m.impl("cosine_fit", &cosine_fit_meta);
  m.impl("encoder_train_steps", &encoder_train_steps_meta);
  m.impl("heads_train_steps", &heads_train_steps_meta);
  m.impl("pose_eval", &pose_eval_meta);
  m.impl("pose_eval_merge", &pose_eval_merge_meta);
  m.impl("mode_gram", &mode_gram_meta);
  m.impl("pose_grams", &pose_grams_meta);
  m.impl("project_identity", &project_identity_meta);
  m.impl("project_pose", &project_pose_meta);
  m.impl("tucker_residual", &tucker_residual_meta);
}
