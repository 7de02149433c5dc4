/*
 * nlml_hpe.h -- C ABI of libnlml_hpe_hip.so: the MI355X (gfx950) implementation of the
 * NLML_HPE batched-inference hot path.
 *
 * The reference (MahdiGhafoorian/NLML_HPE) is pure Python on stock ATen / numpy and has no
 * FFI of its own; each entry point below names the reference call it replaces (file:line
 * under /root/reference) so a maintainer can bind it from the same place (ctypes stubs in
 * INTEGRATION.md).  Conventions for every function:
 *
 *   - plain pointers and sizes only; all data pointers are DEVICE pointers unless the
 *     parameter name starts with "h_" (host);
 *   - the caller owns every buffer; nothing is allocated or freed inside a launch function;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); launches are
 *     asynchronous on it and may be captured into a hipGraph;
 *   - return value 0 on success, otherwise a negative NLML_E_* code or a positive
 *     hipError_t; nlml_last_error() returns a thread-local message for the last failure;
 *   - thread-safe for distinct streams; no global mutable state.
 */
#ifndef NLML_HPE_H
#define NLML_HPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLML_ABI_VERSION 2   /* 2: the TD entry points without _ex default to NLML_TD_ORDER_REFERENCE */

#define NLML_E_BADARG   (-1)  /* null pointer, negative size, misaligned buffer           */
#define NLML_E_BADBLOB  (-2)  /* packed weight blob has wrong magic / version / F         */
#define NLML_E_SHAPE    (-3)  /* architecture other than the reference's (see pack)      */

/* Fixed architecture constants of the reference model. */
#define NLML_NUM_LANDMARKS 468   /* helpers/FeatureExtractor.py:106                      */
#define NLML_F_REFERENCE   1404  /* configs/config_EncoderTrainer.yaml:19                */
#define NLML_LATENT        9     /* 3 x (1,3) matrices, NLML_HPE_Model_Builder.py:187-195 */
#define NLML_TUCKER_Q      135   /* 5*3*3*3 rows of W, TD_main.py:232-238                */

int         nlml_abi_version(void);
const char* nlml_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1  IPD landmark normalisation.
 * Replaces Read_Landmarks_and_Normalizing_using_IPD (helpers/FeatureExtractor.py:30-66) plus
 * the f32 cast of its callers (:101,:142,:187), batched over faces.
 *   raw      f32[B,468,3]  FaceMesh coordinates (x,y,z interleaved)
 *   normalize != 0: out = f32( (f64(v) - f64(raw[1][c])) / ipd ),  ipd = ||raw[33]-raw[263]||
 *                   in f64, replaced by 1e-6 when exactly 0 (:47-48); == 0: out = raw.
 *   out      f32[B,1404]
 *   valid    u8[B] or NULL: 0 where the OUTPUT row is all zero -- the reference's "no face"
 *            sentinel (FeatureExtractor.py:105-106; callers skip: NLML_HPE_Test.py:257-260).
 * Bit-exact with the reference (f64 subtract and divide, one rounding to f32).
 */
int nlml_normalize_ipd(const float* raw, int64_t B, int normalize,
                       float* out, uint8_t* valid, void* stream);

/* ------------------------------------------------------------------------------------------
 * K1c  Landmark normalisation by centroid and RMS radius: the reference's OTHER normalisation.
 * Replaces Normalization_using_Centroid (helpers/FeatureExtractor.py:17-28), which get_feature_vector*
 * offer as the alternative to the IPD form (:86-98), plus the f32 cast of its callers (:101).
 *   raw      f32[B,468,3]
 *   out      f32[B,1404]
 *   valid    u8[B] or NULL: 0 where the RAW row is all zero (+0 or -0) -- the extractor's "no face"
 *            sentinel (:105-106); that row's output is all zero (the bare function would give NaN;
 *            the zero row is what get_feature_vector returns).  1 for every other row.
 *   stats    f64[B,4] or NULL: centroid x, y, z and the scale (0, 0, 0, 0 for a sentinel row)
 * The contract is the operation order, numpy's own, per face, with a[i][c] = (double)raw[i][c]:
 *   1. sum_c = ((0.0 + a[0][c]) + a[1][c]) + ... + a[467][c], sequentially;  centroid_c = sum_c / 468.0
 *   2. d[i][c] = a[i][c] - centroid_c;  q[i][c] = d[i][c] * d[i][c], each rounded on its own (no fma)
 *   3. n[i] = (q[i][0] + q[i][1]) + q[i][2]
 *   4. m = pairwise(n[0..467]) / 468.0 with numpy's pairwise sum: 468 -> 232 + 236 -> (112 + 120) +
 *      (112 + 124); a leaf has eight accumulators seeded from its first eight elements, strides by 8,
 *      combines as ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)) and adds the remainder sequentially
 *   5. s = sqrt(m), correctly rounded;  out[i][c] = (float)(d[i][c] / s): an IEEE f64 divide, one
 *      rounding to f32
 * Identical landmarks give 0/0 = NaN as numpy does; NaN and Inf inputs propagate.  Bit-exact with the
 * reference.  Errors and alignment as nlml_normalize_ipd (raw / out 16-byte aligned); stats 8-byte aligned.
 *
 * nlml_normalize_centroid_host evaluates the same order on HOST buffers in plain C++ (no HIP call, no
 * alignment rule): the order can be pinned on a machine without a GPU.
 */
int nlml_normalize_centroid(const float* raw, int64_t B, float* out, uint8_t* valid, double* stats, void* stream);
int nlml_normalize_centroid_host(const float* h_raw, int64_t B, float* h_out, uint8_t* h_valid, double* h_stats);

/* ------------------------------------------------------------------------------------------
 * K6  Landmarks at a known pose: the rotation training tensor, and one pose per face.
 * Replaces the rotation branch of CreateTensor.Compose_Tensor (CreateTensor.py:96-114, use_rotation_features=1, the
 * default source of the training tensor, TD_main.py:58) and helpers/IntrinsicRotation.apply_rotations
 * (IntrinsicRotation.py:108-120).  No trigonometry runs on the device: the 3x3 f64 matrices are inputs, built on
 * the host as rotation_matrix builds them (IntrinsicRotation.py:90-105).
 *
 * The contract is the operation order, numpy's own for a [468,3] block, with a[i] = (double)lm[i][.]:
 *   1. a stage is b = a @ M:  b[j] = fma(a[2], M[2][j], fma(a[1], M[1][j], fma(a[0], M[0][j], +0.0))).  The
 *      accumulator starts at +0.0 and the first term is an fma too: a product that is -0.0 gives +0.0.
 *   2. a pose is three stages, every stage's outputs rounded to f64 before the next:
 *        NLML_ROT_INTRINSIC   ((L @ Rx(pitch)) @ Ry(yaw)) @ Rz(roll)            stages pitch, yaw, roll
 *        NLML_ROT_EXTRINSIC   ((L @ Rz(roll)^T) @ Ry(yaw)^T) @ Rx(pitch)^T      stages roll, yaw, pitch; the CALLER
 *                             passes the transposed matrices
 *   3. out = (float)(third stage): one rounding to f32 (CreateTensor.py:110);  out64 = the third stage itself.
 *   4. copy rule (grid mode only, CreateTensor.py:97-98): the cell whose three bins are the zero bins is the base
 *      landmarks bit for bit (a -0.0 coordinate stays -0.0; rotating by identity matrices would give +0.0); its
 *      out64 is the same values widened.
 * NaN and Inf inputs propagate as in numpy.  Bit-exact with the reference.
 *
 * nlml_compose_rotation_tensor (grid mode):
 *   base      f32[I,468,3]   the pose-(0,0,0) landmarks per identity
 *   rot_yaw   f64[ny,3,3], rot_pitch f64[np,3,3], rot_roll f64[nr,3,3]   one matrix per bin, row-major
 *   order     NLML_ROT_INTRINSIC or NLML_ROT_EXTRINSIC
 *   zero_yaw, zero_pitch, zero_roll   index of the bin whose value is 0 on that axis, or -1 (no copy)
 *   out       f32[I,ny,np,nr,1404]   the reference's composition_tensor[id, yaw, pitch, roll, :], x,y,z interleaved
 *   out64     f64[I,ny,np,nr,1404] or NULL
 * nlml_rotate_landmarks (one pose per face, apply_rotations itself, no copy rule):
 *   lm        f32[B,468,3]
 *   rot       f64[B,3,3,3]   each face's three matrices in application order
 *   out       f32[B,468,3] or NULL;  out64 f64[B,468,3] or NULL;  at least one of them
 * Checks, in this order, before any launch:
 *   1. a required buffer is NULL (required: while no extent is 0)          -> NLML_E_BADARG
 *   2. a negative extent                                                    -> NLML_E_BADARG
 *   3. an unknown `order`                                                   -> NLML_E_BADARG
 *   4. a zero_* outside -1 .. n-1                                           -> NLML_E_BADARG
 *   5. I, ny, np, nr or B of 0                                              -> 0, no launch, no buffer looked at
 *   6. alignment as nlml_normalize_centroid: f32 buffers 16-byte, f64 buffers 8-byte aligned;
 *      a tensor of more than INT64_MAX elements                            -> NLML_E_BADARG
 * All row and byte offsets are 64-bit.
 *
 * The *_host forms evaluate the same order on HOST buffers in plain C++ (no HIP call, no alignment rule, h_out may
 * be NULL where h_out64 is given): the order can be pinned on a machine without a GPU.
 */
#define NLML_ROT_INTRINSIC 0
#define NLML_ROT_EXTRINSIC 1
int nlml_compose_rotation_tensor(const float* base, int64_t I, const double* rot_yaw, int ny, const double* rot_pitch, int np,
                                 const double* rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll,
                                 float* out, double* out64, void* stream);
int nlml_rotate_landmarks(const float* lm, const double* rot, float* out, double* out64, int64_t B, void* stream);
int nlml_compose_rotation_tensor_host(const float* h_base, int64_t I, const double* h_rot_yaw, int ny, const double* h_rot_pitch, int np,
                                      const double* h_rot_roll, int nr, int order, int zero_yaw, int zero_pitch, int zero_roll,
                                      float* h_out, double* h_out64);
int nlml_rotate_landmarks_host(const float* h_lm, const double* h_rot, float* h_out, double* h_out64, int64_t B);

/* ------------------------------------------------------------------------------------------
 * K2  Encoder + three heads, fused forward.
 * Replaces CombinedAnglePredictionModel.forward (NLML_HPE_Model_Builder.py:115-126), i.e.
 * LandmarkEncoder.forward (:55-68) and 3 x AnglePredictionNetwork.forward (:104-105), called
 * as model(x) at NLML_HPE_Test.py:272 / generatePose_on_video.py:209.
 *
 * Weights are packed ONCE on the host into the kernel's MFMA fragment order:
 *   enc_w[i]/enc_b[i], i<6 : encoder.{0,2,4,6,8,10}.{weight,bias}, weight [out,in] row-major
 *                            with shapes (1024,F) (512,1024) (256,512) (128,256) (64,128) (9,64)
 *   head_w[g][i]/head_b[g][i], g<3 (yaw,pitch,roll), i<5 : model.{0,2,4,6,8}.{weight,bias},
 *                            shapes (128,3) (256,128) (128,256) (64,128) (1,64)
 * (the state-dict layout of models/Encoder.pth and models/{yaw,pitch,roll}_network.pth).
 * mode: NLML_MODE_F32 = f32 storage + f32 MFMA, layers 0 to 3 summed in blocks of 128 k (the strict parity mode: at the
 *       reference's operating range -- poses to +-60 deg, FX3c, 16,384 faces -- its distance from the exact result is
 *       1.25e-5 / 4.0e-5 / 8.7e-5 deg in p50 / p99 / max, no worse than the reference's own 1.7e-5 / 5.5e-5 / 9.9e-5);
 *       NLML_MODE_BF16 = bf16 weights and activations + bf16 MFMA, f32 accumulate (throughput mode:
 *       ~5x the faces/s; its error is ~0.1 deg max / 0.02 deg mean and is never claimed as parity);
 *       NLML_MODE_F16X2 = split-f16 mode, OPT-IN, 1.10x THE REFERENCE'S ERROR: every f32 weight and activation is carried as two f16
 *       pieces (hi + lo, 22 significand bits) and a product runs as three f16 MFMAs with f32 accumulation.
 *       ~1e-5 deg from the reference on small poses; at the reference's operating range (FX3c) 1.86e-5 / 5.9e-5 / 1.22e-4 deg
 *       from the exact result in p50 / p99 / max = 1.10 / 1.08 / 1.24x the reference's own distance, 0.024 % of the faces beyond 1e-4
 *       deg; ~3x NLML_MODE_F32's faces/s (the default of this build's host layer until round 3; NLML_MODE_F16X2S since).  No input-range limit: a
 *       face whose activations leave f16's range (|v| >= 65520 -- e.g. the reference's ipd == 0 -> 1e-6 branch,
 *       FeatureExtractor.py:47-48) is re-evaluated inside the same launch in f32 on the vector ALUs from the same
 *       blob (csrc/encoder_heads_f16x2_rescue.h); NaN/Inf inputs give a non-finite pose, as in the reference.
 *       COST OF THAT SLOW PATH: rescued faces go four at a time, each group streaming the whole 9.6 MB blob through its CU
 *       (~0.15 ms).  A handful of such faces per launch is free; a batch in which EVERY face overflows (un-normalised
 *       pixel-scale landmarks against trained-scale weights) runs ~40x slower: 6.1 ms instead of 0.16 ms for 4,096 faces
 *       (0.67 M faces/s; tests/test_gpu_parity.py::test_split_f16_every_face_of_a_tile_overflows).  Feed such data to
 *       NLML_MODE_F32, which has no range limit and no cliff.  Rescued faces use the blob's weights as hi + lo, i.e. 22
 *       significand bits, not the original f32 weights: ~2x torch-f32's distance from the exact result on such inputs.
 *       NLML_MODE_F16X2S = the same operands and the same three MFMAs per product, but the two SMALL products of a K step
 *       (w_lo*x_hi, w_hi*x_lo) accumulate in registers of their own in layers 0 to 2 and join the big sum once per K
 *       block: the matrix instruction truncates its products to the running sum's exponent, which is what costs
 *       NLML_MODE_F16X2 its distance (profiles/r03_mfma_f16_numerics_probe.txt; that mode has room for the second accumulator set only from
 *       layer 1's second K half on).  THE DEFAULT of the host layer.  Parity at the operating range (FX3c, 16,384 faces): 1.50e-5 /
 *       4.65e-5 / 9.2e-5 deg from the exact result = 0.88 / 0.85 / 0.93x the PINNED reference's own distance (fixture generated in the
 *       build container) but 1.14 / 1.12 / 1.10x torch-f32's on the GPU box's host (1,048,576 faces, profiles/r04_parity_soak_1M.json:
 *       the reference's distance depends on its host's GEMM blocking); 0.03-0.07 % of the faces differ from the reference's batched
 *       OUTPUT by more than 1e-4 deg (NLML_MODE_F32: 0.002-0.012 %, what the reference shows against itself): the looser of the two
 *       parity-class modes -- NLML_MODE_F32 is the one to use where 1e-4 deg must hold face by face.  ~0.9x NLML_MODE_F16X2's faces/s (an eight-wave kernel,
 *       csrc/encoder_heads_f16x2_w8.hip; layer 0 runs in two passes over x to make room for the second accumulator set).
 *       Packed image: NLML_MODE_F16X2's, 256 bytes, then a complete NLML_MODE_F32 image (the size still names the mode).
 *       Range behaviour: a tile with faces beyond f16's range is re-evaluated whole on the f32 matrix cores from the f32 image by a
 *       second launch that the forward entry points enqueue behind the kernel (csrc/encoder_heads.hip, re-evaluation mode; it ends at
 *       once for every other tile; only the out-of-range faces are written): the strict parity kernel's bits on those faces, and a
 *       batch in which EVERY face overflows runs 3x slower, not 40x.
 * The forward entry points recognise the mode of a blob by its size.
 */
#define NLML_MODE_F32   0
#define NLML_MODE_BF16  1
#define NLML_MODE_F16X2 2
#define NLML_MODE_F16X2S 3

size_t nlml_encoder_heads_packed_bytes(int F, int mode);
int    nlml_encoder_heads_pack(int F, int mode,
                               const float* const h_enc_w[6], const float* const h_enc_b[6],
                               const float* const h_head_w[3][5], const float* const h_head_b[3][5],
                               void* h_blob, size_t blob_bytes);

/*   x       f32[B,F], row stride ldx floats (ldx >= F)
 *   blob    device copy of the packed blob (16-byte aligned)
 *   out     f32[B,3]  (yaw, pitch, roll) in RADIANS -- the three [B,1] outputs of the
 *           reference side by side (rad->deg is left to the caller, Model_Builder.py:125)
 *   latent  f32[B,9] or NULL: the encoder output before the split (:58)
 *   valid   u8[B] or NULL: 0 where the input row is all zero -- the "no face" sentinel the
 *           reference's callers test per face (NLML_HPE_Test.py:257-260); the pose is still
 *           computed for such rows, as the reference's forward would.
 */
int nlml_encoder_heads_fwd(const float* x, int64_t ldx, int64_t B, int F,
                           const void* blob, size_t blob_bytes,
                           float* out, float* latent, uint8_t* valid, void* stream);

/* Diagnostic build of nlml_encoder_heads_fwd (x 16-byte aligned, F % 4 == 0).  It also writes
 *   pre_tanh f32[B,64] (or NULL): the Linear(128,64) outputs BEFORE the Tanh (Model_Builder.py:49-50);
 *            everything up to there is pure f32 fma, so it is compared bit for bit against the C
 *            oracle's fmaf chain (tests/test_gpu_parity.py);
 *   stamps   u64[ceil(B/64),4,16] (or NULL): per-wave s_memtime at the stage boundaries, for the
 *            cycle-share breakdown in profiles/ (never a run-time figure). */
int nlml_encoder_heads_fwd_debug(const float* x, int64_t ldx, int64_t B, int F,
                                 const void* blob, size_t blob_bytes,
                                 float* out, float* latent, float* pre_tanh,
                                 unsigned long long* stamps, void* stream);

/* Fused K1+K2: raw landmarks in, pose out; the normalised features never touch HBM.
 *   raw f32[B,468,3]; valid u8[B] or NULL as in nlml_normalize_ipd. F must be 1404. */
int nlml_landmarks_to_pose(const float* raw, int64_t B, int normalize,
                           const void* blob, size_t blob_bytes,
                           float* out, float* latent, uint8_t* valid, void* stream);

/* The same forward for SMALL batches in NLML_MODE_F16X2 / NLML_MODE_F16X2S: the three big layers as one launch each over (neuron blocks x
 * 64-face tiles) plus one launch for the tail, instead of one CU per tile, so 64 or 2,000 faces use the whole chip (a
 * 64-face video tick: 0.06 ms instead of 0.17 ms); the results are bit-identical to nlml_encoder_heads_fwd / nlml_landmarks_to_pose with the same blob.
 * Activations pass between the launches through `workspace` (device memory, 16-byte aligned, at least
 * nlml_encoder_heads_small_workspace_bytes(B, F) bytes, contents irrelevant before and after); stream order is the only
 * synchronisation, so the sequence can be captured into a hipGraph.  Above ~4,500 faces the fused entry points are faster.
 */
size_t nlml_encoder_heads_small_workspace_bytes(int64_t B, int F);
int nlml_encoder_heads_fwd_small(const float* x, int64_t ldx, int64_t B, int F,
                                 const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                 void* workspace, size_t ws_bytes, void* stream);
int nlml_landmarks_to_pose_small(const float* raw, int64_t B, int normalize,
                                 const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                 void* workspace, size_t ws_bytes, void* stream);

/* The same forward in NLML_MODE_F16X2S as TRUNK LAUNCH + STREAMED TAIL LAUNCH (+ the f32 re-evaluation launch): layers 0-2 by the
 * eight-wave kernel, which ends with layer 2's output in `workspace` as MFMA operand fragments (1 KB per face), then layers E3..E5 and
 * the three heads (NLML_HPE_Model_Builder.py:45-53,76-92) by a kernel in which a wave keeps a 32-face block's activations in registers
 * through the whole tail while the tail's 1.06 MB of weights pass through LDS once per 256 faces (csrc/encoder_heads_f16x2_tailws.hip)
 * -- in the fused kernel they stream once per 64 faces through thirteen barrier-separated stages on half the CU's waves.
 * MEASURED 1.4-2.2 % faster than the fused kernel at 65,536 faces (0.801 against 0.815 ms, same box; the trunk launch alone costs 0.90 of the
 * fused kernel = its share of the L2 -> CU bytes; below ~60,000 faces the path LOSES: -5 % at 32,768, -16 % at 16,384): inside
 * the box-to-box spread, so nothing picks it by default
 * (NLML_K2_STREAMED_MIN=<faces> makes the _ws entry points route batches from that size on through it).
 * Bit-identical to nlml_encoder_heads_fwd / nlml_landmarks_to_pose with the same blob.  Input layout: F % 4 == 0, rows 16-byte aligned
 * (ldx % 4 == 0) -- else NLML_E_BADARG.  `workspace`: nlml_encoder_heads_workspace_bytes(B, F) bytes, 16-byte aligned.
 */
int nlml_encoder_heads_fwd_streamed(const float* x, int64_t ldx, int64_t B, int F,
                                    const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                    void* workspace, size_t ws_bytes, void* stream);
int nlml_landmarks_to_pose_streamed(const float* raw, int64_t B, int normalize,
                                    const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                    void* workspace, size_t ws_bytes, void* stream);

/* The same forward in NLML_MODE_F16X2S with FOUR TILES PER WORKGROUP in ONE launch (+ the f32 re-evaluation launch): a workgroup runs
 * the eight-wave kernel's layers 0-2 over four 64-face tiles one after the other, parks each tile's layer-2 output in its own slice of
 * `workspace` (the _streamed form's fragments, 1 KB per face; written and read back by that workgroup alone), then runs the _streamed
 * form's tail once over its 256 faces (csrc/encoder_heads_f16x2_w8.hip, encoder_heads_f16x2_w8q_kernel).  No workgroup waits for another.
 * Bit-identical to nlml_encoder_heads_fwd / nlml_landmarks_to_pose with the same blob; any B >= 0; the _streamed forms' input layout,
 * workspace (nlml_encoder_heads_workspace_bytes(B, F) covers it: the hand-over is the same 1 KB per face of whole 64-face tiles) and
 * refusals (NLML_E_BADARG for a blob of another mode, a small or misaligned workspace, rows that cannot be read 16 bytes at a time).
 * Measurements and what picks it: DESIGN.md section 3.
 */
int nlml_encoder_heads_fwd_quad(const float* x, int64_t ldx, int64_t B, int F,
                                const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                void* workspace, size_t ws_bytes, void* stream);
int nlml_landmarks_to_pose_quad(const float* raw, int64_t B, int normalize,
                                const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                                void* workspace, size_t ws_bytes, void* stream);
/* The _ws entry points' split of a strict-fast batch: *quad_faces = the leading faces that go through the four-tile kernel on a device
 * of `cus` compute units -- whole rounds of one 256-face workgroup per unit, ((B / 64) / (4 cus)) * cus * 256 -- the others go through
 * the fused kernel.  Host arithmetic, no HIP call.  B < 0, cus <= 0 or a NULL quad_faces: NLML_E_BADARG (and *quad_faces = 0).
 */
int nlml_k2_quad_split(int64_t B, int cus, int64_t* quad_faces);
/* The part of a batch of B rows that nlml_encoder_heads_fwd_ws / nlml_landmarks_to_pose_ws send through the four-tile kernel on the
 * calling thread's current device when the workspace holds it, and the bytes of workspace that part needs.  rows / ld: x and ldx, or raw
 * and 1404 (B == 1: ld = F); rows is looked at for its alignment only and never read.  blob_bytes names the blob's mode as in the
 * forwards; a size that is no strict-fast blob of width F gives 0 faces and rc 0 (the forward itself refuses a bad blob).
 * ws_bytes may be NULL.  B < 0, F <= 0 or quad_faces NULL: NLML_E_BADARG, outputs zeroed.
 * The dispatcher's own rule (one function in csrc/abi.cpp), under this process's environment (NLML_K2_QUAD_MIN, NLML_K2_STREAMED_MIN:
 * below; NLML_K2_QUAD_CUS=<n> stands in for the device's compute-unit count, and then no HIP call is made) -- what a host asks to learn
 * whether a workspace is worth allocating. */
int nlml_k2_quad_part(const float* rows, int64_t ld, int64_t B, int F, size_t blob_bytes, int64_t* quad_faces, size_t* ws_bytes);
/* nlml_k2_quad_part for 16-byte aligned rows of the reference width and a strict-fast blob: the same function, evaluated for that input. */
int nlml_k2_quad_faces(int64_t B, int64_t* quad_faces, size_t* ws_bytes);
/* Largest batch the _ws dispatcher sends through the layer-per-launch path for a blob of `mode`; 0 for a mode without that path or an
 * unknown mode. */
int64_t nlml_k2_small_batch_max(int mode);

/* THE FORWARD WITH A WORKSPACE: picks the fastest of the paths above for the batch size and the blob's mode (split-f16 modes: the
 * layer-per-launch path up to 4,096 faces; the fused kernel otherwise and for the other modes, which ignore the workspace; the
 * trunk + streamed-tail path only when the environment asks for it, NLML_K2_STREAMED_MIN=<faces>).  A strict-fast batch with rows readable
 * 16 bytes at a time is split (nlml_k2_quad_split with the device's compute-unit count, asked once per device): the leading whole rounds
 * through the four-tile kernel, the rest through the fused kernel on offset pointers in the same stream, one re-evaluation launch over
 * all B -- if the workspace holds the quad part's hand-over (1 KB per face); with a smaller workspace the call does what it did without
 * the path, so it never fails for want of workspace where the fused kernel would run.  NLML_K2_QUAD_MIN=<faces> (read once): negative
 * switches the path off; otherwise the rule becomes "B >= faces: the whole batch through the four-tile kernel" (then a small workspace
 * IS refused).  NLML_K2_STREAMED_MIN wins where both apply.  Same bits whichever path runs.  For hosts that
 * want one call for every batch size; the packaged host layer asks the library instead of choosing for itself: the _small forms up to
 * nlml_k2_small_batch_max(mode) faces (nlml_hpe_amd/model.py), the _ws form where nlml_k2_quad_part says a quad part exists, the plain
 * forms otherwise -- which is what bench.py times.
 * The plain entry points (nlml_encoder_heads_fwd, nlml_landmarks_to_pose) have no workspace argument, cannot take the four-tile path and
 * stay on the fused kernel.
 * `workspace`: at least nlml_encoder_heads_workspace_bytes(B, F) bytes (>= the _small, _streamed and _quad paths' needs), 16-byte aligned.
 */
size_t nlml_encoder_heads_workspace_bytes(int64_t B, int F);
int nlml_encoder_heads_fwd_ws(const float* x, int64_t ldx, int64_t B, int F,
                              const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                              void* workspace, size_t ws_bytes, void* stream);
int nlml_landmarks_to_pose_ws(const float* raw, int64_t B, int normalize,
                              const void* blob, size_t blob_bytes, float* out, float* latent, uint8_t* valid,
                              void* workspace, size_t ws_bytes, void* stream);

/* K2 ARGUMENT CHECKS.  Every K2 forward entry point (the ten above and nlml_encoder_heads_fwd_debug) checks its arguments in this order
 * and returns at the first that fails, before any launch; a host may rely on which of two errors it gets:
 *   1. nlml_landmarks_to_pose_ws only: B > 0 and raw NULL -> NLML_E_BADARG (every other form reports a missing input at 4)
 *   2. the blob: B < 0 or F <= 0 -> NLML_E_BADARG;  B > 0 and blob or out NULL -> NLML_E_BADARG;  blob not 16-byte aligned ->
 *      NLML_E_BADARG;  blob_bytes not the size of a blob of width F in any mode -> NLML_E_BADBLOB  (the last two at B == 0 as well)
 *   3. the form's mode: _small takes NLML_MODE_F16X2 and NLML_MODE_F16X2S blobs, _streamed and _quad NLML_MODE_F16X2S, _debug
 *      NLML_MODE_F32; another -> NLML_E_BADARG (at B == 0 as well)
 *   4. B > 0 and the input missing (raw NULL; x NULL or ldx < F) -> NLML_E_BADARG
 *   5. B == 0 -> 0: no launch, and neither the input nor the workspace is looked at (a NULL workspace is fine)
 *   6. the workspace of the path that runs -- the form's own; for _ws the one its rule above picks, which is the four-tile path only
 *      where the workspace holds the quad part, unless NLML_K2_QUAD_MIN is set: NULL or fewer bytes than that path needs ->
 *      NLML_E_BADARG; then not 16-byte aligned -> NLML_E_BADARG.  The fused kernels need none.
 *   7. the streamed and the four-tile path: rows that cannot be read 16 bytes at a time (x or raw 16-byte aligned, F % 4 == 0,
 *      ldx % 4 == 0) -> NLML_E_BADARG; _ws never picks these paths for such rows.  _debug with pre_tanh or stamps given: the same
 *      condition -> NLML_E_BADARG.  The other paths read rows of any 4-byte alignment.
 * nlml_last_error() names the path ("small-batch path", "streamed-tail path", "quad path", "debug build") or the function family and
 * the condition.  (tests/test_k2_abi_contract_host.py)
 */

/* ------------------------------------------------------------------------------------------
 * K3  Tucker objective, batched over face-evaluations.
 * Replaces objective() (TD_Tester.py:31-58): f = a*cos(b*w+c)+d (:25-28) in f64 rounded to
 * f32 (:37,40,43); x_hat = einsum('ijklm,i,j,k,l->m', W, u, f_y, f_p, f_r) in f64 (:46);
 * err = 0.5*sum((x-x_hat)^2) (:49).
 *   Wm         f32[135,1404]  = W.reshape(-1,1404) of outputs/features/Trained_data.npz
 *   x          f32[N,1404]    feature rows, row stride ldx
 *   x_index    i32[N] or NULL: evaluation n uses row x_index[n] of x (several evaluations of
 *              one face share its row); NULL = row n
 *   params     f64[N,8]       (w_y, w_p, w_r, u_id[5]) per evaluation (TD_Tester.py:32-33)
 *   cos_params f64[3,3,4]     optimized_{yaw,pitch,roll}[0:3,:] rows (a,b,c,d) (TD_Inference.py:56)
 *   err        f64[N]
 *   x_hat      f64[N,1404] or NULL
 *
 * OPERATION ORDER.  The reference's objective is a fixed sequence of separately rounded f64 operations, and the Powell
 * minimisation on top of it is sensitive to its last bits (the minimum is flat), so the order is part of the contract:
 *   NLML_TD_ORDER_REFERENCE  (the default of the entry points without _ex: the PARITY mode)
 *       np.einsum('ijklm,i,j,k,l->m')'s own loop -- for (i,j,k,l) in nesting order and every m,
 *       x_hat[m] = ((((W*u_i)*f_yj)*f_pk)*f_rl) + x_hat[m], each operation rounded on its own -- and numpy's pairwise np.sum
 *       (TD_Tester.py:46,49): err and x_hat are BIT-IDENTICAL to the reference's (FX4).  Vector ALUs, 5 operations per (q, m).
 *       Alignment: Wm and x 4-byte aligned, any ldx >= 1404.
 *   NLML_TD_ORDER_FAST       (opt-in)
 *       x_hat = c^T Wm with c = ((u*f_y)*f_p)*f_r as a GEMM on the f64 matrix cores, one fma chain per output; agrees with the
 *       reference's objective to <= 1e-12 relative (measured ~2e-16), ~5x the evaluations/s.
 *       Alignment: Wm and x 16-byte aligned and ldx % 4 == 0 (16-byte vector loads), else NLML_E_BADARG.
 *
 * TD ARGUMENT CHECKS.  Every TD entry point (objective, Powell and gradient, of every generation) checks its arguments in this order
 * and returns at the first that fails, before any launch; a host may rely on which of two errors it gets:
 *   1. r_id outside NLML_TUCKER_RANK_MIN..NLML_TUCKER_RANK_MAX -> NLML_E_SHAPE (the entry points that take a rank)
 *   2. unknown order -> NLML_E_BADARG (the entry points that take an order)
 *   3. N < 0 -> NLML_E_BADARG;  N == 0 -> 0: no launch, no buffer is looked at
 *   4. a required buffer NULL -> NLML_E_BADARG (objective: Wm, x, params, cos_params, err; Powell: Wm, x, cos_params, result;
 *      gradient: Wm, x, params, cos_params, grad)
 *   5. ldx < 1404 -> NLML_E_BADARG
 *   6. NLML_TD_ORDER_FAST and its alignment rule broken -> NLML_E_BADARG
 * nlml_last_error() names the entry point family and the condition.
 */
#define NLML_TD_ORDER_FAST      0
#define NLML_TD_ORDER_REFERENCE 1
int nlml_tucker_objective(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index,
                          const double* params, const double* cos_params, int64_t N,
                          double* err, double* x_hat, void* stream);          /* == _ex(..., NLML_TD_ORDER_REFERENCE, stream) */
int nlml_tucker_objective_ex(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index,
                             const double* params, const double* cos_params, int64_t N,
                             double* err, double* x_hat, int order, void* stream);

/* ------------------------------------------------------------------------------------------
 * TD end-to-end: batched, lock-step Powell minimisation of the K3 objective, entirely on device.
 * Replaces Test() (TD_Tester.py:162-199): scipy.optimize.minimize(objective, zeros(8),
 * method='Powell') with scipy's defaults (xtol = ftol = 1e-4, maxiter = maxfev = 8000), one
 * independent minimisation per face; the reference spends 2-4 s per face in it.
 *   Wm, cos_params  as for nlml_tucker_objective
 *   x        f32[N,1404] one feature row per face, row stride ldx
 *   x0       f64[N,8] starting points or NULL for zeros (TD_Tester.py:166)
 *   result   f64[N,8]  minimiser (w_y, w_p, w_r in RADIANS, u_id[5]); degrees are the caller's
 *            np.degrees(result.x)[:3] (:196-199)
 *   fval f64[N], nfev i32[N], nit i32[N], status i32[N] (1 converged, 2 maxfev, 3 maxiter, 4 nan):
 *            scipy's res.fun / res.nfev / res.nit; each may be NULL.
 * NON-FINITE FEATURES OR STARTS (n = the number of parameters, 8 here): what scipy returns for them, never an error.
 *   a NaN feature, or a NaN / Inf in x0: the objective is NaN everywhere -> status 4 after 1 + 3 n evaluations and one iteration,
 *       result and fval NaN;
 *   an Inf feature: the objective is +inf everywhere -> status 2 after exactly 1000 n evaluations, result = x0, fval = +inf.  Such
 *       a face keeps its workgroup, and with it the launch, busy for all 1000 n rounds (0.1-0.3 s on an MI355X): filter such faces out
 *       first where that matters;
 *   an all-zero row (the "no face" sentinel) from x0 = NULL converges in the first iteration: status 1, result = 0, fval = 0.
 * Status 3 cannot occur with the fixed limits maxiter = maxfev = 1000 n: an iteration costs at least n evaluations, so maxfev comes
 * first.  Status 0 is never written.  (tests/test_td_powell_edges_gpu.py)
 * The control flow is scipy 1.15.3's (restated in nlml_hpe_amd/csrc/powell.h, checked against scipy step for step on the CPU).
 *   NLML_TD_ORDER_REFERENCE (default, parity mode): every machine receives the reference's objective values bit for bit, so it
 *       walks scipy's own trajectory: same evaluation counts, same final angles (FX5: identical bits; 1e-4 deg is the bar).
 *       (Up to the cos() of the f-vectors: the device's f64 cos and the host libm's may differ in the last place, which can flip the
 *       f32 rounding of an f-vector entry about once per 1e8 values -- tests/test_gpu_parity.py sweeps 1e6 angles.)
 *   NLML_TD_ORDER_FAST (opt-in, ~3x the faces/s): the same algorithm on the matrix-core objective.  The minimum is flat and
 *       Powell's termination is rounding-sensitive, so the END POINT moves under ANY re-ordering of the objective's sums (scipy
 *       itself: tests/test_powell_sm.py): 6e-3 deg from scipy's on clean grid faces (FX5); on BASELINE config 3's 4,096 noisy
 *       grid faces median 1.8e-3 deg (per face, largest of the three angles), 10 % of the faces > 0.02 deg, 0.3 % > 1 deg, max 8.7 deg.  Not a parity mode.
 */
int nlml_tucker_powell(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N,
                       const double* x0, double* result, double* fval, int32_t* nfev, int32_t* nit,
                       int32_t* status, void* stream);                         /* == _ex(..., NLML_TD_ORDER_REFERENCE, stream) */
int nlml_tucker_powell_ex(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N,
                          const double* x0, double* result, double* fval, int32_t* nfev, int32_t* nit,
                          int32_t* status, int order, void* stream);

/* ------------------------------------------------------------------------------------------
 * The TD path for ANY Tucker identity rank R (configs/config_TD_main.yaml tensor_decom_ranks.R_identity).  The reference reads the
 * rank from the artefact (TD_Inference.py:51, u_id_shape = factors_data['U_id'][1].size) and runs objective() and Test() with
 * 3 + R parameters whatever it is (TD_Tester.py:31-58,162-199); slicing W to fewer identity components is its own advice
 * (TD_Inference.py:54-55).  The angle ranks stay 3.
 *   r_id       NLML_TUCKER_RANK_MIN..NLML_TUCKER_RANK_MAX
 *   Wm         f32[27 r_id, 1404] = W.reshape(-1, 1404), W f32[r_id,3,3,3,1404]
 *   params, x0, result   f64[N, 3 + r_id]: (w_y, w_p, w_r, u_id[r_id])
 *   everything else, the two orders, their alignment rules and the argument checks: as for nlml_tucker_objective_ex /
 *   nlml_tucker_powell_ex ("TD argument checks" above).
 * scipy's defaults follow the number of parameters: maxiter = maxfev = 1000 (3 + r_id).
 * NLML_TD_ORDER_REFERENCE is bit-identical to the reference's objective and walks scipy's trajectory for every rank (FX10: ranks 1, 3
 * and 8); NLML_TD_ORDER_FAST keeps its <= 1e-12 relative.  r_id == 5 runs the kernels of the entry points above: the same bits.
 */
#define NLML_TUCKER_RANK_MIN 1
#define NLML_TUCKER_RANK_MAX 16
int nlml_tucker_objective_r(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index,
                            const double* params, const double* cos_params, int64_t N,
                            double* err, double* x_hat, int r_id, int order, void* stream);
int nlml_tucker_powell_r(const float* Wm, const float* x, int64_t ldx, const double* cos_params, int64_t N,
                         const double* x0, double* result, double* fval, int32_t* nfev, int32_t* nit,
                         int32_t* status, int r_id, int order, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3g -- objective value AND analytic gradient in one call (TD_Tester.py:60-102, compute_gradient: the jac= the reference hands to
 * scipy.optimize.minimize, :194,253-256), in the reference's own operation order, for r_id = NLML_TUCKER_RANK_MIN..NLML_TUCKER_RANK_MAX:
 *   err   f64[N] or NULL      the bits of nlml_tucker_objective_r(..., NLML_TD_ORDER_REFERENCE)
 *   grad  f64[N, 3 + r_id]    (d/dw_y, d/dw_p, d/dw_r, d/du[r_id]); every component is the reference's, bit for bit:
 *       df = float32(((-a) b) sin(b w + c)) with a correctly rounded sin; the four einsums 'ijklm,i,j,k,l->m' in numpy's generic loop
 *       order; np.sum(r * e) by numpy's pairwise tree; the identity term as the reference writes it (:96-97: the inner einsum
 *       'ijklm,j,k,l->m' runs in f32 and sums over i as well; the outer 'ijklm,m->i' in numpy's buffered two-lane order).
 *       csrc/tucker_grad_ref.h states the order.
 *   workspace   nlml_tucker_gradient_workspace_bytes(N, r_id) bytes of device memory, 8-byte aligned (the chains' rows and r * v; about
 *       56 KB per evaluation); the call leaves nothing in it that a later call needs.
 * Arguments, alignment and the argument checks ("TD argument checks" above) otherwise as for nlml_tucker_objective_r in
 * NLML_TD_ORDER_REFERENCE; then a workspace that is too small, or an f64 buffer or workspace that is not 8-byte aligned ->
 * NLML_E_BADARG.  Two launches on `stream`.
 * nlml_tucker_gradient_host: the same arithmetic on HOST buffers in plain C++ (no GPU involved) -- the restatement the device kernels
 * are held to; h_v f32[N,1404] or NULL receives the f32 einsum of the identity term (for tests). */
size_t nlml_tucker_gradient_workspace_bytes(int64_t N, int r_id);   /* 0 for N <= 0 or an r_id out of range */
int nlml_tucker_gradient_r(const float* Wm, const float* x, int64_t ldx, const int32_t* x_index,
                           const double* params, const double* cos_params, int64_t N,
                           double* err, double* grad, int r_id, void* workspace, size_t workspace_bytes, void* stream);
int nlml_tucker_gradient_host(const float* h_Wm, const float* h_x, int64_t ldx, const int32_t* h_x_index,
                              const double* h_params, const double* h_cos_params, int64_t N,
                              double* h_err, double* h_grad, int r_id, float* h_v);

/* ------------------------------------------------------------------------------------------
 * K4  Video post-processing for S concurrent streams, one frame tick per call.
 * Replaces, per stream (generatePose_on_video.py): round(np.degrees(.), 2) (:211), the exponential
 * smoothing s = alpha*new + (1-alpha)*s seeded by the first prediction (:215-224, alpha 0.4 at :179),
 * and visualize_axes_on_face (:73-124): face centre from landmarks 1/33/263 x frame size, the
 * 100-px jump gate, and the three axis end points (size 80).
 *   pose_rad  f32[S,3]      this tick's model output (radians)
 *   raw       f32[S,468,3]  this tick's FaceMesh landmarks (only 1, 33, 263 are read)
 *   valid     u8[S] or NULL 0 = no face in this stream's frame: state and outputs untouched (:193-196); a stream whose
 *                           pose_rad holds NaN/Inf is skipped the same way (the reference would raise at :121)
 *   state     f64[S,6]      persistent: smoothed yaw/pitch/roll, previous centre x/y, prediction count;
 *                           zero-initialise before the first tick
 *   smoothed  f64[S,3] degrees; centre f64[S,2] pixels; endpoints f64[S,3,2] pixels (x,y of the red,
 *             green, blue axis tips; the reference draws int() of them)
 * Parity: every f64 operation is rounded on its own in the reference's Python order (no fma contraction), so smoothed, centre and
 * state are the reference's values bit for bit -- for any S, every stream independent of the others -- given that round(x, 2) is
 * rint(x*100)/100 (it is, unless x*100 lies within an ulp of a .5 tie).  The end points go through the device library's sin / cos
 * instead of the host libm's and stay within eps * (26*size + |centre| + 2*size) of the reference's, eps = 2^-52
 * (tests/test_video_post_gpu.py derives it); int() of them agrees unless the value lies that close to an integer.
 */
int nlml_video_post(const float* pose_rad, const float* raw, const uint8_t* valid, int64_t S,
                    double frame_w, double frame_h, double alpha, double max_jump, double size,
                    double* state, double* smoothed, double* centre, double* endpoints, void* stream);
/* The same with   updated  u8[S] or NULL: 1 where this tick was applied to the stream, 0 where it was skipped (no face, or a
 * non-finite pose) and state / smoothed / centre / endpoints still hold the previous tick's values -- what a caller that saves the
 * outputs must record as "no new result" (the reference drops such a frame, generatePose_on_video.py:193-196). */
int nlml_video_post_ex(const float* pose_rad, const float* raw, const uint8_t* valid, int64_t S,
                       double frame_w, double frame_h, double alpha, double max_jump, double size,
                       double* state, double* smoothed, double* centre, double* endpoints, uint8_t* updated, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  Evaluation: the metrics block of the test entry point in one pass over the predictions.
 * Replaces NLML_HPE_Test.py's evaluation (reference :95-152, :252-273): pred = np.round(np.degrees(pose), d), the GT range
 * filter lo <= gt <= hi (inclusive) and the no-face filter, then over the kept faces compute_errors (per-axis MAE,
 * std ddof=1, total MAE, MAEV and the left/down/front vector errors of R = Rx(pitch) Ry(-yaw) Rz(roll)) and the MAE per
 * half-open GT interval [low, high) of compute_interval_mae.  All per-face arithmetic in f64.
 *   pose_rad  f32[B,3] radians (the model's output) -- or -- pred_deg f64[B,3] degrees: exactly one of the two (B = 0: either may be NULL)
 *   valid     u8[B] or NULL (NULL = every row has a face)
 *   gt_deg    f64[B,3] degrees (yaw, pitch, roll)
 *   h_lo, h_hi   f64[3] host: the inclusive GT range per axis
 *   decimals  d >= 0: pred = rint(deg * 10^d) / 10^d (np.round); d < 0: no rounding; at most 15
 *   h_intervals f64[K,2] host (low, high); h_axes i32[K] host (0 yaw, 1 pitch, 2 roll); K <= NLML_POSE_EVAL_MAX_INTERVALS
 *   workspace  nlml_pose_eval_workspace_bytes(B, K) bytes, 8-byte aligned (may be NULL when that is 0)
 *   record_out f64[record_len] or NULL: the merged partial record (what nlml_pose_eval_merge merges across calls or ranks)
 *   result_out f64[result_len]
 *   pred_out f64[B,3] or NULL: pred;  keep_out u8[B] or NULL: the keep mask
 * Record: [kept, no_face, out_of_range, mean e[3], M2 e[3], sum v[3] (left, down, front), (count_k, sum e[a_k]_k) x K].
 * Result: [mae yaw/pitch/roll, mae_total, maev, v left/down/front, std yaw/pitch/roll, kept, no_face, out_of_range,
 *          (count_k, mae_k) x K]; no kept face gives NaN means, one kept face NaN std, a count_k of 0 a NaN mae_k (numpy's f64).
 * Two launches: one record per NLML_POSE_EVAL_FACES_PER_RECORD faces (a constant), then one workgroup merges them in index
 * order (Chan's pairwise merge for mean / M2, plain sums otherwise).  No atomics, no host-to-device copy (the bounds and the
 * intervals travel in the kernel arguments): bit-identical from run to run, and capturable in a hipGraph.
 * nlml_pose_eval_merge merges n records f64[n, record_len] (e.g. one per rank, in rank order) the same way.
 */
#define NLML_POSE_EVAL_MAX_INTERVALS    64
#define NLML_POSE_EVAL_FACES_PER_RECORD 2048
size_t nlml_pose_eval_record_len(int n_intervals);                 /* 12 + 2K doubles; 0 if K is out of range */
size_t nlml_pose_eval_result_len(int n_intervals);                 /* 14 + 2K doubles; 0 if K is out of range */
size_t nlml_pose_eval_workspace_bytes(int64_t B, int n_intervals);
int nlml_pose_eval(const float* pose_rad, const double* pred_deg, const uint8_t* valid, const double* gt_deg, int64_t B,
                   const double* h_lo, const double* h_hi, int decimals, const double* h_intervals, const int32_t* h_axes,
                   int n_intervals, void* workspace, size_t workspace_bytes, double* record_out, double* result_out,
                   double* pred_out, uint8_t* keep_out, void* stream);
int nlml_pose_eval_merge(const double* records, int64_t n, int n_intervals, double* record_out, double* result_out,
                         void* stream);

/* Artefact producers that are pure tensor algebra.
 *
 * nlml_cosine_table replaces the two nested loops over cosine() that build the heads' training inputs
 * (NLML_HPE_MLPHeadsTrainer.py:71-73,179-205): out[i][j] = a_j*cos(b_j*w_i + c_j) + d_j in f64.
 *   angles_rad f32[n]   np.radians(np.arange(min, max, interval).astype(np.float32)) (:179-181)
 *   cos_params f64[R,4] rows (a,b,c,d) = optimized_{yaw,pitch,roll} of outputs/features/Trained_data.npz
 *   out        f64[n,R]
 *
 * nlml_mode5_product replaces W = tl.tensordot(core, transpose(feature_matrix), axes=(4,0)) (TD_main.py:232-238):
 * W[q][m] = sum_r core[q][r] * U_feat[m][r], an r-ascending f32 fma chain per output.
 *   core   f32[Q,R5]  the Tucker core with its four leading modes flattened (Q = 135 for the shipped model)
 *   U_feat f32[M,R5]  mode-5 factor matrix (M = 1404 features)
 *   W      f32[Q,M]
 */
int nlml_cosine_table(const float* angles_rad, int64_t n, const double* cos_params, int R, double* out, void* stream);
int nlml_mode5_product(const float* core, const float* U_feat, int Q, int R5, int M, float* W, void* stream);

/* K7: the device primitives of the Tucker decomposition of the rotation training tensor (TD_main.py:181; the driver is
 * nlml_hpe_amd/tucker_decompose.py).  The tensor X is f32[I,ny,np,nr,M], row-major; A is its mode-1 unfolding f32[I,K], K = ny np nr M.
 * Every sum and every Gram is f64, factors are f64 [n,R] row-major (column r = the r-th vector).  No floating-point atomics: partial
 * sums go to the caller's workspace and are added in a fixed order that depends on the shape alone, so two calls give the same bits.
 * All offsets are 64-bit.  Checks, in this order, each NLML_E_BADARG with a message and before any GPU call: a NULL required buffer;
 * an extent < 1 or beyond its limit; a product of extents beyond 64-bit byte offsets; a pointer that is not aligned to its element
 * (4 bytes f32, 8 bytes f64 and workspace); a workspace shorter than the *_workspace_bytes query (which returns 0 for a shape the
 * entry point refuses).
 *
 * nlml_mode_gram (K7a)  G f64[I,I] = A A^T on the f64 matrix cores, upper-triangle tiles then mirrored: G is symmetric bit for bit.
 *   1 <= I <= NLML_GRAM_I_MAX, K >= 1.  K is cut into slices: with ceil(I / 128) tile rows and as many pairs as their upper
 *   triangle holds, tiles (tiles + 1) / 2, a slice is ceil(K / max(1, 1024 / pairs)) columns (the inner division rounds down),
 *   rounded up to a multiple of 32 and at least NLML_GRAM_KCHUNK; there are ceil(K / slice) of them and the workspace holds
 *   slices x pairs tiles of 128 x 128 f64.  Within a slice an entry is ONE chain fma(A[i][k], A[j][k], acc), k ascending from +0.0;
 *   the slices are added s = 0.0, s += slice, in ascending order.
 * nlml_pose_grams (K7b)  Gy f64[ny,ny], Gp f64[np,np], Gr f64[nr,nr]: the Grams of the mode-2, -3 and -4 unfoldings in one pass
 *   over X; a NULL output is skipped (at least one must be given) and changes nothing in the others.  ny, np, nr in
 *   1..NLML_POSE_BINS_MAX and ny np nr <= NLML_POSE_GRAMS_MAX_CELLS (all cells by 32 columns stay in LDS).  The order: a slab is one
 *   identity by 32 columns (the last of a row may be short), slab number i ceil(M / 32) + column block; partial b of
 *   min(slabs, 1024) takes the slabs b, b + partials, ...  For a mode of extent n with O cells outside it and J inside
 *   (cell = (o n + a) J + j), wave w of 4 takes the pairs (o, j) numbered o J + j = w, w + 4, ... and for each runs the slab's
 *   columns ascending; an entry of the wave is one fma chain from +0.0 over all of that, slab after slab.  The waves are added
 *   0.0 + w0 + w1 + w2 + w3, then the partials ascending from 0.0; the upper triangle is computed and mirrored.
 * nlml_project_identity (K7c)  out f32[R,K] = U^T A, U f64[I,R], 1 <= R <= NLML_TUCKER_RANK_MAX; one chain
 *   fma(U[i][r], (double)A[i][k], acc) per output, i ascending from +0.0, one rounding to f32.
 * nlml_project_pose (K7d)  out f32[I,ny',np',nr',M] = X x_2 Uy^T x_3 Up^T x_4 Ur^T, Uy f64[ny,ry] etc.; a NULL factor leaves its
 *   mode as it is (n' = n, its rank argument is ignored), else n' = its rank in 1..NLML_POSE_RANK_MAX.  f64 fma chains nested
 *   roll inside pitch inside yaw, each ascending from +0.0: tr[c] = fma(Ur[r][c], x, tr[c]) over r, tp[b][c] = fma(Up[p][b], tr[c],
 *   tp[b][c]) over p, acc[a][b][c] = fma(Uy[y][a], tp[b][c], acc[a][b][c]) over y; a NULL factor's chain has the one step of the
 *   output's own index with coefficient 1.0; one rounding to f32.  With all three NULL, out is X copied bit for bit.
 *
 * The *_ex forms take or give a tensor in f64 where the flag (a_f64, x_f64, out_f64) is nonzero -- same shapes, 8-byte alignment,
 * no rounding of an f64 output, and the sums and orders stated above (on f64 values that f32 holds, the f32 form's bits) -- with one
 * exception: nlml_pose_grams_ex with x_f64 cuts a row into slabs of 16 columns, not 32, so it has min(I ceil(M / 16), 1024) partials
 * and groups the columns differently; on inputs that are not exactly summable its bits may differ from the f32 form's.  The
 * decomposition keeps its projected tensors in f64 between two steps: a factor computed from an f32-rounded projection sits 2^-24
 * from the exact one, far outside the f64 Grams' own error.  The plain forms are the *_ex forms with every flag 0.
 * nlml_pose_grams_workspace_bytes serves both element types (it is the f64 form's partial count, never the smaller). */
#define NLML_GRAM_I_MAX      4096
#define NLML_GRAM_KCHUNK     4096
#define NLML_POSE_BINS_MAX        32
#define NLML_POSE_GRAMS_MAX_CELLS 768
#define NLML_POSE_RANK_MAX        3
size_t nlml_mode_gram_workspace_bytes(int64_t I, int64_t K);
int nlml_mode_gram(const float* A, int64_t I, int64_t K, double* G, void* workspace, size_t workspace_bytes, void* stream);
size_t nlml_pose_grams_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M);
int nlml_pose_grams(const float* X, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr,
                    void* workspace, size_t workspace_bytes, void* stream);
int nlml_project_identity(const float* A, int64_t I, int64_t K, const double* U, int R, float* out, void* stream);
int nlml_project_pose(const float* X, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up, int rp,
                      const double* Ur, int rr, float* out, void* stream);
int nlml_mode_gram_ex(const void* A, int a_f64, int64_t I, int64_t K, double* G, void* workspace, size_t workspace_bytes, void* stream);
int nlml_pose_grams_ex(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, double* Gy, double* Gp, double* Gr,
                       void* workspace, size_t workspace_bytes, void* stream);
int nlml_project_identity_ex(const float* A, int64_t I, int64_t K, const double* U, int R, void* out, int out_f64, void* stream);
int nlml_project_pose_ex(const void* X, int x_f64, int64_t I, int ny, int np, int nr, int64_t M, const double* Uy, int ry, const double* Up,
                         int rp, const double* Ur, int rr, void* out, int out_f64, void* stream);

/* K11: expand a Tucker model and compare it with the tensor in one pass -- tensorly's tucker_to_tensor and the reconstruction error
 * norm(X - reconstructed) / norm(X) of TD_main.py:221-224, without a second tensor of X's size.
 *   X     f32[I,ny,np,nr,M] or NULL (expand only: xhat is required, sums and res_id are not written, no workspace is needed)
 *   W     f32[R,ry,rp,rr,M];  U_id f64[I,R], Uy f64[ny,ry], Up f64[np,rp], Ur f64[nr,rr], row-major (column r = the r-th vector)
 *   1 <= R <= NLML_TUCKER_RANK_MAX, ry, rp, rr in 1..NLML_POSE_RANK_MAX, ny, np, nr in 1..NLML_POSE_BINS_MAX; all offsets are 64-bit
 *   sums   f64[2] = {sum (X - X_hat)^2, sum X^2}: the error is sqrt(sums[0] / sums[1]).  Required when X is given.
 *   res_id f64[I] or NULL: each identity's sum of squared residuals
 *   xhat   f32[I,ny,np,nr,M] or NULL: X_hat itself, rounded once (tucker_to_tensor; with I = 1 and a row of U_id, one identity)
 * The order (csrc/tucker_residual_ref.h holds it in code).  Per element, every chain ascending from +0.0 and every fma f64:
 *   v[b][c][d] = fma(U_id[i][a], (double)W[a][b][c][d][m], v[b][c][d]) over a;  per yaw bin y: ty[c][d] = fma(Uy[y][b], v[b][c][d],
 *   ty[c][d]) over b;  per pitch bin p: tp[d] = fma(Up[p][c], ty[c][d], tp[d]) over c;  per roll bin r: xhat = fma(Ur[r][d], tp[d],
 *   xhat) over d;  e = (double)X[i][y][p][r][m] - xhat;  s[i][m] = fma(e, e, s[i][m]), q[i][m] = fma(x, x, q[i][m]) over the cells
 *   (y, p, r) in row-major order.  The sums: column group g of G = ceil(M / 64) holds the columns 64 g + l, l = 0..63 (a column past
 *   M counts +0.0); its 64 values are added by the halving tree t[l] = t[l] + t[l + h] for l < h, h = 32, 16, .., 1, and t[0] is the
 *   partial P[i][g] in the workspace (f64[I][G][2], s and q).  A second launch of one workgroup of 256 threads: thread t takes the
 *   identities t, t + 256, .. ascending; res_id[i] = (0.0 + P[i][0]) + .. + P[i][G-1]; the thread adds its res_id ascending from
 *   +0.0; the 256 totals are added by the same halving tree, h = 128, .., 1.  No floating-point atomics; two calls give the same bits.
 * nlml_tucker_residual_host runs the same header on HOST buffers in plain C++ (no GPU involved; the workspace is a host buffer of the
 * same size) and returns the same bits.
 * Checks, the K7 list in the K7 order, each NLML_E_BADARG with a message and before any GPU call: a NULL required buffer (W, the four
 * factors, X or xhat; with X: sums and the workspace); an extent < 1 or a rank or bin count beyond its limit; a product of extents
 * beyond 64-bit byte offsets; a pointer that is not aligned to its element (4 bytes f32, 8 bytes f64 and workspace); with X, a
 * workspace shorter than nlml_tucker_residual_workspace_bytes (which returns 0 for a shape the entry point refuses). */
size_t nlml_tucker_residual_workspace_bytes(int64_t I, int ny, int np, int nr, int64_t M);
int nlml_tucker_residual(const float* X, const float* W, const double* U_id, const double* Uy, const double* Up, const double* Ur,
                         int64_t I, int ny, int np, int nr, int64_t M, int R, int ry, int rp, int rr, double* sums, double* res_id,
                         float* xhat, void* workspace, size_t workspace_bytes, void* stream);
int nlml_tucker_residual_host(const float* h_X, const float* h_W, const double* h_U_id, const double* h_Uy, const double* h_Up,
                              const double* h_Ur, int64_t I, int ny, int np, int nr, int64_t M, int R, int ry, int rp, int rr,
                              double* h_sums, double* h_res_id, float* h_xhat, void* h_workspace, size_t workspace_bytes);

/* K8: the cosine fit of the pose factors -- a batch of independent fits of  a cos(b radians(w) + c) + d  to a column, each a whole
 * Powell minimisation, in one launch.  Replaces TD_Trainer.Train's scipy.optimize.minimize(objective, guess, method='Powell') per
 * column of U_yaw, U_pitch and U_roll (TD_Trainer.py:37-42,70-93,320-322); its results are the optimized_* rows of Trained_data.npz.
 *   y       f64[C,ld]   fit f's samples y[f][0..n[f]) (a factor column, upcast: exact)
 *   w_deg   f64[C,ld]   fit f's angles in DEGREES (the bins)
 *   ld      row stride of y and w_deg in elements, >= every n[f]; offsets are 64-bit
 *   n       i32[C]      DEVICE: rows of each fit, 1..NLML_COSINE_FIT_ROWS_MAX; fits of different n may share a launch
 *   h_n     i32[C]      HOST: the same values.  The library never reads device memory on the host, so the checks below read this
 *                       copy; the kernel reads n, and clamps it to min(64, ld) so that no row is read beyond its stride.
 *   x0      f64[C,4]    the starts (a, b, c, d)
 *   xtol, ftol          scipy's xtol / ftol (its defaults: 1e-4 both)
 *   x       f64[C,4]    res.x;   fun f64[C] res.fun;   nfev, nit i32[C] res.nfev, res.nit;   status i32[C] as nlml_tucker_powell's
 *                       (1 converged, 2 maxfev = 4000 reached, 3 maxiter, 4 NaN); fun, nfev, nit, status may be NULL
 * The objective is 1/2 sum_i (y_i - (a cos(b w_i pi/180 + c) + d))^2 in the reference's f64 operation order with its two library calls
 * (np.cos and the scalar ** 2, neither correctly rounded in glibc) replaced by their correctly rounded values; csrc/cosine_fit_ref.h
 * states the order.  The minimiser is the Powell machine of nlml_tucker_powell with four parameters: given the same objective values it
 * visits scipy's trial points bit for bit.  One wave per fit, the whole minimisation inside the launch, no atomics: a fit's result does
 * not depend on its position in the batch or on C.
 * nlml_cosine_fit_objective evaluates that objective on the device at N parameter points params f64[N,4] against ONE fit's rows
 * (y, w_deg f64[n]: pass the fit's row pointers) -> out f64[N]: the evaluation the fit kernel runs, read out.
 * The *_host forms run the same header on HOST buffers in plain C++ (no GPU involved; no device copy of n) and return the same bits.
 * Checks, in this order, each NLML_E_BADARG with a message and before any GPU call.  Fits: a NULL required buffer (unless C == 0);
 * C < 0; C == 0 returns 0 and launches nothing; an n outside 1..64; ld < an n; C above 2^31 - 1 or C ld beyond 64-bit byte offsets;
 * a misaligned pointer (8 bytes f64, 4 bytes i32).  Objective: a NULL buffer (unless N == 0); N < 0; n outside 1..64; N above
 * 2^31 - 1; N == 0 returns 0; a misaligned pointer. */
#define NLML_COSINE_FIT_ROWS_MAX 64
int nlml_cosine_fit(const double* y, const double* w_deg, int64_t ld, const int32_t* n, const int32_t* h_n, int64_t C,
                    const double* x0, double xtol, double ftol, double* x, double* fun, int32_t* nfev, int32_t* nit,
                    int32_t* status, void* stream);
int nlml_cosine_fit_host(const double* h_y, const double* h_w_deg, int64_t ld, const int32_t* h_n, int64_t C, const double* h_x0,
                         double xtol, double ftol, double* h_x, double* h_fun, int32_t* h_nfev, int32_t* h_nit, int32_t* h_status);
int nlml_cosine_fit_objective(const double* y, const double* w_deg, int n, const double* params, int64_t N, double* out,
                              void* stream);
int nlml_cosine_fit_objective_host(const double* h_y, const double* h_w_deg, int n, const double* h_params, int64_t N,
                                   double* h_out);

/* K9: training steps of the landmark encoder -- the inner loop of the reference's NLML_HPE_EncoderTrainer.train_encoder
 * (:393-456, the training loop; :463-517, the validation loop) for the encoder K2 runs:
 *   Linear(F,1024) ReLU Linear(1024,512) ReLU Linear(512,256) ReLU Linear(256,128) ReLU Linear(128,64) Tanh Linear(64,9)
 * nlml_encoder_train_steps runs ceil(n / batch) consecutive steps; step s takes the batch slots [s batch, min(n, (s + 1) batch)) (the
 * last batch may be partial) and does, all in f32 on v_mfma_f32_32x32x2_f32 (csrc/encoder_train_ref.h states every operation order):
 *   forward on the rows x[order[slot]];  t = (t_yaw[labels[row][0]], t_pitch[labels[row][1]], t_roll[labels[row][2]]);
 *   loss = sum (pred - t)^2 / (3 B) (the reference's three MSELoss means, B the batch's real row count);
 *   G <- G + grad (zero_grad != 0: G <- grad; the reference never calls zero_grad, so 0 is its behaviour);
 *   n = ||G||_2 over all twelve tensors (summed in f64), c = min(1, max_norm / (n + 1e-6)), G <- c G IN PLACE (clip_grad_norm_);
 *   p <- p - lr (G + weight_decay p)  (SGD without momentum; the decay term does not enter G).
 *   x        f32[N,ldx]   the dataset, row stride ldx >= F elements; offsets are 64-bit
 *   labels   i32[N,ld_lab]  the rows' (yaw, pitch, roll) bins in the first three columns, ld_lab >= 3
 *   t_yaw    f32[n_yaw,3], t_pitch f32[n_pitch,3], t_roll f32[n_roll,3]  the target tables (float32(U_yaw) ...)
 *   params   f32[P]       W0,b0,W1,b1,...,W5,b5 contiguous, W [out,in] row-major: the state dict's tensors are views of it.
 *                         P = 1024 F + 1024 + 512*1024 + 512 + 256*512 + 256 + 128*256 + 128 + 64*128 + 64 + 9*64 + 9.  Updated in place.
 *   grads    f32[P]       the gradient accumulator G in the same layout, read and written (zero_grad: only written)
 *   F        136 or 1404;   batch 1..NLML_ENCODER_TRAIN_BATCH_MAX
 *   order    i32[n] or NULL (= 0, 1, .., n - 1): the dataset rows in the order they are visited
 *   lr, weight_decay, max_norm  of this call (one epoch: StepLR changes lr between calls); rounded to f32 as torch rounds them
 *   loss_out f32[steps], norm_out f32[steps] (n before clipping), either may be NULL;   steps = ceil(n / batch)
 *   status   i32[1] or NULL: OR of NLML_ENCODER_TRAIN_CLAMPED_ORDER (an order entry outside [0, N)) and
 *            NLML_ENCODER_TRAIN_CLAMPED_LABEL (a label outside its table), overwritten by the call.  The library never reads device
 *            memory on the host, so order and labels cannot be checked there: the kernels clamp both into range, read nothing out of
 *            bounds, and report it here.
 *   workspace  nlml_encoder_train_workspace_bytes(F, batch) bytes (0 for an F or batch outside the above); contents irrelevant
 * Every step is fourteen launches ordered by the stream: no atomics, no grid-wide barrier, no host synchronisation, nothing copied to
 * the host; the same call on the same inputs gives the same bits, and a result does not depend on ldx or on where the rows lie.
 * nlml_encoder_eval_losses: forward and loss only, batch after batch, the batches' losses to loss_out f32[steps] -- the validation
 * pass; the forward is the training step's, bit for bit.
 * The *_host forms run encoder_train_ref.h on HOST buffers in plain C++ (no GPU involved, no workspace).  They are NOT claimed to
 * return the device's bits: tanhf is ocml's on the device and glibc's on the host.  Every sum that is a chain on the device is an
 * fmaf chain in the same order on the host.
 * K9 argument checks, in this order, each NLML_E_BADARG with a message and before any GPU call: F not 136 or 1404; batch outside
 * 1..256; n < 0; n == 0 returns 0 at once (nothing else is looked at); a NULL required buffer (x, labels, the tables, params, grads
 * when training, workspace on the device); N outside 1..2^31-1; ld_lab < 3; a table without rows; ldx < F; N ldx or N ld_lab
 * beyond 64-bit byte offsets; training: lr, weight_decay or max_norm not finite, or max_norm < 0; device: workspace_bytes too
 * small; params, grads or workspace not 16-byte aligned; any other buffer not 4-byte aligned. */
#define NLML_ENCODER_TRAIN_BATCH_MAX     256
#define NLML_ENCODER_TRAIN_CLAMPED_ORDER 1
#define NLML_ENCODER_TRAIN_CLAMPED_LABEL 2
size_t nlml_encoder_train_workspace_bytes(int F, int batch);
int nlml_encoder_train_steps(const float* x, int64_t ldx, int64_t N, const int32_t* labels, int64_t ld_lab, const float* t_yaw,
                             int n_yaw, const float* t_pitch, int n_pitch, const float* t_roll, int n_roll, float* params,
                             float* grads, int F, int batch, const int32_t* order, int64_t n, double lr, double weight_decay,
                             double max_norm, int zero_grad, float* loss_out, float* norm_out, int32_t* status, void* workspace,
                             size_t workspace_bytes, void* stream);
int nlml_encoder_eval_losses(const float* x, int64_t ldx, int64_t N, const int32_t* labels, int64_t ld_lab, const float* t_yaw,
                             int n_yaw, const float* t_pitch, int n_pitch, const float* t_roll, int n_roll, const float* params,
                             int F, int batch, const int32_t* order, int64_t n, float* loss_out, int32_t* status, void* workspace,
                             size_t workspace_bytes, void* stream);
int nlml_encoder_train_steps_host(const float* h_x, int64_t ldx, int64_t N, const int32_t* h_labels, int64_t ld_lab,
                                  const float* h_t_yaw, int n_yaw, const float* h_t_pitch, int n_pitch, const float* h_t_roll,
                                  int n_roll, float* h_params, float* h_grads, int F, int batch, const int32_t* h_order, int64_t n,
                                  double lr, double weight_decay, double max_norm, int zero_grad, float* h_loss_out,
                                  float* h_norm_out, int32_t* h_status);
int nlml_encoder_eval_losses_host(const float* h_x, int64_t ldx, int64_t N, const int32_t* h_labels, int64_t ld_lab,
                                  const float* h_t_yaw, int n_yaw, const float* h_t_pitch, int n_pitch, const float* h_t_roll,
                                  int n_roll, const float* h_params, int F, int batch, const int32_t* h_order, int64_t n,
                                  float* h_loss_out, int32_t* h_status);

/* K10: training steps of the yaw, pitch and roll heads -- the inner loop of the reference's NLML_HPE_MLPHeadsTrainer.train_network
 * (:89-113) for up to three INDEPENDENT networks at once, each
 *   Linear(R,128) ReLU Linear(128,256) ReLU Linear(256,128) ReLU Linear(128,64) ReLU Linear(64,1)
 * on the rows of a cosine table (nlml_cosine_table, cast to f32) with the angle in radians as the target.  Every network of a call has
 * its own data, parameters, Adam state, visiting order and row count (one nlml_heads_net each) and shares every launch with the
 * others: the call runs max_i ceil(n_i / batch) steps, network i takes part in the first ceil(n_i / batch) of them, and afterwards
 * nothing of it is read or written and its Adam step count stays.  A step of a network on its batch of B rows (the last may be
 * partial), all in f32 on v_mfma_f32_32x32x2_f32 (csrc/heads_train_ref.h states every operation order):
 *   forward on the rows x[order[slot]];  loss = sum (pred - y)^2 / B  (MSELoss);  G <- grad (the reference's zero_grad);
 *   n = ||G||_2 over the ten tensors (summed in f64), c = min(1, max_norm / (n + 1e-6)), G <- c G in place (clip_grad_norm_);
 *   Adam with betas 0.9 / 0.999, eps 1e-8 and weight_decay added to the gradient (L2, not AdamW), in torch's single-tensor order, every
 *   operation rounded on its own; the step count t of the bias corrections is step0 + (the network's steps in this call so far) + 1.
 *     x        f32[N,ldx]  the network's table, row stride ldx >= R;   y  f32[N]  its targets
 *     params, grads, m, v  f32[P] each, W0,b0,...,W4,b4 contiguous, W [out,in] row-major: the state dict's tensors are views of
 *              params; P = 128 R + 128 + 256*128 + 256 + 128*256 + 128 + 64*128 + 64 + 64 + 1 (74,753 at R = 3).  params, m and v are
 *              updated in place, grads is overwritten (the clipped gradient of the network's last step).  The evaluation pass reads
 *              params only; grads, m and v may be NULL there.
 *     order    i32[n] or NULL (= 0, 1, .., n - 1);   n >= 1 rows are visited
 *     step0    Adam steps the network has taken before this call (the caller carries it: step0 += ceil(n / batch))
 *     loss_out f32[ceil(n / batch)], norm_out f32[ceil(n / batch)] (n before clipping), either may be NULL
 *     status   i32[1] or NULL: NLML_HEADS_TRAIN_CLAMPED_ORDER if an order entry lay outside [0, N) (it is clamped into range, nothing
 *              is read out of bounds), overwritten by the call
 *   R 1..NLML_HEADS_TRAIN_R_MAX, the same for all networks of a call;  batch 1..NLML_ENCODER_TRAIN_BATCH_MAX;  lr of this call (StepLR
 *   changes it between calls)
 *   workspace  nlml_heads_train_workspace_bytes(R, batch, n_nets) bytes (0 for an argument outside the above), contents irrelevant.
 *              Network i owns the i-th n_nets-th of it; inside, in this order and each padded to 16 bytes: the norm partials f64[78],
 *              the batch's resolved rows i32[256], A_1..A_5 f32[batch,out_l], delta_1..delta_5 f32[batch,out_l] -- the network's last
 *              step.  No other word of it is written.
 * Every step is twelve launches ordered by the stream: no atomics, no grid-wide barrier, no host synchronisation, nothing copied to
 * the host.  nlml_heads_eval_losses: forward and loss only -- the validation pass; the forward is the training step's, bit for bit.
 * The *_host forms run heads_train_ref.h on HOST buffers in plain C++ (no GPU involved) and return the device's bits, word for
 * word; h_workspace may be NULL, or a host buffer that receives what the device's workspace would hold.
 * K10 argument checks, in this order, each NLML_E_BADARG with a message and before any GPU call: n_nets outside 1..3; R outside 1..16;
 * batch outside 1..256; a NULL required pointer (nets; x, y, params of a network; grads, m, v when training; workspace on the
 * device); n <= 0 of a network; workspace_bytes too small; step0 < 0; N outside 1..2^31-1; ldx < R or N ldx beyond 64-bit byte
 * offsets; training: lr, weight_decay or max_norm not finite, or max_norm < 0; device: params, grads, m, v or workspace not 16-byte
 * aligned, any other buffer not 4-byte aligned. */
#define NLML_HEADS_TRAIN_NETS_MAX      3
#define NLML_HEADS_TRAIN_R_MAX         16
#define NLML_HEADS_TRAIN_CLAMPED_ORDER 1
typedef struct nlml_heads_net {
  const float* x; int64_t ldx; int64_t N;
  const float* y;
  float* params; float* grads; float* m; float* v;
  const int32_t* order; int64_t n;
  int64_t step0;
  float* loss_out; float* norm_out; int32_t* status;
} nlml_heads_net;
size_t nlml_heads_train_workspace_bytes(int R, int batch, int n_nets);
int nlml_heads_train_steps(const nlml_heads_net* nets, int n_nets, int R, int batch, double lr, double weight_decay, double max_norm,
                           void* workspace, size_t workspace_bytes, void* stream);
int nlml_heads_eval_losses(const nlml_heads_net* nets, int n_nets, int R, int batch, void* workspace, size_t workspace_bytes,
                           void* stream);
int nlml_heads_train_steps_host(const nlml_heads_net* h_nets, int n_nets, int R, int batch, double lr, double weight_decay,
                                double max_norm, void* h_workspace, size_t workspace_bytes);
int nlml_heads_eval_losses_host(const nlml_heads_net* h_nets, int n_nets, int R, int batch, void* h_workspace,
                                size_t workspace_bytes);

/* Host-side stepping of the same Powell state machine (no GPU involved): the caller evaluates
 * the objective.  Used to check the restated control flow against scipy on the CPU.
 *   h_state: caller-allocated buffer of nlml_powell_state_bytes() bytes.
 *   nlml_powell_step returns 1 and fills h_xeval[8] when it needs f(h_xeval) (pass it as `fin` to
 *   the next call; `fin` of the first call is ignored), 0 when finished. */
size_t nlml_powell_state_bytes(void);
int    nlml_powell_init(void* h_state, const double* h_x0, double xtol, double ftol);
int    nlml_powell_step(void* h_state, double fin, double* h_xeval);
int    nlml_powell_result(const void* h_state, double* h_x, double* h_fval, int* h_nfev, int* h_nit, int* h_status);
/* The same machine for n = 3 + r_id parameters, n = 4..19 (the rank-aware device kernel runs this one): h_x0, h_xeval and h_x hold n
 * doubles.  nlml_powell_state_bytes_n returns 0, the others NLML_E_SHAPE, for an n outside that range; the state remembers its n. */
size_t nlml_powell_state_bytes_n(int n);
int    nlml_powell_init_n(void* h_state, int n, const double* h_x0, double xtol, double ftol);
int    nlml_powell_step_n(void* h_state, double fin, double* h_xeval);
int    nlml_powell_result_n(const void* h_state, double* h_x, double* h_fval, int* h_nfev, int* h_nit, int* h_status);

#ifdef __cplusplus
}
#endif
#endif /* NLML_HPE_H */
