/*
 * okvfe.h -- C ABI of the MI355X (gfx950) vision front-end for OKVIS2.
 *
 * libokvfe.so replaces, for the front-end hot path only, the arithmetic that
 * smartroboticslab/okvis2 reaches through three C++ seams (the reference has
 * no C/FFI boundary of its own; citations are into the reference tree):
 *
 *   (1) cv::FeatureDetector::detect(image, keypoints)
 *         okvis_cv/include/okvis/implementation/Frame.hpp:152, object built at
 *         okvis_frontend/src/Frontend.cpp:2406-2409
 *         (brisk::ScaleSpaceFeatureDetector<HarrisScoreCalculator>(
 *              uniformityRadius, octaves, absoluteThreshold, maxNumKpt))
 *       cv::DescriptorExtractor::compute(image, keypoints, descriptors)
 *         okvis_cv/include/okvis/implementation/Frame.hpp:167, object built at
 *         okvis_frontend/src/Frontend.cpp:2410-2412, configured by
 *         setCameraProperties / setExtractionDirection (Frontend.cpp:239-251)
 *   (2) okvis::Frontend::detectAndDescribe (Frontend.cpp:221-269) and the
 *       brute-force loops of matchStereo (Frontend.cpp:2016-2076),
 *       matchMotionStereo (:1812-1905) and verifyRecognisedPlace (:330-355)
 *   (3) brisk::Hamming::PopcntofXORed(a, b, 3)
 *         (Frontend.cpp:341,1580,1661,1846,2024; FBrisk.cpp:66)
 *
 * Conventions: plain pointers and sizes, caller-allocated outputs, integer
 * status returns, no exceptions across the ABI.  A context is bound to one
 * GPU and is single-threaded (the reference holds one detector/extractor per
 * camera under one mutex per camera, Frontend.cpp:226,2405-2413); different
 * contexts are independent.  "_device" entry points take HIP device pointers
 * and a hipStream_t (as void*) and never synchronise the host: per-call host
 * parameters (gravity, poses) ride through a ring of pinned slots with one
 * asynchronous copy per call.  Stream argument: NULL = the context's own
 * non-blocking stream; OKVFE_STREAM_LEGACY_DEFAULT = the HIP legacy default
 * (null) stream -- the stream torch.cuda.default_stream() denotes, whose raw
 * handle is 0 and therefore cannot be passed as itself; any other value = that
 * hipStream_t.  Work enqueued on one stream is ordered with work on another
 * only by the caller (events), exactly as for any HIP library.  The
 * host-buffer entry points stage through pinned memory and return only when
 * the outputs are written.
 *
 * There is NO CPU fallback: every compute entry point fails with
 * OKVFE_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef OKVFE_H_
#define OKVFE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OKVFE_ABI_VERSION 8
#define OKVFE_STREAM_LEGACY_DEFAULT ((void*)(uintptr_t)1) /* = hipStreamLegacy */
#define OKVFE_DESC_BYTES 48 /* okvis_frontend/include/DBoW2/FBrisk.hpp:35 */

typedef enum okvfe_status {
  OKVFE_OK = 0,
  OKVFE_ERR_INVALID_ARGUMENT = 1,
  OKVFE_ERR_NO_DEVICE = 2,
  OKVFE_ERR_OUT_OF_MEMORY = 3,
  OKVFE_ERR_UNSUPPORTED = 4, /* e.g. octaves > 4 */
  OKVFE_ERR_CAPACITY = 5,    /* a caller- or context-sized buffer was too small */
  OKVFE_ERR_DEVICE = 6,      /* HIP runtime error; see okvfe_last_error */
  OKVFE_ERR_NOT_READY = 7    /* e.g. camera-aware extraction without okvfe_set_camera */
} okvfe_status;

/* Layout-compatible with cv::KeyPoint as the reference consumes it
 * (okvis_cv/include/okvis/implementation/Frame.hpp:253-273). */
typedef struct okvfe_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
  int32_t class_id;
} okvfe_keypoint;

typedef enum okvfe_distortion {
  OKVFE_DIST_NONE = 0,
  OKVFE_DIST_RADTAN = 1,     /* okvis::cameras::RadialTangentialDistortion */
  OKVFE_DIST_EQUIDISTANT = 2, /* okvis::cameras::EquidistantDistortion */
  OKVFE_DIST_RADTAN8 = 3      /* okvis::cameras::RadialTangentialDistortion8 (OpenCV "rational"
                               * model, k1 k2 p1 p2 k3 k4 k5 k6); ABI 8, okvfe_camera_ext only.
                               * distort: rad = (1 + rho (k1 + rho (k2 + k3 rho))) /
                               * (1 + rho (k4 + rho (k5 + k6 rho))), rho = |u|^2; it FAILS for
                               * rho > 9 (projection status Invalid, awareness-map Jacobian 0).
                               * undistort: 5 Gauss-Newton steps, success at chi2 < 1e-4 (the
                               * 4-coefficient model: 1e-6).  Defined deviation: the reference
                               * ignores a failing distort inside its Gauss-Newton loop and reads
                               * an uninitialised point; here such a step ends the iteration and
                               * the back-projection is invalid. */
} okvfe_distortion;

/* okvis::cameras::PinholeCamera<DISTORTION_T> intrinsics
 * (okvis_cv/include/okvis/cameras/PinholeCamera.hpp). */
typedef struct okvfe_camera {
  int32_t width, height;
  double fu, fv, cu, cv;
  int32_t distortion; /* okvfe_distortion */
  double d[4];        /* k1 k2 p1 p2 | k1 k2 k3 k4 */
} okvfe_camera;         /* 80 bytes; distortion 0..2 */

/* ABI 8: every distortion type, OKVFE_DIST_RADTAN8 included.  For RADTAN8 base.d = k1 k2 p1 p2
 * and d_ext = k3 k4 k5 k6 -- the order of PinholeCamera<RadialTangentialDistortion8>::
 * getIntrinsics() after fu fv cu cv; for types 0..2 d_ext is ignored.  112 bytes. */
typedef struct okvfe_camera_ext {
  okvfe_camera base;
  double d_ext[4];
} okvfe_camera_ext;

/* T_WC as rotation (row-major) and translation: p_W = C p_C + r. */
typedef struct okvfe_pose {
  double C[9];
  double r[3];
} okvfe_pose;

/* Detector / extractor / matcher parameters = okvis::FrontendParameters
 * (okvis_common/include/okvis/Parameters.hpp:123-133) plus sizes. */
typedef struct okvfe_config {
  int32_t abi_version;        /* OKVFE_ABI_VERSION */
  int32_t device;             /* HIP device ordinal */
  int32_t width, height;      /* image size, fixed per context */
  int32_t max_batch;          /* images per batch call (>= 1) */
  int32_t num_cameras;        /* camera slots for camera-aware extraction (>= 1) */
  float uniformity_radius;    /* detection_threshold: uniformity radius in px */
  int32_t octaves;            /* 0 = single scale (every shipped config); 1..4 = scale space of
                               * 2*octaves layers (the reference's own smoke test uses 2,
                               * okvis_cv/test/TestFrame.cpp:75-77): every layer may deliver
                               * max_keypoints, so rows per image = 2*octaves*max_keypoints */
  int32_t absolute_threshold; /* Harris noise floor, >= 1 */
  int32_t max_keypoints;      /* max_num_keypoints */
  int32_t rotation_invariant; /* Frontend.cpp:142 default true */
  int32_t scale_invariant;    /* Frontend.cpp:143 default false.  true: the published BRISK scale
                               * ladder -- the pattern of keypoint k is the base pattern scaled to
                               * index okvfe_scale_index(k.size) of 64 (the fixed-scale extractor is
                               * index 17 of the same ladder) */
  int32_t match_threshold;    /* matching_threshold (Hamming bits, strict <) */
  int32_t max_candidates;     /* per-image NMS candidate capacity; 0 = worst case */
  int32_t score_type;         /* OKVFE_SCORE_HARRIS (0): brisk::HarrisScoreCalculator, the x86
                               * reference path and every shipped configuration (Frontend.cpp:2406);
                               * OKVFE_SCORE_AGAST_9_16 (1): the AGAST 9-16 corner score of
                               * brisk::BriskFeatureDetector, the reference's ARM branch
                               * (okvis_cv/test/TestFrame.cpp:71-72), absolute_threshold = its
                               * threshold (34 there); the rest of the detector is shared */
  float box_scale;            /* ABI 7.  Smoothing width of the built-in BRISK2 pattern: every sample's box half-side
                               * = the published one (sigma = 1.3 x the ring's sample spacing) x box_scale; 0 and 1.0 =
                               * the published boxes.  The one parameter of the descriptor that no file of the reference
                               * tree pins (the boxes live in the un-vendored brisk submodule; the vocabulary's statistics
                               * sit best at 1.7 - 2.0 x, tools/pattern/README.md): a named knob instead of an
                               * okvfe_get_pattern / okvfe_set_pattern edit.  Range (0.25, 2.5]; up to 2.05 stays on the
                               * fast descriptor kernels (21 x 21 / 10 x 10 row slots from 1.03 x on).  okvfe_set_pattern
                               * afterwards replaces the whole pattern, this scaling included. */
} okvfe_config;
#define OKVFE_SCORE_HARRIS 0
#define OKVFE_SCORE_AGAST_9_16 1
/* 2: the published BRISK scale-space detector = brisk::BriskFeatureDetector(threshold, octaves)
 * (okvis_cv/test/TestFrame.cpp:71-72): absolute_threshold = the AGAST threshold, octaves as there;
 * AGAST 9-16 scores on the octaves c_i and intra-octaves d_i, the FAST 5-8 score of c0 as the layer
 * below the first octave, maxima over the 3 x 3 neighbourhood and the +-1 px patches of the layers
 * above and below, 2-D sub-pixel fit, and a parabola over the three layers' scores for the CONTINUOUS
 * scale (keypoint.size = 12 x scale, response = the parabola's maximum, octave = layer index; layer nodes
 * 3/4, 1, 3/2 on octaves, 2/3, 1, 4/3 on intra-octaves, 2/3, 1, 3/2 with the result in [0.7, 1.5] on c0).  No
 * uniformity stage (uniformity_radius is ignored); the strongest max_keypoints maxima per layer are
 * kept, (score desc, y, x).  With octaves == 0 it is OKVFE_SCORE_AGAST_9_16.
 * CAVEATS (the brisk sources are not in the reference tree; tools/ref_compare is the check):
 *  - the keypoint POSITION is the 2-D sub-pixel fit on the keypoint's own layer, scaled to image coordinates; the
 *    published detector additionally re-interpolates the position between the fits of the layers above and below
 *    along the fitted scale -- NOT restated here, so x / y may differ from a brisk build by a fraction of a pixel
 *    times the layer's scale while size / response / octave follow the parabola described above;
 *  - the c0 node 2/3 (and the [0.7, 1.5] clamp) is taken from the coefficient matrix quoted in the published
 *    refine1D_2's comment, not from verified code: if the executable coefficients there fit nodes 1/2, 1, 3/2,
 *    sizes and responses of layer-0 keypoints differ. */
#define OKVFE_SCORE_BRISK_SCALESPACE 2

typedef struct okvfe_ctx okvfe_ctx;

/* ---- lifetime ------------------------------------------------------------ */
okvfe_status okvfe_create(const okvfe_config* cfg, okvfe_ctx** out);
void okvfe_destroy(okvfe_ctx* ctx);
/* Message of the last failing call on this context ("" if none). ctx may be
 * NULL to read the message of a failed okvfe_create on this thread. */
const char* okvfe_last_error(const okvfe_ctx* ctx);
int32_t okvfe_abi_version(void);

/* ---- camera-aware extraction setup --------------------------------------- */
/* = BriskDescriptorExtractor::setCameraProperties(rays, imageJacobians, fu)
 * (Frontend.cpp:239-242): host maps, H*W*3 and H*W*6 floats; copied. */
okvfe_status okvfe_set_camera_maps(okvfe_ctx* ctx, int32_t cam, const float* rays_hw3,
                                   const float* jacobians_hw6, float fu);
/* Builds the same maps from intrinsics on the host
 * (= PinholeCamera::initialiseCameraAwarenessMaps, PinholeCamera.hpp:180-208)
 * and uploads them; also stores the intrinsics for back-projection. */
okvfe_status okvfe_set_camera(okvfe_ctx* ctx, int32_t cam, const okvfe_camera* camera);
/* ABI 8: the same for every distortion type (OKVFE_DIST_RADTAN8 included).  The plain okvfe_camera
 * entry points forward here with d_ext zeroed and reject OKVFE_DIST_RADTAN8 with
 * OKVFE_ERR_INVALID_ARGUMENT (its last four coefficients do not fit okvfe_camera). */
okvfe_status okvfe_set_camera_ext(okvfe_ctx* ctx, int32_t cam, const okvfe_camera_ext* camera);
/* Host helper: fills caller buffers with the awareness maps of a camera. */
okvfe_status okvfe_build_awareness_maps(const okvfe_camera* camera, float* rays_hw3,
                                        float* jacobians_hw6);
okvfe_status okvfe_build_awareness_maps_ext(const okvfe_camera_ext* camera, float* rays_hw3,
                                            float* jacobians_hw6);

/* Host helper: field-of-view overlap of `camera` as seen by `other`
 * (= NCameraSystem::computeOverlaps, okvis_cv/src/NCameraSystem.cpp:48-119; decides which
 * camera pairs matchStereo visits, Frontend.cpp:1998).  R_other_cam = rotation part of
 * T_Cother_C, row-major.  mask_hw (H*W of `camera`, 1 = visible) may be NULL. */
okvfe_status okvfe_camera_overlap(const okvfe_camera* camera, const okvfe_camera* other,
                                  const double R_other_cam[9], uint8_t* mask_hw,
                                  int32_t* has_overlap);
okvfe_status okvfe_camera_overlap_ext(const okvfe_camera_ext* camera, const okvfe_camera_ext* other,
                                      const double R_other_cam[9], uint8_t* mask_hw,
                                      int32_t* has_overlap);

/* ---- detect + describe, host buffers (cv::Feature2D-shaped) -------------- */
/* One image: detect(), compute() and Frame::computeBackProjections in one
 * call.  gravity_C = extraction direction (gravity in the camera frame,
 * Frontend.cpp:247-251); NULL or cam < 0 selects the non-camera-aware mode.
 * keypoints/descriptors: capacity `cap` rows; backproj (cap*3 doubles) and
 * backproj_valid (cap bytes) may be NULL. */
okvfe_status okvfe_detect_describe(okvfe_ctx* ctx, const uint8_t* image, size_t stride,
                                   int32_t cam, const float gravity_C[3],
                                   okvfe_keypoint* keypoints, uint8_t* descriptors,
                                   double* backproj, uint8_t* backproj_valid, int32_t cap,
                                   int32_t* n_out);
/* detect() only (no descriptor-stage removal): keypoints in acceptance order. */
okvfe_status okvfe_detect(okvfe_ctx* ctx, const uint8_t* image, size_t stride,
                          okvfe_keypoint* keypoints, int32_t cap, int32_t* n_out);

/* cv::FeatureDetector::detect when the SAME image goes to cv::DescriptorExtractor::compute right after
 * it, as okvis::Frame::detect() / Frame::describe() do (okvis_cv/include/okvis/implementation/
 * Frame.hpp:152,167; the extraction direction is set before both, Frontend.cpp:246-251): returns what
 * okvfe_detect returns, but runs the whole detect + describe chain for (cam, gravity_C) on the one
 * upload and keeps the result.  An okvfe_compute that then asks for exactly this -- same image pointer,
 * stride and pixel content, same cam / gravity_C, the keypoints unchanged -- is answered from the kept
 * result without touching the GPU; any other okvfe_compute runs as usual.  One image upload and one
 * synchronisation per frame instead of two. */
okvfe_status okvfe_detect_ahead(okvfe_ctx* ctx, const uint8_t* image, size_t stride, int32_t cam,
                                const float gravity_C[3], okvfe_keypoint* keypoints, int32_t cap, int32_t* n_out);

/* compute() only = cv::DescriptorExtractor::compute(image, keypoints, descriptors)
 * (Frame.hpp:167): describes the n_in caller keypoints (in/out: the extractor
 * removes keypoints too close to the rim, order preserved) and back-projects
 * the survivors.  n_in <= max_keypoints. */
okvfe_status okvfe_compute(okvfe_ctx* ctx, const uint8_t* image, size_t stride, int32_t cam,
                           const float gravity_C[3], okvfe_keypoint* keypoints, int32_t n_in,
                           uint8_t* descriptors, double* backproj, uint8_t* backproj_valid,
                           int32_t* n_out);

/* ---- detect + describe, device-resident batches -------------------------- */
/* images_dev: n_images contiguous H*W u8 images in HBM.  cam_ids /
 * gravity_C (n_images*3) are HOST arrays (NULL = not camera aware).
 * Results stay in the context's device buffers (okvfe_get_device_outputs). */
okvfe_status okvfe_detect_describe_batch_device(okvfe_ctx* ctx, const uint8_t* images_dev,
                                                int32_t n_images, const int32_t* cam_ids,
                                                const float* gravity_C, void* stream);

/* Host-fed form of the batch call: images_host = n_images contiguous H*W u8 images in HOST
 * memory, as frames arrive in the reference (cv::Mat handed to the multiframe,
 * okvis_multisensor_processing/src/ThreadedSlam.cpp:247-265).  The context owns two device image
 * buffers and a copy stream: the PCIe copy of this batch is enqueued at once and the kernels wait
 * for it through an event, so with pinned host memory (hipHostMalloc / cudaHostRegister; a pageable
 * source makes the runtime stage the copy synchronously) the call returns immediately and the copy
 * of batch k+1 runs under the kernels of batch k.  images_host must stay valid until the work
 * enqueued on `stream` by this call has completed.  Results as okvfe_detect_describe_batch_device. */
okvfe_status okvfe_detect_describe_batch_host(okvfe_ctx* ctx, const uint8_t* images_host,
                                              int32_t n_images, const int32_t* cam_ids,
                                              const float* gravity_C, void* stream);

typedef struct okvfe_device_outputs {
  int32_t max_keypoints;         /* row capacity per image (= max_keypoints * layers) */
  const int32_t* counts;         /* [max_batch] kept keypoints per image */
  const okvfe_keypoint* keypoints; /* [max_batch][max_keypoints] */
  const uint8_t* descriptors;    /* [max_batch][max_keypoints][48] */
  const double* backproj;        /* [max_batch][max_keypoints][3] */
  const uint8_t* backproj_valid; /* [max_batch][max_keypoints] */
  const int32_t* scores;         /* [max_batch][H][score_pitch] score maps of the last detect call (layer 0);
                                  * pixel (x, y) at y * score_pitch + okvfe_score_column(ctx, x).  NULL when
                                  * that call wrote no map: see okvfe_set_keep_score_map */
  const int32_t* detect_counts;  /* [max_batch] keypoints before descriptor-stage removal */
  const int32_t* candidate_counts; /* [max_batch] NMS maxima found (may exceed capacity) */
  int32_t score_pitch;           /* ints per score-map row (>= W: the fused score+NMS kernel pads rows so that
                                  * every wave stores whole 128-byte lines) */
  int32_t score_strips;          /* 0 / 1: dense rows; >= 2: column x sits at okvfe_score_column(ctx, x) */
} okvfe_device_outputs;
okvfe_status okvfe_get_device_outputs(okvfe_ctx* ctx, okvfe_device_outputs* out);
/* Column of pixel x within a row of okvfe_device_outputs.scores (x itself for dense maps).  For a
 * dense copy of the score map use okvfe_harris_score_device. */
int32_t okvfe_score_column(const okvfe_ctx* ctx, int32_t x);
/* Single-scale Harris detection keeps NO score map by default (ABI 5): HarrisScoreCalculator's map
 * (behind cv::FeatureDetector::detect, Frame.hpp:152) is only ever read at the maxima, so the fused
 * score + NMS kernel writes the candidates alone -- one of its five bytes per pixel -- and the selection
 * recomputes the nine sub-pixel scores of the keypoints it keeps from the image, bit-identical.  keep = 1
 * makes the following detect calls of this context write the map again (okvfe_device_outputs.scores);
 * scale-space and AGAST contexts always keep theirs. */
okvfe_status okvfe_set_keep_score_map(okvfe_ctx* ctx, int32_t keep);
/* Lanes inside one call (ABI 7).  okvfe_detect_describe_batch_device / _host cut a batch into `lanes` slices of whole
 * stereo pairs and run each slice's kernel chain on a stream of the context's own, joined back onto the caller's
 * stream before the call returns (still without a host synchronisation): the vector-ALU-bound score kernel of one
 * slice runs under the LDS- and latency-bound selection / descriptor kernels of another -- what a caller used to get
 * only by splitting the batch over several contexts and streams (the camera-parallel shape of
 * okvis_multisensor_processing/src/ThreadedSlam.cpp:434-448, inside the call).  Results are those of the unsplit
 * call, byte for byte (every kernel works per image).  lanes = 0: the library's choice -- at present not to cut: with
 * ONE caller stream every call ends in a join, the slices run in phase and measure 1-5 % slower than the unsplit call,
 * while several contexts on several streams (lanes that drift out of phase across calls) gain 8 %: DESIGN.md (e); 1: off;
 * 2..8: that many.  Single-scale contexts only; others ignore it.
 * NEGATIVE, -2 .. -8: PIPELINED lanes.  The call does not join its lanes onto the caller's stream at all, and an
 * okvfe_match_stereo_batch_device that follows matches each slice's pairs on that slice's lane stream (every pair inside
 * one slice, the slices' pairs in contiguous runs -- what a batch of stereo pairs (2i, 2i + 1) is).  Lane l then starts
 * the NEXT call's score kernel behind its own previous work instead of behind everybody's: the lanes drift out of phase
 * and stay there, which is what makes several contexts on several streams faster than one.  The price is the contract:
 * after such a call returns, work the CALLER queues on its stream is NOT ordered behind the results.  Any other entry
 * point of the context that touches its buffers joins first (the host-array matchers, which do not, are listed in
 * tests/test_capi_join_audit.py): a stream-taking one makes the stream it is given wait for the lanes, every time,
 * until the host has waited for them; a host-side reader (okvfe_download_image_result, okvfe_check_capacity,
 * okvfe_get_device_outputs, okvfe_profile_*) synchronises the lanes themselves, whatever streams were joined before.
 * okvfe_lanes_join(ctx, stream) joins explicitly, and orders THAT stream only: a join on one stream says nothing about
 * another.  The caller must join the stream it uses before it overwrites the input images or reads the match rows with
 * kernels of its own.  A pipelined call that cuts its batch differently from the previous one waits for the old slices
 * first.  okvfe_set_camera* and okvfe_set_pattern apply to LATER calls: they wait for the calls already queued (the
 * lanes, the last stream used, the context's own) before they change anything.  Results are the unsplit call's, byte
 * for byte. */
okvfe_status okvfe_set_internal_lanes(okvfe_ctx* ctx, int32_t lanes);
/* Makes `stream` wait for every pipelined lane of the context (no-op when none was issued since the host last waited).
 * NULL = the context's OWN stream, not the caller's current one: a caller that means torch.cuda.current_stream() or the
 * legacy default stream passes it (OKVFE_STREAM_LEGACY_DEFAULT for the latter). */
okvfe_status okvfe_lanes_join(okvfe_ctx* ctx, void* stream);

/* Order of every 3-term FP64 sum in the matchers' gate chain (dot products, norms, C * v and C^T * v:
 * stereo_triangulation.cpp:62-76, Frontend.cpp:2027-2073 evaluate them through Eigen):
 *   OKVFE_SUM3_EIGEN_TREE (default, ABI 6)  x0 + (x1 + x2) -- Eigen's unrolled non-vectorised reduction of a
 *                                           fixed-size Vector3d (Redux.h, split at Length / 2), which is what a
 *                                           stock build takes because Vector3d is not packet-aligned;
 *   OKVFE_SUM3_LEFT_TO_RIGHT                (x0 + x1) + x2 -- the order ABI <= 5 used.
 * Affects hp_W / quality / back-projection-derived values by <= 1 ulp per sum (decisions rarely flip, bytes do).
 * Neither order can be confirmed against the reference in this tree (no Eigen); tools/ref_compare decides it
 * on a machine with the reference built.  The setting lives on the context's DEVICE: it applies to every
 * context of this process on that device, and the call synchronises the device. */
#define OKVFE_SUM3_LEFT_TO_RIGHT 0
#define OKVFE_SUM3_EIGEN_TREE 1
okvfe_status okvfe_set_fp64_reduction(okvfe_ctx* ctx, int32_t order);

/* Several contexts fed in turn from several host threads / streams on ONE GPU (a camera per context,
 * ThreadedSlam.cpp:434-448): mode 1 runs the score kernels of all contexts of the process on a device
 * one after the other in enqueue order while everything downstream of them overlaps freely, so the
 * VALU-bound score kernel of one context runs beside the latency-bound selection / matching of
 * another instead of beside another score kernel; mode 2 also chains the descriptor kernels; 0 (the
 * default) = off.  Process-wide, takes effect for calls enqueued afterwards.  (The library reads no
 * environment variable.) */
okvfe_status okvfe_set_heavy_kernel_chaining(int32_t mode);

/* Scale index of the scale-invariant extractor (brisk::BriskDescriptorExtractor(rotInv, scaleInv =
 * true), Frontend.cpp:2410-2412) for a keypoint of diameter `size`, published BRISK:
 * max(int(64 / lb(30) * lb(size / (0.6 * 12)) + 0.5), 0), at most 63.  Host-only, no context. */
int32_t okvfe_scale_index(float keypoint_size);

/* NMS candidate capacity check of the last batch (synchronises; one small copy): an image whose
 * score map had more maxima than the context's candidate capacity (okvfe_config.max_candidates)
 * keeps NO keypoints -- which maxima an overflowing list drops would depend on the order of the
 * atomics; in a scale space (octaves > 0) the list of ANY layer empties the whole image, on the
 * device (detect_counts, counts, gather blocks) as on the host -- and makes this call fail with OKVFE_ERR_CAPACITY (*first_overflowed = its index, -1
 * if none; may be NULL).  Device-resident pipelines (batch detect -> match / gather) call this
 * once per batch or once per sequence, as their budget allows. */
okvfe_status okvfe_check_capacity(okvfe_ctx* ctx, int32_t n_images, int32_t* first_overflowed);

/* Copies image `index` of the last batch to host buffers (synchronises). */
okvfe_status okvfe_download_image_result(okvfe_ctx* ctx, int32_t index, okvfe_keypoint* keypoints,
                                         uint8_t* descriptors, double* backproj,
                                         uint8_t* backproj_valid, int32_t cap, int32_t* n_out);

/* The batch call in two halves, = Frame::detect / Frame::describe of the reference
 * (okvis_cv/include/okvis/implementation/Frame.hpp:140-154, 160-175): okvfe_detect_batch_device
 * leaves the detected keypoints in the context, okvfe_describe_batch_device (same images, same
 * n_images) extracts descriptors, compacts and back-projects.  Splitting lets a caller with
 * several contexts / streams enqueue detect for all of them before describe for all of them.
 *
 * okvfe_set_heavy_kernel_chaining(1) makes the score kernels of all contexts of the process (per
 * device) run one after the other, in enqueue order, through events; 2 chains the describe
 * kernels as well.  Contexts fed in turn from different streams then run out of phase, so the
 * latency-bound stages of one overlap the throughput-bound ones of another (bench.py --lanes). */
okvfe_status okvfe_detect_batch_device(okvfe_ctx* ctx, const uint8_t* images_dev,
                                       int32_t n_images, void* stream);
okvfe_status okvfe_describe_batch_device(okvfe_ctx* ctx, const uint8_t* images_dev,
                                         int32_t n_images, const int32_t* cam_ids,
                                         const float* gravity_C, void* stream);

/* ---- single stages on device buffers (parity tests, profiling) ----------- */
/* K1: score maps of the configured score_type (Harris unless the context was created with
 * OKVFE_SCORE_AGAST_9_16), n_images * H * W int32. */
okvfe_status okvfe_harris_score_device(okvfe_ctx* ctx, const uint8_t* images_dev,
                                       int32_t n_images, int32_t* scores_dev, void* stream);
/* Diagnostic: the byte mover of the fused score + NMS kernel -- the same loads and the same stores
 * on the context's score-map layout with no arithmetic in between (the score maps receive pixel
 * bytes; no candidates are produced).  Its duration is that kernel's own memory floor; bench.py
 * times it beside the kernel (roofline.byte_mover_ms).  OKVFE_ERR_UNSUPPORTED where the fused kernel
 * does not apply (AGAST score types, widths that are no multiple of 4, octaves > 0). */
okvfe_status okvfe_harris_byte_mover_device(okvfe_ctx* ctx, const uint8_t* images_dev,
                                            int32_t n_images, void* stream);

/* ---- stage profiling ----------------------------------------------------- */
/* When enabled, every stage launch of the batch entry points is bracketed by a
 * HIP event pair on the launch stream (no synchronisation is added).
 * okvfe_profile_read synchronises and returns, per stage, the summed elapsed
 * milliseconds and the number of launches since okvfe_profile_enable. */
typedef enum okvfe_stage {
  OKVFE_STAGE_HARRIS = 0,   /* K1 score map */
  OKVFE_STAGE_NMS = 1,      /* K2 */
  OKVFE_STAGE_SORT = 2,     /* K3 sort */
  OKVFE_STAGE_SELECT = 3,   /* K3 uniformity + K4 sub-pixel */
  OKVFE_STAGE_MAP = 4,      /* map matchers on device blocks: matchToMap / uninitialised / verifyRecognisedPlace */
  OKVFE_STAGE_DESCRIBE = 5, /* K6 */
  OKVFE_STAGE_COMPACT = 6,  /* compaction + back-projection */
  OKVFE_STAGE_MATCH = 7,    /* K7 gated stereo match */
  OKVFE_STAGE_COUNT = 8
} okvfe_stage;
/* enable: 0 = off, 1 = every stage, or an OR of OKVFE_PROFILE_STAGE(stage) to time only some
 * stages (each timed launch costs two event records, i.e. two barrier packets on the stream). */
#define OKVFE_PROFILE_STAGE(stage) (1 << (8 + (stage)))
okvfe_status okvfe_profile_enable(okvfe_ctx* ctx, int32_t enable);
okvfe_status okvfe_profile_read(okvfe_ctx* ctx, double total_ms[OKVFE_STAGE_COUNT],
                                int32_t launches[OKVFE_STAGE_COUNT]);

/* ---- matching ------------------------------------------------------------ */
typedef struct okvfe_stereo_match {
  int32_t k1;            /* index in image 1, -1 = no match */
  int32_t dist;          /* Hamming distance of the match (match_threshold if none) */
  int32_t initialisable; /* !isParallel */
  int32_t pad;
  double hp_W[4];        /* triangulated homogeneous point, world frame */
} okvfe_stereo_match;

/* One (im0, im1) pair of the last batch, = the k0 x k1 loop of
 * Frontend::matchStereo (Frontend.cpp:2016-2076). */
typedef struct okvfe_stereo_pair {
  int32_t image0, image1; /* indices into the last batch */
  okvfe_pose T_WC0, T_WC1;
  double f0, f1;          /* 0.5*(fu+fv) of each camera */
} okvfe_stereo_pair;

/* pairs: HOST array.  matches_dev: [n_pairs][max_keypoints] device rows. */
okvfe_status okvfe_match_stereo_batch_device(okvfe_ctx* ctx, const okvfe_stereo_pair* pairs,
                                             int32_t n_pairs, okvfe_stereo_match* matches_dev,
                                             void* stream);
/* Host-buffer form on explicit descriptor sets (no context batch needed). */
okvfe_status okvfe_match_stereo(okvfe_ctx* ctx, const uint8_t* desc0, const okvfe_keypoint* kp0,
                                const double* backproj0, const uint8_t* valid0, int32_t n0,
                                const uint8_t* desc1, const okvfe_keypoint* kp1,
                                const double* backproj1, const uint8_t* valid1, int32_t n1,
                                const okvfe_pose* T_WC0, const okvfe_pose* T_WC1, double f0,
                                double f1, okvfe_stereo_match* matches /* n0 */);

typedef struct okvfe_motion_match {
  int32_t k1;            /* index in the current frame, -1 = no match */
  int32_t dist;
  int32_t initialisable; /* !isParallel */
  int32_t accepted;      /* winner re-projects within 4 px (Frontend.cpp:1897-1905) */
  double cos_quality;    /* quality = acos(cos_quality) (Frontend.cpp:1887-1889) */
  double hp_W[4];
} okvfe_motion_match;

/* = the k0 x k1 loop of Frontend::matchMotionStereo for one (older frame, current frame, camera)
 * triple (Frontend.cpp:1789-1905).  Frame 0 = older frame.  skip0[k0] != 0: k0 is not matched
 * (landmark already initialised / already observed, :1814-1841); matched1[k1] != 0: current
 * keypoint already carries a landmark and is left out (:1795-1798).  Either may be NULL.
 * Host buffers; `camera` is the shared camera of both frames. */
okvfe_status okvfe_match_motion_stereo(okvfe_ctx* ctx, const okvfe_camera* camera,
                                       const uint8_t* desc0, const okvfe_keypoint* kp0,
                                       const double* backproj0, const uint8_t* valid0,
                                       const uint8_t* skip0, int32_t n0, const uint8_t* desc1,
                                       const okvfe_keypoint* kp1, const double* backproj1,
                                       const uint8_t* valid1, const uint8_t* matched1, int32_t n1,
                                       const okvfe_pose* T_WC0, const okvfe_pose* T_WC1,
                                       okvfe_motion_match* matches /* n0 */);
okvfe_status okvfe_match_motion_stereo_ext(okvfe_ctx* ctx, const okvfe_camera_ext* camera,
                                           const uint8_t* desc0, const okvfe_keypoint* kp0,
                                           const double* backproj0, const uint8_t* valid0,
                                           const uint8_t* skip0, int32_t n0, const uint8_t* desc1,
                                           const okvfe_keypoint* kp1, const double* backproj1,
                                           const uint8_t* valid1, const uint8_t* matched1, int32_t n1,
                                           const okvfe_pose* T_WC0, const okvfe_pose* T_WC1,
                                           okvfe_motion_match* matches /* n0 */);

/* = Frontend::matchToMapByThread for the 3-D landmarks (Frontend.cpp:1552-1589), all keypoints
 * in one call.  Landmarks in the caller's order (ascending LandmarkId in the reference);
 * landmark l owns pool rows desc_begin[l] .. desc_begin[l+1]-1 (<= 3 descriptors each,
 * :1220-1222) and the projection (2 doubles).  use[k] == 0 skips keypoint k (:1541-1547).
 * reprojection_threshold: 20 px with IMU, 150 without (:1530).  Outputs per keypoint: landmark
 * INDEX (-1 = none) and distance (match_threshold if none). */
okvfe_status okvfe_match_to_map(okvfe_ctx* ctx, const uint8_t* desc, const okvfe_keypoint* kps,
                                const uint8_t* use, int32_t n_kps, const double* projections_l2,
                                const int32_t* desc_begin /* n_landmarks + 1 */,
                                int32_t n_landmarks, const uint8_t* pool,
                                double reprojection_threshold, int32_t* best_landmark,
                                int32_t* best_dist);

/* ---- matchToMap from the raw landmark table (no host-side pooling) ---------------------------
 * = Frontend::matchToMap up to and including its first matcher pass (Frontend.cpp:1219-1411):
 * every landmark is projected into the current camera (FoV check, :1232-1256), its observations
 * are scored and pooled by the three-slot "best views" buffer exactly as written at :1262-1354,
 * and the 3-D landmarks are matched against the frame (matchToMapByThread, :1552-1589) -- all on
 * the device, the pooled set never visits the host.
 * Landmarks in ascending LandmarkId order (the order of the reference's std::map); landmark l owns
 * observations obs_begin[l] .. obs_begin[l+1]-1, listed in the reference's iteration order
 * (observations.rbegin() -> rend()). */
typedef struct okvfe_landmark_table {
  int32_t n_landmarks, n_observations, n_poses;
  const double* hp_W;         /* n_landmarks x 4 homogeneous points (MapPoint::point) */
  const double* quality;      /* n_landmarks (MapPoint::quality) */
  const int32_t* obs_begin;   /* n_landmarks + 1 */
  const int32_t* obs_pose;    /* n_observations: index into poses */
  const uint8_t* obs_desc;    /* n_observations x 48: keypointDescriptor of the observing keypoint */
  const double* obs_backproj; /* n_observations x 3: its cached back-projection (not normalised) */
  const okvfe_pose* poses;    /* n_poses: T_WC of every observing (frame, camera) */
} okvfe_landmark_table;

/* What the pooling left per landmark (caller-allocated, n_landmarks rows; the struct pointer may
 * be NULL): status 0 = not matched against (outside the FoV or no pooled view), 1 = 3-D, 2 = not
 * 3-D yet (LandmarkToMatch::is3d); n_desc = pooled descriptors (0..2); obs_rows[3l + r] =
 * observation whose descriptor is pooled row r (-1 = none; row 2 may be written but is cropped as
 * in the reference); projection (2); e_W / r_W: 2 x 3 doubles, observing unit ray and camera
 * centre per pooled row (LandmarkToMatch::e_W / r_W) -- together the inputs of
 * okvfe_match_to_map_uninitialised for the status-2 landmarks. */
typedef struct okvfe_landmark_pool {
  int32_t* status;
  int32_t* n_desc;
  int32_t* obs_rows;
  double* projection;
  double* e_W;
  double* r_W;
} okvfe_landmark_pool;

/* cam = camera slot with intrinsics (okvfe_set_camera); exclusive != 0 =
 * loopClosureLandmarksToUseExclusively (view-point / scale pruning off, :1293-1303).  Outputs per
 * keypoint as okvfe_match_to_map: landmark index (into the table, -1 = none) and distance. */
okvfe_status okvfe_match_to_map_landmarks(okvfe_ctx* ctx, int32_t cam, const okvfe_landmark_table* table,
                                          const okvfe_pose* T_WC1, double reprojection_threshold,
                                          int32_t exclusive, const uint8_t* desc,
                                          const okvfe_keypoint* kps, const uint8_t* use, int32_t n_kps,
                                          okvfe_landmark_pool* pool_out, int32_t* best_landmark,
                                          int32_t* best_dist);

/* = Frontend::matchToMapByThreadUnitialised (Frontend.cpp:1616-1719), all keypoints in one call:
 * landmarks that are not 3-D yet.  Pool row d carries its observing unit ray e0_W[d] and camera
 * centre r0_W[d] (3 doubles each, LandmarkToMatch::e_W / r_W).  backproj = the current frame's
 * cached back-projections (normalised inside, :1625); use[k] != 0 as computed at :1621-1635;
 * previous_landmark[k] = index of the landmark keypoint k already carries or -1 (:1701-1704).
 * Outputs: landmark index / distance per keypoint, hps_W (4 doubles, written when hp_set[k]:
 * only non-parallel triangulations are stored, :1708-1710) and the count of already-correct
 * matches (ctrs, :1702). */
okvfe_status okvfe_match_to_map_uninitialised(okvfe_ctx* ctx, const uint8_t* desc,
                                              const double* backproj, const uint8_t* use,
                                              const int32_t* previous_landmark, int32_t n_kps,
                                              const int32_t* desc_begin, int32_t n_landmarks,
                                              const uint8_t* pool, const double* e0_W,
                                              const double* r0_W, const okvfe_pose* T_WC1,
                                              double focal_length, int32_t* best_landmark,
                                              int32_t* best_dist, double* hps_W, uint8_t* hp_set,
                                              int32_t* already_matched);

typedef struct okvfe_candidate {
  int32_t i, j, dist;
} okvfe_candidate;
/* All (i, j) with popcnt(A[i]^B[j]) < threshold, ordered by (i, j); host buffers.
 * n_out receives the total found even when it exceeds cap (then OKVFE_ERR_CAPACITY). */
okvfe_status okvfe_hamming_candidates(okvfe_ctx* ctx, const uint8_t* A, int32_t nA,
                                      const uint8_t* B, int32_t nB, int32_t threshold,
                                      okvfe_candidate* out, int32_t cap, int32_t* n_out);
/* Per row of A the first-lowest j with minimal distance < threshold
 * (= the loop of verifyRecognisedPlace, Frontend.cpp:337-346); -1 if none. */
okvfe_status okvfe_hamming_argmin(okvfe_ctx* ctx, const uint8_t* A, int32_t nA, const uint8_t* B,
                                  int32_t nB, uint32_t threshold, int32_t* best_j,
                                  uint32_t* best_dist);

/* = the descriptor matching of Frontend::verifyRecognisedPlace for ALL old landmarks against one
 * camera of the current frame in one launch (Frontend.cpp:330-355): landmark l owns rows
 * desc_begin[l] .. desc_begin[l+1]-1 of landmark_desc (its descriptors in the insertion order of
 * :318-326); per landmark the running minimum over (descriptor, k) with strict <.  k_min[l] = 0 and
 * dist_min[l] = match_threshold when nothing is below the threshold ("distMin < threshold" fails). */
okvfe_status okvfe_verify_place_match(okvfe_ctx* ctx, const uint8_t* landmark_desc,
                                      const int32_t* desc_begin /* n_landmarks + 1 */,
                                      int32_t n_landmarks, const uint8_t* frame_desc, int32_t n_kps,
                                      int32_t* k_min, uint32_t* dist_min);

/* = DBoW2::TemplatedVocabulary<FBrisk::TDescriptor, FBrisk>::transform for n features (the
 * quantisation behind dBow_->database.add / query, Frontend.cpp:756-766): descend from the root
 * (node 0), at every level the child with the smallest FBrisk::distance (FBrisk.cpp:64-67; first
 * child on ties), down to a leaf.  Tree in arrays: node i's children are
 * child_index[child_begin[i] .. child_begin[i+1]); node_word[i] = word id of a leaf, < 0 for an
 * inner node; node descriptors n_nodes x 48 (the root's row is unused).  Nodes must be numbered
 * parents-first (as in DBoW2 files).  Outputs per feature: word id and (optional) leaf node. */
okvfe_status okvfe_fbrisk_transform(okvfe_ctx* ctx, const uint8_t* descriptors, int32_t n,
                                    const uint8_t* node_descriptors, int32_t n_nodes,
                                    const int32_t* child_begin, const int32_t* child_index,
                                    const int32_t* node_word, int32_t* word_ids, int32_t* leaf_nodes);

/* = the weighting / normalisation half of DBoW2::TemplatedVocabulary::transform(features, BowVector)
 * (behind dBow_->database.add / query, Frontend.cpp:756-766), for the word ids okvfe_fbrisk_transform
 * returned: TF_IDF / TF (weighting 0 / 1) sum the word's stored weight per occurrence in feature
 * order, IDF / BINARY (2 / 3) keep the first; words of weight <= 0 are skipped; with
 * normalise_l1 != 0 (the L1 scoring of the shipped vocabulary) the vector is divided by its L1 norm
 * (summed in ascending word order), otherwise TF_IDF / TF divide by the number of distinct words.
 * Host helper (a few thousand features at most).  Output: ascending word ids + values; n_out is the
 * number of distinct words even when it exceeds cap (then OKVFE_ERR_CAPACITY). */
okvfe_status okvfe_bow_vector(const int32_t* word_ids, int32_t n_features, const double* word_weight,
                              int32_t n_words, int32_t weighting, int32_t normalise_l1,
                              int32_t* ids_out, double* values_out, int32_t cap, int32_t* n_out);
/* = DBoW2::TemplatedDatabase::query with L1 scoring (queryL1) against ALL stored entries in one
 * launch: entry e owns db_ids / db_values [db_begin[e], db_begin[e+1]) (ascending word ids, the
 * BowVector it was added with).  Per entry, over the common words in ascending word order:
 * value += |q - d| - |q| - |d|, score = -value / 2 (1 = identical, 0 = nothing in common) -- the
 * same additions in the same order as the inverted-file walk of the reference, so the doubles are
 * bit-identical.  scores[e] = -1 for entries without a common word (DBoW2 does not list them).
 * The reference then sorts the listed entries by id (Frontend.cpp:760-765): this array is already
 * in id order. */
okvfe_status okvfe_bow_query_l1(okvfe_ctx* ctx, const int32_t* db_begin /* n_entries + 1 */,
                                const int32_t* db_ids, const double* db_values, int32_t n_entries,
                                const int32_t* q_ids, const double* q_values, int32_t n_q,
                                double* scores /* n_entries */);

/* = brisk::Hamming::PopcntofXORed(a, b, n128); host, no context. */
uint32_t okvfe_popcnt_xor(const uint8_t* a, const uint8_t* b, int32_t n128);

/* ---- data formats either side of the path (host, no context) ------------- */
/* Text records of OKVIS2 map files, one line per keypoint:
 *   "FRAME:KEYPOINT <stateId> <cameraIdx> <x> <y> <size> BRISK2 <96 hex digits>\n"
 * (okvis::Component::save, okvis_ceres/src/Component.cpp:448-460, precision 17 from :409).
 * out == NULL queries the size; *written always receives the bytes needed. */
okvfe_status okvfe_format_keypoint_lines(uint64_t state_id, uint64_t camera_idx,
                                         const okvfe_keypoint* keypoints,
                                         const uint8_t* descriptors, int32_t n, char* out,
                                         size_t cap, size_t* written);
/* Reads one block of such lines (same stateId / cameraIdx; stops at the first other line), as
 * okvis::Component::load does before MultiFrame::resetKeypoints / resetDescriptors
 * (Component.cpp:235-266).  Descriptor kinds other than BRISK2 -> OKVFE_ERR_UNSUPPORTED. */
okvfe_status okvfe_parse_keypoint_lines(const char* text, size_t len, uint64_t* state_id,
                                        uint64_t* camera_idx, okvfe_keypoint* keypoints,
                                        uint8_t* descriptors, int32_t cap, int32_t* n_out,
                                        size_t* consumed);
/* = DBoW2::FBrisk::meanValue (okvis_frontend/src/FBrisk.cpp:25-58): bitwise majority of n
 * 48-byte descriptors (bit set iff more than n/2 descriptors have it). */
okvfe_status okvfe_fbrisk_mean(const uint8_t* descriptors, int32_t n, uint8_t* mean48);

/* ---- cross-camera gather block (multi-GPU) -------------- */
/* Fixed-size per-image record for the RCCL all-gather: {count, keypoints,
 * descriptors, back-projections, valid flags}; size depends only on
 * max_keypoints. */
size_t okvfe_gather_block_bytes(const okvfe_ctx* ctx);
/* Packs images first_index .. first_index+n-1 of the last batch into n contiguous blocks
 * (stride okvfe_gather_block_bytes) with one kernel. */
okvfe_status okvfe_pack_gather_blocks_device(okvfe_ctx* ctx, int32_t first_index, int32_t n,
                                             void* blocks_dev, void* stream);
/* Matches frame f of blocks0 with frame f of blocks1 for f < n_frames in one launch (both arrays
 * contiguous with the block stride); matches_dev: [n_frames][max_keypoints]. */
okvfe_status okvfe_match_stereo_blocks_batch_device(okvfe_ctx* ctx, const void* blocks0_dev,
                                                    const void* blocks1_dev, int32_t n_frames,
                                                    const okvfe_pose* T_WC0,
                                                    const okvfe_pose* T_WC1, double f0, double f1,
                                                    okvfe_stereo_match* matches_dev, void* stream);
/* Packs image `index` of the last batch into block_dev (device). */
okvfe_status okvfe_pack_gather_block_device(okvfe_ctx* ctx, int32_t index, void* block_dev,
                                            void* stream);
/* Device-resident variant of okvfe_match_motion_stereo: block0 = older frame, block1 = current
 * frame, both gather blocks of camera slot `cam` (intrinsics from okvfe_set_camera; frame size =
 * the context's).  skip0_dev / matched1_dev: device flag arrays [max_keypoints] or NULL.
 * matches_dev: [max_keypoints] okvfe_motion_match, rows >= the block's keypoint count untouched.
 * Nothing crosses PCIe but the two poses. */
okvfe_status okvfe_match_motion_stereo_blocks_device(okvfe_ctx* ctx, int32_t cam,
                                                     const void* block0_dev,
                                                     const void* block1_dev,
                                                     const uint8_t* skip0_dev,
                                                     const uint8_t* matched1_dev,
                                                     const okvfe_pose* T_WC0,
                                                     const okvfe_pose* T_WC1,
                                                     okvfe_motion_match* matches_dev, void* stream);
/* The same for n_pairs (older frame, current frame, camera) triples in ONE launch, and -- with `claim` -- the part of
 * matchMotionStereo's insertion loop that depends on frame data alone, so that the sweep of a current multiframe over
 * its older keyframes (Frontend.cpp:1773-1775), for a whole batch of current frames, is queued without the host
 * waiting for anything.
 *
 * Matching = Frontend.cpp:1789-1905.  Pair p matches older block idx0[p] of blocks0_dev (frame 0) against current
 * block idx1[p] of blocks1_dev (frame 1), both arrays contiguous with the stride okvfe_gather_block_bytes, with the
 * camera of slot cam_ids[p] (okvfe_set_camera; f0 = 0.5 (fu + fv) of the slot, :1786).  Row (p, k0) of matches_dev
 * [n_pairs][K], K = okvfe_device_outputs.max_keypoints, holds the bytes okvfe_match_motion_stereo_blocks_device writes
 * for that pair given row p of skip0_dev [n_pairs][K] (pair-major) and row idx1[p] of matched1_dev [n_blocks1][K]
 * (indexed by the CURRENT block); either array may be NULL.  Rows at or past the older block's count are untouched.
 * The same older block may appear in several pairs.  idx0 / idx1 NULL = the identity (pair p uses block p).
 *
 * Claims = Frontend.cpp:1915-1958 restricted to frame data.  Row (p, k0) is a candidate iff k0 < count0, k1 >= 0 and
 * accepted != 0 (a skipped k0 has k1 == -1, so the re-checks at :1923-1933 add nothing).  Candidates are visited in
 * ascending k0 (:1916); a candidate is claimed iff its k1 is free: matched1_out is NULL or
 * matched1_out[idx1[p] K + k1] == 0 when the claim kernel starts, and no candidate with a smaller k0 of this pair has
 * the same k1 (:1935-1938) -- for each free k1 the candidate with the smallest k0 wins.  n_claimed[p] counts the
 * winners (the pair's share of retCtr, :1957); matched1_out gets 1 at the winners' k1 (:1954) and is otherwise
 * unchanged.  Pairs are resolved in parallel, so a call with claim != NULL must not name a current block twice
 * (OKVFE_ERR_INVALID_ARGUMENT, the block and both pairs named); without claim repeats are allowed: one frozen
 * matched1 against many older frames.  With claim, K above 12288 is OKVFE_ERR_UNSUPPORTED (the per-pair owner table of
 * 4 K bytes stays within 48 KB of LDS); matching alone has no such limit.
 *
 * What stays with the caller: skip0 stands for the estimator-state tests of :1814-1841.  An earlier step of a sweep
 * can initialise a landmark that a keypoint of a later older frame carries; the quality comparison at :1943
 * (lm.quality < acos(cos_quality)) and setLandmark / addLandmark / addObservation (:1940-1956) need estimator state
 * and a libm acos.  A caller that needs that coupling refreshes its skip0 rows between the calls, on the device or the
 * host; with skip0 fixed up front the sweep equals the reference whenever no such landmark exists.  A landmark observed
 * by two keypoints of one older image is not modelled.  The order of the older frames (:1751-1767) is
 * okvfe_overlap_pairs_blocks_device + okvfe_overlap_fraction + okvfe_motion_frame_order, whose output fills the host
 * idx0 / idx1 of this call; which frames are candidates (allFrames, isKeyframe: :1742-1749) stays with the caller.
 * The consensus of runRansac2d2d (:1964-1969, before initialisation only) is
 * okvfe_ransac2d2d_consensus_blocks_device, queued after each step of the sweep; its sampler and minimal solvers are
 * the caller's.
 *
 * An index outside [0, n_blocks*), a NULL required pointer, a negative count, a camera slot out of range or without
 * intrinsics (the pair and the slot named): OKVFE_ERR_INVALID_ARGUMENT before anything is launched.  n_pairs == 0 is OK
 * and launches nothing.  One record per pair (256 bytes) goes through the pinned parameter ring; nothing synchronises
 * the host. */
typedef struct okvfe_motion_claim_device { /* every member device memory; the struct pointer may be NULL */
  uint8_t* claimed;      /* n_pairs x K: 1 = row (p, k0) is inserted by :1915-1958, 0 = not; rows >= count0 untouched */
  int32_t* n_claimed;    /* n_pairs: the pair's contribution to retCtr (:1957); written, not accumulated */
  uint8_t* matched1_out; /* n_blocks1 x K or NULL: byte k1 of the pair's CURRENT block becomes 1 where claimed;
                          * may be matched1_dev itself (the in-place sweep) */
} okvfe_motion_claim_device;
okvfe_status okvfe_match_motion_stereo_blocks_batch_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_blocks0, const void* blocks1_dev, int32_t n_blocks1,
    int32_t n_pairs, const int32_t* idx0 /* HOST n_pairs or NULL = p */, const int32_t* idx1 /* HOST or NULL = p */,
    const int32_t* cam_ids /* HOST n_pairs */, const okvfe_pose* T_WC0 /* HOST n_pairs */,
    const okvfe_pose* T_WC1 /* HOST n_pairs */, const uint8_t* skip0_dev /* n_pairs x K, pair-major, or NULL */,
    const uint8_t* matched1_dev /* n_blocks1 x K, indexed by CURRENT block, or NULL */,
    okvfe_motion_match* matches_dev /* n_pairs x K */, const okvfe_motion_claim_device* claim, void* stream);
/* Matches two gathered blocks (device), as okvfe_match_stereo_batch_device. */
okvfe_status okvfe_match_stereo_blocks_device(okvfe_ctx* ctx, const void* block0_dev,
                                              const void* block1_dev, const okvfe_pose* T_WC0,
                                              const okvfe_pose* T_WC1, double f0, double f1,
                                              okvfe_stereo_match* matches_dev, void* stream);

/* ---- sampling pattern as data ------------------------------------------------ */
/* The extractor's sampling pattern is DATA.  The pattern the library builds at okvfe_create carries
 * BRISK2's pair table and bit order as recovered from the 819 real BRISK2 descriptors of the
 * reference's vocabulary (66 sample points, 384 live bits; tools/pattern/README.md, INTEGRATION.md
 * section 0) on the published BRISK ring radii and smoothing widths, which the reference tree cannot
 * confirm (its `brisk` submodule is empty).  A pattern dumped from a real brisk build -- sample
 * offsets, smoothing half-widths, the short pairs IN BIT ORDER, the long pairs of the orientation
 * estimate -- is installed with okvfe_set_pattern and replaces it without touching a kernel.
 * Limits of the kernels: <= 72 sample points, <= 384 short pairs (bit b of the 48-byte row =
 * value[short_i[b]] > value[short_j[b]]; unused bits stay 0), <= 1100 long pairs, border >= the farthest
 * sample + its half-width + 1.  okvfe_set_pattern synchronises the context.
 * Which descriptor kernel serves a pattern (okvfe_pattern_kernel_class): a wave has 64 lanes, and lane l samples
 * point (n_points - 64) + l; the FIRST n_points - 64 points of a pattern with more than 64 are the extra samples
 * (evaluated beside the wave), so put the smallest boxes first -- the built-in pattern has the centre and one
 * hexagon point there.
 *   class 0: extra samples' half-width < 2.0 (5 x 5 row slots; in float32 a box of exactly 2.0 can span 6 pixels),
 *            all others <= 4.75 (11 x 11): the fast kernels;
 *   class 1: <= 4.25 / <= 9.75 (10 x 10 / 21 x 21 row slots): the WIDE instantiations of the same kernels;
 *   class 2: wider still, or any half-width below 0.5 (bilinear point samples): the all-modes kernel with plain
 *            box loops -- correct for every pattern, several times slower. */
#define OKVFE_PATTERN_POINTS 72
#define OKVFE_PATTERN_SHORT_PAIRS 384
#define OKVFE_PATTERN_LONG_PAIRS 1100
typedef struct okvfe_pattern {
  int32_t n_points;
  float px[OKVFE_PATTERN_POINTS], py[OKVFE_PATTERN_POINTS]; /* offsets from the keypoint, upright, px */
  float sigma_half[OKVFE_PATTERN_POINTS];                   /* half side of the smoothing box */
  int32_t n_short;
  uint8_t short_i[OKVFE_PATTERN_SHORT_PAIRS], short_j[OKVFE_PATTERN_SHORT_PAIRS];
  int32_t n_long;
  uint8_t long_i[OKVFE_PATTERN_LONG_PAIRS], long_j[OKVFE_PATTERN_LONG_PAIRS];
  int32_t long_wdx[OKVFE_PATTERN_LONG_PAIRS], long_wdy[OKVFE_PATTERN_LONG_PAIRS]; /* round(2048 d / |d|^2) */
  int32_t border; /* keypoints closer than this to the image rim are removed */
} okvfe_pattern;
okvfe_status okvfe_get_pattern(const okvfe_ctx* ctx, okvfe_pattern* out);
okvfe_status okvfe_set_pattern(okvfe_ctx* ctx, const okvfe_pattern* pattern);
/* 0 / 1 / 2 as above for the pattern installed now (after okvfe_create's box_scale or okvfe_set_pattern); -1: ctx NULL */
int32_t okvfe_pattern_kernel_class(const okvfe_ctx* ctx);

/* ---- device-resident, batched map matchers ---------------------------------- */
/* The map-side loops of the front-end on data that never leaves the GPU: frame f of the batch is
 * gather block f (okvfe_pack_gather_blocks_device: keypoints, descriptors, back-projections and the
 * keypoint count of one image), the pooled landmark set lives in device memory, ONE launch serves
 * all frames, nothing synchronises the host.  Row capacity of every per-keypoint array = the
 * context's okvfe_device_outputs.max_keypoints (K); rows >= a frame's keypoint count are untouched.
 * The pooled set is what okvfe_match_to_map / okvfe_match_to_map_uninitialised take, as device
 * pointers (e.g. uploaded once per keyframe with okvfe_copy_to_device). */
typedef struct okvfe_map_device {
  int32_t n_landmarks;        /* L */
  const int32_t* desc_begin;  /* device, L + 1: landmark l owns pool rows desc_begin[l] .. desc_begin[l+1]-1 */
  const uint8_t* pool;        /* device, desc_begin[L] x 48 pooled descriptors */
  const double* projections;  /* device, n_frames x L x 2 (frame-major): 3-D landmarks projected into frame f
                               * (Frontend.cpp:1232-1256); only okvfe_match_to_map_blocks_device reads it */
  const double* e0_W;         /* device, desc_begin[L] x 3: observing unit ray per pool row (LandmarkToMatch::e_W) */
  const double* r0_W;         /* device, desc_begin[L] x 3: observing camera centre per pool row */
} okvfe_map_device;
/* = Frontend::matchToMapByThread (Frontend.cpp:1552-1589) for n_frames frames.  use_dev: device
 * n_frames x K flags or NULL (every keypoint).  Outputs (device, n_frames x K): landmark index
 * (-1 = none) and distance (match_threshold if none).  The call keeps the frames' keypoint order in a workspace
 * of its own per stream (ABI 6), so calls on different streams of one context may be in flight together, like
 * every other entry point of the batch API (the host side of a context is still one thread at a time). */
okvfe_status okvfe_match_to_map_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                              const uint8_t* use_dev, const okvfe_map_device* map,
                                              double reprojection_threshold, int32_t* best_landmark_dev,
                                              int32_t* best_dist_dev, void* stream);
/* = Frontend::matchToMapByThreadUnitialised (Frontend.cpp:1616-1719) for n_frames frames.
 * T_WC1: HOST array of n_frames poses (the one thing that crosses PCIe: 96 bytes per frame, through
 * the context's pinned parameter ring); previous_landmark_dev: device n_frames x K or NULL (-1);
 * outputs device: best_landmark / best_dist n_frames x K, hps_W n_frames x K x 4, hp_set
 * n_frames x K, already_matched n_frames (zeroed by this call). */
okvfe_status okvfe_match_to_map_uninitialised_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                                            const uint8_t* use_dev, const int32_t* previous_landmark_dev,
                                                            const okvfe_map_device* map, const okvfe_pose* T_WC1,
                                                            double focal_length, int32_t* best_landmark_dev,
                                                            int32_t* best_dist_dev, double* hps_W_dev, uint8_t* hp_set_dev,
                                                            int32_t* already_matched_dev, void* stream);
/* = the descriptor matching of Frontend::verifyRecognisedPlace (Frontend.cpp:330-355) of all L old
 * landmarks against n_frames frames.  Outputs device n_frames x L as okvfe_verify_place_match. */
okvfe_status okvfe_verify_place_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                              const okvfe_map_device* map, int32_t* k_min_dev,
                                              uint32_t* dist_min_dev, void* stream);

/* ---- matchToMap from the raw landmark table, device-resident and batched -------------------
 * okvfe_match_to_map_landmarks for n_frames frames against ONE landmark table that lives in device memory: the table
 * is uploaded when the map changes (at keyframes: okvfe_device_alloc / okvfe_copy_to_device), every frame then costs
 * one call that uploads 112 bytes per frame (pose, camera slot) through the pinned parameter ring and synchronises
 * nothing.  Frame f = gather block f; its result is exactly what okvfe_match_to_map_landmarks returns for that frame's
 * keypoints with T_WC1[f], camera slot cam_ids[f], the same threshold and the same `exclusive`: projection, view
 * pooling and the three-slot buffer depend on the frame's pose, so every frame gets a pooled set of its own
 * (okvfe_match_to_map_blocks_device shares one set among all frames and takes the projections from the caller).
 *
 * okvfe_landmark_table with every pointer a DEVICE pointer (obs_desc 16-byte aligned, as okvfe_device_alloc returns
 * it).  The matcher does not check the table: call okvfe_landmark_table_check_device once per upload.  An unchecked,
 * malformed table (obs_begin not monotone or outside [0, n_observations], a pose index outside [0, n_poses)) is
 * undefined behaviour, exactly as a bad device pointer is. */
typedef struct okvfe_landmark_table_device {
  int32_t n_landmarks, n_observations, n_poses;
  const double* hp_W;
  const double* quality;
  const int32_t* obs_begin;
  const int32_t* obs_pose;
  const uint8_t* obs_desc;
  const double* obs_backproj;
  const okvfe_pose* poses;
} okvfe_landmark_table_device;

/* okvfe_landmark_pool per frame: device arrays, frame-major n_frames x L rows (obs_rows x 3, projection x 2, e_W / r_W
 * x 6), holding the bytes of the B = 1 call's okvfe_landmark_pool: landmarks that are not kept are zero and their
 * obs_rows -1.  The struct pointer and every member may be NULL.  status, n_desc, obs_rows, e_W and r_W stay on the
 * device: they are the input of okvfe_match_to_map_table_uninitialised_blocks_device, the batched second pass over the
 * landmarks that are not 3-D yet. */
typedef struct okvfe_landmark_pool_device {
  int32_t* status;
  int32_t* n_desc;
  int32_t* obs_rows;
  double* projection;
  double* e_W;
  double* r_W;
} okvfe_landmark_pool_device;

/* The structural checks okvfe_match_to_map_landmarks runs on its host arrays, by one kernel on the device table.  The
 * ONLY call of this group that synchronises the host; meant to run once per upload.  OKVFE_ERR_INVALID_ARGUMENT and an
 * okvfe_last_error that names the first offending row ("obs_begin not monotone at L", "observation O: pose index out of
 * range") if the table is malformed. */
okvfe_status okvfe_landmark_table_check_device(okvfe_ctx* ctx, const okvfe_landmark_table_device* table, void* stream);

/* cam_ids, T_WC1: HOST arrays of n_frames camera slots (with intrinsics: okvfe_set_camera; else OKVFE_ERR_NOT_READY)
 * and poses.  use_dev: device n_frames x K flags or NULL (every keypoint).  Outputs (device, n_frames x K):
 * best_landmark = row of the TABLE (-1 = none), best_dist (match_threshold if none); rows at or past a block's keypoint
 * count are untouched; with n_landmarks == 0 the rows below it still receive -1 / match_threshold.  Ties: the first
 * landmark in ascending table order, pooled row 0 before row 1 (the cropped third row never matches).  Both orders of
 * okvfe_set_fp64_reduction apply.
 * Nothing synchronises the host.  The workspace (32 bytes per (frame, landmark) pair plus the keypoint order) is kept
 * per stream, so calls on different streams of one context may be in flight together; growing it or the parameter
 * ring -- the first call on a stream, or a larger batch -- frees the old buffer, which waits for the device once.  A call that would need more
 * than 1 GiB of workspace runs its frames in slices, one after another on the same stream.
 * A NULL or negative argument: OKVFE_ERR_INVALID_ARGUMENT before anything is launched.
 * The second pass of Frontend::matchToMap over the landmarks that are not 3-D yet is
 * okvfe_match_to_map_table_uninitialised_blocks_device below, on what pool_out leaves on the device.  Between the two
 * passes (Frontend.cpp:1411-1430): okvfe_ransac3d2d_consensus_blocks_device and okvfe_remove_outliers_blocks_device
 * further below, their hypotheses from okvfe_ransac3d2d_hypotheses_blocks_device (a defined sampler and P3P, not
 * opengv's).  Not covered: optimiseRealtimeGraph. */
okvfe_status okvfe_match_to_map_table_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const void* blocks_dev, int32_t n_frames,
    const int32_t* cam_ids /* HOST, n_frames */, const okvfe_pose* T_WC1 /* HOST, n_frames */,
    double reprojection_threshold, int32_t exclusive, const uint8_t* use_dev /* n_frames x K or NULL */,
    const okvfe_landmark_pool_device* pool_out, int32_t* best_landmark_dev, int32_t* best_dist_dev, void* stream);

/* The second pass of Frontend::matchToMap (Frontend.cpp:1434-1496): matchToMapByThreadUnitialised (:1594-1720) for
 * n_frames frames, each over the landmarks that ITS first pass left as not 3-D yet, with the pose as it is NOW (after
 * RANSAC and optimiseRealtimeGraph, which stay with the caller).  table: the table of the first pass; pool: what
 * okvfe_match_to_map_table_blocks_device wrote for these frames (device, n_frames x L, L = table->n_landmarks).
 *
 * Landmark set of frame f: the landmarks l with pool->status[f L + l] == 2, in ascending table order.  Landmark l has
 * pool->n_desc[f L + l] (1 or 2) pooled descriptors: the rows pool->obs_rows[3 (f L + l) + d] of table->obs_desc (the
 * cropped third row is never read); pooled row d carries the ray pool->e_W[6 (f L + l) + 3 d ..] and the centre
 * pool->r_W[6 (f L + l) + 3 d ..].  pool->projection is not read and may be NULL; the other five members are required
 * when L > 0 (else OKVFE_ERR_INVALID_ARGUMENT).  Of the table only obs_desc and n_landmarks are read.  The pool is not
 * checked: a malformed pool (a row outside obs_desc) is undefined behaviour, as a malformed table is.
 *
 * Keypoint k of block f takes part iff k < count, the block's backproj_valid[k] != 0 (:1625), use_dev == NULL or
 * use[k] != 0, and exclusive != 0 or previous[k] < 0 (:1630): the first pass's best_landmark_dev may be passed as
 * previous_landmark_dev unchanged.  previous: device n_frames x K TABLE rows (-1 = none) or NULL (none).
 *
 * cam_ids, T_WC1: HOST arrays of n_frames camera slots and poses.  sigma = 1 / (0.5 (fu + fv)) of slot cam_ids[f];
 * cos(2.6 sigma) and cos(6 sigma) are computed on the host (std::cos); a slot without intrinsics:
 * OKVFE_ERR_NOT_READY, the frame and the slot named.  One record per frame (240 bytes) goes through the pinned
 * parameter ring.
 *
 * Gate chain, acceptance and outputs are those of okvfe_match_to_map_uninitialised_blocks_device: epipolar plane and
 * divergence (unless nearly parallel), triangulateFast, not within 0.2 m of either centre; a gated hit on the landmark
 * the keypoint carries (previous, with exclusive != 0) is counted in already_matched[f], ends that landmark's descriptor
 * loop and is never accepted; `<` is strict (the first pooled row in table order reaching the smallest distance); hps_W
 * is stored, and hp_set is 1, only when the winning triangulation is not parallel.  best_landmark = row of the TABLE.
 * Outputs (device): best_landmark / best_dist n_frames x K, hps_W n_frames x K x 4, hp_set n_frames x K,
 * already_matched n_frames (zeroed by this call).  Rows at or past a block's count are untouched; with L == 0 or an
 * empty set the rows below it still receive -1, match_threshold, a zero hp and hp_set 0.  Both orders of
 * okvfe_set_fp64_reduction apply.
 * Nothing synchronises the host.  The workspace (16 bytes per (frame, landmark) pair plus 4 per frame) is the
 * per-stream one of the first pass; a call above its limit runs in slices of frames.  A NULL or negative argument:
 * OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_frames == 0 is OK and launches nothing. */
okvfe_status okvfe_match_to_map_table_uninitialised_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const okvfe_landmark_pool_device* pool,
    const void* blocks_dev, int32_t n_frames, const int32_t* cam_ids /* HOST, n_frames */,
    const okvfe_pose* T_WC1 /* HOST, n_frames */, int32_t exclusive, const uint8_t* use_dev /* n_frames x K or NULL */,
    const int32_t* previous_landmark_dev /* n_frames x K or NULL */, int32_t* best_landmark_dev, int32_t* best_dist_dev,
    double* hps_W_dev, uint8_t* hp_set_dev, int32_t* already_matched_dev, void* stream);

/* ---- between matchToMap's two passes: RANSAC consensus and outlier removal ------------------
 * The consensus step of Frontend::runRansac3d2d (Frontend.cpp:2208-2261) for n_multiframes multiframes of n_cams
 * cameras each: multiframe m owns the gather blocks m n_cams + c, c = 0 .. n_cams - 1, and the rows
 * (m n_cams + c) K .. of landmark_dev (device, TABLE rows, -1 = none; the first pass's best_landmark_dev as it is).
 * cam_ids, T_SC: HOST arrays of n_cams camera slots (with intrinsics, else OKVFE_ERR_NOT_READY) and sensor-from-camera
 * poses (p_S = C p_C + r), one rig per call as the adapter takes frame->T_SC(im).  Of the table hp_W, obs_begin and
 * n_landmarks are read.
 *
 * Correspondences (FrameNoncentralAbsoluteAdapter.cpp:50-148), camera-major with keypoints ascending: keypoint k of
 * block (m, c) with k < count and l = landmark[k] >= 0, unless fabs(hp_W[4 l + 3]) < 1.0e-8 (:116; a NaN stays in) or
 * the landmark has no observation in the table, obs_begin[l + 1] - obs_begin[l] < 1.  The reference asks for
 * observations.size() >= 2 (:109) AFTER the frame added its own observation at Frontend.cpp:1404; the table holds the
 * observations before that, so one is the floor here.  A row l >= n_landmarks is no correspondence.  Point
 * p = hp.head<3>() / hp[3]; bearing = the block's back-projection, or (1, 0, 0) where backproj_valid[k] == 0
 * (:129-132), normalised as Eigen's normalize() (z = squaredNorm; divided by sqrt(z) iff z > 0);
 * sigma = ((sqrt2 s) s) / (fu fu), s = (0.8 double(size)) / 12.0, fu of slot cam_ids[c] (:128, 135).
 *
 * hypotheses_dev: n_multiframes x n_hyp x 12 doubles, each a row-major 3 x 4 [R | t] = T_WS (ransac.model_coefficients_);
 * hyp_valid_dev: n_multiframes x n_hyp bytes or NULL (all valid), 0 = a sample whose solver failed (opengv skips it).
 * n_hyp in 1 .. OKVFE_RANSAC_MAX_HYPOTHESES (the reference: max_iterations_ 50); threshold: the reference's 16.
 * Distance (FrameAbsolutePoseSacProblem.hpp:140-165): Ri = R^T, ti = (-Ri) t, body = Ri p + ti (four terms),
 * rep = C_SC^T (body - r_SC), rep /= |rep|, e = rep - bearing, dist = e.e / sigma; inlier iff dist < threshold (a NaN
 * is an outlier).  Three- and four-term sums follow okvfe_set_fp64_reduction: Eigen's x0 + (x1 + x2) and
 * (x0 + x1) + (x2 + x3), or left to right.
 *
 * Verdict (Frontend.cpp:2226, 2242-2261): with fewer than 10 correspondences nothing is scored (best_hypothesis -1,
 * n_inliers 0, accepted 0).  Otherwise the winner is the valid hypothesis with the most inliers, more than 0, the first
 * such in list order; accepted = n_inliers >= 10 && double(n_inliers) / double(n_correspondences) > 0.7.  The winning
 * pose is hypotheses[best_hypothesis], which the caller owns.
 *
 * NOT restated: opengv's gp3p and its rand() sampler.  okvfe_ransac3d2d_hypotheses_blocks_device (further below)
 * offers a defined sampler and a central P3P in their place, under the deviations stated there; a caller may as well
 * bring hypotheses of its own.  Nor opengv's adaptive stop, which only ever shortens the list (this call scores every hypothesis
 * it is given).  PARITY UNPINNED: opengv is not in the reference tree; the winner rule (replace on strictly more
 * inliers) is restated from the published source of opengv::sac::Ransac::computeModel.
 *
 * Results (device; each optional one may be NULL): n_correspondences / best_hypothesis / n_inliers int32 and accepted
 * u8 per multiframe; optional hyp_inliers n_multiframes x n_hyp (-1: skipped or, below 10 correspondences, not scored);
 * optional state blocks x K (0 no correspondence, 1 outlier of the winner, 2 inlier; only 0 and 1 without a winner);
 * optional distance blocks x K (the winner's distance at correspondences; untouched elsewhere and without a winner);
 * optional landmark_out blocks x K, which may be landmark_dev itself: the input, -1 where accepted && remove_outliers
 * && state == 1.  Rows at or past a block's keypoint count are untouched.
 * Nothing synchronises the host; no workspace; 112 bytes per camera go through the pinned parameter ring.  A NULL or
 * negative argument: OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_multiframes == 0 is OK and launches
 * nothing. */
#define OKVFE_RANSAC_MAX_HYPOTHESES 64
typedef struct okvfe_ransac_result_device {
  int32_t* n_correspondences;
  int32_t* best_hypothesis;
  int32_t* n_inliers;
  uint8_t* accepted;
  int32_t* hyp_inliers;  /* optional */
  uint8_t* state;        /* optional */
  double* distance;      /* optional */
  int32_t* landmark_out; /* optional */
} okvfe_ransac_result_device;
okvfe_status okvfe_ransac3d2d_consensus_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const void* blocks_dev, int32_t n_multiframes,
    int32_t n_cams, const int32_t* cam_ids /* HOST, n_cams */, const okvfe_pose* T_SC /* HOST, n_cams */,
    const int32_t* landmark_dev, const double* hypotheses_dev, const uint8_t* hyp_valid_dev /* or NULL */, int32_t n_hyp,
    double threshold, int32_t remove_outliers, const okvfe_ransac_result_device* result, void* stream);

/* Frontend::removeOutliers (Frontend.cpp:2152-2205) for n_frames frames (frame f = gather block f).  cam_ids, T_WC:
 * HOST arrays of n_frames camera slots and poses, T_WC = T_WS T_SC as the caller's Transformation class computes it.
 * Of the table hp_W and n_landmarks are read (hp_W may point at refreshed positions after the caller's optimisation).
 * Per keypoint k < count with l = landmark[k] in [0, n_landmarks): hp_C = T_WC^-1 hp_W in the expression order of the
 * first pass, projectHomogeneous (the head negated when hp_C[3] < 0), the camera's project; the row becomes -1 iff the
 * status is not Successful or sqrt(dx dx + dy dy) > max_error (the reference's 4.0), dx = projection - double(keypoint);
 * a NaN norm is kept.  kept_dev[f] (int32, zeroed by this call) counts the kept ones: the reference's return value.
 * Rows with l < 0 (or outside the table) pass through; rows at or past the count are untouched.  landmark_out_dev may
 * be landmark_dev.  Nothing synchronises the host; 112 bytes per frame go through the pinned parameter ring. */
okvfe_status okvfe_remove_outliers_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const void* blocks_dev, int32_t n_frames,
    const int32_t* cam_ids /* HOST, n_frames */, const okvfe_pose* T_WC /* HOST, n_frames */, double max_error,
    const int32_t* landmark_dev, int32_t* landmark_out_dev, int32_t* kept_dev, void* stream);

/* ---- before initialisation: the consensus of runRansac2d2d inside the motion-stereo sweep --------
 * The consensus step of Frontend::runRansac2d2d (Frontend.cpp:2281-2394), which runs after every older frame of the
 * matchMotionStereo sweep while the session is not initialised (:1961-1969) and whose rotationOnly decides whether it
 * initialises at all (:644-648), for n_pairs (older multiframe, current multiframe) pairs of n_cams cameras in ONE
 * launch.  Pair p relates older multiframe mf0[p] to current multiframe mf1[p]: the older one owns the gather blocks
 * mf0[p] n_cams + c of blocks0_dev, the current one the blocks mf1[p] n_cams + c of blocks1_dev (the multiframe-major
 * layout of okvfe_ransac3d2d_consensus_blocks_device; the two block pointers may be equal).  Frame 1 of opengv's model
 * is the older one.  landmark0_dev / landmark1_dev: int32, K per block, block-indexed as in
 * okvfe_stereo_insert_blocks_device; a value < 0 is "no landmark" (lmId == 0).  added_dev: n_landmarks bytes,
 * byte l = estimator.isLandmarkAdded(l), an id >= n_landmarks is not added; NULL: every id >= 0 is added.  No landmark
 * table: the adapter reads no 3-D point.  cam_ids: HOST, n_cams camera slots; fu comes from slot cam_ids[c] for both
 * frames (FrameRelativeAdapter.cpp:78-129 reads fu2 from frame A's geometry at camIdB, the same camera here); a slot
 * without intrinsics: OKVFE_ERR_NOT_READY.
 *
 * Correspondences per camera (FrameRelativeAdapter.cpp:137-165):
 *   :139-152  over the CURRENT block's keypoints k < count, ascending: id < 0 skipped (:143), a not-added id skipped
 *             (:147); the FIRST k of an id is kept (:151, std::map::insert does not overwrite).
 *   :154-165  over the OLDER block's keypoints ascending: a keypoint with id >= 0 (:157) whose id is in that map (:160)
 *             gives one correspondence (kA, kB), in older-keypoint order.  Two older keypoints on one landmark give two
 *             correspondences to the same kB.  The older id is NOT tested for isLandmarkAdded.
 * Bearings and sigmas (:168-193): sigma = ((sqrt2 s) s) / (fu fu), s = (0.8 double(size)) / 12.0, per side (:175-176,
 * :186-187), written as in the 3d2d call.  b2 = the current block's stored back-projection, normalised, whatever its
 * validity byte (:189-193: getBackProjection hands out the stored value, Frame.hpp:196-208).  b1 = (1, 0, 0) if EITHER
 * validity byte is 0 (:178-179, and :190 overwrites bearingVectors1_, not 2_: the reference's slip, restated), else the
 * older block's back-projection, normalised.  Normalisation is Eigen's: z = squaredNorm, divided by sqrt(z) iff z > 0.
 *
 * rot_hyp_dev: n_pairs x n_cams x n_hyp x 9 doubles, a row-major rotation M per hypothesis; rel_hyp_dev: ... x 12
 * doubles, a row-major [R12 | t12] (opengv's model).  rot_valid_dev / rel_valid_dev: bytes of the same leading shape or
 * NULL (all valid); 0 = a sample whose solver failed, skipped.  n_hyp in 1 .. OKVFE_RANSAC_MAX_HYPOTHESES (the
 * reference: max_iterations_ 50, :2313, :2330); threshold: the reference's 9 (:2312, :2329).
 * Distances, FP64 without FMA, 3- and 4-term sums in the order of okvfe_set_fp64_reduction:
 *   rotation only (FrameRotationOnlySacProblem.hpp:126-144): f2u = M b2 (:131), f1u = M^T b1 (:134), e1 = f2u - b1
 *     (:136), e2 = f1u - b2 (:137), d = (e1.e1 * 0.5) / s1 + (e2.e2 * 0.5) / s2 (:140-143).
 *   relative pose (FrameRelativePoseSacProblem.hpp:130-160): Ri = R^T (:136), ti = (-Ri) t (:137),
 *     p = triangulate2(b1, b2; R, t) (:143), rep1 = p / |p| (:147), rep2 = Ri p + ti * 1 in four-term rows (:146), then
 *     / |rep2| (:148), e1 = rep1 - b1 (:153), e2 = rep2 - b2 (:154), d as above (:157-160).
 *   triangulate2, with Eigen's 2 x 2 inverse: f2u = R b2; b0 = t . b1, b1' = t . f2u; A00 = b1 . b1, A10 = b1 . f2u,
 *     A01 = -A10, A11 = -(f2u . f2u); det = A00 A11 - A10 A01, invdet = 1.0 / det; I00 = A11 invdet,
 *     I10 = (-A10) invdet, I01 = (-A01) invdet, I11 = A00 invdet; l0 = I00 b0 + I01 b1', l1 = I10 b0 + I11 b1';
 *     p = (l0 b1 + (t + l1 f2u)) / 2.
 * An inlier is d < threshold; a NaN is an outlier (parallel bearings: det == 0, hence a NaN).
 * Winners: per problem the valid hypothesis with the most inliers, more than 0, the first such in list order.
 *
 * Per camera, in order, the two success flags shared by the cameras of a pair as the reference's locals are (:2289-2290):
 *   :2300      n < 10: skipped (branch 0), nothing is scored, added to the total or removed.
 *   :2320,2337 the ratios are float(inliers) / float(n) in FLOAT32, compared with 0.8f.
 *   :2341-2349 rot_ratio > rel_ratio || rot_ratio > 0.8f: branch 1; rotation_only_success iff rot_inliers > 10;
 *              rotationOnly = true; total += rot_inliers.
 *   :2350-2358 else branch 2; rel_pose_success iff rel_inliers > 10 && rel_ratio > 0.8f; total += rel_inliers.
 *   :2361      neither flag set SO FAR (the earlier cameras' included): the camera is done.
 *   :2365-2375 else removed = 1 and, with remove_outliers, every current keypoint kB with at least one correspondence
 *              that is NOT an inlier of the taken branch's winner gets -1 in landmark1_out (without a winner every
 *              correspondence is such a one).  All other rows below the current block's count copy landmark1_dev; rows
 *              at or past the count are untouched.
 *   :2387-2392 either flag set: total_inliers = the total, rotation_only as accumulated; else total_inliers = -1 and
 *              rotation_only = 1.
 * With landmark1_out a current multiframe may appear in at most one pair of a call (OKVFE_ERR_INVALID_ARGUMENT, the
 * multiframe and both pairs named), and its rows must not be the OLDER rows of another pair of the same call: the
 * reference visits the older frames one after another, so J older frames are J calls on one stream.
 *
 * The hypotheses: okvfe_ransac2d2d_hypotheses_blocks_device (further below) writes both lists and their validity bytes
 * on the device, with a defined sampler and defined two-point and five-point solvers (opengv's rand() sampler,
 * twopt_rotationOnly and Stewenius solver are not restated bit for bit).  NOT restated: opengv's adaptive stop (this call
 * scores every hypothesis it is given); estimator.removeObservation beyond the id row; the LOG lines of :2378-2384; firstFrame and rotationOnly_tmp
 * (:1971-1974) and :644, host lines over the result bytes.  PARITY UNPINNED: opengv's winner
 * rule, as for okvfe_ransac3d2d_consensus_blocks_device.  PARITY UNPINNED: opengv::triangulation::triangulate2 and
 * Eigen's 2 x 2 inverse are not in the reference tree; they are restated above from their published sources.
 *
 * Limits: one work-group keeps the id map of a current block in 4096 four-byte slots of LDS, and a probe ends at an
 * empty slot: K = max_keypoints <= 4095, beyond that OKVFE_ERR_UNSUPPORTED.  8 bytes per pair and 8 per camera go through
 * the pinned parameter ring; nothing synchronises the host; no workspace.  A NULL required pointer, a negative count or
 * a multiframe index out of range: OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_pairs == 0 is OK and
 * launches nothing. */
typedef struct okvfe_ransac2d2d_result_device {
  /* per (pair, camera), n_pairs x n_cams */
  int32_t* n_correspondences;
  int32_t* rot_best;  /* winner of the rotation-only problem, -1 = none */
  int32_t* rot_inliers;
  int32_t* rel_best;  /* winner of the relative-pose problem, -1 = none */
  int32_t* rel_inliers;
  uint8_t* branch;    /* 0 skipped (< 10 correspondences), 1 rotation-only taken (:2341), 2 relative pose taken (:2350) */
  uint8_t* removed;   /* 1 = this camera reached :2365 (outliers kicked) */
  /* per pair, n_pairs */
  int32_t* total_inliers; /* the return value: the sum, or -1 (:2387-2392) */
  uint8_t* rotation_only; /* the bool& of :2283 as it is on return (the "hack" at :2391 included) */
  uint8_t* success;       /* bit 0 rotation_only_success, bit 1 rel_pose_success */
  /* optional, NULL allowed */
  int32_t* rot_hyp_inliers; /* n_pairs x n_cams x n_hyp; -1: skipped hypothesis / not scored */
  int32_t* rel_hyp_inliers;
  int32_t* match1;        /* n_pairs x n_cams x K, by OLDER keypoint: the current keypoint of its correspondence, -1 none */
  uint8_t* state;         /* same shape: 0 no correspondence, 1 outlier of the taken branch's winner (or no winner, or the
                           * camera was skipped), 2 inlier */
  double* distance;       /* same shape: distance to the taken branch's winner; untouched without correspondence / winner */
  int32_t* landmark1_out; /* current blocks x K, may be landmark1_dev itself */
} okvfe_ransac2d2d_result_device;
okvfe_status okvfe_ransac2d2d_consensus_blocks_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_multiframes0, const void* blocks1_dev, int32_t n_multiframes1,
    int32_t n_pairs, const int32_t* mf0 /* HOST, n_pairs */, const int32_t* mf1 /* HOST, n_pairs */, int32_t n_cams,
    const int32_t* cam_ids /* HOST, n_cams */, const int32_t* landmark0_dev, const int32_t* landmark1_dev,
    const uint8_t* added_dev /* n_landmarks bytes or NULL */, int32_t n_landmarks, const double* rot_hyp_dev,
    const uint8_t* rot_valid_dev /* or NULL */, const double* rel_hyp_dev, const uint8_t* rel_valid_dev /* or NULL */,
    int32_t n_hyp, double threshold, int32_t remove_outliers, const okvfe_ransac2d2d_result_device* result, void* stream);

/* ---- matchStereo's landmark bookkeeping, chained over the camera pairs of a rig ----------------
 * Frontend::matchStereo after its k0 x k1 loop (Frontend.cpp:2076-2141) for n_multiframes multiframes of n_cams cameras,
 * over n_pairs ordered camera pairs per multiframe, in ONE launch that synchronises nothing.  The matching (:2016-2075)
 * does not read the landmark ids, so all pairs of a rig are matched first (okvfe_match_stereo_blocks_batch_device, one
 * call per pair, pointed at slice p of matches_dev) and this call then resolves the whole chain per multiframe: ids
 * written for pair (0,1) are read by pair (0,2) (":2081 may change!!"), and rows of one pair that matched the same k1 see
 * each other's writes.
 *
 * table: only hp_W and n_landmarks (= L) are read; one table for the whole batch.  initialised_dev: L bytes, byte l =
 * isLandmarkInitialised of table row l (required when L > 0).
 * blocks_dev, block_stride_m, block_stride_c: the gather block of (multiframe m, camera c) is block
 * m block_stride_m + c block_stride_c; (n_cams, 1) is the multiframe-major layout of the RANSAC call, (1, n_multiframes)
 * the camera-major layout of the stereo matcher and the cross-camera gather.  The rows of every per-keypoint array of
 * (m, c) -- landmark_dev, landmark_out -- start at that block index x K.  Two (m, c) on one block, or a negative stride:
 * OKVFE_ERR_INVALID_ARGUMENT.
 * pairs: HOST, n_pairs x 2 camera indices (c0, c1) in the order the reference visits them: im0 ascending, im1 > im0,
 * overlapping pairs only (:1990-2000).  n_pairs in 1 .. OKVFE_STEREO_MAX_PAIRS; c0 == c1 or an index outside the rig:
 * OKVFE_ERR_INVALID_ARGUMENT, the pair named.  cam_ids: HOST, n_cams camera slots (without intrinsics:
 * OKVFE_ERR_NOT_READY, camera and slot named).  T_WC: HOST, n_multiframes x n_cams poses, T_WS T_SC as the caller's
 * Transformation class computes it (:2004-2005); they travel through the pinned parameter ring (96 bytes each).
 * matches_dev: n_pairs x n_multiframes x K okvfe_stereo_match; row (p, m, k0) is what
 * okvfe_match_stereo_blocks_batch_device wrote for pair p of multiframe m.
 * landmark_dev: int32, K per block: TABLE rows, -1 = none, any value outside [-1, L) is read as none (and leaves as -1):
 * the device form of multiFrame->landmarkId, e.g. what the map matchers and the motion sweep left.
 * as_keyframe_dev: n_multiframes bytes, or NULL for all 1 (:2103).
 *
 * Per multiframe exactly the sequential loop: pairs in list order, k0 ascending within a pair.  State: id[c][k] (from
 * landmark_dev) and a per-multiframe view v -> (point, initialised), for v < L starting as (hp_W[v],
 * initialised_dev[v] != 0).  Row (p, k0), k0 < count(c0):
 *  1. k1 = row.k1; k1 < 0 or k1 >= count(c1): action 0, lm -1, done ("distances < briskMatchingThreshold_" is k1 >= 0).
 *  2. id0 = id[c0][k0], id1 = id[c1][k1], as they are at this moment.
 *  3. both set (:2085-2092): lm = id0; if !initialised(id0) && row.initialisable: point(id0) = row.hp_W,
 *     initialised(id0) = true, action |= OKVFE_STEREO_REINIT.
 *  4. only id1 (:2093-2096): lm = id1, add0.   5. only id0 (:2098-2101): lm = id0, add1.
 *  6. neither (:2102-2114): not a keyframe: action 0, lm -1, done.  Else a landmark with id L + p K + k0,
 *     point = row.hp_W, initialised = (row.initialisable != 0); action |= OKVFE_STEREO_CREATE; add0 and add1.  New ids
 *     are not dense: the id names the creating row, whose hp_W is the record.  addLandmark hands out ascending ids in
 *     creation order, so the caller maps creating rows in ascending (p, k0) onto real LandmarkIds.
 *  7. add0 (:2115-2127): hp_C = T_WC0^-1 point(lm) in the expression order of okvfe_remove_outliers_blocks_device,
 *     projectHomogeneous (head negated when hp_C[3] < 0), the project of slot cam_ids[c0]; iff Successful and
 *     sqrt(dx dx + dy dy) < 4.0 (dx, dy = double(keypoint) - projection): id[c0][k0] = lm, action |= OKVFE_STEREO_OBS0.
 *     A NaN norm adds nothing (removeOutliers KEEPS on NaN; this loop does not).
 *  8. add1 (:2128-2140): the same with c1, k1, T_WC1: id[c1][k1] = lm, action |= OKVFE_STEREO_OBS1.
 * The point read in 7 / 8 is the view's at that moment: re-set by an earlier row of any earlier or the same pair, or the
 * creating row's own hp_W.  No input is exempt: several k0 on one k1, a landmark carried by two keypoints of one image, a
 * row whose id0 landmark another k1 carries -- all equal the loop.
 *
 * result (device pointers): action u8 and lm int32, n_pairs x n_multiframes x K, each may be NULL; lm = the landmark the
 * row acted on (-1 for rows without a match or dropped at 6).  landmark_out int32, shaped as landmark_dev and allowed to
 * BE landmark_dev: id after the last pair.  A value >= L names a landmark created here, which is not in the table: the
 * other device calls (RANSAC, removeOutliers, the matchers' `previous`) treat such rows as "no landmark".  counts int32,
 * n_multiframes x 4, written (not accumulated): {rows with a match (past step 1), created, re-initialised, observations
 * added}.  landmark_out and counts are required.  Rows at or past a block's count are untouched in every output.
 *
 * What stays with the caller: hasOverlap and the pair list; T_WS; addLandmark / setLandmark / addObservation /
 * setLandmarkId themselves, replayed from action / lm without any geometry; the refreshed points reach the table at the
 * next upload.  Both orders of okvfe_set_fp64_reduction apply.
 * Limits: one work-group holds the rig's ids and its tables in 65280 bytes of LDS:
 * 4 (n_cams K + P2(n_cams K) + 3 K + P2(2 K)) bytes, P2(x) = the smallest power of two above x; beyond that
 * OKVFE_ERR_UNSUPPORTED (the need and the limit named).  L + n_pairs K must stay below 2^31.  A NULL required pointer or
 * a negative count: OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_multiframes == 0 is OK and launches
 * nothing. */
#define OKVFE_STEREO_MAX_PAIRS 16
#define OKVFE_STEREO_REINIT 1
#define OKVFE_STEREO_CREATE 2
#define OKVFE_STEREO_OBS0 4
#define OKVFE_STEREO_OBS1 8
typedef struct okvfe_stereo_insert_device {
  uint8_t* action;       /* optional */
  int32_t* lm;           /* optional */
  int32_t* landmark_out; /* may be landmark_dev */
  int32_t* counts;       /* n_multiframes x 4 */
} okvfe_stereo_insert_device;
okvfe_status okvfe_stereo_insert_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const uint8_t* initialised_dev, const void* blocks_dev,
    int32_t block_stride_m, int32_t block_stride_c, int32_t n_multiframes, int32_t n_cams,
    const int32_t* pairs /* HOST, n_pairs x 2 */, int32_t n_pairs, const int32_t* cam_ids /* HOST, n_cams */,
    const okvfe_pose* T_WC /* HOST, n_multiframes x n_cams */, const okvfe_stereo_match* matches_dev,
    const int32_t* landmark_dev, const uint8_t* as_keyframe_dev /* or NULL */,
    const okvfe_stereo_insert_device* result, void* stream);

/* ---- loop closure: verifyRecognisedPlace up to the point where ceres takes over --------------
 * Frontend::verifyRecognisedPlace (Frontend.cpp:270-556) for one candidate old frame against a batch of multiframes,
 * from the old frame's landmark set to the verdict of :389.  The chain, all on one stream and without a host
 * synchronisation:
 *   okvfe_place_landmark_set                  host, once per old frame: the landmark set of :289-327
 *   okvfe_verify_place_blocks_device          the descriptor matching of :330-346 (k_min / dist_min per block and row)
 *   okvfe_place_claims_blocks_device          :347-351, :359, :380: the `matches` map, the counts and the gate
 *   okvfe_place_consensus_blocks_device       :372-397: the consensus over the caller's pose hypotheses and the verdict
 *   okvfe_place_refine_blocks_device          :399-527: the refinement of T_Sold_Snew as a defined algorithm, and H at
 *                                             the pose out
 *   okvfe_place_hessian_blocks_device         :529-551: the Hessian H at the caller's pose, and the residual and minimal
 *                                             Jacobian of every inlier, for a caller that runs a solver of its own
 * Landmarks of a set are rows 0 .. L - 1 in ascending landmark id: the rows and the order of the okvfe_map_device
 * (desc_begin, pool) that okvfe_verify_place_blocks_device is given.  Multiframe m owns gather blocks m n_cams + c, as
 * in okvfe_ransac3d2d_consensus_blocks_device, so the rows of k_min_dev / dist_min_dev of block b start at b L.
 * Several candidate old frames are several chains on one stream; the verdicts are downloaded once and the caller takes
 * the oldest verified candidate.
 *
 * What stays with the caller: the walk over the DBoW results and its non-maximum suppression with the estimator's
 * predicates (:771-819); the sampler and opengv's gp3p; opengv's adaptive stop, which only ever shortens the
 * hypothesis list; the solver of the ceres refinement, for a caller that wants ceres' own and not the defined algorithm
 * of okvfe_place_refine_blocks_device (:399-527: ceres' corrector, the 2 x 7 Jacobian through PoseManifold::minusJacobian
 * and DENSE_QR; its cost terms are what okvfe_place_hessian_blocks_device evaluates); the choice of the pose at which the Hessian H (:529-551) is taken -- the
 * reference takes it at the refined pose, the call takes it wherever poses_dev says; attemptLoopClosure and everything
 * after it.  PARITY UNPINNED: opengv's winner rule, as for okvfe_ransac3d2d_consensus_blocks_device. */

/* The landmark set of the old frame (Frontend.cpp:289-327).  Host helper, no context.  The old frame's keypoints of all
 * n_cams cameras, camera-major and ascending (n_kps[c] of camera c): landmark_ids (0 = none, :293; the use_cnn filter of
 * :305-317 is the caller's, which passes 0), landmarks (x 4, getLandmark's Vector4d), initialised (x 1 byte),
 * descriptors (x 48).  An observation is skipped iff its id is 0, or it is not initialised, or landmark.norm() < 1.0e-12
 * (:301; a NaN norm stays in).  norm() is the square root of the four-term sum of squares, taken in the `order` of
 * okvfe_set_fp64_reduction: 1 = (x0 x0 + x1 x1) + (x2 x2 + x3 x3), 0 = left to right.  A vectorised Eigen build may
 * take a third order (packets of two: (x0 x0 + x2 x2) + (x1 x1 + x3 x3)); the choice matters only to the last ulp of a
 * norm at 1e-12.  The first passing observation of a landmark supplies its Vector4d (:323), every passing observation
 * appends its descriptor (:320-322).
 * Outputs, landmarks in ascending id: ids_out (cap_landmarks), hp_out (cap_landmarks x 4), desc_begin_out
 * (cap_landmarks + 1), pool_out (cap_rows x 48, the rows of a landmark in (camera, keypoint) order).  *n_landmarks and
 * *n_rows receive the totals even when they exceed the capacities (then OKVFE_ERR_CAPACITY and nothing else is
 * written). */
okvfe_status okvfe_place_landmark_set(int32_t n_cams, const int32_t* n_kps /* n_cams */, const uint64_t* landmark_ids,
                                      const double* landmarks, const uint8_t* initialised, const uint8_t* descriptors,
                                      int32_t order, uint64_t* ids_out, double* hp_out, int32_t* desc_begin_out,
                                      int32_t cap_landmarks, uint8_t* pool_out, int32_t cap_rows, int32_t* n_landmarks,
                                      int32_t* n_rows);

typedef struct okvfe_place_set_device {
  int32_t n_landmarks; /* L */
  const double* hp;    /* device, L x 4: okvfe_place_landmark_set's hp_out */
} okvfe_place_set_device;
typedef struct okvfe_place_claims_device {
  int32_t* n_matches;         /* device, per multiframe: the reference's ctr */
  int32_t* n_points;          /* device, per multiframe: points.size() */
  int32_t* n_correspondences; /* device, per multiframe: adapter.getNumberCorrespondences() */
  uint8_t* gate;              /* device, per multiframe */
  int32_t* match_landmark;    /* device, blocks x K */
} okvfe_place_claims_device;
/* The claims of verifyRecognisedPlace (Frontend.cpp:347-351) and its two count gates (:359, :380) for n_multiframes
 * multiframes of n_cams gather blocks.  k_min_dev / dist_min_dev: what okvfe_verify_place_blocks_device wrote for these
 * blocks and this set's (desc_begin, pool), blocks x L.  A hit of row l in block b is dist_min < the context's
 * match_threshold (the value the matcher writes when nothing is below it); a hit whose k_min is outside [0, count) of
 * its block is ignored and not counted (the matcher cannot produce one).
 * Per multiframe: n_matches = the number of hits (ctr, :348); n_points = the number of rows with a hit in at least one
 * camera (:349); match_landmark[b K + k] = the largest hitting row l with k_min == k, or -1 (:350 is std::map
 * assignment with the landmarks in ascending order: the last writer keeps the keypoint, the loser stays in ctr and in
 * points); rows at or past the block's count are untouched.  n_correspondences = the number of claimed keypoints whose
 * landmark passes fabs(hp[3]) >= 1.0e-8 or is a NaN (LoopclosureNoncentralAbsoluteAdapter.cpp:126), written whatever
 * the gate says.  gate = 0 if n_matches < min_inliers || n_points < 8 (:359), else 1 if n_correspondences < 7 (:380: eight
 * above and seven here, as written), else 2: the multiframe goes on to RANSAC.
 * One work-group per multiframe, one camera at a time; the claims of a camera are one int per keypoint in LDS, resolved
 * with atomicMax (order-independent, hence deterministic).  The keypoints are not tiled: a context whose max_keypoints
 * exceeds 12288 is refused with OKVFE_ERR_UNSUPPORTED before anything is launched.  Nothing synchronises the host; no
 * workspace.  A NULL or negative argument: OKVFE_ERR_INVALID_ARGUMENT before any device work; n_multiframes == 0 is OK
 * and launches nothing. */
okvfe_status okvfe_place_claims_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                              int32_t n_multiframes, int32_t n_cams, const int32_t* k_min_dev,
                                              const uint32_t* dist_min_dev, int32_t min_inliers,
                                              const okvfe_place_claims_device* result, void* stream);
/* The consensus of verifyRecognisedPlace (Frontend.cpp:372-397): okvfe_ransac3d2d_consensus_blocks_device's kernel
 * under another policy.  cam_ids, T_SC, hypotheses_dev, hyp_valid_dev, n_hyp (the reference: 50, :383), threshold (16,
 * :382), the distance (FrameAbsolutePoseSacProblem.hpp:135-167, which accepts both adapters: :97-101), the winner rule
 * and the order of the sums are those of that call.  match_landmark_dev: blocks x K rows of the set, as the claims call
 * writes them.
 * Correspondences (LoopclosureNoncentralAbsoluteAdapter.cpp:69-154), camera-major with keypoints ascending: keypoint
 * k < count with l = match_landmark[k] in [0, L), unless fabs(hp[4 l + 3]) < 1.0e-8 (:126; a NaN stays in).  Point,
 * bearing with the (1, 0, 0) fall-back, normalize() and sigma exactly as in FrameNoncentralAbsoluteAdapter; there is no
 * test on the number of observations.
 * verdict_dev (u8 per multiframe): 0 if gate_dev is given and gate_dev[m] == 0 (:359); else 1 if the kernel's own count
 * of correspondences is below 7 (:380); else the hypotheses are scored, the winner picked, and the verdict is 2 if
 * n_inliers < min_inliers || double(n_inliers) / double(n_correspondences) < 0.7 (:389), else 3: verified.  A ratio of
 * exactly 0.7 passes here (runRansac3d2d asks for > 0.7: 14 of 20 is verified here and rejected there).
 * result: n_correspondences is the kernel's own count under every verdict; accepted = (verdict == 3).  For verdicts 0
 * and 1 nothing is scored: best_hypothesis -1, n_inliers 0, hyp_inliers -1.  The optional state, distance and
 * landmark_out mean what they mean in the 3d2d call (:393-397 are the states 2); landmark_out may be
 * match_landmark_dev itself and holds -1 where the multiframe is verified and the state is 1.
 * Nothing synchronises the host; no workspace; 112 bytes per camera go through the pinned parameter ring.  A NULL or
 * negative argument: OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_multiframes == 0 is OK and launches
 * nothing. */
okvfe_status okvfe_place_consensus_blocks_device(
    okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids /* HOST, n_cams */, const okvfe_pose* T_SC /* HOST, n_cams */,
    const int32_t* match_landmark_dev, const uint8_t* gate_dev /* or NULL */, const double* hypotheses_dev,
    const uint8_t* hyp_valid_dev /* or NULL */, int32_t n_hyp, double threshold, int32_t min_inliers,
    const okvfe_ransac_result_device* result, uint8_t* verdict_dev, void* stream);

/* ---- the pose hypotheses of the two consensus calls: sampler and P3P solver -------------------
 * What fills hypotheses_dev / hyp_valid_dev of okvfe_ransac3d2d_consensus_blocks_device and
 * okvfe_place_consensus_blocks_device without a host step in between.  A DEFINED ALGORITHM, PARITY UNPINNED: opengv (not
 * in the reference tree) samples with rand() and solves gp3p, so sample-for-sample parity is impossible by construction;
 * what is stated here is restated in tests/ransac_hyp_ref.py one IEEE operation per line, and host, device and
 * restatement agree byte for byte.  The caller's own solver remains an option: the consensus calls take any hypotheses.
 *
 * Correspondences: exactly those of the consensus call of the same policy (the same device function), camera-major
 * with keypoints ascending; n of them in multiframe m.
 * Sampler (counter-based: a multiframe's samples do not depend on its place in the batch).  With key = sample_keys_dev[m]
 * (or m where that pointer is NULL), hypothesis h and draw j = 0 .. 3:
 *   z = seed + (key 512 + h 8 + j + 1) 0x9E3779B97F4A7C15 (mod 2^64); z ^= z >> 30; z *= 0xBF58476D1CE4E5B9;
 *   z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31;  r(j, range) = ((z >> 32) range) >> 32.
 * i0 = r(0, n); its camera c owns the contiguous range [b_c, e_c) of the list, n_c = e_c - b_c.  n_c < 4: invalid.
 * Draws 1 .. 3: t = r(j, n_c - j), then, over the already chosen positions x of camera c in ascending order, t += 1
 * where x <= t (no rejection loop).  Samples 0 .. 2 go to the solver, sample 3 chooses among its solutions.
 * DEVIATION from gp3p: all four samples come from ONE camera and the solver is a central P3P lifted through T_SC[c]
 * (on a one-camera multiframe: the whole list; on a rig the consensus still scores every camera).
 * Solver: Grunert's P3P in the distance form, a^2 = |P2 - P3|^2, b^2 = |P1 - P3|^2, c^2 = |P1 - P2|^2, ca = f2.f3,
 * cb = f1.f3, cg = f1.f2, k = (a^2 - c^2) / b^2, k2 = (a^2 + c^2) / b^2; the quartic in v = s3 / s1 with
 *   A4 = (k - 1)^2 - 4 (c^2/b^2) ca^2,  A3 = 4 [k (1 - k) cb - (1 - k2) ca cg + 2 (c^2/b^2) ca^2 cb],
 *   A2 = 2 [k^2 - 1 + 2 k^2 cb^2 + 2 ((b^2 - c^2)/b^2) ca^2 - 4 k2 ca cb cg + 2 ((b^2 - a^2)/b^2) cg^2],
 *   A1 = 4 [-k (1 + k) cb + 2 (a^2/b^2) cg^2 cb - (1 - k2) ca cg],  A0 = (1 + k)^2 - 4 (a^2/b^2) cg^2;
 * A4 == 0 or a non-finite coefficient: no solution.  Real roots: Ferrari on the depressed quartic y^4 + p y^2 + q y + r
 * (v = y - A3 / (4 A4)); q == 0: the biquadratic, y = +-sqrt(w) for the two w = (-p +- sqrt(p p - 4 r)) / 2 that are
 * >= 0, in the order +sqrt(w+), -sqrt(w+), +sqrt(w-), -sqrt(w-); otherwise the positive root m of
 * 8 m^3 + 8 p m^2 + (2 p^2 - 8 r) m - q^2 by bisection on [0, hi], hi doubled from 1 until the resolvent is positive
 * there, at most 64 times (else: no root), bisected until the midpoint equals an end, at most 128 steps, m = the upper
 * end; s = sqrt(2 m), t0 = p / 2 + m, u0 = q / (2 s); y = (s +- sqrt(s s - 4 (t0 + u0))) / 2, then
 * y = (-s +- sqrt(s s - 4 (t0 - u0))) / 2, each pair iff its discriminant is >= 0, + before -.  Equal roots are listed as
 * often as they occur.  Each root takes exactly 3 Newton steps on the original quartic (a step whose derivative is
 * exactly 0 leaves v unchanged).  ROOT ORDER IS SOLUTION ORDER.  u = s2 / s1 = ((k - 1) v^2 - 2 k cb v + 1 + k) /
 * (2 (cg - v ca)), s1^2 = b^2 / (1 + v^2 - 2 v cb); a root counts (n_solutions) iff v > 0 && u > 0 && s1^2 > 0 (a NaN
 * fails).  Pose: Q_i = s_i f_i; R_CW from the two orthonormal triads e1 = (X2 - X1) / |..|, e3 = e1 x (X3 - X1)
 * normalised, e2 = e3 x e1 (no SVD); t_CW = Q1 - R_CW P1; inverted; T_WS = T_WC T_SC^-1.  Every sum of the solver runs
 * left to right, whatever okvfe_set_fp64_reduction says.
 * Choice: the distance of the consensus call (the same function, which does follow okvfe_set_fp64_reduction) of sample
 * 3 under every solution; the smallest wins, the first on ties, a NaN or infinite distance never.
 * Invalid (hyp_valid 0, the 12 doubles zero): n_c < 4, no solution, no finite distance, a non-finite output.
 *
 * okvfe_p3p_hypothesis: the solver and the choice for ONE sample on the host, no context (what a caller at B = 1, or
 * one with its own sampler, uses).  points / bearings: 4 x 3 doubles (world points, unit bearings in the camera frame;
 * rows 0 .. 2 are solved, row 3 chooses), sigma: of the fourth correspondence, T_SC: of the samples' camera,
 * order: OKVFE_SUM3_EIGEN_TREE or OKVFE_SUM3_LEFT_TO_RIGHT.  hypothesis: 12 doubles, row-major [R | t] = T_WS;
 * valid, n_solutions (optional): one each. */
okvfe_status okvfe_p3p_hypothesis(const double* points, const double* bearings, double sigma, const okvfe_pose* T_SC,
                                  int32_t order, double* hypothesis, uint8_t* valid, int32_t* n_solutions);
/* The device calls: layouts and argument rules of the consensus calls (table / set, blocks_dev, n_cams, cam_ids, T_SC,
 * landmark_dev / match_landmark_dev, gate_dev).  sample_keys_dev: n_multiframes uint64 or NULL; n_hyp in
 * 1 .. OKVFE_RANSAC_MAX_HYPOTHESES.  With gate_dev[m] == 0 every hypothesis of multiframe m is invalid and nothing is
 * solved (samples -1, n_solutions 0).  result->hypotheses (n_multiframes x n_hyp x 12 doubles) and result->hyp_valid
 * (n_multiframes x n_hyp bytes) ARE the consensus calls' hypotheses_dev / hyp_valid_dev; optional: n_correspondences
 * (int32 per multiframe), samples (n_multiframes x n_hyp x 4 int32: c K + k of the drawn keypoint, -1 where nothing
 * was drawn), n_solutions (int32 per hypothesis).  One work-group per multiframe; the camera-major list of a multiframe
 * is 4 bytes per keypoint slot in LDS: n_cams x K + n_cams + 1 ints above 60 KiB is OKVFE_ERR_UNSUPPORTED.  Nothing
 * synchronises the host; no workspace; 112 bytes per camera go through the pinned parameter ring.  A NULL or negative
 * argument or n_hyp outside its range: OKVFE_ERR_INVALID_ARGUMENT before anything is launched; n_multiframes == 0 is
 * OK and launches nothing. */
typedef struct okvfe_ransac_hypotheses_device {
  double* hypotheses;
  uint8_t* hyp_valid;
  int32_t* n_correspondences; /* optional */
  int32_t* samples;           /* optional */
  int32_t* n_solutions;       /* optional */
} okvfe_ransac_hypotheses_device;
okvfe_status okvfe_ransac3d2d_hypotheses_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* table, const void* blocks_dev, int32_t n_multiframes,
    int32_t n_cams, const int32_t* cam_ids /* HOST, n_cams */, const okvfe_pose* T_SC /* HOST, n_cams */,
    const int32_t* landmark_dev, const uint64_t* sample_keys_dev /* or NULL */, uint64_t seed, int32_t n_hyp,
    const okvfe_ransac_hypotheses_device* result, void* stream);
okvfe_status okvfe_place_hypotheses_blocks_device(
    okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids /* HOST, n_cams */, const okvfe_pose* T_SC /* HOST, n_cams */,
    const int32_t* match_landmark_dev, const uint8_t* gate_dev /* or NULL */, const uint64_t* sample_keys_dev /* or NULL */,
    uint64_t seed, int32_t n_hyp, const okvfe_ransac_hypotheses_device* result, void* stream);

/* ---- the hypotheses of runRansac2d2d: sampler, two-point rotation, five-point relative pose ------
 * What fills rot_hyp_dev / rot_valid_dev / rel_hyp_dev / rel_valid_dev of okvfe_ransac2d2d_consensus_blocks_device
 * without a host step in between.  A DEFINED ALGORITHM, PARITY UNPINNED: opengv (not in the reference tree) samples with
 * rand() and solves with twopt_rotationOnly and Stewenius' five-point, so sample-for-sample parity is impossible by
 * construction; what is stated here is restated in tests/ransac2d2d_hyp_ref.py one IEEE operation per line, and host,
 * device and restatement agree byte for byte.  The caller's own solvers remain an option: the consensus call takes any
 * hypotheses.
 *
 * Correspondences: exactly those of the consensus call, per (pair, camera): FrameRelativeAdapter's list in
 * older-keypoint order, built by the same device functions; n of them.  n < 10: the reference skips the camera
 * (:2300) and the consensus scores nothing: every hypothesis of both problems is invalid, nothing is drawn or solved.
 * Sampler: the draw of the absolute-pose hypotheses above, unchanged, r(j, range) of (seed, key, h, j), under the key
 *   key = (pair_key 128 + c 2 + problem) mod 2^64, pair_key = sample_keys_dev[p] (or p where that pointer is NULL),
 *   c the camera's index in the call (< 64), problem 0 = rotation only, 1 = relative pose,
 * so a pair's samples do not depend on its place in the batch.  The rotation-only problem takes draws j = 0, 1, the
 * relative-pose problem j = 0 .. 7: t = r(j, n - j), then, over the already chosen positions x in ascending order,
 * t += 1 where x <= t (no rejection loop).
 * Rotation only (opengv's twopt_rotationOnly restated from its published source): M = T1 T2^T with the orthonormal
 * triads e1 = f_0, e3 = f_0 x f_1 normalised, e2 = e3 x e1, T1 over the two b1, T2 over the two b2, so that b1 ~ M b2,
 * M[i][j] = (e1[i] e1'[j] + e2[i] e2'[j]) + e3[i] e3'[j].  Invalid: a cross product of squared norm 0, a non-finite M.
 * Relative pose (opengv's STEWENIUS sample size, 5 + 3: samples 0 .. 4 solve, samples 5 .. 7 disambiguate).
 * DEVIATION from Stewenius' Groebner-basis / eigenvalue form: Nister's formulation, the same ten cubic constraints solved
 * through a univariate polynomial; no eigen-solver and no SVD.  Every sum of the solver runs left to right, whatever
 * okvfe_set_fp64_reduction says.
 *   Null space: Q (5 x 9), row i = b1_i (x) b2_i (b1^T E b2 = 0, E row-major).  Gauss-Jordan with FULL pivoting: step s
 *     takes the largest |a| over rows s .. 4 and the columns not yet used (the first in row-major order on ties; 0 or
 *     non-finite: invalid), swaps its row into s, takes (entry of the column / pivot) times that row from every other
 *     row (a row equal to it becomes exactly zero: a pair listed twice fails the next pivot), then divides the row by it.
 *     The free columns f_0 < f_1 < f_2 < f_3 give X, Y, Z, W: 1 at f_k, -a[s][f_k] at the pivot column of row s.
 *     E = x X + y Y + z Z + W.
 *   Constraints: det E = e0 (e4 e8 - e5 e7) - e1 (e3 e8 - e5 e6) + e2 (e3 e7 - e4 e6), then the nine entries of
 *     L E, L = E E^T - 1/2 tr(E E^T) I, row-major: (L_i0 e_0j + L_i1 e_1j) + L_i2 e_2j, (E E^T)_ij = (e_i0 e_j0 +
 *     e_i1 e_j1) + e_i2 e_j2, tr = (d00 + d11) + d22, all coefficient-wise on polynomials.  Columns: x^3, y^3, x^2y, xy^2,
 *     x^2z, x^2, y^2z, y^2, xyz, xy | xz^2, xz, x, yz^2, yz, y, z^3, z^2, z, 1.  An entry of E is a 4-vector over
 *     (x, y, z, 1), a product of two entries a 10-vector over (x^2, xy, xz, x, y^2, yz, y, z^2, z, 1); a product starts
 *     from zeros and adds a_i b_j to its monomial in the order i outer, j inner.
 *   Elimination: Gauss-Jordan on the first ten columns with partial pivoting (the largest |a| of column c over rows
 *     c .. 9, the first on ties; 0 or non-finite: invalid), in the same three steps, over all twenty columns.
 *   The polynomial: rows (x^2z) - z (x^2), (y^2z) - z (y^2), (xyz) - z (xy) give B(z), 3 x 3, columns of degree 3, 3, 4;
 *     det B = B00 (B11 B22 - B12 B21) - B01 (B10 B22 - B12 B20) + B02 (B10 B21 - B11 B20), degree 10.
 *   Real roots: a_10 zero or non-finite: invalid.  bound = 1 + max |a_i / a_10|.  For d = 9 .. 0 the d-th derivative's
 *     roots are sought in the intervals that the (d+1)-th derivative's roots and -bound, +bound cut; an interval whose
 *     end values have strictly opposite signs is bisected (mid = (lo + hi) / 2; a midpoint whose value is > 0 exactly
 *     when the upper end's is becomes the upper end) until the midpoint equals an end, at most 128 steps; the root is
 *     the upper end.  Ascending, at most 10 (rel_n_roots).  A root of even multiplicity is NOT found, nor one whose
 *     interval has an end value of exactly 0.  No Newton polish.
 *   Per root: (x, y, 1) ~ the cross product of the pair of B(z) rows with the largest |third component|, pairs (0,1),
 *     (0,2), (1,2), the first on ties; E = ((x X + y Y) + z Z) + W.
 *   Decomposition (Horn's closed form, no SVD): T = 1/2 tr(E E^T) I - E E^T = b b^T; b = the row of T with the largest
 *     diagonal entry (the first on ties; not > 0: the root has no candidate) over the square root of that entry;
 *     R-/+ = (cof(E) -/+ [b]x E) / (b.b), row i of cof(E) = row i+1 x row i+2; candidates in the order (R-, +b^),
 *     (R-, -b^), (R+, +b^), (R+, -b^), b^ = b / |b|: [R | t] with |t| = 1, p_older = R p_current + t.
 *   Choice: over every candidate of every root, roots ascending then candidate order, the sum (d5 + d6) + d7 of the
 *     consensus call's relative-pose distance (the same function, which does follow okvfe_set_fp64_reduction; it
 *     triangulates, so cheirality needs no test of its own); the smallest wins, the first on ties, a NaN or infinite
 *     sum never.
 *   Invalid (valid byte 0, the 12 doubles zero): n < 10, a failed pivot, no real root, no finite sum, a non-finite output.
 *
 * okvfe_twopt_rotation_hypothesis / okvfe_fivept_hypothesis: ONE sample on the host, no context (what a caller at B = 1,
 * or one with its own sampler, uses).  b1 / b2: 2 x 3 resp. 8 x 3 unit bearings of the older / current frame; sigma1 /
 * sigma2: the sigmas of rows 5 .. 7; order: OKVFE_SUM3_EIGEN_TREE or OKVFE_SUM3_LEFT_TO_RIGHT; valid: one byte; n_roots: optional. */
okvfe_status okvfe_twopt_rotation_hypothesis(const double* b1, const double* b2, double* M, uint8_t* valid);
okvfe_status okvfe_fivept_hypothesis(const double* b1, const double* b2, const double* sigma1, const double* sigma2,
                                     int32_t order, double* hypothesis, uint8_t* valid, int32_t* n_roots);
/* The device call: layouts, argument rules, limits (K <= 4095) and errors of okvfe_ransac2d2d_consensus_blocks_device,
 * before anything is launched; n_cams <= 64; sample_keys_dev: n_pairs uint64 or NULL; n_hyp in
 * 1 .. OKVFE_RANSAC_MAX_HYPOTHESES.  One work-group per (pair, camera), 114 KiB of LDS (one per CU).  Nothing synchronises the host; no
 * workspace; 8 bytes per pair and 8 per camera go through the pinned parameter ring; n_pairs == 0 is OK and launches
 * nothing. */
typedef struct okvfe_ransac2d2d_hypotheses_device {
  double* rot_hyp;             /* n_pairs x n_cams x n_hyp x 9: IS the consensus call's rot_hyp_dev */
  uint8_t* rot_valid;          /* n_pairs x n_cams x n_hyp: IS rot_valid_dev */
  double* rel_hyp;             /* n_pairs x n_cams x n_hyp x 12: IS rel_hyp_dev */
  uint8_t* rel_valid;          /* IS rel_valid_dev */
  /* optional, NULL allowed */
  int32_t* n_correspondences;  /* n_pairs x n_cams */
  int32_t* rot_samples;        /* n_pairs x n_cams x n_hyp x 2: the drawn list positions as OLDER keypoint index, -1: not drawn */
  int32_t* rel_samples;        /* n_pairs x n_cams x n_hyp x 8: the same encoding */
  int32_t* rel_n_roots;        /* n_pairs x n_cams x n_hyp */
} okvfe_ransac2d2d_hypotheses_device;
okvfe_status okvfe_ransac2d2d_hypotheses_blocks_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_multiframes0, const void* blocks1_dev, int32_t n_multiframes1,
    int32_t n_pairs, const int32_t* mf0 /* HOST, n_pairs */, const int32_t* mf1 /* HOST, n_pairs */, int32_t n_cams,
    const int32_t* cam_ids /* HOST, n_cams */, const int32_t* landmark0_dev, const int32_t* landmark1_dev,
    const uint8_t* added_dev /* n_landmarks bytes or NULL */, int32_t n_landmarks,
    const uint64_t* sample_keys_dev /* n_pairs or NULL */, uint64_t seed, int32_t n_hyp,
    const okvfe_ransac2d2d_hypotheses_device* result, void* stream);

typedef struct okvfe_place_hessian_device {
  double* H;                /* device, n_multiframes x 36, row-major 6 x 6 */
  int32_t* n_terms;         /* device, per multiframe */
  int32_t* n_singular;      /* device, per multiframe */
  double* residual;         /* optional: device, blocks x K x 2 */
  double* jacobian_minimal; /* optional: device, blocks x K x 12, row-major 2 x 6 */
} okvfe_place_hessian_device;
/* The Hessian H of verifyRecognisedPlace (Frontend.cpp:529-551), the information of the pose-graph edge that
 * attemptLoopClosure adds, and its terms: per inlier of the consensus one ReprojectionError::EvaluateWithMinimalJacobians
 * with jacobians[0] only (okvis_ceres ReprojectionError.hpp:99-183).  The next link of the chain above, on the same
 * stream; set, blocks_dev, n_multiframes, n_cams, cam_ids and match_landmark_dev are those of
 * okvfe_place_consensus_blocks_device.
 * T_SC_params: HOST, n_cams x 7 doubles in PoseParameterBlock layout (t[3], qx qy qz qw), the extrinsics as
 * estimator.extrinsics() gives them (:421).  poses_dev: device, n_multiframes x 7 doubles in the same layout:
 * T_Sold_Snew as the caller's solver left it (:527), or any iterate of it.  state_dev: blocks x K, the consensus call's
 * optional `state`.  verdict_dev: u8 per multiframe, or NULL: every multiframe counts.
 * Terms, in the order of LoopclosureNoncentralAbsoluteAdapter (camera-major, keypoints ascending): keypoint k < count of
 * block (m, c) iff state == 2 and match_landmark[k] is in [0, L) and (verdict_dev == NULL or verdict_dev[m] == 3).  For
 * a multiframe that is not verified H is 36 zeros and both counts are 0: the reference has returned false by then.
 * Per term, with the 3- and 4-term sums in the order of okvfe_set_fp64_reduction and no FMA:
 *   q.normalize() and toRotationMatrix() of both poses.  PARITY UNPINNED: they are Eigen's, restated from the published
 *   source: the coefficients are divided by sqrt(z), z the four-term sum of their squares, iff z > 0 (a zero or NaN
 *   quaternion stays as it is); the matrix is Eigen's, from tx = 2 x, twx = tx w, ... (Geometry/Quaternion.h).
 *   T_CS and T_SW as full 4 x 4 matrices (rotation transposed, translation (-C^T) t), hp_S = T_SW hp_W, hp_C = T_CS hp_S.
 *   projectHomogeneous (PinholeCamera.hpp:506-526): the head is negated when hp_C[3] < 0 and the 2 x 3 Jacobian is that
 *   of the negated head, not negated back; column 3 of Jh is zero.  The projection status is ignored, as the reference
 *   ignores it: OutsideImage and Behind rows contribute, and so does a RADTAN8 point past the model's guard (rho > 9),
 *   whose projection and Jacobian are the model's formulas evaluated there (the reference reads indeterminate memory).
 *   squareRootInformation = sqrt(64.0 / (size size)) I with size = double(keypoint.size) (:464); error = measurement -
 *   projection; residual = squareRootInformation error.
 *   J0_minimal = ((squareRootInformation Jh) T_CS) J, J = [C_SW hp_W[3] | -C_SW crossMx(hp_W.head<3>() - t_WS hp_W[3])]
 *   over a zero row (ReprojectionError.hpp:155-163).
 * The matrix products are full: the zeros of T_CS, J, Jh and the square-root information are multiplied and added, so a
 * non-finite operand spreads as it does in Eigen.
 * DEFINED DEVIATION: in two cases the residual and the twelve entries of J0_minimal are NaN and the term is counted in
 * n_singular[m]; it still takes part in H, so the NaN is loud.  (1) fabs(head[2]) < 1.0e-12: project returns before it
 * writes imagePoint or the Jacobian (PinholeCamera.hpp:302-304) and the reference goes on with indeterminate memory.
 * (2) size is not a positive finite number.
 * H = the sum over the terms of J0_minimal^T J0_minimal (:550): entry (i, j) of a term is J(0,i) J(0,j) + J(1,i) J(1,j),
 * and the terms are added to H one after the other in adapter order, from zero.  That order is the contract: a fixed
 * lane per entry walks the Jacobians staged in LDS; there is no tree over the terms.  H is symmetric byte for byte.
 * result: H, n_terms and n_singular are required.  residual and jacobian_minimal are optional and written at term rows
 * only: every other row, and every row at or past a block's count, is untouched.  Not returned: the 2 x 7 Jacobian
 * through PoseManifold::minusJacobian, the Cauchy loss and ceres' corrector, which depend on the caller's solver.
 * One work-group per multiframe, one camera after another; the keypoints are tiled, so there is no limit on
 * max_keypoints.  Nothing synchronises the host; no workspace; 64 bytes per camera go through the pinned parameter
 * ring.  A camera slot without intrinsics: OKVFE_ERR_NOT_READY.  A NULL or negative argument:
 * OKVFE_ERR_INVALID_ARGUMENT before any device work; n_multiframes == 0 is OK and launches nothing. */
okvfe_status okvfe_place_hessian_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                               int32_t n_multiframes, int32_t n_cams,
                                               const int32_t* cam_ids /* HOST, n_cams */,
                                               const double* T_SC_params /* HOST, n_cams x 7 */, const double* poses_dev,
                                               const int32_t* match_landmark_dev, const uint8_t* state_dev,
                                               const uint8_t* verdict_dev /* or NULL */,
                                               const okvfe_place_hessian_device* result, void* stream);

typedef struct okvfe_place_refine_device {
  double* poses;         /* device, n_multiframes x 7: T_Sold_Snew out (t[3], qx qy qz qw) */
  int32_t* status;       /* device, per multiframe: 0 .. 4, see below */
  int32_t* n_iterations; /* optional: device, per multiframe */
  int32_t* n_accepted;   /* optional: device, per multiframe */
  int32_t* n_terms;      /* optional: device, per multiframe */
  double* cost;          /* optional: device, n_multiframes x 2: the cost at the start and at the pose out */
  double* start_poses;   /* optional: device, n_multiframes x 7 */
  double* H;             /* optional: device, n_multiframes x 36 */
  int32_t* n_singular;   /* optional: device, per multiframe; written only where H is given */
} okvfe_place_refine_device;
/* The refinement of T_Sold_Snew between the consensus and H (Frontend.cpp:399-527): the ceres problem of one
 * ReprojectionError per inlier with CauchyLoss(3) over one pose with PoseManifold, at most max_iterations iterations (the
 * reference: 10), as the DEFINED ALGORITHM that tests/place_refine_ref.py states one IEEE operation per line:
 * Levenberg-Marquardt with ceres' published trust-region rules and the defaults the reference leaves untouched (radius
 * 1e4, eta 1e-3, the Jacobi scaling 1 / (1 + sqrt(A_jj)), min/max diagonal 1e-6 / 1e32, gradient, parameter and function
 * tolerances 1e-10, 1e-8, 1e-6, minimum radius 1e-32).  The next link of the chain above, on the same stream; set,
 * blocks_dev, n_multiframes, n_cams, cam_ids, T_SC_params, match_landmark_dev, state_dev and verdict_dev are those of
 * okvfe_place_hessian_blocks_device, and the terms and their order are that call's.
 * The start: initial_poses_dev (device, n_multiframes x 7) where given; else Transformation(Matrix4d) of hypothesis
 * best_hypothesis_dev[m] of hypotheses_dev (device, n_multiframes x n_hyp x 12, row-major 3 x 4; best_hypothesis_dev is
 * the consensus call's best_hypothesis), the quaternion by Eigen's Quaterniond(Matrix3d), not normalised.  A winner
 * outside [0, n_hyp) starts at a NaN pose: the multiframe is still evaluated and ends with status 4 and its n_terms.
 * hypotheses_dev and best_hypothesis_dev may be NULL if and only if initial_poses_dev is given.
 * Per term of an evaluation: the residual r and J0_minimal of okvfe_place_hessian_blocks_device at the pose, then
 * s = r0 r0 + r1 r1, total = 1 + s / 9 (as a product with the double nearest 1 / 9), rho0 = 9 log(total),
 * rho1 = max(DBL_MIN, 1 / total), w = sqrt(rho1), and w r, w J enter A = sum (wJ)^T (wJ), g = sum (wJ)^T (w r) and the
 * cost 0.5 sum rho0, every entry added term after term in adapter order from zero by a fixed lane (no tree over the
 * terms).  log, and the sin and cos of PoseManifold::plus, are the fixed sequences of csrc/elementary_fixed.h (within
 * 2 ulp resp. 1 ulp of libm).  The 3-term sum of plus and the 4-term sums of normalized() follow
 * okvfe_set_fp64_reduction, as do the sums of the term; every other sum runs left to right.  No FMA.
 * DEFINED DEVIATIONS from ceres: (1) the 6 x 6 step is a Cholesky factorisation of the scaled normal equations in a
 * written-out order (ceres' default is DENSE_QR on the stacked system: the same minimiser, another rounding); (2) the
 * gradient test takes max |g_j| itself where ceres goes through plus(x, -g).  PARITY UNPINNED: ceres' loop and Eigen's
 * conversion, product and normalized() are restated from their published sources (neither is in the tree).
 * status: 0 = not verified (verdict_dev given and verdict_dev[m] != 3): only status, the counts (0) and cost (0, 0) are
 * written, the multiframe's rows of poses and start_poses are untouched and H is zeros; 1 = converged (gradient,
 * parameter or function tolerance); 2 = the iteration limit; 3 = no term: the pose out is the start; 4 = failed: a
 * non-finite cost, gradient or A at the start or at an accepted point, or a radius below 1e-32.  The pose out is the last
 * accepted point.  n_iterations counts every iteration begun, also one whose step was invalid (a failed pivot, a model
 * change that is not > 0, a half-angle beyond pi / 4) and used no evaluation.
 * H, n_singular: okvfe_place_hessian_blocks_device's H and n_singular at result->poses with the same verdict_dev, queued
 * behind the last step.
 * Launches: 1 (start) + 2 (evaluation, step) + 2 max_iterations (evaluation, step) + 1 where H is asked for; every launch
 * is either a near copy of the Hessian kernel (one work-group per multiframe; a work-group whose multiframe has ended
 * returns after one load) or per-lane arithmetic, a lane per multiframe, that also compiles for the host
 * (csrc/place_refine_dev.h).  After the last step every multiframe has ended: an evaluation is asked for only by an
 * iteration that was counted, so at most max_iterations candidates are evaluated, and the step behind the last of them
 * meets it >= max_iterations before it can ask for another.  0 <= max_iterations <= 64.
 * Nothing synchronises the host.  The per-multiframe records (under 1 KB each) live in a workspace per stream, so two
 * calls on one stream reuse it in order; 64 bytes per camera go once through the pinned parameter ring.  A camera slot
 * without intrinsics: OKVFE_ERR_NOT_READY.  A NULL or negative argument, or max_iterations outside [0, 64]:
 * OKVFE_ERR_INVALID_ARGUMENT before any device work; n_multiframes == 0 is OK and launches nothing. */
okvfe_status okvfe_place_refine_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                              int32_t n_multiframes, int32_t n_cams,
                                              const int32_t* cam_ids /* HOST, n_cams */,
                                              const double* T_SC_params /* HOST, n_cams x 7 */,
                                              const double* hypotheses_dev, int32_t n_hyp,
                                              const int32_t* best_hypothesis_dev,
                                              const double* initial_poses_dev /* or NULL */,
                                              const int32_t* match_landmark_dev, const uint8_t* state_dev,
                                              const uint8_t* verdict_dev /* or NULL */, int32_t max_iterations,
                                              const okvfe_place_refine_device* result, void* stream);

/* ---- place recognition: the DBoW2 query and database on device-resident batches ----------------
 * What decides which old frames verifyRecognisedPlace is run against.  The reference runs
 * dBow_->database.query(features, dBoWResult, -1) on every frame once it is initialised (Frontend.cpp:660-672,
 * :752-766), again per component for multi-session relocalisation (:677-685), and database.add(features) at keyframes
 * (:896-898).  Here the vocabulary and the database stay in device memory, and one chain on one stream takes a batch of
 * multiframes from their gather blocks to the few candidate entries per multiframe that the reference's walk over the
 * sorted results would consider -- without a host synchronisation:
 *   okvfe_vocabulary_check                  host, once per upload: the tree is a tree
 *   okvfe_bow_vectors_blocks_device         features -> words -> BowVector per multiframe (:660-672 and DBoW2's transform)
 *   okvfe_place_query_blocks_device         the L1 scores against every entry, :761-765, :780-799 and :802
 *   okvfe_bow_database_add_blocks_device    :896-898 for the keyframes of the batch
 *   okvfe_bow_database_check_device         the one call of the group that synchronises: did an add run out of room
 * The B = 1 host seams okvfe_fbrisk_transform / okvfe_bow_vector / okvfe_bow_query_l1 above compute the same numbers
 * from host arrays; the descent and the score are one piece of device code under both.
 * Multiframe m owns gather blocks m n_cams + c.  Entry ids are positions in the database; the caller keeps the poseIds
 * (:898).  All queries of one call see the database as it is at the call: the reference, which goes frame by frame,
 * lets frame t see the keyframe added at t - 1.  Batch granularity is the caller's choice; the entries of the last
 * few frames are excluded by the estimator's predicates (:808-819) anyway.
 * What stays with the caller: poseIds; estimator.isPlaceRecognitionFrame per entry (it arrives as suppressible_dev);
 * the attempts / attempts0 limits and the estimator predicates of :801-819, walked over at most a few dozen candidates
 * per multiframe after ONE download of the candidate rows; verifyRecognisedPlace itself is the group above.
 * PARITY UNPINNED: DBoW2 is not in the reference tree (an external dependency of it); transform, addWeight, normalize
 * and queryL1 are restated from DBoW2's published source, as the B = 1 calls and the oracle restate them.
 * okvfe_set_fp64_reduction does NOT apply to anything here: DBoW2's sums are plain loops, and their order -- repeated
 * addition of a word's weight, the L1 norm in ascending word order, the score over the common words in ascending word
 * order -- is part of the contract. */
typedef struct okvfe_vocabulary_device {
  int32_t n_nodes, n_words;
  int32_t weighting;               /* 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY, as in okvfe_bow_vector */
  int32_t normalise_l1;            /* as in okvfe_bow_vector */
  const uint8_t* node_descriptors; /* n_nodes x 48 (the root's row is unused) */
  const int32_t* child_begin;      /* n_nodes + 1 */
  const int32_t* child_index;      /* child_begin[n_nodes] */
  const int32_t* node_word;        /* n_nodes: word id of a leaf, < 0 for an inner node */
  const double* word_weight;       /* n_words */
} okvfe_vocabulary_device;
/* Host-only, no context: the struct filled with HOST pointers.  OKVFE_ERR_INVALID_ARGUMENT (okvfe_last_error(NULL) names
 * the first offence) unless n_nodes >= 1, n_words >= 1, weighting in 0..3, child_begin[0] == 0, child_begin monotone,
 * every child in (parent, n_nodes), every node but the root the child of exactly one node and reachable from the root,
 * node_word in [0, n_words) for every leaf and < 0 for every inner node.  Called once per upload (okvfe_device_alloc /
 * okvfe_copy_to_device); the device calls trust the vocabulary, as the table calls trust a checked landmark table. */
okvfe_status okvfe_vocabulary_check(const okvfe_vocabulary_device* vocabulary_host);

typedef struct okvfe_bow_vectors_device {
  int32_t* n_words;           /* device, per multiframe: the number of distinct words */
  int32_t* ids;               /* device, M x stride: ascending word ids */
  double* values;             /* device, M x stride */
  int32_t stride;
  int32_t n_vocabulary_words; /* n_words of the vocabulary the vectors come from, or 0 if unknown (the query then never
                                 uses its dense table); the vectors call does not read it */
} okvfe_bow_vectors_device;
/* BowVectors of n_multiframes multiframes of n_cams gather blocks.  The features of multiframe m are the descriptors of
 * camera 0's keypoints k < count, then camera 1's, and so on (:663-672).  Per feature the descent of
 * okvfe_fbrisk_transform; per multiframe the vector of okvfe_bow_vector: words with !(weight > 0) are skipped; TF_IDF /
 * TF add the weight once per occurrence by repeated addition (BowVector::addWeight), IDF / BINARY keep it once; words
 * ascending; with normalise_l1 the values are divided by their L1 norm, summed sequentially in ascending word order
 * (one lane per work-group: a dependent chain of at most a few thousand FP64 additions, accepted because the order is
 * the contract), unless the norm is not > 0; otherwise TF_IDF / TF divide by the number of distinct words.
 * vectors->stride must be at least min(n_cams max_keypoints, n_words), so nothing is ever truncated; rows past
 * n_words[m] are untouched.  word_ids_dev: NULL, or device blocks x max_keypoints: the word id of every feature (those
 * of skipped words too), untouched at or past a block's count.
 * One work-group per multiframe sorts the multiframe's word ids in LDS and run-length encodes them, for any n_words.
 * The node descriptors sit in LDS when n_nodes <= 1024 and they fit beside the sort keys (the shipped 9^3 vocabulary
 * does up to 4096 features per multiframe).  A context with n_cams max_keypoints > 8192 is refused with
 * OKVFE_ERR_UNSUPPORTED before anything is launched.  Nothing synchronises the host; no workspace.  A NULL or negative
 * argument: OKVFE_ERR_INVALID_ARGUMENT before any device work; n_multiframes == 0 is OK and launches nothing. */
okvfe_status okvfe_bow_vectors_blocks_device(okvfe_ctx* ctx, const okvfe_vocabulary_device* vocabulary,
                                             const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
                                             const okvfe_bow_vectors_device* vectors, int32_t* word_ids_dev,
                                             void* stream);

typedef struct okvfe_bow_database_device {
  int32_t* begin;      /* device, cap_entries + 1; begin[0] = 0 is the caller's (okvfe_device_fill) */
  int32_t* ids;        /* device, cap_words */
  double* values;      /* device, cap_words */
  int32_t cap_entries, cap_words;
  int32_t n_entries;   /* HOST: grows with every okvfe_bow_database_add_blocks_device */
  int32_t* overflow;   /* device, one int32, zeroed by the caller: entries stored empty for want of room */
} okvfe_bow_database_device;
/* begin / ids / values are the arrays okvfe_bow_query_l1 takes: entry e owns [begin[e], begin[e + 1]), ascending word
 * ids, so a database built on the host uploads as it is. */
typedef struct okvfe_place_candidates_device {
  int32_t* n_listed;     /* device, per multiframe: dBoWResult.size() */
  int32_t* n_candidates; /* device, per multiframe: the true count, even above cap */
  int32_t* entry;        /* device, M x cap */
  double* score;         /* device, M x cap */
  int32_t cap;
} okvfe_place_candidates_device;
/* database.query and the estimator-free part of the walk over its results, for n_multiframes query vectors (rows of
 * `vectors`) against the db->n_entries entries the database holds at the call.
 * Score of entry e for query m = okvfe_bow_query_l1's: over the common words in ascending word order
 * t = |q - d|; t = t - |q|; t = t - |d|; value = value + t; score = -value / 2; -1 and "not listed" when there is no
 * common word (an empty entry is never listed).  scores_dev: NULL, or device M x n_entries doubles receiving them all.
 * The listed entries of a query in ascending entry id are the reference's sorted dBoWResult (:761-765).  Listed position
 * f with score p is a candidate iff
 *   NOT (suppressible[id_f] AND any of the listed neighbours f-1, f-2, f+1, f+2 that exist has Score > p)   (:780-799)
 *   AND p > min_score                                                               (:802, strict; the reference: 0.4)
 * with the comparisons written exactly like that: equal scores do not suppress, a NaN neither suppresses nor passes.
 * suppressible_dev: device, n_entries bytes (estimator.isPlaceRecognitionFrame of the entry's frame), or NULL = all
 * ones, which is the component walk of :700-719.  result: n_listed, the true n_candidates, and the first `cap`
 * candidates in ascending entry id with their scores; rows past the count are untouched.
 * One work-group per multiframe, no workspace: the query vector is staged in LDS (vocabularies up to 4096 words as a
 * dense word -> position table, larger ones as the sorted vector, of which up to 4096 words are staged and longer
 * vectors read from memory); every work-group walks all entries.  Nothing synchronises the host.  A NULL or negative
 * argument, or cap < 0: OKVFE_ERR_INVALID_ARGUMENT before any device work; n_multiframes == 0 is OK. */
okvfe_status okvfe_place_query_blocks_device(okvfe_ctx* ctx, const okvfe_bow_database_device* database,
                                             const okvfe_bow_vectors_device* vectors, int32_t n_multiframes,
                                             double min_score, const uint8_t* suppressible_dev, double* scores_dev,
                                             const okvfe_place_candidates_device* result, void* stream);
/* database.add (:896-898) for n_add multiframes of the batch: entry n_entries + i becomes a copy of the vector of
 * multiframe add_index[i] (HOST array, strictly ascending, each in [0, n_multiframes): the keyframe decision is host
 * arithmetic; the indices travel through the pinned parameter ring).  begin is extended on the device, because the word
 * counts never visit the host; database->n_entries (host) grows by n_add.
 * n_entries + n_add > cap_entries: OKVFE_ERR_CAPACITY before anything is launched, nothing changed.  Not enough room in
 * ids / values is only known on the device: that entry and all later ones of the call are stored empty
 * (begin[e + 1] = begin[e]) and *overflow is incremented once per such entry.  An empty vector is a legal entry.  A
 * query queued after an add on the same stream sees the new entries.  Nothing synchronises the host. */
okvfe_status okvfe_bow_database_add_blocks_device(okvfe_ctx* ctx, okvfe_bow_database_device* database,
                                                  const okvfe_bow_vectors_device* vectors, int32_t n_multiframes,
                                                  const int32_t* add_index /* HOST, n_add */, int32_t n_add,
                                                  void* stream);
/* Waits for the stream and returns OKVFE_ERR_CAPACITY if *overflow != 0 (the message has the count), else OKVFE_OK. */
okvfe_status okvfe_bow_database_check_device(okvfe_ctx* ctx, const okvfe_bow_database_device* database, void* stream);

/* ---- keyframe decision: keypoint coverage masks and their IoU ---------------- */
/* Frontend::doWeNeedANewKeyframe (Frontend.cpp:1058-1167), the step between the map matchers and matchStereo whose
 * answer is *asKeyframe.  Per camera image of size w x h (the context's) the reference keeps two zeroed u8 masks of
 * rows = h / 10 by cols = w / 10 pixels, `detections` and `matches`, and for every keypoint paints
 * cv::circle(mask, keypoint.pt * 0.1, radius, 255, cv::FILLED), radius = int(double(min(rows, cols)) * kptrad), into
 * `detections` and, if the keypoint carries a landmark, into `matches`; it then counts the non-zero pixels of
 * matches & detections and of matches | detections (:1074-1101, :1123-1149).  The coverage calls return these counts
 * per image, okvfe_keyframe_decision turns the records of the current multiframe and of the other multiframes into
 * the verdict.  ViSlamBackend::overlapFraction / trackingQuality (ViSlamBackend.cpp:157-196, 2341-2427) work on the
 * same masks: see the next section.
 *
 * What stays with the caller, because it needs estimator state: the two early returns at :1060-1065 (fewer than
 * 4 frames in the estimator -> keyframe; front-end not initialised -> no keyframe), which come BEFORE anything here,
 * and the choice of the other multiframes (keyframes, loop-closure frames, keyframes in the IMU window: :1105-1115).
 *
 * PARITY UNPINNED: cv::circle and the point conversion are not in the reference tree (OpenCV is an external
 * dependency of it); they are restated from OpenCV's published source.  Centre: Point2f * double gives
 * float(double(x) * 0.1) per coordinate, cv::Point rounds it with cvRound (half to even); a centre may lie outside
 * the mask (cx == cols), the disc is clipped.  Disc: thickness FILLED, LINE_8, shift 0 is the integer midpoint
 * routine -- a fixed stencil of half-widths per row offset (r = 4: 4 3 3 2 0, 49 pixels).  Keypoints whose
 * coordinates are not finite paint nothing.  See DESIGN.md, "keyframe decision".
 *
 * Limits (OKVFE_ERR_UNSUPPORTED beyond them): radius <= 127 mask pixels, and the two bit masks of an image plus the
 * id table must fit 64 KB of LDS -- every frame size okvfe_create accepts does at any radius up to 127, and so would
 * 4096 x 4096. */
typedef struct okvfe_coverage {      /* one camera image; 24 bytes */
  int32_t n_keypoints, n_matched;    /* keypoints painted into detections / into matches */
  int32_t detections_area, matches_area, intersection_area, union_area;  /* countNonZero of the four masks */
} okvfe_coverage;
/* :1074-1101 / :1123-1149 for n_frames gather blocks in one launch, one work-group per block.  landmark_ids_dev:
 * device, n_frames x K (K = okvfe_device_outputs.max_keypoints), 0 = no landmark; rows past a block's count are not
 * read.  id_set_dev == NULL: a keypoint counts as matched iff its id != 0 (the current frame); otherwise iff
 * id != 0 and id is among the n_id_set values at id_set_dev (the other frames, :1138) -- in any order, duplicates and
 * zeros allowed (zeros are ignored), n_id_set == 0 = the empty set.  ONE set per call, on purpose: the set is the
 * current multiframe's, the same for every other frame it is compared with, and may simply be the current frame's
 * own landmark_ids_dev rows, so the whole decision needs no host round trip but the final few records.
 * kptrad: 0.09 in Frontend.cpp:104 (ViSlamBackend uses 0.09 * uniformityRadius / 36).  coverage_dev: device,
 * n_frames records; nothing past them is written.  Nothing synchronises the host. */
okvfe_status okvfe_keyframe_coverage_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                                   const uint64_t* landmark_ids_dev, const uint64_t* id_set_dev,
                                                   int32_t n_id_set, double kptrad, okvfe_coverage* coverage_dev,
                                                   void* stream);
/* host containers in, host record out (the B = 1 seam; like okvfe_match_to_map): the same kernel on the context's
 * own stream, n keypoints of any number, synchronous. */
okvfe_status okvfe_keyframe_coverage(okvfe_ctx* ctx, const okvfe_keypoint* keypoints, int32_t n,
                                     const uint64_t* landmark_ids, const uint64_t* id_set, int32_t n_id_set,
                                     double kptrad, okvfe_coverage* out);
/* pure host arithmetic, no context: :1103, :1116-1166 in the reference's expression order.  current: n_cameras
 * records; others: n_others x n_cameras (multiframe-major), NULL if n_others == 0.  overlap_threshold: 0.55f
 * (keyframeInsertionOverlapThreshold_, :145).  *overlap (may be NULL) receives std::min(overlapOthers, overlap) of
 * :1154.  0 / 0 is NaN and goes through std::max / std::min / the comparisons as in the reference: a multiframe
 * without a painted pixel does not raise overlapOthers, no other frames leave it 0, and a keyframe is then needed
 * (unless the current multiframe has fewer than 7 keypoints per camera, :1157).  Negative counts are rejected. */
okvfe_status okvfe_keyframe_decision(const okvfe_coverage* current, int32_t n_cameras, const okvfe_coverage* others,
                                     int32_t n_others, float overlap_threshold, int32_t* need_keyframe,
                                     double* overlap);

/* ---- overlapFraction, the order of the motion-stereo sweep, trackingQuality ---- */
/* ViSlamBackend::overlapFraction(frameA, frameB) (ViSlamBackend.cpp:2341-2427) on the same masks: per side f (0 = A,
 * 1 = B) and camera every keypoint is painted into `detections`, and into `matches` iff its landmark id is in
 * landmarks(A) n landmarks(B), the sets taken over ALL cameras of each multiframe (:2372-2384, :2402).  An id of this
 * side is in its own set by construction, so that is: id != 0 and some keypoint of any camera of the OTHER multiframe
 * carries it.  Callers: the order of the motion-stereo sweep (Frontend.cpp:1742-1767, once per keyframe and frame)
 * and the back-end's keyframe management (ViSlamBackend.cpp:2237, :2261, :2299).  kptrad there is
 * 0.09 * uniformityRadius / 36 (ViSlamBackend.hpp:209).  Mask size, radius, centre rounding and disc: as above
 * (PARITY UNPINNED for cv::circle, as above).
 *
 * What stays with the caller: which frames are in allFrames (:1742-1749: keyframes, and IMU-window frames that are
 * keyframes, i.e. estimator.isKeyframe), and for okvfe_tracking_quality the observed-elsewhere test of
 * ViSlamBackend.cpp:178-187, which walks the estimator's observations. */
typedef struct okvfe_overlap_counts {  /* one ordered pair (A, B); [0] = side A, [1] = side B; 32 bytes */
  int32_t n_keypoints[2];              /* each field summed over the cameras of its side */
  int32_t n_matched[2];                /* keypoints painted into matches; [0] == 0 iff [1] == 0 iff no common id */
  int32_t intersection_area[2];        /* sum of countNonZero(matches & detections), :2420 */
  int32_t union_area[2];               /* sum of countNonZero(matches | detections), :2421 */
} okvfe_overlap_counts;
/* The counts of n_pairs ordered pairs of multiframes in ONE launch (two work-groups per pair); nothing synchronises
 * the host.  Multiframes are addressed as in okvfe_stereo_insert_blocks_device: the block of (multiframe m, camera c)
 * is block m * block_stride_m + c * block_stride_c of blocks_dev, for m < n_multiframes and c < n_cams (<= 32); two
 * (m, c) on one block, or a negative stride, is OKVFE_ERR_INVALID_ARGUMENT.  landmark_ids_dev: device, K u64 per
 * block AT THAT BLOCK INDEX (K = okvfe_device_outputs.max_keypoints), 0 = none: the ids of
 * okvfe_keyframe_coverage_blocks_device.  Rows at or past a block's count are never read, neither for painting nor
 * as part of the other side's set.  pair_a / pair_b: HOST arrays of n_pairs multiframe indices (a == b is allowed;
 * an index outside [0, n_multiframes) is OKVFE_ERR_INVALID_ARGUMENT and the message names the pair); they travel
 * through the pinned parameter ring, 8 bytes per pair.  n_pairs == 0 is OKVFE_OK and launches nothing; n_pairs < 2^30.
 * counts_dev: device, n_pairs records.  coverage_dev (may be NULL): device, n_pairs x 2 x n_cams per-image records
 * [pair][side][camera], equal to what okvfe_keyframe_coverage_blocks_device reports for that image with the other
 * multiframe's counted ids as the set.  Nothing past n_pairs records is written.
 * Limits (OKVFE_ERR_UNSUPPORTED): those of the coverage call -- radius <= 127, masks + id table within its LDS
 * budget, of which this call uses 256 bytes for the keypoint counts of the two sides. */
okvfe_status okvfe_overlap_pairs_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t block_stride_m,
                                               int32_t block_stride_c, int32_t n_multiframes, int32_t n_cams,
                                               const uint64_t* landmark_ids_dev, const int32_t* pair_a,
                                               const int32_t* pair_b, int32_t n_pairs, double kptrad,
                                               okvfe_overlap_counts* counts_dev, okvfe_coverage* coverage_dev /* or NULL */,
                                               void* stream);
/* pure host arithmetic, no context: :2386-2389 and :2410-2426 for n_pairs records.  `matches` is empty iff
 * n_matched[0] == 0, and the result is then 0.0; otherwise o[f] = double(intersection_area[f]) / double(union_area[f])
 * and the result is std::min(o[0], o[1]), i.e. o[1] < o[0] ? o[1] : o[0].  0 / 0 is NaN and goes through exactly like
 * that (a NaN o[0] is returned, a NaN o[1] alone is not).  A record where exactly one n_matched is 0 (the device call
 * cannot produce one) or with a negative count is OKVFE_ERR_INVALID_ARGUMENT; nothing is written then. */
okvfe_status okvfe_overlap_fraction(const okvfe_overlap_counts* counts, int32_t n_pairs, double* overlap_out);
/* pure host arithmetic, no context: Frontend.cpp:1751-1767.  overlap[i] / frame_ids[i]: overlapFraction(previous
 * frame, frame i) and the frame's StateId value, n entries; the entry at index `previous` (-1 = none) gets 1.0 without
 * its overlap being looked at (:1753-1755).  order_out (n entries of room) receives the INDICES of the frames in
 * descending lexicographic (overlap, id) order -- the reverse of std::sort on the pairs -- cut at the first overlap
 * <= 1.0e-8 (:1765); *n_order their number.  Duplicate ids are OKVFE_ERR_INVALID_ARGUMENT (allFrames is a set).
 * DEFINED DEVIATION: a NaN overlap (other than at `previous`) is OKVFE_ERR_INVALID_ARGUMENT, because std::sort on
 * pairs with a NaN is undefined behaviour in the reference; *n_order then receives the index of the first such
 * entry.  On any other error *n_order is -1. */
okvfe_status okvfe_motion_frame_order(const double* overlap, const uint64_t* frame_ids, int32_t n, int32_t previous,
                                      int32_t* order_out, int32_t* n_order);
/* pure host arithmetic, no context: ViSlamBackend::trackingQuality (ViSlamBackend.cpp:157-196) from the n_cams records
 * that a coverage call WITHOUT an id set (id_set == NULL) returns for the frame, after the caller has zeroed the ids
 * whose landmark is not observed in another frame (:178-187).  rows = height / 10, cols = width / 10;
 * radius = double(min(rows, cols)) * kptrad stays a double here and pointArea = int(radius * radius * M_PI) (:191; 65
 * for 752 x 480 at 0.095, while the painted disc has 49 pixels); per image intersectionCount += max(0, matches_area -
 * pointArea) and unionCount += rows * cols - pointArea; the result is 0.0 if the n_matched sum to less than 8, else
 * double(intersectionCount) / double(unionCount).  Negative counts are rejected. */
okvfe_status okvfe_tracking_quality(const okvfe_coverage* coverage, int32_t n_cams, int32_t width, int32_t height,
                                    double kptrad, double* quality_out);

/* ---- IMU propagation: the pose guess of a frame, its Jacobian and covariance --------------------
 * ViFrontendInterface::propagation, i.e. ImuError::propagation (okvis_ceres/src/ImuError.cpp:557-779): what the
 * reference runs for every frame before anything else (ThreadedSlam.cpp:397-409), the pose matchToMap starts from and,
 * through T_WC = T_WS T_SC (:434-444), the extraction direction T_WC.inverse().C() * (0, 0, -1) of detectAndDescribe
 * (Frontend.cpp:246-251).  Transcribed line by line into one sequence of IEEE operations that the host and the device
 * compile alike (okvis2_amd/csrc/imu_dev.h, which lists every source line it restates); tests/imu_ref.py is the numpy
 * restatement both are held to byte for byte.
 *
 * Layout (host arrays for okvfe_imu_propagation, device arrays for okvfe_imu_propagation_blocks_device):
 *   samples       one record of 8 doubles per IMU sample.  The FIRST double's eight bytes hold the timestamp as two
 *                 uint32, sec in bytes 0-3 and nsec in bytes 4-7 (okvis::Time); doubles 1-3 the gyroscope, 4-6 the
 *                 accelerometer, 7 unused.
 *   sample_begin  n_multiframes + 1 int32 offsets into samples, in records: multiframe m owns
 *                 [sample_begin[m], sample_begin[m + 1]), its ImuMeasurementDeque in order.
 *   states        18 doubles per multiframe: t_start and t_end (each in a sample's timestamp format), the 7 doubles of
 *                 T_WS in PoseParameterBlock layout (t[3], qx qy qz qw; poses_dev of okvfe_place_hessian_blocks_device),
 *                 the 9 of speedAndBias.
 *   T_SC_params   HOST in both calls: n_cams x 7 doubles in the same pose layout.
 * Arithmetic: FP64 without FMA, Eigen expressions in source order, left to right.  3-term sums and the 4-term sums of
 * squaredNorm() follow okvfe_set_fp64_reduction (`order` in the host call); the quaternion product's sums run left to
 * right.  The 15-term sums of F_delta P_delta F_delta^T ((F_delta P_delta) first) and T P_delta T^T run in ascending k
 * from the first product and the switch does not apply to them; zeros are multiplied and added.  PARITY UNPINNED: Eigen's
 * own order for these expressions and products, and its normalized(), inverse() and toRotationMatrix(), are restated
 * from the published sources.  Time - Time and Duration::toSec() are okvis_time's, so a caller's dt comes out bit-equal.
 * DEFINED DEVIATIONS:
 *   - cos / sinc of theta_half and cos / sin of Phi (rightJacobian) are the fixed sequences of
 *     okvis2_amd/csrc/elementary_fixed.h: within 1 ulp of libm for |x| <= pi / 4, NaN beyond.  The NaN spreads into the
 *     outputs; n_out_of_range counts the intervals in which one of them was called outside its domain (a NaN argument
 *     included).  At 200 Hz that takes a rate above 157 rad/s.
 *   - The reference reads element it + 1 before it knows that it exists; here it is read only where it exists.
 *   - t_end <= t_start: zero increments and n_propagated = 0 (the epilogue still normalises the quaternion).
 *   - status bit 1: front().timeStamp > t_start (the reference's assertion); bit 2: an empty sample list.  Nothing but
 *     status and n_out_of_range (= 0) is written for such a multiframe.
 *   - back().timeStamp < t_end: n_propagated = -1 as in the reference; pose and speed_and_bias receive the inputs
 *     unchanged and the per-camera outputs are those of that pose; jacobian and covariance are not written.
 * Not covered: ImuError::initPose, redoPreintegration, Evaluate*. */
typedef struct okvfe_imu_params {
  double a_max, g_max;                                /* saturation thresholds (strict >) */
  double sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c; /* okvis::ImuParameters */
  double g;                                           /* gravity magnitude */
} okvfe_imu_params;
typedef struct okvfe_imu_result_device {
  double* pose;            /* n_multiframes x 7 */
  double* speed_and_bias;  /* n_multiframes x 9 */
  int32_t* n_propagated;   /* per multiframe: the reference's return value */
  int32_t* status;         /* per multiframe: 0, or the bits above */
  int32_t* n_out_of_range; /* per multiframe */
  double* jacobian;        /* optional: n_multiframes x 225, row-major 15 x 15 */
  double* covariance;      /* optional: n_multiframes x 225 */
  double* T_WC;            /* optional: n_multiframes x n_cams x 7 */
  float* gravity_C;        /* optional: n_multiframes x n_cams x 3, the extraction direction: the layout
                            * okvfe_detect_describe_batch_device takes as its HOST gravity_C, so one download feeds it */
} okvfe_imu_result_device;
/* Host loop, no context: the struct filled with HOST pointers; order: OKVFE_SUM3_*.  n_multiframes == 1 is the seam for
 * ViFrontendInterface::propagation.  Optional pointers that are NULL are not written. */
okvfe_status okvfe_imu_propagation(const okvfe_imu_params* params, const double* samples, const int32_t* sample_begin,
                                   const double* states, int32_t n_multiframes, int32_t n_cams,
                                   const double* T_SC_params /* n_cams x 7, or NULL when n_cams == 0 */, int32_t order,
                                   const okvfe_imu_result_device* result);
/* The same on device-resident batches, in one launch.  The form follows the outputs asked for: the mean only and the
 * mean with F run a lane per multiframe; with P a wave per multiframe keeps P_delta, F_delta P_delta and F_delta in LDS,
 * a fixed lane per group of entries.  params and T_SC_params (HOST) travel through the pinned parameter ring, 64 + 56
 * n_cams bytes; n_cams <= 64.  The caller keeps sample_begin within samples_dev: the call cannot check it.  Nothing
 * synchronises the host; no workspace.  A NULL required pointer or a negative count: OKVFE_ERR_INVALID_ARGUMENT before
 * any device work; n_multiframes == 0 is OK and launches nothing. */
okvfe_status okvfe_imu_propagation_blocks_device(okvfe_ctx* ctx, const okvfe_imu_params* params, const double* samples_dev,
                                                 const int32_t* sample_begin_dev, const double* states_dev,
                                                 int32_t n_multiframes, int32_t n_cams,
                                                 const double* T_SC_params /* HOST, n_cams x 7 */,
                                                 const okvfe_imu_result_device* result, void* stream);

/* ---- cross-camera gather collective (RCCL over xGMI) ---------------------- */
/* The one exchange step of the path (okvis_frontend/src/Frontend.cpp:1990-2026 needs the keypoints
 * of BOTH cameras of a pair; with one camera per GPU they live on different ranks): an all-gather of
 * the ranks' gather blocks, issued from C on the caller's stream.  The library loads RCCL at first
 * use (dlopen of librccl.so.1: the copy already mapped by the process -- e.g. torch's -- is the
 * one found); a process that never calls these needs no RCCL.
 *   okvfe_comm_unique_id   ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to every rank
 *                          (any side channel: MPI, a socket, torch.distributed.broadcast, a file);
 *   okvfe_comm_create      ncclCommInitRank on `device` (collective over all ranks).  world == 1 with
 *                          id == NULL makes a local communicator that never touches RCCL;
 *   okvfe_comm_wrap        adopts an ncclComm_t the caller already owns (not destroyed by
 *                          okvfe_comm_destroy);
 *   okvfe_gather_blocks    ncclAllGather(send, recv, bytes_per_rank, ncclUint8) on `stream`
 *                          (a hipStream_t; NULL = the HIP null stream): recv_dev holds world x
 *                          bytes_per_rank bytes, rank-major.  Asynchronous: ordered by the stream. */
typedef struct okvfe_comm okvfe_comm;
#define OKVFE_COMM_ID_BYTES 128
okvfe_status okvfe_comm_unique_id(uint8_t id[OKVFE_COMM_ID_BYTES]);
okvfe_status okvfe_comm_create(const uint8_t* id /* OKVFE_COMM_ID_BYTES or NULL */, int32_t world,
                               int32_t rank, int32_t device, okvfe_comm** out);
okvfe_status okvfe_comm_wrap(void* nccl_comm, int32_t world, int32_t rank, okvfe_comm** out);
void okvfe_comm_destroy(okvfe_comm* comm);
int32_t okvfe_comm_world(const okvfe_comm* comm);
int32_t okvfe_comm_rank(const okvfe_comm* comm);
const char* okvfe_comm_last_error(void);
okvfe_status okvfe_gather_blocks(okvfe_comm* comm, const void* send_dev, void* recv_dev,
                                 size_t bytes_per_rank, void* stream);

/* ---- device utilities for hosts without HIP headers ----------------------- */
/* The C++ mirror (okvis2_amd/host/) is dependency-free; these let it own streams and device
 * buffers (gather blocks, match rows).  Plain hipMalloc / hipStream / hipMemcpyAsync underneath. */
okvfe_status okvfe_device_alloc(int32_t device, size_t bytes, void** out_dev);
void okvfe_device_free(void* dev);
okvfe_status okvfe_stream_create(int32_t device, void** out_stream);
void okvfe_stream_destroy(void* stream);
okvfe_status okvfe_stream_synchronize(void* stream);
okvfe_status okvfe_copy_to_device(void* dst_dev, const void* src_host, size_t bytes, void* stream);
okvfe_status okvfe_copy_to_host(void* dst_host, const void* src_dev, size_t bytes, void* stream);
okvfe_status okvfe_device_fill(void* dst_dev, int32_t byte_value, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OKVFE_H_ */
