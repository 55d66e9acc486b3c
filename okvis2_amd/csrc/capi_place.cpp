// capi_place.cpp -- Frontend::verifyRecognisedPlace behind the C ABI, around the descriptor matching that
// okvfe_verify_place_blocks_device does: the old frame's landmark set (Frontend.cpp:289-327, on the host) and the
// claims with their two count gates (:347-351, :359, :380) on device-resident batches.  The consensus that follows is
// okvfe_place_consensus_blocks_device (capi_ransac.cpp).
#include <algorithm>
#include <cmath>
#include <map>

#include "okvfe_ctx.h"

using namespace okvfe;

namespace {
// What the Hessian and the refinement share.  The rig: pose parameters and slot per camera, 64 bytes each; *rt8 asks for
// the 8-coefficient form of the projection only when a slot this call uses holds that model.
okvfe_status hessian_rig(okvfe_ctx* ctx, const char* who, int n_cams, const int32_t* cam_ids, const double* T_SC_params,
                         std::vector<HessianCamParams>* cp, bool* rt8) {
  return rig_slots(ctx, RigWho{who, "frame"}, n_cams, cam_ids, rt8, [&](int c, const DeviceCamera&) {
    std::copy_n(T_SC_params + 7 * (size_t)c, 7, (*cp)[(size_t)c].pose);
    (*cp)[(size_t)c].cam = cam_ids[c];
  });
}
// ... and the terms' arguments, all but where the results go
void hessian_args(const okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev, int n_cams,
                  const HessianCamParams* rig, const double* poses, const int32_t* match_landmark, const uint8_t* state,
                  const uint8_t* verdict, PlaceHessianArgs* A) {
  const BlockLayout L = block_layout(ctx->kp_cap);
  A->hp = set->hp; A->n_landmarks = set->n_landmarks; A->blocks = static_cast<const uint8_t*>(blocks_dev);
  A->o_count = (int)L.o_count; A->o_kps = (int)L.o_kps; A->block_bytes = L.total;
  A->kp_cap = ctx->kp_cap; A->n_cams = n_cams; A->w = ctx->w; A->h = ctx->h;
  A->cams = rig; A->dcams = ctx->d_cams; A->poses = poses;
  A->match_landmark = match_landmark; A->state = state; A->verdict = verdict;
}
}  // namespace

extern "C" {

okvfe_status okvfe_place_landmark_set(int32_t n_cams, const int32_t* n_kps, const uint64_t* landmark_ids,
                                      const double* landmarks, const uint8_t* initialised, const uint8_t* descriptors,
                                      int32_t order, uint64_t* ids_out, double* hp_out, int32_t* desc_begin_out,
                                      int32_t cap_landmarks, uint8_t* pool_out, int32_t cap_rows, int32_t* n_landmarks,
                                      int32_t* n_rows) {
  if (n_cams < 0 || (n_cams > 0 && !n_kps) || (order != 0 && order != 1) || cap_landmarks < 0 || cap_rows < 0 ||
      !desc_begin_out || !n_landmarks || !n_rows || (cap_landmarks > 0 && (!ids_out || !hp_out)) ||
      (cap_rows > 0 && !pool_out))
    return OKVFE_ERR_INVALID_ARGUMENT;
  int64_t total = 0;
  for (int c = 0; c < n_cams; ++c) {
    if (n_kps[c] < 0) return OKVFE_ERR_INVALID_ARGUMENT;
    total += n_kps[c];
  }
  if (total > INT32_MAX || (total > 0 && (!landmark_ids || !landmarks || !initialised || !descriptors)))
    return OKVFE_ERR_INVALID_ARGUMENT;
  // cameras ascending, keypoints ascending: per landmark the keypoints that pass, the first of them supplies hp (:319-324)
  std::map<uint64_t, std::vector<int32_t>> set;
  int64_t rows = 0;
  for (int64_t i = 0; i < total; ++i) {
    if (landmark_ids[i] == 0) continue;  // :293
    if (!initialised[i]) continue;       // :300
    const double* x = landmarks + 4 * i;
    const double q0 = x[0] * x[0], q1 = x[1] * x[1], q2 = x[2] * x[2], q3 = x[3] * x[3];
    const double norm = std::sqrt(order ? (q0 + q1) + (q2 + q3) : ((q0 + q1) + q2) + q3);
    if (norm < 1.0e-12) continue;        // :301 (a NaN stays in)
    set[landmark_ids[i]].push_back((int32_t)i);
    ++rows;
  }
  *n_landmarks = (int32_t)set.size();
  *n_rows = (int32_t)rows;
  if ((int64_t)set.size() > cap_landmarks || rows > cap_rows) return OKVFE_ERR_CAPACITY;
  int32_t l = 0, row = 0;
  for (const auto& lm : set) {  // ascending id (:330)
    ids_out[l] = lm.first;
    std::copy_n(landmarks + 4 * (int64_t)lm.second.front(), 4, hp_out + 4 * (int64_t)l);
    desc_begin_out[l] = row;
    for (int32_t i : lm.second) {
      std::copy_n(descriptors + 48 * (int64_t)i, 48, pool_out + 48 * (int64_t)row);
      ++row;
    }
    ++l;
  }
  desc_begin_out[l] = row;
  return OKVFE_OK;
}

okvfe_status okvfe_place_claims_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                              int32_t n_multiframes, int32_t n_cams, const int32_t* k_min_dev,
                                              const uint32_t* dist_min_dev, int32_t min_inliers,
                                              const okvfe_place_claims_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!set || set->n_landmarks < 0 || (set->n_landmarks > 0 && (!set->hp || !k_min_dev || !dist_min_dev)) || !blocks_dev ||
      n_multiframes < 0 || n_cams < 1 || min_inliers < 0 || !result || !result->n_matches || !result->n_points ||
      !result->n_correspondences || !result->gate || !result->match_landmark)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_claims_blocks_device: bad argument");
  if (ctx->kp_cap > kPlaceClaimsMaxKeypoints)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "okvfe_place_claims_blocks_device: claims need max_keypoints <= %d (this context: %d)",
                kPlaceClaimsMaxKeypoints, ctx->kp_cap);
  if ((int64_t)n_multiframes * n_cams >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_claims_blocks_device: too many blocks");
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_place_claims(set->hp, set->n_landmarks, L, static_cast<const uint8_t*>(blocks_dev), n_multiframes, n_cams,
                        ctx->kp_cap, k_min_dev, dist_min_dev, (uint32_t)ctx->cfg.match_threshold, min_inliers, *result, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

// The Hessian H of Frontend::verifyRecognisedPlace (Frontend.cpp:529-551) behind the consensus of
// okvfe_place_consensus_blocks_device, and the residual and minimal Jacobian of every term (k_place_hessian.hip).
okvfe_status okvfe_place_hessian_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                               int32_t n_multiframes, int32_t n_cams, const int32_t* cam_ids,
                                               const double* T_SC_params, const double* poses_dev,
                                               const int32_t* match_landmark_dev, const uint8_t* state_dev,
                                               const uint8_t* verdict_dev, const okvfe_place_hessian_device* result,
                                               void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!set || set->n_landmarks < 0 || (set->n_landmarks > 0 && !set->hp) || !blocks_dev || n_multiframes < 0 || n_cams < 1 ||
      n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC_params || !poses_dev || !match_landmark_dev || !state_dev ||
      !result || !result->H || !result->n_terms || !result->n_singular)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_hessian_blocks_device: bad argument");
  if ((int64_t)n_cams * ctx->kp_cap >= (int64_t)1 << 30 || (int64_t)n_multiframes * n_cams >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_hessian_blocks_device: too many keypoints or blocks");
  bool rt8 = false;
  std::vector<HessianCamParams> cp((size_t)n_cams);
  const okvfe_status st = hessian_rig(ctx, "okvfe_place_hessian_blocks_device", n_cams, cam_ids, T_SC_params, &cp, &rt8);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const HessianCamParams* rig) {
    PlaceHessianArgs A;
    hessian_args(ctx, set, blocks_dev, n_cams, rig, poses_dev, match_landmark_dev, state_dev, verdict_dev, &A);
    A.H = result->H; A.n_terms = result->n_terms; A.n_singular = result->n_singular;
    A.residual = result->residual; A.jacobian = result->jacobian_minimal;
    launch_place_hessian(A, n_multiframes, rt8, s);
  });
}

// The refinement of T_Sold_Snew between the consensus and H (Frontend.cpp:399-527) as the defined algorithm of
// tests/place_refine_ref.py: 3 + 2 max_iterations short launches (k_place_refine.hip) and, where H is asked for, the
// Hessian kernel at the pose out.  Nothing here waits for the device.
okvfe_status okvfe_place_refine_blocks_device(okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev,
                                              int32_t n_multiframes, int32_t n_cams, const int32_t* cam_ids,
                                              const double* T_SC_params, const double* hypotheses_dev, int32_t n_hyp,
                                              const int32_t* best_hypothesis_dev, const double* initial_poses_dev,
                                              const int32_t* match_landmark_dev, const uint8_t* state_dev,
                                              const uint8_t* verdict_dev, int32_t max_iterations,
                                              const okvfe_place_refine_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!set || set->n_landmarks < 0 || (set->n_landmarks > 0 && !set->hp) || !blocks_dev || n_multiframes < 0 || n_cams < 1 ||
      n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC_params || !match_landmark_dev || !state_dev || !result ||
      !result->poses || !result->status || max_iterations < 0 || max_iterations > kRefineMaxIterations ||
      (!initial_poses_dev && (!hypotheses_dev || !best_hypothesis_dev || n_hyp < 0)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_refine_blocks_device: bad argument");
  if ((int64_t)n_cams * ctx->kp_cap >= (int64_t)1 << 30 || (int64_t)n_multiframes * n_cams >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_refine_blocks_device: too many keypoints or blocks");
  bool rt8 = false;
  std::vector<HessianCamParams> cp((size_t)n_cams);
  okvfe_status st = hessian_rig(ctx, "okvfe_place_refine_blocks_device", n_cams, cam_ids, T_SC_params, &cp, &rt8);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  // the stream's workspace: a record and an evaluation per multiframe, and the two counts of the Hessian call where the
  // caller does not ask for them
  const size_t n = (size_t)n_multiframes;
  const size_t o_evals = n * sizeof(PlaceRefineRecord), o_counts = o_evals + n * sizeof(PlaceRefineEval);
  uint8_t* ws = nullptr;
  if ((st = stream_workspace(ctx, &ctx->place_refine_ws, s, o_counts + 2 * n * sizeof(int32_t), &ws)) != OKVFE_OK) return st;
  PlaceRefineArgs R{};
  R.records = reinterpret_cast<PlaceRefineRecord*>(ws);
  R.evals = reinterpret_cast<PlaceRefineEval*>(ws + o_evals);
  R.n_multiframes = n_multiframes; R.n_hyp = n_hyp; R.max_iterations = max_iterations;
  R.hypotheses = hypotheses_dev; R.best = best_hypothesis_dev; R.initial = initial_poses_dev;
  R.poses = result->poses; R.start_poses = result->start_poses; R.cost = result->cost;
  R.status = result->status; R.n_iterations = result->n_iterations; R.n_accepted = result->n_accepted;
  R.n_terms = result->n_terms;
  PlaceHessianArgs& A = R.term;
  A.H = result->H;
  A.n_terms = reinterpret_cast<int32_t*>(ws + o_counts);
  A.n_singular = result->n_singular ? result->n_singular : A.n_terms + n;
  A.residual = nullptr; A.jacobian = nullptr;
  // the rig through the ring once for every launch of the call, released behind the last of them
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const HessianCamParams* rig) {
    hessian_args(ctx, set, blocks_dev, n_cams, rig, result->poses, match_landmark_dev, state_dev, verdict_dev, &A);
    launch_place_refine_start(R, s);
    launch_place_refine_eval(R, rt8, s);
    launch_place_refine_step(R, true, s);
    // at most max_iterations candidates are evaluated; the step behind the last one meets it >= max_iterations
    for (int i = 0; i < max_iterations; ++i) {
      launch_place_refine_eval(R, rt8, s);
      launch_place_refine_step(R, false, s);
    }
    if (result->H) launch_place_hessian(A, n_multiframes, rt8, s);
  });
}

// Test hook, deliberately not in include/okvfe.h: the number of terms the Hessian kernel evaluates at a time, so that the
// tests straddle it whatever it is.
int32_t okvfe_test_place_hessian_chunk_terms(void) { return place_hessian_chunk_terms(); }

}  // extern "C"
