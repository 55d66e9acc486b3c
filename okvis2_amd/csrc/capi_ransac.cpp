// capi_ransac.cpp -- what Frontend::matchToMap does between its two matcher passes, behind the C ABI: the consensus
// step of runRansac3d2d (Frontend.cpp:2208-2261) and removeOutliers (:2152-2205), on device-resident batches.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {
// What the four consensus and hypotheses calls share behind their argument checks, all of it before anything is queued:
// the count guard (consensus: keypoint slots of a multiframe within an int32 with room; hypotheses: their list within
// LDS) and the rig, one record per camera with its pose in the sensor frame and its slot.  ring_launch is the rest.
okvfe_status rig_params(okvfe_ctx* ctx, const char* who, bool hypotheses, int n_cams, const int32_t* cam_ids,
                        const okvfe_pose* T_SC, std::vector<RansacCamParams>* cp) {
  if (hypotheses && !ransac_hypotheses_fits(n_cams, ctx->kp_cap))
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: the list of %d x %d keypoint slots does not fit in LDS", who, n_cams,
                ctx->kp_cap);
  if (!hypotheses && (int64_t)n_cams * ctx->kp_cap >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: too many keypoints per multiframe", who);
  cp->assign((size_t)n_cams, RansacCamParams{});
  return rig_slots(ctx, RigWho{who, "frame"}, n_cams, cam_ids, nullptr, [&](int c, const DeviceCamera& dc) {
    RansacCamParams& p = (*cp)[(size_t)c];
    std::memcpy(p.C, T_SC[c].C, sizeof(p.C));
    std::memcpy(p.r, T_SC[c].r, sizeof(p.r));
    p.fu = dc.fu;
    p.cam = cam_ids[c];
  });
}
}  // namespace

extern "C" {

okvfe_status okvfe_ransac3d2d_consensus_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* T, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids, const okvfe_pose* T_SC, const int32_t* landmark_dev, const double* hypotheses_dev,
    const uint8_t* hyp_valid_dev, int32_t n_hyp, double threshold, int32_t remove_outliers,
    const okvfe_ransac_result_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || T->n_landmarks < 0 || (T->n_landmarks > 0 && (!T->hp_W || !T->obs_begin)) || !blocks_dev ||
      n_multiframes < 0 || n_cams < 1 || n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC || !landmark_dev ||
      !hypotheses_dev || n_hyp < 1 || n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !(threshold >= 0.0) || !result ||
      !result->n_correspondences || !result->best_hypothesis || !result->n_inliers || !result->accepted)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_ransac3d2d_consensus_blocks_device: bad argument");
  std::vector<RansacCamParams> cp;
  const okvfe_status st = rig_params(ctx, "okvfe_ransac3d2d_consensus_blocks_device", false, n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const RansacCamParams* rig) {
    launch_ransac_consensus(T->hp_W, T->obs_begin, T->n_landmarks, block_layout(ctx->kp_cap),
                            static_cast<const uint8_t*>(blocks_dev), n_multiframes, n_cams, ctx->kp_cap, rig, landmark_dev,
                            hypotheses_dev, hyp_valid_dev, n_hyp, threshold, remove_outliers ? 1 : 0, *result, s);
  });
}

okvfe_status okvfe_remove_outliers_blocks_device(okvfe_ctx* ctx, const okvfe_landmark_table_device* T,
                                                 const void* blocks_dev, int32_t n_frames, const int32_t* cam_ids,
                                                 const okvfe_pose* T_WC, double max_error, const int32_t* landmark_dev,
                                                 int32_t* landmark_out_dev, int32_t* kept_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || T->n_landmarks < 0 || (T->n_landmarks > 0 && !T->hp_W) || !blocks_dev || n_frames < 0 || !cam_ids || !T_WC ||
      !(max_error >= 0.0) || !landmark_dev || !landmark_out_dev || !kept_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_remove_outliers_blocks_device: bad argument");
  bool rt8 = false;  // the 8-coefficient form of the projection only when a slot this call uses holds that model
  std::vector<MapFrameParams> fp((size_t)n_frames);
  okvfe_status st = rig_slots(ctx, RigWho{"okvfe_remove_outliers_blocks_device", "frame"}, n_frames, cam_ids, &rt8,
                              [&](int f, const DeviceCamera&) {
                                fp[(size_t)f].T1 = T_WC[f];
                                fp[(size_t)f].cam = cam_ids[f];
                              });
  if (st != OKVFE_OK || n_frames == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  // pose and camera slot: one record per frame through the pinned parameter ring (one asynchronous copy, no host sync)
  RingSlot frames(ctx, &ctx->pair_ring, s);
  if ((st = frames.upload(fp.data(), fp.size() * sizeof(MapFrameParams))) != OKVFE_OK) return st;
  HIP_TRY(ctx, hipMemsetAsync(kept_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_remove_outliers_frames(T->hp_W, T->n_landmarks, frames.as<MapFrameParams>(), n_frames, ctx->d_cams,
                                  ctx->w, ctx->h, L, static_cast<const uint8_t*>(blocks_dev), ctx->kp_cap, max_error,
                                  landmark_dev, landmark_out_dev, kept_dev, s, rt8);
  }
  return finish_call(ctx, &frames, s);
}

// The consensus of Frontend::verifyRecognisedPlace (Frontend.cpp:372-397): the kernel above under its kPlace policy, fed
// with the claims of okvfe_place_claims_blocks_device (capi_place.cpp).
okvfe_status okvfe_place_consensus_blocks_device(
    okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids, const okvfe_pose* T_SC, const int32_t* match_landmark_dev, const uint8_t* gate_dev,
    const double* hypotheses_dev, const uint8_t* hyp_valid_dev, int32_t n_hyp, double threshold, int32_t min_inliers,
    const okvfe_ransac_result_device* result, uint8_t* verdict_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!set || set->n_landmarks < 0 || (set->n_landmarks > 0 && !set->hp) || !blocks_dev || n_multiframes < 0 ||
      n_cams < 1 || n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC || !match_landmark_dev || !hypotheses_dev ||
      n_hyp < 1 || n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !(threshold >= 0.0) || min_inliers < 0 || !result ||
      !result->n_correspondences || !result->best_hypothesis || !result->n_inliers || !result->accepted || !verdict_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_consensus_blocks_device: bad argument");
  std::vector<RansacCamParams> cp;
  const okvfe_status st = rig_params(ctx, "okvfe_place_consensus_blocks_device", false, n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const RansacCamParams* rig) {
    launch_place_consensus(set->hp, set->n_landmarks, block_layout(ctx->kp_cap), static_cast<const uint8_t*>(blocks_dev),
                           n_multiframes, n_cams, ctx->kp_cap, rig, match_landmark_dev, gate_dev, hypotheses_dev,
                           hyp_valid_dev, n_hyp, threshold, min_inliers, *result, verdict_dev, s);
  });
}

// The solver and the choice of ransac_hyp_dev.h for one sample on the host (k_ransac_hyp.hip): the B = 1 seam of the two
// calls below.
okvfe_status okvfe_p3p_hypothesis(const double* points, const double* bearings, double sigma, const okvfe_pose* T_SC,
                                  int32_t order, double* hypothesis, uint8_t* valid, int32_t* n_solutions) {
  if (!points || !bearings || !T_SC || !hypothesis || !valid ||
      (order != OKVFE_SUM3_LEFT_TO_RIGHT && order != OKVFE_SUM3_EIGEN_TREE))
    return OKVFE_ERR_INVALID_ARGUMENT;
  int n_sol = 0;
  const bool ok = p3p_hypothesis_host(order == OKVFE_SUM3_EIGEN_TREE, points, bearings, sigma, T_SC->C, T_SC->r, hypothesis, &n_sol);
  *valid = ok ? 1 : 0;
  if (n_solutions) *n_solutions = n_sol;
  return OKVFE_OK;
}

// The hypotheses of okvfe_ransac3d2d_consensus_blocks_device: sampler and P3P on the device (k_ransac_hyp.hip).
okvfe_status okvfe_ransac3d2d_hypotheses_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* T, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids, const okvfe_pose* T_SC, const int32_t* landmark_dev, const uint64_t* sample_keys_dev,
    uint64_t seed, int32_t n_hyp, const okvfe_ransac_hypotheses_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || T->n_landmarks < 0 || (T->n_landmarks > 0 && (!T->hp_W || !T->obs_begin)) || !blocks_dev ||
      n_multiframes < 0 || n_cams < 1 || n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC || !landmark_dev ||
      n_hyp < 1 || n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !result || !result->hypotheses || !result->hyp_valid)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_ransac3d2d_hypotheses_blocks_device: bad argument");
  std::vector<RansacCamParams> cp;
  const okvfe_status st = rig_params(ctx, "okvfe_ransac3d2d_hypotheses_blocks_device", true, n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const RansacCamParams* rig) {
    launch_ransac_hypotheses(T->hp_W, T->obs_begin, T->n_landmarks, block_layout(ctx->kp_cap),
                             static_cast<const uint8_t*>(blocks_dev), n_multiframes, n_cams, ctx->kp_cap, rig, landmark_dev,
                             sample_keys_dev, seed, n_hyp, *result, s);
  });
}

// ... and of okvfe_place_consensus_blocks_device: the same kernel under its kPlace policy.
okvfe_status okvfe_place_hypotheses_blocks_device(
    okvfe_ctx* ctx, const okvfe_place_set_device* set, const void* blocks_dev, int32_t n_multiframes, int32_t n_cams,
    const int32_t* cam_ids, const okvfe_pose* T_SC, const int32_t* match_landmark_dev, const uint8_t* gate_dev,
    const uint64_t* sample_keys_dev, uint64_t seed, int32_t n_hyp, const okvfe_ransac_hypotheses_device* result,
    void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!set || set->n_landmarks < 0 || (set->n_landmarks > 0 && !set->hp) || !blocks_dev || n_multiframes < 0 ||
      n_cams < 1 || n_cams > (int)ctx->h_cams.size() || !cam_ids || !T_SC || !match_landmark_dev || n_hyp < 1 ||
      n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !result || !result->hypotheses || !result->hyp_valid)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_hypotheses_blocks_device: bad argument");
  std::vector<RansacCamParams> cp;
  const okvfe_status st = rig_params(ctx, "okvfe_place_hypotheses_blocks_device", true, n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK || n_multiframes == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  return ring_launch(ctx, s, cp, OKVFE_STAGE_MAP, [&](const RansacCamParams* rig) {
    launch_place_hypotheses(set->hp, set->n_landmarks, block_layout(ctx->kp_cap), static_cast<const uint8_t*>(blocks_dev),
                            n_multiframes, n_cams, ctx->kp_cap, rig, match_landmark_dev, gate_dev, sample_keys_dev, seed,
                            n_hyp, *result, s);
  });
}

// Test hook, deliberately not in include/okvfe.h: the number of correspondences the consensus kernel scores at a time,
// so that the tests straddle it whatever it is.
int32_t okvfe_test_ransac_chunk_records(void) { return ransac_chunk_records(); }
// ... and the records of its LDS ring, so that the tests run whole laps of it
int32_t okvfe_test_ransac_ring_records(void) { return ransac_ring_records(); }

}  // extern "C"
