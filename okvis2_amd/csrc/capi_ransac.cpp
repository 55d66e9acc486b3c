// capi_ransac.cpp -- what Frontend::matchToMap does between its two matcher passes, behind the C ABI: the consensus
// step of runRansac3d2d (Frontend.cpp:2208-2261) and removeOutliers (:2152-2205), on device-resident batches.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {
// the rig of a consensus call: one record per camera, its pose in the sensor frame and its slot
okvfe_status rig_params(okvfe_ctx* ctx, const char* who, int n_cams, const int32_t* cam_ids, const okvfe_pose* T_SC,
                        std::vector<RansacCamParams>* cp) {
  cp->assign((size_t)n_cams, RansacCamParams{});
  for (int c = 0; c < n_cams; ++c) {
    const DeviceCamera* dc = slot_camera(ctx, cam_ids[c]);
    if (!dc)
      return fail(ctx, OKVFE_ERR_NOT_READY, "%s: frame %d: camera slot %d has no intrinsics (okvfe_set_camera)", who, c,
                  cam_ids[c]);
    RansacCamParams& p = (*cp)[(size_t)c];
    std::memcpy(p.C, T_SC[c].C, sizeof(p.C));
    std::memcpy(p.r, T_SC[c].r, sizeof(p.r));
    p.fu = dc->fu;
    p.cam = cam_ids[c];
  }
  return OKVFE_OK;
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
  if ((int64_t)n_cams * ctx->kp_cap >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_ransac3d2d_consensus_blocks_device: too many keypoints per multiframe");
  std::vector<RansacCamParams> cp;
  okvfe_status st = rig_params(ctx, "okvfe_ransac3d2d_consensus_blocks_device", n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK) return st;
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  // the rig: one record per camera through the pinned parameter ring (one asynchronous copy, no host sync)
  RingSlot rig(ctx, &ctx->pair_ring, s);
  if ((st = rig.upload(cp.data(), cp.size() * sizeof(RansacCamParams))) != OKVFE_OK) return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_ransac_consensus(T->hp_W, T->obs_begin, T->n_landmarks, L, static_cast<const uint8_t*>(blocks_dev),
                            n_multiframes, n_cams, ctx->kp_cap, rig.as<RansacCamParams>(), landmark_dev,
                            hypotheses_dev, hyp_valid_dev, n_hyp, threshold, remove_outliers ? 1 : 0, *result, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = rig.release();
  ctx->last_stream = s;
  return rel;
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
  for (int f = 0; f < n_frames; ++f) {
    const DeviceCamera* dc = slot_camera(ctx, cam_ids[f]);
    if (!dc)
      return fail(ctx, OKVFE_ERR_NOT_READY,
                  "okvfe_remove_outliers_blocks_device: frame %d: camera slot %d has no intrinsics (okvfe_set_camera)", f,
                  cam_ids[f]);
    rt8 = rt8 || dc->distortion == OKVFE_DIST_RADTAN8;
    fp[(size_t)f] = MapFrameParams{};
    fp[(size_t)f].T1 = T_WC[f];
    fp[(size_t)f].cam = cam_ids[f];
  }
  if (n_frames == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  // pose and camera slot: one record per frame through the pinned parameter ring (one asynchronous copy, no host sync)
  RingSlot frames(ctx, &ctx->pair_ring, s);
  okvfe_status st = frames.upload(fp.data(), fp.size() * sizeof(MapFrameParams));
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, hipMemsetAsync(kept_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_remove_outliers_frames(T->hp_W, T->n_landmarks, frames.as<MapFrameParams>(), n_frames, ctx->d_cams,
                                  ctx->w, ctx->h, L, static_cast<const uint8_t*>(blocks_dev), ctx->kp_cap, max_error,
                                  landmark_dev, landmark_out_dev, kept_dev, s, rt8);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = frames.release();
  ctx->last_stream = s;
  return rel;
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
  if ((int64_t)n_cams * ctx->kp_cap >= (int64_t)1 << 30)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_place_consensus_blocks_device: too many keypoints per multiframe");
  std::vector<RansacCamParams> cp;
  okvfe_status st = rig_params(ctx, "okvfe_place_consensus_blocks_device", n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK) return st;
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  RingSlot rig(ctx, &ctx->pair_ring, s);
  if ((st = rig.upload(cp.data(), cp.size() * sizeof(RansacCamParams))) != OKVFE_OK) return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_place_consensus(set->hp, set->n_landmarks, L, static_cast<const uint8_t*>(blocks_dev), n_multiframes, n_cams,
                           ctx->kp_cap, rig.as<RansacCamParams>(), match_landmark_dev, gate_dev,
                           hypotheses_dev, hyp_valid_dev, n_hyp, threshold, min_inliers, *result, verdict_dev, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = rig.release();
  ctx->last_stream = s;
  return rel;
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
  if (!ransac_hypotheses_fits(n_cams, ctx->kp_cap))
    return fail(ctx, OKVFE_ERR_UNSUPPORTED,
                "okvfe_ransac3d2d_hypotheses_blocks_device: the list of %d x %d keypoint slots does not fit in LDS", n_cams,
                ctx->kp_cap);
  std::vector<RansacCamParams> cp;
  okvfe_status st = rig_params(ctx, "okvfe_ransac3d2d_hypotheses_blocks_device", n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK) return st;
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  RingSlot rig(ctx, &ctx->pair_ring, s);
  if ((st = rig.upload(cp.data(), cp.size() * sizeof(RansacCamParams))) != OKVFE_OK) return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_ransac_hypotheses(T->hp_W, T->obs_begin, T->n_landmarks, L, static_cast<const uint8_t*>(blocks_dev),
                             n_multiframes, n_cams, ctx->kp_cap, rig.as<RansacCamParams>(), landmark_dev, sample_keys_dev,
                             seed, n_hyp, *result, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = rig.release();
  ctx->last_stream = s;
  return rel;
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
  if (!ransac_hypotheses_fits(n_cams, ctx->kp_cap))
    return fail(ctx, OKVFE_ERR_UNSUPPORTED,
                "okvfe_place_hypotheses_blocks_device: the list of %d x %d keypoint slots does not fit in LDS", n_cams,
                ctx->kp_cap);
  std::vector<RansacCamParams> cp;
  okvfe_status st = rig_params(ctx, "okvfe_place_hypotheses_blocks_device", n_cams, cam_ids, T_SC, &cp);
  if (st != OKVFE_OK) return st;
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  RingSlot rig(ctx, &ctx->pair_ring, s);
  if ((st = rig.upload(cp.data(), cp.size() * sizeof(RansacCamParams))) != OKVFE_OK) return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_place_hypotheses(set->hp, set->n_landmarks, L, static_cast<const uint8_t*>(blocks_dev), n_multiframes, n_cams,
                            ctx->kp_cap, rig.as<RansacCamParams>(), match_landmark_dev, gate_dev, sample_keys_dev, seed,
                            n_hyp, *result, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = rig.release();
  ctx->last_stream = s;
  return rel;
}

// Test hook, deliberately not in include/okvfe.h: the number of correspondences the consensus kernel scores at a time,
// so that the tests straddle it whatever it is.
int32_t okvfe_test_ransac_chunk_records(void) { return ransac_chunk_records(); }
// ... and the records of its LDS ring, so that the tests run whole laps of it
int32_t okvfe_test_ransac_ring_records(void) { return ransac_ring_records(); }

}  // extern "C"
