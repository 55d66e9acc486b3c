// capi_map.cpp -- landmark-to-frame association behind the C ABI: matchToMap incl. landmark
// projection and descriptor-view pooling (Frontend.cpp:1219-1359, 1552-1589), the un-initialised
// variant (:1616-1719), verifyRecognisedPlace (:330-355), and the DBoW2 query path with the FBrisk
// trait (FBrisk.cpp:64-67; Frontend.cpp:756-766).
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {
// the second pass's record of one frame: the pose NOW and the two gate constants of its focal length
PairParams uninit_pair_params(const okvfe_pose& T_WC1, double focal_length) {
  PairParams pp{};
  std::memcpy(pp.C1, T_WC1.C, sizeof(pp.C1));
  std::memcpy(pp.r1, T_WC1.r, sizeof(pp.r1));
  const double sigma = 1.0 / focal_length;  // Frontend.cpp:1636
  pp.cos26 = std::cos(2.6 * sigma);
  pp.cos6 = std::cos(6.0 * sigma);
  return pp;
}
}  // namespace

extern "C" {

okvfe_status okvfe_match_to_map(okvfe_ctx* ctx, const uint8_t* desc, const okvfe_keypoint* kps, const uint8_t* use,
                                int32_t n_kps, const double* projections_l2, const int32_t* desc_begin,
                                int32_t n_landmarks, const uint8_t* pool, double reprojection_threshold,
                                int32_t* best_landmark, int32_t* best_dist) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_kps < 0 || n_landmarks < 0 || !desc_begin || !(reprojection_threshold >= 0.0) ||
      (n_kps > 0 && (!desc || !kps || !use || !best_landmark || !best_dist)) ||
      (n_landmarks > 0 && (!projections_l2 || !pool)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map: bad argument");
  for (int l = 0; l < n_landmarks; ++l)
    if (desc_begin[l + 1] < desc_begin[l] || desc_begin[l] < 0)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map: desc_begin not monotone at %d", l);
  if (n_kps == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  const int n_pool = desc_begin[n_landmarks];
  ScratchLayout lay;
  const size_t o_d = lay.take((size_t)n_kps * 48), o_k = lay.take((size_t)n_kps * sizeof(okvfe_keypoint)),
               o_u = lay.take(n_kps), o_p = lay.take((size_t)n_landmarks * 16),
               o_b = lay.take((size_t)(n_landmarks + 1) * 4), o_pool = lay.take((size_t)n_pool * 48),
               o_lm = lay.take((size_t)n_kps * 4), o_bd = lay.take((size_t)n_kps * 4);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_d, desc, (size_t)n_kps * 48));
  HIP_TRY(ctx, call.up(o_k, kps, (size_t)n_kps * sizeof(okvfe_keypoint)));
  HIP_TRY(ctx, call.up(o_u, use, n_kps));
  HIP_TRY(ctx, call.up(o_p, projections_l2, (size_t)n_landmarks * 16));
  HIP_TRY(ctx, call.up(o_b, desc_begin, (size_t)(n_landmarks + 1) * 4));
  HIP_TRY(ctx, call.up(o_pool, pool, (size_t)n_pool * 48));
  HIP_TRY(ctx, call.sync());
  launch_match_to_map(call.dev(o_d), call.dev<okvfe_keypoint>(o_k), call.dev(o_u), n_kps, call.dev<double>(o_p),
                      call.dev<int32_t>(o_b), n_landmarks, call.dev(o_pool), reprojection_threshold * reprojection_threshold,
                      ctx->cfg.match_threshold, call.dev<int32_t>(o_lm), call.dev<int32_t>(o_bd), s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(best_landmark, o_lm, (size_t)n_kps * 4));
  HIP_TRY(ctx, call.down(best_dist, o_bd, (size_t)n_kps * 4));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_landmarks(okvfe_ctx* ctx, int32_t cam, const okvfe_landmark_table* T,
                                          const okvfe_pose* T_WC1, double reprojection_threshold, int32_t exclusive,
                                          const uint8_t* desc, const okvfe_keypoint* kps, const uint8_t* use,
                                          int32_t n_kps, okvfe_landmark_pool* pool_out, int32_t* best_landmark,
                                          int32_t* best_dist) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || !T_WC1 || n_kps < 0 || !(reprojection_threshold >= 0.0) || T->n_landmarks < 0 || T->n_observations < 0 ||
      T->n_poses < 0 || !T->obs_begin || (n_kps > 0 && (!desc || !kps || !use || !best_landmark || !best_dist)) ||
      (T->n_landmarks > 0 && (!T->hp_W || !T->quality)) ||
      (T->n_observations > 0 && (!T->obs_pose || !T->obs_desc || !T->obs_backproj || !T->poses)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_landmarks: bad argument");
  if (!slot_camera(ctx, cam))
    return fail(ctx, OKVFE_ERR_NOT_READY, "okvfe_match_to_map_landmarks: camera slot %d has no intrinsics (okvfe_set_camera)", cam);
  const int nl = T->n_landmarks, no = T->n_observations;
  for (int l = 0; l < nl; ++l)
    if (T->obs_begin[l + 1] < T->obs_begin[l] || T->obs_begin[l] < 0 || T->obs_begin[l + 1] > no)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_landmarks: obs_begin not monotone at %d", l);
  for (int o = 0; o < no; ++o)
    if (T->obs_pose[o] < 0 || T->obs_pose[o] >= T->n_poses)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_landmarks: observation %d: pose index out of range", o);
  for (int k = 0; k < n_kps; ++k) {
    best_landmark[k] = -1;
    best_dist[k] = ctx->cfg.match_threshold;
  }
  if (nl == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  // inputs
  const size_t o_hp = lay.take((size_t)nl * 32), o_q = lay.take((size_t)nl * 8), o_ob = lay.take((size_t)(nl + 1) * 4),
               o_op = lay.take((size_t)no * 4), o_od = lay.take((size_t)no * 48), o_obp = lay.take((size_t)no * 24),
               o_poses = lay.take((size_t)T->n_poses * sizeof(okvfe_pose));
  const size_t o_d = lay.take((size_t)n_kps * 48), o_k = lay.take((size_t)n_kps * sizeof(okvfe_keypoint)),
               o_u = lay.take(n_kps);
  // pooling results
  const size_t o_st = lay.take((size_t)nl * 4), o_nd = lay.take((size_t)nl * 4), o_rows = lay.take((size_t)nl * 12),
               o_proj = lay.take((size_t)nl * 16), o_e = lay.take((size_t)nl * 48), o_r = lay.take((size_t)nl * 48);
  // packed 3-D set + matcher outputs
  const size_t o_idx = lay.take((size_t)nl * 4), o_p3 = lay.take((size_t)nl * 16), o_b3 = lay.take((size_t)(nl + 1) * 4),
               o_pool3 = lay.take((size_t)nl * 2 * 48), o_n3 = lay.take(8), o_lm = lay.take((size_t)n_kps * 4),
               o_bd = lay.take((size_t)n_kps * 4);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_hp, T->hp_W, (size_t)nl * 32));
  HIP_TRY(ctx, call.up(o_q, T->quality, (size_t)nl * 8));
  HIP_TRY(ctx, call.up(o_ob, T->obs_begin, (size_t)(nl + 1) * 4));
  HIP_TRY(ctx, call.up(o_op, T->obs_pose, (size_t)no * 4));
  HIP_TRY(ctx, call.up(o_od, T->obs_desc, (size_t)no * 48));
  HIP_TRY(ctx, call.up(o_obp, T->obs_backproj, (size_t)no * 24));
  HIP_TRY(ctx, call.up(o_poses, T->poses, (size_t)T->n_poses * sizeof(okvfe_pose)));
  HIP_TRY(ctx, call.up(o_d, desc, (size_t)n_kps * 48));
  HIP_TRY(ctx, call.up(o_k, kps, (size_t)n_kps * sizeof(okvfe_keypoint)));
  HIP_TRY(ctx, call.up(o_u, use, n_kps));
  HIP_TRY(ctx, call.sync());  // pageable sources
  const DeviceCamera& dc = ctx->h_cams[cam];
  const double focal = dc.fu + dc.fv;  // the SUM, as at Frontend.cpp:1213-1215
  auto I = [&](size_t o) { return call.dev<int32_t>(o); };
  auto D = [&](size_t o) { return call.dev<double>(o); };
  launch_prepare_landmarks(D(o_hp), D(o_q), I(o_ob), nl, I(o_op), D(o_obp), call.dev<const okvfe_pose>(o_poses), *T_WC1,
                           ctx->d_cams + cam, ctx->w, ctx->h, reprojection_threshold, exclusive ? 1 : 0,
                           std::cos(10.0 / focal), std::cos(0.6), I(o_st), I(o_nd), I(o_rows), D(o_proj), D(o_e), D(o_r), s,
                           dc.distortion == OKVFE_DIST_RADTAN8);
  launch_compact_landmarks(I(o_st), I(o_nd), I(o_rows), D(o_proj), call.dev(o_od), nl, 1, I(o_idx), D(o_p3), I(o_b3),
                           call.dev(o_pool3), I(o_n3), s);
  HIP_TRY(ctx, hipGetLastError());
  int32_t n3[2] = {0, 0};
  HIP_TRY(ctx, call.down(n3, o_n3, 8));
  HIP_TRY(ctx, call.sync());  // the matcher's grid depends on the number of 3-D landmarks only
  if (n_kps > 0 && n3[0] > 0) {
    launch_match_to_map(call.dev(o_d), call.dev<okvfe_keypoint>(o_k), call.dev(o_u), n_kps, D(o_p3), I(o_b3), n3[0],
                        call.dev(o_pool3), reprojection_threshold * reprojection_threshold, ctx->cfg.match_threshold,
                        I(o_lm), I(o_bd), s);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> idx(n3[0]);
    HIP_TRY(ctx, call.down(best_landmark, o_lm, (size_t)n_kps * 4));
    HIP_TRY(ctx, call.down(best_dist, o_bd, (size_t)n_kps * 4));
    HIP_TRY(ctx, call.down(idx.data(), o_idx, (size_t)n3[0] * 4));
    HIP_TRY(ctx, call.sync());
    for (int k = 0; k < n_kps; ++k)
      if (best_landmark[k] >= 0) best_landmark[k] = idx[best_landmark[k]];  // packed -> table index
  }
  if (pool_out) {
    if (pool_out->status) HIP_TRY(ctx, call.down(pool_out->status, o_st, (size_t)nl * 4));
    if (pool_out->n_desc) HIP_TRY(ctx, call.down(pool_out->n_desc, o_nd, (size_t)nl * 4));
    if (pool_out->obs_rows) HIP_TRY(ctx, call.down(pool_out->obs_rows, o_rows, (size_t)nl * 12));
    if (pool_out->projection) HIP_TRY(ctx, call.down(pool_out->projection, o_proj, (size_t)nl * 16));
    if (pool_out->e_W) HIP_TRY(ctx, call.down(pool_out->e_W, o_e, (size_t)nl * 48));
    if (pool_out->r_W) HIP_TRY(ctx, call.down(pool_out->r_W, o_r, (size_t)nl * 48));
    HIP_TRY(ctx, call.sync());
  }
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_uninitialised(okvfe_ctx* ctx, const uint8_t* desc, const double* backproj,
                                              const uint8_t* use, const int32_t* previous_landmark,
                                              int32_t n_kps, const int32_t* desc_begin, int32_t n_landmarks,
                                              const uint8_t* pool, const double* e0_W, const double* r0_W,
                                              const okvfe_pose* T_WC1, double focal_length,
                                              int32_t* best_landmark, int32_t* best_dist, double* hps_W,
                                              uint8_t* hp_set, int32_t* already_matched) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_kps < 0 || n_landmarks < 0 || !desc_begin || !T_WC1 || !(focal_length > 0.0) || !already_matched ||
      (n_kps > 0 && (!desc || !backproj || !use || !previous_landmark || !best_landmark || !best_dist || !hps_W || !hp_set)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_uninitialised: bad argument");
  for (int l = 0; l < n_landmarks; ++l)
    if (desc_begin[l + 1] < desc_begin[l] || desc_begin[l] < 0)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_uninitialised: desc_begin not monotone at %d", l);
  *already_matched = 0;
  if (n_kps == 0) return OKVFE_OK;
  const int n_pool = desc_begin[n_landmarks];
  if (n_pool > 0 && (!pool || !e0_W || !r0_W))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_uninitialised: null pool");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  const size_t o_pair = lay.take(sizeof(PairParams)), o_d = lay.take((size_t)n_kps * 48), o_bp = lay.take((size_t)n_kps * 24),
               o_u = lay.take(n_kps), o_prev = lay.take((size_t)n_kps * 4), o_b = lay.take((size_t)(n_landmarks + 1) * 4),
               o_pool = lay.take((size_t)n_pool * 48), o_e = lay.take((size_t)n_pool * 24),
               o_r = lay.take((size_t)n_pool * 24), o_lm = lay.take((size_t)n_kps * 4), o_bd = lay.take((size_t)n_kps * 4),
               o_hp = lay.take((size_t)n_kps * 32), o_hs = lay.take(n_kps), o_ctr = lay.take(4);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  const PairParams pp = uninit_pair_params(*T_WC1, focal_length);
  HIP_TRY(ctx, call.up(o_pair, &pp, sizeof(pp)));
  HIP_TRY(ctx, call.up(o_d, desc, (size_t)n_kps * 48));
  HIP_TRY(ctx, call.up(o_bp, backproj, (size_t)n_kps * 24));
  HIP_TRY(ctx, call.up(o_u, use, n_kps));
  HIP_TRY(ctx, call.up(o_prev, previous_landmark, (size_t)n_kps * 4));
  HIP_TRY(ctx, call.up(o_b, desc_begin, (size_t)(n_landmarks + 1) * 4));
  HIP_TRY(ctx, call.up(o_pool, pool, (size_t)n_pool * 48));
  HIP_TRY(ctx, call.up(o_e, e0_W, (size_t)n_pool * 24));
  HIP_TRY(ctx, call.up(o_r, r0_W, (size_t)n_pool * 24));
  HIP_TRY(ctx, hipMemsetAsync(call.dev(o_ctr), 0, 4, s));
  HIP_TRY(ctx, call.sync());
  launch_match_to_map_uninit(call.dev<PairParams>(o_pair), call.dev(o_d), call.dev<double>(o_bp), call.dev(o_u),
                             call.dev<int32_t>(o_prev), n_kps, call.dev<int32_t>(o_b), n_landmarks, call.dev(o_pool),
                             call.dev<double>(o_e), call.dev<double>(o_r), ctx->cfg.match_threshold,
                             call.dev<int32_t>(o_lm), call.dev<int32_t>(o_bd), call.dev<double>(o_hp), call.dev(o_hs),
                             call.dev<int32_t>(o_ctr), s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(best_landmark, o_lm, (size_t)n_kps * 4));
  HIP_TRY(ctx, call.down(best_dist, o_bd, (size_t)n_kps * 4));
  HIP_TRY(ctx, call.down(hps_W, o_hp, (size_t)n_kps * 32));
  HIP_TRY(ctx, call.down(hp_set, o_hs, n_kps));
  HIP_TRY(ctx, call.down(already_matched, o_ctr, 4));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

okvfe_status okvfe_verify_place_match(okvfe_ctx* ctx, const uint8_t* landmark_desc, const int32_t* desc_begin,
                                      int32_t n_landmarks, const uint8_t* frame_desc, int32_t n_kps,
                                      int32_t* k_min, uint32_t* dist_min) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_landmarks < 0 || n_kps < 0 || !desc_begin || (n_landmarks > 0 && (!k_min || !dist_min)) ||
      (n_kps > 0 && !frame_desc))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_verify_place_match: bad argument");
  for (int l = 0; l < n_landmarks; ++l)
    if (desc_begin[l + 1] < desc_begin[l] || desc_begin[l] < 0)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_verify_place_match: desc_begin not monotone at %d", l);
  if (n_landmarks == 0) return OKVFE_OK;
  const int n_pool = desc_begin[n_landmarks];
  if (n_pool > 0 && !landmark_desc) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_verify_place_match: null pool");
  const uint32_t thr = (uint32_t)ctx->cfg.match_threshold;
  if (n_kps == 0 || n_pool == 0) {  // Frontend.cpp:333-335: a camera without keypoints is skipped
    for (int l = 0; l < n_landmarks; ++l) { k_min[l] = 0; dist_min[l] = thr; }
    return OKVFE_OK;
  }
  if ((int64_t)3 * n_kps >= (int64_t)1 << 31) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "too many keypoints");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  const size_t o_pool = lay.take((size_t)n_pool * 48), o_b = lay.take((size_t)(n_landmarks + 1) * 4),
               o_f = lay.take((size_t)n_kps * 48), o_k = lay.take((size_t)n_landmarks * 4),
               o_d = lay.take((size_t)n_landmarks * 4);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_pool, landmark_desc, (size_t)n_pool * 48));
  HIP_TRY(ctx, call.up(o_b, desc_begin, (size_t)(n_landmarks + 1) * 4));
  HIP_TRY(ctx, call.up(o_f, frame_desc, (size_t)n_kps * 48));
  HIP_TRY(ctx, call.sync());
  launch_verify_place(call.dev(o_pool), call.dev<int32_t>(o_b), n_landmarks, call.dev(o_f), n_kps, thr,
                      call.dev<int32_t>(o_k), call.dev<uint32_t>(o_d), s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(k_min, o_k, (size_t)n_landmarks * 4));
  HIP_TRY(ctx, call.down(dist_min, o_d, (size_t)n_landmarks * 4));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

okvfe_status okvfe_fbrisk_transform(okvfe_ctx* ctx, const uint8_t* descriptors, int32_t n,
                                    const uint8_t* node_descriptors, int32_t n_nodes, const int32_t* child_begin,
                                    const int32_t* child_index, const int32_t* node_word, int32_t* word_ids,
                                    int32_t* leaf_nodes) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n < 0 || n_nodes < 1 || !node_descriptors || !child_begin || !node_word || (n > 0 && (!descriptors || !word_ids)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_fbrisk_transform: bad argument");
  // the tree must be a tree: children lists monotone, indices in range and pointing downwards
  if (child_begin[0] != 0) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_fbrisk_transform: child_begin[0] != 0");
  for (int i = 0; i < n_nodes; ++i)
    if (child_begin[i + 1] < child_begin[i])
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_fbrisk_transform: child_begin not monotone at %d", i);
  const int n_child = child_begin[n_nodes];
  if (n_child > 0 && !child_index) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_fbrisk_transform: null children");
  {
    std::vector<int> depth(n_nodes, -1);
    depth[0] = 0;
    for (int i = 0; i < n_nodes; ++i)  // nodes are numbered so that a parent precedes its children
      for (int c = child_begin[i]; c < child_begin[i + 1]; ++c) {
        const int id = child_index[c];
        if (id <= i || id >= n_nodes || depth[i] < 0)
          return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_fbrisk_transform: node %d has child %d (not a tree in id order)", i, id);
        depth[id] = depth[i] + 1;
      }
  }
  if (n == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  const size_t o_d = lay.take((size_t)n * 48), o_n = lay.take((size_t)n_nodes * 48), o_cb = lay.take((size_t)(n_nodes + 1) * 4),
               o_ci = lay.take((size_t)n_child * 4), o_w = lay.take((size_t)n_nodes * 4), o_wo = lay.take((size_t)n * 4),
               o_no = lay.take((size_t)n * 4);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_d, descriptors, (size_t)n * 48));
  HIP_TRY(ctx, call.up(o_n, node_descriptors, (size_t)n_nodes * 48));
  HIP_TRY(ctx, call.up(o_cb, child_begin, (size_t)(n_nodes + 1) * 4));
  HIP_TRY(ctx, call.up(o_ci, child_index, (size_t)n_child * 4));
  HIP_TRY(ctx, call.up(o_w, node_word, (size_t)n_nodes * 4));
  HIP_TRY(ctx, call.sync());
  launch_voc_transform(call.dev(o_d), n, call.dev(o_n), n_nodes, call.dev<int32_t>(o_cb), call.dev<int32_t>(o_ci),
                       call.dev<int32_t>(o_w), call.dev<int32_t>(o_wo), call.dev<int32_t>(o_no), s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(word_ids, o_wo, (size_t)n * 4));
  if (leaf_nodes) HIP_TRY(ctx, call.down(leaf_nodes, o_no, (size_t)n * 4));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

okvfe_status okvfe_bow_vector(const int32_t* word_ids, int32_t n_features, const double* word_weight,
                              int32_t n_words, int32_t weighting, int32_t normalise_l1, int32_t* ids_out,
                              double* values_out, int32_t cap, int32_t* n_out) {
  if (n_features < 0 || n_words < 1 || !word_weight || !n_out || weighting < 0 || weighting > 3 ||
      (n_features > 0 && !word_ids) || cap < 0 || (cap > 0 && (!ids_out || !values_out)))
    return OKVFE_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < n_features; ++i)
    if (word_ids[i] < 0 || word_ids[i] >= n_words) return OKVFE_ERR_INVALID_ARGUMENT;
  // value per word in feature order (the sums are sequential additions of the same weight, as
  // BowVector::addWeight performs them), then the words in ascending order
  const bool sums = weighting == 0 || weighting == 1;  // TF_IDF, TF
  std::vector<double> acc(n_words, 0.0);
  std::vector<uint8_t> seen(n_words, 0);
  for (int i = 0; i < n_features; ++i) {
    const int id = word_ids[i];
    const double wgt = word_weight[id];
    if (!(wgt > 0)) continue;
    if (!seen[id]) {
      seen[id] = 1;
      acc[id] = wgt;
    } else if (sums) {
      acc[id] = acc[id] + wgt;
    }
  }
  int n = 0;
  for (int id = 0; id < n_words; ++id) n += seen[id];
  *n_out = n;
  if (n > cap) return OKVFE_ERR_CAPACITY;
  int k = 0;
  for (int id = 0; id < n_words; ++id)
    if (seen[id]) {
      ids_out[k] = id;
      values_out[k] = acc[id];
      ++k;
    }
  if (normalise_l1) {
    double norm = 0.0;
    for (int i = 0; i < n; ++i) norm = norm + std::fabs(values_out[i]);
    if (norm > 0.0)
      for (int i = 0; i < n; ++i) values_out[i] = values_out[i] / norm;
  } else if (sums && n > 0) {
    const double nd = (double)n;
    for (int i = 0; i < n; ++i) values_out[i] = values_out[i] / nd;
  }
  return OKVFE_OK;
}

okvfe_status okvfe_bow_query_l1(okvfe_ctx* ctx, const int32_t* db_begin, const int32_t* db_ids,
                                const double* db_values, int32_t n_entries, const int32_t* q_ids,
                                const double* q_values, int32_t n_q, double* scores) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_entries < 0 || n_q < 0 || !db_begin || (n_entries > 0 && !scores) || (n_q > 0 && (!q_ids || !q_values)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: bad argument");
  if (db_begin[0] != 0) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: db_begin[0] != 0");
  for (int e = 0; e < n_entries; ++e) {
    if (db_begin[e + 1] < db_begin[e])
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: db_begin not monotone at %d", e);
    for (int i = db_begin[e] + 1; i < db_begin[e + 1]; ++i)
      if (db_ids[i] <= db_ids[i - 1])
        return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: entry %d is not in ascending word order", e);
  }
  for (int j = 1; j < n_q; ++j)
    if (q_ids[j] <= q_ids[j - 1])
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: query is not in ascending word order");
  if (n_entries == 0) return OKVFE_OK;
  const int m = db_begin[n_entries];
  if (m > 0 && (!db_ids || !db_values)) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_query_l1: null database");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  const size_t o_b = lay.take((size_t)(n_entries + 1) * 4), o_i = lay.take((size_t)m * 4), o_v = lay.take((size_t)m * 8),
               o_qi = lay.take((size_t)n_q * 4), o_qv = lay.take((size_t)n_q * 8), o_s = lay.take((size_t)n_entries * 8);
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_b, db_begin, (size_t)(n_entries + 1) * 4));
  HIP_TRY(ctx, call.up(o_i, db_ids, (size_t)m * 4));
  HIP_TRY(ctx, call.up(o_v, db_values, (size_t)m * 8));
  HIP_TRY(ctx, call.up(o_qi, q_ids, (size_t)n_q * 4));
  HIP_TRY(ctx, call.up(o_qv, q_values, (size_t)n_q * 8));
  HIP_TRY(ctx, call.sync());  // pageable host buffers: the copies above have completed
  launch_bow_query_l1(call.dev<int32_t>(o_b), call.dev<int32_t>(o_i), call.dev<double>(o_v), n_entries,
                      call.dev<int32_t>(o_qi), call.dev<double>(o_qv), n_q, call.dev<double>(o_s), s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(scores, o_s, (size_t)n_entries * 8));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

// ---- device-resident, batched map matchers (frame f = gather block f) --------------------------
namespace {
okvfe_status map_args_ok(okvfe_ctx* ctx, const char* who, const void* blocks, int n_frames, const okvfe_map_device* map) {
  if (!blocks || !map || n_frames < 1 || map->n_landmarks < 0 || !map->desc_begin ||
      (map->n_landmarks > 0 && !map->pool))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
  return OKVFE_OK;
}
}  // namespace

okvfe_status okvfe_match_to_map_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                              const uint8_t* use_dev, const okvfe_map_device* map,
                                              double reprojection_threshold, int32_t* best_landmark_dev,
                                              int32_t* best_dist_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  okvfe_status st = map_args_ok(ctx, "okvfe_match_to_map_blocks_device", blocks_dev, n_frames, map);
  if (st != OKVFE_OK) return st;
  if (!best_landmark_dev || !best_dist_dev || !(reprojection_threshold >= 0.0) ||
      (map->n_landmarks > 0 && !map->projections))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_blocks_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  uint8_t* perm = nullptr;  // workspace of the region order
  if ((st = stream_workspace(ctx, &ctx->map_perm, s, (size_t)n_frames * ctx->kp_cap * sizeof(int32_t), &perm)) != OKVFE_OK)
    return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_match_to_map_blocks(L, static_cast<const uint8_t*>(blocks_dev), n_frames, ctx->kp_cap, use_dev,
                               map->projections, (size_t)map->n_landmarks * 2, map->desc_begin, map->n_landmarks,
                               map->pool, reprojection_threshold * reprojection_threshold, ctx->cfg.match_threshold,
                               best_landmark_dev, best_dist_dev, reinterpret_cast<int32_t*>(perm), s);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_uninitialised_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                                            const uint8_t* use_dev, const int32_t* previous_landmark_dev,
                                                            const okvfe_map_device* map, const okvfe_pose* T_WC1,
                                                            double focal_length, int32_t* best_landmark_dev,
                                                            int32_t* best_dist_dev, double* hps_W_dev, uint8_t* hp_set_dev,
                                                            int32_t* already_matched_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  okvfe_status st = map_args_ok(ctx, "okvfe_match_to_map_uninitialised_blocks_device", blocks_dev, n_frames, map);
  if (st != OKVFE_OK) return st;
  if (!T_WC1 || !(focal_length > 0.0) || !best_landmark_dev || !best_dist_dev || !hps_W_dev || !hp_set_dev ||
      !already_matched_dev || (map->n_landmarks > 0 && (!map->e0_W || !map->r0_W)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_uninitialised_blocks_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  // one pose record per frame, through the pinned parameter ring (one asynchronous copy, no host sync)
  std::vector<PairParams> pp((size_t)n_frames);
  for (int f = 0; f < n_frames; ++f) pp[(size_t)f] = uninit_pair_params(T_WC1[f], focal_length);
  RingSlot pairs(ctx, &ctx->pair_ring, s);
  if ((st = pairs.upload(pp.data(), pp.size() * sizeof(PairParams))) != OKVFE_OK) return st;
  HIP_TRY(ctx, hipMemsetAsync(already_matched_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_match_to_map_uninit_blocks(pairs.as<PairParams>(), L,
                                      static_cast<const uint8_t*>(blocks_dev), n_frames, ctx->kp_cap, use_dev,
                                      previous_landmark_dev, map->desc_begin, map->n_landmarks, map->pool, map->e0_W,
                                      map->r0_W, ctx->cfg.match_threshold, best_landmark_dev, best_dist_dev, hps_W_dev,
                                      hp_set_dev, already_matched_dev, s);
  }
  return finish_call(ctx, &pairs, s);
}

// ---- matchToMap from a device-resident landmark table, a batch of frames -----------------------
namespace {
// the workspace of stream s for the table passes and the table check: the context's map_table_ws list
okvfe_status map_table_workspace(okvfe_ctx* ctx, hipStream_t s, size_t bytes, uint8_t** out) {
  return stream_workspace(ctx, &ctx->map_table_ws, s, bytes, out);
}

bool table_pointers_ok(const okvfe_landmark_table_device* T) {
  return T && T->n_landmarks >= 0 && T->n_observations >= 0 && T->n_poses >= 0 && T->obs_begin &&
         !(T->n_landmarks > 0 && (!T->hp_W || !T->quality)) &&
         !(T->n_observations > 0 && (!T->obs_pose || !T->obs_desc || !T->obs_backproj || !T->poses));
}
}  // namespace

okvfe_status okvfe_landmark_table_check_device(okvfe_ctx* ctx, const okvfe_landmark_table_device* T, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!table_pointers_ok(T)) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_landmark_table_check_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  uint8_t* ws = nullptr;
  okvfe_status st = map_table_workspace(ctx, s, 256, &ws);
  if (st != OKVFE_OK) return st;
  uint32_t* bad = reinterpret_cast<uint32_t*>(ws);
  uint32_t h_bad[2] = {0, 0};
  HIP_TRY(ctx, hipMemsetAsync(bad, 0xff, sizeof(h_bad), s));
  launch_check_landmark_table(T->obs_begin, T->n_landmarks, T->obs_pose, T->n_observations, T->n_poses, bad, s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  ctx->last_stream = s;
  if (h_bad[0] != 0xffffffffu)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_landmark_table_check_device: obs_begin not monotone at %d", (int)h_bad[0]);
  if (h_bad[1] != 0xffffffffu)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_landmark_table_check_device: observation %d: pose index out of range", (int)h_bad[1]);
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_table_blocks_device(okvfe_ctx* ctx, const okvfe_landmark_table_device* T,
                                                    const void* blocks_dev, int32_t n_frames, const int32_t* cam_ids,
                                                    const okvfe_pose* T_WC1, double reprojection_threshold,
                                                    int32_t exclusive, const uint8_t* use_dev,
                                                    const okvfe_landmark_pool_device* pool_out,
                                                    int32_t* best_landmark_dev, int32_t* best_dist_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!table_pointers_ok(T) || !blocks_dev || n_frames < 0 || !cam_ids || !T_WC1 || !(reprojection_threshold >= 0.0) ||
      !best_landmark_dev || !best_dist_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_table_blocks_device: bad argument");
  bool rt8 = false;  // the 8-coefficient form of the projection only when a slot this call uses holds that model
  std::vector<MapFrameParams> fp((size_t)n_frames);  // poses and camera slots: one record per frame
  okvfe_status st = rig_slots(ctx, RigWho{"okvfe_match_to_map_table_blocks_device", "frame"}, n_frames, cam_ids, &rt8,
                              [&](int f, const DeviceCamera& dc) {
                                fp[(size_t)f].T1 = T_WC1[f];
                                fp[(size_t)f].cos10 = std::cos(10.0 / (dc.fu + dc.fv));  // the SUM, as at Frontend.cpp:1213-1215
                                fp[(size_t)f].cam = cam_ids[f];
                              });
  if (st != OKVFE_OK || n_frames == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  const size_t nl = (size_t)T->n_landmarks, K = (size_t)ctx->kp_cap;
  // workspace per frame: the packed records, the keypoint order and the count of 3-D landmarks; a call that would need
  // more than the limit runs its frames in slices, one after another on the same stream
  const size_t per_frame = nl * sizeof(MapPacked) + K * sizeof(int32_t) + sizeof(int32_t);
  const int slice = map_table_slice_frames(per_frame, ctx->map_table_ws_limit, n_frames);
  const size_t o_perm = align_up((size_t)slice * nl * sizeof(MapPacked), 256),
               o_cnt = align_up(o_perm + (size_t)slice * K * sizeof(int32_t), 256),
               total = o_cnt + (size_t)slice * sizeof(int32_t);
  uint8_t* ws = nullptr;
  if ((st = map_table_workspace(ctx, s, total, &ws)) != OKVFE_OK) return st;
  // the records through the pinned parameter ring (one asynchronous copy, no host sync)
  RingSlot frames(ctx, &ctx->pair_ring, s);
  if ((st = frames.upload(fp.data(), fp.size() * sizeof(MapFrameParams))) != OKVFE_OK) return st;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    MapPacked* packed = reinterpret_cast<MapPacked*>(ws);
    int32_t* perm = reinterpret_cast<int32_t*>(ws + o_perm);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + o_cnt);
    for (int f0 = 0; f0 < n_frames; f0 += slice) {
      const int nf = std::min(slice, n_frames - f0);
      const size_t row = (size_t)f0 * nl;  // first row of the slice in the caller's frame-major pool arrays
      auto at = [&](auto* p, size_t per_row) { return p ? p + row * per_row : p; };
      launch_prepare_landmarks_frames(
          T->hp_W, T->quality, T->obs_begin, T->n_landmarks, T->obs_pose, T->obs_backproj, T->poses,
          frames.as<MapFrameParams>() + f0, nf, ctx->d_cams, ctx->w, ctx->h, reprojection_threshold,
          exclusive ? 1 : 0, std::cos(0.6), at(pool_out ? pool_out->status : nullptr, 1),
          at(pool_out ? pool_out->n_desc : nullptr, 1), at(pool_out ? pool_out->obs_rows : nullptr, 3),
          at(pool_out ? pool_out->projection : nullptr, 2), at(pool_out ? pool_out->e_W : nullptr, 6),
          at(pool_out ? pool_out->r_W : nullptr, 6), packed, counts, s, rt8);
      launch_match_to_map_table_blocks(L, static_cast<const uint8_t*>(blocks_dev) + (size_t)f0 * L.total, nf,
                                       ctx->kp_cap, use_dev ? use_dev + (size_t)f0 * K : nullptr, packed, counts,
                                       T->n_landmarks, T->obs_desc, reprojection_threshold * reprojection_threshold,
                                       ctx->cfg.match_threshold, best_landmark_dev + (size_t)f0 * K,
                                       best_dist_dev + (size_t)f0 * K, perm, s);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  const okvfe_status rel = frames.release();
  ctx->last_stream = s;
  return rel;
}

okvfe_status okvfe_match_to_map_table_uninitialised_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* T, const okvfe_landmark_pool_device* pool, const void* blocks_dev,
    int32_t n_frames, const int32_t* cam_ids, const okvfe_pose* T_WC1, int32_t exclusive, const uint8_t* use_dev,
    const int32_t* previous_landmark_dev, int32_t* best_landmark_dev, int32_t* best_dist_dev, double* hps_W_dev,
    uint8_t* hp_set_dev, int32_t* already_matched_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || T->n_landmarks < 0 || !pool || !blocks_dev || n_frames < 0 || !cam_ids || !T_WC1 || !best_landmark_dev ||
      !best_dist_dev || !hps_W_dev || !hp_set_dev || !already_matched_dev ||
      (T->n_landmarks > 0 && (!T->obs_desc || !pool->status || !pool->n_desc || !pool->obs_rows || !pool->e_W || !pool->r_W)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_to_map_table_uninitialised_blocks_device: bad argument");
  // the pose NOW and the gate constants of the frame's camera slot: one record per frame
  std::vector<PairParams> pp((size_t)n_frames);
  okvfe_status st = rig_slots(ctx, RigWho{"okvfe_match_to_map_table_uninitialised_blocks_device", "frame"}, n_frames,
                              cam_ids, nullptr, [&](int f, const DeviceCamera& dc) {
                                pp[(size_t)f] = uninit_pair_params(T_WC1[f], 0.5 * (dc.fu + dc.fv));
                              });
  if (st != OKVFE_OK || n_frames == 0) return st;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  const size_t nl = (size_t)T->n_landmarks, K = (size_t)ctx->kp_cap;
  // workspace per frame: one packed record per landmark and the count of the status-2 set; slices as in the first pass
  const size_t per_frame = nl * sizeof(MapUninitPacked) + sizeof(int32_t);
  const int slice = map_table_slice_frames(per_frame, ctx->map_table_ws_limit, n_frames);
  const size_t o_cnt = align_up((size_t)slice * nl * sizeof(MapUninitPacked), 256),
               total = o_cnt + (size_t)slice * sizeof(int32_t);
  uint8_t* ws = nullptr;
  if ((st = map_table_workspace(ctx, s, total, &ws)) != OKVFE_OK) return st;
  // the records through the pinned parameter ring (one asynchronous copy, no host sync)
  RingSlot pairs(ctx, &ctx->pair_ring, s);
  if ((st = pairs.upload(pp.data(), pp.size() * sizeof(PairParams))) != OKVFE_OK) return st;
  HIP_TRY(ctx, hipMemsetAsync(already_matched_dev, 0, (size_t)n_frames * sizeof(int32_t), s));
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    MapUninitPacked* packed = reinterpret_cast<MapUninitPacked*>(ws);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + o_cnt);
    for (int f0 = 0; f0 < n_frames; f0 += slice) {
      const int nf = std::min(slice, n_frames - f0);
      const size_t row = (size_t)f0 * nl;  // first row of the slice in the caller's frame-major pool arrays
      auto at = [&](auto* p, size_t per_row) { return p ? p + row * per_row : p; };
      launch_pack_uninit_frames(at(pool->status, 1), at(pool->n_desc, 1), at(pool->obs_rows, 3), T->n_landmarks, nf,
                                packed, counts, s);
      launch_match_to_map_table_uninit_blocks(
          pairs.as<PairParams>() + f0, L, static_cast<const uint8_t*>(blocks_dev) + (size_t)f0 * L.total,
          nf, ctx->kp_cap, use_dev ? use_dev + (size_t)f0 * K : nullptr,
          previous_landmark_dev ? previous_landmark_dev + (size_t)f0 * K : nullptr, exclusive ? 1 : 0, packed, counts,
          T->n_landmarks, T->obs_desc, at(pool->e_W, 6), at(pool->r_W, 6), ctx->cfg.match_threshold,
          best_landmark_dev + (size_t)f0 * K, best_dist_dev + (size_t)f0 * K, hps_W_dev + 4 * (size_t)f0 * K,
          hp_set_dev + (size_t)f0 * K, already_matched_dev + f0, s);
      HIP_TRY(ctx, hipGetLastError());  // (an early return leaves the slot to ~RingSlot)
    }
  }
  const okvfe_status rel = pairs.release();  // ring_release() behind the last launch of the last slice
  ctx->last_stream = s;
  return rel;
}

// Test hook, deliberately not in include/okvfe.h: lowers the workspace limit above which
// okvfe_match_to_map_table_blocks_device and okvfe_match_to_map_table_uninitialised_blocks_device cut a call into slices of
// frames, so that a test reaches that path with a small batch (0 restores the default of 1 GiB).
okvfe_status okvfe_test_set_map_table_workspace_limit(okvfe_ctx* ctx, uint64_t bytes) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  ctx->map_table_ws_limit = bytes ? (size_t)bytes : (size_t)1 << 30;
  return OKVFE_OK;
}

okvfe_status okvfe_verify_place_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                              const okvfe_map_device* map, int32_t* k_min_dev,
                                              uint32_t* dist_min_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  okvfe_status st = map_args_ok(ctx, "okvfe_verify_place_blocks_device", blocks_dev, n_frames, map);
  if (st != OKVFE_OK) return st;
  if (!k_min_dev || !dist_min_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_verify_place_blocks_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_verify_place_blocks(map->pool, map->desc_begin, map->n_landmarks, L,
                               static_cast<const uint8_t*>(blocks_dev), n_frames, ctx->kp_cap,
                               (uint32_t)ctx->cfg.match_threshold, k_min_dev, dist_min_dev, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}
}  // extern "C"
