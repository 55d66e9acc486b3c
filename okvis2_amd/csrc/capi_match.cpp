// capi_match.cpp -- the Hamming matchers behind the C ABI: matchStereo (Frontend.cpp:2016-2076),
// matchMotionStereo (:1789-1905), candidate lists / arg-min, and the gather blocks that carry one
// image's results between GPUs and into the device-resident matchers.
#include "okvfe_ctx.h"

using namespace okvfe;

extern "C" {

okvfe_status okvfe_match_stereo_batch_device(okvfe_ctx* ctx, const okvfe_stereo_pair* pairs,
                                             int32_t n_pairs, okvfe_stereo_match* matches_dev,
                                             void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!pairs || !matches_dev || n_pairs < 1)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_stereo_batch_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  std::vector<PairParams> pp(n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    if (pairs[i].image0 < 0 || pairs[i].image0 >= ctx->B || pairs[i].image1 < 0 || pairs[i].image1 >= ctx->B ||
        !(pairs[i].f0 > 0.0) || !(pairs[i].f1 > 0.0))
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "pair %d: image index or focal length out of range", i);
    pp[i] = to_pair_params(pairs[i]);
  }
  // pipelined lanes (okvfe_set_internal_lanes(-k)): the pairs of a slice are matched on the slice's lane stream, behind
  // its detect + describe chain, when every pair lies inside one slice and the slices' pairs are contiguous runs
  std::vector<int> lane_first;
  bool piped = ctx->lanes_pipelined && ctx->lanes_open && ctx->n_layers == 1 && ctx->lane_chunk > 0 &&
               ctx->lanes_used > 1 && (int)ctx->lane_ctx.size() >= ctx->lanes_used && ctx->join_stream;
  if (piped) {
    lane_first.assign(ctx->lanes_used + 1, n_pairs);
    int cur = -1;
    for (int i = 0; i < n_pairs && piped; ++i) {
      const int l0 = pairs[i].image0 / ctx->lane_chunk, l1 = pairs[i].image1 / ctx->lane_chunk;
      if (l0 != l1 || l0 < cur || l0 >= ctx->lanes_used) piped = false;
      while (piped && cur < l0) lane_first[++cur] = i;
    }
    while (piped && cur < ctx->lanes_used - 1) lane_first[++cur] = n_pairs;
  }
  hipStream_t s = piped ? pick_stream_raw(ctx, stream) : pick_stream(ctx, stream);
  okvfe_status st;
  RingSlot cls(ctx, &ctx->cls_ring, s), prm(ctx, &ctx->pair_ring, s);
  if (ctx->n_layers > 1) {
    // one table per distinct (f0, f1); usually one for the whole call
    std::vector<double> tables;
    std::vector<std::pair<double, double>> seen;
    std::vector<int> which(n_pairs);
    for (int i = 0; i < n_pairs; ++i) {
      int j = 0;
      for (; j < (int)seen.size(); ++j)
        if (seen[j].first == pairs[i].f0 && seen[j].second == pairs[i].f1) break;
      if (j == (int)seen.size()) {
        seen.emplace_back(pairs[i].f0, pairs[i].f1);
        tables.resize(tables.size() + kClassTableDoubles);
        fill_class_table(tables.data() + (size_t)j * kClassTableDoubles, pairs[i].f0, pairs[i].f1, false);
      }
      which[i] = j;
    }
    if ((st = cls.upload(tables.data(), tables.size() * sizeof(double))) != OKVFE_OK) return st;
    for (int i = 0; i < n_pairs; ++i) pp[i].cls = cls.as<double>() + (size_t)which[i] * kClassTableDoubles;
  }
  if ((st = prm.upload(pp.data(), (size_t)n_pairs * sizeof(PairParams))) != OKVFE_OK) return st;
  if (piped) {
    HIP_TRY(ctx, hipEventRecord(ctx->lane_fork, s));  // behind the pair upload
    for (int l = 0; l < ctx->lanes_used; ++l) {
      const int first = lane_first[l], n = lane_first[l + 1] - first;
      hipStream_t ls = ctx->lane_ctx[l]->stream;
      HIP_TRY(ctx, hipStreamWaitEvent(ls, ctx->lane_fork, 0));
      if (n > 0) {
        StageTimer t(ctx, OKVFE_STAGE_MATCH, ls);
        launch_match_stereo(prm.as<PairParams>() + first, n, ctx->d_kps, ctx->d_desc, ctx->d_bp,
                            ctx->d_bpv, ctx->d_count, ctx->kp_cap, ctx->cfg.match_threshold,
                            matches_dev + (size_t)first * ctx->kp_cap, ls);
      }
      HIP_TRY(ctx, hipEventRecord(ctx->lane_done[l], ls));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->join_stream, ctx->lane_done[l], 0));
    }
    if ((st = prm.release(ctx->join_stream)) != OKVFE_OK) return st;
    HIP_TRY(ctx, hipEventRecord(ctx->join_done, ctx->join_stream));
    HIP_TRY(ctx, hipGetLastError());
    ctx->last_stream = s;
    return OKVFE_OK;
  }
  {
    StageTimer t(ctx, OKVFE_STAGE_MATCH, s);
    launch_match_stereo(prm.as<PairParams>(), n_pairs, ctx->d_kps, ctx->d_desc, ctx->d_bp,
                        ctx->d_bpv, ctx->d_count, ctx->kp_cap, ctx->cfg.match_threshold, matches_dev, s);
  }
  if ((st = prm.release()) != OKVFE_OK) return st;
  if ((st = cls.release()) != OKVFE_OK) return st;
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_match_stereo(okvfe_ctx* ctx, const uint8_t* desc0, const okvfe_keypoint* kp0,
                                const double* backproj0, const uint8_t* valid0, int32_t n0,
                                const uint8_t* desc1, const okvfe_keypoint* kp1, const double* backproj1,
                                const uint8_t* valid1, int32_t n1, const okvfe_pose* T_WC0,
                                const okvfe_pose* T_WC1, double f0, double f1, okvfe_stereo_match* matches) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n0 < 0 || n1 < 0 || !T_WC0 || !T_WC1 || !(f0 > 0.0) || !(f1 > 0.0) ||
      (n0 > 0 && (!desc0 || !backproj0 || !valid0 || !matches)) || (n1 > 0 && (!desc1 || !backproj1 || !valid1)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_stereo: bad argument");
  // keypoint sizes select the triangulation sigma (Frontend.cpp:2031-2035): sizes must be
  // 12 * scale(octave); only a scale-space detector produces anything but 12
  bool multi = false;
  okvfe_status st = check_size_classes(ctx, kp0, n0, &multi);
  if (st == OKVFE_OK) st = check_size_classes(ctx, kp1, n1, &multi);
  if (st != OKVFE_OK) return st;
  if (multi && (!kp0 || !kp1)) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_stereo: keypoints needed");
  if (n0 == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  ScratchLayout lay;
  const size_t o_pair = lay.take(sizeof(PairParams)), o_cls = lay.take(kClassTableDoubles * sizeof(double));
  const size_t o_d0 = lay.take((size_t)n0 * 48), o_b0 = lay.take((size_t)n0 * 24), o_v0 = lay.take(n0),
               o_k0 = lay.take((size_t)n0 * sizeof(okvfe_keypoint));
  const size_t o_d1 = lay.take((size_t)n1 * 48), o_b1 = lay.take((size_t)n1 * 24), o_v1 = lay.take(n1),
               o_k1 = lay.take((size_t)n1 * sizeof(okvfe_keypoint));
  const size_t o_out = lay.take((size_t)n0 * sizeof(okvfe_stereo_match));
  ScratchCall call(ctx, ctx->stream);
  if ((st = call.reserve(lay, true)) != OKVFE_OK) return st;
  okvfe_stereo_pair sp{};
  sp.image0 = 0; sp.image1 = 0; sp.T_WC0 = *T_WC0; sp.T_WC1 = *T_WC1; sp.f0 = f0; sp.f1 = f1;
  PairParams pp = to_pair_params(sp);
  if (multi) {
    fill_class_table(call.host<double>(o_cls), f0, f1, false);
    pp.cls = call.dev<double>(o_cls);
    call.put(o_k0, kp0, (size_t)n0 * sizeof(okvfe_keypoint));
    call.put(o_k1, kp1, (size_t)n1 * sizeof(okvfe_keypoint));
  }
  call.put(o_pair, &pp, sizeof(pp));
  call.put(o_d0, desc0, (size_t)n0 * 48);
  call.put(o_b0, backproj0, (size_t)n0 * 24);
  call.put(o_v0, valid0, (size_t)n0);
  call.put(o_d1, desc1, (size_t)n1 * 48);
  call.put(o_b1, backproj1, (size_t)n1 * 24);
  call.put(o_v1, valid1, (size_t)n1);
  // One kernel moves every input (it reads the pinned block in place), the matcher writes its rows
  // straight into the pinned block, one synchronisation: a frame's matchStereo was seven pageable
  // host-to-device copies, a synchronisation, the kernel, a copy back and another synchronisation
  // (75 us for a 17 us kernel at B = 1)
  HIP_TRY(ctx, call.move_in(o_out));
  launch_match_stereo_arrays(call.dev<PairParams>(o_pair), call.dev(o_d0), call.dev<double>(o_b0), call.dev(o_v0), nullptr,
                             n0, call.dev(o_d1), call.dev<double>(o_b1), call.dev(o_v1), nullptr, n1, n0,
                             ctx->cfg.match_threshold, call.result<okvfe_stereo_match>(o_out), ctx->stream,
                             multi ? call.dev<const okvfe_keypoint>(o_k0) : nullptr,
                             multi ? call.dev<const okvfe_keypoint>(o_k1) : nullptr);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.fetch(matches, o_out, (size_t)n0 * sizeof(okvfe_stereo_match)));
  return OKVFE_OK;
}

okvfe_status okvfe_match_motion_stereo(okvfe_ctx* ctx, const okvfe_camera* camera, const uint8_t* desc0,
                                       const okvfe_keypoint* kp0, const double* backproj0, const uint8_t* valid0,
                                       const uint8_t* skip0, int32_t n0, const uint8_t* desc1,
                                       const okvfe_keypoint* kp1, const double* backproj1, const uint8_t* valid1,
                                       const uint8_t* matched1, int32_t n1, const okvfe_pose* T_WC0,
                                       const okvfe_pose* T_WC1, okvfe_motion_match* matches) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!camera || camera->distortion == OKVFE_DIST_RADTAN8)  // (its k3..k6 need okvfe_camera_ext)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_motion_stereo: bad argument");
  const okvfe_camera_ext e = widen_camera(*camera);
  return okvfe_match_motion_stereo_ext(ctx, &e, desc0, kp0, backproj0, valid0, skip0, n0, desc1, kp1, backproj1,
                                       valid1, matched1, n1, T_WC0, T_WC1, matches);
}

okvfe_status okvfe_match_motion_stereo_ext(okvfe_ctx* ctx, const okvfe_camera_ext* camera_ext, const uint8_t* desc0,
                                           const okvfe_keypoint* kp0, const double* backproj0, const uint8_t* valid0,
                                           const uint8_t* skip0, int32_t n0, const uint8_t* desc1,
                                           const okvfe_keypoint* kp1, const double* backproj1, const uint8_t* valid1,
                                           const uint8_t* matched1, int32_t n1, const okvfe_pose* T_WC0,
                                           const okvfe_pose* T_WC1, okvfe_motion_match* matches) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  const okvfe_camera* camera = camera_ext ? &camera_ext->base : nullptr;
  if (!camera || camera->distortion < OKVFE_DIST_NONE || camera->distortion > OKVFE_DIST_RADTAN8 || n0 < 0 || n1 < 0 || !T_WC0 || !T_WC1 ||
      (n0 > 0 && (!desc0 || !kp0 || !backproj0 || !valid0 || !matches)) ||
      (n1 > 0 && (!desc1 || !kp1 || !backproj1 || !valid1)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_motion_stereo: bad argument");
  bool multi = false;
  {
    okvfe_status cst = check_size_classes(ctx, kp0, n0, &multi);
    if (cst == OKVFE_OK) cst = check_size_classes(ctx, kp1, n1, &multi);
    if (cst != OKVFE_OK) return cst;
  }
  if (n0 == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  ScratchLayout lay;
  const size_t o_pair = lay.take(sizeof(PairParams)), o_cam = lay.take(sizeof(DeviceCamera)),
               o_cls = lay.take(kClassTableDoubles * sizeof(double));
  const size_t o_d0 = lay.take((size_t)n0 * 48), o_k0 = lay.take((size_t)n0 * sizeof(okvfe_keypoint)),
               o_b0 = lay.take((size_t)n0 * 24), o_v0 = lay.take(n0), o_s0 = lay.take(n0);
  const size_t o_d1 = lay.take((size_t)n1 * 48), o_k1 = lay.take((size_t)n1 * sizeof(okvfe_keypoint)),
               o_b1 = lay.take((size_t)n1 * 24), o_v1 = lay.take(n1), o_m1 = lay.take(n1);
  const size_t o_out = lay.take((size_t)n0 * sizeof(okvfe_motion_match));
  ScratchCall call(ctx, ctx->stream);  // the pinned variant (see okvfe_match_stereo)
  const okvfe_status st = call.reserve(lay, true);
  if (st != OKVFE_OK) return st;
  okvfe_stereo_pair sp{};
  sp.T_WC0 = *T_WC0; sp.T_WC1 = *T_WC1;
  sp.f0 = sp.f1 = 0.5 * (camera->fu + camera->fv);  // sigma = size0 / f0 * 0.125 (Frontend.cpp:1834)
  PairParams pp = to_pair_params(sp);
  const DeviceCamera dc = to_device_camera(*camera_ext);
  if (multi) {
    fill_class_table(call.host<double>(o_cls), sp.f0, sp.f1, true);
    pp.cls = call.dev<double>(o_cls);
  }
  call.put(o_pair, &pp, sizeof(pp));
  call.put(o_cam, &dc, sizeof(dc));
  call.put(o_d0, desc0, (size_t)n0 * 48);
  call.put(o_k0, kp0, (size_t)n0 * sizeof(okvfe_keypoint));
  call.put(o_b0, backproj0, (size_t)n0 * 24);
  call.put(o_v0, valid0, n0);
  if (skip0) call.put(o_s0, skip0, n0);
  call.put(o_d1, desc1, (size_t)n1 * 48);
  call.put(o_k1, kp1, (size_t)n1 * sizeof(okvfe_keypoint));
  call.put(o_b1, backproj1, (size_t)n1 * 24);
  call.put(o_v1, valid1, n1);
  if (matched1) call.put(o_m1, matched1, n1);
  HIP_TRY(ctx, call.move_in(o_out));
  launch_match_motion(call.dev<PairParams>(o_pair), call.dev<DeviceCamera>(o_cam), camera->width, camera->height,
                      call.dev(o_d0), call.dev<okvfe_keypoint>(o_k0), call.dev<double>(o_b0), call.dev(o_v0),
                      skip0 ? call.dev(o_s0) : nullptr, n0, call.dev(o_d1), call.dev<okvfe_keypoint>(o_k1),
                      call.dev<double>(o_b1), call.dev(o_v1), matched1 ? call.dev(o_m1) : nullptr, n1,
                      ctx->cfg.match_threshold, call.result<okvfe_motion_match>(o_out), ctx->stream,
                      dc.distortion == OKVFE_DIST_RADTAN8);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.fetch(matches, o_out, (size_t)n0 * sizeof(okvfe_motion_match)));
  return OKVFE_OK;
}

okvfe_status okvfe_hamming_candidates(okvfe_ctx* ctx, const uint8_t* A, int32_t nA, const uint8_t* B,
                                      int32_t nB, int32_t threshold, okvfe_candidate* out, int32_t cap,
                                      int32_t* n_out) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (nA < 0 || nB < 0 || !n_out || cap < 0 || (nA > 0 && !A) || (nB > 0 && !B) || (cap > 0 && !out))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_hamming_candidates: bad argument");
  *n_out = 0;
  if (nA == 0 || nB == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = ctx->stream;
  ScratchLayout lay;
  const size_t o_A = lay.take((size_t)nA * 48), o_B = lay.take((size_t)nB * 48), o_rows = lay.take((size_t)nA * 4),
               o_out = lay.take((size_t)cap * sizeof(okvfe_candidate));
  ScratchCall call(ctx, s);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_A, A, (size_t)nA * 48));
  HIP_TRY(ctx, call.up(o_B, B, (size_t)nB * 48));
  HIP_TRY(ctx, call.sync());
  launch_hamming_count(call.dev(o_A), nA, call.dev(o_B), nB, threshold, call.dev<int32_t>(o_rows), s);
  std::vector<int32_t> rows(nA);
  HIP_TRY(ctx, call.down(rows.data(), o_rows, (size_t)nA * 4));
  HIP_TRY(ctx, call.sync());
  int64_t total_c = 0;
  for (int i = 0; i < nA; ++i) {
    const int32_t c = rows[i];
    rows[i] = (int32_t)std::min<int64_t>(total_c, INT32_MAX);
    total_c += c;
  }
  *n_out = (int32_t)std::min<int64_t>(total_c, INT32_MAX);
  HIP_TRY(ctx, call.up(o_rows, rows.data(), (size_t)nA * 4));
  HIP_TRY(ctx, call.sync());
  launch_hamming_emit(call.dev(o_A), nA, call.dev(o_B), nB, threshold, call.dev<int32_t>(o_rows),
                      call.dev<okvfe_candidate>(o_out), cap, s);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(out, o_out, (size_t)std::min<int64_t>(total_c, cap) * sizeof(okvfe_candidate)));
  HIP_TRY(ctx, call.sync());
  if (total_c > cap) return fail(ctx, OKVFE_ERR_CAPACITY, "%lld candidates, caller capacity %d", (long long)total_c, cap);
  return OKVFE_OK;
}

okvfe_status okvfe_hamming_argmin(okvfe_ctx* ctx, const uint8_t* A, int32_t nA, const uint8_t* B, int32_t nB,
                                  uint32_t threshold, int32_t* best_j, uint32_t* best_dist) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (nA < 0 || nB < 0 || (nA > 0 && (!A || !best_j || !best_dist)) || (nB > 0 && !B))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_hamming_argmin: bad argument");
  if (nA == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  ScratchLayout lay;
  const size_t o_A = lay.take((size_t)nA * 48), o_B = lay.take((size_t)nB * 48), o_j = lay.take((size_t)nA * 4),
               o_d = lay.take((size_t)nA * 4);
  ScratchCall call(ctx, ctx->stream);
  const okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_A, A, (size_t)nA * 48));
  HIP_TRY(ctx, call.up(o_B, B, (size_t)nB * 48));
  HIP_TRY(ctx, call.sync());
  launch_hamming_argmin(call.dev(o_A), nA, call.dev(o_B), nB, threshold, call.dev<int32_t>(o_j), call.dev<uint32_t>(o_d),
                        ctx->stream);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, call.down(best_j, o_j, (size_t)nA * 4));
  HIP_TRY(ctx, call.down(best_dist, o_d, (size_t)nA * 4));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

size_t okvfe_gather_block_bytes(const okvfe_ctx* ctx) { return ctx ? block_layout(ctx->kp_cap).total : 0; }

okvfe_status okvfe_pack_gather_blocks_device(okvfe_ctx* ctx, int32_t first_index, int32_t n, void* blocks_dev,
                                             void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (first_index < 0 || n < 1 || first_index + n > ctx->B || !blocks_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_pack_gather_blocks_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  launch_pack_blocks(L, first_index, n, ctx->kp_cap, ctx->d_count, ctx->d_kps, ctx->d_desc, ctx->d_bp,
                     ctx->d_bpv, static_cast<uint8_t*>(blocks_dev), s);
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_pack_gather_block_device(okvfe_ctx* ctx, int32_t index, void* block_dev, void* stream) {
  return okvfe_pack_gather_blocks_device(ctx, index, 1, block_dev, stream);
}

okvfe_status okvfe_match_stereo_blocks_batch_device(okvfe_ctx* ctx, const void* blocks0_dev,
                                                    const void* blocks1_dev, int32_t n_frames,
                                                    const okvfe_pose* T_WC0, const okvfe_pose* T_WC1, double f0,
                                                    double f1, okvfe_stereo_match* matches_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!blocks0_dev || !blocks1_dev || n_frames < 1 || !T_WC0 || !T_WC1 || !matches_dev || !(f0 > 0.0) || !(f1 > 0.0))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_stereo_blocks_batch_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  okvfe_stereo_pair sp{};
  sp.T_WC0 = *T_WC0; sp.T_WC1 = *T_WC1; sp.f0 = f0; sp.f1 = f1;
  PairParams pp = to_pair_params(sp);
  RingSlot cls(ctx, &ctx->cls_ring, s);
  if (ctx->n_layers > 1) {
    double table[kClassTableDoubles];
    fill_class_table(table, f0, f1, false);
    okvfe_status st = cls.upload(table, sizeof(table));
    if (st != OKVFE_OK) return st;
    pp.cls = cls.as<double>();
  }
  // the pair record travels by value as a kernel argument: nothing to keep alive
  launch_match_stereo_blocks(pp, L, static_cast<const uint8_t*>(blocks0_dev),
                             static_cast<const uint8_t*>(blocks1_dev), n_frames, ctx->kp_cap,
                             ctx->cfg.match_threshold, matches_dev, s);
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return cls.release();
}
okvfe_status okvfe_match_motion_stereo_blocks_device(okvfe_ctx* ctx, int32_t cam, const void* block0_dev,
                                                     const void* block1_dev, const uint8_t* skip0_dev,
                                                     const uint8_t* matched1_dev, const okvfe_pose* T_WC0,
                                                     const okvfe_pose* T_WC1, okvfe_motion_match* matches_dev,
                                                     void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!block0_dev || !block1_dev || !T_WC0 || !T_WC1 || !matches_dev || cam < 0 ||
      cam >= (int)ctx->h_cams.size())
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_match_motion_stereo_blocks_device: bad argument");
  const RigWho who{nullptr, nullptr, OKVFE_ERR_INVALID_ARGUMENT};
  const DeviceCamera* slot = rig_slot(ctx, who, 0, cam);
  if (!slot) return who.bad;
  const DeviceCamera& dc = *slot;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  okvfe_stereo_pair sp{};
  sp.T_WC0 = *T_WC0; sp.T_WC1 = *T_WC1;
  sp.f0 = sp.f1 = 0.5 * (dc.fu + dc.fv);  // sigma = size0 / f0 * 0.125 (Frontend.cpp:1834)
  PairParams pp = to_pair_params(sp);
  RingSlot cls(ctx, &ctx->cls_ring, s);
  if (ctx->n_layers > 1) {
    double table[kClassTableDoubles];
    fill_class_table(table, sp.f0, sp.f1, true);
    okvfe_status st = cls.upload(table, sizeof(table));
    if (st != OKVFE_OK) return st;
    pp.cls = cls.as<double>();
  }
  launch_match_motion_blocks(pp, ctx->d_cams + cam, ctx->w, ctx->h, L,
                             static_cast<const uint8_t*>(block0_dev), static_cast<const uint8_t*>(block1_dev),
                             skip0_dev, matched1_dev, ctx->kp_cap, ctx->cfg.match_threshold, matches_dev, s,
                             dc.distortion == OKVFE_DIST_RADTAN8);
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return cls.release();
}

okvfe_status okvfe_match_motion_stereo_blocks_batch_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_blocks0, const void* blocks1_dev, int32_t n_blocks1,
    int32_t n_pairs, const int32_t* idx0, const int32_t* idx1, const int32_t* cam_ids, const okvfe_pose* T_WC0,
    const okvfe_pose* T_WC1, const uint8_t* skip0_dev, const uint8_t* matched1_dev, okvfe_motion_match* matches_dev,
    const okvfe_motion_claim_device* claim, void* stream) {
  static const char* const fn = "okvfe_match_motion_stereo_blocks_batch_device";
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_pairs < 0 || n_blocks0 < 0 || n_blocks1 < 0)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: negative count (n_blocks0 %d, n_blocks1 %d, n_pairs %d)", fn,
                n_blocks0, n_blocks1, n_pairs);
  if (n_pairs == 0) return OKVFE_OK;
  if (!blocks0_dev || !blocks1_dev || !cam_ids || !T_WC0 || !T_WC1 || !matches_dev)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: NULL %s", fn,
                !blocks0_dev ? "blocks0_dev" : !blocks1_dev ? "blocks1_dev" : !cam_ids ? "cam_ids"
                : !T_WC0 ? "T_WC0" : !T_WC1 ? "T_WC1" : "matches_dev");
  if (claim && (!claim->claimed || !claim->n_claimed))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: NULL claim->%s", fn, !claim->claimed ? "claimed" : "n_claimed");
  // every record is built and checked before anything is queued
  std::vector<MotionPairRecord> recs((size_t)n_pairs);
  std::vector<int> slots;                                   // distinct camera slots of the call ...
  std::vector<int> slot_of((size_t)n_pairs);                // ... and each pair's position among them
  std::vector<int32_t> user(claim ? (size_t)n_blocks1 : 0, -1);  // with claims: the pair that names a current block
  bool rt8 = false;
  const RigWho who{fn, "pair", OKVFE_ERR_INVALID_ARGUMENT};
  for (int p = 0; p < n_pairs; ++p) {
    const int i0 = idx0 ? idx0[p] : p, i1 = idx1 ? idx1[p] : p, cam = cam_ids[p];
    if (i0 < 0 || i0 >= n_blocks0)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: older block %d outside [0, %d)", fn, p, i0, n_blocks0);
    if (i1 < 0 || i1 >= n_blocks1)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: current block %d outside [0, %d)", fn, p, i1, n_blocks1);
    if (cam < 0 || cam >= (int)ctx->h_cams.size())
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: camera slot %d outside [0, %d)", fn, p, cam,
                  (int)ctx->h_cams.size());
    const DeviceCamera* slot = rig_slot(ctx, who, p, cam);  // (not rig_slots: a pair's checks stay in their order)
    if (!slot) return who.bad;
    const DeviceCamera& dc = *slot;
    if (claim) {
      if (user[i1] >= 0)
        return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT,
                    "%s: current block %d is named by pairs %d and %d: with claims a call resolves a current block once",
                    fn, i1, user[i1], p);
      user[i1] = p;
    }
    rt8 = rt8 || dc.distortion == OKVFE_DIST_RADTAN8;
    okvfe_stereo_pair sp{};
    sp.T_WC0 = T_WC0[p]; sp.T_WC1 = T_WC1[p];
    sp.f0 = sp.f1 = 0.5 * (dc.fu + dc.fv);  // sigma = size0 / f0 * 0.125 (Frontend.cpp:1834)
    recs[p].pair = to_pair_params(sp);
    recs[p].cam = cam; recs[p].idx0 = i0; recs[p].idx1 = i1; recs[p].pad = 0;
    size_t j = 0;
    while (j < slots.size() && slots[j] != cam) ++j;
    if (j == slots.size()) slots.push_back(cam);
    slot_of[p] = (int)j;
  }
  if (claim && ctx->kp_cap > kMotionClaimMaxKeypoints)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: claims need max_keypoints <= %d (this context: %d)", fn,
                kMotionClaimMaxKeypoints, ctx->kp_cap);
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  okvfe_status st;
  RingSlot cls(ctx, &ctx->cls_ring, s), rec(ctx, &ctx->pair_ring, s);
  if (ctx->n_layers > 1) {  // one size-class table per distinct camera slot
    std::vector<double> tables(slots.size() * kClassTableDoubles);
    for (size_t j = 0; j < slots.size(); ++j) {
      const DeviceCamera& dc = ctx->h_cams[slots[j]];
      const double f = 0.5 * (dc.fu + dc.fv);
      fill_class_table(tables.data() + j * kClassTableDoubles, f, f, true);
    }
    if ((st = cls.upload(tables.data(), tables.size() * sizeof(double))) != OKVFE_OK) return st;
    for (int p = 0; p < n_pairs; ++p) recs[p].pair.cls = cls.as<double>() + (size_t)slot_of[p] * kClassTableDoubles;
  }
  if ((st = rec.upload(recs.data(), recs.size() * sizeof(MotionPairRecord))) != OKVFE_OK) return st;
  launch_match_motion_pairs(rec.as<MotionPairRecord>(), n_pairs, ctx->d_cams, ctx->w, ctx->h, L,
                            static_cast<const uint8_t*>(blocks0_dev), static_cast<const uint8_t*>(blocks1_dev),
                            skip0_dev, matched1_dev, ctx->kp_cap, ctx->cfg.match_threshold, matches_dev, s, rt8);
  if (claim)  // behind the match kernel on the stream: matched1_out may be matched1_dev
    launch_motion_claim(rec.as<MotionPairRecord>(), n_pairs, L,
                        static_cast<const uint8_t*>(blocks0_dev), ctx->kp_cap, matches_dev, claim->claimed,
                        claim->n_claimed, claim->matched1_out, s);
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  if ((st = rec.release()) != OKVFE_OK) return st;
  return cls.release();
}

okvfe_status okvfe_match_stereo_blocks_device(okvfe_ctx* ctx, const void* block0_dev, const void* block1_dev,
                                              const okvfe_pose* T_WC0, const okvfe_pose* T_WC1, double f0,
                                              double f1, okvfe_stereo_match* matches_dev, void* stream) {
  return okvfe_match_stereo_blocks_batch_device(ctx, block0_dev, block1_dev, 1, T_WC0, T_WC1, f0, f1, matches_dev,
                                                stream);
}

}  // extern "C"
