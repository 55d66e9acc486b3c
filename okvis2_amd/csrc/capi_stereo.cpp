// capi_stereo.cpp -- the landmark bookkeeping of Frontend::matchStereo (Frontend.cpp:2076-2141) behind the C ABI, chained
// over the camera pairs of a rig on device-resident batches (k_map.hip, stereo_insert_kernel).
#include <algorithm>

#include "okvfe_ctx.h"

using namespace okvfe;

extern "C" {

okvfe_status okvfe_stereo_insert_blocks_device(
    okvfe_ctx* ctx, const okvfe_landmark_table_device* T, const uint8_t* initialised_dev, const void* blocks_dev,
    int32_t block_stride_m, int32_t block_stride_c, int32_t n_multiframes, int32_t n_cams, const int32_t* pairs,
    int32_t n_pairs, const int32_t* cam_ids, const okvfe_pose* T_WC, const okvfe_stereo_match* matches_dev,
    const int32_t* landmark_dev, const uint8_t* as_keyframe_dev, const okvfe_stereo_insert_device* result, void* stream) {
  static const char* kName = "okvfe_stereo_insert_blocks_device";
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || T->n_landmarks < 0 || (T->n_landmarks > 0 && (!T->hp_W || !initialised_dev)) || !blocks_dev ||
      block_stride_m < 0 || block_stride_c < 0 || n_multiframes < 0 || n_cams < 1 || n_cams > kStereoInsertMaxCams ||
      !pairs || n_pairs < 1 || n_pairs > OKVFE_STEREO_MAX_PAIRS || !cam_ids || !T_WC || !matches_dev || !landmark_dev ||
      !result || !result->landmark_out || !result->counts)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", kName);
  const int K = ctx->kp_cap;
  StereoInsertArgs A{};
  for (int p = 0; p < n_pairs; ++p) {
    const int c0 = pairs[2 * p], c1 = pairs[2 * p + 1];
    if (c0 < 0 || c0 >= n_cams || c1 < 0 || c1 >= n_cams || c0 == c1)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: cameras (%d, %d) of a rig of %d", kName, p, c0, c1, n_cams);
    A.pair_c0[p] = (int8_t)c0;
    A.pair_c1[p] = (int8_t)c1;
  }
  bool rt8 = false;
  okvfe_status st = rig_slots(ctx, RigWho{kName, "camera"}, n_cams, cam_ids, &rt8, [](int, const DeviceCamera&) {});
  if (st != OKVFE_OK) return st;
  if ((int64_t)T->n_landmarks + (int64_t)n_pairs * K > (int64_t)INT32_MAX)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: %d table rows + %d x %d created ids do not fit an int32", kName,
                T->n_landmarks, n_pairs, K);
  if ((st = check_block_strides(ctx, kName, block_stride_m, block_stride_c, n_multiframes, n_cams)) != OKVFE_OK) return st;
  int ov_log2 = 0, kh_log2 = 0;
  const size_t lds = stereo_insert_lds_bytes(n_cams, K, &ov_log2, &kh_log2);
  if (lds > kStereoInsertMaxLds)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: %d cameras of %d keypoints need %zu bytes of LDS per multiframe, the limit is %zu",
                kName, n_cams, K, lds, kStereoInsertMaxLds);
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(K);
  // the parameter block: the rig's camera slots (padded to 8 bytes), then one pose per (multiframe, camera); one
  // asynchronous copy through the pinned ring, no host synchronisation
  const size_t slots_bytes = ((size_t)n_cams * sizeof(int32_t) + 7) & ~(size_t)7;
  const size_t poses_bytes = (size_t)n_multiframes * (size_t)n_cams * sizeof(okvfe_pose);
  std::vector<uint8_t> block(slots_bytes + poses_bytes, 0);
  std::memcpy(block.data(), cam_ids, (size_t)n_cams * sizeof(int32_t));
  std::memcpy(block.data() + slots_bytes, T_WC, poses_bytes);
  A.hp_W = T->hp_W;
  A.initialised = initialised_dev;
  A.blocks = static_cast<const uint8_t*>(blocks_dev);
  A.cameras = ctx->d_cams;
  A.matches = matches_dev;
  A.landmark = landmark_dev;
  A.as_keyframe = as_keyframe_dev;
  A.action = result->action;
  A.lm = result->lm;
  A.landmark_out = result->landmark_out;
  A.counts = result->counts;
  A.block_bytes = L.total;
  A.n_landmarks = T->n_landmarks;
  A.n_multiframes = n_multiframes;
  A.n_cams = n_cams;
  A.n_pairs = n_pairs;
  A.kp_cap = K;
  A.w = ctx->w;
  A.h = ctx->h;
  A.o_count = (int)L.o_count;
  A.o_kps = (int)L.o_kps;
  A.stride_m = block_stride_m;
  A.stride_c = block_stride_c;
  A.ov_log2 = ov_log2;
  A.kh_log2 = kh_log2;
  return ring_launch(ctx, s, block, OKVFE_STAGE_MATCH, [&](const uint8_t* params) {
    A.cam_slots = reinterpret_cast<const int32_t*>(params);
    A.poses = reinterpret_cast<const okvfe_pose*>(params + slots_bytes);
    launch_stereo_insert(A, lds, s, rt8);
  });
}

}  // extern "C"
