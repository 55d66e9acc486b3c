// capi_ransac2d2d.cpp -- Frontend::runRansac2d2d (Frontend.cpp:2281-2394) behind the C ABI, hypotheses and consensus: what
// the motion-stereo sweep runs after every older frame while the session is not initialised, on device-resident batches.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {

// The parameter block of both 2d2d calls: fu per camera, then {mf0, mf1} per pair; the camera slots and the pairs'
// multiframe indices are checked on the way.  once: a current multiframe may be named by one pair only.
okvfe_status pair_params(okvfe_ctx* ctx, const char* fn, int32_t n_multiframes0, int32_t n_multiframes1, int32_t n_pairs,
                         const int32_t* mf0, const int32_t* mf1, int32_t n_cams, const int32_t* cam_ids, bool once,
                         std::vector<uint8_t>& prm) {
  prm.assign((size_t)n_cams * sizeof(double) + (size_t)n_pairs * 2 * sizeof(int32_t), 0);
  const okvfe_status st = rig_slots(ctx, RigWho{fn, "frame"}, n_cams, cam_ids, nullptr, [&](int c, const DeviceCamera& dc) {
    std::memcpy(prm.data() + (size_t)c * sizeof(double), &dc.fu, sizeof(double));
  });
  if (st != OKVFE_OK) return st;
  int32_t* pr = reinterpret_cast<int32_t*>(prm.data() + (size_t)n_cams * sizeof(double));
  std::vector<int> user(once ? (size_t)n_multiframes1 : 0, -1);
  for (int p = 0; p < n_pairs; ++p) {
    if (mf0[p] < 0 || mf0[p] >= n_multiframes0 || mf1[p] < 0 || mf1[p] >= n_multiframes1)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: multiframes (%d, %d) outside [0, %d) x [0, %d)", fn, p,
                  mf0[p], mf1[p], n_multiframes0, n_multiframes1);
    if (once) {
      if (user[(size_t)mf1[p]] >= 0)
        return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT,
                    "%s: current multiframe %d is named by pairs %d and %d: with landmark1_out a call resolves a current "
                    "multiframe once", fn, mf1[p], user[(size_t)mf1[p]], p);
      user[(size_t)mf1[p]] = p;
    }
    pr[2 * p] = mf0[p];
    pr[2 * p + 1] = mf1[p];
  }
  return OKVFE_OK;
}

// what both kernels read of a call: the blocks and their layout, the id rows, the isLandmarkAdded bytes
Ransac2d2dArgs block_args(okvfe_ctx* ctx, const void* blocks0_dev, const void* blocks1_dev, int32_t n_cams,
                          const int32_t* landmark0_dev, const int32_t* landmark1_dev, const uint8_t* added_dev,
                          int32_t n_landmarks, int32_t n_hyp) {
  const BlockLayout L = block_layout(ctx->kp_cap);
  Ransac2d2dArgs A{};
  A.blocks0 = static_cast<const uint8_t*>(blocks0_dev);
  A.blocks1 = static_cast<const uint8_t*>(blocks1_dev);
  A.o_count = (int)L.o_count; A.o_kps = (int)L.o_kps; A.o_bp = (int)L.o_bp; A.o_bpv = (int)L.o_bpv;
  A.block_bytes = L.total; A.kp_cap = ctx->kp_cap; A.n_cams = n_cams;
  A.landmark0 = landmark0_dev; A.landmark1 = landmark1_dev; A.added = added_dev; A.n_landmarks = n_landmarks;
  A.n_hyp = n_hyp;
  return A;
}

}  // namespace

extern "C" {

okvfe_status okvfe_ransac2d2d_consensus_blocks_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_multiframes0, const void* blocks1_dev, int32_t n_multiframes1,
    int32_t n_pairs, const int32_t* mf0, const int32_t* mf1, int32_t n_cams, const int32_t* cam_ids,
    const int32_t* landmark0_dev, const int32_t* landmark1_dev, const uint8_t* added_dev, int32_t n_landmarks,
    const double* rot_hyp_dev, const uint8_t* rot_valid_dev, const double* rel_hyp_dev, const uint8_t* rel_valid_dev,
    int32_t n_hyp, double threshold, int32_t remove_outliers, const okvfe_ransac2d2d_result_device* result, void* stream) {
  const char* fn = "okvfe_ransac2d2d_consensus_blocks_device";
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!blocks0_dev || !blocks1_dev || n_multiframes0 < 0 || n_multiframes1 < 0 || n_pairs < 0 ||
      (n_pairs > 0 && (!mf0 || !mf1)) || n_cams < 1 || n_cams > (int)ctx->h_cams.size() || !cam_ids || !landmark0_dev ||
      !landmark1_dev || n_landmarks < 0 || !rot_hyp_dev || !rel_hyp_dev || n_hyp < 1 ||
      n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !(threshold >= 0.0) || !result || !result->n_correspondences ||
      !result->rot_best || !result->rot_inliers || !result->rel_best || !result->rel_inliers || !result->branch ||
      !result->removed || !result->total_inliers || !result->rotation_only || !result->success)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", fn);
  if (ctx->kp_cap > kRansac2dMaxKeypoints)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: max_keypoints %d exceeds %d (the id map of a block: 4096 slots of LDS)", fn,
                ctx->kp_cap, kRansac2dMaxKeypoints);
  std::vector<uint8_t> prm;
  const okvfe_status st = pair_params(ctx, fn, n_multiframes0, n_multiframes1, n_pairs, mf0, mf1, n_cams, cam_ids,
                                      result->landmark1_out != nullptr, prm);
  if (st != OKVFE_OK) return st;
  if (n_pairs == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  Ransac2d2dArgs A = block_args(ctx, blocks0_dev, blocks1_dev, n_cams, landmark0_dev, landmark1_dev, added_dev, n_landmarks,
                                n_hyp);
  A.rot_hyp = rot_hyp_dev; A.rot_valid = rot_valid_dev; A.rel_hyp = rel_hyp_dev; A.rel_valid = rel_valid_dev;
  A.threshold = threshold; A.remove_outliers = remove_outliers ? 1 : 0;
  A.out = *result;
  return ring_launch(ctx, s, prm, OKVFE_STAGE_MAP, [&](const uint8_t* prm_dev) {  // one asynchronous copy, no host sync
    A.fu = reinterpret_cast<const double*>(prm_dev);
    A.pairs = reinterpret_cast<const int32_t*>(prm_dev + (size_t)n_cams * sizeof(double));
    launch_ransac2d2d_consensus(A, n_pairs, s);
  });
}

// The hypotheses of the call above: sampler, two-point rotation and five-point relative pose on the device
// (k_ransac2d2d_hyp.hip).
okvfe_status okvfe_ransac2d2d_hypotheses_blocks_device(
    okvfe_ctx* ctx, const void* blocks0_dev, int32_t n_multiframes0, const void* blocks1_dev, int32_t n_multiframes1,
    int32_t n_pairs, const int32_t* mf0, const int32_t* mf1, int32_t n_cams, const int32_t* cam_ids,
    const int32_t* landmark0_dev, const int32_t* landmark1_dev, const uint8_t* added_dev, int32_t n_landmarks,
    const uint64_t* sample_keys_dev, uint64_t seed, int32_t n_hyp, const okvfe_ransac2d2d_hypotheses_device* result,
    void* stream) {
  const char* fn = "okvfe_ransac2d2d_hypotheses_blocks_device";
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!blocks0_dev || !blocks1_dev || n_multiframes0 < 0 || n_multiframes1 < 0 || n_pairs < 0 ||
      (n_pairs > 0 && (!mf0 || !mf1)) || n_cams < 1 || n_cams > (int)ctx->h_cams.size() || n_cams > 64 || !cam_ids ||
      !landmark0_dev || !landmark1_dev || n_landmarks < 0 || n_hyp < 1 || n_hyp > OKVFE_RANSAC_MAX_HYPOTHESES || !result ||
      !result->rot_hyp || !result->rot_valid || !result->rel_hyp || !result->rel_valid)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", fn);
  if (ctx->kp_cap > kRansac2dMaxKeypoints)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: max_keypoints %d exceeds %d (the id map of a block: 4096 slots of LDS)", fn,
                ctx->kp_cap, kRansac2dMaxKeypoints);
  std::vector<uint8_t> prm;
  const okvfe_status st = pair_params(ctx, fn, n_multiframes0, n_multiframes1, n_pairs, mf0, mf1, n_cams, cam_ids, false, prm);
  if (st != OKVFE_OK) return st;
  if (n_pairs == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  Ransac2d2dArgs A = block_args(ctx, blocks0_dev, blocks1_dev, n_cams, landmark0_dev, landmark1_dev, added_dev, n_landmarks,
                                n_hyp);
  return ring_launch(ctx, s, prm, OKVFE_STAGE_MAP, [&](const uint8_t* prm_dev) {  // one asynchronous copy, no host sync
    A.fu = reinterpret_cast<const double*>(prm_dev);
    A.pairs = reinterpret_cast<const int32_t*>(prm_dev + (size_t)n_cams * sizeof(double));
    launch_ransac2d2d_hypotheses(A, sample_keys_dev, seed, *result, n_pairs, s);
  });
}

okvfe_status okvfe_twopt_rotation_hypothesis(const double* b1, const double* b2, double* M, uint8_t* valid) {
  if (!b1 || !b2 || !M || !valid) return OKVFE_ERR_INVALID_ARGUMENT;
  *valid = twopt_rotation_host(b1, b2, M) ? 1 : 0;
  return OKVFE_OK;
}

okvfe_status okvfe_fivept_hypothesis(const double* b1, const double* b2, const double* sigma1, const double* sigma2,
                                     int32_t order, double* hypothesis, uint8_t* valid, int32_t* n_roots) {
  if (!b1 || !b2 || !sigma1 || !sigma2 || !hypothesis || !valid ||
      (order != OKVFE_SUM3_LEFT_TO_RIGHT && order != OKVFE_SUM3_EIGEN_TREE))
    return OKVFE_ERR_INVALID_ARGUMENT;
  int n = 0;
  *valid = fivept_hypothesis_host(order == OKVFE_SUM3_EIGEN_TREE, b1, b2, sigma1, sigma2, hypothesis, &n) ? 1 : 0;
  if (n_roots) *n_roots = n;
  return OKVFE_OK;
}

// Test hook, deliberately not in include/okvfe.h: the number of correspondences the 2d2d consensus kernel scores at a
// time, so that the tests straddle it whatever it is.
int32_t okvfe_test_ransac2d2d_chunk_records(void) { return ransac2d2d_chunk_records(); }
// Test hooks of the same kind: the records of the kernel's LDS ring, and the home slot of a landmark id in its id
// table (the kernel's own function), so that the tests wrap the one and crowd the other whatever their constants are.
int32_t okvfe_test_ransac2d2d_ring_records(void) { return ransac2d2d_ring_records(); }
int32_t okvfe_test_ransac2d2d_id_slot(int32_t id) { return (int32_t)ransac2d2d_id_slot(id); }

}  // extern "C"
