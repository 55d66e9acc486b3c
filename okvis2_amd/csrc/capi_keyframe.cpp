// capi_keyframe.cpp -- Frontend::doWeNeedANewKeyframe behind the C ABI (Frontend.cpp:1058-1167): the keypoint coverage
// masks of a batch of frames on the device (k_keyframe.hip), their B = 1 host seam, and the decision as host arithmetic.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace okvfe {
// cv::circle(img, c, r, colour, cv::FILLED, cv::LINE_8, 0) takes OpenCV's integer midpoint routine (imgproc/src/
// drawing.cpp, Circle()): while dx >= dy the rows cy +- dy receive the span [cx - dx, cx + dx] and the rows cy +- dx the
// span [cx - dy, cx + dy].  A row offset can be visited more than once; the widest span is what ends up painted.
// Restated from the published source: OpenCV is not part of the reference tree (parity unpinned).
void circle_half_widths(int r, uint8_t* hw) {
  for (int j = 0; j <= r; ++j) hw[j] = 0;
  int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
  while (dx >= dy) {
    hw[dy] = (uint8_t)std::max<int>(hw[dy], dx);
    hw[dx] = (uint8_t)std::max<int>(hw[dx], dy);
    ++dy;
    err += plus;
    plus += 2;
    if (err > 0) {
      err -= minus;
      --dx;
      minus -= 2;
    }
  }
}
okvfe_status coverage_geometry(okvfe_ctx* ctx, const char* who, double kptrad, int64_t n_ids, size_t extra_lds,
                               CoverageGeometry* g) {
  g->rows = ctx->h / 10;  // Frontend.cpp:1075-1076
  g->cols = ctx->w / 10;
  const double radius = double(std::min(g->rows, g->cols)) * kptrad;  // :1083
  if (!(radius <= (double)kCoverageMaxRadius))
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: disc radius %g exceeds %d mask pixels", who, radius, kCoverageMaxRadius);
  g->r = int(radius);
  circle_half_widths(g->r, g->hw);
  const size_t mask_bytes = (size_t)2 * g->rows * ((g->cols + 31) / 32) * sizeof(uint32_t) + extra_lds;
  g->log2_slots = 0;
  if (n_ids >= 0) {  // table of twice the set, 256 .. 4096 slots, smaller where the masks leave less room
    g->log2_slots = 8;
    while (g->log2_slots < 12 && ((int64_t)1 << g->log2_slots) < 2 * n_ids) ++g->log2_slots;
    while (g->log2_slots > 8 && mask_bytes + ((size_t)8 << g->log2_slots) > kCoverageLdsBudget) --g->log2_slots;
  }
  g->lds = mask_bytes + (n_ids >= 0 ? (size_t)8 << g->log2_slots : 0);
  if (g->lds > kCoverageLdsBudget)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: two %d x %d bit masks need %zu bytes of LDS (limit %zu)", who, g->rows,
                g->cols, g->lds, kCoverageLdsBudget);
  return OKVFE_OK;
}
}  // namespace okvfe

namespace {
// geometry, LDS budget and launch, shared by the device entry point and the host seam
okvfe_status coverage_launch(okvfe_ctx* ctx, const char* who, CoverageArgs A, int n_frames, double kptrad,
                             okvfe_coverage* out_dev, hipStream_t s) {
  CoverageGeometry g;
  const okvfe_status st = coverage_geometry(ctx, who, kptrad, A.has_set ? (int64_t)A.n_id_set : -1, 0, &g);
  if (st != OKVFE_OK) return st;
  A.rows = g.rows;
  A.cols = g.cols;
  A.r = g.r;
  std::memcpy(A.hw, g.hw, sizeof(A.hw));
  A.log2_slots = g.log2_slots;
  launch_keyframe_coverage(A, n_frames, g.lds, out_dev, s);
  HIP_TRY(ctx, hipGetLastError());
  return OKVFE_OK;
}
}  // namespace

extern "C" {

okvfe_status okvfe_keyframe_coverage_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t n_frames,
                                                   const uint64_t* landmark_ids_dev, const uint64_t* id_set_dev,
                                                   int32_t n_id_set, double kptrad, okvfe_coverage* coverage_dev,
                                                   void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!blocks_dev || n_frames < 1 || !landmark_ids_dev || !coverage_dev || n_id_set < 0 ||
      (!id_set_dev && n_id_set > 0) || !std::isfinite(kptrad) || kptrad < 0.0)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_keyframe_coverage_blocks_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  CoverageArgs A{};
  A.base = static_cast<const uint8_t*>(blocks_dev);
  A.frame_stride = L.total;
  A.o_count = (int)L.o_count;
  A.o_kps = (int)L.o_kps;
  A.kp_limit = ctx->kp_cap;
  A.ids = landmark_ids_dev;
  A.id_stride = (size_t)ctx->kp_cap;
  A.id_set = id_set_dev;
  A.n_id_set = n_id_set;
  A.has_set = id_set_dev ? 1 : 0;
  okvfe_status st = coverage_launch(ctx, "okvfe_keyframe_coverage_blocks_device", A, n_frames, kptrad, coverage_dev, s);
  if (st != OKVFE_OK) return st;
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_keyframe_coverage(okvfe_ctx* ctx, const okvfe_keypoint* keypoints, int32_t n,
                                     const uint64_t* landmark_ids, const uint64_t* id_set, int32_t n_id_set,
                                     double kptrad, okvfe_coverage* out) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n < 0 || (n > 0 && (!keypoints || !landmark_ids)) || !out || n_id_set < 0 || (!id_set && n_id_set > 0) ||
      !std::isfinite(kptrad) || kptrad < 0.0)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_keyframe_coverage: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, nullptr);  // the context's own stream, behind pending pipelined lanes
  ScratchLayout lay;
  const size_t o_n = lay.take(4), o_k = lay.take((size_t)n * sizeof(okvfe_keypoint)), o_id = lay.take((size_t)n * 8),
               o_set = lay.take((size_t)n_id_set * 8), o_out = lay.take(sizeof(okvfe_coverage));
  ScratchCall call(ctx, s);
  okvfe_status st = call.reserve(lay);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.up(o_n, &n, 4));
  HIP_TRY(ctx, call.up(o_k, keypoints, (size_t)n * sizeof(okvfe_keypoint)));
  HIP_TRY(ctx, call.up(o_id, landmark_ids, (size_t)n * 8));
  HIP_TRY(ctx, call.up(o_set, id_set, (size_t)n_id_set * 8));
  HIP_TRY(ctx, call.sync());  // pageable sources
  CoverageArgs A{};
  A.base = call.dev(0);
  A.frame_stride = 0;
  A.o_count = (int)o_n;
  A.o_kps = (int)o_k;
  A.kp_limit = n;
  A.ids = call.dev<const uint64_t>(o_id);
  A.id_stride = 0;
  A.id_set = call.dev<const uint64_t>(o_set);
  A.n_id_set = n_id_set;
  A.has_set = id_set ? 1 : 0;
  st = coverage_launch(ctx, "okvfe_keyframe_coverage", A, 1, kptrad, call.dev<okvfe_coverage>(o_out), s);
  if (st != OKVFE_OK) return st;
  HIP_TRY(ctx, call.down(out, o_out, sizeof(okvfe_coverage)));
  HIP_TRY(ctx, call.sync());
  return OKVFE_OK;
}

okvfe_status okvfe_keyframe_decision(const okvfe_coverage* current, int32_t n_cameras, const okvfe_coverage* others,
                                     int32_t n_others, float overlap_threshold, int32_t* need_keyframe,
                                     double* overlap_out) {
  if (!current || n_cameras < 1 || n_others < 0 || (n_others > 0 && !others) || !need_keyframe)
    return OKVFE_ERR_INVALID_ARGUMENT;
  for (size_t i = 0; i < (size_t)n_cameras * (size_t)(1 + n_others); ++i) {  // counts are counts
    const okvfe_coverage& c = i < (size_t)n_cameras ? current[i] : others[i - (size_t)n_cameras];
    if (c.n_keypoints < 0 || c.intersection_area < 0 || c.union_area < 0) return OKVFE_ERR_INVALID_ARGUMENT;
  }
  // Frontend.cpp:1067-1103: the current multiframe, counts summed over its cameras
  int intersectionCount = 0, unionCount = 0;
  size_t numKeypoints = 0;
  for (int im = 0; im < n_cameras; ++im) {
    numKeypoints += (size_t)current[im].n_keypoints;
    intersectionCount += current[im].intersection_area;
    unionCount += current[im].union_area;
  }
  double overlap = double(intersectionCount) / double(unionCount);
  // :1116-1152: the best overlap with any other multiframe.  0 / 0 is NaN; std::max(a, NaN) keeps a
  double overlapOthers = 0.0;
  for (int f = 0; f < n_others; ++f) {
    int intersectionOther = 0, unionOther = 0;
    for (int im = 0; im < n_cameras; ++im) {
      intersectionOther += others[(size_t)f * n_cameras + im].intersection_area;
      unionOther += others[(size_t)f * n_cameras + im].union_area;
    }
    overlapOthers = std::max(overlapOthers, double(intersectionOther) / double(unionOther));
  }
  overlap = std::min(overlapOthers, overlap);  // :1154, this argument order: a NaN `overlap` yields overlapOthers
  if (overlap_out) *overlap_out = overlap;
  if (numKeypoints < (size_t)7 * (size_t)n_cameras)  // :1157: a respectable keyframe needs some detections
    *need_keyframe = 0;
  else
    *need_keyframe = float(overlap) > overlap_threshold ? 0 : 1;  // :1161-1166
  return OKVFE_OK;
}

}  // extern "C"
