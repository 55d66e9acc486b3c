// capi_overlap.cpp -- ViSlamBackend::overlapFraction (ViSlamBackend.cpp:2341-2427) for a list of multiframe pairs on
// device-resident batches (k_keyframe.hip, overlap_pairs_kernel), and as host arithmetic what follows from its counts:
// the overlap itself, the order of the motion-stereo sweep (Frontend.cpp:1751-1767) and ViSlamBackend::trackingQuality
// (ViSlamBackend.cpp:157-196).
#include <climits>

#include "okvfe_ctx.h"

using namespace okvfe;

extern "C" {

okvfe_status okvfe_overlap_pairs_blocks_device(okvfe_ctx* ctx, const void* blocks_dev, int32_t block_stride_m,
                                               int32_t block_stride_c, int32_t n_multiframes, int32_t n_cams,
                                               const uint64_t* landmark_ids_dev, const int32_t* pair_a,
                                               const int32_t* pair_b, int32_t n_pairs, double kptrad,
                                               okvfe_overlap_counts* counts_dev, okvfe_coverage* coverage_dev,
                                               void* stream) {
  static const char* kName = "okvfe_overlap_pairs_blocks_device";
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!blocks_dev || block_stride_m < 0 || block_stride_c < 0 || n_multiframes < 0 || n_cams < 1 ||
      n_cams > kOverlapMaxCams || !landmark_ids_dev || n_pairs < 0 || n_pairs >= (1 << 30) ||  // two work-groups per pair
      (n_pairs > 0 && (!pair_a || !pair_b || !counts_dev)) || !std::isfinite(kptrad) || kptrad < 0.0)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", kName);
  okvfe_status st = check_block_strides(ctx, kName, block_stride_m, block_stride_c, n_multiframes, n_cams);
  if (st != OKVFE_OK) return st;
  std::vector<int32_t> pairs((size_t)2 * (size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    if (pair_a[p] < 0 || pair_a[p] >= n_multiframes || pair_b[p] < 0 || pair_b[p] >= n_multiframes)
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: pair %d: multiframes (%d, %d) of %d", kName, p, pair_a[p],
                  pair_b[p], n_multiframes);
    pairs[2 * (size_t)p] = pair_a[p];
    pairs[2 * (size_t)p + 1] = pair_b[p];
  }
  const int K = ctx->kp_cap;
  CoverageGeometry g;
  st = coverage_geometry(ctx, kName, kptrad, (int64_t)n_cams * K, kOverlapCountsLds, &g);
  if (st != OKVFE_OK) return st;
  if (n_pairs == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  RingSlot params(ctx, &ctx->pair_ring, s);  // 8 bytes per pair, one asynchronous copy, no host synchronisation
  st = params.upload(pairs.data(), pairs.size() * sizeof(int32_t));
  if (st != OKVFE_OK) return st;
  const BlockLayout L = block_layout(K);
  OverlapArgs A{};
  A.blocks = static_cast<const uint8_t*>(blocks_dev);
  A.block_bytes = L.total;
  A.o_count = (int)L.o_count;
  A.o_kps = (int)L.o_kps;
  A.kp_cap = K;
  A.ids = landmark_ids_dev;
  A.pairs = params.as<int32_t>();
  A.stride_m = block_stride_m;
  A.stride_c = block_stride_c;
  A.n_cams = n_cams;
  A.tiles = (K + 255) / 256;
  A.log2_slots = g.log2_slots;
  A.rows = g.rows;
  A.cols = g.cols;
  A.r = g.r;
  A.counts = counts_dev;
  A.coverage = coverage_dev;
  std::memcpy(A.hw, g.hw, sizeof(A.hw));
  launch_overlap_pairs(A, n_pairs, g.lds, s);
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = params.release();
  ctx->last_stream = s;
  return rel;
}

okvfe_status okvfe_overlap_fraction(const okvfe_overlap_counts* counts, int32_t n_pairs, double* overlap_out) {
  if (n_pairs < 0 || (n_pairs > 0 && (!counts || !overlap_out))) return OKVFE_ERR_INVALID_ARGUMENT;
  for (int p = 0; p < n_pairs; ++p) {
    const okvfe_overlap_counts& c = counts[p];
    for (int f = 0; f < 2; ++f)
      if (c.n_keypoints[f] < 0 || c.n_matched[f] < 0 || c.intersection_area[f] < 0 || c.union_area[f] < 0)
        return OKVFE_ERR_INVALID_ARGUMENT;
    if ((c.n_matched[0] == 0) != (c.n_matched[1] == 0)) return OKVFE_ERR_INVALID_ARGUMENT;  // a common id sits on both sides
  }
  for (int p = 0; p < n_pairs; ++p) {
    const okvfe_overlap_counts& c = counts[p];
    if (c.n_matched[0] == 0) {  // ViSlamBackend.cpp:2386-2389: without matches there will be no overlap
      overlap_out[p] = 0.0;
      continue;
    }
    double overlap[2];
    for (int f = 0; f < 2; ++f) overlap[f] = double(c.intersection_area[f]) / double(c.union_area[f]);  // :2423
    overlap_out[p] = std::min(overlap[0], overlap[1]);                                                  // :2426
  }
  return OKVFE_OK;
}

okvfe_status okvfe_motion_frame_order(const double* overlap, const uint64_t* frame_ids, int32_t n, int32_t previous,
                                      int32_t* order_out, int32_t* n_order) {
  if (!n_order) return OKVFE_ERR_INVALID_ARGUMENT;
  *n_order = -1;
  if (n < 0 || previous < -1 || previous >= n || (n > 0 && (!overlap || !frame_ids || !order_out)))
    return OKVFE_ERR_INVALID_ARGUMENT;
  struct Entry {
    std::pair<double, uint64_t> key;  // Frontend.cpp:1751
    int32_t index;
  };
  std::vector<Entry> overlaps((size_t)n);
  for (int i = 0; i < n; ++i) {
    overlaps[i] = {{i == previous ? 1.0 : overlap[i], frame_ids[i]}, i};  // :1753-1759
    if (std::isnan(overlaps[i].key.first)) {
      *n_order = i;
      return OKVFE_ERR_INVALID_ARGUMENT;
    }
  }
  {
    std::vector<uint64_t> ids(frame_ids, frame_ids + n);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return OKVFE_ERR_INVALID_ARGUMENT;
  }
  std::sort(overlaps.begin(), overlaps.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });  // :1761
  int32_t m = 0;
  for (size_t i = 0; i < overlaps.size(); ++i) {  // :1764-1767
    if (overlaps[overlaps.size() - i - 1].key.first <= 1.0e-8) break;
    order_out[m++] = overlaps[overlaps.size() - i - 1].index;
  }
  *n_order = m;
  return OKVFE_OK;
}

okvfe_status okvfe_tracking_quality(const okvfe_coverage* coverage, int32_t n_cams, int32_t width, int32_t height,
                                    double kptrad, double* quality_out) {
  if (!coverage || n_cams < 1 || width < 1 || height < 1 || !std::isfinite(kptrad) || kptrad < 0.0 || !quality_out)
    return OKVFE_ERR_INVALID_ARGUMENT;
  const int rows = height / 10;  // ViSlamBackend.cpp:169-171
  const int cols = width / 10;
  const double radius = double(std::min(rows, cols)) * kptrad;
  if ((int64_t)rows * cols > (int64_t)INT_MAX || !(radius * radius * M_PI < (double)INT_MAX))
    return OKVFE_ERR_INVALID_ARGUMENT;
  const int pointArea = int(radius * radius * M_PI);  // :191: one point per image does not count
  int64_t intersectionCount = 0, unionCount = 0, matchedPoints = 0;
  for (int im = 0; im < n_cams; ++im) {
    if (coverage[im].n_matched < 0 || coverage[im].matches_area < 0) return OKVFE_ERR_INVALID_ARGUMENT;
    matchedPoints += coverage[im].n_matched;
    intersectionCount += std::max(0, coverage[im].matches_area - pointArea);  // :192
    unionCount += rows * cols - pointArea;                                     // :193
  }
  if (intersectionCount > INT_MAX || unionCount > INT_MAX || unionCount < INT_MIN || matchedPoints > INT_MAX)
    return OKVFE_ERR_INVALID_ARGUMENT;  // the reference's ints would overflow
  *quality_out = matchedPoints < 8 ? 0.0 : double(intersectionCount) / double(unionCount);  // :195
  return OKVFE_OK;
}

}  // extern "C"
