// k_keyframe.hip -- keypoint coverage masks of Frontend::doWeNeedANewKeyframe (Frontend.cpp:1074-1101, :1123-1149).
//
// Per camera image the reference paints one filled disc per keypoint into a rows x cols u8 mask (`detections`), the
// same disc into a second mask (`matches`) for the keypoints that carry a landmark, and counts the non-zero pixels
// of the two masks, of their AND and of their OR.  Here ONE work-group serves one image: the two masks are bit rows
// in LDS (ceil(cols / 32) words per row), every lane paints the discs of its keypoints with LDS atomicOr -- a disc is
// 2r + 1 horizontal spans, a span one or two word masks -- and after a barrier the lanes popcount the words.  All
// discs of an image are equal (one table of half-widths per row offset, built on the host from OpenCV's midpoint
// loop and passed by value), painting is idempotent, so keypoint order and duplicates do not matter.
//
// "Carries a landmark": id != 0 or, with an id set S, id != 0 and id in S (:1138).  S may have any length, order,
// duplicates and zeros: it is streamed through an LDS hash table (open addressing, 0 = empty, 8-byte keys) in chunks
// of half the table, and a lane remembers the hits of its keypoints in one register bit per keypoint (32 keypoints
// per lane and tile, as many tiles as the image needs).
//
// overlap_pairs_kernel is ViSlamBackend::overlapFraction (ViSlamBackend.cpp:2341-2427) up to its counts, for a list of
// ordered multiframe pairs: one work-group per (pair, side) hashes the ids of ALL cameras of the other multiframe --
// the set is per multiframe, not per image -- and paints its own cameras one after another into the same two masks.
#include <hip/hip_runtime.h>

#include "okvfe_internal.h"

namespace okvfe {
namespace {

constexpr int kCovLanes = 256;
constexpr int kCovTile = 32;  // keypoints per lane and tile: one hit bit each

__device__ __forceinline__ uint32_t cov_slot(uint64_t id, int log2_slots) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots));
}

// cv::Point(keypoint.pt * 0.1): Point2f * double is float(double(v) * 0.1) per coordinate, cvRound rounds half to even.
// Centres that cannot touch the mask (and non-finite coordinates) report false.
__device__ __forceinline__ bool cov_centre(float v, int dim, int r, int* c) {
  const float f = rintf((float)((double)v * 0.1));
  if (!(f >= (float)(-r - 1) && f <= (float)(dim + r))) return false;
  *c = (int)f;
  return true;
}

__device__ __forceinline__ void cov_paint(uint32_t* mask, int words, int rows, int cols, int r, const uint8_t* hw,
                                          int cx, int cy) {
  const int y0 = max(cy - r, 0), y1 = min(cy + r, rows - 1);
  for (int y = y0; y <= y1; ++y) {
    const int h = hw[abs(y - cy)];
    const int x0 = max(cx - h, 0), x1 = min(cx + h, cols - 1);
    if (x0 > x1) continue;
    for (int w = x0 >> 5; w <= (x1 >> 5); ++w) {
      const int lo = max(x0 - 32 * w, 0), hi = min(x1 - 32 * w, 31);
      const uint32_t m = (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo);
      atomicOr(&mask[y * words + w], m);
    }
  }
}

__device__ __forceinline__ void cov_table_clear(unsigned long long* tab, int slots, int tid) {
  for (int i = tid; i < slots; i += kCovLanes) tab[i] = 0ull;
}

// the caller keeps the table at most half full: an empty slot is always found
__device__ __forceinline__ void cov_table_insert(unsigned long long* tab, int log2_slots, unsigned long long id) {
  uint32_t s = cov_slot(id, log2_slots);
  for (;;) {
    const unsigned long long old = atomicCAS(&tab[s], 0ull, id);
    if (old == 0ull || old == id) break;
    s = (s + 1) & (uint32_t)((1 << log2_slots) - 1);
  }
}

__device__ __forceinline__ bool cov_table_has(const unsigned long long* tab, int log2_slots, unsigned long long id) {
  uint32_t s = cov_slot(id, log2_slots);
  for (;;) {
    const unsigned long long v = tab[s];
    if (v == id) return true;
    if (v == 0ull) return false;
    s = (s + 1) & (uint32_t)((1 << log2_slots) - 1);
  }
}

// totals (zero on entry) += {matched, |detections|, |matches|, |AND|, |OR|} of the group; barriers on both sides
__device__ __forceinline__ void cov_count(const uint32_t* det, const uint32_t* mat, int mask_words, int matched,
                                          int32_t* totals, int tid) {
  __syncthreads();
  int acc[5] = {matched, 0, 0, 0, 0};
  for (int i = tid; i < mask_words; i += kCovLanes) {
    const uint32_t d = det[i], m = mat[i];
    acc[1] += __popc(d);
    acc[2] += __popc(m);
    acc[3] += __popc(d & m);
    acc[4] += __popc(d | m);
  }
  for (int q = 0; q < 5; ++q) {
    int v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0 && v != 0) atomicAdd(&totals[q], v);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kCovLanes) void keyframe_coverage_kernel(const CoverageArgs A, okvfe_coverage* __restrict__ out) {
  // the id table first: its 8-byte slots (64-bit LDS atomics) need the 16-byte alignment of the block, the masks do not
  extern __shared__ __align__(16) unsigned long long cov_lds[];
  __shared__ int32_t totals[5];  // matched keypoints, |detections|, |matches|, |AND|, |OR|
  __shared__ uint8_t hw[kCoverageMaxRadius + 1];  // the lanes index it by their own row offset
  const int tid = threadIdx.x, f = blockIdx.x;
  const int words = (A.cols + 31) >> 5, mask_words = A.rows * words;
  const int slots = A.has_set ? 1 << A.log2_slots : 0, chunk = slots >> 1;
  unsigned long long* tab = cov_lds;
  uint32_t* det = reinterpret_cast<uint32_t*>(cov_lds + slots);
  uint32_t* mat = det + mask_words;

  const uint8_t* frame = A.base + (size_t)f * A.frame_stride;
  const int n = min(max(*reinterpret_cast<const int32_t*>(frame + A.o_count), 0), A.kp_limit);
  const okvfe_keypoint* kps = reinterpret_cast<const okvfe_keypoint*>(frame + A.o_kps);
  const uint64_t* ids = A.ids + (size_t)f * A.id_stride;

  for (int i = tid; i < 2 * mask_words; i += kCovLanes) det[i] = 0u;
  if (tid < 5) totals[tid] = 0;
  if (tid <= kCoverageMaxRadius) hw[tid] = A.hw[tid];
  __syncthreads();

  int matched = 0;
  for (int k0 = 0; k0 < n; k0 += kCovLanes * kCovTile) {  // every bound below is the same for all lanes of the group
    uint32_t hit = 0u;
    if (!A.has_set) {
      for (int i = 0; i < kCovTile; ++i) {
        const int k = k0 + i * kCovLanes + tid;
        if (k < n && ids[k] != 0ull) hit |= 1u << i;
      }
    } else {
      for (int c0 = 0; c0 < A.n_id_set; c0 += chunk) {
        cov_table_clear(tab, slots, tid);
        __syncthreads();
        for (int i = c0 + tid; i < min(c0 + chunk, A.n_id_set); i += kCovLanes) {  // at most chunk = slots / 2 keys
          const unsigned long long id = A.id_set[i];
          if (id != 0ull) cov_table_insert(tab, A.log2_slots, id);
        }
        __syncthreads();
        for (int i = 0; i < kCovTile; ++i) {
          const int k = k0 + i * kCovLanes + tid;
          if (k >= n || ((hit >> i) & 1u)) continue;
          const unsigned long long id = ids[k];
          if (id != 0ull && cov_table_has(tab, A.log2_slots, id)) hit |= 1u << i;
        }
        __syncthreads();  // the next chunk clears the table
      }
    }
    for (int i = 0; i < kCovTile; ++i) {
      const int k = k0 + i * kCovLanes + tid;
      if (k >= n) break;
      const bool m = (hit >> i) & 1u;
      matched += m ? 1 : 0;
      int cx, cy;
      if (!cov_centre(kps[k].x, A.cols, A.r, &cx) || !cov_centre(kps[k].y, A.rows, A.r, &cy)) continue;
      cov_paint(det, words, A.rows, A.cols, A.r, hw, cx, cy);
      if (m) cov_paint(mat, words, A.rows, A.cols, A.r, hw, cx, cy);
    }
  }
  cov_count(det, mat, mask_words, matched, totals, tid);
  if (tid == 0) {
    okvfe_coverage c;
    c.n_keypoints = n;
    c.n_matched = totals[0];
    c.detections_area = totals[1];
    c.matches_area = totals[2];
    c.intersection_area = totals[3];
    c.union_area = totals[4];
    out[f] = c;
  }
}

// One work-group per (pair, side): blockIdx.x = 2 * pair + side.  A lane owns keypoint t * kCovLanes + tid of camera c
// in "slot" c * tiles + t and keeps one hit bit per slot, 64 slots per pass (Hilti, 5 x 700: 15 slots, one pass), so a
// chunk of the other multiframe's ids is hashed once per pass and not once per camera.
__global__ __launch_bounds__(kCovLanes) void overlap_pairs_kernel(const OverlapArgs A) {
  extern __shared__ __align__(16) unsigned long long cov_lds[];  // table | detections | matches | counts
  __shared__ int32_t totals[5];
  __shared__ uint8_t hw[kCoverageMaxRadius + 1];
  const int tid = threadIdx.x, pair = blockIdx.x >> 1, side = blockIdx.x & 1;
  const int words = (A.cols + 31) >> 5, mask_words = A.rows * words;
  const int slots = 1 << A.log2_slots, chunk = slots >> 1;
  unsigned long long* tab = cov_lds;
  uint32_t* det = reinterpret_cast<uint32_t*>(cov_lds + slots);
  uint32_t* mat = det + mask_words;
  int32_t* cnt = reinterpret_cast<int32_t*>(mat + mask_words);  // [0, n_cams): this side; [kOverlapMaxCams, ...): the other
  const int m_own = A.pairs[2 * pair + side], m_other = A.pairs[2 * pair + (side ^ 1)];
  auto block_of = [&](int m, int c) { return (size_t)((int64_t)m * A.stride_m + (int64_t)c * A.stride_c); };

  if (tid < 2 * A.n_cams) {
    const int other = tid >= A.n_cams ? 1 : 0, c = tid - other * A.n_cams;
    const uint8_t* block = A.blocks + block_of(other ? m_other : m_own, c) * A.block_bytes;
    cnt[other * kOverlapMaxCams + c] = min(max(*reinterpret_cast<const int32_t*>(block + A.o_count), 0), A.kp_cap);
  }
  for (int i = tid; i < 2 * mask_words; i += kCovLanes) det[i] = 0u;
  if (tid < 5) totals[tid] = 0;
  if (tid <= kCoverageMaxRadius) hw[tid] = A.hw[tid];
  __syncthreads();
  int n_other = 0;
  for (int c = 0; c < A.n_cams; ++c) n_other += cnt[kOverlapMaxCams + c];

  const int n_slots = A.n_cams * A.tiles;
  int cur = 0, matched = 0;
  int32_t sum[4] = {0, 0, 0, 0};  // lane 0: keypoints, matched, |AND|, |OR| over the cameras
  auto finish = [&](int c, bool more) {  // camera c is painted: count, report, and clear the masks for the next one
    cov_count(det, mat, mask_words, matched, totals, tid);
    if (tid == 0) {
      okvfe_coverage v;
      v.n_keypoints = cnt[c];
      v.n_matched = totals[0];
      v.detections_area = totals[1];
      v.matches_area = totals[2];
      v.intersection_area = totals[3];
      v.union_area = totals[4];
      if (A.coverage) A.coverage[(size_t)blockIdx.x * A.n_cams + c] = v;
      sum[0] += v.n_keypoints;
      sum[1] += v.n_matched;
      sum[2] += v.intersection_area;
      sum[3] += v.union_area;
    }
    if (!more) return;
    __syncthreads();
    for (int i = tid; i < 2 * mask_words; i += kCovLanes) det[i] = 0u;
    if (tid < 5) totals[tid] = 0;
    __syncthreads();
  };
  for (int s0 = 0; s0 < n_slots; s0 += 64) {  // every bound below is the same for all lanes of the group
    const int s1 = min(s0 + 64, n_slots);
    uint64_t hit = 0ull;
    for (int c0 = 0; c0 < n_other; c0 += chunk) {
      cov_table_clear(tab, slots, tid);
      __syncthreads();
      for (int j = c0 + tid; j < min(c0 + chunk, n_other); j += kCovLanes) {  // row j of the other side's counted rows
        int c = 0, k = j;
        while (k >= cnt[kOverlapMaxCams + c]) k -= cnt[kOverlapMaxCams + c++];
        const unsigned long long id = A.ids[block_of(m_other, c) * A.kp_cap + k];
        if (id != 0ull) cov_table_insert(tab, A.log2_slots, id);
      }
      __syncthreads();
      for (int s = s0; s < s1; ++s) {
        const int c = s / A.tiles, k = (s - c * A.tiles) * kCovLanes + tid;
        if (k >= cnt[c] || ((hit >> (s - s0)) & 1ull)) continue;
        const unsigned long long id = A.ids[block_of(m_own, c) * A.kp_cap + k];
        if (id != 0ull && cov_table_has(tab, A.log2_slots, id)) hit |= 1ull << (s - s0);
      }
      __syncthreads();  // the next chunk clears the table
    }
    for (int s = s0; s < s1; ++s) {
      const int c = s / A.tiles, k = (s - c * A.tiles) * kCovLanes + tid;
      if (c != cur) {
        finish(cur, true);
        cur = c;
        matched = 0;
      }
      if (k >= cnt[c]) continue;
      const bool m = (hit >> (s - s0)) & 1ull;
      matched += m ? 1 : 0;
      const okvfe_keypoint* kps =
          reinterpret_cast<const okvfe_keypoint*>(A.blocks + block_of(m_own, c) * A.block_bytes + A.o_kps);
      int cx, cy;
      if (!cov_centre(kps[k].x, A.cols, A.r, &cx) || !cov_centre(kps[k].y, A.rows, A.r, &cy)) continue;
      cov_paint(det, words, A.rows, A.cols, A.r, hw, cx, cy);
      if (m) cov_paint(mat, words, A.rows, A.cols, A.r, hw, cx, cy);
    }
  }
  finish(cur, false);
  if (tid == 0) {
    okvfe_overlap_counts* o = A.counts + pair;
    o->n_keypoints[side] = sum[0];
    o->n_matched[side] = sum[1];
    o->intersection_area[side] = sum[2];
    o->union_area[side] = sum[3];
  }
}
}  // namespace

void launch_overlap_pairs(const OverlapArgs& args, int n_pairs, size_t lds_bytes, hipStream_t stream) {
  if (n_pairs <= 0) return;
  hipLaunchKernelGGL(overlap_pairs_kernel, dim3(2u * (unsigned)n_pairs), dim3(kCovLanes), lds_bytes, stream, args);
}

void launch_keyframe_coverage(const CoverageArgs& args, int n_frames, size_t lds_bytes, okvfe_coverage* out,
                              hipStream_t stream) {
  if (n_frames <= 0) return;
  hipLaunchKernelGGL(keyframe_coverage_kernel, dim3(n_frames), dim3(kCovLanes), lds_bytes, stream, args, out);
}

}  // namespace okvfe
