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
        for (int i = tid; i < slots; i += kCovLanes) tab[i] = 0ull;
        __syncthreads();
        for (int i = c0 + tid; i < min(c0 + chunk, A.n_id_set); i += kCovLanes) {
          const unsigned long long id = A.id_set[i];
          if (id == 0ull) continue;
          uint32_t s = cov_slot(id, A.log2_slots);
          for (;;) {  // at most chunk = slots / 2 keys: an empty slot is always found
            const unsigned long long old = atomicCAS(&tab[s], 0ull, id);
            if (old == 0ull || old == id) break;
            s = (s + 1) & (uint32_t)(slots - 1);
          }
        }
        __syncthreads();
        for (int i = 0; i < kCovTile; ++i) {
          const int k = k0 + i * kCovLanes + tid;
          if (k >= n || ((hit >> i) & 1u)) continue;
          const unsigned long long id = ids[k];
          if (id == 0ull) continue;
          uint32_t s = cov_slot(id, A.log2_slots);
          for (;;) {
            const unsigned long long v = tab[s];
            if (v == id) hit |= 1u << i;
            if (v == id || v == 0ull) break;
            s = (s + 1) & (uint32_t)(slots - 1);
          }
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
}  // namespace

void launch_keyframe_coverage(const CoverageArgs& args, int n_frames, size_t lds_bytes, okvfe_coverage* out,
                              hipStream_t stream) {
  if (n_frames <= 0) return;
  hipLaunchKernelGGL(keyframe_coverage_kernel, dim3(n_frames), dim3(kCovLanes), lds_bytes, stream, args, out);
}

}  // namespace okvfe
