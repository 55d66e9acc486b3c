// k_place.hip -- what Frontend::verifyRecognisedPlace (okvis_frontend/src/Frontend.cpp:330-355, 359, 380) does with the
// k_min / dist_min rows of okvfe_verify_place_blocks_device, for a batch of multiframes: the `matches` map, in which
// the landmark with the largest id keeps a keypoint, the counts `ctr` and points.size(), the number of correspondences
// LoopclosureNoncentralAbsoluteAdapter (LoopclosureNoncentralAbsoluteAdapter.cpp:69-154) would build, and the gate.
//   place_claims_kernel   one work-group per multiframe, one camera at a time.  The claims of a camera are a table of
//                         one int per keypoint in LDS: every hitting landmark row does atomicMax(claim[k_min], row),
//                         which leaves the largest row whatever the order; the counts are ballots + popcounts.
#include "okvfe_internal.h"

namespace okvfe {
namespace {

constexpr int kPlaceThreads = 256;
constexpr int kPlaceWaves = kPlaceThreads / 64;

struct PlaceArgs {
  const double* hp;  // L x 4
  int n_landmarks;
  const uint8_t* blocks;
  int o_count;
  size_t block_bytes;
  int kp_cap, n_cams;
  const int32_t* k_min;
  const uint32_t* dist_min;
  uint32_t threshold;
  int min_inliers;
  int32_t *n_matches, *n_points, *n_corr;
  uint8_t* gate;
  int32_t* match_landmark;
};

__device__ __forceinline__ int block_count(const PlaceArgs& A, size_t b) {
  const int count = *reinterpret_cast<const int32_t*>(A.blocks + b * A.block_bytes + A.o_count);
  return count < 0 ? 0 : (count > A.kp_cap ? A.kp_cap : count);
}

// Frontend.cpp:337-350 after the descriptor loops: landmark row l hits block b iff distMin < threshold; a k_min outside
// the block's keypoints (which the matcher cannot produce) is no hit
__device__ __forceinline__ bool place_hit(const PlaceArgs& A, size_t b, int l, int count, int& k) {
  const size_t i = b * (size_t)A.n_landmarks + (size_t)l;
  if (!(A.dist_min[i] < A.threshold)) return false;
  k = A.k_min[i];
  return k >= 0 && k < count;
}

__global__ __launch_bounds__(kPlaceThreads) void place_claims_kernel(PlaceArgs A) {
  extern __shared__ int s_claim[];  // kp_cap ints
  __shared__ int s_sum[3][kPlaceWaves];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = A.n_landmarks, K = A.kp_cap;
  const size_t frame0 = (size_t)m * (size_t)A.n_cams;
  const int l_end = (L + kPlaceThreads - 1) / kPlaceThreads * kPlaceThreads;  // whole waves reach every ballot
  int n_matches = 0, n_points = 0, n_corr = 0;  // lane 0 of every wave: the wave's share

  // points.size(): the rows with a hit in at least one camera (:349)
  for (int l = tid; l < l_end; l += kPlaceThreads) {
    bool any = false;
    if (l < L)
      for (int c = 0; c < A.n_cams && !any; ++c) {
        int k;
        any = place_hit(A, frame0 + c, l, block_count(A, frame0 + c), k);
      }
    n_points += (int)__popcll(__ballot(any));
  }

  for (int c = 0; c < A.n_cams; ++c) {
    const size_t b = frame0 + c;
    const int count = block_count(A, b);
    for (int k = tid; k < count; k += kPlaceThreads) s_claim[k] = -1;
    __syncthreads();
    // matches[(frame, im, kMin)] = lmId for the landmarks in ascending order: the largest row stays (:350)
    for (int l = tid; l < l_end; l += kPlaceThreads) {
      int k = 0;
      const bool hit = l < L && place_hit(A, b, l, count, k);
      if (hit) atomicMax(&s_claim[k], l);
      n_matches += (int)__popcll(__ballot(hit));  // ctr++ (:348): a landmark that loses its keypoint still counts
    }
    __syncthreads();
    // the adapter's walk over the keypoints of this camera (LoopclosureNoncentralAbsoluteAdapter.cpp:112-127)
    const int k_end = (count + kPlaceThreads - 1) / kPlaceThreads * kPlaceThreads;
    for (int k = tid; k < k_end; k += kPlaceThreads) {
      bool corr = false;
      if (k < count) {
        const int l = s_claim[k];
        A.match_landmark[b * (size_t)K + k] = l;
        corr = l >= 0 && !(fabs(A.hp[4 * (size_t)l + 3]) < 1.0e-8);  // :126 (a NaN stays in)
      }
      n_corr += (int)__popcll(__ballot(corr));
    }
    __syncthreads();  // the table is reused by the next camera
  }

  if (lane == 0) {
    s_sum[0][wave] = n_matches;
    s_sum[1][wave] = n_points;
    s_sum[2][wave] = n_corr;
  }
  __syncthreads();
  if (tid == 0) {
    int ctr = 0, points = 0, corr = 0;
    for (int w = 0; w < kPlaceWaves; ++w) {
      ctr += s_sum[0][w];
      points += s_sum[1][w];
      corr += s_sum[2][w];
    }
    A.n_matches[m] = ctr;
    A.n_points[m] = points;
    A.n_corr[m] = corr;
    // Frontend.cpp:359 (eight points) before :380 (seven correspondences)
    A.gate[m] = (uint8_t)(ctr < A.min_inliers || points < 8 ? 0 : corr < 7 ? 1 : 2);
  }
}

}  // namespace

void launch_place_claims(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks, int n_multiframes,
                         int n_cams, int kp_cap, const int32_t* k_min, const uint32_t* dist_min, uint32_t threshold,
                         int min_inliers, const okvfe_place_claims_device& out, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  PlaceArgs A;
  A.hp = hp; A.n_landmarks = n_landmarks; A.blocks = blocks; A.o_count = (int)L.o_count; A.block_bytes = L.total;
  A.kp_cap = kp_cap; A.n_cams = n_cams; A.k_min = k_min; A.dist_min = dist_min; A.threshold = threshold;
  A.min_inliers = min_inliers;
  A.n_matches = out.n_matches; A.n_points = out.n_points; A.n_corr = out.n_correspondences; A.gate = out.gate;
  A.match_landmark = out.match_landmark;
  hipLaunchKernelGGL(place_claims_kernel, dim3(n_multiframes), dim3(kPlaceThreads), (size_t)kp_cap * sizeof(int), stream,
                     A);
}

}  // namespace okvfe
