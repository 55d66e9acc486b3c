// k_place_hessian.hip -- the second output of Frontend::verifyRecognisedPlace (okvis_frontend/src/Frontend.cpp:529-551)
// for a batch of multiframes: per inlier of the consensus one ReprojectionError::EvaluateWithMinimalJacobians with
// jacobians[0] only (okvis_ceres/include/okvis/ceres/implementation/ReprojectionError.hpp:99-183) at the caller's pose
// T_Sold_Snew, and H += J0_minimal^T J0_minimal in the order of LoopclosureNoncentralAbsoluteAdapter (camera-major,
// keypoints ascending).  The residuals and minimal Jacobians are also what the caller's ceres problem (:399-527) asks
// for at every iterate.
//   place_hessian_kernel   one work-group per multiframe, cameras one after another.  The term rows of a camera are
//                          compacted into an LDS ring and evaluated kHessChunk at a time, a lane per term; the twelve
//                          entries of J0_minimal are staged in LDS and lane e < 36 adds entry e of J^T J term after term.
//                          That order is the contract: there is no tree over the terms.
// FP64, 3- and 4-term sums in the order of okvfe_set_fp64_reduction (a template argument), no FMA.  The matrix products
// are full: the zeros of T_CS, J, Jh and the square-root information are multiplied and added, so that a non-finite
// operand spreads as it does in Eigen.
// PARITY UNPINNED: Eigen's Quaternion::normalize() and toRotationMatrix() (Eigen is not in the tree), restated from the
// published source (Eigen/src/Geometry/Quaternion.h, Eigen/src/Core/Dot.h).
// The term itself (quaternion_rotation, inverse_transform, hessian_term) is place_term_dev.h, its sums fp64_ops.h.
#include "place_term_dev.h"

namespace okvfe {
namespace {

constexpr int kHessThreads = 256;
constexpr int kHessChunk = kHessThreads;   // terms evaluated at a time: one per lane
constexpr int kHessRing = 2 * kHessChunk;  // a tile of keypoints adds at most a chunk to less than a chunk
constexpr int kHessWaves = kHessThreads / 64;
static_assert((kHessRing & (kHessRing - 1)) == 0, "ring positions are masked");

template <bool kTree, bool kRT8>
__global__ __launch_bounds__(kHessThreads) void place_hessian_kernel(PlaceHessianArgs A) {
  // 24 KiB, entry-major: a lane's twelve stores fall on its own bank pair, and the odd row pitch keeps the six rows the
  // summing lanes read at one term on different banks
  __shared__ double s_J[12][kHessChunk + 1];
  __shared__ int s_ring[kHessRing];       // keypoint rows of the camera in hand
  __shared__ double s_Tsw[16], s_Tcs[16], s_t[3];
  __shared__ int s_wave[kHessWaves];
  __shared__ int s_singular;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.kp_cap;
  const size_t frame0 = (size_t)m * (size_t)A.n_cams;

  // not verified: the reference has returned false before H exists
  if (A.verdict && A.verdict[m] != 3) {
    if (tid < 36) A.H[36 * (size_t)m + tid] = 0.0;
    if (tid == 0) {
      A.n_terms[m] = 0;
      A.n_singular[m] = 0;
    }
    return;
  }
  if (tid == 0) {
    const double* pose = A.poses + 7 * (size_t)m;
    inverse_transform<kTree>(pose, s_Tsw);  // :120-124
    s_t[0] = pose[0]; s_t[1] = pose[1]; s_t[2] = pose[2];
    s_singular = 0;
  }
  const int hi = tid / 6, hj = tid - 6 * hi;  // tid < 36: entry (hi, hj) of H
  double acc = 0.0;

  // evaluates the terms [tail, tail + n) of the ring, n <= kHessChunk, and adds them to H in that order
  auto evaluate = [&](int c, int tail, int n) {
    bool bad = false;
    if (tid < n) {
      const int k = s_ring[(tail + tid) & (kHessRing - 1)];
      const size_t row = (frame0 + c) * (size_t)K + (size_t)k;
      const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
      const okvfe_keypoint kp = reinterpret_cast<const okvfe_keypoint*>(blk + A.o_kps)[k];
      const double* hp = A.hp + 4 * (size_t)A.match_landmark[row];
      const double hp_W[4] = {hp[0], hp[1], hp[2], hp[3]};
      double r[2], J[12];
      bad = hessian_term<kTree, kRT8>(A.dcams[A.cams[c].cam], A.w, A.h, s_Tsw, s_t, s_Tcs, hp_W, kp, r, J);
      if (A.residual) {
        A.residual[2 * row] = r[0];
        A.residual[2 * row + 1] = r[1];
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) {
        s_J[e][tid] = J[e];
        if (A.jacobian) A.jacobian[12 * row + e] = J[e];
      }
    }
    const unsigned long long bal = __ballot(bad);
    if (lane == 0 && bal) atomicAdd(&s_singular, (int)__popcll(bal));
    __syncthreads();
    if (tid < 36)
      for (int t = 0; t < n; ++t) acc = acc + (s_J[hi][t] * s_J[hj][t] + s_J[6 + hi][t] * s_J[6 + hj][t]);  // Frontend.cpp:550
    __syncthreads();  // the stage is rewritten by the next chunk
  };

  int head = 0, tail = 0;  // uniform: terms compacted / terms evaluated
  for (int c = 0; c < A.n_cams; ++c) {
    if (tid == 0) inverse_transform<kTree>(A.cams[c].pose, s_Tcs);  // :115-119 (the last chunk of the camera before is done)
    __syncthreads();
    const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
    int count = *reinterpret_cast<const int32_t*>(blk + A.o_count);
    count = count < 0 ? 0 : (count > K ? K : count);
    for (int base = 0; base < count; base += kHessThreads) {
      const int k = base + tid;
      bool take = false;
      if (k < count) {
        const size_t row = (frame0 + c) * (size_t)K + (size_t)k;
        const int l = A.match_landmark[row];
        take = A.state[row] == 2 && l >= 0 && l < A.n_landmarks;
      }
      const unsigned long long bal = __ballot(take);
      if (lane == 0) s_wave[wave] = (int)__popcll(bal);
      __syncthreads();
      int pos = head + (int)__popcll(bal & ((1ull << lane) - 1ull));
      for (int w = 0; w < kHessWaves; ++w) {
        pos += w < wave ? s_wave[w] : 0;
        head += s_wave[w];
      }
      if (take) s_ring[pos & (kHessRing - 1)] = k;
      __syncthreads();
      if (head - tail >= kHessChunk) {
        evaluate(c, tail, kHessChunk);
        tail += kHessChunk;
      }
    }
    // the rest of this camera: the next one has another T_CS
    if (head > tail) {
      evaluate(c, tail, head - tail);
      tail = head;
    }
  }
  __syncthreads();
  if (tid < 36) A.H[36 * (size_t)m + tid] = acc;
  if (tid == 0) {
    A.n_terms[m] = head;
    A.n_singular[m] = s_singular;
  }
}

}  // namespace

void launch_place_hessian(const PlaceHessianArgs& args, int n_multiframes, bool rt8, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  const bool ltr = fp64_left_to_right();
  auto* kernel = rt8 ? (ltr ? place_hessian_kernel<false, true> : place_hessian_kernel<true, true>)
                     : (ltr ? place_hessian_kernel<false, false> : place_hessian_kernel<true, false>);
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kHessThreads), 0, stream, args);
}

int place_hessian_chunk_terms() { return kHessChunk; }

}  // namespace okvfe
