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
#include "camera_dev.h"
#include "okvfe_internal.h"

namespace okvfe {
namespace {

std::atomic<int> g_fp64_ltr_hessian[kMaxAttrDevices];  // host, per device ordinal: 1 = left to right (0: Eigen's order, the default)
int current_device_slot() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxAttrDevices ? dev : 0;
}
template <bool kTree>
__device__ __forceinline__ double sum3h(double p0, double p1, double p2) {
  if constexpr (kTree) return p0 + (p1 + p2);
  return (p0 + p1) + p2;
}
template <bool kTree>
__device__ __forceinline__ double sum4h(double p0, double p1, double p2, double p3) {
  if constexpr (kTree) return (p0 + p1) + (p2 + p3);
  return ((p0 + p1) + p2) + p3;
}

constexpr int kHessThreads = 256;
constexpr int kHessChunk = kHessThreads;   // terms evaluated at a time: one per lane
constexpr int kHessRing = 2 * kHessChunk;  // a tile of keypoints adds at most a chunk to less than a chunk
constexpr int kHessWaves = kHessThreads / 64;
static_assert((kHessRing & (kHessRing - 1)) == 0, "ring positions are masked");

// q.normalize() and q.toRotationMatrix() of a PoseParameterBlock's (qx, qy, qz, qw) (ReprojectionError.hpp:101-103,
// :110-112, :115, :120): Eigen divides by sqrt(z) iff z = squaredNorm() > 0, so a zero or NaN quaternion stays as it is
template <bool kTree>
__device__ inline void quaternion_rotation(const double* q, double R[9]) {
  double x = q[0], y = q[1], z = q[2], w = q[3];
  const double n2 = sum4h<kTree>(x * x, y * y, z * z, w * w);
  if (n2 > 0) {
    const double n = sqrt(n2);
    x = x / n; y = y / n; z = z / n; w = w / n;
  }
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// the inverse of the pose (t, q) as a full 4 x 4 matrix (ReprojectionError.hpp:115-124): the rotation transposed, the
// translation (-C^T) t, the last row of the identity
template <bool kTree>
__device__ inline void inverse_transform(const double* pose /* t[3], qx qy qz qw */, double T[16]) {
  double C[9];
  quaternion_rotation<kTree>(pose + 3, C);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = C[3 * j + i];
    T[4 * i + 3] = sum3h<kTree>((-C[i]) * pose[0], (-C[3 + i]) * pose[1], (-C[6 + i]) * pose[2]);
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// ReprojectionError.hpp:125-162 for one term: hp_W of the landmark, the keypoint (measurement and size), T_SW and t_WS
// of the multiframe, T_CS and the intrinsics of the camera.  r = the weighted error, J = J0_minimal (2 x 6 row-major).
// Returns true where the result is the defined NaN (okvfe.h): a singular depth or a size that is no positive finite number.
template <bool kTree, bool kRT8>
__device__ __forceinline__ bool hessian_term(const DeviceCamera& cam, int w, int h, const double* T_SW, const double* t_WS,
                                             const double* T_CS, const double* hp_W, const okvfe_keypoint& kp, double r[2],
                                             double J[12]) {
  double hp_S[4], hp_C[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hp_S[i] = sum4h<kTree>(T_SW[4 * i] * hp_W[0], T_SW[4 * i + 1] * hp_W[1], T_SW[4 * i + 2] * hp_W[2],
                           T_SW[4 * i + 3] * hp_W[3]);                                      // :125
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hp_C[i] = sum4h<kTree>(T_CS[4 * i] * hp_S[0], T_CS[4 * i + 1] * hp_S[1], T_CS[4 * i + 2] * hp_S[2],
                           T_CS[4 * i + 3] * hp_S[3]);                                      // :126
  // projectHomogeneous (PinholeCamera.hpp:506-526): the head negated when w < 0, its Jacobian not negated back
  double head[3] = {hp_C[0], hp_C[1], hp_C[2]};
  if (hp_C[3] < 0) {
    head[0] = -head[0]; head[1] = -head[1]; head[2] = -head[2];
  }
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  double pt[2] = {nan, nan}, J23[6] = {nan, nan, nan, nan, nan, nan};
  const bool singular = fabs(head[2]) < 1.0e-12;  // PinholeCamera.hpp:302-304: nothing is written
  (void)cam::project_jacobian<kRT8>(cam, w, h, head, pt, J23);  // the status is ignored (ReprojectionError.hpp:133)
  const double Jh[2][4] = {{J23[0], J23[1], J23[2], 0.0}, {J23[3], J23[4], J23[5], 0.0}};  // :523-524
  // squareRootInformation_ of 64 / (size size) I (Frontend.cpp:464, ReprojectionError.hpp:75-76)
  const double size = (double)kp.size;
  const bool bad_size = !(size > 0.0 && size < __longlong_as_double(0x7FF0000000000000LL));
  const double s = sqrt(64.0 / (size * size));
  const double S[2][2] = {{s, 0.0}, {0.0, s}};
  double Jw[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) Jw[i][j] = S[i][0] * Jh[0][j] + S[i][1] * Jh[1][j];         // :134
  const double e[2] = {(double)kp.x - pt[0], (double)kp.y - pt[1]};                         // :139
  r[0] = S[0][0] * e[0] + S[0][1] * e[1];                                                   // :142
  r[1] = S[1][0] * e[0] + S[1][1] * e[1];
  // J of :155-159: [C_SW hp_W[3] | -C_SW crossMx(p)] over a zero row; C_SW is the rotation of T_SW
  const double p[3] = {hp_W[0] - t_WS[0] * hp_W[3], hp_W[1] - t_WS[1] * hp_W[3], hp_W[2] - t_WS[2] * hp_W[3]};
  const double X[3][3] = {{0.0, -p[2], p[1]}, {p[2], 0.0, -p[0]}, {-p[1], p[0], 0.0}};       // operators.hpp crossMx
  double Jp[4][6];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Jp[i][j] = T_SW[4 * i + j] * hp_W[3];
      Jp[i][3 + j] = sum3h<kTree>((-T_SW[4 * i]) * X[0][j], (-T_SW[4 * i + 1]) * X[1][j], (-T_SW[4 * i + 2]) * X[2][j]);
    }
#pragma unroll
  for (int j = 0; j < 6; ++j) Jp[3][j] = 0.0;
  // J0_minimal = (Jh_weighted T_CS) J (:163)
  double A[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      A[i][j] = sum4h<kTree>(Jw[i][0] * T_CS[j], Jw[i][1] * T_CS[4 + j], Jw[i][2] * T_CS[8 + j], Jw[i][3] * T_CS[12 + j]);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j)
      J[6 * i + j] = sum4h<kTree>(A[i][0] * Jp[0][j], A[i][1] * Jp[1][j], A[i][2] * Jp[2][j], A[i][3] * Jp[3][j]);
  if (singular || bad_size) {
    r[0] = nan; r[1] = nan;
#pragma unroll
    for (int j = 0; j < 12; ++j) J[j] = nan;
    return true;
  }
  return false;
}

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
  const bool ltr = g_fp64_ltr_hessian[current_device_slot()].load() != 0;
  auto* kernel = rt8 ? (ltr ? place_hessian_kernel<false, true> : place_hessian_kernel<true, true>)
                     : (ltr ? place_hessian_kernel<false, false> : place_hessian_kernel<true, false>);
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kHessThreads), 0, stream, args);
}

int place_hessian_chunk_terms() { return kHessChunk; }

bool set_fp64_tree_place_hessian(int tree) {
  g_fp64_ltr_hessian[current_device_slot()].store(tree ? 0 : 1);  // (the caller has set and drained the device)
  return true;
}

}  // namespace okvfe
