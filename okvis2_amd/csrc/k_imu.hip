// k_imu.hip -- ImuError::propagation (okvis_ceres/src/ImuError.cpp:557-779) for a batch of multiframes: the pose guess,
// its Jacobian F, its covariance P, and per camera T_WC and the extraction direction.  The arithmetic is imu_dev.h, the
// same sequence the host entry okvfe_imu_propagation compiles; this file only deals it to lanes.  Three forms, because
// the live state differs by an order of magnitude:
//   imu_lane_kernel<kTree, false>   the mean only (what the reference calls on every frame): a lane per multiframe, about
//                                   two dozen doubles of state; the ragged trip count runs under exec masks
//   imu_lane_kernel<kTree, true>    with F: the six 3 x 3 accumulators on top, still a lane per multiframe
//   imu_cov_kernel<kTree>           with P: a wave per multiframe.  The small state is computed by every lane alike (the
//                                   control flow is uniform); P_delta, F_delta P_delta and F_delta lie in LDS (3 x 1800 B),
//                                   lane l owns entries l, l + 64, l + 128, l + 192 of every product and walks k in
//                                   ascending order (imu_dot15), so the sums are the host's
// FP64 without FMA; 3- and 4-term sums in the order of okvfe_set_fp64_reduction (a template argument).  Every index is
// a 64-bit product.  No scratch in any form (profiles/imu_propagation.txt).
#include "imu_dev.h"
#include "okvfe_internal.h"

namespace okvfe {
namespace {

constexpr int kImuThreads = 64;  // one wave per work-group in every form

__device__ __forceinline__ ImuParams load_params(const double* rig) {
  ImuParams P;
  P.a_max = rig[0]; P.g_max = rig[1]; P.sigma_g_c = rig[2]; P.sigma_a_c = rig[3]; P.sigma_gw_c = rig[4];
  P.sigma_aw_c = rig[5]; P.g = rig[6];
  return P;
}

template <bool kTree, bool kJac>
__global__ __launch_bounds__(kImuThreads) void imu_lane_kernel(ImuArgs A) {
  const long long m = (long long)blockIdx.x * kImuThreads + threadIdx.x;
  if (m >= A.n_multiframes) return;
  const ImuParams prm = load_params(A.rig);
  const int begin = A.sample_begin[m];
  const int n = A.sample_begin[m + 1] - begin;
  ImuOut o;
  ImuCovNone cov;
  double C_WS_0[9];
  imu_propagate<kTree, kJac, false>(prm, A.samples + (long long)begin * kImuSampleDoubles, n,
                                    A.states + m * kImuStateDoubles, cov, o, C_WS_0);
  imu_store<kTree, kJac>(A.out, m, A.n_cams, A.rig + kImuRigHeaderDoubles, o);
}

// the covariance in LDS: the kernel's form of ImuCovHost (imu_dev.h), entry for entry the same sums
struct ImuCovLds {
  double *P, *FP, *F;
  int lane;
  __device__ __forceinline__ void begin() {
    for (int e = lane; e < 225; e += kImuThreads) {
      P[e] = 0.0;
      F[e] = e % 16 == 0 ? 1.0 : 0.0;
    }
    __syncthreads();
  }
  __device__ __forceinline__ void products(double* out, bool noise, ImuNoise N) {
    for (int e = lane; e < 225; e += kImuThreads) FP[e] = imu_dot15(F + 15 * (e / 15), 1, P + e % 15, 15);
    __syncthreads();
    for (int e = lane; e < 225; e += kImuThreads) {
      double v = imu_dot15(FP + 15 * (e / 15), 1, F + 15 * (e % 15), 1);
      if (noise && e % 16 == 0) v = v + imu_noise_of(N, e / 16);
      out[e] = v;
    }
    __syncthreads();  // F and P are free again
  }
  __device__ __forceinline__ void step(const ImuBlocks& B, const ImuNoise& N) {
    if (lane == 0) imu_put_blocks(B, F);
    __syncthreads();
    products(P, true, N);
  }
  __device__ __forceinline__ void finish(const double* C_WS_0, double* out) {
    for (int e = lane; e < 225; e += kImuThreads) F[e] = e % 16 == 0 ? 1.0 : 0.0;
    __syncthreads();
    if (lane == 0) imu_put_T(C_WS_0, F);
    __syncthreads();
    products(out, false, ImuNoise{});
  }
};

template <bool kTree>
__global__ __launch_bounds__(kImuThreads) void imu_cov_kernel(ImuArgs A) {
  __shared__ double s_P[225], s_FP[225], s_F[225];
  const long long m = blockIdx.x;
  const ImuParams prm = load_params(A.rig);
  const int begin = A.sample_begin[m];
  const int n = A.sample_begin[m + 1] - begin;
  ImuOut o;
  ImuCovLds cov{s_P, s_FP, s_F, (int)threadIdx.x};
  double C_WS_0[9];
  // every lane runs the same multiframe: the branches are uniform, so the barriers inside cov are reached by all
  imu_propagate<kTree, true, true>(prm, A.samples + (long long)begin * kImuSampleDoubles, n,
                                   A.states + m * kImuStateDoubles, cov, o, C_WS_0);
  if (o.wrote_jacobian) cov.finish(C_WS_0, A.out.covariance + 225 * m);
  if (threadIdx.x == 0) imu_store<kTree, true>(A.out, m, A.n_cams, A.rig + kImuRigHeaderDoubles, o);
}

}  // namespace

void launch_imu_propagation(const ImuArgs& args, hipStream_t stream) {
  if (args.n_multiframes <= 0) return;
  const bool ltr = fp64_left_to_right();
  const unsigned lane_blocks = (unsigned)((args.n_multiframes + kImuThreads - 1) / kImuThreads);
  if (args.out.covariance) {
    auto* kernel = ltr ? imu_cov_kernel<false> : imu_cov_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)args.n_multiframes), dim3(kImuThreads), 0, stream, args);
  } else if (args.out.jacobian) {
    auto* kernel = ltr ? imu_lane_kernel<false, true> : imu_lane_kernel<true, true>;
    hipLaunchKernelGGL(kernel, dim3(lane_blocks), dim3(kImuThreads), 0, stream, args);
  } else {
    auto* kernel = ltr ? imu_lane_kernel<false, false> : imu_lane_kernel<true, false>;
    hipLaunchKernelGGL(kernel, dim3(lane_blocks), dim3(kImuThreads), 0, stream, args);
  }
}

}  // namespace okvfe
