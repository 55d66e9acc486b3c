// capi_imu.cpp -- ImuError::propagation (okvis_ceres/src/ImuError.cpp:557-779) behind the C ABI: the host loop
// okvfe_imu_propagation (no context; the B = 1 seam and what the device call is timed against) and
// okvfe_imu_propagation_blocks_device on device-resident batches.  Both are imu_dev.h.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {

ImuParams to_params(const okvfe_imu_params& p) {
  ImuParams P;
  P.a_max = p.a_max; P.g_max = p.g_max; P.sigma_g_c = p.sigma_g_c; P.sigma_a_c = p.sigma_a_c;
  P.sigma_gw_c = p.sigma_gw_c; P.sigma_aw_c = p.sigma_aw_c; P.g = p.g;
  return P;
}

ImuResultPtrs to_ptrs(const okvfe_imu_result_device& r) {
  ImuResultPtrs R;
  R.pose = r.pose; R.speed_and_bias = r.speed_and_bias; R.n_propagated = r.n_propagated; R.status = r.status;
  R.n_out_of_range = r.n_out_of_range; R.jacobian = r.jacobian; R.covariance = r.covariance; R.T_WC = r.T_WC;
  R.gravity_C = r.gravity_C;
  return R;
}

bool bad_arguments(const okvfe_imu_params* params, const void* samples, const void* sample_begin, const void* states,
                   int32_t n_multiframes, int32_t n_cams, const double* T_SC_params, const okvfe_imu_result_device* result) {
  return !params || !samples || !sample_begin || !states || n_multiframes < 0 || n_cams < 0 ||
         (n_cams > 0 && !T_SC_params) || !result || !result->pose || !result->speed_and_bias || !result->n_propagated ||
         !result->status || !result->n_out_of_range;
}

}  // namespace

extern "C" {

okvfe_status okvfe_imu_propagation(const okvfe_imu_params* params, const double* samples, const int32_t* sample_begin,
                                   const double* states, int32_t n_multiframes, int32_t n_cams, const double* T_SC_params,
                                   int32_t order, const okvfe_imu_result_device* result) {
  if (bad_arguments(params, samples, sample_begin, states, n_multiframes, n_cams, T_SC_params, result) ||
      (order != OKVFE_SUM3_LEFT_TO_RIGHT && order != OKVFE_SUM3_EIGEN_TREE))
    return OKVFE_ERR_INVALID_ARGUMENT;
  for (int m = 0; m < n_multiframes; ++m)
    if (sample_begin[m] < 0 || sample_begin[m + 1] < sample_begin[m]) return OKVFE_ERR_INVALID_ARGUMENT;
  const ImuParams P = to_params(*params);
  const ImuResultPtrs R = to_ptrs(*result);
  for (int m = 0; m < n_multiframes; ++m) {
    if (order == OKVFE_SUM3_EIGEN_TREE)
      imu_host_multiframe<true>(P, samples, sample_begin, states, m, n_cams, T_SC_params, R);
    else
      imu_host_multiframe<false>(P, samples, sample_begin, states, m, n_cams, T_SC_params, R);
  }
  return OKVFE_OK;
}

okvfe_status okvfe_imu_propagation_blocks_device(okvfe_ctx* ctx, const okvfe_imu_params* params, const double* samples_dev,
                                                 const int32_t* sample_begin_dev, const double* states_dev,
                                                 int32_t n_multiframes, int32_t n_cams, const double* T_SC_params,
                                                 const okvfe_imu_result_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (bad_arguments(params, samples_dev, sample_begin_dev, states_dev, n_multiframes, n_cams, T_SC_params, result))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_imu_propagation_blocks_device: bad argument");
  if (n_cams > 64)
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_imu_propagation_blocks_device: %d cameras (at most 64)", n_cams);
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  // the parameters and the extrinsics: 64 + 56 n_cams bytes through the pinned parameter ring (one asynchronous copy)
  std::vector<double> rig((size_t)kImuRigHeaderDoubles + 7 * (size_t)n_cams, 0.0);
  const ImuParams P = to_params(*params);
  std::memcpy(rig.data(), &P, sizeof P);
  if (n_cams > 0) std::copy_n(T_SC_params, 7 * (size_t)n_cams, rig.data() + kImuRigHeaderDoubles);
  RingSlot slot(ctx, &ctx->pair_ring, s);
  okvfe_status st = slot.upload(rig.data(), rig.size() * sizeof(double));
  if (st != OKVFE_OK) return st;
  ImuArgs A;
  A.samples = samples_dev; A.sample_begin = sample_begin_dev; A.states = states_dev; A.rig = slot.as<double>();
  A.n_multiframes = n_multiframes; A.n_cams = n_cams; A.out = to_ptrs(*result);
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_imu_propagation(A, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = slot.release();
  ctx->last_stream = s;
  return rel;
}

}  // extern "C"
