// k_map.hip -- Frontend::matchToMap before its matcher threads start: projection of every landmark
// into the current camera and the descriptor-view pooling (okvis_frontend/src/Frontend.cpp:1219-1359).
//   prepare_landmarks_kernel   one thread per landmark: FoV check through the camera model
//                              (camera_dev.h), 3-D test, view-point / scale pruning, the three-slot
//                              "keep the best" buffer with the reference's exact write / crop rules
//                              (oracle: orc_prepare_landmarks documents the quirks);
//   compact_landmarks_kernel   the 3-D landmarks as the packed set the matcher kernel reads
//                              (projections, <= 2 pooled descriptors each), in landmark order;
//   prepare_landmarks_frames_kernel / pack_landmarks_frames_kernel   the same two steps for a batch of
//                              frames against one device-resident table: blockIdx.y resp. the work-group
//                              is the frame, the packed record names observation rows instead of copying
//                              descriptors, and the count of 3-D landmarks stays on the device;
//   pack_uninit_frames_kernel   the landmarks a frame's first pass left with status 2 (not 3-D yet), packed in
//                              table order for the second pass (okvfe_match_to_map_table_uninitialised_blocks_device);
//   check_landmark_table_kernel   the structural checks of a device-resident table;
//   stereo_insert_kernel       (stereo_insert_dev.h, included below) matchStereo's landmark bookkeeping
//                              (Frontend.cpp:2076-2141) chained over the camera pairs of a rig, one work-group per
//                              multiframe, on this file's projection chain.
// FP64, 3-term sums in the order of okvfe_set_fp64_reduction, no FMA; acos / cos through atan_fixed.h resp. host-computed constants.
#include "camera_dev.h"
#include "fp64_ops.h"
#include "okvfe_internal.h"

namespace okvfe {
namespace {

// order of the 3-term sums: as in k_match.hip (okvfe_set_fp64_reduction), this translation unit's device symbol
__device__ int g_fp64_tree_map = 1;
__device__ __forceinline__ double sum3(double p0, double p1, double p2) {
  return fp64::sum3_select(g_fp64_tree_map != 0, p0, p1, p2);
}
__device__ __forceinline__ double dot3m(const double a[3], const double b[3]) {
  const double p0 = a[0] * b[0];
  const double p1 = a[1] * b[1];
  const double p2 = a[2] * b[2];
  return sum3(p0, p1, p2);
}
__device__ __forceinline__ void normalize3m(const double v[3], double out[3]) {
  const double n = sqrt(dot3m(v, v));
  out[0] = v[0] / n;
  out[1] = v[1] / n;
  out[2] = v[2] / n;
}

// hp_C = T_WC^-1 * hp_W as the reference's Transformation::inverse() * hp evaluates it.  The ONE copy of this expression
// order: prepare_landmark, remove_outliers_frames_kernel and stereo_insert_kernel (stereo_insert_dev.h) compile it.
__device__ __forceinline__ void pose_inverse_times(const okvfe_pose& T1, const double hp[4], double hp_C[4]) {
  double cr[3], hh[3];
  for (int i = 0; i < 3; ++i) {
    cr[i] = sum3(T1.C[i] * T1.r[0], T1.C[3 + i] * T1.r[1], T1.C[6 + i] * T1.r[2]);
    hh[i] = sum3(T1.C[i] * hp[0], T1.C[3 + i] * hp[1], T1.C[6 + i] * hp[2]);
  }
  for (int i = 0; i < 3; ++i) hp_C[i] = hh[i] + (-cr[i]) * hp[3];
  hp_C[3] = hp[3];
}

// what the pooling leaves of one landmark: the row of okvfe_landmark_pool (zero / -1 when the landmark is not kept)
struct Prepared {
  int32_t status, n_desc, rows[3];
  double proj[2], ew[2][3], rw[2][3];
};

// One landmark of Frontend.cpp:1219-1359.  The ONE copy of the reference's FP64 expression order: both
// prepare_landmarks_kernel (B = 1) and prepare_landmarks_frames_kernel (a batch of frames) compile it.
template <bool kRT8>  // camera_dev.h: the form that also knows OKVFE_DIST_RADTAN8
__device__ __forceinline__ void prepare_landmark(
    int l, const double* __restrict__ hp_W, const double* __restrict__ quality,
    const int32_t* __restrict__ obs_begin, const int32_t* __restrict__ obs_pose,
    const double* __restrict__ obs_bp, const okvfe_pose* __restrict__ poses, const okvfe_pose& T1,
    const DeviceCamera& cam, int w, int h, double repr, int exclusive, double cos10, double cos06, Prepared& P) {
  P.status = P.n_desc = 0;
  P.rows[0] = P.rows[1] = P.rows[2] = -1;
  P.proj[0] = P.proj[1] = 0.0;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 3; ++i) P.ew[k][i] = P.rw[k][i] = 0.0;
  const double hp[4] = {hp_W[4 * (size_t)l], hp_W[4 * (size_t)l + 1], hp_W[4 * (size_t)l + 2], hp_W[4 * (size_t)l + 3]};
  const double p_W[3] = {hp[0] / hp[3], hp[1] / hp[3], hp[2] / hp[3]};
  const double r_Wv[3] = {p_W[0] - T1.r[0], p_W[1] - T1.r[1], p_W[2] - T1.r[2]};
  double e_Wv[3];
  normalize3m(r_Wv, e_Wv);
  const double rn = sqrt(dot3m(r_Wv, r_Wv));
  const double r = 0.01 > rn ? 0.01 : rn;
  double hp_C[4];
  pose_inverse_times(T1, hp, hp_C);
  double head[3], kp[2];
  if (hp_C[3] < 0) {
    head[0] = -hp_C[0]; head[1] = -hp_C[1]; head[2] = -hp_C[2];
  } else {
    head[0] = hp_C[0]; head[1] = hp_C[1]; head[2] = hp_C[2];
  }
  const int st = cam::project<kRT8>(cam, w, h, head, kp);
  if (st == 4 || st == 3) return;  // Invalid, Behind
  const double maxU = (double)w + repr, maxV = (double)h + repr;
  if (kp[0] < -repr || kp[1] < -repr || kp[0] > maxU || kp[1] > maxV) return;
  P.proj[0] = kp[0];
  P.proj[1] = kp[1];
  const double focal = cam.fu + cam.fv;
  bool is3d = false;
  int o = 0, rows[3] = {-1, -1, -1};
  double best[3] = {1.0, 1.0, 1.0}, ew[3][3], rw[3][3];
  for (int ob = obs_begin[l]; ob < obs_begin[l + 1]; ++ob) {
    const okvfe_pose& To = poses[obs_pose[ob]];
    const double r_old[3] = {p_W[0] - To.r[0], p_W[1] - To.r[1], p_W[2] - To.r[2]};
    if (!is3d) {
      const double f = 0.2 / focal / quality[l];
      const double rc[3] = {r_Wv[0] - f * r_old[0], r_Wv[1] - f * r_old[1], r_Wv[2] - f * r_old[2]};
      double a[3], b[3];
      normalize3m(r_Wv, a);
      normalize3m(rc, b);
      if (dot3m(a, b) > cos10) is3d = true;
    }
    double eo[3];
    normalize3m(r_old, eo);
    const double cosVC = dot3m(e_Wv, eo);
    if (cosVC < cos06 && !exclusive) continue;
    const double scaleChange = fabs(r - sqrt(dot3m(r_old, r_old))) / r;
    if (scaleChange > 0.5 && !exclusive) continue;
    const double score = 0.5 * (acos_fixed(cosVC) / 0.6 + scaleChange / 0.5);
    double worst = 0.0;
    int wi = 0;
    for (int n = 0; n < 3; ++n)
      if (best[n] > worst) {
        worst = best[n];
        wi = n;
      }
    if (score < best[wi]) {
      const double bpv[3] = {obs_bp[3 * (size_t)ob], obs_bp[3 * (size_t)ob + 1], obs_bp[3 * (size_t)ob + 2]};
      double en[3], ev[3];
      normalize3m(bpv, en);
      ev[0] = dot3m(To.C, en);
      ev[1] = dot3m(To.C + 3, en);
      ev[2] = dot3m(To.C + 6, en);
      // rows / ew / rw are indexed with the run-time value o in {0, 1, 2}
      for (int k = 0; k < 3; ++k)
        if (k == o) {
          rows[k] = ob;
          ew[k][0] = ev[0]; ew[k][1] = ev[1]; ew[k][2] = ev[2];
          rw[k][0] = To.r[0]; rw[k][1] = To.r[1]; rw[k][2] = To.r[2];
        }
      o = o > wi ? o : wi;
      for (int k = 0; k < 3; ++k)
        if (k == wi) best[k] = score;
    }
  }
  if (o == 0) return;
  P.status = is3d ? 1 : 2;
  P.n_desc = o;
  for (int k = 0; k < 3; ++k) P.rows[k] = rows[k];
  for (int k = 0; k < 2; ++k)
    if (k < o)
      for (int i = 0; i < 3; ++i) {
        P.ew[k][i] = ew[k][i];
        P.rw[k][i] = rw[k][i];
      }
}

__device__ __forceinline__ void store_prepared(const Prepared& P, size_t l, int32_t* __restrict__ status,
                                               int32_t* __restrict__ n_desc, int32_t* __restrict__ obs_rows,
                                               double* __restrict__ projection, double* __restrict__ e_W,
                                               double* __restrict__ r_W) {
  if (status) status[l] = P.status;
  if (n_desc) n_desc[l] = P.n_desc;
  if (obs_rows)
    for (int k = 0; k < 3; ++k) obs_rows[3 * l + k] = P.rows[k];
  if (projection) {
    projection[2 * l] = P.proj[0];
    projection[2 * l + 1] = P.proj[1];
  }
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 3; ++i) {
      if (e_W) e_W[6 * l + 3 * k + i] = P.ew[k][i];
      if (r_W) r_W[6 * l + 3 * k + i] = P.rw[k][i];
    }
}

template <bool kRT8>
__global__ __launch_bounds__(128) void prepare_landmarks_kernel(
    const double* __restrict__ hp_W, const double* __restrict__ quality,
    const int32_t* __restrict__ obs_begin, int n_landmarks, const int32_t* __restrict__ obs_pose,
    const double* __restrict__ obs_bp, const okvfe_pose* __restrict__ poses, okvfe_pose T1,
    const DeviceCamera* __restrict__ camera, int w, int h, double repr, int exclusive, double cos10,
    double cos06, int32_t* __restrict__ status, int32_t* __restrict__ n_desc,
    int32_t* __restrict__ obs_rows, double* __restrict__ projection, double* __restrict__ e_W,
    double* __restrict__ r_W) {
  const int l = blockIdx.x * 128 + threadIdx.x;
  if (l >= n_landmarks) return;
  const DeviceCamera cam = *camera;
  Prepared P;
  prepare_landmark<kRT8>(l, hp_W, quality, obs_begin, obs_pose, obs_bp, poses, T1, cam, w, h, repr, exclusive, cos10,
                         cos06, P);
  store_prepared(P, (size_t)l, status, n_desc, obs_rows, projection, e_W, r_W);
}

// The same for a batch of frames against one device-resident table (okvfe_match_to_map_table_blocks_device):
// blockIdx.y = frame, whose pose, camera slot and cos(10 / focal) come from the parameter block.  The pooling rows go to
// the caller's frame-major arrays (each may be null); what the matcher needs -- projection, table index (-1 = not 3-D)
// and the observation rows of the <= 2 pooled descriptors -- goes to the frame's MapPacked records, unpacked.
template <bool kRT8>
__global__ __launch_bounds__(128) void prepare_landmarks_frames_kernel(
    const double* __restrict__ hp_W, const double* __restrict__ quality,
    const int32_t* __restrict__ obs_begin, int n_landmarks, const int32_t* __restrict__ obs_pose,
    const double* __restrict__ obs_bp, const okvfe_pose* __restrict__ poses,
    const MapFrameParams* __restrict__ frames, const DeviceCamera* __restrict__ cameras, int w, int h, double repr,
    int exclusive, double cos06, int32_t* __restrict__ status, int32_t* __restrict__ n_desc,
    int32_t* __restrict__ obs_rows, double* __restrict__ projection, double* __restrict__ e_W,
    double* __restrict__ r_W, MapPacked* __restrict__ packed) {
  const int l = blockIdx.x * 128 + threadIdx.x;
  if (l >= n_landmarks) return;
  const MapFrameParams& fp = frames[blockIdx.y];
  const DeviceCamera cam = cameras[fp.cam];
  Prepared P;
  prepare_landmark<kRT8>(l, hp_W, quality, obs_begin, obs_pose, obs_bp, poses, fp.T1, cam, w, h, repr, exclusive,
                         fp.cos10, cos06, P);
  const size_t i = (size_t)blockIdx.y * (size_t)n_landmarks + (size_t)l;
  store_prepared(P, i, status, n_desc, obs_rows, projection, e_W, r_W);
  MapPacked rec;
  rec.px = P.proj[0];
  rec.py = P.proj[1];
  rec.index = P.status == 1 ? l : -1;
  rec.row0 = P.rows[0];
  rec.row1 = P.n_desc > 1 ? P.rows[1] : -1;
  rec.pad = 0;
  packed[i] = rec;
}

// The 3-D landmarks of every frame moved to the front of the frame's records, in landmark order and IN PLACE: one
// work-group per frame, the chunked scan of compact_landmarks_kernel below.  A chunk is read into registers before any
// of it is written, and its records land at or below their own place, so no unread record is overwritten.  The count
// stays in device memory (counts[frame]): the matcher reads it there.
__global__ __launch_bounds__(1024) void pack_landmarks_frames_kernel(MapPacked* __restrict__ packed, int n_landmarks,
                                                                      int32_t* __restrict__ counts) {
  __shared__ int s_lm[1024];
  __shared__ int base_lm;
  MapPacked* P = packed + (size_t)blockIdx.x * (size_t)n_landmarks;
  const int tid = threadIdx.x;
  if (tid == 0) base_lm = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n_landmarks; c0 += 1024) {
    const int l = c0 + tid;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0xffffffffu, 0, 0, 0);  // the record as two 16-byte halves
    if (l < n_landmarks) {
      lo = reinterpret_cast<const uint4*>(P + l)[0];
      hi = reinterpret_cast<const uint4*>(P + l)[1];
    }
    const bool take = (int32_t)hi.x >= 0;  // MapPacked::index
    s_lm[tid] = take ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan
      const int a = tid >= d ? s_lm[tid - d] : 0;
      __syncthreads();
      s_lm[tid] += a;
      __syncthreads();
    }
    if (take) {
      uint4* dst = reinterpret_cast<uint4*>(P + (base_lm + s_lm[tid] - 1));
      dst[0] = lo;
      dst[1] = hi;
    }
    __syncthreads();
    if (tid == 1023) base_lm += s_lm[1023];
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = base_lm;
}

// okvfe_match_to_map_table_uninitialised_blocks_device: the landmarks of every frame that the first pass left with
// status 2 (not 3-D yet), as one MapUninitPacked record each at the front of the frame's records, in table order: one
// work-group per frame, the chunked scan of pack_landmarks_frames_kernel.  Reads the frame's rows of the caller's pool
// (status, n_desc, obs_rows; the cropped third row is never read); the count stays in device memory (counts[frame]).
__global__ __launch_bounds__(1024) void pack_uninit_frames_kernel(const int32_t* __restrict__ status,
                                                                   const int32_t* __restrict__ n_desc,
                                                                   const int32_t* __restrict__ obs_rows, int n_landmarks,
                                                                   MapUninitPacked* __restrict__ packed,
                                                                   int32_t* __restrict__ counts) {
  __shared__ int s_lm[1024];
  __shared__ int base_lm;
  const size_t row0 = (size_t)blockIdx.x * (size_t)n_landmarks;
  MapUninitPacked* P = packed + row0;
  const int tid = threadIdx.x;
  if (tid == 0) base_lm = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n_landmarks; c0 += 1024) {
    const int l = c0 + tid;
    const bool take = l < n_landmarks && status[row0 + l] == 2;
    s_lm[tid] = take ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scan
      const int a = tid >= d ? s_lm[tid - d] : 0;
      __syncthreads();
      s_lm[tid] += a;
      __syncthreads();
    }
    if (take) {
      const int nd = n_desc[row0 + l];
      int4 rec;
      rec.x = l;
      rec.y = nd > 0 ? obs_rows[3 * (row0 + l)] : -1;
      rec.z = nd > 1 ? obs_rows[3 * (row0 + l) + 1] : -1;
      rec.w = 0;
      *reinterpret_cast<int4*>(P + (base_lm + s_lm[tid] - 1)) = rec;
    }
    __syncthreads();
    if (tid == 1023) base_lm += s_lm[1023];
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = base_lm;
}

// okvfe_remove_outliers_blocks_device: Frontend::removeOutliers (Frontend.cpp:2152-2205) for a batch of frames.  One
// thread per keypoint, blockIdx.y = frame (pose and camera slot from the parameter block).  A keypoint that carries table
// row l is removed (landmark_out = -1) iff the landmark does not project successfully or lands more than max_error
// pixels from the keypoint; a kept one counts into kept[frame].  Rows without a landmark, or with one outside the table
// (:2177 fails), pass through.  landmark_out may be landmark: a thread reads and writes its own row only.
template <bool kRT8>
__global__ __launch_bounds__(128) void remove_outliers_frames_kernel(
    const double* __restrict__ hp_W, int n_landmarks, const MapFrameParams* __restrict__ frames,
    const DeviceCamera* __restrict__ cameras, int w, int h, const uint8_t* __restrict__ blocks, int o_count, int o_kps,
    size_t block_bytes, int kp_cap, double max_error, const int32_t* landmark, int32_t* landmark_out,
    int32_t* __restrict__ kept) {
  const int k = blockIdx.x * 128 + threadIdx.x;
  const size_t f = blockIdx.y;
  const uint8_t* blk = blocks + f * block_bytes;
  int count = *reinterpret_cast<const int32_t*>(blk + o_count);
  count = count < 0 ? 0 : (count > kp_cap ? kp_cap : count);
  bool keep = false;
  if (k < count) {
    const size_t row = f * (size_t)kp_cap + (size_t)k;
    const int l = landmark[row];
    int out = l;
    if (l >= 0 && l < n_landmarks) {
      const MapFrameParams& fp = frames[f];
      const DeviceCamera cam = cameras[fp.cam];
      const double hp[4] = {hp_W[4 * (size_t)l], hp_W[4 * (size_t)l + 1], hp_W[4 * (size_t)l + 2], hp_W[4 * (size_t)l + 3]};
      double hp_C[4], head[3], proj[2];
      pose_inverse_times(fp.T1, hp, hp_C);
      if (hp_C[3] < 0) {  // projectHomogeneous
        head[0] = -hp_C[0]; head[1] = -hp_C[1]; head[2] = -hp_C[2];
      } else {
        head[0] = hp_C[0]; head[1] = hp_C[1]; head[2] = hp_C[2];
      }
      bool remove = true;
      if (cam::project<kRT8>(cam, w, h, head, proj) == 0) {
        const okvfe_keypoint kp = reinterpret_cast<const okvfe_keypoint*>(blk + o_kps)[k];
        const double dx = proj[0] - (double)kp.x, dy = proj[1] - (double)kp.y;
        remove = sqrt(dx * dx + dy * dy) > max_error;  // :2185 (a NaN norm is kept)
      }
      keep = !remove;
      if (remove) out = -1;
    }
    landmark_out[row] = out;
  }
  const unsigned long long kb = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && kb) atomicAdd(&kept[f], (int)__popcll(kb));
}

// okvfe_landmark_table_check_device: what the host form checks on its host arrays.  bad[0] / bad[1] = first offending
// landmark row of obs_begin / first observation with a pose index out of range (0xffffffff = none).
__global__ __launch_bounds__(256) void check_landmark_table_kernel(const int32_t* __restrict__ obs_begin, int n_landmarks,
                                                                    const int32_t* __restrict__ obs_pose,
                                                                    int n_observations, int n_poses,
                                                                    uint32_t* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_landmarks) {
    const int b = obs_begin[i], e = obs_begin[i + 1];
    if (e < b || b < 0 || e > n_observations) atomicMin(&bad[0], (uint32_t)i);
  }
  if (i < n_observations) {
    const int p = obs_pose[i];
    if (p < 0 || p >= n_poses) atomicMin(&bad[1], (uint32_t)i);
  }
}

// the landmarks with status == want as a packed set, in landmark order (single workgroup: the
// landmark table of a frame is a few thousand rows)
__global__ __launch_bounds__(1024) void compact_landmarks_kernel(
    const int32_t* __restrict__ status, const int32_t* __restrict__ n_desc,
    const int32_t* __restrict__ obs_rows, const double* __restrict__ projection,
    const uint8_t* __restrict__ obs_desc, int n_landmarks, int want, int32_t* __restrict__ index_out,
    double* __restrict__ proj_out, int32_t* __restrict__ begin_out, uint8_t* __restrict__ pool_out,
    int32_t* __restrict__ n_out /* [0] landmarks, [1] pool rows */) {
  __shared__ int s_lm[1024], s_rows[1024];
  __shared__ int base_lm, base_rows;
  const int tid = threadIdx.x;
  if (tid == 0) base_lm = base_rows = 0;
  __syncthreads();
  for (int c0 = 0; c0 < n_landmarks; c0 += 1024) {
    const int l = c0 + tid;
    const bool take = l < n_landmarks && status[l] == want;
    const int nd = take ? n_desc[l] : 0;
    s_lm[tid] = take ? 1 : 0;
    s_rows[tid] = nd;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // inclusive scans
      const int a = tid >= d ? s_lm[tid - d] : 0, b = tid >= d ? s_rows[tid - d] : 0;
      __syncthreads();
      s_lm[tid] += a;
      s_rows[tid] += b;
      __syncthreads();
    }
    if (take) {
      const int pos = base_lm + s_lm[tid] - 1, row0 = base_rows + s_rows[tid] - nd;
      index_out[pos] = l;
      proj_out[2 * pos] = projection[2 * l];
      proj_out[2 * pos + 1] = projection[2 * l + 1];
      begin_out[pos] = row0;
      for (int k = 0; k < nd; ++k) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(obs_desc + (size_t)obs_rows[3 * l + k] * OKVFE_DESC_BYTES);
        uint32_t* dst = reinterpret_cast<uint32_t*>(pool_out + (size_t)(row0 + k) * OKVFE_DESC_BYTES);
        for (int i = 0; i < 12; ++i) dst[i] = src[i];
      }
    }
    __syncthreads();
    if (tid == 1023) {
      base_lm += s_lm[1023];
      base_rows += s_rows[1023];
    }
    __syncthreads();
  }
  if (tid == 0) {
    begin_out[base_lm] = base_rows;
    n_out[0] = base_lm;
    n_out[1] = base_rows;
  }
}

// matchStereo's landmark bookkeeping (okvfe_stereo_insert_blocks_device): stereo_insert_kernel, on the projection chain above
#include "stereo_insert_dev.h"

}  // namespace

size_t stereo_insert_lds_bytes(int n_cams, int kp_cap, int* ov_log2, int* kh_log2) {
  int a = 1, b = 1;
  while (((int64_t)1 << a) <= (int64_t)n_cams * kp_cap) ++a;  // more slots than entries: a probe always ends
  while (((int64_t)1 << b) <= (int64_t)2 * kp_cap) ++b;
  if (ov_log2) *ov_log2 = a;
  if (kh_log2) *kh_log2 = b;
  return sizeof(int32_t) * ((size_t)n_cams * kp_cap + ((size_t)1 << a) + 3 * (size_t)kp_cap + ((size_t)1 << b));
}
void launch_stereo_insert(const StereoInsertArgs& args, size_t lds_bytes, hipStream_t stream, bool rt8) {
  if (args.n_multiframes <= 0 || args.kp_cap <= 0) return;
  hipLaunchKernelGGL(rt8 ? stereo_insert_kernel<true> : stereo_insert_kernel<false>, dim3(args.n_multiframes), dim3(256),
                     lds_bytes, stream, args);
}

void launch_prepare_landmarks(const double* hp_W, const double* quality, const int32_t* obs_begin,
                              int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                              const okvfe_pose* poses, const okvfe_pose& T_WC1, const DeviceCamera* camera,
                              int w, int h, double repr, int exclusive, double cos10, double cos06,
                              int32_t* status, int32_t* n_desc, int32_t* obs_rows, double* projection,
                              double* e_W, double* r_W, hipStream_t stream, bool rt8) {
  if (n_landmarks <= 0) return;
  hipLaunchKernelGGL(rt8 ? prepare_landmarks_kernel<true> : prepare_landmarks_kernel<false>, dim3((n_landmarks + 127) / 128), dim3(128), 0, stream, hp_W,
                     quality, obs_begin, n_landmarks, obs_pose, obs_bp, poses, T_WC1, camera, w, h, repr,
                     exclusive, cos10, cos06, status, n_desc, obs_rows, projection, e_W, r_W);
}
void launch_compact_landmarks(const int32_t* status, const int32_t* n_desc, const int32_t* obs_rows,
                              const double* projection, const uint8_t* obs_desc, int n_landmarks, int want,
                              int32_t* index_out, double* proj_out, int32_t* begin_out, uint8_t* pool_out,
                              int32_t* n_out, hipStream_t stream) {
  hipLaunchKernelGGL(compact_landmarks_kernel, dim3(1), dim3(1024), 0, stream, status, n_desc, obs_rows,
                     projection, obs_desc, n_landmarks, want, index_out, proj_out, begin_out, pool_out, n_out);
}

void launch_prepare_landmarks_frames(const double* hp_W, const double* quality, const int32_t* obs_begin,
                                     int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                                     const okvfe_pose* poses, const MapFrameParams* frames, int n_frames,
                                     const DeviceCamera* cameras, int w, int h, double repr, int exclusive,
                                     double cos06, int32_t* status, int32_t* n_desc, int32_t* obs_rows,
                                     double* projection, double* e_W, double* r_W, MapPacked* packed,
                                     int32_t* counts, hipStream_t stream, bool rt8) {
  if (n_frames <= 0) return;
  if (n_landmarks > 0)
    hipLaunchKernelGGL(rt8 ? prepare_landmarks_frames_kernel<true> : prepare_landmarks_frames_kernel<false>,
                       dim3((n_landmarks + 127) / 128, n_frames), dim3(128), 0, stream, hp_W, quality, obs_begin,
                       n_landmarks, obs_pose, obs_bp, poses, frames, cameras, w, h, repr, exclusive, cos06, status,
                       n_desc, obs_rows, projection, e_W, r_W, packed);
  hipLaunchKernelGGL(pack_landmarks_frames_kernel, dim3(n_frames), dim3(1024), 0, stream, packed, n_landmarks, counts);
}
void launch_pack_uninit_frames(const int32_t* status, const int32_t* n_desc, const int32_t* obs_rows, int n_landmarks,
                               int n_frames, MapUninitPacked* packed, int32_t* counts, hipStream_t stream) {
  if (n_frames <= 0) return;
  hipLaunchKernelGGL(pack_uninit_frames_kernel, dim3(n_frames), dim3(1024), 0, stream, status, n_desc, obs_rows,
                     n_landmarks, packed, counts);
}
void launch_remove_outliers_frames(const double* hp_W, int n_landmarks, const MapFrameParams* frames, int n_frames,
                                   const DeviceCamera* cameras, int w, int h, const BlockLayout& L, const uint8_t* blocks,
                                   int kp_cap, double max_error, const int32_t* landmark, int32_t* landmark_out,
                                   int32_t* kept, hipStream_t stream, bool rt8) {
  if (kp_cap <= 0) return;
  for (int f0 = 0; f0 < n_frames; f0 += 65535) {  // a launch's grid.y
    const int nf = n_frames - f0 < 65535 ? n_frames - f0 : 65535;
    const size_t row = (size_t)f0 * (size_t)kp_cap;
    hipLaunchKernelGGL(rt8 ? remove_outliers_frames_kernel<true> : remove_outliers_frames_kernel<false>,
                       dim3((kp_cap + 127) / 128, nf), dim3(128), 0, stream, hp_W, n_landmarks, frames + f0, cameras, w, h,
                       blocks + (size_t)f0 * L.total, (int)L.o_count, (int)L.o_kps, L.total, kp_cap, max_error,
                       landmark + row, landmark_out + row, kept + f0);
  }
}
void launch_check_landmark_table(const int32_t* obs_begin, int n_landmarks, const int32_t* obs_pose,
                                 int n_observations, int n_poses, uint32_t* bad, hipStream_t stream) {
  const int n = n_landmarks > n_observations ? n_landmarks : n_observations;
  if (n <= 0) return;
  hipLaunchKernelGGL(check_landmark_table_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, obs_begin, n_landmarks,
                     obs_pose, n_observations, n_poses, bad);
}

bool set_fp64_tree_map(int tree) {
  const int v = tree != 0;
  return hipMemcpyToSymbol(HIP_SYMBOL(g_fp64_tree_map), &v, sizeof(v)) == hipSuccess;
}

}  // namespace okvfe
