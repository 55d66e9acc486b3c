// stereo_insert_dev.h -- the kernel of okvfe_stereo_insert_blocks_device.  Included by k_map.hip inside its anonymous
// namespace, so that it compiles that file's ONE copy of the projection chain (pose_inverse_times, the camera's
// project) under that file's device symbol of the okvfe_set_fp64_reduction order.  Not a header for anything else.
// ---- okvfe_stereo_insert_blocks_device: matchStereo's landmark bookkeeping (Frontend.cpp:2076-2141) ----
// One work-group per multiframe walks the camera pairs in list order; the rig's landmark ids live in LDS.  Dynamic LDS,
// int32 each (K = kp_cap):
//   ids    n_cams x K   id[c][k]: table row, L + p K + k0 for a landmark row (p, k0) created, -1 none.  An id is only ever
//                       written over -1 (add0 needs id0 unset, add1 needs id1 unset), so a keypoint's id never changes
//                       once it is set;
//   ov     ov_size      the view's overlay: open-addressed set of the rows (p K + k0) that re-initialised a landmark.  The
//                       key of an entry is not stored: it is id[c0(p)][k0], which cannot change any more.  A landmark is
//                       re-initialised at most once and must be carried by a keypoint then, so n_cams K entries bound it;
//   k1_of  K            the pair's valid k1 per k0 (-1: no match);
//   head   K            per k1: the smallest k0 that matched it (the head of the chain);
//   state  K            per k1: rows in the chain, | kStereoEntangled;
//   kh     kh_size      the pair's landmark keys, open-addressed: entry 2 k0 = "id0 of row k0", 2 k1 + 1 = "id k1 starts the
//                       pair with"; key and owning chain are recomputed from ids / k1_of, which the classification phase
//                       does not write.
// Within a pair a row reads and writes id[c0][k0] (its own), id[c1][k1] (its chain's) and the view of its keys or of a
// landmark its chain created.  Chains whose key sets are disjoint therefore commute: each runs on the lane of its head, in
// ascending k0.  A key that two chains share marks both entangled; all rows of entangled chains run on one lane in
// ascending k0, which is the sequential loop restricted to them.  Nothing else couples rows, so the result is the loop's.
constexpr int kStereoEntangled = 0x40000000;

struct StereoInsertLds {
  int32_t *ids, *ov, *k1_of, *head, *state, *kh;
};

__device__ __forceinline__ uint32_t stereo_hash(int v, int log2_size) {
  return ((uint32_t)v * 0x9E3779B1u) >> (32 - log2_size);
}
__device__ __forceinline__ size_t stereo_row(const StereoInsertArgs& A, size_t m, int r) {  // r = p K + k0
  const int p = r / A.kp_cap, k0 = r - p * A.kp_cap;
  return ((size_t)p * (size_t)A.n_multiframes + m) * (size_t)A.kp_cap + (size_t)k0;
}
// the row that re-initialised landmark v, or -1
__device__ __forceinline__ int stereo_overlay_find(const StereoInsertArgs& A, const StereoInsertLds& S, int v) {
  const volatile int32_t* ov = S.ov;
  const uint32_t mask = (1u << A.ov_log2) - 1u;
  for (uint32_t s = stereo_hash(v, A.ov_log2);; s = (s + 1u) & mask) {
    const int r = ov[s];
    if (r < 0) return -1;
    const int p = r / A.kp_cap, k0 = r - p * A.kp_cap;
    if (S.ids[(int)A.pair_c0[p] * A.kp_cap + k0] == v) return r;
  }
}
__device__ __forceinline__ void stereo_overlay_insert(const StereoInsertArgs& A, const StereoInsertLds& S, int v, int r) {
  const uint32_t mask = (1u << A.ov_log2) - 1u;
  for (uint32_t s = stereo_hash(v, A.ov_log2);; s = (s + 1u) & mask)
    if (atomicCAS(&S.ov[s], -1, r) == -1) return;
}
// classification: key `key` belongs to chain `owner`; a second chain with the same key entangles both
__device__ __forceinline__ void stereo_key_insert(const StereoInsertArgs& A, const StereoInsertLds& S, int c0, int c1,
                                                  int ref, int key, int owner, int* any_entangled) {
  const uint32_t mask = (1u << A.kh_log2) - 1u;
  for (uint32_t s = stereo_hash(key, A.kh_log2);; s = (s + 1u) & mask) {
    const int old = atomicCAS(&S.kh[s], -1, ref);
    if (old == -1) return;
    const int okey = (old & 1) ? S.ids[c1 * A.kp_cap + (old >> 1)] : S.ids[c0 * A.kp_cap + (old >> 1)];
    if (okey != key) continue;
    const int oown = (old & 1) ? (old >> 1) : S.k1_of[old >> 1];
    if (oown != owner) {
      atomicOr(&S.state[oown], kStereoEntangled);
      atomicOr(&S.state[owner], kStereoEntangled);
      *any_entangled = 1;
    }
    return;
  }
}
// getLandmark(v).point of the multiframe's view
__device__ __forceinline__ void stereo_point(const StereoInsertArgs& A, const StereoInsertLds& S, size_t m, int v,
                                             double hp[4]) {
  int r = stereo_overlay_find(A, S, v);
  if (r < 0 && v >= A.n_landmarks) r = v - A.n_landmarks;  // the creating row's hp_W is the record
  const double* src = r >= 0 ? A.matches[stereo_row(A, m, r)].hp_W : A.hp_W + 4 * (size_t)v;
  hp[0] = src[0]; hp[1] = src[1]; hp[2] = src[2]; hp[3] = src[3];
}
// :2121-2122 / :2134-2135: the landmark re-projects into (m, c) within 4 px of keypoint k
template <bool kRT8>
__device__ bool stereo_observable(const StereoInsertArgs& A, const StereoInsertLds& S, size_t m, int c, int k, int v) {
  double hp[4], hp_C[4], head[3], proj[2];
  stereo_point(A, S, m, v, hp);
  pose_inverse_times(A.poses[m * (size_t)A.n_cams + (size_t)c], hp, hp_C);
  if (hp_C[3] < 0) {  // projectHomogeneous
    head[0] = -hp_C[0]; head[1] = -hp_C[1]; head[2] = -hp_C[2];
  } else {
    head[0] = hp_C[0]; head[1] = hp_C[1]; head[2] = hp_C[2];
  }
  const DeviceCamera cam = A.cameras[A.cam_slots[c]];
  if (cam::project<kRT8>(cam, A.w, A.h, head, proj) != 0) return false;
  const uint8_t* blk = A.blocks + ((size_t)m * (size_t)A.stride_m + (size_t)c * (size_t)A.stride_c) * A.block_bytes;
  const okvfe_keypoint kp = reinterpret_cast<const okvfe_keypoint*>(blk + A.o_kps)[k];
  const double dx = (double)kp.x - proj[0], dy = (double)kp.y - proj[1];
  return sqrt(dx * dx + dy * dy) < 4.0;  // a NaN norm adds nothing
}
// one matched row of pair p, = :2076-2141; cnt: {matched, created, re-initialised, observations}
template <bool kRT8>
__device__ void stereo_insert_row(const StereoInsertArgs& A, const StereoInsertLds& S, size_t m, int p, int c0, int c1,
                                  int k0, int k1, bool keyframe, int cnt[4]) {
  const size_t row = ((size_t)p * (size_t)A.n_multiframes + m) * (size_t)A.kp_cap + (size_t)k0;
  const int id0 = S.ids[c0 * A.kp_cap + k0], id1 = S.ids[c1 * A.kp_cap + k1];
  int action = 0, lm = -1;
  bool add0 = false, add1 = false;
  ++cnt[0];
  if (id0 >= 0 && id1 >= 0) {
    lm = id0;
    if (A.matches[row].initialisable != 0) {
      bool initialised = stereo_overlay_find(A, S, id0) >= 0;
      if (!initialised)
        initialised = id0 < A.n_landmarks ? A.initialised[id0] != 0
                                          : A.matches[stereo_row(A, m, id0 - A.n_landmarks)].initialisable != 0;
      if (!initialised) {  // setLandmark(id0, hps_W, true)
        stereo_overlay_insert(A, S, id0, p * A.kp_cap + k0);
        action |= 1;
        ++cnt[2];
      }
    }
  } else if (id1 >= 0) {
    lm = id1;
    add0 = true;
  } else if (id0 >= 0) {
    lm = id0;
    add1 = true;
  } else if (keyframe) {
    lm = A.n_landmarks + p * A.kp_cap + k0;  // addLandmark(hps_W, initialisable): the id names this row
    action |= 2;
    ++cnt[1];
    add0 = add1 = true;
  }
  if (add0 && stereo_observable<kRT8>(A, S, m, c0, k0, lm)) {
    S.ids[c0 * A.kp_cap + k0] = lm;
    action |= 4;
    ++cnt[3];
  }
  if (add1 && stereo_observable<kRT8>(A, S, m, c1, k1, lm)) {
    S.ids[c1 * A.kp_cap + k1] = lm;
    action |= 8;
    ++cnt[3];
  }
  if (A.action) A.action[row] = (uint8_t)action;
  if (A.lm) A.lm[row] = lm;
}

template <bool kRT8>
__global__ __launch_bounds__(256) void stereo_insert_kernel(const StereoInsertArgs A) {
  extern __shared__ int32_t stereo_lds[];
  __shared__ int s_count[kStereoInsertMaxCams], s_total[4], s_any_entangled;
  const int K = A.kp_cap, tid = threadIdx.x;
  const size_t m = blockIdx.x;
  StereoInsertLds S;
  S.ids = stereo_lds;
  S.ov = S.ids + A.n_cams * K;
  S.k1_of = S.ov + (1 << A.ov_log2);
  S.head = S.k1_of + K;
  S.state = S.head + K;
  S.kh = S.state + K;
  if (tid < A.n_cams) {
    const uint8_t* blk = A.blocks + (m * (size_t)A.stride_m + (size_t)tid * (size_t)A.stride_c) * A.block_bytes;
    s_count[tid] = min(max(*reinterpret_cast<const int32_t*>(blk + A.o_count), 0), K);
  }
  if (tid < 4) s_total[tid] = 0;
  for (int i = tid; i < (1 << A.ov_log2); i += 256) S.ov[i] = -1;
  __syncthreads();
  for (int c = 0; c < A.n_cams; ++c) {
    const int32_t* src = A.landmark + (m * (size_t)A.stride_m + (size_t)c * (size_t)A.stride_c) * (size_t)K;
    for (int k = tid; k < K; k += 256) {
      const int v = k < s_count[c] ? src[k] : -1;
      S.ids[c * K + k] = (v >= 0 && v < A.n_landmarks) ? v : -1;  // outside [-1, L): read as none
    }
  }
  const bool keyframe = A.as_keyframe ? A.as_keyframe[m] != 0 : true;
  int cnt[4] = {0, 0, 0, 0};
  for (int p = 0; p < A.n_pairs; ++p) {
    const int c0 = A.pair_c0[p], c1 = A.pair_c1[p];
    const int n0 = s_count[c0], n1 = s_count[c1];
    const okvfe_stereo_match* rows = A.matches + ((size_t)p * (size_t)A.n_multiframes + m) * (size_t)K;
    __syncthreads();  // the ids of the pair before (or the load above) are complete
    for (int k = tid; k < K; k += 256) {
      S.head[k] = INT_MAX;
      S.state[k] = 0;
      int k1 = -1;
      if (k < n0) {
        k1 = rows[k].k1;
        if (k1 < 0 || k1 >= n1) k1 = -1;
      }
      S.k1_of[k] = k1;
    }
    for (int i = tid; i < (1 << A.kh_log2); i += 256) S.kh[i] = -1;
    if (tid == 0) s_any_entangled = 0;
    __syncthreads();
    // classification: chain heads, chain lengths, key collisions
    for (int k0 = tid; k0 < n0; k0 += 256) {
      const int k1 = S.k1_of[k0];
      if (k1 < 0) continue;
      atomicMin(&S.head[k1], k0);
      atomicAdd(&S.state[k1], 1);
      const int id0 = S.ids[c0 * K + k0], id1 = S.ids[c1 * K + k1];
      if (id0 >= 0) stereo_key_insert(A, S, c0, c1, k0 << 1, id0, k1, &s_any_entangled);
      if (id1 >= 0) stereo_key_insert(A, S, c0, c1, (k1 << 1) | 1, id1, k1, &s_any_entangled);
    }
    __syncthreads();
    // resolution: one lane per free chain; in the extra last round lane 255 takes the rows of all entangled chains
    const int rounds = (n0 + 255) / 256 + 1;
    for (int it = 0; it < rounds; ++it) {
      const bool serial = it == rounds - 1;
      int start = 0, left = 0, chain = -1;
      if (!serial) {
        const int k0 = it * 256 + tid;
        if (k0 < n0) {
          const int k1 = S.k1_of[k0];
          if (k1 < 0) {
            const size_t row = ((size_t)p * (size_t)A.n_multiframes + m) * (size_t)K + (size_t)k0;
            if (A.action) A.action[row] = 0;
            if (A.lm) A.lm[row] = -1;
          } else {
            const int st = S.state[k1];
            if (!(st & kStereoEntangled) && S.head[k1] == k0) {
              start = k0;
              left = st;
              chain = k1;
            }
          }
        }
      } else if (tid == 255 && s_any_entangled) {
        left = INT_MAX;
      }
      for (int j = start; left > 0 && j < n0; ++j) {
        const int k1 = S.k1_of[j];
        const bool mine = serial ? (k1 >= 0 && (S.state[k1] & kStereoEntangled)) : k1 == chain;
        if (!mine) continue;
        stereo_insert_row<kRT8>(A, S, m, p, c0, c1, j, k1, keyframe, cnt);
        if (!serial) --left;
      }
    }
  }
  for (int i = 0; i < 4; ++i)
    if (cnt[i]) atomicAdd(&s_total[i], cnt[i]);
  __syncthreads();
  for (int c = 0; c < A.n_cams; ++c) {
    int32_t* dst = A.landmark_out + (m * (size_t)A.stride_m + (size_t)c * (size_t)A.stride_c) * (size_t)K;
    for (int k = tid; k < s_count[c]; k += 256) dst[k] = S.ids[c * K + k];
  }
  if (tid < 4) A.counts[4 * m + tid] = s_total[tid];
}
