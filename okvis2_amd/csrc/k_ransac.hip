// k_ransac.hip -- the consensus step of Frontend::runRansac3d2d (okvis_frontend/src/Frontend.cpp:2208-2261) for a
// batch of multiframes: the correspondences of FrameNoncentralAbsoluteAdapter (FrameNoncentralAbsoluteAdapter.cpp:
// 50-148), the distance of every correspondence to every pose hypothesis (FrameAbsolutePoseSacProblem.hpp:135-167),
// the winner, the acceptance rule and the outlier removal.  The hypotheses: the caller's, or those of k_ransac_hyp.hip.
// The same kernel under the policy kPlace is the consensus of Frontend::verifyRecognisedPlace (Frontend.cpp:372-397)
// over the correspondences of LoopclosureNoncentralAbsoluteAdapter (LoopclosureNoncentralAbsoluteAdapter.cpp:69-154):
// the rows are those of the old frame's landmark set, there is no test on observations, seven correspondences are the
// floor (:380) and the verdict is :389.
//   ransac_consensus_kernel   one work-group per multiframe.  The correspondences are compacted, in the adapter's
//                             order, into an LDS ring of 64-byte records and scored kRansacChunk at a time: a lane
//                             keeps one record (and its camera's extrinsics) in registers and walks the inverted
//                             hypotheses, which sit in LDS; a wave's inliers of a hypothesis are a ballot + popcount.
//                             A final sweep over the keypoints with the winner writes state / distance / landmark_out.
// FP64, 3- and 4-term sums (fp64_ops.h) in the order of okvfe_set_fp64_reduction (a template argument: the host launches
// the kernel compiled for the order in force, fp64_left_to_right(); no selects in the scoring loop), no FMA.
// The inverse of a hypothesis and the distance also compile for the host: the choice among the solutions of a
// P3P sample (k_ransac_hyp.hip, included at the end of this file so that it uses these copies) runs there as well.
#include "fp64_ops.h"
#include "okvfe_internal.h"

namespace okvfe {
namespace {

constexpr int kRansacThreads = 256;
constexpr int kRansacChunk = kRansacThreads;    // records scored at a time: one per lane
constexpr int kRansacRing = 2 * kRansacChunk;   // a tile of keypoints adds at most a chunk to less than a chunk
constexpr int kRansacWaves = kRansacThreads / 64;
static_assert((kRansacRing & (kRansacRing - 1)) == 0, "ring positions are masked");

// one correspondence of the adapter
struct Corr {
  double p[3];  // hp.head<3>() / hp[3]
  double b[3];  // normalised bearing
  double sigma;
  int32_t cam;  // camera index inside the multiframe
  int32_t row;  // keypoint row
};
static_assert(sizeof(Corr) == 64, "64-byte LDS records");

struct RansacArgs {
  const double* hp_W;
  const int32_t* obs_begin;
  int n_landmarks;
  const uint8_t* blocks;
  int o_count, o_kps, o_bp, o_bpv;
  size_t block_bytes;
  int kp_cap, n_cams;
  const RansacCamParams* cams;
  const int32_t* landmark;  // may alias landmark_out
  const double* hyp;
  const uint8_t* hyp_valid;
  int n_hyp;
  double threshold;
  int remove_outliers;
  int32_t *n_corr, *best, *n_inl;
  uint8_t* accepted;
  int32_t* hyp_inliers;
  uint8_t* state;
  double* distance;
  int32_t* landmark_out;
  // kPlace only (at the end: the members above keep their offsets)
  const uint8_t* gate;  // per multiframe or NULL: 0 = Frontend.cpp:359 returned false
  uint8_t* verdict;
  int min_inliers;
};

// FrameNoncentralAbsoluteAdapter.cpp:101-145 for keypoint k (< count) of one block that carries table row l: false =
// no correspondence.  A row outside the table is no correspondence either.  kPlace: the same lines of
// LoopclosureNoncentralAbsoluteAdapter.cpp (:112-150), which has no test on the observations.
template <bool kTree, bool kPlace>
__device__ __forceinline__ bool make_correspondence(const RansacArgs& A, const uint8_t* blk, int c, int k, int l,
                                                    Corr& R) {
  if (l < 0 || l >= A.n_landmarks) return false;                 // :105
  if constexpr (!kPlace)
    if (A.obs_begin[l + 1] - A.obs_begin[l] < 1) return false;   // :109, without the observation of this frame
  const double* hp = A.hp_W + 4 * (size_t)l;
  const double w = hp[3];
  if (fabs(w) < 1.0e-8) return false;                            // :116 (a NaN stays in)
  R.p[0] = hp[0] / w;
  R.p[1] = hp[1] / w;
  R.p[2] = hp[2] / w;                                            // :120
  const float size = reinterpret_cast<const okvfe_keypoint*>(blk + A.o_kps)[k].size;
  const double s = (0.8 * (double)size) / 12.0;                  // :128
  double v[3] = {1.0, 0.0, 0.0};                                 // :129-132
  if (blk[A.o_bpv + k]) {
    const double* bp = reinterpret_cast<const double*>(blk + A.o_bp) + 3 * (size_t)k;
    v[0] = bp[0]; v[1] = bp[1]; v[2] = bp[2];
  }
  const double fu = A.cams[c].fu;
  const double sqrt2 = __longlong_as_double(0x3FF6A09E667F3BCDLL);
  R.sigma = ((sqrt2 * s) * s) / (fu * fu);                       // :135
  const double z = fp64::sum3<kTree>(v[0] * v[0], v[1] * v[1], v[2] * v[2]);  // :137, Eigen's normalize()
  if (z > 0) {
    const double n = sqrt(z);
    v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
  }
  R.b[0] = v[0]; R.b[1] = v[1]; R.b[2] = v[2];
  R.cam = c;
  R.row = k;
  return true;
}

// FrameAbsolutePoseSacProblem.hpp:142-143: inv[0..8] = R^T row-major, inv[9..11] = (-R^T) t
template <bool kTree>
__host__ __device__ __forceinline__ void invert_hypothesis(const double* H /* 3 x 4 row-major */, double* inv) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) inv[3 * i + j] = H[4 * j + i];
  for (int i = 0; i < 3; ++i)
    inv[9 + i] = fp64::sum3<kTree>((-inv[3 * i]) * H[3], (-inv[3 * i + 1]) * H[7], (-inv[3 * i + 2]) * H[11]);
}

// FrameAbsolutePoseSacProblem.hpp:151-165.  The ONE copy of the distance: the scoring loop and the final sweep call it.
template <bool kTree>
__host__ __device__ __forceinline__ double ransac_distance(const double* inv, const double p[3], const double C_SC[9],
                                                           const double r_SC[3], const double b[3], double sigma) {
  double d[3], rep[3], e[3];
  for (int i = 0; i < 3; ++i) {
    const double body = fp64::sum4<kTree>(inv[3 * i] * p[0], inv[3 * i + 1] * p[1], inv[3 * i + 2] * p[2], inv[9 + i] * 1.0);
    d[i] = body - r_SC[i];
  }
  for (int i = 0; i < 3; ++i) rep[i] = fp64::sum3<kTree>(C_SC[i] * d[0], C_SC[3 + i] * d[1], C_SC[6 + i] * d[2]);
  const double n = sqrt(fp64::sum3<kTree>(rep[0] * rep[0], rep[1] * rep[1], rep[2] * rep[2]));
  for (int i = 0; i < 3; ++i) e[i] = rep[i] / n - b[i];
  return fp64::sum3<kTree>(e[0] * e[0], e[1] * e[1], e[2] * e[2]) / sigma;
}

template <bool kTree, bool kPlace>
__global__ __launch_bounds__(kRansacThreads) void ransac_consensus_kernel(RansacArgs A) {
  __shared__ Corr s_rec[kRansacRing];               // 32 KiB
  __shared__ double s_inv[OKVFE_RANSAC_MAX_HYPOTHESES][12];  // 6 KiB
  __shared__ int s_cnt[OKVFE_RANSAC_MAX_HYPOTHESES];
  __shared__ int s_valid[OKVFE_RANSAC_MAX_HYPOTHESES];
  __shared__ int s_wave[kRansacWaves];
  __shared__ int s_best, s_accepted;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.kp_cap, slots = A.n_cams * K;
  const size_t frame0 = (size_t)m * (size_t)A.n_cams;
  // kPlace: the caller's gate 0 (Frontend.cpp:359 returned false before the adapter existed): nothing is scored
  const bool gated = kPlace && A.gate && A.gate[m] == 0;
  constexpr int kMinCorr = kPlace ? 7 : 10;  // Frontend.cpp:380 : Frontend.cpp:2226

  if (tid < A.n_hyp) {
    const size_t h = (size_t)m * (size_t)A.n_hyp + (size_t)tid;
    invert_hypothesis<kTree>(A.hyp + 12 * h, s_inv[tid]);
    s_cnt[tid] = 0;
    s_valid[tid] = A.hyp_valid ? (A.hyp_valid[h] != 0) : 1;
  }
  __syncthreads();

  // scores the records [tail, tail + n) of the ring, n <= kRansacChunk
  auto score = [&](int tail, int n) {
    const bool have = tid < n;
    const Corr R = s_rec[(tail + (have ? tid : 0)) & (kRansacRing - 1)];
    const RansacCamParams P = A.cams[have ? R.cam : 0];
    for (int h = 0; h < A.n_hyp; ++h) {
      if (!s_valid[h]) continue;  // opengv skips a sample whose solver failed
      const double d = ransac_distance<kTree>(s_inv[h], R.p, P.C, P.r, R.b, R.sigma);
      const unsigned long long in = __ballot(have && d < A.threshold);  // a NaN is an outlier
      if (lane == 0 && in) atomicAdd(&s_cnt[h], (int)__popcll(in));
    }
  };

  // the correspondences in the adapter's order (camera-major, keypoints ascending), a tile of keypoints at a time
  int head = 0, tail = 0;  // uniform: records compacted / records scored
  for (int base = 0; base < slots; base += kRansacThreads) {
    const int s = base + tid;
    bool take = false;
    Corr R;
    if (s < slots) {
      const int c = s / K, k = s - c * K;
      const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
      int count = *reinterpret_cast<const int32_t*>(blk + A.o_count);
      count = count < 0 ? 0 : (count > K ? K : count);
      if (k < count) take = make_correspondence<kTree, kPlace>(A, blk, c, k, A.landmark[(frame0 + c) * K + k], R);
    }
    const unsigned long long bal = __ballot(take);
    if (lane == 0) s_wave[wave] = (int)__popcll(bal);
    __syncthreads();  // (also: every lane has loaded its record of the chunk scored in the last round)
    int pos = head + (int)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < kRansacWaves; ++w) {
      pos += w < wave ? s_wave[w] : 0;
      head += s_wave[w];
    }
    if (take) s_rec[pos & (kRansacRing - 1)] = R;
    __syncthreads();
    if (head - tail >= kRansacChunk) {
      if (!gated) score(tail, kRansacChunk);
      tail += kRansacChunk;
    }
  }
  const int n_corr = head;
  const bool scored = !gated && n_corr >= kMinCorr;
  if (scored && head > tail) score(tail, head - tail);
  __syncthreads();

  // opengv's Ransac::computeModel replaces its best model only on strictly more inliers, from zero
  if (tid == 0) {
    int best = -1, most = 0;
    if (scored)
      for (int h = 0; h < A.n_hyp; ++h)
        if (s_valid[h] && s_cnt[h] > most) {
          most = s_cnt[h];
          best = h;
        }
    int acc;
    if constexpr (kPlace) {
      // Frontend.cpp:389: a ratio of exactly 0.7 passes here (and not at :2243)
      const int v = gated ? 0 : !scored ? 1 : (most < A.min_inliers || (double)most / (double)n_corr < 0.7) ? 2 : 3;
      A.verdict[m] = (uint8_t)v;
      acc = v == 3;
    } else {
      acc = most >= 10 && (double)most / (double)n_corr > 0.7;  // Frontend.cpp:2243
    }
    A.n_corr[m] = n_corr;
    A.best[m] = best;
    A.n_inl[m] = most;
    A.accepted[m] = (uint8_t)acc;
    s_best = best;
    s_accepted = acc;
  }
  if (A.hyp_inliers && tid < A.n_hyp)
    A.hyp_inliers[(size_t)m * (size_t)A.n_hyp + tid] = scored && s_valid[tid] ? s_cnt[tid] : -1;
  __syncthreads();
  if (!A.state && !A.distance && !A.landmark_out) return;

  // the final sweep: every keypoint below its block's count against the winner
  const int best = s_best;
  const bool remove = s_accepted && A.remove_outliers;  // Frontend.cpp:2245-2260 (kPlace: the inlier flags of :393-397)
  for (int s = tid; s < slots; s += kRansacThreads) {
    const int c = s / K, k = s - c * K;
    const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
    int count = *reinterpret_cast<const int32_t*>(blk + A.o_count);
    count = count < 0 ? 0 : (count > K ? K : count);
    if (k >= count) continue;
    const size_t row = (frame0 + c) * K + k;
    const int l = A.landmark[row];
    Corr R;
    int st = 0;
    if (make_correspondence<kTree, kPlace>(A, blk, c, k, l, R)) {
      st = 1;
      if (best >= 0) {
        const RansacCamParams P = A.cams[c];
        const double d = ransac_distance<kTree>(s_inv[best], R.p, P.C, P.r, R.b, R.sigma);
        if (d < A.threshold) st = 2;
        if (A.distance) A.distance[row] = d;
      }
    }
    if (A.state) A.state[row] = (uint8_t)st;
    if (A.landmark_out) A.landmark_out[row] = remove && st == 1 ? -1 : l;
  }
}

}  // namespace

namespace {
RansacArgs ransac_args(const double* hp_W, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L,
                       const uint8_t* blocks, int n_cams, int kp_cap, const RansacCamParams* cams, const int32_t* landmark,
                       const double* hypotheses, const uint8_t* hyp_valid, int n_hyp, double threshold, int remove_outliers,
                       const okvfe_ransac_result_device& out) {
  RansacArgs A;
  A.hp_W = hp_W; A.obs_begin = obs_begin; A.n_landmarks = n_landmarks;
  A.blocks = blocks; A.o_count = (int)L.o_count; A.o_kps = (int)L.o_kps; A.o_bp = (int)L.o_bp; A.o_bpv = (int)L.o_bpv;
  A.block_bytes = L.total; A.kp_cap = kp_cap; A.n_cams = n_cams; A.cams = cams;
  A.landmark = landmark; A.hyp = hypotheses; A.hyp_valid = hyp_valid; A.n_hyp = n_hyp;
  A.threshold = threshold; A.remove_outliers = remove_outliers;
  A.n_corr = out.n_correspondences; A.best = out.best_hypothesis; A.n_inl = out.n_inliers; A.accepted = out.accepted;
  A.hyp_inliers = out.hyp_inliers; A.state = out.state; A.distance = out.distance; A.landmark_out = out.landmark_out;
  A.gate = nullptr; A.verdict = nullptr; A.min_inliers = 0;
  return A;
}
}  // namespace

void launch_ransac_consensus(const double* hp_W, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L,
                             const uint8_t* blocks, int n_multiframes, int n_cams, int kp_cap,
                             const RansacCamParams* cams, const int32_t* landmark, const double* hypotheses,
                             const uint8_t* hyp_valid, int n_hyp, double threshold, int remove_outliers,
                             const okvfe_ransac_result_device& out, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  const RansacArgs A = ransac_args(hp_W, obs_begin, n_landmarks, L, blocks, n_cams, kp_cap, cams, landmark, hypotheses,
                                   hyp_valid, n_hyp, threshold, remove_outliers, out);
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac_consensus_kernel<false, false> : ransac_consensus_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kRansacThreads), 0, stream, A);
}

void launch_place_consensus(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks, int n_multiframes,
                            int n_cams, int kp_cap, const RansacCamParams* cams, const int32_t* match_landmark,
                            const uint8_t* gate, const double* hypotheses, const uint8_t* hyp_valid, int n_hyp,
                            double threshold, int min_inliers, const okvfe_ransac_result_device& out, uint8_t* verdict,
                            hipStream_t stream) {
  if (n_multiframes <= 0) return;
  RansacArgs A = ransac_args(hp, nullptr, n_landmarks, L, blocks, n_cams, kp_cap, cams, match_landmark, hypotheses,
                             hyp_valid, n_hyp, threshold, 1, out);
  A.gate = gate; A.verdict = verdict; A.min_inliers = min_inliers;
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac_consensus_kernel<false, true> : ransac_consensus_kernel<true, true>;
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kRansacThreads), 0, stream, A);
}

int ransac_chunk_records() { return kRansacChunk; }
int ransac_ring_records() { return kRansacRing; }

}  // namespace okvfe

// the pose hypotheses of both policies: their kernel uses make_correspondence, invert_hypothesis and ransac_distance above
#include "k_ransac_hyp.hip"
