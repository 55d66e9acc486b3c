// k_ransac_hyp.hip -- the pose hypotheses of the absolute-pose RANSAC for a batch of multiframes: what the caller of
// okvfe_ransac3d2d_consensus_blocks_device / okvfe_place_consensus_blocks_device used to compute on the host between
// two queued calls.  The algorithm (sampler, Grunert's P3P, the choice by the fourth sample) is ransac_hyp_dev.h, the
// correspondences, the inverse of a hypothesis and the distance are the consensus kernel's own: this file is included at
// the end of k_ransac.hip (it is no translation unit of its own), so that each of them exists once.
//   ransac_hypotheses_kernel   one work-group of 256 per multiframe.
//     phase 1  all lanes test keypoint slots with make_correspondence; ballot + prefix count build the camera-major
//              list of slots c K + k in LDS (4 bytes per keypoint slot), then the first list position of every camera.
//     phase 2  hypothesis h belongs to lane (h & 15) of wave (h >> 4): 16 hypotheses per wave, so that the FP64 chains
//              of up to 64 hypotheses issue from all four SIMDs.  The lane draws its four positions, rebuilds the four
//              correspondences from the list, runs the solver and stores 12 doubles and the byte.
// Trip counts (doublings, bisection steps) depend on the data: the lanes of a wave diverge, bounded by
// kHypMaxDoublings + kHypMaxBisections.  FP64, no FMA; the sums of the consensus' functions in the order of
// okvfe_set_fp64_reduction (a template argument).
#include "ransac_hyp_dev.h"

namespace okvfe {
namespace {

constexpr int kHypThreads = 256;
constexpr int kHypWaves = kHypThreads / 64;
constexpr int kHypPerWave = OKVFE_RANSAC_MAX_HYPOTHESES / kHypWaves;  // 16
constexpr size_t kHypMaxLds = 60 * 1024;  // the index list and the camera ranges (dynamic LDS, below the 64 KiB default)

struct HypArgs {
  RansacArgs A;             // what make_correspondence reads (table, blocks, layout, rig, landmark rows, gate)
  const uint64_t* keys;     // per multiframe or NULL (the multiframe's index)
  uint64_t seed;
  int n_hyp;
  double* hyp;              // n x n_hyp x 12
  uint8_t* valid;           // n x n_hyp
  int32_t* n_corr;          // optional
  int32_t* samples;         // optional, n x n_hyp x 4
  int32_t* n_solutions;     // optional
};

// the distance of sample 3 under a solution: the consensus' own functions (k_ransac.hip), host and device
template <bool kTree>
struct ConsensusDistance {
  __host__ __device__ double operator()(const double* H, const double* p, const double* C_SC, const double* r_SC,
                                        const double* b, double sigma) const {
    double inv[12];
    invert_hypothesis<kTree>(H, inv);
    return ransac_distance<kTree>(inv, p, C_SC, r_SC, b, sigma);
  }
};

struct CameraRange {
  const int* list;
  const int* first;  // n_cams + 1 list positions
  int K;
  __host__ __device__ void operator()(int i, int* b, int* e) const {
    const int c = list[i] / K;
    *b = first[c];
    *e = first[c + 1];
  }
};

template <bool kTree, bool kPlace>
__global__ __launch_bounds__(kHypThreads) void ransac_hypotheses_kernel(HypArgs G) {
  extern __shared__ int s_dyn[];  // [slots] the list, [n_cams + 1] the first position of every camera
  __shared__ int s_wave[kHypWaves];
  const RansacArgs& A = G.A;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.kp_cap, slots = A.n_cams * K;
  int* s_list = s_dyn;
  int* s_first = s_dyn + slots;
  const size_t frame0 = (size_t)m * (size_t)A.n_cams;
  const bool gated = kPlace && A.gate && A.gate[m] == 0;

  // phase 1: the correspondences in the adapter's order (camera-major, keypoints ascending), a tile of slots at a time
  int head = 0;  // uniform
  for (int base = 0; base < slots; base += kHypThreads) {
    const int s = base + tid;
    bool take = false;
    if (s < slots) {
      const int c = s / K, k = s - c * K;
      const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
      int count = *reinterpret_cast<const int32_t*>(blk + A.o_count);
      count = count < 0 ? 0 : (count > K ? K : count);
      Corr R;
      if (k < count) take = make_correspondence<kTree, kPlace>(A, blk, c, k, A.landmark[(frame0 + c) * K + k], R);
    }
    const unsigned long long bal = __ballot(take);
    if (lane == 0) s_wave[wave] = (int)__popcll(bal);
    __syncthreads();
    int pos = head + (int)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < kHypWaves; ++w) {
      pos += w < wave ? s_wave[w] : 0;
      head += s_wave[w];
    }
    if (take) s_list[pos] = s;  // pos < slots: at most one entry per slot
    __syncthreads();
  }
  const int n = head;
  // the first list position of every camera: the lower bound of c K in the ascending list
  for (int c = tid; c <= A.n_cams; c += kHypThreads) {
    int lo = 0, hi = n;
    const int want = c * K;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_list[mid] < want) lo = mid + 1; else hi = mid;
    }
    s_first[c] = lo;
  }
  __syncthreads();
  if (tid == 0 && G.n_corr) G.n_corr[m] = n;

  // phase 2: one hypothesis per lane, 16 lanes of every wave
  const int h = wave * kHypPerWave + lane;
  if (lane >= kHypPerWave || h >= G.n_hyp) return;
  const size_t row = (size_t)m * (size_t)G.n_hyp + (size_t)h;
  double H[12];
  for (int i = 0; i < 12; ++i) H[i] = 0.0;
  int pos[4] = {-1, -1, -1, -1}, slot[4] = {-1, -1, -1, -1};
  int n_sol = 0;
  bool valid = false;
  if (!gated) {
    const uint64_t key = G.keys ? G.keys[m] : (uint64_t)m;
    const int drawn = hyp_sample(G.seed, key, h, n, CameraRange{s_list, s_first, K}, pos);
    for (int j = 0; j < 4; ++j)
      if (pos[j] >= 0) slot[j] = s_list[pos[j]];
    if (drawn == 4) {
      const int c = slot[0] / K;
      const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
      double P[12], f[12], sigma3 = 0.0;
      for (int j = 0; j < 4; ++j) {
        const int k = slot[j] - c * K;
        Corr R;
        make_correspondence<kTree, kPlace>(A, blk, c, k, A.landmark[(frame0 + c) * K + k], R);  // true: it is in the list
        for (int i = 0; i < 3; ++i) {
          P[3 * j + i] = R.p[i];
          f[3 * j + i] = R.b[i];
        }
        sigma3 = R.sigma;
      }
      const RansacCamParams& cp = A.cams[c];
      valid = p3p_hypothesis(P, f, sigma3, cp.C, cp.r, H, &n_sol, ConsensusDistance<kTree>{});
    }
  }
  double* out = G.hyp + 12 * row;
  for (int i = 0; i < 12; ++i) out[i] = H[i];
  G.valid[row] = valid ? 1 : 0;
  if (G.samples)
    for (int j = 0; j < 4; ++j) G.samples[4 * row + j] = slot[j];
  if (G.n_solutions) G.n_solutions[row] = n_sol;
}

HypArgs hyp_args(const double* hp, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L, const uint8_t* blocks,
                 int n_cams, int kp_cap, const RansacCamParams* cams, const int32_t* landmark, const uint8_t* gate,
                 const uint64_t* keys, uint64_t seed, int n_hyp, const okvfe_ransac_hypotheses_device& out) {
  HypArgs G{};
  RansacArgs& A = G.A;
  A.hp_W = hp; A.obs_begin = obs_begin; A.n_landmarks = n_landmarks;
  A.blocks = blocks; A.o_count = (int)L.o_count; A.o_kps = (int)L.o_kps; A.o_bp = (int)L.o_bp; A.o_bpv = (int)L.o_bpv;
  A.block_bytes = L.total; A.kp_cap = kp_cap; A.n_cams = n_cams; A.cams = cams;
  A.landmark = landmark; A.gate = gate;
  G.keys = keys; G.seed = seed; G.n_hyp = n_hyp;
  G.hyp = out.hypotheses; G.valid = out.hyp_valid; G.n_corr = out.n_correspondences; G.samples = out.samples;
  G.n_solutions = out.n_solutions;
  return G;
}

}  // namespace

// okvfe_p3p_hypothesis: the header's solver with the same distance, on the host
bool p3p_hypothesis_host(bool tree, const double* points, const double* bearings, double sigma, const double* C_SC,
                         const double* r_SC, double* hypothesis, int* n_solutions) {
  return tree ? p3p_hypothesis(points, bearings, sigma, C_SC, r_SC, hypothesis, n_solutions, ConsensusDistance<true>{})
              : p3p_hypothesis(points, bearings, sigma, C_SC, r_SC, hypothesis, n_solutions, ConsensusDistance<false>{});
}

size_t ransac_hypotheses_lds_bytes(int n_cams, int kp_cap) {
  return ((size_t)n_cams * (size_t)kp_cap + (size_t)n_cams + 1) * sizeof(int);
}
bool ransac_hypotheses_fits(int n_cams, int kp_cap) { return ransac_hypotheses_lds_bytes(n_cams, kp_cap) <= kHypMaxLds; }

void launch_ransac_hypotheses(const double* hp_W, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L,
                              const uint8_t* blocks, int n_multiframes, int n_cams, int kp_cap, const RansacCamParams* cams,
                              const int32_t* landmark, const uint64_t* keys, uint64_t seed, int n_hyp,
                              const okvfe_ransac_hypotheses_device& out, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  const HypArgs G = hyp_args(hp_W, obs_begin, n_landmarks, L, blocks, n_cams, kp_cap, cams, landmark, nullptr, keys, seed,
                             n_hyp, out);
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac_hypotheses_kernel<false, false> : ransac_hypotheses_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kHypThreads), ransac_hypotheses_lds_bytes(n_cams, kp_cap), stream, G);
}

void launch_place_hypotheses(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks,
                             int n_multiframes, int n_cams, int kp_cap, const RansacCamParams* cams,
                             const int32_t* match_landmark, const uint8_t* gate, const uint64_t* keys, uint64_t seed,
                             int n_hyp, const okvfe_ransac_hypotheses_device& out, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  const HypArgs G = hyp_args(hp, nullptr, n_landmarks, L, blocks, n_cams, kp_cap, cams, match_landmark, gate, keys, seed,
                             n_hyp, out);
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac_hypotheses_kernel<false, true> : ransac_hypotheses_kernel<true, true>;
  hipLaunchKernelGGL(kernel, dim3(n_multiframes), dim3(kHypThreads), ransac_hypotheses_lds_bytes(n_cams, kp_cap), stream, G);
}

}  // namespace okvfe
