// k_ransac2d2d_hyp.hip -- the hypotheses of runRansac2d2d for a batch of (older, current) multiframe pairs: what the
// caller of okvfe_ransac2d2d_consensus_blocks_device used to compute on the host between two queued calls.  The algorithm
// (sampler, rotation from two triads, Nister's five-point, the choice by samples 5 .. 7) is ransac2d2d_hyp_dev.h; the id
// table, the correspondences and the distances are the consensus kernel's own: this file is included at the end of
// k_ransac2d2d.hip (it is no translation unit of its own), so that each of them exists once.
//   ransac2d2d_hypotheses_kernel   one work-group of 256 per (pair, camera): the cameras of a pair share nothing here.
//     phase 1  the id table of the current block (id_insert), then the older keypoints look their ids up a tile at a
//              time; ballot + prefix count compact the hits, in older-keypoint order, into an LDS list of kA | kB << 12
//              (4 bytes per older keypoint slot; K <= 4095).
//     phase 2  rotation only: lane h of the work-group draws two positions and solves in registers.  Relative pose:
//              the 10 x 20 system of a solve does not fit a lane's registers, so every solving lane owns
//              kHyp2Stride doubles of LDS (the solver's work arrays and the eight bearing pairs), laid over the id
//              table, which is dead by then.  kHyp2Solvers lanes solve at a time, eight of every wave so that the FP64
//              chains issue from all four SIMDs; hypotheses beyond that take further rounds.  A lane's arrays are its
//              own: the rounds need no barrier.
// Trip counts (roots, bisection steps) depend on the data: the lanes of a wave diverge, every loop is capped.  FP64, no
// FMA; the sums of the consensus' functions in the order of okvfe_set_fp64_reduction (a template argument), the sums
// of the solver left to right.
#include "ransac2d2d_hyp_dev.h"

namespace okvfe {
namespace {

constexpr int kHyp2Threads = 256;
constexpr int kHyp2Waves = kHyp2Threads / 64;
constexpr int kHyp2PerWave = 8;
constexpr int kHyp2Solvers = kHyp2Waves * kHyp2PerWave;  // 32 solves at a time: 50 hypotheses are two rounds
constexpr int kHyp2B1 = kFiveptWork, kHyp2B2 = kFiveptWork + 24, kHyp2S1 = kFiveptWork + 48, kHyp2S2 = kFiveptWork + 51;
constexpr int kHyp2Stride = kFiveptWork + 55;  // odd: the lanes' arrays start in different banks
static_assert(kHyp2Stride >= kFiveptWork + 54 && (kHyp2Stride & 1) == 1, "work arrays + 8 bearing pairs + 6 sigmas");
static_assert((size_t)kHyp2Solvers * kHyp2Stride * sizeof(double) >= (size_t)kRansac2Slots * sizeof(int),
              "the id table lies under the work arrays");
static_assert(kRansac2dMaxKeypoints < (1 << 12), "kA | kB << 12");

struct Hyp2Args {
  Ransac2d2dArgs A;      // what the id table and make_correspondence2 read (blocks, layout, pairs, fu, id rows, added)
  const uint64_t* keys;  // per pair or NULL (the pair's index)
  uint64_t seed;
  okvfe_ransac2d2d_hypotheses_device out;
};

// the sum of the consensus' distance over samples 5 .. 7 under [R | t] = H: its own functions, host and device
template <bool kTree>
struct RelativeSum {
  __host__ __device__ double operator()(const double* H, const double* b1, const double* b2, const double* s1,
                                        const double* s2) const {
    double ti[3], d[3];
    inverse_translation<kTree>(H, ti);
    for (int j = 0; j < 3; ++j) {
      Corr2 R;
      for (int i = 0; i < 3; ++i) {
        R.b1[i] = b1[3 * j + i];
        R.b2[i] = b2[3 * j + i];
      }
      R.s1 = s1[j];
      R.s2 = s2[j];
      d[j] = relative_pose_distance<kTree>(H, ti, R);
    }
    return (d[0] + d[1]) + d[2];
  }
};

template <bool kTree>
__global__ __launch_bounds__(kHyp2Threads) void ransac2d2d_hypotheses_kernel(Hyp2Args G) {
  __shared__ double s_work[kHyp2Solvers * kHyp2Stride];  // phase 1: the id table; phase 2: the solvers' arrays
  __shared__ int s_list[kRansac2Slots];                  // kA | kB << 12, in older-keypoint order
  __shared__ int s_wave[kHyp2Waves];
  int* s_tab = reinterpret_cast<int*>(s_work);
  const Ransac2d2dArgs& A = G.A;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = blockIdx.x / A.n_cams, c = blockIdx.x - p * A.n_cams;
  const int K = A.kp_cap, n_hyp = A.n_hyp;
  const size_t frame0 = (size_t)A.pairs[2 * p] * (size_t)A.n_cams, frame1 = (size_t)A.pairs[2 * p + 1] * (size_t)A.n_cams;
  const size_t pc = (size_t)p * (size_t)A.n_cams + (size_t)c;
  const uint8_t* blk0 = A.blocks0 + (frame0 + c) * A.block_bytes;
  const uint8_t* blk1 = A.blocks1 + (frame1 + c) * A.block_bytes;
  int count0 = *reinterpret_cast<const int32_t*>(blk0 + A.o_count);
  int count1 = *reinterpret_cast<const int32_t*>(blk1 + A.o_count);
  count0 = count0 < 0 ? 0 : (count0 > K ? K : count0);
  count1 = count1 < 0 ? 0 : (count1 > K ? K : count1);
  const int32_t* lm0 = A.landmark0 + (frame0 + c) * K;
  const int32_t* lm1 = A.landmark1 + (frame1 + c) * K;
  const double fu = A.fu[c];

  // phase 1: the adapter's list (FrameRelativeAdapter.cpp:139-165)
  for (int s = tid; s < kRansac2Slots; s += kHyp2Threads) s_tab[s] = -1;
  __syncthreads();
  for (int k = tid; k < count1; k += kHyp2Threads) id_insert(A, s_tab, lm1, k);
  __syncthreads();
  int head = 0;  // uniform
  for (int base = 0; base < count0; base += kHyp2Threads) {
    const int k = base + tid;
    int kB = -1;
    if (k < count0) {
      const int id = lm0[k];
      if (id >= 0) kB = id_lookup(s_tab, lm1, id);
    }
    const bool take = kB >= 0;
    const unsigned long long bal = __ballot(take);
    if (lane == 0) s_wave[wave] = (int)__popcll(bal);
    __syncthreads();
    int pos = head + (int)__popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < kHyp2Waves; ++w) {
      pos += w < wave ? s_wave[w] : 0;
      head += s_wave[w];
    }
    if (take) s_list[pos] = k | (kB << 12);  // pos < count0 <= K: at most one entry per older keypoint
    __syncthreads();
  }
  const int n = head;
  const bool solve = n >= kHyp2MinCorrespondences;  // Frontend.cpp:2300: the camera is skipped, nothing is drawn
  if (tid == 0 && G.out.n_correspondences) G.out.n_correspondences[pc] = n;
  const uint64_t pair_key = G.keys ? G.keys[p] : (uint64_t)p;
  // (the last barrier of phase 1 lies behind every lookup: the table may be overwritten from here on)

  // phase 2, rotation only: hypothesis tid
  if (tid < n_hyp) {
    const size_t row = pc * (size_t)n_hyp + (size_t)tid;
    double M[9];
    for (int i = 0; i < 9; ++i) M[i] = 0.0;
    int kA[kHyp2RotSamples] = {-1, -1};
    bool valid = false;
    if (solve) {
      int pos[kHyp2RotSamples];
      hyp2_sample<kHyp2RotSamples>(G.seed, hyp2_key(pair_key, c, 0), tid, n, pos);
      double b1[6], b2[6];
      OKVFE_FP64_UNROLL
      for (int j = 0; j < kHyp2RotSamples; ++j) {
        const int e = s_list[pos[j]];
        kA[j] = e & 4095;
        Corr2 R;
        make_correspondence2<kTree>(A, blk0, blk1, fu, kA[j], e >> 12, R);
        OKVFE_FP64_UNROLL
        for (int i = 0; i < 3; ++i) {
          b1[3 * j + i] = R.b1[i];
          b2[3 * j + i] = R.b2[i];
        }
      }
      valid = twopt_rotation(b1, b2, M);
    }
    double* out = G.out.rot_hyp + 9 * row;
    for (int i = 0; i < 9; ++i) out[i] = M[i];
    G.out.rot_valid[row] = valid ? 1 : 0;
    if (G.out.rot_samples) {
      G.out.rot_samples[2 * row] = kA[0];
      G.out.rot_samples[2 * row + 1] = kA[1];
    }
  }

  // phase 2, relative pose: kHyp2Solvers hypotheses a round
  if (lane >= kHyp2PerWave) return;
  double* ws = s_work + (size_t)(wave * kHyp2PerWave + lane) * kHyp2Stride;
  for (int base = 0; base < OKVFE_RANSAC_MAX_HYPOTHESES; base += kHyp2Solvers) {
    const int h = base + wave * kHyp2PerWave + lane;
    if (h >= n_hyp) break;
    const size_t row = pc * (size_t)n_hyp + (size_t)h;
    double H[12];
    for (int i = 0; i < 12; ++i) H[i] = 0.0;
    int n_roots = 0;
    bool valid = false;
    int32_t* smp = G.out.rel_samples ? G.out.rel_samples + kHyp2RelSamples * row : nullptr;
    if (solve) {
      int pos[kHyp2RelSamples];
      hyp2_sample<kHyp2RelSamples>(G.seed, hyp2_key(pair_key, c, 1), h, n, pos);
      OKVFE_FP64_UNROLL
      for (int j = 0; j < kHyp2RelSamples; ++j) {
        const int e = s_list[pos[j]];
        const int kA = e & 4095;
        if (smp) smp[j] = kA;
        Corr2 R;
        make_correspondence2<kTree>(A, blk0, blk1, fu, kA, e >> 12, R);
        OKVFE_FP64_UNROLL
        for (int i = 0; i < 3; ++i) {
          ws[kHyp2B1 + 3 * j + i] = R.b1[i];
          ws[kHyp2B2 + 3 * j + i] = R.b2[i];
        }
        if (j >= 5) {
          ws[kHyp2S1 + (j - 5)] = R.s1;
          ws[kHyp2S2 + (j - 5)] = R.s2;
        }
      }
      valid = fivept_hypothesis(ws + kHyp2B1, ws + kHyp2B2, ws + kHyp2S1, ws + kHyp2S2, ws, H, &n_roots, RelativeSum<kTree>{});
    } else if (smp) {
      for (int j = 0; j < kHyp2RelSamples; ++j) smp[j] = -1;
    }
    double* out = G.out.rel_hyp + 12 * row;
    for (int i = 0; i < 12; ++i) out[i] = H[i];
    G.out.rel_valid[row] = valid ? 1 : 0;
    if (G.out.rel_n_roots) G.out.rel_n_roots[row] = n_roots;
  }
}

}  // namespace

// okvfe_twopt_rotation_hypothesis / okvfe_fivept_hypothesis: the header's solvers with the same distance, on the host
bool twopt_rotation_host(const double* b1, const double* b2, double* M) { return twopt_rotation(b1, b2, M); }
bool fivept_hypothesis_host(bool tree, const double* b1, const double* b2, const double* sigma1, const double* sigma2,
                            double* hypothesis, int* n_roots) {
  double ws[kFiveptWork];
  return tree ? fivept_hypothesis(b1, b2, sigma1, sigma2, ws, hypothesis, n_roots, RelativeSum<true>{})
              : fivept_hypothesis(b1, b2, sigma1, sigma2, ws, hypothesis, n_roots, RelativeSum<false>{});
}

void launch_ransac2d2d_hypotheses(const Ransac2d2dArgs& args, const uint64_t* keys, uint64_t seed,
                                  const okvfe_ransac2d2d_hypotheses_device& out, int n_pairs, hipStream_t stream) {
  if (n_pairs <= 0) return;
  Hyp2Args G;
  G.A = args;
  G.keys = keys;
  G.seed = seed;
  G.out = out;
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac2d2d_hypotheses_kernel<false> : ransac2d2d_hypotheses_kernel<true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_pairs * (unsigned)args.n_cams), dim3(kHyp2Threads), 0, stream, G);
}

}  // namespace okvfe
