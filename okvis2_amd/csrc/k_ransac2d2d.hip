// k_ransac2d2d.hip -- the consensus step of Frontend::runRansac2d2d (okvis_frontend/src/Frontend.cpp:2281-2394) for a
// batch of (older multiframe, current multiframe) pairs: the correspondences of FrameRelativeAdapter
// (FrameRelativeAdapter.cpp:137-194), every correspondence against every hypothesis of FrameRotationOnlySacProblem
// (FrameRotationOnlySacProblem.hpp:126-144) and of FrameRelativePoseSacProblem (FrameRelativePoseSacProblem.hpp:130-160),
// the two winners, the choice between them (:2341-2358), the success flags shared by the cameras of a pair (:2289-2290,
// :2361) and the outlier removal (:2365-2375).  The sampler and the two minimal solvers are k_ransac2d2d_hyp.hip, included at
// the end of this file.
//   ransac2d2d_consensus_kernel   one work-group per pair, the cameras one after another.  Per camera: the first k per
//                                 landmark id of the CURRENT block goes into an LDS open-addressing table (a slot keeps
//                                 the minimum k of its id: std::map::insert does not overwrite); the OLDER block's
//                                 keypoints look their ids up, a tile at a time, and the hits are compacted, in
//                                 older-keypoint order, into an LDS ring of 64-byte records; a chunk of kRansac2Chunk
//                                 records is one record per lane of EVERY wave, and wave w walks the hypotheses
//                                 h = w, w + 4, ... of both lists, which sit in LDS: a hypothesis' inliers of a chunk
//                                 are a ballot + popcount, added by the one wave that owns it.  One lane takes the
//                                 decision; a final sweep over the older keypoints with the taken winner writes
//                                 match1 / state / distance and marks the current keypoints to remove.
// opengv::triangulation::triangulate2 and Eigen's 2 x 2 inverse are restated from their published sources (the header
// marks the call PARITY UNPINNED for them).  FP64, 3- and 4-term sums (fp64_ops.h) in the order of
// okvfe_set_fp64_reduction (a template argument: the host launches the kernel compiled for the order in force), no FMA.
#include "fp64_ops.h"
#include "okvfe_internal.h"

namespace okvfe {
namespace {

template <bool kTree>
__host__ __device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
  return fp64::sum3<kTree>(a[0] * b[0], a[1] * b[1], a[2] * b[2]);
}

constexpr int kRansac2Threads = 256;
constexpr int kRansac2Waves = kRansac2Threads / 64;
constexpr int kRansac2Chunk = 64;                     // records scored at a time: one per lane of every wave
constexpr int kRansac2Ring = 512;                     // a tile of keypoints adds at most 256 records to less than a chunk
constexpr int kRansac2Slots = 1 << kRansac2SlotsLog2;  // id table: more slots than a block has keypoints
static_assert((kRansac2Ring & (kRansac2Ring - 1)) == 0 && kRansac2Ring >= kRansac2Chunk - 1 + kRansac2Threads, "ring");
static_assert(kRansac2Slots > kRansac2dMaxKeypoints, "an empty slot always ends a probe");

// one correspondence of the adapter: bearingVectors1_[idxA], bearingVectors2_[idxB], sigmaAngles1_[idxA], sigmaAngles2_[idxB]
struct Corr2 {
  double b1[3], b2[3];
  double s1, s2;
};
static_assert(sizeof(Corr2) == 64, "64-byte LDS records");

// Eigen's normalize(): z = squaredNorm, divided by sqrt(z) iff z > 0
template <bool kTree>
__device__ __forceinline__ void normalize3(double v[3]) {
  const double z = fp64::sum3<kTree>(v[0] * v[0], v[1] * v[1], v[2] * v[2]);
  if (z > 0) {
    const double n = sqrt(z);
    v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
  }
}

// FrameRelativeAdapter.cpp:168-193 for the match (kA of the older block, kB of the current block)
template <bool kTree>
__device__ __forceinline__ void make_correspondence2(const Ransac2d2dArgs& A, const uint8_t* blk0, const uint8_t* blk1,
                                                     double fu, int kA, int kB, Corr2& R) {
  const double sqrt2 = __longlong_as_double(0x3FF6A09E667F3BCDLL);
  const float size1 = reinterpret_cast<const okvfe_keypoint*>(blk0 + A.o_kps)[kA].size;
  const double sa = (0.8 * (double)size1) / 12.0;                 // :175
  R.s1 = ((sqrt2 * sa) * sa) / (fu * fu);                         // :176
  const float size2 = reinterpret_cast<const okvfe_keypoint*>(blk1 + A.o_kps)[kB].size;
  const double sb = (0.8 * (double)size2) / 12.0;                 // :186
  R.s2 = ((sqrt2 * sb) * sb) / (fu * fu);                         // :187 (fu2 is frame A's geometry at camIdB: the same slot)
  // :178-182 and :190: EITHER failed back-projection leaves (1, 0, 0) in bearingVectors1_ -- :190 overwrites 1_, not 2_
  double v[3] = {1.0, 0.0, 0.0};
  if (blk0[A.o_bpv + kA] && blk1[A.o_bpv + kB]) {
    const double* bp = reinterpret_cast<const double*>(blk0 + A.o_bp) + 3 * (size_t)kA;
    v[0] = bp[0]; v[1] = bp[1]; v[2] = bp[2];
  }
  normalize3<kTree>(v);
  R.b1[0] = v[0]; R.b1[1] = v[1]; R.b1[2] = v[2];
  // :189-193: getBackProjection hands out the stored value whatever it returns (Frame.hpp:196-208)
  const double* bq = reinterpret_cast<const double*>(blk1 + A.o_bp) + 3 * (size_t)kB;
  double u[3] = {bq[0], bq[1], bq[2]};
  normalize3<kTree>(u);
  R.b2[0] = u[0]; R.b2[1] = u[1]; R.b2[2] = u[2];
}

// FrameRotationOnlySacProblem.hpp:140-143 and FrameRelativePoseSacProblem.hpp:157-160
template <bool kTree>
__host__ __device__ __forceinline__ double score_of_errors(const double e1[3], const double e2[3], double s1, double s2) {
  const double q1 = dot3<kTree>(e1, e1), q2 = dot3<kTree>(e2, e2);
  return (q1 * 0.5) / s1 + (q2 * 0.5) / s2;
}

// FrameRotationOnlySacProblem.hpp:126-144.  The ONE copy: the scoring loop and the final sweep call it.
template <bool kTree>
__host__ __device__ __forceinline__ double rotation_only_distance(const double* M /* 3 x 3 row-major */, const Corr2& R) {
  double e1[3], e2[3];
  for (int i = 0; i < 3; ++i) {
    const double f2u = fp64::sum3<kTree>(M[3 * i] * R.b2[0], M[3 * i + 1] * R.b2[1], M[3 * i + 2] * R.b2[2]);  // :131
    const double f1u = fp64::sum3<kTree>(M[i] * R.b1[0], M[3 + i] * R.b1[1], M[6 + i] * R.b1[2]);              // :134
    e1[i] = f2u - R.b1[i];                                                                                // :136
    e2[i] = f1u - R.b2[i];                                                                                // :137
  }
  return score_of_errors<kTree>(e1, e2, R.s1, R.s2);
}

// FrameRelativePoseSacProblem.hpp:137: ti = (-R^T) t
template <bool kTree>
__host__ __device__ __forceinline__ void inverse_translation(const double* H /* 3 x 4 row-major */, double* ti) {
  for (int i = 0; i < 3; ++i) ti[i] = fp64::sum3<kTree>((-H[i]) * H[3], (-H[4 + i]) * H[7], (-H[8 + i]) * H[11]);
}

// FrameRelativePoseSacProblem.hpp:130-160 with opengv's triangulate2 (and Eigen's 2 x 2 inverse) as published.  The ONE
// copy: the scoring loop and the final sweep call it.
template <bool kTree>
__host__ __device__ __forceinline__ double relative_pose_distance(const double* H /* [R | t] row-major */, const double* ti,
                                                         const Corr2& R) {
  const double t[3] = {H[3], H[7], H[11]};
  double f2u[3];
  for (int i = 0; i < 3; ++i) f2u[i] = fp64::sum3<kTree>(H[4 * i] * R.b2[0], H[4 * i + 1] * R.b2[1], H[4 * i + 2] * R.b2[2]);
  const double c0 = dot3<kTree>(t, R.b1), c1 = dot3<kTree>(t, f2u);
  const double A00 = dot3<kTree>(R.b1, R.b1), A10 = dot3<kTree>(R.b1, f2u);
  const double A01 = -A10, A11 = -dot3<kTree>(f2u, f2u);
  const double det = A00 * A11 - A10 * A01;
  const double invdet = 1.0 / det;  // parallel bearings: det == 0, the lambdas and the distance become NaN
  const double I00 = A11 * invdet, I10 = (-A10) * invdet, I01 = (-A01) * invdet, I11 = A00 * invdet;
  const double l0 = I00 * c0 + I01 * c1, l1 = I10 * c0 + I11 * c1;
  double p[3], rep2[3], e1[3], e2[3];
  for (int i = 0; i < 3; ++i) p[i] = (l0 * R.b1[i] + (t[i] + l1 * f2u[i])) / 2.0;
  for (int i = 0; i < 3; ++i) rep2[i] = fp64::sum4<kTree>(H[i] * p[0], H[4 + i] * p[1], H[8 + i] * p[2], ti[i] * 1.0);  // :146
  const double n1 = sqrt(dot3<kTree>(p, p)), n2 = sqrt(dot3<kTree>(rep2, rep2));                                 // :147-148
  for (int i = 0; i < 3; ++i) {
    e1[i] = p[i] / n1 - R.b1[i];     // :153
    e2[i] = rep2[i] / n2 - R.b2[i];  // :154
  }
  return score_of_errors<kTree>(e1, e2, R.s1, R.s2);
}

// the current keypoint the adapter's idMap holds for `id` (the first one, FrameRelativeAdapter.cpp:151), -1 = none
__device__ __forceinline__ int id_lookup(const int* tab, const int32_t* lm1, int id) {
  for (uint32_t s = ransac2d2d_id_slot(id);; s = (s + 1) & (uint32_t)(kRansac2Slots - 1)) {
    const int k = tab[s];
    if (k < 0) return -1;
    if (lm1[k] == id) return k;
  }
}

// FrameRelativeAdapter.cpp:139-152 for the current keypoint k: idMap keeps the FIRST current keypoint of every added
// landmark id.  The ONE copy: the consensus kernel and the hypotheses kernel build their tables with it.
__device__ __forceinline__ void id_insert(const Ransac2d2dArgs& A, int* tab, const int32_t* lm1, int k) {
  const int id = lm1[k];
  if (id < 0) return;                                                  // :143
  if (A.added && (id >= A.n_landmarks || A.added[id] == 0)) return;    // :147
  for (uint32_t s = ransac2d2d_id_slot(id);; s = (s + 1) & (uint32_t)(kRansac2Slots - 1)) {
    const int old = atomicCAS(&tab[s], -1, k);
    if (old < 0) break;
    if (lm1[old] == id) {  // the slot is this id's (it only ever holds keypoints of one id): :151 keeps the first
      atomicMin(&tab[s], k);
      break;
    }
  }
}

template <bool kTree>
__global__ __launch_bounds__(kRansac2Threads) void ransac2d2d_consensus_kernel(Ransac2d2dArgs A) {
  __shared__ Corr2 s_rec[kRansac2Ring];                          // 32 KiB
  __shared__ double s_rot[OKVFE_RANSAC_MAX_HYPOTHESES][9];       // 4.5 KiB
  __shared__ double s_rel[OKVFE_RANSAC_MAX_HYPOTHESES][12];      // 6 KiB
  __shared__ double s_ti[OKVFE_RANSAC_MAX_HYPOTHESES][3];        // 1.5 KiB
  __shared__ int s_tab[kRansac2Slots];                           // 16 KiB: a current keypoint per slot, -1 = empty
  __shared__ unsigned s_kick[kRansac2Slots / 32];                // one bit per current keypoint: remove it
  __shared__ int s_cnt[2][OKVFE_RANSAC_MAX_HYPOTHESES];
  __shared__ int s_valid[2][OKVFE_RANSAC_MAX_HYPOTHESES];
  __shared__ int s_wave[kRansac2Waves];
  __shared__ int s_branch, s_taken, s_removed;                   // of this camera
  __shared__ int s_total, s_rot_only, s_success;                 // of the pair: the locals of :2285-2290
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.kp_cap;
  const size_t frame0 = (size_t)A.pairs[2 * p] * (size_t)A.n_cams, frame1 = (size_t)A.pairs[2 * p + 1] * (size_t)A.n_cams;
  if (tid == 0) {
    s_total = 0;
    s_rot_only = 0;
    s_success = 0;
  }

  // scores the records [tail, tail + n) of the ring, 0 < n <= kRansac2Chunk: every wave holds them all, one per lane
  auto score = [&](int tail, int n) {
    const bool have = lane < n;
    const Corr2 R = s_rec[(tail + (have ? lane : 0)) & (kRansac2Ring - 1)];
    for (int h = wave; h < A.n_hyp; h += kRansac2Waves) {
      if (s_valid[0][h]) {  // opengv skips a sample whose solver failed
        const double d = rotation_only_distance<kTree>(s_rot[h], R);
        const unsigned long long in = __ballot(have && d < A.threshold);  // a NaN is an outlier
        if (lane == 0) s_cnt[0][h] += (int)__popcll(in);
      }
      if (s_valid[1][h]) {
        const double d = relative_pose_distance<kTree>(s_rel[h], s_ti[h], R);
        const unsigned long long in = __ballot(have && d < A.threshold);
        if (lane == 0) s_cnt[1][h] += (int)__popcll(in);
      }
    }
  };

  for (int c = 0; c < A.n_cams; ++c) {  // :2293
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

    if (tid < A.n_hyp) {
      const size_t h = pc * (size_t)A.n_hyp + (size_t)tid;
      for (int i = 0; i < 9; ++i) s_rot[tid][i] = A.rot_hyp[9 * h + i];
      for (int i = 0; i < 12; ++i) s_rel[tid][i] = A.rel_hyp[12 * h + i];
      inverse_translation<kTree>(A.rel_hyp + 12 * h, s_ti[tid]);
      s_cnt[0][tid] = 0;
      s_cnt[1][tid] = 0;
      s_valid[0][tid] = A.rot_valid ? (A.rot_valid[h] != 0) : 1;
      s_valid[1][tid] = A.rel_valid ? (A.rel_valid[h] != 0) : 1;
    }
    for (int s = tid; s < kRansac2Slots; s += kRansac2Threads) s_tab[s] = -1;
    for (int s = tid; s < kRansac2Slots / 32; s += kRansac2Threads) s_kick[s] = 0u;
    __syncthreads();

    // FrameRelativeAdapter.cpp:139-152: idMap, the FIRST current keypoint of every added landmark id
    for (int k = tid; k < count1; k += kRansac2Threads) id_insert(A, s_tab, lm1, k);
    __syncthreads();

    // :154-165: the matches in older-keypoint order, a tile of keypoints at a time
    int head = 0, tail = 0;  // uniform: records compacted / records scored
    for (int base = 0; base < count0; base += kRansac2Threads) {
      const int k = base + tid;
      int kB = -1;
      if (k < count0) {
        const int id = lm0[k];
        if (id >= 0) kB = id_lookup(s_tab, lm1, id);  // :157, :160: the older id is not tested for isLandmarkAdded
      }
      const bool take = kB >= 0;
      Corr2 R;
      if (take) make_correspondence2<kTree>(A, blk0, blk1, fu, k, kB, R);
      const unsigned long long bal = __ballot(take);
      if (lane == 0) s_wave[wave] = (int)__popcll(bal);
      __syncthreads();  // (also: every lane has loaded its records of the chunks scored in the last round)
      int pos = head + (int)__popcll(bal & ((1ull << lane) - 1ull));
      for (int w = 0; w < kRansac2Waves; ++w) {
        pos += w < wave ? s_wave[w] : 0;
        head += s_wave[w];
      }
      if (take) s_rec[pos & (kRansac2Ring - 1)] = R;
      __syncthreads();
      while (head - tail >= kRansac2Chunk) {  // (a full chunk is more than the 10 of :2300)
        score(tail, kRansac2Chunk);
        tail += kRansac2Chunk;
      }
    }
    const int n_corr = head;
    const bool scored = n_corr >= 10;  // :2300
    if (scored && head > tail) score(tail, head - tail);
    __syncthreads();

    if (tid == 0) {
      // opengv's Ransac::computeModel replaces its best model only on strictly more inliers, from zero
      int best[2] = {-1, -1}, most[2] = {0, 0};
      int branch = 0, removed = 0, taken = -1;
      if (scored) {
        for (int q = 0; q < 2; ++q)
          for (int h = 0; h < A.n_hyp; ++h)
            if (s_valid[q][h] && s_cnt[q][h] > most[q]) {
              most[q] = s_cnt[q][h];
              best[q] = h;
            }
        const float nf = (float)n_corr;
        const float rot_ratio = (float)most[0] / nf;  // :2320 (float32, correctly rounded)
        const float rel_ratio = (float)most[1] / nf;  // :2337
        if (rot_ratio > rel_ratio || rot_ratio > 0.8f) {  // :2341
          branch = 1;
          if (most[0] > 10) s_success |= 1;               // :2342
          s_rot_only = 1;                                 // :2345
          s_total += most[0];                             // :2346
          taken = best[0];
        } else {
          branch = 2;
          if (most[1] > 10 && rel_ratio > 0.8f) s_success |= 2;  // :2351
          s_total += most[1];                                    // :2354
          taken = best[1];
        }
        removed = s_success != 0;  // :2361: the flags of the earlier cameras count
      }
      A.out.n_correspondences[pc] = n_corr;
      A.out.rot_best[pc] = best[0];
      A.out.rot_inliers[pc] = most[0];
      A.out.rel_best[pc] = best[1];
      A.out.rel_inliers[pc] = most[1];
      A.out.branch[pc] = (uint8_t)branch;
      A.out.removed[pc] = (uint8_t)removed;
      s_branch = branch;
      s_taken = taken;
      s_removed = removed;
    }
    if (tid < A.n_hyp) {
      if (A.out.rot_hyp_inliers) A.out.rot_hyp_inliers[pc * A.n_hyp + tid] = scored && s_valid[0][tid] ? s_cnt[0][tid] : -1;
      if (A.out.rel_hyp_inliers) A.out.rel_hyp_inliers[pc * A.n_hyp + tid] = scored && s_valid[1][tid] ? s_cnt[1][tid] : -1;
    }
    __syncthreads();
    if (A.out.match1 || A.out.state || A.out.distance || A.out.landmark1_out) {
      // the final sweep: every older keypoint below its block's count against the taken branch's winner
      const int branch = s_branch, taken = s_taken;
      const bool kick = s_removed && A.remove_outliers;  // :2367-2374
      for (int k = tid; k < count0; k += kRansac2Threads) {
        const int id = lm0[k];
        const int kB = id >= 0 ? id_lookup(s_tab, lm1, id) : -1;
        const size_t row = pc * (size_t)K + (size_t)k;
        int st = 0;
        if (kB >= 0) {
          st = 1;
          if (taken >= 0) {
            Corr2 R;
            make_correspondence2<kTree>(A, blk0, blk1, fu, k, kB, R);
            double d;
            if (branch == 1) d = rotation_only_distance<kTree>(s_rot[taken], R);
            else d = relative_pose_distance<kTree>(s_rel[taken], s_ti[taken], R);
            if (d < A.threshold) st = 2;
            if (A.out.distance) A.out.distance[row] = d;
          }
          if (kick && st == 1) atomicOr(&s_kick[kB >> 5], 1u << (kB & 31));
        }
        if (A.out.match1) A.out.match1[row] = kB;
        if (A.out.state) A.out.state[row] = (uint8_t)st;
      }
      __syncthreads();  // every id of the older rows is read before a current row is written (the rows may be the same)
      if (A.out.landmark1_out) {
        int32_t* out = A.out.landmark1_out + (frame1 + c) * K;
        for (int k = tid; k < count1; k += kRansac2Threads) {
          const int id = lm1[k];
          out[k] = (s_kick[k >> 5] >> (k & 31)) & 1u ? -1 : id;
        }
      }
      __syncthreads();  // the table and the marks are cleared for the next camera
    }
  }

  if (tid == 0) {  // :2387-2392
    const int ok = s_success != 0;
    A.out.total_inliers[p] = ok ? s_total : -1;
    A.out.rotation_only[p] = (uint8_t)(ok ? s_rot_only : 1);  // (the "hack" of :2391)
    A.out.success[p] = (uint8_t)s_success;
  }
}

}  // namespace

void launch_ransac2d2d_consensus(const Ransac2d2dArgs& args, int n_pairs, hipStream_t stream) {
  if (n_pairs <= 0) return;
  const bool ltr = fp64_left_to_right();
  auto* kernel = ltr ? ransac2d2d_consensus_kernel<false> : ransac2d2d_consensus_kernel<true>;
  hipLaunchKernelGGL(kernel, dim3(n_pairs), dim3(kRansac2Threads), 0, stream, args);
}

int ransac2d2d_chunk_records() { return kRansac2Chunk; }
int ransac2d2d_ring_records() { return kRansac2Ring; }

}  // namespace okvfe

#include "k_ransac2d2d_hyp.hip"
