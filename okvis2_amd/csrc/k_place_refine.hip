// k_place_refine.hip -- the refinement of Frontend::verifyRecognisedPlace's pose T_Sold_Snew
// (okvis_frontend/src/Frontend.cpp:399-527) for a batch of multiframes, as the defined algorithm of
// tests/place_refine_ref.py, in short launches: no launch holds the loop.
//   place_refine_start_kernel   a lane per multiframe: the start pose (the caller's, or Transformation(Matrix4d) of the
//                               winning hypothesis) into a fresh record; an unverified multiframe ends here (status 0)
//   place_refine_eval_kernel    place_hessian_kernel's structure unchanged: one work-group per multiframe, cameras one
//                               after another, the term rows compacted into the LDS ring and evaluated kEvalChunk at a
//                               time, a lane per term, at the record's candidate pose.  A term lane goes on from
//                               hessian_term to the Cauchy-weighted w r and w J (accumulate() of the restatement) and
//                               stages 15 doubles; fixed lanes of the first wave add term after term in adapter order
//                               from zero: lanes 0..20 the upper triangle of A, 21..26 g, 27 the sum of rho0.  That
//                               order is the contract: there is no tree over the terms.  A work-group whose multiframe
//                               has ended returns after one load.
//   place_refine_step_kernel    a lane per multiframe: refine_adopt_start (first launch) and refine_advance of
//                               place_refine_dev.h on the record and the evaluation; a lane that ends writes its outputs
// FP64 without FMA; 3- and 4-term sums in the order of okvfe_set_fp64_reduction (a template argument).  Every index that
// scales a multiframe or a block is 64-bit.
#include <float.h>

#include "place_term_dev.h"

namespace okvfe {
namespace {

constexpr int kLaneThreads = 64;           // the per-multiframe kernels: one wave per work-group
constexpr int kEvalThreads = 256;
constexpr int kEvalChunk = kEvalThreads;   // terms evaluated at a time: one per lane
constexpr int kEvalRing = 2 * kEvalChunk;  // a tile of keypoints adds at most a chunk to less than a chunk
constexpr int kEvalWaves = kEvalThreads / 64;
constexpr int kEvalStage = 15;             // w J (12), w r (2), rho0
static_assert((kEvalRing & (kEvalRing - 1)) == 0, "ring positions are masked");

__global__ __launch_bounds__(kLaneThreads) void place_refine_start_kernel(PlaceRefineArgs A) {
  const int64_t m = (int64_t)blockIdx.x * kLaneThreads + threadIdx.x;
  if (m >= A.n_multiframes) return;
  PlaceRefineRecord* rec = A.records + m;
  // not verified: the reference has returned false before the problem exists
  if (A.term.verdict && A.term.verdict[m] != 3) {
    rec->status = 0;
    rec->pending = 0;
    A.status[m] = 0;
    if (A.n_iterations) A.n_iterations[m] = 0;
    if (A.n_accepted) A.n_accepted[m] = 0;
    if (A.n_terms) A.n_terms[m] = 0;
    if (A.cost) {
      A.cost[2 * m] = 0.0;
      A.cost[2 * m + 1] = 0.0;
    }
    return;
  }
  double x[7];
  bool bad_best = false;
  if (A.initial) {
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = A.initial[7 * m + j];
  } else {
    const int best = A.best[m];
    bad_best = best < 0 || best >= A.n_hyp;
    if (bad_best) {
#pragma unroll
      for (int j = 0; j < 7; ++j) x[j] = elementary_nan();
    } else {
      const double* hyp = A.hypotheses + 12 * (m * (int64_t)A.n_hyp + best);
      double Hm[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) Hm[j] = hyp[j];
      start_pose(Hm, x);
    }
  }
  PlaceRefineRecord r;
  refine_init(r, x, bad_best);
  *rec = r;
}

template <bool kTree, bool kRT8>
__global__ __launch_bounds__(kEvalThreads) void place_refine_eval_kernel(PlaceRefineArgs R) {
  // 30 KiB, entry-major: a lane's fifteen stores fall on its own bank pair, and the odd row pitch keeps the rows the
  // summing lanes read at one term on different banks
  __shared__ double s_J[kEvalStage][kEvalChunk + 1];
  __shared__ int s_ring[kEvalRing];       // keypoint rows of the camera in hand
  __shared__ double s_Tsw[16], s_Tcs[16], s_t[3];
  __shared__ int s_wave[kEvalWaves];
  __shared__ int s_singular;
  const PlaceHessianArgs& A = R.term;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = A.kp_cap;
  const size_t frame0 = (size_t)m * (size_t)A.n_cams;
  const PlaceRefineRecord* rec = R.records + (size_t)m;

  if (rec->status != kRefineRunning) return;  // ended (or never verified): nothing asks for this evaluation
  if (tid == 0) {
    double pose[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) pose[j] = rec->xc[j];
    inverse_transform<kTree>(pose, s_Tsw);  // ReprojectionError.hpp:120-124
    s_t[0] = pose[0]; s_t[1] = pose[1]; s_t[2] = pose[2];
    s_singular = 0;
  }
  // tid < 28: the rows of the stage this lane multiplies, p0 p1 + p2 p3 (lane 27 adds row 14 as it is)
  int p0 = 0, p1 = 0, p2 = 0, p3 = 0;
  if (tid < 21) {
    int i = 0, e = tid;
    while (e >= 6 - i) {
      e -= 6 - i;
      ++i;
    }
    p0 = i; p1 = i + e; p2 = 6 + i; p3 = 6 + i + e;   // (w J)_0i (w J)_0j + (w J)_1i (w J)_1j
  } else if (tid < 27) {
    p0 = tid - 21; p1 = 12; p2 = 6 + (tid - 21); p3 = 13;  // (w J)_0j (w r)_0 + (w J)_1j (w r)_1
  }
  const bool is_cost = tid == 27;
  double acc = 0.0;

  // evaluates the terms [tail, tail + n) of the ring, n <= kEvalChunk, and adds them in that order
  auto evaluate = [&](int c, int tail, int n) {
    bool bad = false;
    if (tid < n) {
      const int k = s_ring[(tail + tid) & (kEvalRing - 1)];
      const size_t row = (frame0 + c) * (size_t)K + (size_t)k;
      const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
      const okvfe_keypoint kp = reinterpret_cast<const okvfe_keypoint*>(blk + A.o_kps)[k];
      const double* hp = A.hp + 4 * (size_t)A.match_landmark[row];
      const double hp_W[4] = {hp[0], hp[1], hp[2], hp[3]};
      double r[2], J[12];
      bad = hessian_term<kTree, kRT8>(A.dcams[A.cams[c].cam], A.w, A.h, s_Tsw, s_t, s_Tcs, hp_W, kp, r, J);
      // CauchyLoss(3) and ceres' corrector without its second-order part, as accumulate() of the restatement writes them
      const double s = r[0] * r[0] + r[1] * r[1];
      const double total = 1.0 + s * 1.11111111111111104943e-01;
      const double rho0 = 9.0 * log_fixed(total);
      const double inv = 1.0 / total;
      const double rho1 = DBL_MIN < inv ? inv : DBL_MIN;  // std::max(DBL_MIN, inv)
      const double w = sqrt(rho1);
#pragma unroll
      for (int e = 0; e < 12; ++e) s_J[e][tid] = w * J[e];
      s_J[12][tid] = w * r[0];
      s_J[13][tid] = w * r[1];
      s_J[14][tid] = rho0;
    }
    const unsigned long long bal = __ballot(bad);
    if (lane == 0 && bal) atomicAdd(&s_singular, (int)__popcll(bal));
    __syncthreads();
    if (tid < 28)
      for (int t = 0; t < n; ++t) {
        const double pair = s_J[p0][t] * s_J[p1][t] + s_J[p2][t] * s_J[p3][t];
        acc = acc + (is_cost ? s_J[14][t] : pair);
      }
    __syncthreads();  // the stage is rewritten by the next chunk
  };

  int head = 0, tail = 0;  // uniform: terms compacted / terms evaluated
  for (int c = 0; c < A.n_cams; ++c) {
    if (tid == 0) inverse_transform<kTree>(A.cams[c].pose, s_Tcs);  // :115-119 (the last chunk of the camera before is done)
    __syncthreads();
    const uint8_t* blk = A.blocks + (frame0 + c) * A.block_bytes;
    int count = *reinterpret_cast<const int32_t*>(blk + A.o_count);
    count = count < 0 ? 0 : (count > K ? K : count);
    for (int base = 0; base < count; base += kEvalThreads) {
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
      for (int w = 0; w < kEvalWaves; ++w) {
        pos += w < wave ? s_wave[w] : 0;
        head += s_wave[w];
      }
      if (take) s_ring[pos & (kEvalRing - 1)] = k;
      __syncthreads();
      if (head - tail >= kEvalChunk) {
        evaluate(c, tail, kEvalChunk);
        tail += kEvalChunk;
      }
    }
    // the rest of this camera: the next one has another T_CS
    if (head > tail) {
      evaluate(c, tail, head - tail);
      tail = head;
    }
  }
  __syncthreads();
  PlaceRefineEval* ev = R.evals + (size_t)m;
  if (tid < 21) ev->a[tid] = acc;
  else if (tid < 27) ev->g[tid - 21] = acc;
  else if (tid == 27) ev->cost = 0.5 * acc;
  if (tid == 0) {
    ev->n_terms = head;
    ev->n_singular = s_singular;
  }
}

template <bool kTree>
__global__ __launch_bounds__(kLaneThreads) void place_refine_step_kernel(PlaceRefineArgs A, int first) {
  const int64_t m = (int64_t)blockIdx.x * kLaneThreads + threadIdx.x;
  if (m >= A.n_multiframes) return;
  if (A.records[m].status != kRefineRunning) return;  // ended at an earlier step: its outputs are written
  PlaceRefineRecord r = A.records[m];
  const PlaceRefineEval e = A.evals[m];
  if (first) refine_adopt_start(r, e);
  refine_advance<kTree>(r, e, A.max_iterations);
  A.records[m] = r;
  if (r.status == kRefineRunning) return;  // a candidate waits for its evaluation
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    A.poses[7 * m + j] = r.x[j];
    if (A.start_poses) A.start_poses[7 * m + j] = r.start[j];
  }
  A.status[m] = r.status;
  if (A.n_iterations) A.n_iterations[m] = r.it;
  if (A.n_accepted) A.n_accepted[m] = r.n_acc;
  if (A.n_terms) A.n_terms[m] = r.n_terms;
  if (A.cost) {
    A.cost[2 * m] = r.cost0;
    A.cost[2 * m + 1] = r.cost;
  }
}

dim3 lane_grid(int n) { return dim3((unsigned)((n + kLaneThreads - 1) / kLaneThreads)); }

}  // namespace

void launch_place_refine_start(const PlaceRefineArgs& args, hipStream_t stream) {
  if (args.n_multiframes <= 0) return;
  hipLaunchKernelGGL(place_refine_start_kernel, lane_grid(args.n_multiframes), dim3(kLaneThreads), 0, stream, args);
}

void launch_place_refine_eval(const PlaceRefineArgs& args, bool rt8, hipStream_t stream) {
  if (args.n_multiframes <= 0) return;
  const bool ltr = fp64_left_to_right();
  auto* kernel = rt8 ? (ltr ? place_refine_eval_kernel<false, true> : place_refine_eval_kernel<true, true>)
                     : (ltr ? place_refine_eval_kernel<false, false> : place_refine_eval_kernel<true, false>);
  hipLaunchKernelGGL(kernel, dim3(args.n_multiframes), dim3(kEvalThreads), 0, stream, args);
}

void launch_place_refine_step(const PlaceRefineArgs& args, bool first, hipStream_t stream) {
  if (args.n_multiframes <= 0) return;
  auto* kernel = fp64_left_to_right() ? place_refine_step_kernel<false> : place_refine_step_kernel<true>;
  hipLaunchKernelGGL(kernel, lane_grid(args.n_multiframes), dim3(kLaneThreads), 0, stream, args, first ? 1 : 0);
}

}  // namespace okvfe
