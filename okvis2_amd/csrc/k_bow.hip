// k_bow.hip -- place recognition on device-resident batches: what dBow_->database.query(features, ...) and
// database.add(features) do (okvis_frontend/src/Frontend.cpp:660-672, :752-766, :896-898), and the part of the walk over
// the sorted results that needs no estimator state (:771-802; :690-723 without the predicate).  One work-group per
// multiframe throughout; multiframe m owns gather blocks m n_cams + c.
//   bow_vectors_kernel    features -> word ids (voc_descend) -> BowVector.  The word ids of a multiframe are sorted in LDS
//                         (bitonic, padded with a sentinel to a power of two) and run-length encoded: the first lane of
//                         a run finds the run's end by binary search, adds the weight once per occurrence and writes the
//                         word.  The L1 norm is summed by ONE lane in ascending word order, 256 words at a time out of
//                         LDS: the order is DBoW2's and is the contract (okvfe_set_fp64_reduction does not apply).
//   place_query_kernel    the query vector in LDS (a dense word -> position table for small vocabularies, else the
//                         sorted vector for bow_l1_merge); the entries 256 at a time, a lane per entry; listed
//                         (entry, score) pairs go into an LDS ring in entry order by ballot + prefix, and a ring element
//                         is decided once its two successors are known or the entries are exhausted.
//   bow_db_add_kernel     work-group i copies multiframe add_index[i]'s vector behind the entries before it; every group
//                         sums the word counts of the groups before it itself, so the call is one launch.
#include "bow_dev.h"

namespace okvfe {
namespace {

constexpr int kBowThreads = 256;
constexpr int kBowWaves = kBowThreads / 64;
constexpr uint32_t kBowNoWord = 0xFFFFFFFFu;  // sorts behind every word id

__device__ __forceinline__ int wave_rank(bool flag, int lane, int* total) {
  const unsigned long long b = __ballot(flag);
  *total = (int)__popcll(b);
  return (int)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBowThreads) void bow_vectors_kernel(BowVectorsArgs A) {
  extern __shared__ uint4 s_dyn[];  // [node descriptors, if they fit beside the keys][keys_cap sort keys]
  __shared__ double s_val[kBowThreads];
  __shared__ int s_cnt[kBowWaves];
  __shared__ double s_norm;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool in_lds = A.nodes_in_lds != 0;
  uint32_t* s_keys = reinterpret_cast<uint32_t*>(s_dyn + (in_lds ? A.n_nodes * 3 : 0));
  if (in_lds) {
    const uint4* src = reinterpret_cast<const uint4*>(A.node_desc);
    for (int i = tid; i < A.n_nodes * 3; i += kBowThreads) s_dyn[i] = src[i];
    __syncthreads();
  }
  // features: camera 0's keypoints k < count, then camera 1's, ... (Frontend.cpp:663-672)
  int n_feat = 0;
  for (int c = 0; c < A.n_cams; ++c) {
    const size_t b = (size_t)m * (size_t)A.n_cams + (size_t)c;
    const uint8_t* block = A.blocks + b * A.block_bytes;
    int count = *reinterpret_cast<const int32_t*>(block + A.o_count);
    count = count < 0 ? 0 : (count > A.kp_cap ? A.kp_cap : count);
    for (int k = tid; k < count; k += kBowThreads) {
      const Desc12 a = load_desc(block + A.o_desc + (size_t)k * OKVFE_DESC_BYTES);
      const int node = voc_descend(a, s_dyn, in_lds, A.node_desc, A.child_begin, A.child_index);
      const int w = A.node_word[node];
      if (A.word_ids) A.word_ids[b * (size_t)A.kp_cap + k] = w;
      // words with !(weight > 0) are skipped (a NaN weight too)
      const bool kept = w >= 0 && w < A.n_words && A.word_weight[w] > 0;
      s_keys[n_feat + k] = kept ? (uint32_t)w : kBowNoWord;
    }
    n_feat += count;
  }
  int P = kBowThreads;
  while (P < n_feat) P <<= 1;  // <= keys_cap: n_feat <= n_cams kp_cap
  for (int i = n_feat + tid; i < P; i += kBowThreads) s_keys[i] = kBowNoWord;
  __syncthreads();
  // bitonic sort, ascending
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kBowThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ixj = i | j;
        const uint32_t a = s_keys[i], b = s_keys[ixj];
        if ((a > b) == ((i & k) == 0)) {
          s_keys[i] = b;
          s_keys[ixj] = a;
        }
      }
      __syncthreads();
    }
  // run-length encoding, 256 sorted keys per round; the words of a round are consecutive in the output
  const bool sums = A.weighting == 0 || A.weighting == 1;  // TF_IDF, TF
  int32_t* ids_row = A.ids + (size_t)m * (size_t)A.stride;
  double* val_row = A.values + (size_t)m * (size_t)A.stride;
  int n = 0;          // distinct words so far (uniform)
  double norm = 0.0;  // thread 0
  for (int r0 = 0; r0 < P; r0 += kBowThreads) {
    if (s_keys[r0] == kBowNoWord) break;  // uniform: only padding from here on
    const int i = r0 + tid;
    const uint32_t key = s_keys[i];
    const bool head = key != kBowNoWord && (i == 0 || s_keys[i - 1] != key);
    int total;
    const int rank = wave_rank(head, lane, &total);
    if (lane == 0) s_cnt[wave] = total;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < kBowWaves; ++w) {
      off += w < wave ? s_cnt[w] : 0;
      all += s_cnt[w];
    }
    if (head) {
      int lo = i + 1, hi = P;  // first index behind the run
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_keys[mid] == key) lo = mid + 1; else hi = mid;
      }
      const double wgt = A.word_weight[key];
      double acc = wgt;  // BowVector::addWeight: the weight once per occurrence, by repeated addition
      if (sums)
        for (int q = i + 1; q < lo; ++q) acc = acc + wgt;
      const int j = n + off + rank;
      if (j < A.stride) {
        ids_row[j] = (int32_t)key;
        val_row[j] = acc;
      }
      s_val[off + rank] = acc;
    }
    __syncthreads();
    if (tid == 0 && A.normalise_l1)
      for (int q = 0; q < all; ++q) norm = norm + fabs(s_val[q]);  // sequential, ascending word order
    n += all;
  }
  if (tid == 0) {
    s_norm = norm;
    A.n_out[m] = n < A.stride ? n : A.stride;
  }
  __syncthreads();  // (also: the values above are visible to the whole group)
  const double nrm = s_norm;
  const int n_store = n < A.stride ? n : A.stride;
  if (A.normalise_l1) {
    if (nrm > 0.0)
      for (int j = tid; j < n_store; j += kBowThreads) val_row[j] = val_row[j] / nrm;
  } else if (sums && n > 0) {
    const double nd = (double)n;
    for (int j = tid; j < n_store; j += kBowThreads) val_row[j] = val_row[j] / nd;
  }
}

// ---- query and candidates ------------------------------------------------------------------------
constexpr int kRing = 512;  // >= 256 new elements + the two undecided ones + their two predecessors

template <bool kDense>
__global__ __launch_bounds__(kBowThreads) void place_query_kernel(PlaceQueryArgs A) {
  extern __shared__ double s_q[];  // [lds_values query values][dense: n_vocab positions | else: lds_values word ids]
  __shared__ int s_rid[kRing];
  __shared__ double s_rsc[kRing];
  __shared__ int s_cnt[2][kBowWaves];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* s_qv = s_q;
  int32_t* s_qi = reinterpret_cast<int32_t*>(s_q + A.lds_values);
  const int32_t* q_ids = A.q_ids + (size_t)m * (size_t)A.stride;
  const double* q_values = A.q_values + (size_t)m * (size_t)A.stride;
  int n_q = A.q_n[m];
  n_q = n_q < 0 ? 0 : (n_q > A.stride ? A.stride : n_q);
  bool staged = true;
  if (kDense) {
    for (int w = tid; w < A.n_vocab; w += kBowThreads) s_qi[w] = -1;
    __syncthreads();
    for (int j = tid; j < n_q && j < A.lds_values; j += kBowThreads) {
      const int id = q_ids[j];
      if (id >= 0 && id < A.n_vocab) {
        s_qi[id] = j;
        s_qv[j] = q_values[j];
      }
    }
  } else {
    staged = n_q <= A.lds_values;  // uniform; a longer vector is merged from memory
    if (staged)
      for (int j = tid; j < n_q; j += kBowThreads) {
        s_qi[j] = q_ids[j];
        s_qv[j] = q_values[j];
      }
  }
  __syncthreads();

  const int E = A.n_entries;
  int32_t* out_entry = A.entry + (size_t)m * (size_t)A.cap;
  double* out_score = A.score + (size_t)m * (size_t)A.cap;
  int n_l = 0, n_d = 0, n_c = 0;  // listed, decided, candidates (uniform)
  // decides the listed positions [n_d, d_end): both successors of each are in the ring, or the entries are exhausted
  auto decide = [&](int d_end) {
    for (int f0 = n_d; f0 < d_end; f0 += kBowThreads) {
      const int f = f0 + tid;
      bool cand = false;
      int id = 0;
      double p = 0.0;
      if (f < d_end) {
        id = s_rid[f & (kRing - 1)];
        p = s_rsc[f & (kRing - 1)];
        bool larger = false;  // Frontend.cpp:780-799
        if (f > 0) {
          if (s_rsc[(f - 1) & (kRing - 1)] > p) larger = true;
          if (f > 1 && s_rsc[(f - 2) & (kRing - 1)] > p) larger = true;
        }
        if (f + 1 < n_l) {
          if (s_rsc[(f + 1) & (kRing - 1)] > p) larger = true;
          if (f + 2 < n_l && s_rsc[(f + 2) & (kRing - 1)] > p) larger = true;
        }
        const bool suppressible = A.suppressible ? A.suppressible[id] != 0 : true;
        cand = !(suppressible && larger) && p > A.min_score;  // :802, strict
      }
      int total;
      const int rank = wave_rank(cand, lane, &total);
      if (lane == 0) s_cnt[1][wave] = total;
      __syncthreads();
      int off = 0, all = 0;
      for (int w = 0; w < kBowWaves; ++w) {
        off += w < wave ? s_cnt[1][w] : 0;
        all += s_cnt[1][w];
      }
      const int pos = n_c + off + rank;
      if (cand && pos < A.cap) {
        out_entry[pos] = id;
        out_score[pos] = p;
      }
      n_c += all;
      __syncthreads();
    }
    if (d_end > n_d) n_d = d_end;
  };

  for (int e0 = 0; e0 < E; e0 += kBowThreads) {
    const int e = e0 + tid;
    double score = -1.0;
    if (e < E) {
      const int i0 = A.db_begin[e], i1 = A.db_begin[e + 1];
      if (kDense) {
        double value = 0.0;
        bool any = false;
        // ascending word order: the additions of the merge, in its order.  Four words are loaded ahead of their use: a
        // lane's loads are a dependent chain of cache misses otherwise, and one work-group has nothing to hide them with
        int i = i0;
        for (; i + 4 <= i1; i += 4) {
          int w[4];
          double d[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            w[u] = A.db_ids[i + u];
            d[u] = A.db_values[i + u];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int j = w[u] >= 0 && w[u] < A.n_vocab ? s_qi[w[u]] : -1;
            if (j >= 0) {
              value = bow_l1_term(value, s_qv[j], d[u]);
              any = true;
            }
          }
        }
        for (; i < i1; ++i) {
          const int w = A.db_ids[i];
          const int j = w >= 0 && w < A.n_vocab ? s_qi[w] : -1;
          if (j >= 0) {
            value = bow_l1_term(value, s_qv[j], A.db_values[i]);
            any = true;
          }
        }
        score = any ? -value / 2.0 : -1.0;
      } else if (staged) {
        score = bow_l1_merge(A.db_ids, A.db_values, i0, i1, s_qi, s_qv, n_q);
      } else {
        score = bow_l1_merge(A.db_ids, A.db_values, i0, i1, q_ids, q_values, n_q);
      }
      if (A.scores) A.scores[(size_t)m * (size_t)E + (size_t)e] = score;
    }
    const bool listed = e < E && score != -1.0;  // (a score is -value / 2 with value <= 0, or a NaN: never -1 when listed)
    int total;
    const int rank = wave_rank(listed, lane, &total);
    if (lane == 0) s_cnt[0][wave] = total;
    __syncthreads();
    int off = 0, all = 0;
    for (int w = 0; w < kBowWaves; ++w) {
      off += w < wave ? s_cnt[0][w] : 0;
      all += s_cnt[0][w];
    }
    if (listed) {
      const int pos = n_l + off + rank;
      s_rid[pos & (kRing - 1)] = e;
      s_rsc[pos & (kRing - 1)] = score;
    }
    n_l += all;
    __syncthreads();
    decide(n_l - 2);
  }
  decide(n_l);
  if (tid == 0) {
    A.n_listed[m] = n_l;
    A.n_candidates[m] = n_c;
  }
}

// ---- database.add ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBowThreads) void bow_db_add_kernel(BowDbAddArgs A) {
  __shared__ long long s_part[kBowThreads];
  const int i_add = blockIdx.x, tid = threadIdx.x;
  // words of the entries of this call before this one, and including it
  long long before = 0;
  for (int t = tid; t < i_add; t += kBowThreads) {
    const int nw = A.q_n[A.add_index[t]];
    before += nw < 0 ? 0 : (nw > A.stride ? A.stride : nw);
  }
  s_part[tid] = before;
  __syncthreads();
  for (int s = kBowThreads / 2; s > 0; s >>= 1) {
    if (tid < s) s_part[tid] += s_part[tid + s];
    __syncthreads();
  }
  before = s_part[0];
  const int src = A.add_index[i_add];
  int nw = A.q_n[src];
  nw = nw < 0 ? 0 : (nw > A.stride ? A.stride : nw);
  const long long base = A.begin[A.n_entries];  // where the database ended before this call
  const bool fits = base + before + nw <= (long long)A.cap_words;
  const int e = A.n_entries + i_add;
  if (fits) {
    const long long at = base + before;
    const int32_t* q_ids = A.q_ids + (size_t)src * (size_t)A.stride;
    const double* q_values = A.q_values + (size_t)src * (size_t)A.stride;
    for (int j = tid; j < nw; j += kBowThreads) {
      A.ids[at + j] = q_ids[j];
      A.values[at + j] = q_values[j];
    }
    if (tid == 0) A.begin[e + 1] = (int32_t)(at + nw);
    return;
  }
  // this entry and all later ones of the call are stored empty: they end where the first that did not fit begins.  The
  // running sums grow, so that one is the first t with base + (words of 0 .. t) > cap_words.
  if (tid == 0) {
    long long run = base;
    for (int t = 0; t <= i_add; ++t) {
      int c = A.q_n[A.add_index[t]];
      c = c < 0 ? 0 : (c > A.stride ? A.stride : c);
      if (run + c > (long long)A.cap_words) break;
      run += c;
    }
    A.begin[e + 1] = (int32_t)run;
    atomicAdd(A.overflow, 1);
  }
}

}  // namespace

size_t bow_vectors_lds_bytes(int n_nodes, int keys_cap, bool* nodes_in_lds) {
  const size_t keys = (size_t)keys_cap * sizeof(uint32_t), nodes = (size_t)n_nodes * OKVFE_DESC_BYTES;
  *nodes_in_lds = n_nodes <= kVocLdsNodes && nodes + keys <= kBowLdsBudget;
  return keys + (*nodes_in_lds ? nodes : 0);
}

void launch_bow_vectors(const BowVectorsArgs& args, int n_multiframes, size_t lds_bytes, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  hipLaunchKernelGGL(bow_vectors_kernel, dim3(n_multiframes), dim3(kBowThreads), lds_bytes, stream, args);
}

void launch_place_query(const PlaceQueryArgs& args, int n_multiframes, bool dense, size_t lds_bytes, hipStream_t stream) {
  if (n_multiframes <= 0) return;
  hipLaunchKernelGGL(dense ? place_query_kernel<true> : place_query_kernel<false>, dim3(n_multiframes), dim3(kBowThreads),
                     lds_bytes, stream, args);
}

void launch_bow_db_add(const BowDbAddArgs& args, int n_add, hipStream_t stream) {
  if (n_add <= 0) return;
  hipLaunchKernelGGL(bow_db_add_kernel, dim3(n_add), dim3(kBowThreads), 0, stream, args);
}

}  // namespace okvfe
