// bow_dev.h -- the device pieces of the DBoW2 query path that exist once: the 384-bit descriptor in registers, the
// vocabulary descent with the FBrisk trait and the L1 score of two BowVectors.  Compiled into the B = 1 kernels of
// k_match.hip (voc_transform_kernel, bow_query_l1_kernel) and into the batched ones of k_bow.hip.
#pragma once
#include "okvfe_internal.h"

namespace okvfe {
namespace {

struct Desc12 {
  uint32_t w[12];
};

__device__ __forceinline__ Desc12 load_desc(const uint8_t* p) {
  Desc12 d;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1], c = q[2];
  d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w;
  d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
  d.w[8] = c.x; d.w[9] = c.y; d.w[10] = c.z; d.w[11] = c.w;
  return d;
}

__device__ __forceinline__ int hamming(const Desc12& a, const uint32_t* __restrict__ b) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) c += __popc(a.w[i] ^ b[i]);
  return c;
}

// ---- DBoW2 vocabulary descent with the FBrisk trait (oracle: orc_voc_transform) ----------------
// The node descriptors (819 x 48 B for the shipped 9^3 vocabulary) sit in LDS when they fit.  At every level the child
// with the smallest Hamming distance wins, the first on ties.  -> the leaf's node id
constexpr int kVocLdsNodes = 1024;
__device__ __forceinline__ int voc_descend(const Desc12& a, const uint4* lds_nodes, bool in_lds,
                                           const uint8_t* __restrict__ node_desc,
                                           const int32_t* __restrict__ child_begin,
                                           const int32_t* __restrict__ child_index) {
  int node = 0;
  while (true) {
    const int c0 = child_begin[node], c1 = child_begin[node + 1];
    if (c1 <= c0) break;
    int best = -1, best_d = 0x7FFFFFFF;
    for (int c = c0; c < c1; ++c) {
      const int id = child_index[c];
      const uint32_t* row = in_lds ? reinterpret_cast<const uint32_t*>(lds_nodes + 3 * id)
                                   : reinterpret_cast<const uint32_t*>(node_desc + (size_t)id * OKVFE_DESC_BYTES);
      const int d = hamming(a, row);
      if (d < best_d) {
        best_d = d;
        best = id;
      }
    }
    node = best;
  }
  return node;
}

// ---- DBoW2 L1 score (TemplatedDatabase::queryL1) -------------------------------------------------
// one common word: value += |q - d| - |q| - |d|, in these three steps
__device__ __forceinline__ double bow_l1_term(double value, double q, double d) {
  double t = fabs(q - d);
  t = t - fabs(q);
  t = t - fabs(d);
  return value + t;
}
// Merge-join of a stored BowVector [i, i_end) with the query's (both in ascending word order) over the common words in
// that order -- the order in which the reference's inverted-file walk reaches this entry.  -> score = -value / 2, or
// -1 without a common word (DBoW2 does not list the entry then).
__device__ __forceinline__ double bow_l1_merge(const int32_t* __restrict__ db_ids, const double* __restrict__ db_values,
                                               int i, int i_end, const int32_t* q_ids, const double* q_values, int n_q) {
  int j = 0;
  double value = 0.0;
  bool any = false;
  while (i < i_end && j < n_q) {
    const int a = db_ids[i], b = q_ids[j];
    if (a == b) {
      value = bow_l1_term(value, q_values[j], db_values[i]);
      any = true;
      ++i;
      ++j;
    } else if (a < b) {
      ++i;
    } else {
      ++j;
    }
  }
  return any ? -value / 2.0 : -1.0;
}

}  // namespace
}  // namespace okvfe
