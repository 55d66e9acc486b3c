// capi_bow.cpp -- place recognition on device-resident batches behind the C ABI: what dBow_->database.query and
// database.add do (Frontend.cpp:660-672, :752-766, :896-898) with the vocabulary and the database in device memory, and
// the estimator-free part of the walk over the results (:771-802).  Kernels: k_bow.hip.
#include "okvfe_ctx.h"

using namespace okvfe;

namespace {
bool vectors_ok(const okvfe_bow_vectors_device* v) {
  return v && v->n_words && v->ids && v->values && v->stride >= 1 && v->n_vocabulary_words >= 0;
}
bool database_ok(const okvfe_bow_database_device* d) {
  return d && d->begin && d->cap_entries >= 0 && d->cap_words >= 0 && d->n_entries >= 0 && d->n_entries <= d->cap_entries &&
         (d->cap_words == 0 || (d->ids && d->values));
}
}  // namespace

extern "C" {

okvfe_status okvfe_vocabulary_check(const okvfe_vocabulary_device* v) {
  const char* who = "okvfe_vocabulary_check";
  if (!v || v->n_nodes < 1 || v->n_words < 1 || !v->node_descriptors || !v->child_begin || !v->node_word || !v->word_weight)
    return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
  if (v->weighting < 0 || v->weighting > 3)
    return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: weighting %d is not one of 0..3", who, v->weighting);
  const int n = v->n_nodes;
  if (v->child_begin[0] != 0) return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: child_begin[0] != 0", who);
  for (int i = 0; i < n; ++i)
    if (v->child_begin[i + 1] < v->child_begin[i])
      return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: child_begin not monotone at %d", who, i);
  if (v->child_begin[n] > 0 && !v->child_index) return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: null children", who);
  // nodes are numbered so that a parent precedes its children: one pass reaches what can be reached
  std::vector<uint8_t> reached((size_t)n, 0);
  reached[0] = 1;
  for (int i = 0; i < n; ++i)
    for (int c = v->child_begin[i]; c < v->child_begin[i + 1]; ++c) {
      const int id = v->child_index[c];
      if (id <= i || id >= n)
        return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: node %d has child %d (not a tree in id order)", who, i, id);
      if (reached[(size_t)id])
        return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: node %d is the child of two nodes", who, id);
      if (!reached[(size_t)i])
        return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: node %d has children but is not reachable from the root", who, i);
      reached[(size_t)id] = 1;
    }
  for (int i = 0; i < n; ++i) {
    if (!reached[(size_t)i])
      return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: node %d is not reachable from the root", who, i);
    const bool leaf = v->child_begin[i + 1] == v->child_begin[i];
    const int w = v->node_word[i];
    if (leaf && (w < 0 || w >= v->n_words))
      return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: leaf %d has word %d outside [0, %d)", who, i, w, v->n_words);
    if (!leaf && w >= 0)
      return fail(nullptr, OKVFE_ERR_INVALID_ARGUMENT, "%s: inner node %d carries word %d", who, i, w);
  }
  return OKVFE_OK;
}

okvfe_status okvfe_bow_vectors_blocks_device(okvfe_ctx* ctx, const okvfe_vocabulary_device* voc, const void* blocks_dev,
                                             int32_t n_multiframes, int32_t n_cams, const okvfe_bow_vectors_device* vectors,
                                             int32_t* word_ids_dev, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  const char* who = "okvfe_bow_vectors_blocks_device";
  if (!voc || voc->n_nodes < 1 || voc->n_words < 1 || voc->weighting < 0 || voc->weighting > 3 || !voc->node_descriptors ||
      !voc->child_begin || !voc->node_word || !voc->word_weight || (voc->n_nodes > 1 && !voc->child_index) || !blocks_dev ||
      n_multiframes < 0 || n_cams < 1 || !vectors_ok(vectors))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
  const int64_t features = (int64_t)n_cams * ctx->kp_cap;
  if (features > kBowMaxFeatures)
    return fail(ctx, OKVFE_ERR_UNSUPPORTED, "%s: n_cams x max_keypoints = %lld exceeds the %d features a multiframe's sort holds",
                who, (long long)features, kBowMaxFeatures);
  if (vectors->stride < std::min<int64_t>(features, voc->n_words))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: stride %d is below min(n_cams x max_keypoints, n_words) = %lld", who,
                vectors->stride, (long long)std::min<int64_t>(features, voc->n_words));
  if ((int64_t)n_multiframes * n_cams >= (int64_t)1 << 30) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: too many blocks", who);
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  const BlockLayout L = block_layout(ctx->kp_cap);
  int keys_cap = 256;
  while (keys_cap < features) keys_cap <<= 1;
  BowVectorsArgs A{};
  A.node_desc = voc->node_descriptors; A.child_begin = voc->child_begin; A.child_index = voc->child_index;
  A.node_word = voc->node_word; A.word_weight = voc->word_weight;
  A.n_nodes = voc->n_nodes; A.n_words = voc->n_words; A.weighting = voc->weighting; A.normalise_l1 = voc->normalise_l1 ? 1 : 0;
  bool in_lds = false;
  const size_t lds = bow_vectors_lds_bytes(voc->n_nodes, keys_cap, &in_lds);
  A.nodes_in_lds = in_lds ? 1 : 0;
  A.blocks = static_cast<const uint8_t*>(blocks_dev);
  A.o_count = (int)L.o_count; A.o_desc = (int)L.o_desc; A.block_bytes = L.total;
  A.kp_cap = ctx->kp_cap; A.n_cams = n_cams;
  A.n_out = vectors->n_words; A.ids = vectors->ids; A.values = vectors->values; A.stride = vectors->stride;
  A.word_ids = word_ids_dev;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_bow_vectors(A, n_multiframes, lds, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_place_query_blocks_device(okvfe_ctx* ctx, const okvfe_bow_database_device* db,
                                             const okvfe_bow_vectors_device* vectors, int32_t n_multiframes, double min_score,
                                             const uint8_t* suppressible_dev, double* scores_dev,
                                             const okvfe_place_candidates_device* result, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  const char* who = "okvfe_place_query_blocks_device";
  if (!database_ok(db) || !vectors_ok(vectors) || n_multiframes < 0 || !result || !result->n_listed || !result->n_candidates ||
      result->cap < 0 || (result->cap > 0 && (!result->entry || !result->score)))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
  if (n_multiframes == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  PlaceQueryArgs A{};
  A.db_begin = db->begin; A.db_ids = db->ids; A.db_values = db->values; A.n_entries = db->n_entries;
  A.q_n = vectors->n_words; A.q_ids = vectors->ids; A.q_values = vectors->values; A.stride = vectors->stride;
  const bool dense = vectors->n_vocabulary_words > 0 && vectors->n_vocabulary_words <= kBowDenseWords;
  A.n_vocab = dense ? vectors->n_vocabulary_words : 0;
  A.lds_values = dense ? std::min(vectors->stride, vectors->n_vocabulary_words) : std::min(vectors->stride, kBowQueryLdsWords);
  const size_t lds = (size_t)A.lds_values * sizeof(double) + (size_t)(dense ? A.n_vocab : A.lds_values) * sizeof(int32_t);
  A.min_score = min_score; A.suppressible = suppressible_dev; A.scores = scores_dev;
  A.n_listed = result->n_listed; A.n_candidates = result->n_candidates; A.entry = result->entry; A.score = result->score;
  A.cap = result->cap;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_place_query(A, n_multiframes, dense, lds, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->last_stream = s;
  return OKVFE_OK;
}

okvfe_status okvfe_bow_database_add_blocks_device(okvfe_ctx* ctx, okvfe_bow_database_device* db,
                                                  const okvfe_bow_vectors_device* vectors, int32_t n_multiframes,
                                                  const int32_t* add_index, int32_t n_add, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  const char* who = "okvfe_bow_database_add_blocks_device";
  if (!database_ok(db) || !db->overflow || !vectors_ok(vectors) || n_multiframes < 0 || n_add < 0 || (n_add > 0 && !add_index))
    return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
  for (int i = 0; i < n_add; ++i)
    if (add_index[i] < 0 || add_index[i] >= n_multiframes || (i > 0 && add_index[i] <= add_index[i - 1]))
      return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "%s: add_index[%d] = %d (strictly ascending indices in [0, %d))", who, i,
                  add_index[i], n_multiframes);
  if ((int64_t)db->n_entries + n_add > db->cap_entries)
    return fail(ctx, OKVFE_ERR_CAPACITY, "%s: %d entries + %d exceed cap_entries = %d", who, db->n_entries, n_add, db->cap_entries);
  if (n_add == 0) return OKVFE_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  RingSlot index(ctx, &ctx->pair_ring, s);
  okvfe_status st = index.upload(add_index, (size_t)n_add * sizeof(int32_t));
  if (st != OKVFE_OK) return st;
  BowDbAddArgs A{};
  A.add_index = index.as<int32_t>();
  A.q_n = vectors->n_words; A.q_ids = vectors->ids; A.q_values = vectors->values; A.stride = vectors->stride;
  A.begin = db->begin; A.ids = db->ids; A.values = db->values; A.n_entries = db->n_entries; A.cap_words = db->cap_words;
  A.overflow = db->overflow;
  {
    StageTimer t(ctx, OKVFE_STAGE_MAP, s);
    launch_bow_db_add(A, n_add, s);
  }
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = index.release();
  db->n_entries += n_add;
  ctx->last_stream = s;
  return rel;
}

okvfe_status okvfe_bow_database_check_device(okvfe_ctx* ctx, const okvfe_bow_database_device* db, void* stream) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!db || !db->overflow) return fail(ctx, OKVFE_ERR_INVALID_ARGUMENT, "okvfe_bow_database_check_device: bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->cfg.device));
  hipStream_t s = pick_stream(ctx, stream);
  int32_t overflow = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&overflow, db->overflow, sizeof(overflow), hipMemcpyDeviceToHost, s));
  HIP_TRY(ctx, hipStreamSynchronize(s));
  if (overflow != 0)
    return fail(ctx, OKVFE_ERR_CAPACITY, "okvfe_bow_database_check_device: %d entries were stored empty: ids / values are full",
                overflow);
  return OKVFE_OK;
}

}  // extern "C"
