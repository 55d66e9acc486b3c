// place_query_cli.cpp -- drives place recognition through the C++ host mirror on frames that live on the device:
// okvfe::HipFrontend::uploadVocabulary -> bowVectorsBlocks -> placeDatabaseAdd -> placeQueryBlocks, all on one stream
// with nothing waited for in between; from a binary request file.  Used by tests/test_gpu_place_query_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K |
//           vocabulary { int32 n_nodes, n_words, n_children, weighting, normalise_l1 | node descriptors n_nodes*48 u8 |
//                        child_begin (n_nodes+1) i32 | child_index n_children i32 | node_word n_nodes i32 |
//                        word_weight n_words f64 } |
//           int32 n_frames, block_bytes | gather blocks n_frames*block_bytes u8 (host-packed; a frame is a multiframe of
//           one camera here) | int32 n_add | add_index n_add i32 | int32 cap, has_suppressible | f64 min_score |
//           suppressible n_add u8 (if has_suppressible)
// response: int32 stride | n_words n_frames i32 | ids n_frames*stride i32 | values n_frames*stride f64 |
//           word_ids n_frames*K i32 | begin (n_add+1) i32 | n_listed, n_candidates n_frames i32 each |
//           entry n_frames*cap i32 | score n_frames*cap f64 | scores n_frames*n_add f64
//           (outputs start as 0xF9 bytes: rows the calls leave alone keep them) |
//           int32: 1 if one more add into the full database threw OKVFE_ERR_CAPACITY and left the entry count alone |
//           int32: 1 if a malformed vocabulary (the last entry of child_begin lowered by one) made uploadVocabulary throw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#include "cli_io.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  okvfe_camera cam{};
  int32_t ci[3];
  rd(f, ci, 3);
  cam.width = ci[0]; cam.height = ci[1]; cam.distortion = ci[2];
  double cd[8];
  rd(f, cd, 8);
  cam.fu = cd[0]; cam.fv = cd[1]; cam.cu = cd[2]; cam.cv = cd[3];
  for (int i = 0; i < 4; ++i) cam.d[i] = cd[4 + i];
  int32_t K32;
  rd(f, &K32, 1);
  int32_t vn[5];
  rd(f, vn, 5);
  okvfe::HipFrontend::Vocabulary voc;
  voc.nodeDescriptors = rdv<uint8_t>(f, size_t(vn[0]) * 48);
  voc.childBegin = rdv<int32_t>(f, size_t(vn[0]) + 1);
  voc.childIndex = rdv<int32_t>(f, size_t(vn[2]));
  voc.nodeWord = rdv<int32_t>(f, size_t(vn[0]));
  voc.wordWeight = rdv<double>(f, size_t(vn[1]));
  voc.weighting = vn[3];
  voc.normaliseL1 = vn[4] != 0;
  int32_t fn[2];
  rd(f, fn, 2);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]), K = size_t(K32);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes);
  int32_t n_add;
  rd(f, &n_add, 1);
  const std::vector<int32_t> add_index = rdv<int32_t>(f, size_t(n_add));
  int32_t cs[2];
  rd(f, cs, 2);
  double min_score;
  rd(f, &min_score, 1);
  const std::vector<uint8_t> suppressible = rdv<uint8_t>(f, cs[1] ? size_t(n_add) : 0);
  fclose(f);
  const size_t cap = size_t(cs[0]), na = size_t(n_add);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = K32;
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    DeviceBuffer d_blocks(nf * block_bytes), d_words(nf * K * 4), d_counts(nf * 8), d_entry(nf * cap * 4),
        d_score(nf * cap * 8), d_scores(nf * na * 8), d_supp(na);
    if (okvfe_copy_to_device(d_blocks.d, blocks.data(), nf * block_bytes, nullptr) != OKVFE_OK ||
        (!suppressible.empty() && okvfe_copy_to_device(d_supp.d, suppressible.data(), na, nullptr) != OKVFE_OK) ||
        okvfe_stream_synchronize(nullptr) != OKVFE_OK)
      return 5;
    const auto dev_voc = frontend.uploadVocabulary(0, voc, stream);
    const auto vectors = frontend.allocBowVectors(0, *dev_voc, int(nf));
    const size_t stride = size_t(vectors->get().stride);
    // (the rows start as 0xF9 bytes like every other output)
    if (okvfe_device_fill(vectors->get().n_words, 0xF9, nf * 4, stream) != OKVFE_OK ||
        okvfe_device_fill(vectors->get().ids, 0xF9, nf * stride * 4, stream) != OKVFE_OK ||
        okvfe_device_fill(vectors->get().values, 0xF9, nf * stride * 8, stream) != OKVFE_OK)
      return 5;
    const auto db = frontend.createPlaceDatabase(0, n_add, int(na * stride), stream);
    frontend.bowVectorsBlocks(0, *dev_voc, d_blocks.d, int(nf), *vectors, d_words.as<int32_t>(), stream);
    frontend.placeDatabaseAdd(0, *db, *vectors, int(nf), add_index, stream);
    okvfe_place_candidates_device res{};
    res.n_listed = d_counts.as<int32_t>();
    res.n_candidates = d_counts.as<int32_t>() + nf;
    res.entry = d_entry.as<int32_t>();
    res.score = d_score.as<double>();
    res.cap = int32_t(cap);
    frontend.placeQueryBlocks(0, *db, *vectors, int(nf), res, min_score,
                              suppressible.empty() ? nullptr : d_supp.as<uint8_t>(), d_scores.as<double>(), stream);
    frontend.placeDatabaseCheck(0, *db, stream);  // (synchronises the stream)
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const int32_t s32 = int32_t(stride);
    fwrite(&s32, 4, 1, o);
    put(o, download<int32_t>(vectors->get().n_words, nf));
    put(o, download<int32_t>(vectors->get().ids, nf * stride));
    put(o, download<double>(vectors->get().values, nf * stride));
    put(o, download<int32_t>(d_words.d, nf * K));
    put(o, download<int32_t>(db->get().begin, na + 1));
    put(o, download<int32_t>(d_counts.d, nf * 2));
    put(o, download<int32_t>(d_entry.d, nf * cap));
    put(o, download<double>(d_score.d, nf * cap));
    put(o, download<double>(d_scores.d, nf * na));
    int32_t threw = 0;
    try {
      frontend.placeDatabaseAdd(0, *db, *vectors, int(nf), std::vector<int32_t>{0}, stream);
    } catch (const okvfe::Exception& e) {
      threw = e.status == OKVFE_ERR_CAPACITY && db->entries() == n_add ? 1 : 0;
    }
    fwrite(&threw, 4, 1, o);
    threw = 0;
    if (vn[0] > 1 && !voc.childIndex.empty()) {
      okvfe::HipFrontend::Vocabulary bad = voc;
      bad.childBegin.back() -= 1;  // no longer monotone, or the last child listed is nobody's child
      try {
        frontend.uploadVocabulary(0, bad, stream);
      } catch (const okvfe::Exception& e) {
        threw = e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
      }
    }
    fwrite(&threw, 4, 1, o);
    fclose(o);
    okvfe_stream_synchronize(stream);
    okvfe_stream_destroy(stream);
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
