// stereo_insert_cli.cpp -- drives matchStereo's landmark bookkeeping of the C++ host mirror on multiframes that live on
// the device: okvfe::HipFrontend::matchStereoInsertBlocks on given matcher rows (mode 0), or matchStereoRig -- the
// matcher for every pair, then the bookkeeping, on one stream with nothing waited for in between (mode 1); from a
// binary request file.  Used by tests/test_gpu_stereo_insert.py and tools/bench_stereo_insert.py.
// request : int32 n_cams, w, h, K, match threshold, n_multiframes, n_pairs, stride_m, stride_c, L, mode, has_keyframe |
//           cameras n_cams x { int32 dist, pad | f64 fu, fv, cu, cv, d[8] } | pairs n_pairs*2 i32 | hp L*4 f64 |
//           initialised L u8 | T_WC n_multiframes*n_cams*12 f64 | int32 block_bytes | gather blocks
//           n_multiframes*n_cams*block_bytes u8 (host-packed, at their strided places) | landmark
//           n_multiframes*n_cams*K i32 | keyframe n_multiframes u8 (if has_keyframe) | matches
//           n_pairs*n_multiframes*K*48 u8 (mode 0)
// response: action n_pairs*n_multiframes*K u8 | lm the same i32 | landmark_out n_multiframes*n_cams*K i32 | counts
//           n_multiframes*4 i32 (outputs start as 0xF9 bytes: rows the call leaves alone keep them) | matches
//           n_pairs*n_multiframes*K*48 u8 (mode 1) | int32: 1 if a pose count that does not fit made the call throw
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
  const std::vector<int32_t> h = rdv<int32_t>(f, 12);
  const size_t nc = size_t(h[0]), K = size_t(h[3]), nm = size_t(h[5]), np = size_t(h[6]), L = size_t(h[9]);
  const int mode = h[10];
  std::vector<okvfe_camera_ext> cams(nc);
  for (size_t c = 0; c < nc; ++c) {
    const std::vector<int32_t> ci = rdv<int32_t>(f, 2);
    const std::vector<double> cd = rdv<double>(f, 12);
    okvfe_camera_ext& e = cams[c];
    e = okvfe_camera_ext{};
    e.base.width = h[1]; e.base.height = h[2]; e.base.distortion = ci[0];
    e.base.fu = cd[0]; e.base.fv = cd[1]; e.base.cu = cd[2]; e.base.cv = cd[3];
    for (int i = 0; i < 4; ++i) e.base.d[i] = cd[4 + size_t(i)], e.d_ext[i] = cd[8 + size_t(i)];
  }
  const std::vector<int32_t> pair_list = rdv<int32_t>(f, np * 2);
  std::vector<std::array<int32_t, 2>> pairs(np);
  for (size_t p = 0; p < np; ++p) pairs[p] = {pair_list[2 * p], pair_list[2 * p + 1]};
  const std::vector<double> hp = rdv<double>(f, L * 4);
  const std::vector<uint8_t> initialised = rdv<uint8_t>(f, L);
  std::vector<okvfe_pose> T_WC = rdv<okvfe_pose>(f, nm * nc);
  const size_t bb = size_t(rdv<int32_t>(f, 1)[0]);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nm * nc * bb);
  const std::vector<int32_t> landmark = rdv<int32_t>(f, nm * nc * K);
  const std::vector<uint8_t> keyframe = rdv<uint8_t>(f, h[11] ? nm : 0);
  const std::vector<uint8_t> matches = rdv<uint8_t>(f, mode == 0 ? np * nm * K * sizeof(okvfe_stereo_match) : 0);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = h[3];
    p.matching_threshold = h[4];
    okvfe::HipFrontend frontend(cams, p);
    if (size_t(frontend.rigMaxKeypoints()) != K || frontend.rigBlockBytes() != bb) {
      fprintf(stderr, "the request was packed for another row capacity\n");
      return 3;
    }
    const std::vector<double> quality(L + 1, 0.0);
    const std::vector<int32_t> obs_begin(L + 1, 0);
    okvfe_landmark_table table{int32_t(L), 0, 0, hp.data(), quality.data(), obs_begin.data(), nullptr, nullptr, nullptr, nullptr};
    const auto dev_table = frontend.uploadLandmarkTable(0, table);
    const size_t rows = np * nm * K;
    DeviceBuffer d_init(L), d_blocks(nm * nc * bb), d_lm(nm * nc * K * 4), d_kf(nm), d_matches(rows * sizeof(okvfe_stereo_match)),
        d_action(rows), d_lmrow(rows * 4), d_out(nm * nc * K * 4), d_counts(nm * 16);
    d_init.upload(initialised);
    d_blocks.upload(blocks);
    d_lm.upload(landmark);
    d_kf.upload(keyframe);
    d_matches.upload(matches);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    okvfe_stereo_insert_device res{};
    res.action = d_action.as<uint8_t>();
    res.lm = d_lmrow.as<int32_t>();
    res.landmark_out = d_out.as<int32_t>();
    res.counts = d_counts.as<int32_t>();
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    const uint8_t* kf = h[11] ? d_kf.as<uint8_t>() : nullptr;
    if (mode == 0)
      frontend.matchStereoInsertBlocks(*dev_table, d_init.as<uint8_t>(), d_blocks.d, h[7], h[8], int(nm), pairs, T_WC,
                                       d_matches.as<okvfe_stereo_match>(), d_lm.as<int32_t>(), kf, res, stream);
    else
      frontend.matchStereoRig(*dev_table, d_init.as<uint8_t>(), d_blocks.d, h[7], h[8], int(nm), pairs, T_WC,
                              d_matches.as<okvfe_stereo_match>(), d_lm.as<int32_t>(), kf, res, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, d_action.download<uint8_t>(rows));
    put(o, d_lmrow.download<uint8_t>(rows * 4));
    put(o, d_out.download<uint8_t>(nm * nc * K * 4));
    put(o, d_counts.download<uint8_t>(nm * 16));
    if (mode != 0) put(o, d_matches.download<uint8_t>(rows * sizeof(okvfe_stereo_match)));
    // error behaviour: one pose per (multiframe, camera), or the call throws before anything is launched
    int32_t threw = 0;
    T_WC.push_back(okvfe_pose{});
    try {
      frontend.matchStereoInsertBlocks(*dev_table, d_init.as<uint8_t>(), d_blocks.d, h[7], h[8], int(nm), pairs, T_WC,
                                       d_matches.as<okvfe_stereo_match>(), d_lm.as<int32_t>(), kf, res, stream);
    } catch (const okvfe::Exception& e) {
      threw = e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
    }
    okvfe_stream_destroy(stream);
    fwrite(&threw, 4, 1, o);
    fclose(o);
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
