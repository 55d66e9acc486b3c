// ransac_hyp_cli.cpp -- drives the pose hypotheses of the C++ host mirror on frames that live on the device:
// okvfe::HipFrontend::ransacHypothesesBlocks (the matchToMap policy, against an uploaded landmark table) and
// verifyPlaceHypothesesBlocks (the loop-closure policy, against an uploaded place set of the same landmarks, with a
// gate), both on one stream with nothing waited for in between; from a binary request file.  Used by
// tests/test_gpu_ransac_hyp_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, nl, n_frames, block_bytes, n_hyp, with_keys |
//           hp nl*4 f64 | obs_begin (nl+1) i32 | gather blocks n_frames*block_bytes u8 (host-packed) | landmark rows
//           n_frames*K i32 | gate n_frames u8 | T_SC 12 f64 | uint64 seed | keys n_frames u64 (read if with_keys)
//           (a frame is a multiframe of one camera here)
// response: for each of the two calls: hypotheses n_frames*n_hyp*12 f64 | hyp_valid n_frames*n_hyp u8 |
//           n_correspondences n_frames i32 | samples n_frames*n_hyp*4 i32 | n_solutions n_frames*n_hyp i32
//           (outputs start as 0xF9 bytes) | int32: 1 if n_hyp = 65 made ransacHypothesesBlocks throw
#include <cstdio>
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
  int32_t par[6];
  rd(f, par, 6);
  const size_t K = size_t(par[0]), nl = size_t(par[1]), nf = size_t(par[2]), block_bytes = size_t(par[3]), nh = size_t(par[4]);
  const std::vector<double> hp = rdv<double>(f, nl * 4);
  const std::vector<int32_t> obs_begin = rdv<int32_t>(f, nl + 1);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes);
  const std::vector<int32_t> rows = rdv<int32_t>(f, nf * K);
  const std::vector<uint8_t> gate = rdv<uint8_t>(f, nf);
  okvfe_pose T_SC;
  rd(f, &T_SC, 1);
  uint64_t seed;
  rd(f, &seed, 1);
  const std::vector<uint64_t> keys = rdv<uint64_t>(f, par[5] ? nf : 0);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    // the table: the observations themselves are not read by these calls, only their counts
    const size_t no = size_t(obs_begin[nl]);
    const std::vector<double> quality(nl + 1, 0.0), obs_bp(no * 3 + 1, 0.0);
    const std::vector<int32_t> obs_pose(no + 1, 0);
    const std::vector<uint8_t> obs_desc(no * 48 + 1, 0);
    okvfe_pose identity{};
    identity.C[0] = identity.C[4] = identity.C[8] = 1.0;
    okvfe_landmark_table table{int32_t(nl), int32_t(no), 1, hp.data(), quality.data(), obs_begin.data(), obs_pose.data(),
                               obs_desc.data(), obs_bp.data(), &identity};
    const auto dev_table = frontend.uploadLandmarkTable(0, table);
    okvfe::HipFrontend::PlaceLandmarkSet set;
    set.ids.resize(nl);
    for (size_t l = 0; l < nl; ++l) set.ids[l] = l + 1;
    set.hp = hp;
    set.descBegin.assign(nl + 1, 0);
    const auto dev_set = frontend.uploadPlaceSet(0, set);
    DeviceBuffer d_blocks(nf * block_bytes), d_rows(nf * K * 4), d_gate(nf), d_keys(nf * 8);
    d_blocks.upload(blocks);
    d_rows.upload(rows);
    d_gate.upload(gate);
    d_keys.upload(keys);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    const uint64_t* keys_dev = par[5] ? d_keys.as<uint64_t>() : nullptr;
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    DeviceBuffer h0(nf * nh * 96), v0(nf * nh), c0(nf * 4), s0(nf * nh * 16), n0(nf * nh * 4);
    DeviceBuffer h1(nf * nh * 96), v1(nf * nh), c1(nf * 4), s1(nf * nh * 16), n1(nf * nh * 4);
    const okvfe_ransac_hypotheses_device r0{h0.as<double>(), v0.as<uint8_t>(), c0.as<int32_t>(), s0.as<int32_t>(), n0.as<int32_t>()};
    const okvfe_ransac_hypotheses_device r1{h1.as<double>(), v1.as<uint8_t>(), c1.as<int32_t>(), s1.as<int32_t>(), n1.as<int32_t>()};
    frontend.ransacHypothesesBlocks(0, *dev_table, d_blocks.d, int(nf), T_SC, d_rows.as<int32_t>(), keys_dev, seed, int(nh), r0,
                                    stream);
    frontend.verifyPlaceHypothesesBlocks(0, *dev_set, d_blocks.d, int(nf), T_SC, d_rows.as<int32_t>(), d_gate.as<uint8_t>(),
                                         keys_dev, seed, int(nh), r1, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const DeviceBuffer* const outs[2][5] = {{&h0, &v0, &c0, &s0, &n0}, {&h1, &v1, &c1, &s1, &n1}};
    for (const auto& b : outs) {
      put(o, b[0]->download<double>(nf * nh * 12));
      put(o, b[1]->download<uint8_t>(nf * nh));
      put(o, b[2]->download<int32_t>(nf));
      put(o, b[3]->download<int32_t>(nf * nh * 4));
      put(o, b[4]->download<int32_t>(nf * nh));
    }
    int32_t threw = 0;
    try {
      frontend.ransacHypothesesBlocks(0, *dev_table, d_blocks.d, int(nf), T_SC, d_rows.as<int32_t>(), keys_dev, seed,
                                      OKVFE_RANSAC_MAX_HYPOTHESES + 1, r0, stream);
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
