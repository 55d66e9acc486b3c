// place_verify_cli.cpp -- drives the loop-closure verification of the C++ host mirror on frames that live on the device:
// okvfe::HipFrontend::placeLandmarkSet -> uploadPlaceSet -> verifyPlaceClaimsBlocks -> verifyPlaceConsensusBlocks, all on
// one stream with nothing waited for in between; from a binary request file.  Used by tests/test_gpu_place_verify_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold, min_inliers |
//           old frame { int32 n | ids n u64 | landmarks n*4 f64 | initialised n u8 | descriptors n*48 u8 } |
//           int32 n_frames, block_bytes | gather blocks n_frames*block_bytes u8 (host-packed) | T_SC 12 f64 |
//           int32 n_hyp, has_valid | hypotheses n_frames*n_hyp*12 f64 | flags n_frames*n_hyp u8 (if has_valid)
//           (a frame is a multiframe of one camera here)
// response: int32 L, rows | ids L u64 | hp L*4 f64 | desc_begin (L+1) i32 | pool rows*48 u8 |
//           k_min n_frames*L i32 | dist_min n_frames*L u32 | n_matches, n_points, n_correspondences n_frames i32 each |
//           gate n_frames u8 | match_landmark n_frames*K i32 | verdict n_frames u8 |
//           n_correspondences, best_hypothesis, n_inliers n_frames i32 each | accepted n_frames u8 |
//           hyp_inliers n_frames*n_hyp i32 | state n_frames*K u8 | distance n_frames*K f64 | landmark_out n_frames*K i32
//           (outputs start as 0xF9 bytes: rows the calls leave alone keep them) |
//           int32: 1 if a hypothesis count that does not fit made verifyPlaceConsensusBlocks throw
#include <array>
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
  int32_t par[3];
  rd(f, par, 3);
  int32_t n_old;
  rd(f, &n_old, 1);
  const size_t no = size_t(n_old);
  okvfe::FrameData old;
  old.keypoints.resize(no);
  old.landmarkIds = rdv<uint64_t>(f, no);
  const std::vector<double> old_hp = rdv<double>(f, no * 4);
  const std::vector<uint8_t> old_init = rdv<uint8_t>(f, no);
  old.descriptors.data = rdv<uint8_t>(f, no * 48);
  int32_t fn[2];
  rd(f, fn, 2);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]), K = size_t(par[0]);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes);
  okvfe_pose T_SC;
  rd(f, &T_SC, 1);
  int32_t hn[2];
  rd(f, hn, 2);
  const size_t n_hyp = size_t(hn[0]);
  std::vector<double> H = rdv<double>(f, nf * n_hyp * 12);
  const std::vector<uint8_t> valid = rdv<uint8_t>(f, hn[1] ? nf * n_hyp : 0);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    std::vector<std::array<double, 4>> lms(no);
    for (size_t i = 0; i < no; ++i) std::memcpy(lms[i].data(), old_hp.data() + 4 * i, 32);
    const okvfe::HipFrontend::PlaceLandmarkSet set = okvfe::HipFrontend::placeLandmarkSet({old}, {lms}, {old_init});
    const size_t L = set.ids.size();
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    DeviceBuffer d_blocks(nf * block_bytes), d_kmin(nf * L * 4), d_dmin(nf * L * 4), d_counts(nf * 12), d_gate(nf),
        d_ml(nf * K * 4), d_verdict(nf), d_head(nf * 12), d_acc(nf), d_hyp(nf * n_hyp * 4), d_state(nf * K),
        d_dist(nf * K * 8), d_out(nf * K * 4);
    if (okvfe_copy_to_device(d_blocks.d, blocks.data(), nf * block_bytes, nullptr) != OKVFE_OK ||
        okvfe_stream_synchronize(nullptr) != OKVFE_OK)
      return 5;
    const auto dev_set = frontend.uploadPlaceSet(0, set, stream);
    okvfe_place_claims_device claims{};
    claims.n_matches = d_counts.as<int32_t>();
    claims.n_points = d_counts.as<int32_t>() + nf;
    claims.n_correspondences = d_counts.as<int32_t>() + 2 * nf;
    claims.gate = d_gate.as<uint8_t>();
    claims.match_landmark = d_ml.as<int32_t>();
    frontend.verifyPlaceClaimsBlocks(0, *dev_set, d_blocks.d, int(nf), d_kmin.as<int32_t>(), d_dmin.as<uint32_t>(), par[2],
                                     claims, stream);
    okvfe_ransac_result_device res{};
    res.n_correspondences = d_head.as<int32_t>();
    res.best_hypothesis = d_head.as<int32_t>() + nf;
    res.n_inliers = d_head.as<int32_t>() + 2 * nf;
    res.accepted = d_acc.as<uint8_t>();
    res.hyp_inliers = d_hyp.as<int32_t>();
    res.state = d_state.as<uint8_t>();
    res.distance = d_dist.as<double>();
    res.landmark_out = d_out.as<int32_t>();
    frontend.verifyPlaceConsensusBlocks(0, *dev_set, d_blocks.d, int(nf), T_SC, d_ml.as<int32_t>(), d_gate.as<uint8_t>(), H,
                                        valid, int(n_hyp), par[2], res, d_verdict.as<uint8_t>(), 16.0, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const int32_t dims[2] = {int32_t(L), set.descBegin.back()};
    fwrite(dims, 4, 2, o);
    put(o, set.ids);
    put(o, set.hp);
    put(o, set.descBegin);
    put(o, set.pool);
    put(o, d_kmin.download<int32_t>(nf * L));
    put(o, d_dmin.download<uint32_t>(nf * L));
    put(o, d_counts.download<int32_t>(nf * 3));
    put(o, d_gate.download<uint8_t>(nf));
    put(o, d_ml.download<int32_t>(nf * K));
    put(o, d_verdict.download<uint8_t>(nf));
    put(o, d_head.download<int32_t>(nf * 3));
    put(o, d_acc.download<uint8_t>(nf));
    put(o, d_hyp.download<int32_t>(nf * n_hyp));
    put(o, d_state.download<uint8_t>(nf * K));
    put(o, d_dist.download<double>(nf * K));
    put(o, d_out.download<int32_t>(nf * K));
    // error behaviour: nHyp hypotheses per multiframe, or the call throws before anything is launched
    int32_t threw = 0;
    H.push_back(0.0);
    try {
      frontend.verifyPlaceConsensusBlocks(0, *dev_set, d_blocks.d, int(nf), T_SC, d_ml.as<int32_t>(), nullptr, H, valid,
                                          int(n_hyp), par[2], res, d_verdict.as<uint8_t>(), 16.0, stream);
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
