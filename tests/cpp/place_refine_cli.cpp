// place_refine_cli.cpp -- drives okvfe::HipFrontend::verifyPlaceRefineBlocks of the C++ host mirror on frames that live
// on the device (the refinement of T_Sold_Snew of Frontend::verifyRecognisedPlace and H at the pose out), from a binary
// request file.  Used by tests/test_gpu_place_refine.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, L | hp L*4 f64 |
//           int32 n_frames, block_bytes | gather blocks n_frames*block_bytes u8 (host-packed) | T_SC 7 f64 (t, qx qy qz qw) |
//           int32 n_hyp, max_iterations | hypotheses n_frames*n_hyp*12 f64 | best n_frames i32 |
//           match_landmark n_frames*K i32 | state n_frames*K u8 | int32 has_verdict |
//           verdict n_frames u8 (if has_verdict)          (a frame is a multiframe of one camera here)
// response: poses, start_poses n_frames*7 f64 each | cost n_frames*2 f64 | H n_frames*36 f64 |
//           status, n_iterations, n_accepted, n_terms, n_singular n_frames i32 each
//           (outputs start as 0xF9 bytes: rows the call leaves alone keep them) |
//           int32: 1 if a negative number of multiframes made verifyPlaceRefineBlocks throw
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
  int32_t par[2];
  rd(f, par, 2);
  const size_t K = size_t(par[0]), L = size_t(par[1]);
  okvfe::HipFrontend::PlaceLandmarkSet set;
  set.hp = rdv<double>(f, L * 4);
  set.ids.resize(L);
  for (size_t l = 0; l < L; ++l) set.ids[l] = 1 + l;
  set.descBegin.assign(L + 1, 0);  // (no descriptors: the call reads the landmarks only)
  int32_t fn[2];
  rd(f, fn, 2);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes);
  std::array<double, 7> T_SC;
  rd(f, T_SC.data(), 7);
  int32_t hi[2];
  rd(f, hi, 2);
  const size_t n_hyp = size_t(hi[0]);
  const std::vector<double> hyp = rdv<double>(f, nf * n_hyp * 12);
  const std::vector<int32_t> best = rdv<int32_t>(f, nf);
  const std::vector<int32_t> ml = rdv<int32_t>(f, nf * K);
  const std::vector<uint8_t> state = rdv<uint8_t>(f, nf * K);
  int32_t has_verdict;
  rd(f, &has_verdict, 1);
  const std::vector<uint8_t> verdict = rdv<uint8_t>(f, has_verdict ? nf : 0);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    DeviceBuffer d_blocks(nf * block_bytes), d_hyp(nf * n_hyp * 96), d_best(nf * 4), d_ml(nf * K * 4), d_state(nf * K),
        d_verdict(nf), d_poses(nf * 56), d_start(nf * 56), d_cost(nf * 16), d_H(nf * 288), d_counts(nf * 20);
    d_blocks.upload(blocks);
    d_hyp.upload(hyp);
    d_best.upload(best);
    d_ml.upload(ml);
    d_state.upload(state);
    d_verdict.upload(verdict);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    const auto dev_set = frontend.uploadPlaceSet(0, set, stream);
    okvfe_place_refine_device res{};
    res.poses = d_poses.as<double>();
    res.start_poses = d_start.as<double>();
    res.cost = d_cost.as<double>();
    res.H = d_H.as<double>();
    res.status = d_counts.as<int32_t>();
    res.n_iterations = d_counts.as<int32_t>() + nf;
    res.n_accepted = d_counts.as<int32_t>() + 2 * nf;
    res.n_terms = d_counts.as<int32_t>() + 3 * nf;
    res.n_singular = d_counts.as<int32_t>() + 4 * nf;
    const uint8_t* v = has_verdict ? d_verdict.as<uint8_t>() : nullptr;
    frontend.verifyPlaceRefineBlocks(0, *dev_set, d_blocks.d, int(nf), T_SC, d_hyp.as<double>(), int(n_hyp),
                                     d_best.as<int32_t>(), nullptr, d_ml.as<int32_t>(), d_state.as<uint8_t>(), v, hi[1],
                                     res, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, d_poses.download<double>(nf * 7));
    put(o, d_start.download<double>(nf * 7));
    put(o, d_cost.download<double>(nf * 2));
    put(o, d_H.download<double>(nf * 36));
    put(o, d_counts.download<int32_t>(nf * 5));
    int32_t threw = 0;
    try {
      frontend.verifyPlaceRefineBlocks(0, *dev_set, d_blocks.d, -1, T_SC, d_hyp.as<double>(), int(n_hyp),
                                       d_best.as<int32_t>(), nullptr, d_ml.as<int32_t>(), d_state.as<uint8_t>(), nullptr,
                                       hi[1], res, stream);
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
