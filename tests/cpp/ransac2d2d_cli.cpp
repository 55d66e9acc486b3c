// ransac2d2d_cli.cpp -- drives okvfe::HipFrontend::ransac2d2dBlocks (the consensus of runRansac2d2d on device batches,
// landmark1_out in place) from a binary request file.  Used by tests/test_gpu_ransac2d2d_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold | int32 n_landmarks |
//           added n_landmarks u8 (n_landmarks 0: no table) | int32 n_frames0, n_frames1, block_bytes |
//           gather blocks n_frames0*block_bytes, n_frames1*block_bytes u8 (host-packed) | ids n_frames0*K, n_frames1*K i32 |
//           int32 n_pairs | mf0, mf1 n_pairs i32 each | int32 n_hyp | rot n_pairs*n_hyp*9 f64 | rel n_pairs*n_hyp*12 f64 |
//           int32 has_valid | rot_valid, rel_valid n_pairs*n_hyp u8 each (if has_valid)
//           (a frame is a multiframe of one camera here)
// response: n_correspondences, rot_best, rot_inliers, rel_best, rel_inliers n_pairs i32 each | branch, removed n_pairs u8
//           each | total_inliers n_pairs i32 | rotation_only, success n_pairs u8 each | rot_hyp_inliers, rel_hyp_inliers
//           n_pairs*n_hyp i32 each | match1 n_pairs*K i32 | state n_pairs*K u8 | distance n_pairs*K f64 | current ids
//           n_frames1*K i32 (outputs start as 0xF9 bytes: rows the call leaves alone keep them) | int32: 1 if a
//           hypothesis count that does not fit made ransac2d2dBlocks throw
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
  int32_t par[2], nl;
  rd(f, par, 2);
  rd(f, &nl, 1);
  const size_t n_added = size_t(nl);
  const std::vector<uint8_t> added = rdv<uint8_t>(f, n_added);
  int32_t fn[3];
  rd(f, fn, 3);
  const size_t n0 = size_t(fn[0]), n1 = size_t(fn[1]), block_bytes = size_t(fn[2]), K = size_t(par[0]);
  const std::vector<uint8_t> blocks0 = rdv<uint8_t>(f, n0 * block_bytes), blocks1 = rdv<uint8_t>(f, n1 * block_bytes);
  const std::vector<int32_t> lm0 = rdv<int32_t>(f, n0 * K), lm1 = rdv<int32_t>(f, n1 * K);
  int32_t n_pairs;
  rd(f, &n_pairs, 1);
  const size_t np = size_t(n_pairs);
  const std::vector<int32_t> mf0 = rdv<int32_t>(f, np), mf1 = rdv<int32_t>(f, np);
  int32_t n_hyp;
  rd(f, &n_hyp, 1);
  const size_t nh = size_t(n_hyp);
  std::vector<double> rot = rdv<double>(f, np * nh * 9);
  const std::vector<double> rel = rdv<double>(f, np * nh * 12);
  int32_t has_valid;
  rd(f, &has_valid, 1);
  std::vector<uint8_t> rot_valid, rel_valid;
  if (has_valid) {
    rot_valid = rdv<uint8_t>(f, np * nh);
    rel_valid = rdv<uint8_t>(f, np * nh);
  }
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    DeviceBuffer d_b0(n0 * block_bytes), d_b1(n1 * block_bytes), d_lm0(n0 * K * 4), d_lm1(n1 * K * 4), d_added(n_added),
        d_cam(np * 5 * 4), d_flags(np * 2), d_total(np * 4), d_pair(np * 2), d_rh(np * nh * 4), d_lh(np * nh * 4),
        d_match(np * K * 4), d_state(np * K), d_dist(np * K * 8);
    d_b0.upload(blocks0);
    d_b1.upload(blocks1);
    d_lm0.upload(lm0);
    d_lm1.upload(lm1);
    d_added.upload(added);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    okvfe_ransac2d2d_result_device res{};
    res.n_correspondences = d_cam.as<int32_t>();
    res.rot_best = d_cam.as<int32_t>() + np;
    res.rot_inliers = d_cam.as<int32_t>() + 2 * np;
    res.rel_best = d_cam.as<int32_t>() + 3 * np;
    res.rel_inliers = d_cam.as<int32_t>() + 4 * np;
    res.branch = d_flags.as<uint8_t>();
    res.removed = d_flags.as<uint8_t>() + np;
    res.total_inliers = d_total.as<int32_t>();
    res.rotation_only = d_pair.as<uint8_t>();
    res.success = d_pair.as<uint8_t>() + np;
    res.rot_hyp_inliers = d_rh.as<int32_t>();
    res.rel_hyp_inliers = d_lh.as<int32_t>();
    res.match1 = d_match.as<int32_t>();
    res.state = d_state.as<uint8_t>();
    res.distance = d_dist.as<double>();
    res.landmark1_out = d_lm1.as<int32_t>();  // in place
    frontend.ransac2d2dBlocks(0, d_b0.d, int(n0), d_b1.d, int(n1), mf0, mf1, d_lm0.as<int32_t>(), d_lm1.as<int32_t>(),
                              nl ? d_added.as<uint8_t>() : nullptr, nl, rot, rot_valid, rel, rel_valid, n_hyp, res, true, 9.0,
                              stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, d_cam.download<int32_t>(np * 5));
    put(o, d_flags.download<uint8_t>(np * 2));
    put(o, d_total.download<int32_t>(np));
    put(o, d_pair.download<uint8_t>(np * 2));
    put(o, d_rh.download<int32_t>(np * nh));
    put(o, d_lh.download<int32_t>(np * nh));
    put(o, d_match.download<int32_t>(np * K));
    put(o, d_state.download<uint8_t>(np * K));
    put(o, d_dist.download<double>(np * K));
    put(o, d_lm1.download<int32_t>(n1 * K));
    // error behaviour: nHyp hypotheses of both problems per pair, or the call throws before anything is launched
    int32_t threw = 0;
    rot.push_back(0.0);
    try {
      frontend.ransac2d2dBlocks(0, d_b0.d, int(n0), d_b1.d, int(n1), mf0, mf1, d_lm0.as<int32_t>(), d_lm1.as<int32_t>(), nullptr,
                                0, rot, rot_valid, rel, rel_valid, n_hyp, res, true, 9.0, stream);
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
