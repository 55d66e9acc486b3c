// map_table_cli.cpp -- drives okvfe::HipFrontend::uploadLandmarkTable and matchToMapBlocks (the C++ host mirror of
// Frontend::matchToMap from the raw landmark table, for frames that live on the device) from a binary request file;
// used by tests/test_gpu_map_table_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold, exclusive | f64 threshold |
//           table { int32 nl,no,np | hp nl*4 f64 | quality nl f64 | obs_begin (nl+1) i32 | obs_pose no i32 |
//           obs_desc no*48 u8 | obs_bp no*3 f64 | poses np*12 f64 } | int32 n_frames, block_bytes |
//           poses n_frames*12 f64 | gather blocks n_frames*block_bytes u8 (host-packed) | use n_frames*K u8
// response: best_landmark n_frames*K i32 | best_dist n_frames*K i32 | status n_frames*nl i32 | obs_rows n_frames*nl*3
//           i32 | projection n_frames*nl*2 f64   (outputs start as 0xF9 bytes: rows the call leaves alone keep them)
//           | int32: 1 if a table with a pose index out of range made uploadLandmarkTable throw
#include <cstdio>
#include <cstdlib>
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
  double threshold;
  rd(f, &threshold, 1);
  int32_t tn[3];
  rd(f, tn, 3);
  const size_t nl = size_t(tn[0]), no = size_t(tn[1]), np = size_t(tn[2]);
  const std::vector<double> hp = rdv<double>(f, nl * 4), quality = rdv<double>(f, nl);
  const std::vector<int32_t> obs_begin = rdv<int32_t>(f, nl + 1);
  std::vector<int32_t> obs_pose = rdv<int32_t>(f, no);
  const std::vector<uint8_t> obs_desc = rdv<uint8_t>(f, no * 48);
  const std::vector<double> obs_bp = rdv<double>(f, no * 3);
  const std::vector<okvfe_pose> poses = rdv<okvfe_pose>(f, np);
  int32_t fn[2];
  rd(f, fn, 2);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]), K = size_t(par[0]);
  std::vector<okvfe_pose> T_WC1 = rdv<okvfe_pose>(f, nf);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes), use = rdv<uint8_t>(f, nf * K);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    okvfe_landmark_table table{tn[0], tn[1], tn[2], hp.data(), quality.data(), obs_begin.data(), obs_pose.data(),
                               obs_desc.data(), obs_bp.data(), poses.data()};
    const auto dev_table = frontend.uploadLandmarkTable(0, table);
    DeviceBuffer d_blocks(nf * block_bytes), d_use(nf * K), d_lm(nf * K * 4), d_bd(nf * K * 4), d_status(nf * nl * 4),
        d_rows(nf * nl * 12), d_proj(nf * nl * 16);
    if (okvfe_copy_to_device(d_blocks.d, blocks.data(), nf * block_bytes, nullptr) != OKVFE_OK ||
        okvfe_copy_to_device(d_use.d, use.data(), nf * K, nullptr) != OKVFE_OK ||
        okvfe_stream_synchronize(nullptr) != OKVFE_OK)
      return 5;
    okvfe_landmark_pool_device pool{};  // some members only: the others stay NULL
    pool.status = static_cast<int32_t*>(d_status.d);
    pool.obs_rows = static_cast<int32_t*>(d_rows.d);
    pool.projection = static_cast<double*>(d_proj.d);
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    frontend.matchToMapBlocks(0, *dev_table, d_blocks.d, int(nf), T_WC1, threshold, par[2] != 0,
                              static_cast<const uint8_t*>(d_use.d), &pool, static_cast<int32_t*>(d_lm.d),
                              static_cast<int32_t*>(d_bd.d), stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    okvfe_stream_destroy(stream);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const auto lm = d_lm.download<int32_t>(nf * K), bd = d_bd.download<int32_t>(nf * K);
    const auto status = d_status.download<int32_t>(nf * nl), rows = d_rows.download<int32_t>(nf * nl * 3);
    const auto proj = d_proj.download<double>(nf * nl * 2);
    fwrite(lm.data(), 4, lm.size(), o);
    fwrite(bd.data(), 4, bd.size(), o);
    fwrite(status.data(), 4, status.size(), o);
    fwrite(rows.data(), 4, rows.size(), o);
    fwrite(proj.data(), 8, proj.size(), o);
    // error behaviour: a malformed table is rejected at the upload
    int32_t threw = 0;
    if (no > 0) {
      obs_pose[no / 2] = tn[2];
      try {
        frontend.uploadLandmarkTable(0, table);
      } catch (const okvfe::Exception& e) {
        threw = e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
      }
    }
    fwrite(&threw, 4, 1, o);
    fclose(o);
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
