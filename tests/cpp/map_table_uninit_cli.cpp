// map_table_uninit_cli.cpp -- drives okvfe::HipFrontend::uploadLandmarkTable, matchToMapBlocks and
// matchToMapUninitialisedBlocks (the C++ host mirror of both matcher passes of Frontend::matchToMap from the raw
// landmark table, for frames that live on the device) from a binary request file; used by
// tests/test_gpu_map_table_uninit_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold, exclusive | f64 threshold |
//           table { int32 nl,no,np | hp nl*4 f64 | quality nl f64 | obs_begin (nl+1) i32 | obs_pose no i32 |
//           obs_desc no*48 u8 | obs_bp no*3 f64 | poses np*12 f64 } | int32 n_frames, block_bytes |
//           first-pass poses n_frames*12 f64 | second-pass poses n_frames*12 f64 |
//           gather blocks n_frames*block_bytes u8 (host-packed) | use n_frames*K u8 | previous n_frames*K i32
// response: first pass best_landmark n_frames*K i32 | status n_frames*nl i32 | second pass best_landmark n_frames*K i32
//           | best_dist n_frames*K i32 | hps_W n_frames*K*4 f64 | hp_set n_frames*K u8 | already_matched n_frames i32
//           (outputs start as 0xF9 bytes: rows the calls leave alone keep them)
//           | int32: 1 if a pose count that differs from n_frames made matchToMapUninitialisedBlocks throw
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
  const std::vector<int32_t> obs_begin = rdv<int32_t>(f, nl + 1), obs_pose = rdv<int32_t>(f, no);
  const std::vector<uint8_t> obs_desc = rdv<uint8_t>(f, no * 48);
  const std::vector<double> obs_bp = rdv<double>(f, no * 3);
  const std::vector<okvfe_pose> poses = rdv<okvfe_pose>(f, np);
  int32_t fn[2];
  rd(f, fn, 2);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]), K = size_t(par[0]);
  std::vector<okvfe_pose> T_first = rdv<okvfe_pose>(f, nf), T_second = rdv<okvfe_pose>(f, nf);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes), use = rdv<uint8_t>(f, nf * K);
  const std::vector<int32_t> previous = rdv<int32_t>(f, nf * K);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    okvfe_landmark_table table{tn[0], tn[1], tn[2], hp.data(), quality.data(), obs_begin.data(), obs_pose.data(),
                               obs_desc.data(), obs_bp.data(), poses.data()};
    const auto dev_table = frontend.uploadLandmarkTable(0, table);
    DeviceBuffer d_blocks(nf * block_bytes), d_use(nf * K), d_prev(nf * K * 4), d_lm(nf * K * 4), d_bd(nf * K * 4),
        d_status(nf * nl * 4), d_ndesc(nf * nl * 4), d_rows(nf * nl * 12), d_e(nf * nl * 48), d_r(nf * nl * 48),
        d_lm2(nf * K * 4), d_bd2(nf * K * 4), d_hp(nf * K * 32), d_hs(nf * K), d_ctr(nf * 4);
    if (okvfe_copy_to_device(d_blocks.d, blocks.data(), nf * block_bytes, nullptr) != OKVFE_OK ||
        okvfe_copy_to_device(d_use.d, use.data(), nf * K, nullptr) != OKVFE_OK ||
        okvfe_copy_to_device(d_prev.d, previous.data(), nf * K * 4, nullptr) != OKVFE_OK ||
        okvfe_stream_synchronize(nullptr) != OKVFE_OK)
      return 5;
    okvfe_landmark_pool_device pool{};  // (projection stays NULL: the second pass does not read it)
    pool.status = d_status.as<int32_t>();
    pool.n_desc = d_ndesc.as<int32_t>();
    pool.obs_rows = d_rows.as<int32_t>();
    pool.e_W = d_e.as<double>();
    pool.r_W = d_r.as<double>();
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    // both passes on one stream, nothing waited for in between
    frontend.matchToMapBlocks(0, *dev_table, d_blocks.d, int(nf), T_first, threshold, par[2] != 0, d_use.as<uint8_t>(),
                              &pool, d_lm.as<int32_t>(), d_bd.as<int32_t>(), stream);
    frontend.matchToMapUninitialisedBlocks(0, *dev_table, pool, d_blocks.d, int(nf), T_second, par[2] != 0,
                                           d_use.as<uint8_t>(), d_prev.as<int32_t>(), d_lm2.as<int32_t>(),
                                           d_bd2.as<int32_t>(), d_hp.as<double>(), d_hs.as<uint8_t>(),
                                           d_ctr.as<int32_t>(), stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, d_lm.download<int32_t>(nf * K));
    put(o, d_status.download<int32_t>(nf * nl));
    put(o, d_lm2.download<int32_t>(nf * K));
    put(o, d_bd2.download<int32_t>(nf * K));
    put(o, d_hp.download<double>(nf * K * 4));
    put(o, d_hs.download<uint8_t>(nf * K));
    put(o, d_ctr.download<int32_t>(nf));
    // error behaviour: one pose per frame, or the call throws before anything is launched
    int32_t threw = 0;
    T_second.push_back(T_second.empty() ? okvfe_pose{} : T_second.back());
    try {
      frontend.matchToMapUninitialisedBlocks(0, *dev_table, pool, d_blocks.d, int(nf), T_second, par[2] != 0, nullptr,
                                             nullptr, d_lm2.as<int32_t>(), d_bd2.as<int32_t>(), d_hp.as<double>(),
                                             d_hs.as<uint8_t>(), d_ctr.as<int32_t>(), stream);
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
