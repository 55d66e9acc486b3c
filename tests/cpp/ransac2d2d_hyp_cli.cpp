// ransac2d2d_hyp_cli.cpp -- drives the 2d2d hypotheses of the C++ host mirror on frames that live on the device:
// okvfe::HipFrontend::ransac2d2dHypothesesBlocks for the pairs (older frame p, current frame p) of one camera, on a
// stream of its own with nothing waited for before the download; from a binary request file.  Used by
// tests/test_gpu_ransac2d2d_hyp_cpp.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, n_pairs, block_bytes, n_hyp, with_keys, pad |
//           older gather blocks n_pairs*block_bytes u8 (host-packed) | current gather blocks, the same | older id rows
//           n_pairs*K i32 | current id rows, the same | uint64 seed | keys n_pairs u64 (read if with_keys)
//           (a frame is a multiframe of one camera here)
// response: rot_hyp n_pairs*n_hyp*9 f64 | rot_valid n_pairs*n_hyp u8 | rel_hyp n_pairs*n_hyp*12 f64 | rel_valid
//           n_pairs*n_hyp u8 | n_correspondences n_pairs i32 | rot_samples n_pairs*n_hyp*2 i32 | rel_samples
//           n_pairs*n_hyp*8 i32 | rel_n_roots n_pairs*n_hyp i32 (outputs start as 0xF9 bytes) |
//           int32: 1 if n_hyp = 65 made ransac2d2dHypothesesBlocks throw
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
  const size_t K = size_t(par[0]), np = size_t(par[1]), block_bytes = size_t(par[2]), nh = size_t(par[3]);
  const std::vector<uint8_t> blocks0 = rdv<uint8_t>(f, np * block_bytes), blocks1 = rdv<uint8_t>(f, np * block_bytes);
  const std::vector<int32_t> rows0 = rdv<int32_t>(f, np * K), rows1 = rdv<int32_t>(f, np * K);
  uint64_t seed;
  rd(f, &seed, 1);
  const std::vector<uint64_t> keys = rdv<uint64_t>(f, par[4] ? np : 0);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    DeviceBuffer d_b0(np * block_bytes), d_b1(np * block_bytes), d_r0(np * K * 4), d_r1(np * K * 4), d_keys(np * 8);
    d_b0.upload(blocks0);
    d_b1.upload(blocks1);
    d_r0.upload(rows0);
    d_r1.upload(rows1);
    d_keys.upload(keys);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    const uint64_t* keys_dev = par[4] ? d_keys.as<uint64_t>() : nullptr;
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    DeviceBuffer rot(np * nh * 72), rotv(np * nh), rel(np * nh * 96), relv(np * nh), nc(np * 4), rs(np * nh * 8),
        ls(np * nh * 32), nr(np * nh * 4);
    const okvfe_ransac2d2d_hypotheses_device res{rot.as<double>(), rotv.as<uint8_t>(), rel.as<double>(), relv.as<uint8_t>(),
                                                 nc.as<int32_t>(), rs.as<int32_t>(), ls.as<int32_t>(), nr.as<int32_t>()};
    std::vector<int32_t> mf(np);
    for (size_t i = 0; i < np; ++i) mf[i] = int32_t(i);
    frontend.ransac2d2dHypothesesBlocks(0, d_b0.d, int(np), d_b1.d, int(np), mf, mf, d_r0.as<int32_t>(), d_r1.as<int32_t>(),
                                        nullptr, 0, keys_dev, seed, int(nh), res, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, rot.download<double>(np * nh * 9));
    put(o, rotv.download<uint8_t>(np * nh));
    put(o, rel.download<double>(np * nh * 12));
    put(o, relv.download<uint8_t>(np * nh));
    put(o, nc.download<int32_t>(np));
    put(o, rs.download<int32_t>(np * nh * 2));
    put(o, ls.download<int32_t>(np * nh * 8));
    put(o, nr.download<int32_t>(np * nh));
    int32_t threw = 0;
    try {
      frontend.ransac2d2dHypothesesBlocks(0, d_b0.d, int(np), d_b1.d, int(np), mf, mf, d_r0.as<int32_t>(),
                                          d_r1.as<int32_t>(), nullptr, 0, keys_dev, seed, OKVFE_RANSAC_MAX_HYPOTHESES + 1,
                                          res, stream);
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
