// motion_sweep_cli.cpp -- drives okvfe::HipFrontend::matchMotionStereoSweep (the loop of Frontend::matchMotionStereo
// over the older frames, matched1 updated in place on the device) from a binary request file: every step of every
// camera queued on one stream, one synchronisation at the end.  Compiled and run by tests/test_gpu_motion_batch.py.
// request : int32 n_cams | per camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold |
//           int32 n_blocks0, n_blocks1, block_bytes, n_steps, pairs_per_step | older blocks | current blocks (host-packed
//           gather blocks) | matched1 n_blocks1*K u8 | per step { idx0, idx1, camera: pairs i32 each | T_WC0, T_WC1:
//           pairs*12 f64 each | skip0 pairs*K u8 }
// response: per step { match rows pairs*K*64 bytes | claimed pairs*K u8 | n_claimed pairs i32 } in the request's pair
//           order (outputs start as 0xF9 bytes: rows the calls leave alone keep them) | matched1 after the sweep
//           n_blocks1*K u8 | int32: 1 if a step that names a current block twice made the call throw
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#include "cli_io.hpp"

struct StepBuffers {  // one camera's share of one step
  std::vector<size_t> where;  // positions of its pairs in the request's step
  std::unique_ptr<DeviceBuffer> skip0, matches, claimed, n_claimed;
};

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  const int32_t n_cams = rdv<int32_t>(f, 1)[0];
  std::vector<okvfe_camera> cams;
  for (int m = 0; m < n_cams; ++m) {
    const std::vector<int32_t> ci = rdv<int32_t>(f, 3);
    const std::vector<double> cd = rdv<double>(f, 8);
    okvfe_camera cam{};
    cam.width = ci[0]; cam.height = ci[1]; cam.distortion = ci[2];
    cam.fu = cd[0]; cam.fv = cd[1]; cam.cu = cd[2]; cam.cv = cd[3];
    for (int i = 0; i < 4; ++i) cam.d[i] = cd[4 + i];
    cams.push_back(cam);
  }
  const std::vector<int32_t> par = rdv<int32_t>(f, 2), dim = rdv<int32_t>(f, 5);
  const size_t K = size_t(par[0]), nb0 = size_t(dim[0]), nb1 = size_t(dim[1]), block_bytes = size_t(dim[2]),
               n_steps = size_t(dim[3]), pairs = size_t(dim[4]);
  const std::vector<uint8_t> blocks0 = rdv<uint8_t>(f, nb0 * block_bytes), blocks1 = rdv<uint8_t>(f, nb1 * block_bytes),
                             matched1 = rdv<uint8_t>(f, nb1 * K);
  struct Step {
    std::vector<int32_t> idx0, idx1, cam;
    std::vector<okvfe_pose> T0, T1;
    std::vector<uint8_t> skip0;
  };
  std::vector<Step> req(n_steps);
  for (Step& s : req) {
    s.idx0 = rdv<int32_t>(f, pairs); s.idx1 = rdv<int32_t>(f, pairs); s.cam = rdv<int32_t>(f, pairs);
    s.T0 = rdv<okvfe_pose>(f, pairs); s.T1 = rdv<okvfe_pose>(f, pairs);
    s.skip0 = rdv<uint8_t>(f, pairs * K);
  }
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(cams, p);
    DeviceBuffer d_blocks0(nb0 * block_bytes), d_blocks1(nb1 * block_bytes), d_matched1(nb1 * K);
    d_blocks0.upload(blocks0);
    d_blocks1.upload(blocks1);
    d_matched1.upload(matched1);
    const size_t nc = size_t(n_cams);
    std::vector<std::vector<StepBuffers>> buf(nc);
    for (auto& b : buf) b.resize(n_steps);
    std::vector<std::vector<okvfe::HipFrontend::MotionSweepStep>> sweep(nc);
    for (int m = 0; m < n_cams; ++m)
      for (size_t j = 0; j < n_steps; ++j) {
        StepBuffers& b = buf[size_t(m)][j];
        okvfe::HipFrontend::MotionSweepStep st;
        std::vector<uint8_t> skip;
        for (size_t q = 0; q < pairs; ++q) {
          if (req[j].cam[q] != m) continue;
          b.where.push_back(q);
          st.idx0.push_back(req[j].idx0[q]); st.idx1.push_back(req[j].idx1[q]);
          st.T_WC0.push_back(req[j].T0[q]); st.T_WC1.push_back(req[j].T1[q]);
          skip.insert(skip.end(), req[j].skip0.begin() + long(q * K), req[j].skip0.begin() + long((q + 1) * K));
        }
        const size_t n = b.where.size();
        b.skip0.reset(new DeviceBuffer(n * K));
        b.matches.reset(new DeviceBuffer(n * K * sizeof(okvfe_motion_match)));
        b.claimed.reset(new DeviceBuffer(n * K));
        b.n_claimed.reset(new DeviceBuffer(n * 4));
        b.skip0->upload(skip);
        st.skip0Dev = b.skip0->as<uint8_t>();
        st.matchesDev = b.matches->as<okvfe_motion_match>();
        st.claimedDev = b.claimed->as<uint8_t>();
        st.nClaimedDev = b.n_claimed->as<int32_t>();
        sweep[size_t(m)].push_back(st);
      }
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;  // (the uploads ran on the null stream)
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    for (int m = 0; m < n_cams; ++m)
      frontend.matchMotionStereoSweep(size_t(m), d_blocks0.d, int(nb0), d_blocks1.d, int(nb1), sweep[size_t(m)],
                                      d_matched1.as<uint8_t>(), stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    const size_t rec = sizeof(okvfe_motion_match);
    for (size_t j = 0; j < n_steps; ++j) {
      std::vector<uint8_t> rows(pairs * K * rec, 0xF9), claimed(pairs * K, 0xF9), ncl(pairs * 4, 0xF9);
      for (int m = 0; m < n_cams; ++m) {
        const StepBuffers& b = buf[size_t(m)][j];
        if (b.where.empty()) continue;
        const std::vector<uint8_t> r = b.matches->download<uint8_t>(b.matches->bytes),
                                   c = b.claimed->download<uint8_t>(b.claimed->bytes),
                                   n = b.n_claimed->download<uint8_t>(b.n_claimed->bytes);
        for (size_t i = 0; i < b.where.size(); ++i) {
          std::memcpy(rows.data() + b.where[i] * K * rec, r.data() + i * K * rec, K * rec);
          std::memcpy(claimed.data() + b.where[i] * K, c.data() + i * K, K);
          std::memcpy(ncl.data() + b.where[i] * 4, n.data() + i * 4, 4);
        }
      }
      fwrite(rows.data(), 1, rows.size(), o);
      fwrite(claimed.data(), 1, claimed.size(), o);
      fwrite(ncl.data(), 1, ncl.size(), o);
    }
    const std::vector<uint8_t> m1 = d_matched1.download<uint8_t>(d_matched1.bytes);
    fwrite(m1.data(), 1, nb1 * K, o);
    // error behaviour: with claims a current block is named once per call, or the call throws before anything is launched
    int32_t threw = 0;
    if (!sweep[0].empty() && !sweep[0][0].idx1.empty()) {
      okvfe::HipFrontend::MotionSweepStep twice = sweep[0][0];
      twice.idx0.push_back(twice.idx0[0]); twice.idx1.push_back(twice.idx1[0]);
      twice.T_WC0.push_back(twice.T_WC0[0]); twice.T_WC1.push_back(twice.T_WC1[0]);
      twice.skip0Dev = nullptr;
      try {
        frontend.matchMotionStereoSweep(0, d_blocks0.d, int(nb0), d_blocks1.d, int(nb1), {twice}, d_matched1.as<uint8_t>(),
                                        stream);
      } catch (const okvfe::Exception& e) {
        threw = e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
      }
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
