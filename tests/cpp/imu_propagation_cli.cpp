// imu_propagation_cli.cpp -- drives okvfe::HipFrontend::propagationBlocks (and, with "host" as the third argument,
// HipFrontend::propagation one multiframe at a time) of the C++ host mirror from the request file of
// tests/cpp/imu_propagation_main.cpp, and writes that program's response.  Used by tests/test_gpu_imu_propagation_cpp.py.
// The outputs start as the sentinel -4321: records a call leaves alone keep it.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#include "cli_io.hpp"

namespace {
constexpr int32_t kMagic = 0x494D5531;
constexpr double kSentinel = -4321.0;
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  const bool host = argc > 3 && std::string(argv[3]) == "host";
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t head[8];
  rd(f, head, 8);
  if (head[0] != kMagic || head[1] < 0 || head[2] < 0 || head[6] < 0) return 3;
  const size_t n = size_t(head[1]), nc = size_t(head[2]), total = size_t(head[6]);
  const size_t n_begin = (n + 2) & ~size_t(1);
  const std::vector<double> prm = rdv<double>(f, 7), T_SC_flat = rdv<double>(f, 7 * nc);
  const std::vector<int32_t> begin = rdv<int32_t>(f, n_begin);
  const std::vector<double> samples = rdv<double>(f, 8 * total), states = rdv<double>(f, 18 * n);
  fclose(f);
  okvfe_imu_params P{};
  P.a_max = prm[0]; P.g_max = prm[1]; P.sigma_g_c = prm[2]; P.sigma_a_c = prm[3]; P.sigma_gw_c = prm[4];
  P.sigma_aw_c = prm[5]; P.g = prm[6];
  std::vector<std::array<double, 7>> T_SC(nc);
  for (size_t c = 0; c < nc; ++c) std::memcpy(T_SC[c].data(), T_SC_flat.data() + 7 * c, 56);
  std::vector<double> pose(7 * n, kSentinel), sb(9 * n, kSentinel), jac(225 * n, kSentinel), cov(225 * n, kSentinel),
      T_WC(7 * n * nc, kSentinel);
  std::vector<int32_t> ints(3 * n_begin, int32_t(kSentinel));
  std::vector<float> grav(3 * n * nc, float(kSentinel));
  try {
    if (host) {
      for (size_t m = 0; m < n; ++m) {
        std::vector<okvfe::HipFrontend::ImuSample> list(size_t(begin[m + 1] - begin[m]));
        for (size_t i = 0; i < list.size(); ++i) {
          const double* r = samples.data() + 8 * (size_t(begin[m]) + i);
          uint64_t bits;
          std::memcpy(&bits, r, 8);
          list[i].sec = uint32_t(bits);
          list[i].nsec = uint32_t(bits >> 32);
          for (size_t k = 0; k < 3; ++k) {
            list[i].gyroscopes[k] = r[1 + k];
            list[i].accelerometers[k] = r[4 + k];
          }
        }
        const double* st = states.data() + 18 * m;
        uint64_t t0, t1;
        std::memcpy(&t0, st, 8);
        std::memcpy(&t1, st + 1, 8);
        std::array<double, 7> T_WS;
        std::array<double, 9> speedAndBias;
        std::memcpy(T_WS.data(), st + 2, 56);
        std::memcpy(speedAndBias.data(), st + 9, 72);
        const okvfe::HipFrontend::Propagation r = okvfe::HipFrontend::propagation(
            list, P, T_WS, speedAndBias, uint32_t(t0), uint32_t(t0 >> 32), uint32_t(t1), uint32_t(t1 >> 32), T_SC,
            head[4] != 0, head[5] != 0, head[3] != 0);
        ints[n_begin + m] = r.status;
        ints[2 * n_begin + m] = r.nOutOfRange;
        if (r.status != 0) continue;
        ints[m] = r.nPropagated;
        std::memcpy(pose.data() + 7 * m, r.T_WS.data(), 56);
        std::memcpy(sb.data() + 9 * m, r.speedAndBias.data(), 72);
        if (!r.jacobian.empty()) std::memcpy(jac.data() + 225 * m, r.jacobian.data(), 1800);
        if (!r.covariance.empty()) std::memcpy(cov.data() + 225 * m, r.covariance.data(), 1800);
        for (size_t c = 0; c < nc; ++c) {
          std::memcpy(T_WC.data() + 7 * (m * nc + c), r.T_WC[c].data(), 56);
          std::memcpy(grav.data() + 3 * (m * nc + c), r.gravity_C[c].data(), 12);
        }
      }
    } else {
      okvfe_camera cam{};
      cam.width = 64; cam.height = 64; cam.fu = 50.0; cam.fv = 50.0; cam.cu = 32.0; cam.cv = 32.0;
      okvfe::FrontendParameters p{};
      p.max_num_keypoints = 10;
      okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
      frontend.setFp64Reduction(head[3] != 0);
      void* stream = nullptr;
      if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
      DeviceBuffer d_samples(8 * 8 * total), d_begin(4 * n_begin), d_states(8 * 18 * n), d_pose(56 * n), d_sb(72 * n),
          d_ints(4 * 3 * n_begin), d_jac(1800 * n), d_cov(1800 * n), d_T_WC(56 * n * nc), d_grav(12 * n * nc);
      d_samples.upload(samples); d_begin.upload(begin); d_states.upload(states);
      d_pose.upload(pose); d_sb.upload(sb); d_ints.upload(ints); d_jac.upload(jac); d_cov.upload(cov);
      d_T_WC.upload(T_WC); d_grav.upload(grav);
      if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
      okvfe_imu_result_device res{};
      res.pose = d_pose.as<double>();
      res.speed_and_bias = d_sb.as<double>();
      res.n_propagated = d_ints.as<int32_t>();
      res.status = d_ints.as<int32_t>() + n_begin;
      res.n_out_of_range = d_ints.as<int32_t>() + 2 * n_begin;
      res.jacobian = head[4] ? d_jac.as<double>() : nullptr;
      res.covariance = head[5] ? d_cov.as<double>() : nullptr;
      res.T_WC = nc ? d_T_WC.as<double>() : nullptr;
      res.gravity_C = nc ? d_grav.as<float>() : nullptr;
      frontend.propagationBlocks(0, P, d_samples.as<double>(), d_begin.as<int32_t>(), d_states.as<double>(), int(n), T_SC,
                                 res, stream);
      if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
      pose = d_pose.download<double>(pose.size());
      sb = d_sb.download<double>(sb.size());
      ints = d_ints.download<int32_t>(ints.size());
      jac = d_jac.download<double>(jac.size());
      cov = d_cov.download<double>(cov.size());
      T_WC = d_T_WC.download<double>(T_WC.size());
      grav = d_grav.download<float>(grav.size());
      bool threw = false;
      try {
        frontend.propagationBlocks(0, P, d_samples.as<double>(), d_begin.as<int32_t>(), d_states.as<double>(), -1, T_SC, res,
                                   stream);
      } catch (const okvfe::Exception& e) {
        threw = e.status == OKVFE_ERR_INVALID_ARGUMENT;
      }
      frontend.setFp64Reduction(true);
      okvfe_stream_destroy(stream);
      if (!threw) return 7;
    }
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 1;
  put(o, pose); put(o, sb); put(o, ints); put(o, jac); put(o, cov); put(o, T_WC); put(o, grav);
  fclose(o);
  return 0;
}
