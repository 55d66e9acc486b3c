// imu_propagation_main.cpp -- runs okvis2_amd/csrc/imu_dev.h on the host for tests/test_imu_host.py, without the library:
// the request file (tests/imu_scenes.py write_request) holds one batch in the layout of
// okvfe_imu_propagation_blocks_device, the response file the outputs of every multiframe over a sentinel.
//   request   int32[8]: magic, n_multiframes, n_cams, order (0 left to right, 1 Eigen's tree), want_jacobian,
//             want_covariance, total samples, 0; 7 doubles of parameters; n_cams x 7 of T_SC; n + 1 int32 offsets (padded
//             to 8 bytes); samples x 8 doubles; n x 18 doubles of states
//   response  pose n x 7, speed_and_bias n x 9 doubles; n_propagated, status, n_out_of_range n int32 each (padded to 8
//             bytes together); jacobian, covariance n x 225 doubles; T_WC n x n_cams x 7 doubles; gravity_C n x n_cams x 3 floats
#include <cstdint>
#include <cstdio>
#include <vector>

#include "okvis2_amd/csrc/imu_dev.h"

namespace {
constexpr int32_t kMagic = 0x494D5531;
constexpr double kSentinel = -4321.0;

template <typename T>
bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}
template <typename T>
bool write_n(std::FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<int32_t> head, begin;
  std::vector<double> prm, T_SC, samples, states;
  if (!read_n(in, &head, 8) || head[0] != kMagic || head[1] < 0 || head[2] < 0 || head[6] < 0) return 4;
  const size_t n = (size_t)head[1], n_cams = (size_t)head[2];
  const size_t n_begin = (n + 2) & ~(size_t)1;
  if (!read_n(in, &prm, 7) || !read_n(in, &T_SC, 7 * n_cams) || !read_n(in, &begin, n_begin) ||
      !read_n(in, &samples, 8 * (size_t)head[6]) || !read_n(in, &states, 18 * n))
    return 4;
  std::fclose(in);
  for (size_t m = 0; m < n; ++m)
    if (begin[m] < 0 || begin[m + 1] < begin[m] || begin[m + 1] > head[6]) return 4;
  std::vector<double> pose(7 * n, kSentinel), sb(9 * n, kSentinel), jac(225 * n, kSentinel), cov(225 * n, kSentinel),
      T_WC(7 * n * n_cams, kSentinel);
  std::vector<int32_t> ints(3 * n_begin, (int32_t)kSentinel);
  std::vector<float> grav(3 * n * n_cams, (float)kSentinel);
  okvfe::ImuParams P;
  P.a_max = prm[0]; P.g_max = prm[1]; P.sigma_g_c = prm[2]; P.sigma_a_c = prm[3]; P.sigma_gw_c = prm[4];
  P.sigma_aw_c = prm[5]; P.g = prm[6];
  okvfe::ImuResultPtrs R;
  R.pose = pose.data(); R.speed_and_bias = sb.data();
  R.n_propagated = ints.data(); R.status = ints.data() + n_begin; R.n_out_of_range = ints.data() + 2 * n_begin;
  R.jacobian = head[4] ? jac.data() : nullptr;
  R.covariance = head[5] ? cov.data() : nullptr;
  R.T_WC = n_cams ? T_WC.data() : nullptr;
  R.gravity_C = n_cams ? grav.data() : nullptr;
  for (size_t m = 0; m < n; ++m) {
    if (head[3])
      okvfe::imu_host_multiframe<true>(P, samples.data(), begin.data(), states.data(), (long long)m, (int)n_cams,
                                       T_SC.data(), R);
    else
      okvfe::imu_host_multiframe<false>(P, samples.data(), begin.data(), states.data(), (long long)m, (int)n_cams,
                                        T_SC.data(), R);
  }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 5;
  const bool ok = write_n(f, pose) && write_n(f, sb) && write_n(f, ints) && write_n(f, jac) && write_n(f, cov) &&
                  write_n(f, T_WC) && write_n(f, grav);
  return std::fclose(f) == 0 && ok ? 0 : 6;
}
