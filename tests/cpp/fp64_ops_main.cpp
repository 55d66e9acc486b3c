// fp64_ops_main.cpp -- evaluates okvis2_amd/csrc/fp64_ops.h on the host, on its own, for tests/test_fp64_ops_host.py.
// Request file: int32 n3, n4, nq, pad; n3 x 3 doubles (triples), n4 x 4 doubles (quadruples), nq x 8 doubles (quaternions
// a, b).  Response file, doubles:
//   per triple      sum3<true>, sum3<false>, sum3_select(true, ..), sum3_select(false, ..), then finite (1.0 / 0.0) and
//                   sqrt of its first term                                                                  (6)
//   per quadruple   sum4<true>, sum4<false>                                                                 (2)
//   per quaternion  quat_normalized<true>(a), quat_normalized<false>(a), quat_product(a, b)                 (12)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "okvis2_amd/csrc/fp64_ops.h"

namespace F = okvfe::fp64;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t head[4] = {0, 0, 0, 0};
  bool ok = std::fread(head, sizeof head, 1, in) == 1 && head[0] >= 0 && head[1] >= 0 && head[2] >= 0;
  const size_t n3 = ok ? (size_t)head[0] : 0, n4 = ok ? (size_t)head[1] : 0, nq = ok ? (size_t)head[2] : 0;
  std::vector<double> x(3 * n3 + 4 * n4 + 8 * nq);
  ok = ok && std::fread(x.data(), sizeof(double), x.size(), in) == x.size();
  std::fclose(in);
  if (!ok) return 3;
  std::vector<double> out;
  out.reserve(6 * n3 + 2 * n4 + 12 * nq);
  const double* t = x.data();
  for (size_t i = 0; i < n3; ++i, t += 3) {
    out.push_back(F::sum3<true>(t[0], t[1], t[2]));
    out.push_back(F::sum3<false>(t[0], t[1], t[2]));
    out.push_back(F::sum3_select(true, t[0], t[1], t[2]));
    out.push_back(F::sum3_select(false, t[0], t[1], t[2]));
    out.push_back(F::finite(t[0]) ? 1.0 : 0.0);
    out.push_back(F::sqrt(t[0]));
  }
  for (size_t i = 0; i < n4; ++i, t += 4) {
    out.push_back(F::sum4<true>(t[0], t[1], t[2], t[3]));
    out.push_back(F::sum4<false>(t[0], t[1], t[2], t[3]));
  }
  for (size_t i = 0; i < nq; ++i, t += 8) {
    double o[12];
    F::quat_normalized<true>(t, o);
    F::quat_normalized<false>(t, o + 4);
    F::quat_product(t, t + 4, o + 8);
    out.insert(out.end(), o, o + 12);
  }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 4;
  ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 5;
}
