// elementary_fixed_main.cpp -- evaluates okvis2_amd/csrc/elementary_fixed.h on the host for
// tests/test_elementary_fixed_host.py: reads n doubles from the request file, writes sin_fixed, cos_fixed, sinc_fixed and
// log_fixed of each (4 x n doubles, function-major) to the response file.
#include <cstdio>
#include <vector>

#include "okvis2_amd/csrc/elementary_fixed.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<double> x;
  double v;
  while (std::fread(&v, sizeof v, 1, in) == 1) x.push_back(v);
  std::fclose(in);
  std::vector<double> out(4 * x.size());
  for (size_t i = 0; i < x.size(); ++i) {
    out[i] = okvfe::sin_fixed(x[i]);
    out[x.size() + i] = okvfe::cos_fixed(x[i]);
    out[2 * x.size() + i] = okvfe::sinc_fixed(x[i]);
    out[3 * x.size() + i] = okvfe::log_fixed(x[i]);
  }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f) return 4;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
  return std::fclose(f) == 0 && ok ? 0 : 5;
}
