// ransac_hyp_main.cpp -- okvis2_amd/csrc/ransac_hyp_dev.h as a stand-alone host program: the sampler, the P3P solver and
// the choice among its solutions driven by correspondence lists from a file, for tests/test_ransac_hyp_host.py (which
// builds it twice, once with the sanitizers).  No device work, no library.
//   request:  int32 tree, n_multiframes; uint64 seed; per multiframe uint64 key, int32 n_hyp, n_cams, K, gate (-1: none),
//             n; n_cams x 12 doubles (C row-major, r of T_SC); n records of 7 doubles (p, b, sigma) and int32 cam, row,
//             camera-major
//   response: per multiframe and hypothesis 12 doubles, int32 samples[4] (c K + k or -1), n_solutions, valid
// The header takes the distance of the consensus as a functor (in the library: the consensus kernel's own functions,
// which are HIP code).  TestDistance below is this program's transcription of tests/ransac_ref.py's `distances`, line by
// line; the library's copy is held to the same restatement by okvfe_p3p_hypothesis in the same test file.
// Exit status 2: a file error or a malformed request.
#include <cstdio>
#include <cstring>
#include <vector>

#include "okvis2_amd/csrc/ransac_hyp_dev.h"

using namespace okvfe;

namespace {

struct Reader {
  const std::vector<unsigned char>& b;
  size_t o = 0;
  bool ok = true;
  void get(void* dst, size_t n) {
    if (o + n > b.size()) {
      ok = false;
      std::memset(dst, 0, n);
      return;
    }
    std::memcpy(dst, b.data() + o, n);
    o += n;
  }
  int32_t i32() {
    int32_t v;
    get(&v, 4);
    return v;
  }
  uint64_t u64() {
    uint64_t v;
    get(&v, 8);
    return v;
  }
};

struct Record {
  double p[3], b[3], sigma;
  int32_t cam, row;
};
static_assert(sizeof(Record) == 64, "7 doubles and two ints");

template <bool kTree>
struct TestDistance {
  static double sum3(double a, double b, double c) { return kTree ? a + (b + c) : (a + b) + c; }
  static double sum4(double a, double b, double c, double d) { return kTree ? (a + b) + (c + d) : ((a + b) + c) + d; }
  double operator()(const double* H, const double* p, const double* C, const double* r, const double* b,
                    double sigma) const {
    double ti[3], d[3], rep[3], e[3];
    for (int i = 0; i < 3; ++i) ti[i] = sum3((-H[i]) * H[3], (-H[4 + i]) * H[7], (-H[8 + i]) * H[11]);
    for (int i = 0; i < 3; ++i) d[i] = sum4(H[i] * p[0], H[4 + i] * p[1], H[8 + i] * p[2], ti[i] * 1.0) - r[i];
    for (int i = 0; i < 3; ++i) rep[i] = sum3(C[i] * d[0], C[3 + i] * d[1], C[6 + i] * d[2]);
    const double n = __builtin_sqrt(sum3(rep[0] * rep[0], rep[1] * rep[1], rep[2] * rep[2]));
    for (int i = 0; i < 3; ++i) e[i] = rep[i] / n - b[i];
    return sum3(e[0] * e[0], e[1] * e[1], e[2] * e[2]) / sigma;
  }
};

struct RangeOf {
  const std::vector<Record>& list;
  void operator()(int i, int* b, int* e) const {
    const int c = list[(size_t)i].cam, n = (int)list.size();
    int lo = i, hi = i;
    while (lo > 0 && list[(size_t)lo - 1].cam == c) --lo;
    while (hi < n && list[(size_t)hi].cam == c) ++hi;
    *b = lo;
    *e = hi;
  }
};

template <bool kTree>
int run(Reader& in, int n_multiframes, uint64_t seed, std::FILE* out) {
  for (int m = 0; m < n_multiframes; ++m) {
    const uint64_t key = in.u64();
    const int n_hyp = in.i32(), n_cams = in.i32(), K = in.i32(), gate = in.i32(), n = in.i32();
    if (!in.ok || n_hyp < 0 || n_cams < 1 || K < 1 || n < 0) return 2;
    std::vector<double> rig((size_t)n_cams * 12);
    in.get(rig.data(), rig.size() * sizeof(double));
    std::vector<Record> list((size_t)n);
    if (n) in.get(list.data(), list.size() * sizeof(Record));
    if (!in.ok) return 2;
    for (const Record& r : list)
      if (r.cam < 0 || r.cam >= n_cams) return 2;
    for (int h = 0; h < n_hyp; ++h) {
      double H[12] = {0};
      int32_t tail[6] = {-1, -1, -1, -1, 0, 0};
      if (gate != 0) {
        int pos[4];
        const int drawn = hyp_sample(seed, key, h, n, RangeOf{list}, pos);
        for (int j = 0; j < 4; ++j)
          if (pos[j] >= 0) tail[j] = list[(size_t)pos[j]].cam * K + list[(size_t)pos[j]].row;
        if (drawn == 4) {
          double P[12], f[12];
          for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 3; ++i) {
              P[3 * j + i] = list[(size_t)pos[j]].p[i];
              f[3 * j + i] = list[(size_t)pos[j]].b[i];
            }
          const double* T = rig.data() + 12 * (size_t)list[(size_t)pos[0]].cam;
          int n_sol = 0;
          tail[5] = p3p_hypothesis(P, f, list[(size_t)pos[3]].sigma, T, T + 9, H, &n_sol, TestDistance<kTree>{}) ? 1 : 0;
          tail[4] = n_sol;
        }
      }
      if (std::fwrite(H, sizeof H, 1, out) != 1 || std::fwrite(tail, sizeof tail, 1, out) != 1) return 2;
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s request response\n", argv[0]);
    return 2;
  }
  std::vector<unsigned char> bytes;
  {
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
  }
  Reader in{bytes};
  const int tree = in.i32(), n_multiframes = in.i32();
  const uint64_t seed = in.u64();
  if (!in.ok || n_multiframes < 0) return 2;
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const int rc = tree ? run<true>(in, n_multiframes, seed, out) : run<false>(in, n_multiframes, seed, out);
  if (std::fclose(out) != 0) return 2;
  if (rc == 0 && in.o != bytes.size()) return 2;
  return rc;
}
