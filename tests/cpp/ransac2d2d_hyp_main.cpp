// ransac2d2d_hyp_main.cpp -- okvis2_amd/csrc/ransac2d2d_hyp_dev.h as a stand-alone host program: the sampler, the
// two-point rotation, the five-point solver and the choice among its candidates driven by correspondence lists from a
// file, for tests/test_ransac2d2d_hyp_host.py (which builds it twice, once with the sanitizers).  No device work, no
// library.
//   request:  int32 tree, n_lists; uint64 seed; per list (one camera of one pair) uint64 pair_key, int32 cam, n_hyp, n,
//             pad; n records of 8 doubles (b1, b2, s1, s2) and int32 kA, pad
//   response: per list and hypothesis 9 doubles (M), 12 doubles ([R | t]), int32 rot_samples[2], rel_samples[8] (kA or
//             -1), n_roots, rot_valid, rel_valid, pad
// The header takes the distance of the consensus as a functor (in the library: the consensus kernel's own functions,
// which are HIP code).  TestDistance below is this program's transcription of tests/ransac2d2d_ref.py's
// `relative_distances`, line by line; the library's copy is held to the same restatement by okvfe_fivept_hypothesis in
// the same test file.
// Exit status 2: a file error or a malformed request.
#include <cstdio>
#include <cstring>
#include <vector>

#include "okvis2_amd/csrc/ransac2d2d_hyp_dev.h"

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
  double b1[3], b2[3], s1, s2;
  int32_t kA, pad;
};
static_assert(sizeof(Record) == 72, "8 doubles and two ints");

struct Answer {
  double M[9], H[12];
  int32_t rot_samples[2], rel_samples[8], n_roots, rot_valid, rel_valid, pad;
};
static_assert(sizeof(Answer) == 224, "21 doubles and 14 ints");

template <bool kTree>
struct TestDistance {
  static double sum3(double a, double b, double c) { return kTree ? a + (b + c) : (a + b) + c; }
  static double sum4(double a, double b, double c, double d) { return kTree ? (a + b) + (c + d) : ((a + b) + c) + d; }
  static double dot(const double* a, const double* b) { return sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2]); }
  static double one(const double* H, const double* ti, const double* b1, const double* b2, double s1, double s2) {
    const double t[3] = {H[3], H[7], H[11]};
    double f2u[3], p[3], rep2[3], e1[3], e2[3];
    for (int i = 0; i < 3; ++i) f2u[i] = sum3(H[4 * i] * b2[0], H[4 * i + 1] * b2[1], H[4 * i + 2] * b2[2]);
    const double c0 = dot(t, b1), c1 = dot(t, f2u);
    const double A00 = dot(b1, b1), A10 = dot(b1, f2u);
    const double A01 = -A10, A11 = -dot(f2u, f2u);
    const double det = A00 * A11 - A10 * A01;
    const double invdet = 1.0 / det;
    const double I00 = A11 * invdet, I10 = (-A10) * invdet, I01 = (-A01) * invdet, I11 = A00 * invdet;
    const double l0 = I00 * c0 + I01 * c1, l1 = I10 * c0 + I11 * c1;
    for (int i = 0; i < 3; ++i) p[i] = (l0 * b1[i] + (t[i] + l1 * f2u[i])) / 2.0;
    for (int i = 0; i < 3; ++i) rep2[i] = sum4(H[i] * p[0], H[4 + i] * p[1], H[8 + i] * p[2], ti[i] * 1.0);
    const double n1 = __builtin_sqrt(dot(p, p)), n2 = __builtin_sqrt(dot(rep2, rep2));
    for (int i = 0; i < 3; ++i) {
      e1[i] = p[i] / n1 - b1[i];
      e2[i] = rep2[i] / n2 - b2[i];
    }
    return (dot(e1, e1) * 0.5) / s1 + (dot(e2, e2) * 0.5) / s2;
  }
  double operator()(const double* H, const double* b1, const double* b2, const double* s1, const double* s2) const {
    double ti[3], d[3];
    for (int i = 0; i < 3; ++i) ti[i] = sum3((-H[i]) * H[3], (-H[4 + i]) * H[7], (-H[8 + i]) * H[11]);
    for (int j = 0; j < 3; ++j) d[j] = one(H, ti, b1 + 3 * j, b2 + 3 * j, s1[j], s2[j]);
    return (d[0] + d[1]) + d[2];
  }
};

template <bool kTree>
int run(Reader& in, int n_lists, uint64_t seed, std::FILE* out) {
  for (int m = 0; m < n_lists; ++m) {
    const uint64_t pair_key = in.u64();
    const int cam = in.i32(), n_hyp = in.i32(), n = in.i32();
    in.i32();
    if (!in.ok || cam < 0 || cam >= 64 || n_hyp < 0 || n < 0) return 2;
    std::vector<Record> list((size_t)n);
    if (n) in.get(list.data(), list.size() * sizeof(Record));
    if (!in.ok) return 2;
    for (int h = 0; h < n_hyp; ++h) {
      Answer a;
      std::memset(&a, 0, sizeof a);
      for (int j = 0; j < 2; ++j) a.rot_samples[j] = -1;
      for (int j = 0; j < 8; ++j) a.rel_samples[j] = -1;
      if (n >= kHyp2MinCorrespondences) {
        int p2[kHyp2RotSamples], p8[kHyp2RelSamples];
        hyp2_sample<kHyp2RotSamples>(seed, hyp2_key(pair_key, cam, 0), h, n, p2);
        double b1[24], b2[24], s1[3], s2[3];
        for (int j = 0; j < 2; ++j) {
          const Record& r = list[(size_t)p2[j]];
          a.rot_samples[j] = r.kA;
          for (int i = 0; i < 3; ++i) {
            b1[3 * j + i] = r.b1[i];
            b2[3 * j + i] = r.b2[i];
          }
        }
        a.rot_valid = twopt_rotation(b1, b2, a.M) ? 1 : 0;
        hyp2_sample<kHyp2RelSamples>(seed, hyp2_key(pair_key, cam, 1), h, n, p8);
        for (int j = 0; j < 8; ++j) {
          const Record& r = list[(size_t)p8[j]];
          a.rel_samples[j] = r.kA;
          for (int i = 0; i < 3; ++i) {
            b1[3 * j + i] = r.b1[i];
            b2[3 * j + i] = r.b2[i];
          }
          if (j >= 5) {
            s1[j - 5] = r.s1;
            s2[j - 5] = r.s2;
          }
        }
        double ws[kFiveptWork];
        int n_roots = 0;
        a.rel_valid = fivept_hypothesis(b1, b2, s1, s2, ws, a.H, &n_roots, TestDistance<kTree>{}) ? 1 : 0;
        a.n_roots = n_roots;
      }
      if (std::fwrite(&a, sizeof a, 1, out) != 1) return 2;
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
  const int tree = in.i32(), n_lists = in.i32();
  const uint64_t seed = in.u64();
  if (!in.ok || n_lists < 0) return 2;
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const int rc = tree ? run<true>(in, n_lists, seed, out) : run<false>(in, n_lists, seed, out);
  if (std::fclose(out) != 0) return 2;
  if (rc == 0 && in.o != bytes.size()) return 2;
  return rc;
}
