// place_refine_step_main.cpp -- okvis2_amd/csrc/place_refine_dev.h as a stand-alone host program: the solver of the
// pose refinement of verifyRecognisedPlace driven by evaluation records from a file, for tests/test_place_refine_host.py
// (which builds it twice, once with the sanitizers).  No device work, no library.
//   request:  int32 tree, n_multiframes, max_iterations; per multiframe int32 mode (0: a 3 x 4 hypothesis, 12 doubles;
//             1: an initial pose, 7 doubles; 2: a winner outside the list, nothing), int32 n_evaluations, then that many
//             PlaceRefineEval records (232 bytes): the evaluation at the start pose, then one per candidate
//   response: per multiframe and evaluation the PlaceRefineRecord after the call that consumed it (the first call is
//             refine_adopt_start followed by refine_advance, the later ones refine_advance alone)
// Exit status 2: a file error; 3: a multiframe asked for more or fewer evaluations than the request holds.
#include <cstdio>
#include <cstring>
#include <vector>

#include "okvis2_amd/csrc/place_refine_dev.h"

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
};

template <bool kTree>
int run(Reader& in, int n_multiframes, int max_iterations, std::FILE* out) {
  for (int m = 0; m < n_multiframes; ++m) {
    const int mode = in.i32(), n_eval = in.i32();
    double x[7];
    if (mode == 0) {
      double Hm[12];
      in.get(Hm, sizeof Hm);
      start_pose(Hm, x);
    } else if (mode == 1) {
      in.get(x, sizeof x);
    } else {
      for (double& v : x) v = elementary_nan();
    }
    if (!in.ok || n_eval < 1) return 2;
    PlaceRefineRecord r;
    std::memset(&r, 0, sizeof r);
    refine_init(r, x, mode == 2);
    for (int k = 0; k < n_eval; ++k) {
      PlaceRefineEval e;
      in.get(&e, sizeof e);
      if (!in.ok) return 2;
      if (k == 0) {
        refine_adopt_start(r, e);
      } else if (!r.pending || r.status != kRefineRunning) {
        return 3;  // the solver has ended, the request goes on
      }
      refine_advance<kTree>(r, e, max_iterations);
      if (std::fwrite(&r, sizeof r, 1, out) != 1) return 2;
    }
    if (r.status == kRefineRunning) return 3;  // the solver waits for an evaluation the request does not hold
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
  const int tree = in.i32(), n_multiframes = in.i32(), max_iterations = in.i32();
  if (!in.ok || n_multiframes < 0) return 2;
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  const int rc = tree ? run<true>(in, n_multiframes, max_iterations, out) : run<false>(in, n_multiframes, max_iterations, out);
  if (std::fclose(out) != 0) return 2;
  if (rc == 0 && in.o != bytes.size()) return 3;
  return rc;
}
