// scratch_layout_main.cpp -- okvis2_amd/csrc/scratch_layout.h on the host, nothing of HIP, for
// tests/test_scratch_layout_host.py: lays out sequences of region sizes and checks what the host-array entry points
// rely on.  Exit status 0 and "ok <sequences> <regions>" on stdout, or the first violation on stderr and status 1.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "okvis2_amd/csrc/scratch_layout.h"

namespace {
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int check(const std::vector<size_t>& sizes, size_t* regions) {
  // the reference: the lambda every host-array entry point carried before it had a layout type
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + std::max<size_t>(bytes, 1), 256); return o; };
  okvfe::ScratchLayout lay;
  std::vector<size_t> at;
  for (size_t bytes : sizes) {
    const size_t want = take(bytes), got = lay.take(bytes);
    if (got != want) return std::fprintf(stderr, "offset %zu, the lambda gives %zu\n", got, want), 1;
    if (got % 256) return std::fprintf(stderr, "offset %zu is no multiple of 256\n", got), 1;
    at.push_back(got);
  }
  if (lay.total() != off || lay.total() % 256)
    return std::fprintf(stderr, "total %zu, the lambda gives %zu\n", lay.total(), off), 1;
  for (size_t i = 0; i < at.size(); ++i) {
    const size_t len = std::max<size_t>(sizes[i], 1);  // an empty array still owns a byte at an address of its own
    if (at[i] + len > lay.total()) return std::fprintf(stderr, "region %zu ends beyond total()\n", i), 1;
    for (size_t j = 0; j < i; ++j)
      if (at[j] == at[i] || at[j] + std::max<size_t>(sizes[j], 1) > at[i])
        return std::fprintf(stderr, "regions %zu and %zu overlap\n", j, i), 1;
  }
  // ... and in memory: every region written in full inside a buffer of exactly total() bytes, each byte by one region
  // only (the sanitised build faults on a write outside the buffer)
  std::vector<unsigned char> buf(lay.total(), 0);
  for (size_t i = 0; i < at.size(); ++i) {
    const size_t len = std::max<size_t>(sizes[i], 1);
    for (size_t k = 0; k < len; ++k)
      if (buf[at[i] + k]++) return std::fprintf(stderr, "byte %zu written twice\n", at[i] + k), 1;
  }
  *regions += at.size();
  return 0;
}
}  // namespace

int main() {
  const std::vector<size_t> edge = {0, 1, 255, 256, 257, (size_t)700 * 48};
  size_t sequences = 0, regions = 0;
  auto run = [&](const std::vector<size_t>& s) { ++sequences; return check(s, &regions); };
  if (run({})) return 1;
  for (size_t a : edge) {
    if (run({a})) return 1;
    for (size_t b : edge) {
      if (run({a, b})) return 1;
      for (size_t c : edge)
        if (run({a, b, c}) || run({a, b, c, 0, 0, 4})) return 1;
    }
  }
  std::vector<size_t> all = edge;
  std::sort(all.begin(), all.end());
  do {
    if (run(all)) return 1;
  } while (std::next_permutation(all.begin(), all.end()));
  // the shapes of the stereo matcher: a record, a table, four arrays per frame, the result -- full, one-sided and empty
  for (size_t n0 : {(size_t)0, (size_t)1, (size_t)3, (size_t)700})
    for (size_t n1 : {(size_t)0, (size_t)2, (size_t)700})
      if (run({200, 2 * 64 * 8, n0 * 48, n0 * 24, n0, n0 * 16, n1 * 48, n1 * 24, n1, n1 * 16, n0 * 48})) return 1;
  std::printf("ok %zu %zu\n", sequences, regions);
  return 0;
}
