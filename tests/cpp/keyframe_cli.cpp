// keyframe_cli.cpp -- drives okvfe::HipFrontend::doWeNeedANewKeyframe (the C++ host mirror of
// okvis::Frontend::doWeNeedANewKeyframe, Frontend.cpp:1058-1167) from a binary request file; used by
// tests/test_gpu_keyframe_cpp.py.
// request : int32 w,h,ncams,nothers | float threshold | (1 + nothers) multiframes (the current one first), each
//           ncams x { int32 n | n*28 keypoints | n*8 landmark ids (u64) }
// response: int32 need | f64 overlap | int32 need with no other frames | f64 its overlap
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"

template <typename T>
static void rd(FILE* f, T* p, size_t n) {
  if (n && fread(p, sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  int32_t hdr[4];
  rd(f, hdr, 4);
  const int w = hdr[0], h = hdr[1], ncams = hdr[2], nothers = hdr[3];
  float threshold;
  rd(f, &threshold, 1);
  std::vector<std::vector<okvfe::FrameData>> frames(size_t(1 + nothers), std::vector<okvfe::FrameData>(size_t(ncams)));
  for (auto& multiframe : frames)
    for (okvfe::FrameData& fd : multiframe) {
      int32_t n;
      rd(f, &n, 1);
      fd.keypoints.resize(size_t(n));
      fd.landmarkIds.resize(size_t(n));
      rd(f, fd.keypoints.data(), size_t(n));
      rd(f, fd.landmarkIds.data(), size_t(n));
    }
  fclose(f);
  std::vector<okvfe_camera> cams(size_t(ncams), okvfe_camera{});
  for (okvfe_camera& c : cams) {
    c.width = w; c.height = h;
    c.fu = c.fv = 0.6 * w; c.cu = 0.5 * w; c.cv = 0.5 * h;
  }
  try {
    okvfe::HipFrontend frontend(cams, okvfe::FrontendParameters{});
    const std::vector<std::vector<okvfe::FrameData>> others(frames.begin() + 1, frames.end());
    double overlap = -1.0, overlapAlone = -1.0;
    const int32_t need = frontend.doWeNeedANewKeyframe(frames[0], others, threshold, &overlap) ? 1 : 0;
    const int32_t needAlone = frontend.doWeNeedANewKeyframe(frames[0], {}, threshold, &overlapAlone) ? 1 : 0;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    fwrite(&need, 4, 1, o);
    fwrite(&overlap, 8, 1, o);
    fwrite(&needAlone, 4, 1, o);
    fwrite(&overlapAlone, 8, 1, o);
    fclose(o);
    // error behaviour: a multiframe with the wrong number of cameras throws
    bool threw = false;
    try {
      frontend.doWeNeedANewKeyframe(std::vector<okvfe::FrameData>(size_t(ncams) + 1), {});
    } catch (const okvfe::Exception&) {
      threw = true;
    }
    if (!threw) return 3;
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
