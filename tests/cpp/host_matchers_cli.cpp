// host_matchers_cli.cpp -- drives the host-buffer matchers of okvfe::HipFrontend (matchStereo, matchMotionStereo,
// matchToMap, matchToMapPooled, matchToMapUninitialised, verifyRecognisedPlace) on a real context from a binary request
// file: FrameData objects filled from arrays (no images, no detection), every returned container written out.
// Compiled and run by tests/test_gpu_cpp_matchers.py.
// request : int32 n_cams | per camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[8] } | int32 K, match threshold | int32 n_ops |
//           per op { int32 kind | ... } with
//             frame = int32 n | keypoints n*28 B | descriptors n*48 B | back-projections n*3 f64 | valid n u8
//             vec<T> = int32 n | n*T            pose = 12 f64 (C row-major, r)
//   0 matchStereo            : int32 im0, im1 | frame f0, f1 | pose T_WC0, T_WC1
//   1 matchMotionStereo      : int32 cam | frame f0, f1 | pose T_WC0, T_WC1 | vec<u8> skip0, matched1
//   2 matchToMap             : int32 cam | frame | int32 nl,no,np | hp nl*4 f64 | quality nl f64 | obs_begin (nl+1) i32 |
//                              obs_pose no i32 | obs_desc no*48 B | obs_bp no*3 f64 | poses np*12 f64 | pose T_WC1 |
//                              f64 threshold | int32 exclusive | vec<u8> use | int32 with_pool
//   3 matchToMapPooled       : int32 cam | frame | vec<u8> use | vec<f64> projections | vec<i32> descBegin | vec<u8> pool |
//                              f64 threshold
//   4 matchToMapUninitialised: int32 cam | frame | vec<u8> use | vec<i32> previous | vec<i32> descBegin | vec<u8> pool |
//                              vec<f64> e0_W, r0_W | pose T_WC1
//   5 verifyRecognisedPlace  : int32 cam | vec<u8> landmarkDescriptors | vec<i32> descBegin | frame
// response: per op, in order: 0: rows n0*sizeof(okvfe_stereo_match) | 1: rows n0*sizeof(okvfe_motion_match) |
//           2: landmark n i32, distance n i32 [, status nl i32, n_desc nl i32, obs_rows nl*3 i32, projection nl*2 f64,
//           e_W nl*6 f64, r_W nl*6 f64] | 3: landmark, distance | 4: landmark, distance, hp_W n*4 f64, hpSet n u8,
//           alreadyMatched i32 | 5: kMin nl i32, distMin nl u32
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"

static FILE* in = nullptr;
static FILE* out = nullptr;

template <typename T>
static std::vector<T> rdv(size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, in) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}
static int32_t rdi() { return rdv<int32_t>(1)[0]; }
static double rdd() { return rdv<double>(1)[0]; }
template <typename T>
static std::vector<T> vec() {
  const int32_t n = rdi();
  return rdv<T>(size_t(n));
}
static okvfe_pose pose() { return rdv<okvfe_pose>(1)[0]; }
static okvfe::FrameData frame() {
  okvfe::FrameData f;
  const size_t n = size_t(rdi());
  f.keypoints = rdv<okvfe::KeyPoint>(n);
  f.descriptors.data = rdv<uint8_t>(n * 48);
  f.descriptors.rows = int(n);
  f.backProjections = rdv<std::array<double, 3>>(n);
  f.backProjectionsValid = rdv<uint8_t>(n);
  f.landmarkIds.assign(n, 0);
  return f;
}
template <typename T>
static void put(const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), out) != v.size()) exit(3);
}
static void put(const okvfe::HipFrontend::MapMatches& m) {
  put(m.landmark);
  put(m.distance);
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  static_assert(sizeof(std::array<double, 3>) == 24 && sizeof(okvfe::KeyPoint) == 28, "request layout");
  const int32_t n_cams = rdi();
  std::vector<okvfe_camera_ext> cams;
  for (int m = 0; m < n_cams; ++m) {
    const std::vector<int32_t> ci = rdv<int32_t>(3);
    const std::vector<double> cd = rdv<double>(12);
    okvfe_camera_ext cam{};
    cam.base.width = ci[0]; cam.base.height = ci[1]; cam.base.distortion = ci[2];
    cam.base.fu = cd[0]; cam.base.fv = cd[1]; cam.base.cu = cd[2]; cam.base.cv = cd[3];
    for (int i = 0; i < 4; ++i) cam.base.d[i] = cd[4 + i];
    for (int i = 0; i < 4; ++i) cam.d_ext[i] = cd[8 + i];
    cams.push_back(cam);
  }
  okvfe::FrontendParameters p{};
  p.max_num_keypoints = rdi();
  p.matching_threshold = rdi();
  const int32_t n_ops = rdi();
  try {
    okvfe::HipFrontend fe(cams, p);
    for (int op = 0; op < n_ops; ++op) {
      const int32_t kind = rdi();
      if (kind == 0) {
        const size_t im0 = size_t(rdi()), im1 = size_t(rdi());
        const okvfe::FrameData f0 = frame(), f1 = frame();
        const okvfe_pose T0 = pose(), T1 = pose();
        put(fe.matchStereo(im0, f0, T0, im1, f1, T1));
      } else if (kind == 1) {
        const size_t cam = size_t(rdi());
        const okvfe::FrameData f0 = frame(), f1 = frame();
        const okvfe_pose T0 = pose(), T1 = pose();
        const std::vector<uint8_t> skip0 = vec<uint8_t>(), matched1 = vec<uint8_t>();
        put(fe.matchMotionStereo(cam, f0, T0, f1, T1, skip0, matched1));
      } else if (kind == 2) {
        const size_t cam = size_t(rdi());
        const okvfe::FrameData f = frame();
        const std::vector<int32_t> tn = rdv<int32_t>(3);
        const size_t nl = size_t(tn[0]), no = size_t(tn[1]), np = size_t(tn[2]);
        const std::vector<double> hp = rdv<double>(nl * 4), quality = rdv<double>(nl);
        const std::vector<int32_t> obs_begin = rdv<int32_t>(nl + 1), obs_pose = rdv<int32_t>(no);
        const std::vector<uint8_t> obs_desc = rdv<uint8_t>(no * 48);
        const std::vector<double> obs_bp = rdv<double>(no * 3);
        const std::vector<okvfe_pose> poses = rdv<okvfe_pose>(np);
        const okvfe_pose T1 = pose();
        const double threshold = rdd();
        const bool exclusive = rdi() != 0;
        const std::vector<uint8_t> use = vec<uint8_t>();
        const bool with_pool = rdi() != 0;
        const okvfe_landmark_table table{tn[0], tn[1], tn[2], hp.data(), quality.data(), obs_begin.data(), obs_pose.data(),
                                         obs_desc.data(), obs_bp.data(), poses.data()};
        std::vector<int32_t> status(nl), n_desc(nl), obs_rows(nl * 3);
        std::vector<double> projection(nl * 2), e_W(nl * 6), r_W(nl * 6);
        okvfe_landmark_pool pool{status.data(), n_desc.data(), obs_rows.data(), projection.data(), e_W.data(), r_W.data()};
        put(fe.matchToMap(cam, f, table, T1, threshold, exclusive, use, with_pool ? &pool : nullptr));
        if (with_pool) {
          put(status); put(n_desc); put(obs_rows); put(projection); put(e_W); put(r_W);
        }
      } else if (kind == 3) {
        const size_t cam = size_t(rdi());
        const okvfe::FrameData f = frame();
        const std::vector<uint8_t> use = vec<uint8_t>();
        const std::vector<double> projections = vec<double>();
        const std::vector<int32_t> begin = vec<int32_t>();
        const std::vector<uint8_t> pool = vec<uint8_t>();
        const double threshold = rdd();
        put(fe.matchToMapPooled(cam, f, use, projections, begin, pool, threshold));
      } else if (kind == 4) {
        const size_t cam = size_t(rdi());
        const okvfe::FrameData f = frame();
        const std::vector<uint8_t> use = vec<uint8_t>();
        const std::vector<int32_t> previous = vec<int32_t>(), begin = vec<int32_t>();
        const std::vector<uint8_t> pool = vec<uint8_t>();
        const std::vector<double> e0 = vec<double>(), r0 = vec<double>();
        const okvfe_pose T1 = pose();
        const okvfe::HipFrontend::UninitialisedMatches u = fe.matchToMapUninitialised(cam, f, use, previous, begin, pool, e0, r0, T1);
        put(u.matches);
        put(u.hp_W);
        put(u.hpSet);
        put(std::vector<int32_t>{u.alreadyMatched});
      } else if (kind == 5) {
        const size_t cam = size_t(rdi());
        const std::vector<uint8_t> lm = vec<uint8_t>();
        const std::vector<int32_t> begin = vec<int32_t>();
        const okvfe::FrameData f = frame();
        const okvfe::HipFrontend::PlaceMatches m = fe.verifyRecognisedPlace(cam, lm, begin, f);
        put(m.kMin);
        put(m.distMin);
      } else {
        fprintf(stderr, "unknown op %d\n", kind);
        return 2;
      }
    }
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  fclose(in);
  fclose(out);
  return 0;
}
