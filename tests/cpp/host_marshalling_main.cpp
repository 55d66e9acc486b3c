// host_marshalling_main.cpp -- CPU check of what okvfe::HipFrontend's host-buffer matchers (matchStereo,
// matchMotionStereo, matchToMap, matchToMapPooled, matchToMapUninitialised, verifyRecognisedPlace) hand to the library:
// every scalar, every array (by checksum), which camera and which context, and how the outputs come back -- against the
// recording stand-in tests/cpp/fake_okvfe.cpp, under AddressSanitizer, so an array passed on too short is an error.
// Ill-formed calls must throw okvfe::Exception(OKVFE_ERR_INVALID_ARGUMENT) before the stand-in is reached.
// Built with the three OKVFE_* defines of adapters_check.cpp and -I tests/mock it also checks the hook route of
// okvfe::HipViFrontend.  Compiled, linked to the stand-in and run by tests/test_host_marshalling.py; never linked against
// libokvfe.so.
#define FAKE_OKVFE_DECLARATIONS_ONLY  // namespace fake alone; the stand-in itself is linked as its own object
#include "fake_okvfe.cpp"

#ifdef OKVFE_WITH_OKVIS
#include "../../okvis2_amd/host/okvfe_okvis_frontend.hpp"
#else
#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#endif

#include <cstdio>
#include <functional>

using okvfe::FrameData;
using okvfe::HipFrontend;

namespace {

int failures = 0;
void fail(const std::string& what) {
  ++failures;
  std::fprintf(stderr, "FAIL: %s\n", what.c_str());
}
void expect(bool ok, const std::string& what) {
  if (!ok) fail(what);
}

okvfe_camera_ext camera(int model) {  // 0: 320 x 240 radial-tangential; 1: 640 x 480 RADTAN8
  okvfe_camera_ext c{};
  c.base.width = model ? 640 : 320;
  c.base.height = model ? 480 : 240;
  c.base.fu = model ? 350.0 : 200.0;
  c.base.fv = model ? 360.0 : 210.0;
  c.base.cu = model ? 318.0 : 161.0;
  c.base.cv = model ? 239.0 : 119.0;
  c.base.distortion = model ? OKVFE_DIST_RADTAN8 : OKVFE_DIST_RADTAN;
  for (int i = 0; i < 4; ++i) c.base.d[i] = (model ? 0.01 : -0.02) * (i + 1);
  if (model)
    for (int i = 0; i < 4; ++i) c.d_ext[i] = 0.003 * (i + 1);
  return c;
}

okvfe_pose pose(double s) {
  okvfe_pose T{};
  for (int i = 0; i < 9; ++i) T.C[i] = s + 0.01 * i;
  for (int i = 0; i < 3; ++i) T.r[i] = -s - 0.1 * i;
  return T;
}

uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

FrameData makeFrame(size_t n, uint32_t seed) {  // exact-size vectors: one byte past any of them is an ASan error
  FrameData f;
  f.keypoints = std::vector<okvfe::KeyPoint>(n);
  f.descriptors.data = std::vector<uint8_t>(n * 48);
  f.descriptors.rows = int(n);
  f.landmarkIds = std::vector<uint64_t>(n, 0);
  f.backProjections = std::vector<std::array<double, 3>>(n);
  f.backProjectionsValid = std::vector<uint8_t>(n);
  for (size_t k = 0; k < n; ++k) {
    f.keypoints[k] = okvfe::KeyPoint{float(seed + k), float(2 * seed + k), 12.0f, 0.5f * k, float(seed), 0, int32_t(k)};
    for (int i = 0; i < 3; ++i) f.backProjections[k][size_t(i)] = 0.001 * seed + 2.0 * double(k) + 0.125 * i * (i + 2);
    f.backProjectionsValid[k] = k % 3 != 1;
  }
  for (uint8_t& b : f.descriptors.data) b = uint8_t(lcg(seed) >> 24);
  return f;
}
std::vector<uint8_t> flags(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  for (uint8_t& b : v) b = (lcg(seed) >> 28) % 3 != 0;
  return v;
}
std::vector<double> reals(size_t n, uint32_t seed) {
  std::vector<double> v(n);
  for (double& d : v) d = double(lcg(seed) >> 8) / 1024.0;
  return v;
}
std::vector<uint8_t> bytes(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  for (uint8_t& b : v) b = uint8_t(lcg(seed) >> 24);
  return v;
}
std::vector<double> flat3(const FrameData& f) {
  std::vector<double> v;
  for (const auto& b : f.backProjections) v.insert(v.end(), b.begin(), b.end());
  return v;
}

// ---- what a call must look like --------------------------------------------------------------------------------------
void frameSide(fake::Call& e, const FrameData& f, const std::string& i, const std::vector<uint8_t>* optional,
               const std::string& optionalName) {
  e.buf.emplace_back("desc" + i, fake::fnv(f.descriptors.data));
  e.buf.emplace_back("kp" + i, fake::fnv(f.keypoints));
  e.buf.emplace_back("backproj" + i, fake::fnv(flat3(f)));
  e.buf.emplace_back("valid" + i, fake::fnv(f.backProjectionsValid));
  if (optional) {
    e.num.emplace_back(optionalName + " given", !optional->empty());
    e.buf.emplace_back(optionalName, fake::fnv(*optional));
  }
  e.num.emplace_back("n" + i, double(f.keypoints.size()));
}

void same(const fake::Call& got, const fake::Call& want, const std::string& what) {
  if (got.padded_null) fail(what + ": a padded array (back-projections / hps_W) arrived as a null pointer");
  if (got == want) return;
  fail(what + ": the call differs from what the arguments say");
  std::fprintf(stderr, "  got %s on context %d, expected %s on context %d\n", got.fn.c_str(), got.ctx, want.fn.c_str(), want.ctx);
  for (size_t i = 0; i < std::max(got.num.size(), want.num.size()); ++i) {
    if (i < got.num.size() && i < want.num.size() && got.num[i] == want.num[i]) continue;
    std::fprintf(stderr, "  scalar %zu: got %s = %.17g, expected %s = %.17g\n", i, i < got.num.size() ? got.num[i].first.c_str() : "-",
                 i < got.num.size() ? got.num[i].second : 0.0, i < want.num.size() ? want.num[i].first.c_str() : "-",
                 i < want.num.size() ? want.num[i].second : 0.0);
  }
  for (size_t i = 0; i < std::max(got.buf.size(), want.buf.size()); ++i) {
    if (i < got.buf.size() && i < want.buf.size() && got.buf[i] == want.buf[i]) continue;
    std::fprintf(stderr, "  array %zu: got %s, expected %s: other bytes\n", i, i < got.buf.size() ? got.buf[i].first.c_str() : "-",
                 i < want.buf.size() ? want.buf[i].first.c_str() : "-");
  }
}

// the one call a well-formed wrapper call adds
const fake::Call& only(size_t before, const std::string& what) {
  static const fake::Call none;
  if (fake::calls().size() != before + 1) {
    fail(what + ": " + std::to_string(fake::calls().size() - before) + " library calls instead of one");
    return fake::calls().empty() ? none : fake::calls().back();
  }
  return fake::calls().back();
}

void mustThrow(const std::string& what, const std::function<void()>& call) {
  const size_t before = fake::calls().size();
  try {
    call();
    fail(what + ": no exception");
  } catch (const okvfe::Exception& e) {
    if (e.status != OKVFE_ERR_INVALID_ARGUMENT) fail(what + ": status " + std::to_string(int(e.status)) + ": " + e.what());
  }
  if (fake::calls().size() != before) fail(what + ": the library was reached");
}
// `good` one entry short and one entry long
template <typename V>
void shortAndLong(const std::string& what, const V& good, const std::function<void(const V&)>& call) {
  V s(good.begin(), good.end() - 1), l(good);
  l.push_back(good.back());
  mustThrow(what + " one short", [&] { call(s); });
  mustThrow(what + " one long", [&] { call(l); });
}
// the members of `good` a method reads, each one entry short and one entry long
void badFrames(const std::string& what, const FrameData& good, bool backProjections,
               const std::function<void(const FrameData&)>& call) {
  shortAndLong<std::vector<uint8_t>>(what + ": descriptors.data", good.descriptors.data, [&](const std::vector<uint8_t>& v) {
    FrameData f = good;
    f.descriptors.data = std::vector<uint8_t>(v);  // (a fresh allocation of exactly that size)
    call(f);
  });
  if (!backProjections) return;
  shortAndLong<std::vector<std::array<double, 3>>>(what + ": backProjections", good.backProjections,
                                                   [&](const std::vector<std::array<double, 3>>& v) {
                                                     FrameData f = good;
                                                     f.backProjections = std::vector<std::array<double, 3>>(v);
                                                     call(f);
                                                   });
  shortAndLong<std::vector<uint8_t>>(what + ": backProjectionsValid", good.backProjectionsValid,
                                     [&](const std::vector<uint8_t>& v) {
                                       FrameData f = good;
                                       f.backProjectionsValid = std::vector<uint8_t>(v);
                                       call(f);
                                     });
}

struct Rig {
  std::vector<okvfe_camera_ext> cams{camera(0), camera(1)};
  int first_ctx;  // creation order of camera 0's context
  HipFrontend fe;
  static int& created() {
    static int n = 0;
    return n;
  }
  static okvfe::FrontendParameters parameters() {
    okvfe::FrontendParameters p;
    p.max_num_keypoints = 64;
    return p;
  }
  Rig() : first_ctx(created()), fe(cams, parameters()) { created() += 2; }
  double focal(size_t cam) const { return 0.5 * (cams[cam].base.fu + cams[cam].base.fv); }
};

const size_t kCounts[3] = {0, 1, 5};
const std::vector<int32_t> kBegins[3] = {{0}, {0, 2}, {0, 1, 1, 4}};  // tables of 0, 1 and 3 landmarks (one without rows)

void checkRows(const std::string& what, const FrameData& f0, size_t got_size, const std::function<void(size_t, int32_t*, int32_t*, int32_t*, double*)>& row) {
  expect(got_size == f0.keypoints.size(), what + ": one row per keypoint of f0");
  const std::vector<double> bp = flat3(f0);
  for (size_t k = 0; k < std::min(got_size, f0.keypoints.size()); ++k) {
    int32_t k1, dist, ini, wk1, wdist, wini;
    double hp[4], whp[4];
    row(k, &k1, &dist, &ini, hp);
    fake::rule_match_row(f0.descriptors.data.data(), bp.data(), int(k), &wk1, &wdist, &wini, whp);
    expect(k1 == wk1 && dist == wdist && ini == wini && std::memcmp(hp, whp, sizeof(hp)) == 0, what + ": row " + std::to_string(k));
  }
}

void checkMapMatches(const std::string& what, const HipFrontend::MapMatches& m, const FrameData& f, const std::vector<uint8_t>& use) {
  const size_t n = f.keypoints.size();
  expect(m.landmark.size() == n && m.distance.size() == n, what + ": one entry per keypoint");
  if (m.landmark.size() != n || m.distance.size() != n) return;
  for (size_t k = 0; k < n; ++k)
    expect(m.landmark[k] == fake::rule_landmark(f.descriptors.data.data(), use.data(), int(k)) && m.distance[k] == fake::rule_dist(int(k)),
           what + ": keypoint " + std::to_string(k));
}

// ---- the six methods, well-formed -----------------------------------------------------------------------------------
void wellFormed() {
  Rig rig;
  HipFrontend& fe = rig.fe;
  const okvfe_pose T0 = pose(0.25), T1 = pose(0.75);
  for (int a = 0; a < 3; ++a)
    for (int given = 0; given < 2; ++given) {
      const size_t n0 = kCounts[a], n1 = kCounts[(a + 1) % 3];
      const FrameData f0 = makeFrame(n0, 11 + uint32_t(a)), f1 = makeFrame(n1, 23 + uint32_t(a));
      const std::string tag = " (" + std::to_string(n0) + " / " + std::to_string(n1) + " keypoints" + (given ? ", optional vectors given)" : ")");
      const std::vector<uint8_t> none;
      // matchStereo: camera pair (0, 1) and (1, 0)
      for (size_t im0 = 0; im0 < 2 && !given; ++im0) {
        const size_t im1 = 1 - im0, before = fake::calls().size();
        const std::vector<okvfe_stereo_match> out = fe.matchStereo(im0, f0, T0, im1, f1, T1);
        fake::Call e;
        e.fn = "okvfe_match_stereo";
        e.ctx = rig.first_ctx + int(im0);
        frameSide(e, f0, "0", nullptr, "");
        frameSide(e, f1, "1", nullptr, "");
        fake::add_pose(e, "T_WC0", T0);
        fake::add_pose(e, "T_WC1", T1);
        e.num.emplace_back("f0", rig.focal(im0));
        e.num.emplace_back("f1", rig.focal(im1));
        same(only(before, "matchStereo" + tag), e, "matchStereo" + tag);
        checkRows("matchStereo" + tag, f0, out.size(), [&](size_t k, int32_t* k1, int32_t* d, int32_t* i, double* hp) {
          *k1 = out[k].k1; *d = out[k].dist; *i = out[k].initialisable;
          std::memcpy(hp, out[k].hp_W, 32);
        });
      }
      // matchMotionStereo on either camera
      for (size_t cam = 0; cam < 2; ++cam) {
        const std::vector<uint8_t> skip0 = given ? flags(n0, 5) : none, matched1 = given ? flags(n1, 6) : none;
        const size_t before = fake::calls().size();
        const std::vector<okvfe_motion_match> out = fe.matchMotionStereo(cam, f0, T0, f1, T1, skip0, matched1);
        fake::Call e;
        e.fn = "okvfe_match_motion_stereo_ext";
        e.ctx = rig.first_ctx + int(cam);
        fake::add_camera(e, rig.cams[cam]);
        frameSide(e, f0, "0", &skip0, "skip0");
        frameSide(e, f1, "1", &matched1, "matched1");
        fake::add_pose(e, "T_WC0", T0);
        fake::add_pose(e, "T_WC1", T1);
        const std::string what = "matchMotionStereo, camera " + std::to_string(cam) + tag;
        same(only(before, what), e, what);
        checkRows(what, f0, out.size(), [&](size_t k, int32_t* k1, int32_t* d, int32_t* i, double* hp) {
          *k1 = out[k].k1; *d = out[k].dist; *i = out[k].initialisable;
          std::memcpy(hp, out[k].hp_W, 32);
          expect(out[k].accepted == int32_t((k & 2) >> 1) && out[k].cos_quality == 0.5 + 0.001 * double(k), what + ": accepted / cos_quality");
        });
      }
      // the map side: current frame f1 against tables of 0, 1 and 3 landmarks
      for (int t = 0; t < 3; ++t) {
        const std::vector<int32_t>& begin = kBegins[t];
        const size_t nl = begin.size() - 1, rows = size_t(begin.back()), cam = size_t(t & 1);
        const std::string tt = tag + ", " + std::to_string(nl) + " landmarks";
        const std::vector<uint8_t> use = given ? flags(n1, 7 + uint32_t(t)) : none, all(n1, 1);
        const std::vector<uint8_t> pool = bytes(rows * 48, 31 + uint32_t(t));
        const std::vector<double> proj = reals(nl * 2, 41), e0 = reals(rows * 3, 43), r0 = reals(rows * 3, 47);
        {  // matchToMapPooled
          const size_t before = fake::calls().size();
          const HipFrontend::MapMatches m = fe.matchToMapPooled(cam, f1, use, proj, begin, pool, 20.0 + t);
          fake::Call e;
          e.fn = "okvfe_match_to_map";
          e.ctx = rig.first_ctx + int(cam);
          e.buf = {{"desc", fake::fnv(f1.descriptors.data)}, {"kps", fake::fnv(f1.keypoints)}, {"use", fake::fnv(given ? use : all)},
                   {"projections", fake::fnv(proj)}, {"desc_begin", fake::fnv(begin)}, {"pool", fake::fnv(pool)}};
          e.num = {{"n_kps", double(n1)}, {"n_landmarks", double(nl)}, {"reprojection_threshold", 20.0 + t}};
          same(only(before, "matchToMapPooled" + tt), e, "matchToMapPooled" + tt);
          checkMapMatches("matchToMapPooled" + tt, m, f1, given ? use : all);
        }
        {  // matchToMapUninitialised: a keypoint takes part iff use (all, if empty) AND backProjectionsValid
          std::vector<int32_t> previous;
          if (given)
            for (size_t k = 0; k < n1; ++k) previous.push_back(k % 2 ? int32_t(k) : -1);
          std::vector<uint8_t> take(n1);
          for (size_t k = 0; k < n1; ++k) take[k] = (given ? use[k] : 1) && f1.backProjectionsValid[k];
          const std::vector<int32_t> nobody(n1, -1);
          const size_t before = fake::calls().size();
          const HipFrontend::UninitialisedMatches u = fe.matchToMapUninitialised(cam, f1, use, previous, begin, pool, e0, r0, T1);
          fake::Call e;
          e.fn = "okvfe_match_to_map_uninitialised";
          e.ctx = rig.first_ctx + int(cam);
          e.buf = {{"desc", fake::fnv(f1.descriptors.data)}, {"backproj", fake::fnv(flat3(f1))}, {"use", fake::fnv(take)},
                   {"previous_landmark", fake::fnv(given ? previous : nobody)}, {"desc_begin", fake::fnv(begin)},
                   {"pool", fake::fnv(pool)}, {"e0_W", fake::fnv(e0)}, {"r0_W", fake::fnv(r0)}};
          e.num = {{"n_kps", double(n1)}, {"n_landmarks", double(nl)}};
          fake::add_pose(e, "T_WC1", T1);
          e.num.emplace_back("focal_length", rig.focal(cam));
          const std::string what = "matchToMapUninitialised" + tt;
          same(only(before, what), e, what);
          checkMapMatches(what, u.matches, f1, take);
          expect(u.hp_W.size() == n1 && u.hpSet.size() == n1, what + ": hp_W / hpSet: one entry per keypoint");
          const std::vector<double> bp = flat3(f1);
          int32_t carried = 0;
          for (size_t k = 0; k < n1 && u.hp_W.size() == n1 && u.hpSet.size() == n1; ++k) {
            for (int i = 0; i < 4; ++i)
              expect(u.hp_W[k][size_t(i)] == fake::rule_hp(bp.data(), int(k), i), what + ": hp_W[" + std::to_string(k) + "][" + std::to_string(i) + "]");
            expect(u.hpSet[k] == take[k], what + ": hpSet");
            carried += given && previous[k] >= 0;
          }
          expect(u.alreadyMatched == carried, what + ": alreadyMatched");
        }
        {  // verifyRecognisedPlace
          const size_t before = fake::calls().size();
          const HipFrontend::PlaceMatches p = fe.verifyRecognisedPlace(cam, pool, begin, f1);
          fake::Call e;
          e.fn = "okvfe_verify_place_match";
          e.ctx = rig.first_ctx + int(cam);
          e.buf = {{"landmark_desc", fake::fnv(pool)}, {"desc_begin", fake::fnv(begin)}, {"frame_desc", fake::fnv(f1.descriptors.data)}};
          e.num = {{"n_landmarks", double(nl)}, {"n_kps", double(n1)}};
          const std::string what = "verifyRecognisedPlace" + tt;
          same(only(before, what), e, what);
          expect(p.kMin.size() == nl && p.distMin.size() == nl, what + ": one entry per landmark");
          for (size_t l = 0; l < nl && p.kMin.size() == nl && p.distMin.size() == nl; ++l)
            expect(p.kMin[l] == fake::rule_kmin(pool.data(), begin.data(), int(l)) && p.distMin[l] == fake::rule_distmin(int(l)),
                   what + ": landmark " + std::to_string(l));
        }
        {  // matchToMap from the raw table; with and without poolOut
          const size_t no = rows, np = 2;
          const std::vector<double> hp = reals(nl * 4, 51), quality = reals(nl, 53), obs_bp = reals(no * 3, 59);
          std::vector<int32_t> obs_pose(no);
          for (size_t o = 0; o < no; ++o) obs_pose[o] = int32_t(o % np);
          const std::vector<okvfe_pose> poses{pose(1.5), pose(2.5)};
          const okvfe_landmark_table table{int32_t(nl), int32_t(no), int32_t(np), hp.data(), quality.data(), begin.data(),
                                           obs_pose.data(), pool.data(), obs_bp.data(), poses.data()};
          std::vector<int32_t> status(nl), n_desc(nl), obs_rows(nl * 3);
          std::vector<double> projection(nl * 2), e_W(nl * 6), r_W(nl * 6);
          okvfe_landmark_pool out{status.data(), n_desc.data(), obs_rows.data(), projection.data(), e_W.data(), r_W.data()};
          const size_t before = fake::calls().size();
          const HipFrontend::MapMatches m = fe.matchToMap(cam, f1, table, T1, 150.0 - t, t == 2, use, given ? &out : nullptr);
          fake::Call e;
          e.fn = "okvfe_match_to_map_landmarks";
          e.ctx = rig.first_ctx + int(cam);
          e.num = {{"cam", 0.0}, {"n_landmarks", double(nl)}, {"n_observations", double(no)}, {"n_poses", double(np)}};
          fake::add_pose(e, "T_WC1", T1);
          e.num.insert(e.num.end(), {{"reprojection_threshold", 150.0 - t}, {"exclusive", t == 2 ? 1.0 : 0.0}, {"n_kps", double(n1)},
                                     {"pool_out given", double(given)}});
          e.buf = {{"hp_W", fake::fnv(hp)}, {"quality", fake::fnv(quality)}, {"obs_begin", fake::fnv(begin)},
                   {"obs_pose", fake::fnv(obs_pose)}, {"obs_desc", fake::fnv(pool)}, {"obs_backproj", fake::fnv(obs_bp)},
                   {"poses", fake::fnv(poses)}, {"desc", fake::fnv(f1.descriptors.data)}, {"kps", fake::fnv(f1.keypoints)},
                   {"use", fake::fnv(given ? use : all)}};
          const std::string what = "matchToMap" + tt;
          const bool first = a == 0 && given == 0 && t < 2;  // the first call on this camera sets the camera itself
          if (first) {
            expect(fake::calls().size() == before + 2, what + ": the first call on a camera is setCamera + the matcher");
            if (fake::calls().size() == before + 2) {
              fake::Call s;
              s.fn = "okvfe_set_camera_ext";
              s.ctx = rig.first_ctx + int(cam);
              s.num.emplace_back("cam", 0.0);
              fake::add_camera(s, rig.cams[cam]);
              same(fake::calls()[before], s, what + ": setCamera");
              same(fake::calls().back(), e, what);
            }
          } else {
            same(only(before, what), e, what);
          }
          checkMapMatches(what, m, f1, given ? use : all);
          for (size_t l = 0; l < nl && given; ++l) expect(status[l] == int32_t(l % 3), what + ": poolOut reached the library");
        }
      }
    }
}

// ---- ill-formed calls: OKVFE_ERR_INVALID_ARGUMENT before the library is reached --------------------------------------
void illFormed() {
  Rig rig;
  HipFrontend& fe = rig.fe;
  const okvfe_pose T0 = pose(0.25), T1 = pose(0.75);
  const FrameData f0 = makeFrame(5, 3), f1 = makeFrame(4, 4);
  const std::vector<uint8_t> skip0 = flags(5, 1), matched1 = flags(4, 2), use = flags(4, 3), none;
  const std::vector<int32_t> previous(4, -1), begin = kBegins[2], empty;
  const std::vector<uint8_t> pool = bytes(4 * 48, 9);
  const std::vector<double> proj = reals(6, 1), e0 = reals(12, 2), r0 = reals(12, 3);
  const size_t bad = fe.numCameras();
  using Bytes = std::vector<uint8_t>;
  using Reals = std::vector<double>;
  using Ints = std::vector<int32_t>;

  mustThrow("matchStereo: im0 = numCameras()", [&] { fe.matchStereo(bad, f0, T0, 1, f1, T1); });
  mustThrow("matchStereo: im1 = numCameras()", [&] { fe.matchStereo(0, f0, T0, bad, f1, T1); });
  badFrames("matchStereo: f0", f0, true, [&](const FrameData& f) { fe.matchStereo(0, f, T0, 1, f1, T1); });
  badFrames("matchStereo: f1", f1, true, [&](const FrameData& f) { fe.matchStereo(0, f0, T0, 1, f, T1); });

  mustThrow("matchMotionStereo: camera = numCameras()", [&] { fe.matchMotionStereo(bad, f0, T0, f1, T1); });
  shortAndLong<Bytes>("matchMotionStereo: skip0", skip0, [&](const Bytes& v) { fe.matchMotionStereo(0, f0, T0, f1, T1, v, matched1); });
  shortAndLong<Bytes>("matchMotionStereo: matched1", matched1, [&](const Bytes& v) { fe.matchMotionStereo(0, f0, T0, f1, T1, skip0, v); });
  badFrames("matchMotionStereo: f0", f0, true, [&](const FrameData& f) { fe.matchMotionStereo(1, f, T0, f1, T1); });
  badFrames("matchMotionStereo: f1", f1, true, [&](const FrameData& f) { fe.matchMotionStereo(1, f0, T0, f, T1); });

  const std::vector<double> hp = reals(12, 5), quality = reals(3, 6), obs_bp = reals(12, 7);
  const Ints obs_pose(4, 0);
  const std::vector<okvfe_pose> poses{pose(1.5)};
  const okvfe_landmark_table table{3, 4, 1, hp.data(), quality.data(), begin.data(), obs_pose.data(), pool.data(), obs_bp.data(), poses.data()};
  mustThrow("matchToMap: camera = numCameras()", [&] { fe.matchToMap(bad, f1, table, T1, 20.0, false); });
  shortAndLong<Bytes>("matchToMap: use", use, [&](const Bytes& v) { fe.matchToMap(0, f1, table, T1, 20.0, false, v); });
  badFrames("matchToMap: frame", f1, false, [&](const FrameData& f) { fe.matchToMap(0, f, table, T1, 20.0, false); });

  mustThrow("matchToMapPooled: camera = numCameras()", [&] { fe.matchToMapPooled(bad, f1, use, proj, begin, pool, 20.0); });
  mustThrow("matchToMapPooled: descBegin empty", [&] { fe.matchToMapPooled(0, f1, use, Reals(), empty, Bytes(), 20.0); });
  shortAndLong<Bytes>("matchToMapPooled: use", use, [&](const Bytes& v) { fe.matchToMapPooled(0, f1, v, proj, begin, pool, 20.0); });
  shortAndLong<Reals>("matchToMapPooled: projections", proj, [&](const Reals& v) { fe.matchToMapPooled(0, f1, use, v, begin, pool, 20.0); });
  shortAndLong<Bytes>("matchToMapPooled: pool", pool, [&](const Bytes& v) { fe.matchToMapPooled(0, f1, use, proj, begin, v, 20.0); });
  badFrames("matchToMapPooled: frame", f1, false, [&](const FrameData& f) { fe.matchToMapPooled(0, f, none, proj, begin, pool, 20.0); });

  mustThrow("matchToMapUninitialised: camera = numCameras()",
            [&] { fe.matchToMapUninitialised(bad, f1, use, previous, begin, pool, e0, r0, T1); });
  mustThrow("matchToMapUninitialised: descBegin empty",
            [&] { fe.matchToMapUninitialised(0, f1, use, previous, empty, Bytes(), Reals(), Reals(), T1); });
  shortAndLong<Bytes>("matchToMapUninitialised: use", use,
                      [&](const Bytes& v) { fe.matchToMapUninitialised(0, f1, v, previous, begin, pool, e0, r0, T1); });
  shortAndLong<Ints>("matchToMapUninitialised: previousLandmark", previous,
                     [&](const Ints& v) { fe.matchToMapUninitialised(0, f1, use, v, begin, pool, e0, r0, T1); });
  shortAndLong<Bytes>("matchToMapUninitialised: pool", pool,
                      [&](const Bytes& v) { fe.matchToMapUninitialised(0, f1, use, previous, begin, v, e0, r0, T1); });
  shortAndLong<Reals>("matchToMapUninitialised: e0_W", e0,
                      [&](const Reals& v) { fe.matchToMapUninitialised(0, f1, use, previous, begin, pool, v, r0, T1); });
  shortAndLong<Reals>("matchToMapUninitialised: r0_W", r0,
                      [&](const Reals& v) { fe.matchToMapUninitialised(0, f1, use, previous, begin, pool, e0, v, T1); });
  badFrames("matchToMapUninitialised: frame", f1, true,
            [&](const FrameData& f) { fe.matchToMapUninitialised(1, f, none, Ints(), begin, pool, e0, r0, T1); });

  mustThrow("verifyRecognisedPlace: camera = numCameras()", [&] { fe.verifyRecognisedPlace(bad, pool, begin, f1); });
  mustThrow("verifyRecognisedPlace: descBegin empty", [&] { fe.verifyRecognisedPlace(0, Bytes(), empty, f1); });
  shortAndLong<Bytes>("verifyRecognisedPlace: landmarkDescriptors", pool, [&](const Bytes& v) { fe.verifyRecognisedPlace(0, v, begin, f1); });
  badFrames("verifyRecognisedPlace: frame", f1, false, [&](const FrameData& f) { fe.verifyRecognisedPlace(0, pool, begin, f); });
}

#ifdef OKVFE_WITH_OKVIS
// ---- the hook route of HipViFrontend ---------------------------------------------------------------------------------
struct Rest : okvis::ViFrontendInterface {  // stands for okvis::Frontend
  int associations = 0;
  bool detectAndDescribe(size_t, std::shared_ptr<okvis::MultiFrame>, const okvis::kinematics::Transformation&,
                         const std::vector<cv::KeyPoint>*) override { return false; }
  bool dataAssociationAndInitialization(okvis::Estimator&, const okvis::ViParameters&, std::shared_ptr<okvis::MultiFrame>,
                                        bool* asKeyframe) override {
    ++associations;
    *asKeyframe = false;
    return true;
  }
  bool propagation(const okvis::ImuMeasurementDeque&, const okvis::ImuParameters&, okvis::kinematics::Transformation&,
                   okvis::SpeedAndBias&, const okvis::Time&, const okvis::Time&, Eigen::Matrix<double, 15, 15>*,
                   Eigen::Matrix<double, 15, 15>*) const override { return true; }
};
struct Hook : okvfe::AssociationHook {
  int calls = 0;
  HipFrontend* gpu = nullptr;
  okvis::ViFrontendInterface* reference = nullptr;
  bool dataAssociationAndInitialization(HipFrontend& g, okvis::ViFrontendInterface& r, okvis::Estimator&, const okvis::ViParameters&,
                                        std::shared_ptr<okvis::MultiFrame>, bool* asKeyframe) override {
    ++calls;
    gpu = &g;
    reference = &r;
    // what a maintainer plugs in: a matcher of the GPU front-end (camera 1 of the rig)
    const FrameData f = makeFrame(3, 77);
    const okvfe::HipFrontend::PlaceMatches p = g.verifyRecognisedPlace(1, bytes(2 * 48, 5), kBegins[1], f);
    *asKeyframe = p.kMin.size() == 1;
    return false;
  }
};

void hookRoute() {
  Rest* rest = new Rest();
  const std::vector<okvfe_camera_ext> cams{camera(0), camera(1)};
  const int first_ctx = Rig::created();
  okvfe::HipViFrontend vi(std::unique_ptr<okvis::ViFrontendInterface>(rest), cams, Rig::parameters());
  Rig::created() += 2;
  okvis::ViFrontendInterface& iface = vi;  // as okvis::ThreadedSlam holds it
  okvis::Estimator estimator;
  auto frames = std::make_shared<okvis::MultiFrame>(2);
  bool key = true;
  size_t before = fake::calls().size();
  expect(!vi.associationOnGpu(), "hook route: no hook, associationOnGpu() is false");
  expect(iface.dataAssociationAndInitialization(estimator, okvis::ViParameters(), frames, &key) && !key && rest->associations == 1,
         "hook route: without a hook the call reaches the wrapped front-end");
  expect(fake::calls().size() == before, "hook route: without a hook the library is not reached");
  auto hook = std::make_shared<Hook>();
  vi.setAssociationHook(hook);
  expect(vi.associationOnGpu(), "hook route: hook installed, associationOnGpu() is true");
  key = false;
  expect(!iface.dataAssociationAndInitialization(estimator, okvis::ViParameters(), frames, &key) && key,
         "hook route: the hook's return value and *asKeyframe come back");
  expect(hook->calls == 1 && rest->associations == 1, "hook route: the hook is called instead of the wrapped front-end");
  expect(hook->gpu == &vi.gpu() && hook->reference == rest, "hook route: the hook receives gpu() and the wrapped front-end");
  expect(fake::calls().size() == before + 1 && fake::calls().back().fn == "okvfe_verify_place_match" &&
             fake::calls().back().ctx == first_ctx + 1,
         "hook route: the hook's matcher call ran on camera 1's context of gpu()");
  vi.setAssociationHook(nullptr);
  key = true;
  expect(!vi.associationOnGpu(), "hook route: hook removed, associationOnGpu() is false");
  expect(iface.dataAssociationAndInitialization(estimator, okvis::ViParameters(), frames, &key) && !key && rest->associations == 2 &&
             hook->calls == 1,
         "hook route: setAssociationHook(nullptr) restores forwarding");
}
#endif

}  // namespace

int main() {
  try {
    wellFormed();
    illFormed();
#ifdef OKVFE_WITH_OKVIS
    hookRoute();
#endif
  } catch (const std::exception& e) {
    fail(std::string("unexpected exception: ") + e.what());
  }
  expect(fake::contexts_alive() == 0, "every context is destroyed with its front-end");
  std::printf("%zu library calls recorded, %d failures\n", fake::calls().size(), failures);
  return failures ? 1 : 0;
}
