// fake_okvfe.cpp -- a recording stand-in for libokvfe.so, CPU only: exactly the C functions that the methods of
// okvfe::HipFrontend / okvfe::HipViFrontend driven by tests/cpp/host_marshalling_main.cpp reference (`nm -C` on that
// program's object lists them), with the signatures of include/okvfe.h, so a drift of either fails the build.
//
// Every matcher entry point here
//  - reads every byte include/okvfe.h entitles the real function to read (a checksum per input array) and writes
//    every byte it may write (0xEE, then values made from the inputs by the rules below): a buffer handed over too
//    short is a heap-buffer-overflow under AddressSanitizer;
//  - appends one fake::Call: its name, the context's creation order, every scalar argument by name and a checksum per
//    input array by name, in the order of the C signature.
// This file is a translation unit of its own, linked to the program in place of libokvfe.so.  The program includes it
// with FAKE_OKVFE_DECLARATIONS_ONLY defined for the namespace fake alone: the record of a call, the checksum and the
// output rules.
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/okvfe.h"

namespace fake {

struct Call {
  std::string fn;
  int ctx = -1;
  std::vector<std::pair<std::string, double>> num;    // scalars (integers are exact in a double here)
  std::vector<std::pair<std::string, uint64_t>> buf;  // FNV-1a of every input array, all its bytes
  bool padded_null = false;  // a back-projection or hps_W array arrived as a null pointer
  bool operator==(const Call& o) const { return fn == o.fn && ctx == o.ctx && num == o.num && buf == o.buf; }
};
inline std::vector<Call>& calls() {
  static std::vector<Call> c;
  return c;
}
inline int& contexts_alive() {
  static int n = 0;
  return n;
}

inline uint64_t fnv(const void* p, size_t bytes) {
  uint64_t h = 1469598103934665603ull;
  const uint8_t* b = static_cast<const uint8_t*>(p);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}
template <typename T>
inline uint64_t fnv(const std::vector<T>& v) { return fnv(v.data(), v.size() * sizeof(T)); }

inline void add_pose(Call& c, const std::string& name, const okvfe_pose& T) {
  for (int i = 0; i < 9; ++i) c.num.emplace_back(name + ".C" + std::to_string(i), T.C[i]);
  for (int i = 0; i < 3; ++i) c.num.emplace_back(name + ".r" + std::to_string(i), T.r[i]);
}
inline void add_camera(Call& c, const okvfe_camera_ext& cam) {
  c.num.emplace_back("camera.width", cam.base.width);
  c.num.emplace_back("camera.height", cam.base.height);
  c.num.emplace_back("camera.fu", cam.base.fu);
  c.num.emplace_back("camera.fv", cam.base.fv);
  c.num.emplace_back("camera.cu", cam.base.cu);
  c.num.emplace_back("camera.cv", cam.base.cv);
  c.num.emplace_back("camera.distortion", cam.base.distortion);
  for (int i = 0; i < 4; ++i) c.num.emplace_back("camera.d" + std::to_string(i), cam.base.d[i]);
  for (int i = 0; i < 4; ++i) c.num.emplace_back("camera.d_ext" + std::to_string(i), cam.d_ext[i]);
}

// the output rules (the program restates them from its own inputs)
inline int32_t rule_landmark(const uint8_t* desc, const uint8_t* use, int k) { return use[k] ? int32_t(desc[48 * k]) : -1; }
inline int32_t rule_dist(int k) { return 1000 + k; }
inline double rule_hp(const double* backproj, int k, int i) { return backproj[3 * k + i % 3] + 0.25 * i; }
inline int32_t rule_kmin(const uint8_t* pool, const int32_t* begin, int l) {
  return begin[l + 1] > begin[l] ? int32_t(pool[48 * begin[l]]) : -7;
}
inline uint32_t rule_distmin(int l) { return 3000u + uint32_t(l); }
inline void rule_match_row(const uint8_t* desc0, const double* backproj0, int k, int32_t* k1, int32_t* dist, int32_t* ini,
                           double hp[4]) {
  *k1 = int32_t(desc0[48 * k]);
  *dist = 100 + k;
  *ini = k & 1;
  for (int i = 0; i < 4; ++i) hp[i] = rule_hp(backproj0, k, i);
}

}  // namespace fake

#ifndef FAKE_OKVFE_DECLARATIONS_ONLY
struct okvfe_ctx {
  okvfe_config cfg;
  int order;  // 0 = the first context created
  bool has_camera;
  std::string error;
};

namespace {
okvfe_status bad(okvfe_ctx* ctx, const char* what) {
  ctx->error = what;
  return OKVFE_ERR_INVALID_ARGUMENT;
}
fake::Call& record(okvfe_ctx* ctx, const char* fn) {
  fake::calls().emplace_back();
  fake::Call& c = fake::calls().back();
  c.fn = fn;
  c.ctx = ctx->order;
  return c;
}
void in(fake::Call& c, const char* name, const void* p, size_t bytes) { c.buf.emplace_back(name, fake::fnv(p, bytes)); }
}  // namespace

extern "C" {

okvfe_status okvfe_create(const okvfe_config* cfg, okvfe_ctx** out) {
  static int created = 0;
  if (!cfg || !out || cfg->abi_version != OKVFE_ABI_VERSION) return OKVFE_ERR_INVALID_ARGUMENT;
  *out = new okvfe_ctx{*cfg, created++, false, ""};
  ++fake::contexts_alive();
  return OKVFE_OK;
}
void okvfe_destroy(okvfe_ctx* ctx) {
  if (ctx) --fake::contexts_alive();
  delete ctx;
}
const char* okvfe_last_error(const okvfe_ctx* ctx) { return ctx ? ctx->error.c_str() : ""; }
okvfe_status okvfe_get_device_outputs(okvfe_ctx* ctx, okvfe_device_outputs* out) {
  if (!ctx || !out) return OKVFE_ERR_INVALID_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->max_keypoints = ctx->cfg.max_keypoints;
  return OKVFE_OK;
}
void okvfe_device_free(void*) {}  // (~HypothesisScratch; the program never allocates device memory)

okvfe_status okvfe_set_camera_ext(okvfe_ctx* ctx, int32_t cam, const okvfe_camera_ext* camera) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!camera || cam < 0 || cam >= ctx->cfg.num_cameras) return bad(ctx, "okvfe_set_camera_ext: bad argument");
  fake::Call& c = record(ctx, "okvfe_set_camera_ext");
  c.num.emplace_back("cam", cam);
  fake::add_camera(c, *camera);
  ctx->has_camera = true;
  return OKVFE_OK;
}

#ifdef OKVFE_WITH_OKVIS
// HipViFrontend::detectAndDescribe is a virtual, so its callee is referenced by the hook build; never called there
okvfe_status okvfe_detect_describe(okvfe_ctx* ctx, const uint8_t*, size_t, int32_t, const float*, okvfe_keypoint*, uint8_t*,
                                   double*, uint8_t*, int32_t, int32_t*) {
  return ctx ? bad(ctx, "okvfe_detect_describe: not part of this stand-in") : OKVFE_ERR_INVALID_ARGUMENT;
}
#endif

okvfe_status okvfe_match_stereo(okvfe_ctx* ctx, const uint8_t* desc0, const okvfe_keypoint* kp0, const double* backproj0,
                                const uint8_t* valid0, int32_t n0, const uint8_t* desc1, const okvfe_keypoint* kp1,
                                const double* backproj1, const uint8_t* valid1, int32_t n1, const okvfe_pose* T_WC0,
                                const okvfe_pose* T_WC1, double f0, double f1, okvfe_stereo_match* matches) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n0 < 0 || n1 < 0 || !T_WC0 || !T_WC1 || !(f0 > 0.0) || !(f1 > 0.0) ||
      (n0 > 0 && (!desc0 || !kp0 || !backproj0 || !valid0 || !matches)) || (n1 > 0 && (!desc1 || !kp1 || !backproj1 || !valid1)))
    return bad(ctx, "okvfe_match_stereo: bad argument");
  fake::Call& c = record(ctx, "okvfe_match_stereo");
  const size_t a = size_t(n0), b = size_t(n1);
  in(c, "desc0", desc0, a * 48); in(c, "kp0", kp0, a * sizeof(okvfe_keypoint)); in(c, "backproj0", backproj0, a * 24);
  in(c, "valid0", valid0, a);
  c.num.emplace_back("n0", n0);
  in(c, "desc1", desc1, b * 48); in(c, "kp1", kp1, b * sizeof(okvfe_keypoint)); in(c, "backproj1", backproj1, b * 24);
  in(c, "valid1", valid1, b);
  c.num.emplace_back("n1", n1);
  fake::add_pose(c, "T_WC0", *T_WC0);
  fake::add_pose(c, "T_WC1", *T_WC1);
  c.num.emplace_back("f0", f0);
  c.num.emplace_back("f1", f1);
  c.padded_null = !backproj0 || !backproj1;
  if (n0) std::memset(static_cast<void*>(matches), 0xEE, a * sizeof(okvfe_stereo_match));
  for (int k = 0; k < n0; ++k) {
    okvfe_stereo_match& m = matches[k];
    m.pad = 0;
    fake::rule_match_row(desc0, backproj0, k, &m.k1, &m.dist, &m.initialisable, m.hp_W);
  }
  return OKVFE_OK;
}

okvfe_status okvfe_match_motion_stereo_ext(okvfe_ctx* ctx, const okvfe_camera_ext* camera, const uint8_t* desc0,
                                           const okvfe_keypoint* kp0, const double* backproj0, const uint8_t* valid0,
                                           const uint8_t* skip0, int32_t n0, const uint8_t* desc1, const okvfe_keypoint* kp1,
                                           const double* backproj1, const uint8_t* valid1, const uint8_t* matched1,
                                           int32_t n1, const okvfe_pose* T_WC0, const okvfe_pose* T_WC1,
                                           okvfe_motion_match* matches) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!camera || n0 < 0 || n1 < 0 || !T_WC0 || !T_WC1 || (n0 > 0 && (!desc0 || !kp0 || !backproj0 || !valid0 || !matches)) ||
      (n1 > 0 && (!desc1 || !kp1 || !backproj1 || !valid1)))
    return bad(ctx, "okvfe_match_motion_stereo: bad argument");
  fake::Call& c = record(ctx, "okvfe_match_motion_stereo_ext");
  const size_t a = size_t(n0), b = size_t(n1);
  fake::add_camera(c, *camera);
  in(c, "desc0", desc0, a * 48); in(c, "kp0", kp0, a * sizeof(okvfe_keypoint)); in(c, "backproj0", backproj0, a * 24);
  in(c, "valid0", valid0, a);
  c.num.emplace_back("skip0 given", skip0 != nullptr);
  in(c, "skip0", skip0, skip0 ? a : 0);
  c.num.emplace_back("n0", n0);
  in(c, "desc1", desc1, b * 48); in(c, "kp1", kp1, b * sizeof(okvfe_keypoint)); in(c, "backproj1", backproj1, b * 24);
  in(c, "valid1", valid1, b);
  c.num.emplace_back("matched1 given", matched1 != nullptr);
  in(c, "matched1", matched1, matched1 ? b : 0);
  c.num.emplace_back("n1", n1);
  fake::add_pose(c, "T_WC0", *T_WC0);
  fake::add_pose(c, "T_WC1", *T_WC1);
  c.padded_null = !backproj0 || !backproj1;
  if (n0) std::memset(static_cast<void*>(matches), 0xEE, a * sizeof(okvfe_motion_match));
  for (int k = 0; k < n0; ++k) {
    okvfe_motion_match& m = matches[k];
    fake::rule_match_row(desc0, backproj0, k, &m.k1, &m.dist, &m.initialisable, m.hp_W);
    m.accepted = (k & 2) >> 1;
    m.cos_quality = 0.5 + 0.001 * k;
  }
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map(okvfe_ctx* ctx, const uint8_t* desc, const okvfe_keypoint* kps, const uint8_t* use,
                                int32_t n_kps, const double* projections_l2, const int32_t* desc_begin, int32_t n_landmarks,
                                const uint8_t* pool, double reprojection_threshold, int32_t* best_landmark,
                                int32_t* best_dist) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_kps < 0 || n_landmarks < 0 || !desc_begin || !(reprojection_threshold >= 0.0) ||
      (n_kps > 0 && (!desc || !kps || !use || !best_landmark || !best_dist)) || (n_landmarks > 0 && (!projections_l2 || !pool)))
    return bad(ctx, "okvfe_match_to_map: bad argument");
  fake::Call& c = record(ctx, "okvfe_match_to_map");
  const size_t n = size_t(n_kps), nl = size_t(n_landmarks);
  in(c, "desc", desc, n * 48); in(c, "kps", kps, n * sizeof(okvfe_keypoint)); in(c, "use", use, n);
  c.num.emplace_back("n_kps", n_kps);
  in(c, "projections", projections_l2, nl * 16);
  in(c, "desc_begin", desc_begin, (nl + 1) * 4);
  c.num.emplace_back("n_landmarks", n_landmarks);
  in(c, "pool", pool, size_t(desc_begin[nl]) * 48);
  c.num.emplace_back("reprojection_threshold", reprojection_threshold);
  for (int k = 0; k < n_kps; ++k) {
    best_landmark[k] = fake::rule_landmark(desc, use, k);
    best_dist[k] = fake::rule_dist(k);
  }
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_landmarks(okvfe_ctx* ctx, int32_t cam, const okvfe_landmark_table* T, const okvfe_pose* T_WC1,
                                          double reprojection_threshold, int32_t exclusive, const uint8_t* desc,
                                          const okvfe_keypoint* kps, const uint8_t* use, int32_t n_kps,
                                          okvfe_landmark_pool* pool_out, int32_t* best_landmark, int32_t* best_dist) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (!T || !T_WC1 || n_kps < 0 || !(reprojection_threshold >= 0.0) || T->n_landmarks < 0 || T->n_observations < 0 ||
      T->n_poses < 0 || !T->obs_begin || (n_kps > 0 && (!desc || !kps || !use || !best_landmark || !best_dist)) ||
      (T->n_landmarks > 0 && (!T->hp_W || !T->quality)) ||
      (T->n_observations > 0 && (!T->obs_pose || !T->obs_desc || !T->obs_backproj || !T->poses)))
    return bad(ctx, "okvfe_match_to_map_landmarks: bad argument");
  if (cam < 0 || cam >= ctx->cfg.num_cameras || !ctx->has_camera) {
    ctx->error = "okvfe_match_to_map_landmarks: camera slot has no intrinsics";
    return OKVFE_ERR_NOT_READY;
  }
  fake::Call& c = record(ctx, "okvfe_match_to_map_landmarks");
  const size_t n = size_t(n_kps), nl = size_t(T->n_landmarks), no = size_t(T->n_observations), np = size_t(T->n_poses);
  c.num.emplace_back("cam", cam);
  c.num.emplace_back("n_landmarks", T->n_landmarks);
  c.num.emplace_back("n_observations", T->n_observations);
  c.num.emplace_back("n_poses", T->n_poses);
  in(c, "hp_W", T->hp_W, nl * 32); in(c, "quality", T->quality, nl * 8); in(c, "obs_begin", T->obs_begin, (nl + 1) * 4);
  in(c, "obs_pose", T->obs_pose, no * 4); in(c, "obs_desc", T->obs_desc, no * 48);
  in(c, "obs_backproj", T->obs_backproj, no * 24); in(c, "poses", T->poses, np * sizeof(okvfe_pose));
  fake::add_pose(c, "T_WC1", *T_WC1);
  c.num.emplace_back("reprojection_threshold", reprojection_threshold);
  c.num.emplace_back("exclusive", exclusive);
  in(c, "desc", desc, n * 48); in(c, "kps", kps, n * sizeof(okvfe_keypoint)); in(c, "use", use, n);
  c.num.emplace_back("n_kps", n_kps);
  c.num.emplace_back("pool_out given", pool_out != nullptr);
  if (pool_out && nl) {
    if (pool_out->status) for (size_t l = 0; l < nl; ++l) pool_out->status[l] = int32_t(l % 3);
    if (pool_out->n_desc) std::memset(pool_out->n_desc, 0xEE, nl * 4);
    if (pool_out->obs_rows) std::memset(pool_out->obs_rows, 0xEE, nl * 12);
    if (pool_out->projection) std::memset(static_cast<void*>(pool_out->projection), 0xEE, nl * 16);
    if (pool_out->e_W) std::memset(static_cast<void*>(pool_out->e_W), 0xEE, nl * 48);
    if (pool_out->r_W) std::memset(static_cast<void*>(pool_out->r_W), 0xEE, nl * 48);
  }
  for (int k = 0; k < n_kps; ++k) {
    best_landmark[k] = fake::rule_landmark(desc, use, k);
    best_dist[k] = fake::rule_dist(k);
  }
  return OKVFE_OK;
}

okvfe_status okvfe_match_to_map_uninitialised(okvfe_ctx* ctx, const uint8_t* desc, const double* backproj, const uint8_t* use,
                                              const int32_t* previous_landmark, int32_t n_kps, const int32_t* desc_begin,
                                              int32_t n_landmarks, const uint8_t* pool, const double* e0_W,
                                              const double* r0_W, const okvfe_pose* T_WC1, double focal_length,
                                              int32_t* best_landmark, int32_t* best_dist, double* hps_W, uint8_t* hp_set,
                                              int32_t* already_matched) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_kps < 0 || n_landmarks < 0 || !desc_begin || !T_WC1 || !(focal_length > 0.0) || !already_matched ||
      (n_kps > 0 && (!desc || !backproj || !use || !previous_landmark || !best_landmark || !best_dist || !hps_W || !hp_set)))
    return bad(ctx, "okvfe_match_to_map_uninitialised: bad argument");
  const size_t n = size_t(n_kps), nl = size_t(n_landmarks), rows = size_t(desc_begin[nl]);
  if (rows > 0 && (!pool || !e0_W || !r0_W)) return bad(ctx, "okvfe_match_to_map_uninitialised: null pool");
  fake::Call& c = record(ctx, "okvfe_match_to_map_uninitialised");
  in(c, "desc", desc, n * 48); in(c, "backproj", backproj, n * 24); in(c, "use", use, n);
  in(c, "previous_landmark", previous_landmark, n * 4);
  c.num.emplace_back("n_kps", n_kps);
  in(c, "desc_begin", desc_begin, (nl + 1) * 4);
  c.num.emplace_back("n_landmarks", n_landmarks);
  in(c, "pool", pool, rows * 48); in(c, "e0_W", e0_W, rows * 24); in(c, "r0_W", r0_W, rows * 24);
  fake::add_pose(c, "T_WC1", *T_WC1);
  c.num.emplace_back("focal_length", focal_length);
  c.padded_null = !backproj || !hps_W;
  *already_matched = 0;
  if (n) std::memset(static_cast<void*>(hps_W), 0xEE, n * 32);
  for (int k = 0; k < n_kps; ++k) {
    best_landmark[k] = fake::rule_landmark(desc, use, k);
    best_dist[k] = fake::rule_dist(k);
    for (int i = 0; i < 4; ++i) hps_W[4 * k + i] = fake::rule_hp(backproj, k, i);
    hp_set[k] = use[k] ? 1 : 0;
    *already_matched += previous_landmark[k] >= 0 ? 1 : 0;
  }
  return OKVFE_OK;
}

okvfe_status okvfe_verify_place_match(okvfe_ctx* ctx, const uint8_t* landmark_desc, const int32_t* desc_begin,
                                      int32_t n_landmarks, const uint8_t* frame_desc, int32_t n_kps, int32_t* k_min,
                                      uint32_t* dist_min) {
  if (!ctx) return OKVFE_ERR_INVALID_ARGUMENT;
  if (n_landmarks < 0 || n_kps < 0 || !desc_begin || (n_landmarks > 0 && (!k_min || !dist_min)) || (n_kps > 0 && !frame_desc))
    return bad(ctx, "okvfe_verify_place_match: bad argument");
  const size_t nl = size_t(n_landmarks), rows = size_t(desc_begin[nl]);
  if (rows > 0 && !landmark_desc) return bad(ctx, "okvfe_verify_place_match: null pool");
  fake::Call& c = record(ctx, "okvfe_verify_place_match");
  in(c, "landmark_desc", landmark_desc, rows * 48);
  in(c, "desc_begin", desc_begin, (nl + 1) * 4);
  c.num.emplace_back("n_landmarks", n_landmarks);
  in(c, "frame_desc", frame_desc, size_t(n_kps) * 48);
  c.num.emplace_back("n_kps", n_kps);
  for (int l = 0; l < n_landmarks; ++l) {
    k_min[l] = fake::rule_kmin(landmark_desc, desc_begin, l);
    dist_min[l] = fake::rule_distmin(l);
  }
  return OKVFE_OK;
}

}  // extern "C"
#endif  // FAKE_OKVFE_DECLARATIONS_ONLY
