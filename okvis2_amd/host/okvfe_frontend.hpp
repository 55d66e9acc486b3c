// okvfe_frontend.hpp -- C++ host mirror of the reference's front-end interfaces over the C ABI.
//
// Dependency-free (no OpenCV / Eigen): the types are layout-compatible stand-ins, so the classes
// keep the reference's names, argument meaning and error behaviour and can be dropped behind
//   cv::FeatureDetector::detect / cv::DescriptorExtractor::compute
//     (okvis_cv/include/okvis/implementation/Frame.hpp:152,167)
//   brisk::BriskDescriptorExtractor::isCameraAware / setCameraProperties / setExtractionDirection
//     (okvis_frontend/src/Frontend.cpp:232-251)
//   okvis::Frontend::detectAndDescribe            (okvis_frontend/src/Frontend.cpp:221-269)
//   okvis::Frontend::matchStereo inner loops      (okvis_frontend/src/Frontend.cpp:2016-2076)
//   okvis::Frontend::doWeNeedANewKeyframe         (okvis_frontend/src/Frontend.cpp:1058-1167)
//   okvis::ViSlamBackend::overlapFraction / trackingQuality (okvis_ceres/src/ViSlamBackend.cpp:2341-2427, :157-196)
//   the order of the motion-stereo sweep          (okvis_frontend/src/Frontend.cpp:1751-1767)
// okvfe_opencv_adapters.hpp wraps these in the real cv:: base classes when OpenCV is available.
//
// Every call goes to libokvfe.so (HIP kernels).  Failures throw okvfe::Exception, the analogue of
// okvis::Frontend::Exception (okvis_util/include/okvis/assert_macros.hpp:49-113).
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/okvfe.h"

namespace okvfe {

// okvfe_camera (distortion types 0..2) as the extended camera of ABI 8 (d_ext = 0)
inline okvfe_camera_ext extendCamera(const okvfe_camera& c) {
  okvfe_camera_ext e{};
  e.base = c;
  return e;
}
inline std::vector<okvfe_camera_ext> extendCameras(const std::vector<okvfe_camera>& cameras) {
  std::vector<okvfe_camera_ext> out;
  out.reserve(cameras.size());
  for (const okvfe_camera& c : cameras) out.push_back(extendCamera(c));
  return out;
}

class Exception : public std::runtime_error {
 public:
  Exception(okvfe_status st, const std::string& what)
      : std::runtime_error("okvfe status " + std::to_string(int(st)) + ": " + what), status(st) {}
  okvfe_status status;
};

struct ImageView {  // cv::Mat CV_8UC1 view
  const uint8_t* data;
  int width, height;
  size_t stride;
};

using KeyPoint = okvfe_keypoint;  // cv::KeyPoint layout
struct Descriptors {              // cv::Mat CV_8UC1, N x 48
  std::vector<uint8_t> data;
  int rows = 0;
  static constexpr int cols = OKVFE_DESC_BYTES;
  const uint8_t* row(int k) const { return data.data() + size_t(k) * cols; }
};

// shared handle: detector and extractor of one camera share one context (one HIP stream)
class Context {
 public:
  explicit Context(const okvfe_config& cfg) {
    okvfe_ctx* c = nullptr;
    const okvfe_status st = okvfe_create(&cfg, &c);
    if (st != OKVFE_OK) throw Exception(st, okvfe_last_error(nullptr));
    ctx_ = c;
    // row capacity per image: with a scale space (octaves > 0) every layer may deliver max_keypoints
    okvfe_device_outputs o{};
    max_keypoints_ = okvfe_get_device_outputs(c, &o) == OKVFE_OK ? o.max_keypoints : cfg.max_keypoints;
  }
  ~Context() { okvfe_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  okvfe_ctx* get() const { return ctx_; }
  int maxKeypoints() const { return max_keypoints_; }
  void check(okvfe_status st) const {
    if (st != OKVFE_OK) throw Exception(st, okvfe_last_error(ctx_));
  }
  // The extractor that shares this context announces what its next compute() will ask for
  // (Frontend.cpp:246-251 sets the direction BEFORE Frame::detect / Frame::describe): the detector
  // then runs okvfe_detect_ahead, and the compute() that follows on the same image costs no GPU work.
  // ONE pairing per context: a second extractor on another camera slot of the same context would overwrite
  // these fields behind the first one's back (the detector cannot know which camera an image belongs to), so
  // it switches the pairing off for good -- both extractors then compute on their own, correct but unpaired.
  // (One context per camera is the intended set-up: ThreadedSlam.cpp:434-448 runs a thread per camera.)
  struct NextExtraction {
    bool paired = false;  // an extractor is attached and wants pairing
    bool conflict = false;  // extractors of different camera slots share this context: never pair
    int cam = -1;
    bool aware = false;
    std::array<float, 3> dir{{0.0f, 1.0f, 0.0f}};
  };
  NextExtraction& nextExtraction() { return next_; }

 private:
  okvfe_ctx* ctx_ = nullptr;
  int max_keypoints_ = 0;
  NextExtraction next_;
};

// = brisk::ScaleSpaceFeatureDetector<brisk::HarrisScoreCalculator>(uniformityRadius, octaves,
//   absoluteThreshold, maxNumKpt) as a cv::FeatureDetector (Frontend.cpp:2406-2409)
class HipBriskDetector {
 public:
  explicit HipBriskDetector(std::shared_ptr<Context> ctx) : ctx_(std::move(ctx)) {}
  void detect(const ImageView& image, std::vector<KeyPoint>& keypoints) const {
    keypoints.resize(size_t(ctx_->maxKeypoints()));
    int32_t n = 0;
    const Context::NextExtraction& nx = ctx_->nextExtraction();
    if (nx.paired)
      ctx_->check(okvfe_detect_ahead(ctx_->get(), image.data, image.stride, nx.aware ? nx.cam : -1,
                                     nx.aware ? nx.dir.data() : nullptr, keypoints.data(), int32_t(keypoints.size()), &n));
    else
      ctx_->check(okvfe_detect(ctx_->get(), image.data, image.stride, keypoints.data(),
                               int32_t(keypoints.size()), &n));
    keypoints.resize(size_t(n));
  }

 private:
  std::shared_ptr<Context> ctx_;
};

// = brisk::BriskDescriptorExtractor(rotationInvariant, scaleInvariant) as a
//   cv::DescriptorExtractor with the camera-aware extras (Frontend.cpp:2410-2412, 232-251)
class HipBriskExtractor {
 public:
  // pairWithDetector: a HipBriskDetector on the same context answers this extractor's compute()
  // ahead of time when both see the same image (okvfe_detect_ahead)
  HipBriskExtractor(std::shared_ptr<Context> ctx, int cameraSlot, bool pairWithDetector = true)
      : ctx_(std::move(ctx)), cam_(cameraSlot) {
    Context::NextExtraction& nx = ctx_->nextExtraction();
    if (nx.paired && nx.cam != cam_) nx.conflict = true;
    nx.paired = pairWithDetector && !nx.conflict;
    if (nx.paired) nx.cam = cam_;
  }
  bool isCameraAware() const { return aware_; }
  // rays: H*W*3 f32, imageJacobians: H*W*6 f32 (PinholeCamera.hpp:180-208)
  void setCameraProperties(const float* rays, const float* imageJacobians, float fu) {
    ctx_->check(okvfe_set_camera_maps(ctx_->get(), cam_, rays, imageJacobians, fu));
    aware_ = true;
    if (ctx_->nextExtraction().cam == cam_) ctx_->nextExtraction().aware = true;
  }
  // full intrinsics: also enables back-projection of the kept keypoints on the GPU
  void setCamera(const okvfe_camera& camera) {
    ctx_->check(okvfe_set_camera(ctx_->get(), cam_, &camera));
    aware_ = true;
    if (ctx_->nextExtraction().cam == cam_) ctx_->nextExtraction().aware = true;
  }
  // every distortion type, OKVFE_DIST_RADTAN8 (PinholeCamera<RadialTangentialDistortion8>) included
  void setCamera(const okvfe_camera_ext& camera) {
    ctx_->check(okvfe_set_camera_ext(ctx_->get(), cam_, &camera));
    aware_ = true;
    if (ctx_->nextExtraction().cam == cam_) ctx_->nextExtraction().aware = true;
  }
  void setExtractionDirection(const std::array<float, 3>& dir) {
    dir_ = dir;
    if (ctx_->nextExtraction().cam == cam_) ctx_->nextExtraction().dir = dir;
  }
  // keypoints in/out: keypoints too close to the rim are removed (Frame.hpp:146)
  void compute(const ImageView& image, std::vector<KeyPoint>& keypoints, Descriptors& descriptors,
               std::vector<std::array<double, 3>>* backProjections = nullptr,
               std::vector<uint8_t>* backProjectionsValid = nullptr) const {
    const int32_t n_in = int32_t(keypoints.size());
    descriptors.data.assign(size_t(std::max(n_in, 1)) * OKVFE_DESC_BYTES, 0);
    std::vector<double> bp(size_t(std::max(n_in, 1)) * 3);
    std::vector<uint8_t> bv(size_t(std::max(n_in, 1)));
    if (keypoints.empty()) keypoints.resize(1);
    int32_t n = 0;
    ctx_->check(okvfe_compute(ctx_->get(), image.data, image.stride, aware_ ? cam_ : -1,
                              aware_ ? dir_.data() : nullptr, keypoints.data(), n_in,
                              descriptors.data.data(), bp.data(), bv.data(), &n));
    keypoints.resize(size_t(n));
    descriptors.rows = n;
    descriptors.data.resize(size_t(n) * OKVFE_DESC_BYTES);
    if (backProjections) {
      backProjections->resize(size_t(n));
      for (int k = 0; k < n; ++k) (*backProjections)[size_t(k)] = {bp[3 * k], bp[3 * k + 1], bp[3 * k + 2]};
    }
    if (backProjectionsValid) backProjectionsValid->assign(bv.begin(), bv.begin() + n);
  }

 private:
  std::shared_ptr<Context> ctx_;
  int cam_;
  bool aware_ = false;
  std::array<float, 3> dir_{{0.0f, 1.0f, 0.0f}};
};

// per-camera slice of okvis::MultiFrame that the front-end fills (okvis_cv/include/okvis/Frame.hpp:248-264)
struct FrameData {
  std::vector<KeyPoint> keypoints;
  Descriptors descriptors;
  std::vector<uint64_t> landmarkIds;  // zero-filled (Frame.hpp:170-173)
  std::vector<std::array<double, 3>> backProjections;
  std::vector<uint8_t> backProjectionsValid;
};

struct FrontendParameters {  // okvis_common/include/okvis/Parameters.hpp:123-133; Frontend.cpp:138-145
  float detection_threshold = 40.0f;  // uniformity radius in px
  int absolute_threshold = 200;
  int matching_threshold = 60;
  int octaves = 0;
  int max_num_keypoints = 450;
  bool rotation_invariance = true;
  bool scale_invariance = false;
  float box_scale = 1.0f;  // okvfe_config.box_scale: smoothing width of the built-in pattern (not a reference parameter)
};

// = the detect/describe/matchStereo part of okvis::Frontend (one GPU, all cameras of one rig)
class HipFrontend {
 public:
  HipFrontend(const std::vector<okvfe_camera>& cameras, const FrontendParameters& p, int device = 0)
      : HipFrontend(extendCameras(cameras), p, device) {}
  HipFrontend(const std::vector<okvfe_camera_ext>& cameras, const FrontendParameters& p, int device = 0)
      : cameras_(cameras), mutexes_(cameras.size()), bp_scratch_(cameras.size()), hyp_scratch_(cameras.size()),
        params_(p), device_(device) {
    if (cameras.empty()) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "no cameras");
    for (size_t i = 0; i < cameras.size(); ++i) {
      okvfe_config cfg{};
      cfg.abi_version = OKVFE_ABI_VERSION;
      cfg.device = device;
      cfg.width = cameras[i].base.width;
      cfg.height = cameras[i].base.height;
      cfg.max_batch = 1;
      cfg.num_cameras = 1;
      cfg.uniformity_radius = p.detection_threshold;
      cfg.octaves = p.octaves;
      cfg.absolute_threshold = p.absolute_threshold;
      cfg.max_keypoints = p.max_num_keypoints;
      cfg.rotation_invariant = p.rotation_invariance;
      cfg.scale_invariant = p.scale_invariance;
      cfg.match_threshold = p.matching_threshold;
      cfg.box_scale = p.box_scale;
      auto ctx = std::make_shared<Context>(cfg);
      contexts_.push_back(ctx);
      detectors_.emplace_back(ctx);
      extractors_.emplace_back(ctx, 0);
    }
  }
  size_t numCameras() const { return cameras_.size(); }

  // Frontend::detectAndDescribe(cameraIndex, frameOut, T_WC): thread-safe per camera.
  bool detectAndDescribe(size_t cameraIndex, const ImageView& image, const okvfe_pose& T_WC,
                         FrameData& frameOut) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    HipBriskExtractor& ex = extractors_[cameraIndex];
    if (!ex.isCameraAware()) ex.setCamera(cameras_[cameraIndex]);  // Frontend.cpp:232-244
    // extraction direction = gravity in the camera frame: T_WC.inverse().C() * (0,0,-1)
    std::array<float, 3> dir;
    for (int i = 0; i < 3; ++i) dir[size_t(i)] = float(-T_WC.C[6 + i]);  // C^T * (0,0,-1)
    ex.setExtractionDirection(dir);
    // Frame::detect + Frame::describe + computeBackProjections (Frontend.cpp:257-266) as ONE call:
    // one image upload, one kernel chain, one synchronisation
    Context& c = *contexts_[cameraIndex];
    const int cap = c.maxKeypoints();
    frameOut.keypoints.resize(size_t(cap));
    frameOut.descriptors.data.resize(size_t(cap) * OKVFE_DESC_BYTES);
    bp_scratch_[cameraIndex].resize(size_t(cap) * 3);
    frameOut.backProjectionsValid.resize(size_t(cap));
    int32_t n = 0;
    c.check(okvfe_detect_describe(c.get(), image.data, image.stride, 0, dir.data(), frameOut.keypoints.data(),
                                  frameOut.descriptors.data.data(), bp_scratch_[cameraIndex].data(),
                                  frameOut.backProjectionsValid.data(), cap, &n));
    frameOut.keypoints.resize(size_t(n));
    frameOut.descriptors.rows = n;
    frameOut.descriptors.data.resize(size_t(n) * OKVFE_DESC_BYTES);
    frameOut.backProjectionsValid.resize(size_t(n));
    frameOut.backProjections.resize(size_t(n));
    const double* bp = bp_scratch_[cameraIndex].data();
    for (int k = 0; k < n; ++k) frameOut.backProjections[size_t(k)] = {bp[3 * k], bp[3 * k + 1], bp[3 * k + 2]};
    frameOut.landmarkIds.assign(size_t(n), 0);
    return true;
  }

  // the k0 x k1 loop of Frontend::matchStereo for one camera pair (Frontend.cpp:2016-2076)
  std::vector<okvfe_stereo_match> matchStereo(size_t im0, const FrameData& f0, const okvfe_pose& T_WC0,
                                              size_t im1, const FrameData& f1, const okvfe_pose& T_WC1) {
    checkCamera(im0);
    checkCamera(im1);
    checkFrame(f0, kDescriptors | kBackProjections, "matchStereo: f0");
    checkFrame(f1, kDescriptors | kBackProjections, "matchStereo: f1");
    std::lock_guard<std::mutex> lock(mutexes_[im0]);
    std::vector<okvfe_stereo_match> out(f0.keypoints.size());
    const double fa = 0.5 * (cameras_[im0].base.fu + cameras_[im0].base.fv);
    const double fb = 0.5 * (cameras_[im1].base.fu + cameras_[im1].base.fv);
    std::vector<double> b0(f0.backProjections.size() * 3 + 3), b1(f1.backProjections.size() * 3 + 3);
    for (size_t k = 0; k < f0.backProjections.size(); ++k)
      for (int i = 0; i < 3; ++i) b0[3 * k + size_t(i)] = f0.backProjections[k][size_t(i)];
    for (size_t k = 0; k < f1.backProjections.size(); ++k)
      for (int i = 0; i < 3; ++i) b1[3 * k + size_t(i)] = f1.backProjections[k][size_t(i)];
    contexts_[im0]->check(okvfe_match_stereo(
        contexts_[im0]->get(), f0.descriptors.data.data(), f0.keypoints.data(), b0.data(),
        f0.backProjectionsValid.data(), int32_t(f0.keypoints.size()), f1.descriptors.data.data(),
        f1.keypoints.data(), b1.data(), f1.backProjectionsValid.data(), int32_t(f1.keypoints.size()),
        &T_WC0, &T_WC1, fa, fb, out.data()));
    return out;
  }

  // the k0 x k1 loops of Frontend::matchMotionStereo for one camera: older frame f0 against the
  // current frame f1 (Frontend.cpp:1789-1905).  skip0[k0] != 0: k0 is left out (:1814-1841);
  // matched1[k1] != 0: the current keypoint already carries a landmark (:1795-1798); either may be
  // empty.  quality of a row = acos(cos_quality) (:1887-1889).
  std::vector<okvfe_motion_match> matchMotionStereo(size_t cameraIndex, const FrameData& f0,
                                                    const okvfe_pose& T_WC0, const FrameData& f1,
                                                    const okvfe_pose& T_WC1,
                                                    const std::vector<uint8_t>& skip0 = {},
                                                    const std::vector<uint8_t>& matched1 = {}) {
    checkCamera(cameraIndex);
    checkFrame(f0, kDescriptors | kBackProjections, "matchMotionStereo: f0");
    checkFrame(f1, kDescriptors | kBackProjections, "matchMotionStereo: f1");
    checkPerKeypoint(skip0.size(), f0, "matchMotionStereo: skip0");
    checkPerKeypoint(matched1.size(), f1, "matchMotionStereo: matched1");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    std::vector<okvfe_motion_match> out(f0.keypoints.size());
    const std::vector<double> b0 = flat(f0.backProjections), b1 = flat(f1.backProjections);
    contexts_[cameraIndex]->check(okvfe_match_motion_stereo_ext(
        contexts_[cameraIndex]->get(), &cameras_[cameraIndex], f0.descriptors.data.data(), f0.keypoints.data(),
        b0.data(), f0.backProjectionsValid.data(), skip0.empty() ? nullptr : skip0.data(),
        int32_t(f0.keypoints.size()), f1.descriptors.data.data(), f1.keypoints.data(), b1.data(),
        f1.backProjectionsValid.data(), matched1.empty() ? nullptr : matched1.data(),
        int32_t(f1.keypoints.size()), &T_WC0, &T_WC1, out.data()));
    return out;
  }

  struct MapMatches {  // per keypoint of the frame: landmark index (-1 = none) and distance
    std::vector<int32_t> landmark, distance;
  };
  // Frontend::matchToMap up to and including its first matcher pass (Frontend.cpp:1219-1411): the
  // landmark table is projected, pooled and matched on the GPU.  use[k] == 0 skips keypoint k.
  MapMatches matchToMap(size_t cameraIndex, const FrameData& frame, const okvfe_landmark_table& table,
                        const okvfe_pose& T_WC1, double reprojectionThreshold, bool exclusive,
                        const std::vector<uint8_t>& use = {}, okvfe_landmark_pool* poolOut = nullptr) {
    checkCamera(cameraIndex);
    checkFrame(frame, kDescriptors, "matchToMap: frame");
    checkPerKeypoint(use.size(), frame, "matchToMap: use");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    const size_t n = frame.keypoints.size();
    MapMatches m{std::vector<int32_t>(n, -1), std::vector<int32_t>(n, 0)};
    const std::vector<uint8_t> all(n, 1);
    contexts_[cameraIndex]->check(okvfe_match_to_map_landmarks(
        contexts_[cameraIndex]->get(), 0, &table, &T_WC1, reprojectionThreshold, exclusive ? 1 : 0,
        frame.descriptors.data.data(), frame.keypoints.data(), use.empty() ? all.data() : use.data(), int32_t(n),
        poolOut, m.landmark.data(), m.distance.data()));
    return m;
  }
  // A landmark table in device memory: uploaded when the map changes (at keyframes), read by every matchToMapBlocks
  // until the next upload.  Owns its device copies (okvfe_device_alloc / okvfe_copy_to_device / okvfe_device_free).
  class DeviceLandmarkTable {
   public:
    DeviceLandmarkTable() = default;
    DeviceLandmarkTable(const DeviceLandmarkTable&) = delete;
    DeviceLandmarkTable& operator=(const DeviceLandmarkTable&) = delete;
    ~DeviceLandmarkTable() {
      for (void* p : allocs_) okvfe_device_free(p);
    }
    const okvfe_landmark_table_device& get() const { return view_; }

   private:
    friend class HipFrontend;
    okvfe_landmark_table_device view_{};
    std::vector<void*> allocs_;
  };
  // Copies `table` to the device of camera `cameraIndex`'s context and runs okvfe_landmark_table_check_device on the
  // copy: throws (OKVFE_ERR_INVALID_ARGUMENT, the first offending row named) if the table is malformed.  Synchronises;
  // meant to run once per map change.
  std::shared_ptr<DeviceLandmarkTable> uploadLandmarkTable(size_t cameraIndex, const okvfe_landmark_table& table) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (table.n_landmarks < 0 || table.n_observations < 0 || table.n_poses < 0 || !table.obs_begin)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "uploadLandmarkTable: bad table");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    auto out = std::make_shared<DeviceLandmarkTable>();
    auto up = [&](const void* src, size_t bytes) -> const void* {
      void* d = nullptr;
      c.check(okvfe_device_alloc(device_, bytes ? bytes : 1, &d));
      out->allocs_.push_back(d);
      if (bytes) {
        if (!src) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "uploadLandmarkTable: null array");
        c.check(okvfe_copy_to_device(d, src, bytes, nullptr));
      }
      return d;
    };
    const size_t nl = size_t(table.n_landmarks), no = size_t(table.n_observations), np = size_t(table.n_poses);
    okvfe_landmark_table_device& v = out->view_;
    v.n_landmarks = table.n_landmarks;
    v.n_observations = table.n_observations;
    v.n_poses = table.n_poses;
    v.hp_W = static_cast<const double*>(up(table.hp_W, nl * 32));
    v.quality = static_cast<const double*>(up(table.quality, nl * 8));
    v.obs_begin = static_cast<const int32_t*>(up(table.obs_begin, (nl + 1) * 4));
    v.obs_pose = static_cast<const int32_t*>(up(table.obs_pose, no * 4));
    v.obs_desc = static_cast<const uint8_t*>(up(table.obs_desc, no * OKVFE_DESC_BYTES));
    v.obs_backproj = static_cast<const double*>(up(table.obs_backproj, no * 24));
    v.poses = static_cast<const okvfe_pose*>(up(table.poses, np * sizeof(okvfe_pose)));
    c.check(okvfe_stream_synchronize(nullptr));  // (the copies ran on the null stream)
    c.check(okvfe_landmark_table_check_device(c.get(), &v, nullptr));
    return out;
  }
  // Loop closure: Frontend::verifyRecognisedPlace (Frontend.cpp:270-397) up to the point where ceres takes over.  The
  // landmark set of an old frame on the host, a device copy of it, the descriptor matching with the claims and count
  // gates, and the consensus with the verdict.  What stays with the caller: the walk over the DBoW results and its
  // non-maximum suppression (:771-819), the sampler and gp3p, opengv's adaptive stop, the ceres refinement (:399-527),
  // the Hessian H (:529-551), attemptLoopClosure and everything after it.
  struct PlaceLandmarkSet {
    std::vector<uint64_t> ids;       // ascending
    std::vector<double> hp;          // x 4
    std::vector<int32_t> descBegin;  // ids.size() + 1
    std::vector<uint8_t> pool;       // descBegin.back() x 48
  };
  // The landmark set of an old frame (Frontend.cpp:289-327): oldFrame one FrameData per camera (keypoints' landmarkIds
  // and descriptors are read; the use_cnn filter of :305-317 is the caller's, which passes id 0); landmarks /
  // initialised: per camera, per keypoint, what getLandmark returns.  eigenTree: the order of norm()'s sum, as
  // okvfe_set_fp64_reduction.
  static PlaceLandmarkSet placeLandmarkSet(const std::vector<FrameData>& oldFrame,
                                           const std::vector<std::vector<std::array<double, 4>>>& landmarks,
                                           const std::vector<std::vector<uint8_t>>& initialised, bool eigenTree = true) {
    if (landmarks.size() != oldFrame.size() || initialised.size() != oldFrame.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "placeLandmarkSet: landmarks and initialised: one vector per camera");
    std::vector<int32_t> nKps;
    std::vector<uint64_t> ids;
    std::vector<double> hp;
    std::vector<uint8_t> init, desc;
    for (size_t im = 0; im < oldFrame.size(); ++im) {
      const FrameData& f = oldFrame[im];
      const size_t n = f.keypoints.size();
      if (f.landmarkIds.size() != n || landmarks[im].size() != n || initialised[im].size() != n ||
          f.descriptors.data.size() != n * size_t(OKVFE_DESC_BYTES))
        throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "placeLandmarkSet: one id, landmark, flag and descriptor per keypoint");
      nKps.push_back(int32_t(n));
      ids.insert(ids.end(), f.landmarkIds.begin(), f.landmarkIds.end());
      for (const auto& l : landmarks[im]) hp.insert(hp.end(), l.begin(), l.end());
      init.insert(init.end(), initialised[im].begin(), initialised[im].end());
      desc.insert(desc.end(), f.descriptors.data.begin(), f.descriptors.data.end());
    }
    const size_t total = ids.size();
    PlaceLandmarkSet out;
    out.ids.resize(total + 1);
    out.hp.resize(4 * total + 4);
    out.descBegin.resize(total + 1);
    out.pool.resize(size_t(OKVFE_DESC_BYTES) * total + 1);
    int32_t nl = 0, nr = 0;
    const okvfe_status st = okvfe_place_landmark_set(
        int32_t(nKps.size()), nKps.data(), ids.data(), hp.data(), init.data(), desc.data(), eigenTree ? 1 : 0,
        out.ids.data(), out.hp.data(), out.descBegin.data(), int32_t(total), out.pool.data(), int32_t(total), &nl, &nr);
    if (st != OKVFE_OK) throw Exception(st, "okvfe_place_landmark_set");
    out.ids.resize(size_t(nl));
    out.hp.resize(4 * size_t(nl));
    out.descBegin.resize(size_t(nl) + 1);
    out.pool.resize(size_t(OKVFE_DESC_BYTES) * size_t(nr));
    return out;
  }
  // A landmark set in device memory: uploaded once per candidate old frame.  Owns its device copies.
  class DevicePlaceSet {
   public:
    DevicePlaceSet() = default;
    DevicePlaceSet(const DevicePlaceSet&) = delete;
    DevicePlaceSet& operator=(const DevicePlaceSet&) = delete;
    ~DevicePlaceSet() {
      for (void* p : allocs_) okvfe_device_free(p);
    }
    const okvfe_place_set_device& get() const { return view_; }
    const okvfe_map_device& map() const { return map_; }  // (desc_begin, pool) for okvfe_verify_place_blocks_device

   private:
    friend class HipFrontend;
    okvfe_place_set_device view_{};
    okvfe_map_device map_{};
    std::vector<void*> allocs_;
  };
  // Copies `set` to the device with asynchronous copies on `stream`: `set` stays valid and unchanged until it has drained.
  std::shared_ptr<DevicePlaceSet> uploadPlaceSet(size_t cameraIndex, const PlaceLandmarkSet& set, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    const size_t nl = set.ids.size();
    if (set.hp.size() != 4 * nl || set.descBegin.size() != nl + 1 || set.descBegin.back() < 0 ||
        set.pool.size() != size_t(OKVFE_DESC_BYTES) * size_t(set.descBegin.back()))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "uploadPlaceSet: bad set");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    auto out = std::make_shared<DevicePlaceSet>();
    auto up = [&](const void* src, size_t bytes) -> const void* {
      void* d = nullptr;
      c.check(okvfe_device_alloc(device_, bytes ? bytes : 1, &d));
      out->allocs_.push_back(d);
      if (bytes) c.check(okvfe_copy_to_device(d, src, bytes, stream));
      return d;
    };
    out->view_.n_landmarks = int32_t(nl);
    out->view_.hp = static_cast<const double*>(up(set.hp.data(), nl * 32));
    out->map_.n_landmarks = int32_t(nl);
    out->map_.desc_begin = static_cast<const int32_t*>(up(set.descBegin.data(), (nl + 1) * 4));
    out->map_.pool = static_cast<const uint8_t*>(up(set.pool.data(), set.pool.size()));
    return out;
  }
  // Frontend.cpp:330-355, 359, 380 for nMultiframes frames of camera `cameraIndex` (a context of this class holds ONE
  // camera, so a multiframe is one gather block here; a rig whose cameras share a context calls the C entry points
  // itself): okvfe_verify_place_blocks_device into kMinDev / distMinDev (device, nMultiframes x L), then
  // okvfe_place_claims_blocks_device into `result`.  Nothing synchronises the host.
  void verifyPlaceClaimsBlocks(size_t cameraIndex, const DevicePlaceSet& set, const void* blocksDev, int nMultiframes,
                               int32_t* kMinDev, uint32_t* distMinDev, int minInliers,
                               const okvfe_place_claims_device& result, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "verifyPlaceClaimsBlocks: nMultiframes");
    if (nMultiframes == 0) return;
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_verify_place_blocks_device(c.get(), blocksDev, nMultiframes, &set.map(), kMinDev, distMinDev, stream));
    c.check(okvfe_place_claims_blocks_device(c.get(), &set.get(), blocksDev, nMultiframes, 1, kMinDev, distMinDev,
                                             minInliers, &result, stream));
  }
  // Frontend.cpp:372-397 for the same frames: matchLandmarkDev / gateDev as verifyPlaceClaimsBlocks wrote them (gateDev
  // may be null), hypotheses / hypValid / nHyp and their upload as in ransac3d2dBlocks; verdictDev: device bytes, 3 =
  // verified.  result.landmark_out may be matchLandmarkDev.  Nothing else synchronises the host.
  void verifyPlaceConsensusBlocks(size_t cameraIndex, const DevicePlaceSet& set, const void* blocksDev, int nMultiframes,
                                  const okvfe_pose& T_SC, const int32_t* matchLandmarkDev, const uint8_t* gateDev,
                                  const std::vector<double>& hypotheses, const std::vector<uint8_t>& hypValid, int nHyp,
                                  int minInliers, const okvfe_ransac_result_device& result, uint8_t* verdictDev,
                                  double threshold = 16.0, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0 || nHyp < 1 || hypotheses.size() != size_t(nMultiframes) * size_t(nHyp) * 12 ||
        (!hypValid.empty() && hypValid.size() != size_t(nMultiframes) * size_t(nHyp)))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "verifyPlaceConsensusBlocks: nHyp hypotheses (and flags) per multiframe");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const size_t hypBytes = hypotheses.size() * sizeof(double);
    uint8_t* d = uploadHypotheses(cameraIndex, hypotheses, hypValid, stream);
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_place_consensus_blocks_device(
        c.get(), &set.get(), blocksDev, nMultiframes, 1, &cam, &T_SC, matchLandmarkDev, gateDev,
        reinterpret_cast<const double*>(d), hypValid.empty() ? nullptr : d + hypBytes, nHyp, threshold, minInliers, &result,
        verdictDev, stream));
  }
  // The hypotheses verifyPlaceConsensusBlocks scores, made on the device: okvfe_place_hypotheses_blocks_device over the
  // rows verifyPlaceClaimsBlocks wrote; with gateDev[m] == 0 nothing of multiframe m is solved.  The other arguments as
  // in ransacHypothesesBlocks.  Nothing synchronises the host.
  void verifyPlaceHypothesesBlocks(size_t cameraIndex, const DevicePlaceSet& set, const void* blocksDev, int nMultiframes,
                                   const okvfe_pose& T_SC, const int32_t* matchLandmarkDev, const uint8_t* gateDev,
                                   const uint64_t* sampleKeysDev, uint64_t seed, int nHyp,
                                   const okvfe_ransac_hypotheses_device& result, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_place_hypotheses_blocks_device(c.get(), &set.get(), blocksDev, nMultiframes, 1, &cam, &T_SC,
                                                 matchLandmarkDev, gateDev, sampleKeysDev, seed, nHyp, &result, stream));
  }
  // Frontend.cpp:529-551 for the same frames: the Hessian H of the relative pose, the information of the pose-graph edge
  // that attemptLoopClosure adds, and per inlier the residual and minimal Jacobian of its ReprojectionError (what the
  // ceres problem of :399-527 asks for at every iterate).  T_SC_params: the camera's extrinsics as a PoseParameterBlock
  // holds them (t[3], qx qy qz qw); posesDev: device, nMultiframes x 7 doubles in that layout, T_Sold_Snew as the
  // caller's solver left it; matchLandmarkDev / stateDev / verdictDev as verifyPlaceConsensusBlocks wrote them
  // (verdictDev may be null: every multiframe counts).  Nothing synchronises the host.
  void verifyPlaceHessianBlocks(size_t cameraIndex, const DevicePlaceSet& set, const void* blocksDev, int nMultiframes,
                                const std::array<double, 7>& T_SC_params, const double* posesDev,
                                const int32_t* matchLandmarkDev, const uint8_t* stateDev, const uint8_t* verdictDev,
                                const okvfe_place_hessian_device& result, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "verifyPlaceHessianBlocks: nMultiframes");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_place_hessian_blocks_device(c.get(), &set.get(), blocksDev, nMultiframes, 1, &cam, T_SC_params.data(),
                                              posesDev, matchLandmarkDev, stateDev, verdictDev, &result, stream));
  }
  // Frontend.cpp:399-527 for the same frames: the refinement of T_Sold_Snew between the consensus and H, as the defined
  // algorithm of okvfe_place_refine_blocks_device (include/okvfe.h: its two deviations from ceres, PARITY UNPINNED), and
  // H at the pose out.  The start of multiframe m is initialPosesDev (nMultiframes x 7) where given, else hypothesis
  // bestHypothesisDev[m] of hypothesesDev (nMultiframes x nHyp x 12), both as verifyPlaceConsensusBlocks holds them on
  // the device; maxIterations: the reference's 10.  3 + 2 maxIterations short launches (+ 1 for H); nothing
  // synchronises the host.
  void verifyPlaceRefineBlocks(size_t cameraIndex, const DevicePlaceSet& set, const void* blocksDev, int nMultiframes,
                               const std::array<double, 7>& T_SC_params, const double* hypothesesDev, int nHyp,
                               const int32_t* bestHypothesisDev, const double* initialPosesDev,
                               const int32_t* matchLandmarkDev, const uint8_t* stateDev, const uint8_t* verdictDev,
                               int maxIterations, const okvfe_place_refine_device& result, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "verifyPlaceRefineBlocks: nMultiframes");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_place_refine_blocks_device(c.get(), &set.get(), blocksDev, nMultiframes, 1, &cam, T_SC_params.data(),
                                             hypothesesDev, nHyp, bestHypothesisDev, initialPosesDev, matchLandmarkDev,
                                             stateDev, verdictDev, maxIterations, &result, stream));
  }
  // ViFrontendInterface::propagation, i.e. ImuError::propagation (okvis_ceres/src/ImuError.cpp:557-779): the pose guess
  // of a frame from the IMU samples since the last one, its 15 x 15 Jacobian and covariance, and per camera
  // T_WC = T_WS T_SC with the extraction direction of detectAndDescribe (Frontend.cpp:246-251).  The arithmetic, its
  // order and its defined deviations are those of okvfe_imu_propagation (include/okvfe.h).  The host form, no device
  // work: imuMeasurements in deque order; T_WS as a PoseParameterBlock holds it (t[3], qx qy qz qw); T_SC_params one
  // such pose per camera.  eigenTree: the order of okvfe_set_fp64_reduction.
  struct ImuSample {
    uint32_t sec = 0, nsec = 0;  // okvis::Time
    std::array<double, 3> gyroscopes{}, accelerometers{};
  };
  struct Propagation {
    int nPropagated = 0;   // the reference's return value (-1: the samples end before t_end; the state is unchanged)
    int status = 0;        // bit 1: the first sample is later than t_start; bit 2: no samples (nothing else is set then)
    int nOutOfRange = 0;   // intervals whose angle lies beyond pi / 4 (their results are NaN)
    std::array<double, 7> T_WS{};
    std::array<double, 9> speedAndBias{};
    std::vector<double> jacobian, covariance;     // 225 each, row-major; empty where not asked for (or nPropagated < 0)
    std::vector<std::array<double, 7>> T_WC;      // per camera
    std::vector<std::array<float, 3>> gravity_C;  // per camera: the extraction direction
  };
  static double imuTimestamp(uint32_t sec, uint32_t nsec) {  // (sec, nsec) in the eight bytes of a record's first double
    const uint64_t bits = uint64_t(sec) | (uint64_t(nsec) << 32);
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
  }
  static Propagation propagation(const std::vector<ImuSample>& imuMeasurements, const okvfe_imu_params& imuParams,
                                 const std::array<double, 7>& T_WS, const std::array<double, 9>& speedAndBias,
                                 uint32_t tStartSec, uint32_t tStartNsec, uint32_t tEndSec, uint32_t tEndNsec,
                                 const std::vector<std::array<double, 7>>& T_SC_params = {}, bool wantJacobian = false,
                                 bool wantCovariance = false, bool eigenTree = true) {
    const size_t n = imuMeasurements.size(), nc = T_SC_params.size();
    std::vector<double> samples(8 * n + 8, 0.0), state(18), T_SC(7 * nc + 7);
    for (size_t i = 0; i < n; ++i) {
      samples[8 * i] = imuTimestamp(imuMeasurements[i].sec, imuMeasurements[i].nsec);
      for (size_t k = 0; k < 3; ++k) {
        samples[8 * i + 1 + k] = imuMeasurements[i].gyroscopes[k];
        samples[8 * i + 4 + k] = imuMeasurements[i].accelerometers[k];
      }
    }
    state[0] = imuTimestamp(tStartSec, tStartNsec);
    state[1] = imuTimestamp(tEndSec, tEndNsec);
    std::copy(T_WS.begin(), T_WS.end(), state.begin() + 2);
    std::copy(speedAndBias.begin(), speedAndBias.end(), state.begin() + 9);
    for (size_t c = 0; c < nc; ++c) std::copy(T_SC_params[c].begin(), T_SC_params[c].end(), T_SC.begin() + 7 * c);
    const int32_t begin[2] = {0, int32_t(n)};
    Propagation out;
    int32_t ints[3] = {0, 0, 0};
    std::vector<double> jac(225), cov(225), T_WC(7 * nc + 7);
    std::vector<float> grav(3 * nc + 3);
    okvfe_imu_result_device res{};
    res.pose = out.T_WS.data();
    res.speed_and_bias = out.speedAndBias.data();
    res.n_propagated = &ints[0];
    res.status = &ints[1];
    res.n_out_of_range = &ints[2];
    res.jacobian = wantJacobian ? jac.data() : nullptr;
    res.covariance = wantCovariance ? cov.data() : nullptr;
    res.T_WC = nc ? T_WC.data() : nullptr;
    res.gravity_C = nc ? grav.data() : nullptr;
    const okvfe_status st = okvfe_imu_propagation(&imuParams, samples.data(), begin, state.data(), 1, int32_t(nc),
                                                  nc ? T_SC.data() : nullptr, eigenTree ? 1 : 0, &res);
    if (st != OKVFE_OK) throw Exception(st, "okvfe_imu_propagation");
    out.nPropagated = ints[0];
    out.status = ints[1];
    out.nOutOfRange = ints[2];
    if (out.status != 0) return out;
    if (wantJacobian && out.nPropagated >= 0) out.jacobian = jac;
    if (wantCovariance && out.nPropagated >= 0) out.covariance = cov;
    out.T_WC.resize(nc);
    out.gravity_C.resize(nc);
    for (size_t c = 0; c < nc; ++c) {
      std::copy_n(T_WC.begin() + 7 * c, 7, out.T_WC[c].begin());
      std::copy_n(grav.begin() + 3 * c, 3, out.gravity_C[c].begin());
    }
    return out;
  }
  // okvfe_set_fp64_reduction: the order of the 3- and 4-term FP64 sums of every device call, device-wide (true: Eigen's
  // tree, the default).  Drains the device.
  void setFp64Reduction(bool eigenTree) {
    std::lock_guard<std::mutex> lock(mutexes_[0]);
    contexts_[0]->check(okvfe_set_fp64_reduction(contexts_[0]->get(), eigenTree ? OKVFE_SUM3_EIGEN_TREE : OKVFE_SUM3_LEFT_TO_RIGHT));
  }
  // The same for nMultiframes multiframes that live in device memory, in one launch on `stream`: samplesDev,
  // sampleBeginDev and statesDev in the layout of okvfe_imu_propagation_blocks_device; result: device pointers, the
  // optional ones null where not wanted (the form of the kernel follows them).  Runs on the context of cameraIndex; no
  // camera of the context is read.  Nothing synchronises the host.
  void propagationBlocks(size_t cameraIndex, const okvfe_imu_params& imuParams, const double* samplesDev,
                         const int32_t* sampleBeginDev, const double* statesDev, int nMultiframes,
                         const std::vector<std::array<double, 7>>& T_SC_params, const okvfe_imu_result_device& result,
                         void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "propagationBlocks: nMultiframes");
    std::vector<double> T_SC(7 * T_SC_params.size() + 7);
    for (size_t c = 0; c < T_SC_params.size(); ++c) std::copy(T_SC_params[c].begin(), T_SC_params[c].end(), T_SC.begin() + 7 * c);
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_imu_propagation_blocks_device(c.get(), &imuParams, samplesDev, sampleBeginDev, statesDev, nMultiframes,
                                                int32_t(T_SC_params.size()), T_SC_params.empty() ? nullptr : T_SC.data(),
                                                &result, stream));
  }
  // Place recognition: dBow_->database.query / add (Frontend.cpp:660-672, :752-766, :896-898) with the vocabulary and the
  // database in device memory, and the estimator-free part of the walk over the results (:771-802).  A context of this
  // class holds ONE camera, so a multiframe is one gather block here (a rig whose cameras share a context calls the C
  // entry points itself).  What stays with the caller: poseIds, isPlaceRecognitionFrame per entry (suppressibleDev), the
  // attempts limits and the estimator predicates of :801-819.
  struct Vocabulary {
    std::vector<uint8_t> nodeDescriptors;  // n_nodes x 48
    std::vector<int32_t> childBegin;       // n_nodes + 1
    std::vector<int32_t> childIndex;
    std::vector<int32_t> nodeWord;         // n_nodes
    std::vector<double> wordWeight;        // n_words
    int weighting = 0;                     // 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY
    bool normaliseL1 = true;
  };
  // Device memory that a holder below owns (okvfe_device_alloc / okvfe_device_free).
  class DeviceArrays {
   public:
    DeviceArrays() = default;
    DeviceArrays(const DeviceArrays&) = delete;
    DeviceArrays& operator=(const DeviceArrays&) = delete;
    ~DeviceArrays() {
      for (void* p : allocs_) okvfe_device_free(p);
    }

   protected:
    friend class HipFrontend;
    std::vector<void*> allocs_;
  };
  class DeviceVocabulary : public DeviceArrays {
   public:
    const okvfe_vocabulary_device& get() const { return view_; }

   private:
    friend class HipFrontend;
    okvfe_vocabulary_device view_{};
  };
  class DeviceBowVectors : public DeviceArrays {
   public:
    const okvfe_bow_vectors_device& get() const { return view_; }
    int multiframes() const { return multiframes_; }

   private:
    friend class HipFrontend;
    okvfe_bow_vectors_device view_{};
    int multiframes_ = 0;
  };
  class DevicePlaceDatabase : public DeviceArrays {
   public:
    const okvfe_bow_database_device& get() const { return view_; }
    int entries() const { return view_.n_entries; }

   private:
    friend class HipFrontend;
    okvfe_bow_database_device view_{};
  };
  // Runs okvfe_vocabulary_check on the host arrays (throws, the first offence named, if the tree is no tree), then copies
  // them to the device with asynchronous copies on `stream`: `v` stays valid and unchanged until it has drained.
  std::shared_ptr<DeviceVocabulary> uploadVocabulary(size_t cameraIndex, const Vocabulary& v, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    const size_t nn = v.nodeWord.size();
    if (nn < 1 || v.nodeDescriptors.size() != nn * size_t(OKVFE_DESC_BYTES) || v.childBegin.size() != nn + 1 ||
        v.wordWeight.empty() || v.childBegin.back() < 0 || v.childIndex.size() < size_t(v.childBegin.back()))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "uploadVocabulary: bad vocabulary");
    okvfe_vocabulary_device h{};
    h.n_nodes = int32_t(nn);
    h.n_words = int32_t(v.wordWeight.size());
    h.weighting = v.weighting;
    h.normalise_l1 = v.normaliseL1 ? 1 : 0;
    h.node_descriptors = v.nodeDescriptors.data();
    h.child_begin = v.childBegin.data();
    h.child_index = v.childIndex.data();
    h.node_word = v.nodeWord.data();
    h.word_weight = v.wordWeight.data();
    const okvfe_status st = okvfe_vocabulary_check(&h);
    if (st != OKVFE_OK) throw Exception(st, okvfe_last_error(nullptr));
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    auto out = std::make_shared<DeviceVocabulary>();
    auto up = [&](const void* src, size_t bytes) -> const void* {
      void* d = nullptr;
      c.check(okvfe_device_alloc(device_, bytes ? bytes : 1, &d));
      out->allocs_.push_back(d);
      if (bytes) c.check(okvfe_copy_to_device(d, src, bytes, stream));
      return d;
    };
    out->view_ = h;
    out->view_.node_descriptors = static_cast<const uint8_t*>(up(v.nodeDescriptors.data(), v.nodeDescriptors.size()));
    out->view_.child_begin = static_cast<const int32_t*>(up(v.childBegin.data(), (nn + 1) * 4));
    out->view_.child_index = static_cast<const int32_t*>(up(v.childIndex.data(), size_t(v.childBegin.back()) * 4));
    out->view_.node_word = static_cast<const int32_t*>(up(v.nodeWord.data(), nn * 4));
    out->view_.word_weight = static_cast<const double*>(up(v.wordWeight.data(), v.wordWeight.size() * 8));
    return out;
  }
  // Rows for the BowVectors of nMultiframes multiframes of `vocabulary`'s words: the stride is the smallest the vectors
  // call accepts for this context, min(max keypoints, n_words).
  std::shared_ptr<DeviceBowVectors> allocBowVectors(size_t cameraIndex, const DeviceVocabulary& vocabulary, int nMultiframes) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 1) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "allocBowVectors: nMultiframes");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    okvfe_device_outputs o{};
    c.check(okvfe_get_device_outputs(c.get(), &o));
    auto out = std::make_shared<DeviceBowVectors>();
    const size_t stride = size_t(std::max(1, std::min(o.max_keypoints, vocabulary.get().n_words)));
    auto alloc = [&](size_t bytes) -> void* {
      void* d = nullptr;
      c.check(okvfe_device_alloc(device_, bytes, &d));
      out->allocs_.push_back(d);
      return d;
    };
    out->view_.n_words = static_cast<int32_t*>(alloc(size_t(nMultiframes) * 4));
    out->view_.ids = static_cast<int32_t*>(alloc(size_t(nMultiframes) * stride * 4));
    out->view_.values = static_cast<double*>(alloc(size_t(nMultiframes) * stride * 8));
    out->view_.stride = int32_t(stride);
    out->view_.n_vocabulary_words = vocabulary.get().n_words;
    out->multiframes_ = nMultiframes;
    return out;
  }
  // An empty database of up to capEntries entries and capWords words in all (begin and the overflow counter zeroed on
  // `stream`).
  std::shared_ptr<DevicePlaceDatabase> createPlaceDatabase(size_t cameraIndex, int capEntries, int capWords,
                                                           void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (capEntries < 0 || capWords < 0) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "createPlaceDatabase: capacities");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    auto out = std::make_shared<DevicePlaceDatabase>();
    auto alloc = [&](size_t bytes, bool zero) -> void* {
      void* d = nullptr;
      c.check(okvfe_device_alloc(device_, bytes ? bytes : 1, &d));
      out->allocs_.push_back(d);
      if (zero) c.check(okvfe_device_fill(d, 0, bytes, stream));
      return d;
    };
    out->view_.begin = static_cast<int32_t*>(alloc((size_t(capEntries) + 1) * 4, true));
    out->view_.ids = static_cast<int32_t*>(alloc(size_t(capWords) * 4, false));
    out->view_.values = static_cast<double*>(alloc(size_t(capWords) * 8, false));
    out->view_.overflow = static_cast<int32_t*>(alloc(4, true));
    out->view_.cap_entries = capEntries;
    out->view_.cap_words = capWords;
    out->view_.n_entries = 0;
    return out;
  }
  // :660-672 and DBoW2's transform for nMultiframes gather blocks into `vectors`.  wordIdsDev: null, or device
  // nMultiframes x K: the word of every feature.  Nothing synchronises the host.
  void bowVectorsBlocks(size_t cameraIndex, const DeviceVocabulary& vocabulary, const void* blocksDev, int nMultiframes,
                        const DeviceBowVectors& vectors, int32_t* wordIdsDev = nullptr, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0 || nMultiframes > vectors.multiframes())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "bowVectorsBlocks: nMultiframes exceeds the rows of the vectors");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_bow_vectors_blocks_device(c.get(), &vocabulary.get(), blocksDev, nMultiframes, 1, &vectors.get(),
                                            wordIdsDev, stream));
  }
  // database.query with :761-765, :780-799 and :802 for the first nMultiframes rows of `vectors`: per multiframe the
  // number of listed entries, the true number of candidates and the first result.cap candidates in ascending entry id.
  // suppressibleDev: device bytes per entry (isPlaceRecognitionFrame) or null = all ones; scoresDev: null, or device
  // nMultiframes x entries() doubles.  Nothing synchronises the host.
  void placeQueryBlocks(size_t cameraIndex, const DevicePlaceDatabase& database, const DeviceBowVectors& vectors,
                        int nMultiframes, const okvfe_place_candidates_device& result, double minScore = 0.4,
                        const uint8_t* suppressibleDev = nullptr, double* scoresDev = nullptr, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0 || nMultiframes > vectors.multiframes())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "placeQueryBlocks: nMultiframes exceeds the rows of the vectors");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_place_query_blocks_device(c.get(), &database.get(), &vectors.get(), nMultiframes, minScore,
                                            suppressibleDev, scoresDev, &result, stream));
  }
  // database.add (:896-898): the vectors of the multiframes addIndex (strictly ascending) become the next entries.
  // Throws OKVFE_ERR_CAPACITY, nothing changed, if the entries do not fit; words that do not fit are only known on the
  // device (placeDatabaseCheck).  Nothing synchronises the host.
  void placeDatabaseAdd(size_t cameraIndex, DevicePlaceDatabase& database, const DeviceBowVectors& vectors, int nMultiframes,
                        const std::vector<int32_t>& addIndex, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0 || nMultiframes > vectors.multiframes())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "placeDatabaseAdd: nMultiframes exceeds the rows of the vectors");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_bow_database_add_blocks_device(c.get(), &database.view_, &vectors.get(), nMultiframes, addIndex.data(),
                                                 int32_t(addIndex.size()), stream));
  }
  // Waits for `stream`; throws OKVFE_ERR_CAPACITY if an add stored entries empty for want of room in ids / values.
  void placeDatabaseCheck(size_t cameraIndex, const DevicePlaceDatabase& database, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    c.check(okvfe_bow_database_check_device(c.get(), &database.get(), stream));
  }
  // matchToMap (above) for nFrames frames that live in device memory as gather blocks, against an uploaded table: one
  // call per frame batch, nothing synchronises the host.  T_WC1: one pose per frame; useDev: device nFrames x K flags
  // or null; outputs device nFrames x K (K = the context's row capacity); poolOut and its members may be null.  All
  // frames are camera `cameraIndex`'s.  The results are ready when `stream` (null = the context's own) has drained.
  void matchToMapBlocks(size_t cameraIndex, const DeviceLandmarkTable& table, const void* blocksDev, int nFrames,
                        const std::vector<okvfe_pose>& T_WC1, double reprojectionThreshold, bool exclusive,
                        const uint8_t* useDev, const okvfe_landmark_pool_device* poolOut, int32_t* bestLandmarkDev,
                        int32_t* bestDistDev, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nFrames < 0 || T_WC1.size() != size_t(nFrames))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchToMapBlocks: one pose per frame");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    const std::vector<int32_t> cams(size_t(nFrames) + 1, 0);  // slot 0 of the camera's own context
    contexts_[cameraIndex]->check(okvfe_match_to_map_table_blocks_device(
        contexts_[cameraIndex]->get(), &table.get(), blocksDev, nFrames, cams.data(), T_WC1.data(),
        reprojectionThreshold, exclusive ? 1 : 0, useDev, poolOut, bestLandmarkDev, bestDistDev, stream));
  }
  // The second pass of matchToMap (Frontend.cpp:1434-1496) after matchToMapBlocks: every frame over the landmarks its
  // first pass left as not 3-D yet.  pool: what matchToMapBlocks wrote as poolOut for these frames (status, n_desc,
  // obs_rows, e_W and r_W are required); T_WC1: one pose per frame, as it is NOW; previousLandmarkDev: device nFrames x
  // K table rows (the first pass's bestLandmarkDev may be passed as it is) or null; outputs device: nFrames x K,
  // hpsWDev x 4, alreadyMatchedDev nFrames.  Nothing synchronises the host.
  void matchToMapUninitialisedBlocks(size_t cameraIndex, const DeviceLandmarkTable& table,
                                     const okvfe_landmark_pool_device& pool, const void* blocksDev, int nFrames,
                                     const std::vector<okvfe_pose>& T_WC1, bool exclusive, const uint8_t* useDev,
                                     const int32_t* previousLandmarkDev, int32_t* bestLandmarkDev, int32_t* bestDistDev,
                                     double* hpsWDev, uint8_t* hpSetDev, int32_t* alreadyMatchedDev,
                                     void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nFrames < 0 || T_WC1.size() != size_t(nFrames))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchToMapUninitialisedBlocks: one pose per frame");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    const std::vector<int32_t> cams(size_t(nFrames) + 1, 0);  // slot 0 of the camera's own context
    contexts_[cameraIndex]->check(okvfe_match_to_map_table_uninitialised_blocks_device(
        contexts_[cameraIndex]->get(), &table.get(), &pool, blocksDev, nFrames, cams.data(), T_WC1.data(),
        exclusive ? 1 : 0, useDev, previousLandmarkDev, bestLandmarkDev, bestDistDev, hpsWDev, hpSetDev,
        alreadyMatchedDev, stream));
  }
  // Between the two passes (Frontend.cpp:1411-1430): the consensus step of runRansac3d2d for nMultiframes frames of
  // camera `cameraIndex` (a context of this class holds ONE camera, so a multiframe is one gather block here; a rig
  // whose cameras share a context calls okvfe_ransac3d2d_consensus_blocks_device itself).  hypotheses: host,
  // nMultiframes x nHyp x 12 doubles ([R | t] = T_WS, row-major), what the caller's minimal solver produced from its
  // samples; hypValid: host nMultiframes x nHyp bytes or empty (all valid).  Both are uploaded on `stream` into a buffer
  // this object keeps per camera (growing it waits for the device once), with asynchronous copies: the two vectors
  // stay valid and unchanged until `stream` has drained, and a second call for the same camera waits for the first
  // one's stream to drain (the buffer is one per camera).  landmarkDev: device nMultiframes x K table
  // rows, the first pass's bestLandmarkDev as it is; result: device pointers, landmark_out may be landmarkDev.  Nothing
  // else synchronises the host.
  void ransac3d2dBlocks(size_t cameraIndex, const DeviceLandmarkTable& table, const void* blocksDev, int nMultiframes,
                        const okvfe_pose& T_SC, const int32_t* landmarkDev, const std::vector<double>& hypotheses,
                        const std::vector<uint8_t>& hypValid, int nHyp, const okvfe_ransac_result_device& result,
                        bool removeOutliers = true, double threshold = 16.0, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nMultiframes < 0 || nHyp < 1 || hypotheses.size() != size_t(nMultiframes) * size_t(nHyp) * 12 ||
        (!hypValid.empty() && hypValid.size() != size_t(nMultiframes) * size_t(nHyp)))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "ransac3d2dBlocks: nHyp hypotheses (and flags) per multiframe");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const size_t hypBytes = hypotheses.size() * sizeof(double);
    uint8_t* d = uploadHypotheses(cameraIndex, hypotheses, hypValid, stream);
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_ransac3d2d_consensus_blocks_device(
        c.get(), &table.get(), blocksDev, nMultiframes, 1, &cam, &T_SC, landmarkDev, reinterpret_cast<const double*>(d),
        hypValid.empty() ? nullptr : d + hypBytes, nHyp, threshold, removeOutliers ? 1 : 0, &result, stream));
  }
  // The hypotheses ransac3d2dBlocks scores, made on the device instead of on the host: the defined sampler and P3P of
  // okvfe_ransac3d2d_hypotheses_blocks_device (include/okvfe.h: not opengv's; all four samples from one camera).
  // sampleKeysDev: device nMultiframes uint64 or null (the multiframe's index); result.hypotheses / result.hyp_valid are
  // what okvfe_ransac3d2d_consensus_blocks_device takes as hypotheses_dev / hyp_valid_dev.  Nothing synchronises the host.
  void ransacHypothesesBlocks(size_t cameraIndex, const DeviceLandmarkTable& table, const void* blocksDev, int nMultiframes,
                              const okvfe_pose& T_SC, const int32_t* landmarkDev, const uint64_t* sampleKeysDev,
                              uint64_t seed, int nHyp, const okvfe_ransac_hypotheses_device& result,
                              void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const int32_t cam = 0;  // slot 0 of the camera's own context
    c.check(okvfe_ransac3d2d_hypotheses_blocks_device(c.get(), &table.get(), blocksDev, nMultiframes, 1, &cam, &T_SC,
                                                      landmarkDev, sampleKeysDev, seed, nHyp, &result, stream));
  }
  // The hypotheses of both problems of runRansac2d2d, made on the device for the pairs (older frame mf0[p] of blocks0Dev,
  // current frame mf1[p] of blocks1Dev) of camera `cameraIndex`: the defined sampler, two-point rotation and five-point
  // relative pose of okvfe_ransac2d2d_hypotheses_blocks_device (include/okvfe.h: not opengv's).  sampleKeysDev: device
  // nPairs uint64 or null (the pair's index); result.rot_hyp / rot_valid / rel_hyp / rel_valid are what
  // okvfe_ransac2d2d_consensus_blocks_device takes as rot_hyp_dev / rot_valid_dev / rel_hyp_dev / rel_valid_dev.  ONE
  // camera per context, as in ransac2d2dBlocks.  Nothing synchronises the host.
  void ransac2d2dHypothesesBlocks(size_t cameraIndex, const void* blocks0Dev, int nFrames0, const void* blocks1Dev,
                                  int nFrames1, const std::vector<int32_t>& mf0, const std::vector<int32_t>& mf1,
                                  const int32_t* landmark0Dev, const int32_t* landmark1Dev, const uint8_t* addedDev,
                                  int nLandmarks, const uint64_t* sampleKeysDev, uint64_t seed, int nHyp,
                                  const okvfe_ransac2d2d_hypotheses_device& result, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (mf0.size() != mf1.size()) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "ransac2d2dHypothesesBlocks: mf0 / mf1 sizes");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const int32_t cam = 0;  // slot 0 of the camera's own context
    const int32_t none = 0;
    c.check(okvfe_ransac2d2d_hypotheses_blocks_device(
        c.get(), blocks0Dev, nFrames0, blocks1Dev, nFrames1, (int32_t)mf0.size(), mf0.empty() ? &none : mf0.data(),
        mf1.empty() ? &none : mf1.data(), 1, &cam, landmark0Dev, landmark1Dev, addedDev, nLandmarks, sampleKeysDev, seed,
        nHyp, &result, stream));
  }
  // Before initialisation (Frontend.cpp:1961-1969): the consensus step of runRansac2d2d for the pairs (older frame
  // mf0[p] of blocks0Dev, current frame mf1[p] of blocks1Dev) of camera `cameraIndex` (ONE camera per context, so a
  // multiframe is one gather block here; a rig whose cameras share a context calls
  // okvfe_ransac2d2d_consensus_blocks_device itself).  rotHypotheses / relHypotheses: host, nPairs x nHyp x 9 / x 12
  // doubles (row-major rotations / [R12 | t12], frame 1 the older one), what the caller's twopt_rotationOnly and
  // five-point solvers produced from their samples; rotValid / relValid: host nPairs x nHyp bytes or empty (all valid).
  // They are uploaded on `stream` as ransac3d2dBlocks uploads its hypotheses, under the same rules: the vectors stay
  // valid and unchanged until `stream` has drained.  landmark0Dev / landmark1Dev: device ids, K per block, < 0 = none;
  // addedDev: device nLandmarks bytes or null.  result: device pointers, landmark1_out may be landmark1Dev (then a
  // current frame appears in one pair only).  Nothing else synchronises the host.
  void ransac2d2dBlocks(size_t cameraIndex, const void* blocks0Dev, int nFrames0, const void* blocks1Dev, int nFrames1,
                        const std::vector<int32_t>& mf0, const std::vector<int32_t>& mf1, const int32_t* landmark0Dev,
                        const int32_t* landmark1Dev, const uint8_t* addedDev, int nLandmarks,
                        const std::vector<double>& rotHypotheses, const std::vector<uint8_t>& rotValid,
                        const std::vector<double>& relHypotheses, const std::vector<uint8_t>& relValid, int nHyp,
                        const okvfe_ransac2d2d_result_device& result, bool removeOutliers = true, double threshold = 9.0,
                        void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    const size_t nPairs = mf0.size(), perPair = size_t(nHyp < 1 ? 0 : nHyp);
    if (mf1.size() != nPairs || nHyp < 1 || rotHypotheses.size() != nPairs * perPair * 9 ||
        relHypotheses.size() != nPairs * perPair * 12 || (!rotValid.empty() && rotValid.size() != nPairs * perPair) ||
        (!relValid.empty() && relValid.size() != nPairs * perPair))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "ransac2d2dBlocks: one (mf0, mf1) and nHyp hypotheses (and flags) of both problems per pair");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    Context& c = *contexts_[cameraIndex];
    const size_t rotBytes = rotHypotheses.size() * sizeof(double), relBytes = relHypotheses.size() * sizeof(double);
    uint8_t* d = uploadParts(cameraIndex, {{rotHypotheses.data(), rotBytes}, {relHypotheses.data(), relBytes},
                                           {rotValid.data(), rotValid.size()}, {relValid.data(), relValid.size()}}, stream);
    const int32_t cam = 0, none = 0;  // slot 0 of the camera's own context
    c.check(okvfe_ransac2d2d_consensus_blocks_device(
        c.get(), blocks0Dev, nFrames0, blocks1Dev, nFrames1, int32_t(nPairs), nPairs ? mf0.data() : &none,
        nPairs ? mf1.data() : &none, 1, &cam, landmark0Dev, landmark1Dev, addedDev, nLandmarks,
        reinterpret_cast<const double*>(d), rotValid.empty() ? nullptr : d + rotBytes + relBytes,
        reinterpret_cast<const double*>(d + rotBytes), relValid.empty() ? nullptr : d + rotBytes + relBytes + rotValid.size(),
        nHyp, threshold, removeOutliers ? 1 : 0, &result, stream));
  }
  // Frontend::removeOutliers (Frontend.cpp:2152-2205) for nFrames frames of camera `cameraIndex`: T_WC one pose per
  // frame (T_WS T_SC as the caller's Transformation computes it); landmarkOutDev may be landmarkDev; keptDev: device
  // nFrames int32, the reference's return value per frame.  Nothing synchronises the host.
  void removeOutliersBlocks(size_t cameraIndex, const DeviceLandmarkTable& table, const void* blocksDev, int nFrames,
                            const std::vector<okvfe_pose>& T_WC, const int32_t* landmarkDev, int32_t* landmarkOutDev,
                            int32_t* keptDev, double maxError = 4.0, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    if (nFrames < 0 || T_WC.size() != size_t(nFrames))
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "removeOutliersBlocks: one pose per frame");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    const std::vector<int32_t> cams(size_t(nFrames) + 1, 0);  // slot 0 of the camera's own context
    contexts_[cameraIndex]->check(okvfe_remove_outliers_blocks_device(
        contexts_[cameraIndex]->get(), &table.get(), blocksDev, nFrames, cams.data(), T_WC.data(), maxError, landmarkDev,
        landmarkOutDev, keptDev, stream));
  }
  // Frontend::matchStereo (Frontend.cpp:1982-2150) for nMultiframes multiframes of the whole rig that live in device
  // memory as gather blocks; which line is whose:
  //   :1988, :2004-2005   T_WS and T_WC = T_WS * T_SC: the caller's (T_WC, nMultiframes x numCameras(), multiframe-major)
  //   :1990-2000          the loop over im0 < im1 and hasOverlap: the caller's `pairs`, (c0, c1) in that order
  //   :2010-2015          keypoint counts and f0 / f1: from the blocks and the cameras of this object
  //   :2016-2075          the k0 x k1 loop: okvfe_match_stereo_blocks_batch_device, one call per pair (matchStereoRig)
  //   :2076-2141          the landmark bookkeeping: okvfe_stereo_insert_blocks_device (matchStereoInsertBlocks), chained
  //                       over the pairs: ids written for pair (0,1) are read by pair (0,2), rows on one k1 see each other
  //   estimator.addLandmark / setLandmark / addObservation, multiFrame->setLandmarkId: the caller's, replayed from
  //                       result.action / result.lm (okvfe.h) without any geometry
  // The rig shares ONE context (every camera a slot of it; all cameras of one image size and the row capacity K of the
  // per-camera contexts), created at the first call.  The block of (multiframe m, camera c) is block
  // m * blockStrideM + c * blockStrideC of blocksDev; landmarkDev / result.landmark_out: K rows per block, table rows,
  // -1 = none; initialisedDev: one byte per table row; asKeyframeDev: nMultiframes bytes or null (all keyframes).
  // Nothing synchronises the host.
  void matchStereoInsertBlocks(const DeviceLandmarkTable& table, const uint8_t* initialisedDev, const void* blocksDev,
                               int blockStrideM, int blockStrideC, int nMultiframes,
                               const std::vector<std::array<int32_t, 2>>& pairs, const std::vector<okvfe_pose>& T_WC,
                               const okvfe_stereo_match* matchesDev, const int32_t* landmarkDev,
                               const uint8_t* asKeyframeDev, const okvfe_stereo_insert_device& result,
                               void* stream = nullptr) {
    if (nMultiframes < 0 || T_WC.size() != size_t(nMultiframes) * cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchStereoInsertBlocks: one pose per (multiframe, camera)");
    Context& c = rigContext();
    std::lock_guard<std::mutex> lock(rigMutex_);
    std::vector<int32_t> cams(cameras_.size());
    for (size_t i = 0; i < cams.size(); ++i) cams[i] = int32_t(i);
    const okvfe_pose none{};
    c.check(okvfe_stereo_insert_blocks_device(
        c.get(), &table.get(), initialisedDev, blocksDev, blockStrideM, blockStrideC, nMultiframes, int32_t(cams.size()),
        pairs.empty() ? nullptr : pairs[0].data(), int32_t(pairs.size()), cams.data(), T_WC.empty() ? &none : T_WC.data(),
        matchesDev, landmarkDev, asKeyframeDev, &result, stream));
  }
  // The whole of matchStereo on one stream: for every pair the matcher (matchesDev: device pairs x nMultiframes x K,
  // slice p written by pair p), then matchStereoInsertBlocks.  The matcher takes one pose pair per launch, so
  // consecutive multiframes share a launch only when their blocks are consecutive (blockStrideM == 1) and their poses
  // equal byte for byte; otherwise a multiframe costs one launch per pair.
  void matchStereoRig(const DeviceLandmarkTable& table, const uint8_t* initialisedDev, const void* blocksDev,
                      int blockStrideM, int blockStrideC, int nMultiframes,
                      const std::vector<std::array<int32_t, 2>>& pairs, const std::vector<okvfe_pose>& T_WC,
                      okvfe_stereo_match* matchesDev, const int32_t* landmarkDev, const uint8_t* asKeyframeDev,
                      const okvfe_stereo_insert_device& result, void* stream = nullptr) {
    const size_t nc = cameras_.size();
    if (nMultiframes < 0 || T_WC.size() != size_t(nMultiframes) * nc || blockStrideM < 0 || blockStrideC < 0)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchStereoRig: one pose per (multiframe, camera)");
    Context& c = rigContext();
    {
      std::lock_guard<std::mutex> lock(rigMutex_);
      const size_t K = size_t(c.maxKeypoints()), bb = okvfe_gather_block_bytes(c.get());
      const uint8_t* blocks = static_cast<const uint8_t*>(blocksDev);
      for (size_t p = 0; p < pairs.size(); ++p) {
        const int32_t c0 = pairs[p][0], c1 = pairs[p][1];
        if (c0 < 0 || size_t(c0) >= nc || c1 < 0 || size_t(c1) >= nc)
          throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchStereoRig: pair " + std::to_string(p) + " names a camera outside the rig");
        const double f0 = 0.5 * (cameras_[size_t(c0)].base.fu + cameras_[size_t(c0)].base.fv);
        const double f1 = 0.5 * (cameras_[size_t(c1)].base.fu + cameras_[size_t(c1)].base.fv);
        for (int m = 0; m < nMultiframes;) {
          const okvfe_pose& T0 = T_WC[size_t(m) * nc + size_t(c0)];
          const okvfe_pose& T1 = T_WC[size_t(m) * nc + size_t(c1)];
          int n = 1;
          while (blockStrideM == 1 && m + n < nMultiframes &&
                 std::memcmp(&T0, &T_WC[size_t(m + n) * nc + size_t(c0)], sizeof(okvfe_pose)) == 0 &&
                 std::memcmp(&T1, &T_WC[size_t(m + n) * nc + size_t(c1)], sizeof(okvfe_pose)) == 0)
            ++n;
          c.check(okvfe_match_stereo_blocks_batch_device(
              c.get(), blocks + (size_t(m) * size_t(blockStrideM) + size_t(c0) * size_t(blockStrideC)) * bb,
              blocks + (size_t(m) * size_t(blockStrideM) + size_t(c1) * size_t(blockStrideC)) * bb, n, &T0, &T1, f0, f1,
              matchesDev + (p * size_t(nMultiframes) + size_t(m)) * K, stream));
          m += n;
        }
      }
    }
    matchStereoInsertBlocks(table, initialisedDev, blocksDev, blockStrideM, blockStrideC, nMultiframes, pairs, T_WC,
                            matchesDev, landmarkDev, asKeyframeDev, result, stream);
  }
  // Row capacity and block size of the rig's shared context (creates it)
  int rigMaxKeypoints() { return rigContext().maxKeypoints(); }
  size_t rigBlockBytes() { return okvfe_gather_block_bytes(rigContext().get()); }
  // Frontend::matchMotionStereo's matcher (Frontend.cpp:1789-1905) for idx0.size() (older block, current block) pairs
  // of camera `cameraIndex` in one launch, and -- with `claim` -- the frame-data part of its insertion loop
  // (:1915-1958; okvfe.h, okvfe_match_motion_stereo_blocks_batch_device).  blocks0Dev / blocks1Dev: device arrays of
  // nBlocks0 / nBlocks1 gather blocks; pair p matches older block idx0[p] against current block idx1[p] with the poses
  // T_WC0[p], T_WC1[p]; skip0Dev: device pairs x K (pair-major) or null; matched1Dev: device nBlocks1 x K (by current
  // block) or null; matchesDev: device pairs x K.  With claim a current block may appear once.  Nothing synchronises
  // the host.
  void matchMotionStereoBlocks(size_t cameraIndex, const void* blocks0Dev, int nBlocks0, const void* blocks1Dev,
                               int nBlocks1, const std::vector<int32_t>& idx0, const std::vector<int32_t>& idx1,
                               const std::vector<okvfe_pose>& T_WC0, const std::vector<okvfe_pose>& T_WC1,
                               const uint8_t* skip0Dev, const uint8_t* matched1Dev, okvfe_motion_match* matchesDev,
                               const okvfe_motion_claim_device* claim = nullptr, void* stream = nullptr) {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
    const size_t n = idx0.size();
    if (idx1.size() != n || T_WC0.size() != n || T_WC1.size() != n)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchMotionStereoBlocks: two block indices and two poses per pair");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    if (!extractors_[cameraIndex].isCameraAware()) extractors_[cameraIndex].setCamera(cameras_[cameraIndex]);
    const std::vector<int32_t> cams(n + 1, 0);  // slot 0 of the camera's own context
    contexts_[cameraIndex]->check(okvfe_match_motion_stereo_blocks_batch_device(
        contexts_[cameraIndex]->get(), blocks0Dev, nBlocks0, blocks1Dev, nBlocks1, int32_t(n), idx0.data(), idx1.data(),
        cams.data(), T_WC0.data(), T_WC1.data(), skip0Dev, matched1Dev, matchesDev, claim, stream));
  }
  // One older frame of a sweep: its pairs (as above) and where their results go (device; claimedDev pairs x K,
  // nClaimedDev pairs int32)
  struct MotionSweepStep {
    std::vector<int32_t> idx0, idx1;
    std::vector<okvfe_pose> T_WC0, T_WC1;
    const uint8_t* skip0Dev = nullptr;
    okvfe_motion_match* matchesDev = nullptr;
    uint8_t* claimedDev = nullptr;
    int32_t* nClaimedDev = nullptr;
  };
  // The loop over the older frames (Frontend.cpp:1773): one matchMotionStereoBlocks call with claims per step, queued
  // back to back on `stream`, matched1Dev (device nBlocks1 x K) read by each step's matcher and updated in place by its
  // claims, so that step j + 1 matches only the current keypoints steps 0 .. j left free (:1792-1796).  Returns without
  // synchronising; the estimator-side half of the insertion loop stays with the caller (okvfe.h).
  void matchMotionStereoSweep(size_t cameraIndex, const void* blocks0Dev, int nBlocks0, const void* blocks1Dev,
                              int nBlocks1, const std::vector<MotionSweepStep>& steps, uint8_t* matched1Dev,
                              void* stream = nullptr) {
    if (!matched1Dev) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "matchMotionStereoSweep: matched1Dev is required");
    for (const MotionSweepStep& st : steps) {
      okvfe_motion_claim_device claim{};
      claim.claimed = st.claimedDev;
      claim.n_claimed = st.nClaimedDev;
      claim.matched1_out = matched1Dev;
      matchMotionStereoBlocks(cameraIndex, blocks0Dev, nBlocks0, blocks1Dev, nBlocks1, st.idx0, st.idx1, st.T_WC0,
                              st.T_WC1, st.skip0Dev, matched1Dev, st.matchesDev, &claim, stream);
    }
  }
  // Frontend::matchToMapByThread on an already pooled 3-D landmark set (Frontend.cpp:1552-1589)
  MapMatches matchToMapPooled(size_t cameraIndex, const FrameData& frame, const std::vector<uint8_t>& use,
                              const std::vector<double>& projections, const std::vector<int32_t>& descBegin,
                              const std::vector<uint8_t>& pool, double reprojectionThreshold) {
    checkCamera(cameraIndex);
    checkFrame(frame, kDescriptors, "matchToMapPooled: frame");
    checkPerKeypoint(use.size(), frame, "matchToMapPooled: use");
    const size_t rows = checkDescBegin(descBegin, "matchToMapPooled");
    checkLength(projections.size(), 2 * (descBegin.size() - 1), "matchToMapPooled: projections: 2 per landmark");
    checkLength(pool.size(), size_t(OKVFE_DESC_BYTES) * rows, "matchToMapPooled: pool: 48 bytes per row of descBegin");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    const size_t n = frame.keypoints.size();
    MapMatches m{std::vector<int32_t>(n, -1), std::vector<int32_t>(n, 0)};
    const std::vector<uint8_t> all(n, 1);
    contexts_[cameraIndex]->check(okvfe_match_to_map(
        contexts_[cameraIndex]->get(), frame.descriptors.data.data(), frame.keypoints.data(),
        use.empty() ? all.data() : use.data(), int32_t(n), projections.data(), descBegin.data(),
        int32_t(descBegin.size()) - 1, pool.data(), reprojectionThreshold, m.landmark.data(), m.distance.data()));
    return m;
  }

  struct UninitialisedMatches {
    MapMatches matches;
    std::vector<std::array<double, 4>> hp_W;  // written where hpSet[k]
    std::vector<uint8_t> hpSet;
    int32_t alreadyMatched = 0;  // ctrs of Frontend.cpp:1702
  };
  // Frontend::matchToMapByThreadUnitialised (Frontend.cpp:1616-1719): landmarks without a 3-D
  // position yet; pool row d carries its observing unit ray e0_W[d] and camera centre r0_W[d].
  // A keypoint takes part iff use[k] (empty = every keypoint) AND frame.backProjectionsValid[k]: the
  // reference sets its use[k] only where getBackProjection(im, k, ...) succeeds (Frontend.cpp:1622-1634),
  // as the device-resident form does.  The other half of those lines ("already matched", :1628-1632)
  // needs the exclusive flag and stays in the caller's use.
  UninitialisedMatches matchToMapUninitialised(size_t cameraIndex, const FrameData& frame,
                                               const std::vector<uint8_t>& use,
                                               const std::vector<int32_t>& previousLandmark,
                                               const std::vector<int32_t>& descBegin,
                                               const std::vector<uint8_t>& pool, const std::vector<double>& e0_W,
                                               const std::vector<double>& r0_W, const okvfe_pose& T_WC1) {
    checkCamera(cameraIndex);
    checkFrame(frame, kDescriptors | kBackProjections, "matchToMapUninitialised: frame");
    // empty = "every keypoint" / "no keypoint carries a landmark yet", like the sibling wrappers
    checkPerKeypoint(use.size(), frame, "matchToMapUninitialised: use");
    checkPerKeypoint(previousLandmark.size(), frame, "matchToMapUninitialised: previousLandmark");
    const size_t rows = checkDescBegin(descBegin, "matchToMapUninitialised");
    checkLength(pool.size(), size_t(OKVFE_DESC_BYTES) * rows, "matchToMapUninitialised: pool: 48 bytes per row of descBegin");
    checkLength(e0_W.size(), 3 * rows, "matchToMapUninitialised: e0_W: 3 per row of descBegin");
    checkLength(r0_W.size(), 3 * rows, "matchToMapUninitialised: r0_W: 3 per row of descBegin");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    const size_t n = frame.keypoints.size();
    UninitialisedMatches u;
    u.matches = MapMatches{std::vector<int32_t>(n, -1), std::vector<int32_t>(n, 0)};
    std::vector<double> hp(4 * n + 4);
    u.hpSet.assign(n, 0);
    const std::vector<double> bp = flat(frame.backProjections);
    const double focal = 0.5 * (cameras_[cameraIndex].base.fu + cameras_[cameraIndex].base.fv);
    std::vector<uint8_t> take(n);  // Frontend.cpp:1622-1634
    for (size_t k = 0; k < n; ++k) take[k] = (use.empty() || use[k]) && frame.backProjectionsValid[k] ? 1 : 0;
    const std::vector<int32_t> none(n, -1);
    contexts_[cameraIndex]->check(okvfe_match_to_map_uninitialised(
        contexts_[cameraIndex]->get(), frame.descriptors.data.data(), bp.data(), take.data(),
        previousLandmark.empty() ? none.data() : previousLandmark.data(), int32_t(n), descBegin.data(),
        int32_t(descBegin.size()) - 1, pool.data(),
        e0_W.data(), r0_W.data(), &T_WC1, focal, u.matches.landmark.data(), u.matches.distance.data(), hp.data(),
        u.hpSet.data(), &u.alreadyMatched));
    u.hp_W.resize(n);
    for (size_t k = 0; k < n; ++k) u.hp_W[k] = {hp[4 * k], hp[4 * k + 1], hp[4 * k + 2], hp[4 * k + 3]};
    return u;
  }

  struct PlaceMatches {  // per old landmark: best keypoint of the frame and its distance
    std::vector<int32_t> kMin;
    std::vector<uint32_t> distMin;
  };
  // the descriptor matching of Frontend::verifyRecognisedPlace for all old landmarks against one
  // camera of the current frame (Frontend.cpp:330-355)
  PlaceMatches verifyRecognisedPlace(size_t cameraIndex, const std::vector<uint8_t>& landmarkDescriptors,
                                     const std::vector<int32_t>& descBegin, const FrameData& frame) {
    checkCamera(cameraIndex);
    checkFrame(frame, kDescriptors, "verifyRecognisedPlace: frame");
    const size_t rows = checkDescBegin(descBegin, "verifyRecognisedPlace");
    checkLength(landmarkDescriptors.size(), size_t(OKVFE_DESC_BYTES) * rows,
                "verifyRecognisedPlace: landmarkDescriptors: 48 bytes per row of descBegin");
    std::lock_guard<std::mutex> lock(mutexes_[cameraIndex]);
    const size_t nl = descBegin.size() - 1;
    PlaceMatches p{std::vector<int32_t>(nl, 0), std::vector<uint32_t>(nl, 0)};
    contexts_[cameraIndex]->check(okvfe_verify_place_match(
        contexts_[cameraIndex]->get(), landmarkDescriptors.data(), descBegin.data(), int32_t(nl),
        frame.descriptors.data.data(), int32_t(frame.keypoints.size()), p.kMin.data(), p.distMin.data()));
    return p;
  }

  // Frontend::doWeNeedANewKeyframe(estimator, currentFrame) (Frontend.cpp:1058-1167) from :1067 on: the coverage
  // masks of every camera image are painted and counted on the GPU (okvfe_keyframe_coverage), the decision is
  // okvfe_keyframe_decision.  currentFrame / every entry of otherFrames: one FrameData per camera, whose landmarkIds
  // say which keypoints carry a landmark (0 = none).  otherFrames are the multiframes the reference walks at
  // :1105-1122 (keyframes, loop-closure frames, keyframes in the IMU window): that choice needs the estimator and
  // stays with the caller, as do the two early returns at :1060-1065 (estimator.numFrames() < 4 -> true;
  // !isInitialized_ -> false), which come before this call.  overlapOut: the value compared at :1161.
  bool doWeNeedANewKeyframe(const std::vector<FrameData>& currentFrame,
                            const std::vector<std::vector<FrameData>>& otherFrames,
                            float keyframeInsertionOverlapThreshold = 0.55f, double* overlapOut = nullptr,
                            double kptrad = 0.09) {
    const size_t nc = cameras_.size();
    if (currentFrame.size() != nc) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "currentFrame: one FrameData per camera");
    std::vector<uint64_t> lmIds;  // :1073, :1091 -- as a list: the library ignores order, duplicates and zeros
    for (const FrameData& f : currentFrame) lmIds.insert(lmIds.end(), f.landmarkIds.begin(), f.landmarkIds.end());
    if (lmIds.empty()) lmIds.push_back(0);  // an empty set is still a set (non-null pointer)
    std::vector<okvfe_coverage> current(nc), others(otherFrames.size() * nc);
    auto coverage = [&](size_t im, const FrameData& f, bool withSet, okvfe_coverage* out) {
      if (f.landmarkIds.size() != f.keypoints.size())
        throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "landmarkIds: one entry per keypoint");
      std::lock_guard<std::mutex> lock(mutexes_[im]);
      contexts_[im]->check(okvfe_keyframe_coverage(contexts_[im]->get(), f.keypoints.data(), int32_t(f.keypoints.size()),
                                                   f.landmarkIds.data(), withSet ? lmIds.data() : nullptr,
                                                   withSet ? int32_t(lmIds.size()) : 0, kptrad, out));
    };
    for (size_t im = 0; im < nc; ++im) coverage(im, currentFrame[im], false, &current[im]);
    for (size_t o = 0; o < otherFrames.size(); ++o) {
      if (otherFrames[o].size() != nc) throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "otherFrames: one FrameData per camera");
      for (size_t im = 0; im < nc; ++im) coverage(im, otherFrames[o][im], true, &others[o * nc + im]);
    }
    int32_t need = 0;
    double overlap = 0.0;
    const okvfe_status st = okvfe_keyframe_decision(current.data(), int32_t(nc), others.empty() ? nullptr : others.data(),
                                                    int32_t(otherFrames.size()), keyframeInsertionOverlapThreshold, &need,
                                                    &overlap);
    if (st != OKVFE_OK) throw Exception(st, "okvfe_keyframe_decision");
    if (overlapOut) *overlapOut = overlap;
    return need != 0;
  }

  // kptradius_ after ViSlamBackend::setDetectorUniformityRadius (ViSlamBackend.hpp:208-210)
  double backendKeypointRadius() const { return 0.09 * double(params_.detection_threshold) / 36.0; }

  // ViSlamBackend::overlapFraction(frameA, frameB) (ViSlamBackend.cpp:2341-2427), the B = 1 form: one FrameData per
  // camera on each side; per image the masks are painted and counted by okvfe_keyframe_coverage with the OTHER
  // multiframe's ids, all cameras concatenated, as the set (an id of this side is in its own set by construction), the
  // sums go through okvfe_overlap_fraction.  kptrad < 0: backendKeypointRadius().  countsOut: the summed counts.
  double overlapFraction(const std::vector<FrameData>& frameA, const std::vector<FrameData>& frameB, double kptrad = -1.0,
                         okvfe_overlap_counts* countsOut = nullptr) {
    const size_t nc = cameras_.size();
    if (frameA.size() != nc || frameB.size() != nc)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "overlapFraction: one FrameData per camera on both sides");
    if (kptrad < 0.0) kptrad = backendKeypointRadius();
    const std::vector<FrameData>* frames[2] = {&frameA, &frameB};
    okvfe_overlap_counts counts{};
    for (int f = 0; f < 2; ++f) {
      std::vector<uint64_t> otherIds;  // as a list: the library ignores order, duplicates and zeros
      for (const FrameData& o : *frames[1 - f]) {
        if (o.landmarkIds.size() != o.keypoints.size())
          throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "landmarkIds: one entry per keypoint");
        otherIds.insert(otherIds.end(), o.landmarkIds.begin(), o.landmarkIds.end());
      }
      if (otherIds.empty()) otherIds.push_back(0);  // an empty set is still a set (non-null pointer)
      for (size_t im = 0; im < nc; ++im) {
        const FrameData& fd = (*frames[f])[im];
        okvfe_coverage c{};
        std::lock_guard<std::mutex> lock(mutexes_[im]);
        contexts_[im]->check(okvfe_keyframe_coverage(contexts_[im]->get(), fd.keypoints.data(), int32_t(fd.keypoints.size()),
                                                     fd.landmarkIds.data(), otherIds.data(), int32_t(otherIds.size()),
                                                     kptrad, &c));
        counts.n_keypoints[f] += c.n_keypoints;
        counts.n_matched[f] += c.n_matched;
        counts.intersection_area[f] += c.intersection_area;
        counts.union_area[f] += c.union_area;
      }
    }
    if (countsOut) *countsOut = counts;
    double overlap = 0.0;
    const okvfe_status st = okvfe_overlap_fraction(&counts, 1, &overlap);
    if (st != OKVFE_OK) throw Exception(st, "okvfe_overlap_fraction");
    return overlap;
  }
  // The counts of overlapFraction for pairA.size() ordered pairs of multiframes that live in device memory as gather
  // blocks, in one launch on the rig's shared context (okvfe_overlap_pairs_blocks_device; addressing as in
  // matchStereoInsertBlocks).  landmarkIdsDev: K u64 per block at the block's index.  countsDev: one record per pair;
  // coverageDev: null, or pairs x 2 x numCameras() per-image records.  Nothing synchronises the host: download the
  // counts and hand them to okvfe_overlap_fraction.
  void overlapFractionBlocks(const void* blocksDev, int blockStrideM, int blockStrideC, int nMultiframes,
                             const uint64_t* landmarkIdsDev, const std::vector<int32_t>& pairA,
                             const std::vector<int32_t>& pairB, okvfe_overlap_counts* countsDev,
                             okvfe_coverage* coverageDev = nullptr, double kptrad = -1.0, void* stream = nullptr) {
    if (pairA.size() != pairB.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "overlapFractionBlocks: pairA / pairB: one multiframe index each per pair");
    if (kptrad < 0.0) kptrad = backendKeypointRadius();
    Context& c = rigContext();
    std::lock_guard<std::mutex> lock(rigMutex_);
    c.check(okvfe_overlap_pairs_blocks_device(c.get(), blocksDev, blockStrideM, blockStrideC, nMultiframes,
                                              int32_t(cameras_.size()), landmarkIdsDev, pairA.data(), pairB.data(),
                                              int32_t(pairA.size()), kptrad, countsDev, coverageDev, stream));
  }
  // ViSlamBackend::trackingQuality(id) (ViSlamBackend.cpp:157-196): frame one FrameData per camera;
  // observedElsewhere[im][k] != 0 iff the landmark of keypoint k exists and has an observation in another frame
  // (:178-187, estimator state: the caller's).  The matches masks are painted by okvfe_keyframe_coverage.
  double trackingQuality(const std::vector<FrameData>& frame, const std::vector<std::vector<uint8_t>>& observedElsewhere,
                         double kptrad = -1.0) {
    const size_t nc = cameras_.size();
    if (frame.size() != nc || observedElsewhere.size() != nc)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "trackingQuality: one FrameData and one flag row per camera");
    if (kptrad < 0.0) kptrad = backendKeypointRadius();
    std::vector<okvfe_coverage> records(nc);
    for (size_t im = 0; im < nc; ++im) {
      const FrameData& fd = frame[im];
      if (fd.landmarkIds.size() != fd.keypoints.size() || observedElsewhere[im].size() != fd.keypoints.size())
        throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "trackingQuality: one landmark id and one flag per keypoint");
      if (cameras_[im].base.width != cameras_[0].base.width || cameras_[im].base.height != cameras_[0].base.height)
        throw Exception(OKVFE_ERR_UNSUPPORTED, "trackingQuality: cameras of one image size");
      std::vector<uint64_t> ids(fd.landmarkIds);
      for (size_t k = 0; k < ids.size(); ++k)
        if (!observedElsewhere[im][k]) ids[k] = 0;
      std::lock_guard<std::mutex> lock(mutexes_[im]);
      contexts_[im]->check(okvfe_keyframe_coverage(contexts_[im]->get(), fd.keypoints.data(), int32_t(fd.keypoints.size()),
                                                   ids.data(), nullptr, 0, kptrad, &records[im]));
    }
    double quality = 0.0;
    const okvfe_status st = okvfe_tracking_quality(records.data(), int32_t(nc), cameras_[0].base.width,
                                                   cameras_[0].base.height, kptrad, &quality);
    if (st != OKVFE_OK) throw Exception(st, "okvfe_tracking_quality");
    return quality;
  }
  // The order of the motion-stereo sweep (Frontend.cpp:1751-1767): overlaps[i] = overlapFraction(previous frame, frame
  // i), frameIds[i] its StateId; previous: index of the previous frame among them, -1 = not among them.  Returns the
  // indices in sweep order.  Which frames are candidates (:1742-1749) is the caller's.  A NaN overlap throws.
  static std::vector<int32_t> motionStereoFrameOrder(const std::vector<double>& overlaps,
                                                     const std::vector<uint64_t>& frameIds, int32_t previous = -1) {
    if (overlaps.size() != frameIds.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "motionStereoFrameOrder: one id per overlap");
    std::vector<int32_t> order(overlaps.size());
    int32_t n = 0;
    const okvfe_status st = okvfe_motion_frame_order(overlaps.data(), frameIds.data(), int32_t(overlaps.size()), previous,
                                                     order.data(), &n);
    if (st != OKVFE_OK)
      throw Exception(st, n >= 0 ? "okvfe_motion_frame_order: entry " + std::to_string(n) + ": NaN overlap"
                                 : std::string("okvfe_motion_frame_order"));
    order.resize(size_t(n));
    return order;
  }

 private:
  // What the host-buffer matchers check before anything reaches the library (they hand it plain pointers and the
  // frame's keypoint count): every failure throws OKVFE_ERR_INVALID_ARGUMENT.
  enum FrameMembers { kDescriptors = 1, kBackProjections = 2 };
  void checkCamera(size_t cameraIndex) const {
    if (cameraIndex >= cameras_.size())
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, "Camera index exceeds number of cameras.");
  }
  static void checkLength(size_t got, size_t want, const std::string& what) {
    if (got != want)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT,
                      what + " (" + std::to_string(got) + " given, " + std::to_string(want) + " needed)");
  }
  // A FrameData is well-formed when descriptors.data holds 48 bytes per keypoint and backProjections /
  // backProjectionsValid one entry per keypoint; a method asks for the members it reads.
  static void checkFrame(const FrameData& f, int members, const std::string& what) {
    const size_t n = f.keypoints.size();
    if (members & kDescriptors)
      checkLength(f.descriptors.data.size(), size_t(OKVFE_DESC_BYTES) * n, what + ": descriptors.data: 48 bytes per keypoint");
    if (members & kBackProjections) {
      checkLength(f.backProjections.size(), n, what + ": backProjections: one per keypoint");
      checkLength(f.backProjectionsValid.size(), n, what + ": backProjectionsValid: one per keypoint");
    }
  }
  // skip0 / matched1 / use / previousLandmark: empty, or one entry per keypoint of their frame
  static void checkPerKeypoint(size_t size, const FrameData& f, const std::string& what) {
    if (size != 0) checkLength(size, f.keypoints.size(), what + ": empty or one entry per keypoint");
  }
  // descBegin: n_landmarks + 1 entries, the last one the number of pool rows -> that number
  static size_t checkDescBegin(const std::vector<int32_t>& descBegin, const std::string& what) {
    if (descBegin.empty() || descBegin.back() < 0)
      throw Exception(OKVFE_ERR_INVALID_ARGUMENT, what + ": descBegin needs n_landmarks + 1 entries");
    return size_t(descBegin.back());
  }
  static std::vector<double> flat(const std::vector<std::array<double, 3>>& v) {
    std::vector<double> b(v.size() * 3 + 3);
    for (size_t k = 0; k < v.size(); ++k)
      for (int i = 0; i < 3; ++i) b[3 * k + size_t(i)] = v[k][size_t(i)];
    return b;
  }
  std::vector<okvfe_camera_ext> cameras_;
  std::vector<std::mutex> mutexes_;
  std::vector<std::shared_ptr<Context>> contexts_;
  std::vector<HipBriskDetector> detectors_;
  std::vector<HipBriskExtractor> extractors_;
  std::vector<std::vector<double>> bp_scratch_;  // per camera (one thread per camera)
  struct HypothesisScratch {  // ransac3d2dBlocks: the device copy of a call's hypotheses and flags
    void* d = nullptr;
    size_t bytes = 0;
    HypothesisScratch() = default;
    HypothesisScratch(const HypothesisScratch&) = delete;
    HypothesisScratch& operator=(const HypothesisScratch&) = delete;
    ~HypothesisScratch() {
      if (d) okvfe_device_free(d);
    }
  };
  std::vector<HypothesisScratch> hyp_scratch_;  // per camera
  // host arrays, one behind the other, into the camera's scratch buffer with asynchronous copies on `stream` (mutex held)
  struct HostPart {
    const void* p;
    size_t bytes;
  };
  uint8_t* uploadParts(size_t cameraIndex, std::initializer_list<HostPart> parts, void* stream) {
    Context& c = *contexts_[cameraIndex];
    HypothesisScratch& hs = hyp_scratch_[cameraIndex];
    size_t bytes = 0;
    for (const HostPart& part : parts) bytes += part.bytes;
    if (bytes > hs.bytes) {
      if (hs.d) {
        c.check(okvfe_stream_synchronize(nullptr));
        if (stream) c.check(okvfe_stream_synchronize(stream));
        okvfe_device_free(hs.d);
        hs.d = nullptr;
        hs.bytes = 0;
      }
      c.check(okvfe_device_alloc(device_, bytes, &hs.d));
      hs.bytes = bytes;
    }
    uint8_t* d = static_cast<uint8_t*>(hs.d);
    size_t at = 0;
    for (const HostPart& part : parts) {
      if (part.bytes) c.check(okvfe_copy_to_device(d + at, part.p, part.bytes, stream));
      at += part.bytes;
    }
    return d;
  }
  // hypotheses, then the flags
  uint8_t* uploadHypotheses(size_t cameraIndex, const std::vector<double>& hypotheses, const std::vector<uint8_t>& hypValid,
                            void* stream) {
    return uploadParts(cameraIndex, {{hypotheses.data(), hypotheses.size() * sizeof(double)}, {hypValid.data(), hypValid.size()}},
                       stream);
  }
  // the context matchStereoInsertBlocks / matchStereoRig run on: every camera of the rig in a slot of its own
  Context& rigContext() {
    std::lock_guard<std::mutex> lock(rigMutex_);
    if (!rigContext_) {
      for (const okvfe_camera_ext& cam : cameras_)
        if (cam.base.width != cameras_[0].base.width || cam.base.height != cameras_[0].base.height)
          throw Exception(OKVFE_ERR_UNSUPPORTED, "the rig's shared context needs cameras of one image size");
      okvfe_config cfg{};
      cfg.abi_version = OKVFE_ABI_VERSION;
      cfg.device = device_;
      cfg.width = cameras_[0].base.width;
      cfg.height = cameras_[0].base.height;
      cfg.max_batch = 1;
      cfg.num_cameras = int32_t(cameras_.size());
      cfg.uniformity_radius = params_.detection_threshold;
      cfg.octaves = params_.octaves;
      cfg.absolute_threshold = params_.absolute_threshold;
      cfg.max_keypoints = params_.max_num_keypoints;
      cfg.rotation_invariant = params_.rotation_invariance;
      cfg.scale_invariant = params_.scale_invariance;
      cfg.match_threshold = params_.matching_threshold;
      cfg.box_scale = params_.box_scale;
      auto ctx = std::make_shared<Context>(cfg);
      for (size_t i = 0; i < cameras_.size(); ++i) ctx->check(okvfe_set_camera_ext(ctx->get(), int32_t(i), &cameras_[i]));
      rigContext_ = ctx;
    }
    return *rigContext_;
  }
  FrontendParameters params_;
  std::shared_ptr<Context> rigContext_;
  std::mutex rigMutex_;
  int device_ = 0;
};

}  // namespace okvfe
