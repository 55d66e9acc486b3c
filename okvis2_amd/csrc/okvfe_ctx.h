// okvfe_ctx.h -- the context behind the C ABI and the runtime helpers its entry points share
// (capi_context.cpp: creation, cameras, pattern, profiling; capi_detect.cpp: detector / extractor
// pipeline; capi_match.cpp: stereo / motion / Hamming matchers and gather blocks; capi_map.cpp: map
// matchers and the host seam of place recognition; capi_ransac.cpp: consensus, hypotheses and outlier removal
// between the two matcher passes; capi_ransac2d2d.cpp: the consensus of runRansac2d2d; capi_stereo.cpp: matchStereo's
// landmark bookkeeping; capi_place.cpp: verifyRecognisedPlace, its Hessian and refinement; capi_bow.cpp: vocabulary,
// BoW vectors and the place database; capi_keyframe.cpp: coverage masks and the keyframe decision; capi_overlap.cpp:
// overlapFraction / trackingQuality; capi_imu.cpp: IMU propagation).  Internal to libokvfe.so.
//
// A new entry point writes none of the plumbing itself: a call on the caller's host arrays lays them out with
// ScratchLayout and moves them with ScratchCall; a call on device batches checks its camera slots with rig_slots and
// ends in ring_launch or finish_call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "okvfe_internal.h"
#include "scratch_layout.h"

using namespace okvfe;  // internal header of the runtime's own translation units

// The context holds what outlives a call.  A call's decisions travel in its CallPlan: built once by the entry point
// (make_call_plan, capi_detect.cpp), handed down by const reference -- a lane view receives its owner's -- and gone
// when the call returns.
struct BatchFacts {  // of the images of one parameter upload (upload_image_params)
  bool wide_patches = false;      // a camera-aware image comes from a camera whose patches often exceed the LDS buffer
  bool aware_fast = true;         // none comes from a cam_aware_slow camera
  bool all_aware = false;         // every image is extracted camera-aware
  bool none_aware = true;         // no image is
  bool rt8 = false;               // an image uses an OKVFE_DIST_RADTAN8 slot
  bool counters_cleared = false;  // the upload zeroed d_cand_count / d_fix_count on the call's stream
};
struct CallPlan {  // (the default is a detect-only call's: nothing fused, no batch looked at)
  DescribeRoute route = DescribeRoute::kAllModes;
  int aware_extra_box = -1;       // what describe_route says of the samples beyond 64
  bool wide_boxes = false;        // pattern of box class 1
  bool rt8 = false;               // compact_kernel<true>
  bool fuse_setup = false;        // the call describes what it detects: the set-up rides in the selection kernel
  bool counters_cleared = false;  // BatchFacts::counters_cleared
};
// What a call's selection launch did for its extractor: nothing (describe_setup_kernel runs), the per-keypoint set-up into
// the *_tmp buffers, or the set-up with final slots assigned in d_kps / d_desc / d_count (DescribeSetup::kps_out: the
// descriptor kernel works in place and a back-projection kernel stands in for the compaction pass).
enum SetupDone : int { kSetupNone = 0, kSetupTmp = 1, kSetupFinal = 2 };

struct okvfe_ctx {
  okvfe_config cfg{};
  hipStream_t stream = nullptr;
  hipEvent_t heavy_done[2] = {nullptr, nullptr};  // okvfe_set_heavy_kernel_chaining: after the score / describe kernel
  int detected_images = 0;  // images covered by the last okvfe_detect_batch_device
  std::string err;
  int w = 0, h = 0, B = 0, kp_cap = 0, cand_cap = 0, ws_stride = 0;
  int occ_rows = 0, occ_cols = 0;
  size_t occ_image_bytes = 0;
  int mode_default = kUpright;
  Pattern host_pattern{};
  PatternFacts pattern_facts{};  // of host_pattern, refreshed wherever it changes

  std::vector<void*> allocs;
  int32_t* d_scores = nullptr;
  int32_t* d_virtual = nullptr;   // scale-space parent, OKVFE_SCORE_BRISK_SCALESPACE: FAST 5-8 map of layer 0
  // A device buffer PER STREAM an entry point was called on (stream_workspace): calls on one stream are ordered, calls on
  // different streams do not share a buffer.  map_perm: okvfe_match_to_map_blocks_device's keypoint order per frame
  // [frames][kp_cap]; map_table_ws: okvfe_match_to_map_table_blocks_device / okvfe_landmark_table_check_device and the
  // second pass, packed records, counts and keypoint order of a slice of frames
  struct StreamWorkspace {
    hipStream_t stream = nullptr;
    uint8_t* d = nullptr;
    size_t bytes = 0;
  };
  // place_refine_ws: okvfe_place_refine_blocks_device's per-multiframe records, evaluations and spare counts
  std::vector<StreamWorkspace> map_perm, map_table_ws, place_refine_ws;
  size_t map_table_ws_limit = (size_t)1 << 30;  // more than this per call: the frames go in slices
  ScoreLayout score_layout{0, 0};  // of d_scores: slotted where the fused score+NMS kernel applies
  ScoreLayout live_layout{0, 0};   // the layout the LAST score launch actually wrote (dense when the fused kernel refused the call)
  // Map-free detection (round 4): single-scale Harris calls whose selection kernel can recompute the nine
  // sub-pixel scores from the image write NO score map (okvfe_set_keep_score_map(ctx, 1) restores it).
  bool keep_score_map = false;
  bool layer_child = false;        // detect-only context of one scale-space layer: its map is read by the other layers
  bool map_free_live = false;      // the LAST detect call wrote no map: okvfe_device_outputs.scores is null
  const uint8_t* live_images = nullptr;  // images of the running detect call (map-free: read again by the selection)
  Candidate* d_cand = nullptr;
  int32_t* d_cand_count = nullptr;
  int32_t* d_fix_count = nullptr;  // flagged-record counts [B] and their lists [B][kFixListCap]: inside d_cand_count's
  int32_t* d_fix_list = nullptr;   // allocation (creation) -- separate names so that a lane view can offset them
  uint64_t* d_sort_ws = nullptr;
  uint8_t* d_occ = nullptr;
  float* d_lut = nullptr;
  Pattern* d_pattern = nullptr;
  PatternScales* d_scales = nullptr;  // scale_invariant extraction: the pattern at 64 scales
  okvfe_keypoint* d_kps_det = nullptr;
  int32_t* d_det_count = nullptr;
  okvfe_keypoint* d_kps_tmp = nullptr;
  uint8_t* d_desc_tmp = nullptr;
  uint8_t* d_valid_tmp = nullptr;
  okvfe_keypoint* d_kps = nullptr;
  uint8_t* d_desc = nullptr;
  double* d_bp = nullptr;
  uint8_t* d_bpv = nullptr;
  int32_t* d_count = nullptr;
  ImageParams* d_prm = nullptr;  // current slot of prm_ring
  DeviceCamera* d_cams = nullptr;
  const float** d_rays_ptrs = nullptr;
  const float** d_jac_ptrs = nullptr;
  uint8_t* d_img_stage = nullptr;
  okvfe_stereo_match* d_match_stage = nullptr;
  // Per-call host parameters (ImageParams per image, PairParams per stereo pair) travel through
  // rings of pinned host slots + device slots: the call fills a pinned slot, enqueues ONE async
  // copy on its stream and the kernels read the device slot -- no host synchronisation.  A slot is
  // reused only after the event recorded behind its last consumer has completed (normally long
  // ago; the wait only bites when more than kRingSlots calls are in flight).
  struct ParamRing {
    static constexpr int kRingSlots = 8;
    uint8_t* h = nullptr;  // pinned, kRingSlots * slot_bytes
    uint8_t* d = nullptr;
    size_t slot_bytes = 0;
    hipEvent_t done[kRingSlots] = {};
    bool pending[kRingSlots] = {};   // in use by work enqueued on `used_on`
    bool recorded[kRingSlots] = {};  // ... and done[slot] was recorded behind its last reader (ring_release)
    hipStream_t used_on[kRingSlots] = {};
    unsigned next = 0;
  };
  ParamRing prm_ring, pair_ring, cls_ring;
  int prm_slot = -1;  // slot d_prm points into

  // Lanes inside one call (round 6; okvfe_set_internal_lanes): a device-resident batch is cut into `internal_lanes`
  // slices, each run on a stream of the context's own -- the VALU-bound score kernel of one slice under the LDS- and
  // latency-bound selection / descriptor / matcher kernels of another (the camera-parallel shape of
  // okvis_multisensor_processing/src/ThreadedSlam.cpp:434-448, inside the call).  A lane is a VIEW: an okvfe_ctx
  // whose per-image pointers are this context's, offset to the slice (bind_lane, capi_detect.cpp); it owns a stream
  // and two events, nothing else.
  int internal_lanes = 0;  // 0 = the library's choice (not to cut: lanes_for_call), 1 = off, 2..8 = that many
  bool lane_view = false;
  okvfe_ctx* prof_owner = nullptr;  // lane view: stage timers record into the owning context
  hipEvent_t k1_wait = nullptr;     // lane view: its score kernel starts behind this event (the previous lane's k1_done)
  hipEvent_t k1_done = nullptr;     // ... and records this one behind itself
  std::vector<okvfe_ctx*> lane_ctx;
  std::vector<hipEvent_t> lane_done;
  hipEvent_t lane_fork = nullptr;
  // PIPELINED lanes (okvfe_set_internal_lanes(ctx, -k)): the call does not join its lanes onto the caller's stream; the
  // slices' chains -- and those of the okvfe_match_stereo_batch_device call that follows -- stay on the lane streams, so
  // lane l starts the next call's score kernel behind ITS OWN previous work and the lanes drift out of phase, as separate
  // contexts do.  The join happens when something needs the results: any other entry point of this context (the stream
  // it is given waits for `join_done`; host-side readers synchronise), or okvfe_lanes_join.
  bool lanes_pipelined = false;        // owner: internal_lanes was set negative
  // owner: pipelined lane work has been issued and the HOST has not yet waited for it.  Only lanes_join_host clears it: a
  // stream that waited for `join_done` orders that one stream, not the others, so every stream-taking entry point waits
  // again (pick_stream) for as long as the flag is set
  bool lanes_unsynced = false;
  // owner: the last detect + describe ran on pipelined lanes and no call of this context has been ordered behind them
  // since (pick_stream and lanes_join_host clear it): an okvfe_match_stereo_batch_device that follows may run on the
  // lane streams, each slice's pairs behind that slice's chain
  bool lanes_open = false;
  int lanes_used = 0;                  // owner: lanes of the pending call
  int lane_chunk = 0;                  // owner: images per lane of the pending call
  hipStream_t join_stream = nullptr;   // owner: waits for every lane, releases the parameter slots, records join_done
  hipEvent_t join_done = nullptr;

  // scale space (octaves > 0): one detect-only child context per layer (K1..K4 at the layer's
  // size), layer images for l >= 1 owned here; this (parent) context keeps the merged keypoints
  // and everything from the descriptor stage on
  bool child = false;
  int n_layers = 1;
  std::vector<okvfe_ctx*> layers;
  std::vector<uint8_t*> d_layer_img;
  // scale-space parent: the layers of a call run concurrently on the layer contexts' own streams (round 6) -- per layer
  // {image ready, score map + candidates ready, keypoints ready} and the fork of the call
  std::vector<hipEvent_t> layer_ev;
  hipEvent_t layer_fork = nullptr;
  std::vector<int> layer_w, layer_h;

  // host-fed batches (okvfe_detect_describe_batch_host): two device image buffers filled by an
  // internal copy stream, so the PCIe copy of batch k+1 runs under the kernels of batch k
  uint8_t* d_feed[2] = {nullptr, nullptr};
  hipStream_t feed_stream = nullptr;
  hipEvent_t feed_copied[2] = {nullptr, nullptr}, feed_consumed[2] = {nullptr, nullptr};
  bool feed_busy[2] = {false, false};
  unsigned feed_next = 0;
  std::vector<float*> cam_rays, cam_jac;  // device maps per camera slot (nullptr = not set)
  std::vector<float> cam_fu;
  std::vector<uint8_t> cam_wide;  // camera-aware patches of this camera often exceed the LDS buffer (describe_kernel<5>)
  // row norms (nx, ny) of the image Jacobian / fu at every 8th pixel, kept so that okvfe_set_pattern can re-derive
  // the two statistics; cam_aware_slow: more than a tenth of the camera's keypoints would have a patch of neither LDS
  // class of describe_aware_kernel (k_describe_aware.hip) -> such a camera keeps describe_kernel
  std::vector<std::vector<float>> cam_norms;
  std::vector<uint8_t> cam_aware_slow;
  std::vector<DeviceCamera> h_cams;
  std::vector<bool> cam_has_intrinsics;
  int last_n_images = 0;
  hipStream_t last_stream = nullptr;

  // scratch for the explicit-array matchers (grown on demand)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  uint8_t* h_pinned = nullptr;  // pinned staging for the host-buffer API: [image][keypoints in]
  void* h_pinned_dev = nullptr; // its device-visible address (the copy kernels read it in place)
  size_t h_pinned_bytes = 0;
  // single-image host-buffer API: ONE image's results land in this pinned block (export_result_kernel),
  // so a caller waiting for a frame pays one stream synchronisation
  uint8_t* h_result = nullptr;
  void* h_result_dev = nullptr;
  // okvfe_detect_ahead: the whole detect + describe chain ran for this image with this extraction
  // set-up; an okvfe_compute that asks for exactly that is answered from h_result
  struct Ahead {
    bool valid = false;
    const uint8_t* image = nullptr;
    size_t stride = 0;
    int32_t cam = -1;
    bool aware = false;
    float g[3] = {0.0f, 0.0f, 0.0f};
  } ahead;
  std::vector<uint8_t> ahead_shadow;  // the image okvfe_detect_ahead ran on (ordinary memory)

  // stage profiling (okvfe_profile_*): event pairs per recorded stage launch
  uint32_t prof_mask = 0;  // bit s = stage s is timed
  struct StageEvents {
    int stage;
    hipEvent_t a, b;
  };
  std::vector<StageEvents> prof_events;
  std::vector<hipEvent_t> event_pool;
};

namespace okvfe {

extern thread_local std::string g_create_error;  // message of a failed okvfe_create (no context yet)
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

okvfe_status fail(okvfe_ctx* ctx, okvfe_status st, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                  \
  do {                                                                                      \
    hipError_t e__ = (expr);                                                                \
    if (e__ != hipSuccess)                                                                  \
      return fail((ctx), e__ == hipErrorOutOfMemory ? OKVFE_ERR_OUT_OF_MEMORY               \
                                                    : OKVFE_ERR_DEVICE,                     \
                  "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

template <typename T>
okvfe_status dev_alloc(okvfe_ctx* ctx, T** p, size_t count) {
  void* q = nullptr;
  HIP_TRY(ctx, hipMalloc(&q, std::max<size_t>(count * sizeof(T), 256)));
  ctx->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return OKVFE_OK;
}

okvfe_status ensure_scratch(okvfe_ctx* ctx, size_t bytes);
okvfe_status ensure_pinned(okvfe_ctx* ctx, size_t bytes);
#pragma GCC visibility push(hidden)  // (the shared plumbing adds nothing to the library's dynamic symbols)
// One call on the caller's host arrays: the regions of a ScratchLayout in ctx->scratch, the copies in and out on stream
// s.  The pinned variant keeps the same layout in ctx->h_pinned: the inputs are staged there, ONE move brings [0, o_out)
// to the device and the result is read from the pinned block (okvfe_match_stereo says why).
class ScratchCall {
 public:
  ScratchCall(okvfe_ctx* ctx, hipStream_t s) : ctx_(ctx), s_(s) {}
  okvfe_status reserve(const ScratchLayout& L, bool pinned = false) {
    okvfe_status st = ensure_scratch(ctx_, L.total());
    if (st == OKVFE_OK && pinned) st = ensure_pinned(ctx_, L.total());
    base_ = static_cast<uint8_t*>(ctx_->scratch);
    return st;
  }
  template <typename T = uint8_t>
  T* dev(size_t o) const { return reinterpret_cast<T*>(base_ + o); }
  hipError_t up(size_t o, const void* src, size_t bytes) const {  // an empty array is no copy
    return bytes ? hipMemcpyAsync(base_ + o, src, bytes, hipMemcpyHostToDevice, s_) : hipSuccess;
  }
  hipError_t down(void* dst, size_t o, size_t bytes) const {
    return bytes ? hipMemcpyAsync(dst, base_ + o, bytes, hipMemcpyDeviceToHost, s_) : hipSuccess;
  }
  hipError_t sync() const { return hipStreamSynchronize(s_); }
  // ---- the pinned variant
  template <typename T = uint8_t>
  T* host(size_t o) const { return reinterpret_cast<T*>(ctx_->h_pinned + o); }
  void put(size_t o, const void* src, size_t bytes) const {
    if (bytes) std::memcpy(ctx_->h_pinned + o, src, bytes);
  }
  // every input at once: a kernel that reads the pinned block in place, or one copy where the block has no device address
  hipError_t move_in(size_t o_out) const {
    if (!ctx_->h_pinned_dev) return hipMemcpyAsync(base_, ctx_->h_pinned, o_out, hipMemcpyHostToDevice, s_);
    launch_param_copy(base_, ctx_->h_pinned_dev, o_out, nullptr, 0, s_);
    return hipSuccess;
  }
  // where the kernel writes its result: straight into the pinned block if the device sees it
  template <typename T>
  T* result(size_t o_out) const {
    return ctx_->h_pinned_dev ? reinterpret_cast<T*>(static_cast<uint8_t*>(ctx_->h_pinned_dev) + o_out) : dev<T>(o_out);
  }
  // the call's one synchronisation, and the result from the pinned block
  hipError_t fetch(void* dst, size_t o_out, size_t bytes) const {
    hipError_t e = hipSuccess;
    if (!ctx_->h_pinned_dev) e = hipMemcpyAsync(ctx_->h_pinned + o_out, base_ + o_out, bytes, hipMemcpyDeviceToHost, s_);
    if (e == hipSuccess) e = hipStreamSynchronize(s_);
    if (e == hipSuccess) std::memcpy(dst, ctx_->h_pinned + o_out, bytes);
    return e;
  }

 private:
  okvfe_ctx* ctx_;
  hipStream_t s_;
  uint8_t* base_ = nullptr;
};
#pragma GCC visibility pop
okvfe_status ring_reserve(okvfe_ctx* ctx, okvfe_ctx::ParamRing* r, size_t slot_bytes);
okvfe_status ring_upload(okvfe_ctx* ctx, okvfe_ctx::ParamRing* r, const void* src, size_t bytes, hipStream_t s,
                         void** d_out, int* slot_out, int32_t* zero_dev = nullptr, int n_zero = 0,
                         bool* zeroed = nullptr);
okvfe_status ring_release(okvfe_ctx* ctx, okvfe_ctx::ParamRing* r, int slot, hipStream_t s);
void ring_destroy(okvfe_ctx::ParamRing* r);
// One call's slot of pair_ring or cls_ring: filled by upload() on the call's stream and released behind the slot's last
// reader by release(), at most once.  A call that returns early leaves the release to the destructor, which keeps the
// error the call reports.
class RingSlot {
 public:
  RingSlot(okvfe_ctx* ctx, okvfe_ctx::ParamRing* ring, hipStream_t s) : ctx_(ctx), ring_(ring), s_(s) {}
  RingSlot(const RingSlot&) = delete;
  RingSlot& operator=(const RingSlot&) = delete;
  ~RingSlot() {
    if (slot_ < 0) return;
    std::string err = ctx_->err;
    (void)release();
    ctx_->err.swap(err);
  }
  okvfe_status upload(const void* src, size_t bytes) { return ring_upload(ctx_, ring_, src, bytes, s_, &d_, &slot_); }
  template <typename T>
  const T* as() const { return static_cast<const T*>(d_); }  // the device copy
  okvfe_status release() { return release(s_); }
  okvfe_status release(hipStream_t other) {  // the readers ran on another stream (pipelined lanes: the join stream)
    const int slot = slot_;
    slot_ = -1;
    return ring_release(ctx_, ring_, slot, other);
  }

 private:
  okvfe_ctx* ctx_;
  okvfe_ctx::ParamRing* ring_;
  hipStream_t s_;
  void* d_ = nullptr;
  int slot_ = -1;
};
// the workspace of stream s in `list`, at least max(bytes, 256) large and never shrunk.  At most eight streams keep one:
// the oldest entry is evicted after a device synchronisation (a launch may still read it), and growing frees the old
// buffer, which synchronises the device once
okvfe_status stream_workspace(okvfe_ctx* ctx, std::vector<okvfe_ctx::StreamWorkspace>* list, hipStream_t s, size_t bytes,
                              uint8_t** out);
// the intrinsics of camera slot `cam`; null when there is no such slot or okvfe_set_camera has not filled it
inline const DeviceCamera* slot_camera(const okvfe_ctx* ctx, int cam) {
  if (cam < 0 || cam >= (int)ctx->h_cams.size() || !(ctx->h_cams[cam].fu > 0.0)) return nullptr;
  return &ctx->h_cams[cam];
}
DeviceCamera to_device_camera(const okvfe_camera_ext& c);
okvfe_camera_ext widen_camera(const okvfe_camera& c);  // d_ext = 0
PairParams to_pair_params(const okvfe_stereo_pair& p);
double layer_keypoint_size(int l);
void fill_class_table(double* t, double f0, double f1, bool motion);
constexpr size_t kClassTableDoubles = 2 * kSizeClasses * kSizeClasses;
okvfe_status check_size_classes(okvfe_ctx* ctx, const okvfe_keypoint* kp, int n, bool* multi);
hipStream_t pick_stream(okvfe_ctx* ctx, void* stream);      // joins pending pipelined lanes onto the stream it returns
hipStream_t pick_stream_raw(okvfe_ctx* ctx, void* stream);  // no join (the lane-aware entry points)
okvfe_status lanes_join_host(okvfe_ctx* ctx);               // host-side join of pending pipelined lanes
// Mask size, disc and LDS of the coverage kernels (capi_keyframe.cpp): n_ids < 0 = no id table, else a table for up to
// n_ids ids (chunked beyond half of it); extra_lds bytes follow the masks.  OKVFE_ERR_UNSUPPORTED beyond the limits.
okvfe_status coverage_geometry(okvfe_ctx* ctx, const char* who, double kptrad, int64_t n_ids, size_t extra_lds,
                               CoverageGeometry* g);
// every (m, c), m < n_multiframes, c < n_cams, on a block m * stride_m + c * stride_c of its own, all within an int32
okvfe_status check_block_strides(okvfe_ctx* ctx, const char* who, int stride_m, int stride_c, int n_multiframes,
                                 int n_cams);
void layer_size(int w, int h, int l, int* lw, int* lh);
void layer_scale(int l, int* num, int* den);

// serialisation of the heavy kernels across the contexts of a process (okvfe_set_heavy_kernel_chaining)
constexpr int kMaxTokenDevices = 64;
extern std::mutex g_token_mutex;
extern hipEvent_t g_score_token[kMaxTokenDevices];
int score_token_mode();

// RAII-free stage timer: records an event pair around a launch when profiling is on
struct StageTimer {
  okvfe_ctx* ctx;
  hipStream_t s;
  int idx = -1;
  StageTimer(okvfe_ctx* c0, int stage, hipStream_t st) : ctx(c0->prof_owner ? c0->prof_owner : c0), s(st) {
    okvfe_ctx* c = ctx;
    if (!((c->prof_mask >> stage) & 1u) || c->prof_events.size() >= 65536) return;
    hipEvent_t e[2];
    for (int i = 0; i < 2; ++i) {
      if (!c->event_pool.empty()) {
        e[i] = c->event_pool.back();
        c->event_pool.pop_back();
      } else if (hipEventCreate(&e[i]) != hipSuccess) {
        return;
      }
    }
    c->prof_events.push_back({stage, e[0], e[1]});
    idx = (int)c->prof_events.size() - 1;
    (void)hipEventRecord(e[0], s);
  }
  ~StageTimer() {
    if (idx >= 0) (void)hipEventRecord(ctx->prof_events[idx].b, s);
  }
};

#pragma GCC visibility push(hidden)
// Who asks for a camera slot: the entry point's name (or none), what it calls the things that name a slot ("frame",
// "camera", "pair", or nothing) and the status of a slot without intrinsics.  They differ between the entry points for
// no recorded reason; each keeps its own until someone decides.
struct RigWho {
  const char* fn;
  const char* noun;
  okvfe_status bad = OKVFE_ERR_NOT_READY;
};
// the intrinsics of slot `cam`, named by the call's `index`-th frame / camera / pair; null if it has none: the message is
// set and the call returns who.bad
const DeviceCamera* rig_slot(okvfe_ctx* ctx, const RigWho& who, int index, int cam);
// The camera slots of a call, checked in order before anything is queued: fill(index, camera) builds the caller's record
// of each, *rt8 (if asked for) says whether one of them holds the 8-coefficient model.
template <typename Fill>
okvfe_status rig_slots(okvfe_ctx* ctx, const RigWho& who, int n, const int32_t* cam_ids, bool* rt8, Fill&& fill) {
  for (int c = 0; c < n; ++c) {
    const DeviceCamera* dc = rig_slot(ctx, who, c, cam_ids[c]);
    if (!dc) return who.bad;
    if (rt8) *rt8 = *rt8 || dc->distortion == OKVFE_DIST_RADTAN8;
    fill(c, *dc);
  }
  return OKVFE_OK;
}
// the end of a device-batch call whose launches read `slot`: the slot is released behind them
inline okvfe_status finish_call(okvfe_ctx* ctx, RingSlot* slot, hipStream_t s) {
  HIP_TRY(ctx, hipGetLastError());
  const okvfe_status rel = slot->release();
  ctx->last_stream = s;
  return rel;
}
// ... and the whole tail of one that uploads once and launches: the records through the pinned parameter ring (one
// asynchronous copy, no host synchronisation), launch(device records) under the stage's timer, finish_call
template <typename Rec, typename Launch>
okvfe_status ring_launch(okvfe_ctx* ctx, hipStream_t s, const std::vector<Rec>& recs, int stage, Launch&& launch) {
  RingSlot slot(ctx, &ctx->pair_ring, s);
  const okvfe_status st = slot.upload(recs.data(), recs.size() * sizeof(Rec));
  if (st != OKVFE_OK) return st;
  {
    StageTimer t(ctx, stage, s);
    launch(slot.as<Rec>());
  }
  return finish_call(ctx, &slot, s);
}
#pragma GCC visibility pop

// okvfe_match_to_map_table_blocks_device: frames per slice when a frame needs `per_frame` bytes of workspace and a call
// may hold `limit`: all of them if they fit, never fewer than one, never more than a launch's grid.y
inline int map_table_slice_frames(size_t per_frame, size_t limit, int n_frames) {
  const size_t fit = per_frame ? limit / per_frame : (size_t)n_frames;
  return (int)std::min<size_t>(std::max<size_t>(fit, 1), std::min<size_t>((size_t)std::max(n_frames, 1), 65535));
}

}  // namespace okvfe
