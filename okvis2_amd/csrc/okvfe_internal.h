// okvfe_internal.h -- shared declarations of the libokvfe.so runtime (host + HIP kernels).
// Product code; never includes or links anything under oracle/.
#pragma once
#include <cstddef>
#include <atomic>
#include <cstdlib>

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/okvfe.h"
#include "imu_dev.h"
#include "place_refine_dev.h"

namespace okvfe {

// Lab switches = the A/B knobs of the experiments recorded in LAB_NOTES.md.  The product library
// reads NO environment variable: lab_env() is a constant nullptr there, so every knob folds away at
// compile time.  `make lab` builds libokvfe_lab.so with -DOKVFE_LAB, where the knobs are live
// (tests/test_gpu_detector_paths.py loads that build for the tests that flip them).
#ifdef OKVFE_LAB
inline const char* lab_env(const char* name) { return std::getenv(name); }
#else
inline const char* lab_env(const char*) { return nullptr; }
#endif

// A function attribute (opt-in to > 64 KiB of dynamic LDS) belongs to the function ON THE CURRENT DEVICE: one process may
// hold contexts on several GPUs, so the one-shot is kept per device ordinal, thread-safe.
constexpr int kMaxAttrDevices = 64;
struct PerDeviceOnce {
  std::atomic<int> state[kMaxAttrDevices];  // 0 = not yet, 1 = being set, 2 = set
  template <typename F>
  void run(F&& f) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxAttrDevices) {
      f();  // (unknown ordinal: set it every time)
      return;
    }
    int expect = 0;
    if (state[dev].load(std::memory_order_acquire) == 2) return;
    if (state[dev].compare_exchange_strong(expect, 1)) {
      f();
      state[dev].store(2, std::memory_order_release);
    } else {
      while (state[dev].load(std::memory_order_acquire) != 2) {}  // another host thread is setting it right now
    }
  }
};



constexpr int kPatternPoints = 72;  // capacity (lane i and, past 64, a second sample on lane i - 64); built-in: 66
constexpr int kMaxLongPairs = 1100;
constexpr int kRot = 1024;

// BRISK2-style sampling pattern, host-built (host_tables.cpp), uploaded once per context.
struct Pattern {
  int32_t n_points;
  float px[kPatternPoints];
  float py[kPatternPoints];
  float sigma_half[kPatternPoints];
  int32_t n_short;
  uint8_t short_i[384], short_j[384];
  int32_t n_long;
  uint8_t long_i[kMaxLongPairs], long_j[kMaxLongPairs];
  int32_t long_wdx[kMaxLongPairs], long_wdy[kMaxLongPairs];
  int32_t border;
  int32_t rot_cos[kRot], rot_sin[kRot];
  float rot_cosf[kRot], rot_sinf[kRot];
  // per sample, constants of the box mean that depend on sigma_half only: scaling =
  // (int)(4194304 / (4 sigma^2)), scaling2 = (int)(scaling * 4 sigma^2 / 1024) (same float
  // sequence as the device code used per keypoint before they were tabulated)
  int32_t box_scaling[kPatternPoints], box_scaling2[kPatternPoints];
  // max_i |p_i| + sigma_half_i, rounded up: the patch geometry of describe_setup_one (describe_setup_dev.h)
  float reach;
  // describe_aware_kernel's per-lane constants in ONE 32-byte record (two 16-byte loads, no dependent look-ups in a
  // wave's prologue): lane l samples point extra + l (a lane without a point: point 0) -- {px, py, sigma_half (float
  // bits), box_scaling, box_scaling2, short pairs of words 0|1, 2|3, 4|5 (i | j << 8 each, two per dword)}
  int32_t aware_lane[64][8];
};
void fill_aware_lanes(Pattern* p);
void build_pattern(Pattern* p);
void scale_pattern_boxes(Pattern* p, float s);
float pattern_reach(const Pattern& p);
// What the descriptor kernels may assume of a pattern; computed where a pattern is installed (okvfe_create,
// okvfe_set_pattern) and kept next to it, so that no call walks the pattern.
struct PatternFacts {
  // 0: every box fits the fixed-trip slots of the fast descriptor kernels (first-pass samples 11 x 11: sigma_half <=
  // 4.75; second-pass samples = points 0 .. n - 65 of a pattern with more than 64 points, 5 x 5: sigma_half < 2.0);
  // 1: the slots of the WIDE instantiations (21 x 21: <= 9.75, 10 x 10: <= 4.25); 2: wider still, or a half-width
  // below 0.5 (k_describe.hip: kMaxBox / kSmallBox / kWideBox / kWideSmallBox)
  int32_t box_class = 0;
  // describe_rot_kernel takes the pattern: its circle fits a 64-byte row pitch, its samples beyond 64 lanes fit the
  // kernel's table, its long-pair weights fit 16 bits and its rotation tables follow the quarter-wave rule exactly
  bool rot_ok = false;
  int32_t extra = 0;  // samples beyond 64 lanes
};
PatternFacts pattern_facts(const Pattern& p);
// scale_invariant = true (Frontend.hpp:235-237): the published BRISK extractor keeps the pattern at 64
// scales spanning a factor of 30 and picks index max(int(64 / lb(30) * lb(size / 7.2) + 0.5), 0)
// (<= 63) from the keypoint's diameter; the fixed-scale extractor is index 17 of the same ladder.
// Scale i = the base pattern with offsets, box half-sides and reach times 2^((i - 17) lb(30) / 64).
constexpr int kPatternScales = 64;
constexpr int kBasicScale = 17;
struct PatternScales {
  float px[kPatternScales][kPatternPoints], py[kPatternScales][kPatternPoints];
  float sigma_half[kPatternScales][kPatternPoints];
  int32_t box_scaling[kPatternScales][kPatternPoints], box_scaling2[kPatternScales][kPatternPoints];
  int32_t border[kPatternScales];
  float size_from[kPatternScales];  // index(size) = #{i >= 1 : size >= size_from[i]} (bisected on the host formula)
};
int pattern_scale_index(float size);
void build_pattern_scales(const Pattern& base, PatternScales* out);
// d_lut layout: [0, 961) the 31x31 weights; from kStampTableOffset the compacted stamp, one
// {(ry << 8) | rx, weight} pair per non-zero cell (697 of them), padded to kStampSlots.
constexpr int kStampSlots = 704;
constexpr int kStampCells = 697;
constexpr int kStampTableOffset = 1024;
constexpr int kLutFloats = kStampTableOffset + 2 * kStampSlots;
void build_uniformity_lut(float lut[kLutFloats]);
// (the extended camera of ABI 8: every distortion type; okvfe_camera callers widen with d_ext = 0)
void build_awareness_maps(const okvfe_camera_ext& cam, float* rays_hw3, float* jac_hw6);
bool camera_overlap(const okvfe_camera_ext& cam, const okvfe_camera_ext& other, const double R_other_cam[9],
                    uint8_t* mask_hw);
bool host_backproject(const okvfe_camera_ext& cam, double px, double py, double dir[3]);

struct Candidate {  // NMS maximum
  int32_t x, y, score;
};
// set in Candidate::y by the fused score+NMS kernel: acceptance still depends on the raster-scan
// rule over a run of equal maxima, settled by nms_fixup_kernel
constexpr int32_t kCandidateFixupFlag = 0x40000000;
// the fused kernel also lists the positions of the flagged records, up to this many per image (more:
// nms_fixup_kernel scans the whole list)
constexpr int kFixListCap = 1024;

struct DeviceCamera {  // intrinsics for on-device back-projection
  double fu, fv, cu, cv;
  double one_over_fu, one_over_fv;
  double d[8];  // k1 k2 p1 p2 | k1 k2 k3 k4, then k3 k4 k5 k6 of OKVFE_DIST_RADTAN8 (zero otherwise)
  int32_t distortion;
  int32_t pad;
};

enum ExtractMode : int32_t { kUpright = 0, kGradient = 1, kCameraAware = 2 };

// per-image launch parameters of one batch (host-filled, uploaded per call)
struct ImageParams {
  int32_t cam;     // camera slot or -1
  int32_t mode;    // ExtractMode
  float dir[3];    // extraction direction
  float fu;
};

struct PairParams {  // one stereo pair on device
  int32_t image0, image1;
  double C0[9], r0[3], C1[9], r1[3];
  double f0, f1;
  double cos26, cos6;  // cos(2.6 sigma), cos(6 sigma) of size class (0, 0): keypoint size 12
  // scale space (octaves > 0): keypoint sizes are 12 * scale(layer) and sigma depends on the sizes
  // of the two keypoints; cls = device table [2][kSizeClasses][kSizeClasses] of cos(2.6 sigma) /
  // cos(6 sigma) indexed by the layers (= okvfe_keypoint::octave) of keypoint 0 and keypoint 1,
  // or null when every keypoint has size 12
  const double* cls;
};
constexpr int kSizeClasses = 8;
// okvfe_match_motion_stereo_blocks_batch_device: one pair's record in the parameter block (host-filled, one upload per call)
struct MotionPairRecord {
  PairParams pair;  // poses, f0 = f1 = 0.5 (fu + fv) of the slot, cls = the slot's size-class table or null
  int32_t cam;      // camera slot
  int32_t idx0;     // older block (frame 0) in blocks0
  int32_t idx1;     // current block (frame 1) in blocks1; also the row of matched1 / matched1_out
  int32_t pad;
};
static_assert(sizeof(MotionPairRecord) == 256, "PairParams (240 bytes) and four int32");
// (the owner table of motion_claim_kernel, 4 bytes per keypoint slot, within 48 KB of LDS)
constexpr int kMotionClaimMaxKeypoints = 12288;

// okvfe_match_to_map_table_blocks_device: one frame's record in the parameter block (host-filled, one upload per call)
struct MapFrameParams {
  okvfe_pose T1;  // T_WC1 of the frame
  double cos10;   // cos(10 / (fu + fv)) of the frame's camera slot (Frontend.cpp:1213-1215)
  int32_t cam;    // camera slot
  int32_t pad;
};
// ... and its workspace record per (frame, landmark): written unpacked by prepare_landmarks_frames_kernel (index -1 =
// not a 3-D landmark), packed in place to the frame's 3-D landmarks in table order by pack_landmarks_frames_kernel
struct MapPacked {
  double px, py;        // projection into the frame
  int32_t index;        // landmark row of the table
  int32_t row0, row1;   // observation rows of the pooled descriptors (row1 = -1: one descriptor)
  int32_t pad;
};
static_assert(sizeof(MapPacked) == 32 && offsetof(MapPacked, index) == 16, "two 16-byte halves, index first in the second");
// okvfe_match_to_map_table_uninitialised_blocks_device: its workspace record per status-2 landmark of a frame, written
// packed in table order by pack_uninit_frames_kernel
struct MapUninitPacked {
  int32_t index;       // landmark row of the table
  int32_t row0, row1;  // observation rows of the pooled descriptors (row1 = -1: one descriptor)
  int32_t pad;
};
static_assert(sizeof(MapUninitPacked) == 16, "one 16-byte store");
// okvfe_ransac3d2d_consensus_blocks_device: one camera of the rig in the parameter block (host-filled, one upload per call)
struct RansacCamParams {
  double C[9], r[3];  // T_SC: p_S = C p_C + r
  double fu;          // of the camera slot (FrameNoncentralAbsoluteAdapter.cpp:73-100)
  int32_t cam;        // camera slot
  int32_t pad;
};
static_assert(sizeof(RansacCamParams) == 112, "112 bytes per camera");
// okvfe_stereo_insert_blocks_device: the kernel's arguments, passed by value.  cam_slots (n_cams int32) and poses
// (n_multiframes x n_cams, T_WC) lie in the parameter block of the call; every other pointer is the caller's device memory.
constexpr int kStereoInsertMaxCams = 32;          // every camera of OKVFE_STEREO_MAX_PAIRS pairs
constexpr size_t kStereoInsertMaxLds = 64 * 1024 - 256;  // dynamic LDS of one work-group (ids, overlay, the pair's tables) beside its static words
struct StereoInsertArgs {
  const double* hp_W;
  const uint8_t* initialised;
  const uint8_t* blocks;
  const DeviceCamera* cameras;
  const int32_t* cam_slots;
  const okvfe_pose* poses;
  const okvfe_stereo_match* matches;
  const int32_t* landmark;
  const uint8_t* as_keyframe;
  uint8_t* action;
  int32_t* lm;
  int32_t* landmark_out;
  int32_t* counts;
  size_t block_bytes;
  int32_t n_landmarks, n_multiframes, n_cams, n_pairs, kp_cap, w, h, o_count, o_kps, stride_m, stride_c, ov_log2, kh_log2;
  int8_t pair_c0[OKVFE_STEREO_MAX_PAIRS], pair_c1[OKVFE_STEREO_MAX_PAIRS];
};

// Layout of a context's int32 score map in HBM.
//   dense   (strips <= 1): pixel (x, y) at y * pitch + x, pitch == w;
//   slotted (strips >= 2): what the fused score+NMS kernel (k_harris.hip) writes.  A wave of that
//     kernel owns a strip of 62 dwords-of-pixels (quads) of a row plus one halo lane on either side;
//     in the slotted layout every strip has a 1024-byte slot of its own in the row and ALL 64 lanes
//     store, so that each store instruction writes eight whole 128-byte lines (partial-line stores
//     cost the memory system as much as whole lines: profiles/round2_k1_store_pattern.txt).  Quad
//     d = x >> 2 belongs to strip s(d) = d <= 62 ? 0 : min((d - 1) / 62, strips - 1) and sits at
//     column x + 8 * s(d); the 2 * s quads in between are pad (halo-lane values, never read).
//     pitch = 4 * (w / 4 + 2 * (strips - 1)) rounded up to 32 ints (128 bytes).
struct ScoreLayout {
  int32_t pitch;   // ints per row
  int32_t strips;  // 0 / 1 = dense
};
__host__ __device__ inline int score_col(const ScoreLayout& L, int x) {
  if (L.strips <= 1) return x;
  const int d = x >> 2;
  int s = d <= 62 ? 0 : (d - 1) / 62;
  s = s > L.strips - 1 ? L.strips - 1 : s;
  return x + 8 * s;
}
__host__ __device__ inline size_t score_index(const ScoreLayout& L, int x, int y) {
  return (size_t)y * (size_t)L.pitch + (size_t)score_col(L, x);
}

}  // namespace okvfe

// XCD-aware tile mapping (device): the dispatcher is observed to place linear workgroup id L on
// XCD L % 8 (used for speed only, never for correctness).  All tiles of one image are handed to
// ONE XCD, so row halos and the cache lines shared by neighbouring strips are served by that
// XCD's L2 instead of being fetched from HBM once per XCD.  1-D grid of n_images * tiles blocks.
#ifdef __HIPCC__
__device__ __forceinline__ void xcd_tile(int tiles, int n_images, int* image, int* tile) {
  const int L = blockIdx.x;
  const int n8 = n_images & ~7;
  const int full = n8 * tiles;
  if (L < full) {
    const int xcd = L & 7, slot = L >> 3;
    const int g = slot / tiles;
    *image = g * 8 + xcd;
    *tile = slot - g * tiles;
  } else {
    const int r = L - full;
    const int i = r / tiles;
    *image = n8 + i;
    *tile = r - i * tiles;
  }
}
#endif

// ---- kernel launchers (defined in the .hip files) ----------------------------------------------
namespace okvfe {

// The order of the 3- and 4-term FP64 sums (fp64_ops.h, okvfe_set_fp64_reduction).  k_match.hip and k_map.hip read a
// device symbol each (no relocatable device code: one symbol cannot serve both); false: the symbol write failed.
bool set_fp64_tree_match(int tree);
bool set_fp64_tree_map(int tree);
// Every other kernel takes the order as a template argument, and its launcher picks the instantiation from ONE host flag
// per device ordinal (capi_context.cpp): 0 = Eigen's order (the default), 1 = left to right.
int current_device_slot();   // the current device's ordinal; 0 where it is unknown or beyond kMaxAttrDevices
bool fp64_left_to_right();   // the flag of the current device
void set_fp64_left_to_right(bool ltr);  // (the caller has set and drained the device)
void launch_bow_query_l1(const int32_t* db_begin, const int32_t* db_ids, const double* db_values, int n_entries,
                         const int32_t* q_ids, const double* q_values, int n_q, double* scores,
                         hipStream_t stream);
void launch_agast_score(const uint8_t* img, int w, int h, int n_images, int32_t* score,
                        hipStream_t stream);
void launch_fast58_score(const uint8_t* img, int w, int h, int n_images, int32_t* score, hipStream_t stream);
void launch_brisk_refine(const int32_t* score, int w, int h, int n_images, int cand_cap, const int32_t* cand_count,
                         const uint64_t* sort_ws, int max_kpts, const int32_t* below, int wb, int hb, int rn_b,
                         int rd_b, const int32_t* above, int wa, int ha, int rn_a, int rd_a, double rb, double ra, double lo,
                         okvfe_keypoint* kps, int kp_cap, int32_t* kp_count, hipStream_t stream);
void launch_harris(const uint8_t* img, int w, int h, int n_images, int32_t* score,
                   hipStream_t stream);
// Score map and NMS candidates in one pass (k_harris.hip); false = not applicable (unaligned
// width, >32 rows per wave): the caller then runs launch_harris + launch_nms.  Must be followed by
// launch_nms_fixup.
bool launch_harris_nms(const uint8_t* img, int w, int h, int n_images, int32_t* score,
                       ScoreLayout layout, int abs_threshold, Candidate* cand, int cand_cap,
                       int32_t* cand_count, int32_t* fix_count, int32_t* fix_list, hipStream_t stream,
                       bool store_map = true);
void launch_param_copy(void* dst_dev, const void* src_host_mapped, size_t bytes, int32_t* zero_dev, int n_zero,
                       hipStream_t stream, int32_t* poke_dev = nullptr, int32_t poke_value = 0);
// one image's results -> one block of pinned host memory (k_util.hip); null sources are skipped
struct ResultSrc {
  const int32_t* count;          // [B] final keypoint counts
  const okvfe_keypoint* kps;     // [B][kp_cap]
  const uint8_t* desc;           // [B][kp_cap][48]
  const double* bp;              // [B][kp_cap][3]
  const uint8_t* bpv;            // [B][kp_cap]
  const int32_t* det_count;      // [B] detector's counts
  const okvfe_keypoint* det_kps; // [B][kp_cap]
  const int32_t* cand_count;     // [B] NMS maxima found (may exceed the capacity)
};
struct ResultLayout {  // byte offsets inside the host block: header {n, candidates, detected, 0}
  int32_t o_count, o_kps, o_desc, o_bp, o_bpv, o_det, total;
};
void launch_export_result(const ResultSrc& src, int index, int kp_cap, const ResultLayout& layout,
                          void* dst_host_mapped, hipStream_t stream);
bool launch_harris_byte_mover(const uint8_t* img, int w, int h, int n_images, int32_t* score,
                              ScoreLayout layout, hipStream_t stream);
// the layout launch_harris_nms writes for w x h images (dense when the fused kernel does not apply)
ScoreLayout harris_nms_layout(int w, int h);
void launch_nms_fixup(const int32_t* score, ScoreLayout layout, int w, int h, int n_images,
                      int abs_threshold, Candidate* cand, int cand_cap, int32_t* cand_count,
                      const int32_t* fix_count, const int32_t* fix_list, hipStream_t stream, bool map_free = false,
                      int32_t* idle_score_buffer = nullptr);
void launch_nms(const int32_t* score, int w, int h, int n_images, int abs_threshold,
                Candidate* cand, int cand_cap, int32_t* cand_count, hipStream_t stream);
void launch_sort(const Candidate* cand, int cand_cap, const int32_t* cand_count, int n_images,
                 float radius, uint64_t* sort_ws, hipStream_t stream);
// per-keypoint preparation of the extractor (describe_setup_dev.h), optionally run by the selection kernel
struct DescribeSetup {  // pat == nullptr: not requested
  const Pattern* pat;
  const ImageParams* prm;
  const float* const* rays;
  const float* const* jac;
  okvfe_keypoint* kps_tmp;
  uint8_t* desc_tmp;
  uint8_t* valid_tmp;
  const PatternScales* scales;
  // describe_aware_kernel's inputs (k_describe_aware.hip): the set-up thread also evaluates the pattern's samples
  // beyond 64 ("extra", <= kAwareMaxExtra of them) from `images` -- boxes of at most extra_box + 1 pixels a side
  // (4 or 9); 0 = not wanted (the call will run describe_kernel)
  const uint8_t* images = nullptr;
  int extra_box = 0;
  // FINAL SLOTS (set for a fused call on the batched camera-aware route whose selection runs in select_lazy_kernel,
  // null otherwise): the selection tail decides validity completely, counts the survivors in order and writes each one's
  // record to kps_out and its M / patch geometry / extra samples to its slot of desc_out -- the call's output buffers --
  // and the number valid to count_out; describe_aware_kernel<.., true> then works in place and no compaction pass runs.
  // kps_tmp / desc_tmp / valid_tmp stay unwritten.
  okvfe_keypoint* kps_out = nullptr;
  uint8_t* desc_out = nullptr;
  int32_t* count_out = nullptr;
};
constexpr int kAwareMaxExtra = 6;  // ints that fit the descriptor slot behind M (16 B) and the patch geometry (8 B)
// cells of the occupancy grid of a w x h image at a uniformity radius (> 0): 15 cells per radius, a stamp's reach of
// border (what a context allocates and hands to launch_select as occ_rows x occ_cols)
inline void occupancy_grid_dims(int w, int h, float radius, int* rows, int* cols) {
  const float scaling = (float)(15.0 / (double)radius);
  *rows = (int)((float)(h - 1) * scaling + 16.0f) + 17;
  *cols = (int)((float)(w - 1) * scaling + 16.0f) + 17;
}
// true: launch_select orders the candidates itself for this configuration (array-bin lazy selection): the
// caller launches no sort before it
bool select_sorts_candidates(float radius, int max_kpts, int kp_cap, const uint8_t* occupancy, size_t occ_image_bytes,
                             int occ_rows, int occ_cols);
// grid fall-backs of launch_select (k_select_grid.hip)
void launch_select_grid(const int32_t* score, ScoreLayout layout, int w, int h, int n_images, Candidate* cand,
                        int cand_cap, const int32_t* cand_count, float radius, int max_kpts, const float* lut,
                        uint8_t* occupancy, size_t occ_image_bytes, int occ_rows, int occ_cols, okvfe_keypoint* kps,
                        int kp_cap, int32_t* kp_count, uint64_t* sort_ws, hipStream_t stream);
bool launch_select(const int32_t* score, ScoreLayout layout, int w, int h, int n_images, Candidate* cand,
                   int cand_cap, const int32_t* cand_count, float radius, int max_kpts,
                   const float* lut, uint8_t* occupancy, size_t occ_pitch_bytes, int occ_rows,
                   int occ_cols, okvfe_keypoint* kps, int kp_cap, int32_t* kp_count,
                   uint64_t* sort_ws, hipStream_t stream, const DescribeSetup* setup = nullptr,
                   const uint8_t* images = nullptr);  // images != null: map-free call, see select_recomputes_scores
bool select_recomputes_scores(float radius, int max_kpts, int kp_cap, const uint8_t* occupancy, size_t occ_image_bytes,
                              int occ_rows, int occ_cols);
// true: launch_select runs select_lazy_kernel for this configuration, whose tail can assign final slots
// (DescribeSetup::kps_out); select_list_kernel and the grid kernels keep the *_tmp hand-over
bool select_assigns_final_slots(float radius, int max_kpts, int kp_cap, const uint8_t* occupancy, size_t occ_image_bytes,
                                int occ_rows, int occ_cols);
// Which descriptor kernel serves a call, one value per form launch_describe can launch: describe_aware_kernel (every
// image camera-aware, extra samples batched), describe_rot_kernel (no image camera-aware), describe_kernel<4, true, true>,
// <4, false, true>, <4, false, false> (all modes), <5, true, false>, <6, true, false>
enum class DescribeRoute : int32_t { kAwareBatched, kRot, kAwareWideBoxes, kWideBoxes, kAllModes, kAware5, kAware6 };
// Everything the choice depends on, as plain numbers (no pointer, no HIP type): the batch (upload_image_params), the
// installed pattern (PatternFacts), the context and the alignment of the call's image pointer.
struct RouteFacts {
  bool all_aware, none_aware, aware_fast, wide_patches;  // of the images of the batch
  int32_t box_class;
  bool rot_ok;
  int32_t extra;
  bool scale_invariant;  // the context extracts with the pattern at 64 scales (d_scales)
  int32_t n_layers, w, h;
  bool aligned;  // the call's image pointer is a multiple of 4
};
// *aware_extra_box = -1: the batched camera-aware kernel cannot serve the call; otherwise (samples beyond 64) << 8 |
// their largest box side minus one (0: no such samples).  Its low byte is what the set-up (describe_setup_kernel or the
// selection kernel's fused set-up) is told, whichever route serves the call.
DescribeRoute describe_route(const RouteFacts& f, int* aware_extra_box);
// setup_done: the selection kernel has prepared the per-keypoint inputs (detection and description in one call);
// wide_boxes: the pattern is of box class 1 (the WIDE slots of describe_aware_kernel);
// final_slots (route kAwareBatched with setup_done only): the selection tail assigned final slots -- kps_in /
// kp_count_in / desc_tmp are the call's output buffers, valid_tmp is not touched
void launch_describe(const uint8_t* img, int w, int h, int n_images, const Pattern* pat,
                     const ImageParams* prm, const float* const* rays, const float* const* jac,
                     const okvfe_keypoint* kps_in, int kp_cap, const int32_t* kp_count_in,
                     okvfe_keypoint* kps_tmp, uint8_t* desc_tmp, uint8_t* valid_tmp,
                     const PatternScales* scales, hipStream_t stream, bool setup_done, DescribeRoute route,
                     bool wide_boxes, int aware_extra_box, bool final_slots = false);
bool describe_patch_fits(float nx, float ny, int border);
// k_describe_aware.hip: the camera-aware-only extractor with batched extra samples (round 6)
int describe_aware_patch_class(float nx, float ny, float reach);
void launch_describe_aware(const uint8_t* img, int w, int h, int n_images, const Pattern* pat,
                           const okvfe_keypoint* kps_in, int kp_cap, const int32_t* kp_count_in, uint8_t* desc_tmp,
                           uint8_t* valid_tmp, bool wide_boxes, hipStream_t stream, bool final_slots);
// Quarter-wave lookup of the pattern's 1024-step rotation tables: sin(k) = +-Q[r or 256 - r] with Q = the first 257
// entries of the sine table, cos(k) = sin(k + 256).  describe_rot_kernel keeps Q (ints and floats, 2 KB) in LDS instead
// of gathering from the 16 KB of global tables inside every keypoint's chain; the host verifies once per pattern that the
// rule reproduces all 4096 table entries bit for bit (pattern_facts, host_tables.cpp) and keeps the all-modes kernel
// otherwise.
template <typename V>
__host__ __device__ inline V quarter_sin(const V* Q, int k) {
  k &= 1023;
  const int r = k & 255, q = k >> 8;
  const V v = (q & 1) ? Q[256 - r] : Q[r];
  return (q & 2) ? -v : v;
}
template <typename V>
__host__ __device__ inline V quarter_cos(const V* Q, int k) { return quarter_sin(Q, k + 256); }
void launch_describe_rot(const uint8_t* img, int w, int h, int n_images, const Pattern* pat, const ImageParams* prm,
                         const okvfe_keypoint* kps_in, int kp_cap, const int32_t* kp_count_in, okvfe_keypoint* kps_tmp,
                         uint8_t* desc_tmp, uint8_t* valid_tmp, hipStream_t stream);
void launch_compact(int n_images, const DeviceCamera* cams, const ImageParams* prm,
                    const okvfe_keypoint* kps_tmp, const uint8_t* desc_tmp,
                    const uint8_t* valid_tmp, const int32_t* kp_count_in, int kp_cap,
                    okvfe_keypoint* kps, uint8_t* desc, double* bp, uint8_t* bpv,
                    int32_t* kp_count, hipStream_t stream, bool rt8 = false);
// back-projection of keypoints that already sit in their final slots (DescribeSetup::kps_out): one thread per keypoint
void launch_backproject(int n_images, const DeviceCamera* cams, const ImageParams* prm, const okvfe_keypoint* kps,
                        const int32_t* kp_count, int kp_cap, double* bp, uint8_t* bpv, hipStream_t stream, bool rt8);
void launch_match_stereo(const PairParams* pairs, int n_pairs, const okvfe_keypoint* kps,
                         const uint8_t* desc, const double* bp, const uint8_t* bpv,
                         const int32_t* counts, int kp_cap, int threshold,
                         okvfe_stereo_match* out, hipStream_t stream);
void launch_match_stereo_arrays(const PairParams* pair, const uint8_t* desc0, const double* bp0,
                                const uint8_t* bpv0, const int32_t* n0p, int n0,
                                const uint8_t* desc1, const double* bp1, const uint8_t* bpv1,
                                const int32_t* n1p, int n1, int max_rows, int threshold,
                                okvfe_stereo_match* out, hipStream_t stream,
                                const okvfe_keypoint* kp0 = nullptr, const okvfe_keypoint* kp1 = nullptr);
void launch_match_motion(const PairParams* pair, const DeviceCamera* camera, int w, int h,
                         const uint8_t* desc0, const okvfe_keypoint* kp0, const double* bp0,
                         const uint8_t* bpv0, const uint8_t* skip0, int n0, const uint8_t* desc1,
                         const okvfe_keypoint* kp1, const double* bp1, const uint8_t* bpv1,
                         const uint8_t* matched1, int n1, int threshold, okvfe_motion_match* out,
                         hipStream_t stream, bool rt8 = false);
void launch_match_to_map(const uint8_t* desc_k, const okvfe_keypoint* kps, const uint8_t* use, int n_k,
                         const double* projections, const int32_t* desc_begin, int n_lm,
                         const uint8_t* pool, double thr_sq, int threshold, int32_t* best_lm,
                         int32_t* best_d, hipStream_t stream);
void launch_match_to_map_uninit(const PairParams* pair, const uint8_t* desc_k, const double* bp,
                                const uint8_t* use, const int32_t* previous, int n_k,
                                const int32_t* desc_begin, int n_lm, const uint8_t* pool,
                                const double* e0_W, const double* r0_W, int threshold,
                                int32_t* best_lm, int32_t* best_d, double* hps_W, uint8_t* hp_set,
                                int32_t* ctr_total, hipStream_t stream);
// gather block = what travels between GPUs and what the device-resident matchers read: byte offsets of its parts
struct BlockLayout {
  size_t o_count, o_kps, o_desc, o_bp, o_bpv, total;
};
BlockLayout block_layout(int kp_cap);  // capi_context.cpp
// device-resident batches of the map matchers (frame f reads gather block f; k_match.hip, MapBatch)
void launch_match_to_map_blocks(const BlockLayout& L, const uint8_t* blocks, int n_frames, int kp_cap,
                                const uint8_t* use, const double* projections, size_t proj_stride,
                                const int32_t* desc_begin, int n_lm, const uint8_t* pool, double thr_sq,
                                int threshold, int32_t* best_lm, int32_t* best_d, int32_t* perm_ws,
                                hipStream_t stream);
void launch_match_to_map_uninit_blocks(const PairParams* pairs, const BlockLayout& L, const uint8_t* blocks,
                                       int n_frames, int kp_cap, const uint8_t* use, const int32_t* previous,
                                       const int32_t* desc_begin, int n_lm, const uint8_t* pool,
                                       const double* e0_W, const double* r0_W, int threshold, int32_t* best_lm,
                                       int32_t* best_d, double* hps_W, uint8_t* hp_set, int32_t* ctr_total,
                                       hipStream_t stream);
void launch_verify_place_blocks(const uint8_t* pool, const int32_t* desc_begin, int n_landmarks, const BlockLayout& L,
                                const uint8_t* blocks, int n_frames, int kp_cap, uint32_t threshold,
                                int32_t* k_min, uint32_t* dist_min, hipStream_t stream);
void launch_pack_blocks(const BlockLayout& L, int first, int n, int kp_cap, const int32_t* counts,
                        const okvfe_keypoint* kps, const uint8_t* desc, const double* bp,
                        const uint8_t* bpv, uint8_t* blocks, hipStream_t stream);
void launch_match_motion_blocks(const PairParams& pair, const DeviceCamera* camera, int w, int h,
                                const BlockLayout& L, const uint8_t* block0, const uint8_t* block1,
                                const uint8_t* skip0, const uint8_t* matched1, int kp_cap,
                                int threshold, okvfe_motion_match* out, hipStream_t stream, bool rt8 = false);
// n_pairs (older block, current block, slot) pairs in one launch; skip0 [n_pairs][kp_cap], matched1 [n_blocks1][kp_cap]
void launch_match_motion_pairs(const MotionPairRecord* recs, int n_pairs, const DeviceCamera* cams, int w, int h,
                               const BlockLayout& L, const uint8_t* blocks0, const uint8_t* blocks1,
                               const uint8_t* skip0, const uint8_t* matched1, int kp_cap, int threshold,
                               okvfe_motion_match* out, hipStream_t stream, bool rt8);
// ... and the frame-data part of the insertion loop on its rows (kp_cap <= kMotionClaimMaxKeypoints)
void launch_motion_claim(const MotionPairRecord* recs, int n_pairs, const BlockLayout& L, const uint8_t* blocks0,
                         int kp_cap, const okvfe_motion_match* matches, uint8_t* claimed, int32_t* n_claimed,
                         uint8_t* matched1_out, hipStream_t stream);
void launch_match_stereo_blocks(const PairParams& pair, const BlockLayout& L, const uint8_t* blocks0,
                                const uint8_t* blocks1, int n_frames, int kp_cap, int threshold,
                                okvfe_stereo_match* out, hipStream_t stream);
void launch_verify_place(const uint8_t* pool, const int32_t* desc_begin, int n_landmarks,
                         const uint8_t* frame_desc, int K, uint32_t threshold, int32_t* k_min,
                         uint32_t* dist_min, hipStream_t stream);
void launch_voc_transform(const uint8_t* desc, int n, const uint8_t* node_desc, int n_nodes,
                          const int32_t* child_begin, const int32_t* child_index, const int32_t* word,
                          int32_t* word_out, int32_t* node_out, hipStream_t stream);
// matchToMap preparation (k_map.hip)
void launch_prepare_landmarks(const double* hp_W, const double* quality, const int32_t* obs_begin,
                              int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                              const okvfe_pose* poses, const okvfe_pose& T_WC1, const DeviceCamera* camera,
                              int w, int h, double repr, int exclusive, double cos10, double cos06,
                              int32_t* status, int32_t* n_desc, int32_t* obs_rows, double* projection,
                              double* e_W, double* r_W, hipStream_t stream, bool rt8 = false);
void launch_compact_landmarks(const int32_t* status, const int32_t* n_desc, const int32_t* obs_rows,
                              const double* projection, const uint8_t* obs_desc, int n_landmarks, int want,
                              int32_t* index_out, double* proj_out, int32_t* begin_out, uint8_t* pool_out,
                              int32_t* n_out, hipStream_t stream);
void launch_prepare_landmarks_frames(const double* hp_W, const double* quality, const int32_t* obs_begin,
                                     int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                                     const okvfe_pose* poses, const MapFrameParams* frames, int n_frames,
                                     const DeviceCamera* cameras, int w, int h, double repr, int exclusive,
                                     double cos06, int32_t* status, int32_t* n_desc, int32_t* obs_rows,
                                     double* projection, double* e_W, double* r_W, MapPacked* packed,
                                     int32_t* counts, hipStream_t stream, bool rt8);
void launch_check_landmark_table(const int32_t* obs_begin, int n_landmarks, const int32_t* obs_pose,
                                 int n_observations, int n_poses, uint32_t* bad, hipStream_t stream);
// the matcher on the frames' packed records (k_match.hip, match_to_map_table_kernel)
void launch_match_to_map_table_blocks(const BlockLayout& L, const uint8_t* blocks, int n_frames, int kp_cap,
                                      const uint8_t* use, const MapPacked* packed, const int32_t* counts,
                                      int n_landmarks, const uint8_t* obs_desc, double thr_sq, int threshold,
                                      int32_t* best_lm, int32_t* best_d, int32_t* perm_ws, hipStream_t stream);
// the second pass on the frames' status-2 landmarks (k_map.hip, pack_uninit_frames_kernel; k_match.hip,
// match_to_map_table_uninit_kernel)
void launch_pack_uninit_frames(const int32_t* status, const int32_t* n_desc, const int32_t* obs_rows, int n_landmarks,
                               int n_frames, MapUninitPacked* packed, int32_t* counts, hipStream_t stream);
void launch_match_to_map_table_uninit_blocks(const PairParams* pairs, const BlockLayout& L, const uint8_t* blocks,
                                             int n_frames, int kp_cap, const uint8_t* use, const int32_t* previous,
                                             int exclusive, const MapUninitPacked* packed, const int32_t* counts,
                                             int n_landmarks, const uint8_t* obs_desc, const double* e_W,
                                             const double* r_W, int threshold, int32_t* best_lm, int32_t* best_d,
                                             double* hps_W, uint8_t* hp_set, int32_t* ctr_total, hipStream_t stream);
// Frontend::removeOutliers for a batch of frames (k_map.hip, remove_outliers_frames_kernel); kept is zeroed by the caller
void launch_remove_outliers_frames(const double* hp_W, int n_landmarks, const MapFrameParams* frames, int n_frames,
                                   const DeviceCamera* cameras, int w, int h, const BlockLayout& L, const uint8_t* blocks,
                                   int kp_cap, double max_error, const int32_t* landmark, int32_t* landmark_out,
                                   int32_t* kept, hipStream_t stream, bool rt8);
// matchStereo's landmark bookkeeping for a batch of multiframes (k_map.hip, stereo_insert_kernel); the LDS one work-group
// needs, and the sizes (log2) of its two open-addressed tables
size_t stereo_insert_lds_bytes(int n_cams, int kp_cap, int* ov_log2, int* kh_log2);
void launch_stereo_insert(const StereoInsertArgs& args, size_t lds_bytes, hipStream_t stream, bool rt8);
// the consensus step of runRansac3d2d for a batch of multiframes (k_ransac.hip)
void launch_ransac_consensus(const double* hp_W, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L,
                             const uint8_t* blocks, int n_multiframes, int n_cams, int kp_cap,
                             const RansacCamParams* cams, const int32_t* landmark, const double* hypotheses,
                             const uint8_t* hyp_valid, int n_hyp, double threshold, int remove_outliers,
                             const okvfe_ransac_result_device& out, hipStream_t stream);
// the pose hypotheses of both consensus calls (k_ransac_hyp.hip, a part of k_ransac.hip's translation unit): sampler,
// P3P, the choice by the fourth sample
bool p3p_hypothesis_host(bool tree, const double* points, const double* bearings, double sigma, const double* C_SC,
                         const double* r_SC, double* hypothesis, int* n_solutions);
size_t ransac_hypotheses_lds_bytes(int n_cams, int kp_cap);
bool ransac_hypotheses_fits(int n_cams, int kp_cap);
void launch_ransac_hypotheses(const double* hp_W, const int32_t* obs_begin, int n_landmarks, const BlockLayout& L,
                              const uint8_t* blocks, int n_multiframes, int n_cams, int kp_cap, const RansacCamParams* cams,
                              const int32_t* landmark, const uint64_t* keys, uint64_t seed, int n_hyp,
                              const okvfe_ransac_hypotheses_device& out, hipStream_t stream);
void launch_place_hypotheses(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks,
                             int n_multiframes, int n_cams, int kp_cap, const RansacCamParams* cams,
                             const int32_t* match_landmark, const uint8_t* gate, const uint64_t* keys, uint64_t seed,
                             int n_hyp, const okvfe_ransac_hypotheses_device& out, hipStream_t stream);
int ransac_chunk_records();  // correspondences the consensus kernel scores at a time
int ransac_ring_records();   // records of its LDS ring
// the consensus step of runRansac2d2d for a batch of (older, current) multiframe pairs (k_ransac2d2d.hip).  pairs
// (n_pairs x {mf0, mf1}) and fu (n_cams) lie in the parameter block of the call; every other pointer is the caller's.
constexpr int kRansac2SlotsLog2 = 12;  // the id table of a work-group: 4096 slots of 4 bytes
constexpr int kRansac2dMaxKeypoints = (1 << kRansac2SlotsLog2) - 1;  // an empty slot always ends a probe
// the home slot of a landmark id in that table: the ONE definition, the kernel's and the test hook's
__host__ __device__ inline uint32_t ransac2d2d_id_slot(int32_t id) {
  return ((uint32_t)id * 2654435761u) >> (32 - kRansac2SlotsLog2);
}
struct Ransac2d2dArgs {
  const uint8_t *blocks0, *blocks1;
  int o_count, o_kps, o_bp, o_bpv;
  size_t block_bytes;
  int kp_cap, n_cams;
  const int32_t* pairs;
  const double* fu;
  const int32_t *landmark0, *landmark1;  // landmark1 may alias out.landmark1_out
  const uint8_t* added;
  int n_landmarks;
  const double* rot_hyp;
  const uint8_t* rot_valid;
  const double* rel_hyp;
  const uint8_t* rel_valid;
  int n_hyp;
  double threshold;
  int remove_outliers;
  okvfe_ransac2d2d_result_device out;
};
void launch_ransac2d2d_consensus(const Ransac2d2dArgs& args, int n_pairs, hipStream_t stream);
int ransac2d2d_chunk_records();
int ransac2d2d_ring_records();
// the hypotheses of both problems of runRansac2d2d (k_ransac2d2d_hyp.hip, a part of k_ransac2d2d.hip's translation unit):
// sampler, rotation from two triads, five-point, the choice by samples 5 .. 7.  args: the consensus call's (its
// hypothesis lists, threshold and result are not read)
bool twopt_rotation_host(const double* b1, const double* b2, double* M);
bool fivept_hypothesis_host(bool tree, const double* b1, const double* b2, const double* sigma1, const double* sigma2,
                            double* hypothesis, int* n_roots);
void launch_ransac2d2d_hypotheses(const Ransac2d2dArgs& args, const uint64_t* keys, uint64_t seed,
                                  const okvfe_ransac2d2d_hypotheses_device& out, int n_pairs, hipStream_t stream);
// verifyRecognisedPlace after the descriptor matching (Frontend.cpp:347-397): the claims (k_place.hip) and the consensus
// over LoopclosureNoncentralAbsoluteAdapter's correspondences (k_ransac.hip, the kPlace policy of the kernel above)
constexpr int kPlaceClaimsMaxKeypoints = 12288;  // one int per keypoint in LDS
void launch_place_claims(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks, int n_multiframes,
                         int n_cams, int kp_cap, const int32_t* k_min, const uint32_t* dist_min, uint32_t threshold,
                         int min_inliers, const okvfe_place_claims_device& out, hipStream_t stream);
void launch_place_consensus(const double* hp, int n_landmarks, const BlockLayout& L, const uint8_t* blocks, int n_multiframes,
                            int n_cams, int kp_cap, const RansacCamParams* cams, const int32_t* match_landmark,
                            const uint8_t* gate, const double* hypotheses, const uint8_t* hyp_valid, int n_hyp,
                            double threshold, int min_inliers, const okvfe_ransac_result_device& out, uint8_t* verdict,
                            hipStream_t stream);
// the Hessian H of verifyRecognisedPlace (Frontend.cpp:529-551) and its terms for a batch of multiframes
// (k_place_hessian.hip).  cams (one record per camera) lies in the parameter block of the call, dcams are the context's
// camera slots; every other pointer is the caller's.
struct HessianCamParams {
  double pose[7];  // T_SC as a PoseParameterBlock holds it: t[3], qx qy qz qw
  int32_t cam;     // camera slot
  int32_t pad;
};
static_assert(sizeof(HessianCamParams) == 64, "64 bytes per camera");
struct PlaceHessianArgs {
  const double* hp;  // L x 4
  int n_landmarks;
  const uint8_t* blocks;
  int o_count, o_kps;
  size_t block_bytes;
  int kp_cap, n_cams, w, h;
  const HessianCamParams* cams;
  const DeviceCamera* dcams;
  const double* poses;  // n_multiframes x 7
  const int32_t* match_landmark;
  const uint8_t* state;
  const uint8_t* verdict;  // or null
  double* H;
  int32_t *n_terms, *n_singular;
  double *residual, *jacobian;  // optional
};
void launch_place_hessian(const PlaceHessianArgs& args, int n_multiframes, bool rt8, hipStream_t stream);
int place_hessian_chunk_terms();  // terms the kernel evaluates at a time
// the refinement of verifyRecognisedPlace's pose (Frontend.cpp:399-527) for a batch of multiframes (k_place_refine.hip; the
// solver is place_refine_dev.h, the term place_term_dev.h).  term: the Hessian call's arguments (poses, H and the rows are
// not read: an evaluation takes its pose from the multiframe's record); records and evals lie in the call's workspace.
struct PlaceRefineArgs {
  PlaceHessianArgs term;
  PlaceRefineRecord* records;  // n_multiframes
  PlaceRefineEval* evals;      // n_multiframes
  int n_multiframes, n_hyp, max_iterations;
  const double* hypotheses;    // n_multiframes x n_hyp x 12, or null where initial is given
  const int32_t* best;         // per multiframe, or null where initial is given
  const double* initial;       // n_multiframes x 7, or null
  double *poses, *start_poses, *cost;  // start_poses, cost: optional
  int32_t *status, *n_iterations, *n_accepted, *n_terms;  // all but status optional
};
void launch_place_refine_start(const PlaceRefineArgs& args, hipStream_t stream);
void launch_place_refine_eval(const PlaceRefineArgs& args, bool rt8, hipStream_t stream);
void launch_place_refine_step(const PlaceRefineArgs& args, bool first, hipStream_t stream);
// ImuError::propagation for a batch of multiframes (k_imu.hip; the arithmetic is imu_dev.h).  rig lies in the parameter
// block of the call: the seven doubles of okvfe_imu_params, one unused, then seven per camera of T_SC; every other pointer
// is the caller's.  The form follows out: covariance != null -> a wave per multiframe, else a lane per multiframe with
// or without F.
constexpr int kImuRigHeaderDoubles = 8;
struct ImuArgs {
  const double* samples;        // records of kImuSampleDoubles
  const int32_t* sample_begin;  // n_multiframes + 1
  const double* states;         // n_multiframes x kImuStateDoubles
  const double* rig;
  int n_multiframes, n_cams;
  ImuResultPtrs out;
};
void launch_imu_propagation(const ImuArgs& args, hipStream_t stream);
// scale space (k_pyramid.hip)
void launch_halfsample(const uint8_t* src, int w, int h, int n_images, uint8_t* dst, hipStream_t stream);
void launch_twothird(const uint8_t* src, int w, int h, int n_images, uint8_t* dst, hipStream_t stream);
void launch_scale_filter(Candidate* cand, int cand_cap, int32_t* cand_count, int n_images,
                         const int32_t* below, ScoreLayout lb, int wb, int hb, int rn_b, int rd_b,
                         const int32_t* above, ScoreLayout la, int wa, int ha, int rn_a, int rd_a,
                         hipStream_t stream);
void launch_merge_layers(const okvfe_keypoint* const* kps, const int32_t* const* counts,
                         const int32_t* const* cand_counts, const int* cand_cap, const float* scale, int n_layers,
                         int layer_cap, int n_images, okvfe_keypoint* out, int out_cap,
                         int32_t* out_count, hipStream_t stream);
void launch_hamming_argmin(const uint8_t* A, int nA, const uint8_t* B, int nB, uint32_t thr,
                           int32_t* best_j, uint32_t* best_d, hipStream_t stream);
void launch_hamming_count(const uint8_t* A, int nA, const uint8_t* B, int nB, int thr,
                          int32_t* row_counts, hipStream_t stream);
void launch_hamming_emit(const uint8_t* A, int nA, const uint8_t* B, int nB, int thr,
                         const int32_t* row_offsets, okvfe_candidate* out, int cap,
                         hipStream_t stream);
// keyframe coverage masks (k_keyframe.hip): one work-group per frame; frame f has its keypoint count at
// base + f * frame_stride + o_count, its okvfe_keypoint rows at ... + o_kps and its landmark ids at ids + f * id_stride
constexpr int kCoverageMaxRadius = 127;
constexpr size_t kCoverageLdsBudget = 64 * 1024 - 256;  // dynamic LDS of a group; the kernel's static LDS is below 256 B
struct CoverageArgs {
  const uint8_t* base;
  size_t frame_stride;
  int o_count, o_kps;
  int kp_limit;  // a frame's count is clamped to this
  const uint64_t* ids;
  size_t id_stride;
  const uint64_t* id_set;  // has_set: a keypoint is matched iff its id != 0 and is among these n_id_set values
  int n_id_set, has_set;
  int log2_slots;  // LDS hash table of the id set: 2^log2_slots 8-byte slots, filled to half at most (has_set only)
  int rows, cols, r;
  uint8_t hw[kCoverageMaxRadius + 1];  // half-width of the disc's span at row offset |j| <= r
};
// OpenCV's filled midpoint circle of radius r as half-widths per row offset 0..r (capi_keyframe.cpp)
void circle_half_widths(int r, uint8_t* hw);
struct CoverageGeometry {  // of a context's image size and a kptrad (coverage_geometry, okvfe_ctx.h)
  int rows, cols, r;
  int log2_slots;  // 0 without an id table
  size_t lds;      // dynamic LDS of a work-group
  uint8_t hw[kCoverageMaxRadius + 1];
};
void launch_keyframe_coverage(const CoverageArgs& args, int n_frames, size_t lds_bytes, okvfe_coverage* out,
                              hipStream_t stream);
// overlap counts of ordered multiframe pairs (k_keyframe.hip): two work-groups per pair, one per side.  The block of
// (multiframe m, camera c) is block m * stride_m + c * stride_c; its ids are the kp_cap values at ids + block * kp_cap.
constexpr int kOverlapMaxCams = 32;
constexpr size_t kOverlapCountsLds = 2 * kOverlapMaxCams * sizeof(int32_t);  // keypoint counts of both sides, behind the masks
struct OverlapArgs {
  const uint8_t* blocks;
  size_t block_bytes;
  int o_count, o_kps, kp_cap;
  const uint64_t* ids;
  const int32_t* pairs;  // device, (a, b) per pair
  int stride_m, stride_c, n_cams;
  int tiles;       // ceil(kp_cap / 256): hit bits a lane keeps per camera
  int log2_slots;  // LDS hash table of the other side's ids, filled to half at most per chunk
  int rows, cols, r;
  okvfe_overlap_counts* counts;
  okvfe_coverage* coverage;  // or null: [pair][side][camera]
  uint8_t hw[kCoverageMaxRadius + 1];
};
void launch_overlap_pairs(const OverlapArgs& args, int n_pairs, size_t lds_bytes, hipStream_t stream);

// place recognition on device-resident batches (k_bow.hip): one work-group per multiframe
constexpr int kBowMaxFeatures = 8192;            // n_cams x max_keypoints: the sort keys of a multiframe, padded to a power of two
constexpr size_t kBowLdsBudget = 61 * 1024;      // dynamic LDS of bow_vectors_kernel; its static LDS is below 2.2 KB
constexpr int kBowDenseWords = 4096;             // vocabularies up to here: the query is a dense word -> position table
constexpr int kBowQueryLdsWords = 4096;          // query words staged in LDS (12 bytes each); longer vectors are read from memory
struct BowVectorsArgs {
  const uint8_t* node_desc;
  const int32_t *child_begin, *child_index, *node_word;
  const double* word_weight;
  int n_nodes, n_words, weighting, normalise_l1, nodes_in_lds;
  const uint8_t* blocks;
  int o_count, o_desc;
  size_t block_bytes;
  int kp_cap, n_cams;
  int32_t* n_out;
  int32_t* ids;
  double* values;
  int stride;
  int32_t* word_ids;  // or null
};
struct PlaceQueryArgs {
  const int32_t *db_begin, *db_ids;
  const double* db_values;
  int n_entries;
  const int32_t *q_n, *q_ids;
  const double* q_values;
  int stride, n_vocab, lds_values;
  double min_score;
  const uint8_t* suppressible;  // or null
  double* scores;               // or null
  int32_t *n_listed, *n_candidates, *entry;
  double* score;
  int cap;
};
struct BowDbAddArgs {
  const int32_t* add_index;  // device, n_add
  const int32_t *q_n, *q_ids;
  const double* q_values;
  int stride;
  int32_t *begin, *ids;
  double* values;
  int n_entries, cap_words;
  int32_t* overflow;
};
size_t bow_vectors_lds_bytes(int n_nodes, int keys_cap, bool* nodes_in_lds);
void launch_bow_vectors(const BowVectorsArgs& args, int n_multiframes, size_t lds_bytes, hipStream_t stream);
void launch_place_query(const PlaceQueryArgs& args, int n_multiframes, bool dense, size_t lds_bytes, hipStream_t stream);
void launch_bow_db_add(const BowDbAddArgs& args, int n_add, hipStream_t stream);

}  // namespace okvfe
