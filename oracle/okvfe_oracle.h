/*
 * okvfe_oracle.h -- CPU oracle for the OKVIS2 vision front-end hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, the smoke check
 * in __graft_entry__.py and the cpu_baseline leg of bench.py may load it.  The
 * product library (libokvfe.so, okvis2_amd/csrc) never links or calls it.
 *
 * PARITY STATUS: "parity unpinned" for the detector / extractor arithmetic.
 *   The reference (smartroboticslab/okvis2 @ 2025-03-21) keeps that arithmetic
 *   in the un-vendored submodule external/brisk (.gitmodules:4-6, url
 *   ../brisk.git = github.com/smartroboticslab/brisk, pinned commit NOT
 *   recoverable from the snapshot) and ships no known-answer test for it
 *   (okvis_cv/test/TestFrame.cpp:56-93 has zero assertions).  The detector and
 *   extractor below are therefore a restatement of BRISK2's published
 *   algorithm (Harris scale-space detector with uniformity enforcement,
 *   ring-pattern binary descriptor), anchored on the reference's call sites:
 *     detector   ctor (uniformityRadius, octaves, absoluteThreshold, maxNumKpt)
 *                okvis_frontend/src/Frontend.cpp:2406-2409
 *     extractor  ctor (rotationInvariant, scaleInvariant), 48-byte rows
 *                okvis_frontend/src/Frontend.cpp:2410-2412, FBrisk.hpp:35
 *     extractor  setCameraProperties / setExtractionDirection
 *                okvis_frontend/src/Frontend.cpp:232-251
 *   Everything that IS in the reference tree is restated line-for-meaning and
 *   cites file:line at each function: the matcher loops and their FP64 gates
 *   (Frontend.cpp), triangulateFast (stereo_triangulation.cpp), the pinhole
 *   camera model with its distortions and camera-awareness maps (okvis_cv).
 *   Pins that do exist (Hamming known answers on the 819 real BRISK2
 *   descriptors of resources/small_voc.yml.gz, camera round-trip tolerances of
 *   okvis_cv/test/TestPinholeCamera.cpp:52-140) are checked in tests/.
 *
 * Determinism rules: build with -ffp-contract=off and no fast-math; every
 * float expression below is written with explicit temporaries so that host
 * and device evaluate the same IEEE-754 operations in the same order.
 */
#ifndef OKVFE_ORACLE_H_
#define OKVFE_ORACLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- plain data types (layout shared with include/okvfe.h by value) ------ */

/* Layout-compatible with cv::KeyPoint as consumed by the reference
 * (okvis_cv/include/okvis/implementation/Frame.hpp:253-273). */
typedef struct orc_keypoint {
  float x, y;      /* pt */
  float size;      /* 12 * layer scale */
  float angle;     /* -1 or pattern orientation in degrees */
  float response;  /* Harris score */
  int32_t octave;
  int32_t class_id;
} orc_keypoint;

typedef struct orc_point_score {
  int32_t x, y, score;
} orc_point_score;

#define ORC_DESC_BYTES 48      /* FBrisk.hpp:35 (L = 48) */
#define ORC_PATTERN_POINTS 72     /* capacity; the default pattern has 66 */
#define ORC_SHORT_PAIRS 384
#define ORC_MAX_LONG_PAIRS 1100

typedef struct orc_pattern {
  int32_t n_points;
  float px[ORC_PATTERN_POINTS];         /* unrotated offsets at the fixed scale */
  float py[ORC_PATTERN_POINTS];
  float sigma_half[ORC_PATTERN_POINTS]; /* half side of the smoothing box */
  int32_t n_short;
  uint8_t short_i[384], short_j[384];   /* bit b set iff value[i] > value[j] */
  int32_t n_long;
  uint8_t long_i[ORC_MAX_LONG_PAIRS], long_j[ORC_MAX_LONG_PAIRS];
  int32_t long_wdx[ORC_MAX_LONG_PAIRS], long_wdy[ORC_MAX_LONG_PAIRS];
  int32_t border;                       /* keypoints closer than this to the rim are removed */
  int32_t rot_cos[1024], rot_sin[1024]; /* round(2^15 * cos/sin(2 pi k / 1024)) */
  float rot_cosf[1024], rot_sinf[1024]; /* (float)cos/sin(2 pi k / 1024) */
} orc_pattern;

/* extractor modes */
#define ORC_MODE_UPRIGHT 0      /* rotationInvariant=false: pattern not rotated */
#define ORC_MODE_GRADIENT 1     /* rotationInvariant=true, not camera aware: long-pair gradient */
#define ORC_MODE_CAMERA_AWARE 2 /* setCameraProperties + setExtractionDirection given */

/* order of the 3-term FP64 sums of the matchers' gate chain: 1 = Eigen's x0 + (x1 + x2) (default), 0 = left to right */
void orc_set_reduction(int tree);
int orc_get_reduction(void);

/* ---- detector (A1) ------------------------------------------------------- */
void orc_harris_score(const uint8_t* img, int w, int h, int stride, int32_t* score /* h*w */);
int orc_nms(const int32_t* score, int w, int h, int abs_threshold,
            orc_point_score* out, int cap);
int orc_uniformity_select(orc_point_score* pts, int n, int w, int h, float radius,
                          int max_kpts);
void orc_subpixel2d(const int32_t s[9], float* dx, float* dy);
/* scale space (octaves > 0): layer images, sizes, scales and the cross-layer maximum test */
void orc_halfsample(const uint8_t* src, int w, int h, int stride, uint8_t* dst);
void orc_twothirdsample(const uint8_t* src, int w, int h, int stride, uint8_t* dst);
void orc_layer_scale(int l, int* num, int* den);
void orc_layer_size(int w, int h, int l, int* lw, int* lh);
int orc_scale_neighbour_ok(const int32_t* other, int wo, int ho, int x, int y, int32_t s, int rn, int rd);
/* octaves > 0: kps capacity should be 2*octaves*max_kpts */
void orc_agast_score(const uint8_t* img, int w, int h, int stride, int32_t* score /* h*w */);
void orc_fast58_score(const uint8_t* img, int w, int h, int stride, int32_t* score /* h*w */);
int32_t orc_scale_neighbour_max(const int32_t* other, int wo, int ho, int x, int y, int rn, int rd);
void orc_scale_refine(double rb, int have_b, int32_t sb, int32_t s, double ra, int have_a, int32_t sa,
                      double lo, float* rel_scale, float* score);
void orc_scale_refine_many(double rb, double ra, double lo, const int32_t* sb, const int32_t* s, const int32_t* sa,
                           int n, float* rel_scale, float* score);
void orc_score_map(int score_type, const uint8_t* img, int w, int h, int stride, int32_t* score);
int orc_detect_scored(const uint8_t* img, int w, int h, int stride, float uniformity_radius, int octaves,
                      int abs_threshold, int max_kpts, orc_keypoint* kps, int cap, int32_t* score_out,
                      int score_type);
int orc_detect(const uint8_t* img, int w, int h, int stride, float uniformity_radius,
               int octaves, int abs_threshold, int max_kpts, orc_keypoint* kps, int cap,
               int32_t* score_out /* optional h*w */);

/* ---- extractor (A2) ------------------------------------------------------ */
void orc_pattern_build(orc_pattern* p);           /* recovered BRISK2 table, 66 points (default) */
void orc_pattern_build_published(orc_pattern* p); /* published BRISK rings, 60 points, 383 pairs */
void orc_integral(const uint8_t* img, int w, int h, int stride, int32_t* integral /* (h+1)*(w+1) */);
int orc_smoothed_intensity(const uint8_t* img, const int32_t* integral, int w, int h, int stride,
                           float xf, float yf, float sigma_half);
/* returns number of kept keypoints; kps compacted in place, desc n'*48 */
int orc_describe(const uint8_t* img, int w, int h, int stride, const orc_pattern* pat, int mode,
                 const float* rays_hw3, const float* jac_hw6, float fu, const float dir[3],
                 orc_keypoint* kps, int n, uint8_t* desc);

/* scaleInvariant = true: per keypoint the pattern at scale index orc_scale_index(kp.size) */
int orc_scale_index(float size);
void orc_pattern_scaled(const orc_pattern* base, int index, orc_pattern* out);
int orc_describe_scaled(const uint8_t* img, int w, int h, int stride, const orc_pattern* pat, int mode,
                        const float* rays_hw3, const float* jac_hw6, float fu, const float dir[3],
                        orc_keypoint* kps, int n, uint8_t* desc);

/* ---- Hamming (A3) -------------------------------------------------------- */
uint32_t orc_popcnt_xor(const uint8_t* a, const uint8_t* b, int n128);

/* ---- camera model (A6, awareness maps) ----------------------------------- */
#define ORC_DIST_NONE 0
#define ORC_DIST_RADTAN 1
#define ORC_DIST_EQUI 2
typedef struct orc_camera {
  int32_t w, h;
  double fu, fv, cu, cv;
  int32_t dist_type;
  double d[4]; /* k1 k2 p1 p2 | k1 k2 k3 k4 */
} orc_camera;

/* fixed-sequence FP64 atan used by the equidistant model (see orc_camera.c header) */
double orc_atan_fixed(double x);
/* 1 = libm atan / acos (the reference's calls) instead of the fixed sequences (default 0) */
void orc_set_libm(int on);
int orc_get_libm(void);
double orc_atan_eval(double x);
int orc_cam_distort(const orc_camera* c, const double u[2], double out[2], double J[4]);
int orc_cam_undistort(const orc_camera* c, const double pd[2], double out[2]);
int orc_cam_backproject(const orc_camera* c, const double pt[2], double dir[3]);
/* status: 0 Successful, 1 OutsideImage, 2 Masked, 3 Behind, 4 Invalid */
int orc_cam_project(const orc_camera* c, const double p[3], double pt[2], double J23[6]);
void orc_cam_awareness_maps(const orc_camera* c, float* rays_hw3, float* jac_hw6);
int orc_cam_overlap(const orc_camera* c, const orc_camera* o, const double R_other_c[9],
                    uint8_t* mask_hw);
int orc_backproject_keypoints(const orc_camera* c, const orc_keypoint* kps, int n,
                              double* dirs_n3, uint8_t* valid);

/* ---- triangulation + matchers (A7, A8, A10, A11) ------------------------- */
typedef struct orc_pose { /* T_WC: p_W = C * p_C + r */
  double C[9]; /* row-major rotation */
  double r[3];
} orc_pose;

void orc_triangulate_fast(const double p1[3], const double e1[3], const double p2[3],
                          const double e2[3], double sigma, double hp[4], int* is_valid,
                          int* is_parallel);

typedef struct orc_stereo_match {
  int32_t k1;            /* matched index in image 1, -1 if none */
  int32_t dist;          /* Hamming distance of the match (threshold if none) */
  int32_t initialisable; /* !isParallel */
  int32_t pad;
  double hp_W[4];
} orc_stereo_match;

void orc_match_stereo(const uint8_t* desc0, const orc_keypoint* kp0, const double* bp0,
                      const uint8_t* bpv0, int n0, const uint8_t* desc1, const orc_keypoint* kp1,
                      const double* bp1, const uint8_t* bpv1, int n1, const orc_pose* T_WC0,
                      const orc_pose* T_WC1, double f0, double f1, double threshold,
                      orc_stereo_match* out /* n0 */);

typedef struct orc_motion_match {
  int32_t k1;     /* matched index in the current frame, -1 if none or rejected */
  int32_t dist;
  int32_t initialisable;
  int32_t accepted; /* passed the 4 px reprojection check */
  double quality;
  double hp_W[4];
} orc_motion_match;

void orc_match_motion_stereo(const uint8_t* desc0, const orc_keypoint* kp0, const double* bp0,
                             const uint8_t* bpv0, const uint8_t* skip0, int n0,
                             const uint8_t* desc1, const orc_keypoint* kp1, const double* bp1,
                             const uint8_t* bpv1, const uint8_t* matched1, int n1,
                             const orc_pose* T_WC0, const orc_pose* T_WC1, const orc_camera* cam,
                             uint32_t threshold, orc_motion_match* out /* n0 */);

void orc_match_to_map(const uint8_t* desc, const orc_keypoint* kps, const uint8_t* use, int n_k,
                      const double* proj, const int32_t* desc_begin, int n_lm, const uint8_t* pool,
                      double reprojection_threshold, double threshold, int32_t* best_lm,
                      int32_t* best_d);

void orc_match_to_map_uninit(const uint8_t* desc, const double* bp, const uint8_t* use,
                             const int32_t* previous, int n_k, const int32_t* desc_begin, int n_lm,
                             const uint8_t* pool, const double* e0_W, const double* r0_W,
                             const orc_pose* T_WC1, double focal, double threshold,
                             int32_t* best_lm, int32_t* best_d, double* hps_W, uint8_t* hp_set,
                             int32_t* ctr_out);

/* ---- gate census: which branches of the gate chain a scene reaches ---------------------------
 * The *_census entry points run the very loop of their plain counterpart (one shared static
 * function) and add, into counters[ORC_CEN_COUNT] when it is not null, one count per gate
 * evaluation AS THE SEQUENTIAL LOOP MAKES IT (a pair the running minimum never lets through is
 * not counted).  Outputs are the plain entry point's, byte for byte. */
enum {
  ORC_CEN_BP_INVALID = 0,  /* back-projection invalid on either side (gated pair dropped) */
  ORC_CEN_DET_SINGULAR,    /* !(|det| > 1e-12) */
  ORC_CEN_L_SMALL,         /* l0 < 0.01 || l1 < 0.01 */
  ORC_CEN_TN_SMALL,        /* |t12| < 0.01 inside midpoint_parallel */
  ORC_CEN_PAR_COS26_E1,    /* midpoint_parallel: first cos 2.6 sigma test fails */
  ORC_CEN_PAR_COS26_E2,    /* midpoint_parallel: second fails */
  ORC_CEN_TRI_COS26_E1,    /* plain triangulation: first cos 2.6 sigma test fails */
  ORC_CEN_TRI_COS26_E2,    /* plain triangulation: second fails */
  ORC_CEN_COS6_PARALLEL,   /* dot(n2, n1) > cos 6 sigma */
  ORC_CEN_DEPTH0,          /* depth in camera 0 below 0.05 (stereo) / 0.2 (motion) */
  ORC_CEN_DEPTH1,          /* depth in camera 1 below it */
  ORC_CEN_EE_05,           /* ee < 0.5 (motion) */
  ORC_CEN_EE_08,           /* ee < 0.8 */
  ORC_CEN_PX4_ACCEPT,      /* winner passes the 4 px check */
  ORC_CEN_PX4_REJECT,      /* winner fails it */
  ORC_CEN_PROJ_STATUS,     /* winner's projection status != 0 */
  ORC_CEN_EPIPOLAR,        /* uninitialised: not in the epipolar plane */
  ORC_CEN_DIVERGENT,       /* uninitialised: divergent rays */
  ORC_CEN_NEAR_PARALLEL,   /* uninitialised: near-parallel rays bypass both tests */
  ORC_CEN_DIST0,           /* uninitialised: point within 0.2 m of the observation centre */
  ORC_CEN_DIST1,           /* uninitialised: within 0.2 m of the current centre */
  ORC_CEN_PREVIOUS,        /* uninitialised: l == previous[k] counted */
  ORC_CEN_WIN_HP,          /* uninitialised: winner replaced, hp stored */
  ORC_CEN_WIN_NO_HP,       /* uninitialised: winner replaced, parallel: no hp */
  ORC_CEN_RADIUS_PASS,     /* 3-D map: inside the reprojection radius */
  ORC_CEN_RADIUS_FAIL,     /* 3-D map: outside */
  ORC_CEN_MIN_REPLACED,    /* 3-D map: a running minimum replaced by a LATER landmark */
  ORC_CEN_NAN_OPERAND,     /* a comparison of the chain saw a NaN operand */
  ORC_CEN_COUNT
};
const char* orc_census_label(int label); /* NULL outside [0, ORC_CEN_COUNT) */

void orc_match_stereo_census(const uint8_t* desc0, const orc_keypoint* kp0, const double* bp0,
                             const uint8_t* bpv0, int n0, const uint8_t* desc1, const orc_keypoint* kp1,
                             const double* bp1, const uint8_t* bpv1, int n1, const orc_pose* T_WC0,
                             const orc_pose* T_WC1, double f0, double f1, double threshold,
                             orc_stereo_match* out /* n0 */, int64_t* counters);
void orc_match_motion_stereo_census(const uint8_t* desc0, const orc_keypoint* kp0, const double* bp0,
                                    const uint8_t* bpv0, const uint8_t* skip0, int n0,
                                    const uint8_t* desc1, const orc_keypoint* kp1, const double* bp1,
                                    const uint8_t* bpv1, const uint8_t* matched1, int n1,
                                    const orc_pose* T_WC0, const orc_pose* T_WC1, const orc_camera* cam,
                                    uint32_t threshold, orc_motion_match* out /* n0 */, int64_t* counters);
void orc_match_to_map_census(const uint8_t* desc, const orc_keypoint* kps, const uint8_t* use, int n_k,
                             const double* proj, const int32_t* desc_begin, int n_lm, const uint8_t* pool,
                             double reprojection_threshold, double threshold, int32_t* best_lm,
                             int32_t* best_d, int64_t* counters);
void orc_match_to_map_uninit_census(const uint8_t* desc, const double* bp, const uint8_t* use,
                                    const int32_t* previous, int n_k, const int32_t* desc_begin, int n_lm,
                                    const uint8_t* pool, const double* e0_W, const double* r0_W,
                                    const orc_pose* T_WC1, double focal, double threshold,
                                    int32_t* best_lm, int32_t* best_d, double* hps_W, uint8_t* hp_set,
                                    int32_t* ctr_out, int64_t* counters);

/* candidates: all (i, j) with popcnt(A[i]^B[j]) < thr in (i, j) order */
typedef struct orc_cand {
  int32_t i, j, dist;
} orc_cand;
int orc_hamming_candidates(const uint8_t* A, int nA, const uint8_t* B, int nB, int thr,
                           orc_cand* out, int cap);
/* min-distance per row (verifyRecognisedPlace style, no gate): Frontend.cpp:330-355 */
void orc_hamming_argmin(const uint8_t* A, int nA, const uint8_t* B, int nB, uint32_t thr,
                        int32_t* best_j, uint32_t* best_d);

/* ---- end to end, per image (A4 minus bookkeeping) ------------------------ */
typedef struct orc_frontend_params {
  float uniformity_radius;
  int32_t octaves;
  int32_t abs_threshold;
  int32_t max_kpts;
  int32_t mode;
} orc_frontend_params;

int orc_detect_describe(const uint8_t* img, int w, int h, int stride,
                        const orc_frontend_params* prm, const orc_pattern* pat,
                        const float* rays_hw3, const float* jac_hw6, float fu, const float dir[3],
                        orc_keypoint* kps, uint8_t* desc, int cap);

/* verifyRecognisedPlace for all landmarks of one camera; DBoW2 vocabulary descent (FBrisk) */
void orc_verify_place(const uint8_t* pool, const int32_t* desc_begin, int n_landmarks,
                      const uint8_t* frame_desc, int K, uint32_t threshold, int32_t* k_min,
                      uint32_t* dist_min);
void orc_voc_transform(const uint8_t* desc, int n, const uint8_t* node_desc, const int32_t* child_begin,
                       const int32_t* child_index, const int32_t* word, int32_t* word_out,
                       int32_t* node_out);

/* matchToMap: landmark projection + descriptor-view pooling (Frontend.cpp:1219-1359) */
double orc_acos_fixed(double x);
void orc_prepare_landmarks(const double* hp_W, const double* quality, const int32_t* obs_begin,
                           int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                           const orc_pose* poses_old, const orc_pose* T_WC1, const orc_camera* cam,
                           double repr_threshold, int exclusive, int32_t* status, int32_t* n_desc,
                           int32_t* obs_rows, double* projection, double* e_W, double* r_W);

/* ---- census of the landmark preparation: which branches of Frontend.cpp:1219-1359 a table reaches.
 * orc_prepare_landmarks_census runs the very loop of orc_prepare_landmarks (one shared static
 * function) and adds one count per event into counters[ORC_PCEN_COUNT]; its outputs are the plain
 * entry point's, byte for byte.  Per landmark unless it says per observation. */
enum {
  ORC_PCEN_HEAD_NEGATED = 0, /* hp_C[3] < 0: the head of hp_C is negated before it is projected */
  ORC_PCEN_PROJ_INVALID,     /* projection status Invalid (|z| < 1e-12) */
  ORC_PCEN_PROJ_BEHIND,      /* status Behind */
  ORC_PCEN_PROJ_OUTSIDE_KEPT,/* status OutsideImage, and inside the reprojection margin */
  ORC_PCEN_PROJ_SUCCESSFUL,  /* status Successful */
  ORC_PCEN_MARGIN_U_LOW,     /* kp[0] < -thr */
  ORC_PCEN_MARGIN_V_LOW,     /* kp[1] < -thr */
  ORC_PCEN_MARGIN_U_HIGH,    /* kp[0] > w + thr */
  ORC_PCEN_MARGIN_V_HIGH,    /* kp[1] > h + thr */
  ORC_PCEN_CLAMP_R,          /* max(0.01, |r_W|) takes 0.01 (landmarks past the FoV check) */
  ORC_PCEN_IS3D_FIRST,       /* is3d set at the first observation */
  ORC_PCEN_IS3D_LATER,       /* is3d set at a later observation */
  ORC_PCEN_IS3D_NEVER,       /* at least one observation, is3d never set */
  ORC_PCEN_VP_REJECT,        /* per observation: cosVC < cos(0.6), dropped */
  ORC_PCEN_VP_KEPT_EXCL,     /* per observation: cosVC < cos(0.6), kept because the call is exclusive */
  ORC_PCEN_SCALE_REJECT,     /* per observation: scaleChange > 0.5, dropped */
  ORC_PCEN_SCALE_KEPT_EXCL,  /* per observation: scaleChange > 0.5, kept because the call is exclusive */
  ORC_PCEN_ACOS_TINY,        /* per scored observation: |x| < 2^-57 */
  ORC_PCEN_ACOS_SMALL,       /* 2^-57 <= |x| < 0.5 */
  ORC_PCEN_ACOS_NEG,         /* -1 <= x <= -0.5 */
  ORC_PCEN_ACOS_POS,         /* 0.5 <= x <= 1 */
  ORC_PCEN_ACOS_ABOVE_ONE,   /* |x| > 1: NaN */
  ORC_PCEN_NOT_STORED,       /* per scored observation: !(score < best[worst]) */
  ORC_PCEN_NOT_STORED_TIE,   /*   of those: score == best[worst] */
  ORC_PCEN_NOT_STORED_GE1,   /*   of those: score >= 1 */
  ORC_PCEN_NOT_STORED_NAN,   /*   of those: score is a NaN */
  ORC_PCEN_WRITE_S0_O0,      /* per stored observation: slot `worst` replaced, descriptor written at row o */
  ORC_PCEN_WRITE_S0_O1,
  ORC_PCEN_WRITE_S0_O2,
  ORC_PCEN_WRITE_S1_O0,
  ORC_PCEN_WRITE_S1_O1,
  ORC_PCEN_WRITE_S1_O2,
  ORC_PCEN_WRITE_S2_O0,
  ORC_PCEN_WRITE_S2_O1,
  ORC_PCEN_WRITE_S2_O2,
  ORC_PCEN_FINAL_O0_STORED,  /* final o == 0 with one stored view: "no observations -- weird", status 0 */
  ORC_PCEN_FINAL_O1,         /* final o == 1 */
  ORC_PCEN_FINAL_O2,         /* final o == 2, three views stored */
  ORC_PCEN_FINAL_O2_CROPPED, /* final o == 2 and a third row written, then cropped */
  ORC_PCEN_COUNT
};
const char* orc_prepare_census_label(int label); /* NULL outside [0, ORC_PCEN_COUNT) */
void orc_prepare_landmarks_census(const double* hp_W, const double* quality, const int32_t* obs_begin,
                                  int n_landmarks, const int32_t* obs_pose, const double* obs_bp,
                                  const orc_pose* poses_old, const orc_pose* T_WC1, const orc_camera* cam,
                                  double repr_threshold, int exclusive, int32_t* status, int32_t* n_desc,
                                  int32_t* obs_rows, double* projection, double* e_W, double* r_W,
                                  int64_t* counters);

#ifdef __cplusplus
}
#endif
int orc_bow_vector(const int32_t* word_ids, int n_features, const double* word_weight, int n_words, int weighting,
                   int normalise_l1, int32_t* ids_out /* n_words */, double* values_out /* n_words */);
void orc_bow_query_l1(const int32_t* db_begin, const int32_t* db_ids, const double* db_values, int n_entries,
                      const int32_t* q_ids, const double* q_values, int n_q, int n_words, double* scores);
#endif /* OKVFE_ORACLE_H_ */
