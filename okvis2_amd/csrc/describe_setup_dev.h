// describe_setup_dev.h -- the per-keypoint preparation of the extractor (border test, scale index,
// camera-aware matrix M), shared by describe_setup_kernel (k_describe.hip) and the tail of
// select_lazy_kernel (k_select.hip), which runs it for the keypoints it has just emitted when
// detection and description are one call (one launch and ~15 us per batch less).  On the batched camera-aware route that
// tail also assigns the keypoints' final slots: the set-up then decides validity completely and stores nothing itself
// (SetupDeferred below).
#pragma once
#include "okvfe_internal.h"

namespace okvfe {

// Lab builds of k_select.hip only (tools/lab/select_traffic.sh): ONE source of the selection kernel's memory traffic is
// switched off per build so that the byte counters and the kernel time price it.  Results of such a build are wrong by
// design.  Bits: 1 = the tail (K4) is skipped, 2 = no extra samples, 4 = the key workspace is no longer written once the
// first batches have filled it (same images every step), 8 = every image reads image 0's candidate list (L2-resident),
// 16 = ray and Jacobian from one fixed pixel, 32 = the tail computes but stores nothing.
#if defined(OKVFE_LAB) && defined(OKVFE_SELECT_OFF)
constexpr int kSelectOff = OKVFE_SELECT_OFF;
__device__ int g_select_off_flag;  // 1: the key workspace is filled (bit 4); never 2 (keeps the unstored values alive, bit 32)
#define OKVFE_TAIL_STORE(stmt)                                   \
  do {                                                           \
    if (!(kSelectOff & 32) || g_select_off_flag == 2) { stmt; } \
  } while (0)
#else
constexpr int kSelectOff = 0;
#define OKVFE_TAIL_STORE(stmt) \
  do {                         \
    stmt;                      \
  } while (0)
#endif

// one pixel's entry of a camera's ray map (3 floats) and of its Jacobian map (2 x 3 floats, row-major); the maps are
// device allocations of the library, so entry i of the Jacobian map is 8-byte aligned
// (vector types, so that each is ONE load instruction by construction: 12 bytes, and 16 + 8 bytes; in the global
// address space -- the map pointers come out of a table in memory, which leaves the compiler with flat loads)
#define OKVFE_GLOBAL_AS __attribute__((address_space(1)))
typedef float MapFloat3 __attribute__((ext_vector_type(3)));
typedef float MapFloat4 __attribute__((ext_vector_type(4)));
typedef float MapFloat2 __attribute__((ext_vector_type(2)));
typedef MapFloat3 MapRay __attribute__((aligned(4)));
typedef MapFloat4 MapJacobianLo __attribute__((aligned(8)));  // J00 J01 J02 J10
typedef MapFloat2 MapJacobianHi __attribute__((aligned(8)));  // J11 J12

// M = J * [e_x e_y] / fu on the tangent plane of the keypoint's ray, e_y along `dir`
__device__ __forceinline__ bool camera_aware_matrix(const float* __restrict__ rays,
                                                    const float* __restrict__ jac, int w, float fu,
                                                    const float dir[3], float kx, float ky,
                                                    float M[4]) {
  int u = (int)(kx + 0.5f), v = (int)(ky + 0.5f);
  if (kSelectOff & 16) {
    u = w / 2;
    v = w / 4;
  }
  // One element index, then the entry's 12 bytes of ray as one load and its 24 bytes of Jacobian as 16 + 8 (entries
  // are 24 bytes apart: 8-byte aligned).  Every load of a lane is a cache line of its own here, so their count is the
  // cost; written float by float, the compiler did merge the nine reads into these three, but as flat loads.
  const size_t at = (size_t)v * w + u;
  const MapRay ray = *(const OKVFE_GLOBAL_AS MapRay*)(rays + at * 3);
  // (requested with the ray, ahead of the tests below: behind them the Jacobian was a memory round trip of its own)
  const MapJacobianLo ja = *(const OKVFE_GLOBAL_AS MapJacobianLo*)(jac + at * 6);
  const MapJacobianHi jb = *(const OKVFE_GLOBAL_AS MapJacobianHi*)(jac + at * 6 + 4);
  const float r0 = ray.x, r1 = ray.y, r2 = ray.z;
  const float J0 = ja.x, J1 = ja.y, J2 = ja.z, J3 = ja.w, J4 = jb.x, J5 = jb.y;
  if (r0 == 0.0f && r1 == 0.0f && r2 == 0.0f) return false;
  float ey0 = 0.f, ey1 = 0.f, ey2 = 0.f, n2 = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float g0 = c == 0 ? dir[0] : (c == 1 ? 0.0f : 1.0f);
    const float g1 = c == 0 ? dir[1] : (c == 1 ? 1.0f : 0.0f);
    const float g2 = c == 0 ? dir[2] : 0.0f;
    if (c > 0 && n2 >= 1.0e-12f) break;
    float gr = g0 * r0;
    float t = g1 * r1;
    gr = gr + t;
    t = g2 * r2;
    gr = gr + t;
    t = gr * r0; ey0 = g0 - t;
    t = gr * r1; ey1 = g1 - t;
    t = gr * r2; ey2 = g2 - t;
    n2 = ey0 * ey0;
    t = ey1 * ey1;
    n2 = n2 + t;
    t = ey2 * ey2;
    n2 = n2 + t;
  }
  if (!(n2 >= 1.0e-12f)) return false;
  const float n = sqrtf(n2);
  ey0 = ey0 / n;
  ey1 = ey1 / n;
  ey2 = ey2 / n;
  float t1, t2;
  t1 = ey1 * r2; t2 = ey2 * r1; const float ex0 = t1 - t2;
  t1 = ey2 * r0; t2 = ey0 * r2; const float ex1 = t1 - t2;
  t1 = ey0 * r1; t2 = ey1 * r0; const float ex2 = t1 - t2;
  float s;
  s = J0 * ex0; t1 = J1 * ex1; s = s + t1; t1 = J2 * ex2; s = s + t1; M[0] = s / fu;
  s = J0 * ey0; t1 = J1 * ey1; s = s + t1; t1 = J2 * ey2; s = s + t1; M[1] = s / fu;
  s = J3 * ex0; t1 = J4 * ex1; s = s + t1; t1 = J5 * ex2; s = s + t1; M[2] = s / fu;
  s = J3 * ey0; t1 = J4 * ey1; s = s + t1; t1 = J5 * ey2; s = s + t1; M[3] = s / fu;
  return true;
}

// Extra sample e (a pattern point beyond the 64 lanes of describe_aware_kernel) of one keypoint, by ONE THREAD and
// straight from the image: the published BRISK smoothedIntensity with sub-pixel rim weights (same float / integer
// sequence as box_mean, k_describe_aware.hip), boxes of at most MAXB2 + 1 pixels a side.  All rows are loaded up
// front (aligned dword windows, one memory round trip); false = the box leaves the image (the keypoint is dropped).
template <int MAXB2>
__device__ __forceinline__ bool extra_sample_value(const uint8_t* __restrict__ im, int w, int h, float xf, float yf,
                                                   float sigma_half, int scaling, int scaling2, int* value) {
  const float x_1 = xf - sigma_half, x1 = xf + sigma_half;
  const float y_1 = yf - sigma_half, y1 = yf + sigma_half;
  if (!(x_1 >= 0.0f && y_1 >= 0.0f && x1 < (float)(w - 1) && y1 < (float)(h - 1))) return false;
  const int x_left = (int)(x_1 + 0.5f), y_top = (int)(y_1 + 0.5f);
  const int x_right = (int)(x1 + 0.5f), y_bottom = (int)(y1 + 0.5f);
  float r_x_1 = (float)x_left - x_1;  r_x_1 = r_x_1 + 0.5f;
  float r_y_1 = (float)y_top - y_1;   r_y_1 = r_y_1 + 0.5f;
  float r_x1 = x1 - (float)x_right;   r_x1 = r_x1 + 0.5f;
  float r_y1 = y1 - (float)y_bottom;  r_y1 = r_y1 + 0.5f;
  const float fs = (float)scaling;
  float t;
  t = r_x_1 * r_y_1; const int A = (int)(t * fs);
  t = r_x1 * r_y_1;  const int B = (int)(t * fs);
  t = r_x1 * r_y1;   const int C = (int)(t * fs);
  t = r_x_1 * r_y1;  const int D = (int)(t * fs);
  const int r_x_1_i = (int)(r_x_1 * fs), r_y_1_i = (int)(r_y_1 * fs);
  const int r_x1_i = (int)(r_x1 * fs), r_y1_i = (int)(r_y1 * fs);
  const int bw = x_right - x_left, bh = y_bottom - y_top;
  if (bw > MAXB2 || bh > MAXB2) return false;  // (cannot happen: the host checked the pattern's half-widths)
  // row window: NDW dwords from the dword that holds x_left (byte b of it); x_right is byte b + bw <= 3 + MAXB2
  constexpr int NDW = (3 + MAXB2) / 4 + 1;
  const int b = x_left & 3;
  const uint8_t* p0 = im + (size_t)y_top * w + (x_left & ~3);
  // byte `pos` of a row window, by a binary tree of selects on the bits of pos >> 2 (a chain of compares
  // against j is folded back into an indexed read, which puts the whole window in scratch)
  auto byte_at = [&](const uint32_t (&r)[NDW], int pos) -> int {
    uint32_t v[NDW];
#pragma unroll
    for (int j = 0; j < NDW; ++j) v[j] = r[j];
#pragma unroll
    for (int bit = 0; (1 << bit) < NDW; ++bit) {
      const bool hi = ((pos >> (2 + bit)) & 1) != 0;
#pragma unroll
      for (int j = 0; j + (1 << bit) < NDW; j += 2 << bit) v[j] = hi ? v[j + (1 << bit)] : v[j];
    }
    return (int)((v[0] >> (8 * (pos & 3))) & 0xFFu);
  };
  uint32_t msk[NDW];  // bytes b + 1 .. b + bw - 1 of a row window
#pragma unroll
  for (int j = 0; j < NDW; ++j) {
    int lo = b + 1 - 4 * j, hi = b + bw - 4 * j;
    lo = lo < 0 ? 0 : (lo > 4 ? 4 : lo);
    hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
    const uint32_t mlo = lo >= 4 ? 0xFFFFFFFFu : ((1u << (8 * lo)) - 1u);
    const uint32_t mhi = hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u);
    msk[j] = mhi & ~mlo;
  }
  int upper = 0, middle = 0, left = 0, right = 0, bottom = 0, pl_t = 0, pr_t = 0, pl_b = 0, pr_b = 0;
  // five rows per memory round trip (registers: the selection kernel's tail has 80)
  constexpr int kChunk = 5;
#pragma unroll
  for (int c0 = 0; c0 <= MAXB2; c0 += kChunk) {
    uint32_t d[kChunk][NDW];
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      const int dy = c0 + r;
      if (dy <= MAXB2) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p0 + (size_t)(dy < bh ? dy : bh) * w);
#pragma unroll
        for (int j = 0; j < NDW; ++j) d[r][j] = q[j];
      }
    }
#pragma unroll
    for (int r = 0; r < kChunk; ++r) {
      const int dy = c0 + r;
      if (dy <= MAXB2) {
        const int pl = byte_at(d[r], b), pr = byte_at(d[r], b + bw);
        int in = 0;
#pragma unroll
        for (int j = 0; j < NDW; ++j) in += (int)__builtin_amdgcn_sad_u8(d[r][j] & msk[j], 0u, 0u);
        if (dy == 0) {
          pl_t = pl;
          pr_t = pr;
          upper = in;
        } else if (dy < bh) {
          left += pl;
          right += pr;
          middle += in;
        } else if (dy == bh) {
          pl_b = pl;
          pr_b = pr;
          bottom = in;
        }
      }
    }
  }
  int ret = A * pl_t;
  ret += B * pr_t;
  ret += C * pr_b;
  ret += D * pl_b;
  ret += upper * r_y_1_i + middle * scaling + left * r_x_1_i + right * r_x1_i + bottom * r_y1_i;
  *value = (ret + scaling2 / 2) / scaling2;  // (non-negative: floor)
  return true;
}

// the constants of extra sample e (uniform over the workgroup: every lane reads the same five words)
struct ExtraSampleParams {
  float px, py, sigma_half;
  int scaling, scaling2;
};
__device__ __forceinline__ ExtraSampleParams extra_sample_params(const Pattern* __restrict__ pat, int e) {
  return ExtraSampleParams{pat->px[e], pat->py[e], pat->sigma_half[e], pat->box_scaling[e], pat->box_scaling2[e]};
}

// extra sample e of the keypoint at (kx, ky) under M -> extras_out[e] (bytes 24 + 4 e of its descriptor slot, or where
// the caller parks the samples until the slot is known); false: box outside the image
__device__ __forceinline__ bool extra_sample_one(const ExtraSampleParams& sp, const uint8_t* __restrict__ im, int w,
                                                 int h, int extra_box, int e, const float M[4], float kx, float ky,
                                                 int* __restrict__ extras_out, int stride = 1) {
  const float px = sp.px, py = sp.py, sg = sp.sigma_half;
  float a = M[0] * px, b2 = M[1] * py;  // (the sequence of sample_pos, k_describe_aware.hip)
  a = a + b2;
  const float xf = kx + a;
  float c = M[2] * px, d2 = M[3] * py;
  c = c + d2;
  const float yf = ky + c;
  int v = 0;
  const bool ok = extra_box <= 4 ? extra_sample_value<4>(im, w, h, xf, yf, sg, sp.scaling, sp.scaling2, &v)
                                 : extra_sample_value<9>(im, w, h, xf, yf, sg, sp.scaling, sp.scaling2, &v);
  OKVFE_TAIL_STORE(extras_out[e * stride] = v);
  return ok;
}

// sample position of a pattern point under M; ok = box inside the image (NaN-safe).  ONE definition for the descriptor
// kernels (k_describe_aware.hip) and for the set-up's validity test below: separate multiplies and adds, these comparisons.
__device__ __forceinline__ bool aware_sample_pos(float M0, float M1, float M2, float M3, float kx, float ky, float px,
                                                 float py, float sg, int w, int h, float* xf, float* yf) {
  float a = M0 * px;
  float b = M1 * py;
  a = a + b;
  *xf = kx + a;
  float c = M2 * px;
  float d = M3 * py;
  c = c + d;
  *yf = ky + c;
  const float x_1 = *xf - sg, x1 = *xf + sg, y_1 = *yf - sg, y1 = *yf + sg;
  return (x_1 >= 0.0f && y_1 >= 0.0f && x1 < (float)(w - 1) && y1 < (float)(h - 1));
}

// describe_aware_kernel's own drop test, by the set-up thread: every sample box of the pattern points first ..
// n_points - 1 (the kernel's 64 lanes) inside the image.  The trip count and every address are uniform over the
// workgroup (no early exit), so the pattern's constants arrive as scalar loads.
__device__ __forceinline__ bool first_pass_boxes_inside(const Pattern* __restrict__ pat, int first, int n_points,
                                                        const float M[4], float kx, float ky, int w, int h) {
  typedef const float __attribute__((address_space(4))) * cfloat_p;
  const cfloat_p px = (cfloat_p)(uintptr_t)pat->px, py = (cfloat_p)(uintptr_t)pat->py;
  const cfloat_p sg = (cfloat_p)(uintptr_t)pat->sigma_half;
  bool ok = true;
#pragma unroll 1
  for (int p = first; p < n_points; ++p) {
    float xf, yf;
    ok &= aware_sample_pos(M[0], M[1], M[2], M[3], kx, ky, px[p], py[p], sg[p], w, h, &xf, &yf);
  }
  return ok;
}

// What describe_setup_one returns instead of storing when the caller assigns the keypoint's FINAL slot itself
// (DescribeSetup::kps_out, the selection kernel's tail): validity decided completely -- the first-pass boxes included, so
// that describe_aware_kernel has nothing left to drop; M, the patch geometry and the extra samples wait in memory of the
// caller's (LDS: the selection kernel's tail has no register to spare for them across the samples and the fit).
// Word j of a thread's area is kSetupParkStride words behind word j - 1 (the areas of a workgroup's threads interleave:
// one base register, immediate offsets, no bank conflict).
constexpr int kSetupParkInts = kAwareMaxExtra + 2;  // extra samples | g0 | g1 (bit 31, free in g1: "patch inside", private)
constexpr int kSetupParkStride = 256;
struct SetupDeferred {
  bool valid;
  int n_extra;    // samples parked
  int* park;      // in: the workgroup's kSetupParkInts x kSetupParkStride words; a thread's word j = park[j * stride + thread]
  float* park_m;  // in: likewise for M, four words per thread
};
// the thread's index into the parked words, opaque to the optimiser: an address formed from it is formed where it is used
// (hoisted out of the caller's loop it would be one more register held across the sub-pixel fit and the samples)
__device__ __forceinline__ int setup_park_lane() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// What describe_setup_one needs that is the same for every keypoint of an image: the image's launch parameters, its
// camera's maps and three fields of the pattern.  Every address is uniform over the workgroup, so a caller that loads
// them before its first store (the selection kernels: at their start) gets scalar loads whose latency nothing waits
// for; read per keypoint, in the tail, they were six dependent memory round trips of every lane.
struct DescribeImageParams {
  ImageParams ip;
  const float* rays;
  const float* jac;
  int border;   // of the fixed-scale pattern
  float reach;
  int extra;    // samples beyond describe_aware_kernel's 64 lanes
};
__device__ __forceinline__ DescribeImageParams describe_image_params(const DescribeSetup& ds, int img) {
  DescribeImageParams p;
  p.ip = ds.prm[img];
  const bool aware = p.ip.mode == kCameraAware;
  p.rays = aware ? ds.rays[p.ip.cam] : nullptr;
  p.jac = aware ? ds.jac[p.ip.cam] : nullptr;
  p.border = ds.pat->border;
  p.reach = ds.pat->reach;
  p.extra = ds.pat->n_points - 64;
  return p;
}

// One keypoint: valid byte (bit 0 = inside the rim and a usable ray, bits 1..6 = scale index of the
// scale-invariant extractor), M into the first 16 bytes of the (not yet written) descriptor slot, the
// record into kps_tmp.  later != null (camera-aware fixed-scale calls only): nothing is stored, see SetupDeferred.
__device__ __forceinline__ void describe_setup_one(const DescribeSetup& ds, const DescribeImageParams& dp, int w, int h,
                                                   int img, size_t slot, const okvfe_keypoint& kp,
                                                   SetupDeferred* later = nullptr) {
  const ImageParams& ip = dp.ip;
  int scale = 0;
  if (ds.scales) {
    for (int i = 1; i < kPatternScales; ++i) scale += kp.size >= ds.scales->size_from[i] ? 1 : 0;
  }
  const int border = ds.scales ? ds.scales->border[scale] : dp.border;
  bool valid = !(kp.x < (float)border || kp.x >= (float)(w - border) || kp.y < (float)border ||
                 kp.y >= (float)(h - border));
  float M[4] = {1.0f, 0.0f, 0.0f, 1.0f};
  // (the first extra sample's constants travel with the ray and the Jacobian, each further one's with the rows of the
  // sample before it: read where they are used, every sample began with a round trip for five uniform words)
  const bool extras = ip.mode == kCameraAware && !ds.scales && ds.extra_box > 0 && dp.extra > 0 && !(kSelectOff & 2);
  ExtraSampleParams sp{};
  if (extras) sp = extra_sample_params(ds.pat, 0);
  if (valid && ip.mode == kCameraAware) {
    const float dir[3] = {ip.dir[0], ip.dir[1], ip.dir[2]};
    valid = camera_aware_matrix(dp.rays, dp.jac, w, ip.fu, dir, kp.x, kp.y, M);
  }
  if (later) {
    float* pm = later->park_m + setup_park_lane();
    for (int j = 0; j < 4; ++j) pm[j * kSetupParkStride] = M[j];
  } else {
    OKVFE_TAIL_STORE(*reinterpret_cast<float4*>(ds.desc_tmp + slot * OKVFE_DESC_BYTES) = make_float4(M[0], M[1], M[2], M[3]));
  }
  if (ip.mode == kCameraAware && !ds.scales) {
    // patch geometry for describe_aware_kernel (k_describe_aware.hip), bytes 16..23 of the slot: a superset of every
    // sample box under M -- |M p|_x <= |row_x(M)| |p|, boxes are not scaled by M, a box spans at most half a pixel
    // beyond x -+ sigma_half (the 0.75 leaves a quarter pixel for the float rounding of the positions) -- clipped to
    // the image (boxes that leave it drop the keypoint).  Class 0 / 1: rows of 64 / 80 bytes in LDS; 3: neither.
    int g0 = 0, g1 = 3 << 29;
    // the conservative patch bound lies strictly inside the image: so does every sample box (a subset of the exact test,
    // DESIGN.md "final slots"), and first_pass_boxes_inside need not walk the points
    bool patch_inside = false;
    if (valid) {
      const float reach = dp.reach;
      float nx = M[0] * M[0], t = M[1] * M[1];
      nx = sqrtf(nx + t) * 1.001f;
      float ny = M[2] * M[2];
      t = M[3] * M[3];
      ny = sqrtf(ny + t) * 1.001f;
      const float ex = fmaxf(nx, 1.0f) * reach + 0.75f, ey = fmaxf(ny, 1.0f) * reach + 0.75f;
      if (ex < 1024.0f && ey < 1024.0f) {  // (false for NaN)
        patch_inside = kp.x - ex >= 0.0f && kp.x + ex < (float)(w - 1) && kp.y - ey >= 0.0f && kp.y + ey < (float)(h - 1);
        int bx0 = (int)floorf(kp.x - ex), bx1 = (int)ceilf(kp.x + ex);
        int by0 = (int)floorf(kp.y - ey), by1 = (int)ceilf(kp.y + ey);
        bx0 = bx0 < 0 ? 0 : bx0;
        by0 = by0 < 0 ? 0 : by0;
        bx1 = bx1 > w - 1 ? w - 1 : bx1;
        by1 = by1 > h - 1 ? h - 1 : by1;
        const int px0 = bx0 & ~3, pw = bx1 - px0 + 1, ph = by1 - by0 + 1;
#ifndef OKVFE_AWARE_PITCH80
#define OKVFE_AWARE_PITCH80 0  // A/B: every patch in the 80-byte-pitch class (rows step through 16 bank phases instead of 4)
#endif
        const int cls = (!OKVFE_AWARE_PITCH80 && pw <= 64 && ph <= 64) ? 0 : ((pw <= 80 && ph <= 72) ? 1 : 3);
        if (pw >= 1 && ph >= 1 && px0 < 4096 && by0 < 4096) {
          g0 = by0 * w + px0;
          g1 = (px0 >> 2) | (by0 << 10) | ((cls == 3 ? 0 : ph) << 22) | (cls << 29);
        }
      }
    }
    if (later) {
      int* pk = later->park + setup_park_lane();
      pk[kAwareMaxExtra * kSetupParkStride] = g0;
      pk[(kAwareMaxExtra + 1) * kSetupParkStride] = g1 | (patch_inside ? (int)0x80000000u : 0);
    } else {
      OKVFE_TAIL_STORE(*reinterpret_cast<int2*>(ds.desc_tmp + slot * OKVFE_DESC_BYTES + 16) = make_int2(g0, g1));
    }
    // ... and the samples beyond its 64 lanes, bytes 24.. of the slot; a box outside the image drops the keypoint
    // (extra_box == 0: the pattern has none, or describe_kernel serves the call)
    if (valid && extras) {
      const int extra = dp.extra;  // 1 .. kAwareMaxExtra (host-checked)
      int* extras_out = later ? later->park + setup_park_lane() : reinterpret_cast<int*>(ds.desc_tmp + slot * OKVFE_DESC_BYTES + 24);
      for (int e = 0; e < extra && valid; ++e) {
        const ExtraSampleParams next = extra_sample_params(ds.pat, e + 1 < extra ? e + 1 : e);
        valid = extra_sample_one(sp, ds.images + (size_t)img * w * h, w, h, ds.extra_box, e, M, kp.x, kp.y, extras_out,
                                 later ? kSetupParkStride : 1);
        sp = next;
      }
    }
    if (later) {
      const int first = dp.extra > 0 ? dp.extra : 0;
      if (valid && later->park[(kAwareMaxExtra + 1) * kSetupParkStride + setup_park_lane()] >= 0)
        valid = first_pass_boxes_inside(ds.pat, first, dp.extra + 64, M, kp.x, kp.y, w, h);
      later->valid = valid;
      later->n_extra = extras ? dp.extra : 0;
      return;
    }
  }
  if (later) {  // (not reached: final slots are asked for on camera-aware fixed-scale calls only)
    later->valid = false;
    return;
  }
  OKVFE_TAIL_STORE(ds.valid_tmp[slot] = (uint8_t)((valid ? 1 : 0) | (scale << 1)));
  OKVFE_TAIL_STORE(ds.kps_tmp[slot] = kp);  // the record travels on from here; describe_kernel only rewrites the angle
}

// (describe_setup_kernel, k_describe.hip: one keypoint per thread of any image)
__device__ __forceinline__ void describe_setup_one(const DescribeSetup& ds, int w, int h, int img, size_t slot,
                                                   const okvfe_keypoint& kp) {
  describe_setup_one(ds, describe_image_params(ds, img), w, h, img, slot, kp);
}

}  // namespace okvfe
