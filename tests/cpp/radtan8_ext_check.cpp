// Type check (compiled with -fsyntax-only against tests/mock/, never run) of the okvfe_camera_ext
// overloads of the C++ host classes: a PinholeCamera<RadialTangentialDistortion8> calibration goes
// in as OKVFE_DIST_RADTAN8 with its last four coefficients in d_ext, while the okvfe_camera
// overloads keep compiling for existing callers.
#define OKVFE_WITH_OPENCV 1
#define OKVFE_WITH_OKVIS 1
#define OKVFE_MOCK_OKVIS 1
#include "../../okvis2_amd/host/okvfe_cross_camera.hpp"
#include "../../okvis2_amd/host/okvfe_okvis_frontend.hpp"

static_assert(sizeof(okvfe_camera) == 80, "okvfe_camera keeps its ABI 7 layout");
static_assert(sizeof(okvfe_camera_ext) == 112, "okvfe_camera + k3 k4 k5 k6");
static_assert(OKVFE_DIST_RADTAN8 == 3, "okvfe_distortion numbering");

int main() {
  okvfe_camera_ext cam{};
  cam.base.width = 752; cam.base.height = 480;
  cam.base.fu = 350; cam.base.fv = 360; cam.base.cu = 378; cam.base.cv = 238;
  cam.base.distortion = OKVFE_DIST_RADTAN8;
  const double k[8] = {0.6261, 0.001, -0.0002, 0.0001, 0.0001, 0.9541, 0.1151, -0.0075};
  for (int i = 0; i < 4; ++i) cam.base.d[i] = k[i];
  for (int i = 0; i < 4; ++i) cam.d_ext[i] = k[4 + i];
  const std::vector<okvfe_camera_ext> rig{cam, cam};
  okvfe::FrontendParameters p;
  okvfe::HipFrontend fe(rig, p);
  okvfe::HipFrontend fe_plain(std::vector<okvfe_camera>{cam.base}, p);
  okvfe::HipViFrontend vi(nullptr, rig, p);
  okvfe::HipViFrontend vi_plain(nullptr, std::vector<okvfe_camera>{cam.base}, p);
  std::vector<okvfe_pose> poses(2);
  okvfe::CrossCameraMatcher ccm(rig, poses, p, 1, [](int, int) { return true; }, nullptr, 0);
  auto ctx = std::make_shared<okvfe::Context>(okvfe_config{});
  okvfe::HipBriskExtractor ex(ctx, 0);
  ex.setCamera(cam);
  ex.setCamera(cam.base);
  okvfe::cv_adapters::HipExtractor cvex(ctx, 0);
  cvex.setCamera(cam);
  cvex.setCamera(cam.base);
  float rays[3], jac[6];
  uint8_t mask[1];
  int32_t has = 0;
  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  (void)okvfe_build_awareness_maps_ext(&cam, rays, jac);
  (void)okvfe_camera_overlap_ext(&cam, &cam, R, mask, &has);
  (void)okvfe_set_camera_ext(ctx->get(), 0, &cam);
  okvfe_pose T{};
  (void)okvfe_match_motion_stereo_ext(ctx->get(), &cam, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, 0, &T, &T, nullptr);
  return 0;
}
