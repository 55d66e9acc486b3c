// map_ransac_cli.cpp -- drives the whole matchToMap chain of the C++ host mirror on frames that live on the device:
// okvfe::HipFrontend::matchToMapBlocks -> ransac3d2dBlocks (landmark_out in place) -> removeOutliersBlocks (in place)
// -> matchToMapUninitialisedBlocks with the filtered rows as `previous`, all on one stream with nothing waited for in
// between; from a binary request file.  Used by tests/test_gpu_map_ransac_cpp.py and tools/bench_map_ransac.py.
// request : camera { int32 w,h,dist | f64 fu,fv,cu,cv,d[4] } | int32 K, match threshold, exclusive | f64 threshold |
//           table { int32 nl,no,np | hp nl*4 f64 | quality nl f64 | obs_begin (nl+1) i32 | obs_pose no i32 |
//           obs_desc no*48 u8 | obs_bp no*3 f64 | poses np*12 f64 } | int32 n_frames, block_bytes, o_kps, o_bp, o_bpv |
//           first-pass poses n_frames*12 f64 | poses now n_frames*12 f64 | gather blocks n_frames*block_bytes u8
//           (host-packed) | use n_frames*K u8 | T_SC 12 f64 | int32 n_hyp | hypotheses n_frames*n_hyp*12 f64
//           (a frame is a multiframe of one camera here)
// response: filtered rows n_frames*K i32 | n_correspondences, best_hypothesis, n_inliers n_frames i32 each |
//           accepted n_frames u8 | hyp_inliers n_frames*n_hyp i32 | state n_frames*K u8 | distance n_frames*K f64 |
//           kept n_frames i32 | second pass best_landmark, best_dist n_frames*K i32 each | hps_W n_frames*K*4 f64 |
//           hp_set n_frames*K u8 | already_matched n_frames i32 (outputs start as 0xF9 bytes: rows the calls leave
//           alone keep them) | int32: 1 if a hypothesis count that does not fit made ransac3d2dBlocks throw
// With a third argument `host N`: instead of the chain, the host form of the step it replaces, N times on frame 0 --
// the first pass's match rows downloaded, the correspondences rebuilt and every hypothesis scored by a plain loop, the
// filtered rows uploaded -- and one line "host_chain_us median p10 p90 n_corr best n_inliers" on stdout.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#include "cli_io.hpp"

// The host form of the consensus on one frame: a straightforward loop over hypotheses and correspondences (plain double
// arithmetic, sums left to right).  rows: the frame's landmark rows, filtered in place.  -> {n_corr, best, n_inliers}
struct HostVerdict {
  int n_corr = 0, best = -1, n_inliers = 0;
};
static HostVerdict host_consensus(const uint8_t* block, int o_kps, int o_bp, int o_bpv, const double* hp,
                                  const int32_t* obs_begin, int nl, double fu, const okvfe_pose& T_SC, const double* H,
                                  int n_hyp, double threshold, int32_t* rows) {
  struct Corr {
    double p[3], b[3], sigma;
    int k;
  };
  int32_t count;
  std::memcpy(&count, block, 4);
  const okvfe_keypoint* kps = reinterpret_cast<const okvfe_keypoint*>(block + o_kps);
  const double* bp = reinterpret_cast<const double*>(block + o_bp);
  std::vector<Corr> corr;
  for (int k = 0; k < count; ++k) {
    const int l = rows[k];
    if (l < 0 || l >= nl || obs_begin[l + 1] - obs_begin[l] < 1 || std::fabs(hp[4 * l + 3]) < 1.0e-8) continue;
    Corr c;
    for (int i = 0; i < 3; ++i) c.p[i] = hp[4 * l + i] / hp[4 * l + 3];
    double v[3] = {1.0, 0.0, 0.0};
    if (block[o_bpv + k])
      for (int i = 0; i < 3; ++i) v[i] = bp[3 * k + i];
    const double s = 0.8 * double(kps[k].size) / 12.0;
    c.sigma = std::sqrt(2.0) * s * s / (fu * fu);
    const double z = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    for (int i = 0; i < 3; ++i) c.b[i] = z > 0 ? v[i] / std::sqrt(z) : v[i];
    c.k = k;
    corr.push_back(c);
  }
  HostVerdict out;
  out.n_corr = int(corr.size());
  if (out.n_corr < 10) return out;
  std::vector<uint8_t> inl(corr.size()), best_inl(corr.size(), 0);
  for (int h = 0; h < n_hyp; ++h) {
    const double* M = H + 12 * h;
    double ti[3];
    for (int i = 0; i < 3; ++i) ti[i] = -M[i] * M[3] - M[4 + i] * M[7] - M[8 + i] * M[11];
    int n = 0;
    for (size_t j = 0; j < corr.size(); ++j) {
      const Corr& c = corr[j];
      double d[3], rep[3];
      for (int i = 0; i < 3; ++i) d[i] = M[i] * c.p[0] + M[4 + i] * c.p[1] + M[8 + i] * c.p[2] + ti[i] - T_SC.r[i];
      for (int i = 0; i < 3; ++i) rep[i] = T_SC.C[i] * d[0] + T_SC.C[3 + i] * d[1] + T_SC.C[6 + i] * d[2];
      const double nr = std::sqrt(rep[0] * rep[0] + rep[1] * rep[1] + rep[2] * rep[2]);
      double e2 = 0.0;
      for (int i = 0; i < 3; ++i) e2 += (rep[i] / nr - c.b[i]) * (rep[i] / nr - c.b[i]);
      inl[j] = e2 / c.sigma < threshold;
      n += inl[j];
    }
    if (n > out.n_inliers) {
      out.n_inliers = n;
      out.best = h;
      best_inl = inl;
    }
  }
  if (out.n_inliers >= 10 && double(out.n_inliers) / double(out.n_corr) > 0.7)
    for (size_t j = 0; j < corr.size(); ++j)
      if (!best_inl[j]) rows[corr[j].k] = -1;
  return out;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  okvfe_camera cam{};
  int32_t ci[3];
  rd(f, ci, 3);
  cam.width = ci[0]; cam.height = ci[1]; cam.distortion = ci[2];
  double cd[8];
  rd(f, cd, 8);
  cam.fu = cd[0]; cam.fv = cd[1]; cam.cu = cd[2]; cam.cv = cd[3];
  for (int i = 0; i < 4; ++i) cam.d[i] = cd[4 + i];
  int32_t par[3];
  rd(f, par, 3);
  double threshold;
  rd(f, &threshold, 1);
  int32_t tn[3];
  rd(f, tn, 3);
  const size_t nl = size_t(tn[0]), no = size_t(tn[1]), np = size_t(tn[2]);
  const std::vector<double> hp = rdv<double>(f, nl * 4), quality = rdv<double>(f, nl);
  const std::vector<int32_t> obs_begin = rdv<int32_t>(f, nl + 1), obs_pose = rdv<int32_t>(f, no);
  const std::vector<uint8_t> obs_desc = rdv<uint8_t>(f, no * 48);
  const std::vector<double> obs_bp = rdv<double>(f, no * 3);
  const std::vector<okvfe_pose> poses = rdv<okvfe_pose>(f, np);
  int32_t fn[5];
  rd(f, fn, 5);
  const size_t nf = size_t(fn[0]), block_bytes = size_t(fn[1]), K = size_t(par[0]);
  std::vector<okvfe_pose> T_first = rdv<okvfe_pose>(f, nf), T_now = rdv<okvfe_pose>(f, nf);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nf * block_bytes), use = rdv<uint8_t>(f, nf * K);
  okvfe_pose T_SC;
  rd(f, &T_SC, 1);
  int32_t n_hyp;
  rd(f, &n_hyp, 1);
  std::vector<double> H = rdv<double>(f, nf * size_t(n_hyp) * 12);
  fclose(f);
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = par[0];
    p.matching_threshold = par[1];
    okvfe::HipFrontend frontend(std::vector<okvfe_camera>{cam}, p);
    okvfe_landmark_table table{tn[0], tn[1], tn[2], hp.data(), quality.data(), obs_begin.data(), obs_pose.data(),
                               obs_desc.data(), obs_bp.data(), poses.data()};
    const auto dev_table = frontend.uploadLandmarkTable(0, table);
    DeviceBuffer d_blocks(nf * block_bytes), d_use(nf * K), d_lm(nf * K * 4), d_bd(nf * K * 4), d_status(nf * nl * 4),
        d_ndesc(nf * nl * 4), d_rows(nf * nl * 12), d_e(nf * nl * 48), d_r(nf * nl * 48), d_lm2(nf * K * 4),
        d_bd2(nf * K * 4), d_hp(nf * K * 32), d_hs(nf * K), d_ctr(nf * 4), d_head(nf * 12), d_acc(nf),
        d_hyp(nf * size_t(n_hyp) * 4), d_state(nf * K), d_dist(nf * K * 8), d_kept(nf * 4);
    if (okvfe_copy_to_device(d_blocks.d, blocks.data(), nf * block_bytes, nullptr) != OKVFE_OK ||
        okvfe_copy_to_device(d_use.d, use.data(), nf * K, nullptr) != OKVFE_OK ||
        okvfe_stream_synchronize(nullptr) != OKVFE_OK)
      return 5;
    okvfe_landmark_pool_device pool{};  // (projection stays NULL: the second pass does not read it)
    pool.status = d_status.as<int32_t>();
    pool.n_desc = d_ndesc.as<int32_t>();
    pool.obs_rows = d_rows.as<int32_t>();
    pool.e_W = d_e.as<double>();
    pool.r_W = d_r.as<double>();
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    frontend.matchToMapBlocks(0, *dev_table, d_blocks.d, int(nf), T_first, threshold, par[2] != 0, d_use.as<uint8_t>(),
                              &pool, d_lm.as<int32_t>(), d_bd.as<int32_t>(), stream);
    if (argc >= 5 && std::strcmp(argv[3], "host") == 0) {
      // the host chain this step replaces, on frame 0: rows down, a plain scoring loop, filtered rows up
      if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
      const int reps = std::max(1, atoi(argv[4]));
      std::vector<double> us;
      std::vector<int32_t> rows(K);
      HostVerdict v;
      DeviceBuffer d_prev(K * 4);
      for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        if (okvfe_copy_to_host(rows.data(), d_lm.d, K * 4, stream) != OKVFE_OK || okvfe_stream_synchronize(stream) != OKVFE_OK)
          return 6;
        v = host_consensus(blocks.data(), fn[2], fn[3], fn[4], hp.data(), obs_begin.data(), int(nl), cam.fu, T_SC, H.data(),
                           n_hyp, 16.0, rows.data());
        if (okvfe_copy_to_device(d_prev.d, rows.data(), K * 4, stream) != OKVFE_OK || okvfe_stream_synchronize(stream) != OKVFE_OK)
          return 6;
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
      }
      std::sort(us.begin(), us.end());
      printf("host_chain_us %.2f %.2f %.2f %d %d %d\n", us[us.size() / 2], us[us.size() / 10], us[us.size() * 9 / 10], v.n_corr,
             v.best, v.n_inliers);
      okvfe_stream_destroy(stream);
      return 0;
    }
    okvfe_ransac_result_device res{};
    res.n_correspondences = d_head.as<int32_t>();
    res.best_hypothesis = d_head.as<int32_t>() + nf;
    res.n_inliers = d_head.as<int32_t>() + 2 * nf;
    res.accepted = d_acc.as<uint8_t>();
    res.hyp_inliers = d_hyp.as<int32_t>();
    res.state = d_state.as<uint8_t>();
    res.distance = d_dist.as<double>();
    res.landmark_out = d_lm.as<int32_t>();  // in place
    frontend.ransac3d2dBlocks(0, *dev_table, d_blocks.d, int(nf), T_SC, d_lm.as<int32_t>(), H, {}, n_hyp, res, true, 16.0,
                              stream);
    frontend.removeOutliersBlocks(0, *dev_table, d_blocks.d, int(nf), T_now, d_lm.as<int32_t>(), d_lm.as<int32_t>(),
                                  d_kept.as<int32_t>(), 4.0, stream);
    frontend.matchToMapUninitialisedBlocks(0, *dev_table, pool, d_blocks.d, int(nf), T_now, par[2] != 0,
                                           d_use.as<uint8_t>(), d_lm.as<int32_t>(), d_lm2.as<int32_t>(),
                                           d_bd2.as<int32_t>(), d_hp.as<double>(), d_hs.as<uint8_t>(),
                                           d_ctr.as<int32_t>(), stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, d_lm.download<int32_t>(nf * K));
    put(o, d_head.download<int32_t>(nf * 3));
    put(o, d_acc.download<uint8_t>(nf));
    put(o, d_hyp.download<int32_t>(nf * size_t(n_hyp)));
    put(o, d_state.download<uint8_t>(nf * K));
    put(o, d_dist.download<double>(nf * K));
    put(o, d_kept.download<int32_t>(nf));
    put(o, d_lm2.download<int32_t>(nf * K));
    put(o, d_bd2.download<int32_t>(nf * K));
    put(o, d_hp.download<double>(nf * K * 4));
    put(o, d_hs.download<uint8_t>(nf * K));
    put(o, d_ctr.download<int32_t>(nf));
    // error behaviour: nHyp hypotheses per multiframe, or the call throws before anything is launched
    int32_t threw = 0;
    H.push_back(0.0);
    try {
      frontend.ransac3d2dBlocks(0, *dev_table, d_blocks.d, int(nf), T_SC, d_lm.as<int32_t>(), H, {}, n_hyp, res, true, 16.0,
                                stream);
    } catch (const okvfe::Exception& e) {
      threw = e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
    }
    okvfe_stream_destroy(stream);
    fwrite(&threw, 4, 1, o);
    fclose(o);
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
