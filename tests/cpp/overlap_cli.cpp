// overlap_cli.cpp -- drives the C++ host mirror's forms of ViSlamBackend::overlapFraction / trackingQuality and of the
// order of the motion-stereo sweep from a binary request file: okvfe::HipFrontend::overlapFraction (B = 1, host
// containers), overlapFractionBlocks (gather blocks on the device), trackingQuality and motionStereoFrameOrder.  Used by
// tests/test_gpu_overlap_cpp.py.
// request : int32 n_cams, w, h, K, n_multiframes, n_pairs, stride_m, stride_c, previous, block_bytes |
//           f64 kptrad (< 0: the mirror's default), f64 uniformity radius |
//           n_multiframes x n_cams x { int32 n | n*28 keypoints | n*8 landmark ids (u64) | n observed-elsewhere u8 } |
//           pair_a n_pairs i32 | pair_b n_pairs i32 | frame ids n_multiframes u64 |
//           gather blocks n_multiframes*n_cams*block_bytes u8 (host-packed, at their strided places) |
//           landmark ids n_multiframes*n_cams*K u64 (at the blocks' places)
// response: per pair f64 overlapFraction | per pair 32 B its counts | per pair 32 B the counts of overlapFractionBlocks |
//           per pair f64 okvfe_overlap_fraction of those | n_pairs*2*n_cams*24 B per-image records |
//           per multiframe f64 trackingQuality | int32 n_order | n_order i32: motionStereoFrameOrder over
//           overlapFraction(previous, i) | int32 bits: 1 a NaN overlap threw, 2 a multiframe short of a camera threw
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../okvis2_amd/host/okvfe_frontend.hpp"
#include "cli_io.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  const std::vector<int32_t> h = rdv<int32_t>(f, 10);
  const size_t nc = size_t(h[0]), K = size_t(h[3]), nm = size_t(h[4]), np = size_t(h[5]), bb = size_t(h[9]);
  const int previous = h[8];
  const std::vector<double> real = rdv<double>(f, 2);
  std::vector<std::vector<okvfe::FrameData>> frames(nm, std::vector<okvfe::FrameData>(nc));
  std::vector<std::vector<std::vector<uint8_t>>> observed(nm, std::vector<std::vector<uint8_t>>(nc));
  for (size_t m = 0; m < nm; ++m)
    for (size_t c = 0; c < nc; ++c) {
      const size_t n = size_t(rdv<int32_t>(f, 1)[0]);
      frames[m][c].keypoints = rdv<okvfe::KeyPoint>(f, n);
      frames[m][c].landmarkIds = rdv<uint64_t>(f, n);
      observed[m][c] = rdv<uint8_t>(f, n);
    }
  const std::vector<int32_t> pair_a = rdv<int32_t>(f, np), pair_b = rdv<int32_t>(f, np);
  const std::vector<uint64_t> frame_ids = rdv<uint64_t>(f, nm);
  const std::vector<uint8_t> blocks = rdv<uint8_t>(f, nm * nc * bb);
  const std::vector<uint64_t> ids = rdv<uint64_t>(f, nm * nc * K);
  fclose(f);
  std::vector<okvfe_camera> cams(nc, okvfe_camera{});
  for (okvfe_camera& c : cams) {
    c.width = h[1]; c.height = h[2];
    c.fu = c.fv = 0.6 * h[1]; c.cu = 0.5 * h[1]; c.cv = 0.5 * h[2];
  }
  try {
    okvfe::FrontendParameters p{};
    p.max_num_keypoints = h[3];
    p.detection_threshold = float(real[1]);
    okvfe::HipFrontend frontend(cams, p);
    if (size_t(frontend.rigMaxKeypoints()) != K || frontend.rigBlockBytes() != bb) {
      fprintf(stderr, "the request was packed for another row capacity\n");
      return 3;
    }
    const double kptrad = real[0];
    // B = 1
    std::vector<double> overlap(np);
    std::vector<okvfe_overlap_counts> counts(np);
    for (size_t i = 0; i < np; ++i)
      overlap[i] = frontend.overlapFraction(frames[size_t(pair_a[i])], frames[size_t(pair_b[i])], kptrad, &counts[i]);
    // device-resident
    DeviceBuffer d_blocks(nm * nc * bb), d_ids(nm * nc * K * 8), d_counts(np * sizeof(okvfe_overlap_counts)),
        d_cov(np * 2 * nc * sizeof(okvfe_coverage));
    d_blocks.upload(blocks);
    d_ids.upload(ids);
    if (okvfe_stream_synchronize(nullptr) != OKVFE_OK) return 5;
    void* stream = nullptr;
    if (okvfe_stream_create(0, &stream) != OKVFE_OK) return 5;
    frontend.overlapFractionBlocks(d_blocks.d, h[6], h[7], int(nm), d_ids.as<uint64_t>(), pair_a, pair_b,
                                   d_counts.as<okvfe_overlap_counts>(), d_cov.as<okvfe_coverage>(), kptrad, stream);
    if (okvfe_stream_synchronize(stream) != OKVFE_OK) return 5;
    okvfe_stream_destroy(stream);
    const std::vector<okvfe_overlap_counts> counts_dev = d_counts.download<okvfe_overlap_counts>(np);
    std::vector<double> overlap_dev(np + 1);
    if (okvfe_overlap_fraction(counts_dev.data(), int32_t(np), overlap_dev.data()) != OKVFE_OK) return 7;
    overlap_dev.resize(np);
    std::vector<double> quality(nm);
    for (size_t m = 0; m < nm; ++m) quality[m] = frontend.trackingQuality(frames[m], observed[m], kptrad);
    std::vector<double> row(nm);
    for (size_t m = 0; m < nm; ++m)
      row[m] = int(m) == previous ? 0.0 : frontend.overlapFraction(frames[size_t(previous)], frames[m], kptrad);
    const std::vector<int32_t> order = okvfe::HipFrontend::motionStereoFrameOrder(row, frame_ids, previous);
    const int32_t n_order = int32_t(order.size());
    int32_t threw = 0;
    try {
      std::vector<double> bad(row);
      bad[size_t(previous == 0 ? 1 : 0)] = std::numeric_limits<double>::quiet_NaN();
      okvfe::HipFrontend::motionStereoFrameOrder(bad, frame_ids, previous);
    } catch (const okvfe::Exception& e) {
      threw |= e.status == OKVFE_ERR_INVALID_ARGUMENT ? 1 : 0;
    }
    try {
      frontend.overlapFraction(frames[0], std::vector<okvfe::FrameData>(nc + 1), kptrad);
    } catch (const okvfe::Exception& e) {
      threw |= e.status == OKVFE_ERR_INVALID_ARGUMENT ? 2 : 0;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 1;
    put(o, overlap);
    put(o, counts);
    put(o, counts_dev);
    put(o, overlap_dev);
    put(o, d_cov.download<uint8_t>(np * 2 * nc * sizeof(okvfe_coverage)));
    put(o, quality);
    fwrite(&n_order, 4, 1, o);
    put(o, order);
    fwrite(&threw, 4, 1, o);
    fclose(o);
  } catch (const okvfe::Exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
