// vlcal::DeviceCloud from float32 records (nidreg_cloud_create_f32) against the Frame (double) constructor: the same scene
// uploaded three ways -- Frame doubles, the stored 16 B PLY record (x y z intensity), glk::PLYData-style separate arrays
// (vertices stride 12, intensities stride 4) -- and one NIDCost per cloud, without and with the view cull.
// Prints the six double-instantiation costs: frame rec16 soa (no cull), frame rec16 soa (cull).
#include <cstdio>
#include <memory>
#include <vector>

#include "vlcal_amd/nid_cost.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int W, H, N, bins, nintr, ndist;
  char model[64] = {0};
  double intr[5], dist[8], se3[7], min_z, T[16];
  if (fread(model, 1, 64, f) != 64) return 4;
  if (fread(&W, 4, 1, f) != 1 || fread(&H, 4, 1, f) != 1 || fread(&N, 4, 1, f) != 1 || fread(&bins, 4, 1, f) != 1 || fread(&nintr, 4, 1, f) != 1 || fread(&ndist, 4, 1, f) != 1) return 4;
  if (fread(intr, 8, 5, f) != 5 || fread(dist, 8, 8, f) != 8 || fread(se3, 8, 7, f) != 7 || fread(&min_z, 8, 1, f) != 1 || fread(T, 8, 16, f) != 16) return 4;
  cv::Mat img8(H, W, cv::CV_8UC1_), img64(H, W, cv::CV_64FC1_);
  if (fread(img8.data, 1, size_t(W) * H, f) != size_t(W) * H) return 4;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) img64.at<double>(y, x) = img8.at<unsigned char>(y, x) * (1.0 / 255.0);
  std::vector<float> xyz(size_t(N) * 3), inten(static_cast<size_t>(N));
  if (fread(xyz.data(), 12, N, f) != size_t(N) || fread(inten.data(), 4, N, f) != size_t(N)) return 4;
  fclose(f);

  auto proj = camera::create_camera(model, std::vector<double>(intr, intr + nintr), std::vector<double>(dist, dist + ndist));
  if (!proj) return 6;
  // what visual_lidar_data.cpp:19-26 builds on the host: x y z 1 doubles + double intensities
  std::vector<Eigen::Vector4d> pts(N);
  std::vector<double> ints(N);
  std::vector<float> rec(size_t(N) * 4);
  for (int i = 0; i < N; i++) {
    pts[i] = Eigen::Vector4d{{xyz[3 * size_t(i)], xyz[3 * size_t(i) + 1], xyz[3 * size_t(i) + 2], 1.0}};
    ints[i] = inten[i];
    for (int k = 0; k < 3; k++) rec[4 * size_t(i) + k] = xyz[3 * size_t(i) + k];
    rec[4 * size_t(i) + 3] = inten[i];
  }
  auto frame = std::make_shared<vlcal::Frame>();
  frame->num_points = N;
  frame->points = pts.data();
  frame->intensities = ints.data();

  try {
    const vlcal::DeviceCloud clouds[3] = {
      vlcal::DeviceCloud(frame),
      vlcal::DeviceCloud(rec.data(), 16, rec.data() + 3, 16, N),
      vlcal::DeviceCloud(xyz.data(), 12, inten.data(), 4, N),
    };
    for (int cull = 0; cull < 2; cull++) {
      for (const auto& cloud : clouds) {
        vlcal::NIDCost cost(proj, img64, cloud, cull ? T : nullptr, min_z, true, bins);
        double c = 0.0;
        if (!cost(se3, &c)) return 7;
        printf("%.17g\n", c);
      }
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 8;
  }
  return 0;
}
