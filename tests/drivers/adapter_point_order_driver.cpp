// adapter_point_order_driver.cpp — TEST DRIVER for include/mot_adapters.hpp (not product code).
//
// mot_adapters::Config::point_order reaches mot_set_point_order: one elevated cloud through the reference-signature functions
// componentClustering + boxFitting (OT/include/component_clustering.h:20-22, box_fitting.h:34-36) on a context of 8192 points.
//
//   adapter_point_order_driver IN.bin OUT.bin order        order: 0 = MOT_ORDER_SCAN, 1 = MOT_ORDER_ANY, anything else as given
//
// IN.bin: int32 n, float32 xyzw[n][4]. OUT.bin: int32 boxes, float32 corners[boxes][8][3]. A refusal of the library: its message on
// stderr, exit status 3.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "mot_adapters.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s IN.bin OUT.bin order\n", argv[0]); return 2; }
  mot_adapters::Config c;
  c.max_points = 8192;
  c.max_tracks_total = 64;
  c.point_order = std::atoi(argv[3]);
  mot_adapters::configure(c);
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::perror("open"); return 2; }
  int n = 0;
  if (std::fread(&n, 4, 1, in) != 1 || n < 0) return 2;
  std::vector<float> pts((size_t)n * 4 + 1);
  if (n && std::fread(pts.data(), 4, (size_t)n * 4, in) != (size_t)n * 4) return 2;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>());
  for (int i = 0; i < n; i++) cloud->push_back(pcl::PointXYZ(pts[4 * i], pts[4 * i + 1], pts[4 * i + 2]));
  try {
    auto grid = std::make_unique<std::array<std::array<int, 250>, 250>>();
    int num_cluster = 0;
    componentClustering<250>(cloud, *grid, num_cluster);
    visualization_msgs::MarkerArray ma;
    std::vector<pcl::PointCloud<pcl::PointXYZ>> boxes = boxFitting<250>(cloud, *grid, num_cluster, ma);
    const int nb = (int)boxes.size();
    std::fwrite(&nb, 4, 1, out);
    for (const auto& b : boxes)
      for (size_t k = 0; k < b.size(); k++) { const float v[3] = {b[k].x, b[k].y, b[k].z}; std::fwrite(v, 4, 3, out); }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  std::fclose(out);
  return 0;
}
