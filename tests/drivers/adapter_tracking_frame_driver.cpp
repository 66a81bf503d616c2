// adapter_tracking_frame_driver.cpp — TEST DRIVER for mot_adapters::trackingNodeFrame (include/mot_adapters.hpp; not product code).
//
// Feeds a recorded sequence of sensor-frame box lists through the one-call helper and writes what it returned, frame by frame, as text
// (floats with 9 digits, doubles with 17: both round-trip). tests/test_nodes_tracking_frame.py compares with the stage-wise sequence.
//
//   adapter_tracking_frame_driver IN.bin OUT.txt max_tracks_total
//
// IN.bin: int32 frames; per frame: int32 m, float64 timestamp, v, yaw, float32 boxes[m][8][3] (tests/adapter_case.py's format).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mot_adapters.hpp"

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s IN.bin OUT.txt max_tracks_total\n", argv[0]); return 2; }
  mot_adapters::Config c;
  c.max_points = 4096;
  c.max_tracks_total = std::atoi(argv[3]);
  mot_adapters::configure(c);
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) { std::perror("open"); return 2; }
  int frames = 0;
  if (std::fread(&frames, 4, 1, in) != 1) return 2;
  for (int f = 0; f < frames; f++) {
    int m = 0; double hdr[3];
    if (std::fread(&m, 4, 1, in) != 1 || std::fread(hdr, 8, 3, in) != 3) return 2;
    std::vector<float> b((size_t)m * 24 + 1);
    if (m && std::fread(b.data(), 4, (size_t)m * 24, in) != (size_t)m * 24) return 2;
    std::vector<pcl::PointCloud<pcl::PointXYZ>> bBoxes(m);
    for (int i = 0; i < m; i++)
      for (int k = 0; k < 8; k++) bBoxes[i].push_back(pcl::PointXYZ(b[(i * 8 + k) * 3], b[(i * 8 + k) * 3 + 1], b[(i * 8 + k) * 3 + 2]));
    const mot_adapters::TrackingFrame r = mot_adapters::trackingNodeFrame(bBoxes, hdr[0], hdr[1], hdr[2]);
    std::fprintf(out, "%d %zu %d %zu", f, r.ids.size(), r.tracksEver, r.visBBs.size());
    for (int k = 0; k < 2; k++) std::fprintf(out, " %.17g %.17g %.17g", r.egoPoints[k][0], r.egoPoints[k][1], r.egoPoints[k][2]);
    size_t shown = 0;
    for (size_t i = 0; i < r.ids.size(); i++) {
      std::fprintf(out, " %d:%d:%d:%d:%.9g:%.9g:%.9g:%.17g:%.17g", r.ids[i], r.trackManage[i], (int)r.isStaticVec[i], (int)r.isVisVec[i], (double)r.targetPoints[i].x,
                   (double)r.targetPoints[i].y, (double)r.targetPoints[i].z, r.targetVandYaw[i][0], r.targetVandYaw[i][1]);
      if (r.isVisVec[i]) {
        const pcl::PointCloud<pcl::PointXYZ>& bb = r.visBBs[shown++];
        for (int k = 0; k < 8; k++) std::fprintf(out, ":%.9g:%.9g:%.9g", (double)bb[k].x, (double)bb[k].y, (double)bb[k].z);
      }
    }
    std::fprintf(out, "\n");
  }
  std::fclose(in); std::fclose(out);
  return 0;
}
