// tf_to_sensor_driver.cpp — TEST DRIVER (not product code): the tracking node's way back into the sensor frame, as the node itself calls it.
//
// Per case: broadcast the ego pose as StampedTransform(transform, stamp, "velodyne", "global") (OT/tracking/main.cpp:76-83), then take a cloud whose
// frame_id is "global" through pcl_ros::transformPointCloud("/velodyne", ...) with the listener (:183-184), on the tf / pcl_ros restatement of
// oracle/ref_shim and the reference's vendored Eigen. tests/test_emu_sensor_tracks.py compares the points with the library's restated matrix;
// tests/golden/make_tf_sensor_golden.py records 64 cases as tests/golden/tf_to_sensor.npz.
//
//   tf_to_sensor_driver IN.bin OUT.bin
//
// IN.bin: int32 cases, int32 points per case; per case float64 x, y, yaw, then float32 points[n][3]. OUT.bin: float32 images[cases][n][3].
#include <cstdio>
#include <vector>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl_ros/transforms.h>
#include <tf/transform_broadcaster.h>
#include <tf/transform_listener.h>

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s IN.bin OUT.bin\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::perror("open"); return 2; }
  int head[2];
  if (std::fread(head, 4, 2, in) != 2) return 2;
  const int cases = head[0], n = head[1];
  tf::TransformBroadcaster br;
  tf::TransformListener listener(ros::Duration(100));
  std::vector<float> pts((size_t)n * 3), img((size_t)n * 3);
  for (int k = 0; k < cases; k++) {
    double pose[3];
    if (std::fread(pose, 8, 3, in) != 3 || std::fread(pts.data(), 4, pts.size(), in) != pts.size()) return 2;
    tf::Transform transform;
    transform.setOrigin(tf::Vector3(pose[0], pose[1], 0.0));
    tf::Quaternion q;
    q.setRPY(0, 0, pose[2]);
    transform.setRotation(q);
    br.sendTransform(tf::StampedTransform(transform, ros::Time(), "velodyne", "global"));
    pcl::PointCloud<pcl::PointXYZ> cloud, local;
    cloud.header.frame_id = "global";
    for (int i = 0; i < n; i++) cloud.push_back(pcl::PointXYZ(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]));
    if (!pcl_ros::transformPointCloud("/velodyne", cloud, local, listener) || (int)local.size() != n) return 3;
    for (int i = 0; i < n; i++) { img[3 * i] = local[i].x; img[3 * i + 1] = local[i].y; img[3 * i + 2] = local[i].z; }
    if (std::fwrite(img.data(), 4, img.size(), out) != img.size()) return 2;
  }
  std::fclose(in); std::fclose(out);
  return 0;
}
