// `tracking` node (ROS name obj_track) of package object_tracking on the MI355X library: same topics, tf traffic and
// message contents as OT/tracking/main.cpp (subscribes track_box and /gps/odom; broadcasts tf velodyne -> global; publishes
// the ARROW / POINTS markers on visualization_marker; advertises output and visualization_marker2, which stay silent).
//
// The whole callback is one library call (mot_tracking_node_frame): the ego dead reckoning, the boxes' change of frame velodyne -> global, the IMM-UKF-PDA
// step over all tracks of the stream and the live tracks' way back into the sensor frame run on the GPU — the frame changes in the arithmetic of the tf /
// pcl_ros calls the reference makes, bit for bit (csrc/mot_api_tracks.hip: tf_velodyne_to_global, tf_global_to_velodyne). The node broadcasts the tf from the
// origin it gets back and draws from sensor-frame records; it has no listener.
#include <cmath>

#include <nav_msgs/Odometry.h>
#include <object_tracking/trackbox.h>
#include <tf/transform_broadcaster.h>
#include <visualization_msgs/Marker.h>

#include "mot_ros_common.hpp"
#include "mot_ros_markers.hpp"

namespace {

class TrackingNode {
 public:
  TrackingNode(ros::NodeHandle& nh, ros::NodeHandle& pnh) {
    settings_ = mot_ros::settings(pnh);
    mot_params prm;
    if (mot_params_preset(settings_.preset, &prm) != MOT_OK) throw std::runtime_error("unknown preset");
    ctx_ = mot_ros::create(prm, settings_);
    cloud_pub_ = nh.advertise<sensor_msgs::PointCloud2>("output", 1);
    marker_pub_ = nh.advertise<visualization_msgs::Marker>("visualization_marker", 0);
    marker2_pub_ = nh.advertise<visualization_msgs::Marker>("visualization_marker2", 0);
    boxes_sub_ = nh.subscribe("track_box", 160, &TrackingNode::on_boxes, this);
    odom_sub_ = nh.subscribe("/gps/odom", 1000, &TrackingNode::on_odometry, this);
  }
  ~TrackingNode() { mot_destroy(ctx_); }

 private:
  // speed over ground and the raw orientation.z the reference reads as yaw (main.cpp:395-410)
  void on_odometry(const nav_msgs::Odometry& odom) {
    const double vx = odom.twist.twist.linear.x, vy = odom.twist.twist.linear.y;
    ego_yaw_ = odom.pose.pose.orientation.z;
    ego_speed_ = std::sqrt(vx * vx + vy * vy);
  }

  void on_boxes(const object_tracking::trackbox& msg) {
    const ros::Time stamp = msg.header.stamp;
    const double timestamp = stamp.toSec();

    // the message's corners, box by box, in the sensor frame
    const int n_boxes = msg.box_num;
    const std::vector<float>* corner[8] = {&msg.x1, &msg.x2, &msg.x3, &msg.x4, &msg.y1, &msg.y2, &msg.y3, &msg.y4};
    boxes_.resize(24 * (size_t)n_boxes + 24);
    for (int b = 0; b < n_boxes; b++)
      for (int k = 0; k < 8; k++)
        for (int a = 0; a < 3; a++) boxes_[(size_t)(b * 8 + k) * 3 + a] = (*corner[k])[3 * b + a];

    mot_tracking_frame frame;
    mot_ros::tracking_frame_or_restart(ctx_, 0, boxes_.data(), n_boxes, timestamp, ego_speed_, ego_yaw_, &frame);

    // the ego pose the step ran with, broadcast as velodyne -> global
    tf::Quaternion heading;
    heading.setRPY(0, 0, frame.origin6[2]);
    tf::Transform ego;
    ego.setOrigin(tf::Vector3(frame.origin6[0], frame.origin6[1], 0.0));
    ego.setRotation(heading);
    broadcaster_.sendTransform(tf::StampedTransform(ego, stamp, "velodyne", "global"));

    // the live tracks, already in the sensor frame and in id order: arrows carry the track's index as marker id, dots go by colour
    const int n_live = frame.n_live;
    local_xy_.resize(2 * (size_t)n_live + 2);
    for (int i = 0; i < n_live; i++) { local_xy_[2 * i] = frame.tracks[i].px; local_xy_[2 * i + 1] = frame.tracks[i].py; }
    for (int i = 0; i < n_live; i++)
      if (mot_ros::wants_arrow(frame.tracks[i])) marker_pub_.publish(mot_ros::track_arrow("/velodyne", frame.tracks[i], frame.tracks[i].id, local_xy_[2 * i], local_xy_[2 * i + 1]));
    for (const auto& m : mot_ros::track_dots("velodyne", frame.tracks, n_live, local_xy_.data())) marker_pub_.publish(m);
  }

  mot_ros::Settings settings_;
  mot_ctx* ctx_ = nullptr;
  double ego_speed_ = 0.0, ego_yaw_ = 0.0;
  tf::TransformBroadcaster broadcaster_;
  ros::Publisher cloud_pub_, marker_pub_, marker2_pub_;
  ros::Subscriber boxes_sub_, odom_sub_;
  std::vector<float> boxes_, local_xy_;
};

}  // namespace

int main(int argc, char** argv) {
  ros::init(argc, argv, "obj_track");
  ros::NodeHandle nh, private_nh("~");   // topics and the reference's own parameters: public names; this node's extras: ~device, ~preset, ...
  try {
    TrackingNode node(nh, private_nh);
    ros::spin();
  } catch (const std::exception& e) {   // no GPU, a capacity limit, a malformed message: say so and stop (required="true" in the launch file)
    std::cerr << "obj_track: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}
