// mot_api_tracks.hip — host side of the C-ABI (include/mot.h), everything about tracks: the tf chain's matrices, ego dead reckoning, the tracker step and its getters, the box /
// point links' getters, the per-track point clouds and accumulators, stream resets and snapshots, the exports (global and sensor frame) and the tracking node's callback. Context and helpers: mot_host.h.
#include "mot_host.h"

// The sensor -> global change of frame the tracking node asks tf for (OT/tracking/main.cpp:76-83 broadcast, :143-158
// pcl_ros::transformPointCloud("/global", box, newBox, *tran)), walked down to the float matrix pcl::transformPointCloud
// applies, every step in the arithmetic of the library that performs it in the reference's process:
//   1. tf::Quaternion::setRPY(0, 0, yaw); tf::Transform::setRotation -> Matrix3x3::setRotation            (double, tf LinearMath)
//   2. TransformBroadcaster::sendTransform stores (Transform::getRotation() = Matrix3x3::getRotation, origin)   (double, tf2)
//   3. lookupTransform(global <- velodyne) inverts the stored edge: Transform(q^-1, quatRotate(q^-1, -v))  (double, tf2 BufferCore)
//   4. pcl_ros: Eigen::Quaternionf(q), Eigen::Vector3f(v); Translation * Quaternion -> Affine3f:
//      Eigen's QuaternionBase::toRotationMatrix in FLOAT                                                    (float, Eigen 3.2)
// tf, tf2 and pcl_ros are not part of the reference tree: restated from their published sources, the same restatement the
// node-level oracle runs on (oracle/ref_shim/tf, pcl_ros); tests/test_tf_exact.py compares the fused path's boxes with the
// reference node's own call sequence executed on that shim, bit for bit.
static void tf_set_rotation(const double q[4], double b[3][3]) {   // tf::Matrix3x3::setRotation
  const double d = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const double s = 2.0 / d;
  const double xs = q[0] * s, ys = q[1] * s, zs = q[2] * s;
  const double wx = q[3] * xs, wy = q[3] * ys, wz = q[3] * zs;
  const double xx = q[0] * xs, xy = q[0] * ys, xz = q[0] * zs;
  const double yy = q[1] * ys, yz = q[1] * zs, zz = q[2] * zs;
  b[0][0] = 1.0 - (yy + zz); b[0][1] = xy - wz; b[0][2] = xz + wy;
  b[1][0] = xy + wz; b[1][1] = 1.0 - (xx + zz); b[1][2] = yz - wx;
  b[2][0] = xz - wy; b[2][1] = yz + wx; b[2][2] = 1.0 - (xx + yy);
}
static void tf_get_rotation(const double b[3][3], double e[4]) {   // tf::Matrix3x3::getRotation
  const double trace = b[0][0] + b[1][1] + b[2][2];
  if (trace > 0.0) {
    double s = sqrt(trace + 1.0);
    e[3] = s * 0.5;
    s = 0.5 / s;
    e[0] = (b[2][1] - b[1][2]) * s; e[1] = (b[0][2] - b[2][0]) * s; e[2] = (b[1][0] - b[0][1]) * s;
  } else {
    const int i = b[0][0] < b[1][1] ? (b[1][1] < b[2][2] ? 2 : 1) : (b[0][0] < b[2][2] ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    double s = sqrt(b[i][i] - b[j][j] - b[k][k] + 1.0);
    e[i] = s * 0.5;
    s = 0.5 / s;
    e[3] = (b[k][j] - b[j][k]) * s; e[j] = (b[j][i] + b[i][j]) * s; e[k] = (b[k][i] + b[i][k]) * s;
  }
}
// steps 1 and 2 of either direction: tf::Quaternion::setRPY(0, 0, yaw) — the roll / pitch factors are cos(0) = 1, sin(0) = 0 exactly — and Transform::setRotation ->
// Matrix3x3::setRotation (double, tf LinearMath); TransformBroadcaster::sendTransform stores Transform::getRotation() = Matrix3x3::getRotation (double, tf2)
static void tf_broadcast_rotation(double yaw, double e[4]) {
  const double halfYaw = yaw * 0.5;
  const double cosYaw = cos(halfYaw), sinYaw = sin(halfYaw);
  const double cosPitch = 1.0, sinPitch = 0.0, cosRoll = 1.0, sinRoll = 0.0;
  const double q[4] = {sinRoll * cosPitch * cosYaw - cosRoll * sinPitch * sinYaw, cosRoll * sinPitch * cosYaw + sinRoll * cosPitch * sinYaw,
                       cosRoll * cosPitch * sinYaw - sinRoll * sinPitch * cosYaw, cosRoll * cosPitch * cosYaw + sinRoll * sinPitch * sinYaw};
  double b[3][3];
  tf_set_rotation(q, b);
  tf_get_rotation(b, e);
}
// the last steps of either direction: the looked-up StampedTransform is a Transform(q, v), i.e. q becomes a matrix once more; pcl_ros::transformPointCloud(cloud, cloud,
// tf::Transform) takes transform.getRotation() -> Eigen::Quaternionf, origin -> Eigen::Vector3f (double -> float), and Translation3f * Quaternionf is Eigen's
// QuaternionBase::toRotationMatrix in FLOAT (Eigen 3.2)
static void tf_looked_up_matrix(const double q[4], const double v[3], float m[12]) {
  double b2[3][3], q2[4];
  tf_set_rotation(q, b2);
  tf_get_rotation(b2, q2);
  const float fx = (float)q2[0], fy = (float)q2[1], fz = (float)q2[2], fw = (float)q2[3];
  const float tx = 2.0f * fx, ty = 2.0f * fy, tz = 2.0f * fz;
  const float twx = tx * fw, twy = ty * fw, twz = tz * fw;
  const float txx = tx * fx, txy = ty * fx, txz = tz * fx;
  const float tyy = ty * fy, tyz = tz * fy, tzz = tz * fz;
  m[0] = 1.0f - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy; m[3] = (float)v[0];
  m[4] = txy + twz; m[5] = 1.0f - (txx + tzz); m[6] = tyz - twx; m[7] = (float)v[1];
  m[8] = txz - twy; m[9] = tyz + twx; m[10] = 1.0f - (txx + tyy); m[11] = (float)v[2];
}
void tf_velodyne_to_global(double x, double y, double yaw, float m[12]) {
  double e[4];
  tf_broadcast_rotation(yaw, e);
  // 3. inverse edge: qi = (-x, -y, -z, w); v' = quatRotate(qi, -v) = ((qi * (-v)) * qi^-1).xyz
  const double qi[4] = {-e[0], -e[1], -e[2], e[3]};
  const double w[3] = {-x, -y, -0.0};
  const double t[4] = {qi[3] * w[0] + qi[1] * w[2] - qi[2] * w[1], qi[3] * w[1] + qi[2] * w[0] - qi[0] * w[2],
                       qi[3] * w[2] + qi[0] * w[1] - qi[1] * w[0], -qi[0] * w[0] - qi[1] * w[1] - qi[2] * w[2]};   // Quaternion * Vector3
  const double r[4] = {-qi[0], -qi[1], -qi[2], qi[3]};                                                               // qi.inverse()
  const double v[3] = {t[3] * r[0] + t[0] * r[3] + t[1] * r[2] - t[2] * r[1], t[3] * r[1] + t[1] * r[3] + t[2] * r[0] - t[0] * r[2],
                       t[3] * r[2] + t[2] * r[3] + t[0] * r[1] - t[1] * r[0]};                                      // Quaternion * Quaternion, xyz
  tf_looked_up_matrix(qi, v, m);   // 4.
}

// The way back: the float 3 x 4 matrix that pcl_ros::transformPointCloud("/velodyne", cloud_in_global, cloud_out, listener) applies after the node has broadcast
// StampedTransform(transform, stamp, "velodyne", "global") (OT/tracking/main.cpp:76-83, 183-184, 195): what takes targetPoints and every visBBs[i] back into the
// sensor frame. The lookup velodyne <- global walks the stored edge AS IT LIES (global is the child of velodyne), so nothing is inverted here — and this is not
// inverse(tf_velodyne_to_global): that matrix went through a quaternion inversion and a quatRotate this one never sees. Same slices of tf, tf2 and pcl_ros as above
// (oracle/ref_shim); tests/test_emu_sensor_tracks.py compares with the node's own call sequence on that shim, bit for bit.
static void tf_global_to_velodyne(double x, double y, double yaw, float m[12]) {
  double e[4];
  tf_broadcast_rotation(yaw, e);
  // 3. BufferCore's walk from "global" up to "velodyne" meets that one edge, child to parent: TransformAccum starts from the identity and its first (only)
  //    accumulation step takes the stored (quaternion, vector) over unchanged
  const double v[3] = {x, y, 0.0};
  tf_looked_up_matrix(e, v, m);   // 4., 5.
}

// ------------------------------------------------------------------------------------------ tracker
TrackBuffers track_buffers(mot_ctx* c, bool fused) {
  TrackBuffers t;
  t.tracks = c->d_tracks; t.nt = c->d_nt; t.boxes = c->d_tboxes; t.args = c->d_targs; t.gate = c->d_gate; t.prog = c->d_prog;
  t.live = c->d_live; t.out = c->d_tout; t.flags = c->d_tflags; t.m_dev = fused ? c->d_counts : nullptr; t.T = c->max_tracks_total;
  t.box_stride = (long)kMaxBoxesPerFrame * 24; t.step_mode = c->tracker_mode;
  t.nlive = c->d_nlive; t.pos = c->d_pos; t.cp = c->d_cp; t.items = c->d_items; t.n_items = c->d_nitems;
  t.owner = c->track_links ? c->d_owner : nullptr; t.owner_n = c->track_links ? c->d_owner_n : nullptr;
  t.slot_of = c->d_slot_of; t.tomb = c->d_tomb; t.used = c->d_used; t.zomb = c->d_zomb; t.nzomb = c->d_nzomb; t.E = c->max_tracks_ever;
  // fused path: the box stage's boxes (sensor frame) become the tracker's input through the dead-reckoned ego pose
  t.boxes_sensor = fused ? c->d_boxes : nullptr; t.ego = fused ? c->d_ego : nullptr; t.boxes_out = fused ? c->d_tboxes : nullptr;
  t.tp.gamma_g = c->params.gamma_g; t.tp.p_g = c->params.p_g; t.tp.p_d = c->params.p_d; t.tp.distance_thres = c->params.distance_thres;
  t.tp.bb_yaw_change_thres = c->params.bb_yaw_change_thres; t.tp.seed_px = c->params.seed_px; t.tp.seed_py = c->params.seed_py;
  t.tp.life_time_thres = c->params.life_time_thres; t.tp.seed_box_index = c->params.seed_box_index;
  return t;
}

// getOriginPoints(), OT/tracking/imm_ukf_jpda.cpp:74-172. Scalar dead reckoning, kept on the host (its cos/sin are the
// same libm calls the reference makes). The reference replays the whole delta history every frame (:137-151); every
// replay repeats the previous one and appends one step, so the running state is carried instead — same operations,
// same values.
extern "C" int mot_ego_update(mot_ctx* c, int slot, double timestamp, double v_gps, double yaw_gps, double* origin6) {
  if (!c) return MOT_E_ARG;
  if (slot < 0 || slot >= c->batch) return fail(c, MOT_E_ARG, "slot out of range");
  mot_ctx::SlotEgo& e = c->ego[slot];
  double dt = (timestamp - e.timestamp) / 1000000.0;
  e.egoVelo = v_gps;
  e.egoYaw = yaw_gps;
  e.egoYaw += c->params.first_ego_yaw_offset;
  e.ego_called = true;
  if (!e.init) {
    e.egoPoint[0] = 0; e.egoPoint[1] = 0; e.egoPoint[2] = e.egoYaw;
    if (origin6) { origin6[0] = 0; origin6[1] = 0; origin6[2] = e.egoYaw; origin6[3] = 0; origin6[4] = 0; origin6[5] = e.egoYaw + M_PI / 2; }
    return MOT_OK;
  }
  double diffYaw = (e.egoYaw - e.egoPreYaw);
  double dX = dt * e.egoVelo * cos(diffYaw);
  double dY = dt * e.egoVelo * sin(diffYaw);
  double x = e.rx, y = e.ry, egoYaw = e.ryaw;
  x -= dX;
  y -= dY;
  double preX = x, preY = y;
  double yaw = diffYaw * -1;
  egoYaw += yaw;
  x = cos(yaw) * preX - sin(yaw) * preY;
  y = sin(yaw) * preX + cos(yaw) * preY;
  e.rx = x; e.ry = y; e.ryaw = egoYaw;
  e.egoPoint[0] = x; e.egoPoint[1] = y; e.egoPoint[2] = egoYaw;
  if (origin6) { origin6[0] = x; origin6[1] = y; origin6[2] = egoYaw; origin6[3] = x; origin6[4] = y; origin6[5] = egoYaw + M_PI / 2; }
  return MOT_OK;
}

// fills the per-slot launch arguments and advances the host-side copies of timestamp_ / egoPreYaw_ / init_
void prepare_track_args(mot_ctx* c, TrackFrameArgs* targs, int slot, int m, double timestamp, bool run) {
  mot_ctx::SlotEgo& e = c->ego[slot];
  TrackFrameArgs& a = targs[slot];
  a.m = m; a.run = run ? 1 : 0; a.pad = 0;
  a.first_frame = (e.init && !e.tracks_restart) ? 0 : 1;
  if (run) e.tracks_restart = false;
  a.dt = (timestamp - e.timestamp) / 1000000.0;
  a.ego_yaw = e.egoPoint[2];
  if (run) e.step_ego_yaw = e.egoPoint[2];
  if (run) { e.timestamp = timestamp; e.egoPreYaw = e.egoYaw; e.init = true; }
}

int pinned_scratch(mot_ctx* c, size_t bytes, char** out) {
  if (c->h_pin_bytes < bytes) {
    MOT_TRY(release(c, &c->h_pin));
    c->h_pin_bytes = 0;
    const size_t want = (bytes + 65535) & ~(size_t)65535;
    MOT_TRY(pinned_alloc(c, &c->h_pin, want));
    c->h_pin_bytes = want;
  }
  *out = c->h_pin;
  return MOT_OK;
}

// The tracker's capacity flag of a stream is STICKY: once a birth has been dropped the stream keeps answering MOT_E_CAPACITY (the records are still delivered) until the caller
// starts it over with mot_reset / mot_reset_slot / mot_reset_tracks_slot — a caller that ignores one error is told again on every call, not only at the next dropped birth.
// fused_feeds: the caller's stream may be fed by the fused path, whose refused frames raise the flag too.
static int sticky_capacity(mot_ctx* c, int sticky, bool fused_feeds) {
  if (!sticky) return MOT_OK;
  c->err = std::string("a stream ran out of track slots (more than max_tracks_total tracks alive or just dead) or of its lifetime track budget "
                       "(mot_params.max_tracks_ever): births are being dropped") +
           (fused_feeds ? "; or a fused frame of the stream was refused for capacity (see mot_get_boxes) and the tracker stepped on an incomplete box list" : "") +
           "; mot_reset_tracks_slot() starts its tracks over";
  return MOT_E_CAPACITY;
}

extern "C" int mot_get_tracks(mot_ctx* c, int slot, mot_track* tracks, int max_tracks, int* n_tracks) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || !n_tracks || max_tracks < 0) return fail(c, MOT_E_ARG, "mot_get_tracks: slot out of range, null n_tracks or negative max_tracks");
  const size_t T = c->max_tracks_total, E = c->max_tracks_ever, usedW = (T + 63) / 64;
  const size_t o_used = 16, o_rec = (o_used + usedW * sizeof(unsigned long long) + 15) & ~(size_t)15;
  char* pin;
  MOT_TRY(pinned_scratch(c, o_rec, &pin));
  int* meta = reinterpret_cast<int*>(pin);
  const unsigned long long* used = reinterpret_cast<const unsigned long long*>(pin + o_used);
  MOT_HIP(c, hipMemcpyAsync(&meta[0], c->d_nt + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[1], c->d_tflags + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(pin + o_used, c->d_used + (size_t)slot * usedW, usedW * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const int n = meta[0], sticky = meta[1];
  c->ego[slot].nt = n;
  *n_tracks = n;
  if (n > max_tracks) return fail(c, MOT_E_CAPACITY, "more tracks than the caller's buffer holds");
  if (tracks && n > 0) {
    // One record per track EVER created, in the reference's index order (its output vectors are sized that way,
    // OT/tracking/imm_ukf_jpda.cpp:995-1041). A track that still owns a slot — alive, or dead since the last step only — has its
    // record there; of an evicted one (dead for longer) the position, lifetime_ and the static flag are kept: trackManage 0, not
    // shown, the frozen speed, and the frozen yaw + the current ego yaw, as the reference reports them (every consumer skips dead tracks).
    // Only the slots up to the highest one in use are read back (slots are handed out lowest first).
    size_t hi = 0;
    for (size_t w = 0; w < usedW; w++) if (used[w]) hi = w * 64 + (63 - (size_t)__builtin_clzll(used[w])) + 1;
    if (hi > T) hi = T;
    const size_t o_out = 0, o_slot = o_out + hi * sizeof(mot_track), o_tomb = (o_slot + (size_t)n * sizeof(int) + 15) & ~(size_t)15 /* TrackTomb holds doubles since round 5 */, o_pos = (o_tomb + (size_t)n * sizeof(TrackTomb) + 15) & ~(size_t)15;
    MOT_TRY(pinned_scratch(c, o_rec + o_pos + (size_t)n * sizeof(Vec2d), &pin));   // (may move the scratch: `used` and `meta` are not read again)
    char* h = pin + o_rec;
    if (hi) MOT_HIP(c, hipMemcpyAsync(h + o_out, c->d_tout + (size_t)slot * T, hi * sizeof(mot_track), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipMemcpyAsync(h + o_slot, c->d_slot_of + (size_t)slot * E, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipMemcpyAsync(h + o_tomb, c->d_tomb + (size_t)slot * E, (size_t)n * sizeof(TrackTomb), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipMemcpyAsync(h + o_pos, c->d_pos + (size_t)slot * E, (size_t)n * sizeof(Vec2d), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));
    const mot_track* rec = reinterpret_cast<const mot_track*>(h + o_out);
    const int* slot_of = reinterpret_cast<const int*>(h + o_slot);
    const TrackTomb* tomb = reinterpret_cast<const TrackTomb*>(h + o_tomb);
    const Vec2d* pos = reinterpret_cast<const Vec2d*>(h + o_pos);
    for (int i = 0; i < n; i++) {
      if (slot_of[i] >= 0 && (size_t)slot_of[i] < hi) tracks[i] = rec[slot_of[i]];
      else {
        mot_track o;
        memset(&o, 0, sizeof o);
        o.id = i; o.px = (float)pos[i].x; o.py = (float)pos[i].y; o.pz = (float)(-1.73 / 2);
        o.lifetime = tomb[i].lifetime; o.is_static = tomb[i].is_static;
        // the reference goes on reporting a dead track's frozen speed, and its frozen yaw + the CURRENT ego yaw (:1012-1016)
        o.v = tomb[i].v;
        double tyaw = tomb[i].yaw + c->ego[slot].step_ego_yaw;
        if (fabs(tyaw) > 64. * M_PI) { const double r = tyaw - trunc(tyaw / (2. * M_PI)) * (2. * M_PI); tyaw = fabs(tyaw) < 0x1p55 && fabs(r) <= 64. * M_PI ? r : NAN; }   // (wrap_pi of mot_track_prep.h)
        while (tyaw > M_PI) tyaw -= 2. * M_PI;
        while (tyaw < -M_PI) tyaw += 2. * M_PI;
        o.yaw = tyaw;
        tracks[i] = o;
      }
    }
  }
  return sticky_capacity(c, sticky, true);
}

extern "C" int mot_get_box_tracks(mot_ctx* c, int slot, int32_t* box_track, int max_boxes, int* n_boxes) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || max_boxes < 0 || !n_boxes) return fail(c, MOT_E_ARG, "mot_get_box_tracks: slot or max_boxes out of range, or null n_boxes");
  if (!c->track_links) return fail(c, MOT_E_STATE, "mot_get_box_tracks: track links are off (mot_set_track_links)");
  if (!c->res.box_tracks_valid(slot)) return fail(c, MOT_E_STATE, "mot_get_box_tracks: no tracker step on this slot since the links were turned on");
  if (c->res.point_tracks_valid(slot)) MOT_TRY(fetch_counts(c, slot));   // the step's boxes came from the slot's own frame: a refused frame says so
  char* pin;
  MOT_TRY(pinned_scratch(c, (size_t)(kMaxBoxesPerFrame + 4) * sizeof(int), &pin));
  int* h = reinterpret_cast<int*>(pin);
  MOT_HIP(c, hipMemcpyAsync(h, c->d_owner_n + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(h + 4, c->d_owner + (size_t)slot * kMaxBoxesPerFrame, (size_t)kMaxBoxesPerFrame * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const int n = h[0];
  if (n < 0 || n > kMaxBoxesPerFrame) return fail(c, MOT_E_STATE, "mot_get_box_tracks: inconsistent box count");
  *n_boxes = n;
  if (n > max_boxes) return fail(c, MOT_E_CAPACITY, "more boxes than the caller's buffer holds");
  if (box_track && n > 0) memcpy(box_track, h + 4, (size_t)n * sizeof(int));
  return MOT_OK;
}

extern "C" int mot_get_point_tracks(mot_ctx* c, int slot, int32_t* ids, int capacity, int* n_elevated) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || capacity < 0 || !n_elevated) return fail(c, MOT_E_ARG, "mot_get_point_tracks: slot or capacity out of range, or null n_elevated");
  MOT_TRY(check_point_tracks(c, slot, "mot_get_point_tracks"));
  MOT_TRY(fetch_counts(c, slot));
  const int ne = c->h_counts[slot * kCountsStride + kCntElev];
  *n_elevated = ne;
  if (ne > capacity) return fail(c, MOT_E_CAPACITY, "more elevated points than the caller's id buffer holds");
  if (ids && ne > 0) {
    MOT_HIP(c, hipMemcpyAsync(ids, c->d_point_track + (size_t)slot * c->cap, (size_t)ne * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MOT_OK;
}

// the ids of slots 0..batch-1 into the caller's device block, d_ids[b * stride + i], and every slot's elevated count into d_counts[b]: the link kernel again, on what the
// slots hold, writing there instead of into the library's buffer (the same reads, the same values). Asynchronous on the context stream; a slot with more elevated
// points than `stride` gets the first `stride` ids (d_counts carries the true count). A frame refused for capacity cannot answer MOT_E_CAPACITY here — nothing is
// read back — and reads -1 throughout; mot_get_point_tracks on that slot tells.
extern "C" int mot_export_point_tracks_dev(mot_ctx* c, int batch, int32_t* d_ids, long stride, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!d_ids || !d_counts || batch < 1 || batch > c->batch || stride < 0 || ((size_t)d_ids & 3)) return fail(c, MOT_E_ARG, "mot_export_point_tracks_dev: bad argument");
  for (int b = 0; b < batch; b++) { const int rc = check_point_tracks(c, b, "mot_export_point_tracks_dev"); if (rc) return rc; }
  ClusterBuffers cb = cluster_buffers(c, 0);
  cb.ecell = c->params.num_grid < MOT_MAX_GRID ? c->d_ecell : nullptr;   // (as the fused compaction left them: ground_buffers)
  mot_launch_point_tracks(c->dp, cb, c->d_owner, batch, c->max_points, reinterpret_cast<int*>(d_ids), stride, reinterpret_cast<int*>(d_counts), c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- per-track point clouds (track_points.hip)
// Scratch of the feature's own, at its first call; a failure half-way leaves what exists for mot_destroy and the next call, which resumes. Sized from max_points
// (c->cap is max_points rounded up to 64). Nothing here aliases what a getter reads: the kernels read the ids, the input-order cloud, the counters and the owner
// rows, and write only these buffers and the caller's blocks — MOT_ORDER_ANY's cluster-ordered copy (mot_box_markers reads it later) is not touched.
static int ensure_track_points(mot_ctx* c, bool host_stage) {
  const size_t B = c->batch;
  c->tp_chunks = (c->cap + kTrackPointChunk - 1) / kTrackPointChunk;
  MOT_TRY(dev_alloc(c, &c->d_tp_seg_id, B * kMaxBoxesPerFrame * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tp_seg_boxes, B * kMaxBoxesPerFrame * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tp_seg_n, B * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tp_rows, B * (size_t)c->tp_chunks * kTrackPointKeys * sizeof(int)));
  MOT_TRY(dev_alloc(c, &c->d_tp_tf, B * (sizeof(EgoTf) + sizeof(int))));   // (the matrices, and behind them the step stamps of mot_accumulate_track_points)
  MOT_TRY(c->tp_tf_ring.create(c, B * (sizeof(EgoTf) + sizeof(int))));
  if (host_stage) MOT_TRY(dev_alloc(c, &c->d_tp_stage, (size_t)c->cap * sizeof(mot_track_point) + (size_t)kTrackPointKeys * sizeof(mot_track_segment) + 16));
  return MOT_OK;
}
static int check_track_points_args(mot_ctx* c, const char* who, int flags, int frame) {
  if (flags & ~MOT_TRACK_POINTS_REST) return fail(c, MOT_E_ARG, who, ": unknown flag bits");
  if (frame != MOT_FRAME_GLOBAL && frame != MOT_FRAME_SENSOR) return fail(c, MOT_E_ARG, who, ": frame must be MOT_FRAME_GLOBAL or MOT_FRAME_SENSOR");
  return MOT_OK;
}
// the four kernels over slots first .. first + n - 1, block k of the caller's buffers for slot first + k; one launch per run of slots of one cloud layout (for_layout_runs)
static int launch_track_points(mot_ctx* c, int first, int n, int flags, int frame, mot_track_point* d_points, long point_stride, mot_track_segment* d_segments, int max_segments,
                               int* d_counts) {
  const EgoTf* tf = nullptr;
  if (frame == MOT_FRAME_GLOBAL) MOT_TRY(send_link_tf(c, &c->tp_tf_ring, c->d_tp_tf, first, n, nullptr, &tf));
  TrackPointBuffers t = track_point_buffers(c);
  for_layout_runs(c, first, n, [&](int k0, int k1, int packed) {
    t.elevated_packed = packed;
    mot_launch_track_points(t, first + k0, k1 - k0, c->max_points, flags & MOT_TRACK_POINTS_REST, tf ? tf + k0 : nullptr, d_points + (long)k0 * point_stride, point_stride,
                            d_segments + (long)k0 * max_segments, max_segments, d_counts + 2 * k0, c->stream);
  });
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_export_track_points_dev(mot_ctx* c, int batch, int flags, int frame, mot_track_point* d_points, long point_stride, mot_track_segment* d_segments, int max_segments,
                                           int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_track_points_dev";
  MOT_TRY(check_track_points_args(c, who, flags, frame));
  if (!d_points || !d_segments || !d_counts || batch < 1 || batch > c->batch || point_stride < 0 || max_segments < 0 || (((size_t)d_points | (size_t)d_segments | (size_t)d_counts) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument");
  for (int b = 0; b < batch; b++) MOT_TRY(check_point_tracks(c, b, who));
  MOT_TRY(ensure_track_points(c, false));
  return launch_track_points(c, 0, batch, flags, frame, d_points, point_stride, d_segments, max_segments, reinterpret_cast<int*>(d_counts));
}

extern "C" int mot_get_track_points(mot_ctx* c, int slot, int flags, int frame, mot_track_point* points, int point_capacity, mot_track_segment* segments, int max_segments,
                                    int* n_points, int* n_segments) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_track_points";
  MOT_TRY(check_track_points_args(c, who, flags, frame));
  if (slot < 0 || slot >= c->batch || point_capacity < 0 || max_segments < 0 || !n_points || !n_segments) return fail(c, MOT_E_ARG, who, ": slot or a capacity out of range, or a null count");
  MOT_TRY(check_point_tracks(c, slot, who));
  MOT_TRY(ensure_track_points(c, true));
  MOT_TRY(fetch_counts(c, slot));   // a refused frame says so
  // the slot alone into the staging block — [cap records][1025 segments][2 counts] — with the block's own capacities; what fits the caller's buffers is decided here
  mot_track_point* d_pts = reinterpret_cast<mot_track_point*>(c->d_tp_stage);
  mot_track_segment* d_seg = reinterpret_cast<mot_track_segment*>(c->d_tp_stage + (size_t)c->cap * sizeof(mot_track_point));
  int* d_cnt = reinterpret_cast<int*>(d_seg + kTrackPointKeys);
  MOT_TRY(launch_track_points(c, slot, 1, flags, frame, d_pts, c->cap, d_seg, kTrackPointKeys, d_cnt));
  int h[2];
  MOT_TRY(read_counts(c, d_cnt, 2, h));
  const int ns = h[0], np = h[1];
  if (ns < 0 || ns > kTrackPointKeys || np < 0 || np > c->cap) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  *n_segments = ns; *n_points = np;
  if (np > point_capacity) return fail(c, MOT_E_CAPACITY, "more points than the caller's point buffer holds");
  if (ns > max_segments) return fail(c, MOT_E_CAPACITY, "more segments than the caller's segment buffer holds");
  if (points && np > 0) MOT_HIP(c, hipMemcpyAsync(points, d_pts, (size_t)np * sizeof(mot_track_point), hipMemcpyDeviceToHost, c->stream));
  if (segments && ns > 0) MOT_HIP(c, hipMemcpyAsync(segments, d_seg, (size_t)ns * sizeof(mot_track_segment), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- per-track accumulators (track_accum.hip)
// The setter owns the feature's memory: rows, the two rings and the plan are allocated together and released together (off, or another geometry). The scratch
// the kernels share with the per-track point clouds (distinct owners, per-chunk rows, matrices + step stamps) is ensure_track_points', at the first accumulate call.
static bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }
static int accum_release(mot_ctx* c, mot_accum_row** rows, mot_accum_point** points, mot_accum_obs** obs, TrackAccumPlan** plan) {
  MOT_TRY(release(c, rows)); MOT_TRY(release(c, points)); MOT_TRY(release(c, obs));
  return release(c, plan);
}
// what the track models took at their first call goes with the tables it was sized for (the caller has drained the stream)
static int track_models_release(mot_ctx* c) {
  MOT_TRY(release(c, &c->d_tm_latest)); MOT_TRY(release(c, &c->tm_ring.base)); MOT_TRY(release(c, &c->d_tm_stage)); MOT_TRY(release(c, &c->d_tm_points));
  MOT_TRY(release(c, &c->d_tv_scratch)); MOT_TRY(release(c, &c->d_tv_stage)); MOT_TRY(release(c, &c->d_tv_voxels));
  for (bool& u : c->tm_ring.used) u = false;
  c->tm_points_cap = 0; c->tv_voxels_cap = 0;
  return MOT_OK;
}
// what mot_sequence_accumulate_dev took at its first call: both blocks or neither
static int seq_accum_release(mot_ctx* c) {
  MOT_TRY(release(c, &c->d_tas_cap));
  return release(c, &c->d_tas_seg);
}
int accum_restart_slots(mot_ctx* c, int first, int n) {
  if (!c->accum_K) return MOT_OK;
  mot_launch_track_accum_clear(c->d_ta_rows, (long)first * c->max_tracks_total, (long)n * c->max_tracks_total, c->stream);
  MOT_HIP(c, hipGetLastError());
  for (int b = first; b < first + n; b++) { c->accum_step[b] = 0; c->res.step_accumulated(b); }
  return MOT_OK;
}
extern "C" int mot_set_track_accumulation(mot_ctx* c, int points_per_track, int obs_per_track) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_set_track_accumulation";
  const int K = points_per_track, O = obs_per_track;
  if (K == 0) {   // off: nothing may still read the tables
    if (!c->accum_K) return MOT_OK;
    MOT_HIP(c, hipStreamSynchronize(c->stream));
    c->accum_K = c->accum_O = 0;
    MOT_TRY(track_models_release(c));
    MOT_TRY(seq_accum_release(c));
    return accum_release(c, &c->d_ta_rows, &c->d_ta_points, &c->d_ta_obs, &c->d_ta_plan);
  }
  if (!pow2_in(K, 64, 1 << 20)) return fail(c, MOT_E_ARG, who, ": points_per_track must be 0 (off) or a power of two in [64, 2^20]");
  if (O != 0 && !pow2_in(O, 1, 4096)) return fail(c, MOT_E_ARG, who, ": obs_per_track must be 0 or a power of two in [1, 4096]");
  MOT_TRY(check_links_on(c, who));
  if (K == c->accum_K && O == c->accum_O) return MOT_OK;
  // the new tables first: a failure leaves the mode, an earlier geometry included, as it was
  const size_t rows_n = (size_t)c->batch * c->max_tracks_total;
  mot_accum_row* d_accum_rows = nullptr; mot_accum_point* d_accum_points = nullptr; mot_accum_obs* d_accum_obs = nullptr; TrackAccumPlan* d_accum_plan = nullptr;
  int rc = dev_alloc(c, &d_accum_rows, rows_n * sizeof(mot_accum_row));
  if (!rc) rc = dev_alloc(c, &d_accum_points, rows_n * (size_t)K * sizeof(mot_accum_point));
  if (!rc && O) rc = dev_alloc(c, &d_accum_obs, rows_n * (size_t)O * sizeof(mot_accum_obs));
  if (!rc) rc = dev_alloc(c, &d_accum_plan, (size_t)c->batch * kMaxBoxesPerFrame * sizeof(TrackAccumPlan));
  if (rc) {
    const std::string why = c->err;
    (void)accum_release(c, &d_accum_rows, &d_accum_points, &d_accum_obs, &d_accum_plan);
    c->err = why;
    return rc;
  }
  if (c->accum_K) {
    MOT_HIP(c, hipStreamSynchronize(c->stream));
    MOT_TRY(track_models_release(c));
    MOT_TRY(seq_accum_release(c));
    MOT_TRY(accum_release(c, &c->d_ta_rows, &c->d_ta_points, &c->d_ta_obs, &c->d_ta_plan));
  }
  c->d_ta_rows = d_accum_rows; c->d_ta_points = d_accum_points; c->d_ta_obs = d_accum_obs; c->d_ta_plan = d_accum_plan;
  c->accum_K = K; c->accum_O = O;
  c->accum_step.assign(c->batch, 0);
  return accum_restart_slots(c, 0, c->batch);   // every row empty; the steps the slots hold were taken without the feature: the next fused call is the first to append
}

static int check_accum_on(mot_ctx* c, const char* who) { return c->accum_K ? MOT_OK : fail(c, MOT_E_STATE, who, ": the per-track accumulators are off (mot_set_track_accumulation)"); }

// the accumulators as the kernels see them: every stream's tables, i.e. stream 0's for a recorded drive (steps: the live launch's stamps, set per run)
static TrackAccumBuffers accum_buffers(const mot_ctx* c) {
  TrackAccumBuffers a;
  a.rows = c->d_ta_rows; a.points = c->d_ta_points; a.obs = c->d_ta_obs; a.plan = c->d_ta_plan; a.slot_of = c->d_slot_of; a.out = c->d_tout; a.steps = nullptr;
  a.T = c->max_tracks_total; a.E = c->max_tracks_ever; a.K = c->accum_K; a.O = c->accum_O;
  return a;
}

extern "C" int mot_accumulate_track_points(mot_ctx* c, int batch) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_accumulate_track_points";
  MOT_TRY(check_accum_on(c, who));
  if (batch < 1 || batch > c->batch) return fail(c, MOT_E_ARG, who, ": batch out of range");
  for (int b = 0; b < batch; b++) {   // every slot before anything is launched or counted
    MOT_TRY(check_point_tracks(c, b, who));
    if (c->res.sequence_frame(b)) return fail(c, MOT_E_STATE, who, ": the slots hold the frames of ONE stream (mot_sequence_dev); the accumulators do not support sequence mode");
    if (c->res.accumulated(b)) return fail(c, MOT_E_STATE, who, ": a slot of the batch was already accumulated for its current step, or was reset / loaded since that step");
  }
  MOT_TRY(ensure_track_points(c, false));
  const EgoTf* d_tf; const int* d_steps;   // the matrices the slots' boxes took and the slots' step stamps
  MOT_TRY(send_link_tf(c, &c->tp_tf_ring, c->d_tp_tf, 0, batch, &c->accum_step, &d_tf, &d_steps));
  TrackPointBuffers t = track_point_buffers(c);
  TrackAccumBuffers a = accum_buffers(c);
  for_layout_runs(c, 0, batch, [&](int k0, int k1, int packed) {
    t.elevated_packed = packed;
    a.steps = d_steps + k0;
    mot_launch_track_accum(t, a, k0, k1 - k0, c->max_points, d_tf + k0, c->stream);
  });
  MOT_HIP(c, hipGetLastError());
  for (int b = 0; b < batch; b++) { c->accum_step[b]++; c->res.step_accumulated(b); }
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- the accumulators fed by sequence mode (track_accum_seq.hip)
// mot_sequence_accumulate_dev is mot_sequence_dev's body (mot_api.hip) with these three hooks. The scratch of the feature's own — the capture table and the plan,
// 72 KB per slot — is taken at the first call, both blocks or neither (a failure leaves the live allocations as they were), and goes with the accumulators.
int seq_accum_ready(mot_ctx* c, const char* who) {
  MOT_TRY(check_accum_on(c, who));
  MOT_TRY(check_links_on(c, who));
  MOT_TRY(ensure_track_points(c, false));
  if (c->d_tas_cap && c->d_tas_seg) return MOT_OK;
  const size_t n = (size_t)c->batch * kMaxBoxesPerFrame;
  int rc = dev_alloc(c, &c->d_tas_cap, n * sizeof(TrackAccumCapture));
  if (!rc) rc = dev_alloc(c, &c->d_tas_seg, n * sizeof(TrackAccumSeqSeg));
  if (rc) {
    const std::string why = c->err;
    (void)seq_accum_release(c);
    c->err = why;
  }
  return rc;
}
void seq_accum_capture(mot_ctx* c, int frame) { mot_launch_track_accum_capture(c->d_counts, c->d_owner, accum_buffers(c), c->d_tas_cap, frame, c->stream); }
int seq_accum_append(mot_ctx* c, int frames, int max_n) {
  const TrackPointBuffers t = track_point_buffers(c);   // (slot 0's layout: one fused call filled the slots)
  const TrackAccumSeqBuffers s = {c->d_tas_cap, c->d_tas_seg, c->accum_step[0]};
  // frame k's matrix is entry k of the call's own argument block (what link_tf[k] keeps on the host): later calls rewrite it behind these kernels, stream-ordered
  mot_launch_track_accum_sequence(t, accum_buffers(c), s, frames, max_n, c->d_ego, c->stream);
  MOT_HIP(c, hipGetLastError());
  c->accum_step[0] += frames;   // (a frame refused for capacity appended nothing and counts)
  c->res.sequence_accumulated(frames);
  return MOT_OK;
}

extern "C" int mot_track_accumulators_dev(mot_ctx* c, mot_accum_view* out) {
  if (!c) return MOT_E_ARG;
  if (!out) return fail(c, MOT_E_ARG, "mot_track_accumulators_dev: null result");
  MOT_TRY(check_accum_on(c, "mot_track_accumulators_dev"));
  out->d_rows = c->d_ta_rows; out->d_points = c->d_ta_points; out->d_obs = c->d_ta_obs;
  out->tracks_per_slot = c->max_tracks_total; out->points_per_track = c->accum_K; out->obs_per_track = c->accum_O; out->max_batch = c->batch;
  return MOT_OK;
}

extern "C" int mot_get_accum_rows(mot_ctx* c, int slot, mot_accum_row* rows, int max_rows, int* n_rows) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_accum_rows";
  if (slot < 0 || slot >= c->batch || max_rows < 0 || !n_rows) return fail(c, MOT_E_ARG, who, ": slot or max_rows out of range, or null n_rows");
  MOT_TRY(check_accum_on(c, who));
  const int T = c->max_tracks_total;
  *n_rows = T;
  if (T > max_rows) return fail(c, MOT_E_CAPACITY, "more rows (max_tracks_total) than the caller's buffer holds");
  if (rows) {
    MOT_HIP(c, hipMemcpyAsync(rows, c->d_ta_rows + (size_t)slot * T, (size_t)T * sizeof(mot_accum_row), hipMemcpyDeviceToHost, c->stream));
    MOT_HIP(c, hipStreamSynchronize(c->stream));
  }
  return MOT_OK;
}

extern "C" int mot_get_track_accumulated(mot_ctx* c, int slot, int track_id, mot_accum_row* row, mot_accum_point* points, int point_capacity, int* n_points,
                                         mot_accum_obs* obs, int obs_capacity, int* n_obs) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_track_accumulated";
  if (slot < 0 || slot >= c->batch || track_id < 0 || point_capacity < 0 || obs_capacity < 0 || !n_points || !n_obs)
    return fail(c, MOT_E_ARG, who, ": slot, track_id or a capacity out of range, or a null count");
  MOT_TRY(check_accum_on(c, who));
  const size_t T = c->max_tracks_total, K = c->accum_K, O = c->accum_O;
  char* pin;
  MOT_TRY(pinned_scratch(c, T * sizeof(mot_accum_row), &pin));
  MOT_HIP(c, hipMemcpyAsync(pin, c->d_ta_rows + (size_t)slot * T, T * sizeof(mot_accum_row), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_accum_row* rows = reinterpret_cast<const mot_accum_row*>(pin);
  size_t r = 0;
  while (r < T && rows[r].track_id != track_id) r++;
  if (r == T) return fail(c, MOT_E_STATE, who, ": no accumulator holds this track (never accumulated, or its track slot went to another track)");
  const mot_accum_row found = rows[r];
  const size_t np = found.total < K ? (size_t)found.total : K, no = O ? ((size_t)found.obs_total < O ? (size_t)found.obs_total : O) : 0;
  *n_points = (int)np; *n_obs = (int)no;
  if (points && np > (size_t)point_capacity) return fail(c, MOT_E_CAPACITY, "more accumulated points than the caller's point buffer holds");
  if (obs && no > (size_t)obs_capacity) return fail(c, MOT_E_CAPACITY, "more observations than the caller's observation buffer holds");
  if (row) *row = found;
  // the ring unrolled, oldest first: [oldest, kept) then [0, oldest)
  const size_t at = (size_t)slot * T + r;
  if (points && np) {
    const size_t oldest = found.total > K ? (size_t)(found.total & (K - 1)) : 0;
    const mot_accum_point* ring = c->d_ta_points + at * K;
    MOT_HIP(c, hipMemcpyAsync(points, ring + oldest, (np - oldest) * sizeof(mot_accum_point), hipMemcpyDeviceToHost, c->stream));
    if (oldest) MOT_HIP(c, hipMemcpyAsync(points + (np - oldest), ring, oldest * sizeof(mot_accum_point), hipMemcpyDeviceToHost, c->stream));
  }
  if (obs && no) {
    const size_t oldest = (size_t)found.obs_total > O ? ((size_t)found.obs_total & (O - 1)) : 0;
    const mot_accum_obs* ring = c->d_ta_obs + at * O;
    MOT_HIP(c, hipMemcpyAsync(obs, ring + oldest, (no - oldest) * sizeof(mot_accum_obs), hipMemcpyDeviceToHost, c->stream));
    if (oldest) MOT_HIP(c, hipMemcpyAsync(obs + (no - oldest), ring, oldest * sizeof(mot_accum_obs), hipMemcpyDeviceToHost, c->stream));
  }
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- object-centred track models (track_models.hip)
// Scratch of the feature's own at its first call (a failure half-way leaves what exists for the next call, which resumes), released by the accumulators' setter:
// track_models_release, above. The kernels read the accumulators alone: no slot state is asked.
static int check_track_models(mot_ctx* c, const char* who, int flags) {
  if (flags & ~(MOT_MODEL_AXES | MOT_MODEL_CURRENT)) return fail(c, MOT_E_ARG, who, ": unknown flag bits");
  return MOT_OK;
}
static int check_track_models_on(mot_ctx* c, const char* who) {
  MOT_TRY(check_accum_on(c, who));
  return c->accum_O ? MOT_OK : fail(c, MOT_E_STATE, who, ": the accumulators keep no observations (mot_set_track_accumulation with obs_per_track > 0)");
}
static int ensure_track_models(mot_ctx* c, bool host_stage) {
  MOT_TRY(dev_alloc(c, &c->d_tm_latest, (size_t)c->batch * sizeof(int)));
  MOT_TRY(c->tm_ring.create(c, (size_t)c->batch * sizeof(int)));
  if (host_stage) MOT_TRY(dev_alloc(c, &c->d_tm_stage, (size_t)c->max_tracks_total * sizeof(mot_track_model) + 16));
  return MOT_OK;
}
// the tables as the kernels see them; with MOT_MODEL_CURRENT every slot's latest accumulated step goes ahead of them in one stream-ordered copy
static int track_model_buffers(mot_ctx* c, int flags, TrackModelBuffers* a) {
  if (flags & MOT_MODEL_CURRENT) {
    char* raw;
    MOT_TRY(c->tm_ring.acquire(c, &raw));
    int* latest = reinterpret_cast<int*>(raw);
    for (int b = 0; b < c->batch; b++) latest[b] = c->accum_step[b] - 1;
    MOT_TRY(c->tm_ring.commit(c, c->d_tm_latest, 0, (size_t)c->batch * sizeof(int), c->stream));
  }
  a->rows = c->d_ta_rows; a->points = c->d_ta_points; a->obs = c->d_ta_obs; a->latest = c->d_tm_latest;
  a->T = c->max_tracks_total; a->K = c->accum_K; a->O = c->accum_O;
  return MOT_OK;
}

extern "C" int mot_export_track_models_dev(mot_ctx* c, int batch, int flags, mot_accum_point* d_points, long point_stride, mot_track_model* d_models, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_track_models_dev";
  MOT_TRY(check_track_models(c, who, flags));
  if (!d_models || !d_counts || batch < 1 || batch > c->batch || point_stride < 0 || (!d_points && point_stride > 0) || ((size_t)d_points & 15) ||
      (((size_t)d_models | (size_t)d_counts) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument");
  MOT_TRY(check_track_models_on(c, who));
  MOT_TRY(ensure_track_models(c, false));
  TrackModelBuffers a;
  MOT_TRY(track_model_buffers(c, flags, &a));
  mot_launch_track_models_plan(a, 0, batch, flags, d_models, reinterpret_cast<int*>(d_counts), c->stream);
  mot_launch_track_models_transform(a, 0, batch, flags, d_points, point_stride, d_models, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_get_track_models(mot_ctx* c, int slot, int flags, mot_track_model* models, int max_models, int* n_models, mot_accum_point* points, int point_capacity,
                                    int* n_points) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_track_models";
  MOT_TRY(check_track_models(c, who, flags));
  if (slot < 0 || slot >= c->batch || max_models < 0 || point_capacity < 0 || !n_models || !n_points) return fail(c, MOT_E_ARG, who, ": slot or a capacity out of range, or a null count");
  MOT_TRY(check_track_models_on(c, who));
  MOT_TRY(ensure_track_models(c, true));
  const int T = c->max_tracks_total;
  TrackModelBuffers a;
  MOT_TRY(track_model_buffers(c, flags, &a));
  // the slot's headers and counts into the staging block; the counts decide what fits the caller's buffers before a record moves
  mot_track_model* d_mod = reinterpret_cast<mot_track_model*>(c->d_tm_stage);
  int* d_cnt = reinterpret_cast<int*>(d_mod + T);
  mot_launch_track_models_plan(a, slot, 1, flags, d_mod, d_cnt, c->stream);
  MOT_HIP(c, hipGetLastError());
  int h[2];
  MOT_TRY(read_counts(c, d_cnt, 2, h));
  const int np = h[1];
  if (h[0] < 0 || h[0] > T || np < 0) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  *n_models = T; *n_points = np;
  if (models && T > max_models) return fail(c, MOT_E_CAPACITY, "more models (max_tracks_total) than the caller's buffer holds");
  if (points && np > point_capacity) return fail(c, MOT_E_CAPACITY, "more records than the caller's point buffer holds");
  const bool want_points = points && np > 0;
  if (want_points) MOT_TRY(grow_stage(c, &c->d_tm_points, &c->tm_points_cap, (size_t)np, sizeof(mot_accum_point)));
  mot_launch_track_models_transform(a, slot, 1, flags, want_points ? c->d_tm_points : nullptr, want_points ? (long)np : 0, d_mod, c->stream);   // (the extents, with or without records)
  MOT_HIP(c, hipGetLastError());
  if (models) MOT_HIP(c, hipMemcpyAsync(models, d_mod, (size_t)T * sizeof(mot_track_model), hipMemcpyDeviceToHost, c->stream));
  if (want_points) MOT_HIP(c, hipMemcpyAsync(points, c->d_tm_points, (size_t)np * sizeof(mot_accum_point), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- voxel-thinned object models (track_voxels.hip)
// The raw models' checks and latest-step block, and a scratch of the feature's own — the plan's headers and the per-model results, 96 bytes per row — taken at
// the first call and released with the raw models' blocks (track_models_release). Everything is validated before anything is launched or allocated.
static int check_track_voxels(mot_ctx* c, const char* who, int flags, const mot_voxel_params* p, TrackVoxelArgs* v) {
  MOT_TRY(check_track_models(c, who, flags));
  if (!p) return fail(c, MOT_E_ARG, who, ": null params");
  const float leaf[3] = {p->leaf_x, p->leaf_y, p->leaf_z};
  for (float l : leaf)
    if (!(l >= 1e-3f && l <= 1e3f)) return fail(c, MOT_E_ARG, who, ": a leaf must be finite and in [1e-3, 1e3]");   // (NaN fails both comparisons)
  if (p->min_points < 1 || p->min_points > MOT_MODEL_VOXEL_MAX_K) return fail(c, MOT_E_ARG, who, ": min_points must be in [1, MOT_MODEL_VOXEL_MAX_K]");
  v->inv_x = 1.0f / leaf[0]; v->inv_y = 1.0f / leaf[1]; v->inv_z = 1.0f / leaf[2]; v->min_points = p->min_points;
  return MOT_OK;
}
static int check_track_voxels_on(mot_ctx* c, const char* who) {
  MOT_TRY(check_track_models_on(c, who));
  if (c->accum_K > MOT_MODEL_VOXEL_MAX_K)
    return fail(c, MOT_E_STATE, who, ": points_per_track exceeds MOT_MODEL_VOXEL_MAX_K = 4096, the longest model the voxel calls sort (mot_export_track_models_dev serves it)");
  return MOT_OK;
}
struct TrackVoxelScratch { mot_track_model* plan; TrackVoxelResult* res; int* plan_counts; };
static int ensure_track_voxels(mot_ctx* c, bool host_stage, TrackVoxelScratch* s) {
  MOT_TRY(ensure_track_models(c, false));
  const size_t rows_n = (size_t)c->batch * c->max_tracks_total;
  MOT_TRY(dev_alloc(c, &c->d_tv_scratch, rows_n * (sizeof(mot_track_model) + sizeof(TrackVoxelResult)) + (size_t)c->batch * 2 * sizeof(int)));
  if (host_stage) MOT_TRY(dev_alloc(c, &c->d_tv_stage, (size_t)c->max_tracks_total * sizeof(mot_track_voxel_model) + 16));
  s->plan = reinterpret_cast<mot_track_model*>(c->d_tv_scratch);
  s->res = reinterpret_cast<TrackVoxelResult*>(s->plan + rows_n);
  s->plan_counts = reinterpret_cast<int*>(s->res + rows_n);
  return MOT_OK;
}

extern "C" int mot_export_track_model_voxels_dev(mot_ctx* c, int batch, int flags, const mot_voxel_params* params, mot_model_voxel* d_voxels, long voxel_stride,
                                                 mot_track_voxel_model* d_models, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_export_track_model_voxels_dev";
  TrackVoxelArgs v;
  MOT_TRY(check_track_voxels(c, who, flags, params, &v));
  if (!d_models || !d_counts || batch < 1 || batch > c->batch || voxel_stride < 0 || (!d_voxels && voxel_stride > 0) || ((size_t)d_voxels & 15) ||
      (((size_t)d_models | (size_t)d_counts) & 3))
    return fail(c, MOT_E_ARG, who, ": bad argument");
  MOT_TRY(check_track_voxels_on(c, who));
  TrackVoxelScratch s;
  MOT_TRY(ensure_track_voxels(c, false, &s));
  TrackModelBuffers a;
  MOT_TRY(track_model_buffers(c, flags, &a));
  mot_launch_track_models_plan(a, 0, batch, flags, s.plan, s.plan_counts, c->stream);
  mot_launch_track_voxels_count(a, 0, batch, flags, v, s.plan, s.res, d_models, reinterpret_cast<int*>(d_counts), c->stream);
  if (d_voxels && voxel_stride > 0) mot_launch_track_voxels_write(a, 0, batch, flags, v, s.plan, d_voxels, voxel_stride, d_models, c->stream);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

extern "C" int mot_get_track_model_voxels(mot_ctx* c, int slot, int flags, const mot_voxel_params* params, mot_track_voxel_model* models, int max_models, int* n_models,
                                          mot_model_voxel* voxels, int voxel_capacity, int* n_voxels) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const char* who = "mot_get_track_model_voxels";
  TrackVoxelArgs v;
  MOT_TRY(check_track_voxels(c, who, flags, params, &v));
  if (slot < 0 || slot >= c->batch || max_models < 0 || voxel_capacity < 0 || !n_models || !n_voxels) return fail(c, MOT_E_ARG, who, ": slot or a capacity out of range, or a null count");
  MOT_TRY(check_track_voxels_on(c, who));
  TrackVoxelScratch s;
  MOT_TRY(ensure_track_voxels(c, true, &s));
  const int T = c->max_tracks_total;
  TrackModelBuffers a;
  MOT_TRY(track_model_buffers(c, flags, &a));
  // the slot's headers and counts into the staging block; the counts decide what fits the caller's buffers before a voxel moves
  mot_track_voxel_model* d_mod = reinterpret_cast<mot_track_voxel_model*>(c->d_tv_stage);
  int* d_cnt = reinterpret_cast<int*>(d_mod + T);
  mot_launch_track_models_plan(a, slot, 1, flags, s.plan, s.plan_counts, c->stream);
  mot_launch_track_voxels_count(a, slot, 1, flags, v, s.plan, s.res, d_mod, d_cnt, c->stream);
  MOT_HIP(c, hipGetLastError());
  int h[2];
  MOT_TRY(read_counts(c, d_cnt, 2, h));
  const int nv = h[1];
  if (h[0] < 0 || h[0] > T || nv < 0) return fail(c, MOT_E_STATE, who, ": inconsistent counts");
  *n_models = T; *n_voxels = nv;
  if (models && T > max_models) return fail(c, MOT_E_CAPACITY, "more models (max_tracks_total) than the caller's buffer holds");
  if (voxels && nv > voxel_capacity) return fail(c, MOT_E_CAPACITY, "more voxels than the caller's voxel buffer holds");
  const bool want_voxels = voxels && nv > 0;
  if (want_voxels) MOT_TRY(grow_stage(c, &c->d_tv_voxels, &c->tv_voxels_cap, (size_t)nv, sizeof(mot_model_voxel)));
  if (want_voxels) {
    mot_launch_track_voxels_write(a, slot, 1, flags, v, s.plan, c->d_tv_voxels, (long)nv, d_mod, c->stream);
    MOT_HIP(c, hipGetLastError());
  }
  if (models) MOT_HIP(c, hipMemcpyAsync(models, d_mod, (size_t)T * sizeof(mot_track_voxel_model), hipMemcpyDeviceToHost, c->stream));
  if (want_voxels) MOT_HIP(c, hipMemcpyAsync(voxels, c->d_tv_voxels, (size_t)nv * sizeof(mot_model_voxel), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

// the track counters of one stream back to zero (stream-ordered: after the steps already queued, before the next one)
static int clear_tracks(mot_ctx* c, int slot) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch) return fail(c, MOT_E_ARG, "slot out of range");
  MOT_HIP(c, hipMemsetAsync(c->d_nt + slot, 0, sizeof(int), c->stream));
  MOT_HIP(c, hipMemsetAsync(c->d_nlive + slot, 0, sizeof(int), c->stream));
  MOT_HIP(c, hipMemsetAsync(c->d_tflags + slot, 0, sizeof(int), c->stream));
  MOT_TRY(accum_restart_slots(c, slot, 1));
  return scene_restart_slots(c, slot, 1);
}
// forget the TRACKS of one stream, keep its ego dead reckoning (the origin of its global frame)
extern "C" int mot_reset_tracks_slot(mot_ctx* c, int slot) {
  MOT_TRY(clear_tracks(c, slot));
  c->ego[slot].tracks_restart = true;   // the next step is a "first frame" for the tracker only: prepare_track_args
  c->ego[slot].nt = 0;
  return MOT_OK;
}
// forget the tracker state of ONE stream (mot_reset does it for all of them)
extern "C" int mot_reset_slot(mot_ctx* c, int slot) {
  MOT_TRY(clear_tracks(c, slot));
  c->ego[slot] = mot_ctx::SlotEgo();
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- stream snapshots
// The tracker state of ONE stream as a relocatable block of host memory: save it, load it into any slot of any context with the same
// track-slot count (another GPU, another process, after a restart) and the stream continues bit for bit. The reference keeps this state
// in file-scope globals (imm_ukf_jpda.cpp:19-24,56-70) and can neither save nor reset it (checkpoint / resume).
// Layout: SnapshotHeader, then the arrays in the order written below; the per-ever-track arrays carry nt entries, not E.
// The FORMAT has a version of its own (MOT_SNAPSHOT_FORMAT, include/mot.h), decoupled from the ABI version since ABI v6: a library whose entry points
// grow keeps loading the snapshots it wrote before. Format 5 = what ABI v5 wrote (its `abi` field held 5). Snapshots of ABI v4 and older (no
// step_ego_yaw, 16-byte tombs) are refused: INTEGRATION.md says so.
struct SnapshotHeader {
  uint32_t magic, abi, header_bytes, track_bytes, record_bytes;   // 'MOTS', MOT_SNAPSHOT_FORMAT, sizeof(SnapshotHeader), sizeof(DevTrack), sizeof(mot_track)
  int32_t T, nt, nlive, nzomb, flags;
  uint8_t init, ego_called, tracks_restart, pad[5];
  double timestamp, egoVelo, egoYaw, egoPreYaw, rx, ry, ryaw, egoPoint[3], step_ego_yaw;
  uint64_t total_bytes;
};
static size_t snapshot_bytes(size_t T, size_t nt) {
  const size_t usedW = (T + 63) / 64;
  return sizeof(SnapshotHeader) + T * sizeof(DevTrack) + T * sizeof(int) /*live*/ + T * sizeof(int) /*zomb*/ + usedW * sizeof(unsigned long long) +
         T * sizeof(mot_track) + nt * (sizeof(Vec2d) + sizeof(int) + sizeof(TrackTomb));
}

extern "C" int mot_stream_snapshot_size(mot_ctx* c, size_t* bytes) {
  if (!c) return MOT_E_ARG;
  if (!bytes) return fail(c, MOT_E_ARG, "mot_stream_snapshot_size: null bytes");
  *bytes = snapshot_bytes((size_t)c->max_tracks_total, (size_t)c->max_tracks_ever);
  return MOT_OK;
}

extern "C" int mot_stream_save(mot_ctx* c, int slot, void* blob, size_t capacity, size_t* written) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || !blob || !written) return fail(c, MOT_E_ARG, "mot_stream_save: slot out of range, null blob or null written");
  const size_t T = c->max_tracks_total, E = c->max_tracks_ever, usedW = (T + 63) / 64;
  int meta[4] = {0, 0, 0, 0};
  MOT_HIP(c, hipMemcpyAsync(&meta[0], c->d_nt + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[1], c->d_nlive + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[2], c->d_nzomb + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[3], c->d_tflags + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  const mot_ctx::SlotEgo& e = c->ego[slot];
  const bool seeded = e.init && !e.tracks_restart;   // before the first tracker step (or after a restart) the device arrays of the slot mean nothing
  const size_t nt = seeded ? (size_t)meta[0] : 0;
  if (nt > E) return fail(c, MOT_E_STATE, "mot_stream_save: the slot's track count exceeds the context's capacity");
  const size_t total = snapshot_bytes(T, nt);
  *written = total;
  if (total > capacity) return fail(c, MOT_E_CAPACITY, "mot_stream_save: the blob is smaller than the snapshot (mot_stream_snapshot_size gives the upper bound)");
  SnapshotHeader h;
  memset(&h, 0, sizeof h);
  h.magic = 0x53544f4du; h.abi = MOT_SNAPSHOT_FORMAT; h.header_bytes = sizeof(SnapshotHeader); h.track_bytes = sizeof(DevTrack); h.record_bytes = sizeof(mot_track);
  h.T = (int32_t)T; h.nt = (int32_t)nt; h.nlive = seeded ? meta[1] : 0; h.nzomb = seeded ? meta[2] : 0; h.flags = seeded ? meta[3] : 0;
  h.init = e.init; h.ego_called = e.ego_called; h.tracks_restart = e.tracks_restart;
  h.timestamp = e.timestamp; h.egoVelo = e.egoVelo; h.egoYaw = e.egoYaw; h.egoPreYaw = e.egoPreYaw; h.rx = e.rx; h.ry = e.ry; h.ryaw = e.ryaw;
  for (int k = 0; k < 3; k++) h.egoPoint[k] = e.egoPoint[k];
  h.step_ego_yaw = e.step_ego_yaw;
  h.total_bytes = total;
  char* o = static_cast<char*>(blob);
  memcpy(o, &h, sizeof h); o += sizeof h;
  auto take = [&](const void* d, size_t bytes) -> hipError_t {
    hipError_t rc = bytes ? hipMemcpyAsync(o, d, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    o += bytes;
    return rc;
  };
  MOT_HIP(c, take(c->d_tracks + (size_t)slot * T, T * sizeof(DevTrack)));
  MOT_HIP(c, take(c->d_live + (size_t)slot * 2 * T, T * sizeof(int)));
  MOT_HIP(c, take(c->d_zomb + (size_t)slot * T, T * sizeof(int)));
  MOT_HIP(c, take(c->d_used + (size_t)slot * usedW, usedW * sizeof(unsigned long long)));
  MOT_HIP(c, take(c->d_tout + (size_t)slot * T, T * sizeof(mot_track)));
  MOT_HIP(c, take(c->d_pos + (size_t)slot * E, nt * sizeof(Vec2d)));
  MOT_HIP(c, take(c->d_slot_of + (size_t)slot * E, nt * sizeof(int)));
  MOT_HIP(c, take(c->d_tomb + (size_t)slot * E, nt * sizeof(TrackTomb)));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  return MOT_OK;
}

extern "C" int mot_stream_load(mot_ctx* c, int slot, const void* blob, size_t bytes) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || !blob) return fail(c, MOT_E_ARG, "mot_stream_load: slot out of range or null blob");
  const size_t T = c->max_tracks_total, E = c->max_tracks_ever, usedW = (T + 63) / 64;
  SnapshotHeader h;
  if (bytes < sizeof h) return fail(c, MOT_E_ARG, "mot_stream_load: not a snapshot (shorter than its header)");
  memcpy(&h, blob, sizeof h);
  // everything is checked before the slot is touched
  if (h.magic != 0x53544f4du || h.header_bytes != sizeof(SnapshotHeader)) return fail(c, MOT_E_ARG, "mot_stream_load: not a snapshot of this library");
  if (h.abi != MOT_SNAPSHOT_FORMAT || h.track_bytes != sizeof(DevTrack) || h.record_bytes != sizeof(mot_track))
    return fail(c, MOT_E_ARG, "mot_stream_load: the snapshot was written by another version of the library");
  if ((size_t)h.T != T) return fail(c, MOT_E_ARG, "mot_stream_load: the snapshot's track-slot count differs from this context's max_tracks_total");
  if (h.nt < 0 || h.nlive < 0 || h.nzomb < 0 || (size_t)h.nlive > T || (size_t)h.nzomb > T) return fail(c, MOT_E_ARG, "mot_stream_load: corrupt counters");
  if ((size_t)h.nt > E) return fail(c, MOT_E_CAPACITY, "mot_stream_load: the stream has created more tracks than this context's max_tracks_ever");
  const size_t nt = (size_t)h.nt;
  if (h.total_bytes != snapshot_bytes(T, nt) || bytes < h.total_bytes) return fail(c, MOT_E_ARG, "mot_stream_load: truncated snapshot");
  {  // the index arrays the kernels follow without looking: a damaged file must not send them out of bounds
    const char* b0 = static_cast<const char*>(blob) + sizeof h;
    const char* p_tracks = b0;
    const int* p_live = reinterpret_cast<const int*>(b0 + T * sizeof(DevTrack));
    const int* p_zomb = p_live + T;
    const char* p_after = reinterpret_cast<const char*>(p_zomb + T) + usedW * sizeof(unsigned long long) + T * sizeof(mot_track) + nt * sizeof(Vec2d);
    const int* p_slot_of = reinterpret_cast<const int*>(p_after);
    auto ref_of = [&](int sl) { int r; memcpy(&r, p_tracks + (size_t)sl * sizeof(DevTrack) + offsetof(DevTrack, ref_id), sizeof r); return r; };
    bool ok = true;
    for (int i = 0; i < h.nlive && ok; i++) { int sl; memcpy(&sl, p_live + i, sizeof sl); ok = sl >= 0 && (size_t)sl < T && ref_of(sl) >= 0 && ref_of(sl) < h.nt; }
    for (int i = 0; i < h.nzomb && ok; i++) { int sl; memcpy(&sl, p_zomb + i, sizeof sl); ok = sl >= 0 && (size_t)sl < T && ref_of(sl) >= 0 && ref_of(sl) < h.nt; }
    for (size_t i = 0; i < nt && ok; i++) { int sl; memcpy(&sl, p_slot_of + i, sizeof sl); ok = sl >= -1 && (sl < 0 || (size_t)sl < T); }
    if (!ok) return fail(c, MOT_E_ARG, "mot_stream_load: corrupt snapshot (a track slot or reference index out of range)");
    // ... and the slot bookkeeping must be CONSISTENT, not only in range: the finish kernel lists the free slots from the `used` bitmap
    // and appends newborns to the live list, so a bitmap that misses a listed slot (or a slot listed twice) would let nlive + births
    // exceed T and the next step write past the slot's live / zombie arrays — into another stream's state. Required: every listed
    // slot is listed once and has its bit set, no other bit is set (none at or beyond T), nlive + nzomb <= T, and the per-track-ever
    // table points back at each listed slot.
    const char* p_used = reinterpret_cast<const char*>(p_zomb + T);
    auto used_bit = [&](size_t sl) { unsigned long long w; memcpy(&w, p_used + (sl >> 6) * sizeof w, sizeof w); return (w >> (sl & 63)) & 1ull; };
    std::vector<unsigned char> seen(T, 0);
    size_t listed = 0;
    auto visit = [&](const int* list, int n) {
      for (int i = 0; i < n && ok; i++) {
        int sl; memcpy(&sl, list + i, sizeof sl);
        int back; memcpy(&back, p_slot_of + ref_of(sl), sizeof back);
        ok = !seen[sl] && used_bit((size_t)sl) && back == sl;
        seen[sl] = 1; listed++;
      }
    };
    visit(p_live, h.nlive); visit(p_zomb, h.nzomb);
    size_t bits = 0;
    const bool seeded = h.init && !h.tracks_restart;   // otherwise the arrays mean nothing (mot_stream_save wrote the counters as zero): the next step seeds them anew
    if (!seeded) { if (h.nt || h.nlive || h.nzomb) ok = false; bits = listed; }
    for (size_t w = 0; seeded && w < usedW && ok; w++) {
      unsigned long long v; memcpy(&v, p_used + w * sizeof v, sizeof v);
      if (w == usedW - 1 && (T & 63)) ok = (v >> (T & 63)) == 0;
      bits += (size_t)__builtin_popcountll(v);
    }
    if (!ok || listed > T || bits != listed)
      return fail(c, MOT_E_ARG, "mot_stream_load: corrupt snapshot (the live / just-died lists, the slot bitmap and the per-track table disagree)");
  }
  const char* in = static_cast<const char*>(blob) + sizeof h;
  auto give = [&](void* d, size_t n) -> hipError_t {
    hipError_t rc = n ? hipMemcpyAsync(d, in, n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    in += n;
    return rc;
  };
  MOT_HIP(c, give(c->d_tracks + (size_t)slot * T, T * sizeof(DevTrack)));
  MOT_HIP(c, give(c->d_live + (size_t)slot * 2 * T, T * sizeof(int)));
  MOT_HIP(c, give(c->d_zomb + (size_t)slot * T, T * sizeof(int)));
  MOT_HIP(c, give(c->d_used + (size_t)slot * usedW, usedW * sizeof(unsigned long long)));
  MOT_HIP(c, give(c->d_tout + (size_t)slot * T, T * sizeof(mot_track)));
  MOT_HIP(c, give(c->d_pos + (size_t)slot * E, nt * sizeof(Vec2d)));
  MOT_HIP(c, give(c->d_slot_of + (size_t)slot * E, nt * sizeof(int)));
  MOT_HIP(c, give(c->d_tomb + (size_t)slot * E, nt * sizeof(TrackTomb)));
  const int meta[4] = {h.nt, h.nlive, h.nzomb, h.flags};
  MOT_HIP(c, hipMemcpyAsync(c->d_nt + slot, &meta[0], sizeof(int), hipMemcpyHostToDevice, c->stream));
  MOT_HIP(c, hipMemcpyAsync(c->d_nlive + slot, &meta[1], sizeof(int), hipMemcpyHostToDevice, c->stream));
  MOT_HIP(c, hipMemcpyAsync(c->d_nzomb + slot, &meta[2], sizeof(int), hipMemcpyHostToDevice, c->stream));
  MOT_HIP(c, hipMemcpyAsync(c->d_tflags + slot, &meta[3], sizeof(int), hipMemcpyHostToDevice, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));   // the caller's blob and `meta` may go away
  mot_ctx::SlotEgo e;
  e.init = h.init != 0; e.ego_called = h.ego_called != 0; e.tracks_restart = h.tracks_restart != 0;
  e.timestamp = h.timestamp; e.egoVelo = h.egoVelo; e.egoYaw = h.egoYaw; e.egoPreYaw = h.egoPreYaw; e.rx = h.rx; e.ry = h.ry; e.ryaw = h.ryaw;
  for (int k = 0; k < 3; k++) e.egoPoint[k] = h.egoPoint[k];
  e.step_ego_yaw = h.step_ego_yaw;
  e.nt = h.nt;
  c->ego[slot] = e;
  MOT_TRY(accum_restart_slots(c, slot, 1));   // (the accumulators are not stream state: the loaded stream's ids start with empty rows)
  return scene_restart_slots(c, slot, 1);     // (nor is the scene grid)
}

// immUkfJpdaf(), OT/tracking/imm_ukf_jpda.cpp:704
extern "C" int mot_track_step(mot_ctx* c, int slot, const float* boxes_global, int m, double timestamp, mot_track* tracks,
                              int max_tracks, int* n_tracks) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || m < 0 || (!boxes_global && m > 0) || !n_tracks) return fail(c, MOT_E_ARG, "mot_track_step: slot out of range, negative m, null boxes or null n_tracks");
  static_assert(kMaxBoxesPerFrame == MOT_MAX_BOXES_PER_FRAME, "mot.h documents the limit");
  *n_tracks = -1;   // until the step has run (callers tell "refused" from "births dropped" by it: include/mot.h)
  if (m > kMaxBoxesPerFrame) return fail(c, MOT_E_CAPACITY, "more boxes in a frame than the library supports (1024): the step was not taken");
  if (!c->ego[slot].ego_called) return fail(c, MOT_E_STATE, "mot_ego_update must precede mot_track_step (getOriginPoints precedes immUkfJpdaf, OT/tracking/main.cpp:74,166)");
  {
    char* blk;
    MOT_TRY(arg_block_acquire(c, &blk));
    TrackFrameArgs* targs = reinterpret_cast<TrackFrameArgs*>(blk + c->arg_off_targs);
    for (int b = 0; b < c->batch; b++) targs[b].run = 0;
    prepare_track_args(c, targs, slot, m, timestamp, true);
    MOT_TRY(arg_block_commit(c, c->arg_off_targs, c->batch * sizeof(TrackFrameArgs)));
  }
  if (m > 0) MOT_HIP(c, hipMemcpyAsync(c->d_tboxes + (size_t)slot * kMaxBoxesPerFrame * 24, boxes_global, (size_t)m * 24 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  mot_launch_track(track_buffers(c, false), c->batch, c->stream);
  if (c->track_links) c->res.tracker_fed(slot);
  MOT_HIP(c, hipGetLastError());
  return mot_get_tracks(c, slot, tracks, max_tracks, n_tracks);
}

// immUkfJpdaf for one frame of EVERY slot 0..batch-1 with the boxes already on the device (global frame): d_boxes_global holds
// box_stride_floats floats per slot (>= 24 * m[b]), m[] (host) the number of boxes per slot. Callers with their own detector,
// and the tracker's load measurements, enter here; mot_ego_update(slot) must have been called for the frame as usual.
extern "C" int mot_track_steps_dev(mot_ctx* c, const float* d_boxes_global, long box_stride_floats, const int* m, int batch, const double* timestamps) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (!d_boxes_global || !m || !timestamps || batch < 1 || batch > c->batch || box_stride_floats < 0) return fail(c, MOT_E_ARG, "mot_track_steps_dev: bad argument");
  for (int b = 0; b < batch; b++) {
    if (m[b] < 0 || (long)m[b] * 24 > box_stride_floats) return fail(c, MOT_E_ARG, "mot_track_steps_dev: m[b] boxes do not fit box_stride_floats");
    if (m[b] > kMaxBoxesPerFrame) return fail(c, MOT_E_CAPACITY, "more boxes in a frame than the library supports (1024)");
    if (!c->ego[b].ego_called) return fail(c, MOT_E_STATE, "mot_ego_update must precede the tracker step of a slot");
  }
  {
    char* blk;
    MOT_TRY(arg_block_acquire(c, &blk));
    TrackFrameArgs* targs = reinterpret_cast<TrackFrameArgs*>(blk + c->arg_off_targs);
    for (int b = 0; b < c->batch; b++) targs[b].run = 0;
    for (int b = 0; b < batch; b++) prepare_track_args(c, targs, b, m[b], timestamps[b], true);
    MOT_TRY(arg_block_commit(c, c->arg_off_targs, c->batch * sizeof(TrackFrameArgs)));
  }
  TrackBuffers t = track_buffers(c, false);
  t.boxes = d_boxes_global; t.box_stride = box_stride_floats;
  { ProfScope ps(c, kT1); mot_launch_track(t, batch, c->stream); }
  if (c->track_links) for (int b = 0; b < batch; b++) c->res.tracker_fed(b);
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- live tracks in the sensor frame
// both matrices of the pose the slot's dead reckoning holds now (mot_ego_update or a fused step last wrote it; (0, 0, 0) before the first). Host only.
extern "C" int mot_sensor_pose(mot_ctx* c, int slot, float* sensor_from_global, float* global_from_sensor) {
  if (!c) return MOT_E_ARG;
  if (slot < 0 || slot >= c->batch) return fail(c, MOT_E_ARG, "slot out of range");
  const double* p = c->ego[slot].egoPoint;
  if (sensor_from_global) tf_global_to_velodyne(p[0], p[1], p[2], sensor_from_global);
  if (global_from_sensor) tf_velodyne_to_global(p[0], p[1], p[2], global_from_sensor);
  return MOT_OK;
}

// The global -> sensor matrices of slots first .. first + n - 1 onto the device, ahead of the export kernel that reads them: one stream-ordered copy from the next block of the
// page-locked ring (PinnedRing, mot_host.h).
static int ensure_sensor_tf(mot_ctx* c) {   // at the first sensor-frame call; a failure half-way leaves what exists for mot_destroy and the next call
  MOT_TRY(dev_alloc(c, &c->d_sensor_tf, (size_t)c->batch * sizeof(EgoTf)));
  return c->sensor_tf_ring.create(c, (size_t)c->batch * sizeof(EgoTf));
}
static int send_sensor_tf(mot_ctx* c, int first, int n, const EgoTf** d_tf) {
  MOT_TRY(ensure_sensor_tf(c));
  char* raw;
  MOT_TRY(c->sensor_tf_ring.acquire(c, &raw));
  EgoTf* blk = reinterpret_cast<EgoTf*>(raw);
  for (int k = 0; k < n; k++) { const double* p = c->ego[first + k].egoPoint; tf_global_to_velodyne(p[0], p[1], p[2], blk[k].m); }
  MOT_TRY(c->sensor_tf_ring.commit(c, c->d_sensor_tf, 0, (size_t)n * sizeof(EgoTf), c->stream));
  *d_tf = c->d_sensor_tf;
  return MOT_OK;
}

// ---------------------------------------------------------------------------------------- exports: live tracks of slots 0..batch-1, global or sensor frame
// One implementation per pair of entry points; `who` is the name the caller's messages carry (a _frame call with MOT_FRAME_GLOBAL IS the global call, name included).
static int check_export(mot_ctx* c, const char* who, int frame, bool args_ok) {
  if (frame != MOT_FRAME_GLOBAL && frame != MOT_FRAME_SENSOR) return fail(c, MOT_E_ARG, who, ": frame must be MOT_FRAME_GLOBAL or MOT_FRAME_SENSOR");
  return args_ok ? MOT_OK : fail(c, MOT_E_ARG, who, ": bad argument");
}
// fixed-stride records: out[b * max_per_slot + i], counts[b]
static int launch_export(mot_ctx* c, int frame, int batch, mot_track* out, int max_per_slot, int* counts) {
  if (frame == MOT_FRAME_SENSOR) {
    const EgoTf* tf;
    MOT_TRY(send_sensor_tf(c, 0, batch, &tf));
    mot_launch_export_tracks_sensor(track_buffers(c, false), 0, batch, tf, out, max_per_slot, counts, c->stream);
  } else {
    mot_launch_export_tracks(track_buffers(c, false), batch, out, max_per_slot, counts, c->stream);
  }
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}
static int export_tracks(mot_ctx* c, const char* who, int batch, int frame, void* d_tracks, int max_per_slot, int32_t* d_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_export(c, who, frame, d_tracks && d_counts && batch >= 1 && batch <= c->batch && max_per_slot >= 1));
  return launch_export(c, frame, batch, (mot_track*)d_tracks, max_per_slot, (int*)d_counts);
}
static int export_tracks_packed(mot_ctx* c, const char* who, int batch, int frame, void* d_block, long block_bytes) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  const long head = mot_packed_head_bytes(batch);
  MOT_TRY(check_export(c, who, frame, d_block && batch >= 1 && batch <= c->batch && !((size_t)d_block & 15) && block_bytes >= head));
  const long fit = (block_bytes - head) / (long)sizeof(mot_track);
  const int cap = (int)(fit > 0x7fffffff ? 0x7fffffff : fit);
  mot_track* rec = (mot_track*)((char*)d_block + head);
  if (frame == MOT_FRAME_SENSOR) {
    const EgoTf* tf;
    MOT_TRY(send_sensor_tf(c, 0, batch, &tf));
    mot_launch_export_tracks_packed_sensor(track_buffers(c, false), batch, tf, (int*)d_block, rec, cap, c->stream);
  } else {
    mot_launch_export_tracks_packed(track_buffers(c, false), batch, (int*)d_block, rec, cap, c->stream);
  }
  MOT_HIP(c, hipGetLastError());
  return MOT_OK;
}
// live tracks of every slot -> the caller's HOST block, asynchronously on the context stream (read after mot_synchronize), through the context's device block: grown (never
// shrunk) to the largest max_per_slot asked for
static int fetch_tracks(mot_ctx* c, const char* who, int batch, int frame, void* h_tracks, int max_per_slot, int32_t* h_counts) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  MOT_TRY(check_export(c, who, frame, h_tracks && h_counts && batch >= 1 && batch <= c->batch && max_per_slot >= 1));
  if (c->fetch_cap < max_per_slot) {
    if (c->d_fetch) { MOT_HIP(c, hipStreamSynchronize(c->stream)); MOT_TRY(release(c, &c->d_fetch)); }
    MOT_TRY(dev_alloc(c, &c->d_fetch, (size_t)c->batch * max_per_slot * sizeof(mot_track)));
    MOT_TRY(dev_alloc(c, &c->d_fetch_counts, (size_t)c->batch * sizeof(int)));
    c->fetch_cap = max_per_slot;
  }
  MOT_TRY(launch_export(c, frame, batch, c->d_fetch, max_per_slot, c->d_fetch_counts));
  MOT_HIP(c, hipMemcpyAsync(h_tracks, c->d_fetch, (size_t)batch * max_per_slot * sizeof(mot_track), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(h_counts, c->d_fetch_counts, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  return MOT_OK;
}
extern "C" int mot_export_tracks_dev(mot_ctx* c, int batch, void* d_tracks, int max_per_slot, int32_t* d_counts) { return export_tracks(c, "mot_export_tracks_dev", batch, MOT_FRAME_GLOBAL, d_tracks, max_per_slot, d_counts); }
extern "C" int mot_export_tracks_frame_dev(mot_ctx* c, int batch, int frame, void* d_tracks, int max_per_slot, int32_t* d_counts) {
  return export_tracks(c, frame == MOT_FRAME_GLOBAL ? "mot_export_tracks_dev" : "mot_export_tracks_frame_dev", batch, frame, d_tracks, max_per_slot, d_counts);
}
extern "C" int mot_export_tracks_packed_dev(mot_ctx* c, int batch, void* d_block, long block_bytes) { return export_tracks_packed(c, "mot_export_tracks_packed_dev", batch, MOT_FRAME_GLOBAL, d_block, block_bytes); }
extern "C" int mot_export_tracks_packed_frame_dev(mot_ctx* c, int batch, int frame, void* d_block, long block_bytes) {
  return export_tracks_packed(c, frame == MOT_FRAME_GLOBAL ? "mot_export_tracks_packed_dev" : "mot_export_tracks_packed_frame_dev", batch, frame, d_block, block_bytes);
}
extern "C" int mot_fetch_tracks_async(mot_ctx* c, int batch, void* h_tracks, int max_per_slot, int32_t* h_counts) { return fetch_tracks(c, "mot_fetch_tracks_async", batch, MOT_FRAME_GLOBAL, h_tracks, max_per_slot, h_counts); }
extern "C" int mot_fetch_tracks_frame_async(mot_ctx* c, int batch, int frame, void* h_tracks, int max_per_slot, int32_t* h_counts) {
  return fetch_tracks(c, frame == MOT_FRAME_GLOBAL ? "mot_fetch_tracks_async" : "mot_fetch_tracks_frame_async", batch, frame, h_tracks, max_per_slot, h_counts);
}

// The tracking node's callback (OT/tracking/main.cpp:65-196) in one call: getOriginPoints on the host, then on the device the frame's boxes sensor -> global in the
// tracker's prologue (mot_track_prep.h, the code the fused sequence runs, fed from a staging buffer of this call's own instead of the box stage's d_boxes),
// immUkfJpdaf, and the live tracks back in the sensor frame (export_tracks_sensor_kernel on this one stream). One upload, one synchronisation, one batch of copies back.
extern "C" int mot_tracking_node_frame(mot_ctx* c, int slot, const float* boxes_sensor, int m, double timestamp, double v_gps, double yaw_gps, mot_tracking_frame* out) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || m < 0 || (!boxes_sensor && m > 0) || !out) return fail(c, MOT_E_ARG, "mot_tracking_node_frame: slot out of range, negative m, null boxes or null result");
  if (m > kMaxBoxesPerFrame) return fail(c, MOT_E_ARG, "mot_tracking_node_frame: more boxes in a frame than the library supports (1024): nothing was run");
  memset(out, 0, sizeof *out);
  const size_t T = c->max_tracks_total, o_meta = T * sizeof(mot_track);
  char* pin;
  MOT_TRY(pinned_scratch(c, o_meta + 16, &pin));
  MOT_TRY(dev_alloc(c, &c->d_node_boxes, (size_t)kMaxBoxesPerFrame * 24 * sizeof(float)));
  MOT_TRY(dev_alloc(c, &c->d_node_out, o_meta + 16));
  MOT_TRY(ensure_sensor_tf(c));   // (everything the call allocates, before it changes the stream's state: a call refused here can be repeated)
  MOT_TRY(mot_ego_update(c, slot, timestamp, v_gps, yaw_gps, out->origin6));
  {
    char* blk;
    MOT_TRY(arg_block_acquire(c, &blk));
    TrackFrameArgs* targs = reinterpret_cast<TrackFrameArgs*>(blk + c->arg_off_targs);
    EgoTf* ego = reinterpret_cast<EgoTf*>(blk + c->arg_off_ego);
    for (int b = 0; b < c->batch; b++) targs[b].run = 0;
    prepare_track_args(c, targs, slot, m, timestamp, true);
    tf_velodyne_to_global(c->ego[slot].egoPoint[0], c->ego[slot].egoPoint[1], c->ego[slot].egoPoint[2], ego[slot].m);
    MOT_TRY(arg_block_commit(c, c->arg_off_targs, c->arg_off_launch - c->arg_off_targs));   // the tracker arguments and the matrices lie back to back
  }
  if (m > 0) MOT_HIP(c, hipMemcpyAsync(c->d_node_boxes, boxes_sensor, (size_t)m * 24 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  TrackBuffers t = track_buffers(c, false);
  // the prologue addresses stream b's sensor-frame boxes at boxes_sensor + b * 1024 * 24 and only the stream that runs reads them: the base is placed so that
  // `slot` finds the staging buffer (an address computation, nothing is read before it)
  t.boxes_sensor = reinterpret_cast<const float*>(reinterpret_cast<uintptr_t>(c->d_node_boxes) - (uintptr_t)slot * kMaxBoxesPerFrame * 24 * sizeof(float));
  t.ego = c->d_ego; t.boxes_out = c->d_tboxes;
  mot_launch_track(t, c->batch, c->stream);
  if (c->track_links) c->res.tracker_fed(slot);
  const EgoTf* tf;
  MOT_TRY(send_sensor_tf(c, slot, 1, &tf));
  int* d_meta = reinterpret_cast<int*>(c->d_node_out + o_meta);
  mot_launch_export_tracks_sensor(t, slot, 1, tf, reinterpret_cast<mot_track*>(c->d_node_out), (int)T, d_meta, c->stream);
  MOT_HIP(c, hipGetLastError());
  int* meta = reinterpret_cast<int*>(pin + o_meta);
  MOT_HIP(c, hipMemcpyAsync(pin, c->d_node_out, o_meta + sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[1], c->d_nt + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipMemcpyAsync(&meta[2], c->d_tflags + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (meta[0] < 0 || (size_t)meta[0] > T) return fail(c, MOT_E_STATE, "mot_tracking_node_frame: inconsistent counts");
  c->ego[slot].nt = meta[1];
  out->n_live = meta[0]; out->n_ever = meta[1]; out->tracks = reinterpret_cast<const mot_track*>(pin);
  return sticky_capacity(c, meta[2], false);   // like mot_get_tracks: the step has run and the records are delivered
}

extern "C" int mot_track_get_state(mot_ctx* c, int slot, int id, mot_track_state* o) {
  if (!c) return MOT_E_ARG;
  MOT_GUARD(c);
  if (slot < 0 || slot >= c->batch || !o || id < 0) return fail(c, MOT_E_ARG, "mot_track_get_state: slot / id out of range or null result");
  int nt = 0;
  MOT_HIP(c, hipMemcpyAsync(&nt, c->d_nt + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (id >= nt) return fail(c, MOT_E_ARG, "no such track");
  int sl = -1;
  MOT_HIP(c, hipMemcpyAsync(&sl, c->d_slot_of + (size_t)slot * c->max_tracks_ever + id, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  if (sl < 0 || sl >= c->max_tracks_total) return fail(c, MOT_E_STATE, "mot_track_get_state: the track died more than a step ago; its filter state has been evicted");
  DevTrack t;
  MOT_HIP(c, hipMemcpyAsync(&t, c->d_tracks + (size_t)slot * c->max_tracks_total + sl, sizeof t, hipMemcpyDeviceToHost, c->stream));
  MOT_HIP(c, hipStreamSynchronize(c->stream));
  memset(o, 0, sizeof *o);
  memcpy(o->x_merge, t.x[0], 40); memcpy(o->x_cv, t.x[1], 40); memcpy(o->x_ctrv, t.x[2], 40); memcpy(o->x_rm, t.x[3], 40);
  memcpy(o->p_merge, t.P[0], 200); memcpy(o->p_cv, t.P[1], 200); memcpy(o->p_ctrv, t.P[2], 200); memcpy(o->p_rm, t.P[3], 200);
  memcpy(o->mode_prob, t.mode, 24); memcpy(o->z_pred, t.zpred, sizeof t.zpred); memcpy(o->s, t.S, sizeof t.S); memcpy(o->k, t.K, sizeof t.K);
  o->init_meas[0] = t.init_meas[0]; o->init_meas[1] = t.init_meas[1]; o->dist_from_init = t.dist_from_init; o->best_yaw = t.best_yaw;
  o->lifetime = t.lifetime; o->track_manage = t.track_num; o->is_static = t.is_static; o->is_vis = t.is_vis; o->has_best_box = t.has_best;
  if (t.has_bbox) memcpy(o->bbox, t.bbox, sizeof t.bbox);
  if (t.has_best) memcpy(o->best_bbox, t.best_bbox, sizeof t.best_bbox);
  return MOT_OK;
}

// test hook (mot_debug_api.h): the float matrix of the fused path's sensor -> global change of frame for an ego pose
extern "C" int mot_debug_tf_matrix(double x, double y, double yaw, float* m12) {
  if (!m12) return MOT_E_ARG;
  tf_velodyne_to_global(x, y, yaw, m12);
  return MOT_OK;
}

// test hook (mot_debug_api.h): the float matrix of the way back, global -> sensor, for an ego pose
extern "C" int mot_debug_tf_matrix_inv(double x, double y, double yaw, float* m12) {
  if (!m12) return MOT_E_ARG;
  tf_global_to_velodyne(x, y, yaw, m12);
  return MOT_OK;
}
