// state_features.h — the per-body arithmetic of dm_batch_state_features (include/dmenv.h DM_NSTATE): DeepMimic's
// state features (cCtController::BuildStatePose / BuildStateVel as quoted in the reference's notes, code.md:307-489) of one humanoid state.
//
// Plain functions on plain arrays, templated on the real type, with no HIP dependency: state_kernel.h calls them from k_state_features
// (hipcc, gfx950, float64 and float32), and the CPU tests build the same file with a host compiler (tests/state_host.cpp) to check this
// arithmetic against the float64 restatement without a GPU.  That host build is test infrastructure; libdmenv.so has no CPU path.
//
// Inputs are what forward kinematics gives: the bodies' frame origins xpos [14][3], their unit quaternions xquat [14][4] (w, x, y, z), their
// centres of mass xipos [14][3], the world axis of every dof (dof d at axis + d * axis_stride; the free joint's rotational dofs 3..5 are the
// columns of the root's rotation: MuJoCo's free-joint angular velocity is body-local), and qvel [34].
#pragma once

#include "topology.h"

#if defined(__HIPCC__)
#define SF_FN __host__ __device__ __forceinline__
#else
#define SF_FN inline
#endif

namespace dmsf {

constexpr int NBODY = dmt::NB - 1;                              // model bodies 1..13, k = b - 1
constexpr int POSE_W = 7, VEL_W = 6;                            // per body: position [3] + quaternion [4]; linear [3] + angular [3] velocity
constexpr int O_PHASE = 0, O_HEIGHT = 1, O_POS = 2, O_VEL = O_POS + POSE_W * NBODY;
constexpr int NSTATE = O_VEL + VEL_W * NBODY;
static_assert(NSTATE == 171 && O_VEL == 93, "the layout include/dmenv.h documents");

// the heading frame of a state: cos / sin of the heading hd = atan2(f_y, f_x), f = the root's x axis in the world, and of hd / 2
template <class R>
struct Heading {
  R c, s, ch, sh;
};

template <class R> SF_FN R sf_sqrt(R x) { return (R)__builtin_sqrt((double)x); }
template <> SF_FN float sf_sqrt<float>(float x) { return __builtin_sqrtf(x); }
template <class R> SF_FN R sf_copysign(R m, R s) { return (R)__builtin_copysign((double)m, (double)s); }
template <> SF_FN float sf_copysign<float>(float m, float s) { return __builtin_copysignf(m, s); }

// rq: the root quaternion as stored (normalised here).  No angle is ever formed: cos hd = f_x / |f_xy|, sin hd = f_y / |f_xy|, and the half
// angle comes from whichever of (1 + cos) / 2, (1 - cos) / 2 does not cancel.  A vertical root x axis (f_x = f_y = 0) has heading 0, as
// atan2(0, 0) does; sin hd = -0 gives hd = -pi, as atan2 does.
template <class R>
SF_FN Heading<R> heading(const R* rq) {
  const R n2 = rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3];
  const R k = R(1) / n2;                                        // (f of the normalised quaternion = f of the stored one / |q|^2)
  const R fx = (rq[0] * rq[0] + rq[1] * rq[1] - rq[2] * rq[2] - rq[3] * rq[3]) * k, fy = R(2) * (rq[1] * rq[2] + rq[0] * rq[3]) * k;
  const R n = sf_sqrt(fx * fx + fy * fy);
  Heading<R> h;
  if (!(n > R(0))) { h.c = 1; h.s = 0; h.ch = 1; h.sh = 0; return h; }
  h.c = fx / n; h.s = fy / n;
  if (h.c >= R(0)) { h.ch = sf_sqrt((R(1) + h.c) * R(0.5)); h.sh = h.s / (R(2) * h.ch); }
  else { h.sh = sf_copysign(sf_sqrt((R(1) - h.c) * R(0.5)), h.s); h.ch = h.s / (R(2) * h.sh); }
  return h;
}

// out = Rz(-hd) v
template <class R>
SF_FN void to_heading(const Heading<R>& h, const R* v, R* out) {
  const R x = h.c * v[0] + h.s * v[1], y = h.c * v[1] - h.s * v[0];
  out[0] = x; out[1] = y; out[2] = v[2];
}

// out = q_z(-hd) (x) q, negated as a whole when its w < 0 (code.md:406-412)
template <class R>
SF_FN void quat_to_heading(const Heading<R>& h, const R* q, R* out) {
  R w = h.ch * q[0] + h.sh * q[3], x = h.ch * q[1] + h.sh * q[2], y = h.ch * q[2] - h.sh * q[1], z = h.ch * q[3] - h.sh * q[0];
  if (w < R(0)) { w = -w; x = -x; y = -y; z = -z; }
  out[0] = w; out[1] = x; out[2] = y; out[3] = z;
}

template <class R>
SF_FN void cross_acc(R* out, const R* a, const R* b) {
  out[0] += a[1] * b[2] - a[2] * b[1]; out[1] += a[2] * b[0] - a[0] * b[2]; out[2] += a[0] * b[1] - a[1] * b[0];
}

// world velocity of the point c of body b and the body's world angular velocity, from the dofs of b and of its ancestors: every such body a
// turns about its own frame origin with w_a = sum of its dofs' axis * rate, so  v = qvel[0:3] + sum_a w_a x (c - xpos_a),  w = sum_a w_a.
// Each lever arm is a difference of two nearby points: nothing is referred to the world origin.  T: the tree (dmt::Topo).
template <class R, class T>
SF_FN void body_velocity(const T& topo, int b, const R* c, const R (*xpos)[3], const R* axis, int axis_stride, const R* qvel, R* v, R* w) {
  v[0] = qvel[0]; v[1] = qvel[1]; v[2] = qvel[2];
  w[0] = w[1] = w[2] = 0;
  for (int a = b; a > 0; a = topo.body_parent[a]) {
    const int d0 = a == 1 ? 3 : topo.body_dofadr[a], nd = a == 1 ? 3 : topo.body_dofnum[a];
    R wa[3] = {0, 0, 0};
    for (int k = 0; k < nd; k++) {
      const R* ax = axis + (d0 + k) * axis_stride;
      const R qd = qvel[d0 + k];
      wa[0] += ax[0] * qd; wa[1] += ax[1] * qd; wa[2] += ax[2] * qd;
    }
    const R r[3] = {c[0] - xpos[a][0], c[1] - xpos[a][1], c[2] - xpos[a][2]};
    cross_acc(v, wa, r);
    w[0] += wa[0]; w[1] += wa[1]; w[2] += wa[2];
  }
}

// the 13 numbers of body b (1..13) into its two slots of `row` [NSTATE]
template <class R, class T>
SF_FN void body_features(const T& topo, const Heading<R>& h, int b, const R (*xpos)[3], const R (*xquat)[4], const R (*xipos)[3], const R* axis,
                         int axis_stride, const R* qvel, R* row) {
  const int k = b - 1;
  const R rel[3] = {xipos[b][0] - xpos[1][0], xipos[b][1] - xpos[1][1], xipos[b][2] - xpos[1][2]};
  to_heading(h, rel, row + O_POS + POSE_W * k);
  quat_to_heading(h, xquat[b], row + O_POS + POSE_W * k + 3);
  R v[3], w[3];
  body_velocity(topo, b, xipos[b], xpos, axis, axis_stride, qvel, v, w);
  to_heading(h, v, row + O_VEL + VEL_W * k);
  to_heading(h, w, row + O_VEL + VEL_W * k + 3);
}

// phase of the clip from the batch's cursor fields (include/dmenv.h): reward modes 2 (v2-pose) and 4 (v1-quat) count steps from 0 and add the RSI draw
SF_FN double phase_of(int reward_mode, int frame_idx, int frame_init, int n_frames) {
  long long k = frame_idx;
  if (reward_mode == 2 || reward_mode == 4) k += frame_init;
  k %= n_frames;
  if (k < 0) k += n_frames;
  return (double)k / (double)n_frames;
}

}  // namespace dmsf
