// push_kernel.h — external pushes (include/dmenv.h dm_batch_push, dm_batch_set_push_schedule): an impulse p (N s, world frame) at the
// centre of mass of model body b changes the velocity by  dqvel = M(q)^-1 J_b(q)^T p  at the state the environment is in.  One wave per environment, beside
// the step kernels, whose code and signatures stay as they are:
//   k_push_now   dm_batch_push: the caller's body and impulse per environment, one launch on the batch's stream
//   k_push       the random schedule (PushArgs): BEFORE every per-step launch of a part while a schedule is set.  Every lane works the env's state machine out
//                on wave-uniform values, lane 0 stores it; a wave with nothing to apply returns before it touches LDS.  A force F held over an env step is
//                the single impulse F h before that step, h = timestep * n_substeps formed in float64 (first-order splitting of an applied force: exact for
//                one unconstrained Euler step, not identical under RK4).
// Both apply the impulse through push_impulse: the step's own kinematics, mass matrix (armature included) and L^T D L solves.  Only qvel is stored: qpos,
// time, the warm start, the cursors and the parked kinematics (position-only) are untouched; contacts and joint limits are ignored — the next step's
// constraint solve meets the new velocity.
#pragma once

#include "env_step.h"

namespace dm {

// what the push kernels need beyond the batch: an argument struct of its own, as TermArgs and ClipArgs are
struct PushArgs {
  int* state;                  // [N,5] DM_F_PUSH_STATE {episode_seen, wait, left, body, count}
  double* force;               // [N,3] DM_F_PUSH_FORCE (float64 in both libraries)
  unsigned bodies;             // dm_push_desc
  int wait_min, wait_max, dur_min, dur_max;
  double force_min, force_max, z_min, z_max;
  double h;                    // timestep * n_substeps of the step this launch precedes, in float64
  int first, count;            // the part's env range
};

// an impulse is applied when its body is a model body and it is finite and not zero (a zero impulse leaves qvel bit for bit, the sign of a zero included)
DM_DEV bool push_applies(int body, double px, double py, double pz) {
  const double big = 1.7976931348623157e308;
  const bool finite = fabs(px) <= big && fabs(py) <= big && fabs(pz) <= big;
  return body >= 1 && body < NB && finite && (px != 0.0 || py != 0.0 || pz != 0.0);
}

// qvel[env] += M^-1 J_b^T p, wave-collective; `body` (1..13) and p are wave-uniform.  (J_b^T p)_d for a dof d on the chain root -> b is p . (w_d x c + v_d) with
// (w_d, v_d) = cdof[d], the dof's motion axis about the world origin, and c = xipos[b]: the hinge's  axis x (c - xpos_body(d)), the identity for the root's
// translation, xmat_root[:, k] x (c - xpos_root) for its rotation; zero off the chain.
template <class R>
DM_DEV void push_impulse(const DevModel<R>& M, const Batch<R>& B, Shared<R>& s, int env, int lane, int body, R px, R py, R pz) {
  const LaneTopo lt = lane_topo(lane);
  load_env(M, B, s, env, lane, (const double*)0);         // ends with a hand-off
  stage_tables(s, lane);
  dmw::sync();
  stage_kinematics(M, s, lane, lt);
  stage_mass_matrix(M, s, lane, lt, (const DebugOut*)0);  // ends with a sync: s.u is free for the solves' exchange
  R rhs = 0;
  if (lane < NV && ((TOPO.chain[body] >> lane) & 1ull)) {
    const R* cd = s.cdof[lane];
    const R* c = s.xipos[body];
    R j[3];
    cross3(j, cd, c);
    j[0] += cd[3]; j[1] += cd[4]; j[2] += cd[5];
    rhs = j[0] * px + j[1] * py + j[2] * pz;
  }
  R mine = lane_solve_LT(s, lane, rhs);
  if (lane < NV) mine *= s.dinv[lane];
  dmw::sync();
  const R dv = lane_solve_L(s, lane, mine);
  if (lane < NV) B.qvel[(size_t)env * NV + lane] = s.qvel[lane] + dv;
}

// the integer draw  lo + min(floor(u (hi - lo + 1)), hi - lo)
DM_DEV int push_draw_int(double u, int lo, int hi) {
  const int span = hi - lo;
  int k = (int)floor(u * (double)(span + 1));
  if (k > span) k = span;
  return lo + k;
}
// the k-th set bit of `mask`, ascending, k = floor(u popcount(mask)) clamped
DM_DEV int push_draw_body(double u, unsigned mask) {
  int cnt = 0;
  for (int b = 1; b < NB; b++) cnt += (int)((mask >> b) & 1u);
  int k = (int)floor(u * (double)cnt);
  if (k > cnt - 1) k = cnt - 1;
  for (int b = 1; b < NB; b++) if ((mask >> b) & 1u) { if (k == 0) return b; k--; }
  return 0;
}

// The schedule's rule for one environment and one step (include/dmenv.h has it in words), on wave-uniform values: st = {episode_seen, wait, left, body,
// count} and F are updated in place; -> whether the impulse F h on body st[3] is applied before this step.  u_k(j) = rng_uniform(seed, genv, ep, 256 + 8 j + k).
DM_DEV bool push_schedule_step(const PushArgs& P, unsigned long long seed, int genv, int ep, int* st, double* F) {
  if (st[0] != ep) {
    st[0] = ep; st[4] = 0; st[2] = 0;
    st[1] = push_draw_int(rng_uniform(seed, genv, ep, 256), P.wait_min, P.wait_max);
  }
  if (st[2] == 0) {
    if (st[1] > 0) { st[1] -= 1; return false; }
    const int j = 256 + 8 * st[4];
    st[2] = push_draw_int(rng_uniform(seed, genv, ep, j + 1), P.dur_min, P.dur_max);
    st[3] = push_draw_body(rng_uniform(seed, genv, ep, j + 2), P.bodies);
    const double mag = P.force_min + rng_uniform(seed, genv, ep, j + 3) * (P.force_max - P.force_min);
    const double phi = 6.283185307179586476925 * rng_uniform(seed, genv, ep, j + 4);
    const double z = P.z_min + rng_uniform(seed, genv, ep, j + 5) * (P.z_max - P.z_min);
    const double rxy = sqrt(1.0 - z * z);
    F[0] = mag * (rxy * cos(phi)); F[1] = mag * (rxy * sin(phi)); F[2] = mag * z;
    st[4] += 1;
  }
  st[2] -= 1;
  if (st[2] == 0) st[1] = push_draw_int(rng_uniform(seed, genv, ep, 256 + 8 * st[4]), P.wait_min, P.wait_max);
  return true;
}

// ---- the two kernels' waves (kernels_push.hip launches them; the wave testbench runs them as they are) -------------------------------------------------------
// k_push_now's wave for env `env`: body[env] (0 or outside 1..13: untouched), impulse[env] (N s, world frame), mask[env] (null: every env)
template <class R>
DM_DEV void push_now_wave(const DevModel<R>& M, const Batch<R>& B, Shared<R>& s, int env, int lane, const int* body, const double* impulse, const unsigned char* mask) {
  if (mask && dmw::uniform((int)mask[env]) == 0) return;
  const int b = dmw::uniform(body[env]);
  const double px = impulse[(size_t)env * 3], py = impulse[(size_t)env * 3 + 1], pz = impulse[(size_t)env * 3 + 2];
  if (!dmw::uniform(push_applies(b, px, py, pz))) return;
  push_impulse(M, B, s, env, lane, b, (R)px, (R)py, (R)pz);
}
// k_push's wave for env `env`: every lane works the record out on wave-uniform values, lane 0 stores it; nothing to apply: back before LDS is touched
template <class R>
DM_DEV void push_schedule_wave(const DevModel<R>& M, const Batch<R>& B, Shared<R>& s, const PushArgs& P, int env, int lane) {
  int st[5];
  double F[3];
  for (int k = 0; k < 5; k++) st[k] = dmw::uniform(P.state[(size_t)env * 5 + k]);
  for (int k = 0; k < 3; k++) F[k] = P.force[(size_t)env * 3 + k];
  const bool apply = dmw::uniform(push_schedule_step(P, B.seed, B.env_offset + env, dmw::uniform(B.episode[env]), st, F));
  dmw::sync();                                            // every lane has read the record before lane 0 replaces it
  if (lane == 0) {
    for (int k = 0; k < 5; k++) P.state[(size_t)env * 5 + k] = st[k];
    for (int k = 0; k < 3; k++) P.force[(size_t)env * 3 + k] = F[k];
  }
  const double px = F[0] * P.h, py = F[1] * P.h, pz = F[2] * P.h;
  if (!apply || !dmw::uniform(push_applies(st[3], px, py, pz))) return;
  push_impulse(M, B, s, env, lane, st[3], (R)px, (R)py, (R)pz);
}

}  // namespace dm
