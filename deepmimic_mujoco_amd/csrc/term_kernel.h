// term_kernel.h — the floor-contact query and DeepMimic's early termination.  Included by dmenv.hip after kernels.h;
// k_floor_contacts is launched from views.hip (dm_batch_floor_contacts), k_terminate from dmenv.hip's step_impl.
//
//   k_floor_contacts  one wave per state: the step kernels' kinematics (stage_kinematics) at the state's qpos, then one lane per geom decides
//                     whether the collision stage's narrow phase would emit a contact for (floor, geom) (floor_contact.h); bit g of out[v].
//                     A read-only kernel beside the step kernels: it changes no batch state and none of their instruction streams.
//   k_terminate       one wave per environment of a part, AFTER the part's step launches on the same stream (DM_OPT_FALL_BODIES,
//                     DM_OPT_MAX_EPISODE_STEPS): counts the episode's steps, tests the state the step left for a fall contact and the step
//                     limit, and ends the episode where either fires — done, the reason, and with DM_OPT_AUTORESET the tail of the step
//                     kernels' epilogue (reset_env, the fresh observation row, store_state).  The step kernels carry none of this: with both
//                     options off the launch is not issued.  With DM_OPT_TRUNCATION_LOG it first appends the state of an episode that the time
//                     limit alone ends to the batch's truncation log (dm_batch_truncations).
#pragma once

#include "floor_contact.h"

// what k_terminate needs beyond the batch: an argument struct of its own (dm::Batch is passed by value to every kernel and stays as it is)
struct TermArgs {
  int* steps;              // [N] DM_F_EPISODE_STEPS
  int* reason;             // [N] DM_F_DONE_REASON
  unsigned fall_bodies;    // DM_OPT_FALL_BODIES
  int max_steps;           // DM_OPT_MAX_EPISODE_STEPS
  int first, count;        // the part's env range
  // the truncation log (DM_OPT_TRUNCATION_LOG): the state an episode had when the time limit ALONE ended it, kept for the
  // learner's value bootstrap before reset_env overwrites it.  log_cap = 0: off, nothing below is read.
  int* log_count;          // [1] records appended since the log was cleared (keeps counting beyond log_cap: overflow is visible)
  int* log_index;          // [log_cap, 4] {env, tick, frame_idx, frame_init}
  double* log_qpos;        // [log_cap, 35]
  double* log_qvel;        // [log_cap, 34]
  int log_cap, tick;       // capacity in records; the batch's step calls since the log was cleared
};

#ifndef DM_TERM_ARGS_ONLY      // (slot_term.h — the horizon launch's termination phase, a unit of its own — wants the struct alone)
// bit g (1..15) of the result: geom g touches the floor at the kinematics in `s` (wave-collective; the same value in every lane)
DM_DEV unsigned floor_touch_mask(const DevModel<Real>& M, const Shared<Real>& s, int lane) {
  bool t = false;
  if (lane >= 1 && lane < NG) t = dmfc::geom_touches_floor(lane, M.geom_body, M.geom_type, M.geom_pos, M.geom_mat, M.geom_size, M.geom_margin, s.xpos, s.xmat);
  return (unsigned)dmw::ballot(t);
}

#ifndef DM_TERM_NO_KERNELS    // (kernels_clips.hip — the clip form of k_terminate, a unit of its own — wants the struct and the floor test)
// state v: an explicit pose (qpos_ext [n,35]) or the batch's state of env env_ids[v] (or v)
__global__ __launch_bounds__(64) void k_floor_contacts(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos,
                                                       const double* __restrict__ qpos_ext, const int* __restrict__ env_ids, int* __restrict__ out) {
  __shared__ Shared<Real> s;
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  if (lane < NQ) s.qpos[lane] = qpos_ext ? (Real)qpos_ext[(size_t)v * NQ + lane] : state_qpos[(size_t)(env_ids ? env_ids[v] : v) * NQ + lane];
  dmw::sync();
  stage_kinematics(M, s, lane, lane_topo(lane));          // ends with a sync
  const unsigned m = floor_touch_mask(M, s, lane);
  if (lane == 0) out[v] = (int)m;
}

__global__ __launch_bounds__(64) void k_terminate(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, TermArgs T, Ext* __restrict__ obs,
                                                  unsigned char* __restrict__ done) {
  __shared__ Shared<Real> s;
  if ((int)blockIdx.x >= T.count) return;
  const int env = T.first + (int)blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  // the step kernel ended the episode itself (COM band, clip end): the state may already be a fresh episode's, and a reference pose of a
  // floor clip legitimately touches the floor — nothing is tested
  if (dmw::uniform((int)done[env]) != 0) {
    const TermVerdict v = term_verdict(true, 0, T.max_steps);
    if (lane == 0) { T.reason[env] = v.reason(false); T.steps[env] = v.steps_kept(false); }
    return;
  }
  const TermVerdict v = term_verdict(false, dmw::uniform(T.steps[env]), T.max_steps);
  load_env(M, B, s, env, lane, (const double*)0);         // ends with a hand-off
  bool fall = false;
  if (T.fall_bodies) {
    stage_kinematics(M, s, lane, lane_topo(lane));
    fall = (floor_touch_mask(M, s, lane) & dmfc::geoms_of_bodies(T.fall_bodies, M.geom_body, NG)) != 0u;
  }
  if (!v.ends(fall)) {
    if (lane == 0) { T.steps[env] = v.steps_kept(fall); T.reason[env] = v.reason(fall); }
    return;
  }
  if (T.log_cap > 0 && !fall) {                           // ended by the time limit alone: a truncation, not a failure — log the state the step left
    int slot = 0;
    if (lane == 0) slot = atomicAdd(T.log_count, 1);      // (device scope: pipelined parts on other streams share the counter)
    slot = dmw::uniform(slot);
    if (slot < T.log_cap) {
      if (lane < 4) T.log_index[(size_t)slot * 4 + lane] = trunc_index_value(lane, env, T.tick, B);
      if (lane < NQ) T.log_qpos[(size_t)slot * NQ + lane] = (double)s.qpos[lane];
      if (lane < NV) T.log_qvel[(size_t)slot * NV + lane] = (double)s.qvel[lane];
    }
  }
  if (lane == 0) { done[env] = 1; T.reason[env] = v.reason(fall); T.steps[env] = v.steps_kept(fall); }
  if (B.autoreset) {                                      // the tail of env_step_impl's epilogue: the fresh episode's state and observation row
    dmw::sync_mem();
    reset_env(M, B, s, env, lane, B.autoreset == 1 ? 0 : 1, 1);
    if (lane < NOBS) obs[(size_t)env * NOBS + lane] = obs_element(s.qpos, s.qvel, lane);
    store_state(B, s, env, lane);
    if (lane == 0 && B.kin) B.kin_ok[env] = 0;            // the parked kinematics belong to the old state
  }
}

// dm_batch_reset: the step counters of the masked environments start again
__global__ void k_zero_masked(int* __restrict__ v, const unsigned char* __restrict__ mask, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) v[i] = 0;
}
#endif  // DM_TERM_NO_KERNELS
#endif  // DM_TERM_ARGS_ONLY
