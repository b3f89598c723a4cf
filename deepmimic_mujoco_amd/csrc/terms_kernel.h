// terms_kernel.h — dm_batch_imitation_terms' launch.  Included by dmenv.hip after kernels.h; launched from views.hip.
//
//   k_imitation_terms  one wave per state: the step kernels' kinematics at the state, then the lane code of reward mode 3 itself —
//                      imitation_reward<Real, true> (env_step.h), the step's own text with the blocks that keep what the step throws away:
//                      lanes 0..12 the root and the joint groups, lanes 13..16 the end effectors, lanes 0..33 the momentum per dof.  The lanes
//                      leave the 28 numbers (include/dmenv.h DM_NTERMS) in an LDS row and the wave writes it as one run.  A read-only kernel
//                      beside the step kernels: it changes no batch state and none of their instruction streams.
//
// Unlike k_state_features the kinematics keep the root's x and y: the root term compares them with the reference's (plus the cycle shift).
#pragma once

// state v: explicit (qpos_ext [n,35], qvel_ext [n,34], frame_ext [n], cycle_ext [n] or NULL = 0) or the batch's state and cursors of env
// env_ids[v] (or v).  A frame outside [0, n_frames) gives a row of NaNs: the lanes then work on table row 0 and the result is not stored.
__global__ __launch_bounds__(64) void k_imitation_terms(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                                        const double* __restrict__ qvel_ext, const int* __restrict__ frame_ext,
                                                        const int* __restrict__ cycle_ext, const int* __restrict__ env_ids, Ext* __restrict__ out) {
  __shared__ Shared<Real> s;
  __shared__ Real row[IMIT_NTERMS];
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  const int env = qpos_ext ? v : dmw::uniform(env_ids ? env_ids[v] : v);
  if (lane < NQ) s.qpos[lane] = qpos_ext ? (Real)qpos_ext[(size_t)v * NQ + lane] : B.qpos[(size_t)env * NQ + lane];
  if (lane < NV) s.qvel[lane] = qpos_ext ? (Real)qvel_ext[(size_t)v * NV + lane] : B.qvel[(size_t)env * NV + lane];
  const int k = dmw::uniform(qpos_ext ? frame_ext[v] : B.frame_idx[env]);
  const int cyc = dmw::uniform(qpos_ext ? (cycle_ext ? cycle_ext[v] : 0) : B.cycle[env]);
  const bool inside = k >= 0 && k < B.n_frames;
  dmw::sync();
  imitation_reward<Real, true>(M, B, s, lane, lane_topo(lane), B.imit_table + (size_t)(inside ? k : 0) * IMIT_FEAT, cyc * B.imit_params[13],
                               cyc * B.imit_params[14], row);
  dmw::sync();
  if (lane < IMIT_NTERMS) out[(size_t)v * IMIT_NTERMS + lane] = inside ? (Ext)row[lane] : (Ext)NAN;
}
