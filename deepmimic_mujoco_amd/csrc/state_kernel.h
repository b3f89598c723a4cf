// state_kernel.h — dm_batch_state_features' launch.  Included by dmenv.hip after kernels.h; launched from views.hip.
//
//   k_state_features  one wave per state: the step kernels' kinematics (stage_kinematics) at the state's qpos, then one lane per body forms
//                     its 13 numbers (state_features.h: heading frame, quaternion product and sign rule, the velocity of its centre of mass
//                     and its angular velocity from its ancestor dofs) into an LDS row, and the wave writes the 171 values as one coalesced
//                     row.  A read-only kernel beside the step kernels: it changes no batch state and none of their instruction streams.
//
// The features do not depend on the root's x and y, so the kinematics run with both set to 0: the float32 build then keeps its precision
// however far the humanoid has walked from the world origin.
#pragma once

#include "state_features.h"

// state v: explicit (qpos_ext [n,35], qvel_ext [n,34], phase_ext [n]) or the batch's state of env env_ids[v] (or v)
__global__ __launch_bounds__(64) void k_state_features(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                                       const double* __restrict__ qvel_ext, const double* __restrict__ phase_ext,
                                                       const int* __restrict__ env_ids, Ext* __restrict__ out) {
  __shared__ Shared<Real> s;
  __shared__ Real row[dmsf::NSTATE];
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  const int env = qpos_ext ? v : dmw::uniform(env_ids ? env_ids[v] : v);
  if (lane < NQ) s.qpos[lane] = lane < 2 ? Real(0) : (qpos_ext ? (Real)qpos_ext[(size_t)v * NQ + lane] : B.qpos[(size_t)env * NQ + lane]);
  if (lane < NV) s.qvel[lane] = qpos_ext ? (Real)qvel_ext[(size_t)v * NV + lane] : B.qvel[(size_t)env * NV + lane];
  const double phase = qpos_ext ? phase_ext[v] : dmsf::phase_of(B.reward_mode, B.frame_idx[env], B.frame_init[env], B.n_frames);
  dmw::sync();
  stage_kinematics(M, s, lane, lane_topo(lane));          // ends with a sync; leaves xpos, xipos, the unit xquat and the world dof axes (cdof[d][0:3])
  if (lane < dmsf::NBODY) {
    const dmsf::Heading<Real> h = dmsf::heading(s.ua.xquat[1]);
    dmsf::body_features(TOPO, h, lane + 1, s.xpos, s.ua.xquat, s.xipos, &s.cdof[0][0], 6, s.qvel, row);
  }
  if (lane == 0) row[dmsf::O_HEIGHT] = s.xpos[1][2];
  dmw::sync();
  Ext* o = out + (size_t)v * dmsf::NSTATE;
  for (int k = lane; k < dmsf::NSTATE; k += 64) o[k] = k == dmsf::O_PHASE ? (Ext)phase : (Ext)row[k];
}
