// packed_body.h — bodies of the four-environments-per-wavefront per-step kernels, shared by kernels_packed.hip (action modes 0..2: SPD = false) and
// kernels_packed_spd.hip (action modes 3 and 4: SPD = true, the stable PD controller of slot_step.h slot_spd_control compiled in).
#pragma once
#include "kernels.h"

namespace dm {

// FOUR environments per wavefront (slot_kernel.h / slot_step.h): workgroup w steps the envs at dispatch positions first + 4 w .. + 3.
// Environments that exceed a capacity of that path are appended to the sub-batch's redo list instead of being stored ...
template <int MAXR, bool SPD>
DM_DEV void step_packed_body(const DevModel<Real>* __restrict__ Mp, const Batch<Real>& B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                             unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count) {
  __shared__ SlotShared<Real> sh[SLOTS];
  __shared__ SlotTables tb;
  const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  slot_env_step_impl<Real, false, false, MAXR, SPD>(*Mp, B, sh[slot], tb, env, sl, lane, live, action, obs, reward, done, n_substeps, redo_count, B.redo_list + first);
}
// ... followed, in the same wave, by the policy's step on the four observations it produced (dm_batch_step_act on the packed path): one
// weight stream per wave serves four environments
template <int MAXR, bool SPD>
DM_DEV void step_packed_act_body(const DevModel<Real>* __restrict__ Mp, const Batch<Real>& B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                 unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, const dmp::PolicyArgs& pa) {
  __shared__ SlotShared<Real> sh[SLOTS];
  __shared__ SlotTables tb;
  const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  const bool stored = slot_env_step_impl<Real, false, false, MAXR, SPD>(*Mp, B, sh[slot], tb, env, sl, lane, live, action, obs, reward, done, n_substeps, redo_count, B.redo_list + first);
  // s.qpos / s.qvel of every slot hold the state its observation was written from (the fresh episode's after an auto-reset); r1 is free
  // the r1 + r2 regions (adjacent) are free
  static_assert(offsetof(SlotShared<Real>, r2) == offsetof(SlotShared<Real>, r1) + sizeof(sh[0].r1) && sizeof(sh[0].r1) + sizeof(sh[0].r2) >= 464 * sizeof(float), "policy scratch");
  dmw::sync();
  const int envs[4] = {dmw::bcast_i(env, 0), dmw::bcast_i(env, 16), dmw::bcast_i(env, 32), dmw::bcast_i(env, 48)};
  const int st = stored ? 1 : 0;
  const bool wr[4] = {dmw::bcast_i(st, 0) != 0, dmw::bcast_i(st, 16) != 0, dmw::bcast_i(st, 32) != 0, dmw::bcast_i(st, 48) != 0};
  dmp::policy_wave4<Real>(pa, envs, wr, lane, reinterpret_cast<char*>(&sh[0]), (unsigned)sizeof(SlotShared<Real>), (unsigned)(offsetof(SlotShared<Real>, qpos) + 7 * sizeof(Real)),
                          (unsigned)(offsetof(SlotShared<Real>, qvel) + 6 * sizeof(Real)), (unsigned)offsetof(SlotShared<Real>, r1));
}
// the same with shader-clock stamps per stage, one record of 16 per wave (DM option 101 with option 105; diagnostic).  (k_step_packed_prof itself keeps this
// body written out in kernels_packed.hip: through this template its register allocation came out different — it stays the code object it was.)
template <bool SPD>
DM_DEV void step_packed_prof_body(const DevModel<Real>* __restrict__ Mp, const Batch<Real>& B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, long long* __restrict__ prof) {
  __shared__ SlotShared<Real> sh[SLOTS];
  __shared__ SlotTables tb;
  const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  slot_env_step_impl<Real, true, false, 2 * SW, SPD>(*Mp, B, sh[slot], tb, env, sl, lane, live, action, obs, reward, done, n_substeps, redo_count, B.redo_list + first, prof + (size_t)blockIdx.x * 32);
}

}  // namespace dm
