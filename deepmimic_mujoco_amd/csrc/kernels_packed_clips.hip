// kernels_packed_clips.hip — the four-environments-per-wavefront step kernels of a MULTI-CLIP batch (dm_mocap_create_set): the kernels of
// kernels_packed.hip with the clip switch on (slot_env_step_impl<.., CLIPS = ClipArgs>).  The four environments of a wave may imitate four different clips: the
// clip view is per slot, built from the clip's record (K x 48 bytes, resident in L2) at its uses in the action front end, the reward epilogue and the reset and
// not carried across the constraint solve.  A translation unit of its own, built with the packed backend options (csrc/build.py PACKED_FLAGS), so that the
// kernels of single-clip batches stay the code objects they were.  The stable-PD instantiation is picked by the batch's action mode at run time (slot_env_step).
#define DM_NO_LAUNCH_KERNELS
#include "kernels.h"

using namespace dm;

// (packed_body.h step_packed_body / step_packed_act_body with the clip argument; pa null: no fused policy step)
template <int MAXR>
static DM_DEV void step_packed_clips_body(const DevModel<Real>* __restrict__ Mp, const Batch<Real>& B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                          unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, const ClipArgs<Real>& ca,
                                          const dmp::PolicyArgs* pa) {
  __shared__ SlotShared<Real> sh[SLOTS];
  __shared__ SlotTables tb;
  const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  const bool stored = slot_env_step<Real, false, false, MAXR>(*Mp, B, sh[slot], tb, env, sl, lane, live, action, obs, reward, done, n_substeps, redo_count, B.redo_list + first,
                                                              (long long*)0, false, ca);
  if (!pa) return;
  static_assert(offsetof(SlotShared<Real>, r2) == offsetof(SlotShared<Real>, r1) + sizeof(sh[0].r1) && sizeof(sh[0].r1) + sizeof(sh[0].r2) >= 464 * sizeof(float), "policy scratch");
  dmw::sync();
  const int envs[4] = {dmw::bcast_i(env, 0), dmw::bcast_i(env, 16), dmw::bcast_i(env, 32), dmw::bcast_i(env, 48)};
  const int st = stored ? 1 : 0;
  const bool wr[4] = {dmw::bcast_i(st, 0) != 0, dmw::bcast_i(st, 16) != 0, dmw::bcast_i(st, 32) != 0, dmw::bcast_i(st, 48) != 0};
  dmp::policy_wave4<Real>(*pa, envs, wr, lane, reinterpret_cast<char*>(&sh[0]), (unsigned)sizeof(SlotShared<Real>), (unsigned)(offsetof(SlotShared<Real>, qpos) + 7 * sizeof(Real)),
                          (unsigned)(offsetof(SlotShared<Real>, qvel) + 6 * sizeof(Real)), (unsigned)offsetof(SlotShared<Real>, r1));
}

__global__ __launch_bounds__(64) void k_step_packed_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, ClipArgs<Real> ca) {
  step_packed_clips_body<2 * SW>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, ca, nullptr);
}
__global__ __launch_bounds__(64) void k_step_packed_ext_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, ClipArgs<Real> ca) {
  step_packed_clips_body<SLOT_MAXROWS>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, ca, nullptr);
}
__global__ __launch_bounds__(64) void k_step_packed_act_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa,
    ClipArgs<Real> ca) {
  step_packed_clips_body<2 * SW>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, ca, &pa);
}
__global__ __launch_bounds__(64) void k_step_packed_act_ext_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa,
    ClipArgs<Real> ca) {
  step_packed_clips_body<SLOT_MAXROWS>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, ca, &pa);
}
