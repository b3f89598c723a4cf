// kernels_packed.hip — the four-environments-per-wavefront step kernels of libdmenv.so (see kernels.h; built by csrc/build.py with PACKED_FLAGS)
#define DM_NO_LAUNCH_KERNELS
#include "packed_body.h"

using namespace dm;

// (the bodies: packed_body.h; these are the kernels of action modes 0..2 — no controller code)
__global__ __launch_bounds__(64) void k_step_packed(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                    int n_substeps, int first, int count, int* __restrict__ redo_count) {
  step_packed_body<2 * SW, false>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count);
}
// The same launch with the three-set code compiled in (DM_OPT_PACKED = 2): 33 .. 40 rows stay in their wave, everything else runs ~8 % slower than in
// k_step_packed (slot_kernel.h slot_forward) — for populations that stand on both feet.  Horizon launches pick per wave-step instead (slot_step.h slot_rollout).
__global__ __launch_bounds__(64) void k_step_packed_ext(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                        Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                        int n_substeps, int first, int count, int* __restrict__ redo_count) {
  step_packed_body<SLOT_MAXROWS, false>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count);
}
__global__ __launch_bounds__(64) void k_step_packed_act(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                        Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                        int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa) {
  step_packed_act_body<2 * SW, false>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, pa);
}
__global__ __launch_bounds__(64) void k_step_packed_act_ext(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                            Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                            int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa) {
  step_packed_act_body<SLOT_MAXROWS, false>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, pa);
}
// the same with shader-clock stamps per stage, one record of 16 per wave (DM option 101 with option 105; diagnostic)
__global__ __launch_bounds__(64) void k_step_packed_prof(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                         Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                         int n_substeps, int first, int count, int* __restrict__ redo_count, long long* __restrict__ prof) {
  __shared__ SlotShared<Real> sh[SLOTS];
  __shared__ SlotTables tb;
  const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  slot_env_step_impl<Real, true, false, 2 * SW, false>(*Mp, B, sh[slot], tb, env, sl, lane, live, action, obs, reward, done, n_substeps, redo_count, B.redo_list + first, prof + (size_t)blockIdx.x * 32);
}
