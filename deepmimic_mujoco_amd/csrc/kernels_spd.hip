// kernels_spd.hip — the one-environment-per-wavefront step kernels of action modes 3 and 4 (stable PD control per substep: env_step.h spd_control).
// k_step_narrow, k_step_act, k_step, k_step_redo and k_step_prof of dmenv.hip with the controller compiled in (env_step_impl<.., SPD = true>), in a
// translation unit of their own so that the kernels of modes 0..2 stay the code objects they were; default backend options, as dmenv.hip.
// (the bodies stay written out in both units: through a shared template, as packed_body.h has for the packed kernels, every one of the ten kernels' code
//  objects came out different — profiles/host_split.md)
#define DM_NO_LAUNCH_KERNELS
#include "kernels.h"

using namespace dm;

__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_narrow_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                        Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                        int n_substeps, int first, int count) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step_impl<Real, NARROW_ROWS, false, true>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
}
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_act_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                     Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                     int n_substeps, int first, int count, dmp::PolicyArgs pa) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step_impl<Real, NARROW_ROWS, false, true>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
  static_assert(sizeof(s.u) >= 464 * sizeof(float), "policy scratch");
  dmw::sync();
  dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u));
}
__global__ __launch_bounds__(64) void k_step_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                 Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                 int n_substeps) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  env_step_impl<Real, MAXEFC, false, true>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
}
// the packed launch's overflowing environments, re-stepped from their unchanged state with the same control rule (see k_step_redo)
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_redo_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                      Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                      int n_substeps, int first, const int* __restrict__ redo_count, int* __restrict__ redo_count_next, dmp::PolicyArgs pa) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int n = dmw::uniform(*redo_count);
  if (blockIdx.x == 0 && threadIdx.x == 0) *redo_count_next = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0) atomicAdd(B.redo_why, n);
  for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
    const int env = B.redo_list[first + i];
    env_step_impl<Real, NARROW_ROWS, false, true>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
    if (pa.P) { dmw::sync(); dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u)); }
    dmw::sync_mem();
  }
}
__global__ __launch_bounds__(64) void k_step_prof_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                      Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                      int n_substeps, long long* prof) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  env_step_impl<Real, MAXEFC, true, true>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, prof);
}
