// kernels_clips.hip — the one-environment-per-wavefront kernels of a MULTI-CLIP batch (dm_mocap_create_set): every env imitates a clip of
// its own.  k_step, k_step_narrow, k_step_act and k_step_redo of dmenv.hip with the clip switch on (env_step_impl<.., CLIPS = ClipArgs>), and the clip forms of
// k_reset, k_terminate, k_state_features and k_imitation_terms.  A translation unit of its own, with dmenv.hip's default backend options, so that the kernels of
// single-clip batches stay the code objects they were.  An env is a wave here, so its clip view (step_rules.h clip_view) is wave-uniform.
// The step kernels pick the stable-PD instantiation by the batch's action mode at run time (env_step), as the wave testbench does, instead of doubling the kernel count.
#define DM_NO_LAUNCH_KERNELS
#include "kernels.h"

using namespace dm;
#define DM_TERM_NO_KERNELS
#include "term_kernel.h"
#include "state_features.h"

__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_narrow_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                          Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                          int n_substeps, int first, int count, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step<Real, NARROW_ROWS, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, (long long*)0, ca);
}
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_act_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                       Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                       int n_substeps, int first, int count, dmp::PolicyArgs pa, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step<Real, NARROW_ROWS, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, (long long*)0, ca);
  static_assert(sizeof(s.u) >= 464 * sizeof(float), "policy scratch");
  dmw::sync();
  dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u));
}
__global__ __launch_bounds__(64) void k_step_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                   Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                   int n_substeps, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  env_step<Real, MAXEFC, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, (long long*)0, ca);
}
// the packed launch's overflowing environments, re-stepped from their unchanged state (see k_step_redo)
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_redo_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                        Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                        int n_substeps, int first, const int* __restrict__ redo_count, int* __restrict__ redo_count_next, dmp::PolicyArgs pa,
                                                        ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int n = dmw::uniform(*redo_count);
  if (blockIdx.x == 0 && threadIdx.x == 0) *redo_count_next = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0) atomicAdd(B.redo_why, n);
  for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
    const int env = B.redo_list[first + i];
    env_step<Real, NARROW_ROWS, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, (long long*)0, ca);
    if (pa.P) { dmw::sync(); dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u)); }
    dmw::sync_mem();
  }
}

// dm_batch_set(DM_F_CLIP): a write leaves the cursors where they are, and a cursor of the old clip may lie beyond the new one — a step taken before the reset
// or set_state the contract asks for would then index the concatenated tables past the clip (past their end for the last clip).  The cursors that name a
// table row directly are therefore held inside the new clip: frame_init always, frame_idx where it is the frame (reward modes 0, 1 and 3).
__global__ void k_clip_clamp(Batch<Real> B, ClipArgs<Real> ca) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B.n_envs) return;
  const int last = ca.rec[ca.clip[env]].n_frames - 1;
  if (B.frame_init[env] > last) B.frame_init[env] = last;
  if (B.reward_mode != REW_V2_POSE && B.reward_mode != REW_V1_QUAT && B.frame_idx[env] > last) B.frame_idx[env] = last;
}

// dm_batch_reset (k_reset): DM_OPT_CLIP_MODE "episode" draws the env's clip before the frame
__global__ __launch_bounds__(64) void k_reset_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, int mode, int hard,
                                                    const unsigned char* __restrict__ mask, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  const int env = blockIdx.x, lane = dmw::lane();
  if (env >= B.n_envs) return;
  if (mask && !mask[env]) return;
  load_env(*Mp, B, s, env, lane, (const Ext*)0);
  reset_env_clips(*Mp, B, ca, s, env, lane, mode, hard);
  store_state(B, s, env, lane);
  { const LaneTopo lt = lane_topo(lane); stage_tables(s, lane); dmw::sync(); forward(*Mp, s, lane, lt, (const DebugOut*)0); }
  store_derived(B, *Mp, s, env, lane);
}

// early termination behind a step launch (term_kernel.h k_terminate, which see): the same verdict, log and stores; the reset is the clip form's
__global__ __launch_bounds__(64) void k_terminate_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, TermArgs T, Ext* __restrict__ obs,
                                                        unsigned char* __restrict__ done, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  if ((int)blockIdx.x >= T.count) return;
  const int env = T.first + (int)blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  if (dmw::uniform((int)done[env]) != 0) {
    const TermVerdict v = term_verdict(true, 0, T.max_steps);
    if (lane == 0) { T.reason[env] = v.reason(false); T.steps[env] = v.steps_kept(false); }
    return;
  }
  const TermVerdict v = term_verdict(false, dmw::uniform(T.steps[env]), T.max_steps);
  load_env(M, B, s, env, lane, (const double*)0);
  bool fall = false;
  if (T.fall_bodies) {
    stage_kinematics(M, s, lane, lane_topo(lane));
    fall = (floor_touch_mask(M, s, lane) & dmfc::geoms_of_bodies(T.fall_bodies, M.geom_body, NG)) != 0u;
  }
  if (!v.ends(fall)) {
    if (lane == 0) { T.steps[env] = v.steps_kept(fall); T.reason[env] = v.reason(fall); }
    return;
  }
  if (T.log_cap > 0 && !fall) {
    int slot = 0;
    if (lane == 0) slot = atomicAdd(T.log_count, 1);
    slot = dmw::uniform(slot);
    if (slot < T.log_cap) {
      if (lane < 4) T.log_index[(size_t)slot * 4 + lane] = trunc_index_value(lane, env, T.tick, B);
      if (lane < NQ) T.log_qpos[(size_t)slot * NQ + lane] = (double)s.qpos[lane];
      if (lane < NV) T.log_qvel[(size_t)slot * NV + lane] = (double)s.qvel[lane];
    }
  }
  if (lane == 0) { done[env] = 1; T.reason[env] = v.reason(fall); T.steps[env] = v.steps_kept(fall); }
  if (B.autoreset) {
    dmw::sync_mem();
    reset_env_clips(M, B, ca, s, env, lane, B.autoreset == 1 ? 0 : 1, 1);
    if (lane < NOBS) obs[(size_t)env * NOBS + lane] = obs_element(s.qpos, s.qvel, lane);
    store_state(B, s, env, lane);
    if (lane == 0 && B.kin) B.kin_ok[env] = 0;
  }
}

// dm_batch_state_features (state_kernel.h k_state_features): the phase runs over the length of the env's clip
__global__ __launch_bounds__(64) void k_state_features_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                                             const double* __restrict__ qvel_ext, const double* __restrict__ phase_ext,
                                                             const int* __restrict__ env_ids, Ext* __restrict__ out, ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ Real row[dmsf::NSTATE];
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  const int env = qpos_ext ? v : dmw::uniform(env_ids ? env_ids[v] : v);
  if (lane < NQ) s.qpos[lane] = lane < 2 ? Real(0) : (qpos_ext ? (Real)qpos_ext[(size_t)v * NQ + lane] : B.qpos[(size_t)env * NQ + lane]);
  if (lane < NV) s.qvel[lane] = qpos_ext ? (Real)qvel_ext[(size_t)v * NV + lane] : B.qvel[(size_t)env * NV + lane];
  const double phase = qpos_ext ? phase_ext[v] : dmsf::phase_of(B.reward_mode, B.frame_idx[env], B.frame_init[env], ca.rec[dmw::uniform(ca.clip[env])].n_frames);
  dmw::sync();
  stage_kinematics(M, s, lane, lane_topo(lane));
  if (lane < dmsf::NBODY) {
    const dmsf::Heading<Real> h = dmsf::heading(s.ua.xquat[1]);
    dmsf::body_features(TOPO, h, lane + 1, s.xpos, s.ua.xquat, s.xipos, &s.cdof[0][0], 6, s.qvel, row);
  }
  if (lane == 0) row[dmsf::O_HEIGHT] = s.xpos[1][2];
  dmw::sync();
  Ext* o = out + (size_t)v * dmsf::NSTATE;
  for (int k = lane; k < dmsf::NSTATE; k += 64) o[k] = k == dmsf::O_PHASE ? (Ext)phase : (Ext)row[k];
}

// dm_batch_imitation_terms (terms_kernel.h k_imitation_terms) against the clip of env env_ids[v] (or v; an explicit state's frame is local to that clip)
__global__ __launch_bounds__(64) void k_imitation_terms_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B_in, const double* __restrict__ qpos_ext,
                                                              const double* __restrict__ qvel_ext, const int* __restrict__ frame_ext,
                                                              const int* __restrict__ cycle_ext, const int* __restrict__ env_ids, Ext* __restrict__ out,
                                                              ClipArgs<Real> ca) {
  __shared__ Shared<Real> s;
  __shared__ Real row[IMIT_NTERMS];
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  const int env = qpos_ext ? v : dmw::uniform(env_ids ? env_ids[v] : v);
  const Batch<Real> B = ca.view_uniform(B_in, env);
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
