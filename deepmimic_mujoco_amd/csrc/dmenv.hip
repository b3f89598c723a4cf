// dmenv.hip — libdmenv.so: the one-env step kernels of action modes 0..2, the reset / state / ordering kernels, and the batch half of the C ABI of
// include/dmenv.h: models, mocap tables and batches, options, state, step / rollout / queue, profiling and timing.  (views.hip: render and state
// features, whose kernels are compiled here; learner.hip: the learner half; kernels.h lists the units.)
// There is no CPU execution path in this library: every entry point that computes runs a HIP kernel.
#define DM_NO_LAUNCH_KERNELS
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "batch_host.h"
#include "model_host.h"

using namespace dm;
// the kernels of views.hip's entry points (written against namespace dm, like the kernels below) stay in this unit, beside the step kernels whose
// kinematics they share: in a unit of their own k_state_features and k_render_pose came out as different code objects (profiles/host_split.md)
#include "render_kernel.h"
#include "state_kernel.h"
#include "term_kernel.h"
#include "terms_kernel.h"
#include "push_kernel.h"
static_assert(DM_NSTATE == dmsf::NSTATE, "include/dmenv.h documents the feature row: keep it in step with state_features.h");
static_assert(DM_NTERMS == IMIT_NTERMS, "include/dmenv.h documents the terms row: keep it in step with env_step.h imitation_reward");
static_assert((DM_PACKED_MAXROWS == SLOT_MAXROWS || DM_SLOT_MAXROWS != 40 /* an experiment build */) && DM_PACKED_MAXROWS_PER_STEP == 2 * SW && DM_PACKED_MAXLIMROWS == SLOT_MAXLIMROWS && DM_PACKED_MAXCON == SLOT_MAXCON && DM_PACKED_MAXFRAME == SLOT_MAXFRAME &&
              DM_PACKED_MAXCAND == SLOT_MAXCAND, "include/dmenv.h documents the packed path's capacities: keep it in step with slot_kernel.h");
// ============================================ kernels ======================================================
// one 64-lane workgroup (= one wavefront) per environment.
// k_step_narrow (the timed path) keeps NARROW_ROWS columns of the constraint matrix A per env in registers, which fits
// 256 VGPRs -> 2 waves per SIMD; evaluations with more rows (up to MAXEFC = 64; < 1% in practice) keep the remaining
// columns in a per-env global-memory strip.  k_step holds all 64 columns in registers (512 VGPRs, 1 wave per SIMD) and is
// the single-tier fallback (DM option 102 = 0) and the profiling / debug instantiation.  Both perform identical
// arithmetic on the rows that exist.
static_assert(AOVF_COLS >= MAXEFC, "memory strip too small");
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_narrow(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                    int n_substeps, int first, int count) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
#ifdef DM_LDS_PAD      // experiment (profiles/r02_slot16_ubench.md): extra LDS per workgroup lowers the residency (6 880 -> 6 envs per CU,
  __shared__ volatile char lds_pad[DM_LDS_PAD];   // 20 500 -> 4) without touching the code path; build with DM_BUILD_DEFINES=-DDM_LDS_PAD=...
  if (n_substeps < 0) lds_pad[threadIdx.x] = 1;
#endif
  // position blockIdx.x in the dispatch order of the part [first, first + count) (a pipelined sub-batch, or the whole batch)
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step_impl<Real, NARROW_ROWS, false, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
}
// the same step followed, in the same wave, by the policy's step on the observation it produced (dm_batch_step_act)
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_act(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                 Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                 int n_substeps, int first, int count, dmp::PolicyArgs pa) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  if ((int)blockIdx.x >= count) return;
  int env;
  dispatch_env<1>(B, first, count, (int)blockIdx.x, dmw::lane(), blockIdx.x == 0, &env);
  env_step_impl<Real, NARROW_ROWS, false, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
  // s.qpos / s.qvel hold the state the observation was written from (the fresh episode's after an auto-reset); the row-descriptor
  // region is free
  static_assert(sizeof(s.u) >= 464 * sizeof(float), "policy scratch");
  dmw::sync();
  dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u));
}
__global__ __launch_bounds__(64) void k_step(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                             Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                             int n_substeps) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  env_step_impl<Real, MAXEFC, false, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
}

// the batch descriptor into device memory, stream-ordered before the horizon launch that reads it there
__global__ void k_put_batch(Batch<Real> B, Batch<Real>* __restrict__ dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = B; }
// the horizon's table of per-step buffers (slot_step.h StepRow), stream-ordered before the launch that reads it: rows of the caller's
// [T, N, .] tensors (dm_batch_rollout) ...
__global__ void k_fill_rows(StepRow* __restrict__ dst, const Ext* action, Ext* obs, Ext* reward, unsigned char* done, int T, size_t n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < T) dst[t] = StepRow{action + (size_t)t * n * NU, obs + (size_t)t * n * NOBS, reward + (size_t)t * n, done + (size_t)t * n};
}
// ... or the buffers of queued dm_batch_step calls (DM_OPT_STEP_QUEUE), a chunk of them per launch in the kernel-argument segment
__global__ void k_put_rows(StepRowChunk c, StepRow* __restrict__ dst, int count) { const int t = threadIdx.x; if (t < count) dst[t] = c.r[t]; }
// ... and stepped here, from their unchanged state, by the one-env code (a handful of persistent single-wave workgroups walk the list)
__global__ __launch_bounds__(64, DM_STEP_WAVES) void k_step_redo(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                  Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                  int n_substeps, int first, const int* __restrict__ redo_count, int* __restrict__ redo_count_next, dmp::PolicyArgs pa) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int n = dmw::uniform(*redo_count);
  // the two counters of a sub-batch alternate from step to step: this launch clears the one the NEXT packed launch will count into (its last
  // reader, the redo launch of the step before, finished before this step's packed launch began: stream order) — no memset between launches
  if (blockIdx.x == 0 && threadIdx.x == 0) *redo_count_next = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && n > 0) atomicAdd(B.redo_why, n);       // running total (dm_batch_redo_total)
  for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
    const int env = B.redo_list[first + i];
    env_step_impl<Real, NARROW_ROWS, false, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps);
    if (pa.P) { dmw::sync(); dmp::policy_wave(pa, env, dmw::lane(), &s.qpos[7], &s.qvel[6], reinterpret_cast<float*>(&s.u)); }
    dmw::sync_mem();
  }
}

// Dispatch order of a HORIZON launch (k_rollout_packed): environments with similar cost keys (env_step.h DM_ORDER_KEY: constraint rows + a quarter
// of the PGS sweeps of the last evaluation) share a wave — a wave pays for its largest row count and its slowest PGS.  Counting sort, descending;
// the order inside a bucket is arbitrary — results never depend on the dispatch order.  One launch per horizon: off the per-step path, where the
// step kernels order themselves (env_step.h dispatch_env / order_ticket; rounds 1-4 ran this kernel — or its one-wave form — between every two steps:
// 9 % of the GPU time of the one-launch-per-call form).
// (measured, round 4: DEALING the sorted list over the waves of a horizon launch — rank r to wave r % W, slot r / W, one environment of each
//  quartile per wave instead of the four heaviest together — shortens the slowest wave of a 64-step launch by 1.3 % and lengthens the
//  driver's 20-step window by 2 %: profiles/r04_ab_kernel_variants.md; the grouped order stays)
#ifndef DM_GROUP_KEY
#define DM_GROUP_KEY(nefc, iter) DM_ORDER_KEY(nefc, iter)
#endif
#ifndef DM_GROUP_BUCKETS
#define DM_GROUP_BUCKETS 64
#endif
DM_DEV int group_bucket(int nefc, int iter) { const int k = DM_GROUP_KEY(nefc, iter); return k < 0 ? 0 : (k > DM_GROUP_BUCKETS - 1 ? DM_GROUP_BUCKETS - 1 : k); }
__global__ __launch_bounds__(1024) void k_order(Batch<Real> B, int* __restrict__ order, int first, int count) {
  constexpr int NBK = DM_GROUP_BUCKETS;
  static_assert(NBK <= 1024, "one thread per bucket");
  __shared__ int hist[NBK], start[NBK];
  const int tid = threadIdx.x, n = count;                // envs first .. first + count - 1 are sorted into order[first ..]
  if (tid < NBK) hist[tid] = 0;
  __syncthreads();
  constexpr int PER = 8;                 // keys of up to 8192 envs stay in registers between the two passes
  int key[PER];
#pragma unroll
  for (int j = 0; j < PER; j++) {
    const int e = tid + j * 1024;
    key[j] = -1;
    if (e < n) { key[j] = group_bucket(B.nefc[first + e], B.solver_iter[first + e]); atomicAdd(&hist[key[j]], 1); }
  }
  for (int e = tid + PER * 1024; e < n; e += 1024) atomicAdd(&hist[group_bucket(B.nefc[first + e], B.solver_iter[first + e])], 1);
  __syncthreads();
  if (tid == 0) { int acc = 0; for (int k = NBK - 1; k >= 0; k--) { start[k] = acc; acc += hist[k]; } }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < PER; j++) if (key[j] >= 0) order[first + atomicAdd(&start[key[j]], 1)] = first + tid + j * 1024;
  for (int e = tid + PER * 1024; e < n; e += 1024) order[first + atomicAdd(&start[group_bucket(B.nefc[first + e], B.solver_iter[first + e])], 1)] = first + e;
}

// same step with per-stage shader-clock accounting (DM_OPT 101); not used on the timed path
__global__ __launch_bounds__(64) void k_step_prof(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
                                                  Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done,
                                                  int n_substeps, long long* prof) {
  __shared__ Shared<Real> s;
  __shared__ StepScratch<Real> x;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  env_step_impl<Real, MAXEFC, true, false>(*Mp, B, s, x, env, dmw::lane(), action, obs, reward, done, n_substeps, prof);
}

__global__ __launch_bounds__(64) void k_set_state(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ qpos,
                                                  const Ext* __restrict__ qvel, const int* __restrict__ frame_idx,
                                                  const unsigned char* __restrict__ mask) {
  __shared__ Shared<Real> s;
  const int env = blockIdx.x, lane = dmw::lane();
  if (env >= B.n_envs) return;
  if (mask && !mask[env]) return;
  load_env(*Mp, B, s, env, lane, (const Ext*)0);
  if (lane < NQ) s.qpos[lane] = (Real)qpos[(size_t)env * NQ + lane];
  if (lane < NV) s.qvel[lane] = (Real)qvel[(size_t)env * NV + lane];
  if (frame_idx && lane == 0) set_frame(B, env, frame_idx[env]);
  dmw::sync();
  store_state(B, s, env, lane);
  { const LaneTopo lt = lane_topo(lane); stage_tables(s, lane); dmw::sync(); forward(*Mp, s, lane, lt, (const DebugOut*)0); }   // sim.forward()
  store_derived(B, *Mp, s, env, lane);
}

__global__ __launch_bounds__(64) void k_reset(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, int mode, int hard,
                                              const unsigned char* __restrict__ mask) {
  __shared__ Shared<Real> s;
  const int env = blockIdx.x, lane = dmw::lane();
  if (env >= B.n_envs) return;
  if (mask && !mask[env]) return;
  load_env(*Mp, B, s, env, lane, (const Ext*)0);
  reset_env(*Mp, B, s, env, lane, mode, hard);
  store_state(B, s, env, lane);
  { const LaneTopo lt = lane_topo(lane); stage_tables(s, lane); dmw::sync(); forward(*Mp, s, lane, lt, (const DebugOut*)0); }
  store_derived(B, *Mp, s, env, lane);
}

__global__ void k_get_obs(Batch<Real> B, Ext* __restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B.n_envs * NOBS) return;
  const int env = i / NOBS, k = i % NOBS;
  obs[i] = k < 28 ? B.qpos[(size_t)env * NQ + 7 + k] : B.qvel[(size_t)env * NV + 6 + (k - 28)];   // (step_rules.h obs_element, restated: through it the kernel takes two more registers)
}

// field reads / writes of the float32 build: device state is `Real`, the C ABI speaks float64
__global__ void k_to_ext(const Real* __restrict__ src, Ext* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (Ext)src[i];
}
__global__ void k_from_ext(const Ext* __restrict__ src, Real* __restrict__ dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (Real)src[i];
}

__global__ __launch_bounds__(64) void k_debug_forward(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, int env, double* out) {
  __shared__ Shared<Real> s;
  const int lane = dmw::lane();
  load_env(*Mp, B, s, env, lane, (const Ext*)0);
  // actuator forces from the stored ctrl
  if (lane < NU) s.act[lane + 6] = act_force(*Mp, lane + 6, B.ctrl[(size_t)env * NU + lane]);
  dmw::sync();
  DebugOut dbg{out};
  { const LaneTopo lt = lane_topo(lane); stage_tables(s, lane); dmw::sync(); forward(*Mp, s, lane, lt, &dbg); }
  store_derived(B, *Mp, s, env, lane);
}

// ============================================ host side ====================================================
thread_local std::string g_err;

struct dm_model { DevModel<Real> h; double timestep64; /* the descriptor's, whatever the arithmetic type (a held push's impulse F h: push_kernel.h) */ };
// a clip of a clip set (dm_mocap_create_set): its rows in the concatenated tables, its own dt and imitation parameters 13..15, its draw cdf
struct ClipInfo { int row0, n_frames; double dt, loop, shift_x, shift_y, cdf; };
struct dm_mocap { std::vector<double> cfg, vel, imit_table, imit_params; int n_frames; double dt; std::vector<ClipInfo> clips; /* empty: a single clip */ };

extern "C" const char* dm_last_error(void) { return g_err.c_str(); }
extern "C" int dm_abi_version(void) { return DM_ABI_VERSION; }
extern "C" int dm_real_bits(void) { return (int)(8 * sizeof(Real)); }   /* 64: libdmenv.so, 32: libdmenv32.so */
extern "C" int dm_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

extern "C" int dm_model_create(const dm_model_desc* d, dm_model** out) {
  if (!d || !out) return fail(DM_EINVAL, "dm_model_create: null argument");
  dm_model* m = new (std::nothrow) dm_model();
  if (!m) return fail(DM_ENOMEM, "dm_model_create: out of memory");
  std::string err;
  const int rc = dm::build_dev_model(d, &m->h, &err);
  if (rc != DM_OK) { delete m; return fail(rc, err); }
  m->timestep64 = d->timestep;
  *out = m;
  return DM_OK;
}
extern "C" void dm_model_destroy(dm_model* m) { delete m; }

extern "C" int dm_mocap_create(const double* cfg, const double* vel, int32_t F, double dt, dm_mocap** out) {
  if (!cfg || !vel || F <= 0 || !out) return fail(DM_EINVAL, "dm_mocap_create: bad argument");
  dm_mocap* mc = new (std::nothrow) dm_mocap();
  if (!mc) return fail(DM_ENOMEM, "dm_mocap_create: out of memory");
  mc->cfg.assign(cfg, cfg + (size_t)F * NQ); mc->vel.assign(vel, vel + (size_t)F * NV); mc->n_frames = F; mc->dt = dt;
  *out = mc;
  return DM_OK;
}
extern "C" int dm_mocap_set_imitation(dm_mocap* mc, const double* table, int32_t n_cols, const double* params) {
  if (!mc || !table || !params) return fail(DM_EINVAL, "dm_mocap_set_imitation: null argument");
  if (n_cols != IMIT_FEAT) return fail(DM_EINVAL, "dm_mocap_set_imitation: a feature row has 112 columns");
  for (int e = 0; e < 4; e++) { const int b = (int)params[16 + e]; if (b < 1 || b >= NB) return fail(DM_EINVAL, "dm_mocap_set_imitation: end-effector body id out of range"); }
  mc->imit_table.assign(table, table + (size_t)mc->n_frames * IMIT_FEAT);
  mc->imit_params.assign(params, params + 32);
  return DM_OK;
}
extern "C" int dm_mocap_create_set(const dm_mocap* const* clips, int32_t K, const double* weights, dm_mocap** out) {
  if (!clips || !out || K < 1 || K > DM_MAX_CLIPS) return fail(DM_EINVAL, "dm_mocap_create_set: null argument, or n_clips outside 1..DM_MAX_CLIPS");
  double total = 0;
  for (int c = 0; c < K; c++) {
    if (!clips[c]) return fail(DM_EINVAL, "dm_mocap_create_set: null clip");
    if (!clips[c]->clips.empty()) return fail(DM_EINVAL, "dm_mocap_create_set: a clip of a set must be a single clip, not a set");
    if (clips[c]->imit_table.empty() != clips[0]->imit_table.empty()) return fail(DM_EINVAL, "dm_mocap_create_set: either every clip carries an imitation table or none does");
    if (!clips[c]->imit_table.empty())
      for (int k = 0; k < 32; k++)
        if ((k < 13 || k > 15) && clips[c]->imit_params[k] != clips[0]->imit_params[k]) return fail(DM_EINVAL, "dm_mocap_create_set: imitation parameters 0..12 and 16..31 must be equal across the set");
    const double w = weights ? weights[c] : 1.0;
    if (!(w >= 0) || !(w <= 1.7976931348623157e308)) return fail(DM_EINVAL, "dm_mocap_create_set: weights must be finite and >= 0");
    total += w;
  }
  if (!(total > 0) || !(total <= 1.7976931348623157e308)) return fail(DM_EINVAL, "dm_mocap_create_set: the weights must have a positive, finite sum");
  dm_mocap* mc = new (std::nothrow) dm_mocap();
  if (!mc) return fail(DM_ENOMEM, "dm_mocap_create_set: out of memory");
  mc->n_frames = 0; mc->dt = clips[0]->dt; mc->imit_params = clips[0]->imit_params;
  double run = 0;
  for (int c = 0; c < K; c++) {
    const dm_mocap* q = clips[c];
    run += weights ? weights[c] : 1.0;
    const bool im = !q->imit_table.empty();
    mc->clips.push_back(ClipInfo{mc->n_frames, q->n_frames, q->dt, im ? q->imit_params[15] : 0.0, im ? q->imit_params[13] : 0.0, im ? q->imit_params[14] : 0.0,
                                 c == K - 1 ? 1.0 : run / total});
    mc->cfg.insert(mc->cfg.end(), q->cfg.begin(), q->cfg.end()); mc->vel.insert(mc->vel.end(), q->vel.begin(), q->vel.end());
    mc->imit_table.insert(mc->imit_table.end(), q->imit_table.begin(), q->imit_table.end());
    mc->n_frames += q->n_frames;
  }
  if (K == 1) mc->clips.clear();      // a set of one clip IS that clip: n_frames, dt and the parameters above are its own
  *out = mc;
  return DM_OK;
}
extern "C" void dm_mocap_destroy(dm_mocap* mc) { delete mc; }

template <class T> static hipError_t dalloc(T** p, size_t n) { hipError_t e = hipMalloc((void**)p, n * sizeof(T)); if (e == hipSuccess) e = hipMemset(*p, 0, n * sizeof(T)); return e; }

extern "C" void dm_batch_destroy(dm_batch* b) {
  if (!b) return;
  hipSetDevice(b->device);
  b->queue.q.clear();    // queued steps are dropped, not run: their buffers belong to the caller and may be gone
  b->pipe.join(b->stream);
  if (b->stream) hipStreamSynchronize(b->stream);
  b->pipe.destroy(); b->trunc.release();
  void* ptrs[] = {b->d_model, b->B.qpos, b->B.qvel, b->B.qws, b->B.time, b->B.ctrl, b->B.xipos, b->B.comz, b->B.frame_idx, b->B.frame_init,
                  b->B.ncon, b->B.nefc, b->B.cong, b->B.status, b->B.solver_iter, b->B.episode, b->d_cfg, b->d_vel, b->d_action, b->d_obs,
                  b->d_mask, b->d_cvt, b->d_qpos_in, b->d_qvel_in, b->d_fidx_in, b->d_debug, b->d_prof, b->B.aovf, b->B.cycle, b->d_imit, b->d_order, b->B.kin, b->B.kin_ok, b->B.redo_list, b->B.redo_count, b->B.redo_why, b->d_B, b->queue.d_rows, b->ord.d_cnt, b->ord.d_list, b->d_rbuf, b->d_ep_steps, b->d_done_reason, b->d_clip, b->d_clip_rec, b->d_push_state, b->d_push_force};
  for (void* p : ptrs) if (p) hipFree(p);
  if (b->h_out) hipHostFree(b->h_out);
  if (b->h_action) hipHostFree(b->h_action);
  if (b->timing.ev0) hipEventDestroy(b->timing.ev0); if (b->timing.ev1) hipEventDestroy(b->timing.ev1);
  if (b->own_stream && b->stream) hipStreamDestroy(b->stream);
  delete b;
}

extern "C" int dm_batch_create(const dm_model* m, const dm_mocap* mc, int32_t n, int32_t device, uint32_t flags, dm_batch** out) {
  if (!m || !mc || n <= 0 || !out) return fail(DM_EINVAL, "dm_batch_create: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(DM_ENODEVICE, "dm_batch_create: no HIP device visible (libdmenv has no CPU path)");
  if (device < 0 || device >= ndev) return fail(DM_EINVAL, "dm_batch_create: bad device id");
  HIPCHK(hipSetDevice(device));
  dm_batch* b = new (std::nothrow) dm_batch();
  if (!b) return fail(DM_ENOMEM, "dm_batch_create: out of memory");
  b->n = n; b->device = device; b->timestep64 = m->timestep64;
  hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete b; return fail(DM_EHIP, "hipStreamCreate failed"); }
  b->own_stream = true;
  DevModel<Real> hm = m->h;
  hm.enable_contact = (flags & DM_FLAG_NO_CONTACT) ? 0 : 1;
  hm.enable_limit = (flags & DM_FLAG_NO_LIMIT) ? 0 : 1;
  b->has_rows = hm.enable_contact || hm.enable_limit;     // without rows every env costs the same: no reordering
  bool ok = true;
#define A(p, cnt) ok = ok && (dalloc(&(p), (size_t)(cnt)) == hipSuccess)
  A(b->d_model, 1); A(b->d_B, 1);
  A(b->B.qpos, (size_t)n * NQ); A(b->B.qvel, (size_t)n * NV); A(b->B.qws, (size_t)n * NV); A(b->B.time, n); A(b->B.ctrl, (size_t)n * NU);
  A(b->B.xipos, (size_t)n * NB * 3); A(b->B.comz, n); A(b->B.frame_idx, n); A(b->B.frame_init, n); A(b->B.ncon, n); A(b->B.nefc, n);
  A(b->B.cong, (size_t)n * MAXEFC * 2); A(b->B.status, n); A(b->B.solver_iter, n); A(b->B.episode, n); A(b->B.cycle, n); A(b->d_order, n);
  A(b->d_cfg, (size_t)mc->n_frames * NQ); A(b->d_vel, (size_t)mc->n_frames * NV);
  if (!mc->imit_table.empty()) A(b->d_imit, mc->imit_table.size() + 32);   // [32 parameters][F x 112 feature rows]
  A(b->d_action, (size_t)n * NU); A(b->d_mask, n);
  b->out_bytes = (size_t)n * (NOBS + 1) * sizeof(Ext) + (size_t)n;
  { unsigned char* blk = nullptr; ok = ok && (dalloc(&blk, b->out_bytes) == hipSuccess);
    b->d_obs = (Ext*)blk; b->d_reward = b->d_obs + (size_t)n * NOBS; b->d_done = (unsigned char*)(b->d_reward + n); }
  ok = ok && hipHostMalloc((void**)&b->h_out, b->out_bytes, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&b->h_action, (size_t)n * NU * sizeof(Ext), hipHostMallocDefault) == hipSuccess;
  A(b->B.aovf, (size_t)n * AOVF_COLS * 64);
  A(b->B.kin, (size_t)n * KIN_DOUBLES); A(b->B.kin_ok, n);
  A(b->B.redo_list, n); A(b->B.redo_count, 2 * DM_MAX_PIPELINE); A(b->B.redo_why, 8);
  A(b->ord.d_cnt, DM_MAX_PIPELINE * 3 * ORD_BUCKETS);
  A(b->ord.d_list, (size_t)3 * ORD_BUCKETS * n);                      // (768 B per env of address space, 8 B of it touched per step; allocated here so that no step call can run out of memory half-way through its parts)
  A(b->d_ep_steps, n); A(b->d_done_reason, n);
  A(b->d_qpos_in, (size_t)n * NQ); A(b->d_qvel_in, (size_t)n * NV); A(b->d_fidx_in, n); A(b->d_debug, DM_DEBUG_DOUBLES);
  if (sizeof(Real) != sizeof(Ext)) A(b->d_cvt, (size_t)n * NB * 3);   // largest Real field per env: xipos (42)
  A(b->d_clip, n);                                                    // DM_F_CLIP and the clip records: the last allocations, so that a single-clip batch's other arrays lie where they always lay
  if (!mc->clips.empty()) A(b->d_clip_rec, mc->clips.size());
  A(b->d_push_state, (size_t)n * 5); A(b->d_push_force, (size_t)n * 3);   // DM_F_PUSH_STATE, DM_F_PUSH_FORCE (after every older allocation, like the clip arrays)
#undef A
  if (!ok) { dm_batch_destroy(b); return fail(DM_ENOMEM, "dm_batch_create: hipMalloc failed"); }
  ok = hipMemcpy(b->d_model, &hm, sizeof hm, hipMemcpyHostToDevice) == hipSuccess;
  auto upload = [](Real* dst, const double* src, size_t cnt) {      // host float64 table -> device `Real` array
    std::vector<Real> tmp(src, src + cnt);
    return hipMemcpy(dst, tmp.data(), cnt * sizeof(Real), hipMemcpyHostToDevice) == hipSuccess;
  };
  ok = ok && upload(b->d_cfg, mc->cfg.data(), mc->cfg.size());
  ok = ok && upload(b->d_vel, mc->vel.data(), mc->vel.size());
  if (b->d_imit) {
    ok = ok && upload(b->d_imit, mc->imit_params.data(), 32);
    ok = ok && upload(b->d_imit + 32, mc->imit_table.data(), mc->imit_table.size());
    for (int k = 0; k < 32; k++) b->B.imit_params[k] = mc->imit_params[k];
  }
  b->B.imit_pdev = b->d_imit;
  b->B.imit_table = b->d_imit ? b->d_imit + 32 : nullptr;
  if (!mc->clips.empty()) {             // the clip set: records, and the default assignment (global env) % K
    b->n_clips = (int)mc->clips.size();
    std::vector<ClipRec<Real>> rec;
    for (const ClipInfo& c : mc->clips) { rec.push_back(ClipRec<Real>{c.row0, c.n_frames, (Real)c.dt, (Real)c.loop, (Real)c.shift_x, (Real)c.shift_y, c.cdf}); b->clip_frames.push_back(c.n_frames); }
    std::vector<int> ids((size_t)n);
    for (int e2 = 0; e2 < n; e2++) ids[e2] = e2 % b->n_clips;
    ok = ok && hipMemcpy(b->d_clip_rec, rec.data(), rec.size() * sizeof(ClipRec<Real>), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(b->d_clip, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  } else b->clip_frames.push_back(mc->n_frames);
  // initial state = MjSim(model): qpos0, zero velocity
  std::vector<Real> q0((size_t)n * NQ);
  for (int e2 = 0; e2 < n; e2++) for (int k = 0; k < NQ; k++) q0[(size_t)e2 * NQ + k] = hm.qpos0[k];
  ok = ok && hipMemcpy(b->B.qpos, q0.data(), q0.size() * sizeof(Real), hipMemcpyHostToDevice) == hipSuccess;
  { std::vector<int> ps((size_t)n * 5, 0); for (int e2 = 0; e2 < n; e2++) ps[(size_t)e2 * 5] = -1;       // DM_F_PUSH_STATE: no episode seen yet
    ok = ok && hipMemcpy(b->d_push_state, ps.data(), ps.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess; }
  if (!ok) { dm_batch_destroy(b); return fail(DM_EHIP, "dm_batch_create: upload failed"); }
  b->B.mocap_cfg = b->d_cfg; b->B.mocap_vel = b->d_vel; b->B.mocap_dt = mc->dt; b->B.n_frames = mc->n_frames; b->B.n_envs = n; b->B.env_offset = 0;
  b->B.reward_mode = 0; b->B.autoreset = 0; b->B.action_mode = 0; b->B.seed = 0; b->B.diag = 1;
  hipEventCreate(&b->timing.ev0); hipEventCreate(&b->timing.ev1);
  { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) == hipSuccess && cus > 0) b->resident_waves = cus * 4 * DM_STEP_WAVES; }
  *out = b;
  return DM_OK;
}

extern "C" int dm_batch_set_stream(dm_batch* b, void* s) {
  if (!b) return fail(DM_EINVAL, "null batch");
  if (settle(b)) return fail(DM_EHIP, "dm_batch_set_stream: flushing the step queue failed");
  hipStreamSynchronize(b->stream);   /* keep ordering with work already queued on the previous stream */
  if (b->own_stream && b->stream) hipStreamDestroy(b->stream);
  b->stream = (hipStream_t)s; b->own_stream = false;
  return DM_OK;
}

extern "C" int dm_batch_set_option(dm_batch* b, int32_t opt, int64_t v) {
  if (!b) return fail(DM_EINVAL, "null batch");
  if (!b->queue.q.empty()) { HIPCHK(hipSetDevice(b->device)); const int rc = flush_queue(b); if (rc != DM_OK) return rc; }   /* queued steps ran under the old options */
  switch (opt) {
    case DM_OPT_STEP_QUEUE:
      if (v < 0 || v > DM_MAX_STEP_QUEUE) return fail(DM_EINVAL, "step queue depth must be 0..DM_MAX_STEP_QUEUE");
      b->queue.cap = (int)v; break;
    case DM_OPT_REWARD_MODE:
      if (v < 0 || v > 4) return fail(DM_EINVAL, "reward mode must be 0..4");
      if (v >= 3 && !b->d_imit) return fail(DM_EINVAL, "reward modes 3 and 4 need dm_mocap_set_imitation() before dm_batch_create()");
      b->B.reward_mode = (int)v; break;
    case DM_OPT_AUTORESET: if (v < 0 || v > 2) return fail(DM_EINVAL, "autoreset must be 0..2"); b->B.autoreset = (int)v; break;
    case DM_OPT_ACTION_MODE: if (v < 0 || v > 4) return fail(DM_EINVAL, "action mode must be 0..4"); b->B.action_mode = (int)v; break;
    case DM_OPT_SEED: b->B.seed = (unsigned long long)v; break;
    case DM_OPT_DIAGNOSTICS: b->B.diag = v != 0; break;
    case DM_OPT_FALL_BODIES:
      if (v < 0 || (v & ~(int64_t)0x3ffe)) return fail(DM_EINVAL, "DM_OPT_FALL_BODIES: a mask over model bodies 1..13 (bits 1..13)");
      b->fall_bodies = (unsigned)v; break;
    case DM_OPT_MAX_EPISODE_STEPS:
      if (v < 0 || v > 0x7fffffff) return fail(DM_EINVAL, "DM_OPT_MAX_EPISODE_STEPS must be 0 (off) or a positive step count");
      b->max_episode_steps = (int)v; break;
    case DM_OPT_TRUNCATION_LOG:
      if (v < 0 || v > 0x7fffffff) return fail(DM_EINVAL, "DM_OPT_TRUNCATION_LOG must be 0 (off) or a capacity in records");
      HIPCHK(hipSetDevice(b->device));
      if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
      HIPCHK(hipStreamSynchronize(b->stream));       /* (a termination launch still appending to the old log) */
      if (const int rc = b->trunc.resize((int)v, b->stream)) return rc;
      break;
    case DM_OPT_HORIZON_TERMINATION:
      if (v != 0 && v != 1) return fail(DM_EINVAL, "DM_OPT_HORIZON_TERMINATION must be 0 or 1");
      b->horizon_term = v != 0; break;
    case DM_OPT_HORIZON_SPD:
      if (v != 0 && v != 1) return fail(DM_EINVAL, "DM_OPT_HORIZON_SPD must be 0 or 1");
      b->horizon_spd = v != 0; break;
    case DM_OPT_CLIP_MODE:
      if (v != 0 && v != 1) return fail(DM_EINVAL, "DM_OPT_CLIP_MODE must be 0 (fixed) or 1 (episode)");
      b->clip_mode = (int)v; break;
    case DM_OPT_PIPELINE:
      if (v < 1 || v > DM_MAX_PIPELINE) return fail(DM_EINVAL, "pipeline depth must be 1..DM_MAX_PIPELINE");
      HIPCHK(hipSetDevice(b->device));
      if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
      if (const int rc = set_pipeline(b, (int)v)) return rc;
      break;
    case 106: b->horizon_mode = v < 0 ? -1 : (v != 0 ? 1 : 0); break;   /* dm_batch_rollout on the packed path: 1 one launch per horizon, 0 step launches, -1 (default) by batch size */
    case DM_OPT_PACKED: case 105:                                   /* 1: four environments per wavefront (k_step_packed) where it covers the configuration; 2: the same, per-step launches with the three-set code */
      if (v < 0 || v > 2) return fail(DM_EINVAL, "DM_OPT_PACKED must be 0, 1 or 2");
      b->packed = v != 0; b->packed_ext = v == 2; break;
    case 104: b->reorder = v != 0; if (!b->reorder) b->B.order = nullptr; break;   /* 1 (default): longest-first dispatch order (k_order) */
    case 100:                                   /* global id of env 0 (multi-GPU sharding); a multi-clip batch's default assignment follows it */
      b->B.env_offset = (int)v;
      if (multi_clip(b)) {
        HIPCHK(hipSetDevice(b->device));
        if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
        std::vector<int> ids((size_t)b->n);
        for (int e = 0; e < b->n; e++) ids[e] = (int)(((long long)v + e) % b->n_clips + b->n_clips) % b->n_clips;
        HIPCHK(hipMemcpyAsync(b->d_clip, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
      }
      break;
    case 102: b->two_tier = v != 0; break;       /* 1 (default): register tier of NARROW_ROWS columns + overflow strip; 0: all 64 columns in registers */
    case 103: {                                 /* test hook: 1 = every PGS sweep takes the guarded-replay path (results must not change) */
      const Real lvl = v ? Real(-1e300) : Real(1e-10);
      HIPCHK(hipMemcpyAsync((char*)b->d_model + offsetof(DevModel<Real>, pgs_detect), &lvl, sizeof lvl, hipMemcpyHostToDevice, b->stream));
      HIPCHK(hipStreamSynchronize(b->stream));
      break;
    }
    case 101:                                   /* per-stage cycle profile on/off (diagnostic) */
      b->prof = v != 0;
      if (b->prof && !b->d_prof) { if (hipMalloc((void**)&b->d_prof, (size_t)b->n * dm::PROF_SLOTS * sizeof(long long)) != hipSuccess) return fail(DM_ENOMEM, "prof alloc"); }
      break;
    default: return fail(DM_EINVAL, "unknown option");
  }
  return DM_OK;
}

extern "C" int dm_batch_set_state(dm_batch* b, const double* qpos, const double* qvel, const int32_t* fidx, const uint8_t* mask, int32_t kind) {
  if (!b || !qpos || !qvel) return fail(DM_EINVAL, "dm_batch_set_state: null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const void *q, *v, *f, *mk; int rc;
  if (multi_clip(b) && fidx && kind == DM_PTR_HOST) {       // a frame is local to the env's clip
    std::vector<int> ids;
    if ((rc = clip_ids_host(b, ids))) return rc;
    for (int e = 0; e < b->n; e++)
      if ((!mask || mask[e]) && (fidx[e] < 0 || fidx[e] >= b->clip_frames[ids[e]])) return fail(DM_EINVAL, "dm_batch_set_state: frame_idx outside the env's clip");
  }
  if ((rc = stage_in(b, b->d_qpos_in, qpos, (size_t)b->n * NQ * 8, kind, &q))) return rc;
  if ((rc = stage_in(b, b->d_qvel_in, qvel, (size_t)b->n * NV * 8, kind, &v))) return rc;
  if ((rc = stage_in(b, b->d_fidx_in, fidx, (size_t)b->n * 4, kind, &f))) return rc;
  if ((rc = stage_in(b, b->d_mask, mask, (size_t)b->n, kind, &mk))) return rc;
  HIPCHK(hipMemsetAsync(b->B.kin_ok, 0, (size_t)b->n, b->stream));          // parked kinematics belong to the old states
  hipLaunchKernelGGL(k_set_state, dim3(b->n), dim3(64), 0, b->stream, b->d_model, b->B, (const Ext*)q, (const Ext*)v, (const int*)f, (const unsigned char*)mk);
  HIPCHK(hipGetLastError());
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}

extern "C" int dm_batch_reset(dm_batch* b, int32_t mode, int32_t hard, const uint8_t* mask, int32_t kind) {
  if (!b || mode < 0 || mode > 2) return fail(DM_EINVAL, "dm_batch_reset: bad argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const void* mk; int rc;
  if ((rc = stage_in(b, b->d_mask, mask, (size_t)b->n, kind, &mk))) return rc;
  HIPCHK(hipMemsetAsync(b->B.kin_ok, 0, (size_t)b->n, b->stream));
  launch_clip_or_plain(b, k_reset, k_reset_clips, dim3(b->n), dim3(64), b->stream, b->d_model, b->B, (int)mode, (int)hard, (const unsigned char*)mk);
  hipLaunchKernelGGL(k_zero_masked, dim3((b->n + 255) / 256), dim3(256), 0, b->stream, b->d_ep_steps, (const unsigned char*)mk, b->n);   // DM_F_EPISODE_STEPS
  HIPCHK(hipGetLastError());
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}

// the packed path covers this batch's configuration (reward modes alive / v3-config / v2-pose / imitation, the two-tier kernel family)
// early termination is on: k_terminate follows every per-step launch; the horizon launch and the step queue carry no termination code, unless
// DM_OPT_HORIZON_TERMINATION asks for the horizon kernel that does (k_rollout_packed_term)
static bool term_on(const dm_batch* b) { return b->fall_bodies != 0u || b->max_episode_steps > 0; }
static bool packed_covers(const dm_batch* b) { return b->packed && b->B.reward_mode <= 4 && b->two_tier; }
// a dm_batch_step call may be queued: device pointers, no fused policy step, no per-stage profiling, and a configuration for which ONE launch
// per horizon is the faster form (rollout_as_one_launch)
static bool rollout_as_one_launch(const dm_batch* b) {
  // ONE launch for the horizon where that wins (measured, profiles/r03_bench_*): batches with constraint rows of up to two packed waves per
  // SIMD (8 192 envs on an MI355X; at 4 096 envs 17.3 M env-steps/s against 12.2 M for the one-env steps and 11.4 M for the packed ones).
  // Larger batches run several rounds of waves per step, which balances the slow waves by itself, while a horizon launch has its own
  // end-of-horizon tail (16 384 envs: 19.5 M per step, ~17 M per horizon); without rows there is no slow wave to wait for.
  // (action modes 3 and 4 — a control evaluation per substep — run their horizons and queued steps as step launches, unless DM_OPT_HORIZON_SPD asks for the
  //  horizon kernels that carry the controller; so do those of a batch with early termination on, unless DM_OPT_HORIZON_TERMINATION is set; those of a
  //  multi-clip batch, with or without either; and those of a batch with a push schedule set, whose k_push precedes every step launch)
  const int simds = b->resident_waves / DM_STEP_WAVES;
  return packed_covers(b) && !multi_clip(b) && !push_on(b) && (b->B.action_mode <= 2 || b->horizon_spd) && (!term_on(b) || b->horizon_term) && (b->horizon_mode == 1 || (b->horizon_mode < 0 && b->has_rows && b->n <= 2 * SLOTS * simds));
}
static bool can_queue(const dm_batch* b, int kind, const dmp::PolicyArgs* pol) {
  return kind == DM_PTR_DEVICE && !pol && !b->prof && rollout_as_one_launch(b);      // (with timing on, the events bracket the horizon launch)
}
// the termination arguments of the part [lo, lo + count) for a launch whose first step has the truncation log's tick `first_tick`
static TermArgs term_args(const dm_batch* b, int lo, int count, int first_tick) {
  return TermArgs{b->d_ep_steps, b->d_done_reason, b->fall_bodies, b->max_episode_steps, lo, count,
                  b->trunc.d_count, b->trunc.d_index, b->trunc.d_qpos, b->trunc.d_qvel, b->trunc.cap, first_tick};
}
// the push schedule's arguments for the part [lo, lo + count) ahead of a step of nsub substeps
static PushArgs push_args(const dm_batch* b, int nsub, int lo, int count) {
  const dm_push_desc& d = b->push;
  return PushArgs{b->d_push_state, b->d_push_force, d.bodies, d.wait_min, d.wait_max, d.duration_min, d.duration_max, d.force_min, d.force_max, d.z_min, d.z_max,
                  b->timestep64 * (double)nsub, lo, count};
}
// T steps of every environment in ONE launch (k_rollout_packed) on the batch's stream; b->queue.d_rows[0 .. T) has been written on that stream.
// With early termination on (rollout_as_one_launch: DM_OPT_HORIZON_TERMINATION then) the launch is k_rollout_packed_term, whose steps count as T
// step calls on the truncation log's clock: step t's records carry the tick a dm_batch_step call in its place would have had.
static const dmp::PolicyArgs NOPOL{nullptr, nullptr, nullptr, 0, 0ull, 0ull};      // no policy step
// THE horizon kernels, one row per controller: action modes 0..2 (kernels_rollout.hip, kernels_rollout_term.hip) and modes 3 and 4 (kernels_rollout_spd.hip; reached
// only with DM_OPT_HORIZON_SPD: rollout_as_one_launch); one column per termination form: none, or the phase inside the loop (the trailing TermArgs)
struct HorizonKernels { decltype(&k_rollout_packed) plain; decltype(&k_rollout_packed_term) term; };
static const HorizonKernels& horizon_kernels(const dm_batch* b) {
  static const HorizonKernels K[2] = {{k_rollout_packed, k_rollout_packed_term}, {k_rollout_packed_spd, k_rollout_packed_term_spd}};
  return K[b->B.action_mode >= 3 ? 1 : 0];
}
static int launch_horizon(dm_batch* b, int T, int nsub, const dmp::PolicyArgs& pa) {
  hipLaunchKernelGGL(k_put_batch, dim3(1), dim3(64), 0, b->stream, b->B, b->d_B);
  if (const int rc = b->timing.start(b->stream)) return rc;
  long long* const clk = b->prof ? b->d_prof : (long long*)nullptr;
  const HorizonKernels& K = horizon_kernels(b);
  if (term_on(b))
    hipLaunchKernelGGL(K.term, dim3((b->n + SLOTS - 1) / SLOTS), dim3(64), 0, b->stream, b->d_model, (const Batch<Real>*)b->d_B, (const StepRow*)b->queue.d_rows, (int)nsub, 0, b->n, (int)T, pa, clk, term_args(b, 0, b->n, b->trunc.take_ticks(T)));
  else
    hipLaunchKernelGGL(K.plain, dim3((b->n + SLOTS - 1) / SLOTS), dim3(64), 0, b->stream, b->d_model, (const Batch<Real>*)b->d_B, (const StepRow*)b->queue.d_rows, (int)nsub, 0, b->n, (int)T, pa, clk);
  if (const int rc = b->timing.stop(b->stream)) return rc;
  // dispatch order for the next launch: environments with similar row counts share a wave (and, for per-step launches, longest first)
  if (b->reorder && b->has_rows) {
    for (int h = 0; h < b->pipe.depth; h++) {
      const Pipeline::Part p = b->pipe.part(b->n, h);
      if (p.count > 0) hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, b->stream, b->B, b->d_order, p.lo, p.count);
    }
    b->B.order = b->d_order;
  }
  HIPCHK(hipGetLastError()); return DM_OK;
}
void StepQueue::upload(hipStream_t stream) {
  const int T = (int)q.size();
  for (int t0 = 0; t0 < T; t0 += ROW_CHUNK) {
    StepRowChunk c;
    const int cnt = T - t0 < ROW_CHUNK ? T - t0 : ROW_CHUNK;
    for (int k = 0; k < cnt; k++) c.r[k] = q[t0 + k];
    for (int k = cnt; k < ROW_CHUNK; k++) c.r[k] = StepRow{nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(k_put_rows, dim3(1), dim3(ROW_CHUNK), 0, stream, c, d_rows + t0, cnt);
  }
  q.clear(); flushes += 1; steps += T;                 // (cleared before the horizon launch: an error there must not leave the steps queued for a second run)
}
int flush_queue(dm_batch* b) {
  const int T = (int)b->queue.q.size(); if (T == 0) return DM_OK;
  HIPCHK(hipSetDevice(b->device));
  if (b->pipe.join(b->stream)) return fail(DM_EHIP, "pipeline join failed");
  if (const int rc = b->queue.ensure_rows(T, b->stream)) return rc;
  b->queue.upload(b->stream);
  return launch_horizon(b, T, b->queue.nsub, NOPOL);
}

// the bytes of a dm_batch_step call's buffers overlap the bytes of ANY buffer of a queued call, in whatever role: the same tensors step after step, a view that
// starts elsewhere in one of them, a queued call's observations handed in as this call's action
static bool overlaps_queued(const dm_batch* b, const double* action, const double* obs, const double* reward, const uint8_t* done) {
  const size_t n = (size_t)b->n;
  const char* p[4] = {(const char*)action, (const char*)obs, (const char*)reward, (const char*)done};
  const size_t len[4] = {n * NU * sizeof(Ext), n * NOBS * sizeof(Ext), n * sizeof(Ext), n};
  for (const StepRow& r : b->queue.q) {
    const char* qp[4] = {(const char*)r.action, (const char*)r.obs, (const char*)r.reward, (const char*)r.done};
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) if (p[i] < qp[j] + len[j] && qp[j] < p[i] + len[i]) return true;
  }
  return false;
}

// the kernels of a step call: action modes 3 and 4 have their own instantiations (kernels_spd.hip, kernels_packed_spd.hip), DM_OPT_PACKED = 2 the packed
// kernels with the three-set code; every one is launched exactly like its counterpart
struct StepKernels {
  static constexpr bool has_prof = true; decltype(&k_step_packed) packed; decltype(&k_step_packed_act) packed_act; decltype(&k_step_packed_prof) packed_prof;
  decltype(&k_step_redo) redo; decltype(&k_step_narrow) narrow; decltype(&k_step_act) act; decltype(&k_step) single; decltype(&k_step_prof) prof;
};
// ... and a multi-clip batch's (kernels_clips.hip, kernels_packed_clips.hip): the same launches with the clip argument last; one set for every action mode
// (they pick the controller at run time), none with per-stage profiling (step_impl refuses that combination before anything is launched)
struct ClipStepKernels {
  static constexpr bool has_prof = false; decltype(&k_step_packed_clips) packed; decltype(&k_step_packed_act_clips) packed_act; decltype(&k_step_redo_clips) redo; decltype(&k_step_narrow_clips) narrow;
  decltype(&k_step_act_clips) act; decltype(&k_step_clips) single;
};
static ClipStepKernels clip_step_kernels(bool ext) {
  return {ext ? k_step_packed_ext_clips : k_step_packed_clips, ext ? k_step_packed_act_ext_clips : k_step_packed_act_clips, k_step_redo_clips, k_step_narrow_clips, k_step_act_clips, k_step_clips};
}
// which of a table's kernels steps a part: four envs per wave (or that profiled), the two-tier one-env kernel (narrow / act), all 64 columns in registers (option 102 = 0), that profiled (101)
enum StepSelect { SEL_PACKED, SEL_PACKED_PROF, SEL_NARROW, SEL_SINGLE, SEL_PROF };
// what the launches of one step call share: the buffers (the caller's, or a host-pointer step's staging block), the substep count, the select, the truncation log's tick
struct StepCall { const Ext* a; Ext* o; Ext* r; unsigned char* dn; int nsub; StepSelect sel; int tick; };
// THE per-step launch sequence, the only place one goes out from: the launches of one part [lo, lo + count) of the batch (a pipelined sub-batch, or the whole
// batch) on stream `st` with the descriptor Bp, over the kernel table K and its trailing arguments (none, or the clip argument).
//   push       the schedule's launch ahead of the part's step launches (k_push: push_kernel.h); off: nothing is launched
//   step       `pa`: a fused policy step (the act kernels), or null.  Packed: the kernel counts the environments beyond its capacities into redo.count, the
//              redo launch steps them one per wave and clears redo.next for the next call (RedoCounters)
//   terminate  early termination on: k_terminate on the same stream (a fused policy step would act on the observation of an episode it may still end: step_impl passes no `pa` then)
template <class Table, class... Tail>
static void launch_part(const dm_batch* b, const Table& K, const StepCall& c, hipStream_t st, const Batch<Real>& Bp, int lo, int count, RedoCounters::Pair redo, const dmp::PolicyArgs* pa, Tail... tail) {
  constexpr int REDO_BLOCKS = 1024;     // (round 5: 64 persistent one-wave workgroups took 5 ms to walk the 1 100 overflows a standing population of 8 192 envs produces per step on the lean kernel; an empty launch of 1 024 costs the same few microseconds)
  const dim3 envs(count), slots((count + SLOTS - 1) / SLOTS), wave(64);
  if (push_on(b)) hipLaunchKernelGGL(k_push, envs, wave, 0, st, b->d_model, Bp, push_args(b, c.nsub, lo, count));
  switch (c.sel) {
    case SEL_PACKED_PROF: if constexpr (Table::has_prof) hipLaunchKernelGGL(K.packed_prof, slots, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, count, redo.count, b->d_prof); break;
    case SEL_PACKED:
      if (pa) hipLaunchKernelGGL(K.packed_act, slots, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, count, redo.count, *pa, tail...);
      else hipLaunchKernelGGL(K.packed, slots, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, count, redo.count, tail...);
      break;
    case SEL_NARROW:
      if (pa) hipLaunchKernelGGL(K.act, envs, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, count, *pa, tail...);
      else hipLaunchKernelGGL(K.narrow, envs, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, count, tail...);
      break;
    case SEL_SINGLE: hipLaunchKernelGGL(K.single, envs, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, tail...); break;      // (the whole batch: these two kernels take no part)
    case SEL_PROF: if constexpr (Table::has_prof) hipLaunchKernelGGL(K.prof, envs, wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, b->d_prof); break;
  }
  if ((c.sel == SEL_PACKED || c.sel == SEL_PACKED_PROF) && b->has_rows)
    hipLaunchKernelGGL(K.redo, dim3(REDO_BLOCKS), wave, 0, st, b->d_model, Bp, c.a, c.o, c.r, c.dn, c.nsub, lo, (const int*)redo.count, redo.next, pa ? *pa : NOPOL, tail...);
  if (term_on(b)) launch_clip_or_plain(b, k_terminate, k_terminate_clips, envs, wave, st, b->d_model, Bp, term_args(b, lo, count, c.tick), c.o, c.dn);
}
static StepKernels step_kernels(bool spd, bool ext) {
  if (spd) return {ext ? k_step_packed_ext_spd : k_step_packed_spd, ext ? k_step_packed_act_ext_spd : k_step_packed_act_spd, k_step_packed_prof_spd,
                   k_step_redo_spd, k_step_narrow_spd, k_step_act_spd, k_step_spd, k_step_prof_spd};
  return {ext ? k_step_packed_ext : k_step_packed, ext ? k_step_packed_act_ext : k_step_packed_act, k_step_packed_prof,
          k_step_redo, k_step_narrow, k_step_act, k_step, k_step_prof};
}

static int step_impl(dm_batch* b, const double* action, double* obs, double* reward, uint8_t* done, int32_t nsub, int32_t kind, const dmp::PolicyArgs* pol) {
  if (!b || !action || !obs || !reward || !done || nsub < 1) return fail(DM_EINVAL, "dm_batch_step: bad argument");
  if (pol && (kind != DM_PTR_DEVICE || b->prof || !b->two_tier)) return fail(DM_EINVAL, "dm_batch_step_act: device pointers, the two-tier kernel and no profiling");
  if (b->prof && multi_clip(b)) return fail(DM_EUNSUPPORTED, "dm_batch_step: the profiling kernels (option 101) do not cover a multi-clip batch");
  HIPCHK(hipSetDevice(b->device));
  StepQueue& Q = b->queue;
  if (Q.cap > 0 && can_queue(b, kind, pol)) {
    // DM_OPT_STEP_QUEUE: remember the call; the queued steps run as ONE horizon launch (flush_queue).  A call that names a buffer an
    // earlier queued call names (the same action / output tensors step after step) runs that earlier call first: a caller that reuses
    // buffers has, by the pipelined contract, joined in between and sees plain step-by-step behaviour.
    const bool reuse = (nsub != Q.nsub && !Q.q.empty()) || overlaps_queued(b, action, obs, reward, done);
    if (reuse || (int)Q.q.size() >= Q.cap) { const int rc = flush_queue(b); if (rc != DM_OK) return rc; }
    Q.q.push_back(StepRow{action, obs, reward, done}); Q.nsub = nsub; return DM_OK;
  }
  if (!Q.q.empty()) { const int rc = flush_queue(b); if (rc != DM_OK) return rc; }
  const Ext* a = action;
  if (kind == DM_PTR_HOST) {
    memcpy(b->h_action, action, (size_t)b->n * NU * sizeof(Ext));
    HIPCHK(hipMemcpyAsync(b->d_action, b->h_action, (size_t)b->n * NU * sizeof(Ext), hipMemcpyHostToDevice, b->stream));
    a = b->d_action;
  }
  const bool dev = kind == DM_PTR_DEVICE;      // outputs: the caller's tensors, or the staging block
  Pipeline& P = b->pipe;
  const bool piped = P.depth > 1 && kind == DM_PTR_DEVICE && !b->prof && b->two_tier;
  if (!piped && P.join(b->stream)) return fail(DM_EHIP, "pipeline join failed");
  int rc = DM_OK; b->timing.collect();
  if (!piped && (rc = b->timing.start(b->stream)) != DM_OK) return rc;
  const bool reorder = b->reorder && b->has_rows && b->n > b->resident_waves;   // more envs than resident waves: later rounds exist, their tail matters
  const bool packed = packed_covers(b);      // this call runs on the packed kernels (profiled or not)
  const bool term = term_on(b);
  const StepCall c{a, dev ? obs : b->d_obs, dev ? reward : b->d_reward, dev ? done : b->d_done, (int)nsub, packed ? (b->prof ? SEL_PACKED_PROF : SEL_PACKED) : b->prof ? SEL_PROF : b->two_tier ? SEL_NARROW : SEL_SINGLE, b->trunc.take_ticks(1)};
  const dmp::PolicyArgs* fused = term ? nullptr : pol;      // (launch_part: with termination on the policy runs behind it, below)
  if (packed && (rc = b->redo.begin_step(piped, b->B.redo_count, P, b->stream)) != DM_OK) return rc;
  // part h of this call through THE launch sequence, over the plain table or — the third axis — a multi-clip batch's, with the clip argument last
  auto part = [&](hipStream_t st, const Batch<Real>& Bp, Pipeline::Part p, int h) {
    const RedoCounters::Pair redo = b->redo.pair(b->B.redo_count, h);
    if (multi_clip(b)) launch_part(b, clip_step_kernels(b->packed_ext), c, st, Bp, p.lo, p.count, redo, fused, clip_args(b));
    else launch_part(b, step_kernels(b->B.action_mode >= 3, b->packed_ext), c, st, Bp, p.lo, p.count, redo, fused);
  };
  unsigned ord_bound = 0;               // parts whose launch of this call took a ticket descriptor (committed below, after the launches went out)
  if (piped) {
    // Sub-batch h's launch of THIS call depends on its own launch of the previous call (stream order on ps[h]) and on the
    // caller's inputs (ev_in), not on the other sub-batches: while the last, cheap workgroups of one sub-batch drain, the
    // next sub-batch's fill the freed wave slots, across calls.  Nothing is inserted into the caller's stream here — it joins
    // (dm_batch_join, or any other entry point) when it needs the outputs.
    HIPCHK(hipEventRecord(P.ev_in, b->stream));
    for (int h = 0; h < P.depth; h++) {
      const Pipeline::Part p = P.part(b->n, h);
      if (p.count <= 0) continue;
      HIPCHK(hipStreamWaitEvent(P.ps[h], P.ev_in, 0));
      Batch<Real> Bh = b->B;                                                   // this part's launch orders itself from the tickets its previous launch left
      if (reorder) { if ((rc = b->ord.bind(Bh, b->n, h, p.lo, P.ps[h])) != DM_OK) return rc; ord_bound |= 1u << h; }
      if (h == 0 && (rc = b->timing.start(P.ps[0])) != DM_OK) return rc;     // timing: sub-batch 0's kernel on ITS stream
      part(P.ps[h], Bh, p, h);
      if (h == 0 && (rc = b->timing.stop(P.ps[0])) != DM_OK) return rc;
      HIPCHK(hipEventRecord(P.ev_done[h], P.ps[h]));
    }
    P.pending = true;
  } else {
    // (one launch over the whole batch.  With a pipeline depth configured the tickets are kept per part — a pipelined launch must find exactly its
    //  part's envs in them, otherwise two streams could step one env at once — so this launch takes none and falls back to the stored order: DM_OPT 104
    //  has no effect on host-pointer steps and other unpipelined launches of a batch whose DM_OPT_PIPELINE is above 1 — a performance matter only,
    //  results do not depend on the dispatch order; include/dmenv.h says so.  The profiled and the single-tier kernels take no tickets either.)
    if (c.sel == SEL_PACKED_PROF) HIPCHK(hipMemsetAsync(b->d_prof, 0, (size_t)b->n * dm::PROF_SLOTS * sizeof(long long), b->stream));
    Batch<Real> Bh = b->B;
    if (reorder && P.depth <= 1 && !b->prof && b->two_tier) { if ((rc = b->ord.bind(Bh, b->n, 0, 0, b->stream)) != DM_OK) return rc; ord_bound |= 1u; }
    part(b->stream, Bh, Pipeline::Part{0, b->n}, 0);
  }
  HIPCHK(hipGetLastError());
  for (int h = 0; h < DM_MAX_PIPELINE; h++) if ((ord_bound >> h) & 1u) b->ord.commit(h);
  if (packed) b->redo.advance();
  if (!piped && (rc = b->timing.stop(b->stream)) != DM_OK) return rc;
  if (pol && term) {      // the policy's step on the observations the termination launch left: one launch over the whole batch, behind every part
    if (P.join(b->stream)) return fail(DM_EHIP, "pipeline join failed");
    if ((rc = dm_policy_act(pol->P, c.o, pol->action, pol->vpred, b->n, pol->stochastic, pol->seed, pol->counter, (void*)b->stream)) != DM_OK) return rc;
  }
  if (kind == DM_PTR_HOST) {
    HIPCHK(hipMemcpyAsync(b->h_out, b->d_obs, b->out_bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    const size_t ob = (size_t)b->n * NOBS * sizeof(Ext), rb = (size_t)b->n * sizeof(Ext);
    memcpy(obs, b->h_out, ob); memcpy(reward, b->h_out + ob, rb); memcpy(done, b->h_out + ob + rb, (size_t)b->n);
  }
  return DM_OK;
}

extern "C" int dm_batch_step(dm_batch* b, const double* action, double* obs, double* reward, uint8_t* done, int32_t nsub, int32_t kind) {
  return step_impl(b, action, obs, reward, done, nsub, kind, nullptr);
}
extern "C" int dm_batch_step_act(dm_batch* b, const double* action, double* obs, double* reward, uint8_t* done, int32_t nsub,
                                 const float* weights, double* next_action, float* next_vpred, int32_t stochastic, uint64_t seed, uint64_t counter) {
  if (!weights || !next_action || !next_vpred) return fail(DM_EINVAL, "dm_batch_step_act: null policy argument");
  if (!aligned16(weights)) return fail(DM_EINVAL, "dm_batch_step_act: weights must be 16-byte aligned");
  dmp::PolicyArgs pa{weights, next_action, next_vpred, (int)stochastic, (unsigned long long)seed, (unsigned long long)counter};
  return step_impl(b, action, obs, reward, done, nsub, DM_PTR_DEVICE, &pa);
}

/* T steps per call (device pointers).  On the packed path ONE launch runs the whole horizon (k_rollout_packed); elsewhere T step launches. */
extern "C" int dm_batch_rollout(dm_batch* b, double* action, double* obs, double* reward, uint8_t* done, int32_t T, int32_t nsub,
                                const float* weights, float* vpred, int32_t stochastic, uint64_t seed, uint64_t counter) {
  // (the in-wave policy step loads the weights as float4.  Refused before `b` is looked at, as in dm_batch_step_act, where step_impl checks `b`: a call
  //  can then be shown to be refused without a device, on which alone a batch exists)
  if (!aligned16(weights)) return fail(DM_EINVAL, "dm_batch_rollout: weights must be 16-byte aligned");
  if (!b || !action || !obs || !reward || !done || T < 1 || nsub < 1) return fail(DM_EINVAL, "dm_batch_rollout: bad argument");
  if (weights && !vpred) return fail(DM_EINVAL, "dm_batch_rollout: a policy needs the value rows");
  const size_t n = (size_t)b->n;
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  if (!rollout_as_one_launch(b)) {        // (with option 101 the horizon launch records every wave's cycles)
    for (int t = 0; t < T; t++) {
      dmp::PolicyArgs pa{weights, action + (size_t)(t + 1) * n * NU, weights ? vpred + (size_t)t * n : nullptr, (int)stochastic, (unsigned long long)seed, (unsigned long long)counter + t};
      const int rc = step_impl(b, action + (size_t)t * n * NU, obs + (size_t)t * n * NOBS, reward + (size_t)t * n, done + (size_t)t * n, nsub, DM_PTR_DEVICE, weights ? &pa : nullptr);
      if (rc != DM_OK) return rc;
    }
    return DM_OK;
  }
  const int rc = b->queue.ensure_rows((int)T, b->stream);
  if (rc != DM_OK) return rc;
  hipLaunchKernelGGL(k_fill_rows, dim3(((int)T + 63) / 64), dim3(64), 0, b->stream, b->queue.d_rows, (const Ext*)action, obs, reward, done, (int)T, n);
  dmp::PolicyArgs pa{weights, action, vpred, (int)stochastic, (unsigned long long)seed, (unsigned long long)counter};
  return launch_horizon(b, (int)T, (int)nsub, pa);
}

extern "C" int dm_batch_get_obs(dm_batch* b, double* obs, int32_t kind) {
  if (!b || !obs) return fail(DM_EINVAL, "dm_batch_get_obs: null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  Ext* o = kind == DM_PTR_DEVICE ? obs : b->d_obs;
  const int tot = b->n * NOBS;
  hipLaunchKernelGGL(k_get_obs, dim3((tot + 255) / 256), dim3(256), 0, b->stream, b->B, o);
  HIPCHK(hipGetLastError());
  if (kind == DM_PTR_HOST) { HIPCHK(hipMemcpyAsync(obs, b->d_obs, (size_t)tot * 8, hipMemcpyDeviceToHost, b->stream)); HIPCHK(hipStreamSynchronize(b->stream)); }
  return DM_OK;
}

// field -> device array, element count, and whether its elements are `Real` (float64 at the ABI) or int32
static int field_ptr(dm_batch* b, int field, void** p, size_t* count, bool* is_real, size_t* esize) {
  const size_t n = b->n;
  *is_real = false; *esize = 0;
  switch (field) {
    case DM_F_QPOS: *p = b->B.qpos; *count = n * NQ; *is_real = true; break;
    case DM_F_QVEL: *p = b->B.qvel; *count = n * NV; *is_real = true; break;
    case DM_F_QACC_WARMSTART: *p = b->B.qws; *count = n * NV; *is_real = true; break;
    case DM_F_TIME: *p = b->B.time; *count = n; *is_real = true; break;
    case DM_F_FRAME_IDX: *p = b->B.frame_idx; *count = n; break;
    case DM_F_FRAME_INIT: *p = b->B.frame_init; *count = n; break;
    case DM_F_XIPOS: *p = b->B.xipos; *count = n * NB * 3; *is_real = true; break;
    case DM_F_COM_Z: *p = b->B.comz; *count = n; *is_real = true; break;
    case DM_F_NCON: *p = b->B.ncon; *count = n; break;
    case DM_F_NEFC: *p = b->B.nefc; *count = n; break;
    case DM_F_CONTACT_GEOMS: *p = b->B.cong; *count = n * MAXEFC * 2; break;
    case DM_F_STATUS: *p = b->B.status; *count = n; break;
    case DM_F_SOLVER_ITER: *p = b->B.solver_iter; *count = n; break;
    case DM_F_CTRL: *p = b->B.ctrl; *count = n * NU; *is_real = true; break;
    case DM_F_EPISODE: *p = b->B.episode; *count = n; break;
    case DM_F_CYCLE: *p = b->B.cycle; *count = n; break;
    case DM_F_EPISODE_STEPS: *p = b->d_ep_steps; *count = n; break;
    case DM_F_DONE_REASON: *p = b->d_done_reason; *count = n; break;
    case DM_F_CLIP: *p = b->d_clip; *count = n; break;
    case DM_F_PUSH_STATE: *p = b->d_push_state; *count = n * 5; break;
    case DM_F_PUSH_FORCE: *p = b->d_push_force; *count = n * 3; *esize = sizeof(double); break;   // float64 on the device in both libraries: copied as it is
    default: return fail(DM_EINVAL, "unknown field");
  }
  if (!*esize) *esize = *is_real ? sizeof(Ext) : 4;      // bytes per element at the ABI
  return DM_OK;
}
extern "C" int dm_batch_get(dm_batch* b, int32_t field, void* out, size_t bytes, int32_t kind) {
  if (!b || !out) return fail(DM_EINVAL, "dm_batch_get: null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  void* p; size_t cnt, esz; bool real; int rc;
  if ((rc = field_ptr(b, field, &p, &cnt, &real, &esz))) return rc;
  const size_t need = cnt * esz;
  if (bytes != need) return fail(DM_EINVAL, "dm_batch_get: buffer size does not match the field");
  if (real && sizeof(Real) != sizeof(Ext)) {       // float32 build: widen on the device, then copy
    Ext* dst = kind == DM_PTR_DEVICE ? (Ext*)out : b->d_cvt;
    hipLaunchKernelGGL(k_to_ext, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, b->stream, (const Real*)p, dst, cnt);
    HIPCHK(hipGetLastError());
    if (kind == DM_PTR_HOST) HIPCHK(hipMemcpyAsync(out, dst, need, hipMemcpyDeviceToHost, b->stream));
  } else HIPCHK(hipMemcpyAsync(out, p, need, kind == DM_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, b->stream));
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}
extern "C" int dm_batch_set(dm_batch* b, int32_t field, const void* in, size_t bytes, int32_t kind) {
  if (!b || !in) return fail(DM_EINVAL, "dm_batch_set: null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  void* p; size_t cnt, esz; bool real; int rc;
  if ((rc = field_ptr(b, field, &p, &cnt, &real, &esz))) return rc;
  const size_t need = cnt * esz;
  if (bytes != need) return fail(DM_EINVAL, "dm_batch_set: buffer size does not match the field");
  if (field == DM_F_XIPOS || field == DM_F_COM_Z || field == DM_F_NCON || field == DM_F_NEFC || field == DM_F_CONTACT_GEOMS || field == DM_F_SOLVER_ITER)
    return fail(DM_EINVAL, "dm_batch_set: derived field is read-only");
  if (field == DM_F_CLIP) {                      // validated on the host (a device caller's ids are read back first: one copy and a wait)
    std::vector<int> ids((size_t)b->n);
    if (kind == DM_PTR_HOST) memcpy(ids.data(), in, need);
    else { HIPCHK(hipMemcpyAsync(ids.data(), in, need, hipMemcpyDeviceToHost, b->stream)); HIPCHK(hipStreamSynchronize(b->stream)); }
    for (int e = 0; e < b->n; e++) if (ids[e] < 0 || ids[e] >= b->n_clips) return fail(DM_EINVAL, "dm_batch_set: DM_F_CLIP outside [0, n_clips)");
    HIPCHK(hipMemsetAsync(b->B.kin_ok, 0, (size_t)b->n, b->stream));
  }
  if (field == DM_F_QPOS) HIPCHK(hipMemsetAsync(b->B.kin_ok, 0, (size_t)b->n, b->stream));   // parked kinematics belong to the old positions
  if (real && sizeof(Real) != sizeof(Ext)) {       // float32 build: copy, then narrow on the device
    const Ext* src = (const Ext*)in;
    if (kind == DM_PTR_HOST) { HIPCHK(hipMemcpyAsync(b->d_cvt, in, need, hipMemcpyHostToDevice, b->stream)); src = b->d_cvt; }
    hipLaunchKernelGGL(k_from_ext, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, b->stream, src, (Real*)p, cnt);
    HIPCHK(hipGetLastError());
  } else HIPCHK(hipMemcpyAsync(p, in, need, kind == DM_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream));
  if (field == DM_F_CLIP && multi_clip(b)) {     // cursors beyond the new clip are held inside it (k_clip_clamp): no step can read past a clip's rows
    hipLaunchKernelGGL(k_clip_clamp, dim3((b->n + 255) / 256), dim3(256), 0, b->stream, b->B, clip_args(b));
    HIPCHK(hipGetLastError());
  }
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}

extern "C" int dm_batch_debug_forward(dm_batch* b, int32_t env, double* out_host) {
  if (!b || !out_host || env < 0 || env >= b->n) return fail(DM_EINVAL, "dm_batch_debug_forward: bad argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  HIPCHK(hipMemsetAsync(b->d_debug, 0, DM_DEBUG_DOUBLES * 8, b->stream));
  hipLaunchKernelGGL(k_debug_forward, dim3(1), dim3(64), 0, b->stream, b->d_model, b->B, (int)env, b->d_debug);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_host, b->d_debug, DM_DEBUG_DOUBLES * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}

extern "C" int dm_batch_read_profile(dm_batch* b, long long* out_host) {   /* [N,8]: kin, mass, bias, rows, constraint, total, nefc, iters */
  if (!b || !out_host || !b->d_prof) return fail(DM_EINVAL, "profile not enabled");
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(out_host, b->d_prof, (size_t)b->n * dm::PROF_SLOTS * sizeof(long long), hipMemcpyDeviceToHost));
  return DM_OK;
}
extern "C" int dm_batch_enable_timing(dm_batch* b, int32_t on) { if (!b) return fail(DM_EINVAL, "null batch"); b->timing.on = on != 0; b->timing.pending = false; return DM_OK; }
extern "C" int dm_batch_last_step_ms(dm_batch* b, float* ms) {
  if (!b || !ms) return fail(DM_EINVAL, "null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "dm_batch_last_step_ms: running the queued steps failed");      // (queued steps are timed by the launch that runs them)
  if (!b->timing.pending) return fail(DM_EINVAL, "no timed step recorded");
  HIPCHK(hipEventSynchronize(b->timing.ev1));
  HIPCHK(hipEventElapsedTime(&b->timing.last_ms, b->timing.ev0, b->timing.ev1));
  *ms = b->timing.last_ms;
  return DM_OK;
}
extern "C" int dm_batch_redo_total(dm_batch* b, int64_t* out) {
  if (!b || !out) return fail(DM_EINVAL, "dm_batch_redo_total: null argument");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  int v[8] = {0};
  HIPCHK(hipMemcpyAsync(v, b->B.redo_why, sizeof v, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (int k = 0; k < 8; k++) out[k] = v[k];      /* [0] total; [1..5] by reason: candidates, box slots, contacts, rows, PGS cost test */
  return DM_OK;
}
extern "C" int dm_batch_queue_stats(dm_batch* b, int64_t* out) {
  if (!b || !out) return fail(DM_EINVAL, "dm_batch_queue_stats: null argument");
  out[0] = b->queue.flushes; out[1] = b->queue.steps; out[2] = (int64_t)b->queue.q.size();
  return DM_OK;
}
extern "C" int dm_batch_truncations(dm_batch* b, int32_t* count, int32_t* index, double* qpos, double* qvel, int32_t cap, int32_t clear, int32_t kind) {
  if (!b || !count || cap < 0 || (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE)) return fail(DM_EINVAL, "dm_batch_truncations: null batch or count, negative cap, or bad ptr_kind");
  if (b->trunc.cap <= 0) return fail(DM_EINVAL, "dm_batch_truncations: the truncation log is off (DM_OPT_TRUNCATION_LOG)");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const hipMemcpyKind k = kind == DM_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t m = (size_t)(cap < b->trunc.cap ? cap : b->trunc.cap);
  HIPCHK(hipMemcpyAsync(count, b->trunc.d_count, sizeof(int32_t), k, b->stream));
  if (index && m) HIPCHK(hipMemcpyAsync(index, b->trunc.d_index, m * 4 * sizeof(int32_t), k, b->stream));
  if (qpos && m) HIPCHK(hipMemcpyAsync(qpos, b->trunc.d_qpos, m * NQ * sizeof(double), k, b->stream));
  if (qvel && m) HIPCHK(hipMemcpyAsync(qvel, b->trunc.d_qvel, m * NV * sizeof(double), k, b->stream));
  if (clear) { HIPCHK(hipMemsetAsync(b->trunc.d_count, 0, sizeof(int), b->stream)); b->trunc.tick = 0; }
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}
// ---- external pushes (include/dmenv.h; push_kernel.h, kernels_push.hip) ---------------------------------------------------------------------------------
static bool finite64(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }
extern "C" int dm_batch_push(dm_batch* b, const int32_t* body, const double* impulse, const uint8_t* mask, int32_t kind) {
  if (!b || !body || !impulse || (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE)) return fail(DM_EINVAL, "dm_batch_push: null batch, body or impulse, or bad ptr_kind");
  if (kind == DM_PTR_HOST)
    for (int e = 0; e < b->n; e++) {
      if (body[e] < 0 || body[e] >= NB) return fail(DM_EINVAL, "dm_batch_push: body outside 0..13");
      for (int k = 0; k < 3; k++) if (!finite64(impulse[(size_t)e * 3 + k])) return fail(DM_EINVAL, "dm_batch_push: non-finite impulse");
    }
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const void *bd, *ip, *mk; int rc;
  if ((rc = stage_in(b, b->d_fidx_in, body, (size_t)b->n * 4, kind, &bd))) return rc;
  if ((rc = stage_in(b, b->d_qvel_in, impulse, (size_t)b->n * 3 * 8, kind, &ip))) return rc;
  if ((rc = stage_in(b, b->d_mask, mask, (size_t)b->n, kind, &mk))) return rc;
  hipLaunchKernelGGL(k_push_now, dim3(b->n), dim3(64), 0, b->stream, b->d_model, b->B, (const int*)bd, (const double*)ip, (const unsigned char*)mk);
  HIPCHK(hipGetLastError());
  if (kind == DM_PTR_HOST) HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}
extern "C" int dm_batch_set_push_schedule(dm_batch* b, const dm_push_desc* d) {
  dm_push_desc p{};
  if (d && d->bodies != 0u) {      // (the description is judged before `b` is looked at: a bad one can then be shown to be refused without a device)
    p = *d;
    if (p.bodies & ~0x3ffeu) return fail(DM_EINVAL, "dm_batch_set_push_schedule: bodies is a mask over model bodies 1..13 (bits 1..13)");
    if (p.wait_min < 0 || p.wait_max < p.wait_min) return fail(DM_EINVAL, "dm_batch_set_push_schedule: 0 <= wait_min <= wait_max");
    if (p.duration_min < 1 || p.duration_max < p.duration_min) return fail(DM_EINVAL, "dm_batch_set_push_schedule: 1 <= duration_min <= duration_max");
    if (!finite64(p.force_min) || !finite64(p.force_max) || !(p.force_min >= 0) || !(p.force_max >= p.force_min)) return fail(DM_EINVAL, "dm_batch_set_push_schedule: 0 <= force_min <= force_max, finite");
    if (!(p.z_min >= -1) || !(p.z_max >= p.z_min) || !(p.z_max <= 1)) return fail(DM_EINVAL, "dm_batch_set_push_schedule: -1 <= z_min <= z_max <= 1");
  }
  if (!b) return fail(DM_EINVAL, "dm_batch_set_push_schedule: null batch");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  std::vector<int> ps((size_t)b->n * 5, 0);
  for (int e = 0; e < b->n; e++) ps[(size_t)e * 5] = -1;
  HIPCHK(hipMemcpyAsync(b->d_push_state, ps.data(), ps.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipMemsetAsync(b->d_push_force, 0, (size_t)b->n * 3 * sizeof(double), b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));              // (the host vector is read until the copy is done)
  b->push = p;
  return DM_OK;
}

extern "C" int dm_batch_join(dm_batch* b) {
  if (!b) return fail(DM_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  return DM_OK;
}
extern "C" int dm_batch_sync(dm_batch* b) {
  if (!b) return fail(DM_EINVAL, "null batch");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}
