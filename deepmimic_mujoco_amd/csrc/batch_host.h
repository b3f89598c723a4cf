// batch_host.h — the batch behind a dm_batch* and what every entry point that takes one does first, shared by the units with batch entry points
// (dmenv.hip: life cycle, state, step / rollout / queue; views.hip: render, state features and floor contacts).  Private to csrc/.
#pragma once
#include <vector>

#include "kernels.h"
#include "host_common.h"

struct dm_batch {
  int n = 0, device = 0;
  hipStream_t stream = nullptr; bool own_stream = false;
  dm::DevModel<Real>* d_model = nullptr;
  dm::Batch<Real> B{};
  dm::Batch<Real>* d_B = nullptr;   // a copy of B in device memory for the horizon launch (refreshed before each: its code is reached through calls, which take a pointer)
  Real *d_cfg = nullptr, *d_vel = nullptr, *d_imit = nullptr; int* d_order = nullptr;
  // self-ordering per-step launches (env_step.h dispatch_env): per pipelined part three phases of 64 bucket counters, and three phases of bucket
  // lists ([phase][bucket][n], a part's entries at its first env); ord_phase = the phase the part's last launch counted into, valid once one did
  int* d_ord_cnt = nullptr; int* d_ord_list = nullptr; int ord_phase[DM_MAX_PIPELINE] = {}; bool ord_valid[DM_MAX_PIPELINE] = {};
  // staging for DM_PTR_HOST callers
  Ext *d_action = nullptr, *d_obs = nullptr, *d_reward = nullptr; unsigned char *d_done = nullptr, *d_mask = nullptr;
  // host-pointer steps: obs | reward | done are ONE device block (d_obs points at its start) mirrored in pinned host memory, so a
  // step costs one H2D (action, from the pinned mirror) and one D2H instead of one pageable copy per array
  unsigned char* h_out = nullptr; Ext* h_action = nullptr; size_t out_bytes = 0;
  Ext* d_cvt = nullptr;   // float32 build: float64 staging for field reads / writes through host pointers
  Ext *d_qpos_in = nullptr, *d_qvel_in = nullptr; int* d_fidx_in = nullptr;
  double* d_debug = nullptr;
  long long* d_prof = nullptr; bool prof = false;
  int redo_phase = 0;    // which of a sub-batch's two redo counters the next packed launch counts into
  int redo_mode = -1;    // 1 / 0: the last packed step was / was not pipelined (the counter pairs are re-zeroed when that changes)
  // DM_OPT_STEP_QUEUE: dm_batch_step calls with device pointers are queued (nothing is launched) and executed together — one horizon launch,
  // every wave at its own pace — when the queue is full or any other entry point of the batch is called (dm_batch_join, ...)
  int queue_cap = 0; std::vector<dm::StepRow> q; int q_nsub = 1; dm::StepRow* d_rows = nullptr; int rows_cap = 0; long long queue_flushes = 0, queue_steps = 0;
  int horizon_mode = -1; // option 106: dm_batch_rollout on the packed path as ONE launch per horizon (1), as step launches (0), by batch size (-1, default)
  bool packed = false;   // option 105: four environments per wavefront (k_step_packed) where that kernel covers the configuration
  bool packed_ext = false;   // DM_OPT_PACKED = 2: per-step packed launches with the three-set code (k_step_packed_ext: 40 rows per env, ~8 % slower otherwise)
  bool two_tier = true, reorder = true, has_rows = true; int resident_waves = 2048;   // CUs x 8 single-wave workgroups (LDS-limited)
  bool timing = false; hipEvent_t ev0 = nullptr, ev1 = nullptr; float last_ms = 0.f; bool ev_pending = false;
  // pipelined sub-batches (DM_OPT_PIPELINE): the env range is cut into `pipe` contiguous parts, each stepped on its own stream
  int pipe = 1; hipStream_t ps[DM_MAX_PIPELINE] = {}; hipEvent_t ev_in = nullptr, ev_done[DM_MAX_PIPELINE] = {}; bool pipe_pending = false;
  // the views' staging block (views.hip Stage): a host caller's arrays and render's view records, laid out per call, grown on demand, freed with the batch
  unsigned char* d_rbuf = nullptr; size_t rbuf_bytes = 0;
  // early termination (DM_OPT_FALL_BODIES, DM_OPT_MAX_EPISODE_STEPS; term_kernel.h): k_terminate follows every per-step launch while either is non-zero
  unsigned fall_bodies = 0; int max_episode_steps = 0; int *d_ep_steps = nullptr, *d_done_reason = nullptr;   // [N] DM_F_EPISODE_STEPS, DM_F_DONE_REASON
  // DM_OPT_HORIZON_TERMINATION: the horizon launch and the step queue run with termination inside (k_rollout_packed_term) instead of falling back to step launches
  bool horizon_term = false;
  // the truncation log (DM_OPT_TRUNCATION_LOG, dm_batch_truncations): trunc_cap records, allocated when the option is set; trunc_tick = step calls since it was cleared
  int trunc_cap = 0, trunc_tick = 0; int *d_trunc_count = nullptr, *d_trunc_index = nullptr; double *d_trunc_qpos = nullptr, *d_trunc_qvel = nullptr;
  // the clip set (dm_mocap_create_set; step_rules.h ClipArgs): n_clips > 1 makes the batch multi-clip — its launches are the clip kernels (kernels_clips.hip,
  // kernels_packed_clips.hip).  d_clip is DM_F_CLIP (all 0 on a single-clip batch); clip_frames: the clips' lengths, for the host's range checks
  int n_clips = 1, clip_mode = 0; int* d_clip = nullptr; dm::ClipRec<Real>* d_clip_rec = nullptr; std::vector<int> clip_frames;
  // external pushes (dm_batch_push, dm_batch_set_push_schedule; push_kernel.h): DM_F_PUSH_STATE and DM_F_PUSH_FORCE, the schedule (push.bodies == 0: off — no
  // k_push launch) and the model descriptor's timestep in float64, from which a held force's impulse F h is formed
  int* d_push_state = nullptr; double* d_push_force = nullptr; dm_push_desc push{}; double timestep64 = 0;
};
inline bool push_on(const dm_batch* b) { return b->push.bodies != 0u; }
inline bool multi_clip(const dm_batch* b) { return b->n_clips > 1; }
inline dm::ClipArgs<Real> clip_args(const dm_batch* b) { return dm::ClipArgs<Real>{b->d_clip, b->d_clip_rec, b->n_clips, b->clip_mode}; }
// the batch's DM_F_CLIP on the host (stream-ordered copy and a wait): the per-env range checks of a multi-clip batch
inline int clip_ids_host(dm_batch* b, std::vector<int>& ids) {
  ids.resize((size_t)b->n);
  HIPCHK(hipMemcpyAsync(ids.data(), b->d_clip, (size_t)b->n * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return DM_OK;
}
// make the batch's stream wait for every sub-batch launch still in flight (no host wait)
inline int pipe_join(dm_batch* b) {
  if (!b->pipe_pending) return DM_OK;
  for (int h = 0; h < b->pipe; h++) if (hipStreamWaitEvent(b->stream, b->ev_done[h], 0) != hipSuccess) return DM_EHIP;
  b->pipe_pending = false;
  return DM_OK;
}

int flush_queue(dm_batch* b);      // (dmenv.hip)
// what every entry point other than a queued dm_batch_step does first: run the queued steps, then make the batch's stream wait for the sub-batch launches
inline int settle(dm_batch* b) {
  if (!b->q.empty()) { const int rc = flush_queue(b); if (rc != DM_OK) return rc; }
  return pipe_join(b);
}

inline int stage_in(dm_batch* b, void* dst, const void* src, size_t bytes, int kind, const void** use) {
  if (!src) { *use = nullptr; return DM_OK; }
  if (kind == DM_PTR_DEVICE) { *use = src; return DM_OK; }
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
  *use = dst;
  return DM_OK;
}
