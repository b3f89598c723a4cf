// batch_host.h — the batch behind a dm_batch* and what every entry point that takes one does first, shared by the units with batch entry points
// (dmenv.hip: life cycle, state, step / rollout / queue; views.hip: render, state features and floor contacts).  Private to csrc/.
#pragma once
#include <vector>

#include "kernels.h"
#include "host_common.h"

// ---- the parts of a batch's step path: each owns its state and states its invariant once; dmenv.hip's entry points call them.
// DM_OPT_STEP_QUEUE: dm_batch_step calls with device pointers are queued (nothing is launched) and executed together — one horizon launch, every wave at
// its own pace — when the queue is full or any other entry point of the batch is called (dm_batch_join, ...).  d_rows: the horizon's table of per-step
// buffers, shared with dm_batch_rollout
struct StepQueue {
  int cap = 0; std::vector<dm::StepRow> q; int nsub = 1; dm::StepRow* d_rows = nullptr; int rows_cap = 0; long long flushes = 0, steps = 0;
  int ensure_rows(int T, hipStream_t stream) {
    if (T <= rows_cap) return DM_OK;
    HIPCHK(hipStreamSynchronize(stream));            // (a launch still reading the old table)
    if (d_rows) { HIPCHK(hipFree(d_rows)); d_rows = nullptr; rows_cap = 0; }
    HIPCHK(hipMalloc((void**)&d_rows, up256((size_t)T) * sizeof(dm::StepRow)));
    rows_cap = (int)up256((size_t)T);
    return DM_OK;
  }
  void upload(hipStream_t stream);   // the queued rows into d_rows, a chunk per k_put_rows launch; empties the queue and counts the flush (dmenv.hip, beside the kernel)
};
// pipelined sub-batches (DM_OPT_PIPELINE): the env range is cut into `depth` contiguous parts, each stepped on its own stream
struct Pipeline {
  int depth = 1; hipStream_t ps[DM_MAX_PIPELINE] = {}; hipEvent_t ev_in = nullptr, ev_done[DM_MAX_PIPELINE] = {}; bool pending = false;
  struct Part { int lo, count; };
  Part part(int n, int h) const { const int lo = (int)((long long)n * h / depth), hi = (int)((long long)n * (h + 1) / depth); return {lo, hi - lo}; }   // the partition: stated here alone
  int configure(int d) {             // streams and events are created once and kept; the depth moves only when all of them exist
    for (int h = 0; h < d && d > 1; h++) { if (!ps[h]) HIPCHK(hipStreamCreateWithFlags(&ps[h], hipStreamNonBlocking)); if (!ev_done[h]) HIPCHK(hipEventCreateWithFlags(&ev_done[h], hipEventDisableTiming)); }
    if (d > 1 && !ev_in) HIPCHK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    depth = d; return DM_OK;
  }
  int join(hipStream_t stream) {     // make `stream` wait for every sub-batch launch still in flight (no host wait)
    for (int h = 0; h < depth && pending; h++) if (hipStreamWaitEvent(stream, ev_done[h], 0) != hipSuccess) return DM_EHIP;
    pending = false; return DM_OK;
  }
  void destroy() { for (int h = 0; h < DM_MAX_PIPELINE; h++) { if (ps[h]) hipStreamDestroy(ps[h]); if (ev_done[h]) hipEventDestroy(ev_done[h]); } if (ev_in) hipEventDestroy(ev_in); }
};
// Self-ordering per-step launches (env_step.h dispatch_env / order_ticket): per pipelined part three phases of 64 bucket counters (d_cnt), and three phases of
// bucket lists (d_list: [phase][bucket][n], a part's entries at its first env).  A step launch of part h = [lo, ...) reads the tickets the part's previous
// launch left (phase p), its envs take theirs from phase p + 1, its first workgroup clears phase p + 2 for the launch after it.  A part's tickets stay a
// permutation of the part whatever runs in between (horizon launches, resets: only their keys grow stale); a new partition (DM_OPT_PIPELINE) starts afresh.
// The part's phase and `valid` flag move on only once its launch is known to have gone out (commit after hipGetLastError): a failed launch leaves the
// descriptor where the last successful one put it, so the next launch reads tickets somebody really counted.
struct OrderTickets {
  int* d_cnt = nullptr; int* d_list = nullptr; int phase[DM_MAX_PIPELINE] = {}; bool valid[DM_MAX_PIPELINE] = {};
  int bind(dm::Batch<Real>& Bh, int n, int h, int lo, hipStream_t st) {      // the descriptor of part h's next launch, which goes to `st`
    int* cnt = d_cnt + (size_t)h * 3 * dm::ORD_BUCKETS;
    if (!valid[h]) { HIPCHK(hipMemsetAsync(cnt, 0, 3 * dm::ORD_BUCKETS * sizeof(int), st)); phase[h] = 0; }
    const int p = phase[h], pn = (p + 1) % 3, pz = (p + 2) % 3;
    Bh.ord_in = valid[h] ? cnt + p * dm::ORD_BUCKETS : nullptr; Bh.ordl_in = d_list + (size_t)p * dm::ORD_BUCKETS * n + lo;
    Bh.ord_out = cnt + pn * dm::ORD_BUCKETS; Bh.ordl_out = d_list + (size_t)pn * dm::ORD_BUCKETS * n + lo;
    Bh.ord_zero = cnt + pz * dm::ORD_BUCKETS; Bh.ord_stride = n;
    return DM_OK;
  }
  void commit(int h) { phase[h] = (phase[h] + 1) % 3; valid[h] = true; }
  void invalidate() { for (int h = 0; h < DM_MAX_PIPELINE; h++) valid[h] = false; }
};
// The packed kernels' redo counters (Batch::redo_count: a pair per sub-batch).  The packed kernel counts the environments beyond its capacities into the
// pair's first counter (this call's phase), the redo launch steps them one per wave and clears the other one for the next call: the two alternate from step
// to step, no memset between launches.  mode: 1 / 0 the last packed step was / was not pipelined, -1 unknown; when it changes all pairs are re-zeroed and the
// phase restarts.  (A step that is not pipelined has joined every sub-batch stream: all of them are idle, so pair 0 alone is clean for it.)
struct RedoCounters {
  int phase = 0, mode = -1;
  struct Pair { int* count; int* next; };
  int begin_step(bool piped, int* d_count, Pipeline& pipe, hipStream_t stream) {
    if ((piped ? 1 : 0) == mode) return DM_OK;      // (else rare: the first packed step, or a host-pointer step between pipelined ones; every earlier launch is ordered before `stream` here)
    if (piped && pipe.join(stream)) return fail(DM_EHIP, "pipeline join failed");
    HIPCHK(hipMemsetAsync(d_count, 0, 2 * DM_MAX_PIPELINE * sizeof(int), stream));
    mode = piped ? 1 : 0; phase = 0; return DM_OK;
  }
  Pair pair(int* d_count, int h) const { return {d_count + 2 * h + phase, d_count + 2 * h + (1 - phase)}; }
  void advance() { phase ^= 1; }
  void invalidate() { mode = -1; }
};
// the truncation log (DM_OPT_TRUNCATION_LOG, dm_batch_truncations): `cap` records; tick = step calls since it was cleared, the log's clock
struct TruncLog {
  int cap = 0, tick = 0; int *d_count = nullptr, *d_index = nullptr; double *d_qpos = nullptr, *d_qvel = nullptr;
  void release() {                   // the only free
    for (void* x : {(void*)d_count, (void*)d_index, (void*)d_qpos, (void*)d_qvel}) if (x) hipFree(x);
    d_count = d_index = nullptr; d_qpos = d_qvel = nullptr; cap = 0; tick = 0;
  }
  int resize(int records, hipStream_t stream) {      // the only allocator; nothing may still be appending to the old log (the caller has waited)
    release();
    const size_t c = (size_t)records, ni = c * 4 * sizeof(int), nq = c * dm::NQ * sizeof(double), nv = c * dm::NV * sizeof(double);
    if (records <= 0) return DM_OK;
    if (hipMalloc((void**)&d_count, sizeof(int)) != hipSuccess || hipMalloc((void**)&d_index, ni) != hipSuccess || hipMalloc((void**)&d_qpos, nq) != hipSuccess ||
        hipMalloc((void**)&d_qvel, nv) != hipSuccess) { release(); (void)hipGetLastError(); return fail(DM_ENOMEM, "DM_OPT_TRUNCATION_LOG: hipMalloc failed"); }
    /* cleared on the batch's stream, ahead of every later launch (a pipelined part's waits for this stream at the time of its call) */
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(int), stream)); HIPCHK(hipMemsetAsync(d_index, 0, ni, stream));
    HIPCHK(hipMemsetAsync(d_qpos, 0, nq, stream)); HIPCHK(hipMemsetAsync(d_qvel, 0, nv, stream));
    cap = records; return DM_OK;
  }
  int take_ticks(int T) { const int first = tick; if (cap > 0) tick += T; return first; }      // T step calls' ticks -> the first; the clock runs only while the log is on
};
// dm_batch_enable_timing: ev0 / ev1 bracket the last step's (sub-batch 0's, the horizon's) launches on the stream they went to
struct StepTiming {
  bool on = false; hipEvent_t ev0 = nullptr, ev1 = nullptr; float last_ms = 0.f; bool pending = false;
  void collect() { if (on && pending) { hipEventSynchronize(ev1); hipEventElapsedTime(&last_ms, ev0, ev1); } }      // the previous step's time, before its events are recorded anew
  int start(hipStream_t st) { if (on) HIPCHK(hipEventRecord(ev0, st)); return DM_OK; }
  int stop(hipStream_t st) { if (on) { HIPCHK(hipEventRecord(ev1, st)); pending = true; } return DM_OK; }
};

struct dm_batch {
  int n = 0, device = 0;
  hipStream_t stream = nullptr; bool own_stream = false;
  dm::DevModel<Real>* d_model = nullptr;
  dm::Batch<Real> B{};
  dm::Batch<Real>* d_B = nullptr;   // a copy of B in device memory for the horizon launch (refreshed before each: its code is reached through calls, which take a pointer)
  Real *d_cfg = nullptr, *d_vel = nullptr, *d_imit = nullptr; int* d_order = nullptr;
  StepQueue queue; Pipeline pipe; OrderTickets ord; RedoCounters redo; TruncLog trunc; StepTiming timing;      // the step path's parts (above)
  // staging for DM_PTR_HOST callers
  Ext *d_action = nullptr, *d_obs = nullptr, *d_reward = nullptr; unsigned char *d_done = nullptr, *d_mask = nullptr;
  // host-pointer steps: obs | reward | done are ONE device block (d_obs points at its start) mirrored in pinned host memory, so a
  // step costs one H2D (action, from the pinned mirror) and one D2H instead of one pageable copy per array
  unsigned char* h_out = nullptr; Ext* h_action = nullptr; size_t out_bytes = 0;
  Ext* d_cvt = nullptr;   // float32 build: float64 staging for field reads / writes through host pointers
  Ext *d_qpos_in = nullptr, *d_qvel_in = nullptr; int* d_fidx_in = nullptr;
  double* d_debug = nullptr;
  long long* d_prof = nullptr; bool prof = false;
  int horizon_mode = -1; // option 106: dm_batch_rollout on the packed path as ONE launch per horizon (1), as step launches (0), by batch size (-1, default)
  bool packed = false;   // option 105: four environments per wavefront (k_step_packed) where that kernel covers the configuration
  bool packed_ext = false;   // DM_OPT_PACKED = 2: per-step packed launches with the three-set code (k_step_packed_ext: 40 rows per env, ~8 % slower otherwise)
  bool two_tier = true, reorder = true, has_rows = true; int resident_waves = 2048;   // CUs x 8 single-wave workgroups (LDS-limited)
  // the views' staging block (views.hip Stage): a host caller's arrays and render's view records, laid out per call, grown on demand, freed with the batch
  unsigned char* d_rbuf = nullptr; size_t rbuf_bytes = 0;
  // early termination (DM_OPT_FALL_BODIES, DM_OPT_MAX_EPISODE_STEPS; term_kernel.h): k_terminate follows every per-step launch while either is non-zero
  unsigned fall_bodies = 0; int max_episode_steps = 0; int *d_ep_steps = nullptr, *d_done_reason = nullptr;   // [N] DM_F_EPISODE_STEPS, DM_F_DONE_REASON
  // DM_OPT_HORIZON_TERMINATION: the horizon launch and the step queue run with termination inside (k_rollout_packed_term) instead of falling back to step launches
  bool horizon_term = false;
  // DM_OPT_HORIZON_SPD: in action modes 3 and 4 the horizon launch and the step queue run with the controller inside (kernels_rollout_spd.hip) instead of falling back to step launches
  bool horizon_spd = false;
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
// launch the kernel `plain`, or on a multi-clip batch its twin `clips` with the clip argument appended
template <class KP, class KC, class... Args>
inline void launch_clip_or_plain(const dm_batch* b, KP plain, KC clips, dim3 grid, dim3 block, hipStream_t st, Args... args) {
  if (multi_clip(b)) hipLaunchKernelGGL(clips, grid, block, 0, st, args..., clip_args(b));
  else hipLaunchKernelGGL(plain, grid, block, 0, st, args...);
}
// DM_OPT_PIPELINE: the stored dispatch order belongs to the previous partition (identity for the next launch), and so do the tickets of the per-step
// launches; sub-batches beyond the new depth keep whatever their redo counters last held, so the next packed step re-zeroes all 2 * DM_MAX_PIPELINE counters
// and restarts the phase.  (The caller has joined everything in flight.)
inline int set_pipeline(dm_batch* b, int depth) {
  if (const int rc = b->pipe.configure(depth)) return rc;
  b->B.order = nullptr; b->ord.invalidate(); b->redo.invalidate(); return DM_OK;
}

int flush_queue(dm_batch* b);      // (dmenv.hip)
// what every entry point other than a queued dm_batch_step does first: run the queued steps, then make the batch's stream wait for the sub-batch launches
inline int settle(dm_batch* b) {
  if (!b->queue.q.empty()) { const int rc = flush_queue(b); if (rc != DM_OK) return rc; }
  return b->pipe.join(b->stream);
}

inline int stage_in(dm_batch* b, void* dst, const void* src, size_t bytes, int kind, const void** use) {
  if (!src) { *use = nullptr; return DM_OK; }
  if (kind == DM_PTR_DEVICE) { *use = src; return DM_OK; }
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
  *use = dst;
  return DM_OK;
}
