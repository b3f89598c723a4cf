// emu_clips.cpp — TEST INFRASTRUCTURE: the wave testbench's front end for the clip instantiations of the step and reset routines (step_rules.h ClipArgs;
// the device's kernels_clips.hip / kernels_packed_clips.hip), both lane layouts.  The EmuBatch and the emu_* entry points are those of ../emu/emu_main.cpp,
// compiled into this library as they are (with it the fibre runner of ../emu/wave_fibres.h, the host batch of ../emu/host_batch.h and the unmodified kernel
// source); the emuc_* entry points below add the clip set beside an EmuBatch, as the device keeps its ClipArgs beside the Batch.
#include "../emu/emu_main.cpp"

namespace {
struct EmuClips {
  EmuBatch* e = nullptr;
  std::vector<int> clip;
  std::vector<ClipRec<double>> rec;
  int mode = 0;
  ClipArgs<double> args() { return ClipArgs<double>{clip.data(), rec.data(), (int)rec.size(), mode}; }
};
}  // namespace

extern "C" {
// cfg / vel: the clips' tables concatenated row-wise ([F, 35], [F, 34], F = sum of n_frames); one {row0, n_frames, dt, cdf} per clip
void* emuc_create(const dm_model_desc* d, const double* cfg, const double* vel, int F, int n, unsigned flags, int K, const int* row0, const int* n_frames,
                  const double* dt, const double* cdf) {
  EmuClips* c = new EmuClips();
  c->e = (EmuBatch*)emu_create(d, cfg, vel, F, n, flags, dt[0]);
  if (!c->e) { delete c; return nullptr; }
  for (int k = 0; k < K; k++) c->rec.push_back(ClipRec<double>{row0[k], n_frames[k], dt[k], 0.0, 0.0, 0.0, cdf[k]});
  c->clip.resize(n);
  for (int i = 0; i < n; i++) c->clip[i] = i % K;
  return c;
}
// table: the clips' feature tables concatenated; params: the shared block (13..15 unused); per clip its loop flag and cycle shift
void emuc_set_imitation(void* h, const double* table, const double* params, const double* loop, const double* shift_x, const double* shift_y) {
  EmuClips* c = (EmuClips*)h;
  emu_set_imitation(c->e, table, params);
  for (size_t k = 0; k < c->rec.size(); k++) { c->rec[k].loop = loop[k]; c->rec[k].shift_x = shift_x[k]; c->rec[k].shift_y = shift_y[k]; }
}
void emuc_destroy(void* h) { EmuClips* c = (EmuClips*)h; emu_destroy(c->e); delete c; }
void* emuc_batch(void* h) { return ((EmuClips*)h)->e; }        // for emu_set_option / emu_field / emu_set_state / emu_invalidate_kin
int* emuc_clip(void* h) { return ((EmuClips*)h)->clip.data(); }
void emuc_set_clip_mode(void* h, int mode) { ((EmuClips*)h)->mode = mode; }

// emu_step with the clip argument: the device's routing on a multi-clip batch (dmenv.hip step_impl)
void emuc_step(void* h, const double* action, double* obs, double* reward, unsigned char* done, int nsub) {
  EmuClips* c = (EmuClips*)h;
  EmuBatch* e = c->e;
  const ClipArgs<double> ca = c->args();
  if (e->packed && e->B.reward_mode <= 4) {
    const int n = e->B.n_envs;
    e->B.redo_count[0] = 0;
    for (int first = 0; first < n; first += SLOTS)
      run_wave([&](int lane) {
        const int slot = lane >> 4, sl = lane & 15;
        stage_slot_tables(e->tabs, lane);
        int pos = first + slot;
        const bool live = pos < n;
        if (!live) pos = n - 1;
        if (e->packed_ext) slot_env_step<double, false, false, SLOT_MAXROWS>(e->M, e->B, e->slots[slot], e->tabs, pos, sl, lane, live, action, obs, reward, done, nsub, e->B.redo_count, e->B.redo_list, (long long*)0, false, ca);
        else slot_env_step<double, false, false, 2 * SW>(e->M, e->B, e->slots[slot], e->tabs, pos, sl, lane, live, action, obs, reward, done, nsub, e->B.redo_count, e->B.redo_list, (long long*)0, false, ca);
      });
    e->redo_total += e->B.redo_count[0];
    for (int i = 0; i < e->B.redo_count[0]; i++) {
      const int env = e->B.redo_list[i];
      run_wave([&](int lane) { env_step<double, 32, false>(e->M, e->B, e->sh, e->xs, env, lane, action, obs, reward, done, nsub, (long long*)0, ca); });
    }
    return;
  }
  for (int env = 0; env < e->B.n_envs; env++) {
    if (e->two_tier) run_wave([&](int lane) { env_step<double, 32, false>(e->M, e->B, e->sh, e->xs, env, lane, action, obs, reward, done, nsub, (long long*)0, ca); });
    else run_wave([&](int lane) { env_step<double, MAXEFC, false>(e->M, e->B, e->sh, e->xs, env, lane, action, obs, reward, done, nsub, (long long*)0, ca); });
  }
}
// k_reset_clips
void emuc_reset(void* h, int mode, int hard, const unsigned char* mask) {
  EmuClips* c = (EmuClips*)h;
  EmuBatch* e = c->e;
  const ClipArgs<double> ca = c->args();
  std::fill(e->kin_ok.begin(), e->kin_ok.end(), 0);
  for (int env = 0; env < e->B.n_envs; env++) {
    if (mask && !mask[env]) continue;
    run_wave([&](int lane) {
      load_env(e->M, e->B, e->sh, env, lane, (const double*)0);
      reset_env_clips(e->M, e->B, ca, e->sh, env, lane, mode, hard);
      store_state(e->B, e->sh, env, lane);
      { const LaneTopo lt = lane_topo(lane); stage_tables(e->sh, lane); dmw::sync(); forward(e->M, e->sh, lane, lt, (const DebugOut*)0); }
      store_derived(e->B, e->M, e->sh, env, lane);
    });
  }
}
}
