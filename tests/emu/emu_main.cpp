// emu_main.cpp — TEST INFRASTRUCTURE: C entry points that run the HIP kernel source on the fibre wave testbench.
// Mirrors the subset of include/dmenv.h the parity tests use, one environment after another.  The batch, set_state and the packed-step and horizon
// launches are host_batch.h's; here stand the options, the fields, the one-env step, reset, the debug dump and the dispatch order.
#include <cstdio>
#include <string>

#include "host_batch.h"      // the fibre runner (wave_fibres.h), the kernel source, HostBatch and the launches

namespace {
struct EmuBatch : HostBatch {
  bool two_tier = true, packed = false, packed_ext = false;   // packed_ext: DM_OPT_PACKED = 2 (per-step launches with the three-set code: k_step_packed_ext)
  long redo_total = 0;
};
}  // namespace

extern "C" {
void* emu_create(const dm_model_desc* d, const double* cfg, const double* vel, int F, int n, unsigned flags, double mocap_dt) {
  EmuBatch* e = new EmuBatch();
  std::string err;
  if (build_dev_model(d, &e->M, &err) != 0) { fprintf(stderr, "emu_create: %s\n", err.c_str()); delete e; return nullptr; }
  e->M.enable_contact = (flags & DM_FLAG_NO_CONTACT) ? 0 : 1;
  e->M.enable_limit = (flags & DM_FLAG_NO_LIMIT) ? 0 : 1;
  wire(*e, n, cfg, vel, F, mocap_dt);
  for (int i = 0; i < n; i++) for (int k = 0; k < NQ; k++) e->qpos[(size_t)i * NQ + k] = e->M.qpos0[k];
  e->B.diag = 1;
  return e;
}
void emu_set_imitation(void* h, const double* table, const double* params) { set_imitation(*(EmuBatch*)h, table, params); }
void emu_destroy(void* h) { delete (EmuBatch*)h; }
void emu_invalidate_kin(void* h) { EmuBatch* e = (EmuBatch*)h; std::fill(e->kin_ok.begin(), e->kin_ok.end(), 0); }   // as the device entry points do
void emu_set_option(void* h, int opt, long long v) {
  EmuBatch* e = (EmuBatch*)h;
  if (opt == DM_OPT_REWARD_MODE) e->B.reward_mode = (int)v;
  else if (opt == DM_OPT_AUTORESET) e->B.autoreset = (int)v;
  else if (opt == DM_OPT_ACTION_MODE) e->B.action_mode = (int)v;
  else if (opt == DM_OPT_SEED) e->B.seed = (unsigned long long)v;
  else if (opt == DM_OPT_DIAGNOSTICS) e->B.diag = v != 0;
  else if (opt == 100) e->B.env_offset = (int)v;
  else if (opt == 102) e->two_tier = v != 0;
  else if (opt == 105 || opt == DM_OPT_PACKED) { e->packed = v != 0; e->packed_ext = v == 2; }
  else if (opt == 103) e->M.pgs_detect = v ? -1e300 : 1e-10;
}
void* emu_field(void* h, int field) {
  EmuBatch* e = (EmuBatch*)h;
  switch (field) {
    case DM_F_QPOS: return e->qpos.data(); case DM_F_QVEL: return e->qvel.data(); case DM_F_QACC_WARMSTART: return e->qws.data();
    case DM_F_TIME: return e->time.data(); case DM_F_FRAME_IDX: return e->fidx.data(); case DM_F_FRAME_INIT: return e->finit.data();
    case DM_F_XIPOS: return e->xipos.data(); case DM_F_COM_Z: return e->comz.data(); case DM_F_NCON: return e->ncon.data();
    case DM_F_NEFC: return e->nefc.data(); case DM_F_CONTACT_GEOMS: return e->cong.data(); case DM_F_STATUS: return e->status.data();
    case DM_F_SOLVER_ITER: return e->siter.data(); case DM_F_CTRL: return e->ctrl.data(); case DM_F_EPISODE: return e->episode.data();
    case DM_F_CYCLE: return e->cycle.data();
  }
  return nullptr;
}
void emu_step(void* h, const double* action, double* obs, double* reward, unsigned char* done, int nsub) {
  EmuBatch* e = (EmuBatch*)h;
  if (e->packed && e->B.reward_mode <= 4) {          // the device's routing (dmenv.hip step_impl): four envs per wave, overflowing envs re-stepped one per wave
    e->redo_total += e->packed_ext ? packed_step_launch<true>(*e, action, obs, reward, done, nsub) : packed_step_launch<false>(*e, action, obs, reward, done, nsub);
    return;
  }
  for (int env = 0; env < e->B.n_envs; env++)
  {
    // same scheme as the device: register tier (32 columns of A here, so that the overflow strip is exercised by every
    // evaluation with more than 32 rows) or, with option 102 = 0, all 64 columns in registers
    if (e->two_tier) run_wave([&](int lane) { env_step<double, 32>(e->M, e->B, e->sh, e->xs, env, lane, action, obs, reward, done, nsub); });
    else run_wave([&](int lane) { env_step<double, MAXEFC>(e->M, e->B, e->sh, e->xs, env, lane, action, obs, reward, done, nsub); });
  }
}
// dm_batch_rollout on the packed path, open loop (k_rollout_packed without a policy): action [T, n, 28], obs [T, n, 56], reward / done [T, n]
void emu_rollout(void* h, const double* action, double* obs, double* reward, unsigned char* done, int nsub, int T) {
  EmuBatch* e = (EmuBatch*)h;
  e->redo_total += horizon_launch<false>(*e, action, obs, reward, done, nsub, T, [](int, int) {});
}
long emu_redo_total(void* h) { return ((EmuBatch*)h)->redo_total; }
// dm_batch_redo_total's six counters: the total, then the reasons the packed step tallies in B.redo_why[1 .. 5] (candidates, box slots, contacts, rows, PGS test)
void emu_redo_reasons(void* h, long* out) {
  EmuBatch* e = (EmuBatch*)h;
  out[0] = e->redo_total;
  for (int r = 1; r < 6; r++) out[r] = e->B.redo_why[r];
}
// emu_rollout, and what a policy behind every step would read: the slots' qpos[7 ..] and qvel[6 ..] at the place of the policy's step -> pin [T, n, 56]
void emu_rollout_inputs(void* h, const double* action, double* obs, double* reward, unsigned char* done, int nsub, int T, double* pin) {
  EmuBatch* e = (EmuBatch*)h;
  const int n = e->B.n_envs;
  e->redo_total += horizon_launch<false>(*e, action, obs, reward, done, nsub, T, [&](int first, int t) {
    const int lane = dmw::lane(), slot = lane >> 4, sl = lane & 15, env = first + slot;
    if (env >= n) return;
    for (int o = sl; o < NOBS; o += SW) pin[((size_t)t * n + env) * NOBS + o] = o < 28 ? e->roll.sh[slot].qpos[7 + o] : e->roll.sh[slot].qvel[6 + (o - 28)];
  });
}
// Self-ordering per-step launches (env_step.h order_ticket / dispatch_env) without the physics: `count` envs first .. first + count - 1 of a batch of n take
// their tickets in the order `arrival` names them (n_arrival of them; keys from nefc / iter), then the waves of the next launch look their envs up — one env per wave
// (out1[count]) and four per wave (out4[4 * ceil(count / 4)], spare slots repeat the last position).  with_tickets = 0: no tickets -> `order` / identity.
void emu_dispatch(int n, int first, int count, const int* nefc, const int* iter, const int* arrival, int n_arrival, const int* order, int with_tickets, int* out1, int* out4) {
  std::vector<int> cnt(3 * ORD_BUCKETS, 0), list((size_t)3 * ORD_BUCKETS * n, -1);
  Batch<double> B{};
  B.order = const_cast<int*>(order);
  B.ord_stride = n;
  B.ord_out = cnt.data() + ORD_BUCKETS; B.ordl_out = list.data() + (size_t)ORD_BUCKETS * n + first;
  if (with_tickets) for (int i = 0; i < n_arrival; i++) { const int e = arrival[i]; order_ticket(B, e, nefc[e], iter[e]); }
  B.ord_in = with_tickets ? cnt.data() + ORD_BUCKETS : nullptr; B.ordl_in = list.data() + (size_t)ORD_BUCKETS * n + first;
  B.ord_out = cnt.data() + 2 * ORD_BUCKETS; B.ordl_out = list.data() + (size_t)2 * ORD_BUCKETS * n + first;
  B.ord_zero = cnt.data();
  for (int k = 0; k < ORD_BUCKETS; k++) cnt[k] = 12345;              // the phase the launch's first workgroup clears
  for (int w = 0; w < count; w++)
    run_wave([&](int lane) { int e; dispatch_env<1>(B, first, count, w, lane, w == 0, &e); if (lane == 0) out1[w] = e; });
  for (int k = 0; k < ORD_BUCKETS; k++) if (cnt[k] != 0) out1[0] = -1000 - k;   // (reported as a bad env)
  for (int w = 0; w * SLOTS < count; w++)
    run_wave([&](int lane) { int e[SLOTS]; dispatch_env<SLOTS>(B, first, count, SLOTS * w, lane, false, e); if (lane == 0) for (int j = 0; j < SLOTS; j++) out4[SLOTS * w + j] = e[j]; });
}
void emu_set_state(void* h, const double* qpos, const double* qvel, const int* fidx, const unsigned char* mask) { set_state(*(EmuBatch*)h, qpos, qvel, fidx, mask); }
void emu_reset(void* h, int mode, int hard, const unsigned char* mask) {
  EmuBatch* e = (EmuBatch*)h;
  std::fill(e->kin_ok.begin(), e->kin_ok.end(), 0);
  for (int env = 0; env < e->B.n_envs; env++) {
    if (mask && !mask[env]) continue;
    run_wave([&](int lane) {
      load_env(e->M, e->B, e->sh, env, lane, (const double*)0);
      reset_env(e->M, e->B, e->sh, env, lane, mode, hard);
      store_state(e->B, e->sh, env, lane);
      { const LaneTopo lt = lane_topo(lane); stage_tables(e->sh, lane); dmw::sync(); forward(e->M, e->sh, lane, lt, (const DebugOut*)0); }
      store_derived(e->B, e->M, e->sh, env, lane);
    });
  }
}
void emu_debug_forward(void* h, int env, double* out) {
  EmuBatch* e = (EmuBatch*)h;
  for (int i = 0; i < DM_DEBUG_DOUBLES; i++) out[i] = 0;
  run_wave([&](int lane) {
    load_env(e->M, e->B, e->sh, env, lane, (const double*)0);
    if (lane < NU) { const int d = lane + 6; e->sh.act[d] = e->M.gear[d] * clampr(e->B.ctrl[(size_t)env * NU + lane], e->M.ctrl_lo[d], e->M.ctrl_hi[d]); }
    dmw::sync();
    DebugOut dbg{out};
    { const LaneTopo lt = lane_topo(lane); stage_tables(e->sh, lane); dmw::sync(); forward(e->M, e->sh, lane, lt, &dbg); }
    store_derived(e->B, e->M, e->sh, env, lane);
  });
}
}
