// host_batch.h — TEST INFRASTRUCTURE: the one host batch of the wave testbench and the launches it emulates.  HostBatch owns every array a Batch<double>
// points to; wire() is the only place in tests/ that sizes them and sets the pointers, so a new Batch field is wired here or nowhere.  The launches are the
// device's, one wave after another on the fibres of wave_fibres.h: set_state (k_set_state), the packed step launch with its one-env re-steps (dmenv.hip
// step_impl's routing), the horizon launch (k_rollout_packed and its kin).  Used by emu_main.cpp (libdmemu*.so) and, through host_rollout.h, by the two
// horizon twins; like wave_fibres.h, which it includes, it belongs in one translation unit per program.
#pragma once
#include <algorithm>
#include <vector>

#include "wave_fibres.h"
// kernel source, unmodified
#include "env_step.h"
#include "slot_step.h"
#include "model_host.h"

using namespace dm;

namespace {
constexpr int RESTEP_ROWS = 48;      // = csrc/kernels.h RESTEP_ROWS: the register tier of the horizon launch's in-wave re-step

struct HostBatch {
  DevModel<double> M;
  Batch<double> B;
  int n = 0;
  std::vector<double> qpos, qvel, qws, time, ctrl, xipos, comz, cfg, vel, aovf, imit, kin;
  std::vector<unsigned char> kin_ok;
  std::vector<int> fidx, finit, ncon, nefc, cong, status, siter, episode, cycle, redo;
  std::vector<int> steps, reason;                                                          // the termination launch's arrays (term_kernel.h TermArgs) ...
  std::vector<int> log_count, log_index; std::vector<double> log_qpos, log_qvel;           // ... and its truncation log
  SlotShared<double> slots[SLOTS];
  SlotOrOne<double> roll;            // the horizon launch: the one-env code's LDS ALIASES the four slots', as in k_rollout_packed
  SlotTables tabs;
  Shared<double> sh;
  StepScratch<double> xs;
};

// Sizes every array for n environments (zeroed state; M is the caller's) and points a fresh Batch<double> at them: a mocap table of F frames, no imitation
// table, a truncation log of log_cap records.  reward_mode, autoreset, action_mode, seed and diag stay 0 for the caller to set.
void wire(HostBatch& e, int n, const double* cfg, const double* vel, int F, double mocap_dt, int log_cap = 0) {
  e.n = n;
  e.qpos.assign((size_t)n * NQ, 0); e.qvel.assign((size_t)n * NV, 0); e.qws.assign((size_t)n * NV, 0);
  e.time.assign(n, 0); e.ctrl.assign((size_t)n * NU, 0); e.xipos.assign((size_t)n * NB * 3, 0); e.comz.assign(n, 0);
  e.cfg.assign(cfg, cfg + (size_t)F * NQ); e.vel.assign(vel, vel + (size_t)F * NV);
  e.fidx.assign(n, 0); e.finit.assign(n, 0); e.ncon.assign(n, 0); e.nefc.assign(n, 0); e.cong.assign((size_t)n * MAXEFC * 2, -1);
  e.status.assign(n, 0); e.siter.assign(n, 0); e.episode.assign(n, 0); e.cycle.assign(n, 0); e.aovf.assign((size_t)n * AOVF_COLS * 64, 0);
  e.kin.assign((size_t)n * KIN_DOUBLES, 0); e.kin_ok.assign(n, 0); e.redo.assign((size_t)n + 16, 0);
  e.steps.assign(n, 0); e.reason.assign(n, 0);
  const size_t cap = (size_t)std::max(log_cap, 1);
  e.log_count.assign(1, 0); e.log_index.assign(cap * 4, 0); e.log_qpos.assign(cap * NQ, 0); e.log_qvel.assign(cap * NV, 0);
  Batch<double>& B = e.B;
  B = Batch<double>{};
  B.qpos = e.qpos.data(); B.qvel = e.qvel.data(); B.qws = e.qws.data(); B.time = e.time.data(); B.ctrl = e.ctrl.data();
  B.xipos = e.xipos.data(); B.comz = e.comz.data(); B.frame_idx = e.fidx.data(); B.frame_init = e.finit.data();
  B.ncon = e.ncon.data(); B.nefc = e.nefc.data(); B.cong = e.cong.data(); B.status = e.status.data();
  B.aovf = e.aovf.data(); B.cycle = e.cycle.data(); B.imit_table = nullptr; B.imit_pdev = nullptr; B.order = nullptr;
  B.solver_iter = e.siter.data(); B.episode = e.episode.data(); B.mocap_cfg = e.cfg.data(); B.mocap_vel = e.vel.data();
  B.kin = e.kin.data(); B.kin_ok = e.kin_ok.data();
  B.redo_list = e.redo.data() + 16; B.redo_count = e.redo.data(); B.redo_why = e.redo.data() + 8;
  B.mocap_dt = mocap_dt; B.n_frames = F; B.n_envs = n; B.env_offset = 0;
}

// the imitation reward's table [n_frames, IMIT_FEAT] and its 32 parameters
void set_imitation(HostBatch& e, const double* table, const double* params) {
  e.imit.assign(table, table + (size_t)e.B.n_frames * IMIT_FEAT);
  e.B.imit_table = e.imit.data();
  for (int k = 0; k < 32; k++) e.B.imit_params[k] = params[k];
  e.B.imit_pdev = e.B.imit_params;
}

// dm_batch_set_state (the body of k_set_state, one environment per wave): fidx null leaves the frame cursors, mask null takes every environment
void set_state(HostBatch& e, const double* qpos, const double* qvel, const int* fidx, const unsigned char* mask) {
  std::fill(e.kin_ok.begin(), e.kin_ok.end(), 0);      // as the device entry point does: parked kinematics belong to the old positions
  for (int env = 0; env < e.n; env++) {
    if (mask && !mask[env]) continue;
    run_wave([&](int lane) {
      load_env(e.M, e.B, e.sh, env, lane, (const double*)0);
      if (lane < NQ) e.sh.qpos[lane] = qpos[(size_t)env * NQ + lane];
      if (lane < NV) e.sh.qvel[lane] = qvel[(size_t)env * NV + lane];
      if (fidx && lane == 0) set_frame(e.B, env, fidx[env]);
      dmw::sync();
      store_state(e.B, e.sh, env, lane);
      { const LaneTopo lt = lane_topo(lane); stage_tables(e.sh, lane); dmw::sync(); forward(e.M, e.sh, lane, lt, (const DebugOut*)0); }
      store_derived(e.B, e.M, e.sh, env, lane);
    });
  }
}

// One packed step launch with the device's routing (dmenv.hip step_impl): four environments per wave, then the environments beyond the packed path's
// capacities re-stepped one per wave with the one-env code.  EXT: the three-set code (DM_OPT_PACKED = 2, k_step_packed_ext) instead of the lean step
// (k_step_packed); SPD: the stable PD controller of action modes 3 and 4 compiled into both (k_step_packed_ext_spd, k_step_redo_spd).  Returns the number of
// re-steps; their ids stand in B.redo_list.
template <bool EXT, bool SPD = false>
int packed_step_launch(HostBatch& e, const double* action, double* obs, double* reward, unsigned char* done, int nsub) {
  static_assert(EXT || !SPD, "the controller comes with the three-set code");
  const int n = e.n;
  e.B.redo_count[0] = 0;
  for (int first = 0; first < n; first += SLOTS)
    run_wave([&](int lane) {
      const int slot = lane >> 4, sl = lane & 15;
      stage_slot_tables(e.tabs, lane);
      int pos = first + slot;
      const bool live = pos < n;
      if (!live) pos = n - 1;
      if constexpr (SPD) slot_env_step_impl<double, false, false, SLOT_MAXROWS, true>(e.M, e.B, e.slots[slot], e.tabs, pos, sl, lane, live, action, obs, reward, done, nsub, e.B.redo_count, e.B.redo_list);
      else if constexpr (EXT) slot_env_step<double, false, false, SLOT_MAXROWS>(e.M, e.B, e.slots[slot], e.tabs, pos, sl, lane, live, action, obs, reward, done, nsub, e.B.redo_count, e.B.redo_list);
      else slot_env_step<double>(e.M, e.B, e.slots[slot], e.tabs, pos, sl, lane, live, action, obs, reward, done, nsub, e.B.redo_count, e.B.redo_list);
    });
  for (int i = 0; i < e.B.redo_count[0]; i++) {
    const int env = e.B.redo_list[i];
    if constexpr (SPD) run_wave([&](int lane) { env_step_impl<double, 32, false, true>(e.M, e.B, e.sh, e.xs, env, lane, action, obs, reward, done, nsub); });
    else run_wave([&](int lane) { env_step<double, 32>(e.M, e.B, e.sh, e.xs, env, lane, action, obs, reward, done, nsub); });
  }
  return e.B.redo_count[0];
}

// One horizon launch without a policy (k_rollout_packed; SPD: k_rollout_packed_spd; with a SlotTermination for `term`: k_rollout_packed_term[_spd]): the table
// of per-step buffers (k_fill_rows) over action [T, n, 28], obs [T, n, 56], reward / done [T, n], then slot_rollout one wave after another.  hook(first, t)
// stands where the policy's step would, in the wave of environments first .. first + SLOTS - 1: behind step t, its in-wave re-steps and the termination phase.
// Returns the number of in-wave re-steps.
template <bool SPD, class HOOK, class TERM = NoTermination>
int horizon_launch(HostBatch& e, const double* action, double* obs, double* reward, unsigned char* done, int nsub, int T, HOOK&& hook, const TERM& term = TERM()) {
  const int n = e.n;
  std::vector<StepRow> rows((size_t)T);
  for (int t = 0; t < T; t++) rows[t] = StepRow{action + (size_t)t * n * NU, obs + (size_t)t * n * NOBS, reward + (size_t)t * n, done + (size_t)t * n};
  const int before = e.B.redo_why[0];
  for (int first = 0; first < n; first += SLOTS)
    run_wave([&](int lane) {
      const int slot = lane >> 4;
      stage_slot_tables(e.tabs, lane);
      int pos = first + slot;
      const bool live = pos < n;
      if (!live) pos = n - 1;
      slot_rollout<double, RESTEP_ROWS, SPD>(e.M, e.B, e.roll.sh, e.tabs, e.roll.one.s, e.roll.one.x, pos, lane, live, rows.data(), nsub, T, [&](int t) { hook(first, t); },
                                             (long long*)nullptr, false, TERM(term));
    });
  return e.B.redo_why[0] - before;
}
}  // namespace
