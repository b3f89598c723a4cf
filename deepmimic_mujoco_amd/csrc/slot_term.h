// slot_term.h — DeepMimic's early termination inside a horizon launch (DM_OPT_HORIZON_TERMINATION): k_terminate's rule
// (term_kernel.h) for the four-environments-per-wavefront layout, as a phase of slot_rollout's loop (slot_step.h) behind the step and its in-wave
// re-steps and ahead of the policy's step.  Used by k_rollout_packed_term (kernels_rollout_term.hip) alone: no other kernel carries this code.
#pragma once

#include "slot_step.h"
#define DM_TERM_ARGS_ONLY
#include "term_kernel.h"
#undef DM_TERM_ARGS_ONLY

namespace dm {

// Step t of the horizon has been taken and stored: row t of obs / done and the batch state are what the step (packed, or the one-env re-step) left.
// Per slot: where the step ended the episode itself, the reason and a cleared counter; otherwise the step is counted, the time limit and — with a
// fall set — the floor contacts of the state's kinematics are tested (slot lane g = geom g), and an episode that either ends gets done, the reason,
// a record in the truncation log if the time limit alone ended it, and with auto-reset the fresh episode: state, observation row t, cleared kinematics
// flags.  The reward row is left as the step wrote it; a slot that is not `live` writes nothing.
// `lds_lost` (wave-uniform): an in-wave re-step overwrote the slots' LDS since the step.  The kinematics are the slot's own where its `kin_ok` flag
// stands (the 5-term reward's pass ran on the end state: slot_env_step_impl); elsewhere one slot_kinematics pass on the stored state, for the whole wave,
// after which no slot's flag stands: kinematics formed here are used by the fall test alone, never carried into a step.
template <class R>
DM_DEV void slot_terminate(const DevModel<R>& M, const Batch<R>& B, SlotShared<R>& s, const TermArgs& T, int t, int env, int sl, int lane, bool live,
                           bool lds_lost, double* obs, unsigned char* done) {
  dmw::sync_mem();                                             // the step's rows and state, written by other lanes of this wave
  const TermVerdict v = term_verdict(done[env] != 0, T.steps[env], T.max_steps);
  const bool test = live && !v.stepdone;
  dmw::sync();                                                 // every lane has read the flag and the counter that lane 0 of the slot writes below
  if (live && v.stepdone && sl == 0) { T.reason[env] = v.reason(false); T.steps[env] = v.steps_kept(false); }
  bool fall = false;
  if (T.fall_bodies) {                                         // (wave-uniform)
    const bool own = !lds_lost && s.kin_ok() != R(0);
    if (dmw::ballot(test && !own) != 0ull) {
      if (!own) {
#pragma unroll
        for (int c = 0; c < Q_PASSES; c++) { const int i = sl + SW * c; if (i < NQ) s.qpos[i] = B.qpos[(size_t)env * NQ + i]; }
      }
      if (sl == 0) s.kin_ok() = R(0);
      dmw::sync();
      R xip[3];
      slot_kinematics(M, s, sl, lane_topo(sl), xip);           // ends with a sync
    }
    bool touch = false;
    if (sl >= 1 && sl < NG) touch = dmfc::geom_touches_floor(sl, M.geom_body, M.geom_type, M.geom_pos, M.geom_mat, M.geom_size, M.geom_margin, s.xpos, s.xmat);
    fall = (dmw::row_ballot(touch, lane) & dmfc::geoms_of_bodies(T.fall_bodies, M.geom_body, NG)) != 0u;
  }
  const bool end = live && v.ends(fall);
  if (test && !end && sl == 0) { T.steps[env] = v.steps_kept(fall); T.reason[env] = v.reason(fall); }
  if (T.log_cap > 0) {                                         // ended by the time limit alone: a truncation — log the state the step left
    const bool rec = end && !fall;
    int k = 0;
    if (rec && sl == 0) k = dmw::global_counter_next(T.log_count);
    k = dmw::row_bcast_i<0>(k);
    if (rec && k < T.log_cap) {
      if (sl < 4) T.log_index[(size_t)k * 4 + sl] = trunc_index_value(sl, env, T.tick + t, B);
#pragma unroll
      for (int c = 0; c < Q_PASSES; c++) {
        const int i = sl + SW * c;
        if (i < NQ) T.log_qpos[(size_t)k * NQ + i] = (double)B.qpos[(size_t)env * NQ + i];
        if (i < NV) T.log_qvel[(size_t)k * NV + i] = (double)B.qvel[(size_t)env * NV + i];
      }
    }
  }
  if (end && sl == 0) { done[env] = 1; T.reason[env] = v.reason(fall); T.steps[env] = v.steps_kept(fall); }
  if (B.autoreset) {                                           // the tail of the step's epilogue: the fresh episode's state and observation row
    dmw::sync_mem();
    slot_reset_env(M, B, s, env, sl, end, B.autoreset == 1 ? 0 : 1, 1);
    if (end) {
#pragma unroll
      for (int c = 0; c < (NOBS + SW - 1) / SW; c++) {
        const int o = sl + SW * c;
        if (o < NOBS) obs[(size_t)env * NOBS + o] = obs_element(s.qpos, s.qvel, o);
      }
      if (sl == 0) { if (B.kin) B.kin_ok[env] = 0; s.kin_ok() = R(0); }   // parked and carried kinematics belong to the old state
    }
    slot_store_state(B, s, env, sl, end);
  }
  dmw::sync_mem();
}

// the phase as a call (slot_step.h DM_CALL_SLOT): slot_rollout's loop keeps its register picture, the phase its own
template <class R>
DM_DEV_CALL64 void slot_terminate_call(const DevModel<R>* M, const Batch<R>* B, SlotShared<R>* s, TermArgs T, int t, int env, int sl, int lane, bool live,
                                       int lds_lost, double* obs, unsigned char* done DM_CALL_SLOT_PARAM) {
  using dmw::uniform_ptr; using dmw::in_lds; using dmw::in_global; using dmw::in_constant;
  DM_CALL_SLOT_TOUCH(env);
  const Batch<R> Bv = *in_constant(B);
  T.steps = in_global(uniform_ptr(T.steps)); T.reason = in_global(uniform_ptr(T.reason)); T.log_count = in_global(uniform_ptr(T.log_count));
  T.log_index = in_global(uniform_ptr(T.log_index)); T.log_qpos = in_global(uniform_ptr(T.log_qpos)); T.log_qvel = in_global(uniform_ptr(T.log_qvel));
  T.fall_bodies = (unsigned)dmw::uniform((int)T.fall_bodies); T.max_steps = dmw::uniform(T.max_steps); T.log_cap = dmw::uniform(T.log_cap); T.tick = dmw::uniform(T.tick);
  slot_terminate<R>(*in_constant(M), global_members(Bv), *in_lds(s), T, dmw::uniform(t), env, sl, lane, live, dmw::uniform(lds_lost) != 0,
                    in_global(uniform_ptr(obs)), in_global(uniform_ptr(done)));
}

// slot_rollout's termination switch: the phase of one wave-step
struct SlotTermination {
  static constexpr bool on = true;
  TermArgs T;
  template <class R>
  DM_DEV void operator()(const DevModel<R>* M, const Batch<R>* B, SlotShared<R>* s, int t, int env, int sl, int lane, bool live, bool lds_lost, double* obs,
                         unsigned char* done DM_CALL_SLOT_PARAM) const {
    slot_terminate_call<R>(M, B, s, T, t, env, sl, lane, live, lds_lost ? 1 : 0, obs, done
#ifdef DM_STATIC_CALLS
                           , call_slot
#endif
    );
  }
};

}  // namespace dm
