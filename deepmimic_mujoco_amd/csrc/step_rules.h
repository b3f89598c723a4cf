// step_rules.h — the rules of DPEnv.step, each stated once, for the two lane layouts that run them: one environment per wavefront (env_step.h,
// term_kernel.h) and four (slot_step.h, slot_term.h).  Layout-free: scalars and indices in, values out — no lane id, no barrier, no cross-lane
// operation, and no store but reset_commit's (which one lane calls).  The layouts own which lane holds which dof, the sums, the barriers, the
// `live` / `doit` predicates and every other store.  Cursor values (frame_idx, frame_init, cycle) arrive as arguments: the caller loads them, uniform
// per wave or per slot as its layout has it.  A floating-point formula stands here in ONE source expression where it is one: the float32 library
// fuses a product and a sum only inside an expression (csrc/build.py FLOAT32_DEFS), and both layouts must round alike.
#pragma once

#include "dmenv.h"
#include "env_kernel.h"

namespace dm {

// device pointers to the batch's state (row-major [N, width] arrays) and its configuration
template <class R>
struct Batch {
  R* qpos;      // [N,35]
  R* qvel;      // [N,34]
  R* qws;       // [N,34] qacc_warmstart
  R* time;      // [N]
  R* ctrl;      // [N,28] last raw ctrl
  R* xipos;     // [N,14,3]
  R* comz;      // [N]
  int* frame_idx;   // [N] DPEnv.idx_curr
  int* frame_init;  // [N] DPEnv.idx_init
  int* ncon;        // [N]
  int* nefc;        // [N]
  int* cong;        // [N,MAXEFC,2]
  R* aovf;          // [N, AOVF_COLS, 64] overflow columns of A for the register-tier kernel (nullptr if unused)
  int* status;      // [N]
  int* solver_iter; // [N]
  int* episode;     // [N]
  int* order;       // [N] dispatch order: workgroup w steps env order[w] (nullptr: identity) — costly envs first shortens the tail
  // self-ordering per-step launches (env_step.h dispatch_env / order_ticket): every env stepped by launch t takes a ticket in the bucket of its cost
  // key; launch t + 1 turns (bucket counts, bucket lists) into its dispatch order on the fly — no ordering kernel between two steps.
  // All null: off.  The pointers are those of ONE launch (one pipelined part, one phase): the host rotates three phases per part.
  const int* ord_in;       // [64] bucket counts the previous launch of this part left (nullptr: no order yet -> `order` / identity)
  const int* ordl_in;      // its bucket lists: env of (bucket k, ticket p) at ordl_in[k * ord_stride + p]
  int* ord_out;            // [64] bucket counters this launch's envs take their tickets from (zero when the launch starts)
  int* ordl_out;           // this launch's bucket lists
  int* ord_zero;           // [64] the counters the NEXT launch will count into: cleared by this launch's first workgroup
  int ord_stride;
  int* cycle;       // [N] completed motion cycles since the episode started (imitation reward: root advance of the reference)
  R* kin;           // [N, KIN_DOUBLES] kinematics of the state an env was left in (see save_kin), valid where kin_ok[env] != 0
  unsigned char* kin_ok;   // [N]
  int* redo_list;          // [N] envs the four-envs-per-wave kernel could not step (a capacity of slot_kernel.h exceeded): re-stepped by the one-env kernel
  int* redo_count;         // [DM_MAX_PIPELINE] one counter per pipelined sub-batch (its list starts at redo_list[first env of the sub-batch])
  int* redo_why;           // [8] diagnostic tallies of the reasons (see slot_step.h)
  const R* mocap_cfg;  // [F,35]
  const R* mocap_vel;  // [F,34]
  const R* imit_table; // [F,112] reference feature rows of the 5-term imitation reward (nullptr: not provided)
  const R* imit_pdev;  // the same 32 parameters in device memory (the reward indexes them per lane)
  R imit_params[32];   // joint weights [12], root weight, cycle shift x y, loop flag, end-effector bodies [4], offsets [4][3]
  R mocap_dt;          // duration of a mocap frame (MocapDM.dt): dp_env_v1's update interval (reward mode 4)
  int n_frames;
  int n_envs;
  int env_offset;      // global id of env 0 of this shard (multi-GPU: RNG streams do not depend on the sharding)
  int reward_mode, autoreset, action_mode;
  int diag;            // 1: k_step also stores the per-step diagnostics (xipos, contact geom list); 0: state, obs and the row counts only
  unsigned long long seed;
};

// the same batch for code behind a real call (slot_step.h): there the struct arrives through a generic pointer and so would its members
template <class R>
DM_DEV Batch<R> global_members(Batch<R> b) {
  using dmw::in_global;          // (the members are wave-uniform: loaded through a uniform pointer)
  b.qpos = in_global(b.qpos); b.qvel = in_global(b.qvel); b.qws = in_global(b.qws); b.time = in_global(b.time); b.ctrl = in_global(b.ctrl);
  b.xipos = in_global(b.xipos); b.comz = in_global(b.comz); b.frame_idx = in_global(b.frame_idx); b.frame_init = in_global(b.frame_init);
  b.ncon = in_global(b.ncon); b.nefc = in_global(b.nefc); b.cong = in_global(b.cong); b.aovf = in_global(b.aovf); b.status = in_global(b.status);
  b.solver_iter = in_global(b.solver_iter); b.episode = in_global(b.episode); b.order = in_global(b.order); b.cycle = in_global(b.cycle);
  b.kin = in_global(b.kin); b.kin_ok = in_global(b.kin_ok); b.redo_list = in_global(b.redo_list); b.redo_count = in_global(b.redo_count);
  b.redo_why = in_global(b.redo_why); b.mocap_cfg = in_global(b.mocap_cfg); b.mocap_vel = in_global(b.mocap_vel);
  b.imit_table = in_global(b.imit_table); b.imit_pdev = in_global(b.imit_pdev);
  // (the ord_* members stay as they are: code behind a call runs inside horizon launches, which take no tickets — the members are null there)
  return b;
}

// counter-based RNG: splitmix64 finaliser over (seed, global env, episode, k) -> U[0,1)
DM_DEV unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
DM_DEV double rng_uniform(unsigned long long seed, int genv, int episode, int k) {
  unsigned long long h = mix64(seed ^ mix64((unsigned long long)(unsigned)genv * 0x100000001B3ull + 0x1234567ull));
  h = mix64(h ^ ((unsigned long long)(unsigned)episode << 32 | (unsigned)k));
  return (double)(h >> 11) * (1.0 / 9007199254740992.0);
}

// ---- clip sets: K clips concatenated row-wise in the batch's three tables, one clip per env ---------------------------------------
// A rule below reads the clip through the Batch it is given: n_frames, mocap_dt, the three table pointers, imit_params[13..15].  On a single-clip batch
// that is the batch itself.  On a multi-clip batch the layouts hand the rules the env's CLIP VIEW (clip_view): the same batch with exactly those members
// replaced by the clip's own — the tables start at the clip's first row, so frame_idx / frame_init / cycle stay local to the clip.  The view is uniform
// per wave in the one-env layout and per slot in the packed one (which builds it at its uses and does not carry it across the solve).
template <class R>
struct ClipRec { int row0, n_frames; R dt, loop, shift_x, shift_y; double cdf; };   // cdf: running sum of the draw weights over their total, 1.0 for the last clip
template <class R>
DM_DEV Batch<R> clip_view(Batch<R> b, const ClipRec<R>& r) {
  b.mocap_cfg += (size_t)r.row0 * NQ; b.mocap_vel += (size_t)r.row0 * NV;
  if (b.imit_table) b.imit_table += (size_t)r.row0 * IMIT_FEAT;
  b.n_frames = r.n_frames; b.mocap_dt = r.dt;
  b.imit_params[13] = r.shift_x; b.imit_params[14] = r.shift_y; b.imit_params[15] = r.loop;
  return b;
}
// The switch the step and reset routines are instantiated with (the last template parameter; the way slot_rollout takes its termination).  NoClips — every
// kernel of a single-clip batch — hands the batch itself back by reference and compiles no trace of the clip code.
struct NoClips {
  static constexpr bool on = false;
  template <class R> DM_DEV const Batch<R>& view(const Batch<R>& B, int) const { return B; }
  template <class R> DM_DEV const Batch<R>& view_uniform(const Batch<R>& B, int) const { return B; }
};
// ... and the kernel argument of the clip forms (kernels_clips.hip, kernels_packed_clips.hip), beside the batch as PolicyArgs and TermArgs are
template <class R>
struct ClipArgs {
  static constexpr bool on = true;
  int* clip;                   // [N] DM_F_CLIP: the env's clip (stored by reset_commit's lane where DM_OPT_CLIP_MODE draws it)
  const ClipRec<R>* rec;       // [n_clips]
  int n_clips, mode;           // DM_OPT_CLIP_MODE
  DM_DEV Batch<R> view(const Batch<R>& B, int env) const { return clip_view(B, rec[clip[env]]); }
  DM_DEV Batch<R> view_uniform(const Batch<R>& B, int env) const { return clip_view(B, rec[dmw::uniform(clip[env])]); }
  // The clip of episode `ep` of env `env`.  "episode" mode draws it wherever the reset sets the frame cursor (reset_commit's condition), from stream
  // index 128 of the episode's RNG (0 is the frame, 1..35 and 64..97 the pose noise): the first clip whose cdf exceeds the draw.  Otherwise the env keeps its clip.
  DM_DEV int episode_clip(const Batch<R>& B, int env, int ep, int reset_mode, int hard) const {
    if (mode != 1 || !(reset_mode == 0 || (reset_mode == 1 && hard))) return clip[env];
    const double u = rng_uniform(B.seed, B.env_offset + env, ep, 128);
    int c = 0;
    while (c < n_clips - 1 && !(u < rec[c].cdf)) c++;
    return c;
  }
};

// ---- mocap frame cursors ---------------------------------------------------------------------------------------------------------------
// dp_env_v1's update interval (src/dp_env_v1.py:82-158): env steps per mocap frame, at least one
template <class R>
DM_DEV int v1_update_interval(const DevModel<R>& M, const Batch<R>& B, int n_substeps) {
  int upd = (int)floor(B.mocap_dt / (M.timestep * n_substeps));
  if (upd < 1) upd = 1;
  return upd;
}

// The mocap frame env `env` is at as the env step starts: what the action front ends of modes 1, 2 and 4 track.  Reward modes 0, 1 and 3 keep
// the frame itself in frame_idx.  Modes 2 and 4 keep the reference's two cursors (set_frame below): frame_idx counts steps without bound and the
// frame is looked up through frame_init, exactly as their reward epilogues do (frame_step) — mode 4 with the v1 epilogue's update interval.  Always a
// row of the mocap tables while frame_idx and frame_init are not negative.  Called inside the action-mode branches only: mode 0 pays nothing for it.
template <class R>
DM_DEV int step_start_frame(const DevModel<R>& M, const Batch<R>& B, int env, int n_substeps) {
  const int idx = B.frame_idx[env];
  if (B.reward_mode == REW_V2_POSE) return (idx + B.frame_init[env]) % B.n_frames;
  if (B.reward_mode == REW_V1_QUAT) return (idx / v1_update_interval(M, B, n_substeps) + B.frame_init[env]) % B.n_frames;
  return idx;
}

// DPEnv.reference_state_init for one env: `idx` is the drawn mocap frame.  dp_env_v3 (src/dp_env_v3.py:67-71) starts its frame
// cursor AT the drawn frame; dp_env_v2 (src/dp_env_v2.py:68-70) keeps the draw in idx_init and counts steps from 0 in idx_curr
// (its target frame is (idx_curr + idx_init) % F, :128-129); dp_env_v1 does the same (src/dp_env_v1.py:58-60,94-96).
template <class R>
DM_DEV void set_frame(const Batch<R>& B, int env, int idx) {
  B.frame_init[env] = idx;
  B.frame_idx[env] = (B.reward_mode == REW_V2_POSE || B.reward_mode == REW_V1_QUAT) ? 0 : idx;
  B.cycle[env] = 0;
}

// What the reward epilogue of `mode` (the caller's branch: a literal) does with the cursors it loaded — idx = frame_idx, init = frame_init (modes 2
// and 4), cyc = cycle (mode 3); the others are not read.  store: the frame_idx to store; row: the table row the state after the step is compared with.
//   v3-config (src/dp_env_v3.py:89-104)   compares with the frame the env is at, then advances and wraps
//   v2-pose   (src/dp_env_v2.py:116-183)  the cursor counts steps; row = (cursor + init) % F
//   imitation (code.md:1017-1143)         frame idx + 1; a looping clip wraps and counts a cycle, a "Loop: none" clip holds its last frame and ends
//   v1-quat   (src/dp_env_v1.py:82-158)   the cursor counts steps; every `upd` steps (take) the pose reward against row, with the rates of row_v
struct FrameStep { int store, row, row_v, cycle; bool ended, take; };
template <class R>
DM_DEV FrameStep frame_step(int mode, const DevModel<R>& M, const Batch<R>& B, int n_substeps, int idx, int init, int cyc) {
  FrameStep f = {idx + 1, idx, idx, cyc, false, true};
  if (mode == REW_V3_CONFIG) f.store = (idx + 1) % B.n_frames;
  else if (mode == REW_V2_POSE) f.row = (f.store + init) % B.n_frames;
  else if (mode == REW_IMITATION) {
    if (f.store >= B.n_frames) { if (B.imit_params[15] != R(0)) { f.store = 0; f.cycle += 1; } else { f.store = B.n_frames - 1; f.ended = true; } }
    f.row = f.store;
  } else if (mode == REW_V1_QUAT) {
    const int upd = v1_update_interval(M, B, n_substeps);
    f.take = f.store % upd == 0;
    f.row = (f.store / upd + init) % B.n_frames;
    f.row_v = f.row + 1 < B.n_frames ? f.row + 1 : B.n_frames - 1;
  }
  return f;
}

// ---- action front end --------------------------------------------------------------------------------------------------------------------
// Action modes 0..2: data.ctrl of actuator u from its action a and the joint's state (q_u, v_u) = (qpos[7 + u], qvel[6 + u]).
template <class R>
DM_DEV R ctrl_of_action(const DevModel<R>& M, const Batch<R>& B, int env, int u, R a, R q_u, R v_u, int n_substeps) {
  if (B.action_mode == 1) {  // P-control towards the current mocap frame (src/env_torque_test.py:14-20)
    const int idx = step_start_frame(M, B, env, n_substeps);
    a += R(0.8) * (B.mocap_cfg[(size_t)idx * NQ + 7 + u] - q_u);
  } else if (B.action_mode == 2) {  // PD torque kp*dq + kd*dv written to ctrl (src/mujoco/setting_states.py:207-226)
    const int idx = step_start_frame(M, B, env, n_substeps);
    a += M.kp[u + 6] * (B.mocap_cfg[(size_t)idx * NQ + 7 + u] - q_u) + M.kd[u + 6] * (B.mocap_vel[(size_t)idx * NV + 6 + u] - v_u);
  }
  return a;
}
// Action modes 3 and 4 (stable PD control, env_step.h spd_control): the target of actuator u — qbar = action (3) or mocap frame + action (4), vbar = 0 or
// the mocap frame's rate.  The frame is the one the env is at as the env step starts.
template <class R>
DM_DEV void spd_target(const DevModel<R>& M, const Batch<R>& B, int env, int u, const double* action, int n_substeps, R& qbar, R& vbar) {
  qbar = 0; vbar = 0;
  if (action) qbar = (R)action[(size_t)env * NU + u];
  if (B.action_mode == 4) {
    const int idx = step_start_frame(M, B, env, n_substeps);
    qbar += B.mocap_cfg[(size_t)idx * NQ + 7 + u];
    vbar = B.mocap_vel[(size_t)idx * NV + 6 + u];
  }
}
// ... and the control of dof d from the solve: tau = (p + d) - h kd a, ctrl = tau / gear (kept unclamped in B.ctrl).  The terms p = kp (qbar - q - h v) and
// d = kd (vbar - v) stay with the layouts: the one-env code forms them in two statements and adds, the packed code in one expression, and in float32 the
// two round differently (one fused multiply-add against none) — each is what its kernels have always computed.
template <class R>
DM_DEV R spd_ctrl(const DevModel<R>& M, int d, R p_plus_d, R kd, R qacc, R h) { return (p_plus_d - h * kd * qacc) / M.gear[d]; }
// actuator force of dof d: the gear times the control clamped to ctrlrange
template <class R>
DM_DEV R act_force(const DevModel<R>& M, int d, R ctrl) { return M.gear[d] * clampr(ctrl, M.ctrl_lo[d], M.ctrl_hi[d]); }

// ---- reward and done -------------------------------------------------------------------------------------------------------------------------
// sum of squares of data.ctrl (the control cost of reward modes 2 and 4, weight 0.1)
template <class R>
DM_DEV R control_cost(const Batch<R>& B, int env) {
  R acs = 0;
  for (int u = 0; u < NU; u++) { const R c = B.ctrl[(size_t)env * NU + u]; acs += c * c; }
  return acs;
}
// DPEnv.is_done (src/dp_env_v3.py:134-146): the COM height left its band
template <class R>
DM_DEV bool com_out_of_band(R z) { return (z < R(0.7)) || (z > R(2.0)); }

// element o of the observation row  qpos[7:] (+) qvel[6:]  (src/dp_env_v3.py:62-65) of the state in (qpos, qvel)
template <class R>
DM_DEV R obs_element(const R* qpos, const R* qvel, int o) { return o < 28 ? qpos[7 + o] : qvel[6 + (o - 28)]; }

// ---- reset variants (src/dp_env_v3.py:67-71,148-164).  mode 0: RSI, 1: noisy init pose, 2: qpos0 / zero velocity. -------------------------------
// `hard` = sim.reset() semantics: time = 0, qacc_warmstart = 0 (the latter is the layouts' store).
// Modes 0 and 1 with `hard` are the two episode starts of the reference's trainer: env.reset() = sim.reset() + reset_model()
// (RSI: draws the frame, copies the mocap state), optionally followed by reset_model_init() which overrides the STATE only
// (src/trpo.py:78-79) — so mode 1 draws the frame as well; the frame-indexed rewards then start from it.
// the mocap frame drawn for episode `ep` of env `env`
template <class R>
DM_DEV int reset_draw(const Batch<R>& B, int env, int ep) {
  const int idx = (int)(rng_uniform(B.seed, B.env_offset + env, ep, 0) * (double)B.n_frames);
  return idx >= B.n_frames ? B.n_frames - 1 : idx;
}
// element i (< NQ) of the fresh episode's qpos, and of its qvel where it has one (i < NV; genv = B.env_offset + env)
template <class R>
DM_DEV void reset_element(const DevModel<R>& M, const Batch<R>& B, int mode, int idx, int genv, int ep, int i, R& q, R& v) {
  if (mode == 0) {
    q = B.mocap_cfg[(size_t)idx * NQ + i];
    if (i < NV) v = B.mocap_vel[(size_t)idx * NV + i];
  } else if (mode == 1) {
    q = M.qpos0[i] + (R)((rng_uniform(B.seed, genv, ep, 1 + i) * 2.0 - 1.0) * 0.01);
    if (i < NV) v = (R)((rng_uniform(B.seed, genv, ep, 64 + i) * 2.0 - 1.0) * 0.01);
  } else {
    q = M.qpos0[i];
    v = 0;
  }
}
// one lane per reset env, behind the state's hand-off: the clock, the episode counter, the frame cursors
template <class R>
DM_DEV void reset_commit(const Batch<R>& B, int env, int ep, int mode, int hard, int idx) {
  if (hard) B.time[env] = 0;
  B.episode[env] = ep + 1;
  if (mode == 0 || (mode == 1 && hard)) set_frame(B, env, idx); else B.cycle[env] = 0;
}

// ---- early termination behind a step: k_terminate and slot_terminate ------------------------------------------------------------
// The verdict for one environment from the step's own done flag, the episode's step counter before this step (not read where the step ended the episode)
// and the step limit; `fall` is the layouts' floor test (floor_contact.h).  A step that ended the episode itself is not tested: reason DM_DONE_STEP.
struct TermVerdict {
  bool stepdone, limit;
  int steps;                                                     // the episode's steps, this one counted
  DM_DEV bool ends(bool fall) const { return !stepdone && (fall || limit); }
  DM_DEV int reason(bool fall) const { return stepdone ? DM_DONE_STEP : ((fall ? DM_DONE_FALL : 0) | (limit ? DM_DONE_TIME_LIMIT : 0)); }   // DM_F_DONE_REASON
  DM_DEV int steps_kept(bool fall) const { return (stepdone || fall || limit) ? 0 : steps; }                                                  // DM_F_EPISODE_STEPS
};
DM_DEV TermVerdict term_verdict(bool stepdone, int steps_before, int max_steps) {
  const int steps = steps_before + 1;
  return TermVerdict{stepdone, max_steps > 0 && steps >= max_steps, steps};
}
// integer j of a truncation record: {env, tick, frame_idx, frame_init}
template <class R>
DM_DEV int trunc_index_value(int j, int env, int tick, const Batch<R>& B) { return j == 0 ? env : (j == 1 ? tick : (j == 2 ? B.frame_idx[env] : B.frame_init[env])); }

}  // namespace dm
