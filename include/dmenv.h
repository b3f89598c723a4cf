/* dmenv.h — C ABI of libdmenv.so: the MI355X-native batched DeepMimic humanoid environment.
 *
 * This is the drop-in boundary for the hot path of mingfeisun/DeepMimic_mujoco.  In the reference the
 * path sits behind mujoco-py's Cython API (third-party, EXTERNAL) as used by gym's MujocoEnv and by
 * src/dp_env_v3.py; each entry point below names the reference interface it replaces.  Plain C types
 * only (no torch / numpy types); every function returns 0 on success or a negative DM_E* code, and
 * dm_last_error() returns a thread-local message.  A dm_batch is confined to one host thread and one
 * HIP stream; different batches (e.g. one per GPU) may be driven from different threads/processes.
 *
 * All per-environment state (qpos, qvel, time, qacc_warmstart, mocap frame indices) lives in device
 * memory owned by the library, as [N, 35] / [N, 34] row-major float64 arrays: one wavefront per
 * environment loads its row with one coalesced access.  Caller buffers (actions in, obs / reward /
 * done out) may be host or device memory (DM_PTR_HOST / DM_PTR_DEVICE).
 */
#ifndef DMENV_H
#define DMENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DM_ABI_VERSION 9

/* fixed sizes of the DeepMimic humanoid (dp_env_v3.xml:21-156): the kernels are specialised to this tree */
#define DM_NBODY 14
#define DM_NJNT 29
#define DM_NQ 35
#define DM_NV 34
#define DM_NU 28
#define DM_NGEOM 16
#define DM_NOBS 56
#define DM_NSTATE 171 /* DeepMimic's state features (dm_batch_state_features): 1 + 1 + 13 * 7 + 13 * 6 */
#define DM_NTERMS 28  /* the imitation reward's terms (dm_batch_imitation_terms): 5 + 5 + 1 + 13 + 4 */
#define DM_MAXPAIR 128
#define DM_MAXEFC 64   /* lanes of the per-env wavefront = stride of the per-row arrays */
#define DM_MAXROWS 63  /* constraint rows per environment held on chip (one lane each; the 64th lane carries the smooth force);
                          overflow is reported (DM_F_STATUS bit 0), not silent */

enum { DM_OK = 0, DM_EINVAL = -1, DM_EHIP = -2, DM_ENOMEM = -3, DM_EUNSUPPORTED = -4, DM_ENODEVICE = -5 };
enum { DM_PTR_HOST = 0, DM_PTR_DEVICE = 1 };

typedef struct dm_model dm_model;
typedef struct dm_mocap dm_mocap;
typedef struct dm_batch dm_batch;

/* Compiled model tables (host pointers, float64 / int32, read once by dm_model_create).
 * Replaces: mujoco_py.load_model_from_path(xml) -> PyMjModel, called from gym MujocoEnv.__init__
 * (reference call site src/dp_env_v3.py:59).  Filled by deepmimic_mujoco_amd/model.py. */
typedef struct {
  int32_t abi_version;
  int32_t nbody, njnt, nq, nv, nu, ngeom, npair, iterations;
  const int32_t* body_parentid;   /* [nbody] */
  const int32_t* body_dofnum;     /* [nbody] */
  const double* body_pos;         /* [nbody,3] */
  const double* body_ipos;        /* [nbody,3] */
  const double* body_mass;        /* [nbody] */
  const double* body_inertia;     /* [nbody,9] about COM, body axes */
  const double* body_invweight0;  /* [nbody,2] */
  const int32_t* jnt_type;        /* [njnt] 0 free, 3 hinge */
  const int32_t* jnt_bodyid;      /* [njnt] */
  const int32_t* jnt_limited;     /* [njnt] */
  const double* jnt_axis;         /* [njnt,3] */
  const double* jnt_range;        /* [njnt,2] */
  const double* dof_armature;     /* [nv] */
  const double* dof_damping;      /* [nv] */
  const double* dof_invweight0;   /* [nv] */
  const int32_t* geom_type;       /* [ngeom] mjtGeom */
  const int32_t* geom_bodyid;     /* [ngeom] */
  const int32_t* geom_condim;     /* [ngeom] */
  const double* geom_pos;         /* [ngeom,3] in body frame */
  const double* geom_mat;         /* [ngeom,9] in body frame */
  const double* geom_size;        /* [ngeom,3] */
  const double* geom_margin;      /* [ngeom] */
  const double* geom_friction;    /* [ngeom,3] */
  const int32_t* pair_geom;       /* [npair,2] candidate pairs in contact-list order, geom1 = lower type */
  const int32_t* actuator_dofid;  /* [nu] */
  const double* actuator_gear;    /* [nu] */
  const double* actuator_ctrlrange; /* [nu,2] */
  double timestep, gravity[3], tolerance, solref[2], solimp[5], meaninertia;
} dm_model_desc;

int dm_model_create(const dm_model_desc* desc, dm_model** out);
void dm_model_destroy(dm_model* m);

/* Mocap reference tables (MocapDM.data_config [F,35], .data_vel [F,34]; src/mujoco/mocap_v2.py:78-149).
 * Replaces: the Python-list lookups `self.mocap.data_config[idx]`, `.data_vel[idx]` at
 * src/dp_env_v3.py:93,150-151 — the tables become device-resident. */
int dm_mocap_create(const double* data_config, const double* data_vel, int32_t n_frames, double dt,
                    dm_mocap** out);
/* Reference feature rows of the full 5-term imitation reward (code.md:1017-1143 — the reward the reference's notes
 * specify but dp_env_v3.py:117-128 never computes): table [n_frames, 112] and params [32], both built on the host by
 * deepmimic_mujoco_amd/imitation.py (row layout documented there).  Call before dm_batch_create; enables reward mode 3. */
int dm_mocap_set_imitation(dm_mocap* mc, const double* table, int32_t n_cols, const double* params);
/* A CLIP SET: K = n_clips clips (1 <= K <= DM_MAX_CLIPS) for one batch, every environment imitating one of them (DM_F_CLIP) — DeepMimic trains one policy
 * on a set of motions and picks one as an episode starts.  The clips' data_config, data_vel and, where present, imitation tables are concatenated row-wise
 * on the device; a clip keeps its own n_frames, dt and imitation parameters 13..15 (cycle shift x, y and the loop flag).  Either every clip carries an
 * imitation table or none does, and parameters 0..12 and 16..31 (joint weights, root weight, end effectors) must be equal across the set: DM_EINVAL otherwise.
 * weights [K]: the probabilities (up to their sum) with which DM_OPT_CLIP_MODE 1 draws a clip; NULL: uniform; all >= 0 and finite, sum > 0, else DM_EINVAL.
 * The draw uses cdf[c] = (w[0] + .. + w[c]) / sum in float64, the last entry exactly 1.0.  The result goes to dm_batch_create like any other mocap handle (the clips
 * may be destroyed afterwards) and makes the batch MULTI-CLIP:
 *   - DM_F_FRAME_IDX, DM_F_FRAME_INIT and DM_F_CYCLE stay local to the env's clip; the table row is the clip's first row + the local frame.  Every rule that
 *     reads the clip reads the env's: the frame cursors of reward modes 1..4 (mode 4's update interval from the clip's own dt), the wrap with its cycle count
 *     against a "Loop: none" clip holding its last frame and ending, the root's cycle shift, the mocap frame of action modes 1, 2 and 4, the RSI draw and pose.
 *   - the default assignment is clip (env_offset + env) % K, so it does not depend on the sharding.  Setting option 100 deals it afresh EVERY time
 *     (a host copy and a wait for the stream): it overwrites an assignment written through DM_F_CLIP or drawn by DM_OPT_CLIP_MODE 1, so set the offset first.
 *   - dm_batch_step, dm_batch_step_act, dm_batch_reset, early termination and the views below run kernels of their own (one-env and DM_OPT_PACKED, where the
 *     four environments of a wavefront may follow four clips); dm_batch_rollout and DM_OPT_STEP_QUEUE issue step launches, as they do for action modes 3 and 4
 *     (DM_OPT_HORIZON_TERMINATION included); a profiled step (option 101) is DM_EUNSUPPORTED.  The packed forms keep their promise: an environment's result
 *     does not depend on its wave neighbours, so env e equals env e of a single-clip batch of its clip bit for bit (DM_OPT_PACKED 0 and 2; with 1, as rows 33..40).
 *   - dm_batch_set_state with host pointers range-checks frame_idx[e] against the clip of env e (DM_EINVAL).
 * A set of ONE clip gives a batch that behaves exactly as that clip's own (same kernels; DM_F_CLIP reads 0). */
int dm_mocap_create_set(const dm_mocap* const* clips, int32_t n_clips, const double* weights, dm_mocap** out);
void dm_mocap_destroy(dm_mocap* mc);

/* flags for dm_batch_create */
#define DM_FLAG_NO_CONTACT (1u << 0) /* BASELINE.json config 2: collision off   */
#define DM_FLAG_NO_LIMIT   (1u << 1) /* BASELINE.json config 2: joint limits off */

/* Replaces: mujoco_py.MjSim(model) (gym MujocoEnv.__init__), once per environment; here once per batch.
 * device_id: HIP device ordinal.  There is no CPU backend: no device -> DM_ENODEVICE. */
int dm_batch_create(const dm_model* m, const dm_mocap* mc, int32_t n_envs, int32_t device_id, uint32_t flags,
                    dm_batch** out);
void dm_batch_destroy(dm_batch* b);
int dm_batch_set_stream(dm_batch* b, void* hip_stream); /* default: a stream owned by the batch */

/* options */
enum {
  DM_OPT_REWARD_MODE = 1, /* 0 alive=1.0 (dp_env_v3.py:117-128, default), 1 v3-config (:89-104), 2 v2-pose (dp_env_v2.py:116-183),
                             3 imitation: pose/velocity/end-effector/root/COM terms of code.md:1017-1143 against frame idx+1,
                             4 v1-quat: dp_env_v1's reward (dp_env_v1.py:82-158: JOINT_WEIGHT-ed |quaternion difference angle| pose error,
                               L1 angular-rate and root errors, every int(mocap_dt // dt) steps, minus 0.1 sum ctrl^2) on this model's
                               hinge triples; modes 3 and 4 need dm_mocap_set_imitation() */
  DM_OPT_AUTORESET = 2,   /* 0 off (default), 1 RSI on done, 2 noisy-init on done (DummyVecEnv convention) */
  DM_OPT_ACTION_MODE = 3, /* 0 raw ctrl (dp_env_v3.py:112, default), 1 P-control 0.8*(mocap_cfg[k] - q) + action (env_torque_test.py:20),
                             2 PD kp*(mocap_cfg[k] - q) + kd*(mocap_vel[k] - v) + action (setting_states.py:207-226, gains mocap_util.py:22-24).
                             Modes 1 and 2 add their feedback term, evaluated ONCE per env step, to an action that is a motor command.
                             k, in modes 1, 2 and 4, is THE MOCAP FRAME THE ENV IS AT AS THE ENV STEP STARTS — the frame its reward mode
                             counts from: DM_F_FRAME_IDX in reward modes 0, 1 and 3; (DM_F_FRAME_IDX + DM_F_FRAME_INIT) % n_frames in mode 2
                             and (DM_F_FRAME_IDX / upd + DM_F_FRAME_INIT) % n_frames in mode 4, where DM_F_FRAME_IDX counts the episode's
                             steps without bound and upd = max(1, floor(mocap_dt / (timestep * n_substeps))) is that reward's update interval.
                             3 "spd-target": the action is a TARGET POSE qbar = action (28 absolute hinge angles, rad), target rate vbar = 0 —
                             DeepMimic's action.  4 "spd-mocap": qbar = mocap_cfg[k][7:] + action, vbar = mocap_vel[k][6:]
                             (k as above) — the stable form of mode 2.  In both a stable (implicit) PD controller
                             (cImpPDController::CalcControlForces, code.md:147-179) turns the target into ctrl at the start of EVERY simulation
                             substep, from the state (q, v) that substep starts at, and holds it through the substep; h = the timestep:
                               p = kp (qbar - q - h v),  d = kd (vbar - v)   (hinge dofs; kp, kd as in mode 2; 0 on the root dofs)
                               c = qfrc_bias - qfrc_passive,  a = (M + h diag(kd))^-1 (p + d - c)   (full 34 x 34 M; contacts ignored)
                               tau = p + d - h kd a,  ctrl = tau / gear;  actuator force = gear * clamp(ctrl, ctrlrange)
                             The target is not clamped.  DM_F_CTRL (and the control cost of reward modes 2 and 4) is the last substep's
                             unclamped ctrl.  Modes 3 and 4 run on the per-step kernels, one-env and DM_OPT_PACKED, with or without the
                             fused policy step; dm_batch_rollout and DM_OPT_STEP_QUEUE issue step launches for them (see there), unless
                             DM_OPT_HORIZON_SPD (below). */
  DM_OPT_SEED = 4,
  DM_OPT_DIAGNOSTICS = 5, /* 1 (default): every step also stores sim.data.xipos and the contact (geom1, geom2) list (DM_F_XIPOS,
                             DM_F_CONTACT_GEOMS: 848 B per env-step); 0: state, obs, reward, done and the row / contact counts only —
                             those two fields then keep the values of the last set_state / reset (DPVecEnv's default) */
  DM_OPT_PIPELINE = 6,    /* 1 (default): a step is one launch on the batch's stream.  P = 2..DM_MAX_PIPELINE: the env range is cut
                             into P contiguous sub-batches, each stepped on its own internal stream.  With DEVICE pointers a
                             sub-batch's launch of call k+1 waits only for its own launch of call k and for the caller's stream
                             at the time of the call (the inputs), so consecutive calls overlap: the next sub-batch's workgroups
                             take the wave slots freed while the previous one drains.  The outputs of such calls are complete
                             once the caller's stream has joined: dm_batch_join() (no host wait), dm_batch_sync(), or any other
                             entry point of the batch.  Results are identical for every P. */
  DM_OPT_PACKED = 7,      /* 0 (default): one environment per wavefront (k_step_narrow).  1 / 2: FOUR environments per wavefront, one 16-lane
                             DPP row each (k_step_packed, csrc/slot_kernel.h) wherever that kernel covers the call: every reward mode (0..4; mode 4,
                             v1-quat, included), with or without the fused policy step.  Per-environment
                             capacities of that path (csrc/slot_kernel.h SLOT_*): DM_PACKED_MAXROWS constraint rows inside a horizon launch
                             (dm_batch_rollout, DM_OPT_STEP_QUEUE: two full 16-row sets and a partial third — a humanoid standing on both
                             feet holds 32 contact rows plus joint limits), DM_PACKED_MAXROWS_PER_STEP in a per-step launch — unless the option
                             is 2: per-step launches then run k_step_packed_ext, the same step with the three-set code compiled in
                             (DM_PACKED_MAXROWS rows; ~8 % slower for environments that never get there: meant for populations that stand
                             on both feet) — (of them at most DM_PACKED_MAXLIMROWS joint limits), DM_PACKED_MAXCON contacts from at most DM_PACKED_MAXFRAME geom pairs,
                             DM_PACKED_MAXCAND pairs past the bounding spheres; an environment that exceeds one in some step is re-stepped
                             by the one-env code in the same call (dm_batch_redo_total counts them).  The throughput kernel from 4096 envs up
                             on one MI355X (round 6, closed loop with two pipelined sub-batches: 13.3 against 12.4 M env-steps/s at 4096 envs,
                             18.7 against 12.4 M at 6144; below — 10.3 against 10.6 M at 3072 — a per-step launch is less than one round of
                             lone waves and the one-env kernel stays ahead), while horizon launches (dm_batch_rollout, DM_OPT_STEP_QUEUE)
                             use it at any size.  Results agree with the oracle to the same 1e-9 bar and do not depend
                             on which environments share a wave; they differ from the one-env kernel's in the last bits (other
                             summation orders). */
  DM_OPT_STEP_QUEUE = 8,  /* 0 (default): every dm_batch_step call launches.  Q = 1..DM_MAX_STEP_QUEUE: dm_batch_step calls with DEVICE
                             pointers are QUEUED — nothing is launched — and run together, in call order, as one horizon launch
                             (k_rollout_packed: every wavefront steps its four environments through all queued steps at its own pace
                             instead of waiting for the slowest wave of every step) when Q calls are queued or when any other entry
                             point of the batch is called: dm_batch_join() (no host wait), dm_batch_sync(), dm_batch_get(), ...  The
                             contract is DM_OPT_PIPELINE's, extended to the inputs: the outputs of a queued call are complete once the
                             caller's stream has joined, and its action buffer must stay untouched until then.  A call one of whose four
                             buffers OVERLAPS (byte ranges, in any role) a buffer of a queued call — the same tensors step after step,
                             a view into them, a queued call's observations handed in as actions: a closed loop — first runs what is
                             queued, i.e. degenerates to one launch per call.  Results are bit-identical to unqueued DM_OPT_PACKED
                             steps.  Queuing applies where dm_batch_rollout uses one launch per horizon (DM_OPT_PACKED on, reward modes
                             0..3, action modes 0..2, constraint rows, at most two packed waves per SIMD); elsewhere — action modes 3 and
                             4 among it, unless DM_OPT_HORIZON_SPD: nothing is queued, dm_batch_queue_stats stays 0 — calls launch at once as without it.
                             dm_batch_destroy() DROPS what is still queued (the buffers belong to the caller and may be gone). */
  DM_OPT_FALL_BODIES = 9, /* DeepMimic's early termination by fall contact (--fall_contact_bodies).  A bit mask over model bodies, bit b for
                             body b = 1..13; 0 (default): off.  An environment FALLS when a geom of a body in the mask touches the floor
                             (dm_batch_floor_contacts has the rule) at the state the step left it in. */
  DM_OPT_MAX_EPISODE_STEPS = 10, /* the episode time limit (--time_end_lim_max), in env steps.  0 (default): off.  M > 0: the episode ends on its
                             M-th env step.
                             While either of the two options is non-zero, every per-step launch of dm_batch_step is followed on the same
                             stream (a pipelined part's: on that part's stream, over its env range) by one more launch, one wave per
                             environment (k_terminate).  Where the step itself reported done (COM band, end of a "Loop: none" clip) it only
                             records the reason and restarts DM_F_EPISODE_STEPS: the state may already be a fresh episode's, and a
                             reference pose of a floor clip legitimately touches the floor.  Elsewhere it counts the step, tests the state
                             the step left, and where a test fires sets done = 1 and DM_F_DONE_REASON, leaves the reward as it is, and with
                             DM_OPT_AUTORESET resets the environment exactly as the step kernels do on their own done (RSI / noisy init,
                             hard: time and warm start zeroed, the episode counter, the frame cursors and DM_F_CYCLE as there) and writes
                             the fresh episode's observation row.  Host-pointer steps copy out after this launch.  The step kernels carry
                             no termination code: with both options 0 nothing is launched and nothing changes.  Neither do the horizon
                             launch and the step queue, unless DM_OPT_HORIZON_TERMINATION: while an option is on and that one is not, dm_batch_rollout and DM_OPT_STEP_QUEUE issue step launches
                             (as for action modes 3 and 4 unless DM_OPT_HORIZON_SPD; dm_batch_queue_stats stays 0), and dm_batch_step_act and the policy rows of
                             dm_batch_rollout run as the plain step launch, the termination launch, then the launch behind dm_policy_act
                             on the returned observations (over the whole batch, after the parts of a pipelined step have joined): the
                             result of dm_batch_step followed by dm_policy_act, bit for bit. */
  DM_OPT_TRUNCATION_LOG = 11, /* the truncation log's capacity C in records.  0 (default): off; negative: DM_EINVAL.  It has an effect only while
                             DM_OPT_MAX_EPISODE_STEPS > 0.  A time limit truncates an infinite-horizon task: the state it cuts off is worth the
                             critic's value, not 0 as after a fall, and with DM_OPT_AUTORESET the termination launch overwrites that state.  With
                             C > 0 it first appends a record for every episode it ends by the time limit ALONE (DM_F_DONE_REASON exactly
                             DM_DONE_TIME_LIMIT; not where the fall test fired as well, not where the step itself reported done), with or without
                             auto-reset: an int32 row {env, tick, frame_idx, frame_init} and qpos [35] / qvel [34] (float64 in both libraries) as
                             the step left them, the cursors as the step left them too.  tick = the batch's dm_batch_step calls (the steps of a
                             dm_batch_rollout count one each) since the log was last cleared, 0 for the first.  Records beyond C are not
                             stored but still counted, so an overflow shows in the count.  The order of the records is the order in which
                             wavefronts arrived (the parts of a pipelined step share the one counter) and carries no meaning: key on
                             (tick, env).  Setting the option (again) joins the batch, waits for its stream, reallocates and clears the log and the
                             tick.  Off, the termination launch is bit for bit what it is without the option.  dm_batch_truncations reads it. */
  DM_OPT_HORIZON_TERMINATION = 12 /* 0 (default): as described under DM_OPT_MAX_EPISODE_STEPS — while early termination is on, dm_batch_rollout and
                             DM_OPT_STEP_QUEUE issue step launches, each followed by the termination launch.  1: early termination no longer keeps a
                             batch from the one-launch horizon.  Where dm_batch_rollout would use one launch per horizon without termination
                             (DM_OPT_PACKED on, action modes 0..2 — 3 and 4 with DM_OPT_HORIZON_SPD —, constraint rows, at most two packed waves per SIMD — the conditions are unchanged)
                             it does so with it, and DM_OPT_STEP_QUEUE queues again (dm_batch_queue_stats counts): the launch is a second horizon
                             kernel (k_rollout_packed_term) with the termination rule inside every wavefront's loop.  Order within a step of the
                             horizon: the step (with its in-wave re-steps), then termination on the state it left, then — dm_batch_rollout with
                             weights — the policy's step, which therefore acts on the observation of the episode termination leaves; the result is
                             that of dm_batch_step, the termination launch and dm_policy_act step after step.  done, DM_F_DONE_REASON,
                             DM_F_EPISODE_STEPS, the reset under DM_OPT_AUTORESET, the fresh observation row and the truncation log follow the
                             termination launch's rule to the letter (the step's own done only records its reason; the reward row is left alone; a
                             record for an episode the time limit ALONE ends); as for a step-launch rollout only the last step's reasons remain in
                             DM_F_DONE_REASON.  Ticks: step t of a horizon launch that starts at tick k logs with tick k + t, and the launch advances
                             the batch's tick by its T steps, so a record's tick is the step call's index since the log was cleared whichever way
                             the steps were launched.  The fall test runs on the four-per-wavefront kinematics, which differ from the termination
                             launch's in the last bits: a geom within rounding of the touch boundary may be decided differently.  Apart from that the
                             result is bit for bit the step launches' where both forms run the same step code: DM_OPT_PACKED 2, or DM_OPT_PACKED 1
                             while no environment holds 33..40 constraint rows.  An env-step at 33..40 rows stays on the packed three-set code in any
                             horizon launch while DM_OPT_PACKED 1's step launches hand it to the one-env code, whose float64 sums differ in the last
                             bits (with or without termination; measured 1e-14 on observations): done flags, reasons, counters, cursors and the
                             records' ticks and environments stay equal, float rows and state agree to rounding.  Values other than 0 and 1: DM_EINVAL.  Without early termination, and for
                             everything that is not a horizon launch (dm_batch_step unqueued, dm_batch_step_act, action modes 3 and 4 unless DM_OPT_HORIZON_SPD), the option
                             changes nothing.  Measured on an MI355X (profiles/term_horizon.md): a 128-step fused rollout 1.66x faster at 4096 envs, 1.38x at 8192. */
};
/* bits of DM_F_DONE_REASON */
#define DM_DONE_STEP 1       /* the step's own done: COM height outside (0.7, 2.0), or the end of a "Loop: none" clip */
#define DM_DONE_FALL 2       /* DM_OPT_FALL_BODIES: a masked body touches the floor */
#define DM_DONE_TIME_LIMIT 4 /* DM_OPT_MAX_EPISODE_STEPS */
/* per-environment capacities of the DM_OPT_PACKED path (= csrc/slot_kernel.h SLOT_MAXROWS, SLOT_MAXLIMROWS, SLOT_MAXCON, SLOT_MAXFRAME, SLOT_MAXCAND) */
#define DM_PACKED_MAXROWS 40
#define DM_PACKED_MAXROWS_PER_STEP 32
#define DM_PACKED_MAXLIMROWS 16
#define DM_PACKED_MAXCON 13
#define DM_PACKED_MAXFRAME 8
#define DM_PACKED_MAXCAND 32
/* What dm_batch_redo_total counts an environment past one of them under — out[k], k in this order; tests/test_gpu_slot_capacities.py depends on it:
 *   out[0]  every env-step re-stepped by the one-env code, whatever the reason (an env-step is counted here once, and once under each reason it met).
 *   out[1]  candidates: more than DM_PACKED_MAXCAND geom pairs passed the bounding spheres in some evaluation of the step.
 *   out[2]  box slots: a model with more box geoms than the packed narrow phase has staging slots for (never, for the humanoid's two feet).
 *   out[3]  contacts: more than DM_PACKED_MAXCON contacts, or contacts from more than DM_PACKED_MAXFRAME geom pairs.
 *   out[4]  rows: more than DM_PACKED_MAXROWS (per-step launches without the three-set code: DM_PACKED_MAXROWS_PER_STEP) constraint rows, or more than
 *           DM_PACKED_MAXLIMROWS joint-limit rows.
 *   out[5]  PGS test: a solver step the cost test would reject, which the packed loop does not replay. */
#define DM_MAX_STEP_QUEUE 256
#define DM_MAX_PIPELINE 8
/* DM_OPT_CLIP_MODE: an option of dm_batch_set_option like those of the enum above (whose ids end at 12), for multi-clip batches (dm_mocap_create_set).
 * 0 (default, "fixed"): an environment keeps its clip (DM_F_CLIP).  1 ("episode"): every reset that sets the frame cursor — dm_batch_reset modes 0 and
 * 1-with-hard, the auto-reset inside the step kernels, the termination launch's — first draws the episode's clip: u = the env's counter-based RNG at
 * (seed, global env, episode, index 128) (index 0 is the frame, 1..35 and 64..97 the pose noise), clip = the first c with u < cdf[c]; then the frame is
 * drawn as always, over that clip's n_frames, and DM_F_CLIP is stored with the cursors.  On a single-clip batch the option is accepted and changes
 * nothing.  Other values: DM_EINVAL. */
#define DM_OPT_CLIP_MODE 13
/* DM_OPT_HORIZON_SPD: an option of dm_batch_set_option like those of the enum above, for action modes 3 and 4 (DM_OPT_ACTION_MODE).  0 (default): as
 * described there — dm_batch_rollout and DM_OPT_STEP_QUEUE issue step launches in those modes (the fused policy step inside them), and dm_batch_queue_stats
 * stays 0.  1: action modes 3 and 4 no longer keep a batch from the one-launch horizon.  Where dm_batch_rollout would use one launch per horizon in modes
 * 0..2 (DM_OPT_PACKED on, a single-clip batch without a push schedule, constraint rows, at most two packed waves per SIMD, early termination off or
 * DM_OPT_HORIZON_TERMINATION on — the conditions are unchanged) it does so in modes 3 and 4, and DM_OPT_STEP_QUEUE queues again (dm_batch_queue_stats
 * counts): the launch is a horizon kernel with the stable PD controller inside every wavefront's loop (k_rollout_packed_spd; with early termination on and
 * DM_OPT_HORIZON_TERMINATION 1, k_rollout_packed_term_spd).  Order within a step of the horizon: at the start of every substep the control pass on the state
 * that substep starts at, then the substep; after the last substep the step's epilogue; the in-wave re-steps of environments beyond the packed capacities,
 * by the one-env code with the same controller; then — DM_OPT_HORIZON_TERMINATION — termination on the state the step left; then — dm_batch_rollout with
 * weights — the policy's step.  DM_F_CTRL is the last substep's unclamped ctrl, as after a step launch.  The result is bit for bit the step launches' where
 * both forms run the same step code: DM_OPT_PACKED 2, or DM_OPT_PACKED 1 while no environment holds 33..40 constraint rows.  An env-step at 33..40 rows stays
 * on the packed three-set code in any horizon launch while DM_OPT_PACKED 1's step launches hand it to the one-env code, whose float64 sums differ in the last
 * bits: discrete outputs stay equal, float rows and state agree to rounding (with termination, the caveat of DM_OPT_HORIZON_TERMINATION about a geom within
 * rounding of the touch boundary holds as well).  The policy rows are bit for bit those of dm_batch_step_act step after step (with early termination on:
 * of dm_batch_step, the termination launch and dm_policy_act).  A multi-clip batch and a batch with a push schedule still run step launches, with the
 * option too; in action modes 0..2 the option changes nothing: a batch that leaves it 0 never runs the second pair of horizon kernels.  Values other than
 * 0 and 1: DM_EINVAL.  Measurements: profiles/spd_horizon.md. */
#define DM_OPT_HORIZON_SPD 14
#define DM_MAX_CLIPS 32     /* clips of a clip set (dm_mocap_create_set) */
/* further option ids (diagnostics / tests; defaults are what the timed path uses):
 *   100 global id of env 0 of this batch (multi-GPU sharding: RNG streams are keyed by the global env id)
 *   101 per-stage shader-clock profile (k_step_prof + dm_batch_read_profile)
 *   102 1: register tier of 32 columns of A + memory strip (default); 0: all 64 columns in registers (k_step)
 *   103 1: force the guarded PGS re-solve path (results must not change)
 *   104 1: longest-first dispatch order from the previous step's row counts (default: per-step launches order themselves through tickets their envs take at the end of a step, horizon launches are grouped by a counting sort once per launch); 0: identity.
 *       Tickets are kept per pipelined part (DM_OPT_PIPELINE): a launch over the WHOLE batch of a batch configured with a pipeline depth above 1 (host-pointer
 *       steps, profiled steps) takes none and runs in the stored order — results never depend on the dispatch order, only the duration of such a launch does */
int dm_batch_set_option(dm_batch* b, int32_t opt, int64_t value);

/* Replaces: MujocoEnv.set_state(qpos, qvel) = sim.set_state(...) + sim.forward() (src/dp_env_v3.py:153,160):
 * qpos/qvel replaced for the masked envs (mask NULL = all), time and qacc_warmstart kept, derived
 * quantities (xipos ...) recomputed.  frame_idx may be NULL (unchanged). */
int dm_batch_set_state(dm_batch* b, const double* qpos, const double* qvel, const int32_t* frame_idx,
                       const uint8_t* mask, int32_t ptr_kind);

/* Replaces: MujocoEnv.reset() = sim.reset() + DPEnv.reset_model() (src/dp_env_v3.py:148-156), or
 * DPEnv.reset_model_init() (:158-164).  mode 0 = RSI (frame ~ U{0..F-1}), 1 = noisy init pose
 * (init_qpos/init_qvel + U(-0.01, 0.01)), both from a counter-based per-env RNG keyed by (seed, env, episode);
 * mode 2 = sim.reset() only (qpos0, zero velocity).  time and qacc_warmstart are zeroed for modes 0/1 only when
 * `hard` is nonzero (sim.reset() semantics); reset_model_init() called on its own keeps them. */
int dm_batch_reset(dm_batch* b, int32_t mode, int32_t hard, const uint8_t* mask, int32_t ptr_kind);

/* EXTERNAL PUSHES (DeepMimic's perturbations, code.md:949-952 Perturb / PerturbManager).  Additive: the ABI version stays 9 and the options enum is untouched.
 * A push is an IMPULSE p (N s, world frame) at the centre of mass xipos_b of model body b (1..13), at the state the env is in:
 *     dqvel = M(q)^-1 J_b(q)^T p
 * M is the step's own mass matrix, armature included; J_b the 3 x 34 translational Jacobian of the point xipos_b: for hinge dof d of a body on the chain
 * root -> b the column axis_world_d x (xipos_b - xpos_body(d)) (this model's joints sit at their body's frame origin), the identity columns for the root's
 * translation, xmat_root[:, k] x (xipos_b - xpos_root) for the root's rotation (body-frame angular velocity, MuJoCo's free joint), zero off the chain.
 * Only qvel changes: qpos, time, qacc_warmstart, the cursors and the parked kinematics (position-only: dm_batch_set(DM_F_QVEL) does not invalidate them
 * either) are untouched.  Contacts and joint limits are ignored by the impulse; the next step's constraint solve meets the new velocity.  A zero impulse
 * changes nothing, bit for bit.
 * A FORCE F held over an env step is applied as the single impulse F h BEFORE that step, h = timestep * n_substeps: the product F h is formed in float64
 * from the model descriptor's timestep and then converted to the library's arithmetic type.  This is the first-order splitting of MuJoCo's xfrc_applied:
 * exact for one unconstrained Euler step, not identical under RK4, whose stages would each see the force.
 *
 * dm_batch_push — the scripted form: one launch (k_push_now, one wave per env) now, on the batch's stream; runs what is queued and joins the pipelined
 * parts first.  body [N] int32, impulse [N,3] float64, mask [N] or NULL (every env).  body[e] == 0 or mask[e] == 0 leaves env e untouched, bit for bit.
 * Host pointers: a body outside 0..13 or a non-finite impulse is DM_EINVAL (nothing is launched), and the call waits for the launch.  Device arrays are not
 * read back: an out-of-range body or a non-finite impulse leaves its env untouched. */
int dm_batch_push(dm_batch* b, const int32_t* body, const double* impulse, const uint8_t* mask, int32_t ptr_kind);
/* The RANDOM SCHEDULE.  While one is set, every per-step launch of dm_batch_step — every layout (one env or four per wave), dm_batch_step_act, host or device
 * pointers, a profiled step — is PRECEDED by one launch, k_push (one wave per env), on the same stream (a pipelined part's on that part's stream over its env
 * range).  dm_batch_rollout and DM_OPT_STEP_QUEUE then issue step launches (dm_batch_queue_stats stays 0), with DM_OPT_HORIZON_TERMINATION too, as for action
 * modes 3 and 4.  Off (the default), nothing is launched and nothing changes.
 * For env e with ep = DM_F_EPISODE[e] (every reset path advances it) and u_k(j) = the env's counter-based RNG at (seed, env_offset + e, ep, 256 + 8 j + k)
 * (indices 0, 1..35, 64..97 and 128 are the resets'), on the record DM_F_PUSH_STATE[e] = {episode_seen, wait, left, body, count}:
 *   1. episode_seen != ep:  episode_seen = ep, count = 0, left = 0, wait = wait_min + min(floor(u_0(0) (wait_max - wait_min + 1)), wait_max - wait_min)
 *   2. left == 0 and wait > 0:  wait -= 1; done
 *   3. left == 0 and wait == 0:  push j = count begins: left = the same integer draw from u_1(j) over the duration range; body = the
 *      floor(u_2(j) popcount(bodies))-th set bit of `bodies`, ascending, clamped; |F| = force_min + u_3(j) (force_max - force_min); phi = 2 pi u_4(j);
 *      z = z_min + u_5(j) (z_max - z_min); F = |F| (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z), all in float64, stored in DM_F_PUSH_FORCE[e]; count += 1
 *   4. left > 0:  the impulse F h on `body` is applied; left -= 1; if that makes it 0, wait is drawn from u_0(count)
 * Steps 1, 3 and 4 may follow one another in one launch.  The streams are keyed by the global env id: sharding (option 100) does not change them. */
typedef struct {
  uint32_t bodies;                       /* bit b = 1..13, as DM_OPT_FALL_BODIES; other bits: DM_EINVAL */
  int32_t wait_min, wait_max;            /* env steps between pushes, 0 <= min <= max */
  int32_t duration_min, duration_max;    /* env steps a force is held, 1 <= min <= max */
  double force_min, force_max;           /* N, 0 <= min <= max, finite */
  double z_min, z_max;                   /* the direction's vertical component, -1 <= min <= max <= 1 (0, 0 = horizontal) */
} dm_push_desc;
/* NULL or bodies == 0: off.  Setting it (on or off) runs what is queued, joins the pipelined parts and clears every env's record to episode_seen = -1
 * (the other entries and DM_F_PUSH_FORCE to 0).  DM_EINVAL: a bound outside the ranges above. */
int dm_batch_set_push_schedule(dm_batch* b, const dm_push_desc* desc);

/* Replaces: DPEnv.step(action) (src/dp_env_v3.py:106-132) = do_simulation(action, n) [ctrl <- action; n x mj_step]
 * + _get_obs() + reward + is_done(), for every environment of the batch in one launch.
 * action [N,28], obs [N,56], reward [N] float64; done [N] uint8. */
int dm_batch_step(dm_batch* b, const double* action, double* obs, double* reward, uint8_t* done,
                  int32_t n_substeps, int32_t ptr_kind);
/* Replaces: DPEnv._get_obs() (src/dp_env_v3.py:62-65) without stepping. */
int dm_batch_get_obs(dm_batch* b, double* obs, int32_t ptr_kind);

/* state / diagnostics access.  Replaces reads and writes of sim.data.<field> (numpy views in mujoco-py). */
enum {
  DM_F_QPOS = 1,        /* double [N,35] */
  DM_F_QVEL = 2,        /* double [N,34] */
  DM_F_QACC_WARMSTART = 3, /* double [N,34] */
  DM_F_TIME = 4,        /* double [N] */
  DM_F_FRAME_IDX = 5,   /* int32 [N]  (DPEnv.idx_curr) */
  DM_F_FRAME_INIT = 6,  /* int32 [N]  (DPEnv.idx_init) */
  DM_F_XIPOS = 7,       /* double [N,14,3] body COM positions of the last forward evaluation */
  DM_F_COM_Z = 8,       /* double [N] */
  DM_F_NCON = 9,        /* int32 [N] contacts of the last forward evaluation */
  DM_F_NEFC = 10,       /* int32 [N] constraint rows */
  DM_F_CONTACT_GEOMS = 11, /* int32 [N,DM_MAXEFC,2] (geom1, geom2) per contact, -1 padded */
  DM_F_STATUS = 12,     /* int32 [N] bit0: constraint rows overflowed DM_MAXROWS, bit1: non-finite state */
  DM_F_SOLVER_ITER = 13,/* int32 [N] PGS sweeps of the last forward evaluation */
  DM_F_CTRL = 14,       /* double [N,28] last (unclamped) ctrl */
  DM_F_EPISODE = 15,    /* int32 [N] episode counter used by the reset RNG */
  DM_F_CYCLE = 16,      /* int32 [N] completed motion cycles since the episode started (reward mode 3) */
  DM_F_EPISODE_STEPS = 17, /* int32 [N] env steps since the episode began; maintained only while DM_OPT_FALL_BODIES or DM_OPT_MAX_EPISODE_STEPS
                              is on; readable and writable; dm_batch_reset zeroes it for the masked envs */
  DM_F_DONE_REASON = 18,/* int32 [N] why the LAST step ended the episode (maintained like DM_F_EPISODE_STEPS): DM_DONE_STEP, or
                           DM_DONE_FALL | DM_DONE_TIME_LIMIT (both may be set); 0 where the env is not done */
  DM_F_CLIP = 19,       /* int32 [N] the env's clip in the batch's clip set (0 on a single-clip batch).  Writable: values outside [0, n_clips) are DM_EINVAL (device
                           pointers are read back for the check).  A write leaves the cursors alone — follow it with dm_batch_reset or dm_batch_set_state —
                           except that a cursor naming a table row beyond the new clip is set to that clip's last frame (DM_F_FRAME_INIT always,
                           DM_F_FRAME_IDX in reward modes 0, 1 and 3), so that a step taken in between stays inside the clip's rows */
  DM_F_PUSH_STATE = 20, /* int32 [N,5] the push schedule's record {episode_seen, wait, left, body, count} (dm_batch_set_push_schedule); readable and writable */
  DM_F_PUSH_FORCE = 21  /* double [N,3] the force (N, world frame) of the env's current or last scheduled push; float64 in both libraries; readable and writable */
};
int dm_batch_get(dm_batch* b, int32_t field, void* out, size_t bytes, int32_t ptr_kind);
/* Read the truncation log (DM_OPT_TRUNCATION_LOG = C > 0).  Runs what is queued and joins the pipelined parts first, like dm_batch_join.  count [1]
 * receives the number of records appended since the log was last cleared — it may exceed C (overflow); index [cap,4], qpos [cap,35], qvel [cap,34]
 * (each may be NULL) receive the first min(cap, C) records, of which the first min(count, C) are valid.  With `clear` the count and the tick then start
 * again from 0, on the batch's stream.  Device pointers: stream-ordered copies, no host wait; host pointers: one wait at the end.
 * DM_EINVAL: null batch, null count, cap < 0, a bad ptr_kind, or the log is off. */
int dm_batch_truncations(dm_batch* b, int32_t* count, int32_t* index, double* qpos, double* qvel, int32_t cap, int32_t clear, int32_t ptr_kind);
int dm_batch_set(dm_batch* b, int32_t field, const void* in, size_t bytes, int32_t ptr_kind);

/* One forward evaluation (mj_forward = sim.forward()) of environment `env` with every intermediate dumped:
 * used by the parity tests to compare stage by stage with the oracle.  Layout of `out` (float64):
 *   M[34*34] | qfrc_bias[34] | qacc_smooth[34] | qacc[34] | xipos[14*3] | nefc | ncon | solver_iter |
 *   per row r < DM_MAXEFC: J[34] , then pos, margin, R, aref, b, force   (DM_DEBUG_DOUBLES in total) */
#define DM_DEBUG_DOUBLES (34 * 34 + 34 * 3 + 42 + 3 + DM_MAXEFC * (34 + 6))
int dm_batch_debug_forward(dm_batch* b, int32_t env, double* out_host);

/* Replaces: mujoco-py `sim.render(w, h, camera_name=, depth=)` / `MjViewer.render` behind gym `MujocoEnv.render`
 * (src/trpo.py:421, src/mujoco/mocap_v2.py:161-178): ray-cast images of n environment states.
 * The scene is the model's 16 geoms at the frames forward kinematics gives (the floor plane z = 0, visible from above, finite at
 * |x|, |y| <= its size; spheres, capsules, boxes), each view alone.  Pinhole camera, vertical `fovy` in degrees; cam_mat is
 * row-major like MuJoCo's cam_xmat: its columns are the camera's x (right), y (up) and z (backward) axes, and it looks along -z.
 * With track_com, cam_pos is an offset from the root's subtree centre of mass at each view's qpos.  Pixel (r, c), row 0 at the top:
 *   u = (2 (c + 0.5) / W - 1) tan(fovy / 2) W / H,   v = (1 - 2 (r + 0.5) / H) tan(fovy / 2),   d = normalize(u x + v y - z).
 * Shading: c = clamp(albedo (ambient + headlight max(0, -n.d) + diffuse vis max(0, -n.l)), 0, 1), byte = floor(255 c + 0.5), with
 * l = normalize(light_dir) and vis = 0 where a ray from the hit point (offset 1e-4 along n) towards -l meets a body geom.  The floor's
 * albedo is a checker of squares of `floor_square` metres (floor_rgb1 where floor(x / sq) + floor(y / sq) is even); a pixel that
 * hits nothing takes the unlit skybox sky_bottom + (1 + d_z) / 2 (sky_top - sky_bottom).  geom_rgb[0] is unused. */
typedef struct {
  int32_t width, height;            /* 1 .. 4096 each */
  int32_t track_com;                /* cam_pos is an offset from the humanoid's centre of mass */
  double cam_pos[3], cam_mat[9], fovy;
  double geom_rgb[DM_NGEOM][3], floor_rgb1[3], floor_rgb2[3], floor_square;
  double sky_top[3], sky_bottom[3], light_dir[3], ambient, headlight, diffuse;
} dm_render_desc;
/* qpos == NULL: the batch's current states of env_ids[0..n) (env_ids NULL: envs 0..n-1, n <= the batch size).  qpos [n,35] non-NULL:
 * those poses, rendered with the batch's model on its stream (mocap playback, recorded trajectories); env_ids must then be NULL.
 * Outputs (each may be NULL, at least one given): rgb [n,H,W,3] uint8, depth [n,H,W] float32 (distance along the optical axis, +inf
 * where nothing is hit), seg [n,H,W] int32 (geom id: 0 the floor, 1..15 body geoms, -1 nothing), geom_xform [n,16,12] float64 (each
 * geom's world position, then its row-major rotation).  ptr_kind applies to every array, qpos and env_ids included: host outputs
 * are written when the call returns; device outputs are valid once the caller's stream has joined, like a step's (device env_ids
 * are read back to the host to be checked).  Queued steps run and pipelined sub-batches join first, so an image shows the latest
 * step; no simulation state changes.  DM_EINVAL: n <= 0, n beyond the batch without qpos, an env id out of range, a size outside
 * 1..4096, n W H >= 2^31, fovy outside (0, 180), no output. */
int dm_batch_render(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, const dm_render_desc* d, uint8_t* rgb,
                    float* depth, int32_t* seg, double* geom_xform, int32_t ptr_kind);

/* DeepMimic's state features of n humanoid states (cCtController::BuildStatePose / BuildStateVel, code.md:307-489):
 * the observation the imitation task was designed around — where dm_batch_step's 56 numbers (hinge angles and rates) carry neither the
 * root's height or orientation, nor the bodies' positions, nor the position in the clip.  out [n, DM_NSTATE] float64, one row per state.
 * Coordinates are the model's (z up, x forward); bodies are model bodies b = 1..13 in model order (the root first), k = b - 1:
 *   [0]                 phase in [0, 1)
 *   [1]                 root height: z of the root body's frame origin (xpos[1][2] = qpos[2])
 *   [2 + 7k .. +3]      Rz(-hd) (xipos_b - xpos_root): the body's centre of mass relative to the root's frame origin, in the heading frame
 *                       (the root's own entry is its centre-of-mass offset, not a special case)
 *   [2 + 7k + 3 .. +4]  q_z(-hd) (x) xquat_b as (w, x, y, z), negated as a whole when w < 0 (code.md:406-412)
 *   [93 + 6k .. +3]     Rz(-hd) v_b, v_b the world velocity of the point xipos_b
 *   [93 + 6k + 3 .. +3] Rz(-hd) w_b, w_b the body's world angular velocity
 * Heading: hd = atan2(f_y, f_x) with f the root's x axis in the world (the root quaternion is normalised first) — the heading of the
 * imitation reward's end-effector features.  qvel[0:3] is the world velocity of the root's frame origin, qvel[3:6] the root's angular
 * velocity in its own frame (MuJoCo's free joint).  Upstream's defaults otherwise: no flip_stance, mRecordWorldRootPos / Rot off.
 * The sign rule is discontinuous where the heading-frame quaternion's w crosses 0.
 * qpos == NULL: the batch's current states of env_ids[0..n) (env_ids NULL: envs 0..n-1, n <= the batch size); the phase comes from the
 * batch's cursor fields: frame_idx / n_frames in reward modes 0, 1 and 3 (mode 0 never advances the cursor: the phase stays the RSI
 * draw), ((frame_idx + frame_init) mod n_frames) / n_frames in modes 2 and 4.  In mode 4 that is the STEP cursor: it is the mocap frame
 * only when one env step spans one mocap frame.  qpos [n,35] non-NULL: explicit states — qvel [n,34] and phase [n] must be given too, and
 * env_ids must be NULL (mocap frames, recorded trajectories).
 * One launch on the batch's stream; ptr_kind applies to every array.  Device arrays are stream-ordered with no host wait, except env_ids:
 * device env_ids are read back and range-checked on the host first (one copy and a wait for the stream), as dm_batch_render does.  Queued steps run and pipelined sub-batches join first, so the
 * features are those of the latest step (after an auto-reset: of the fresh episode's state, like a step's observation).  Read-only: the
 * call reads qpos, qvel, the two cursor fields and the reward mode and changes no batch state.  DM_EINVAL: n <= 0, n beyond the batch
 * without qpos, an env id out of range, a partial explicit state, env_ids with an explicit state, a bad ptr_kind.
 * On a multi-clip batch (dm_mocap_create_set) n_frames is the length of the env's clip. */
int dm_batch_state_features(dm_batch* b, const double* qpos, const double* qvel, const double* phase, const int32_t* env_ids, int32_t n,
                            double* out, int32_t ptr_kind);

/* Which geoms touch the floor at n humanoid states: bit g of out[i] (g = 1..15) is set exactly when the collision
 * stage of a step would emit at least one contact for the pair (floor geom 0, geom g) at state i — with the floor's frame (point p0,
 * normal n) and the pair margin max(margin_0, margin_g): a sphere (centre c, radius r) when n.(c - p0) <= margin + r; a capsule when that
 * holds for either end's centre p +- axis * half; a box when some corner has ld = n.corner <= 0 and n.(p - p0) + ld <= margin.  The fall
 * test of DM_OPT_FALL_BODIES is this mask against the geoms of the masked bodies.
 * qpos == NULL: the batch's current states of env_ids[0..n) (env_ids NULL: envs 0..n-1, n <= the batch size).  qpos [n,35] non-NULL:
 * explicit states; env_ids must then be NULL.  out [n] int32.  One launch on the batch's stream, one wave per state; argument checks,
 * stream ordering, settle-first behaviour and ptr_kind as for dm_batch_state_features.  Read-only: changes no batch state. */
int dm_batch_floor_contacts(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, int32_t* out, int32_t ptr_kind);

/* The five terms of reward mode 3 at n humanoid states: what dm_batch_step adds up and returns as one number,
 *   r = 0.5 e^(-2 pose) + 0.05 e^(-0.1 vel) + 0.15 e^(-40 eff) + 0.2 e^(-5 root) + 0.1 e^(-10 com),
 * taken apart.  out [n, DM_NTERMS] float64, one row per state, each state compared with one row of the mocap's imitation table:
 *   [0..5)    the errors e_k: pose sum_j w_j theta_j^2, velocity sum_j w_j |dw_j|^2, end effector sum_e |dp_e|^2 / 4,
 *             root |dp|^2 + 0.1 theta_root^2 + 0.01 |dv|^2 + 0.001 |dw|^2, centre of mass 0.1 |dv_com|^2
 *   [5..10)   the weighted terms w_k exp(-s_k e_k), w = (0.5, 0.05, 0.15, 0.2, 0.1), s = (2, 0.1, 40, 5, 10)
 *   [10]      their sum: the reward of mode 3
 *   [11..24)  each joint group's share w_j theta_j^2 of the pose error, in the weight-slot order of the parameter block: the 12 joint
 *             groups in model body order, then the root (slot 12); they sum to [0]
 *   [24..28)  each end effector's squared distance |dp_e|^2 to the reference's, in the parameter block's order; their sum / 4 is [2]
 * The arithmetic is the library's (float64, or float32 in libdmenv32.so) and the step kernels' own lane code; a caller re-weights the reward
 * from [0..5) alone.
 * qpos [n,35] non-NULL: explicit states — qvel [n,34] and frame [n] (the table row each state is compared with) must be given too,
 * cycle [n] may be (NULL: 0; the reference's root is shifted by cycle completed cycles), and env_ids must be NULL.  Works in any reward
 * mode.  Host-pointer frames outside [0, n_frames) are DM_EINVAL; device-pointer frames are not read back: such a row is written as
 * DM_NTERMS NaNs and the table is not read out of range.
 * qpos == NULL (qvel, frame and cycle must then be NULL too): the batch's current states and cursors (frame_idx, cycle) of
 * env_ids[0..n) (env_ids NULL: envs 0..n-1, n <= the batch size).  Reward mode 3 only (DM_EINVAL otherwise): only there do the cursors name
 * the row the last step compared the state with, so that right after a step [10] is the reward that step returned — except for an
 * environment the step reset (done with DM_OPT_AUTORESET on): its state and cursors are the fresh episode's, like its observation, and
 * its row is that state against the frame it was drawn at.
 * One launch on the batch's stream, one wave per state; argument checks, stream ordering (device env_ids are read back and
 * range-checked, nothing else waits), settle-first behaviour and ptr_kind as for dm_batch_state_features.  Read-only: changes no batch
 * state.  DM_EINVAL also when the mocap has no imitation table (dm_mocap_set_imitation was not called) and for a partial explicit state.
 * On a multi-clip batch (dm_mocap_create_set) a state is compared with the clip of env env_ids[i] (or i): explicit state i with the clip of env i (n <= the
 * batch size), its frame local to that clip and range-checked against that clip's n_frames. */
int dm_batch_imitation_terms(dm_batch* b, const double* qpos, const double* qvel, const int32_t* frame, const int32_t* cycle,
                             const int32_t* env_ids, int32_t n, double* out /* [n, DM_NTERMS] */, int32_t ptr_kind);

/* kernel timing of the last dm_batch_step launch, measured with HIP events on the batch's stream (ms) */
int dm_batch_last_step_ms(dm_batch* b, float* ms);
int dm_batch_enable_timing(dm_batch* b, int32_t on);

/* diagnostic: per-env shader-clock cycles of the last step by stage (enable with dm_batch_set_option(b, 101, 1)):
 * out [N,32] int64 = kinematics, mass matrix+factor, bias, rows(collision), constraint, whole step, nefc, PGS sweeps;
 * [8..13] the constraint stage's parts (smooth solve, J rows, impedance + half solve, A, warm start + PGS, assembly);
 * [16] geom poses + limit rows, [17,18,19] / [20,21,22] broad phase, narrow phase, row emission of pair pass 0 / 1, [23] tail,
 * [24,25] evaluations in which a pair of pass 0 / 1 passed the bounding spheres, [26,27] such pairs (summed over the step) */
int dm_batch_read_profile(dm_batch* b, long long* out_host);

/* Replaces: MlpPolicy.act(stochastic, ob) (src/mlp_policy_trpo.py:63-65; network :35-58, DiagGaussianPd src/distributions.py:220-245)
 * for a whole batch in one launch: obz = clip((ob - mean) / std, +-5), policy and value 2x100 tanh MLPs, Gaussian sample.
 * All pointers are DEVICE pointers on the current HIP device; `weights` is the packed float32 parameter block
 * (dm_policy_weight_count() floats; layout in csrc/policy_kernel.h, filled by deepmimic_mujoco_amd/policy.py MlpPolicy.pack).
 * Noise is a counter-based stream keyed by (seed, counter, env, action): pass a fresh `counter` per call.  dm_policy_act reads `weights`
 * element by element: it asks for no alignment beyond a float's (dm_batch_step_act / dm_batch_rollout below do). */
int dm_policy_weight_count(void);
int dm_policy_act(const float* weights, const double* obs, double* action, float* vpred, int32_t n, int32_t stochastic,
                  uint64_t seed, uint64_t counter, void* hip_stream);

/* dm_batch_step followed, INSIDE the step kernel, by dm_policy_act on the observations it produced: the wave that steps env e writes
 * obs / reward / done as dm_batch_step does and then next_action[e] (28) and next_vpred[e] for that observation (the fresh episode's
 * after an auto-reset).  One launch per rollout step (src/trpo.py:47-66: `ac, vpred = pi.act(ob)`; `ob, rew, new, _ = env.step(ac)`),
 * so consecutive steps of a pipelined batch (DM_OPT_PIPELINE) overlap although every step's action depends on the last one's
 * observation: that dependency stays inside a sub-batch's stream.  Device pointers only; same noise stream as dm_policy_act.  `weights` must
 * be 16-byte aligned (the in-wave policy step loads it as float4s): DM_EINVAL otherwise, before anything is launched. */
int dm_batch_step_act(dm_batch* b, const double* action, double* obs, double* reward, uint8_t* done, int32_t n_substeps,
                      const float* weights, double* next_action, float* next_vpred, int32_t stochastic, uint64_t seed, uint64_t counter);

/* T steps per call — the loop body of traj_segment_generator (src/trpo.py:47-80: `ac, vpred = pi.act(stochastic, ob)`;
 * `ob, rew, new, _ = env.step(ac)`; on `new` the reset of :77-79 through DM_OPT_AUTORESET) for a whole horizon.  Device pointers only.
 *   action [T + 1, N, 28] f64: row t is consumed by step t; with `weights` rows 1..T are WRITTEN (the policy's action for the observation
 *                              of step t - 1: row 0 is the caller's, row T belongs to the next horizon); without, rows 0..T-1 are read only
 *   obs [T, N, 56] f64, reward [T, N] f64, done [T, N] u8: row t = what dm_batch_step returns for step t
 *   vpred [T, N] f32 (with `weights`): row t = the value of obs row t;  counter: the draw counter of step 0 (step t uses counter + t)
 * Results are those of T dm_batch_step / dm_batch_step_act calls.  With DM_OPT_PACKED (a reward mode that kernel covers, a model with
 * constraint rows, at most two packed waves per SIMD = 8 192 environments on an MI355X; DM option 106 = 1 / 0 forces / forbids it) the
 * horizon is ONE launch: every wavefront steps its four environments T times at its own pace, so the horizon lasts as long as the slowest
 * wave's sum over T steps instead of the sum of every step's slowest wave (4 096 envs: 17.3 M env-steps/s against 12.2 M through
 * dm_batch_step); an environment that exceeds the packed path's capacities in some step is re-stepped inside its wave by the one-env code.
 * Otherwise — in action modes 3 and 4 unless DM_OPT_HORIZON_SPD, whose horizon kernels carry the controller — T step launches are issued: the results are those
 * of T dm_batch_step / dm_batch_step_act calls, bit for bit.  `weights`, when given, must be 16-byte aligned (DM_EINVAL otherwise). */
int dm_batch_rollout(dm_batch* b, double* action, double* obs, double* reward, uint8_t* done, int32_t T, int32_t n_substeps,
                     const float* weights, float* vpred, int32_t stochastic, uint64_t seed, uint64_t counter);

/* Replaces: add_vtarg_and_adv (src/trpo.py:83-94) for N environments at once: rew, vpred, adv, tdlamret [T, N] float32,
 * isnew [T, N] int32 (isnew[t] = the observation of step t starts an episode), nextvpred [N]; device pointers. */
int dm_gae(const float* rew, const float* vpred, const int32_t* isnew, const float* nextvpred, float* adv, float* tdlamret,
           int32_t T, int32_t n, double gamma, double lam, void* hip_stream);
/* The same with a bootstrap value per row (the time limit as a truncation: DM_OPT_TRUNCATION_LOG): vboot [T, N] float32, vboot[t] = the value of the
 * state step t left where its episode was truncated there, 0 everywhere else.  The one-step target gains one term,
 *   delta[t] = rew[t] + gamma * (vpred[t+1] * (1 - isnew[t+1]) + vboot[t]) - vpred[t],
 * and the chain still cuts where isnew[t+1] = 1.  With vboot all zeros the outputs are dm_gae's bit for bit. */
int dm_gae_boot(const float* rew, const float* vpred, const int32_t* isnew, const float* nextvpred, const float* vboot, float* adv, float* tdlamret,
                int32_t T, int32_t n, double gamma, double lam, void* hip_stream);

/* Replaces: the episode bookkeeping of the generator's loop (src/trpo.py:68-79) over a [T, N] segment that dm_batch_rollout / T dm_batch_step
 * calls wrote (reward f64, done u8).  cur_ret [N] f64 / cur_len [N] i64: return and length of every environment's open episode, read and
 * updated.  Every episode that ends inside the segment appends a record of three int64 words to `records` [cap][3] — {t << 32 | env, the
 * float64 return's bits, length} — in arrival order (*count = number of episodes, which may exceed cap: the rest is dropped); sorted by the
 * first word they are in the order a one-env loop appends them (t, then env).  Device pointers; returns are float64 sums in step order. */
int dm_episode_scan(const double* reward, const uint8_t* done, int32_t T, int32_t n, double* cur_ret, int64_t* cur_len, int32_t* count,
                    int32_t cap, int64_t* records, void* hip_stream);

/* Replaces: one epoch of the value fit of src/trpo.py:288-296 — for each of `nb` minibatches of `bs` samples (already shuffled:
 * ob [nb*bs, 56] float32, ret [nb*bs] float32): `pi.ob_rms.update(mbob)` (src/utils/misc_util.py:53-70: rms_sum / rms_sumsq [56] and
 * rms_count float64, rms_mean / rms_std [56] float32 refreshed), the gradient of mean((vpred - ret)^2) w.r.t. the 56-100-100-1 tanh
 * value net (theta: dm_vf_param_count() floats = vffc1/w, vffc1/b, vffc2/w, vffc2/b, vffinal/w, vffinal/b, weights row-major
 * [in][out]) and the MpiAdam step (src/mpi_adam.py:21-35) with the caller's per-step scale a_i = stepsize sqrt(1 - b2^t) / (1 - b1^t)
 * (step_scale_host: HOST array [nb]).  All of it enqueued by this one call; device pointers otherwise; `scratch`:
 * dm_vf_scratch_bytes(nb, bs) bytes on the device.  epoch_filter = 1: the filter's sums of all nb minibatches are taken up front (two
 * launches) and two launches per minibatch remain (gradient partials; reduction + Adam); 0: three launches per minibatch.  Same arithmetic
 * in the same order either way: bit-identical results.  theta must be 16-byte aligned (the kernels stage it with float4 loads): DM_EINVAL
 * otherwise, before anything is launched. */
int dm_vf_param_count(void);
size_t dm_vf_scratch_bytes(int32_t nb, int32_t bs);
int dm_vf_fit_epoch(const float* ob, const float* ret, int32_t nb, int32_t bs, float* theta, float* adam_m, float* adam_v,
                    const float* step_scale_host, double beta1, double beta2, double eps, double* rms_sum, double* rms_sumsq,
                    double* rms_count, float* rms_mean, float* rms_std, void* scratch, void* hip_stream, int32_t epoch_filter);

/* Replaces: `pi.ob_rms.update(ob)` of src/trpo.py:242 with the whole batch (RunningMeanStd.update, src/utils/misc_util.py:47-70) in one launch:
 * column sums / sums of squares of ob [n, 56] float32 in float64 (fixed order), added to the filter's state; mean / std (float32, the
 * variance floored at 1e-2) refreshed.  Device pointers; `scratch`: dm_rms_scratch_bytes() bytes on the device. */
size_t dm_rms_scratch_bytes(void);
int dm_rms_update(const float* ob, int32_t n, double* rms_sum, double* rms_sumsq, double* rms_count, float* rms_mean, float* rms_std,
                  void* scratch, void* hip_stream);

/* Replaces: the policy half of one TRPO update (src/trpo.py:228-230, 245-283) for the 56-100-100-28 tanh Gaussian policy of
 * src/mlp_policy_trpo.py:50-60.  theta: dm_pg_param_count() floats = polfc1/w, polfc1/b, polfc2/w, polfc2/b, polfinal/w, polfinal/b, logstd
 * (weights row-major [in][out]: the learner's flat `var_list` order, :139); ob [n, 56] float32 raw observations, normalised inside with
 * rms_mean / rms_std [56] and clipped to +-5; everything is a device pointer; `scratch`: dm_pg_scratch_bytes() bytes on the device.
 *   dm_pg_losses  `compute_losses` / `compute_lossandgrad` (:224-226): out_losses[2] (float64) = {surrgain = mean(pnew / pold * atarg),
 *                 meankl = mean KL(old || new)}; with_grad: out_grad = flat gradient of optimgain = surrgain + entcoeff * mean entropy.
 *                 write_old != 0: old == new, and old_mean [n, 28] is WRITTEN (`assign_old_eq_new`, :247); else it is read, with old_logstd [28].
 *   dm_pg_fvp     `compute_fvp` (:228-230) on the samples ob[i * stride], i < n (`fvpargs = arr[::5]`, :245): out_fv = Hessian of the mean KL
 *                 at new == old times v — exactly J^T diag(1 / sigma^2) J v / n on the mean parameters and 2 v on logstd (pg_kernel.h); the
 *                 caller adds cg_damping * v (:229).  One forward-mode and one reverse pass per sample, no second-order graph.
 * Both run one workgroup per CU (their LDS fills it); max_blocks > 0 caps the grid, which leaves the other CUs to a kernel of another stream
 * (the learner runs the value fit beside the policy step that way).  Sums are taken in block order: the result is a function of the grid
 * size, not of timing.  max_blocks = 0: every CU.  Both refuse a theta that is not 16-byte aligned (float4 loads) with DM_EINVAL, before anything
 * is launched. */
int dm_pg_param_count(void);
size_t dm_pg_scratch_bytes(void);
int dm_pg_losses(const float* ob, int32_t n, const float* ac, const float* atarg, float* old_mean, const float* old_logstd, int32_t write_old,
                 const float* theta, const float* rms_mean, const float* rms_std, double entcoeff, int32_t with_grad,
                 float* out_grad, double* out_losses, void* scratch, void* hip_stream, int32_t max_blocks);
int dm_pg_fvp(const float* ob, int32_t stride, int32_t n, const float* theta, const float* v, const float* rms_mean, const float* rms_std,
              float* out_fv, void* scratch, void* hip_stream, int32_t max_blocks);

/* The GAIL discriminator (src/adversary.py TransitionClassifier, driven by src/gail.py) on the device, fp32 like the reference:
 * logit = fc(100->1)(tanh fc(100->100)(tanh fc(84->100)(concat((ob - rms_mean) / rms_std, ac)))), no clip of the normalised observation.
 * theta: dm_disc_param_count() = 18 701 floats = adversary/fully_connected/{weights,biases}, fully_connected_1/..., fully_connected_2/...
 * (weights row-major [in][out]), 16-byte aligned; rms_mean / rms_std [56] float32 (the adversary's own obs filter).  Every pointer is a
 * DEVICE pointer on one device; the work is enqueued on `hip_stream`; no device visible -> DM_ENODEVICE.
 *   dm_disc_reward    Replaces: reward_giver.get_reward(ob, ac) (src/gail.py:78, once per env step there) for a whole segment in one launch:
 *                     ob [n, 56], ac [n, 28] float64 (the rollout's buffers), reward [n] float64 = -log(1 - sigmoid(logit) + 1e-8) in fp32.
 *   dm_disc_lossgrad  Replaces: reward_giver.lossandgrad(ob, ac, ob_expert, ac_expert) (src/gail.py:336): generator rows g_ob [n_g, 56] /
 *                     g_ac [n_g, 28] and expert rows e_ob [n_e, 56] / e_ac [n_e, 28], float32.  out_grad [18 701] float32 = flat gradient of
 *                     mean_g CE(x, 0) + mean_e CE(x, 1) - entcoeff * mean H(x); out_losses [6] float64 = generator_loss, expert_loss, entropy,
 *                     entropy_loss, generator_acc, expert_acc.  scratch: dm_disc_scratch_bytes(n_g, n_e) bytes.  Sums are taken in a fixed
 *                     order: two calls with the same inputs give bitwise-identical results. */
int dm_disc_param_count(void);
size_t dm_disc_scratch_bytes(int32_t n_g, int32_t n_e);
int dm_disc_reward(const float* theta, const float* rms_mean, const float* rms_std, const double* ob, const double* ac, int32_t n, double* reward,
                   void* hip_stream);
int dm_disc_lossgrad(const float* theta, const float* rms_mean, const float* rms_std, const float* g_ob, const float* g_ac, int32_t n_g,
                     const float* e_ob, const float* e_ac, int32_t n_e, double entcoeff, float* out_grad, double* out_losses, void* scratch,
                     size_t scratch_bytes, void* hip_stream);

/* Behaviour cloning of the policy on expert transitions: the `behavior_clone.learn(pi, dataset, max_iters=BC_max_iter)` that src/gail.py:490-495
 * calls for --pretrained (OpenAI baselines' GAIL; the module is not in the reference's tree).  loss = mean over n rows x 28 of (x - pi.ac)^2
 * with the stochastic action pi.ac = mean + exp(logstd) eps, eps = the policy's counter noise normal_from(seed, counter, s * 28 + a) (s: the
 * row's position in the batch; stochastic = 0: eps = 0, the mode).  theta: the policy's dm_pg_param_count() floats (dm_pg_* order), 16-byte
 * aligned; rms_mean / rms_std [56]: the policy's obs filter, read and never updated.  ob_all [N, 56] / ac_all [N, 28] float32: the expert's
 * transitions; rows are gathered by idx.  idx is NOT checked: every entry must lie in 0 .. N - 1 (a null idx takes rows 0 .. n - 1, resp.
 * 0 .. bs - 1 every iteration).  Every pointer but step_scale_host is a DEVICE pointer on one device; the work is enqueued on `hip_stream`;
 * no device visible -> DM_ENODEVICE.  Sums are taken in a fixed order: two calls with the same inputs give bitwise-identical results.
 *   dm_bc_scratch_bytes  scratch both calls need for a batch of bs rows (0 for bs < 1).
 *   dm_bc_lossgrad       Replaces: `lossandgrad(ob, ac, True)` of one BC iteration: out_loss [1] float64 and, unless out_grad is null,
 *                        out_grad [dm_pg_param_count()] float32 = the flat gradient of the loss (logstd included; the value net's is zero).
 *   dm_bc_fit            Replaces: `iters` iterations of `lossandgrad` + `adam.update(g, optim_stepsize)` (MpiAdam(epsilon=adam_epsilon), one
 *                        process): iteration i takes rows idx[i * bs .. (i + 1) * bs) and counter0 + i, and steps theta, adam_m, adam_v
 *                        [dm_pg_param_count()] in place with the Adam rule of dm_vf_fit_epoch (step_scale_host [iters] on the HOST:
 *                        a_t = stepsize sqrt(1 - beta2^t) / (1 - beta1^t)); out_loss [iters] float64 = each iteration's loss before its step.
 *                        Two launches per iteration, nothing comes back to the host. */
size_t dm_bc_scratch_bytes(int32_t bs);
int dm_bc_lossgrad(const float* ob_all, const float* ac_all, const int32_t* idx, int32_t n, const float* theta, const float* rms_mean,
                   const float* rms_std, int32_t stochastic, uint64_t seed, uint64_t counter, float* out_grad, double* out_loss, void* scratch,
                   size_t scratch_bytes, void* hip_stream);
int dm_bc_fit(const float* ob_all, const float* ac_all, const int32_t* idx, int32_t iters, int32_t bs, float* theta, float* adam_m, float* adam_v,
              const float* step_scale_host, double beta1, double beta2, double eps, const float* rms_mean, const float* rms_std, int32_t stochastic,
              uint64_t seed, uint64_t counter0, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream);

/* PPO's clipped-surrogate update (OpenAI baselines' ppo1 `pposgd_simple.learn`, whose policy file the reference trains: src/mlp_policy_trpo.py;
 * the reference's --algo ppo, src/gail.py:394) for the 56-100-100-28 policy and the 56-100-100-1 value net of src/mlp_policy_trpo.py together.
 * theta (and adam_m / adam_v): [dm_pg_param_count() + dm_vf_param_count()] float32 = the policy's dm_pg_* flat order, then the value net's
 * dm_vf_* order (vffc1/w, vffc1/b, vffc2/w, vffc2/b, vffinal/w, vffinal/b), 16-byte aligned.  The segment's rows: ob_all [N, 56],
 * ac_all [N, 28], atarg_all [N] (already normalised: (adv - mean) / std), old_mean_all [N, 28] (the old policy's means, e.g. written by
 * dm_pg_losses with write_old = 1), ret_all [N] (tdlamret), old_logstd [28]; all float32.  Rows are gathered by idx, which is NOT checked:
 * every entry must lie in 0 .. N - 1 (a null idx takes rows 0 .. n - 1, resp. 0 .. bs - 1 every minibatch).  rms_mean / rms_std [56]: the
 * obs filter, read and never updated (ppo1 updates it once per segment, before the epochs: dm_rms_update).  With ratio = exp(logp_new -
 * logp_old) and A = atarg, a minibatch's losses (out_loss, DM_PPO_NLOSS float64 each) are
 *     pol_surr = -mean(min(ratio A, clip(ratio, 1 - clip, 1 + clip) A)),  pol_entpen = -entcoeff * ent,  vf_loss = mean((vpred - ret)^2),
 *     kl = mean KL(old || new),  ent = entropy of the policy (state-independent),  clipfrac = fraction of rows with |ratio - 1| > clip;
 * the gradient is that of pol_surr + pol_entpen + vf_loss, d pol_surr / d ratio = -A / n where ratio A <= clip(ratio) A, else 0.
 * Every pointer but step_scale_host / clip_host is a DEVICE pointer on one device; the work is enqueued on `hip_stream`; no device visible
 * -> DM_ENODEVICE.  Sums are taken in a fixed order: two calls with the same inputs give bitwise-identical results.
 *   dm_ppo_scratch_bytes  scratch both calls need for a minibatch of bs rows (0 for bs < 1).  A losses-only dm_ppo_lossgrad (out_grad null)
 *                         of any n needs no more than dm_ppo_scratch_bytes(1).
 *   dm_ppo_lossgrad       Replaces: `lossandgrad(ob, ac, atarg, tdlamret, cur_lrmult)` of one minibatch (and, with out_grad null,
 *                         `compute_losses`): out_loss [DM_PPO_NLOSS] and, unless out_grad is null, out_grad [dm_pg_param_count() +
 *                         dm_vf_param_count()] float32 = the flat gradient of both nets.  The multi-process path: MpiAdam all-means it.
 *   dm_ppo_fit            Replaces: `iters` minibatches of `lossandgrad` + `adam.update(g, optim_stepsize * cur_lrmult)` (MpiAdam(epsilon =
 *                         adam_epsilon) over both nets, one process): minibatch i takes rows idx[i * bs .. (i + 1) * bs), the clip range
 *                         clip_host[i] and the Adam scale step_scale_host[i] (both on the HOST; a_t = stepsize sqrt(1 - beta2^t) / (1 - beta1^t)),
 *                         and steps theta, adam_m, adam_v in place; out_loss [iters, DM_PPO_NLOSS] = each minibatch's losses before its step.
 *                         Three launches per minibatch (policy gradient, value gradient, reduction + step); nothing comes back to the host. */
#define DM_PPO_NLOSS 6
size_t dm_ppo_scratch_bytes(int32_t bs);
int dm_ppo_lossgrad(const float* ob_all, const float* ac_all, const float* atarg_all, const float* old_mean_all, const float* old_logstd,
                    const float* ret_all, const int32_t* idx, int32_t n, const float* theta, const float* rms_mean, const float* rms_std,
                    double clip, double entcoeff, float* out_grad, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream);
int dm_ppo_fit(const float* ob_all, const float* ac_all, const float* atarg_all, const float* old_mean_all, const float* old_logstd,
               const float* ret_all, const int32_t* idx, int32_t iters, int32_t bs, float* theta, float* adam_m, float* adam_v,
               const float* step_scale_host, const float* clip_host, double beta1, double beta2, double eps, double entcoeff,
               const float* rms_mean, const float* rms_std, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream);

/* Diagnostics of DM_OPT_PACKED (four environments per wavefront, csrc/slot_kernel.h): env-steps so far that exceeded a capacity of that
 * path (DM_PACKED_*: rows, contacts / contact pairs, pairs past the bounding spheres, box staging slots; or a PGS step the cost test would
 * reject) and were re-stepped by the one-env code.  out[0] total; out[1..5] by reason: candidates, box slots, contacts, rows, PGS cost test. */
int dm_batch_redo_total(dm_batch* b, int64_t* out /* [8] */);
/* Diagnostics of DM_OPT_STEP_QUEUE: out[0] = horizon launches issued for queued steps so far, out[1] = steps they carried, out[2] = steps queued now. */
int dm_batch_queue_stats(dm_batch* b, int64_t* out /* [3] */);
int dm_batch_sync(dm_batch* b);
/* Run what DM_OPT_STEP_QUEUE has queued and make the batch's stream wait (device-side, no host wait) for every pipelined sub-batch launch in
 * flight (DM_OPT_PIPELINE): afterwards work enqueued on the batch's stream sees the outputs of every earlier dm_batch_step call. */
int dm_batch_join(dm_batch* b);
const char* dm_last_error(void);
int dm_abi_version(void);
/* Arithmetic / device-state type of the loaded library: 64 (libdmenv.so) or 32 (libdmenv32.so, the same source built with
 * -DDM_REAL_FLOAT: SURVEY.md section 8b's `dtype 32`).  Every buffer of this ABI is float64 in both. */
int dm_real_bits(void);
int dm_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* DMENV_H */
