"""`DPEnv` / `DPVecEnv`: the reference's environment API on top of the HIP batch.

`DPEnv` keeps the surface `trpo.py` consumes from `dp_env_v3.DPEnv` (src/dp_env_v3.py:34-171; callers at
src/trpo.py:30-32,66,78-79,343,403-404,461-463): `reset() -> ob[56]`, `step(ac[28]) -> (ob, reward, done, {})`,
`seed`, `close`, `action_space`, `observation_space`, `reset_model`, `reset_model_init`, `load_mocap`,
`calc_config_reward`, `is_done`, `goto`, `get_time`, `set_state`, and the attributes `sim.data.qpos/qvel/xipos/ctrl/
time`, `model.{nq,nv,nu,body_mass,opt.timestep}`, `mocap`, `idx_curr`, `idx_init`, `mocap_dt`, `mocap_data_len`,
`init_qpos`, `init_qvel`, `np_random`.  It is one environment of a `Batch` of size 1; every physics call is a HIP
kernel launch (there is no CPU path — constructing it without a GPU raises).

`DPVecEnv` is the batched form (N envs in lock step, one wavefront each), following the vendored VecEnv contract
(src/utils/vec_env/__init__.py:26-100) and DummyVecEnv's auto-reset-on-done convention
(src/utils/vec_env/dummy_vec_env.py:45-56).  It accepts numpy arrays or torch CUDA tensors.

Semantics kept from the reference: reward is the constant 1.0 unless another reward mode
is selected; `frame_skip=6` is stored but `step` runs ONE mj_step; `done` is the whole-body COM height outside
[0.7, 2.0] evaluated on the derived data of the last RK4 stage; actions are not clipped in Python; the constructor
performs gym's warm-up `step(zeros)`; `reset()` = sim.reset() + reference-state-init from Python's global `random`;
`reset_model_init()` perturbs the init pose with `self.np_random` and keeps time / warm-start.
"""
import math
import random

import numpy as np

from . import _abi as A
from .batch import Batch, batch_option
from .config import Config
from .humanoid import humanoid_spec, humanoid_visual
from .mjcf import load_mjcf, load_visual
from .mocap import MocapDM
from .model import CompiledModel
from .spaces import Box
from .state_features import obs_width
from .termination import fall_body_mask, geoms_of_bodies

REWARD_MODES = {"alive": 0, "v3-config": 1, "v2-pose": 2, "imitation": 3, "v1-quat": 4}


def _load_model(xml_path=None, explicit=True):
    """An explicit `xml_path` must exist; `Config.xml_path` (the reference's cwd-relative default, src/config.py:16) falls back
    to the built-in table of the same model (humanoid.py) when the reference tree is not the working directory."""
    import os
    if xml_path and os.path.isfile(xml_path):
        return CompiledModel(load_mjcf(xml_path))
    if xml_path and explicit:
        raise FileNotFoundError("model file %r does not exist" % (xml_path,))
    return CompiledModel(humanoid_spec())


def _load_visual(xml_path=None):
    """the rendering description that goes with `_load_model(xml_path)`"""
    import os
    if xml_path and os.path.isfile(xml_path):
        return load_visual(xml_path)
    return humanoid_visual()


def _camera(camera_name):
    from .render import DEFAULT_CAMERA
    return DEFAULT_CAMERA if camera_name is None else camera_name


# DM_OPT_ACTION_MODE by name.  "raw": motor commands; "p-control" / "pd": a feedback term around the mocap frame, evaluated once per env step, added to
# a motor command; "spd-target": the action is a target pose (28 absolute hinge angles, rad) tracked by a stable PD controller that is evaluated at the
# start of every simulation substep (DeepMimic's action); "spd-mocap": the same controller around mocap frame + action (include/dmenv.h has the rule).
ACTION_MODES = {"raw": 0, "p-control": 1, "pd": 2, "spd-target": 3, "spd-mocap": 4}
# DM_OPT_CLIP_MODE of a multi-clip DPVecEnv (a list of motions): an env keeps its clip, or every episode start draws one
CLIP_MODES = {"fixed": 0, "episode": 1}


def _action_space(cm, action_mode):
    """Box of the action: the actuators' ctrlrange; for "spd-target" the hinges' jnt_range (informative: targets are not clamped)."""
    if action_mode == "spd-target":
        jr = cm.jnt_range[cm.actuator_jntid]
        return Box(low=jr[:, 0], high=jr[:, 1], dtype=np.float32)
    cr = cm.actuator_ctrlrange
    return Box(low=cr[:, 0], high=cr[:, 1], dtype=np.float32)


class _Opt(object):
    def __init__(self, timestep):
        self.timestep = timestep


class _ModelView(object):
    """The handful of `sim.model` attributes the reference's scripts read."""

    def __init__(self, cm):
        self.nq, self.nv, self.nu, self.nbody = cm.nq, cm.nv, cm.nu, cm.nbody
        self.body_mass = cm.body_mass.copy()
        self.actuator_ctrlrange = cm.actuator_ctrlrange.copy()
        self.opt = _Opt(cm.timestep)


class _DataView(object):
    """`sim.data` look-alike for env 0 of a batch: attribute reads fetch from the device (copies)."""

    def __init__(self, batch, env=0):
        self._b, self._e = batch, env

    qpos = property(lambda self: self._b.get(A.F_QPOS)[self._e])
    qvel = property(lambda self: self._b.get(A.F_QVEL)[self._e])
    xipos = property(lambda self: self._b.get(A.F_XIPOS)[self._e])
    ctrl = property(lambda self: self._b.get(A.F_CTRL)[self._e])
    time = property(lambda self: float(self._b.get(A.F_TIME)[self._e]))
    qacc_warmstart = property(lambda self: self._b.get(A.F_QACC_WARMSTART)[self._e])
    ncon = property(lambda self: int(self._b.get(A.F_NCON)[self._e]))


class _SimView(object):
    def __init__(self, env):
        self._env = env
        self.data = _DataView(env._batch)
        self.model = env.model

    def forward(self):   # sim.forward(): recompute derived quantities from the current state
        b = self._env._batch
        b.set_state(b.get(A.F_QPOS), b.get(A.F_QVEL))

    def step(self):      # sim.step() with the stored ctrl
        b = self._env._batch
        b.step(b.get(A.F_CTRL))

    def reset(self):     # mj_resetData
        self._env._batch.reset(mode=2, hard=1)


class DPEnv(object):
    metadata = {"render.modes": ["rgb_array", "depth_array"]}
    reward_range = (-float("inf"), float("inf"))
    spec = None

    def __init__(self, motion=None, mocap_path=None, xml_path=None, device=0, reward="alive", batch_factory=None, action_mode="raw", obs_mode="dp_env_v3",
                 fall_contact_bodies=None, max_episode_steps=0):
        """fall_contact_bodies / max_episode_steps: DeepMimic's early termination (termination.py; include/dmenv.h DM_OPT_FALL_BODIES,
        DM_OPT_MAX_EPISODE_STEPS): `step` also reports done when a body of the set touches the floor, or on the episode's M-th step.  Both are
        switched on after the constructor's warm-up step.
        action_mode: one of ACTION_MODES ("raw" is the reference's behaviour; "spd-target" / "spd-mocap" make the action a PD target pose).
        obs_mode: "dp_env_v3" (default: the reference's 56 numbers) or "deepmimic": `reset`, `step`, `_get_obs` and `reset_model*` return DeepMimic's
        171 state features (state_features.py) of the batch's state; their phase comes from the batch's cursor fields, which this class then writes from
        `idx_curr` / `idx_init` before every features call — for reward "alive" too, whose cursor never advances: its phase is the RSI draw."""
        self.mocap = MocapDM()
        self._terms_batch = None                          # reward_terms(): a one-env batch of its own, made on the first call
        obs_width(obs_mode)
        self.obs_mode = obs_mode
        self._action_mode = action_mode
        self._fall_mask = fall_body_mask(fall_contact_bodies)
        self._max_episode_steps = int(max_episode_steps)
        if action_mode not in ACTION_MODES:
            raise ValueError("action_mode must be one of %s" % sorted(ACTION_MODES))
        self._cm = _load_model(xml_path if xml_path is not None else Config.xml_path, explicit=xml_path is not None)
        self._visual = _load_visual(xml_path if xml_path is not None else Config.xml_path)
        self.model = _ModelView(self._cm)
        self._device = device
        self._batch_factory = batch_factory or (lambda cm, cfg, vel, n, dt: Batch(cm, cfg, vel, n, device=device, mocap_dt=dt))
        self._batch = None
        self._reward_mode = REWARD_MODES[reward]
        # reward weights / scales (src/dp_env_v3.py:42-53; unused by the default reward)
        self.weight_pose, self.weight_vel, self.weight_root, self.weight_end_eff, self.weight_com = 0.5, 0.05, 0.2, 0.15, 0.1
        self.scale_pose, self.scale_vel, self.scale_end_eff, self.scale_root, self.scale_com, self.scale_err = 2.0, 0.1, 40.0, 5.0, 10.0, 1.0
        if mocap_path is None:
            mocap_path = motion if motion is not None else Config.mocap_path
        self.load_mocap(mocap_path)
        self.reference_state_init()
        self.idx_curr = -1
        self.idx_tmp_count = -1
        # --- gym MujocoEnv.__init__(xml, 6) ---------------------------------------------------------------
        self.frame_skip = 6
        self.init_qpos = self._cm.qpos0.copy()
        self.init_qvel = np.zeros(self._cm.nv)
        self.sim = _SimView(self)
        self.data = self.sim.data
        observation, _r, done, _i = self.step(np.zeros(self._cm.nu))   # the base class's warm-up step
        assert not done
        self.action_space = _action_space(self._cm, action_mode)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(observation.size,), dtype=np.float32)
        self._set_termination()
        self.seed()

    # ---- plumbing ----------------------------------------------------------------------------------------
    @property
    def unwrapped(self):
        return self

    @property
    def dt(self):
        return self._cm.timestep * self.frame_skip

    def seed(self, seed=None):
        self.np_random = np.random.RandomState(seed)
        return [seed]

    def close(self):
        if self._batch is not None:
            self._batch.close(); self._batch = None
        if self._terms_batch is not None:
            self._terms_batch.close(); self._terms_batch = None

    def reward_terms(self, frame=None, cycle=0):
        """The 5-term imitation reward (imitation.py) of the current state against mocap frame `frame` (default: the frame the cursor is at, as the
        "deepmimic" observation's phase counts it), the reference's root advanced by `cycle` completed cycles, by name: the five errors under
        imitation.TERM_NAMES, "reward", and the dicts "terms" (the weighted terms), "joints" (each joint group's share of the pose error, by body
        name, and "root") and "end_effectors" (squared distances).  This class steps with the reference's rewards, so the call is the explicit form of
        Batch.imitation_terms on a one-env batch of its own that carries the clip's feature table, made on the first call."""
        from .imitation import END_EFFECTORS, TERM_NAMES, ImitationSpec, O_TERM_ERR, O_TERM_VALUE, O_TERM_REWARD, O_TERM_JOINT, O_TERM_ENDEFF
        if self._terms_batch is None or self._terms_clip is not self.mocap.data_config:
            if self._terms_batch is not None:
                self._terms_batch.close()
            self._terms_spec = ImitationSpec(self._cm)
            self._terms_batch = Batch(self._cm, self.mocap.data_config, self.mocap.data_vel, 1, device=self._device, mocap_dt=float(self.mocap_dt),
                                      imitation=self._terms_spec.table_for(self.mocap))
            self._terms_clip = self.mocap.data_config
        if frame is None:
            shifted = self._reward_mode in (REWARD_MODES["v2-pose"], REWARD_MODES["v1-quat"])
            frame = (max(self.idx_curr, 0) + (self.idx_init if shifted else 0)) % self.mocap_data_len
        row = self._terms_batch.imitation_terms(qpos=self._batch.get(A.F_QPOS), qvel=self._batch.get(A.F_QVEL), frame=np.array([int(frame)], dtype=np.int32),
                                                cycle=np.array([int(cycle)], dtype=np.int32))[0]
        out = {name: float(row[O_TERM_ERR + k]) for k, name in enumerate(TERM_NAMES)}
        out["reward"] = float(row[O_TERM_REWARD])
        out["terms"] = {name: float(row[O_TERM_VALUE + k]) for k, name in enumerate(TERM_NAMES)}
        names = [self._cm.body_names[b] for b in self._terms_spec.bodies] + ["root"]
        out["joints"] = {name: float(row[O_TERM_JOINT + k]) for k, name in enumerate(names)}
        out["end_effectors"] = {name: float(row[O_TERM_ENDEFF + k]) for k, (name, _off) in enumerate(END_EFFECTORS)}
        return out

    def render(self, mode="human", width=500, height=500, camera_name=None):
        """gym MujocoEnv.render: "rgb_array" -> uint8 [height, width, 3], "depth_array" -> float32 [height, width] (distance
        along the optical axis, metres; +inf where nothing is hit), ray-cast by dm_batch_render from a model camera
        (camera_name: "side" (default) or "back", dp_env_v3.xml:23-24) or a render.FreeCamera.  There is no display: "human"
        raises NotImplementedError."""
        if mode not in self.metadata["render.modes"]:
            raise NotImplementedError("render mode %r: no display here; modes are %s" % (mode, self.metadata["render.modes"]))
        depth = mode == "depth_array"
        r = self._batch.render(width, height, _camera(camera_name), depth=depth, rgb=not depth, visual=self._visual)
        return r["depth"][0] if depth else r["rgb"][0]

    def viewer_setup(self):
        pass

    def push(self, body, impulse):
        """An external push, now (Batch.push): the impulse (3 numbers, N s, world frame) at the centre of mass of `body` — a body's name or its model id
        1..13 — changes qvel by M^-1 J_b^T p.  A force F held over one `step` is the impulse F * frame_skip * model.opt.timestep before it."""
        if isinstance(body, str):
            body = int(fall_body_mask([body])).bit_length() - 1
        self._batch.push(np.array([int(body)], dtype=np.int32), np.asarray(impulse, dtype=np.float64).reshape(1, 3))

    def _sync_frame_idx(self):
        self._batch.set(A.F_FRAME_IDX, np.array([max(self.idx_curr, 0)], dtype=np.int32))
        self._batch.set(A.F_FRAME_INIT, np.array([self.idx_init], dtype=np.int32))

    # ---- reference API -------------------------------------------------------------------------------------
    def load_mocap(self, filepath):
        self.mocap.load_mocap(filepath)
        self.mocap_dt = self.mocap.dt
        self.mocap_data_len = len(self.mocap.data)
        if self._batch is not None:
            self._batch.close()
        self._batch = self._batch_factory(self._cm, self.mocap.data_config, self.mocap.data_vel, 1, float(self.mocap_dt))
        self._batch.set_option(A.OPT_REWARD_MODE, self._reward_mode)
        if self._action_mode != "raw":
            self._batch.set_option(A.OPT_ACTION_MODE, ACTION_MODES[self._action_mode])
        if hasattr(self, "sim"):
            self.sim = _SimView(self); self.data = self.sim.data
            self._set_termination()

    def _set_termination(self):
        if self._fall_mask:
            self._batch.set_option(A.OPT_FALL_BODIES, self._fall_mask)
        if self._max_episode_steps:
            self._batch.set_option(A.OPT_MAX_EPISODE_STEPS, self._max_episode_steps)

    def _get_obs(self):
        if self.obs_mode == "deepmimic":
            return self._features()[0].copy()
        return self._batch.get_obs()[0].copy()

    def _features(self):
        self._sync_frame_idx()                          # the phase is read from the batch's cursor (reward "alive" never writes it otherwise)
        return self._batch.state_features()

    def reference_state_init(self):
        self.idx_init = random.randint(0, self.mocap_data_len - 1)
        # dp_env_v3 starts its frame cursor at the draw (src/dp_env_v3.py:67-71); dp_env_v2 counts steps from 0 and adds idx_init
        # when it looks the target frame up (src/dp_env_v2.py:68-70,128-129)
        self.idx_curr = 0 if self._reward_mode in (REWARD_MODES["v2-pose"], REWARD_MODES["v1-quat"]) else self.idx_init
        self.idx_tmp_count = 0

    def early_termination(self):
        """the fall test of the current state: a body of `fall_contact_bodies` touches the floor (False without a set).  `is_done` stays the
        reference's COM rule; `step` reports either."""
        if not self._fall_mask:
            return False
        return bool(int(self._batch.floor_contacts()[0]) & geoms_of_bodies(self._fall_mask, self._cm.geom_bodyid))

    def get_joint_configs(self):
        return self.sim.data.qpos[7:]

    def calc_config_errs(self, env_config, mocap_config):
        assert len(env_config) == len(mocap_config)
        return np.sum(np.abs(env_config - mocap_config))

    def calc_config_reward(self):
        assert len(self.mocap.data) != 0
        target_config = self.mocap.data_config[self.idx_curr][7:]
        self.curr_frame = target_config
        err_configs = self.calc_config_errs(self.get_joint_configs(), target_config)
        reward_config = math.exp(-err_configs)
        self.idx_curr += 1
        self.idx_curr = self.idx_curr % self.mocap_data_len
        return reward_config

    def do_simulation(self, ctrl, n_frames):
        a = np.ascontiguousarray(np.asarray(ctrl, dtype=np.float64).reshape(1, self._cm.nu))
        return self._batch.step(a, n_substeps=int(n_frames))

    def step(self, action):
        self.step_len = 1
        if self._reward_mode != 0:
            self._sync_frame_idx()
        obs, rew, done = self.do_simulation(action, 1)
        if self._reward_mode != 0:
            self.idx_curr = int(self._batch.get(A.F_FRAME_IDX)[0])
        if self.obs_mode == "deepmimic":
            obs = self._features()                        # of the state the step left, one more launch
        return obs[0].copy(), float(rew[0]), bool(done[0]), dict()

    def is_done(self):
        z_com = float(self._batch.get(A.F_COM_Z)[0])
        return bool((z_com < 0.7) or (z_com > 2.0))

    def goto(self, pos):
        self._batch.set_state(np.asarray(pos, dtype=np.float64).reshape(1, -1), self._batch.get(A.F_QVEL))

    def get_time(self):
        return self.sim.data.time

    def set_state(self, qpos, qvel):
        qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64)
        assert qpos.shape == (self._cm.nq,) and qvel.shape == (self._cm.nv,)
        self._batch.set_state(qpos.reshape(1, -1), qvel.reshape(1, -1))

    def reset(self):
        self._batch.reset(mode=2, hard=1)          # sim.reset()
        return self.reset_model()

    def reset_model(self):
        self.reference_state_init()
        qpos = self.mocap.data_config[self.idx_init]
        qvel = self.mocap.data_vel[self.idx_init]
        self.set_state(qpos, qvel)
        observation = self._get_obs()
        self.idx_tmp_count = -self.step_len
        return observation

    def reset_model_init(self):
        c = 0.01
        self.set_state(self.init_qpos + self.np_random.uniform(low=-c, high=c, size=self.model.nq),
                       self.init_qvel + self.np_random.uniform(low=-c, high=c, size=self.model.nv))
        return self._get_obs()


# DPVecEnv(packed=None): batches of at least this many environments step four per wavefront.  Measured closed loop (one launch set per call, two pipelined
# sub-batches, BASELINE configs[2]; profiles/r06_ab_kernel_variants.md section 3, gpurun call a5), M env-steps/s one-env / packed kernel: 2 048 envs 7.49 / 7.33,
# 3 072: 10.59 / 10.27, 4 096: 12.41 / 13.32, 6 144: 12.39 / 18.65 — the crossover sits between 3 072 and 4 096 since round 5's cuts of the packed step
# (rounds 3-4: 12.3 / 11.4 at 4 096, hence the old threshold of 6 144).
PACKED_FROM_ENVS = 4096


class _Info(dict):
    """An env's `info` dict that tells its list when something is written into it (so that the list is not rebuilt every step)."""
    __slots__ = ("_owner",)

    def _touch(self):
        self._owner.dirty = True

    def __setitem__(self, k, v):
        self._touch(); dict.__setitem__(self, k, v)

    def update(self, *a, **kw):
        self._touch(); dict.update(self, *a, **kw)

    def setdefault(self, k, d=None):
        self._touch(); return dict.setdefault(self, k, d)

    def __ior__(self, other):
        self._touch(); dict.update(self, other); return self


class _InfoList(list):
    """The list `step_wait` hands out every step while nobody has written into it.  The reference's DummyVecEnv returns a fresh copy per step
    (src/utils/vec_env/dummy_vec_env.py:56): any write — into a dict (_Info) or into the list itself — marks it dirty, and the next step starts a new one."""

    def __init__(self, n):
        list.__init__(self, (_Info() for _ in range(n)))
        self.dirty = False
        for d in self:
            d._owner = self


def _marking(name):                                    # every list mutator marks the list before it acts
    f = getattr(list, name)

    def g(self, *a, **kw):
        self.dirty = True
        return f(self, *a, **kw)
    g.__name__ = name
    return g


_INFO_LIST_MUTATORS = ("__setitem__", "__delitem__", "__iadd__", "__imul__", "append", "extend", "insert", "pop", "remove", "clear", "sort", "reverse")
for _m in _INFO_LIST_MUTATORS:
    setattr(_InfoList, _m, _marking(_m))
del _m


class DPVecEnv(object):
    """N DeepMimic humanoids in lock step on one GPU (one wavefront per environment)."""

    def __init__(self, num_envs, motion="walk", xml_path=None, device=0, reward="alive", autoreset="rsi", seed=0,
                 contacts=True, limits=True, action_mode="raw", env_offset=0, batch_factory=None, frame_skip=None, diagnostics=False, dtype=64, packed=None,
                 step_queue=0, obs_mode="dp_env_v3", fall_contact_bodies=None, max_episode_steps=0, truncation_log=0, reward_terms=False,
                 horizon_termination=False, clip_weights=None, clip_mode="fixed", perturb=None, horizon_spd=False):
        """horizon_spd (DM_OPT_HORIZON_SPD; action_mode "spd-target" / "spd-mocap" only, else ValueError; ValueError with obs_mode="deepmimic", which has no
        horizon launch): keep the one-launch horizon in the two PD-target modes — `Batch.rollout`, the fused collector and the step queue run a horizon
        kernel with the stable PD controller inside every wavefront's loop, with the step launches' results (bit for bit with packed=2; with packed=True an
        env-step at 33..40 constraint rows agrees to rounding: include/dmenv.h).  It takes effect where `Batch.rollout` uses one launch per horizon at all (a
        packed batch); a list of motions and `perturb` pass through, and the library issues step launches for them.  Together with `horizon_termination` the
        horizon kernel carries both.  Off (default): these modes' horizons and queued steps are step launches.  profiles/spd_horizon.md has the measurements.
        perturb: external pushes on a random schedule (perturb.PushSchedule, a dict of its arguments, or the trainers' "bodies=...,force=a:b,..." string;
        None: off) — a random force on a random body of the set for a few env steps, again and again over every episode (DeepMimic's perturbations).  While
        it is on, one more launch precedes every step launch; horizon launches and the step queue run as step launches.  `push` applies scripted impulses
        at any time, `push_state()` reads the schedule's records.
        motion: a clip, or a LIST of clips (names / files): the batch is then multi-clip (clips.ClipSet, dm_mocap_create_set) — env e imitates clip
        (env_offset + e) % K (`clip_ids`, `set_clip_ids`) and, with clip_mode="episode", every reset that sets the frame cursor first draws the episode's clip
        with the probabilities clip_weights (None: uniform).  `mocap` / `mocap_dt` / `mocap_data_len` are then the FIRST clip's, `clip_set` the whole set, and
        frame_skip="mocap" (the imitation reward's default) is taken from the first clip's dt for every env: clips of another dt (walk 0.0333 s, spinkick
        0.0167 s) then play at the wrong speed, with a warning.  Horizon launches and the step queue run as step launches (`horizon_termination` included).  clip_mode="fixed" (default): an env keeps its clip.
        reward_terms (reward="imitation" only, else ValueError): after every `step` one more launch (Batch.imitation_terms) takes the reward the step
        returned apart, and `last_reward_terms` is the [N, 28] float64 rows (imitation.py has the columns: the five errors, the five weighted terms, their
        sum — the step's reward —, the joint groups' shares of the pose error, the end effectors' distances), numpy or device tensor like the step's
        outputs and overwritten by the next step.  With `autoreset`, the row of an environment the step ended is NaN: the step kernel has already
        replaced that state by the fresh episode's.  Off (default): nothing is launched or allocated and `last_reward_terms` stays None;
        `reward_terms()` queries the current states either way.
        truncation_log: capacity in records of the truncation log (DM_OPT_TRUNCATION_LOG; 0: off): with `max_episode_steps`, the state of every episode that
        the time limit alone ends is kept for `truncations()` before auto-reset overwrites it — a truncation is not a failure, and a learner bootstraps the
        value there (rollout.SegmentCollector(bootstrap_time_limit=True) sizes and reads the log itself).
        fall_contact_bodies: DeepMimic's early termination by fall contact — a set name of termination.FALL_BODY_SETS ("deepmimic": every body but the two
        ankles; "crawl": root, chest, neck), or body names / ids; None: off.  max_episode_steps: the episode's limit in env steps; 0: off.  While either is on,
        one more launch follows every step launch, ends the episodes of the environments that fell or ran out of steps (done = 1, `done_reason()` says why) and,
        with `autoreset`, starts their next episode as the step itself does on its own done; horizon launches and the step queue fall back to step launches.
        horizon_termination (DM_OPT_HORIZON_TERMINATION; needs `fall_contact_bodies` or `max_episode_steps`): keep the one-launch horizon instead — `Batch.rollout`,
        the fused collector and the step queue run a horizon kernel with the termination rule inside every wavefront's loop (step, termination, then the
        policy's step), with the step launches' results.  The flag takes effect where `Batch.rollout` uses one launch per horizon at all (a packed batch: `packed=True` / 2, the automatic choice, or a collector that
        picks the packed horizon — `horizon_packed_ok`); on a one-env batch it changes nothing.  ValueError for the two combinations that never have a horizon launch: the
        "spd-target" / "spd-mocap" action modes without `horizon_spd`, and obs_mode="deepmimic".
        reward="imitation": the 5-term reward of code.md:1017-1143 (imitation.py) against the frame after the current one.
        frame_skip: sim steps per env step (src/dp_env_v3.py:108-112 hard-codes 1); "mocap" = floor(mocap_dt / timestep), the
        commented intent of :107-110, so that one env step spans one mocap frame.  Default (None): 1, except "mocap" for the
        imitation reward — its reference advances one mocap frame per env step and its velocity features are per second, so any
        other value plays the clip at the wrong speed (a warning says so when one is given).
        diagnostics: keep `sim.data.xipos` / the contact geom list up to date after every step (DM_OPT_DIAGNOSTICS; the batched
        training path does not read them, `DPEnv` and raw `Batch` objects default to on).
        dtype: 64 (default) or 32 — arithmetic of the kernels; observations / actions stay float64 arrays.
        packed: DM_OPT_PACKED — four environments per wavefront (k_step_packed) instead of one.  True / False pin the kernel; 2 pins the per-step launches
        with the three-set code (k_step_packed_ext: 40 constraint rows per env instead of 32, ~8 % slower otherwise — for populations that stand on both
        feet: 8.96 against 6.18 M env-steps/s one env per wave at 8 192 envs, closed loop).  None
        (default): batches of PACKED_FROM_ENVS environments or more (two or more waves per SIMD on one MI355X; float64; every reward mode, v1-quat
        included since round 6) start on the packed kernel and re-decide every 256 steps from their own row statistics (Batch.enable_auto_packed): it is
        1.4-1.5x faster while environments stay within its per-env capacities (the RSI / early-termination regimes), and hands over to
        the one-env kernel when a competent policy keeps most environments on both feet (32+ rows).  Smaller batches: one env per wave —
        except for models without contacts and limits (BASELINE configs[1]): all waves cost the same there and four per wave is 1.5x
        faster at any size.
        action_mode: one of ACTION_MODES.  "spd-target" / "spd-mocap": the action is a PD target pose, tracked by a stable PD controller evaluated at every
        simulation substep (include/dmenv.h DM_OPT_ACTION_MODE); `action_space` is then the hinges' joint range ("spd-target") — informative, not enforced.
        These two modes run on the per-step kernels: horizon launches and the step queue fall back to step launches with identical results, unless `horizon_spd`.
        "p-control", "pd" and "spd-mocap" track the mocap frame the env is at as the env step starts — the frame its `reward` counts from: the frame cursor
        itself, but (cursor + drawn frame) % n_frames with reward="v2-pose" and (cursor // update interval + drawn frame) % n_frames with "v1-quat",
        whose cursors count the episode's steps.
        step_queue: DM_OPT_STEP_QUEUE depth (0 = off): queue `batch.step` calls and run them as one horizon launch (see below).
        obs_mode: "dp_env_v3" (default: the 56 numbers the step launch writes; nothing else is launched) or "deepmimic": `reset`, `step` and `step_wait` return
        [N, 171] DeepMimic state features (state_features.py) and `observation_space` has shape (171,).  A step is then the step launch into an internal
        56-wide buffer plus one features launch on the same stream, which reads the state after the step: with `autoreset`, a done environment's row is
        the fresh episode's features — the convention of the 56-wide observation.  The features call runs queued steps first, so with `step_queue`
        every `step` is executed at once, as in the closed loop."""
        self.num_envs = int(num_envs)
        self.horizon_termination = bool(horizon_termination)
        self.horizon_spd = bool(horizon_spd)
        if self.horizon_spd:                       # (refused before anything touches a device)
            if action_mode not in ("spd-target", "spd-mocap"):
                raise ValueError("horizon_spd=True runs the stable PD controller inside the horizon launch: it needs action_mode \"spd-target\" or \"spd-mocap\", not %r" % (action_mode,))
            if obs_mode == "deepmimic":
                raise ValueError("horizon_spd=True: obs_mode=\"deepmimic\" takes a features launch after every step, there is no horizon launch to run the controller in")
        if self.horizon_termination:               # (refused before anything touches a device)
            if not (fall_body_mask(fall_contact_bodies) or int(max_episode_steps)):
                raise ValueError("horizon_termination=True runs early termination inside the horizon launch: it needs fall_contact_bodies or max_episode_steps")
            if action_mode in ("spd-target", "spd-mocap") and not self.horizon_spd:
                raise ValueError("horizon_termination=True: action_mode=%r runs on the per-step kernels, there is no horizon launch to terminate in" % (action_mode,))
            if obs_mode == "deepmimic":
                raise ValueError("horizon_termination=True: obs_mode=\"deepmimic\" takes a features launch after every step, there is no horizon launch to terminate in")
        self.obs_mode = obs_mode
        self._obs_width = obs_width(obs_mode)
        self._ob56 = None
        if reward_terms and reward != "imitation":
            raise ValueError("reward_terms=True takes the \"imitation\" reward apart: it needs reward=\"imitation\", not %r" % (reward,))
        self._reward_terms = bool(reward_terms)
        self._autoreset = autoreset not in (None, "none")
        self.last_reward_terms = None
        if clip_mode not in CLIP_MODES:
            raise ValueError("clip_mode must be one of %s" % sorted(CLIP_MODES))
        self.clip_set = None
        many = isinstance(motion, (list, tuple))
        if not many and clip_weights is not None:
            raise ValueError("clip_weights needs a list of motions")
        if many and batch_factory is not None:
            raise ValueError("a list of motions makes a multi-clip Batch: batch_factory is not supported with it")
        self.mocap = MocapDM()
        self.mocap.load_mocap(motion[0] if many else motion)
        self.mocap_dt = self.mocap.dt
        self.mocap_data_len = len(self.mocap.data)
        self._cm = _load_model(xml_path)
        self._visual = _load_visual(xml_path)
        self.model = _ModelView(self._cm)
        flags = (0 if contacts else A.FLAG_NO_CONTACT) | (0 if limits else A.FLAG_NO_LIMIT)
        per_frame = max(1, int(float(self.mocap_dt) / float(self._cm.timestep)))
        if frame_skip is None:
            frame_skip = "mocap" if reward == "imitation" else 1
        self.frame_skip = per_frame if frame_skip == "mocap" else int(frame_skip)
        if reward == "imitation" and self.frame_skip != per_frame:
            import warnings
            warnings.warn("imitation reward with frame_skip=%d: the reference clip advances one frame (%.4f s) per env step of "
                          "%.4f s; use frame_skip='mocap' (= %d) to play it in sim time"
                          % (self.frame_skip, float(self.mocap_dt), self.frame_skip * float(self._cm.timestep), per_frame))
        imit = None
        if reward in ("imitation", "v1-quat"):
            from .imitation import ImitationSpec
            self.imitation = ImitationSpec(self._cm)
            imit = self.imitation.table_for(self.mocap)
        if many:
            from .clips import ClipSet
            self.clip_set = ClipSet(motion, clip_weights, self.imitation if imit is not None else None)
            if reward == "imitation" and self.frame_skip == per_frame and len(set(max(1, int(d / float(self._cm.timestep))) for d in self.clip_set.dt)) > 1:
                import warnings
                warnings.warn("a list of motions with different frame durations %s: frame_skip=%d is the first clip's; the imitation reward advances one frame per "
                              "env step, so the other clips play at another speed" % ([round(float(d), 4) for d in self.clip_set.dt], self.frame_skip))
            self._batch = Batch(self._cm, None, None, self.num_envs, device=device, flags=flags, dtype=dtype, clips=self.clip_set)
        elif batch_factory is None:
            self._batch = Batch(self._cm, self.mocap.data_config, self.mocap.data_vel, self.num_envs, device=device,
                                flags=flags, mocap_dt=float(self.mocap_dt), imitation=imit, dtype=dtype)
        elif imit is not None:
            self._batch = batch_factory(self._cm, self.mocap.data_config, self.mocap.data_vel, self.num_envs, flags, imitation=imit)
        else:
            self._batch = batch_factory(self._cm, self.mocap.data_config, self.mocap.data_vel, self.num_envs, flags)
        b = self._batch
        b.set_option(A.OPT_REWARD_MODE, REWARD_MODES[reward])
        b.set_option(A.OPT_AUTORESET, {"none": 0, None: 0, "rsi": 1, "init": 2}[autoreset])
        if action_mode not in ACTION_MODES:
            raise ValueError("action_mode must be one of %s" % sorted(ACTION_MODES))
        b.set_option(A.OPT_ACTION_MODE, ACTION_MODES[action_mode])
        self.action_mode = action_mode
        b.set_option(A.OPT_SEED, int(seed))
        b.set_option(A.OPT_ENV_OFFSET, int(env_offset))
        if many:
            b.set_option(A.OPT_CLIP_MODE, CLIP_MODES[clip_mode])
        self.clip_mode = clip_mode
        b.set_option(A.OPT_DIAGNOSTICS, 1 if diagnostics else 0)
        self.fall_body_mask = fall_body_mask(fall_contact_bodies)
        self.max_episode_steps = int(max_episode_steps)
        if self.fall_body_mask:
            b.set_option(A.OPT_FALL_BODIES, self.fall_body_mask)
        if self.max_episode_steps:
            b.set_option(A.OPT_MAX_EPISODE_STEPS, self.max_episode_steps)
        if int(truncation_log):
            b.set_option(A.OPT_TRUNCATION_LOG, int(truncation_log))
        if self.horizon_termination:
            b.set_option(A.OPT_HORIZON_TERMINATION, 1)
        if self.horizon_spd:
            b.set_option(A.OPT_HORIZON_SPD, 1)
        self.perturb = None
        if perturb is not None:
            from .perturb import PushSchedule
            self.perturb = PushSchedule.coerce(perturb)
            if self.perturb is not None:
                b.set_push_schedule(self.perturb)
        rowless = not (contacts or limits)          # no constraint rows: every wave costs the same, the packed kernel wins at any batch size
        auto = packed is None and batch_factory is None and (self.num_envs >= PACKED_FROM_ENVS or (rowless and self.num_envs >= 256)) and dtype == 64
        # a horizon launch (Batch.rollout, rollout.SegmentCollector) may use the packed kernel at ANY batch size: there a wave does not wait
        # for the slowest wave of every step
        # (with early termination on there is no horizon launch unless `horizon_termination`: a horizon is step launches, for which the per-step choice above holds)
        self.horizon_packed_ok = (packed is None and batch_factory is None and self.num_envs >= 256 and dtype == 64
                                  and (self.horizon_termination or not (self.fall_body_mask or self.max_episode_steps))
                                  and not many and perturb is None)      # (a multi-clip batch's horizons are step launches too, and so are those under a push schedule)
        if packed or auto:
            b.set_option(A.OPT_PACKED, 2 if (packed is not True and packed == 2) else 1)     # (packed=2: per-step launches with the three-set code, see the docstring)
        if auto:
            b.enable_auto_packed(True)
        if step_queue:
            # DM_OPT_STEP_QUEUE (include/dmenv.h): `batch.step` calls with device tensors are queued and run together as one horizon launch when `step_queue`
            # calls are queued or at `batch.join()` / any other entry point — for open-loop callers (pre-drawn or scripted actions) that do not read a step's
            # outputs before the next call.  It rides on the packed kernels; `step()` / `step_wait()` of this class join, so the facade keeps its semantics.
            if not self.packed:
                b.set_option(A.OPT_PACKED, 1)
            b.set_option(A.OPT_STEP_QUEUE, int(step_queue))
        self.action_space = _action_space(self._cm, action_mode)
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self._obs_width,), dtype=np.float32)
        self._pending = None

    @property
    def batch(self):
        return self._batch

    @property
    def packed(self):
        """True while the batch steps four environments per wavefront (DM_OPT_PACKED; may change over a run with packed=None)"""
        return bool(batch_option(self._batch, A.OPT_PACKED))

    def seed(self, seed):
        self._batch.set_option(A.OPT_SEED, int(seed))

    def clip_ids(self, out=None):
        """int32 [N]: the clip of `clip_set` each environment imitates (F_CLIP; all 0 with a single motion).  `out`: a numpy array or a device tensor."""
        return self._batch.get(A.F_CLIP, out)

    def set_clip_ids(self, ids):
        """Assign the environments' clips (values outside the set raise).  The frame cursors are left alone: follow with `reset` or `batch.set_state`."""
        self._batch.set(A.F_CLIP, ids)

    def push(self, body, impulse, mask=None):
        """Scripted pushes, now (Batch.push): env e's velocity takes impulse[e] (N s, world frame) at the centre of mass of model body body[e] (1..13; 0: none);
        body [N] int32, impulse [N,3] float64, mask [N] uint8 or None — numpy arrays or device tensors.  A force F held over one env step is the impulse
        F * frame_skip * model.opt.timestep before that step."""
        self._batch.push(body, impulse, mask)

    def push_state(self):
        """(state int32 [N,5] {episode_seen, wait, left, body, count}, force float64 [N,3]) of the push schedule (`perturb`): F_PUSH_STATE and F_PUSH_FORCE"""
        return self._batch.get(A.F_PUSH_STATE), self._batch.get(A.F_PUSH_FORCE)

    def done_reason(self, out=None):
        """int32 [N]: why the last step ended each environment's episode — bits termination.DONE_STEP (COM band, clip end), DONE_FALL, DONE_TIME_LIMIT; 0
        where it did not.  Maintained while `fall_contact_bodies` or `max_episode_steps` is on.  `out`: a numpy array or a device tensor."""
        return self._batch.get(A.F_DONE_REASON, out)

    def truncations(self, clear=True, out=None):
        """(count, index [C,4] {env, tick, frame_idx, frame_init}, qpos [C,35], qvel [C,34]) of the episodes the time limit alone ended since the log was
        last cleared (`truncation_log=C`; Batch.truncations has the contract)."""
        return self._batch.truncations(clear, out)

    def reset(self, mode="rsi", out=None):
        self._batch.reset(mode={"rsi": 0, "init": 1, "qpos0": 2}[mode], hard=1)
        if self.obs_mode == "deepmimic":
            return self._batch.state_features(out)
        return self._batch.get_obs(out)

    def _step_features(self, actions, out):
        """a step in obs_mode "deepmimic": the step launch writes its 56 numbers into an internal buffer, the features launch the [N, 171] rows"""
        b = self._batch
        if out is None:
            _o56, rew, done = b.step(actions, self.frame_skip)
            obs = None
            if type(rew).__module__.startswith("torch"):
                import torch
                obs = torch.empty((self.num_envs, self._obs_width), dtype=torch.float64, device=rew.device)
        else:
            obs, rew, done = out
            o56 = self._ob56
            if o56 is None or type(o56) is not type(rew) or getattr(o56, "device", None) != getattr(rew, "device", None):
                if type(rew).__module__.startswith("torch"):
                    import torch
                    o56 = torch.empty((self.num_envs, A.NOBS), dtype=torch.float64, device=rew.device)
                else:
                    o56 = np.empty((self.num_envs, A.NOBS))
                self._ob56 = o56
            b.step(actions, self.frame_skip, (o56, rew, done))
        return b.state_features(obs), rew, done

    def _step_terms(self, rew, done):
        """reward_terms=True: the rows of the step that has just run, into a buffer of the kind of the step's outputs; NaN where the step reset the env"""
        buf = self.last_reward_terms
        on_device = type(rew).__module__.startswith("torch")
        if buf is None or type(buf) is not type(rew) or getattr(buf, "device", None) != getattr(rew, "device", None):
            if on_device:
                import torch
                buf = torch.empty((self.num_envs, A.NTERMS), dtype=torch.float64, device=rew.device)
            else:
                buf = np.empty((self.num_envs, A.NTERMS))
        self._batch.imitation_terms(out=buf)
        if self._autoreset:
            if on_device:
                buf.masked_fill_(done.to(dtype=buf.dtype)[:, None] != 0, float("nan"))
            else:
                buf[np.asarray(done) != 0] = np.nan
        self.last_reward_terms = buf

    def reward_terms(self, env_ids=None, out=None):
        """[n, 28] float64: the "imitation" reward's terms (imitation.py has the columns) of the environments' CURRENT states against the frame their
        cursors name — after a step, the step's reward taken apart; for an environment the step reset, the fresh episode's state against the frame it
        was drawn at.  env_ids [n]: a subset (default: all).  reward="imitation" only (Batch.imitation_terms)."""
        return self._batch.imitation_terms(env_ids=env_ids, out=out)

    def step_async(self, actions):
        self._pending = actions

    def step_wait(self, out=None):
        if self.obs_mode == "deepmimic":
            obs, rew, done = self._step_features(self._pending, out)
        else:
            obs, rew, done = self._batch.step(self._pending, self.frame_skip, out)
        self._pending = None
        if getattr(self._batch, "_queue_refs", None) is not None:
            self._batch.join()      # OPT_STEP_QUEUE: the call was only queued, and what this method returns is read in stream order
        if self._reward_terms:
            self._step_terms(rew, done)
        # `infos`: one dict per env (src/utils/vec_env/dummy_vec_env.py:45-56).  This env never puts anything into them, so the list is
        # built once and handed out again while every dict is still empty (building 4 096 dicts per step cost more than the step's
        # launch); a caller that writes into one (bench/monitor.py:73-74 does, at episode ends) gets fresh dicts from the next step on.
        infos = self._infos
        if infos is None or infos.dirty:
            infos = self._infos = _InfoList(self.num_envs)
        return obs, rew, done, infos

    _infos = None

    def step(self, actions, out=None):
        self.step_async(actions)
        return self.step_wait(out)

    metadata = {"render.modes": ["rgb_array"]}

    def get_images(self, width=128, height=128, camera_name=None):
        """baselines VecEnv.get_images: uint8 [N, height, width, 3], one image per environment (dm_batch_render)"""
        return self._batch.render(width, height, _camera(camera_name), visual=self._visual)["rgb"]

    def render(self, mode="rgb_array", width=128, height=128, camera_name=None):
        """baselines VecEnv.render: the environments' images tiled into one (render.tile_images); "human" raises"""
        if mode != "rgb_array":
            raise NotImplementedError("render mode %r: no display here; the mode is 'rgb_array'" % (mode,))
        from .render import tile_images
        return tile_images(self.get_images(width, height, camera_name))

    def close(self):
        self._batch.close()
