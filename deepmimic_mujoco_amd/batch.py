"""`Batch`: thin Python owner of a `dm_batch` (include/dmenv.h) — N lock-step environments on one GPU.

Buffers may be numpy arrays (host pointers; the library stages them) or torch tensors on the batch's device
(device pointers, zero-copy, stream-ordered).  Nothing here computes physics: every call lands in a HIP kernel.
"""
import ctypes as C

import numpy as np

from . import _abi as A


def _is_torch(x):
    return type(x).__module__.startswith("torch")


# numpy dtype -> the torch dtype's name (torch itself is imported only where a tensor is met or made)
_TORCH_DTYPE = {np.float64: "float64", np.float32: "float32", np.int32: "int32", np.uint8: "uint8"}


def _view_args(ptr, n_batch, device, state, env_ids, outs, who):
    """The arrays of a read-only view call (Batch.render, state_features, floor_contacts, imitation_terms).  ptr: Batch._ptr; state: the optional explicit
    state as (value, dtype, shape after n) entries, all given or all None; env_ids [n] or None; outs: the requested outputs as (given or None,
    dtype, shape after n).  n comes from the explicit state, else from env_ids, else it is the batch's.  One tensor among them makes the
    call a device call: missing outputs are then allocated on cuda:<device> and numpy inputs moved there; otherwise everything is numpy.
    -> (n, input pointers [state..., env_ids], output pointers, ptr_kind, keepalives, output objects); None inputs give None pointers."""
    explicit = bool(state) and state[0][0] is not None
    if explicit and env_ids is not None:
        raise ValueError("%s: an explicit state and env_ids exclude each other" % who)
    n = int(state[0][0].shape[0]) if explicit else (int(len(env_ids)) if env_ids is not None else n_batch)
    ins = list(state) + [(env_ids, np.int32, ())]
    on_device = False
    for x, _dt, _shp in ins + outs:
        if x is not None and _is_torch(x):
            on_device = True
            import torch
            where = "cuda:%d" % device
            break
    in_ptrs, out_ptrs, objs, keep, kinds = [], [], [], [], set()
    for x, dt, shp in ins:
        if x is None:
            in_ptrs.append(None)
            continue
        if on_device and not _is_torch(x):
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=dt), device=where)
        p, kind, ka = ptr(x, dt, (n,) + shp)
        in_ptrs.append(p); keep.append(ka); kinds.add(kind)
    for x, dt, shp in outs:
        shp = (n,) + shp
        if x is None:
            x = torch.empty(shp, dtype=getattr(torch, _TORCH_DTYPE[dt]), device=where) if on_device else np.empty(shp, dtype=dt)
        p, kind, ka = ptr(x, dt, shp, out=True)
        out_ptrs.append(p); keep.append(ka); objs.append(x); kinds.add(kind)
    if len(kinds) != 1:
        raise ValueError("%s buffers must be all numpy arrays or all device tensors" % who)
    return n, in_ptrs, out_ptrs, kinds.pop(), keep, objs


def batch_option(batch, opt, default=0):
    """Option `opt` as last set on `batch`.  The one place that tolerates batches that are not `Batch` (DPVecEnv(batch_factory=...): the emulator's
    and the host tests' batches keep no `options`): they read as `default`."""
    return int(getattr(batch, "options", {}).get(int(opt), default))


class Batch(object):
    def __init__(self, compiled_model, data_config, data_vel, n_envs, device=0, flags=0, mocap_dt=0.0, imitation=None, dtype=64, clips=None):
        """clips: a clips.ClipSet — the batch is then MULTI-CLIP (dm_mocap_create_set: every env imitates one clip of the set, F_CLIP; OPT_CLIP_MODE);
        data_config, data_vel, mocap_dt and imitation are the set's and must be None / left at their defaults.
        dtype: arithmetic / device-state type of the kernels, 64 (default: the parity path) or 32 (the float32 build of the same
        source, libdmenv32.so: faster; per step ~4e-7 of the observation scale at the median and ~4e-6 at worst against a float64 evaluation
        of the same float32-rounded state, the error of any float32 evaluation: DESIGN.md section 5).  Buffers are float64 either way."""
        # the Python side's own state, all of it
        self.options = {}                  # what set_option has set, by option number
        self._stream_handle = None         # the stream the library was last told to use (None: its own; no device tensor seen yet)
        self._render_descs = {}            # render(): camera descriptions by (size, model camera, visual table)
        self._queue_refs = None            # OPT_STEP_QUEUE: the tensors of the steps that may still be queued
        self._auto = False                 # the per-step kernel chooser (enable_auto_packed) and its window
        self._auto_ctr = self._redo_last = self._redo_rows_last = self._calm_checks = 0
        self.auto_switches = None          # (None: this batch never had a chooser)
        self.push_schedule = None          # the perturb.PushSchedule set_push_schedule last set (None: off)
        L = A.load(dtype)
        self.dtype = int(dtype)
        self._L = L
        self.n = int(n_envs)
        self.device = int(device)
        self.compiled_model = compiled_model
        md, self._keep = A.make_model_desc(compiled_model)
        self._model = C.c_void_p(); self._mocap = C.c_void_p(); self._h = C.c_void_p()
        A.check(L.dm_model_create(C.byref(md), C.byref(self._model)), L)
        self.clips = clips
        if clips is not None:
            if data_config is not None or data_vel is not None or imitation is not None:
                raise ValueError("clips=ClipSet carries the mocap tables: data_config, data_vel and imitation must be None")
            self.n_frames = int(clips.n_frames.sum())
            self._mocap = self._create_clip_set(L, clips)
            A.check(L.dm_batch_create(self._model, self._mocap, self.n, self.device, int(flags), C.byref(self._h)), L)
            return
        cfg = np.ascontiguousarray(data_config, dtype=np.float64); vel = np.ascontiguousarray(data_vel, dtype=np.float64)
        if cfg.ndim != 2 or cfg.shape[1] != A.NQ or vel.shape != (cfg.shape[0], A.NV):
            raise ValueError("mocap tables must be [F,35] and [F,34]")
        self.n_frames = cfg.shape[0]
        A.check(L.dm_mocap_create(cfg.ctypes.data_as(A._dp), vel.ctypes.data_as(A._dp), cfg.shape[0], float(mocap_dt),
                                  C.byref(self._mocap)), L)
        if imitation is not None:            # (table [F,112], params [32]) from imitation.ImitationSpec: enables reward mode 3
            tab = np.ascontiguousarray(imitation[0], dtype=np.float64); par = np.ascontiguousarray(imitation[1], dtype=np.float64)
            if tab.shape != (cfg.shape[0], 112) or par.shape != (32,):
                raise ValueError("imitation = (table [F,112], params [32])")
            A.check(L.dm_mocap_set_imitation(self._mocap, tab.ctypes.data_as(A._dp), 112, par.ctypes.data_as(A._dp)), L)
        A.check(L.dm_batch_create(self._model, self._mocap, self.n, self.device, int(flags), C.byref(self._h)), L)

    @staticmethod
    def _create_clip_set(L, clips):
        """dm_mocap_create_set over one dm_mocap per clip of the ClipSet (destroyed again: the set holds its own copy) -> the set's handle"""
        hs = []
        try:
            for k, m in enumerate(clips.mocaps):
                cfg = np.ascontiguousarray(m.data_config, dtype=np.float64); vel = np.ascontiguousarray(m.data_vel, dtype=np.float64)
                h = C.c_void_p()
                A.check(L.dm_mocap_create(cfg.ctypes.data_as(A._dp), vel.ctypes.data_as(A._dp), cfg.shape[0], float(m.dt), C.byref(h)), L)
                hs.append(h)
                if clips.imitation is not None:
                    tab = np.ascontiguousarray(clips.imitation[k][0], dtype=np.float64); par = np.ascontiguousarray(clips.imitation[k][1], dtype=np.float64)
                    A.check(L.dm_mocap_set_imitation(h, tab.ctypes.data_as(A._dp), 112, par.ctypes.data_as(A._dp)), L)
            arr = (C.c_void_p * len(hs))(*[h.value for h in hs])
            w = np.ascontiguousarray(clips.weights, dtype=np.float64)
            out = C.c_void_p()
            A.check(L.dm_mocap_create_set(arr, len(hs), w.ctypes.data_as(A._dp), C.byref(out)), L)
            return out
        finally:
            for h in hs:
                L.dm_mocap_destroy(h)

    def close(self):
        L = getattr(self, "_L", None)
        if L is None:
            return
        if getattr(self, "_h", None):
            L.dm_batch_destroy(self._h); self._h = None
        if getattr(self, "_mocap", None):
            L.dm_mocap_destroy(self._mocap); self._mocap = None
        if getattr(self, "_model", None):
            L.dm_model_destroy(self._model); self._model = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers ------------------------------------------------------------------------------------
    def _ptr(self, x, dtype, shape, out=False):
        """-> (pointer, kind, keepalive)"""
        if x is None:
            return None, A.PTR_HOST, None
        if _is_torch(x):
            import torch
            want = getattr(torch, _TORCH_DTYPE[dtype])
            if x.dtype != want or not x.is_contiguous() or tuple(x.shape) != tuple(shape):
                raise ValueError("tensor must be contiguous %s of shape %s" % (want, shape))
            if x.device.type != "cuda" or (x.device.index or 0) != self.device:
                raise ValueError("tensor must live on cuda:%d" % self.device)
            # device buffers are ordered on the batch's stream: follow torch's current stream so that kernels producing
            # the tensor (e.g. the policy, torch.randn) and our launch are serialised without extra synchronisation
            cur = torch.cuda.current_stream(x.device).cuda_stream
            if cur != self._stream_handle:
                self.set_stream(cur)
            return C.c_void_p(x.data_ptr()), A.PTR_DEVICE, x
        a = x if out else np.ascontiguousarray(x, dtype=dtype)
        if a.dtype != dtype or not a.flags.c_contiguous or a.shape != tuple(shape):
            raise ValueError("array must be C-contiguous %s of shape %s" % (np.dtype(dtype), shape))
        return C.c_void_p(a.ctypes.data), A.PTR_HOST, a

    def set_option(self, opt, value):
        A.check(self._L.dm_batch_set_option(self._h, int(opt), int(value)), self._L)
        self.options[int(opt)] = int(value)
        if int(opt) == A.OPT_STEP_QUEUE:
            self._queue_refs = [] if int(value) > 0 else None

    def queue_stats(self):
        """OPT_STEP_QUEUE: (horizon launches issued for queued steps, steps they carried, steps queued now)"""
        v = (C.c_int64 * 3)()
        A.check(self._L.dm_batch_queue_stats(self._h, v), self._L)
        return int(v[0]), int(v[1]), int(v[2])

    @property
    def can_step_act(self):
        """dm_batch_step_act needs the two-tier kernel (option 102, default on) and no per-stage profiling (option 101)."""
        return self.options.get(102, 1) != 0 and self.options.get(101, 0) == 0

    def set_stream(self, stream_handle):
        A.check(self._L.dm_batch_set_stream(self._h, C.c_void_p(int(stream_handle))), self._L)
        self._stream_handle = int(stream_handle)

    # ---- kernel choice by workload (DPVecEnv(packed=None)) ---------------------------------------------------------------
    ADAPT_EVERY = 256            # steps between looks at the batch's row statistics (one small D2H + stream sync each)
    REDO_RATE_MAX = 3e-4         # packed -> one-env: env-steps per env-step that overflowed the packed path's capacities
    HEAVY_ROWS = 30              # one-env -> packed: no environment of the batch holds more constraint rows than this (per-step packed launches hold 32)
    HEAVY_ROWS_EXT = 38          # ... -> packed with the three-set code (OPT_PACKED 2: 40 rows per env)

    def enable_auto_packed(self, on=True):
        """Let the batch choose between one and four environments per wavefront (DM_OPT_PACKED) from what it is simulating: the packed
        kernel is 1.4-1.5x faster while environments stay within its per-env capacities (_abi.PACKED_*: 32 rows per step, 13 contacts), but every
        environment beyond them is re-stepped one per wave AFTER the packed launch.  A population that stands on both feet (33 .. 37 rows for a few per
        cent of its env-steps) is moved to the per-step launches with the three-set code (OPT_PACKED 2: 40 rows per env, ~8 % slower otherwise) and back
        when nobody holds more than 32 rows; overflows of another kind send the batch to the one-env kernel.  Every ADAPT_EVERY steps the redo rate and
        its reasons (packed) or the largest row count (one-env) of the batch decide; the choice is a deterministic function of the trajectory."""
        self._auto = bool(on)
        self._auto_ctr = 0
        self._redo_last = self.redo_total() if on else 0
        self._redo_rows_last = self.redo_reasons()[4] if on else 0
        self._calm_checks = 0
        self.auto_switches = 0

    CALM_CHECKS = 3              # OPT_PACKED 2 -> 1 only after this many consecutive looks with nobody above 32 rows (a population near the redo threshold
                                 #  holds ~2.5 such environments per step: a single snapshot reads zero one time in twelve and the batch would flip 2 -> 1 -> 2)

    def rebaseline_auto(self):
        """The redo counters moved while the chooser was suspended (SegmentCollector's horizon launches re-step inside the wave and count there): start
        the next window from where they stand now."""
        r = self.redo_reasons()
        self._redo_last = r[0]; self._redo_rows_last = r[4]
        self._calm_checks = 0

    def suspend_auto(self):
        """Switch the chooser off for a caller that picks the kernel itself for a while (rollout.HorizonKernelChoice); its counters stay.
        -> whether it was on.  With `resume_auto` the only way anything outside this class touches the chooser."""
        was, self._auto = self._auto, False
        return was

    def resume_auto(self):
        """the chooser on again after `suspend_auto`, its window starting where the redo counters stand now"""
        self._auto = True
        self.rebaseline_auto()

    def _adapt(self):
        self._auto_ctr += 1
        if self._auto_ctr % self.ADAPT_EVERY:
            return
        mode = self.options.get(A.OPT_PACKED, 0)
        if mode:
            reasons = self.redo_reasons()
            redo = reasons[0]
            rate = (redo - self._redo_last) / float(self.ADAPT_EVERY * self.n)
            rows_share = (reasons[4] - self._redo_rows_last) / float(max(1, redo - self._redo_last))
            self._redo_last = redo; self._redo_rows_last = reasons[4]
            if rate > self.REDO_RATE_MAX:
                self._calm_checks = 0
                # too many environments beyond the per-step capacities.  Nearly all of them for ROWS (a population standing on both feet: 33 .. 37): the
                # per-step launches with the three-set code (OPT_PACKED 2, 40 rows per env); otherwise — or if that was already on — the one-env kernel
                self.set_option(A.OPT_PACKED, 2 if (mode == 1 and rows_share >= 0.9) else 0); self.auto_switches += 1
            elif mode == 2:
                # nobody above 32 rows at CALM_CHECKS looks in a row: the lean per-step kernel (8 % faster)
                self._calm_checks = self._calm_checks + 1 if int((self.get(A.F_NEFC) > A.PACKED_MAXROWS_PER_STEP).sum()) == 0 else 0
                if self._calm_checks >= self.CALM_CHECKS:
                    self._calm_checks = 0
                    self.set_option(A.OPT_PACKED, 1); self.auto_switches += 1
        else:
            top = int(self.get(A.F_NEFC).max())
            if top <= self.HEAVY_ROWS_EXT:
                self.set_option(A.OPT_PACKED, 1 if top <= self.HEAVY_ROWS else 2); self.auto_switches += 1
                self.rebaseline_auto()

    # ---- the hot path -------------------------------------------------------------------------------
    def _out_ptrs(self, out, lead, kind, error):
        """out = (obs, rew, done) with the leading shape `lead` -> their three pointers, every one of pointer kind `kind`: else ValueError(error)"""
        obs, rew, done = out
        op, k1, _ = self._ptr(obs, np.float64, lead + (A.NOBS,), out=True)
        rp, k2, _ = self._ptr(rew, np.float64, lead, out=True)
        dp, k3, _ = self._ptr(done, np.uint8, lead, out=True)
        if not (kind == k1 == k2 == k3):
            raise ValueError(error)
        return op, rp, dp

    def _weights_ptr(self, weights):
        import torch
        if not (weights.is_cuda and weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() == self._L.dm_policy_weight_count()):
            raise ValueError("weights: the packed float32 policy block (MlpPolicy.pack()) on the device")
        return C.c_void_p(weights.data_ptr())

    def _step_device(self, action, n_substeps, out):
        """`step` for device tensors with every buffer given: the same checks as `_ptr`, written out once (the generic path costs ~10 us
        of Python per call — 4 % of a 250 us step).  Returns None when the arguments are not of that form."""
        obs, rew, done = out
        try:
            dev = action.device
            if not (action.is_cuda and obs.is_cuda and rew.is_cuda and done.is_cuda):
                return None
        except AttributeError:
            return None
        import torch
        n = self.n
        if not (action.dtype == obs.dtype == rew.dtype == torch.float64 and done.dtype == torch.uint8 and action.is_contiguous() and obs.is_contiguous()
                and rew.is_contiguous() and done.is_contiguous() and action.shape == (n, A.NU) and obs.shape == (n, A.NOBS) and rew.shape == (n,) and done.shape == (n,)):
            return None                                            # the generic path raises the precise error
        if (dev.index or 0) != self.device or obs.device != dev or rew.device != dev or done.device != dev:
            return None
        cur = torch.cuda.current_stream(dev).cuda_stream
        if cur != self._stream_handle:
            self.set_stream(cur)
        rc = self._L.dm_batch_step(self._h, action.data_ptr(), obs.data_ptr(), rew.data_ptr(), done.data_ptr(), int(n_substeps), A.PTR_DEVICE)
        if rc:
            A.check(rc, self._L)
        if self._queue_refs is not None:
            self._queue_refs.append((action, obs, rew, done))
            if len(self._queue_refs) > 2 * A.MAX_STEP_QUEUE:
                del self._queue_refs[:A.MAX_STEP_QUEUE]
        return out

    def step(self, action, n_substeps=1, out=None):
        if self._auto:
            self._adapt()
        if out is not None:
            r = self._step_device(action, n_substeps, out)
            if r is not None:
                return r
        n = self.n
        ap, kind, _ka = self._ptr(action, np.float64, (n, A.NU))
        if out is None:
            if kind == A.PTR_DEVICE:
                import torch
                dev = action.device
                out = (torch.empty((n, A.NOBS), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                       torch.empty(n, dtype=torch.uint8, device=dev))
            else:
                out = (np.empty((n, A.NOBS)), np.empty(n), np.empty(n, dtype=np.uint8))
        obs, rew, done = out
        op, rp, dp = self._out_ptrs(out, (n,), kind, "action and output buffers must all be host arrays or all be device tensors")
        A.check(self._L.dm_batch_step(self._h, ap, op, rp, dp, int(n_substeps), kind), self._L)
        if self._queue_refs is not None and kind == A.PTR_DEVICE:
            # OPT_STEP_QUEUE: the call may only have been queued — its tensors must outlive the flush (any other entry point of the batch)
            self._queue_refs.append((action, obs, rew, done))
            if len(self._queue_refs) > 2 * A.MAX_STEP_QUEUE:
                del self._queue_refs[:A.MAX_STEP_QUEUE]      # (older than any step that can still be queued)
        return obs, rew, done

    def step_act(self, action, n_substeps, out, weights, next_action, next_vpred, stochastic, seed, counter):
        """`step` followed, inside the step kernel, by the policy's step on the new observations (dm_batch_step_act): device tensors
        only.  action [n, 28] f64 -> out = (obs [n, 56] f64, rew [n] f64, done [n] u8); next_action [n, 28] f64 and next_vpred [n] f32
        receive the action / value for those observations; `weights` is MlpPolicy.pack()'s float32 block."""
        if self._auto:
            self._adapt()
        n = self.n
        ap, kind, _ka = self._ptr(action, np.float64, (n, A.NU))
        np_, k4, _ = self._ptr(next_action, np.float64, (n, A.NU), out=True)
        if not (kind == k4 == A.PTR_DEVICE):
            raise ValueError("step_act works on device tensors")
        op, rp, dp = self._out_ptrs(out, (n,), A.PTR_DEVICE, "step_act works on device tensors")
        wp = self._weights_ptr(weights)
        import torch
        if not (next_vpred.is_cuda and next_vpred.dtype == torch.float32 and next_vpred.is_contiguous() and next_vpred.numel() == n):
            raise ValueError("next_vpred: float32 [n] on the device")
        A.check(self._L.dm_batch_step_act(self._h, ap, op, rp, dp, int(n_substeps), wp, np_,
                                          C.c_void_p(next_vpred.data_ptr()), 1 if stochastic else 0, int(seed) & (2 ** 64 - 1), int(counter)), self._L)
        obs, rew, done = out
        return obs, rew, done

    def rollout(self, action, out, n_substeps=1, weights=None, vpred=None, stochastic=True, seed=0, counter=0):
        """T steps in one call (dm_batch_rollout), device tensors only: action [T + 1, n, 28] f64 (row t feeds step t; with `weights` — the
        packed policy block — rows 1..T are written by the policy), out = (obs [T, n, 56] f64, rew [T, n] f64, done [T, n] u8), vpred [T, n]
        f32 (with weights).  Same results as T `step` / `step_act` calls; on the packed path (option 105) one launch for the horizon — with early
        termination on (OPT_FALL_BODIES, OPT_MAX_EPISODE_STEPS) only under OPT_HORIZON_TERMINATION, else T step launches with their termination launches."""
        import torch
        obs, rew, done = out
        T, n = int(obs.shape[0]), self.n
        ap, k0, _ = self._ptr(action, np.float64, (T + 1, n, A.NU), out=True)
        if k0 != A.PTR_DEVICE:
            raise ValueError("rollout works on device tensors")
        op, rp, dp = self._out_ptrs(out, (T, n), A.PTR_DEVICE, "rollout works on device tensors")
        wp = vp = None
        if weights is not None:
            wp = self._weights_ptr(weights)
            if vpred is None or not (vpred.is_cuda and vpred.dtype == torch.float32 and vpred.is_contiguous() and tuple(vpred.shape) == (T, n)):
                raise ValueError("vpred: float32 [T, n] on the device")
            vp = C.c_void_p(vpred.data_ptr())
        A.check(self._L.dm_batch_rollout(self._h, ap, op, rp, dp, T, int(n_substeps), wp, vp, 1 if stochastic else 0, int(seed) & (2 ** 64 - 1), int(counter)), self._L)
        return obs, rew, done

    def get_obs(self, out=None):
        if out is None:
            out = np.empty((self.n, A.NOBS))
        p, kind, _ = self._ptr(out, np.float64, (self.n, A.NOBS), out=True)
        A.check(self._L.dm_batch_get_obs(self._h, p, kind), self._L)
        return out

    def render(self, width, height, camera="side", qpos=None, env_ids=None, depth=False, segmentation=False, out=None, visual=None,
               rgb=True, geom_xform=False):
        """Images of environment states through dm_batch_render.  camera: a model camera's name or a
        render.FreeCamera; qpos [n,35]: render these poses instead of the batch's state (env_ids must then be None); env_ids [n]:
        a subset of the batch's environments (default: all).  Returns a dict with "rgb" uint8 [n,H,W,3] and, when asked,
        "depth" float32 [n,H,W], "segmentation" int32 [n,H,W], "geom_xform" float64 [n,16,12].  out: a dict of buffers under
        the same keys; like `step`, numpy arrays (host) or torch tensors on the batch's device (stream-ordered, no host wait)."""
        from . import render as R
        want = [k for k, on in (("rgb", rgb), ("depth", depth), ("segmentation", segmentation), ("geom_xform", geom_xform)) if on]
        if not want:
            raise ValueError("nothing to render")
        W, H = int(width), int(height)
        spec = {"rgb": (np.uint8, (H, W, 3)), "depth": (np.float32, (H, W)), "segmentation": (np.int32, (H, W)), "geom_xform": (np.float64, (A.NGEOM, 12))}
        out = out or {}
        n, (qp, ip), ps, kind, _keep, objs = _view_args(self._ptr, self.n, self.device, [(qpos, np.float64, (A.NQ,))], env_ids,
                                                         [(out.get(k),) + spec[k] for k in want], "render")
        ptrs = dict(zip(want, ps))
        key = (W, H, camera, id(visual)) if isinstance(camera, str) else None      # (model cameras: resolved once per size and visual table)
        cache = self._render_descs
        desc = cache[key][0] if key in cache else None
        if desc is None:
            desc = R.make_desc(self.compiled_model, W, H, camera, visual)
            if key is not None:
                cache[key] = (desc, visual)          # (holding `visual` keeps its id from being reused)
        A.check(self._L.dm_batch_render(self._h, qp, ip, n, C.byref(desc), ptrs.get("rgb"), ptrs.get("depth"), ptrs.get("segmentation"),
                                        ptrs.get("geom_xform"), kind), self._L)
        return dict(zip(want, objs))

    def state_features(self, out=None, env_ids=None, qpos=None, qvel=None, phase=None):
        """DeepMimic's state features through dm_batch_state_features (one launch; state_features.py has the layout): [n, 171]
        float64.  Default: the batch's current state of every environment, or of `env_ids` [n]; with qpos [n,35], qvel [n,34] and
        phase [n] (all three, env_ids must then be None): those states instead (mocap frames, recorded trajectories).  Like `step`,
        the arrays are numpy arrays (host) or torch tensors on the batch's device (stream-ordered; no host wait, except that device
        `env_ids` are first copied back and range-checked on the host, which waits for the stream).  Reads the batch, changes
        nothing in it."""
        explicit = [x is not None for x in (qpos, qvel, phase)]
        if any(explicit) and not all(explicit):
            raise ValueError("an explicit state needs qpos, qvel and phase")
        f64 = np.float64
        n, (qp, vp, pp, ip), (op,), kind, _keep, (out,) = _view_args(self._ptr, self.n, self.device, [(qpos, f64, (A.NQ,)), (qvel, f64, (A.NV,)), (phase, f64, ())],
                                                                     env_ids, [(out, f64, (A.NSTATE,))], "state_features")
        A.check(self._L.dm_batch_state_features(self._h, qp, vp, pp, ip, n, op, kind), self._L)
        return out

    def floor_contacts(self, qpos=None, env_ids=None, out=None):
        """Which geoms touch the floor, through dm_batch_floor_contacts (one launch): int32 [n], bit g (1..15) set when the collision stage of a
        step would emit a contact for (floor, geom g) at the state.  Default: the batch's current state of every environment, or of `env_ids`
        [n]; with qpos [n,35] (env_ids must then be None): those states.  Arrays as for `state_features`.  Reads the batch, changes nothing."""
        n, (qp, ip), (op,), kind, _keep, (out,) = _view_args(self._ptr, self.n, self.device, [(qpos, np.float64, (A.NQ,))], env_ids, [(out, np.int32, ())],
                                                             "floor_contacts")
        A.check(self._L.dm_batch_floor_contacts(self._h, qp, ip, n, op, kind), self._L)
        return out

    def imitation_terms(self, qpos=None, qvel=None, frame=None, cycle=None, env_ids=None, out=None):
        """The five terms of the "imitation" reward through dm_batch_imitation_terms (one launch; imitation.py has the columns): [n, 28] float64 —
        the errors [0:5], the weighted terms [5:10], their sum (the reward) [10], each joint group's share of the pose error [11:24], each end
        effector's squared distance [24:28].  Default: the batch's current state and cursors of every environment, or of `env_ids` [n] — reward mode 3
        only; right after a step column 10 is that step's reward, except where the step reset the environment (the row is then the fresh episode's).
        With qpos [n,35], qvel [n,34] and frame [n] int32 (all three; cycle [n] int32 optional, env_ids must then be None): those states against
        those rows of the imitation table, in any reward mode; a frame outside the table raises for numpy arrays and gives a row of NaN for device
        tensors.  Arrays as for `state_features`.  Reads the batch, changes nothing."""
        explicit = [x is not None for x in (qpos, qvel, frame)]
        if (any(explicit) or cycle is not None) and not all(explicit):
            raise ValueError("an explicit state needs qpos, qvel and frame")
        f64, i32 = np.float64, np.int32
        n, (qp, vp, fp, cp, ip), (op,), kind, _keep, (out,) = _view_args(self._ptr, self.n, self.device, [(qpos, f64, (A.NQ,)), (qvel, f64, (A.NV,)), (frame, i32, ()),
                                                                          (cycle, i32, ())], env_ids, [(out, f64, (A.NTERMS,))], "imitation_terms")
        A.check(self._L.dm_batch_imitation_terms(self._h, qp, vp, fp, cp, ip, n, op, kind), self._L)
        return out

    def truncations(self, clear=True, out=None, device=None):
        """The truncation log (set_option(OPT_TRUNCATION_LOG, C), C > 0; include/dmenv.h) through dm_batch_truncations: the states of the episodes
        the time limit ALONE ended since the log was last cleared, kept because auto-reset overwrites them — what a learner bootstraps the value
        from.  -> (count, index [C,4] int32 rows {env, tick, frame_idx, frame_init}, qpos [C,35], qvel [C,34] float64); the first min(count, C) records
        are valid, in arrival order (key on (tick, env)), and count > C says the log overflowed.  clear: the count and the tick (step calls since
        the last clear) then start again.  out: the four buffers, each of index / qpos / qvel optional (None: not copied), all numpy arrays (host:
        count is an int32 [1] array, the call waits once) or all tensors on the batch's device (count an int32 [1] tensor; stream-ordered, nothing
        waits).  Without `out`: device tensors when the batch has been stepped with device tensors (or device=True), else numpy arrays."""
        C_ = self.options.get(A.OPT_TRUNCATION_LOG, 0)
        if out is None:
            if device is None:
                device = self._stream_handle is not None
            if device:
                import torch
                where = "cuda:%d" % self.device
                out = (torch.zeros(1, dtype=torch.int32, device=where), torch.zeros((C_, 4), dtype=torch.int32, device=where),
                       torch.zeros((C_, A.NQ), dtype=torch.float64, device=where), torch.zeros((C_, A.NV), dtype=torch.float64, device=where))
            else:
                out = (np.zeros(1, dtype=np.int32), np.zeros((C_, 4), dtype=np.int32), np.zeros((C_, A.NQ)), np.zeros((C_, A.NV)))
        count, index, qpos, qvel = out
        if count is None:
            raise ValueError("truncations: the count buffer is required")
        rows = [int(x.shape[0]) for x in (index, qpos, qvel) if x is not None]
        if len(set(rows)) > 1:
            raise ValueError("truncations: index, qpos and qvel must hold the same number of records")
        cap = rows[0] if rows else 0
        cp, k0, _a = self._ptr(count, np.int32, (1,), out=True)
        ip, k1, _b = self._ptr(index, np.int32, (cap, 4), out=True)
        qp, k2, _c = self._ptr(qpos, np.float64, (cap, A.NQ), out=True)
        vp, k3, _d = self._ptr(qvel, np.float64, (cap, A.NV), out=True)
        if len({k0} | {k for k, x in ((k1, index), (k2, qpos), (k3, qvel)) if x is not None}) != 1:
            raise ValueError("truncations buffers must be all numpy arrays or all device tensors")
        A.check(self._L.dm_batch_truncations(self._h, cp, ip, qp, vp, cap, 1 if clear else 0, k0), self._L)
        return count, index, qpos, qvel

    def set_state(self, qpos, qvel, frame_idx=None, mask=None):
        n = self.n
        qp, k, _a = self._ptr(qpos, np.float64, (n, A.NQ)); vp, k2, _b = self._ptr(qvel, np.float64, (n, A.NV))
        fp, k3, _c = self._ptr(frame_idx, np.int32, (n,)); mp, k4, _d = self._ptr(mask, np.uint8, (n,))
        kinds = {k, k2} | ({k3} if frame_idx is not None else set()) | ({k4} if mask is not None else set())
        if len(kinds) != 1:
            raise ValueError("mixed host/device buffers")
        A.check(self._L.dm_batch_set_state(self._h, qp, vp, fp, mp, k), self._L)

    def reset(self, mode=0, hard=1, mask=None):
        mp, k, _ = self._ptr(mask, np.uint8, (self.n,))
        A.check(self._L.dm_batch_reset(self._h, int(mode), int(hard), mp, k), self._L)

    def push(self, body, impulse, mask=None):
        """External pushes through dm_batch_push (one launch, now): env e's velocity takes the impulse[e] (N s, world frame) applied at the centre of mass of
        model body body[e] (1..13), dqvel = M^-1 J_b^T p with the step's own mass matrix; body[e] == 0 or mask[e] == 0 leaves env e untouched, bit for bit.
        body [n] int32, impulse [n,3] float64, mask [n] uint8: numpy arrays (a body outside 0..13 or a non-finite impulse raises) or tensors on the
        batch's device (stream-ordered, not read back: such an env is left untouched).  Only qvel changes."""
        n = self.n
        bp, k0, _a = self._ptr(body, np.int32, (n,)); ip, k1, _b = self._ptr(impulse, np.float64, (n, 3)); mp, k2, _c = self._ptr(mask, np.uint8, (n,))
        if len({k0, k1} | ({k2} if mask is not None else set())) != 1:
            raise ValueError("push buffers must be all numpy arrays or all device tensors")
        A.check(self._L.dm_batch_push(self._h, bp, ip, mp, k0), self._L)

    def set_push_schedule(self, schedule):
        """The random push schedule through dm_batch_set_push_schedule: a perturb.PushSchedule (or what PushSchedule.coerce takes); None: off.  While one
        is set every per-step launch is preceded by the schedule's launch (k_push), and rollouts and queued steps run as step launches.  Setting it clears
        the schedule's records (F_PUSH_STATE, F_PUSH_FORCE)."""
        from .perturb import PushSchedule
        schedule = PushSchedule.coerce(schedule)
        A.check(self._L.dm_batch_set_push_schedule(self._h, None if schedule is None else C.byref(schedule.desc())), self._L)
        self.push_schedule = schedule

    def get(self, field, out=None):
        dt, shp = A.FIELD_SPEC[field]
        if out is None:
            out = np.empty((self.n,) + shp, dtype=dt)
        p, kind, _ = self._ptr(out, dt, (self.n,) + shp, out=True)
        nbytes = int(np.prod((self.n,) + shp)) * np.dtype(dt).itemsize
        A.check(self._L.dm_batch_get(self._h, int(field), p, nbytes, kind), self._L)
        return out

    def set(self, field, value):
        dt, shp = A.FIELD_SPEC[field]
        if not _is_torch(value):
            value = np.ascontiguousarray(np.asarray(value, dtype=dt).reshape((self.n,) + shp))
        p, kind, _ka = self._ptr(value, dt, (self.n,) + shp)
        nbytes = int(np.prod((self.n,) + shp)) * np.dtype(dt).itemsize
        A.check(self._L.dm_batch_set(self._h, int(field), p, nbytes, kind), self._L)

    def debug_forward(self, env=0):
        buf = np.zeros(A.DEBUG_DOUBLES)
        A.check(self._L.dm_batch_debug_forward(self._h, int(env), buf.ctypes.data_as(A._dp)), self._L)
        return A.parse_debug(buf)

    def enable_timing(self, on=True):
        A.check(self._L.dm_batch_enable_timing(self._h, 1 if on else 0), self._L)

    def last_step_ms(self):
        ms = C.c_float(0)
        A.check(self._L.dm_batch_last_step_ms(self._h, C.byref(ms)), self._L)
        return float(ms.value)

    def read_profile(self):
        """[N,32] int64 shader-clock cycles of the last step: kin, mass, bias, rows, constraint, total, nefc, sweeps | 8..13 the
        constraint stage's parts | 16..23 the collision stage's parts, 24..27 its near-pair counts (include/dmenv.h)."""
        out = np.zeros((self.n, 32), dtype=np.int64)
        A.check(self._L.dm_batch_read_profile(self._h, out.ctypes.data_as(C.POINTER(C.c_longlong))), self._L)
        return out

    def redo_total(self):
        """env-steps the four-envs-per-wave path (option 105) handed to the one-env kernel so far"""
        return self.redo_reasons()[0]

    def redo_reasons(self):
        """[total, then by reason: > PACKED_MAXCAND pairs past the bounding spheres, box staging slots, > PACKED_MAXCON contacts (or > PACKED_MAXFRAME
        contact pairs), > PACKED_MAXROWS rows (or > PACKED_MAXLIMROWS limits), PGS cost test] env-steps handed to the one-env code (_abi.PACKED_*)"""
        v = (C.c_int64 * 8)()
        A.check(self._L.dm_batch_redo_total(self._h, v), self._L)
        return [int(x) for x in v[:6]]

    def sync(self):
        A.check(self._L.dm_batch_sync(self._h), self._L)
        if self._queue_refs:
            del self._queue_refs[:]

    def join(self):
        """Run the steps OPT_STEP_QUEUE has queued and make the batch's stream wait for every pipelined step launch still in flight
        (OPT_PIPELINE > 1), without a host wait.  Call before consuming the outputs of queued / pipelined `step` calls on that stream."""
        A.check(self._L.dm_batch_join(self._h), self._L)
