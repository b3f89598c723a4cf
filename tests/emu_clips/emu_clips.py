"""Python front end of the wave testbench for MULTI-CLIP batches (TEST INFRASTRUCTURE): the clip instantiations of the step and reset
routines on CPU fibres, behind the interface of deepmimic_mujoco_amd.batch.Batch(..., clips=ClipSet) that the clip tests use."""
import ctypes as C
import os

import numpy as np

from deepmimic_mujoco_amd import _abi as A
from tests.emu.emu import EmuBatch, load_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_u8p = C.POINTER(C.c_uint8)


def lib():
    global _LIB
    if _LIB is None:
        L = load_lib(_HERE, "libdmemu_clips.so")        # (with the prototypes of the EmuBatch entry points compiled into this library)
        L.emuc_create.restype = C.c_void_p
        L.emuc_create.argtypes = [C.POINTER(A.ModelDesc), A._dp, A._dp, C.c_int, C.c_int, C.c_uint, C.c_int, A._ip, A._ip, A._dp, A._dp]
        L.emuc_set_imitation.argtypes = [C.c_void_p, A._dp, A._dp, A._dp, A._dp, A._dp]
        L.emuc_destroy.argtypes = [C.c_void_p]
        L.emuc_batch.restype = C.c_void_p; L.emuc_batch.argtypes = [C.c_void_p]
        L.emuc_clip.restype = C.POINTER(C.c_int32); L.emuc_clip.argtypes = [C.c_void_p]
        L.emuc_set_clip_mode.argtypes = [C.c_void_p, C.c_int]
        L.emuc_step.argtypes = [C.c_void_p, A._dp, A._dp, A._dp, _u8p, C.c_int]
        L.emuc_reset.argtypes = [C.c_void_p, C.c_int, C.c_int, _u8p]
        _LIB = L
    return _LIB


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class EmuClipBatch(EmuBatch):
    """A multi-clip batch on the testbench: `clips` is a deepmimic_mujoco_amd.clips.ClipSet."""

    def __init__(self, cm, clips, n_envs, flags=0):
        self.n = n_envs
        self.clips = clips
        self.options = {}
        md, self._keep = A.make_model_desc(cm)
        K = len(clips)
        cfg, vel = _d(clips.data_config), _d(clips.data_vel)
        row0 = np.ascontiguousarray(clips.row0, dtype=np.int32); nf = np.ascontiguousarray(clips.n_frames, dtype=np.int32)
        dt, cdf = _d(clips.dt), _d(clips.cdf)
        self.hc = lib().emuc_create(C.byref(md), cfg.ctypes.data_as(A._dp), vel.ctypes.data_as(A._dp), cfg.shape[0], n_envs, flags, K,
                                    row0.ctypes.data_as(A._ip), nf.ctypes.data_as(A._ip), dt.ctypes.data_as(A._dp), cdf.ctypes.data_as(A._dp))
        if not self.hc:
            raise RuntimeError("emuc_create failed")
        self.hb = lib().emuc_batch(self.hc)
        if clips.imitation is not None:
            rec = clips.records()
            tab, par = _d(clips.imit_table), _d(clips.imitation[0][1])
            loop, sx, sy = (_d([r[k] for r in rec]) for k in ("loop", "shift_x", "shift_y"))
            lib().emuc_set_imitation(self.hc, tab.ctypes.data_as(A._dp), par.ctypes.data_as(A._dp), loop.ctypes.data_as(A._dp), sx.ctypes.data_as(A._dp),
                                     sy.ctypes.data_as(A._dp))

    def __del__(self):
        if getattr(self, "hc", None):
            lib().emuc_destroy(self.hc); self.hc = None

    def set_option(self, opt, value):
        self.options[int(opt)] = int(value)
        if opt == A.OPT_CLIP_MODE:
            lib().emuc_set_clip_mode(self.hc, int(value))
            return
        lib().emu_set_option(self.hb, opt, int(value))
        if opt == A.OPT_ENV_OFFSET:            # the default assignment follows the global env id, as in dm_batch_set_option
            self._clip_view()[...] = self.clips.default_assignment(self.n, value)

    def _clip_view(self):
        return np.ctypeslib.as_array(lib().emuc_clip(self.hc), shape=(self.n,))

    def _view(self, field):
        if field == A.F_CLIP:
            return self._clip_view()
        dt, shp = A.FIELD_SPEC[field]
        p = lib().emu_field(self.hb, field)
        n = int(np.prod((self.n,) + shp))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double if dt == np.float64 else C.c_int32)), shape=(n,)).reshape((self.n,) + shp)

    def set(self, field, value):
        self._view(field)[...] = np.asarray(value).reshape(self._view(field).shape)
        if field in (A.F_QPOS, A.F_CLIP):
            lib().emu_invalidate_kin(self.hb)
        if field == A.F_CLIP:                   # dm_batch_set's k_clip_clamp: cursors that name a table row stay inside the new clip
            last = np.asarray(self.clips.n_frames)[self._clip_view()] - 1
            init = self._view(A.F_FRAME_INIT); init[...] = np.minimum(init, last)
            if self.options.get(A.OPT_REWARD_MODE, 0) not in (2, 4):
                idx = self._view(A.F_FRAME_IDX); idx[...] = np.minimum(idx, last)

    def step(self, action, n_substeps=1, out=None):
        a = _d(action).reshape(self.n, A.NU)
        if out is None:
            out = (np.zeros((self.n, A.NOBS)), np.zeros(self.n), np.zeros(self.n, dtype=np.uint8))
        obs, rew, done = out
        lib().emuc_step(self.hc, a.ctypes.data_as(A._dp), obs.ctypes.data_as(A._dp), rew.ctypes.data_as(A._dp), done.ctypes.data_as(_u8p), n_substeps)
        return obs, rew, done

    def rollout(self, actions, n_substeps=1):
        """a multi-clip batch's horizon is step launches (dmenv.hip rollout_as_one_launch)"""
        outs = [self.step(a, n_substeps) for a in np.asarray(actions)]
        return tuple(np.stack([o[k] for o in outs]) for k in range(3))

    def set_state(self, qpos, qvel, frame_idx=None, mask=None):
        q, v = _d(qpos).reshape(self.n, A.NQ), _d(qvel).reshape(self.n, A.NV)
        f = None if frame_idx is None else np.ascontiguousarray(frame_idx, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().emu_set_state(self.hb, q.ctypes.data_as(A._dp), v.ctypes.data_as(A._dp), None if f is None else f.ctypes.data_as(A._ip),
                            None if m is None else m.ctypes.data_as(_u8p))

    def reset(self, mode=0, hard=1, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().emuc_reset(self.hc, mode, hard, None if m is None else m.ctypes.data_as(_u8p))

    def redo_total(self):
        raise NotImplementedError

    def debug_forward(self, env=0):
        raise NotImplementedError
