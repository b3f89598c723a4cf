"""Python front end of the wave testbench for EXTERNAL PUSHES (TEST INFRASTRUCTURE): the push kernels' waves on CPU fibres, behind the interface of
deepmimic_mujoco_amd.batch.Batch (push, set_push_schedule, the two push fields) that the push tests use."""
import ctypes as C
import os

import numpy as np

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.perturb import PushSchedule
from tests.emu.emu import EmuBatch, load_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_u8p = C.POINTER(C.c_uint8)


def lib():
    global _LIB
    if _LIB is None:
        L = load_lib(_HERE, "libdmemu_push.so")        # (with the prototypes of the EmuBatch entry points compiled into this library)
        L.emup_push.argtypes = [C.c_void_p, A._ip, A._dp, _u8p]
        L.emup_schedule.argtypes = [C.c_void_p, C.POINTER(A.PushDesc), A._ip, A._dp, C.c_double]
        _LIB = L
    return _LIB


class EmuPushBatch(EmuBatch):
    """An EmuBatch (of this library) with the push entry points; the schedule's launch precedes every step while one is set, as in dm_batch_step."""

    def __init__(self, cm, data_config, data_vel, n_envs, flags=0, mocap_dt=0.033332):
        self.n = n_envs
        self.cm = cm
        md, self._keep = A.make_model_desc(cm)
        cfg = np.ascontiguousarray(data_config, dtype=np.float64); vel = np.ascontiguousarray(data_vel, dtype=np.float64)
        self.h = lib().emu_create(C.byref(md), cfg.ctypes.data_as(A._dp), vel.ctypes.data_as(A._dp), cfg.shape[0], n_envs, flags, float(mocap_dt))
        if not self.h:
            raise RuntimeError("emu_create failed")
        self.push_schedule = None
        self._push_state = np.zeros((n_envs, 5), dtype=np.int32); self._push_state[:, 0] = -1
        self._push_force = np.zeros((n_envs, 3))

    def __del__(self):
        if getattr(self, "h", None):
            lib().emu_destroy(self.h); self.h = None

    def set_option(self, opt, value):
        lib().emu_set_option(self.h, opt, int(value))

    def _view(self, field):
        if field == A.F_PUSH_STATE:
            return self._push_state
        if field == A.F_PUSH_FORCE:
            return self._push_force
        dt, shp = A.FIELD_SPEC[field]
        p = lib().emu_field(self.h, field)
        n = int(np.prod((self.n,) + shp))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double if dt == np.float64 else C.c_int32)), shape=(n,)).reshape((self.n,) + shp)

    def set(self, field, value):
        self._view(field)[...] = np.asarray(value).reshape(self._view(field).shape)
        if field == A.F_QPOS:
            lib().emu_invalidate_kin(self.h)

    def push(self, body, impulse, mask=None):
        b = np.ascontiguousarray(body, dtype=np.int32).reshape(self.n); p = np.ascontiguousarray(impulse, dtype=np.float64).reshape(self.n, 3)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().emup_push(self.h, b.ctypes.data_as(A._ip), p.ctypes.data_as(A._dp), None if m is None else m.ctypes.data_as(_u8p))

    def set_push_schedule(self, schedule):
        self.push_schedule = PushSchedule.coerce(schedule)
        self._push_state[...] = 0; self._push_state[:, 0] = -1; self._push_force[...] = 0

    def step(self, action, n_substeps=1, out=None):
        if self.push_schedule is not None:
            d = self.push_schedule.desc()
            lib().emup_schedule(self.h, C.byref(d), self._push_state.ctypes.data_as(A._ip), self._push_force.ctypes.data_as(A._dp),
                                float(self.cm.timestep) * float(n_substeps))
        a = np.ascontiguousarray(action, dtype=np.float64).reshape(self.n, A.NU)
        if out is None:
            out = (np.zeros((self.n, A.NOBS)), np.zeros(self.n), np.zeros(self.n, dtype=np.uint8))
        obs, rew, done = out
        lib().emu_step(self.h, a.ctypes.data_as(A._dp), obs.ctypes.data_as(A._dp), rew.ctypes.data_as(A._dp), done.ctypes.data_as(_u8p), n_substeps)
        return obs, rew, done

    def set_state(self, qpos, qvel, frame_idx=None, mask=None):
        q = np.ascontiguousarray(qpos, dtype=np.float64).reshape(self.n, A.NQ); v = np.ascontiguousarray(qvel, dtype=np.float64).reshape(self.n, A.NV)
        f = None if frame_idx is None else np.ascontiguousarray(frame_idx, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().emu_set_state(self.h, q.ctypes.data_as(A._dp), v.ctypes.data_as(A._dp), None if f is None else f.ctypes.data_as(A._ip),
                            None if m is None else m.ctypes.data_as(_u8p))

    def reset(self, mode=0, hard=1, mask=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        lib().emu_reset(self.h, mode, hard, None if m is None else m.ctypes.data_as(_u8p))

    def rollout(self, actions, n_substeps=1):
        raise NotImplementedError

    def redo_total(self):
        raise NotImplementedError

    def debug_forward(self, env=0):
        raise NotImplementedError
