"""Stand-alone host programs of the test suite (TEST INFRASTRUCTURE): the compiler command line of tests/*_host.cpp, and the input format of the two
horizon twins (tests/emu/host_rollout.h read_input / read_model)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))


def build_host(src, out_path, testbench=False, sanitize=False, opt=("-O2",), abi=False):
    """Compiles tests/<src> to out_path and returns out_path.  opt: the optimisation and debug flags; testbench: the kernel source on the wave testbench
    (tests/emu's headers, unfused arithmetic); sanitize: AddressSanitizer and UBSan, every report fatal; abi: include/dmenv.h on the include path (the
    testbench has it anyway)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build tests/%s" % src)
    cmd = [cxx] + list(opt) + ["-std=c++17"]
    if testbench:
        cmd += ["-DDM_WAVE_TESTBENCH", "-ffp-contract=off", "-Wno-unknown-pragmas"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if testbench:
        cmd += ["-I" + os.path.join(ROOT, "tests", "emu")]
    cmd += ["-I" + os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc")]
    if testbench or abi:
        cmd += ["-I" + os.path.join(ROOT, "include")]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", src), "-o", str(out_path)])
    return str(out_path)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


def model_arrays(cm, mocap_dt):
    """the compiled model as read_model reads it: the sizes, the 27 tables in _abi.make_model_desc's order, then the scalars row (with the mocap clip's dt)"""
    return [i32([cm.nbody, cm.njnt, cm.nq, cm.nv, cm.nu, cm.ngeom, cm.npair, cm.iterations]),
            i32(cm.body_parentid), i32(cm.body_dofnum), f64(cm.body_pos), f64(cm.body_ipos), f64(cm.body_mass), f64(cm.body_inertia), f64(cm.body_invweight0),
            i32(cm.jnt_type), i32(cm.jnt_bodyid), i32(cm.jnt_limited), f64(cm.jnt_axis), f64(cm.jnt_range),
            f64(cm.dof_armature), f64(cm.dof_damping), f64(cm.dof_invweight0),
            i32(cm.geom_type), i32(cm.geom_bodyid), i32(cm.geom_condim), f64(cm.geom_pos), f64(cm.geom_mat), f64(cm.geom_size), f64(cm.geom_margin), f64(cm.geom_friction),
            i32(cm.pair_geom), i32(cm.actuator_dofid), f64(cm.actuator_gear), f64(cm.actuator_ctrlrange),
            f64([cm.timestep] + list(cm.gravity) + [cm.tolerance] + list(cm.solref) + list(cm.solimp) + [cm.meaninertia, float(mocap_dt)])]


def write_arrays(path, arrays):
    """a sequence of arrays (each from i32 or f64), each written as {int32 kind (0: int32, 1: float64), int64 count, data}"""
    with open(path, "wb") as f:
        for a in arrays:
            assert a.dtype in (np.int32, np.float64) and a.ndim == 1
            f.write(np.int32(0 if a.dtype == np.int32 else 1).tobytes()); f.write(np.int64(a.size).tobytes()); f.write(a.tobytes())
