"""Build libdmenv.so (HIP, gfx950) in-tree with hipcc.  Usage: python -m deepmimic_mujoco_amd.csrc.build [--force]"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
SOURCES = ["dmenv.hip", "views.hip", "learner.hip", "kernels_packed.hip", "kernels_rollout.hip", "kernels_rollout_term.hip", "kernels_rollout_spd.hip", "kernels_spd.hip", "kernels_packed_spd.hip", "kernels_clips.hip", "kernels_packed_clips.hip", "kernels_push.hip", "push_kernel.h", "packed_body.h", "host_common.h", "batch_host.h", "kernels.h", "env_kernel.h", "step_rules.h", "env_step.h", "model_host.h", "topology.h", "wave.h", "policy_kernel.h", "policy_wave_launch_order.h", "rng.h", "mlp_tile.h", "vf_kernel.h", "pg_kernel.h", "disc_kernel.h", "slot_kernel.h", "slot_step.h", "slot_term.h", "render.h", "render_kernel.h", "state_features.h", "state_kernel.h", "floor_contact.h", "term_kernel.h", "terms_kernel.h", "view_stage.h"]
OUT = os.path.join(HERE, "libdmenv.so")
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-shift-count-negative", "-Wno-implicit-const-int-float-conversion"]
# Twelve translation units (kernels.h lists them), each with the backend options its kernels want (round 4, A/B in profiles/r04_ab_kernel_variants.md):
#   kernels_packed.hip — four environments per wavefront: ONE wave per SIMD with the whole register file.  The default scheduling strategy (max-occupancy: keep
#                        register pressure low) buys nothing there; scheduling for instruction-level parallelism hides more of a lone wave's LDS / f64 latencies
#                        (+1.0 .. +1.6 % env-steps/s), register-class priority in the greedy allocator +0.4 %.
#   dmenv.hip          — the one-env step kernels (two waves per SIMD at 256 registers: 2 % SLOWER under max-ilp), the reset / state / view kernels, the batch half of
#                        the C ABI: defaults.  views.hip (render / state features, host side) and learner.hip (the learner kernels and their entry points): defaults too.
# Neither option touches floating-point semantics: results are bit-identical.
#                        -enable-ipra (round 6): inter-procedural register allocation — the horizon launch's called step bodies (internal functions, slot_step.h
#                        DM_CALL_SLOT) are compiled without callee-saved registers: no 337-register save / restore per call, +3.7 % (profiles/r06_ab_kernel_variants.md §4).
PACKED_FLAGS = ["-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-greedy-regclass-priority-trumps-globalness=1", "-mllvm", "-enable-ipra"]
if os.environ.get("DM_PACKED_FLAGS") is not None:      # experiments: replace the packed unit's backend options altogether (tools/build_variant.sh)
    PACKED_FLAGS = os.environ["DM_PACKED_FLAGS"].split()
#   kernels_rollout.hip — k_rollout_packed and its called step bodies: the packed options + the IR-level load-store vectoriser off (round 6: +0.8 .. +1.4 % on the
#                        horizon launch, -1 % on the per-step packed kernel, hence a unit of its own).
#                        -amdgpu-use-amdgpu-trackers: the backend's own register-pressure trackers in the scheduler: +0.5 .. +1.3 % there (section 17 of the same file).
ROLLOUT_FLAGS = PACKED_FLAGS + ["-mllvm", "-amdgpu-load-store-vectorizer=false", "-mllvm", "-amdgpu-use-amdgpu-trackers=true"]
if os.environ.get("DM_ROLLOUT_FLAGS") is not None:
    ROLLOUT_FLAGS = os.environ["DM_ROLLOUT_FLAGS"].split()
#   kernels_rollout_term.hip — k_rollout_packed_term (the horizon launch with early termination inside: slot_term.h) with the same options, beside it: k_rollout_packed's code object is not touched.
#   kernels_rollout_spd.hip — the two horizon launches of action modes 3 and 4 (DM_OPT_HORIZON_SPD), likewise: the same options, beside them.
#   kernels_spd.hip / kernels_packed_spd.hip — the step kernels of action modes 3 and 4, with the options of the units whose kernels they mirror.
#   kernels_clips.hip / kernels_packed_clips.hip — the kernels of multi-clip batches (one clip per env), likewise.
#   kernels_push.hip — the two launches of external pushes (push_kernel.h), one wave per env: defaults.
UNITS = [("dmenv.hip", []), ("views.hip", []), ("learner.hip", []), ("kernels_packed.hip", PACKED_FLAGS), ("kernels_rollout.hip", ROLLOUT_FLAGS), ("kernels_rollout_term.hip", ROLLOUT_FLAGS), ("kernels_rollout_spd.hip", ROLLOUT_FLAGS), ("kernels_spd.hip", []), ("kernels_packed_spd.hip", PACKED_FLAGS), ("kernels_clips.hip", []), ("kernels_packed_clips.hip", PACKED_FLAGS), ("kernels_push.hip", [])]


def hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm)")


OUT32 = os.path.join(HERE, "libdmenv32.so")
# The float32 library contracts a multiply and an add into an FMA only where they stand in ONE source expression (-ffp-contract=on; hipcc's default,
# `fast`, lets the backend fuse across expressions wherever inlining brings a product and a sum together).  Its cross-lane and PGS primitives are
# compiler-visible C++ (csrc/wave.h; the float64 forms are inline assembly), and the step is instantiated several times — lean / three-set, per-step /
# horizon, the position stage once in the step and once in the 5-term reward — so under `fast` the instantiations rounded differently: results depended
# on the launch form and on which environments shared a wave (tests/test_gpu_float32.py: 226 of 256 envs differed between the step queue's horizon
# launch and unqueued packed steps in reward mode 3).  With `on` every copy of a formula is the same arithmetic and the packed forms agree bit for bit, as
# include/dmenv.h promises.  The float64 library's commands are unchanged.
FLOAT32_DEFS = ["-DDM_REAL_FLOAT", "-ffp-contract=on"]

def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def build_one(out, defs=(), extra=(), verbose=False, objdir=None):
    """Compile the translation units side by side and link them into `out`.  defs: extra -D... for every unit; extra: extra compiler options for every unit."""
    objdir = objdir or os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    tag = os.path.splitext(os.path.basename(out))[0]
    jobs, objs = [], []
    for src, flags in UNITS:
        obj = os.path.join(objdir, "%s_%s.o" % (tag, os.path.splitext(src)[0]))
        flags = list(flags) + os.environ.get("DM_FLAGS_" + os.path.splitext(src)[0].upper(), "").split()      # experiments: DM_FLAGS_DMENV / DM_FLAGS_KERNELS_PACKED
        cmd = [hipcc()] + COMMON + list(flags) + list(defs) + list(extra) + ["-I" + os.path.join(REPO, "include"), "-I" + HERE, "-c", os.path.join(HERE, src), "-o", obj]
        if verbose:
            cmd.insert(-4, "-Rpass-analysis=kernel-resource-usage")
            print(" ".join(cmd))
        jobs.append((cmd, subprocess.Popen(cmd))); objs.append(obj)
    for cmd, pr in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    link = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out]
    subprocess.check_call(link)
    return out


def build(force=False, verbose=False):
    """libdmenv.so (float64 arithmetic: the parity build) and libdmenv32.so (FLOAT32_DEFS: the same kernels in float32, the
    `dtype 32` batch), compiled side by side.  Returns the path of libdmenv.so."""
    import threading
    srcs = [os.path.join(HERE, s) for s in SOURCES] + [os.path.join(REPO, "include", "dmenv.h"), os.path.abspath(__file__)]      # (this file: the units' backend options)
    extra = os.environ.get("DM_BUILD_DEFINES", "").split()
    todo = [(out, defs) for out, defs in ((OUT, []), (OUT32, FLOAT32_DEFS)) if force or _stale(out, srcs)]
    errs = []

    def run(out, defs):
        try:
            build_one(out, defs, extra, verbose)
        except Exception as e:       # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=run, args=t) for t in todo]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    return OUT


if __name__ == "__main__":
    if "--out" in sys.argv:        # python build.py --out build_ab/X.so [compiler options ...]: one float64 library with extra options (A/B builds: tools/build_variant.sh)
        i = sys.argv.index("--out")
        print(build_one(os.path.abspath(sys.argv[i + 1]), extra=sys.argv[i + 2:], objdir=os.path.join(os.path.dirname(os.path.abspath(sys.argv[i + 1])), "obj")))
    else:
        print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))
