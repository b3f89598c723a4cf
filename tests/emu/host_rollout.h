// host_rollout.h — TEST INFRASTRUCTURE: what the two horizon twins (tests/term_rollout_host.cpp, tests/spd_rollout_host.cpp) share on top of host_batch.h:
// what the host compiler needs to read k_terminate, the termination launch, the input file and the model description in it, the output rows of a run and the
// bit-for-bit comparison of two runs.  The twins are stand-alone programs built with -fsanitize=address,undefined; a twin keeps its Config, its tallies, the
// conditions its run must meet and main().
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// a fibre's stack under the sanitizers: kept small, and its high-water mark checked at the end of main() (wave_fibres.h says why)
#define DM_FIBRE_STACK (1 << 18)
#include "wave_fibres.h"

// k_terminate is a kernel: what the host compiler needs to read its definition, and the one atomic it uses
#define __global__
#define __shared__ static
#define __launch_bounds__(n)
struct Dim3 { unsigned x, y, z; };
static Dim3 blockIdx, blockDim, threadIdx;
static inline int atomicAdd(int* p, int v) { const int o = *p; *p = o + v; return o; }
typedef double Real;
typedef double Ext;

#include "host_batch.h"
// k_terminate hands a value from lane 0 to the wave with dmw::uniform: a readfirstlane on the device, the identity on the testbench (where every lane of the
// kernels written so far held the value already).  For the termination launch's kernel alone it is lane 0's value, as on the device.
namespace dmw { inline int uniform_from_lane0(int v) { return exchange(v, 0); } }
#define uniform uniform_from_lane0
#include "term_kernel.h"       // TermArgs and the termination launch's kernel ...
#undef uniform
#include "slot_term.h"         // ... and the horizon launch's phase

namespace {
// the input: a sequence of arrays, each { int32 kind (0: int32, 1: float64), int64 count, data }, handed out in the file's order per kind
struct Input {
  std::vector<std::vector<int>> I;
  std::vector<std::vector<double>> D;
  size_t ni = 0, nd = 0;
  const std::vector<int>& i() { return I.at(ni++); }
  const std::vector<double>& d() { return D.at(nd++); }
};
bool read_input(const char* path, Input& in) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  for (;;) {
    int kind; long long cnt;
    if (std::fread(&kind, 4, 1, f) != 1) break;
    if (std::fread(&cnt, 8, 1, f) != 1 || cnt < 0 || (kind != 0 && kind != 1)) { std::fclose(f); return false; }
    if (kind == 0) { std::vector<int> v((size_t)cnt); if (cnt && std::fread(v.data(), 4, (size_t)cnt, f) != (size_t)cnt) { std::fclose(f); return false; } in.I.push_back(v); }
    else { std::vector<double> v((size_t)cnt); if (cnt && std::fread(v.data(), 8, (size_t)cnt, f) != (size_t)cnt) { std::fclose(f); return false; } in.D.push_back(v); }
  }
  std::fclose(f);
  return true;
}

// the model (include/dmenv.h dm_model_desc): sizes, the int tables, the float tables, the scalars — in _abi.make_model_desc's order, as
// tests/emu/hostprog.py model_arrays writes them.  d points into `in`; scalars: timestep, gravity [3], tolerance, solref [2], solimp [5], meaninertia, mocap_dt
void read_model(Input& in, dm_model_desc& d, std::vector<double>& scalars) {
  const std::vector<int>& sz = in.i();
  d.abi_version = DM_ABI_VERSION;
  d.nbody = sz.at(0); d.njnt = sz.at(1); d.nq = sz.at(2); d.nv = sz.at(3); d.nu = sz.at(4); d.ngeom = sz.at(5); d.npair = sz.at(6); d.iterations = sz.at(7);
  d.body_parentid = in.i().data(); d.body_dofnum = in.i().data();
  d.body_pos = in.d().data(); d.body_ipos = in.d().data(); d.body_mass = in.d().data(); d.body_inertia = in.d().data(); d.body_invweight0 = in.d().data();
  d.jnt_type = in.i().data(); d.jnt_bodyid = in.i().data(); d.jnt_limited = in.i().data(); d.jnt_axis = in.d().data(); d.jnt_range = in.d().data();
  d.dof_armature = in.d().data(); d.dof_damping = in.d().data(); d.dof_invweight0 = in.d().data();
  d.geom_type = in.i().data(); d.geom_bodyid = in.i().data(); d.geom_condim = in.i().data(); d.geom_pos = in.d().data(); d.geom_mat = in.d().data();
  d.geom_size = in.d().data(); d.geom_margin = in.d().data(); d.geom_friction = in.d().data();
  d.pair_geom = in.i().data();
  d.actuator_dofid = in.i().data(); d.actuator_gear = in.d().data(); d.actuator_ctrlrange = in.d().data();
  scalars = in.d();
  const std::vector<double>& sc = scalars;
  d.timestep = sc.at(0); for (int k = 0; k < 3; k++) d.gravity[k] = sc.at(1 + k);
  d.tolerance = sc.at(4); d.solref[0] = sc.at(5); d.solref[1] = sc.at(6); for (int k = 0; k < 5; k++) d.solimp[k] = sc.at(7 + k);
  d.meaninertia = sc.at(12);
}

TermArgs term_args(HostBatch& e, int fall, int limit, int log_cap, int tick) {
  return TermArgs{e.steps.data(), e.reason.data(), (unsigned)fall, limit, 0, e.n, e.log_count.data(), e.log_index.data(), e.log_qpos.data(), e.log_qvel.data(), log_cap, tick};
}
// the termination launch: k_terminate's own body (csrc/term_kernel.h), one environment per wave
void terminate_launch(HostBatch& e, const TermArgs& ta, double* obs, unsigned char* done) {
  for (int env = 0; env < e.n; env++) {
    blockIdx.x = (unsigned)env;
    run_wave([&](int) { k_terminate(&e.M, e.B, ta, obs, done); });
  }
}

// a run's output rows: obs [T, n, 56], reward / done [T, n]
struct Rows {
  std::vector<double> obs, rew; std::vector<unsigned char> done;
  Rows(int T, int n) : obs((size_t)T * n * NOBS, 0), rew((size_t)T * n, 0), done((size_t)T * n, 0) {}
};

template <class T> bool same(const char* prog, const char* what, const std::vector<T>& a, const std::vector<T>& b, int per) {
  if (a.size() != b.size()) { std::fprintf(stderr, "%s: %s: sizes differ\n", prog, what); return false; }
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) {
      std::fprintf(stderr, "%s: %s differs at element %zu (row %zu, column %zu): %.17g against %.17g\n", prog, what, i, i / (size_t)per, i % (size_t)per, (double)a[i], (double)b[i]);
      return false;
    }
  return true;
}

// two runs of one batch, bit for bit: every output row, the final state (DM_F_CTRL included), the counters, the reasons and the parked-kinematics flags
bool compare(const char* prog, const char* tag, const HostBatch& a, const HostBatch& b, const Rows& ra, const Rows& rb) {
  const std::string t(tag);
  auto eq = [&](const char* field, const auto& x, const auto& y, int per) { return same(prog, (t + field).c_str(), x, y, per); };
  return eq(" obs", ra.obs, rb.obs, NOBS) && eq(" reward", ra.rew, rb.rew, a.n) && eq(" done", ra.done, rb.done, a.n) &&
         eq(" qpos", a.qpos, b.qpos, NQ) && eq(" qvel", a.qvel, b.qvel, NV) && eq(" qacc_warmstart", a.qws, b.qws, NV) && eq(" ctrl", a.ctrl, b.ctrl, NU) &&
         eq(" time", a.time, b.time, 1) && eq(" frame_idx", a.fidx, b.fidx, 1) && eq(" frame_init", a.finit, b.finit, 1) &&
         eq(" cycle", a.cycle, b.cycle, 1) && eq(" episode", a.episode, b.episode, 1) && eq(" episode_steps", a.steps, b.steps, 1) &&
         eq(" done_reason", a.reason, b.reason, 1) && eq(" parked-kinematics flags", a.kin_ok, b.kin_ok, 1);
}
}  // namespace
