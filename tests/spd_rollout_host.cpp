// Host twin of the horizon launch in action modes 3 and 4 (DM_OPT_HORIZON_SPD: csrc/kernels_rollout_spd.hip, slot_step.h's SPD switch) for
// tests/test_horizon_spd.py: the unmodified kernel source on the fibre wave testbench (tests/emu/wave_testbench.h), built with -fsanitize=address,undefined.
// One batch is stepped through a horizon twice from the same states and actions:
//   (a) as the step launches do it: per step the packed step (three-set code, the controller compiled in, no carried kinematics) of every wave, the one-env
//       re-step with the controller of the environments beyond its capacities, then — the termination runs — k_terminate's own body, one environment per wave;
//   (b) as k_rollout_packed_spd / k_rollout_packed_term_spd do it: slot_rollout with the SPD switch on, one wave after another, without / with slot_term.h's phase.
// and every output row, the final state (DM_F_CTRL included), the counters and the reasons are compared bit for bit: action mode 4, then mode 3, each
// without and with the termination phase.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: spd_rollout_host IN OUT
//   IN   a sequence of arrays, each { int32 kind (0: int32, 1: float64), int64 count, data }, in the order main() reads them
//   OUT  float64, for mode 4 then mode 3: the termination run (a)'s state after every step's step launches, ahead of termination (qpos [T, n, 35]) and that
//        step's own done [T, n], for the test's input condition (no fall decision within rounding of its boundary)
//   exit status 0 and a summary line per run when everything agrees and every horizon held a step taken with carried kinematics, an in-wave re-step of the
//   environment that starts in the many-row state, and an auto-reset that a later step follows; else the first difference on stderr and 1
#include <ucontext.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "wave_testbench.h"

// k_terminate is a kernel: what the host compiler needs to read its definition, and the one atomic it uses
#define __global__
#define __shared__ static
#define __launch_bounds__(n)
struct Dim3 { unsigned x, y, z; };
static Dim3 blockIdx, blockDim, threadIdx;
static inline int atomicAdd(int* p, int v) { const int o = *p; *p = o + v; return o; }
typedef double Real;
typedef double Ext;

// kernel source, unmodified
#include "env_step.h"
#include "slot_step.h"
#include "model_host.h"
using namespace dm;
// (k_terminate's dmw::uniform is lane 0's value, as on the device: tests/term_rollout_host.cpp)
namespace dmw { inline int uniform_from_lane0(int v) { return exchange(v, 0); } }
#define uniform uniform_from_lane0
#include "term_kernel.h"       // TermArgs and the termination launch's kernel ...
#undef uniform
#include "slot_term.h"         // ... and the horizon launch's phase

namespace dmw {
static WaveBench g_bench;
WaveBench& bench() { return g_bench; }
}  // namespace dmw

namespace {
// (a fibre's stack: kept small for the sanitizer's swapcontext, its high-water mark checked at the end — tests/term_rollout_host.cpp)
constexpr size_t STACK = 1 << 18;
constexpr unsigned char STACK_FILL = 0xA5;
ucontext_t g_main, g_fib[64];
bool g_done[64];
std::function<void(int)>* g_body;
char* g_stacks;

void yield_to_main() { swapcontext(&g_fib[dmw::g_bench.cur_lane], &g_main); }
void fibre_entry() {
  const int l = dmw::g_bench.cur_lane;
  (*g_body)(l);
  g_done[l] = true;
  swapcontext(&g_fib[l], &g_main);
}
// run body(lane) on 64 fibres to completion
void run_wave(std::function<void(int)> body) {
  if (!g_stacks) { g_stacks = (char*)malloc(STACK * 64); std::memset(g_stacks, STACK_FILL, STACK * 64); }
  g_body = &body;
  dmw::g_bench.arrived = 0; dmw::g_bench.gen = 0; dmw::g_bench.yield_fn = yield_to_main;
  for (int l = 0; l < 64; l++) {
    g_done[l] = false;
    getcontext(&g_fib[l]);
    g_fib[l].uc_stack.ss_sp = g_stacks + STACK * l; g_fib[l].uc_stack.ss_size = STACK; g_fib[l].uc_link = &g_main;
    makecontext(&g_fib[l], fibre_entry, 0);
  }
  for (;;) {
    bool all = true;
    for (int l = 0; l < 64; l++) if (!g_done[l]) { all = false; dmw::g_bench.cur_lane = l; swapcontext(&g_main, &g_fib[l]); }
    if (all) break;
  }
}

size_t stack_high_water() {
  size_t worst = 0;
  for (int l = 0; l < 64 && g_stacks; l++) {
    const unsigned char* p = (const unsigned char*)g_stacks + STACK * l;
    size_t k = 0;
    while (k < STACK && p[k] == STACK_FILL) k++;
    worst = std::max(worst, STACK - k);
  }
  return worst;
}

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

// the batch of tests/term_rollout_host.cpp
struct HostBatch {
  DevModel<double> M;
  Batch<double> B;
  int n = 0;
  std::vector<double> qpos, qvel, qws, time, ctrl, xipos, comz, cfg, vel, aovf, imit, kin;
  std::vector<unsigned char> kin_ok;
  std::vector<int> fidx, finit, ncon, nefc, cong, status, siter, episode, cycle, redo, steps, reason;
  std::vector<int> log_count, log_index; std::vector<double> log_qpos, log_qvel;
  SlotShared<double> slots[SLOTS];
  SlotOrOne<double> roll;
  SlotTables tabs;
  Shared<double> sh;
  StepScratch<double> xs;
};

struct Config { int n, T, nsub, seed, fall, limit, autoreset, reward_mode, F, many_env; double mocap_dt; };

void create(HostBatch& e, const DevModel<double>& M, const Config& c, int action_mode, const std::vector<double>& cfg, const std::vector<double>& vel, const std::vector<double>& table,
            const std::vector<double>& params) {
  const int n = c.n;
  e.M = M; e.n = n;
  e.qpos.assign((size_t)n * NQ, 0); e.qvel.assign((size_t)n * NV, 0); e.qws.assign((size_t)n * NV, 0);
  e.time.assign(n, 0); e.ctrl.assign((size_t)n * NU, 0); e.xipos.assign((size_t)n * NB * 3, 0); e.comz.assign(n, 0);
  e.cfg = cfg; e.vel = vel; e.imit = table;
  e.fidx.assign(n, 0); e.finit.assign(n, 0); e.ncon.assign(n, 0); e.nefc.assign(n, 0); e.cong.assign((size_t)n * MAXEFC * 2, -1);
  e.status.assign(n, 0); e.siter.assign(n, 0); e.episode.assign(n, 0); e.cycle.assign(n, 0); e.aovf.assign((size_t)n * AOVF_COLS * 64, 0);
  e.steps.assign(n, 0); e.reason.assign(n, 0);
  e.log_count.assign(1, 0); e.log_index.assign(4, 0); e.log_qpos.assign(NQ, 0); e.log_qvel.assign(NV, 0);
  Batch<double>& B = e.B;
  B = Batch<double>{};
  B.qpos = e.qpos.data(); B.qvel = e.qvel.data(); B.qws = e.qws.data(); B.time = e.time.data(); B.ctrl = e.ctrl.data();
  B.xipos = e.xipos.data(); B.comz = e.comz.data(); B.frame_idx = e.fidx.data(); B.frame_init = e.finit.data();
  B.ncon = e.ncon.data(); B.nefc = e.nefc.data(); B.cong = e.cong.data(); B.status = e.status.data();
  B.aovf = e.aovf.data(); B.cycle = e.cycle.data(); B.order = nullptr;
  B.solver_iter = e.siter.data(); B.episode = e.episode.data(); B.mocap_cfg = e.cfg.data(); B.mocap_vel = e.vel.data();
  e.kin.assign((size_t)n * KIN_DOUBLES, 0); e.kin_ok.assign(n, 0); B.kin = e.kin.data(); B.kin_ok = e.kin_ok.data();
  e.redo.assign((size_t)n + 16, 0); B.redo_list = e.redo.data() + 16; B.redo_count = e.redo.data(); B.redo_why = e.redo.data() + 8;
  B.mocap_dt = c.mocap_dt; B.n_frames = c.F; B.n_envs = n; B.env_offset = 0; B.reward_mode = c.reward_mode; B.autoreset = c.autoreset; B.action_mode = action_mode;
  B.seed = (unsigned long long)c.seed; B.diag = 0;
  B.imit_table = e.imit.data();
  for (int k = 0; k < 32; k++) B.imit_params[k] = params[k];
  B.imit_pdev = B.imit_params;
}

// dm_batch_set_state on zeroed warm starts and clocks (tests/emu/emu_main.cpp emu_set_state)
void set_state(HostBatch& e, const std::vector<double>& qpos, const std::vector<double>& qvel, const std::vector<int>& fidx) {
  for (int env = 0; env < e.n; env++)
    run_wave([&](int lane) {
      load_env(e.M, e.B, e.sh, env, lane, (const double*)0);
      if (lane < NQ) e.sh.qpos[lane] = qpos[(size_t)env * NQ + lane];
      if (lane < NV) e.sh.qvel[lane] = qvel[(size_t)env * NV + lane];
      if (lane == 0) set_frame(e.B, env, fidx[env]);
      dmw::sync();
      store_state(e.B, e.sh, env, lane);
      { const LaneTopo lt = lane_topo(lane); stage_tables(e.sh, lane); dmw::sync(); forward(e.M, e.sh, lane, lt, (const DebugOut*)0); }
      store_derived(e.B, e.M, e.sh, env, lane);
    });
}

TermArgs term_args(HostBatch& e, const Config& c, int tick) {
  return TermArgs{e.steps.data(), e.reason.data(), (unsigned)c.fall, c.limit, 0, e.n, e.log_count.data(), e.log_index.data(), e.log_qpos.data(), e.log_qvel.data(), 0, tick};
}

struct Rows {
  std::vector<double> obs, rew; std::vector<unsigned char> done;
  Rows(int T, int n) : obs((size_t)T * n * NOBS, 0), rew((size_t)T * n, 0), done((size_t)T * n, 0) {}
};
// what a run held: re-steps in all, re-steps of the many-row environment at step 0, steps a wave took with carried kinematics, auto-resets that a later step follows
struct Tally { long redo = 0, redo_many = 0, carried = 0, resets = 0; };

// (a) the step launches: dmenv.hip step_impl's routing for a packed batch in action modes 3 and 4 (k_step_packed_ext_spd, then k_step_redo_spd), then — `term` —
// the termination launch.  The packed step is the one with the three-set code (DM_OPT_PACKED = 2), as in tests/term_rollout_host.cpp.
void run_steps(HostBatch& e, const Config& c, bool term, const std::vector<double>& act, Rows& r, Tally& tl, std::vector<double>* pre_q, std::vector<double>* pre_done) {
  const int n = e.n;
  for (int t = 0; t < c.T; t++) {
    const double* a = act.data() + (size_t)t * n * NU;
    double* o = r.obs.data() + (size_t)t * n * NOBS; double* rw = r.rew.data() + (size_t)t * n; unsigned char* dn = r.done.data() + (size_t)t * n;
    e.B.redo_count[0] = 0;
    for (int first = 0; first < n; first += SLOTS)
      run_wave([&](int lane) {
        const int slot = lane >> 4, sl = lane & 15;
        stage_slot_tables(e.tabs, lane);
        int pos = first + slot;
        const bool live = pos < n;
        if (!live) pos = n - 1;
        slot_env_step_impl<double, false, false, SLOT_MAXROWS, true>(e.M, e.B, e.slots[slot], e.tabs, pos, sl, lane, live, a, o, rw, dn, c.nsub, e.B.redo_count, e.B.redo_list);
      });
    tl.redo += e.B.redo_count[0];
    for (int i = 0; i < e.B.redo_count[0]; i++) {
      const int env = e.B.redo_list[i];
      if (t == 0 && env == c.many_env) tl.redo_many++;
      run_wave([&](int lane) { env_step_impl<double, 32, false, true>(e.M, e.B, e.sh, e.xs, env, lane, a, o, rw, dn, c.nsub); });
    }
    if (pre_q) {
      std::copy(e.qpos.begin(), e.qpos.end(), pre_q->begin() + (size_t)t * n * NQ);
      for (int i = 0; i < n; i++) (*pre_done)[(size_t)t * n + i] = dn[i];
    }
    if (term) {
      const TermArgs ta = term_args(e, c, t);
      for (int env = 0; env < n; env++) {
        blockIdx.x = (unsigned)env;
        run_wave([&](int) { k_terminate(&e.M, e.B, ta, o, dn); });
      }
    }
    if (t + 1 < c.T) for (int i = 0; i < n; i++) if (dn[i]) tl.resets++;
  }
}

// (b) the horizon launch (kernels_rollout_spd.hip, without a policy).  slot_rollout's policy hook stands where the policy's step would: behind the step, its
// re-steps and the termination phase.  There the wave's next step takes carried kinematics exactly if every slot's flag stands and no in-wave re-step
// overwrote the slots' LDS during this step (slot_rollout `carry`, slot_spd_control): counted from the flags in LDS and the batch's re-step total.
void run_horizon(HostBatch& e, const Config& c, bool term, const std::vector<double>& act, Rows& r, Tally& tl) {
  const int n = e.n;
  std::vector<StepRow> rows((size_t)c.T);
  for (int t = 0; t < c.T; t++) rows[t] = StepRow{act.data() + (size_t)t * n * NU, r.obs.data() + (size_t)t * n * NOBS, r.rew.data() + (size_t)t * n, r.done.data() + (size_t)t * n};
  const int before = e.B.redo_why[0];
  const TermArgs ta = term_args(e, c, 0);
  for (int first = 0; first < n; first += SLOTS) {
    int redo_seen = e.B.redo_why[0];
    auto hook = [&](int t) {
      dmw::sync();
      if (dmw::lane() == 0) {
        bool all = true;
        for (int k = 0; k < SLOTS; k++) all = all && e.roll.sh[k].kin_ok() != 0.0;
        if (all && e.B.redo_why[0] == redo_seen && t + 1 < c.T) tl.carried++;
        if (t == 0 && e.B.redo_why[0] != redo_seen && c.many_env >= first && c.many_env < first + SLOTS) tl.redo_many++;
        redo_seen = e.B.redo_why[0];
      }
      dmw::sync();
    };
    run_wave([&](int lane) {
      const int slot = lane >> 4;
      stage_slot_tables(e.tabs, lane);
      int pos = first + slot;
      const bool live = pos < n;
      if (!live) pos = n - 1;
      if (term) slot_rollout<double, 48, true>(e.M, e.B, e.roll.sh, e.tabs, e.roll.one.s, e.roll.one.x, pos, lane, live, rows.data(), c.nsub, c.T, hook, (long long*)nullptr, false, SlotTermination{ta});
      else slot_rollout<double, 48, true>(e.M, e.B, e.roll.sh, e.tabs, e.roll.one.s, e.roll.one.x, pos, lane, live, rows.data(), c.nsub, c.T, hook);
    });
  }
  tl.redo += e.B.redo_why[0] - before;
  for (int t = 0; t + 1 < c.T; t++) for (int i = 0; i < n; i++) if (r.done[(size_t)t * n + i]) tl.resets++;
}

template <class T> bool same(const char* what, const std::vector<T>& a, const std::vector<T>& b, int per) {
  if (a.size() != b.size()) { std::fprintf(stderr, "spd_rollout_host: %s: sizes differ\n", what); return false; }
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) {
      std::fprintf(stderr, "spd_rollout_host: %s differs at element %zu (row %zu, column %zu): %.17g against %.17g\n", what, i, i / (size_t)per, i % (size_t)per, (double)a[i], (double)b[i]);
      return false;
    }
  return true;
}

bool compare(const char* tag, const HostBatch& a, const HostBatch& b, const Rows& ra, const Rows& rb) {
  const std::string t(tag);
  return same((t + " obs").c_str(), ra.obs, rb.obs, NOBS) && same((t + " reward").c_str(), ra.rew, rb.rew, a.n) && same((t + " done").c_str(), ra.done, rb.done, a.n) &&
         same((t + " qpos").c_str(), a.qpos, b.qpos, NQ) && same((t + " qvel").c_str(), a.qvel, b.qvel, NV) && same((t + " qacc_warmstart").c_str(), a.qws, b.qws, NV) &&
         same((t + " ctrl").c_str(), a.ctrl, b.ctrl, NU) &&
         same((t + " time").c_str(), a.time, b.time, 1) && same((t + " frame_idx").c_str(), a.fidx, b.fidx, 1) && same((t + " frame_init").c_str(), a.finit, b.finit, 1) &&
         same((t + " cycle").c_str(), a.cycle, b.cycle, 1) && same((t + " episode").c_str(), a.episode, b.episode, 1) && same((t + " episode_steps").c_str(), a.steps, b.steps, 1) &&
         same((t + " done_reason").c_str(), a.reason, b.reason, 1) && same((t + " parked-kinematics flags").c_str(), a.kin_ok, b.kin_ok, 1);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: spd_rollout_host IN OUT\n"); return 2; }
  static Input in;
  if (!read_input(argv[1], in)) { std::fprintf(stderr, "spd_rollout_host: cannot read %s\n", argv[1]); return 2; }
  // the model (include/dmenv.h dm_model_desc): sizes, the int tables, the float tables, the scalars — in _abi.make_model_desc's order
  dm_model_desc d{};
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
  const std::vector<double>& sc = in.d();       // timestep, gravity [3], tolerance, solref [2], solimp [5], meaninertia, mocap_dt
  d.timestep = sc.at(0); for (int k = 0; k < 3; k++) d.gravity[k] = sc.at(1 + k);
  d.tolerance = sc.at(4); d.solref[0] = sc.at(5); d.solref[1] = sc.at(6); for (int k = 0; k < 5; k++) d.solimp[k] = sc.at(7 + k);
  d.meaninertia = sc.at(12);
  static DevModel<double> M;
  std::string err;
  if (build_dev_model(&d, &M, &err) != 0) { std::fprintf(stderr, "spd_rollout_host: %s\n", err.c_str()); return 2; }
  M.enable_contact = 1; M.enable_limit = 1;
  const std::vector<double>& cfg = in.d(); const std::vector<double>& vel = in.d(); const std::vector<double>& table = in.d(); const std::vector<double>& params = in.d();
  const std::vector<int>& rc = in.i();          // n, T, nsub, seed, fall mask, limit, autoreset, reward mode, frames, the env that starts in the many-row state
  Config c{rc.at(0), rc.at(1), rc.at(2), rc.at(3), rc.at(4), rc.at(5), rc.at(6), rc.at(7), rc.at(8), rc.at(9), sc.at(13)};
  const std::vector<double>& q0 = in.d(); const std::vector<double>& v0 = in.d(); const std::vector<int>& f0 = in.i();
  const std::vector<double>& act4 = in.d(); const std::vector<double>& act3 = in.d();      // mode 4: offsets from the mocap frame; mode 3: target poses
  const int n = c.n, T = c.T;
  if (n < 1 || T < 1 || cfg.size() != (size_t)c.F * NQ || vel.size() != (size_t)c.F * NV || table.size() != (size_t)c.F * IMIT_FEAT || params.size() != 32 ||
      q0.size() != (size_t)n * NQ || v0.size() != (size_t)n * NV || f0.size() != (size_t)n || act4.size() != (size_t)T * n * NU || act3.size() != act4.size() ||
      c.many_env < 0 || c.many_env >= n) {
    std::fprintf(stderr, "spd_rollout_host: the input's array sizes do not fit n = %d, T = %d, F = %d\n", n, T, c.F); return 2;
  }
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) { std::fprintf(stderr, "spd_rollout_host: cannot write %s\n", argv[2]); return 2; }
  static HostBatch A, H;
  for (int mode = 4; mode >= 3; mode--) {
    const std::vector<double>& act = mode == 4 ? act4 : act3;
    for (int term = 0; term < 2; term++) {
      char tag[64];
      std::snprintf(tag, sizeof tag, "mode %d, %s:", mode, term ? "termination inside" : "no termination");
      std::vector<double> pre_q((size_t)T * n * NQ), pre_done((size_t)T * n);
      Tally ta, th;
      Rows ra(T, n), rh(T, n);
      create(A, M, c, mode, cfg, vel, table, params); set_state(A, q0, v0, f0); run_steps(A, c, term != 0, act, ra, ta, term ? &pre_q : nullptr, term ? &pre_done : nullptr);
      create(H, M, c, mode, cfg, vel, table, params); set_state(H, q0, v0, f0); run_horizon(H, c, term != 0, act, rh, th);
      if (!compare(tag, A, H, ra, rh)) return 1;
      // (the horizon's waves predict which step to call: a miss is re-stepped, so its count may exceed the step launches')
      std::printf("spd_rollout_host: %s %d envs x %d steps x %d substeps agree bit for bit; inside the horizon %ld steps of a wave on carried kinematics, %ld re-steps "
                  "(%ld by the step launches), %ld auto-resets followed by a step\n", tag, n, T, c.nsub, th.carried, th.redo, ta.redo, th.resets);
      if (th.carried < 1 || th.redo_many < 1 || ta.redo_many < 1 || th.resets < 1 || th.resets != ta.resets) {
        std::fprintf(stderr, "spd_rollout_host: %s the horizon must hold a step taken with carried kinematics (%ld), an in-wave re-step of env %d's many-row state (%ld; "
                             "%ld by the step launches) and an auto-reset that a step follows (%ld; %ld by the step launches)\n", tag, th.carried, c.many_env, th.redo_many, ta.redo_many, th.resets, ta.resets);
        return 1;
      }
      if (term) { std::fwrite(pre_q.data(), 8, pre_q.size(), fo); std::fwrite(pre_done.data(), 8, pre_done.size(), fo); }
    }
  }
  std::fclose(fo);
  std::printf("spd_rollout_host: deepest fibre stack %zu of %zu bytes\n", stack_high_water(), STACK);
  if (stack_high_water() > STACK * 3 / 4) { std::fprintf(stderr, "spd_rollout_host: a fibre used more than three quarters of its stack\n"); return 1; }
  free(g_stacks);
  return 0;
}
