// Host twin of the horizon launch with early termination (csrc/slot_term.h, k_rollout_packed_term) for tests/test_horizon_termination.py: the
// unmodified kernel source on the fibre wave testbench (tests/emu/wave_testbench.h), built with -fsanitize=address,undefined.  One batch is stepped
// through a horizon twice from the same states and actions:
//   (a) as the step launches do it: per step the packed step (three-set code) of every wave, the one-env re-step of the environments beyond its capacities, then
//       k_terminate's own body (csrc/term_kernel.h), one environment per wave;
//   (b) as k_rollout_packed_term does it: slot_rollout with slot_term.h's phase inside the loop, one wave after another.
// and every output row, the final state, the counters and the reasons are compared bit for bit; then the same pair once more with the fall set off and
// the truncation log on, whose sorted records are compared the same way.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: term_rollout_host IN OUT
//   IN   a sequence of arrays, each { int32 kind (0: int32, 1: float64), int64 count, data }, in the order main() reads them
//   OUT  float64: run (a)'s state after every step's step launches, ahead of termination (qpos [T, n, 35]) and that step's own done [T, n], for the
//        test's input condition (no fall decision within rounding of its boundary)
//   exit status 0 and one summary line when everything agrees and the horizon held every kind of ending; else the first difference on stderr and 1
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
// k_terminate hands a value from lane 0 to the wave with dmw::uniform: a readfirstlane on the device, the identity on the testbench (where every lane of the
// kernels written so far held the value already).  For the termination launch's kernel alone it is lane 0's value, as on the device.
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
// (a fibre's stack: the sanitizer's swapcontext clears the shadow of the whole stack at every switch, so it is kept small — and its high-water mark is
//  checked at the end, since one fibre's overflow would land in its neighbour's stack, where the sanitizer does not look)
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

// bytes of the deepest fibre stack ever used (stacks grow downwards: the first byte from the bottom that lost the fill pattern)
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

// the batch of tests/emu/emu_main.cpp, with the termination launch's arrays
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

struct Config { int n, T, nsub, seed, fall, limit, autoreset, reward_mode, F; double mocap_dt; };

void create(HostBatch& e, const DevModel<double>& M, const Config& c, const std::vector<double>& cfg, const std::vector<double>& vel, const std::vector<double>& table,
            const std::vector<double>& params, int log_cap) {
  const int n = c.n;
  e.M = M; e.n = n;
  e.qpos.assign((size_t)n * NQ, 0); e.qvel.assign((size_t)n * NV, 0); e.qws.assign((size_t)n * NV, 0);
  e.time.assign(n, 0); e.ctrl.assign((size_t)n * NU, 0); e.xipos.assign((size_t)n * NB * 3, 0); e.comz.assign(n, 0);
  e.cfg = cfg; e.vel = vel; e.imit = table;
  e.fidx.assign(n, 0); e.finit.assign(n, 0); e.ncon.assign(n, 0); e.nefc.assign(n, 0); e.cong.assign((size_t)n * MAXEFC * 2, -1);
  e.status.assign(n, 0); e.siter.assign(n, 0); e.episode.assign(n, 0); e.cycle.assign(n, 0); e.aovf.assign((size_t)n * AOVF_COLS * 64, 0);
  e.steps.assign(n, 0); e.reason.assign(n, 0);
  e.log_count.assign(1, 0); e.log_index.assign((size_t)std::max(log_cap, 1) * 4, 0); e.log_qpos.assign((size_t)std::max(log_cap, 1) * NQ, 0); e.log_qvel.assign((size_t)std::max(log_cap, 1) * NV, 0);
  Batch<double>& B = e.B;
  B = Batch<double>{};
  B.qpos = e.qpos.data(); B.qvel = e.qvel.data(); B.qws = e.qws.data(); B.time = e.time.data(); B.ctrl = e.ctrl.data();
  B.xipos = e.xipos.data(); B.comz = e.comz.data(); B.frame_idx = e.fidx.data(); B.frame_init = e.finit.data();
  B.ncon = e.ncon.data(); B.nefc = e.nefc.data(); B.cong = e.cong.data(); B.status = e.status.data();
  B.aovf = e.aovf.data(); B.cycle = e.cycle.data(); B.order = nullptr;
  B.solver_iter = e.siter.data(); B.episode = e.episode.data(); B.mocap_cfg = e.cfg.data(); B.mocap_vel = e.vel.data();
  e.kin.assign((size_t)n * KIN_DOUBLES, 0); e.kin_ok.assign(n, 0); B.kin = e.kin.data(); B.kin_ok = e.kin_ok.data();
  e.redo.assign((size_t)n + 16, 0); B.redo_list = e.redo.data() + 16; B.redo_count = e.redo.data(); B.redo_why = e.redo.data() + 8;
  B.mocap_dt = c.mocap_dt; B.n_frames = c.F; B.n_envs = n; B.env_offset = 0; B.reward_mode = c.reward_mode; B.autoreset = c.autoreset; B.action_mode = 0;
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

TermArgs term_args(HostBatch& e, const Config& c, int fall, int log_cap, int tick) {
  return TermArgs{e.steps.data(), e.reason.data(), (unsigned)fall, c.limit, 0, e.n, e.log_count.data(), e.log_index.data(), e.log_qpos.data(), e.log_qvel.data(), log_cap, tick};
}

struct Rows {
  std::vector<double> obs, rew; std::vector<unsigned char> done;
  Rows(int T, int n) : obs((size_t)T * n * NOBS, 0), rew((size_t)T * n, 0), done((size_t)T * n, 0) {}
};
struct Tally { long falls = 0, limits = 0, stepdone = 0, redo = 0; };

// (a) the step launches: dmenv.hip step_impl's routing for a packed batch, then the termination launch.  The packed step is the one with the three-set code
// (DM_OPT_PACKED = 2, k_step_packed_ext): a horizon's waves call that instantiation for an environment near the two-set capacity (slot_rollout `heavy`), so
// an environment at 33 .. 40 rows stays on the packed path in both forms.  The lean step hands it to the one-env code, whose sums differ from the packed
// path's in the last bits — with or without termination, which this program is not about.
void run_steps(HostBatch& e, const Config& c, int fall, int log_cap, const std::vector<double>& act, Rows& r, Tally& tl, std::vector<double>* pre_q, std::vector<double>* pre_done) {
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
        slot_env_step<double, false, false, SLOT_MAXROWS>(e.M, e.B, e.slots[slot], e.tabs, pos, sl, lane, live, a, o, rw, dn, c.nsub, e.B.redo_count, e.B.redo_list);
      });
    tl.redo += e.B.redo_count[0];
    for (int i = 0; i < e.B.redo_count[0]; i++) {
      const int env = e.B.redo_list[i];
      run_wave([&](int lane) { env_step<double, 32>(e.M, e.B, e.sh, e.xs, env, lane, a, o, rw, dn, c.nsub); });
    }
    if (pre_q) {
      std::copy(e.qpos.begin(), e.qpos.end(), pre_q->begin() + (size_t)t * n * NQ);
      for (int i = 0; i < n; i++) (*pre_done)[(size_t)t * n + i] = dn[i];
    }
    for (int i = 0; i < n; i++) if (dn[i]) tl.stepdone++;
    const TermArgs ta = term_args(e, c, fall, log_cap, t);
    for (int env = 0; env < n; env++) {
      blockIdx.x = (unsigned)env;
      run_wave([&](int) { k_terminate(&e.M, e.B, ta, o, dn); });
    }
    for (int i = 0; i < n; i++) { if (e.reason[i] & DM_DONE_FALL) tl.falls++; if (e.reason[i] & DM_DONE_TIME_LIMIT) tl.limits++; }
  }
}

// (b) the horizon launch with termination inside (kernels_rollout_term.hip k_rollout_packed_term, without a policy)
void run_horizon(HostBatch& e, const Config& c, int fall, int log_cap, const std::vector<double>& act, Rows& r, Tally& tl) {
  const int n = e.n;
  std::vector<StepRow> rows((size_t)c.T);
  for (int t = 0; t < c.T; t++) rows[t] = StepRow{act.data() + (size_t)t * n * NU, r.obs.data() + (size_t)t * n * NOBS, r.rew.data() + (size_t)t * n, r.done.data() + (size_t)t * n};
  const int before = e.B.redo_why[0];
  const TermArgs ta = term_args(e, c, fall, log_cap, 0);
  for (int first = 0; first < n; first += SLOTS)
    run_wave([&](int lane) {
      const int slot = lane >> 4;
      stage_slot_tables(e.tabs, lane);
      int pos = first + slot;
      const bool live = pos < n;
      if (!live) pos = n - 1;
      slot_rollout<double, 48>(e.M, e.B, e.roll.sh, e.tabs, e.roll.one.s, e.roll.one.x, pos, lane, live, rows.data(), c.nsub, c.T, [](int) {}, (long long*)nullptr, false, SlotTermination{ta});
    });
  tl.redo += e.B.redo_why[0] - before;
}

template <class T> bool same(const char* what, const std::vector<T>& a, const std::vector<T>& b, int per) {
  if (a.size() != b.size()) { std::fprintf(stderr, "term_rollout_host: %s: sizes differ\n", what); return false; }
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) {
      std::fprintf(stderr, "term_rollout_host: %s differs at element %zu (row %zu, column %zu): %.17g against %.17g\n", what, i, i / (size_t)per, i % (size_t)per, (double)a[i], (double)b[i]);
      return false;
    }
  return true;
}

// the log's records keyed on (tick, env): {env, tick, frame_idx, frame_init, qpos bits ..., qvel bits ...}
std::vector<std::vector<long long>> records(const HostBatch& e, int log_cap) {
  std::vector<std::vector<long long>> out;
  const int cnt = std::min(e.log_count[0], log_cap);
  for (int k = 0; k < cnt; k++) {
    std::vector<long long> r;
    r.push_back(e.log_index[(size_t)k * 4 + 1]); r.push_back(e.log_index[(size_t)k * 4]); r.push_back(e.log_index[(size_t)k * 4 + 2]); r.push_back(e.log_index[(size_t)k * 4 + 3]);
    for (int i = 0; i < NQ; i++) { long long b; std::memcpy(&b, &e.log_qpos[(size_t)k * NQ + i], 8); r.push_back(b); }
    for (int i = 0; i < NV; i++) { long long b; std::memcpy(&b, &e.log_qvel[(size_t)k * NV + i], 8); r.push_back(b); }
    out.push_back(r);
  }
  std::sort(out.begin(), out.end());
  return out;
}

bool compare(const char* tag, const HostBatch& a, const HostBatch& b, const Rows& ra, const Rows& rb) {
  const std::string t(tag);
  return same((t + " obs").c_str(), ra.obs, rb.obs, NOBS) && same((t + " reward").c_str(), ra.rew, rb.rew, a.n) && same((t + " done").c_str(), ra.done, rb.done, a.n) &&
         same((t + " qpos").c_str(), a.qpos, b.qpos, NQ) && same((t + " qvel").c_str(), a.qvel, b.qvel, NV) && same((t + " qacc_warmstart").c_str(), a.qws, b.qws, NV) &&
         same((t + " time").c_str(), a.time, b.time, 1) && same((t + " frame_idx").c_str(), a.fidx, b.fidx, 1) && same((t + " frame_init").c_str(), a.finit, b.finit, 1) &&
         same((t + " cycle").c_str(), a.cycle, b.cycle, 1) && same((t + " episode").c_str(), a.episode, b.episode, 1) && same((t + " episode_steps").c_str(), a.steps, b.steps, 1) &&
         same((t + " done_reason").c_str(), a.reason, b.reason, 1) && same((t + " parked-kinematics flags").c_str(), a.kin_ok, b.kin_ok, 1);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: term_rollout_host IN OUT\n"); return 2; }
  static Input in;
  if (!read_input(argv[1], in)) { std::fprintf(stderr, "term_rollout_host: cannot read %s\n", argv[1]); return 2; }
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
  if (build_dev_model(&d, &M, &err) != 0) { std::fprintf(stderr, "term_rollout_host: %s\n", err.c_str()); return 2; }
  M.enable_contact = 1; M.enable_limit = 1;
  const std::vector<double>& cfg = in.d(); const std::vector<double>& vel = in.d(); const std::vector<double>& table = in.d(); const std::vector<double>& params = in.d();
  const std::vector<int>& rc = in.i();          // n, T, nsub, seed, fall mask, limit, autoreset, reward mode, frames
  Config c{rc.at(0), rc.at(1), rc.at(2), rc.at(3), rc.at(4), rc.at(5), rc.at(6), rc.at(7), rc.at(8), sc.at(13)};
  const std::vector<double>& q0 = in.d(); const std::vector<double>& v0 = in.d(); const std::vector<int>& f0 = in.i(); const std::vector<double>& act = in.d();
  const int n = c.n, T = c.T;
  if (n < 1 || T < 1 || cfg.size() != (size_t)c.F * NQ || vel.size() != (size_t)c.F * NV || table.size() != (size_t)c.F * IMIT_FEAT || params.size() != 32 ||
      q0.size() != (size_t)n * NQ || v0.size() != (size_t)n * NV || f0.size() != (size_t)n || act.size() != (size_t)T * n * NU) {
    std::fprintf(stderr, "term_rollout_host: the input's array sizes do not fit n = %d, T = %d, F = %d\n", n, T, c.F); return 2;
  }
  std::vector<double> pre_q((size_t)T * n * NQ), pre_done((size_t)T * n);
  static HostBatch A1, B1, A2, B2;
  // first pair: the fall set and the limit, no log
  Tally ta1, tb1;
  Rows ra1(T, n), rb1(T, n);
  create(A1, M, c, cfg, vel, table, params, 0); set_state(A1, q0, v0, f0); run_steps(A1, c, c.fall, 0, act, ra1, ta1, &pre_q, &pre_done);
  create(B1, M, c, cfg, vel, table, params, 0); set_state(B1, q0, v0, f0); run_horizon(B1, c, c.fall, 0, act, rb1, tb1);
  if (!compare("fall set + limit:", A1, B1, ra1, rb1)) return 1;
  // second pair: the limit alone, the truncation log on
  const int cap = n * 3;
  Tally ta2, tb2;
  Rows ra2(T, n), rb2(T, n);
  create(A2, M, c, cfg, vel, table, params, cap); set_state(A2, q0, v0, f0); run_steps(A2, c, 0, cap, act, ra2, ta2, nullptr, nullptr);
  create(B2, M, c, cfg, vel, table, params, cap); set_state(B2, q0, v0, f0); run_horizon(B2, c, 0, cap, act, rb2, tb2);
  if (!compare("limit + log:", A2, B2, ra2, rb2)) return 1;
  if (A2.log_count[0] != B2.log_count[0]) { std::fprintf(stderr, "term_rollout_host: %d records by the step launches, %d inside the horizon\n", A2.log_count[0], B2.log_count[0]); return 1; }
  if (A2.log_count[0] > cap) { std::fprintf(stderr, "term_rollout_host: the log overflowed (%d records, capacity %d)\n", A2.log_count[0], cap); return 1; }
  const auto la = records(A2, cap), lb = records(B2, cap);
  for (size_t k = 0; k < la.size() && k < lb.size(); k++)
    for (size_t i = 0; i < la[k].size(); i++)
      if (la[k][i] != lb[k][i]) {
        std::fprintf(stderr, "term_rollout_host: sorted truncation record %zu differs in word %zu: (tick %lld, env %lld) %lld against (tick %lld, env %lld) %lld\n", k, i,
                     la[k][0], la[k][1], la[k][i], lb[k][0], lb[k][1], lb[k][i]);
        return 1;
      }
  if (la.size() != lb.size()) { std::fprintf(stderr, "term_rollout_host: %zu against %zu truncation records\n", la.size(), lb.size()); return 1; }
  if (ta2.limits != A2.log_count[0]) { std::fprintf(stderr, "term_rollout_host: %ld time-limit ends, %d records\n", ta2.limits, A2.log_count[0]); return 1; }
  // (the horizon's waves predict which step to call: a miss is re-stepped, so its count may exceed the step launches')
  std::printf("term_rollout_host: %d envs x %d steps agree bit for bit; %ld falls, %ld time-limit ends, %ld ended by the step, %ld re-steps inside the horizon (%ld by the step launches); "
              "%d truncation records; deepest fibre stack %zu of %zu bytes\n", n, T, ta1.falls, ta1.limits, ta1.stepdone, tb1.redo, ta1.redo, A2.log_count[0], stack_high_water(), STACK);
  if (stack_high_water() > STACK * 3 / 4) { std::fprintf(stderr, "term_rollout_host: a fibre used more than three quarters of its stack\n"); return 1; }
  if (ta1.falls < 1 || ta1.limits < 1 || ta1.stepdone < 1 || tb1.redo < 1 || A2.log_count[0] < 1) {
    std::fprintf(stderr, "term_rollout_host: the horizon must hold a fall, a time-limit end, a step-own done, a re-step and a truncation record\n"); return 1;
  }
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) { std::fprintf(stderr, "term_rollout_host: cannot write %s\n", argv[2]); return 2; }
  std::fwrite(pre_q.data(), 8, pre_q.size(), fo); std::fwrite(pre_done.data(), 8, pre_done.size(), fo);
  std::fclose(fo);
  free(g_stacks);
  return 0;
}
