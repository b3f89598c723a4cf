// Host twin of the horizon launch in action modes 3 and 4 (DM_OPT_HORIZON_SPD: csrc/kernels_rollout_spd.hip, slot_step.h's SPD switch) for
// tests/test_horizon_spd.py: the unmodified kernel source on the fibre wave testbench (tests/emu/wave_testbench.h), built with -fsanitize=address,undefined.
// One batch is stepped through a horizon twice from the same states and actions:
//   (a) as the step launches do it: per step the packed step (three-set code, the controller compiled in, no carried kinematics) of every wave, the one-env
//       re-step with the controller of the environments beyond its capacities, then — the termination runs — k_terminate's own body, one environment per wave;
//   (b) as k_rollout_packed_spd / k_rollout_packed_term_spd do it: slot_rollout with the SPD switch on, one wave after another, without / with slot_term.h's phase.
// and every output row, the final state (DM_F_CTRL included), the counters and the reasons are compared bit for bit: action mode 4, then mode 3, each
// without and with the termination phase.  Test infrastructure only (libdmenv.so has no CPU path).
// The fibre runner is tests/emu/wave_fibres.h, the batch and the launches it emulates tests/emu/host_batch.h, and what this program shares with
// tests/term_rollout_host.cpp (k_terminate's shims, the input, the termination launch, the comparison) tests/emu/host_rollout.h; here stand the run's
// Config, its tallies and main().
//
// usage: spd_rollout_host IN OUT
//   IN   a sequence of arrays, each { int32 kind (0: int32, 1: float64), int64 count, data }, in the order main() reads them
//   OUT  float64, for mode 4 then mode 3: the termination run (a)'s state after every step's step launches, ahead of termination (qpos [T, n, 35]) and that
//        step's own done [T, n], for the test's input condition (no fall decision within rounding of its boundary)
//   exit status 0 and a summary line per run when everything agrees and every horizon held a step taken with carried kinematics, an in-wave re-step of the
//   environment that starts in the many-row state, and an auto-reset that a later step follows; else the first difference on stderr and 1
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_rollout.h"      // the fibre runner, the kernel source, the host batch and its launches (tests/emu/host_batch.h), and the twins' shared layer

namespace {
const char* const PROG = "spd_rollout_host";

struct Config { int n, T, nsub, seed, fall, limit, autoreset, reward_mode, F, many_env; double mocap_dt; };

void create(HostBatch& e, const DevModel<double>& M, const Config& c, int action_mode, const std::vector<double>& cfg, const std::vector<double>& vel, const std::vector<double>& table,
            const std::vector<double>& params) {
  e.M = M;
  wire(e, c.n, cfg.data(), vel.data(), c.F, c.mocap_dt);
  e.B.reward_mode = c.reward_mode; e.B.autoreset = c.autoreset; e.B.action_mode = action_mode; e.B.seed = (unsigned long long)c.seed; e.B.diag = 0;
  set_imitation(e, table.data(), params.data());
}

// what a run held: re-steps in all, re-steps of the many-row environment at step 0, steps a wave took with carried kinematics, auto-resets that a later step follows
struct Tally { long redo = 0, redo_many = 0, carried = 0, resets = 0; };

// (a) the step launches: dmenv.hip step_impl's routing for a packed batch in action modes 3 and 4 (k_step_packed_ext_spd, then k_step_redo_spd), then — `term` —
// the termination launch.  The packed step is the one with the three-set code (DM_OPT_PACKED = 2), as in tests/term_rollout_host.cpp.
void run_steps(HostBatch& e, const Config& c, bool term, const std::vector<double>& act, Rows& r, Tally& tl, std::vector<double>* pre_q, std::vector<double>* pre_done) {
  const int n = e.n;
  for (int t = 0; t < c.T; t++) {
    const double* a = act.data() + (size_t)t * n * NU;
    double* o = r.obs.data() + (size_t)t * n * NOBS; double* rw = r.rew.data() + (size_t)t * n; unsigned char* dn = r.done.data() + (size_t)t * n;
    const int redo = packed_step_launch<true, true>(e, a, o, rw, dn, c.nsub);
    tl.redo += redo;
    for (int i = 0; i < redo; i++) if (t == 0 && e.B.redo_list[i] == c.many_env) tl.redo_many++;
    if (pre_q) {
      std::copy(e.qpos.begin(), e.qpos.end(), pre_q->begin() + (size_t)t * n * NQ);
      for (int i = 0; i < n; i++) (*pre_done)[(size_t)t * n + i] = dn[i];
    }
    if (term) terminate_launch(e, term_args(e, c.fall, c.limit, 0, t), o, dn);
    if (t + 1 < c.T) for (int i = 0; i < n; i++) if (dn[i]) tl.resets++;
  }
}

// (b) the horizon launch (kernels_rollout_spd.hip, without a policy).  slot_rollout's policy hook stands where the policy's step would: behind the step, its
// re-steps and the termination phase.  There the wave's next step takes carried kinematics exactly if every slot's flag stands and no in-wave re-step
// overwrote the slots' LDS during this step (slot_rollout `carry`, slot_spd_control): counted from the flags in LDS and the batch's re-step total.
void run_horizon(HostBatch& e, const Config& c, bool term, const std::vector<double>& act, Rows& r, Tally& tl) {
  int redo_seen = e.B.redo_why[0];          // the total behind the previous step of this wave, or behind the previous wave: the hook follows every step, the last one too
  auto hook = [&](int first, int t) {
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
  double* o = r.obs.data(); double* rw = r.rew.data(); unsigned char* dn = r.done.data();
  tl.redo += term ? horizon_launch<true>(e, act.data(), o, rw, dn, c.nsub, c.T, hook, SlotTermination{term_args(e, c.fall, c.limit, 0, 0)})
                  : horizon_launch<true>(e, act.data(), o, rw, dn, c.nsub, c.T, hook);
  for (int t = 0; t + 1 < c.T; t++) for (int i = 0; i < e.n; i++) if (r.done[(size_t)t * e.n + i]) tl.resets++;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: spd_rollout_host IN OUT\n"); return 2; }
  static Input in;
  if (!read_input(argv[1], in)) { std::fprintf(stderr, "spd_rollout_host: cannot read %s\n", argv[1]); return 2; }
  dm_model_desc d{};
  std::vector<double> sc;
  read_model(in, d, sc);
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
      create(A, M, c, mode, cfg, vel, table, params); set_state(A, q0.data(), v0.data(), f0.data(), nullptr); run_steps(A, c, term != 0, act, ra, ta, term ? &pre_q : nullptr, term ? &pre_done : nullptr);
      create(H, M, c, mode, cfg, vel, table, params); set_state(H, q0.data(), v0.data(), f0.data(), nullptr); run_horizon(H, c, term != 0, act, rh, th);
      if (!compare(PROG, tag, A, H, ra, rh)) return 1;
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
