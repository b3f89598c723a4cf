// Host twin of the horizon launch with early termination (csrc/slot_term.h, k_rollout_packed_term) for tests/test_horizon_termination.py: the
// unmodified kernel source on the fibre wave testbench (tests/emu/wave_testbench.h), built with -fsanitize=address,undefined.  One batch is stepped
// through a horizon twice from the same states and actions:
//   (a) as the step launches do it: per step the packed step (three-set code) of every wave, the one-env re-step of the environments beyond its capacities, then
//       k_terminate's own body (csrc/term_kernel.h), one environment per wave;
//   (b) as k_rollout_packed_term does it: slot_rollout with slot_term.h's phase inside the loop, one wave after another.
// and every output row, the final state, the counters and the reasons are compared bit for bit; then the same pair once more with the fall set off and
// the truncation log on, whose sorted records are compared the same way.  Test infrastructure only (libdmenv.so has no CPU path).
// The fibre runner is tests/emu/wave_fibres.h, the batch and the launches it emulates tests/emu/host_batch.h, and what this program shares with
// tests/spd_rollout_host.cpp (k_terminate's shims, the input, the termination launch, the comparison) tests/emu/host_rollout.h; here stand the run's
// Config, its tallies, the truncation records and main().
//
// usage: term_rollout_host IN OUT
//   IN   a sequence of arrays, each { int32 kind (0: int32, 1: float64), int64 count, data }, in the order main() reads them
//   OUT  float64: run (a)'s state after every step's step launches, ahead of termination (qpos [T, n, 35]) and that step's own done [T, n], for the
//        test's input condition (no fall decision within rounding of its boundary)
//   exit status 0 and one summary line when everything agrees and the horizon held every kind of ending; else the first difference on stderr and 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_rollout.h"      // the fibre runner, the kernel source, the host batch and its launches (tests/emu/host_batch.h), and the twins' shared layer

namespace {
const char* const PROG = "term_rollout_host";

struct Config { int n, T, nsub, seed, fall, limit, autoreset, reward_mode, F; double mocap_dt; };

void create(HostBatch& e, const DevModel<double>& M, const Config& c, const std::vector<double>& cfg, const std::vector<double>& vel, const std::vector<double>& table,
            const std::vector<double>& params, int log_cap) {
  e.M = M;
  wire(e, c.n, cfg.data(), vel.data(), c.F, c.mocap_dt, log_cap);
  e.B.reward_mode = c.reward_mode; e.B.autoreset = c.autoreset; e.B.action_mode = 0; e.B.seed = (unsigned long long)c.seed; e.B.diag = 0;
  set_imitation(e, table.data(), params.data());
}

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
    tl.redo += packed_step_launch<true>(e, a, o, rw, dn, c.nsub);
    if (pre_q) {
      std::copy(e.qpos.begin(), e.qpos.end(), pre_q->begin() + (size_t)t * n * NQ);
      for (int i = 0; i < n; i++) (*pre_done)[(size_t)t * n + i] = dn[i];
    }
    for (int i = 0; i < n; i++) if (dn[i]) tl.stepdone++;
    terminate_launch(e, term_args(e, fall, c.limit, log_cap, t), o, dn);
    for (int i = 0; i < n; i++) { if (e.reason[i] & DM_DONE_FALL) tl.falls++; if (e.reason[i] & DM_DONE_TIME_LIMIT) tl.limits++; }
  }
}

// (b) the horizon launch with termination inside (kernels_rollout_term.hip k_rollout_packed_term, without a policy)
void run_horizon(HostBatch& e, const Config& c, int fall, int log_cap, const std::vector<double>& act, Rows& r, Tally& tl) {
  tl.redo += horizon_launch<false>(e, act.data(), r.obs.data(), r.rew.data(), r.done.data(), c.nsub, c.T, [](int, int) {}, SlotTermination{term_args(e, fall, c.limit, log_cap, 0)});
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
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: term_rollout_host IN OUT\n"); return 2; }
  static Input in;
  if (!read_input(argv[1], in)) { std::fprintf(stderr, "term_rollout_host: cannot read %s\n", argv[1]); return 2; }
  dm_model_desc d{};
  std::vector<double> sc;
  read_model(in, d, sc);
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
  create(A1, M, c, cfg, vel, table, params, 0); set_state(A1, q0.data(), v0.data(), f0.data(), nullptr); run_steps(A1, c, c.fall, 0, act, ra1, ta1, &pre_q, &pre_done);
  create(B1, M, c, cfg, vel, table, params, 0); set_state(B1, q0.data(), v0.data(), f0.data(), nullptr); run_horizon(B1, c, c.fall, 0, act, rb1, tb1);
  if (!compare(PROG, "fall set + limit:", A1, B1, ra1, rb1)) return 1;
  // second pair: the limit alone, the truncation log on
  const int cap = n * 3;
  Tally ta2, tb2;
  Rows ra2(T, n), rb2(T, n);
  create(A2, M, c, cfg, vel, table, params, cap); set_state(A2, q0.data(), v0.data(), f0.data(), nullptr); run_steps(A2, c, 0, cap, act, ra2, ta2, nullptr, nullptr);
  create(B2, M, c, cfg, vel, table, params, cap); set_state(B2, q0.data(), v0.data(), f0.data(), nullptr); run_horizon(B2, c, 0, cap, act, rb2, tb2);
  if (!compare(PROG, "limit + log:", A2, B2, ra2, rb2)) return 1;
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
