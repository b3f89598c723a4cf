// kernels_rollout_spd.hip — the horizon launch in action modes 3 and 4 (DM_OPT_HORIZON_SPD): k_rollout_packed_spd and
// k_rollout_packed_term_spd, which are k_rollout_packed (kernels_rollout.hip) and k_rollout_packed_term (kernels_rollout_term.hip) with slot_rollout's SPD switch
// on — the packed step bodies and the in-wave one-env re-step with the stable PD controller compiled in (slot_step.h slot_spd_control), which the two kernels
// share inside this unit.  A translation unit of its own, built with the options of kernels_rollout.hip (csrc/build.py ROLLOUT_FLAGS), so that the horizon
// kernels of modes 0..2 and every step kernel stay the code objects they were: a batch without the option never runs a line of this file.
#define DM_NO_LAUNCH_KERNELS
#include "kernels.h"
#include "slot_term.h"
#include "policy_wave_launch_order.h"

using namespace dm;

namespace {
// What the two kernels share: the wave's four environments, then slot_rollout with the controller.  POLICY4: the in-wave policy step (dmp::policy_wave4 or
// dmp::policy_wave4_launch_order, as a callable), TERM: slot_rollout's termination switch.  The LDS is k_rollout_packed's.
template <class POLICY4, class TERM>
DM_DEV void rollout_packed_spd_body(const DevModel<Real>* __restrict__ Mp, const Batch<Real>* __restrict__ Bp, const StepRow* __restrict__ rows, int n_substeps, int first,
                                    int count, int T, const dmp::PolicyArgs& pa, long long* __restrict__ wave_clk, POLICY4&& policy4, TERM&& term) {
  __shared__ SlotOrOne<Real> u;
  __shared__ SlotTables tb;
  static_assert(sizeof(SlotOrOne<Real>) == sizeof(SlotShared<Real>) * SLOTS, "the one-env code's LDS fits into the four slots'");
  static_assert(sizeof(SlotOrOne<Real>) + sizeof(SlotTables) <= 40960, "one wave per SIMD, four per CU");
  const bool policy_clobbers_kin = pa.P != nullptr && sizeof(((SlotShared<Real>*)0)->r1) < 464 * sizeof(float);      // (see k_rollout_packed)
  const Batch<Real>& B = *Bp;
  const int lane = dmw::lane(), slot = lane >> 4;
  stage_slot_tables(tb, lane);
  const bool live = SLOTS * (int)blockIdx.x + slot < count;
  int envs4[SLOTS];
  dispatch_env<SLOTS>(B, first, count, SLOTS * (int)blockIdx.x, lane, blockIdx.x == 0, envs4);
  const int env = slot == 0 ? envs4[0] : slot == 1 ? envs4[1] : slot == 2 ? envs4[2] : envs4[3];
  const int envs[4] = {dmw::bcast_i(env, 0), dmw::bcast_i(env, 16), dmw::bcast_i(env, 32), dmw::bcast_i(env, 48)};
  const int lv = live ? 1 : 0;
  const bool wr[4] = {dmw::bcast_i(lv, 0) != 0, dmw::bcast_i(lv, 16) != 0, dmw::bcast_i(lv, 32) != 0, dmw::bcast_i(lv, 48) != 0};
  const size_t n = (size_t)B.n_envs;
  const long long t_enter = wave_clk ? dmw::clk() : 0;
  slot_rollout<Real, RESTEP_ROWS, true>(*Mp, B, u.sh, tb, u.one.s, u.one.x, env, lane, live, rows, n_substeps, T, [&](int t) {
    if (!pa.P) return;
    dmp::PolicyArgs p = pa;
    p.action = pa.action + (size_t)(t + 1) * n * NU; p.vpred = pa.vpred + (size_t)t * n; p.counter = pa.counter + (unsigned long long)t;
    dmw::sync();
    policy4(p, envs, wr, lane, reinterpret_cast<char*>(&u.sh[0]), (unsigned)sizeof(SlotShared<Real>), (unsigned)(offsetof(SlotShared<Real>, qpos) + 7 * sizeof(Real)),
            (unsigned)(offsetof(SlotShared<Real>, qvel) + 6 * sizeof(Real)), (unsigned)offsetof(SlotShared<Real>, r1));
  }, (long long*)nullptr, policy_clobbers_kin, term);
  if (wave_clk && lane == 0) wave_clk[(size_t)blockIdx.x * dm::PROF_SLOTS + 5] = dmw::clk() - t_enter;       // (DM option 101: this wave's cycles)
}
}  // namespace

// k_rollout_packed in action modes 3 and 4.  The policy's step is policy_wave4, as there: the step launches of these modes fuse the policy the same way
// (k_step_packed_act_spd), and this kernel's actions and values are theirs bit for bit.
__global__ __launch_bounds__(64) void k_rollout_packed_spd(const DevModel<Real>* __restrict__ Mp, const Batch<Real>* __restrict__ Bp, const StepRow* __restrict__ rows,
                                                           int n_substeps, int first, int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk) {
  rollout_packed_spd_body(Mp, Bp, rows, n_substeps, first, count, T, pa, wave_clk,
                          [](auto&&... a) { dmp::policy_wave4<Real>(a...); }, NoTermination{});
}

// k_rollout_packed_term in action modes 3 and 4: the same termination phase on the same tick rule (`ta`: see there), the policy's step in the order of the
// policy LAUNCH (policy_wave_launch_order.h), which is how the step launches of a batch with termination on run it.
__global__ __launch_bounds__(64) void k_rollout_packed_term_spd(const DevModel<Real>* __restrict__ Mp, const Batch<Real>* __restrict__ Bp, const StepRow* __restrict__ rows,
                                                                int n_substeps, int first, int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk, TermArgs ta) {
  rollout_packed_spd_body(Mp, Bp, rows, n_substeps, first, count, T, pa, wave_clk,
                          [](auto&&... a) { dmp::policy_wave4_launch_order<Real>(a...); }, SlotTermination{ta});
}
