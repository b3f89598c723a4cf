// learner.hip — the learner half of the C ABI of include/dmenv.h: the policy's launch kernels, GAE and the episode scan (policy_kernel.h), the value fit and
// the observation filter (vf_kernel.h), the policy half of TRPO, behaviour cloning and PPO (pg_kernel.h), the GAIL discriminator (disc_kernel.h).  No entry
// point here takes a batch: they work on the caller's device arrays and stream.  Default backend options (csrc/build.py).
#include <cmath>

#include "host_common.h"
#include "policy_kernel.h"
#include "vf_kernel.h"
#include "pg_kernel.h"
#include "disc_kernel.h"

extern "C" int dm_policy_weight_count(void) { return dmp::N_WEIGHTS; }
extern "C" int dm_policy_act(const float* weights, const double* obs, double* action, float* vpred, int32_t n, int32_t stochastic,
                             uint64_t seed, uint64_t counter, void* hip_stream) {
  if (!weights || !obs || !action || !vpred || n <= 0) return fail(DM_EINVAL, "dm_policy_act: bad argument");
  hipLaunchKernelGGL(dmp::k_policy_act, dim3((n + dmp::EB - 1) / dmp::EB), dim3(256), 0, (hipStream_t)hip_stream, weights, obs, action, vpred,
                     (int)n, (int)stochastic, (unsigned long long)seed, (unsigned long long)counter);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_gae(const float* rew, const float* vpred, const int32_t* isnew, const float* nextvpred, float* adv, float* tdlamret,
                      int32_t T, int32_t n, double gamma, double lam, void* hip_stream) {
  if (!rew || !vpred || !isnew || !nextvpred || !adv || !tdlamret || T <= 0 || n <= 0) return fail(DM_EINVAL, "dm_gae: bad argument");
  hipLaunchKernelGGL(dmp::k_gae, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, rew, vpred, (const int*)isnew, nextvpred, adv,
                     tdlamret, (int)T, (int)n, (float)gamma, (float)lam);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_gae_boot(const float* rew, const float* vpred, const int32_t* isnew, const float* nextvpred, const float* vboot, float* adv,
                           float* tdlamret, int32_t T, int32_t n, double gamma, double lam, void* hip_stream) {
  if (!rew || !vpred || !isnew || !nextvpred || !vboot || !adv || !tdlamret || T <= 0 || n <= 0) return fail(DM_EINVAL, "dm_gae_boot: bad argument");
  hipLaunchKernelGGL(dmp::k_gae_boot, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, rew, vpred, (const int*)isnew, nextvpred, vboot, adv,
                     tdlamret, (int)T, (int)n, (float)gamma, (float)lam);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_episode_scan(const double* reward, const uint8_t* done, int32_t T, int32_t n, double* cur_ret, int64_t* cur_len, int32_t* count,
                               int32_t cap, int64_t* records, void* hip_stream) {
  if (!reward || !done || !cur_ret || !cur_len || !count || !records || T <= 0 || n <= 0 || cap < 0) return fail(DM_EINVAL, "dm_episode_scan: bad argument");
  if (set_device_of(reward)) return fail(DM_EHIP, "dm_episode_scan: hipSetDevice failed");      // (the launches go to the device that owns the arrays, whatever the thread's current one)
  hipStream_t st = (hipStream_t)hip_stream;
  HIPCHK(hipMemsetAsync(count, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(dmp::k_episodes, dim3((n + 255) / 256), dim3(256), 0, st, reward, done, (int)T, (int)n, cur_ret, (long long*)cur_len, (int*)count, (int)cap,
                     (long long*)records);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_vf_param_count(void) { return dmv::NP; }
struct VfScratch { size_t partial, rpart, part_all, means, stds, total; };
static VfScratch vf_scratch_layout(int nb, int bs) {
  const size_t ntile = (size_t)((bs + dmv::SB - 1) / dmv::SB);
  VfScratch L;
  size_t o = 0;
  L.partial = o; o += up256(ntile * dmv::NPAD * sizeof(float));
  L.rpart = o; o += up256((size_t)dmv::RMS_BLOCKS * 2 * dmv::OB * sizeof(double) + 64);          // + the ticket of the three-launch form
  L.part_all = o; o += up256((size_t)nb * dmv::RMS_BLOCKS * 2 * dmv::OB * sizeof(double));
  L.means = o; o += up256((size_t)nb * dmv::OB * sizeof(float));
  L.stds = o; o += up256((size_t)nb * dmv::OB * sizeof(float));
  L.total = o;
  return L;
}
extern "C" size_t dm_vf_scratch_bytes(int32_t nb, int32_t bs) { return vf_scratch_layout(nb < 1 ? 1 : nb, bs < 1 ? 1 : bs).total; }
extern "C" int dm_vf_fit_epoch(const float* ob, const float* ret, int32_t nb, int32_t bs, float* theta, float* adam_m, float* adam_v,
                               const float* step_scale_host, double beta1, double beta2, double eps, double* rms_sum, double* rms_sumsq,
                               double* rms_count, float* rms_mean, float* rms_std, void* scratch, void* hip_stream, int32_t epoch_filter) {
  if (!ob || !ret || !theta || !adam_m || !adam_v || !step_scale_host || !rms_sum || !rms_sumsq || !rms_count || !rms_mean || !rms_std || !scratch ||
      nb < 1 || bs < 1 || !aligned16(theta))                    // (the kernels stage theta with float4 loads)
    return fail(DM_EINVAL, "dm_vf_fit_epoch: bad argument");
  hipStream_t st = (hipStream_t)hip_stream;
  { // launch on the device that owns the parameters (the caller's stream belongs to it), whatever the thread's current device is
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, theta) == hipSuccess) HIPCHK(hipSetDevice(at.device));
    else (void)hipGetLastError();
  }
  const VfScratch L = vf_scratch_layout(nb, bs);
  const int nblk = (bs + dmv::SB - 1) / dmv::SB;
  char* base = (char*)scratch;
  float* partial = (float*)(base + L.partial);
  if (epoch_filter) {
    // the obs filter's sums of every minibatch up front and their scan (csrc/vf_kernel.h); per minibatch: gradient partials, reduction + Adam
    double* part_all = (double*)(base + L.part_all);
    float* means = (float*)(base + L.means); float* stds = (float*)(base + L.stds);
    hipLaunchKernelGGL(dmv::k_vf_rms_part, dim3(dmv::RMS_BLOCKS, nb), dim3(256), 0, st, ob, (int)bs, part_all);
    hipLaunchKernelGGL(dmv::k_vf_rms_fold, dim3(nb), dim3(128), 0, st, part_all);
    hipLaunchKernelGGL(dmv::k_vf_rms_scan, dim3(1), dim3(64), 0, st, (const double*)part_all, (int)nb, (int)bs, rms_sum, rms_sumsq, rms_count, rms_mean, rms_std, means, stds);
    for (int i = 0; i < nb; i++) {
      hipLaunchKernelGGL(dmv::k_vf_grad, dim3(nblk), dim3(256), 0, st, ob + (size_t)i * bs * dmv::OB, ret + (size_t)i * bs, (int)bs, (const float*)theta,
                         (const float*)(means + (size_t)i * dmv::OB), (const float*)(stds + (size_t)i * dmv::OB), partial);
      hipLaunchKernelGGL(dmv::k_vf_adam, dim3((dmv::NP + dmv::ADAM_PARAMS - 1) / dmv::ADAM_PARAMS), dim3(256), 0, st, (const float*)partial, nblk, theta, adam_m, adam_v,
                         step_scale_host[i], (float)beta1, (float)beta2, (float)eps);
    }
    HIPCHK(hipGetLastError());
    return DM_OK;
  }
  double* rpart = (double*)(base + L.rpart);
  unsigned* ticket = (unsigned*)(rpart + dmv::RMS_BLOCKS * 2 * dmv::OB);
  HIPCHK(hipMemsetAsync(ticket, 0, sizeof(unsigned), st));
  for (int i = 0; i < nb; i++) {
    const float* mbob = ob + (size_t)i * bs * dmv::OB;
    const float* mbret = ret + (size_t)i * bs;
    hipLaunchKernelGGL(dmv::k_vf_rms, dim3(dmv::RMS_BLOCKS), dim3(256), 0, st, mbob, (int)bs, rpart, ticket, rms_sum, rms_sumsq, rms_count, rms_mean, rms_std);
    hipLaunchKernelGGL(dmv::k_vf_grad, dim3(nblk), dim3(256), 0, st, mbob, mbret, (int)bs, (const float*)theta, (const float*)rms_mean,
                       (const float*)rms_std, partial);
    hipLaunchKernelGGL(dmv::k_vf_adam, dim3((dmv::NP + dmv::ADAM_PARAMS - 1) / dmv::ADAM_PARAMS), dim3(256), 0, st, (const float*)partial, nblk, theta, adam_m, adam_v,
                       step_scale_host[i], (float)beta1, (float)beta2, (float)eps);
    HIPCHK(hipGetLastError());
  }
  return DM_OK;
}
// the obs filter's update with a whole batch (src/trpo.py:242 `pi.ob_rms.update(ob)`): k_vf_rms on a grid sized to the batch — one launch
constexpr int RMS_UPDATE_BLOCKS = 256;              // (the last block adds the partials up column by column: 32 rounds of 8 loads)
extern "C" size_t dm_rms_scratch_bytes(void) { return (size_t)RMS_UPDATE_BLOCKS * 2 * dmv::OB * sizeof(double) + 64; }
extern "C" int dm_rms_update(const float* ob, int32_t n, double* rms_sum, double* rms_sumsq, double* rms_count, float* rms_mean, float* rms_std,
                             void* scratch, void* hip_stream) {
  if (!ob || n < 1 || !rms_sum || !rms_sumsq || !rms_count || !rms_mean || !rms_std || !scratch) return fail(DM_EINVAL, "dm_rms_update: bad argument");
  if (set_device_of(ob)) return fail(DM_EHIP, "dm_rms_update: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  int blocks = (n + 255) / 256;                               // >= 64 rows per row group of a block
  if (blocks > RMS_UPDATE_BLOCKS) blocks = RMS_UPDATE_BLOCKS;
  double* part = (double*)scratch;
  unsigned* ticket = (unsigned*)(part + (size_t)RMS_UPDATE_BLOCKS * 2 * dmv::OB);
  HIPCHK(hipMemsetAsync(ticket, 0, sizeof(unsigned), st));
  hipLaunchKernelGGL(dmv::k_vf_rms, dim3(blocks), dim3(256), 0, st, ob, (int)n, part, ticket, rms_sum, rms_sumsq, rms_count, rms_mean, rms_std);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
// ---- policy half of the TRPO update (csrc/pg_kernel.h) -------------------------------------------------------------------------
// one block per CU; `max_blocks` (0: all of them) leaves CUs to a kernel of another stream (the value fit beside the policy step)
static int pg_blocks(int ntiles, int max_blocks) {
  const int cap = (max_blocks > 0 && max_blocks < dmg::MAX_BLOCKS) ? max_blocks : dmg::MAX_BLOCKS;
  return ntiles < cap ? ntiles : cap;
}
extern "C" int dm_pg_param_count(void) { return dmg::NP; }
extern "C" size_t dm_pg_scratch_bytes(void) { return (size_t)dmg::MAX_BLOCKS * dmg::NPAD * sizeof(float) + (size_t)dmg::MAX_BLOCKS * 2 * sizeof(double) + 256; }
extern "C" int dm_pg_losses(const float* ob, int32_t n, const float* ac, const float* atarg, float* old_mean, const float* old_logstd, int32_t write_old,
                            const float* theta, const float* rms_mean, const float* rms_std, double entcoeff, int32_t with_grad,
                            float* out_grad, double* out_losses, void* scratch, void* hip_stream, int32_t max_blocks) {
  if (!ob || !ac || !atarg || !old_mean || !old_logstd || !theta || !rms_mean || !rms_std || !out_losses || !scratch || n < 1 || (with_grad && !out_grad) || max_blocks < 0 ||
      !aligned16(theta))
    return fail(DM_EINVAL, "dm_pg_losses: bad argument");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_pg_losses: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  const int ntiles = (n + dmg::SB - 1) / dmg::SB, nblk = pg_blocks(ntiles, max_blocks);
  float* partial = (float*)scratch;
  double* lpart = (double*)((char*)scratch + (((size_t)dmg::MAX_BLOCKS * dmg::NPAD * sizeof(float) + 255) / 256) * 256);
  if (with_grad)
    hipLaunchKernelGGL(dmg::k_pg<dmg::MODE_GRAD>, dim3(nblk), dim3(256), 0, st, ob, 1, (int)n, ac, atarg, old_mean, old_logstd, (int)write_old, theta,
                       (const float*)nullptr, rms_mean, rms_std, 1.0f / (float)n, partial, lpart, dmg::BcArgs{});
  else
    hipLaunchKernelGGL(dmg::k_pg<dmg::MODE_LOSS>, dim3(nblk), dim3(256), 0, st, ob, 1, (int)n, ac, atarg, old_mean, old_logstd, (int)write_old, theta,
                       (const float*)nullptr, rms_mean, rms_std, 1.0f / (float)n, partial, lpart, dmg::BcArgs{});
  hipLaunchKernelGGL(dmg::k_pg_reduce, dim3((dmg::NP + 255) / 256), dim3(256), 0, st, (const float*)partial, (const double*)lpart, nblk,
                     with_grad ? (int)dmg::MODE_GRAD : (int)dmg::MODE_LOSS, (float)entcoeff, (const float*)nullptr, 1.0 / (double)n, out_grad, out_losses);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_pg_fvp(const float* ob, int32_t stride, int32_t n, const float* theta, const float* v, const float* rms_mean, const float* rms_std,
                         float* out_fv, void* scratch, void* hip_stream, int32_t max_blocks) {
  if (!ob || !theta || !v || !rms_mean || !rms_std || !out_fv || !scratch || n < 1 || stride < 1 || max_blocks < 0 || !aligned16(theta))
    return fail(DM_EINVAL, "dm_pg_fvp: bad argument");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_pg_fvp: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  const int ntiles = (n + dmg::SB - 1) / dmg::SB, nblk = pg_blocks(ntiles, max_blocks);
  float* partial = (float*)scratch;
  double* lpart = (double*)((char*)scratch + (((size_t)dmg::MAX_BLOCKS * dmg::NPAD * sizeof(float) + 255) / 256) * 256);
  hipLaunchKernelGGL(dmg::k_pg<dmg::MODE_FVP>, dim3(nblk), dim3(256), 0, st, ob, (int)stride, (int)n, (const float*)nullptr, (const float*)nullptr,
                     (float*)nullptr, (const float*)nullptr, 0, theta, v, rms_mean, rms_std, 1.0f / (float)n, partial, lpart, dmg::BcArgs{});
  hipLaunchKernelGGL(dmg::k_pg_reduce, dim3((dmg::NP + 255) / 256), dim3(256), 0, st, (const float*)partial, (const double*)lpart, nblk, (int)dmg::MODE_FVP,
                     0.0f, v, 1.0 / (double)n, out_fv, (double*)nullptr);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
// ---- the GAIL discriminator (csrc/disc_kernel.h) --------------------------------------------------------------------------------
static int disc_blocks(int n) { return (n + dmd::SB - 1) / dmd::SB; }
extern "C" int dm_disc_param_count(void) { return dmd::NP; }
extern "C" size_t dm_disc_scratch_bytes(int32_t n_g, int32_t n_e) {
  if (n_g < 1 || n_e < 1) return 0;
  return (size_t)(disc_blocks(n_g) + disc_blocks(n_e)) * dmd::NPAD * sizeof(float);
}
extern "C" int dm_disc_reward(const float* theta, const float* rms_mean, const float* rms_std, const double* ob, const double* ac, int32_t n, double* reward,
                              void* hip_stream) {
  if (!theta || !rms_mean || !rms_std || !ob || !ac || !reward || n < 1 || !aligned16(theta)) return fail(DM_EINVAL, "dm_disc_reward: bad argument");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_disc_reward: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_disc_reward: hipSetDevice failed");
  hipLaunchKernelGGL(dmd::k_disc_reward, dim3(disc_blocks(n)), dim3(256), 0, (hipStream_t)hip_stream, ob, ac, (int)n, theta, rms_mean, rms_std, reward);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_disc_lossgrad(const float* theta, const float* rms_mean, const float* rms_std, const float* g_ob, const float* g_ac, int32_t n_g,
                                const float* e_ob, const float* e_ac, int32_t n_e, double entcoeff, float* out_grad, double* out_losses, void* scratch,
                                size_t scratch_bytes, void* hip_stream) {
  if (!theta || !rms_mean || !rms_std || !g_ob || !g_ac || !e_ob || !e_ac || !out_grad || !out_losses || !scratch || n_g < 1 || n_e < 1 || !aligned16(theta) ||
      !(entcoeff == entcoeff) || (int64_t)disc_blocks(n_g) + disc_blocks(n_e) > INT32_MAX / dmd::NPAD)
    return fail(DM_EINVAL, "dm_disc_lossgrad: bad argument");
  if (scratch_bytes < dm_disc_scratch_bytes(n_g, n_e)) return fail(DM_EINVAL, "dm_disc_lossgrad: scratch smaller than dm_disc_scratch_bytes(n_g, n_e)");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_disc_lossgrad: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_disc_lossgrad: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  const int nbg = disc_blocks(n_g), nblk = nbg + disc_blocks(n_e);
  float* partial = (float*)scratch;
  hipLaunchKernelGGL(dmd::k_disc_grad, dim3(nblk), dim3(256), 0, st, g_ob, g_ac, (int)n_g, e_ob, e_ac, (int)n_e, nbg, theta, rms_mean, rms_std,
                     (float)entcoeff, partial);
  hipLaunchKernelGGL(dmd::k_disc_reduce, dim3(dmd::RED_BLOCKS + 1), dim3(256), 0, st, (const float*)partial, nblk, nbg,
                     (int)n_g, (int)n_e, (float)entcoeff, out_grad, out_losses);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
// ---- behaviour cloning of the policy on expert transitions (csrc/pg_kernel.h MODE_BC) -----------------------------------------------
static int bc_blocks(int n) { return pg_blocks((n + dmg::SB - 1) / dmg::SB, 0); }
static size_t bc_lpart_offset(int n) { return up256((size_t)bc_blocks(n) * dmg::NPAD * sizeof(float)); }
extern "C" size_t dm_bc_scratch_bytes(int32_t bs) {
  if (bs < 1) return 0;
  return bc_lpart_offset(bs) + (size_t)bc_blocks(bs) * 2 * sizeof(double);
}
// k_pg<BC> over rows idx[0 .. n) (or 0 .. n) and the reduction: partial / lpart in scratch (dm_bc_scratch_bytes(n) bytes)
static void bc_launch(const float* ob_all, const float* ac_all, const int32_t* idx, int n, const float* theta, const float* rms_mean, const float* rms_std,
                      int stochastic, uint64_t seed, uint64_t counter, int grad, void* scratch, hipStream_t st) {
  float* partial = (float*)scratch;
  double* lpart = (double*)((char*)scratch + bc_lpart_offset(n));
  const dmg::BcArgs bc{idx, (unsigned long long)seed, (unsigned long long)counter, stochastic ? 1 : 0, grad};
  hipLaunchKernelGGL(dmg::k_pg<dmg::MODE_BC>, dim3(bc_blocks(n)), dim3(256), 0, st, ob_all, 1, n, ac_all, (const float*)nullptr, (float*)nullptr,
                     (const float*)nullptr, 1, theta, (const float*)nullptr, rms_mean, rms_std, (float)(1.0 / (28.0 * (double)n)), partial, lpart, bc);
}
extern "C" int dm_bc_lossgrad(const float* ob_all, const float* ac_all, const int32_t* idx, int32_t n, const float* theta, const float* rms_mean,
                              const float* rms_std, int32_t stochastic, uint64_t seed, uint64_t counter, float* out_grad, double* out_loss, void* scratch,
                              size_t scratch_bytes, void* hip_stream) {
  if (!ob_all || !ac_all || !theta || !rms_mean || !rms_std || !out_loss || !scratch || n < 1 || n > INT32_MAX / dmg::AC || !aligned16(theta))
    return fail(DM_EINVAL, "dm_bc_lossgrad: bad argument");
  if (scratch_bytes < dm_bc_scratch_bytes(n)) return fail(DM_EINVAL, "dm_bc_lossgrad: scratch smaller than dm_bc_scratch_bytes(n)");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_bc_lossgrad: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_bc_lossgrad: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  bc_launch(ob_all, ac_all, idx, (int)n, theta, rms_mean, rms_std, (int)stochastic, seed, counter, out_grad ? 1 : 0, scratch, st);
  const float* partial = (const float*)scratch;
  const double* lpart = (const double*)((const char*)scratch + bc_lpart_offset(n));
  hipLaunchKernelGGL(dmg::k_pg_reduce, dim3(out_grad ? (dmg::NP + 255) / 256 : 1), dim3(256), 0, st, partial, lpart, bc_blocks(n), (int)dmg::MODE_BC, 0.0f,
                     (const float*)nullptr, 1.0 / (28.0 * (double)n), out_grad, out_loss);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_bc_fit(const float* ob_all, const float* ac_all, const int32_t* idx, int32_t iters, int32_t bs, float* theta, float* adam_m, float* adam_v,
                         const float* step_scale_host, double beta1, double beta2, double eps, const float* rms_mean, const float* rms_std, int32_t stochastic,
                         uint64_t seed, uint64_t counter0, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream) {
  if (!ob_all || !ac_all || !theta || !adam_m || !adam_v || !step_scale_host || !rms_mean || !rms_std || !out_loss || !scratch || iters < 1 || bs < 1 ||
      bs > INT32_MAX / dmg::AC || !aligned16(theta) || !std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps))
    return fail(DM_EINVAL, "dm_bc_fit: bad argument");
  for (int i = 0; i < iters; i++) if (!std::isfinite(step_scale_host[i])) return fail(DM_EINVAL, "dm_bc_fit: non-finite step scale");
  if (scratch_bytes < dm_bc_scratch_bytes(bs)) return fail(DM_EINVAL, "dm_bc_fit: scratch smaller than dm_bc_scratch_bytes(bs)");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_bc_fit: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_bc_fit: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  const float* partial = (const float*)scratch;
  const double* lpart = (const double*)((const char*)scratch + bc_lpart_offset(bs));
  for (int i = 0; i < iters; i++) {
    bc_launch(ob_all, ac_all, idx ? idx + (size_t)i * bs : nullptr, (int)bs, theta, rms_mean, rms_std, (int)stochastic, seed, counter0 + (uint64_t)i, 1, scratch, st);
    hipLaunchKernelGGL(dmg::k_bc_adam, dim3((dmg::NP + 255) / 256), dim3(256), 0, st, partial, lpart, bc_blocks(bs), 1.0 / (28.0 * (double)bs), theta, adam_m,
                       adam_v, step_scale_host[i], (float)beta1, (float)beta2, (float)eps, out_loss + i);
  }
  HIPCHK(hipGetLastError());
  return DM_OK;
}
// ---- PPO's clipped-surrogate update of the policy and the value net (csrc/pg_kernel.h MODE_PPO, k_ppo_step; vf_kernel.h k_vf_grad_rows) -----
// scratch: both halves' loss sums first (their offsets do not depend on n), then the gradient partials of a call with the gradient
static int ppo_vf_blocks(int n, int grad) { const int t = (n + dmv::SB - 1) / dmv::SB; return grad ? t : (t < dmg::MAX_BLOCKS ? t : dmg::MAX_BLOCKS); }
static_assert(dmg::NP % 4 == 0, "the value half of a PPO theta starts 16-byte aligned");
struct PpoScratch { size_t pg_lp, vf_lp, pg_part, vf_part, total; };
static PpoScratch ppo_scratch_layout(int n, int grad) {
  PpoScratch L;
  size_t o = 0;
  L.pg_lp = o; o += up256((size_t)dmg::MAX_BLOCKS * dmg::PPO_LP * sizeof(double));
  const int vb = ppo_vf_blocks(n, grad);
  L.vf_lp = o; o += up256((size_t)(vb > dmg::MAX_BLOCKS ? vb : dmg::MAX_BLOCKS) * sizeof(double));
  L.pg_part = o; if (grad) o += up256((size_t)pg_blocks((n + dmg::SB - 1) / dmg::SB, 0) * dmg::NPAD * sizeof(float));
  L.vf_part = o; if (grad) o += up256((size_t)vb * dmv::NPAD * sizeof(float));
  L.total = o;
  return L;
}
extern "C" size_t dm_ppo_scratch_bytes(int32_t bs) {
  if (bs < 1 || bs > INT32_MAX / dmg::AC) return 0;
  return ppo_scratch_layout((int)bs, 1).total;
}
struct PpoRows { const float *ob, *ac, *atarg, *old_mean, *old_logstd, *ret; };
// k_pg<PPO> and k_vf_grad_rows over rows idx[0 .. n) (or 0 .. n): partials and loss sums in scratch; -> the two grids
static void ppo_grad_launch(const PpoRows& R, const int32_t* idx, int n, const float* theta, const float* rms_mean, const float* rms_std, float clip,
                            int grad, const PpoScratch& L, void* scratch, hipStream_t st, int* pg_nblk, int* vf_nblk) {
  char* base = (char*)scratch;
  *pg_nblk = pg_blocks((n + dmg::SB - 1) / dmg::SB, 0);
  *vf_nblk = ppo_vf_blocks(n, grad);
  const dmg::BcArgs pa{idx, 0ull, 0ull, 0, grad, clip};
  hipLaunchKernelGGL(dmg::k_pg<dmg::MODE_PPO>, dim3(*pg_nblk), dim3(256), 0, st, R.ob, 1, n, R.ac, R.atarg, (float*)R.old_mean, R.old_logstd, 0, theta,
                     (const float*)nullptr, rms_mean, rms_std, 1.0f / (float)n, (float*)(base + L.pg_part), (double*)(base + L.pg_lp), pa);
  if (grad)
    hipLaunchKernelGGL(dmv::k_vf_grad_rows<true>, dim3(*vf_nblk), dim3(256), 0, st, R.ob, R.ret, idx, n, theta + dmg::NP, rms_mean, rms_std,
                       (float*)(base + L.vf_part), (double*)(base + L.vf_lp));
  else
    hipLaunchKernelGGL(dmv::k_vf_grad_rows<false>, dim3(*vf_nblk), dim3(256), 0, st, R.ob, R.ret, idx, n, theta + dmg::NP, rms_mean, rms_std,
                       (float*)nullptr, (double*)(base + L.vf_lp));
}
static bool ppo_rows_ok(const PpoRows& R) { return R.ob && R.ac && R.atarg && R.old_mean && R.old_logstd && R.ret; }
extern "C" int dm_ppo_lossgrad(const float* ob_all, const float* ac_all, const float* atarg_all, const float* old_mean_all, const float* old_logstd,
                               const float* ret_all, const int32_t* idx, int32_t n, const float* theta, const float* rms_mean, const float* rms_std,
                               double clip, double entcoeff, float* out_grad, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream) {
  const PpoRows R{ob_all, ac_all, atarg_all, old_mean_all, old_logstd, ret_all};
  if (!ppo_rows_ok(R) || !theta || !rms_mean || !rms_std || !out_loss || !scratch || n < 1 || n > INT32_MAX / dmg::AC || !aligned16(theta) ||
      !std::isfinite(clip) || clip < 0.0 || !std::isfinite(entcoeff))
    return fail(DM_EINVAL, "dm_ppo_lossgrad: bad argument");
  const int grad = out_grad ? 1 : 0;
  const PpoScratch L = ppo_scratch_layout((int)n, grad);
  if (scratch_bytes < L.total) return fail(DM_EINVAL, "dm_ppo_lossgrad: scratch smaller than dm_ppo_scratch_bytes(n)");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_ppo_lossgrad: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_ppo_lossgrad: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  int pg_nblk, vf_nblk;
  ppo_grad_launch(R, idx, (int)n, theta, rms_mean, rms_std, (float)clip, grad, L, scratch, st, &pg_nblk, &vf_nblk);
  const char* base = (const char*)scratch;
  hipLaunchKernelGGL(dmg::k_ppo_step, dim3(grad ? dmg::PPO_STEP_BLOCKS : 1), dim3(256), 0, st, (const float*)(base + L.pg_part),
                     (const double*)(base + L.pg_lp), pg_nblk, (const float*)(base + L.vf_part), (const double*)(base + L.vf_lp), vf_nblk,
                     1.0 / (double)n, (float)entcoeff, (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.0f, 0.0f, 0.0f, 0.0f, out_grad, out_loss);
  HIPCHK(hipGetLastError());
  return DM_OK;
}
extern "C" int dm_ppo_fit(const float* ob_all, const float* ac_all, const float* atarg_all, const float* old_mean_all, const float* old_logstd,
                          const float* ret_all, const int32_t* idx, int32_t iters, int32_t bs, float* theta, float* adam_m, float* adam_v,
                          const float* step_scale_host, const float* clip_host, double beta1, double beta2, double eps, double entcoeff,
                          const float* rms_mean, const float* rms_std, double* out_loss, void* scratch, size_t scratch_bytes, void* hip_stream) {
  const PpoRows R{ob_all, ac_all, atarg_all, old_mean_all, old_logstd, ret_all};
  if (!ppo_rows_ok(R) || !theta || !adam_m || !adam_v || !step_scale_host || !clip_host || !rms_mean || !rms_std || !out_loss || !scratch || iters < 1 ||
      bs < 1 || bs > INT32_MAX / dmg::AC || !aligned16(theta) || !std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) ||
      !std::isfinite(entcoeff))
    return fail(DM_EINVAL, "dm_ppo_fit: bad argument");
  for (int i = 0; i < iters; i++)
    if (!std::isfinite(step_scale_host[i]) || !std::isfinite(clip_host[i]) || clip_host[i] < 0.0f) return fail(DM_EINVAL, "dm_ppo_fit: bad step scale or clip");
  const PpoScratch L = ppo_scratch_layout((int)bs, 1);
  if (scratch_bytes < L.total) return fail(DM_EINVAL, "dm_ppo_fit: scratch smaller than dm_ppo_scratch_bytes(bs)");
  if (!have_device()) return fail(DM_ENODEVICE, "dm_ppo_fit: no HIP device visible (libdmenv has no CPU path)");
  if (set_device_of(theta)) return fail(DM_EHIP, "dm_ppo_fit: hipSetDevice failed");
  hipStream_t st = (hipStream_t)hip_stream;
  const char* base = (const char*)scratch;
  for (int i = 0; i < iters; i++) {
    int pg_nblk, vf_nblk;
    ppo_grad_launch(R, idx ? idx + (size_t)i * bs : nullptr, (int)bs, theta, rms_mean, rms_std, clip_host[i], 1, L, scratch, st, &pg_nblk, &vf_nblk);
    hipLaunchKernelGGL(dmg::k_ppo_step, dim3(dmg::PPO_STEP_BLOCKS), dim3(256), 0, st, (const float*)(base + L.pg_part), (const double*)(base + L.pg_lp),
                       pg_nblk, (const float*)(base + L.vf_part), (const double*)(base + L.vf_lp), vf_nblk, 1.0 / (double)bs, (float)entcoeff, theta,
                       adam_m, adam_v, step_scale_host[i], (float)beta1, (float)beta2, (float)eps, (float*)nullptr, out_loss + (size_t)i * DM_PPO_NLOSS);
  }
  HIPCHK(hipGetLastError());
  return DM_OK;
}
