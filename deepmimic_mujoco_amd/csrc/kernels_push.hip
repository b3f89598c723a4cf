// kernels_push.hip — the two launches of external pushes (push_kernel.h): k_push_now behind dm_batch_push and k_push, the random schedule's
// launch ahead of every per-step launch while dm_batch_set_push_schedule has one set.  A translation unit of its own with dmenv.hip's default backend options:
// the step kernels' code objects are not touched, and with the schedule off neither kernel is launched.  One 64-lane wave per environment; no four-per-wave form.
#define DM_NO_LAUNCH_KERNELS
#include "kernels.h"
#include "push_kernel.h"

using namespace dm;

__global__ __launch_bounds__(64) void k_push_now(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const int* __restrict__ body, const double* __restrict__ impulse,
                                                 const unsigned char* __restrict__ mask) {
  __shared__ Shared<Real> s;
  const int env = blockIdx.x;
  if (env >= B.n_envs) return;
  push_now_wave(*Mp, B, s, env, dmw::lane(), body, impulse, mask);
}

__global__ __launch_bounds__(64) void k_push(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, PushArgs P) {
  __shared__ Shared<Real> s;
  if ((int)blockIdx.x >= P.count) return;
  push_schedule_wave(*Mp, B, s, P, P.first + (int)blockIdx.x, dmw::lane());
}
