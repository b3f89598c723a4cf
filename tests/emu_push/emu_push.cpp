// emu_push.cpp — TEST INFRASTRUCTURE: the wave testbench's front end for external pushes (csrc/push_kernel.h; the device's kernels_push.hip).  The EmuBatch
// and the emu_* entry points are those of ../emu/emu_main.cpp, compiled into this library as they are (with it the fibre runner of ../emu/wave_fibres.h and the
// host batch of ../emu/host_batch.h); the emup_* entry points below run the
// two kernels' waves (push_now_wave, push_schedule_wave — the unmodified kernel source) one environment after another, with the schedule's records kept by the
// caller beside the EmuBatch, as the device keeps its PushArgs beside the Batch.
#include "../emu/emu_main.cpp"
#include "push_kernel.h"

extern "C" {
// k_push_now: body [n], impulse [n, 3], mask [n] or null
void emup_push(void* h, const int* body, const double* impulse, const unsigned char* mask) {
  EmuBatch* e = (EmuBatch*)h;
  for (int env = 0; env < e->B.n_envs; env++)
    run_wave([&](int lane) { push_now_wave(e->M, e->B, e->sh, env, lane, body, impulse, mask); });
}
// k_push ahead of one step: state [n, 5] and force [n, 3] are DM_F_PUSH_STATE / DM_F_PUSH_FORCE; hstep = timestep * n_substeps
void emup_schedule(void* h, const dm_push_desc* d, int* state, double* force, double hstep) {
  EmuBatch* e = (EmuBatch*)h;
  const PushArgs P{state, force, d->bodies, d->wait_min, d->wait_max, d->duration_min, d->duration_max, d->force_min, d->force_max, d->z_min, d->z_max, hstep, 0, e->B.n_envs};
  for (int env = 0; env < e->B.n_envs; env++)
    run_wave([&](int lane) { push_schedule_wave(e->M, e->B, e->sh, P, env, lane); });
}
}
