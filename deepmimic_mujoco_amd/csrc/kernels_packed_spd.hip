// kernels_packed_spd.hip — the four-environments-per-wavefront step kernels of action modes 3 and 4 (stable PD control per substep: slot_step.h
// slot_spd_control).  The kernels of kernels_packed.hip with the controller compiled in (packed_body.h, SPD = true), in a translation unit of their own so
// that the kernels of modes 0..2 stay the code objects they were; built with the same backend options (csrc/build.py PACKED_FLAGS).
#define DM_NO_LAUNCH_KERNELS
#include "packed_body.h"

using namespace dm;

__global__ __launch_bounds__(64) void k_step_packed_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count) {
  step_packed_body<2 * SW, true>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count);
}
__global__ __launch_bounds__(64) void k_step_packed_ext_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count) {
  step_packed_body<SLOT_MAXROWS, true>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count);
}
__global__ __launch_bounds__(64) void k_step_packed_act_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa) {
  step_packed_act_body<2 * SW, true>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, pa);
}
__global__ __launch_bounds__(64) void k_step_packed_act_ext_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa) {
  step_packed_act_body<SLOT_MAXROWS, true>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, pa);
}
__global__ __launch_bounds__(64) void k_step_packed_prof_spd(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const Ext* __restrict__ action,
    Ext* __restrict__ obs, Ext* __restrict__ reward, unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, long long* __restrict__ prof) {
  step_packed_prof_body<true>(Mp, B, action, obs, reward, done, n_substeps, first, count, redo_count, prof);
}
