// kernels.h — what the translation units of libdmenv.so with environment kernels share: the build's arithmetic type and the prototypes of the step
// kernels that one unit defines and dmenv.hip launches.  The library's twelve units (csrc/build.py UNITS):
//   dmenv.hip           one-env step kernels of action modes 0..2, reset / state / ordering / render / state-feature / termination kernels, the batch half of the C ABI
//                       (host side: models, mocap, batches, options, state, step / rollout / queue, profiling and timing)
//   views.hip           dm_batch_render, dm_batch_state_features and dm_batch_floor_contacts (host side: one prologue, one staging helper over view_stage.h; kernels in dmenv.hip's unit)
//   learner.hip         the learner half of the C ABI with its kernels (policy_kernel.h, vf_kernel.h, pg_kernel.h, disc_kernel.h); does not include this file
//   kernels_rollout.hip the horizon launch (k_rollout_packed + the step bodies it calls): the packed options and the load-store vectoriser off
//   kernels_rollout_term.hip   the horizon launch with early termination inside (k_rollout_packed_term, DM_OPT_HORIZON_TERMINATION: slot_term.h), with the
//                       options of kernels_rollout.hip; a unit of its own so that k_rollout_packed stays the code object it was
//   kernels_rollout_spd.hip    the two horizon launches in action modes 3 and 4 (k_rollout_packed_spd, k_rollout_packed_term_spd, DM_OPT_HORIZON_SPD: slot_rollout's
//                       SPD switch), with the options of kernels_rollout.hip; a unit of its own for the same reason
//   kernels_spd.hip / kernels_packed_spd.hip   the one-env and the packed step kernels of action modes 3 and 4 (stable PD control per substep), units
//                       of their own with the options of dmenv.hip / kernels_packed.hip: the kernels of modes 0..2 carry no controller code
//   kernels_clips.hip / kernels_packed_clips.hip   the kernels of MULTI-CLIP batches (dm_mocap_create_set: one clip per env, step_rules.h ClipArgs): the one-env and
//                       the packed step kernels, and the clip forms of k_reset, k_terminate, k_state_features and k_imitation_terms; units of their own with the
//                       options of dmenv.hip / kernels_packed.hip.  They pick the stable-PD instantiation by the action mode at run time.
//   kernels_push.hip    external pushes (push_kernel.h): k_push_now behind dm_batch_push and k_push, the random schedule's launch ahead of every per-step launch;
//                       a unit of its own with dmenv.hip's options, launched only where a push is asked for
//   kernels_packed.hip  the four-environments-per-wavefront per-step kernels (slot_kernel.h / slot_step.h): compiled with their own backend options
//                       (csrc/build.py PACKED_FLAGS — one wave per SIMD with the whole register file wants a scheduler that goes for
//                       instruction-level parallelism, the two-waves-per-SIMD one-env kernels do not: profiles/r04_ab_kernel_variants.md)
#pragma once
#include <cstddef>
#include <hip/hip_runtime.h>

#include "dmenv.h"
#include "policy_kernel.h"
#include "env_step.h"
#include "slot_step.h"

// Arithmetic / device-state type of this build: float64 (libdmenv.so, the parity build) or float32 (libdmenv32.so, -DDM_REAL_FLOAT:
// the `dtype 32` batch of SURVEY.md section 8b — same kernels, half the registers and LDS per env).  Everything that crosses the
// C ABI (actions, observations, rewards, field reads / writes, mocap tables) stays float64 (`Ext`) in both builds.
#ifdef DM_REAL_FLOAT
typedef float Real;
#define DM_STEP_WAVES 3
#else
typedef double Real;
#define DM_STEP_WAVES 2
#endif
typedef double Ext;

#ifndef DM_NARROW_ROWS
#define DM_NARROW_ROWS 32
#endif
constexpr int NARROW_ROWS = DM_NARROW_ROWS;
// The one-env step a packed horizon launch falls back to for an environment beyond the packed path's 32 rows (restep_one_env, slot_step.h): those
// environments hold 33 .. 37 rows (a standing humanoid: 8 foot corners x 4 pyramid edges + joint limits; profiles/r04_ab_kernel_variants.md).  With the
// 32-column register tier every PGS sweep fetches their last columns of A from the memory strip; the wave is alone on its SIMD here, so the tier is 48
// columns: no strip below 49 rows.  Worth 4 % of a re-step (734 k -> 705 k cycles: the one-env step of such an environment is 680 k cycles by itself,
// 300 k of it the 36-row sweeps), 1.4 % of a standing population's horizon.
#ifndef DM_RESTEP_ROWS
#define DM_RESTEP_ROWS 48
#endif
constexpr int RESTEP_ROWS = DM_RESTEP_ROWS;

// the table of per-step buffers of a horizon launch arrives a chunk per launch in the kernel-argument segment (k_put_rows)
constexpr int ROW_CHUNK = 64;
struct StepRowChunk { dm::StepRow r[ROW_CHUNK]; };

// ---- kernels_packed.hip ------------------------------------------------------------------------------------------------------------
__global__ void k_step_packed(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                              unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count);
__global__ void k_step_packed_act(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa);
__global__ void k_step_packed_ext(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count);
__global__ void k_step_packed_act_ext(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                      unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa);
__global__ void k_rollout_packed(const dm::DevModel<Real>* __restrict__ Mp, const dm::Batch<Real>* __restrict__ Bp, const dm::StepRow* __restrict__ rows, int n_substeps, int first,
                                 int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk);
__global__ void k_step_packed_prof(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                   unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, long long* __restrict__ prof);
// ---- kernels_rollout_term.hip ------------------------------------------------------------------------------------------------------
struct TermArgs;       // (term_kernel.h)
__global__ void k_rollout_packed_term(const dm::DevModel<Real>* __restrict__ Mp, const dm::Batch<Real>* __restrict__ Bp, const dm::StepRow* __restrict__ rows, int n_substeps, int first,
                                      int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk, TermArgs ta);
// ---- kernels_rollout_spd.hip: the two horizon launches in action modes 3 and 4 (DM_OPT_HORIZON_SPD) --------------------------------------------------------
__global__ void k_rollout_packed_spd(const dm::DevModel<Real>* __restrict__ Mp, const dm::Batch<Real>* __restrict__ Bp, const dm::StepRow* __restrict__ rows, int n_substeps, int first,
                                     int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk);
__global__ void k_rollout_packed_term_spd(const dm::DevModel<Real>* __restrict__ Mp, const dm::Batch<Real>* __restrict__ Bp, const dm::StepRow* __restrict__ rows, int n_substeps, int first,
                                          int count, int T, dmp::PolicyArgs pa, long long* __restrict__ wave_clk, TermArgs ta);
// ---- kernels_packed_spd.hip, kernels_spd.hip: the same launches in action modes 3 and 4 -----------------------------------------------------
__global__ void k_step_packed_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                              unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count);
__global__ void k_step_packed_act_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa);
__global__ void k_step_packed_ext_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count);
__global__ void k_step_packed_act_ext_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                      unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa);
__global__ void k_step_packed_prof_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                   unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, long long* __restrict__ prof);
__global__ void k_step_narrow_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, int count);
__global__ void k_step_act_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                               unsigned char* __restrict__ done, int n_substeps, int first, int count, dmp::PolicyArgs pa);
__global__ void k_step_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                           unsigned char* __restrict__ done, int n_substeps);
__global__ void k_step_redo_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                unsigned char* __restrict__ done, int n_substeps, int first, const int* __restrict__ redo_count, int* __restrict__ redo_count_next, dmp::PolicyArgs pa);
__global__ void k_step_prof_spd(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                unsigned char* __restrict__ done, int n_substeps, long long* prof);
// ---- kernels_packed_clips.hip, kernels_clips.hip: the same launches on a multi-clip batch (the clip argument last; action modes 0..4) ------------------
__global__ void k_step_packed_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                    unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dm::ClipArgs<Real> ca);
__global__ void k_step_packed_ext_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                        unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dm::ClipArgs<Real> ca);
__global__ void k_step_packed_act_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                        unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa, dm::ClipArgs<Real> ca);
__global__ void k_step_packed_act_ext_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                            unsigned char* __restrict__ done, int n_substeps, int first, int count, int* __restrict__ redo_count, dmp::PolicyArgs pa, dm::ClipArgs<Real> ca);
__global__ void k_step_narrow_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                    unsigned char* __restrict__ done, int n_substeps, int first, int count, dm::ClipArgs<Real> ca);
__global__ void k_step_act_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                 unsigned char* __restrict__ done, int n_substeps, int first, int count, dmp::PolicyArgs pa, dm::ClipArgs<Real> ca);
__global__ void k_step_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                             unsigned char* __restrict__ done, int n_substeps, dm::ClipArgs<Real> ca);
__global__ void k_step_redo_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const Ext* __restrict__ action, Ext* __restrict__ obs, Ext* __restrict__ reward,
                                  unsigned char* __restrict__ done, int n_substeps, int first, const int* __restrict__ redo_count, int* __restrict__ redo_count_next, dmp::PolicyArgs pa,
                                  dm::ClipArgs<Real> ca);
__global__ void k_clip_clamp(dm::Batch<Real> B, dm::ClipArgs<Real> ca);
__global__ void k_reset_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, int mode, int hard, const unsigned char* __restrict__ mask, dm::ClipArgs<Real> ca);
__global__ void k_terminate_clips(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, TermArgs T, Ext* __restrict__ obs, unsigned char* __restrict__ done, dm::ClipArgs<Real> ca);
// ---- kernels_push.hip: external pushes (push_kernel.h), one wave per environment -----------------------------------------------------------------------
namespace dm { struct PushArgs; }
__global__ void k_push_now(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, const int* __restrict__ body, const double* __restrict__ impulse,
                           const unsigned char* __restrict__ mask);
__global__ void k_push(const dm::DevModel<Real>* __restrict__ Mp, dm::Batch<Real> B, dm::PushArgs P);
