// views.hip — read-only views of a batch's environments: images (dm_batch_render), DeepMimic's state features (dm_batch_state_features), the
// floor-contact query (dm_batch_floor_contacts) and the imitation reward's terms (dm_batch_imitation_terms), DESIGN.md section 9.  Host side only: the
// kernels (render_kernel.h, state_kernel.h, term_kernel.h, terms_kernel.h) are compiled in dmenv.hip's unit, which see.  Every view is: view_args, its own argument rules, view_enter, the arrays it declares on a Stage,
// commit(), its launches on ptr(index), finish().
#define DM_NO_LAUNCH_KERNELS
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "render.h"
#include "view_stage.h"

using namespace dm;

__global__ void k_render_pose(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos, const double* __restrict__ qpos_ext,
                              const int* __restrict__ env_ids, dmr::Camera cam, dmr::ViewRec* __restrict__ rec, double* __restrict__ geom_xform);
__global__ void k_render_rays(const dmr::ViewRec* __restrict__ rec, dmr::Params P, int tiles_x, int view0, unsigned char* __restrict__ rgb,
                              float* __restrict__ depth, int* __restrict__ seg);
__global__ void k_state_features(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                 const double* __restrict__ qvel_ext, const double* __restrict__ phase_ext, const int* __restrict__ env_ids,
                                 Ext* __restrict__ out);
__global__ void k_imitation_terms(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                  const double* __restrict__ qvel_ext, const int* __restrict__ frame_ext, const int* __restrict__ cycle_ext,
                                  const int* __restrict__ env_ids, Ext* __restrict__ out);
__global__ void k_floor_contacts(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos, const double* __restrict__ qpos_ext,
                                 const int* __restrict__ env_ids, int* __restrict__ out);

// ... and their forms on a multi-clip batch (kernels_clips.hip)
__global__ void k_state_features_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                       const double* __restrict__ qvel_ext, const double* __restrict__ phase_ext, const int* __restrict__ env_ids,
                                       Ext* __restrict__ out, ClipArgs<Real> ca);
__global__ void k_imitation_terms_clips(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                        const double* __restrict__ qvel_ext, const int* __restrict__ frame_ext, const int* __restrict__ cycle_ext,
                                        const int* __restrict__ env_ids, Ext* __restrict__ out, ClipArgs<Real> ca);

// the argument checks every view starts with, in this order; nothing here touches a device.  required: the pointers the view cannot do without;
// explicit_state: the caller gave states of their own (`state_word` names them in the message) instead of the batch's
static int view_args(dm_batch* b, bool required, int kind, int n, bool explicit_state, const char* state_word, const int32_t* env_ids, const char* who) {
  if (!b || !required) return fail(DM_EINVAL, std::string(who) + ": null argument");
  if (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE) return fail(DM_EINVAL, std::string(who) + ": bad ptr_kind");
  if (n <= 0) return fail(DM_EINVAL, std::string(who) + ": n must be positive");
  if (explicit_state && env_ids) return fail(DM_EINVAL, std::string(who) + ": env_ids must be NULL when " + state_word + " is given");
  if (!explicit_state && n > b->n) return fail(DM_EINVAL, std::string(who) + ": n exceeds the batch size");
  return DM_OK;
}
// the first touch of the device: run what the batch has queued, then range-check the env ids on the host — before anything is allocated for the call.
// Ids given by device pointer are read back first: the one host wait of a device caller
static int view_enter(dm_batch* b, const int32_t* env_ids, int n, bool host, const char* who) {
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  if (!env_ids) return DM_OK;
  std::vector<int32_t> ids((size_t)n);
  if (host) std::memcpy(ids.data(), env_ids, (size_t)n * sizeof(int32_t));
  else { HIPCHK(hipMemcpyAsync(ids.data(), env_ids, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream)); HIPCHK(hipStreamSynchronize(b->stream)); }
  for (int i = 0; i < n; i++) if (ids[i] < 0 || ids[i] >= b->n) return fail(DM_EINVAL, std::string(who) + ": env id out of range");
  return DM_OK;
}
// grow the batch's staging buffer (d_rbuf) to `bytes`
static int grow_rbuf(dm_batch* b, size_t bytes, const char* who) {
  if (bytes <= b->rbuf_bytes) return DM_OK;
  HIPCHK(hipStreamSynchronize(b->stream));       // (the old buffer may still be read by an earlier call)
  if (b->d_rbuf) { HIPCHK(hipFree(b->d_rbuf)); b->d_rbuf = nullptr; b->rbuf_bytes = 0; }
  if (hipMalloc((void**)&b->d_rbuf, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(DM_ENOMEM, std::string(who) + ": hipMalloc failed"); }
  b->rbuf_bytes = bytes;
  return DM_OK;
}
// One call's arrays (view_stage.h has the layout).  A host caller's arrays are staged in d_rbuf: inputs copied in by commit(), outputs copied back by
// finish(), which then waits for the stream.  A device caller's arrays are used where they are and nothing waits; only scratch takes room in d_rbuf.
// in / out / scratch return the array's index; ptr(index) is what the kernel gets, valid once commit() has returned (the buffer may move when it grows)
struct Stage : dmst::Layout {
  dm_batch* b; const char* who;
  Stage(dm_batch* b_, int kind, const char* who_) : dmst::Layout(kind == DM_PTR_HOST), b(b_), who(who_) {}
  int in(const void* user, size_t bytes) { return add(dmst::COPY_IN, user, bytes); }
  int out(void* user, size_t bytes) { return add(dmst::COPY_OUT, user, bytes); }
  int scratch(size_t bytes) { return add(dmst::SCRATCH, nullptr, bytes); }
  template <class T> T* ptr(int i) const { return (T*)at(i, b->d_rbuf); }
  int commit() {
    if (full) return fail(DM_EINVAL, std::string(who) + ": more arrays than the staging table holds");
    const int rc = grow_rbuf(b, total, who);
    if (rc) return rc;
    for (int i = 0; i < n; i++) if (r[i].staged && r[i].dir == dmst::COPY_IN) HIPCHK(hipMemcpyAsync(b->d_rbuf + r[i].off, r[i].user, r[i].bytes, hipMemcpyHostToDevice, b->stream));
    return DM_OK;
  }
  int finish() {
    if (!host) return DM_OK;
    for (int i = 0; i < n; i++) if (r[i].staged && r[i].dir == dmst::COPY_OUT) HIPCHK(hipMemcpyAsync(r[i].user, b->d_rbuf + r[i].off, r[i].bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return DM_OK;
  }
};

// ------------------------------------------------------------------ rendering (render_kernel.h)
extern "C" int dm_batch_render(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, const dm_render_desc* d, uint8_t* rgb,
                               float* depth, int32_t* seg, double* geom_xform, int32_t kind) {
  const char* who = "dm_batch_render";
  int rc;
  if ((rc = view_args(b, d != nullptr, kind, n, qpos != nullptr, "qpos", env_ids, who))) return rc;
  const int W = d->width, H = d->height;
  if (W < 1 || W > 4096 || H < 1 || H > 4096) return fail(DM_EINVAL, "dm_batch_render: width and height must be 1..4096");
  const size_t npix = (size_t)n * W * H;
  if (npix >= (size_t)1 << 31) return fail(DM_EINVAL, "dm_batch_render: n * width * height must stay below 2^31");
  if (!(d->fovy > 0 && d->fovy < 180)) return fail(DM_EINVAL, "dm_batch_render: fovy must lie in (0, 180) degrees");
  if (!rgb && !depth && !seg && !geom_xform) return fail(DM_EINVAL, "dm_batch_render: no output requested");
  const double ln = std::sqrt(d->light_dir[0] * d->light_dir[0] + d->light_dir[1] * d->light_dir[1] + d->light_dir[2] * d->light_dir[2]);
  if (!(ln > 0)) return fail(DM_EINVAL, "dm_batch_render: light_dir must be nonzero");
  if (!(d->floor_square > 0)) return fail(DM_EINVAL, "dm_batch_render: floor_square must be positive");
  if ((rc = view_enter(b, env_ids, n, kind == DM_PTR_HOST, who))) return rc;
  Stage st(b, kind, who);
  const int i_rec = st.scratch((size_t)n * sizeof(dmr::ViewRec)), i_q = st.in(qpos, (size_t)n * NQ * sizeof(double)), i_id = st.in(env_ids, (size_t)n * sizeof(int32_t));
  const int i_rgb = st.out(rgb, npix * 3), i_dep = st.out(depth, npix * sizeof(float)), i_seg = st.out(seg, npix * sizeof(int32_t));
  const int i_xf = st.out(geom_xform, (size_t)n * NG * 12 * sizeof(double));
  if ((rc = st.commit())) return rc;
  dmr::ViewRec* rec = st.ptr<dmr::ViewRec>(i_rec);
  unsigned char* drgb = st.ptr<unsigned char>(i_rgb); float* ddep = st.ptr<float>(i_dep); int* dseg = st.ptr<int>(i_seg);
  dmr::Camera cam{};
  for (int k = 0; k < 3; k++) cam.pos[k] = d->cam_pos[k];
  for (int k = 0; k < 9; k++) cam.mat[k] = d->cam_mat[k];
  cam.track_com = d->track_com != 0;
  hipLaunchKernelGGL(k_render_pose, dim3(n), dim3(64), 0, b->stream, b->d_model, (const Real*)b->B.qpos, st.ptr<const double>(i_q), st.ptr<const int>(i_id), cam, rec,
                     st.ptr<double>(i_xf));
  HIPCHK(hipGetLastError());
  if (drgb || ddep || dseg) {
    const dmr::Params P = dmr::make_params(*d);
    const int tiles_x = (W + 15) / 16, tiles = tiles_x * ((H + 15) / 16);
    for (int v0 = 0; v0 < n; v0 += 65535) {
      const int nv = n - v0 < 65535 ? n - v0 : 65535;
      hipLaunchKernelGGL(k_render_rays, dim3(tiles, nv), dim3(256), 0, b->stream, (const dmr::ViewRec*)rec, P, tiles_x, v0, drgb, ddep, dseg);
      HIPCHK(hipGetLastError());
    }
  }
  return st.finish();
}

// ------------------------------------------------------------------ DeepMimic's state features (state_kernel.h)
extern "C" int dm_batch_state_features(dm_batch* b, const double* qpos, const double* qvel, const double* phase, const int32_t* env_ids, int32_t n,
                                       double* out, int32_t kind) {
  const char* who = "dm_batch_state_features";
  int rc;
  if ((rc = view_args(b, out != nullptr, kind, n, qpos || qvel || phase, "a state", env_ids, who))) return rc;
  if ((qpos || qvel || phase) && !(qpos && qvel && phase)) return fail(DM_EINVAL, "dm_batch_state_features: an explicit state needs qpos, qvel and phase");
  if ((rc = view_enter(b, env_ids, n, kind == DM_PTR_HOST, who))) return rc;
  Stage st(b, kind, who);
  const int i_q = st.in(qpos, (size_t)n * NQ * sizeof(double)), i_v = st.in(qvel, (size_t)n * NV * sizeof(double)), i_p = st.in(phase, (size_t)n * sizeof(double));
  const int i_id = st.in(env_ids, (size_t)n * sizeof(int32_t)), i_o = st.out(out, (size_t)n * DM_NSTATE * sizeof(double));
  if ((rc = st.commit())) return rc;
  launch_clip_or_plain(b, k_state_features, k_state_features_clips, dim3(n), dim3(64), b->stream, b->d_model, b->B, st.ptr<const double>(i_q), st.ptr<const double>(i_v),
                       st.ptr<const double>(i_p), st.ptr<const int>(i_id), st.ptr<Ext>(i_o));
  HIPCHK(hipGetLastError());
  return st.finish();
}

// ------------------------------------------------------------------ which geoms touch the floor (term_kernel.h)
extern "C" int dm_batch_floor_contacts(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, int32_t* out, int32_t kind) {
  const char* who = "dm_batch_floor_contacts";
  int rc;
  if ((rc = view_args(b, out != nullptr, kind, n, qpos != nullptr, "qpos", env_ids, who))) return rc;
  if ((rc = view_enter(b, env_ids, n, kind == DM_PTR_HOST, who))) return rc;
  Stage st(b, kind, who);
  const int i_q = st.in(qpos, (size_t)n * NQ * sizeof(double)), i_id = st.in(env_ids, (size_t)n * sizeof(int32_t)), i_o = st.out(out, (size_t)n * sizeof(int32_t));
  if ((rc = st.commit())) return rc;
  hipLaunchKernelGGL(k_floor_contacts, dim3(n), dim3(64), 0, b->stream, b->d_model, (const Real*)b->B.qpos, st.ptr<const double>(i_q),
                     st.ptr<const int>(i_id), st.ptr<int>(i_o));
  HIPCHK(hipGetLastError());
  return st.finish();
}

// ------------------------------------------------------------------ the imitation reward's five terms (terms_kernel.h)
extern "C" int dm_batch_imitation_terms(dm_batch* b, const double* qpos, const double* qvel, const int32_t* frame, const int32_t* cycle,
                                        const int32_t* env_ids, int32_t n, double* out, int32_t kind) {
  const char* who = "dm_batch_imitation_terms";
  int rc;
  const bool explicit_state = qpos || qvel || frame || cycle;
  if ((rc = view_args(b, out != nullptr, kind, n, explicit_state, "a state", env_ids, who))) return rc;
  if (explicit_state && !(qpos && qvel && frame)) return fail(DM_EINVAL, "dm_batch_imitation_terms: an explicit state needs qpos, qvel and frame");
  if (!b->B.imit_table) return fail(DM_EINVAL, "dm_batch_imitation_terms: the mocap has no imitation table (dm_mocap_set_imitation)");
  if (!explicit_state && b->B.reward_mode != REW_IMITATION) return fail(DM_EINVAL, "dm_batch_imitation_terms: the batch's own cursors name the compared row in reward mode 3 only");
  if (explicit_state && multi_clip(b) && n > b->n) return fail(DM_EINVAL, "dm_batch_imitation_terms: on a multi-clip batch state i is compared with the clip of env i: n exceeds the batch size");
  if (explicit_state && kind == DM_PTR_HOST && !multi_clip(b))
    for (int i = 0; i < n; i++) if (frame[i] < 0 || frame[i] >= b->B.n_frames) return fail(DM_EINVAL, "dm_batch_imitation_terms: frame out of range");
  if ((rc = view_enter(b, env_ids, n, kind == DM_PTR_HOST, who))) return rc;
  if (explicit_state && kind == DM_PTR_HOST && multi_clip(b)) {      // frame i is local to the clip of env i
    std::vector<int> ids;
    if ((rc = clip_ids_host(b, ids))) return rc;
    for (int i = 0; i < n; i++) if (frame[i] < 0 || frame[i] >= b->clip_frames[ids[i]]) return fail(DM_EINVAL, "dm_batch_imitation_terms: frame outside the env's clip");
  }
  Stage st(b, kind, who);
  const int i_q = st.in(qpos, (size_t)n * NQ * sizeof(double)), i_v = st.in(qvel, (size_t)n * NV * sizeof(double)), i_f = st.in(frame, (size_t)n * sizeof(int32_t));
  const int i_c = st.in(cycle, (size_t)n * sizeof(int32_t)), i_id = st.in(env_ids, (size_t)n * sizeof(int32_t)), i_o = st.out(out, (size_t)n * DM_NTERMS * sizeof(double));
  if ((rc = st.commit())) return rc;
  launch_clip_or_plain(b, k_imitation_terms, k_imitation_terms_clips, dim3(n), dim3(64), b->stream, b->d_model, b->B, st.ptr<const double>(i_q), st.ptr<const double>(i_v),
                       st.ptr<const int>(i_f), st.ptr<const int>(i_c), st.ptr<const int>(i_id), st.ptr<Ext>(i_o));
  HIPCHK(hipGetLastError());
  return st.finish();
}
