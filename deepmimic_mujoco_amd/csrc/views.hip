// views.hip — read-only views of a batch's environments: images (dm_batch_render), DeepMimic's state features (dm_batch_state_features) and the
// floor-contact query (dm_batch_floor_contacts), DESIGN.md section 9.  Host side only: the kernels (render_kernel.h, state_kernel.h, term_kernel.h)
// are compiled in dmenv.hip's unit, which see.
#define DM_NO_LAUNCH_KERNELS
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "render.h"

using namespace dm;

__global__ void k_render_pose(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos, const double* __restrict__ qpos_ext,
                              const int* __restrict__ env_ids, dmr::Camera cam, dmr::ViewRec* __restrict__ rec, double* __restrict__ geom_xform);
__global__ void k_render_rays(const dmr::ViewRec* __restrict__ rec, dmr::Params P, int tiles_x, int view0, unsigned char* __restrict__ rgb,
                              float* __restrict__ depth, int* __restrict__ seg);
__global__ void k_state_features(const DevModel<Real>* __restrict__ Mp, Batch<Real> B, const double* __restrict__ qpos_ext,
                                 const double* __restrict__ qvel_ext, const double* __restrict__ phase_ext, const int* __restrict__ env_ids,
                                 Ext* __restrict__ out);
__global__ void k_floor_contacts(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos, const double* __restrict__ qpos_ext,
                                 const int* __restrict__ env_ids, int* __restrict__ out);

// env ids given by host or device pointer are checked on the host (device ids are read back first)
static int check_env_ids(dm_batch* b, const int32_t* env_ids, int n, bool host, const char* who) {
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

// ------------------------------------------------------------------ rendering (render_kernel.h)
extern "C" int dm_batch_render(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, const dm_render_desc* d, uint8_t* rgb,
                               float* depth, int32_t* seg, double* geom_xform, int32_t kind) {
  if (!b || !d) return fail(DM_EINVAL, "dm_batch_render: null argument");
  if (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE) return fail(DM_EINVAL, "dm_batch_render: bad ptr_kind");
  if (n <= 0) return fail(DM_EINVAL, "dm_batch_render: n must be positive");
  if (qpos && env_ids) return fail(DM_EINVAL, "dm_batch_render: env_ids must be NULL when qpos is given");
  if (!qpos && n > b->n) return fail(DM_EINVAL, "dm_batch_render: n exceeds the batch size");
  const int W = d->width, H = d->height;
  if (W < 1 || W > 4096 || H < 1 || H > 4096) return fail(DM_EINVAL, "dm_batch_render: width and height must be 1..4096");
  const size_t npix = (size_t)n * W * H;
  if (npix >= (size_t)1 << 31) return fail(DM_EINVAL, "dm_batch_render: n * width * height must stay below 2^31");
  if (!(d->fovy > 0 && d->fovy < 180)) return fail(DM_EINVAL, "dm_batch_render: fovy must lie in (0, 180) degrees");
  if (!rgb && !depth && !seg && !geom_xform) return fail(DM_EINVAL, "dm_batch_render: no output requested");
  const double ln = std::sqrt(d->light_dir[0] * d->light_dir[0] + d->light_dir[1] * d->light_dir[1] + d->light_dir[2] * d->light_dir[2]);
  if (!(ln > 0)) return fail(DM_EINVAL, "dm_batch_render: light_dir must be nonzero");
  if (!(d->floor_square > 0)) return fail(DM_EINVAL, "dm_batch_render: floor_square must be positive");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const bool host = kind == DM_PTR_HOST;
  // scratch: records | qpos | env ids | (host outputs) rgb | depth | seg | xform
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
  const size_t o_rec = take((size_t)n * sizeof(dmr::ViewRec));
  const size_t o_q = host && qpos ? take((size_t)n * NQ * sizeof(double)) : 0;
  const size_t o_id = host && env_ids ? take((size_t)n * sizeof(int32_t)) : 0;
  const size_t o_rgb = host && rgb ? take(npix * 3) : 0;
  const size_t o_dep = host && depth ? take(npix * sizeof(float)) : 0;
  const size_t o_seg = host && seg ? take(npix * sizeof(int32_t)) : 0;
  const size_t o_xf = host && geom_xform ? take((size_t)n * NG * 12 * sizeof(double)) : 0;
  int rc;
  if ((rc = grow_rbuf(b, off, "dm_batch_render"))) return rc;
  unsigned char* base = b->d_rbuf;
  if ((rc = check_env_ids(b, env_ids, n, host, "dm_batch_render"))) return rc;
  const double* q = qpos;
  const int32_t* ids = env_ids;
  if (host && qpos) { HIPCHK(hipMemcpyAsync(base + o_q, qpos, (size_t)n * NQ * sizeof(double), hipMemcpyHostToDevice, b->stream)); q = (const double*)(base + o_q); }
  if (host && env_ids) { HIPCHK(hipMemcpyAsync(base + o_id, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream)); ids = (const int32_t*)(base + o_id); }
  unsigned char* drgb = host && rgb ? base + o_rgb : rgb;
  float* ddep = host && depth ? (float*)(base + o_dep) : depth;
  int32_t* dseg = host && seg ? (int32_t*)(base + o_seg) : seg;
  double* dxf = host && geom_xform ? (double*)(base + o_xf) : geom_xform;
  dmr::ViewRec* rec = (dmr::ViewRec*)(base + o_rec);
  dmr::Camera cam{};
  for (int k = 0; k < 3; k++) cam.pos[k] = d->cam_pos[k];
  for (int k = 0; k < 9; k++) cam.mat[k] = d->cam_mat[k];
  cam.track_com = d->track_com != 0;
  hipLaunchKernelGGL(k_render_pose, dim3(n), dim3(64), 0, b->stream, b->d_model, (const Real*)b->B.qpos, q, (const int*)ids, cam, rec, dxf);
  HIPCHK(hipGetLastError());
  if (drgb || ddep || dseg) {
    const dmr::Params P = dmr::make_params(*d);
    const int tiles_x = (W + 15) / 16, tiles = tiles_x * ((H + 15) / 16);
    for (int v0 = 0; v0 < n; v0 += 65535) {
      const int nv = n - v0 < 65535 ? n - v0 : 65535;
      hipLaunchKernelGGL(k_render_rays, dim3(tiles, nv), dim3(256), 0, b->stream, (const dmr::ViewRec*)rec, P, tiles_x, v0, drgb, ddep, (int*)dseg);
      HIPCHK(hipGetLastError());
    }
  }
  if (host) {
    if (rgb) HIPCHK(hipMemcpyAsync(rgb, drgb, npix * 3, hipMemcpyDeviceToHost, b->stream));
    if (depth) HIPCHK(hipMemcpyAsync(depth, ddep, npix * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (seg) HIPCHK(hipMemcpyAsync(seg, dseg, npix * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    if (geom_xform) HIPCHK(hipMemcpyAsync(geom_xform, dxf, (size_t)n * NG * 12 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return DM_OK;
}

// ------------------------------------------------------------------ DeepMimic's state features (state_kernel.h)
extern "C" int dm_batch_state_features(dm_batch* b, const double* qpos, const double* qvel, const double* phase, const int32_t* env_ids, int32_t n,
                                       double* out, int32_t kind) {
  if (!b || !out) return fail(DM_EINVAL, "dm_batch_state_features: null argument");
  if (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE) return fail(DM_EINVAL, "dm_batch_state_features: bad ptr_kind");
  if (n <= 0) return fail(DM_EINVAL, "dm_batch_state_features: n must be positive");
  if ((qpos || qvel || phase) && !(qpos && qvel && phase)) return fail(DM_EINVAL, "dm_batch_state_features: an explicit state needs qpos, qvel and phase");
  if (qpos && env_ids) return fail(DM_EINVAL, "dm_batch_state_features: env_ids must be NULL when a state is given");
  if (!qpos && n > b->n) return fail(DM_EINVAL, "dm_batch_state_features: n exceeds the batch size");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const bool host = kind == DM_PTR_HOST;
  int rc;
  if ((rc = check_env_ids(b, env_ids, n, host, "dm_batch_state_features"))) return rc;
  const double *q = qpos, *qv = qvel, *ph = phase;
  const int32_t* ids = env_ids;
  double* o = out;
  if (host) {      // staging: qpos | qvel | phase | env ids | out
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
    const size_t o_q = qpos ? take((size_t)n * NQ * sizeof(double)) : 0, o_v = qpos ? take((size_t)n * NV * sizeof(double)) : 0;
    const size_t o_p = qpos ? take((size_t)n * sizeof(double)) : 0, o_id = env_ids ? take((size_t)n * sizeof(int32_t)) : 0;
    const size_t o_out = take((size_t)n * DM_NSTATE * sizeof(double));
    if ((rc = grow_rbuf(b, off, "dm_batch_state_features"))) return rc;
    unsigned char* base = b->d_rbuf;
    if (qpos) {
      HIPCHK(hipMemcpyAsync(base + o_q, qpos, (size_t)n * NQ * sizeof(double), hipMemcpyHostToDevice, b->stream)); q = (const double*)(base + o_q);
      HIPCHK(hipMemcpyAsync(base + o_v, qvel, (size_t)n * NV * sizeof(double), hipMemcpyHostToDevice, b->stream)); qv = (const double*)(base + o_v);
      HIPCHK(hipMemcpyAsync(base + o_p, phase, (size_t)n * sizeof(double), hipMemcpyHostToDevice, b->stream)); ph = (const double*)(base + o_p);
    }
    if (env_ids) { HIPCHK(hipMemcpyAsync(base + o_id, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream)); ids = (const int32_t*)(base + o_id); }
    o = (double*)(base + o_out);
  }
  hipLaunchKernelGGL(k_state_features, dim3(n), dim3(64), 0, b->stream, b->d_model, b->B, q, qv, ph, (const int*)ids, (Ext*)o);
  HIPCHK(hipGetLastError());
  if (host) {
    HIPCHK(hipMemcpyAsync(out, o, (size_t)n * DM_NSTATE * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return DM_OK;
}

// ------------------------------------------------------------------ which geoms touch the floor (term_kernel.h)
extern "C" int dm_batch_floor_contacts(dm_batch* b, const double* qpos, const int32_t* env_ids, int32_t n, int32_t* out, int32_t kind) {
  if (!b || !out) return fail(DM_EINVAL, "dm_batch_floor_contacts: null argument");
  if (kind != DM_PTR_HOST && kind != DM_PTR_DEVICE) return fail(DM_EINVAL, "dm_batch_floor_contacts: bad ptr_kind");
  if (n <= 0) return fail(DM_EINVAL, "dm_batch_floor_contacts: n must be positive");
  if (qpos && env_ids) return fail(DM_EINVAL, "dm_batch_floor_contacts: env_ids must be NULL when qpos is given");
  if (!qpos && n > b->n) return fail(DM_EINVAL, "dm_batch_floor_contacts: n exceeds the batch size");
  HIPCHK(hipSetDevice(b->device));
  if (settle(b)) return fail(DM_EHIP, "pipeline join failed");
  const bool host = kind == DM_PTR_HOST;
  int rc;
  if ((rc = check_env_ids(b, env_ids, n, host, "dm_batch_floor_contacts"))) return rc;
  const double* q = qpos;
  const int32_t* ids = env_ids;
  int32_t* o = out;
  if (host) {      // staging: qpos | env ids | out
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
    const size_t o_q = qpos ? take((size_t)n * NQ * sizeof(double)) : 0, o_id = env_ids ? take((size_t)n * sizeof(int32_t)) : 0;
    const size_t o_out = take((size_t)n * sizeof(int32_t));
    if ((rc = grow_rbuf(b, off, "dm_batch_floor_contacts"))) return rc;
    unsigned char* base = b->d_rbuf;
    if (qpos) { HIPCHK(hipMemcpyAsync(base + o_q, qpos, (size_t)n * NQ * sizeof(double), hipMemcpyHostToDevice, b->stream)); q = (const double*)(base + o_q); }
    if (env_ids) { HIPCHK(hipMemcpyAsync(base + o_id, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, b->stream)); ids = (const int32_t*)(base + o_id); }
    o = (int32_t*)(base + o_out);
  }
  hipLaunchKernelGGL(k_floor_contacts, dim3(n), dim3(64), 0, b->stream, b->d_model, (const Real*)b->B.qpos, q, (const int*)ids, (int*)o);
  HIPCHK(hipGetLastError());
  if (host) {
    HIPCHK(hipMemcpyAsync(out, o, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  return DM_OK;
}
