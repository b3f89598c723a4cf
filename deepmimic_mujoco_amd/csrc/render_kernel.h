// render_kernel.h — dm_batch_render's two launches.  Included by dmenv.hip after kernels.h; launched from views.hip.
//
//   k_render_pose  one wave per view: the step kernels' kinematics (stage_kinematics) at the view's qpos, the 16 geom frames
//                  formed as stage_rows forms them, the centre of mass, the resolved camera, and the view's ~1 KB record for
//                  the ray caster (camera-relative float32 geoms + a bounding sphere of the body).  Changes no batch state.
//   k_render_rays  one thread per pixel: a 256-thread workgroup holds a 16 x 16 tile of one view as four waves of 8 x 8 pixels
//                  (coherent rays per wave); grid = (tiles, views).  The view's record is read with wave-uniform loads.
#pragma once

#include "render.h"

// qpos of view v: an explicit pose (qpos_ext [n,35]) or the batch's state of env env_ids[v] (or v)
__global__ __launch_bounds__(64) void k_render_pose(const DevModel<Real>* __restrict__ Mp, const Real* __restrict__ state_qpos,
                                                    const double* __restrict__ qpos_ext, const int* __restrict__ env_ids, dmr::Camera cam,
                                                    dmr::ViewRec* __restrict__ rec, double* __restrict__ geom_xform) {
  __shared__ Shared<Real> s;
  __shared__ Real gframe[NG][12];
  __shared__ Real campos[3];
  __shared__ dmr::ViewRec vr;
  const int v = blockIdx.x, lane = dmw::lane();
  const DevModel<Real>& M = *Mp;
  if (lane < NQ) s.qpos[lane] = qpos_ext ? (Real)qpos_ext[(size_t)v * NQ + lane] : state_qpos[(size_t)(env_ids ? env_ids[v] : v) * NQ + lane];
  dmw::sync();
  stage_kinematics(M, s, lane, lane_topo(lane));
  // geom world frames, as stage_rows forms them: gpos = xpos_b + xmat_b geom_pos, gmat = xmat_b geom_mat
  if (lane < NG) {
    const int g = lane, gb = M.geom_body[g];
    Real w[3];
    mat_vec(w, s.xmat[gb], M.geom_pos[g]);
    for (int k = 0; k < 3; k++) gframe[g][k] = s.xpos[gb][k] + w[k];
    const Real* a = s.xmat[gb]; const Real* bm = M.geom_mat[g];
    for (int i = 0; i < 3; i++) for (int jx = 0; jx < 3; jx++) gframe[g][3 + 3 * i + jx] = a[3 * i] * bm[jx] + a[3 * i + 1] * bm[3 + jx] + a[3 * i + 2] * bm[6 + jx];
  }
  // the root's subtree centre of mass (bodies 1..13, a fixed order) and the camera: trackcom = that + the offset
  Real com[3] = {0, 0, 0};
  if (lane == 0) {
    Real m = 0;
    for (int b = 1; b < NB; b++) { for (int k = 0; k < 3; k++) com[k] += M.body_mass[b] * s.xipos[b][k]; m += M.body_mass[b]; }
    for (int k = 0; k < 3; k++) { com[k] /= m; campos[k] = (cam.track_com ? com[k] : Real(0)) + (Real)cam.pos[k]; }
  }
  dmw::sync();
  if (lane >= 1 && lane < NG) {
    const Real sz[3] = {M.geom_size[lane][0], M.geom_size[lane][1], M.geom_size[lane][2]};
    dmr::fill_geom(vr.g[lane - 1], M.geom_type[lane], &gframe[lane][0], &gframe[lane][3], sz, campos);
  }
  if (geom_xform) for (int k = lane; k < NG * 12; k += 64) geom_xform[(size_t)v * NG * 12 + k] = (double)(&gframe[0][0])[k];
  dmw::sync();
  if (lane == 0) {
    dmr::set_camera(vr, cam.mat, campos, M.geom_size[0]);
    const float centre[3] = {(float)(com[0] - campos[0]), (float)(com[1] - campos[1]), (float)(com[2] - campos[2])};   // (any centre is valid)
    dmr::finish_bound(vr, centre);
  }
  dmw::sync();
  static_assert(sizeof(dmr::ViewRec) % 4 == 0, "the record is copied out in words");
  for (int k = lane; k < (int)(sizeof(dmr::ViewRec) / 4); k += 64) ((unsigned*)&rec[v])[k] = ((const unsigned*)&vr)[k];
}

__global__ __launch_bounds__(256) void k_render_rays(const dmr::ViewRec* __restrict__ rec, dmr::Params P, int tiles_x, int view0,
                                                     unsigned char* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ seg) {
  const int v = view0 + (int)blockIdx.y;
  const int tile = (int)blockIdx.x, wv = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & 63u);
  const int row = (tile / tiles_x) * 16 + (wv >> 1) * 8 + (l >> 3);
  const int col = (tile % tiles_x) * 16 + (wv & 1) * 8 + (l & 7);
  if (row >= P.height || col >= P.width) return;
  const dmr::Pixel px = dmr::shade_pixel(rec[v], P, row, col);
  const size_t i = ((size_t)v * P.height + row) * P.width + col;
  if (rgb) { rgb[3 * i] = px.rgb[0]; rgb[3 * i + 1] = px.rgb[1]; rgb[3 * i + 2] = px.rgb[2]; }
  if (depth) depth[i] = px.depth;
  if (seg) seg[i] = px.seg;
}
