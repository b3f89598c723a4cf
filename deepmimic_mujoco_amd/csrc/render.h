// render.h — the per-pixel math of dm_batch_render: camera rays, ray / geom intersections, shading.
//
// Plain functions with no HIP dependency: render_kernel.h calls them from the ray-casting kernel (hipcc, gfx950), and the
// CPU tests build the same file with a host compiler (tests/render_host.cpp) to check this math against the float64
// restatement without a GPU.  That host build is test infrastructure; libdmenv.so has no CPU path.
//
// All ray math is float32 in CAMERA-RELATIVE coordinates (origin at the camera): an 8-bit image does not need float64, and
// subtracting the camera position once, in the caller's precision, keeps the geometry exact when the humanoid is far from
// the world origin.
#pragma once

#include <cmath>

#include "dmenv.h"

#if defined(__HIPCC__)
#define RD_FN __host__ __device__ __forceinline__
#else
#define RD_FN inline
#endif

namespace dmr {

constexpr int NG = 16;                           // geoms of the model: 0 = the floor plane, 1..15 body geoms
enum { RG_PLANE = 0, RG_SPHERE = 2, RG_CAPSULE = 3, RG_BOX = 6 };
constexpr float SHADOW_OFFSET = 1e-4f;           // metres along the normal from which a shadow ray starts
constexpr float INF = __builtin_huge_valf();

// constants of one call (a kernel argument: wave-uniform)
struct Params {
  int width, height;
  float tan_half_fovy, aspect;                   // tan(fovy / 2), width / height
  float geom_rgb[NG][3];                         // albedo of the body geoms (entry 0 unused: the floor is the checker)
  float floor_rgb1[3], floor_rgb2[3], floor_inv_square;   // checker: rgb1 where floor(x / square) + floor(y / square) is even
  float sky_top[3], sky_bottom[3];               // gradient skybox: c = bottom + (1 + d_z) / 2 (top - bottom)
  float light[3];                                // unit direction the directional light travels in
  float ambient, headlight, diffuse;
};

// the camera of one call, as dm_render_desc gives it (float64 on the host side of every build; a kernel argument of the pose pass)
struct Camera {
  double pos[3];      // world position, or the offset from the centre of mass when track_com
  double mat[9];      // row-major; columns = camera x (right), y (up), z (backward)
  int track_com;
};

// one body geom as the ray caster sees it: centre relative to the camera, world axes (row-major: column k = local axis k)
struct GeomRec {
  float c[3];
  int type;
  float size[3];
  float m[9];
};

// one view: about 1 KB, written by the pose pass, read once per workgroup with wave-uniform loads
struct ViewRec {
  float x[3], y[3], z[3];                        // camera axes in the world (it looks along -z)
  float cam[3];                                  // camera position in the world
  float bs[3], bs_r2;                            // bounding sphere of the body geoms (centre relative to the camera, radius squared)
  float floor_half[2];                           // the floor is finite: |x| <= floor_half[0], |y| <= floor_half[1]
  float pad[2];
  GeomRec g[NG - 1];                             // geoms 1..15
};

RD_FN float dot3f(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
RD_FN float minf(float a, float b) { return a < b ? a : b; }
RD_FN float maxf(float a, float b) { return a > b ? a : b; }
RD_FN float sgn_mag(float mag, float s) { return s < 0.f ? -mag : mag; }
RD_FN void normalize3f(float* v) { const float k = 1.f / sqrtf(dot3f(v, v)); v[0] *= k; v[1] *= k; v[2] *= k; }

// ---- the call's constants and a view's record (host side of dm_batch_render, the pose pass, the tests' host driver) ----------
// (the descriptor was validated: fovy in (0, 180), light_dir nonzero, floor_square > 0)
inline Params make_params(const dm_render_desc& d) {
  Params P{};
  P.width = d.width; P.height = d.height;
  P.tan_half_fovy = (float)std::tan(d.fovy * 3.14159265358979323846 / 360.0); P.aspect = (float)((double)d.width / d.height);
  for (int g = 0; g < NG; g++) for (int k = 0; k < 3; k++) P.geom_rgb[g][k] = (float)d.geom_rgb[g][k];
  const double ln = std::sqrt(d.light_dir[0] * d.light_dir[0] + d.light_dir[1] * d.light_dir[1] + d.light_dir[2] * d.light_dir[2]);
  for (int k = 0; k < 3; k++) {
    P.floor_rgb1[k] = (float)d.floor_rgb1[k]; P.floor_rgb2[k] = (float)d.floor_rgb2[k];
    P.sky_top[k] = (float)d.sky_top[k]; P.sky_bottom[k] = (float)d.sky_bottom[k]; P.light[k] = (float)(d.light_dir[k] / ln);
  }
  P.floor_inv_square = (float)(1.0 / d.floor_square);
  P.ambient = (float)d.ambient; P.headlight = (float)d.headlight; P.diffuse = (float)d.diffuse;
  return P;
}
// the camera part of a record: axes = the columns of the row-major cam_mat, position in the world, the floor's half sizes
template <class R>
RD_FN void set_camera(ViewRec& v, const double* cam_mat, const R* cam, const R* floor_size) {
  for (int k = 0; k < 3; k++) { v.x[k] = (float)cam_mat[3 * k]; v.y[k] = (float)cam_mat[3 * k + 1]; v.z[k] = (float)cam_mat[3 * k + 2]; v.cam[k] = (float)cam[k]; }
  v.floor_half[0] = (float)floor_size[0]; v.floor_half[1] = (float)floor_size[1];
  v.pad[0] = v.pad[1] = 0.f;
}
// geom frame in the world (pos, row-major mat, both of the caller's precision R) -> camera-relative float32 record
template <class R>
RD_FN void fill_geom(GeomRec& g, int type, const R* pos, const R* mat, const R* size, const R* cam) {
  for (int k = 0; k < 3; k++) g.c[k] = (float)(pos[k] - cam[k]);
  for (int k = 0; k < 9; k++) g.m[k] = (float)mat[k];
  for (int k = 0; k < 3; k++) g.size[k] = (float)size[k];
  g.type = type;
}
// radius of a sphere about the geom's centre that holds it
RD_FN float geom_extent(const GeomRec& g) {
  if (g.type == RG_SPHERE) return g.size[0];
  if (g.type == RG_CAPSULE) return g.size[0] + g.size[1];
  return sqrtf(g.size[0] * g.size[0] + g.size[1] * g.size[1] + g.size[2] * g.size[2]);
}
// bounding sphere of the body geoms about `centre` (camera-relative), widened so that float32 rounding never culls a hit
RD_FN void finish_bound(ViewRec& v, const float* centre) {
  float r = 0.f;
  for (int i = 0; i < NG - 1; i++) {
    const float d[3] = {v.g[i].c[0] - centre[0], v.g[i].c[1] - centre[1], v.g[i].c[2] - centre[2]};
    r = maxf(r, sqrtf(dot3f(d, d)) + geom_extent(v.g[i]));
  }
  r = r * 1.001f + 1e-3f;
  for (int k = 0; k < 3; k++) v.bs[k] = centre[k];
  v.bs_r2 = r * r;
}

// ---- intersections: nearest t > 0 at which the ray o + t d (|d| = 1) meets the surface, INF if none -------------------------
// roots of t^2 + 2 b t + cc = 0 given disc = b^2 - cc computed stably; the smaller positive one
RD_FN float first_root(float b, float cc, float disc) {
  const float q = -b - sgn_mag(sqrtf(disc), b);   // |q| = |b| + sqrt(disc): no cancellation
  const float t0 = q, t1 = cc / q;
  const float lo = minf(t0, t1), hi = maxf(t0, t1);
  return lo > 0.f ? lo : (hi > 0.f ? hi : INF);
}
RD_FN float hit_sphere(const float* o, const float* d, const float* c, float r) {
  const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
  const float b = dot3f(oc, d);
  const float h[3] = {oc[0] - b * d[0], oc[1] - b * d[1], oc[2] - b * d[2]};   // closest approach: disc = r^2 - |h|^2
  const float disc = r * r - dot3f(h, h);
  if (!(disc >= 0.f)) return INF;
  return first_root(b, dot3f(oc, oc) - r * r, disc);
}
// capsule: the segment c +- hl a (a = the geom's z axis) widened by r.  Its surface is the cylinder wall where the axial
// coordinate lies in [-hl, hl] plus the two outer hemispheres; the first crossing of any of them is the hit.
RD_FN float hit_capsule(const float* o, const float* d, const GeomRec& g) {
  const float a[3] = {g.m[2], g.m[5], g.m[8]};
  const float r = g.size[0], hl = g.size[1];
  const float oc[3] = {o[0] - g.c[0], o[1] - g.c[1], o[2] - g.c[2]};
  const float da = dot3f(d, a), oa = dot3f(oc, a);
  float best = INF;
  const float dp[3] = {d[0] - da * a[0], d[1] - da * a[1], d[2] - da * a[2]};
  const float op[3] = {oc[0] - oa * a[0], oc[1] - oa * a[1], oc[2] - oa * a[2]};
  const float A = dot3f(dp, dp);
  if (A > 1e-12f) {
    const float B = dot3f(dp, op), kB = B / A;
    const float h[3] = {op[0] - kB * dp[0], op[1] - kB * dp[1], op[2] - kB * dp[2]};
    const float disc = r * r - dot3f(h, h);
    if (disc >= 0.f) {
      const float q = -B - sgn_mag(sqrtf(A * disc), B);
      const float t0 = q / A, t1 = (dot3f(op, op) - r * r) / q;
      const float y0 = oa + t0 * da, y1 = oa + t1 * da;
      if (t0 > 0.f && y0 >= -hl && y0 <= hl) best = minf(best, t0);
      if (t1 > 0.f && y1 >= -hl && y1 <= hl) best = minf(best, t1);
    }
  }
  for (int s = -1; s <= 1; s += 2) {             // the caps: roots on the outer hemisphere of the end sphere at s hl
    const float e[3] = {oc[0] - s * hl * a[0], oc[1] - s * hl * a[1], oc[2] - s * hl * a[2]};
    const float b = dot3f(e, d);
    const float h[3] = {e[0] - b * d[0], e[1] - b * d[1], e[2] - b * d[2]};
    const float disc = r * r - dot3f(h, h);
    if (disc >= 0.f) {
      const float q = -b - sgn_mag(sqrtf(disc), b);
      const float t0 = q, t1 = (dot3f(e, e) - r * r) / q;
      if (t0 > 0.f && s * (oa + t0 * da) >= hl) best = minf(best, t0);
      if (t1 > 0.f && s * (oa + t1 * da) >= hl) best = minf(best, t1);
    }
  }
  return best;
}
// box: slab test in the box frame; *face = signed axis (+-(k + 1)) of the face hit, for the normal
RD_FN float hit_box(const float* o, const float* d, const GeomRec& g, int* face) {
  const float oc[3] = {o[0] - g.c[0], o[1] - g.c[1], o[2] - g.c[2]};
  float tn = -INF, tf = INF;
  int fn = 0, ff = 0;
  for (int k = 0; k < 3; k++) {
    const float ol = g.m[k] * oc[0] + g.m[3 + k] * oc[1] + g.m[6 + k] * oc[2];
    const float dl = g.m[k] * d[0] + g.m[3 + k] * d[1] + g.m[6 + k] * d[2];
    const float inv = 1.f / dl;
    const float t1 = (-g.size[k] - ol) * inv, t2 = (g.size[k] - ol) * inv;
    const float lo = minf(t1, t2), hi = maxf(t1, t2);
    const int s = dl < 0.f ? 1 : -1;             // outward normal of the entry face points against d
    if (lo > tn) { tn = lo; fn = s * (k + 1); }
    if (hi < tf) { tf = hi; ff = -s * (k + 1); }
  }
  if (!(tn <= tf) || !(tf > 0.f)) return INF;
  if (tn > 0.f) { *face = fn; return tn; }
  *face = ff;
  return tf;
}
// outward unit normal of geom g at the camera-relative point p
RD_FN void geom_normal(const GeomRec& g, const float* p, int face, float* n) {
  const float e[3] = {p[0] - g.c[0], p[1] - g.c[1], p[2] - g.c[2]};
  if (g.type == RG_BOX) {
    const int k = (face < 0 ? -face : face) - 1;
    const float s = face < 0 ? -1.f : 1.f;
    n[0] = s * g.m[k]; n[1] = s * g.m[3 + k]; n[2] = s * g.m[6 + k];
    return;
  }
  if (g.type == RG_CAPSULE) {
    const float a[3] = {g.m[2], g.m[5], g.m[8]};
    const float y = minf(maxf(dot3f(e, a), -g.size[1]), g.size[1]);
    n[0] = e[0] - y * a[0]; n[1] = e[1] - y * a[1]; n[2] = e[2] - y * a[2];
  } else {
    n[0] = e[0]; n[1] = e[1]; n[2] = e[2];
  }
  normalize3f(n);
}
RD_FN float hit_geom(const float* o, const float* d, const GeomRec& g, int* face) {
  if (g.type == RG_SPHERE) return hit_sphere(o, d, g.c, g.size[0]);
  if (g.type == RG_CAPSULE) return hit_capsule(o, d, g);
  return hit_box(o, d, g, face);
}
// does the ray possibly meet the body's bounding sphere?  (a cull: false only where no body geom can be hit)
RD_FN bool near_body(const ViewRec& v, const float* o, const float* d) {
  const float oc[3] = {o[0] - v.bs[0], o[1] - v.bs[1], o[2] - v.bs[2]};
  const float b = dot3f(oc, d), cc = dot3f(oc, oc);
  if (b > 0.f && cc > v.bs_r2) return false;     // outside and moving away
  const float h[3] = {oc[0] - b * d[0], oc[1] - b * d[1], oc[2] - b * d[2]};
  return dot3f(h, h) <= v.bs_r2;
}

// ---- one pixel ------------------------------------------------------------------------------------------------------------
struct Pixel {
  unsigned char rgb[3];
  float depth;                                   // along the optical axis; +inf where nothing is hit
  int seg;                                       // geom id, -1 where nothing is hit
  int shadow;                                    // 1: lit face, light blocked
};

RD_FN unsigned char to_byte(float c) {
  c = minf(maxf(c, 0.f), 1.f);
  return (unsigned char)floorf(255.f * c + 0.5f);
}

RD_FN Pixel shade_pixel(const ViewRec& v, const Params& P, int row, int col) {
  const float u = (2.f * ((float)col + 0.5f) / (float)P.width - 1.f) * P.tan_half_fovy * P.aspect;
  const float w = (1.f - 2.f * ((float)row + 0.5f) / (float)P.height) * P.tan_half_fovy;
  float d[3] = {u * v.x[0] + w * v.y[0] - v.z[0], u * v.x[1] + w * v.y[1] - v.z[1], u * v.x[2] + w * v.y[2] - v.z[2]};
  normalize3f(d);
  const float o[3] = {0.f, 0.f, 0.f};
  Pixel px;
  // the floor: z = 0 seen from above, finite
  float t = INF;
  int id = -1, face = 0;
  if (d[2] < 0.f && v.cam[2] > 0.f) {
    const float tf = -v.cam[2] / d[2];
    const float fx = v.cam[0] + tf * d[0], fy = v.cam[1] + tf * d[1];
    if (fabsf(fx) <= v.floor_half[0] && fabsf(fy) <= v.floor_half[1]) { t = tf; id = 0; }
  }
  if (near_body(v, o, d)) {
    for (int i = 0; i < NG - 1; i++) {
      int f = 0;
      const float tg = hit_geom(o, d, v.g[i], &f);
      if (tg < t) { t = tg; id = i + 1; face = f; }
    }
  }
  px.seg = id;
  px.shadow = 0;
  if (id < 0) {
    px.depth = INF;
    const float k = 0.5f * (1.f + d[2]);
    for (int c = 0; c < 3; c++) px.rgb[c] = to_byte(P.sky_bottom[c] + k * (P.sky_top[c] - P.sky_bottom[c]));
    return px;
  }
  px.depth = t * -dot3f(d, v.z);
  const float p[3] = {t * d[0], t * d[1], t * d[2]};
  float n[3] = {0.f, 0.f, 1.f};
  float alb[3];
  if (id == 0) {
    const float fx = v.cam[0] + p[0], fy = v.cam[1] + p[1];
    const int parity = ((int)floorf(fx * P.floor_inv_square) + (int)floorf(fy * P.floor_inv_square)) & 1;
    for (int c = 0; c < 3; c++) alb[c] = parity ? P.floor_rgb2[c] : P.floor_rgb1[c];
  } else {
    geom_normal(v.g[id - 1], p, face, n);
    for (int c = 0; c < 3; c++) alb[c] = P.geom_rgb[id][c];
  }
  const float lit = -dot3f(n, P.light);
  float vis = 0.f;
  if (lit > 0.f) {                               // a shadow ray towards the light; only body geoms cast shadows
    const float so[3] = {p[0] + SHADOW_OFFSET * n[0], p[1] + SHADOW_OFFSET * n[1], p[2] + SHADOW_OFFSET * n[2]};
    const float sd[3] = {-P.light[0], -P.light[1], -P.light[2]};
    vis = 1.f;
    if (near_body(v, so, sd)) {
      for (int i = 0; i < NG - 1; i++) {
        int f = 0;
        if (hit_geom(so, sd, v.g[i], &f) < INF) { vis = 0.f; break; }
      }
    }
    px.shadow = vis == 0.f;
  }
  const float k = P.ambient + P.headlight * maxf(0.f, -dot3f(n, d)) + P.diffuse * vis * maxf(0.f, lit);
  for (int c = 0; c < 3; c++) px.rgb[c] = to_byte(alb[c] * k);
  return px;
}

}  // namespace dmr
