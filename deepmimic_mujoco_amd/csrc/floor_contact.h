// floor_contact.h — "does geom g touch the floor at this state": the decision of dm_batch_floor_contacts and of the fall test of early
// termination (DM_OPT_FALL_BODIES; term_kernel.h).
//
// Geom g (1..15) touches the floor exactly when the step kernels' narrow phase (env_kernel.h narrowphase_at) would emit at least one contact
// for the pair (floor geom 0, g) at that state: the tests below are that routine's own hit conditions for a plane against a sphere, a capsule
// and a box, in its order of operations, without the contact records it goes on to fill.  The pair margin is max(margin_0, margin_g).
//
// Plain functions on plain arrays, templated on the real type, with no HIP dependency and no wave intrinsics (like state_features.h):
// term_kernel.h calls them from its kernels, one lane per geom, and the CPU tests build the same file with a host compiler
// (tests/floor_host.cpp).  That host build is test infrastructure; libdmenv.so has no CPU path.
#pragma once

#if defined(__HIPCC__)
#define FC_FN __host__ __device__ __forceinline__
#else
#define FC_FN inline
#endif

namespace dmfc {

enum { PLANE = 0, SPHERE = 2, CAPSULE = 3, BOX = 6 };       // mjtGeom values (env_kernel.h GEOM_*)

template <class R> FC_FN R dot(const R* a, const R* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// world frame (p [3], m [9] row-major) of a geom from its body's, as the collision stage forms it: p = xpos_b + xmat_b geom_pos, m = xmat_b geom_mat
template <class R>
FC_FN void geom_frame(const R* xpos, const R* xmat, const R* gpos, const R* gmat, R* p, R* m) {
  const R x = xmat[0] * gpos[0] + xmat[1] * gpos[1] + xmat[2] * gpos[2], y = xmat[3] * gpos[0] + xmat[4] * gpos[1] + xmat[5] * gpos[2],
          z = xmat[6] * gpos[0] + xmat[7] * gpos[1] + xmat[8] * gpos[2];
  p[0] = xpos[0] + x; p[1] = xpos[1] + y; p[2] = xpos[2] + z;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) m[3 * i + j] = xmat[3 * i] * gmat[j] + xmat[3 * i + 1] * gmat[3 + j] + xmat[3 * i + 2] * gmat[6 + j];
}

// plane through p0 with unit normal n against the sphere (c, r): plane_sphere's hit condition
template <class R>
FC_FN bool sphere_touches(const R* p0, const R* n, const R* c, R r, R margin) {
  const R t[3] = {c[0] - p0[0], c[1] - p0[1], c[2] - p0[2]};
  return !(dot(t, n) > margin + r);
}

// the floor's frame (p0, m0: its normal is m0's third column) against a geom of `type` at (p, m) with `size`
template <class R>
FC_FN bool touches_floor(const R* p0, const R* m0, int type, const R* p, const R* m, const R* size, R margin) {
  const R n[3] = {m0[2], m0[5], m0[8]};
  if (type == SPHERE) return sphere_touches(p0, n, p, size[0], margin);
  if (type == CAPSULE) {                       // either end's sphere: p +- axis * half
    const R ax[3] = {m[2], m[5], m[8]};
    R c[3] = {p[0] + ax[0] * size[1], p[1] + ax[1] * size[1], p[2] + ax[2] * size[1]};
    const bool ha = sphere_touches(p0, n, c, size[0], margin);
    c[0] = p[0] - ax[0] * size[1]; c[1] = p[1] - ax[1] * size[1]; c[2] = p[2] - ax[2] * size[1];
    const bool hb = sphere_touches(p0, n, c, size[0], margin);
    return ha || hb;
  }
  if (type == BOX) {                           // some corner below the box's centre plane and within the margin of the floor
    const R dif[3] = {p[0] - p0[0], p[1] - p0[1], p[2] - p0[2]};
    const R dist = dot(dif, n);
    bool hit = false;
    for (int i = 0; i < 8; i++) {
      const R v[3] = {(i & 1) ? size[0] : -size[0], (i & 2) ? size[1] : -size[1], (i & 4) ? size[2] : -size[2]};
      const R corner[3] = {m[0] * v[0] + m[1] * v[1] + m[2] * v[2], m[3] * v[0] + m[4] * v[1] + m[5] * v[2], m[6] * v[0] + m[7] * v[1] + m[8] * v[2]};
      const R ld = dot(n, corner);
      if (dist + ld > margin || ld > 0) continue;
      hit = true;
    }
    return hit;
  }
  return false;
}

// geom g of a model given by its tables (geom_body [ng], geom_type [ng], geom_pos [ng][3], geom_mat [ng][9], geom_size [ng][3], geom_margin [ng])
// at the body frames xpos [nb][3], xmat [nb][9]; geom 0 is the floor
template <class R>
FC_FN bool geom_touches_floor(int g, const int* geom_body, const int* geom_type, const R (*geom_pos)[3], const R (*geom_mat)[9], const R (*geom_size)[3],
                              const R* geom_margin, const R (*xpos)[3], const R (*xmat)[9]) {
  R p0[3], m0[9], p[3], m[9];
  geom_frame(xpos[geom_body[0]], xmat[geom_body[0]], geom_pos[0], geom_mat[0], p0, m0);
  geom_frame(xpos[geom_body[g]], xmat[geom_body[g]], geom_pos[g], geom_mat[g], p, m);
  const R margin = geom_margin[0] > geom_margin[g] ? geom_margin[0] : geom_margin[g];
  return touches_floor(p0, m0, geom_type[g], p, m, geom_size[g], margin);
}

// bit g of the result: a body of the mask `bodies` (bit b = model body b) owns geom g
FC_FN unsigned geoms_of_bodies(unsigned bodies, const int* geom_body, int ng) {
  unsigned out = 0;
  for (int g = 1; g < ng; g++) if ((bodies >> geom_body[g]) & 1u) out |= 1u << g;
  return out;
}

}  // namespace dmfc
