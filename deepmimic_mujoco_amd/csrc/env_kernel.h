// env_kernel.h — the batched DeepMimic humanoid step as wave64 device code (gfx950 / CDNA4).
//
// One wavefront simulates one environment.  All per-environment working data of a forward-dynamics
// evaluation lives in LDS (`Shared`, ~22 KB) or in registers; HBM is touched only to load the state row
// (qpos/qvel/qacc_warmstart/action) at the start of a step and to store it plus obs/reward/done at the end.
//
// What one step computes is MuJoCo 2.0's mj_step for dp_env_v3.xml (RK4, PGS, pyramidal cones), i.e. what
// `self.do_simulation(action, 1)` does at src/dp_env_v3.py:112, followed by the env epilogue of
// src/dp_env_v3.py:115-132 (obs, reward, done).  The algorithms are chosen for the wave, not translated:
//   * kinematics / RNE run level-by-level over the 4-deep body tree, one lane per body;
//   * the mass matrix is built as 310 independent tree-sparse entries (lanes over entries) and factorised
//     L^T D L in MuJoCo's sparse layout, one elimination column per step with lanes over the rank-1 update;
//   * every constraint row owns a lane: the lane regenerates its Jacobian row from a 6-D contact wrench,
//     half-solves it against the factor in registers (static indices, factor broadcast from LDS) and keeps
//     its row of A = J M^-1 J^T + R in 64 registers — the Gauss-Seidel sweep then needs one v_readlane
//     broadcast and one FMA per row and no memory at all;
//   * collision runs lanes over the 104 candidate geom pairs with deterministic prefix-sum compaction, so
//     the contact list (and hence the PGS row order) is bit-identical to a serial walk of the pair list.
// fp64 throughout (the reference computes in float64; parity bar 1e-5 relative, test bar 1e-9).
// The matrix core is used in one place: A = Y Y^T of an evaluation with at most 16 rows (a_block16: nine v_mfma_f64_16x16x4
// blocks).  On gfx950 v_mfma_f64 runs at the f64 VALU rate (78.6 TF both), so a block only pays where its padding is cheaper than
// the vector unit's idle lanes; the same treatment of the Jacobian rows was measured and is exactly as fast as the vector loop.
#pragma once

#include <type_traits>

#include "topology.h"
#include "wave.h"

// assembly-listing marker (a comment in the .s output, no instruction): tools/isa_stage_count.py splits the listing on these
#if defined(DM_WAVE_TESTBENCH)
#define DM_MARK(name) ((void)0)
#else
#define DM_MARK(name) asm volatile("; DM_MARK " name)
#endif

namespace dm {

using namespace dmt;

DM_CONSTANT Topo TOPO = make_topo();

#define DM_MINVAL 1e-15

enum { GEOM_PLANE = 0, GEOM_SPHERE = 2, GEOM_CAPSULE = 3, GEOM_BOX = 6 };
enum { REW_ALIVE = 0, REW_V3_CONFIG = 1, REW_V2_POSE = 2, REW_IMITATION = 3, REW_V1_QUAT = 4 };
constexpr int KIN_A = NB * 3 + NB * 9 + NB * 3 + NV * 6, KIN_B = 2 * NB * 10, KIN_DOUBLES = KIN_A + KIN_B;   // see env_step.h save_kin
constexpr int PROF_SLOTS = 32;  // per-env profile record (k_step_prof): see dm_batch_read_profile
constexpr int IMIT_FEAT = 112;   // doubles per reference feature row (deepmimic_mujoco_amd/imitation.py)
enum { ROW_NONE = 0, ROW_LIMIT = 1, ROW_CONTACT = 2 };

// ---------------------------------------------------------------------------------------------------------
// everything the collision stage needs to know about one candidate geom pair, in one 96-byte record: lane L always handles
// pairs L and 64 + L, so its record is fetched with one burst of loads at the top of the stage instead of a chain of
// dependent per-geom table look-ups (pair -> geom -> type / size / margin / body -> inverse weight: 4 global-load latencies).
template <class R>
struct alignas(16) PairRec {
  int g1, g2;          // geom ids (geom1 = lower geom type)
  int t1t2;            // type1 | type2 << 8 | condim << 16
  int meta;            // body1 | body2 << 8 | (staging slot + 1) << 16
  R margin, mu, bound, tran;   // max margin, max friction, broad-phase bound (incl. margin), invweight(body1) + invweight(body2)
  R s1[3], s2[3];      // geom sizes
};

// device-resident constant model (one copy in HBM, L2-resident; uniform reads become scalar loads)
template <class R>
struct DevModel {
  R body_pos[NB][3], body_ipos[NB][3], body_mass[NB], body_inertia[NB][6], body_invw[NB];
  R jnt_axis[NJ][3], jnt_lo[NJ], jnt_hi[NJ];
  int jnt_limited[NJ];
  R dof_armature[NV], dof_damping[NV], dof_invw[NV];
  R gear[NV], ctrl_lo[NV], ctrl_hi[NV];  // per dof (0 for the free joint)
  R kp[NV], kd[NV];                      // PD gains per dof (PARAMS_KP_KD, src/mujoco/mocap_util.py:22-24), action mode 2
  int geom_type[NG], geom_body[NG], geom_condim[NG], geom_boxslot[NG];   // boxslot: index among box geoms (< 4) or -1
  R geom_pos[NG][3], geom_mat[NG][9], geom_size[NG][3], geom_margin[NG], geom_mu[NG], geom_rbound[NG];
  int npair;
  short pair_g1[MAXPAIR], pair_g2[MAXPAIR];
  short pair_stage[MAXPAIR];   // LDS staging slot of a pair that can yield > 2 contacts (plane-box 0..3, box-box 4..5), else -1
  PairRec<R> pair_rec[MAXPAIR];
  R qpos0[NQ];
  R timestep, gravity[3], tolerance, solref[2], solimp[5], meaninertia, total_mass;
  R K, B, pgs_scale;  // constraint stiffness / damping (refsafe applied), 1/(meaninertia*nv)
  R imp_rlo, imp_rhi; // 1 / midpoint^(power-1), 1 / (1-midpoint)^(power-1) of solimp (impedance, power == 2 fast path)
  R pgs_detect;       // cost-increase level that sends a PGS sweep to the guarded replay (1e-10 = [MJ costChange]; tests lower it)
  int iterations, enable_contact, enable_limit;
};

// per-wave LDS working set.  Regions whose lifetimes do not overlap inside one forward evaluation share storage:
//   ua: body quaternions (kinematics only)            | smooth force / y_tau / qacc (bias .. constraint, RK driver)
//   ub: spatial inertias (kinematics .. bias)          | geom world poses (collision)
//   u : M-build scratch | RNE scratch | row descriptors (collision -> row registers) | broadcast / reduce buffers
template <class R>
struct Shared {
  R qpos[36], qvel[NV], act[NV], qws[NV];
  R xpos[NB][3], xmat[NB][9], xipos[NB][3];
  R cdof[NV][6];
  R qLD[312], dinv[NV], dsq[NV];
  union {
    R xquat[NB][4];
    struct { R tau[NV], qaccs[NV], qacc[NV]; } f;
  } ua;
  union {
    struct { R sin[NB][10], crb[NB][10]; } i;
    struct { R gpos[NG][3], gmat[NG][9], poly[2][8][3], axes[2][3][3]; } g;   // poly / axes: box-box scratch (dynamically indexed)
  } ub;
  union {
    R fdof[NV][6];
    struct { R cvel[NB][6], cacc[NB][6], cfrc[NB][6], csub[NB][6]; } v;
    R rowd[MAXEFC][10];  // w[6], dist, margin, dA, rscale
    R ybuf[17][NV];      // 16 broadcast slots + slot 16: z = D^-1/2 L^-T tau (lives from the half solve to the final assembly)
  } u;
  R boxc[6][4][4];     // contacts (dist, pos) of the pair types with > 2 contacts: plane-box (slots 0..3), box-box (4..5)
  int rowi[MAXEFC];    // type | b1<<8 | b2<<16   (limit: type | dof<<8)
  int cong[MAXEFC][2]; // contact geom ids
  int nefc, ncon, status, solver_iter;
  R* aovf;   // this env's memory strip for columns of A, [MAXEFC][64]: columns past the register tier; all of them during a PGS replay
  // static index tables staged from the compile-time topology once per kernel (LDS lookups instead of global loads)
  unsigned short tab_dst[NV][14];   // tab_dst[k][a] = madr[anc_a(k)]: first stored entry of the row of k's a-th ancestor
  unsigned short tab_ent[312];      // entry e of the sparse M -> (i << 8) | j
};

// per-lane topology constants, read once per kernel
struct LaneTopo {
  int parent, dofadr, dofnum, depth;
  unsigned subtree;
  unsigned long long tri;   // six byte codes (e << 4) | a of the lower-triangular pair numbers t = (lane & 15) + 16 j, j = 0..5:
                            // t = e (e - 1) / 2 + (a - 1),  1 <= a <= e   (byte j of the word)
};
// Everything a lane reads at kernel entry is a compile-time table: one independent load per field instead of chains of
// dependent topology look-ups and a search loop per lane in every launch.
constexpr unsigned tri_pair(int t) {
  int e = 1;
  while (e * (e + 1) / 2 <= t) e++;
  return (unsigned)((e << 4) | (t - e * (e - 1) / 2 + 1));
}
struct LaneTables {
  LaneTopo lane[64];
  unsigned short tab_ent[312];       // entry e of the sparse M -> (i << 8) | j
  unsigned short tab_dst[NV * 14];   // [k * 14 + a] = madr[anc_a(k)]
};
constexpr LaneTables make_lane_tables() {
  LaneTables T{};
  for (int lane = 0; lane < 64; lane++) {
    LaneTopo& t = T.lane[lane];
    const int b = lane < NB - 1 ? lane + 1 : 0;
    const int p1 = TOPO.body_parent[b] < 0 ? 0 : TOPO.body_parent[b], p2 = TOPO.body_parent[p1] < 0 ? 0 : TOPO.body_parent[p1], p3 = TOPO.body_parent[p2] < 0 ? 0 : TOPO.body_parent[p2];
    t.parent = p1 | (p2 << 4) | (p3 << 8);   // parent, grandparent, great-grandparent (0 = world)
    t.dofadr = TOPO.body_dofadr[b]; t.dofnum = TOPO.body_dofnum[b];
    t.depth = lane < NB - 1 ? TOPO.body_depth[b] : 0; t.subtree = TOPO.subtree[b];
    t.tri = 0;
    for (int j = 0; j < 6; j++) t.tri |= (unsigned long long)(tri_pair((lane & 15) + 16 * j) & 0xff) << (8 * j);
  }
  for (int e = 0; e < 312; e++) T.tab_ent[e] = e < TOPO.nM ? (unsigned short)((TOPO.ent_i[e] << 8) | TOPO.ent_j[e]) : (unsigned short)0;
  for (int k = 0; k < NV; k++) for (int a = 0; a < 14; a++) { const int i = TOPO.dof_anc[k][a]; T.tab_dst[k * 14 + a] = (unsigned short)(i >= 0 ? TOPO.madr[i] : 0); }
  return T;
}
DM_CONSTANT LaneTables LTAB = make_lane_tables();
DM_DEV LaneTopo lane_topo(int lane) { return LTAB.lane[lane & 63]; }
template <class R>
DM_DEV void stage_tables(Shared<R>& s, int lane) {
#pragma unroll
  for (int c = 0; c < (312 + 63) / 64; c++) { const int e = lane + 64 * c; if (e < 312) s.tab_ent[e] = LTAB.tab_ent[e]; }
#pragma unroll
  for (int c = 0; c < (NV * 14 + 63) / 64; c++) { const int t = lane + 64 * c; if (t < NV * 14) (&s.tab_dst[0][0])[t] = LTAB.tab_dst[t]; }
}

// optional dump of one forward evaluation (parity tests)
struct DebugOut {
  double* out;  // DM_DEBUG_DOUBLES
};

// ---------------------------------------------------------------------------------------------------------
// small math
template <class R> DM_DEV R dot3(const R* a, const R* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
template <class R> DM_DEV void cross3(R* r, const R* a, const R* b) {
  R x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
template <class R> DM_DEV R dot6(const R* a, const R* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
template <class R> DM_DEV R rsqrt_nr(R x) { return R(1) / sqrt(x); }
template <class R> DM_DEV R normalize3(R* v) {
  R n = sqrt(dot3(v, v));
  if (n < R(DM_MINVAL)) { v[0] = 1; v[1] = 0; v[2] = 0; }
  else { R s = R(1) / n; v[0] *= s; v[1] *= s; v[2] *= s; }
  return n;
}
template <class R> DM_DEV void normalize4(R* q) {
  R n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < R(DM_MINVAL)) { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  else if (fabs(n - R(1)) > R(DM_MINVAL)) { R s = R(1) / n; q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s; }
}
template <class R> DM_DEV void quat_mul(R* r, const R* a, const R* b) {
  R w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  R x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  R y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  R z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
template <class R> DM_DEV void quat2mat(R* m, const R* q) {
  R q00 = q[0] * q[0], q11 = q[1] * q[1], q22 = q[2] * q[2], q33 = q[3] * q[3];
  R q01 = q[0] * q[1], q02 = q[0] * q[2], q03 = q[0] * q[3], q12 = q[1] * q[2], q13 = q[1] * q[3], q23 = q[2] * q[3];
  m[0] = q00 + q11 - q22 - q33; m[1] = 2 * (q12 - q03);       m[2] = 2 * (q13 + q02);
  m[3] = 2 * (q12 + q03);       m[4] = q00 - q11 + q22 - q33; m[5] = 2 * (q23 - q01);
  m[6] = 2 * (q13 - q02);       m[7] = 2 * (q23 + q01);       m[8] = q00 - q11 - q22 + q33;
}
template <class R> DM_DEV void mat_vec(R* r, const R* m, const R* v) {
  R x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2], y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2], z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
template <class R> DM_DEV void matT_vec(R* r, const R* m, const R* v) {
  R x = m[0] * v[0] + m[3] * v[1] + m[6] * v[2], y = m[1] * v[0] + m[4] * v[1] + m[7] * v[2], z = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
// sin and cos of one angle with a single range reduction.  Not inlined: inlined into the RK loop, the compiler hoists the
// polynomial's dozen literal coefficients to kernel entry as loop invariants and, for want of registers, SPILLS them there and
// re-reads them from scratch in every evaluation (measured: 45 MB of scratch writes per launch).
// The same holds for the other libm routines used once per step or on cold paths (pow, exp, acos, atan2).
// (Results come back by value: out-pointers of a non-inlined function would live in scratch memory.)
#if defined(DM_WAVE_TESTBENCH)
#define DM_OUTLINE DM_DEV
#else
#define DM_OUTLINE __device__ __attribute__((noinline))
#endif
template <class R> DM_OUTLINE R pow_once(R x, R y) { return pow(x, y); }
template <class R> DM_OUTLINE R exp_once(R x) { return exp(x); }
template <class R> DM_OUTLINE R acos_once(R x) { return acos(x); }
template <class R> DM_OUTLINE R atan2_once(R y, R x) { return atan2(y, x); }
template <class R> struct SinCos { R s, c; };
#if defined(DM_WAVE_TESTBENCH)
template <class R> DM_DEV SinCos<R> sincos_once(R x) { return SinCos<R>{sin(x), cos(x)}; }
#else
__device__ __attribute__((noinline)) inline SinCos<double> sincos_once(double x) { SinCos<double> r; sincos(x, &r.s, &r.c); return r; }
__device__ __attribute__((noinline)) inline SinCos<float> sincos_once(float x) { SinCos<float> r; sincosf(x, &r.s, &r.c); return r; }
#endif
template <class R> DM_DEV void quat_rot(R* r, const R* q, const R* v) { R m[9]; quat2mat(m, q); mat_vec(r, m, v); }
template <class R> DM_DEV void axisangle2quat(R* q, const R* axis, R angle) {
  const SinCos<R> sc = sincos_once(angle * R(0.5));
  const R s = sc.s, c = sc.c;
  q[0] = c; q[1] = axis[0] * s; q[2] = axis[1] * s; q[3] = axis[2] * s;
}
DM_DEV int imin(int a, int b) { return a < b ? a : b; }
template <class R> DM_DEV R clampr(R x, R lo, R hi) { return x < lo ? lo : (x > hi ? hi : x); }
// spatial algebra about the world origin, vectors [ang; lin]
template <class R> DM_DEV void cross_motion(R* r, const R* v, const R* s) {
  R a[3], b[3], c[3];
  cross3(a, v, s); cross3(b, v, s + 3); cross3(c, v + 3, s);
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = b[0] + c[0]; r[4] = b[1] + c[1]; r[5] = b[2] + c[2];
}
template <class R> DM_DEV void cross_force(R* r, const R* v, const R* f) {
  R a[3], b[3], c[3];
  cross3(a, v, f); cross3(b, v + 3, f + 3); cross3(c, v, f + 3);
  r[0] = a[0] + b[0]; r[1] = a[1] + b[1]; r[2] = a[2] + b[2]; r[3] = c[0]; r[4] = c[1]; r[5] = c[2];
}
// spatial inertia S = {Ixx,Iyy,Izz,Ixy,Ixz,Iyz (about origin), m*c[3], m};  f = S v
template <class R> DM_DEV void sinert_mul(R* f, const R* S, const R* v) {
  R t0 = S[0] * v[0] + S[3] * v[1] + S[4] * v[2];
  R t1 = S[3] * v[0] + S[1] * v[1] + S[5] * v[2];
  R t2 = S[4] * v[0] + S[5] * v[1] + S[2] * v[2];
  R u[3];
  cross3(u, S + 6, v + 3);
  f[0] = t0 + u[0]; f[1] = t1 + u[1]; f[2] = t2 + u[2];
  cross3(u, v, S + 6);
  f[3] = S[9] * v[3] + u[0]; f[4] = S[9] * v[4] + u[1]; f[5] = S[9] * v[5] + u[2];
}

// ---------------------------------------------------------------------------------------------------------
// tree-sparse L^T D L solves with a vector held in registers (static indices: everything below is unrolled at compile
// time from TOPO).  Factor entries are read from LDS at wave-uniform addresses (broadcast).  The loops are software
// pipelined by hand: the entries of the NEXT row are loaded while the current row is applied, and the order pins
// (wave.h) keep the compiler from either hoisting all 310 loads to the top (>500 VGPRs) or issuing each load just
// before its use (every LDS round trip exposed).
template <int I, class R>
DM_DEV void load_factor_row(R* dst, const R* qLD) {
  if constexpr (I >= 0 && I < NV) {
#pragma unroll
    for (int a = 1; a < 14; a++) if (TOPO.dof_anc[I][a] >= 0) dst[a] = qLD[TOPO.madr[I] + a];
  }
}
template <int I, class R>
struct SolveLTStep {   // x <- L^-T x, rows NV-1 .. 1:  x[anc] -= L(I, anc) * x[I]
  static DM_DEV void run(R* x, const R* qLD, const R* cur) {
    R nxt[14];
    dmw::reload_fence();
    load_factor_row<I - 1>(nxt, qLD);
    dmw::sched_fence();
#pragma unroll
    for (int a = 1; a < 14; a++) { const int j = TOPO.dof_anc[I][a]; if (j >= 0) x[j] -= cur[a] * x[I]; }
    dmw::pin_value(x[TOPO.dof_anc[I][1]]);
    SolveLTStep<I - 1, R>::run(x, qLD, nxt);
  }
};
template <class R> struct SolveLTStep<0, R> { static DM_DEV void run(R*, const R*, const R*) {} };
template <class R> DM_DEV void solve_LT(R* x, const R* qLD) {
  R cur[14];
  dmw::reload_fence();
  load_factor_row<NV - 1>(cur, qLD);
  SolveLTStep<NV - 1, R>::run(x, qLD, cur);
}
template <int I, class R>
struct SolveLStep {    // x <- L^-1 x, rows 1 .. NV-1:  x[I] -= L(I, anc) * x[anc]
  static DM_DEV void run(R* x, const R* qLD, const R* cur) {
    R nxt[14];
    dmw::reload_fence();
    load_factor_row<I + 1>(nxt, qLD);
    dmw::sched_fence();
    R acc0 = 0, acc1 = 0;   // two partial sums: halves the dependent FMA chain of a 13-entry row
#pragma unroll
    for (int a = 1; a < 14; a++) {
      const int j = TOPO.dof_anc[I][a];
      if (j >= 0) { if (a & 1) acc0 += cur[a] * x[j]; else acc1 += cur[a] * x[j]; }
    }
    x[I] -= acc0 + acc1;
    dmw::pin_value(x[I]);
    SolveLStep<I + 1, R>::run(x, qLD, nxt);
  }
};
template <class R> struct SolveLStep<NV, R> { static DM_DEV void run(R*, const R*, const R*) {} };
template <class R> DM_DEV void solve_L(R* x, const R* qLD) {
  R cur[14];
  dmw::reload_fence();
  load_factor_row<1>(cur, qLD);
  SolveLStep<1, R>::run(x, qLD, cur);
}

// ---- subtree sums, lane-parallel over (body, component) ------------------------------------------------------------------
// out[b][k] = sum over the bodies c of b's subtree of in[c][k].  One lane per body would make the root's lane walk all 13
// bodies x NC components while the others idle; instead a lane owns one (body, component) pair — W lanes per body, 64 / W
// bodies per pass — and a pass only visits the bodies that occur in the subtrees of ITS bodies (compile-time union).
template <int NC, int W, int PASS>
constexpr unsigned subtree_union() {
  unsigned u = 0;
  for (int g = 0; g < 64 / W; g++) { const int b = 1 + PASS * (64 / W) + g; if (b < NB) u |= TOPO.subtree[b]; }
  return u;
}
template <int NC, int W, int PASS, int C, class R>
struct SubtreeAcc {
  static DM_DEV void run(R& acc, unsigned msk, const R (*in)[NC], int k) {
    if constexpr (C < NB) {
      if constexpr ((subtree_union<NC, W, PASS>() >> C) & 1u) acc += ((msk >> C) & 1u) ? in[C][k] : R(0);
      SubtreeAcc<NC, W, PASS, C + 1, R>::run(acc, msk, in, k);
    }
  }
};
template <int NC, int W, int PASS, class R>
DM_DEV void subtree_sums_pass(const R (*in)[NC], R (*out)[NC], int lane) {
  if constexpr (1 + PASS * (64 / W) < NB) {
    const int b = 1 + PASS * (64 / W) + lane / W, k = lane % W;       // W is a power of two
    if (b < NB && k < NC) {
      R acc = 0;
      SubtreeAcc<NC, W, PASS, 1, R>::run(acc, TOPO.subtree[b], in, k);
      out[b][k] = acc;
    }
    subtree_sums_pass<NC, W, PASS + 1, R>(in, out, lane);
  }
}

// ---------------------------------------------------------------------------------------------------------
// position stage: kinematics, motion axes, spatial inertias   [MJ mj_kinematics, mj_comPos]
// Only the composition of a body's frame with its parent's is serial in the tree depth, so the work is split:
//   1. per body (parallel): the product of its own hinge rotations q_loc and each hinge axis in the parent frame;
//   2. four levels (serial): xpos = xpos_p + R_p pos,  xquat = normalize(xquat_p * q_loc),  xmat;
//   3. per body (parallel): world joint axes -> cdof (about the world origin), xipos, spatial inertia;
//   4. composite inertias as static subtree sums.
template <class R>
DM_DEV void stage_kinematics(const DevModel<R>& M, Shared<R>& s, int lane_in, const LaneTopo& lt, R* qloc_out = nullptr, R (*aloc_out)[3] = nullptr) {
  const int lane = dmw::launder(lane_in);
  const int b = lane + 1;
  const bool isbody = lane < NB - 1;
  // laundered: otherwise every model constant indexed by these per-lane values (joint axes, body offsets, inertias) is
  // hoisted out of the RK loop as loop-invariant, spilled at kernel entry and re-read from scratch in every evaluation
  const int depth = dmw::launder(lt.depth), da = dmw::launder(lt.dofadr), nd = dmw::launder(lt.dofnum), panc = dmw::launder(lt.parent), p = panc & 15;
  R qloc[4] = {1, 0, 0, 0}, aloc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  if (lane == 0) {
    s.xpos[0][0] = s.xpos[0][1] = s.xpos[0][2] = 0; s.xipos[0][0] = s.xipos[0][1] = s.xipos[0][2] = 0;
    s.ua.xquat[0][0] = 1; s.ua.xquat[0][1] = s.ua.xquat[0][2] = s.ua.xquat[0][3] = 0;
    for (int k = 0; k < 9; k++) s.xmat[0][k] = (k % 4 == 0) ? R(1) : R(0);
  }
  // 1a. half-angle sine / cosine of every hinge, one lane per hinge (one sincos evaluation deep instead of three)
  if (lane < NU) {
    const R half = (s.qpos[lane + 7] - M.qpos0[lane + 7]) * R(0.5);
    const SinCos<R> sc = sincos_once(half);
    s.u.fdof[lane][0] = sc.c; s.u.fdof[lane][1] = sc.s;                   // (u.fdof is free until the mass-matrix stage)
  }
  dmw::sync();
  // 1b. local hinge chain (bodies 2..13)
  if (isbody && b > 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) if (k < nd) {
      const int d = da + k, j = d - 5;
      const R axl[3] = {M.jnt_axis[j][0], M.jnt_axis[j][1], M.jnt_axis[j][2]};
      R qm[9];
      quat2mat(qm, qloc);
      mat_vec(aloc[k], qm, axl);                       // axis of hinge k before its own rotation, in the parent frame
      const R c = s.u.fdof[d - 6][0], sn = s.u.fdof[d - 6][1];
      const R ql[4] = {c, axl[0] * sn, axl[1] * sn, axl[2] * sn};
      quat_mul(qloc, qloc, ql);
    }
  }
  if (qloc_out) {   // by-products the imitation reward's joint features are made of: child-in-parent rotation, hinge axes in the parent frame
    for (int k = 0; k < 4; k++) qloc_out[k] = qloc[k];
    for (int k = 0; k < 3; k++) for (int r = 0; r < 3; r++) aloc_out[k][r] = aloc[k][r];
  }
  // 2. compose down the tree.  Only the quaternion PRODUCT rides the serial chain (one quat_mul per level, unnormalised:
  // norms are multiplicative, so normalising the product is the per-level normalisation of mj_kinematics up to rounding);
  // normalisation, rotation matrices and frame offsets are then formed by all bodies at once, and a body's position is
  // the root-first sum of the offsets along its (at most 4 deep) chain — the same additions in the same order as
  // xpos = xpos_parent + R_parent pos.
  R q[4] = {1, 0, 0, 0};
#pragma unroll
  for (int L = 1; L <= MAXDEPTH_BODY; L++) {
    if (isbody && depth == L) {
      if (b == 1) { q[0] = s.qpos[3]; q[1] = s.qpos[4]; q[2] = s.qpos[5]; q[3] = s.qpos[6]; }
      else quat_mul(q, s.ua.xquat[p], qloc);
      for (int k = 0; k < 4; k++) s.ua.xquat[b][k] = q[k];
    }
    dmw::sync();
  }
  if (isbody) {
    R mat[9];
    normalize4(q);
    quat2mat(mat, q);
    for (int k = 0; k < 4; k++) s.ua.xquat[b][k] = q[k];
    for (int k = 0; k < 9; k++) s.xmat[b][k] = mat[k];
  }
  dmw::sync();
  if (isbody) {   // own frame offset in the world (s.xipos is the scratch list: it is only filled in step 3; entry 0 = world = 0)
    R v[3];
    if (b == 1) { v[0] = s.qpos[0]; v[1] = s.qpos[1]; v[2] = s.qpos[2]; }
    else mat_vec(v, s.xmat[p], M.body_pos[b]);
    for (int k = 0; k < 3; k++) s.xipos[b][k] = v[k];
  }
  dmw::sync();
  R xp[3] = {0, 0, 0};
  if (isbody) {
    const int p2 = (panc >> 4) & 15, p3 = (panc >> 8) & 15;
    for (int k = 0; k < 3; k++) xp[k] = ((s.xipos[p3][k] + s.xipos[p2][k]) + s.xipos[p][k]) + s.xipos[b][k];
  }
  dmw::sync();                                    // (everyone has read the offsets before step 3 overwrites them)
  if (isbody) for (int k = 0; k < 3; k++) s.xpos[b][k] = xp[k];
  // 3. motion axes, inertial frame position, own spatial inertia about the origin
  if (isbody) {
    const R* mat = s.xmat[b];
    if (b == 1) {
      for (int k = 0; k < 3; k++) {
        for (int r = 0; r < 6; r++) s.cdof[k][r] = (r == 3 + k) ? R(1) : R(0);
        const R ax[3] = {mat[k], mat[3 + k], mat[6 + k]};
        s.cdof[3 + k][0] = ax[0]; s.cdof[3 + k][1] = ax[1]; s.cdof[3 + k][2] = ax[2];
        cross3(&s.cdof[3 + k][3], xp, ax);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) if (k < nd) {
        R axw[3];
        mat_vec(axw, s.xmat[p], aloc[k]);
        s.cdof[da + k][0] = axw[0]; s.cdof[da + k][1] = axw[1]; s.cdof[da + k][2] = axw[2];
        cross3(&s.cdof[da + k][3], xp, axw);
      }
    }
    const R ip[3] = {M.body_ipos[b][0], M.body_ipos[b][1], M.body_ipos[b][2]};
    R c[3];
    mat_vec(c, mat, ip);
    c[0] += xp[0]; c[1] += xp[1]; c[2] += xp[2];
    s.xipos[b][0] = c[0]; s.xipos[b][1] = c[1]; s.xipos[b][2] = c[2];
    // Iw = R Ib R^T, then parallel-axis shift to the origin
    const R* Ib = M.body_inertia[b];
    const R A[9] = {Ib[0], Ib[3], Ib[4], Ib[3], Ib[1], Ib[5], Ib[4], Ib[5], Ib[2]};
    R T[9], Iw[9];
    for (int i = 0; i < 3; i++) for (int jx = 0; jx < 3; jx++) T[3 * i + jx] = mat[3 * i] * A[jx] + mat[3 * i + 1] * A[3 + jx] + mat[3 * i + 2] * A[6 + jx];
    for (int i = 0; i < 3; i++) for (int jx = 0; jx < 3; jx++) Iw[3 * i + jx] = T[3 * i] * mat[3 * jx] + T[3 * i + 1] * mat[3 * jx + 1] + T[3 * i + 2] * mat[3 * jx + 2];
    const R m = M.body_mass[b];
    const R cc = dot3(c, c);
    s.ub.i.sin[b][0] = Iw[0] + m * (cc - c[0] * c[0]); s.ub.i.sin[b][1] = Iw[4] + m * (cc - c[1] * c[1]); s.ub.i.sin[b][2] = Iw[8] + m * (cc - c[2] * c[2]);
    s.ub.i.sin[b][3] = Iw[1] - m * c[0] * c[1]; s.ub.i.sin[b][4] = Iw[2] - m * c[0] * c[2]; s.ub.i.sin[b][5] = Iw[5] - m * c[1] * c[2];
    s.ub.i.sin[b][6] = m * c[0]; s.ub.i.sin[b][7] = m * c[1]; s.ub.i.sin[b][8] = m * c[2]; s.ub.i.sin[b][9] = m;
  }
  dmw::sync();
  // 4. composite inertias: sum over the (static) subtree   [MJ mj_crb backward pass]
  subtree_sums_pass<10, 16, 0, R>(s.ub.i.sin, s.ub.i.crb, lane);
  dmw::sync();
}

// velocity stage: bias forces C(q, v) incl. gravity; smooth generalized force   [MJ mj_comVel, mj_rne, mj_passive]
// The recursion down the tree is  v_b = v_p + sum_k T_k,  a_b = a_p + sum_k (v_p + sum_{j<k} T_j) x T_k  with T_k = cdof_k qvel_k
// the body's own joint velocities (x = spatial motion cross product).  The cross product is bilinear, so
//   a_b = a_p + v_p x S_b + C_b,   S_b = sum_k T_k,   C_b = sum_{j<k} T_j x T_k
// and S_b, C_b need nothing from the parent: all bodies form them at once, and a level of the recursion is one cross product
// and two vector adds.  (The root's free joint keeps mj_comVel's special form: its three rotations all see the velocity
// after the translations.)  Then, each needing only an LDS hand-off from the one before: body forces I a + v x* I v for all
// bodies, their subtree sums, tau per dof.
// (Measured dead end: issuing the phases inside the elimination steps of the L^T D L factorisation, to overlap the two
//  independent serial chains in one instruction stream, gained nothing.)
template <class R>
DM_DEV void stage_bias(const DevModel<R>& M, Shared<R>& s, int lane_in, const LaneTopo& lt) {
  const int lane = dmw::launder(lane_in);
  const int b = lane + 1;
  const bool isbody = lane < NB - 1;
  const int depth = dmw::launder(lt.depth), p = dmw::launder(lt.parent) & 15, da = dmw::launder(lt.dofadr), nd = dmw::launder(lt.dofnum);
  if (lane == 0) {
    for (int r = 0; r < 6; r++) { s.u.v.cvel[0][r] = 0; s.u.v.cacc[0][r] = 0; }
    s.u.v.cacc[0][3] = -M.gravity[0]; s.u.v.cacc[0][4] = -M.gravity[1]; s.u.v.cacc[0][5] = -M.gravity[2];
  }
  R S[6] = {0, 0, 0, 0, 0, 0}, C[6] = {0, 0, 0, 0, 0, 0};
  if (isbody && b > 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) if (k < nd) {
      const R qd = s.qvel[da + k];
      R T[6], cd[6];
      for (int r = 0; r < 6; r++) T[r] = s.cdof[da + k][r] * qd;
      if (k > 0) { cross_motion(cd, S, T); for (int r = 0; r < 6; r++) C[r] += cd[r]; }
      for (int r = 0; r < 6; r++) S[r] += T[r];
    }
  }
  dmw::sync();
#pragma unroll
  for (int L = 1; L <= MAXDEPTH_BODY; L++) {
    if (isbody && depth == L) {
      R v[6], a[6];
      for (int r = 0; r < 6; r++) { v[r] = s.u.v.cvel[p][r]; a[r] = s.u.v.cacc[p][r]; }
      if (b == 1) {
        for (int k = 0; k < 3; k++) { const R qd = s.qvel[k]; for (int r = 0; r < 6; r++) v[r] += s.cdof[k][r] * qd; }
        R vb[6];
        for (int r = 0; r < 6; r++) vb[r] = v[r];
        for (int k = 3; k < 6; k++) {
          R cd[6]; cross_motion(cd, vb, s.cdof[k]);
          const R qd = s.qvel[k];
          for (int r = 0; r < 6; r++) { a[r] += cd[r] * qd; v[r] += s.cdof[k][r] * qd; }
        }
      } else {
        R cd[6];
        cross_motion(cd, v, S);
        for (int r = 0; r < 6; r++) { a[r] += cd[r] + C[r]; v[r] += S[r]; }
      }
      for (int r = 0; r < 6; r++) { s.u.v.cvel[b][r] = v[r]; s.u.v.cacc[b][r] = a[r]; }
    }
    dmw::sync();
  }
  // body forces I a + v x* (I v): they need only the body's own velocity / acceleration, so all bodies form them at once
  if (isbody) {
    R v[6], a[6];
    for (int r = 0; r < 6; r++) { v[r] = s.u.v.cvel[b][r]; a[r] = s.u.v.cacc[b][r]; }
    R Ia[6], Iv[6], x[6];
    sinert_mul(Ia, s.ub.i.sin[b], a); sinert_mul(Iv, s.ub.i.sin[b], v); cross_force(x, v, Iv);
    for (int r = 0; r < 6; r++) s.u.v.cfrc[b][r] = Ia[r] + x[r];
  }
  dmw::sync();
  subtree_sums_pass<6, 8, 0, R>(s.u.v.cfrc, s.u.v.csub, lane);
  dmw::sync();
  if (lane < NV) {
    const R bias = dot6(s.cdof[lane], s.u.v.csub[TOPO.dof_body[lane]]);
    s.ua.f.tau[lane] = -M.dof_damping[lane] * s.qvel[lane] - bias + s.act[lane];
  }
  dmw::sync();
}

// mass matrix (tree-sparse, MuJoCo qM order) and its L^T D L factor   [MJ mj_crb, mj_factorM]
// Elimination schedule.  Column K only touches entries (i, j) with i, j proper ancestors of K, and reads its own row, so
// columns of dofs in different branches of the tree commute: the four limbs (and the neck beside the hips) are eliminated
// side by side, each in its own group of lanes — 15 dependent steps instead of 33.  Entries of common ancestors (root and
// chest blocks) receive one contribution per limb in the same step; the updates are LDS atomics (dmw::lds_sub), which
// also makes every update fire-and-forget.
struct ElimStep { int ncol; int K[4]; };
constexpr int N_ELIM_STEPS = 15;
constexpr ElimStep ELIM_STEPS[N_ELIM_STEPS] = {
  {4, {33, 26, 19, 15}}, {4, {32, 25, 18, 14}}, {4, {31, 24, 17, 13}}, {4, {30, 23, 16, 12}},   // ankles | elbows, shoulders;  knees
  {3, {29, 22, 11, 0}}, {3, {28, 21, 10, 0}}, {3, {27, 20, 9, 0}},                                // hips (16 lanes each) | neck (32 lanes)
  {1, {8, 0, 0, 0}}, {1, {7, 0, 0, 0}}, {1, {6, 0, 0, 0}},                                        // chest
  {1, {5, 0, 0, 0}}, {1, {4, 0, 0, 0}}, {1, {3, 0, 0, 0}}, {1, {2, 0, 0, 0}}, {1, {1, 0, 0, 0}}}; // root
constexpr bool dof_is_ancestor(int anc, int d) {
  for (int a = 1; a < 16; a++) if (TOPO.dof_anc[d][a] == anc) return true;
  return false;
}
constexpr bool elim_schedule_ok() {
  bool seen[NV] = {};
  for (int st = 0; st < N_ELIM_STEPS; st++) {
    const ElimStep& e = ELIM_STEPS[st];
    for (int c = 0; c < e.ncol; c++) {
      const int K = e.K[c];
      if (K < 1 || K >= NV || seen[K]) return false;
      for (int d = 0; d < NV; d++) if (dof_is_ancestor(K, d) && !seen[d]) return false;          // descendants first
      for (int c2 = 0; c2 < e.ncol; c2++) if (c2 != c && (dof_is_ancestor(K, e.K[c2]) || dof_is_ancestor(e.K[c2], K) || e.K[c2] == K)) return false;
    }
    for (int c = 0; c < e.ncol; c++) seen[e.K[c]] = true;
  }
  for (int d = 1; d < NV; d++) if (!seen[d]) return false;
  return true;
}
static_assert(elim_schedule_ok(), "elimination schedule: every dof once, descendants before ancestors, independent columns per step");
constexpr int elim_group_size(int ncol, int c) { return ncol == 1 ? 64 : ncol == 2 ? 32 : ncol == 4 ? 16 : (c < 2 ? 16 : 32); }
constexpr int elim_npairs(int K) { return (TOPO.dof_depth[K] - 1) * TOPO.dof_depth[K] / 2; }
constexpr int elim_passes(int S) {
  const ElimStep& e = ELIM_STEPS[S];
  int m = 0;
  for (int c = 0; c < e.ncol; c++) { const int g = elim_group_size(e.ncol, c), q = (elim_npairs(e.K[c]) + g - 1) / g; m = q > m ? q : m; }
  return m;
}
constexpr bool elim_codes_ok() {   // a lane holds the codes of pair numbers (lane & 15) + 16 j, j < 6
  for (int S = 0; S < N_ELIM_STEPS; S++) for (int c = 0; c < ELIM_STEPS[S].ncol; c++) {
    const int g = elim_group_size(ELIM_STEPS[S].ncol, c), np = elim_npairs(ELIM_STEPS[S].K[c]);
    if (np > 96 || (g == 64 && np > 64)) return false;
  }
  return true;
}
static_assert(elim_codes_ok(), "pair numbers of a column must stay below 96 (below 64 for a full-wave column)");
// per step and lane: the column the lane works on, packed  row base (9 bits) | number of pairs << 9 (7) | ancestor-table row << 16 (9) |
// log2(group size / 16) << 25;  a lane's index inside its group is lane & (group size - 1)
struct ElimLaneTable { unsigned a[64][N_ELIM_STEPS + 1]; };
constexpr ElimLaneTable make_elim_lane_table() {
  ElimLaneTable T{};
  for (int S = 0; S < N_ELIM_STEPS; S++) {
    const ElimStep& st = ELIM_STEPS[S];
    for (int lane = 0; lane < 64; lane++) {
      int ci = 0;
      if (st.ncol == 2) ci = lane >> 5;
      else if (st.ncol == 3) ci = lane < 32 ? (lane >> 4) : 2;
      else if (st.ncol == 4) ci = lane >> 4;
      const int K = st.K[ci], gs = elim_group_size(st.ncol, ci);
      T.a[lane][S] = (unsigned)TOPO.madr[K] | ((unsigned)elim_npairs(K) << 9) | ((unsigned)(K * 14) << 16) | ((unsigned)(gs == 16 ? 0 : gs == 32 ? 1 : 2) << 25);
    }
  }
  return T;
}
DM_CONSTANT ElimLaneTable ELIM_LANE = make_elim_lane_table();

template <int S, class R>
DM_DEV void eliminate_step(Shared<R>& s, int lane_in, const LaneTopo& lt, const unsigned* ew) {
  // column K:  for every ancestor pair (a, c), row i = anc_a(K):   M(i, anc_c(i)) -= M(K, anc_{a+c}(K)) * M(K, i) / M(K, K)
  // Row K itself is left unscaled (nothing reads it again during the factorisation); all rows are scaled at the end.
  // The update pairs (a, e = a + c), 1 <= a <= e <= nk, are the lower triangle of an nk x nk matrix; enumerated by
  // t = e (e - 1) / 2 + a - 1 the first nk (nk + 1) / 2 numbers are exactly a column's pairs, whatever nk is, so each lane
  // keeps the codes of the six pair numbers it can ever be given (LaneTopo) and a step needs no index arithmetic.
  constexpr ElimStep st = ELIM_STEPS[S];
  constexpr int NC = st.ncol;
  const int lane = dmw::launder(lane_in);     // (laundered: the per-lane step constants below must not be hoisted out of the RK loop)
  // this lane's column of the step (row base, number of pairs, ancestor-table row) and its lane group: one table word per step
  // and lane (compile-time schedule, loaded at the top of the stage), not a chain of selects
  const unsigned w = ew[S];
  const int base = (int)(w & 511u), np = (int)((w >> 9) & 127u), k14 = (int)((w >> 16) & 511u);
  const int gs = 16 << (w >> 25), lg = lane & (gs - 1);
  constexpr int passes = elim_passes(S);
  const R inv = dmw::rcp_fast(s.qLD[base]);
  const unsigned short* tdst = &s.tab_dst[0][0];
#pragma unroll
  for (int p = 0; p < passes; p++) {
    const int t = lg + gs * p;
    const bool on = t < np;
    const int code = on ? (int)(lt.tri >> (8 * (t >> 4))) & 0xff : 0, e = code >> 4, a = code & 15;
    const int dst = tdst[k14 + a] + (e - a);
    dmw::lds_sub(on, &s.qLD[dst], s.qLD[base + e] * (s.qLD[base + a] * inv));
  }
  dmw::sync();
}
template <int S, class R>
struct EliminateFrom {
  static DM_DEV void run(Shared<R>& s, int lane, const LaneTopo& lt, const unsigned* ew) {
    if constexpr (S < N_ELIM_STEPS) { eliminate_step<S>(s, lane, lt, ew); EliminateFrom<S + 1, R>::run(s, lane, lt, ew); }
  }
};

// SPD (action modes 3 and 4, env_step.h spd_control): the factor of M + h diag(kd) instead — only the diagonal moves, the sparsity and the schedule stay.
template <class R, bool SPD = false>
DM_DEV void stage_mass_matrix(const DevModel<R>& M, Shared<R>& s, int lane_in, const LaneTopo& lt, const DebugOut* dbg) {
  const int lane = dmw::launder(lane_in);
  // the elimination schedule's per-lane words, all requested here: their latency hides behind the assembly of M
  unsigned ew[N_ELIM_STEPS];
#pragma unroll
  for (int k = 0; k < N_ELIM_STEPS; k++) ew[k] = ELIM_LANE.a[lane][k];
  if (lane < NV) {
    R f[6];
    sinert_mul(f, s.ub.i.crb[TOPO.dof_body[lane]], s.cdof[lane]);
    for (int r = 0; r < 6; r++) s.u.fdof[lane][r] = f[r];
    if constexpr (SPD) s.dinv[lane] = M.dof_armature[lane] + M.timestep * M.kd[lane];
    else
    s.dinv[lane] = M.dof_armature[lane];     // staged once (coalesced) — s.dinv is dead until the end of the factorisation;
  }                                          // a per-entry `M.dof_armature[i]` would be a divergent global load in every pass
  dmw::sync();
  // (compile-time trip count: only the last of the 5 passes is partial and needs a lane predicate — ~45 cycles each)
#pragma unroll
  for (int c = 0; c < (TOPO.nM + 63) / 64; c++) {
    const int e = lane + 64 * c;
    if ((c + 1) * 64 <= TOPO.nM || e < TOPO.nM) {
      const int ij = s.tab_ent[e], i = ij >> 8, j = ij & 0xff;
      R v = dot6(s.cdof[j], s.u.fdof[i]);
      if (i == j) v += s.dinv[i];
      s.qLD[e] = v;
      if (dbg) { dbg->out[i * NV + j] = (double)v; dbg->out[j * NV + i] = (double)v; }
    }
  }
  dmw::sync();
  EliminateFrom<0, R>::run(s, lane, lt, ew);   // 15 steps of mutually independent columns, one barrier each (fully unrolled)
  // D^-1, D^-1/2 and the unit-triangular scaling L(k, j) = M(k, j) / D_k, all entries at once
  if (lane < NV) { const R inv = R(1) / s.qLD[TOPO.madr[lane]]; s.dinv[lane] = inv; s.dsq[lane] = sqrt(inv); }
  dmw::sync();
#pragma unroll
  for (int c = 0; c < (TOPO.nM + 63) / 64; c++) {
    const int e = lane + 64 * c;
    if ((c + 1) * 64 <= TOPO.nM || e < TOPO.nM) {
      const int ij = s.tab_ent[e], i = ij >> 8, j = ij & 0xff;
      const R sc = i != j ? s.dinv[i] : R(1);     // (select, not a predicated region)
      s.qLD[e] *= sc;
    }
  }
  dmw::sync();
}

// ---------------------------------------------------------------------------------------------------------
// collision: narrow phase for one candidate pair.  Contacts of a pair share the frame (normal n, tangent hint h).
// Up to two contacts live in registers (static slots); plane-box corners (up to 4) are staged in LDS (s.boxc).
template <class R>
struct PairContacts {
  int n, boxslot;
  R nrm[3], hint[3];
  R d0, p0[3], d1, p1[3];
};

// plane through p0 with unit normal n vs sphere (c, r): returns hit, distance and contact position  [MJ mjc_PlaneSphere]
template <class R>
DM_DEV bool plane_sphere(const R* p0, const R* n, const R* c, R r, R margin, R& dist, R* pos) {
  R t[3] = {c[0] - p0[0], c[1] - p0[1], c[2] - p0[2]};
  const R cd = dot3(t, n);
  dist = cd - r;
  const R sc = -dist / 2 - r;
  pos[0] = c[0] + n[0] * sc; pos[1] = c[1] + n[1] * sc; pos[2] = c[2] + n[2] * sc;
  return !(cd > margin + r);
}
template <class R>
DM_DEV void sphere_sphere(PairContacts<R>& pc, const R* c1, R r1, const R* c2, R r2, R margin) {
  R dif[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  const R bound = margin + r1 + r2;
  if (dot3(dif, dif) > bound * bound) return;
  const R nn = normalize3(dif);
  pc.n = 1;
  pc.nrm[0] = dif[0]; pc.nrm[1] = dif[1]; pc.nrm[2] = dif[2];
  pc.d0 = nn - r1 - r2;
  const R sc = r1 + R(0.5) * pc.d0;
  pc.p0[0] = c1[0] + dif[0] * sc; pc.p0[1] = c1[1] + dif[1] * sc; pc.p0[2] = c1[2] + dif[2] * sc;
}

// box-box: separating-axis test (6 face normals + 9 edge cross products); least-penetration axis -> either a face
// contact (incident face clipped against the reference face, the 4 deepest clipped vertices within the margin) or one
// edge-edge contact.  Own algorithm, identical to the oracle's box_box (MuJoCo's mjc_BoxBox is not restated).  Runs in a
// single lane (the feet pair); the clipping polygons and the contacts are staged in LDS.
// LDS scratch of the narrow phase, by pointer so that the one-env kernel (Shared) and the four-envs-per-wave kernel (slot_kernel.h)
// share the routines: box axes [2][3][3] and clipping polygons [2][8][3] of box-box (dynamically indexed), and the staged contacts
// (dist, pos) [slot][4][4] of the pair types that can yield more than two.
template <class R>
struct BoxScratch {
  R (*axes)[3][3];
  R (*poly)[8][3];
  R (*boxc)[4][4];
};
template <class R>
DM_DEV void box_box(const BoxScratch<R>& bx, const R* p1, const R* m1, const R* s1, const R* p2, const R* m2, const R* s2, int slot, R margin,
                    PairContacts<R>& pc) {
  // box axes live in LDS: they are indexed with run-time axis numbers below (register arrays would go to scratch)
  R (*A)[3] = bx.axes[0];
  R (*B)[3] = bx.axes[1];
  R aR[3][3];
  for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) { A[i][k] = m1[3 * k + i]; B[i][k] = m2[3 * k + i]; }
  const R d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) aR[i][j] = fabs(dot3(A[i], B[j]));
  R best = R(-1e300);
  int code = -1;
  for (int i = 0; i < 3; i++) {
    const R sep = fabs(dot3(d, A[i])) - (s1[i] + s2[0] * aR[i][0] + s2[1] * aR[i][1] + s2[2] * aR[i][2]);
    if (sep > margin) return;
    if (sep > best) { best = sep; code = i; }
  }
  for (int j = 0; j < 3; j++) {
    const R sep = fabs(dot3(d, B[j])) - (s2[j] + s1[0] * aR[0][j] + s1[1] * aR[1][j] + s1[2] * aR[2][j]);
    if (sep > margin) return;
    if (sep > best) { best = sep; code = 3 + j; }
  }
  R ebest = R(-1e300), en[3] = {0, 0, 0};
  int ei = -1, ej = -1;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
    R L[3];
    cross3(L, A[i], B[j]);
    const R len = sqrt(dot3(L, L));
    if (len < R(1e-6)) continue;
    L[0] /= len; L[1] /= len; L[2] /= len;
    const R rA = s1[0] * fabs(dot3(A[0], L)) + s1[1] * fabs(dot3(A[1], L)) + s1[2] * fabs(dot3(A[2], L));
    const R rB = s2[0] * fabs(dot3(B[0], L)) + s2[1] * fabs(dot3(B[1], L)) + s2[2] * fabs(dot3(B[2], L));
    const R dl = dot3(d, L), sep = fabs(dl) - rA - rB;
    if (sep > margin) return;
    if (sep > ebest) { ebest = sep; ei = i; ej = j; const R sg = dl < 0 ? R(-1) : R(1); en[0] = sg * L[0]; en[1] = sg * L[1]; en[2] = sg * L[2]; }
  }
  pc.boxslot = slot;
  if (ei >= 0 && ebest > best + R(1e-6)) {
    R ca[3] = {p1[0], p1[1], p1[2]}, cb[3] = {p2[0], p2[1], p2[2]};
    for (int k = 0; k < 3; k++) if (k != ei) { const R sg = (dot3(en, A[k]) > 0 ? R(1) : R(-1)) * s1[k]; ca[0] += A[k][0] * sg; ca[1] += A[k][1] * sg; ca[2] += A[k][2] * sg; }
    for (int k = 0; k < 3; k++) if (k != ej) { const R sg = (dot3(en, B[k]) > 0 ? R(-1) : R(1)) * s2[k]; cb[0] += B[k][0] * sg; cb[1] += B[k][1] * sg; cb[2] += B[k][2] * sg; }
    const R w[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    const R ab = dot3(A[ei], B[ej]), aw = dot3(A[ei], w), bw = dot3(B[ej], w), den = 1 - ab * ab;
    R ta = den > R(1e-12) ? (ab * bw - aw) / den : R(0), tb = den > R(1e-12) ? (bw - ab * aw) / den : R(0);
    ta = clampr(ta, -s1[ei], s1[ei]); tb = clampr(tb, -s2[ej], s2[ej]);
    R* o = bx.boxc[slot][0];
    o[0] = ebest;
    for (int k = 0; k < 3; k++) o[1 + k] = R(0.5) * ((ca[k] + A[ei][k] * ta) + (cb[k] + B[ej][k] * tb));
    pc.nrm[0] = en[0]; pc.nrm[1] = en[1]; pc.nrm[2] = en[2];
    pc.n = 1;
    return;
  }
  const bool refB = code >= 3;
  const int ax = refB ? code - 3 : code;
  const R* pr = refB ? p2 : p1; const R* pi = refB ? p1 : p2; const R* sr = refB ? s2 : s1; const R* si = refB ? s1 : s2;
  R (*Rr)[3] = refB ? B : A; R (*Ri)[3] = refB ? A : B;
  const R dr[3] = {pi[0] - pr[0], pi[1] - pr[1], pi[2] - pr[2]};
  const R sgn = dot3(dr, Rr[ax]) < 0 ? R(-1) : R(1);
  const R n[3] = {sgn * Rr[ax][0], sgn * Rr[ax][1], sgn * Rr[ax][2]};
  int k = 0;
  R bestdot = -1;
  for (int j = 0; j < 3; j++) { const R dd = fabs(dot3(n, Ri[j])); if (dd > bestdot) { bestdot = dd; k = j; } }
  const R fs = dot3(n, Ri[k]) > 0 ? R(-1) : R(1);
  const int k1 = (k + 1) % 3, k2 = (k + 2) % 3, u = (ax + 1) % 3, v = (ax + 2) % 3;
  int np = 4, cur = 0;
  for (int c = 0; c < 4; c++) {
    const R a1 = (c == 0 || c == 3) ? R(1) : R(-1), a2 = (c < 2) ? R(1) : R(-1);
    R rel[3];
    for (int t = 0; t < 3; t++) rel[t] = pi[t] + fs * si[k] * Ri[k][t] + a1 * si[k1] * Ri[k1][t] + a2 * si[k2] * Ri[k2][t] - pr[t];
    bx.poly[0][c][0] = dot3(rel, Rr[u]); bx.poly[0][c][1] = dot3(rel, Rr[v]); bx.poly[0][c][2] = sgn * dot3(rel, Rr[ax]);
  }
  for (int e = 0; e < 4 && np > 0; e++) {
    const int cdim = e / 2;
    const R sg = (e % 2) ? R(-1) : R(1), lim = cdim == 0 ? sr[u] : sr[v];
    int nn = 0;
    for (int a = 0; a < np; a++) {
      const R* P = bx.poly[cur][a]; const R* Q = bx.poly[cur][(a + 1) % np];
      const R P0 = P[0], P1 = P[1], P2 = P[2], Q0 = Q[0], Q1 = Q[1], Q2 = Q[2];
      const R dp = lim - sg * (cdim == 0 ? P0 : P1), dq = lim - sg * (cdim == 0 ? Q0 : Q1);
      if (dp >= 0 && nn < 8) { R* o = bx.poly[1 - cur][nn]; o[0] = P0; o[1] = P1; o[2] = P2; nn++; }
      if ((dp >= 0) != (dq >= 0) && nn < 8) {
        const R tt = dp / (dp - dq);
        R* o = bx.poly[1 - cur][nn];
        o[0] = P0 + tt * (Q0 - P0); o[1] = P1 + tt * (Q1 - P1); o[2] = P2 + tt * (Q2 - P2); nn++;
      }
    }
    np = nn; cur = 1 - cur;
  }
  // keep the (up to) 4 deepest candidates within the margin, in polygon order (bit mask instead of an array)
  unsigned keep = 0;
  int nk = 0;
  for (int a = 0; a < np; a++) if (bx.poly[cur][a][2] - sr[ax] < margin) { keep |= 1u << a; nk++; }
  while (nk > 4) {
    int worst = -1;
    R wd = 0;
    for (int a = 0; a < np; a++) if ((keep >> a) & 1u) { const R da = bx.poly[cur][a][2] - sr[ax]; if (worst < 0 || da > wd) { worst = a; wd = da; } }
    keep &= ~(1u << worst); nk--;
  }
  int cnt = 0;
  for (int a = 0; a < np; a++) if ((keep >> a) & 1u) {
    const R* P = bx.poly[cur][a];
    const R da = P[2] - sr[ax];
    R* o = bx.boxc[slot][cnt];
    o[0] = da;
    for (int t = 0; t < 3; t++) o[1 + t] = (pr[t] + P[0] * Rr[u][t] + P[1] * Rr[v][t] + sgn * P[2] * Rr[ax][t]) - n[t] * da / 2;
    cnt++;
  }
  pc.nrm[0] = refB ? -n[0] : n[0]; pc.nrm[1] = refB ? -n[1] : n[1]; pc.nrm[2] = refB ? -n[2] : n[2];
  pc.n = cnt;
}

// p1, m1 / p2, m2: world position and orientation (row-major 3x3) of the two geoms
template <class R>
DM_DEV void narrowphase_at(const BoxScratch<R>& bx, const R* p1, const R* m1, const R* p2, const R* m2, int t1, int t2, const R* s1, const R* s2,
                           const R* gs1, const R* gs2, int stage_slot, R margin, PairContacts<R>& pc) {
  // s1 / s2: the geom sizes in registers (requested with the rest of the pair record: no load inside the divergent type
  // branches); gs1 / gs2: the same in memory, for box-box, which indexes them with run-time axis numbers
  pc.n = 0; pc.boxslot = -1;
  pc.hint[0] = pc.hint[1] = pc.hint[2] = 0;
  pc.nrm[0] = pc.nrm[1] = 0; pc.nrm[2] = 1;
  pc.d0 = pc.d1 = 0; pc.p0[0] = pc.p0[1] = pc.p0[2] = 0; pc.p1[0] = pc.p1[1] = pc.p1[2] = 0;
  if (t1 == GEOM_PLANE) {
    const R n[3] = {m1[2], m1[5], m1[8]};
    pc.nrm[0] = n[0]; pc.nrm[1] = n[1]; pc.nrm[2] = n[2];
    if (t2 == GEOM_SPHERE) {
      if (plane_sphere(p1, n, p2, s2[0], margin, pc.d0, pc.p0)) pc.n = 1;
    } else if (t2 == GEOM_CAPSULE) {   // [MJ mjc_PlaneCapsule] +axis end first, tangent hint = axis
      const R ax[3] = {m2[2], m2[5], m2[8]};
      R c[3] = {p2[0] + ax[0] * s2[1], p2[1] + ax[1] * s2[1], p2[2] + ax[2] * s2[1]};
      const bool ha = plane_sphere(p1, n, c, s2[0], margin, pc.d0, pc.p0);
      c[0] = p2[0] - ax[0] * s2[1]; c[1] = p2[1] - ax[1] * s2[1]; c[2] = p2[2] - ax[2] * s2[1];
      const bool hb = plane_sphere(p1, n, c, s2[0], margin, pc.d1, pc.p1);
      if (!ha && hb) { pc.d0 = pc.d1; pc.p0[0] = pc.p1[0]; pc.p0[1] = pc.p1[1]; pc.p0[2] = pc.p1[2]; }
      pc.n = (ha ? 1 : 0) + (hb ? 1 : 0);
      pc.hint[0] = ax[0]; pc.hint[1] = ax[1]; pc.hint[2] = ax[2];
    } else if (t2 == GEOM_BOX) {       // [MJ mjc_PlaneBox] corners below the margin, at most 4, staged in LDS
      const R dif[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
      const R dist = dot3(dif, n);
      const int slot = stage_slot;
      pc.boxslot = slot;
      for (int i = 0; i < 8 && pc.n < 4; i++) {
        const R vec[3] = {(i & 1) ? s2[0] : -s2[0], (i & 2) ? s2[1] : -s2[1], (i & 4) ? s2[2] : -s2[2]};
        R corner[3];
        mat_vec(corner, m2, vec);
        const R ld = dot3(n, corner);
        if (dist + ld > margin || ld > 0) continue;
        const int k = pc.n++;
        const R dk = dist + ld, sc = -dk / 2;
        R* o = bx.boxc[slot][k];
        o[0] = dk; o[1] = corner[0] + p2[0] + n[0] * sc; o[2] = corner[1] + p2[1] + n[1] * sc; o[3] = corner[2] + p2[2] + n[2] * sc;
      }
    }
    return;
  }
  if (t2 <= GEOM_CAPSULE) {  // sphere/capsule family: closest points of two (possibly degenerate) segments
    R c1[3] = {p1[0], p1[1], p1[2]}, c2[3] = {p2[0], p2[1], p2[2]};
    if (t1 == GEOM_SPHERE && t2 == GEOM_CAPSULE) {        // [MJ mjc_SphereCapsule]
      const R ax[3] = {m2[2], m2[5], m2[8]};
      const R v[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
      const R x = clampr(dot3(ax, v), -s2[1], s2[1]);
      c2[0] += ax[0] * x; c2[1] += ax[1] * x; c2[2] += ax[2] * x;
    } else if (t1 == GEOM_CAPSULE) {                       // [MJ mjc_CapsuleCapsule], non-parallel branch
      const R a1[3] = {m1[2], m1[5], m1[8]}, a2[3] = {m2[2], m2[5], m2[8]};
      const R dif[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
      const R ma = dot3(a1, a1), mb = -dot3(a1, a2), mc = dot3(a2, a2), u = -dot3(a1, dif), v = dot3(a2, dif);
      const R det = ma * mc - mb * mb;
      R x1, x2;
      if (fabs(det) >= R(DM_MINVAL)) {
        x1 = (mc * u - mb * v) / det; x2 = (ma * v - mb * u) / det;
        if (x1 > s1[1]) { x1 = s1[1]; x2 = (v - mb * s1[1]) / mc; } else if (x1 < -s1[1]) { x1 = -s1[1]; x2 = (v + mb * s1[1]) / mc; }
        if (x2 > s2[1]) { x2 = s2[1]; x1 = (u - mb * s2[1]) / ma; } else if (x2 < -s2[1]) { x2 = -s2[1]; x1 = (u + mb * s2[1]) / ma; }
        if (x1 > s1[1]) x1 = s1[1]; else if (x1 < -s1[1]) x1 = -s1[1];
      } else {  // parallel axes (measure zero): first end of capsule 1 against segment 2
        x1 = s1[1];
        const R t[3] = {p1[0] + a1[0] * x1 - p2[0], p1[1] + a1[1] * x1 - p2[1], p1[2] + a1[2] * x1 - p2[2]};
        x2 = clampr(dot3(t, a2), -s2[1], s2[1]);
      }
      c1[0] += a1[0] * x1; c1[1] += a1[1] * x1; c1[2] += a1[2] * x1;
      c2[0] += a2[0] * x2; c2[1] += a2[1] * x2; c2[2] += a2[2] * x2;
    }
    sphere_sphere(pc, c1, s1[0], c2, s2[0], margin);
    return;
  }
  if (t1 == GEOM_SPHERE && t2 == GEOM_BOX) {  // [MJ mjc_SphereBox]
    R t[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]}, center[3], clamped[3], nrm[3], pl[3];
    matT_vec(center, m2, t);
    for (int i = 0; i < 3; i++) clamped[i] = clampr(center[i], -s2[i], s2[i]);
    t[0] = center[0] - clamped[0]; t[1] = center[1] - clamped[1]; t[2] = center[2] - clamped[2];
    const R dist = sqrt(dot3(t, t));
    if (dist - s1[0] > margin) return;
    if (dist <= R(DM_MINVAL)) {
      R closest = 2 * fmax(s2[0], fmax(s2[1], s2[2]));
      int k = 0;
#pragma unroll
      for (int i = 0; i < 6; i++) { const R fd = fabs(((i % 2) ? R(1) : R(-1)) * s2[i / 2] - center[i / 2]); if (closest > fd) { closest = fd; k = i; } }
      nrm[0] = nrm[1] = nrm[2] = 0; nrm[k / 2] = (k % 2) ? R(-1) : R(1);
      const R sc = (s1[0] - closest) / 2;
      pl[0] = center[0] + nrm[0] * sc; pl[1] = center[1] + nrm[1] * sc; pl[2] = center[2] + nrm[2] * sc;
      pc.d0 = -closest - s1[0];
    } else {
      for (int i = 0; i < 3; i++) nrm[i] = -t[i] / dist;
      const R sc = s1[0] + R(0.5) * (dist - s1[0]);
      pl[0] = center[0] + nrm[0] * sc; pl[1] = center[1] + nrm[1] * sc; pl[2] = center[2] + nrm[2] * sc;
      pc.d0 = dist - s1[0];
    }
    pc.n = 1;
    mat_vec(pc.nrm, m2, nrm);
    mat_vec(pc.p0, m2, pl);
    pc.p0[0] += p2[0]; pc.p0[1] += p2[1]; pc.p0[2] += p2[2];
    return;
  }
  if (t1 == GEOM_CAPSULE && t2 == GEOM_BOX) {
    // closest point of the capsule segment to the box, then one sphere-box contact there (own algorithm, shared with the CPU oracle;
    // MuJoCo's mjc_CapsuleBox is a case analysis that is not restated).  In the box frame the squared distance of
    // c0 + t u to the box is convex and piecewise quadratic in t: its half-derivative g(t) = sum_k u_k (p_k - clamp(p_k)) is
    // piecewise linear, non-decreasing, with breakpoints where a coordinate crosses a face plane.  The zero of g is bracketed
    // between consecutive breakpoints inside [-L, L] and interpolated: exact up to rounding, no iteration (an earlier
    // 48-step golden-section search cost ~7 k cycles whenever a leg came near the other foot).
    const R ax[3] = {m1[2], m1[5], m1[8]};
    R t[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]}, c0[3], u[3];
    matT_vec(c0, m2, t); matT_vec(u, m2, ax);
    // slab rejection first (a leg next to the other foot is the common case: its bounding sphere reaches the box, the
    // capsule does not): the segment's extent along a box axis lies farther from the box's than radius + margin
    for (int k = 0; k < 3; k++) {
      const R half = s1[1] * fabs(u[k]), reach = s2[k] + s1[0] + margin;
      if (c0[k] - half > reach || c0[k] + half < -reach) return;
    }
    auto gfun = [&](R tt) { R acc = 0; for (int k = 0; k < 3; k++) { const R pk = c0[k] + tt * u[k]; acc += u[k] * (pk - clampr(pk, -s2[k], s2[k])); } return acc; };
    // Where the segment runs through the INSIDE of the box g is zero on a whole interval, and its computed value at the interval's ends
    // (a face crossing) is +-1 ulp with a rounding-dependent sign: values within eps of zero are therefore a set of their own.  If any
    // sample point (the two ends, the face crossings inside the segment) lies in it the answer is the point of that set's extent nearest
    // the capsule's centre (t = 0) — the root itself when it falls on a sample; only when no sample is numerically zero is the root
    // bracketed between the neighbouring samples and interpolated (the generic case; identical to the oracle's sequence).  (Not the
    // plateau's middle: entering through one face and leaving through the opposite one would tie the closest-face choice below.)
    const R L = s1[1], eps = sizeof(R) == 8 ? R(1e-12) : R(1e-6);
    R ta = -L, tb = L, ga = gfun(ta), gb = gfun(tb), ts;
    const R g_lo = ga, g_hi = gb;
    R z0 = R(1e30), z1 = R(-1e30);
    if (fabs(ga) <= eps) { z0 = ta; z1 = ta; }
    if (fabs(gb) <= eps) { if (tb < z0) z0 = tb; if (tb > z1) z1 = tb; }
    for (int k = 0; k < 3; k++) for (int sg = 0; sg < 2; sg++) {
      if (fabs(u[k]) <= R(1e-12)) continue;
      const R tc = ((sg ? s2[k] : -s2[k]) - c0[k]) / u[k];
      if (!(tc > -L && tc < L)) continue;
      const R gc = gfun(tc);
      if (fabs(gc) <= eps) { if (tc < z0) z0 = tc; if (tc > z1) z1 = tc; }
      else if (gc < 0) { if (tc > ta) { ta = tc; ga = gc; } }
      else { if (tc < tb) { tb = tc; gb = gc; } }
    }
    if (z0 <= z1) ts = z0 > 0 ? z0 : (z1 < 0 ? z1 : R(0));   // the point of the zero set nearest the capsule's centre
    else if (g_lo > 0) ts = -L;
    else if (g_hi < 0) ts = L;
    else ts = (gb - ga > R(1e-300)) ? ta - ga * (tb - ta) / (gb - ga) : R(0.5) * (ta + tb);
    R center[3], clamped[3], nrm[3], pl[3];
    for (int k = 0; k < 3; k++) { center[k] = c0[k] + ts * u[k]; clamped[k] = clampr(center[k], -s2[k], s2[k]); t[k] = center[k] - clamped[k]; }
    const R dist = sqrt(dot3(t, t));
    if (dist - s1[0] > margin) return;
    if (dist <= R(DM_MINVAL)) {
      R closest = 2 * fmax(s2[0], fmax(s2[1], s2[2]));
      int k = 0;
#pragma unroll
      for (int i = 0; i < 6; i++) { const R fd = fabs(((i % 2) ? R(1) : R(-1)) * s2[i / 2] - center[i / 2]); if (closest > fd) { closest = fd; k = i; } }
      nrm[0] = nrm[1] = nrm[2] = 0; nrm[k / 2] = (k % 2) ? R(-1) : R(1);
      const R sc = (s1[0] - closest) / 2;
      pl[0] = center[0] + nrm[0] * sc; pl[1] = center[1] + nrm[1] * sc; pl[2] = center[2] + nrm[2] * sc;
      pc.d0 = -closest - s1[0];
    } else {
      for (int i = 0; i < 3; i++) nrm[i] = -t[i] / dist;
      const R sc = s1[0] + R(0.5) * (dist - s1[0]);
      pl[0] = center[0] + nrm[0] * sc; pl[1] = center[1] + nrm[1] * sc; pl[2] = center[2] + nrm[2] * sc;
      pc.d0 = dist - s1[0];
    }
    pc.n = 1;
    mat_vec(pc.nrm, m2, nrm);
    mat_vec(pc.p0, m2, pl);
    pc.p0[0] += p2[0]; pc.p0[1] += p2[1]; pc.p0[2] += p2[2];
    return;
  }
  if (t1 == GEOM_BOX && t2 == GEOM_BOX) box_box(bx, p1, m1, gs1, p2, m2, gs2, stage_slot, margin, pc);
}
template <class R>
DM_DEV void narrowphase(Shared<R>& s, int g1, int g2, int t1, int t2, const R* s1, const R* s2, const R* gs1, const R* gs2, int stage_slot, R margin, PairContacts<R>& pc) {
  const BoxScratch<R> bx{s.ub.g.axes, s.ub.g.poly, s.boxc};
  narrowphase_at(bx, s.ub.g.gpos[g1], s.ub.g.gmat[g1], s.ub.g.gpos[g2], s.ub.g.gmat[g2], t1, t2, s1, s2, gs1, gs2, stage_slot, margin, pc);
}

// [MJ mju_makeFrame] rows of f: normal, tangent 1, tangent 2
template <class R>
DM_DEV void make_frame(R* f, const R* nrm, const R* hint) {
  f[0] = nrm[0]; f[1] = nrm[1]; f[2] = nrm[2];
  f[3] = hint[0]; f[4] = hint[1]; f[5] = hint[2];
  normalize3(f);
  if (sqrt(dot3(f + 3, f + 3)) < R(0.5)) {
    f[3] = f[4] = f[5] = 0;
    if (f[1] < R(0.5) && f[1] > R(-0.5)) f[4] = 1; else f[5] = 1;
  }
  const R dp = dot3(f, f + 3);
  f[3] -= f[0] * dp; f[4] -= f[1] * dp; f[5] -= f[2] * dp;
  normalize3(f + 3);
  cross3(f + 6, f, f + 3);
}

// constraint rows: joint limits first (joint order), then contacts (pair-list order)  [MJ mj_collision, mj_makeConstraint]
template <class R, int ROWS, bool PROF = false>
DM_DEV void stage_rows(const DevModel<R>& M, Shared<R>& s, int lane_in, long long* prof = 0) {
  const int lane = dmw::launder(lane_in);
  int nrow = 0;
  long long rt0 = 0, rt1 = 0;
  if (PROF) rt0 = dmw::clk();
#define DM_RSTAMP(k) if (PROF) { rt1 = dmw::clk(); prof[k] += rt1 - rt0; rt0 = rt1; }
  // this lane's two candidate pairs: issued here, consumed after the geom poses and the limit rows are done
  const int npair = dmw::uniform(M.npair);
  // (scalars, not a struct copy: the narrow phase indexes the sizes dynamically, which would pin a local struct in scratch)
  int pr = lane < npair ? lane : 0;
  int r_g1 = M.pair_rec[pr].g1, r_g2 = M.pair_rec[pr].g2, r_tt = M.pair_rec[pr].t1t2, r_meta = M.pair_rec[pr].meta;
  R r_margin = M.pair_rec[pr].margin, r_mu = M.pair_rec[pr].mu, r_bound = M.pair_rec[pr].bound, r_tran = M.pair_rec[pr].tran;
  R r_s1a = M.pair_rec[pr].s1[0], r_s1b = M.pair_rec[pr].s1[1], r_s1c = M.pair_rec[pr].s1[2];
  R r_s2a = M.pair_rec[pr].s2[0], r_s2b = M.pair_rec[pr].s2[1], r_s2c = M.pair_rec[pr].s2[2];
  // (joint-limit constants too: one exposed global-load latency for the stage instead of one per block)
  const bool lim_on = M.enable_limit && lane < NU && M.jnt_limited[lane < NU ? lane + 1 : 1];
  const R lim_lo = M.jnt_lo[lane < NU ? lane + 1 : 1], lim_hi = M.jnt_hi[lane < NU ? lane + 1 : 1];
  if (M.enable_contact) {   // (the inertia region these poses overwrite is dead by now)
    // geom world poses
    if (lane < NG) {
      const int g = lane, gb = M.geom_body[g];
      R v[3];
      mat_vec(v, s.xmat[gb], M.geom_pos[g]);
      s.ub.g.gpos[g][0] = s.xpos[gb][0] + v[0]; s.ub.g.gpos[g][1] = s.xpos[gb][1] + v[1]; s.ub.g.gpos[g][2] = s.xpos[gb][2] + v[2];
      const R* a = s.xmat[gb]; const R* bm = M.geom_mat[g];
      for (int i = 0; i < 3; i++) for (int jx = 0; jx < 3; jx++) s.ub.g.gmat[g][3 * i + jx] = a[3 * i] * bm[jx] + a[3 * i + 1] * bm[3 + jx] + a[3 * i + 2] * bm[6 + jx];
    }
  }
  dmw::sync();
  // ---- joint limits: hinge j = lane + 1, dof = lane + 6
  {
    bool viol = false;
    R dist = 0, sgn = 0;
    if (lim_on) {
      const R q = s.qpos[lane + 7];
      const R dlo = q - lim_lo, dhi = lim_hi - q;
      if (dlo < 0) { viol = true; dist = dlo; sgn = 1; }
      else if (dhi < 0) { viol = true; dist = dhi; sgn = -1; }
    }
    const unsigned long long mask = dmw::ballot(viol);
    if (viol) {
      const int r = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
      s.u.rowd[r][0] = sgn; s.u.rowd[r][6] = dist; s.u.rowd[r][7] = 0;
      s.u.rowd[r][8] = M.dof_invw[lane + 6]; s.u.rowd[r][9] = 1;
      s.rowi[r] = ROW_LIMIT | ((lane + 6) << 8);
    }
    nrow = __builtin_popcountll(mask);
  }
  DM_RSTAMP(16);
  // ---- contacts: lanes over candidate pairs, two passes of 64
  int ncon = 0, firstdrop = 1 << 20;
  if (M.enable_contact) {
    // (Measured dead ends, round 2: compacting the survivors of both passes onto lanes for ONE narrow-phase / emission trip takes 3 % off
    //  a lone wave's step — exposed latencies — and is 1 % SLOWER at two waves per SIMD, where those latencies were already covered
    //  and the two passes mostly run different geometry-type paths anyway; an oriented-bounding-box test behind the spheres cuts the
    //  pairs entering the narrow phase from 4.9 to 1.7 per evaluation and costs as much as it saves.)
    for (int pass = 0; pass * 64 < npair; pass++) {
      if (pass > 0) {
        pr = pass * 64 + lane < npair ? pass * 64 + lane : 0;
        r_g1 = M.pair_rec[pr].g1; r_g2 = M.pair_rec[pr].g2; r_tt = M.pair_rec[pr].t1t2; r_meta = M.pair_rec[pr].meta;
        r_margin = M.pair_rec[pr].margin; r_mu = M.pair_rec[pr].mu; r_bound = M.pair_rec[pr].bound; r_tran = M.pair_rec[pr].tran;
        r_s1a = M.pair_rec[pr].s1[0]; r_s1b = M.pair_rec[pr].s1[1]; r_s1c = M.pair_rec[pr].s1[2];
        r_s2a = M.pair_rec[pr].s2[0]; r_s2b = M.pair_rec[pr].s2[1]; r_s2c = M.pair_rec[pr].s2[2];
      }
      const int pidx = pass * 64 + lane;
      PairContacts<R> pc;
      pc.n = 0; pc.boxslot = -1;
      bool cand = false;
      const int g1 = r_g1, g2 = r_g2, t1 = r_tt & 0xff, t2 = (r_tt >> 8) & 0xff, dim = (r_tt >> 16) & 0xff;
      const R margin = r_margin, mu = r_mu;
      if (pidx < npair) {
        // bounding-sphere rejection (conservative; [MJ mj_collideGeoms] does the same before the narrow phase)
        if (t1 == GEOM_PLANE) {
          const R* m1 = s.ub.g.gmat[g1];
          const R dz = (s.ub.g.gpos[g2][0] - s.ub.g.gpos[g1][0]) * m1[2] + (s.ub.g.gpos[g2][1] - s.ub.g.gpos[g1][1]) * m1[5] + (s.ub.g.gpos[g2][2] - s.ub.g.gpos[g1][2]) * m1[8];
          cand = dz <= r_bound;
        } else {
          const R d[3] = {s.ub.g.gpos[g2][0] - s.ub.g.gpos[g1][0], s.ub.g.gpos[g2][1] - s.ub.g.gpos[g1][1], s.ub.g.gpos[g2][2] - s.ub.g.gpos[g1][2]};
          cand = dot3(d, d) <= r_bound * r_bound;
        }
      }
      DM_RSTAMP(17 + 3 * pass);
      if (dmw::ballot(cand) == 0ull) continue;        // nothing near anything in this pass (the common case for body-body pairs)
      if (PROF) { prof[24 + pass] += 1; prof[26 + pass] += __builtin_popcountll(dmw::ballot(cand)); }
      if (cand) {
        const R z1[3] = {r_s1a, r_s1b, r_s1c}, z2[3] = {r_s2a, r_s2b, r_s2c};
        narrowphase(s, g1, g2, t1, t2, z1, z2, M.pair_rec[pr].s1, M.pair_rec[pr].s2, ((r_meta >> 16) & 0xff) - 1, margin, pc);
      }
      DM_RSTAMP(18 + 3 * pass);
      if (dmw::ballot(pc.n > 0) == 0ull) continue;
      const int rows_per = dim == 1 ? 1 : 2 * (dim - 1);
      int tot_rows, tot_con;
      const int r0 = nrow + dmw::wave_exclusive_scan(pc.n * rows_per, lane, &tot_rows);
      const int c0 = ncon + dmw::wave_exclusive_scan(pc.n, lane, &tot_con);
      // Row emission, one row per lane.  The lanes that found contacts only STAGE them — position, distance, frame and pair
      // constants go into the contact's own (still empty) descriptor rows, a marker (row within the contact, condim, bodies)
      // into rowi — then lane L builds row nrow + L from the staged contact.  The work no longer grows with the number of
      // rows a single lane has to write (a foot on the floor: 4 corners x 4 pyramid rows from one lane).
      if (pc.n > 0) {
        R fr[9];
        make_frame(fr, pc.nrm, pc.hint);
        const int b1 = r_meta & 0xff, b2 = (r_meta >> 8) & 0xff;
        for (int k = 0; k < pc.n; k++) {
          R cdist, cpos[3];
          if (pc.boxslot >= 0) { const R* o = s.boxc[pc.boxslot][k]; cdist = o[0]; cpos[0] = o[1]; cpos[1] = o[2]; cpos[2] = o[3]; }
          else if (k == 0) { cdist = pc.d0; cpos[0] = pc.p0[0]; cpos[1] = pc.p0[1]; cpos[2] = pc.p0[2]; }
          else { cdist = pc.d1; cpos[0] = pc.p1[0]; cpos[1] = pc.p1[1]; cpos[2] = pc.p1[2]; }
          const int rk = r0 + k * rows_per;
          if (c0 + k < MAXEFC) { s.cong[c0 + k][0] = g1; s.cong[c0 + k][1] = g2; }
          // rows past the on-chip capacity are dropped contact-wise, in list order (status bit 0)
          if (rk + rows_per > MAXROWS) { if (rk < firstdrop) firstdrop = rk; continue; }
          R* st = s.u.rowd[rk];
          st[0] = cpos[0]; st[1] = cpos[1]; st[2] = cpos[2]; st[3] = fr[0]; st[4] = fr[1]; st[5] = fr[2];
          st[6] = cdist; st[7] = margin; st[8] = mu; st[9] = r_tran;
          if (dim != 1) { R* s2 = s.u.rowd[rk + 1]; for (int t = 0; t < 6; t++) s2[t] = fr[3 + t]; }
          const int mark = (1 << 30) | (dim << 4) | (b1 << 8) | (b2 << 16);
          for (int q = 0; q < rows_per; q++) s.rowi[rk + q] = mark | q;
        }
      }
      dmw::sync();
      {
        const int r = nrow + lane;
        const int code = (lane < tot_rows && r < MAXEFC) ? s.rowi[r] : 0;
        const bool mine = ((code >> 30) & 1) != 0;
        const int q = code & 15, cdim = (code >> 4) & 15;
        R st[10], tg[3] = {0, 0, 0};
        if (mine) {
          const R* b0 = s.u.rowd[r - q];
          for (int t = 0; t < 10; t++) st[t] = b0[t];
          if (cdim != 1) { const R* b1p = s.u.rowd[r - q + 1] + 3 * (q >> 1); tg[0] = b1p[0]; tg[1] = b1p[1]; tg[2] = b1p[2]; }
        }
        dmw::sync();                                // every lane has read its staged contact before the rows are overwritten
        if (mine) {
          const R cmu = st[8], ctran = st[9];
          R dir[3] = {st[3], st[4], st[5]};
          if (cdim != 1) { const R sg = (q & 1) ? -cmu : cmu; dir[0] += sg * tg[0]; dir[1] += sg * tg[1]; dir[2] += sg * tg[2]; }
          R* rd = s.u.rowd[r];
          cross3(rd, st, dir);
          rd[3] = dir[0]; rd[4] = dir[1]; rd[5] = dir[2];
          rd[6] = st[6]; rd[7] = st[7];
          rd[8] = cdim == 1 ? ctran : ctran + cmu * cmu * ctran;
          rd[9] = cdim == 1 ? R(1) : 2 * cmu * cmu;
          s.rowi[r] = ROW_CONTACT | (code & 0x00ffff00);
        }
      }
      nrow += tot_rows; ncon += tot_con;
      DM_RSTAMP(19 + 3 * pass);
    }
  }
  // first dropped row index over the wave (min), if any
  if (dmw::ballot(firstdrop < (1 << 20)) != 0ull) {      // only when some contact did not fit (six cross-lane round trips otherwise wasted)
    firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 32)); firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 16));
    firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 8));  firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 4));
    firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 2));  firstdrop = imin(firstdrop, dmw::shfl_xor_i(firstdrop, 1));
  }
  int status = 0;
  if (firstdrop < nrow) { status = 1; nrow = firstdrop; }
  if (lane == 0) { s.nefc = nrow; s.ncon = ncon; s.status |= status; }
  dmw::sync();
  DM_RSTAMP(23);
#undef DM_RSTAMP
}

// [MJ getimpedance]
// The model's solimp power is a per-model constant: for the default (2) the two pow() calls (a few hundred instructions
// each, evaluated by every lane) reduce to a square, and the constant denominators are reciprocals prepared on the host.
template <class R>
DM_DEV R impedance(const DevModel<R>& M, R x) {
  const R* si = M.solimp;
  if (si[0] == si[1] || si[2] <= R(DM_MINVAL)) return R(0.5) * (si[0] + si[1]);
  x = fabs(x / si[2]);
  if (x >= 1) return si[1];
  if (x <= 0) return si[0];
  R y;
  if (si[4] == R(1)) y = x;
  else if (si[4] == R(2)) y = (x <= si[3]) ? (x * x) * M.imp_rlo : 1 - ((1 - x) * (1 - x)) * M.imp_rhi;
  else if (x <= si[3]) y = pow_once(x, si[4]) / pow_once(si[3], si[4] - 1);
  else y = 1 - pow_once(1 - x, si[4]) / pow_once(1 - si[3], si[4] - 1);
  return si[0] + y * (si[1] - si[0]);
}

// x = L^-1 rhs for ONE vector, one dof per lane (rhs / result in lane d < NV), level by level down the tree:
//   x_i = rhs_i - sum_{j in anc(i)} L(i, j) x_j.
// When the dofs of depth l are final they publish x; every deeper lane then takes the term of ITS ancestor at depth l —
// one FMA per level and lane, 12 LDS hand-offs, instead of every lane redundantly running all 310 FMAs of the sparse
// solve on a private copy.  x is exchanged through the row-descriptor region (s.u, must be free), indexed by the
// ancestors' diagonal addresses that s.tab_dst already holds; terms are added root-first.
template <class R>
DM_DEV R lane_solve_L(Shared<R>& s, int lane_in, R rhs) {
  constexpr int MAXD = 13;
  static_assert([] { for (int d = 0; d < NV; d++) if (TOPO.dof_depth[d] > MAXD) return false; return true; }(), "dof chains are at most 13 deep");
  const int ll = dmw::launder(lane_in);
  const bool isdof = ll < NV;
  const int dd = isdof ? TOPO.dof_depth[ll] : 0;
  const unsigned short* td = &s.tab_dst[isdof ? ll : 0][0];
  const int own = td[0];
  R acc = rhs;
  R* xs = &s.u.rowd[0][0];
  int a = dd - 1;                               // my ancestor at depth l is my (dd - l)-th ancestor
  R La = s.qLD[own + (a > 0 ? a : 0)]; int xi = td[a > 0 ? a : 0];
#pragma unroll
  for (int l = 1; l < MAXD; l++) {
    xs[dd == l ? own : 576 + ll] = acc;         // branch-free (cells 576.. are per-lane scratch): a predicated region costs ~45 cycles (tools/ubench), a select ~8
    const int an = a - 1;                       // next level's operands do not depend on x: fetched ahead of the hand-off
    const R Ln = s.qLD[own + (an > 0 ? an : 0)]; const int xn = td[an > 0 ? an : 0];
    dmw::sync();
    const R term = La * xs[xi];
    acc -= a >= 1 ? term : R(0);
    a = an; La = Ln; xi = xn;
  }
  return acc;
}

// y = L^-T rhs for ONE vector, one dof per lane, level by level UP the tree:  y_j = rhs_j - sum_{i in desc(j)} L(i, j) y_i.
// Deepest dofs first: a dof whose descendants have all reported is final and pushes its term to every ancestor with
// fire-and-forget LDS atomics (several limbs report to the same ancestors in one step).  Same exchange buffer as above.
template <int L, class R>
struct PushLevel {
  static DM_DEV void run(R* xs, int own, int dd, const R* Lr, const int* xa) {
    if constexpr (L >= 2) {
      const bool on = dd == L;
      const R v = xs[on ? own : 0];
#pragma unroll
      for (int a = 1; a < L; a++) dmw::lds_sub(on, &xs[xa[a]], Lr[a] * v);
      dmw::sync();
      PushLevel<L - 1, R>::run(xs, own, dd, Lr, xa);
    }
  }
};
template <class R>
DM_DEV R lane_solve_LT(Shared<R>& s, int lane_in, R rhs) {
  constexpr int MAXD = 13;
  const int ll = dmw::launder(lane_in);
  const bool isdof = ll < NV;
  const int dd = isdof ? TOPO.dof_depth[ll] : 0;
  const unsigned short* td = &s.tab_dst[isdof ? ll : 0][0];
  const int own = td[0];
  R* xs = &s.u.rowd[0][0];
  R Lr[MAXD]; int xa[MAXD];
#pragma unroll
  for (int a = 1; a < MAXD; a++) { const bool on = a < dd; Lr[a] = s.qLD[own + (on ? a : 0)]; xa[a] = td[on ? a : 0]; }
  if (isdof) xs[own] = rhs;
  dmw::sync();
  PushLevel<MAXD, R>::run(xs, own, dd, Lr, xa);
  return isdof ? xs[own] : R(0);
}

// x <- M^-1 x for a vector held identically by every lane (uniform operands: no divergence, no reduction).
template <class R>
DM_DEV void uniform_solve(const Shared<R>& s, R* x) {
  solve_LT(x, s.qLD);
#pragma unroll
  for (int d = 0; d < NV; d++) x[d] *= s.dinv[d];
  solve_L(x, s.qLD);
}

// Jacobian row of one constraint, one dof per step, operands of the next dof prefetched (see solve_LT above).
template <class R>
struct RowAcc {
  // J_d = (w . cdof_d + w7 + w8 tau_d) * (plus_d - minus_d):
  //   contact row: w = the contact wrench direction, masks = ancestor chains of body2 (+) and body1 (-) — a dof that moves
  //                both bodies (common ancestor) cancels exactly;
  //   limit row:   w7 = +-1, plus mask = the one dof;      TAU_LANE (the smooth force rides along): w8 = 1, plus mask = all dofs.
  // One formula for all three kinds: an add and an FMA per dof instead of compares and selects.
  R w[6], w7, w8;
  unsigned plus_lo, plus_hi, minus_lo, minus_hi;
  R vel, jws;
};
template <int D, class R>
DM_DEV void load_dof_operands(R* dst, const Shared<R>& s, int z) {
  if constexpr (D < NV) {
#pragma unroll
    for (int r = 0; r < 6; r++) dst[r] = s.cdof[D + z][r];
    dst[6] = s.qvel[D + z]; dst[7] = s.ua.f.tau[D + z]; dst[8] = s.qws[D + z];
  }
}
template <int D, class R>
struct RowStep {
  static DM_DEV void run(R* y, RowAcc<R>& ra, const Shared<R>& s, const R* cur) {
    R nxt[9];
    dmw::reload_fence();
    load_dof_operands<D + 1>(nxt, s, 0);
    dmw::sched_fence();
    const int pb = (int)(D < 32 ? (ra.plus_lo >> D) & 1u : (ra.plus_hi >> (D - 32)) & 1u);
    const int mb = (int)(D < 32 ? (ra.minus_lo >> D) & 1u : (ra.minus_hi >> (D - 32)) & 1u);
    R j = ra.w[0] * cur[0] + ra.w[1] * cur[1] + ra.w[2] * cur[2] + ra.w[3] * cur[3] + ra.w[4] * cur[4] + ra.w[5] * cur[5];
    j = (j + ra.w7 + ra.w8 * cur[7]) * (R)(pb - mb);
    ra.vel += j * cur[6]; ra.jws += j * cur[8];
    y[D] = j;
    // pin both running sums: an unpinned one is sunk to the end of the loop by the optimiser, which keeps its 34
    // operands (loaded here) alive — and spilled — until then
    dmw::pin_value(ra.vel); dmw::pin_value(ra.jws);
    RowStep<D + 1, R>::run(y, ra, s, nxt);
  }
};
template <class R> struct RowStep<NV, R> { static DM_DEV void run(R*, RowAcc<R>&, const Shared<R>&, const R*) {} };

// dot(Y_lane, q) for a 34-vector q read at wave-uniform LDS addresses (broadcast), in chunks of 6 entries, double-buffered:
// the next chunk is loaded while the current one is multiplied (order pins: see solve_LT above).
template <class R>
DM_DEV R row_dot(const R* y, const R* q) {
  R acc0 = 0, acc1 = 0;      // two partial sums (even / odd chunks): halves the dependent-FMA chain of the 34-term dot product
  R qa[6], qb[6];
  dmw::reload_fence();
#pragma unroll
  for (int d = 0; d < 6; d++) qa[d] = q[d];
#pragma unroll
  for (int c0 = 0; c0 < NV; c0 += 12) {
    dmw::reload_fence();
#pragma unroll
    for (int d = 0; d < 6; d++) if (c0 + 6 + d < NV) qb[d] = q[c0 + 6 + d];
    dmw::sched_fence();
#pragma unroll
    for (int d = 0; d < 6; d++) if (c0 + d < NV) acc0 += y[c0 + d] * qa[d];
    dmw::pin_value(acc0);
    dmw::reload_fence();
#pragma unroll
    for (int d = 0; d < 6; d++) if (c0 + 12 + d < NV) qa[d] = q[c0 + 12 + d];
    dmw::sched_fence();
#pragma unroll
    for (int d = 0; d < 6; d++) if (c0 + 6 + d < NV) acc1 += y[c0 + 6 + d] * qb[d];
    dmw::pin_value(acc1);
  }
  return acc0 + acc1;
}

// PGS update of one row: f' = max(f - r / A_ii, 0)   [MJ mj_solPGS, scalar row], as the step
//   delta = f' - f = max(-f, t),   t = -r / A_ii.
// The solver carries the SCALED residual t_j = -r_j / A_jj (and the columns of A scaled the same way, row j by -1 / A_jj),
// so the row-to-row chain is: max, broadcast, fma — nothing else.

// ---- nested unrolling over constraint rows --------------------------------------------------------------------------
// nefc is small and wave-uniform, ROWS is the compile-time capacity.  A flat unrolled loop with one scalar test per row
// slot pays ~35 cycles for EVERY slot, taken or not; nesting the tests (slot I+1 is only reached through slot I) makes
// the cost proportional to nefc: one untaken branch per live slot and a single exit.
template <int I, int ROWS, class R>
struct ACol {        // column I of A = Y Y^T + diag(R); precondition: I < nefc
  static DM_DEV void run(R* AR, const R* y, Shared<R>& s, int lane, int nefc, R Rr, R& diag) {
    if constexpr (I < ROWS) {
      if constexpr (I % 16 == 0) {          // stage rows I .. I+15 of Y in the broadcast buffer
        dmw::sync();
        if ((lane >> 4) == I / 16) {
#pragma unroll
          for (int d = 0; d < NV; d++) s.u.ybuf[lane & 15][d] = y[d];
        }
        dmw::sync();
      }
      R acc = row_dot(y, s.u.ybuf[I % 16]);
      if (lane == I) { acc += Rr; diag = acc; }
      AR[I] = acc;
      if (I + 1 < nefc) ACol<I + 1, ROWS, R>::run(AR, y, s, lane, nefc, Rr, diag);
    }
  }
};
// A = Y Y^T + diag(R) for an evaluation with at most 16 rows (95 % of those with any), on the matrix core: the 16 x 34 block of Y
// goes through the broadcast buffer once, nine 16x16x4 MFMA blocks (both operands the same register: the product is symmetric)
// leave the 16 x 16 result spread over the wave, and a second trip through LDS hands lane r its row.  ~75 instructions whatever the
// row count, against 34 FMAs + 17 LDS reads PER COLUMN on the vector unit with a handful of its 64 lanes doing useful work.
// Rows past nefc have Y = 0, so their rows / columns of A come out as exact zeros, as the sweeps expect.
template <class R, int ROWS>
DM_DEV void a_block16(R* AR, const R* y, Shared<R>& s, int lane, bool active, R Rr, R& diag) {
  constexpr int LD = 18;                       // row stride of the result in LDS: 16-byte aligned rows, two-way bank conflicts at worst
  dmw::sync();
  if (lane < 16) {
#pragma unroll
    for (int d = 0; d < NV; d++) s.u.ybuf[lane][d] = y[d];
  }
  dmw::sync();
  R acc[4] = {0, 0, 0, 0};
  {
    const int i = lane & 15, k = lane >> 4;
    const R* src = &s.u.ybuf[i][k];
#pragma unroll
    for (int st = 0; st < 8; st++) { const R a = src[4 * st]; dmw::mfma_16x16x4(a, a, acc); }
    const R a = k < 2 ? src[32] : R(0);        // dofs 32, 33; the block's last two k are padding
    dmw::mfma_16x16x4(a, a, acc);
  }
  dmw::sync();                                 // every lane has read its operands: rows 0 .. 8 of the buffer become the result tile
  R* ab = &s.u.ybuf[0][0];
#pragma unroll
  for (int v = 0; v < 4; v++) ab[dmw::mfma_row(lane, v, R(0)) * LD + (lane & 15)] = acc[v];
  dmw::sync();
  const int r = lane & 15;
  if (active) { const R dg = ab[r * (LD + 1)] + Rr; diag = dg; ab[r * (LD + 1)] = dg; }
  dmw::sync();
#pragma unroll
  for (int j = 0; j < 16; j++) { AR[j] = lane < 16 ? ab[r * LD + j] : R(0); dmw::pin_value(AR[j]); }
#pragma unroll
  for (int j = 16; j < ROWS; j++) { AR[j] = 0; dmw::pin_value(AR[j]); }
}
template <int B, int ROWS, class R>
struct WarmBlock {   // A[:, 8B .. 8B+7] scaled in place (row j by -1 / A_jj);  t += A_scaled[:, 8B .. 8B+7] f   (slots past nefc: f = 0, zero column)
  static DM_DEV void run(R* AR, R& t, R f, R ndinv, int nefc) {
    if constexpr (B * 8 < ROWS) {
#pragma unroll
      for (int ii = 0; ii < 8; ii++) { const int i = B * 8 + ii; if (i < ROWS && i < MAXROWS) { AR[i] *= ndinv; t += AR[i] * dmw::bcast(f, i); } }
      if ((B + 1) * 8 < nefc) WarmBlock<B + 1, ROWS, R>::run(AR, t, f, ndinv, nefc);
    }
  }
};
// one row of the sweep.  With at most 16 rows (the instantiation chosen for 95 % of the solves) all rows sit in lanes 0..15 = DPP row 0, and the
// broadcast + multiply-add is ONE v_fmac_f64_dpp row_newbcast (round 3: the form the four-envs-per-wave kernel is built on) instead of two
// v_readlane and a fused multiply-add; the other rows' lanes read their own row's lane i, which holds an idle row (delta = 0).
template <int I, int ROWS, class R>
DM_DEV void sweep_row(const R* AR, R& t, R& tsave, R nf0, int ln) {
  if constexpr (I < ROWS && I < MAXROWS) {
    const R delta = dmw::max_raw(nf0, t);                    // every lane evaluates its own; only lane i's is used
    if (ln == I) tsave = t;
    // (round 3: one v_fmac_f64_dpp in inline assembly instead of two v_readlane and a multiply-add, 12.11 -> 12.24 M env-steps/s; round 5: the broadcast as a
    //  compiler-visible v_mov_b64_dpp + a plain multiply-add — one instruction more on the chain, but the scheduler sees the hazards and fills the slots that
    //  the opaque assembly block had to pad with three s_nop per row: 8 -> 6-7 instructions per row, 12.27 -> 12.38 M, gpurun call f7)
    if constexpr (ROWS <= 16) t += AR[I] * dmw::row_bcast<I & 15>(delta);
    else { const R di = dmw::bcast(delta, I); t += AR[I] * di; }
  }
}
template <int G, int ROWS, class R>
struct SweepGroup {  // PGS rows 4G .. 4G+3 (a slot past nefc computes delta = 0: idle lane, zero column)
  // strip / ndinv: rows past the register tier take their (unscaled) column of A from the env's memory strip; they hang off the
  // deepest level of the nest, so a sweep with fewer rows never even tests for them
  static DM_DEV void run(const R* AR, R& t, R& tsave, R nf0, int ln, int ne, const R* strip, R ndinv, const Shared<R>* sp) {
    if constexpr (G * 4 < ROWS) {
      sweep_row<G * 4, ROWS, R>(AR, t, tsave, nf0, ln); sweep_row<G * 4 + 1, ROWS, R>(AR, t, tsave, nf0, ln);
      sweep_row<G * 4 + 2, ROWS, R>(AR, t, tsave, nf0, ln); sweep_row<G * 4 + 3, ROWS, R>(AR, t, tsave, nf0, ln);
      if ((G + 1) * 4 < ne) SweepGroup<G + 1, ROWS, R>::run(AR, t, tsave, nf0, ln, ne, strip, ndinv, sp);
    } else if constexpr (ROWS < MAXEFC) {
      strip = sp->aovf;                                              // (the pointer is only fetched when such rows exist)
      for (int i = ROWS; i < ne; i++) {                              // overflow rows: same update, column of A from memory
        const R a = strip[i * 64 + ln] * ndinv;
        const R delta = dmw::max_raw(nf0, t);
        const R di = dmw::bcast(delta, i);
        if (ln == i) tsave = t;
        t += a * di;
      }
    }
  }
};

// constraint solve.  Lane r < nefc owns constraint row r (limits first, then contacts in list order).
//   [MJ mj_fwdAcceleration, mj_projectConstraint, mj_fwdConstraint (warmstart, mj_solPGS)]
template <class R, int ROWS, bool PROF = false>
DM_DEV void stage_constraint(const DevModel<R>& M, Shared<R>& s, int lane_in, const DebugOut* dbg, long long* prof = 0) {
  const int lane = dmw::launder(lane_in);
  long long pt0 = 0, pt1 = 0;
  if (PROF) pt0 = dmw::clk();
#define DM_STAMP(k) DM_MARK("constraint_" #k); if (PROF) { pt1 = dmw::clk(); prof[k] += pt1 - pt0; pt0 = pt1; }
  const int nefc = dmw::uniform(s.nefc);   // in an SGPR so that the row loops branch scalar
  const bool active = lane < nefc;
  const bool taul = lane == TAU_LANE;
  // With M = L^T D L and Y_r = D^-1/2 L^-T J_r^T (one row per lane), every product the solver needs is a dot product of
  // half-solved vectors:  A = Y Y^T + diag(R),  J qacc_smooth = Y z  with  z = D^-1/2 L^-T tau,  and
  //     qacc = M^-1 (tau + J^T f) = L^-1 D^-1/2 (z + sum_r f_r Y_r).
  // The smooth force tau rides through the rows' half solve in the spare lane TAU_LANE (no cost: the solve is SIMD over
  // lanes), so one evaluation costs one L^-T pass for all rows + tau and one L^-1 pass on the final vector; qacc_smooth
  // itself is only formed when there are no rows at all (or for the debug dump).
  if (lane == 0) s.solver_iter = 0;
  if (nefc == 0) {
    // qacc = qacc_smooth = L^-1 D^-1 L^-T tau, one dof per lane: up the tree, scale, down the tree (the row-descriptor
    // region the passes exchange the vector through is unused without rows)
    R mine = lane_solve_LT(s, lane, lane < NV ? s.ua.f.tau[lane] : R(0));
    if (lane < NV) mine *= s.dinv[lane];
    dmw::sync();
    const R acc = lane_solve_L(s, lane, mine);
    if (lane < NV) {
      s.ua.f.qaccs[lane] = acc; s.ua.f.qacc[lane] = acc;
      if (dbg) dbg->out[34 * 34 + 34 + lane] = (double)acc;
    }
    dmw::sync();
  } else if (dbg) {   // debug dump only: qacc_smooth next to a constrained solve
    R x[NV];
#pragma unroll
    for (int d = 0; d < NV; d++) x[d] = s.ua.f.tau[d];
    uniform_solve(s, x);
    dmw::sync();
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < NV; d++) { s.ua.f.qaccs[d] = x[d]; dbg->out[34 * 34 + 34 + d] = (double)x[d]; }
    }
    dmw::sync();
  }
  DM_STAMP(8)
  if (nefc == 0) return;

  // ---- this lane's row: Jacobian from the contact wrench, reference acceleration, warm-start force -----------------
  const int info = active ? s.rowi[lane] : 0;
  const int type = info & 0xff;
  int ldof = -1;
  R lsgn = 0;
  R Rr = 1, aref = 0, bb = 0, f = 0, pos = 0, margin = 0;
  R AR[ROWS];
  R diag = 1;
  R y[NV];     // stays live through the PGS sweeps: the final assembly needs f_r Y_r
  {
    R w[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long mplus = 0, mminus = 0;
    R dA = 0, rscale = 1;
    if (active) {
      const R* rd = s.u.rowd[lane];
      pos = rd[6]; margin = rd[7]; dA = rd[8]; rscale = rd[9];
      if (type == ROW_LIMIT) { ldof = (info >> 8) & 0xff; lsgn = rd[0]; mplus = 1ull << ldof; }
      else {
        for (int r = 0; r < 6; r++) w[r] = rd[r];
        mminus = TOPO.chain[(info >> 8) & 0xff]; mplus = TOPO.chain[(info >> 16) & 0xff];
      }
    }
    RowAcc<R> ra;
    for (int r = 0; r < 6; r++) ra.w[r] = w[r];
    ra.plus_lo = (unsigned)mplus; ra.plus_hi = (unsigned)(mplus >> 32); ra.minus_lo = (unsigned)mminus; ra.minus_hi = (unsigned)(mminus >> 32);
    ra.w7 = lsgn; ra.w8 = taul ? R(1) : R(0); ra.vel = 0; ra.jws = 0;
    if (taul) { ra.plus_lo = 0xffffffffu; ra.plus_hi = 0xffffffffu; }
    {
      R cur[9];
      dmw::reload_fence();
      load_dof_operands<0>(cur, s, 0);
      RowStep<0, R>::run(y, ra, s, cur);
    }
    const R vel = ra.vel, jws = ra.jws;
    if (dbg && active) {
      double* o = dbg->out + (34 * 34 + 34 * 3 + 42 + 3) + lane * (34 + 6);
#pragma unroll
      for (int d = 0; d < NV; d++) o[d] = (double)y[d];
    }
    DM_STAMP(9)
    const R imp = impedance(M, pos - margin);
    Rr = fmax(R(DM_MINVAL), (1 - imp) * dA / imp);
    if (rscale != R(1)) Rr = fmax(R(DM_MINVAL), rscale * Rr);
    aref = -M.B * vel - M.K * imp * (pos - margin);
    const R jar = jws - aref;
    f = (active && jar < 0) ? -jar / Rr : R(0);
    // half solve: y <- D^-1/2 L^-T y  (rows: J^T -> Y;  TAU_LANE: tau -> z)
    solve_LT(y, s.qLD);
#pragma unroll
    for (int d = 0; d < NV; d++) y[d] *= s.dsq[d];
    DM_STAMP(10)
    // z goes to the extra slot of the broadcast buffer (it aliases the row descriptors, which every lane has read by now)
    dmw::sync();
    if (taul) {
#pragma unroll
      for (int d = 0; d < NV; d++) s.u.ybuf[16][d] = y[d];
    }
    dmw::sync();
    bb = active ? row_dot(y, s.u.ybuf[16]) - aref : R(0);     // b = J qacc_smooth - aref
    // overflow tier first (while AR is not live yet): columns ROWS.. of A do not fit the register budget of this
    // instantiation; they go to a per-env global-memory strip [col][lane] that only this lane ever reads back
    // (rare: < 1% of evaluations).
    if (ROWS < MAXEFC && nefc > ROWS) {
      R* const aov = (&s.aovf)[dmw::pin_zero()];      // (re-read where needed: a live pointer would cost registers on the hot path)
      for (int c = ROWS / 16; c * 16 < nefc; c++) {
        dmw::sync();
        if ((lane >> 4) == c) {
#pragma unroll
          for (int d = 0; d < NV; d++) s.u.ybuf[lane & 15][d] = y[d];
        }
        dmw::sync();
        for (int ii = 0; ii < 16; ii++) {
          const int i = c * 16 + ii;
          if (i < ROWS || i >= nefc) continue;
          R acc = row_dot(y, s.u.ybuf[ii]);        // same arithmetic as the register columns
          if (lane == i) { acc += Rr; diag = acc; }
          aov[i * 64 + lane] = acc;
        }
      }
    }
    // ---- A = Y Y^T + diag(R): rows of Y broadcast through LDS, 16 at a time ---------------------------------
    // columns past nefc are exact zeros (the row groups of the sweeps may touch them); zeroed here, not earlier, so that
    // the array is not live during the row build and the half solve
    if (nefc <= 16) a_block16<R, ROWS>(AR, y, s, lane, active, Rr, diag);
    else {
#pragma unroll
      for (int i = 0; i < ROWS; i++) { AR[i] = 0; dmw::pin_value(AR[i]); }   // (opaque zeros stay in their registers: as known constants
      ACol<0, ROWS, R>::run(AR, y, s, lane, nefc, Rr, diag);              //  they would be re-materialised before every early-exit test)
    }
  }
  const R dinvr = R(1) / diag;
  DM_STAMP(11)
  // ---- warm start: keep f(qacc_warmstart) only if its dual cost beats f = 0 ------------------------------------
  // (zero for a lane without a row — TAU_LANE included, whose "row of A" is a by-product of the build: its scaled residual and
  //  columns are then exact zeros, and the sweeps need no predicate to keep it at f = 0)
  R ndinv = active ? -dinvr : R(0);
  dmw::pin_value(ndinv);
  const R tb = bb * ndinv;
  R t = tb;    // scaled residual t_j = -(b_j + sum_i A_ji f_i) / A_jj, maintained incrementally; the columns are scaled on the way
  // (rows are taken in unguarded groups: a scalar branch costs as much as ~4 rows of work, and a row slot past nefc is
  //  harmless — its lane is idle with f = 0, and its column of A is zero)
  WarmBlock<0, ROWS, R>::run(AR, t, f, ndinv, nefc);
  if (ROWS < MAXEFC && nefc > ROWS) {
    const R* const aov = (&s.aovf)[dmw::pin_zero()];
    for (int i = ROWS; i < nefc; i++) t += (aov[i * 64 + lane] * ndinv) * dmw::bcast(f, i);     // (strip columns stay unscaled)
  }
  {
    const R res = -t * diag;                      // the residual itself, for the dual cost
    const R cost = dmw::wave_sum(active ? f * (R(0.5) * (res - bb) + bb) : R(0));
    if (cost > 0) { f = 0; t = tb; }
  }
  // ---- projected Gauss-Seidel, rows in order; one broadcast + one FMA per row, no memory ------------------------
  // Row i only ever needs lane i's force, and lane i's force only changes at row i, so a sweep leaves f alone: each row costs
  // the serial chain (delta = max(-f, t) -> broadcast -> scaled-residual update) plus one select that records the residual
  // lane i saw at its own row; forces and cost changes follow once per sweep, lane-wise, from exactly the operands the row-by-row
  // form would have used.
  // [MJ costChange] rejects an update that would raise the dual cost by more than 1e-10.  In exact arithmetic the
  // one-dimensional step never raises it, so the sweeps run without the test; if any row of any sweep did trip it
  // (`anybad`), the whole solve is redone from the warm-start state with the in-place guarded update (cold path below) —
  // results are identical to testing every row in place.
  // The termination test of sweep k (a 6-stage cross-lane reduction + compare) is independent of the rows of sweep k + 1,
  // so sweep k + 1 is issued speculatively right behind the reduction and dropped if sweep k turns out to have converged:
  // one discarded sweep per solve buys the reduction latency off the serial chain of every sweep.
  // (Round 2 measured the generalisation — blocks of K = 2 / 3 / 4 sweeps whose K tests run beside the next block's K speculative sweeps,
  //  the state after every sweep kept for the roll-back; bit-identical results — at 11.54 / 11.39 / 11.35 M env-steps/s against 11.65 M:
  //  with two waves per SIMD the partner wave already fills this chain's stalls, so the extra discarded sweeps only add instructions.)
  // (Also measured: lane i's `tsave = t` as a v_mov under EXEC = 1 << i (two scalar instructions around one move) instead of the compare and
  //  the two selects: two vector instructions fewer per row and 1.3 % SLOWER — 11.65 / 11.67 against 11.80 / 11.84 M; an EXEC write costs the
  //  vector pipe more than the selects; the lane mask made by the scalar unit (s_lshl_b64) feeding the two selects, no v_cmp: 11.69 M — the
  //  scalar-write -> mask-read hazard puts a wait state in front of every select.)
  int iter = 0;
  const int maxiter = dmw::uniform(M.iterations);
  // loop constants pinned in VGPRs: left to itself the compiler re-loads them from memory (s_load + wait) every sweep
  R pgs_scale = M.pgs_scale, pgs_tol = M.tolerance;
  dmw::pin_value(pgs_scale); dmw::pin_value(pgs_tol);
  R pgs_detect = M.pgs_detect;
  dmw::pin_value(pgs_detect);
  const R f_ws = f, t_ws = t;
  bool anybad = false;
  // Two instantiations of the sweep loop, chosen once per solve: with at most 16 rows (95 % of the solves) the row nest stops at four
  // groups and the improvement of a sweep is lane 0's 16-lane sum alone — rows 16.. hold exact zeros, so the value is the wave sum's
  // to the bit, without the three cross-row broadcasts and additions of every sweep's termination test.
  auto solve = [&](auto small_tag) {
    constexpr bool SMALL = decltype(small_tag)::value;
    constexpr int NEST = SMALL ? (ROWS < 16 ? ROWS : 16) : ROWS;
    auto sweep = [&](R& myimp) {
      // fresh opaque copies per sweep: otherwise the 64 row-exists tests and 64 lane==row masks are hoisted out of the
      // sweep loop as 128 SGPR pairs, spilled to VGPR lanes and read back with v_readlane on every row
      const int ne = dmw::launder_uniform(nefc);
      const int ln = dmw::launder(lane);
      const R f0 = f, nf0 = -f;
      R tsave = t;
      SweepGroup<0, NEST, R>::run(AR, t, tsave, nf0, ln, ne, (const R*)0, ndinv, &s);
      {   // every lane, unpredicated: a lane without a row has f = 0 and t = 0 throughout, so its step, its new force and its
          // cost change are exact zeros (a branch around this block costs more than the block)
        const R delta = dmw::max_raw(nf0, tsave);
        const R fn = f0 + delta;
        const R change = (delta * diag) * (R(0.5) * delta - tsave);      // = delta (delta A_ii / 2 + r)
        f = fn; myimp = -change; anybad = anybad || (change > pgs_detect);
      }
    };
    R myimp;
    sweep(myimp);
    iter = 1;
    bool more = iter < maxiter, conv = false;
    R fprev = f, tprev = t;
    while (more) {                                                                  // (one exit test per sweep)
      fprev = f; tprev = t;
      const R total = SMALL ? dmw::bcast(dmw::sum16(myimp), 0) : dmw::wave_sum(myimp);   // of sweep `iter` (idle lanes hold 0)
      const R improvement = total * pgs_scale;
      R myimp_next;
      sweep(myimp_next);                                                          // sweep iter + 1, speculative
      conv = dmw::uniform(improvement < pgs_tol);
      myimp = myimp_next;
      iter += 1;
      more = !conv && iter < maxiter;
    }
    if (conv) { f = fprev; t = tprev; iter -= 1; }                                  // converged: the speculative sweep is dropped (once, after the loop)
  };
  if (maxiter > 0) {
    if (nefc <= 16) solve(std::true_type{}); else solve(std::false_type{});
  }
  if (dmw::ballot(anybad) != 0) {
    // guarded re-solve (cold): the (scaled) register columns are parked in the env's memory strip so that one compact loop
    // can walk all rows with a run-time index; the strip's own columns (rows past the register tier) are unscaled
    R* const strip = (&s.aovf)[dmw::pin_zero()];
#pragma unroll
    for (int i = 0; i < ROWS; i++) strip[i * 64 + lane] = AR[i];
    f = f_ws; t = t_ws; iter = 0;
    while (iter < maxiter) {
      R myimp = 0;
      for (int i = 0; i < nefc; i++) {
        R a = strip[i * 64 + lane];
        if (i >= ROWS) a *= ndinv;
        R delta = dmw::max_raw(-f, t);
        const R fn = f + delta;
        const R change = (delta * diag) * (R(0.5) * delta - t);
        const bool rej = change > R(1e-10);          // never accept an increase
        if (rej) delta = 0;
        const R di = dmw::bcast(delta, i);
        if (lane == i && !rej) { f = fn; myimp -= change; }
        t += a * di;
      }
      const R improvement = dmw::wave_sum(active ? myimp : R(0)) * pgs_scale;
      iter++;
      if (dmw::uniform(improvement < pgs_tol)) break;
    }
  }
  DM_STAMP(12)
  if (dbg && active) {
    double* o = dbg->out + (34 * 34 + 34 * 3 + 42 + 3) + lane * (34 + 6) + 34;
    o[0] = (double)pos; o[1] = (double)margin; o[2] = (double)Rr; o[3] = (double)aref; o[4] = (double)bb; o[5] = (double)f;
  }
  // ---- qacc = L^-1 D^-1/2 (z + sum_r f_r Y_r): the scaled rows are summed through the broadcast buffer, 16 at a time
  // (lane d < NV owns component d; idle lanes carry f = 0 and add nothing), z is still in its slot ------------------
  R wsum = 0;
  for (int c = 0; c * 16 < nefc; c++) {
    dmw::sync();
    if ((lane >> 4) == c) {
#pragma unroll
      for (int d = 0; d < NV; d++) s.u.ybuf[lane & 15][d] = f * y[d];
    }
    dmw::sync();
    if (lane < NV) {
#pragma unroll
      for (int k = 0; k < 16; k++) wsum += s.u.ybuf[k][lane];
    }
  }
  {
    const R rhs = lane < NV ? (wsum + s.u.ybuf[16][lane]) * s.dsq[lane] : R(0);
    dmw::sync();                                  // every lane has read z (ybuf slot 16): the region becomes the solve's exchange buffer
    const R acc = lane_solve_L(s, lane, rhs);
    if (lane < NV) s.ua.f.qacc[lane] = acc;
    if (lane == 0) s.solver_iter = iter;
  }
  dmw::sync();
  DM_STAMP(13)
#undef DM_STAMP
}

// one forward-dynamics evaluation: s.qpos, s.qvel, s.act, s.qws  ->  s.ua.f.qacc (+ s.xipos, contact bookkeeping)
// PROF: accumulate shader-clock cycles per stage into prof[0..4] (profiling kernel only).
template <class R, int ROWS = MAXEFC, bool PROF = false>
DM_DEV void forward(const DevModel<R>& M, Shared<R>& s, int lane, const LaneTopo& lt, const DebugOut* dbg, long long* prof = 0, bool kin = false) {
  long long t0 = 0, t1 = 0;
  if (PROF) t0 = dmw::clk();
  DM_MARK("kinematics");
  if (!kin) stage_kinematics(M, s, lane, lt);   // (kin: this state's kinematics are already in LDS — env_step.h load_kin)
  if (PROF) { t1 = dmw::clk(); prof[0] += t1 - t0; t0 = t1; }
  if (dbg) { for (int e = lane; e < NV * NV; e += 64) dbg->out[e] = 0; dmw::sync(); }
  DM_MARK("mass_factor");
  stage_mass_matrix(M, s, lane, lt, dbg);
  if (PROF) { t1 = dmw::clk(); prof[1] += t1 - t0; t0 = t1; }
  DM_MARK("bias");
  stage_bias(M, s, lane, lt);
  if (PROF) { t1 = dmw::clk(); prof[2] += t1 - t0; t0 = t1; }
  if (dbg && lane < NV) {
    const double bias = (double)(-M.dof_damping[lane] * s.qvel[lane] + s.act[lane] - s.ua.f.tau[lane]);
    dbg->out[34 * 34 + lane] = bias;
  }
  DM_MARK("rows");
  if (M.enable_contact || M.enable_limit) stage_rows<R, ROWS, PROF>(M, s, lane, prof);
  else { if (lane == 0) { s.nefc = 0; s.ncon = 0; } dmw::sync(); }      // contact-free, limit-free model: no row can exist
  if (PROF) { t1 = dmw::clk(); prof[3] += t1 - t0; t0 = t1; }
  DM_MARK("constraint");
  stage_constraint<R, ROWS, PROF>(M, s, lane, dbg, prof);
  DM_MARK("forward_end");
  if (PROF) { t1 = dmw::clk(); prof[4] += t1 - t0; t0 = t1; }
  if (dbg) {
    if (lane < NV) dbg->out[34 * 34 + 68 + lane] = (double)s.ua.f.qacc[lane];
    if (lane < NB * 3) dbg->out[34 * 34 + 102 + lane] = (double)s.xipos[lane / 3][lane % 3];
    if (lane == 0) { dbg->out[34 * 34 + 144] = s.nefc; dbg->out[34 * 34 + 145] = s.ncon; dbg->out[34 * 34 + 146] = s.solver_iter; }
  }
}

}  // namespace dm
