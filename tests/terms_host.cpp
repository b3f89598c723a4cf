// Host build of the imitation reward's lane code (csrc/env_step.h imitation_reward<R, true>, what csrc/terms_kernel.h launches) for
// tests/test_imitation_terms.py: the unmodified kernel source on the fibre wave testbench (tests/emu/wave_testbench.h), one wave per state,
// wrapped as k_imitation_terms wraps it.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: terms_host in.bin out.bin [32]     ("32": the arithmetic in float, as libdmenv32.so computes; default double)
//   in.bin (float64): n, F | body_pos [14,3], body_ipos [14,3], body_mass [14], body_inertia [14,9], jnt_axis [29,3] (the model constants the
//   kinematics and the reward read) | params [32] | table [F,112] | n x { qpos [35], qvel [34], frame, cycle }
//   out.bin: [n, 28] float64; a frame outside [0, F) gives a row of NaNs, as on the device
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wave_testbench.h"
namespace dmw {
// the testbench has wave.h's sums in double only; the float build adds in float in the device's butterfly order (wave.h sum16 / wave_sum)
inline float wave_sum(float v) {
  v += exchange(v, lane() ^ 1); v += exchange(v, lane() ^ 2);
  { const int l = lane(); v += exchange(v, (l & ~7) | (7 - (l & 7))); }
  { const int l = lane(); v += exchange(v, (l & ~15) | (15 - (l & 15))); }
  return ((bcast(v, 0) + bcast(v, 16)) + bcast(v, 32)) + bcast(v, 48);
}
}  // namespace dmw
// kernel source, unmodified
#include "env_step.h"

#include "wave_fibres.h"      // the fibre runner: dmw::bench(), run_wave

namespace {
using namespace dm;

template <class R>
int run(const std::vector<double>& in, const char* fout) {
  const int n = (int)in[0], F = (int)in[1];
  const double* p = in.data() + 2;
  const size_t need = 2 + 42 + 42 + 14 + 126 + 87 + 32 + (size_t)F * IMIT_FEAT + (size_t)n * (NQ + NV + 2);
  if (n < 1 || F < 1 || in.size() != need) { std::fprintf(stderr, "terms_host: bad input (%zu doubles, want %zu)\n", in.size(), need); return 1; }
  static DevModel<R> M;
  static Batch<R> B;
  static Shared<R> s;
  static R row[IMIT_NTERMS];
  double tm = 0;
  for (int b = 0; b < NB; b++) for (int k = 0; k < 3; k++) M.body_pos[b][k] = (R)p[3 * b + k];
  p += 42;
  for (int b = 0; b < NB; b++) for (int k = 0; k < 3; k++) M.body_ipos[b][k] = (R)p[3 * b + k];
  p += 42;
  for (int b = 0; b < NB; b++) { M.body_mass[b] = (R)p[b]; tm += p[b]; }
  p += 14;
  for (int b = 0; b < NB; b++) {                     // as model_host.h build_dev_model packs the symmetric tensor
    const double* I = p + 9 * b;
    M.body_inertia[b][0] = (R)I[0]; M.body_inertia[b][1] = (R)I[4]; M.body_inertia[b][2] = (R)I[8];
    M.body_inertia[b][3] = (R)I[1]; M.body_inertia[b][4] = (R)I[2]; M.body_inertia[b][5] = (R)I[5];
  }
  p += 126;
  for (int j = 0; j < NJ; j++) for (int k = 0; k < 3; k++) M.jnt_axis[j][k] = (R)p[3 * j + k];
  p += 87;
  M.qpos0[0] = M.body_pos[1][0]; M.qpos0[1] = M.body_pos[1][1]; M.qpos0[2] = M.body_pos[1][2]; M.qpos0[3] = 1;
  M.total_mass = (R)tm;
  for (int k = 0; k < 32; k++) B.imit_params[k] = (R)p[k];
  p += 32;
  std::vector<R> table((size_t)F * IMIT_FEAT);
  for (size_t i = 0; i < table.size(); i++) table[i] = (R)p[i];
  p += table.size();
  B.imit_pdev = B.imit_params; B.imit_table = table.data(); B.n_frames = F;
  std::vector<double> out((size_t)n * IMIT_NTERMS);
  for (int v = 0; v < n; v++, p += NQ + NV + 2) {
    const double* qpos = p; const double* qvel = p + NQ;
    const int k = (int)p[NQ + NV], cyc = (int)p[NQ + NV + 1];
    const bool inside = k >= 0 && k < F;
    run_wave([&](int lane) {
      if (lane < NQ) s.qpos[lane] = (R)qpos[lane];
      if (lane < NV) s.qvel[lane] = (R)qvel[lane];
      dmw::sync();
      imitation_reward<R, true>(M, B, s, lane, lane_topo(lane), B.imit_table + (size_t)(inside ? k : 0) * IMIT_FEAT, cyc * B.imit_params[13], cyc * B.imit_params[14], row);
      dmw::sync();
      if (lane < IMIT_NTERMS) out[(size_t)v * IMIT_NTERMS + lane] = inside ? (double)row[lane] : (double)NAN;
    });
  }
  FILE* f = std::fopen(fout, "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::fprintf(stderr, "terms_host: cannot write %s\n", fout); return 1; }
  std::fclose(f);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: terms_host in.bin out.bin [32]\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "terms_host: cannot read %s\n", argv[1]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double));
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size() || in.size() < 2) { std::fprintf(stderr, "terms_host: short read\n"); return 1; }
  std::fclose(f);
  const bool f32 = argc > 3 && std::atoi(argv[3]) == 32;
  return f32 ? run<float>(in, argv[2]) : run<double>(in, argv[2]);
}
