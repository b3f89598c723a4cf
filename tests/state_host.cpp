// Host build of csrc/state_features.h for tests/test_state_features.py: the features kernel's own per-body arithmetic, compiled with a
// host C++ compiler, evaluated on kinematics the test supplies, so that it can be checked against the float64 restatement without a
// GPU.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: state_host IN OUT [32]
//   IN  float64 values: nstates, then per state: xpos [14][3], xquat [14][4], xipos [14][3], world dof axes [34][3], qvel [34], phase
//   OUT per state: 171 float64 values.  With "32" the arithmetic runs in float (the float32 library's), inputs rounded to float first.
#include <cstdio>
#include <cstring>
#include <vector>

#include "state_features.h"

static constexpr dmt::Topo TOPO = dmt::make_topo();

template <class R>
static void run(const double* in, double* out) {
  R xpos[dmt::NB][3], xquat[dmt::NB][4], xipos[dmt::NB][3], axis[dmt::NV][3], qvel[dmt::NV], row[dmsf::NSTATE];
  size_t p = 0;
  for (int b = 0; b < dmt::NB; b++) for (int k = 0; k < 3; k++) xpos[b][k] = (R)in[p++];
  for (int b = 0; b < dmt::NB; b++) for (int k = 0; k < 4; k++) xquat[b][k] = (R)in[p++];
  for (int b = 0; b < dmt::NB; b++) for (int k = 0; k < 3; k++) xipos[b][k] = (R)in[p++];
  for (int d = 0; d < dmt::NV; d++) for (int k = 0; k < 3; k++) axis[d][k] = (R)in[p++];
  for (int d = 0; d < dmt::NV; d++) qvel[d] = (R)in[p++];
  const double phase = in[p++];
  const dmsf::Heading<R> h = dmsf::heading(xquat[1]);
  for (int b = 1; b < dmt::NB; b++) dmsf::body_features(TOPO, h, b, xpos, xquat, xipos, &axis[0][0], 3, qvel, row);
  row[dmsf::O_HEIGHT] = xpos[1][2];
  for (int k = 0; k < dmsf::NSTATE; k++) out[k] = k == dmsf::O_PHASE ? phase : (double)row[k];
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: state_host IN OUT [32]\n"); return 2; }
  const bool f32 = argc == 4 && std::strcmp(argv[3], "32") == 0;
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  std::vector<double> in;
  double x;
  while (std::fread(&x, sizeof x, 1, fi) == 1) in.push_back(x);
  std::fclose(fi);
  const size_t per = dmt::NB * 10 + dmt::NV * 4 + 1;
  const size_t n = (size_t)in.at(0);
  if (in.size() != 1 + n * per) { std::fprintf(stderr, "input size does not match the state count\n"); return 2; }
  std::vector<double> out(n * dmsf::NSTATE);
  for (size_t i = 0; i < n; i++) {
    if (f32) run<float>(&in[1 + i * per], &out[i * dmsf::NSTATE]);
    else run<double>(&in[1 + i * per], &out[i * dmsf::NSTATE]);
  }
  std::fwrite(out.data(), sizeof(double), out.size(), fo);
  std::fclose(fo);
  return 0;
}
