// Host build of csrc/floor_contact.h for tests/test_termination.py: the floor-contact decision the termination kernels make per geom,
// compiled with a host C++ compiler and evaluated on body frames the test supplies, so that it can be checked against the float64
// restatement (tests/floor_numpy.py) without a GPU.  Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: floor_host IN OUT [32]
//   IN  float64 values: nstates, then the model's geom tables: geom_body [16], geom_type [16], geom_pos [16][3], geom_mat [16][9],
//       geom_size [16][3], geom_margin [16]; then per state: xpos [14][3], xmat [14][9]
//   OUT per state: one float64 value, the bit mask (bit g: geom g touches the floor).  With "32" the arithmetic runs in float (the float32
//       library's), inputs rounded to float first.
#include <cstdio>
#include <cstring>
#include <vector>

#include "floor_contact.h"
#include "topology.h"

static constexpr int NG = dmt::NG, NB = dmt::NB;
static constexpr size_t MODEL = NG * (1 + 1 + 3 + 9 + 3 + 1), PER = NB * 12;

template <class R>
static void run(const double* model, const double* states, size_t n, double* out) {
  int body[NG], type[NG];
  R gpos[NG][3], gmat[NG][9], gsize[NG][3], gmargin[NG];
  size_t p = 0;
  for (int g = 0; g < NG; g++) body[g] = (int)model[p++];
  for (int g = 0; g < NG; g++) type[g] = (int)model[p++];
  for (int g = 0; g < NG; g++) for (int k = 0; k < 3; k++) gpos[g][k] = (R)model[p++];
  for (int g = 0; g < NG; g++) for (int k = 0; k < 9; k++) gmat[g][k] = (R)model[p++];
  for (int g = 0; g < NG; g++) for (int k = 0; k < 3; k++) gsize[g][k] = (R)model[p++];
  for (int g = 0; g < NG; g++) gmargin[g] = (R)model[p++];
  for (size_t i = 0; i < n; i++) {
    R xpos[NB][3], xmat[NB][9];
    const double* in = states + i * PER;
    size_t q = 0;
    for (int b = 0; b < NB; b++) for (int k = 0; k < 3; k++) xpos[b][k] = (R)in[q++];
    for (int b = 0; b < NB; b++) for (int k = 0; k < 9; k++) xmat[b][k] = (R)in[q++];
    unsigned m = 0;
    for (int g = 1; g < NG; g++) if (dmfc::geom_touches_floor(g, body, type, gpos, gmat, gsize, gmargin, xpos, xmat)) m |= 1u << g;
    out[i] = (double)m;
  }
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: floor_host IN OUT [32]\n"); return 2; }
  const bool f32 = argc == 4 && std::strcmp(argv[3], "32") == 0;
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  std::vector<double> in;
  double x;
  while (std::fread(&x, sizeof x, 1, fi) == 1) in.push_back(x);
  std::fclose(fi);
  const size_t n = (size_t)in.at(0);
  if (in.size() != 1 + MODEL + n * PER) { std::fprintf(stderr, "input size does not match the state count\n"); return 2; }
  std::vector<double> out(n);
  if (f32) run<float>(&in[1], &in[1 + MODEL], n, out.data());
  else run<double>(&in[1], &in[1 + MODEL], n, out.data());
  std::fwrite(out.data(), sizeof(double), out.size(), fo);
  std::fclose(fo);
  return 0;
}
