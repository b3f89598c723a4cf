// Host build of csrc/render.h for tests/test_render.py: the ray caster's own per-pixel math, compiled with a host C++
// compiler, renders views described by the test so that it can be checked against the float64 restatement without a GPU.
// Test infrastructure only (libdmenv.so has no CPU path).
//
// usage: render_host IN OUT
//   IN  float64 values: nviews, then per view: width, height, camera position (world) [3], cam_mat [9], fovy, geom_rgb [16][3],
//       floor_rgb1 [3], floor_rgb2 [3], floor_square, sky_top [3], sky_bottom [3], light_dir [3], ambient, headlight, diffuse,
//       floor half sizes [2], centre of mass [3], then per geom 0..15: type, world position [3], row-major rotation [9], size [3]
//   OUT per view: rgb uint8 [H,W,3], depth float32 [H,W], segmentation int32 [H,W]
#include <cstdio>
#include <cstdint>
#include <vector>

#include "render.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: render_host IN OUT\n"); return 2; }
  std::FILE* fi = std::fopen(argv[1], "rb");
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fi || !fo) { std::fprintf(stderr, "cannot open files\n"); return 2; }
  std::vector<double> in;
  double x;
  while (std::fread(&x, sizeof x, 1, fi) == 1) in.push_back(x);
  std::fclose(fi);
  size_t p = 0;
  auto take = [&](double* dst, int n) { for (int k = 0; k < n; k++) dst[k] = in.at(p++); };
  const int nviews = (int)in.at(p++);
  for (int view = 0; view < nviews; view++) {
    dm_render_desc d{};
    double wh[2], cam[3], floor_half[2], com[3];
    take(wh, 2); d.width = (int32_t)wh[0]; d.height = (int32_t)wh[1];
    take(cam, 3); take(d.cam_mat, 9); take(&d.fovy, 1);
    take(&d.geom_rgb[0][0], 48); take(d.floor_rgb1, 3); take(d.floor_rgb2, 3); take(&d.floor_square, 1);
    take(d.sky_top, 3); take(d.sky_bottom, 3); take(d.light_dir, 3); take(&d.ambient, 1); take(&d.headlight, 1); take(&d.diffuse, 1);
    take(floor_half, 2); take(com, 3);
    dmr::ViewRec v{};
    for (int g = 0; g < dmr::NG; g++) {
      double type, pos[3], mat[9], size[3];
      take(&type, 1); take(pos, 3); take(mat, 9); take(size, 3);
      if (g > 0) dmr::fill_geom(v.g[g - 1], (int)type, pos, mat, size, cam);
    }
    dmr::set_camera(v, d.cam_mat, cam, floor_half);
    const float centre[3] = {(float)(com[0] - cam[0]), (float)(com[1] - cam[1]), (float)(com[2] - cam[2])};
    dmr::finish_bound(v, centre);
    const dmr::Params P = dmr::make_params(d);
    const size_t npx = (size_t)d.width * d.height;
    std::vector<unsigned char> rgb(npx * 3);
    std::vector<float> depth(npx);
    std::vector<int32_t> seg(npx);
    for (int r = 0; r < d.height; r++)
      for (int c = 0; c < d.width; c++) {
        const dmr::Pixel px = dmr::shade_pixel(v, P, r, c);
        const size_t i = (size_t)r * d.width + c;
        for (int k = 0; k < 3; k++) rgb[3 * i + k] = px.rgb[k];
        depth[i] = px.depth; seg[i] = px.seg;
      }
    std::fwrite(rgb.data(), 1, rgb.size(), fo);
    std::fwrite(depth.data(), sizeof(float), depth.size(), fo);
    std::fwrite(seg.data(), sizeof(int32_t), seg.size(), fo);
  }
  std::fclose(fo);
  return 0;
}
