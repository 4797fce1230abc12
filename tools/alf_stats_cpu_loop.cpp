// the arithmetic of getBlkStats / calcCovariance as a plain loop on one core: per luma sample the vector of 13 values per clipping bin, then the upper triangle of the
// 13 x 13 products for every pair of bins and the 13 products with the difference, accumulated in doubles per class (1920 x 1080, 8 bit)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>
static inline int clip2(int c, int cur, int a, int b) { return std::min(c, std::max(-c, a - cur)) + std::min(c, std::max(-c, b - cur)); }
int main()
{
  const int W = 1920, H = 1080, P = 3;
  std::vector<short> rec((W + 2 * P) * (H + 2 * P)), org(W * H);
  srand(1);
  for (auto &v : rec) v = rand() & 255;
  for (auto &v : org) v = rand() & 255;
  const int S = W + 2 * P;
  static const int DX[12] = { 0, 1, 0, -1, 2, 1, 0, -1, -2, 3, 2, 1 }, DY[12] = { 3, 2, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0 };
  const int clipv[4] = { 256, 64, 16, 4 };
  for (int nb : { 1, 4 }) {
    std::vector<double> E(25 * 16 * 169, 0.), Y(25 * 4 * 13, 0.), pix(25, 0.);
    const auto t0 = std::chrono::steady_clock::now();
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
      const int cls = ((x >> 2) * 7 + (y >> 2) * 3) % 25;
      const short *c = &rec[(y + P) * S + x + P];
      const int cur = *c, d = org[y * W + x] - cur;
      int v[13][4];
      for (int k = 0; k < 12; k++) for (int b = 0; b < nb; b++) v[k][b] = clip2(clipv[b], cur, c[DY[k] * S + DX[k]], c[-DY[k] * S - DX[k]]);
      for (int b = 0; b < nb; b++) v[12][b] = cur;
      double *e = &E[cls * 16 * 169];
      for (int k = 0; k < 13; k++) for (int l = k; l < 13; l++) for (int b0 = 0; b0 < nb; b0++) for (int b1 = 0; b1 < nb; b1++) e[(b0 * 4 + b1) * 169 + k * 13 + l] += (double) v[k][b0] * v[l][b1];
      for (int k = 0; k < 13; k++) for (int b = 0; b < nb; b++) Y[(cls * 4 + b) * 13 + k] += (double) v[k][b] * d;
      pix[cls] += (double) d * d;
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    double chk = 0; for (double v : E) chk += v;
    printf("cpu_loop 1920x1080 luma n_bins %d: %.1f ms (checksum %.0f)\n", nb, ms, chk + Y[5] + pix[3]);
  }
  return 0;
}
