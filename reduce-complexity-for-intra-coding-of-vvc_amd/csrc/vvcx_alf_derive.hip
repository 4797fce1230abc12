// vvcx_alf_derive.hip — the host numeric code of ALF behind the C-ABI (include/vvcx.h): the filter tables of the caller's parameter sets, and the filter derivation of
// the encoder side (vvcx_alf_decide; alf_decide_frames for the decisions whose statistics stay on the device).  The only device work is what alf_decide_frames asks
// of alf_sums / alf_errors and, for several chroma alternatives, of alf_label_sums / alf_assign (vvcx_api_loopfilter.hip).
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "vvcx.h"
#include "vvcx_handle.h"      // fail
#include "vvcx_alf_derive.h"

// ---- adaptive loop filter (≙ AdaptiveLoopFilter::ALFProcess, CL/AdaptiveLoopFilter.cpp:205-383) with the caller's parameter sets: the per-class tables of every frame's
// slice are built here (≙ reconstructCoeffAPSs 385-418 / reconstructCoeff 420-608, JVET_O0669 form), the kernels (vvcx_alf.hip) classify and filter.
int alf_clip_value(int chroma, int bit_depth, int idx)      // create() 633-654
{
  if (!chroma) return (int) std::round(std::pow(2., (double) (bit_depth * (4 - idx)) / 4));
  if (idx == 0) return 1 << bit_depth;
  return (int) std::round(std::pow(2., bit_depth - 8 + 8. * (4 - idx - 1) / 3));
}
int alf_build(const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int n_frames, int nctu, int bit_depth, int chroma, std::vector<VxAlfFrame> &tabs)
{
  if (n_aps < 0 || n_aps > 8) return fail(VVCX_ERR_ARG, "ALF: %d parameter sets (0..8)", n_aps);
  for (int i = 0; i < n_aps; i++) {
    const vvcx_alf_aps &a = aps[i];
    if (a.num_luma_filters < 1 || a.num_luma_filters > 25 || a.num_chroma_alt < 0 || a.num_chroma_alt > 8) return fail(VVCX_ERR_ARG, "ALF parameter set %d: %d luma filters / %d chroma alternatives", i, a.num_luma_filters, a.num_chroma_alt);
    for (int c = 0; c < 25; c++) if (a.class_to_filter[c] >= a.num_luma_filters) return fail(VVCX_ERR_ARG, "ALF parameter set %d: class %d uses filter %d of %d", i, c, a.class_to_filter[c], a.num_luma_filters);
    for (int f = 0; f < a.num_luma_filters; f++) for (int k = 0; k < 12; k++) if (a.luma_clip_idx[f][k] > 3) return fail(VVCX_ERR_ARG, "ALF parameter set %d: clipping index above 3", i);
    for (int t = 0; t < a.num_chroma_alt; t++) for (int k = 0; k < 6; k++) if (a.chroma_clip_idx[t][k] > 3) return fail(VVCX_ERR_ARG, "ALF parameter set %d: clipping index above 3", i);
  }
  tabs.assign((size_t) n_frames, VxAlfFrame());
  for (int f = 0; f < n_frames; f++) {
    const vvcx_alf_slice &sl = slices[f];
    VxAlfFrame &t = tabs[(size_t) f];
    memset(&t, 0, sizeof t);
    if (sl.n_luma_aps < 0 || sl.n_luma_aps > 8 || sl.chroma_aps >= n_aps) return fail(VVCX_ERR_ARG, "ALF slice of frame %d: %d luma sets / chroma set %d of %d", f, sl.n_luma_aps, sl.chroma_aps, n_aps);
    t.n_sets = sl.n_luma_aps;
    for (int k = 0; k < sl.n_luma_aps; k++) {
      if (sl.luma_aps[k] < 0 || sl.luma_aps[k] >= n_aps) return fail(VVCX_ERR_ARG, "ALF slice of frame %d: luma set %d of %d", f, sl.luma_aps[k], n_aps);
      const vvcx_alf_aps &a = aps[sl.luma_aps[k]];
      for (int c = 0; c < 25; c++) for (int i = 0; i < 12; i++) {
        const int fl = a.class_to_filter[c];
        t.luma_coeff[k][c][i] = a.luma_coeff[fl][i];
        t.luma_clip[k][c][i] = (int16_t) alf_clip_value(0, bit_depth, a.nonlinear_luma ? a.luma_clip_idx[fl][i] : 0);
      }
    }
    const bool chromaOn = chroma && sl.chroma_aps >= 0;
    if (chromaOn) {
      const vvcx_alf_aps &a = aps[sl.chroma_aps];
      t.n_alt = a.num_chroma_alt;
      for (int alt = 0; alt < a.num_chroma_alt; alt++) for (int i = 0; i < 6; i++) {
        t.chroma_coeff[alt][i] = a.chroma_coeff[alt][i];
        t.chroma_clip[alt][i] = (int16_t) alf_clip_value(1, bit_depth, a.nonlinear_chroma[alt] ? a.chroma_clip_idx[alt][i] : 0);
      }
    }
    for (int a = 0; a < nctu; a++) {
      const vvcx_alf_ctu &u = ctus[(size_t) f * nctu + a];
      if (u.flag[0] && (u.set < 0 || u.set >= 16 + t.n_sets)) return fail(VVCX_ERR_ARG, "ALF: frame %d CTU %d uses luma filter set %d of %d", f, a, u.set, 16 + t.n_sets);
      for (int c = 1; c < 3; c++) if (chromaOn && u.flag[c] && u.alt[c - 1] >= t.n_alt) return fail(VVCX_ERR_ARG, "ALF: frame %d CTU %d uses chroma alternative %d of %d", f, a, u.alt[c - 1], t.n_alt);
    }
  }
  return VVCX_OK;
}
// the per-CTU choices as the kernels read them: chroma flags cleared where the slice has no chroma set (≙ slice-level alf_chroma_idc)
void alf_ctus(const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int n_frames, int nctu, int chroma, std::vector<VxAlfCtu> &out)
{
  out.resize((size_t) n_frames * nctu);
  for (int f = 0; f < n_frames; f++) for (int a = 0; a < nctu; a++) {
    const vvcx_alf_ctu &u = ctus[(size_t) f * nctu + a]; VxAlfCtu &o = out[(size_t) f * nctu + a];
    const bool con = chroma && slices[f].chroma_aps >= 0;
    o.flag[0] = u.flag[0] != 0; o.flag[1] = con && u.flag[1]; o.flag[2] = con && u.flag[2]; o.set = u.set; o.alt[0] = u.alt[0]; o.alt[1] = u.alt[1];
  }
}
// ---- the filter decision for ONE picture from bin 0 of its statistics: linear filters only (see include/vvcx.h for what is in and out of scope and for the bit count).
// The structure is the reference's (ALFProcess 661, mergeClasses 2344, deriveFilterCoeffs 2158, deriveCoeffQuant 2279, deriveCtbAlfEnableFlags 834); the code is this
// project's.  A filter c (taps without the centre, 7 fractional bits) on statistics (E, y, pixAcc) predicts the squared error  pixAcc - 2 c.y / 128 + c.E.c / 128^2.
namespace {
struct AlfCov {
  double E[12][12], y[12], pix;
  void clear() { memset(this, 0, sizeof *this); }
  // bin 0 of one (CTU, class) block of the statistics arrays: nc x nc | .. | y | .. | pixAcc; the centre row / column (nc - 1) is left out
  void add(const int64_t *s, int nb, int nc)
  {
    const int64_t *ys = s + (size_t) nb * nb * nc * nc;
    for (int k = 0; k < nc - 1; k++) { for (int l = 0; l < nc - 1; l++) E[k][l] += (double) s[k * nc + l]; y[k] += (double) ys[k]; }
    pix += (double) ys[(size_t) nb * nc];
  }
  void add(const AlfCov &o, int n) { for (int k = 0; k < n; k++) { for (int l = 0; l < n; l++) E[k][l] += o.E[k][l]; y[k] += o.y[k]; } pix += o.pix; }
  double err_q(const int *q, int n) const
  {
    double a = 0, b = 0;
    for (int k = 0; k < n; k++) { a += q[k] * y[k]; double r = 0; for (int l = 0; l < n; l++) r += E[k][l] * q[l]; b += q[k] * r; }
    return pix - a / 64. + b / 16384.;
  }
};
// Cholesky solve of (E + eps I) c = y; false when a pivot is not positive
static bool alf_chol(const AlfCov &s, int n, double eps, double *c)
{
  double L[12][12], z[12], dmax = 0;
  for (int k = 0; k < n; k++) dmax = std::max(dmax, s.E[k][k] + eps);
  for (int i = 0; i < n; i++) for (int j = 0; j <= i; j++) {
    double v = s.E[i][j] + (i == j ? eps : 0.);
    for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
    if (i == j) { if (!(v > 1e-12 * dmax)) return false; L[i][i] = std::sqrt(v); } else L[i][j] = v / L[j][j];
  }
  for (int i = 0; i < n; i++) { double v = s.y[i]; for (int k = 0; k < i; k++) v -= L[i][k] * z[k]; z[i] = v / L[i][i]; }
  for (int i = n - 1; i >= 0; i--) { double v = z[i]; for (int k = i + 1; k < n; k++) v -= L[k][i] * c[k]; c[i] = v / L[i][i]; }
  return true;
}
// least-squares coefficients: plain, then with a growing multiple of the mean diagonal on the diagonal while the matrix is singular; zero when nothing helps
static void alf_solve(const AlfCov &s, int n, double *c)
{
  double tr = 0; for (int k = 0; k < n; k++) tr += s.E[k][k];
  for (int k = 0; k < n; k++) c[k] = 0;
  if (!(tr > 0)) return;
  if (alf_chol(s, n, 0., c)) return;
  for (double rel = 1e-10; rel < 1.; rel *= 100.) if (alf_chol(s, n, rel * tr / n, c)) return;
  for (int k = 0; k < n; k++) c[k] = 0;
}
// the least error any real filter reaches on these statistics
static double alf_ls_error(const AlfCov &s, int n) { double c[12], a = 0; alf_solve(s, n, c); for (int k = 0; k < n; k++) a += c[k] * s.y[k]; return s.pix - a; }
// integer coefficients (7 fractional bits, -128 .. 127): rounding, then single steps of one coefficient while the predicted error falls; the zero filter if that is better
static double alf_quant(const AlfCov &s, int n, int *q)
{
  double c[12]; alf_solve(s, n, c);
  for (int k = 0; k < n; k++) q[k] = (int) std::min(127., std::max(-128., std::floor(c[k] * 128. + .5)));
  double best = s.err_q(q, n);
  for (int pass = 0; pass < 64; pass++) {
    bool moved = false;
    for (int k = 0; k < n; k++) for (int st = -1; st <= 1; st += 2) {
      if (q[k] + st < -128 || q[k] + st > 127) continue;
      q[k] += st;
      const double e = s.err_q(q, n);
      if (e < best) { best = e; moved = true; } else q[k] -= st;
    }
    if (!moved) break;
  }
  if (!(best < s.pix)) { for (int k = 0; k < n; k++) q[k] = 0; best = s.pix; }
  return best;
}
static int alf_ue_bits(int v) { int b = 1; for (v++; v > 1; v >>= 1) b += 2; return b; }      // ue(v)
static int alf_coeff_bits(const int *q, int n) { int b = 0; for (int k = 0; k < n; k++) b += alf_ue_bits(q[k] < 0 ? -q[k] : q[k]) + (q[k] != 0); return b; }
struct AlfLuma { int n; uint8_t map[25]; int q[25][12]; double dist; int bits; };
// merge the classes greedily from 25 groups to 1 (always the pair whose merge raises the least-squares error least), then the filter count <= max_filters with the least
// predicted distortion + lambda * bits
static void alf_derive_luma(const AlfCov *cls, double lambda, int max_filters, AlfLuma &best)
{
  AlfCov grp[25]; double gerr[25]; int of[25]; bool alive[25];
  static thread_local uint8_t maps[26][25];
  for (int c = 0; c < 25; c++) { grp[c] = cls[c]; gerr[c] = alf_ls_error(grp[c], 12); of[c] = c; alive[c] = true; }
  for (int n = 25; n >= 1; n--) {
    int idx[25], m = 0;
    for (int g = 0; g < 25; g++) if (alive[g]) idx[g] = m++;
    for (int c = 0; c < 25; c++) maps[n][c] = (uint8_t) idx[of[c]];
    if (n == 1) break;
    int bi = -1, bj = -1; double bd = 0, be = 0;
    for (int i = 0; i < 25; i++) if (alive[i]) for (int j = i + 1; j < 25; j++) if (alive[j]) {
      AlfCov t = grp[i]; t.add(grp[j], 12);
      const double e = alf_ls_error(t, 12), d = e - gerr[i] - gerr[j];
      if (bi < 0 || d < bd) { bi = i; bj = j; bd = d; be = e; }
    }
    grp[bi].add(grp[bj], 12); gerr[bi] = be; alive[bj] = false;
    for (int c = 0; c < 25; c++) if (of[c] == bj) of[c] = bi;
  }
  bool have = false;
  for (int n = std::min(25, std::max(1, max_filters)); n >= 1; n--) {
    AlfLuma t; t.n = n; t.dist = 0; memcpy(t.map, maps[n], 25);
    int mapBits = 0; for (int v = n - 1; v > 0; v >>= 1) mapBits++;
    t.bits = 1 + alf_ue_bits(n - 1) + (n > 1 ? 25 * mapBits : 0);
    for (int g = 0; g < n; g++) {
      AlfCov s; s.clear();
      for (int c = 0; c < 25; c++) if (t.map[c] == g) s.add(cls[c], 12);
      t.dist += alf_quant(s, 12, t.q[g]); t.bits += alf_coeff_bits(t.q[g], 12);
    }
    if (!have || t.dist + lambda * t.bits < best.dist + lambda * best.bits) { best = t; have = true; }
  }
}
}      // namespace

extern "C" int vvcx_alf_decide(int pic_w, int pic_h, int bit_depth, int chroma, int n_bins, const int64_t *luma, const int64_t *chroma_stats,
                               const double lambda[3], int max_luma_filters, vvcx_alf_aps *aps, vvcx_alf_slice *slice, vvcx_alf_ctu *ctus)
{
  if (!luma || !lambda || !aps || !slice || !ctus || (chroma && !chroma_stats)) return fail(VVCX_ERR_ARG, "null argument");
  if (pic_w < 8 || pic_h < 8 || (pic_w & 7) || (pic_h & 7) || pic_w > 16384 || pic_h > 16384 || bit_depth < 8 || bit_depth > 12 || (n_bins != 1 && n_bins != 4) ||
      max_luma_filters < 1 || max_luma_filters > 25 || !(lambda[0] >= 0) || !(lambda[1] >= 0) || !(lambda[2] >= 0))
    return fail(VVCX_ERR_ARG, "vvcx_alf_decide: picture size / bit depth / bins / filter count / lambdas");
  const int nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128), nb = n_bins;
  const size_t szl = alf_stat_size(nb, 13), szc = alf_stat_size(nb, 7);
  memset(aps, 0, sizeof *aps); memset(slice, 0, sizeof *slice); memset(ctus, 0, sizeof *ctus * (size_t) nctu);
  slice->n_luma_aps = 1; slice->luma_aps[0] = 0; slice->chroma_aps = -1;
  aps->num_luma_filters = 1;
  for (int a = 0; a < nctu; a++) ctus[a].set = 16;
  // ---- luma: filters from all CTUs, the CTUs' flags against them, the filters once more from the enabled CTUs
  {
    std::vector<AlfCov> cc((size_t) nctu * 25);
    for (int a = 0; a < nctu; a++) for (int c = 0; c < 25; c++) { AlfCov &s = cc[(size_t) a * 25 + c]; s.clear(); s.add(luma + ((size_t) a * 25 + c) * szl, nb, 13); }
    std::vector<uint8_t> on((size_t) nctu, 1);
    AlfLuma fl; int n_on = nctu; double gain = 0;
    for (int round = 0; round < 2 && n_on; round++) {
      AlfCov cls[25];
      for (int c = 0; c < 25; c++) { cls[c].clear(); for (int a = 0; a < nctu; a++) if (on[(size_t) a]) cls[c].add(cc[(size_t) a * 25 + c], 12); }
      alf_derive_luma(cls, lambda[0], max_luma_filters, fl);
      if (round == 0) {
        n_on = 0;
        for (int a = 0; a < nctu; a++) {
          double d_on = 0, d_off = 0;
          for (int c = 0; c < 25; c++) { const AlfCov &s = cc[(size_t) a * 25 + c]; d_on += s.err_q(fl.q[fl.map[c]], 12); d_off += s.pix; }
          on[(size_t) a] = d_on + lambda[0] * 1. < d_off;      // an enabled CTU codes one more bin (alf_use_aps_flag)
          n_on += on[(size_t) a];
        }
      }
    }
    if (n_on) {
      for (int a = 0; a < nctu; a++) if (on[(size_t) a]) {
        for (int c = 0; c < 25; c++) { const AlfCov &s = cc[(size_t) a * 25 + c]; gain += s.pix - s.err_q(fl.q[fl.map[c]], 12); }
        gain -= lambda[0];
      }
      if (!(gain > lambda[0] * fl.bits)) n_on = 0;      // the parameter set costs more than the filter gains: luma stays unfiltered
    }
    if (n_on) {
      aps->num_luma_filters = fl.n;
      for (int c = 0; c < 25; c++) aps->class_to_filter[c] = fl.map[c];
      for (int g = 0; g < fl.n; g++) for (int k = 0; k < 12; k++) aps->luma_coeff[g][k] = (int16_t) fl.q[g][k];
      for (int a = 0; a < nctu; a++) ctus[a].flag[0] = on[(size_t) a];
    }
  }
  // ---- chroma: one alternative for both components, flags per component
  if (chroma) {
    std::vector<AlfCov> cc((size_t) nctu * 2);
    for (size_t i = 0; i < cc.size(); i++) { cc[i].clear(); cc[i].add(chroma_stats + i * szc, nb, 7); }
    std::vector<uint8_t> on(cc.size(), 1);
    int q[6] = { 0 }, n_on = (int) cc.size();
    for (int round = 0; round < 2 && n_on; round++) {
      AlfCov s; s.clear();
      for (size_t i = 0; i < cc.size(); i++) if (on[i]) s.add(cc[i], 6);
      alf_quant(s, 6, q);
      if (round == 0) { n_on = 0; for (size_t i = 0; i < cc.size(); i++) { on[i] = cc[i].err_q(q, 6) < cc[i].pix; n_on += on[i]; } }      // one alternative: a CTU codes its flag only
    }
    double gain = 0;
    for (size_t i = 0; i < cc.size(); i++) if (on[i]) gain += cc[i].pix - cc[i].err_q(q, 6);
    const int bits = 1 + alf_ue_bits(0) + alf_coeff_bits(q, 6);
    if (n_on && gain > .5 * (lambda[1] + lambda[2]) * bits) {      // the parameter set's bits weigh with the mean of the two chroma lambdas
      slice->chroma_aps = 0; aps->num_chroma_alt = 1;
      for (int k = 0; k < 6; k++) aps->chroma_coeff[0][k] = (int16_t) q[k];
      for (size_t i = 0; i < cc.size(); i++) ctus[i >> 1].flag[1 + (i & 1)] = on[i];
    }
  }
  return VVCX_OK;
}

// (E, y, pixAcc) of one block of nb-bin statistics with tap k read at clipping index clip[k]
static void alf_gather(const int64_t *blk, int nb, int nc, const int *clip, AlfCov &s)
{
  const int64_t *ys = blk + (size_t) nb * nb * nc * nc;
  s.clear();
  for (int k = 0; k < nc - 1; k++) {
    for (int l = 0; l < nc - 1; l++) s.E[k][l] = (double) blk[((size_t) (clip[k] * nb + clip[l]) * nc + k) * nc + l];
    s.y[k] = (double) ys[clip[k] * nc + k];
  }
  s.pix = (double) ys[(size_t) nb * nc];
}
// tap k reads the same numbers at index a as at index b while the other taps stay at clip[]
static bool alf_same_rows(const int64_t *blk, int nb, int nc, const int *clip, int k, int a, int b)
{
  const int64_t *ys = blk + (size_t) nb * nb * nc * nc;
  if (ys[a * nc + k] != ys[b * nc + k] || blk[((size_t) (a * nb + a) * nc + k) * nc + k] != blk[((size_t) (b * nb + b) * nc + k) * nc + k]) return false;
  for (int l = 0; l < nc - 1; l++) if (l != k && blk[((size_t) (a * nb + clip[l]) * nc + k) * nc + l] != blk[((size_t) (b * nb + clip[l]) * nc + k) * nc + l]) return false;
  return true;
}
// The clipping indices of one filter on one block of 4-bin statistics (≙ AlfCovariance::optimizeFilter, EL 88-223, in this project's form): from index 0 everywhere the
// best single move of one tap by +- step (2, then 1), judged by the least-squares error of the re-solved gathered system, while one improves; integer coefficients by
// alf_quant on the gathered system; kept only if they predict less than the linear filter q_lin; then every index is lowered whose lower neighbour reads the same rows
// or whose coefficient is 0 (≙ reduceClipCost, EL 68-86).  false: the linear filter stays (q, clip untouched)
static bool alf_clip_search(const int64_t *blk, int nb, int nc, const int *q_lin, int *q, int *clip)
{
  const int n = nc - 1;
  int c[12] = { 0 }, qn[12];
  AlfCov s; alf_gather(blk, nb, nc, c, s);
  const double e_lin = s.err_q(q_lin, n);
  double best = alf_ls_error(s, n);
  for (int step = 2; step >= 1; step--) for (;;) {
    int bk = -1, bv = 0; double be = best;
    for (int k = 0; k < n; k++) for (int d = -step; d <= step; d += 2 * step) {
      const int v = c[k] + d, old = c[k];
      if (v < 0 || v >= nb) continue;
      c[k] = v; alf_gather(blk, nb, nc, c, s); c[k] = old;
      const double e = alf_ls_error(s, n);
      if (e < be) { be = e; bk = k; bv = v; }
    }
    if (bk < 0) break;
    c[bk] = bv; best = be;
  }
  alf_gather(blk, nb, nc, c, s);
  if (!(alf_quant(s, n, qn) < e_lin)) return false;
  bool any = false;
  for (int k = 0; k < n; k++) {
    if (qn[k] == 0) c[k] = 0;
    while (c[k] > 0 && alf_same_rows(blk, nb, nc, c, k, c[k], c[k] - 1)) c[k]--;
    any |= c[k] != 0;
  }
  if (!any) return false;
  for (int k = 0; k < n; k++) { q[k] = qn[k]; clip[k] = c[k]; }
  return true;
}

struct AlfLumaSet { AlfLuma f; int clip[25][12]; bool valid, nonlinear; };
static void alf_expand(const AlfLumaSet &t, vvcx_alf_luma_cand &cd)
{
  memset(&cd, 0, sizeof cd);
  if (t.valid) for (int c = 0; c < 25; c++) for (int k = 0; k < 12; k++) { cd.coeff[c][k] = (int16_t) t.f.q[t.f.map[c]][k]; cd.clip_idx[c][k] = (uint8_t) t.clip[t.f.map[c]][k]; }
}
// filters from the frame sums `sums` ([25][szl]); with `nonlinear` the clip search per group on the summed 4-bin blocks (the merge itself reads bin 0)
static void alf_luma_sets(const int64_t *sums, int nb, double lambda, int max_filters, bool nonlinear, AlfLumaSet &lin, AlfLumaSet &nl)
{
  const size_t szl = alf_stat_size(nb, 13);
  AlfCov cls[25];
  for (int c = 0; c < 25; c++) { cls[c].clear(); cls[c].add(sums + (size_t) c * szl, nb, 13); }
  alf_derive_luma(cls, lambda, max_filters, lin.f);
  memset(lin.clip, 0, sizeof lin.clip); lin.valid = true; lin.nonlinear = false;
  nl.valid = false;
  if (!nonlinear) return;
  nl = lin;
  std::vector<int64_t> blk(szl);
  for (int g = 0; g < lin.f.n; g++) {
    std::fill(blk.begin(), blk.end(), 0);
    for (int c = 0; c < 25; c++) if (lin.f.map[c] == g) for (size_t i = 0; i < szl; i++) blk[i] += sums[(size_t) c * szl + i];
    if (alf_clip_search(blk.data(), nb, 13, lin.f.q[g], nl.f.q[g], nl.clip[g])) {
      nl.nonlinear = true;
      nl.f.bits += alf_coeff_bits(nl.f.q[g], 12) - alf_coeff_bits(lin.f.q[g], 12);
    }
  }
  nl.f.bits += 2 * 12 * nl.f.n;      // two bits per clipping index of every filter once the flag is on
  nl.valid = nl.nonlinear;
}

// ---- several chroma alternatives (≙ the chroma loop of alfEncoder, EL 1041-1135, in this project's form; include/vvcx.h has the algorithm and the bit count).  For
// K = k_max .. 2 the CTUs start in K raster runs (≙ initCtuAlternativeChroma, EL 3831-3847) and two steps alternate: the filters of the alternatives from the blocks that
// carry their label (alf_label_sums), and per (CTU, component) the cheapest of off and the alternatives (alf_assign).  All frames advance in the same device calls; a
// frame whose J has stopped falling is carried along unchanged.  j1[f] = J of the one-alternative decision already in aps / slices / ctus; a frame is overwritten only
// where an alternative set has a smaller J.
struct AlfAltSet { int K, q[8][6], clip[8][6]; bool nl[8]; std::vector<uint8_t> lab; double J; };
static int alf_alt_bits(int a, int K) { return K == 1 ? 0 : std::min(a + 1, K - 1); }      // codeAlfCtuAlternative: truncated unary, one bit per bin
static int alf_chroma_alts(AlfRes &r, const double lambda[3], bool nonlinear, int k_max, const double *j1, vvcx_alf_aps *aps, vvcx_alf_slice *slices, vvcx_alf_ctu *ctus)
{
  const int n = r.n, nctu = r.nctu, nb = r.nb, nblk = 2 * nctu;
  const size_t szc = alf_stat_size(nb, 7);
  const double lamC = .5 * (lambda[1] + lambda[2]), lam_c[2] = { lambda[1], lambda[2] };
  std::vector<AlfAltSet> best((size_t) n), cur((size_t) n);
  std::vector<uint8_t> lab((size_t) n * nblk), labOut((size_t) n * nblk), done((size_t) n);
  std::vector<int64_t> sums((size_t) n * k_max * szc), err((size_t) n * nblk);
  std::vector<double> cost((size_t) n), prevJ((size_t) n);
  std::vector<vvcx_alf_chroma_cand> cd((size_t) n * k_max);
  for (int f = 0; f < n; f++) { best[(size_t) f].K = 0; best[(size_t) f].J = j1[f]; }
  for (int K = k_max; K >= 2; K--) {
    for (int f = 0; f < n; f++) {
      AlfAltSet &c = cur[(size_t) f];
      c.K = K; memset(c.q, 0, sizeof c.q); memset(c.clip, 0, sizeof c.clip); memset(c.nl, 0, sizeof c.nl);
      for (int a = 0, alt = 0; a < nctu; a++) {
        lab[((size_t) f * nctu + a) * 2] = lab[((size_t) f * nctu + a) * 2 + 1] = (uint8_t) alt;
        if ((a + 1) * K >= (alt + 1) * nctu) ++alt;
      }
      done[(size_t) f] = 0; prevJ[(size_t) f] = INFINITY;
    }
    for (int it = 0; it < K + 1; it++) {      // two half-steps each: at most 2 (K + 1) of the 2 (K + 1) + 1 the reference allows
      if (std::find(done.begin(), done.end(), 0) == done.end()) break;
      // (a) the filters of the alternatives that have blocks; the others keep theirs
      if (const int rc = alf_label_sums(r, lab.data(), K, sums.data())) return rc;
      for (int f = 0; f < n; f++) {
        AlfAltSet &c = cur[(size_t) f];
        if (!done[(size_t) f]) for (int a = 0; a < K; a++) {
          const uint8_t *lf = lab.data() + (size_t) f * nblk;
          if (std::find(lf, lf + nblk, (uint8_t) a) == lf + nblk) continue;
          const int64_t *blk = sums.data() + ((size_t) f * K + a) * szc;
          AlfCov s; s.clear(); s.add(blk, nb, 7);
          alf_quant(s, 6, c.q[a]);
          memset(c.clip[a], 0, sizeof c.clip[a]); c.nl[a] = false;
          int qn[6], cn[6];
          if (nonlinear && alf_clip_search(blk, nb, 7, c.q[a], qn, cn)) {
            AlfCov g; alf_gather(blk, nb, 7, cn, g);
            if (s.err_q(c.q[a], 6) - g.err_q(qn, 6) > lamC * 12) {      // the clipped filter where its gain on these sums pays its clip bits
              for (int k = 0; k < 6; k++) { c.q[a][k] = qn[k]; c.clip[a][k] = cn[k]; }
              c.nl[a] = true;
            }
          }
        }
        for (int a = 0; a < K; a++) for (int k = 0; k < 6; k++) {
          cd[(size_t) f * K + a].coeff[k] = (int16_t) c.q[a][k]; cd[(size_t) f * K + a].clip_idx[k] = (uint8_t) c.clip[a][k];
        }
      }
      // (b) the CTUs' choices among them
      if (const int rc = alf_assign(r, cd.data(), K, lam_c, labOut.data(), err.data(), cost.data())) return rc;
      for (int f = 0; f < n; f++) {
        if (done[(size_t) f]) continue;
        const AlfAltSet &c = cur[(size_t) f];
        const uint8_t *lo = labOut.data() + (size_t) f * nblk;
        int to[8], used = 0, pbits = 0;
        for (int a = 0; a < K; a++) {
          to[a] = std::find(lo, lo + nblk, (uint8_t) a) != lo + nblk ? used++ : -1;
          if (to[a] >= 0) pbits += 1 + alf_coeff_bits(c.q[a], 6) + (c.nl[a] ? 12 : 0);
        }
        double J = 0.;
        if (used) {
          double ct = cost[(size_t) f];
          if (used != K) {      // fewer alternatives are left: the CTUs' bits are those of the final numbering
            ct = 0.;
            for (int i = 0; i < nblk; i++) if (lo[i] != 255) {
              const double e = (double) err[(size_t) f * nblk + i] / 16384., b = lam_c[i & 1] * (double) alf_alt_bits(to[lo[i]], used);
              ct = ct + (e + b);
            }
          }
          J = ct + lamC * (alf_ue_bits(used - 1) + pbits);
          if (J < best[(size_t) f].J) {
            AlfAltSet &b = best[(size_t) f];
            b.K = used; b.J = J; b.lab.assign(lo, lo + nblk);
            for (int i = 0; i < nblk; i++) if (lo[i] != 255) b.lab[(size_t) i] = (uint8_t) to[lo[i]];
            for (int a = 0; a < K; a++) if (to[a] >= 0) { memcpy(b.q[to[a]], c.q[a], sizeof c.q[a]); memcpy(b.clip[to[a]], c.clip[a], sizeof c.clip[a]); b.nl[to[a]] = c.nl[a]; }
          }
        }
        if (!(J < prevJ[(size_t) f])) { done[(size_t) f] = 1; continue; }
        prevJ[(size_t) f] = J;
        memcpy(lab.data() + (size_t) f * nblk, lo, (size_t) nblk);
      }
    }
  }
  for (int f = 0; f < n; f++) {
    const AlfAltSet &b = best[(size_t) f];
    if (!b.K) continue;
    vvcx_alf_aps &ap = aps[f]; vvcx_alf_ctu *cu = ctus + (size_t) f * nctu;
    slices[f].chroma_aps = 0; ap.num_chroma_alt = b.K;
    memset(ap.nonlinear_chroma, 0, sizeof ap.nonlinear_chroma); memset(ap.chroma_coeff, 0, sizeof ap.chroma_coeff); memset(ap.chroma_clip_idx, 0, sizeof ap.chroma_clip_idx);
    for (int a = 0; a < b.K; a++) {
      ap.nonlinear_chroma[a] = b.nl[a];
      for (int k = 0; k < 6; k++) { ap.chroma_coeff[a][k] = (int16_t) b.q[a][k]; ap.chroma_clip_idx[a][k] = (uint8_t) b.clip[a][k]; }
    }
    for (int i = 0; i < nblk; i++) { const bool on = b.lab[(size_t) i] != 255; cu[i >> 1].flag[1 + (i & 1)] = on; cu[i >> 1].alt[i & 1] = on ? b.lab[(size_t) i] : 0; }
  }
  return VVCX_OK;
}

int alf_decide_frames(AlfRes &r, bool chroma, const double lambda[3], int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slices, vvcx_alf_ctu *ctus)
{
  const int n = r.n, nctu = r.nctu, nb = r.nb;
  const bool nlL = (flags & VVCX_ALF_NONLINEAR_LUMA) != 0, nlC = (flags & VVCX_ALF_NONLINEAR_CHROMA) != 0 && chroma, fx = (flags & VVCX_ALF_FIXED_SETS) != 0;
  const size_t szl = alf_stat_size(nb, 13), szc = alf_stat_size(nb, 7);
  const double lamC = .5 * (lambda[1] + lambda[2]);
  std::vector<int64_t> sl((size_t) n * 25 * szl), sc(chroma ? (size_t) n * 2 * szc : 0), slB;
  // ---- round 0: filters from all CTUs, the CTUs' choices against them (and against the fixed sets)
  if (const int rc = alf_sums(r, nullptr, sl.data(), chroma ? sc.data() : nullptr)) return rc;
  std::vector<AlfLumaSet> set((size_t) n * 4);      // per frame: linear / nonlinear from the flags-0 mask, linear / nonlinear from the CTUs that chose the new set over the fixed ones
  std::vector<vvcx_alf_luma_cand> lc((size_t) n * 4);
  std::vector<vvcx_alf_chroma_cand> cc((size_t) n * 2);
  std::vector<int> qc((size_t) n * 6), qcn((size_t) n * 6), clipc((size_t) n * 6); std::vector<uint8_t> cnl((size_t) n, 0);
  AlfLumaSet none; none.valid = false;
  std::vector<double> j1c((size_t) n, 0.);      // J of each frame's one-alternative chroma decision (0: chroma off)
  for (int f = 0; f < n; f++) {
    alf_luma_sets(sl.data() + (size_t) f * 25 * szl, nb, lambda[0], max_luma_filters, false, set[(size_t) f * 4], none);
    alf_expand(set[(size_t) f * 4], lc[(size_t) f]);
    if (chroma) {
      AlfCov s; s.clear(); s.add(sc.data() + (size_t) f * 2 * szc, nb, 7); s.add(sc.data() + ((size_t) f * 2 + 1) * szc, nb, 7);
      alf_quant(s, 6, &qc[(size_t) f * 6]);
      memset(&cc[(size_t) f], 0, sizeof cc[0]);
      for (int k = 0; k < 6; k++) cc[(size_t) f].coeff[k] = (int16_t) qc[(size_t) f * 6 + k];
    }
  }
  const int n0 = 16 * (int) fx + 1;
  std::vector<int64_t> e0((size_t) n * nctu * n0), ec0(chroma ? (size_t) n * nctu * 2 : 0);
  if (const int rc = alf_errors(r, fx, lc.data(), 1, chroma ? cc.data() : nullptr, chroma ? 1 : 0, e0.data(), ec0.data())) return rc;
  std::vector<uint8_t> maskA((size_t) n * nctu * 3, 0), maskB;
  std::vector<int> onA((size_t) n, 0), onB((size_t) n, 0), onC((size_t) n, 0);
  for (int f = 0; f < n; f++) for (int a = 0; a < nctu; a++) {
    const size_t i = (size_t) f * nctu + a;
    maskA[i * 3] = (double) e0[i * n0 + n0 - 1] / 16384. + lambda[0] * 1. < 0.;      // an enabled CTU codes one more bin (alf_use_aps_flag)
    onA[(size_t) f] += maskA[i * 3];
    if (chroma) for (int c = 0; c < 2; c++) { maskA[i * 3 + 1 + c] = ec0[i * 2 + c] < 0; onC[(size_t) f] += maskA[i * 3 + 1 + c]; }
  }
  bool needB = false;
  if (fx) {
    maskB = maskA;
    for (int f = 0; f < n; f++) for (int a = 0; a < nctu; a++) {
      const size_t i = (size_t) f * nctu + a;
      double best = 0.; int ch = -1;
      for (int s = 0; s < 16; s++) { const double v = (double) e0[i * n0 + s] / 16384. + 5. * lambda[0]; if (v < best) { best = v; ch = s; } }
      { const double v = (double) e0[i * n0 + 16] / 16384. + lambda[0]; if (v < best) { best = v; ch = 16; } }
      maskB[i * 3] = ch == 16; onB[(size_t) f] += ch == 16;
      needB |= maskB[i * 3] != maskA[i * 3];
    }
  }
  // ---- round 1: the filters once more from the CTUs that use them, the clip search on those sums, the last evaluation
  if (const int rc = alf_sums(r, maskA.data(), sl.data(), chroma ? sc.data() : nullptr)) return rc;
  if (needB) { slB.resize(sl.size()); if (const int rc = alf_sums(r, maskB.data(), slB.data(), nullptr)) return rc; }
  const int n1 = 1 + (int) nlL + (fx ? 1 + (int) nlL : 0), nc1 = 1 + (int) nlC, iB = 1 + (int) nlL;
  std::vector<vvcx_alf_luma_cand> lc1((size_t) n * n1);
  for (int f = 0; f < n; f++) {
    AlfLumaSet *t = &set[(size_t) f * 4];
    if (onA[(size_t) f]) alf_luma_sets(sl.data() + (size_t) f * 25 * szl, nb, lambda[0], max_luma_filters, nlL, t[0], t[1]); else t[1].valid = false;
    t[2].valid = t[3].valid = false;
    if (fx && onB[(size_t) f]) {
      if (needB) alf_luma_sets(slB.data() + (size_t) f * 25 * szl, nb, lambda[0], max_luma_filters, nlL, t[2], t[3]);
      else { t[2] = t[0]; t[3] = t[1]; t[2].valid = t[0].valid && onA[(size_t) f]; }
    }
    alf_expand(t[0], lc1[(size_t) f * n1]);
    if (nlL) alf_expand(t[1], lc1[(size_t) f * n1 + 1]);
    if (fx) { alf_expand(t[2], lc1[(size_t) f * n1 + iB]); if (nlL) alf_expand(t[3], lc1[(size_t) f * n1 + iB + 1]); }
    if (chroma) {
      int *q = &qc[(size_t) f * 6];
      std::vector<int64_t> blk(szc);
      for (size_t i = 0; i < szc; i++) blk[i] = sc[(size_t) f * 2 * szc + i] + sc[((size_t) f * 2 + 1) * szc + i];
      if (onC[(size_t) f]) { AlfCov s; s.clear(); s.add(blk.data(), nb, 7); alf_quant(s, 6, q); }
      if (nlC && onC[(size_t) f]) cnl[(size_t) f] = alf_clip_search(blk.data(), nb, 7, q, &qcn[(size_t) f * 6], &clipc[(size_t) f * 6]);
      memset(&cc[(size_t) f * nc1], 0, sizeof cc[0] * (size_t) nc1);
      for (int k = 0; k < 6; k++) {
        cc[(size_t) f * nc1].coeff[k] = (int16_t) q[k];
        if (cnl[(size_t) f]) { cc[(size_t) f * nc1 + 1].coeff[k] = (int16_t) qcn[(size_t) f * 6 + k]; cc[(size_t) f * nc1 + 1].clip_idx[k] = (uint8_t) clipc[(size_t) f * 6 + k]; }
      }
    }
  }
  std::vector<int64_t> e1((size_t) n * nctu * n1), ec1(chroma ? (size_t) n * nctu * 2 * nc1 : 0);
  if (const int rc = alf_errors(r, 0, lc1.data(), n1, chroma ? cc.data() : nullptr, chroma ? nc1 : 0, e1.data(), ec1.data())) return rc;
  // ---- per frame the least of the complete decisions: J = sum over CTUs (predicted error + lambda * bits) + lambda * parameter-set bits, relative to everything off
  for (int f = 0; f < n; f++) {
    vvcx_alf_aps &ap = aps[f]; vvcx_alf_slice &sl_o = slices[f]; vvcx_alf_ctu *cu = ctus + (size_t) f * nctu;
    const AlfLumaSet *t = &set[(size_t) f * 4];
    memset(&ap, 0, sizeof ap); memset(&sl_o, 0, sizeof sl_o); memset(cu, 0, sizeof *cu * (size_t) nctu);
    sl_o.n_luma_aps = 1; sl_o.luma_aps[0] = 0; sl_o.chroma_aps = -1;
    ap.num_luma_filters = 1;
    for (int a = 0; a < nctu; a++) cu[a].set = 16;
    const int64_t *ef = e0.data() + (size_t) f * nctu * n0, *en = e1.data() + (size_t) f * nctu * n1;
    // the flags-0 decision: vvcx_alf_decide's
    std::vector<int> choice((size_t) nctu, -1), trial((size_t) nctu);      // per CTU: -1 off, 0..15 fixed set, 16 the new set
    double bestJ = 0.; int bestSet = -1;
    if (onA[(size_t) f]) {
      double gain = 0;
      for (int a = 0; a < nctu; a++) if (maskA[((size_t) f * nctu + a) * 3]) gain += -(double) en[(size_t) a * n1] / 16384. - lambda[0];
      if (gain > lambda[0] * t[0].f.bits) {
        bestJ = lambda[0] * t[0].f.bits - gain; bestSet = 0;
        for (int a = 0; a < nctu; a++) choice[(size_t) a] = maskA[((size_t) f * nctu + a) * 3] ? 16 : -1;
      }
    }
    // the decisions the flags add: per CTU the least of off, the fixed sets and the new set x (x < 0: no new set)
    for (int x = fx ? -1 : 1; x < (fx || nlL ? 4 : 0); x++) {
      if (x >= 0 && (!t[x].valid || (!fx && x != 1))) continue;
      const int col = x < 0 ? 0 : x < 2 ? x : iB + (x - 2);
      double J = 0; int used = 0;
      for (int a = 0; a < nctu; a++) {
        double b = 0.; int ch = -1;
        if (fx) for (int s = 0; s < 16; s++) { const double v = (double) ef[(size_t) a * n0 + s] / 16384. + 5. * lambda[0]; if (v < b) { b = v; ch = s; } }
        if (x >= 0) { const double v = (double) en[(size_t) a * n1 + col] / 16384. + lambda[0]; if (v < b) { b = v; ch = 16; } }
        trial[(size_t) a] = ch; J += b; used += ch == 16;
      }
      if (x >= 0) { if (!used) continue; J += lambda[0] * t[x].f.bits; }
      if (J < bestJ) { bestJ = J; bestSet = x >= 0 ? x : -1; choice = trial; }
    }
    bool newUsed = false;
    for (int a = 0; a < nctu; a++) {
      const int ch = choice[(size_t) a];
      cu[a].flag[0] = ch >= 0; if (ch >= 0) cu[a].set = (int8_t) ch;
      newUsed |= ch == 16;
    }
    if (newUsed) {
      const AlfLumaSet &b = t[bestSet];
      ap.num_luma_filters = b.f.n; ap.nonlinear_luma = b.nonlinear;
      for (int c = 0; c < 25; c++) ap.class_to_filter[c] = b.f.map[c];
      for (int g = 0; g < b.f.n; g++) for (int k = 0; k < 12; k++) { ap.luma_coeff[g][k] = (int16_t) b.f.q[g][k]; ap.luma_clip_idx[g][k] = (uint8_t) b.clip[g][k]; }
    } else if (fx && bestJ < 0.) sl_o.n_luma_aps = 0;      // fixed sets only: the slice carries no luma parameter set
    // chroma: one alternative for both components, flags per component; the nonlinear one where it is cheaper
    if (chroma && onC[(size_t) f]) {
      const int64_t *ec = ec1.data() + (size_t) f * nctu * 2 * nc1;
      const int *q = &qc[(size_t) f * 6], *qn = &qcn[(size_t) f * 6];
      double gain = 0, J = 0., Jn = 0.;
      for (int i = 0; i < 2 * nctu; i++) if (maskA[((size_t) f * nctu + (i >> 1)) * 3 + 1 + (i & 1)]) gain += -(double) ec[(size_t) i * nc1] / 16384.;
      const int bits = 1 + alf_ue_bits(0) + alf_coeff_bits(q, 6);
      const bool lin = gain > lamC * bits;      // the parameter set's bits weigh with the mean of the two chroma lambdas
      if (lin) J = lamC * bits - gain;
      bool useN = false;
      if (cnl[(size_t) f]) {
        for (int i = 0; i < 2 * nctu; i++) Jn += std::min(0., (double) ec[(size_t) i * nc1 + 1] / 16384.);
        Jn += lamC * (1 + alf_ue_bits(0) + alf_coeff_bits(qn, 6) + 2 * 6);
        useN = Jn < J;
      }
      if (lin || useN) {
        j1c[(size_t) f] = useN ? Jn : J;
        sl_o.chroma_aps = 0; ap.num_chroma_alt = 1; ap.nonlinear_chroma[0] = useN;
        for (int k = 0; k < 6; k++) { ap.chroma_coeff[0][k] = (int16_t) (useN ? qn[k] : q[k]); ap.chroma_clip_idx[0][k] = (uint8_t) (useN ? clipc[(size_t) f * 6 + k] : 0); }
        for (int i = 0; i < 2 * nctu; i++) cu[i >> 1].flag[1 + (i & 1)] = useN ? ec[(size_t) i * nc1 + 1] < 0 : maskA[((size_t) f * nctu + (i >> 1)) * 3 + 1 + (i & 1)];
      }
    }
  }
  const int k_max = chroma ? std::min((flags >> 8) + 1, 2 * nctu) : 1;      // ≙ getMaxNumAlternativesChroma, EL 3849
  if (k_max >= 2) return alf_chroma_alts(r, lambda, nlC, k_max, j1c.data(), aps, slices, ctus);
  return VVCX_OK;
}
