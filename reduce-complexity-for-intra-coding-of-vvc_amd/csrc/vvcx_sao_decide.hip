// vvcx_sao_decide.hip — the SAO parameter decision on the device, from the statistics vvcx_sao_stats_kernel_* leaves in device memory (the RD half).
//
// What is computed is what vvcx_sao_decide (vvcx_api.hip: SaoDecision / SaoRate, ≙ EncSampleAdaptiveOffset::decideBlkParams, EL/EncSampleAdaptiveOffset.cpp:793-1098)
// computes on the host, bit for bit; that host code stays the yardstick.  It splits in two:
//   vvcx_sao_cand_kernel   everything that depends on the statistics and lambda only (SaoDecision::offsets, ::distortion, the bypass bins of SaoRate::component): one
//                          workgroup per (CTU, frame), one wave per component, one lane per (type, class) - 32 band lanes and 4 x 5 edge lanes of work per wave.
//   vvcx_sao_chain_kernel  the choice among the priced candidates and the two merge candidates (explicit_mode, merge_mode, the final choice), which depends on the two
//                          adaptive context models and on the neighbours' result: one wave per frame, CTUs in picture raster order (the models run on across tile borders,
//                          only the merge candidates are tile-restricted).  The wave stages a CTU's records and the merge distortions, lane 0 does the few dozen double
//                          operations of the walk.
// All cost arithmetic is fp64 in the host code's order of operations (built with -ffp-contract=off like the host and the emulator build): the same expressions, the same
// bits.  The one expression that is not repeated is the mean's division: round(diff / (count << step)) is taken in integers.  |diff| < 2^26 and count << step <= 2^18, so
// the exact quotient + 0.5 is an integer or at least 2^-19 away from one while the two double roundings of the host route move it by less than 2^-25: both give the same
// integer.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "vvcx_dev.h"

// estSaoDist: SSE change of adding o to n samples with difference sum d
__device__ static inline long long sao_gain(long long n, long long o, long long d) { return n * o * o - d * o * 2; }
__device__ static inline int sao_max_q(int bd) { return (1 << ((bd < 10 ? bd : 10) - 5)) - 1; }      // SampleAdaptiveOffset::getMaxOffsetQVal
// truncated-unary bins of one offset + (band offset) its sign bin
__device__ static inline int sao_offset_bins(int v, int th, bool band) { const int a = v < 0 ? -v : v; return (th ? (a < th ? a + 1 : th) : 0) + (band && v ? 1 : 0); }

extern "C" __global__ void __launch_bounds__(192) vvcx_sao_cand_kernel(VxSaoDecideParams p)
{
  __shared__ double s_cost[3][32];                   // band type: the cost of every band
  __shared__ long long s_gain[3][52];                // per lane of work: the SSE change of its kept offset
  __shared__ int s_off[3][52], s_band[3];
  const int a = blockIdx.x, f = blockIdx.y, c = threadIdx.x >> 6, r = threadIdx.x & 63;
  const bool band = r < 32, work = r < 52;
  const int t = band ? 4 : work ? (r - 32) / 5 : 0, k = band ? r : work ? (r - 32) % 5 : 0;
  const size_t at = (size_t) f * gridDim.x + a;
  const int th = sao_max_q(p.bit_depth);
  const double lambda = p.lambda[c];
  if (work) {
    // deriveOffsets 481-595: the mean difference of the class, rounded and clipped, then lowered towards zero while distortion + lambda * bits improves (estIterOffset)
    const long long *st = p.stats + ((at * 3 + c) * 5 + t) * 64;
    const long long n = st[k], d = st[32 + k];
    double cost = lambda; int best = 0;
    if (!(t != 4 && k == 2) && n != 0) {
      const long long den = n << p.step, ad = d < 0 ? -d : d, m = (2 * ad + den) / (2 * den);
      int q = m > th ? th : (int) m;
      if (d < 0) q = -q;
      if (t != 4 && ((k < 2 && q < 0) || (k > 2 && q > 0))) q = 0;            // a valley is never lowered, a peak never raised
      double bestCost = lambda;
      for (int it = q; it != 0; it += it > 0 ? -1 : 1) {
        const int ab = it < 0 ? -it : it;
        const long long bitsOf = (t == 4 ? ab + 2 : ab + 1) - (ab == th ? 1 : 0);
        const double cc = (double) sao_gain(n, (long long) it * (1 << p.step), d) + lambda * (double) bitsOf;
        if (cc < bestCost) { bestCost = cc; best = it; }
      }
      cost = bestCost;
    }
    s_off[c][r] = best; s_gain[c][r] = sao_gain(n, (long long) best * (1 << p.step), d);
    if (band) s_cost[c][k] = cost;
  }
  __syncthreads();
  // the four consecutive bands with the smallest cost: the first least of the 29 sums (a sum that is not below the largest double leaves position 0, as on the host)
  double sum = __DBL_MAX__; int pos = 0;
  if (r <= 28) { sum = s_cost[c][r] + s_cost[c][r + 1] + s_cost[c][r + 2] + s_cost[c][r + 3]; pos = r; }
  for (int m = 16; m; m >>= 1) {
    const double os = __shfl_xor(sum, m); const int op = __shfl_xor(pos, m);
    if (os < sum || (os == sum && op < pos)) { sum = os; pos = op; }
  }
  if (r == 0) s_band[c] = pos;
  __syncthreads();
  if (threadIdx.x < 15) {
    // one record per (component, type): the kept offsets, their distortion and the bypass bins of SaoRate::component (Y and Cb carry the type of their channel: one
    // bypass bin behind the context-coded one, and the two bins of the edge class)
    const int cc = threadIdx.x / 5, tt = threadIdx.x % 5;
    const bool first = cc < 2;
    VxSaoCand o; memset(&o, 0, sizeof o);
    int bins = first ? 1 : 0;
    for (int i = 0; i < 4; i++) {
      const int at_l = tt == 4 ? s_band[cc] + i : 32 + tt * 5 + (i < 2 ? i : i + 1), v = s_off[cc][at_l];
      o.off[i] = (int8_t) v; o.dist += s_gain[cc][at_l];
      bins += sao_offset_bins(v, th, tt == 4);
    }
    if (tt == 4) { o.band = (int8_t) s_band[cc]; bins += 5; } else if (first) bins += 2;
    o.bypass = bins;
    p.cands[(at * 3 + cc) * 5 + tt] = o;
  }
}

// the bit estimator of the SAO syntax (SaoRate of vvcx_api.hip): model 0 = SaoMergeFlag, 1 = SaoTypeIdx; everything else is bypass
struct SaoRateDev { uint16_t s0[2], s1[2]; unsigned long long bits; };
template <int W> __device__ static inline void sao_coded(SaoRateDev &r, const uint32_t *frac, const VxSaoDecideParams &p, bool bin)
{
  const unsigned st = (unsigned) (r.s0[W] + r.s1[W]) >> 8;
  r.bits += frac[st * 2 + (bin ? 1 : 0)];
  const int r0 = p.r0[W], r1 = p.r1[W];
  r.s0[W] -= (r.s0[W] >> r0) & 0x7FE0; r.s1[W] -= (r.s1[W] >> r1) & 0x7FFE;
  if (bin) { r.s0[W] += (0x7fffu >> r0) & 0x7FE0; r.s1[W] += (0x7fffu >> r1) & 0x7FFE; }
}

extern "C" __global__ void __launch_bounds__(64) vvcx_sao_chain_kernel(VxSaoDecideParams p)
{
  __shared__ uint32_t frac[512];
  __shared__ VxSaoEntry row[VXD_SAO_MAX_CTUS_W][3];   // reconstructed parameters: columns left of the current CTU from its row, the others from the row above
  __shared__ VxSaoCand cand[15];                      // the current CTU's records [component][type]
  __shared__ long long mdist[2][3];                   // distortion of merging from the left / above, per component
  const int f = blockIdx.x, lane = threadIdx.x, cw = p.ctus_w, nctu = p.ctus_w * p.ctus_h;
  for (int i = lane; i < 512; i += 64) frac[i] = p.frac_bits[i];
  SaoRateDev rate;
  for (int w = 0; w < 2; w++) { rate.s0[w] = p.s0[w]; rate.s1[w] = p.s1[w]; }
  rate.bits = 0;
  const double lam[3] = { p.lambda[0], p.lambda[1], p.lambda[2] };
  for (int a = 0; a < nctu; a++) {
    const int cx = a % cw, cy = a / cw;
    const size_t at = (size_t) f * nctu + a;
    const bool leftAv = cx > 0 && p.tile_of_ctu[a - 1] == p.tile_of_ctu[a], aboveAv = cy > 0 && p.tile_of_ctu[a - cw] == p.tile_of_ctu[a];
    __syncthreads();                                  // the table and the row entry of the CTU before this one are written, its records read
    {
      const uint32_t *src = (const uint32_t *) (p.cands + at * 15); uint32_t *dst = (uint32_t *) cand;
      for (int i = lane; i < (int) (15 * sizeof(VxSaoCand) / 4); i += 64) dst[i] = src[i];
    }
    if (lane < 6) {
      // deriveModeMergeRDO 737-791: the neighbour's reconstructed (scaled) offsets on this CTU's statistics of the neighbour's type
      const int m = lane / 3, k = lane % 3;
      long long d = 0;
      if (m ? aboveAv : leftAv) {
        const VxSaoEntry e = row[m ? cx : cx - 1][k];
        if (e.type >= 0) {
          const long long *st = p.stats + ((at * 3 + k) * 5 + e.type) * 64;
          for (int i = 0; i < 4; i++) { const int cl = e.type == 4 ? e.band + i : (i < 2 ? i : i + 1); d += sao_gain(st[cl], e.off[i], st[32 + cl]); }
        }
      }
      mdist[m][k] = d;
    }
    __syncthreads();
    if (lane == 0) {
      const SaoRateDev atStart = rate;
      // ---- deriveModeNewRDO 597-735: per channel the type with the least distortion + lambda * bits, Cb and Cr together
      int sel[3] = { -1, -1, -1 };                    // chosen type per component, -1: off
      long long dist[3] = { 0, 0, 0 };
      SaoRateDev r = atStart;
      if (leftAv) sao_coded<0>(r, frac, p, false);
      if (aboveAv) sao_coded<0>(r, frac, p, false);
      const SaoRateDev beforeLuma = r;
      SaoRateDev afterLuma;
      {
        r.bits = 0; sao_coded<1>(r, frac, p, false);
        double least = lam[0] * ((double) r.bits / 32768.0);
        afterLuma = r;
        for (int t = 0; t < 5; t++) {
          const long long d = cand[t].dist;
          r = beforeLuma; r.bits = 0; sao_coded<1>(r, frac, p, true); r.bits += (unsigned long long) cand[t].bypass << 15;
          const double c = (double) d + lam[0] * ((double) r.bits / 32768.0);
          if (c < least) { least = c; dist[0] = d; sel[0] = t; afterLuma = r; }
        }
        r = afterLuma;
      }
      {
        double c = 0; unsigned long long seen = 0;
        r.bits = 0;
        sao_coded<1>(r, frac, p, false);
        c += lam[1] * (1.0 / 32768.0) * (double) (r.bits - seen); seen = r.bits;
        c += lam[2] * (1.0 / 32768.0) * (double) (r.bits - seen); seen = r.bits;
        double least = c;
        for (int t = 0; t < 5; t++) {
          const long long d1 = cand[5 + t].dist, d2 = cand[10 + t].dist;
          r = afterLuma; r.bits = 0; seen = 0; c = 0;
          sao_coded<1>(r, frac, p, true); r.bits += (unsigned long long) cand[5 + t].bypass << 15;
          c += (double) d1 + lam[1] * (1.0 / 32768.0) * (double) (r.bits - seen); seen = r.bits;
          r.bits += (unsigned long long) cand[10 + t].bypass << 15;
          c += (double) d2 + lam[2] * (1.0 / 32768.0) * (double) (r.bits - seen); seen = r.bits;
          if (c < least) { least = c; dist[1] = d1; dist[2] = d2; sel[1] = sel[2] = t; }
        }
      }
      double norm = 0;
      for (int k = 0; k < 3; k++) norm += (double) dist[k] / lam[k];
      r = atStart; r.bits = 0;
      if (leftAv) sao_coded<0>(r, frac, p, false);
      if (aboveAv) sao_coded<0>(r, frac, p, false);
      sao_coded<1>(r, frac, p, sel[0] >= 0); if (sel[0] >= 0) r.bits += (unsigned long long) cand[sel[0]].bypass << 15;
      sao_coded<1>(r, frac, p, sel[1] >= 0); if (sel[1] >= 0) r.bits += (unsigned long long) cand[5 + sel[1]].bypass << 15;
      if (sel[2] >= 0) r.bits += (unsigned long long) cand[10 + sel[2]].bypass << 15;
      double least = norm + (double) r.bits / 32768.0;
      SaoRateDev after = r;
      // ---- deriveModeMergeRDO: the better of the two merge candidates, then the final choice
      int merge = -1;
      {
        double mleast = __DBL_MAX__; int mbest = -1; SaoRateDev best = atStart;
        for (int m = 0; m < 2; m++) {
          if (!(m ? aboveAv : leftAv)) continue;
          double nd = 0;
          for (int k = 0; k < 3; k++) if (row[m ? cx : cx - 1][k].type >= 0) nd += (double) mdist[m][k] / lam[k];
          r = atStart; r.bits = 0;
          if (leftAv) sao_coded<0>(r, frac, p, m == 0);
          if (m == 1) sao_coded<0>(r, frac, p, true);
          const double c = nd + (double) r.bits / 32768.0;
          if (c < mleast) { mleast = c; mbest = m; best = r; }
        }
        if (mleast < least) { least = mleast; merge = mbest; after = best; }
      }
      rate = after;
      // ---- the coded parameters and the reconstructed ones (xReconstructBlkSAOParams 265-290, invertQuantOffsets 147-170)
      for (int k = 0; k < 3; k++) {
        VxSaoSyn s; memset(&s, 0, sizeof s);
        VxSaoEntry e; memset(&e, 0, sizeof e); e.type = -1;
        if (merge >= 0) { s.mode = 2; s.type = (int8_t) merge; e = row[merge ? cx : cx - 1][k]; }
        else if (sel[k] >= 0) {
          const VxSaoCand &cd = cand[k * 5 + sel[k]];
          s.mode = 1; s.type = (int8_t) sel[k]; s.band = sel[k] == 4 ? cd.band : 0;
          e.type = (int8_t) sel[k]; e.band = s.band;
          for (int i = 0; i < 4; i++) { s.offset[i] = cd.off[i]; e.off[i] = (int16_t) (cd.off[i] * (1 << p.step)); }
        }
        row[cx][k] = e; p.table[at * 3 + k] = e; p.syn[at * 3 + k] = s;
      }
    }
  }
}
