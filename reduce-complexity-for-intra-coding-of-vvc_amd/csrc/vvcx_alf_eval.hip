// vvcx_alf_eval.hip — the passes the ALF encoder's decision makes over the covariance statistics while they stay in device memory (vvcx_alf_stats.hip wrote them):
// the masked frame sums (≙ EncAdaptiveLoopFilter::getFrameStats, EL/EncAdaptiveLoopFilter.cpp:2491-2565) and the error every candidate filter set is predicted to leave
// on every CTU (≙ AlfCovariance::calcErrorForCoeffs, EL 225-242, as alfEncoderCtb 3153-3300 calls it per CTU and set).  What crosses to the host afterwards is one block
// per frame and one int64 per (CTU, candidate) instead of 25 blocks per CTU.
//
// vvcx_alf_sum_kernel: one thread OWNS one output element (frame, class | chroma component, statistic element) and walks the CTUs whose mask byte is set; neighbouring
// threads read neighbouring int64, four CTUs in flight.  The pass is memory-bound: it reads nctu * 25 * size * 8 bytes per frame and writes 1 / nctu of that.
//
// vvcx_alf_cand_kernel: one workgroup OWNS one (frame, CTU, luma | Cb | Cr).  For every candidate s
//   err[s] = sum over classes ( sum_{k,l < n} q_k q_l E[clip_k][clip_l][k][l]  -  256 sum_k q_k y[clip_k][k] ),      n = 12 luma / 6 chroma (the centre row is not used),
// so that err / 16384 + pixAcc is the squared error the filter q (7 fractional bits) leaves.  Exact in int64: |v| < 2^(bd+1), at most 2^14 samples per CTU, |q| <= 128
// (the host layer refuses more), 144 terms: |quadratic term| < 2^(2 bd + 2 + 14 + 14 + 7.2) = 2^(2 bd + 37.2) - 2^57.2 at 10 bit, 2^61.2 at 12 bit; the linear term is
// below 2^(2 bd + 1 + 14 + 8 + 7 + 3.6).  Luma: the four waves take the classes in turn, a lane holds the (k, l) pairs lane, lane + 64, lane + 128 < 144; bin (0, 0) of a
// class is loaded once and serves every tap pair whose clipping indices are 0 (all of the fixed sets and of a linear set), the others are gathered from the class's
// block; per (class, candidate) one wave reduction of int64 and the sum of the wave's classes in its own LDS row.  Chroma (one class, 36 pairs): the waves take the
// candidates in turn.  Nothing is atomic, every output is written once, and integer adds make the result independent of the order.
// The two passes of the chroma-alternative iteration (vvcx_alf_chroma_label_sum_kernel, vvcx_alf_chroma_assign_kernel) stand at the end of the file.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vvcx_dev.h"
#include "vvcx_alf_tables.h"

extern "C" __global__ void __launch_bounds__(256) vvcx_alf_sum_kernel(VxAlfSumParams p)
{
  const int f = blockIdx.z, comp = blockIdx.y;                 // comp 0: the 25 luma classes, 1: Cb | Cr
  const size_t sz = comp ? p.size_c : p.size_l, per = (size_t) (comp ? 2 : 25) * sz;
  const size_t e = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  const long long *src = (comp ? p.chroma : p.luma) + (size_t) f * p.nctu * per + e;
  const uint8_t *on = p.ctu_on ? p.ctu_on + (size_t) f * p.nctu * 3 + (comp ? 1 + (int) (e / sz) : 0) : nullptr;
  long long s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  int a = 0;
  for (; a + 4 <= p.nctu; a += 4) {
    const bool m0 = !on || on[3 * a], m1 = !on || on[3 * a + 3], m2 = !on || on[3 * a + 6], m3 = !on || on[3 * a + 9];
    const long long v0 = m0 ? src[(size_t) a * per] : 0, v1 = m1 ? src[(size_t) (a + 1) * per] : 0, v2 = m2 ? src[(size_t) (a + 2) * per] : 0, v3 = m3 ? src[(size_t) (a + 3) * per] : 0;
    s0 += v0; s1 += v1; s2 += v2; s3 += v3;
  }
  for (; a < p.nctu; a++) if (!on || on[3 * a]) s0 += src[(size_t) a * per];
  ((comp ? p.chroma_out : p.luma_out) + (size_t) f * per)[e] = s0 + s1 + s2 + s3;
}

__device__ inline long long alf_wave_sum(long long v)
{
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// What lane `lane` of a wave adds to the error of chroma candidate cd on one block: the 36 tap pairs sit on lanes 0..35, the y terms on lanes 0..5.  e0 / y0 = bin (0, 0)
// and y[0] of the lane's pair / tap (0 on the other lanes), loaded once per block: they serve every candidate whose clipping indices are 0.  vvcx_alf_cand_kernel and
// vvcx_alf_chroma_assign_kernel both sum exactly this
__device__ inline long long alf_chroma_cand_term(const long long *blk, const long long *yb, int nb, int lane, long long e0, long long y0, const VxAlfChromaCand &cd)
{
  const bool pair = lane < 36, ylane = lane < 6;
  const int k = pair ? lane / 6 : 0, l = pair ? lane % 6 : 0;
  const int ck = cd.clip_idx[k], cl = cd.clip_idx[l];
  long long e = e0;
  if (pair && (ck | cl)) e = blk[((size_t) (ck * nb + cl) * 7 + k) * 7 + l];
  long long v = (long long) ((int) cd.coeff[k] * (int) cd.coeff[l]) * e;
  if (ylane) v -= 256ll * cd.coeff[lane] * (cd.clip_idx[lane] ? yb[cd.clip_idx[lane] * 7 + lane] : y0);
  return v;
}

extern "C" __global__ void __launch_bounds__(256) vvcx_alf_cand_kernel(VxAlfCandParams p)
{
  __shared__ long long acc[4][VX_ALF_MAX_CAND];
  const int ctu = blockIdx.x, c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = p.nb, nfix = p.fixed_sets ? 16 : 0;
  const size_t fc = (size_t) f * p.nctu + ctu;
  for (int i = tid; i < 4 * VX_ALF_MAX_CAND; i += 256) (&acc[0][0])[i] = 0;
  __syncthreads();
  if (c == 0) {
    const int ncand = nfix + p.n_luma;
    const size_t sz = (size_t) nb * nb * 169 + nb * 13 + 1;
    int pk[3], pl[3];                                          // the lane's (k, l) pairs; the third one exists on lanes 0..15
    for (int j = 0; j < 3; j++) { const int pr = lane + 64 * j; pk[j] = pr < 144 ? pr / 12 : 0; pl[j] = pr < 144 ? pr % 12 : 0; }
    const bool third = lane + 128 < 144, ylane = lane < 12;
    for (int cls = wave; cls < 25; cls += 4) {
      const long long *blk = p.luma + (fc * 25 + cls) * sz, *yb = blk + (size_t) nb * nb * 169;
      long long e0[3], y0 = ylane ? yb[lane] : 0;
      for (int j = 0; j < 3; j++) e0[j] = j < 2 || third ? blk[pk[j] * 13 + pl[j]] : 0;
      for (int s = 0; s < ncand; s++) {
        const int16_t *q; const uint8_t *ci = nullptr;
        if (s < nfix) {
          const int8_t *fx = VX_ALF_FIXED[VX_ALF_CLASS_TO_FIXED[s][cls]];
          long long v = 0;
          for (int j = 0; j < 3; j++) v += (long long) ((int) fx[pk[j]] * (int) fx[pl[j]]) * e0[j];
          if (ylane) v -= 256ll * fx[lane] * y0;
          v = alf_wave_sum(v);
          if (lane == 0) acc[wave][s] += v;
          continue;
        }
        const VxAlfLumaCand &cd = p.luma_cands[(size_t) f * p.n_luma + (s - nfix)];
        q = cd.coeff[cls]; ci = cd.clip_idx[cls];
        long long v = 0;
        for (int j = 0; j < 3; j++) {
          const int k = pk[j], l = pl[j], ck = ci[k], cl = ci[l];
          long long e = e0[j];
          if ((ck | cl) && (j < 2 || third)) e = blk[((size_t) (ck * nb + cl) * 13 + k) * 13 + l];
          v += (long long) ((int) q[k] * (int) q[l]) * e;
        }
        if (ylane) { const int ck = ci[lane]; v -= 256ll * q[lane] * (ck ? yb[ck * 13 + lane] : y0); }
        v = alf_wave_sum(v);
        if (lane == 0) acc[wave][s] += v;
      }
    }
    __syncthreads();
    if (tid < ncand) p.luma_err[fc * ncand + tid] = acc[0][tid] + acc[1][tid] + acc[2][tid] + acc[3][tid];
  } else {
    const size_t sz = (size_t) nb * nb * 49 + nb * 7 + 1;
    const long long *blk = p.chroma + (fc * 2 + (c - 1)) * sz, *yb = blk + (size_t) nb * nb * 49;
    const bool pair = lane < 36, ylane = lane < 6;
    const int k = pair ? lane / 6 : 0, l = pair ? lane % 6 : 0;
    const long long e0 = pair ? blk[k * 7 + l] : 0, y0 = ylane ? yb[lane] : 0;
    for (int s = wave; s < p.n_chroma; s += 4) {
      const long long v = alf_wave_sum(alf_chroma_cand_term(blk, yb, nb, lane, e0, y0, p.chroma_cands[(size_t) f * p.n_chroma + s]));
      if (lane == 0) p.chroma_err[(fc * 2 + (c - 1)) * p.n_chroma + s] = v;
    }
  }
}

// ---- the two passes of the chroma-alternative iteration (alf_decide_frames, vvcx_alf_derive.hip; ≙ the chroma loop of alfEncoder, EL 1041-1135).
//
// vvcx_alf_chroma_label_sum_kernel (≙ getFrameStats with the alternatives' CTU masks): one thread OWNS one statistic element e < size_c of one frame and walks the
// ctus * 2 chroma blocks ONCE, four loads in flight, with one int64 accumulator per alternative.  A block's label is the same for every lane: it is read through the
// scalar path and selects the accumulator by a wave-uniform branch; the accumulators are named, so none of them is a runtime-indexed array.  Cb and Cr are pooled.  The
// pass reads ctus * 2 * size_c * 8 bytes per frame (1.76 MB at 1080p with 4 bins) however many alternatives there are, and never touches the luma statistics.
#define VX_ALF_LS_ADD(lab_, v_) switch (lab_) { case 0: s0 += (v_); break; case 1: s1 += (v_); break; case 2: s2 += (v_); break; case 3: s3 += (v_); break; \
                                                 case 4: s4 += (v_); break; case 5: s5 += (v_); break; case 6: s6 += (v_); break; case 7: s7 += (v_); break; default: break; }
extern "C" __global__ void __launch_bounds__(256) vvcx_alf_chroma_label_sum_kernel(VxAlfLabelSumParams p)
{
  const int f = blockIdx.z, nblk = 2 * p.nctu;
  const size_t sz = p.size_c, e = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= sz) return;
  const long long *src = p.chroma + (size_t) f * nblk * sz + e;
  const uint8_t *lab = p.labels + (size_t) f * nblk;
  long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
  int b = 0;
  for (; b + 4 <= nblk; b += 4) {
    const int l0 = __builtin_amdgcn_readfirstlane((int) lab[b]), l1 = __builtin_amdgcn_readfirstlane((int) lab[b + 1]);
    const int l2 = __builtin_amdgcn_readfirstlane((int) lab[b + 2]), l3 = __builtin_amdgcn_readfirstlane((int) lab[b + 3]);
    const long long v0 = l0 != VX_ALF_LABEL_OFF ? src[(size_t) b * sz] : 0, v1 = l1 != VX_ALF_LABEL_OFF ? src[(size_t) (b + 1) * sz] : 0;
    const long long v2 = l2 != VX_ALF_LABEL_OFF ? src[(size_t) (b + 2) * sz] : 0, v3 = l3 != VX_ALF_LABEL_OFF ? src[(size_t) (b + 3) * sz] : 0;
    VX_ALF_LS_ADD(l0, v0) VX_ALF_LS_ADD(l1, v1) VX_ALF_LS_ADD(l2, v2) VX_ALF_LS_ADD(l3, v3)
  }
  for (; b < nblk; b++) {
    const int l0 = __builtin_amdgcn_readfirstlane((int) lab[b]);
    if (l0 != VX_ALF_LABEL_OFF) { const long long v0 = src[(size_t) b * sz]; VX_ALF_LS_ADD(l0, v0) }
  }
  long long *out = p.out + (size_t) f * p.n_alts * sz + e;
  const int K = p.n_alts;
  out[0] = s0;
  if (K > 1) out[sz] = s1;
  if (K > 2) out[2 * sz] = s2;
  if (K > 3) out[3 * sz] = s3;
  if (K > 4) out[4 * sz] = s4;
  if (K > 5) out[5 * sz] = s5;
  if (K > 6) out[6 * sz] = s6;
  if (K > 7) out[7 * sz] = s7;
}

// vvcx_alf_chroma_assign_kernel (≙ the alternative choice of deriveCtbAlfEnableFlags, EL 927-954): one workgroup OWNS one (frame, CTU, component).  The waves take the
// alternatives in turn, one int64 wave reduction per alternative into LDS; then one lane compares  err / 16384 + lambda * bits  in the order off, 0, 1, .. with a strict
// <, so the earliest wins a tie and off wins against a cost of exactly 0.  bits(a, K) is the truncated-unary length codeAlfCtuAlternative writes: 0 for K = 1, else
// min(a + 1, K - 1).  The product and the sum are rounded separately (a host loop in float64 gives the same bits).
extern "C" __global__ void __launch_bounds__(256) vvcx_alf_chroma_assign_kernel(VxAlfAssignParams p)
{
  __shared__ long long acc[VX_ALF_MAX_ALTS];
  const int ctu = blockIdx.x, c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = p.nb, K = p.n_alts;
  const size_t i = ((size_t) f * p.nctu + ctu) * 2 + c, sz = (size_t) nb * nb * 49 + nb * 7 + 1;
  const long long *blk = p.chroma + i * sz, *yb = blk + (size_t) nb * nb * 49;
  const bool pair = lane < 36, ylane = lane < 6;
  const long long e0 = pair ? blk[(lane / 6) * 7 + lane % 6] : 0, y0 = ylane ? yb[lane] : 0;
  for (int s = wave; s < K; s += 4) {
    const long long v = alf_wave_sum(alf_chroma_cand_term(blk, yb, nb, lane, e0, y0, p.cands[(size_t) f * K + s]));
    if (lane == 0) acc[s] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const double lam = p.lambda_c[c];
    double best = 0.; long long be = 0; int lab = VX_ALF_LABEL_OFF;
    for (int a = 0; a < K; a++) {
      const int bits = K == 1 ? 0 : (a + 1 < K - 1 ? a + 1 : K - 1);
      const double cost = __dadd_rn((double) acc[a] / 16384., __dmul_rn(lam, (double) bits));
      if (cost < best) { best = cost; be = acc[a]; lab = a; }
    }
    p.labels[i] = (uint8_t) lab; p.err[i] = be; p.term[i] = best;
  }
}
// the cost of a frame: one lane adds the terms in raster order, Cb before Cr, so that the sum is the one a host loop gives
extern "C" __global__ void __launch_bounds__(64) vvcx_alf_chroma_cost_kernel(VxAlfAssignParams p)
{
  if (threadIdx.x) return;
  const int f = blockIdx.x, nblk = 2 * p.nctu;
  const double *t = p.term + (size_t) f * nblk;
  double s = 0.;
  for (int b = 0; b < nblk; b++) s = __dadd_rn(s, t[b]);
  p.cost[f] = s;
}
