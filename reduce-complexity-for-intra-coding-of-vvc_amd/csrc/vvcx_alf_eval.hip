// vvcx_alf_eval.hip — the two passes the ALF encoder's decision makes over the covariance statistics while they stay in device memory (vvcx_alf_stats.hip wrote them):
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
      const VxAlfChromaCand &cd = p.chroma_cands[(size_t) f * p.n_chroma + s];
      const int ck = cd.clip_idx[k], cl = cd.clip_idx[l];
      long long e = e0, v = 0;
      if (pair && (ck | cl)) e = blk[((size_t) (ck * nb + cl) * 7 + k) * 7 + l];
      v = (long long) ((int) cd.coeff[k] * (int) cd.coeff[l]) * e;
      if (ylane) v -= 256ll * cd.coeff[lane] * (cd.clip_idx[lane] ? yb[cd.clip_idx[lane] * 7 + lane] : y0);
      v = alf_wave_sum(v);
      if (lane == 0) p.chroma_err[(fc * 2 + (c - 1)) * p.n_chroma + s] = v;
    }
  }
}
