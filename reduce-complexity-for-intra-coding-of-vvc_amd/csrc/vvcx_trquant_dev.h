// vvcx_trquant_dev.h — the block pipeline of one wave: residual -> transform -> quantiser -> dequantiser -> inverse transform -> reconstruction + SSE.
// Included by vvcx_kernel.hip (behind vvcx_depquant_dev.h, vvcx_lfnst_dev.h and the LMCS scale helpers, which it calls).
//
// Reference: TrQuant::xT / xIT (CL/TrQuant.cpp:835-992), Quant::quant / dequant (CL/Quant.cpp:994-1089, 423-549), TrQuant::getTrTypes (752-830).
// Every stage is defined once (VX_STAGE helpers, inlined into their callers); the __noinline__ entry functions below put them together:
//   wave_code_block      DCT-II, with the matrix-core rows, LFNST, LMCS chroma scaling and the raw / given modes
//   wave_fwd_sumabs      forward half of an explicit-MTS pair, ending in the sum of |coefficient|
//   wave_code_block_mts  explicit-MTS pairs (DST-VII / DCT-VIII)
//   wave_code_block_isp  strided tiles of ISP sub-partitions and the one-stage N x 1 / 1 x N forms
//   wave_ts_fwd / wave_ts_recon  transform skip
// A transform type (tr: 0 DCT-II, 1 DCT-VIII, 2 DST-VII) that an entry function knows is passed as a constant and folds away; a runtime one is tested per
// output, outside the loop of the dot product.
#pragma once
#define VX_STAGE __device__ __attribute__((always_inline)) inline

// ------------------------------------------------------------------------------------------------ packed dot products, matrices
// four matrix coefficients (int8, one 32-bit load) times four int16 samples (one 64-bit load) / four int32 values (one 128-bit load):
// rows of the matrices and of the sample tiles start at multiples of their length (>= 4 elements) in 16-byte aligned buffers
struct alignas(16) I32x4 { int x, y, z, w; };
// The first transform stage multiplies int8 matrix rows with 16-bit samples: two packed dot products (v_dot2c_i32_i16: two int16 x int16 products accumulated into 32
// bits, exact) per four samples; the residual pair comes from one packed subtraction (v_pk_sub_i16; samples and predictions are below 2^15).
#ifndef VX_DOT2_I16
typedef short vx_s2 __attribute__((ext_vector_type(2)));
#define VX_DOT2_I16(a_, b_, c_) __builtin_amdgcn_sdot2(__builtin_bit_cast(vx_s2, (uint32_t) (a_)), __builtin_bit_cast(vx_s2, (uint32_t) (b_)), (c_), false)
#define VX_PKSUB_I16(a_, b_) __builtin_bit_cast(uint32_t, __builtin_bit_cast(vx_s2, (uint32_t) (a_)) - __builtin_bit_cast(vx_s2, (uint32_t) (b_)))
#endif
__device__ inline uint2 m8x4_to_16(uint32_t m)                    // four int8 coefficients -> two words of packed int16 pairs
{
  uint2 r;
  r.x = (uint32_t) (uint16_t) (int16_t) (int8_t) m | ((uint32_t) (int) (int8_t) (m >> 8) << 16);
  r.y = (uint32_t) (uint16_t) (int16_t) (int8_t) (m >> 16) | ((uint32_t) ((int) m >> 24) << 16);
  return r;
}
__device__ inline int dot4_s16(uint32_t m, uint2 d)
{
  const uint2 c = m8x4_to_16(m);
  return VX_DOT2_I16(c.y, d.y, VX_DOT2_I16(c.x, d.x, 0));
}
__device__ inline int dot4_resi(uint32_t m, uint2 a, uint2 b)     // coefficients times (a - b), element-wise int16
{
  const uint2 c = m8x4_to_16(m);
  return VX_DOT2_I16(c.y, VX_PKSUB_I16(a.y, b.y), VX_DOT2_I16(c.x, VX_PKSUB_I16(a.x, b.x), 0));
}
__device__ inline int dot4_s32(uint32_t m, I32x4 d)
{
  return (int) (int8_t) m * d.x + (int) (int8_t) (m >> 8) * d.y + (int) (int8_t) (m >> 16) * d.z + (int) (int8_t) (m >> 24) * d.w;
}
// the same with the four data elements taken in reverse order (DCT-VIII rows are DST-VII rows on the reversed input)
__device__ inline uint2 rev4_s16(uint2 d) { uint2 r; r.x = (d.y >> 16) | (d.y << 16); r.y = (d.x >> 16) | (d.x << 16); return r; }
__device__ inline I32x4 rev4_s32(I32x4 d) { I32x4 r; r.x = d.w; r.y = d.z; r.z = d.y; r.w = d.x; return r; }
template <bool SMALL> __device__ inline const int8_t *dct2_matrix(int n)
{
  switch (n) { case 2: return VX_DCT2_2; case 4: return VX_DCT2_4; case 8: return VX_DCT2_8; case 16: return VX_DCT2_16; case 32: return VX_DCT2_32; default: return VX_DCT2_64; }
}
// ---- explicit MTS (TrQuant::getTrTypes 817-830): mts_idx 2..5 → (horizontal, vertical) ∈ {DST-VII, DCT-VIII}; tr: 0 DCT2, 1 DCT8, 2 DST7
__device__ inline void mts_types(int mts, int &trh, int &trv)
{
  if (mts < 2) { trh = trv = 0; return; }
  trh = ((mts - 2) & 1) ? 1 : 2; trv = ((mts - 2) >> 1) ? 1 : 2;
}
template <bool SMALL> __device__ inline const int8_t *tr_matrix(int tr, int n)
{
  if (tr == 0) return dct2_matrix<SMALL>(n);
  return n == 4 ? VX_DST7_4 : n == 8 ? VX_DST7_8 : n == 16 ? VX_DST7_16 : VX_DST7_32;
}
__device__ inline int tr_coef(const int8_t *M, int n, int tr, int k, int i)
{
  if (tr == 1) { const int v = M[k * n + (n - 1 - i)]; return (k & 1) ? -v : v; }
  return M[k * n + i];
}
// coefficients an explicit-MTS transform of length n keeps: 16 of a 32-point one (TrQuant::xT 853-854, xIT 935-936).  Blocks with an MTS pair are at most 32 long
// (mts_allowed), so there is no 64-point row to cut to 32 as the DCT-II callers do (imin(n, 32)).
__device__ inline int mts_kept(int tr, int n) { return (tr && n == 32) ? 16 : n; }

// ------------------------------------------------------------------------------------------------ shifts and quantiser parameters
__device__ inline int clip16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
// getTransformShift of a block of 2^lw x 2^lh, with the sqrt(2) adjustment of TU::needsSqrt2Scale where asked for (transform skip never asks)
__device__ inline int tr_shift_of(int lw, int lh, int bd, int need_sqrt) { return 15 - bd - ((lw + lh) >> 1) + (need_sqrt ? -1 : 0); }
// the two forward stages: (sum + rnd1) >> shift1 behind the horizontal one, (sum + rnd2) >> shift2 behind the vertical one.  The one-stage forms of N x 1 / 1 x N
// blocks are the horizontal stage of a block of lw + lh, 0.
struct FwdShifts { int shift1, rnd1, shift2, rnd2; };
VX_STAGE FwdShifts fwd_shifts(int lw, int lh, int bd)
{
  FwdShifts f;
  f.shift1 = lw + bd + 6 - 15; f.shift2 = lh + 6;
  f.rnd1 = f.shift1 > 0 ? 1 << (f.shift1 - 1) : 0; f.rnd2 = 1 << (f.shift2 - 1);
  return f;
}
// second inverse stage: (sum + (1 << (s - 1))) >> s; the first one is (sum + 64) >> 7 at every bit depth
__device__ inline int inv_shift2(int bd) { return (6 + 15 - 1) - bd; }
// Quant::quant without RDOQ (the 171 / 512 dead zone of intra slices)
struct QuantPar { int need_sqrt, tr_shift, qscale, qbits; long long qadd; };
VX_STAGE QuantPar quant_par(int lw, int lh, int bd, int qp)
{
  QuantPar q;
  q.need_sqrt = (lw + lh) & 1;
  q.qscale = L.t.qscale[q.need_sqrt * 6 + qp % 6];
  q.tr_shift = tr_shift_of(lw, lh, bd, q.need_sqrt);
  q.qbits = 14 + qp / 6 + q.tr_shift;
  q.qadd = (long long) 171 << (q.qbits - 9);
  return q;
}
// Quant::dequant 423-549 at the transform shift tr_shift (need_sqrt: the scale of the sqrt(2)-adjusted row)
struct DequantPar { int scale, right_shift, in_min, in_max; };
VX_STAGE DequantPar dequant_par(int need_sqrt, int tr_shift, int qp)
{
  DequantPar d;
  d.scale = L.t.iqscale[need_sqrt * 6 + qp % 6];
  d.right_shift = 6 - (tr_shift + qp / 6);
  int tbd = 32 + d.right_shift - 7; if (tbd > 16) tbd = 16;
  d.in_min = -(1 << (tbd - 1)); d.in_max = (1 << (tbd - 1)) - 1;
  return d;
}
__device__ inline int ts_shift(int w, int h, int bd) { return tr_shift_of(ilog2i(w), ilog2i(h), bd, 0); }                     // getTransformShift, TU::needsSqrt2Scale false for TS
__device__ inline int ts_scale(int r, int sh) { return sh >= 0 ? r * (1 << sh) : (r + (1 << (-sh - 1))) >> -sh; }
__device__ inline int ts_qp(int qp) { return imax(qp, 4); }                                                                   // QpParam::Qp(isTransformSkip), min_qp_prime_ts_minus4 0

// ------------------------------------------------------------------------------------------------ the stages
// plain quantiser of one coefficient; its magnitude goes into abs_sum
VX_STAGE int quant_plain(int c, const QuantPar &q, int &abs_sum)
{
  const long long t = (long long) iabs(c) * q.qscale;
  int l = (int) ((t + q.qadd) >> q.qbits);
  abs_sum += l;
  if (c < 0) l = -l;
  return clip16(l);
}
// plain dequantiser of one level, clipped to 16 bits.  The left shift is written as a product: the input clip keeps |l * scale| below 2^(31 + right_shift), so
// it cannot overflow and `<< -right_shift` (the form one copy of this had) gives the same bits.
VX_STAGE int dequant_plain(int l, const DequantPar &d)
{
  l = l < d.in_min ? d.in_min : l > d.in_max ? d.in_max : l;
  const int v = d.right_shift > 0 ? (l * d.scale + (1 << (d.right_shift - 1))) >> d.right_shift : (l * d.scale) * (1 << -d.right_shift);
  return clip16(v);
}
// the kept zw x zh levels (stride w) dequantised once: deq[m*zw + k]
VX_STAGE void wave_dequant_plain(const int16_t *lev, int16_t *deq, int w, int zw, int zh, int lzw, const DequantPar &d, int lane)
{
  for (int o = lane; o < zw * zh; o += 64) {
    const int m = o >> lzw, k = o & (zw - 1);
    deq[o] = (int16_t) dequant_plain(lev[m * w + k], d);
  }
}
// How a forward stage reads its rows: PK_ALWAYS with the packed loads above (dense tiles with rows of at least 4), PK_IF4 the same where the row has 4 (chroma
// blocks may be 2 wide or high), PK_NEVER sample by sample (the strided tiles of ISP: rows of 1 or 2, no alignment)
enum { PK_NEVER, PK_IF4, PK_ALWAYS };
// forward stage 1 (horizontal): tmp[k*h + j] = (sum_i M[k][i] * resi[j][i] + rnd1) >> shift1 for k < nk; resi = org - pred (rows st apart), or, with pre, what
// the caller left in resi.  DCT-VIII[k][i] = (-1)^k DST-VII[k][n-1-i]: the DST-VII row applied to the reversed input, sign by the parity of k (explicit MTS only:
// dense luma tiles, never pre)
template <int PK>
VX_STAGE void wave_fwd_h(const int8_t *M, int tr, const int16_t *org, const int16_t *pred, int pre, const int16_t *resi, int st, int32_t *tmp, int w, int h, int lh, int nk,
                         const FwdShifts &f, int lane)
{
  for (int o = lane; o < nk * h; o += 64) {
    const int k = o >> lh, j = o & (h - 1);
    int s = 0;
    if (tr == 1) { for (int i = 0; i < w; i += 4) s += dot4_resi(*(const uint32_t *) (M + k * w + i), rev4_s16(*(const uint2 *) (org + j * st + w - 4 - i)), rev4_s16(*(const uint2 *) (pred + j * st + w - 4 - i))); if (k & 1) s = -s; }
    else if (pre) { if (PK == PK_ALWAYS || (PK == PK_IF4 && w >= 4)) for (int i = 0; i < w; i += 4) s += dot4_s16(*(const uint32_t *) (M + k * w + i), *(const uint2 *) (resi + j * st + i)); else for (int i = 0; i < w; i++) s += M[k * w + i] * resi[j * st + i]; }
    else if (PK == PK_ALWAYS || (PK == PK_IF4 && w >= 4)) for (int i = 0; i < w; i += 4) s += dot4_resi(*(const uint32_t *) (M + k * w + i), *(const uint2 *) (org + j * st + i), *(const uint2 *) (pred + j * st + i));
    else for (int i = 0; i < w; i++) s += M[k * w + i] * (org[j * st + i] - pred[j * st + i]);
    tmp[o] = (s + f.rnd1) >> f.shift1;
  }
}
// forward stage 2 (vertical) of the nk x nm kept coefficients (lnk = log2 nk): c = (sum_j M[m][j] * tmp[k*h + j] + rnd2) >> shift2.  SUM: |c| is added to coef_sum.
// STORE: out[m*w + k] receives c itself (coef: the trellis works on the coefficients, 15 bits + sign by construction of the transform shifts) or its plain level
// (q; the magnitudes go into abs_sum)
template <int PK, bool SUM, bool STORE>
VX_STAGE void wave_fwd_v(const int8_t *M, int tr, const int32_t *tmp, int16_t *out, int w, int h, int nk, int nm, int lnk, const FwdShifts &f, int coef, const QuantPar *q,
                         int lane, int &coef_sum, int &abs_sum)
{
  for (int o = lane; o < nk * nm; o += 64) {
    const int m = o >> lnk, k = o & (nk - 1);
    int s = 0;
    if (tr == 1) { for (int j = 0; j < h; j += 4) s += dot4_s32(*(const uint32_t *) (M + m * h + j), rev4_s32(*(const I32x4 *) (tmp + k * h + h - 4 - j))); if (m & 1) s = -s; }
    else if (PK == PK_ALWAYS || (PK == PK_IF4 && h >= 4)) for (int j = 0; j < h; j += 4) s += dot4_s32(*(const uint32_t *) (M + m * h + j), *(const I32x4 *) (tmp + k * h + j));
    else for (int j = 0; j < h; j++) s += M[m * h + j] * tmp[k * h + j];
    const int c = (s + f.rnd2) >> f.shift2;
    if (SUM) coef_sum += iabs(c);
    if (!STORE) continue;
    if (coef) { out[m * w + k] = (int16_t) c; continue; }
    out[m * w + k] = (int16_t) quant_plain(c, *q, abs_sum);
  }
}
// inverse stage 1 (vertical): tcol[j*h + i] = clip16((sum_k M[k][i] * deq[k*zw + j] + 64) >> 7), j < zw
VX_STAGE void wave_inv_v(const int8_t *M, int tr, const int16_t *deq, int16_t *tcol, int h, int lh, int zw, int zh, int lzw, int lane)
{
  for (int o = lane; o < zw * h; o += 64) {
    const int j = o >> lh, i = o & (h - 1);
    int s = 0;
    if (tr == 1) for (int k = 0; k < zh; k++) { const int v = M[k * h + h - 1 - i] * deq[(k << lzw) + j]; s += (k & 1) ? -v : v; }
    else for (int k = 0; k < zh; k++) s += M[k * h + i] * deq[(k << lzw) + j];
    tcol[o] = (int16_t) clip16((s + 64) >> 7);
  }
}
__device__ inline unsigned long long sq_diff(int a, int b) { const int d = a - b; return (unsigned long long) (d * d); }
// reconstruction of the sample at offset a from its residual r (clipped to 16 bits); its SSE term is added to sse.  raw: the block is a bare residual, rec
// receives r unclipped and there is no SSE; cadj: LMCS chroma scale that multiplies the residual back (0: none)
VX_STAGE void recon_sample(const int16_t *org, int16_t *rec, int a, int r, int raw, int cadj, int bd, unsigned long long &sse)
{
  if (raw) { rec[a] = (int16_t) r; return; }
  if (cadj) r = lmcs_scale_inv((int) (int16_t) r, cadj, bd);
  const int mx = (1 << bd) - 1;
  int v = rec[a] + (int) (int16_t) r;
  v = v < 0 ? 0 : v > mx ? mx : v;
  rec[a] = (int16_t) v;
  sse += sq_diff(org[a], v);
}
// inverse stage 2 (horizontal): r = clip16((sum_k M[k][i] * tcol[k*h + j] + rnd) >> inv_shift2), reconstructed over the prediction in rec; returns the lane's SSE.
// STRIDED: org / rec rows are st apart, else the tiles are dense
template <bool STRIDED>
VX_STAGE unsigned long long wave_inv_h_recon(const int8_t *M, int tr, const int16_t *tcol, const int16_t *org, int16_t *rec, int st, int w, int h, int lw, int zw, int bd,
                                             int raw, int cadj, int lane)
{
  const int ishift2 = inv_shift2(bd), irnd2 = 1 << (ishift2 - 1);
  unsigned long long sse = 0;
  for (int o = lane; o < w * h; o += 64) {
    const int j = o >> lw, i = o & (w - 1);
    int s = 0;
    if (tr == 1) for (int k = 0; k < zw; k++) { const int v = M[k * w + w - 1 - i] * tcol[k * h + j]; s += (k & 1) ? -v : v; }
    else for (int k = 0; k < zw; k++) s += M[k * w + i] * tcol[k * h + j];
    recon_sample(org, rec, STRIDED ? j * st + i : o, clip16((s + irnd2) >> ishift2), raw, cadj, bd, sse);
  }
  return sse;
}
// no coefficient: the prediction is the reconstruction; the lane's SSE of org against it
template <bool STRIDED>
VX_STAGE unsigned long long wave_sse_pred(const int16_t *org, const int16_t *rec, int st, int w, int lw, int P, int lane)
{
  unsigned long long sse = 0;
  for (int o = lane; o < P; o += 64) { const int a = STRIDED ? (o >> lw) * st + (o & (w - 1)) : o; sse += sq_diff(org[a], rec[a]); }
  return sse;
}

// ------------------------------------------------------------------------------------------------ entry functions (one wave each)
// residual (org - pred) → forward stages (TrQuant::xT 835-915) → plain quant (Quant::quant 994-1089) → levels;
// if any level: dequant (423-549) → inverse stages (xIT 917-992) → reco = clip(pred + resi) written over pred; else the prediction stands.
// Returns SSE(org, reco) and the cbf via out params.  rec/lev tiles have stride w.  Buffers: the forward stages pass zw*h int32 through tmp; the decoder half
// re-uses it as int16: the dequantised coefficients deq[m*zw + k] (clipped to 16 bits) followed by the (16-bit clipped) output of the vertical stage:
// zw*zh + zw*h int16 <= the zw*h int32 of the forward pass.
// given >= 0: the levels in lev are taken as coded (cbf = given): only the decoder half runs (DecCu::xIntraRecBlk, DL/DecCu.cpp:199-414).
// given == -2: forward half only (batched full-RD stage): the coefficients stay in lev for the trellis of the batch.
// SMALL: rec / lev / tmp are the calling wave's LDS buffers (L.wm[wave].slot + buf_off, + 1024, L.wm[wave].tmp); else the _g pointers.
// With VVCX_TOOL_DEPQUANT the quantiser is the trellis of wave_depquant (comp: 0 Y / 1 Cb / 2 Cr, ci: the context set its rate terms are read from =
// the estimator's contexts at this point of the search, cbf_cb: tu.cbf[Cb] when Cr is quantised) and the dequantiser its state machine.
//
// wave_code_block: the DCT-II form of it, and what only DCT-II blocks have:
// cadj: LMCS chroma residual scale of the block (0: none): the residual is divided by it in front of the transform and multiplied back behind the inverse
// raw: the block is a bare residual (org = the residual, rec = zeros on entry): rec receives the reconstructed residual, unclipped (joint chroma blocks)
// lf: cu.lfnstIdx for a block of at least 4x4 (0 otherwise), lfmode: lfnst_mode() of its final intra mode (dependent quantisation only)
// SUMABS: sum of |DCT-II coefficient| for the MTS pruning (TrQuant::transformNxN 1049-1124)
template <bool SMALL, bool SUMABS = false>
__device__ __noinline__ void wave_code_block(const int16_t *org_g, int org_off, int buf_off, int16_t *rec_g, int16_t *lev_g, int32_t *tmp_g, int w, int h, int bd, int qp,
                                int lane, unsigned long long &sse_out, int &cbf_out, int given = -1, int *sumabs_out = nullptr, int comp = 0, int ci = 0, int cbf_cb = 0,
                                int lf = 0, int lfmode = 0, int raw = 0, int qidx = -1, int cadj = 0)
{
  org_g = uni_p(org_g); rec_g = uni_p(rec_g); lev_g = uni_p(lev_g); tmp_g = uni_p(tmp_g); sumabs_out = uni_p(sumabs_out);      // uniform arguments arrive in vector registers: scalar from here on
  int coef_sum = 0;
  w = uni(w); h = uni(h); bd = uni(bd); qp = uni(qp); given = uni(given);
  const int dq = uni((int) (L.par.tools & TOOL_DEPQUANT)) != 0;
  const int wave_ = uni(VTX >> 6);
  const int16_t *org = (SMALL ? L.org : org_g) + uni(org_off);
  int16_t *rec = SMALL ? L.wm[wave_].slot + uni(buf_off) : rec_g, *lev = SMALL ? L.wm[wave_].slot + BUF + uni(buf_off) : lev_g;
  int32_t *tmp = SMALL ? L.wm[wave_].tmp : tmp_g;
  const int P = w * h, lw = ilog2i(w), lh = ilog2i(h);
  const int zw = imin(w, 32), zh = imin(h, 32), lzw = imin(lw, 5);
  lf = uni(lf); lfmode = uni(lfmode);
  const int lfsb = (w >= 8 && h >= 8) ? 8 : 4;            // with LFNST only the top-left 4x4 / 8x8 of the primary coefficients is kept (xT 855-868)
  const int fzw = lf ? lfsb : zw, fzh = lf ? lfsb : zh, lfzw = lf ? ilog2i(lfsb) : lzw;
  const int8_t *Mw = dct2_matrix<SMALL>(w), *Mh = dct2_matrix<SMALL>(h);
  const FwdShifts f = fwd_shifts(lw, lh, bd);
  cadj = uni(cadj);
  if (cadj && given < 0) {                              // the scaled residual passes through the (still unused) level buffer
    for (int o = lane; o < P; o += 64) lev[o] = (int16_t) lmcs_scale_fwd(org[o] - rec[o], cadj, bd);
    wave_sync();
  }
#ifndef VX_NO_MFMA
  // 32- and 64-point rows on the matrix cores: D[k][j] = sum_i Mw[k][i] * resi[j][i] is a 32 x w by w x h GEMM of an int8 matrix with 11-bit residuals.  The residual is
  // split into a signed high byte and an unsigned low byte; the low byte is re-centred (lo - 128, so that it is an int8) and the 128 * (row sum of Mw) it leaves out is added back:
  // the DCT-II rows sum to zero except row 0 (64 * w; tests/test_host_cpu.py checks the tables).  v_mfma_i32_32x32x16_i8: lane l feeds row l % 32 of A / column l % 32 of B
  // with the eight k of half l / 32; the 16 results of a lane are rows 8 * (r / 4) + 4 * (l / 32) + r % 4 of column l % 32.  Exact: all partial sums stay far below 2^31.
  if (!SMALL && given < 0 && !cadj && !lf && (w == 32 || w == 64)) {
    typedef int vx_i16 __attribute__((ext_vector_type(16)));
    const int col = lane & 31, half = lane >> 5;
    for (int jt = 0; jt < h; jt += 32) {
      vx_i16 accH = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, accL = accH;
      const int j = jt + col;
      for (int q = 0; q < w; q += 16) {
        const int i0 = q + half * 8;
        const uint32_t a0 = *(const uint32_t *) (Mw + col * w + i0), a1 = *(const uint32_t *) (Mw + col * w + i0 + 4);
        const long a = (long) (((unsigned long long) a1 << 32) | a0);
        unsigned long long bh = 0, bl = 0;
        if (j < h) {
#pragma unroll
          for (int e = 0; e < 8; e++) {
            const int r = org[j * w + i0 + e] - rec[j * w + i0 + e];
            bh |= (unsigned long long) (unsigned) ((r >> 8) & 255) << (8 * e);
            bl |= (unsigned long long) (unsigned) (((r & 255) - 128) & 255) << (8 * e);
          }
        }
        accH = __builtin_amdgcn_mfma_i32_32x32x16_i8(a, (long) bh, accH, 0, 0, 0);
        accL = __builtin_amdgcn_mfma_i32_32x32x16_i8(a, (long) bl, accL, 0, 0, 0);
      }
      if (j < h) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int k = 8 * (r >> 2) + 4 * half + (r & 3);
          const int sacc = 256 * accH[r] + accL[r] + (k == 0 ? 128 * 64 * w : 0);
          tmp[k * h + j] = (sacc + f.rnd1) >> f.shift1;
        }
      }
    }
  } else
#endif
  if (given < 0) wave_fwd_h<PK_IF4>(Mw, 0, org, rec, cadj, lev, w, tmp, w, h, lh, fzw, f, lane);
  wave_sync();
  const QuantPar qpar = quant_par(lw, lh, bd, qp);
  // levels outside the kept region are zero (zw = min(w, 32): zw < w is w > 32, the form this test had here)
  if (given < 0 && (zw < w || zh < h)) { for (int o = lane; o < P; o += 64) lev[o] = 0; wave_sync(); }
  int abs_sum = 0;
  if (given < 0) wave_fwd_v<PK_IF4, SUMABS, true>(Mh, 0, tmp, lev, w, h, fzw, fzh, lfzw, f, dq, &qpar, lane, coef_sum, abs_sum);
  if (lf && given < 0) { wave_sync(); wave_lfnst_fwd(lev, w, w, h, lfmode, lf, (int32_t *) &L.wm[wave_].ws, lane); }      // xFwdLfnst (TrQuant::transformNxN 1220-1223)
  if (given == -2) {
    if (SUMABS) *sumabs_out = wave_sum_i32(coef_sum);
    wave_sync();
    sse_out = 0; cbf_out = 0;
    return;
  }
  if (dq && given < 0) {
    wave_sync();
    abs_sum = wave_depquant<SMALL>(lev, buf_off, L.par.scratch + (size_t) blockIdx.x * L.par.scratch_per_stream, ci, w, h, comp, VX_CTX_QtCbf[comp] + (comp == 2 ? cbf_cb : 0), 0, lf, lane, qidx);
  } else abs_sum = given < 0 ? uni(wave_sum_i32(abs_sum)) : given;
  if (SUMABS) *sumabs_out = wave_sum_i32(coef_sum);
  wave_sync();
  unsigned long long sse = 0;
  if (abs_sum > 0) {
    int16_t *deq = (int16_t *) tmp, *tcol = deq + zw * zh;
    if (dq) { wave_dequant_dq(lev, deq, w, h, zw, zh, bd, qp, lane); if (lf) wave_lfnst_inv(deq, zw, w, h, lfmode, lf, (int32_t *) &L.wm[wave_].ws, lane); }      // xInvLfnst (invTransformNxN 593-596)
    else { wave_dequant_plain(lev, deq, w, zw, zh, lzw, dequant_par(qpar.need_sqrt, qpar.tr_shift, qp), lane); wave_sync(); }
    wave_inv_v(Mh, 0, deq, tcol, h, lh, zw, zh, lzw, lane);
    wave_sync();
    sse = wave_inv_h_recon<false>(Mw, 0, tcol, org, rec, 0, w, h, lw, zw, bd, raw, cadj, lane);
  } else sse = wave_sse_pred<false>(org, rec, 0, w, lw, P, lane);
  wave_sync();
  sse_out = wave_sum_u64(sse);
  cbf_out = abs_sum > 0;
}

// forward 2-D transform of (org - pred) with the transform pair of mts and the sum of |coefficient| (the measure TrQuant::transformNxN
// 1049-1124 prunes the MTS candidates with); pred is the calling wave's candidate buffer (SMALL) or pred_g
template <bool SMALL>
__device__ __noinline__ int wave_fwd_sumabs(const int16_t *org_g, const int16_t *pred_g, int32_t *tmp_g, int w, int h, int bd, int mts, int lane)
{
  org_g = uni_p(org_g); pred_g = uni_p(pred_g); tmp_g = uni_p(tmp_g);
  w = uni(w); h = uni(h); bd = uni(bd); mts = uni(mts);
  const int wave_ = uni(VTX >> 6);
  const int16_t *org = SMALL ? L.org : org_g, *pred = SMALL ? L.wm[wave_].slot : pred_g;
  int32_t *tmp = SMALL ? L.wm[wave_].tmp : tmp_g;
  int trh, trv; mts_types(mts, trh, trv);
  const int lw = ilog2i(w), lh = ilog2i(h);
  const int zw = mts_kept(trh, w), zh = mts_kept(trv, h), lzw = ilog2i(zw);
  const int8_t *Mw = tr_matrix<SMALL>(trh, w), *Mh = tr_matrix<SMALL>(trv, h);
  const FwdShifts f = fwd_shifts(lw, lh, bd);
  wave_fwd_h<PK_ALWAYS>(Mw, trh, org, pred, 0, nullptr, w, tmp, w, h, lh, zw, f, lane);
  wave_sync();
  int sa = 0, none = 0;
  wave_fwd_v<PK_ALWAYS, true, false>(Mh, trv, tmp, nullptr, w, h, zw, zh, lzw, f, 0, nullptr, lane, sa, none);
  sa = wave_sum_i32(sa);
  wave_sync();
  return sa;
}
// wave_code_block with an explicit-MTS transform pair: the same stages with DST-VII / DCT-VIII matrices; no LFNST, LMCS scale or bare residual
template <bool SMALL>
__device__ __noinline__ void wave_code_block_mts(const int16_t *org_g, int16_t *rec_g, int16_t *lev_g, int32_t *tmp_g, int w, int h, int bd, int qp, int mts,
                                                 int lane, unsigned long long &sse_out, int &cbf_out, int given = -1)
{
  org_g = uni_p(org_g); rec_g = uni_p(rec_g); lev_g = uni_p(lev_g); tmp_g = uni_p(tmp_g);
  w = uni(w); h = uni(h); bd = uni(bd); qp = uni(qp); given = uni(given); mts = uni(mts);
  const int dq = uni((int) (L.par.tools & TOOL_DEPQUANT)) != 0;        // luma only: the rate terms come from the node's start contexts (CI_CUR)
  const int wave_ = uni(VTX >> 6);
  const int16_t *org = SMALL ? L.org : org_g;
  int16_t *rec = SMALL ? L.wm[wave_].slot : rec_g, *lev = SMALL ? L.wm[wave_].slot + BUF : lev_g;
  int32_t *tmp = SMALL ? L.wm[wave_].tmp : tmp_g;
  const int P = w * h;
  int trh, trv; mts_types(mts, trh, trv);
  const int lw = ilog2i(w), lh = ilog2i(h);
  const int zw = mts_kept(trh, w), zh = mts_kept(trv, h), lzw = ilog2i(zw);
  const int8_t *Mw = tr_matrix<SMALL>(trh, w), *Mh = tr_matrix<SMALL>(trv, h);
  const FwdShifts f = fwd_shifts(lw, lh, bd);
  if (given < 0) wave_fwd_h<PK_ALWAYS>(Mw, trh, org, rec, 0, nullptr, w, tmp, w, h, lh, zw, f, lane);
  wave_sync();
  const QuantPar qpar = quant_par(lw, lh, bd, qp);
  if (given < 0 && (zw < w || zh < h)) { for (int o = lane; o < P; o += 64) lev[o] = 0; wave_sync(); }
  int abs_sum = 0, none = 0;
  if (given < 0) wave_fwd_v<PK_ALWAYS, false, true>(Mh, trv, tmp, lev, w, h, zw, zh, lzw, f, dq, &qpar, lane, none, abs_sum);
  if (given == -2) { wave_sync(); sse_out = 0; cbf_out = 0; return; }
  if (dq && given < 0) {
    wave_sync();
    abs_sum = wave_depquant<SMALL>(lev, 0, L.par.scratch + (size_t) blockIdx.x * L.par.scratch_per_stream, CI_CUR, w, h, 0, VX_CTX_QtCbf[0], 1, 0, lane);
  } else abs_sum = given < 0 ? uni(wave_sum_i32(abs_sum)) : given;
  wave_sync();
  unsigned long long sse = 0;
  if (abs_sum > 0) {
    int16_t *deq = (int16_t *) tmp, *tcol = deq + zw * zh;
    if (dq) wave_dequant_dq(lev, deq, w, h, zw, zh, bd, qp, lane);
    else { wave_dequant_plain(lev, deq, w, zw, zh, lzw, dequant_par(qpar.need_sqrt, qpar.tr_shift, qp), lane); wave_sync(); }
    wave_inv_v(Mh, trv, deq, tcol, h, lh, zw, zh, lzw, lane);
    wave_sync();
    sse = wave_inv_h_recon<false>(Mw, trh, tcol, org, rec, 0, w, h, lw, zw, bd, 0, 0, lane);
  } else sse = wave_sse_pred<false>(org, rec, 0, w, lw, P, lane);
  wave_sync();
  sse_out = wave_sum_u64(sse);
  cbf_out = abs_sum > 0;
}
// The block pipeline of one sub-partition of an ISP CU (TU of tw x th samples; 1 x N, 2 x N, N x 1, N x 2 and larger).  What differs: implicit transform selection
// (TrQuant::getTrTypes 752-780: DST-VII along a side of 4..16 samples, DCT-II otherwise), the one-stage forms of N x 1 / 1 x N blocks (xT 895-914, xIT 970-983), always
// dependent quantisation, against the context set ci (the estimator's live contexts: the sub-partitions of a CU are coded one after the other) with the cbf context
// cbf_ctx (< 0: the cbf is inferred).  org / rec / lev: tiles of the CU (stride cst) at the TU's origin.  tmp: th * min(32, tw) int32 (and its int16 re-use).
// LDSP: every tile of the call lives in LDS (the search of ISP CUs of at most 128 samples)
template <bool LDSP>
__device__ __noinline__ void wave_code_block_isp(const int16_t *org, int16_t *rec, int16_t *lev, int cst, int32_t *tmp, int16_t *cf, uint8_t *scratch, int w, int h, int bd, int qp,
                                                 int lane, unsigned long long &sse_out, int &cbf_out, int given, int ci, int cbf_ctx)
{
  org = uni_p(org); rec = uni_p(rec); lev = uni_p(lev); tmp = uni_p(tmp); cf = uni_p(cf); scratch = uni_p(scratch); ci = uni(ci); cbf_ctx = uni(cbf_ctx);
  if (LDSP) { org = as_lds(org); rec = as_lds(rec); lev = as_lds(lev); tmp = as_lds(tmp); cf = as_lds(cf); }
  // cf: a dense w * h int16 tile for the coefficients / levels (the trellis and the residual syntax take stride w)
  w = uni(w); h = uni(h); bd = uni(bd); qp = uni(qp); given = uni(given); cst = uni(cst);
  const int trh = (w >= 4 && w <= 16) ? 2 : 0, trv = (h >= 4 && h <= 16) ? 2 : 0;
  const int P = w * h, lw = ilog2i(w), lh = ilog2i(h);
  const int zw = imin(w, 32), zh = imin(h, 32), lzw = ilog2i(zw);
  const int8_t *Mw = w > 1 ? tr_matrix<false>(trh, w) : nullptr, *Mh = h > 1 ? tr_matrix<false>(trv, h) : nullptr;
  const int oneD = w == 1 || h == 1;
  ISP_T(i0);
  if (given < 0) {
    if (!oneD) {
      const FwdShifts f = fwd_shifts(lw, lh, bd);
      wave_fwd_h<PK_NEVER>(Mw, trh, org, rec, 0, nullptr, cst, tmp, w, h, lh, zw, f, lane);
      wave_sync();
      for (int o = lane; o < P; o += 64) cf[o] = 0;
      wave_sync();
      int none = 0;
      wave_fwd_v<PK_NEVER, false, true>(Mh, trv, tmp, cf, w, h, zw, zh, lzw, f, 1, nullptr, lane, none, none);
    } else {
      const FwdShifts f = fwd_shifts(lw + lh, 0, bd);
      const int n = w * h, zn = imin(n, 32), step = w == 1 ? cst : 1;
      const int8_t *M = w == 1 ? Mh : Mw;
      for (int o = lane; o < n; o += 64) {
        int s = 0;
        if (o < zn) for (int i = 0; i < n; i++) s += M[o * n + i] * (org[i * step] - rec[i * step]);
        cf[o] = (int16_t) (o < zn ? (s + f.rnd1) >> f.shift1 : 0);
      }
    }
    wave_sync();
  } else {
    for (int o = lane; o < P; o += 64) cf[o] = lev[(o >> lw) * cst + (o & (w - 1))];
    wave_sync();
  }
  int abs_sum = given;
  ISP_T(i1);
  if (given < 0) abs_sum = LDSP ? wave_depquant<true>(nullptr, (int) (cf - (L.wm[uni(VTX >> 6)].slot + BUF)), scratch, ci, w, h, 0, cbf_ctx, 0, 0, lane)
                                : wave_depquant<false>(cf, 0, scratch, ci, w, h, 0, cbf_ctx, 0, 0, lane);
  wave_sync();
  ISP_T(i2);
  if (given < 0) { for (int o = lane; o < P; o += 64) lev[(o >> lw) * cst + (o & (w - 1))] = cf[o]; }
  unsigned long long sse = 0;
  if (abs_sum > 0) {
    int16_t *deq = (int16_t *) tmp, *tcol = deq + zw * zh;
    wave_dequant_dq(cf, deq, w, h, zw, zh, bd, qp, lane);
    if (!oneD) {
      wave_inv_v(Mh, trv, deq, tcol, h, lh, zw, zh, lzw, lane);
      wave_sync();
      sse = wave_inv_h_recon<true>(Mw, trh, tcol, org, rec, cst, w, h, lw, zw, bd, 0, 0, lane);
    } else {                                            // one stage: the sum of both inverse shifts, less the 6 bits of the stage that is not there
      const int n = w * h, zn = imin(n, 32), sh = inv_shift2(bd) + 1, rnd = 1 << (sh - 1), step = w == 1 ? cst : 1;
      const int8_t *M = w == 1 ? Mh : Mw;
      for (int o = lane; o < n; o += 64) {
        int s = 0;
        for (int k = 0; k < zn; k++) s += M[k * n + o] * deq[k];
        recon_sample(org, rec, o * step, clip16((s + rnd) >> sh), 0, 0, bd, sse);
      }
    }
  } else sse = wave_sse_pred<true>(org, rec, cst, w, lw, P, lane);
  wave_sync();
  sse_out = wave_sum_u64(sse);
  cbf_out = abs_sum > 0;
  { ISP_T(i3); ISP_ADD(16, i0, i1); ISP_ADD(17, i1, i2); ISP_ADD(18, i2, i3); }
}

// ------------------------------------------------------------------------------------------------ transform skip
// sum |xTransformSkip(org - pred)| scaled as TrQuant::transformNxN (1049-1124) scales the transform-skip entry of its pruning; optionally the coefficients to coef_out
__device__ inline int wave_ts_fwd(const int16_t *org, const int16_t *pred, int16_t *coef_out, int w, int h, int bd, int lane)
{
  const int P = w * h, sh = ts_shift(w, h, bd);
  int sa = 0;
  for (int e = lane; e < P; e += 64) { const int c = ts_scale(org[e] - pred[e], sh); if (coef_out) coef_out[e] = (int16_t) c; sa += iabs(c); }
  sa = wave_sum_i32(sa);
  const double scale = ((ilog2i(w) + ilog2i(h)) & 1) ? 1.0 / 1.414213562 : 1.0;
  return (int) ((double) sa * scale);
}
// decoder half of a transform-skip block by one wave: the plain dequantiser without the sqrt(2) adjustment at max(QP', 4), xITransformSkip, reconstruction over
// the prediction in rec, SSE against org.  raw: rec receives the bare residual (leaf test).  cbf 0: the prediction is the reconstruction.
__device__ __noinline__ void wave_ts_recon(const int16_t *org, int16_t *rec, const int16_t *lev, int w, int h, int bd, int qp, int cbf, int lane, unsigned long long &sse_out, int raw = 0)
{
  org = uni_p(org); rec = uni_p(rec); lev = uni_p(lev); raw = uni(raw);
  w = uni(w); h = uni(h); bd = uni(bd); qp = uni(qp); cbf = uni(cbf);
  const int P = w * h, sh = ts_shift(w, h, bd);
  const DequantPar d = dequant_par(0, sh, ts_qp(qp));
  unsigned long long sse = 0;
  for (int e = lane; e < P; e += 64) {
    int r = 0;
    if (cbf) {
      const int v = dequant_plain(lev[e], d);
      r = (int) (int16_t) (sh >= 0 ? (v + (sh == 0 ? 0 : 1 << (sh - 1))) >> sh : v * (1 << -sh));
    }
    recon_sample(org, rec, e, r, raw, 0, bd, sse);
  }
  wave_sync();
  sse_out = wave_sum_u64(sse);
}
