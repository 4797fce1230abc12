// vvcx_alf_stats.hip — the covariance statistics the ALF encoder derives its filters from (the O(samples) half of EL/EncAdaptiveLoopFilter.cpp,
// deriveStatsForFiltering -> getBlkStats 2746-2843 + calcCovariance 2844-2965 with m_alfWSSD off), on the pictures the ALF filter would read.
//
// Per sample and clipping bin b the vector v[.][b] holds the clipped sums of the tap pairs (in coefficient order, that is after the block's transpose index has been
// applied), the centre sample and, as one more row, d = org - rec.  Per (CTU, class) the sums E[b0][b1][k][l] = sum v[k][b0] v[l][b1], y[b][k] = sum v[k][b] d and
// pixAcc = sum d d are then the 16 x 16 products  V_b0 . V_b1^T  over the samples of the class, with V = [tap pairs | centre | d | 0 ..]: E is the upper-left nc x nc
// part, y column nc and pixAcc the entry (nc, nc) (nc = 13 luma / 7 chroma).  One workgroup OWNS one (frame, CTU, component): it stages the CTU's rec with three samples
// around it (picture borders repeat the edge sample) and its org in LDS, derives the class of every 4 x 4 block with the filter's own derivation (vvcx_alf_dev.h), sorts
// the blocks by class, and walks one class at a time, so that one class's product is live in registers and nothing is summed across workgroups.  A step multiplies four
// samples (one row of a block) on the matrix cores: v_mfma_f64_16x16x4_f64, lane l feeds row l % 16 of V_b0 / column l % 16 of V_b1^T for sample l / 16; doubles hold
// these integers exactly (|v| <= 2^13, 2^14 samples: sums below 2^41) and are written as int64.  With 4 bins wave w keeps b0 = w against all four b1; with 1 bin the
// four waves split the blocks of a class and add their parts through LDS (integer adds).  Where there are no matrix cores (VX_NO_MFMA: the CPU emulation) the same lane
// layout is multiplied out through LDS.  Nothing here is atomic and every element of the output is written exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vvcx_dev.h"
#include "vvcx_alf_dev.h"

#define AS_CTU 128
#define AS_HALO 3
#define AS_PAD 4
#define AS_LW (AS_CTU + 2 * AS_PAD)
#define AS_LH (AS_CTU + 2 * AS_HALO)

#ifdef VX_NO_MFMA
struct as_d4 { double v[4]; __device__ double &operator[](int i) { return v[i]; } };
#else
typedef double as_d4 __attribute__((ext_vector_type(4)));
#endif

// acc += A . B with A[i][k] = a of lane 16 k + i, B[k][j] = b of lane 16 k + j; lane l holds acc[(l / 16) + 4 r][l % 16] in element r
__device__ inline void as_mma(double a, double b, as_d4 &acc, double (*mm)[64], int lane)
{
#ifdef VX_NO_MFMA
  mm[0][lane] = a; mm[1][lane] = b;
  __builtin_amdgcn_wave_barrier();
  for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) acc[r] += mm[0][16 * k + (lane >> 4) + 4 * r] * mm[1][16 * k + (lane & 15)];
  __builtin_amdgcn_wave_barrier();
#else
  (void) mm; (void) lane;
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
#endif
}

template <typename T, int NB>
__device__ void alf_stats(const VxAlfStatParams &p)
{
  __shared__ int16_t rec[AS_LH][AS_LW];
  __shared__ int16_t org[AS_CTU][AS_CTU];
  __shared__ uint8_t cls_of[1024];             // class | transpose << 5 per 4 x 4 block of the CTU (blocks inside the picture, row by row)
  __shared__ uint16_t order[1024];             // the blocks sorted by class
  __shared__ int cnt[25], start[25];
  __shared__ int8_t tap_dx[4][16], tap_dy[4][16];      // per transpose index and row of V: the offset of the pair's first sample (the second one is mirrored)
  __shared__ long long red[NB == 1 ? 4 : 1][256];
#ifdef VX_NO_MFMA
  __shared__ double mm_s[4][2][64];
#endif
  const int ctu = blockIdx.x, c = blockIdx.y, f = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sh = c ? 1 : 0, pw = p.pic_w >> sh, ph = p.pic_h >> sh, lcs = 7 - sh, ctuS = 1 << lcs, nctu = p.ctus_w * p.ctus_h;
  const int ctuY = ctu / p.ctus_w, tx0 = (ctu - ctuY * p.ctus_w) << lcs, ty0 = ctuY << lcs;
  const int cw = alf_min(ctuS, pw - tx0), chh = alf_min(ctuS, ph - ty0), nbw = cw >> 2, nblk = nbw * (chh >> 2);      // the picture is a multiple of 8: whole blocks
  const int ncls = c ? 1 : 25, ntap = c ? 6 : 12, nc = ntap + 1;
  const VxFrameDev &fd = p.frames[p.frame_first + f];
  {
    const T *srec = (const T *) fd.rec[c], *sorg = (const T *) fd.org[c];
    const int st = fd.stride[c];
    for (int i = tid; i < (chh + 2 * AS_HALO) * AS_LW; i += 256) {
      const int ly = i / AS_LW, lx = i - ly * AS_LW;
      if (lx < cw + 2 * AS_PAD) rec[ly][lx] = (int16_t) srec[(size_t) alf_clampi(ty0 - AS_HALO + ly, 0, ph - 1) * st + alf_clampi(tx0 - AS_PAD + lx, 0, pw - 1)];
    }
    for (int i = tid; i < chh * AS_CTU; i += 256) {
      const int oy = i >> 7, ox = i & 127;
      if (ox < cw) org[oy][ox] = (int16_t) sorg[(size_t) (ty0 + oy) * st + tx0 + ox];
    }
    if (tid < 64) {
      const int8_t DX[12] = { 0, 1, 0, -1, 2, 1, 0, -1, -2, 3, 2, 1 }, DY[12] = { 3, 2, 2, 2, 1, 1, 1, 1, 1, 0, 0, 0 }, CH[6] = { 2, 5, 6, 7, 10, 11 };
      const int tr = tid >> 4, row = tid & 15;
      int g = -1;                                  // the tap pair (in the filter's geometric order) whose sum is row `row` of V
      if (c) { if (row < 6) g = CH[row]; }
      else for (int i = 0; i < 12; i++) if (ALF_PERM7[tr][i] == row) g = i;
      tap_dx[tr][row] = g < 0 ? 0 : DX[g]; tap_dy[tr][row] = g < 0 ? 0 : DY[g];
    }
  }
  const int vbPos = alf_vb_pos(ctuY, p.ctus_h, p.pic_h, ctuS, c);
  __syncthreads();
  // ---- classes of all blocks (luma; chroma has one), whatever the CTU's flags will be
  if (c == 0) {
    for (int q = tid; q < ((4 * nblk + 255) & ~255); q += 256) {
      const int b = alf_min(q >> 2, nblk - 1), by = b / nbw, bx = b - by * nbw;
      const int v = alf_class_of_block([&](int x, int y) { return (int) rec[y - ty0 + AS_HALO][x - tx0 + AS_PAD]; }, tx0 + 4 * bx, ty0 + 4 * by, q & 3, ctuS, vbPos, p.bit_depth);
      if ((q & 3) == 0 && (q >> 2) < nblk) cls_of[b] = (uint8_t) v;
    }
  } else for (int b = tid; b < nblk; b += 256) cls_of[b] = 0;
  __syncthreads();
  if (tid < ncls) { int n = 0; for (int b = 0; b < nblk; b++) n += (cls_of[b] & 31) == tid; cnt[tid] = n; }
  __syncthreads();
  if (tid < ncls) {
    int s = 0; for (int j = 0; j < tid; j++) s += cnt[j];
    start[tid] = s;
    for (int b = 0; b < nblk; b++) if ((cls_of[b] & 31) == tid) order[s++] = (uint16_t) b;
  }
  __syncthreads();
  // ---- one class at a time
  const int row = lane & 15, sx = lane >> 4, b0 = NB == 4 ? wave : 0;
  const size_t sz = (size_t) NB * NB * nc * nc + NB * nc + 1;
  long long *out = c ? p.chroma + (((size_t) f * nctu + ctu) * 2 + (c - 1)) * sz : p.luma + ((size_t) f * nctu + ctu) * 25 * sz;
#ifdef VX_NO_MFMA
  double (*mm)[64] = mm_s[wave];
#else
  double (*mm)[64] = nullptr;
#endif
  int clipv[NB];
#pragma unroll
  for (int b = 0; b < NB; b++) clipv[b] = p.clip[sh][b];
  for (int cls = 0; cls < ncls; cls++, out += sz) {
    as_d4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) for (int r = 0; r < 4; r++) acc[b][r] = 0.;
    const int s0 = start[cls], n = cnt[cls];
    for (int j = NB == 4 ? 0 : wave; j < n; j += NB == 4 ? 1 : 4) {
      const int b = order[s0 + j], tr = cls_of[b] >> 5, by = b / nbw, bx = b - by * nbw;
      const int dx = tap_dx[tr][row], dyi = tap_dy[tr][row], x = 4 * bx + sx;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int y = 4 * by + t, dy = alf_min(dyi, alf_vb_room(y, vbPos, c));
        const int cur = rec[y + AS_HALO][x + AS_PAD], r0 = rec[y + AS_HALO + dy][x + AS_PAD + dx], r1 = rec[y + AS_HALO - dy][x + AS_PAD - dx];
        const int d = org[y][x] - cur;
        double val[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) { const int v = alf_clip2(clipv[k], cur, r0, r1); val[k] = (double) (row == ntap ? cur : row == nc ? d : v); }
        double a = val[0];
#pragma unroll
        for (int k = 1; k < NB; k++) a = b0 == k ? val[k] : a;      // (a select, not an indexed register array)
#pragma unroll
        for (int k = 0; k < NB; k++) as_mma(a, val[k], acc[k], mm, lane);
      }
    }
    if (NB == 4) {
#pragma unroll
      for (int b1 = 0; b1 < NB; b1++) for (int r = 0; r < 4; r++) {
        const int k = sx + 4 * r, l = row;
        const long long v = (long long) acc[b1][r];
        if (k < nc && l < nc) out[((size_t) (b0 * NB + b1) * nc + k) * nc + l] = v;
        if (b1 == 0 && k < nc && l == nc) out[(size_t) NB * NB * nc * nc + b0 * nc + k] = v;
        if (b1 == 0 && b0 == 0 && k == nc && l == nc) out[sz - 1] = v;
      }
    } else {
      for (int r = 0; r < 4; r++) red[wave & (NB == 1 ? 3 : 0)][4 * lane + r] = (long long) acc[0][r];
      __syncthreads();
      {
        const int l2 = tid >> 2, r = tid & 3, k = (l2 >> 4) + 4 * r, l = l2 & 15;
        long long v = 0;
        for (int w = 0; w < (NB == 1 ? 4 : 1); w++) v += red[w][tid];
        if (k < nc && l < nc) out[(size_t) k * nc + l] = v;
        if (k < nc && l == nc) out[(size_t) nc * nc + k] = v;
        if (k == nc && l == nc) out[sz - 1] = v;
      }
      __syncthreads();
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) vvcx_alf_stats_b1_kernel_u8(VxAlfStatParams p) { alf_stats<uint8_t, 1>(p); }
extern "C" __global__ void __launch_bounds__(256) vvcx_alf_stats_b4_kernel_u8(VxAlfStatParams p) { alf_stats<uint8_t, 4>(p); }
extern "C" __global__ void __launch_bounds__(256) vvcx_alf_stats_b1_kernel_u16(VxAlfStatParams p) { alf_stats<uint16_t, 1>(p); }
extern "C" __global__ void __launch_bounds__(256) vvcx_alf_stats_b4_kernel_u16(VxAlfStatParams p) { alf_stats<uint16_t, 4>(p); }
