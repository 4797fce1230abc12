// vvcx_alf_dev.h — what the two ALF kernels share (vvcx_alf.hip: the filter; vvcx_alf_stats.hip: the encoder's covariance statistics): the class derivation of a luma
// 4 x 4 block by a quad of lanes (CL/AdaptiveLoopFilter.cpp deriveClassificationBlk 792-1002), the coefficient order of the four transpose indices and how far a row's
// vertical taps may reach next to the virtual boundary (filterBlk 1005-1296).  Device only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ static const uint8_t ALF_PERM7[4][12] = { { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 }, { 9, 4, 10, 8, 1, 5, 11, 7, 3, 0, 2, 6 }, { 0, 3, 2, 1, 8, 7, 6, 5, 4, 9, 10, 11 }, { 9, 8, 10, 4, 3, 7, 11, 5, 1, 0, 2, 6 } };
__device__ static const uint8_t ALF_TH_TAB[16] = { 0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4 };
__device__ static const uint8_t ALF_TRANSPOSE[8] = { 0, 1, 0, 2, 2, 3, 1, 3 };

__device__ inline int alf_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ inline int alf_min(int a, int b) { return a < b ? a : b; }
__device__ inline int alf_abs(int v) { return v < 0 ? -v : v; }
__device__ inline int alf_clip2(int clip, int ref, int a, int b) { return alf_clampi(a - ref, -clip, clip) + alf_clampi(b - ref, -clip, clip); }

// the virtual boundary of CTU row ctuY in rows of the component inside the CTU; in the last CTU row the reference passes the LUMA height for every component (ALFProcess
// 296, 313): only a picture of at most 128 rows reaches it
__device__ inline int alf_vb_pos(int ctuY, int ctus_h, int pic_h, int ctuS, int c) { return ctuY == ctus_h - 1 ? pic_h : ctuS - (c ? 2 : 4); }
// how far the vertical taps of row yVb (inside the CTU) may reach: tap distance j becomes min(j, room); 3 away from the boundary
__device__ inline int alf_vb_room(int yVb, int vbPos, int c)
{
  const int reach = c ? 2 : 4;
  if (yVb < vbPos && yVb >= vbPos - reach) return vbPos - 1 - yVb;
  if (yVb >= vbPos && yVb <= vbPos + reach - 1) return yVb - vbPos;
  return 3;
}

// Class | transpose << 5 of the luma 4 x 4 block at (X, Y): the four lanes of a quad (r = lane & 3, neighbouring lanes) call this together, lane r takes the pair r of the
// window's rows and the sums are added across the quad; every lane of the quad returns the value.  at(x, y) = the sample at picture position (x, y) (two samples around
// the 8 x 8 window are read: the staged area repeats the picture's edge samples).  All lanes of the wave must call it (shuffles).
template <typename At>
__device__ inline int alf_class_of_block(At at, int X, int Y, int r, int ctuS, int vbPos, int bit_depth)
{
  const int yIn = Y & (ctuS - 1);
  int sV = 0, sH = 0, sD0 = 0, sD1 = 0;
  const bool skip = (yIn == vbPos - 4 && r == 3) || (yIn == vbPos && r == 0);      // the window does not cross the boundary
  if (!skip) {
    const int y1 = Y - 2 + 2 * r, y2 = y1 + 1;
    int y0 = y1 - 1, y3 = y2 + 1;
    if (y1 > 0 && (y1 & (ctuS - 1)) == vbPos - 2) y3 = y2; else if (y1 > 0 && (y1 & (ctuS - 1)) == vbPos) y0 = y1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int x = X - 2 + 2 * k;
      const int a = at(x, y1) << 1, bb = at(x + 1, y2) << 1;
      sV += alf_abs(a - at(x, y0) - at(x, y2)) + alf_abs(bb - at(x + 1, y1) - at(x + 1, y3));
      sH += alf_abs(a - at(x + 1, y1) - at(x - 1, y1)) + alf_abs(bb - at(x + 2, y2) - at(x, y2));
      sD0 += alf_abs(a - at(x - 1, y0) - at(x + 1, y2)) + alf_abs(bb - at(x, y1) - at(x + 2, y3));
      sD1 += alf_abs(a - at(x - 1, y2) - at(x + 1, y0)) + alf_abs(bb - at(x, y3) - at(x + 2, y1));
    }
  }
  sV += __shfl_xor(sV, 1); sH += __shfl_xor(sH, 1); sD0 += __shfl_xor(sD0, 1); sD1 += __shfl_xor(sD1, 1);
  sV += __shfl_xor(sV, 2); sH += __shfl_xor(sH, 2); sD0 += __shfl_xor(sD0, 2); sD1 += __shfl_xor(sD1, 2);
  const int scaled = (yIn == vbPos - 4 || yIn == vbPos) ? 96 : 64;
  int cls = ALF_TH_TAB[alf_clampi(((sV + sH) * scaled) >> (bit_depth + 4), 0, 15)];
  int hv1, hv0, d1, d0, dirHV, dirD, hvd1, hvd0, mainDir, secDir;
  if (sV > sH) { hv1 = sV; hv0 = sH; dirHV = 1; } else { hv1 = sH; hv0 = sV; dirHV = 3; }
  if (sD0 > sD1) { d1 = sD0; d0 = sD1; dirD = 0; } else { d1 = sD1; d0 = sD0; dirD = 2; }
  if ((uint32_t) d1 * (uint32_t) hv0 > (uint32_t) hv1 * (uint32_t) d0) { hvd1 = d1; hvd0 = d0; mainDir = dirD; secDir = dirHV; }
  else { hvd1 = hv1; hvd0 = hv0; mainDir = dirHV; secDir = dirD; }
  int strength = 0;
  if (hvd1 > 2 * hvd0) strength = 1;
  if (hvd1 * 2 > 9 * hvd0) strength = 2;
  if (strength) cls += (((mainDir & 1) << 1) + strength) * 5;
  return cls | (ALF_TRANSPOSE[mainDir * 2 + (secDir >> 1)] << 5);
}
