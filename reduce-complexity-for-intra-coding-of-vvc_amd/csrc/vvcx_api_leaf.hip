// vvcx_api_leaf.hip — the leaf operators of the C-ABI (include/vvcx.h): one batch entry per kernel that the tests pin against the reference on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "vvcx.h"
#include "vvcx_handle.h"      // the handle, fail, dq_consts_of, ctx_init_islice
#include "vvcx_kernels.h"
#include "vvcx_tables.h"      // host copy of the constant tables: the reference's flat order of the context models

static void ctx_from_reference_order(const uint16_t *s0, const uint16_t *s1, uint16_t *kept)      // kept: s0[VXD_NUM_CTX] | s1[VXD_NUM_CTX]
{
  for (int k = 0; k < VXD_NUM_CTX; k++) { kept[k] = s0[VX_CTX_REF_INDEX[k]]; kept[VXD_NUM_CTX + k] = s1[VX_CTX_REF_INDEX[k]]; }
}


// ------------------------------------------------------------------------------------------------ leaf operators
namespace {
bool pow2_block(int w, int h) { return w >= 2 && h >= 2 && w <= 64 && h <= 64 && !(w & (w - 1)) && !(h & (h - 1)); }
}

extern "C" int vvcx_distortion_batch(const int16_t *a, const int16_t *b, int w, int h, int n, uint64_t *out, int device)
{
  if (!a || !b || !out || n < 0 || !pow2_block(w, h)) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const size_t bytes = (size_t) n * w * h * 2;
  DevBuf<int16_t> da, db, ds; DevBuf<unsigned long long> dout;
  HIPCHK(da.alloc(bytes / 2)); HIPCHK(db.alloc(bytes / 2)); HIPCHK(ds.alloc(bytes / 2)); HIPCHK(dout.alloc((size_t) n * 3));
  HIPCHK(hipMemcpy(da.p, a, bytes, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(db.p, b, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vvcx_leaf_dist_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, da.p, db.p, w, h, ds.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout.p, (size_t) n * 3 * 8, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

extern "C" int vvcx_intra_pred_batch(vvcx_handle *h, const void *const reco[3], const uint8_t *const coded[2], const vvcx_pred_case *cases, int n, int16_t *pred)
{
  NOT_PENDING(h);
  if (!h || !reco || !coded || !cases || !pred || n < 0) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(h->cfg.device);
  const int bps = h->cfg.bit_depth == 8 ? 1 : 2, W = h->cfg.pic_w, H = h->cfg.pic_h;
  std::vector<int> off((size_t) n); size_t total = 0; bool any_lm = false;
  for (int i = 0; i < n; i++) {
    const vvcx_pred_case &c = cases[i];
    const int cw = c.comp ? W >> 1 : W, chh = c.comp ? H >> 1 : H;
    const bool lm = c.mode >= 67 && c.mode <= 69;                          // LM / MDLM_L / MDLM_T: chroma blocks of at least 4 x 2 samples, at most 32 x 32 (a 64 x 64 chroma-tree node)
    if (c.comp < 0 || c.comp > 2 || !pow2_block(c.w, c.h) || c.x < 0 || c.y < 0 || c.x + c.w > cw || c.y + c.h > chh || c.mode < 0 || (c.mode > 66 && !lm) ||
        (lm && (c.comp == 0 || c.w < 4 || c.w > 32 || c.h > 32 || (c.x & 1) || (c.y & 1))) ||
        (c.mrl != 0 && (c.comp != 0 || (c.mrl != 1 && c.mrl != 3)))) return fail(VVCX_ERR_ARG, "bad prediction case %d", i);
    any_lm |= lm;
    off[(size_t) i] = (int) total; total += (size_t) c.w * c.h;
  }
  DevBuf<uint8_t> dplane[3]; DevBuf<VxUnit> dunits; DevBuf<VxFrameDev> dframe; DevBuf<VxLeafPred> dcases; DevBuf<int> doff; DevBuf<int16_t> dpred;
  VxFrameDev fd; memset(&fd, 0, sizeof fd);
  for (int c = 0; c < 3; c++) {
    const size_t pw = c ? W >> 1 : W, ph = c ? H >> 1 : H;
    if (!reco[c]) return fail(VVCX_ERR_ARG, "plane %d is null", c);
    HIPCHK(dplane[c].alloc(pw * ph * bps)); HIPCHK(hipMemcpy(dplane[c].p, reco[c], pw * ph * bps, hipMemcpyHostToDevice));
    fd.org[c] = dplane[c].p; fd.rec[c] = dplane[c].p; fd.stride[c] = (int32_t) pw;
  }
  const size_t nu = (size_t) h->uw * h->uh;
  std::vector<VxUnit> units(2 * nu); memset(units.data(), 0, units.size() * sizeof(VxUnit));
  for (int t = 0; t < 2; t++) { if (!coded[t]) return fail(VVCX_ERR_ARG, "coded map %d is null", t); for (size_t i = 0; i < nu; i++) units[(size_t) t * nu + i].tag = coded[t][i] ? 1 : 0; }
  HIPCHK(dunits.alloc(units.size())); HIPCHK(hipMemcpy(dunits.p, units.data(), units.size() * sizeof(VxUnit), hipMemcpyHostToDevice));
  fd.units[0] = dunits.p; fd.units[1] = dunits.p + nu;
  HIPCHK(dframe.alloc(1)); HIPCHK(hipMemcpy(dframe.p, &fd, sizeof fd, hipMemcpyHostToDevice));
  HIPCHK(dcases.alloc((size_t) n)); HIPCHK(hipMemcpy(dcases.p, cases, (size_t) n * sizeof(VxLeafPred), hipMemcpyHostToDevice));
  HIPCHK(doff.alloc((size_t) n)); HIPCHK(hipMemcpy(doff.p, off.data(), (size_t) n * 4, hipMemcpyHostToDevice));
  HIPCHK(dpred.alloc(total));
  VxParams p; memset(&p, 0, sizeof p);
  p.pic_w = W; p.pic_h = H; p.bit_depth = h->cfg.bit_depth; p.tools = h->cfg.tools; p.uw = h->uw; p.uh = h->uh; p.frames = dframe.p;
  DevBuf<uint8_t> dscr;                                                    // the CCLM modes keep the down-sampled luma of a big block in the workgroup's scratch slice (VXD_OFF_LM)
  if (any_lm) { HIPCHK(dscr.alloc((size_t) n * VXD_OFF_DQ)); p.scratch = dscr.p; p.scratch_per_stream = VXD_OFF_DQ; }
  if (bps == 1) hipLaunchKernelGGL(vvcx_leaf_pred_kernel_u8, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dcases.p, dpred.p, doff.p);
  else hipLaunchKernelGGL(vvcx_leaf_pred_kernel_u16, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dcases.p, dpred.p, doff.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(pred, dpred.p, total * 2, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// the leaf operators exchange whole context arrays in the reference's flat order (ContextSetCfg, 386 models); the library keeps the models an intra slice touches
// (VXD_NUM_CTX, vvcx_tables.h VX_CTX_REF_INDEX)
extern "C" int vvcx_ctx_init(int qp, uint16_t *s0, uint16_t *s1)
{
  if (!s0 || !s1) return fail(VVCX_ERR_ARG, "null argument");
  qp = qp < 0 ? 0 : qp > 63 ? 63 : qp;
  for (int k = 0; k < VX_NUM_CTX_REF; k++) {               // CtxStore::init for an I slice, every model of the reference (ctx_init_islice: the kept ones)
    const int id = VX_CTX_INIT_I_REF[k];
    const int slope = (id >> 3) - 4, offset = ((id & 7) * 18) + 1;
    int st = ((slope * (qp - 16)) >> 1) + offset;
    st = st < 1 ? 1 : st > 127 ? 127 : st;
    const int p1 = st << 8;
    s0[k] = (uint16_t) (p1 & 0x7FE0); s1[k] = (uint16_t) (p1 & 0x7FFE);
  }
  return VVCX_OK;
}

extern "C" int vvcx_cabac_code_bins(uint16_t *s0, uint16_t *s1, int ctx, const uint8_t *bins, int nbins, uint64_t *frac_bits, int device)
{
  if (!s0 || !s1 || !bins || !frac_bits || nbins < 0 || ctx < 0 || ctx >= VX_NUM_CTX_REF) return fail(VVCX_ERR_ARG, "bad argument");      // ctx: the reference's flat index; only its adaptation rate matters
  ON_DEVICE(device);
  DevBuf<uint16_t> dio; DevBuf<uint8_t> dbins; DevBuf<unsigned long long> dbits;
  uint16_t io[2] = { *s0, *s1 };
  HIPCHK(dio.alloc(2)); HIPCHK(dbins.alloc((size_t) nbins)); HIPCHK(dbits.alloc(1));
  HIPCHK(hipMemcpy(dio.p, io, 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dbins.p, bins, (size_t) nbins, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vvcx_leaf_cabac_kernel, dim3(1), dim3(VXD_NT), 0, 0, dio.p, (int) VX_CTX_RATE_REF[ctx], dbins.p, nbins, dbits.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(io, dio.p, 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(frac_bits, dbits.p, 8, hipMemcpyDeviceToHost));
  *s0 = io[0]; *s1 = io[1];
  return VVCX_OK;
}

extern "C" int vvcx_rd_cost_batch(double lambda, const uint64_t *frac_bits, const uint64_t *dist, int n, double *cost, int device)
{
  if (!(lambda > 0.0) || !frac_bits || !dist || !cost || n < 0) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  DevBuf<unsigned long long> db, dd; DevBuf<double> dc;
  HIPCHK(db.alloc((size_t) n)); HIPCHK(dd.alloc((size_t) n)); HIPCHK(dc.alloc((size_t) n));
  HIPCHK(hipMemcpy(db.p, frac_bits, (size_t) n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dd.p, dist, (size_t) n * 8, hipMemcpyHostToDevice));
  VxParams p; memset(&p, 0, sizeof p);
  p.lambda = lambda; p.dist_scale = (double) (1 << 15) / lambda;
  hipLaunchKernelGGL(vvcx_leaf_rdcost_kernel, dim3((unsigned) ((n + VXD_NT - 1) / VXD_NT)), dim3(VXD_NT), 0, 0, p, db.p, dd.p, n, dc.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(cost, dc.p, (size_t) n * 8, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

extern "C" int vvcx_scan_order(int w, int h, uint16_t *idx, int device)
{
  if (!idx || !pow2_block(w, h)) return fail(VVCX_ERR_ARG, "bad argument");
  ON_DEVICE(device);
  const int n = (w < 32 ? w : 32) * (h < 32 ? h : 32);
  DevBuf<uint16_t> d; HIPCHK(d.alloc((size_t) n));
  hipLaunchKernelGGL(vvcx_leaf_scan_kernel, dim3(1), dim3(VXD_NT), 0, 0, w, h, d.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(idx, d.p, (size_t) n * 2, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// ≙ IntraPrediction::initIntraMip + predIntraMip (CL/IntraPrediction.cpp:2152-2205) for n blocks: case i = {w, h, mode, bit_depth}, its
// unfiltered line-0 reference samples top[w] | left[h] at refs + ref_off[i], prediction (w*h, stride w) to pred + pred_off[i]; host pointers
extern "C" int vvcx_mip_pred_batch(const int32_t *cases, int n, const int16_t *refs, int n_refs, int16_t *pred, int n_pred, int device)
{
  if (!cases || !refs || !pred || n < 0) return fail(VVCX_ERR_ARG, "bad argument");
  std::vector<VxMipCase> cs((size_t) n);
  int ro = 0, po = 0;
  for (int i = 0; i < n; i++) {
    const int w = cases[4 * i], h = cases[4 * i + 1], mode = cases[4 * i + 2], bd = cases[4 * i + 3];
    const bool shape = pow2_block(w, h) && w <= 64 && h <= 64 && w <= 4 * h && h <= 4 * w;
    const int nm = !shape ? 0 : (w == 4 && h == 4) ? 35 : (w <= 8 && h <= 8) ? 19 : 11;
    if (!shape || mode < 0 || mode >= nm || (bd != 8 && bd != 10)) return fail(VVCX_ERR_ARG, "MIP case %d: block %dx%d mode %d bit depth %d", i, w, h, mode, bd);
    cs[(size_t) i] = { w, h, mode, bd, ro, po };
    ro += w + h; po += w * h;
  }
  if (ro > n_refs || po > n_pred) return fail(VVCX_ERR_ARG, "reference / prediction buffers too small");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  DevBuf<VxMipCase> dc; DevBuf<int16_t> dr, dp; HIPCHK(dc.alloc((size_t) n)); HIPCHK(dr.alloc((size_t) ro)); HIPCHK(dp.alloc((size_t) po));
  HIPCHK(hipMemcpy(dc.p, cs.data(), sizeof(VxMipCase) * (size_t) n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dr.p, refs, (size_t) ro * 2, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vvcx_leaf_mip_kernel, dim3((unsigned) n), dim3(64), 0, 0, dc.p, dr.p, dp.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(pred, dp.p, (size_t) po * 2, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// ≙ GetPartition(C0..C25, 2) of BIN/TEST.py for n feature rows (26 int32 each, host pointers): the forest set with vvcx_set_forest
extern "C" int vvcx_forest_predict_batch(vvcx_handle *h, const int32_t *rows, int n, int32_t *out)
{
  NOT_PENDING(h);
  if (!h || !rows || !out || n < 0) return fail(VVCX_ERR_ARG, "bad argument");
  if (!h->f_ntrees) return fail(VVCX_ERR_STATE, "vvcx_set_forest first");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(h->cfg.device);
  DevBuf<int32_t> dr, dout; HIPCHK(dr.alloc((size_t) n * 26)); HIPCHK(dout.alloc((size_t) n));
  HIPCHK(hipMemcpy(dr.p, rows, (size_t) n * 26 * 4, hipMemcpyHostToDevice));
  VxParams p; memset(&p, 0, sizeof p);
  p.f_node = h->f_node_d.p; p.f_value = h->f_value_d.p; p.f_root = h->f_root_d.p; p.f_ntrees = h->f_ntrees; p.f_nclasses = h->f_nclasses;
  for (int c = 0; c < 8; c++) p.f_classes[c] = h->f_classes[c];
  hipLaunchKernelGGL(vvcx_leaf_forest_kernel, dim3((unsigned) ((n + VXD_NT - 1) / VXD_NT)), dim3(VXD_NT), 0, 0, p, dr.p, n, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout.p, (size_t) n * 4, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

extern "C" int vvcx_transform_quant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int n,
                                          int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device)
{
  if (!org || !pred || !lev || !rec || !sse || !cbf || n < 0 || !pow2_block(w, h) || (bit_depth != 8 && bit_depth != 10) || qp < 0 || qp > 75) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const size_t bytes = (size_t) n * w * h * 2;
  DevBuf<int16_t> dorg, drec, dlev; DevBuf<int32_t> dtmp; DevBuf<unsigned long long> dout;
  HIPCHK(dorg.alloc(bytes / 2)); HIPCHK(drec.alloc(bytes / 2)); HIPCHK(dlev.alloc(bytes / 2)); HIPCHK(dtmp.alloc((size_t) n * 2048)); HIPCHK(dout.alloc((size_t) n * 2));
  HIPCHK(hipMemcpy(dorg.p, org, bytes, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(drec.p, pred, bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vvcx_leaf_trq_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, dorg.p, drec.p, dlev.p, dtmp.p, w, h, bit_depth, qp,
                     dout.p);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> o((size_t) n * 2);
  HIPCHK(hipMemcpy(lev, dlev.p, bytes, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(rec, drec.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o.data(), dout.p, (size_t) n * 16, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) { sse[i] = o[(size_t) i * 2]; cbf[i] = (uint8_t) o[(size_t) i * 2 + 1]; }
  return VVCX_OK;
}

static int depquant_batch_impl(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int comp, int mts_idx, int cbf_cb, double lambda,
                               const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device, int lfnst_idx, int intra_dir)
{
  if (!org || !pred || !lev || !rec || !sse || !cbf || !s0 || !s1 || n < 0 || !pow2_block(w, h) || (bit_depth != 8 && bit_depth != 10) || qp < 0 || qp > 75 || comp < 0 || comp > 2 ||
      !(lambda > 0.0) || (mts_idx != 0 && (mts_idx < 2 || mts_idx > 5 || comp != 0 || w > 32 || h > 32 || w < 4 || h < 4))) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const size_t bytes = (size_t) n * w * h * 2;
  DevBuf<int16_t> dorg, drec, dlev; DevBuf<int32_t> dtmp; DevBuf<unsigned long long> dout; DevBuf<uint16_t> dctx; DevBuf<VxDqConst> dtab; DevBuf<uint8_t> dscr;
  HIPCHK(dorg.alloc(bytes / 2)); HIPCHK(drec.alloc(bytes / 2)); HIPCHK(dlev.alloc(bytes / 2)); HIPCHK(dtmp.alloc((size_t) n * 2048)); HIPCHK(dout.alloc((size_t) n * 2));
  HIPCHK(dctx.alloc(2 * VXD_NUM_CTX)); HIPCHK(dtab.alloc(48)); HIPCHK(dscr.alloc((size_t) n * VXD_OFF_CACHE));
  HIPCHK(hipMemcpy(dorg.p, org, bytes, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(drec.p, pred, bytes, hipMemcpyHostToDevice));
  { uint16_t kept[2 * VXD_NUM_CTX]; ctx_from_reference_order(s0, s1, kept); HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); }
  VxDqConst tab[48]; memset(tab, 0, sizeof tab);
  for (int lsum = 2; lsum <= 12; lsum++) tab[comp * 16 + lsum] = dq_consts_of(lsum, bit_depth, qp, lambda);
  HIPCHK(hipMemcpy(dtab.p, tab, sizeof tab, hipMemcpyHostToDevice));
  VxParams p; memset(&p, 0, sizeof p);
  p.bit_depth = bit_depth; p.tools = VVCX_TOOL_DEPQUANT | VVCX_TOOL_MTS | (lfnst_idx ? VVCX_TOOL_LFNST : 0); p.dq_consts = dtab.p; p.scratch = dscr.p; p.scratch_per_stream = VXD_OFF_CACHE;
  hipLaunchKernelGGL(vvcx_leaf_dq_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dctx.p, dorg.p, drec.p, dlev.p, dtmp.p,
                     w, h, qp, comp, mts_idx, cbf_cb, dout.p, (w >= 4 && h >= 4) ? lfnst_idx : 0, intra_dir);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> o((size_t) n * 2);
  HIPCHK(hipMemcpy(lev, dlev.p, bytes, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(rec, drec.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o.data(), dout.p, (size_t) n * 16, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) { sse[i] = o[(size_t) i * 2]; cbf[i] = (uint8_t) o[(size_t) i * 2 + 1]; }
  return VVCX_OK;
}

extern "C" int vvcx_depquant_items(const int16_t *coef, int w, int h, int bit_depth, int qp, double lambda, const uint16_t *s0, const uint16_t *s1, int n,
                                   int16_t *lev, int32_t *abs_sum, int *max_items, int device)
{
  if (!coef || !lev || !abs_sum || !s0 || !s1 || n < 0 || n > 16 || !pow2_block(w, h) || w < 4 || h < 4 || w > 32 || h > 32 || (bit_depth != 8 && bit_depth != 10) || qp < 0 || qp > 75 ||
      !(lambda > 0.0)) return fail(VVCX_ERR_ARG, "bad argument");
  ON_DEVICE(device);
  const size_t P = (size_t) w * h;
  DevBuf<int16_t> dcoef; DevBuf<uint8_t> dnodes; DevBuf<int> dout; DevBuf<uint16_t> dctx; DevBuf<VxDqConst> dtab;
  HIPCHK(dcoef.alloc(P * 16)); HIPCHK(dnodes.alloc(4 * P * 16)); HIPCHK(dout.alloc(17)); HIPCHK(dctx.alloc(2 * VXD_NUM_CTX)); HIPCHK(dtab.alloc(48));
  HIPCHK(hipMemset(dcoef.p, 0, P * 16 * 2)); HIPCHK(hipMemset(dnodes.p, 0, 4 * P * 16)); HIPCHK(hipMemset(dout.p, 0, 17 * sizeof(int)));
  if (n) HIPCHK(hipMemcpy(dcoef.p, coef, P * n * 2, hipMemcpyHostToDevice));
  { uint16_t kept[2 * VXD_NUM_CTX]; ctx_from_reference_order(s0, s1, kept); HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); }
  VxDqConst tab[48]; memset(tab, 0, sizeof tab);
  for (int lsum = 2; lsum <= 12; lsum++) tab[lsum] = dq_consts_of(lsum, bit_depth, qp, lambda);
  HIPCHK(hipMemcpy(dtab.p, tab, sizeof tab, hipMemcpyHostToDevice));
  VxParams p; memset(&p, 0, sizeof p);
  p.bit_depth = bit_depth; p.tools = VVCX_TOOL_DEPQUANT; p.dq_consts = dtab.p;
  hipLaunchKernelGGL(vvcx_leaf_dq_items_kernel, dim3(1), dim3(VXD_NT), 0, 0, p, dctx.p, dcoef.p, dnodes.p, n, w, h, dout.p);
  HIPCHK(hipGetLastError());
  int o[17];
  HIPCHK(hipMemcpy(o, dout.p, sizeof o, hipMemcpyDeviceToHost));
  if (max_items) *max_items = o[16];
  if (n > o[16]) return fail(VVCX_ERR_ARG, "more blocks than one wave takes for the shape");
  if (n) HIPCHK(hipMemcpy(lev, dcoef.p, P * n * 2, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) abs_sum[i] = o[i];
  return VVCX_OK;
}

extern "C" int vvcx_depquant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int comp, int mts_idx, int cbf_cb, double lambda,
                                   const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device)
{
  return depquant_batch_impl(org, pred, w, h, bit_depth, qp, comp, mts_idx, cbf_cb, lambda, s0, s1, n, lev, rec, sse, cbf, device, 0, 0);
}
extern "C" int vvcx_lfnst_depquant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int comp, int lfnst_idx, int intra_dir, int cbf_cb, double lambda,
                                         const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device)
{
  if (lfnst_idx < 0 || lfnst_idx > 2 || intra_dir < 0 || intra_dir > 66) return fail(VVCX_ERR_ARG, "bad argument");
  return depquant_batch_impl(org, pred, w, h, bit_depth, qp, comp, 0, cbf_cb, lambda, s0, s1, n, lev, rec, sse, cbf, device, lfnst_idx, intra_dir);
}

// ≙ TrQuant::transformNxN / DepQuant::quant / invTransformNxN of one luma TU (tw x th: 1 x N, 2 x N, N x 1, N x 2 or larger) of a CU with cu.ispMode set: implicit DST-VII /
// DCT-II (getTrTypes 752-780), the one-stage transforms of one-sample-wide blocks, the cbf context of ISP sub-partitions (QtCbf[Y] + 2 + prev_cbf; inferred: no cbf rate)
extern "C" int vvcx_isp_tu_batch(const int16_t *org, const int16_t *pred, int tw, int th, int bit_depth, int qp, double lambda, int prev_cbf, int cbf_inferred,
                                 const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device)
{
  const bool shape = tw >= 1 && th >= 1 && tw <= 64 && th <= 64 && !(tw & (tw - 1)) && !(th & (th - 1)) && tw * th >= 16;
  if (!org || !pred || !lev || !rec || !sse || !cbf || !s0 || !s1 || n < 0 || !shape || (bit_depth != 8 && bit_depth != 10) || qp < 0 || qp > 75 || !(lambda > 0.0)) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const size_t bytes = (size_t) n * tw * th * 2;
  DevBuf<int16_t> dorg, drec, dlev; DevBuf<int32_t> dtmp; DevBuf<unsigned long long> dout; DevBuf<uint16_t> dctx; DevBuf<VxDqConst> dtab; DevBuf<uint8_t> dscr;
  HIPCHK(dorg.alloc(bytes / 2)); HIPCHK(drec.alloc(bytes / 2)); HIPCHK(dlev.alloc(bytes / 2)); HIPCHK(dtmp.alloc((size_t) n * 2048)); HIPCHK(dout.alloc((size_t) n * 2));
  HIPCHK(dctx.alloc(2 * VXD_NUM_CTX)); HIPCHK(dtab.alloc(96)); HIPCHK(dscr.alloc((size_t) n * VXD_OFF_CACHE));
  HIPCHK(hipMemcpy(dorg.p, org, bytes, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(drec.p, pred, bytes, hipMemcpyHostToDevice));
  { uint16_t kept[2 * VXD_NUM_CTX]; ctx_from_reference_order(s0, s1, kept); HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); }
  VxDqConst tab[96]; memset(tab, 0, sizeof tab);
  for (int lsum = 2; lsum <= 12; lsum++) tab[lsum] = dq_consts_of(lsum, bit_depth, qp, lambda);
  HIPCHK(hipMemcpy(dtab.p, tab, sizeof tab, hipMemcpyHostToDevice));
  VxParams p; memset(&p, 0, sizeof p);
  p.bit_depth = bit_depth; p.tools = VVCX_TOOL_DEPQUANT | VVCX_TOOL_MTS | VVCX_TOOL_LFNST | VVCX_TOOL_ISP; p.dq_consts = dtab.p; p.scratch = dscr.p; p.scratch_per_stream = VXD_OFF_CACHE;
  p.lambda = lambda;
  hipLaunchKernelGGL(vvcx_leaf_isp_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dctx.p, dorg.p, drec.p, dlev.p, dtmp.p,
                     tw, th, qp, cbf_inferred ? -1 : (int) VX_CTX_QtCbf[0] + 2 + (prev_cbf ? 1 : 0), dout.p);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> o((size_t) n * 2);
  HIPCHK(hipMemcpy(lev, dlev.p, bytes, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(rec, drec.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o.data(), dout.p, (size_t) n * 16, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) { sse[i] = o[(size_t) i * 2]; cbf[i] = (uint8_t) o[(size_t) i * 2 + 1]; }
  return VVCX_OK;
}

// ≙ TrQuant::transformNxN / invTransformNxN of a luma TU with tu.mtsIdx = MTS_SKIP and the {DCT2, TS} pruning in front of it (CL/TrQuant.cpp:1049-1124, 1394-1440, 996-1041),
// QuantRDOQ::xRateDistOptQuantTS (CL/QuantRDOQ.cpp:1243-1483), CABACWriter::residual_codingTS (EL/CABACWriter.cpp:4306-4555) for n residual blocks (host pointers, stride w):
// levels, reconstructed residual, absSum, whether the pruning keeps the candidate, and the fractional bits of the levels from the given context models
extern "C" int vvcx_transform_skip_batch(const int16_t *resi, int w, int h, int bit_depth, int qp, double lambda, const uint16_t *s0, const uint16_t *s1, int n,
                                         int16_t *lev, int16_t *resi_out, int32_t *abs_sum, uint8_t *keep, uint64_t *frac_bits, int device)
{
  if (!resi || !lev || !resi_out || !abs_sum || !keep || !frac_bits || !s0 || !s1 || n < 0 || !pow2_block(w, h) || w < 4 || h < 4 || w > 32 || h > 32 || (bit_depth != 8 && bit_depth != 10) ||
      qp < 0 || qp > 75 || !(lambda > 0.0)) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const size_t bytes = (size_t) n * w * h * 2;
  DevBuf<int16_t> dres, dout, dlev; DevBuf<int32_t> dtmp; DevBuf<int> do2; DevBuf<unsigned long long> dbits; DevBuf<uint16_t> dctx;
  HIPCHK(dres.alloc(bytes / 2)); HIPCHK(dout.alloc(bytes / 2)); HIPCHK(dlev.alloc(bytes / 2)); HIPCHK(dtmp.alloc((size_t) n * 2048)); HIPCHK(do2.alloc((size_t) n * 2)); HIPCHK(dbits.alloc((size_t) n));
  HIPCHK(dctx.alloc(2 * VXD_NUM_CTX));
  HIPCHK(hipMemcpy(dres.p, resi, bytes, hipMemcpyHostToDevice)); HIPCHK(hipMemset(dout.p, 0, bytes));
  { uint16_t kept[2 * VXD_NUM_CTX]; ctx_from_reference_order(s0, s1, kept); HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); }
  VxParams p; memset(&p, 0, sizeof p);
  p.bit_depth = bit_depth; p.tools = VVCX_TOOL_DEPQUANT | VVCX_TOOL_LFNST | VVCX_TOOL_TS; p.lambda = lambda;
  hipLaunchKernelGGL(vvcx_leaf_ts_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dctx.p, dres.p, dlev.p, dout.p, dtmp.p, w, h, qp,
                     do2.p, dbits.p);
  HIPCHK(hipGetLastError());
  std::vector<int> o((size_t) n * 2);
  HIPCHK(hipMemcpy(lev, dlev.p, bytes, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(resi_out, dout.p, bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(o.data(), do2.p, (size_t) n * 8, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(frac_bits, dbits.p, (size_t) n * 8, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) { abs_sum[i] = o[(size_t) i * 2]; keep[i] = (uint8_t) o[(size_t) i * 2 + 1]; }
  return VVCX_OK;
}

static void ctx_to_reference_order(const uint16_t *kept, uint16_t *s0, uint16_t *s1)      // the models the library keeps, back into arrays that hold the start states
{
  for (int k = 0; k < VXD_NUM_CTX; k++) { s0[VX_CTX_REF_INDEX[k]] = kept[k]; s1[VX_CTX_REF_INDEX[k]] = kept[VXD_NUM_CTX + k]; }
}

// ≙ CABACWriter::residual_coding (EL/CABACWriter.cpp:3773-3883) / residual_codingTS (4306-4555) of n blocks of levels, each from the same start states, in one of the
// forms the path has; see include/vvcx.h
extern "C" int vvcx_residual_coding_batch(const int16_t *lev, int w, int h, int n, int comp, uint32_t tools, int ts_allowed, int mts_allowed, int mts_idx,
                                          const uint16_t *s0, const uint16_t *s1, int form, uint64_t *frac_bits, uint16_t *s0_out, uint16_t *s1_out, int32_t *rc_last,
                                          uint8_t *bytes, int bytes_cap, int32_t *nbytes, int device)
{
  const bool shape = w >= 1 && h >= 1 && w <= 64 && h <= 64 && !(w & (w - 1)) && !(h & (h - 1)) && w * h >= 4;
  if (!lev || !s0 || !s1 || !frac_bits || !s0_out || !s1_out || !rc_last || n < 0 || !shape || comp < 0 || comp > 1 || form < 0 || form > 3 || mts_idx < 0 || mts_idx > 5)
    return fail(VVCX_ERR_ARG, "bad argument");
  const bool small = w <= 32 && h <= 32;
  if ((ts_allowed || mts_allowed || mts_idx) && (comp != 0 || !small)) return fail(VVCX_ERR_ARG, "transform indices belong to luma blocks of at most 32 x 32");
  if ((mts_idx == 1 && (!ts_allowed || w < 4 || h < 4)) || (mts_idx > 1 && !mts_allowed)) return fail(VVCX_ERR_ARG, "mts_idx %d is not allowed for the block", mts_idx);
  if (mts_idx == 1 && (form == 1 || form == 2)) return fail(VVCX_ERR_ARG, "transform-skip levels have no wave form");
  if (form == 1 && w * h > VXD_BUF) return fail(VVCX_ERR_ARG, "form 1 takes blocks of at most %d levels", VXD_BUF);
  if (form == 3 && (!bytes || !nbytes || bytes_cap <= 0)) return fail(VVCX_ERR_ARG, "form 3 needs a byte buffer");
  const int P = w * h, zw = (mts_idx > 1 && w == 32) ? 16 : (mts_idx == 1 || w < 32) ? w : 32, zh = (mts_idx > 1 && h == 32) ? 16 : (mts_idx == 1 || h < 32) ? h : 32;
  for (int i = 0; i < n; i++) {
    bool any = false;
    for (int y = 0; y < h; y++) for (int x = 0; x < w; x++) {
      const int v = lev[(size_t) i * P + y * w + x];
      if (v && (x >= zw || y >= zh)) return fail(VVCX_ERR_ARG, "block %d has a level in its zeroed area", i);
      any |= v != 0;
    }
    if (!any) return fail(VVCX_ERR_ARG, "block %d has no level (residual coding needs cbf = 1)", i);
  }
  if (n == 0) return VVCX_OK;
  ON_DEVICE(device);
  const uint32_t cap = form == 3 ? (uint32_t) bytes_cap : 0;
  DevBuf<int16_t> dlev; DevBuf<uint16_t> dctx, dscan, dco; DevBuf<unsigned long long> dout; DevBuf<uint8_t> dby; DevBuf<uint32_t> dnb;
  HIPCHK(dlev.alloc((size_t) n * P)); HIPCHK(dctx.alloc(2 * VXD_NUM_CTX)); HIPCHK(dscan.alloc((size_t) n * 1024)); HIPCHK(dco.alloc((size_t) n * 2 * VXD_NUM_CTX));
  HIPCHK(dout.alloc((size_t) n * 2)); HIPCHK(dby.alloc((size_t) n * cap + 1)); HIPCHK(dnb.alloc((size_t) n));
  HIPCHK(hipMemcpy(dlev.p, lev, (size_t) n * P * 2, hipMemcpyHostToDevice));
  { uint16_t kept[2 * VXD_NUM_CTX]; ctx_from_reference_order(s0, s1, kept); HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); }
  HIPCHK(hipMemset(dnb.p, 0, (size_t) n * 4));
  VxParams p; memset(&p, 0, sizeof p);
  p.bit_depth = 8; p.tools = (tools & VVCX_TOOL_DEPQUANT) | (ts_allowed ? VVCX_TOOL_TS : 0) | (mts_allowed ? VVCX_TOOL_MTS : 0);
  hipLaunchKernelGGL(vvcx_leaf_rc_kernel, dim3((unsigned) n), dim3(VXD_NT), 0, 0, p, dctx.p, dlev.p, w, h, comp, mts_idx, form, dscan.p, dco.p, dout.p, dby.p, cap, dnb.p);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> o((size_t) n * 2); std::vector<uint16_t> co((size_t) n * 2 * VXD_NUM_CTX); std::vector<uint32_t> nb((size_t) n);
  HIPCHK(hipMemcpy(o.data(), dout.p, (size_t) n * 16, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(co.data(), dco.p, co.size() * 2, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nb.data(), dnb.p, (size_t) n * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    frac_bits[i] = o[(size_t) i * 2]; rc_last[i] = (int32_t) (long long) o[(size_t) i * 2 + 1];
    uint16_t *d0 = s0_out + (size_t) i * VX_NUM_CTX_REF, *d1 = s1_out + (size_t) i * VX_NUM_CTX_REF;
    memcpy(d0, s0, VX_NUM_CTX_REF * 2); memcpy(d1, s1, VX_NUM_CTX_REF * 2);
    ctx_to_reference_order(co.data() + (size_t) i * 2 * VXD_NUM_CTX, d0, d1);
    if (form == 3) {
      if (nb[(size_t) i] > cap) return fail(VVCX_ERR_ARG, "block %d wrote %u bytes, room for %u", i, nb[(size_t) i], cap);
      nbytes[i] = (int32_t) nb[(size_t) i];
    }
  }
  if (form == 3) HIPCHK(hipMemcpy(bytes, dby.p, (size_t) n * cap, hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// ≙ BinEncoder_Std (EL/BinEncoder.cpp:106-420) over an operation string from the I-slice contexts at qp: the device's arith_bin / arith_bins_ep / arith_trm / arith_finish
extern "C" int vvcx_arith_encode(int qp, const int32_t *ops, int nops, uint8_t *out, int cap, int *nbytes, int device)
{
  if (!ops || !out || !nbytes || nops < 0 || cap <= 0) return fail(VVCX_ERR_ARG, "bad argument");
  int kept_of[VX_NUM_CTX_REF];
  for (int k = 0; k < VX_NUM_CTX_REF; k++) kept_of[k] = -1;
  for (int k = 0; k < VXD_NUM_CTX; k++) kept_of[VX_CTX_REF_INDEX[k]] = k;
  std::vector<int32_t> o((size_t) nops * 3 + 1);
  for (int i = 0; i < nops; i++) {
    const int kind = ops[3 * i], a = ops[3 * i + 1], b = ops[3 * i + 2];
    int a2 = a;
    if (kind == 0) { if (a < 0 || a >= VX_NUM_CTX_REF || kept_of[a] < 0 || (b != 0 && b != 1)) return fail(VVCX_ERR_ARG, "operation %d: context %d is not one the library keeps, or bin %d", i, a, b); a2 = kept_of[a]; }
    else if (kind == 1) { if (b < 1 || b > 32 || (b < 32 && ((uint32_t) a >> b))) return fail(VVCX_ERR_ARG, "operation %d: %d bypass bins of value %u", i, b, (uint32_t) a); }
    else if (kind != 2 || (a != 0 && a != 1)) return fail(VVCX_ERR_ARG, "operation %d: kind %d", i, kind);
    o[(size_t) i * 3] = kind; o[(size_t) i * 3 + 1] = a2; o[(size_t) i * 3 + 2] = b;
  }
  uint16_t s0[VX_NUM_CTX_REF], s1[VX_NUM_CTX_REF], kept[2 * VXD_NUM_CTX];
  vvcx_ctx_init(qp, s0, s1); ctx_from_reference_order(s0, s1, kept);
  ON_DEVICE(device);
  DevBuf<uint16_t> dctx; DevBuf<int32_t> dops; DevBuf<uint8_t> dby; DevBuf<uint32_t> dnb;
  HIPCHK(dctx.alloc(2 * VXD_NUM_CTX)); HIPCHK(dops.alloc(o.size())); HIPCHK(dby.alloc((size_t) cap)); HIPCHK(dnb.alloc(1));
  HIPCHK(hipMemcpy(dctx.p, kept, sizeof kept, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dops.p, o.data(), o.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(vvcx_leaf_arith_kernel, dim3(1), dim3(VXD_NT), 0, 0, dctx.p, dops.p, nops, dby.p, (uint32_t) cap, dnb.p);
  HIPCHK(hipGetLastError());
  uint32_t nb = 0;
  HIPCHK(hipMemcpy(&nb, dnb.p, 4, hipMemcpyDeviceToHost));
  if (nb > (uint32_t) cap) return fail(VVCX_ERR_ARG, "buffer too small: %u bytes needed", nb);
  HIPCHK(hipMemcpy(out, dby.p, nb, hipMemcpyDeviceToHost));
  *nbytes = (int) nb;
  return VVCX_OK;
}
