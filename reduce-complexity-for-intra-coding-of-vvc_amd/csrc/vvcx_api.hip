// vvcx_api.hip — host side of the C-ABI declared in include/vvcx.h: owns the device-resident state of a
// batch of pictures (level planes, CU maps, per-stream contexts and scratch), turns compressCtu-style
// tasks into one launch of the persistent per-stream kernel and reads results back.  The other entry points of the interface: vvcx_api_loopfilter.hip (LMCS inverse,
// deblocking, SAO, ALF; with vvcx_sao_rd.hip and vvcx_alf_derive.hip for their host numeric code) and vvcx_api_leaf.hip (the leaf operators).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "vvcx.h"
#include "vvcx_handle.h"      // the handle, NOT_PENDING; vvcx_host.h: DevBuf, ON_DEVICE / DevGuard, HIPCHK
#include "vvcx_kernels.h"
#include "vvcx_tables.h"      // host copy of the constant tables (context init values)
#include "vvcx_ctu_syntax_tables.h"      // the models of the SAO / ALF CTU syntax: flat indices, init values, rates

static thread_local char g_err[512];
extern "C" const char *vvcx_last_error(void) { return g_err; }
// (for vvcx_host.h and the other translation units of the library)
extern "C" int vvcx_fail_msg_(int code, const char *msg) { snprintf(g_err, sizeof g_err, "%s", msg); return code; }
int fail(int code, const char *fmt, ...)
{
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
  return code;
}

#define VVCX_PAYLOAD_BYTES_PER_CTU 32768u
static const uint32_t kBuiltTools = VVCX_TOOL_ISP | VVCX_TOOL_MRL | VVCX_TOOL_MIP | VVCX_TOOL_LFNST | VVCX_TOOL_MTS | VVCX_TOOL_JCCR | VVCX_TOOL_DEPQUANT | VVCX_TOOL_CU_REUSE | VVCX_TOOL_CCLM | VVCX_TOOL_FAST |
                                    VVCX_TOOL_TS | VVCX_TOOL_RDOQ | VVCX_TOOL_LMCS | VVCX_TOOL_WPP;

// Quantizer::initQuantBlock (CL/DepQuant.cpp:694-739) for blocks with log2 w + log2 h = lsum: the quantiser's shift / scale / thresholds and the fixed-point
// distortion normalisation, which the reference derives in fp64 from lambda.  qp: what QpParam hands over (with QpBDOffset).
VxDqConst dq_consts_of(int lsum, int bit_depth, int qp, double lambda)
{
  VxDqConst c; memset(&c, 0, sizeof c);
  const int sq = lsum & 1, qpDQ = qp + 1, per = qpDQ / 6, rem = qpDQ - 6 * per;
  const int nomShift = 15 - bit_depth - (lsum >> 1), trShift = nomShift + (sq ? -1 : 0);
  const int qshift = 14 - 1 + per + trShift;
  const int64_t qscale = VX_QUANT_SCALES[sq * 6 + rem];
  const int invShift = 6 + 1 - per - trShift;
  int qIdxBD = 32 + invShift - 6 - 1; if (qIdxBD > 16) qIdxBD = 16;
  const int nomDShift = 15 - 2 * nomShift + qshift + (sq ? 1 : 0);
  const double qScale2 = (double) (qscale * qscale);
  const double nomDistFactor = nomDShift < 0 ? 1.0 / ((double) ((int64_t) 1 << (-nomDShift)) * qScale2 * lambda) : (double) ((int64_t) 1 << nomDShift) / (qScale2 * lambda);
  const int64_t pow2dfShift = (int64_t) (nomDistFactor * qScale2) + 1;
  int dfShift = (pow2dfShift & (pow2dfShift - 1)) ? 1 : 0;                   // ceil_log2 (680-693)
  for (uint64_t x = (uint64_t) pow2dfShift; x > 1; x >>= 1) dfShift++;
  const int dshift = 62 + qshift - 2 * 15 - dfShift;
  c.qshift = qshift; c.qadd = -(((int64_t) 3 << qshift) >> 1); c.qscale = qscale; c.max_qidx = (1 << (qIdxBD - 1)) - 4;
  c.thres = (int32_t) ((int64_t) 4 << qshift);
  c.dshift = dshift; c.dadd = ((int64_t) 1 << dshift) >> 1;
  c.dstep = (int64_t) (nomDistFactor * (double) ((int64_t) 1 << (dshift + qshift)) + .5);
  c.dorg = (int64_t) (nomDistFactor * (double) ((int64_t) 1 << (dshift + 1)) + .5);
  return c;
}

extern "C" int vvcx_create(const vvcx_cfg *cfg, vvcx_handle **out)
{
  if (!cfg || !out) return fail(VVCX_ERR_ARG, "null argument");
  if (cfg->tools & ~kBuiltTools) return fail(VVCX_ERR_UNSUPPORTED, "tool set 0x%x not built yet (available: 0x%x)", cfg->tools, kBuiltTools);
  // LFNST is built on top of the dependent quantiser (the reference's plain quantiser keeps positions its own decoder rejects with LFNST, CL/Quant.cpp:1054-1058)
  // and on the search's MIP form of the saved mode lists (EL/IntraSearch.cpp:750-775)
  if ((cfg->tools & VVCX_TOOL_LFNST) && (cfg->tools & (VVCX_TOOL_DEPQUANT | VVCX_TOOL_MIP)) != (VVCX_TOOL_DEPQUANT | VVCX_TOOL_MIP))
    return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_LFNST needs VVCX_TOOL_DEPQUANT and VVCX_TOOL_MIP (tool set 0x%x)", cfg->tools);
  // transform skip is searched inside the LFNST pass structure and quantised by RDOQ-TS the way DepQuant::quant reaches it (CL/DepQuant.cpp:1755-1781); RDOQ alone (the
  // cfg sets RDOQ / RDOQTS beside DepQuant) only acts on transform-skip blocks
  if ((cfg->tools & VVCX_TOOL_TS) && (cfg->tools & (VVCX_TOOL_DEPQUANT | VVCX_TOOL_LFNST)) != (VVCX_TOOL_DEPQUANT | VVCX_TOOL_LFNST))
    return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_TS needs VVCX_TOOL_DEPQUANT and VVCX_TOOL_LFNST (tool set 0x%x)", cfg->tools);
  // ISP is one of the candidate kinds of the first (lfnstIdx 0, DCT-II) pass of the LFNST pass loop and its sub-partitions go through the dependent quantiser with
  // the implicit DST-VII of explicit-MTS sequences (TrQuant::getTrTypes)
  if ((cfg->tools & VVCX_TOOL_ISP) && (cfg->tools & (VVCX_TOOL_DEPQUANT | VVCX_TOOL_LFNST | VVCX_TOOL_MTS)) != (VVCX_TOOL_DEPQUANT | VVCX_TOOL_LFNST | VVCX_TOOL_MTS))
    return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_ISP needs VVCX_TOOL_DEPQUANT, VVCX_TOOL_LFNST and VVCX_TOOL_MTS (tool set 0x%x)", cfg->tools);
  if ((cfg->tools & VVCX_TOOL_LMCS) && !(cfg->tools & VVCX_TOOL_DEPQUANT)) return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_LMCS needs VVCX_TOOL_DEPQUANT (tool set 0x%x)", cfg->tools);
  if ((cfg->tools & VVCX_TOOL_JCCR) && !(cfg->tools & VVCX_TOOL_DEPQUANT)) return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_JCCR needs VVCX_TOOL_DEPQUANT (tool set 0x%x)", cfg->tools);
  // the classifier's features read the CUs above-right and below-left of a node through the unrestricted getCU (EL/EncCu.cpp:1126-1217): with the CTU rows running as lagged
  // streams whether those exist yet would depend on timing
  if ((cfg->tools & VVCX_TOOL_WPP) && (cfg->tools & VVCX_TOOL_FAST)) return fail(VVCX_ERR_UNSUPPORTED, "VVCX_TOOL_WPP cannot be combined with VVCX_TOOL_FAST (tool set 0x%x)", cfg->tools);
  if (cfg->ctu_size != 128 || !cfg->dual_tree) return fail(VVCX_ERR_UNSUPPORTED, "only CTUSize 128 with DualITree 1");
  if ((cfg->pic_w & 7) || (cfg->pic_h & 7) || cfg->pic_w <= 0 || cfg->pic_h <= 0) return fail(VVCX_ERR_ARG, "picture size must be a positive multiple of 8");
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10) return fail(VVCX_ERR_UNSUPPORTED, "bit depth %d", cfg->bit_depth);
  if (cfg->max_frames < 1 || cfg->tile_cols < 1 || cfg->tile_rows < 1) return fail(VVCX_ERR_ARG, "max_frames / tile grid");
  ON_DEVICE(cfg->device);
  vvcx_handle *h = new vvcx_handle();          // every field zero, every buffer empty
  h->cfg = *cfg;
  h->ctus_w = (cfg->pic_w + 127) >> 7; h->ctus_h = (cfg->pic_h + 127) >> 7;
  if (cfg->tile_cols > h->ctus_w || cfg->tile_rows > h->ctus_h) { delete h; return fail(VVCX_ERR_ARG, "more tiles than CTUs"); }
  h->uw = (cfg->pic_w + 3) >> 2; h->uh = (cfg->pic_h + 3) >> 2;
  h->ntiles = cfg->tile_cols * cfg->tile_rows;
  h->ctu_tile.resize((size_t) h->ctus_w * h->ctus_h);
  h->tile_ctus.assign((size_t) h->ntiles, std::vector<int>());
  for (int ry = 0; ry < h->ctus_h; ry++) for (int rx = 0; rx < h->ctus_w; rx++) {
    int tc = 0, tr = 0;                          // uniform spacing: boundary i = i*N/T
    for (int i = 0; i < cfg->tile_cols; i++) if (rx >= (i * h->ctus_w) / cfg->tile_cols) tc = i;
    for (int i = 0; i < cfg->tile_rows; i++) if (ry >= (i * h->ctus_h) / cfg->tile_rows) tr = i;
    const int t = tr * cfg->tile_cols + tc;
    h->ctu_tile[(size_t) ry * h->ctus_w + rx] = t;
    h->tile_ctus[(size_t) t].push_back(ry * h->ctus_w + rx);
  }
  {
    const bool wpp = (cfg->tools & VVCX_TOOL_WPP) != 0;
    h->ctu_sub.assign(h->ctu_tile.size(), 0); h->tile_sub0.assign((size_t) h->ntiles, 0); h->tile_nsub.assign((size_t) h->ntiles, 1);
    h->sub_ctus.clear(); h->sub_tile.clear(); h->sub_above.clear();
    for (int t = 0; t < h->ntiles; t++) {
      h->tile_sub0[(size_t) t] = (int) h->sub_ctus.size();
      int prev_row = -1, n = 0;
      for (int a : h->tile_ctus[(size_t) t]) {
        const int row = a / h->ctus_w;
        if (n == 0 || (wpp && row != prev_row)) { h->sub_ctus.push_back(std::vector<int>()); h->sub_tile.push_back(t); h->sub_above.push_back(n ? (int) h->sub_ctus.size() - 2 : -1); n++; }
        prev_row = row;
        h->sub_ctus.back().push_back(a); h->ctu_sub[(size_t) a] = (int) h->sub_ctus.size() - 1;
      }
      h->tile_nsub[(size_t) t] = n;
    }
    h->nsub = (int) h->sub_ctus.size();
  }
  { const char *e = getenv("VVCX_WPP_TEST_INTERLEAVE"); h->wpp_rr = e && *e == '1'; }
  const int wc = cfg->pic_w >> 1, hc = cfg->pic_h >> 1;
  h->lev_plane[0] = (size_t) cfg->pic_w * cfg->pic_h; h->lev_plane[1] = h->lev_plane[2] = (size_t) wc * hc;
  h->lev_frame = h->lev_plane[0] + 2 * h->lev_plane[1];
  h->units_plane = (size_t) h->uw * h->uh; h->units_frame = 2 * h->units_plane;
  const int F = cfg->max_frames;
  const size_t nstream = (size_t) F * h->nsub;
  const bool wpp = (cfg->tools & VVCX_TOOL_WPP) != 0;
  if (h->frames_d.alloc((size_t) F) != hipSuccess || h->lev_d.alloc(h->lev_frame * F) != hipSuccess || h->units_d.alloc(h->units_frame * F) != hipSuccess ||
      h->stream_ctx_d.alloc(nstream * 2 * VXD_NUM_CTX) != hipSuccess ||
      (wpp && (h->wpp_progress_d.alloc(nstream) != hipSuccess || h->wpp_sync_d.alloc(nstream * 2 * VXD_NUM_CTX) != hipSuccess)) ||
      h->counters_d.alloc(56) != hipSuccess || h->dq_d.alloc(17 * 96) != hipSuccess) { vvcx_destroy(h); return fail(VVCX_ERR_DEVICE, "device allocation failed"); }
  if (cfg->emit_payload) {                       // VVCX_PAYLOAD_BYTES_PER_CTU per CTU: a CTU of 8-bit video at QP >= 17 stays far below (raw samples are 24 KB)
    h->payload_off.resize(nstream); h->payload_cap.resize(nstream);
    uint64_t off = 0;
    for (size_t s2 = 0; s2 < nstream; s2++) { const uint32_t cap = (uint32_t) h->sub_ctus[s2 % (size_t) h->nsub].size() * VVCX_PAYLOAD_BYTES_PER_CTU; h->payload_off[s2] = off; h->payload_cap[s2] = cap; off += cap; }
    if (h->payload_d.alloc(off) != hipSuccess || h->payload_off_d.alloc(nstream) != hipSuccess || h->payload_cap_d.alloc(nstream) != hipSuccess ||
        h->arith_d.alloc(nstream * 32) != hipSuccess) { vvcx_destroy(h); return fail(VVCX_ERR_DEVICE, "device allocation failed"); }
    (void) hipMemcpy(h->payload_off_d.p, h->payload_off.data(), nstream * 8, hipMemcpyHostToDevice);
    (void) hipMemcpy(h->payload_cap_d.p, h->payload_cap.data(), nstream * 4, hipMemcpyHostToDevice);
    (void) hipMemset(h->arith_d.p, 0, nstream * 32);
  }
  (void) hipEventCreate(&h->ev0); (void) hipEventCreate(&h->ev1); (void) hipEventCreate(&h->ev2);
  *out = h;
  return VVCX_OK;
}

extern "C" void vvcx_destroy(vvcx_handle *h)
{
  if (!h) return;
  if (h->pending) (void) hipStreamSynchronize(h->pend_stream);      // first: a launch still in flight reads and writes what is freed below
  (void) hipHostFree(h->pend_res);
  (void) hipEventDestroy(h->ev0); (void) hipEventDestroy(h->ev1); (void) hipEventDestroy(h->ev2);
  delete h;                                     // frees every device buffer
}

// ---- slice-level inputs (host only)
extern "C" int vvcx_chroma_qp_table(int bit_depth, int n_pts, const int32_t *qp_in, const int32_t *qp_out, int32_t *table)
{
  if (!qp_in || !qp_out || !table || n_pts < 1 || n_pts > 8 || (bit_depth != 8 && bit_depth != 10)) return fail(VVCX_ERR_ARG, "bad argument");
  const int off = 6 * (bit_depth - 8), maxQp = 63;
  for (int j = 0; j < n_pts; j++) {
    if (qp_in[j] < -off || qp_in[j] > maxQp || qp_out[j] < -off || qp_out[j] > maxQp || (j && qp_in[j] <= qp_in[j - 1])) return fail(VVCX_ERR_ARG, "chroma QP pivot %d out of range or not increasing", j);
  }
  auto clipq = [&](int v) { return v < -off ? -off : v > maxQp ? maxQp : v; };
  int32_t *t = table + off;                           // t[q], q = -off .. 63
  t[qp_in[0]] = qp_out[0];
  for (int k = qp_in[0] - 1; k >= -off; k--) t[k] = clipq(t[k + 1] - 1);
  for (int j = 0; j + 1 < n_pts; j++) {
    const int dIn = qp_in[j + 1] - qp_in[j], dOut = qp_out[j + 1] - qp_out[j], sh = (dIn + 1) >> 1;      // deltaQpInValMinus1 + 1 = dIn
    for (int k = qp_in[j] + 1, m = 1; k <= qp_in[j + 1]; k++, m++) t[k] = t[qp_in[j]] + (dOut * m + sh) / dIn;
  }
  for (int k = qp_in[n_pts - 1] + 1; k <= maxQp; k++) t[k] = clipq(t[k - 1] + 1);
  return VVCX_OK;
}
extern "C" int vvcx_derive_slice(const vvcx_slice_cfg *c, vvcx_slice *out)
{
  if (!c || !out) return fail(VVCX_ERR_ARG, "null argument");
  const int off = 6 * (c->bit_depth - 8);
  if (c->qp < -off || c->qp > 63 || c->gop_size < 1) return fail(VVCX_ERR_ARG, "qp / gop_size");
  int32_t table[64 + 12];
  const int rc = vvcx_chroma_qp_table(c->bit_depth, c->n_pts, c->qp_in, c->qp_out, table);
  if (rc) return rc;
  memset(out, 0, sizeof *out);
  out->qp = c->qp;
  double scale = 0.05 * (double) (c->gop_size - 1); scale = scale < 0.0 ? 0.0 : scale > 0.5 ? 0.5 : scale;
  out->lambda = 0.57 * (1.0 - scale) * pow(2.0, ((double) c->qp + (double) off - 12.0) / 3.0);
  if (c->dep_quant) out->lambda *= pow(2.0, 0.25 / 3.0);
  const int offs[2] = { c->cb_qp_offset, c->cr_qp_offset };
  for (int k = 0; k < 2; k++) {
    const int mapped = table[c->qp + off];                                    // getMappedChromaQpValue(compID, qp), JVET_O0650
    int q = mapped + offs[k]; q = q < -off ? -off : q > 63 ? 63 : q;           // QpParam (CL/Quant.cpp:95-97): map, add the offset, clip
    out->qp_c[k] = q;
    out->dist_weight[k] = pow(2.0, ((double) c->qp - (double) (mapped + offs[k])) / 3.0);      // setUpLambda 120-126: unclipped
    if (c->dep_quant) out->dist_weight[k] *= (c->gop_size >= 8 ? pow(2.0, 0.1 / 3.0) : pow(2.0, 0.2 / 3.0));      // 127-130 (LFNST off)
  }
  return VVCX_OK;
}

// The partition forest of the FAST_ALGORITHM path (the reference: joblib.load("Partition_32.pkl").predict, BIN/TEST.py:21-25), as
// flattened sklearn tree arrays; validated here so that the device walk cannot leave the arrays or loop.
extern "C" int vvcx_set_forest(vvcx_handle *h, int n_trees, int n_nodes, int n_classes, const int32_t *root, const int32_t *feature, const double *threshold,
                               const int32_t *left, const int32_t *right, const double *value, const int32_t *classes)
{
  NOT_PENDING(h);
  if (!h || !root || !feature || !threshold || !left || !right || !value || !classes) return fail(VVCX_ERR_ARG, "null argument");
  if (n_trees < 1 || n_nodes < n_trees || n_classes < 1 || n_classes > 8) return fail(VVCX_ERR_ARG, "forest shape");
  std::vector<VxForestNode> nodes((size_t) n_nodes);
  for (int i = 0; i < n_nodes; i++) {
    if (left[i] >= 0) {
      // children of sklearn trees always follow their parent in the node array: a walk therefore ends
      if (left[i] <= i || right[i] <= i || left[i] >= n_nodes || right[i] >= n_nodes || feature[i] < 0 || feature[i] >= 26) return fail(VVCX_ERR_ARG, "forest node %d: child or feature index out of range", i);
    }
    nodes[(size_t) i].thr = threshold[i]; nodes[(size_t) i].left = left[i] >= 0 ? left[i] : -1; nodes[(size_t) i].right = right[i]; nodes[(size_t) i].feature = left[i] >= 0 ? feature[i] : 0; nodes[(size_t) i].pad = 0;
  }
  for (int t = 0; t < n_trees; t++) if (root[t] < 0 || root[t] >= n_nodes) return fail(VVCX_ERR_ARG, "forest root %d out of range", t);
  for (int c = 0; c < n_classes; c++) if (classes[c] < 0 || classes[c] > 5) return fail(VVCX_ERR_ARG, "forest class label %d", classes[c]);
  ON_DEVICE(h->cfg.device);
  h->f_ntrees = 0; h->f_node_d.release(); h->f_value_d.release(); h->f_root_d.release();      // no forest until the new one is complete
  HIPCHK(h->f_node_d.alloc((size_t) n_nodes)); HIPCHK(h->f_value_d.alloc((size_t) n_nodes * (size_t) n_classes)); HIPCHK(h->f_root_d.alloc((size_t) n_trees));
  HIPCHK(hipMemcpy(h->f_node_d.p, nodes.data(), sizeof(VxForestNode) * (size_t) n_nodes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->f_value_d.p, value, sizeof(double) * (size_t) n_nodes * (size_t) n_classes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->f_root_d.p, root, sizeof(int32_t) * (size_t) n_trees, hipMemcpyHostToDevice));
  h->f_ntrees = n_trees; h->f_nclasses = n_classes;
  for (int c = 0; c < 8; c++) h->f_classes[c] = c < n_classes ? classes[c] : 0;
  return VVCX_OK;
}

extern "C" int vvcx_set_slice(vvcx_handle *h, const vvcx_slice *s)
{
  NOT_PENDING(h);
  if (!h || !s) return fail(VVCX_ERR_ARG, "null argument");
  if (!(s->lambda > 0.0) || s->qp < -6 * (h->cfg.bit_depth - 8) || s->qp > 63) return fail(VVCX_ERR_ARG, "bad slice parameters (QP range -QpBDOffset..63, like vvcx_derive_slice)");
  bool lmcs = false;
  // what the bound pictures were prepared with (vvcx_bind_frames): start contexts of the slice QP, the forward-mapped luma and the device LUTs of the LMCS model
  const bool was_bound = h->have_slice && h->n_frames > 0, lmcs_before = h->lmcs_on; const int qp_before = h->sl.qp;
  int16_t fwd_before[1024]; if (was_bound && lmcs_before) memcpy(fwd_before, h->lmcs_fwd, sizeof fwd_before);
  if (s->lmcs_enable) {
    // the piece-wise linear model of the slice -> LUTs (Reshape::constructReshaper, CL/Reshape.cpp:297-333, JVET_O0428 form: 16 input bins of equal width,
    // bin i owns orgCW + delta code words in the mapped domain; 11 fractional bits for the slopes; the inverse slope of a bin is also its chroma residual scale)
    if (!(h->cfg.tools & VVCX_TOOL_LMCS)) return fail(VVCX_ERR_ARG, "the slice enables LMCS, the handle's tool set does not");
    const int n = 1 << h->cfg.bit_depth, orgCW = n >> 4, lg = h->cfg.bit_depth - 4;
    if (s->lmcs_min_bin < 0 || s->lmcs_max_bin > 15 || s->lmcs_min_bin > s->lmcs_max_bin) return fail(VVCX_ERR_ARG, "LMCS bin range %d..%d", s->lmcs_min_bin, s->lmcs_max_bin);
    int cw[16], fwdSlope[16], invSlope[16], total = 0;
    for (int b = 0; b < 16; b++) {
      cw[b] = (b < s->lmcs_min_bin || b > s->lmcs_max_bin) ? 0 : orgCW + s->lmcs_delta_cw[b];
      if (cw[b] < 0 || cw[b] > 0xffff) return fail(VVCX_ERR_ARG, "LMCS bin %d: %d code words", b, cw[b]);
      total += cw[b];
    }
    if (total > n - 1) return fail(VVCX_ERR_ARG, "LMCS model uses %d code words of %d", total, n - 1);
    h->lmcs_pivot[0] = 0;
    for (int b = 0; b < 16; b++) {
      h->lmcs_pivot[b + 1] = h->lmcs_pivot[b] + cw[b];
      fwdSlope[b] = (cw[b] * 2048 + (1 << (lg - 1))) >> lg;
      invSlope[b] = cw[b] ? orgCW * 2048 / cw[b] : 0;
      h->lmcs_cadj[b] = cw[b] ? invSlope[b] : 2048;
    }
    for (int v = 0; v < n; v++) {
      const int b = v >> lg;
      int t = h->lmcs_pivot[b] + ((fwdSlope[b] * (v - b * orgCW) + 1024) >> 11);
      h->lmcs_fwd[v] = (int16_t) (t < 0 ? 0 : t > n - 1 ? n - 1 : t);
      int k = s->lmcs_min_bin;                           // getPWLIdxInv 268-283: the first bin whose upper border lies above v
      while (k <= s->lmcs_max_bin && v >= h->lmcs_pivot[k + 1]) k++;
      if (k > 15) k = 15;
      t = k * orgCW + ((invSlope[k] * (v - h->lmcs_pivot[k]) + 1024) >> 11);
      h->lmcs_inv[v] = (int16_t) (t < 0 ? 0 : t > n - 1 ? n - 1 : t);
    }
    lmcs = true;
  }
  h->sl = *s; h->have_slice = true; h->lmcs_on = lmcs;
  // a slice whose QP or LMCS model differs from the one the pictures were bound with unbinds them: searching them would start from the wrong contexts, on unmapped
  // (or differently mapped) luma and with LUTs that are not on the device.  The caller binds again (header: "before vvcx_bind_frames").
  if (was_bound && (qp_before != s->qp || lmcs_before != lmcs || (lmcs && memcmp(fwd_before, h->lmcs_fwd, (size_t) 2 << h->cfg.bit_depth) != 0))) h->n_frames = 0;
  return VVCX_OK;
}

extern "C" int vvcx_lmcs_tables(vvcx_handle *h, int16_t *fwd, int16_t *inv, int32_t pivot[17], int32_t chroma_scale[16])
{
  if (!h || !fwd || !inv || !pivot || !chroma_scale) return fail(VVCX_ERR_ARG, "null argument");
  if (!h->have_slice || !h->lmcs_on) return fail(VVCX_ERR_STATE, "the slice does not enable LMCS");
  memcpy(fwd, h->lmcs_fwd, (size_t) 2 << h->cfg.bit_depth); memcpy(inv, h->lmcs_inv, (size_t) 2 << h->cfg.bit_depth);
  memcpy(pivot, h->lmcs_pivot, sizeof h->lmcs_pivot); memcpy(chroma_scale, h->lmcs_cadj, sizeof h->lmcs_cadj);
  return VVCX_OK;
}

// CtxStore::init for an I slice (CL/Contexts.cpp:135-151 JVET_O0065 form, 1818-1833)
void ctx_init_islice(int qp, uint16_t *s0, uint16_t *s1)
{
  qp = qp < 0 ? 0 : qp > 63 ? 63 : qp;
  for (int k = 0; k < VXD_NUM_CTX; k++) {
    const int id = VX_CTX_INIT_I[k];
    const int slope = (id >> 3) - 4, offset = ((id & 7) * 18) + 1;
    int st = ((slope * (qp - 16)) >> 1) + offset;
    st = st < 1 ? 1 : st > 127 ? 127 : st;
    const int p1 = st << 8;
    s0[k] = (uint16_t) (p1 & 0x7FE0); s1[k] = (uint16_t) (p1 & 0x7FFE);
  }
}

static_assert(VXD_NUM_CTX == VX_NUM_CTX, "vvcx_dev.h and the generated tables disagree on the number of context models");

extern "C" int vvcx_bind_frames(vvcx_handle *h, const vvcx_frame *frames, int n)
{
  NOT_PENDING(h);
  if (h) h->alf_res_valid = h->sao_res_valid = false;      // the resident ALF statistics / SAO decision no longer describe the bound pictures
  if (!h || !frames) return fail(VVCX_ERR_ARG, "null argument");
  ON_DEVICE(h->cfg.device);
  if (n < 1 || n > h->cfg.max_frames) return fail(VVCX_ERR_ARG, "n_frames %d outside 1..%d", n, h->cfg.max_frames);
  if (!h->have_slice) return fail(VVCX_ERR_STATE, "vvcx_set_slice must precede vvcx_bind_frames");
  h->frames_h.resize((size_t) n);
  for (int f = 0; f < n; f++) {
    VxFrameDev &d = h->frames_h[(size_t) f];
    for (int c = 0; c < 3; c++) {
      if (!frames[f].org[c] || !frames[f].reco[c]) return fail(VVCX_ERR_ARG, "frame %d plane %d is null", f, c);
      d.org[c] = frames[f].org[c]; d.rec[c] = frames[f].reco[c]; d.stride[c] = frames[f].stride[c];
      if (d.stride[c] < (c ? h->cfg.pic_w >> 1 : h->cfg.pic_w)) return fail(VVCX_ERR_ARG, "frame %d plane %d stride too small", f, c);
      const size_t bps = h->cfg.bit_depth == 8 ? 1 : 2;   // the deblocking kernel loads four samples at a time: strides and bases must keep that alignment
      if ((d.stride[c] & 3) || (((uintptr_t) d.org[c] | (uintptr_t) d.rec[c]) & (4 * bps - 1))) return fail(VVCX_ERR_ARG, "frame %d plane %d: base address / stride not aligned to 4 samples", f, c);
    }
    int16_t *lev = h->lev_d.p + (size_t) f * h->lev_frame;
    d.lev[0] = lev; d.lev[1] = lev + h->lev_plane[0]; d.lev[2] = lev + h->lev_plane[0] + h->lev_plane[1];
    d.lstride[0] = h->cfg.pic_w; d.lstride[1] = d.lstride[2] = h->cfg.pic_w >> 1;
    d.units[0] = h->units_d.p + (size_t) f * h->units_frame; d.units[1] = d.units[0] + h->units_plane;
  }
  h->lmcs_inverted = false;
  if (h->lmcs_on) {
    // EncGOP::xPicInitLMCS (EL/EncGOP.cpp:1689-1695): the original luma of an intra picture is forward mapped once, before the slice is compressed; the search
    // reads the mapped copy (same stride as the caller's plane: the picture record has one stride per component)
    const size_t bps = h->cfg.bit_depth == 8 ? 1 : 2;
    size_t need = 0;
    for (int f = 0; f < n; f++) need += (size_t) h->frames_h[(size_t) f].stride[0] * h->cfg.pic_h * bps;
    HIPCHK(h->lmcs_org_d.reserve(need));
    HIPCHK(h->lmcs_lut_d.reserve(2 * 1024));
    HIPCHK(hipMemcpy(h->lmcs_lut_d.p, h->lmcs_fwd, 2048, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(h->lmcs_lut_d.p + 1024, h->lmcs_inv, 2048, hipMemcpyHostToDevice));
    // the records with the caller's own luma: the SAO encoder measures against the true original, which the reference restores in front of the loop filters
    // (a second record array of the handle; the search's records get the mapped copy below)
    HIPCHK(h->frames_org_d.reserve((size_t) n));
    HIPCHK(hipMemcpy(h->frames_org_d.p, h->frames_h.data(), sizeof(VxFrameDev) * (size_t) n, hipMemcpyHostToDevice));
    size_t off = 0;
    for (int f = 0; f < n; f++) {
      VxFrameDev &d = h->frames_h[(size_t) f];
      void *dst = h->lmcs_org_d.p + off;
      const unsigned blocks = (unsigned) (((size_t) h->cfg.pic_w * h->cfg.pic_h + VXD_NT - 1) / VXD_NT);
      if (bps == 1) hipLaunchKernelGGL(vvcx_lmcs_map_kernel_u8, dim3(blocks), dim3(VXD_NT), 0, 0, (const uint8_t *) d.org[0], (uint8_t *) dst, h->cfg.pic_w, h->cfg.pic_h, d.stride[0], h->lmcs_lut_d.p);
      else hipLaunchKernelGGL(vvcx_lmcs_map_kernel_u16, dim3(blocks), dim3(VXD_NT), 0, 0, (const uint16_t *) d.org[0], (uint16_t *) dst, h->cfg.pic_w, h->cfg.pic_h, d.stride[0], h->lmcs_lut_d.p);
      HIPCHK(hipGetLastError());
      d.org[0] = dst;
      off += (size_t) d.stride[0] * h->cfg.pic_h * bps;
    }
  }
  HIPCHK(hipMemcpy(h->frames_d.p, h->frames_h.data(), sizeof(VxFrameDev) * (size_t) n, hipMemcpyHostToDevice));
  if (h->cfg.tools & VVCX_TOOL_JCCR) {                    // the slice's joint_cb_cr_sign_flag from the bound picture (EL/EncSlice.cpp:1594-1597), left in its record
    if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_jccr_sign_kernel_u8, dim3((unsigned) n), dim3(VXD_NT), 0, 0, h->frames_d.p, h->cfg.pic_w >> 1, h->cfg.pic_h >> 1);
    else hipLaunchKernelGGL(vvcx_jccr_sign_kernel_u16, dim3((unsigned) n), dim3(VXD_NT), 0, 0, h->frames_d.p, h->cfg.pic_w >> 1, h->cfg.pic_h >> 1);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemset(h->units_d.p, 0, h->units_frame * sizeof(VxUnit) * (size_t) n));
  HIPCHK(hipMemset(h->lev_d.p, 0, h->lev_frame * 2 * (size_t) n));
  std::vector<uint16_t> ctx((size_t) n * h->nsub * 2 * VXD_NUM_CTX);
  for (size_t s = 0; s < (size_t) n * h->nsub; s++) ctx_init_islice(h->sl.qp, &ctx[s * 2 * VXD_NUM_CTX], &ctx[s * 2 * VXD_NUM_CTX + VXD_NUM_CTX]);
  HIPCHK(hipMemcpy(h->stream_ctx_d.p, ctx.data(), ctx.size() * 2, hipMemcpyHostToDevice));
  {
    // activity per CTU (read back here: binding is synchronous anyway); a failure only costs the ordering
    const size_t nact = (size_t) n * h->ctus_w * h->ctus_h;
    h->activity.assign(nact, 0);
    DevBuf<unsigned> dact;
    if (dact.alloc(nact) == hipSuccess) {
      const dim3 grid((unsigned) (h->ctus_w * h->ctus_h), (unsigned) n);
      if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_ctu_activity_kernel_u8, grid, dim3(VXD_NT), 0, 0, h->frames_d.p, h->cfg.pic_w, h->cfg.pic_h, h->ctus_w, dact.p);
      else hipLaunchKernelGGL(vvcx_ctu_activity_kernel_u16, grid, dim3(VXD_NT), 0, 0, h->frames_d.p, h->cfg.pic_w, h->cfg.pic_h, h->ctus_w, dact.p);
      if (hipGetLastError() != hipSuccess || hipMemcpy(h->activity.data(), dact.p, nact * 4, hipMemcpyDeviceToHost) != hipSuccess) h->activity.assign(nact, 0);
    }
  }
  h->n_frames = n;
  if (h->wpp_progress_d.p) HIPCHK(hipMemset(h->wpp_progress_d.p, 0, (size_t) n * h->nsub * 4));
  if (h->train_n_d.p) HIPCHK(hipMemset(h->train_n_d.p, 0, 4));
  h->next_idx.assign((size_t) n * h->nsub, 0);
  h->rw_trace_n.clear(); h->rw_trace_cap = 0;
  return VVCX_OK;
}

extern "C" int vvcx_ctus_per_frame(const vvcx_handle *h) { return h ? h->ctus_w * h->ctus_h : 0; }

extern "C" int vvcx_resident_streams(const vvcx_handle *h)
{
  if (!h) return 0;
  DevGuard guard(h->cfg.device);                  // (a count, not an error code: no ON_DEVICE)
  int cus = 0, per_cu = 0;
  if (!guard.ok || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) != hipSuccess) return 0;
  const bool wpp = (h->cfg.tools & VVCX_TOOL_WPP) != 0;
  const void *k = h->cfg.bit_depth == 8 ? (wpp ? (const void *) vvcx_compress_wpp_kernel_u8 : (const void *) vvcx_compress_kernel_u8) : (wpp ? (const void *) vvcx_compress_wpp_kernel_u16 : (const void *) vvcx_compress_kernel_u16);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, VXD_NT, 0) != hipSuccess) return 0;
  { const char *e = getenv("VVCX_MAX_WG_PER_CU"); const int cap = e ? atoi(e) : 0; if (cap > 0 && cap < per_cu) per_cu = cap; }      // diagnostic: the rate against the workgroups sharing a CU
  return cus * per_cu;
}

// the launch parameters every kernel that codes CTU syntax reads (the search and the payload rewrite): picture and slice constants, the handle's device state
static void stream_params(vvcx_handle *h, VxParams &p)
{
  memset(&p, 0, sizeof p);
  p.pic_w = h->cfg.pic_w; p.pic_h = h->cfg.pic_h; p.bit_depth = h->cfg.bit_depth; p.chroma = h->cfg.chroma; p.tools = h->cfg.tools;
  for (int k = 0; k < 2; k++) { p.min_qt[k] = h->cfg.min_qt[k]; p.max_bt_depth[k] = h->cfg.max_bt_depth[k]; p.max_bt_size[k] = h->cfg.max_bt_size[k]; p.max_tt_size[k] = h->cfg.max_tt_size[k]; p.qp_c[k] = h->sl.qp_c[k]; p.dist_weight[k] = h->sl.dist_weight[k]; }
  p.ctus_w = h->ctus_w; p.ctus_h = h->ctus_h; p.uw = h->uw; p.uh = h->uh; p.qp = h->sl.qp;
  p.lambda = h->sl.lambda;
  { const int bdo = 6 * (h->cfg.bit_depth - 8); p.qp_tr = h->sl.qp + bdo; p.qp_tr_c[0] = h->sl.qp_c[0] + bdo; p.qp_tr_c[1] = h->sl.qp_c[1] + bdo;
    // QpParam of the modes +-2: the mapping table's value (one table for all chroma) + pps_joint_cbcr_qp_offset (CbCrQpOffset -1, APP/EncAppCfg.cpp:1082)
    int qj = h->sl.qp_c[0] - 1; qj = qj < -bdo ? -bdo : qj > 63 ? 63 : qj; p.qp_tr_j = qj + bdo; }
  p.dist_scale = (double) (1 << 15) / h->sl.lambda;                       // CL/RdCost.cpp:79
  p.sqrt_lambda_fp = sqrt(h->sl.lambda) * (1.0 / (double) (1 << 15));     // EL/IntraSearch.cpp:297
  p.frames = h->frames_d.p; p.streams = h->streams_d.p; p.task_ctu = h->task_ctu_d.p; p.results = h->results_d.p; p.stream_ctx = h->stream_ctx_d.p;
  p.payload = h->payload_d.p; p.payload_off = h->payload_off_d.p; p.payload_cap = h->payload_cap_d.p; p.arith_state = h->arith_d.p;
  p.scratch = h->scratch_d.p; p.counters = h->counters_d.p; p.ntiles = h->ntiles; p.nsub = h->nsub; p.wpp_progress = h->wpp_progress_d.p; p.wpp_sync = h->wpp_sync_d.p;
  p.train_rows = h->train_rows_d.p; p.train_n = h->train_n_d.p; p.train_cap = h->train_cap; p.wpp_sched = h->wpp_sched_d.p; p.wpp_rr = h->wpp_rr;
  p.f_node = h->f_node_d.p; p.f_value = h->f_value_d.p; p.f_root = h->f_root_d.p; p.f_ntrees = h->f_ntrees; p.f_nclasses = h->f_nclasses;
  for (int c = 0; c < 8; c++) p.f_classes[c] = h->f_classes[c];
  p.lmcs_on = h->lmcs_on; p.lmcs_cadj_on = h->lmcs_on && h->sl.lmcs_chroma_adj; p.lmcs_min_bin = h->sl.lmcs_min_bin; p.lmcs_max_bin = h->sl.lmcs_max_bin;
  for (int b = 0; b < 17; b++) p.lmcs_pivot[b] = h->lmcs_on ? h->lmcs_pivot[b] : 0;
  for (int b = 0; b < 16; b++) p.lmcs_cadj[b] = h->lmcs_on ? h->lmcs_cadj[b] : 0;
}

// The enqueue half: everything up to and including the device-to-host copy of the CTU results goes onto `hip_stream`; nothing waits.
extern "C" int vvcx_submit_ctus(vvcx_handle *h, const vvcx_ctu_task *tasks, int n, void *hip_stream)
{
  NOT_PENDING(h);
  if (h) h->alf_res_valid = h->sao_res_valid = false;      // the resident ALF statistics / SAO decision no longer describe the bound pictures
  if (h && (h->cfg.tools & VVCX_TOOL_FAST) && !h->f_ntrees) return fail(VVCX_ERR_STATE, "VVCX_TOOL_FAST needs vvcx_set_forest before the first CTU");
  if (!h || (!tasks && n) || n < 0) return fail(VVCX_ERR_ARG, "bad argument");
  if (n == 0) { h->pending = true; h->pend_n = 0; h->pend_stream = (hipStream_t) hip_stream; h->pend_src.clear(); h->pend_next = h->next_idx; return VVCX_OK; }   // nothing to code: an empty submission, not an error
  if (h->n_frames == 0) return fail(VVCX_ERR_STATE, "no frames bound");
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  const int nctu = h->ctus_w * h->ctus_h;
  // group tasks by stream, keeping their order; validate that every stream continues in tile raster order
  std::vector<std::vector<int>> by_stream((size_t) h->n_frames * h->nsub);
  for (int i = 0; i < n; i++) {
    if (tasks[i].frame < 0 || tasks[i].frame >= h->n_frames || tasks[i].ctu_rs_addr < 0 || tasks[i].ctu_rs_addr >= nctu) return fail(VVCX_ERR_ARG, "task %d out of range", i);
    by_stream[(size_t) tasks[i].frame * h->nsub + h->ctu_sub[(size_t) tasks[i].ctu_rs_addr]].push_back(i);
  }
  std::vector<VxStreamDesc> &sd = h->pend_sd; std::vector<int32_t> &task_ctu = h->pend_task_ctu; std::vector<int> &task_src = h->pend_src;
  sd.clear(); task_ctu.clear(); task_src.clear();
  std::vector<int> &new_next = h->pend_next; new_next = h->next_idx;
  for (size_t s = 0; s < by_stream.size(); s++) {
    if (by_stream[s].empty()) continue;
    const int sub = (int) (s % (size_t) h->nsub), tile = h->sub_tile[(size_t) sub];
    VxStreamDesc d; d.frame = (int) (s / (size_t) h->nsub); d.tile = tile; d.first_task = (int) task_ctu.size(); d.n_tasks = (int) by_stream[s].size();
    d.done_before = h->next_idx[s]; d.tile_ctus = (int) h->sub_ctus[(size_t) sub].size();
    d.sub = sub; d.above = (h->cfg.tools & VVCX_TOOL_WPP) ? h->sub_above[(size_t) sub] : -1;
    for (int i : by_stream[s]) {
      const std::vector<int> &order = h->sub_ctus[(size_t) sub];
      if (new_next[s] >= (int) order.size() || order[(size_t) new_next[s]] != tasks[i].ctu_rs_addr)
        return fail(VVCX_ERR_STATE, "task %d (frame %d, CTU %d) is not the next CTU of its stream", i, tasks[i].frame, tasks[i].ctu_rs_addr);
      new_next[s]++;
      task_ctu.push_back(tasks[i].ctu_rs_addr); task_src.push_back(i);
    }
    sd.push_back(d);
  }
  // WPP: a CTU row waits, CTU by CTU, for the row above it; whatever it waits for must be coded already or be part of this launch
  if (h->cfg.tools & VVCX_TOOL_WPP)
    for (size_t s = 0; s < by_stream.size(); s++) {
      const int above = h->sub_above[s % (size_t) h->nsub];
      if (by_stream[s].empty() || above < 0) continue;
      const size_t sa = s - (s % (size_t) h->nsub) + (size_t) above;
      if (new_next[sa] < new_next[s]) return fail(VVCX_ERR_STATE, "WPP: CTU row (sub-stream %d) of frame %d would wait for CTUs of the row above that are neither coded nor submitted", (int) (s % (size_t) h->nsub), (int) (s / (size_t) h->nsub));
    }
  // longest first: the workgroups take the streams from the queue in this order; results are addressed through first_task, so the order is free.  Under WPP the rows of a
  // tile stay together and in order (a row's workgroup waits for the row above, which must therefore have been taken from the queue before it): the key is the tile's
  {
    std::vector<uint64_t> key(sd.size());
    std::vector<uint64_t> group((size_t) h->n_frames * h->ntiles, 0);
    for (size_t i = 0; i < sd.size(); i++) {
      uint64_t a = 0;
      for (int t = 0; t < sd[i].n_tasks; t++) a += h->activity.empty() ? 0 : h->activity[(size_t) sd[i].frame * nctu + (size_t) task_ctu[(size_t) sd[i].first_task + t]];
      key[i] = a; group[(size_t) sd[i].frame * h->ntiles + sd[i].tile] += a;
    }
    if (h->cfg.tools & VVCX_TOOL_WPP) for (size_t i = 0; i < sd.size(); i++) key[i] = group[(size_t) sd[i].frame * h->ntiles + sd[i].tile];
    std::vector<size_t> order(sd.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return key[a] > key[b]; });
    std::vector<VxStreamDesc> sorted(sd.size());
    for (size_t i = 0; i < order.size(); i++) sorted[i] = sd[order[i]];
    sd.swap(sorted);
  }
  const int ns = (int) sd.size();
  HIPCHK(h->streams_d.reserve((size_t) ns)); HIPCHK(h->task_ctu_d.reserve((size_t) n)); HIPCHK(h->results_d.reserve((size_t) n));
  const size_t per_stream = (h->cfg.tools & VVCX_TOOL_CU_REUSE) ? (size_t) VXD_SCRATCH_BYTES : (size_t) VXD_OFF_CACHE;   // the CU cache only when used
  // one workgroup per resident stream slot (they take the streams from a queue): scratch is per slot
  int resident = vvcx_resident_streams(h);
  if (resident < 1) resident = 1;
  const int grid = ns < resident ? ns : resident;
  const size_t need = (size_t) grid * per_stream;
  bool grew;
  HIPCHK(h->scratch_d.reserve(need, &grew));
  if (grew) HIPCHK(hipMemsetAsync(h->scratch_d.p, 0, need, stream));       // CU-cache entries and generation counters start empty
  if (h->cfg.tools & VVCX_TOOL_WPP) {                    // scheduler state of this launch: nothing finished, nothing owned, every stream with its tasks left
    HIPCHK(h->wpp_sched_d.reserve((size_t) (4 + 2 * ns)));
    std::vector<int32_t> sched((size_t) (4 + 2 * ns), 0);
    for (int i = 0; i < ns; i++) sched[(size_t) (4 + ns + i)] = sd[(size_t) i].n_tasks;
    HIPCHK(hipMemcpy(h->wpp_sched_d.p, sched.data(), sched.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpyAsync(h->streams_d.p, sd.data(), sizeof(VxStreamDesc) * (size_t) ns, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(h->task_ctu_d.p, task_ctu.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(h->counters_d.p, 0, 56 * sizeof(unsigned long long), stream));

  VxParams p; stream_params(h, p);
  p.scratch_per_stream = per_stream; p.n_streams = ns;
  if (h->cfg.tools & VVCX_TOOL_DEPQUANT) {
    // the quantiser's lambda of a component: TrQuant::setLambdas / selectLambda (EL/EncSlice.cpp:107-149, EL/IntraSearch.cpp:2889) = lambda / distortion weight for chroma
    VxDqConst *tab = h->pend_dq; memset(tab, 0, sizeof h->pend_dq);
    const bool jccr = (h->cfg.tools & VVCX_TOOL_JCCR) != 0;
    for (int comp = 0; comp < 3; comp++) {
      double lam = comp ? h->sl.lambda / h->sl.dist_weight[comp - 1] : h->sl.lambda;
      if (comp && jccr && h->sl.qp > 18) lam = 1.3 * lam;          // EL/IntraSearch.cpp:2937-2942: every chroma block once JointCbCr is on
      const int qp = comp ? p.qp_tr_c[comp - 1] : p.qp_tr;
      for (int lsum = 2; lsum <= 12; lsum++) tab[comp * 16 + lsum] = dq_consts_of(lsum, h->cfg.bit_depth, qp, lam);
    }
    if (jccr) for (int mask = 1; mask <= 3; mask++) {              // joint blocks: the Cb lambda loosened by 0.8 (modes +-1, +-3) or 0.5 (+-2), QP of the coded component or the JointCbCr QP
      double lam = (mask == 3 ? 0.5 : 0.8) * (h->sl.lambda / h->sl.dist_weight[0]);
      if (h->sl.qp > 18) lam = 1.3 * lam;
      const int qp = mask == 3 ? p.qp_tr_j : p.qp_tr_c[(mask >> 1) ? 0 : 1];
      for (int lsum = 2; lsum <= 12; lsum++) tab[(2 + mask) * 16 + lsum] = dq_consts_of(lsum, h->cfg.bit_depth, qp, lam);
    }
    if (h->lmcs_on && h->sl.lmcs_chroma_adj) {
      // chroma residual scaling: the quantiser's lambda of a scaled chroma block is first divided by the square of 2048 / scale (EL/IntraSearch.cpp:2919-2931), one
      // table per bin of the model; the luma row is never read from these tables
      for (int b = 0; b < 16; b++) {
        const double cResScale = 2048.0 / (double) h->lmcs_cadj[b], cbBase = (h->sl.lambda / h->sl.dist_weight[0]) / (cResScale * cResScale);
        VxDqConst *tb = tab + (1 + b) * 96;
        for (int comp = 1; comp < 3; comp++) {
          double lam = (h->sl.lambda / h->sl.dist_weight[comp - 1]) / (cResScale * cResScale);
          if (jccr && h->sl.qp > 18) lam = 1.3 * lam;
          for (int lsum = 2; lsum <= 12; lsum++) tb[comp * 16 + lsum] = dq_consts_of(lsum, h->cfg.bit_depth, p.qp_tr_c[comp - 1], lam);
        }
        if (jccr) for (int mask = 1; mask <= 3; mask++) {
          double lam = (mask == 3 ? 0.5 : 0.8) * cbBase;
          if (h->sl.qp > 18) lam = 1.3 * lam;
          const int qp = mask == 3 ? p.qp_tr_j : p.qp_tr_c[(mask >> 1) ? 0 : 1];
          for (int lsum = 2; lsum <= 12; lsum++) tb[(2 + mask) * 16 + lsum] = dq_consts_of(lsum, h->cfg.bit_depth, qp, lam);
        }
      }
    }
    HIPCHK(hipMemcpyAsync(h->dq_d.p, tab, sizeof h->pend_dq, hipMemcpyHostToDevice, stream));
    p.dq_consts = h->dq_d.p;
  }

  HIPCHK(hipEventRecord(h->ev0, stream));
  if (h->cfg.tools & VVCX_TOOL_WPP) {
    if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_compress_wpp_kernel_u8, dim3((unsigned) grid), dim3(VXD_NT), 0, stream, p);
    else hipLaunchKernelGGL(vvcx_compress_wpp_kernel_u16, dim3((unsigned) grid), dim3(VXD_NT), 0, stream, p);
  } else if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_compress_kernel_u8, dim3((unsigned) grid), dim3(VXD_NT), 0, stream, p);
  else hipLaunchKernelGGL(vvcx_compress_kernel_u16, dim3((unsigned) grid), dim3(VXD_NT), 0, stream, p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev1, stream));
  if (n > h->pend_cap) {                               // pinned, so that the copy back does not block the caller
    (void) hipHostFree(h->pend_res); h->pend_res = nullptr; h->pend_cap = 0;
    HIPCHK(hipHostMalloc((void **) &h->pend_res, sizeof(VxCtuRes) * (size_t) n, 0)); h->pend_cap = n;
  }
  HIPCHK(hipMemcpyAsync(h->pend_res, h->results_d.p, sizeof(VxCtuRes) * (size_t) n, hipMemcpyDeviceToHost, stream));
  h->pending = true; h->pend_stream = stream; h->pend_n = n;
  return VVCX_OK;
}

// 1 once the submitted launch and its copy back have finished (vvcx_wait_ctus will not block), 0 while it runs, < 0 on error
extern "C" int vvcx_poll_ctus(vvcx_handle *h)
{
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  if (!h->pending) return fail(VVCX_ERR_STATE, "nothing submitted");
  if (h->pend_n == 0) return 1;
  ON_DEVICE(h->cfg.device);
  const hipError_t e = hipStreamQuery(h->pend_stream);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(VVCX_ERR_DEVICE, "hipStreamQuery: %s", hipGetErrorString(e));
}

// The collecting half: waits for the stream, advances the streams' positions and hands the results over in task order.
extern "C" int vvcx_wait_ctus(vvcx_handle *h, vvcx_ctu_result *out, int n)
{
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  if (!h->pending) return fail(VVCX_ERR_STATE, "nothing submitted");
  if (n != h->pend_n || (!out && n)) return fail(VVCX_ERR_ARG, "vvcx_wait_ctus: %d results asked, %d tasks submitted", n, h->pend_n);
  h->pending = false;
  if (n == 0) return VVCX_OK;
  ON_DEVICE(h->cfg.device);
  HIPCHK(hipStreamSynchronize(h->pend_stream));
  HIPCHK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  if (h->cfg.tools & VVCX_TOOL_WPP) {
    int32_t st[2] = { 0, 0 };
    HIPCHK(hipMemcpy(st, h->wpp_sched_d.p, sizeof st, hipMemcpyDeviceToHost));
    if (st[1]) {
      // the rows' contexts, coder states and progress counts on the device have advanced part of the way; the host's positions have not: the streams cannot be continued
      h->n_frames = 0;
      return fail(VVCX_ERR_DEVICE, "WPP scheduler gave up: %d of the launch's CTU rows finished, the others never became ready (the pictures are unbound: bind them again)", st[0]);
    }
  }
  h->next_idx = h->pend_next;
  const VxCtuRes *res = h->pend_res;
  for (int k = 0; k < n; k++) {
    vvcx_ctu_result &o = out[h->pend_src[(size_t) k]];
    o.dist = res[k].dist; o.frac_bits = res[k].bits; o.cost = res[k].cost; o.n_cu = res[k].n_cu;
    if (!(res[k].cost < 1.7e+308)) return fail(VVCX_ERR_NO_ENCODING, "no possible encoding found for task %d (EL/EncCu.cpp:555-557)", h->pend_src[(size_t) k]);
  }
  return VVCX_OK;
}

extern "C" int vvcx_compress_ctus(vvcx_handle *h, const vvcx_ctu_task *tasks, int n, vvcx_ctu_result *out, void *hip_stream)
{
  if (h && n == 0 && !h->pending) return (h->cfg.tools & VVCX_TOOL_FAST) && !h->f_ntrees ? fail(VVCX_ERR_STATE, "VVCX_TOOL_FAST needs vvcx_set_forest before the first CTU") : VVCX_OK;
  if (!out) return fail(VVCX_ERR_ARG, "bad argument");
  const int rc = vvcx_submit_ctus(h, tasks, n, hip_stream);
  return rc != VVCX_OK ? rc : vvcx_wait_ctus(h, out, n);
}

extern "C" int vvcx_compress_bound_frames(vvcx_handle *h, vvcx_ctu_result *out, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h || !out) return fail(VVCX_ERR_ARG, "null argument");
  if (h->n_frames == 0) return fail(VVCX_ERR_STATE, "no frames bound");
  const int nctu = h->ctus_w * h->ctus_h;
  std::vector<vvcx_ctu_task> tasks; std::vector<int> dst;
  for (int f = 0; f < h->n_frames; f++) for (int t = 0; t < h->nsub; t++) {
    const std::vector<int> &order = h->sub_ctus[(size_t) t];
    for (size_t k = (size_t) h->next_idx[(size_t) f * h->nsub + t]; k < order.size(); k++) { vvcx_ctu_task tk; tk.frame = f; tk.ctu_rs_addr = order[k]; tasks.push_back(tk); dst.push_back(f * nctu + order[k]); }
  }
  std::vector<vvcx_ctu_result> tmp(tasks.size());
  const int rc = vvcx_compress_ctus(h, tasks.data(), (int) tasks.size(), tmp.data(), hip_stream);
  if (rc != VVCX_OK) return rc;
  for (size_t k = 0; k < tasks.size(); k++) out[dst[k]] = tmp[k];
  return VVCX_OK;
}

// what the picture-level passes behind the search (inverse LMCS, the loop filters, the payload rewrite) start from: every CTU of the bound pictures is coded
int require_all_coded(const vvcx_handle *h, const char *what)
{
  for (size_t i = 0; i < h->next_idx.size(); i++)
    if (h->next_idx[i] != (int) h->sub_ctus[i % (size_t) h->nsub].size())
      return fail(VVCX_ERR_STATE, "%s needs every CTU of the bound pictures coded (frame %d tile %d is not)", what, (int) (i / (size_t) h->nsub), h->sub_tile[i % (size_t) h->nsub]);
  return VVCX_OK;
}

// quantised levels of one component of a coded picture at their sample positions (≙ tu.getCoeffs(compID) of the final TUs), host plane
extern "C" int vvcx_get_levels(vvcx_handle *h, int frame, int comp, int16_t *plane, int stride)
{
  NOT_PENDING(h);
  if (!h || !plane || frame < 0 || frame >= h->n_frames || comp < 0 || comp > 2) return fail(VVCX_ERR_ARG, "bad argument");
  const int w = comp ? h->cfg.pic_w >> 1 : h->cfg.pic_w, hh = comp ? h->cfg.pic_h >> 1 : h->cfg.pic_h;
  if (stride < w) return fail(VVCX_ERR_ARG, "stride smaller than the plane width");
  ON_DEVICE(h->cfg.device);
  const int16_t *src = h->lev_d.p + (size_t) frame * h->lev_frame + (comp == 0 ? 0 : comp == 1 ? h->lev_plane[0] : h->lev_plane[0] + h->lev_plane[1]);
  std::vector<int16_t> tmp((size_t) w * hh);
  HIPCHK(hipMemcpy(tmp.data(), src, tmp.size() * 2, hipMemcpyDeviceToHost));
  for (int y = 0; y < hh; y++) memcpy(plane + (size_t) y * stride, tmp.data() + (size_t) y * w, (size_t) w * 2);
  return VVCX_OK;
}

extern "C" int vvcx_get_cus(vvcx_handle *h, int frame, vvcx_cu *cus, int max_cus, int *n_cus)
{
  NOT_PENDING(h);
  if (!h || !n_cus || frame < 0 || frame >= h->n_frames) return fail(VVCX_ERR_ARG, "bad argument");
  ON_DEVICE(h->cfg.device);
  std::vector<VxUnit> um(h->units_frame);
  HIPCHK(hipMemcpy(um.data(), h->units_d.p + (size_t) frame * h->units_frame, h->units_frame * sizeof(VxUnit), hipMemcpyDeviceToHost));
  int n = 0;
  for (int ry = 0; ry < h->ctus_h; ry++) for (int rx = 0; rx < h->ctus_w; rx++)
    for (int ch = 0; ch < (h->cfg.chroma ? 2 : 1); ch++) {
      const int ul = ch ? 1 : 2;
      for (int uy = ry * 32; uy < std::min(ry * 32 + 32, h->uh); uy++) for (int ux = rx * 32; ux < std::min(rx * 32 + 32, h->uw); ux++) {
        const VxUnit &u = um[(size_t) ch * h->units_plane + (size_t) uy * h->uw + ux];
        if (!u.tag || (u.x >> ul) != ux || (u.y >> ul) != uy) continue;
        if (cus && n < max_cus) {
          vvcx_cu &o = cus[n];
          o.x = u.x; o.y = u.y; o.w = (int16_t) (1 << u.lw); o.h = (int16_t) (1 << u.lh); o.ch_type = (uint8_t) ch;
          o.qt_depth = u.qt; o.bt_depth = u.bt; o.mt_depth = u.mt; o.depth = u.depth; o.intra_dir = u.dir; o.mrl_idx = u.mrl & 0x7f; o.mip_flag = u.mrl >> 7; o.cbf = u.cbf & 7; o.mts_idx = ch ? 0 : (u.mts & 7); o.joint_cb_cr = ch ? (u.mts & 7) : 0; o.lfnst_idx = (u.mts >> 4) & 3; o.split_series = u.ss;
          o.isp_mode = ch ? 0 : u.mts >> 6; o.tu_cbf = ch ? 0 : u.cbf >> 4;
        }
        n++;
      }
    }
  *n_cus = n;
  return (cus && n > max_cus) ? fail(VVCX_ERR_ARG, "CU table too small (%d > %d)", n, max_cus) : VVCX_OK;
}

// The transform units of the coded picture (cs.tus as the reference's encodeCtus / the bitstream writer walk them, CL/CodingStructure.h:216-241): in this
// configuration every CU carries exactly one TU (MaxTbSize 64 = the largest intra CU of a dual-tree I slice), in the order of vvcx_get_cus.
extern "C" int vvcx_get_tus(vvcx_handle *h, int frame, vvcx_tu *tus, int max_tus, int *n_tus)
{
  NOT_PENDING(h);
  if (!h || !n_tus || frame < 0 || frame >= h->n_frames) return fail(VVCX_ERR_ARG, "bad argument");
  int ncu = 0;
  const int rc = vvcx_get_cus(h, frame, nullptr, 0, &ncu);
  if (rc != VVCX_OK) return rc;
  std::vector<vvcx_cu> cus((size_t) ncu);
  const int rc2 = vvcx_get_cus(h, frame, cus.data(), ncu, &ncu);
  if (rc2 != VVCX_OK) return rc2;
  // sub-partitions of a CU coded with ISP (CU::getISPSplitDim, CL/UnitTools.cpp:437-459): a quarter of the side along the split, at least 16 samples each
  auto isp_parts = [](const vvcx_cu &c, int &tw, int &th) {
    if (!c.isp_mode) { tw = c.w; th = c.h; return 1; }
    const int hor = c.isp_mode == 1, split = hor ? c.h : c.w, non = hor ? c.w : c.h;
    int factor = 1; if (non < 16) { int l = 0; while ((1 << (l + 1)) <= non) l++; factor = 16 >> l; }
    const int psz = (split >> 2) < factor ? factor : (split >> 2);
    tw = hor ? c.w : psz; th = hor ? psz : c.h;
    return split / psz;
  };
  int n = 0;
  for (int i = 0; i < ncu; i++) { int tw, th; n += isp_parts(cus[(size_t) i], tw, th); }
  *n_tus = n;
  if (!tus) return VVCX_OK;
  if (n > max_tus) return fail(VVCX_ERR_ARG, "TU table too small (%d > %d)", n, max_tus);
  const int wl = h->cfg.pic_w, wc = h->cfg.pic_w >> 1;
  int o = 0;
  for (int i = 0; i < ncu; i++) {
    const vvcx_cu &c = cus[(size_t) i];
    int tw, th; const int parts = isp_parts(c, tw, th);
    for (int k = 0; k < parts; k++) {
      vvcx_tu &t = tus[o++];
      memset(&t, 0, sizeof t);
      t.cu_index = i; t.ch_type = c.ch_type; t.w = (int16_t) tw; t.h = (int16_t) th; t.depth = c.isp_mode ? 1 : 0;
      t.x = (int16_t) (c.x + (c.isp_mode == 2 ? k * tw : 0)); t.y = (int16_t) (c.y + (c.isp_mode == 1 ? k * th : 0));
      t.mts_idx = c.mts_idx; t.joint_cb_cr = c.joint_cb_cr;
      if (!c.ch_type) { t.cbf[0] = c.isp_mode ? (c.tu_cbf >> k) & 1 : c.cbf & 1; t.coeff_offset[0] = (int32_t) t.y * wl + t.x; t.coeff_stride[0] = wl; t.coeff_offset[1] = t.coeff_offset[2] = -1; }
      else {
        t.cbf[1] = (c.cbf >> 1) & 1; t.cbf[2] = (c.cbf >> 2) & 1;
        t.coeff_offset[0] = -1; t.coeff_offset[1] = t.coeff_offset[2] = (int32_t) c.y * wc + c.x; t.coeff_stride[1] = t.coeff_stride[2] = wc;
      }
    }
  }
  return VVCX_OK;
}

extern "C" float vvcx_last_kernel_ms(const vvcx_handle *h) { return h ? h->last_ms : 0.f; }

extern "C" int vvcx_get_counters(vvcx_handle *h, uint64_t out[4])
{
  NOT_PENDING(h);
  if (!h || !out) return fail(VVCX_ERR_ARG, "null argument");
  ON_DEVICE(h->cfg.device);
  unsigned long long c[4];
  HIPCHK(hipMemcpy(c, h->counters_d.p, sizeof c, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; i++) out[i] = c[i];
  return VVCX_OK;
}

// diagnostic: shader-clock ticks summed over streams per controller/operation kind of the last launch
// [0] controller, [op] parallel operation `op` (enum in vvcx_kernel.hip), [12] estimator pass
extern "C" int vvcx_get_profile(vvcx_handle *h, uint64_t out[48])
{
  NOT_PENDING(h);
  if (!h || !out) return fail(VVCX_ERR_ARG, "null argument");
  ON_DEVICE(h->cfg.device);
  unsigned long long c[52];
  HIPCHK(hipMemcpy(c, h->counters_d.p, sizeof c, hipMemcpyDeviceToHost));
  for (int i = 0; i < 48; i++) out[i] = c[4 + i];
  return VVCX_OK;
}

// ≙ what CABACWriter::coding_tree_unit writes in front of every coding tree (EL/CABACWriter.cpp:254-309: sao 323-462, codeAlfCtuEnableFlag 4700-4725, codeAlfCtuFilterIndex
// 4833-4892, codeAlfCtuAlternative 4920-4943).  The parameters exist only after the picture has been searched and analysed, so every tile's payload is written once more,
// from the CU maps and level planes that persist on the device (vvcx_kernel.hip rewrite_tile).  Everything the syntax cannot carry is refused here, before any launch.
static int rewrite_check(const vvcx_handle *h, const vvcx_ctu_syntax *hdr, const vvcx_sao_param *sao, const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slices,
                         const vvcx_alf_ctu *ctus, std::vector<VxCtuSynFrame> &hd, std::vector<VxAlfCtu> &alf)
{
  const int cw = h->ctus_w, nctu = cw * h->ctus_h, bd = h->cfg.bit_depth, maxQ = (1 << ((bd < 10 ? bd : 10) - 5)) - 1;      // SampleAdaptiveOffset::getMaxOffsetQVal
  hd.assign((size_t) h->n_frames, VxCtuSynFrame());
  if (ctus) alf.assign((size_t) h->n_frames * nctu, VxAlfCtu());
  if (n_aps < 0 || n_aps > 8 || (n_aps > 0 && !aps)) return fail(VVCX_ERR_ARG, "ALF: %d parameter sets (0..8)", n_aps);
  for (int f = 0; f < h->n_frames; f++) {
    VxCtuSynFrame &o = hd[(size_t) f];
    memset(&o, 0, sizeof o);
    o.sao_luma = hdr[f].sao_luma != 0; o.sao_chroma = hdr[f].sao_chroma != 0;
    for (int c = 0; c < 3; c++) o.alf[c] = hdr[f].alf[c] != 0;
    if (!h->cfg.chroma && (o.sao_chroma || o.alf[1] || o.alf[2])) return fail(VVCX_ERR_ARG, "frame %d: chroma syntax enabled on a handle without chroma", f);
    if ((o.sao_luma || o.sao_chroma) && !sao) return fail(VVCX_ERR_ARG, "frame %d has SAO on and no parameters were given", f);
    if ((o.alf[0] || o.alf[1] || o.alf[2]) && (!slices || !ctus)) return fail(VVCX_ERR_ARG, "frame %d has ALF on and no slice / CTU choices were given", f);
    if (sao) for (int a = 0; a < nctu; a++) {
      const vvcx_sao_param *p = sao + ((size_t) f * nctu + a) * 3;
      const int on[3] = { o.sao_luma, o.sao_chroma, o.sao_chroma };
#define SAO_BAD(fmt, ...) return fail(VVCX_ERR_ARG, "SAO parameters of frame %d CTU %d: " fmt, f, a, ##__VA_ARGS__)
      for (int c = 0; c < 3; c++) if (p[c].mode < 0 || p[c].mode > 2) SAO_BAD("component %d has mode %d", c, p[c].mode);
      if (p[0].mode == 2 || p[1].mode == 2 || p[2].mode == 2) {
        if (p[0].mode != 2 || p[1].mode != 2 || p[2].mode != 2 || p[1].type != p[0].type || p[2].type != p[0].type) SAO_BAD("a merge must be set on all three components alike");
        if (p[0].type != 0 && p[0].type != 1) SAO_BAD("merge type %d", p[0].type);
        if (!on[0] && !on[1]) SAO_BAD("a merge in a slice that has SAO off");
        const int left = p[0].type == 0, src = left ? a - 1 : a - cw;
        if ((left ? a % cw == 0 : a < cw) || h->ctu_tile[(size_t) src] != h->ctu_tile[(size_t) a]) SAO_BAD("no %s merge candidate in the tile", left ? "left" : "above");
        continue;
      }
      for (int c = 0; c < 3; c++) {
        if (p[c].mode == 0) continue;
        if (!on[c]) SAO_BAD("component %d is on in a slice that has it disabled", c);
        if (p[c].type < 0 || p[c].type > 4 || p[c].band < 0 || p[c].band > 31) SAO_BAD("component %d: type %d band %d", c, p[c].type, p[c].band);
        for (int i = 0; i < 4; i++) {
          const int v = p[c].offset[i];
          if (v < -maxQ || v > maxQ) SAO_BAD("component %d: offset %d beyond +-%d", c, v, maxQ);
          if (p[c].type != 4 && (i < 2 ? v < 0 : v > 0)) SAO_BAD("component %d: edge offset %d is %d, its sign is implicit", c, i, v);
        }
      }
      if (p[1].mode != p[2].mode || (p[1].mode == 1 && p[1].type != p[2].type)) SAO_BAD("Cb and Cr share sao_type_idx_chroma and the edge class");
#undef SAO_BAD
    }
    const bool alfOn = o.alf[0] || o.alf[1] || o.alf[2];
    if (alfOn) {
      const vvcx_alf_slice &sl = slices[f];
      if (o.alf[0]) {
        if (sl.n_luma_aps < 0 || sl.n_luma_aps > 8) return fail(VVCX_ERR_ARG, "ALF slice of frame %d: %d luma sets", f, sl.n_luma_aps);
        for (int k = 0; k < sl.n_luma_aps; k++) if (sl.luma_aps[k] < 0 || sl.luma_aps[k] >= n_aps) return fail(VVCX_ERR_ARG, "ALF slice of frame %d: luma set %d of %d", f, sl.luma_aps[k], n_aps);
        o.n_aps = (uint8_t) sl.n_luma_aps;
      }
      if (o.alf[1] || o.alf[2]) {
        if (sl.chroma_aps < 0 || sl.chroma_aps >= n_aps || aps[sl.chroma_aps].num_chroma_alt < 1 || aps[sl.chroma_aps].num_chroma_alt > 8)
          return fail(VVCX_ERR_ARG, "ALF slice of frame %d: chroma is on and chroma set %d of %d has no alternatives", f, sl.chroma_aps, n_aps);
        o.n_alt = (uint8_t) aps[sl.chroma_aps].num_chroma_alt;
      }
    }
    if (ctus) for (int a = 0; a < nctu; a++) {
      const vvcx_alf_ctu &u = ctus[(size_t) f * nctu + a]; VxAlfCtu &d = alf[(size_t) f * nctu + a];
      memset(&d, 0, sizeof d);
      for (int c = 0; c < 3; c++) {
        if (!u.flag[c]) continue;
        if (!o.alf[c]) return fail(VVCX_ERR_ARG, "ALF: frame %d CTU %d has the flag of component %d set, which the slice disables", f, a, c);
        d.flag[c] = 1;
      }
      if (u.flag[0]) { if (u.set < 0 || u.set >= 16 + o.n_aps) return fail(VVCX_ERR_ARG, "ALF: frame %d CTU %d uses luma filter set %d of %d", f, a, u.set, 16 + o.n_aps); d.set = u.set; }
      for (int c = 1; c < 3; c++) if (u.flag[c]) { if (u.alt[c - 1] >= o.n_alt) return fail(VVCX_ERR_ARG, "ALF: frame %d CTU %d uses chroma alternative %d of %d", f, a, u.alt[c - 1], o.n_alt); d.alt[c - 1] = u.alt[c - 1]; }
    }
  }
  return VVCX_OK;
}
static void ctx_state_islice(int id, int qp, uint16_t &s0, uint16_t &s1)      // one model of CtxStore::init (ctx_init_islice)
{
  qp = qp < 0 ? 0 : qp > 63 ? 63 : qp;
  const int slope = (id >> 3) - 4, offset = ((id & 7) * 18) + 1;
  int st = ((slope * (qp - 16)) >> 1) + offset;
  st = st < 1 ? 1 : st > 127 ? 127 : st;
  s0 = (uint16_t) ((st << 8) & 0x7FE0); s1 = (uint16_t) ((st << 8) & 0x7FFE);
}
static_assert(VXD_NUM_CS_CTX == VX_CS_NUM_CTX, "vvcx_dev.h and vvcx_ctu_syntax_tables.h disagree on the number of CTU-syntax models");
static_assert(sizeof(VxSaoSyn) == sizeof(vvcx_sao_param) && sizeof(VxAlfCtu) == sizeof(vvcx_alf_ctu), "device copies of the C-ABI records");
extern "C" int vvcx_rewrite_payload_bound_frames(vvcx_handle *h, const vvcx_ctu_syntax *hdr, const vvcx_sao_param *sao, const vvcx_alf_aps *aps, int n_aps,
                                                 const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int trace_ops_per_tile, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h || !hdr || trace_ops_per_tile < 0) return fail(VVCX_ERR_ARG, "bad argument");
  if (!h->payload_d.p) return fail(VVCX_ERR_STATE, "handle was created without emit_payload");
  if (!h->n_frames || !h->have_slice) return fail(VVCX_ERR_STATE, "no bound frames / slice");
  if (const int rc = require_all_coded(h, "the payload rewrite")) return rc;
  std::vector<VxCtuSynFrame> hd; std::vector<VxAlfCtu> alf;
  if (const int rc = rewrite_check(h, hdr, sao, aps, n_aps, slices, ctus, hd, alf)) return rc;
  const int nctu = h->ctus_w * h->ctus_h, nwg = h->n_frames * h->ntiles;
  // tile and sub-stream tables: tile_sub0[ntiles] | tile_nsub[ntiles] | sub_first[nsub + 1] | sub_ctu[nctu] | tile_of_ctu[nctu]
  std::vector<int32_t> tab;
  for (int t = 0; t < h->ntiles; t++) tab.push_back(h->tile_sub0[(size_t) t]);
  for (int t = 0; t < h->ntiles; t++) tab.push_back(h->tile_nsub[(size_t) t]);
  { int n = 0; for (int s = 0; s < h->nsub; s++) { tab.push_back(n); n += (int) h->sub_ctus[(size_t) s].size(); } tab.push_back(n); }
  for (int s = 0; s < h->nsub; s++) for (int a : h->sub_ctus[(size_t) s]) tab.push_back(a);
  for (int a = 0; a < nctu; a++) tab.push_back(h->ctu_tile[(size_t) a]);
  uint16_t ctx0[VXD_RW_CTX];
  ctx_init_islice(h->sl.qp, ctx0, ctx0 + VXD_NUM_CTX);
  for (int k = 0; k < VX_CS_NUM_CTX; k++) ctx_state_islice(VX_CS_INIT_I[k], h->sl.qp, ctx0[2 * VXD_NUM_CTX + k], ctx0[2 * VXD_NUM_CTX + VX_CS_NUM_CTX + k]);
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  const bool saoOn = sao != nullptr, alfOn = ctus != nullptr;
  HIPCHK(h->rw_hdr_d.reserve(hd.size())); HIPCHK(h->rw_tab_d.reserve(tab.size())); HIPCHK(h->rw_ctx_d.reserve((size_t) VXD_RW_CTX * (1 + (size_t) nwg)));
  HIPCHK(h->rw_scratch_d.reserve((size_t) nwg * VXD_RW_SCRATCH)); HIPCHK(h->rw_trace_n_d.reserve((size_t) nwg));
  if (saoOn) HIPCHK(h->rw_sao_d.reserve((size_t) h->n_frames * nctu * 3));
  if (alfOn) HIPCHK(h->rw_alf_d.reserve(alf.size()));
  if (trace_ops_per_tile) HIPCHK(h->rw_trace_d.reserve((size_t) nwg * 3 * (size_t) trace_ops_per_tile));
  h->rw_trace_n.clear(); h->rw_trace_cap = 0;
  HIPCHK(hipMemcpyAsync(h->rw_hdr_d.p, hd.data(), hd.size() * sizeof(VxCtuSynFrame), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(h->rw_tab_d.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(h->rw_ctx_d.p, ctx0, sizeof ctx0, hipMemcpyHostToDevice, stream));
  if (saoOn) HIPCHK(hipMemcpyAsync(h->rw_sao_d.p, sao, (size_t) h->n_frames * nctu * 3 * sizeof(VxSaoSyn), hipMemcpyHostToDevice, stream));
  if (alfOn) HIPCHK(hipMemcpyAsync(h->rw_alf_d.p, alf.data(), alf.size() * sizeof(VxAlfCtu), hipMemcpyHostToDevice, stream));
  VxParams p; stream_params(h, p);
  VxRewriteParams r; memset(&r, 0, sizeof r);
  r.hdr = h->rw_hdr_d.p; r.sao = saoOn ? h->rw_sao_d.p : nullptr; r.alf = alfOn ? h->rw_alf_d.p : nullptr;
  r.tile_sub0 = h->rw_tab_d.p; r.tile_nsub = r.tile_sub0 + h->ntiles; r.sub_first = r.tile_nsub + h->ntiles; r.sub_ctu = r.sub_first + h->nsub + 1; r.tile_of_ctu = r.sub_ctu + nctu;
  r.ctx0 = h->rw_ctx_d.p; r.sync = h->rw_ctx_d.p + VXD_RW_CTX; r.scratch = h->rw_scratch_d.p;
  r.trace = trace_ops_per_tile ? h->rw_trace_d.p : nullptr; r.trace_n = h->rw_trace_n_d.p; r.trace_cap = trace_ops_per_tile;
  // one workgroup per (frame, tile), VXD_NT threads each: thread 0 codes the tile, the others exist only to stage the constant tables (load_tables strides by VXD_NT) and leave
  HIPCHK(hipEventRecord(h->ev0, stream));
  if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_rewrite_kernel_u8, dim3((unsigned) nwg), dim3(VXD_NT), 0, stream, p, r);
  else hipLaunchKernelGGL(vvcx_rewrite_kernel_u16, dim3((unsigned) nwg), dim3(VXD_NT), 0, stream, p, r);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev1, stream));
  HIPCHK(hipStreamSynchronize(stream));             // (the host tables above must outlive the copies)
  HIPCHK(hipEventElapsedTime(&h->last_rewrite_ms, h->ev0, h->ev1));
  if (trace_ops_per_tile) {
    h->rw_trace_n.resize((size_t) nwg);
    HIPCHK(hipMemcpy(h->rw_trace_n.data(), h->rw_trace_n_d.p, (size_t) nwg * sizeof(uint32_t), hipMemcpyDeviceToHost));
    h->rw_trace_cap = trace_ops_per_tile;
  }
  return VVCX_OK;
}
extern "C" float vvcx_last_rewrite_ms(const vvcx_handle *h) { return h ? h->last_rewrite_ms : 0.f; }
// diagnostic: the operation string the last rewrite coded for one tile (what pins its bytes to the reference's coder, tests/test_ctu_syntax.py)
extern "C" int vvcx_get_payload_ops(vvcx_handle *h, int frame, int tile, int32_t *ops, int max_ops, int *n_ops)
{
  NOT_PENDING(h);
  if (!h || !n_ops || max_ops < 0 || (!ops && max_ops) || frame < 0 || frame >= h->n_frames || tile < 0 || tile >= h->ntiles) return fail(VVCX_ERR_ARG, "bad argument");
  if (!h->rw_trace_cap || h->rw_trace_n.size() != (size_t) h->n_frames * h->ntiles) return fail(VVCX_ERR_STATE, "no rewrite with a trace since the pictures were bound");
  const size_t wg = (size_t) frame * h->ntiles + tile;
  const uint32_t n = h->rw_trace_n[wg];
  *n_ops = (int) n;
  if (n > (uint32_t) h->rw_trace_cap) return fail(VVCX_ERR_ARG, "tile %d of frame %d coded %u operations, the rewrite kept room for %d per tile", tile, frame, n, h->rw_trace_cap);
  if (!ops) return VVCX_OK;                            // count query
  if (n > (uint32_t) max_ops) return fail(VVCX_ERR_ARG, "room for %d operations, the tile has %u", max_ops, n);
  ON_DEVICE(h->cfg.device);
  HIPCHK(hipMemcpy(ops, h->rw_trace_d.p + wg * 3 * (size_t) h->rw_trace_cap, (size_t) n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// slice_data() payload of one tile of a bound frame (≙ the sub-streams EncSlice::encodeSlice hands to the NAL writer, EL/EncSlice.cpp:1884-2006): one byte string, or with
// VVCX_TOOL_WPP the byte strings of the tile's CTU rows back to back (sizes: vvcx_get_substream_sizes)
static int payload_of_tile(vvcx_handle *h, int frame, int tile, uint8_t *buf, int cap, int *nbytes, int *sizes, int max_sizes, int *n_sizes)
{
  if (!h || frame < 0 || frame >= h->n_frames || tile < 0 || tile >= h->ntiles) return fail(VVCX_ERR_ARG, "bad argument");
  if (!h->payload_d.p) return fail(VVCX_ERR_STATE, "handle was created without emit_payload");
  ON_DEVICE(h->cfg.device);
  const int sub0 = h->tile_sub0[(size_t) tile], ns = h->tile_nsub[(size_t) tile];
  if (n_sizes) *n_sizes = ns;
  if (sizes && max_sizes < ns) return fail(VVCX_ERR_ARG, "room for %d sub-stream sizes, the tile has %d", max_sizes, ns);
  size_t total = 0;
  for (int k = 0; k < ns; k++) {
    const size_t s = (size_t) frame * h->nsub + (size_t) (sub0 + k);
    if (h->next_idx[s] != (int) h->sub_ctus[(size_t) (sub0 + k)].size()) return fail(VVCX_ERR_STATE, "tile %d of frame %d is not completely coded yet", tile, frame);
    uint32_t st[8];
    HIPCHK(hipMemcpy(st, (const uint8_t *) h->arith_d.p + s * 32, 32, hipMemcpyDeviceToHost));
    const uint32_t n = st[7];                        // Arith::n
    if (n > h->payload_cap[s]) return fail(VVCX_ERR_STATE, "payload of tile %d exceeds the %u bytes reserved", tile, h->payload_cap[s]);
    if (sizes) sizes[k] = (int) n;
    if (buf && total + n <= (size_t) cap) HIPCHK(hipMemcpy(buf + total, h->payload_d.p + h->payload_off[s], n, hipMemcpyDeviceToHost));
    total += n;
  }
  if (nbytes) *nbytes = (int) total;
  if (buf && total > (size_t) cap) return fail(VVCX_ERR_ARG, "buffer too small: %zu bytes needed", total);
  return VVCX_OK;
}
// GET_TRAINING_SET counterpart (the fork's CL/TypeDef.h:54-56 switch; EL/EncCu.cpp:863-1123 computes the features, the label is the partition the full search chose)
extern "C" int vvcx_enable_training_dump(vvcx_handle *h, int cap_rows)
{
  NOT_PENDING(h);
  if (!h || cap_rows < 0) return fail(VVCX_ERR_ARG, "bad argument");
  // the features look at the CUs above-right and below-left of a node through the unrestricted neighbour lookup; under WPP those belong to rows that run at their own
  // pace, so the rows would depend on timing (the same reason VVCX_TOOL_FAST is refused together with WPP)
  if (cap_rows > 0 && (h->cfg.tools & VVCX_TOOL_WPP)) return fail(VVCX_ERR_UNSUPPORTED, "the training dump is not available on a WPP handle");
  ON_DEVICE(h->cfg.device);
  h->train_cap = 0; h->train_rows_d.release(); h->train_n_d.release();
  if (cap_rows == 0) return VVCX_OK;
  if (h->train_rows_d.alloc((size_t) cap_rows * 28) != hipSuccess || h->train_n_d.alloc(1) != hipSuccess) {
    h->train_rows_d.release();                        // (a dump is on while the rows exist)
    return fail(VVCX_ERR_DEVICE, "device allocation of %d training rows failed", cap_rows);
  }
  HIPCHK(hipMemset(h->train_n_d.p, 0, 4));
  h->train_cap = cap_rows;
  return VVCX_OK;
}
extern "C" int vvcx_get_training_rows(vvcx_handle *h, int32_t *rows, int max_rows, int *n_rows)
{
  NOT_PENDING(h);
  if (!h || !n_rows || max_rows < 0 || (!rows && max_rows)) return fail(VVCX_ERR_ARG, "bad argument");
  if (!h->train_rows_d.p) return fail(VVCX_ERR_STATE, "vvcx_enable_training_dump first");
  ON_DEVICE(h->cfg.device);
  uint32_t n = 0;
  HIPCHK(hipMemcpy(&n, h->train_n_d.p, 4, hipMemcpyDeviceToHost));
  *n_rows = (int) n;                                  // rows asked for; more than the capacity means the tail was dropped
  const int have = (int) (n < (uint32_t) h->train_cap ? n : (uint32_t) h->train_cap), take = have < max_rows ? have : max_rows;
  if (take) HIPCHK(hipMemcpy(rows, h->train_rows_d.p, (size_t) take * 28 * 4, hipMemcpyDeviceToHost));
  return VVCX_OK;
}
extern "C" int vvcx_get_payload(vvcx_handle *h, int frame, int tile, uint8_t *buf, int cap, int *nbytes)
{
  NOT_PENDING(h);
  if (!buf || !nbytes) return fail(VVCX_ERR_ARG, "bad argument");
  return payload_of_tile(h, frame, tile, buf, cap, nbytes, nullptr, 0, nullptr);
}
extern "C" int vvcx_get_substream_sizes(vvcx_handle *h, int frame, int tile, int *sizes, int max_sizes, int *n_sizes)
{
  NOT_PENDING(h);
  if (!n_sizes) return fail(VVCX_ERR_ARG, "bad argument");
  return payload_of_tile(h, frame, tile, nullptr, 0, nullptr, sizes, max_sizes, n_sizes);
}
