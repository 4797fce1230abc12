// vvcx_api_loopfilter.hip — the entry points of the C-ABI (include/vvcx.h) behind the search: inverse LMCS, deblocking, SAO and ALF with their encoder sides, on the
// pictures bound to a handle (the caller's stream, HIP events around the kernels) and on one picture in host memory (the null stream).  What they share is said once,
// in front of them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "vvcx.h"
#include "vvcx_handle.h"      // the handle, NOT_PENDING, fail; vvcx_host.h: DevBuf, ON_DEVICE / DevGuard, HIPCHK
#include "vvcx_kernels.h"
#include "vvcx_sao_rd.h"      // SaoRate: the start states of the device decision's two context models; VX_BIN_FRAC_BITS
#include "vvcx_alf_derive.h"  // the tables of the caller's ALF parameter sets, the filter derivation

// ---- what the entries share

// the resident results a bound-frame call ends: the statistics of vvcx_alf_statistics_resident, the decision of vvcx_sao_decide_resident
enum { ENDS_ALF = 1, ENDS_SAO = 2 };

// The opening of a bound-frame entry, behind NOT_PENDING.  `ends` is carried out first, whatever the call then returns: a call that changes the pictures ends both
// resident results, the two statistics entries only reuse the buffers of their own side.  Then the refusals, in this order: a null argument (args: the entry's
// pointer arguments are there); no bound pictures or no slice; an LMCS slice at all, for the entries that read the original (refused_on_lmcs names what they gather):
// the handle keeps the mapped copy only; a CTU that is not coded (`what` needs them all); an LMCS slice whose reconstruction has not been mapped back.
static int bound_entry(vvcx_handle *h, bool args, int ends, const char *what, const char *refused_on_lmcs = nullptr)
{
  if (h && (ends & ENDS_ALF)) h->alf_res_valid = false;
  if (h && (ends & ENDS_SAO)) h->sao_res_valid = false;
  if (!h || !args) return fail(VVCX_ERR_ARG, "null argument");
  if (!h->n_frames || !h->have_slice) return fail(VVCX_ERR_STATE, "no bound frames / slice");
  if (h->lmcs_on && refused_on_lmcs) return fail(VVCX_ERR_UNSUPPORTED, "%s of an LMCS slice: the handle keeps the mapped original only", refused_on_lmcs);
  if (const int rc = require_all_coded(h, what)) return rc;
  if (h->lmcs_on && !h->lmcs_inverted) return fail(VVCX_ERR_STATE, "LMCS slice: vvcx_lmcs_inverse_reco first (the loop filters work in the original domain)");
  return VVCX_OK;
}

// The timed bracket of a bound-frame entry: ev0 is recorded in front of its launches; behind them timed_end takes their launch error and records ev1; at the end of
// the call, behind the copies it queued after ev1, timed_wait waits for the stream and writes the kernel time ev0 .. ev1
static hipError_t timed_end(vvcx_handle *h, hipStream_t stream) { const hipError_t e = hipGetLastError(); return e != hipSuccess ? e : hipEventRecord(h->ev1, stream); }
static hipError_t timed_wait(vvcx_handle *h, hipStream_t stream, float *ms) { const hipError_t e = hipStreamSynchronize(stream); return e != hipSuccess ? e : hipEventElapsedTime(ms, h->ev0, h->ev1); }

// the pictures an entry works on, frame records in device memory and their geometry: the bound pictures of a handle, or one picture from host memory (DevPicture)
struct Pics {
  const VxFrameDev *frames; int n, w, h, bit_depth, chroma; size_t bps;
  int ctus_w() const { return (w + 127) / 128; }
  int ctus_h() const { return (h + 127) / 128; }
  int nctu() const { return ctus_w() * ctus_h(); }
  size_t ny() const { return (size_t) w * h; }                 // samples of the luma plane; a chroma plane has a quarter
  size_t samples() const { return ny() + 2 * (ny() >> 2); }    // of one picture
};
static Pics bound_pics(const vvcx_handle *h) { return Pics{ h->frames_d.p, h->n_frames, h->cfg.pic_w, h->cfg.pic_h, h->cfg.bit_depth, h->cfg.chroma, (size_t) (h->cfg.bit_depth == 8 ? 1 : 2) }; }

// what every host-picture entry asks of its picture: sides that are multiples of 8 up to 16384, 8 .. 12 bits; of its tile grid: the picture has the CTUs for it, at
// most 255 tiles (the CTU -> tile table holds bytes)
static bool picture_ok(int pic_w, int pic_h, int bit_depth) { return pic_w >= 8 && pic_h >= 8 && !(pic_w & 7) && !(pic_h & 7) && pic_w <= 16384 && pic_h <= 16384 && bit_depth >= 8 && bit_depth <= 12; }
static bool tiles_ok(int pic_w, int pic_h, int tile_cols, int tile_rows) { return tile_cols >= 1 && tile_rows >= 1 && tile_cols <= (pic_w + 127) / 128 && tile_rows <= (pic_h + 127) / 128 && tile_cols * tile_rows <= 255; }

// tile of each CTU (raster address) of cw x chh CTUs under a uniform split: boundary i = i * N / T
static std::vector<uint8_t> tile_of_ctu_table(int cw, int chh, int tile_cols, int tile_rows)
{
  std::vector<uint8_t> tile((size_t) cw * chh);
  for (int a = 0; a < cw * chh; a++) {
    int tx = 0, ty = 0;
    for (int i = 0; i < tile_cols; i++) if (a % cw >= (i * cw) / tile_cols) tx = i;
    for (int i = 0; i < tile_rows; i++) if (a / cw >= (i * chh) / tile_rows) ty = i;
    tile[(size_t) a] = (uint8_t) (ty * tile_cols + tx);
  }
  return tile;
}

// One 4:2:0 picture of uint16 samples in host memory (stride = plane width) the way the host-picture entries keep it on the device: the planes in one allocation and
// the frame record the kernels reach them through.  rec: the planes the kernels work on, copied back by download; org: the original beside them, for the encoder-side
// statistics; units_d: both trees' unit maps, for the deblocking
struct DevPicture {
  DevBuf<uint16_t> planes; DevBuf<VxFrameDev> frame; int w, h; size_t ny, nc;
  int upload(int pic_w, int pic_h, const uint16_t *const rec[3], const uint16_t *const org[3] = nullptr, VxUnit *units_d = nullptr)
  {
    w = pic_w; h = pic_h; ny = (size_t) pic_w * pic_h; nc = ny >> 2;
    const size_t per = ny + 2 * nc, off[3] = { 0, ny, ny + nc };
    HIPCHK(planes.alloc(org ? 2 * per : per)); HIPCHK(frame.alloc(1));
    VxFrameDev fd; memset(&fd, 0, sizeof fd);
    for (int c = 0; c < 3; c++) {
      fd.rec[c] = planes.p + off[c]; fd.stride[c] = c ? pic_w >> 1 : pic_w;
      HIPCHK(hipMemcpy(planes.p + off[c], rec[c], (c ? nc : ny) * 2, hipMemcpyHostToDevice));
      if (!org) continue;
      fd.org[c] = planes.p + per + off[c];
      HIPCHK(hipMemcpy(planes.p + per + off[c], org[c], (c ? nc : ny) * 2, hipMemcpyHostToDevice));
    }
    if (units_d) { fd.units[0] = units_d; fd.units[1] = units_d + (size_t) (pic_w >> 2) * (pic_h >> 2); }
    HIPCHK(hipMemcpy(frame.p, &fd, sizeof fd, hipMemcpyHostToDevice));
    return VVCX_OK;
  }
  Pics pics(int bit_depth) const { return Pics{ frame.p, 1, w, h, bit_depth, 1, 2 }; }
  int download(uint16_t *y, uint16_t *cb, uint16_t *cr)      // behind the launches: their launch errors, their end, the planes
  {
    HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(y, planes.p, ny * 2, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(cb, planes.p + ny, nc * 2, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cr, planes.p + ny + nc, nc * 2, hipMemcpyDeviceToHost));
    return VVCX_OK;
  }
};

// LMCS: luma reconstruction of every bound picture back to the original domain, in place (the picture-level inverse rspSignal in front of the loop filters).
// Its opening is its own: what bound_entry asks of an LMCS slice is what this call brings about, and its refusals say so
extern "C" int vvcx_lmcs_inverse_reco(vvcx_handle *h, void *hip_stream)
{
  NOT_PENDING(h);
  if (h) h->alf_res_valid = h->sao_res_valid = false;      // the resident ALF statistics / SAO decision no longer describe the bound pictures
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  if (!h->n_frames || !h->have_slice || !h->lmcs_on) return fail(VVCX_ERR_STATE, "no bound frames coded with an LMCS slice");
  if (!h->lmcs_lut_d.p) return fail(VVCX_ERR_STATE, "the bound pictures were not prepared with an LMCS slice: vvcx_bind_frames after vvcx_set_slice");
  if (h->lmcs_inverted) return fail(VVCX_ERR_STATE, "the reconstruction has already been mapped back");
  if (const int rc = require_all_coded(h, "the inverse LMCS mapping (intra prediction reads mapped neighbours)")) return rc;
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  const unsigned blocks = (unsigned) (((size_t) h->cfg.pic_w * h->cfg.pic_h + VXD_NT - 1) / VXD_NT);
  for (int f = 0; f < h->n_frames; f++) {
    const VxFrameDev &d = h->frames_h[(size_t) f];
    if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_lmcs_map_kernel_u8, dim3(blocks), dim3(VXD_NT), 0, stream, (const uint8_t *) d.rec[0], (uint8_t *) d.rec[0], h->cfg.pic_w, h->cfg.pic_h, d.stride[0], h->lmcs_lut_d.p + 1024);
    else hipLaunchKernelGGL(vvcx_lmcs_map_kernel_u16, dim3(blocks), dim3(VXD_NT), 0, stream, (const uint16_t *) d.rec[0], (uint16_t *) d.rec[0], h->cfg.pic_w, h->cfg.pic_h, d.stride[0], h->lmcs_lut_d.p + 1024);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(stream));
  h->lmcs_inverted = true;
  return VVCX_OK;
}

// ≙ LoopFilter::loopFilterPic (CL/LoopFilter.cpp:153) on every bound picture, in place on the reconstruction planes the search wrote:
// one launch for all vertical edges, one for all horizontal edges (vvcx_deblock.hip).  Every CTU of the pictures must have been coded.
extern "C" int vvcx_deblock_bound_frames(vvcx_handle *h, int beta_offset_div2, int tc_offset_div2, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  if (const int rc = bound_entry(h, true, ENDS_ALF | ENDS_SAO, "deblocking")) return rc;
  if (beta_offset_div2 < -6 || beta_offset_div2 > 6 || tc_offset_div2 < -6 || tc_offset_div2 > 6) return fail(VVCX_ERR_ARG, "deblocking offsets outside -6..6");
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  VxDeblockParams p; memset(&p, 0, sizeof p);
  p.frames = h->frames_d.p; p.uw = h->uw; p.uh = h->uh; p.bit_depth = h->cfg.bit_depth; p.chroma = h->cfg.chroma;
  p.qp = h->sl.qp; p.qp_c[0] = h->sl.qp_c[0]; p.qp_c[1] = h->sl.qp_c[1]; p.beta_off2 = beta_offset_div2; p.tc_off2 = tc_offset_div2;
  const dim3 grid((unsigned) ((2 * h->uw * h->uh + 255) / 256), (unsigned) h->n_frames);
  const size_t nedge = (size_t) h->n_frames * 4 * h->uw * h->uh;
  HIPCHK(h->db_edges_d.reserve(nedge));
  p.edges = h->db_edges_d.p;
  HIPCHK(hipEventRecord(h->ev0, stream));
  hipLaunchKernelGGL(vvcx_deblock_edges_kernel, grid, dim3(256), 0, stream, p);      // the unit records -> one edge byte per unit, map and direction
  HIPCHK(hipGetLastError());
  for (int dir = 0; dir < 2; dir++) {
    p.dir = dir;
    if (h->cfg.bit_depth == 8) hipLaunchKernelGGL(vvcx_deblock_kernel_u8, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(vvcx_deblock_kernel_u16, grid, dim3(256), 0, stream, p);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(h->ev1, stream));      // (every launch above took its own error)
  HIPCHK(timed_wait(h, stream, &h->last_deblock_ms));
  return VVCX_OK;
}
extern "C" float vvcx_last_deblock_ms(const vvcx_handle *h) { return h ? h->last_deblock_ms : 0.f; }

// ≙ SampleAdaptiveOffset::SAOProcess (CL/SampleAdaptiveOffset.cpp:617-670) with the caller's parameters prm[frame][ctu][component]: merges are resolved here
// (xReconstructBlkSAOParams 265-290: the CTU to the left / above in the same tile (`tile`: tile_of_ctu_table), in raster order; invertQuantOffsets 147-170), the samples
// are filtered on the device (vvcx_sao.hip) in place on the reconstruction planes.
static int sao_resolve(const vvcx_sao_param *prm, int n_frames, int cw, int chh, const std::vector<uint8_t> &tile, int log2_offset_scale, std::vector<VxSaoEntry> &tab)
{
  const int nctu = cw * chh;
  tab.resize((size_t) n_frames * nctu * 3);
  for (int f = 0; f < n_frames; f++) for (int a = 0; a < nctu; a++) for (int c = 0; c < 3; c++) {
    const vvcx_sao_param &p = prm[((size_t) f * nctu + a) * 3 + c];
    VxSaoEntry &e = tab[((size_t) f * nctu + a) * 3 + c];
    memset(&e, 0, sizeof e); e.type = -1;
    if (p.mode == 0) continue;
    if (p.mode == 1) {
      if (p.type < 0 || p.type > 4 || p.band < 0 || p.band > 31) return fail(VVCX_ERR_ARG, "SAO parameters of frame %d CTU %d component %d: type %d band %d", f, a, c, p.type, p.band);
      e.type = p.type; e.band = p.type == 4 ? p.band : 0;
      for (int i = 0; i < 4; i++) e.off[i] = (int16_t) (p.offset[i] * (1 << log2_offset_scale));
    } else if (p.mode == 2) {
      const int left = p.type == 0, s = left ? a - 1 : a - cw;
      if ((p.type != 0 && p.type != 1) || (left ? a % cw == 0 : a < cw) || tile[(size_t) s] != tile[(size_t) a])
        return fail(VVCX_ERR_ARG, "SAO parameters of frame %d CTU %d component %d: no %s merge candidate in the tile", f, a, c, left ? "left" : "above");
      e = tab[((size_t) f * nctu + s) * 3 + c];
    } else return fail(VVCX_ERR_ARG, "SAO mode %d", p.mode);
  }
  return VVCX_OK;
}
// the filter on `pc` with the resolved parameters `table`: the pictures copied into tmp (pc.n pictures of pc.samples()), then filtered from the copy
static void sao_filter(const Pics &pc, const VxSaoEntry *table, const uint8_t *tile_of_ctu, void *tmp, int lf_across_tiles, hipStream_t stream)
{
  VxSaoParams p; memset(&p, 0, sizeof p);
  p.frames = pc.frames; p.table = table; p.tile_of_ctu = tile_of_ctu; p.tmp = tmp; p.tmp_frame = pc.samples(); p.tmp_comp[0] = 0; p.tmp_comp[1] = pc.ny(); p.tmp_comp[2] = pc.ny() + (pc.ny() >> 2);
  p.pic_w = pc.w; p.pic_h = pc.h; p.ctus_w = pc.ctus_w(); p.ctus_h = pc.ctus_h(); p.bit_depth = pc.bit_depth; p.chroma = pc.chroma; p.lf_across_tiles = lf_across_tiles != 0;
  const dim3 grid((unsigned) ((p.pic_w + 1023) / 1024), (unsigned) p.pic_h, (unsigned) (3 * pc.n));      // the filter: four samples per lane
  const dim3 gridC((unsigned) ((p.pic_w + 1023) / 1024), (unsigned) ((p.pic_h + 3) / 4), (unsigned) (3 * pc.n));      // the copy: strips of 4 rows x 1024 samples
  if (pc.bps == 1) { hipLaunchKernelGGL(vvcx_sao_copy_kernel_u8, gridC, dim3(256), 0, stream, p); hipLaunchKernelGGL(vvcx_sao_kernel_u8, grid, dim3(256), 0, stream, p); }
  else { hipLaunchKernelGGL(vvcx_sao_copy_kernel_u16, gridC, dim3(256), 0, stream, p); hipLaunchKernelGGL(vvcx_sao_kernel_u16, grid, dim3(256), 0, stream, p); }
}
extern "C" int vvcx_sao_bound_frames(vvcx_handle *h, const vvcx_sao_param *prm, int lf_across_tiles, int log2_offset_scale, void *hip_stream)
{
  NOT_PENDING(h);
  if (const int rc = bound_entry(h, prm != nullptr, ENDS_ALF | ENDS_SAO, "SAO")) return rc;
  if (log2_offset_scale < 0 || log2_offset_scale > 4) return fail(VVCX_ERR_ARG, "log2 offset scale outside 0..4");
  const Pics pc = bound_pics(h);
  const std::vector<uint8_t> tile = tile_of_ctu_table(pc.ctus_w(), pc.ctus_h(), h->cfg.tile_cols, h->cfg.tile_rows);
  std::vector<VxSaoEntry> tab;
  if (const int rc = sao_resolve(prm, pc.n, pc.ctus_w(), pc.ctus_h(), tile, log2_offset_scale, tab)) return rc;
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  HIPCHK(h->sao_tmp_d.reserve(pc.n * pc.samples() * pc.bps)); HIPCHK(h->sao_tab_d.reserve(tab.size())); HIPCHK(h->sao_tile_d.reserve(tile.size()));
  HIPCHK(hipMemcpyAsync(h->sao_tab_d.p, tab.data(), tab.size() * sizeof(VxSaoEntry), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(h->sao_tile_d.p, tile.data(), tile.size(), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(h->ev0, stream));
  sao_filter(pc, h->sao_tab_d.p, h->sao_tile_d.p, h->sao_tmp_d.p, lf_across_tiles, stream);
  HIPCHK(timed_end(h, stream));
  HIPCHK(timed_wait(h, stream, &h->last_sao_ms));             // (the host tables above must outlive their copies)
  return VVCX_OK;
}
// the same kernels on one picture in host memory (uint16 planes, stride = plane width; filtered in place): the leaf entry the filter is pinned through
extern "C" int vvcx_sao_picture(int pic_w, int pic_h, int bit_depth, int tile_cols, int tile_rows, const vvcx_sao_param *prm, int lf_across_tiles, int log2_offset_scale,
                                uint16_t *y, uint16_t *cb, uint16_t *cr, int device)
{
  if (!prm || !y || !cb || !cr) return fail(VVCX_ERR_ARG, "null argument");
  if (!picture_ok(pic_w, pic_h, bit_depth) || !tiles_ok(pic_w, pic_h, tile_cols, tile_rows) || log2_offset_scale < 0 || log2_offset_scale > 4)
    return fail(VVCX_ERR_ARG, "vvcx_sao_picture: picture size / bit depth / tiles / offset scale");
  const int cw = (pic_w + 127) / 128, chh = (pic_h + 127) / 128;
  const std::vector<uint8_t> tile = tile_of_ctu_table(cw, chh, tile_cols, tile_rows);
  std::vector<VxSaoEntry> tab;
  if (const int rc = sao_resolve(prm, 1, cw, chh, tile, log2_offset_scale, tab)) return rc;
  ON_DEVICE(device);
  DevPicture pic; DevBuf<uint16_t> tmp_d; DevBuf<VxSaoEntry> tab_d; DevBuf<uint8_t> tile_d;
  const uint16_t *const rec[3] = { y, cb, cr };
  if (const int rc = pic.upload(pic_w, pic_h, rec)) return rc;
  const Pics pc = pic.pics(bit_depth);
  HIPCHK(tmp_d.alloc(pc.samples())); HIPCHK(tab_d.alloc(tab.size())); HIPCHK(tile_d.alloc(tile.size()));
  HIPCHK(hipMemcpy(tab_d.p, tab.data(), tab.size() * sizeof(VxSaoEntry), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(tile_d.p, tile.data(), tile.size(), hipMemcpyHostToDevice));
  sao_filter(pc, tab_d.p, tile_d.p, tmp_d.p, lf_across_tiles, 0);
  return pic.download(y, cb, cr);
}
extern "C" float vvcx_last_sao_ms(const vvcx_handle *h) { return h ? h->last_sao_ms : 0.f; }

// ≙ EncSampleAdaptiveOffset::getStatistics (EL/EncSampleAdaptiveOffset.cpp:284-353, SAOLcuBoundary 0) on the bound, deblocked pictures: the statistics the reference's
// decideBlkParams works from, in host memory as [frame][ctu][component][type 0..4][count | diff][32] int64 (≙ SAOStatData per CTU, component and type)
static size_t sao_stat_size(const Pics &pc) { return (size_t) pc.n * pc.nctu() * 3 * 5 * 64; }
// the statistics kernel on `pc` into stat_d, cleared first; ev0 / ev1 (optional) around the kernel
static int sao_stats_launch(const Pics &pc, const uint8_t *tile_d, long long *stat_d, int lf_across_tiles, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1)
{
  HIPCHK(hipMemsetAsync(stat_d, 0, sao_stat_size(pc) * sizeof(long long), stream));
  VxSaoStatParams sp; memset(&sp, 0, sizeof sp);
  sp.frames = pc.frames; sp.tile_of_ctu = tile_d; sp.out = stat_d;
  sp.pic_w = pc.w; sp.pic_h = pc.h; sp.ctus_w = pc.ctus_w(); sp.ctus_h = pc.ctus_h(); sp.bit_depth = pc.bit_depth; sp.chroma = pc.chroma; sp.lf_across_tiles = lf_across_tiles != 0;
  if (ev0) HIPCHK(hipEventRecord(ev0, stream));
  const dim3 grid((unsigned) pc.nctu(), 3u, (unsigned) pc.n);
  if (pc.bps == 1) hipLaunchKernelGGL(vvcx_sao_stats_kernel_u8, grid, dim3(256), 0, stream, sp);
  else hipLaunchKernelGGL(vvcx_sao_stats_kernel_u16, grid, dim3(256), 0, stream, sp);
  HIPCHK(hipGetLastError());
  if (ev1) HIPCHK(hipEventRecord(ev1, stream));
  return VVCX_OK;
}
extern "C" int vvcx_sao_statistics_bound_frames(vvcx_handle *h, int lf_across_tiles, int64_t *stats, void *hip_stream)
{
  NOT_PENDING(h);
  if (const int rc = bound_entry(h, stats != nullptr, ENDS_SAO, "the SAO statistics", "SAO statistics")) return rc;      // sao_stat_d / sao_tile_d are reused: ENDS_SAO
  const Pics pc = bound_pics(h);
  const std::vector<uint8_t> tile = tile_of_ctu_table(pc.ctus_w(), pc.ctus_h(), h->cfg.tile_cols, h->cfg.tile_rows);
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  HIPCHK(h->sao_stat_d.reserve(sao_stat_size(pc))); HIPCHK(h->sao_tile_d.reserve(tile.size()));
  HIPCHK(hipMemcpyAsync(h->sao_tile_d.p, tile.data(), tile.size(), hipMemcpyHostToDevice, stream));
  if (const int rc = sao_stats_launch(pc, h->sao_tile_d.p, h->sao_stat_d.p, lf_across_tiles, stream, h->ev0, h->ev1)) return rc;
  HIPCHK(hipMemcpyAsync(stats, h->sao_stat_d.p, sao_stat_size(pc) * sizeof(long long), hipMemcpyDeviceToHost, stream));
  HIPCHK(timed_wait(h, stream, &h->last_sao_stats_ms));       // (the host tile table above must outlive its copy)
  return VVCX_OK;
}
extern "C" float vvcx_last_sao_stats_ms(const vvcx_handle *h) { return h ? h->last_sao_stats_ms : 0.f; }

// ---- the same decision on the device (vvcx_sao_decide.hip), from statistics that stay in device memory: the candidate kernel prices every (CTU, component, type), the
// chain kernel walks the CTUs of each picture with the two context models.  What it leaves: the resolved filter table (exactly what sao_resolve builds from the coded
// parameters) and the coded parameters, both in device memory; 21 bytes per CTU cross to the host when the caller asks for them.
// buffers of a decision over the pictures `pc`: every allocation of the call, in front of its first launch
static int sao_decide_reserve(const Pics &pc, SaoWork &w, DevBuf<long long> &stat_d, DevBuf<VxSaoEntry> &tab_d, DevBuf<uint8_t> &tile_d)
{
  const size_t n = (size_t) pc.n * pc.nctu();
  HIPCHK(stat_d.reserve(sao_stat_size(pc))); HIPCHK(tab_d.reserve(n * 3)); HIPCHK(tile_d.reserve((size_t) pc.nctu()));
  HIPCHK(w.cand.reserve(n * 15)); HIPCHK(w.syn.reserve(n * 3));
  bool grew = false;
  HIPCHK(w.frac.reserve(512, &grew));
  if (grew) HIPCHK(hipMemcpy(w.frac.p, VX_BIN_FRAC_BITS, 512 * sizeof(uint32_t), hipMemcpyHostToDevice));
  return VVCX_OK;
}
// the two decision kernels on the statistics of `pc` in stat_d (sao_stats_launch): the resolved table into tab_d, the coded parameters into w.syn
static int sao_decide_launch(const Pics &pc, SaoWork &w, const long long *stat_d, VxSaoEntry *tab_d, const uint8_t *tile_d, int slice_qp, const double *lambda, int log2_offset_scale,
                             hipStream_t stream)
{
  VxSaoDecideParams p; memset(&p, 0, sizeof p);
  p.stats = stat_d; p.cands = w.cand.p; p.tile_of_ctu = tile_d; p.frac_bits = w.frac.p; p.table = tab_d; p.syn = w.syn.p;
  for (int k = 0; k < 3; k++) p.lambda[k] = lambda[k];
  p.ctus_w = pc.ctus_w(); p.ctus_h = pc.ctus_h(); p.bit_depth = pc.bit_depth; p.step = log2_offset_scale;
  SaoRate rate; rate.init(slice_qp); rate.export_models(p);
  hipLaunchKernelGGL(vvcx_sao_cand_kernel, dim3((unsigned) pc.nctu(), (unsigned) pc.n), dim3(192), 0, stream, p);
  hipLaunchKernelGGL(vvcx_sao_chain_kernel, dim3((unsigned) pc.n), dim3(64), 0, stream, p);
  HIPCHK(hipGetLastError());
  return VVCX_OK;
}
static_assert(sizeof(VxSaoSyn) == sizeof(vvcx_sao_param), "device copy of the C-ABI record");
extern "C" int vvcx_sao_decide_resident(vvcx_handle *h, int lf_across_tiles, const double lambda[3], int log2_offset_scale, vvcx_sao_param *prm, void *hip_stream)
{
  NOT_PENDING(h);
  if (const int rc = bound_entry(h, lambda != nullptr, ENDS_SAO, "the SAO decision")) return rc;
  if (log2_offset_scale < 0 || log2_offset_scale > 4 || !(lambda[0] > 0) || !(lambda[1] > 0) || !(lambda[2] > 0)) return fail(VVCX_ERR_ARG, "vvcx_sao_decide_resident: offset scale / lambdas");
  Pics pc = bound_pics(h);
  if (pc.ctus_w() > VXD_SAO_MAX_CTUS_W || h->ntiles > 255) return fail(VVCX_ERR_UNSUPPORTED, "vvcx_sao_decide_resident: %d CTU columns / %d tiles", pc.ctus_w(), h->ntiles);
  if (h->lmcs_on) pc.frames = h->frames_org_d.p;      // the search's records carry the forward-mapped luma: the statistics read the records with the caller's own plane
  const std::vector<uint8_t> tile = tile_of_ctu_table(pc.ctus_w(), pc.ctus_h(), h->cfg.tile_cols, h->cfg.tile_rows);
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  if (const int rc = sao_decide_reserve(pc, h->sao_work, h->sao_stat_d, h->sao_tab_d, h->sao_tile_d)) return rc;
  HIPCHK(hipMemcpyAsync(h->sao_tile_d.p, tile.data(), tile.size(), hipMemcpyHostToDevice, stream));
  if (const int rc = sao_stats_launch(pc, h->sao_tile_d.p, h->sao_stat_d.p, lf_across_tiles, stream, h->ev0, h->ev1)) return rc;
  if (const int rc = sao_decide_launch(pc, h->sao_work, h->sao_stat_d.p, h->sao_tab_d.p, h->sao_tile_d.p, h->sl.qp, lambda, log2_offset_scale, stream)) return rc;
  HIPCHK(hipEventRecord(h->ev2, stream));
  if (prm) HIPCHK(hipMemcpyAsync(prm, h->sao_work.syn.p, (size_t) pc.n * pc.nctu() * 3 * sizeof(VxSaoSyn), hipMemcpyDeviceToHost, stream));
  HIPCHK(timed_wait(h, stream, &h->last_sao_stats_ms));       // (the host tile table above must outlive its copy)
  HIPCHK(hipEventElapsedTime(&h->last_sao_decide_ms, h->ev1, h->ev2));
  h->sao_res_valid = true; h->sao_res_lf = lf_across_tiles != 0;
  return VVCX_OK;
}
extern "C" float vvcx_last_sao_decide_ms(const vvcx_handle *h) { return h ? h->last_sao_decide_ms : 0.f; }
// the filter of vvcx_sao_bound_frames with the table the decision left in sao_tab_d.  Its opening is its own: whether a decision is resident is read before the call
// ends it, and the decision has already seen the pictures coded and, on an LMCS slice, mapped back
extern "C" int vvcx_sao_bound_frames_resident(vvcx_handle *h, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  const bool valid = h->sao_res_valid;
  h->alf_res_valid = h->sao_res_valid = false;      // the pictures change: a second pass would filter filtered samples
  if (!h->n_frames || !h->have_slice) return fail(VVCX_ERR_STATE, "no bound frames / slice");
  if (!valid) return fail(VVCX_ERR_STATE, "no resident SAO decision (vvcx_sao_decide_resident), or a call has touched the bound pictures since");
  const Pics pc = bound_pics(h);
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  HIPCHK(h->sao_tmp_d.reserve(pc.n * pc.samples() * pc.bps));
  HIPCHK(hipEventRecord(h->ev0, stream));
  sao_filter(pc, h->sao_tab_d.p, h->sao_tile_d.p, h->sao_tmp_d.p, h->sao_res_lf, stream);
  HIPCHK(timed_end(h, stream));
  HIPCHK(timed_wait(h, stream, &h->last_sao_ms));
  return VVCX_OK;
}
// the decision kernels on one picture in host memory (uint16 planes, stride = plane width): the leaf entry the decision is pinned through
extern "C" int vvcx_sao_decide_picture(int pic_w, int pic_h, int bit_depth, int tile_cols, int tile_rows, int slice_qp, const double lambda[3], int log2_offset_scale,
                                       int lf_across_tiles, const uint16_t *const org[3], const uint16_t *const rec[3], vvcx_sao_param *prm, int device)
{
  if (!lambda || !org || !rec || !prm) return fail(VVCX_ERR_ARG, "null argument");
  for (int c = 0; c < 3; c++) if (!org[c] || !rec[c]) return fail(VVCX_ERR_ARG, "null plane");
  if (!picture_ok(pic_w, pic_h, bit_depth) || !tiles_ok(pic_w, pic_h, tile_cols, tile_rows) || log2_offset_scale < 0 || log2_offset_scale > 4 ||
      !(lambda[0] > 0) || !(lambda[1] > 0) || !(lambda[2] > 0))
    return fail(VVCX_ERR_ARG, "vvcx_sao_decide_picture: picture size / bit depth / tiles / offset scale / lambdas");
  const std::vector<uint8_t> tile = tile_of_ctu_table((pic_w + 127) / 128, (pic_h + 127) / 128, tile_cols, tile_rows);
  ON_DEVICE(device);
  DevPicture pic; SaoWork w; DevBuf<long long> stat_d; DevBuf<VxSaoEntry> tab_d; DevBuf<uint8_t> tile_d;
  if (const int rc = pic.upload(pic_w, pic_h, rec, org)) return rc;
  const Pics pc = pic.pics(bit_depth);
  if (const int rc = sao_decide_reserve(pc, w, stat_d, tab_d, tile_d)) return rc;
  HIPCHK(hipMemcpy(tile_d.p, tile.data(), tile.size(), hipMemcpyHostToDevice));
  if (const int rc = sao_stats_launch(pc, tile_d.p, stat_d.p, lf_across_tiles, 0, nullptr, nullptr)) return rc;
  if (const int rc = sao_decide_launch(pc, w, stat_d.p, tab_d.p, tile_d.p, slice_qp, lambda, log2_offset_scale, 0)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(prm, w.syn.p, (size_t) pc.nctu() * 3 * sizeof(VxSaoSyn), hipMemcpyDeviceToHost));
  return VVCX_OK;
}

// ---- adaptive loop filter with the caller's parameter sets (vvcx_alf_derive.hip builds the per-class tables of every frame's slice; the kernels of vvcx_alf.hip
// classify and filter).  The filter on `pc`: the pictures copied into tmp (pc.n pictures of pc.samples()), then filtered from the copy; classes: optional, see VxAlfParams
static void alf_filter(const Pics &pc, const VxAlfFrame *tabs, const VxAlfCtu *ctus, void *tmp, uint8_t *classes, hipStream_t stream)
{
  VxAlfParams p; memset(&p, 0, sizeof p);
  p.frames = pc.frames; p.tabs = tabs; p.ctus = ctus; p.tmp = tmp; p.tmp_frame = pc.samples(); p.tmp_comp[0] = 0; p.tmp_comp[1] = pc.ny(); p.tmp_comp[2] = pc.ny() + (pc.ny() >> 2);
  p.classes = classes; p.pic_w = pc.w; p.pic_h = pc.h; p.ctus_w = pc.ctus_w(); p.ctus_h = pc.ctus_h(); p.bit_depth = pc.bit_depth; p.chroma = pc.chroma;
  const dim3 gridC((unsigned) ((p.pic_w + 1023) / 1024), (unsigned) ((p.pic_h + 3) / 4), (unsigned) (3 * pc.n));      // the copy: strips of 4 rows x 1024 samples
  const dim3 gridF((unsigned) ((p.pic_w + 63) / 64), (unsigned) ((p.pic_h + 15) / 16), (unsigned) (3 * pc.n));
  if (pc.bps == 1) { hipLaunchKernelGGL(vvcx_alf_copy_kernel_u8, gridC, dim3(256), 0, stream, p); hipLaunchKernelGGL(vvcx_alf_kernel_u8, gridF, dim3(256), 0, stream, p); }
  else { hipLaunchKernelGGL(vvcx_alf_copy_kernel_u16, gridC, dim3(256), 0, stream, p); hipLaunchKernelGGL(vvcx_alf_kernel_u16, gridF, dim3(256), 0, stream, p); }
}
extern "C" int vvcx_alf_bound_frames(vvcx_handle *h, const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, void *hip_stream)
{
  NOT_PENDING(h);
  if (const int rc = bound_entry(h, slices && ctus && (n_aps <= 0 || aps), ENDS_ALF | ENDS_SAO, "ALF")) return rc;
  const Pics pc = bound_pics(h);
  std::vector<VxAlfFrame> tabs; std::vector<VxAlfCtu> cts;
  if (const int rc = alf_build(aps, n_aps, slices, ctus, pc.n, pc.nctu(), pc.bit_depth, pc.chroma, tabs)) return rc;
  alf_ctus(slices, ctus, pc.n, pc.nctu(), pc.chroma, cts);
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  HIPCHK(h->sao_tmp_d.reserve(pc.n * pc.samples() * pc.bps));
  HIPCHK(h->alf_tab_d.reserve(tabs.size())); HIPCHK(h->alf_ctu_d.reserve(cts.size()));
  HIPCHK(hipMemcpyAsync(h->alf_tab_d.p, tabs.data(), tabs.size() * sizeof(VxAlfFrame), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(h->alf_ctu_d.p, cts.data(), cts.size() * sizeof(VxAlfCtu), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(h->ev0, stream));
  alf_filter(pc, h->alf_tab_d.p, h->alf_ctu_d.p, h->sao_tmp_d.p, nullptr, stream);      // (the picture copy is the SAO one)
  HIPCHK(timed_end(h, stream));
  HIPCHK(timed_wait(h, stream, &h->last_alf_ms));             // (the host tables above must outlive their copies)
  return VVCX_OK;
}
// the same kernels on one picture in host memory (uint16 planes, stride = plane width; filtered in place): the leaf entry the filter is pinned through
extern "C" int vvcx_alf_picture(int pic_w, int pic_h, int bit_depth, const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slice, const vvcx_alf_ctu *ctus,
                                uint16_t *y, uint16_t *cb, uint16_t *cr, uint8_t *classes, int device)
{
  if (!slice || !ctus || !y || !cb || !cr || (n_aps > 0 && !aps)) return fail(VVCX_ERR_ARG, "null argument");
  if (!picture_ok(pic_w, pic_h, bit_depth)) return fail(VVCX_ERR_ARG, "vvcx_alf_picture: picture size / bit depth");
  const int nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128);
  std::vector<VxAlfFrame> tabs; std::vector<VxAlfCtu> cts;
  if (const int rc = alf_build(aps, n_aps, slice, ctus, 1, nctu, bit_depth, 1, tabs)) return rc;
  alf_ctus(slice, ctus, 1, nctu, 1, cts);
  ON_DEVICE(device);
  DevPicture pic; DevBuf<uint16_t> tmp_d; DevBuf<VxAlfFrame> tab_d; DevBuf<VxAlfCtu> ctu_d; DevBuf<uint8_t> cls_d;
  const uint16_t *const rec[3] = { y, cb, cr };
  if (const int rc = pic.upload(pic_w, pic_h, rec)) return rc;
  const Pics pc = pic.pics(bit_depth);
  const size_t ncls = (size_t) (pic_w >> 2) * (pic_h >> 2);
  HIPCHK(tmp_d.alloc(pc.samples())); HIPCHK(tab_d.alloc(1)); HIPCHK(ctu_d.alloc(cts.size())); HIPCHK(cls_d.alloc(ncls));
  HIPCHK(hipMemcpy(tab_d.p, tabs.data(), sizeof(VxAlfFrame), hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(ctu_d.p, cts.data(), cts.size() * sizeof(VxAlfCtu), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(cls_d.p, 255, ncls));
  alf_filter(pc, tab_d.p, ctu_d.p, tmp_d.p, cls_d.p, 0);
  if (const int rc = pic.download(y, cb, cr)) return rc;
  if (classes) HIPCHK(hipMemcpy(classes, cls_d.p, ncls, hipMemcpyDeviceToHost));
  return VVCX_OK;
}
extern "C" float vvcx_last_alf_ms(const vvcx_handle *h) { return h ? h->last_alf_ms : 0.f; }

// ---- the encoder side of ALF.  The statistics (≙ EncAdaptiveLoopFilter::deriveStatsForFiltering, EL/EncAdaptiveLoopFilter.cpp:2650-2745 -> getBlkStats / calcCovariance)
// are gathered on the device (vvcx_alf_stats.hip): per (CTU, class) E | y | pixAcc as int64, nc = 13 luma / 7 chroma coefficients, nb clipping bins.

// the statistics kernel on n pictures of `pc` from frame_first on, nb clipping bins, into luma_d / chroma_d (NULL: luma only)
static void alf_stats_launch(const Pics &pc, int frame_first, int n, int nb, long long *luma_d, long long *chroma_d, hipStream_t stream)
{
  VxAlfStatParams p; memset(&p, 0, sizeof p);
  p.frames = pc.frames; p.luma = luma_d; p.chroma = chroma_d; p.frame_first = frame_first;
  p.pic_w = pc.w; p.pic_h = pc.h; p.ctus_w = pc.ctus_w(); p.ctus_h = pc.ctus_h(); p.bit_depth = pc.bit_depth;
  for (int b = 0; b < 4; b++) { p.clip[0][b] = alf_clip_value(0, p.bit_depth, b); p.clip[1][b] = alf_clip_value(1, p.bit_depth, b); }
  const dim3 grid((unsigned) pc.nctu(), p.chroma ? 3u : 1u, (unsigned) n);      // one workgroup owns one (CTU, component, frame)
  if (pc.bps == 1) { if (nb == 1) hipLaunchKernelGGL(vvcx_alf_stats_b1_kernel_u8, grid, dim3(256), 0, stream, p); else hipLaunchKernelGGL(vvcx_alf_stats_b4_kernel_u8, grid, dim3(256), 0, stream, p); }
  else { if (nb == 1) hipLaunchKernelGGL(vvcx_alf_stats_b1_kernel_u16, grid, dim3(256), 0, stream, p); else hipLaunchKernelGGL(vvcx_alf_stats_b4_kernel_u16, grid, dim3(256), 0, stream, p); }
}
// one picture in host memory -> its statistics in luma_d / chroma_d (the caller's device is current); the checks of the host-plane entries
static int alf_stats_of_planes(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], bool chroma,
                               DevBuf<long long> &luma_d, DevBuf<long long> &chroma_d)
{
  DevPicture pic;
  if (const int rc = pic.upload(pic_w, pic_h, rec, org)) return rc;
  const Pics pc = pic.pics(bit_depth);
  HIPCHK(luma_d.alloc((size_t) pc.nctu() * 25 * alf_stat_size(n_bins, 13)));
  if (chroma) HIPCHK(chroma_d.alloc((size_t) pc.nctu() * 2 * alf_stat_size(n_bins, 7)));
  alf_stats_launch(pc, 0, 1, n_bins, luma_d.p, chroma ? chroma_d.p : nullptr, 0);
  HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
  return VVCX_OK;
}
static int alf_picture_args(const char *who, int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3])
{
  if (!org || !rec) return fail(VVCX_ERR_ARG, "null argument");
  for (int c = 0; c < 3; c++) if (!org[c] || !rec[c]) return fail(VVCX_ERR_ARG, "null plane");
  if (!picture_ok(pic_w, pic_h, bit_depth)) return fail(VVCX_ERR_ARG, "%s: picture size / bit depth", who);
  if (n_bins != 1 && n_bins != 4) return fail(VVCX_ERR_ARG, "%s: %d clipping bins (1 or 4)", who, n_bins);
  return VVCX_OK;
}
extern "C" int vvcx_alf_statistics_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3],
                                           int64_t *luma, int64_t *chroma, int device)
{
  if (!luma) return fail(VVCX_ERR_ARG, "null argument");
  if (const int rc = alf_picture_args("vvcx_alf_statistics_picture", pic_w, pic_h, bit_depth, n_bins, org, rec)) return rc;
  const int nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128);
  const size_t nl = (size_t) nctu * 25 * alf_stat_size(n_bins, 13), nch = (size_t) nctu * 2 * alf_stat_size(n_bins, 7);
  ON_DEVICE(device);
  DevBuf<long long> luma_d, chroma_d;
  if (const int rc = alf_stats_of_planes(pic_w, pic_h, bit_depth, n_bins, org, rec, chroma != nullptr, luma_d, chroma_d)) return rc;
  HIPCHK(hipMemcpy(luma, luma_d.p, nl * sizeof(long long), hipMemcpyDeviceToHost));
  if (chroma) HIPCHK(hipMemcpy(chroma, chroma_d.p, nch * sizeof(long long), hipMemcpyDeviceToHost));
  return VVCX_OK;
}
// the checks and the launch of the two bound forms: the statistics of frames frame_first .. in alf_stat_*_d when `stream` gets there (ev0 .. ev1 around the kernel).
// luma: the entry's pointer argument is there; the statistics buffers are reused, hence ENDS_ALF
static int alf_stats_bound(vvcx_handle *h, const char *who, bool luma, int frame_first, int n, int n_bins, bool wantC, hipStream_t stream)
{
  if (const int rc = bound_entry(h, luma, ENDS_ALF, "the ALF statistics", "ALF statistics")) return rc;
  if (n_bins != 1 && n_bins != 4) return fail(VVCX_ERR_ARG, "%s: %d clipping bins (1 or 4)", who, n_bins);
  if (frame_first < 0 || n < 1 || frame_first > h->n_frames - n) return fail(VVCX_ERR_ARG, "%s: frames %d .. %d of %d", who, frame_first, frame_first + n - 1, h->n_frames);
  const Pics pc = bound_pics(h);
  HIPCHK(h->alf_stat_luma_d.reserve((size_t) n * pc.nctu() * 25 * alf_stat_size(n_bins, 13)));
  if (wantC) HIPCHK(h->alf_stat_chroma_d.reserve((size_t) n * pc.nctu() * 2 * alf_stat_size(n_bins, 7)));
  HIPCHK(hipEventRecord(h->ev0, stream));
  alf_stats_launch(pc, frame_first, n, n_bins, h->alf_stat_luma_d.p, wantC ? h->alf_stat_chroma_d.p : nullptr, stream);
  HIPCHK(timed_end(h, stream));
  return VVCX_OK;
}
extern "C" int vvcx_alf_statistics_bound_frames(vvcx_handle *h, int frame_first, int n, int n_bins, int64_t *luma, int64_t *chroma, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null argument");
  const bool wantC = chroma && h->cfg.chroma;
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  if (const int rc = alf_stats_bound(h, "vvcx_alf_statistics_bound_frames", luma != nullptr, frame_first, n, n_bins, wantC, stream)) return rc;
  const int nctu = h->ctus_w * h->ctus_h;
  const size_t nl = (size_t) n * nctu * 25 * alf_stat_size(n_bins, 13), nch = (size_t) n * nctu * 2 * alf_stat_size(n_bins, 7);
  HIPCHK(hipMemcpyAsync(luma, h->alf_stat_luma_d.p, nl * sizeof(long long), hipMemcpyDeviceToHost, stream));
  if (wantC) HIPCHK(hipMemcpyAsync(chroma, h->alf_stat_chroma_d.p, nch * sizeof(long long), hipMemcpyDeviceToHost, stream));
  HIPCHK(timed_wait(h, stream, &h->last_alf_stats_ms));
  if (chroma && !wantC) memset(chroma, 0, nch * sizeof(int64_t));      // a handle without chroma
  return VVCX_OK;
}
// the same without the copy: the statistics stay in device memory for vvcx_alf_frame_statistics / _candidate_errors / _decide_resident until a call touches the pictures
extern "C" int vvcx_alf_statistics_resident(vvcx_handle *h, int frame_first, int n, int n_bins, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  ON_DEVICE(h->cfg.device);
  hipStream_t stream = (hipStream_t) hip_stream;
  if (const int rc = alf_stats_bound(h, "vvcx_alf_statistics_resident", true, frame_first, n, n_bins, h->cfg.chroma != 0, stream)) return rc;
  HIPCHK(timed_wait(h, stream, &h->last_alf_stats_ms));
  h->alf_res_valid = true; h->alf_res_chroma = h->cfg.chroma != 0; h->alf_res_first = frame_first; h->alf_res_n = n; h->alf_res_bins = n_bins;
  return VVCX_OK;
}
extern "C" float vvcx_last_alf_stats_ms(const vvcx_handle *h) { return h ? h->last_alf_stats_ms : 0.f; }

// ---- the decision from statistics that stay in device memory (vvcx_alf_eval.hip): masked frame sums and per-CTU candidate errors are the only things that cross to the
// host; with them the code of vvcx_alf_derive.hip (AlfCov, alf_solve, alf_quant, alf_derive_luma) sees the inputs it would have built from downloaded statistics - the
// sums are exact integers, and doubles of them are exact below 2^53.  include/vvcx.h says what the flags add and how the bits are counted.
static_assert(sizeof(VxAlfLumaCand) == sizeof(vvcx_alf_luma_cand) && sizeof(VxAlfChromaCand) == sizeof(vvcx_alf_chroma_cand), "device copies of the C-ABI records");
int alf_sums(AlfRes &r, const uint8_t *ctu_on, int64_t *luma, int64_t *chroma)
{
  const size_t szl = alf_stat_size(r.nb, 13), szc = alf_stat_size(r.nb, 7), nl = (size_t) r.n * 25 * szl, nch = (size_t) r.n * 2 * szc;
  const bool wantC = chroma && r.chroma;
  AlfWork &w = *r.w;
  HIPCHK(w.sum_l.reserve(nl));
  if (wantC) HIPCHK(w.sum_c.reserve(nch));
  if (ctu_on) {
    HIPCHK(w.mask.reserve((size_t) r.n * r.nctu * 3));
    HIPCHK(hipMemcpyAsync(w.mask.p, ctu_on, (size_t) r.n * r.nctu * 3, hipMemcpyHostToDevice, r.stream));
  }
  VxAlfSumParams p; memset(&p, 0, sizeof p);
  p.luma = r.luma; p.chroma = wantC ? r.chroma : nullptr; p.ctu_on = ctu_on ? w.mask.p : nullptr; p.luma_out = w.sum_l.p; p.chroma_out = wantC ? w.sum_c.p : nullptr;
  p.nctu = r.nctu; p.size_l = szl; p.size_c = szc;
  const dim3 grid((unsigned) ((25 * szl + 255) / 256), wantC ? 2u : 1u, (unsigned) r.n);      // one thread owns one element of the output (25 size_l >= 2 size_c)
  if (r.ev0) HIPCHK(hipEventRecord(r.ev0, r.stream));
  hipLaunchKernelGGL(vvcx_alf_sum_kernel, grid, dim3(256), 0, r.stream, p);
  HIPCHK(hipGetLastError());
  if (r.ev0) HIPCHK(hipEventRecord(r.ev1, r.stream));
  HIPCHK(hipMemcpyAsync(luma, w.sum_l.p, nl * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
  if (wantC) HIPCHK(hipMemcpyAsync(chroma, w.sum_c.p, nch * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
  HIPCHK(hipStreamSynchronize(r.stream));
  if (r.ev0) HIPCHK(hipEventElapsedTime(&r.sum_ms, r.ev0, r.ev1));
  r.calls++;
  if (chroma && !wantC) memset(chroma, 0, nch * sizeof(int64_t));
  return VVCX_OK;
}

int alf_errors(AlfRes &r, int fixed_sets, const vvcx_alf_luma_cand *lc, int n_luma, const vvcx_alf_chroma_cand *cc, int n_chroma, int64_t *luma_err, int64_t *chroma_err)
{
  if (fixed_sets < 0 || fixed_sets > 1 || n_luma < 0 || n_chroma < 0 || 16 * fixed_sets + n_luma > VX_ALF_MAX_CAND || n_chroma > VX_ALF_MAX_CAND)
    return fail(VVCX_ERR_ARG, "ALF candidates: fixed_sets %d, %d luma, %d chroma (at most %d per component, the fixed sets included)", fixed_sets, n_luma, n_chroma, VX_ALF_MAX_CAND);
  const int ncl = 16 * fixed_sets + n_luma;
  if (!ncl && !n_chroma) return fail(VVCX_ERR_ARG, "ALF candidates: none given");
  if ((n_luma && !lc) || (ncl && !luma_err) || (n_chroma && (!cc || !chroma_err))) return fail(VVCX_ERR_ARG, "null argument");
  for (size_t i = 0; i < (size_t) r.n * n_luma; i++) for (int c = 0; c < 25; c++) for (int k = 0; k < 12; k++)
    if (lc[i].coeff[c][k] < -128 || lc[i].coeff[c][k] > 128 || lc[i].clip_idx[c][k] >= r.nb)
      return fail(VVCX_ERR_ARG, "ALF luma candidate %d: coefficient %d / clipping index %d (|q| <= 128, index < %d gathered bins)", (int) i, lc[i].coeff[c][k], lc[i].clip_idx[c][k], r.nb);
  for (size_t i = 0; i < (size_t) r.n * n_chroma; i++) for (int k = 0; k < 6; k++)
    if (cc[i].coeff[k] < -128 || cc[i].coeff[k] > 128 || cc[i].clip_idx[k] >= r.nb)
      return fail(VVCX_ERR_ARG, "ALF chroma candidate %d: coefficient %d / clipping index %d (|q| <= 128, index < %d gathered bins)", (int) i, cc[i].coeff[k], cc[i].clip_idx[k], r.nb);
  const bool wantC = n_chroma && r.chroma;
  const size_t nle = (size_t) r.n * r.nctu * ncl, nce = (size_t) r.n * r.nctu * 2 * n_chroma;
  AlfWork &w = *r.w;
  if (ncl) HIPCHK(w.err_l.reserve(nle));
  if (n_luma) { HIPCHK(w.lc.reserve((size_t) r.n * n_luma)); HIPCHK(hipMemcpyAsync(w.lc.p, lc, (size_t) r.n * n_luma * sizeof *lc, hipMemcpyHostToDevice, r.stream)); }
  if (wantC) { HIPCHK(w.err_c.reserve(nce)); HIPCHK(w.cc.reserve((size_t) r.n * n_chroma)); HIPCHK(hipMemcpyAsync(w.cc.p, cc, (size_t) r.n * n_chroma * sizeof *cc, hipMemcpyHostToDevice, r.stream)); }
  if (ncl || wantC) {
    VxAlfCandParams p; memset(&p, 0, sizeof p);
    p.luma = r.luma; p.chroma = r.chroma; p.luma_cands = w.lc.p; p.chroma_cands = w.cc.p; p.luma_err = w.err_l.p; p.chroma_err = w.err_c.p;
    p.nctu = r.nctu; p.nb = r.nb; p.fixed_sets = fixed_sets; p.n_luma = n_luma; p.n_chroma = wantC ? n_chroma : 0;
    const dim3 grid((unsigned) r.nctu, wantC ? 3u : 1u, (unsigned) r.n);      // one workgroup owns one (CTU, component, frame)
    if (r.ev0) HIPCHK(hipEventRecord(r.ev0, r.stream));
    hipLaunchKernelGGL(vvcx_alf_cand_kernel, grid, dim3(256), 0, r.stream, p);
    HIPCHK(hipGetLastError());
    if (r.ev0) HIPCHK(hipEventRecord(r.ev1, r.stream));
    if (ncl) HIPCHK(hipMemcpyAsync(luma_err, w.err_l.p, nle * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
    if (wantC) HIPCHK(hipMemcpyAsync(chroma_err, w.err_c.p, nce * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
    HIPCHK(hipStreamSynchronize(r.stream));
    if (r.ev0) HIPCHK(hipEventElapsedTime(&r.cand_ms, r.ev0, r.ev1));
    r.calls++;
  }
  if (n_chroma && !wantC) memset(chroma_err, 0, nce * sizeof(int64_t));      // no chroma statistics
  return VVCX_OK;
}

// the chroma blocks of every frame summed per label (vvcx_alf_chroma_label_sum_kernel): Cb and Cr pooled, zeros for a label no block carries
int alf_label_sums(AlfRes &r, const uint8_t *labels, int n_alts, int64_t *sums)
{
  if (!r.chroma) return fail(VVCX_ERR_STATE, "ALF chroma alternatives: the statistics have no chroma");
  if (!labels || !sums) return fail(VVCX_ERR_ARG, "null argument");
  if (n_alts < 1 || n_alts > VX_ALF_MAX_ALTS) return fail(VVCX_ERR_ARG, "ALF chroma alternatives: %d (1..%d)", n_alts, VX_ALF_MAX_ALTS);
  const size_t nlab = (size_t) r.n * r.nctu * 2, szc = alf_stat_size(r.nb, 7), ns = (size_t) r.n * n_alts * szc;
  for (size_t i = 0; i < nlab; i++) if (labels[i] >= n_alts && labels[i] != VX_ALF_LABEL_OFF)
    return fail(VVCX_ERR_ARG, "ALF chroma alternatives: label %d of block %d (0..%d, or 255 = off)", labels[i], (int) i, n_alts - 1);
  AlfWork &w = *r.w;
  HIPCHK(w.lab.reserve(nlab)); HIPCHK(w.lab_sum.reserve(ns));
  HIPCHK(hipMemcpyAsync(w.lab.p, labels, nlab, hipMemcpyHostToDevice, r.stream));
  VxAlfLabelSumParams p; memset(&p, 0, sizeof p);
  p.chroma = r.chroma; p.labels = w.lab.p; p.out = w.lab_sum.p; p.nctu = r.nctu; p.n_alts = n_alts; p.size_c = szc;
  const dim3 grid((unsigned) ((szc + 255) / 256), 1u, (unsigned) r.n);      // one thread owns one element of one frame's sums
  if (r.ev0) HIPCHK(hipEventRecord(r.ev0, r.stream));
  hipLaunchKernelGGL(vvcx_alf_chroma_label_sum_kernel, grid, dim3(256), 0, r.stream, p);
  HIPCHK(hipGetLastError());
  if (r.ev0) HIPCHK(hipEventRecord(r.ev1, r.stream));
  HIPCHK(hipMemcpyAsync(sums, w.lab_sum.p, ns * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
  HIPCHK(hipStreamSynchronize(r.stream));
  if (r.ev0) HIPCHK(hipEventElapsedTime(&r.sum_ms, r.ev0, r.ev1));
  r.calls++;
  return VVCX_OK;
}
// per (frame, CTU, component) the cheapest of off and the frame's alternatives (vvcx_alf_chroma_assign_kernel), then the frames' costs (vvcx_alf_chroma_cost_kernel)
int alf_assign(AlfRes &r, const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], uint8_t *labels, int64_t *err, double *cost)
{
  if (!r.chroma) return fail(VVCX_ERR_STATE, "ALF chroma alternatives: the statistics have no chroma");
  if (!cands || !lambda_c || !labels || !err || !cost) return fail(VVCX_ERR_ARG, "null argument");
  if (n_alts < 1 || n_alts > VX_ALF_MAX_ALTS) return fail(VVCX_ERR_ARG, "ALF chroma alternatives: %d (1..%d)", n_alts, VX_ALF_MAX_ALTS);
  if (!(lambda_c[0] >= 0) || !(lambda_c[1] >= 0)) return fail(VVCX_ERR_ARG, "ALF chroma alternatives: lambdas");
  for (size_t i = 0; i < (size_t) r.n * n_alts; i++) for (int k = 0; k < 6; k++)
    if (cands[i].coeff[k] < -128 || cands[i].coeff[k] > 128 || cands[i].clip_idx[k] >= r.nb)
      return fail(VVCX_ERR_ARG, "ALF chroma candidate %d: coefficient %d / clipping index %d (|q| <= 128, index < %d gathered bins)", (int) i, cands[i].coeff[k], cands[i].clip_idx[k], r.nb);
  const size_t nlab = (size_t) r.n * r.nctu * 2;
  AlfWork &w = *r.w;
  HIPCHK(w.lab.reserve(nlab)); HIPCHK(w.alt_err.reserve(nlab)); HIPCHK(w.alt_term.reserve(nlab)); HIPCHK(w.alt_cost.reserve((size_t) r.n)); HIPCHK(w.cc.reserve((size_t) r.n * n_alts));
  HIPCHK(hipMemcpyAsync(w.cc.p, cands, (size_t) r.n * n_alts * sizeof *cands, hipMemcpyHostToDevice, r.stream));
  VxAlfAssignParams p; memset(&p, 0, sizeof p);
  p.chroma = r.chroma; p.cands = w.cc.p; p.labels = w.lab.p; p.err = w.alt_err.p; p.term = w.alt_term.p; p.cost = w.alt_cost.p;
  p.lambda_c[0] = lambda_c[0]; p.lambda_c[1] = lambda_c[1]; p.nctu = r.nctu; p.nb = r.nb; p.n_alts = n_alts;
  const dim3 grid((unsigned) r.nctu, 2u, (unsigned) r.n);      // one workgroup owns one (CTU, component, frame)
  if (r.ev0) HIPCHK(hipEventRecord(r.ev0, r.stream));
  hipLaunchKernelGGL(vvcx_alf_chroma_assign_kernel, grid, dim3(256), 0, r.stream, p);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(vvcx_alf_chroma_cost_kernel, dim3((unsigned) r.n), dim3(64), 0, r.stream, p);
  HIPCHK(hipGetLastError());
  if (r.ev0) HIPCHK(hipEventRecord(r.ev1, r.stream));
  HIPCHK(hipMemcpyAsync(labels, w.lab.p, nlab, hipMemcpyDeviceToHost, r.stream));
  HIPCHK(hipMemcpyAsync(err, w.alt_err.p, nlab * sizeof(long long), hipMemcpyDeviceToHost, r.stream));
  HIPCHK(hipMemcpyAsync(cost, w.alt_cost.p, (size_t) r.n * sizeof(double), hipMemcpyDeviceToHost, r.stream));
  HIPCHK(hipStreamSynchronize(r.stream));
  if (r.ev0) HIPCHK(hipEventElapsedTime(&r.cand_ms, r.ev0, r.ev1));
  r.calls++;
  return VVCX_OK;
}

static int alf_decide_args(const double lambda[3], int max_luma_filters, int flags, int nb)
{
  if (!lambda || max_luma_filters < 1 || max_luma_filters > 25 || !(lambda[0] >= 0) || !(lambda[1] >= 0) || !(lambda[2] >= 0) || flags < 0 || (flags & 0xff) > 7 || (flags >> 8) > 7)
    return fail(VVCX_ERR_ARG, "ALF decision: filter count / lambdas / flags");
  if ((flags & (VVCX_ALF_NONLINEAR_LUMA | VVCX_ALF_NONLINEAR_CHROMA)) && nb != 4) return fail(VVCX_ERR_ARG, "ALF decision: nonlinear filters need statistics with 4 clipping bins");
  return VVCX_OK;
}
static int alf_resident(vvcx_handle *h, void *hip_stream, AlfRes &r)
{
  if (!h->alf_res_valid) return fail(VVCX_ERR_STATE, "no resident ALF statistics (vvcx_alf_statistics_resident), or a call has touched the bound pictures since");
  r.luma = h->alf_stat_luma_d.p; r.chroma = h->alf_res_chroma ? h->alf_stat_chroma_d.p : nullptr; r.n = h->alf_res_n; r.nctu = h->ctus_w * h->ctus_h; r.nb = h->alf_res_bins;
  r.w = &h->alf_work; r.stream = (hipStream_t) hip_stream; r.ev0 = h->ev0; r.ev1 = h->ev1; r.sum_ms = h->last_alf_sum_ms; r.cand_ms = h->last_alf_cand_ms; r.calls = 0;
  return VVCX_OK;
}

extern "C" int vvcx_alf_frame_statistics(vvcx_handle *h, const uint8_t *ctu_on, int64_t *luma, int64_t *chroma, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h || !luma) return fail(VVCX_ERR_ARG, "null argument");
  AlfRes r;
  if (const int rc = alf_resident(h, hip_stream, r)) return rc;
  ON_DEVICE(h->cfg.device);
  const int rc = alf_sums(r, ctu_on, luma, chroma);
  h->last_alf_sum_ms = r.sum_ms;
  return rc;
}
extern "C" int vvcx_alf_candidate_errors(vvcx_handle *h, int fixed_sets, const vvcx_alf_luma_cand *luma_cands, int n_luma, const vvcx_alf_chroma_cand *chroma_cands, int n_chroma,
                                         int64_t *luma_err, int64_t *chroma_err, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  AlfRes r;
  if (const int rc = alf_resident(h, hip_stream, r)) return rc;
  ON_DEVICE(h->cfg.device);
  const int rc = alf_errors(r, fixed_sets, luma_cands, n_luma, chroma_cands, n_chroma, luma_err, chroma_err);
  h->last_alf_cand_ms = r.cand_ms;
  return rc;
}
extern "C" int vvcx_alf_decide_resident(vvcx_handle *h, const double lambda[3], int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slices, vvcx_alf_ctu *ctus,
                                        void *hip_stream)
{
  NOT_PENDING(h);
  if (!h || !aps || !slices || !ctus) return fail(VVCX_ERR_ARG, "null argument");
  AlfRes r;
  if (const int rc = alf_resident(h, hip_stream, r)) return rc;
  if (const int rc = alf_decide_args(lambda, max_luma_filters, flags, r.nb)) return rc;
  ON_DEVICE(h->cfg.device);
  const int rc = alf_decide_frames(r, r.chroma != nullptr, lambda, max_luma_filters, flags, aps, slices, ctus);
  h->last_alf_sum_ms = r.sum_ms; h->last_alf_cand_ms = r.cand_ms; h->last_alf_calls = r.calls;
  return rc;
}
extern "C" int vvcx_alf_chroma_label_sums(vvcx_handle *h, const uint8_t *labels, int n_alts, int64_t *sums, void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  AlfRes r;
  if (const int rc = alf_resident(h, hip_stream, r)) return rc;
  ON_DEVICE(h->cfg.device);
  const int rc = alf_label_sums(r, labels, n_alts, sums);
  h->last_alf_sum_ms = r.sum_ms;
  return rc;
}
extern "C" int vvcx_alf_chroma_assign(vvcx_handle *h, const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], uint8_t *labels, int64_t *err, double *cost,
                                      void *hip_stream)
{
  NOT_PENDING(h);
  if (!h) return fail(VVCX_ERR_ARG, "null handle");
  AlfRes r;
  if (const int rc = alf_resident(h, hip_stream, r)) return rc;
  ON_DEVICE(h->cfg.device);
  const int rc = alf_assign(r, cands, n_alts, lambda_c, labels, err, cost);
  h->last_alf_cand_ms = r.cand_ms;
  return rc;
}
extern "C" int vvcx_last_alf_device_calls(const vvcx_handle *h) { return h ? h->last_alf_calls : 0; }
extern "C" float vvcx_last_alf_sum_ms(const vvcx_handle *h) { return h ? h->last_alf_sum_ms : 0.f; }
extern "C" float vvcx_last_alf_cand_ms(const vvcx_handle *h) { return h ? h->last_alf_cand_ms : 0.f; }

extern "C" int vvcx_alf_evaluate_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const uint8_t *ctu_on,
                                         int fixed_sets, const vvcx_alf_luma_cand *luma_cands, int n_luma, const vvcx_alf_chroma_cand *chroma_cands, int n_chroma,
                                         int64_t *luma_sum, int64_t *chroma_sum, int64_t *luma_err, int64_t *chroma_err, int device)
{
  if (const int rc = alf_picture_args("vvcx_alf_evaluate_picture", pic_w, pic_h, bit_depth, n_bins, org, rec)) return rc;
  const bool sums = luma_sum != nullptr, errs = luma_err || chroma_err;
  if (!sums && !errs) return fail(VVCX_ERR_ARG, "vvcx_alf_evaluate_picture: no output asked for");
  ON_DEVICE(device);
  DevBuf<long long> luma_d, chroma_d; AlfWork work;
  if (const int rc = alf_stats_of_planes(pic_w, pic_h, bit_depth, n_bins, org, rec, true, luma_d, chroma_d)) return rc;
  AlfRes r; memset(&r, 0, sizeof r);
  r.luma = luma_d.p; r.chroma = chroma_d.p; r.n = 1; r.nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128); r.nb = n_bins; r.w = &work;
  if (sums) if (const int rc = alf_sums(r, ctu_on, luma_sum, chroma_sum)) return rc;
  if (errs) if (const int rc = alf_errors(r, fixed_sets, luma_cands, n_luma, chroma_cands, n_chroma, luma_err, chroma_err)) return rc;
  return VVCX_OK;
}
extern "C" int vvcx_alf_chroma_alts_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const uint8_t *labels_in,
                                            const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], int64_t *sums, uint8_t *labels_out, int64_t *err, double *cost,
                                            int device)
{
  if (const int rc = alf_picture_args("vvcx_alf_chroma_alts_picture", pic_w, pic_h, bit_depth, n_bins, org, rec)) return rc;
  const bool want_sums = sums != nullptr, want_assign = labels_out || err || cost;
  if (!want_sums && !want_assign) return fail(VVCX_ERR_ARG, "vvcx_alf_chroma_alts_picture: no output asked for");
  ON_DEVICE(device);
  DevBuf<long long> luma_d, chroma_d; AlfWork work;
  if (const int rc = alf_stats_of_planes(pic_w, pic_h, bit_depth, n_bins, org, rec, true, luma_d, chroma_d)) return rc;
  AlfRes r; memset(&r, 0, sizeof r);
  r.luma = luma_d.p; r.chroma = chroma_d.p; r.n = 1; r.nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128); r.nb = n_bins; r.w = &work;
  if (want_sums) if (const int rc = alf_label_sums(r, labels_in, n_alts, sums)) return rc;
  if (want_assign) if (const int rc = alf_assign(r, cands, n_alts, lambda_c, labels_out, err, cost)) return rc;
  return VVCX_OK;
}
extern "C" int vvcx_alf_decide_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const double lambda[3],
                                       int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slice, vvcx_alf_ctu *ctus, int device)
{
  if (!aps || !slice || !ctus) return fail(VVCX_ERR_ARG, "null argument");
  if (const int rc = alf_picture_args("vvcx_alf_decide_picture", pic_w, pic_h, bit_depth, n_bins, org, rec)) return rc;
  if (const int rc = alf_decide_args(lambda, max_luma_filters, flags, n_bins)) return rc;
  ON_DEVICE(device);
  DevBuf<long long> luma_d, chroma_d; AlfWork work;
  if (const int rc = alf_stats_of_planes(pic_w, pic_h, bit_depth, n_bins, org, rec, true, luma_d, chroma_d)) return rc;
  AlfRes r; memset(&r, 0, sizeof r);
  r.luma = luma_d.p; r.chroma = chroma_d.p; r.n = 1; r.nctu = ((pic_w + 127) / 128) * ((pic_h + 127) / 128); r.nb = n_bins; r.w = &work;
  return alf_decide_frames(r, true, lambda, max_luma_filters, flags, aps, slice, ctus);
}

// the same two kernels on a picture the caller describes by a CU table (host memory in, host memory out): the unit maps the kernels read are built here from the rows
extern "C" int vvcx_deblock_cu_table(int pic_w, int pic_h, int bit_depth, int qp, int qp_cb, int qp_cr, int beta_offset_div2, int tc_offset_div2,
                                     const int32_t *rows, int n_rows, uint16_t *y, uint16_t *cb, uint16_t *cr, int device)
{
  if (!rows || !y || !cb || !cr || n_rows <= 0) return fail(VVCX_ERR_ARG, "null argument");
  if (pic_w < 8 || pic_h < 8 || (pic_w & 7) || (pic_h & 7) || pic_w > 16384 || pic_h > 16384) return fail(VVCX_ERR_ARG, "picture size must be a multiple of 8 (MinCUSize of the cfg) up to 16384");
  if (bit_depth < 8 || bit_depth > 12 || qp < 0 || qp > 63 || beta_offset_div2 < -6 || beta_offset_div2 > 6 || tc_offset_div2 < -6 || tc_offset_div2 > 6) return fail(VVCX_ERR_ARG, "bit depth / QP / offsets out of range");
  const int uw = pic_w >> 2, uh = pic_h >> 2;
  std::vector<VxUnit> um((size_t) 2 * uw * uh);
  memset(um.data(), 0, um.size() * sizeof(VxUnit));
  for (int i = 0; i < n_rows; i++) {
    const int32_t *r = rows + 6 * i;
    const int ch = r[0], sh = ch ? 1 : 0;
    const bool pow2 = r[3] > 0 && r[4] > 0 && !(r[3] & (r[3] - 1)) && !(r[4] & (r[4] - 1));
    if (ch < 0 || ch > 1 || !pow2 || r[3] < 4 || r[4] < 4 || r[3] > 128 || r[4] > 128 || (r[1] & 3) || (r[2] & 3) || r[1] < 0 || r[2] < 0 || r[1] + r[3] > pic_w || r[2] + r[4] > pic_h ||
        r[5] < 0 || r[5] > 2 || (r[5] && (ch || r[3] * r[4] <= 16 || r[3] > 64 || r[4] > 64)))
      return fail(VVCX_ERR_ARG, "CU row %d is not a CU of a %dx%d picture", i, pic_w, pic_h);
    int lw = 0, lh = 0;
    while ((1 << lw) < (r[3] >> sh)) lw++;
    while ((1 << lh) < (r[4] >> sh)) lh++;
    for (int v = r[2] >> 2; v < (r[2] + r[4]) >> 2; v++) for (int u = r[1] >> 2; u < (r[1] + r[3]) >> 2; u++) {
      VxUnit &t = um[(size_t) ch * uw * uh + (size_t) v * uw + u];
      t.tag = 1; t.x = (int16_t) (r[1] >> sh); t.y = (int16_t) (r[2] >> sh); t.lw = (uint8_t) lw; t.lh = (uint8_t) lh; t.mts = (uint8_t) (r[5] << 6);
    }
  }
  for (size_t i = 0; i < um.size(); i++) if (!um[i].tag) return fail(VVCX_ERR_ARG, "the CU table does not cover the picture (%s tree, 4x4 unit %d)", i < um.size() / 2 ? "luma" : "chroma", (int) (i % (um.size() / 2)));
  ON_DEVICE(device);
  DevPicture pic; DevBuf<VxUnit> um_d; DevBuf<uint8_t> ed_d;
  HIPCHK(ed_d.alloc((size_t) 4 * uw * uh)); HIPCHK(um_d.alloc(um.size()));
  HIPCHK(hipMemcpy(um_d.p, um.data(), um.size() * sizeof(VxUnit), hipMemcpyHostToDevice));
  const uint16_t *const rec[3] = { y, cb, cr };
  if (const int rc = pic.upload(pic_w, pic_h, rec, nullptr, um_d.p)) return rc;
  VxDeblockParams p; memset(&p, 0, sizeof p);
  p.frames = pic.frame.p; p.uw = uw; p.uh = uh; p.bit_depth = bit_depth; p.chroma = 1; p.qp = qp; p.qp_c[0] = qp_cb; p.qp_c[1] = qp_cr; p.beta_off2 = beta_offset_div2; p.tc_off2 = tc_offset_div2; p.edges = ed_d.p;
  const dim3 grid((unsigned) ((2 * uw * uh + 255) / 256), 1);
  hipLaunchKernelGGL(vvcx_deblock_edges_kernel, grid, dim3(256), 0, 0, p);
  HIPCHK(hipGetLastError());
  for (int dir = 0; dir < 2; dir++) {
    p.dir = dir;
    hipLaunchKernelGGL(vvcx_deblock_kernel_u16, grid, dim3(256), 0, 0, p);
    HIPCHK(hipGetLastError());
  }
  return pic.download(y, cb, cr);
}

