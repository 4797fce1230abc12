/*
 * vvcx.h — C-ABI of the MI355X-native VVC intra CU-partition RDO path.
 *
 * Drop-in boundary: the reference has no FFI; the functional seam is the member call
 *     void EncCu::compressCtu(CodingStructure& cs, const UnitArea& area, unsigned ctuRsAddr,
 *                             const int prevQP[], const int currQP[]);          // EL/EncCu.h:177
 * invoked once per CTU from EncSlice::encodeCtus (EL/EncSlice.cpp:1768), plus its set-up contract
 * create()/init()/destroy() (EL/EncCu.h:167-174) and the per-slice state the caller pushes before
 * the CTU loop (lambda, QP, contexts: EL/EncSlice.cpp:1568-1572,1640-1661).  Each entry point below
 * names the reference interface it replaces.  Plain C structs, no exceptions across the ABI: every
 * function returns 0 on success or a negative vvcx_status; vvcx_last_error() gives the text.
 * A handle is not thread-safe (one per GPU / host thread), like one EncCu instance per worker
 * (EL/EncLib.cpp:115-125).
 *
 * Paths in comments are relative to /root/reference/VVC_project/source/Lib (EL = EncoderLib, CL = CommonLib).
 */
#ifndef VVCX_H
#define VVCX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  VVCX_OK = 0, VVCX_ERR_ARG = -1, VVCX_ERR_UNSUPPORTED = -2, VVCX_ERR_DEVICE = -3, VVCX_ERR_STATE = -4, VVCX_ERR_NO_ENCODING = -5
} vvcx_status;

/* encoder tools of BIN/encoder_intra.cfg that reach the hot path.  Requesting a tool that
 * is not built yet fails with VVCX_ERR_UNSUPPORTED instead of silently changing the result. */
enum {
  VVCX_TOOL_MRL = 1 << 0, VVCX_TOOL_MIP = 1 << 1, VVCX_TOOL_ISP = 1 << 2, VVCX_TOOL_LFNST = 1 << 3, VVCX_TOOL_MTS = 1 << 4,
  VVCX_TOOL_TS = 1 << 5, VVCX_TOOL_DEPQUANT = 1 << 6, VVCX_TOOL_RDOQ = 1 << 7, VVCX_TOOL_CCLM = 1 << 8,
  VVCX_TOOL_JCCR = 1 << 9, VVCX_TOOL_LMCS = 1 << 10, VVCX_TOOL_CU_REUSE = 1 << 11,
  VVCX_TOOL_FAST = 1 << 12,     /* the fork's FAST_ALGORITHM (CL/TypeDef.h:54-56): features + forest pick the one partition mode of a luma node */
  VVCX_TOOL_WPP = 1 << 13       /* cfg WaveFrontSynchro 1 (off in encoder_intra.cfg): a CTU row of a tile starts from the contexts behind the first CTU of the row above
                                 * (EL/EncSlice.cpp:1648-1661, 1801-1805), the CTU above-right is unavailable (CL/CodingStructure.cpp:1634-1657), one sub-stream per CTU row.
                                 * The rows of a tile become streams of their own that run one CTU behind the row above */
};

/* ≙ the EncCfg/SPS fields EncCu::create/init read (EL/EncCu.cpp:167-236, CL/Slice.h PreCalcValues 2229-2275) */
typedef struct {
  int32_t pic_w, pic_h;          /* luma samples, multiples of 8 (APP/EncAppCfg.cpp:2709) */
  int32_t bit_depth;             /* InternalBitDepth: 8 (uint8 planes) or 10 (uint16 planes) */
  int32_t ctu_size;              /* CTUSize 128 */
  int32_t min_qt[2];             /* MinQTLumaISlice, MinQTChromaISlice */
  int32_t max_bt_depth[2];       /* MaxBTDepthISliceL / C */
  int32_t max_bt_size[2];        /* MAX_BT_SIZE / MAX_BT_SIZE_C (CL/CommonDef.h:427,437) */
  int32_t max_tt_size[2];        /* MAX_TT_SIZE / MAX_TT_SIZE_C */
  int32_t dual_tree;             /* DualITree */
  int32_t tile_cols, tile_rows;  /* uniform tile grid; every tile is an independent CTU stream */
  uint32_t tools;                /* VVCX_TOOL_* */
  int32_t chroma;                /* 1 = code the chroma tree too (4:2:0) */
  int32_t max_frames;            /* frames resident per batch */
  int32_t device;                /* HIP device ordinal */
  int32_t emit_payload;          /* 1 = also arithmetic-code the final CTU syntax: slice_data() payload per tile (vvcx_get_payload) */
} vvcx_cfg;

/* ≙ per-slice state pushed by EncSlice before the CTU loop: setUpLambda (EL/EncSlice.cpp:107-149),
 * slice QP, mapped chroma QPs; CABAC contexts are (re)initialised at each tile start (1640-1647) */
typedef struct {
  int32_t qp;
  int32_t qp_c[2];
  double  lambda;
  double  dist_weight[2];
  /* LMCS (VVCX_TOOL_LMCS): the model the slice's LMCS APS carries (SliceReshapeInfo, CL/Slice.h; chosen per picture by EncReshape::preAnalyzerLMCS, which is the
   * caller's job like lambda and QP).  The handle builds the forward / inverse LUTs and the chroma scale table from it the way Reshape::constructReshaper does
   * (CL/Reshape.cpp:297-333).  lmcs_enable 0 (the analysis switched the tool off for this picture): the other fields are ignored. */
  int32_t lmcs_enable;           /* slice_lmcs_enabled_flag */
  int32_t lmcs_chroma_adj;       /* slice_chroma_residual_scale_flag */
  int32_t lmcs_min_bin, lmcs_max_bin;   /* reshaperModelMinBinIdx / MaxBinIdx */
  int32_t lmcs_delta_cw[16];     /* reshaperModelBinCWDelta: signed deviation of each bin's code words from (1 << bit_depth) / 16 */
} vvcx_slice;

/* one picture of a batch: DEVICE pointers to planar 4:2:0 samples (uint8 for 8 bit, uint16 for 10 bit),
 * strides in samples.  ≙ cs.picture->getOrigBuf()/getRecoBuf() (CL/Picture.h); reco is written in place */
typedef struct {
  const void *org[3];
  void       *reco[3];
  int32_t     stride[3];
} vvcx_frame;

/* ≙ arguments of compressCtu: which CTU of which bound picture */
typedef struct { int32_t frame; int32_t ctu_rs_addr; } vvcx_ctu_task;

/* ≙ bestCS->dist / fracBits / cost after compressCtu (CL/CodingStructure.h:178-184), luma + chroma tree */
typedef struct {
  uint64_t dist;
  uint64_t frac_bits;            /* 2^-15 bit units (CL/CommonDef.h:354) */
  double   cost;
  int32_t  n_cu;
} vvcx_ctu_result;

/* ≙ the CodingUnit/PredictionUnit/TransformUnit fields of the final CUs appended to cs (CL/Unit.h:292-470) */
typedef struct {
  int16_t  x, y, w, h;           /* luma samples for ch_type 0, chroma samples for ch_type 1 */
  uint8_t  ch_type;
  uint8_t  qt_depth, bt_depth, mt_depth, depth;
  uint8_t  intra_dir;            /* luma mode 0..66; chroma mode (70 = DM) */
  uint8_t  mrl_idx;              /* multiRefIdx */
  uint8_t  cbf;                  /* bit0 Y, bit1 Cb, bit2 Cr */
  uint8_t  mts_idx;              /* tu.mtsIdx of the luma TU: 0 DCT2xDCT2, 1 transform skip (VVCX_TOOL_TS), 2..5 explicit MTS (VVCX_TOOL_MTS) */
  uint8_t  mip_flag;             /* cu.mipFlag of a luma CU (VVCX_TOOL_MIP): intra_dir is then the MIP mode, mrl_idx 0 */
  uint8_t  lfnst_idx;            /* cu.lfnstIdx of the CU (VVCX_TOOL_LFNST): 0 none, 1 / 2 the kernel of the set */
  uint8_t  joint_cb_cr;          /* tu.jointCbCr of a chroma CU (VVCX_TOOL_JCCR): 0 separate residuals, 1..3 the cbf mask of the joint residual */
  uint8_t  isp_mode;             /* cu.ispMode of a luma CU (VVCX_TOOL_ISP): 0 none, 1 horizontal split (sub-partitions stacked), 2 vertical split */
  uint8_t  tu_cbf;               /* ISP: bit k = cbf of sub-partition k (cbf bit 0 is then their OR) */
  uint64_t split_series;         /* CU::splitSeries, 5 bits per depth */
} vvcx_cu;

/* one transform unit ≙ TransformUnit (CL/Unit.h:412-470): area, depth, mtsIdx, cbf[], jointCbCr and where its coefficients are */
typedef struct {
  int32_t  cu_index;             /* index of its CU in vvcx_get_cus order */
  int16_t  x, y, w, h;           /* like the CU: luma samples for ch_type 0, chroma samples for ch_type 1 */
  uint8_t  ch_type, depth;       /* transform depth (0: the TU is the CU; 1: a sub-partition of an ISP CU) */
  uint8_t  mts_idx;              /* tu.mtsIdx (luma) */
  uint8_t  joint_cb_cr;          /* tu.jointCbCr (chroma) */
  uint8_t  cbf[3];               /* Y, Cb, Cr */
  uint8_t  pad_;
  int32_t  coeff_offset[3];      /* sample offset of the block's levels in the level plane of component c, -1 if absent */
  int32_t  coeff_stride[3];
} vvcx_tu;

typedef struct vvcx_handle vvcx_handle;

/* ≙ EncCu::create(EncCfg*) + init(EncLib*, const SPS&)  (EL/EncCu.h:167-171) */
int  vvcx_create(const vvcx_cfg *cfg, vvcx_handle **h);
/* ≙ EncCu::destroy() (EL/EncCu.h:173) */
void vvcx_destroy(vvcx_handle *h);
/* ≙ EncSlice::setUpLambda + slice QP (EL/EncSlice.cpp:107-149, 1568-1572).  Precedes vvcx_bind_frames: binding prepares the pictures for the slice (start contexts of
 * its QP, forward-mapped luma and device LUTs of its LMCS model).  A later call whose QP or LMCS model differs UNBINDS the pictures (the next search call then reports
 * VVCX_ERR_STATE until they are bound again); one that changes only lambda / the distortion weights leaves them bound. */
int  vvcx_set_slice(vvcx_handle *h, const vvcx_slice *s);
/* ---- slice-level inputs: what the reference derives before the CTU loop, as pure host functions ---- */
typedef struct {
  int32_t qp;                    /* slice QP (cfg QP) */
  int32_t bit_depth;             /* 8 or 10 */
  int32_t n_pts;                 /* chroma QP mapping pivots: cfg QpInValCb / QpOutValCb (SameCQPTablesForAllChroma 1), 1..8 */
  int32_t qp_in[8], qp_out[8];   /* BIN/encoder_intra.cfg:86-87: "2 31 43" -> "2 32 41" */
  int32_t cb_qp_offset, cr_qp_offset;   /* cfg CbQpOffset / CrQpOffset */
  int32_t gop_size;              /* cfg GOPSize (1 for All-Intra): lambda scale 1 - clip(0, 0.5, 0.05 * (GOPSize - 1)) */
  int32_t dep_quant;             /* cfg DepQuant: lambda * 2^(0.25/3) */
} vvcx_slice_cfg;
/* ≙ ChromaQpMappingTable::derivedChromaQPMappingTables (CL/Slice.cpp:1540-1581): table[q + 6*(bit_depth-8)] = mapped chroma QP of
 * luma-scale QP q, q = -6*(bit_depth-8) .. 63 */
int  vvcx_chroma_qp_table(int bit_depth, int n_pts, const int32_t *qp_in, const int32_t *qp_out, int32_t *table);
/* ≙ EncSlice::calculateLambda for an I slice (EL/EncSlice.cpp:752-845: QPFactor 0.57 * scale, 2^((QP + 6*(bd-8) - 12)/3), DepQuant factor)
 * + the chroma QPs QpParam uses (CL/Quant.cpp:68-106) + EncSlice::setUpLambda's distortion weights 2^((QP - QPc)/3) (107-149) */
int  vvcx_derive_slice(const vvcx_slice_cfg *cfg, vvcx_slice *out);

/* ≙ the model the fork's classifier asks at every qualifying luma node: Py_Initialize + joblib.load("Partition_32.pkl").predict(x)
 * per call (EL/EncCu.cpp:1140-1166, BIN/TEST.py:7-25), replaced by one upload of the forest's flattened sklearn tree arrays (host
 * pointers): root[n_trees]; feature / left / right [n_nodes] (children -1 at leaves, children after their parent); threshold[n_nodes]
 * (go left when float(x[feature]) <= threshold); value[n_nodes][n_classes] class distributions; classes[n_classes] = label of each
 * column (0 do not split, 1 QT, 2 BT_H, 3 BT_V, 4 TT_H, 5 TT_V).  Needed before the first CTU when VVCX_TOOL_FAST is set. */
int  vvcx_set_forest(vvcx_handle *h, int n_trees, int n_nodes, int n_classes, const int32_t *root, const int32_t *feature, const double *threshold,
                     const int32_t *left, const int32_t *right, const double *value, const int32_t *classes);
/* bind n pictures (device pointers) as the current batch and reset every CTU stream to its tile start
 * (≙ Picture::finalInit + the context reset of EL/EncSlice.cpp:1640-1647) */
int  vvcx_bind_frames(vvcx_handle *h, const vvcx_frame *frames, int n);
/* ≙ n calls of EncCu::compressCtu (EL/EncCu.cpp:428) followed by the estimator pass
 * CABACWriter::coding_tree_unit that advances the contexts (EL/EncSlice.cpp:1775-1776).
 * Tasks of one (frame, tile) stream must appear in raster order of the tile and continue where the last
 * call stopped; different streams run concurrently, one workgroup per stream.  `out` is host memory [n].
 * `hip_stream` is a hipStream_t (NULL = default stream); the call returns after the work completed. */
int  vvcx_compress_ctus(vvcx_handle *h, const vvcx_ctu_task *tasks, int n, vvcx_ctu_result *out, void *hip_stream);
/* The same call in two halves, for a host that keeps working while the device searches (the reference's CTU loop is synchronous,
 * EL/EncSlice.cpp:1560-1790; an encoder with frame threads would overlap picture N's search with picture N-1's write-out here).
 * vvcx_submit_ctus validates and enqueues uploads, the launch and the copy of the results into pinned host memory on `hip_stream`
 * and returns without waiting; vvcx_poll_ctus = 1 when done, 0 while running; vvcx_wait_ctus blocks, advances the streams'
 * positions and fills out[n] (n = the submitted count).  One submission per handle may be outstanding; until it is collected
 * every other entry point that touches the handle's device state returns VVCX_ERR_STATE. */
int  vvcx_submit_ctus(vvcx_handle *h, const vvcx_ctu_task *tasks, int n, void *hip_stream);
int  vvcx_poll_ctus(vvcx_handle *h);
int  vvcx_wait_ctus(vvcx_handle *h, vvcx_ctu_result *out, int n);
/* convenience: all CTUs of all bound frames in stream order (one launch) */
int  vvcx_compress_bound_frames(vvcx_handle *h, vvcx_ctu_result *out /* [n_frames * ctus_per_frame], host */, void *hip_stream);
/* final CU table of one bound frame (CTU raster order; per CTU luma CUs then chroma CUs, by origin).
 * ≙ walking cs.cus after the CTU loop; same fields D_BLOCK_STATISTICS_CODED traces */
int  vvcx_get_cus(vvcx_handle *h, int frame, vvcx_cu *cus, int max_cus, int *n_cus);
/* The TU records of the same picture (≙ cs.tus; EL/EncSlice.cpp reads them through CodingStructure::traverseTUs when it writes the slice): one per CU
 * (every intra CU of a dual-tree I slice fits MaxTbSize 64) or one per sub-partition of a luma CU coded with ISP (2 or 4, in coding order), CUs in vvcx_get_cus order.  coeff_offset[c] / coeff_stride[c] address the block's quantised levels
 * inside the plane vvcx_get_levels(h, frame, c, ...) returns (-1: the TU has no block of component c); a joint chroma TU keeps its levels with the coded
 * component (Cb for joint_cb_cr 2 / 3, Cr for 1).  tus may be NULL to query the count. */
int  vvcx_get_tus(vvcx_handle *h, int frame, vvcx_tu *tus, int max_tus, int *n_tus);
/* ≙ tu.getCoeffs(compID) of the final TUs: the quantised levels of component comp (0 Y, 1 Cb, 2 Cr) at their sample positions, copied to
 * a host plane (what a caller needs to rebuild cs.tus for the reference's own CABACWriter instead of taking vvcx_get_payload) */
int  vvcx_get_levels(vvcx_handle *h, int frame, int comp, int16_t *plane, int stride);
/* LMCS: the search runs, and leaves the luma reconstruction, in the mapped domain (the original luma of a bound picture is forward mapped into a buffer of the handle
 * when it is bound, ≙ EncGOP::xPicInitLMCS, EL/EncGOP.cpp:1689-1695; an SDR intra picture has no CTU-level weighted distortion: EL/EncSlice.cpp sets
 * CTUFlag false for it, so the mapped-domain SSE is the reference's distortion).  This maps the luma reconstruction of every bound picture back through the
 * inverse LUT in place (≙ the picture-level rspSignal before the loop filters, DL/DecLib.cpp executeLoopFilters); call it once all CTUs are coded and before
 * vvcx_deblock_bound_frames.  VVCX_ERR_STATE when the slice does not enable LMCS. */
int  vvcx_lmcs_inverse_reco(vvcx_handle *h, void *hip_stream);
/* ≙ EncGOP::xPicInitLMCS → EncReshape::preAnalyzerLMCS + the model half of constructReshaperLMCS (EL/EncReshape.cpp:410-559, 166-409, 977-1229, 1835-1893, 2194-2256) for an intra
 * picture with the cfg's LMCSSignalType 0 and LMCSAdpOption 0: the picture analysis that decides whether the slice uses LMCS and with which model.  org / stride: the original
 * 4:2:0 planes in HOST memory (uint8 below 10 bit, else uint16), update_ctrl = cfg LMCSUpdateCtrl (1 in encoder_intra.cfg; 0 supported, 2 is not an intra setting).  Fills
 * slice->lmcs_enable / lmcs_chroma_adj / lmcs_min_bin / lmcs_max_bin / lmcs_delta_cw (the other members are left alone); hand the slice to vvcx_set_slice before
 * vvcx_bind_frames.  Like the reference it leaves LMCS off for every picture below 10 bit and for full-range 10-bit content.  Needs no handle; the statistics pass (window
 * variances per luma bin, moments of the three planes) runs on the current HIP device: vvcx_lmcs_analyze uploads the host planes first, vvcx_lmcs_analyze_device takes planes
 * that are in device memory already (the pointers later given to vvcx_bind_frames) */
int  vvcx_lmcs_analyze(const void *const org[3], const int stride[3], int pic_w, int pic_h, int bit_depth, int slice_qp, int update_ctrl, vvcx_slice *slice);
int  vvcx_lmcs_analyze_device(const void *const org[3], const int stride[3], int pic_w, int pic_h, int bit_depth, int slice_qp, int update_ctrl, vvcx_slice *slice);
/* the LUTs and tables the handle derived from the slice's model: fwd / inv [1 << bit_depth], pivot[17] (mapped-domain bin borders), chroma_scale[16] (11 fractional bits) */
int  vvcx_lmcs_tables(vvcx_handle *h, int16_t *fwd, int16_t *inv, int32_t pivot[17], int32_t chroma_scale[16]);
/* ≙ LoopFilter::loopFilterPic (CL/LoopFilter.cpp:153; called from EncGOP after the slices of a picture are compressed): in-loop deblocking
 * of every bound picture, in place on its reconstruction planes; offsets = cfg LoopFilterBetaOffset_div2 / LoopFilterTcOffset_div2.
 * Every CTU of the pictures must have been compressed.  SAO and ALF follow in the reference: vvcx_sao_bound_frames and vvcx_alf_bound_frames below. */
int  vvcx_deblock_bound_frames(vvcx_handle *h, int beta_offset_div2, int tc_offset_div2, void *hip_stream);
float vvcx_last_deblock_ms(const vvcx_handle *h);
/* ≙ SampleAdaptiveOffset::SAOProcess(cs, saoBlkParams) (CL/SampleAdaptiveOffset.cpp:617-670): sample adaptive offset on every bound (completely coded) picture, in place on
 * the reconstruction planes, with the caller's per-CTU parameters prm[frame][ctu raster address][component] (≙ SAOBlkParam, CL/TypeDef.h:1122-1140): mode 0 off / 1 new /
 * 2 merge; type: for a new CTU 0..3 = edge class 0 / 90 / 135 / 45 degrees, 4 = band offset, for a merge 0 = from the CTU to the left, 1 = from the CTU above (which must be
 * in the same tile); band = band position (0..31); offset[4] = the four coded offsets (edge: full valley, half valley, half peak, full peak; band: the four bands from the
 * band position), multiplied by 2^log2_offset_scale.  lf_across_tiles = pps loop_filter_across_bricks_enabled_flag.  The parameter DECISION (EncSampleAdaptiveOffset) is
 * vvcx_sao_statistics_bound_frames + vvcx_sao_decide below, or vvcx_sao_decide_resident (both halves on the device; vvcx_sao_bound_frames_resident then filters without
 * the parameters crossing to the host and back).  In the reference's order this follows vvcx_deblock_bound_frames. */
typedef struct vvcx_sao_param { int8_t mode, type, band, offset[4]; } vvcx_sao_param;
int   vvcx_sao_bound_frames(vvcx_handle *h, const vvcx_sao_param *prm, int lf_across_tiles, int log2_offset_scale, void *hip_stream);
float vvcx_last_sao_ms(const vvcx_handle *h);
/* ≙ EncSampleAdaptiveOffset::getStatistics (EL/EncSampleAdaptiveOffset.cpp:284-353 with getBlkStats 1135-1549, SAOLcuBoundary 0 as in the cfg): the statistics the
 * reference's parameter decision (decideBlkParams) works from, gathered on the device from the bound original and the deblocked reconstruction - the O(samples) half of that
 * decision; its RD half stays with the caller's encoder.  stats (host memory): [frame][ctu raster address][component][type 0..3 = edge class 0 / 90 / 135 / 45 degrees,
 * 4 = band][0: count, 1: sum of (original - deblocked)][32] int64 (≙ SAOStatData::count / ::diff; edge types use entries 0..4 = the classes full valley, half valley, plain,
 * half peak, full peak; band: 32 bands).  Call it after vvcx_deblock_bound_frames and before vvcx_sao_bound_frames.  Not available for an LMCS slice (the handle keeps the
 * mapped original only): VVCX_ERR_UNSUPPORTED. */
int   vvcx_sao_statistics_bound_frames(vvcx_handle *h, int lf_across_tiles, int64_t *stats, void *hip_stream);
float vvcx_last_sao_stats_ms(const vvcx_handle *h);
/* ≙ EncSampleAdaptiveOffset::decideBlkParams (EL/EncSampleAdaptiveOffset.cpp:793-1098, SAOGreedyEnc 0; deriveModeNewRDO 597-735, deriveModeMergeRDO 737-791, deriveOffsets
 * 481-595): the RD half of the SAO parameter decision for ONE picture from its statistics (the [ctu][component][type][count | diff][32] block of that picture as
 * vvcx_sao_statistics_bound_frames returns it): per CTU the better of new parameters (per component the type and offsets with the least distortion + lambda * bits; Cb and Cr
 * share the type) and a merge with the CTU to the left / above in the same tile, bits as CABACWriter::sao_block_pars codes them against the two SAO context models, which
 * start from the I-slice initialisation at slice_qp and adapt from CTU to CTU.  lambda[3] = the slice's lambdas per component (≙ Slice::getLambdas); every component is
 * enabled (what decidePicParams decides for temporal layer 0).  Host code, needs no handle.  prm[ctu][component] = the coded parameters vvcx_sao_bound_frames takes.
 * Parity with the reference is unpinned (the unit does not compile in this environment). */
int   vvcx_sao_decide(int pic_w, int pic_h, int bit_depth, int tile_cols, int tile_rows, int slice_qp, const double *lambda, int log2_offset_scale,
                      const int64_t *stats, vvcx_sao_param *prm);
/* ---- the same decision on the device, from statistics that STAY in device memory (csrc/vvcx_sao_decide.hip).  Call order on bound pictures:
 *   ... -> vvcx_deblock_bound_frames -> vvcx_sao_decide_resident -> vvcx_sao_bound_frames_resident -> vvcx_alf_statistics_resident -> ...
 * vvcx_sao_decide_resident runs the statistics kernel of vvcx_sao_statistics_bound_frames on the bound (completely coded, deblocked) pictures without the copy to the
 * host, then two decision kernels: one prices every (CTU, component, type) - the offset search, its distortion, the bypass bins - with one lane per (component, type,
 * class); one walks the CTUs of each picture in raster order with the two context models (one wave per picture) and chooses among the priced candidates and the two merge
 * candidates.  The result is vvcx_sao_decide's, bit for bit (fp64 cost arithmetic in the same order of operations; that host code is what the tests compare with, and like
 * it the decision is not pinned to the reference encoder).  The slice QP of the context initialisation is the handle's.  Two things stay in device memory: the resolved
 * filter table (merges resolved, offsets scaled) that vvcx_sao_bound_frames_resident reads, and the coded parameters.  prm[frame][ctu][component] (host memory, may be
 * NULL) receives the coded parameters, 21 bytes per CTU - what vvcx_rewrite_payload_bound_frames takes.  Works on an LMCS slice (after vvcx_lmcs_inverse_reco, else
 * VVCX_ERR_STATE): the handle remembers the caller's own luma plane beside the forward-mapped copy, and the statistics are measured against it, as the reference restores
 * the true original in front of the loop filters.  VVCX_ERR_ARG: a lambda that is not > 0, an offset scale outside 0..4; VVCX_ERR_STATE: nothing bound, a CTU not coded.
 * vvcx_last_sao_stats_ms / vvcx_last_sao_decide_ms: HIP-event times of the statistics kernel and of the two decision kernels of the last call.
 * vvcx_sao_bound_frames_resident: the copy and filter kernels of vvcx_sao_bound_frames on the resident table, lf_across_tiles as given to the decision.  The decision is
 * valid until a call touches the bound pictures or the buffers: binding, compressing, vvcx_lmcs_inverse_reco, deblocking, either SAO filter call (a second pass would
 * filter filtered samples), the ALF filter, vvcx_sao_statistics_bound_frames.  VVCX_ERR_STATE without a valid decision. */
int   vvcx_sao_decide_resident(vvcx_handle *h, int lf_across_tiles, const double lambda[3], int log2_offset_scale, vvcx_sao_param *prm, void *hip_stream);
int   vvcx_sao_bound_frames_resident(vvcx_handle *h, void *hip_stream);
float vvcx_last_sao_decide_ms(const vvcx_handle *h);
/* the same kernels on one picture in host memory (uint16 planes, stride = plane width; prm[ctu][component]): uploads the planes, gathers the statistics, decides.  Needs no
 * handle; the form the decision kernels are tested through. */
int   vvcx_sao_decide_picture(int pic_w, int pic_h, int bit_depth, int tile_cols, int tile_rows, int slice_qp, const double lambda[3], int log2_offset_scale,
                              int lf_across_tiles, const uint16_t *const org[3], const uint16_t *const rec[3], vvcx_sao_param *prm, int device);
/* the same filter on one picture in host memory (uint16 planes, stride = plane width, filtered in place; prm[ctu][component]): needs no handle */
int   vvcx_sao_picture(int pic_w, int pic_h, int bit_depth, int tile_cols, int tile_rows, const vvcx_sao_param *prm, int lf_across_tiles, int log2_offset_scale,
                       uint16_t *y, uint16_t *cb, uint16_t *cr, int device);
/* ≙ AdaptiveLoopFilter::ALFProcess(cs) (CL/AdaptiveLoopFilter.cpp:205-383): the adaptive loop filter on every bound (completely coded) picture, in place on the
 * reconstruction planes, with the caller's parameter sets and per-CTU choices.  aps[n_aps] (n_aps <= 8) = what the ALF parameter sets carry (≙ AlfParam,
 * CL/AlfParameters.h:134-160, JVET_O0669 form: no coefficient prediction): up to 25 luma filters of 12 coefficients + clipping indices (used when nonlinear_luma), the filter of
 * each of the 25 classes (filterCoeffDeltaIdx), up to 8 chroma alternatives of 6 coefficients + clipping indices.  slices[frame] (≙ the slice header): the parameter sets luma
 * is filtered with (luma_aps[k] -> filter set 16 + k; sets 0..15 are the standard's fixed ones) and the set of the chroma alternatives (chroma_aps < 0: chroma stays).
 * ctus[frame][ctu raster address]: enable flags Y / Cb / Cr (≙ Picture::getAlfCtuEnableFlag), luma filter set (getAlfCtbFilterIndex), chroma alternatives
 * (getAlfCtuAlternativeData).  Class derivation (deriveClassificationBlk 792-1002), the 7 x 7 / 5 x 5 diamond filters with clipping (filterBlk 1005-1296) and the virtual
 * boundary above every lower CTU border are the reference's; tiles are not looked at (its ALF of this version does not either).  The parameter DECISION
 * (EncAdaptiveLoopFilter) is vvcx_alf_statistics_bound_frames + vvcx_alf_decide below (linear filters), or vvcx_alf_statistics_resident + vvcx_alf_decide_resident
 * (statistics kept in device memory; nonlinear filters and the fixed sets as candidates).  In the reference's order this follows vvcx_sao_bound_frames. */
typedef struct vvcx_alf_aps {
  int32_t num_luma_filters; uint8_t class_to_filter[25]; uint8_t nonlinear_luma; int16_t luma_coeff[25][12]; uint8_t luma_clip_idx[25][12];
  int32_t num_chroma_alt; uint8_t nonlinear_chroma[8]; int16_t chroma_coeff[8][6]; uint8_t chroma_clip_idx[8][6];
} vvcx_alf_aps;
typedef struct vvcx_alf_slice { int32_t n_luma_aps, luma_aps[8], chroma_aps; } vvcx_alf_slice;
typedef struct vvcx_alf_ctu { uint8_t flag[3]; int8_t set; uint8_t alt[2]; } vvcx_alf_ctu;
int   vvcx_alf_bound_frames(vvcx_handle *h, const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, void *hip_stream);
float vvcx_last_alf_ms(const vvcx_handle *h);
/* the same filter on one picture in host memory (uint16 planes, stride = plane width, filtered in place): needs no handle.  classes (may be NULL): class | transpose << 5 of
 * every luma 4 x 4 block of the CTUs with luma enabled (255 elsewhere), (pic_w / 4) per row */
int   vvcx_alf_picture(int pic_w, int pic_h, int bit_depth, const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slice, const vvcx_alf_ctu *ctus,
                       uint16_t *y, uint16_t *cb, uint16_t *cr, uint8_t *classes, int device);
/* ---- the encoder side of ALF (EL/EncAdaptiveLoopFilter.cpp).  Call order of the loop-filter stage on bound pictures:
 *   vvcx_deblock_bound_frames -> vvcx_sao_statistics_bound_frames -> vvcx_sao_decide -> vvcx_sao_bound_frames
 *   -> vvcx_alf_statistics_bound_frames -> vvcx_alf_decide -> vvcx_alf_bound_frames
 * or, with both decisions from statistics that stay in device memory (on an LMCS slice vvcx_lmcs_inverse_reco comes in front of the deblocking),
 *   ... -> vvcx_deblock_bound_frames -> vvcx_sao_decide_resident -> vvcx_sao_bound_frames_resident -> vvcx_alf_statistics_resident -> vvcx_alf_decide_resident
 *   -> vvcx_alf_bound_frames
 * and, for the bitstream, ... -> vvcx_alf_decide -> vvcx_rewrite_payload_bound_frames -> vvcx_get_payload (the rewrite reads no samples: before or after the filter calls).
 *
 * ≙ EncAdaptiveLoopFilter::deriveStatsForFiltering (EL/EncAdaptiveLoopFilter.cpp:2650-2745; getBlkStats 2746-2843, calcCovariance 2844-2965, m_alfWSSD off): the content of
 * AlfCovariance per CTU and class, gathered on the device from the original and the picture the ALF filter would read (after deblocking and SAO).  Per sample s and
 * clipping bin b < n_bins (n_bins = 1: bin 0 only, enough for linear filters; or 4):  v[k][b] = clip(-C_b, C_b, r0 - cur) + clip(-C_b, C_b, r1 - cur)  for the tap pairs
 * k = 0..11 (luma) / 0..5 (chroma), k being the coefficient index of vvcx_alf_aps.luma_coeff / chroma_coeff (luma: after the block's transpose index has been applied),
 * v[12 / 6][b] = cur, C_b = the clipping value of index b (C_0 = 1 << bit_depth: no clipping), d = org - cur; vertical tap distances shorten at the virtual boundary and
 * picture borders repeat the edge sample exactly as in the filter.  Per (CTU, class; chroma: per CTU and component) the exact int64 sums
 *   E[b0][b1][k][l] = sum v[k][b0] v[l][b1] (the full array: E[b0][b1][k][l] == E[b1][b0][l][k]),  y[b][k] = sum v[k][b] d,  pixAcc = sum d d
 * in the order E, y, pixAcc:  luma[frame][ctu][25][nb*nb*169 + nb*13 + 1],  chroma[frame][ctu][2][nb*nb*49 + nb*7 + 1]  (host memory; 4 bins are about 550 KB per CTU,
 * hence the frame range of the bound form).  Every block of the picture is classified, whatever flags its CTU gets later; class and transpose index are the filter's.
 * The host-plane form needs no handle (like vvcx_alf_picture): org / rec = uint16 planes, stride = plane width; chroma may be NULL (luma only). */
int   vvcx_alf_statistics_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3],
                                  int64_t *luma, int64_t *chroma, int device);
/* the same on the bound pictures frame_first .. frame_first + n - 1 (every CTU coded): after vvcx_sao_bound_frames (or vvcx_deblock_bound_frames when SAO is not used),
 * before vvcx_alf_bound_frames.  VVCX_ERR_UNSUPPORTED for an LMCS slice (the handle keeps the mapped original only).  chroma may be NULL; a handle without chroma fills it
 * with zeros. */
int   vvcx_alf_statistics_bound_frames(vvcx_handle *h, int frame_first, int n, int n_bins, int64_t *luma, int64_t *chroma, void *hip_stream);
float vvcx_last_alf_stats_ms(const vvcx_handle *h);
/* ≙ EncAdaptiveLoopFilter::ALFProcess (EL/EncAdaptiveLoopFilter.cpp:661; mergeClasses 2344, deriveFilterCoeffs 2158, deriveCoeffQuant 2279, deriveCtbAlfEnableFlags 834)
 * for ONE picture from its statistics (the [ctu][..] block of that picture, n_bins as gathered; bin 0 is read), LINEAR filters only: nonlinear_luma = 0, clip indices 0.
 * Host code, needs no handle.  Fills one parameter set (aps[0]), the slice (n_luma_aps = 1, luma_aps = {0}, chroma_aps = 0 or -1) and ctus[ctu] (set = 16).
 * Luma: the frame statistics are the sum over the enabled CTUs (all at first); the 25 classes are merged greedily down to 1 filter (always the two groups whose merge
 * raises the least-squares error least) and the filter count <= max_luma_filters with the least distortion + lambda[0] * bits is kept; per group the coefficients are the
 * Cholesky solution in double (a multiple of the mean diagonal is added while the matrix is singular), rounded to 7 fractional bits in [-128, 127] and refined by single
 * steps of one coefficient while the predicted error falls - never worse than plain rounding, never worse than the zero filter.  A CTU is enabled where its own statistics
 * predict  distortion with the filter + lambda * bits < unfiltered distortion; then the filters are derived once more from the enabled CTUs.  Chroma (chroma != 0): one
 * alternative (6 coefficients) from Cb + Cr, flags per component; chroma_aps = -1 when no CTU of either component gains.
 * Bits (this project's own count of the syntax, not the reference's estimator): parameter set luma = 1 (clip flag) + ue(filters - 1) + 25 * ceil(log2 filters) when there
 * are several + per coefficient ue(|c|) + 1 sign bit when c != 0; chroma = 1 + ue(0) + the coefficients; an enabled luma CTU costs one bin more than a disabled one
 * (alf_use_aps_flag), a chroma CTU's flag costs the same either way; a component whose gain does not pay for its parameter-set bits stays unfiltered.
 * Not here: the clip-index search for nonlinear filters and the fixed filter sets as candidates (vvcx_alf_decide_resident / vvcx_alf_decide_picture below have both);
 * out of scope here: several chroma alternatives (VVCX_ALF_CHROMA_ALTS of the resident decision has them), parameter-set reuse across pictures.  Parity with the reference's RD choice is unpinned (the unit does not compile in this environment). */
int   vvcx_alf_decide(int pic_w, int pic_h, int bit_depth, int chroma, int n_bins, const int64_t *luma, const int64_t *chroma_stats,
                      const double lambda[3], int max_luma_filters, vvcx_alf_aps *aps, vvcx_alf_slice *slice, vvcx_alf_ctu *ctus);
/* ---- the decision from statistics that STAY in device memory, with nonlinear filters and the fixed filter sets (csrc/vvcx_alf_eval.hip).  Call order on bound pictures:
 *   ... -> vvcx_sao_bound_frames -> vvcx_alf_statistics_resident -> vvcx_alf_decide_resident -> vvcx_alf_bound_frames
 * (vvcx_alf_bound_frames takes at most 8 parameter sets per call and vvcx_alf_decide_resident fills one per frame: a caller with more bound frames than that filters them
 * in groups of pictures that share their sets.)  What the decision needs from the 550 KB of a CTU are two things, both device passes:
 *   the masked frame sums (≙ getFrameStats, EL/EncAdaptiveLoopFilter.cpp:2491-2565): per frame and class the sum of the blocks of the CTUs whose mask byte is set;
 *   the candidate errors (≙ calcErrorForCoeffs, EL 225-242, per CTU and filter set as alfEncoderCtb 3153-3300 asks for them): per (CTU, candidate set s)
 *     err[s] = sum over classes ( sum_{k,l < 12} q_k q_l E[clip_k][clip_l][k][l]  -  256 sum_k q_k y[clip_k][k] )      (chroma: one class, 6 taps; the centre row is not used)
 *   with q / clip the candidate's filter of the class; err / 16384 + pixAcc is the squared error the set is predicted to leave on the CTU.  err is EXACT in int64:
 *   |v| < 2^(bd+1), at most 2^14 samples per CTU, |q| <= 128, 144 terms, so |quadratic term| < 2^(2 bd + 37.2): 2^57.2 at 10 bit, 2^61.2 at 12 bit (a double would round
 *   it).  Coefficients beyond +-128 and clipping indices >= the gathered bin count are refused (VVCX_ERR_ARG).  With fixed_sets the candidates 0..15 are the standard's
 *   fixed filter sets (clipping index 0), the caller's follow; at most 64 candidates per component and call.
 * vvcx_alf_statistics_resident: vvcx_alf_statistics_bound_frames without the copy to the host; the handle remembers (frame range, bins, chroma).  Every call that binds,
 * compresses or filters the bound pictures (and vvcx_alf_statistics_bound_frames, which uses the same memory) makes them stale: the three calls below then return
 * VVCX_ERR_STATE, as they do when nothing was gathered.  ctu_on = [n][ctus][3] bytes (Y, Cb, Cr; NULL: every CTU); luma = [n][25][size], chroma = [n][2][size] (sizes
 * as for the statistics; chroma may be NULL); candidates are given per frame: luma_cands[n][n_luma], chroma_cands[n][n_chroma]; luma_err = [n][ctus][16 fixed_sets +
 * n_luma], chroma_err = [n][ctus][2][n_chroma].  All of these are host memory; the calls block until their results have arrived. */
typedef struct vvcx_alf_luma_cand { int16_t coeff[25][12]; uint8_t clip_idx[25][12]; } vvcx_alf_luma_cand;      /* per class, class_to_filter applied */
typedef struct vvcx_alf_chroma_cand { int16_t coeff[6]; uint8_t clip_idx[6]; } vvcx_alf_chroma_cand;
int   vvcx_alf_statistics_resident(vvcx_handle *h, int frame_first, int n, int n_bins, void *hip_stream);
int   vvcx_alf_frame_statistics(vvcx_handle *h, const uint8_t *ctu_on, int64_t *luma, int64_t *chroma, void *hip_stream);
int   vvcx_alf_candidate_errors(vvcx_handle *h, int fixed_sets, const vvcx_alf_luma_cand *luma_cands, int n_luma, const vvcx_alf_chroma_cand *chroma_cands, int n_chroma,
                                int64_t *luma_err, int64_t *chroma_err, void *hip_stream);
float vvcx_last_alf_sum_ms(const vvcx_handle *h);       /* the kernel of the last frame sums / candidate errors of the handle (the decision's last ones included) */
float vvcx_last_alf_cand_ms(const vvcx_handle *h);
/* The decision of every resident frame; only frame sums and error tables cross to the host.  Per frame i it fills aps[i], slices[i] and ctus[i][ctu] exactly in
 * vvcx_alf_decide's layout (luma_aps = {0} and chroma_aps = 0 refer to aps[i]).  flags = 0: vvcx_alf_decide's result on the same statistics (the per-CTU comparisons
 * read the device's exact errors, so this holds wherever none of them is a tie at double precision).  The flags add candidates; parity with the reference's RD choice
 * is unpinned, as for vvcx_alf_decide.
 * VVCX_ALF_NONLINEAR_LUMA / _CHROMA (4 bins must have been gathered, else VVCX_ERR_ARG): per filter group, from the linear solution with clipping index 0, a greedy
 *   search in the manner of AlfCovariance::optimizeFilter (EL 88-223): with step 2, then 1, per tap clip +- step on the gathered E[clip_k][clip_l][k][l], y[clip_k][k],
 *   re-solved; the best improving move is taken until none improves; then the rounding and single-step refinement of vvcx_alf_decide on the gathered matrix (kept only
 *   when it predicts less than the linear filter); then every index whose lower neighbour has identical rows, or whose coefficient is 0, is lowered (≙ reduceClipCost,
 *   EL 68-86).  The nonlinear flag is set only if an index stays non-zero and the gain pays for the clip bits: 2 bits per tap of every filter once the flag is on (this
 *   project's own count).  Merging keeps using bin 0 (the reference re-optimises the clips inside mergeClasses, EL 2344-2490).
 * VVCX_ALF_FIXED_SETS: per CTU the least of off, fixed set 0..15 (1 bin + 4 bypass bits, as codeAlfCtuFilterIndex writes them, EL/CABACWriter.cpp:4833-4892) and the new
 *   set (1 bin); the new set is derived once more from the CTUs that chose it and evaluated a last time; if its gain over the best choice without it does not pay for
 *   its parameter-set bits the slice carries no luma set (n_luma_aps = 0, CTU sets < 16).
 * With J = sum over CTUs (predicted error + lambda * bits) + lambda * parameter-set bits, the returned decision has by construction J <= J(all off), J <= J(the flags-0
 * decision) and, with VVCX_ALF_FIXED_SETS, J <= J(the best choice among off and the fixed sets): it is the least of these complete decisions and the new-set ones.
 * VVCX_ALF_CHROMA_ALTS(n), n = 1..8, OR-ed into flags: up to min(n, 2 * ctus) chroma alternatives (≙ the chroma loop of alfEncoder, EL 1041-1135; getMaxNumAlternativesChroma
 *   3849).  n = 1 (the value 0) is the decision described above, byte for byte; a handle without chroma ignores the field; luma is never touched.  For n >= 2, per frame:
 *   D1 = the one-alternative decision above with its cost J1 (0 when chroma stays off).  Then for K = min(n, 2 * ctus) down to 2: the CTUs start in K raster runs, the same
 *   for Cb and Cr (≙ initCtuAlternativeChroma, EL 3831-3847: label[a] = alt; if ((a + 1) * K >= (alt + 1) * ctus) ++alt), and two steps alternate:
 *     (a) re-derive: vvcx_alf_chroma_label_sums, then per alternative the quantised least-squares filter of its pooled Cb + Cr sums; with VVCX_ALF_NONLINEAR_CHROMA also the
 *         clip search on those sums, kept only where its predicted gain over the linear filter exceeds 12 clip bits at the mean chroma lambda (the nonlinear flag is per
 *         alternative).  An alternative no block carries keeps its previous filter (the zero filter at first);
 *     (b) assign: vvcx_alf_chroma_assign - per (CTU, component) the cheapest of off and the K alternatives.
 *   J_K = sum of the chosen costs + mean chroma lambda * (ue(K' - 1) + sum over the used alternatives (1 + coefficient bits + 12 when nonlinear)), K' = the alternatives
 *   still used; unused ones are dropped and the rest renumbered in ascending order, and the CTUs' alternative bits are then those of the final numbering.  The pair of
 *   steps is repeated while J falls, K + 1 times at most (2 (K + 1) of the reference's 2 (K + 1) + 1 half-steps, EL 1084); the least J_K seen is kept with its filters and
 *   labels.  The result is the least of J1 and the J_K, so J_chroma(n) <= J_chroma(1) <= 0 by construction.  It has chroma_aps = 0, 1 <= num_chroma_alt <= min(n, 2 * ctus),
 *   every alternative used by an enabled (CTU, component), alt[c] < num_chroma_alt and alt[c] = 0 where the flag is 0.  All frames of a call advance in the same device
 *   calls (a frame whose J stopped falling is carried along), so the number of blocking passes per call does not depend on the frame count: at most the sum over
 *   K = min(n, 2 * ctus) .. 2 of 2 (K + 1) (84 for K = 8) on top of the one-alternative decision's; the passes read the chroma statistics only.
 * Out of scope: parameter-set reuse across pictures, clip re-optimisation inside the class merge, parity with EncAdaptiveLoopFilter's RD choice. */
#define VVCX_ALF_NONLINEAR_LUMA   1
#define VVCX_ALF_NONLINEAR_CHROMA 2
#define VVCX_ALF_FIXED_SETS       4
#define VVCX_ALF_CHROMA_ALTS(n)   (((n) - 1) << 8)
int   vvcx_alf_decide_resident(vvcx_handle *h, const double lambda[3], int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slices, vvcx_alf_ctu *ctus,
                               void *hip_stream);
int   vvcx_last_alf_device_calls(const vvcx_handle *h);      /* blocking device passes of the handle's last vvcx_alf_decide_resident */
/* The two passes of the chroma-alternative iteration on the resident statistics (they need chroma: VVCX_ERR_STATE without it, and when nothing is resident or it is stale).
 * A label is an alternative 0 .. n_alts - 1 (n_alts = 1..8) or 255 = off; anything else is VVCX_ERR_ARG.
 * vvcx_alf_chroma_label_sums (≙ getFrameStats per alternative): labels[n][ctus][2] (Cb, Cr) -> sums[n][n_alts][size]: per frame and alternative the element-wise sum of
 *   the Cb and Cr blocks that carry its label (the two components are pooled); zeros for an alternative no block carries.
 * vvcx_alf_chroma_assign (≙ the alternative choice of deriveCtbAlfEnableFlags, EL 927-954): cands[n][n_alts]; per (frame, CTU, component c) and alternative a
 *     cost_a = (double) err_a / 16384. + lambda_c[c] * bits(a, n_alts),      bits(a, K) = 0 for K = 1, else min(a + 1, K - 1)
 *   with err_a exactly vvcx_alf_candidate_errors' chroma error and bits the truncated-unary length codeAlfCtuAlternative writes (one bit per bin, this project's own
 *   count); off costs 0.  The candidates are compared in the order off, 0, 1, .. with a strict <: the earliest wins a tie, off wins against a cost of exactly 0.  Product
 *   and sum are rounded separately (never fused).  labels[n][ctus][2] = the choice, err[n][ctus][2] = its err (0 when off), cost[n] = the chosen costs added by one lane
 *   in raster order, Cb before Cr - a float64 loop on the host gives the same bits.  Coefficients beyond +-128 and clipping indices >= the gathered bins are VVCX_ERR_ARG.
 * All arrays are host memory; the calls block.  vvcx_last_alf_sum_ms / _cand_ms report these kernels when they ran last.
 * vvcx_alf_chroma_alts_picture: the host-plane form (no handle, like vvcx_alf_evaluate_picture).  Either half may be NULL: labels_in -> sums; cands, lambda_c ->
 * labels_out, err, cost. */
int   vvcx_alf_chroma_label_sums(vvcx_handle *h, const uint8_t *labels, int n_alts, int64_t *sums, void *hip_stream);
int   vvcx_alf_chroma_assign(vvcx_handle *h, const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], uint8_t *labels, int64_t *err, double *cost,
                             void *hip_stream);
int   vvcx_alf_chroma_alts_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const uint8_t *labels_in,
                                   const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], int64_t *sums, uint8_t *labels_out, int64_t *err, double *cost,
                                   int device);
/* the host-plane forms (no handle; org / rec as for vvcx_alf_statistics_picture, chroma planes required): the planes are uploaded, the statistics gathered into temporary
 * device memory, and the same kernels and the same decision code run.  vvcx_alf_evaluate_picture: ctu_on[ctus][3] (may be NULL) -> luma_sum[25][size], chroma_sum[2][size];
 * the candidates -> luma_err[ctus][16 fixed_sets + n_luma], chroma_err[ctus][2][n_chroma] (either pair of outputs may be NULL).  Parity unpinned, as above. */
int   vvcx_alf_evaluate_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const uint8_t *ctu_on,
                                int fixed_sets, const vvcx_alf_luma_cand *luma_cands, int n_luma, const vvcx_alf_chroma_cand *chroma_cands, int n_chroma,
                                int64_t *luma_sum, int64_t *chroma_sum, int64_t *luma_err, int64_t *chroma_err, int device);
int   vvcx_alf_decide_picture(int pic_w, int pic_h, int bit_depth, int n_bins, const uint16_t *const org[3], const uint16_t *const rec[3], const double lambda[3],
                              int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slice, vvcx_alf_ctu *ctus, int device);
/* ≙ LoopFilter::loopFilterPic on a picture the caller describes itself (the way the reference's LoopFilter sees a CodingStructure: cs.cus + cs.tus + the reconstruction buffer):
 * rows = n_rows x {channel type (0 luma tree, 1 chroma tree), x, y, w, h in luma samples, cu.ispMode (0, 1 = horizontal, 2 = vertical split; luma rows only)} covering both
 * trees of the whole 4:2:0 picture, every CU intra at the slice QP (qp_cb / qp_cr = mapped chroma QPs); y / cb / cr = host planes of 16-bit samples, stride = plane width,
 * filtered in place.  The transform edges of ISP sub-partitions are filtered as xDeblockCU does (CL/LoopFilter.cpp:306-317, filter lengths from the sub-partition sizes,
 * 474-575).  Needs no handle: it is the filter of vvcx_deblock_bound_frames behind a table interface */
int  vvcx_deblock_cu_table(int pic_w, int pic_h, int bit_depth, int qp, int qp_cb, int qp_cr, int beta_offset_div2, int tc_offset_div2,
                           const int32_t *rows, int n_rows, uint16_t *y, uint16_t *cb, uint16_t *cr, int device);
/* slice_data() payload of one completely coded tile of a bound frame: the bytes EncSlice::encodeSlice would hand to the NAL writer
 * for that brick (CABACWriter::coding_tree_unit per CTU, end_of_ctu / end_of_slice terminating bins, byte alignment;
 * EL/EncSlice.cpp:1884-2006).  Requires cfg.emit_payload.  buf is host memory.  After the search the payload carries the coding trees only - no SAO / ALF CTU syntax, the
 * bytes of a slice whose header switches both filters off - until vvcx_rewrite_payload_bound_frames has written it again with the pictures' parameters */
int  vvcx_get_payload(vvcx_handle *h, int frame, int tile, uint8_t *buf, int cap, int *nbytes);
/* ≙ the CTU-level loop-filter syntax CABACWriter::coding_tree_unit (EL/CABACWriter.cpp:254-309) writes in front of every coding tree: sao() / sao_block_pars /
 * sao_offset_pars (323-462), codeAlfCtuEnableFlag (4700-4725), codeAlfCtuFilterIndex (4833-4892), codeAlfCtuAlternative (4920-4943).  The parameters exist only after the
 * whole picture is searched, deblocked and analysed, but their bins lie inside each tile's arithmetic codeword: this call writes every tile's payload of the bound pictures
 * a second time, from the CU tables and levels the search left on the device (what vvcx_get_cus / vvcx_get_levels return; no samples are read, so it may run before or
 * after the loop-filter calls), one workgroup per (frame, tile), none waiting on another.  vvcx_get_payload / vvcx_get_substream_sizes then return the new bytes and sizes.
 * Repeatable: a later call with other parameters, or with everything off (which gives the bytes of the search again), writes from the tables, never from earlier bytes.
 * hdr[frame] (≙ the slice header): slice_sao_luma_flag, slice_sao_chroma_flag, tile_group_alf_enabled_flag Y / Cb / Cr.  sao = prm[frame][ctu][3] as vvcx_sao_decide
 * returns them (may be NULL when no frame has SAO on); aps / slices / ctus as for vvcx_alf_bound_frames (slices, ctus NULL when no frame has ALF on; of a parameter set only
 * num_chroma_alt is read).  trace_ops_per_tile > 0 also keeps up to that many coder operations per tile for vvcx_get_payload_ops.
 * VVCX_ERR_STATE: no payload buffer (cfg.emit_payload), nothing bound, a CTU not coded yet.  VVCX_ERR_ARG, found on the host before anything is launched, for what the syntax
 * cannot carry: SAO mode outside 0..2, type outside 0..4 (merge: 0..1), band outside 0..31, |offset| above (1 << (min(bit_depth, 10) - 5)) - 1, an edge-offset CTU with
 * offset[0..1] < 0 or offset[2..3] > 0 (those signs are implicit), Cb and Cr of different mode or type (they share sao_type_idx_chroma and the edge class), a merge whose
 * candidate CTU lies outside the tile or the picture or that is not set on all three components, a component that is not off in a slice that disables it; an ALF luma set
 * outside 0..15 and 16..16 + n_luma_aps - 1, a chroma alternative >= num_chroma_alt of the slice's chroma set, a CTU flag of a component the slice disables.
 * When sao is given, the records of EVERY frame are checked, also of a frame whose slice has SAO off: such a frame must carry all-off records (mode 0); likewise the CTU
 * flags of a frame whose slice has ALF off must be 0 when ctus is given.  The work is enqueued on hip_stream, but the call BLOCKS until it has completed there (it
 * synchronises the stream before it returns: the host tables it uploads must outlive the copies).  The slice header and the parameter-set NAL units are the caller's. */
typedef struct vvcx_ctu_syntax { uint8_t sao_luma, sao_chroma, alf[3]; } vvcx_ctu_syntax;
int   vvcx_rewrite_payload_bound_frames(vvcx_handle *h, const vvcx_ctu_syntax *hdr, const vvcx_sao_param *sao, const vvcx_alf_aps *aps, int n_aps,
                                        const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int trace_ops_per_tile, void *hip_stream);
float vvcx_last_rewrite_ms(const vvcx_handle *h);
/* Diagnostic (it is what lets a test pin the rewritten bytes to the reference's BinEncoder_Std): the operation string the last rewrite coded for one tile, in the format of
 * vvcx_arith_encode - ops[i] = {kind, a, b}, context models as the reference's flat indices (the models of the SAO / ALF syntax included, which vvcx_arith_encode does not
 * keep).  With VVCX_TOOL_WPP the CTU rows of the tile follow one another; each ends with its terminating-bin operations ({2, 0, 0} behind every CTU but the last of the
 * picture, then {2, 1, 0}), so the rows can be split.  ops may be NULL (max_ops 0) to query the count.  VVCX_ERR_STATE without a traced rewrite; VVCX_ERR_ARG when the
 * tile coded more operations than the rewrite kept room for (*n_ops tells how many; the payload itself is complete all the same) or than max_ops. */
int   vvcx_get_payload_ops(vvcx_handle *h, int frame, int tile, int32_t *ops, int max_ops, int *n_ops);
/* ≙ the fork's GET_TRAINING_SET build (CL/TypeDef.h:54-56; EL/CABACWriter.cpp:515-855 writes the rows the forests of BIN/TEST.py are trained on): with a dump enabled every luma
 * node of the search that qualifies for the classifier (EL/EncCu.cpp:810-846, 933) leaves one row of 28 int32: the 26 features (EL/EncCu.cpp:863-1123), the complexity class
 * (0 simple, 1 fuzzy, 2 complex; 1127-1138) and the partition the full search chose at that node (0 none, 1 QT, 2 BT_H, 3 BT_V, 4 TT_H, 5 TT_V; -1: no encoding).  Rows
 * accumulate from vvcx_bind_frames on, in no particular order across streams; cap_rows 0 switches the dump off.  vvcx_get_training_rows copies min(rows so far, capacity,
 * max_rows) rows to host memory and reports in *n_rows how many the search produced.  Works with and without VVCX_TOOL_FAST (without: the plain full search labels the rows,
 * which is how a forest is trained: tools/train_partition_forest.py).  VVCX_ERR_UNSUPPORTED on a VVCX_TOOL_WPP handle (the features read neighbour CUs of other CTU rows,
 * whose progress under WPP is a matter of timing - the reason vvcx_create refuses VVCX_TOOL_FAST with WPP) */
int  vvcx_enable_training_dump(vvcx_handle *h, int cap_rows);
int  vvcx_get_training_rows(vvcx_handle *h, int32_t *rows, int max_rows, int *n_rows);
/* the sub-streams inside the bytes vvcx_get_payload returns for a tile, in order: one (the tile), or with VVCX_TOOL_WPP one per CTU row of the tile - what the slice header's
 * entry points are made of (EL/EncSlice.cpp:1982-1990 addSubstreamSize).  sizes may be NULL to query the count */
int  vvcx_get_substream_sizes(vvcx_handle *h, int frame, int tile, int *sizes, int max_sizes, int *n_sizes);
/* Diagnostic environment variables (read by vvcx_create / at launch; they never change a result):
 *   VVCX_MAX_WG_PER_CU=n          at most n resident CTU streams per CU (the rate-against-occupancy curve of DESIGN.md §6)
 *   VVCX_WPP_TEST_INTERLEAVE=1    VVCX_TOOL_WPP: one CTU per visit and round-robin choice of the next CTU row, so that the rows of a picture take turns */
/* device time of the last compress launch, measured with HIP events on the launch stream (ms) */
float vvcx_last_kernel_ms(const vvcx_handle *h);
/* work counters of the last launch: [0] SATD-stage candidates, [1] full-RD TU evaluations, [2] RD pixels, [3] nodes */
int  vvcx_get_counters(vvcx_handle *h, uint64_t out[4]);
/* diagnostic (only filled by a -DVVCX_STAMP=1 build): shader-clock ticks summed over streams of the last launch:
 * [0] mode controller, [1..11] parallel operation kinds, [12] estimator pass, [16..27] controller phases, [30] steps */
int  vvcx_get_profile(vvcx_handle *h, uint64_t out[48]);
const char *vvcx_last_error(void);
int  vvcx_ctus_per_frame(const vvcx_handle *h);
/* number of CTU streams the device runs concurrently (CUs x resident workgroups per CU); batches with at least this
 * many (frame, tile) streams fill the GPU.  ≙ the worker-thread count a frame-parallel host loop would size for */
int  vvcx_resident_streams(const vvcx_handle *h);


/* ---- leaf operators: the device functions of the path, individually callable.  They stand where the
 * reference has its run-time seams — RdCost::m_afpDistortFunc[DF_*] (CL/RdCost.h:60,104) — and its CommonLib entry points
 * IntraPrediction::initIntraPatternChType + predIntraAng (CL/IntraPrediction.cpp:304,1064), BinProbModel_Std
 * (CL/Contexts.h:86-155), RdCost::calcRdCost (CL/RdCost.cpp:63), the scan tables (CL/Rom.cpp:133-370).  Test and
 * diagnostic entry points: all pointers are HOST memory, the work runs on the device the handle / call selects.  Like every entry point
 * of this header they leave the calling thread's current HIP device as they found it (the LMCS analysis runs on that device). */
/* SAD, SATD (RdCost::xGetHADs tiling and normalisation) and SSE of n pairs of w x h blocks stored back to back; out[n][3] */
int  vvcx_distortion_batch(const int16_t *a, const int16_t *b, int w, int h, int n, uint64_t *out, int device);
/* intra prediction of n blocks of one picture: reco = planar 4:2:0 samples of the handle's size and bit depth (uint8 / uint16),
 * coded[2] = one byte per 4x4 luma unit (uw x uh, 1 = already reconstructed) for the luma and the chroma tree.
 * x, y, w, h in samples of the component; mode 0..66, mrl 0/1/3 (luma); for comp 1 / 2 also mode 67 / 68 / 69 (LM, MDLM_L, MDLM_T: the co-located luma of reco[0]
 * down-sampled, line parameters from the neighbours the chroma-tree map allows; blocks 4x2 .. 32x32 at even x, y).  pred: concatenated w*h tiles */
typedef struct { int32_t comp, x, y, w, h, mode, mrl; } vvcx_pred_case;
int  vvcx_intra_pred_batch(vvcx_handle *h, const void *const reco[3], const uint8_t *const coded[2], const vvcx_pred_case *cases, int n, int16_t *pred);
/* CtxStore initialisation of an I slice (CL/Contexts.cpp:135-151) and the estimator's model update over a bin string */
int  vvcx_ctx_init(int qp, uint16_t s0[386], uint16_t s1[386]);
int  vvcx_cabac_code_bins(uint16_t *s0, uint16_t *s1, int ctx, const uint8_t *bins, int nbins, uint64_t *frac_bits, int device);
/* RdCost::calcRdCost for n (fracBits, dist) pairs at one lambda */
int  vvcx_rd_cost_batch(double lambda, const uint64_t *frac_bits, const uint64_t *dist, int n, double *cost, int device);
/* the core of IntraSearch::xIntraCodingTUBlock (EL/IntraSearch.cpp:2852-3168) for n blocks: residual org - pred → TrQuant::transformNxN
 * (DCT-II, plain Quant::quant) → levels; if any: invTransformNxN → rec = clip(pred + residual'); SSE(org, rec).  qp is the QP QpParam
 * hands to the quantiser (slice QP + QpBDOffset, chroma after the mapping table) */
int  vvcx_transform_quant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int n,
                                int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device);
/* the same block pipeline with the dependent quantiser (≙ DepQuant::quant / dequant, CL/DepQuant.cpp:1755-1810, with the slice's dep_quant_enabled_flag on):
 * comp 0 Y / 1 Cb / 2 Cr; mts_idx 0 or 2..5 (luma, up to 32x32); cbf_cb = tu.cbf[Cb] when Cr is quantised; lambda = the quantiser's lambda of the
 * component (TrQuant::selectLambda); s0 / s1 = the two states of each of the 386 context models the rate terms are read from */
int  vvcx_depquant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int comp, int mts_idx, int cbf_cb, double lambda,
                         const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device);
/* the same with the LFNST of a CU with lfnstIdx 1 / 2 between the (zeroed-out) DCT-II and the dependent quantiser and back (≙ TrQuant::xFwdLfnst / xInvLfnst,
 * CL/TrQuant.cpp:319-560; blocks below 4x4 take none): intra_dir = the block's final intra mode (0..66; planar for a MIP CU, the co-located luma
 * mode for DM / CCLM chroma), from which the kernel set and the transposition follow after the wide-angle mapping of the block shape */
int  vvcx_lfnst_depquant_batch(const int16_t *org, const int16_t *pred, int w, int h, int bit_depth, int qp, int comp, int lfnst_idx, int intra_dir, int cbf_cb, double lambda,
                               const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device);
/* the trellis alone on n luma coefficient blocks (w x h each, 4..32 per side, int16 as the forward transforms leave them) quantised side by side by one wavefront
 * against one set of context models, as the full-RD rounds of the search quantise the candidates of a node: lev = the levels, abs_sum[i] = DepQuant::quant's absSum of
 * block i.  *max_items (may be NULL) receives the most blocks one wavefront takes for the shape (at most 16); n beyond it is VVCX_ERR_ARG */
int  vvcx_depquant_items(const int16_t *coef, int w, int h, int bit_depth, int qp, double lambda, const uint16_t *s0, const uint16_t *s1, int n,
                         int16_t *lev, int32_t *abs_sum, int *max_items, int device);
/* transform skip of n luma residual blocks (4..32 per side; VVCX_TOOL_TS): ≙ the {DCT2, TS} pruning of TrQuant::transformNxN (CL/TrQuant.cpp:1049-1124; keep = the
 * transform-skip candidate survives), xTransformSkip 1394-1440, QuantRDOQ::xRateDistOptQuantTS (CL/QuantRDOQ.cpp:1243-1483, reached through DepQuant::quant for
 * MTS_SKIP blocks) with rates from the context models s0 / s1 and the quantiser's lambda, Quant::dequant + xITransformSkip 996-1041 (resi_out), and the fractional
 * bits CABACWriter::residual_codingTS (EL/CABACWriter.cpp:4306-4555) spends on the levels.  qp = slice QP + QpBDOffset (the TS minimum QP 4 is applied inside). */
int  vvcx_transform_skip_batch(const int16_t *resi, int w, int h, int bit_depth, int qp, double lambda, const uint16_t *s0, const uint16_t *s1, int n,
                               int16_t *lev, int16_t *resi_out, int32_t *abs_sum, uint8_t *keep, uint64_t *frac_bits, int device);
/* the block pipeline of n luma TUs of tw x th samples (1 x N, 2 x N, N x 1, N x 2 or larger; at least 16 samples) of CUs coded with intra sub-partitions (VVCX_TOOL_ISP): ≙
 * TrQuant::transformNxN with the implicit DST-VII / DCT-II choice of ISP blocks (getTrTypes, CL/TrQuant.cpp:752-780) and the one-stage transforms of one-sample-wide
 * blocks (895-914, 970-983), DepQuant::quant with the cbf context of ISP sub-partitions (prev_cbf = the previous sub-partition's cbf; cbf_inferred: the last
 * sub-partition after all-zero ones, EL/CABACWriter.cpp:3574-3600), dequantisation, inverse, reconstruction over pred; qp = slice QP + QpBDOffset */
int  vvcx_isp_tu_batch(const int16_t *org, const int16_t *pred, int tw, int th, int bit_depth, int qp, double lambda, int prev_cbf, int cbf_inferred,
                       const uint16_t *s0, const uint16_t *s1, int n, int16_t *lev, int16_t *rec, uint64_t *sse, uint8_t *cbf, int device);
/* residual coding of n blocks of w x h levels (back to back, stride w; every block with at least one level, none in the area the block's transform zeroes): ≙
 * CABACWriter::residual_coding (EL/CABACWriter.cpp:3773-3883, last_sig_coeff 4102-4160, residual_coding_subblock 4164-4304) or, for mts_idx 1, residual_codingTS
 * (4306-4555).  Every block starts from the same states s0 / s1 of the 386 context models.  comp 0 luma / 1 chroma; tools: VVCX_TOOL_DEPQUANT runs the quantiser's state
 * machine (context set of sig_coeff_flag, zero position of the bypass pass); ts_allowed / mts_allowed = TU::isTSAllowed / TU::isMTSAllowed of the block (luma up to
 * 32 x 32, not in an ISP CU); mts_idx = tu.mtsIdx: 0, 1 (transform skip, sides 4..32) or 2..5 (a 32-point side then codes 16).  The path holds this syntax in four
 * forms, which must agree:
 *   form 0  the single-lane estimator of the controller (mts_idx 1: the single-lane residual_codingTS)
 *   form 1  the lane-parallel estimator on levels staged in the wave's LDS slot (blocks of at most 256 levels, not mts_idx 1)
 *   form 2  the lane-parallel estimator on levels in device memory (not mts_idx 1)
 *   form 3  the writer: a fresh arithmetic coder, mts_coding (3885-3941) of a luma block as the final pass writes it, the levels, a terminating bin of 1, finish and
 *           byte alignment; block i's bytes at bytes + i * bytes_cap, their count in nbytes[i]
 * Out per block: the fractional bits (2^-15; forms 0..2 the levels alone, form 3 including the transform indices), the end states of all 386 models
 * (s0_out / s1_out [n][386]), rc_last = the last significant scan position (-1 for mts_idx 1).  bytes / nbytes may be null for forms 0..2. */
int  vvcx_residual_coding_batch(const int16_t *lev, int w, int h, int n, int comp, uint32_t tools, int ts_allowed, int mts_allowed, int mts_idx,
                                const uint16_t *s0, const uint16_t *s1, int form, uint64_t *frac_bits, uint16_t *s0_out, uint16_t *s1_out, int32_t *rc_last,
                                uint8_t *bytes, int bytes_cap, int32_t *nbytes, int device);
/* the arithmetic coder (≙ BinEncoder_Std, EL/BinEncoder.cpp:106-420) over an operation string, from the I-slice context models at qp: ops[i] = {kind, a, b}:
 * kind 0 = bin b on context model a (the reference's flat index; a model the library keeps), 1 = b bypass bins (1..32) of value a, MSB first, 2 = terminating bin a.
 * Ends with finish and byte alignment; the bytes go to out (room for cap), their count to nbytes */
int  vvcx_arith_encode(int qp, const int32_t *ops, int nops, uint8_t *out, int cap, int *nbytes, int device);
/* coefficient scan (diagonal, grouped) of a w x h block: idx[min(w,32) * min(h,32)] raster offsets in scan order */
int  vvcx_scan_order(int w, int h, uint16_t *idx, int device);
/* ≙ BIN/TEST.py GetPartition(C0..C25, 2): the forest of vvcx_set_forest on n rows of 26 int32 features (host pointers) → class per row */
/* ≙ IntraPrediction::initIntraMip + predIntraMip (CL/IntraPrediction.cpp:2152-2205; MatrixIntraPrediction, JVET_O0925 form) for n luma
 * blocks: cases = n x {w, h, mode, bit_depth}; refs = per case top[w] | left[h] (unfiltered line-0 reference samples); pred = per case w*h.
 * The search uses the same device functions for its MIP candidates (VVCX_TOOL_MIP); this entry point exposes them for the parity test. */
int  vvcx_mip_pred_batch(const int32_t *cases, int n, const int16_t *refs, int n_refs, int16_t *pred, int n_pred, int device);
int  vvcx_forest_predict_batch(vvcx_handle *h, const int32_t *rows, int n, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
