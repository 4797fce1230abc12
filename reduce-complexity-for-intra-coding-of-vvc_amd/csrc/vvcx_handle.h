// vvcx_handle.h — what the host translation units behind the C-ABI (vvcx_api*.hip, vvcx_sao_rd.hip, vvcx_alf_derive.hip) share: the handle, how an entry point reports
// an error, and the few functions of the core file the others call.  Host only: nothing here is seen by a kernel.
#pragma once
#include <stdint.h>
#include <vector>
#include "vvcx.h"
#include "vvcx_dev.h"
#include "vvcx_host.h"        // DevBuf, ON_DEVICE / DevGuard, HIPCHK

// what crosses translation units inside the library and is no part of its interface
#define VVCX_INTERNAL __attribute__((visibility("hidden")))

// vvcx_api.hip: sets what vvcx_last_error returns (printf form of vvcx_fail_msg_); returns `code`
VVCX_INTERNAL int fail(int code, const char *fmt, ...);
// vvcx_api.hip: the quantiser constants of a block shape; the start states of the context models the library keeps (s0 / s1[VXD_NUM_CTX])
VVCX_INTERNAL VxDqConst dq_consts_of(int lsum, int bit_depth, int qp, double lambda);
VVCX_INTERNAL void ctx_init_islice(int qp, uint16_t *s0, uint16_t *s1);

// device buffers of the ALF decision passes (vvcx_alf_eval.hip): frame sums, error tables, the CTU mask and the candidates of a call
struct AlfWork {
  DevBuf<long long> sum_l, sum_c, err_l, err_c; DevBuf<uint8_t> mask; DevBuf<VxAlfLumaCand> lc; DevBuf<VxAlfChromaCand> cc;
  DevBuf<uint8_t> lab; DevBuf<long long> lab_sum, alt_err; DevBuf<double> alt_term, alt_cost;      // the chroma-alternative passes: labels, sums per label, chosen errors, cost terms, frame costs
};
// device buffers of the SAO decision kernels (vvcx_sao_decide.hip): candidate records, the coded parameters, the estimator's bit table
struct SaoWork { DevBuf<VxSaoCand> cand; DevBuf<VxSaoSyn> syn; DevBuf<uint32_t> frac; };

struct vvcx_handle {
  vvcx_cfg cfg; vvcx_slice sl; bool have_slice;
  int ctus_w, ctus_h, uw, uh, ntiles;
  std::vector<int> ctu_tile;                    // tile of each CTU (raster address)
  std::vector<std::vector<int>> tile_ctus;      // CTUs of each tile in coding (raster-in-tile) order
  int n_frames;
  std::vector<VxFrameDev> frames_h;
  // sub-streams: the units the search runs as independent (or, under WPP, lagged) sequences of CTUs and the arithmetic coder writes as one byte string each - a tile, or
  // with VVCX_TOOL_WPP one CTU row of a tile (EL/EncSlice.cpp:1972-1990).  Per frame: nsub of them, numbered tile by tile, row by row
  int nsub;
  std::vector<int> ctu_sub, sub_tile, sub_above, tile_sub0, tile_nsub;      // sub-stream of each CTU; its tile; the sub-stream of the CTU row above in the same tile (-1: none); per tile: first sub-stream, count
  std::vector<std::vector<int>> sub_ctus;       // CTUs of each sub-stream in coding order
  DevBuf<int32_t> train_rows_d; DevBuf<uint32_t> train_n_d; int train_cap;      // vvcx_enable_training_dump: rows of 28 values, how many were asked for, room for train_cap rows
  DevBuf<int32_t> wpp_sched_d; int wpp_rr;      // the launch's WPP scheduler state (vvcx_kernel.hip run_streams_wpp); test mode (env VVCX_WPP_TEST_INTERLEAVE)
  DevBuf<int32_t> wpp_progress_d; DevBuf<uint16_t> wpp_sync_d;  // WPP: CTUs finished per (frame, sub-stream); the contexts behind the first CTU of each (m_entropyCodingSyncContextState)
  std::vector<int> next_idx;                    // per (frame, sub-stream): how many CTUs of the stream are done
  // device memory: every *_d member owns its block (vvcx_host.h) and is freed with the handle
  DevBuf<VxFrameDev> frames_d; DevBuf<int16_t> lev_d; DevBuf<VxUnit> units_d; DevBuf<uint16_t> stream_ctx_d;
  DevBuf<uint8_t> scratch_d;
  DevBuf<VxStreamDesc> streams_d; DevBuf<int32_t> task_ctu_d; DevBuf<VxCtuRes> results_d;
  DevBuf<unsigned long long> counters_d;
  // optional slice_data writer: payload bytes per (frame, tile), byte ranges, persistent arithmetic-coder state
  DevBuf<uint8_t> payload_d; DevBuf<uint64_t> payload_off_d; DevBuf<uint32_t> payload_cap_d; DevBuf<uint8_t> arith_d; std::vector<uint64_t> payload_off; std::vector<uint32_t> payload_cap;
  // FAST_ALGORITHM forest (vvcx_set_forest)
  DevBuf<VxForestNode> f_node_d; DevBuf<double> f_value_d; DevBuf<int32_t> f_root_d; int f_ntrees, f_nclasses; int32_t f_classes[8];
  DevBuf<VxDqConst> dq_d;                           // dependent-quantiser constants per (chroma scale table, component, log2 w + log2 h)
  // LMCS of the current slice (vvcx_set_slice): LUTs and tables, their device copy (fwd | inv), the forward-mapped original luma of the bound pictures
  bool lmcs_on, lmcs_inverted; int16_t lmcs_fwd[1024], lmcs_inv[1024]; int32_t lmcs_pivot[17], lmcs_cadj[16];
  DevBuf<int16_t> lmcs_lut_d; DevBuf<uint8_t> lmcs_org_d;
  std::vector<uint32_t> activity;               // per (frame, CTU) of the bound pictures: orders the stream queue of a launch, longest first
  hipEvent_t ev0, ev1; float last_ms, last_deblock_ms, last_sao_ms;
  DevBuf<uint8_t> sao_tmp_d; DevBuf<VxSaoEntry> sao_tab_d; DevBuf<uint8_t> sao_tile_d;      // vvcx_sao_bound_frames: picture copy, resolved parameters, CTU -> tile
  DevBuf<uint8_t> db_edges_d;      // vvcx_deblock_bound_frames: one edge byte per unit, map and direction
  DevBuf<long long> sao_stat_d; float last_sao_stats_ms;      // vvcx_sao_statistics_bound_frames
  // vvcx_sao_decide_resident: sao_tab_d / sao_tile_d hold the decision of the bound pictures (for vvcx_sao_bound_frames_resident) while no call has touched the
  // pictures or these buffers since; the decision kernels' buffers; on an LMCS slice the frame records whose org[0] is the caller's own (unmapped) luma
  bool sao_res_valid; int sao_res_lf; SaoWork sao_work; hipEvent_t ev2; float last_sao_decide_ms;
  DevBuf<VxFrameDev> frames_org_d;
  DevBuf<VxAlfFrame> alf_tab_d; DevBuf<VxAlfCtu> alf_ctu_d; float last_alf_ms;      // vvcx_alf_bound_frames: per-frame tables and per-CTU choices (the picture copy is the SAO one)
  DevBuf<long long> alf_stat_luma_d, alf_stat_chroma_d; float last_alf_stats_ms;      // vvcx_alf_statistics_bound_frames
  // vvcx_alf_statistics_resident: what alf_stat_*_d hold (frame range, bins, chroma) while no call has touched the pictures since; the decision passes' buffers
  bool alf_res_valid, alf_res_chroma; int alf_res_first, alf_res_n, alf_res_bins; AlfWork alf_work; float last_alf_sum_ms, last_alf_cand_ms; int last_alf_calls;
  // vvcx_rewrite_payload_bound_frames: per-frame header flags, coded SAO parameters, ALF choices, the tile / sub-stream tables, start states, per-workgroup sync states,
  // walk scratch and operation trace; the host copy of the last trace counts
  DevBuf<VxCtuSynFrame> rw_hdr_d; DevBuf<VxSaoSyn> rw_sao_d; DevBuf<VxAlfCtu> rw_alf_d; DevBuf<uint8_t> rw_scratch_d; DevBuf<int32_t> rw_tab_d, rw_trace_d;
  DevBuf<uint16_t> rw_ctx_d; DevBuf<uint32_t> rw_trace_n_d; std::vector<uint32_t> rw_trace_n; int rw_trace_cap; float last_rewrite_ms;
  // a submitted, not yet collected launch (vvcx_submit_ctus .. vvcx_wait_ctus): staging the async copies read from / write to stays alive here
  bool pending; hipStream_t pend_stream; int pend_n; VxCtuRes *pend_res; int pend_cap;
  std::vector<VxStreamDesc> pend_sd; std::vector<int32_t> pend_task_ctu; std::vector<int> pend_src, pend_next; VxDqConst pend_dq[17 * 96];
  size_t lev_plane[3], lev_frame, units_plane, units_frame;
};

// entry points that touch a handle's device state refuse to run between vvcx_submit_ctus and vvcx_wait_ctus
#define NOT_PENDING(h) do { if ((h) && (h)->pending) return fail(VVCX_ERR_STATE, "a submitted launch is outstanding: call vvcx_wait_ctus first"); } while (0)
// vvcx_api.hip: VVCX_OK, or the VVCX_ERR_STATE of `what` when a CTU of the bound pictures is not coded yet
VVCX_INTERNAL int require_all_coded(const vvcx_handle *h, const char *what);
