// vvcx_kernels.h — the kernels of the library as its host translation units launch them (defined in vvcx_kernel.hip, vvcx_deblock.hip, vvcx_mip.hip, vvcx_lmcs.hip,
// vvcx_sao*.hip, vvcx_alf*.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vvcx_dev.h"

extern "C" __global__ void vvcx_compress_kernel_u8(VxParams p);
extern "C" __global__ void vvcx_compress_kernel_u16(VxParams p);
extern "C" __global__ void vvcx_compress_wpp_kernel_u8(VxParams p);
extern "C" __global__ void vvcx_compress_wpp_kernel_u16(VxParams p);
extern "C" __global__ void vvcx_rewrite_kernel_u8(VxParams p, VxRewriteParams r);
extern "C" __global__ void vvcx_rewrite_kernel_u16(VxParams p, VxRewriteParams r);
extern "C" __global__ void vvcx_leaf_dist_kernel(const int16_t *a, const int16_t *b, int w, int h, int16_t *scr, unsigned long long *out);
extern "C" __global__ void vvcx_leaf_pred_kernel_u8(VxParams p, const VxLeafPred *cases, int16_t *out, const int *out_off);
extern "C" __global__ void vvcx_leaf_pred_kernel_u16(VxParams p, const VxLeafPred *cases, int16_t *out, const int *out_off);
extern "C" __global__ void vvcx_leaf_cabac_kernel(uint16_t *io, int ctx, const uint8_t *bins, int nbins, unsigned long long *bits);
extern "C" __global__ void vvcx_leaf_rdcost_kernel(VxParams p, const unsigned long long *bits, const unsigned long long *dist, int n, double *cost);
extern "C" __global__ void vvcx_leaf_scan_kernel(int w, int h, uint16_t *idx);
extern "C" __global__ void vvcx_leaf_forest_kernel(VxParams p, const int32_t *rows, int n, int32_t *out);
extern "C" __global__ void vvcx_leaf_rc_kernel(VxParams p, const uint16_t *ctx, const int16_t *lev, int w, int h, int ch, int mts, int form, uint16_t *scan, uint16_t *ctx_out,
                                               unsigned long long *out, uint8_t *bytes, uint32_t cap, uint32_t *nbytes);
extern "C" __global__ void vvcx_leaf_arith_kernel(const uint16_t *ctx, const int32_t *ops, int nops, uint8_t *bytes, uint32_t cap, uint32_t *nbytes);
struct VxMipCase { int32_t w, h, mode, bit_depth, ref_off, pred_off; };
extern "C" __global__ void vvcx_leaf_mip_kernel(const VxMipCase *cases, const int16_t *refs, int16_t *preds);
extern "C" __global__ void vvcx_sao_copy_kernel_u8(VxSaoParams p);
extern "C" __global__ void vvcx_sao_copy_kernel_u16(VxSaoParams p);
extern "C" __global__ void vvcx_sao_kernel_u8(VxSaoParams p);
extern "C" __global__ void vvcx_sao_kernel_u16(VxSaoParams p);
extern "C" __global__ void vvcx_sao_stats_kernel_u8(VxSaoStatParams p);
extern "C" __global__ void vvcx_sao_stats_kernel_u16(VxSaoStatParams p);
extern "C" __global__ void vvcx_sao_cand_kernel(VxSaoDecideParams p);
extern "C" __global__ void vvcx_sao_chain_kernel(VxSaoDecideParams p);
extern "C" __global__ void vvcx_alf_copy_kernel_u8(VxAlfParams p);
extern "C" __global__ void vvcx_alf_copy_kernel_u16(VxAlfParams p);
extern "C" __global__ void vvcx_alf_kernel_u8(VxAlfParams p);
extern "C" __global__ void vvcx_alf_kernel_u16(VxAlfParams p);
extern "C" __global__ void vvcx_alf_stats_b1_kernel_u8(VxAlfStatParams p);
extern "C" __global__ void vvcx_alf_stats_b4_kernel_u8(VxAlfStatParams p);
extern "C" __global__ void vvcx_alf_stats_b1_kernel_u16(VxAlfStatParams p);
extern "C" __global__ void vvcx_alf_stats_b4_kernel_u16(VxAlfStatParams p);
extern "C" __global__ void vvcx_alf_sum_kernel(VxAlfSumParams p);
extern "C" __global__ void vvcx_alf_cand_kernel(VxAlfCandParams p);
extern "C" __global__ void vvcx_alf_chroma_label_sum_kernel(VxAlfLabelSumParams p);
extern "C" __global__ void vvcx_alf_chroma_assign_kernel(VxAlfAssignParams p);
extern "C" __global__ void vvcx_alf_chroma_cost_kernel(VxAlfAssignParams p);
extern "C" __global__ void vvcx_deblock_edges_kernel(VxDeblockParams p);
extern "C" __global__ void vvcx_deblock_kernel_u8(VxDeblockParams p);
extern "C" __global__ void vvcx_deblock_kernel_u16(VxDeblockParams p);
extern "C" __global__ void vvcx_jccr_sign_kernel_u8(VxFrameDev *frames, int wc, int hc);
extern "C" __global__ void vvcx_jccr_sign_kernel_u16(VxFrameDev *frames, int wc, int hc);
extern "C" __global__ void vvcx_leaf_dq_items_kernel(VxParams p, const uint16_t *ctx, int16_t *coef, uint8_t *nodes, int n, int w, int h, int *out);
extern "C" __global__ void vvcx_leaf_dq_kernel(VxParams p, const uint16_t *ctx, const int16_t *org, int16_t *rec, int16_t *lev, int32_t *tmp, int w, int h, int qp, int comp, int mts, int cbf_cb, unsigned long long *out, int lf, int lfdir);
extern "C" __global__ void vvcx_leaf_ts_kernel(VxParams p, const uint16_t *ctx, const int16_t *resi, int16_t *lev, int16_t *resi_out, int32_t *tmp, int w, int h, int qp, int *out, unsigned long long *bits);
extern "C" __global__ void vvcx_lmcs_map_kernel_u8(const uint8_t *src, uint8_t *dst, int w, int h, int stride, const int16_t *lut);
extern "C" __global__ void vvcx_lmcs_map_kernel_u16(const uint16_t *src, uint16_t *dst, int w, int h, int stride, const int16_t *lut);
extern "C" __global__ void vvcx_leaf_isp_kernel(VxParams p, const uint16_t *ctx, const int16_t *org, int16_t *rec, int16_t *lev, int32_t *tmp, int w, int h, int qp, int cbf_ctx, unsigned long long *out);
extern "C" __global__ void vvcx_ctu_activity_kernel_u8(const VxFrameDev *frames, int pic_w, int pic_h, int ctus_w, unsigned *out);
extern "C" __global__ void vvcx_ctu_activity_kernel_u16(const VxFrameDev *frames, int pic_w, int pic_h, int ctus_w, unsigned *out);
extern "C" __global__ void vvcx_leaf_trq_kernel(const int16_t *org, int16_t *rec, int16_t *lev, int32_t *tmp, int w, int h, int bd, int qp, unsigned long long *out);
