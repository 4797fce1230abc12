// vvcx_alf_derive.h — what the ALF entry points (vvcx_api_loopfilter.hip) and the ALF host numeric code (vvcx_alf_derive.hip) call of each other.  Host only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "vvcx.h"
#include "vvcx_handle.h"      // AlfWork, VVCX_INTERNAL

// int64 values of one (CTU, class) / (CTU, component) block of the encoder statistics: E | y | pixAcc for nb clipping bins and nc coefficients
static inline size_t alf_stat_size(int nb, int nc) { return (size_t) nb * nb * nc * nc + (size_t) nb * nc + 1; }

// statistics of n frames in device memory (chroma NULL: none) and where the passes put their results; ev0 / ev1 (optional) time the kernel of the last call
// calls: the blocking device passes made through this record
struct AlfRes { const long long *luma, *chroma; int n, nctu, nb; AlfWork *w; hipStream_t stream; hipEvent_t ev0, ev1; float sum_ms, cand_ms; int calls; };

// vvcx_alf_derive.hip
VVCX_INTERNAL int alf_clip_value(int chroma, int bit_depth, int idx);
VVCX_INTERNAL int alf_build(const vvcx_alf_aps *aps, int n_aps, const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int n_frames, int nctu, int bit_depth, int chroma, std::vector<VxAlfFrame> &tabs);
VVCX_INTERNAL void alf_ctus(const vvcx_alf_slice *slices, const vvcx_alf_ctu *ctus, int n_frames, int nctu, int chroma, std::vector<VxAlfCtu> &out);
VVCX_INTERNAL int alf_decide_frames(AlfRes &r, bool chroma, const double lambda[3], int max_luma_filters, int flags, vvcx_alf_aps *aps, vvcx_alf_slice *slices, vvcx_alf_ctu *ctus);
// vvcx_api_loopfilter.hip: the device passes of the decision (vvcx_alf_eval.hip)
VVCX_INTERNAL int alf_sums(AlfRes &r, const uint8_t *ctu_on, int64_t *luma, int64_t *chroma);
VVCX_INTERNAL int alf_errors(AlfRes &r, int fixed_sets, const vvcx_alf_luma_cand *lc, int n_luma, const vvcx_alf_chroma_cand *cc, int n_chroma, int64_t *luma_err, int64_t *chroma_err);
// the chroma-alternative passes: labels [n][ctus][2] (0 .. n_alts - 1, or 255 = off) -> sums [n][n_alts][size_c]; cands [n][n_alts] -> labels, err [n][ctus][2], cost [n]
VVCX_INTERNAL int alf_label_sums(AlfRes &r, const uint8_t *labels, int n_alts, int64_t *sums);
VVCX_INTERNAL int alf_assign(AlfRes &r, const vvcx_alf_chroma_cand *cands, int n_alts, const double lambda_c[2], uint8_t *labels, int64_t *err, double *cost);
