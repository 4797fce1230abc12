// vvcx_sao_rd.h — the parameter records and the bit estimator of the SAO decision: vvcx_sao_rd.hip prices its candidates with them on the host, the device decision
// (vvcx_api_loopfilter.hip -> vvcx_sao_decide.hip) starts from the estimator's two context models.  Host only.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include "vvcx_dev.h"
#include "vvcx_tables.h"                 // context init values and rates in the reference's flat order, the bin cost table
#include "vvcx_ctu_syntax_tables.h"      // VX_CTX_REF_SaoMergeFlag

namespace {
struct SaoSet { int mode = 0, type = 0, band = 0; int off[32] = { 0 }; };      // one component of one CTU: off / new / merge; offsets by class (coded or reconstructed)
struct SaoCtu { SaoSet c[3]; };
// the bit estimator of the SAO syntax (sao_block_pars / sao_offset_pars, EL/CABACWriter.cpp:354-462): models SaoMergeFlag and SaoTypeIdx, everything else bypass
class SaoRate {
public:
  void init(int qp)
  {
    for (int k = 0; k < 2; k++) {
      const int id = VX_CTX_INIT_I_REF[kFirst + k], slope = (id >> 3) - 4, offset = ((id & 7) * 18) + 1;
      int st = ((slope * ((qp < 0 ? 0 : qp > 63 ? 63 : qp) - 16)) >> 1) + offset;
      st = st < 1 ? 1 : st > 127 ? 127 : st;
      s0_[k] = (uint16_t) ((st << 8) & 0x7FE0); s1_[k] = (uint16_t) ((st << 8) & 0x7FFE);
    }
    bits = 0;
  }
  uint64_t bits = 0;
  void block(const SaoCtu &u, int bd, bool leftAvail, bool aboveAvail, bool mergeFlagsOnly)
  {
    bool left = false, above = false;
    if (leftAvail) { left = u.c[0].mode == 2 && u.c[0].type == 0; coded(0, left); }
    if (aboveAvail && !left) { above = u.c[0].mode == 2 && u.c[0].type == 1; coded(0, above); }
    if (mergeFlagsOnly || left || above) return;
    for (int k = 0; k < 3; k++) component(u.c[k], k, bd);
  }
  void component(const SaoSet &p, int comp, int bd)
  {
    const bool first = comp < 2;                       // Y and Cb carry the type of their channel
    if (first) { coded(1, p.mode != 0); if (p.mode != 0) bypass(1); }
    if (p.mode != 1) return;
    const int mx = max_q(bd);
    int o[4];
    for (int i = 0; i < 4; i++) o[i] = p.off[p.type == 4 ? (p.band + i) & 31 : (i < 2 ? i : i + 1)];
    for (int i = 0; i < 4; i++) { const int a = std::abs(o[i]); if (mx) bypass(a < mx ? a + 1 : mx); }      // truncated unary
    if (p.type == 4) { for (int i = 0; i < 4; i++) if (o[i]) bypass(1); bypass(5); }
    else if (first) bypass(2);
  }
  static int max_q(int bd) { return (1 << (std::min(bd, 10) - 5)) - 1; }      // SampleAdaptiveOffset::getMaxOffsetQVal
  // the two models as the device form of this estimator (vvcx_sao_decide.hip) starts from them: states, adaptation shifts
  void export_models(VxSaoDecideParams &p) const
  {
    for (int k = 0; k < 2; k++) {
      const int rate = VX_CTX_RATE_REF[kFirst + k];
      p.s0[k] = s0_[k]; p.s1[k] = s1_[k]; p.r0[k] = 2 + ((rate >> 2) & 3); p.r1[k] = 3 + p.r0[k] + (rate & 3);
    }
  }
private:
  static const int kFirst = VX_CTX_REF_SaoMergeFlag;    // Ctx::SaoMergeFlag in the reference's flat order (ContextSetCfg); SaoTypeIdx follows
  uint16_t s0_[2], s1_[2];
  void bypass(int n) { bits += (uint64_t) n << 15; }
  void coded(int which, bool bin)
  {
    const unsigned st = (unsigned) (s0_[which] + s1_[which]) >> 8;
    bits += VX_BIN_FRAC_BITS[st * 2 + (bin ? 1 : 0)];
    const int rate = VX_CTX_RATE_REF[kFirst + which], r0 = 2 + ((rate >> 2) & 3), r1 = 3 + r0 + (rate & 3);
    s0_[which] -= (s0_[which] >> r0) & 0x7FE0; s1_[which] -= (s1_[which] >> r1) & 0x7FFE;
    if (bin) { s0_[which] += (0x7fffu >> r0) & 0x7FE0; s1_[which] += (0x7fffu >> r1) & 0x7FFE; }
  }
};
}      // namespace
