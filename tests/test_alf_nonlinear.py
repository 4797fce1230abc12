"""The ALF decision from statistics that stay in device memory (csrc/vvcx_alf_eval.hip: masked frame sums and per-CTU candidate errors) with nonlinear filters and the
fixed filter sets (vvcx_alf_decide_resident / _picture).  The expected sums and errors are Python integers computed from statistics that test_alf_encoder.py pins to
the reference-pinned filter; the decision is checked for what it must reach on constructed pictures and for the invariants of its cost
J = sum over CTUs (predicted error + lambda * bits) + lambda * parameter-set bits, recomputed here from the statistics.  Parity with the reference's RD choice is unpinned."""
import functools
import os
import re
import numpy as np
import pytest
import oracle_lib as O
import test_alf_encoder as T
from test_alf_encoder import picture, stat_parts, all_on_params, decision_picture, _coded_pair, KNOWN_LUMA, KNOWN_CHROMA, emu_so  # noqa: F401 (emu_so: the fixture; T.reference = model_stats on classes_of)

ROOT = T.ROOT
pkg, vv = T.pkg, T.vv
NL = vv.ALF_NONLINEAR_LUMA | vv.ALF_NONLINEAR_CHROMA
ALL = NL | vv.ALF_FIXED_SETS


@functools.lru_cache(maxsize=None)
def fixed_tables():
    """the standard's 64 fixed filters and the filter of each (fixed set, class): the oracle's tables, which the pinned filter reads"""
    txt = open(os.path.join(ROOT, "oracle", "orc_alf_tables.h")).read()
    a, b = txt.index("ORC_ALF_FIXED[64][12]"), txt.index("ORC_ALF_CLASS_TO_FIXED[16][25]")
    num = lambda s: [int(v) for v in re.findall(r"-?\d+", s[s.index("=") + 1:])]
    return np.array(num(txt[a:b])[:64 * 12]).reshape(64, 12), np.array(num(txt[b:])[:16 * 25]).reshape(16, 25)


def filter_err(blk, nb, nc, q, clip):
    """sum q_k q_l E[clip_k][clip_l][k][l] - 256 sum q_k y[clip_k][k] of one block of statistics, as a Python integer"""
    E, y, _ = stat_parts(blk, nb, nc)
    n = nc - 1
    q = np.array([int(v) for v in q], object); c = np.asarray(clip, np.int64); i = np.arange(n)
    Eg = E[c[:, None], c[None, :], i[:, None], i[None, :]].astype(object); yg = y[c, i].astype(object)
    return int((np.outer(q, q) * Eg).sum()) - 256 * int((q * yg).sum())


def luma_err(ctu_blocks, nb, cand):
    return sum(filter_err(ctu_blocks[cl], nb, 13, cand["coeff"][cl], cand["clip_idx"][cl]) for cl in range(25))


def fixed_cand(s):
    fx, c2f = fixed_tables()
    cd = np.zeros((), vv.ALF_LUMA_CAND); cd["coeff"] = fx[c2f[s]]
    return cd


def model_errors(luma, chroma, nb, fixed_sets, lcands, ccands):
    """[ctus][candidate] / [ctus][2][candidate] lists of Python integers"""
    cands = ([fixed_cand(s) for s in range(16)] if fixed_sets else []) + list(lcands)
    el = [[luma_err(luma[a], nb, cd) for cd in cands] for a in range(luma.shape[0])]
    ec = [[[filter_err(chroma[a, c], nb, 7, cd["coeff"], cd["clip_idx"]) for cd in ccands] for c in range(2)] for a in range(chroma.shape[0])]
    return el, ec


def candidates_for(w, h, nb):
    """a seeded 25-filter set with random clipping indices (index 0 on 1-bin statistics), every coefficient 127, every coefficient -128; the same for chroma"""
    row = pkg.alf_test_params(31, w, h)["aps"][0].copy()
    row[26] = nb == 4; row[628] = nb == 4
    lc = np.zeros(3, vv.ALF_LUMA_CAND); cc = np.zeros(3, vv.ALF_CHROMA_CAND)
    lc[0] = vv.alf_luma_cand(row); cc[0] = vv.alf_chroma_cand(row)
    lc[1]["coeff"] = 127; lc[2]["coeff"] = -128; cc[1]["coeff"] = 127; cc[2]["coeff"] = -128
    return lc, cc


def masked_sums(luma, chroma, on):
    return (luma * on[:, 0, None, None].astype(np.int64)).sum(0), (chroma * on[:, 1:3, None].astype(np.int64)).sum(0)


def check_passes(name, nb, lib_path, masks):
    org, rec, bd = picture(name)
    h, w = rec[0].shape
    luma, chroma = T.reference(name, nb)
    nctu = luma.shape[0]
    lc, cc = candidates_for(w, h, nb)
    sl, sc, el, ec = vv.alf_evaluate_picture(org, rec, bd, nb, fixed_sets=True, luma_cands=lc, chroma_cands=cc, lib_path=lib_path)
    assert np.array_equal(sl, luma.sum(0)) and np.array_equal(sc, chroma.sum(0))
    ml, mc = model_errors(luma, chroma, nb, True, lc, cc)
    assert el.shape == (nctu, 19) and el.tolist() == ml, (name, nb)
    assert ec.shape == (nctu, 2, 3) and ec.tolist() == mc, (name, nb)
    for kind in masks:
        on = np.zeros((nctu, 3), np.uint8)
        if kind == "one":
            on[nctu - 1] = (1, 0, 1)
        sl, sc, el, ec = vv.alf_evaluate_picture(org, rec, bd, nb, ctu_on=on, lib_path=lib_path)
        xl, xc = masked_sums(luma, chroma, on)
        assert el is None and ec is None and np.array_equal(sl, xl) and np.array_equal(sc, xc), (name, nb, kind)
    return ml


# ---------------------------------------------------------------- 1: the two passes against the integer model
@pytest.mark.parametrize("name,nb,masks", [("P1", 4, ("none", "one")), ("P2", 4, ("one",)), ("P3", 1, ("none",))])
def test_sums_and_errors_on_the_emulator_equal_the_integer_model(emu_so, name, nb, masks):
    ml = check_passes(name, nb, emu_so, masks)
    if name == "P3":
        assert max(abs(v) for r in ml for v in r) > 1 << 53          # a double would not hold this error exactly


def test_pass_argument_errors_are_status_codes(emu_so):
    org, rec, bd = picture("P2")
    lc, cc = candidates_for(136, 72, 1)
    for bad in ("coeff", "clip", "bins", "count", "nothing"):
        l2, kw = lc.copy(), dict(n_bins=1, luma_cands=lc, chroma_cands=cc)
        if bad == "coeff":
            l2[0]["coeff"][3, 2] = 129; kw["luma_cands"] = l2
        elif bad == "clip":
            l2[0]["clip_idx"][24, 11] = 1; kw["luma_cands"] = l2                # 1 bin gathered
        elif bad == "bins":
            kw["n_bins"] = 2
        elif bad == "count":
            kw.update(luma_cands=np.zeros(49, vv.ALF_LUMA_CAND), fixed_sets=True)      # 16 + 49 > 64
        else:
            kw.update(luma_cands=None, chroma_cands=None, want_sums=False)
        with pytest.raises(pkg.VvcxError, match="error -1"):
            vv.alf_evaluate_picture(org, rec, bd, lib_path=emu_so, **kw)
    c2 = cc.copy(); c2[1]["coeff"][0] = -129
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_evaluate_picture(org, rec, bd, 1, chroma_cands=c2, lib_path=emu_so)
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_decide_picture(org, rec, bd, [1.0] * 3, n_bins=1, flags=vv.ALF_NONLINEAR_LUMA, lib_path=emu_so)      # the clip search needs 4 bins
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_decide_picture(org, rec, bd, [1.0] * 3, n_bins=4, flags=8, lib_path=emu_so)


# ---------------------------------------------------------------- 2 + 3: the resident route on bound pictures
def same_decision(a, b):
    return np.array_equal(a["aps"], b["aps"]) and a["luma_aps"] == b["luma_aps"] and a["chroma_aps"] == b["chroma_aps"] and np.array_equal(a["ctu"], b["ctu"])


def round0_margins(luma, chroma, w, h, bd, lam, nb, lib_path):
    """|d_on + lambda - d_off| of every CTU against the filters vvcx_alf_decide derives from all CTUs: a one-CTU picture whose statistics are the frame sums gets exactly
    those filters back (both of its rounds see the same sums)"""
    prm = vv.alf_decide(luma.sum(0)[None], chroma.sum(0)[None], 128, 128, bd, [lam] * 3, n_bins=nb, lib_path=lib_path)
    assert prm["ctu"][0, :3].tolist() == [1, 1, 1]
    lcd, ccd = vv.alf_luma_cand(prm["aps"][0]), vv.alf_chroma_cand(prm["aps"][0])
    el, ec = model_errors(luma, chroma, nb, False, [lcd], [ccd])
    return [abs(e[0] / 16384.0 + lam) for e in el] + [abs(e[c][0] / 16384.0) for e in ec for c in range(2)]


def check_resident(lib_path, to_dev, to_host):
    enc, frames, recs = _coded_pair(lib_path, to_dev, to_host)
    nctu = enc.ctus_per_frame
    for call in (enc.alf_frame_statistics, enc.alf_candidate_errors, lambda: enc.alf_decide_resident([8.0] * 3)):
        with pytest.raises(pkg.VvcxError, match="error -4"):
            call()                                             # nothing resident yet
    luma, chroma, _ = enc.alf_statistics_bound_frames(0, 2, 4)
    enc.alf_statistics_resident(0, 2, 4)
    sl, sc = enc.alf_frame_statistics()
    assert np.array_equal(sl, luma.sum(1)) and np.array_equal(sc, chroma.sum(1))
    on = np.zeros((2, nctu, 3), np.uint8); on[0, 0] = (1, 1, 0); on[1, 1] = (0, 1, 1); on[1, 0, 0] = 1
    sl, sc = enc.alf_frame_statistics(on)
    for f in range(2):
        xl, xc = masked_sums(luma[f], chroma[f], on[f])
        assert np.array_equal(sl[f], xl) and np.array_equal(sc[f], xc)
    lc = np.zeros((2, 2), vv.ALF_LUMA_CAND); cc = np.zeros((2, 1), vv.ALF_CHROMA_CAND)
    for f in range(2):
        c3, c1 = candidates_for(136, 72, 4)
        lc[f, 0] = c3[0]; lc[f, 1]["coeff"] = 127 - 255 * f; cc[f, 0] = c1[0]
        lc[f, 0]["coeff"][:, f] += 1                           # the frames' candidates differ
    el, ec = enc.alf_candidate_errors(True, lc, cc)
    for f in range(2):
        ml, mc = model_errors(luma[f], chroma[f], 4, True, lc[f], cc[f])
        assert el[f].tolist() == ml and ec[f].tolist() == mc, f
    # flags 0 is vvcx_alf_decide on the downloaded statistics, wherever no comparison is close to a tie
    lam = 8.0
    res = enc.alf_decide_resident([lam] * 3)
    for f in range(2):
        assert min(round0_margins(luma[f], chroma[f], 136, 72, 8, lam, 4, lib_path)) > 1
        assert same_decision(res[f], vv.alf_decide(luma[f], chroma[f], 136, 72, 8, [lam] * 3, n_bins=4, lib_path=lib_path)), f
    # 1-bin statistics: clipping indices of 4-bin candidates are refused, as is the clip search
    one, _, _ = enc.alf_statistics_bound_frames(1, 1, 1)
    enc.alf_statistics_resident(1, 1, 1)
    assert np.array_equal(enc.alf_frame_statistics()[0], one.sum(1))
    with pytest.raises(pkg.VvcxError, match="error -1"):
        enc.alf_candidate_errors(False, lc[1:, :1], None)
    with pytest.raises(pkg.VvcxError, match="error -1"):
        enc.alf_decide_resident([lam] * 3, flags=NL)
    assert same_decision(enc.alf_decide_resident([lam] * 3)[0], vv.alf_decide(one[0], enc.alf_statistics_bound_frames(1, 1, 1)[1][0], 136, 72, 8, [lam] * 3, lib_path=lib_path))
    # anything that touches the pictures makes the statistics stale
    enc.alf_statistics_resident(0, 2, 1)
    enc.alf_bound_frames([all_on_params(136, 72, KNOWN_LUMA, KNOWN_CHROMA)] * 2)
    for call in (enc.alf_frame_statistics, lambda: enc.alf_candidate_errors(True), lambda: enc.alf_decide_resident([lam] * 3)):
        with pytest.raises(pkg.VvcxError, match="error -4"):
            call()
    enc.close()


def test_resident_route_on_the_emulator(emu_so):
    check_resident(emu_so, lambda a: (a, a.ctypes.data), lambda a: a)


def test_flags_0_is_the_decision_from_downloaded_statistics(emu_so):
    org, rec, bd = decision_picture(256, 128, left_equal=True)
    luma, chroma = vv.alf_statistics_picture(org, rec, bd, 1, lib_path=emu_so)
    assert min(round0_margins(luma, chroma, 256, 128, bd, 8.0, 1, emu_so)[:2]) > 1      # luma; chroma of the left CTU is an exact tie (org == rec), which both sides see as 0 < 0
    want = vv.alf_decide(luma, chroma, 256, 128, bd, [8.0] * 3, lib_path=emu_so)
    got = vv.alf_decide_picture(org, rec, bd, [8.0] * 3, lib_path=emu_so)
    assert same_decision(got, want) and got["ctu"][:, :3].tolist() == [[0, 0, 0], [1, 1, 1]]


# ---------------------------------------------------------------- the cost J of a decision, from the statistics
def ue_bits(v):
    return 2 * int(v + 1).bit_length() - 1


def coeff_bits(q):
    return sum(ue_bits(abs(int(c))) + (c != 0) for c in q)


def decision_cost(prm, luma, chroma, nb, lam):
    """(J luma, J chroma, predicted luma error of the enabled CTUs) of a decision relative to everything off, in units of squared error; the bits as include/vvcx.h counts them"""
    a = prm["aps"][0]
    jl = jc = 0.0
    pred = 0.0
    new = vv.alf_luma_cand(a)
    for i, u in enumerate(prm["ctu"]):
        if u[0]:
            e = luma_err(luma[i], nb, new if u[3] == 16 else fixed_cand(u[3])) / 16384.0
            jl += e + lam * (1 if u[3] == 16 else 5)
            pred += e + sum(int(luma[i, cl, -1]) for cl in range(25))
        for c in range(2):
            if u[1 + c]:
                jc += filter_err(chroma[i, c], nb, 7, a[636:642], a[684:690] if a[628] else [0] * 6) / 16384.0
    if (prm["ctu"][:, 0] != 0).any() and (prm["ctu"][prm["ctu"][:, 0] != 0, 3] == 16).any():
        n = int(a[0])
        jl += lam * (1 + ue_bits(n - 1) + (25 * (n - 1).bit_length() if n > 1 else 0) + sum(coeff_bits(a[27 + 12 * g:39 + 12 * g]) for g in range(n)) + (24 * n if a[26] else 0))
    if prm["chroma_aps"] >= 0:
        jc += lam * (1 + ue_bits(0) + coeff_bits(a[636:642]) + (12 if a[628] else 0))
    return jl, jc, pred


def fixed_only_cost(luma, nb, lam):
    return sum(min([0.0] + [luma_err(luma[i], nb, fixed_cand(s)) / 16384.0 + 5 * lam for s in range(16)]) for i in range(luma.shape[0]))


# ---------------------------------------------------------------- 4: fixed sets
@functools.lru_cache(maxsize=None)
def fixed_set_picture():
    _, rec, bd = decision_picture(256, 128)
    prm = dict(aps=np.zeros((1, pkg.ALF_APS_INTS), np.int32), luma_aps=[], chroma_aps=0, ctu=np.array([[1, 0, 0, 3, 0, 0], [1, 0, 0, 11, 0, 0]], np.int32))
    prm["aps"][0, 0] = 1
    org = [p.astype(np.uint16) for p in O.alf_picture(rec, 256, 128, bd, prm)]
    assert org[0].min() > 0 and org[0].max() < 1023
    return org, rec, bd


def test_fixed_sets_are_found_where_they_made_the_picture(emu_so):
    org, rec, bd = fixed_set_picture()
    lam = 256.0
    luma, chroma = vv.alf_statistics_picture(org, rec, bd, 1, lib_path=emu_so)
    errs = [[luma_err(luma[a], 1, fixed_cand(s)) / 16384.0 for s in range(16)] for a in range(2)]
    print("fixed-set errors", [sorted(e)[:2] for e in errs])
    resid = 0.0
    for a, s, best, second in ((0, 3, -595028, -525775), (1, 11, -18689, -7818)):
        order = np.argsort(errs[a])
        assert order[0] == s and abs(errs[a][s] - best) < 1 and abs(errs[a][order[1]] - second) < 1, (a, errs[a])
        resid += errs[a][s] + sum(int(luma[a, cl, -1]) for cl in range(25))
    least_bits = 1 + ue_bits(0) + 11 * ue_bits(0) + ue_bits(1) + 1          # a parameter set with one filter and one coefficient of +-1
    print("residual %.1f, lambda * least bits %.1f" % (resid, lam * least_bits))
    assert 0 <= resid < 2600 < lam * least_bits
    assert min(second - best for _, _, best, second in ((0, 3, -595028, -525775), (1, 11, -18689, -7818))) > resid      # no new set can beat the fixed choice by its bits
    prm = vv.alf_decide_picture(org, rec, bd, [lam] * 3, flags=vv.ALF_FIXED_SETS, lib_path=emu_so)
    assert prm["ctu"][:, 3].tolist() == [3, 11] and prm["ctu"][:, 0].tolist() == [1, 1] and prm["luma_aps"] == []
    out = O.alf_picture(rec, 256, 128, bd, prm)
    assert all(np.array_equal(o.astype(np.int64), g.astype(np.int64)) for o, g in zip(out, org))
    jl, jc, _ = decision_cost(prm, luma, chroma, 1, lam)
    j0 = decision_cost(vv.alf_decide_picture(org, rec, bd, [lam] * 3, lib_path=emu_so), luma, chroma, 1, lam)
    assert jl <= min(0.0, j0[0], fixed_only_cost(luma, 1, lam)) + 1e-6 and jc <= min(0.0, j0[1]) + 1e-6


# ---------------------------------------------------------------- 5: nonlinear filters
@functools.lru_cache(maxsize=None)
def nonlinear_picture():
    _, rec, bd = decision_picture(256, 128)
    org = [p.astype(np.uint16) for p in O.alf_picture(rec, 256, 128, bd, all_on_params(256, 128, KNOWN_LUMA, KNOWN_CHROMA, clip=2))]
    assert all(p.min() > 0 and p.max() < 1023 for p in org)          # nothing clamps
    return org, rec, bd


def check_nonlinear(lib_path, filter_fn, lams):
    org, rec, bd = nonlinear_picture()
    luma, chroma = vv.alf_statistics_picture(org, rec, bd, 4, lib_path=lib_path)
    gen = all_on_params(256, 128, KNOWN_LUMA, KNOWN_CHROMA, clip=2)
    e_gen = decision_cost(gen, luma, chroma, 4, 0.0)[2]
    floor = 0.0                                                   # what the best real-valued LINEAR filters, one per class, leave
    for cl in range(25):
        E, y, pix = stat_parts(luma[:, cl].sum(0), 4, 13)
        E12, y12 = E[0, 0, :12, :12].astype(np.float64), y[0, :12].astype(np.float64)
        c = np.linalg.lstsq(E12, y12, rcond=None)[0]
        floor += pix - 2 * c @ y12 + c @ E12 @ c
    print("generating filter predicts %.1f, per-class linear floor %.1f" % (e_gen, floor))
    assert e_gen < 0.1 * floor
    for lam in lams:
        prm = vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=4, flags=NL, lib_path=lib_path)
        a = prm["aps"][0]
        jl, jc, pred = decision_cost(prm, luma, chroma, 4, lam)
        j0 = decision_cost(vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=4, lib_path=lib_path), luma, chroma, 4, lam)
        full = vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=4, flags=ALL, lib_path=lib_path)
        jf = decision_cost(full, luma, chroma, 4, lam)
        print("lambda %g: J luma %.1f (flags 0: %.1f, all flags: %.1f), J chroma %.1f (flags 0: %.1f), predicted %.1f" % (lam, jl, j0[0], jf[0], jc, j0[1], pred))
        assert jl <= min(0.0, j0[0]) + 1e-6 and jc <= min(0.0, j0[1]) + 1e-6
        assert jf[0] <= min(0.0, j0[0], fixed_only_cost(luma, 4, lam)) + 1e-6 and jf[1] <= min(0.0, j0[1]) + 1e-6
        assert a[327:627].max() <= 3 and a[684:732].max() <= 3
        if lam == 0:
            assert a[26] == 1 and a[327:627].max() > 0 and prm["luma_aps"] == [0] and prm["ctu"][:, 0].all() and pred < floor, (pred, floor)
            filtered = filter_fn(rec, 256, 128, bd, prm)
            n = org[0].size
            act = int(((org[0].astype(np.int64) - np.asarray(filtered[0]).astype(np.int64)) ** 2).sum())
            print("luma: predicted %.1f actual %d samples %d" % (pred, act, n))
            assert abs(act - pred) <= np.sqrt(n * max(pred, 0.0)) + n / 4, (pred, act)


def test_clip_search_beats_every_linear_filter(emu_so):
    check_nonlinear(emu_so, lambda rec, w, h, bd, prm: O.alf_picture(rec, w, h, bd, prm), (0.0, 8.0))


# ---------------------------------------------------------------- 6: clipping that cannot act
def test_inert_clipping_leaves_the_linear_decision(emu_so):
    bd = 10
    tex = pkg.alf_test_frame(256, 128, bd, 21)
    rec = [(512 + (p.astype(np.int64) & 3)).astype(np.uint16) for p in tex]          # every difference is below the smallest clipping value (6 luma, 4 chroma)
    org = [p.astype(np.uint16) for p in O.alf_picture(rec, 256, 128, bd, all_on_params(256, 128, (0, 0, 0, 0, 0, 0, 40, 0, 0, 0, 0, 40), (0, 0, 30, 0, 0, 30)))]
    luma, chroma = vv.alf_statistics_picture(org, rec, bd, 4, lib_path=emu_so)
    for blk, nc in ((luma, 13), (chroma, 7)):
        ne = 16 * nc * nc
        E = blk[..., :ne].reshape(blk.shape[:2] + (16, nc * nc)); y = blk[..., ne:ne + 4 * nc].reshape(blk.shape[:2] + (4, nc))
        assert (E == E[..., :1, :]).all() and (y == y[..., :1, :]).all()                # all bins identical
    lin = vv.alf_decide_picture(org, rec, bd, [0.0] * 3, n_bins=4, lib_path=emu_so)
    got = vv.alf_decide_picture(org, rec, bd, [0.0] * 3, n_bins=4, flags=NL, lib_path=emu_so)
    assert lin["ctu"][:, :3].any()
    assert same_decision(got, lin) and got["aps"][0, 26] == 0 and not got["aps"][0, 628:636].any()


# ---------------------------------------------------------------- on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name,nb,masks", [("P1", 4, ("none", "one")), ("P3", 1, ("none",))])
def test_sums_and_errors_on_the_gpu_equal_the_integer_model(name, nb, masks):
    check_passes(name, nb, None, masks)


@pytest.mark.gpu
def test_resident_route_on_the_gpu():
    import torch

    def to_dev(a):
        t = torch.from_numpy(a).cuda()
        return t, t.data_ptr()
    check_resident(None, to_dev, lambda t: t.cpu().numpy())


@pytest.mark.gpu
def test_clip_search_on_the_gpu_predicts_the_device_filter():
    check_nonlinear(None, lambda rec, w, h, bd, prm: vv.alf_picture(rec, bd, prm), (0.0,))
