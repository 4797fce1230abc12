"""Several chroma alternatives in the ALF decision (VVCX_ALF_CHROMA_ALTS of vvcx_alf_decide_resident / _picture) and the two device passes behind it
(csrc/vvcx_alf_eval.hip: vvcx_alf_chroma_label_sum_kernel, vvcx_alf_chroma_assign_kernel).  The passes are compared exactly with numpy / Python-integer models of their
definition in include/vvcx.h on statistics that test_alf_encoder.py pins; the decision is checked for what it must reach on a picture made with three planted
alternatives and for the invariants of its cost, recomputed here from the statistics with the header's bit count.  Parity with the reference's RD choice is unpinned."""
import functools
import numpy as np
import pytest
import oracle_lib as O
import test_alf_encoder as T
from test_alf_encoder import all_on_params, decision_picture, _coded_pair, KNOWN_LUMA, KNOWN_CHROMA, emu_so  # noqa: F401 (emu_so: the fixture)
from test_alf_nonlinear import filter_err, same_decision, ue_bits, coeff_bits, nonlinear_picture

pkg, vv = T.pkg, T.vv
OFF = vv.ALF_LABEL_OFF
ALTS = vv.ALF_CHROMA_ALTS
PLANTED = ((-3, 5, 10, 5, -4, 11), (6, -8, -12, 9, 14, -20), (0, 0, 25, 0, 0, -18))
PLANTED_CB, PLANTED_CR = (0, 1, 2, 2, 0, 1), (1, 2, 0, 1, 2, 0)


# ---------------------------------------------------------------- pictures and their statistics (one gather per library and bin count, shared by the tests)
@functools.lru_cache(maxsize=None)
def six_ctu_picture():
    """384 x 256, 10 bit: 3 x 2 CTUs, so the label pass runs one group of four blocks' loads three times; org == rec in the left CTU column"""
    return decision_picture(384, 256, left_equal=True)


@functools.lru_cache(maxsize=None)
def six_ctu_stats(lib_path, nb):
    org, rec, bd = six_ctu_picture()
    return vv.alf_statistics_picture(org, rec, bd, nb, lib_path=lib_path)[1]


@functools.lru_cache(maxsize=None)
def planted_picture():
    """rec = decision_picture's texture; org = the pinned filter's output with three linear chroma alternatives spread over the 12 (CTU, component) blocks"""
    _, rec, bd = decision_picture(384, 256)
    prm = all_on_params(384, 256, KNOWN_LUMA)
    a = prm["aps"][0]
    a[627] = 3; a[628:636] = 0
    for t, q in enumerate(PLANTED):
        a[636 + 6 * t:642 + 6 * t] = q
    prm["ctu"][:, 4] = PLANTED_CB; prm["ctu"][:, 5] = PLANTED_CR
    org = [p.astype(np.uint16) for p in O.alf_picture(rec, 384, 256, bd, prm)]
    return org, rec, bd, prm


def cand(q, clip=None):
    cd = np.zeros((), vv.ALF_CHROMA_CAND)
    cd["coeff"] = q
    if clip is not None:
        cd["clip_idx"] = clip
    return cd


def cands_of(*cds):
    out = np.zeros(len(cds), vv.ALF_CHROMA_CAND)
    for i, c in enumerate(cds):
        out[i] = c
    return out


# ---------------------------------------------------------------- the models
def alt_bits(a, k):
    return 0 if k == 1 else min(a + 1, k - 1)


def model_label_sums(chroma, labels, n_alts):
    flat, lab = chroma.reshape(-1, chroma.shape[-1]), np.asarray(labels).ravel()
    return np.stack([flat[lab == a].sum(0) for a in range(n_alts)])


def model_errs(chroma, nb, cds):
    """[ctu][component][alternative] Python integers: what vvcx_alf_candidate_errors defines"""
    return [[[filter_err(chroma[a, c], nb, 7, cd["coeff"], cd["clip_idx"]) for cd in cds] for c in range(2)] for a in range(chroma.shape[0])]


def model_assign(errs, lam_c, n_alts):
    """labels, err, cost of include/vvcx.h in float64, in its order: off, 0, 1, .. with a strict <; the frame's cost added in raster order, Cb before Cr"""
    nctu = len(errs)
    lab = np.full((nctu, 2), OFF, np.uint8); err = np.zeros((nctu, 2), np.int64)
    cost = 0.0
    for a in range(nctu):
        for c in range(2):
            best = 0.0
            for s in range(n_alts):
                v = float(errs[a][c][s]) / 16384.0 + float(lam_c[c]) * float(alt_bits(s, n_alts))
                if v < best:
                    best, lab[a, c], err[a, c] = v, s, errs[a][c][s]
            cost = cost + best
    return lab, err, cost


# ---------------------------------------------------------------- 1: label sums
def label_sets(nctu):
    eight = np.array([0, 1, 2, 3, 4, 5, 6, 7, OFF, 7, OFF, 0], np.uint8).reshape(nctu, 2)          # all eight values, two blocks off
    split = np.zeros((nctu, 2), np.uint8); split[2] = (1, 0); split[5] = (0, 1)                      # Cb and Cr of one CTU in different alternatives
    gap = np.array([0, 2, 2, 0, OFF, 2, 0, 0, 2, 2, 0, OFF], np.uint8).reshape(nctu, 2)            # alternative 1 unused
    return [(eight, 8), (split, 2), (gap, 3), (np.full((nctu, 2), OFF, np.uint8), 2), (np.zeros((nctu, 2), np.uint8), 1)]


def check_label_sums(lib_path):
    org, rec, bd = six_ctu_picture()
    for nb in (1, 4):
        chroma = six_ctu_stats(lib_path, nb)
        assert chroma.shape[0] == 6
        for labels, k in label_sets(6):
            got = vv.alf_chroma_alts_picture(org, rec, bd, nb, labels=labels, n_alts=k, lib_path=lib_path)[0]
            want = model_label_sums(chroma, labels, k)
            assert got.shape == want.shape and np.array_equal(got, want), (nb, k, np.argwhere(got != want)[:4])
            if k == 3:
                assert not got[1].any() and got[0].any() and got[2].any()                            # an alternative nobody uses gives zeros
            if (labels == OFF).all():
                assert not got.any()
        sc = vv.alf_evaluate_picture(org, rec, bd, nb, lib_path=lib_path)[1]                         # vvcx_alf_frame_statistics' pass
        assert np.array_equal(got[0], sc[0] + sc[1])


def test_label_sums_on_the_emulator_equal_the_integer_model(emu_so):
    check_label_sums(emu_so)


# ---------------------------------------------------------------- 2: assignment
def assign_candidates(nb):
    """a neighbour of KNOWN_CHROMA, KNOWN_CHROMA itself (what made the picture), a seeded filter, the neighbour once more, then seeded filters; at 4 bins the third is
    KNOWN_CHROMA with mixed clipping indices (so that three alternatives already gather other bins) and three more have seeded indices"""
    near = list(KNOWN_CHROMA); near[2] += 1
    g = np.random.default_rng(5)
    cds = [cand(near), cand(KNOWN_CHROMA), cand(g.integers(-40, 41, 6)), cand(near)] + [cand(g.integers(-40, 41, 6)) for _ in range(4)]
    if nb == 4:
        cds[2]["coeff"] = KNOWN_CHROMA; cds[2]["clip_idx"] = (0, 1, 2, 3, 3, 0)
        for cd in cds[4:7]:
            cd["clip_idx"] = g.integers(0, 4, 6)
    return cands_of(*cds)


def check_assign(lib_path):
    org, rec, bd = six_ctu_picture()
    for nb in (1, 4):
        chroma = six_ctu_stats(lib_path, nb)
        all_cd = assign_candidates(nb)
        errs8 = model_errs(chroma, nb, all_cd)
        assert all(e >= 0 for a in (0, 3) for c in range(2) for e in errs8[a][c])                   # org == rec there: no filter gains
        assert all(errs8[a][c][1] < 0 for a in (1, 2, 4, 5) for c in range(2))
        # a lambda at which the bits decide: where KNOWN_CHROMA (alternative 1: 2 bits among 3 or more) predicts a little less than its neighbour (alternative 0: 1 bit),
        # the neighbour wins once lambda exceeds the gap; twice the least gap puts one block at least on the other side
        gaps = [(errs8[a][c][0] - errs8[a][c][1]) / 16384.0 for a in range(6) for c in range(2) if errs8[a][c][1] < errs8[a][c][0] < 0]
        assert gaps, nb
        lams = [(0.0, 0.0), (50.0, 70.0), (2 * min(gaps), 2 * min(gaps))]
        decided = False
        for k in (1, 2, 3, 8):
            cds = all_cd[:k]
            errs = [[e[:k] for e in row] for row in errs8]
            # On the GPU every lambda runs with every count at both bin counts.  On the emulator only 1 bin covers that product: at 4 bins each call gathers the
            # statistics again, which takes seconds there, so the emulator runs all three lambdas at 3 alternatives only, lambda (0, 0) at 1 and (50, 70) at 2 and 8.
            # The emulator therefore does NOT check the duplicate candidate (index 3 against 0) with mixed clipping indices at any lambda but (50, 70); the GPU test does.
            for lam_c in (lams if lib_path is None or nb == 1 or k == 3 else lams[:1] if k == 1 else lams[1:2]):
                _, lab, err, cost = vv.alf_chroma_alts_picture(org, rec, bd, nb, cands=cds, lambda_c=lam_c, lib_path=lib_path)
                mlab, merr, mcost = model_assign(errs, lam_c, k)
                print("bins %d alternatives %d lambda %s: labels %s cost %r" % (nb, k, lam_c, lab.ravel().tolist(), cost))
                assert np.array_equal(lab, mlab) and np.array_equal(err, merr) and cost == mcost, (nb, k, lam_c, lab.tolist(), mlab.tolist(), cost, mcost)
                assert (lab[[0, 3]] == OFF).all() and not (lab == 3).any()                           # off wins a cost of 0; the earlier of two equal candidates wins
                if k == 3 and lam_c == lams[-1]:
                    lab0 = model_assign(errs, (0.0, 0.0), k)[0]
                    decided = bool(((lab0 == 1) & (mlab == 0)).any())
            if k == 1:
                ec = vv.alf_evaluate_picture(org, rec, bd, nb, chroma_cands=cds, want_sums=False, lib_path=lib_path)[3]
                lab = model_assign(errs, (0.0, 0.0), 1)[0]                                            # == the library's at lambda 0, compared above
                assert np.array_equal(lab == 0, ec[:, :, 0] < 0) and np.array_equal(lab == OFF, ec[:, :, 0] >= 0)
        assert decided, nb
    return True


def test_assignment_on_the_emulator_equals_the_float64_model(emu_so):
    check_assign(emu_so)


# ---------------------------------------------------------------- 3: errors
def check_pass_errors(lib_path):
    org, rec, bd = six_ctu_picture()
    kw = dict(lib_path=lib_path)
    lab = np.zeros((6, 2), np.uint8)
    bad = lab.copy(); bad[3, 1] = 8
    cds = assign_candidates(1)
    c129 = cds[:2].copy(); c129[1]["coeff"][4] = 129
    cclip = cds[:2].copy(); cclip[0]["clip_idx"][5] = 1
    for args in (dict(labels=bad, n_alts=8), dict(labels=lab, n_alts=0), dict(labels=lab, n_alts=9), dict(cands=cds[:1], n_alts=0), dict(cands=np.zeros(9, vv.ALF_CHROMA_CAND), n_alts=9),
                 dict(cands=c129), dict(cands=cclip), dict()):
        with pytest.raises(pkg.VvcxError, match="error -1"):
            vv.alf_chroma_alts_picture(org, rec, bd, 1, **args, **kw)
    c128 = cds[:2].copy(); c128[1]["coeff"][4] = 128                                                # the existing pass's limit: +-128 is taken
    vv.alf_chroma_alts_picture(org, rec, bd, 1, cands=c128, **kw)
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_decide_picture(org, rec, bd, [1.0] * 3, n_bins=4, flags=8, **kw)
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_decide_picture(org, rec, bd, [1.0] * 3, n_bins=1, flags=ALTS(9), **kw)
    with pytest.raises(pkg.VvcxError, match="error -1"):
        vv.alf_decide_picture(org, rec, bd, [1.0] * 3, n_bins=1, flags=ALTS(2) | vv.ALF_NONLINEAR_CHROMA, **kw)      # the clip search needs 4 bins


def test_pass_argument_errors_are_status_codes(emu_so):
    check_pass_errors(emu_so)


# ---------------------------------------------------------------- the chroma cost of a decision, from the statistics
def chroma_cost(prm, chroma, nb, lam):
    """(J chroma relative to chroma off, predicted error per component, enabled blocks): per enabled block err / 16384 + lambda * bits(alt, K), then the parameter set:
    lambda * (ue(K - 1) + per alternative 1 + coefficient bits + 12 when nonlinear) - include/vvcx.h's count"""
    a = prm["aps"][0]
    k = int(a[627])
    j, pred, on = 0.0, [0.0, 0.0], 0
    for i, u in enumerate(prm["ctu"]):
        for c in range(2):
            if u[1 + c]:
                t = int(u[4 + c])
                e = filter_err(chroma[i, c], nb, 7, a[636 + 6 * t:642 + 6 * t], a[684 + 6 * t:690 + 6 * t] if a[628 + t] else [0] * 6) / 16384.0
                j += e + lam * alt_bits(t, k); pred[c] += e + int(chroma[i, c, -1]); on += 1
    if prm["chroma_aps"] >= 0:
        j += lam * (ue_bits(k - 1) + sum(1 + coeff_bits(a[636 + 6 * t:642 + 6 * t]) + (12 if a[628 + t] else 0) for t in range(k)))
    return j, pred, on


def check_valid(prm, k_max):
    a, ctu = prm["aps"][0], prm["ctu"]
    if prm["chroma_aps"] < 0:
        assert not ctu[:, 1:3].any() and not ctu[:, 4:6].any()
        return
    k = int(a[627])
    assert prm["chroma_aps"] == 0 and 1 <= k <= k_max
    used = set(ctu[:, 4][ctu[:, 1] != 0].tolist()) | set(ctu[:, 5][ctu[:, 2] != 0].tolist())
    assert used == set(range(k)), (used, k)                                                          # every alternative is used, every choice exists
    assert not ctu[:, 4][ctu[:, 1] == 0].any() and not ctu[:, 5][ctu[:, 2] == 0].any()
    assert a[636:684].min() >= -128 and a[636:684].max() <= 127 and a[684:732].max() <= 3
    assert not a[636 + 6 * k:684].any() and not a[628 + k:636].any()


def luma_part(prm):
    return prm["aps"][0, :627].tolist(), prm["luma_aps"], prm["ctu"][:, [0, 3]].tolist()


# ---------------------------------------------------------------- 4: planted alternatives
def check_planted(lib_path, filter_fn):
    org, rec, bd, gen = planted_picture()
    assert min(p.min() for p in org[1:]) >= 444 and max(p.max() for p in org[1:]) <= 621          # nothing clamps
    chroma = vv.alf_statistics_picture(org, rec, bd, 1, lib_path=lib_path)[1]
    errs = model_errs(chroma, 1, [cand(q) for q in PLANTED])
    planted = np.stack([PLANTED_CB, PLANTED_CR], 1)
    margin = []
    for a in range(6):
        for c in range(2):
            e = [v / 16384.0 for v in errs[a][c]]
            t = planted[a, c]
            assert abs(e[t] + int(chroma[a, c, -1])) <= 350, (a, c, e[t], int(chroma[a, c, -1]))      # the planted alternative leaves next to nothing
            margin.append(min(e[s] - e[t] for s in range(3) if s != t))
    print("least margin of the planted alternative %.1f" % min(margin))
    assert min(margin) >= 9944
    for lam in (0.0, 50.0):
        j_planted = chroma_cost(gen, chroma, 1, lam)[0]
        prm = vv.alf_decide_picture(org, rec, bd, [lam] * 3, flags=ALTS(4), lib_path=lib_path)
        one = vv.alf_decide_picture(org, rec, bd, [lam] * 3, flags=ALTS(1), lib_path=lib_path)
        check_valid(prm, 4)
        j, pred, on = chroma_cost(prm, chroma, 1, lam)
        j_one = chroma_cost(one, chroma, 1, lam)[0]
        k = int(prm["aps"][0, 627])
        print("lambda %g: %d alternatives, J %.1f, planted %.1f, one alternative %.1f, labels %s" % (lam, k, j, j_planted, j_one, prm["ctu"][:, 4:6].ravel().tolist()))
        # (i) every block on, the planted partition up to renaming: blocks share a returned alternative only if they share the planted one, and with three returned
        # alternatives that is a bijection (lambda 0 may split a planted group where a fourth filter fits its rounding noise: (ii) allows more than three there)
        assert on == 12 and prm["ctu"][:, 1:3].all()
        got = prm["ctu"][:, 4:6]
        assert all(len(set(planted[got == t].tolist())) == 1 for t in range(k)), (got.tolist(), planted.tolist())
        # (ii)
        assert k == 3 if lam else k >= 3
        if k == 3:
            assert len({(int(g), int(p)) for g, p in zip(got.ravel(), planted.ravel())}) == 3
        # (iii), (iv)
        assert j <= j_planted + 0.01 * abs(j_planted), (j, j_planted)
        assert j < j_one - 100000, (j, j_one)
        assert same_decision(one, vv.alf_decide_picture(org, rec, bd, [lam] * 3, lib_path=lib_path))
        assert luma_part(prm) == luma_part(one)
        # (v) the filter leaves what the statistics predict
        filtered = filter_fn(rec, 384, 256, bd, prm)
        for c in range(2):
            n = org[1 + c].size
            act = int(((org[1 + c].astype(np.int64) - np.asarray(filtered[1 + c]).astype(np.int64)) ** 2).sum())
            print("component %d: predicted %.1f actual %d samples %d" % (1 + c, pred[c], act, n))
            assert abs(act - pred[c]) <= np.sqrt(n * max(pred[c], 0.0)) + n / 4, (c, pred[c], act)


def test_planted_alternatives_are_found(emu_so):
    check_planted(emu_so, lambda rec, w, h, bd, prm: O.alf_picture(rec, w, h, bd, prm))


# ---------------------------------------------------------------- 5: monotone and inert
def check_monotone(lib_path):
    NLC = vv.ALF_NONLINEAR_LUMA | vv.ALF_NONLINEAR_CHROMA
    for (org, rec, bd), nb, base in ((decision_picture(256, 128), 1, 0), (nonlinear_picture(), 4, NLC)):
        chroma = vv.alf_statistics_picture(org, rec, bd, nb, lib_path=lib_path)[1]
        for lam in (0.0, 8.0):
            plain = vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=nb, flags=base, lib_path=lib_path)
            assert same_decision(vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=nb, flags=base | ALTS(1), lib_path=lib_path), plain)
            many = vv.alf_decide_picture(org, rec, bd, [lam] * 3, n_bins=nb, flags=base | ALTS(8), lib_path=lib_path)
            check_valid(many, min(8, 2 * plain["ctu"].shape[0]))
            j1, j8 = chroma_cost(plain, chroma, nb, lam)[0], chroma_cost(many, chroma, nb, lam)[0]
            print("bins %d lambda %g: J chroma %.1f with one alternative, %.1f with up to 8 (%d used)" % (nb, lam, j1, j8, many["aps"][0, 627]))
            assert j8 <= j1 + 1e-6 and j1 <= 1e-6
            assert luma_part(many) == luma_part(plain)
    org, rec, bd = decision_picture(128, 128)
    prm = vv.alf_decide_picture(org, rec, bd, [0.0] * 3, flags=ALTS(8), lib_path=lib_path)                # one CTU: at most 2 * ctus alternatives
    check_valid(prm, 2)


def test_more_alternatives_never_cost_more_and_leave_luma_alone(emu_so):
    check_monotone(emu_so)


# ---------------------------------------------------------------- 6: the resident route
def merged(res):
    """the frames' decisions (each with its own parameter set as aps[0]) as one call's: the sets stacked, frame f pointing at set f"""
    aps = np.concatenate([r["aps"] for r in res])
    return [dict(aps=aps, luma_aps=[f] if r["luma_aps"] else [], chroma_aps=f if r["chroma_aps"] >= 0 else -1, ctu=r["ctu"]) for f, r in enumerate(res)]


def check_resident(lib_path, to_dev, to_host, emit_payload=False):
    enc, frames, recs = _coded_pair(lib_path, to_dev, to_host) if not emit_payload else _payload_pair(to_dev, to_host)
    nctu, lam = enc.ctus_per_frame, 2.0
    lab = np.zeros((2, nctu, 2), np.uint8)
    cds = np.zeros((2, 2), vv.ALF_CHROMA_CAND); cds[:, 0]["coeff"] = KNOWN_CHROMA
    for call in (lambda: enc.alf_chroma_label_sums(lab, 2), lambda: enc.alf_chroma_assign(cds, (lam, lam))):
        with pytest.raises(pkg.VvcxError, match="error -4"):
            call()                                             # nothing resident yet
    _, chroma, _ = enc.alf_statistics_bound_frames(0, 2, 1)
    enc.alf_statistics_resident(0, 2, 1)
    lab[0, 0] = (1, OFF); lab[1, nctu - 1] = (0, 1)
    sums = enc.alf_chroma_label_sums(lab, 2)
    elab, eerr, ecost = enc.alf_chroma_assign(cds, (lam, 3.0))
    for f in range(2):
        assert np.array_equal(sums[f], model_label_sums(chroma[f], lab[f], 2)), f
        mlab, merr, mcost = model_assign(model_errs(chroma[f], 1, cds[f]), (lam, 3.0), 2)
        assert np.array_equal(elab[f], mlab) and np.array_equal(eerr[f], merr) and ecost[f] == mcost, f
    with pytest.raises(pkg.VvcxError, match="error -1"):
        enc.alf_chroma_label_sums(np.full((2, nctu, 2), 2, np.uint8), 2)
    res = enc.alf_decide_resident([lam] * 3, flags=ALTS(3))
    calls = enc.alf_device_calls()
    assert 4 < calls <= 4 + 2 * (4 + 3)                        # the one-alternative decision's four passes, then at most K + 1 pairs for K = 3, 2
    planes = [[np.asarray(p) for p in r] for r in recs]
    for f in range(2):
        check_valid(res[f], 3)
        assert same_decision(res[f], vv.alf_decide_picture(frames[f], planes[f], 8, [lam] * 3, flags=ALTS(3), lib_path=lib_path)), f
    if emit_payload:
        hdr = [(0, 0, int(r["ctu"][:, 0].any() or r["chroma_aps"] >= 0), int(r["ctu"][:, 1].any()), int(r["ctu"][:, 2].any())) for r in res]
        enc.rewrite_payload(np.array(hdr, np.uint8), alf=merged(res))
    enc.alf_bound_frames(merged(res))
    for call in (lambda: enc.alf_chroma_label_sums(lab, 2), lambda: enc.alf_chroma_assign(cds, (lam, lam))):
        with pytest.raises(pkg.VvcxError, match="error -4"):
            call()                                             # the filter has touched the pictures
    enc.close()
    return res


def _payload_pair(to_dev, to_host):
    """_coded_pair's two pictures behind a handle that keeps the payload (the rewrite pass needs it)"""
    w, h, bd = 136, 72, 8
    sp = pkg.slice_params(45)
    frames = [pkg.synth_frame(w, h, i, bd, 90 + i, chroma_texture=0.5) for i in range(2)]
    enc = pkg.VvcxEncoder(w, h, bd, tools=pkg.TOOL_CU_REUSE, max_frames=2, emit_payload=True)
    enc.set_slice(sp["qp"], sp["qp_c"], sp["lam"], sp["dist_weight"])
    dev = [([to_dev(np.ascontiguousarray(p)) for p in f], [to_dev(np.zeros_like(p)) for p in f]) for f in frames]
    enc.bind_frames([([ptr for _, ptr in o], [ptr for _, ptr in r], [p.shape[1] for p in f]) for (o, r), f in zip(dev, frames)])
    enc.compress_bound_frames(); enc.deblock_bound_frames()
    enc.sao_bound_frames(np.stack([pkg.sao_test_params(70 + i, w, h) for i in range(2)]))
    return enc, frames, [[to_host(t) for t, _ in r] for _, r in dev]


def test_resident_route_on_the_emulator(emu_so):
    check_resident(emu_so, lambda a: (a, a.ctypes.data), lambda a: a)


# ---------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_label_sums_on_the_gpu_equal_the_integer_model():
    check_label_sums(None)


@pytest.mark.gpu
def test_assignment_on_the_gpu_equals_the_float64_model():
    check_assign(None)


@pytest.mark.gpu
def test_pass_argument_errors_on_the_gpu_are_status_codes():
    check_pass_errors(None)


@pytest.mark.gpu
def test_planted_alternatives_are_found_on_the_gpu():
    check_planted(None, lambda rec, w, h, bd, prm: vv.alf_picture(rec, bd, prm))


@pytest.mark.gpu
def test_more_alternatives_never_cost_more_on_the_gpu():
    check_monotone(None)


@pytest.mark.gpu
def test_resident_route_on_the_gpu():
    import torch

    def to_dev(a):
        t = torch.from_numpy(a).cuda()
        return t, t.data_ptr()
    check_resident(None, to_dev, lambda t: t.cpu().numpy(), emit_payload=True)
