"""Leaf operators of the C-ABI (include/vvcx.h) against the golden vectors produced by the REAL reference code
(tests/golden/make_golden.py → oracle/_ref/libvtmref.so): the device functions of the path are pinned directly to the
reference, not only to the oracle.  GPU tests run every vector; the CPU tests run a slice of them through the CPU
debug emulation of the same sources."""
import importlib
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGNAME = "reduce-complexity-for-intra-coding-of-vvc_amd"
pkg = importlib.import_module(PKGNAME)
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def emu_so():
    from conftest import locked_make
    locked_make(os.path.join(ROOT, PKGNAME, "csrc"), "emu")
    return os.path.join(ROOT, "tools", "hipemu", "build", "libvvcx_emu.so")


def _distortion(lib, limit):
    g = np.load(os.path.join(G, "dist.npz"))
    off, n = 0, 0
    for (w, h, bd, had, sad, sse) in g["rows"][:limit]:
        k = int(w * h)
        a, b = g["a"][off:off + k], g["b"][off:off + k]; off += k
        got = pkg.distortion_batch(a, b, int(w), int(h), lib_path=lib)[0]
        assert (int(got[0]), int(got[1]), int(got[2])) == (int(sad), int(had), int(sse)), (w, h, bd)
        n += 1
    return n


def _cabac(lib, limit):
    g = np.load(os.path.join(G, "cabac.npz"))
    for i, qp in enumerate(g["qps"]):
        s0, s1 = pkg.ctx_init(int(qp), lib_path=lib)
        assert np.array_equal(s0, g["s0"][i]) and np.array_equal(s1, g["s1"][i])
    for (ctx, qi, bits, e0, e1), bins in list(zip(g["seq_meta"], g["seq_bins"]))[:limit]:
        got = pkg.cabac_code_bins(int(g["s0"][qi, ctx]), int(g["s1"][qi, ctx]), int(ctx), bins, lib_path=lib)
        assert got == (int(bits), int(e0), int(e1)), ctx
    rd = g["rd"]
    for lam in np.unique(rd[:, 0]):
        rows = rd[rd[:, 0] == lam]
        cost = pkg.rd_cost_batch(lam, rows[:, 1].astype(np.uint64), rows[:, 2].astype(np.uint64), lib_path=lib)
        assert np.array_equal(cost, rows[:, 3])                 # identical doubles: two roundings, no FMA (CL/RdCost.cpp:63-74)
    # the ends of the ranges (cabac_range.npz): every QP the C-ABI takes and beyond, every adaptation rate into saturation and out of it, operands up to 2^62
    import oracle_lib as O
    r = np.load(os.path.join(G, "cabac_range.npz"))
    for i, qp in list(enumerate(r["qps"]))[::(7 if limit else 1)]:
        s0, s1 = pkg.ctx_init(int(qp), lib_path=lib)
        assert np.array_equal(s0, r["s0"][i]) and np.array_equal(s1, r["s1"][i]), qp
    for (ctx, rt, a0, b0, kind, bits, e0, e1) in r["seq"][::(9 if limit else 1)]:
        got = pkg.cabac_code_bins(int(a0), int(b0), int(ctx), O.cabac_range_bins(int(kind)), lib_path=lib)
        assert got == (int(bits), int(e0), int(e1)), (ctx, rt, a0, b0, kind)
    for lam in np.unique(r["lam"]):
        k = r["lam"] == lam
        assert np.array_equal(pkg.rd_cost_batch(lam, r["frac_bits"][k], r["dist"][k], lib_path=lib), r["cost"][k]), lam


def _scan(lib, keys=None):
    g = np.load(os.path.join(G, "scan.npz"))
    for key in (keys or g.files):
        w, h = map(int, key[1:].split("x"))
        idx = pkg.scan_order(w, h, lib_path=lib)
        assert np.array_equal(idx, g[key][:len(idx)]), key


def _intra(lib, limit):
    g = np.load(os.path.join(G, "intra.npz"))
    meta, off, n = g["case_meta"], 0, 0
    offs = []
    for m in meta:
        ei, bd, comp, x, y, w, h, dirm, mrl, force = map(int, m)
        cw, chh = (w, h) if comp == 0 else (w // 2, h // 2)
        offs.append((off, cw * chh)); off += cw * chh
    by_env = {}
    for i, m in enumerate(meta[:limit] if limit else meta):
        by_env.setdefault((int(m[0]), int(m[1])), []).append(i)
    for (ei, bd), idxs in by_env.items():
        reco = [g["env%d_reco%d" % (ei, c)] for c in range(3)]
        H, W = reco[0].shape
        dt = np.uint8 if bd == 8 else np.uint16
        coded = np.repeat(np.repeat(g["env%d_coded" % ei], 2, axis=0), 2, axis=1).astype(np.uint8)     # 8x8 luma → 4x4 units
        enc = pkg.VvcxEncoder(W, H, bd, lib_path=lib)
        cases = np.zeros(len(idxs), pkg.PRED_CASE_DTYPE)
        for k, i in enumerate(idxs):
            _, _, comp, x, y, w, h, dirm, mrl, force = map(int, meta[i])
            sh = 1 if comp else 0
            cases[k] = (comp, x >> sh, y >> sh, w >> sh, h >> sh, dirm, mrl)
        preds = enc.intra_pred_batch([p.astype(dt) for p in reco], [coded, coded], cases)
        enc.close()
        for k, i in enumerate(idxs):
            o, sz = offs[i]
            assert np.array_equal(preds[k].ravel(), g["case_pred"][o:o + sz]), ("pred", tuple(meta[i]))
            n += 1
    return n


def _trquant(lib, limit):
    g = np.load(os.path.join(G, "trquant.npz"))
    off, n = 0, 0
    for (bd, qp, w, h, abs_sum) in g["meta"]:
        k = int(w * h)
        resi = g["resi"][off:off + k].astype(np.int32); lev_e = g["lev"][off:off + k]; out_e = g["resi_out"][off:off + k].astype(np.int32); off += k
        if limit and n >= limit:
            break
        if limit and k > 256:
            continue
        mid, mx = 1 << (int(bd) - 1), (1 << int(bd)) - 1
        org = (mid + resi).astype(np.int16); pred = np.full(k, mid, np.int16)
        lev, rec, sse, cbf = pkg.transform_quant_batch(org, pred, int(w), int(h), int(bd), int(qp) + 6 * (int(bd) - 8), lib_path=lib)
        rec_e = np.clip(mid + out_e, 0, mx) if abs_sum > 0 else np.full(k, mid)
        assert np.array_equal(lev.ravel(), lev_e) and int(cbf[0]) == int(abs_sum > 0), ("levels", bd, qp, w, h)
        assert np.array_equal(rec.ravel().astype(np.int32), rec_e), ("rec", bd, qp, w, h)
        assert int(sse[0]) == int(((org.astype(np.int64) - rec_e) ** 2).sum())
        n += 1
    return n


def _depquant(lib, limit):
    """vvcx_depquant_batch (the search's wave_depquant + wave_dequant_dq) against the reference's DepQuant vectors (tests/golden/depquant.npz)"""
    from test_oracle_golden import _depquant_cases
    n = 0
    for c in _depquant_cases():
        w, h, bd = c["w"], c["h"], c["bd"]
        if limit and (n >= limit or w * h > 64):
            continue
        mid, mx = 1 << (bd - 1), (1 << bd) - 1
        resi = c["resi"].astype(np.int32)
        org = (mid + resi).astype(np.int16); pred = np.full(w * h, mid, np.int16)
        lev, rec, sse, cbf = pkg.depquant_batch(org, pred, w, h, bd, c["qp_used"], c["comp"], c["mts"], c["cbf_cb"], c["lam"], c["ctx"][0], c["ctx"][1], lib_path=lib)
        key = (bd, c["qp"], c["comp"], w, h, c["mts"])
        assert np.array_equal(lev.ravel(), c["lev"]) and int(cbf[0]) == int(c["asum"] > 0), ("levels", key)
        rec_e = np.clip(mid + c["out"].astype(np.int32), 0, mx) if c["asum"] > 0 else np.full(w * h, mid)
        assert np.array_equal(rec.ravel().astype(np.int32), rec_e), ("rec", key)
        assert int(sse[0]) == int(((org.astype(np.int64) - rec_e) ** 2).sum())
        n += 1
    return n


def _lfnst(lib, limit):
    """vvcx_lfnst_depquant_batch (wave_lfnst_fwd / wave_lfnst_inv around the trellis, as the search runs them) against the reference's LFNST vectors
    (tests/golden/lfnst.npz; the DepQuant cases: the device runs LFNST only over the dependent quantiser)"""
    from test_oracle_golden import _lfnst_cases
    n = 0
    for c in _lfnst_cases():
        w, h, bd = c["w"], c["h"], c["bd"]
        if not c["dq"] or (limit and (n >= limit or w * h > 64)):
            continue
        mid, mx = 1 << (bd - 1), (1 << bd) - 1
        resi = c["resi"].astype(np.int32)
        org = (mid + resi).astype(np.int16); pred = np.full(w * h, mid, np.int16)
        d = 0 if c["mip"] else c["dir"]
        lev, rec, sse, cbf = pkg.lfnst_depquant_batch(org, pred, w, h, bd, c["qp_used"], c["comp"], c["lfnst"], d, c["cbf_cb"], c["lam"], c["ctx"][0], c["ctx"][1], lib_path=lib)
        key = (bd, c["qp"], c["comp"], w, h, c["dir"], c["mip"], c["lfnst"])
        assert np.array_equal(lev.ravel(), c["lev"]) and int(cbf[0]) == int(c["asum"] > 0), ("levels", key)
        rec_e = np.clip(mid + c["out"].astype(np.int32), 0, mx) if c["asum"] > 0 else np.full(w * h, mid)
        assert np.array_equal(rec.ravel().astype(np.int32), rec_e), ("rec", key)
        n += 1
    return n


def _transform_skip(lib, limit):
    """vvcx_transform_skip_batch (the {DCT2, TS} pruning, xTransformSkip, ts_rdoq_lane, wave_ts_recon as the search runs them) against the reference's TrQuant /
    QuantRDOQ vectors (tests/golden/ts.npz); the bits of residual_codingTS against the oracle's estimator, whose syntax the reference decoder parsed (bitstream_ts.npz)"""
    import ctypes as C
    import oracle_lib as O
    vv = importlib.import_module(PKGNAME + ".vvcx")
    OL = O.lib()
    OL.orc_residual_bits_ts.restype = C.c_uint64
    OL.orc_residual_bits_ts.argtypes = [C.c_void_p] * 3 + [C.c_int] * 2
    g = np.load(os.path.join(G, "ts.npz"))
    off = n = 0
    for i, (bd, qp, w, h, kind, keep, qu, a, gi) in enumerate(g["meta"]):
        P = int(w) * int(h)
        resi, lev, ro = g["resi"][off:off + P], g["lev"][off:off + P], g["resi_out"][off:off + P]
        off += P
        if limit and (n >= limit or P > 64):
            continue
        s0, s1 = g["ctx"][gi]
        l, o, aa, kk, bits = vv.transform_skip_batch(resi, int(w), int(h), int(bd), int(qp + 6 * (bd - 8)), float(g["lam"][i]), s0, s1, lib_path=lib)
        key = (int(bd), int(qp), int(w), int(h), int(kind))
        assert np.array_equal(l.ravel(), lev) and int(aa[0]) == int(a), ("levels", key)
        assert int(kk[0]) == int(keep), ("pruning", key)
        if a > 0:
            assert np.array_equal(o.ravel(), ro), ("residual", key)
            t0, t1, lv = s0.copy(), s1.copy(), np.ascontiguousarray(lev)
            assert int(bits[0]) == OL.orc_residual_bits_ts(t0.ctypes.data, t1.ctypes.data, lv.ctypes.data, int(w), int(h)), ("bits", key)
        n += 1
    return n


def _isp_tu(lib, limit):
    """vvcx_isp_tu_batch (wave_code_block_isp: implicit DST-VII / DCT-II, the one-stage transforms of one-sample-wide blocks, the trellis on 1 x 16 / 16 x 1 / 2 x 8 / 8 x 2
    coefficient groups with the cbf contexts of ISP sub-partitions) against the reference's TrQuant / DepQuant vectors for TUs of ISP CUs (tests/golden/isp.npz)"""
    vv = importlib.import_module(PKGNAME + ".vvcx")
    g = np.load(os.path.join(G, "isp.npz"))
    off = n = 0
    for i, (bd, qp, w, h, isp, k, nsub, tw, th, prev, inferred, a, gi) in enumerate(g["meta"]):
        P = int(tw) * int(th)
        resi, lev, ro = g["resi"][off:off + P], g["lev"][off:off + P], g["resi_out"][off:off + P]
        off += P
        if limit and (n >= limit or P > 64 or i % 5):
            continue
        mid, mx = 1 << (bd - 1), (1 << bd) - 1
        org = (mid + resi.astype(np.int32)).astype(np.int16); pred = np.full(P, mid, np.int16)
        s0, s1 = g["ctx"][gi]
        l, r, sse, cbf = vv.isp_tu_batch(org, pred, int(tw), int(th), int(bd), int(qp + 6 * (bd - 8)), float(g["lam"][i]), int(prev), int(inferred), s0, s1, lib_path=lib)
        key = (int(bd), int(qp), int(w), int(h), int(isp), int(k), int(tw), int(th))
        assert np.array_equal(l.ravel(), lev) and int(cbf[0]) == int(a > 0), ("levels", key)
        rec_e = np.clip(mid + ro.astype(np.int32), 0, mx) if a > 0 else np.full(P, mid)
        assert np.array_equal(r.ravel().astype(np.int32), rec_e), ("rec", key)
        n += 1
    return n


# ---- full-range residuals (tests/golden/trquant_range.npz): the fixture's own org and pred, so that org - pred spans +-(2^bd - 1) ----
def _range_slice(fam, limit):
    """every case of a family, or (CPU emulation) limit blocks of at most 256 samples spread evenly over the patterns, bit depths and QPs"""
    from test_oracle_golden import _range_cases
    cases = _range_cases(fam)
    if not limit:
        return cases
    small = [c for c in cases if c["w"] * c["h"] <= 256]
    return small[::max(1, len(small) // limit)][:limit]


def _range_expect(c, lev, rec, sse, cbf, key):
    """block results of a leaf call against the reference: levels, cbf, rec == clip(pred + resi_out) if coded else pred, SSE(org, rec)"""
    mx = (1 << c["bd"]) - 1
    assert np.array_equal(lev.ravel(), c["lev"]) and int(cbf) == int(c["asum"] > 0), ("levels", key)
    rec_e = np.clip(c["pred"].astype(np.int32) + c["out"], 0, mx) if c["asum"] > 0 else c["pred"].astype(np.int32)
    assert np.array_equal(rec.ravel().astype(np.int32), rec_e), ("rec", key)
    assert int(sse) == int(((c["org"].astype(np.int64) - rec_e) ** 2).sum()), ("sse", key)


def _range_trquant(lib, limit):
    n = 0
    for c in _range_slice("a", limit):
        lev, rec, sse, cbf = pkg.transform_quant_batch(c["org"], c["pred"], c["w"], c["h"], c["bd"], c["qp"] + 6 * (c["bd"] - 8), lib_path=lib)
        _range_expect(c, lev, rec, sse[0], cbf[0], ("a", c["bd"], c["qp"], c["w"], c["h"], c["pat"]))
        n += 1
    return n


def _range_depquant(lib, limit):
    n = 0
    for c in _range_slice("b", limit):
        lev, rec, sse, cbf = pkg.depquant_batch(c["org"], c["pred"], c["w"], c["h"], c["bd"], c["qp_used"], c["comp"], c["mts"], c["cbf_cb"], c["lam"], c["ctx"][0], c["ctx"][1], lib_path=lib)
        _range_expect(c, lev, rec, sse[0], cbf[0], ("b", c["bd"], c["qp"], c["comp"], c["w"], c["h"], c["mts"], c["cbf_cb"], c["pat"]))
        n += 1
    return n


def _range_lfnst(lib, limit):
    n = 0
    for c in _range_slice("c", limit):
        lev, rec, sse, cbf = pkg.lfnst_depquant_batch(c["org"], c["pred"], c["w"], c["h"], c["bd"], c["qp_used"], c["comp"], c["lfnst"], c["dir"], c["cbf_cb"], c["lam"], c["ctx"][0], c["ctx"][1], lib_path=lib)
        _range_expect(c, lev, rec, sse[0], cbf[0], ("c", c["bd"], c["qp"], c["w"], c["h"], c["dir"], c["lfnst"], c["pat"]))
        n += 1
    return n


def _range_transform_skip(lib, limit):
    vv = importlib.import_module(PKGNAME + ".vvcx")
    n = 0
    for c in _range_slice("d", limit):
        s0, s1 = c["ctx"]
        l, o, aa, kk, bits = vv.transform_skip_batch(c["resi"], c["w"], c["h"], c["bd"], c["qp"] + 6 * (c["bd"] - 8), c["lam"], s0, s1, lib_path=lib)
        key = ("d", c["bd"], c["qp"], c["w"], c["h"], c["pat"])
        assert np.array_equal(l.ravel(), c["lev"]) and int(aa[0]) == c["asum"], ("levels", key)
        assert int(kk[0]) == c["keep"], ("pruning", key)
        if c["asum"] > 0:
            assert np.array_equal(o.ravel(), c["out"]), ("residual", key)
        n += 1
    return n


def _range_isp_tu(lib, limit):
    vv = importlib.import_module(PKGNAME + ".vvcx")
    n = 0
    for c in _range_slice("e", limit):
        s0, s1 = c["ctx"]
        l, r, sse, cbf = vv.isp_tu_batch(c["org"], c["pred"], c["w"], c["h"], c["bd"], c["qp"] + 6 * (c["bd"] - 8), c["lam"], c["prev"], c["inferred"], s0, s1, lib_path=lib)
        _range_expect(c, l, r, sse[0], cbf[0], ("e", c["bd"], c["qp"], c["w"], c["h"], c["isp"], c["prev"], c["pat"]))
        n += 1
    return n


def _range_batched(lib, shapes):
    """all patterns of one (shape, bit depth, QP) back to back in one launch of the plain and one of the dependent quantiser: block i (workgroup i with its own slice of the
    transform scratch, 2048 int32 that a 64x64 block fills to the last word, and of the trellis scratch) must equal the reference's case i"""
    from test_oracle_golden import _range_cases
    n = 0
    for fam in "ab":
        groups = {}
        for c in _range_cases(fam):
            if (c["w"], c["h"]) in shapes and c.get("comp", 0) == 0 and c.get("mts", 0) == 0:
                groups.setdefault((c["w"], c["h"], c["bd"], c["qp"]), []).append(c)
        assert len(groups) == len(shapes) * 6
        for (w, h, bd, qp), cs in groups.items():
            assert len(cs) == (11 if qp == 27 else 9) and len(set(c["pat"] for c in cs)) == len(cs)
            org = np.concatenate([c["org"] for c in cs]); pred = np.concatenate([c["pred"] for c in cs])
            if fam == "a":
                lev, rec, sse, cbf = pkg.transform_quant_batch(org, pred, w, h, bd, qp + 6 * (bd - 8), lib_path=lib)
            else:
                c0 = cs[0]
                assert all((c["qp_used"], c["lam"], c["gi"]) == (c0["qp_used"], c0["lam"], c0["gi"]) for c in cs)
                lev, rec, sse, cbf = pkg.depquant_batch(org, pred, w, h, bd, c0["qp_used"], 0, 0, 0, c0["lam"], c0["ctx"][0], c0["ctx"][1], lib_path=lib)
            for i, c in enumerate(cs):
                _range_expect(c, lev[i], rec[i], sse[i], cbf[i], ("batch", fam, i, bd, qp, w, h, c["pat"]))
                n += 1
    return n


@pytest.mark.gpu
def test_gpu_full_range_transform_quant_matches_reference():
    """incl. the matrix-core rows of 32- and 64-wide blocks, which only the GPU build has: high bytes -4 .. 3 of the operand split, idle half tiles (32x4, 64x8), two tiles (32x64)"""
    assert _range_trquant(None, None) == 580


@pytest.mark.gpu
def test_gpu_full_range_dependent_quantisation_matches_reference():
    assert _range_depquant(None, None) == 1276


@pytest.mark.gpu
def test_gpu_full_range_lfnst_matches_reference():
    assert _range_lfnst(None, None) == 432


@pytest.mark.gpu
def test_gpu_full_range_transform_skip_matches_reference():
    assert _range_transform_skip(None, None) == 232


@pytest.mark.gpu
def test_gpu_full_range_isp_sub_partition_blocks_match_reference():
    assert _range_isp_tu(None, None) == 290


@pytest.mark.gpu
def test_gpu_batched_leaf_launches_match_reference_block_by_block():
    assert _range_batched(None, ((4, 4), (32, 4), (32, 32), (64, 64))) == 2 * 4 * (2 * 9 + 11) * 2


def test_emulated_batched_leaf_launches_match_reference_block_by_block(emu_so):
    assert _range_batched(emu_so, ((4, 4), (32, 4))) == 2 * 2 * (2 * 9 + 11) * 2


@pytest.mark.gpu
def test_gpu_isp_sub_partition_blocks_match_reference():
    assert _isp_tu(None, None) == 624


@pytest.mark.gpu
def test_gpu_transform_skip_matches_reference():
    assert _transform_skip(None, None) == 384


@pytest.mark.gpu
def test_gpu_dependent_quantisation_matches_reference():
    assert _depquant(None, None) == 575


@pytest.mark.gpu
def test_gpu_lfnst_matches_reference():
    assert _lfnst(None, None) == 895


@pytest.mark.gpu
def test_gpu_transform_quant_matches_reference():
    assert _trquant(None, None) == 75


@pytest.mark.gpu
def test_gpu_distortion_matches_reference():
    assert _distortion(None, None) == 180


@pytest.mark.gpu
def test_gpu_cabac_model_rdcost_and_scan_match_reference():
    _cabac(None, None)
    _scan(None)


@pytest.mark.gpu
def test_gpu_intra_prediction_matches_reference():
    assert _intra(None, None) > 1000


def test_emulated_leaf_operators_match_reference(emu_so):
    assert _distortion(emu_so, 24) == 24
    _cabac(emu_so, 6)
    _scan(emu_so, ["s4x4", "s8x8", "s16x4", "s32x32"])
    assert _intra(emu_so, 40) == 40
    assert _trquant(emu_so, 8) == 8
    assert _depquant(emu_so, 12) == 12
    assert _lfnst(emu_so, 16) == 16
    assert _transform_skip(emu_so, 40) == 40
    assert _isp_tu(emu_so, 30) == 30
    assert _range_trquant(emu_so, 32) == 32                 # full-range residuals: slices of tests/golden/trquant_range.npz
    assert _range_depquant(emu_so, 32) == 32
    assert _range_lfnst(emu_so, 24) == 24
    assert _range_transform_skip(emu_so, 24) == 24
    assert _range_isp_tu(emu_so, 24) == 24


# ---- every block shape, picture edges, range edges (tests/golden/intra_shapes_*.npz, cclm_shapes.npz, mip_range.npz, dist_range.npz) ----
def _shape_slice(cases, limit, need):
    """every case, or (CPU emulation) `limit` small blocks spread evenly plus the first case that satisfies each predicate of `need`"""
    if not limit:
        return cases
    small = [c for c in cases if c["w"] * c["h"] <= 256]
    pick = small[::max(1, len(small) // limit)][:limit]
    for f in need:
        pick.append(next(c for c in cases if f(c) and not any(c is q for q in pick)))
    return pick


def _shapes(lib, name, bd, limit=None, need=()):
    """vvcx_intra_pred_batch on the cases of a shape fixture at one bit depth: one call per (picture, coded map), every prediction bit exact"""
    import oracle_lib as O
    from test_oracle_golden import _shape_cases, _leaf_planes
    cases = _shape_slice([c for c in _shape_cases(name) if c["bd"] == bd], limit, need)
    groups = {}
    for c in cases:
        groups.setdefault((c["pattern"], c["kind"], c["x"], c["y"], c["w"], c["h"]), []).append(c)
    enc = pkg.VvcxEncoder(O.LEAF_PIC, O.LEAF_PIC, bd, lib_path=lib)
    n = 0
    for (pattern, kind, x, y, w, h), cs in groups.items():
        reco = [p.astype(np.uint8 if bd == 8 else np.uint16) for p in _leaf_planes(bd, pattern)]
        coded = np.repeat(np.repeat(O.leaf_coded_map(x, y, w, h, kind), 2, axis=0), 2, axis=1)            # 8x8 luma -> 4x4 units
        pc = np.zeros(len(cs), pkg.PRED_CASE_DTYPE)
        for k, c in enumerate(cs):
            sh = 1 if c["comp"] else 0
            pc[k] = (c["comp"], x >> sh, y >> sh, w >> sh, h >> sh, c["mode"], c["mrl"])
        preds = enc.intra_pred_batch(reco, [coded, coded], pc)
        for c, got in zip(cs, preds):
            assert np.array_equal(got.ravel(), c["pred"]), {k: v for k, v in c.items() if k != "pred"}
            n += 1
    enc.close()
    return n


def _remap_edge(r, tall, remapped):
    """luma cases of aspect ratio 2^r at the edge of getWideAngle's substitution: the last mode it remaps (2 + modeShift - 1 for wide blocks, mirrored for tall ones) or the
    first it leaves alone; a wrong modeShift entry for that ratio moves one of the two"""
    m = (0, 6, 10, 12, 14, 15)[r] + (1 if remapped else 2)
    return lambda c: c["comp"] == 0 and ((c["h"], c["w"]) if tall else (c["w"], c["h"])) == (c["h" if tall else "w"], c["h" if tall else "w"] >> r) and c["mode"] == (68 - m if tall else m)


INTRA_NEED = (lambda c: c["x"] == 0 and c["y"] == 0, lambda c: c["mrl"] == 3, lambda c: c["comp"] == 2 and c["h"] == 4) + tuple(
    _remap_edge(r, tall, remapped) for r in (1, 2, 3, 4) for tall in (0, 1) for remapped in (1, 0))
CCLM_NEED = (lambda c: c["mode"] == 67, lambda c: c["mode"] == 68, lambda c: c["mode"] == 69, lambda c: c["w"] * c["h"] == 64 * 64 and c["x"] > 0 and c["y"] > 0)      # the last: luma kept in the scratch slice


def _mip_range(lib, bd, step=1):
    vv = importlib.import_module(PKGNAME + ".vvcx")
    g = np.load(os.path.join(G, "mip_range.npz"))
    meta = g["meta"].astype(np.int64)
    ro = np.concatenate([[0], np.cumsum(meta[:, 1] + meta[:, 2])]); po = np.concatenate([[0], np.cumsum(meta[:, 1] * meta[:, 2])])
    idx = [i for i in range(len(meta)) if meta[i, 0] == bd][::step]
    cases = np.stack([meta[idx, 1], meta[idx, 2], meta[idx, 3], meta[idx, 0]], axis=1).astype(np.int32)
    refs = np.concatenate([g["refs"][ro[i]:ro[i + 1]] for i in idx]); exp = [g["preds"][po[i]:po[i + 1]] for i in idx]
    got = vv.mip_pred_batch(cases, refs, lib_path=lib)
    off = 0
    for i, e in zip(idx, exp):
        assert np.array_equal(got[off:off + len(e)], e), tuple(meta[i]); off += len(e)
    return len(idx)


def _dist_range(lib, bd, shapes=None):
    """all patterns of a shape in one launch (one workgroup per pair of blocks)"""
    from test_oracle_golden import _dist_range_cases
    groups = {}
    for c in _dist_range_cases():
        if c[2] == bd and (shapes is None or (c[0], c[1]) in shapes):
            groups.setdefault((c[0], c[1]), []).append(c)
    n = 0
    for (w, h), cs in groups.items():
        got = pkg.distortion_batch(np.concatenate([c[7] for c in cs]), np.concatenate([c[8] for c in cs]), w, h, lib_path=lib)
        for c, r in zip(cs, got):
            assert (int(r[0]), int(r[1]), int(r[2])) == (c[4], c[3], c[5]), ("sad, satd, sse", w, h, bd, "pattern", c[6])
            n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_intra_prediction_matches_reference_at_every_shape_and_range_edge(bd):
    assert _shapes(None, "intra_shapes_%d" % bd, bd) == 4957


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_cclm_prediction_matches_reference_at_every_shape_and_parameter_branch(bd):
    """cclm_prepare + cclm_params + chroma_pred_wave, as the chroma search sets them up, through modes 67 / 68 / 69 of vvcx_intra_pred_batch"""
    assert _shapes(None, "cclm_shapes", bd) == 1596


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_mip_prediction_matches_reference_on_saturated_lines(bd):
    assert _mip_range(None, bd) == 257


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10])
def test_gpu_distortion_matches_reference_at_the_ends_of_the_range(bd):
    assert _dist_range(None, bd) == 324


def test_emulated_leaf_operators_match_reference_at_shapes_and_range_edges(emu_so):
    """slices of the shape and range fixtures through the CPU emulation of the same sources: small blocks spread over the fixtures plus the corner without neighbours, MRL 3, the
    two modes at the edge of the wide-angle substitution for every aspect ratio and orientation, a chroma block two samples high, every CCLM mode, a CCLM block that keeps its luma in the scratch slice, MIP on every fourth case,
    every saturated SAD / SATD pattern on each Hadamard tile shape"""
    for bd in (8, 10):
        assert _shapes(emu_so, "intra_shapes_%d" % bd, bd, 30, INTRA_NEED) == 30 + len(INTRA_NEED)
        assert _shapes(emu_so, "cclm_shapes", bd, 24, CCLM_NEED) == 24 + len(CCLM_NEED)
        assert _mip_range(emu_so, bd, 4) == 65
        assert _dist_range(emu_so, bd, ((2, 2), (2, 16), (4, 4), (8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (64, 16))) == 9 * 9


def _deblock_range(lib, want):
    import oracle_lib as O
    return O.check_deblock_range(lambda pl, rows, bd, qp, qpc, boff, toff: pkg.vvcx.deblock_cu_table(pl, rows, bd, qp, qpc, boff, toff, lib_path=lib), want)


def _sao_range(lib, want):
    import oracle_lib as O
    return O.check_sao_range(lambda pl, bd, prm, tc, tr, lf, sc: pkg.vvcx.sao_picture(pl, bd, prm, tc, tr, lf, sc, lib_path=lib), want)


def _alf_range(lib, want):
    import oracle_lib as O
    return O.check_alf_range(lambda pl, bd, prm: pkg.vvcx.alf_picture(pl, bd, prm, want_classes=True, lib_path=lib), want)


@pytest.mark.gpu
@pytest.mark.parametrize("bd,n", [(8, 47), (10, 4), (12, 4)])
def test_gpu_deblocking_matches_reference_at_qp_limits_offsets_and_range_edges(bd, n):
    """vvcx_deblock_cu_table against the REFERENCE's filtered planes of tests/golden/deblock_range*.npz: QP 0..63, offsets that clip the table indices, tc = 0 / beta = 0 alone,
    Cb != Cr, every pair of transform sizes on every kind of edge, forced ISP splits"""
    assert _deblock_range(None, lambda m: m[0] == bd) == n


@pytest.mark.gpu
@pytest.mark.parametrize("bd,n", [(8, 13), (10, 14), (12, 13)])
def test_gpu_sample_adaptive_offset_matches_reference_at_offset_limits_and_range_edges(bd, n):
    """vvcx_sao_picture against the REFERENCE's planes of tests/golden/sao_range.npz: offsets of +-max and +-1, offset scales 0 / 2 / 4, the band wrap, both clips, tiles, 1032 samples wide"""
    assert _sao_range(None, lambda m: m[2] == bd) == n


@pytest.mark.gpu
@pytest.mark.parametrize("bd,n", [(8, 10), (10, 12), (12, 10)])
def test_gpu_adaptive_loop_filter_matches_reference_at_coefficient_limits_and_range_edges(bd, n):
    """vvcx_alf_picture (planes and block classes) against the REFERENCE's of tests/golden/alf_range.npz: coefficients of +-127, every clipping index on every tap, partial CTUs,
    every (fixed filter set, class) pair"""
    assert _alf_range(None, lambda m: m[2] == bd) == n


def test_emulated_loop_filters_match_reference_at_limits_and_range_edges(emu_so):
    """the cases of the three loop-filter range fixtures that the CPU emulation of the kernel sources can afford (oracle_lib.DEBLOCK_EMU / SAO_EMU / ALF_EMU): deblocking with
    both table indices clipped at either end, tc = 0 alone, beta = 0 alone, Cb != Cr, 10 and 12 bit, forced ISP; SAO wider than 1024 samples and with the largest offsets on
    pictures at the ends of the range; ALF with +-127 coefficients on the small pictures and with every fixed filter set on every class"""
    import oracle_lib as O
    assert _deblock_range(emu_so, O.DEBLOCK_EMU) == 10
    assert _sao_range(emu_so, O.SAO_EMU) == 13
    assert _alf_range(emu_so, O.ALF_EMU) == 13


@pytest.mark.gpu
def test_mip_prediction():
    """Device MIP prediction (vvcx_mip.hip: one wave per block, closed-form up-sampling) against MatrixIntraPrediction of the reference:
    every allowed block shape, every mode incl. the transposed half, 8 and 10 bit."""
    import importlib
    vv = importlib.import_module("reduce-complexity-for-intra-coding-of-vvc_amd.vvcx")
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mip.npz"))
    cases = np.stack([g["meta"][:, 1], g["meta"][:, 2], g["meta"][:, 3], g["meta"][:, 0]], axis=1).astype(np.int32)
    assert np.array_equal(vv.mip_pred_batch(cases, g["refs"]), g["preds"])


# ---- residual coding in its four forms and the arithmetic coder (tests/golden/residual_range.npz, arith_range.npz) ----
_RC_CASES = []


def _rc_cases():
    """the cases of residual_range.npz, regenerated once"""
    import oracle_lib as O
    if not _RC_CASES:
        _RC_CASES.extend(O.residual_range_expected())
    return _RC_CASES


def _rc_form_takes(c, form):
    """what a form exists for: the wave forms have no transform-skip syntax, form 1 stages at most 256 levels in the wave's LDS slot (the blocks the search keeps there)"""
    return not (form in (1, 2) and c["mi"] == 1) and not (form == 1 and c["w"] * c["h"] > 256)


def _residual_range(lib, form, comp, pick=lambda c: True):
    import oracle_lib as O
    vv = importlib.import_module(PKGNAME + ".vvcx")
    cases = [c for c in _rc_cases() if c["comp"] == comp and _rc_form_takes(c, form) and pick(c)]
    return O.check_residual_range(lambda *a: vv.residual_coding_batch(*a, lib_path=lib), form, cases)


def _arith_range(lib, step=1):
    vv = importlib.import_module(PKGNAME + ".vvcx")
    g = np.load(os.path.join(G, "arith_range.npz"))
    o_off = b_off = n = 0
    for i, (qp, nops, nbytes) in enumerate(g["meta"]):
        ops = g["ops"][o_off:o_off + 3 * nops]; o_off += 3 * int(nops)
        exp = g["bytes"][b_off:b_off + nbytes]; b_off += int(nbytes)
        if i % step == 0:
            assert np.array_equal(vv.arith_encode(int(qp), ops, lib_path=lib), exp), (i, qp, ops[:12])
            n += 1
    return n


def _rc_emu_pick():
    """the cases the CPU emulation runs: for every branch counter of the oracle one case that raises it, every kind of pattern on its smallest block, the block with more
    than 64 models in a run, and a thin spread over the rest; blocks of at most 256 levels, but for the skipped groups of a zeroed area, which need 16 x 32"""
    import ctypes as C
    import oracle_lib as O
    from test_oracle_golden import _orc_residual_leaf
    L = O.lib()
    cnt = np.zeros(O.RC_COUNTERS, np.int64)
    small = [c for c in _rc_cases() if c["w"] * c["h"] <= 256 or (c["w"], c["h"], c["pat"]) == (16, 32, O.RC_NOISE)]
    need = set(range(O.RC_COUNTERS)) - {O.RC_MAX_MODELS_IN_64} - set(O.RC_REM + (p * 4 + r) * 3 + f for (p, r, f) in O.RC_REM_UNREACHABLE)
    ids = set()
    for c in small:
        L.orc_residual_counters(cnt.ctypes.data_as(C.c_void_p))
        _orc_residual_leaf(L, c, 0)
        L.orc_residual_counters(cnt.ctypes.data_as(C.c_void_p))
        hit = set(np.flatnonzero(cnt).tolist()) & need
        if hit or c["pat"] == O.RC_CHAIN:
            ids.add(c["i"]); need -= hit
    assert not need, sorted(need)
    ids |= set(c["i"] for c in small[::40])
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_gpu_residual_coding_forms_match_reference_at_range_edges(form, comp):
    """vvcx_residual_coding_batch on every vector of residual_range.npz: the single-lane estimator, the wave estimator from LDS and from device memory (rc_chain with more
    than 64 models in a round among them) return the stored bits, end states of all models and last position; the writer returns the bytes the REFERENCE's reader parsed"""
    n = _residual_range(None, form, comp)
    assert n == len([c for c in _rc_cases() if c["comp"] == comp and _rc_form_takes(c, form)]) and n > 1000


@pytest.mark.gpu
def test_gpu_transform_skip_bits_of_the_leaf_and_of_the_batch_agree():
    """the bits vvcx_transform_skip_batch reports for the levels it chose are the bits form 0 of vvcx_residual_coding_batch spends on the same levels from the same states"""
    from test_oracle_golden import _range_cases
    vv = importlib.import_module(PKGNAME + ".vvcx")
    n = 0
    for c in _range_cases("d")[::4]:
        s0, s1 = c["ctx"]
        l, o, aa, kk, bits = vv.transform_skip_batch(c["resi"], c["w"], c["h"], c["bd"], c["qp"] + 6 * (c["bd"] - 8), c["lam"], s0, s1)
        if aa[0] > 0:
            b0 = vv.residual_coding_batch(l, c["w"], c["h"], 0, 0x40, 1, 1, 1, s0, s1, 0)[0]
            assert int(b0[0]) == int(bits[0]), (c["bd"], c["qp"], c["w"], c["h"], c["pat"])
            n += 1
    assert n > 30


@pytest.mark.gpu
def test_gpu_arithmetic_coder_matches_reference_at_range_edges():
    """vvcx_arith_encode (arith_bin, arith_bins_ep, arith_trm, arith_write_out, arith_finish) on every constructed string of arith_range.npz: the REFERENCE's bytes"""
    assert _arith_range(None) == 728


def test_emulated_residual_coding_forms_and_arithmetic_coder_match_reference(emu_so):
    """a slice of residual_range.npz with at least one case per branch counter, and every seventh string of arith_range.npz, through the CPU emulation of the kernel sources"""
    ids = _rc_emu_pick()
    pick = lambda c: c["i"] in ids
    for comp in (0, 1):
        ns = [_residual_range(emu_so, form, comp, pick) for form in range(4)]
        assert ns[0] == ns[3] >= ns[2] >= ns[1] > 20, ns
    assert _arith_range(emu_so, 7) == 104
