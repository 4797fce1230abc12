#!/usr/bin/env python3
"""Generate tests/golden/ctu_syntax.npz for tests/test_ctu_syntax.py (the cases, the restated syntax and the decoder live there).

Runs in the authoring container: the device code on the CPU emulator (tools/hipemu/build/libvvcx_emu.so) and the reference's arithmetic coder and model update from
oracle/_ref/libvtmref.so (ref_arith_encode, ref_ctx_code_bins, ref_ctx_init).  Asserts, per case, the five steps of the test file's docstring; stores only what the
tests compare with: the model start states and rates, per (configuration, tile) the all-off operation trace (the coding trees), per (configuration, variant, tile) the
bytes and sub-stream sizes - bytes that the reference's coder produced from the trace - and for later WPP rows the states the row starts from."""
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ctu_syntax as T      # noqa: E402

R = C.CDLL(os.path.join(ROOT, "oracle/_ref/libvtmref.so"))
R.ref_arith_encode.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
R.ref_ctx_init.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3
R.ref_ctx_code_bins.restype = C.c_uint64
R.ref_ctx_code_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_uint8, C.c_void_p, C.c_int]
P = lambda a: a.ctypes.data


def ref_encode(qp, ops):
    o, out = np.ascontiguousarray(ops, np.int32), np.zeros(1 << 16, np.uint8)
    n = R.ref_arith_encode(qp, P(o), len(o), P(out), len(out))
    assert n > 0
    return out[:n].copy()


def ref_states_after(s0, s1, rate, ops):
    """the reference's model update over the context-coded bins of ops, model by model (the models are independent of one another)"""
    s0, s1 = s0.copy(), s1.copy()
    for c in sorted({int(a) for k, a, b in ops if k == 0}):
        bins = np.array([b for k, a, b in ops if k == 0 and a == c], np.uint8)
        a0, a1 = s0[c:c + 1].copy(), s1[c:c + 1].copy()
        R.ref_ctx_code_bins(P(a0), P(a1), int(rate[c]), P(bins), len(bins))
        s0[c], s1[c] = a0[0], a1[0]
    return s0, s1


def main():
    fix = {}
    qp = T.pkg.slice_params(42)["qp"]
    s0, s1, rate = np.zeros(T.NUM_CTX, np.uint16), np.zeros(T.NUM_CTX, np.uint16), np.zeros(T.NUM_CTX, np.uint8)
    R.ref_ctx_init(qp, 2, P(s0), P(s1), P(rate))
    fix["init/s0"], fix["init/s1"], fix["rate"] = s0, s1, rate
    # the flat indices of the six sets, confirmed against the I-slice and rate rows of CL/Contexts.cpp:655-669, 823-853
    tab = (C.c_uint8 * T.NUM_CTX)()
    assert R.ref_ctx_init_table(2, tab) == T.NUM_CTX
    assert [tab[i] for i in T.NEW_MODELS] == [59, 5, 39, 39, 39, 54, 39, 39, 31, 62, 39, 44, 44, 31, 35]
    assert R.ref_ctx_init_table(3, tab) == T.NUM_CTX and not any(tab[i] for i in T.NEW_MODELS)
    seen = set()
    for name, cfg in T.CONFIGS.items():
        ses = T.Session(cfg, T.EMU_SO)
        ses.search()
        pay, tree = ses.rewrite((0, 0, 0, 0, 0), None, None)
        for t in range(ses.ntiles):                                              # 1
            assert np.array_equal(pay[t][0], ses.searched[t][0]) and np.array_equal(pay[t][1], ses.searched[t][1])
            fix["%s/tree/%d" % (name, t)] = tree[t]
        for vname, hdr, sao, alf in cfg["variants"]:
            pay, ops = ses.rewrite(hdr, sao, alf)
            for t, subs in enumerate(T.tile_ctus(cfg)):
                key = "%s/%s/%d" % (name, vname, t)
                got_subs, tree_subs = T.split_subs(ops[t]), T.split_subs(tree[t])
                assert len(got_subs) == len(subs) == len(pay[t][1])
                at, firsts = 0, []
                for r, ctus in enumerate(subs):
                    got, want = T.split_ctus(got_subs[r]), T.split_ctus(tree_subs[r])
                    assert len(got) == len(want) == len(ctus)
                    for k, addr in enumerate(ctus):
                        head = T.ctu_header_ops(cfg, hdr, sao, alf, addr)
                        assert got[k][:len(head)] == head, (key, addr, got[k][:len(head) + 2], head)      # 3
                        assert got[k][len(head):] == want[k], (key, addr)                                   # 2
                        seen.update((o[1], o[2]) for o in head if o[0] == 0)
                    data = pay[t][0][at:at + int(pay[t][1][r])]
                    at += int(pay[t][1][r])
                    if r == 0:
                        assert np.array_equal(ref_encode(qp, got_subs[0]), data), key                       # 4
                        assert T.decode_ops(data, s0.copy(), s1.copy(), rate, got_subs[0]), key             # (b) reads back every bin the reference coder wrote
                    else:                                                                                   # 5
                        a0, a1 = ref_states_after(s0, s1, rate, [o for c in firsts for o in c])
                        fix[key + "/start/%d/s0" % r], fix[key + "/start/%d/s1" % r] = a0, a1
                        assert T.decode_ops(data, a0.copy(), a1.copy(), rate, got_subs[r]), key
                        assert not T.decode_ops(data, s0.copy(), s1.copy(), rate, got_subs[r]), key         # not from the initial states
                        b0, b1 = a0.copy(), a1.copy()                                                       # nor with only the new models left at their start:
                        b0[list(T.NEW_MODELS)], b1[list(T.NEW_MODELS)] = s0[list(T.NEW_MODELS)], s1[list(T.NEW_MODELS)]
                        moved = any(a0[i] != s0[i] or a1[i] != s1[i] for i in T.NEW_MODELS)
                        assert moved and not T.decode_ops(data, b0, b1, rate, got_subs[r]), key              # they moved before the sync point and the sync carries them
                    firsts.append(got[0])
                assert at == len(pay[t][0])
                fix[key + "/bytes"], fix[key + "/sizes"] = pay[t][0], np.asarray(pay[t][1], np.int32)
        ses.close()
    # coverage of the new models: every one of the 15 coded with both bin values somewhere - the three ctbAlfFlag contexts of each component included
    assert seen == {(c, b) for c in T.NEW_MODELS for b in (0, 1)}, sorted({(c, b) for c in T.NEW_MODELS for b in (0, 1)} - seen)
    np.savez_compressed(T.FIXTURE, **fix)
    print("wrote", T.FIXTURE, os.path.getsize(T.FIXTURE), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
