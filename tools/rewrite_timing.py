"""python tools/rewrite_timing.py [OUT.json] - timing of vvcx_rewrite_payload_bound_frames (device events: vvcx_last_rewrite_ms) beside vvcx_last_kernel_ms of the search, on
the same 18 bound 1080p pictures, for 15 x 9 tiles and for one tile per picture.  Those two searches run the cheapest tool set (VVCX_TOOL_CU_REUSE alone) at QP 45,
so the pass looks large beside them; a third case searches with the shipped tool set (0xfff) at QP 32, 15 x 9 tiles.  Each case records its tool set and QP.  The pass is serial per tile (one lane codes the tile's CTUs), so the tile count is what
decides its time.  SAO and ALF are on for every component with random, codable parameters.  No threshold: the file is the record of a pass nobody had measured"""
import importlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.init()
pkg = importlib.import_module("reduce-complexity-for-intra-coding-of-vvc_amd")
out = {"command": "python tools/rewrite_timing.py [OUT.json]", "pictures": 18, "method": "vvcx_last_rewrite_ms / vvcx_last_kernel_ms (HIP events); rewrite: 2 warm-up calls, median of 5",
       "cases": []}
N, W, H, bd = 18, 1920, 1080, 8
cw, ch = (W + 127) // 128, (H + 127) // 128


def sao_params(rng, tc, tr):
    """random parameters the syntax can carry: off / band / edge per channel type (Cb and Cr share the type), merges only where the candidate lies in the tile"""
    tile = [max(i for i in range(tr) if a // cw >= (i * ch) // tr) * tc + max(i for i in range(tc) if a % cw >= (i * cw) // tc) for a in range(cw * ch)]
    prm = np.zeros((N, cw * ch, 3, 7), np.int8)
    for f in range(N):
        for a in range(cw * ch):
            k = rng.integers(0, 8)
            if k == 0 and a % cw and tile[a - 1] == tile[a]:
                prm[f, a, :, 0] = 2
            elif k == 1 and a >= cw and tile[a - cw] == tile[a]:
                prm[f, a, :, 0], prm[f, a, :, 1] = 2, 1
            else:
                for c0, c1 in ((0, 1), (1, 3)):
                    typ = rng.integers(-1, 5)
                    if typ < 0:
                        continue
                    for c in range(c0, c1):
                        off = rng.integers(0, 8, 4)
                        prm[f, a, c] = [1, typ, rng.integers(0, 32) if typ == 4 else 0] + list(off * rng.choice([-1, 1], 4) if typ == 4 else off * [1, 1, -1, -1])
    return prm


for tc, tr, tools, qp in ((15, 9, pkg.TOOL_CU_REUSE, 45), (1, 1, pkg.TOOL_CU_REUSE, 45), (15, 9, 0xfff, 32)):
    rng = np.random.default_rng(7)
    sp = pkg.slice_params(qp, bit_depth=bd, dep_quant=bool(tools & pkg.TOOL_DEPQUANT))
    base = pkg.synth_frame(W, H, 0, bd, 1000, chroma_texture=0.5)
    enc = pkg.VvcxEncoder(W, H, bd, tile_cols=tc, tile_rows=tr, tools=tools, max_frames=N, emit_payload=True)
    enc.set_slice(sp["qp"], sp["qp_c"], sp["lam"], sp["dist_weight"])
    org = [[torch.roll(torch.from_numpy(p).cuda(), 8 * i, 1) for p in base] for i in range(N)]
    rec = [[torch.zeros_like(t) for t in f] for f in org]
    enc.bind_frames([([t.data_ptr() for t in o], [t.data_ptr() for t in r], [t.shape[1] for t in o]) for o, r in zip(org, rec)])
    enc.compress_bound_frames()
    search_ms = enc.last_kernel_ms()
    print("search done", tc, tr, search_ms, flush=True)
    nbytes = sum(len(enc.get_payload(f, t)) for f in range(N) for t in range(tc * tr))
    sao = sao_params(rng, tc, tr)
    alf = [pkg.alf_test_params(123, W, H)] * N             # codable as generated: sets below 16 + the slice's count, alternatives below the chroma set's
    hdr = np.ones((N, 5), np.uint8)
    ms = sorted([enc.rewrite_payload(hdr, sao=sao, alf=alf) for rep in range(7)][2:])
    nbytes2 = sum(len(enc.get_payload(f, t)) for f in range(N) for t in range(tc * tr))
    off = sorted([enc.rewrite_payload(np.zeros((N, 5), np.uint8)) for rep in range(7)][2:])
    case = {"width": W, "height": H, "bit_depth": bd, "tile_cols": tc, "tile_rows": tr, "search_tools": hex(tools), "slice_qp": qp, "workgroups": N * tc * tr, "ctus_per_tile_max": -(-cw // tc) * -(-ch // tr),
            "search_kernel_ms": search_ms, "rewrite_ms": {"median": ms[2], "min": ms[0], "max": ms[-1]}, "rewrite_all_off_ms": {"median": off[2], "min": off[0], "max": off[-1]},
            "payload_bytes_search": nbytes, "payload_bytes_with_syntax": nbytes2, "rewrite_over_search": ms[2] / search_ms}
    print(case, flush=True)
    out["cases"].append(case)
    enc.close()
    del org, rec
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
