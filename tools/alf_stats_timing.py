"""python tools/alf_stats_timing.py [OUT.json] - timing of vvcx_alf_statistics_bound_frames (device events: vvcx_last_alf_stats_ms) and of the ALF filter on the same 18 bound pictures; synthetic reconstructions written
straight into the reco planes behind the cheapest search (the handle wants every CTU coded)"""
import importlib, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.init()
pkg = importlib.import_module("reduce-complexity-for-intra-coding-of-vvc_amd")
out = {"command": "python tools/alf_stats_timing.py [OUT.json]", "pictures": 18, "method": "vvcx_last_alf_stats_ms / vvcx_last_alf_ms (HIP events), 2 warm-up calls, median of 5", "cases": []}
N = 18
for (W, H, bd, tc, tr) in ((1920, 1080, 8, 15, 9), (3840, 2160, 10, 30, 17)):
    sp = pkg.slice_params(45, bit_depth=bd)
    base = pkg.synth_frame(W, H, 0, bd, 1000, chroma_texture=0.5)
    enc = pkg.VvcxEncoder(W, H, bd, tile_cols=tc, tile_rows=tr, tools=pkg.TOOL_CU_REUSE, max_frames=N)
    enc.set_slice(sp["qp"], sp["qp_c"], sp["lam"], sp["dist_weight"])
    dt = torch.uint8 if bd == 8 else torch.int16
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    org = [[torch.roll(torch.from_numpy(p if bd == 8 else p.view(np.int16)).cuda(), 8 * i, 1) for p in base] for i in range(N)]
    rec = [[torch.zeros_like(t) for t in f] for f in org]
    enc.bind_frames([([t.data_ptr() for t in o], [t.data_ptr() for t in r], [t.shape[1] for t in o]) for o, r in zip(org, rec)])
    enc.compress_bound_frames()
    print("search done", W, H, enc.last_kernel_ms(), flush=True)
    mx = (1 << bd) - 1
    for o, r in zip(org, rec):
        for c in range(3):
            noise = torch.randint(-(3 << (bd - 8)), (3 << (bd - 8)) + 1, o[c].shape, device="cuda", generator=g)
            r[c].copy_(torch.clamp(o[c].to(torch.int32) + noise, 0, mx).to(dt))
    torch.cuda.synchronize()
    case = {"width": W, "height": H, "bit_depth": bd}
    for nb in (1, 4):
        chunk = N if nb == 1 else 3
        ms = []
        for rep in range(7):
            t = 0.0
            for f0 in range(0, N, chunk):
                l, c, m = enc.alf_statistics_bound_frames(f0, chunk, nb)
                t += m
            ms.append(t)
        del l, c
        ms = sorted(ms[2:])
        mfma = 1.5 * W * H / 4 * nb * nb * N
        case["stats_ms_%dbin" % nb] = {"median": ms[2], "min": ms[0], "max": ms[-1], "frames_per_call": chunk,
                                       "mfma_f64_16x16x4": mfma, "tflops": mfma * 2048 / (ms[2] * 1e-3) / 1e12}
        print(W, H, nb, case["stats_ms_%dbin" % nb], flush=True)
    prm = pkg.alf_test_params(123, W, H)
    fm = []
    for rep in range(7):
        fm.append(enc.alf_bound_frames([prm] * N))
    fm = sorted(fm[2:])
    case["alf_filter_ms"] = {"median": fm[2], "min": fm[0], "max": fm[-1]}
    print(W, H, "filter", case["alf_filter_ms"], flush=True)
    out["cases"].append(case)
    enc.close()
    del org, rec
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
