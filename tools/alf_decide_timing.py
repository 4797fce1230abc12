"""python tools/alf_decide_timing.py [OUT.json] [--cases 1080p,4k] - what the ALF decision costs per picture on 18 bound pictures (synthetic reconstructions written straight
into the reco planes behind the cheapest search, as tools/alf_stats_timing.py does):
 (a) the route over the host: vvcx_alf_statistics_bound_frames (with its download) + vvcx_alf_decide per picture, at 1 and 4 bins, wall time;
 (b) the resident route: vvcx_alf_statistics_resident + vvcx_alf_decide_resident with flags 0 (1 and 4 bins) and with all flags (4 bins), wall time;
 (c) the two kernels of csrc/vvcx_alf_eval.hip alone by HIP events (vvcx_last_alf_sum_ms / _cand_ms), the sum kernel also as bytes read / time.
2 warm-up repetitions, median of 5.  An existing OUT.json keeps the cases that are not measured again."""
import importlib, json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.cuda.init()
pkg = importlib.import_module("reduce-complexity-for-intra-coding-of-vvc_amd")
vv = importlib.import_module("reduce-complexity-for-intra-coding-of-vvc_amd.vvcx")
N, LAM = 18, [30.0, 30.0, 30.0]
CASES = {"1080p": (1920, 1080, 8, 15, 9), "4k": (3840, 2160, 10, 30, 17)}
args = [a for a in sys.argv[1:] if not a.startswith("--")]
names = ["1080p", "4k"]
for i, a in enumerate(sys.argv):
    if a == "--cases":
        names = [n for n in CASES if n in sys.argv[i + 1].split(",")]
out = {"command": "python tools/alf_decide_timing.py [OUT.json] [--cases 1080p,4k]", "pictures": N, "lambda": LAM[0],
       "method": "wall time (time.perf_counter around the calls, which block) and HIP events for the kernels; 2 warm-up repetitions, median of 5; ms per picture", "cases": {}}
if args and os.path.exists(args[0]):
    out["cases"] = json.load(open(args[0])).get("cases", {})


def stat(ms):
    ms = sorted(ms[2:])
    return {"median": ms[len(ms) // 2] / N, "min": ms[0] / N, "max": ms[-1] / N}


for name in names:
    W, H, bd, tc, tr = CASES[name]
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
    nctu = enc.ctus_per_frame
    case = {"width": W, "height": H, "bit_depth": bd, "ctus": nctu}
    for nb in (1, 4):
        szl, szc = vv.alf_stat_sizes(nb)
        chunk = N if nb == 1 else 3                              # the host copy of 4-bin statistics is about 550 KB per CTU
        host, dl = [], []
        for rep in range(7):
            t0 = time.perf_counter(); td = 0.0
            for f0 in range(0, N, chunk):
                t1 = time.perf_counter()
                l, c, _ = enc.alf_statistics_bound_frames(f0, chunk, nb)
                td += time.perf_counter() - t1
                for f in range(chunk):
                    vv.alf_decide(l[f], c[f], W, H, bd, LAM, n_bins=nb)
            host.append((time.perf_counter() - t0) * 1e3); dl.append(td * 1e3)
        del l, c
        case["host_route_ms_%dbin" % nb] = dict(stat(host), statistics_with_download=stat(dl), frames_per_call=chunk)
        print(name, nb, "host route", case["host_route_ms_%dbin" % nb], flush=True)
        for label, flags in (("flags0", 0),) + ((("all_flags", 7),) if nb == 4 else ()):
            res, kst = [], []
            for rep in range(7):
                t0 = time.perf_counter()
                kst.append(enc.alf_statistics_resident(0, N, nb))
                enc.alf_decide_resident(LAM, flags=flags)
                res.append((time.perf_counter() - t0) * 1e3)
            case["resident_route_ms_%dbin_%s" % (nb, label)] = dict(stat(res), statistics_kernel=stat(kst))
            print(name, nb, label, "resident route", case["resident_route_ms_%dbin_%s" % (nb, label)], flush=True)
        # the two kernels alone: all CTUs summed; the 16 fixed sets and one linear set per frame
        lc = np.zeros((N, 1), vv.ALF_LUMA_CAND); lc["coeff"][..., 6] = 20; lc["coeff"][..., 11] = 30
        cc = np.zeros((N, 1), vv.ALF_CHROMA_CAND); cc["coeff"][..., 2] = 20
        ksum, kcand = [], []
        for rep in range(7):
            enc.alf_frame_statistics(); ksum.append(enc.alf_pass_ms()[0])
            enc.alf_candidate_errors(True, lc, cc); kcand.append(enc.alf_pass_ms()[1])
        rd = N * nctu * (25 * szl + 2 * szc) * 8
        s = stat(ksum)
        case["sum_kernel_ms_%dbin" % nb] = dict(s, bytes_read=rd, gb_per_s=rd / (s["median"] * N * 1e-3) / 1e9)
        case["cand_kernel_ms_%dbin" % nb] = dict(stat(kcand), candidates_luma=17, candidates_chroma=1)
        print(name, nb, "kernels", case["sum_kernel_ms_%dbin" % nb], case["cand_kernel_ms_%dbin" % nb], flush=True)
    out["cases"][name] = case
    enc.close()
    del org, rec
    torch.cuda.empty_cache()
    if args:
        json.dump(out, open(args[0], "w"), indent=1)
print(json.dumps(out))
