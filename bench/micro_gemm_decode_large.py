"""Microbenchmark: the decode GEMM at M = 32 / 64 / 128 rows for the Llama-3-8B
projections in the modes the fused decode layer uses (qkv: split-K slabs; o / down: split-K +
last-arriver residual update; gate/up: row-norm scale + SiLU*mul), every (wr, kc, sk) tile that
exists for the row count, tile-order packed weights, against hipBLASLt.

Cold-cache protocol as bench/micro_gemm_decode.py (>= 1.5 GiB of distinct weight copies cycled in a
hipGraph). One JSON line per (shape, M, variant): us per call and effective weight GB/s.

    python bench/micro_gemm_decode_large.py [M ...]
    python bench/micro_gemm_decode_large.py [M ...] --w8    # M in 33 .. 128: the wide W8A16 GEMM against the bf16 one
"""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from src import ops  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from micro_gemm_decode import timeit  # noqa: E402

SHAPES = {  # name: (N_out, K, mode)
    "qkv_8b": (6144, 4096, 2),
    "o_8b": (4096, 4096, 3),
    "gate_up_8b": (14336, 4096, 4),
    "down_8b": (4096, 14336, 3),
}
TILES = [(32, 256), (48, 256), (64, 256), (32, 128), (48, 128), (64, 128), (96, 128), (112, 128), (128, 128),
         (64, 64), (128, 64), (64, 32), (128, 32)]


def splits(n, k, mode, wr, kc):
    cols = wr // 2 if mode == 4 else wr
    if n % cols:
        return []
    if mode == 4:
        return [1]
    out = []
    for sk in (1, 2, 4, 8):
        if k % (kc * sk) == 0 and (mode != 3 or wr in (32, 64, 128)):
            t = n // cols * sk
            if 96 <= t <= 1024:
                out.append(sk)
    return out


def capture(fn, ws):
    """A hipGraph of one call of fn per weight copy (cold weights: the copies exceed every cache), and its call count."""
    for w in ws[:2]:
        fn(w)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for w in ws:
            fn(w)
    torch.cuda.synchronize()
    return g, len(ws)


def main_w8(ms, rounds=7):
    """`--w8`: the wide W8A16 decode GEMM (ops.gemm_decode_w8_wide) at every W8 tile that divides the shape x its split
    counts against the bf16 decode GEMM as an FP8-weight engine runs it above 32 rows without the wide kernel
    (ops.linear_slab / ops.linear_silu_mul on the row-major weights, the bucket's tuned tile). Cold weights; every
    variant is captured first, then the graphs are replayed in turn, `rounds` times: best, median and worst us per
    call, and the weight bytes per second of the median."""
    dev = torch.device("cuda:0")
    for name, (n, k, mode) in SHAPES.items():
        silu = mode == 4
        rows = 2 * n if silu else n
        copies = max(2, int(1.5 * 2**30 // (rows * k * 2)) + 1)
        ws = [torch.randn(rows, k, device=dev, dtype=torch.bfloat16) / 64 for _ in range(copies)]
        qs = [torch.randint(0, 0x78, (rows, k), device=dev, dtype=torch.uint8) for _ in range(2 * copies)]  # timing only
        sc = torch.ones(rows, device=dev)
        for m in ms:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            wr, kc, sk = ops.decode_tile(n, k, ops.MODE_SILU if silu else ops.MODE_SLAB, ops.decode_bucket(m))
            runs = [("bf16", wr, kc, sk, 2) + capture((lambda w: ops.linear_silu_mul(x, w)) if silu else
                                                      (lambda w: ops.linear_slab(x, w)), ws)]
            for wr8, kc8 in ops.W8_TILES:
                if n % (wr8 // 2 if silu else wr8) or k % kc8:
                    continue
                for sk8 in ((1,) if silu else (1, 2, 4, 8)):
                    fn = lambda q, t=(wr8, kc8, sk8): ops.gemm_decode_w8_wide(  # noqa: E731
                        x, q, sc, ops.W8_SILU if silu else ops.W8_SLAB, *t)
                    runs.append(("w8_wide", wr8, kc8, sk8, 1) + capture(fn, qs))
            us = [[] for _ in runs]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(rounds):
                for i, r in enumerate(runs):
                    s.record()
                    r[5].replay()
                    e.record()
                    torch.cuda.synchronize()
                    us[i].append(s.elapsed_time(e) * 1e3 / r[6])
            for (kernel, w_, k_, s_, bpw, _, _), t in zip(runs, us):
                print(json.dumps({"bench": "w8_wide_micro", "shape": name, "M": m, "kernel": kernel, "wr": w_, "kc": k_,
                                  "sk": s_, "us_best": round(min(t), 2), "us_median": round(statistics.median(t), 2),
                                  "us_worst": round(max(t), 2),
                                  "weight_GBps": round(rows * k * bpw / statistics.median(t) / 1e3, 1)}), flush=True)
            del runs
        del ws, qs
        torch.cuda.empty_cache()


def main():
    if "--w8" in sys.argv[1:]:
        return main_w8([int(a) for a in sys.argv[1:] if a != "--w8"] or [64, 128])
    ms = [int(a) for a in sys.argv[1:]] or [32, 64, 128]
    dev = torch.device("cuda:0")
    for name, (n, k, mode) in SHAPES.items():
        rows = 2 * n if mode == 4 else n
        wbytes = rows * k * 2
        copies = max(2, int(1.5 * 2**30 // wbytes) + 1)
        ws = [torch.randn(rows, k, device=dev, dtype=torch.bfloat16) / 64 for _ in range(copies)]
        for m in ms:
            x = torch.randn(m, k, device=dev, dtype=torch.bfloat16)
            res = []
            if mode == 4:
                res.append(("hipblaslt+silu", timeit(lambda w: ops.silu_and_mul(torch.nn.functional.linear(x, w)), ws)))
            else:
                res.append(("hipblaslt", timeit(lambda w: torch.nn.functional.linear(x, w), ws)))
            resid = torch.randn(m, n, device=dev, dtype=torch.bfloat16)
            ssp_in = torch.ones(1, ops.SSP_LD, device=dev) * k
            for wr, kc in TILES:
                for sk in splits(n, k, mode, wr, kc):
                    wts = [ops.gd_pack_weights(w, wr, silu=mode == 4, kc=kc) for w in ws[:2]]
                    wts = (wts * ((copies + 1) // 2))[:copies]
                    try:
                        if mode == 2:
                            fn = lambda w: ops.gemm_decode(x, w, ops.MODE_SLAB | ops.TILED, wr, sk, kc=kc)  # noqa: E731
                        elif mode == 3:
                            ssp = torch.zeros(n // wr, ops.SSP_LD, device=dev)
                            cnt = torch.zeros(n // wr, dtype=torch.int32, device=dev)
                            fn = lambda w, ssp=ssp, cnt=cnt: ops.linear_slab_residual(  # noqa: E731
                                x, w, resid, ssp, cnt, wr, sk, tiled=True, kc=kc)
                        else:
                            fn = lambda w: ops.linear_silu_mul_rownorm(x, w, ssp_in, 1e-5, wr, tiled=True, kc=kc)  # noqa: E731
                        fn(wts[0])
                        torch.cuda.synchronize()
                    except RuntimeError:
                        continue  # no image of this many rows for the tile
                    # the packed copies alias 2 buffers: use real distinct copies for the cold protocol
                    wts = [ops.gd_pack_weights(w, wr, silu=mode == 4, kc=kc) for w in ws]
                    res.append((f"gd_wr{wr}_kc{kc}_sk{sk}", timeit(fn, wts)))
                    del wts
            base = res[0][1]
            for nm, us in sorted(res, key=lambda r: r[1]):
                print(json.dumps({"shape": name, "m": m, "variant": nm, "us": round(us, 2),
                                  "gbps": round(wbytes / us / 1e3, 1), "vs_hipblaslt": round(base / us, 3)}),
                      flush=True)
        del ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
