"""
Decode-GEMM (csrc/kernels/gemm_decode.hip) tile selection and tile geometry: the mode word, the instantiated
tiles, the row bucket, the one measured table and the one lookup. Pure Python (neither torch nor the extension),
so every choice can be pinned on a machine without a GPU (tests/test_decode_tiles_cpu.py). A new tile sweep's
winner is one line in DECODE_TILE_CFG.
"""

from __future__ import annotations

import math
import os
from typing import Optional

# The decode GEMM's mode word (_C.gemm_decode / gemm_decode_car / gd_occupancy): an epilogue, or-ed with flags.
MODE_BF16 = 0          # bf16 x @ w^T
MODE_SILU = 1          # bf16 silu(gate) * up, w = [gate; up]
MODE_SLAB = 2          # fp32 split-K slabs [sk, M, N], reduced by the consumer kernel
MODE_RESID = 3         # split-K, the last arriver adds into the residual and writes the next norm's statistics
MODE_SILU_NORM = 4     # MODE_SILU with the rows scaled by the RMSNorm statistics (norm weight folded into w)
MODE_SILU_NORM_SK = 6  # MODE_SILU_NORM split over sk K slices, the tile's last arriver finishes
MODE_MASK = 31
TILED = 32             # flag: w in tile order (ops.gd_pack_weights)
HALF_RING = 64         # flag: half-LDS ring, two workgroups per CU (MODE_RESID at <= 32 rows)
P13 = 128              # flag: w in the lossless 13-bit layout (ops.gd_pack_weights_p13): tile (128, 128), <= 32 rows,
P13_BASE_SHIFT = 8     # MODE_BF16 / MODE_SILU_NORM, nt loads; the tensor's base7 rides in mode bits 8..14

DECODE_GEMM_MAX_M = 128   # weight-streaming decode GEMM / fused decode path (gemm_decode.hip)
SSP_LD = 128              # row stride of the norm-statistics arrays [tiles, SSP_LD]
SSP_MAX_TILES = 256       # statistics tiles a consumer takes at <= 32 decode rows (launchers.h)
SSP_MAX_TILES_WIDE = 128  # ... above 32 rows

# The instantiated (wr, kc) tiles, in the order of csrc/kernels/gd_tiles.h's GD_TILES.
GD_TILES = ((32, 256), (48, 256), (64, 256), (32, 128), (48, 128), (64, 128), (96, 128), (112, 128), (128, 128),
            (64, 64), (128, 64), (64, 32), (128, 32))
# Candidates of the "grid closest to 256 workgroups" choice above 32 rows; the order decides ties.
GENERIC_TILES = ((64, 128), (128, 64), (32, 128), (64, 64), (128, 32), (64, 32), (112, 128), (96, 128), (48, 128),
                 (128, 128))
# LM head tiles tried in order (bench/micro_tp_tiles.py --shapes lm_head, cold, 32 rows: tile-order
# (128, 128) 171.8 us vs the row-major (64, 256) 187.0 us for Llama-3's 128,256 x 4,096)
LM_HEAD_TILES = ((128, 128), (64, 256), (64, 128))
assert set(GENERIC_TILES) | set(LM_HEAD_TILES) <= set(GD_TILES)

# Tile geometry: a mirror of gd_tiles.h (ring_slots / gd_lds / gd_valid), compared with it by the CPU tests.
LDS_BYTES = 160 * 1024  # LDS of a CU
RING_BYTES = 147456     # LDS for the ring (144 KiB; the epilogue scratch reuses it)


def ring_slots(wr: int, kc: int, xr: int) -> int:
    """LDS ring depth of a (wr, kc) tile with an xr-row activation image: the deepest that fits RING_BYTES and
    the 6-bit vmcnt."""
    per_wave = (wr + xr) // (64 // (kc // 8)) // 4
    s = min(8, RING_BYTES // ((wr + xr) * kc * 2))
    while s > 2 and (s - 1) * per_wave > 63:
        s -= 1
    return s


def gd_lds(wr: int, kc: int, xr: int) -> int:
    """LDS bytes of one launch: the ring, and after the loop the fp32 partials + scratch."""
    red = (4 if xr < 64 and kc >= 128 else 1) * max(xr, 32) * wr * 4 + 2048
    return max(ring_slots(wr, kc, xr) * (wr + xr) * kc * 2, red)


def gd_tile_valid(wr: int, kc: int, xr: int) -> bool:
    """A (wr, kc) tile has an xr-row activation image (mirror of gd_tiles.h gd_valid)."""
    rpp = 64 // (kc // 8)
    return (ring_slots(wr, kc, xr) >= 2 and (wr + xr) % (4 * rpp) == 0 and xr % rpp == 0 and wr % rpp == 0
            and not (xr < 64 and kc < 128 and wr % 64) and gd_lds(wr, kc, xr) <= LDS_BYTES)


def gd_tile(wr: int, kc: Optional[int] = None):
    """(weight rows, K slot) of a decode-GEMM tile; ``kc`` defaults to 128 for >= 96 rows, else 256."""
    return wr, (128 if wr >= 96 else 256) if kc is None else kc


def decode_bucket(m: int) -> int:
    """Row bucket of a decode step of m rows: the activation image of its GEMMs (32, 64 or 128 rows)."""
    return 32 if m <= 32 else (64 if m <= 64 else 128)


# (N, K, mode, row bucket) -> (wr, kc, sk): every measured decode-GEMM tile (MI355X, cold weights). Fastest configs
# put (N / cols) * sk at (a multiple of) ~256 workgroups, one per CU.
DECODE_TILE_CFG = {
    # Round 1, 32 rows: bench/micro_gemm_decode.py (M = 32, nt weight loads, row-major weights;
    # profiles/micro_gemm_decode_m32_r1b.jsonl). At <= 32 rows the mode-2 / mode-1 entries also stand in for a
    # mode 3 / 4 projection of the same shape (decode_tile)
    (6144, 4096, 2, 32): (48, 256, 2),      # Llama-3-8B / Mixtral qkv  (11.6 us vs hipBLASLt 15.3)
    (4096, 4096, 2, 32): (64, 256, 4),      # 8B o_proj                  (9.3 vs 13.3)
    (14336, 4096, 1, 32): (112, 128, 1),    # 8B gate/up + SiLU          (46.4 vs 53.4)
    (4096, 14336, 2, 32): (64, 256, 4),     # 8B down_proj               (22.2 vs 33.9)
    (128256, 4096, 0, 32): (64, 256, 1),    # Llama-3 LM head            (177 vs 190, 5.9 TB/s)
    (1280, 8192, 2, 32): (64, 256, 8),      # 70B TP=8 qkv               (7.8 vs 15.3)
    (8192, 1024, 0, 32): (32, 256, 1),      # 70B TP=8 o_proj            (6.3 vs 11.4)
    (3584, 8192, 1, 32): (32, 256, 1),      # 70B TP=8 gate/up + SiLU    (26.6 vs 29.7)
    (8192, 3584, 0, 32): (32, 256, 1),      # 70B TP=8 down_proj         (13.3 vs 15.6)
    # the fused decode layer's projections (mode 2 qkv slabs, 3 o / down residual update, 4 gate/up row-norm +
    # SiLU), Llama-3-8B shapes at 64 / 128 rows: bench/micro_gemm_decode_large.py (tile-order packed;
    # profiles/micro_gemm_decode_large_r2.jsonl)
    (6144, 4096, 2, 64): (96, 128, 4),     # qkv   15.0 us vs hipBLASLt 17.9
    (6144, 4096, 2, 128): (48, 128, 2),    #       20.2 vs 25.3
    (4096, 4096, 3, 64): (64, 128, 4),     # o     13.4 vs 15.3
    (4096, 4096, 3, 128): (32, 128, 2),    #       16.5 vs 24.6
    (14336, 4096, 4, 64): (112, 128, 1),   # gate/up + SiLU  45.6 vs 50.5
    (14336, 4096, 4, 128): (128, 64, 1),   #                 57.2 vs 54.7
    (4096, 14336, 3, 64): (64, 128, 4),    # down  28.3 vs 40.0
    (4096, 14336, 3, 128): (128, 64, 8),   #       38.3 vs 75.3
    # the bench's 32-row bucket, round-4 sweep (bench/micro_tp_tiles.py --shapes 8b, profiles/micro_8b_tiles_r4.jsonl,
    # cold us) confirmed in the real graph: bench 50.49 -> 51.45 req/s with all three, same box
    # (profiles/bench_r4_tile_ab.jsonl; gate/up alone 50.94, o alone 50.44). Until then mode 3 (split-K +
    # last-arriver residual update) ran o and down at (64, 256, 4): in isolation (micro_gemm_decode.py resid)
    # wr32/sk2 won by ~1 us, but inside the decode graph wr64/sk4 was faster (bench decode 4.07 -> 3.93 ms/step):
    # keep what the real step measures
    (4096, 4096, 3, 32): (32, 256, 2),     # o      13.96 vs 15.44 for (64, 256, 4)
    (14336, 4096, 4, 32): (128, 128, 1),   # gate/up + SiLU 42.08 vs 43.96 for (112, 128, 1)
    (4096, 14336, 3, 32): (64, 128, 4),    # down   29.6 vs 30.2 for (64, 256, 4)
    # tensor-parallel shards, 32 rows (bench/micro_tp_tiles.py, profiles/micro_tp_tiles_r4.jsonl, cold, us)
    # round 5: consumers take 256 statistics tiles at <= 32 rows, so the 70B shard's wr = 32 tiles (one workgroup
    # per CU, no split-K) are usable (bench/micro_tp_tiles.py --proj o,down, profiles/r5_tp8_tiles_wr32.jsonl):
    # o 10.00 vs 11.28 us for (64, 256, 1), down 17.20 vs 17.96 for (64, 128, 2); probe 5.74 -> 5.58 ms/step
    (8192, 1024, 3, 32): (32, 128, 1),     # 70B TP=8 o
    (8192, 3584, 3, 32): (32, 256, 1),     # 70B TP=8 down
    (4096, 2048, 3, 32): (32, 128, 2),     # 8B TP=2 o      11.48 vs 12.68
    (4096, 7168, 3, 32): (64, 128, 4),     # 8B TP=2 down   18.40 vs 18.88
    (3072, 4096, 2, 32): (48, 128, 4),     # 8B TP=2 qkv    11.08 vs 11.80
    (7168, 4096, 4, 32): (64, 128, 1),     # 8B TP=2 gate/up 24.84 vs 25.68
    (1280, 8192, 2, 64): (32, 256, 4),     # 70B TP=8 qkv at 64 rows  13.80 vs 14.40 for (32, 128, 4)
    (8192, 1024, 3, 128): (64, 64, 2),     # 70B TP=8 o at 128 rows   17.52 vs 18.20 for (64, 128, 2)
    # Llama-3-70B on ONE GPU (TP=1): decode streams the row-major weights (their tile-order copies do not fit beside
    # 141 GB); round-6 sweep (bench/micro_tp_tiles.py --shapes 70b --row-major, profiles/r6_70b_tp1_tiles.jsonl, cold us)
    (10240, 8192, 2, 32): (64, 256, 1),    # qkv            38.76 vs 43.68 for the generic (64, 256, 2)
    (10240, 8192, 3, 32): (64, 256, 2),    # no model's projection, not measured: the generic tile, which a mode-3
                                           # call got before the qkv entry above could stand in for it (rule 3)
    (28672, 8192, 4, 32): (112, 128, 1),   # gate/up + SiLU 165.76 vs 189.88 for (64, 256, 1)
    (8192, 28672, 3, 32): (128, 128, 4),   # down           80.68 vs 88.48 for (64, 256, 2)
    # the split-K gate/up (mode 6), where the full-K form's grid forces narrow tiles (bench/micro_gd_splitk_silu.py,
    # profiles/micro_gd_splitk_silu_r3.jsonl): Llama-3-70B's TP=8 shard 27.1 us vs 30.0 for the best full-K tile
    # (32, 256). Dense 8B shapes lose with split-K (not listed).
    (3584, 8192, 6, 32): (64, 128, 2),   # round 4 sweep (micro_tp_tiles_r4): 26.84 us vs 30.36 for (64, 256, 2) cold
    # 64 / 128 rows (micro_tp_tiles --rows 64 / 128, profiles/micro_tp_tiles_r4_rows64_128.jsonl, cold us)
    (3584, 8192, 6, 64): (112, 128, 4),  # 34.76 vs 41.28 for the full-K (32, 128)
    (3584, 8192, 6, 128): (64, 128, 2),  # 46.36 vs 52.12
}

# (N, K, mode, row bucket) -> (wr, kc, sk) where the decode GEMM streams the ROW-MAJOR weights by choice
# (EngineConfig.decode_weight_layout = single: the KV pool is the constraint, no tile-order copies), measured with
# bench/micro_tp_tiles.py --row-major; shapes not listed fall back to the tile-order table's choice
# Round 6, Llama-3-8B at 32 rows: the cold sweep's row-major winners (o (64, 256, 4) 14.44 vs 15.28 us, gate/up
# (64, 256, 1) 48.28 vs 53.68, profiles/r6_8b_rm_tiles.jsonl) LOST in the graph — decode 3.96 vs 3.76 ms/step,
# profiles/r6_decode_layout_rm_tiles_negative.jsonl — so the 8B shapes keep the tile-order table's tiles.
DECODE_TILE_CFG_RM: dict = {}


def _tile_overrides(spec: str) -> dict:
    """DIE_TILE_OVERRIDE="N,K,mode,bucket=wr,kc,sk;...": decode-GEMM tiles to try in the real graph (A/B runs of
    a micro-bench winner) without editing DECODE_TILE_CFG; mode 6 names the split-K SiLU gate/up tile."""
    out = {}
    for item in filter(None, (s.strip() for s in spec.split(";"))):
        key, val = item.split("=")
        out[tuple(int(v) for v in key.split(","))] = tuple(int(v) for v in val.split(","))
    return out


DECODE_TILE_CFG.update(_tile_overrides(os.environ.get("DIE_TILE_OVERRIDE", "")))


def _closest_to_256(n: int, k: int, mode: int, tiles, max_sk: int):
    """The first (wr, kc, sk) over ``tiles`` that divides [N, K] and brings the grid closest (in log2) to 256
    workgroups, one per CU; split-K only where the mode reduces slabs. None when no tile divides."""
    best, score = None, 1e9
    for wr, kc in tiles:
        cols = wr // 2 if mode in (MODE_SILU, MODE_SILU_NORM) else wr
        if n % cols:
            continue
        for sk in ((1, 2, 4, 8) if mode in (MODE_SLAB, MODE_RESID) else (1,)):
            if sk > max_sk or k % (kc * sk):
                continue
            sc = abs(math.log2((n // cols) * sk / 256.0))
            if sc < score - 1e-9:
                best, score = (wr, kc, sk), sc
    return best


def generic_tile(n: int, k: int, mode: int, bucket: int, max_sk: int = 8):
    """The (wr, kc, sk) of GENERIC_TILES that exists for ``bucket`` activation rows and brings the grid closest
    to 256 workgroups."""
    tiles = [(wr, kc) for wr, kc in GENERIC_TILES
             if (mode != MODE_RESID or wr in (32, 64, 128)) and gd_tile_valid(wr, kc, bucket)]
    best = _closest_to_256(n, k, mode, tiles, max_sk)
    if best is None:
        raise ValueError(f"no decode-GEMM tile for N={n} K={k} mode={mode} at {bucket} rows")
    return best


def decode_tile(n: int, k: int, mode: int, bucket: int = 32, max_sk: int = 8, row_major: bool = False):
    """(wr, kc, sk) of the decode GEMM for an [N, K] projection in ``mode`` at steps of up to ``bucket`` rows (32,
    64, 128) with at most ``max_sk`` K splits; ``row_major``: on weights kept row-major. The first that applies:

    1. DECODE_TILE_CFG_RM's entry (``row_major`` only), then
    2. DECODE_TILE_CFG's entry — each taken only if its sk <= ``max_sk`` and, for MODE_RESID (one statistics tile
       per wr output columns), N / wr is within what its consumers take (SSP_MAX_TILES at <= 32 rows,
       SSP_MAX_TILES_WIDE above).
    3. At <= 32 rows, MODE_RESID takes (wr, sk) from MODE_SLAB's 32-row choice — its entry under ``max_sk``, else
       rule 4 — and MODE_SILU_NORM takes MODE_SILU's: the round-1 measurements, made without those epilogues.
       MODE_RESID keeps wr in {32, 64, 128} dividing N (else 64, else 32) with the default K slot of :func:`gd_tile`,
       and halves sk until K splits into whole slots.
    4. The grid closest to 256 workgroups: at <= 32 rows over (64, 256) and (32, 256) — (64, 256, 1) when neither
       divides — above over GENERIC_TILES (:func:`generic_tile`, ValueError when none fits).
    """
    lim = SSP_MAX_TILES if bucket <= 32 else SSP_MAX_TILES_WIDE
    for table in ((DECODE_TILE_CFG_RM, DECODE_TILE_CFG) if row_major else (DECODE_TILE_CFG,)):
        c = table.get((n, k, mode, bucket))
        if c is not None and c[2] <= max_sk and (mode != MODE_RESID or n // c[0] <= lim):
            return c
    if bucket > 32:
        return generic_tile(n, k, mode, bucket, max_sk)
    base = {MODE_RESID: MODE_SLAB, MODE_SILU_NORM: MODE_SILU}.get(mode, mode)
    c = DECODE_TILE_CFG.get((n, k, base, 32)) if base != mode else None
    if c is None or c[2] > max_sk:
        c = _closest_to_256(n, k, base, ((64, 256), (32, 256)), max_sk) or (64, 256, 1)
    if mode == MODE_RESID:
        wr, _, sk = c
        if wr not in (32, 64, 128) or n % wr:
            wr = 64 if n % 64 == 0 else 32
        wr, kc = gd_tile(wr)
        while sk > 1 and k % (kc * sk):
            sk //= 2
        return wr, kc, sk
    return c


def decode_tile_silu(n: int, k: int, bucket: int = 32, row_major: bool = False):
    """(wr, kc, sk) of the norm-scaled SiLU gate/up decode GEMM: the split-K tile (MODE_SILU_NORM_SK) where one
    was measured faster, else the full-K tile (:func:`decode_tile` of MODE_SILU_NORM, sk = 1). ``row_major``:
    DECODE_TILE_CFG_RM's entry of either mode first."""
    key6, key4 = (n, k, MODE_SILU_NORM_SK, bucket), (n, k, MODE_SILU_NORM, bucket)
    c = (row_major and (DECODE_TILE_CFG_RM.get(key6) or DECODE_TILE_CFG_RM.get(key4))) or DECODE_TILE_CFG.get(key6)
    return c or (*decode_tile(n, k, MODE_SILU_NORM, bucket)[:2], 1)


def moe_decode_tiles(hdim: int, inter: int, t: int):
    """((wr, kc) of the gate/up grouped GEMM, (wr, kc) of the down one) for a decode step of t tokens, or
    None when the shapes do not tile. Up to 32 rows: round 1's measured choice (gate/up as the dense
    gate/up shape, down (64, 256)); above, the row bucket's generic tile."""
    if hdim % 32 or inter % 32:
        return None
    if t <= 32:
        wr1, kc1, _ = decode_tile(inter, hdim, MODE_SILU, 32)
        if not (hdim % 256 or inter % 256 or inter % (wr1 // 2) or hdim % 64):
            return (wr1, kc1), gd_tile(64)
    try:  # the row bucket's generic tiles (also for small shards, e.g. experts split under TP)
        b = decode_bucket(t)
        wr1, kc1, _ = generic_tile(inter, hdim, MODE_SILU, b, max_sk=1)
        wr2, kc2, _ = generic_tile(hdim, inter, MODE_BF16, b, max_sk=1)
    except ValueError:
        return None
    return (wr1, kc1), (wr2, kc2)
