"""Pins of the decode-GEMM tile selection (src/ops/decode_tiles.py) that need no GPU.

* The selection snapshot: what ``decode_tile`` / ``decode_tile_silu`` / ``moe_decode_tiles`` returned before the
  five tables became one (tests/golden/decode_tiles_snapshot.json, recorded from the five-table code and never
  regenerated from this module), compared row for row.
* The geometry parity: the C++ tile list and ``gd_valid`` / ``ring_slots`` / ``gd_lds`` of csrc/kernels/gd_tiles.h,
  printed by a stand-alone host program, against the Python tile tuple and ``gd_tile_valid``.
"""

import json
import os
import shutil
import subprocess

import pytest

from src.models.presets import PRESETS
from src.ops import decode_tiles as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAPSHOT = os.path.join(ROOT, "tests", "golden", "decode_tiles_snapshot.json")

MODES = (0, 1, 2, 3, 4)
BUCKETS = (32, 64, 128)
MOE_TOKENS = (1, 16, 32, 33, 64, 100, 128)


def preset_shapes():
    """(N, K) of the qkv / o / gate-up / down / LM-head shards of every preset at TP 1, 2, 4, 8."""
    out = set()
    for a in PRESETS.values():
        h, d = a.hidden_size, a.head_dim
        for tp in (1, 2, 4, 8):
            if a.num_heads % tp or a.intermediate_size % tp:
                continue
            hq, hkv, inter = a.num_heads // tp, max(1, a.num_kv_heads // tp), a.intermediate_size // tp
            vocab = a.vocab_size // tp if a.vocab_size % tp == 0 else a.vocab_size
            out |= {((hq + 2 * hkv) * d, h), (h, hq * d), (inter, h), (h, inter), (vocab, h)}
    return out


def grid_shapes(table_shapes):
    synthetic = {(n, k) for n in (256, 384, 512, 1536, 3072, 5120) for k in (256, 512, 768, 1024, 3584)}
    return sorted(set(table_shapes) | preset_shapes() | synthetic)


def _call(fn, *args, **kw):
    """'wr,kc,sk' (or 'wr,kc,wr,kc' of a tile pair), 'none' for a None result, None for a ValueError."""
    try:
        r = fn(*args, **kw)
    except ValueError:
        return None
    if r is None:
        return "none"
    flat = [v for t in r for v in t] if isinstance(r[0], tuple) else r
    return ",".join(str(int(v)) for v in flat)


def grid_rows(decode_tile, decode_tile_silu, moe_tiles, shapes):
    """{"N,K": {"tile": [...], "silu": [...], "moe": [...]}} in the fixed order of the loops below."""
    out = {}
    for n, k in shapes:
        tile = [_call(decode_tile, n, k, mode, b, max_sk=max_sk, row_major=rm)
                for mode in MODES for b in BUCKETS for rm in (False, True)
                for max_sk in ((8, 5, 1) if mode == 2 else (8,))]
        silu = [_call(decode_tile_silu, n, k, b, row_major=rm) for b in BUCKETS for rm in (False, True)]
        moe = [_call(moe_tiles, k, n, t) for t in MOE_TOKENS]  # an expert's gate/up is [2 inter, hidden] = [2N, K]
        out[f"{n},{k}"] = {"tile": tile, "silu": silu, "moe": moe}
    return out


def test_selection_matches_the_five_table_snapshot():
    with open(SNAPSHOT) as f:
        want = json.load(f)
    assert not os.environ.get("DIE_TILE_OVERRIDE"), "the snapshot was recorded with no override"
    shapes = grid_shapes({key[:2] for key in dt.DECODE_TILE_CFG} | {key[:2] for key in dt.DECODE_TILE_CFG_RM})
    assert [f"{n},{k}" for n, k in shapes] == list(want), "the grid's shapes changed"
    got = grid_rows(dt.decode_tile, dt.decode_tile_silu, dt.moe_decode_tiles, shapes)
    rows = bad = 0
    for shape, sections in want.items():
        for name, vals in sections.items():
            assert len(got[shape][name]) == len(vals), (shape, name)
            for i, (g, w) in enumerate(zip(got[shape][name], vals)):
                rows += 1
                if g != w:
                    bad += 1
                    print(f"{shape} {name}[{i}]: {g} != {w}")
    print(f"decode-tile snapshot: {rows} rows compared over {len(want)} shapes")
    assert rows >= 4500 and bad == 0, f"{bad} of {rows} selections differ from the snapshot"


@pytest.fixture(scope="module")
def cxx_geometry(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("gd_tiles") / "gd_tiles_dump")
    src = os.path.join(ROOT, "csrc", "kernels", "tests", "gd_tiles_dump.cpp")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
    rows = [tuple(int(v) for v in line.split())
            for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    return rows  # (wr, kc, xr, valid, ring_slots, half_ring_slots, lds)


def test_python_tile_list_is_the_cxx_list(cxx_geometry):
    tiles = list(dict.fromkeys(r[:2] for r in cxx_geometry))
    assert tiles == list(dt.GD_TILES) and len(tiles) == 13
    assert set(dt.GENERIC_TILES) | set(dt.LM_HEAD_TILES) <= set(dt.GD_TILES)


def test_gd_tile_valid_mirrors_cxx(cxx_geometry):
    assert len(cxx_geometry) == 52
    invalid = set()
    for wr, kc, xr, valid, slots, half_slots, lds in cxx_geometry:
        assert dt.gd_tile_valid(wr, kc, xr) == bool(valid), (wr, kc, xr)
        assert dt.ring_slots(wr, kc, xr) == slots, (wr, kc, xr)
        # the half ring (no Python mirror): no deeper than the full one, two of them within a CU's LDS
        assert half_slots == 0 or (2 <= half_slots <= slots and 2 * half_slots * (wr + xr) * kc * 2 <= dt.LDS_BYTES)
        assert dt.gd_lds(wr, kc, xr) == lds, (wr, kc, xr)
        if not valid:
            invalid.add((wr, kc, xr))
    assert invalid == ({(wr, 256, 128) for wr in (32, 48, 64)} | {(wr, 64, 16) for wr in (64, 128)}
                       | {(wr, 32, xr) for wr in (64, 128) for xr in (16, 32)})
