"""The decode-path kernels are built with kernarg preload (src/_build.py PRELOAD_ON): their kernel descriptors must
report a non-zero preload length, or the argument order of gemm_decode.hip / attention.hip / sampling.hip buys
nothing. Reads metadata only — the gfx950 code object bundled in build/obj/<file>.o and its 64-byte kernel
descriptors (`<kernel>.kd`; KERNARG_PRELOAD is the 16-bit field at byte 58, length in dwords in bits 0..6) — no
instructions. Skipped when the objects are not built."""

import os
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# 16 user SGPRs less the kernarg segment pointer; every named kernel has at least that many leading argument dwords
FULL_PRELOAD = 14


def _sections(elf):
    assert elf[:4] == b"\x7fELF" and elf[4] == 2 and elf[5] == 1, "ELF64 little-endian expected"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    if shnum == 0:  # more than 0xff00 sections: the count is section 0's size
        shnum, = struct.unpack_from("<Q", elf, shoff + 0x20)
    if shstrndx == 0xFFFF:  # ... and the string table's index its link
        shstrndx, = struct.unpack_from("<I", elf, shoff + 0x28)
    secs = []
    for i in range(shnum):
        name, typ, _, addr, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
        secs.append({"name": name, "type": typ, "addr": addr, "off": off, "size": size, "link": link,
                     "entsize": entsize})
    strtab = secs[shstrndx]
    for s in secs:
        end = elf.index(b"\0", strtab["off"] + s["name"])
        s["name"] = elf[strtab["off"] + s["name"]:end].decode()
    return secs


def _device_code_object(obj_path, arch="gfx950"):
    host = open(obj_path, "rb").read()
    fat = next(s for s in _sections(host) if s["name"] == ".hip_fatbin")
    blob = host[fat["off"]:fat["off"] + fat["size"]]
    assert blob[:len(BUNDLE_MAGIC)] == BUNDLE_MAGIC, "uncompressed clang offload bundle expected"
    n, = struct.unpack_from("<Q", blob, len(BUNDLE_MAGIC))
    p = len(BUNDLE_MAGIC) + 8
    for _ in range(n):
        off, size, tlen = struct.unpack_from("<QQQ", blob, p)
        triple = blob[p + 24:p + 24 + tlen].decode()
        p += 24 + tlen
        if triple.startswith("hip") and triple.endswith(arch):
            return blob[off:off + size]
    raise AssertionError(f"no {arch} code object in {obj_path}")


def preload_lengths(obj_path):
    """{kernel symbol: kernarg preload length in dwords} of the object's gfx950 code object."""
    co = _device_code_object(obj_path)
    secs = _sections(co)
    symtab = next(s for s in secs if s["type"] == 2)  # SHT_SYMTAB
    strs = secs[symtab["link"]]
    out = {}
    for i in range(symtab["size"] // symtab["entsize"]):
        name, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", co, symtab["off"] + i * symtab["entsize"])
        end = co.index(b"\0", strs["off"] + name)
        sym = co[strs["off"] + name:end].decode()
        if not sym.endswith(".kd") or size != 64 or shndx == 0 or shndx >= len(secs):
            continue
        sec = secs[shndx]
        kd = co[sec["off"] + value - sec["addr"]:][:64]
        spec, = struct.unpack_from("<H", kd, 58)
        out[sym[:-3]] = spec & 0x7F
    return out


def _lengths(name):
    path = os.path.join(OBJ, name + ".o")
    if not os.path.exists(path):
        pytest.skip(f"{name}.o is not built")
    return preload_lengths(path)


def test_decode_gemm_and_lm_head_kernels_preload_their_arguments():
    lens = _lengths("gemm_decode")
    gd = {k: v for k, v in lens.items() if "gemm_decode_kernel" in k}
    assert gd, "no gemm_decode_kernel instantiation found"
    assert all(v == FULL_PRELOAD for v in gd.values()), sorted(set(gd.values()))
    # the LM head: mode 0 at the nt policy, e.g. the 128-row tile of the 128,256-entry vocabulary
    lm = [k for k in gd if "ILi128ELi0E" in k and "Lb1E" in k]
    assert lm and all(gd[k] > 0 for k in lm)


def test_decode_attention_kernels_preload_their_arguments():
    lens = _lengths("attention")
    v3 = {k: v for k, v in lens.items() if "attn_decode_v3_kernel" in k}
    assert len(v3) == 16, sorted(v3)  # G in {1, 2, 4, 8} x fused / plain x two K/V cache policies
    assert all(v == FULL_PRELOAD for v in v3.values()), v3


def test_sampling_kernel_preloads_its_arguments():
    lens = _lengths("sampling")
    sk = {k: v for k, v in lens.items() if "sample_kernel" in k}
    assert len(sk) == 1 and all(v == FULL_PRELOAD for v in sk.values()), sk
