"""
Not a test: the table of good calls into ``src._C`` that test_binding_args_cpu.py and test_binding_args_gpu.py share,
one row per entry point that takes a tensor (a second row where one call cannot use every tensor: the decode GEMM's
fusion operands depend on the mode), and the mutations of a tensor argument that the binding must refuse.

A row builds its call at the smallest legal shapes on the device it is given, with contents a kernel can run on
(block tables, slots, ids and offsets inside their tables; rows of the logit ops mapped to slot -1, "untouched").
Every tensor the binding checks is an :class:`A`, which says how the binding reads it:

* ``kind``: ``"dense"`` (a contiguous array behind a raw pointer) or ``"rows"`` (a 2-D matrix with a row stride);
* ``short``: the axes along which one element, row or column less than the call needs must be refused
  (``{axis: size}`` where the need is not "all of it": ``cnt`` needs one element and has two, so that it can be
  strided);
* ``grow``: the axes along which the tensor sets a count that the other arguments must cover (``ctx_lens`` sets the
  number of sequences, ``x`` the rows): there one *more* must be refused, the others being one short of it;
* ``align``: the base must be 8- or 16-byte aligned; ``rank``: the rank is checked.

An axis in neither ``short`` nor ``grow`` is one whose length the binding hands to the kernel as the bound (an
arena, a table of any size): a shorter one is another good call.
"""

from __future__ import annotations

import torch

BF16, F32, I32, I64, I16, U8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.int16, torch.uint8

# entry points without a tensor parameter
TENSOR_FREE = {"decode_partials", "gd_occupancy", "attn_set_few_pair_parts", "check_only", "car_alloc", "car_tensor",
               "car_release", "car_handle", "car_open", "car_close", "car_read_words"}

MUTATIONS = ("device", "dtype", "strided", "short", "align", "rank")


class A:
    def __init__(self, t, kind="dense", short=None, grow=(), align=None, rank=None):
        self.t, self.kind = t, kind
        rows = kind == "rows"
        self.short = ((0, 1) if rows else (0,)) if short is None else short
        self.grow = grow
        self.align = rows if align is None else align
        self.rank = (rows or t.dim() > 1) if rank is None else rank


OTHER_DTYPE = {BF16: torch.float16, F32: I32, I32: F32, I64: I32, I16: BF16, U8: torch.int8}


def _resized(t, axis, size, view):
    """t with `size` entries along axis. Shrinking a row matrix keeps its base and row stride (a view: only the size
    changes); a dense array stays dense (a copy); growing makes a fresh tensor."""
    if size <= t.shape[axis]:
        return t.narrow(axis, 0, size) if view else t.narrow(axis, 0, size).contiguous()
    shape = list(t.shape)
    shape[axis] = size
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def mutations(a: A, other_device):
    """(mutation, detail, tensor) for every mutation that applies to the argument"""
    t = a.t
    if other_device == "meta":
        yield "device", "", torch.empty_like(t, device="meta")
    else:
        yield "device", "", t.to(other_device)
    yield "dtype", "", t.to(OTHER_DTYPE[t.dtype])
    wide = torch.zeros(list(t.shape[:-1]) + [2 * t.shape[-1]], dtype=t.dtype, device=t.device)
    yield "strided", "", wide[..., ::2]        # a [::2] view of a doubled buffer / a column-strided matrix
    short = a.short if isinstance(a.short, dict) else {ax: t.shape[ax] - 1 for ax in a.short}
    for ax, size in short.items():
        yield "short", f"axis {ax}", _resized(t, ax, size, a.kind == "rows")
    for ax in a.grow:
        yield "short", f"others short of axis {ax} + 1", _resized(t, ax, t.shape[ax] + 1, False)
    if a.align:
        need = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
        buf = torch.zeros(need + 8, dtype=t.dtype, device=t.device)
        yield "align", "", buf.as_strided(t.shape, t.stride(), 1)
    if a.rank:
        yield "rank", "", t.flatten(0, 1) if t.dim() > 1 else t[0]


class Row:
    def __init__(self, name, build, gpu=True, cleanup=None):
        self.name, self.op, self.build, self.gpu, self.cleanup = name, name.split("/")[0], build, gpu, cleanup


ROWS: list = []

# (row, argument, mutation) -> why it does not apply. At most one (row, mutation) pair in ten, none for "device"
# or "short".
LEAVE_OUT = {
    ("car_copy_to", "src", "dtype"): "the copy moves bytes: src may have any dtype",
}


def row(name, gpu=True, cleanup=None):
    def deco(f):
        ROWS.append(Row(name, f, gpu, cleanup))
        return f
    return deco


def call_args(args: dict, replace=None):
    """the positional arguments of the call; replace = (name, tensor) swaps one in"""
    out = []
    for k, v in args.items():
        if replace is not None and k == replace[0]:
            v = replace[1]
        out.append(v.t if isinstance(v, A) else v)
    return out


def z(dev, shape, dtype):
    return torch.zeros(shape, dtype=dtype, device=dev)


def vec(dev, vals, dtype):
    return torch.tensor(vals, dtype=dtype, device=dev)


def rows_(dev, r, c, dtype=BF16, **kw):
    return A(z(dev, (r, c), dtype), "rows", **kw)


def empty(dev):
    return torch.empty(0, device=dev)


# ---- norms and activations: 2 x 64 rows
@row("rms_norm")
def _(d):
    return dict(out=rows_(d, 2, 64), x=rows_(d, 2, 64), w=A(z(d, 64, BF16)), eps=1e-5)


@row("fused_add_rms_norm")
def _(d):
    return dict(out=rows_(d, 2, 64), x=rows_(d, 2, 64), residual=A(z(d, (2, 64), BF16), short=(0, 1)),
                w=A(z(d, 64, BF16)), eps=1e-5)


@row("fused_add_rms_norm_slab")
def _(d):
    return dict(out=rows_(d, 2, 64), slab=A(z(d, (1, 2, 64), F32), short=(1, 2)),
                residual=A(z(d, (2, 64), BF16), short=(0, 1)), w=A(z(d, 64, BF16)), eps=1e-5)


@row("silu_and_mul")
def _(d):
    return dict(out=A(z(d, (2, 8), BF16), short=(0, 1)), x=A(z(d, (2, 16), BF16), short=(0, 1)),
                row_scale=A(z(d, 2, F32)))


@row("silu_and_mul_views")
def _(d):
    return dict(out=rows_(d, 2, 8), gate=rows_(d, 2, 8), up=rows_(d, 2, 8), row_scale=A(z(d, 2, F32)), per=0)


@row("rms_row_scale")
def _(d):
    return dict(rs=A(z(d, 2, F32)), resid=rows_(d, 2, 64), x=rows_(d, 2, 64), eps=1e-5)


@row("residual_add_sumsq")
def _(d):
    return dict(ssp=A(z(d, 2, F32)), resid=rows_(d, 2, 64), x=rows_(d, 2, 64))


@row("row_sumsq")
def _(d):
    return dict(ssp=A(z(d, 2, F32)), x=rows_(d, 2, 64, short=(), grow=(0,)))


@row("embed_sumsq")
def _(d):
    return dict(out=A(z(d, (2, 8), BF16), short=(0, 1)), ssp=A(z(d, 128, F32)),
                table=A(z(d, (8, 8), BF16), short=(1,)), ids=A(z(d, 2, I64)))


# ---- RoPE and paged attention: head_dim 128, one KV head, block size 16; sequences of 17 tokens and 1 token
def caches(d, blocks=3, **kw):
    kw.setdefault("short", (1, 3))
    return A(z(d, (blocks, 1, 16, 128), BF16), **kw), A(z(d, (blocks, 1, 16, 128), BF16), **kw)


@row("rope_and_cache")
def _(d):
    k, v = caches(d, short=(0, 1, 2, 3))     # the two caches must also have one shape
    return dict(qkv=rows_(d, 2, 384, short=(1,), grow=(0,)), positions=A(z(d, 2, I64)),
                cos_sin=A(z(d, (4, 128), F32), short=(1,)), slot_mapping=A(vec(d, [0, 1], I64)), k_cache=k,
                v_cache=v, hq=1, hkv=1, head_dim=128, rot_q=True, row_scale=A(z(d, 2, F32)))


@row("rope_and_cache_slab")
def _(d):
    k, v = caches(d)
    return dict(q_out=A(z(d, (2, 128), BF16), rank=False), slab=A(z(d, (1, 2, 384), F32), short=(2,), grow=(1,)),
                positions=A(z(d, 2, I64)), cos_sin=A(z(d, (4, 128), F32), short=(1,)),
                slot_mapping=A(vec(d, [0, 1], I64)), k_cache=k, v_cache=v, hq=1, hkv=1, head_dim=128)


@row("attn_prefill")
def _(d):
    k, v = caches(d)
    return dict(out=A(z(d, (18, 128), BF16), rank=False), q=rows_(d, 18, 128, short=(1,), grow=(0,)), k_cache=k,
                v_cache=v, block_tables=A(vec(d, [[0, 1], [2, 2]], I32)), cu_q=A(vec(d, [0, 17, 18], I32)),
                ctx_lens=A(vec(d, [17, 1], I32), short=(), grow=(0,)), max_q_len=17, hq=1, hkv=1, scale=0.1,
                cos_sin=A(z(d, (32, 128), F32), short=(1,)), q_scale=A(z(d, 18, F32)))


def decode_parts(d):
    from src import _C
    maxp = _C.decode_partials(32)
    return dict(part_o=A(z(d, 2 * maxp * 128, F32)), part_ml=A(z(d, 2 * maxp * 2, F32)), counters=A(z(d, 2, I32)))


def paged(d):
    k, v = caches(d)
    return dict(k_cache=k, v_cache=v, block_tables=A(vec(d, [[0, 1], [2, 2]], I32), short=(0, 1)),
                ctx_lens=A(vec(d, [17, 1], I32), short=(), grow=(0,)), max_ctx=32, hq=1, hkv=1, scale=0.1)


@row("attn_decode")
def _(d):
    return dict(out=A(z(d, (2, 128), BF16), rank=False), **decode_parts(d), q=rows_(d, 2, 128), **paged(d),
                kv_once=True)


@row("attn_decode_fused")
def _(d):
    return dict(out=A(z(d, (2, 128), BF16), rank=False), **decode_parts(d),
                slab=A(z(d, (1, 2, 384), F32), short=(1, 2)), ssp=A(z(d, (1, 128), F32), short=(0, 1)),
                positions=A(vec(d, [16, 0], I64)), cos_sin=A(z(d, (32, 128), F32), short=(1,)),
                slot_mapping=A(vec(d, [16, 32], I64)), **paged(d), eps=1e-5, hidden=128, kv_once=True)


# ---- sampling and the logit ops: 2 rows, vocab 8, 2 slots; every row mapped to slot -1 (untouched)
def logits(d, **kw):
    kw.setdefault("short", ())         # vocab % 8 is the launcher's check
    return rows_(d, 2, 8, grow=(0,), **kw)


def lm_part(d):
    return A(z(d, (2, 1, 2), I32), short=(0, 2))


@row("sample")
def _(d):
    return dict(out=A(z(d, 2, I64)), logits=logits(d, short=(1,)), temperature=A(z(d, 2, F32)), top_k=A(z(d, 2, I32)),
                top_p=A(torch.ones(2, dtype=F32, device=d)), seeds=A(z(d, 2, I64)), steps=A(z(d, 2, I64)),
                part=A(z(d, 64, I32)), cnt=A(z(d, 2, I32)), lm_part=lm_part(d))


def advance(d):
    return dict(ids=A(z(d, 2, I64)), pos=A(z(d, 2, I64)), ctx=A(vec(d, [1, 1], I32)), slots=A(z(d, 2, I64)),
                bt=A(z(d, (2, 2), I32), short=(0,)), step=A(z(d, 2, I64)), tokens=A(z(d, (2, 2), I64), short=(1,)),
                cnt=A(z(d, 2, I32), short={0: 0}), n_real=A(vec(d, [2, 0], I32), short={0: 0}))


@row("sample_advance")
def _(d):
    adv = advance(d)
    return dict(out=A(z(d, 2, I64)), logits=logits(d, short=(1,)), temperature=A(z(d, 2, F32)), top_k=A(z(d, 2, I32)),
                top_p=A(torch.ones(2, dtype=F32, device=d)), seeds=A(z(d, 2, I64)), lm_part=lm_part(d),
                **{k: adv[k] for k in ("ids", "pos", "ctx", "slots", "bt", "step", "tokens", "cnt", "n_real")},
                block_size=16, ticket=A(z(d, 2, I32), short={0: 0}), table=A(z(d, (8, 8), BF16), short=(1,)),
                h_out=A(z(d, (2, 8), BF16), short=(0, 1)), ssp_out=A(z(d, 2, F32)))


@row("decode_advance")
def _(d):
    return dict(out=A(z(d, 2, I64)), **advance(d), rows=2, block_size=16)


@row("token_logprobs")
def _(d):
    return dict(lp=A(z(d, 2, F32)), rank=A(z(d, 2, I32)), top_lp=rows_(d, 2, 2, F32, align=False),
                top_id=rows_(d, 2, 2, I32, align=False), logits=logits(d), targets=A(z(d, 2, I64)), top_n=2)


def untouched(d):
    return A(vec(d, [-1, -1], I32))


@row("logit_process")
def _(d):
    return dict(logits=logits(d, short=(1,)), slot=untouched(d), state=A(z(d, (2, 8), I16), short=(1,), grow=(0,)),
                params=A(z(d, (2, 4), F32), align=True, rank=False), bias_cnt=A(z(d, 2, I32)),
                bias_ids=A(z(d, (2, 2), I32), short=(0, 1)), bias_vals=A(z(d, (2, 2), F32), short=(0, 1)),
                count_ids=A(z(d, 2, I64)), lm_part=lm_part(d))


def guide(d):
    return dict(logits=logits(d), slot=untouched(d), desc=A(z(d, (2, 4), I32), short=(1,), grow=(0,), align=True))


def guide_tail(d):
    return dict(err=A(z(d, 2, I32)), advance_ids=A(z(d, 2, I64)), lm_part=lm_part(d))


def tok_table(d):     # 8 tokens of one byte each
    return dict(tok_off=A(torch.arange(9, dtype=I32, device=d), short=(), rank=True),
                tok_bytes=A(z(d, 8, U8), short=(), rank=True))


@row("token_guide")
def _(d):
    return dict(**guide(d), rowptr=A(z(d, 4, I32), short=(), rank=True),
                edges=A(z(d, (2, 2), I32), short=(1,), align=True), cur=A(z(d, 2, I32)), **guide_tail(d))


@row("byte_guide")
def _(d):
    return dict(**guide(d), trans=A(z(d, (2, 256), I16), short=(1,)), accept=A(z(d, 2, U8), short=(), rank=True),
                **tok_table(d), cur=A(z(d, 2, I32)), **guide_tail(d))


@row("json_guide")
def _(d):
    return dict(**guide(d), trans=A(z(d, (3, 256), I16), short=(1,)), **tok_table(d), cur=A(z(d, 2, I32)),
                jstk=A(z(d, (2, 2), I32), short=(0, 1)), **guide_tail(d))


@row("schema_guide")
def _(d):
    return dict(**guide(d), trans=A(z(d, (2, 256), I32), short=(1,)), accept=A(z(d, 2, U8), short=(), rank=True),
                **tok_table(d), cur=A(z(d, 2, I32)), sdep=A(z(d, 2, I32)), sstk=A(z(d, (2, 32), I16), short=(0, 1)),
                **guide_tail(d))


@row("pool_embed")
def _(d):      # one mean segment over all 4 rows, first and final chunk at once
    return dict(out=A(z(d, (1, 8), F32), short=(0, 1)), acc=A(z(d, (2, 8), F32), short=(1,)),
                hidden=rows_(d, 4, 8, short=(1,), align=False),
                segs=A(vec(d, [[0, 4, 0, 4, 7, 0, 1, 0]], I32), short=(1,), grow=(0,)), dims=0, normalize=True,
                part=A(z(d, (2, 8), F32), short=(1,)), tickets=A(z(d, 2, I32), short=(), rank=True), max_parts=1)


# ---- the KV block movers: a pool of 2 planes x 3 blocks x 16 elements
def pool(d):
    return A(z(d, (2, 3, 16), BF16), short=(), rank=True)


@row("copy_blocks")
def _(d):
    return dict(pool=pool(d), pairs=A(vec(d, [[0, 1], [0, 2]], I64), short=(1,)))


@row("move_blocks")
def _(d):
    return dict(pool=pool(d), buf=A(z(d, 2 * 2 * 16, BF16)), ids=A(vec(d, [0, 2], I64), short=(), grow=(0,)),
                gather=True)


@row("gather_blocks_rows")
def _(d):
    packets = z(d, (2, 32), BF16)      # dst: the address of each packet row; kept alive by the call's arguments
    dst = vec(d, [packets.data_ptr(), packets.data_ptr() + 64], I64)
    return dict(pool=pool(d), ids=A(vec(d, [0, 2], I64)), dst=A(dst), plane0=0, nplanes=2, _keep=packets)


# ---- MoE: 2 tokens, top-2 of 8 experts, hidden 8
@row("topk_softmax")
def _(d):
    return dict(w=A(z(d, (2, 2), F32), short=(0, 1)), ids=A(z(d, (2, 2), I32), short=(0, 1)),
                gating=A(z(d, (2, 8), BF16)), renorm=True)


@row("moe_route")
def _(d):
    return dict(w=A(z(d, (2, 2), F32), short=(0, 1)), ids=A(z(d, (2, 2), I32), short=(0, 1)), x=rows_(d, 2, 8),
                wg=A(z(d, (8, 8), BF16), short=(1,)), renorm=True)


@row("moe_align")
def _(d):
    return dict(offsets=A(z(d, 3, I32)), sorted=A(z(d, 4, I32)), pos=A(z(d, 4, I32)),
                ids=A(vec(d, [0, 1, 1, 0], I32), short=(), grow=(0,)), num_experts=2)


@row("moe_gather")
def _(d):
    return dict(xs=A(z(d, (4, 8), BF16), short=(0, 1)), x=A(z(d, (2, 8), BF16), short=(0, 1)),
                sorted=A(vec(d, [0, 1, 2, 3], I32)), topk=2)


def combine(d):
    return dict(ys=A(z(d, (4, 8), BF16), short=(0, 1)), pos=A(vec(d, [0, 1, 2, 3], I32)),
                w=A(z(d, (2, 2), F32), short=(0, 1)))


@row("moe_combine")
def _(d):
    return dict(out=A(z(d, (2, 8), BF16), short=(0, 1)), **combine(d))


@row("moe_combine_residual")
def _(d):
    return dict(ssp=A(z(d, 2, F32)), resid=rows_(d, 2, 8), **combine(d))


# ---- the decode GEMM: M = 1, tile (wr, kc) = (64, 128); one K-chunk, two where split-K brings in the tickets
def gemm(d, mode, n_out, w_rows, k=128, sk=1, slab=False, **fuse):
    y = A(z(d, (sk, 1, n_out), F32), short=(0, 1, 2)) if slab else rows_(d, 1, n_out)
    e = empty(d)
    return dict(y=y, x=rows_(d, 1, k), w=A(z(d, (w_rows, k), BF16), short=(0, 1)), mode=mode, wr=64, kc=128, sk=sk,
                nt=True, resid=fuse.get("resid", e), ssp_out=fuse.get("ssp_out", e), counters=fuse.get("counters", e),
                ssp_in=fuse.get("ssp_in", e), eps=1e-5)


@row("gemm_decode/plain")
def _(d):
    return gemm(d, 0, 64, 64)


@row("gemm_decode/residual")       # mode 3, split-K: resid, the statistics tiles and the tickets
def _(d):
    return gemm(d, 3, 128, 128, k=256, sk=2, slab=True, resid=rows_(d, 1, 128), ssp_out=A(z(d, 256, F32)),
                counters=A(z(d, 2, I32)))


@row("gemm_decode/silu_norm")      # mode 6, split-K: the partial slab rides in ssp_out
def _(d):
    return gemm(d, 6, 64, 128, k=256, sk=2, ssp_out=A(z(d, 2 * 1 * 128, F32)), counters=A(z(d, 2, I32)),
                ssp_in=A(z(d, (1, 128), F32), short=(0, 1)))


@row("gemm_decode_argmax")
def _(d):
    return dict(y=rows_(d, 1, 64), x=rows_(d, 1, 128), w=A(z(d, (64, 128), BF16), short=(0, 1)), wr=64, kc=128,
                layout=0, amax=A(z(d, (1, 1, 2), I32), short=(0, 1, 2)))


@row("gemm_decode_grouped")
def _(d):      # one expert, two tokens gathered through rows
    return dict(y=rows_(d, 2, 64), x=rows_(d, 2, 128), w=A(z(d, (1, 64, 128), BF16), short=(1, 2)),
                offsets=A(vec(d, [0, 2], I32)), mode=0, wr=64, kc=128, rows=A(vec(d, [0, 1], I32)), k=1,
                max_rows=16, segs=1)


# ---- the one-shot collectives: the peers are raw addresses, arbitrary here: these rows never launch
PEERS = dict(rank=0, bufs=[4096, 8192], sigs=[12288, 16384], ctl=20480, cap_elems=1 << 20)


@row("gemm_decode_car", gpu=False)
def _(d):
    g = gemm(d, 3, 64, 64, slab=True, resid=rows_(d, 1, 64), ssp_out=A(z(d, 128, F32)))
    del g["ssp_in"], g["eps"]
    return dict(**g, **PEERS)


def dense2(d, r, c):
    return A(z(d, (r, c), BF16), short=(0, 1), align=True)


@row("car_all_reduce", gpu=False)
def _(d):
    return dict(inp=A(z(d, 8, BF16), align=True), out=A(z(d, 8, BF16), align=True), **PEERS, blocks=1)


@row("car_all_gather", gpu=False)
def _(d):
    return dict(inp=dense2(d, 2, 8), out=dense2(d, 2, 16), **PEERS, blocks=1)


@row("car_all_reduce_residual", gpu=False)
def _(d):
    return dict(x=dense2(d, 2, 8), resid=dense2(d, 2, 8), ssp=A(z(d, 2, F32)), **PEERS)


@row("car_copy_to")
def _(d):      # 16 bytes into a buffer of our own
    dst = z(d, 8, BF16)
    return dict(dst_ptr=dst.data_ptr(), src=A(z(d, 8, BF16)), _keep=dst)


# ---- the diagnostics setters keep the pointer: a real run would have every later GEMM / attention launch write
# its stamps there, so these rows never run for real, and both tests switch the stamps off again
def stamps_off():
    from src import _C
    _C.gd_set_timestamps(torch.empty(0, dtype=I64))
    _C.attn_set_timestamps(torch.empty(0, dtype=I64))


@row("gd_set_timestamps", gpu=False, cleanup=stamps_off)
def _(d):
    return dict(t=A(z(d, 6, I64), short=()))


@row("attn_set_timestamps", gpu=False, cleanup=stamps_off)
def _(d):
    return dict(t=A(z(d, 6, I64), short=()))


def tensors(args: dict):
    """every tensor of a call, by argument name"""
    return {k: (v.t if isinstance(v, A) else v) for k, v in args.items()
            if isinstance(v, (A, torch.Tensor))}


def invoke(_C, r: Row, args: dict, replace=None):
    a = call_args({k: v for k, v in args.items() if not k.startswith("_")}, replace)
    return getattr(_C, r.op)(*a)
