"""
Plain-PyTorch fp32 reference implementations of every custom op.

They define the semantics the gfx950 kernels must match (the numerics tests
compare kernel vs. these) and run the engine on CPU tensors for control-flow
tests. They are never used for GPU tensors: :mod:`src.ops` routes GPU tensors
to the HIP extension and raises if it is missing.
"""

from __future__ import annotations

import math
from typing import Optional

import torch


def _wide(x: torch.Tensor) -> torch.Tensor:
    """The working precision of the model ops: fp32, or float64 for a float64 tensor (a float64 copy of the
    model is not cut to fp32 at every op)."""
    return x if x.dtype == torch.float64 else x.float()


def rms_norm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = _wide(x)
    var = xf.pow(2).mean(-1, keepdim=True)
    return (xf * torch.rsqrt(var + eps) * _wide(w)).to(x.dtype)


def fused_add_rms_norm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float):
    r = (_wide(x) + _wide(residual)).to(residual.dtype)
    return rms_norm(r, w, eps), r


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    i = x.shape[-1] // 2
    g, u = _wide(x[..., :i]), _wide(x[..., i:])
    return (torch.nn.functional.silu(g) * u).to(x.dtype)


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, device=None, scaling: Optional[dict] = None) -> torch.Tensor:
    """[max_pos, head_dim] fp32 table: cos in the first half, sin in the second."""
    half = head_dim // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    if scaling and scaling.get("rope_type") == "llama3":
        factor = scaling["factor"]
        lo, hi = scaling.get("low_freq_factor", 1.0), scaling.get("high_freq_factor", 4.0)
        old = scaling.get("original_max_position_embeddings", 8192)
        wavelen = 2 * math.pi / inv
        lo_w, hi_w = old / lo, old / hi
        smooth = (old / wavelen - lo) / (hi - lo)
        scaled = torch.where(wavelen > lo_w, inv / factor, inv)
        mid = (wavelen <= lo_w) & (wavelen >= hi_w)
        inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def apply_rope(x: torch.Tensor, positions: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, H, D] neox-style rotation."""
    d = x.shape[-1]
    half = d // 2
    cs = cos_sin[positions.long()]
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    xf = _wide(x)
    a, b = xf[..., :half], xf[..., half:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1).to(x.dtype)


def rope_and_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, hq, hkv, head_dim):
    t = qkv.shape[0]
    q = qkv[:, : hq * head_dim].view(t, hq, head_dim)
    k = qkv[:, hq * head_dim:(hq + hkv) * head_dim].view(t, hkv, head_dim)
    v = qkv[:, (hq + hkv) * head_dim:(hq + 2 * hkv) * head_dim].view(t, hkv, head_dim)
    qr = apply_rope(q, positions, cos_sin)
    kr = apply_rope(k, positions, cos_sin)
    qkv[:, : hq * head_dim] = qr.reshape(t, -1)
    bs = k_cache.shape[2]
    for i in range(t):
        s = int(slot_mapping[i])
        if s < 0:
            continue
        k_cache[s // bs, :, s % bs] = kr[i]
        v_cache[s // bs, :, s % bs] = v[i]


def gather_kv(cache: torch.Tensor, block_table: torch.Tensor, n: int) -> torch.Tensor:
    """[n, hkv, D] rows 0..n-1 of one sequence from the paged cache."""
    bs = cache.shape[2]
    pos = torch.arange(n, device=cache.device)
    blocks = block_table[(pos // bs).long()].long()
    return cache[blocks, :, pos % bs]


def attention(q, k_cache, v_cache, block_tables, cu_q, ctx_lens, hq, hkv, scale):
    """Causal paged attention; q [T, >=hq*D] (rows may be strided) → [T, hq, D]."""
    d = 128
    out = torch.empty(q.shape[0], hq, d, dtype=q.dtype, device=q.device)
    g = hq // hkv
    for s in range(ctx_lens.numel()):
        a, b = int(cu_q[s]), int(cu_q[s + 1])
        qlen, ctx = b - a, int(ctx_lens[s])
        if qlen == 0:
            continue
        qs = _wide(q[a:b, : hq * d].reshape(qlen, hq, d))
        k = _wide(gather_kv(k_cache, block_tables[s], ctx)).repeat_interleave(g, dim=1)
        v = _wide(gather_kv(v_cache, block_tables[s], ctx)).repeat_interleave(g, dim=1)
        sc = torch.einsum("qhd,khd->hqk", qs, k) * scale
        qpos = torch.arange(ctx - qlen, ctx, device=q.device)[:, None]
        kpos = torch.arange(ctx, device=q.device)[None, :]
        sc = sc.masked_fill((kpos > qpos)[None], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[a:b] = torch.einsum("hqk,khd->qhd", p, v).to(q.dtype)
    return out


def sample(logits, temperature=None, top_k=None, top_p=None, seeds=None, steps=None):
    """Greedy where temperature==0; otherwise a (non-bit-exact) torch sampler
    with the same filtering semantics (top-k, then top-p on the renormalised set)."""
    out = torch.empty(logits.shape[0], dtype=torch.long, device=logits.device)
    for r in range(logits.shape[0]):
        row = logits[r].float()
        t = float(temperature[r]) if temperature is not None else 0.0
        k = int(top_k[r]) if top_k is not None else 0
        if t <= 0 or k == 1:
            out[r] = int(torch.argmax(row))
            continue
        z = row / t
        keep = torch.ones_like(z, dtype=torch.bool)
        if 0 < k < z.numel():
            kth = torch.topk(z, k).values[-1]
            keep &= z >= kth
        p = float(top_p[r]) if top_p is not None else 1.0
        if p < 1.0:
            zz = z.masked_fill(~keep, float("-inf"))
            probs = torch.softmax(zz, -1)
            sp, si = torch.sort(probs, descending=True)
            cum = torch.cumsum(sp, 0)
            cut = int(torch.searchsorted(cum, torch.tensor(p, device=cum.device))) + 1
            thr = sp[min(cut, sp.numel()) - 1]
            keep &= probs >= thr
        probs = torch.softmax(z.masked_fill(~keep, float("-inf")), -1)
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seeds[r]) * 1000003 + int(steps[r]) if seeds is not None and steps is not None else 0)
        out[r] = int(torch.multinomial(probs.cpu(), 1, generator=gen))
    return out


def token_logprobs(logits: torch.Tensor, targets: torch.Tensor, top_n: int):
    """Log-probabilities of the raw distribution: float64 ``log_softmax``; tokens ordered by larger logit, then
    lower id (a stable descending sort). Returns (lp fp32 [R], rank int32 [R], top_lp fp32 [R, top_n], top_id
    int32 [R, top_n]); a target outside [0, vocab) gives -inf and rank vocab."""
    if not 0 <= top_n <= 20:
        raise ValueError("top_n must be in [0, 20]")
    rows, vocab = logits.shape
    if top_n > vocab:
        raise ValueError("top_n exceeds the vocabulary")
    z = logits.double()
    lsm = torch.log_softmax(z, dim=-1)
    _, order = torch.sort(z, dim=-1, descending=True, stable=True)
    targets = targets.to(device=logits.device, dtype=torch.long)[:rows]
    ok = (targets >= 0) & (targets < vocab)
    t = torch.where(ok, targets, torch.zeros_like(targets))
    place = torch.empty_like(order)
    place.scatter_(1, order, torch.arange(vocab, device=logits.device).expand(rows, vocab))
    rank = torch.where(ok, place.gather(1, t[:, None])[:, 0], torch.full_like(t, vocab)).int()
    lp = torch.where(ok, lsm.gather(1, t[:, None])[:, 0], torch.full((rows,), float("-inf"), dtype=torch.float64,
                                                                     device=logits.device)).float()
    top_id = order[:, :top_n]
    return lp, rank, lsm.gather(1, top_id).float(), top_id.int()


LOGIT_COUNT_MAX = 32767  # the output count's 15 bits (bit 15 of a state entry: "in the prompt")


def logit_process(logits: torch.Tensor, in_prompt: torch.Tensor, counts: torch.Tensor, rp: float, inv_rp: float,
                  freq: float, pres: float, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Penalties and logit_bias on bf16 logits [..., V] (the contract of csrc/kernels/logit_process.hip): per
    entry, one individually rounded fp32 operation per step —
    x = float(z) + bias; if in the prompt or count > 0: x = x * inv_rp if x > 0 else x * rp;
    x = x - freq * float(count); if count > 0: x = x - pres; one rounding to bf16.
    in_prompt bool [..., V], counts integer [..., V], bias fp32 [..., V] or None; inv_rp = fp32(1 / rp)."""
    f32 = torch.float32
    x = logits.to(f32)
    b = torch.zeros_like(x) if bias is None else bias.to(f32)
    x = x + b
    c = counts.to(torch.int64).clamp(max=LOGIT_COUNT_MAX)
    seen = in_prompt.to(torch.bool) | (c > 0)
    t_rp, t_inv = torch.tensor(rp, dtype=f32), torch.tensor(inv_rp, dtype=f32)
    x = torch.where(seen, torch.where(x > 0, x * t_inv, x * t_rp), x)
    x = x - torch.tensor(freq, dtype=f32) * c.to(f32)
    x = torch.where(c > 0, x - torch.tensor(pres, dtype=f32), x)
    return x.to(torch.bfloat16)


def logit_process_rows(logits, slot, state, params, bias_cnt, bias_ids, bias_vals, count_ids=None, lm_part=None):
    """ops.logit_process on host tensors: the kernel's arguments (state int16 [slots, V] with bit 15 = in the
    prompt and bits 0-14 = output count, params [slots, 4] = rp, 1/rp, freq, pres, the per-slot bias lists),
    rows rewritten in place, count_ids counted first (saturating), lm_part candidates overwritten."""
    vocab = logits.shape[1]
    for r in range(logits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= state.shape[0]:
            continue
        st = state[s].to(torch.int32) & 0xffff
        if count_ids is not None:
            t = int(count_ids[r])
            if 0 <= t < vocab:
                c = int(st[t]) & 0x7fff
                v = (int(st[t]) & 0x8000) | min(c + 1, LOGIT_COUNT_MAX)
                st[t] = v
                state[s, t] = v - 65536 if v >= 32768 else v
        bias = None
        nb = min(int(bias_cnt[s]), bias_ids.shape[1])
        if nb > 0:
            bias = torch.zeros(vocab, dtype=torch.float32)
            ids = bias_ids[s, :nb].long()
            ok = (ids >= 0) & (ids < vocab)
            bias[ids[ok]] = bias_vals[s, :nb][ok].float()
        rp, inv_rp, freq, pres = (float(v) for v in params[s])
        # z is a bf16 logit by contract (an fp32 host model's row is rounded to it first)
        logits[r] = logit_process(logits[r].to(torch.bfloat16), (st & 0x8000) != 0, st & 0x7fff, rp, inv_rp, freq, pres, bias)
        if lm_part is not None:
            v, i = torch.max(logits[r].float(), 0)  # first maximal index
            lm_part[r, :, 0] = torch.tensor(float("-inf")).view(torch.int32)
            lm_part[r, :, 1] = 0x7fffffff
            lm_part[r, 0, 0] = v.view(torch.int32)
            lm_part[r, 0, 1] = int(i)
    return logits


GUIDE_ERR_NO_EDGE = 1  # err bits of token_guide: the advance token has no edge in the current state
GUIDE_ERR_TABLE = 2    # a descriptor, state, row pointer or edge outside its bounds: the row is left untouched


def _guide_mask_row(logits, r, vocab, allowed, lm_part):
    """The tail of every *_guide_rows: row r's entries outside allowed (bool [vocab]) become -inf, the others keep
    their bits; lm_part candidates are overwritten with the best allowed entry (largest value, then lowest index)."""
    logits[r, :vocab] = torch.where(allowed, logits[r, :vocab], torch.tensor(float("-inf"), dtype=logits.dtype))
    if lm_part is None:
        return
    x = logits[r, :vocab].float()
    ok = allowed & ~torch.isnan(x)  # a NaN never wins a comparison (sampling.hip's better())
    x = torch.where(ok, x, torch.tensor(float("-inf")))
    v = x.max()
    first = ((x == v) & ok).nonzero()  # lowest allowed index holding the maximum
    lm_part[r, :, 0] = torch.tensor(float("-inf")).view(torch.int32)
    lm_part[r, :, 1] = 0x7fffffff
    if first.numel():
        lm_part[r, 0, 0] = x[int(first[0])].view(torch.int32)  # that entry's own bits (-0.0 equals +0.0)
        lm_part[r, 0, 1] = int(first[0])


def token_guide_rows(logits, slot, desc, rowptr, edges, cur, err, advance_ids=None, lm_part=None):
    """ops.token_guide on host tensors (the contract of csrc/kernels/token_guide.hip): row r -> slot[r] -> desc
    (state_base, n_states, edge_base, n_edges) into rowptr / edges [E, 2]; the state advances over advance_ids[r]
    first (no edge: err |= 1, state kept); entries outside the state's edge tokens become -inf, the others keep
    their bits; lm_part candidates overwritten with the best allowed entry (largest value, then lowest index).
    Anything out of bounds: err |= 2 and row, candidates and state stay untouched."""
    vocab = logits.shape[1]
    n_rp, n_ed = rowptr.shape[0], edges.shape[0]
    for r in range(logits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        sb, ns, eb, ne = (int(v) for v in desc[s])
        c = int(cur[s])
        if sb < 0 or ns < 1 or sb + ns + 1 > n_rp or eb < 0 or ne < 0 or eb + ne > n_ed or not 0 <= c < ns:
            err[s] |= GUIDE_ERR_TABLE
            continue
        flags = 0
        bad = False
        if advance_ids is not None:
            lo, hi = int(rowptr[sb + c]), int(rowptr[sb + c + 1])
            if lo < 0 or hi < lo or hi > ne:
                err[s] |= GUIDE_ERR_TABLE
                continue
            hit = (edges[eb + lo: eb + hi, 0].long() == int(advance_ids[r])).nonzero()
            if hit.numel():
                nx = int(edges[eb + lo + int(hit[0]), 1])
                if not 0 <= nx < ns:
                    bad = True
                c = nx
            else:
                flags = GUIDE_ERR_NO_EDGE
        if not bad:
            lo, hi = int(rowptr[sb + c]), int(rowptr[sb + c + 1])
            bad = lo < 0 or hi < lo or hi > ne
        if not bad:
            toks = edges[eb + lo: eb + hi, 0].long()
            bad = bool(((toks < 0) | (toks >= vocab)).any())
        if bad:
            err[s] |= GUIDE_ERR_TABLE
            continue
        cur[s] = c
        err[s] |= flags
        allowed = torch.zeros(vocab, dtype=torch.bool)
        allowed[toks] = True
        _guide_mask_row(logits, r, vocab, allowed, lm_part)
    return logits


GUIDE_MAX_TOKEN_BYTES = 32  # byte_guide never allows a longer token


def byte_guide_rows(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, err, advance_ids=None, lm_part=None):
    """ops.byte_guide on host tensors (the contract of csrc/kernels/byte_guide.hip): row r -> slot[r] -> desc
    (state_base, n_states, eos, 0) into trans int16 [A, 256] / accept uint8 [A]; state n_states is the sink. The
    state advances over advance_ids[r] first (EOS from an accepting state or the sink: the sink; a token whose
    bytes die, without bytes, over the length cap, beyond the table, or any token but EOS in the sink: err |= 1,
    state kept). Allowed next: in the sink EOS alone; else EOS iff the state accepts, and every token of 1..32
    bytes whose walk never dies. Barred entries become -inf, the others keep their bits; lm_part candidates are
    overwritten with the best allowed entry. Anything out of bounds: err |= 2 and row, candidates and state stay
    untouched."""
    import numpy as np

    vocab = logits.shape[1]
    tr_all, ac_all = trans.numpy(), accept.numpy()
    off, by = tok_off.numpy().astype(np.int64), tok_bytes.numpy()
    arena, n_tok, blen = min(tr_all.shape[0], ac_all.shape[0]), len(off) - 1, len(by)
    lim = min(vocab, n_tok)
    for r in range(logits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        sb, ns, eos = (int(v) for v in desc[s, :3])
        c = int(cur[s])
        if sb < 0 or ns < 1 or sb + ns > arena or not 0 <= c <= ns or not 0 <= eos < vocab:
            err[s] |= GUIDE_ERR_TABLE
            continue
        tr, ac = tr_all[sb:sb + ns], ac_all[sb:sb + ns]
        flags, bad = 0, False
        if advance_ids is not None:
            tok = int(advance_ids[r])
            if tok == eos:
                if c == ns or ac[c]:
                    c = ns
                else:
                    flags = GUIDE_ERR_NO_EDGE
            elif c == ns or not 0 <= tok < lim:
                flags = GUIDE_ERR_NO_EDGE
            else:
                lo, hi = int(off[tok]), int(off[tok + 1])
                if not 0 <= lo <= hi <= blen:
                    bad = True
                elif hi == lo or hi - lo > GUIDE_MAX_TOKEN_BYTES:
                    flags = GUIDE_ERR_NO_EDGE
                else:
                    st = c
                    for p in range(lo, hi):
                        st = int(tr[st, by[p]])
                        if st < -1 or st >= ns:
                            bad = True
                        if st < 0 or bad:
                            break
                    if st < 0:
                        flags = GUIDE_ERR_NO_EDGE
                    elif not bad:
                        c = st
        allowed = np.zeros(vocab, dtype=bool)
        if not bad and c < ns:
            lo, hi = off[:lim], off[1:lim + 1]
            bad = bool(((lo < 0) | (hi < lo) | (hi > blen)).any())
            if not bad:
                ln = hi - lo
                st = np.where((ln >= 1) & (ln <= GUIDE_MAX_TOKEN_BYTES), c, -1).astype(np.int64)
                for level in range(GUIDE_MAX_TOKEN_BYTES):
                    idx = np.nonzero((st >= 0) & (level < ln))[0]
                    if not len(idx):
                        break
                    v = tr[st[idx], by[lo[idx] + level]].astype(np.int64)
                    bad = bad or bool(((v < -1) | (v >= ns)).any())
                    st[idx] = np.where((v < -1) | (v >= ns), -1, v)
                allowed[:lim] = st >= 0
                allowed[eos] = bool(ac[c])
        elif not bad:
            allowed[eos] = True
        if bad:
            err[s] |= GUIDE_ERR_TABLE
            continue
        cur[s] = c
        err[s] |= flags
        _guide_mask_row(logits, r, vocab, torch.from_numpy(allowed), lm_part)
    return logits


GUIDE_JSON_MAX_DEPTH = 32   # json_guide: containers open at once
GUIDE_JSON_MAX_STATES = 92  # json_guide: states of the pushdown table


def json_guide_rows(logits, slot, desc, trans, tok_off, tok_bytes, cur, jstk, err, advance_ids=None, lm_part=None):
    """ops.json_guide on host tensors (the contract of csrc/kernels/json_guide.hip): row r -> slot[r] -> desc
    (n_states, done, eos, 0); trans int16 [S, 256] holds -1 or next state | action << 8 (1 push-object, 2
    push-array, 3 pop: the landing state is the field + 0 / 1 / 2 for an object on top / an array / depth 0). The
    configuration (cur, jstk = (depth, stack bits)) advances over advance_ids[r] first (EOS from done or the sink:
    the sink; a token whose walk dies or pushes at the cap, without bytes, over the length cap, beyond the table,
    or any token but EOS in the sink: err |= 1, configuration kept). Allowed next: in the sink EOS alone; else EOS
    iff the state is done, and every token of 1..32 bytes whose walk never dies. Barred entries become -inf, the
    others keep their bits; lm_part candidates are overwritten with the best allowed entry. Anything out of bounds
    (any entry of the table's first n_states rows, a pop at depth 0): err |= 2 and row, candidates and configuration stay untouched."""
    import numpy as np

    vocab = logits.shape[1]
    tr = trans.numpy()
    off, by = tok_off.numpy().astype(np.int64), tok_bytes.numpy()
    n_tok, blen = len(off) - 1, len(by)
    lim = min(vocab, n_tok)
    cap = GUIDE_JSON_MAX_DEPTH

    def step(ns, st, dp, kb, b):
        """The chains (int64 arrays) over bytes b: (states or -1, depths, bits, a value was out of bounds)."""
        v = tr[st, b].astype(np.int64)
        none = v == -1
        nxt, act = v & 0xFF, (v >> 8) & 3
        push, pop = (act == 1) | (act == 2), act == 3
        oob = ~none & ((v < 0) | (v >= 1024) | (nxt + np.where(pop, 2, 0) >= ns) | (pop & (dp < 1)))
        dead = none | oob | (push & (dp >= cap))
        dpop = dp - 1
        k_push = kb | (np.where(act == 2, 1, 0) << np.minimum(dp, 31))
        k_pop = kb & ~(np.int64(1) << np.maximum(dpop, 0))
        top = np.where(dpop <= 0, 2, (k_pop >> np.maximum(dpop - 1, 0)) & 1)
        s_new = np.where(pop, nxt + top, nxt)
        kb = np.where(dead, kb, np.where(push, k_push, np.where(pop, k_pop, kb)))
        dp = np.where(dead, dp, np.where(push, dp + 1, np.where(pop, dpop, dp)))
        return np.where(dead, -1, s_new), dp, kb, bool(oob.any())

    for r in range(logits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        ns, done, eos = (int(v) for v in desc[s, :3])
        c, d, k = int(cur[s]), int(jstk[s, 0]), int(jstk[s, 1]) & 0xFFFFFFFF
        if (ns < 3 or ns > tr.shape[0] or ns > GUIDE_JSON_MAX_STATES or not 0 <= done < ns or not 0 <= c <= ns
                or not 0 <= d <= cap or (k >> d) != 0 or not 0 <= eos < vocab):
            err[s] |= GUIDE_ERR_TABLE
            continue
        t = tr[:ns].astype(np.int64)  # the whole table is validated at every launch
        if ((t != -1) & ((t < 0) | (t >= 1024) | ((t & 0xFF) + np.where(t >> 8 == 3, 2, 0) >= ns))).any():
            err[s] |= GUIDE_ERR_TABLE
            continue
        flags, bad = 0, False
        if advance_ids is not None:
            tok = int(advance_ids[r])
            if tok == eos:
                if c == ns or c == done:
                    c = ns
                else:
                    flags = GUIDE_ERR_NO_EDGE
            elif c == ns or not 0 <= tok < lim:
                flags = GUIDE_ERR_NO_EDGE
            else:
                lo, hi = int(off[tok]), int(off[tok + 1])
                if not 0 <= lo <= hi <= blen:
                    bad = True
                elif hi == lo or hi - lo > GUIDE_MAX_TOKEN_BYTES:
                    flags = GUIDE_ERR_NO_EDGE
                else:
                    st, dp, kb = np.array([c]), np.array([d]), np.array([k])
                    for p in range(lo, hi):
                        st, dp, kb, oob = step(ns, st, dp, kb, by[p:p + 1])
                        bad = bad or oob
                        if st[0] < 0:
                            break
                    if bad:
                        pass
                    elif st[0] < 0:
                        flags = GUIDE_ERR_NO_EDGE
                    else:
                        c, d, k = int(st[0]), int(dp[0]), int(kb[0])
        allowed = np.zeros(vocab, dtype=bool)
        if not bad and c < ns:
            lo, hi = off[:lim], off[1:lim + 1]
            bad = bool(((lo < 0) | (hi < lo) | (hi > blen)).any())
            if not bad:
                ln = hi - lo
                st = np.where((ln >= 1) & (ln <= GUIDE_MAX_TOKEN_BYTES), c, -1).astype(np.int64)
                dp, kb = np.full(lim, d, dtype=np.int64), np.full(lim, k, dtype=np.int64)
                for level in range(GUIDE_MAX_TOKEN_BYTES):
                    idx = np.nonzero((st >= 0) & (level < ln))[0]
                    if not len(idx):
                        break
                    st[idx], dp[idx], kb[idx], oob = step(ns, st[idx], dp[idx], kb[idx], by[lo[idx] + level])
                    bad = bad or oob
                allowed[:lim] = st >= 0
                allowed[eos] = c == done
        elif not bad:
            allowed[eos] = True
        if bad:
            err[s] |= GUIDE_ERR_TABLE
            continue
        cur[s] = c
        jstk[s, 0] = d
        jstk[s, 1] = k - (1 << 32) if k >= 1 << 31 else k
        err[s] |= flags
        _guide_mask_row(logits, r, vocab, torch.from_numpy(allowed), lm_part)
    return logits


GUIDE_SCHEMA_MAX_DEPTH = 32       # schema_guide: return states live at once
GUIDE_SCHEMA_TOKEN_PUSHES = 4     # schema_guide: a token's own pushes held at once
GUIDE_SCHEMA_STATE_ARENA = 16384  # schema_guide: states shared by all slots (trans int32 [., 256]: 16 MiB)


def schema_guide_rows(logits, slot, desc, trans, accept, tok_off, tok_bytes, cur, sdep, sstk, err, advance_ids=None,
                      lm_part=None):
    """ops.schema_guide on host tensors (the contract of csrc/kernels/schema_guide.hip): row r -> slot[r] -> desc
    (state_base, n_states, eos, 0) into trans int32 [A, 256] / accept uint8 [A]. An entry is -1 or next state |
    return state << 14 | action << 28 (1 push, 2 pop). The configuration (cur, sdep, sstk[:sdep]) advances over
    advance_ids[r] first (EOS from an accepting state at depth 0 or in the sink: the sink; a token whose walk dies,
    pushes at the depth cap or holds more than four of its own pushes, without bytes, over the length cap, beyond
    the table, or any token but EOS in the sink: err |= 1, configuration kept). Allowed next: in the sink EOS alone;
    else EOS iff the state accepts at depth 0, and every token of 1..32 bytes whose walk never dies. Barred entries
    become -inf, the others keep their bits; lm_part candidates are overwritten with the best allowed entry.
    Anything out of bounds (the region, the state, the depth, a live stack entry, eos, an offset, an entry read
    that is negative but not -1, has a bit above 29, action 3, a state field at or above n_states, or pops at depth
    0): err |= 2 and row, candidates and configuration stay untouched."""
    import numpy as np

    vocab = logits.shape[1]
    tr_all, ac_all = trans.numpy(), accept.numpy()
    off, by = tok_off.numpy().astype(np.int64), tok_bytes.numpy()
    arena, n_tok, blen = min(tr_all.shape[0], ac_all.shape[0]), len(off) - 1, len(by)
    lim = min(vocab, n_tok)
    cap, held_cap = GUIDE_SCHEMA_MAX_DEPTH, GUIDE_SCHEMA_TOKEN_PUSHES

    def step(tr, ns, stack, st, dp, ov, cnt, b):
        """The chains (int64 arrays; ov [N, 4]: a chain's own pushes, the latest first) over bytes b."""
        v = tr[st, b].astype(np.int64)
        none = v == -1
        nxt, ret, act = v & 0x3FFF, (v >> 14) & 0x3FFF, (v >> 28) & 3
        push, pop = act == 1, act == 2
        oob = ~none & ((v < 0) | (v >= 1 << 30) | (act == 3) | (nxt >= ns) | (ret >= ns) | (pop & (dp < 1)))
        dead = none | oob | (push & ((dp >= cap) | (cnt >= held_cap)))
        own = cnt > 0
        landed = np.where(own, ov[:, 0], stack[np.clip(dp - 1, 0, cap - 1)])
        do_push, do_pop = push & ~dead, pop & ~dead & own
        shifted_in = np.concatenate([ret[:, None], ov[:, :3]], axis=1)
        shifted_out = np.concatenate([ov[:, 1:], np.zeros((len(v), 1), dtype=np.int64)], axis=1)
        ov = np.where(do_push[:, None], shifted_in, np.where(do_pop[:, None], shifted_out, ov))
        cnt = cnt + do_push - do_pop
        dp = dp + do_push - (pop & ~dead)
        return np.where(dead, -1, np.where(pop, landed, nxt)), dp, ov, cnt, bool(oob.any())

    for r in range(logits.shape[0]):
        s = int(slot[r])
        if s < 0 or s >= desc.shape[0]:
            continue
        sb, ns, eos = (int(v) for v in desc[s, :3])
        c, d = int(cur[s]), int(sdep[s])
        if (sb < 0 or ns < 1 or sb + ns > arena or ns > 16384 or not 0 <= c <= ns or not 0 <= d <= cap
                or not 0 <= eos < vocab):
            err[s] |= GUIDE_ERR_TABLE
            continue
        stack = np.zeros(cap, dtype=np.int64)
        stack[:d] = sstk[s, :d].numpy()
        if ((stack[:d] < 0) | (stack[:d] >= ns)).any():
            err[s] |= GUIDE_ERR_TABLE
            continue
        tr, ac = tr_all[sb:sb + ns], ac_all[sb:sb + ns]
        flags, bad = 0, False
        if advance_ids is not None:
            tok = int(advance_ids[r])
            if tok == eos:
                if c == ns or (ac[c] and d == 0):
                    c = ns
                else:
                    flags = GUIDE_ERR_NO_EDGE
            elif c == ns or not 0 <= tok < lim:
                flags = GUIDE_ERR_NO_EDGE
            else:
                lo, hi = int(off[tok]), int(off[tok + 1])
                if not 0 <= lo <= hi <= blen:
                    bad = True
                elif hi == lo or hi - lo > GUIDE_MAX_TOKEN_BYTES:
                    flags = GUIDE_ERR_NO_EDGE
                else:
                    st, dp, cnt = np.array([c]), np.array([d]), np.array([0])
                    ov = np.zeros((1, 4), dtype=np.int64)
                    for p in range(lo, hi):
                        st, dp, ov, cnt, oob = step(tr, ns, stack, st, dp, ov, cnt, by[p:p + 1])
                        bad = bad or oob
                        if st[0] < 0:
                            break
                    if bad:
                        pass
                    elif st[0] < 0:
                        flags = GUIDE_ERR_NO_EDGE
                    else:
                        c, d, k = int(st[0]), int(dp[0]), int(cnt[0])
                        stack[d - k:d] = ov[0, :k][::-1]   # the token's pushes that are still held, oldest first
        allowed = np.zeros(vocab, dtype=bool)
        if not bad and c < ns:
            lo, hi = off[:lim], off[1:lim + 1]
            bad = bool(((lo < 0) | (hi < lo) | (hi > blen)).any())
            if not bad:
                ln = hi - lo
                st = np.where((ln >= 1) & (ln <= GUIDE_MAX_TOKEN_BYTES), c, -1).astype(np.int64)
                dp, cnt = np.full(lim, d, dtype=np.int64), np.zeros(lim, dtype=np.int64)
                ov = np.zeros((lim, 4), dtype=np.int64)
                for level in range(GUIDE_MAX_TOKEN_BYTES):
                    idx = np.nonzero((st >= 0) & (level < ln))[0]
                    if not len(idx):
                        break
                    st[idx], dp[idx], ov[idx], cnt[idx], oob = step(tr, ns, stack, st[idx], dp[idx], ov[idx],
                                                                   cnt[idx], by[lo[idx] + level])
                    bad = bad or oob
                allowed[:lim] = st >= 0
                allowed[eos] = bool(ac[c]) and d == 0
        elif not bad:
            allowed[eos] = True
        if bad:
            err[s] |= GUIDE_ERR_TABLE
            continue
        cur[s] = c
        sdep[s] = d
        sstk[s, :d] = torch.from_numpy(stack[:d]).to(sstk.dtype)
        err[s] |= flags
        _guide_mask_row(logits, r, vocab, torch.from_numpy(allowed), lm_part)
    return logits


POOL_MEAN, POOL_FIRST, POOL_FINAL = 1, 2, 4  # flag bits of a pool_embed segment descriptor


def pool_embed_rows(hidden, segs, acc, out, dims: int = 0, normalize: bool = True):
    """ops.pool_embed on host tensors (the contract of csrc/kernels/pooling.hip), fp32 throughout: per segment
    (first row, rows, slot, total, flags): the last row, or (FIRST ? 0 : acc[slot]) + the rows' sum, stored to
    acc[slot] unless FINAL, else divided by total; cut to the first dims components; divided by max(norm, 1e-12).
    A descriptor that does not fit the tensors writes nothing."""
    t, h = hidden.shape
    d = dims if dims else h
    for i in range(segs.shape[0]):
        first, rows, slot, total, flags = (int(v) for v in segs[i, :5])
        mean = bool(flags & POOL_MEAN)
        if first < 0 or rows < 1 or first + rows > t:
            continue
        if mean and (acc is None or not 0 <= slot < acc.shape[0] or total < 1):
            continue
        if not mean:
            v = hidden[first + rows - 1, :d].float()
        else:
            v = hidden[first:first + rows, :d].float().sum(0)
            if not flags & POOL_FIRST:
                v = acc[slot, :d] + v
            if not flags & POOL_FINAL:
                acc[slot, :d] = v
                continue
            v = v / torch.tensor(float(total), dtype=torch.float32)
        if normalize:
            v = v / torch.clamp(torch.sqrt((v * v).sum()), min=1e-12)
        out[i, :d] = v
    return out


def topk_softmax(gating: torch.Tensor, k: int, renorm: bool = True):
    """Slots in descending logit order, the lowest expert index first among equal logits: the rule of the HIP
    kernels (torch.topk leaves the order of ties open), stated by a stable descending sort."""
    g = _wide(gating)
    p = torch.softmax(g, dim=-1)
    ids = torch.sort(g, dim=-1, descending=True, stable=True).indices[..., :k]
    w = p.gather(-1, ids)
    if renorm:
        w = w / w.sum(-1, keepdim=True)
    return w, ids.int()


def moe_forward(x, w13, w2, gating, k: int, renorm: bool = True):
    """Reference MoE FFN: x [T,H], w13 [E, 2I, H], w2 [E, H, I]."""
    w, ids = topk_softmax(gating, k, renorm)
    return moe_experts(x, w13, w2, w, ids)


def moe_experts(x, w13, w2, w, ids):
    """Experts' weighted sum for given routing (w [T,k], ids [T,k]); ids >= E are skipped."""
    out = torch.zeros(x.shape, dtype=_wide(x).dtype, device=x.device)
    inter = w2.shape[-1]
    for e in range(w13.shape[0]):
        tok, slot = (ids == e).nonzero(as_tuple=True)
        if tok.numel() == 0:
            continue
        h = _wide(x[tok]) @ _wide(w13[e]).t()
        a = torch.nn.functional.silu(h[:, :inter]) * h[:, inter:]
        y = _wide(a.to(x.dtype)) @ _wide(w2[e]).t()
        out.index_add_(0, tok, y * w[tok, slot][:, None].to(out.dtype))
    return out.to(x.dtype)
