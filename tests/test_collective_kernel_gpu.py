"""The one-shot collectives (csrc/kernels/allreduce.hip) and the tensor-parallel exchange of the decode GEMM's residual
epilogue (car_tile_exchange, gemm_decode.hip) against the float64 oracle of tests/collective_reference.py, on its plan
of calls, with 2, 4 and 8 ranks as processes sharing the one GPU. test_collective_reference_cpu.py proves for every
call used here that the mutations it claims (a rank dropped or doubled, the wrong staging half, the wrong order, a
skipped rounding, a neighbour's slice, row or tile, ...) change the expectation.

One module-scoped fixture per world size spawns the ranks once; every rank runs the whole plan in the same order
(inputs in NaN-poisoned buffers, outputs in sentinel-filled ones), then the refused launches on its own, and returns
bf16 / fp32 bit arrays, guard verdicts and the control words after every group. The parent judges case by case:
torch.equal on every output and every exact statistic, the derived bounds on the others, guards untouched, every rank
bit-identical, epoch / ticket / error words exact. After a timeout or a worker killed by a signal the remaining
children are terminated and the other world sizes fail at once without spawning anything."""

import hashlib
import os
import socket
import time
import traceback

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import collective_reference as cr  # noqa: E402

NAN = float("nan")
GUARD = 64                       # guard elements on either side of a flat tensor (128 bytes: keeps 16-byte alignment)
DEADLINE = 150.0                 # seconds for a world's ranks to report: start-up of 8 processes takes most of it
_ABORTED = []                    # set once a world hung or a worker died by a signal: nothing more is started


def _port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------------------------------------- worker side

def _poisoned(t: torch.Tensor, dev) -> torch.Tensor:
    """t on the device as a contiguous view of a NaN-filled buffer."""
    n = t.numel()
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=t.dtype, device=dev)
    v = buf[GUARD:GUARD + n].view(t.shape)
    v.copy_(t)
    return v


class _Guarded:
    """A tensor as a view of a sentinel-filled buffer; ok(*regions) is true when the buffer still holds the sentinel
    everywhere outside the given index regions."""

    def __init__(self, shape, dtype, dev, view, value=cr.SENT):
        self.value = int(value) if dtype == torch.int32 else value
        self.buf = torch.full(shape, self.value, dtype=dtype, device=dev)
        self.t = view(self.buf)

    def ok(self, *regions) -> bool:
        keep = torch.ones(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        for r in regions:
            keep[r] = False
        return bool((self.buf[keep] == self.value).all())


def _np(t: torch.Tensor) -> np.ndarray:
    return cr.bits(t.cpu()).numpy()


def _run_gemm(c, car, rank, x, w, resid_view, so, cb, dev):
    from src import ops

    wd = w.to(dev)
    if c.tiled:
        wd = ops.gd_pack_weights(wd, c.wr, kc=c.kc)
    assert car.fused_ok(c.ntiles), (c.ntiles, car.ranks_per_gpu, car.cus)
    car.row_parallel_residual(_poisoned(x, dev), _poisoned(wd, dev), resid_view, so.t, cb.t, c.wr, c.kc, c.sk, c.tiled,
                              half_ring=c.half_ring)


def _run_case(c, i, rank, cars, dev):
    """One call of the plan on this rank: {output name: bits}, guards verdict."""
    from src import _C

    car = cars[c.obj]
    args = (rank, car.bufs, car.sigs, car.ctl, car.cap)
    out = {}
    if c.kind == "ar":
        n = c.n
        g = _Guarded((n + 2 * GUARD,), torch.bfloat16, dev, lambda b: b[GUARD:GUARD + n])
        if c.inplace:
            g.t.copy_(i.xs[rank])
            src = g.t
        else:
            src = _poisoned(i.xs[rank], dev)
        _C.car_all_reduce(src, g.t, *args, c.blocks)
        out["out"] = _np(g.t)
        ok = g.ok(slice(GUARD, GUARD + n))
        if not c.inplace:   # the input is left as it was
            ok = ok and torch.equal(cr.bits(src.cpu()), cr.bits(i.xs[rank]))
    elif c.kind == "res":
        r, h = c.rows, c.hidden
        g = _Guarded(((r + 2) * h,), torch.bfloat16, dev, lambda b: b[h:(r + 1) * h].view(r, h))
        g.t.copy_(i.resid)
        ssp = _Guarded((r + 8,), torch.float32, dev, lambda b: b)
        car.all_reduce_residual(_poisoned(i.xs[rank], dev), g.t, ssp.t)
        out["out"], out["ss"] = _np(g.t), _np(ssp.t[:r])
        ok = g.ok(slice(h, (r + 1) * h)) and ssp.ok(slice(0, r))
    elif c.kind == "gat":
        r, wc = c.rows, car.world * c.cols
        g = _Guarded((r + 2, wc), torch.bfloat16, dev, lambda b: b[1:r + 1])
        _C.car_all_gather(_poisoned(i.xs[rank], dev), g.t, *args, c.blocks)
        out["out"] = _np(g.t)
        ok = g.ok(slice(1, r + 1))
    else:
        m, n, nt = c.rows, c.ncols, c.ntiles
        g = _Guarded((m + 2, n + 16), torch.bfloat16, dev, lambda b: b[1:m + 1, 8:8 + n])
        g.t.copy_(i.resid)
        so = _Guarded((nt + 1, cr.SSP_LD), torch.float32, dev, lambda b: b[:nt])
        cb = _Guarded((nt + 1,), torch.int32, dev, lambda b: b[:nt], cr.SENT_I)
        cb.t.zero_()
        _run_gemm(c, car, rank, i.xs[rank], i.ws[rank], g.t, so, cb, dev)
        out["out"], out["ss"] = _np(g.t), _np(so.t[:, :c.rr])
        ok = (g.ok((slice(1, m + 1), slice(8, 8 + n))) and so.ok((slice(0, nt), slice(0, c.rr)))
              and cb.ok(slice(0, nt)) and int(cb.t.abs().sum()) == 0)
    return out, bool(ok)


def _run_sequences(world, rank, car, dev, res):
    """The decode-shaped chain of five different collectives: two eager passes, then one captured graph replayed
    three times, every pass with freshly stamped inputs copied into the same buffers."""
    from src import ops

    m, n, nt, wr = cr.SEQ_ROWS, cr.SEQ_TILES * cr.SEQ_WR, cr.SEQ_TILES, cr.SEQ_WR
    chain0 = cr.seq_chain(0)
    k = chain0[0].k
    bf = dict(dtype=torch.bfloat16, device=dev)
    x0, x2 = torch.empty(m, k, **bf), torch.empty(m, k, **bf)
    w0, w2 = torch.empty(n, k, **bf), torch.empty(n, k, **bf)
    a1, b3 = torch.empty(m, n, **bf), torch.empty(m * n, **bf)
    g4 = torch.empty(m, chain0[4].cols, **bf)
    stream = torch.empty(m, n, **bf)
    snaps = [torch.empty(m, n, **bf) for _ in range(3)]
    ss0 = _Guarded((nt + 1, cr.SSP_LD), torch.float32, dev, lambda b: b[:nt])
    ss2 = _Guarded((nt + 1, cr.SSP_LD), torch.float32, dev, lambda b: b[:nt])
    ss1 = _Guarded((m + 8,), torch.float32, dev, lambda b: b)
    out3 = _Guarded((m * n + 2 * GUARD,), torch.bfloat16, dev, lambda b: b[GUARD:GUARD + m * n])
    cnt = torch.zeros(nt, dtype=torch.int32, device=dev)
    assert car.fused_ok(nt)

    def chain():
        car.row_parallel_residual(x0, w0, stream, ss0.t, cnt, wr, 128, 2, False)
        snaps[0].copy_(stream)
        car.all_reduce_residual(a1, stream, ss1.t)
        snaps[1].copy_(stream)
        car.row_parallel_residual(x2, w2, stream, ss2.t, cnt, wr, 128, 2, True)
        snaps[2].copy_(stream)
        car.all_reduce(b3, out3.t)
        return car.all_gather_last(g4)

    graph, gout = None, None
    for p in range(cr.SEQ_PASSES):
        cs = cr.seq_chain(p)
        ins = [cr.inputs(c.name, world) for c in cs]
        x0.copy_(ins[0].xs[rank]), w0.copy_(ins[0].ws[rank])
        a1.copy_(ins[1].xs[rank])
        x2.copy_(ins[2].xs[rank]), w2.copy_(ops.gd_pack_weights(ins[2].ws[rank].to(dev), wr, kc=128))
        b3.copy_(ins[3].xs[rank]), g4.copy_(ins[4].xs[rank])
        stream.copy_(cr.seq_resid(p, world))
        torch.cuda.synchronize()
        if p < cr.SEQ_EAGER:
            gout = chain()
        else:
            if graph is None:   # one graph, a single chain on one stream; capturing runs nothing
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    gout = chain()
            graph.replay()
        torch.cuda.synchronize()
        outs = [{"out": _np(snaps[0]), "ss": _np(ss0.t[:, :32])}, {"out": _np(snaps[1]), "ss": _np(ss1.t[:m])},
                {"out": _np(snaps[2]), "ss": _np(ss2.t[:, :32])}, {"out": _np(out3.t)}, {"out": _np(gout)}]
        ok = (ss0.ok((slice(0, nt), slice(0, 32))) and ss2.ok((slice(0, nt), slice(0, 32))) and ss1.ok(slice(0, m))
              and out3.ok(slice(GUARD, GUARD + m * n)) and int(cnt.abs().sum()) == 0)
        for c, o in zip(cs, outs):
            res["out"][c.name], res["guards"][c.name] = o, bool(ok)
        res["seq_ctl"].append(car.read_ctl())


def _refusals(world, rank, cars, dev):
    """Launches every binding has to refuse before anything runs: [(label, raised)]; this rank alone, no peer joins."""
    from src import _C
    from src.ops import MODE_RESID

    car, small = cars["main"], cars["small"]
    a = (rank, car.bufs, car.sigs, car.ctl, car.cap)
    bf = dict(dtype=torch.bfloat16, device=dev)
    x = torch.ones(64, **bf)
    big = torch.ones(small.cap + 8, **bf)
    wide = torch.ones(128, **bf)
    x2 = torch.ones(2, 16, **bf)
    ssp = torch.zeros(8, device=dev)
    null = [0 if p == (rank + 1) % world else b for p, b in enumerate(car.bufs)]

    def ar(t, o=None, rank_=rank, bufs=None, sigs=None, c=car, blocks=16):
        o = t if o is None else o
        return lambda: _C.car_all_reduce(t, o, rank_, c.bufs if bufs is None else bufs, c.sigs if sigs is None else sigs,
                                         c.ctl, c.cap, blocks)

    def gemm(mode=MODE_RESID, m=1, wr=64, nt=3, c=car):
        n = nt * wr
        xs, w = torch.ones(m, 128, **bf), torch.ones(n, 128, **bf)
        r = torch.ones(m, n, **bf)
        slab = torch.empty(1, m, n, device=dev)
        so = torch.zeros(nt, cr.SSP_LD, device=dev)
        cnt = torch.zeros(nt, dtype=torch.int32, device=dev)
        return lambda: _C.gemm_decode_car(slab, xs, w, mode, wr, 128, 1, True, r, so, cnt, rank, c.bufs, c.sigs, c.ctl,
                                          c.cap)

    cases = [
        ("n % 8", ar(torch.ones(12, **bf))),
        ("n > cap", ar(big, c=small)),
        ("blocks 0", ar(x, blocks=0)),
        ("blocks 257", ar(x, blocks=257)),
        ("1-entry peer list", ar(x, bufs=car.bufs[:1], sigs=car.sigs[:1], rank_=0)),
        ("9-entry peer list", ar(x, bufs=(car.bufs * 9)[:9], sigs=(car.sigs * 9)[:9])),
        ("null peer pointer", ar(x, bufs=null)),
        ("rank out of range", ar(x, rank_=world)),
        ("rank negative", ar(x, rank_=-1)),
        ("misaligned view", ar(wide[4:68])),
        ("non-contiguous input", ar(wide[::2])),
        ("in / out sizes differ", ar(x, wide)),
        ("residual rows 257", lambda: _C.car_all_reduce_residual(torch.ones(257, 8, **bf), torch.ones(257, 8, **bf),
                                                                 torch.zeros(264, device=dev), *a)),
        ("residual hidden % 8", lambda: _C.car_all_reduce_residual(torch.ones(2, 12, **bf), torch.ones(2, 12, **bf),
                                                                   ssp, *a)),
        ("residual ssp too small", lambda: _C.car_all_reduce_residual(torch.ones(9, 8, **bf), torch.ones(9, 8, **bf),
                                                                      ssp, *a)),
        ("gather cols % 8", lambda: _C.car_all_gather(torch.ones(2, 12, **bf), torch.ones(2, 12 * world, **bf), *a, 16)),
        ("gather out shape", lambda: _C.car_all_gather(x2, torch.ones(2, 16 * world + 8, **bf), *a, 16)),
        ("gather out rows", lambda: _C.car_all_gather(x2, torch.ones(3, 16 * world, **bf), *a, 16)),
        ("gemm_decode_car outside mode 3", gemm(mode=2)),
        ("gemm_decode_car M N > cap", gemm(m=33, nt=64, c=small)),
        ("gemm_decode_car N / wr > 256", gemm(wr=32, nt=257)),
    ]
    before = {o: c.read_ctl() for o, c in cars.items()}
    out = []
    for label, f in cases:
        try:
            f()
            out.append((label, False))
        except RuntimeError:
            out.append((label, True))
    torch.cuda.synchronize()
    after = {o: c.read_ctl() for o, c in cars.items()}
    return out, before, after


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from src.parallel.custom_allreduce import CustomAllReduce

        cars = {"main": CustomAllReduce(rank, world, max_bytes=cr.MAIN_BYTES, blocks=16),
                "small": CustomAllReduce(rank, world, max_bytes=cr.SMALL_BYTES, blocks=16)}
        assert {o: c.cap for o, c in cars.items()} == cr.CAPS
        res = {"out": {}, "guards": {}, "ctl": {}, "seq_ctl": []}
        t0 = time.time()
        for group in ("ar", "res", "gat", "gemm"):
            for name in cr.names(group):
                c = cr.case(name, world)
                res["out"][name], res["guards"][name] = _run_case(c, cr.inputs(name, world), rank, cars, dev)
            res["ctl"][group] = {o: c.read_ctl() for o, c in cars.items()}
        _run_sequences(world, rank, cars["main"], dev, res)
        res["ctl"]["seq"] = {o: c.read_ctl() for o, c in cars.items()}
        res["refused"], res["ctl_before"], res["ctl_after"] = _refusals(world, rank, cars, dev)
        res["seconds"] = time.time() - t0
        dist.barrier()
        for c in cars.values():
            c.close()
        # every rank reports a digest of each output; rank 0 the outputs themselves (numpy: pickled by value)
        res["digest"] = {n: hashlib.sha256(b"".join(v.tobytes() for _, v in sorted(o.items()))).hexdigest()
                         for n, o in res["out"].items()}
        if rank != 0:
            res["out"] = None
        q.put((rank, res))
        dist.destroy_process_group()
    except Exception:  # surface the failure in the parent
        q.put((rank, traceback.format_exc()))
        raise


# ---------------------------------------------------------------------------------------------- parent side

def _spawn(world):
    import queue

    import torch.multiprocessing as mp

    if _ABORTED:
        pytest.fail(f"not started: the {_ABORTED[0]}-rank run hung or a worker died by a signal")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    t0 = time.time()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    why = None
    while len(res) < world and why is None:
        try:
            r = q.get(timeout=2)
            res[r[0]] = r[1]
            if isinstance(r[1], str):
                why = f"rank {r[0]} raised:\n{r[1]}"
        except queue.Empty:
            if any(p.exitcode is not None and p.exitcode < 0 for p in procs):
                why = f"a worker ended by a signal: {[p.exitcode for p in procs]}"
            elif any(p.exitcode not in (None, 0) for p in procs) and q.empty():
                why = f"a worker failed: {[p.exitcode for p in procs]}"
            elif time.time() - t0 > DEADLINE:
                why = f"no report after {DEADLINE} s"
    if why is not None:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
        if "raised" not in why:
            _ABORTED.append(world)
        pytest.fail(why)
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    print(f"world {world}: {time.time() - t0:.1f} s in all, {res[0]['seconds']:.1f} s of calls on rank 0")
    return res


@pytest.fixture(scope="module")
def w2():
    return _spawn(2)


@pytest.fixture(scope="module")
def w4():
    return _spawn(4)


@pytest.fixture(scope="module")
def w8():
    return _spawn(8)


def _t(a: np.ndarray, dtype) -> torch.Tensor:
    return torch.from_numpy(a.copy()).view(dtype)


def _judge(name, world, got):
    st = cr.simulate(world)[name]
    c, e = st.c, st.exp
    if c.kind == "gat":
        assert torch.equal(_t(got["out"], torch.bfloat16).view(torch.int16), cr.bits(e.out)), f"{name}: gather"
        return
    out = _t(got["out"], torch.bfloat16).double()
    if c.kind == "gemm" and c.family == "random":
        lo, hi = cr.random_gemm_bracket(st)
        bad = (out < lo) | (out > hi)
        print(f"{name} W={world}: undecided {float((lo != hi).double().mean()):.3f}")
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the bracket"
    else:
        assert torch.equal(out, e.out), f"{name}: {int((out != e.out).sum())} of {out.numel()} elements differ"
    if e.ss is None:
        return
    ss = _t(got["ss"], torch.float32).double()
    if c.kind == "gemm":
        assert bool((ss[:, c.rows:] == 0).all()), f"{name}: ss rows M .. RR - 1 not zero"
        ss = ss[:, :c.rows]
    if c.family == "exact":
        assert torch.equal(ss, e.ss), f"{name}: ss differs in {int((ss != e.ss).sum())} entries"
        return
    if c.kind == "gemm":    # gemm_decode_reference's rule: against the sums of squares of the residual the kernel wrote
        ref = (out ** 2).view(c.rows, c.ntiles, c.wr).sum(-1).T
        tol = cr.gemm_ss_bound(ref, c.wr)
    else:
        ref, tol = e.ss, cr.ss_bound(e.ss, c.hidden)
    err = (ss - ref).abs()
    print(f"{name} W={world}: ss worst err / tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all()), f"{name}: ss off by up to {float((err / tol.clamp_min(1e-300)).max()):.2f} tol"


@pytest.mark.parametrize("name", [c.name for c, _ in cr.PLAN])
@pytest.mark.parametrize("world", cr.WORLDS)
def test_call_against_oracle(world, name, request):
    res = request.getfixturevalue(f"w{world}")
    assert res[0]["guards"][name], f"{name}: a guard or sentinel was written on rank 0"
    for r in range(1, world):
        assert res[r]["guards"][name], f"{name}: a guard or sentinel was written on rank {r}"
        assert res[r]["digest"][name] == res[0]["digest"][name], f"{name}: rank {r} differs from rank 0"
    _judge(name, world, res[0]["out"][name])
    c = cr.CASES[name]
    if c.twin:              # the half ring against the full ring on the same inputs
        a, b = res[0]["out"][name], res[0]["out"][c.twin]
        assert (a["out"] == b["out"]).all() and (a["ss"] == b["ss"]).all(), f"{name}: half ring != full ring"


@pytest.mark.parametrize("world", cr.WORLDS)
def test_control_words(world, request):
    """The epoch word equals the exact call count after every group and after every pass of the sequence (a captured
    graph advances it on the device), the ticket is back at 0 and the error word is 0, on every rank."""
    res = request.getfixturevalue(f"w{world}")
    for r in range(world):
        for group in cr.GROUPS:
            want = cr.epoch_after(group)
            for o in ("main", "small"):
                assert res[r]["ctl"][group][o] == [want[o], 0, 0], (r, group, o, res[r]["ctl"][group][o])
        base = cr.epoch_after("gemm")["main"]
        for p, ctl in enumerate(res[r]["seq_ctl"]):
            assert ctl == [base + 5 * (p + 1), 0, 0], (r, p, ctl)
        assert res[r]["ctl"]["seq"]["main"][0] == cr.FINAL_EPOCH["main"]


@pytest.mark.parametrize("world", cr.WORLDS)
def test_refused_launches(world, request):
    """Every refusal raises before any launch and consumes no epoch."""
    res = request.getfixturevalue(f"w{world}")
    for r in range(world):
        assert len(res[r]["refused"]) >= 20
        for label, raised in res[r]["refused"]:
            assert raised, f"rank {r}: '{label}' was not refused"
        assert res[r]["ctl_before"] == res[r]["ctl_after"] == res[r]["ctl"]["seq"], (r, res[r]["ctl_after"])


def test_rows_wording_matches_the_launcher():
    """The residual form takes one workgroup and one flag slot per row: up to 256 rows (128 run in the plan, 257 are
    among the refusals), and the binding's message says so."""
    assert any(c.kind == "res" and c.rows == 128 for c, _ in cr.plan(2))
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from src import _C

    x = torch.ones(257, 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="rows <= 256"):
        _C.car_all_reduce_residual(x, x.clone(), torch.zeros(264, device="cuda"), 0, [1, 1], [1, 1], 1, 1 << 20)


@pytest.mark.parametrize("nbytes", [16, 256 * 16, (2048 * 256 + 1) * 16])
def test_ipc_copy(nbytes):
    """ipc_copy_kernel through car_copy_to into a car_alloc'd buffer: one vector, one workgroup, and one vector more
    than the 2048 x 256 grid covers (the grid-stride loop takes a second turn); byte-exact inside sentinel guards."""
    if _ABORTED:
        pytest.fail("not started after a hung or killed run")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from src import _C

    g = 256
    total = (nbytes + 2 * g + 255) // 256 * 256
    ptr = _C.car_alloc(total)
    try:
        view = _C.car_tensor(ptr, total, torch.cuda.current_device())
        view.fill_(0xA5)
        gen = torch.Generator().manual_seed(nbytes)
        src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=gen)
        _C.car_copy_to(ptr + g, src.cuda())
        torch.cuda.synchronize()
        got = view.cpu()
        assert torch.equal(got[g:g + nbytes], src)
        assert bool((got[:g] == 0xA5).all()) and bool((got[g + nbytes:] == 0xA5).all())
        with pytest.raises(RuntimeError):
            _C.car_copy_to(ptr + g, torch.zeros(24, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        assert torch.equal(view.cpu(), got)
        del view
    finally:
        _C.car_release(ptr)
