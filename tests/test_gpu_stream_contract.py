"""The stream= contract of hpc_patterns_amd.ops (docs/gemm.md, "Streams") on
the GPU: every piece of device work a call issues — pads, clones, kernels,
crops, copies into `out` — runs on the stream given, its temporaries live in
that stream's pool, and it never synchronizes the host.

Two fresh streams, `main` (made current) and `side` (passed as stream=),
chosen once so that they do not share a hardware queue (fixture `streams`). A
one-workgroup busy_wait of about BLOCK_MS holds one of them while the call is
issued; the result is read through `side` alone. Three probes per case
(tests/stream_contract_cases.py holds the table):

  A  blocker on main: work left on the current stream (a pad, a clone) waits
     behind it, and the kernel on side reads an operand not yet written
  B  blocker on side: work left on the current stream (the crop, out.copy_)
     runs at once, before the kernel
  C  blocker on side, then four poison tensors of every temporary's byte size
     are allocated and filled on main: a temporary taken from main's pool is
     handed out again while the kernel on side still needs it. The result is
     wrong, or — a workspace the kernel writes before it reads — the poison
     is overwritten; both are asserted.

Every probe asserts that the blocker was still running when the call
returned, and still running when the stream it does not hold had finished: a
probe whose blocker had finished, or whose streams were ordered by the
runtime anyway, proves nothing and fails as inconclusive, and a call that
synchronizes the host fails the same way.
Payloads are integers with an exact float64 reference (asserted per payload),
so every comparison is bitwise; each (case, probe) has a seed of its own, so
stale memory never holds the expected answer. BLOCK_MS = 200 was enough for
every case here.
"""

import pytest
import torch

import stream_contract_cases as cases

pytestmark = pytest.mark.gpu

BLOCK_MS = 200.0
BF = torch.bfloat16
_DT = {"bf16": BF, "fp8": torch.float8_e4m3fn, "i8": torch.int8}


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops
    from hpc_patterns_amd._native import native

    torch.cuda.set_device(0)
    native()  # fail loudly, not skip: on a GPU box it must exist
    return _ops


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.delenv("HPK_GEMM_GROUP", raising=False)
    monkeypatch.delenv("HPK_GEMM_VARIANT", raising=False)


@pytest.fixture(scope="module")
def blocker():
    """launch(stream) -> event recorded behind a busy_wait of ~BLOCK_MS on
    one workgroup; the tripcount is scaled from one timed launch"""
    from hpc_patterns_amd import ops as _ops

    torch.cuda.set_device(0)
    out = torch.zeros(64, device="cuda")
    probe_trips = 50_000
    _ops.busy_wait(out, probe_trips, globalsize=64)     # code object load
    t0, t1 = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    t0.record()
    _ops.busy_wait(out, probe_trips, globalsize=64)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1)
    assert ms > 0.5, f"busy_wait({probe_trips}) took {ms} ms: too short to scale"
    trips = int(probe_trips * BLOCK_MS / ms)
    print(f"blocker: {probe_trips} trips = {ms:.2f} ms -> {trips} trips")

    def launch(stream, scale=1.0):
        _ops.busy_wait(out, int(trips * scale), globalsize=64, stream=stream)
        done = torch.cuda.Event()
        done.record(stream)
        return done
    return launch


def _runs_ahead(blocker, held, free):
    """whether work on `free` completes while a (short) blocker holds `held`:
    two streams that the runtime put on one hardware queue do not"""
    buf = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    done = blocker(held, scale=0.1)
    with torch.cuda.stream(free):
        buf.fill_(1.0)
    passed = torch.cuda.Event()
    passed.record(free)
    passed.synchronize()
    ahead = not done.query()
    torch.cuda.synchronize()
    return ahead


@pytest.fixture(scope="module")
def streams(blocker):
    """(main, side): fresh streams, neither the legacy default stream, that
    run concurrently with each other and with the default stream. The
    runtime multiplexes streams onto a few hardware queues; a pair that
    shares one is ordered by accident, and every probe on it would pass
    whatever the call does — so such a pair is not used (and each probe
    checks again that the stream it does not block ran ahead)."""
    legacy = torch.cuda.default_stream()
    picked = []
    for _ in range(16):
        cand = torch.cuda.Stream()
        assert cand.cuda_stream != legacy.cuda_stream
        if all(cand.cuda_stream != s.cuda_stream
               and _runs_ahead(blocker, s, cand) for s in [legacy] + picked):
            picked.append(cand)
        if len(picked) == 2:
            return tuple(picked)
    pytest.fail("no two streams that run concurrently with each other and "
                "with the default stream among 16")


# ---------------------------------------------------------------------------
# per function: upload the payload, return call(stream) -> result tensors
# ---------------------------------------------------------------------------

def _stored(t, transposed):
    """logical [.., R, C] on the GPU, stored as it is or as its transpose
    (then handed over as the transposed view of that)"""
    if not transposed:
        return t.contiguous().cuda()
    return t.transpose(-1, -2).contiguous().cuda().transpose(-1, -2)


def _mx_operand(ops, t, fmt):
    """logical [R, K] float64 integers -> (q, scale) on the GPU, scale 127"""
    q = t.float().to(torch.float8_e4m3fn) if fmt == "mxfp8" \
        else ops.e2m1_pack(t.float())
    scale = torch.full((t.shape[0], t.shape[1] // 32), 127, dtype=torch.uint8)
    return q.cuda(), scale.cuda()


def _prepare(ops, case, p):
    kw = dict(case.kw)
    fn = getattr(ops, case.fn)
    nan = float("nan")

    if case.fn == "matmul_nt":
        bt = p.b.t()
        if case.path in ("mxfp8", "mxfp4"):
            (a, sa), (b, sb) = (_mx_operand(ops, t, case.path)
                                for t in (p.a, bt))
            return lambda s: (fn(a, b, sa, sb, stream=s),)
        a, b = (t.to(_DT[case.path]).contiguous().cuda() for t in (p.a, bt))
        return lambda s: (fn(a, b, stream=s, **kw),)

    if case.fn == "matmul_mx":
        a, b = p.a.to(BF).cuda(), p.b.t().to(BF).contiguous().cuda()
        return lambda s: (fn(a, b, fmt=case.path, stream=s),)

    if case.fn == "matmul":
        lay = kw.pop("layout", case.path)
        off = kw.pop("offset_a", 0)
        a = _stored(p.a.to(BF), lay[0] == "t")
        b = _stored(p.b.to(BF), lay[1] == "t")
        if off:     # the same values, `off` elements into an allocation
            flat = torch.zeros(a.numel() + 8, dtype=BF, device="cuda")
            flat[off:off + a.numel()] = a.reshape(-1)
            a = flat[off:off + a.numel()].view(a.shape)
            assert a.data_ptr() % 16 == 2 * off
        if kw.pop("out_dtype", None):
            kw["out_dtype"] = BF
        if kw.pop("bias", None):
            kw["bias"] = p.bias.float().cuda()
        if kw.get("activation_grad"):
            kw["activation_grad"] = (kw["activation_grad"],
                                     p.aux.to(BF).cuda())

        def call(s):
            res = fn(a, b, stream=s, **kw)
            return res if isinstance(res, tuple) else (res,)
        return call

    if case.fn == "bmm":
        batch = kw.pop("batch")
        if kw.pop("out_dtype", None):
            kw["out_dtype"] = BF
        if case.name == "bmm-heads":
            # a [H,T,D], b [H,D,T] as permutes of x, y [T, H*D]
            t_, d = p.a.shape[1], p.a.shape[2]
            x = p.a.to(BF).permute(1, 0, 2).reshape(t_, batch * d).cuda()
            y = p.b.to(BF).permute(2, 0, 1).reshape(t_, batch * d).cuda()
            a = x.view(t_, batch, d).permute(1, 0, 2)
            b = y.view(t_, batch, d).permute(1, 2, 0)
            assert ops.bmm_direct(a, 128, 64)
        else:
            a, b = p.a.to(BF).cuda(), p.b.to(BF).cuda()
            if kw.pop("broadcast_a", False):
                a = a.expand(batch, -1, -1)
        return lambda s: (fn(a, b, stream=s, **kw),)

    if case.fn == "colsum_bf16":
        x = p.a.to(BF).cuda()
        n = x.shape[1]
        out = None
        if kw.get("out") == "aligned":
            out = torch.full((n,), nan, device="cuda")
            assert out.data_ptr() % 16 == 0
        elif kw.get("out") == "offset":
            out = torch.full((n + 4,), nan, device="cuda")[1:n + 1]
            assert out.data_ptr() % 16 == 4
        return lambda s: (fn(x, out=out, stream=s),)

    if case.fn == "quantize_mx":
        x = p.a.to(BF).cuda()
        return lambda s: fn(x, case.path, stream=s)

    if case.fn in ("fill", "iota", "accumulate", "copy_kernel"):
        a, b = p.a.float().cuda(), p.b.float().cuda()
        if case.fn == "fill":
            value = float(p.wide[0][0])
            return lambda s: (fn(a, value, stream=s), a)[1:]
        if case.fn == "iota":
            return lambda s: (fn(a, stream=s), a)[1:]
        return lambda s: (fn(a, b, stream=s), a)[1:]

    # the strict GEMM calls: c is the caller's, poisoned
    lay = case.path if case.fn != "gemm_splitk" else "nt"
    dt = _DT.get(case.path, BF)
    a = p.a.t() if lay[0] == "t" else p.a
    b = p.b if lay in ("nn", "tn") else p.b.t()
    a, b = (t.to(dt).contiguous().cuda() for t in (a, b))
    m, n, _ = case.shape
    out_dt = p.refs[0].dtype
    if out_dt == torch.int32:
        c = torch.full((m, n), cases.I32_POISON, dtype=out_dt, device="cuda")
    else:
        c = torch.full((m, n), nan, dtype=out_dt, device="cuda")
    splits = kw.pop("splits")
    if kw.pop("bias", None):
        kw["bias"] = p.bias.float().cuda()
    if case.fn == "gemm_splitk":
        return lambda s: (fn(c, a, b, splits, stream=s), c)[1:]
    if case.fn == "gemm_bf16_layout_splitk":
        return lambda s: (fn(c, a, b, lay, splits, stream=s), c)[1:]
    res = (c,)
    if kw.pop("aux_out", None):
        kw["aux_out"] = torch.full((m, n), nan, dtype=BF, device="cuda")
        res = (c, kw["aux_out"])
    return lambda s: (fn(c, a, b, lay, splits=splits, stream=s, **kw),
                      *res)[1:]


def _refs(ops, case, p):
    if case.fn == "quantize_mx":
        return ops.quantize_mx_reference(p.a.to(BF), case.path)
    return p.refs


# ---------------------------------------------------------------------------
# the probes
# ---------------------------------------------------------------------------

def _poison_alloc(nbytes, integer):
    """nbytes from the current stream's pool, filled with NaN / 0x7FFFFFFF;
    returns (allocation, filled view)"""
    raw = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if integer:
        view = raw[:nbytes // 4 * 4].view(torch.int32)
        view.fill_(cases.I32_POISON)
    else:
        view = raw[:nbytes // 4 * 4].view(torch.float32)
        view.fill_(float("nan"))
    return raw, view


def _intact(view):
    if view.dtype == torch.int32:
        return bool((view == cases.I32_POISON).all())
    return bool(torch.isnan(view).all())


def _differences(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    g, r = (t.view(torch.uint8) if t.dtype in (torch.float8_e4m3fn,)
            else t for t in (got, ref))
    if torch.equal(g, r):
        return None
    bad = g != r  # NaN poison compares unequal too
    idx = bad.nonzero()[:4].tolist()
    return (f"{what}: {int(bad.sum())} of {g.numel()} outputs differ; first "
            f"(index, got, ref): "
            f"{[(i, g[tuple(i)].item(), r[tuple(i)].item()) for i in idx]}")


def _probe(ops, blocker, streams, case, probe, raw_handle=False):
    p = cases.payload(case.name, probe)
    cases.assert_exact(case, p)
    refs = _refs(ops, case, p)
    main, side = streams
    call = _prepare(ops, case, p)
    torch.cuda.synchronize()        # inputs ready, every stream idle
    integer = case.path == "i8"
    poison = []
    try:
        with torch.cuda.stream(main):
            done = blocker(main if probe == "A" else side)
            results = call(side.cuda_stream if raw_handle else side)
            running = not done.query()
            if probe == "C":
                poison = [_poison_alloc(nbytes, integer)
                          for nbytes in case.temps for _ in range(4)]
            if probe != "A":    # whatever was left on main has run by now
                main.synchronize()
                ahead = not done.query()
        with torch.cuda.stream(side):
            got = [r.cpu() for r in results]
        side.synchronize()
        if probe == "A":        # side never waited for main
            ahead = not done.query()
    finally:
        torch.cuda.synchronize()
    assert running, ("inconclusive: the blocker had finished when the call "
                     "returned (a host synchronization inside the call, or "
                     "a blocker that is too short)")
    assert ahead, ("inconclusive: the stream without the blocker did not "
                   "run ahead of it")
    assert len(got) == len(refs)
    problems = [_differences(g, r, f"{case.name} probe {probe} result {i}")
                for i, (g, r) in enumerate(zip(got, refs))]
    overwritten = sum(not _intact(view) for _, view in poison)
    if overwritten:
        problems.append(f"{overwritten} of {len(poison)} tensors allocated "
                        f"on the current stream after the call were "
                        f"overwritten by it")
    problems = [x for x in problems if x]
    assert not problems, "\n".join(problems)


_FRONT = cases.case_probes(cases.FRONT_DOOR_CASES)
_STRICT = cases.case_probes(cases.STRICT_CASES)


@pytest.mark.parametrize("name,probe", _FRONT,
                         ids=[f"{n}-{p}" for n, p in _FRONT])
def test_front_door(ops, blocker, streams, name, probe):
    _probe(ops, blocker, streams, cases.by_name(name), probe)


@pytest.mark.parametrize("handle", [False, True], ids=["torch", "raw"])
@pytest.mark.parametrize("name,probe", _STRICT,
                         ids=[f"{n}-{p}" for n, p in _STRICT])
def test_strict(ops, blocker, streams, name, probe, handle):
    _probe(ops, blocker, streams, cases.by_name(name), probe,
           raw_handle=handle)


def test_front_door_raw_handle(ops, blocker, streams):
    """a front door given the raw handle: the ExternalStream branch with
    pads, a bias, a workspace and a crop behind it"""
    case = cases.by_name("mm-tn-bf16-bias")
    for probe in "AC":
        _probe(ops, blocker, streams, case, probe, raw_handle=True)


# ---------------------------------------------------------------------------
# autograd under a non-default current stream
# ---------------------------------------------------------------------------

def _autograd_inputs(which):
    g = cases.gen("stream-contract-autograd", which)
    m, n, k = cases.RAGGED

    def t(*shape):
        return cases.ints(g, shape, 2).to(BF)

    if which == "bmm":
        return [t(3, m, k), t(3, k, n)], t(3, m, n)
    if which == "mlp-relu":
        return [t(m, k), t(n, k), t(n), t(k, n), t(k)], t(m, k)
    if which == "linear-bias":
        return [t(m, k), t(n, k), t(n)], t(m, n)
    return [t(m, k), t(n, k)], t(m, n)


def _autograd_run(ops, which, inputs, dy):
    """forward and backward on the current stream, on fresh leaves of the
    uploaded inputs; (y, grads...)"""
    xs = [x.detach().clone().requires_grad_() for x in inputs]
    if which == "bmm":
        y = ops.bmm_bf16(*xs)
    elif which == "mlp-relu":
        y = ops.mlp_bf16(*xs, activation="relu")
    elif which == "linear-bias":
        y = ops.linear_bf16(xs[0], xs[1], bias=xs[2])
    else:
        y = ops.linear_bf16(*xs)
    y.backward(dy)
    return [y.detach()] + [x.grad for x in xs]


@pytest.mark.parametrize("which", cases.AUTOGRAD)
def test_autograd_follows_the_current_stream(ops, blocker, streams, which):
    """linear_bf16, mlp_bf16 and bmm_bf16 take no stream=: under
    torch.cuda.stream(main) everything they issue, backward included, has to
    run on main. The legacy default stream is held by the blocker, so a
    launch or a torch op that leaks to it shows as a difference from the
    same call made with no stream context."""
    inputs, dy = _autograd_inputs(which)
    inputs, dy = [x.cuda() for x in inputs], dy.cuda()
    want = [t.cpu() for t in _autograd_run(ops, which, inputs, dy)]
    main, _ = streams
    torch.cuda.synchronize()
    try:
        done = blocker(torch.cuda.default_stream())
        with torch.cuda.stream(main):
            res = _autograd_run(ops, which, inputs, dy)
            running = not done.query()
            got = [t.cpu() for t in res]
        main.synchronize()
        ahead = not done.query()
    finally:
        torch.cuda.synchronize()
    assert running, "inconclusive: the blocker had finished after backward"
    assert ahead, ("inconclusive: main did not run ahead of the blocker on "
                   "the default stream")
    assert len(got) == len(want)
    problems = [_differences(g, w, f"{which} tensor {i}")
                for i, (g, w) in enumerate(zip(got, want))]
    problems = [x for x in problems if x]
    assert not problems, "\n".join(problems)
