"""CPU guards of tests/test_gpu_stream_contract.py: every ops function with
a stream= keyword is placed in the table, the padded shapes and temporary
sizes of the table are what the front doors compute, every case but the
"aligned, whole tiles" ones pads and crops, and every payload makes "bitwise
equal" the right expectation. No GPU."""

import inspect

import pytest
import torch

import stream_contract_cases as cases


@pytest.fixture
def ops():
    from hpc_patterns_amd import ops as _ops

    return _ops


def _with_stream(ops):
    return {name for name, fn in inspect.getmembers(ops, inspect.isfunction)
            if not name.startswith("_")
            and fn.__module__ == ops.__name__
            and "stream" in inspect.signature(fn).parameters}


def test_every_stream_keyword_is_placed(ops):
    """a new op with stream= fails here until someone places it"""
    found = _with_stream(ops)
    assert {"matmul", "bmm", "gemm_splitk", "reduce_sum", "fill"} <= found
    sets = [cases.FRONT_DOORS, set(cases.STRICT), set(cases.EXEMPT)]
    for name in sorted(found):
        assert sum(name in s for s in sets) == 1, \
            f"ops.{name} takes stream=: place it in exactly one of " \
            f"FRONT_DOORS, STRICT and EXEMPT of stream_contract_cases.py"
    for s in sets:
        assert s <= found, f"no longer ops functions with stream=: {s - found}"
    for name, reason in cases.EXEMPT.items():
        assert isinstance(reason, str) and reason and "\n" not in reason


def test_every_placed_function_has_its_probes():
    names = [c.name for c in cases.all_cases()]
    assert len(set(names)) == len(names)
    front = {c.fn for c in cases.FRONT_DOOR_CASES}
    assert front == cases.FRONT_DOORS
    own = {c.fn for c in cases.STRICT_CASES}
    for fn, via in cases.STRICT.items():
        if via is None:
            assert fn in own, f"{fn} has no STRICT_CASES"
        else:
            assert cases.by_name(via) in cases.FRONT_DOOR_CASES
    assert own == {fn for fn, via in cases.STRICT.items() if via is None}
    for c in cases.all_cases():
        assert c.probes in ("ABC", "BC", "B")
        # without a temporary to hand out again probe C is probe B
        assert "C" in c.probes or not c.temps
        assert all(t > 0 for t in c.temps)
    for c in cases.STRICT_CASES:
        assert "A" not in c.probes


def _padded(ops, c):
    m, n, k = c.shape
    if c.fn == "matmul_nt":
        if "split_k" in c.kw:
            return ops.gemm_layout_pad_shapes(m, n, k)  # 128 / 128 / 64
        return ops.gemm_pad_shapes(c.path, m, n, k)
    if c.fn == "matmul_mx":
        return ops.gemm_pad_shapes(c.path, m, n, -(-k // 32) * 32)
    if c.fn == "matmul" and c.path == "nt" and not c.kw:
        return ops.gemm_pad_shapes("bf16", m, n, k)     # matmul_nt
    return ops.gemm_layout_pad_shapes(m, n, k)


def _gemm_temps(c, es_in):
    """byte sizes from the padded shape: the operands that are copied, C when
    it is cropped, the workspace, the padded bias and aux"""
    mp, np_, kp = c.padded
    m, n, k = c.shape
    batch = c.kw.get("batch", 1)
    out = 2 if c.kw.get("out_dtype") == "bf16" else 4
    temps = []
    if (m, k) != (mp, kp) or c.kw.get("offset_a"):
        temps.append((1 if c.kw.get("broadcast_a") else batch) * mp * kp
                     * es_in)
    if (n, k) != (np_, kp):
        temps.append(batch * np_ * kp * es_in)
    if (m, n) != (mp, np_):
        temps.append(batch * mp * np_ * out)
        if c.kw.get("return_aux") or c.kw.get("activation_grad"):
            temps.append(mp * np_ * 2)
        if c.kw.get("bias"):
            temps.append(np_ * 4)
    if c.kw.get("split_k"):
        temps.append(c.kw["split_k"] * mp * np_ * 4)
    return temps


def test_padded_shapes_and_temporaries(ops):
    from hpc_patterns_amd._native import native

    lib = native()
    for c in cases.FRONT_DOOR_CASES:
        m, n, k = c.shape
        if c.fn == "colsum_bf16":
            n8 = -(-n // 8) * 8
            chunks = {lib.colsum_plan(m, n8, cu) for cu in (1, 64, 256)}
            assert chunks == {c.padded[2]}      # whatever the device
            assert c.padded[:2] == (m, n8)
            width = n8 if c.padded[2] == 1 else lib.colsum_pitch(n8)
            out = c.kw.get("out")
            direct = out == "aligned" and width == n
            want = [m * n8 * 2] if n8 != n else []
            if out is not None and not direct:  # buf is dropped after copy_
                want.append((width + (lib.colsum_pitch(n8) * c.padded[2]
                                      if c.padded[2] > 1 else 0)) * 4)
            assert sorted(c.temps) == sorted(want), c.name
            pads = n8 != n or (out is not None and not direct)
        else:
            assert tuple(c.padded) == tuple(_padded(ops, c)), c.name
            mp, np_, kp = c.padded
            pads = (m, k) != (mp, kp) or (n, k) != (np_, kp)
            crops = (m, n) != (mp, np_)
            if c.fn == "matmul_mx":
                k32 = -(-k // 32) * 32
                q = 1 if c.path == "mxfp8" else 2
                want = [m * k32 * 2, n * k32 * 2, m * k32 // q, n * k32 // q,
                        m * k32 // 32, n * k32 // 32,
                        mp * kp // q, np_ * kp // q, mp * np_ * 4,
                        mp * kp // 32, np_ * kp // 32]
            elif c.path in ("mxfp8", "mxfp4"):
                q = 1 if c.path == "mxfp8" else 2
                want = [mp * kp // q, np_ * kp // q, mp * np_ * 4,
                        mp * kp // 32, np_ * kp // 32]
            else:
                want = _gemm_temps(c, 1 if c.path in ("fp8", "i8") else 2)
            assert sorted(c.temps) == sorted(want), c.name
            if not c.path.startswith(cases.ALIGNED):
                assert pads and crops, c.name
        if c.path.startswith(cases.ALIGNED):
            assert c.shape[:2] == c.padded[:2]
        else:
            assert pads, c.name
    for c in cases.STRICT_CASES:
        if "splits" in c.kw:
            m, n, _ = c.shape
            assert c.temps == (c.kw["splits"] * m * n * 4,)
            assert c.shape == c.padded
            assert ops.gemm_layout_pad_shapes(*c.shape) == c.shape


def test_heads_case_copies_nothing(ops):
    c = cases.by_name("bmm-heads")
    t_, _, d = c.shape
    h = c.kw["batch"]
    x = torch.zeros(t_, h * d, dtype=torch.bfloat16)
    a = x.view(t_, h, d).permute(1, 0, 2)
    b = x.view(t_, h, d).permute(1, 2, 0)
    layout, a_st, b_st = ops.bmm_layout(a, b)
    assert layout == "nt"
    assert ops.bmm_direct(a_st, 128, 64) and ops.bmm_direct(b_st, 128, 64)
    assert ops.gemm_layout_pad_shapes(*c.shape) == c.shape and not c.temps


def test_every_payload_is_exact():
    seen = set()
    for c in cases.all_cases():
        for probe in c.probes:
            p = cases.payload(c.name, probe)
            cases.assert_exact(c, p)
            # a seed of its own: no two (case, probe) share their operands
            key = (tuple(p.a.shape), p.a.flatten()[:64].tolist().__repr__())
            assert key not in seen, (c.name, probe)
            seen.add(key)
            for ref in p.refs:      # not a constant a stale buffer could hold
                assert ref.double().std() > 0 or c.fn == "fill"


def test_mx_payloads_quantize_exactly(ops):
    """integers -4..4 survive both MX formats, so the float64 product is the
    reference of the MX cases too: as e4m3 / e2m1 values under the scale byte
    127 where the test builds the MX operands itself (matmul_nt), and through
    quantize_mx_reference — which picks the scale from the block maximum —
    where the call quantizes (matmul_mx, quantize_mx)"""
    checked = 0
    for c in cases.all_cases():
        if c.path not in ("mxfp8", "mxfp4"):
            continue
        for probe in c.probes:
            p = cases.payload(c.name, probe)
            k = c.shape[2]
            k32 = -(-k // 32) * 32
            for t in [p.a] if p.b is None else [p.a, p.b.t()]:
                x = torch.zeros(t.shape[0], k32)
                x[:, :k] = t.float()
                if c.fn == "matmul_nt":
                    q = x.to(torch.float8_e4m3fn) if c.path == "mxfp8" \
                        else ops.e2m1_pack(x)
                    scale = torch.full((x.shape[0], k32 // 32), 127,
                                       dtype=torch.uint8)
                else:
                    q, scale = ops.quantize_mx_reference(x, c.path)
                assert torch.equal(ops.dequantize_mx(q, scale, c.path),
                                   x.double())
                checked += 1
    assert checked >= 2 * 3 * 4 + 2


def test_on_stream_none_is_the_function_itself(ops):
    """stream=None takes no context at all; the wrapper keeps the signature"""
    assert ops._on(None) is ops._NO_SWITCH
    for name in cases.FRONT_DOORS:
        fn = getattr(ops, name)
        assert "stream" in inspect.signature(fn).parameters
        assert fn.__wrapped__.__name__ == name and fn.__doc__
