"""ops — hand-written HIP/CDNA4 kernels exposed on torch tensors.

Python face of the native kernels in native/kernels.hip (the MI355X
equivalents of the reference's device-code sites). All
functions launch on the CURRENT torch CUDA stream unless given one, and all
REQUIRE the native extension when a GPU is present — no silent eager
fallback. A function given stream= issues ALL its device work — pads,
casts, copies and allocations as well as kernels — on that stream
(docs/gemm.md, "Streams").
"""

from __future__ import annotations

import contextlib
import functools
import inspect

import torch

from .._native import native


def _stream_handle(stream=None) -> int:
    if stream is not None:
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    return torch.cuda.current_stream().cuda_stream


_NO_SWITCH = contextlib.nullcontext()


def _on(stream):
    """Context that makes `stream` torch's current stream, so that torch ops
    and the caching allocator follow the kernels (docs/gemm.md, "Streams").
    None — and a stream that is current already — switch nothing. A raw
    handle, as _stream_handle takes it, is wrapped in an ExternalStream."""
    if stream is None:
        return _NO_SWITCH
    if not hasattr(stream, "cuda_stream"):
        stream = torch.cuda.ExternalStream(int(stream))
    if stream.cuda_stream == torch.cuda.current_stream().cuda_stream:
        return _NO_SWITCH
    return torch.cuda.stream(stream)


def _body_on_stream(fn):
    """Run the whole of fn under _on(its stream argument); stream=None calls
    fn as it is."""
    pos = list(inspect.signature(fn).parameters).index("stream")

    @functools.wraps(fn)
    def on_stream(*args, **kwargs):
        stream = args[pos] if len(args) > pos else kwargs.get("stream")
        if stream is None:
            return fn(*args, **kwargs)
        with _on(stream):
            return fn(*args, **kwargs)
    return on_stream


def _check_f32(t: torch.Tensor, name: str):
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous float32 CUDA tensor")


def busy_wait(out: torch.Tensor, tripcount: int, globalsize: int | None = None,
              stream=None) -> None:
    """K1: every work-item runs 64*tripcount dependent FMAs, stores 1 float.

    Reference payload: concurency/bench.hpp:23-31 (MAD_64) submitted at
    bench_sycl.cpp:92-97.
    """
    _check_f32(out, "out")
    gs = out.numel() if globalsize is None else globalsize
    if gs > out.numel():
        raise ValueError("globalsize exceeds out buffer")
    native().busy_wait(out.data_ptr(), int(tripcount), int(gs),
                       _stream_handle(stream))


def busy_wait_mfma(out: torch.Tensor, tripcount: int, n_waves: int = 1,
                   stream=None) -> None:
    """K1-MFMA: chained v_mfma_f32_16x16x32_bf16 busy loop (matrix cores)."""
    _check_f32(out, "out")
    if out.numel() < ((n_waves * 64 + 255) // 256) * 256:
        raise ValueError("out too small: need >= ceil(n_waves*64/256)*256 floats")
    native().busy_wait_mfma(out.data_ptr(), int(tripcount), int(n_waves),
                            _stream_handle(stream))


def copy_kernel(dst: torch.Tensor, src: torch.Tensor, stream=None) -> None:
    """K2: vectorized shader copy (the blit-engine sibling of hipMemcpyAsync)."""
    if dst.numel() * dst.element_size() != src.numel() * src.element_size():
        raise ValueError("size mismatch")
    if not (dst.is_contiguous() and src.is_contiguous()):
        raise TypeError("contiguous tensors required")
    if not (dst.is_cuda and src.is_cuda):
        raise TypeError("dst and src must be CUDA tensors (a host pointer "
                        "would crash the GPU copy kernel)")
    native().copy_kernel(dst.data_ptr(), src.data_ptr(),
                         dst.numel() * dst.element_size(),
                         _stream_handle(stream))


def fill(dst: torch.Tensor, value: float, stream=None) -> None:
    """K4: dst[:] = value (reference Initialize, allreduce-mpi-sycl.cpp:34-41)."""
    _check_f32(dst, "dst")
    native().fill_f32(dst.data_ptr(), float(value), dst.numel(),
                      _stream_handle(stream))


def iota(dst: torch.Tensor, stream=None) -> None:
    """dst[i] = float(i) — device-side checksum payload generator."""
    _check_f32(dst, "dst")
    native().iota_f32(dst.data_ptr(), dst.numel(), _stream_handle(stream))


def accumulate(dst: torch.Tensor, src: torch.Tensor, stream=None) -> None:
    """K3: dst += src (reference Accumulate, allreduce-mpi-sycl.cpp:27-31)."""
    _check_f32(dst, "dst")
    _check_f32(src, "src")
    if dst.numel() != src.numel():
        raise ValueError("size mismatch")
    native().acc_f32(dst.data_ptr(), src.data_ptr(), dst.numel(),
                     _stream_handle(stream))


def reduce_sum(src: torch.Tensor, stream=None) -> float:
    """Exact float64 sum of a float32 tensor (device reduction; synchronizes).

    Order-independent when all addends are integer-valued (every partial sum
    stays below 2^53), which is what the checksum payloads guarantee —
    replaces the reference's host sort+sum (peer2pear.cpp:56-63).
    """
    _check_f32(src, "src")
    return native().reduce_sum_f32(src.data_ptr(), src.numel(),
                                   _stream_handle(stream))


def iota_checksum(n: int) -> float:
    """Expected exact double sum of [float(i) for i in range(n)]."""
    import numpy as np

    # float32 rounding of the iota values, summed exactly in float64
    return float(np.arange(n, dtype=np.float32).astype(np.float64).sum())


def gemm_bf16(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
              stream=None, xcd_swizzle: bool = False) -> None:
    """K7 (r2): C[M,N] fp32 = A[M,K] @ B[N,K]^T, A/B bf16 K-contiguous.

    Hand-written LDS-tiled v_mfma_f32_16x16x32_bf16 kernel (native/gemm.hip):
    zero-bank-conflict cyclic-skew LDS layout, 16-byte global_load_lds
    staging, and (for M,N % 256, K % 128 shapes) the 256^2-tile 8-phase
    counted-vmcnt pipeline selected by default — 1085 TF bf16 at 8192^3 on
    random operands (43% of the 2.5 PF dense peak;
    profiles/gemm_showcase_r2.log). HPK_GEMM_VARIANT=plain|db|8ph forces a
    variant. xcd_swizzle enables the bijective XCD workgroup remap
    (measured slower here, off by default). Requires M,N multiples of 128
    and K a multiple of 64 (use matmul_nt for arbitrary shapes).
    """
    if c.dtype != torch.float32 or a.dtype != torch.bfloat16 \
            or b.dtype != torch.bfloat16:
        raise TypeError("c must be fp32; a, b must be bf16")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, k = a.shape
    n, kb = b.shape
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    native().gemm_bf16_nt(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                          m, n, k, _stream_handle(stream), int(xcd_swizzle))


def gemm_fp8(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
             stream=None, xcd_swizzle: bool = False) -> None:
    """K7-fp8: C[M,N] fp32 = A[M,K] @ B[N,K]^T, A/B torch.float8_e4m3fn.

    gfx950 fp8 is OCP e4m3 — exactly torch's float8_e4m3fn. Default for
    256-divisible shapes: the 256^2-tile 32x32x64 scaled-MFMA kernel with
    hardcoded x1.0 scales (2154-2194 TF — no non-scaled 32x32x64 fp8 MFMA
    exists); otherwise the mfma_f32_16x16x32_fp8_fp8 family
    (HPK_GEMM_VARIANT=8ph|plain|db selects). Same shape constraints as
    gemm_bf16.
    """
    if c.dtype != torch.float32 or a.dtype != torch.float8_e4m3fn \
            or b.dtype != torch.float8_e4m3fn:
        raise TypeError("c must be fp32; a, b must be float8_e4m3fn")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, k = a.shape
    n, kb = b.shape
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    native().gemm_fp8_nt(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                         m, n, k, _stream_handle(stream), int(xcd_swizzle))


def gemm_mxfp8(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
               a_scale: torch.Tensor, b_scale: torch.Tensor,
               stream=None, xcd_swizzle: bool = False) -> None:
    """K7-mx: block-scaled MX-fp8 GEMM (the 2x-bf16 rate class;
    1824-1863 TF via the default 256^2-tile 32x32x64 kernel for
    256-divisible shapes, HPK_MX8_VARIANT=plain selects the 128^2 one).

    C[M,N] fp32 = (A * 2^(As-127)) @ (B * 2^(Bs-127))^T — A/B are
    float8_e4m3fn [M,K]/[N,K]; a_scale/b_scale are uint8 e8m0 exponents
    with ONE scale per 32-element K-block ([M,K//32] / [N,K//32]; 127 =
    scale 1.0) — the OCP MX-FP8 format, dequantized in hardware by
    mfma_scale_f32_16x16x128_f8f6f4. Requires M,N,K multiples of 128.

    Scale bytes 0..254 are all exact (the exponents of both scales add;
    only the product has to fit fp32). Byte 255 is the e8m0 NaN: the
    block reads as all NaN, like the element codes 0x7F / 0xFF, and makes
    its row / column of C NaN (findings.md #31).
    """
    if c.dtype != torch.float32 or a.dtype != torch.float8_e4m3fn \
            or b.dtype != torch.float8_e4m3fn:
        raise TypeError("c must be fp32; a, b must be float8_e4m3fn")
    if a_scale.dtype != torch.uint8 or b_scale.dtype != torch.uint8:
        raise TypeError("scales must be uint8 (e8m0 exponents)")
    for t, name in ((c, "c"), (a, "a"), (b, "b"),
                    (a_scale, "a_scale"), (b_scale, "b_scale")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, k = a.shape
    n, kb = b.shape
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    if a_scale.shape != (m, k // 32) or b_scale.shape != (n, k // 32):
        raise ValueError("scales must be [rows, K//32]")
    native().gemm_mxfp8_nt(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                           a_scale.data_ptr(), b_scale.data_ptr(),
                           m, n, k, _stream_handle(stream), int(xcd_swizzle))


# the 16 OCP e2m1 (fp4) values, indexed by nibble
_E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0]


def e2m1_pack(t: torch.Tensor) -> torch.Tensor:
    """Pack a float tensor of exactly-representable e2m1 values
    (0, ±0.5, ±1, ±1.5, ±2, ±3, ±4, ±6) into uint8 nibbles, two per byte
    (low nibble = even index along the last dim). Raises on values
    outside the e2m1 set — this is a test/packing utility, not a
    quantizer. Last dim must be even."""
    if t.shape[-1] % 2 != 0:
        raise ValueError("last dim must be even")
    table = torch.tensor(_E2M1_VALUES[:8], dtype=torch.float32,
                         device=t.device)
    mag = t.abs().float()
    idx = (mag.unsqueeze(-1) == table).to(torch.uint8).argmax(-1)
    ok = table[idx] == mag
    if not bool(ok.all()):
        raise ValueError("tensor contains values not representable in e2m1")
    nib = (idx + 8 * (t < 0).to(idx.dtype)).to(torch.uint8)
    lo = nib[..., 0::2]
    hi = nib[..., 1::2]
    return (lo | (hi << 4)).contiguous()


def e2m1_decode(p: torch.Tensor) -> torch.Tensor:
    """Inverse of e2m1_pack: uint8 nibble-packed -> float32 (last dim
    doubles)."""
    table = torch.tensor(_E2M1_VALUES, dtype=torch.float32, device=p.device)
    lo = table[(p & 0xF).long()]
    hi = table[(p >> 4).long()]
    out = torch.stack([lo, hi], dim=-1)
    return out.view(*p.shape[:-1], p.shape[-1] * 2)


def gemm_mxfp4(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
               a_scale: torch.Tensor, b_scale: torch.Tensor,
               stream=None, xcd_swizzle: bool = False) -> None:
    """K7-mx4: block-scaled OCP MX-fp4 GEMM — the 4x-bf16 MFMA rate class.

    C[M,N] fp32 = (A * 2^(As-127)) @ (B * 2^(Bs-127))^T where A/B are
    nibble-PACKED e2m1 uint8 tensors [M,K//2]/[N,K//2] (low nibble = even
    k; e2m1_pack produces this layout) and a_scale/b_scale are e8m0
    exponents [M,K//32]/[N,K//32] as for gemm_mxfp8. The fp4 mode of the
    scaled MFMAs; operand/scale layout measured on hardware (diagonal —
    scripts/probes/fp4_probe*). Default kernel: the 256^2-tile
    double-buffered 32x32x64 design, 2903-3197 TF at 8192^3-16384^3
    (3.2 PFLOP/s; HPK_MX4_WAVES=db|8|4 selects the 128^2 variants, used
    automatically when M or N is not a multiple of 256). K =
    2*a.shape[1]; requires M,N,K % 128 == 0.

    Scale bytes 0..254 are all exact, as for gemm_mxfp8. e2m1 has no NaN
    code, but scale byte 255 (e8m0 NaN) makes its block all NaN and so
    its row / column of C (findings.md #31).
    """
    if c.dtype != torch.float32 or a.dtype != torch.uint8 \
            or b.dtype != torch.uint8:
        raise TypeError("c must be fp32; a, b must be nibble-packed uint8")
    if a_scale.dtype != torch.uint8 or b_scale.dtype != torch.uint8:
        raise TypeError("scales must be uint8 (e8m0 exponents)")
    for t, name in ((c, "c"), (a, "a"), (b, "b"),
                    (a_scale, "a_scale"), (b_scale, "b_scale")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, kb = a.shape
    n, kb2 = b.shape
    k = kb * 2
    if kb2 != kb or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    if a_scale.shape != (m, k // 32) or b_scale.shape != (n, k // 32):
        raise ValueError("scales must be [rows, K//32]")
    native().gemm_mxfp4_nt(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                           a_scale.data_ptr(), b_scale.data_ptr(),
                           m, n, k, _stream_handle(stream), int(xcd_swizzle))


def gemm_i8(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
            stream=None, xcd_swizzle: bool = False) -> None:
    """K7-i8: C[M,N] int32 = A[M,K] @ B[N,K]^T, int8 operands.

    mfma_i32_16x16x64_i8 at ~2x the bf16 MFMA rate with EXACT int32
    accumulation — the quantized-inference dtype. Same NT layout and
    shape constraints as gemm_bf16 (M,N % 128, K % 64).
    """
    if c.dtype != torch.int32 or a.dtype != torch.int8 or b.dtype != torch.int8:
        raise TypeError("c must be int32; a, b must be int8")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, k = a.shape
    n, kb = b.shape
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    native().gemm_i8_nt(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                        m, n, k, _stream_handle(stream), int(xcd_swizzle))


# operand dtype -> (native kind, dtype of C and of the workspace)
_SPLITK_KINDS = {torch.bfloat16: ("bf16", torch.float32),
                 torch.float8_e4m3fn: ("fp8", torch.float32),
                 torch.int8: ("i8", torch.int32)}


def gemm_splitk(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                splits: int, workspace: torch.Tensor = None, stream=None,
                xcd_swizzle: bool = False) -> None:
    """K7 split-K: C[M,N] = A[M,K] @ B[N,K]^T with the K loop cut into
    `splits` parts that run as separate workgroups (native/gemm_splitk.hip)
    — for small M, N and a long K, where one workgroup per output tile
    leaves most of the machine idle.

    Dispatches on a.dtype: bf16 or float8_e4m3fn (c fp32), int8 (c int32,
    exact). Split s of S walks T/S + (s < T%S) consecutive K-tiles of 64
    (T = K/64) and writes its partial to workspace[s]; a second kernel on
    the same stream computes C = ((P0 + P1) + P2) + ... in ascending s, so
    the result is deterministic. splits == 1 writes C directly. Requires
    M,N % 128 == 0, K % 64 == 0 and 1 <= splits <= K/64 (matmul_nt pads).

    workspace: None allocates [splits, M, N] of c's dtype; a caller's must
    be a contiguous CUDA tensor of c's dtype with at least splits*M*N
    elements, starting on a 16-byte boundary. It is scratch: its first
    splits*M*N elements are overwritten, the rest is not touched.
    """
    if a.dtype not in _SPLITK_KINDS:
        raise TypeError(f"unsupported operand dtype {a.dtype}: gemm_splitk "
                        f"takes bfloat16, float8_e4m3fn or int8")
    kind, out_dtype = _SPLITK_KINDS[a.dtype]
    if b.dtype != a.dtype or c.dtype != out_dtype:
        raise TypeError(f"b must be {a.dtype} like a, and c {out_dtype}")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    m, k = a.shape
    n, kb = b.shape
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)}"
                         f" C{tuple(c.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_splitk requires M,N % 128 == 0 and "
                         f"K % 64 == 0; got M={m} N={n} K={k}")
    splits = int(splits)
    if not 1 <= splits <= k // 64:
        raise ValueError(f"need 1 <= splits <= K/64 = {k // 64}; got {splits}")
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda \
                or not workspace.is_contiguous() \
                or workspace.dtype != c.dtype:
            raise TypeError(f"workspace must be a contiguous {c.dtype} CUDA "
                            f"tensor")
        if workspace.numel() < splits * m * n:
            raise ValueError(f"workspace holds {workspace.numel()} elements; "
                             f"{splits} x {m} x {n} are needed")
        if workspace.data_ptr() % 16 != 0:
            raise ValueError("workspace must start on a 16-byte boundary")
    ws_ptr = 0
    if splits > 1:
        if c.data_ptr() % 16 != 0:
            raise ValueError("c must start on a 16-byte boundary")
        if workspace is None:
            with _on(stream):   # from the pool of the stream that uses it
                workspace = torch.empty(splits, m, n, dtype=c.dtype,
                                        device=c.device)
        ws_ptr = workspace.data_ptr()
    getattr(native(), f"gemm_splitk_{kind}_nt")(
        c.data_ptr(), a.data_ptr(), b.data_ptr(), m, n, k, splits, ws_ptr,
        _stream_handle(stream), int(xcd_swizzle))


@functools.lru_cache(maxsize=None)
def _device_cu_count(index: int) -> int:
    return torch.cuda.get_device_properties(index).multi_processor_count


def gemm_splitk_plan(m: int, n: int, k: int, n_cu: int = None) -> int:
    """The split count matmul_nt(split_k="auto") uses for an (m, n, k)
    problem: 1 when the 128^2 tiles already fill the n_cu compute units,
    else n_cu // tiles, bounded so that every split keeps enough K-tiles
    (constants and the sweep behind them: docs/gemm.md, "Split-K").
    n_cu=None reads the current device. Pure shape math otherwise."""
    if n_cu is None:
        n_cu = _device_cu_count(torch.cuda.current_device())
    return native().gemm_splitk_plan(int(m), int(n), int(k), int(n_cu))


def gemm_pad_shapes(kind: str, m: int, n: int, k: int):
    """Padded (M, N, K) that puts a (m, n, k) problem on the fast path.

    kind is "bf16" / "fp8" (8-phase needs M,N % 256, K % 128), "i8"
    (M,N % 256, K % 256), "mxfp8" (plain kernel only: M,N,K % 128) or
    "mxfp4" (the 256^2 32x32x64 kernel: M,N % 256, K % 128).
    Pure shape math — unit-tested on CPU (tests/test_gemm_skew_logic.py).
    """
    if kind not in ("bf16", "fp8", "i8", "mxfp8", "mxfp4"):
        raise ValueError(f"unknown gemm kind {kind!r}")
    def up(x, q):
        return -(-x // q) * q
    if kind == "mxfp8":
        return up(m, 128), up(n, 128), up(k, 128)
    kq = 256 if kind == "i8" else 128
    return up(m, 256), up(n, 256), up(k, kq)


def _pad2d(t: torch.Tensor, rows: int, cols: int, fill=0):
    if t.shape == (rows, cols):
        return t
    out = torch.zeros(rows, cols, dtype=t.dtype, device=t.device) if fill == 0 \
        else torch.full((rows, cols), fill, dtype=t.dtype, device=t.device)
    out[: t.shape[0], : t.shape[1]] = t
    return out


@_body_on_stream
def matmul_nt(a: torch.Tensor, b: torch.Tensor,
              a_scale: torch.Tensor = None, b_scale: torch.Tensor = None,
              stream=None, xcd_swizzle: bool = False,
              split_k=None) -> torch.Tensor:
    """Arbitrary-shape front door to the K7 GEMM family: returns A @ B^T.

    Dispatches on dtype — bf16 -> gemm_bf16, float8_e4m3fn -> gemm_fp8
    (or gemm_mxfp8 when e8m0 scales are given), int8 -> gemm_i8, uint8 +
    scales -> gemm_mxfp4 (nibble-packed e2m1; shapes in elements) — after
    zero-padding the operands up to the fast-path tile multiples
    (gemm_pad_shapes). Zero rows/columns contribute nothing, so the
    result is bit-identical to the unpadded kernel output; the padded
    region of C is sliced away (result is a fresh contiguous tensor when
    padding occurred). Scale padding uses 127 (= 2^0) — irrelevant since
    the padded data is zero.

    split_k (bf16, fp8 and int8 without scales only): None keeps the path
    above. An int runs gemm_splitk with that many splits, after padding M
    and N to 128 and K to 64 only. "auto" asks gemm_splitk_plan: small M, N
    with a long K take the split path, everything the plan answers 1 for
    keeps the path above and its 256^2 kernels.
    """
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"need A[M,K], B[N,K]; got A{tuple(a.shape)} "
                         f"B{tuple(b.shape)}")
    m, k = a.shape
    n = b.shape[0]
    if split_k is not None:
        if a_scale is not None or b_scale is not None \
                or a.dtype == torch.uint8:
            raise ValueError("split_k does not take MX operands (scales or "
                             "packed fp4): the scale rows need a staging of "
                             "their own")
        if a.dtype not in _SPLITK_KINDS:
            raise TypeError(f"unsupported operand dtype {a.dtype}")
        if split_k == "auto":
            splits = gemm_splitk_plan(m, n, k)
        elif isinstance(split_k, int) and not isinstance(split_k, bool):
            splits = split_k
        else:
            raise ValueError(f"split_k must be None, an int or 'auto'; got "
                             f"{split_k!r}")
        if split_k != "auto" or splits > 1:
            mp, np_, kp = -(-m // 128) * 128, -(-n // 128) * 128, \
                -(-k // 64) * 64
            ap = _pad2d(a.contiguous(), mp, kp)
            bp = _pad2d(b.contiguous(), np_, kp)
            c = torch.empty(mp, np_, dtype=_SPLITK_KINDS[a.dtype][1],
                            device=a.device)
            gemm_splitk(c, ap, bp, splits, stream=stream,
                        xcd_swizzle=xcd_swizzle)
            if (mp, np_) == (m, n):
                return c
            return c[:m, :n].contiguous()
    if a.dtype == torch.bfloat16:
        kind, fn, out_dtype = "bf16", gemm_bf16, torch.float32
    elif a.dtype == torch.int8:
        kind, fn, out_dtype = "i8", gemm_i8, torch.int32
    elif a.dtype == torch.float8_e4m3fn:
        if a_scale is not None:
            kind, fn, out_dtype = "mxfp8", None, torch.float32
        else:
            kind, fn, out_dtype = "fp8", gemm_fp8, torch.float32
    elif a.dtype == torch.uint8:
        # nibble-packed e2m1 (e2m1_pack layout): shapes are in ELEMENTS,
        # K = 2 * packed columns; zero nibbles pad exactly (+0.0)
        if a_scale is None:
            raise TypeError("packed-fp4 operands need e8m0 scales")
        kind, fn, out_dtype = "mxfp4", None, torch.float32
        k = 2 * k
    else:
        raise TypeError(f"unsupported operand dtype {a.dtype}")
    mp, np_, kp = gemm_pad_shapes(kind, m, n, k)
    if kind == "mxfp4":
        if b_scale is None or a_scale.shape != (m, k // 32) \
                or b_scale.shape != (n, k // 32):
            raise ValueError("mx4 path needs a_scale [M,K//32] and "
                             "b_scale [N,K//32] (K = 2*packed cols, "
                             "K % 32 == 0)")
        ap = _pad2d(a.contiguous(), mp, kp // 2)
        bp = _pad2d(b.contiguous(), np_, kp // 2)
        c = torch.empty(mp, np_, dtype=out_dtype, device=a.device)
        asp = _pad2d(a_scale.contiguous(), mp, kp // 32, fill=127)
        bsp = _pad2d(b_scale.contiguous(), np_, kp // 32, fill=127)
        gemm_mxfp4(c, ap, bp, asp, bsp, stream=stream,
                   xcd_swizzle=xcd_swizzle)
        if (mp, np_) == (m, n):
            return c
        return c[:m, :n].contiguous()
    ap = _pad2d(a.contiguous(), mp, kp)
    bp = _pad2d(b.contiguous(), np_, kp)
    c = torch.empty(mp, np_, dtype=out_dtype, device=a.device)
    if kind == "mxfp8":
        if b_scale is None or a_scale.shape != (m, k // 32) \
                or b_scale.shape != (n, k // 32):
            raise ValueError("mx path needs a_scale [M,K//32] and "
                             "b_scale [N,K//32] (K % 32 == 0)")
        asp = _pad2d(a_scale.contiguous(), mp, kp // 32, fill=127)
        bsp = _pad2d(b_scale.contiguous(), np_, kp // 32, fill=127)
        gemm_mxfp8(c, ap, bp, asp, bsp, stream=stream,
                   xcd_swizzle=xcd_swizzle)
    else:
        fn(c, ap, bp, stream=stream, xcd_swizzle=xcd_swizzle)
    if (mp, np_) == (m, n):
        return c
    return c[:m, :n].contiguous()


# ---------------------------------------------------------------------------
# MX quantize: the convert-to-MX step (OCP MX v1.0 §6.3) in front of
# gemm_mxfp8 / gemm_mxfp4. Contract: docs/gemm.md, "MX quantize".
# ---------------------------------------------------------------------------

# fmt -> (native format code, emax of the element format, largest magnitude)
_MX_FORMATS = {"mxfp8": (0, 8, 448.0), "mxfp4": (1, 2, 6.0)}

# midpoints between adjacent e2m1 magnitudes (0, .5, 1, 1.5, 2, 3, 4, 6)
_E2M1_MIDPOINTS = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def _mx_format(fmt):
    if fmt not in _MX_FORMATS:
        raise ValueError(f"unknown MX format {fmt!r}; expected one of "
                         f"{sorted(_MX_FORMATS)}")
    return _MX_FORMATS[fmt]


def _pow2_f64(exponent: torch.Tensor) -> torch.Tensor:
    """2.0 ** exponent as float64, built from the bits (exact on any
    device). exponent: integer tensor within the float64 normal range."""
    return ((exponent.to(torch.int64) + 1023) << 52).view(torch.float64)


def quantize_mx_reference(x: torch.Tensor, fmt: str):
    """Pure-torch oracle of quantize_mx, on whatever device x lives on.

    Same contract and same (q, scale) layouts, bit for bit. The scaling is
    done in float64, where v * 2^(127 - s) is exact for every fp32 v, and
    the value is clamped and rounded to the element grid (nearest, ties to
    the even code) before the final cast, so that cast is exact and no
    device's conversion rules enter the result.
    """
    _, emax, vmax = _mx_format(fmt)
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("x must be a 2-D float32 or bfloat16 tensor")
    rows, k = x.shape
    if k % 32 != 0:
        raise ValueError(f"K = {k} is not a multiple of 32")
    xf = x.float().contiguous()          # bf16 -> fp32 is exact
    field = (xf.view(torch.int32) >> 23) & 0xFF
    e = field.view(rows, k // 32, 32).amax(-1)
    scale = torch.where(e == 255, torch.full_like(e, 255),
                        (e - emax).clamp_min(0))
    v = xf.double()
    # exponent field 0 (zeros and fp32 subnormals) -> zero, sign kept
    v = torch.where(field == 0, torch.copysign(torch.zeros_like(v), v), v)
    y = v.view(rows, k // 32, 32) * _pow2_f64(127 - scale).unsqueeze(-1)
    y = y.clamp(-vmax, vmax).view(rows, k)
    if fmt == "mxfp8":
        # e4m3 grid: 3 mantissa bits, smallest normal exponent -6, below it
        # the subnormal step 2^-9. torch.round rounds half to even, and an
        # even multiple of the step is the code with the even mantissa.
        _, ex = torch.frexp(y)                      # |y| in [2^(ex-1), 2^ex)
        step = _pow2_f64((ex - 1).clamp_min(-6) - 3)
        y = torch.round(y / step) * step            # keeps the sign of zero
        q = y.float().to(torch.float8_e4m3fn)
    else:
        # midpoint bucketing; a tie goes to the code with the even index:
        # 0.25->0, 0.75->1, 1.25->1, 1.75->2, 2.5->2, 3.5->4, 5->4
        mag = y.abs()
        idx = torch.zeros_like(mag, dtype=torch.uint8)
        for i, mid in enumerate(_E2M1_MIDPOINTS):
            idx += ((mag > mid) if i % 2 == 0 else (mag >= mid)).to(torch.uint8)
        nib = idx | (torch.signbit(y).to(torch.uint8) << 3)
        q = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    return q, scale.to(torch.uint8)


def dequantize_mx(q: torch.Tensor, scale: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 value of an MX tensor: element * 2^(scale - 127) per 32-block
    along K; a block whose scale byte is 255 (e8m0 NaN) is all NaN.
    Reference only — pure torch."""
    _mx_format(fmt)
    v = q.float().double() if fmt == "mxfp8" else e2m1_decode(q).double()
    rows, k = v.shape
    if scale.shape != (rows, k // 32) or scale.dtype != torch.uint8:
        raise ValueError("scale must be uint8 [rows, K//32]")
    s = scale.to(torch.int64)
    factor = torch.where(s == 255, torch.full_like(s, 0, dtype=torch.float64)
                         + float("nan"), _pow2_f64(s - 127))
    return (v.view(rows, k // 32, 32) * factor.unsqueeze(-1)).view(rows, k)


@_body_on_stream
def quantize_mx(x: torch.Tensor, fmt: str, stream=None):
    """Convert-to-MX on the GPU (native/quant.hip): fp32 or bf16 [rows, K]
    -> (q, scale), exactly the operands gemm_mxfp8 / gemm_mxfp4 take.

    One e8m0 scale byte per 32 consecutive elements along K, scale =
    max(largest exponent field of the block - emax, 0) (255 if the block
    holds an Inf or NaN); elements scaled by 2^(127 - scale), saturated to
    +-448 / +-6 and rounded to nearest-even. "mxfp8": q is float8_e4m3fn
    [rows, K]; "mxfp4": q is uint8 [rows, K//2], low nibble = even k (the
    e2m1_pack layout). scale is uint8 [rows, K//32]. Full contract:
    docs/gemm.md. K must be a multiple of 32 (matmul_mx pads). The element
    codes of a scale-255 block are unspecified; the MX GEMMs read such a
    block as all NaN whatever they are (findings.md #31).
    """
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError("x must be a CUDA tensor")
    if x.dim() != 2 or not x.is_contiguous():
        raise TypeError("x must be a contiguous 2-D tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"x must be float32 or bfloat16, got {x.dtype}")
    code, _, _ = _mx_format(fmt)
    rows, k = x.shape
    if rows < 1 or k < 32 or k % 32 != 0:
        raise ValueError(f"need rows >= 1 and K a positive multiple of 32; "
                         f"got {tuple(x.shape)}")
    if x.data_ptr() % 16 != 0:
        raise ValueError("x must start on a 16-byte boundary (the kernel "
                         "reads it with 16-byte loads)")
    if fmt == "mxfp8":
        q = torch.empty(rows, k, dtype=torch.float8_e4m3fn, device=x.device)
    else:
        q = torch.empty(rows, k // 2, dtype=torch.uint8, device=x.device)
    scale = torch.empty(rows, k // 32, dtype=torch.uint8, device=x.device)
    native().quantize_mx(q.data_ptr(), scale.data_ptr(), x.data_ptr(),
                         int(x.dtype == torch.bfloat16), code, rows, k,
                         _stream_handle(stream))
    return q, scale


@_body_on_stream
def matmul_mx(a: torch.Tensor, b: torch.Tensor, fmt: str = "mxfp8",
              stream=None) -> torch.Tensor:
    """A @ B^T through the MX GEMMs from real tensors: a [M,K], b [N,K],
    fp32 or bf16, any M, N, K; returns fp32 [M,N].

    K is zero-padded up to a multiple of 32 (zeros change no block
    maximum), both operands go through quantize_mx, and matmul_nt does
    the tile padding and picks the kernel.

    An Inf or NaN in a makes row i of the result NaN, one in b column j
    (its block gets scale byte 255, which the scaled MFMAs read as NaN);
    every other output is unaffected (tests/test_gpu_gemm_specials.py).
    """
    _mx_format(fmt)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"need A[M,K], B[N,K]; got A{tuple(a.shape)} "
                         f"B{tuple(b.shape)}")
    k = a.shape[1]
    kp = -(-k // 32) * 32
    def operand(t):
        t = _pad2d(t.contiguous(), t.shape[0], kp)
        # a contiguous view may start off a 16-byte boundary; a copy does not
        return t if t.data_ptr() % 16 == 0 else t.clone()

    aq, a_scale = quantize_mx(operand(a), fmt, stream=stream)
    bq, b_scale = quantize_mx(operand(b), fmt, stream=stream)
    return matmul_nt(aq, bq, a_scale, b_scale, stream=stream)


# ---------------------------------------------------------------------------
# Operand layouts: bf16 products whose operands are not K-contiguous
# (native/gemm_layout.hip). Contract: docs/gemm.md, "Operand layouts".
# ---------------------------------------------------------------------------

# layout -> (A is stored [K,M], B is stored [K,N]); row-major names, transA
# then transB. "nt" is the rest of the family.
_LAYOUTS = {"nn": (False, True), "tn": (True, True), "tt": (True, False)}

_NO_NARROW_TR = ("only bf16 has the nn/tn/tt layouts: the 8-bit and 4-bit "
                 "transposed LDS reads (ds_read_b64_tr_b8 / _tr_b4) are not "
                 "built here; pass K-contiguous operands (layout nt)")


def gemm_bf16_layout(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                     layout: str, stream=None,
                     xcd_swizzle: bool = False) -> None:
    """K7 layouts: C[M,N] fp32 = op(A) @ op(B) on bf16 operands AS STORED.

        layout  a        b
        "nn"    [M,K]    [K,N]
        "tn"    [K,M]    [K,N]
        "tt"    [K,M]    [N,K]
        "nt"    [M,K]    [N,K]   (forwards to gemm_bf16)

    An operand stored [K, X] is staged by the family's 16-byte DMAs along
    its contiguous dimension and transposed on the way out of LDS by
    ds_read_b64_tr_b16 — no transposed copy in HBM. The result is bit for
    bit what gemm_bf16's double-buffered 128^2 kernel (HPK_GEMM_VARIANT=db)
    gives on t().contiguous() copies. Requires M,N % 128 == 0, K % 64 == 0
    and a, b starting on 16-byte boundaries (matmul pads). Any other layout
    string raises ValueError.
    """
    if layout == "nt":
        return gemm_bf16(c, a, b, stream=stream, xcd_swizzle=xcd_swizzle)
    if layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected one of "
                         f"'nn', 'tn', 'tt', 'nt'")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError(_NO_NARROW_TR)
        raise TypeError("c must be fp32; a, b must be bf16")
    if c.dtype != torch.float32:
        raise TypeError("c must be fp32; a, b must be bf16")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    a_t, b_n = _LAYOUTS[layout]
    k, m = a.shape if a_t else a.shape[::-1]
    kb, n = b.shape if b_n else b.shape[::-1]
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch for layout {layout}: "
                         f"A{tuple(a.shape)} B{tuple(b.shape)} "
                         f"C{tuple(c.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_bf16_layout requires M,N % 128 == 0 and "
                         f"K % 64 == 0; got M={m} N={n} K={k}")
    if a.data_ptr() % 16 != 0 or b.data_ptr() % 16 != 0:
        raise ValueError("a and b must start on 16-byte boundaries (they "
                         "are fetched in 16-byte chunks)")
    native().gemm_bf16_layout(c.data_ptr(), a.data_ptr(), b.data_ptr(),
                              m, n, k, layout, _stream_handle(stream),
                              int(xcd_swizzle))


def gemm_bf16_layout_splitk(c: torch.Tensor, a: torch.Tensor,
                            b: torch.Tensor, layout: str, splits: int,
                            workspace: torch.Tensor = None, stream=None,
                            xcd_swizzle: bool = False) -> None:
    """K7 layouts, split-K: gemm_bf16_layout with the K loop cut into
    `splits` parts that run as separate workgroups
    (native/gemm_layout_splitk.hip) — for the dW product of a linear layer,
    dW[N,K] = dy[M,N]^T @ x[M,K] (layout "tn" on the tensors as stored),
    whose output is a weight and whose sum runs over the tokens.

    Operands, layouts and their rules are gemm_bf16_layout's; splits,
    workspace and the fold are gemm_splitk's: split s of S walks
    T/S + (s < T%S) consecutive K-tiles of 64 (T = K/64) — rows of an
    operand stored [K, X] — and writes its partial to workspace[s]; a
    second kernel on the same stream computes C = ((P0 + P1) + P2) + ... in
    ascending s. splits == 1 writes C directly and gives gemm_bf16_layout's
    bits; every splits gives the bits of gemm_splitk on t().contiguous()
    copies. Requires M,N % 128 == 0, K % 64 == 0, 1 <= splits <= K/64
    (matmul pads). layout "nt" forwards to gemm_splitk.

    workspace: None allocates [splits, M, N] fp32; a caller's must be a
    contiguous fp32 CUDA tensor with at least splits*M*N elements, starting
    on a 16-byte boundary. It is scratch: its first splits*M*N elements are
    overwritten, the rest is not touched.
    """
    if layout == "nt":
        return gemm_splitk(c, a, b, splits, workspace=workspace,
                           stream=stream, xcd_swizzle=xcd_swizzle)
    if layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected one of "
                         f"'nn', 'tn', 'tt', 'nt'")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError(_NO_NARROW_TR)
        raise TypeError("c must be fp32; a, b must be bf16")
    if c.dtype != torch.float32:
        raise TypeError("c must be fp32; a, b must be bf16")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    a_t, b_n = _LAYOUTS[layout]
    k, m = a.shape if a_t else a.shape[::-1]
    kb, n = b.shape if b_n else b.shape[::-1]
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch for layout {layout}: "
                         f"A{tuple(a.shape)} B{tuple(b.shape)} "
                         f"C{tuple(c.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_bf16_layout_splitk requires M,N % 128 == 0 "
                         f"and K % 64 == 0; got M={m} N={n} K={k}")
    if a.data_ptr() % 16 != 0 or b.data_ptr() % 16 != 0:
        raise ValueError("a and b must start on 16-byte boundaries (they "
                         "are fetched in 16-byte chunks)")
    splits = int(splits)
    if not 1 <= splits <= k // 64:
        raise ValueError(f"need 1 <= splits <= K/64 = {k // 64}; got {splits}")
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda \
                or not workspace.is_contiguous() \
                or workspace.dtype != c.dtype:
            raise TypeError(f"workspace must be a contiguous {c.dtype} CUDA "
                            f"tensor")
        if workspace.numel() < splits * m * n:
            raise ValueError(f"workspace holds {workspace.numel()} elements; "
                             f"{splits} x {m} x {n} are needed")
        if workspace.data_ptr() % 16 != 0:
            raise ValueError("workspace must start on a 16-byte boundary")
    ws_ptr = 0
    if splits > 1:
        if c.data_ptr() % 16 != 0:
            raise ValueError("c must start on a 16-byte boundary")
        if workspace is None:
            with _on(stream):   # from the pool of the stream that uses it
                workspace = torch.empty(splits, m, n, dtype=c.dtype,
                                        device=c.device)
        ws_ptr = workspace.data_ptr()
    native().gemm_bf16_layout_splitk(
        c.data_ptr(), a.data_ptr(), b.data_ptr(), m, n, k, layout, splits,
        ws_ptr, _stream_handle(stream), int(xcd_swizzle))


def matmul_layout(a: torch.Tensor, b: torch.Tensor):
    """(layout, a_stored, b_stored) of the logical product a [M,K] @ b [K,N],
    read from the strides; pure tensor metadata, any device.

    Each argument is row-major contiguous or the .t() view of a row-major
    contiguous tensor; a_stored / b_stored are those contiguous tensors
    (views, never copies). a row-major is "n", its .t() view "t"; b
    row-major [K,N] is "n", the .t() view of a stored [N,K] is "t".
    is_contiguous() is asked first, so a tensor with a size-1 dimension —
    whose strides fit both readings, the memory being the same — counts as
    row-major. Anything else raises TypeError.
    """
    def stored(t, name):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f"{name} must be a 2-D tensor")
        if t.is_contiguous():
            return t, "n"
        if t.t().is_contiguous():
            return t.t(), "t"
        raise TypeError(f"{name} is neither row-major contiguous nor the "
                        f".t() view of such a tensor (shape "
                        f"{tuple(t.shape)}, strides {t.stride()}); "
                        f"matmul makes no hidden copies")
    a_st, fa = stored(a, "a")
    b_st, fb = stored(b, "b")
    if a.shape[1] != b.shape[0]:
        raise ValueError(f"need a[M,K] @ b[K,N]; got a{tuple(a.shape)} "
                         f"b{tuple(b.shape)}")
    return fa + fb, a_st, b_st


def gemm_layout_pad_shapes(m: int, n: int, k: int):
    """Padded (M, N, K) of the nn/tn/tt kernels: M, N up to 128, K to 64."""
    return -(-m // 128) * 128, -(-n // 128) * 128, -(-k // 64) * 64


def _check_split_k(split_k, ints: bool):
    """split_k of matmul (ints) / linear_bf16 (no ints), on its type and
    value alone: before any tensor is looked at"""
    if split_k is None or (isinstance(split_k, str) and split_k == "auto"):
        return
    if ints and isinstance(split_k, int) and not isinstance(split_k, bool):
        return
    raise ValueError(f"split_k must be None{', an int' if ints else ''} or "
                     f"'auto'; got {split_k!r}")


def _check_out_dtype_bias(out_dtype, bias):
    """out_dtype and bias of matmul, on their type and value alone: before
    any tensor is looked at"""
    if out_dtype is not None and out_dtype is not torch.bfloat16:
        raise ValueError(f"out_dtype must be None or torch.bfloat16; got "
                         f"{out_dtype!r}")
    if bias is not None and not isinstance(bias, torch.Tensor):
        raise TypeError(f"bias must be None or a tensor; got "
                        f"{type(bias).__name__}")
    if bias is not None and out_dtype is None:
        raise ValueError("bias needs out_dtype=torch.bfloat16: an fp32 output "
                         "with a bias is not built")


def _bias_f32(bias, n: int, n_padded: int, device):
    """bias [n] (bf16 or fp32) -> contiguous fp32 [n_padded], zero-padded;
    bf16 -> fp32 is exact"""
    if bias.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"bias must be bfloat16 or float32, got {bias.dtype}")
    if bias.dim() != 1 or bias.shape[0] != n:
        raise ValueError(f"bias must have shape ({n},); got "
                         f"{tuple(bias.shape)}")
    if bias.device != device:
        raise TypeError(f"bias is on {bias.device}, the operands on {device}")
    bias = bias.float().contiguous()
    if n_padded == n:
        return bias
    out = torch.zeros(n_padded, dtype=torch.float32, device=device)
    out[:n] = bias
    return out


def gemm_bf16_epilogue(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                       layout: str = "nt", bias: torch.Tensor = None,
                       splits: int = 1, workspace: torch.Tensor = None,
                       stream=None, xcd_swizzle: bool = False) -> None:
    """K7 with a bf16 output: C[M,N] bf16 = bf16(op(A) @ op(B) + bias[n]),
    written by the GEMM kernel itself (native/gemm_epilogue.hip) — no fp32 C
    in HBM and no elementwise pass behind it.

        layout  a        b
        "nt"    [M,K]    [N,K]
        "nn"    [M,K]    [K,N]
        "tn"    [K,M]    [K,N]
        "tt"    [K,M]    [N,K]

    The products are those of the double-buffered 128^2 kernels
    (gemm_bf16 under HPK_GEMM_VARIANT=db, gemm_bf16_layout): the result is
    (c32 + bias).to(bfloat16) of their fp32 C bit for bit — one fp32 add,
    one round-to-nearest-even conversion, the bias never rounded first.
    bias is fp32 [N], contiguous, on c's device; None adds nothing at all.
    splits > 1 runs the split-K tile kernels of gemm_splitk /
    gemm_bf16_layout_splitk into workspace ([splits, M, N] fp32; None
    allocates) and one fold kernel that sums the partials in ascending s,
    adds the bias and converts. Requires M,N % 128 == 0, K % 64 == 0,
    1 <= splits <= K/64 and a, b, c on 16-byte boundaries (matmul pads).
    """
    if layout != "nt" and layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected one of "
                         f"'nn', 'tn', 'tt', 'nt'")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError("only bf16 operands have a bf16 output: fp8, "
                            "int8 and MX outputs are not built")
        raise TypeError("c, a and b must be bf16")
    if c.dtype != torch.bfloat16:
        raise TypeError("c, a and b must be bf16")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    a_t, b_n = _LAYOUTS.get(layout, (False, False))
    k, m = a.shape if a_t else a.shape[::-1]
    kb, n = b.shape if b_n else b.shape[::-1]
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch for layout {layout}: "
                         f"A{tuple(a.shape)} B{tuple(b.shape)} "
                         f"C{tuple(c.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_bf16_epilogue requires M,N % 128 == 0 and "
                         f"K % 64 == 0; got M={m} N={n} K={k}")
    for t, name in ((a, "a"), (b, "b"), (c, "c")):
        if t.data_ptr() % 16 != 0:
            raise ValueError(f"{name} must start on a 16-byte boundary")
    bias_ptr = 0
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 \
                or not bias.is_contiguous() or bias.device != c.device:
            raise TypeError("bias must be a contiguous float32 tensor on c's "
                            "device")
        if bias.dim() != 1 or bias.shape[0] != n:
            raise ValueError(f"bias must have shape ({n},); got "
                             f"{tuple(bias.shape)}")
        bias_ptr = bias.data_ptr()
    splits = int(splits)
    if not 1 <= splits <= k // 64:
        raise ValueError(f"need 1 <= splits <= K/64 = {k // 64}; got {splits}")
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda \
                or not workspace.is_contiguous() \
                or workspace.dtype != torch.float32:
            raise TypeError("workspace must be a contiguous float32 CUDA "
                            "tensor")
        if workspace.numel() < splits * m * n:
            raise ValueError(f"workspace holds {workspace.numel()} elements; "
                             f"{splits} x {m} x {n} are needed")
        if workspace.data_ptr() % 16 != 0:
            raise ValueError("workspace must start on a 16-byte boundary")
    ws_ptr = 0
    if splits > 1:
        if workspace is None:
            with _on(stream):   # from the pool of the stream that uses it
                workspace = torch.empty(splits, m, n, dtype=torch.float32,
                                        device=c.device)
        ws_ptr = workspace.data_ptr()
    native().gemm_bf16_epilogue(
        c.data_ptr(), a.data_ptr(), b.data_ptr(), bias_ptr, m, n, k, layout,
        splits, ws_ptr, _stream_handle(stream), int(xcd_swizzle))


def colsum_plan(m: int, n: int, n_cu: int = None) -> int:
    """Row chunks colsum_bf16 cuts an [m, n] input into: enough 64-thread
    workgroups (one thread per 8 columns) for COLSUM waves on every compute
    unit, at least 32 rows per chunk, at most 256 chunks (docs/gemm.md,
    "bf16 output and bias"). n_cu=None reads the current device."""
    if n_cu is None:
        n_cu = _device_cu_count(torch.cuda.current_device())
    return native().colsum_plan(int(m), int(n), int(n_cu))


@_body_on_stream
def colsum_bf16(x: torch.Tensor, out: torch.Tensor = None,
                stream=None) -> torch.Tensor:
    """out[n] = sum_m x[m, n] in fp32 for a bf16 [M, N] contiguous CUDA
    tensor (native/gemm_epilogue.hip): the bias gradient of linear_bf16.

    The rows are cut into colsum_plan(M, N) chunks; chunk r sums its rows
    in ascending order in fp32, and the chunk sums are folded in ascending
    r (the split-K fold kernel), so the result is the same bits on every
    run for the same shape on the same device. N is zero-padded to a
    multiple of 8 (a copy) when it is not one. out: None allocates; a
    caller's must be a contiguous fp32 CUDA tensor of shape (N,). Returns
    the sums, shape (N,).
    """
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise TypeError("x must be a CUDA tensor")
    if x.dtype != torch.bfloat16 or x.dim() != 2 or not x.is_contiguous():
        raise TypeError("x must be a contiguous 2-D bfloat16 tensor")
    m, n = x.shape
    if m < 1 or n < 1:
        raise ValueError(f"need M >= 1 and N >= 1; got {tuple(x.shape)}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or not out.is_cuda \
                or out.dtype != torch.float32 or not out.is_contiguous():
            raise TypeError("out must be a contiguous float32 CUDA tensor")
        if out.shape != (n,):
            raise ValueError(f"out must have shape ({n},); got "
                             f"{tuple(out.shape)}")
    n8 = -(-n // 8) * 8
    xp = _pad2d(x, m, n8)
    if xp.data_ptr() % 16 != 0:
        xp = xp.clone()
    chunks = colsum_plan(m, n8)
    lib = native()
    pitch = lib.colsum_pitch(n8)
    # the kernel writes n8 sums, the fold of chunks > 1 a whole pitch
    width = n8 if chunks == 1 else pitch
    direct = out is not None and width == n and out.data_ptr() % 16 == 0
    buf = torch.empty(width * (0 if direct else 1)
                      + (pitch * chunks if chunks > 1 else 0),
                      dtype=torch.float32, device=x.device)
    res = out if direct else buf[:width]
    ws_ptr = buf[0 if direct else width:].data_ptr() if chunks > 1 else 0
    lib.colsum_bf16(res.data_ptr(), xp.data_ptr(), m, n8, chunks, ws_ptr,
                    _stream_handle(stream))
    if direct:
        return out
    if out is not None:
        out.copy_(buf[:n])
        return out
    return buf[:n]


ACTIVATIONS = ("relu", "gelu")
_SQRT_2_OVER_PI = 0.7978845608028654


def _check_activation_name(act, what: str):
    if not isinstance(act, str) or act not in ACTIVATIONS:
        raise ValueError(f"{what} must be one of {ACTIVATIONS} (gelu is the "
                         f"tanh form; the erf form is not built); got "
                         f"{act!r}")


def _gelu_sigmoids(z: torch.Tensor):
    """(s, 1 - s) of the tanh GELU in float64: s = 1 / (1 + exp(-2u)),
    u = sqrt(2/pi) (z + 0.044715 z^3); 1 - s as 1 / (1 + exp(2u)), which
    does not cancel"""
    u2 = 2.0 * _SQRT_2_OVER_PI * (z + 0.044715 * z * z * z)
    return 1.0 / (1.0 + torch.exp(-u2)), 1.0 / (1.0 + torch.exp(u2))


def activation_reference(z: torch.Tensor, act: str) -> torch.Tensor:
    """act(z) in float64, pure torch, any device: the reference of the
    activation epilogues. relu: z where z > 0, NaN where z is NaN, else 0.
    gelu: z * s with s = 1 / (1 + exp(-2u)), u = sqrt(2/pi) (z + 0.044715
    z^3) — torch.nn.functional.gelu(approximate="tanh") in its sigmoid form,
    special values included (gelu(-Inf) is NaN there too)."""
    _check_activation_name(act, "act")
    z = z.double()
    if act == "relu":
        return torch.where(z > 0, z, torch.where(torch.isnan(z), z,
                                                 torch.zeros_like(z)))
    return z * _gelu_sigmoids(z)[0]


def activation_grad_terms(z: torch.Tensor, act: str):
    """(first, second) with act'(z) = first + second, float64: gelu' =
    s + z s (1 - s) 2 sqrt(2/pi) (1 + 0.134145 z^2); relu' = (z > 0) + 0.
    |first| + |second| is the T of the acceptance rule (docs/gemm.md)."""
    _check_activation_name(act, "act")
    z = z.double()
    if act == "relu":
        return (z > 0).double(), torch.zeros_like(z)
    s, sc = _gelu_sigmoids(z)
    return s, z * s * sc * (2.0 * _SQRT_2_OVER_PI) * (1.0 + 0.134145 * z * z)


def activation_grad_reference(z: torch.Tensor, act: str) -> torch.Tensor:
    """act'(z) in float64, pure torch, any device (activation_grad_terms
    summed)."""
    first, second = activation_grad_terms(z, act)
    return first + second


def gemm_bf16_act(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                  layout: str = "nt", activation: str = None,
                  bias: torch.Tensor = None, aux_out: torch.Tensor = None,
                  grad_aux: torch.Tensor = None, splits: int = 1,
                  workspace: torch.Tensor = None, stream=None,
                  xcd_swizzle: bool = False) -> None:
    """K7 with an activation epilogue (native/gemm_act.hip), layouts and
    shapes as gemm_bf16_epilogue. activation is "relu" or "gelu" (the tanh
    form; the erf form is not built).

    Forward (grad_aux is None): with z = op(A) @ op(B) + bias[n] in fp32,
    c = bf16(act(z)); aux_out, a bf16 [M,N] tensor, also receives bf16(z) —
    the bits gemm_bf16_epilogue writes — which is what the gelu backward
    needs; relu needs none, its output carries the mask.

    Gradient (grad_aux given): c = bf16((op(A) @ op(B)) * act'(grad_aux)),
    grad_aux a bf16 [M,N] tensor: the forward's z for gelu, its output or z
    for relu. One fp32 multiply before the one rounding. bias and aux_out
    must be None.

    relu is exact; gelu is within the relative error derived in
    docs/gemm.md, "Activations". splits, workspace, stream, xcd_swizzle: as
    gemm_bf16_epilogue.
    """
    _check_activation_name(activation, "activation")
    grad = grad_aux is not None
    if grad and (bias is not None or aux_out is not None):
        raise ValueError("grad_aux chooses the gradient mode, which takes "
                         "neither bias nor aux_out")
    if layout != "nt" and layout not in _LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected one of "
                         f"'nn', 'tn', 'tt', 'nt'")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 \
            or c.dtype != torch.bfloat16:
        raise TypeError("c, a and b must be bf16")
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError(f"{name} must be a contiguous 2-D CUDA tensor")
    a_t, b_n = _LAYOUTS.get(layout, (False, False))
    k, m = a.shape if a_t else a.shape[::-1]
    kb, n = b.shape if b_n else b.shape[::-1]
    if kb != k or c.shape != (m, n):
        raise ValueError(f"shape mismatch for layout {layout}: "
                         f"A{tuple(a.shape)} B{tuple(b.shape)} "
                         f"C{tuple(c.shape)}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_bf16_act requires M,N % 128 == 0 and "
                         f"K % 64 == 0; got M={m} N={n} K={k}")
    for t, name in ((a, "a"), (b, "b"), (c, "c")):
        if t.data_ptr() % 16 != 0:
            raise ValueError(f"{name} must start on a 16-byte boundary")
    aux = grad_aux if grad else aux_out
    aux_ptr = 0
    if aux is not None:
        name = "grad_aux" if grad else "aux_out"
        if not isinstance(aux, torch.Tensor) or aux.dtype != torch.bfloat16 \
                or not aux.is_contiguous() or aux.device != c.device:
            raise TypeError(f"{name} must be a contiguous bfloat16 tensor on "
                            f"c's device")
        if aux.shape != (m, n):
            raise ValueError(f"{name} must have shape ({m}, {n}); got "
                             f"{tuple(aux.shape)}")
        if aux.data_ptr() % 16 != 0:
            raise ValueError(f"{name} must start on a 16-byte boundary")
        if aux.data_ptr() == c.data_ptr():
            raise ValueError(f"{name} and c must not be the same memory")
        aux_ptr = aux.data_ptr()
    bias_ptr = 0
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 \
                or not bias.is_contiguous() or bias.device != c.device:
            raise TypeError("bias must be a contiguous float32 tensor on c's "
                            "device")
        if bias.dim() != 1 or bias.shape[0] != n:
            raise ValueError(f"bias must have shape ({n},); got "
                             f"{tuple(bias.shape)}")
        bias_ptr = bias.data_ptr()
    splits = int(splits)
    if not 1 <= splits <= k // 64:
        raise ValueError(f"need 1 <= splits <= K/64 = {k // 64}; got {splits}")
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda \
                or not workspace.is_contiguous() \
                or workspace.dtype != torch.float32:
            raise TypeError("workspace must be a contiguous float32 CUDA "
                            "tensor")
        if workspace.numel() < splits * m * n:
            raise ValueError(f"workspace holds {workspace.numel()} elements; "
                             f"{splits} x {m} x {n} are needed")
        if workspace.data_ptr() % 16 != 0:
            raise ValueError("workspace must start on a 16-byte boundary")
    ws_ptr = 0
    if splits > 1:
        if workspace is None:
            with _on(stream):   # from the pool of the stream that uses it
                workspace = torch.empty(splits, m, n, dtype=torch.float32,
                                        device=c.device)
        ws_ptr = workspace.data_ptr()
    lib = native()
    lib.gemm_bf16_act(
        c.data_ptr(), aux_ptr, a.data_ptr(), b.data_ptr(), bias_ptr, m, n, k,
        layout, lib.ACT_RELU if activation == "relu" else lib.ACT_GELU,
        lib.ACT_GRAD if grad else lib.ACT_FORWARD, splits, ws_ptr,
        _stream_handle(stream), int(xcd_swizzle))


def _check_activation_keywords(activation, return_aux, activation_grad,
                               out_dtype, bias):
    """activation, return_aux and activation_grad of matmul, on their type
    and value alone: before any tensor is looked at"""
    if activation is not None:
        _check_activation_name(activation, "activation")
    if not isinstance(return_aux, bool):
        raise ValueError(f"return_aux must be True or False; got "
                         f"{return_aux!r}")
    if activation_grad is not None:
        if not isinstance(activation_grad, tuple) or len(activation_grad) != 2:
            raise ValueError("activation_grad must be None or a tuple (name, "
                             "aux)")
        _check_activation_name(activation_grad[0], "activation_grad's name")
        if not isinstance(activation_grad[1], torch.Tensor):
            raise TypeError(f"activation_grad's aux must be a tensor; got "
                            f"{type(activation_grad[1]).__name__}")
    if activation is not None and activation_grad is not None:
        raise ValueError("activation and activation_grad exclude each other: "
                         "one call has one epilogue")
    if return_aux and activation is None:
        raise ValueError("return_aux needs an activation")
    if (activation is not None or activation_grad is not None) \
            and out_dtype is not torch.bfloat16:
        raise ValueError("activation and activation_grad need "
                         "out_dtype=torch.bfloat16")
    if activation_grad is not None and bias is not None:
        raise ValueError("activation_grad takes no bias")


@_body_on_stream
def matmul(a: torch.Tensor, b: torch.Tensor, stream=None,
           xcd_swizzle: bool = False, split_k=None, out_dtype=None,
           bias: torch.Tensor = None, activation=None,
           return_aux: bool = False, activation_grad=None) -> torch.Tensor:
    """Layout-agnostic front door: returns the logical a [M,K] @ b [K,N].

    The layout is read from the strides (matmul_layout: row-major or a
    .t() view; no hidden .contiguous() copies, anything else is a
    TypeError). nt — b the .t() view of a stored [N,K] — goes to matmul_nt
    in every dtype it takes without scales. nn, tn and tt are bf16 only:
    the stored tensors are zero-padded to multiples of 128 / 128 / 64
    (zeros add nothing, so the result is the unpadded product bit for bit)
    and run through gemm_bf16_layout; other dtypes raise TypeError. A stored
    tensor that needs no padding but starts off a 16-byte boundary is
    cloned. This change does not switch kernels on size: at large shapes a
    t().contiguous() copy plus the 256^2 kernel of matmul_nt can be faster
    (docs/gemm.md, "Operand layouts").

    split_k: None keeps the path above. It is checked first — None, an int
    or "auto", anything else is a ValueError — and nt hands it to matmul_nt.
    For nn, tn and tt an int runs gemm_bf16_layout_splitk with that many
    splits on the same padded tensors (1 <= split_k <= K_padded / 64, else
    ValueError); "auto" asks gemm_splitk_plan(m, n, k): a small output with
    a long sum — dW = dy^T x over many tokens — takes the split path,
    everything the plan answers 1 for keeps the path above.

    out_dtype=torch.bfloat16 (bf16 operands only) returns bf16, rounded once
    from the fp32 accumulators by the GEMM kernel itself, in all four
    layouts, nt included: gemm_bf16_epilogue on the tensors padded as
    above, i.e. the double-buffered 128^2 kernels, not matmul_nt's 256^2
    one. bias ([N], bf16 or fp32; a bf16 one is widened, which is exact) is
    added in fp32 before that one rounding; it is zero-padded with N. A
    bias without out_dtype=torch.bfloat16 is a ValueError. split_k works as
    above; a plan of 1 takes the kernel without a split. out_dtype and bias
    are checked with split_k, before any tensor.

    activation="relu" | "gelu" (tanh form; needs out_dtype=torch.bfloat16)
    applies the activation in the same epilogue: bf16(act(a @ b + bias)),
    gemm_bf16_act. return_aux=True then returns (y, z), z the bf16
    pre-activation the GEMM wrote beside y. activation_grad=(name, aux), aux
    a bf16 [M,N] tensor, returns bf16((a @ b) * act'(aux)) — the backward of
    the activation folded into the product that forms its incoming gradient;
    it takes no bias and excludes activation. aux is zero-padded with the
    output; the padded accumulators are 0, so the cropped result does not
    change. The three keywords are judged with the ones above, before any
    tensor; without them this function runs what it ran before them.
    """
    _check_split_k(split_k, ints=True)
    _check_out_dtype_bias(out_dtype, bias)
    _check_activation_keywords(activation, return_aux, activation_grad,
                               out_dtype, bias)
    layout, a_st, b_st = matmul_layout(a, b)
    if a.dtype != b.dtype:
        raise TypeError(f"a is {a.dtype}, b is {b.dtype}")
    if out_dtype is not None:
        if a.dtype != torch.bfloat16:
            raise TypeError(f"out_dtype=torch.bfloat16 takes bf16 operands; "
                            f"got {a.dtype}")
        m, k = a.shape
        n = b.shape[1]
        mp, np_, kp = gemm_layout_pad_shapes(m, n, k)
        a_t, b_n = _LAYOUTS.get(layout, (False, False))
        splits = 1
        if split_k == "auto":
            splits = gemm_splitk_plan(m, n, k)
        elif split_k is not None:
            if not 1 <= split_k <= kp // 64:
                raise ValueError(f"need 1 <= split_k <= K_padded/64 = "
                                 f"{kp // 64} (K = {k} padded to {kp}); got "
                                 f"{split_k}")
            splits = split_k
        bias_p = None if bias is None else _bias_f32(bias, n, np_, a.device)

        def operand(t, rows, cols):
            t = _pad2d(t, rows, cols)
            return t if t.data_ptr() % 16 == 0 else t.clone()

        ap = operand(a_st, *((kp, mp) if a_t else (mp, kp)))
        bp = operand(b_st, *((kp, np_) if b_n else (np_, kp)))
        c = torch.empty(mp, np_, dtype=torch.bfloat16, device=a.device)
        if activation is None and activation_grad is None:
            gemm_bf16_epilogue(c, ap, bp, layout, bias=bias_p, splits=splits,
                               stream=stream, xcd_swizzle=xcd_swizzle)
            if (mp, np_) == (m, n):
                return c
            return c[:m, :n].contiguous()

        def crop(t):
            return t if (mp, np_) == (m, n) else t[:m, :n].contiguous()

        if activation_grad is not None:
            name, aux = activation_grad
            if aux.dtype != torch.bfloat16 or aux.dim() != 2 \
                    or not aux.is_contiguous():
                raise TypeError("activation_grad's aux must be a contiguous "
                                "2-D bfloat16 tensor")
            if aux.shape != (m, n):
                raise ValueError(f"activation_grad's aux must have shape "
                                 f"({m}, {n}); got {tuple(aux.shape)}")
            if aux.device != a.device:
                raise TypeError(f"activation_grad's aux is on {aux.device}, "
                                f"the operands on {a.device}")
            gemm_bf16_act(c, ap, bp, layout, activation=name,
                          grad_aux=operand(aux, mp, np_), splits=splits,
                          stream=stream, xcd_swizzle=xcd_swizzle)
            return crop(c)
        z = None
        if return_aux:
            z = torch.empty(mp, np_, dtype=torch.bfloat16, device=a.device)
        gemm_bf16_act(c, ap, bp, layout, activation=activation, bias=bias_p,
                      aux_out=z, splits=splits, stream=stream,
                      xcd_swizzle=xcd_swizzle)
        return (crop(c), crop(z)) if return_aux else crop(c)
    if layout == "nt":
        return matmul_nt(a_st, b_st, stream=stream, xcd_swizzle=xcd_swizzle,
                         split_k=split_k)
    if a.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError(_NO_NARROW_TR)
        raise TypeError(f"unsupported operand dtype {a.dtype}")
    m, k = a.shape
    n = b.shape[1]
    mp, np_, kp = gemm_layout_pad_shapes(m, n, k)
    a_t, b_n = _LAYOUTS[layout]
    splits = None  # None: the kernel without a split
    if split_k == "auto":
        plan = gemm_splitk_plan(m, n, k)
        splits = plan if plan > 1 else None
    elif split_k is not None:
        if not 1 <= split_k <= kp // 64:
            raise ValueError(f"need 1 <= split_k <= K_padded/64 = {kp // 64} "
                             f"(K = {k} padded to {kp}); got {split_k}")
        splits = split_k

    def operand(t, rows, cols):
        t = _pad2d(t, rows, cols)
        return t if t.data_ptr() % 16 == 0 else t.clone()

    ap = operand(a_st, *((kp, mp) if a_t else (mp, kp)))
    bp = operand(b_st, *((kp, np_) if b_n else (np_, kp)))
    c = torch.empty(mp, np_, dtype=torch.float32, device=a.device)
    if splits is None:
        gemm_bf16_layout(c, ap, bp, layout, stream=stream,
                         xcd_swizzle=xcd_swizzle)
    else:
        gemm_bf16_layout_splitk(c, ap, bp, layout, splits, stream=stream,
                                xcd_swizzle=xcd_swizzle)
    if (mp, np_) == (m, n):
        return c
    return c[:m, :n].contiguous()


class _LinearBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, split_k):
        ctx.save_for_backward(x, w)
        ctx.split_k = split_k
        return matmul_nt(x, w, split_k=split_k).to(torch.bfloat16)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        sk = ctx.split_k
        if not dy.is_contiguous():  # e.g. the expanded scalar of sum()
            dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:     # nn: dy [M,N] w [N,K]
            dx = matmul(dy, w, split_k=sk).to(torch.bfloat16)
        if ctx.needs_input_grad[1]:     # tn: dy [M,N] x [M,K]
            dw = matmul(dy.t(), x, split_k=sk).to(torch.bfloat16)
        return dx, dw, None


class _LinearBf16Bias(torch.autograd.Function):
    """_LinearBf16 with a bias through torch elementwise ops: the composition
    the fused path replaces, kept as its A/B row and its oracle"""

    @staticmethod
    def forward(ctx, x, w, bias, split_k):
        ctx.save_for_backward(x, w)
        ctx.split_k = split_k
        ctx.bias_dtype = bias.dtype
        return (matmul_nt(x, w, split_k=split_k)
                + bias.float()).to(torch.bfloat16)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        sk = ctx.split_k
        if not dy.is_contiguous():
            dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = matmul(dy, w, split_k=sk).to(torch.bfloat16)
        if ctx.needs_input_grad[1]:
            dw = matmul(dy.t(), x, split_k=sk).to(torch.bfloat16)
        if ctx.needs_input_grad[2]:
            db = dy.float().sum(0).to(ctx.bias_dtype)
        return dx, dw, db, None


class _LinearBf16Fused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, split_k):
        ctx.save_for_backward(x, w)
        ctx.split_k = split_k
        ctx.bias_dtype = None if bias is None else bias.dtype
        return matmul(x, w.t(), split_k=split_k, out_dtype=torch.bfloat16,
                      bias=bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        sk = ctx.split_k
        if not dy.is_contiguous():  # e.g. the expanded scalar of sum()
            dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:     # nn: dy [M,N] w [N,K]
            dx = matmul(dy, w, split_k=sk, out_dtype=torch.bfloat16)
        if ctx.needs_input_grad[1]:     # tn: dy [M,N] x [M,K]
            dw = matmul(dy.t(), x, split_k=sk, out_dtype=torch.bfloat16)
        if ctx.bias_dtype is not None and ctx.needs_input_grad[2]:
            db = colsum_bf16(dy).to(ctx.bias_dtype)
        return dx, dw, db, None


def linear_bf16(x: torch.Tensor, w: torch.Tensor, split_k=None,
                bias: torch.Tensor = None, fused=None) -> torch.Tensor:
    """y = x @ w^T (+ bias) for bf16 x [M,K] and w [N,K], differentiable;
    every product runs on the K7 kernels with fp32 accumulation and comes
    out in bf16, and nothing is transposed in memory:

        forward   y  = matmul_nt(x, w)       nt
        backward  dx = matmul(dy, w)         nn
                  dw = matmul(dy.t(), x)     tn

    dw sums over the token dimension M. With many tokens and a small
    weight that is a split-K shape (few output tiles, a long sum), and
    without a split it runs on (N/128)*(K/128) workgroups. split_k="auto"
    hands "auto" to all three products, so each one gemm_splitk_plan
    answers more than 1 for — in practice such a dw — runs split over the
    machine (gemm_bf16_layout_splitk); its fp32 summation order, and with
    it possibly the last bit of the result, then differs from the default's.
    split_k is None (the default: no split anywhere) or "auto"; anything
    else is a ValueError.

    Without bias and fused this is the path above: fp32 products, each
    followed by a torch cast to bf16. bias ([N], bf16 or fp32) and fused
    choose the fused products (matmul(out_dtype=torch.bfloat16)): the GEMM
    kernels add the bias in fp32 and write bf16 themselves, the split
    products fold, add and convert in one kernel, and dbias is
    colsum_bf16(dy) cast to the bias's dtype; only the gradients asked for
    are computed. fused=None means fused iff a bias is given; True fuses
    without a bias; False with a bias runs the fp32 products plus torch
    elementwise ops (add, cast, and a torch column sum), the composition
    the fusion replaces. The fused forward runs the double-buffered 128^2
    kernel where the default runs the 256^2 8-phase one: on random data its
    last bit may differ from the default's (another fp32 summation order),
    for the same reason split_k="auto" may. Measured (docs/gemm.md, "bf16
    output and bias"): the 256^2 kernel plus add and cast is behind the
    fused call up to 4096^3 and level with it at 8192^3, the largest size
    swept.
    """
    _check_split_k(split_k, ints=False)
    if fused is not None and not isinstance(fused, bool):
        raise ValueError(f"fused must be None, True or False; got {fused!r}")
    if bias is not None and not isinstance(bias, torch.Tensor):
        raise TypeError(f"bias must be None or a tensor; got "
                        f"{type(bias).__name__}")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"need x[M,K], w[N,K]; got x{tuple(x.shape)} "
                         f"w{tuple(w.shape)}")
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise TypeError("x and w must be bf16")
    if not x.is_contiguous() or not w.is_contiguous():
        raise TypeError("x and w must be contiguous")
    if bias is None and not fused:
        return _LinearBf16.apply(x, w, split_k)
    if bias is not None:
        if bias.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"bias must be bfloat16 or float32, got "
                            f"{bias.dtype}")
        if bias.dim() != 1 or bias.shape[0] != w.shape[0]:
            raise ValueError(f"bias must have shape ({w.shape[0]},); got "
                             f"{tuple(bias.shape)}")
    if fused is False:
        return _LinearBf16Bias.apply(x, w, bias, split_k)
    return _LinearBf16Fused.apply(x, w, bias, split_k)


class _MlpBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, activation, split_k):
        gelu = activation == "gelu"
        res = matmul(x, w1.t(), split_k=split_k, out_dtype=torch.bfloat16,
                     bias=b1, activation=activation, return_aux=gelu)
        h, z = res if gelu else (res, None)
        y = matmul(h, w2.t(), split_k=split_k, out_dtype=torch.bfloat16,
                   bias=b2)
        # relu: h carries the mask; gelu: the derivative needs z
        ctx.save_for_backward(x, w1, w2, h, *((z,) if gelu else ()))
        ctx.activation = activation
        ctx.split_k = split_k
        ctx.bias_dtypes = tuple(None if b is None else b.dtype
                                for b in (b1, b2))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, h = ctx.saved_tensors[:4]
        aux = ctx.saved_tensors[4] if ctx.activation == "gelu" else h
        sk = ctx.split_k
        need = ctx.needs_input_grad
        bd1, bd2 = ctx.bias_dtypes
        if not dy.is_contiguous():  # e.g. the expanded scalar of sum()
            dy = dy.contiguous()
        dx = dw1 = db1 = dw2 = db2 = None
        need_b1 = bd1 is not None and need[2]
        if need[0] or need[1] or need_b1:   # nn: dy [M,O] w2 [O,H]
            dz = matmul(dy, w2, split_k=sk, out_dtype=torch.bfloat16,
                        activation_grad=(ctx.activation, aux))
            if need[0]:                     # nn: dz [M,H] w1 [H,I]
                dx = matmul(dz, w1, split_k=sk, out_dtype=torch.bfloat16)
            if need[1]:                     # tn: dz [M,H] x [M,I]
                dw1 = matmul(dz.t(), x, split_k=sk, out_dtype=torch.bfloat16)
            if need_b1:
                db1 = colsum_bf16(dz).to(bd1)
        if need[3]:                         # tn: dy [M,O] h [M,H]
            dw2 = matmul(dy.t(), h, split_k=sk, out_dtype=torch.bfloat16)
        if bd2 is not None and need[4]:
            db2 = colsum_bf16(dy).to(bd2)
        return dx, dw1, db1, dw2, db2, None, None


def mlp_bf16(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
             w2: torch.Tensor, b2: torch.Tensor, activation: str = "gelu",
             split_k=None) -> torch.Tensor:
    """y = act(x @ w1^T + b1) @ w2^T + b2 for bf16 x [M,I], w1 [H,I],
    w2 [O,H], differentiable; b1 [H] and b2 [O] are bf16, fp32 or None.
    activation is "relu" or "gelu" (tanh form; the erf form is not built).
    Every product is a matmul(out_dtype=torch.bfloat16) on the K7 kernels,
    and the activation and its derivative live in GEMM epilogues
    (gemm_bf16_act), so no elementwise pass touches the [M,H] tensor:

        forward   h (, z) = matmul(x, w1.t(), bias=b1, activation=...)   nt
                  y  = matmul(h, w2.t(), bias=b2)                        nt
        backward  dz  = matmul(dy, w2, activation_grad=(act, aux))       nn
                  dw2 = matmul(dy.t(), h)                                tn
                  db2 = colsum_bf16(dy)
                  dx  = matmul(dz, w1)                                   nn
                  dw1 = matmul(dz.t(), x)                                tn
                  db1 = colsum_bf16(dz)

    Saved for the backward pass: x, w1, w2, h and, for gelu, the bf16
    pre-activation z (aux = z); relu saves no z (aux = h, whose sign is the
    mask). Only the gradients asked for are computed. split_k is None or
    "auto", handed to every product (linear_bf16). Shape and dtype rules are
    linear_bf16's.
    """
    _check_split_k(split_k, ints=False)
    _check_activation_name(activation, "activation")
    for b, name in ((b1, "b1"), (b2, "b2")):
        if b is not None and not isinstance(b, torch.Tensor):
            raise TypeError(f"{name} must be None or a tensor; got "
                            f"{type(b).__name__}")
    if x.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 \
            or x.shape[1] != w1.shape[1] or w1.shape[0] != w2.shape[1]:
        raise ValueError(f"need x[M,I], w1[H,I], w2[O,H]; got "
                         f"x{tuple(x.shape)} w1{tuple(w1.shape)} "
                         f"w2{tuple(w2.shape)}")
    if x.dtype != torch.bfloat16 or w1.dtype != torch.bfloat16 \
            or w2.dtype != torch.bfloat16:
        raise TypeError("x, w1 and w2 must be bf16")
    if not x.is_contiguous() or not w1.is_contiguous() \
            or not w2.is_contiguous():
        raise TypeError("x, w1 and w2 must be contiguous")
    for b, w, name in ((b1, w1, "b1"), (b2, w2, "b2")):
        if b is None:
            continue
        if b.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"{name} must be bfloat16 or float32, got "
                            f"{b.dtype}")
        if b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"{name} must have shape ({w.shape[0]},); got "
                             f"{tuple(b.shape)}")
    return _MlpBf16.apply(x, w1, b1, w2, b2, activation, split_k)


# ---------------------------------------------------------------------------
# Batched and strided operands (native/gemm_batched.hip)
# ---------------------------------------------------------------------------

_BATCHED_LAYOUTS = {"nt": (False, False), **_LAYOUTS}
GEMM_BATCHED_MAX_BATCH = 65535      # gridDim.y


def gemm_batched_c_disjoint(batch: int, m: int, n: int, ldc: int,
                            bsc: int) -> bool:
    """ldc >= n and the C images of the batches pairwise disjoint, in one of
    the two forms gemm_bf16_batched takes: batch-major, bsc >= (m-1)*ldc + n
    (an image ends before the next begins), or interleaved inside a row,
    bsc >= n and ldc >= (batch-1)*bsc + n (the batches are column blocks of
    one wide row). With batch == 1 bsc is ignored. Pure arithmetic — the
    launcher's own rule (native gemm_batched_c_disjoint)."""
    if batch < 1 or m < 1 or n < 1 or ldc < n:
        return False
    if batch == 1:
        return True
    if bsc >= (m - 1) * ldc + n:
        return True
    return bsc >= n and ldc >= (batch - 1) * bsc + n


def _check_alpha(alpha):
    """alpha of bmm / bmm_bf16, on its type alone: a real number, finite or
    not, never a tensor"""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)):
        raise TypeError(f"alpha must be a real number (int or float), not "
                        f"{type(alpha).__name__}")


def gemm_bf16_batched(c: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                      layout: str = "nt", alpha: float = 1.0, stream=None,
                      xcd_swizzle: bool = False) -> None:
    """K7 batched: C_i[M,N] = alpha * op(A_i) @ op(B_i) for every i of the
    leading dimension, on 3-D bf16 operands AS STORED and read in place
    through their strides (native/gemm_batched.hip).

        layout  a          b
        "nt"    [B,M,K]    [B,N,K]
        "nn"    [B,M,K]    [B,K,N]
        "tn"    [B,K,M]    [B,K,N]
        "tt"    [B,K,M]    [B,N,K]

    c is [B,M,N], fp32 or bf16; its dtype picks the kernel. Every tensor
    needs stride(2) == 1; stride(1) is its row stride ld and stride(0) its
    batch stride bs, in elements, taken from the tensor — a head of a
    [tokens, heads*dim] activation is a, b or c with ld = heads*dim and
    bs = dim. bs may be 0 for a or b (an expand()ed operand: one matrix for
    every batch). Requires M,N % 128 == 0, K % 64 == 0, B <= 65535; a and b
    on 16-byte boundaries with ld and bs multiples of 8; the C images
    pairwise disjoint (gemm_batched_c_disjoint); a bf16 c also on a 16-byte
    boundary with ld and bs multiples of 8 (bmm pads and copies where
    needed). With B == 1 the batch strides mean nothing and are not judged.

    With alpha == 1 an fp32 c holds the bits of gemm_bf16_layout (nt: of
    gemm_bf16 under HPK_GEMM_VARIANT=db) per batch. alpha is one fp32
    multiply on the accumulator, always executed; a bf16 c is rounded once,
    to nearest even, after it. No bias, activation or split-K.
    """
    if layout not in _BATCHED_LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}; expected one of "
                         f"'nt', 'nn', 'tn', 'tt'")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8) \
                or b.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError("only bf16 has the batched, strided GEMM: the "
                            "8-bit and 4-bit transposed LDS reads "
                            "(ds_read_b64_tr_b8 / _tr_b4) are not built here")
        raise TypeError("a and b must be bf16; c fp32 or bf16")
    if c.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("a and b must be bf16; c fp32 or bf16")
    _check_alpha(alpha)
    for t, name in ((c, "c"), (a, "a"), (b, "b")):
        if not t.is_cuda or t.dim() != 3 or t.stride(2) != 1:
            raise TypeError(f"{name} must be a 3-D CUDA tensor with "
                            f"stride(2) == 1; got shape {tuple(t.shape)}, "
                            f"strides {t.stride()}")
    if a.device != c.device or b.device != c.device:
        raise TypeError("a, b and c must be on one device")
    a_t, b_n = _BATCHED_LAYOUTS[layout]
    batch = c.shape[0]
    k, m = a.shape[1:] if a_t else a.shape[:0:-1]
    kb, n = b.shape[1:] if b_n else b.shape[:0:-1]
    if kb != k or tuple(c.shape[1:]) != (m, n) or a.shape[0] != batch \
            or b.shape[0] != batch:
        raise ValueError(f"shape mismatch for layout {layout}: "
                         f"A{tuple(a.shape)} B{tuple(b.shape)} "
                         f"C{tuple(c.shape)}")
    if not 1 <= batch <= GEMM_BATCHED_MAX_BATCH:
        raise ValueError(f"gemm_bf16_batched requires 1 <= batch <= "
                         f"{GEMM_BATCHED_MAX_BATCH}; got {batch}")
    if m < 128 or n < 128 or k < 64 or m % 128 or n % 128 or k % 64:
        raise ValueError(f"gemm_bf16_batched requires M,N % 128 == 0 and "
                         f"K % 64 == 0; got M={m} N={n} K={k}")
    if a.data_ptr() % 16 != 0 or b.data_ptr() % 16 != 0:
        raise ValueError("a and b must start on 16-byte boundaries (they "
                         "are fetched in 16-byte chunks)")

    def strides(t):
        return t.stride(1), (t.stride(0) if batch > 1 else 0)

    (lda, bsa), (ldb, bsb), (ldc, bsc) = strides(a), strides(b), strides(c)
    for name, ld, bs, row in (("a", lda, bsa, a.shape[2]),
                              ("b", ldb, bsb, b.shape[2])):
        if ld % 8 or bs % 8:
            raise ValueError(f"{name}: stride(1) = {ld} and stride(0) = {bs} "
                             f"must be multiples of 8 elements (every "
                             f"16-byte chunk stays aligned)")
        if ld < row:
            raise ValueError(f"{name}: stride(1) = {ld} is below its row "
                             f"length {row}")
    if not gemm_batched_c_disjoint(batch, m, n, ldc, bsc):
        raise ValueError(f"c's batches overlap or its rows do: stride(1) = "
                         f"{ldc}, stride(0) = {bsc} for {batch} x {m} x {n}; "
                         f"need stride(1) >= N and either stride(0) >= "
                         f"(M-1)*stride(1) + N or stride(0) >= N and "
                         f"stride(1) >= (B-1)*stride(0) + N")
    if c.dtype == torch.bfloat16 and (c.data_ptr() % 16 or ldc % 8
                                      or bsc % 8):
        raise ValueError("a bf16 c must start on a 16-byte boundary with "
                         "stride(1) and stride(0) multiples of 8 elements "
                         "(its rows are written as 16-byte stores)")
    native().gemm_bf16_batched(
        c.data_ptr(), int(c.dtype == torch.bfloat16), a.data_ptr(),
        b.data_ptr(), m, n, k, batch, lda, bsa, ldb, bsb, ldc, bsc, layout,
        float(alpha), _stream_handle(stream), int(xcd_swizzle))


def bmm_layout(a: torch.Tensor, b: torch.Tensor):
    """(layout, a_stored, b_stored) of the logical batched product
    a [B,M,K] @ b [B,K,N], read from the strides; pure tensor metadata, any
    device.

    An argument is "n" if its stride(2) == 1 — asked first, so a tensor with
    a size-1 dimension, whose strides fit both readings, counts as row-major
    as in matmul_layout — and its stored tensor is itself; otherwise "t" if
    its stride(1) == 1, stored as transpose(1, 2) (a view, never a copy).
    The other strides are free: an expand()ed batch (stride(0) == 0) and a
    head of an interleaved activation (permute) are both fine. Anything
    else raises TypeError: no hidden copy.
    """
    def stored(t, name):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise TypeError(f"{name} must be a 3-D tensor")
        if t.stride(2) == 1:
            return t, "n"
        if t.stride(1) == 1:
            return t.transpose(1, 2), "t"
        raise TypeError(f"{name} has no unit stride in its last two "
                        f"dimensions (shape {tuple(t.shape)}, strides "
                        f"{t.stride()}); bmm makes no hidden copies")
    a_st, fa = stored(a, "a")
    b_st, fb = stored(b, "b")
    if a.shape[0] != b.shape[0] or a.shape[2] != b.shape[1]:
        raise ValueError(f"need a[B,M,K] @ b[B,K,N]; got a{tuple(a.shape)} "
                         f"b{tuple(b.shape)}")
    return fa + fb, a_st, b_st


def bmm_direct(t: torch.Tensor, row_mult: int, col_mult: int) -> bool:
    """Whether bmm hands the stored operand t [B,R,C] to the kernel as it
    is (True) or makes a zero-padded contiguous copy (False): whole tiles
    (R % row_mult == 0, C % col_mult == 0; 128 along M or N, 64 along K), a
    unit last stride, stride(1) and — for B > 1 — stride(0) multiples of 8,
    stride(1) no shorter than a row, and a start on a 16-byte boundary.
    Pure metadata, any device."""
    batch, rows, cols = t.shape
    if rows == 0 or cols == 0 or rows % row_mult or cols % col_mult:
        return False
    if t.stride(2) != 1 or t.stride(1) % 8 or t.stride(1) < cols:
        return False
    if batch > 1 and t.stride(0) % 8:
        return False
    return t.data_ptr() % 16 == 0


def _bmm_operand(t: torch.Tensor, rows: int, cols: int, row_mult: int,
                 col_mult: int):
    """t as the kernel takes it: itself, or a zero-padded contiguous copy
    [B, rows, cols]; a broadcast operand (stride(0) == 0) is padded once and
    expanded again"""
    if bmm_direct(t, row_mult, col_mult):
        return t
    batch = t.shape[0]
    once = batch > 1 and t.stride(0) == 0
    out = torch.zeros(1 if once else batch, rows, cols, dtype=t.dtype,
                      device=t.device)
    out[:, : t.shape[1], : t.shape[2]] = t[:1] if once else t
    return out.expand(batch, rows, cols) if once else out


@_body_on_stream
def bmm(a: torch.Tensor, b: torch.Tensor, out_dtype=None, alpha=1.0,
        stream=None) -> torch.Tensor:
    """Batched front door: alpha * (a [B,M,K] @ b [B,K,N]) for bf16 a, b of
    any B, M, N, K, as a fresh contiguous [B,M,N] tensor — fp32, or bf16
    for out_dtype=torch.bfloat16 (rounded once, after the multiply).

    The layout is read from the strides (bmm_layout: no hidden copy of a
    tensor with no unit stride, that is a TypeError). A stored operand of
    whole tiles with qualifying strides and alignment (bmm_direct) goes to
    gemm_bf16_batched as it is — for x, y [T, H*D] with T, D % 128 == 0,

        q = x.view(T, H, D).permute(1, 0, 2)
        k = y.view(T, H, D).permute(1, 2, 0)
        s = bmm(q, k, alpha=D ** -0.5)

    is layout nt with ld = H*D, bs = D and copies nothing. Everything else
    is copied zero-padded to gemm_layout_pad_shapes (zeros add nothing) and
    the result is sliced, as matmul does; a broadcast operand is padded
    once, not B times. More than 65535 batches run as several launches.
    out_dtype and alpha (a real number, finite or not, never a tensor) are
    judged before any tensor is looked at.
    """
    if out_dtype is not None and out_dtype is not torch.bfloat16:
        raise ValueError(f"out_dtype must be None or torch.bfloat16; got "
                         f"{out_dtype!r}")
    _check_alpha(alpha)
    layout, a_st, b_st = bmm_layout(a, b)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        if a.dtype in (torch.float8_e4m3fn, torch.int8, torch.uint8):
            raise TypeError(_NO_NARROW_TR)
        raise TypeError(f"bmm takes bf16 operands; got {a.dtype} and "
                        f"{b.dtype}")
    if a.device != b.device:
        raise TypeError(f"a is on {a.device}, b on {b.device}")
    batch, m, k = a.shape
    n = b.shape[2]
    dtype = torch.float32 if out_dtype is None else torch.bfloat16
    if batch == 0 or m == 0 or n == 0 or k == 0:
        return torch.zeros(batch, m, n, dtype=dtype, device=a.device)
    mp, np_, kp = gemm_layout_pad_shapes(m, n, k)
    a_t, b_n = _BATCHED_LAYOUTS[layout]
    ap = _bmm_operand(a_st, *((kp, mp, 64, 128) if a_t else (mp, kp, 128, 64)))
    bp = _bmm_operand(b_st, *((kp, np_, 64, 128) if b_n
                              else (np_, kp, 128, 64)))
    c = torch.empty(batch, mp, np_, dtype=dtype, device=a.device)
    for b0 in range(0, batch, GEMM_BATCHED_MAX_BATCH):
        b1 = min(batch, b0 + GEMM_BATCHED_MAX_BATCH)
        gemm_bf16_batched(c[b0:b1], ap[b0:b1], bp[b0:b1], layout,
                          alpha=alpha, stream=stream)
    if (mp, np_) == (m, n):
        return c
    return c[:, :m, :n].contiguous()


class _BmmBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, alpha):
        ctx.save_for_backward(a, b)
        ctx.alpha = alpha
        return bmm(a, b, out_dtype=torch.bfloat16, alpha=alpha)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        if dy.stride(2) != 1 and dy.stride(1) != 1:
            dy = dy.contiguous()    # e.g. the expanded scalar of sum()
        da = db = None
        if ctx.needs_input_grad[0]:     # [B,M,N] @ [B,N,K]
            da = bmm(dy, b.transpose(1, 2), out_dtype=torch.bfloat16,
                     alpha=ctx.alpha)
        if ctx.needs_input_grad[1]:     # [B,K,M] @ [B,M,N]
            db = bmm(a.transpose(1, 2), dy, out_dtype=torch.bfloat16,
                     alpha=ctx.alpha)
        return da, db, None


def bmm_bf16(a: torch.Tensor, b: torch.Tensor, alpha=1.0) -> torch.Tensor:
    """y = alpha * (a [B,M,K] @ b [B,K,N]) for bf16 a and b, differentiable;
    every product is a bmm(out_dtype=torch.bfloat16) on the batched K7
    kernels, fp32 accumulation, one rounding, and nothing is transposed in
    memory — the layouts come from the strides:

        forward   y  = bmm(a, b, alpha)
        backward  da = bmm(dy, b.transpose(1, 2), alpha)
                  db = bmm(a.transpose(1, 2), dy, alpha)

    Only the gradients asked for are computed. a and b are what bmm takes:
    heads of an interleaved activation and expand()ed operands included
    (autograd sums the gradient of an expand itself).
    """
    _check_alpha(alpha)
    return _BmmBf16.apply(a, b, alpha)
