"""MI355X workload kernels (native: ops/kernels/workload.hip) with torch tensors.

* :func:`gemm_bf16_nt` — ``C = A @ B.T`` on MFMA (bf16 in, fp32 accumulate, bf16 out)
* :func:`stream_triad` — ``c = a + s * b`` (fp32, HBM-bound)
* :func:`gemm_mxfp8_nt` — the same product on block-scaled fp8 (OCP e4m3 with one
  E8M0 scale per 32 along K, "MXFP8"), and :func:`quantize_mxfp8`, which makes
  such operands from bf16 on the device
* :func:`gemm_mxfp4_nt` and :func:`quantize_mxfp4` — the same pair on block-scaled
  fp4 (OCP e2m1, two elements per byte, "MXFP4"), the format with CDNA4's highest
  matrix rate
* :func:`gemm_mxfp4_skinny_nt` — the MXFP4 product for a decode batch of 1-64 rows:
  weights streamed once from HBM, K split over blocks, ordered reduction
* :func:`attn_decode_bf16` — decode attention ``softmax(q·Kᵀ)·V`` of one new token per
  sequence over a bf16 KV cache with grouped query heads: the cache streamed once from
  HBM, the keys split over blocks, partials merged in a fixed order
* ``attn_prefill_bf16`` — causal prefill attention over the same cache, lives in :mod:`.attention` (ops/attention.py)
* :class:`Burner` — runs a GEMM + triad mix on a side stream for a target
  duration: the synthetic "GPU pod" whose power / HBM / activity the
  exporter reports (``precision="mxfp8"`` / ``"mxfp4"``: inference-like mixes;
  ``batch=``: the decode mix; ``context=``: with attention over a KV cache).

Shapes are validated on the host before any launch (the kernels assume full
tiles and 16-byte alignment); there is no PyTorch fallback.
"""
from __future__ import annotations

import threading
from typing import Optional

import torch

from . import load_native

_mod = None


def native():
    global _mod
    if _mod is None:
        _mod = load_native("_workload")
    return _mod


def tile():
    return native().tile()


def _stream_handle(stream: Optional[torch.cuda.Stream], device) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return int(s.cuda_stream)


#: Kernel variants of gemm_bf16_nt (see kernels/workload.hip): picked by shape
#: by default; forcing one is for tests and A/B timing.
GEMM_VARIANTS = {"auto": 0, "tile128": 1, "tile256": 2, "tile256_dma": 3}
#: Operand precisions of the GEMM in Burner and time_gemm.
PRECISIONS = ("bf16", "mxfp8", "mxfp4")


def gemm_bf16_nt(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None, variant: str = "auto") -> torch.Tensor:
    """C[M,N] = A[M,K] @ B[N,K]^T with M,N multiples of 128 and K of 64.

    ``variant`` forces one kernel: ``tile256`` needs M,N multiples of 256 and
    ``tile256_dma`` (the 8-phase LDS-DMA kernel) additionally K a multiple of 128.
    """
    if variant not in GEMM_VARIANTS:
        raise ValueError(f"unknown variant {variant!r}; one of {sorted(GEMM_VARIANTS)}")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16:
        raise TypeError("gemm_bf16_nt expects bfloat16 inputs")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)} (need A[M,K], B[N,K])")
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise ValueError("A and B must be on the same GPU")
    bm, bn, bk = tile()
    m, k = a.shape
    n = b.shape[0]
    if m % bm or n % bn or k % bk:
        raise ValueError(f"gemm_bf16_nt needs M%{bm}==0, N%{bn}==0, K%{bk}==0 (got {m}x{n}x{k})")
    a = a.contiguous()
    b = b.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a contiguous bfloat16 [M,N] tensor on A's device")
    native().gemm_bf16_nt(a.data_ptr(), b.data_ptr(), out.data_ptr(), m, n, k, _stream_handle(stream, a.device),
                          GEMM_VARIANTS[variant])
    return out


def _check_mx_scales(name: str, scale: torch.Tensor, operand: torch.Tensor, per_byte: int = 1) -> None:
    rows, k = operand.shape[0], operand.shape[1] * per_byte  # per_byte: elements in one byte of the operand
    if scale.dtype != torch.uint8:
        raise TypeError(f"{name} must be uint8 (E8M0)")
    if scale.shape != (rows, k // 32) or scale.device != operand.device:
        raise ValueError(f"{name} must be [{rows},{k // 32}] (one byte per 32 along K) on its operand's device, "
                         f"got {tuple(scale.shape)}")


def gemm_mxfp8_nt(a: torch.Tensor, b: torch.Tensor, scale_a: Optional[torch.Tensor] = None,
                  scale_b: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                  stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """C[M,N] = (A·2^(SA−127)) @ (B·2^(SB−127))^T in bf16, with fp32 accumulation.

    ``a`` [M,K] and ``b`` [N,K] are ``float8_e4m3fn``; ``scale_a`` [M,K/32] and
    ``scale_b`` [N,K/32] are ``uint8`` E8M0 exponents, one per 32 elements along
    K, both given or both ``None`` (a plain fp8 GEMM). M and N must be multiples
    of 256, K of 128, and M·K and N·K below 2^32; ``out`` must be 16-byte aligned.
    """
    if a.dtype != torch.float8_e4m3fn or b.dtype != torch.float8_e4m3fn:
        raise TypeError("gemm_mxfp8_nt expects float8_e4m3fn inputs")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)} (need A[M,K], B[N,K])")
    m, k = a.shape
    n = b.shape[0]
    if m % 256 or n % 256 or k % 128 or m * k >= 2 ** 32 or n * k >= 2 ** 32:
        raise ValueError(f"gemm_mxfp8_nt needs M%256==0, N%256==0, K%128==0, M*K and N*K < 2^32 (got {m}x{n}x{k})")
    if (scale_a is None) != (scale_b is None):
        raise ValueError("give both scale_a and scale_b, or neither")
    if scale_a is not None:
        _check_mx_scales("scale_a", scale_a, a)
        _check_mx_scales("scale_b", scale_b, b)
        scale_a = scale_a.contiguous()
        scale_b = scale_b.contiguous()
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise ValueError("A and B must be on the same GPU")
    a = a.contiguous()
    b = b.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a contiguous bfloat16 [M,N] tensor on A's device")
    native().gemm_mxfp8_nt(a.data_ptr(), b.data_ptr(), scale_a.data_ptr() if scale_a is not None else 0,
                           scale_b.data_ptr() if scale_b is not None else 0, out.data_ptr(), m, n, k,
                           _stream_handle(stream, a.device))
    return out


def quantize_mxfp8(x: torch.Tensor, stream: Optional[torch.cuda.Stream] = None):
    """bf16 [R,K] → (``float8_e4m3fn`` [R,K], ``uint8`` E8M0 scales [R,K/32]) by the OCP MX rule.

    Per block of 32 along K: X = floor(log2(amax)) − 8 clamped to [−127, 127], scale
    byte X + 127, elements RNE_e4m3(clamp(v·2^−X, ±448)); an all-zero block gets
    scale byte 127. ``x`` is contiguous and finite, K a multiple of 32.
    """
    if x.dtype != torch.bfloat16:
        raise TypeError("quantize_mxfp8 expects bfloat16")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 32 or not x.is_contiguous():
        raise ValueError(f"quantize_mxfp8 needs a contiguous [R,K] tensor with K%32==0 (got {tuple(x.shape)})")
    if not x.is_cuda:
        raise ValueError("x must be on a GPU")
    rows, k = x.shape
    q = torch.empty((rows, k), dtype=torch.float8_e4m3fn, device=x.device)
    scales = torch.empty((rows, k // 32), dtype=torch.uint8, device=x.device)
    native().quantize_mxfp8(x.data_ptr(), q.data_ptr(), scales.data_ptr(), rows, k, _stream_handle(stream, x.device))
    return q, scales


def gemm_mxfp4_nt(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                  out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """C[M,N] = (A·2^(SA−127)) @ (B·2^(SB−127))^T in bf16, on packed fp4 with fp32 accumulation.

    ``a`` [M,K/2] and ``b`` [N,K/2] are ``uint8`` holding two OCP e2m1 elements per byte,
    element 2i in bits 0-3 of byte i; ``scale_a`` [M,K/32] and ``scale_b`` [N,K/32] are
    ``uint8`` E8M0 exponents, one per 32 elements along K, and mandatory. M and N must be
    multiples of 256, K of 512 (the kernel consumes 256-element K-tiles in pairs), and
    M·K/2 and N·K/2 below 2^32; ``out`` must be 16-byte aligned.
    """
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError("gemm_mxfp4_nt expects uint8 inputs (two e2m1 elements per byte)")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)} (need A[M,K/2], B[N,K/2])")
    m, k = a.shape[0], 2 * a.shape[1]
    n = b.shape[0]
    if m % 256 or n % 256 or k % 512 or m * k // 2 >= 2 ** 32 or n * k // 2 >= 2 ** 32:
        raise ValueError(f"gemm_mxfp4_nt needs M%256==0, N%256==0, K%512==0, M*K/2 and N*K/2 < 2^32 (got {m}x{n}x{k})")
    if scale_a is None or scale_b is None:
        raise ValueError("gemm_mxfp4_nt needs both scale_a and scale_b")
    _check_mx_scales("scale_a", scale_a, a, per_byte=2)
    _check_mx_scales("scale_b", scale_b, b, per_byte=2)
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise ValueError("A and B must be on the same GPU")
    a, b, scale_a, scale_b = a.contiguous(), b.contiguous(), scale_a.contiguous(), scale_b.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a contiguous bfloat16 [M,N] tensor on A's device")
    native().gemm_mxfp4_nt(a.data_ptr(), b.data_ptr(), scale_a.data_ptr(), scale_b.data_ptr(), out.data_ptr(), m, n, k,
                           _stream_handle(stream, a.device))
    return out


def quantize_mxfp4(x: torch.Tensor, stream: Optional[torch.cuda.Stream] = None):
    """bf16 [R,K] → (``uint8`` packed e2m1 [R,K/2], ``uint8`` E8M0 scales [R,K/32]) by the OCP MX rule.

    Per block of 32 along K: X = floor(log2(amax)) − 2 clamped to [−127, 127], scale byte
    X + 127, elements RNE_e2m1(clamp(v·2^−X, ±6)) with the sign of v kept (a negative value
    that rounds to zero is −0); an all-zero block gets scale byte 127. Element 2i is in bits
    0-3 of byte i. ``x`` is contiguous and finite, K a multiple of 32.
    """
    if x.dtype != torch.bfloat16:
        raise TypeError("quantize_mxfp4 expects bfloat16")
    if x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % 32 or not x.is_contiguous():
        raise ValueError(f"quantize_mxfp4 needs a contiguous [R,K] tensor with K%32==0 (got {tuple(x.shape)})")
    if not x.is_cuda:
        raise ValueError("x must be on a GPU")
    rows, k = x.shape
    q = torch.empty((rows, k // 2), dtype=torch.uint8, device=x.device)
    scales = torch.empty((rows, k // 32), dtype=torch.uint8, device=x.device)
    native().quantize_mxfp4(x.data_ptr(), q.data_ptr(), scales.data_ptr(), rows, k, _stream_handle(stream, x.device))
    return q, scales


#: ``split_k=0`` keeps (N/128)·split_k at or below this multiple of the CU count
#: (measured: profiles/mxfp4_skinny_ab.md).
SKINNY_CU_MULTIPLE = 1


def skinny_split_k(n: int, k: int, device) -> int:
    """The split ``gemm_mxfp4_skinny_nt`` picks for ``split_k=0``: the largest divisor of K/256 that keeps
    (N/128)·split_k at or below ``SKINNY_CU_MULTIPLE`` times the device's CU count."""
    limit = SKINNY_CU_MULTIPLE * torch.cuda.get_device_properties(device).multi_processor_count // (n // 128)
    return max((d for d in range(1, k // 256 + 1) if (k // 256) % d == 0 and d <= limit), default=1)


def gemm_mxfp4_skinny_nt(a: torch.Tensor, b: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                         out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                         split_k: int = 0, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The product of :func:`gemm_mxfp4_nt` for a decode batch: 1 ≤ M ≤ 64 (any value), N a multiple of 128,
    K of 256, N·K/2 below 2^32; operands and scales in the same formats.

    K is split over ``split_k`` blocks (a divisor of K/256; 0: :func:`skinny_split_k`) whose fp32 partial sums
    go to ``workspace`` (float32, at least split_k·M·N elements, allocated on the launch stream when absent) and
    are added in ascending order by a second kernel, so the result is bit-identical from run to run.
    ``out`` and ``workspace`` must be 16-byte aligned.
    """
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError("gemm_mxfp4_skinny_nt expects uint8 inputs (two e2m1 elements per byte)")
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"shape mismatch: A{tuple(a.shape)} B{tuple(b.shape)} (need A[M,K/2], B[N,K/2])")
    m, k = a.shape[0], 2 * a.shape[1]
    n = b.shape[0]
    if not 1 <= m <= 64 or n == 0 or n % 128 or k == 0 or k % 256 or n * k // 2 >= 2 ** 32:
        raise ValueError(f"gemm_mxfp4_skinny_nt needs 1<=M<=64, N%128==0, K%256==0, N*K/2 < 2^32 (got {m}x{n}x{k})")
    if split_k < 0 or (split_k and (k // 256) % split_k):
        raise ValueError(f"split_k must divide K/256 = {k // 256} (got {split_k})")
    if scale_a is None or scale_b is None:
        raise ValueError("gemm_mxfp4_skinny_nt needs both scale_a and scale_b")
    _check_mx_scales("scale_a", scale_a, a, per_byte=2)
    _check_mx_scales("scale_b", scale_b, b, per_byte=2)
    if not (a.is_cuda and b.is_cuda) or a.device != b.device:
        raise ValueError("A and B must be on the same GPU")
    a, b, scale_a, scale_b = a.contiguous(), b.contiguous(), scale_a.contiguous(), scale_b.contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.bfloat16, device=a.device)
    elif out.shape != (m, n) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("out must be a contiguous bfloat16 [M,N] tensor on A's device")
    split_k = split_k or skinny_split_k(n, k, a.device)
    s = stream if stream is not None else torch.cuda.current_stream(a.device)
    if split_k == 1:
        workspace = None
    elif workspace is None:
        with torch.cuda.stream(s):
            workspace = torch.empty(split_k * m * n, dtype=torch.float32, device=a.device)
    elif (workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != a.device
          or workspace.numel() < split_k * m * n):
        raise ValueError(f"workspace must be a contiguous float32 tensor of at least split_k*M*N = "
                         f"{split_k * m * n} elements on A's device")
    native().gemm_mxfp4_skinny_nt(a.data_ptr(), b.data_ptr(), scale_a.data_ptr(), scale_b.data_ptr(), out.data_ptr(),
                                  m, n, k, split_k, workspace.data_ptr() if workspace is not None else 0,
                                  workspace.numel() * 4 if workspace is not None else 0, int(s.cuda_stream))
    return out


#: ``split_kv=0`` keeps B·Hkv·split_kv at or below this multiple of the CU count and every slice at least
#: ``ATTN_MIN_SLICE`` keys long (measured: profiles/attn_decode_ab.md).
ATTN_CU_MULTIPLE = 1
ATTN_MIN_SLICE = 512


def attn_split_kv(b: int, hkv: int, s_max: int, device) -> int:
    """The split ``attn_decode_bf16`` picks for ``split_kv=0``: the largest that keeps B·Hkv·split at or below
    ``ATTN_CU_MULTIPLE`` times the device's CU count and leaves every slice of an ``s_max``-long sequence at
    least ``ATTN_MIN_SLICE`` keys. It looks at ``s_max``, not at the lengths, so it needs no device sync."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(ATTN_CU_MULTIPLE * cus // (b * hkv), s_max // ATTN_MIN_SLICE))


def attn_decode_bf16(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, seq_lens: torch.Tensor,
                     out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                     split_kv: int = 0, workspace: Optional[torch.Tensor] = None,
                     scale: Optional[float] = None) -> torch.Tensor:
    """out[b,h] = Σ_s softmax_s(scale · q[b,h]·k_cache[b,h//G,s]) · v_cache[b,h//G,s] over s < seq_lens[b].

    ``q`` [B,Hq,128] and the contiguous caches [B,Hkv,S_max,128] are bfloat16, ``seq_lens`` [B] int32 with
    1 ≤ len ≤ S_max, Hq = G·Hkv with 1 ≤ G ≤ 16 (any value); ``scale`` defaults to 128^-½. Accumulation is
    fp32, the result [B,Hq,128] bfloat16. A cache must be smaller than 2^32 bytes.

    Each sequence's keys are split over ``split_kv`` blocks (0: :func:`attn_split_kv`) whose fp32 partial
    accumulators, maxima and sums go to ``workspace`` (float32, at least split_kv·B·Hq·130 elements, allocated
    on the launch stream when absent) and are merged in ascending order by a second kernel, so the result is
    bit-identical from run to run. ``q``, ``out`` and ``workspace`` must be 16-byte aligned.
    """
    if any(t.dtype != torch.bfloat16 for t in (q, k_cache, v_cache)):
        raise TypeError("attn_decode_bf16 expects bfloat16 q, k_cache and v_cache")
    if q.dim() != 3 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[0] != k_cache.shape[0]:
        raise ValueError(f"shape mismatch: q{tuple(q.shape)} k_cache{tuple(k_cache.shape)} v_cache"
                         f"{tuple(v_cache.shape)} (need q[B,Hq,128], caches [B,Hkv,S_max,128])")
    b, hq, d = q.shape
    hkv, s_max = k_cache.shape[1], k_cache.shape[2]
    if d != 128 or k_cache.shape[3] != 128:
        raise ValueError(f"attn_decode_bf16 needs head dim 128 (got {d} and {k_cache.shape[3]})")
    if b == 0 or hkv == 0 or s_max == 0 or hq == 0 or hq % hkv:
        raise ValueError(f"Hq must be a positive multiple of Hkv, B and S_max positive (got Hq {hq}, Hkv {hkv}, "
                         f"B {b}, S_max {s_max})")
    g = hq // hkv
    if g > 16:
        raise ValueError(f"attn_decode_bf16 needs Hq/Hkv <= 16 (got {g})")
    if b * hkv * s_max * 256 >= 2 ** 32 or b > 65535:
        raise ValueError("attn_decode_bf16 needs B <= 65535 and caches smaller than 2^32 bytes (B*Hkv*S_max*256)")
    if seq_lens.dtype != torch.int32:
        raise TypeError("seq_lens must be int32")
    if seq_lens.shape != (b,) or not 0 <= split_kv <= 65535:
        raise ValueError(f"seq_lens must be [{b}], got {tuple(seq_lens.shape)}; split_kv in 0..65535, got {split_kv}")
    if not (k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("k_cache and v_cache must be contiguous")
    if not all(t.is_cuda and t.device == q.device for t in (q, k_cache, v_cache, seq_lens)):
        raise ValueError("q, k_cache, v_cache and seq_lens must be on the same GPU")
    q, seq_lens = q.contiguous(), seq_lens.contiguous()
    if out is None:
        out = torch.empty((b, hq, 128), dtype=torch.bfloat16, device=q.device)
    elif out.shape != (b, hq, 128) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != q.device:
        raise ValueError("out must be a contiguous bfloat16 [B,Hq,128] tensor on q's device")
    split_kv = split_kv or attn_split_kv(b, hkv, s_max, q.device)
    s = stream if stream is not None else torch.cuda.current_stream(q.device)
    need = split_kv * b * hq * 130
    if split_kv == 1:
        workspace = None
    elif workspace is None:
        with torch.cuda.stream(s):
            workspace = torch.empty(need, dtype=torch.float32, device=q.device)
    elif (workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != q.device
          or workspace.numel() < need):
        raise ValueError(f"workspace must be a contiguous float32 tensor of at least split_kv*B*Hq*130 = {need} "
                         f"elements on q's device")
    native().attn_decode_bf16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), seq_lens.data_ptr(),
                              out.data_ptr(), b, hkv, g, s_max, float(scale if scale is not None else 128 ** -0.5),
                              split_kv, workspace.data_ptr() if workspace is not None else 0,
                              workspace.numel() * 4 if workspace is not None else 0, int(s.cuda_stream))
    return out


#: The block-scaled precisions: (quantiser, GEMM) with one calling convention.
_MX = {"mxfp8": (quantize_mxfp8, gemm_mxfp8_nt), "mxfp4": (quantize_mxfp4, gemm_mxfp4_nt)}


def stream_triad(a: torch.Tensor, b: torch.Tensor, s: float, out: Optional[torch.Tensor] = None,
                 stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """out = a + s * b over contiguous float32 vectors whose length is a multiple of 4."""
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError("stream_triad expects float32")
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("a and b must be contiguous and the same shape")
    n = a.numel()
    if n % 4:
        raise ValueError("length must be a multiple of 4")
    if out is None:
        out = torch.empty_like(a)
    native().stream_triad(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, float(s), _stream_handle(stream, a.device))
    return out


class Burner:
    """Keeps one GPU busy with a training-like mix until stopped.

    Each iteration runs ``gemms`` MFMA GEMMs of ``size``³ then one HBM triad
    over ``triad_mb`` MB on its own stream. With ``graph_iters > 0`` that many
    iterations are captured once into a HIP graph and replayed, so the host
    thread wakes once per replay instead of launching every kernel from
    Python. The default is eager launches: on this ROCm stack a device-wide
    ``torch.cuda.synchronize()`` takes ~0.4-2 s once a graph has been replayed
    on the device, even with the device idle (tools/diag/sync_vs_burner.py,
    profiles/r1_diag_graph_sync.md), and the benchmark's timed region is
    bracketed by exactly that call. Callers keep the launch rate low with
    larger kernels instead (bench.py: 2 × 8192³ GEMMs + triad per iteration).
    ``precision="mxfp8"`` and ``"mxfp4"`` are the inference-like mixes: the
    weight operand is quantised once, and each iteration re-quantises the
    activation operand once and runs the ``gemms`` GEMMs on MXFP8 / MXFP4.
    ``batch`` (1..64, ``precision="mxfp4"`` only, ``size`` a multiple of 256) is
    the decode mix: the activation operand is ``[batch, size]`` and the GEMMs
    are :func:`gemm_mxfp4_skinny_nt`, which stream the weights from HBM.
    ``context`` (with ``batch``, ``size`` a multiple of 1024) adds the other HBM
    stream of a decode step: after each GEMM one :func:`attn_decode_bf16` of
    ``size/128`` query heads in groups of 8 over a random bf16 KV cache of
    ``context`` keys per sequence, its queries the GEMM's output.
    """

    def __init__(self, device: int = 0, size: int = 4096, gemms: int = 4, triad_mb: int = 1024,
                 graph_iters: int = 0, precision: str = "bf16", batch: Optional[int] = None,
                 context: Optional[int] = None):
        if precision not in PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}; one of {PRECISIONS}")
        if batch is not None and (precision != "mxfp4" or not 1 <= batch <= 64 or size % 256):
            raise ValueError(f"batch needs precision='mxfp4', 1 <= batch <= 64 and size%256==0 "
                             f"(got {precision!r}, batch {batch}, size {size})")
        if context is not None and (batch is None or size % 1024 or context < 1):
            raise ValueError(f"context needs batch, size%1024==0 and context >= 1 "
                             f"(got batch {batch}, size {size}, context {context})")
        self.precision = precision
        self.batch = batch
        self.context = context
        self.device = torch.device("cuda", device)
        self.size = size
        self.gemms = gemms
        self.triad_n = (triad_mb * 1024 * 1024 // 4) // 4 * 4
        self.graph_iters = graph_iters
        self.mode = "pending"  # "graph" once capture succeeded, "eager" if graphs are disabled
        self._stop = threading.Event()
        self._pause = threading.Event()
        self._idle = threading.Event()
        self._thread: Optional[threading.Thread] = None
        self.iterations = 0
        self.error: Optional[BaseException] = None

    def _run(self) -> None:
        try:
            torch.cuda.set_device(self.device)
            g = torch.Generator(device=self.device).manual_seed(0)
            a = torch.randn(self.batch or self.size, self.size, device=self.device, dtype=torch.bfloat16, generator=g)
            b = torch.randn(self.size, self.size, device=self.device, dtype=torch.bfloat16, generator=g)
            c = torch.empty_like(a)
            x = torch.rand(self.triad_n, device=self.device, generator=g)
            y = torch.rand(self.triad_n, device=self.device, generator=g)
            z = torch.empty_like(x)
            stream = torch.cuda.Stream(self.device)

            if self.precision in _MX:
                quantise, gemm = _MX[self.precision]
                stream.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(stream):
                    bq, bs = quantise(b)  # the weights: once
                    if self.batch:  # decode: the skinny kernel, split and workspace fixed once
                        split = skinny_split_k(self.size, self.size, self.device)
                        ws = torch.empty(split * self.batch * self.size, dtype=torch.float32, device=self.device)

                        def gemm(aq, bq, as_, bs, out, stream):
                            gemm_mxfp4_skinny_nt(aq, bq, as_, bs, out=out, stream=stream, split_k=split, workspace=ws)

                        if self.context:  # attention over the KV cache after every projection
                            hq = self.size // 128
                            kv = [torch.randn(self.batch, hq // 8, self.context, 128, device=self.device,
                                              dtype=torch.bfloat16, generator=g) for _ in range(2)]
                            lens = torch.full((self.batch,), self.context, device=self.device, dtype=torch.int32)
                            o = torch.empty(self.batch, hq, 128, device=self.device, dtype=torch.bfloat16)
                            asplit = attn_split_kv(self.batch, hq // 8, self.context, self.device)
                            aws = torch.empty(asplit * self.batch * hq * 130, dtype=torch.float32, device=self.device)
                            project = gemm

                            def gemm(aq, bq, as_, bs, out, stream):
                                project(aq, bq, as_, bs, out=out, stream=stream)
                                attn_decode_bf16(out.view(self.batch, hq, 128), kv[0], kv[1], lens, out=o,
                                                 stream=stream, split_kv=asplit, workspace=aws)

                def one_iteration():
                    aq, as_ = quantise(a, stream=stream)
                    for _ in range(self.gemms):
                        gemm(aq, bq, as_, bs, out=c, stream=stream)
                    stream_triad(x, y, 0.5, out=z, stream=stream)
            else:
                def one_iteration():
                    for _ in range(self.gemms):
                        gemm_bf16_nt(a, b, out=c, stream=stream)
                    stream_triad(x, y, 0.5, out=z, stream=stream)

            with torch.cuda.stream(stream):
                one_iteration()  # warm-up outside capture (sets kernel attributes once)
            stream.synchronize()
            if self.graph_iters > 0:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    for _ in range(self.graph_iters):
                        one_iteration()
                self.mode = "graph"
                while not self._stop.is_set():
                    if self._pause.is_set():
                        self._hold()
                        continue
                    graph.replay()
                    stream.synchronize()
                    self.iterations += self.graph_iters
            else:
                self.mode = "eager"
                while not self._stop.is_set():
                    if self._pause.is_set():
                        self._hold()
                        continue
                    with torch.cuda.stream(stream):
                        one_iteration()
                    stream.synchronize()
                    self.iterations += 1
        except BaseException as e:  # surfaced by stop()
            self.error = e
        finally:
            self._idle.set()

    def _hold(self) -> None:
        self._idle.set()
        while self._pause.is_set() and not self._stop.is_set():
            self._stop.wait(0.001)
        self._idle.clear()

    def pause(self, timeout: float = 10.0) -> None:
        """Stop issuing work and wait until the in-flight iteration finished
        (a device-wide synchronize then only waits for the caller's work)."""
        if self._thread is None or not self._thread.is_alive():
            return
        self._pause.set()
        self._idle.wait(timeout)

    def resume(self) -> None:
        self._pause.clear()

    def start(self) -> "Burner":
        self._thread = threading.Thread(target=self._run, daemon=True, name="gpu-burner")
        self._thread.start()
        return self

    def stop(self, timeout: float = 30.0) -> int:
        self._stop.set()
        if self._thread:
            self._thread.join(timeout)
        if self.error:
            raise RuntimeError(f"burner failed: {self.error}") from self.error
        return self.iterations

    def __enter__(self):
        return self.start()

    def __exit__(self, *exc):
        self.stop()


def gemm_tflops(m: int, n: int, k: int, seconds: float) -> float:
    return 2.0 * m * n * k / seconds / 1e12


def time_gemm(size: int = 8192, iters: int = 20, device: int = 0, variant: str = "auto",
              precision: str = "bf16") -> float:
    """Median TFLOP/s of the GEMM at size³ (uniform random operands): gemm_bf16_nt, or with
    ``precision="mxfp8"`` / ``"mxfp4"`` that precision's GEMM on the quantised operands (same 2·M·N·K count)."""
    if precision not in PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}; one of {PRECISIONS}")
    dev = torch.device("cuda", device)
    a = (torch.rand(size, size, device=dev) * 2 - 1).to(torch.bfloat16)
    b = (torch.rand(size, size, device=dev) * 2 - 1).to(torch.bfloat16)
    c = torch.empty_like(a)
    if precision in _MX:
        quantise, gemm = _MX[precision]
        operands = quantise(a) + quantise(b)

        def run():
            gemm(operands[0], operands[2], operands[1], operands[3], out=c)
    else:
        def run():
            gemm_bf16_nt(a, b, out=c, variant=variant)
    for _ in range(3):
        run()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        run()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    times.sort()
    return gemm_tflops(size, size, size, times[len(times) // 2])


def time_gemm_skinny(m: int, n: int, k: int, iters: int = 20, device: int = 0, split_k: int = 0,
                     padded: bool = False) -> float:
    """Median TB/s of gemm_mxfp4_skinny_nt over the bytes it must move (B, SB, A, SA, C) at a decode shape.

    The weights rotate over enough distinct buffers to exceed 512 MiB, twice the 256 MiB Infinity Cache, so the
    figure is HBM bandwidth. Each sample is one pass over all buffers between two events, enqueued behind a
    long triad so the launches are back to back on the device, divided by the number of buffers.
    ``padded=True`` times the other route instead: A zero-padded to 256 rows through gemm_mxfp4_nt, over the
    same buffers and the same byte count.
    """
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev).manual_seed(m + n + k)
    rand = lambda lo, hi, *shape: torch.randint(lo, hi, shape, device=dev, dtype=torch.uint8, generator=g)  # noqa: E731
    count = (512 << 20) // (n * k // 2) + 1
    weights = [(rand(0, 256, n, k // 2), rand(120, 135, n, k // 32)) for _ in range(count)]
    rows = 256 if padded else m
    a, sa = torch.zeros(rows, k // 2, device=dev, dtype=torch.uint8), rand(120, 135, rows, k // 32)
    a[:m] = rand(0, 256, m, k // 2)
    c = torch.empty(rows, n, device=dev, dtype=torch.bfloat16)
    split = 1 if padded else split_k or skinny_split_k(n, k, dev)
    ws = torch.empty(split * m * n, device=dev, dtype=torch.float32) if split > 1 else None
    x = torch.rand(1 << 28, device=dev)
    y = torch.rand(1 << 28, device=dev)
    z = torch.empty_like(x)

    def one_pass():
        for b, sb in weights:
            if padded:
                gemm_mxfp4_nt(a, b, sa, sb, out=c)
            else:
                gemm_mxfp4_skinny_nt(a, b, sa, sb, out=c, split_k=split, workspace=ws)

    one_pass()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream_triad(x, y, 0.5, out=z)  # ~0.6 ms: the pass below is enqueued before the device reaches it
        s.record()
        one_pass()
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3 / count)
    times.sort()
    moved = n * k // 2 + n * k // 32 + m * k // 2 + m * k // 32 + m * n * 2
    return moved / times[len(times) // 2] / 1e12


def time_attn_decode(b: int, hkv: int, g: int, s: int, iters: int = 20, split_kv: int = 0, sdpa: bool = False,
                     device: int = 0, lens=None) -> float:
    """Median TB/s of attn_decode_bf16 over the bytes it must move: the K and V rows below each length, q and out.

    Built like :func:`time_gemm_skinny`: the caches rotate over enough distinct K+V pairs to exceed 512 MiB when
    one pair is smaller, a sample is one pass over all pairs between two events, enqueued behind a long triad,
    divided by the number of pairs. ``lens`` (default: all ``s``) gives a ragged batch. ``sdpa=True`` times the
    other route instead, over the same buffers and the same byte count:
    ``torch.nn.functional.scaled_dot_product_attention`` on the same tensors with ``enable_gqa=True``, which
    expands the KV heads to the query heads as that function requires, and, for a ragged batch, a boolean key mask.
    """
    dev = torch.device("cuda", device)
    gen = torch.Generator(device=dev).manual_seed(b + hkv + g + s)
    pair = 2 * b * hkv * s * 256
    count = (512 << 20) // pair + 1 if pair < (512 << 20) else 1
    caches = [[torch.randn(b, hkv, s, 128, device=dev, dtype=torch.bfloat16, generator=gen) for _ in range(2)]
              for _ in range(count)]
    q = torch.randn(b, hkv * g, 128, device=dev, dtype=torch.bfloat16, generator=gen)
    out = torch.empty_like(q)
    lens_list = [s] * b if lens is None else list(lens)
    seq_lens = torch.tensor(lens_list, device=dev, dtype=torch.int32)
    split = split_kv or attn_split_kv(b, hkv, s, dev)
    ws = torch.empty(split * b * hkv * g * 130, device=dev, dtype=torch.float32) if split > 1 else None
    mask = None if lens is None else (torch.arange(s, device=dev)[None, :] < seq_lens[:, None])[:, None, None, :]
    x, y, z = (torch.rand(1 << 28, device=dev) for _ in range(3))

    def one_pass():
        for k, v in caches:
            if sdpa:
                torch.nn.functional.scaled_dot_product_attention(q[:, :, None], k, v, attn_mask=mask, enable_gqa=True)
            else:
                attn_decode_bf16(q, k, v, seq_lens, out=out, split_kv=split, workspace=ws)

    one_pass()
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream_triad(x, y, 0.5, out=z)  # ~0.6 ms: the pass below is enqueued before the device reaches it
        t0.record()
        one_pass()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / 1e3 / count)
    times.sort()
    moved = 2 * hkv * 256 * sum(lens_list) + 2 * b * hkv * g * 256
    return moved / times[len(times) // 2] / 1e12


def time_triad(mb: int = 2048, iters: int = 20, device: int = 0) -> float:
    """Median TB/s of stream_triad over ``mb`` MB per vector (3 streams of traffic)."""
    dev = torch.device("cuda", device)
    n = (mb * 1024 * 1024 // 4) // 4 * 4
    x = torch.rand(n, device=dev)
    y = torch.rand(n, device=dev)
    z = torch.empty_like(x)
    for _ in range(3):
        stream_triad(x, y, 0.5, out=z)
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        stream_triad(x, y, 0.5, out=z)
        e.record()
        e.synchronize()
        times.append(s.elapsed_time(e) / 1e3)
    times.sort()
    return 3 * n * 4 / times[len(times) // 2] / 1e12

