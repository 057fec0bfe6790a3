"""Prefill attention on the MI355X (native: ops/kernels/attn_prefill.h, part of ``_workload``) with torch tensors.

* :func:`attn_prefill_bf16` — causal ``softmax(q·Kᵀ)·V`` of a prompt, or a chunk of one, over the bf16 KV cache
  that :func:`workload.attn_decode_bf16` reads: grouped query heads, a ragged batch as left-padded queries, no mask
  tensor; K and V tiles shared by a block's waves through LDS
* :func:`time_attn_prefill` — its rate, and that of ``scaled_dot_product_attention`` on the same tensors
* :func:`kv_append_fp8`, :func:`attn_decode_fp8` — the FP8 KV cache (native: ops/kernels/attn_decode_fp8.h): the
  kernel that quantises new K/V rows into it and decode attention over it, 129 bytes per cached row for the bf16
  cache's 256; :func:`attn_fp8_split_kv`, :func:`time_attn_decode_fp8`

Shapes are validated on the host before any launch; there is no PyTorch fallback.

FP8 KV-cache format (the contract between :func:`kv_append_fp8`, :func:`attn_decode_fp8` and any other writer):

* ``k_cache``, ``v_cache``: [B, Hkv, S_max, 128] ``torch.float8_e4m3fn`` (OCP "fn", as ``gemm_mxfp8_nt``), contiguous;
* ``k_scale``, ``v_scale``: [B, Hkv, S_max] ``uint8`` E8M0, contiguous: row s of head h means
  ``e4m3 · 2^(byte − 127)``, one power-of-two scale per token and KV head;
* ``S_max % 4 == 0`` (a lane's four scale bytes are one aligned dword).

A bf16 row ``x[0..127]`` is quantised, in exact arithmetic, as ``amax = max|x|``, ``X = floor(log2 amax) − 8``,
``X += 1`` if ``amax · 2^−X > 448``; the scale byte is ``X + 127`` clamped to [1, 254] (127 for an all-zero row), so
``float(byte << 23)`` is the scale and no NaN code is written; the elements are ``RNE_e4m3(x · 2^−X)`` with the sign
kept (−0 stays −0). Nothing exceeds 448, so nothing saturates (``quantize_mxfp8`` saturates the (448, 512) band).
"""
from __future__ import annotations

from typing import Optional

import torch

from .workload import _stream_handle, attn_decode_bf16, attn_split_kv, native, stream_triad


def attn_prefill_bf16(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, seq_lens: torch.Tensor,
                      out: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                      scale: Optional[float] = None) -> torch.Tensor:
    """out[b,i,h] = Σ_s softmax_s(scale · q[b,i,h]·k_cache[b,h//G,s]) · v_cache[b,h//G,s] over s ≤ seq_lens[b] − Sq + i.

    ``q`` [B,Sq,Hq,128] (the view of a projection's [B·Sq, Hq·128] output) and the caches [B,Hkv,S_max,128] are
    contiguous bfloat16, ``seq_lens`` [B] int32 with 1 ≤ len ≤ S_max: the number of valid keys, the chunk's own
    included, which are already in the cache. Hq = G·Hkv for any G ≥ 1; ``scale`` defaults to 128^-½. Accumulation
    is fp32, the result [B,Sq,Hq,128] bfloat16, bit-identical from run to run.

    The causal mask is bottom-right aligned: query row i sits at position ``seq_lens[b] − Sq + i`` and attends the
    keys up to it. ``seq_lens == Sq`` is a plain causal prefill, ``seq_lens > Sq`` a chunk of a longer prompt, and
    with ``seq_lens[b] < Sq`` the first ``Sq − len`` rows are left padding whose output is exactly 0, so a ragged
    batch of prompts is one call. B ≤ 65535; each cache and ``q`` must be smaller than 2^32 bytes; ``q``, the
    caches and ``out`` must be 16-byte aligned.
    """
    if any(t.dtype != torch.bfloat16 for t in (q, k_cache, v_cache)):
        raise TypeError("attn_prefill_bf16 expects bfloat16 q, k_cache and v_cache")
    if q.dim() != 4 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape or q.shape[0] != k_cache.shape[0]:
        raise ValueError(f"shape mismatch: q{tuple(q.shape)} k_cache{tuple(k_cache.shape)} v_cache"
                         f"{tuple(v_cache.shape)} (need q[B,Sq,Hq,128], caches [B,Hkv,S_max,128])")
    b, sq, hq, d = q.shape
    hkv, s_max = k_cache.shape[1], k_cache.shape[2]
    if d != 128 or k_cache.shape[3] != 128:
        raise ValueError(f"attn_prefill_bf16 needs head dim 128 (got {d} and {k_cache.shape[3]})")
    if b == 0 or sq == 0 or hkv == 0 or s_max == 0 or hq == 0 or hq % hkv:
        raise ValueError(f"Hq must be a positive multiple of Hkv, B, Sq and S_max positive (got Hq {hq}, Hkv {hkv}, "
                         f"B {b}, Sq {sq}, S_max {s_max})")
    if b > 65535 or b * hkv * s_max * 256 >= 2 ** 32 or b * sq * hq * 256 >= 2 ** 32:
        raise ValueError("attn_prefill_bf16 needs B <= 65535, caches (B*Hkv*S_max*256) and q (B*Sq*Hq*256) smaller "
                         "than 2^32 bytes")
    if seq_lens.dtype != torch.int32:
        raise TypeError("seq_lens must be int32")
    if seq_lens.shape != (b,):
        raise ValueError(f"seq_lens must be [{b}], got {tuple(seq_lens.shape)}")
    if not (q.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()):
        raise ValueError("q, k_cache and v_cache must be contiguous")
    if not all(t.is_cuda and t.device == q.device for t in (q, k_cache, v_cache, seq_lens)):
        raise ValueError("q, k_cache, v_cache and seq_lens must be on the same GPU")
    seq_lens = seq_lens.contiguous()
    if out is None:
        out = torch.empty_like(q)
    elif out.shape != q.shape or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != q.device:
        raise ValueError("out must be a contiguous bfloat16 [B,Sq,Hq,128] tensor on q's device")
    native().attn_prefill_bf16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), seq_lens.data_ptr(),
                               out.data_ptr(), b, hkv, hq // hkv, sq, s_max,
                               float(scale if scale is not None else 128 ** -0.5), _stream_handle(stream, q.device))
    return out


def time_attn_prefill(b: int, hkv: int, g: int, sq: int, s: Optional[int] = None, lens=None, iters: int = 20,
                      sdpa: bool = False, device: int = 0) -> float:
    """Median TFLOP/s of attn_prefill_bf16 over 4·128 flops per visible (query, key) pair and query head.

    ``s`` is the cache length (default ``sq``), ``lens`` the valid keys per sequence (default all ``s``): ``s > sq``
    is a chunk at the end of a longer prompt, ``lens`` below ``sq`` a ragged batch of left-padded prompts. Built
    like :func:`workload.time_attn_decode`: q, the caches and out rotate over enough distinct sets to exceed
    512 MiB when one set is smaller, a sample is one pass over all sets between two events, enqueued behind a long
    triad, divided by the number of sets. ``sdpa=True`` times the other route instead, over the same tensors and
    the same flop count: ``torch.nn.functional.scaled_dot_product_attention(..., enable_gqa=True)`` on transposed
    views, with ``is_causal=True`` where every length equals ``sq`` and ``s == sq``; a chunked or ragged point is
    outside what ``is_causal`` expresses, so there the boolean mask [B,1,Sq,S] that route needs is built once,
    outside the timed region, and passed as ``attn_mask`` (rows of left padding come back NaN from that route).
    """
    dev = torch.device("cuda", device)
    s = sq if s is None else s
    lens_list = [s] * b if lens is None else list(lens)
    if len(lens_list) != b or not all(1 <= n <= s for n in lens_list):
        raise ValueError(f"lens must be {b} lengths in 1..{s}")
    # Row i of a sequence of n keys sees max(n - sq + i + 1, 0) of them.
    pairs = sum(sq * (n - sq) + sq * (sq + 1) // 2 if n >= sq else n * (n + 1) // 2 for n in lens_list)
    gen = torch.Generator(device=dev).manual_seed(b + hkv + g + sq + s)
    one = 2 * b * sq * hkv * g * 256 + 2 * b * hkv * s * 256
    count = (512 << 20) // one + 1 if one < (512 << 20) else 1
    rand = lambda *shape: torch.randn(*shape, device=dev, dtype=torch.bfloat16, generator=gen)  # noqa: E731
    sets = [(rand(b, sq, hkv * g, 128), rand(b, hkv, s, 128), rand(b, hkv, s, 128)) for _ in range(count)]
    out = torch.empty_like(sets[0][0])
    seq_lens = torch.tensor(lens_list, device=dev, dtype=torch.int32)
    square = s == sq and all(n == sq for n in lens_list)
    mask = None
    if sdpa and not square:
        pos = seq_lens[:, None] - sq + torch.arange(sq, device=dev)[None, :]
        mask = (torch.arange(s, device=dev)[None, None, :] <= pos[:, :, None])[:, None]
    x, y, z = (torch.rand(1 << 28, device=dev) for _ in range(3))

    def one_pass():
        for q, k, v in sets:
            if sdpa:
                torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k, v, attn_mask=mask,
                                                                 is_causal=square, enable_gqa=True)
            else:
                attn_prefill_bf16(q, k, v, seq_lens, out=out)

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
    return 4 * 128 * pairs * hkv * g / times[len(times) // 2] / 1e12


#: ``split_kv=0`` of :func:`attn_decode_fp8` keeps B·Hkv·split_kv at or below the CU count and every slice at least
#: ``ATTN_FP8_MIN_SLICE`` keys long (measured: profiles/attn_decode_fp8_ab.md).
ATTN_FP8_MIN_SLICE = 1024


def attn_fp8_split_kv(b: int, hkv: int, s_max: int, device) -> int:
    """The split ``attn_decode_fp8`` picks for ``split_kv=0``: the largest that keeps B·Hkv·split at or below the
    device's CU count and leaves every slice of an ``s_max``-long sequence at least ``ATTN_FP8_MIN_SLICE`` keys.
    It looks at ``s_max``, not at the lengths, so it needs no device sync."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(1, min(cus // (b * hkv), s_max // ATTN_FP8_MIN_SLICE))


def _check_fp8_cache(name: str, k_cache, v_cache, k_scale, v_scale, seq_lens, b: int):
    """The refusals the two FP8-cache functions share, in the order dtype, shape, limits; returns (Hkv, S_max)."""
    if k_cache.dtype != torch.float8_e4m3fn or v_cache.dtype != torch.float8_e4m3fn:
        raise TypeError(f"{name} expects float8_e4m3fn k_cache and v_cache")
    if k_scale.dtype != torch.uint8 or v_scale.dtype != torch.uint8:
        raise TypeError(f"{name} expects uint8 (E8M0) k_scale and v_scale")
    if seq_lens.dtype != torch.int32:
        raise TypeError("seq_lens must be int32")
    if (k_cache.dim() != 4 or v_cache.shape != k_cache.shape or k_cache.shape[0] != b
            or k_scale.shape != k_cache.shape[:3] or v_scale.shape != k_cache.shape[:3]):
        raise ValueError(f"shape mismatch: k_cache{tuple(k_cache.shape)} v_cache{tuple(v_cache.shape)} k_scale"
                         f"{tuple(k_scale.shape)} v_scale{tuple(v_scale.shape)} (need caches [{b},Hkv,S_max,128], "
                         f"scales [{b},Hkv,S_max])")
    hkv, s_max, d = k_cache.shape[1:]
    if d != 128:
        raise ValueError(f"{name} needs head dim 128 (got {d})")
    if b == 0 or hkv == 0 or s_max == 0 or s_max % 4:
        raise ValueError(f"B and Hkv must be positive, S_max a positive multiple of 4 (got B {b}, Hkv {hkv}, "
                         f"S_max {s_max})")
    if b > 65535 or b * hkv * s_max * 128 >= 2 ** 32:
        raise ValueError(f"{name} needs B <= 65535 and caches smaller than 2^32 bytes (B*Hkv*S_max*128)")
    if seq_lens.shape != (b,):
        raise ValueError(f"seq_lens must be [{b}], got {tuple(seq_lens.shape)}")
    if not all(t.is_contiguous() for t in (k_cache, v_cache, k_scale, v_scale)):
        raise ValueError("k_cache, v_cache, k_scale and v_scale must be contiguous")
    return hkv, s_max


def kv_append_fp8(k_new: torch.Tensor, v_new: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                  k_scale: torch.Tensor, v_scale: torch.Tensor, seq_lens: torch.Tensor,
                  stream: Optional[torch.cuda.Stream] = None) -> None:
    """Quantise new K and V rows into the FP8 KV cache (format and rule: this module's docstring), in place.

    ``k_new``, ``v_new`` [B,Sq,Hkv,128] contiguous bfloat16 (the view of a projection's output; Sq = 1 is a decode
    step), finite. ``seq_lens`` [B] int32 counts the new rows as already included, as :func:`attn_prefill_bf16`
    takes it: row i of sequence b goes to position ``seq_lens[b] − Sq + i``; rows of negative position are left
    padding and are skipped, as are positions at or past S_max. K and V are done in one launch; no other byte of
    the caches or scales changes. ``k_new`` and ``v_new`` must be 16-byte, the caches 8-byte aligned.
    """
    if k_new.dtype != torch.bfloat16 or v_new.dtype != torch.bfloat16:
        raise TypeError("kv_append_fp8 expects bfloat16 k_new and v_new")
    if k_new.dim() != 4 or v_new.shape != k_new.shape:
        raise ValueError(f"shape mismatch: k_new{tuple(k_new.shape)} v_new{tuple(v_new.shape)} (need [B,Sq,Hkv,128])")
    b, sq, hkv_new, d = k_new.shape
    if d != 128:
        raise ValueError(f"kv_append_fp8 needs head dim 128 (got {d})")
    hkv, s_max = _check_fp8_cache("kv_append_fp8", k_cache, v_cache, k_scale, v_scale, seq_lens, b)
    if hkv_new != hkv or sq == 0 or b * sq * hkv >= 2 ** 31:
        raise ValueError(f"k_new must be [B,Sq,{hkv},128] with 0 < B*Sq*Hkv < 2^31 (got {tuple(k_new.shape)})")
    if not (k_new.is_contiguous() and v_new.is_contiguous()):
        raise ValueError("k_new and v_new must be contiguous")
    tensors = (k_new, v_new, k_cache, v_cache, k_scale, v_scale, seq_lens)
    if not all(t.is_cuda and t.device == k_new.device for t in tensors):
        raise ValueError("k_new, v_new, the caches, the scales and seq_lens must be on the same GPU")
    seq_lens = seq_lens.contiguous()
    native().kv_append_fp8(k_new.data_ptr(), v_new.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                           k_scale.data_ptr(), v_scale.data_ptr(), seq_lens.data_ptr(), b, sq, hkv, s_max,
                           _stream_handle(stream, k_new.device))


def attn_decode_fp8(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k_scale: torch.Tensor,
                    v_scale: torch.Tensor, seq_lens: torch.Tensor, out: Optional[torch.Tensor] = None,
                    stream: Optional[torch.cuda.Stream] = None, split_kv: int = 0,
                    workspace: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """:func:`workload.attn_decode_bf16` over the FP8 KV cache (format: this module's docstring).

    out[b,h] = Σ_s softmax_s(scale · q[b,h]·K[b,h//G,s]) · V[b,h//G,s] over s < seq_lens[b], K and V the dequantised
    caches ``e4m3 · 2^(scale byte − 127)``. Dequantisation to bf16 is exact and the arithmetic is the bf16 kernel's
    (bf16 MFMA operands, fp32 softmax and accumulation), so the result has that kernel's error bound on the
    dequantised cache. ``q`` and ``out`` [B,Hq,128] bfloat16, Hq = G·Hkv with 1 ≤ G ≤ 16, ``seq_lens`` [B] int32
    with 1 ≤ len ≤ S_max; every row below a length must have been written (scale bytes 1..254), rows and scale
    bytes past it may hold anything. ``split_kv`` (0: :func:`attn_fp8_split_kv`), ``workspace`` (float32, at least
    split_kv·B·Hq·130 elements) and the ordered merge are attn_decode_bf16's: bit-identical from run to run.
    B ≤ 65535, a cache smaller than 2^32 bytes; ``q``, the caches, ``out`` and ``workspace`` 16-byte, the scales
    4-byte aligned.
    """
    if q.dtype != torch.bfloat16:
        raise TypeError("attn_decode_fp8 expects bfloat16 q")
    if q.dim() != 3:
        raise ValueError(f"shape mismatch: q{tuple(q.shape)} (need q[B,Hq,128])")
    b, hq, d = q.shape
    if d != 128:
        raise ValueError(f"attn_decode_fp8 needs head dim 128 (got {d})")
    hkv, s_max = _check_fp8_cache("attn_decode_fp8", k_cache, v_cache, k_scale, v_scale, seq_lens, b)
    if hq == 0 or hq % hkv:
        raise ValueError(f"Hq must be a positive multiple of Hkv (got Hq {hq}, Hkv {hkv})")
    g = hq // hkv
    if g > 16:
        raise ValueError(f"attn_decode_fp8 needs Hq/Hkv <= 16 (got {g})")
    if not 0 <= split_kv <= 65535:
        raise ValueError(f"split_kv in 0..65535, got {split_kv}")
    if not all(t.is_cuda and t.device == q.device for t in (q, k_cache, v_cache, k_scale, v_scale, seq_lens)):
        raise ValueError("q, the caches, the scales and seq_lens must be on the same GPU")
    q, seq_lens = q.contiguous(), seq_lens.contiguous()
    if out is None:
        out = torch.empty((b, hq, 128), dtype=torch.bfloat16, device=q.device)
    elif out.shape != (b, hq, 128) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != q.device:
        raise ValueError("out must be a contiguous bfloat16 [B,Hq,128] tensor on q's device")
    split_kv = split_kv or attn_fp8_split_kv(b, hkv, s_max, q.device)
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
    native().attn_decode_fp8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                             v_scale.data_ptr(), seq_lens.data_ptr(), out.data_ptr(), b, hkv, g, s_max,
                             float(scale if scale is not None else 128 ** -0.5), split_kv,
                             workspace.data_ptr() if workspace is not None else 0,
                             workspace.numel() * 4 if workspace is not None else 0, int(s.cuda_stream))
    return out


def dequantize_fp8_cache(cache: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The bf16 cache an FP8 cache stands for: ``e4m3 · 2^(byte − 127)``, exact for scale bytes near 127."""
    return (cache.float() * torch.exp2(scale.float() - 127.0)[..., None]).bfloat16()


def time_attn_decode_fp8(b: int, hkv: int, g: int, s: int, lens=None, iters: int = 20, split_kv: int = 0,
                         bf16: bool = False, device: int = 0):
    """(seconds per call, TB/s): medians for attn_decode_fp8 over the bytes it must move, the rows below each length
    at 129 bytes in K and in V, q and out.

    Built like :func:`workload.time_attn_decode`: N(0,1) K and V rows are written by :func:`kv_append_fp8`, the
    caches rotate over enough distinct sets to exceed 512 MiB when one set is smaller, a sample is one pass over
    all sets between two events, enqueued behind a long triad, divided by the number of sets. ``bf16=True`` times
    ``attn_decode_bf16`` instead, on the dequantised copies of the same caches with its own automatic split, and
    counts 256 bytes per row.
    """
    dev = torch.device("cuda", device)
    gen = torch.Generator(device=dev).manual_seed(b + hkv + g + s)
    lens_list = [s] * b if lens is None else list(lens)
    if len(lens_list) != b or not all(1 <= n <= s for n in lens_list):
        raise ValueError(f"lens must be {b} lengths in 1..{s}")
    one = 2 * b * hkv * s * 129
    count = (512 << 20) // one + 1 if one < (512 << 20) else 1
    full = torch.full((b,), s, device=dev, dtype=torch.int32)
    sets = []
    for _ in range(count):
        kc, vc = (torch.empty(b, hkv, s, 128, device=dev, dtype=torch.float8_e4m3fn) for _ in range(2))
        ks, vs = (torch.empty(b, hkv, s, device=dev, dtype=torch.uint8) for _ in range(2))
        kn, vn = (torch.randn(b, s, hkv, 128, device=dev, dtype=torch.bfloat16, generator=gen) for _ in range(2))
        kv_append_fp8(kn, vn, kc, vc, ks, vs, full)
        sets.append((dequantize_fp8_cache(kc, ks), dequantize_fp8_cache(vc, vs)) if bf16 else (kc, vc, ks, vs))
        del kn, vn
    q = torch.randn(b, hkv * g, 128, device=dev, dtype=torch.bfloat16, generator=gen)
    out = torch.empty_like(q)
    seq_lens = torch.tensor(lens_list, device=dev, dtype=torch.int32)
    split = split_kv or (attn_split_kv if bf16 else attn_fp8_split_kv)(b, hkv, s, dev)
    ws = torch.empty(split * b * hkv * g * 130, device=dev, dtype=torch.float32) if split > 1 else None
    x, y, z = (torch.rand(1 << 28, device=dev) for _ in range(3))

    def one_pass():
        for c in sets:
            if bf16:
                attn_decode_bf16(q, c[0], c[1], seq_lens, out=out, split_kv=split, workspace=ws)
            else:
                attn_decode_fp8(q, c[0], c[1], c[2], c[3], seq_lens, out=out, split_kv=split, workspace=ws)

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
    sec = times[len(times) // 2]
    moved = 2 * hkv * (256 if bf16 else 129) * sum(lens_list) + 2 * b * hkv * g * 256
    return sec, moved / sec / 1e12
