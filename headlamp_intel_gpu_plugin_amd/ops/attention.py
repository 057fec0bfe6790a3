"""Prefill attention on the MI355X (native: ops/kernels/attn_prefill.h, part of ``_workload``) with torch tensors.

* :func:`attn_prefill_bf16` — causal ``softmax(q·Kᵀ)·V`` of a prompt, or a chunk of one, over the bf16 KV cache
  that :func:`workload.attn_decode_bf16` reads: grouped query heads, a ragged batch as left-padded queries, no mask
  tensor; K and V tiles shared by a block's waves through LDS
* :func:`time_attn_prefill` — its rate, and that of ``scaled_dot_product_attention`` on the same tensors

Shapes are validated on the host before any launch; there is no PyTorch fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from .workload import _stream_handle, native, stream_triad


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
