"""GPU tests of decode attention (attn_decode_bf16, Burner context=) against plain torch in float64."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import workload  # noqa: E402

SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _reference(q, k, v, lens, scale):
    """(softmax(scale·q·kᵀ)·v, softmax·|v|) over s < len in float64; both [B,Hq,128]."""
    b, hkv, s_max, _ = k.shape
    scores = scale * (q.double().view(b, hkv, -1, 128) @ k.double().transpose(2, 3))  # [B,Hkv,G,S]
    dead = torch.arange(s_max, device=q.device)[None, :] >= lens[:, None]
    p = scores.masked_fill(dead[:, None, None, :], float("-inf")).softmax(dim=-1)
    return (p @ v.double()).view(q.shape), (p @ v.double().abs()).view(q.shape)


@pytest.mark.parametrize("b,hkv,g,s_max,lens,split_kv", [(1, 1, 1, 64, [1], 1), (2, 2, 8, 512, [512, 333], 1),
                                                         (3, 1, 16, 1024, [1024, 129, 1], 4),
                                                         (2, 2, 5, 2048, [2047, 700], 8), (1, 1, 3, 256, [200], 2)])
def test_attn_decode_one_hot_exact(dev, b, hkv, g, s_max, lens, split_kv):
    # Head h asks for coordinate h mod G and exactly one key below len, at t(b,h), has it: that score is 256, every
    # other 0, so the softmax is 1 at t and exp(-256) elsewhere, which vanishes against 1 in fp32 and in float64
    # alike: out[b,h] is v[b,g,t] bit for bit. Keys at s >= len would score 1024 and carry a sentinel V.
    hq = hkv * g
    gen = torch.Generator(device=dev).manual_seed(s_max + g)
    q = torch.zeros(b, hq, 128, device=dev, dtype=torch.bfloat16)
    k = torch.zeros(b, hkv, s_max, 128, device=dev, dtype=torch.bfloat16)
    v = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen).bfloat16()
    want = torch.empty(b, hq, 128, device=dev, dtype=torch.bfloat16)
    for bi, n in enumerate(lens):
        k[bi, :, n:] = 64.0
        v[bi, :, n:] = 1000.0
        edge = 32 * -(-(-(-n // 32)) // split_kv)  # first key of the second slice: 32·⌈⌈n/32⌉/split⌉
        # 0, the last key, both sides of the slice boundary, of a 32-key tile and of a 128-key round of the four waves
        spots = [min(t, n - 1) for t in (0, n - 1, edge, edge - 1, 32, 31, 128, 127, n // 2)]
        for h in range(hq):
            t = spots[(h + bi) % len(spots)]
            q[bi, h, h % g] = 16.0
            k[bi, h // g, t, h % g] = 16.0
            want[bi, h] = v[bi, h // g, t]
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    buf = torch.full((b + 1, hq, 128), SENTINEL, device=dev, dtype=torch.bfloat16)
    out = workload.attn_decode_bf16(q, k, v, seq_lens, out=buf[:b], split_kv=split_kv, scale=1.0)
    assert torch.equal(_reference(q, k, v, seq_lens, 1.0)[0].float().bfloat16(), want)
    assert not out.isnan().any()
    assert torch.equal(out, want), (out.double() - want.double()).abs().max().item()
    assert (buf[b:] == SENTINEL).all()


@pytest.mark.parametrize("b,hkv,g,s_max,lens", [(2, 2, 8, 1536, [1536, 777]), (4, 1, 4, 4096, [4096, 3000, 65, 1])])
def test_attn_decode_random(dev, b, hkv, g, s_max, lens):
    gen = torch.Generator(device=dev).manual_seed(s_max)
    q = torch.randn(b, hkv * g, 128, device=dev, generator=gen).bfloat16()
    k = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen)
    v = (v * torch.exp2(torch.randint(-3, 4, v.shape, device=dev, generator=gen).float())).bfloat16()
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    out = workload.attn_decode_bf16(q, k, v, seq_lens, split_kv=0)
    ref, ref_abs = _reference(q, k, v, seq_lens, 128 ** -0.5)
    # P rounded to bf16 in numerator and sum (2^-9 per term each), bf16 output rounding (2^-9), fp32 accumulation
    # over at most 4096 terms below that: about twice the first-order bound.
    tol = 2.0 ** -7 * ref.abs() + 2.0 ** -8 * ref_abs
    err = (out.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()
    assert torch.equal(out, workload.attn_decode_bf16(q, k, v, seq_lens, split_kv=0))  # no atomics: bit-identical


def test_attn_decode_burner_and_refusal(dev):
    with workload.Burner(device=0, size=1024, gemms=1, triad_mb=16, precision="mxfp4", batch=8, context=512) as b:
        time.sleep(0.5)
    assert b.iterations > 0 and b.error is None
    q = torch.zeros(1, 8, 128, device=dev, dtype=torch.bfloat16)
    kv = torch.zeros(1, 1, 64, 128, device=dev, dtype=torch.bfloat16)
    out = torch.empty(8 * 128 + 1, device=dev, dtype=torch.bfloat16)[1:].view(1, 8, 128)  # 2-byte offset
    with pytest.raises(RuntimeError):
        workload.attn_decode_bf16(q, kv, kv, torch.ones(1, device=dev, dtype=torch.int32), out=out)
