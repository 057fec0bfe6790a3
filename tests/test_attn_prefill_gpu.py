"""GPU tests of prefill attention (attention.attn_prefill_bf16) against plain torch in float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import attention  # noqa: E402

SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _positions(lens, sq):
    """[B,Sq]: position of query row i of sequence b, seq_lens[b] − Sq + i (negative: left padding)."""
    return lens.long()[:, None] - sq + torch.arange(sq, device=lens.device)[None, :]


def _reference(q, k, v, lens, scale):
    """(softmax(scale·q·kᵀ)·v, softmax·|v|) over s ≤ position in float64, 0 where no key is visible; [B,Sq,Hq,128]."""
    b, sq, hq, _ = q.shape
    hkv, s_max = k.shape[1], k.shape[2]
    qd = q.double().view(b, sq, hkv, hq // hkv, 128).permute(0, 2, 3, 1, 4)  # [B,Hkv,G,Sq,128]
    scores = scale * (qd @ k.double()[:, :, None].transpose(-1, -2))  # [B,Hkv,G,Sq,S]
    dead = torch.arange(s_max, device=q.device)[None, None, :] > _positions(lens, sq)[:, :, None]
    p = scores.masked_fill(dead[:, None, None], float("-inf")).softmax(dim=-1).nan_to_num(0.0)
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(b, sq, hq, 128)  # noqa: E731
    return back(p @ v.double()[:, :, None]), back(p @ v.double().abs()[:, :, None])


@pytest.mark.parametrize("b,hkv,g,sq,s_max,lens", [(1, 1, 1, 1, 64, [1]), (2, 2, 3, 200, 320, [320, 150]),
                                                   (1, 1, 8, 129, 129, [129]), (2, 1, 5, 64, 1024, [1000, 65])])
def test_attn_prefill_one_hot_exact(dev, b, hkv, g, sq, s_max, lens):
    # Key t holds 16 at coordinates t%32 and 32 + t//32, and the query row that wants key tt holds 16 at tt's two: the
    # wanted key scores 512, a key sharing one coordinate 256, every other 0, so with scale 1 the rivals weigh
    # exp(-256), which is 0 in fp32 and vanishes in float64's rounding to bf16: the row is v[b, h//G, tt] bit for bit.
    # Row i at position p wants tt = max(p - delta, 0), delta cycling through the diagonal, the first key and both
    # sides of a 64-key and a 128-row tile edge. Keys at s >= len would score 2048 and carry a sentinel V.
    hq = hkv * g
    gen = torch.Generator(device=dev).manual_seed(s_max + g)
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    q = torch.zeros(b, sq, hq, 128, device=dev, dtype=torch.bfloat16)
    k = torch.zeros(b, hkv, s_max, 128, device=dev, dtype=torch.bfloat16)
    v = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen).bfloat16()
    t = torch.arange(s_max, device=dev)
    k[:, :, t, t % 32] = 16.0
    k[:, :, t, 32 + t // 32] = 16.0
    want = torch.zeros(b, sq, hq, 128, device=dev, dtype=torch.bfloat16)
    heads = torch.arange(hq, device=dev)
    for bi, n in enumerate(lens):
        k[bi, :, n:] = 64.0
        v[bi, :, n:] = 1000.0
        p = _positions(seq_lens, sq)[bi]
        deltas = torch.stack([0 * p, 0 * p + 1, p, p // 2, p % 64, p % 64 + 1, 0 * p + 63, 0 * p + 64, 0 * p + 127,
                              0 * p + 128], dim=1)  # [Sq,10]
        pick = (heads[None, :] + torch.arange(sq, device=dev)[:, None] + bi) % 10
        tt = (p[:, None] - deltas.gather(1, pick)).clamp_min(0)  # [Sq,Hq]
        q[bi].scatter_(2, (tt % 32)[..., None], 16.0)
        q[bi].scatter_(2, (32 + tt // 32)[..., None], 16.0)
        want[bi] = torch.where((p >= 0)[:, None, None], v[bi][(heads // g)[None, :], tt], want[bi])
    buf = torch.full((b + 1, sq, hq, 128), SENTINEL, device=dev, dtype=torch.bfloat16)
    out = attention.attn_prefill_bf16(q, k, v, seq_lens, out=buf[:b], scale=1.0)
    assert torch.equal(_reference(q, k, v, seq_lens, 1.0)[0].float().bfloat16(), want)
    assert not out.isnan().any()
    assert torch.equal(out, want), (out.double() - want.double()).abs().max().item()
    assert (buf[b:] == SENTINEL).all()


@pytest.mark.parametrize("b,hkv,g,sq,s_max,lens", [(2, 2, 4, 200, 320, [320, 150]), (1, 1, 8, 513, 513, [513]),
                                                   (2, 1, 16, 96, 2048, [2048, 700])])
def test_attn_prefill_random(dev, b, hkv, g, sq, s_max, lens):
    gen = torch.Generator(device=dev).manual_seed(s_max + sq)
    q = torch.randn(b, sq, hkv * g, 128, device=dev, generator=gen).bfloat16()
    k = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(b, hkv, s_max, 128, device=dev, generator=gen)
    v = (v * torch.exp2(torch.randint(-3, 4, v.shape, device=dev, generator=gen).float())).bfloat16()
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    out = attention.attn_prefill_bf16(q, k, v, seq_lens)
    ref, ref_abs = _reference(q, k, v, seq_lens, 128 ** -0.5)
    # The error model of test_attn_decode_random: P rounded to bf16 in numerator and sum (2^-9 per term each), bf16
    # output rounding (2^-9), fp32 accumulation over at most 2048 terms below that: about twice the first-order bound.
    tol = 2.0 ** -7 * ref.abs() + 2.0 ** -8 * ref_abs
    err = (out.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()
    padding = _positions(seq_lens, sq) < 0
    assert (out[padding] == 0).all() and padding.sum().item() == sum(max(sq - n, 0) for n in lens)
    assert torch.equal(out, attention.attn_prefill_bf16(q, k, v, seq_lens))  # no atomics: bit-identical


def test_attn_prefill_refuses_misaligned_out(dev):
    q = torch.zeros(1, 4, 8, 128, device=dev, dtype=torch.bfloat16)
    kv = torch.zeros(1, 1, 64, 128, device=dev, dtype=torch.bfloat16)
    out = torch.empty(q.numel() + 1, device=dev, dtype=torch.bfloat16)[1:].view(q.shape)  # 2-byte offset
    with pytest.raises(RuntimeError):
        attention.attn_prefill_bf16(q, kv, kv, torch.full((1,), 4, device=dev, dtype=torch.int32), out=out)
