"""GPU tests of the FP8 KV cache (kv_append_fp8, attn_decode_fp8) against plain torch: the quantisation rule written
out on the CPU, and float64 attention on the dequantised cache."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import attention  # noqa: E402

E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _dequant(cache, scale):
    return cache.float().double() * torch.exp2(scale.double() - 127.0)[..., None]


def _reference(q, k, v, lens, scale):
    """(softmax(scale·q·kᵀ)·v, softmax·|v|) over s < len in float64 on dequantised k, v; both [B,Hq,128]."""
    b, hkv, s_max, _ = k.shape
    live = torch.arange(s_max, device=q.device)[None, :] < lens[:, None]
    k, v = (torch.where(live[:, None, :, None], t, 0.0) for t in (k, v))  # past len: NaN codes, never attended
    scores = scale * (q.double().view(b, hkv, -1, 128) @ k.transpose(2, 3))  # [B,Hkv,G,S]
    p = scores.masked_fill(~live[:, None, None, :], float("-inf")).softmax(dim=-1)
    return (p @ v).view(q.shape), (p @ v.abs()).view(q.shape)


def _quantise_rows(x):
    """The cache format's rule on the CPU: x [..., 128] bf16 → (e4m3 bytes, E8M0 bytes)."""
    x = x.double().cpu()
    amax = x.abs().amax(-1)
    _, exp = torch.frexp(amax)  # amax = m·2^exp, ½ ≤ m < 1: floor(log2 amax) = exp − 1
    big = exp - 9
    big = big + (amax * torch.pow(2.0, -big.double()) > 448).int()
    byte = torch.where(amax == 0, 127, (big + 127).clamp(1, 254))
    q = (x * torch.pow(2.0, (127 - byte).double())[..., None]).float().to(E4M3)
    return q.view(torch.uint8), byte.to(torch.uint8)


@pytest.mark.parametrize("b,hkv,sq,s_max,lens", [(1, 1, 1, 64, [1]), (2, 2, 1, 64, [64, 17]),
                                                 (2, 1, 40, 128, [128, 25])])  # the last: 15 rows of left padding
def test_kv_append_fp8_bit_exact(dev, b, hkv, sq, s_max, lens):
    gen = torch.Generator(device=dev).manual_seed(s_max + sq)
    new = []
    for _ in range(2):
        x = torch.randn(b * sq * hkv, 128, device=dev, generator=gen)
        x = x * torch.exp2(torch.randint(-20, 21, (x.shape[0], 1), device=dev, generator=gen).float())
        new.append(x.bfloat16())
    k_new, v_new = new
    if k_new.shape[0] >= 4:  # the last rows are never padding
        k_new[-1] = 0.0
        k_new[-2] = torch.rand(128, device=dev, generator=gen) - 0.5
        k_new[-2, 5] = 480.0  # 1.875·2^8: X bumps to 1, 480 → 240
        v_new[-1] = torch.rand(128, device=dev, generator=gen) - 0.5
        v_new[-1, 7] = -448.0  # 1.75·2^8: no bump, the largest e4m3
        v_new[-2] = 0.0
        v_new[-2, :4] = torch.tensor([256.0, 17.0, 19.0, -0.0])  # X = 0; ties 17 → 16, 19 → 20; −0 stays −0
    k_new, v_new = (t.view(b, sq, hkv, 128) for t in (k_new, v_new))
    caches = [torch.full((b, hkv, s_max, 128), 0x5A, device=dev, dtype=torch.uint8) for _ in range(2)]
    scales = [torch.full((b, hkv, s_max), 0x5A, device=dev, dtype=torch.uint8) for _ in range(2)]
    want_c, want_s = [t.cpu().clone() for t in caches], [t.cpu().clone() for t in scales]
    for new, wc, ws in zip((k_new, v_new), want_c, want_s):
        qb, sb = _quantise_rows(new)
        for bi, n in enumerate(lens):
            lo = max(sq - n, 0)  # rows below lo have a negative position
            wc[bi, :, n - sq + lo:n] = qb[bi, lo:].transpose(0, 1)
            ws[bi, :, n - sq + lo:n] = sb[bi, lo:].transpose(0, 1)
    attention.kv_append_fp8(k_new, v_new, caches[0].view(E4M3), caches[1].view(E4M3), scales[0], scales[1],
                            torch.tensor(lens, device=dev, dtype=torch.int32))
    for got, want in zip(caches + scales, want_c + want_s):
        assert torch.equal(got.cpu(), want)
    if sq == 40:  # the rule's corners, spelled out
        assert want_s[0][1, 0, 23:25].tolist() == [128, 127] and want_c[1][1, 0, 24, 7].item() == 0xFE
        assert want_c[1][1, 0, 23, :4].tolist() == [0x78, 0x58, 0x5A, 0x80]


@pytest.mark.parametrize("b,hkv,g,s_max,lens,split_kv", [(1, 1, 1, 64, [1], 1), (2, 2, 8, 512, [512, 333], 1),
                                                         (3, 1, 16, 1024, [1024, 129, 1], 4),
                                                         (2, 2, 5, 2048, [2047, 700], 8), (1, 1, 3, 256, [200], 2)])
def test_attn_decode_fp8_one_hot_exact(dev, b, hkv, g, s_max, lens, split_kv):
    # As test_attn_decode_one_hot_exact: head h asks for coordinate h mod G and exactly one key below len, at t(b,h),
    # has it (dequantised 16, so the score is 256 and every other 0): out[b,h] is the dequantised V row at t bit for
    # bit, which pins the V transposing read, the key order of P and both scale paths. Past len everything is NaN codes.
    hq = hkv * g
    gen = torch.Generator(device=dev).manual_seed(s_max + g)
    q = torch.zeros(b, hq, 128, device=dev, dtype=torch.bfloat16)
    kb = torch.zeros(b, hkv, s_max, 128, device=dev, dtype=torch.uint8)
    vb = torch.randint(0, 254, (b, hkv, s_max, 128), device=dev, generator=gen).to(torch.uint8)
    vb = vb + (vb >= 0x7F).to(torch.uint8)  # any byte but 0x7F and 0xFF
    # K's scale bytes 123..134 keep the spot's e4m3 code, 2^(131 − byte), a normal number (2^8 .. 2^-3)
    ks, vs = (torch.randint(lo, 135, (b, hkv, s_max), device=dev, generator=gen).to(torch.uint8) for lo in (123, 120))
    want = torch.empty(b, hq, 128, device=dev, dtype=torch.bfloat16)
    for bi, n in enumerate(lens):
        kb[bi, :, n:], vb[bi, :, n:], ks[bi, :, n:], vs[bi, :, n:] = 0x7F, 0xFF, 0xFF, 0xFF
        edge = 64 * -(-(-(-n // 64)) // split_kv)  # first key of the second slice: 64·⌈⌈n/64⌉/split⌉
        # 0, the last key, both sides of the slice edge, of a lane's 4 keys, a 16-key sub-tile, a 64-key wave tile and
        # a 256-key round of the four waves
        spots = [min(t, n - 1) for t in (0, n - 1, edge, edge - 1, 4, 3, 16, 15, 64, 63, 256, 255, n // 2)]
        for h in range(hq):
            t = spots[(h + bi) % len(spots)]
            q[bi, h, h % g] = 16.0
            kb[bi, h // g, t, h % g] = (138 - ks[bi, h // g, t]) << 3  # e4m3 2^(131 − scale byte): dequantised 16
            want[bi, h] = _dequant(vb[bi, h // g, t].view(E4M3), vs[bi, h // g, t]).bfloat16()
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    buf = torch.full((b + 1, hq, 128), -7.0, device=dev, dtype=torch.bfloat16)
    out = attention.attn_decode_fp8(q, kb.view(E4M3), vb.view(E4M3), ks, vs, seq_lens, out=buf[:b],
                                    split_kv=split_kv, scale=1.0)
    ref = _reference(q, _dequant(kb.view(E4M3), ks), _dequant(vb.view(E4M3), vs), seq_lens, 1.0)[0]
    assert torch.equal(ref.float().bfloat16(), want)
    assert not out.isnan().any()
    assert torch.equal(out, want), (out.double() - want.double()).abs().max().item()
    assert (buf[b:] == -7.0).all()


@pytest.mark.parametrize("b,hkv,g,s_max,lens", [(2, 2, 8, 1536, [1536, 777]), (4, 1, 4, 4096, [4096, 3000, 65, 1])])
def test_attn_decode_fp8_random(dev, b, hkv, g, s_max, lens):
    gen = torch.Generator(device=dev).manual_seed(s_max)
    q = torch.randn(b, hkv * g, 128, device=dev, generator=gen).bfloat16()
    k_new = torch.randn(b, s_max, hkv, 128, device=dev, generator=gen).bfloat16()
    v_new = torch.randn(b, s_max, hkv, 128, device=dev, generator=gen)
    v_new = (v_new * torch.exp2(torch.randint(-3, 4, v_new.shape, device=dev, generator=gen).float())).bfloat16()
    seq_lens = torch.tensor(lens, device=dev, dtype=torch.int32)
    # Caches of NaN codes; the append writes the last len rows of each sequence below len and skips the rest.
    kc, vc = (torch.full((b, hkv, s_max, 128), 0x7F, device=dev, dtype=torch.uint8).view(E4M3) for _ in range(2))
    ks, vs = (torch.full((b, hkv, s_max), 0xFF, device=dev, dtype=torch.uint8) for _ in range(2))
    attention.kv_append_fp8(k_new, v_new, kc, vc, ks, vs, seq_lens)
    out = attention.attn_decode_fp8(q, kc, vc, ks, vs, seq_lens, split_kv=0)
    ref, ref_abs = _reference(q, _dequant(kc, ks), _dequant(vc, vs), seq_lens, 128 ** -0.5)
    # attn_decode_bf16's bound, unchanged: dequantisation is exact, P is rounded to bf16 once per term in the
    # numerator and in the sum (2^-9 each), bf16 output rounding (2^-9), fp32 accumulation below that.
    tol = 2.0 ** -7 * ref.abs() + 2.0 ** -8 * ref_abs
    err = (out.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()
    assert torch.equal(out, attention.attn_decode_fp8(q, kc, vc, ks, vs, seq_lens, split_kv=0))  # bit-identical
