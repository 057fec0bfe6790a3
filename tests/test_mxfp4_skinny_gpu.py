"""GPU tests of the MXFP4 decode path (gemm_mxfp4_skinny_nt, Burner batch=) against plain torch in float64, with the
dequantisation of test_mxfp4_gpu.py: nibble codes through the e2m1 table, scaled by 2^(s−127) per 32 along K."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import workload  # noqa: E402

E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _deq(q, s):
    codes = torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1)  # element 2i: bits 0-3 of byte i
    scale = (s.to(torch.int32) << 23).view(torch.float32).double()  # 2^(s−127) from its bits, exact for s ≥ 1
    return E2M1.to(q.device)[codes.long()] * scale.repeat_interleave(32, dim=1)


def _pack(codes):
    return codes[:, 0::2].to(torch.uint8) | (codes[:, 1::2].to(torch.uint8) << 4)


@pytest.mark.parametrize("m,n,k,split_k", [(1, 128, 256, 1), (16, 128, 512, 2), (17, 256, 768, 3),
                                           (33, 384, 2048, 4), (64, 256, 2048, 8), (64, 128, 1024, 1)])
def test_mxfp4_skinny_exact_scaled(dev, m, n, k, split_k):
    # Operands and scales of test_mxfp4_gemm_exact_scaled: every term is a multiple of 2^-4 and at most 96, so up to
    # K = 2048 every partial and total sum is exact in fp32 in any order and under any split. A wrong lane/k map,
    # scale byte, row clamp, split boundary, reduce order or masked store shows.
    i = torch.arange(m * k, device=dev)
    a = _pack(((i + i // k) % 16).reshape(m, k))  # every code, shifted by one from row to row
    b_sign = ((torch.arange(n * k, device=dev) * 7 + 3) % 3 - 1).reshape(n, k)  # -1, 0, 1
    b = _pack(torch.where(b_sign < 0, 10, b_sign * 2))
    sa = (torch.arange(m * k // 32, device=dev) % 5 + 125).to(torch.uint8).reshape(m, k // 32)
    j = torch.arange(n * k // 32, device=dev)
    sb = ((j * 3 + j // 4 + j // (k // 32)) % 4 + 126).to(torch.uint8).reshape(n, k // 32)
    buf = torch.full((m + 16, n), SENTINEL, device=dev, dtype=torch.bfloat16)
    c = workload.gemm_mxfp4_skinny_nt(a, b, sa, sb, out=buf[:m], split_k=split_k)
    ref = _deq(a, sa) @ _deq(b, sb).T
    assert torch.equal(c, ref.float().bfloat16()), (c.double() - ref).abs().max().item()
    assert (buf[m:] == SENTINEL).all()


def _random_bf16(rows, k, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, k, device=dev, generator=g)
    return (x * torch.exp2(torch.randint(-6, 7, (rows, 1), device=dev, generator=g).float())).bfloat16()


@pytest.mark.parametrize("m,n,k", [(5, 256, 1536), (48, 384, 4096)])
def test_mxfp4_skinny_quantise_then_gemm_random(dev, m, n, k):
    aq, sa = workload.quantize_mxfp4(_random_bf16(m, k, dev, m + k))
    bq, sb = workload.quantize_mxfp4(_random_bf16(n, k, dev, n + k + 1))
    c = workload.gemm_mxfp4_skinny_nt(aq, bq, sa, sb, split_k=0)
    a, b = _deq(aq, sa), _deq(bq, sb)
    ref = a @ b.T
    # bf16 output rounding (2^-8 relative, ×2) + first-order bound of a length-K fp32 sum in any order (×2).
    tol = 2.0 ** -7 * ref.abs() + k * 2.0 ** -23 * (a.abs() @ b.abs().T)
    err = (c.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()
    assert torch.equal(c, workload.gemm_mxfp4_skinny_nt(aq, bq, sa, sb, split_k=0))  # no atomics: bit-identical


def test_mxfp4_skinny_burner_and_refusal(dev):
    with workload.Burner(device=0, size=1024, gemms=1, triad_mb=16, precision="mxfp4", batch=8) as b:
        time.sleep(0.5)
    assert b.mode == "eager" and b.iterations > 0
    a = torch.zeros(8, 128, device=dev, dtype=torch.uint8)
    w = torch.zeros(128, 128, device=dev, dtype=torch.uint8)
    s = torch.full((128, 8), 127, device=dev, dtype=torch.uint8)
    out = torch.empty(8 * 128 + 1, device=dev, dtype=torch.bfloat16)[1:].view(8, 128)  # 2-byte offset
    with pytest.raises(RuntimeError):
        workload.gemm_mxfp4_skinny_nt(a, w, s[:8], s, out=out)
