"""GPU tests of the MXFP8 path (gemm_mxfp8_nt, quantize_mxfp8, Burner precision="mxfp8") against plain torch in
float64: operands are dequantised to q · 2^(s−127), the scale repeated over its 32 elements along K, then matmul."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import workload  # noqa: E402

F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda", 0)


def _deq(q, s):
    # 2^(s−127) built from its bits: exact for the scale bytes ≥ 1 that these tests produce.
    scale = (s.to(torch.int32) << 23).view(torch.float32).double()
    return q.float().double() * scale.repeat_interleave(32, dim=1)


@pytest.mark.parametrize("m,n,k", [(256, 256, 128), (256, 512, 384), (768, 512, 256), (512, 256, 1024)])
def test_mxfp8_gemm_exact_integers_scaled(dev, m, n, k):
    # Every partial sum is a multiple of 2^-4 below 2^14, hence exact in fp32: a scale from the wrong row, K-block
    # or byte of its dword changes the result.
    a = (torch.arange(m * k, device=dev) % 5 - 2).reshape(m, k).float().to(F8)
    b = ((torch.arange(n * k, device=dev) * 7 + 3) % 3 - 1).reshape(n, k).float().to(F8)
    sa = (torch.arange(m * k // 32, device=dev) % 5 + 125).to(torch.uint8).reshape(m, k // 32)
    sb = ((torch.arange(n * k // 32, device=dev) * 3) % 4 + 126).to(torch.uint8).reshape(n, k // 32)
    c = workload.gemm_mxfp8_nt(a, b, sa, sb)
    ref = _deq(a, sa) @ _deq(b, sb).T
    assert torch.equal(c, ref.float().bfloat16()), (c.double() - ref).abs().max().item()


def test_mxfp8_gemm_identity_asymmetric_unscaled(dev):
    # A = I with an asymmetric B: a transposed store or a swapped half-tile shows up exactly.
    m, n, k = 512, 768, 256
    a = torch.zeros(m, k, device=dev)
    a[:k, :k] = torch.eye(k, device=dev)
    bvals = (torch.arange(n * k, device=dev, dtype=torch.float32).reshape(n, k) % 31) - 15  # exact in e4m3
    c = workload.gemm_mxfp8_nt(a.to(F8), bvals.to(F8))
    assert torch.equal(c[:k].float(), bvals.T[:k].contiguous())
    assert torch.count_nonzero(c[k:]) == 0


def _random_bf16(rows, k, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, k, device=dev, generator=g)
    return (x * torch.exp2(torch.randint(-6, 7, (rows, 1), device=dev, generator=g).float())).bfloat16()


@pytest.mark.parametrize("m,n,k", [(256, 512, 384), (768, 512, 1024)])
def test_mxfp8_quantise_then_gemm_random(dev, m, n, k):
    aq, sa = workload.quantize_mxfp8(_random_bf16(m, k, dev, m + k))
    bq, sb = workload.quantize_mxfp8(_random_bf16(n, k, dev, n + k + 1))
    c = workload.gemm_mxfp8_nt(aq, bq, sa, sb)
    a, b = _deq(aq, sa), _deq(bq, sb)
    ref = a @ b.T
    # bf16 output rounding (2^-8 relative, ×2) + first-order bound of a length-K fp32 sum in any order (×2).
    tol = 2.0 ** -7 * ref.abs() + k * 2.0 ** -23 * (a.abs() @ b.abs().T)
    err = (c.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()


def _quantise_reference(x):
    """OCP MX rule on the CPU: exponent from frexp, exact power-of-two scaling, clamp, torch's RNE e4m3 cast."""
    rows, k = x.shape
    v = x.cpu().double().reshape(rows, k // 32, 32)
    amax = v.abs().amax(-1)
    exp = (torch.frexp(amax)[1] - 1 - 8).clamp(-127, 127)  # frexp: amax = f · 2^e with f in [0.5, 1)
    exp = torch.where(amax == 0, torch.zeros_like(exp), exp)
    q = (v * 2.0 ** (-exp.double()).unsqueeze(-1)).clamp(-448, 448).float().to(F8)
    return q.reshape(rows, k), (exp + 127).to(torch.uint8)


@pytest.mark.parametrize("rows,k", [(256, 128), (512, 384)])
def test_mxfp8_quantiser_bit_exact(dev, rows, k):
    x = _random_bf16(rows, k, dev, rows + k)
    x[rows // 2, 32:64] = 0  # one all-zero block: scale byte 127, zeros
    q, s = workload.quantize_mxfp8(x)
    q_ref, s_ref = _quantise_reference(x)
    assert s.shape == (rows, k // 32) and torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu().view(torch.uint8), q_ref.view(torch.uint8))


def test_mxfp8_refusals_and_burner(dev):
    a = torch.zeros(256, 192, device=dev).to(F8)
    with pytest.raises(ValueError):
        workload.gemm_mxfp8_nt(a, a)  # K % 128 != 0
    a = torch.zeros(256, 128, device=dev).to(F8)
    out = torch.empty(256 * 256 + 1, device=dev, dtype=torch.bfloat16)[1:].view(256, 256)  # 2-byte offset
    with pytest.raises(RuntimeError):
        workload.gemm_mxfp8_nt(a, a, out=out)
    with workload.Burner(device=0, size=1024, gemms=1, triad_mb=16, precision="mxfp8") as b:
        time.sleep(0.5)
    assert b.mode == "eager" and b.iterations > 0
