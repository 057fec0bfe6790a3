"""GPU tests of the MXFP4 path (gemm_mxfp4_nt, quantize_mxfp4, Burner precision="mxfp4") against plain torch in
float64: nibble codes are decoded through the 16-entry e2m1 table and scaled by 2^(s−127), the scale repeated over
its 32 elements along K, then matmul. G is the kernel's K granule: it consumes 256-element K-tiles in pairs."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from headlamp_intel_gpu_plugin_amd.ops import workload  # noqa: E402

G = 512
E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)


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


@pytest.mark.parametrize("m,n,k", [(256, 256, G), (256, 512, 3 * G), (768, 512, 2 * G), (512, 256, 4 * G)])
def test_mxfp4_gemm_exact_scaled(dev, m, n, k):
    # Every term is a multiple of 2^-4 and at most 96, so up to K = 2048 the sums stay below 2^18 and need at most
    # 22 bits: exact in fp32 in any order. A wrong nibble order, k-to-lane map, scale byte or row shows.
    i = torch.arange(m * k, device=dev)
    a = _pack(((i + i // k) % 16).reshape(m, k))  # every code, shifted by one from row to row
    b_sign = ((torch.arange(n * k, device=dev) * 7 + 3) % 3 - 1).reshape(n, k)  # -1, 0, 1
    b = _pack(torch.where(b_sign < 0, 10, b_sign * 2))
    sa = (torch.arange(m * k // 32, device=dev) % 5 + 125).to(torch.uint8).reshape(m, k // 32)
    # SB block j of row r is (3j + j//4 + r) % 4: bytes g and 4+g of a K-tile, K-tiles and rows all differ.
    j = torch.arange(n * k // 32, device=dev)
    sb = ((j * 3 + j // 4 + j // (k // 32)) % 4 + 126).to(torch.uint8).reshape(n, k // 32)
    c = workload.gemm_mxfp4_nt(a, b, sa, sb)
    ref = _deq(a, sa) @ _deq(b, sb).T
    assert torch.equal(c, ref.float().bfloat16()), (c.double() - ref).abs().max().item()


def test_mxfp4_gemm_identity_asymmetric(dev):
    # A = I (code 2 is 1.0) over zero rows, asymmetric B, scales 127: catches transposed stores and swapped nibbles.
    m, n, k = 768, 512, G
    a = torch.zeros(m, k, device=dev, dtype=torch.uint8)
    a[:k] = 2 * torch.eye(k, device=dev, dtype=torch.uint8)
    b = _pack((torch.arange(n * k, device=dev) % 13).reshape(n, k))  # 512 % 13 != 0: differs from row to row
    one = torch.full((1, k // 32), 127, device=dev, dtype=torch.uint8)
    c = workload.gemm_mxfp4_nt(_pack(a), b, one.expand(m, -1), one.expand(n, -1))
    assert torch.equal(c[:k].double(), _deq(b, one.expand(n, -1)).T)
    assert torch.count_nonzero(c[k:]) == 0


def _random_bf16(rows, k, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(rows, k, device=dev, generator=g)
    return (x * torch.exp2(torch.randint(-6, 7, (rows, 1), device=dev, generator=g).float())).bfloat16()


@pytest.mark.parametrize("m,n,k", [(256, 512, 3 * G), (768, 512, 4 * G)])
def test_mxfp4_quantise_then_gemm_random(dev, m, n, k):
    aq, sa = workload.quantize_mxfp4(_random_bf16(m, k, dev, m + k))
    bq, sb = workload.quantize_mxfp4(_random_bf16(n, k, dev, n + k + 1))
    c = workload.gemm_mxfp4_nt(aq, bq, sa, sb)
    a, b = _deq(aq, sa), _deq(bq, sb)
    ref = a @ b.T
    # bf16 output rounding (2^-8 relative, ×2) + first-order bound of a length-K fp32 sum in any order (×2).
    tol = 2.0 ** -7 * ref.abs() + k * 2.0 ** -23 * (a.abs() @ b.abs().T)
    err = (c.double() - ref).abs()
    print(f"worst error/tolerance {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= tol).all()


def _quantise_reference(x):
    """OCP MX rule on the CPU in float64: exponent from frexp, exact scaling, clamp to 6, nearest table entry with
    ties to the even code. The input's sign bit is kept: a negative value that rounds to zero is −0 (code 8)."""
    rows, k = x.shape
    v = x.cpu().double().reshape(rows, k // 32, 32)
    amax = v.abs().amax(-1)
    exp = (torch.frexp(amax)[1] - 1 - 2).clamp(-127, 127)  # frexp: amax = f · 2^e with f in [0.5, 1)
    exp = torch.where(amax == 0, torch.zeros_like(exp), exp)
    dist = ((v * 2.0 ** (-exp.double()).unsqueeze(-1)).abs().clamp(max=6).unsqueeze(-1) - E2M1[:8]).abs()
    lo = dist.argmin(-1)  # the first minimum: the lower code of a tie
    hi = (lo + 1).clamp(max=7)
    tie = (hi != lo) & (dist.gather(-1, hi.unsqueeze(-1)) == dist.gather(-1, lo.unsqueeze(-1))).squeeze(-1)
    codes = torch.where(tie & (lo % 2 == 1), hi, lo) + 8 * torch.signbit(v)
    return codes.reshape(rows, k).to(torch.uint8), (exp + 127).to(torch.uint8)


@pytest.mark.parametrize("rows,k", [(256, 128), (512, 384)])
def test_mxfp4_quantiser_bit_exact(dev, rows, k):
    x = _random_bf16(rows, k, dev, rows + k)
    r = rows // 2
    x[r, :96] = 0  # block 2 of this row stays all zero: scale byte 127, zeros
    # Block 0: amax 48 fixes X = 3; then 2.5, 5, −3.5, .25, −.25, .75, 1.75, 1.25 times 8 are exact ties.
    x[r, :9] = torch.tensor([48, 20, 40, -28, 2, -2, 6, 14, 10], device=dev, dtype=torch.bfloat16)
    x[r, 32:34] = torch.tensor([60, 52], device=dev, dtype=torch.bfloat16)  # X = 3: 7.5 and 6.5 clamp to 6
    q, s = workload.quantize_mxfp4(x)
    codes_ref, s_ref = _quantise_reference(x)
    assert s.shape == (rows, k // 32) and torch.equal(s.cpu(), s_ref)
    codes = torch.stack((q.cpu() & 15, q.cpu() >> 4), dim=-1).reshape(rows, k)
    assert codes[r, :9].tolist() == [7, 4, 6, 14, 0, 8, 2, 4, 2] and codes[r, 32:34].tolist() == [7, 7]
    assert torch.equal(codes, codes_ref)


def test_mxfp4_refusals_and_burner(dev):
    a = torch.zeros(256, 128, device=dev, dtype=torch.uint8)  # K = 256: not a multiple of 512
    s = torch.full((256, 8), 127, device=dev, dtype=torch.uint8)
    with pytest.raises(ValueError):
        workload.gemm_mxfp4_nt(a, a, s, s)
    a = torch.zeros(256, 256, device=dev, dtype=torch.uint8)
    s = torch.full((256, 16), 127, device=dev, dtype=torch.uint8)
    out = torch.empty(256 * 256 + 1, device=dev, dtype=torch.bfloat16)[1:].view(256, 256)  # 2-byte offset
    with pytest.raises(RuntimeError):
        workload.gemm_mxfp4_nt(a, a, s, s, out=out)
    with workload.Burner(device=0, size=1024, gemms=1, triad_mb=16, precision="mxfp4") as b:
        time.sleep(0.5)
    assert b.mode == "eager" and b.iterations > 0
