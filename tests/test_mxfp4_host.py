"""Host-side validation of the MXFP4 interface: every refusal below is raised before the native module is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import workload


def _operands(m=256, n=256, k=512, k_b=None):
    a = torch.zeros(m, k // 2, dtype=torch.uint8)
    b = torch.zeros(n, (k if k_b is None else k_b) // 2, dtype=torch.uint8)
    return a, b, torch.full((m, k // 32), 127, dtype=torch.uint8), torch.full((n, k // 32), 127, dtype=torch.uint8)


def test_gemm_mxfp4_refuses_cpu_tensors_and_wrong_dtypes():
    a, b, sa, sb = _operands()
    with pytest.raises(ValueError, match="GPU"):
        workload.gemm_mxfp4_nt(a, b, sa, sb)
    with pytest.raises(TypeError):
        workload.gemm_mxfp4_nt(a.to(torch.float8_e4m3fn), b, sa, sb)
    with pytest.raises(TypeError):
        workload.gemm_mxfp4_nt(a, b, sa.float(), sb)
    with pytest.raises(TypeError):
        workload.quantize_mxfp4(torch.zeros(4, 32))
    with pytest.raises(ValueError, match="GPU"):
        workload.quantize_mxfp4(torch.zeros(4, 32, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        workload.quantize_mxfp4(torch.zeros(4, 48, dtype=torch.bfloat16))  # a partial block of 32


@pytest.mark.parametrize("case", ["mismatched_k", "partial_tile", "k_not_512", "scale_shape", "missing_scale"])
def test_gemm_mxfp4_refuses_bad_shapes(case):
    a, b, sa, sb = _operands(k_b=1024 if case == "mismatched_k" else None)
    if case == "partial_tile":
        a, sa = a[:128], sa[:128]
    if case == "k_not_512":  # one 256-element K-tile: the kernel takes them in pairs
        a, b, sa, sb = a[:, :128], b[:, :128], sa[:, :8], sb[:, :8]
    if case == "scale_shape":
        sa = sa[:, :8]
    if case == "missing_scale":
        sb = None
    with pytest.raises(ValueError):
        workload.gemm_mxfp4_nt(a, b, sa, sb)


def test_mxfp4_is_a_precision():
    assert "mxfp4" in workload.PRECISIONS
    assert workload.Burner(precision="mxfp4").precision == "mxfp4"
