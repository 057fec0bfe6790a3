"""Host-side validation of the MXFP8 interface: every refusal below is raised before the native module is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import workload

F8 = torch.float8_e4m3fn


def _operands(m=256, n=256, k=128, k_b=None):
    a = torch.zeros(m, k).to(F8)
    b = torch.zeros(n, k if k_b is None else k_b).to(F8)
    return a, b, torch.full((m, k // 32), 127, dtype=torch.uint8), torch.full((n, k // 32), 127, dtype=torch.uint8)


def test_gemm_mxfp8_refuses_cpu_tensors_and_wrong_dtypes():
    a, b, sa, sb = _operands()
    with pytest.raises(ValueError, match="GPU"):
        workload.gemm_mxfp8_nt(a, b, sa, sb)
    with pytest.raises(TypeError):
        workload.gemm_mxfp8_nt(a.to(torch.bfloat16), b)
    with pytest.raises(TypeError):
        workload.gemm_mxfp8_nt(a, b, sa.float(), sb)
    with pytest.raises(TypeError):
        workload.quantize_mxfp8(torch.zeros(4, 32))
    with pytest.raises(ValueError, match="GPU"):
        workload.quantize_mxfp8(torch.zeros(4, 32, dtype=torch.bfloat16))


@pytest.mark.parametrize("case", ["mismatched_k", "partial_tile", "scale_shape", "one_sided_scales"])
def test_gemm_mxfp8_refuses_bad_shapes(case):
    a, b, sa, sb = _operands(k_b=256 if case == "mismatched_k" else None)
    if case == "partial_tile":
        a, sa = a[:128], sa[:128]
    if case == "scale_shape":
        sa = sa[:, :2]
    if case == "one_sided_scales":
        sb = None
    with pytest.raises(ValueError):
        workload.gemm_mxfp8_nt(a, b, sa, sb)


def test_quantize_mxfp8_refuses_partial_blocks():
    with pytest.raises(ValueError):
        workload.quantize_mxfp8(torch.zeros(4, 48, dtype=torch.bfloat16))


def test_unknown_precision_is_refused():
    with pytest.raises(ValueError):
        workload.Burner(precision="nope")
    with pytest.raises(ValueError):
        workload.time_gemm(precision="nope")
