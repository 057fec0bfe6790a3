"""Host-side validation of the MXFP4 decode interface: every refusal below is raised before the native module or a
device is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import workload


def _operands(m=8, n=128, k=512):
    a = torch.zeros(m, k // 2, dtype=torch.uint8)
    b = torch.zeros(n, k // 2, dtype=torch.uint8)
    return a, b, torch.full((m, k // 32), 127, dtype=torch.uint8), torch.full((n, k // 32), 127, dtype=torch.uint8)


def test_skinny_refuses_cpu_tensors():
    with pytest.raises(ValueError, match="GPU"):
        workload.gemm_mxfp4_skinny_nt(*_operands())


@pytest.mark.parametrize("shape,split_k,match", [(dict(m=0), 1, "1<=M<=64"), (dict(m=65), 1, "1<=M<=64"),
                                                 (dict(n=192), 1, "N%128"), (dict(k=384), 1, "K%256"),
                                                 (dict(k=768), 2, "split_k")])
def test_skinny_refuses_bad_shapes(shape, split_k, match):
    with pytest.raises(ValueError, match=match):
        workload.gemm_mxfp4_skinny_nt(*_operands(**shape), split_k=split_k)


@pytest.mark.parametrize("precision,batch", [("bf16", 8), ("mxfp4", 65)])
def test_burner_refuses_bad_batch(precision, batch):
    with pytest.raises(ValueError, match="batch"):
        workload.Burner(precision=precision, batch=batch)
