"""Host-side validation of the prefill attention interface: every refusal below is raised before the native module or
a device is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import attention


def _operands(b=2, kb=None, sq=8, hq=8, hkv=2, s=64, d=128, lens_dtype=torch.int32, lens_shape=None, q_view=False):
    q = torch.zeros(b, hq, sq, d, dtype=torch.bfloat16).transpose(1, 2) if q_view else \
        torch.zeros(b, sq, hq, d, dtype=torch.bfloat16)
    k = torch.zeros(kb or b, hkv, s, d, dtype=torch.bfloat16)
    return q, k, k.clone(), torch.ones(lens_shape or (b,), dtype=lens_dtype)


@pytest.mark.parametrize("kwargs,error,match", [
    (dict(), ValueError, "GPU"),  # CPU tensors, everything else in order
    (dict(d=64), ValueError, "head dim 128"),
    (dict(hq=7), ValueError, "multiple of Hkv"),
    (dict(lens_dtype=torch.int64), TypeError, "int32"),
    (dict(lens_shape=(3,)), ValueError, "seq_lens must be"),
    (dict(q_view=True), ValueError, "contiguous"),
    (dict(kb=3), ValueError, "shape mismatch"),
])
def test_attn_prefill_refuses(kwargs, error, match):
    with pytest.raises(error, match=match):
        attention.attn_prefill_bf16(*_operands(**kwargs))
