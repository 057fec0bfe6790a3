"""Host-side validation of the decode attention interface: every refusal below is raised before the native module or a
device is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import workload


def _operands(b=2, hq=8, hkv=2, s=64, d=128, lens_dtype=torch.int32, lens_shape=None):
    q = torch.zeros(b, hq, d, dtype=torch.bfloat16)
    k = torch.zeros(b, hkv, s, d, dtype=torch.bfloat16)
    return q, k, k.clone(), torch.ones(lens_shape or (b,), dtype=lens_dtype)


@pytest.mark.parametrize("kwargs,error,match", [
    (dict(), ValueError, "GPU"),  # CPU tensors, everything else in order
    (dict(d=64), ValueError, "head dim 128"),
    (dict(hq=7), ValueError, "multiple of Hkv"),
    (dict(hq=34), ValueError, "<= 16"),  # G = 17
    (dict(lens_dtype=torch.int64), TypeError, "int32"),
    (dict(lens_shape=(3,)), ValueError, "seq_lens must be"),
])
def test_attn_decode_refuses(kwargs, error, match):
    with pytest.raises(error, match=match):
        workload.attn_decode_bf16(*_operands(**kwargs))


def test_attn_decode_refuses_non_contiguous_cache():
    q, k, v, lens = _operands()
    with pytest.raises(ValueError, match="contiguous"):
        workload.attn_decode_bf16(q, k.transpose(1, 2).contiguous().transpose(1, 2), v, lens)


@pytest.mark.parametrize("kwargs", [dict(context=512), dict(batch=8, size=512, context=512)])
def test_burner_refuses_bad_context(kwargs):
    with pytest.raises(ValueError, match="context"):
        workload.Burner(precision="mxfp4", **kwargs)
