"""Host-side validation of the FP8 KV-cache interface (kv_append_fp8, attn_decode_fp8): every refusal below is raised
before the native module or a device is touched."""
import pytest
import torch

from headlamp_intel_gpu_plugin_amd.ops import attention


def _operands(b=2, hq=8, hkv=2, s=64, d=128, sq=1, q_dtype=torch.bfloat16, cache_dtype=torch.float8_e4m3fn,
              scale_dtype=torch.uint8, lens_dtype=torch.int32, lens_shape=None, scale_s=None, new_hkv=None):
    q = torch.zeros(b, hq, d, dtype=q_dtype)
    new = torch.zeros(b, sq, new_hkv or hkv, d, dtype=q_dtype)
    cache = torch.zeros(b, hkv, s, d, dtype=torch.uint8).view(cache_dtype)
    scale = torch.full((b, hkv, scale_s or s), 127, dtype=scale_dtype)
    return q, new, cache, scale, torch.ones(lens_shape or (b,), dtype=lens_dtype)


def _decode(q, new, cache, scale, lens):
    attention.attn_decode_fp8(q, cache, cache.clone(), scale, scale.clone(), lens)


def _append(q, new, cache, scale, lens):
    attention.kv_append_fp8(new, new.clone(), cache, cache.clone(), scale, scale.clone(), lens)


SHARED = [
    (dict(), ValueError, "GPU"),  # CPU tensors, everything else in order
    (dict(q_dtype=torch.float16), TypeError, "bfloat16"),
    (dict(cache_dtype=torch.uint8), TypeError, "float8_e4m3fn"),
    (dict(scale_dtype=torch.int8), TypeError, "uint8"),
    (dict(lens_dtype=torch.int64), TypeError, "int32"),
    (dict(lens_shape=(3,)), ValueError, "seq_lens must be"),
    (dict(scale_s=60), ValueError, "shape mismatch"),
    (dict(d=64), ValueError, "head dim 128"),
    (dict(s=66), ValueError, "multiple of 4"),
    (dict(b=1, hq=1, hkv=1, s=2 ** 25), ValueError, "2\\^32"),
]


@pytest.mark.parametrize("call", [_decode, _append])
@pytest.mark.parametrize("kwargs,error,match", SHARED)
def test_fp8_cache_functions_refuse(call, kwargs, error, match):
    if kwargs.get("s") == 2 ** 25:  # 4 GiB caches: meta tensors carry the shape without the memory
        with torch.device("meta"):
            ops = _operands(**kwargs)
    else:
        ops = _operands(**kwargs)
    with pytest.raises(error, match=match):
        call(*ops)


@pytest.mark.parametrize("call,kwargs,match", [
    (_decode, dict(hq=7), "multiple of Hkv"),
    (_decode, dict(hq=34), "<= 16"),  # G = 17
    (_append, dict(new_hkv=3), "k_new must be"),
])
def test_fp8_cache_functions_refuse_heads(call, kwargs, match):
    with pytest.raises(ValueError, match=match):
        call(*_operands(**kwargs))


@pytest.mark.parametrize("call", [_decode, _append])
@pytest.mark.parametrize("which", ["cache", "scale"])
def test_fp8_cache_functions_refuse_non_contiguous(call, which):
    q, new, cache, scale, lens = _operands()
    if which == "cache":
        cache = cache.view(torch.uint8).transpose(1, 2).contiguous().transpose(1, 2).view(torch.float8_e4m3fn)
    else:
        scale = scale.transpose(1, 2).contiguous().transpose(1, 2)
    with pytest.raises(ValueError, match="contiguous"):
        call(q, new, cache, scale, lens)
