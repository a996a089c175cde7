"""CPU: the public surface of the opt-in FP8 KV cache (GARModel(kv_cache_dtype=...), the --kv_cache_dtype flags, the bindings of
the three kernels). The kernels themselves are exercised in tests/test_gpu_kv_fp8.py."""
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp8_cache_refuses_the_f32_parity_mode_and_unknown_names():
    from gar_amd import GARConfig, hip
    from gar_amd.modeling_gar import GARModel
    cfg = GARConfig.tiny()
    with pytest.raises(hip.GarError, match="fp8"):
        GARModel(cfg, {}, torch.float32, "cpu", kv_cache_dtype="fp8")
    with pytest.raises(hip.GarError, match="kv_cache_dtype"):
        GARModel(cfg, {}, torch.bfloat16, "cpu", kv_cache_dtype="e5m2")


def test_kv_cache_dtype_is_a_constructor_argument():
    from gar_amd.modeling_gar import GARModel
    for fn in (GARModel.__init__, GARModel.from_pretrained):
        p = inspect.signature(fn).parameters["kv_cache_dtype"]
        assert p.default is None


def test_kernels_are_bound():
    from gar_amd import hip, ops
    assert hip.ABI_VERSION == 16
    for name in ("gar_kv_quantize_fp8", "gar_attention_decode_fp8", "gar_attention_decode_fp8_workspace",
                 "gar_attention_decode_qkv_fp8"):
        assert name in hip.SIGNATURES
    for name in ("kv_quantize_fp8", "attention_decode_fp8", "attention_decode_qkv_fp8", "attention_decode_fp8_workspace"):
        assert callable(getattr(ops, name))


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "demo"))
    try:
        import _common
    finally:
        sys.path.pop(0)
    from gar_amd import bench_loops
    ap = _common.base_parser("x")
    assert ap.parse_args([]).kv_cache_dtype == "auto"
    assert ap.parse_args(["--kv_cache_dtype", "fp8"]).kv_cache_dtype == "fp8"
    bp = bench_loops.base_parser("x", "m", "c", "i")
    assert bp.parse_args(["--anno_file", "a"]).kv_cache_dtype == "auto"
    assert bp.parse_args(["--anno_file", "a", "--kv_cache_dtype", "fp8"]).kv_cache_dtype == "fp8"
    with pytest.raises(SystemExit):
        bp.parse_args(["--anno_file", "a", "--kv_cache_dtype", "fp16"])
