"""CPU: the public surface of the opt-in FP8 decode weights (GARModel(decode_weight_dtype=...), the --decode_weight_dtype flags, the
bindings of gar_weight_quantize_fp8 / gar_gemm_w8). The kernels and the model path are exercised in
tests/test_gpu_decode_weights_fp8.py."""
import inspect
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp8_weights_refuse_the_f32_parity_mode_and_unknown_names():
    from gar_amd import GARConfig, hip
    from gar_amd.modeling_gar import GARModel
    cfg = GARConfig.tiny()
    with pytest.raises(hip.GarError, match="fp8"):
        GARModel(cfg, {}, torch.float32, "cpu", decode_weight_dtype="fp8")
    with pytest.raises(hip.GarError, match="decode_weight_dtype"):
        GARModel(cfg, {}, torch.bfloat16, "cpu", decode_weight_dtype="e4m3")
    with pytest.raises(hip.GarError, match="decode_weight_dtype"):
        GARModel(cfg, {}, torch.bfloat16, "cpu", decode_weight_dtype="int8")


def test_decode_weight_dtype_is_a_constructor_argument():
    from gar_amd.modeling_gar import GARModel
    for fn in (GARModel.__init__, GARModel.from_pretrained):
        p = inspect.signature(fn).parameters["decode_weight_dtype"]
        assert p.default is None


def test_more_than_64_decode_rows_are_refused():
    from gar_amd import hip
    from gar_amd.continuous import ContinuousBatcher
    from gar_amd.modeling_gar import GARModel
    stub = types.SimpleNamespace(w_fp8=True, W8_MAX_ROWS=GARModel.W8_MAX_ROWS)
    stub._check_decode_rows = types.MethodType(GARModel._check_decode_rows, stub)
    assert GARModel.W8_MAX_ROWS == 64
    stub._check_decode_rows(64, "generate")          # the largest skinny decode batch is taken
    with pytest.raises(hip.GarError, match="at most 64 rows"):
        stub._check_decode_rows(65, "generate")
    with pytest.raises(hip.GarError, match="ContinuousBatcher"):
        ContinuousBatcher(stub, slots=65)
    off = types.SimpleNamespace(w_fp8=False, W8_MAX_ROWS=64)
    GARModel._check_decode_rows(off, 4096, "generate")  # the default weights decode any batch


def test_kernels_are_bound():
    from gar_amd import hip, ops
    assert hip.ABI_VERSION == 16                       # additive: gar_gemm_params is unchanged
    for name in ("gar_weight_quantize_fp8", "gar_gemm_w8"):
        assert name in hip.SIGNATURES
    assert callable(ops.weight_quantize_fp8)
    assert "w_scale" in inspect.signature(ops.gemm).parameters
    assert open(os.path.join(ROOT, "include", "gar_hip.h")).read().count("#define GAR_ABI_VERSION 16") == 1


def test_gemm_refuses_a_scale_without_fp8_weights_and_fp8_weights_without_a_scale():
    from gar_amd import hip, ops
    a = torch.zeros(1, 64, dtype=torch.bfloat16)
    with pytest.raises(hip.GarError, match="w_scale"):
        ops.gemm(a, torch.zeros(16, 64, dtype=torch.uint8), torch.zeros(1, 16, dtype=torch.bfloat16))
    with pytest.raises(hip.GarError, match="w_scale"):
        ops.gemm(a, torch.zeros(16, 64, dtype=torch.bfloat16), torch.zeros(1, 16, dtype=torch.bfloat16),
                 w_scale=torch.ones(16))


def test_cli_flags():
    sys.path.insert(0, os.path.join(ROOT, "demo"))
    try:
        import _common
    finally:
        sys.path.pop(0)
    from gar_amd import bench_loops
    ap = _common.base_parser("x")
    assert ap.parse_args([]).decode_weight_dtype == "auto"
    assert ap.parse_args(["--decode_weight_dtype", "fp8"]).decode_weight_dtype == "fp8"
    with pytest.raises(SystemExit):
        ap.parse_args(["--decode_weight_dtype", "int4"])
    bp = bench_loops.base_parser("x", "m", "c", "i")
    assert bp.parse_args(["--anno_file", "a"]).decode_weight_dtype == "auto"
    assert bp.parse_args(["--anno_file", "a", "--decode_weight_dtype", "fp8"]).decode_weight_dtype == "fp8"
    with pytest.raises(SystemExit):
        bp.parse_args(["--anno_file", "a", "--decode_weight_dtype", "bf16"])
