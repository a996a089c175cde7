"""CPU: the host side of generate(sampling_warpers=...) — tests/sampling_warpers_ref.py against what transformers' own
MinP / Typical / Epsilon / Eta warpers keep (tests/golden/sampling_warpers.npz, tools/capture_sampling_warpers_goldens.py),
SamplingWarpers' checks and packing, the declaration / export / binding of gar_sample_ext, the refusals that need no device, and
the condition the GPU test's inputs have to meet."""
import inspect
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import sampling_warpers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_transformers_masks():
    g = np.load(os.path.join(ROOT, "tests", "golden", "sampling_warpers.npz"))
    meta = json.loads(bytes(g["meta"]).decode())
    logits, masks = g["logits"], g["masks"]
    assert logits.shape == (6, 1000) and logits.dtype == np.float32 and masks.shape[:2] == (len(meta["cases"]), 6)
    assert np.isinf(logits[5]).sum() > 100 and (logits[4] == logits[4].max()).sum() == 3
    defaults = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    removed_max = 0
    for ci, o in enumerate(meta["cases"]):
        full = dict(defaults, **o)
        want = np.unpackbits(masks[ci], axis=1)[:, :1000].astype(bool)
        for b in range(6):
            _, keep, amb = R.warp_ext(logits[b], *[full[k] for k in meta["keys"]])
            assert not amb.any(), (o, b)
            assert np.array_equal(keep, want[b]), (o, b, np.flatnonzero(keep != want[b]).tolist())
            assert keep.any() and not keep[np.isinf(logits[b])].any()
            removed_max += not keep[int(np.argmax(logits[b]))]
    assert removed_max > 0                       # typical_p does remove the most likely token in some case


def test_restatement_with_all_off_is_the_oracles_warp():
    from oracle import sampling as S
    lg = R.fixture("flat1000").numpy()
    for t, k, p in [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.6, 40, 0.8)]:
        z0, k0 = S.warp(lg[0], t, k, p)
        z, keep, _ = R.warp_ext(lg[0], t, k, p)
        assert np.array_equal(z, z0) and np.array_equal(keep, k0)


def test_sampling_warpers_validation_and_packing():
    from gar_amd import SamplingWarpers
    import gar_amd.sampling_warpers as M
    assert M.SamplingWarpers is SamplingWarpers
    n = SamplingWarpers()
    assert n.neutral and n.pack() == [0.0, 1.0, 0.0, 0.0]
    for kw in (dict(min_p=0), dict(min_p=0.0), dict(typical_p=1.0), dict(typical_p=1), dict(typical_p=3.5), dict(epsilon_cutoff=0),
               dict(eta_cutoff=0.0), dict(min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None)):
        assert SamplingWarpers(**kw).neutral and SamplingWarpers(**kw).pack() == [0.0, 1.0, 0.0, 0.0], kw
    w = SamplingWarpers(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    assert not w.neutral and w.pack() == [0.05, 0.9, 3e-4, 2e-3] and all(isinstance(x, float) for x in w.pack())
    assert SamplingWarpers(min_p=1).pack() == [1.0, 1.0, 0.0, 0.0] and not SamplingWarpers(min_p=1).neutral
    for kw in (dict(min_p=0.1), dict(typical_p=0.5), dict(epsilon_cutoff=0.5), dict(eta_cutoff=1e-3)):
        assert not SamplingWarpers(**kw).neutral
    with pytest.raises(Exception):                                   # frozen
        w.min_p = 0.2
    for kw, name in [(dict(min_p=-0.1), "min_p"), (dict(min_p=1.01), "min_p"), (dict(min_p="a"), "min_p"), (dict(min_p=True), "min_p"),
                     (dict(min_p=float("nan")), "min_p"),
                     (dict(typical_p=0), "typical_p"), (dict(typical_p=-1.0), "typical_p"), (dict(typical_p=float("nan")), "typical_p"),
                     (dict(epsilon_cutoff=1.0), "epsilon_cutoff"), (dict(epsilon_cutoff=-1e-3), "epsilon_cutoff"),
                     (dict(epsilon_cutoff=2), "epsilon_cutoff"), (dict(eta_cutoff=1.0), "eta_cutoff"), (dict(eta_cutoff=-0.5), "eta_cutoff"),
                     (dict(eta_cutoff=float("nan")), "eta_cutoff"), (dict(eta_cutoff=[0.1]), "eta_cutoff")]:
        with pytest.raises(ValueError, match=name):
            SamplingWarpers(**kw)
    assert SamplingWarpers.coerce(None) == n and SamplingWarpers.coerce(w) is w
    assert SamplingWarpers.coerce(dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)) == w
    with pytest.raises(TypeError, match="top_h"):
        SamplingWarpers.coerce(dict(top_h=0.5))
    with pytest.raises(TypeError):
        SamplingWarpers.coerce(0.05)


def test_header_declares_and_libraries_export_gar_sample_ext():
    subprocess.run(["make", "-C", os.path.join(ROOT, "grasp-any-region_amd", "csrc"), "-j8"], check=True, capture_output=True)
    from gar_amd import hip, ops
    src = open(os.path.join(ROOT, "include", "gar_hip.h")).read()
    assert "#define GAR_ABI_VERSION 16" in src                      # additive: the ABI number stands
    assert src.index("EXTRAS") < src.index("int gar_sample_ext")
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+gar_sample_ext\s*\(([^;]*)\)\s*;", src)
    assert decl, "gar_sample_ext is not declared in include/gar_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 20 == len(hip.SIGNATURES["gar_sample_ext"][0])
    lp = [a.strip() for a in re.search(r"\bint\s+gar_sample_lp\s*\(([^;]*)\)\s*;", src).group(1).split(",")]
    assert args[:18] == lp[:18] and args[18] == "int32_t* n_kept" and args[19] == lp[18]       # gar_sample_lp's, plus n_kept
    assert [len(hip.SIGNATURES[n][0]) for n in ("gar_sample", "gar_sample_lp", "gar_sample_rows")] == [17, 19, 15]
    assert hip.ABI_VERSION == 16 and ops.SAMPLE_EXT_PARAMS == 8 and ops.SAMPLE_ROW_WORDS == 8
    for f16 in (False, True):
        lib = hip.load_library(f16=f16)
        assert hasattr(lib, "gar_sample_ext") and lib.gar_abi_version() == 16
    for name in ("libgar_hip.so", "libgar_hip_f16.so"):
        out = subprocess.run(["nm", "-D", os.path.join(ROOT, "grasp-any-region_amd", "gar_amd", name)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        assert any(ln.split()[-1] == "gar_sample_ext" and " T " in ln for ln in out.stdout.splitlines()), name
    ps = list(inspect.signature(ops.sample_ext).parameters)
    assert ps == list(inspect.signature(ops.sample).parameters) + ["n_kept"]


def _stub_model():
    return types.SimpleNamespace(MAX_EOS_IDS=8, _check_decode_rows=lambda rows, what: None)


def _sample():
    import torch
    return dict(input_ids=torch.zeros(1, 4, dtype=torch.int64))


def test_continuous_batcher_refuses_by_name():
    from gar_amd import SamplingWarpers, hip
    from gar_amd.continuous import ContinuousBatcher
    for val in (SamplingWarpers(min_p=0.05), dict(min_p=0.05), {}):
        with pytest.raises(hip.GarError, match="sampling_warpers"):
            ContinuousBatcher(_stub_model(), 4, sampling=True, sampling_warpers=val)
    cb = ContinuousBatcher(_stub_model(), 4, max_new_tokens=16, sampling=True)
    with pytest.raises(hip.GarError, match="sampling_warpers"):
        cb.submit(_sample(), do_sample=True, sampling_warpers=SamplingWarpers(min_p=0.05))
    with pytest.raises(hip.GarError, match="sampling_warpers"):
        cb.submit(dict(_sample(), sampling_warpers=dict(typical_p=0.5)), do_sample=True)
    assert not cb.queue and cb._next_ticket == 0
    assert cb.submit(_sample(), do_sample=True, seed=3) == 0           # the plain sampled request is taken as before


def test_config_fields_stay_refused_with_the_hint():
    from gar_amd import hip
    from gar_amd.modeling_gar import _option_reader, _sampling_options
    for kw in (dict(min_p=0.1), dict(typical_p=0.5), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
        name = next(iter(kw))
        for get in (_option_reader(dict(do_sample=True, **kw), {}), _option_reader(None, dict(do_sample=True, **kw))):
            with pytest.raises(hip.GarError, match=name) as e:
                _sampling_options(get)
            assert "pass generate(sampling_warpers=SamplingWarpers(...)) instead" in str(e.value)
    # neutral values of the fields pass as before
    assert _sampling_options(_option_reader(dict(do_sample=True, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), {})) \
        == (1.0, 1.0, 50)


def test_generate_signature_and_state_plumbing():
    from gar_amd.modeling_gar import GARModel
    for fn in (GARModel.generate_begin,):
        assert inspect.signature(fn).parameters["sampling_warpers"].default is None


@pytest.mark.parametrize("name", R.FIXTURES)
def test_gpu_inputs_are_mostly_unambiguous(name):
    """the condition of tests/test_gpu_sampling_warpers.py's inputs: in every (fixture, dtype) group at least 80 % of the 80
    (parameter set, row) pairs have no ambiguous token. Seen: flat37 0 / 0 / 0, flat1000 8 / 3 / 6, peaked128256 1 / 2 / 3 of 80
    (float32 / bfloat16 / float16)."""
    assert len(R.PARAM_SETS) == 10
    for dt in R.DTYPES:
        lg, sets = R.group(name, dt)
        assert lg.shape[0] == 8 and sum(len(rows) for rows in sets) == 80
        n = R.ambiguous_rows(name, dt)
        print(name, dt, "ambiguous rows:", n, "of 80")
        assert n <= 16, (name, dt, n)
    # sets nine and ten leave one token; sets four and eight remove the row maximum in most rows
    lg, sets = R.group(name, "float32")
    assert all(len(kept) == 1 for i in (8, 9) for kept, _ in sets[i])
    if name != "flat37":
        for i in (3, 7):
            gone = sum(int(np.argmax(lg[b])) not in set(sets[i][b][0].tolist()) for b in range(8))
            assert gone >= 5, (name, i, gone)
