"""The sampling entry points (gar_sample, gar_sample_lp, gar_sample_ext, gar_sample_rows) against what the commit before the pick
refactor answered, bit for bit: tests/golden/pick_parent.npz was written once by tools/capture_pick_goldens.py with that commit's
libraries (its hash is in the file) and is never regenerated from the code under test. The oracle suites allow an ambiguity share
near a cut; this one allows nothing: int64 tokens, the raw and warped planes as uint32 bit patterns, n_kept, finished and
done_count are compared for exact equality over every call of tests/pick_parent_cases.py.

The unmarked test runs on the CPU: the golden's tokens lie in the kept sets of the CPU restatements and its greedy rows are first
maxima, so the golden itself is sane."""
import functools
import json
import os

import numpy as np
import pytest

import pick_parent_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pick_parent.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    meta = json.loads(g.pop("meta").tobytes().decode())
    assert meta["rows_sha256"] == C.rows_sha256(), "numpy.random.default_rng rebuilt other rows than the golden was captured on"
    assert len(meta["commit"]) == 40
    return g


def test_golden_is_sane_on_the_cpu():
    g = _golden()
    n = C.check_sane(g["tokens"])
    per_call = {"float32": C.B, "bfloat16": C.B, "float16": len(C.QUANT_ROWS)}
    assert n == sum(per_call[c[2]] for c in C.calls())
    assert len(g["lp_raw"]) == len(g["lp_warped"]) and 0 < len(g["n_kept"]) < n
    assert (g["finished"] >= 0).any() and (g["finished"] < 0).any() and g["done_count"].max() > 0          # the latches are exercised


@pytest.mark.gpu
def test_pick_equals_parent_bit_for_bit():
    from gar_amd import hip
    hip.require_device(0)
    want = _golden()
    got = C.replay()
    assert sorted(got) == sorted(want)
    for name in ("tokens", "n_kept", "finished", "done_count", "lp_raw", "lp_warped"):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        diff = np.flatnonzero(got[name] != want[name])
        assert diff.size == 0, (name, diff.size, diff[:8].tolist(), got[name][diff[:8]].tolist(), want[name][diff[:8]].tolist())
