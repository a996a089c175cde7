#!/usr/bin/env python
"""Writes tests/golden/pick_parent.npz on an MI355X: what the sampling entry points of a PARENT commit's libraries answer
(gar_sample, gar_sample_lp, gar_sample_ext, gar_sample_rows) on the calls of tests/pick_parent_cases.py, for
tests/test_gpu_pick_parent.py to hold a refactor of the pick code against, bit for bit.

Run once, with the libraries built from the parent commit and that commit's hash:

    GAR_HIP_LIB=<parent>/libgar_hip.so GAR_HIP_LIB_F16=<parent>/libgar_hip_f16.so \\
        python tools/capture_pick_goldens.py --commit <hash of the parent commit> [--out DIR]

It refuses to run on the tree's own libraries: the file must never be regenerated from the code under test. Stored: the outputs,
the parent's hash and the SHA-256 of the inputs (the rows are rebuilt from their seeds, not stored). Asserted here, on the CPU,
before anything is written: every token of a plain request lies in oracle/sampling.py's kept set, every token of an ext request in
tests/sampling_warpers_ref.py's, every greedy row is the first maximum."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "grasp-any-region_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the libraries were built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    for var in ("GAR_HIP_LIB", "GAR_HIP_LIB_F16"):
        lib = os.environ.get(var)
        if not lib or not os.path.isfile(lib):
            sys.exit(f"{var} has to name a library built from the parent commit")
    import pick_parent_cases as C
    from gar_amd import hip
    hip.require_device(0)
    arrays = C.replay()
    arrays["meta"] = np.frombuffer(json.dumps({"commit": a.commit, "rows_sha256": C.rows_sha256()}).encode(), dtype=np.uint8)
    C.check_sane(arrays["tokens"])
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "pick_parent.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in arrays.items()})
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    sys.exit(main())
