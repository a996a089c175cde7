"""CPU: host logic of generate(num_return_sequences = N) — option reading, the C ABI of the shared-prefix decode attention, the
tests' float64 restatement of prefix + suffix attention, and the row bookkeeping of the expanded batch. No device."""
import os
import re
import subprocess
import types

import pytest
import torch

import fanout_util as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gar_attention_decode_fanout", "gar_attention_decode_fanout_workspace")


def test_num_return_sequences_is_read_by_all_three_readers():
    from gar_amd import hip
    from gar_amd.modeling_gar import _num_return_sequences, _option_reader, _refuse_non_greedy
    opts = dict(do_sample=True, num_return_sequences=4)
    readers = [_option_reader(types.SimpleNamespace(**opts), {}),       # a GenerationConfig-like object
               _option_reader(dict(opts), {}),                          # a dict
               _option_reader(None, dict(opts)),                        # keywords of the call
               _option_reader(dict(do_sample=True), dict(num_return_sequences=4))]      # a keyword laid over a config
    for get in readers:
        assert _num_return_sequences(get) == 4
        _refuse_non_greedy(get)
    assert _option_reader(None, {}) is None
    assert _num_return_sequences(_option_reader(dict(do_sample=True), {})) == 1
    # without sampling the option stays refused, by name, as before
    for reader in (_option_reader(dict(num_return_sequences=2), {}), _option_reader(None, dict(num_return_sequences=2))):
        with pytest.raises(hip.GarError, match="num_return_sequences"):
            _refuse_non_greedy(reader)
    for bad in (0, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="num_return_sequences"):
            _num_return_sequences(_option_reader(dict(do_sample=True, num_return_sequences=bad), {}))
    # the fp8 KV cache has no shared-prefix kernel: refused on the option path, by name; N = 1 passes
    with pytest.raises(hip.GarError, match="num_return_sequences=2.*fp8"):
        _num_return_sequences(_option_reader(dict(opts, num_return_sequences=2), {}), "fp8")
    assert _num_return_sequences(_option_reader(dict(do_sample=True, num_return_sequences=1), {}), "fp8") == 1
    with pytest.raises(TypeError):
        _option_reader(None, dict(not_an_option=1))


def test_fanout_symbols_are_declared_exported_and_bound():
    from gar_amd import hip, ops
    subprocess.run(["make", "-C", os.path.join(ROOT, "grasp-any-region_amd", "csrc"), "-j8"], check=True, capture_output=True)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gar_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.SIGNATURES
        for lib in (hip.load_library(), hip.load_library(f16=True)):
            assert hasattr(lib, name), name
    assert callable(ops.attention_decode_fanout)
    # one more (m, l, O) slot per (row, head) than the plain decode workspace: the suffix partial
    R, Hq, hd, ns = 64, 32, 64, 3
    assert ops.attention_decode_fanout_workspace(R, Hq, hd, ns) == ops.attention_decode_workspace(R, Hq, hd, ns + 1)


@pytest.mark.parametrize("P,left_pad,t,nsplit", [(1, 0, 0, 1), (63, 0, 1, 2), (64, 37, 0, 8), (200, 199, 5, 3), (1000, 101, 63, 4),
                                                 (1000, 0, 64, 7), (4718, 333, 65, 8), (130, 129, 0, 8)])
def test_prefix_splits_and_suffix_merge_to_plain_softmax(P, left_pad, t, nsplit):
    """the (m, l, O) partials of any number of prefix splits and of the suffix merge to plain softmax attention over the
    concatenated keys — with the suffix holding only the step's new token (t = 0) and with a prefix hidden behind left_pad"""
    g = torch.Generator().manual_seed(P * 131 + t)
    hd, Sp, T = 16, (P + 63) // 64 * 64, (t + 64) // 64 * 64
    q = torch.randn(hd, generator=g, dtype=torch.float64) * 1.5
    Kp, Vp = (torch.randn(Sp, hd, generator=g, dtype=torch.float64) for _ in range(2))
    Ks, Vs = (torch.randn(T, hd, generator=g, dtype=torch.float64) for _ in range(2))
    ranges = F.prefix_split_ranges(P, left_pad, nsplit)
    lo = max(min(left_pad, P - 1), 0)
    covered = [r for a, b in ranges for r in range(a, b)]
    assert covered == list(range(lo, P))                        # the splits tile the live prefix exactly once, in order
    got = F.fanout_attention(q, Kp, Vp, P, left_pad, Ks, Vs, t, nsplit)
    ref = F.softmax_attention(q, torch.cat([Kp[lo:P], Ks[:t + 1]]), torch.cat([Vp[lo:P], Vs[:t + 1]]))
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    # the batched form the GPU test uses is the same function
    K = torch.cat([Kp[:P], Ks[:t + 1]])[None, None]
    V = torch.cat([Vp[:P], Vs[:t + 1]])[None, None]
    bat = F.batched_attention(q[None, None], K, V, torch.tensor([lo]), P + t + 1)[0, 0]
    assert float((bat - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_merge_ignores_empty_partials():
    g = torch.Generator().manual_seed(5)
    q, K, V = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((8,), (5, 8), (5, 8)))
    empty = F.partial(q, K[:0], V[:0])
    assert empty[0] == float("-inf") and empty[1] == 0.0
    one = F.merge([empty, F.partial(q, K, V), empty])
    assert torch.allclose(one, F.softmax_attention(q, K, V), rtol=0, atol=1e-14)


@pytest.mark.parametrize("chunks,N", [([(0, 3)], 4), ([(0, 1), (1, 2), (2, 3)], 4), ([(0, 2), (2, 5)], 3), ([(0, 5)], 1)])
def test_expanded_rows_carry_their_own_philox_row_counter(chunks, N):
    """row b * N + i of the expanded batch draws with row counter b * N + i whatever the prompt chunking: gar_sample counts the
    draw of row j of a launch by row_offset + j, and a chunk's launch covers the rows _fanout_rows gives it"""
    from gar_amd.modeling_gar import _fanout_rows
    counters, owners = [], []
    for b0, b1 in chunks:
        r0, r1 = _fanout_rows(b0, b1, N)
        assert r1 - r0 == (b1 - b0) * N
        counters += [r0 + j for j in range(r1 - r0)]                    # row_offset + local row
        owners += torch.arange(b0, b1).repeat_interleave(N).tolist()    # the prompt whose logits the local row holds
    B = chunks[-1][1]
    assert counters == list(range(B * N))
    assert owners == [r // N for r in range(B * N)]
