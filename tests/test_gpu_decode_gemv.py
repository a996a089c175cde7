"""GPU (-m gpu): the 16-bit weight-streaming GEMVs of the decode step (csrc/gemm_skinny.hip through gar_gemm at M <= 64 — what every
default run and bench.py time) against the f64 restatement of tests/gemv_ref.py, ELEMENT BY ELEMENT, at the real (N, K) of every
Llama GEMV of GAR-1B and GAR-8B and in exactly the forms GARModel._decode_step and _head issue:

    qkv      (3072, 2048) / (6144, 4096)      norm_folded; norm_w (M <= 16); plain on a pre-normed input
    o        (2048, 2048) / (4096, 4096)      EPI_RES in place
    gate/up  (16384, 2048) / (28672, 4096)    EPI_SWIGLU (gate / up interleaved in groups of 16 rows) with norm_folded, norm_w (M <= 16), plain
    down     (2048, 8192) / (4096, 14336)     EPI_RES in place; split-K partials (4 and 2 slices) + gar_splitk_residual_rmsnorm
    lm_head  (128262, 2048) / (128262, 4096)  norm_w (M <= 16), plain above; the logits' row pitch is the model's (V rounded up to 64)

A rewrite of these kernels has to pass this file. Two statistics, because one alone is blind: the per-element bound (f32 accumulation
plus one output rounding — tests/gemv_ref.py) and, for the forms that carry an RMSNorm, the ROW GAIN <out_m, ref_m> / <ref_m, ref_m>:
a row whose sum of squares lost one 64-wide K step is scaled by 1 + 1 / (2 K / 64), which at K >= 8192 is below one bf16 rounding of
a single element but 2 x the gain limit 1 / (4 K / 64) used here (the limit is that condition, not a measurement).

Every output buffer starts as NaN and a NaN fails the comparison, so an element that is never stored is a failure.

Measured on an MI355X when the file was written (the tests print these figures; none is a limit). Worst |err| / bound, bf16, GAR-1B /
GAR-8B: qkv 0.78 / 0.55, o 0.79 / 0.55, gate/up 0.59 / 0.29, down 0.29 / 0.17, lm_head 0.82 / 0.56; every M from 1 to 64: o 0.82,
qkv 0.78; per-lane fragment path 0.50 .. 0.75 and bit-equal to the staged path for o at M = 2; fp16 0.07 .. 0.38. Split-K + reduce:
h 0.17 .. 0.37; the norm output 0.96 .. 0.98 of a bound that is two half-ulp roundings and little else, so the worst of 10^5 elements
sits near it. Worst |row gain - 1|: 1.5e-4 bf16 (limits 7.8e-3 at K = 2048, 3.9e-3 at K = 4096), 2.1e-5 fp16. The whole file: 4 s.
With the NORM == 2 sum of squares missing one K step of one wave (a build made for that, never committed): the per-element tests fail
at every norm_folded shape (worst 5.8 / 2.5 x the bound at qkv, 8.0 / 2.3 at gate/up; 149 934 of 196 608 elements at GAR-1B qkv, M = 64)
and the row gain lands at 2.5e-2 / 1.2e-2 / 1.3e-2 (3.2 x its limit) for qkv and gate/up; norm_w, lm_head, o and down stay green."""
import gc

import pytest
import torch

from gemv_ref import OUT_EPS, gemv_ref, rmsnorm_ref, row_gain

pytestmark = pytest.mark.gpu

EPS = 1e-5
SHAPES = {   # (hidden, intermediate, qkv rows, vocab) of the two Llama configurations
    "gar_1b": (2048, 8192, (32 + 2 * 8) * 64, 128262),
    "gar_8b": (4096, 14336, (32 + 2 * 8) * 128, 128262),
}
MS = (1, 8, 9, 16, 17, 32, 33, 64)      # both sides of the dispatcher's switches: deep ring 8 / 9, half tiles and MT 1 -> 2 at 16 / 17, MT 2 -> 4 at 32 / 33
FUSE_MAX_M = 16                         # GARModel.FUSE_NORM_MAX_BATCH: the decode step passes norm_w up to this many rows
# (prologue, epilogue) per GEMV, as the decode step issues them
FORMS = {
    "qkv": (("norm_folded", "none"), ("norm_w", "none"), ("prenormed", "none")),
    "o": (("plain", "res"),),
    "gu": (("norm_folded", "swiglu"), ("norm_w", "swiglu"), ("prenormed", "swiglu")),
    "down": (("plain", "res"),),
    "lm_head": (("norm_w", "none"), ("prenormed", "none")),
}


def _ms(name, pro, ms=MS):
    if pro == "norm_w":
        return tuple(m for m in ms if m <= FUSE_MAX_M)
    if name == "lm_head":       # _head: the norm rides in the prologue up to 16 rows and is a launch of its own above
        return tuple(m for m in ms if m > FUSE_MAX_M)
    return tuple(ms)


@pytest.fixture(scope="module")
def weights():
    """per configuration, GEMV and type: the 16-bit weight [N, K], built once; freed at module teardown (GAR-8B's lm_head is 1 GiB)"""
    cache = {}

    def get(cfg, name, dt=torch.bfloat16):
        key = (cfg, name, dt)
        if key not in cache:
            C, F, Nq, V = SHAPES[cfg]
            N, K = {"qkv": (Nq, C), "o": (C, C), "gu": (2 * F, C), "down": (C, F), "lm_head": (V, C)}[name]
            g = torch.Generator(device="cuda").manual_seed(len(cfg) * 1000 + len(name) * 10 + (dt == torch.float16))
            cache[key] = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(dt)
        return cache[key]
    yield get
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _poison_lds(dt):
    """a launch that DMA-stages NaN rows through the LDS of every CU (as tests/test_gpu_ops.py::test_skinny_gemm_half_tiles)"""
    from gar_amd import ops
    nan = torch.full((1, 64, 256, 64), float("nan"), dtype=dt, device="cuda")
    junk = torch.empty(256, 64 * 64, dtype=dt, device="cuda")
    ops.attention(nan, nan, nan, junk, 1, 64, 64, 64, 256, 256, 256, 256, causal=False, v_row_major=True)


def _activations(M, K, pro, seed, dt, lda=0):
    """randn * 2 + 0.3 (the rows have a mean, rstd differs from row to row); "prenormed": the unit-gain RMSNorm of that, rounded
    once, as the norm launch in front of a plain GEMV leaves it. lda: a row-strided view whose last row lies beyond 2 GiB."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x0 = torch.randn(M, K, generator=g, device="cuda") * 2 + 0.3
    if pro == "prenormed":
        x0 = x0 * torch.rsqrt((x0 * x0).mean(1, keepdim=True) + EPS)
    x0 = x0.to(dt)
    if not lda:
        return x0, g
    store = torch.zeros((M - 1) * lda + K, dtype=dt, device="cuda")
    x = store.as_strided((M, K), (lda, 1))
    x.copy_(x0)
    return x, g


def _run(w, pro, epi, M, dt=torch.bfloat16, seed=0, lda=0, rows=0, pitch=0, poison=False):
    """one GEMV -> (out [M, N'], f64 reference, bound, the whole NaN-primed buffer [max(rows, M), max(pitch, N')] `out` is a view of)"""
    from gar_amd import hip, ops
    code = {"none": hip.EPI_NONE, "res": hip.EPI_RES, "swiglu": hip.EPI_SWIGLU, "bias": hip.EPI_BIAS}[epi]
    N, K = w.shape
    x, g = _activations(M, K, pro, seed * 7919 + M * 131 + len(pro), dt, lda)
    kw, res, bias, norm_w = {}, None, None, None
    if pro == "norm_folded":
        kw = dict(norm_folded=True, norm_eps=EPS)
    if pro == "norm_w":
        norm_w = (1 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dt)
        kw = dict(norm_w=norm_w, norm_eps=EPS)
    No = N // 2 if epi == "swiglu" else N
    buf = torch.full((max(rows, M), max(pitch, No)), float("nan"), dtype=dt, device="cuda")
    out = buf[:M, :No]
    if epi == "res":            # in place, as the decode step's residual stream
        res = torch.randn(M, N, generator=g, device="cuda").to(dt)
        out.copy_(res)
        kw["residual"] = out
    if epi == "bias":
        bias = torch.randn(N, generator=g, device="cuda").to(dt)
        kw["bias"] = bias
    if poison:
        _poison_lds(dt)
    ops.gemm(x, w, out, code, **kw)
    torch.cuda.synchronize()
    ref, tol = gemv_ref(x, w, code, res, norm_w, pro == "norm_folded", EPS, dt, bias)
    return out, ref, tol, buf


def _ratio(out, ref, tol):
    """(elements outside the bound — a NaN is outside, worst |out - ref| / bound)"""
    r = (out.double() - ref).abs() / tol
    bad = ~(r <= 1)
    return int(bad.sum()), float(torch.nan_to_num(r, nan=float("inf")).max())


def _untouched(buf, M, No):
    """rows past M and columns past N' of the NaN-primed buffer are still NaN: no row tile or ragged last block stores beyond the output"""
    return bool(torch.isnan(buf[M:]).all()) and bool(torch.isnan(buf[:, No:]).all())


def _pitch(name, N):
    return (N + 63) // 64 * 64 if name == "lm_head" else 0


def _table(weights, cfg, name, dt, ms):
    """every form of one GEMV over the given row counts, per element -> failures; prints the worst err / bound per form"""
    fails = []
    for pro, epi in FORMS[name]:
        worst = 0.0
        w = weights(cfg, name, dt)
        for M in _ms(name, pro, ms):
            out, ref, tol, buf = _run(w, pro, epi, M, dt, pitch=_pitch(name, w.shape[0]))
            n, r = _ratio(out, ref, tol)
            worst = max(worst, r)
            if n or not _untouched(buf, M, out.shape[1]):
                fails.append((cfg, name, pro, epi, M, n, round(r, 3), _untouched(buf, M, out.shape[1])))
        print(f"{cfg} {name} {tuple(w.shape)} {pro}/{epi} {str(dt)[6:]}: worst |err| / bound {worst:.3f} over M = {_ms(name, pro, ms)}")
    return fails


@pytest.mark.parametrize("cfg", ["gar_1b", "gar_8b"])
@pytest.mark.parametrize("name", ["qkv", "o", "gu", "down", "lm_head"])
def test_gemv_matches_f64_restatement(weights, cfg, name):
    """bf16, every form of the table x MS: 8-row half tiles and the DEEP ring (o / down at N = 2048, M <= 16 / 8), MT 1 / 2 / 4,
    NT 1 / 2 / 4, NORM 0 / 1 / 2, EPI NONE / RES / SWIGLU, the ragged last block of the lm_head (N = 128262)"""
    fails = _table(weights, cfg, name, torch.bfloat16, MS)
    assert not fails, f"(cfg, gemv, prologue, epilogue, M, elements out of bound, worst err / bound, beyond the output untouched): {fails}"


@pytest.mark.parametrize("name", ["qkv", "o", "gu", "down", "lm_head"])
def test_gemv_fp16_twin(weights, name):
    """the fp16 twin library at GAR-1B, plus one split-K case"""
    fails = _table(weights, "gar_1b", name, torch.float16, (1, 9, 16, 33, 64))
    assert not fails, fails
    if name == "down":
        fails, _, _ = _split_k(weights("gar_1b", "down", torch.float16), 24, 4, torch.float16)
        assert not fails, fails


def test_gemv_bias_epilogue(weights):
    """EPI_BIAS, which the 16-bit skinny kernel builds (the fp8 one does not): plain and with the folded norm, qkv at GAR-1B"""
    w = weights("gar_1b", "qkv")
    fails = []
    for pro in ("plain", "norm_folded"):
        for M in MS:
            out, ref, tol, _ = _run(w, pro, "bias", M)
            n, r = _ratio(out, ref, tol)
            if n:
                fails.append((pro, M, n, round(r, 3)))
    assert not fails, fails


@pytest.mark.parametrize("name", ["o", "qkv"])
def test_gemv_every_row_count(weights, name):
    """every M from 1 to 64 at GAR-1B (o: EPI_RES in place; qkv: norm_folded), per element; the output is the head of an 80-row
    NaN buffer whose rows >= M must stay NaN: a row tile reaching past M is never stored"""
    pro, epi = FORMS[name][0]
    w = weights("gar_1b", name)
    fails, worst = [], 0.0
    for M in range(1, 65):
        out, ref, tol, buf = _run(w, pro, epi, M, rows=80)
        n, r = _ratio(out, ref, tol)
        worst = max(worst, r)
        if n or not _untouched(buf, M, out.shape[1]):
            fails.append((M, n, round(r, 3), _untouched(buf, M, out.shape[1])))
    print(f"gar_1b {name} {pro}/{epi}, M = 1 .. 64: worst |err| / bound {worst:.3f}")
    assert not fails, f"(M, elements out of bound, worst err / bound, rows >= M untouched): {fails}"


@pytest.mark.parametrize("cfg,dt", [("gar_1b", torch.bfloat16), ("gar_8b", torch.bfloat16), ("gar_1b", torch.float16)])
@pytest.mark.parametrize("name", ["qkv", "gu", "lm_head"])
def test_gemv_row_gain_of_the_normed_forms(weights, cfg, name, dt):
    """norm_folded and norm_w: |<out_m, ref_m> / <ref_m, ref_m> - 1| <= 1 / (4 K / 64) for every row, before the SwiGLU (gate/up runs
    the same weights with EPI_NONE). One 64-wide K step missing from a row's sum of squares moves the gain by ~ 1 / (2 K / 64)."""
    w = weights(cfg, name, dt)
    K = w.shape[1]
    limit = 1.0 / (4 * K / 64)
    fails = []
    for pro in ("norm_folded", "norm_w"):
        if (pro, "none") not in FORMS[name] and (pro, "swiglu") not in FORMS[name]:
            continue
        worst = 0.0
        for M in _ms(name, pro):
            out, ref, _, _ = _run(w, pro, "none", M, dt, seed=1, pitch=_pitch(name, w.shape[0]))
            dev = (row_gain(out, ref) - 1).abs()
            d = float(torch.nan_to_num(dev, nan=float("inf")).max())
            worst = max(worst, d)
            if not d <= limit:
                fails.append((pro, M, int((~(dev <= limit)).sum()), d))
        print(f"{cfg} {name} {tuple(w.shape)} {pro} {str(dt)[6:]}: worst |row gain - 1| {worst:.3e} (limit {limit:.3e})")
    assert not fails, f"limit {limit:.3e}; (prologue, M, rows beyond it, worst |gain - 1|): {fails}"


def _split_k(w, M, split, dt):
    """`down` as K slices: every f32 partial against the f64 product of its own K range (the bound without the output rounding), then
    gar_splitk_residual_rmsnorm on them: h within the per-element bound of h0 + x W^T, the norm output against the f64 RMSNorm of
    the ROUNDED h (two roundings, as the ABI states: tests/gemv_ref.py rmsnorm_ref) -> failures"""
    from gar_amd import hip, ops
    N, K = w.shape
    x, g = _activations(M, K, "plain", M * 131 + split, dt)
    part = torch.full((split, M, N), float("nan"), device="cuda")
    ops.gemm(x, w, None, partial=part)
    torch.cuda.synchronize()
    fails, ks = [], K // split
    for j in range(split):
        rj, tj = gemv_ref(x[:, j * ks:(j + 1) * ks], w[:, j * ks:(j + 1) * ks], hip.EPI_NONE, dt=dt)
        n, r = _ratio(part[j], rj, tj - rj.abs() * OUT_EPS[dt])
        if n:
            fails.append(("slice", j, M, n, round(r, 3)))
    h0 = torch.randn(M, N, generator=g, device="cuda").to(dt)
    gain = (1 + 0.1 * torch.randn(N, generator=g, device="cuda")).to(dt)
    h = h0.clone()
    y = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
    ops.splitk_residual_rmsnorm(part, h, gain, EPS, out=y)
    torch.cuda.synchronize()
    ref, tol = gemv_ref(x, w, hip.EPI_RES, h0, dt=dt)
    n, r = _ratio(h, ref, tol)
    if n:
        fails.append(("h", M, n, round(r, 3)))
    yr, ty = rmsnorm_ref(h, gain, EPS, dt)
    n, r2 = _ratio(y, yr, ty)
    if n:
        i = int(torch.nan_to_num((y.double() - yr).abs() / ty, nan=float("inf")).argmax())
        fails.append(("norm", M, n, round(r2, 3), "worst element: out, ref", float(y.view(-1)[i]), float(yr.view(-1)[i])))
    return fails, r, r2


@pytest.mark.parametrize("cfg,split", [("gar_1b", 4), ("gar_8b", 2), ("gar_1b", 2), ("gar_8b", 4)])
def test_gemv_split_k_partials_and_fused_reduce(weights, cfg, split):
    """the model's slice counts (4 at hidden 2048, 2 at 4096) and their neighbours, at both `down` shapes — GAR-8B's (4096, 14336)
    is the one tests/test_gpu_ops.py::test_decode_gemm_split_k_and_fused_reduce never ran"""
    w = weights(cfg, "down")
    fails, wh, wy = [], 0.0, 0.0
    for M in MS:
        f, r, r2 = _split_k(w, M, split, torch.bfloat16)
        fails += f
        wh, wy = max(wh, r), max(wy, r2)
    print(f"{cfg} down {tuple(w.shape)} split_k {split}: worst |err| / bound of h {wh:.3f}, of the norm output {wy:.3f}")
    assert not fails, fails


def _lda(M):
    """(M - 1) * lda * 2 bytes > 2 GiB: buffer descriptors take 32-bit offsets, the launcher takes the per-lane fragment loads"""
    return ((2 ** 30) // (M - 1)) // 64 * 64 + 128


@pytest.mark.parametrize("name,M", [("o", 2), ("lm_head", 3), ("gu", 33), ("qkv", 20)])
def test_gemv_per_lane_fragment_path(weights, name, M):
    """STAGED = false of the 16-bit kernels, which no contiguous activation reaches: half tile with EPI_RES (o), NORM 1 (lm_head),
    NT 4 with NORM 2 and SwiGLU (gate/up), MT 2 with NORM 2 (qkv)"""
    pro, epi = FORMS[name][0]
    w = weights("gar_1b", name)
    out, ref, tol, buf = _run(w, pro, epi, M, lda=_lda(M), pitch=_pitch(name, w.shape[0]))
    n, r = _ratio(out, ref, tol)
    print(f"gar_1b {name} {pro}/{epi} M = {M}, per-lane fragment path: worst |err| / bound {r:.3f}")
    assert n == 0 and _untouched(buf, M, out.shape[1]), (name, M, n, r)


def test_gemv_per_lane_fragment_path_equals_staged_bits(weights):
    """o at M = 2: the same activations behind a 2-GiB row pitch (per-lane fragment loads, 8-row half tiles) and in a small
    contiguous buffer (the staged DEEP ring) give the same output BITS: both launch 8 waves over the 32 K steps of K = 2048, every
    wave adds its 4 steps in order, and the merge adds the waves in order"""
    w = weights("gar_1b", "o")
    far, _, _, _ = _run(w, "plain", "res", 2, lda=_lda(2))
    near, _, _, _ = _run(w, "plain", "res", 2)
    assert torch.equal(far.view(torch.int16), near.view(torch.int16)), int((far.view(torch.int16) != near.view(torch.int16)).sum())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N", [2048, 768])
@pytest.mark.parametrize("ksteps", [7, 13])
def test_gemv_ragged_k_split(N, ksteps, dt):
    """K steps that do not divide over the waves (per = ceil(ksteps / nw): the last wave is short), at N = 2048 (half tiles, and
    the deep ring at M <= 8) and N = 768, every prologue and the residual epilogue, with the LDS poisoned first"""
    K = 64 * ksteps
    g = torch.Generator(device="cuda").manual_seed(N + ksteps)
    w = (torch.randn(N, K, generator=g, device="cuda") * 0.02).to(dt)
    fails = []
    for pro, epi in (("plain", "none"), ("plain", "res"), ("norm_folded", "none"), ("norm_w", "none")):
        for M in _ms("ragged", pro, (1, 8, 9, 33)):
            out, ref, tol, buf = _run(w, pro, epi, M, dt, rows=80, poison=True)
            n, r = _ratio(out, ref, tol)
            if n or not _untouched(buf, M, N):
                fails.append((pro, epi, M, n, round(r, 3)))
    assert not fails, fails
