"""GPU (-m gpu): generate(num_return_sequences = N) — gar_attention_decode_fanout (decode attention over a prompt prefix shared
by N sibling rows plus each row's private suffix) against the float64 restatement of tests/fanout_util.py and against the
existing gar_attention_decode_qkv on replicated caches, then GARModel.generate end to end: the oracle's draws from the run's own
logits, f32 against today's generate on the repeat_interleave'd batch, 16-bit against the replicated 16-bit path."""
import itertools

import numpy as np
import pytest
import torch

import fanout_util as F
from parity_util import F32_LOGIT_TOL

pytestmark = pytest.mark.gpu

HALF = [torch.bfloat16, torch.float16]
MARGIN = 2e-5           # tests/test_gpu_sampling.py: how close to a CDF boundary a draw may sit and land on the neighbour
# 16-bit fan-out against the replicated 16-bit path, both measured by their rows' relative L2 against the f32 fan-out run on the
# same forced tokens: worst fan-out row <= HALF_RATIO_MARGIN x worst replicated row. Measured on an MI355X: ratio
# 0.988 / 0.995 (tiny bf16 / fp16), 1.080 / 1.003 (GAR-1B dims) — the two paths differ in f32 summation order and in the running
# max a 16-bit P value was rounded under; the margin is the project's 1.5 x measured: 1.5 x 1.080.
HALF_RATIO_MARGIN = 1.62


def tol(dt):            # tests/test_gpu_ops.py's constants
    return {torch.bfloat16: 1.6e-2, torch.float16: 2e-3}[dt]


def _up(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def dev():
    from gar_amd import hip
    hip.require_device(0)
    return torch.device("cuda:0")


def _kernel_case(dev, dt, hd, strip, B, N, P, padded, t, g):
    """one launch of each form on the same inputs; returns the checked figures"""
    from gar_amd import ops
    Hq, Hkv = 8, 2
    R, Wd = B * N, (Hq + 2 * Hkv) * hd
    Sp, T = _up(P, 256), _up(t + 1, 64)
    Smax = Sp + T
    lp_list = [min(v, P - 1) for v in ((37, P - 1, 101)[:B] if padded else (0,) * B)]
    lp = torch.tensor(lp_list, dtype=torch.int32, device=dev)
    lpR = lp.repeat_interleave(N)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev).to(dt)
    Kp, Vp = rn(B, Hkv, Sp, hd), rn(B, Hkv, Sp, hd)
    Kp[:, :, P:], Vp[:, :, P:] = 0, 0                       # rows behind the prompt: zero, as the states allocate them
    Ks, Vs = rn(R, Hkv, T, hd), rn(R, Hkv, T, hd)
    Ks[:, :, t:], Vs[:, :, t:] = 0, 0
    x = rn(R, Wd)
    if strip:
        x = x[:, ops.llm_qkv_weight_order(hd, Hq, Hkv).to(dev)].contiguous()
    pos = torch.arange(Smax, dtype=torch.float32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    fr = (pos[:, None] * inv[None]).to(dev)
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    qs = hd ** -0.5 * 1.4426950408889634
    # the replicated batch: R full caches, the generated rows behind the prompt's
    Kf, Vf = (torch.zeros(R, Hkv, Smax, hd, dtype=dt, device=dev) for _ in range(2))
    Kf[:, :, :P], Vf[:, :, :P] = Kp.repeat_interleave(N, 0)[:, :, :P], Vp.repeat_interleave(N, 0)[:, :, :P]
    Kf[:, :, P:P + t], Vf[:, :, P:P + t] = Ks[:, :, :t], Vs[:, :, :t]
    posd = torch.tensor([P + t], dtype=torch.int32, device=dev)
    Q1 = torch.empty(R, Hq, 1, hd, dtype=dt, device=dev)
    K2, V2 = Kf.clone(), Vf.clone()
    ops.llm_qkv_post(x, cos, sin, Q1, K2, V2, R, 1, 1, Hq, Hkv, hd, Smax, 0, posd, qs, left_pad=lpR, strip_order=strip)
    ns_rep = max(1, min(8, 192 // (R * Hkv)))
    ws = torch.empty(ops.attention_decode_workspace(R, Hq, hd, ns_rep), dtype=torch.uint8, device=dev)
    o_rep = torch.full((R, Hq * hd), float("nan"), dtype=dt, device=dev)
    assert ops.attention_decode_qkv(x, cos, sin, Kf, Vf, o_rep, R, Hq, Hkv, hd, Smax, posd, qs, ns_rep, ws, left_pad=lpR,
                                    strip_order=strip)
    # the fan-out launch
    ns = max(1, min(8, 192 // (B * Hkv * -(-N // 8))))
    wsf = torch.empty(ops.attention_decode_fanout_workspace(R, Hq, hd, ns), dtype=torch.uint8, device=dev)
    o = torch.full((R, Hq * hd), float("nan"), dtype=dt, device=dev)
    Kp0, Vp0, Ks0, Vs0 = Kp.clone(), Vp.clone(), Ks.clone(), Vs.clone()
    cnt = torch.tensor([t, 0, 0, P], dtype=torch.int32, device=dev)
    ops.attention_decode_fanout(x, cos, sin, Kp, Vp, Ks, Vs, o, B, N, Hq, Hkv, hd, Sp, T, cnt[3:4], cnt[0:1], qs, ns, wsf,
                                left_pad=lp, strip_order=strip)
    ref = F.batched_attention(Q1.view(R, Hq, hd), K2, V2, lpR, P + t + 1).reshape(R, Hq * hd)
    torch.cuda.synchronize()
    what = (dt, hd, strip, B, N, P, lp_list, t)
    assert torch.equal(Kp, Kp0) and torch.equal(Vp, Vp0), ("prompt cache written", what)
    assert torch.equal(Ks[:, :, t], K2[:, :, P + t]) and torch.equal(Vs[:, :, t], V2[:, :, P + t]), ("appended row", what)
    keep = torch.arange(T, device=dev) != t
    assert torch.equal(Ks[:, :, keep], Ks0[:, :, keep]) and torch.equal(Vs[:, :, keep], Vs0[:, :, keep]), ("other suffix rows", what)
    scale = max(float(ref.abs().max()), 1e-6)
    e_ref = float((o.double() - ref).abs().max()) / scale
    e_rep = float((o.double() - o_rep.double()).abs().max()) / scale
    assert e_ref <= tol(dt) and e_rep <= 2 * tol(dt), (what, e_ref, e_rep)
    return e_ref, e_rep


@pytest.mark.parametrize("strip", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dt", HALF)
def test_fanout_kernel_against_f64_and_replicated(dev, dt, hd, strip):
    """every (N, B, P, left_pad, t) of the issue's list: O within tol(dt) of the float64 result's scale and within 2 tol(dt) of
    gar_attention_decode_qkv on R replicated caches; the appended suffix rows bit-equal to gar_llm_qkv_post's; the prompt caches
    and the other suffix rows untouched"""
    g = torch.Generator(device=dev).manual_seed(1000 + hd + 7 * int(strip))
    worst = [0.0, 0.0]
    n = 0
    for N, B, P, padded, t in itertools.product((1, 2, 3, 4, 8, 16), (1, 3), (1, 63, 64, 1000, 4718), (False, True),
                                                (0, 1, 63, 64, 65)):
        e = _kernel_case(dev, dt, hd, strip, B, N, P, padded, t, g)
        worst = [max(a, b) for a, b in zip(worst, e)]
        n += 1
    print(f"fanout kernel {dt} hd {hd} strip {strip}: {n} cases, worst err / scale vs f64 {worst[0]:.3g} (bound {tol(dt):.3g}), "
          f"vs replicated {worst[1]:.3g} (bound {2 * tol(dt):.3g})")


# ---- end to end -------------------------------------------------------------------------------------------------------------
SAMPLING = dict(do_sample=True, temperature=0.8, top_p=0.9)


def _tiny_setup(n=3):
    from gar_amd import GARConfig
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    from test_gpu_e2e import _left_pad_batch, _lengthen, _sample
    cfg = GARConfig.tiny()
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    base = [_sample(cfg, proc, i) for i in (3, 4, 6)]
    ss = [_lengthen(x, e, 300 + i) for i, (x, e) in enumerate(zip(base, (0, 21, 21)))]      # two different prompt lengths
    return cfg, synthetic_weights(cfg), _left_pad_batch(ss[:n])


def _gc(cfg, n, N, **kw):
    V = cfg.mllm_config.text_config.vocab_size
    return dict(SAMPLING, top_k=min(50, V), max_new_tokens=n, num_return_sequences=N, **kw)


def _repeat(batch, N):
    """the replicated batch: what HF's repeat_interleave(N) of the inputs gives"""
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            B = batch["input_ids"].shape[0]
            out[k] = v.reshape(B, -1, *v.shape[1:]).repeat_interleave(N, 0).reshape(-1, *v.shape[1:]) if v.shape[0] != B \
                else v.repeat_interleave(N, 0)
        elif isinstance(v, list):
            out[k] = [x for x in v for _ in range(N)]
        else:
            out[k] = v
    return out


def _check_draws(cfg, seq, logits, seed, skip_after=None):
    """2(a): every token is the oracle's draw from the run's own logits (seed, row, step); returns the near-miss count"""
    from oracle import sampling as S
    V = cfg.mllm_config.text_config.vocab_size
    seq, lg = seq.cpu(), logits.float().cpu().numpy()
    near = total = 0
    for r in range(seq.shape[0]):
        for j in range(seq.shape[1]):
            if skip_after is not None and skip_after[r] is not None and j >= skip_after[r]:
                continue                        # behind the row's eos: padding, not a draw
            exp, margin, keep = S.sample(lg[r, j, :V], 0.8, min(50, V), 0.9, seed, r, j)
            tok = int(seq[r, j])
            assert keep[tok], (r, j, tok)
            total += 1
            if tok != exp:
                assert margin < MARGIN, (r, j, tok, exp, margin)
                near += 1
    assert near <= max(1, total // 100), (near, total)
    return near


def test_fanout_f32_tiny_end_to_end(dev):
    """3 left-padded prompts of two lengths x N = 4, 12 tokens, f32 (parity mode: one prompt phase, the prompt's cache rows
    copied to the B * N rows, the plain step)"""
    from gar_amd.modeling_gar import GARModel
    cfg, W, batch = _tiny_setup()
    B, N, NT = 3, 4, 12
    m = GARModel(cfg, W, torch.float32)
    greedy0 = m.generate(**batch, max_new_tokens=NT).sequences.cpu()
    one0 = m.generate(**batch, generation_config=_gc(cfg, NT, 1), seed=5).sequences.cpu()
    out = m.generate(**batch, generation_config=_gc(cfg, NT, N), seed=777, return_logits=True)
    seq = out.sequences.cpu()
    assert tuple(seq.shape) == (B * N, NT) and tuple(out.logits.shape)[:2] == (B * N, NT)
    _check_draws(cfg, seq, out.logits, 777)                                                     # (a)
    for b in range(B):                                                                          # (b)
        assert len({tuple(r.tolist()) for r in seq[b * N:(b + 1) * N]}) == N, b
        assert all(torch.equal(out.logits[b * N, 0], out.logits[b * N + i, 0]) for i in range(N))
    eager = m.generate(**batch, generation_config=_gc(cfg, NT, N), seed=777, use_graph=False).sequences.cpu()
    assert torch.equal(eager, seq)
    assert torch.equal(m.generate(**batch, num_return_sequences=N, seed=777, max_new_tokens=NT, top_k=_gc(cfg, NT, N)["top_k"],
                                  **SAMPLING).sequences.cpu(), seq)                             # keywords; the same seed repeats
    assert not torch.equal(m.generate(**batch, generation_config=_gc(cfg, NT, N), seed=778).sequences.cpu(), seq)
    # (c) forced on (a)'s tokens: today's generate on the replicated batch, same seed, same forced tokens
    fan = m.generate(**batch, generation_config=_gc(cfg, NT, N), seed=777, return_logits=True, forced_tokens=seq)
    rep = m.generate(**_repeat(batch, N), generation_config=_gc(cfg, NT, 1), seed=777, return_logits=True, forced_tokens=seq)
    err = float((fan.logits - rep.logits).abs().max())
    bound = F32_LOGIT_TOL * float(rep.logits.abs().max())
    print(f"f32 fan-out vs replicated, forced: max |dlogit| {err:.3g} (bound {bound:.3g})")
    assert err <= bound, (err, bound)
    _check_draws(cfg, fan.sequences, fan.logits, 777)
    # (d) per-row eos latching: an eos id that some siblings draw early and others do not
    col = seq[:, 3].tolist()
    eos = max(set(col), key=col.count)
    hit = [next((j + 1 for j, tk in enumerate(r.tolist()) if tk == eos), None) for r in seq]
    assert any(h is not None and h < NT for h in hit) and any(h is None or h == NT for h in hit), hit
    pad = 1
    e = m.generate(**batch, generation_config=_gc(cfg, NT, N, eos_token_id=eos, pad_token_id=pad), seed=777, sync_every=4)
    es = e.sequences.cpu()
    for r in range(B * N):
        end = hit[r] if hit[r] is not None else NT
        assert es[r, :min(end, es.shape[1])].tolist() == seq[r, :min(end, es.shape[1])].tolist(), r
        assert all(int(v) == pad for v in es[r, end:]), (r, es[r].tolist())
    # 6: the other paths of the same model object are untouched
    assert torch.equal(m.generate(**batch, max_new_tokens=NT).sequences.cpu(), greedy0)
    assert torch.equal(m.generate(**batch, generation_config=_gc(cfg, NT, 1), seed=5).sequences.cpu(), one0)


def _rel_l2_rows(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return [float((a[r] - b[r]).norm() / b[r].norm()) for r in range(a.shape[0])]


@pytest.mark.parametrize("which", ["tiny", "gar1b"])
def test_fanout_half_against_replicated_half(dev, which):
    """3: bf16 / fp16 through the shared kernel, teacher-forced on the f32 fan-out run's tokens: worst row's relative L2 against
    the f32 fan-out logits, compared with the same figure of the unchanged replicated 16-bit path"""
    from gar_amd import GARConfig, ops
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    from test_gpu_e2e import _left_pad_batch, _sample
    if which == "tiny":
        cfg, W, batch = _tiny_setup()
        N, NT = 4, 12
    else:
        cfg = GARConfig.gar_1b(**{"vision.depth": 1, "text.num_hidden_layers": 2})
        W = synthetic_weights(cfg)
        proc = GARProcessor.from_config(cfg, max_num_tiles=2)
        batch = _left_pad_batch([_sample(cfg, proc, 3, 300, 220), _sample(cfg, proc, 4, 300, 220)])
        N, NT = 4, 8
    gc = _gc(cfg, NT, N)
    ref = GARModel(cfg, W, torch.float32).generate(**batch, generation_config=gc, seed=31, return_logits=True)
    forced = ref.sequences
    for dt in HALF:
        m = GARModel(cfg, W, dt)
        hb = {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
        n0 = ops.FANOUT_LAUNCHES
        fan = m.generate(**hb, generation_config=gc, seed=31, return_logits=True, forced_tokens=forced)
        L = cfg.mllm_config.text_config.num_hidden_layers
        assert ops.FANOUT_LAUNCHES - n0 >= L, "the shared-prefix kernel did not run"
        n1 = ops.FANOUT_LAUNCHES
        rep = m.generate(**_repeat(hb, N), generation_config=_gc(cfg, NT, 1), seed=31, return_logits=True, forced_tokens=forced)
        assert ops.FANOUT_LAUNCHES == n1
        assert torch.isfinite(fan.logits).all()
        e_fan, e_rep = max(_rel_l2_rows(fan.logits, ref.logits)), max(_rel_l2_rows(rep.logits, ref.logits))
        print(f"{which} {dt}: worst row rel L2 vs f32 — fan-out {e_fan:.4g}, replicated {e_rep:.4g}, ratio {e_fan / e_rep:.3f}")
        assert e_fan <= HALF_RATIO_MARGIN * e_rep, (which, dt, e_fan, e_rep)
        _check_draws(cfg, fan.sequences, fan.logits, 31)
        eager = m.generate(**hb, generation_config=gc, seed=31, forced_tokens=forced, use_graph=False)
        assert torch.equal(eager.sequences, fan.sequences)


def test_fanout_with_fp8_decode_weights_and_row_limit(dev):
    """4: decode_weight_dtype="fp8" with B * N = 8 passes the draw check; B * N = 65 hits the decode-row refusal"""
    from gar_amd import hip
    from gar_amd.modeling_gar import GARModel
    cfg, W, two = _tiny_setup(2)
    m = GARModel(cfg, W, torch.bfloat16, decode_weight_dtype="fp8")
    half = lambda d: {k: (v.to(torch.bfloat16) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in d.items()}
    out = m.generate(**half(two), generation_config=_gc(cfg, 12, 4), seed=9, return_logits=True)
    assert tuple(out.sequences.shape) == (8, 12)
    _check_draws(cfg, out.sequences, out.logits, 9)
    with pytest.raises(hip.GarError, match="decodes at most"):
        m.generate(**half(_tiny_setup(1)[2]), generation_config=_gc(cfg, 4, 65), seed=9)


@pytest.mark.parametrize("kind", ["multi", "video"])
def test_fanout_multi_mask_and_video_prompts(dev, kind):
    """5: N = 2 over a multi-mask prompt and a video-replay prompt: shapes, the draw check, and first-token logits bit-equal to
    the N = 1 call's (the same prompt phase)"""
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    from gar_amd.weights import synthetic_weights
    from test_gpu_e2e import _sample, _video_sample
    cfg = GARConfig.tiny()
    proc = GARProcessor.from_config(cfg, max_num_tiles=4)
    dt = torch.bfloat16
    s = _sample(cfg, proc, 0, dtype=dt, multi=True) if kind == "multi" else _video_sample(cfg, proc, 3, dtype=dt)
    m = GARModel(cfg, synthetic_weights(cfg), dt)
    one = m.generate(**s, generation_config=_gc(cfg, 8, 1), seed=3, return_logits=True)
    two = m.generate(**s, generation_config=_gc(cfg, 8, 2), seed=3, return_logits=True)
    assert tuple(two.sequences.shape) == (2, 8)
    assert torch.equal(two.logits[0, 0], one.logits[0, 0]) and torch.equal(two.logits[1, 0], one.logits[0, 0])
    _check_draws(cfg, two.sequences, two.logits, 3)
    assert int(two.sequences[0, 0]) == int(one.sequences[0, 0])         # row 0, step 0: the same draw from the same logits


def test_fanout_states_do_not_leak_and_refusals(dev):
    """6 on a 16-bit model (shared prompt cache, own graphs): greedy and N = 1 sampling before and after a fan-out call are
    identical; the pipelined driver and the fp8 KV cache refuse N > 1 by name"""
    from gar_amd import hip
    from gar_amd.modeling_gar import GARModel
    cfg, W, batch = _tiny_setup()
    dt = torch.bfloat16
    hb = {k: (v.to(dt) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    m = GARModel(cfg, W, dt)
    g0 = m.generate(**hb, max_new_tokens=12).sequences.cpu()
    s0 = m.generate(**hb, generation_config=_gc(cfg, 12, 1), seed=5).sequences.cpu()
    f0 = m.generate(**hb, generation_config=_gc(cfg, 12, 4), seed=5).sequences.cpu()
    assert torch.equal(m.generate(**hb, max_new_tokens=12).sequences.cpu(), g0)
    assert torch.equal(m.generate(**hb, generation_config=_gc(cfg, 12, 1), seed=5).sequences.cpu(), s0)
    assert torch.equal(m.generate(**hb, generation_config=_gc(cfg, 12, 4), seed=5).sequences.cpu(), f0)
    with pytest.raises(hip.GarError, match="num_return_sequences"):
        m.generate_pipelined([hb], generation_config=_gc(cfg, 4, 2), seed=1)
    with pytest.raises(hip.GarError, match="num_return_sequences"):
        m.generate(**hb, num_return_sequences=2, max_new_tokens=4)                      # greedy + N > 1
    m8 = GARModel(cfg, W, dt, kv_cache_dtype="fp8")
    with pytest.raises(hip.GarError, match="fp8"):
        m8.generate(**hb, generation_config=_gc(cfg, 4, 2), seed=1)


def test_demo_cli_prints_n_sampled_captions(dev, tmp_path):
    """demo/gar_with_mask.py --num_return_sequences N: N lines, repeatable under --seed; without the flag one greedy caption"""
    import os
    import subprocess
    import sys

    from PIL import Image

    from gar_amd.synthetic import synthetic_image, synthetic_mask
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ip, mp = str(tmp_path / "img.png"), str(tmp_path / "mask.png")
    synthetic_image(11, 300, 220).save(ip)
    Image.fromarray(synthetic_mask(11, 300, 220).astype(np.uint8) * 255).save(mp)

    def run(*args):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "grasp-any-region_amd")]), PYTHONHASHSEED="0")
        r = subprocess.run([sys.executable, os.path.join(root, "demo", "gar_with_mask.py"), "--synthetic_weights", "--model_name_or_path",
                            "tiny", "--data_type", "bf16", "--max_num_tiles", "4", "--max_new_tokens", "12", "--image_path", ip,
                            "--mask_path", mp, *args], capture_output=True, text=True, timeout=600, env=env,
                           cwd=os.path.join(root, "demo"))
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.rstrip("\n").split("\n")
    three = run("--num_return_sequences", "3", "--temperature", "0.8", "--seed", "7")
    assert len(three) == 3 and len(set(three)) > 1, three
    assert run("--num_return_sequences", "3", "--temperature", "0.8", "--seed", "7") == three
    assert len(run()) == 1
