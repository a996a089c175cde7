"""GARModel — host-side sequencing of the region-captioning hot path on one MI355X.

Keeps the call surface of the reference's ``GARModel`` (projects/grasp_any_region/hf_models/modeling_gar.py):
``model.config.prompt_numbers``, ``model.generate(input_ids=, attention_mask=, pixel_values=, global_mask_values=,
bboxes=, aspect_ratios=, generation_config=, return_dict=)`` -> object with ``.sequences`` (new tokens only, :418-426),
``get_image_features`` (modeling_perception_lm.py:239-269).  Everything numeric is a HIP kernel behind the C ABI
(``gar_amd.ops``); this file only allocates buffers, orders launches and captures the decode step in a hipGraph.

Differences by design: the mask conv + patch-embed conv are one im2col GEMM; ``_merge`` and the fp32
copy of the feature map are never materialised (``gar_roi_replay`` indexes the tile layout); placeholder / crop-token
bookkeeping runs on the device, so ``generate`` has no host sync before the first EOS check.
"""
from __future__ import annotations

import gc
import math
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import hip, ops
from .beam_search import BeamBudgetError, BeamSearch
from .constrained import PhraseConstraint
from .configuration_gar import GARConfig
from .logits_processing import LogitsProcessing, _Refused as _ProcessingRefused
from .sampling_warpers import SamplingWarpers
from .planner import plan_chunks
from .weights import LM, PJ, VT, check_weights, load_weights, normalize_checkpoint, synthetic_weights

LOG2E = 1.4426950408889634


# 16-bit element types: the fused bf16 kernels serve both (libgar_hip.so / its twin libgar_hip_f16.so, hip.lib(dtype))
HALF_DTYPES = (torch.bfloat16, torch.float16)

class _PendingGeneration:
    """What generate_begin hands to generate_finish: the KV state (slot) the prompt was prefilled into and the loop's settings."""
    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.ready = None


@dataclass
class GenerateOutput:
    sequences: torch.Tensor                      # [B, n_new] int64 (only new tokens, as with inputs_embeds in HF)
    logits: Optional[torch.Tensor] = None        # [B, n_new, V] when return_logits=True (tests)
    # validate=False only: device int32 [1], OR of the INPUT_* bits below found by the device-side checks (0 = the
    # inputs were what validate=True would have accepted). Reading it is the caller's sync; generate() itself raises on it
    # wherever it synchronises anyway (EOS polls).
    input_flags: Optional[torch.Tensor] = None
    # GenerationPipeline only: event on the decode stream behind this output's last kernel — a consumer on another stream
    # (the caller's) waits for it before it reads ``sequences``
    done: Optional[object] = None
    # return_logprobs=True only: the log-probability of every token of ``sequences``, written by the launch that
    # chose it. A row counts up to and including its first eos; the columns behind it (``pad`` in ``sequences``) hold 0.
    token_logprobs: Optional[torch.Tensor] = None           # f32 [B * N, n]: x[tok] - logsumexp(x) over the raw logits
    token_logprobs_warped: Optional[torch.Tensor] = None    # f32 [B * N, n]: under the warped distribution the token was drawn
    #                                                         from (temperature, top-k, top-p); greedy search: equal to the raw one
    sum_logprobs: Optional[torch.Tensor] = None             # f32 [B * N]
    sum_logprobs_warped: Optional[torch.Tensor] = None      # f32 [B * N]
    n_tokens: Optional[torch.Tensor] = None                 # int32 [B * N]: counted tokens per row
    # top_logprobs=k / candidate_token_ids=[...] only: RAW log-probabilities x[i] - logsumexp(x) of every step's logits,
    # also under do_sample. Columns behind a row's first eos hold id -1 and value 0.0.
    top_logprob_ids: Optional[torch.Tensor] = None          # int64 [B * N, n, k]: the k most likely tokens, best first, equal logits
    #                                                         by ascending id — entry 0 is the greedy token
    top_logprobs: Optional[torch.Tensor] = None             # f32 [B * N, n, k]: their log-probabilities
    candidate_logprobs: Optional[torch.Tensor] = None       # f32 [B * N, n, C]: log-probabilities of candidate_token_ids, in their order
    # beam_search=BeamSearch(...) only: ``sequences`` is [B * num_return_sequences, n], each prompt's hypotheses best
    # first, ``pad`` behind each one's end; this is each one's sum of log-probabilities / length ** length_penalty
    sequences_scores: Optional[torch.Tensor] = None         # f32 [B * num_return_sequences]
    # constraint=PhraseConstraint(...) only: the index, in the row's prompt's list, of the phrase the row completed —
    # its tokens before its first eos, or all of them when max_new_tokens cut it, are exactly one phrase — else -1 (host tensor)
    phrase_index: Optional[torch.Tensor] = None             # int32 [B * N]


class _PickTargets(NamedTuple):
    """where a pick (GARModel._pick) writes: the token matrix, the current tokens and the eos latches of its rows, the batch row of
    its first row (the Philox row counter of a draw), the (raw, warped) log-probability planes of a return_logprobs request or
    None, the planes of a top_logprobs / candidate_token_ids request (GARModel._topk_planes) or None, the rows' own request
    words (int32 [rows, 8], gar_sample_rows) of a state that carries them or None, and the rows' own processing blocks (int32
    [rows, LOGITS_PROCESS_WORDS], gar_logits_process_rows) of a state that carries them or None, and the rows of the node plane
    (int32 [rows, cols + 1], gar_constrain) of a request with a phrase constraint or None."""
    out_tokens: torch.Tensor
    cur: torch.Tensor
    finished: torch.Tensor
    row0: int
    lp: Optional[tuple]
    tk: Optional[dict]
    row_words: Optional[torch.Tensor] = None
    row_proc: Optional[torch.Tensor] = None
    nodes: Optional[torch.Tensor] = None

    @classmethod
    def of(cls, st, out_tokens) -> "_PickTargets":          # every row of a state
        return cls(out_tokens, st["cur"], st["finished"], 0, st.get("lp"), st.get("tk"), st.get("row_words"), st.get("row_proc"),
                   st.get("nodes"))

    def rows(self, r0: int, r1: int) -> "_PickTargets":
        """cut to rows r0 .. r1 - 1: a prompt chunk's first-token head"""
        tk = self.tk and dict(self.tk, **{n: self.tk[n][r0:r1] for n in ("ids", "lp", "cand_lp") if self.tk[n] is not None})
        return _PickTargets(self.out_tokens[r0:r1], self.cur[r0:r1], self.finished[r0:r1], self.row0 + r0,
                            self.lp and tuple(p[r0:r1] for p in self.lp), tk,
                            None if self.row_words is None else self.row_words[r0:r1],
                            None if self.row_proc is None else self.row_proc[r0:r1],
                            None if self.nodes is None else self.nodes[r0:r1])


def _process_blocks(rows) -> torch.Tensor:
    """host int32 [len(rows), LOGITS_PROCESS_WORDS]: every row's words (continuous.pack_process_row) in front, zeros behind"""
    blocks = torch.zeros((len(rows), ops.LOGITS_PROCESS_WORDS), dtype=torch.int32)
    for b, words in enumerate(rows):
        blocks[b, :len(words)] = torch.tensor(words, dtype=torch.int32)
    return blocks


def logprob_outputs(raw: torch.Tensor, warped: torch.Tensor, finished_at: Sequence[Optional[int]]):
    """The log-probability fields of a :class:`GenerateOutput` from the planes the decode steps wrote ([R, n] f32, one column
    per step) and ``finished_at`` (per row: number of tokens up to and including its first eos, None = no eos among the n):
    (token_logprobs, token_logprobs_warped, sum_logprobs, sum_logprobs_warped, n_tokens), 0 in the columns behind a row's eos
    (ScoreOutput's "0 where ignored"). Torch ops on the planes' device; nothing is read back."""
    R, n = raw.shape
    ends = torch.tensor([n if f is None else min(int(f), n) for f in finished_at], dtype=torch.int64, device=raw.device)
    keep = torch.arange(n, device=raw.device)[None, :] < ends[:, None]
    zero = torch.zeros((), dtype=raw.dtype, device=raw.device)
    raw, warped = torch.where(keep, raw, zero), torch.where(keep, warped, zero)
    return raw, warped, raw.sum(1), warped.sum(1), ends.to(torch.int32)


def top_logprob_options(top_logprobs, candidate_token_ids, V: int):
    """(k, candidate id list) of a generate(top_logprobs=, candidate_token_ids=) request, checked against the vocabulary size and
    gar_topk_lp's limits. ValueError names what is refused."""
    k = top_logprobs
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= min(ops.TOPK_MAX, V):
        raise ValueError(f"top_logprobs={k!r}: an int in 0..{min(ops.TOPK_MAX, V)} (min({ops.TOPK_MAX}, vocab_size = {V}))")
    cands = [] if candidate_token_ids is None else list(candidate_token_ids)
    if len(cands) > ops.TOPK_CAND_MAX:
        raise ValueError(f"candidate_token_ids: {len(cands)} ids, at most {ops.TOPK_CAND_MAX}")
    for c in cands:
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < V:
            raise ValueError(f"candidate_token_ids: id {c!r} is outside [0, vocab_size = {V})")
    return k, [int(c) for c in cands]


def top_logprob_outputs(tk, n: int, finished_at: Sequence[Optional[int]]):
    """The top_logprob_ids / top_logprobs / candidate_logprobs fields from a state's planes ([R, T, k] / [R, T, C], one column per
    step), masked as :func:`logprob_outputs` masks: behind a row's first eos ids are -1 and values 0.0."""
    dev = tk["cand_lp"].device if tk["ids"] is None else tk["ids"].device
    ends = torch.tensor([n if f is None else min(int(f), n) for f in finished_at], dtype=torch.int64, device=dev)
    keep = (torch.arange(n, device=dev)[None, :] < ends[:, None])[:, :, None]
    out = {}
    if tk["ids"] is not None:
        out["top_logprob_ids"] = torch.where(keep, tk["ids"][:, :n].to(torch.int64), torch.full((), -1, dtype=torch.int64, device=dev))
        out["top_logprobs"] = torch.where(keep, tk["lp"][:, :n], torch.zeros((), dtype=torch.float32, device=dev))
    if tk["cand_lp"] is not None:
        out["candidate_logprobs"] = torch.where(keep, tk["cand_lp"][:, :n], torch.zeros((), dtype=torch.float32, device=dev))
    return out


INPUT_COUNT_MISMATCH, INPUT_SPAN_LENGTH, INPUT_MISSING_BBOX, INPUT_ID_RANGE, INPUT_MASK_NOT_LEFT_PADDED = 1, 2, 4, 8, 16
INPUT_LABEL_RANGE = 32          # score(validate=False): a label outside [0, vocab) and not -100 (set by gar_xent_combine)


def phrase_indices(constraint: PhraseConstraint, rows, eos, fanout: int = 1) -> torch.Tensor:
    """GenerateOutput.phrase_index of a constrained request from its ``sequences`` (as lists): row r belongs to prompt r // fanout"""
    return torch.tensor([constraint.phrase_index(r // fanout, row, eos) for r, row in enumerate(rows)], dtype=torch.int32)


def describe_input_flags(flags: int) -> str:
    names = {INPUT_COUNT_MISMATCH: "image token count != image feature rows (reference: ValueError)",
             INPUT_SPAN_LENGTH: "a crop-token span is not P*P long (the reference's splice would change the sequence length)",
             INPUT_MISSING_BBOX: "a crop token present in input_ids has no bbox (reference: KeyError)",
             INPUT_ID_RANGE: "input_ids outside [0, vocab)",
             INPUT_MASK_NOT_LEFT_PADDED: "attention_mask is not LEFT-padded (a row is not 0...01...1): HF generation would continue "
                                         "such a row after its padding",
             INPUT_LABEL_RANGE: "labels outside [0, vocab) other than -100 (ignored; validate=True raises ValueError)"}
    return "; ".join(v for k, v in names.items() if flags & k)


@dataclass
class ScoreOutput:
    """:meth:`GARModel.score`: teacher-forced log-probabilities, all on the device."""
    token_logprobs: torch.Tensor                 # f32 [B, S]: log p(labels[t] | prefix) at column t; 0 where ignored
    sum_logprobs: torch.Tensor                   # f32 [B]
    n_tokens: torch.Tensor                       # int32 [B]: scored tokens per row
    loss: torch.Tensor                           # f32 0-dim: -sum / count over the batch (HF's mean; NaN with no token)
    input_flags: Optional[torch.Tensor] = None   # validate=False only: int32 [1], INPUT_* bits (INPUT_LABEL_RANGE included)


def score_targets(input_ids: torch.Tensor, labels: torch.Tensor, crop_ids: Sequence[int],
                  attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The label semantics of the reference's loss (modeling_gar.py:176-190 + HF's causal-LM shift), in torch ops on the
    labels' device, no host sync: int64 [B, S - 1], entry t = the target of row t (its next token), -100 where ignored.
    Inside each crop token's span (first to last occurrence), which the RoI replay replaces, labels become -100. With a
    left-padding ``attention_mask``, a padding row predicts nothing, so the first real token is not scored (as in the
    unpadded run)."""
    ids = input_ids.to(labels.device, torch.int64)
    lab = labels.to(torch.int64).clone()
    B, S = ids.shape
    col = torch.arange(S, device=lab.device)[None, :]
    for c in crop_ids:
        hit = ids == int(c)
        first = torch.where(hit, col, S).min(1).values[:, None]
        last = torch.where(hit, col, -1).max(1).values[:, None]
        lab = lab.masked_fill((col >= first) & (col <= last), -100)
    tgt = lab[:, 1:]
    if attention_mask is not None:
        tgt = tgt.masked_fill(~(attention_mask.to(lab.device) != 0)[:, :-1], -100)
    return tgt


def causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """HF's ForCausalLMLoss restated: logits cast to f32, labels shifted by one, cross-entropy with ignore_index=-100, mean
    over the tokens that remain (NaN with none)."""
    lg = logits.float()[:, :-1].reshape(-1, logits.shape[-1])
    return torch.nn.functional.cross_entropy(lg, labels[:, 1:].reshape(-1).to(lg.device), ignore_index=-100, reduction="mean")


# GenerationConfig fields the reference forwards to HF's generate (modeling_gar.py:418-426) that would change the tokens of a
# greedy search and are NOT implemented here: name -> the value(s) that leave greedy search unchanged. Anything else raises
# instead of being ignored (the reference's own callers pass max_new_tokens / do_sample=False / eos / pad only).
_NEUTRAL_GENERATION_OPTIONS = {
    "num_beams": (None, 1), "num_beam_groups": (None, 1), "penalty_alpha": (None, 0, 0.0), "repetition_penalty": (None, 1, 1.0),
    "encoder_repetition_penalty": (None, 1, 1.0), "length_penalty": (None, 1, 1.0), "no_repeat_ngram_size": (None, 0),
    "diversity_penalty": (None, 0, 0.0), "bad_words_ids": (None,), "force_words_ids": (None,), "constraints": (None,),
    "forced_bos_token_id": (None,), "forced_eos_token_id": (None,), "suppress_tokens": (None,), "begin_suppress_tokens": (None,),
    "sequence_bias": (None,), "min_length": (None, 0), "min_new_tokens": (None, 0), "num_return_sequences": (None, 1),
    "prompt_lookup_num_tokens": (None,), "assistant_model": (None,),
}
# sampling-only knobs: without do_sample they do not touch greedy search (HF warns and ignores them) — accepted
_SAMPLING_ONLY_OPTIONS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


# keywords generate() accepts besides its own parameters: the generation options it reads or refuses by value
_GENERATION_KWARGS = set(_NEUTRAL_GENERATION_OPTIONS) | {"do_sample", "temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff",
                                                          "eta_cutoff", "max_new_tokens", "eos_token_id", "pad_token_id", "use_cache",
                                                          "return_dict_in_generate", "output_scores", "output_logits", "output_attentions",
                                                          "synced_gpus", "streamer", "labels"}


class _OverlaidOptions:
    """generation options: keyword arguments laid over a GenerationConfig / dict (HF: `generate(generation_config, **kwargs)`)"""

    def __init__(self, base_get, over):
        self._base, self._over = base_get, over

    def get(self, k, d=None):
        return self._over[k] if k in self._over else self._base(k, d)


def _option_reader(generation_config, generate_kwargs):
    """``get(name, default)`` over the options of a request: a GenerationConfig object or a dict, with the keyword arguments of the
    call laid over it (HF: `generate(generation_config, **kwargs)`). None when the request carries no option at all."""
    gc = generation_config
    if generate_kwargs:
        # the reference forwards **generate_kwargs to HF's generate (modeling_gar.py:418-426), which lays them OVER the generation
        # config: the same here — an option passed as a keyword is read (and refused if not built) like one in the config, never
        # swallowed; a keyword that is no generation option at all is an error as it is in HF
        unknown = sorted(k for k in generate_kwargs if k not in _GENERATION_KWARGS)
        if unknown:
            raise TypeError(f"generate() got unexpected keyword arguments {unknown} (generation options: see GenerationConfig)")
        base = gc
        base_get = (lambda k, d=None: d) if base is None else \
            ((lambda k, d=None: base.get(k, d)) if isinstance(base, dict) else (lambda k, d=None: getattr(base, k, d)))
        gc = _OverlaidOptions(base_get, dict(generate_kwargs))
    if gc is None:
        return None
    return gc.get if isinstance(gc, (dict, _OverlaidOptions)) else (lambda k, d=None: getattr(gc, k, d))


def _num_return_sequences(get, kv_cache_dtype=None) -> int:
    """N of a request (HF: ``sequences`` is [B * N, n], row b * N + i = sample i of prompt b). N > 1 needs do_sample = True — without
    it :func:`_refuse_non_greedy` refuses the option as before — and the 16-bit KV cache."""
    v = get("num_return_sequences")
    if v is None:
        return 1
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"`num_return_sequences` has to be an integer >= 1, but is {v!r}")
    if v > 1 and get("do_sample", False) and kv_cache_dtype == "fp8":
        raise hip.GarError(f"num_return_sequences={v} with kv_cache_dtype='fp8' is not implemented (the shared-prefix decode "
                           "attention reads 16-bit caches)")
    return v


def _fanout_rows(b0: int, b1: int, N: int):
    """rows of the expanded batch that prompts b0 .. b1 - 1 fan out to: prompt b owns rows b * N .. b * N + N - 1, and row r is
    also the Philox row counter of its draws — what the replicated batch (repeat_interleave(N) of the inputs) would use"""
    return b0 * N, b1 * N


# the refused options that generate(logits_processing=...) provides under a parameter of its own
_LOGITS_PROCESSING_FIELDS = ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "min_length", "suppress_tokens",
                             "begin_suppress_tokens", "bad_words_ids")


# the refused options that generate(beam_search=...) provides under a parameter of its own
_BEAM_SEARCH_FIELDS = ("num_beams", "length_penalty")


def _refuse_non_greedy(get):
    for name, neutral in _NEUTRAL_GENERATION_OPTIONS.items():
        v = get(name)
        if name == "num_return_sequences" and get("do_sample", False):
            continue                                        # sampling: read by _num_return_sequences
        if not any((v is n) or (n is not None and not isinstance(v, bool) and v == n) for n in neutral):
            hint = " — pass generate(logits_processing=LogitsProcessing(...)) instead" if name in _LOGITS_PROCESSING_FIELDS else \
                (" — pass generate(beam_search=BeamSearch(...)) instead" if name in _BEAM_SEARCH_FIELDS else "")
            raise hip.GarError(f"generation option {name}={v!r} is not implemented (greedy search only: it would change the tokens "
                               f"and is refused rather than ignored){hint}")


def _sampling_options(get):
    """(temperature, top_p, top_k) of a do_sample = True request, with HF's defaults (GenerationConfig: temperature 1.0, top_k 50,
    top_p 1.0) and HF's argument checks (TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper). The warpers that are not
    read from the options (min_p, typical_p, epsilon / eta cutoff) are refused when they would act: they come under
    generate(sampling_warpers=...), DESIGN 7.9."""
    for name, neutral in (("min_p", (None, 0, 0.0)), ("typical_p", (None, 1, 1.0)), ("epsilon_cutoff", (None, 0, 0.0)),
                          ("eta_cutoff", (None, 0, 0.0))):
        v = get(name)
        if not any((v is n) or (n is not None and not isinstance(v, bool) and v == n) for n in neutral):
            raise hip.GarError(f"sampling option {name}={v!r} is not implemented (temperature, top_k and top_p are) — pass "
                               "generate(sampling_warpers=SamplingWarpers(...)) instead")
    temperature = get("temperature", 1.0)
    temperature = 1.0 if temperature is None else float(temperature)
    if not temperature > 0:
        raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")
    top_k = get("top_k", 50)
    top_k = 0 if top_k is None else int(top_k)
    if top_k < 0:
        raise ValueError(f"`top_k` has to be a non-negative integer (0 = off), but is {top_k}")
    top_p = get("top_p", 1.0)
    top_p = 1.0 if top_p is None else float(top_p)
    if not 0 < top_p <= 1.0:
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
    return temperature, top_p, top_k


def _draw_seed() -> int:
    """the Philox key of a sampled request that names none. HF draws from torch's global generator: so does this key
    (torch.manual_seed reproduces it)"""
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        # identically seeded data-parallel ranks must not replay one stream on different regions
        seed = (seed ^ (0x9E3779B97F4A7C15 * (torch.distributed.get_rank() + 1))) & (2 ** 62 - 1)
    return seed


def _round_up(x, m):
    return (x + m - 1) // m * m


def _rope2d_tables(v) -> (torch.Tensor, torch.Tensor):
    """timm RotaryEmbeddingCat tables: host-side constant generation, fp32."""
    hd, g, nb = v.head_dim, v.grid, v.head_dim // 4
    bands = 1.0 / (v.rope_temperature ** (torch.arange(0, nb, dtype=torch.int64).to(torch.float32) / nb))
    t = torch.arange(g, dtype=torch.int64).to(torch.float32) + v.rope_grid_offset
    g0, g1 = torch.meshgrid(t, t, indexing=v.rope_grid_indexing)
    pos = torch.stack([g0, g1], dim=-1).unsqueeze(-1) * bands
    sin = pos.sin().reshape(g * g, -1).repeat_interleave(2, -1)
    cos = pos.cos().reshape(g * g, -1).repeat_interleave(2, -1)
    return sin.contiguous(), cos.contiguous()


def _llama_inv_freq(t) -> torch.Tensor:
    """HF rope init incl. rope_type 'llama3' (SURVEY.md A.4): host-side constant generation, fp32."""
    dim = t.head_dim
    inv = 1.0 / (t.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.int64).to(torch.float32) / dim))
    sc = t.rope_scaling
    if sc and sc.get("rope_type", sc.get("type", "llama3")) == "llama3":
        factor, low, high, old = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"], \
            sc["original_max_position_embeddings"]
        wavelen = 2 * math.pi / inv
        inv_l = torch.where(wavelen > old / low, inv / factor, inv)
        smooth = (old / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        med = ~(wavelen < old / high) * ~(wavelen > old / low)
        inv = torch.where(med, smoothed, inv_l)
    return inv


def _on_model_device(fn):
    """Run a public entry point with the model's device current: the C ABI launches on the current HIP device and
    ``hip.stream()`` hands it torch's current stream of THAT device, so a model on cuda:1 must not enqueue on device 0."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        with torch.cuda.device(self.device):
            return fn(self, *a, **kw)
    return wrapped


class _InputEmbeddings:
    """callable returned by ``get_input_embeddings()``: ids [...] -> rows of embed_tokens [..., C] (gar_embed_lookup)."""

    def __init__(self, model):
        self._m = model
        self.weight = model.E

    def __call__(self, input_ids: torch.Tensor) -> torch.Tensor:
        m = self._m
        with torch.cuda.device(m.device):
            ids = input_ids.to(m.device, torch.int64).contiguous()
            out = torch.empty(*ids.shape, m.E.shape[1], dtype=m.dtype, device=m.device)
            if ids.numel():
                ops.embed_lookup(ids.view(-1), m.E, out.view(-1, m.E.shape[1]))
        return out


class _MllmFacade:
    """``model.mllm`` of the reference's GARModel (modeling_gar.py:47-50): the helper calls its generate() makes
    (:332-346) for callers that script the stages themselves. Each method is the HIP kernel ``generate`` itself uses
    (or a pure index view); the reference's own callers in scope never touch them."""

    def __init__(self, model):
        self._m = model
        self.config = model.config.mllm_config

    @property
    def dtype(self):
        return self._m.dtype

    @property
    def device(self):
        return self._m.device

    def get_input_embeddings(self):
        return _InputEmbeddings(self._m)

    def get_image_features(self, pixel_values, mask_embeds=None, global_mask_values=None, **kw):
        """modeling_perception_lm.py:239-269, the reference's signature: ``mask_embeds`` [T, C_v, g, g] is the output of
        ``model.mask_patch_embedding`` (modeling_gar.py:326-337) and is added to the patch embeddings
        (modeling_perception_lm.py:195-196). ``generate`` does not come through here: it hands the processor's
        ``global_mask_values`` to the patch-embed GEMM, which carries the mask convolution as extra K columns; that form is
        available to callers too (``global_mask_values=``; not both)."""
        if mask_embeds is not None and global_mask_values is not None:
            raise hip.GarError("pass either mask_embeds (the reference's form) or global_mask_values (the fused form), not both")
        return self._m.get_image_features(pixel_values, global_mask_values, mask_embeds=mask_embeds)

    def get_placeholder_mask(self, input_ids, inputs_embeds, image_features=None, video_features=None):
        """(special_image_mask, special_video_mask) expanded to ``inputs_embeds``' shape, with the reference's count check
        (modeling_perception_lm.py:271-331) — from gar_placeholder_scan's slot table."""
        m = self._m
        if input_ids is None:
            raise hip.GarError("get_placeholder_mask needs input_ids (the embeds-only form of the reference is not built)")
        with torch.cuda.device(m.device):
            ids = input_ids.to(m.device, torch.int64).contiguous()
            B, S = ids.shape
            masks = []
            for tok, feats, what in ((self.config.image_token_id, image_features, "Image"),
                                     (self.config.video_token_id, video_features, "Videos")):
                slot = torch.empty(B, S, dtype=torch.int32, device=m.device)
                counts = torch.empty(B, dtype=torch.int32, device=m.device)
                spans = torch.empty(B, 1, 2, dtype=torch.int32, device=m.device)
                ops.placeholder_scan(ids, tok, m.crop_ids_dev[:1], slot, counts, spans)
                n_tok = int(counts.sum().item())
                if feats is not None and n_tok * inputs_embeds.shape[-1] != feats.numel():
                    raise ValueError(f"{what} features and image tokens do not match: tokens: {n_tok}, features "
                                     f"{feats.numel() // feats.shape[-1]}")
                masks.append((slot >= 0).unsqueeze(-1).expand_as(inputs_embeds))
        return masks[0], masks[1]


class _MaskPatchEmbedding:
    """``model.mask_patch_embedding`` of the reference (nn.Conv2d(3, C_v, 14, 14, bias=False), modeling_gar.py:54-60) as a
    callable: binary mask tiles [T, 3, H, W] -> mask embeddings [T, C_v, g, g] (modeling_gar.py:326-328). The mask half of the
    patch-embed GEMM run on its own (gar_patch_embed with zero weights in the pixel slots, or gar_patch_im2col + gar_gemm); the
    result is a channel-first VIEW of token-major storage, which is what ``mllm.get_image_features(mask_embeds=)`` reads."""

    def __init__(self, model):
        self._m = model

    @property
    def weight(self):       # [C_v, 3, p, p], reconstructed from the fused patch-embed operand (fp32 master in model dtype)
        m = self._m
        v = m.config.mllm_config.vision_config
        pp = v.patch_size * v.patch_size
        return m.w_patch[:, 3 * pp:6 * pp].reshape(-1, 3, v.patch_size, v.patch_size)

    def __call__(self, binary_mask: torch.Tensor) -> torch.Tensor:
        return self._m._mask_embed(binary_mask)


class GenerationPipeline:
    """Software pipeline over consecutive ``generate`` calls: the decode loop of batch i on a second HIP stream, the prompt
    phase (vision tower, sequence assembly, prefill) of batch i + 1 on the caller's stream, two KV-state slots. The decode step
    is HBM-bound (weights and KV cache stream, matrix pipes idle), the prompt phase MFMA-bound: wherever the hardware can
    co-schedule their workgroups — under the attention kernels and at kernel boundaries; the persistent tile GEMM owns its
    CUs — the decode loop costs no wall time. Same kernels on the same data as ``model.generate``: bit-identical outputs.

    ``submit(sample)`` returns the outputs that became available (at most one, of the previous batch; stream-ordered, not
    host-synchronised), ``flush()`` the last one and makes the caller's stream wait for the decode stream."""

    PRIORITY = 0        # of the decode stream (-1 = high)

    def __init__(self, model: "GARModel", **generate_kwargs):
        if generate_kwargs.get("beam_search") is not None:
            raise hip.GarError("GenerationPipeline / generate_pipelined: beam_search is not implemented (call generate)")
        if generate_kwargs.get("constraint") is not None:
            raise hip.GarError("constraint with GenerationPipeline / generate_pipelined is not implemented (DESIGN 7.13): call generate")
        self.model, self.kwargs = model, generate_kwargs
        self.side = None
        self.done = {}              # slot -> event: that slot's previous decode loop has finished
        self.prev = None
        self.n = 0

    def _finish(self, pend):
        m = self.model
        if self.side is None:
            with torch.cuda.device(m.device):
                self.side = torch.cuda.Stream(device=m.device, priority=self.PRIORITY)
        self.side.wait_event(pend.ready)
        with torch.cuda.device(m.device), torch.cuda.stream(self.side):
            out = m.generate_finish(pend)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.done[pend.st["slot"]] = out.done = ev
        return out

    def submit(self, sample) -> List[GenerateOutput]:
        m = self.model
        outs = []
        # Without EOS polling the decode loop enqueues without a host sync: put it in flight FIRST, so that nothing the prompt
        # phase's host code waits for can delay it. With EOS polling generate_finish blocks the host until its batch is done:
        # then the next prompt phase has to be enqueued before it.
        early = self.prev is not None and not self.prev.eos
        if early:
            outs.append(self._finish(self.prev))
            self.prev = None
        if sample.get("beam_search") is not None:
            raise hip.GarError("GenerationPipeline / generate_pipelined: beam_search is not implemented (call generate)")
        if sample.get("constraint") is not None:
            raise hip.GarError("constraint with GenerationPipeline / generate_pipelined is not implemented (DESIGN 7.13): call generate")
        slot = self.n & 1
        self.n += 1
        with torch.cuda.device(m.device):
            main = torch.cuda.current_stream(m.device)
            if slot in self.done:
                main.wait_event(self.done[slot])            # the prefill overwrites that slot's cache, counters and token buffer
            pend = m.generate_begin(**sample, **self.kwargs, state_slot=slot)
            if pend.N > 1:
                raise hip.GarError(f"GenerationPipeline / generate_pipelined: num_return_sequences={pend.N} is not implemented "
                                   "(call generate)")
            pend.ready = torch.cuda.Event()
            pend.ready.record(main)
        if self.prev is not None:
            outs.append(self._finish(self.prev))
        self.prev = pend
        return outs

    def flush(self) -> List[GenerateOutput]:
        outs = []
        if self.prev is not None:
            outs.append(self._finish(self.prev))
            self.prev = None
        if self.side is not None:
            with torch.cuda.device(self.model.device):
                torch.cuda.current_stream(self.model.device).wait_stream(self.side)
        return outs


class GARModel:
    # bf16: the LayerNorms of the ViT blocks and the RMSNorms of the Llama prefill are folded into the GEMM pairs around
    # them (gar_gemm_params.row_scale / row_stats): the consumer GEMM reads the residual stream itself with a weight that
    # carries gamma (and, for LayerNorm, centred rows), the producer GEMM's epilogue writes the row statistics — the
    # stand-alone norm passes (3.3 % of a step, at HBM bandwidth) disappear
    FOLD_NORMS = True
    # bf16 with FOLD_NORMS: RoPE, q scale and the KV-cache append run in the Llama prefill qkv GEMM's epilogue
    # (GAR_EPI_QKV_ROPE_LLM) — no [B*S, (Hq + 2 Hkv) hd] intermediate, no llm_qkv_post pass
    LLM_QKV_EPILOGUE = True
    DECODE_GU_NORM_FOLDED = True  # bf16, 16 < B <= 64: post-attention RMSNorm inside the gate/up GEMM (gar_gemm_params.norm_folded)
    DECODE_ATTN_TAKES_QKV = True  # bf16: the decode attention launch does llm_qkv_post's work (gar_attention_decode_qkv)
    VIT_CLS_KEY_FOLD = True       # bf16: the cls key / value row enters the ViT attention through the initial softmax state
    VIT_V_ROW_MAJOR = True        # bf16: v leaves the qkv GEMM head-major, gar_attention_vrow transposes on its LDS reads
    # split-KV decode attention: kv splits per (sequence, kv head) so that ~DECODE_ATTN_BLOCKS workgroups exist, at most
    # DECODE_ATTN_MAX_SPLITS — measured optimum at kv ~ 4.75k (tools/bench_decode_attn.py, hipGraph replays, round 4): B = 1 / 2 / 4:
    # 8 splits (12.0 us against 21.9 with the 64 splits a 512-block target gave: more splits = a longer combine launch and more
    # partial-block overhead than bytes in flight are worth), B = 8: 2-4, B = 12: 2, B >= 16: 1 (no combine launch)
    DECODE_ATTN_BLOCKS = 192
    DECODE_ATTN_MAX_SPLITS = 8
    FUSE_NORM_MAX_BATCH = 16      # largest decode batch that keeps `down` un-split (f32 / plain weights: RMSNorm in the GEMV prologue)
    # The LAST Llama layer of a prefill computes attention / o / gate-up / down for the last prompt row of every sequence only:
    # the head reads nothing else (modeling_perception_lm.py:545-552, `lm_head(hidden_states[:, slice_indices, :])`) and the
    # decode steps read the layer's K / V rows, which the qkv GEMM still writes for every row. Exact w.r.t. the reference,
    # which computes and discards the other S - 1 rows; 2.5 % of a region's GEMM + attention work at GAR-1B / 1024^2.
    PRUNE_LAST_PREFILL_LAYER = True

    def __init__(self, config: GARConfig, weights: Dict[str, torch.Tensor], dtype: torch.dtype = torch.bfloat16,
                 device: str = "cuda:0", prefill_chunk: Optional[int] = None, keep_plain_weights: bool = False,
                 kv_cache_dtype: Optional[str] = None, decode_weight_dtype: Optional[str] = None):
        self.device = torch.device(device)
        # the decode KV cache: None / "auto" = the model dtype; "fp8" = OCP e4m3fn bytes + one f32 scale per (layer, row, kv head,
        # position), K and V apart (include/gar_hip.h, FP8 KV cache). A property of the model, like its dtype: one model = one
        # configuration. The prompt's own attention stays 16-bit, so prefill logits and the first token do not change.
        if kv_cache_dtype not in (None, "auto", "fp8"):
            raise hip.GarError(f"kv_cache_dtype {kv_cache_dtype!r}: None, 'auto' or 'fp8'")
        self.kv_fp8 = kv_cache_dtype == "fp8"
        if self.kv_fp8 and dtype not in HALF_DTYPES:
            raise hip.GarError(f"kv_cache_dtype='fp8' needs a 16-bit model (bfloat16 / float16), not {dtype}: "
                               "float32 is the parity mode")
        self.kv_cache_dtype = "fp8" if self.kv_fp8 else None
        # the weights the decode GEMVs stream: None / "auto" = the prepared 16-bit weights; "fp8" = e4m3 copies with one f32 scale
        # per output row (include/gar_hip.h, FP8 weights) of every Llama layer's qkv / o / gate-up / down operand and of lm_head,
        # read by decode steps 2 and later. The prompt phase (vision tower, prefill, first token) keeps the 16-bit weights, which
        # stay resident beside the copies (decode_weight_fp8_bytes). Decode batches above 64 rows run on the tile GEMM: refused.
        if decode_weight_dtype not in (None, "auto", "fp8"):
            raise hip.GarError(f"decode_weight_dtype {decode_weight_dtype!r}: None, 'auto' or 'fp8'")
        self.w_fp8 = decode_weight_dtype == "fp8"
        if self.w_fp8 and dtype not in HALF_DTYPES:
            raise hip.GarError(f"decode_weight_dtype='fp8' needs a 16-bit model (bfloat16 / float16), not {dtype}: "
                               "float32 is the parity mode")
        self.decode_weight_dtype = "fp8" if self.w_fp8 else None
        self._w8: Dict[int, tuple] = {}
        # bf16 keeps ONE copy of every weight: the norm-folded forms (ViT qkv / fc1, Llama qkv / gate-up) serve the tile GEMMs
        # (row_scale), the decode GEMVs (norm_folded) and — behind a unit-gain norm pass — the shapes neither takes.
        # keep_plain_weights=True also keeps the un-folded copies (+1.6 GB GAR-1B, +11 GB GAR-8B): A/B switch for FOLD_NORMS = False
        self.keep_plain_weights = bool(keep_plain_weights)
        hip.require_device(self.device.index or 0)
        self.config = config
        self.dtype = dtype
        self.prompt_numbers = config.prompt_numbers
        self.crop_tokens_ids = list(config.crop_tokens_ids)
        check_weights(config, weights)
        with torch.cuda.device(self.device):
            self._prepare_weights(weights)
            self._pack_weights()
            if self.w_fp8:
                self._build_w8()
        self.mllm = _MllmFacade(self)
        self.mask_patch_embedding = _MaskPatchEmbedding(self)
        self._mask_only_w = {}
        self._ws: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self._graphs: Dict[tuple, object] = {}
        self._llm_lru: List[tuple] = []
        self._video_crop_ids: Dict[tuple, torch.Tensor] = {}
        # None: the vision tower runs over chunks of image TILES and the prefill over chunks of SEQUENCES, both chosen by
        # gar_amd.planner so that the persistent tile GEMMs run whole rounds (decode serves all B at once).
        # An int pins both passes to chunks of that many regions (the pre-planner behaviour; bench.py --prefill-chunk).
        self.prefill_chunk = None if prefill_chunk is None else int(prefill_chunk)

    # ---- construction -------------------------------------------------------------------------------------------
    @classmethod
    def from_synthetic(cls, config: GARConfig, seed: int = 0, dtype=torch.bfloat16, device="cuda:0", **kw):
        return cls(config, synthetic_weights(config, seed), dtype, device, **kw)

    @classmethod
    def from_pretrained(cls, path: str, dtype=torch.bfloat16, device="cuda:0", config: GARConfig = None,
                        kv_cache_dtype: Optional[str] = None, decode_weight_dtype: Optional[str] = None):
        import os
        if config is None:
            config = GARConfig.from_json_file(os.path.join(path, "config.json"))
        return cls(config, normalize_checkpoint(config, load_weights(path)), dtype, device, kv_cache_dtype=kv_cache_dtype,
                   decode_weight_dtype=decode_weight_dtype)

    @classmethod
    def from_shapes(cls, config: GARConfig, dtype=torch.bfloat16, device="cuda:0", **kw):
        """Replica with UNINITIALISED device weights of the right shapes — to be filled by ``broadcast_weights``
        (non-source ranks of the data-parallel runner never touch host weights)."""
        from .weights import weight_shapes
        W = {k: torch.empty(s, dtype=dtype, device=device) for k, s in weight_shapes(config).items()}
        return cls(config, W, dtype, device, **kw)

    def _weight_slots(self):
        """where every prepared weight tensor lives: (container, key, index-in-tuple or None), in a fixed order"""
        own = self.__dict__
        slots = [(own, "w_patch", None), (own, "pos", None), (own, "norm_pre", 0), (own, "norm_pre", 1)]
        slots += [(self.pj, k, None) for k in self.pj]
        slots += [(own, "E", None), (own, "final_norm", None)]
        if self.cls is not None:
            slots.append((own, "cls", None))
        if self.w_patch_gather is not None:
            slots.append((own, "w_patch_gather", None))
        if self.lm_head is not self.E:
            slots.append((own, "lm_head", None))
        for d in list(self.vblocks) + list(self.layers):
            for k, v in d.items():
                slots += [(d, k, i) for i in range(len(v))] if isinstance(v, tuple) else [(d, k, None)]
        return slots

    def weight_tensors(self) -> List[torch.Tensor]:
        return [c[k] if i is None else c[k][i] for c, k, i in self._weight_slots()]

    def _pack_weights(self):
        """Move every prepared weight into ONE allocation per dtype (``self.arenas``) and re-bind the tensors as views of it: the
        data-parallel weight exchange is then one in-place RCCL broadcast per arena — no concatenated bucket
        copies — and a replica's weights are one contiguous range of HBM."""
        from .weights import pack_arenas
        tied = self.lm_head is self.E
        slots = self._weight_slots()
        self.arenas, views = pack_arenas([c[k] if i is None else c[k][i] for c, k, i in slots])
        for (c, k, i), v in zip(slots, views):
            if i is None:
                c[k] = v
            else:
                c[k] = tuple(v if j == i else x for j, x in enumerate(c[k]))
        if tied:
            self.lm_head = self.E

    @_on_model_device
    def broadcast_weights(self, src: int = 0):
        """RCCL broadcast of the prepared weights from rank ``src``: one collective per dtype arena, in place (one-off)."""
        from .dp import broadcast_arenas
        n = broadcast_arenas(self.arenas, src)
        self._mask_only_w.clear()       # derived from w_patch / w_patch_gather (mask_patch_embedding): rebuilt from the new weights
        if self.w_fp8:                  # derived too: re-quantized in place from the received weights (deterministic: every rank
            self._build_w8()            # holds the same bytes; captured decode graphs keep their pointers)
        return n

    def weight_arena_bytes(self) -> int:
        return sum(a.numel() * a.element_size() for a in self.arenas.values())

    def decode_weight_fp8_bytes(self) -> int:
        """device bytes of the e4m3 decode-weight copies and their scales (decode_weight_dtype="fp8"; 0 otherwise), held in
        addition to weight_arena_bytes()"""
        return sum(q.numel() + 4 * sc.numel() for q, sc in self._w8.values())

    def _build_w8(self):
        """(Re)build the e4m3 copies the decode GEMVs read: every Llama layer's qkv / o / gate-up / down operand (qkv_f with its
        permuted rows when folded) and lm_head — a copy when it is tied to E, which embed_lookup keeps reading in 16 bits. Keyed
        by the 16-bit tensor's data_ptr; an existing copy is rewritten in place."""
        names = ("qkv_f", "o", "gu_f", "down") if self._decode_uses_folded_w() else ("qkv", "o", "gu", "down")
        srcs = [ly[k] for ly in self.layers for k in names] + [self.lm_head]
        old, self._w8 = self._w8, {}
        for w in srcs:
            q, sc = old.get(w.data_ptr(), (None, None))
            self._w8[w.data_ptr()] = ops.weight_quantize_fp8(w, q, sc)

    def _check_decode_rows(self, rows: int, what: str):
        """decode_weight_dtype="fp8" decodes on the skinny GEMV only: more rows would run on the 16-bit tile GEMM, with other
        numerics and no notice, so they are refused"""
        if getattr(self, "w_fp8", False) and rows > self.W8_MAX_ROWS:
            raise hip.GarError(f"{what}: decode_weight_dtype='fp8' decodes at most {self.W8_MAX_ROWS} rows, not {rows} (larger "
                               "decode batches run on the 16-bit tile GEMM)")

    def _decode_uses_folded_w(self) -> bool:
        """the decode step's qkv / gate-up operands: the norm-folded weights (qkv_f / gu_f) or the plain ones (qkv / gu)"""
        ly = self.layers[0]
        return "qkv_f" in ly and (self.FOLD_NORMS or "qkv" not in ly)

    def _gemm_w8(self, a, w, out, *args, **kw):
        """ops.gemm on the e4m3 copy of the prepared 16-bit weight ``w`` (decode steps of a decode_weight_dtype="fp8" model)"""
        if w.data_ptr() not in self._w8:
            raise hip.GarError("decode_weight_dtype='fp8': this decode operand has no e4m3 copy (the copies follow FOLD_NORMS as it "
                               "was at construction)")
        q, sc = self._w8[w.data_ptr()]
        return ops.gemm(a, q, out, *args, w_scale=sc, **kw)

    def eval(self):
        return self

    def get_input_embeddings(self):
        """modeling_gar.py:67-68"""
        return _InputEmbeddings(self)

    @staticmethod
    def _merge(tiles: torch.Tensor, ncw: int, nch: int) -> torch.Tensor:
        """modeling_gar.py:248-260: [B, nch*ncw, C, th, tw] tiles -> [B, C, nch*th, ncw*tw] image. A pure index permutation;
        ``generate`` never materialises it (gar_roi_replay indexes the tile layout), kept for callers that want the map."""
        b, n, c, th, tw = tiles.shape
        assert n == ncw * nch, f"{ncw * nch} != {n}"
        return tiles.view(b, nch, ncw, c, th, tw).permute(0, 3, 1, 4, 2, 5).contiguous().view(b, c, nch * th, ncw * tw)

    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        return t.to(device=self.device, dtype=self.dtype).contiguous()

    def _prepare_weights(self, W: Dict[str, torch.Tensor]):
        cfg = self.config
        v, t = cfg.mllm_config.vision_config, cfg.mllm_config.text_config
        pp = v.patch_size * v.patch_size
        self.Kp = _round_up(6 * pp, 64)
        D = v.embed_dim
        wcat = torch.zeros(D, self.Kp, dtype=torch.float32, device=W[VT + "patch_embed.proj.weight"].device)
        wcat[:, :3 * pp] = W[VT + "patch_embed.proj.weight"].float().flatten(1)
        wcat[:, 3 * pp:6 * pp] = W["mask_patch_embedding.weight"].float().flatten(1)
        d = self._dev
        self.w_patch = d(wcat)
        # the same two conv weights in the K order of gar_patch_embed (patches gathered from the image tiles by the GEMM's
        # DMA): column ((tensor*3 + c)*4 + ky//4)*64 + (ky%4)*16 + kx; zero in the slots no pixel of the patch maps to
        self.w_patch_gather = None
        P_ = v.patch_size
        Kg = ops.patch_embed_k(v.img_size, P_) if self.dtype in HALF_DTYPES else 0
        if Kg:
            wg = torch.zeros(D, 2, 3, 4, 4, 16, dtype=torch.float32, device=wcat.device)
            for ti, key in enumerate((VT + "patch_embed.proj.weight", "mask_patch_embedding.weight")):
                w4 = torch.zeros(D, 3, 16, 16, dtype=torch.float32, device=wcat.device)
                w4[:, :, :P_, :P_] = W[key].float()
                wg[:, ti] = w4.view(D, 3, 4, 4, 16)
            self.w_patch_gather = d(wg.view(D, Kg))
        self.npt = 1 if cfg.mllm_config.vision_use_cls_token else 0
        self.cls = d(W[VT + "cls_token"].reshape(-1)) if self.npt else None
        self.pos = d(W[VT + "pos_embed"].reshape(-1, D))
        self.norm_pre = (d(W[VT + "norm_pre.weight"]), d(W[VT + "norm_pre.bias"]))
        self.vblocks = []
        # The vision attention path is built for head_dim 64, 128 and — bf16 only — 96 (PE-G/14, GAR-8B). Any other head
        # dim (and 96 in the f32 parity mode) runs zero-padded to the next built size: padded q/k/v rows of the fused qkv
        # weight and bias and padded input columns of the output projection are zero (and the RoPE table rotates them by
        # the identity), so scores and outputs are unchanged.
        H, hd = v.num_heads, v.head_dim
        if hd > 128:
            raise hip.GarError(f"vision head_dim {hd} > 128 is not built")
        native = (64, 96, 128) if self.dtype in HALF_DTYPES else (64, 128)
        self.v_hd = hdp = hd if hd in native else (64 if hd < 64 else 128)

        def pad_qkv(w):          # [3*H*hd, ...] -> [3*H*hdp, ...]
            if hdp == hd:
                return w
            w = w.reshape(3, H, hd, *w.shape[1:])
            out = w.new_zeros(3, H, hdp, *w.shape[3:])
            out[:, :, :hd] = w
            return out.reshape(3 * H * hdp, *w.shape[3:])

        def pad_proj(w):         # [D, H*hd] -> [D, H*hdp]
            if hdp == hd:
                return w
            out = w.new_zeros(w.shape[0], H, hdp)
            out[:, :, :hd] = w.reshape(w.shape[0], H, hd)
            return out.reshape(w.shape[0], H * hdp)

        fold = self.dtype in HALF_DTYPES
        plain = not fold or self.keep_plain_weights

        def fold_ln(w, bias, gamma, beta):
            """LN(x) W^T + b = rstd * (x Wc^T) + b': Wc = W diag(gamma) with every row's mean removed (the mean subtraction
            of the LayerNorm is linear and is absorbed by the weight), b' = b + W beta. fp32 in, model dtype out."""
            wg = w.float() * gamma.float()[None, :]
            return d(wg - wg.mean(dim=1, keepdim=True)), d(bias.float() + w.float() @ beta.float())

        for i in range(v.depth):
            b = f"{VT}blocks.{i}."
            blk = {}
            if fold:
                qw, qb = pad_qkv(W[b + "attn.qkv.weight"]), pad_qkv(W[b + "attn.qkv.bias"])
                blk["qkv_wf"], blk["qkv_bf"] = fold_ln(qw, qb, W[b + "norm1.weight"], W[b + "norm1.bias"])
                blk["fc1_wf"], blk["fc1_bf"] = fold_ln(W[b + "mlp.fc1.weight"], W[b + "mlp.fc1.bias"],
                                                       W[b + "norm2.weight"], W[b + "norm2.bias"])
            if plain:
                blk.update(n1=(d(W[b + "norm1.weight"]), d(W[b + "norm1.bias"])),
                           qkv_w=d(pad_qkv(W[b + "attn.qkv.weight"])), qkv_b=d(pad_qkv(W[b + "attn.qkv.bias"])),
                           n2=(d(W[b + "norm2.weight"]), d(W[b + "norm2.bias"])),
                           fc1_w=d(W[b + "mlp.fc1.weight"]), fc1_b=d(W[b + "mlp.fc1.bias"]))
            blk.update(proj_w=d(pad_proj(W[b + "attn.proj.weight"])), proj_b=d(W[b + "attn.proj.bias"]), g1=d(W[b + "gamma_1"]),
                       fc2_w=d(W[b + "mlp.fc2.weight"]), fc2_b=d(W[b + "mlp.fc2.bias"]), g2=d(W[b + "gamma_2"]))
            self.vblocks.append(blk)
        # unit LayerNorm / RMSNorm parameters: a folded weight carries its norm's gain (and bias), so where no folded-norm
        # kernel takes a shape the norm runs as its own pass with gamma = 1, beta = 0 in front of the SAME weight
        self.unit_ln = (torch.ones(D, dtype=self.dtype, device=self.device), torch.zeros(D, dtype=self.dtype, device=self.device)) \
            if fold else None
        self.pj = dict(w1=d(W[PJ + "linear_1.weight"]), b1=d(W[PJ + "linear_1.bias"]),
                       w2=d(W[PJ + "linear_2.weight"]), b2=d(W[PJ + "linear_2.bias"]))
        sin, cos = _rope2d_tables(v)
        if hdp != hd:
            sin = torch.nn.functional.pad(sin, (0, hdp - hd), value=0.0).contiguous()
            cos = torch.nn.functional.pad(cos, (0, hdp - hd), value=1.0).contiguous()
        self.vit_sin, self.vit_cos = sin.to(self.device), cos.to(self.device)
        self.E = d(W[LM + "embed_tokens.weight"])
        self.lm_head = self.E if t.tie_word_embeddings or "mllm.lm_head.weight" not in W else d(W["mllm.lm_head.weight"])
        self.layers = []
        F = t.intermediate_size
        assert F % 16 == 0
        qkv_order = ops.llm_qkv_weight_order(t.head_dim, t.num_attention_heads, t.num_key_value_heads) \
            if (fold and self.LLM_QKV_EPILOGUE and t.head_dim in (64, 128)) else torch.arange((t.num_attention_heads + 2 * t.num_key_value_heads) * t.head_dim)
        self.qkv_f_permuted = bool((qkv_order != torch.arange(qkv_order.numel())).any())
        for i in range(t.num_hidden_layers):
            b = f"{LM}layers.{i}."
            qkv = torch.cat([W[b + "self_attn.q_proj.weight"], W[b + "self_attn.k_proj.weight"],
                             W[b + "self_attn.v_proj.weight"]], dim=0)
            g, u = W[b + "mlp.gate_proj.weight"], W[b + "mlp.up_proj.weight"]
            # [gate16 | up16] row interleave expected by GAR_EPI_SWIGLU
            gu = torch.stack([g.view(F // 16, 16, -1), u.view(F // 16, 16, -1)], dim=1).reshape(2 * F, -1)
            ly = {}
            if fold:          # RMSNorm folded: W diag(g) — the tile GEMM's row_scale form, the decode GEMVs' norm_folded form
                # rows in the order the fused RoPE epilogue wants (identity for head_dim 64): self.qkv_f_permuted
                ly["qkv_f"] = d((qkv.float() * W[b + "input_layernorm.weight"].float()[None, :])[qkv_order])
                ly["gu_f"] = d(gu.float() * W[b + "post_attention_layernorm.weight"].float()[None, :])
            if plain:
                ly.update(ln1=d(W[b + "input_layernorm.weight"]), qkv=d(qkv), ln2=d(W[b + "post_attention_layernorm.weight"]),
                          gu=d(gu))
            ly.update(o=d(W[b + "self_attn.o_proj.weight"]), down=d(W[b + "mlp.down_proj.weight"]))
            self.layers.append(ly)
        self.unit_rms = torch.ones(t.hidden_size, dtype=self.dtype, device=self.device) if fold else None
        self.final_norm = d(W[LM + "norm.weight"])
        self.inv_freq = _llama_inv_freq(t)
        self.crop_ids_dev = torch.tensor(self.crop_tokens_ids, dtype=torch.int64, device=self.device)
        self._rope_cache = {}

    def _llm_rope(self, max_pos: int):
        if max_pos not in self._rope_cache:
            pos = torch.arange(max_pos, dtype=torch.float32)
            fr = pos[:, None] * self.inv_freq[None, :]
            self._rope_cache[max_pos] = (fr.cos().contiguous().to(self.device), fr.sin().contiguous().to(self.device))
        return self._rope_cache[max_pos]

    # Workspaces. Families whose shapes follow the request (tiles of a chunk, prompt length) are CAPACITY based: one flat
    # zero-filled allocation per (family, name) that only grows (x1.25) and is sliced into views, so an evaluation loop
    # with a different prompt length / tile count per item (gar_amd/bench_loops.py) does not allocate per shape.
    # Buffers a captured decode graph points at ("llm", "decode", "head") are keyed by their exact shape and never move;
    # the KV-cache states are kept in an LRU of MAX_LLM_STATES entries (their graphs go with them).
    _CAPACITY_FAMILIES = ("vit", "emb", "prefill", "score")
    MAX_LLM_STATES = 2
    MAX_EOS_IDS = 16          # eos_token_id list entries the device-side stopping criterion holds (longer lists: host scan)
    W8_MAX_ROWS = 64          # gar_gemm_w8 (decode_weight_dtype="fp8") is the skinny GEMV: M <= 64
    SPLITK_MAX_ROWS = 64      # csrc/gemm.hip: split_k > 1 and gar_splitk_residual_rmsnorm are built for M <= 64 rows
    DOWN_SPLIT_K = 0          # K slices of the decode `down` GEMM at more than FUSE_NORM_MAX_BATCH rows: 0 = as many as give the
                              # two-weight-tile blocks of the skinny kernel a full grid — (hidden / 32) * slices >= 256: 4 at
                              # hidden 2048, 2 at 4096 (round 4: four row tiles re-read per ONE weight tile was 4 bytes of L2
                              # traffic per weight byte; GAR-1B 20.4 -> 18.7 us per layer with the reduce, GAR-8B 52.5 -> 44.1;
                              # unsplit 27.3 / 50.1; tools/bench_skinny.py); 1 = off

    def _buf(self, key: tuple, name: str, shape, dtype=None, zero=False):
        dtype = dtype or self.dtype
        if key[0] in self._CAPACITY_FAMILIES:
            n = 1
            for d in shape:
                n *= int(d)
            fam = self._ws.setdefault((key[0],), {})
            flat = fam.get(name)
            if flat is None or flat.dtype != dtype or flat.numel() < n:
                cap = n if flat is None or flat.dtype != dtype else max(n, int(flat.numel() * 1.25))
                flat = torch.zeros(cap, dtype=dtype, device=self.device)      # zero: padding rows must stay finite
                fam[name] = flat
            return flat[:n].view(*shape)
        d = self._ws.setdefault(key, {})
        t = d.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=self.device)
            d[name] = t
        return t

    def workspace_bytes(self) -> int:
        """device bytes held by the cached workspaces (tests / soak checks)."""
        return sum(t.numel() * t.element_size() for d in self._ws.values() for t in d.values())

    # ---- vision tower + projector (A1-A6) -----------------------------------------------------------------------------
    @_on_model_device
    def get_image_features(self, pixel_values: torch.Tensor, global_mask_values: Optional[torch.Tensor] = None,
                           pooled: bool = True, out: Optional[torch.Tensor] = None,
                           mask_embeds: Optional[torch.Tensor] = None):
        """[Tt,3,H,W] (+ mask values of the same shape, still in the processor's [-1,1] encoding) -> [Tt, P*P, C_l].
        ``pooled=False`` stops after the projector and returns its [Tt * tokens, C_l] output (cls rows included),
        written into ``out`` when given. ``mask_embeds`` [Tt, C_v, g, g] (instead of ``global_mask_values``): the reference's
        form — the mask-embedding conv's output, added to the patch embeddings (modeling_perception_lm.py:195-196)."""
        cfg = self.config
        v = cfg.mllm_config.vision_config
        C_l = cfg.mllm_config.text_config.hidden_size
        if pixel_values.dim() == 5:
            pixel_values = pixel_values.flatten(0, 1)
        assert pixel_values.dim() == 4, f"pixel_values should be [tiles, 3, H, W], got {tuple(pixel_values.shape)}"
        pix = pixel_values.to(self.device, self.dtype).contiguous()
        msk = None
        if global_mask_values is not None:
            msk = global_mask_values.to(self.device, self.dtype).reshape(pix.shape).contiguous()
        Tt = pix.shape[0]
        n, D, Dm, H, hd = v.num_patches, v.embed_dim, v.mlp_dim, v.num_heads, self.v_hd     # hd: padded head dim
        Da = H * hd
        N = n + self.npt
        Npad = _round_up(N, 64)
        key = ("vit", Tt)
        x = self._buf(key, "x", (Tt, N, D))
        # zero-initialised once: the fused qkv GEMM writes the N real token rows only, rows N..Npad must stay finite
        Q = self._buf(key, "Q", (Tt, H, Npad, hd), zero=True)
        K = self._buf(key, "K", (Tt, H, Npad, hd), zero=True)
        att = self._buf(key, "att", (Tt * N, Da))
        qkv = Vt = vrow = None             # only the paths that need them allocate them (2.4 GB + 0.9 GB at 387 tiles)
        # bf16 at sizes the ping-pong GEMM takes: q / k leave the qkv GEMM already rotated, scaled and in attention
        # layout (GAR_EPI_QKV_ROPE), only V still needs its transpose; otherwise gemm + vit_qkv_post
        fused = self.dtype in HALF_DTYPES
        # bf16: V stays row-major [Tt, H, Npad, hd] (zero-initialised like Q / K: pad rows must be finite)
        Vr = self._buf(key, "Vr", (Tt, H, Npad, hd), zero=True) if fused and self.VIT_V_ROW_MAJOR else None
        f1 = self._buf(key, "f1", (Tt * N, max(Dm, C_l)))
        x2 = x.view(Tt * N, D)
        gathered = False
        if self.w_patch_gather is not None:
            # patches DMA'd from the image tiles into LDS by the GEMM itself: no im2col matrix (1216 columns per patch
            # written and re-read); the mask decode is one elementwise pass
            mb = self._buf(key, "maskbin", tuple(pix.shape))
            if msk is not None:
                ops.mask_decode(msk, mb, cfg.prompt_numbers)
            else:
                mb.zero_()
            gathered = ops.patch_embed(pix, mb, self.w_patch_gather, self.pos, x, v.patch_size, self.npt)
        if not gathered:
            A = self._buf(key, "im2col", (Tt * n, self.Kp))
            ops.patch_im2col(pix, msk, A, v.patch_size, cfg.prompt_numbers)
            ops.gemm(A, self.w_patch, x2, hip.EPI_PATCH_POS, pos=self.pos, tokens_in=n, tokens_out=N, token_offset=self.npt)
        if mask_embeds is not None:         # x = x + mask_embeds.flatten(2).transpose(1, 2) on the patch rows
            assert msk is None, "mask_embeds and global_mask_values are alternatives"
            me = mask_embeds.to(self.device, self.dtype)
            if tuple(me.shape) != (Tt, D, v.grid, v.grid):
                raise ValueError(f"mask_embeds {tuple(me.shape)} should be {(Tt, D, v.grid, v.grid)}")
            ops.tokens_add(x, me.flatten(2).transpose(1, 2).contiguous(), self.npt)
        if self.npt:
            ops.cls_pos_fill(x, self.cls, self.pos)
        ops.layernorm(x2, *self.norm_pre, v.ln_eps)
        q_scale = (v.head_dim ** -0.5) * LOG2E
        f1v = f1.view(-1)[:Tt * N * Dm].view(Tt * N, Dm)
        # Folded LayerNorms (bf16, passes large enough for the tile GEMM): qkv and fc1 read the residual stream x itself with
        # the folded weights and scale their accumulator rows by rstd; proj and fc2 write x's row statistics from their
        # epilogues; a one-thread-per-row kernel turns them into rstd. No LayerNorm pass, no normalised copy of x.
        M = Tt * N
        has_folded = "qkv_wf" in self.vblocks[0]
        use_folded_w = has_folded and (self.FOLD_NORMS or "qkv_w" not in self.vblocks[0])      # bf16 keeps only these by default
        fold = (self.FOLD_NORMS and fused and Vr is not None and has_folded and D % 64 == 0 and
                ops.tile_gemm_takes(M, 3 * Da, D, epilogue=hip.EPI_QKV_ROPE, row_scale=True) and
                ops.tile_gemm_takes(M, D, Da, epilogue=hip.EPI_BIAS_SCALE_RES, row_stats=True) and
                ops.tile_gemm_takes(M, Dm, D, epilogue=hip.EPI_BIAS_GELU, row_scale=True) and
                ops.tile_gemm_takes(M, D, Dm, epilogue=hip.EPI_BIAS_SCALE_RES, row_stats=True))
        # the cls key (row 0) enters through the softmax's initial state: 1 + 1024 keys are 16 kv tiles, not 17 (built for ONE
        # prefix row: a tower with cls + register tokens keeps them as ordinary keys)
        kv_prefix = 1 if (self.VIT_CLS_KEY_FOLD and self.npt == 1 and N > 1) else 0
        if fold:
            rstd = self._buf(key, "rstd", (M,), torch.float32)
            stats = self._buf(key, "stats", (M, D // 64, 2), torch.float32)
            ops.row_rstd(x2, v.ln_eps, False, rstd)                  # LN1 of block 0: its input came out of norm_pre
            for bi, blk in enumerate(self.vblocks):
                if not ops.gemm_qkv_rope(x2, blk["qkv_wf"], blk["qkv_bf"], att, Q, K, self.vit_sin, self.vit_cos, H, hd, N,
                                         Npad, self.npt, q_scale, V=Vr, row_scale=rstd):
                    raise hip.GarError("folded qkv GEMM refused a shape gar_gemm_tile_takes() accepted")
                ops.attention(Q, K, Vr, att, Tt, H, H, hd, N, Npad, N, Npad, causal=False, v_row_major=True, kv_prefix=kv_prefix)
                ops.gemm(att, blk["proj_w"], x2, hip.EPI_BIAS_SCALE_RES, bias=blk["proj_b"], residual=x2, gamma=blk["g1"],
                         row_stats=stats)
                ops.row_stats_finalize(stats, D, v.ln_eps, False, rstd)
                ops.gemm(x2, blk["fc1_wf"], f1v, hip.EPI_BIAS_GELU, bias=blk["fc1_bf"], row_scale=rstd)
                last = bi + 1 == len(self.vblocks)
                ops.gemm(f1v, blk["fc2_w"], x2, hip.EPI_BIAS_SCALE_RES, bias=blk["fc2_b"], residual=x2, gamma=blk["g2"],
                         row_stats=None if last else stats)
                if not last:
                    ops.row_stats_finalize(stats, D, v.ln_eps, False, rstd)
        hbuf = None if fold else self._buf(key, "h", (M, D))

        def ln_operand(blk, which):
            """stand-alone LayerNorm of the residual stream into hbuf + the (weight, bias) that goes with it: the plain pair
            behind the block's own gamma / beta, or — bf16 keeps only those — the FOLDED pair behind a unit LayerNorm
            ((x - mean) rstd: gamma, beta and the row centring live in the weight, LN(x) W^T + b = ((x - mean) rstd) Wc^T + b')."""
            if use_folded_w:
                ops.layernorm(x2, self.unit_ln[0], self.unit_ln[1], v.ln_eps, out=hbuf)
                return (blk["qkv_wf"], blk["qkv_bf"]) if which == 1 else (blk["fc1_wf"], blk["fc1_bf"])
            n = blk["n1" if which == 1 else "n2"]
            ops.layernorm(x2, n[0], n[1], v.ln_eps, out=hbuf)
            return (blk["qkv_w"], blk["qkv_b"]) if which == 1 else (blk["fc1_w"], blk["fc1_b"])

        for blk in ([] if fold else self.vblocks):
            qw, qb = ln_operand(blk, 1)
            if fused:
                if Vr is None and vrow is None:
                    qkv = self._buf(key, "qkv", (M, 3 * Da))
                    vrow = qkv.view(-1)[:M * Da].view(M, Da)
                    Vt = self._buf(key, "Vt", (Tt, H, hd, Npad))
                # with V= the row-major v output is not written (att stands in for the pointer the ABI wants)
                fused = ops.gemm_qkv_rope(hbuf, qw, qb, att if Vr is not None else vrow, Q, K,
                                          self.vit_sin, self.vit_cos, H, hd, N, Npad, self.npt, q_scale, V=Vr)
            if fused and Vr is None:
                ops.vit_v_transpose(vrow, Vt, Tt, N, H, hd, Npad)
            elif not fused:
                Vr = None
                if qkv is None:
                    qkv = self._buf(key, "qkv", (M, 3 * Da))
                if Vt is None:
                    Vt = self._buf(key, "Vt", (Tt, H, hd, Npad))
                ops.gemm(hbuf, qw, qkv, hip.EPI_BIAS, bias=qb)
                ops.vit_qkv_post(qkv, self.vit_sin, self.vit_cos, Q, K, Vt, Tt, N, self.npt, H, hd, Npad, q_scale)
            if Vr is not None:      # v left the qkv GEMM head-major like k: the attention transposes it on its LDS reads
                ops.attention(Q, K, Vr, att, Tt, H, H, hd, N, Npad, N, Npad, causal=False, v_row_major=True, kv_prefix=kv_prefix)
            else:
                ops.attention(Q, K, Vt, att, Tt, H, H, hd, N, Npad, N, Npad, causal=False)
            ops.gemm(att, blk["proj_w"], x2, hip.EPI_BIAS_SCALE_RES, bias=blk["proj_b"], residual=x2, gamma=blk["g1"])
            fw, fb = ln_operand(blk, 2)
            ops.gemm(hbuf, fw, f1v, hip.EPI_BIAS_GELU, bias=fb)
            ops.gemm(f1v, blk["fc2_w"], x2, hip.EPI_BIAS_SCALE_RES, bias=blk["fc2_b"], residual=x2, gamma=blk["g2"])
        # projector over all N tokens of a tile (cls row included, dropped by the pooling window)
        p1 = f1.view(-1)[:Tt * N * C_l].view(Tt * N, C_l)
        ops.gemm(x2, self.pj["w1"], p1, hip.EPI_BIAS_GELU, bias=self.pj["b1"])
        p2 = self._buf(key, "p2", (Tt * N, C_l)) if out is None or pooled else out
        assert tuple(p2.shape) == (Tt * N, C_l) and p2.is_contiguous()
        ops.gemm(p1, self.pj["w2"], p2, hip.EPI_BIAS, bias=self.pj["b2"])
        if cfg.mllm_config.projector_pooling_ratio != 2:
            raise hip.GarError("projector_pooling_ratio != 2 is not built")
        if not pooled:
            return p2                       # generate(): pooled on the way into the sequence (gar_pool_assemble)
        P = cfg.pooled_side
        feats = self._buf(key, "feats", (Tt, P * P, C_l))
        ops.pool2x2(p2, feats, v.grid, in_tile_tokens=N, in_token_offset=self.npt)
        return feats

    @_on_model_device
    def _mask_embed(self, binary_mask: torch.Tensor) -> torch.Tensor:
        """mask_patch_embedding(binary) (modeling_gar.py:326-328): [T,3,H,W] in {0,1} -> [T, C_v, g, g] (view of [T, g*g, C_v])."""
        v = self.config.mllm_config.vision_config
        D, n, g = v.embed_dim, v.num_patches, v.grid
        mb = binary_mask.to(self.device, self.dtype)
        if mb.dim() == 5:
            mb = mb.flatten(0, 1)
        mb = mb.contiguous()
        T = mb.shape[0]
        out = torch.empty(T, n, D, dtype=self.dtype, device=self.device)
        done = False
        if self.w_patch_gather is not None:
            if "gather" not in self._mask_only_w:       # the gather-ordered operand with the pixel tensor's slots zeroed + a zero pos table
                wg = self.w_patch_gather.clone().view(D, 2, -1)
                wg[:, 0] = 0
                self._mask_only_w["gather"] = (wg.view(D, -1), torch.zeros(n, D, dtype=self.dtype, device=self.device))
            wg, zpos = self._mask_only_w["gather"]
            done = ops.patch_embed(mb, mb, wg, zpos, out, v.patch_size, 0)       # pixel slots carry zero weights: any finite tensor does
        if not done:
            pp = v.patch_size * v.patch_size
            if "im2col" not in self._mask_only_w:       # the mask conv's weight in the pixel columns of the im2col operand
                w = torch.zeros_like(self.w_patch)
                w[:, :3 * pp] = self.w_patch[:, 3 * pp:6 * pp]
                self._mask_only_w["im2col"] = w
            A = torch.empty(T * n, self.Kp, dtype=self.dtype, device=self.device)
            ops.patch_im2col(mb, None, A, v.patch_size, self.config.prompt_numbers)
            ops.gemm(A, self._mask_only_w["im2col"], out.view(T * n, D))
        return out.view(T, g, g, D).permute(0, 3, 1, 2)

    # ---- inputs_embeds: embedding + placeholder scatter + RoI replay (A7-A11) -----------------------------------------
    @_on_model_device
    def build_inputs_embeds(self, input_ids, feats, bboxes, aspect_ratios, tiles_per_sample: int, validate=True,
                            video_frame_tokens: Optional[Sequence[int]] = None, proj: Optional[torch.Tensor] = None):
        """``feats`` [B*tiles, P*P, C] pooled features (embed_assemble + replay from the feature tensor), or — what
        ``generate`` uses — ``proj``: the un-pooled projector output of ``get_image_features(pooled=False)``; then the
        2x2 pool runs on the way into the sequence and the replay reads the pooled rows back from it (one read of the
        projector output + one write of the sequence per region: SURVEY.md section 8d's algorithmic bytes)."""
        cfg = self.config
        B, S = input_ids.shape
        C_l = cfg.mllm_config.text_config.hidden_size
        P = cfg.pooled_side
        key = ("emb", B, S)
        ids = input_ids.to(self.device, torch.int64).contiguous()
        if video_frame_tokens is not None:
            # A13 video replay (modeling_perception_lm.py:765-852): one pooled map per frame, crop token per frame
            crop_ids = [int(t) for t in video_frame_tokens]
            if len(crop_ids) != tiles_per_sample or len(crop_ids) > 8:
                raise hip.GarError(f"video replay: {len(crop_ids)} frame tokens for {tiles_per_sample} frames (max 8)")
            vkey = tuple(crop_ids)
            if vkey not in self._video_crop_ids:
                self._video_crop_ids[vkey] = torch.tensor(crop_ids, dtype=torch.int64, device=self.device)
            crop_ids_dev = self._video_crop_ids[vkey]
        else:
            crop_ids, crop_ids_dev = self.crop_tokens_ids, self.crop_ids_dev
        slot = self._buf(key, "slot", (B, S), torch.int32)
        counts = self._buf(key, "counts", (B,), torch.int32)
        spans = self._buf(key, "spans", (B, len(crop_ids), 2), torch.int32)
        embeds = self._buf(key, "embeds", (B, S, C_l))
        n_rows = tiles_per_sample * P * P
        rank_pos = None
        if proj is not None:
            rank_pos = self._buf(key, "rank_pos", (B, n_rows), torch.int32)
            rank_pos.zero_()                # ranks without a placeholder (count mismatch) must still index inside the row
        ops.placeholder_scan(ids, cfg.mllm_config.image_token_id, crop_ids_dev, slot, counts, spans, rank_pos)
        if proj is not None:
            v = cfg.mllm_config.vision_config
            ops.pool_assemble(ids, slot, self.E, proj, embeds, tiles_per_sample, v.grid, v.num_patches + self.npt, self.npt)
        else:
            ops.embed_assemble(ids, slot, self.E, feats, embeds, n_rows)
        if not validate:
            # the same conditions, evaluated on the device by ONE small kernel and OR-ed into a flag nobody has to wait for
            # (ADVICE r1 #5 / r2): what the kernels do with such inputs (clamped slots / ids, P*P rows written from the span
            # head) is defined but not what the reference computes. The per-sample "has a bbox for crop token c" bits are the
            # only host data (B int32, one small pinned upload).
            hb = self._upload([sum(1 << ci for ci, t in enumerate(crop_ids) if str(t) in bboxes[b]) for b in range(B)], torch.int32)
            if getattr(self, "_input_flags", None) is None:
                self._input_flags = torch.zeros(1, dtype=torch.int32, device=self.device)
            ops.input_check(ids, self.E.shape[0], counts, n_rows, spans, P * P, hb, self._input_flags)
        if validate:
            # reference errors (modeling_perception_lm.py:309-315, modeling_gar.py:356-360) need the counts on the host
            cnt = counts.tolist()
            sp = spans.tolist()
            for b in range(B):
                if cnt[b] != n_rows:
                    raise ValueError(f"Image features and image tokens do not match: tokens: {cnt[b]}, features {n_rows}")
        video = video_frame_tokens is not None
        if not video:
            ar = aspect_ratios.tolist() if torch.is_tensor(aspect_ratios) else aspect_ratios
        jobs = []
        for b in range(B):
            if video:
                ncw = nch = 1                       # each frame is its own P x P map (feat_h = feat_w = P, :787)
            else:
                ncw, nch = int(ar[b][0]), int(ar[b][1])
                assert ncw * nch == tiles_per_sample - 1, f"{ncw * nch} != {tiles_per_sample - 1}"
            feat_h, feat_w = P * nch, P * ncw
            for ci, crop_token in enumerate(crop_ids):
                if str(crop_token) not in bboxes[b]:
                    if validate and sp[b][ci][1] >= 0:
                        raise KeyError(str(crop_token))
                    continue
                if validate:
                    if sp[b][ci][1] < 0:
                        continue            # token not in input_ids: the reference skips it (:356)
                    if sp[b][ci][1] - sp[b][ci][0] + 1 != P * P:
                        raise ValueError(f"crop token {crop_token} spans {sp[b][ci]} but the replay is {P * P} rows")
                # box math of modeling_gar.py:366-387 in Python floats, then fp32 like torch.tensor(..., float32)
                x1, y1, x2, y2 = [float(z) for z in bboxes[b][str(crop_token)]]
                orig_h, orig_w = feat_h * cfg.feat_stride, feat_w * cfg.feat_stride
                ss = feat_w / orig_w
                roi = (x1 * orig_w * ss, y1 * orig_h * ss, x2 * orig_w * ss, y2 * orig_h * ss)
                # image: map = tiles 1.. (thumbnail dropped, modeling_gar.py:351); video: map = frame ci only
                jobs.append((b, ci, ci if video else 1, ncw, nch, *roi, ss))
        if jobs:         # every crop token of every sample in one launch (the roi table is the only H2D copy)
            jt = ops.roi_jobs_tensor(jobs, self.device)
            if proj is not None:
                ops.roi_replay_inplace(embeds, spans, rank_pos, jt, len(crop_ids), P, C_l, S, 2, True)
            else:
                ops.roi_replay_batched(feats, embeds, spans, jt, len(crop_ids), tiles_per_sample, P, C_l, S, 2, True)
        return embeds

    # ---- Llama (A12) --------------------------------------------------------------------------------------------------
    def _llm_state(self, B: int, Smax: int, slot: int = 0, fan=None):
        """KV cache + counters of one (B, Smax) bucket. ``slot``: independent copies of the same bucket — the pipelined driver
        (generate_pipelined) decodes batch i from one slot while batch i + 1 prefills into the other. ``fan`` = (prompts, Sp): the
        B rows are the continuations of a num_return_sequences request, Kc / Vc hold their generated tokens only (Smax = T rows),
        counters = [t, -, step, P]; the prompts' rows stay in the (prompts, Sp) state (:meth:`_generate_begin_fanout`)."""
        t = self.config.mllm_config.text_config
        key = ("llm", B, Smax, slot) if fan is None else ("llm", B, Smax, slot, fan)
        if key in self._llm_lru:
            self._llm_lru.remove(key)
        self._llm_lru.append(key)
        while sum(1 for k in self._llm_lru if k[3] == slot) > self.MAX_LLM_STATES:        # MAX_LLM_STATES buckets per slot
            old = next(k for k in self._llm_lru if k[3] == slot)
            self._llm_lru.remove(old)
            self._ws.pop(old, None)
            for gk in [g for g in self._graphs if g[0] == old]:
                del self._graphs[gk]
            # the per-batch decode / head workspaces (logits [B, vocab], attention partials, split-K slices) go with the
            # last live state of that batch size: a service that sees many distinct B does not accumulate them
            if not any(k[1] == old[1] for k in self._llm_lru):
                for wk in [w for w in self._ws if w[0] in ("decode", "head") and w[1] == old[1]]:
                    self._ws.pop(wk, None)
        L, Hkv, hd = t.num_hidden_layers, t.num_key_value_heads, t.head_dim
        kv_dt = torch.uint8 if self.kv_fp8 else None
        st = dict(
            Kc=self._buf(key, "Kc", (L, B, Hkv, Smax, hd), kv_dt, zero=True),
            Vc=self._buf(key, "Vc", (L, B, Hkv, Smax, hd), kv_dt, zero=True),      # row-major like K: an append is one row
            counters=self._buf(key, "counters", (4,), torch.int32, zero=True),   # [pos, kv_len, step, -]
            cur=self._buf(key, "cur", (B,), torch.int64, zero=True),
            # first real row of every sequence (left-padded batch; zeros otherwise): read by the qkv-post and attention
            # kernels of the prefill and of the captured decode step, so one graph serves padded and unpadded requests
            left_pad=self._buf(key, "left_pad", (B,), torch.int32, zero=True),
            # the greedy loop's stopping criterion, evaluated by the argmax kernel (gar_argmax): the eos ids of the request
            # (-1 = unused entry), the step at which a row first produced one (-1 = running), the number of finished rows
            eos_ids=self._buf(key, "eos_ids", (self.MAX_EOS_IDS,), torch.int64),
            finished=self._buf(key, "finished", (B,), torch.int32),
            done_count=self._buf(key, "done_count", (1,), torch.int32, zero=True),
            # do_sample = True: the request's sampling block and Philox key, read by the captured step — [temperature, top_p, top_k, 0]
            # (gar_sample reads the first three), then sampling_warpers' [min_p, typical_p, epsilon_cutoff, eta_cutoff] (gar_sample_ext)
            sample_params=self._buf(key, "sample_params", (ops.SAMPLE_EXT_PARAMS,), torch.float32, zero=True),
            sample_seed=self._buf(key, "sample_seed", (1,), torch.int64, zero=True),
            sampling=False,
            slot=slot,
        )
        if self.kv_fp8:     # e4m3 bytes in Kc / Vc, their scales here
            st["Ks"] = self._buf(key, "Ks", (L, B, Hkv, Smax), torch.float32, zero=True)
            st["Vs"] = self._buf(key, "Vs", (L, B, Hkv, Smax), torch.float32, zero=True)
        return key, st

    def _prefill(self, embeds: torch.Tensor, st, Smax: int, b0: int = 0, prune: Optional[bool] = None):
        """Prefill of one chunk of sequences [B,S,C] whose KV goes to rows b0..b0+B of the shared cache. Returns the last
        prompt row of every sequence after the last layer ([B, C] row-strided view): what the head reads. ``prune``: None =
        PRUNE_LAST_PREFILL_LAYER; False runs the last layer at full width, so every row of ``embeds`` holds the residual
        stream after the last layer (what :meth:`score` reads)."""
        t = self.config.mllm_config.text_config
        B, S, C_l = embeds.shape
        Hq, Hkv, hd, F = t.num_attention_heads, t.num_key_value_heads, t.head_dim, t.intermediate_size
        key = ("prefill", B, S)
        h = embeds.view(B * S, C_l)
        M = B * S
        qd = (Hq + 2 * Hkv) * hd
        Spad = _round_up(S, 64)
        Q = self._buf(key, "Q", (B, Hq, Spad, hd))
        cos, sin = self._llm_rope(Smax)
        q_scale = (hd ** -0.5) * LOG2E
        lp = st["left_pad"][b0:b0 + B]
        bf16 = self.dtype in HALF_DTYPES
        has_folded = "qkv_f" in self.layers[0]
        use_folded_w = has_folded and (self.FOLD_NORMS or "qkv" not in self.layers[0])         # bf16 keeps only these by default
        # Folded RMSNorms (bf16, tile-GEMM sized passes): qkv and gate/up read the residual stream h with W diag(g) and scale
        # their accumulator rows by rstd; o and down write h's row sums of squares from their epilogues (see get_image_features)
        fold = (self.FOLD_NORMS and bf16 and has_folded and C_l % 64 == 0 and
                ops.tile_gemm_takes(M, qd, C_l, row_scale=True) and
                ops.tile_gemm_takes(M, C_l, Hq * hd, epilogue=hip.EPI_RES, row_stats=True) and
                ops.tile_gemm_takes(M, 2 * F, C_l, epilogue=hip.EPI_SWIGLU, row_scale=True) and
                ops.tile_gemm_takes(M, C_l, F, epilogue=hip.EPI_RES, row_stats=True))
        rstd = stats = xn = None
        if fold:
            rstd = self._buf(key, "rstd", (M,), torch.float32)
            stats = self._buf(key, "stats", (M, C_l // 64, 2), torch.float32)
            ops.row_rstd(h, t.rms_norm_eps, True, rstd)                  # input_layernorm of layer 0: h came from the embedding pass
        else:
            xn = self._buf(key, "xn", (M, C_l))                          # the normalised copy of h: only without folded norms
        fused_qkv = fold and self.LLM_QKV_EPILOGUE and hd in (64, 128)
        strip = use_folded_w and self.qkv_f_permuted        # q / k head columns of a qkv_f product are in the fused epilogue's order
        L = len(self.layers)
        prune = (self.PRUNE_LAST_PREFILL_LAYER if prune is None else prune) and S > 1
        att = ff = None
        if L > 1 or not prune:
            att = self._buf(key, "att", (M, Hq * hd))
            ff = self._buf(key, "ff", (M, F))
        # fp8 cache: the prompt kernels write a 16-bit K / V scratch of the layer (kv stride Spad) and read it for the prompt's
        # own attention; one quantize launch per layer then fills the fp8 cache the decode steps read
        kv_stride = Spad if self.kv_fp8 else Smax
        for li, ly in enumerate(self.layers):
            last = li + 1 == L
            if self.kv_fp8:
                Kc, Vc = self._buf(key, "K16", (B, Hkv, Spad, hd)), self._buf(key, "V16", (B, Hkv, Spad, hd))
            else:
                Kc, Vc = st["Kc"][li][b0:b0 + B], st["Vc"][li][b0:b0 + B]         # this chunk's rows of the shared cache
            # ---- q / k / v of EVERY row (the decode steps read this layer's K / V rows too)
            if fused_qkv:
                if not ops.gemm_qkv_rope_llm(h, ly["qkv_f"], Q, Kc, Vc, cos, sin, B, S, Spad, Hq, Hkv, hd, kv_stride, 0, None,
                                             q_scale, left_pad=lp, row_scale=rstd):
                    raise hip.GarError("fused qkv GEMM refused a shape gar_gemm_tile_takes() accepted")
            else:
                qb = self._qkv_buf(key, B, S, Hq, Hkv, hd)
                if fold:
                    ops.gemm(h, ly["qkv_f"], qb, row_scale=rstd)
                elif use_folded_w:      # unit-gain RMSNorm pass + the folded weight (its gain is in W)
                    ops.rmsnorm(h, self.unit_rms, t.rms_norm_eps, out=xn)
                    ops.gemm(xn, ly["qkv_f"], qb)
                else:
                    ops.rmsnorm(h, ly["ln1"], t.rms_norm_eps, out=xn)
                    ops.gemm(xn, ly["qkv"], qb)
                ops.llm_qkv_post(qb, cos, sin, Q, Kc, Vc, B, S, Spad, Hq, Hkv, hd, kv_stride, 0, None, q_scale, left_pad=lp,
                                 strip_order=strip)
            if self.kv_fp8:
                ops.kv_quantize_fp8(Kc, Vc, st["Kc"][li][b0:b0 + B], st["Vc"][li][b0:b0 + B], st["Ks"][li][b0:b0 + B],
                                    st["Vs"][li][b0:b0 + B], B, Hkv, hd, Smax, S)
            if last and prune:
                return self._prefill_tail(ly, h, Q, Kc, Vc, st, key, B, S, Spad, kv_stride, lp)
            ops.attention(Q, Kc, Vc, att, B, Hq, Hkv, hd, S, Spad, S, kv_stride, causal=True, kv_start=lp, v_row_major=True)
            if fold:
                ops.gemm(att, ly["o"], h, hip.EPI_RES, residual=h, row_stats=stats)
                ops.row_stats_finalize(stats, C_l, t.rms_norm_eps, True, rstd)
                ops.gemm(h, ly["gu_f"], ff, hip.EPI_SWIGLU, row_scale=rstd)
                ops.gemm(ff, ly["down"], h, hip.EPI_RES, residual=h, row_stats=None if last else stats)
                if not last:
                    ops.row_stats_finalize(stats, C_l, t.rms_norm_eps, True, rstd)
            else:
                ops.gemm(att, ly["o"], h, hip.EPI_RES, residual=h)
                if use_folded_w:
                    ops.rmsnorm(h, self.unit_rms, t.rms_norm_eps, out=xn)
                    ops.gemm(xn, ly["gu_f"], ff, hip.EPI_SWIGLU)
                else:
                    ops.rmsnorm(h, ly["ln2"], t.rms_norm_eps, out=xn)
                    ops.gemm(xn, ly["gu"], ff, hip.EPI_SWIGLU)
                ops.gemm(ff, ly["down"], h, hip.EPI_RES, residual=h)
        return h.view(B, S, C_l)[:, S - 1, :]                                   # row-strided view [B, C]

    def _prefill_tail(self, ly, h, Q, Kc, Vc, st, key, B, S, Spad, kv_stride, lp):
        """The last layer of a prefill behind its qkv GEMM, for the LAST prompt row of each of the B sequences only
        (PRUNE_LAST_PREFILL_LAYER): single-row attention over the sequence's S cache rows with the split-KV decode kernel —
        the query is read in place from row S - 1 of Q [B, Hq, Spad, hd] — then o / RMSNorm / gate-up / down as B-row GEMMs on
        the rows h[b, S - 1] (row-strided views, updated in place like the full-width layers update h)."""
        t = self.config.mllm_config.text_config
        C_l = h.shape[1]
        Hq, Hkv, hd, F = t.num_attention_heads, t.num_key_value_heads, t.head_dim, t.intermediate_size
        hl = h.view(B, S, C_l)[:, S - 1, :]
        attl = self._buf(key, "att_last", (B, Hq * hd))
        ffl = self._buf(key, "ff_last", (B, F))
        kv_len = st["counters"][3:4]                    # scratch word of the counters: the prompt length, for the kernel's kv_len_dev
        kv_len.fill_(S)
        nsplit = max(1, min(self.DECODE_ATTN_MAX_SPLITS, self.DECODE_ATTN_BLOCKS // max(1, B * Hkv)))
        dws = self._buf(key, "attn_ws_last", (ops.attention_decode_workspace(B, Hq, hd, nsplit),), torch.uint8)
        ops.attention_decode(Q[:, :, S - 1], Kc, Vc, attl, B, Hq, Hkv, hd, kv_stride, kv_len, nsplit, dws, kv_start=lp,
                             q_stride=Spad * hd)
        ops.gemm(attl, ly["o"], hl, hip.EPI_RES, residual=hl)
        if "gu_f" in ly and (self.FOLD_NORMS or "gu" not in ly):
            if B <= 64:     # RMSNorm inside the GEMM: gain in the weight, row sums of squares off the matrix pipe
                ops.gemm(hl, ly["gu_f"], ffl, hip.EPI_SWIGLU, norm_folded=True, norm_eps=t.rms_norm_eps)
            else:
                xnl = self._buf(key, "xn_last", (B, C_l))
                ops.rmsnorm(hl, self.unit_rms, t.rms_norm_eps, out=xnl)
                ops.gemm(xnl, ly["gu_f"], ffl, hip.EPI_SWIGLU)
        else:
            xnl = self._buf(key, "xn_last", (B, C_l))
            ops.rmsnorm(hl, ly["ln2"], t.rms_norm_eps, out=xnl)
            ops.gemm(xnl, ly["gu"], ffl, hip.EPI_SWIGLU)
        ops.gemm(ffl, ly["down"], hl, hip.EPI_RES, residual=hl)
        return hl

    def _qkv_buf(self, key, B, S, Hq, Hkv, hd):
        """the [B*S, (Hq + 2 Hkv) hd] qkv GEMM output of the unfused prefill path (f32 / FOLD_NORMS off): lazily allocated"""
        return self._buf(key, "qkv", (B * S, (Hq + 2 * Hkv) * hd))

    def _upload(self, values, dtype, cache: bool = True) -> torch.Tensor:
        """small host constants of a request (eos ids, has-bbox bits, sampling parameters) as a device tensor. The values repeat from
        call to call (one eos set, one crop-token pattern per evaluation loop): their device copies are cached by value — no pinned
        host allocation and no upload per generate() (visible at batch 1). A cache miss is one pageable H2D copy."""
        key = (dtype, tuple(values))
        memo = self.__dict__.setdefault("_upload_cache", {})
        t = memo.get(key) if cache else None
        if t is None:
            t = torch.tensor(list(values), dtype=dtype).to(self.device)
            if cache:
                if len(memo) > 256:
                    memo.clear()
                memo[key] = t
        return t

    def _head(self, last_rows: torch.Tensor, B: int, st, to: Optional["_PickTargets"], normed: Optional[torch.Tensor] = None,
              decode: bool = False):
        """final RMSNorm + lm_head of the given [B, C] rows (row-strided view allowed), then :meth:`_pick` into ``to``; returns the
        logits. ``to`` None: the logits only — the caller draws the tokens (N draws per prompt row: _generate_begin_fanout).
        ``normed``: the rows after the final norm, when the caller's last launch produced them already (split-K decode path).
        ``decode``: a decode step's head (the e4m3 lm_head of a decode_weight_dtype="fp8" model), not the prompt's first token."""
        gemm = self._gemm_w8 if decode and self.w_fp8 else ops.gemm
        t = self.config.mllm_config.text_config
        C_l, V = t.hidden_size, t.vocab_size
        key = ("head", B, st.get("slot", 0))       # per slot: a pipelined prefill's first-token head runs beside the other slot's decode
        xn = self._buf(key, "xn", (B, C_l))
        Vld = _round_up(V, 64)
        logits = self._buf(key, "logits", (B, Vld))
        if normed is not None:
            gemm(normed, self.lm_head, logits)
        elif B <= 16:       # RMSNorm folded into the GEMV prologue; for more rows one tiny norm launch is cheaper
            gemm(last_rows, self.lm_head, logits, norm_w=self.final_norm, norm_eps=t.rms_norm_eps)
        else:
            ops.rmsnorm(last_rows, self.final_norm, t.rms_norm_eps, out=xn)
            gemm(xn, self.lm_head, logits)
        if to is not None:
            self._pick(logits, V, st, to)
        return logits

    def _process(self, logits, V, st, out_tokens, row_proc=None):
        """the request's logits processors on ``logits`` in place (one gar_logits_process launch), the rows' histories read from
        ``out_tokens`` up to the state's step; nothing — no launch — for a request without a non-neutral ``logits_processing``.
        ``row_proc`` (ContinuousBatcher(processing=True)): the rows' own blocks instead, one gar_logits_process_rows launch — a row's
        history starts at its block's ``col0``, a row with a zero header is left alone."""
        if st.get("proc") is None and row_proc is None:
            return
        if st.get("proc") is not None and row_proc is not None:
            raise hip.GarError("per-row processing blocks and a logits_processing of the call's own do not combine")
        if out_tokens is not None:
            # out_tokens is a [:, :max_new_tokens] slice of the state's token buffer; the captured step serves every
            # max_new_tokens of the bucket, so the history's bound is the buffer's row (its stride), not the slice's width
            cap = out_tokens.stride(0)
            out_tokens = out_tokens.as_strided((out_tokens.shape[0], cap), (cap, 1), out_tokens.storage_offset())
        if row_proc is not None:
            ops.logits_process_rows(logits, V, out_tokens, st["counters"][2:3], st["eos_ids"], row_proc)
        else:
            ops.logits_process(logits, V, out_tokens, st["counters"][2:3], st["eos_ids"], st["proc"])

    def _arm_processing(self, skey, st, proc: Optional[LogitsProcessing], eos_list, eos_on_device: bool):
        """st["proc"] of a request: None without (non-neutral) logits_processing, else the state's int32 parameter block with the
        request's values uploaded — a buffer of the state, so the captured step that reads it serves any values"""
        st["proc"] = None
        if proc is None:
            return
        V = self.config.mllm_config.text_config.vocab_size
        if V > ops.logits_process_max_vocab():
            raise hip.GarError(f"logits_processing: vocab_size {V} above gar_logits_process's {ops.logits_process_max_vocab()}")
        if proc.min_new_tokens and eos_list and not eos_on_device:
            raise hip.GarError(f"logits_processing: min_new_tokens with {len(eos_list)} eos ids: the device-side eos table holds "
                               f"{self.MAX_EOS_IDS}")
        try:
            words = proc.pack(V, eos_list)
        except _ProcessingRefused as e:
            raise hip.GarError(str(e)) from None
        buf = self._buf(skey, "proc", (ops.LOGITS_PROCESS_WORDS,), torch.int32, zero=True)
        buf[:len(words)].copy_(self._upload(words, torch.int32))
        st["proc"] = buf

    def _arm_constraint(self, skey, st, constraint: Optional[PhraseConstraint], B: int, N: int, cols: int):
        """st["trie"] / st["nodes"] of a request: None without a constraint, else the state's trie block with the request's phrases
        uploaded and the node plane [B * N, cols + 1] with column 0 = every row's root — buffers of the state, so the captured step
        that reads them serves any phrase set"""
        st["trie"] = st["nodes"] = None
        if constraint is None:
            return
        V = self.config.mllm_config.text_config.vocab_size
        if V > ops.logits_process_max_vocab():
            raise hip.GarError(f"constraint: vocab_size {V} above gar_constrain's {ops.logits_process_max_vocab()}")
        try:
            words = constraint.pack(V, B, N)
        except _ProcessingRefused as e:
            raise hip.GarError(str(e)) from None
        trie = self._buf(skey, "trie", (ops.CONSTRAINT_WORDS,), torch.int32, zero=True)
        host = torch.tensor(words, dtype=torch.int32)
        trie[:len(words)].copy_(host)
        nodes = self._buf(skey, "nodes", (B * N, cols + 1), torch.int32, zero=True)
        nodes[:, 0].copy_(host[ops.CONSTRAINT_HEADER:ops.CONSTRAINT_HEADER + B * N])
        st["trie"], st["nodes"] = trie, nodes

    def _constrain(self, logits, V, st, out_tokens, nodes):
        """the request's phrase constraint on ``logits`` in place (one gar_constrain launch) over the rows ``nodes`` of the node
        plane; nothing — no launch — for a request without one. ``out_tokens`` None: step 0, no history."""
        if nodes is None:
            return
        step = None
        if out_tokens is not None:      # as _process: the history's bound is the token buffer's row, not the slice's width
            cap = out_tokens.stride(0)
            out_tokens = out_tokens.as_strided((out_tokens.shape[0], cap), (cap, 1), out_tokens.storage_offset())
            step = st["counters"][2:3]
        ops.constrain(logits, V, out_tokens, step, st["eos_ids"], st["trie"], nodes)

    def _pick(self, logits, V, st, to: "_PickTargets", process: bool = True):
        """the token of every row of ``logits`` into ``to``, by the request words of ``st``: the request's logits processors first
        (gar_logits_process, in place; ``process`` False: the caller ran them), then one gar_topk_lp when the request
        has top_logprobs / candidate_token_ids planes (it reads the logits only), then the draw (gar_sample) or the greedy pick
        (gar_argmax) — with log-probability planes the launch that also writes the chosen token's (gar_sample_lp / gar_argmax_lp); a
        sampled request with sampling_warpers draws with gar_sample_ext in gar_sample's place.
        A state whose rows carry requests of their own (``to.row_words``: ContinuousBatcher(sampling=True)) picks every row with
        gar_sample_rows instead; one whose rows carry processing blocks of their own (``to.row_proc``: ContinuousBatcher(
        processing=True)) runs gar_logits_process_rows in front of that pick, or of the greedy one."""
        B, tk, step = logits.shape[0], to.tk, st["counters"][2:3]
        key = ("head", B, st.get("slot", 0))
        if st.get("beam") is not None:      # beam_search: the rows' M best, the beams' bookkeeping, the caches behind their parents
            self._beam_pick(logits, V, st, key)
            return
        if to.row_proc is not None and (to.lp is not None or tk is not None):
            raise hip.GarError("per-row processing blocks carry no log-probability planes (they are defined over the unprocessed logits)")
        if process:
            self._process(logits, V, st, to.out_tokens, to.row_proc)
            self._constrain(logits, V, st, to.out_tokens, to.nodes)      # behind the processors: HF's order, and -inf stays -inf
        if tk is not None:
            ws = self._buf(key, f"tkws{tk['k']}", (ops.topk_lp_workspace(B, V, tk["k"]),), torch.uint8)   # by k: a captured step keeps its own
            ops.topk_lp(logits, V, step, ws, top_ids=tk["ids"], top_lp=tk["lp"], cand_ids=tk["cand_ids"], cand_lp=tk["cand_lp"])
        raw, warped = to.lp or (None, None)
        latches = dict(eos_ids=st["eos_ids"], finished=to.finished, done_count=st["done_count"], logprobs=raw, logprobs_warped=warped)
        if to.row_words is not None:
            if to.lp is not None or tk is not None or st.get("proc") is not None or st.get("sampling"):
                raise hip.GarError("per-row sampling requests carry no log-probability planes and no logits_processing of the "
                                   "call's own (a row's processing goes in its block: _row_proc)")
            ops.sample_rows(logits, V, to.out_tokens, to.out_tokens.stride(0), step, to.cur, to.row_words, eos_ids=st["eos_ids"],
                            finished=to.finished, done_count=st["done_count"])
        elif st.get("sampling") and st.get("warpers"):          # sampling_warpers: the same pick through gar_sample_ext
            ops.sample_ext(logits, V, to.out_tokens, to.out_tokens.stride(0), step, to.cur, st["sample_params"], st["sample_seed"],
                           row_offset=to.row0, **latches)
        elif st.get("sampling"):
            ops.sample(logits, V, to.out_tokens, to.out_tokens.stride(0), step, to.cur, st["sample_params"], st["sample_seed"],
                       row_offset=to.row0, **latches)
        else:                       # with planes one more f32 per partial block: a workspace of its own size
            name, size = ("amws", ops.argmax_workspace) if to.lp is None else ("amws_lp", ops.argmax_lp_workspace)
            ws = self._buf(key, name, (size(B, V),), torch.uint8)
            ops.argmax(logits, V, to.out_tokens, to.out_tokens.stride(0), step, to.cur, ws, **latches)

    def _beam_pick(self, logits, V, st, key):
        """a decode step's pick of a beam_search request: gar_topk_lp (k = M) into the beam state's planes, gar_beam_step, then
        gar_kv_beam_reorder over the cache rows the beams have written so far — counters[2] of them, from suffix row 0 of the
        shared layout or from the prompt length (counters[3]) of the f32 parity mode's ordinary cache"""
        bs, step = st["beam"], st["counters"][2:3]
        R, M = bs["B"] * bs["K"], bs["M"]
        ws = self._buf(key, f"tkws{M}", (ops.topk_lp_workspace(R, V, M),), torch.uint8)
        ops.topk_lp(logits, V, None, ws, top_ids=bs["top_ids"].view(R, 1, M), top_lp=bs["top_lp"].view(R, 1, M))
        ops.beam_step(bs, step, V)
        ops.kv_beam_reorder(st["Kc"], st["Vc"], bs["K"], step, bs["parent"], s0_dev=None if st.get("fan") else st["counters"][3:4])

    _BEAM_LATCHES = ("run_scores", "parent", "hist", "fin_tokens", "fin_scores", "fin_len", "fin_flag", "heur", "done")

    def _beam_state(self, skey, st, B: int, K: int, M: int, T: int, beam: BeamSearch, max_new_tokens: int, eos_list):
        """st["beam"] of a request: the buffers gar_beam_step reads and writes — buffers of the state named by (K, M, T), so their
        pointers are the captured step's — initialised as HF initialises them, with the request's parameter block and
        length-penalty table uploaded"""
        R = B * K

        def buf(name, shape, dt):
            return self._buf(skey, f"beam_{name}_{K}_{M}_{T}", shape, dt, zero=True)
        bs = dict(B=B, K=K, M=M, T=T, key=(K, M, T), cur_tokens=st["cur"], done_count=st["done_count"],
                  top_ids=buf("top_ids", (R, M), torch.int32), top_lp=buf("top_lp", (R, M), torch.float32),
                  run_scores=buf("run_scores", (R,), torch.float32), parent=buf("parent", (R,), torch.int32),
                  hist=buf("hist", (2, R, T), torch.int32), fin_tokens=buf("fin_tokens", (R, T), torch.int32),
                  fin_scores=buf("fin_scores", (R,), torch.float32), fin_len=buf("fin_len", (R,), torch.int32),
                  fin_flag=buf("fin_flag", (R,), torch.int32), heur=buf("heur", (B,), torch.int32),
                  done=buf("done", (B,), torch.int32), params=buf("params", (ops.BEAM_PARAM_WORDS,), torch.int32),
                  len_pow=buf("len_pow", (T,), torch.float32))
        for name in ("parent", "hist", "fin_tokens", "fin_len", "fin_flag", "done"):
            bs[name].zero_()
        bs["run_scores"].fill_(-1.0e9)              # HF: the first beam starts at 0, its siblings at -1e9, the finished set at -1e9
        bs["run_scores"].view(B, K)[:, 0].zero_()
        bs["fin_scores"].fill_(-1.0e9)
        bs["heur"].fill_(1)
        bs["params"].copy_(self._upload(beam.pack(max_new_tokens, eos_list), torch.int32))
        bs["len_pow"].copy_(self._upload(beam.length_powers(T), torch.float32))
        st["beam"] = bs
        return bs

    def _generate_begin_beam(self, beam, M, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, attention_mask,
                             max_new_tokens, eos_token_id, pad_token_id, use_graph, validate, return_logits, sync_every,
                             feature_replay_video, video_frame_tokens, state_slot):
        """generate_begin of a beam_search request, :meth:`_generate_begin_fanout` with N = K: ONE prompt phase over the B prompts
        and a state of B * K rows — row b * K + j is beam j of prompt b. The prompt's logits row is repeated K times and step 0 is
        an ordinary gar_beam_step: HF's initial scores {0, -1e9, ...} make every first candidate a child of beam 0.
        16-bit models: the beams share the prompt's cache rows and keep only their generated tokens' rows. f32 parity mode: the
        prompt's rows are copied into an ordinary (B * K, Smax) state."""
        t = self.config.mllm_config.text_config
        B, S = input_ids.shape
        K = beam.num_beams
        R, V = B * K, t.vocab_size
        left_pad, _ = self._begin_inputs(input_ids, attention_mask, validate, None)
        shared = self.dtype in HALF_DTYPES
        T = _round_up(max_new_tokens, 64)
        if shared:
            Sp = _round_up(S, 256)
            _, pst = self._llm_state(B, Sp, state_slot)
            skey, st = self._llm_state(R, T, state_slot, fan=(B, Sp))
            st["fan"] = dict(B=B, N=K, Sp=Sp, Kp=pst["Kc"], Vp=pst["Vc"], left_pad=pst["left_pad"])
            Smax = Sp + T
        else:
            Sp = Smax = _round_up(S + max_new_tokens, 256)
            _, pst = self._llm_state(B, Smax, state_slot)
            skey, st = self._llm_state(R, Smax, state_slot)
        out_tokens = self._buf(skey, "out_tokens", (R, T if shared else Smax), torch.int64, zero=True)[:, :max_new_tokens]
        st["lp"] = st["tk"] = st["proc"] = st["trie"] = st["nodes"] = None
        self._arm_state(pst, left_pad, None, None, None)
        eos_list, _ = self._arm_state(st, None, eos_token_id, None, None)
        bs = self._beam_state(skey, st, B, K, M, T, beam, max_new_tokens, eos_list)
        first_logits = []
        for b0, b1, embeds in self._prompt_chunks(pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, validate,
                                                  feature_replay_video, video_frame_tokens):
            last = self._prefill(embeds, pst, Sp, b0)
            lg = self._head(last, b1 - b0, pst, None).repeat_interleave(K, 0)       # the SAME logits for the K beams
            r0, r1 = _fanout_rows(b0, b1, K)
            ws = self._buf(("head", r1 - r0, state_slot), f"tkws{M}", (ops.topk_lp_workspace(r1 - r0, V, M),), torch.uint8)
            ops.topk_lp(lg, V, None, ws, top_ids=bs["top_ids"][r0:r1].view(r1 - r0, 1, M), top_lp=bs["top_lp"][r0:r1].view(r1 - r0, 1, M))
            if return_logits:
                first_logits.append(lg[:, :V].float())
        c = st["counters"]
        ops.beam_step(bs, c[2:3], V)            # step 0 of every prompt (counters are zero): nothing to reorder yet
        if shared:                      # [t, -, step, P]
            c[2:3].fill_(1)
            c[3:4].fill_(S)
        else:                           # the prompts' cache rows, K times; [pos, kv_len, step, prompt length]
            L, Hkv, hd = t.num_hidden_layers, t.num_key_value_heads, t.head_dim
            for name in ("Kc", "Vc"):
                st[name].view(L, B, K, Hkv, Smax, hd).copy_(pst[name][:, :, None])
            st["left_pad"].copy_(pst["left_pad"].repeat_interleave(K))
            c[0:1].fill_(S)
            c[1:2].fill_(S + 1)
            c[2:3].fill_(1)
            c[3:4].fill_(S)
        return self._begin_pending(first_logits, eos_list, eos_on_device=True, st=st, skey=skey, B=R, Smax=Smax,
                                   out_tokens=out_tokens, max_new_tokens=max_new_tokens, pad_token_id=pad_token_id,
                                   return_logits=return_logits, forced_tokens=None, use_graph=use_graph, validate=validate,
                                   sync_every=sync_every, N=K, beam=beam, prompts=B)

    def _topk_planes(self, skey, st, shape, k: int, cands):
        """st["tk"] of a request: None without top_logprobs / candidate_token_ids, else the planes gar_topk_lp writes — buffers of the
        state named by (k, C), [rows, T, k] / [rows, T, C] with T the state's token capacity, so their pointers are the captured
        step's as long as the state lives — and the candidate ids, uploaded once per request."""
        if not k and not cands:
            st["tk"] = None
            return None
        R, T = shape
        C_ = len(cands)
        tk = dict(k=k, C=C_, ids=None, lp=None, cand_ids=None, cand_lp=None)
        if k:
            tk["ids"] = self._buf(skey, f"top_ids{k}", (R, T, k), torch.int32, zero=True)
            tk["lp"] = self._buf(skey, f"top_lp{k}", (R, T, k), torch.float32, zero=True)
        if C_:
            tk["cand_ids"] = self._buf(skey, f"cand_ids{C_}", (C_,), torch.int32, zero=True)
            tk["cand_ids"].copy_(self._upload(cands, torch.int32))
            tk["cand_lp"] = self._buf(skey, f"cand_lp{C_}", (R, T, C_), torch.float32, zero=True)
        st["tk"] = tk
        return tk

    def _decode_step(self, st, B: int, Smax: int, out_tokens):
        t = self.config.mllm_config.text_config
        C_l = t.hidden_size
        Hq, Hkv, hd, F = t.num_attention_heads, t.num_key_value_heads, t.head_dim, t.intermediate_size
        key = ("decode", B)
        h = self._buf(key, "h", (B, C_l))
        xn = self._buf(key, "xn", (B, C_l))
        qkv = self._buf(key, "qkv", (B, (Hq + 2 * Hkv) * hd))
        Q = self._buf(key, "Q", (B, Hq, 1, hd))
        att = self._buf(key, "att", (B, Hq * hd))
        ff = self._buf(key, "ff", (B, F))
        cos, sin = self._llm_rope(Smax)
        q_scale = (hd ** -0.5) * LOG2E
        pos_dev, kvlen_dev = st["counters"][0:1], st["counters"][1:2]
        fan = st.get("fan")         # B = prompts x N rows over shared prompt caches: the prefix splits count over the prompts
        if fan:
            blocks = fan["B"] * Hkv * -(-fan["N"] // max(1, 32 // (Hq // Hkv)))
            nsplit = max(1, min(self.DECODE_ATTN_MAX_SPLITS, self.DECODE_ATTN_BLOCKS // blocks))
            dws = self._buf(key, "attn_ws_fan", (ops.attention_decode_fanout_workspace(B, Hq, hd, nsplit),), torch.uint8)
        else:
            nsplit = max(1, min(self.DECODE_ATTN_MAX_SPLITS, self.DECODE_ATTN_BLOCKS // max(1, B * Hkv)))
            dws = self._buf(key, "attn_ws", (ops.attention_decode_workspace(B, Hq, hd, nsplit),), torch.uint8)
        ops.embed_lookup(st["cur"], self.E, h)
        gemm = self._gemm_w8 if self.w_fp8 else ops.gemm       # the weight GEMVs: e4m3 copies (decode_weight_dtype="fp8") or 16-bit
        bf16 = self.dtype in HALF_DTYPES
        use_folded_w = self._decode_uses_folded_w()
        # how the two RMSNorms of a layer reach their GEMVs:
        #   folded  (bf16, B <= 64): gain in the weight (qkv_f / gu_f), row sums of squares off the matrix pipe inside the GEMV
        #           (gar_gemm_params.norm_folded) — no norm launch, no normalised copy, ONE copy of the weights
        #   fuse    (plain weights, B <= 16): x * g in the GEMV prologue (gar_gemm_params.norm_w)
        #   else    a norm launch in front of the GEMV (unit gain when only the folded weights exist)
        folded = use_folded_w and bf16 and B <= 64
        fuse = not use_folded_w and B <= self.FUSE_NORM_MAX_BATCH
        strip = use_folded_w and self.qkv_f_permuted
        # `down` (K = intermediate size, only hidden/16 weight tiles) streams from DOWN_SPLIT_K x the workgroups as K slices
        # whose fp32 products are reduced — with the residual add and, on the last layer, the final RMSNorm — by the launch that
        # follows anyway (gar_gemm's split_k and gar_splitk_residual_rmsnorm take at most SPLITK_MAX_ROWS rows; larger batches
        # keep EPI_RES)
        want = self.DOWN_SPLIT_K or (4 if C_l <= 2048 else 2)
        split = want if (B > self.FUSE_NORM_MAX_BATCH and B <= self.SPLITK_MAX_ROWS and bf16
                         and F % (64 * want) == 0 and C_l <= 4096) else 1
        partial = self._buf(key, "down_partial", (split, B, C_l), torch.float32) if split > 1 else None
        normed = None
        gu_folded = folded and (self.DECODE_GU_NORM_FOLDED or "gu" not in self.layers[0])
        qkv_folded = folded and (self.DECODE_GU_NORM_FOLDED or "qkv" not in self.layers[0])
        L = len(self.layers)
        xn_ready = False            # xn holds RMSNorm(h; this layer's input_layernorm) — written by the previous layer's reduce
        for li, ly in enumerate(self.layers):
            if qkv_folded:
                gemm(h, ly["qkv_f"], qkv, norm_folded=True, norm_eps=t.rms_norm_eps)
            elif fuse:
                gemm(h, ly["qkv"], qkv, norm_w=ly["ln1"], norm_eps=t.rms_norm_eps)
            else:
                if not xn_ready:
                    ops.rmsnorm(h, self.unit_rms if use_folded_w else ly["ln1"], t.rms_norm_eps, out=xn)
                gemm(xn, ly["qkv_f"] if use_folded_w else ly["qkv"], qkv)
            # bf16: RoPE, q scale and the cache append run inside the attention launch (one launch instead of two)
            if fan:             # prompt rows once per kv head for up to 32 / G siblings, then each row's own generated rows
                ops.attention_decode_fanout(qkv, cos, sin, fan["Kp"][li], fan["Vp"][li], st["Kc"][li], st["Vc"][li], att, fan["B"],
                                            fan["N"], Hq, Hkv, hd, fan["Sp"], Smax - fan["Sp"], st["counters"][3:4],
                                            st["counters"][0:1], q_scale, nsplit, dws, left_pad=fan["left_pad"], strip_order=strip)
            elif self.kv_fp8:   # the fp8 cache has only the fused form: the new row is quantized inside the launch
                ops.attention_decode_qkv_fp8(qkv, cos, sin, st["Kc"][li], st["Vc"][li], st["Ks"][li], st["Vs"][li], att, B, Hq, Hkv,
                                             hd, Smax, pos_dev, q_scale, nsplit, dws, left_pad=st["left_pad"], strip_order=strip)
            elif not (self.DECODE_ATTN_TAKES_QKV and
                    ops.attention_decode_qkv(qkv, cos, sin, st["Kc"][li], st["Vc"][li], att, B, Hq, Hkv, hd, Smax, pos_dev,
                                             q_scale, nsplit, dws, left_pad=st["left_pad"], strip_order=strip)):
                ops.llm_qkv_post(qkv, cos, sin, Q, st["Kc"][li], st["Vc"][li], B, 1, 1, Hq, Hkv, hd, Smax, 0, pos_dev, q_scale,
                                 left_pad=st["left_pad"], strip_order=strip)
                ops.attention_decode(Q, st["Kc"][li], st["Vc"][li], att, B, Hq, Hkv, hd, Smax, kvlen_dev, nsplit, dws,
                                     kv_start=st["left_pad"])
            gemm(att, ly["o"], h, hip.EPI_RES, residual=h)
            if gu_folded:       # W diag(g) + row sums of squares off the matrix pipe: no RMSNorm launch, no normalised copy
                gemm(h, ly["gu_f"], ff, hip.EPI_SWIGLU, norm_folded=True, norm_eps=t.rms_norm_eps)
            elif fuse:
                gemm(h, ly["gu"], ff, hip.EPI_SWIGLU, norm_w=ly["ln2"], norm_eps=t.rms_norm_eps)
            else:
                ops.rmsnorm(h, self.unit_rms if use_folded_w else ly["ln2"], t.rms_norm_eps, out=xn)
                gemm(xn, ly["gu_f"] if use_folded_w else ly["gu"], ff, hip.EPI_SWIGLU)
            xn_ready = False
            if split > 1:
                gemm(ff, ly["down"], None, partial=partial)
                lastl = li + 1 == L
                # h += down (one rounding, like EPI_RES); the reduce also writes the RMSNorm the next GEMV wants when that GEMV
                # does not take it folded: the final norm for the head, or the next layer's input_layernorm
                if lastl:
                    ops.splitk_residual_rmsnorm(partial, h, self.final_norm, t.rms_norm_eps, out=xn)
                    normed = xn
                elif qkv_folded:
                    ops.splitk_residual_rmsnorm(partial, h, None, t.rms_norm_eps, out=None)
                else:
                    nxt = self.unit_rms if use_folded_w else self.layers[li + 1]["ln1"]
                    ops.splitk_residual_rmsnorm(partial, h, nxt, t.rms_norm_eps, out=xn)
                    xn_ready = True
            else:
                gemm(ff, ly["down"], h, hip.EPI_RES, residual=h)
        logits = self._head(h, B, st, _PickTargets.of(st, out_tokens), normed=normed, decode=True)
        ops.counter_add(st["counters"][0:3], 1)
        return logits

    # ---- pass planning --------------------------------------------------------------------------------------------
    VIT_CHUNK_ROWS = 400_000      # row caps of one vision-tower / prefill pass (activation workspaces: ~28 KB resp.
    PREFILL_CHUNK_ROWS = 131_072  # ~38 KB per row for GAR-1B); the 4-GiB operand limit of the tile GEMM caps them too

    def _plan_passes(self, B: int, tiles: int, S: int):
        """(image tiles per vision-tower pass, sequences per prefill pass), see gar_amd/planner.py."""
        if self.prefill_chunk is not None:
            c = max(1, min(B, self.prefill_chunk))
            seq = [min(c, B - b) for b in range(0, B, c)]
            return [n * tiles for n in seq], seq
        cfg = self.config
        v, t = cfg.mllm_config.vision_config, cfg.mllm_config.text_config
        cus = hip.num_cus(self.device.index or 0)
        Da = v.num_heads * self.v_hd
        vit_gemms = [(3 * Da, v.embed_dim), (v.embed_dim, Da), (v.mlp_dim, v.embed_dim), (v.embed_dim, v.mlp_dim)]
        lim = (1 << 31) - 4096                 # A operand bytes / 2 addressable by the GEMM's buffer descriptor
        vrows = min(self.VIT_CHUNK_ROWS, lim // max(v.mlp_dim, self.Kp, 3 * Da))
        tile_chunks = plan_chunks(B * tiles, v.num_patches + self.npt, vit_gemms, vrows, cus) if tiles else []
        qd = (t.num_attention_heads + 2 * t.num_key_value_heads) * t.head_dim
        llm_gemms = [(qd, t.hidden_size), (t.hidden_size, t.num_attention_heads * t.head_dim),
                     (2 * t.intermediate_size, t.hidden_size), (t.hidden_size, t.intermediate_size)]
        lrows = min(self.PREFILL_CHUNK_ROWS, lim // max(t.intermediate_size, qd))
        seq_chunks = plan_chunks(B, S, llm_gemms, lrows, cus)
        return tile_chunks, seq_chunks

    def _left_pad(self, attention_mask, B: int, S: int, validate: bool):
        """(left_pad int32 [B] or None, the mask on the device when validate=False or None) of a LEFT-padded attention_mask."""
        left_pad = am_dev = None
        if attention_mask is not None:
            am = (attention_mask != 0)
            if tuple(am.shape) != (B, S):
                raise ValueError(f"attention_mask {tuple(am.shape)} does not match input_ids {(B, S)}")
            if validate:
                amc = am.cpu()
                if not bool(amc.all()):
                    if not bool((amc[:, 1:] >= amc[:, :-1]).all()) or not bool(amc[:, -1].all()):
                        raise hip.GarError("attention_mask must be LEFT-padded (zeros only in front of every prompt): a "
                                           "right-padded row would be continued after its padding")
                    left_pad = (S - amc.sum(1)).to(torch.int32).to(self.device)
            else:                      # no host sync: the zero count is the pad; the device-side input check (gar_input_check)
                am_dev = am.to(self.device).contiguous()       # raises INPUT_MASK_NOT_LEFT_PADDED for a row that is not 0...01...1
                left_pad = (S - am_dev.sum(1)).to(torch.int32)
        return left_pad, am_dev

    def _prompt_chunks(self, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, validate: bool,
                       feature_replay_video: bool = False, video_frame_tokens: Optional[Sequence[int]] = None):
        """The prompt phase up to the prefill, shared by generate_begin and score: the vision tower over chunks of image tiles,
        then per chunk of sequences the assembled and RoI-replayed embeddings. Yields (b0, b1, embeds [b1 - b0, S, C]); the
        caller prefills each chunk before it asks for the next (the embeddings buffer is reused)."""
        cfg = self.config
        B, S = input_ids.shape
        C_l = cfg.mllm_config.text_config.hidden_size
        tiles = 0
        if pixel_values is not None:
            tiles = pixel_values.shape[0] // B if pixel_values.dim() == 4 else pixel_values.shape[1]
            pv = pixel_values.reshape(B, tiles, *pixel_values.shape[-3:])
            gm = None if global_mask_values is None else global_mask_values.reshape(pv.shape)
            if feature_replay_video and video_frame_tokens is None:
                # <|reserved_special_token_{2+f}|> of frame f (modeling_perception_lm.py:777-780): the first
                # prompt_numbers ids are config.crop_tokens_ids, the following reserved tokens are consecutive ids
                base = list(self.crop_tokens_ids)
                video_frame_tokens = (base + [base[-1] + 1 + i for i in range(max(0, tiles - len(base)))])[:tiles]
        # The vision tower runs over chunks of image tiles and the prefill over chunks of sequences (bounded activation
        # memory, GEMM operands < 4 GiB; sizes from _plan_passes); the projector output of the whole batch is kept, and
        # the decode loop then serves all B sequences of the shared KV cache in one weight pass per token.
        tile_chunks, seq_chunks = self._plan_passes(B, tiles, S)
        proj_all, rows_per_sample = None, 0
        if pixel_values is not None:
            v = cfg.mllm_config.vision_config
            rows_per_sample = tiles * (v.num_patches + self.npt)
            proj_all = self._buf(("vit", "all"), "proj_all", (B * rows_per_sample, C_l))
            pvf = pv.reshape(B * tiles, *pv.shape[-3:])
            gmf = None if gm is None else gm.reshape(pvf.shape)
            t0 = 0
            for tc in tile_chunks:
                r0, r1 = t0 * (v.num_patches + self.npt), (t0 + tc) * (v.num_patches + self.npt)
                self.get_image_features(pvf[t0:t0 + tc], None if gmf is None else gmf[t0:t0 + tc], pooled=False,
                                        out=proj_all[r0:r1])
                t0 += tc
        b0 = 0
        for sc in seq_chunks:
            b1 = b0 + sc
            ids_c = input_ids[b0:b1]
            if pixel_values is not None:
                ar_c = None if aspect_ratios is None else aspect_ratios[b0:b1]
                embeds = self.build_inputs_embeds(ids_c, None, bboxes[b0:b1], ar_c, tiles, validate,
                                                  video_frame_tokens if feature_replay_video else None,
                                                  proj=proj_all[b0 * rows_per_sample:b1 * rows_per_sample])
            else:
                embeds = self._buf(("emb", b1 - b0, S), "embeds", (b1 - b0, S, C_l))
                ops.embed_assemble(ids_c.to(self.device, torch.int64).contiguous(), None, self.E, None, embeds, 0)
            yield b0, b1, embeds
            b0 = b1

    # ---- generate -------------------------------------------------------------------------------------------------
    def generate(self, *args, **kwargs) -> GenerateOutput:
        """Greedy region captioning, reference semantics of GARModel.generate (modeling_gar.py:295-428): the prompt phase
        (:meth:`generate_begin`: vision tower, sequence assembly + RoI replay, prefill, first token) followed by the decode
        loop (:meth:`generate_finish`) on the current stream. See generate_begin for the arguments."""
        return self.generate_finish(self.generate_begin(*args, **kwargs))

    def generate_pipelined(self, samples, **kwargs) -> List[GenerateOutput]:
        """``[generate(**s, **kwargs) for s in samples]`` through a :class:`GenerationPipeline`: the decode loop of batch i
        runs on a second HIP stream beside the prompt phase of batch i + 1. Bit-identical to the sequential calls."""
        pipe = GenerationPipeline(self, **kwargs)
        outs = []
        for smp in samples:
            outs.extend(pipe.submit(smp))
        outs.extend(pipe.flush())
        return outs

    @_on_model_device
    @torch.no_grad()
    def generate_begin(self, pixel_values=None, global_mask_values=None, aspect_ratios=None, bboxes=None, input_ids=None,
                       attention_mask=None, generation_config=None, output_hidden_states=None, return_dict=None,
                       max_new_tokens: Optional[int] = None, eos_token_id=None, use_graph: bool = True, validate: bool = True,
                       return_logits: bool = False, sync_every: int = 16, feature_replay_video: bool = False,
                       video_frame_tokens: Optional[Sequence[int]] = None, forced_tokens: Optional[torch.Tensor] = None,
                       state_slot: int = 0, seed: Optional[int] = None, return_logprobs: bool = False,
                       top_logprobs: int = 0, candidate_token_ids: Optional[Sequence[int]] = None, logits_processing=None,
                       sampling_warpers=None, beam_search=None, constraint=None, _row_words=None, _row_proc=None,
                       **generate_kwargs) -> "_PendingGeneration":
        """Region captioning, reference semantics of GARModel.generate (modeling_gar.py:295-428): greedy search, or — with
        ``do_sample=True`` in the generation config — temperature / top-k / top-p sampling on the device (``seed``: the Philox key of
        the request; None draws one from torch's global generator).

        B = input_ids.shape[0] samples are processed together (the reference handles B=1 per call; its loop over
        ``batch_idx`` is kept). ``pixel_values`` / ``global_mask_values``: [B*(T+1), 3, H, W] (flattened tiles as the
        reference's callers pass them) or [B, T+1, 3, H, W].

        ``forced_tokens`` [B, n] (tests): teacher forcing — ``sequences`` / ``logits`` still report what the model chose at
        every step, but the token fed back as step j's input is ``forced_tokens[:, j]``, so two models (bf16 vs f32) can be
        compared on identical contexts over a whole caption.

        ``return_logprobs``: the output carries the log-probability of every generated token (``token_logprobs`` under the raw
        logits, ``token_logprobs_warped`` under the distribution a sampled token was drawn from, their per-row sums and
        ``n_tokens``), written by the launch that picks the token — no dense logits leave the step. ``sequences`` are
        bit for bit those of the call without it.

        ``top_logprobs`` = k (0..min(32, vocab)) / ``candidate_token_ids`` (at most 64 ids in [0, vocab)): per generated token the
        k most likely tokens with their log-probabilities (``top_logprob_ids`` / ``top_logprobs`` [B * N, n, k], best first, equal
        logits by ascending id) and the log-probabilities of the given ids (``candidate_logprobs`` [B * N, n, C]). The
        values are always RAW log-probabilities x[i] - logsumexp(x) of the step's logits, also with ``do_sample=True`` — the warped
        value of the drawn token stays ``token_logprobs_warped``. Columns behind a row's first eos hold id -1 / value 0.0; with
        ``forced_tokens`` the fields describe the model's own distribution. Independent of ``return_logprobs``; tokens unchanged.

        ``logits_processing``: a :class:`LogitsProcessing` (or a dict of its fields) — repetition penalty, no-repeat n-gram size,
        min_new_tokens, suppress / begin-suppress tokens and bad words, HF's processors applied on the device to every step's
        logits before the pick, or before temperature / top-k / top-p with ``do_sample=True``. As the reference calls
        HF's generate with ``inputs_embeds`` only, a row's history is its own generated tokens: the prompt is never penalised or
        scanned. ``return_logits=True`` then returns the processed scores (HF's ``scores``). None or all-neutral values: the path
        and the launches of a call without it. Refused with ``GarError``: together with ``forced_tokens`` (the fed history would
        differ from ``sequences``), and with ``return_logprobs`` / ``top_logprobs`` / ``candidate_token_ids`` (defined over the raw
        logits). The GenerationConfig fields of the same names stay refused.

        ``sampling_warpers``: a :class:`SamplingWarpers` (or a dict of its fields) — ``min_p``, ``typical_p``, ``epsilon_cutoff``,
        ``eta_cutoff``: HF's four further warpers, applied on the device in HF's order after temperature / top-k / top-p and before
        the draw, each over the tokens the stage before it left. Needs ``do_sample=True`` (``ValueError`` otherwise).
        ``token_logprobs_warped`` is then the drawn token's log-probability under the final kept set. None or all-neutral values:
        the path, the launches and the captured graph of a call without it. The GenerationConfig fields of the same names stay
        refused.

        ``beam_search``: a :class:`BeamSearch` (or a dict of its fields) — HF's beam search (``GenerationMixin._beam_search``,
        do_sample=False) on the device: ``num_beams`` beams per prompt over ONE prompt phase and, in the 16-bit
        modes, one shared prompt cache. ``sequences`` is then [B * num_return_sequences, n] — each prompt's hypotheses best first,
        ``pad`` behind each one's end, n the longest returned one — and ``sequences_scores`` holds their scores. Equal scores
        order by (beam, token) ascending where HF leaves them to torch.topk. Refused with ``GarError``: together with
        ``do_sample``, ``sampling_warpers``, ``logits_processing`` (HF processes the log-probabilities behind the softmax with each
        beam's own history: a follow-up), ``return_logprobs`` / ``top_logprobs`` / ``candidate_token_ids``, ``forced_tokens`` and
        ``kv_cache_dtype="fp8"``, and ``num_beams * max(2, 1 + number of eos ids) > 32``. The GenerationConfig fields
        ``num_beams`` / ``length_penalty`` stay refused.

        ``constraint``: a :class:`PhraseConstraint` (or a dict with ``phrases``) — the answer is taken from a closed set of token
        phrases, shared by the prompts or one set per prompt: HF's ``PrefixConstrainedLogitsProcessor`` under the
        callback "the generated tokens stay a prefix of one of the prompt's phrases", as one launch per step that walks a token
        trie on the device and masks the logits, behind ``logits_processing`` and in front of the pick. Needs ``eos_token_id`` (at
        most ``MAX_EOS_IDS`` ids): eos is allowed once a phrase is complete, and alone behind it. ``phrase_index`` reports the
        phrase every row completed. ``return_logits=True`` returns the masked scores (HF's ``scores``); ``return_logprobs`` /
        ``top_logprobs`` / ``candidate_token_ids`` are taken over the masked scores too, so ``sum_logprobs`` is the chosen
        phrase's log-probability renormalised over the allowed set at every step. Composes with ``do_sample``,
        ``sampling_warpers``, ``num_return_sequences`` and ``logits_processing``. None: the path, the launches and the captured
        graph of a call without it. Refused with ``GarError``: together with ``beam_search``, ``forced_tokens`` and per-row
        requests (``ContinuousBatcher``), and in ``GenerationPipeline`` / ``generate_pipelined``."""
        constraint = PhraseConstraint.coerce(constraint)
        if constraint is not None:
            for name, on in (("beam_search", beam_search is not None), ("forced_tokens", forced_tokens is not None),
                             ("ContinuousBatcher.submit", _row_words is not None or _row_proc is not None)):
                if on:
                    raise hip.GarError(f"constraint with {name} is not implemented (DESIGN 7.13)")
        beam = BeamSearch.coerce(beam_search)
        if beam is not None:
            for name, on in (("sampling_warpers", sampling_warpers is not None), ("logits_processing", logits_processing is not None),
                             ("return_logprobs", return_logprobs), ("top_logprobs", top_logprobs),
                             ("candidate_token_ids", candidate_token_ids), ("forced_tokens", forced_tokens is not None),
                             ("per-row requests", _row_words is not None or _row_proc is not None)):
                if on:
                    raise hip.GarError(f"beam_search with {name} is not implemented (DESIGN 7.11)")
            if self.kv_cache_dtype == "fp8":
                raise hip.GarError("beam_search with kv_cache_dtype='fp8' is not implemented (the beams' cache rows are reordered as "
                                   "16-bit / f32 rows, and the shared-prefix decode attention reads 16-bit caches)")
        warpers = SamplingWarpers.coerce(sampling_warpers)
        warpers = None if warpers.neutral else warpers
        proc = LogitsProcessing.coerce(logits_processing)
        proc = None if proc.neutral else proc
        if _row_proc is not None and (proc is not None or forced_tokens is not None):
            raise hip.GarError("generate_begin: per-row processing blocks go with no logits_processing of the call's own and no "
                               "forced_tokens")
        if proc is not None:
            if forced_tokens is not None:
                raise hip.GarError("logits_processing with forced_tokens is not implemented (the processors read the history from the "
                                   "token matrix, which would differ from the tokens fed back)")
            for name, on in (("return_logprobs", return_logprobs), ("top_logprobs", top_logprobs),
                             ("candidate_token_ids", candidate_token_ids)):
                if on:
                    raise hip.GarError(f"logits_processing with {name} is not implemented ({name} is defined over the unprocessed "
                                       "logits, DESIGN 7.5 / 7.6; over processed scores it is a follow-up)")
        top_k_lp, cands = top_logprob_options(top_logprobs, candidate_token_ids, self.config.mllm_config.text_config.vocab_size)
        sampling = None
        N = 1
        get = _option_reader(generation_config, generate_kwargs)
        if get is not None:
            if beam is not None and get("do_sample", False):
                raise hip.GarError("beam_search with do_sample=True (beam-search multinomial sampling) is not implemented")
            N = _num_return_sequences(get, self.kv_cache_dtype)
            _refuse_non_greedy(get)
            if get("do_sample", False):
                sampling = _sampling_options(get)
            max_new_tokens = max_new_tokens or get("max_new_tokens")
            if eos_token_id is None:
                eos_token_id = get("eos_token_id")
            pad_token_id = get("pad_token_id")
        else:
            pad_token_id = None
        if warpers is not None and sampling is None:
            raise ValueError("sampling_warpers acts on a sampled request only: pass do_sample=True (greedy search draws nothing "
                             "to warp)")
        if warpers is not None and _row_words is not None:
            raise hip.GarError("generate_begin: per-row requests carry no sampling_warpers")
        max_new_tokens = int(max_new_tokens or 64)
        cfg = self.config
        B, S = input_ids.shape
        if constraint is not None:
            n_eos = 0 if eos_token_id is None else (len(eos_token_id) if isinstance(eos_token_id, (list, tuple)) else 1)
            if not 1 <= n_eos <= GARModel.MAX_EOS_IDS:
                raise hip.GarError(f"constraint needs eos_token_id with 1..{GARModel.MAX_EOS_IDS} ids on the device, got {n_eos}: a complete "
                                   "phrase could never end otherwise")
            if constraint.per_prompt and len(constraint.sets) != B:
                raise ValueError(f"constraint: {len(constraint.sets)} per-prompt phrase sets for a batch of {B} prompts")
        if beam is not None:
            n_eos = 0 if eos_token_id is None else (len(eos_token_id) if isinstance(eos_token_id, (list, tuple)) else 1)
            try:            # HF's beams_to_keep: known only now that the eos ids are
                M = beam.candidates(n_eos)
                beam.pack(max_new_tokens, [0] * n_eos)
            except BeamBudgetError as e:
                raise hip.GarError(str(e)) from None
            if M > cfg.mllm_config.text_config.vocab_size:
                raise hip.GarError(f"beam_search: {M} candidates per step above vocab_size {cfg.mllm_config.text_config.vocab_size}")
            self._check_decode_rows(B * beam.num_beams, "generate(beam_search=...)")
            return self._generate_begin_beam(beam, M, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids,
                                             attention_mask, max_new_tokens, eos_token_id, pad_token_id, use_graph, validate,
                                             return_logits, sync_every, feature_replay_video, video_frame_tokens, state_slot)
        self._check_decode_rows(B * N, "generate")
        if N > 1 and _row_proc is not None:
            raise hip.GarError("generate_begin: per-row processing blocks with num_return_sequences > 1 are not implemented")
        if N > 1:
            return self._generate_begin_fanout(N, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, attention_mask,
                                               max_new_tokens, eos_token_id, pad_token_id, sampling, seed, use_graph, validate,
                                               return_logits, sync_every, feature_replay_video, video_frame_tokens, forced_tokens,
                                               state_slot, return_logprobs, top_k_lp, cands, proc, warpers, constraint)
        left_pad, forced_tokens = self._begin_inputs(input_ids, attention_mask, validate, forced_tokens)
        # KV capacity in buckets of 256 positions: evaluation loops with a different prompt length per item reuse one
        # cache, one token buffer ([B, Smax], sliced) and one captured decode graph per bucket
        Smax = _round_up(S + max_new_tokens, 256)
        skey, st = self._llm_state(B, Smax, state_slot)
        out_tokens = self._buf(skey, "out_tokens", (B, Smax), torch.int64, zero=True)[:, :max_new_tokens]
        st["lp"] = self._logprob_planes(skey, out_tokens, (B, Smax)) if return_logprobs else None
        self._topk_planes(skey, st, (B, Smax), top_k_lp, cands)
        eos_list, eos_on_device = self._arm_state(st, left_pad, eos_token_id, sampling, seed, warpers)
        self._arm_processing(skey, st, proc, eos_list, eos_on_device)
        self._arm_constraint(skey, st, constraint, B, 1, Smax)
        if _row_words is not None:      # ContinuousBatcher(sampling=True): the rows of this prompt phase pick under requests of their own
            if len(_row_words) != B or sampling is not None:
                raise hip.GarError("generate_begin: one request of eight words per row, and no do_sample of the call's own")
            st["row_words"] = self._buf(skey, "row_words", (B, ops.SAMPLE_ROW_WORDS), torch.int32)
            st["row_words"].copy_(self._upload([w for r in _row_words for w in r], torch.int32, cache=False).view(B, -1))
        if _row_proc is not None:       # ContinuousBatcher(processing=True): the rows' own blocks, their step 0 at column 0 of this state
            if len(_row_proc) != B or any(not ops.LOGITS_PROCESS_HEADER <= len(r) <= ops.LOGITS_PROCESS_WORDS for r in _row_proc):
                raise hip.GarError(f"generate_begin: one processing block of {ops.LOGITS_PROCESS_HEADER}.."
                                   f"{ops.LOGITS_PROCESS_WORDS} words per row")
            st["row_proc"] = self._buf(skey, "row_proc", (B, ops.LOGITS_PROCESS_WORDS), torch.int32)
            st["row_proc"].copy_(_process_blocks(_row_proc))
        to = _PickTargets.of(st, out_tokens)
        V = cfg.mllm_config.text_config.vocab_size
        first_logits = []
        for b0, b1, embeds in self._prompt_chunks(pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, validate,
                                                  feature_replay_video, video_frame_tokens):
            last = self._prefill(embeds, st, Smax, b0)
            lg = self._head(last, b1 - b0, st, to.rows(b0, b1))
            if forced_tokens is not None:
                st["cur"][b0:b1].copy_(forced_tokens[b0:b1, 0])
            if return_logits:
                first_logits.append(lg[:, :V].float().clone())
        # counters after prefill: pos = S (position of the next token), kv_len = S+1 (incl. it), step = 1
        # (fills take their value as a kernel argument: no host-to-device copy, nothing the host waits for)
        c = st["counters"]
        c[0:1].fill_(S)
        c[1:2].fill_(S + 1)
        c[2:3].fill_(1)
        c[3:4].zero_()
        return self._begin_pending(first_logits, eos_list, eos_on_device=eos_on_device, st=st, skey=skey, B=B, Smax=Smax,
                                   out_tokens=out_tokens, max_new_tokens=max_new_tokens, pad_token_id=pad_token_id,
                                   return_logits=return_logits, forced_tokens=forced_tokens, use_graph=use_graph, validate=validate,
                                   sync_every=sync_every, N=1, constraint=constraint)

    def _begin_inputs(self, input_ids, attention_mask, validate: bool, forced_tokens):
        """What both begin methods do with a request's inputs before they touch a state: the mask's left padding, forced_tokens
        moved to the device, and the flag word of the device-side input check with the mask's check launched into it (it reads the
        ids and the mask and writes the flag only, so its place before the state's zeroing fills is free). Returns (left_pad,
        forced_tokens). attention_mask is forwarded to the Llama generate by the reference (modeling_gar.py:418-426). A LEFT-padded batch
        (HF's convention for generation: prompts of different lengths right-aligned, zeros in front) is supported: a sequence keeps
        its rows in the padded layout, its RoPE positions count from its first real token and the padding keys stay hidden (HF:
        position_ids = cumsum(mask) - 1, causal mask AND attention_mask)."""
        B, S = input_ids.shape
        left_pad, am_dev = self._left_pad(attention_mask, B, S, validate)
        if forced_tokens is not None:
            forced_tokens = forced_tokens.to(self.device, torch.int64)
        self._input_flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        if am_dev is not None:      # validate=False: the mask's left-padded form is checked on the device, flag read by the caller
            ops.input_check(input_ids.to(self.device, torch.int64).contiguous(), self.config.mllm_config.text_config.vocab_size,
                            None, 0, None, 0, None, self._input_flags, attn_mask=am_dev)
        return left_pad, forced_tokens

    def _begin_pending(self, first_logits, eos_list, **kw) -> "_PendingGeneration":
        """what both begin methods return: the request's words (``kw``) for :meth:`generate_finish`; ``first_logits`` holds the first
        tokens' logits per prompt chunk when they were asked for, and is empty otherwise"""
        return _PendingGeneration(V=self.config.mllm_config.text_config.vocab_size,
                                  all_logits=[torch.cat(first_logits, 0)] if first_logits else [], eos=set(eos_list),
                                  eos_first=eos_list[0] if eos_list else None, input_flags=self._input_flags, **kw)

    def _logprob_planes(self, skey, out_tokens, shape):
        """(raw, warped) f32 planes of a return_logprobs request: buffers of the state shaped like its token buffer and sliced
        like ``out_tokens``, so (row stride, step column) address all three alike."""
        return tuple(self._buf(skey, name, shape, torch.float32, zero=True)[:, :out_tokens.shape[1]]
                     for name in ("lp_raw", "lp_warped"))

    def _arm_state(self, st, left_pad, eos_token_id, sampling, seed, warpers=None):
        """A state's request words before the prompt phase: counters, left_pad, the stopping criterion's latches and eos table, the
        sampling parameters and Philox key, and the eight floats of a request with sampling_warpers. Returns (eos ids, whether the
        device holds them)."""
        st["counters"].zero_()
        if left_pad is None:
            st["left_pad"].zero_()
        else:
            st["left_pad"].copy_(left_pad)
        eos_list = []
        if eos_token_id is not None:
            eos_list = [int(e) for e in (eos_token_id if isinstance(eos_token_id, (list, tuple)) else [eos_token_id])]
        # the stopping criterion lives on the device (gar_argmax latches each row's first eos step): fills take their value as a
        # kernel argument, the id table is one small upload
        eos_on_device = len(eos_list) <= self.MAX_EOS_IDS
        st["finished"].fill_(-1)
        st["done_count"].zero_()
        st["eos_ids"].fill_(-1)
        if eos_list and eos_on_device:
            st["eos_ids"][:len(eos_list)].copy_(self._upload(eos_list, torch.int64))
        st["sampling"] = sampling is not None
        if sampling is not None:
            if seed is None:
                seed = _draw_seed()
            tail = warpers.pack() if warpers is not None else [0.0, 1.0, 0.0, 0.0]         # no sampling_warpers: all four off
            st["sample_params"].copy_(self._upload([sampling[0], sampling[1], float(sampling[2]), 0.0] + tail, torch.float32))
            st["sample_seed"].copy_(self._upload([int(seed)], torch.int64, cache=False))
        st["warpers"] = sampling is not None and warpers is not None
        return eos_list, eos_on_device

    def _generate_begin_fanout(self, N, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, attention_mask,
                               max_new_tokens, eos_token_id, pad_token_id, sampling, seed, use_graph, validate, return_logits,
                               sync_every, feature_replay_video, video_frame_tokens, forced_tokens, state_slot,
                               return_logprobs=False, top_k_lp=0, cands=(), proc=None, warpers=None, constraint=None):
        """generate_begin of a num_return_sequences = N > 1 request (do_sample): ONE prompt phase over the B prompts, N first
        tokens drawn from each prompt's logits, and a state of B * N rows for :meth:`generate_finish` — row b * N + i is sample i
        of prompt b, its draws counted by (seed, step, b * N + i) as the replicated batch's would be.
        16-bit models: the rows share the prompt's cache rows (the (B, Sp) state the prefill wrote) and keep only their generated
        tokens (gar_attention_decode_fanout). f32 parity mode: the prompt's rows are copied into an ordinary (B * N, Smax) state
        and the plain step decodes it — the N - 1 prompt phases are saved, the cache is not shared."""
        t = self.config.mllm_config.text_config
        B, S = input_ids.shape
        R, V = B * N, t.vocab_size
        if forced_tokens is not None and forced_tokens.shape[0] != R:
            raise ValueError(f"forced_tokens must have B * num_return_sequences = {R} rows, got {forced_tokens.shape[0]}")
        left_pad, forced_tokens = self._begin_inputs(input_ids, attention_mask, validate, forced_tokens)
        shared = self.dtype in HALF_DTYPES
        if shared:
            Sp, T = _round_up(S, 256), _round_up(max_new_tokens, 64)
            _, pst = self._llm_state(B, Sp, state_slot)
            skey, st = self._llm_state(R, T, state_slot, fan=(B, Sp))
            st["fan"] = dict(B=B, N=N, Sp=Sp, Kp=pst["Kc"], Vp=pst["Vc"], left_pad=pst["left_pad"])
            Smax = Sp + T               # what generate_finish hands to the step: RoPE table rows; T = Smax - Sp
        else:
            Sp = Smax = _round_up(S + max_new_tokens, 256)
            _, pst = self._llm_state(B, Smax, state_slot)
            skey, st = self._llm_state(R, Smax, state_slot)
        out_tokens = self._buf(skey, "out_tokens", (R, Smax - Sp if shared else Smax), torch.int64, zero=True)[:, :max_new_tokens]
        st["lp"] = self._logprob_planes(skey, out_tokens, (R, Smax - Sp if shared else Smax)) if return_logprobs else None
        self._topk_planes(skey, st, (R, Smax - Sp if shared else Smax), top_k_lp, list(cands))
        self._arm_state(pst, left_pad, None, None, None)
        eos_list, eos_on_device = self._arm_state(st, None, eos_token_id, sampling, seed, warpers)
        self._arm_processing(skey, st, proc, eos_list, eos_on_device)
        self._arm_constraint(skey, st, constraint, B, N, Smax - Sp if shared else Smax)
        to = _PickTargets.of(st, out_tokens)
        first_logits = []
        for b0, b1, embeds in self._prompt_chunks(pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, validate,
                                                  feature_replay_video, video_frame_tokens):
            last = self._prefill(embeds, pst, Sp, b0)
            lg = self._head(last, b1 - b0, pst, None)
            r0, r1 = _fanout_rows(b0, b1, N)
            # the history of every row is empty at step 0: the N draws of a prompt share ONE processed row
            self._process(lg, V, st, None)
            self._constrain(lg, V, st, None, None if to.nodes is None else to.nodes[r0:r1:N])      # the N rows share the prompt's root
            lg = lg.repeat_interleave(N, 0)                                        # the SAME logits for the N draws
            self._pick(lg, V, st, to.rows(r0, r1), process=False)   # the N rows of a prompt carry that prompt's top-k / candidate values at step 0
            if forced_tokens is not None:
                st["cur"][r0:r1].copy_(forced_tokens[r0:r1, 0])
            if return_logits:
                first_logits.append(lg[:, :V].float())
        c = st["counters"]
        if shared:                      # [t, -, step, P]: the first decode step appends at suffix row 0
            c[2:3].fill_(1)
            c[3:4].fill_(S)
        else:                           # the prompts' cache rows, N times; counters as generate_begin leaves them
            L, Hkv, hd = t.num_hidden_layers, t.num_key_value_heads, t.head_dim
            for name in ("Kc", "Vc"):
                st[name].view(L, B, N, Hkv, Smax, hd).copy_(pst[name][:, :, None])
            st["left_pad"].copy_(pst["left_pad"].repeat_interleave(N))
            c[0:1].fill_(S)
            c[1:2].fill_(S + 1)
            c[2:3].fill_(1)
        return self._begin_pending(first_logits, eos_list, eos_on_device=eos_on_device, st=st, skey=skey, B=R, Smax=Smax,
                                   out_tokens=out_tokens, max_new_tokens=max_new_tokens, pad_token_id=pad_token_id,
                                   return_logits=return_logits, forced_tokens=forced_tokens, use_graph=use_graph, validate=validate,
                                   sync_every=sync_every, N=N, constraint=constraint)

    # ---- teacher-forced scoring ---------------------------------------------------------------------------------------
    XENT_CHUNK_ROWS = 8192          # scored rows per fused-head launch: partials workspace <= chunk x 16 KiB at V = 128256
    XENT_DENSE_ROWS = 64            # rows per launch of the dense form (skinny GEMM to [rows, V] logits + combine)

    def forward(self, data, data_samples=None, mode: str = "loss"):
        """The reference's training entry point (modeling_gar.py:74-246) in its ``mode="loss"`` form: ``{"loss": tensor}``, HF's
        causal-LM loss of ``data["labels"]`` with labels inside every replayed crop-token span set to -100, positions 0..S-1 and
        an all-ones attention mask. ``data`` holds pixel_values, global_mask_values, input_ids, aspect_ratios, bboxes, labels.
        B >= 1 (the reference asserts 1): the mean over all valid tokens of the batch, as HF computes it. No gradients."""
        if mode != "loss":
            raise hip.GarError(f"forward(mode={mode!r}): only mode='loss' is built (the reference's 'predict' / 'tensor' "
                               "modes return an undefined value)")
        out = self.score(data["pixel_values"], data["global_mask_values"], data["aspect_ratios"], data["bboxes"],
                         data["input_ids"], data["labels"])
        return {"loss": out.loss}

    __call__ = forward

    @_on_model_device
    @torch.no_grad()
    def score(self, pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, labels, attention_mask=None,
              validate: bool = True, state_slot: int = 0) -> ScoreOutput:
        """Teacher-forced log-probabilities of ``labels`` [B, S] (-100 = ignored) under the prompt ``input_ids`` [B, S]: the
        batched form under :meth:`forward`. Column t + 1 of ``token_logprobs`` holds log p(labels[t + 1] | rows 0..t), f32, 0
        where ignored (labels -100, the replayed crop-token spans, padding). Arguments as :meth:`generate_begin`; a LEFT-padded
        ``attention_mask`` follows generate's rules (RoPE positions from each row's first real token, padding keys hidden).

        The prompt phase of generate (vision tower, sequence assembly + RoI replay, prefill) with the last layer at full width,
        then one gather + final-RMSNorm launch over the scored rows and the lm_head fused with the cross-entropy (the tile GEMM
        writes per-strip (max, sum exp) partials, never the [rows, V] logits); below 65 rows, or in f32, 64-row chunks of
        dense logits. Models built with kv_cache_dtype="fp8" or decode_weight_dtype="fp8" score with 16-bit numerics: the
        prompt phase uses neither option.

        ``validate=False``: no host sync. Labels are not checked on the host (one outside [0, vocab) other than -100 is
        ignored and sets INPUT_LABEL_RANGE in ``input_flags``), the input checks of generate(validate=False) go to the same
        flag, and the head runs over every row, since the number of labelled rows is not known without a sync."""
        cfg = self.config
        t = cfg.mllm_config.text_config
        V, C_l = t.vocab_size, t.hidden_size
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, S], got {tuple(input_ids.shape)}")
        B, S = input_ids.shape
        if not torch.is_tensor(labels):
            labels = torch.as_tensor(labels)
        if tuple(labels.shape) != (B, S):
            raise ValueError(f"labels {tuple(labels.shape)} must have the shape of input_ids {(B, S)}")
        if validate:
            lc = labels.detach().cpu().to(torch.int64)
            bad = (lc != -100) & ((lc < 0) | (lc >= V))
            if bool(bad.any()):
                raise ValueError(f"labels must be in [0, {V}) or -100; found {int(lc[bad][0])}")
        left_pad, am_dev = self._left_pad(attention_mask, B, S, validate)
        Smax = _round_up(S, 256)
        skey, st = self._llm_state(B, Smax, state_slot)
        st["counters"].zero_()
        if left_pad is None:
            st["left_pad"].zero_()
        else:
            st["left_pad"].copy_(left_pad)
        self._input_flags = torch.zeros(1, dtype=torch.int32, device=self.device)
        if am_dev is not None:
            ops.input_check(input_ids.to(self.device, torch.int64).contiguous(), V, None, 0, None, 0, None, self._input_flags,
                            attn_mask=am_dev)
        am = None if attention_mask is None else (attention_mask != 0).to(self.device)
        tgt = score_targets(input_ids.to(self.device), labels.to(self.device), self.crop_tokens_ids, am)       # [B, S - 1]
        token_lp = torch.zeros((B, S), dtype=torch.float32, device=self.device)
        sum_lp = torch.zeros((B,), dtype=torch.float32, device=self.device)
        n_tok = torch.zeros((B,), dtype=torch.int32, device=self.device)
        for b0, b1, embeds in self._prompt_chunks(pixel_values, global_mask_values, aspect_ratios, bboxes, input_ids, validate):
            self._prefill(embeds, st, Smax, b0, prune=False)
            self._score_rows(embeds.view((b1 - b0) * S, C_l), tgt[b0:b1], b0, S, validate, token_lp, sum_lp, n_tok)
        loss = -(sum_lp.sum() / n_tok.sum().to(torch.float32))
        return ScoreOutput(token_logprobs=token_lp, sum_logprobs=sum_lp, n_tokens=n_tok, loss=loss,
                           input_flags=None if validate else self._input_flags)

    def _score_rows(self, h: torch.Tensor, tgt: torch.Tensor, b0: int, S: int, validate: bool, token_lp, sum_lp, n_tok):
        """Head + cross-entropy of one prefill chunk: ``h`` [sc * S, C] residual stream after the last layer, ``tgt`` [sc, S - 1]
        targets of rows 0..S-2 (-100 = ignored). validate: only the labelled rows (their list costs one sync); otherwise all."""
        t = self.config.mllm_config.text_config
        V, C_l = t.vocab_size, t.hidden_size
        sc = tgt.shape[0]
        if S < 2:
            return
        src = (torch.arange(sc, device=self.device)[:, None] * S + torch.arange(S - 1, device=self.device)[None, :]).reshape(-1)
        tg = tgt.reshape(-1)
        if validate:
            keep = torch.nonzero(tg != -100).reshape(-1)
            src, tg = src[keep], tg[keep]
        R = int(src.numel())
        if R == 0:
            return
        rows = src.to(torch.int32)
        dest = (rows + b0 * S + 1).to(torch.int32)                  # row t predicts column t + 1 of token_logprobs
        tg32 = tg.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)      # out-of-range labels stay out of range
        xn = self._buf(("score",), "xn", (R, C_l))
        ops.gather_rmsnorm(h, rows, self.final_norm, t.rms_norm_eps, xn)
        flags = self._input_flags
        # equal chunks of at most XENT_CHUNK_ROWS rows; a chunk the fused head takes (16-bit, > 64 rows) runs there with a
        # partials workspace sized to it, any other one as dense [<= 64, V] logits pieces
        n = -(-R // -(-R // self.XENT_CHUNK_ROWS))
        strips = ops.lm_head_xent_strips(V)
        for c0 in range(0, R, n):
            c1 = min(R, c0 + n)
            if ops.lm_head_xent_takes(self.dtype, c1 - c0, V, C_l):
                part = self._buf(("score",), "partials", ((c1 - c0) * strips * 2,), torch.float32)
                tl = self._buf(("score",), "tgt_logit", (c1 - c0,), torch.float32)
                ops.lm_head_xent(xn[c0:c1], self.lm_head, tg32[c0:c1], part, tl)
                ops.xent_combine(tg32[c0:c1], dest[c0:c1], S, token_lp, sum_lp, n_tok, V, partials=part, target_logit=tl,
                                 flags=flags)
                continue
            d = self.XENT_DENSE_ROWS
            logits = self._buf(("score",), "logits", (min(d, c1 - c0), _round_up(V, 64)))
            for r0 in range(c0, c1, d):
                r1 = min(c1, r0 + d)
                ops.gemm(xn[r0:r1], self.lm_head, logits[:r1 - r0])
                ops.xent_combine(tg32[r0:r1], dest[r0:r1], S, token_lp, sum_lp, n_tok, V, logits=logits[:r1 - r0], flags=flags)

    @_on_model_device
    @torch.no_grad()
    def generate_finish(self, pend: "_PendingGeneration") -> GenerateOutput:
        """The decode loop of a :meth:`generate_begin` (current stream; the caller orders it behind the prompt phase)."""
        st, skey, B, Smax, V, out_tokens = pend.st, pend.skey, pend.B, pend.Smax, pend.V, pend.out_tokens
        max_new_tokens, eos, eos_first, pad_token_id = pend.max_new_tokens, pend.eos, pend.eos_first, pend.pad_token_id
        return_logits, all_logits, forced_tokens = pend.return_logits, pend.all_logits, pend.forced_tokens
        use_graph, validate, sync_every = pend.use_graph, pend.validate, pend.sync_every
        beam = getattr(pend, "beam", None)
        self._input_flags = pend.input_flags
        # tensors the prompt phase allocated (possibly on another stream: GenerationPipeline) and this loop reads: the caching
        # allocator must not hand their memory to that stream's next allocation before this stream is done with them
        cur_stream = torch.cuda.current_stream(self.device)
        for t_ in list(all_logits) + [forced_tokens, pend.input_flags]:
            if t_ is not None:
                t_.record_stream(cur_stream)
        graph = None
        if use_graph and max_new_tokens > 1:
            graph, graph_logits = self._decode_graph(st, B, Smax, out_tokens, skey)
        n_done = 1
        finished_at = [None] * B
        if ops.KERNEL_TIMERS is not None:       # bench.py's per-kernel timers: the decode steps' launches are priced separately
            ops.KERNEL_PHASE = "decode:"
        while n_done < max_new_tokens:
            if graph is not None:
                graph.replay()
                lg = graph_logits            # the buffer the captured step writes: copied out stream-ordered below
            else:
                lg = self._decode_step(st, B, Smax, out_tokens)
            if return_logits:
                all_logits.append(lg[:, :V].float().clone())
            n_done += 1
            if forced_tokens is not None and n_done - 1 < forced_tokens.shape[1]:
                st["cur"].copy_(forced_tokens[:, n_done - 1])
            if beam is not None:
                # every prompt done? gar_beam_step latches each prompt's and counts them; without eos ids none is before the last step
                if eos and (n_done % sync_every == 0 or n_done == max_new_tokens):
                    fin = int(st["done_count"].item()) >= pend.prompts
                    if not validate:
                        self._raise_on_input_flags()
                    if fin:
                        break
            elif eos and (n_done % sync_every == 0 or n_done == max_new_tokens):
                # every row done? ONE int off the device (the argmax kernel latches each row's first eos step and counts the
                # latched rows); a list longer than MAX_EOS_IDS keeps the host scan of the token matrix
                fin = int(st["done_count"].item()) >= B if pend.eos_on_device else \
                    self._all_finished(out_tokens, n_done, eos, finished_at)
                if not validate:
                    self._raise_on_input_flags()        # the poll above synchronised already
                if fin:
                    break
        ops.KERNEL_PHASE = ""
        if beam is not None:
            return self._beam_output(pend, torch.stack(all_logits, 1) if return_logits else None)
        seq = out_tokens[:, :n_done].clone()
        if eos:
            if pend.eos_on_device:      # finished[b] = the column of row b's first eos (-1: none within n_done tokens)
                finished_at = [(c + 1 if 0 <= c < n_done else None) for c in st["finished"].tolist()]
            else:
                self._all_finished(out_tokens, n_done, eos, finished_at)
            cut = max((f if f is not None else n_done) for f in finished_at)
            if cut < n_done or any(f is not None and f < cut for f in finished_at):
                pad = pad_token_id if pad_token_id is not None else eos_first      # HF: pad defaults to eos_token_id[0]
                # rows that finished early hold `pad` behind their eos, as HF's loop writes them; the batch ends at the LAST row's eos
                cols = torch.arange(cut, device=self.device)[None, :]
                ends = torch.tensor([(f if f is not None else cut) for f in finished_at], dtype=torch.int64, device=self.device)
                seq = torch.where(cols < ends[:, None], seq[:, :cut], torch.full_like(seq[:, :cut], int(pad)))
        lp_fields = {}
        if st.get("lp") is not None:
            # the planes hold the model's own choice of every step, as `sequences` does; behind a row's first eos — where
            # `sequences` holds `pad` — they hold 0. Masks and sums: a few torch ops on the planes, nothing read back
            raw, warped = (p[:, :seq.shape[1]] for p in st["lp"])
            names = ("token_logprobs", "token_logprobs_warped", "sum_logprobs", "sum_logprobs_warped", "n_tokens")
            lp_fields = dict(zip(names, logprob_outputs(raw, warped, finished_at if eos else [None] * B)))
        if st.get("tk") is not None:
            lp_fields.update(top_logprob_outputs(st["tk"], seq.shape[1], finished_at if eos else [None] * B))
        constraint = getattr(pend, "constraint", None)
        if constraint is not None:
            lp_fields["phrase_index"] = phrase_indices(constraint, seq.tolist(), eos, pend.N)
        return GenerateOutput(sequences=seq, logits=torch.stack(all_logits, 1) if return_logits else None,
                              input_flags=None if validate else self._input_flags, **lp_fields)

    def _beam_output(self, pend, logits) -> GenerateOutput:
        """the output of a beam_search request from the finished set the steps kept: the best num_return_sequences hypotheses of
        every prompt, cropped to the longest and padded behind each one's end (HF: ``pad_token_id``, else the first eos id)"""
        bs, beam, B = pend.st["beam"], pend.beam, pend.prompts
        K, T, n = bs["K"], bs["T"], beam.num_return_sequences
        lens = bs["fin_len"].view(B, K)[:, :n].reshape(-1).to(torch.int64)
        width = int(lens.max().item())
        seq = bs["fin_tokens"].view(B, K, T)[:, :n, :width].reshape(B * n, width).to(torch.int64)
        pad = pend.pad_token_id if pend.pad_token_id is not None else (pend.eos_first or 0)
        seq = torch.where(torch.arange(width, device=self.device)[None, :] < lens[:, None], seq, torch.full_like(seq, int(pad)))
        return GenerateOutput(sequences=seq, logits=logits, input_flags=None if pend.validate else self._input_flags,
                              sequences_scores=bs["fin_scores"].view(B, K)[:, :n].reshape(-1).clone())

    def _raise_on_input_flags(self):
        f = int(self._input_flags.item())
        if f:
            raise ValueError("generate(validate=False): " + describe_input_flags(f))

    @staticmethod
    def _all_finished(out_tokens, n_done, eos, finished_at) -> bool:
        host = out_tokens[:, :n_done].tolist()
        for b, row in enumerate(host):
            if finished_at[b] is None:
                for j, tok in enumerate(row):
                    if tok in eos:
                        finished_at[b] = j + 1
                        break
        return all(f is not None for f in finished_at)

    def _decode_graph(self, st, B, Smax, out_tokens, skey):
        """(graph, logits buffer of the captured step). out_tokens is a [:, :n] slice of the state's [B, Smax] buffer:
        pointer and row stride depend on the state only, so one graph serves every max_new_tokens of the bucket."""
        gkey = (skey, out_tokens.data_ptr(), out_tokens.stride(0), bool(st.get("sampling")), self.kv_cache_dtype,
                st["fan"]["Kp"].data_ptr() if st.get("fan") else 0,         # (the prompt caches live in another state)
                st.get("lp") is not None,                                   # return_logprobs: the step picks with the _lp launch
                (st["tk"]["k"], st["tk"]["C"]) if st.get("tk") else (0, 0),  # top_logprobs / candidates: one more launch, planes by (k, C)
                st.get("proc") is not None,                                 # logits_processing: one more launch in front of the pick
                st.get("row_words") is not None,                            # per-row requests: the step picks with gar_sample_rows
                st.get("row_proc") is not None,                             # per-row processing: gar_logits_process_rows in front of the pick
                bool(st.get("warpers")),                                    # sampling_warpers: the step draws with gar_sample_ext
                st.get("nodes") is not None,                                # constraint: one more launch in front of the pick
                st["beam"]["key"] if st.get("beam") else None)              # beam_search: the step picks with gar_beam_step, buffers by (K, M, T)
        g = self._graphs.get(gkey)
        if g is None:
            # what the warm-up step writes and the loop reads: counters, the current tokens, the stopping-criterion latches
            names = ("counters", "cur", "finished", "done_count")
            saved = {n: st[n].clone() for n in names}
            # beam_search: the warm-up step also moves the beams' scores, histories, finished set and latches. The cache rows it
            # reorders are the ones it has just appended, which the first real step writes again
            beam_saved = {n: st["beam"][n].clone() for n in self._BEAM_LATCHES} if st.get("beam") else {}

            def restore():
                for n in names:
                    st[n].copy_(saved[n])
                for n, v in beam_saved.items():
                    st["beam"][n].copy_(v)
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):                       # warm-up launch outside capture (lazy module load)
                self._decode_step(st, B, Smax, out_tokens)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize(self.device)
            restore()
            # a dropped model is a reference cycle (model <-> mllm facade): its captured graphs and their memory pools go when the
            # cycle collector runs. Inside a capture that is an illegal call and the HIP runtime aborts — and torch.cuda.graph no
            # longer collects before it captures — so the dead cycles go here, and the step itself creates none that hold a graph
            gc.collect()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                logits = self._decode_step(st, B, Smax, out_tokens)
            restore()                                        # capture does not execute; keep state explicit
            g = self._graphs[gkey] = (g, logits)
        return g
