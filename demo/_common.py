"""Shared by the demo CLIs: model / processor construction with the reference's flags plus --device,
--max_num_tiles and --synthetic_weights (no checkpoint is reachable offline)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "grasp-any-region_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gar_amd.bench_loops import DATA_TYPE_CHOICES, TORCH_DTYPE_MAP, resolve_data_type  # noqa: E402,F401


def base_parser(description):
    ap = argparse.ArgumentParser(description=description)
    ap.add_argument("--model_name_or_path", default="HaochenWang/GAR-1B",
                    help="checkpoint directory (config.json + *.safetensors [+ tokenizer]); with --synthetic_weights a "
                         "size name: gar_1b | gar_8b | tiny")
    ap.add_argument("--data_type", choices=DATA_TYPE_CHOICES, default="bf16",
                    help="bf16 | fp16 | fp32 (parity mode)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max_num_tiles", type=int, default=16)
    ap.add_argument("--max_new_tokens", type=int, default=1024)
    ap.add_argument("--host_preprocessing", action="store_true",
                    help="resize / tile / normalise on the CPU (torch bicubic) instead of the device kernels")
    ap.add_argument("--kv_cache_dtype", choices=("auto", "fp8"), default="auto",
                    help="decode KV cache: auto = the model dtype; fp8 = OCP e4m3 with one scale per vector (16-bit models only)")
    ap.add_argument("--decode_weight_dtype", choices=("auto", "fp8"), default="auto",
                    help="weights of the decode GEMVs: auto = the model dtype; fp8 = OCP e4m3 copies with one scale per output row "
                         "(16-bit models, decode batches <= 64 rows; the prompt phase keeps 16-bit weights)")
    ap.add_argument("--num_return_sequences", type=int, default=1,
                    help="N > 1: N sampled captions of the region from ONE prompt phase (implies sampling; --seed keys the draws)")
    ap.add_argument("--num_beams", type=int, default=1, metavar="K",
                    help="K > 1: beam search with K beams over one prompt phase; --num_return_sequences N <= K then prints the N "
                         "best hypotheses with their scores (not combined with the sampling flags)")
    ap.add_argument("--length_penalty", type=float, default=1.0,
                    help="beam search: a hypothesis of n tokens scores sum of log-probabilities / n ** length_penalty")
    ap.add_argument("--early_stopping", choices=("false", "true", "never"), default="false",
                    help="beam search: HF's early_stopping (false: its default heuristic, true: stop at K hypotheses, never: "
                         "the canonical criterion)")
    ap.add_argument("--temperature", type=float, default=None, help="sampling temperature (implies sampling)")
    ap.add_argument("--top_p", type=float, default=None, help="nucleus sampling (implies sampling)")
    ap.add_argument("--top_k", type=int, default=None, help="top-k sampling (implies sampling)")
    ap.add_argument("--min_p", type=float, default=None,
                    help="drop tokens less likely than min_p x the most likely one (implies sampling)")
    ap.add_argument("--typical_p", type=float, default=None, help="locally typical sampling mass (implies sampling)")
    ap.add_argument("--epsilon_cutoff", type=float, default=None, help="drop tokens of probability < epsilon (implies sampling)")
    ap.add_argument("--eta_cutoff", type=float, default=None, help="entropy-dependent probability cutoff (implies sampling)")
    ap.add_argument("--top_logprobs", type=int, default=0, metavar="K",
                    help="print, under each output and per generated token, the K most likely tokens as decoded-token:probability "
                         "(raw softmax of the step's logits, also when sampling; K <= 32)")
    ap.add_argument("--repetition_penalty", type=float, default=1.0,
                    help="HF's repetition penalty over the tokens generated so far (1.0 = off; e.g. 1.2 against a looping caption)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, metavar="N",
                    help="no N-gram of the generated tokens occurs twice (0 = off)")
    ap.add_argument("--choices", default=None, metavar="A,B,...",
                    help="comma-separated phrases: the answer is constrained to one of them (a token trie walked on the device, "
                         "one mask launch per step) and printed as that phrase; with --return_logprobs behind its probability "
                         "among the choices. Not combined with --num_beams")
    ap.add_argument("--synthetic_weights", action="store_true",
                    help="seeded random weights of the named size + the stub tokenizer (plumbing / benchmarking)")
    return ap


def load(args):
    from gar_amd import GARConfig
    from gar_amd.modeling_gar import GARModel
    from gar_amd.processing import GARProcessor
    dtype = resolve_data_type(args.data_type)
    kv = None if getattr(args, "kv_cache_dtype", "auto") == "auto" else args.kv_cache_dtype
    dw = None if getattr(args, "decode_weight_dtype", "auto") == "auto" else args.decode_weight_dtype
    torch.manual_seed(args.seed)
    if args.synthetic_weights:
        name = args.model_name_or_path if args.model_name_or_path in ("gar_1b", "gar_8b", "tiny") else "gar_1b"
        cfg = getattr(GARConfig, name)()
        model = GARModel.from_synthetic(cfg, args.seed, dtype, args.device, kv_cache_dtype=kv, decode_weight_dtype=dw)
        processor = GARProcessor.from_config(cfg, max_num_tiles=args.max_num_tiles)
    else:
        model = GARModel.from_pretrained(args.model_name_or_path, dtype, args.device, kv_cache_dtype=kv, decode_weight_dtype=dw)
        processor = GARProcessor.from_pretrained(args.model_name_or_path, model.config, args.max_num_tiles)
    if not args.host_preprocessing:
        processor.use_gpu_preprocessing(args.device, dtype)
    return model.eval(), processor, dtype


def generation_config(args, processor):
    # transformers.GenerationConfig(max_new_tokens, do_sample=False, eos, pad) of the reference, as a plain dict
    gc = dict(max_new_tokens=args.max_new_tokens, do_sample=False, eos_token_id=processor.tokenizer.eos_token_id,
              pad_token_id=processor.tokenizer.pad_token_id)
    knobs = {k: getattr(args, k, None) for k in ("temperature", "top_p", "top_k")}
    n = getattr(args, "num_return_sequences", 1)
    if getattr(args, "num_beams", 1) > 1:       # beam search: --num_return_sequences goes to beam_search_kwargs
        n = 1
    # the reference CLI is greedy: sampling only when asked for
    if n != 1 or any(v is not None for v in knobs.values()) or any(v is not None for v in _warper_args(args).values()):
        gc.update(do_sample=True, num_return_sequences=n, **{k: v for k, v in knobs.items() if v is not None})
    return gc


WARPER_ARGS = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def _warper_args(args):
    return {k: getattr(args, k, None) for k in WARPER_ARGS}


def sampling_kwargs(args, gc):
    """generate() keywords that go with :func:`generation_config`: the request's Philox key when it samples, and the
    sampling_warpers parameter when one of --min_p / --typical_p / --epsilon_cutoff / --eta_cutoff acts"""
    if not gc.get("do_sample"):
        return {}
    from gar_amd import SamplingWarpers
    sw = SamplingWarpers(**_warper_args(args))
    return dict(seed=args.seed) if sw.neutral else dict(seed=args.seed, sampling_warpers=sw)


def beam_search_kwargs(args):
    """generate() keywords of --num_beams / --length_penalty / --early_stopping: the beam_search parameter when K > 1"""
    if getattr(args, "num_beams", 1) <= 1:
        return {}
    from gar_amd import BeamSearch
    return dict(beam_search=BeamSearch(args.num_beams, length_penalty=args.length_penalty,
                                       early_stopping={"false": False, "true": True, "never": "never"}[args.early_stopping],
                                       num_return_sequences=getattr(args, "num_return_sequences", 1)))


def print_hypotheses(out, tokenizer):
    """beam search: one line per returned hypothesis, best first; with several, each behind its score"""
    many = len(out.sequences) > 1
    for seq, score in zip(out.sequences, out.sequences_scores.tolist()):
        text = tokenizer.decode(seq, skip_special_tokens=True).strip()
        print(f"[{score:.4f}] {text}" if many else text)


def logits_processing_kwargs(args):
    """generate() keywords of --repetition_penalty / --no_repeat_ngram_size: the logits_processing parameter when either acts"""
    from gar_amd import LogitsProcessing
    lp = LogitsProcessing(repetition_penalty=getattr(args, "repetition_penalty", 1.0),
                          no_repeat_ngram_size=getattr(args, "no_repeat_ngram_size", 0))
    return {} if lp.neutral else dict(logits_processing=lp)


def top_logprob_lines(out, row, tokenizer):
    """--top_logprobs: one line per generated token of ``out.sequences[row]`` — the K alternatives of that step as
    decoded-token:probability, best first. Stops at the row's first eos (ids -1 behind it)."""
    lines = []
    for ids, lps in zip(out.top_logprob_ids[row].tolist(), out.top_logprobs[row].exp().tolist()):
        if ids[0] < 0:
            break
        lines.append("    " + "  ".join(f"{tokenizer.decode([i])!r}:{p:.4f}" for i, p in zip(ids, lps)))
    return lines


def constraint_kwargs(args, processor):
    """generate() keywords of --choices: the constraint parameter over the comma-separated phrases"""
    if not getattr(args, "choices", None):
        return {}
    from gar_amd import PhraseConstraint
    texts = [c.strip() for c in args.choices.split(",") if c.strip()]
    return dict(constraint=PhraseConstraint.from_text(processor.tokenizer, texts))


def print_choices(out, constraint, return_logprobs=False):
    """--choices: one line per row — the phrase the row completed (or a note that max_new_tokens cut it); with log-probabilities
    behind its probability, exp(sum_logprobs): the phrase's probability renormalised over the allowed set at every step"""
    for r, i in enumerate(out.phrase_index.tolist()):
        text = constraint.text_of(0, i) if i >= 0 else "(no choice completed within max_new_tokens)"
        print(f"[{float(out.sum_logprobs[r].exp()):.4f}] {text}" if return_logprobs else text)
