#!/usr/bin/env python
"""Region captioning from an image + a binary mask on the MI355X path — CLI counterpart of the reference's
demo/gar_with_mask.py (same flags: --model_name_or_path --image_path --mask_path --data_type --seed)."""
import numpy as np
from PIL import Image

from _common import (base_parser, beam_search_kwargs, constraint_kwargs, generation_config, load, logits_processing_kwargs,
                     print_choices, print_hypotheses, sampling_kwargs, top_logprob_lines)


def main():
    ap = base_parser("Inference demo of Grasp Any Region models (MI355X-native path).")
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--mask_path", required=True)
    ap.add_argument("--return_logprobs", action="store_true",
                    help="print each caption's mean token log-probability; with --num_return_sequences N the captions come "
                         "ordered by it, best first")
    args = ap.parse_args()
    model, processor, dtype = load(args)
    from evaluation.eval_dataset import SingleRegionCaptionDataset
    img = Image.open(args.image_path)
    mask = np.array(Image.open(args.mask_path).convert("L")).astype(bool)
    prompt_number = model.config.prompt_numbers
    prompt_tokens = [f"<Prompt{i}>" for i in range(prompt_number)] + ["<NO_Prompt>"]
    dataset = SingleRegionCaptionDataset(image=img, mask=mask, processor=processor, prompt_number=prompt_number,
                                         visual_prompt_tokens=prompt_tokens, data_dtype=dtype, device=args.device)
    data_sample = dataset[0]
    gc = generation_config(args, processor)
    choices = constraint_kwargs(args, processor)
    out = model.generate(**data_sample, generation_config=gc, return_dict=True, return_logprobs=args.return_logprobs,
                         top_logprobs=args.top_logprobs, **sampling_kwargs(args, gc), **logits_processing_kwargs(args),
                         **beam_search_kwargs(args), **choices)
    if choices:                             # --choices: the phrase each row completed
        print_choices(out, choices["constraint"], args.return_logprobs)
        return
    if out.sequences_scores is not None:    # --num_beams: the hypotheses, best first
        print_hypotheses(out, processor.tokenizer)
        return
    if args.return_logprobs:                # the model's own confidence in each caption: mean log-probability of its tokens
        mean = (out.sum_logprobs / out.n_tokens.clamp(min=1)).tolist()
        for r in sorted(range(len(mean)), key=lambda i: -mean[i]):
            print(f"[{mean[r]:.4f}] " + processor.tokenizer.decode(out.sequences[r], skip_special_tokens=True).strip())
            if args.top_logprobs:
                print("\n".join(top_logprob_lines(out, r, processor.tokenizer)))
        return
    for r, seq in enumerate(out.sequences):     # one caption, or the --num_return_sequences sampled ones
        print(processor.tokenizer.decode(seq, skip_special_tokens=True).strip())
        if args.top_logprobs:
            print("\n".join(top_logprob_lines(out, r, processor.tokenizer)))


if __name__ == "__main__":
    main()
