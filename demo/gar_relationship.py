#!/usr/bin/env python
"""Multi-region relationship question on the MI355X path — CLI counterpart of the reference's demo/gar_relationship.py
(--image_path, --mask_paths ..., --question_str with <PromptK> tokens)."""
import numpy as np
from PIL import Image

from _common import (base_parser, beam_search_kwargs, constraint_kwargs, generation_config, load, logits_processing_kwargs,
                     print_choices, print_hypotheses, sampling_kwargs, top_logprob_lines)


def main():
    ap = base_parser("Multi-region inference demo of Grasp Any Region models (MI355X-native path).")
    ap.add_argument("--image_path", required=True)
    ap.add_argument("--mask_paths", nargs="+", required=True)
    ap.add_argument("--question_str", required=True)
    ap.add_argument("--return_logprobs", action="store_true",
                    help="with --choices: print the chosen phrase's probability among the choices in front of it")
    args = ap.parse_args()
    model, processor, dtype = load(args)
    from evaluation.eval_dataset import MultiRegionDataset
    img = Image.open(args.image_path)
    masks = [np.array(Image.open(p).convert("L")).astype(bool) for p in args.mask_paths]
    prompt_number = model.config.prompt_numbers
    prompt_tokens = [f"<Prompt{i}>" for i in range(prompt_number)] + ["<NO_Prompt>"]
    question = args.question_str + "\nAnswer with the correct option's letter directly."
    dataset = MultiRegionDataset(image=img, masks=masks, question_str=question, processor=processor,
                                 prompt_number=prompt_number, visual_prompt_tokens=prompt_tokens, data_dtype=dtype,
                                 device=args.device)
    data_sample = dataset[0]
    gc = generation_config(args, processor)
    choices = constraint_kwargs(args, processor)
    out = model.generate(**data_sample, generation_config=gc, return_dict=True, top_logprobs=args.top_logprobs,
                         return_logprobs=bool(choices) and args.return_logprobs, **sampling_kwargs(args, gc),
                         **logits_processing_kwargs(args), **beam_search_kwargs(args), **choices)
    if choices:                             # --choices: the phrase each row completed
        print_choices(out, choices["constraint"], args.return_logprobs)
        return
    if out.sequences_scores is not None:    # --num_beams: the hypotheses, best first
        print_hypotheses(out, processor.tokenizer)
        return
    for r, seq in enumerate(out.sequences):     # one answer, or the --num_return_sequences sampled ones
        print(processor.tokenizer.decode(seq, skip_special_tokens=True).strip())
        if args.top_logprobs:
            print("\n".join(top_logprob_lines(out, r, processor.tokenizer)))


if __name__ == "__main__":
    main()
