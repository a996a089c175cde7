"""Torch CPU, f32 restatement of transformers' ``GenerationMixin._beam_search`` (do_sample=False) as ``gar_beam_step`` implements
it (include/gar_hip.h): ``beam_step_ref`` is one step on an explicit state, ``beam_search_ref`` the driver over a
``logits_fn(histories)``. The arithmetic is HF's own, operation by operation (``_get_top_k_continuations``,
``_get_running_beams_for_next_iteration``, ``_update_finished_beams``, ``_check_early_stop_heuristic``,
``_beam_search_has_unfinished_sequences``); the one thing added is an order for equal scores, which ``torch.topk`` leaves open:
(score descending, beam ascending, token ascending) among candidates, position ascending elsewhere.

tests/test_beam_search_host.py checks it against goldens recorded from transformers (tools/capture_beam_goldens.py) and against
the live functions; tests/test_gpu_beam.py checks the kernel against it bit for bit."""
import torch

NEG = -1.0e9
LIVE = -1.0e8           # scores above this carry no -1e9 sentinel


def new_state(B, K, T):
    run = torch.full((B, K), NEG, dtype=torch.float32)
    run[:, 0] = 0.0
    return dict(run_scores=run, cur_tokens=torch.zeros(B, K, dtype=torch.int64), parent=torch.zeros(B, K, dtype=torch.int32),
                hist=torch.zeros(B, K, T, dtype=torch.int32), fin_tokens=torch.zeros(B, K, T, dtype=torch.int32),
                fin_scores=torch.full((B, K), NEG, dtype=torch.float32), fin_len=torch.zeros(B, K, dtype=torch.int32),
                fin_flag=torch.zeros(B, K, dtype=torch.int32), heur=torch.ones(B, dtype=torch.int32),
                done=torch.zeros(B, dtype=torch.int32), done_count=0, min_margin=float("inf"), tied_candidates=0)


def _desc(x):
    """indices of x in (value descending, position ascending) order"""
    return torch.sort(x, descending=True, stable=True)[1]


def _gaps(sorted_live):
    return float((sorted_live[:-1] - sorted_live[1:]).min()) if sorted_live.numel() > 1 else float("inf")


def beam_step_ref(st, top_ids, top_lp, t, max_new_tokens, early_stopping, length_penalty, eos_ids, V):
    """One step t of every prompt that is not done, in place on ``st`` (:func:`new_state`). ``top_ids`` int [B, K, M] /
    ``top_lp`` f32 [B, K, M]: each running beam's M best raw log-probabilities (value descending, index ascending).
    Also keeps ``st["min_margin"]``: the least gap between neighbours in any order this step decided among live scores (the M + 1
    best candidates, the merged finished scores, the heuristic's comparison), and ``st["tied_candidates"]``: live candidate
    scores of one prompt that were equal."""
    B, K, M = top_ids.shape
    eos = torch.tensor(sorted(int(e) for e in eos_ids), dtype=torch.int64)
    first_k = torch.arange(M) < K
    for b in range(B):
        if st["done"][b]:
            continue
        ids = top_ids[b].to(torch.int64).clamp(0, V - 1).reshape(-1)
        beams = torch.arange(K).repeat_interleave(M)
        # log_probs + running_beam_scores[:, :, None]
        cand = (top_lp[b].to(torch.float32) + st["run_scores"][b][:, None]).reshape(-1)
        by_key = torch.sort(beams * V + ids, stable=True)[1]                 # (beam, token) ascending ...
        order = by_key[_desc(cand[by_key])]                                  # ... kept among equal scores
        live = cand[order][cand[order] > LIVE]
        st["tied_candidates"] += int(live.numel() - torch.unique(live).numel())
        st["min_margin"] = min(st["min_margin"], _gaps(live[:M + 1]))
        top = order[:M]
        s, tok, beam = cand[top], ids[top], beams[top]
        st.setdefault("last_tokens", {})[b] = tok.clone()                    # the step's M candidate tokens, best first (tests)
        hits = torch.isin(tok, eos) | (t >= max_new_tokens - 1)
        # _get_running_beams_for_next_iteration
        run = s + hits.to(torch.float32) * -1.0e9
        sel = _desc(run)[:K]
        # _update_finished_beams
        did = hits & first_k
        f = s / ((t + 1) ** length_penalty)
        full = bool(st["fin_flag"][b].all()) and (early_stopping is True)
        f = f + torch.tensor(full).to(torch.float32) * -1.0e9
        f = f + torch.tensor(not bool(st["heur"][b])).to(torch.float32) * -1.0e9
        f = f + (~did) * -1.0e9
        merged = torch.cat((st["fin_scores"][b], f))
        msel = _desc(merged)[:K]
        mlive = merged[_desc(merged)]
        st["min_margin"] = min(st["min_margin"], _gaps(mlive[mlive > LIVE]))
        cand_seq = st["hist"][b][beam].clone()                               # [M, T]
        cand_seq[:, t] = tok.to(torch.int32)
        merged_seq = torch.cat((st["fin_tokens"][b], cand_seq))
        merged_len = torch.cat((st["fin_len"][b], torch.full((M,), t + 1, dtype=torch.int32)))
        merged_flag = torch.cat((st["fin_flag"][b], did.to(torch.int32)))
        st["fin_tokens"][b] = merged_seq[msel]
        st["fin_scores"][b] = merged[msel]
        st["fin_len"][b] = merged_len[msel]
        st["fin_flag"][b] = merged_flag[msel]
        st["hist"][b] = cand_seq[sel]
        st["run_scores"][b] = run[sel]
        st["parent"][b] = beam[sel].to(torch.int32)
        st["cur_tokens"][b] = tok[sel]
        # _check_early_stop_heuristic at cur_len + 1
        if early_stopping == "never" and length_penalty > 0.0:
            best_len = max_new_tokens
        else:
            best_len = t + 1
        best = st["run_scores"][b][:1] / (best_len ** length_penalty)
        flag = st["fin_flag"][b].bool()
        worst = torch.where(flag, st["fin_scores"][b].min(), torch.tensor(-1.0e9))
        if bool(flag.any()) and float(best) > LIVE:
            st["min_margin"] = min(st["min_margin"], abs(float(best) - float(st["fin_scores"][b].min())))
        heur = bool(st["heur"][b]) and bool((best > worst).any())
        st["heur"][b] = int(heur)
        # _beam_search_has_unfinished_sequences, per prompt
        if (not heur) or (bool(flag.all()) and early_stopping is True) or t >= max_new_tokens - 1:
            st["done"][b] = 1
            st["done_count"] += 1
    return st


def top_m(logits, M):
    """gar_topk_lp's planes: (ids, lp) of the M largest log-probabilities of every row, (value descending, index ascending)"""
    lp = torch.log_softmax(logits.to(torch.float32), dim=-1)
    v, i = torch.sort(lp, dim=-1, descending=True, stable=True)
    return i[..., :M], v[..., :M]


def beam_search_ref(logits_fn, B, K, max_new_tokens, early_stopping=False, length_penalty=1.0, eos_ids=(), V=None,
                    num_return_sequences=1, pad_token_id=None, planes_fn=None):
    """The driver. ``logits_fn(hist, t)`` -> f32 [B, K, V]: the next-token logits of every running beam, ``hist`` int32 [B, K, t]
    its generated tokens so far (t = 0: the prompt's logits, K times). ``planes_fn(hist, t)`` -> (ids, lp) [B, K, M] replaces it
    where the caller has the top-M planes already. Returns (sequences int64 [B * n, len], sequences_scores f32 [B * n], state):
    each prompt's hypotheses best first, padded behind each one's end with ``pad_token_id`` (HF: eos_ids[0] when None or 0)."""
    M = max(2, 1 + len(eos_ids)) * K
    st = new_state(B, K, max_new_tokens)
    for t in range(max_new_tokens):
        hist = st["hist"][:, :, :t]
        if planes_fn is not None:
            ids, lp = planes_fn(hist, t)
        else:
            lg = logits_fn(hist, t)
            V = V or lg.shape[-1]
            ids, lp = top_m(lg, M)
        beam_step_ref(st, ids, lp, t, max_new_tokens, early_stopping, length_penalty, eos_ids, V)
        if int(st["done"].sum()) == B:
            break
    return (*finished_output(st["fin_tokens"], st["fin_scores"], st["fin_len"], num_return_sequences, pad_token_id, eos_ids), st)


def finished_output(fin_tokens, fin_scores, fin_len, n, pad_token_id, eos_ids):
    B, K, T = fin_tokens.shape
    pad = pad_token_id or (eos_ids[0] if len(eos_ids) else 0)
    lens = fin_len[:, :n].reshape(-1).to(torch.int64)
    width = int(lens.max())
    seq = fin_tokens[:, :n, :width].reshape(B * n, width).to(torch.int64)
    seq = torch.where(torch.arange(width)[None, :] < lens[:, None], seq, torch.full_like(seq, int(pad)))
    return seq, fin_scores[:, :n].reshape(-1).clone()
