"""``generate(constraint=PhraseConstraint(...))``: an answer taken from a closed set of phrases. The set is checked on the host and
packed into the int32 token trie ``gar_constrain`` walks on the device (include/gar_hip.h). Pure Python: importing it needs neither
torch nor the library.

Semantics are those of HF's ``PrefixConstrainedLogitsProcessor`` (``scores + mask``, mask 0 at the allowed ids and -inf elsewhere)
under the callback "the history stays a prefix of one of the prompt's phrases". As the reference runs
``self.mllm.generate(inputs_embeds=...)`` without ``input_ids``, a row's history is its generated tokens only. With history h:
every token that extends h to a longer prefix of a phrase is allowed; when h is a complete phrase every eos id is allowed as well;
when h is no prefix of any phrase (behind a phrase's eos, or a finished row fed pad) exactly the eos ids are allowed.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

from .logits_processing import _Refused, _is_int

HEADER_WORDS = 4          # gar_constrain: [n_nodes, n_edges, n_rows, 0], then root, first, tok, child and the terminal bits
BLOCK_WORDS = 65536       # int32 words of the trie block a KV state keeps: about 1200 category names of up to 8 tokens
DEAD = -1                 # the node of a history that is no prefix of any phrase


def _phrase_set(phrases, what: str) -> Tuple[Tuple[int, ...], ...]:
    if isinstance(phrases, (str, bytes)) or not hasattr(phrases, "__iter__"):
        raise ValueError(f"{what} has to be a list of token-id lists, but is {phrases!r}")
    out = []
    for p in phrases:
        if isinstance(p, (str, bytes)) or not hasattr(p, "__iter__"):
            raise ValueError(f"{what} has to be a list of token-id lists, but holds {p!r}")
        p = tuple(p)
        if len(p) == 0:
            raise ValueError(f"{what} holds an empty phrase (a phrase has at least one token)")
        for i in p:
            if not _is_int(i):
                raise ValueError(f"{what}: a phrase is a list of integers, but holds {i!r}")
        out.append(tuple(int(i) for i in p))
    if not out:
        raise ValueError(f"{what} is empty (a constraint needs at least one phrase)")
    return tuple(out)


class PhraseConstraint:
    """The closed set of answers of one ``generate()`` request: every returned row is one of its prompt's phrases, followed by eos.

    ``phrases``: a list of token-id lists shared by all prompts, or a list of B such lists — prompt b's own set (each GAR-Bench
    item has its own options). A phrase may be a proper prefix of another; duplicates merge and the first index wins.

    ``generate`` masks every step's logits on the device (one ``gar_constrain`` launch per step, after ``logits_processing``,
    before the pick) and reports ``GenerateOutput.phrase_index``: the index, in the row's prompt's list, of the phrase the row
    completed, or -1. The request needs ``eos_token_id`` — a complete phrase could never end otherwise.

    Capacity: 4 + rows + (nodes + 1) + 2 * edges + ceil(nodes / 32) int32 words have to fit the 65536-word block of a state, where
    nodes and edges count the merged tries of the distinct sets (``GarError`` otherwise, never truncation); ids outside
    [0, vocab) are a ``GarError`` too."""

    def __init__(self, phrases, texts=None):
        if isinstance(phrases, (str, bytes)) or not hasattr(phrases, "__iter__"):
            raise ValueError(f"phrases has to be a list of token-id lists (or one such list per prompt), but is {phrases!r}")
        phrases = list(phrases)
        if not phrases:
            raise ValueError("phrases is empty (a constraint needs at least one phrase)")

        def listy(x):
            return hasattr(x, "__iter__") and not isinstance(x, (str, bytes))
        # one set per prompt when the entries are lists of lists; the first non-empty entry decides (an empty one is refused below,
        # as an empty phrase or an empty set)
        phrases = [list(p) if listy(p) else p for p in phrases]
        probe = next((p for p in phrases if listy(p) and p), None)
        self.per_prompt = probe is not None and listy(probe[0])
        if self.per_prompt:
            self.sets = tuple(_phrase_set(s, f"phrases[{b}]") for b, s in enumerate(phrases))
        else:
            self.sets = (_phrase_set(phrases, "phrases"),)
        self.texts = texts      # from_text: the strings, laid out like ``phrases`` (callers print the chosen one)

    def __repr__(self):
        return f"PhraseConstraint({[list(map(list, s)) for s in self.sets] if self.per_prompt else list(map(list, self.sets[0]))!r})"

    @classmethod
    def from_text(cls, tokenizer, strings) -> "PhraseConstraint":
        """the phrases of ``strings`` — a list of strings shared by all prompts, or a list of such lists, one per prompt — encoded
        without special tokens"""
        def enc(s):
            if not isinstance(s, str):
                raise ValueError(f"from_text: a phrase is a string, but is {s!r}")
            # the call form: what HF tokenizers, the processor's adapter and the stub tokenizer share
            return [int(i) for i in tokenizer([s], add_special_tokens=False)["input_ids"][0]]
        strings = list(strings)
        if strings and all(isinstance(s, str) for s in strings):
            return cls([enc(s) for s in strings], texts=list(strings))
        return cls([[enc(s) for s in group] for group in strings], texts=[list(g) for g in strings])

    @classmethod
    def coerce(cls, value) -> Optional["PhraseConstraint"]:
        """``generate(constraint=value)``: None, a PhraseConstraint, or a dict with the key ``phrases``"""
        if value is None or isinstance(value, cls):
            return value
        if isinstance(value, dict):
            unknown = sorted(set(value) - {"phrases"})
            if unknown or "phrases" not in value:
                raise TypeError(f"constraint: a dict with the key 'phrases' (unknown keys {unknown})")
            return cls(value["phrases"])
        raise TypeError(f"constraint: a PhraseConstraint, a dict or None, not {type(value).__name__}")

    def set_of(self, b: int) -> Tuple[Tuple[int, ...], ...]:
        """prompt b's phrases"""
        return self.sets[b] if self.per_prompt else self.sets[0]

    def text_of(self, b: int, index: int) -> Optional[str]:
        """the string of prompt b's phrase ``index`` of a constraint made by :meth:`from_text` (None otherwise, or for index -1)"""
        if self.texts is None or index < 0:
            return None
        return (self.texts[b] if self.per_prompt else self.texts)[index]

    def pack(self, vocab_size: int, batch: int, fanout: int = 1) -> List[int]:
        """the int32 words of gar_constrain's trie block for a model of ``vocab_size`` and ``batch`` prompts of ``fanout`` rows
        each (``num_return_sequences``: row b * fanout + i walks prompt b's trie). Equal sets share one trie. Raises ``ValueError``
        for a per-prompt list whose length is not ``batch`` and :class:`_Refused` (the caller's GarError) for an id outside
        [0, vocab_size) and for a block above the capacity."""
        V, B, N = int(vocab_size), int(batch), int(fanout)
        if self.per_prompt and len(self.sets) != B:
            raise ValueError(f"constraint: {len(self.sets)} per-prompt phrase sets for a batch of {B} prompts")
        first, tok, child, term, roots = [0], [], [], [], {}
        for s in dict.fromkeys(self.sets):
            for p in s:
                for i in p:
                    if not 0 <= i < V:
                        raise _Refused(f"constraint: token id {i} is outside [0, vocab_size = {V})")
            # breadth first: node = a distinct prefix, its edges ascending by token
            kids: Dict[Tuple[int, ...], set] = {(): set()}
            ends = set(s)
            for p in s:
                for j in range(len(p)):
                    kids.setdefault(p[:j], set()).add(p[j])
                    kids.setdefault(p[:j + 1], set())
            base = len(term)
            order, index = [()], {(): base}
            for prefix in order:            # grows while it is walked
                for t in sorted(kids[prefix]):
                    index[prefix + (t,)] = base + len(order)
                    order.append(prefix + (t,))
            roots[s] = base
            for prefix in order:
                for t in sorted(kids[prefix]):
                    tok.append(t)
                    child.append(index[prefix + (t,)])
                first.append(len(tok))
                term.append(prefix in ends)
        n_nodes, n_edges = len(term), len(tok)
        bits = [0] * ((n_nodes + 31) // 32)
        for i, on in enumerate(term):
            if on:
                bits[i >> 5] |= 1 << (i & 31)
        bits = [w - (1 << 32) if w >= 1 << 31 else w for w in bits]        # as int32
        root = [roots[self.set_of(b)] for b in range(B) for _ in range(N)]
        words = [n_nodes, n_edges, len(root), 0] + root + first + tok + child + bits
        if len(words) > BLOCK_WORDS:
            raise _Refused(f"constraint: a trie of {n_nodes} nodes and {n_edges} edges for {len(root)} rows takes {len(words)} words "
                           f"(4 + rows + nodes + 1 + 2 * edges + nodes / 32), the device block holds {BLOCK_WORDS}")
        return words

    def phrase_index(self, b: int, tokens: Sequence[int], eos_ids: Sequence[int] = ()) -> int:
        """the index in prompt b's list of the phrase ``tokens`` completed — its tokens before its first eos, or all of them when
        none occurs (``max_new_tokens`` cut it), form exactly one phrase — else -1. Duplicates: the first index."""
        eos = set(int(e) for e in eos_ids)
        head = []
        for t in tokens:
            if int(t) in eos:
                break
            head.append(int(t))
        head = tuple(head)
        for i, p in enumerate(self.set_of(b)):
            if p == head:
                return i
        return -1
