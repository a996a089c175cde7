"""generate(constraint=PhraseConstraint(...)) restated in plain Python / torch on (phrase set, row history, logits row): the trie
walk, then HF's PrefixConstrainedLogitsProcessor arithmetic ``scores + mask``. The expected value of the host tests (against
transformers' own class, tests/golden/constraint.npz) and of the kernel tests (gar_constrain, bit for bit); also a reader of the
packed trie block, independent of the packer. Semantics: DESIGN 7.13. Not the product: gar_amd never imports this."""
import torch

DEAD = -1
HEADER = 4


def allowed_ids(phrases, history, V: int, eos_ids=()) -> set:
    """ids whose score survives at step t = len(history): every token that extends the history to a longer prefix of a phrase;
    the eos ids as well when the history is a complete phrase; exactly the eos ids when it is no prefix of any phrase"""
    h = [int(x) for x in history]
    t = len(h)
    eos = {int(e) for e in eos_ids if 0 <= int(e) < V}
    ps = [[int(i) for i in p] for p in phrases]
    prefix_of = [p for p in ps if len(p) >= t and p[:t] == h]
    if not prefix_of:
        return eos
    out = {p[t] for p in prefix_of if len(p) > t}
    if any(len(p) == t for p in prefix_of):
        out |= eos
    return {i for i in out if 0 <= i < V}


def mask_row(phrases, history, row: torch.Tensor, V: int, eos_ids=()) -> torch.Tensor:
    """HF: ``scores + mask``, mask = -inf with 0 at the allowed ids, over columns 0 .. V - 1 of one row (any float dtype; columns
    V.. untouched)"""
    mask = torch.full((V,), float("-inf"), dtype=row.dtype)
    ok = sorted(allowed_ids(phrases, history, V, eos_ids))
    if ok:
        mask[torch.tensor(ok, dtype=torch.int64)] = 0
    out = row.clone()
    out[:V] = row[:V] + mask
    return out


def mask(sets, histories, logits: torch.Tensor, V: int, eos_ids=()) -> torch.Tensor:
    """rows of ``logits`` [B, ld] with their phrase sets (``sets[b]``) and histories (a list of B id lists)"""
    return torch.stack([mask_row(sets[b], h, logits[b], V, eos_ids) for b, h in enumerate(histories)])


def first_argmax(row: torch.Tensor) -> int:
    """greedy pick with the first-index tie rule of gar_argmax"""
    x = row.to(torch.float32)
    return int((x == x.max()).nonzero()[0, 0])


def phrase_index(phrases, tokens, eos_ids=()) -> int:
    """index of the phrase the tokens before the first eos (all of them without one) are, first index for duplicates; else -1"""
    eos = {int(e) for e in eos_ids}
    head = []
    for t in tokens:
        if int(t) in eos:
            break
        head.append(int(t))
    for i, p in enumerate(phrases):
        if [int(x) for x in p] == head:
            return i
    return -1


# ---- the packed block (include/gar_hip.h, gar_constrain), read without the packer -----------------------------------------------
def block_arrays(words):
    """(n_nodes, n_edges, root, first, tok, child, terminal flags) of a trie block"""
    w = [int(x) for x in words]
    n_nodes, n_edges, n_rows = w[0], w[1], w[2]
    o = HEADER
    root = w[o:o + n_rows]
    o += n_rows
    first = w[o:o + n_nodes + 1]
    o += n_nodes + 1
    tok = w[o:o + n_edges]
    o += n_edges
    child = w[o:o + n_edges]
    o += n_edges
    bits = w[o:o + (n_nodes + 31) // 32]
    assert o + len(bits) == len(w), "words behind the block"
    term = [bool((bits[i >> 5] >> (i & 31)) & 1) for i in range(n_nodes)]
    return n_nodes, n_edges, root, first, tok, child, term


def unpack(words):
    """per row, the set of phrases its root spells: every root-to-terminal path of the block"""
    n_nodes, n_edges, root, first, tok, child, term = block_arrays(words)
    for i in range(n_nodes):
        edge = tok[first[i]:first[i + 1]]
        assert edge == sorted(set(edge)), "a node's tokens ascend strictly"
    out = []
    for r in root:
        found, stack = set(), [(r, ())]
        while stack:
            node, path = stack.pop()
            if term[node] and path:
                found.add(path)
            for e in range(first[node], first[node + 1]):
                stack.append((child[e], path + (tok[e],)))
        out.append(found)
    return out


def walk(words, row: int, history, V: int) -> int:
    """the node of ``row`` behind ``history`` (DEAD when it is no prefix of any phrase, or holds an id outside [0, V))"""
    n_nodes, n_edges, root, first, tok, child, term = block_arrays(words)
    node = root[row]
    for t in history:
        t = int(t)
        if node == DEAD or not 0 <= t < V:
            return DEAD
        nxt = DEAD
        for e in range(first[node], first[node + 1]):
            if tok[e] == t:
                nxt = child[e]
        node = nxt
    return node
