// Phrase-constrained decoding (gar_constrain, GARModel.generate(constraint=PhraseConstraint(...))): HF's
// PrefixConstrainedLogitsProcessor — scores + mask, mask 0 at the allowed ids and -inf elsewhere — for the callback "the row's
// generated tokens stay a prefix of one of its prompt's phrases", with the phrases on the device as a token trie.
//
// One 1024-thread workgroup per row, one launch per step, in gar_logits_process's frame (llm.hip):
//   walk    nodes[b][t] from nodes[b][t - 1] and out_tokens[b][t - 1] by a binary search among the node's children (their tokens
//           ascend): O(log children) loads, the same in every thread, one store by thread 0. A relaunch of step t rewrites the same
//           value, so the warm-up launch and the capture of the decode graph need nothing saved.
//   mark    one bitmap over the vocabulary in LDS (4 bytes per 32 ids, 32 KB at V = 262144): the node's children, and the eos ids
//           when the node is terminal or DEAD, by LDS atomic OR.
//   sweep   the row in 16-byte pieces: a piece without an allowed id is stored as -inf and never loaded, a piece with only allowed
//           ids is neither loaded nor stored, a mixed piece is loaded, selected on its raw bits and stored. Allowed entries and
//           the columns V..ld-1 keep their bytes.
// Every index is checked before it is used: the header against trie_words, a node against n_nodes, an edge range against n_edges,
// a token id against V, t against out_cols. What fails a check names DEAD and is never followed.
#include "common.h"

#define CN_THREADS 1024
#define CN_HEADER 4                 // trie: [n_nodes, n_edges, n_rows, 0] root[n_rows] first[n_nodes + 1] tok[n_edges] child[n_edges] term bits
#define CN_DEAD (-1)

template <typename T> struct CnBits;
template <> struct CnBits<float> {
    static constexpr unsigned int NEG_INF = 0xFF800000u;
};
template <> struct CnBits<bf16_t> {
#if GAR_HALF_F16
    static constexpr unsigned int NEG_INF = 0xFC00u;
#else
    static constexpr unsigned int NEG_INF = 0xFF80u;
#endif
};

// the 16-byte piece `v` (E elements of T, element j allowed when bit j of `m` is set) with -inf at the other elements
template <typename T>
__device__ __forceinline__ u32x4 cn_select(u32x4 v, unsigned int m) {
    constexpr unsigned int NI = CnBits<T>::NEG_INF;
    if (sizeof(T) == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!((m >> j) & 1u)) v[j] = NI;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!((m >> (2 * j)) & 1u)) v[j] = (v[j] & 0xffff0000u) | NI;
            if (!((m >> (2 * j + 1)) & 1u)) v[j] = (v[j] & 0x0000ffffu) | (NI << 16);
        }
    }
    return v;
}

template <typename T>
__global__ __launch_bounds__(CN_THREADS) void constrain_kernel(T* __restrict__ logits, int64_t ld, int V,
                                                               const int64_t* __restrict__ out_tokens, int64_t out_stride,
                                                               int out_cols, const int32_t* __restrict__ step_dev,
                                                               const int64_t* __restrict__ eos_ids, int n_eos,
                                                               const int32_t* __restrict__ trie, int trie_words,
                                                               int32_t* __restrict__ nodes, int64_t node_stride) {
    extern __shared__ unsigned int cn_bits[];       // W + 1 words: the sweep reads word w + 1 beside word w
    const int b = blockIdx.x, tid = threadIdx.x;
    const int W = (V + 31) >> 5;
    for (int w = tid; w <= W; w += CN_THREADS) cn_bits[w] = 0u;

    int t = step_dev ? step_dev[0] : 0;
    t = out_tokens ? max(0, min(t, out_cols)) : 0;
    // the block: sizes first, then five arrays behind one another; a block that does not fit its buffer has no node
    int n_nodes = trie[0], n_edges = trie[1];
    const int n_rows = trie[2];
    const int64_t term_words = ((int64_t)n_nodes + 31) >> 5;
    const bool ok = n_nodes >= 0 && n_edges >= 0 && n_rows >= 0 &&
                    (int64_t)CN_HEADER + n_rows + ((int64_t)n_nodes + 1) + 2 * (int64_t)n_edges + term_words <= (int64_t)trie_words;
    if (!ok) n_nodes = n_edges = 0;
    const int32_t* first = trie + CN_HEADER + (ok ? n_rows : 0);
    const int32_t* tok = first + n_nodes + 1;
    const int32_t* child = tok + n_edges;
    const int32_t* term = child + n_edges;

    int32_t* plane = nodes + (int64_t)b * node_stride;
    int node;
    if (t == 0) {
        node = plane[0];                            // written when the request was armed: the row's root
    } else {
        const int prev = plane[t - 1];
        const int64_t id = out_tokens[(int64_t)b * out_stride + (t - 1)];
        node = CN_DEAD;
        if (prev >= 0 && prev < n_nodes && id >= 0 && id < V) {
            int lo = first[prev], hi = first[prev + 1];
            if (lo >= 0 && lo <= hi && hi <= n_edges) {
                while (lo < hi) {                   // the first edge whose token is >= id
                    const int mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)tok[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < first[prev + 1] && (int64_t)tok[lo] == id) node = child[lo];
            }
        }
    }
    if (node < 0 || node >= n_nodes) node = CN_DEAD;
    if (t > 0 && tid == 0) plane[t] = node;
    __syncthreads();

    bool eos_ok = node == CN_DEAD;
    if (node != CN_DEAD) {
        eos_ok = (term[node >> 5] >> (node & 31)) & 1;
        const int e0 = first[node], e1 = first[node + 1];
        if (e0 >= 0 && e0 <= e1 && e1 <= n_edges)
            for (int e = e0 + tid; e < e1; e += CN_THREADS) {
                const int id = tok[e];
                if (id >= 0 && id < V) atomicOr(&cn_bits[id >> 5], 1u << (id & 31));
            }
    }
    if (eos_ok)
        for (int e = tid; e < n_eos; e += CN_THREADS) {
            const int64_t id = eos_ids[e];
            if (id >= 0 && id < V) atomicOr(&cn_bits[id >> 5], 1u << (id & 31));
        }
    __syncthreads();

    // the sweep: elements in front of the row's first 16-byte boundary and behind its last one singly, the pieces between whole
    constexpr int E = 16 / (int)sizeof(T);
    constexpr unsigned int FULL = (1u << E) - 1u;
    T* row = logits + (int64_t)b * ld;
    const int mis = (int)(((uintptr_t)row / sizeof(T)) & (E - 1));
    const int head = min(V, (E - mis) & (E - 1));
    const int n_pieces = (V - head) / E;
    const int tail0 = head + n_pieces * E;
    auto allowed = [&](int i) { return (cn_bits[i >> 5] >> (i & 31)) & 1u; };
    auto ninf = [&](int i) {
        if (sizeof(T) == 4) reinterpret_cast<unsigned int*>(row)[i] = CnBits<T>::NEG_INF;
        else reinterpret_cast<uint16_t*>(row)[i] = (uint16_t)CnBits<T>::NEG_INF;
    };
    if (tid < head && !allowed(tid)) ninf(tid);
    if (tid < V - tail0 && !allowed(tail0 + tid)) ninf(tail0 + tid);
    const u32x4 all_ninf = cn_select<T>(u32x4{0u, 0u, 0u, 0u}, 0u);
    for (int p = tid; p < n_pieces; p += CN_THREADS) {
        const int i = head + p * E;
        const unsigned long long two = (unsigned long long)cn_bits[i >> 5] | ((unsigned long long)cn_bits[(i >> 5) + 1] << 32);
        const unsigned int m = (unsigned int)(two >> (i & 31)) & FULL;
        u32x4* piece = reinterpret_cast<u32x4*>(row + i);
        if (m == 0u) *piece = all_ninf;
        else if (m != FULL) *piece = cn_select<T>(*piece, m);
    }
}

extern "C" int gar_constrain(int dtype, void* logits, int64_t ld, int B, int V, const int64_t* out_tokens, int64_t out_stride,
                             int out_cols, const int32_t* step_dev, const int64_t* eos_ids, int n_eos, const int32_t* trie,
                             int trie_words, int32_t* nodes, int64_t node_stride, gar_stream_t stream) {
    GAR_CHECK_ARG(dtype == GAR_F32 || dtype == GAR_BF16, "constrain: dtype %d", dtype);
    GAR_CHECK_ARG(logits && trie && nodes && B > 0 && V > 0 && ld >= V, "constrain: bad args");
    GAR_CHECK_ARG(V <= gar_logits_process_max_vocab(), "constrain: V %d above %d (a vocabulary bitmap in LDS)", V,
                  gar_logits_process_max_vocab());
    GAR_CHECK_ARG(trie_words >= CN_HEADER, "constrain: a trie block of %d words, the header alone has %d", trie_words, CN_HEADER);
    GAR_CHECK_ARG(!out_tokens || (out_cols >= 0 && out_stride >= out_cols), "constrain: out_cols %d / out_stride %lld", out_cols,
                  (long long)out_stride);
    GAR_CHECK_ARG(node_stride >= (out_tokens ? (int64_t)out_cols + 1 : 1), "constrain: node_stride %lld below out_cols + 1 = %lld",
                  (long long)node_stride, (long long)(out_tokens ? (int64_t)out_cols + 1 : 1));
    GAR_CHECK_ARG(n_eos >= 0 && (n_eos == 0 || eos_ids), "constrain: eos_ids");
    const size_t lds = ((size_t)((V + 31) >> 5) + 1) * 4;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GAR_BF16)
        hipLaunchKernelGGL((constrain_kernel<bf16_t>), dim3(B), dim3(CN_THREADS), lds, s, (bf16_t*)logits, ld, V, out_tokens, out_stride,
                           out_cols, step_dev, eos_ids, n_eos, trie, trie_words, nodes, node_stride);
    else
        hipLaunchKernelGGL((constrain_kernel<float>), dim3(B), dim3(CN_THREADS), lds, s, (float*)logits, ld, V, out_tokens, out_stride,
                           out_cols, step_dev, eos_ids, n_eos, trie, trie_words, nodes, node_stride);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}
