// Beam search on the device (GARModel.generate(beam_search=BeamSearch(...))): the bookkeeping of one step and the
// reorder of the beams' cache rows by parent. Semantics: transformers' GenerationMixin._beam_search with do_sample=False, its
// f32 arithmetic restated operation by operation (tests/beam_search_ref.py is the torch restatement this file is checked
// against bit for bit, and that one against transformers itself).
//
// gar_beam_step: one 512-thread workgroup per prompt. The K rows of a prompt bring their M best raw log-probabilities each
// (gar_topk_lp: value descending, index ascending); the best M of the prompt's K * V continuations lie among these K * M.
//   1. candidates   score = running score + lp (f32), ranked by (score descending, beam ascending, token ascending): the best M
//   2. stopping     a candidate hits the criteria at an eos id, every candidate at the last step
//   3. running set  score + (-1e9 where it hit), the best K by (score descending, candidate rank ascending)
//   4. finished set score / len_pow[t], -1e9 for each of: set full under early_stopping=True, heuristic latch off, not one of the
//                   first K candidates that hit; merged behind the K kept hypotheses, the best K by (score descending, merged index
//                   ascending)
//   5. latches      the "improvement still possible" bit, the prompt's done bit, the count of done prompts
// Ranks are counted (every entry against every other, at most 512 x 512 compares out of LDS): no sort network, no atomics but
// the done counter, whose final value does not depend on order.
#include "common.h"

#define BEAM_THREADS 512
#define BEAM_MAX_K 16
#define BEAM_MAX_M 32
#define BEAM_NEG 1.0e9f

__global__ __launch_bounds__(BEAM_THREADS) void beam_step_kernel(gar_beam_state s) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = s.K, M = s.M, T = s.T, V = s.V;
    if (s.done[b]) return;                                  // latched: this prompt's state is frozen
    __shared__ float c_score[BEAM_THREADS];                 // the K * M candidates, (beam, rank in its row) order
    __shared__ int c_tok[BEAM_THREADS];
    __shared__ int top[BEAM_MAX_M];                         // candidate index by rank
    __shared__ float t_score[BEAM_MAX_M], t_run[BEAM_MAX_M], m_score[BEAM_MAX_K + BEAM_MAX_M];
    __shared__ int t_tok[BEAM_MAX_M], t_beam[BEAM_MAX_M], t_hit[BEAM_MAX_M];
    __shared__ int run_sel[BEAM_MAX_K], fin_sel[BEAM_MAX_K];
    __shared__ float run_old[BEAM_MAX_K], fin_old[BEAM_MAX_K];
    __shared__ int len_old[BEAM_MAX_K], flag_old[BEAM_MAX_K];
    __shared__ int full_sh;

    const int max_new = min(max(s.params[0], 1), T);
    const int mode = s.params[1];                           // 0 False, 1 True, 2 "never"
    const int lp_pos = s.params[2];
    const int n_eos = min(max(s.params[3], 0), GAR_BEAM_MAX_EOS);
    const int t = min(max(s.step_dev ? s.step_dev[0] : 0, 0), T - 1);
    const int KM = K * M;
    const int64_t row0 = (int64_t)b * K;

    if (tid < BEAM_MAX_M) top[tid] = 0;
    if (tid < BEAM_MAX_K) run_sel[tid] = fin_sel[tid] = 0;
    if (tid < K) {
        run_old[tid] = s.run_scores[row0 + tid];
        fin_old[tid] = s.fin_scores[row0 + tid];
        len_old[tid] = s.fin_len[row0 + tid];
        flag_old[tid] = s.fin_flag[row0 + tid] != 0;
    }
    __syncthreads();
    if (tid == 0) {
        int f = 1;
        for (int k = 0; k < K; ++k) f &= flag_old[k];
        full_sh = f;
    }
    if (tid < KM) {
        const int j = tid / M;
        const int id = s.top_ids[row0 * M + tid];
        c_tok[tid] = min(max(id, 0), V - 1);
        c_score[tid] = __fadd_rn(run_old[j], s.top_lp[row0 * M + tid]);
    }
    __syncthreads();
    if (tid < KM) {                                         // 1. rank among the K * M
        const float x = c_score[tid];
        const int j = tid / M, tok = c_tok[tid];
        int rank = 0;
        for (int o = 0; o < KM; ++o) {
            const float y = c_score[o];
            const int oj = o / M, ot = c_tok[o];
            const bool before = y > x || (y == x && (oj < j || (oj == j && (ot < tok || (ot == tok && o < tid)))));
            rank += before ? 1 : 0;
        }
        if (rank < M) top[rank] = tid;
    }
    __syncthreads();
    const bool heur = s.heur[b] != 0;
    if (tid < M) {                                          // 2. stopping criteria, the two derived scores
        const int c = top[tid];
        const int tok = c_tok[c];
        bool hit = t >= max_new - 1;
        for (int e = 0; e < n_eos; ++e) hit = hit || tok == s.params[4 + e];
        const float x = c_score[c];
        t_score[tid] = x;
        t_tok[tid] = tok;
        t_beam[tid] = c / M;
        t_hit[tid] = hit;
        t_run[tid] = hit ? __fadd_rn(x, -BEAM_NEG) : x;
        float f = __fdiv_rn(x, s.len_pow[t]);
        if (full_sh && mode == 1) f = __fadd_rn(f, -BEAM_NEG);
        if (!heur) f = __fadd_rn(f, -BEAM_NEG);
        if (!(hit && tid < K)) f = __fadd_rn(f, -BEAM_NEG);
        m_score[K + tid] = f;
    }
    if (tid < K) m_score[tid] = fin_old[tid];
    __syncthreads();
    if (tid < M) {                                          // 3. the K running beams of the next step
        const float x = t_run[tid];
        int rank = 0;
        for (int o = 0; o < M; ++o) rank += (t_run[o] > x || (t_run[o] == x && o < tid)) ? 1 : 0;
        if (rank < K) run_sel[rank] = tid;
    }
    if (tid < K + M) {                                      // 4. the K finished hypotheses
        const float x = m_score[tid];
        int rank = 0;
        for (int o = 0; o < K + M; ++o) rank += (m_score[o] > x || (m_score[o] == x && o < tid)) ? 1 : 0;
        if (rank < K) fin_sel[rank] = tid;
    }
    __syncthreads();

    const int32_t* hsrc = s.hist + (int64_t)(t & 1) * s.B * K * T;
    int32_t* hdst = s.hist + (int64_t)((t + 1) & 1) * s.B * K * T;
    for (int i = tid; i < K * (t + 1); i += BEAM_THREADS) {   // histories by parent, the new token at column t
        const int j = i / (t + 1), col = i - j * (t + 1);
        const int r = run_sel[j];
        hdst[(row0 + j) * T + col] = col < t ? hsrc[(row0 + t_beam[r]) * T + col] : t_tok[r];
    }
    if (tid < K) {
        const int r = run_sel[tid];
        s.run_scores[row0 + tid] = t_run[r];
        s.parent[row0 + tid] = t_beam[r];
        s.cur_tokens[row0 + tid] = t_tok[r];
        const int src = fin_sel[tid];
        s.fin_scores[row0 + tid] = m_score[src];
        s.fin_len[row0 + tid] = src < K ? len_old[src] : t + 1;
        s.fin_flag[row0 + tid] = src < K ? flag_old[src] : (t_hit[src - K] && src - K < K);
    }
    // the kept hypotheses' tokens, in place: kept ones stay in score order, so slot k takes a kept one from a slot <= k only;
    // filled from the last slot down, no source is overwritten before it is read
    for (int k = K - 1; k >= 0; --k) {
        const int src = fin_sel[k];
        int32_t* dst = s.fin_tokens + (row0 + k) * T;
        if (src < K) {
            if (src != k) {
                const int32_t* from = s.fin_tokens + (row0 + src) * T;
                for (int col = tid; col <= t; col += BEAM_THREADS) dst[col] = from[col];
            }
        } else {
            const int r = src - K;
            const int32_t* from = hsrc + (row0 + t_beam[r]) * T;
            for (int col = tid; col <= t; col += BEAM_THREADS) dst[col] = col < t ? from[col] : t_tok[r];
        }
        __syncthreads();
    }
    if (tid == 0) {                                         // 5. latches
        const float best_len = s.len_pow[(mode == 2 && lp_pos) ? max_new - 1 : t];
        const float best = __fdiv_rn(t_run[run_sel[0]], best_len);
        float worst = INFINITY;
        int full = 1, some = 0;
        for (int k = 0; k < K; ++k) {
            const int src = fin_sel[k];
            const int fl = src < K ? flag_old[src] : (t_hit[src - K] && src - K < K);
            worst = fminf(worst, m_score[src]);
            full &= fl;
            some |= fl;
        }
        // HF: any over the slots of best > (slot finished ? min score of the K : -1e9)
        const bool any = (some && best > worst) || (!full && best > -BEAM_NEG);
        const int h = heur && any;
        s.heur[b] = h;
        if (!h || (mode == 1 && full) || t >= max_new - 1) {
            s.done[b] = 1;
            atomicAdd(s.done_count, 1);
        }
    }
}

extern "C" int gar_beam_step(const gar_beam_state* s, gar_stream_t stream) {
    GAR_CHECK_ARG(s, "beam_step: null state");
    GAR_CHECK_ARG(s->top_ids && s->top_lp && s->run_scores && s->cur_tokens && s->parent && s->hist && s->fin_tokens &&
                      s->fin_scores && s->fin_len && s->fin_flag && s->heur && s->done && s->done_count && s->params && s->len_pow,
                  "beam_step: null pointer");
    GAR_CHECK_ARG(s->B > 0 && s->K >= 2 && s->K <= BEAM_MAX_K && s->M >= s->K && s->M <= BEAM_MAX_M &&
                      s->K * s->M <= BEAM_THREADS && s->T > 0 && s->V > 0,
                  "beam_step: bad shape (B %d, K %d in 2..16, M %d in K..32, T %d, V %d)", s->B, s->K, s->M, s->T, s->V);
    hipLaunchKernelGGL(beam_step_kernel, dim3(s->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *s);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// gar_kv_beam_reorder: cache row b * K + j takes the bytes of row b * K + parent[j] over positions s0 .. s0 + n - 1, for every
// layer, both caches, every kv head — one launch, in place. A thread owns one 16-byte chunk of one position for all K siblings:
// it loads the chunk every moved sibling takes, then stores them, so a cycle of parents needs no second cache. Consecutive
// threads own consecutive chunks of a position's hd elements and then of the next position: loads and stores are coalesced
// 16-byte accesses over a contiguous span of n * hd elements.
#define REORDER_THREADS 256

__global__ __launch_bounds__(REORDER_THREADS) void kv_beam_reorder_kernel(uint4* Kc, uint4* Vc, int R, int K, int Hkv,
                                                                          int64_t cap_chunks, int row_chunks, int cap, int s0,
                                                                          const int32_t* s0_dev, const int32_t* n_dev,
                                                                          const int32_t* parent) {
    // blockIdx.x = ((cache * L + layer) * B + prompt) * Hkv + head
    const int head = blockIdx.x % Hkv;
    const int B = R / K;
    const int b = (blockIdx.x / Hkv) % B;
    const int64_t lc = blockIdx.x / (Hkv * B);              // cache * L + layer
    const int L = gridDim.x / (2 * Hkv * B);
    uint4* base = lc < L ? Kc : Vc;
    const int64_t layer = lc < L ? lc : lc - L;
    if (s0_dev) s0 = s0_dev[0];
    s0 = min(max(s0, 0), cap);
    const int n = min(max(n_dev[0], 0), cap - s0);
    int par[BEAM_MAX_K];
    bool any = false;
#pragma unroll
    for (int j = 0; j < BEAM_MAX_K; ++j) {
        par[j] = j < K ? min(max(parent[b * K + j], 0), K - 1) : j;
        any = any || par[j] != j;
    }
    if (!any) return;
    const int64_t sib = (int64_t)Hkv * cap_chunks;          // chunks between sibling rows
    uint4* p0 = base + ((layer * R + (int64_t)b * K) * Hkv + head) * cap_chunks + (int64_t)s0 * row_chunks;
    const int64_t total = (int64_t)n * row_chunks;
    for (int64_t i = (int64_t)blockIdx.y * REORDER_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.y * REORDER_THREADS) {
        uint4 v[BEAM_MAX_K];
#pragma unroll
        for (int j = 0; j < BEAM_MAX_K; ++j)
            if (j < K && par[j] != j) v[j] = p0[par[j] * sib + i];
#pragma unroll
        for (int j = 0; j < BEAM_MAX_K; ++j)
            if (j < K && par[j] != j) p0[j * sib + i] = v[j];
    }
}

extern "C" int gar_kv_beam_reorder(void* Kc, void* Vc, int elem_size, int L, int R, int K, int Hkv, int cap, int hd, int s0,
                                   const int32_t* s0_dev, const int32_t* n_dev, const int32_t* parent, gar_stream_t stream) {
    GAR_CHECK_ARG(Kc && Vc && n_dev && parent, "kv_beam_reorder: null pointer");
    GAR_CHECK_ARG(elem_size == 2 || elem_size == 4, "kv_beam_reorder: element size %d (2 or 4)", elem_size);
    GAR_CHECK_ARG(L > 0 && K >= 2 && K <= BEAM_MAX_K && R > 0 && R % K == 0 && Hkv > 0 && cap > 0 && hd > 0 && s0 >= 0 && s0 <= cap,
                  "kv_beam_reorder: bad shape (L %d, rows %d, K %d in 2..16, Hkv %d, capacity %d, hd %d, s0 %d)", L, R, K, Hkv, cap,
                  hd, s0);
    GAR_CHECK_ARG(((int64_t)hd * elem_size) % 16 == 0 && ((uintptr_t)Kc & 15) == 0 && ((uintptr_t)Vc & 15) == 0,
                  "kv_beam_reorder: a position's hd * element bytes and the caches must be 16-byte aligned");
    const int row_chunks = hd * elem_size / 16;
    const int64_t cap_chunks = (int64_t)cap * row_chunks;
    const int64_t slabs = 2LL * L * (R / K) * Hkv;
    GAR_CHECK_ARG(slabs < (1LL << 31), "kv_beam_reorder: %lld (cache, layer, prompt, head) slabs", (long long)slabs);
    // the grid cannot follow n (a device value of a captured launch): enough workgroups per slab to fill the device at the
    // full capacity, each striding over the n * row_chunks chunks that exist
    int64_t per = (cap_chunks + REORDER_THREADS - 1) / REORDER_THREADS;
    int64_t want = (8LL * gar_num_cus() + slabs - 1) / slabs;
    int gy = (int)std::max<int64_t>(1, std::min<int64_t>(per, std::min<int64_t>(want, 65535)));
    hipLaunchKernelGGL(kv_beam_reorder_kernel, dim3((unsigned)slabs, gy), dim3(REORDER_THREADS), 0, (hipStream_t)stream, (uint4*)Kc,
                       (uint4*)Vc, R, K, Hkv, cap_chunks, row_chunks, cap, s0, s0_dev, n_dev, parent);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}
