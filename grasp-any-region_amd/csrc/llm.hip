// Llama-side data movement kernels:
//   llm_qkv_post   half-split RoPE (llama3-scaled tables) + q scale + head-major relayout + KV-cache append
//                  (K and V both [B,Hkv,Smax,hd]: one contiguous row per appended token; the attention kernels form the PV
//                  operand with gfx950's transposing LDS read)
//   embed_lookup   embedding rows of the just-sampled tokens
//   argmax         greedy sampling with first-index tie break; writes into the device-side token matrix
//   sample         do_sample = True: temperature / top-k / top-p warpers + one Philox draw per row and step — one body (sample_row), one
//                  radix descent (smp_descent) for its three thresholds, one kernel templated on where a row's request comes from
//                  (the state's words: gar_sample; those and HF's min_p / typical_p / epsilon / eta cutoff warpers between top-p and
//                  the draw: gar_sample_ext; a word table per row: gar_sample_rows)
//                  (argmax and sample both with an LP instantiation that also writes the chosen token's log-probability; one sink,
//                  PickSink, and one epilogue, commit_token, commit the token)
//   topk_lp        the k most likely tokens of a step and the log-probabilities of given token ids
#include <type_traits>

#include "common.h"

// Column of natural dim d0 (first element of an 8-wide slice) inside a q / k head whose rows of W — and therefore whose columns
// of the qkv GEMM output — are in the fused RoPE epilogue's strip order (include/gar_hip.h, GAR_EPI_QKV_ROPE_LLM: the only
// bf16 copy of the Llama qkv weight is the folded one in that order): head_dim 128 keeps dims [0..31, 64..95, 32..63, 96..127],
// head_dim 64 the natural order.
template <int HD>
__device__ __forceinline__ int strip_col(int d0, bool strip) {
    if (HD != 128 || !strip) return d0;
    const int blk = d0 >> 5;
    return blk == 1 ? d0 + 32 : (blk == 2 ? d0 - 32 : d0);
}

// block = (batch b, 64-position chunk); loops over all heads of q, k, v.
// thread (token nl = tid/ (HD/16), i8 = 8-wide slice of the FIRST half): rotates (x[i], x[i+HD/2]) pairs of the q / k heads;
// the v heads go through the same loop unrotated (cos = 1, sin = 0) into the row-major V cache.
template <typename T, int HD>
__global__ __launch_bounds__(256) void llm_qkv_post_kernel(const T* __restrict__ qkv, const float* __restrict__ cs,
                                                           const float* __restrict__ sn, T* __restrict__ Q,
                                                           T* __restrict__ Kc, T* __restrict__ Vc, int S, int Spad,
                                                           int Hq, int Hkv, int Smax, int pos0,
                                                           const int32_t* __restrict__ pos_dev,
                                                           const int32_t* __restrict__ left_pad, float q_scale, int strip) {
    constexpr int HALF = HD / 2;
    constexpr int LPT = HALF / 8;               // lanes per token (4 for hd 64, 8 for hd 128)
    constexpr int TPP = 256 / LPT;              // tokens per pass (64 / 32)
    const int chunks = (Spad + 63) / 64;
    const int ch = blockIdx.x % chunks;
    const int b = blockIdx.x / chunks;
    const int tid = threadIdx.x;
    const int i8 = (tid % LPT) * 8;
    const int p0 = pos_dev ? pos_dev[0] : pos0;
    // left-padded batch (HF generation): sequence b starts at row left_pad[b]; the CACHE row of a token stays its row in the
    // padded sequence, only its RoPE position is counted from the first real token (rows before it: position 0, never read)
    const int lp = left_pad ? left_pad[b] : 0;
    const int nh = Hq + 2 * Hkv;
    const int W = nh * HD;
    // a thread keeps its token and its 8-wide slice for every head, so cos / sin are loaded once per pass and the rows of
    // RU heads are in flight together (a CU holds 16 waves: the latency cover has to come from here)
    constexpr int RU = 4;
    for (int pass = 0; pass < 64 / TPP; ++pass) {
        const int nl = pass * TPP + tid / LPT;
        const int s = ch * 64 + nl;
        float c[8], sv[8];
        if (s < S) {
            const int rp = max(p0 + s - lp, 0);
            ld8(cs + (int64_t)rp * HALF + i8, c);
            ld8(sn + (int64_t)rp * HALF + i8, sv);
        }
        for (int head0 = 0; head0 < nh; head0 += RU) {
            float x1[RU][8], x2[RU][8];
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int head = head0 + u;
                if (s < S && head < nh) {
                    const T* row = qkv + ((int64_t)b * S + s) * W + head * HD;
                    const bool so = strip && head < Hq + Hkv;          // v heads keep the natural order
                    ld8(row + strip_col<HD>(i8, so), x1[u]);
                    ld8(row + strip_col<HD>(HALF + i8, so), x2[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) x1[u][e] = x2[u][e] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int head = head0 + u;
                if (head >= nh) break;
                const bool isq = head < Hq, isv = head >= Hq + Hkv;
                if (s < S && !isv) {
                    const float sc = isq ? q_scale : 1.0f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) rope_half_pair(x1[u][e], x2[u][e], c[e], sv[e], sc, x1[u][e], x2[u][e]);
                }
                if (isq && s < Spad) {
                    T* o = Q + (((int64_t)b * Hq + head) * Spad + s) * HD;
                    st8(o + i8, x1[u]);
                    st8(o + HALF + i8, x2[u]);
                } else if (!isq && s < S) {         // k and v rows of the cache: [B, Hkv, Smax, HD] both
                    T* o = (isv ? Vc + ((int64_t)b * Hkv + (head - Hq - Hkv)) * (int64_t)Smax * HD
                                : Kc + ((int64_t)b * Hkv + (head - Hq)) * (int64_t)Smax * HD) + (int64_t)(p0 + s) * HD;
                    st8(o + i8, x1[u]);
                    st8(o + HALF + i8, x2[u]);
                }
            }
        }
    }
}

// decode (S == 1): one thread per (batch, head, 8-wide slice of the first half) — a single small launch.
template <typename T, int HD>
__global__ __launch_bounds__(256) void llm_qkv_post_decode_kernel(const T* __restrict__ qkv, const float* __restrict__ cs,
                                                                  const float* __restrict__ sn, T* __restrict__ Q,
                                                                  T* __restrict__ Kc, T* __restrict__ Vc, int B, int Spad,
                                                                  int Hq, int Hkv, int Smax, int pos0,
                                                                  const int32_t* __restrict__ pos_dev,
                                                                  const int32_t* __restrict__ left_pad, float q_scale, int strip) {
    constexpr int HALF = HD / 2, LPH = HALF / 8;
    const int nh = Hq + 2 * Hkv;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * nh * LPH) return;
    const int i8 = (idx % LPH) * 8;
    const int head = (idx / LPH) % nh;
    const int b = idx / (LPH * nh);
    const int p0 = pos_dev ? pos_dev[0] : pos0;
    const T* row = qkv + (int64_t)b * nh * HD + head * HD;
    float x1[8], x2[8];
    const bool so = strip && head < Hq + Hkv;
    ld8(row + strip_col<HD>(i8, so), x1);
    ld8(row + strip_col<HD>(HALF + i8, so), x2);
    if (head < Hq + Hkv) {
        const int rp = max(p0 - (left_pad ? left_pad[b] : 0), 0);          // RoPE position; the cache row stays p0
        const float* cp = cs + (int64_t)rp * HALF + i8;
        const float* sp = sn + (int64_t)rp * HALF + i8;
        const float sc = head < Hq ? q_scale : 1.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) rope_half_pair(x1[e], x2[e], cp[e], sp[e], sc, x1[e], x2[e]);
        T* o = head < Hq ? Q + (((int64_t)b * Hq + head) * Spad) * HD
                         : Kc + (((int64_t)b * Hkv + (head - Hq)) * Smax + p0) * HD;
        st8(o + i8, x1);
        st8(o + HALF + i8, x2);
    } else {
        T* o = Vc + (((int64_t)b * Hkv + (head - Hq - Hkv)) * Smax + p0) * HD;
        st8(o + i8, x1);
        st8(o + HALF + i8, x2);
    }
}

extern "C" int gar_llm_qkv_post(int dtype, const void* qkv, const float* cs, const float* sn, void* Q, void* Kc,
                                void* Vc, int B, int S, int Spad, int Hq, int Hkv, int hd, int Smax, int pos0,
                                const int32_t* pos_dev, const int32_t* left_pad, float q_scale, int qk_strip_order,
                                gar_stream_t stream) {
    GAR_CHECK_ARG(qkv && cs && sn && Q && Kc && Vc, "llm_qkv_post: null pointer");
    const int strip = qk_strip_order ? 1 : 0;
    GAR_CHECK_ARG(B > 0 && S > 0 && Spad >= S && Smax % 64 == 0, "llm_qkv_post: bad shape");
    GAR_CHECK_ARG(pos_dev || pos0 + S <= Smax, "llm_qkv_post: cache overflow %d+%d > %d", pos0, S, Smax);
    GAR_CHECK_ARG(hd == 64 || hd == 128, "llm_qkv_post: head_dim %d not built (64, 128)", hd);
    hipStream_t s = (hipStream_t)stream;
    if (S == 1) {
        const int total = B * (Hq + 2 * Hkv) * (hd / 16);
        dim3 g1((total + 255) / 256), b1(256);
#define LAUNCH_LQD(TT, HD_)                                                                                         \
    hipLaunchKernelGGL((llm_qkv_post_decode_kernel<TT, HD_>), g1, b1, 0, s, (const TT*)qkv, cs, sn, (TT*)Q, (TT*)Kc, \
                       (TT*)Vc, B, Spad, Hq, Hkv, Smax, pos0, pos_dev, left_pad, q_scale, strip)
        if (dtype == GAR_BF16) { if (hd == 64) LAUNCH_LQD(bf16_t, 64); else LAUNCH_LQD(bf16_t, 128); }
        else { if (hd == 64) LAUNCH_LQD(float, 64); else LAUNCH_LQD(float, 128); }
#undef LAUNCH_LQD
        GAR_CHECK_LAUNCH();
        return GAR_OK;
    }
    dim3 grid(B * ((Spad + 63) / 64)), block(256);
#define LAUNCH_LQP(TT, HD_)                                                                                       \
    hipLaunchKernelGGL((llm_qkv_post_kernel<TT, HD_>), grid, block, 0, s, (const TT*)qkv, cs, sn, (TT*)Q, (TT*)Kc,  \
                       (TT*)Vc, S, Spad, Hq, Hkv, Smax, pos0, pos_dev, left_pad, q_scale, strip)
    if (dtype == GAR_BF16) { if (hd == 64) LAUNCH_LQP(bf16_t, 64); else LAUNCH_LQP(bf16_t, 128); }
    else { if (hd == 64) LAUNCH_LQP(float, 64); else LAUNCH_LQP(float, 128); }
#undef LAUNCH_LQP
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_lookup_kernel(const int64_t* __restrict__ tokens, const T* __restrict__ E,
                                                           T* __restrict__ out, int C, int64_t vocab) {
    int64_t id = tokens[blockIdx.x];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const T* src = E + id * C;
    T* dst = out + (int64_t)blockIdx.x * C;
    for (int i = threadIdx.x * 8; i < C; i += 256 * 8) {
        float v[8];
        ld8(src + i, v);
        st8(dst + i, v);
    }
}

extern "C" int gar_embed_lookup(int dtype, const int64_t* tokens, const void* E, void* out, int B, int C, int64_t vocab,
                                gar_stream_t stream) {
    GAR_CHECK_ARG(tokens && E && out && B > 0 && C % 8 == 0, "embed_lookup: bad args");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GAR_BF16)
        hipLaunchKernelGGL((embed_lookup_kernel<bf16_t>), dim3(B), dim3(256), 0, s, tokens, (const bf16_t*)E, (bf16_t*)out,
                           C, vocab);
    else
        hipLaunchKernelGGL((embed_lookup_kernel<float>), dim3(B), dim3(256), 0, s, tokens, (const float*)E, (float*)out, C,
                           vocab);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Token pick. What the greedy kernels, sample_kernel and the topk_lp kernels share is written once here: the order of (value, index)
// pairs and its wave reduction (beside common.h's wave_sum / wave_max), the two halves of logsumexp over AM_BLOCKS blocks, and the
// sink a row's token is committed to. Every reduction has a fixed shape (xor tree inside a wave, waves in order): deterministic.
// ---------------------------------------------------------------------------------------------------------------
#define AM_BLOCKS 64

__device__ __forceinline__ void am_better(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

__device__ __forceinline__ void wave_best(float& bv, int& bi) {         // every lane: the wave's best pair in am_better's order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        am_better(bv, bi, ov, oi);
    }
}

// Per-block half of logsumexp, 256 threads: sum exp(x - bv) over the block's elements, bv the block's maximum. each(f) calls
// f(x) for the calling thread's elements. The four wave sums land in ss (behind a barrier); block_exp_sum4 adds them.
// An empty block or one of -inf logits only has bv = -inf and sums to 0, never exp(-inf - -inf) = NaN.
template <typename Each>
__device__ __forceinline__ void block_exp_sums(float bv, float* ss, Each each) {
    float s = 0.f;
    if (bv > -INFINITY) each([&](float x) { s += __expf(x - bv); });
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) ss[threadIdx.x >> 6] = s;
    __syncthreads();
}

__device__ __forceinline__ float block_exp_sum4(const float* ss) { return ((ss[0] + ss[1]) + ss[2]) + ss[3]; }

// Per-row half, one wave, lane j holding block j's (max mv, sum *ps): sum_j s_j exp(m_j - M), M the row's maximum
__device__ __forceinline__ float merge_exp_sums(float mv, float M, const float* ps) {
    return wave_sum(mv > -INFINITY ? *ps * __expf(mv - M) : 0.f);
}

// Where a pick kernel commits row b's token of a step: the token matrix and the current tokens, the log-probability planes laid out
// like out_tokens (each may be NULL), and the stopping criterion on the device (HF: EosTokenCriteria over eos_token_id, a list): the
// FIRST step at which row b produced an end-of-sequence id is latched in finished[b] (-1 = still running), and done_count counts the
// latched rows — the host's "is every row done" poll reads one int instead of scanning the token matrix (entries < 0 of eos_ids
// never match). Passed by value to the kernels; pick_sink fills and checks it.
struct PickSink {
    int64_t* out_tokens;
    int64_t out_stride;
    int64_t* cur_tokens;
    const int64_t* eos_ids;
    int n_eos;
    int32_t* finished;
    int32_t* done_count;
    float* lp_raw;
    float* lp_warped;
};

template <bool LP>          // LP = false: no plane code is compiled
__device__ __forceinline__ void commit_token(const PickSink& sk, int b, int tok, int col, float raw, float warped) {
    if (sk.out_tokens) sk.out_tokens[(int64_t)b * sk.out_stride + col] = tok;
    if (sk.cur_tokens) sk.cur_tokens[b] = tok;
    if constexpr (LP) {
        if (sk.lp_raw) sk.lp_raw[(int64_t)b * sk.out_stride + col] = raw;
        if (sk.lp_warped) sk.lp_warped[(int64_t)b * sk.out_stride + col] = warped;
    }
    if (sk.finished && sk.eos_ids && sk.finished[b] < 0) {
        bool hit = false;
        for (int e = 0; e < sk.n_eos; ++e) hit |= (sk.eos_ids[e] == (int64_t)tok);
        if (hit) {
            sk.finished[b] = col;
            if (sk.done_count) atomicAdd(sk.done_count, 1);
        }
    }
}

// The sink of an entry point's nine commit arguments. lp: the entry point writes log-probabilities, so it needs a plane.
static int pick_sink(PickSink& sk, const char* who, bool lp, int64_t* out_tokens, int64_t out_stride, int64_t* cur_tokens,
                     const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, float* lp_raw, float* lp_warped) {
    GAR_CHECK_ARG(out_tokens || cur_tokens, "%s: neither out_tokens nor cur_tokens", who);
    GAR_CHECK_ARG(n_eos >= 0 && (n_eos == 0 || eos_ids) && (!finished || eos_ids), "%s: eos_ids / finished", who);
    GAR_CHECK_ARG(!lp || lp_raw || lp_warped, "%s: no log-probability plane (the entry point without _lp is the form without)", who);
    sk = {out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, lp_raw, lp_warped};
    return GAR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// argmax: stage 1 = AM_BLOCKS partial (max, first index) per row; stage 2 = one wave per row.
// LP (gar_argmax_lp): the instantiations that also write the chosen token's log-probability. Stage 1 adds, per block,
// s = sum exp(x - block max) (a second pass over the block's ~V/64 logits, which the first just pulled into the cache) into ps;
// stage 2 merges the 64 (max, s) pairs. The chosen token IS the maximum, so log p = -log of that sum. LP = false (gar_argmax)
// reads neither ps nor the planes.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, bool LP>
__global__ __launch_bounds__(256) void argmax_partial_kernel(const T* __restrict__ logits, int64_t ld, int V,
                                                             float* __restrict__ pv, int* __restrict__ pi,
                                                             float* __restrict__ ps) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float ss[4];
    const int b = blockIdx.y, blk = blockIdx.x;
    const T* row = logits + (int64_t)b * ld;
    const int per = (V + AM_BLOCKS - 1) / AM_BLOCKS;
    const int lo = blk * per, hi = min(V, lo + per);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = lo + threadIdx.x; i < hi; i += 256) am_better(bv, bi, DT<T>::ld(row + i), i);
    wave_best(bv, bi);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (LP || threadIdx.x == 0) {                   // the block's (max, first index): LP in every thread, for the sum
        if constexpr (LP) { bv = sv[0]; bi = si[0]; }
        for (int w = 1; w < 4; ++w) am_better(bv, bi, sv[w], si[w]);
    }
    if constexpr (LP)
        block_exp_sums(bv, ss, [&](auto f) {
            for (int i = lo + threadIdx.x; i < hi; i += 256) f(DT<T>::ld(row + i));
        });
    if (threadIdx.x == 0) {
        pv[b * AM_BLOCKS + blk] = bv;
        pi[b * AM_BLOCKS + blk] = bi;
        if constexpr (LP) ps[b * AM_BLOCKS + blk] = block_exp_sum4(ss);
    }
}

// (the greedy kernels are as they were: this one keeps its scalar parameter list, which compiles to the code it always had, and
// forms the sink itself)
template <bool LP>
__global__ __launch_bounds__(64) void argmax_final_kernel(const float* __restrict__ pv, const int* __restrict__ pi,
                                                          const float* __restrict__ ps, int64_t* __restrict__ out_tokens,
                                                          int64_t out_stride, const int32_t* __restrict__ step_dev,
                                                          int64_t* __restrict__ cur_tokens,
                                                          const int64_t* __restrict__ eos_ids, int n_eos,
                                                          int32_t* __restrict__ finished, int32_t* __restrict__ done_count,
                                                          float* __restrict__ lp_raw, float* __restrict__ lp_warped) {
    const int b = blockIdx.x;
    const float mv = pv[b * AM_BLOCKS + threadIdx.x];
    float bv = mv;
    int bi = pi[b * AM_BLOCKS + threadIdx.x];
    wave_best(bv, bi);
    float s = 0.f;
    if constexpr (LP) s = merge_exp_sums(mv, bv, &ps[b * AM_BLOCKS + threadIdx.x]);
    if (threadIdx.x == 0) {
        const int step = step_dev ? step_dev[0] : 0;
        const float lp = 0.f - logf(s);             // x[tok] - max = 0: HF's processed scores of greedy search are the raw logits
        commit_token<LP>({out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, lp_raw, lp_warped}, b, bi, step, lp, lp);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Sampling (do_sample = True): HF's warpers in their order — temperature, top-k, top-p — then one draw from what is left
// (transformers TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper + torch.multinomial in GenerationMixin._sample;
// the reference forwards the caller's GenerationConfig, modeling_gar.py:418-426). One 1024-thread workgroup per row, the row read
// ~12 times out of L2 (128 k logits: tens of microseconds); no sort:
//   z = logit / T (fp32 division), ordered by an order-preserving 32-bit key;
//   top-k: the k-th largest key, that is the smallest key with fewer than k strictly larger ones, by a 4 x 8-bit radix descent
//          (smp_descent) over COUNTS; keep key >= it (ties at the k-th value stay, as `scores < topk(scores, k)[0][..., -1]` removes
//          strictly smaller ones only);
//   top-p: a token stays iff the probability mass of the strictly larger keys is < top_p (HF removes ascending-cumsum <= 1 - top_p:
//          the same set up to ties, which stay or go together here) — the smallest such key by the same descent over MASS;
//   draw: u = 24 random bits of Philox4x32-10(key = seed, counter = (step, row)) / 2^24; the token is the first index (in VOCABULARY
//          order) whose running sum of kept exp(z - max) exceeds u x their total. Deterministic: per-wave histograms merged in wave
//          order, fixed-shape scans — the same (logits, seed, step, row) always give the same token; oracle/sampling.py restates it.
// ---------------------------------------------------------------------------------------------------------------
#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)

__device__ __forceinline__ unsigned int smp_key(float z) {           // larger z <-> larger key; -0 and +0 differ (harmless), NaN sorts high
    const unsigned int u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned int smp_mulhi(unsigned int a, unsigned int b) { return __umulhi(a, b); }

// Philox4x32-10 (Salmon et al. 2011), first output word
__device__ __forceinline__ unsigned int philox_first(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                                                     unsigned int k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned int hi0 = smp_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned int hi1 = smp_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned int n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// One row's request, as sample_row reads it: the warpers' parameters, the Philox key, the two counter words of the draw (the row's
// step and its counter row) and the column of the token matrix the token is committed at. sample_kernel fills it from its source.
struct SmpReq {
    float temperature, top_p;
    int top_k;
    unsigned int seed_lo, seed_hi, step, crow;
    int col;
    float min_p = 0.f, typical_p = 1.f, epsilon = 0.f, eta = 0.f;       // EXT only (gar_sample_ext): 0 / 1 / 0 / 0 = off
    int32_t* n_kept = nullptr;                                          // EXT only: the size of the final kept set, [B] or NULL
};

// The key floor of "keep z >= thr": -0 sorts below +0 in smp_key's order, so a threshold of either zero takes the lower key
__device__ __forceinline__ unsigned int smp_floor_key(float thr) { return smp_key(thr == 0.f ? -0.f : thr); }

// A sampling workgroup's LDS
struct SmpLds {
    float hist_f[SMP_WAVES][256];       // per-wave mass histograms (merged in wave order: deterministic)
    int hist_i[256];
    float red_f[SMP_WAVES];
    float scan_f[SMP_THREADS];
    unsigned int sh_u[4];
    float sh_f[4];
};

// Block reductions of the 1024 threads, every thread gets the result. Fixed shape: xor tree inside a wave, waves in order. The leading
// barrier frees red_f from the reduction before. The empty asm takes the result where it is written: left alone, the compiler sinks
// the 16-operand chain to its first use and holds the operands in registers until then (the LP sum across the whole kernel).
__device__ __forceinline__ float block_sum(SmpLds& L, float v) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) L.red_f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < SMP_WAVES; ++w) t += L.red_f[w];
    asm volatile("" : "+v"(t));
    return t;
}

__device__ __forceinline__ float block_max(SmpLds& L, float v) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) L.red_f[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = L.red_f[0];
    for (int w = 1; w < SMP_WAVES; ++w) t = fmaxf(t, L.red_f[w]);
    asm volatile("" : "+v"(t));
    return t;
}

// The radix descent of top-k, top-p and typical_p: four levels of 8 bits over 32-bit keys. each(i, key, w) says whether element i is in
// the set and yields its key and its weight. With the buckets walked from the near end — the largest key (DESC) or the smallest — the
// result is the LAST key of the set whose strictly nearer keys amount to less than lim, and that amount (`beyond`); the nearest key
// always qualifies. Acc = int counts elements, in hist_i alone: no float histograms, no float clears, no merge barrier. Acc = float
// adds the weights, in a fixed order: per-wave histograms, a wave's lanes adding inside one LDS instruction; the waves merged in wave
// order by threads 0..255; the buckets scanned by thread 0 (hist_i tells an empty bucket from one of mass 0).
template <typename Acc>
struct SmpCut {
    unsigned int key;
    Acc beyond;
};

template <typename Acc, bool DESC, typename Each>
__device__ __forceinline__ SmpCut<Acc> smp_descent(SmpLds& L, int V, Acc lim, Each each) {
    constexpr bool MASS = std::is_same<Acc, float>::value;
    const int tid = threadIdx.x, wave = tid >> 6;
    unsigned int prefix = 0u;
    Acc beyond = 0;
#pragma unroll 1                                 // one copy of the body: the levels are separated by barriers anyway
    for (int level = 3; level >= 0; --level) {
        const int sh = level * 8;
        const unsigned int pmask = level == 3 ? 0u : (0xffffffffu << (sh + 8));
        if constexpr (MASS)
            for (int i = tid; i < SMP_WAVES * 256; i += SMP_THREADS) (&L.hist_f[0][0])[i] = 0.f;
        for (int i = tid; i < 256; i += SMP_THREADS) L.hist_i[i] = 0;
        __syncthreads();
        for (int i = tid; i < V; i += SMP_THREADS) {     // a wave's 64 consecutive elements per turn
            unsigned int k;
            float w;
            if (each(i, k, w) && (k & pmask) == prefix) {
                if constexpr (MASS) atomicAdd(&L.hist_f[wave][(k >> sh) & 255u], w);
                atomicAdd(&L.hist_i[(k >> sh) & 255u], 1);
            }
        }
        __syncthreads();
        if constexpr (MASS) {
            if (tid < 256) {
                float t = 0.f;
                for (int w = 0; w < SMP_WAVES; ++w) t += L.hist_f[w][tid];
                L.scan_f[tid] = t;
            }
            __syncthreads();
        }
        if (tid == 0) {
            // four buckets are read ahead of their turn, so the walk waits for LDS once per four; the amounts are added one by one,
            // in bucket order, up to the first non-empty bucket that does not qualify
            int bsel = -1;
            bool open = true;
            Acc run = beyond, run_sel = beyond;
            for (int j0 = 0; j0 < 256 && open; j0 += 4) {
                int n[4];
                Acc amount[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = DESC ? 255 - (j0 + u) : j0 + u;
                    n[u] = L.hist_i[q];
                    if constexpr (MASS) amount[u] = L.scan_f[q];
                    else amount[u] = n[u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (n[u] > 0) {
                        open = run < lim || bsel < 0;
                        if (!open) break;
                        bsel = DESC ? 255 - (j0 + u) : j0 + u;
                        run_sel = run;
                    }
                    run += amount[u];
                }
            }
            L.sh_u[0] = (unsigned int)max(bsel, 0);
            if constexpr (MASS) L.sh_f[0] = run_sel;
            else L.sh_u[1] = (unsigned int)run_sel;
        }
        __syncthreads();
        prefix |= L.sh_u[0] << sh;
        if constexpr (MASS) beyond = L.sh_f[0];
        else beyond = (Acc)L.sh_u[1];
        __syncthreads();
    }
    return {prefix, beyond};
}

// The body of the sampling kernel: row b's token under rq, drawn by its 1024-thread workgroup (every thread of it calls this, with
// the same rq) and committed at column rq.col. Top to bottom: max, top-k, mass, top-p, the EXT stages, draw.
// LP (gar_sample_lp): the instantiation that also writes the drawn token's log-probabilities — raw = x[tok] - logsumexp(x[0:V]) over the
// logits as stored, warped = z[tok] - max z - log Z2 over the kept set (the distribution the draw was taken from) — into planes laid
// out like out_tokens. One more strided pass for sum exp(x - max z * T), reduced by block_sum; LP = false (gar_sample, gar_sample_rows)
// makes no such pass and writes no plane.
// EXT (gar_sample_ext): HF's four further warpers between top-p and the draw, in GenerationMixin._get_logits_processor's order, each
// over the set the stage before it left (p = e / Z of that set, e = exp(z - mx), mx the ROW maximum: a common shift cancels):
//   min_p     keep p >= min_p x max p. The row maximum is in the set, so this is e >= min_p: a key floor at mx + log(min_p), no pass;
//   typical_p s = |(z - mx) - mean|, mean = sum e (z - mx) / Z (the entropy is log Z - mean); keep s <= s_cut, s_cut the largest s whose
//             strictly smaller s hold less than typical_p of the mass: one pass for (Z, mean), then the descent run ASCENDING over
//             the bits of s (s >= 0: its bits order like its value). It may remove the maximum;
//   epsilon   keep p >= epsilon, and the set's maximum: one mass pass, a key floor at min(mx + log(epsilon Z), max of the set);
//   eta       the same with eta' = min(eta, sqrt(eta) exp(-H)), H the set's entropy: one mass + entropy pass.
// The kept set is ONE predicate, kept(z): the key floor key_lo and, when typical_p acted, s <= typ_cut recomputed from the saved
// (typ_mean, typ_cut) — every pass after a stage and the draw evaluate exactly it. A stage that is off adds no pass and no barrier;
// with all four off the instantiation computes gar_sample's token and planes bit for bit. EXT = false compiles none of it.
template <typename T, bool LP, bool EXT>
__device__ __forceinline__ void sample_row(const T* __restrict__ row, int V, int b, const SmpReq& rq, const PickSink& sk) {
    __shared__ SmpLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    const float top_p = rq.top_p;
    const int top_k = rq.top_k;
    const float temp = rq.temperature > 0.f ? rq.temperature : 1.0f;       // (the host refuses temperature <= 0, as HF does)
    auto zof = [&](int i) { return DT<T>::ld(row + i) / temp; };
    // ---- max
    float mx = -INFINITY;
    for (int i = tid; i < V; i += SMP_THREADS) mx = fmaxf(mx, zof(i));
    mx = block_max(L, mx);
    // ---- LP: the mass of the whole row at temperature 1, shifted by xs = max z * T (the row maximum up to one rounding)
    const float xs = mx * temp;
    float Zraw = 0.f;
    if constexpr (LP) {
        float praw = 0.f;
        for (int i = tid; i < V; i += SMP_THREADS) praw += __expf(DT<T>::ld(row + i) - xs);
        Zraw = block_sum(L, praw);
    }
    // ---- the kept set: keep key >= key_lo and, EXT, once typical_p acted, s <= typ_cut. All four are uniform over the workgroup
    unsigned int key_lo = 0u;
    bool typ_on = false;
    float typ_mean = 0.f, typ_cut = 0.f;
    auto kept = [&](float z) -> bool {
        if constexpr (EXT) return smp_key(z) >= key_lo && (!typ_on || fabsf((z - mx) - typ_mean) <= typ_cut);
        else return smp_key(z) >= key_lo;
    };
    // its mass Z = sum e and, with S, S = sum e (z - mx) (e = 0: no term, never 0 x inf)
    auto kept_mass = [&](float* S) -> float {
        float pz = 0.f, ps = 0.f;
        for (int i = tid; i < V; i += SMP_THREADS) {
            const float z = zof(i);
            if (kept(z)) {
                const float e = __expf(z - mx);
                pz += e;
                if (S) ps += e > 0.f ? e * (z - mx) : 0.f;
            }
        }
        const float Z = block_sum(L, pz);
        if (S) *S = block_sum(L, ps);
        return Z;
    };
    // ---- top-k: the k-th largest key
    if (top_k > 0 && top_k < V)
        key_lo = smp_descent<int, true>(L, V, top_k, [&](int i, unsigned int& k, float& w) {
                     k = smp_key(zof(i));
                     w = 1.f;
                     return true;
                 }).key;
    // ---- mass of what top-k left
    const float Z1 = kept_mass(nullptr);
    // ---- top-p: the smallest key whose strictly-larger keys hold less than top_p of the mass
    if (top_p < 1.0f)
        key_lo = max(key_lo, smp_descent<float, true>(L, V, top_p * Z1, [&](int i, unsigned int& k, float& w) {
                                 const float z = zof(i);
                                 k = smp_key(z);
                                 w = __expf(z - mx);
                                 return k >= key_lo;
                             }).key);
    // ---- EXT: min_p, typical_p, epsilon, eta (see above)
    if constexpr (EXT) {
        if (rq.min_p > 0.f) key_lo = max(key_lo, smp_floor_key(mx + logf(rq.min_p)));
        if (rq.typical_p > 0.f && rq.typical_p < 1.0f) {
            float St;
            const float Zt = kept_mass(&St);
            const float mean = St / Zt;
            // the largest s whose strictly smaller s hold less than typical_p of the mass (the smallest always qualifies: HF keeps one token)
            const SmpCut<float> cut = smp_descent<float, false>(L, V, rq.typical_p * Zt, [&](int i, unsigned int& k, float& w) {
                const float z = zof(i);
                k = __float_as_uint(fabsf((z - mx) - mean));
                w = __expf(z - mx);
                return kept(z);                     // (typ_on is still false: the set min_p left)
            });
            typ_on = true;
            typ_mean = mean;
            typ_cut = __uint_as_float(cut.key);
        }
        const bool eps_on = rq.epsilon > 0.f && rq.epsilon < 1.0f, eta_on = rq.eta > 0.f && rq.eta < 1.0f;
        float m2 = mx;                              // the maximum of the set: the row's unless typical_p removed it
        if (typ_on && (eps_on || eta_on)) {
            m2 = -INFINITY;
            for (int i = tid; i < V; i += SMP_THREADS) {
                const float z = zof(i);
                if (kept(z)) m2 = fmaxf(m2, z);
            }
            m2 = block_max(L, m2);
        }
        if (eps_on) {
            const float Ze = kept_mass(nullptr);
            key_lo = max(key_lo, smp_floor_key(fminf(mx + logf(rq.epsilon * Ze), m2)));
        }
        if (eta_on) {
            float Sh;
            const float Zh = kept_mass(&Sh);
            const float H = logf(Zh) - Sh / Zh;
            const float cut = fminf(rq.eta, sqrtf(rq.eta) * __expf(-H));
            key_lo = max(key_lo, smp_floor_key(fminf(mx + logf(cut * Zh), m2)));
        }
        if (rq.n_kept) {
            if (tid == 0) L.hist_i[0] = 0;
            __syncthreads();
        }
    }
    // ---- draw: contiguous chunks of the vocabulary per thread, exclusive scan of the chunk sums, the owning thread walks its chunk
    const int per = (V + SMP_THREADS - 1) / SMP_THREADS;
    const int c0 = tid * per, c1 = min(V, c0 + per);
    float csum = 0.f;
    int ckept = 0;
    for (int i = c0; i < c1; ++i) {
        const float z = zof(i);
        const bool k = kept(z);
        csum += k ? __expf(z - mx) : 0.f;
        if constexpr (EXT) ckept += (k && z > -INFINITY) ? 1 : 0;
    }
    L.scan_f[tid] = csum;
    if constexpr (EXT) {
        if (rq.n_kept) {                            // integer adds: any order gives the same count
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) ckept += __shfl_xor(ckept, o, 64);
            if (lane == 0 && ckept) atomicAdd(&L.hist_i[0], ckept);
        }
    }
    __syncthreads();
    if (tid < SMP_WAVES) {                          // 16 segment sums of 64 chunks each, sequential: a fixed order
        float t = 0.f;
        for (int j = 0; j < 64; ++j) t += L.scan_f[tid * 64 + j];
        L.red_f[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        float Z2 = 0.f;
        for (int w = 0; w < SMP_WAVES; ++w) Z2 += L.red_f[w];
        const unsigned int r = philox_first(rq.step, rq.crow, 0u, 0u, rq.seed_lo, rq.seed_hi);
        const float u = (float)(r >> 8) * (1.0f / 16777216.0f);
        const float target = u * Z2;
        // segment, then chunk, then (below) element: running sums in the same fixed order
        float run = 0.f;
        int seg = SMP_WAVES - 1;
        for (int w = 0; w < SMP_WAVES; ++w) {
            if (run + L.red_f[w] > target) { seg = w; break; }
            run += L.red_f[w];
        }
        if (seg == SMP_WAVES - 1 && !(run + L.red_f[seg] > target)) {     // rounding at the very end: fall back to the whole last segment
            run = 0.f;
            for (int w = 0; w < seg; ++w) run += L.red_f[w];
        }
        int ch = seg * 64 + 63, lastnz = -1;
        float run_nz = run;
        bool found = false;
        for (int j = 0; j < 64; ++j) {
            const float cs = L.scan_f[seg * 64 + j];
            if (run + cs > target) { ch = seg * 64 + j; found = true; break; }
            if (cs > 0.f) { lastnz = seg * 64 + j; run_nz = run; }
            run += cs;
        }
        if (!found && lastnz >= 0) {      // the chunk-by-chunk sum rounded below the segment sum: the segment's last kept element
            ch = lastnz;
            run = run_nz;
            found = true;
        }
        L.sh_u[0] = (unsigned int)ch;
        L.sh_u[1] = found ? 1u : 0u;
        L.sh_f[0] = run;
        L.sh_f[1] = target;
        if constexpr (LP) L.sh_f[2] = Z2;
        if constexpr (EXT) {
            if (rq.n_kept) rq.n_kept[b] = L.hist_i[0];
        }
    }
    __syncthreads();
    if (tid == (int)L.sh_u[0] || (!L.sh_u[1] && tid == 0)) {
        int tok = -1;
        if (L.sh_u[1] && tid == (int)L.sh_u[0]) {
            float run = L.sh_f[0];
            const float target = L.sh_f[1];
            for (int i = c0; i < c1; ++i) {
                const float z = zof(i);
                if (kept(z)) {
                    run += __expf(z - mx);
                    tok = i;                               // the last kept index seen: the answer if rounding leaves run == target
                    if (run > target) break;
                }
            }
        }
        if (tok < 0 && tid == 0) {                         // nothing exceeded the target (u x total rounded up to the total): last kept index
            for (int i = V - 1; i >= 0; --i)
                if (kept(zof(i))) { tok = i; break; }
        }
        if (tok >= 0) {                                    // every exit above ends here with its tok: one place commits it
            float raw = 0.f, warped = 0.f;
            if constexpr (LP) {
                raw = (DT<T>::ld(row + tok) - xs) - logf(Zraw);
                warped = (zof(tok) - mx) - logf(L.sh_f[2]);
            }
            commit_token<LP>(sk, b, tok, rq.col, raw, warped);
        }
    }
}

// The sampling kernel, one workgroup per row, templated on where row b's request comes from:
//   SMP_STATE      gar_sample / gar_sample_lp: one request for all rows out of the state's words — params [3] = {temperature, top_p,
//                  top_k}, seed_dev [1]; step = col = step_dev[0], counter row = row_offset + b;
//   SMP_STATE_EXT  gar_sample_ext: the same with params [8] = {temperature, top_p, top_k, 0, min_p, typical_p, epsilon_cutoff,
//                  eta_cutoff} and the nullable n_kept [B]: sample_row's EXT instantiation;
//   SMP_ROWS       gar_sample_rows: every row its own request, out of row_words [B][8] = {mode, temperature bits, top_p bits, top_k,
//                  seed low, seed high, col0, counter row}. The column is the shared step_dev[0]; the row's step is its distance from
//                  col0. Mode 0 picks the largest logit as stored in am_better's order (gar_argmax's token) with the row's own
//                  workgroup and draws nothing. The branch on the mode is uniform over the workgroup (one word per row), so the
//                  barriers of either side are reached by all of its threads or by none.
enum { SMP_STATE, SMP_STATE_EXT, SMP_ROWS };

struct SmpSource {
    const int32_t* step_dev;            // NULL: column 0
    const float* params;                // SMP_STATE, SMP_STATE_EXT
    const int64_t* seed_dev;
    int row_offset;
    int32_t* n_kept;                    // SMP_STATE_EXT
    const int32_t* row_words;           // SMP_ROWS
};

template <typename T, bool LP, int SRC>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const T* __restrict__ logits, int64_t ld, int V, SmpSource src,
                                                             PickSink sk) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const T* row = logits + (int64_t)b * ld;
    const int col = src.step_dev ? src.step_dev[0] : 0;
    SmpReq rq;
    if constexpr (SRC == SMP_ROWS) {
        __shared__ float gv[SMP_WAVES];
        __shared__ int gi[SMP_WAVES];
        const int32_t* w = src.row_words + (int64_t)b * 8;
        if (w[0] == 0) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int i = tid; i < V; i += SMP_THREADS) am_better(bv, bi, DT<T>::ld(row + i), i);
            wave_best(bv, bi);
            if ((tid & 63) == 0) { gv[tid >> 6] = bv; gi[tid >> 6] = bi; }
            __syncthreads();
            if (tid == 0) {
                for (int k = 1; k < SMP_WAVES; ++k) am_better(bv, bi, gv[k], gi[k]);
                commit_token<false>(sk, b, bi, col, 0.f, 0.f);
            }
            return;
        }
        rq = {__int_as_float(w[1]), __int_as_float(w[2]), w[3], (unsigned int)w[4], (unsigned int)w[5],
              (unsigned int)max(0, col - w[6]), (unsigned int)w[7], col};
    } else {
        const unsigned long long seed = (unsigned long long)src.seed_dev[0];
        rq = {src.params[0], src.params[1], (int)src.params[2], (unsigned int)seed, (unsigned int)(seed >> 32), (unsigned int)col,
              (unsigned int)(b + src.row_offset), col};
        if constexpr (SRC == SMP_STATE_EXT) {
            rq.min_p = src.params[4];
            rq.typical_p = src.params[5];
            rq.epsilon = src.params[6];
            rq.eta = src.params[7];
            rq.n_kept = src.n_kept;
        }
    }
    sample_row<T, LP, SRC == SMP_STATE_EXT>(row, V, b, rq, sk);
}

template <bool LP, int SRC>
static int sample_launch(const char* who, int dtype, const void* logits, int64_t ld, int B, int V, const SmpSource& src,
                         const PickSink& sk, gar_stream_t stream) {
    GAR_CHECK_ARG(logits && B > 0 && V > 0 && (SRC == SMP_ROWS ? src.row_words != nullptr
                                                               : src.params && src.seed_dev && src.row_offset >= 0),
                  "%s: bad args", who);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GAR_BF16)
        hipLaunchKernelGGL((sample_kernel<bf16_t, LP, SRC>), dim3(B), dim3(SMP_THREADS), 0, s, (const bf16_t*)logits, ld, V, src, sk);
    else
        hipLaunchKernelGGL((sample_kernel<float, LP, SRC>), dim3(B), dim3(SMP_THREADS), 0, s, (const float*)logits, ld, V, src, sk);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

extern "C" int gar_sample(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens, int64_t out_stride,
                          const int32_t* step_dev, int64_t* cur_tokens, const float* params_dev, const int64_t* seed_dev,
                          const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, int row_offset,
                          gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "sample", false, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, nullptr, nullptr))
        return e;
    return sample_launch<false, SMP_STATE>("sample", dtype, logits, ld, B, V, {step_dev, params_dev, seed_dev, row_offset, nullptr, nullptr},
                                           sk, stream);
}

extern "C" int gar_sample_lp(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens, int64_t out_stride,
                             const int32_t* step_dev, int64_t* cur_tokens, const float* params_dev, const int64_t* seed_dev,
                             const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, int row_offset,
                             float* lp_raw, float* lp_warped, gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "sample_lp", true, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, lp_raw, lp_warped))
        return e;
    return sample_launch<true, SMP_STATE>("sample_lp", dtype, logits, ld, B, V, {step_dev, params_dev, seed_dev, row_offset, nullptr, nullptr},
                                          sk, stream);
}

// the host picks LP by the planes
extern "C" int gar_sample_ext(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens, int64_t out_stride,
                              const int32_t* step_dev, int64_t* cur_tokens, const float* params_dev, const int64_t* seed_dev,
                              const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, int row_offset,
                              float* lp_raw, float* lp_warped, int32_t* n_kept, gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "sample_ext", false, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, lp_raw, lp_warped))
        return e;
    const SmpSource src = {step_dev, params_dev, seed_dev, row_offset, n_kept, nullptr};
    return lp_raw || lp_warped ? sample_launch<true, SMP_STATE_EXT>("sample_ext", dtype, logits, ld, B, V, src, sk, stream)
                               : sample_launch<false, SMP_STATE_EXT>("sample_ext", dtype, logits, ld, B, V, src, sk, stream);
}

extern "C" int gar_sample_rows(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens, int64_t out_stride,
                               const int32_t* step_dev, int64_t* cur_tokens, const int32_t* row_words, const int64_t* eos_ids,
                               int n_eos, int32_t* finished, int32_t* done_count, gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "sample_rows", false, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, nullptr, nullptr))
        return e;
    return sample_launch<false, SMP_ROWS>("sample_rows", dtype, logits, ld, B, V, {step_dev, nullptr, nullptr, 0, nullptr, row_words}, sk,
                                          stream);
}

// workspace: pv | pi (gar_argmax), pv | pi | ps (gar_argmax_lp), AM_BLOCKS entries per row each
template <bool LP>
static int argmax_launch(const char* who, int dtype, const void* logits, int64_t ld, int B, int V, const int32_t* step_dev,
                         void* workspace, const PickSink& sk, gar_stream_t stream) {
    GAR_CHECK_ARG(logits && workspace && B > 0 && V > 0, "%s: bad args", who);
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + (int64_t)B * AM_BLOCKS);
    float* ps = LP ? pv + (int64_t)B * AM_BLOCKS * 2 : nullptr;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(AM_BLOCKS, B);
    if (dtype == GAR_BF16)
        hipLaunchKernelGGL((argmax_partial_kernel<bf16_t, LP>), grid, dim3(256), 0, s, (const bf16_t*)logits, ld, V, pv, pi, ps);
    else
        hipLaunchKernelGGL((argmax_partial_kernel<float, LP>), grid, dim3(256), 0, s, (const float*)logits, ld, V, pv, pi, ps);
    hipLaunchKernelGGL(argmax_final_kernel<LP>, dim3(B), dim3(64), 0, s, pv, pi, ps, sk.out_tokens, sk.out_stride, step_dev, sk.cur_tokens,
                       sk.eos_ids, sk.n_eos, sk.finished, sk.done_count, sk.lp_raw, sk.lp_warped);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

extern "C" int64_t gar_argmax_workspace(int B, int V) {
    (void)V;
    return (int64_t)B * AM_BLOCKS * 8;
}

extern "C" int gar_argmax(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens,
                          int64_t out_stride, const int32_t* step_dev, int64_t* cur_tokens, void* workspace,
                          const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "argmax", false, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, nullptr, nullptr))
        return e;
    return argmax_launch<false>("argmax", dtype, logits, ld, B, V, step_dev, workspace, sk, stream);
}

extern "C" int64_t gar_argmax_lp_workspace(int B, int V) {
    (void)V;
    return (int64_t)B * AM_BLOCKS * 12;
}

extern "C" int gar_argmax_lp(int dtype, const void* logits, int64_t ld, int B, int V, int64_t* out_tokens,
                             int64_t out_stride, const int32_t* step_dev, int64_t* cur_tokens, void* workspace,
                             const int64_t* eos_ids, int n_eos, int32_t* finished, int32_t* done_count, float* lp_raw,
                             float* lp_warped, gar_stream_t stream) {
    PickSink sk;
    if (int e = pick_sink(sk, "argmax_lp", true, out_tokens, out_stride, cur_tokens, eos_ids, n_eos, finished, done_count, lp_raw, lp_warped))
        return e;
    return argmax_launch<true>("argmax_lp", dtype, logits, ld, B, V, step_dev, workspace, sk, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// top-k / candidate log-probabilities of a step's logits (gar_topk_lp): lp[i] = x[i] - logsumexp(x[0:V]), the k largest entries in
// the order (value descending, index ascending) — am_better's order, so entry 0 is gar_argmax's token — and lp at a fixed id list.
// Both stages select by k rounds of block arg-max. Nothing is removed between rounds: round r takes the best element that comes
// strictly AFTER round r-1's winner in that order (tk_after), so the elements stay untouched in registers (static indexing, no
// scratch), ties and -inf logits keep their index order, and an exhausted block answers (-inf, TK_NONE) from then on.
// Stage 1, grid (AM_BLOCKS, B): a block's ~V/64 logits in TK_ITEMS registers per thread (ITEMS = 0: V > 64 x 256 x TK_ITEMS, re-read
// from the cache every round), its k best, and sum exp(x - block max) by argmax_partial_kernel<T, true>'s block_exp_sums. Stage 2, one
// block per row: the 64 (max, sum) pairs merged by argmax_final_kernel<true>'s merge_exp_sums — entry 0's value is gar_argmax_lp's
// lp_raw bit for bit — the 64 x k candidates selected the same way, the candidate ids gathered from the row. Fixed-shape reductions
// (xor tree in a wave, waves in order), no atomics: deterministic.
// ---------------------------------------------------------------------------------------------------------------
#define TK_MAX 32
#define TK_CAND_MAX 64
#define TK_ITEMS 8
#define TK_NONE 0x7fffffff

__device__ __forceinline__ bool tk_after(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }

// k rounds of block arg-max over what the 256 threads hold. local(pv, pi, v, i): the calling thread's best element strictly after
// (pv, pi), (-inf, TK_NONE) when it has none left; emit(r, v, i): called by every thread with round r's winner. A thread's best
// changes only when it held the last winner, and a wave's only when that thread is in it: every round one thread rescans its
// elements and one wave redoes its xor tree; the other waves hand their standing best to the round's LDS slots. sv / si alternate
// between two sets of 4 slots, so one barrier per round is enough (a set is rewritten two rounds later, behind the next barrier).
template <typename Local, typename Emit>
__device__ __forceinline__ void tk_select(int k, float (*sv)[4], int (*si)[4], Local local, Emit emit) {
    const int wave = threadIdx.x >> 6;
    float lv, wv;
    int li, wi;
    auto wave_of_local = [&]() { wv = lv; wi = li; wave_best(wv, wi); };
    local(INFINITY, -1, lv, li);
    wave_of_local();
    for (int r = 0; r < k; ++r) {
        if ((threadIdx.x & 63) == 0) { sv[r & 1][wave] = wv; si[r & 1][wave] = wi; }
        __syncthreads();
        float bv = sv[r & 1][0];
        int bi = si[r & 1][0], bw = 0;
        for (int w = 1; w < 4; ++w) {
            const float v = sv[r & 1][w];
            const int i = si[r & 1][w];
            if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; bw = w; }
        }
        emit(r, bv, bi);
        if (bi == TK_NONE) {                    // fewer than k elements here (uniform: every thread holds the same bi)
            for (++r; r < k; ++r) emit(r, -INFINITY, TK_NONE);
            break;
        }
        if (bw == wave) {
            if (li == bi) local(bv, bi, lv, li);
            wave_of_local();
        }
    }
}

template <typename T, int ITEMS>
__global__ __launch_bounds__(256) void topk_lp_partial_kernel(const T* __restrict__ logits, int64_t ld, int V, int k,
                                                              float* __restrict__ cv, int* __restrict__ ci,
                                                              float* __restrict__ ps) {
    __shared__ float sv[2][4];
    __shared__ int si[2][4];
    __shared__ float ss[4];
    __shared__ float rv[TK_MAX];                // the rounds' winners, stored together behind the loop
    __shared__ int ri[TK_MAX];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const T* row = logits + (int64_t)b * ld;
    const int per = (V + AM_BLOCKS - 1) / AM_BLOCKS;
    const int lo = blk * per, hi = min(V, lo + per);
    float x[ITEMS > 0 ? ITEMS : 1];
    if constexpr (ITEMS > 0) {
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int i = lo + tid + 256 * j;
            x[j] = i < hi ? DT<T>::ld(row + i) : -INFINITY;
        }
    }
    float* ov = cv + ((int64_t)b * AM_BLOCKS + blk) * k;
    int* oi = ci + ((int64_t)b * AM_BLOCKS + blk) * k;
    float m0 = -INFINITY;
    tk_select(
        k, sv, si,
        [&](float pv, int pi, float& bv, int& bi) {
            bv = -INFINITY;
            bi = TK_NONE;
            if constexpr (ITEMS > 0) {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) {
                    const int i = lo + tid + 256 * j;
                    if (i < hi && tk_after(x[j], i, pv, pi)) am_better(bv, bi, x[j], i);
                }
            } else {
                for (int i = lo + tid; i < hi; i += 256) {
                    const float v = DT<T>::ld(row + i);
                    if (tk_after(v, i, pv, pi)) am_better(bv, bi, v, i);
                }
            }
        },
        [&](int r, float v, int i) {
            if (r == 0) m0 = v;
            if (tid == 0) { rv[r] = v; ri[r] = i; }
        });
    block_exp_sums(m0, ss, [&](auto f) {
        if constexpr (ITEMS > 0) {
#pragma unroll
            for (int j = 0; j < ITEMS; ++j)
                if (lo + tid + 256 * j < hi) f(x[j]);
        } else {
            for (int i = lo + tid; i < hi; i += 256) f(DT<T>::ld(row + i));
        }
    });
    if (tid < k) { ov[tid] = rv[tid]; oi[tid] = ri[tid]; }
    if (tid == 0) ps[b * AM_BLOCKS + blk] = block_exp_sum4(ss);
}

// kw = the k of stage 1 (>= 1: the row maximum is its entry 0 also when only candidates are asked for), k = entries to write (0: none)
template <typename T>
__global__ __launch_bounds__(256) void topk_lp_final_kernel(const T* __restrict__ logits, int64_t ld, int V, int k, int kw,
                                                            const float* __restrict__ cv, const int* __restrict__ ci,
                                                            const float* __restrict__ ps, int32_t* __restrict__ top_ids,
                                                            float* __restrict__ top_lp, int64_t top_row_stride,
                                                            int64_t top_step_stride, const int32_t* __restrict__ cand_ids,
                                                            int n_cand, float* __restrict__ cand_lp, int64_t cand_row_stride,
                                                            int64_t cand_step_stride, const int32_t* __restrict__ step_dev) {
    __shared__ float sv[2][4];
    __shared__ int si[2][4];
    __shared__ float sms[2];
    __shared__ float rv[TK_MAX];
    __shared__ int ri[TK_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = step_dev ? step_dev[0] : 0;
    cv += (int64_t)b * AM_BLOCKS * kw;
    ci += (int64_t)b * AM_BLOCKS * kw;
    if (tid < 64) {                             // the row's (max, sum exp(x - max)) out of the 64 blocks'
        const float mv = cv[tid * kw];
        const float M = wave_max(mv);
        const float s = merge_exp_sums(mv, M, &ps[b * AM_BLOCKS + tid]);
        if (tid == 0) { sms[0] = M; sms[1] = logf(s); }
    }
    __syncthreads();
    const float M = sms[0], logS = sms[1];
    if (k > 0) {
        const int n = AM_BLOCKS * kw;           // <= 64 x 32 = 256 x TK_ITEMS
        float x[TK_ITEMS];
        int xi[TK_ITEMS];
#pragma unroll
        for (int j = 0; j < TK_ITEMS; ++j) {
            const int e = tid + 256 * j;
            x[j] = e < n ? cv[e] : -INFINITY;
            xi[j] = e < n ? ci[e] : TK_NONE;
        }
        int32_t* oid = top_ids + (int64_t)b * top_row_stride + (int64_t)step * top_step_stride;
        float* olp = top_lp + (int64_t)b * top_row_stride + (int64_t)step * top_step_stride;
        tk_select(
            k, sv, si,
            [&](float pv, int pi, float& bv, int& bi) {
                bv = -INFINITY;
                bi = TK_NONE;
#pragma unroll
                for (int j = 0; j < TK_ITEMS; ++j)
                    if (xi[j] != TK_NONE && tk_after(x[j], xi[j], pv, pi)) am_better(bv, bi, x[j], xi[j]);
            },
            [&](int r, float v, int i) {
                if (tid == 0) { rv[r] = v; ri[r] = i; }
            });
        __syncthreads();
        if (tid < k) {                          // k <= V: the row holds k elements, so every ri is one of them
            oid[tid] = ri[tid];
            olp[tid] = (rv[tid] - M) - logS;
        }
    }
    if (cand_lp && tid < n_cand) {
        const int id = cand_ids[tid];           // the caller checked the list; an id outside the row is not read
        const float lp = (id >= 0 && id < V) ? (DT<T>::ld(logits + (int64_t)b * ld + id) - M) - logS : __builtin_nanf("");
        cand_lp[(int64_t)b * cand_row_stride + (int64_t)step * cand_step_stride + tid] = lp;
    }
}

extern "C" int64_t gar_topk_lp_workspace(int B, int V, int k) {
    (void)V;
    return (int64_t)B * AM_BLOCKS * (2 * (k > 1 ? k : 1) + 1) * 4;
}

extern "C" int gar_topk_lp(int dtype, const void* logits, int64_t ld, int B, int V, int k, int32_t* top_ids, float* top_lp,
                           int64_t top_row_stride, int64_t top_step_stride, const int32_t* cand_ids, int n_cand, float* cand_lp,
                           int64_t cand_row_stride, int64_t cand_step_stride, const int32_t* step_dev, void* workspace,
                           gar_stream_t stream) {
    GAR_CHECK_ARG(logits && workspace && B > 0 && V > 0 && ld >= V, "topk_lp: bad args");
    GAR_CHECK_ARG((top_ids != nullptr) == (top_lp != nullptr), "topk_lp: top_ids and top_lp go together");
    GAR_CHECK_ARG(top_ids || cand_lp, "topk_lp: neither the top-k planes nor the candidate plane");
    if (top_ids)
        GAR_CHECK_ARG(k >= 1 && k <= TK_MAX && k <= V && top_step_stride >= k && top_row_stride >= top_step_stride,
                      "topk_lp: k %d not in 1..min(%d, V = %d), or strides below k", k, TK_MAX, V);
    else
        GAR_CHECK_ARG(k == 0, "topk_lp: k %d without the top-k planes", k);
    if (cand_lp)
        GAR_CHECK_ARG(cand_ids && n_cand >= 1 && n_cand <= TK_CAND_MAX && cand_step_stride >= n_cand && cand_row_stride >= cand_step_stride,
                      "topk_lp: %d candidates not in 1..%d, no id list, or strides below the count", n_cand, TK_CAND_MAX);
    else
        GAR_CHECK_ARG(n_cand == 0, "topk_lp: %d candidates without the candidate plane", n_cand);
    const int kw = k > 1 ? k : 1;
    float* cv = (float*)workspace;
    int* ci = (int*)(cv + (int64_t)B * AM_BLOCKS * kw);
    float* ps = cv + (int64_t)B * AM_BLOCKS * kw * 2;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(AM_BLOCKS, B);
    const bool regs = (int64_t)V <= (int64_t)AM_BLOCKS * 256 * TK_ITEMS;
#define LAUNCH_TK(TT)                                                                                                              \
    do {                                                                                                                           \
        if (regs)                                                                                                                  \
            hipLaunchKernelGGL((topk_lp_partial_kernel<TT, TK_ITEMS>), grid, dim3(256), 0, s, (const TT*)logits, ld, V, kw, cv, ci, ps); \
        else                                                                                                                       \
            hipLaunchKernelGGL((topk_lp_partial_kernel<TT, 0>), grid, dim3(256), 0, s, (const TT*)logits, ld, V, kw, cv, ci, ps);  \
        hipLaunchKernelGGL((topk_lp_final_kernel<TT>), dim3(B), dim3(256), 0, s, (const TT*)logits, ld, V, k, kw, cv, ci, ps,     \
                           top_ids, top_lp, top_row_stride, top_step_stride, cand_ids, n_cand, cand_lp, cand_row_stride,           \
                           cand_step_stride, step_dev);                                                                            \
    } while (0)
    if (dtype == GAR_BF16) LAUNCH_TK(bf16_t); else LAUNCH_TK(float);
#undef LAUNCH_TK
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Logits processors of a step (gar_logits_process): HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
// NoBadWordsLogitsProcessor, MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor and
// SuppressTokensAtBeginLogitsProcessor over a row's own generated tokens (out_tokens[b][0:t], t = step_dev[0]), as sparse edits of
// the row in place before the pick. One 1024-thread workgroup per row and two bitmaps over the vocabulary in LDS (2 x 4 bytes per
// 32 ids: 32 KB at V = 128256): phase 1 marks — history ids into `pen` (LDS atomic OR: a token that occurs a hundred times sets one
// bit), every banned id into `ban`; phase 2, behind one barrier, gives each thread bitmap words of its own, so every marked entry is
// read once (the value stored before the launch), computed once and written once by exactly one thread: no compounding, no two
// writers. Unmarked entries and the columns V..ld-1 are never touched. The bans are -inf and a penalised -inf stays -inf, so HF's
// list order among these processors does not show in the result. Every read of the parameter block is bounded by params_words,
// every read of the history by out_cols, every marked id by V.
// ---------------------------------------------------------------------------------------------------------------
#define LP_THREADS 1024
#define LP_HEADER 8                 // params: [penalty f32 bits, n, m, n_suppress, n_begin, n_bad, n_bad_tokens, col0] then the lists
#define LP_COL0 7                   // gar_logits_process_rows only: the token column of the row's step 0 (gar_logits_process never reads it)
#define LP_MAX_VOCAB 262144         // two bitmaps in 64 KB of LDS

// One row under one parameter block — the body of both entry points, run by the row's whole workgroup: `row` the row's logits, `hist`
// its t generated tokens (never dereferenced at t = 0), `params` its block, read within params_words. gar_logits_process hands every
// row the call's one block and the history at columns 0 .. t-1; gar_logits_process_rows hands row b its own block and the history
// that starts at the block's col0.
template <typename T>
__device__ __forceinline__ void logits_process_row(T* __restrict__ row, int V, const int64_t* __restrict__ hist, int t,
                                                   const int64_t* __restrict__ eos_ids, int n_eos,
                                                   const int32_t* __restrict__ params, int params_words) {
    extern __shared__ unsigned int lp_bits[];
    const int W = (V + 31) >> 5;
    unsigned int* pen = lp_bits;
    unsigned int* ban = lp_bits + W;
    const int tid = threadIdx.x;
    for (int w = tid; w < 2 * W; w += LP_THREADS) lp_bits[w] = 0u;
    const float p = __int_as_float(params[0]);
    const int n = params[1], m = params[2];
    int n_sup = params[3], n_beg = params[4], n_bad = params[5], n_bt = params[6];
    // the lists, in this order behind the header; a block that does not fit its buffer names no list
    const bool lists_ok = n_sup >= 0 && n_beg >= 0 && n_bad >= 0 && n_bt >= 0 &&
                          (int64_t)LP_HEADER + n_sup + n_beg + (n_bad ? n_bad + 1 : 0) + n_bt <= (int64_t)params_words;
    if (!lists_ok) n_sup = n_beg = n_bad = n_bt = 0;
    const int32_t* sup = params + LP_HEADER;
    const int32_t* beg = sup + n_sup;
    const int32_t* bad_off = beg + n_beg;           // n_bad + 1 offsets into bad_tok
    const int32_t* bad_tok = bad_off + (n_bad ? n_bad + 1 : 0);
    __syncthreads();
    auto mark = [&](unsigned int* bits, int64_t id) {
        if (id >= 0 && id < V) atomicOr(&bits[id >> 5], 1u << (id & 31));
    };
    if (p != 1.0f)
        for (int j = tid; j < t; j += LP_THREADS) mark(pen, hist[j]);
    if (n > 0 && t + 1 >= n)                        // an n-gram of the history whose first n - 1 tokens are the history's last n - 1
        for (int j = tid; j + n <= t; j += LP_THREADS) {
            bool same = true;
            for (int k = 0; k < n - 1 && same; ++k) same = hist[j + k] == hist[t - n + 1 + k];
            if (same) mark(ban, hist[j + n - 1]);
        }
    if (t < m)
        for (int e = tid; e < n_eos; e += LP_THREADS) mark(ban, eos_ids[e]);
    for (int i = tid; i < n_sup; i += LP_THREADS) mark(ban, sup[i]);
    if (t == 0)
        for (int i = tid; i < n_beg; i += LP_THREADS) mark(ban, beg[i]);
    for (int e = tid; e < n_bad; e += LP_THREADS) {
        const int o0 = bad_off[e], o1 = bad_off[e + 1], L = o1 - o0;
        if (o0 < 0 || L < 1 || o1 > n_bt) continue;
        if (L == 1) { mark(ban, bad_tok[o0]); continue; }
        if (L > t) continue;                        // HF's SequenceBiasLogitsProcessor skips an entry longer than the context
        bool same = true;
        for (int k = 0; k < L - 1 && same; ++k) same = hist[t - (L - 1) + k] == (int64_t)bad_tok[o0 + k];
        if (same) mark(ban, bad_tok[o1 - 1]);
    }
    __syncthreads();
    for (int w = tid; w < W; w += LP_THREADS) {
        const unsigned int bw = ban[w];
        unsigned int bits = pen[w] | bw;
        while (bits) {
            const int bit = __ffs(bits) - 1;
            bits &= bits - 1;
            const int i = (w << 5) + bit;           // < V: mark() set no bit at or past V
            if ((bw >> bit) & 1u) {
                DT<T>::st(row + i, -INFINITY);
            } else {
                const float x = DT<T>::ld(row + i);
                DT<T>::st(row + i, x < 0.f ? x * p : x / p);        // HF: where(x < 0, x * p, x / p) — a true division
            }
        }
    }
}

// ROWS = false (gar_logits_process): one block for every row, a row's step is the shared step and its history starts at column 0.
// ROWS = true (gar_logits_process_rows, ContinuousBatcher(processing=True)): params is [B][params_words], row b its own block. A block
// whose word 0 is 0 — no penalty's f32 bits are: pack() writes a penalty > 0 — is a row without a request, left before anything is
// read or written (one word, the same for the whole workgroup, in front of the body's barriers). Word LP_COL0 is the column of the
// token matrix at which the row's step 0 was written: with the shared column c the row's step is c - col0 and its history
// out_tokens[b][col0 .. c-1]; columns in front of col0 belong to retired captions and are never read.
template <typename T, bool ROWS>
__global__ __launch_bounds__(LP_THREADS) void logits_process_kernel(T* __restrict__ logits, int64_t ld, int V,
                                                                    const int64_t* __restrict__ out_tokens, int64_t out_stride,
                                                                    int out_cols, const int32_t* __restrict__ step_dev,
                                                                    const int64_t* __restrict__ eos_ids, int n_eos,
                                                                    const int32_t* __restrict__ params, int params_words) {
    const int b = blockIdx.x;
    if (ROWS) {
        params += (int64_t)b * params_words;
        if (params[0] == 0) return;
    }
    int t = step_dev ? step_dev[0] : 0;
    t = out_tokens ? max(0, min(t, out_cols)) : 0;
    const int64_t* hist = out_tokens + (int64_t)b * out_stride;
    if (ROWS) {
        const int col0 = max(0, min(params[LP_COL0], t));
        hist += col0;
        t -= col0;
    }
    logits_process_row<T>(logits + (int64_t)b * ld, V, hist, t, eos_ids, n_eos, params, params_words);
}

extern "C" int gar_logits_process_max_vocab(void) { return LP_MAX_VOCAB; }

template <bool ROWS>
static int logits_process_launch(const char* who, int dtype, void* logits, int64_t ld, int B, int V, const int64_t* out_tokens,
                                 int64_t out_stride, int out_cols, const int32_t* step_dev, const int64_t* eos_ids, int n_eos,
                                 const int32_t* params_dev, int params_words, gar_stream_t stream) {
    GAR_CHECK_ARG(logits && params_dev && B > 0 && V > 0 && ld >= V, "%s: bad args", who);
    GAR_CHECK_ARG(V <= LP_MAX_VOCAB, "%s: V %d above %d (two vocabulary bitmaps in 64 KB of LDS)", who, V, LP_MAX_VOCAB);
    GAR_CHECK_ARG(params_words >= LP_HEADER, "%s: a parameter block of %d words, the header alone has %d", who, params_words, LP_HEADER);
    GAR_CHECK_ARG(!out_tokens || (out_cols >= 0 && out_stride >= out_cols), "%s: out_cols %d / out_stride %lld", who, out_cols,
                  (long long)out_stride);
    GAR_CHECK_ARG(n_eos >= 0 && (n_eos == 0 || eos_ids), "%s: eos_ids", who);
    const size_t lds = (size_t)((V + 31) >> 5) * 8;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == GAR_BF16)
        hipLaunchKernelGGL((logits_process_kernel<bf16_t, ROWS>), dim3(B), dim3(LP_THREADS), lds, s, (bf16_t*)logits, ld, V, out_tokens,
                           out_stride, out_cols, step_dev, eos_ids, n_eos, params_dev, params_words);
    else
        hipLaunchKernelGGL((logits_process_kernel<float, ROWS>), dim3(B), dim3(LP_THREADS), lds, s, (float*)logits, ld, V, out_tokens,
                           out_stride, out_cols, step_dev, eos_ids, n_eos, params_dev, params_words);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

extern "C" int gar_logits_process(int dtype, void* logits, int64_t ld, int B, int V, const int64_t* out_tokens, int64_t out_stride,
                                  int out_cols, const int32_t* step_dev, const int64_t* eos_ids, int n_eos,
                                  const int32_t* params_dev, int params_words, gar_stream_t stream) {
    return logits_process_launch<false>("logits_process", dtype, logits, ld, B, V, out_tokens, out_stride, out_cols, step_dev, eos_ids,
                                        n_eos, params_dev, params_words, stream);
}

extern "C" int gar_logits_process_rows(int dtype, void* logits, int64_t ld, int B, int V, const int64_t* out_tokens,
                                       int64_t out_stride, int out_cols, const int32_t* step_dev, const int64_t* eos_ids, int n_eos,
                                       const int32_t* row_params, int row_words, gar_stream_t stream) {
    return logits_process_launch<true>("logits_process_rows", dtype, logits, ld, B, V, out_tokens, out_stride, out_cols, step_dev,
                                       eos_ids, n_eos, row_params, row_words, stream);
}
