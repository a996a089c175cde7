// Caption scoring (GARModel.score / forward(mode="loss")): the combine step behind the lm_head. HF's causal-LM loss takes
// log_softmax over the f32 upcast of the logits the model dtype holds; per scored row r, with target t = targets[r]:
//   logprob = logit[t] - logsumexp(logits)
// written to token_logprobs[dest[r]] and accumulated into sum_logprobs[dest[r] / S] and n_tokens[dest[r] / S].
// Two forms of the row's logits:
//   partials  (gar_lm_head_xent): `strips` pairs (max, sum exp(x - max)) per row and the target logit — merged here;
//   dense     ([R, ld] logits of gar_gemm, R <= 64 rows per launch or the f32 parity mode): reduced here over V in one
//             pass with a running (max, sum) per lane, 16-byte loads when the rows are 16-byte aligned.
// One wave per row. Ignored rows: target == -100; a target outside [0, V) otherwise is ignored too and sets
// GAR_SCORE_LABEL_RANGE in flags[0] (no fault, no host sync: what validate=False reports).
#include "common.h"

template <typename T, bool DENSE, bool VEC = false>
__global__ __launch_bounds__(256) void xent_combine_kernel(const float2* __restrict__ part, int strips,
                                                           const float* __restrict__ tgt_logit, const T* __restrict__ logits,
                                                           int64_t ld, int R, int V, const int32_t* __restrict__ targets,
                                                           const int32_t* __restrict__ dest, int S, float* __restrict__ out,
                                                           float* __restrict__ sum_lp, int32_t* __restrict__ n_tok,
                                                           int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int t = targets[r];
    if (t == -100) return;
    if (t < 0 || t >= V) {
        if (lane == 0 && flags) atomicOr(flags, GAR_SCORE_LABEL_RANGE);
        return;
    }
    float mx = -INFINITY, se = 0.f, xt;
    if (DENSE) {
        const T* row = logits + (int64_t)r * ld;
        // running (max, sum exp(x - max)) per lane: a group's max first, the sum rescaled when the max rises
        auto add = [&](const float* x, int n) {
            float gm = -INFINITY;
            for (int e = 0; e < n; ++e) gm = fmaxf(gm, x[e]);
            if (gm > mx) {
                se *= expf(mx - gm);
                mx = gm;
            }
            if (mx == -INFINITY) return;
            for (int e = 0; e < n; ++e) se += expf(x[e] - mx);
        };
        int v0 = 0;
        if (VEC) {
            for (int v = lane * 8; v + 8 <= V; v += 512) {
                float x[8];
                ld8(row + v, x);
                add(x, 8);
            }
            v0 = V & ~7;
        }
        for (int v = v0 + lane; v < V; v += 64) {
            const float x = DT<T>::ld(row + v);
            add(&x, 1);
        }
        const float m = wave_max(mx);
        se = wave_sum(mx == -INFINITY ? 0.f : se * expf(mx - m));
        mx = m;
        xt = DT<T>::ld(row + t);
    } else {
        const float2* pr = part + (int64_t)r * strips;
        for (int k = lane; k < strips; k += 64) mx = fmaxf(mx, pr[k].x);
        mx = wave_max(mx);
        for (int k = lane; k < strips; k += 64) {
            const float2 q = pr[k];
            if (q.y > 0.f) se += q.y * expf(q.x - mx);
        }
        se = wave_sum(se);
        xt = tgt_logit[r];
    }
    if (lane == 0) {
        const float lp = xt - (mx + logf(se));
        const int d = dest[r];
        out[d] = lp;
        atomicAdd(sum_lp + d / S, lp);
        atomicAdd(n_tok + d / S, 1);
    }
}

extern "C" int gar_xent_combine(int dtype, const float* partials, int strips, const float* target_logit, const void* logits,
                                int64_t ld, int R, int V, const int32_t* targets, const int32_t* dest, int S,
                                float* token_logprobs, float* sum_logprobs, int32_t* n_tokens, int32_t* flags,
                                gar_stream_t stream) {
    GAR_CHECK_ARG(dtype == GAR_F32 || dtype == GAR_BF16, "xent_combine: bad dtype");
    GAR_CHECK_ARG(targets && dest && token_logprobs && sum_logprobs && n_tokens, "xent_combine: null pointer");
    GAR_CHECK_ARG(R > 0 && V > 0 && S > 0, "xent_combine: bad shape (R %d, V %d, S %d)", R, V, S);
    const bool dense = logits != nullptr;
    GAR_CHECK_ARG(dense ? ld >= V : (partials && target_logit && strips > 0),
                  "xent_combine: pass the dense logits (ld >= V) or the partials and target logits");
    dim3 grid((R + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (!dense)
        hipLaunchKernelGGL((xent_combine_kernel<float, false>), grid, block, 0, s, (const float2*)partials, strips, target_logit,
                           (const float*)nullptr, ld, R, V, targets, dest, S, token_logprobs, sum_logprobs, n_tokens, flags);
    else {
        const int esz = dtype == GAR_BF16 ? 2 : 4;
        const bool vec = ((uintptr_t)logits & 15) == 0 && (ld * esz) % 16 == 0;
#define LAUNCH_DENSE(TT, VV)                                                                                                  \
    hipLaunchKernelGGL((xent_combine_kernel<TT, true, VV>), grid, block, 0, s, (const float2*)nullptr, 0, (const float*)nullptr, \
                       (const TT*)logits, ld, R, V, targets, dest, S, token_logprobs, sum_logprobs, n_tokens, flags)
        if (dtype == GAR_BF16) {
            if (vec) LAUNCH_DENSE(bf16_t, true); else LAUNCH_DENSE(bf16_t, false);
        } else {
            if (vec) LAUNCH_DENSE(float, true); else LAUNCH_DENSE(float, false);
        }
#undef LAUNCH_DENSE
    }
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}
