// Decode attention (q_len = 1): split-KV, GQA-aware, HBM-bound.
//
//   Block = 4 waves = one (split, kv head, batch). The G = Hq/Hkv query heads sharing a kv head are the columns of
//   the MFMA B operand (columns >= G are zero), so K and V of that kv head stream from HBM exactly ONCE per step.
//   The block's kv range is cut in 64-kv tiles dealt round-robin to its waves; each wave brings its K / V tiles — both
//   row-major [kv][HD], the cache's layout — into a private LDS region with `buffer_load ... lds` DMA, forms the QK^T
//   fragments with ds_read_b128 and the PV fragments (k = kv: a column of the V tile) with gfx950's transposing
//   ds_read_b64_tr_b16, keeps an online softmax, and the four waves are merged in LDS into one un-normalised partial
//   (m, l, O[G][HD]) per block. decode_combine_kernel merges the splits.
//   kv length comes from device memory so the captured hipGraph replays unchanged for every token.
//   Algorithmic bytes per launch: B * Hkv * kv_len * HD * 2 (K and V) * sizeof(bf16).
#include <stdlib.h>

#include "common.h"
#include "fp8.h"

__device__ __forceinline__ unsigned int cvt_pk_d(float lo, float hi) { return pack_bf2(lo, hi); }

typedef short tr4_d __attribute__((ext_vector_type(4)));
// PV A-operand fragment (rows = d, k = 8 consecutive kv) out of a row-major V tile in LDS: two transposing reads, each a
// [4 kv][16 d] block per 16-lane group (see attention_bf16.hip, VROW); `p` = this lane's chunk address for kv rows 0..3
__device__ __forceinline__ bf16x8 v_frag_tr(const char* p, int row4_bytes) {
    const tr4_d lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4_d*)(p));
    const tr4_d hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) tr4_d*)(p + row4_bytes));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---------------------------------------------------------------------------------------------------------------
// head_dim 64: every wave brings its 64-kv K / V tiles in with `buffer_load_dwordx4 ... lds` — 1 KiB per instruction,
// eight full 128-byte lines (per-lane fragment loads from global memory touch 32 different lines, 32 B each, per
// instruction: measured with the compute removed they top out at 3.3 TB/s). A wave owns a private 16 KiB LDS region
// (K tile | V tile, XOR-swizzled through the DMA source offsets like attention_bf16.hip): wait for tile t, pull its
// fragments into registers, immediately re-arm the region with the DMA of the wave's next tile, then compute on the
// registers — no block-level barrier in the loop.
// 64 KiB + merge buffer per block -> two blocks (8 waves) per CU, 128 KiB of loads in flight per CU.
// ---- gar_llm_qkv_post (S = 1) fused into the attention launch (gar_attention_decode_qkv) ------------------------------
// The step's raw qkv GEMM output [B, (Hq + 2 Hkv) HD] replaces Q: every block rotates and scales its G query heads while it
// loads them (a lane's MFMA fragments hold dims 16 kd + 8 h + e for all kd: both halves of every rotation pair), and the
// wave that owns the LAST kv tile rotates the new key, appends key and value to the caches (global rows `pos`) and patches
// them into its LDS tiles after the DMA of that tile has landed — the DMA may or may not have seen the global rows.
struct decode_qkv_args {
    const bf16_t* raw;          // NULL: plain gar_attention_decode (Q, caches already appended)
    const float* cs;
    const float* sn;            // [max_pos, HD / 2] f32
    float q_scale;
    int strip;                  // q / k head columns of `raw` in the fused RoPE epilogue's strip order (head_dim 128: dims
                                // [0..31, 64..95, 32..63, 96..127]; include/gar_hip.h GAR_EPI_QKV_ROPE_LLM) — the folded qkv weight's
};
template <int HD>
__device__ __forceinline__ int strip_col_d(int d0, bool strip) {
    if (HD != 128 || !strip) return d0;
    const int blk = d0 >> 5;
    return blk == 1 ? d0 + 32 : (blk == 2 ? d0 - 32 : d0);
}

template <int HD>
__device__ __forceinline__ void load_q_rotated(bf16x8 (&qf)[HD / 16], const decode_qkv_args& fa, int b, int Hq, int Hkv, int head,
                                               bool valid, int h, int rp) {
    constexpr int HALF = HD / 2, NKD = HD / 16;
    const bf16_t* rq = fa.raw + ((int64_t)b * (Hq + 2 * Hkv) + head) * HD;
#pragma unroll
    for (int kd = 0; kd < NKD / 2; ++kd) {
        const int off = kd * 16 + h * 8;
        float x1[8], x2[8], c[8], sv[8];
        ld8(rq + strip_col_d<HD>(off, fa.strip), x1);
        ld8(rq + strip_col_d<HD>(HALF + off, fa.strip), x2);
        ld8(fa.cs + (int64_t)rp * HALF + off, c);
        ld8(fa.sn + (int64_t)rp * HALF + off, sv);
#pragma unroll
        for (int e = 0; e < 8; ++e) rope_half_pair(x1[e], x2[e], c[e], sv[e], fa.q_scale, x1[e], x2[e]);
        const u32x4 w1 = {pack_bf2(x1[0], x1[1]), pack_bf2(x1[2], x1[3]), pack_bf2(x1[4], x1[5]), pack_bf2(x1[6], x1[7])};
        const u32x4 w2 = {pack_bf2(x2[0], x2[1]), pack_bf2(x2[2], x2[3]), pack_bf2(x2[4], x2[5]), pack_bf2(x2[6], x2[7])};
        const u32x4 z = {0u, 0u, 0u, 0u};
        qf[kd] = __builtin_bit_cast(bf16x8, valid ? w1 : z);
        qf[kd + NKD / 2] = __builtin_bit_cast(bf16x8, valid ? w2 : z);
    }
}

// new key (rotated) and value row of (b, kvh) at cache row `pos`: global append + patch of the wave's LDS tiles (row pos & 63).
// KEYFN / VKEYFN: chunk swizzle of a K / V tile row (the kernels' DMA layouts). Lanes 0 .. HD/16-1 do the key (8 dims of each
// half), lanes 0 .. HD/8-1 the value.
template <int HD, bool DO_K, bool DO_V, typename KF, typename VF>
__device__ __forceinline__ void append_new_kv(const decode_qkv_args& fa, bf16_t* Kp, bf16_t* Vp, char* ks, char* vs, int b, int Hq,
                                              int Hkv, int kvh, int lane, int pos, int rp, KF kkey, VF vkey) {
    constexpr int HALF = HD / 2, RB = HD * 2;
    const int r = pos & 63;
    const bf16_t* row = fa.raw + (int64_t)b * (Hq + 2 * Hkv) * HD;
    if (DO_K && lane < HALF / 8) {
        const int i8 = lane * 8;
        const bf16_t* rk = row + (Hq + kvh) * HD;
        float x1[8], x2[8], c[8], sv[8];
        ld8(rk + strip_col_d<HD>(i8, fa.strip), x1);
        ld8(rk + strip_col_d<HD>(HALF + i8, fa.strip), x2);
        ld8(fa.cs + (int64_t)rp * HALF + i8, c);
        ld8(fa.sn + (int64_t)rp * HALF + i8, sv);
#pragma unroll
        for (int e = 0; e < 8; ++e) rope_half_pair(x1[e], x2[e], c[e], sv[e], 1.0f, x1[e], x2[e]);
        const uint4 w1 = make_uint4(pack_bf2(x1[0], x1[1]), pack_bf2(x1[2], x1[3]), pack_bf2(x1[4], x1[5]), pack_bf2(x1[6], x1[7]));
        const uint4 w2 = make_uint4(pack_bf2(x2[0], x2[1]), pack_bf2(x2[2], x2[3]), pack_bf2(x2[4], x2[5]), pack_bf2(x2[6], x2[7]));
        *reinterpret_cast<uint4*>(Kp + (int64_t)pos * HD + i8) = w1;
        *reinterpret_cast<uint4*>(Kp + (int64_t)pos * HD + HALF + i8) = w2;
        *reinterpret_cast<uint4*>(ks + r * RB + ((lane ^ kkey(r)) << 4)) = w1;
        *reinterpret_cast<uint4*>(ks + r * RB + (((lane + HALF / 8) ^ kkey(r)) << 4)) = w2;
    }
    if (DO_V && lane < HD / 8) {
        const uint4 w = *reinterpret_cast<const uint4*>(row + (Hq + Hkv + kvh) * HD + lane * 8);
        *reinterpret_cast<uint4*>(Vp + (int64_t)pos * HD + lane * 8) = w;
        *reinterpret_cast<uint4*>(vs + r * RB + ((lane ^ vkey(r)) << 4)) = w;
    }
    asm volatile("" ::: "memory");          // the fragment reads that follow (ds_read / transposing reads) stay behind the patch
}

// merge the four waves in LDS (red = [4 waves][8 heads][HD + 2] f32) into the block's partial (m, l, O[G][HD]) in `part`; with a
// single split (O_direct set) that partial, normalised, IS the result (what decode_combine_kernel computes for nsplit = 1)
template <int HD>
__device__ __forceinline__ void merge_waves_store(const f32x16 (&o)[HD / 32], float m_run, float l_run, float (*red)[8][HD + 2],
                                                  float* __restrict__ part, bf16_t* __restrict__ O_direct, int tid, int wave,
                                                  int l31, int h, int b, int Hq, int Hkv, int kvh, int G, int split, int nsplit) {
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (l31 < G) {
        float* pp = &red[wave][l31][0];
#pragma unroll
        for (int d = 0; d < HD / 32; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int e = 0; e < 4; ++e) pp[d * 32 + g4 * 8 + h * 4 + e] = o[d][g4 * 4 + e];
        if (h == 0) { pp[HD] = m_run; pp[HD + 1] = l_tot; }
    }
    __syncthreads();
    for (int idx = tid; idx < G * HD; idx += 256) {
        const int g = idx / HD, d = idx % HD;
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) m = fmaxf(m, red[w][g][HD]);
        const float m_use = m == -INFINITY ? 0.f : m;
        float acc = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc = __builtin_amdgcn_exp2f(red[w][g][HD] - m_use);
            acc += sc * red[w][g][d];
            l += sc * red[w][g][HD + 1];
        }
        if (O_direct) {
            const float inv = l > 0.f ? 1.0f / l : 0.f;
            O_direct[((int64_t)b * Hq + kvh * G + g) * HD + d] = f2bf(acc * inv);
            continue;
        }
        float* pp = part + ((((int64_t)b * Hkv + kvh) * nsplit + split) * G + g) * (HD + 2);
        pp[d] = acc;
        if (d == 0) { pp[HD] = m; pp[HD + 1] = l; }
    }
}

struct identity_d {
    template <class T, class... I>
    __device__ T operator()(T x, I...) const { return x; }
};
// O = alpha O + V^T P: vf[d][c4] = the A operand of d block d, kv 16 c4 .. +15, made 16-bit by `cvt`
template <int NDB, class VF, class CV = identity_d>
__device__ __forceinline__ void pv_update(f32x16 (&o)[NDB], const VF (&vf)[NDB][4], const bf16x8 (&pf)[2][2], float alpha,
                                          CV cvt = CV()) {
#pragma unroll
    for (int d = 0; d < NDB; ++d) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
                o[d] = MFMA_32x32x16(cvt(vf[d][blk * 2 + tt]), pf[blk][tt], o[d]);
    }
}

// ---- fan-out decode (gar_attention_decode_fanout): N sampled continuations ("siblings") of one prompt -------------------
// Rows r = b N + i share prompt b's K / V rows (PROMPT cache [B, Hkv, Sp, HD], rows left_pad[b] .. P - 1) and own the rows they
// generated (SUFFIX cache [R, Hkv, T, HD], rows 0 .. t). One launch, two kinds of block, the same tile loop:
//   prefix block (split, column block cb, kv head, prompt b): the heads of up to 32 / G siblings are the live MFMA columns
//     (column c = head c % G of sibling cb (32 / G) + c / G), so the prompt's K / V stream once per column block, not once per row;
//   suffix block (kv head, row r): the fused step of decode_qkv_args over the row's own suffix rows — G live columns, the new
//     key / value appended at suffix row t.
// Every block leaves (m, l, O) partials of one softmax per (row, head): slots 0 .. nsplit - 1 from the prefix splits, slot nsplit
// from the suffix; decode_combine_kernel merges the nsplit + 1 slots. P and t come from device memory (one graph per bucket).
struct decode_fan_args {
    bf16_t* Ks;                 // suffix caches
    bf16_t* Vs;
    const int32_t* prefix_len;  // device: P
    const int32_t* step;        // device: t
    int B, N, T, nsplit;        // prompts, siblings per prompt, suffix rows per sequence, prefix splits
};
// what one block works on: sequence `b` (its left_pad), cache rows kv_lo .. kv_len - 1 of slab Kp / Vp, of which this block
// takes the 64-kv tiles t0 .. t1 - 1; live columns c < ncols = head c % G of row row0 + c / G; its partial goes to `slot` of `nslots`
struct decode_work {
    bf16_t* Kp;
    bf16_t* Vp;
    int kv_stride, kv_len, kv_lo, t0, t1, rp, row0, ncols, slot, nslots;
    bool appends;
};
__device__ __forceinline__ decode_work fan_work(const decode_fan_args& fan, bf16_t* K, bf16_t* V, int Sp, const int32_t* left_pad,
                                                int Hkv, int G, int HD, int kvh, int x) {
    decode_work w;
    const int spb = 32 / G, ncb = (fan.N + spb - 1) / spb;                  // siblings per column block, column blocks
    const int P = min(max(fan.prefix_len[0], 1), Sp), t = min(max(fan.step[0], 0), fan.T - 1);
    const int nprefix = fan.B * ncb * fan.nsplit;
    const bool sfx = x >= nprefix;
    const int b = sfx ? (x - nprefix) / fan.N : x / (fan.nsplit * ncb);
    const int lp = left_pad ? left_pad[b] : 0;
    w.rp = max(P - lp + t, 0);                                              // RoPE position of the step's token
    w.nslots = fan.nsplit + 1;
    w.appends = sfx;
    if (sfx) {
        const int r = x - nprefix;
        w.Kp = fan.Ks + (((int64_t)r * Hkv + kvh) * (int64_t)fan.T) * HD;
        w.Vp = fan.Vs + (((int64_t)r * Hkv + kvh) * (int64_t)fan.T) * HD;
        w.kv_stride = fan.T; w.kv_len = t + 1; w.kv_lo = 0;
        w.t0 = 0; w.t1 = (t + 64) / 64;
        w.row0 = r; w.ncols = G; w.slot = fan.nsplit;
    } else {
        const int split = x % fan.nsplit, cb = (x / fan.nsplit) % ncb;
        w.Kp = K + (((int64_t)b * Hkv + kvh) * (int64_t)Sp) * HD;
        w.Vp = V + (((int64_t)b * Hkv + kvh) * (int64_t)Sp) * HD;
        w.kv_stride = Sp; w.kv_len = P; w.kv_lo = max(min(lp, P - 1), 0);
        const int ntiles = (P + 63) / 64, t_lo = w.kv_lo >> 6;
        const int per = (ntiles - t_lo + fan.nsplit - 1) / fan.nsplit;
        w.t0 = t_lo + split * per; w.t1 = min(ntiles, w.t0 + per);
        w.row0 = b * fan.N + cb * spb; w.ncols = min(fan.N - cb * spb, spb) * G; w.slot = split;
    }
    return w;
}

// a block (split, kv head, sequence) of the plain / fused launches on the grid (splits, Hkv, B)
__device__ __forceinline__ decode_work plain_work(bf16_t* K, bf16_t* V, int kv_stride, const int32_t* kv_len_dev,
                                                  const int32_t* kv_start, bool fused, int Hkv, int G, int HD, int kvh) {
    decode_work w;
    const int split = blockIdx.x, nsplit = gridDim.x, b = blockIdx.z;
    w.kv_len = kv_len_dev[0] + (fused ? 1 : 0);                 // fused: kv_len_dev is the step's position, the new row included
    const int ntiles = (w.kv_len + 63) / 64;
    // left-padded batch: sequence b lives in cache rows kv_lo .. kv_len - 1; the splits divide THAT range
    w.kv_lo = kv_start ? max(min(kv_start[b], w.kv_len - 1), 0) : 0;
    const int t_lo = w.kv_lo >> 6;
    const int per = (ntiles - t_lo + nsplit - 1) / nsplit;
    w.t0 = t_lo + split * per; w.t1 = min(ntiles, w.t0 + per);
    w.Kp = K + (((int64_t)b * Hkv + kvh) * (int64_t)kv_stride) * HD;
    w.Vp = V + (((int64_t)b * Hkv + kvh) * (int64_t)kv_stride) * HD;
    w.kv_stride = kv_stride;
    w.rp = max(w.kv_len - 1 - (kv_start ? kv_start[b] : 0), 0);     // fused: RoPE position of the step's token
    w.row0 = b; w.ncols = G; w.slot = split; w.nslots = nsplit;
    w.appends = fused;
    return w;
}

// merge_waves_store with up to 32 live columns: every wave parks its (O, m, l) in its OWN tile region (its tiles are in
// registers and consumed; `wave_bytes` apart, [32][HD + 2] f32 fit both head dims), so the merge needs no LDS of its own
template <int HD>
__device__ __forceinline__ void merge_waves_store_fan(const f32x16 (&o)[HD / 32], float m_run, float l_run, char* smem, int wave_bytes,
                                                      float* __restrict__ part, const decode_work& w, int tid, int wave, int l31,
                                                      int h, int Hkv, int kvh, int G) {
    static_assert(32 * (HD + 2) * 4 <= HD * 256, "a wave's partial has to fit its tile region");
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (l31 < w.ncols) {
        float* pp = reinterpret_cast<float*>(smem + wave * wave_bytes) + l31 * (HD + 2);
#pragma unroll
        for (int d = 0; d < HD / 32; ++d)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int e = 0; e < 4; ++e) pp[d * 32 + g4 * 8 + h * 4 + e] = o[d][g4 * 4 + e];
        if (h == 0) { pp[HD] = m_run; pp[HD + 1] = l_tot; }
    }
    __syncthreads();
    for (int idx = tid; idx < w.ncols * HD; idx += 256) {
        const int c = idx / HD, d = idx % HD;
        const float* r0 = reinterpret_cast<const float*>(smem) + c * (HD + 2);
        const int ws = wave_bytes / 4;
        float m = -INFINITY;
#pragma unroll
        for (int v = 0; v < 4; ++v) m = fmaxf(m, r0[v * ws + HD]);
        const float m_use = m == -INFINITY ? 0.f : m;
        float acc = 0.f, l = 0.f;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float sc = __builtin_amdgcn_exp2f(r0[v * ws + HD] - m_use);
            acc += sc * r0[v * ws + d];
            l += sc * r0[v * ws + HD + 1];
        }
        float* pp = part + ((((int64_t)(w.row0 + c / G) * Hkv + kvh) * w.nslots + w.slot) * G + c % G) * (HD + 2);
        pp[d] = acc;
        if (d == 0) { pp[HD] = m; pp[HD + 1] = l; }
    }
}

#ifndef DA_KV_AUX               /* cache policy of the K / V DMA: 2 = nt — every byte of the cache is read once per step:
                                   B = 64, kv 4750: 105.8 -> 98.2 us (5.88 -> 6.34 TB/s; profiles/r3_decode_nt.txt) */
#define DA_KV_AUX 2
#endif
#define LDS_AS(p) ((__attribute__((address_space(3))) void*)(p))
// FAN: a block of the fan-out launch (decode_fan_args; Q / kv_len_dev unused, K / V the prompt caches, kv_stride their rows)
template <bool FAN>
__device__ __forceinline__ void decode_block64(const bf16_t* __restrict__ Q, bf16_t* K, bf16_t* V, float* __restrict__ part,
    int Hq, int Hkv, int kv_stride, const int32_t* __restrict__ kv_len_dev, const int32_t* __restrict__ kv_start,
    bf16_t* __restrict__ O_direct, const decode_qkv_args& fa, int64_t q_stride, const decode_fan_args& fan) {
    constexpr int HD = 64, NKD = HD / 16, NDB = HD / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [4 waves][K 8 KiB | V 8 KiB] then red
    float (*red)[8][HD + 2] = reinterpret_cast<float (*)[8][HD + 2]>(smem + 4 * 16384);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int kvh = blockIdx.y;
    const int G = Hq / Hkv;
    const decode_work w = FAN ? fan_work(fan, K, V, kv_stride, kv_start, Hkv, G, HD, kvh, blockIdx.x)
                              : plain_work(K, V, kv_stride, kv_len_dev, kv_start, fa.raw != nullptr, Hkv, G, HD, kvh);
    const int kv_len = w.kv_len, kv_lo = w.kv_lo, t0 = w.t0, t1 = w.t1, rp = w.rp;
    const int ntiles = (kv_len + 63) / 64;
    bf16_t* Kp = w.Kp;
    bf16_t* Vp = w.Vp;
    const unsigned slab = (unsigned)w.kv_stride * HD * 2u;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kp, 0, (int)slab, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vp, 0, (int)slab, 0x00020000);
    char* ks = smem + wave * 16384;
    char* vs = ks + 8192;
    // DMA piece i = rows 8i .. 8i+7 of the tile (1 KiB, lane-linear in LDS). K: row r keeps its 16-byte chunk c at
    // position c ^ key(r), key(r) = (r >> 1) & 7 = (lane >> 4) | ((i & 1) << 2). V: chunk c at c ^ 4 ((r >> 1) & 1) — the
    // four rows of a transposing read's block then cover all 64 banks once (attention_bf16.hip) — the same for every piece
    const int sub = lane >> 3, chunk = lane & 7, kq = lane >> 4;
    int offK[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) offK[par] = sub * 128 + ((chunk ^ (kq | (par << 2))) << 4);
    const int offV = sub * 128 + ((chunk ^ (((sub >> 1) & 1) << 2)) << 4);
    auto stage = [&](int t) {
        const unsigned base = (unsigned)t * 64u * 128u;         // 64 kv rows of 128 B, K and V alike
#pragma unroll
        for (int i = 0; i < 8; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, LDS_AS(ks + i * 1024), 16,
                                                     offK[i & 1] + (int)(base + (unsigned)i * 1024u), 0, 0, DA_KV_AUX);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, LDS_AS(vs + i * 1024), 16,
                                                     offV + (int)(base + (unsigned)i * 1024u), 0, 0, DA_KV_AUX);
    };
    bf16x8 qf[NKD];
    if (FAN) {                  // column c: head c % G of row row0 + c / G
        const int c = min(l31, w.ncols - 1);
        load_q_rotated<HD>(qf, fa, w.row0 + c / G, Hq, Hkv, kvh * G + c % G, l31 < w.ncols, h, rp);
    } else if (fa.raw) {
        load_q_rotated<HD>(qf, fa, w.row0, Hq, Hkv, kvh * G + min(l31, G - 1), l31 < G, h, rp);
    } else {
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16_t* qp = Q + ((int64_t)w.row0 * Hq + kvh * G + min(l31, G - 1)) * q_stride;
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd)
            qf[kd] = l31 < G ? *reinterpret_cast<const bf16x8*>(qp + kd * 16 + h * 8) : z;
    }
    f32x16 o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int prow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int koff[2], kkey[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int row = blk * 32 + prow;
        koff[blk] = row * 128;
        kkey[blk] = (row >> 1) & 7;
    }
    // this lane's chunk of its 16-lane group's [4 kv][16 d] block: kv row 8h + (i >> 2) of a 16-kv step, d columns
    // 16 ((lane >> 4) & 1) + 4 (i & 3) of a 32-d block; d-block 1 = chunk index + 4 = ^ 64 bytes
    int vtr;
    {
        const int i = lane & 15, r = 8 * h + (i >> 2), col = 16 * ((lane >> 4) & 1) + 4 * (i & 3);
        vtr = r * 128 + ((((col >> 3) ^ (((r >> 1) & 1) << 2)) << 4) | ((col & 7) << 1));
    }

    int t = t0 + wave;
    if (t < t1) stage(t);
    for (; t < t1; t += 4) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (w.appends && t == ntiles - 1)           // the tile that holds the step's own row: this wave appends it
            append_new_kv<HD, true, true>(fa, Kp, Vp, ks, vs, w.row0, Hq, Hkv, kvh, lane,
                                          kv_len - 1, rp, [](int r) { return (r >> 1) & 7; }, [](int r) { return ((r >> 1) & 1) << 2; });
        bf16x8 kf[2][NKD], vf[NDB][4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kd = 0; kd < NKD; ++kd)
                kf[blk][kd] = *reinterpret_cast<const bf16x8*>(ks + koff[blk] + (((kd * 2 + h) ^ kkey[blk]) << 4));
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) vf[d][c4] = v_frag_tr(vs + c4 * 16 * 128 + (vtr ^ (d << 6)), 4 * 128);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (t + 4 < t1) stage(t + 4);            // re-arm the region: its fragments are in registers now
        __builtin_amdgcn_sched_barrier(0);
        const int kv0 = t * 64;
        f32x16 s[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kd = 0; kd < NKD; ++kd)
                s[blk] = MFMA_32x32x16(kf[blk][kd], qf[kd], kd == 0 ? zero16 : s[blk]);
        if (kv0 + 64 > kv_len || kv0 < kv_lo) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kv0 + blk * 32 + ((r >> 3) << 4) + h * 8 + (r & 7);
                    s[blk][r] = (kv < kv_len && kv >= kv_lo) ? s[blk][r] : -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[blk][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        m_run = m_new;
        float ps = 0.f;
        bf16x8 pf[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(s[blk][r] - m_use); ps += p[r]; }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                u32x4 w;
                w[0] = cvt_pk_d(p[tt * 8 + 0], p[tt * 8 + 1]);
                w[1] = cvt_pk_d(p[tt * 8 + 2], p[tt * 8 + 3]);
                w[2] = cvt_pk_d(p[tt * 8 + 4], p[tt * 8 + 5]);
                w[3] = cvt_pk_d(p[tt * 8 + 6], p[tt * 8 + 7]);
                pf[blk][tt] = __builtin_bit_cast(bf16x8, w);
            }
        }
        l_run = l_run * alpha + ps;
        pv_update(o, vf, pf, alpha);
    }
    if (FAN) merge_waves_store_fan<HD>(o, m_run, l_run, smem, 16384, part, w, tid, wave, l31, h, Hkv, kvh, G);
    else merge_waves_store<HD>(o, m_run, l_run, red, part, O_direct, tid, wave, l31, h, w.row0, Hq, Hkv, kvh, G, w.slot, w.nslots);
}

__global__ __launch_bounds__(256, 2) void decode_attn_lds_kernel(const bf16_t* __restrict__ Q, bf16_t* K, bf16_t* V,      // K / V: appended to in fused mode
        float* __restrict__ part, int Hq, int Hkv, int kv_stride, const int32_t* __restrict__ kv_len_dev,
        const int32_t* __restrict__ kv_start, bf16_t* __restrict__ O_direct, const decode_qkv_args fa, int64_t q_stride) {
    decode_block64<false>(Q, K, V, part, Hq, Hkv, kv_stride, kv_len_dev, kv_start, O_direct, fa, q_stride, decode_fan_args{});
}
// grid (B column-blocks nsplit + R, Hkv): K / V the prompt caches [B, Hkv, Sp, HD], left_pad [B] or NULL
__global__ __launch_bounds__(256, 2) void decode_attn_lds_fan_kernel(bf16_t* K, bf16_t* V, float* __restrict__ part, int Hq, int Hkv, int Sp,
        const int32_t* __restrict__ left_pad, const decode_qkv_args fa, const decode_fan_args fan) {
    decode_block64<true>(nullptr, K, V, part, Hq, Hkv, Sp, nullptr, left_pad, nullptr, fa, 0, fan);
}

// ---------------------------------------------------------------------------------------------------------------
// head_dim 128 (Llama-3.1-8B): a 64-kv tile is 16 KiB of K (256-byte rows) + 16 KiB of V per wave.
// Pulling both into registers before re-arming the region (what the head_dim-64 kernel does) would need 128 VGPRs of
// fragments on top of the 64 of O, so K and V are two phases with their own DMA groups and counted waits:
//   wait K(t) [vmcnt: the 16 V pieces behind it may stay out] -> K fragments -> re-arm K with tile t+4 -> QK^T, softmax
//   wait V(t) [the 16 K pieces just issued may stay out]      -> V fragments -> re-arm V             -> PV
// 128 KiB + merge buffer per block: one block (4 waves) per CU, the same 128 KiB of loads in flight per CU.
// FAN: a block of the fan-out launch (decode_fan_args; Q / kv_len_dev unused, K / V the prompt caches, kv_stride their rows)
template <bool FAN>
__device__ __forceinline__ void decode_block128(const bf16_t* __restrict__ Q, bf16_t* K, bf16_t* V, float* __restrict__ part,
    int Hq, int Hkv, int kv_stride, const int32_t* __restrict__ kv_len_dev, const int32_t* __restrict__ kv_start,
    bf16_t* __restrict__ O_direct, const decode_qkv_args& fa, int64_t q_stride, const decode_fan_args& fan) {
    constexpr int HD = 128, NKD = HD / 16, NDB = HD / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [4 waves][K 16 KiB | V 16 KiB] then red
    float (*red)[8][HD + 2] = reinterpret_cast<float (*)[8][HD + 2]>(smem + 4 * 32768);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int kvh = blockIdx.y;
    const int G = Hq / Hkv;
    const decode_work w = FAN ? fan_work(fan, K, V, kv_stride, kv_start, Hkv, G, HD, kvh, blockIdx.x)
                              : plain_work(K, V, kv_stride, kv_len_dev, kv_start, fa.raw != nullptr, Hkv, G, HD, kvh);
    const int kv_len = w.kv_len, kv_lo = w.kv_lo, t0 = w.t0, t1 = w.t1, rp = w.rp;
    const int ntiles = (kv_len + 63) / 64;
    bf16_t* Kp = w.Kp;
    bf16_t* Vp = w.Vp;
    const unsigned slab = (unsigned)w.kv_stride * HD * 2u;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kp, 0, (int)slab, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vp, 0, (int)slab, 0x00020000);
    char* ks = smem + wave * 32768;
    char* vs = ks + 16384;
    // K piece i = rows 4i .. 4i+3 (256 B each); row r keeps its 16-byte chunk c at position c ^ (r & 15)
    // V piece i = rows 4i .. 4i+3 too; row r keeps chunk c at c ^ 4 (r & 3): the four rows of a transposing read's block are
    // 256 B apart and take the four 64-byte bank groups (attention_bf16.hip) — the same offsets for every piece
    int offK[4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const int r = lane >> 4;                                    // row inside the piece
        const int c = (lane & 15) ^ ((q4 * 4 + r) & 15);
        offK[q4] = r * 256 + (c << 4);
    }
    const int offV = (lane >> 4) * 256 + (((lane & 15) ^ ((lane >> 4) << 2)) << 4);
    auto stageK = [&](int t) {
        const unsigned kbase = (unsigned)t * 64u * 256u;        // 64 kv rows of 256 B
#pragma unroll
        for (int i = 0; i < 16; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, LDS_AS(ks + i * 1024), 16,
                                                     offK[i & 3] + (int)(kbase + (unsigned)i * 1024u), 0, 0, DA_KV_AUX);
    };
    auto stageV = [&](int t) {
        const unsigned vbase = (unsigned)t * 64u * 256u;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, LDS_AS(vs + i * 1024), 16,
                                                     offV + (int)(vbase + (unsigned)i * 1024u), 0, 0, DA_KV_AUX);
    };
    bf16x8 qf[NKD];
    if (FAN) {                  // column c: head c % G of row row0 + c / G
        const int c = min(l31, w.ncols - 1);
        load_q_rotated<HD>(qf, fa, w.row0 + c / G, Hq, Hkv, kvh * G + c % G, l31 < w.ncols, h, rp);
    } else if (fa.raw) {
        load_q_rotated<HD>(qf, fa, w.row0, Hq, Hkv, kvh * G + min(l31, G - 1), l31 < G, h, rp);
    } else {
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16_t* qp = Q + ((int64_t)w.row0 * Hq + kvh * G + min(l31, G - 1)) * q_stride;
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd)
            qf[kd] = l31 < G ? *reinterpret_cast<const bf16x8*>(qp + kd * 16 + h * 8) : z;
    }
    f32x16 o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int prow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int koff[2], kkey[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int row = blk * 32 + prow;
        koff[blk] = row * 256;
        kkey[blk] = row & 15;
    }
    int vtr;            // see decode_attn_lds_kernel; 256-byte rows, chunk key 4 (r & 3)
    {
        const int i = lane & 15, r = 8 * h + (i >> 2), col = 16 * ((lane >> 4) & 1) + 4 * (i & 3);
        vtr = r * 256 + ((((col >> 3) ^ ((r & 3) << 2)) << 4) | ((col & 7) << 1));
    }

    int t = t0 + wave;
    if (t < t1) { stageK(t); stageV(t); }
    for (; t < t1; t += 4) {
        const bool more = t + 4 < t1;
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");          // K(t) landed; the 16 V(t) pieces may still be out
        const bool own_new = w.appends && t == ntiles - 1;            // the tile that holds the step's own row (this wave's last tile)
        if (own_new)
            append_new_kv<HD, true, false>(fa, Kp, Vp, ks, vs, w.row0, Hq, Hkv, kvh, lane,
                                           kv_len - 1, rp, [](int r) { return r & 15; }, [](int r) { return (r & 3) << 2; });
        f32x16 s[2];
        {
            bf16x8 kf[2][NKD];
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int kd = 0; kd < NKD; ++kd)
                    kf[blk][kd] = *reinterpret_cast<const bf16x8*>(ks + koff[blk] + (((kd * 2 + h) ^ kkey[blk]) << 4));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (more) stageK(t + 4);             // re-arm the K half: its fragments are in registers now
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int kd = 0; kd < NKD; ++kd)
                    s[blk] = MFMA_32x32x16(kf[blk][kd], qf[kd], kd == 0 ? zero16 : s[blk]);
        }
        const int kv0 = t * 64;
        if (kv0 + 64 > kv_len || kv0 < kv_lo) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kv0 + blk * 32 + ((r >> 3) << 4) + h * 8 + (r & 7);
                    s[blk][r] = (kv < kv_len && kv >= kv_lo) ? s[blk][r] : -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[blk][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        m_run = m_new;
        float ps = 0.f;
        bf16x8 pf[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { p[r] = __builtin_amdgcn_exp2f(s[blk][r] - m_use); ps += p[r]; }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                u32x4 w;
                w[0] = cvt_pk_d(p[tt * 8 + 0], p[tt * 8 + 1]);
                w[1] = cvt_pk_d(p[tt * 8 + 2], p[tt * 8 + 3]);
                w[2] = cvt_pk_d(p[tt * 8 + 4], p[tt * 8 + 5]);
                w[3] = cvt_pk_d(p[tt * 8 + 6], p[tt * 8 + 7]);
                pf[blk][tt] = __builtin_bit_cast(bf16x8, w);
            }
        }
        l_run = l_run * alpha + ps;
        // V(t): everything issued before K(t+4) has to be in; the 16 K pieces just issued may stay out
        if (more) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (own_new)                            // (the key row's global stores sit behind vmcnt(0) too: `more` is false here)
            append_new_kv<HD, false, true>(fa, Kp, Vp, ks, vs, w.row0, Hq, Hkv, kvh, lane,
                                           kv_len - 1, rp, [](int r) { return r & 15; }, [](int r) { return (r & 3) << 2; });
        bf16x8 vf[NDB][4];
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) vf[d][c4] = v_frag_tr(vs + c4 * 16 * 256 + (vtr ^ (d << 6)), 4 * 256);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (more) stageV(t + 4);
        __builtin_amdgcn_sched_barrier(0);
        pv_update(o, vf, pf, alpha);
    }
    if (FAN) merge_waves_store_fan<HD>(o, m_run, l_run, smem, 32768, part, w, tid, wave, l31, h, Hkv, kvh, G);
    else merge_waves_store<HD>(o, m_run, l_run, red, part, O_direct, tid, wave, l31, h, w.row0, Hq, Hkv, kvh, G, w.slot, w.nslots);
}

__global__ __launch_bounds__(256, 1) void decode_attn_lds128_kernel(const bf16_t* __restrict__ Q, bf16_t* K, bf16_t* V,      // K / V: appended to in fused mode
        float* __restrict__ part, int Hq, int Hkv, int kv_stride, const int32_t* __restrict__ kv_len_dev,
        const int32_t* __restrict__ kv_start, bf16_t* __restrict__ O_direct, const decode_qkv_args fa, int64_t q_stride) {
    decode_block128<false>(Q, K, V, part, Hq, Hkv, kv_stride, kv_len_dev, kv_start, O_direct, fa, q_stride, decode_fan_args{});
}
// grid (B column-blocks nsplit + R, Hkv): K / V the prompt caches [B, Hkv, Sp, HD], left_pad [B] or NULL
__global__ __launch_bounds__(256, 1) void decode_attn_lds128_fan_kernel(bf16_t* K, bf16_t* V, float* __restrict__ part, int Hq, int Hkv, int Sp,
        const int32_t* __restrict__ left_pad, const decode_qkv_args fa, const decode_fan_args fan) {
    decode_block128<true>(nullptr, K, V, part, Hq, Hkv, Sp, nullptr, left_pad, nullptr, fa, 0, fan);
}

// one wave per (b, q head): lanes over splits for the statistics, then over d for the accumulation
template <int HD>
__global__ __launch_bounds__(64) void decode_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ O, int Hq,
                                                            int Hkv, int nsplit) {
    const int head = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int G = Hq / Hkv, kvh = head / G, g = head % G;
    const float* base = part + ((((int64_t)b * Hkv + kvh) * nsplit) * G + g) * (HD + 2);
    const int64_t sstride = (int64_t)G * (HD + 2);
    const float ms = lane < nsplit ? base[lane * sstride + HD] : -INFINITY;
    const float ls = lane < nsplit ? base[lane * sstride + HD + 1] : 0.f;
    const float m = wave_max(ms);
    const float m_use = m == -INFINITY ? 0.f : m;
    const float wgt = __builtin_amdgcn_exp2f(ms - m_use);          // 0 for empty splits / lanes >= nsplit
    const float l = wave_sum(wgt * ls);
    float acc[HD / 64];
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) acc[i] = 0.f;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {
        const float w = __shfl(wgt, s, 64);
#pragma unroll
        for (int i = 0; i < HD / 64; ++i) acc[i] += w * base[s * sstride + i * 64 + lane];
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int i = 0; i < HD / 64; ++i) O[((int64_t)b * Hq + head) * HD + i * 64 + lane] = f2bf(acc[i] * inv);
}

extern "C" int64_t gar_attention_decode_workspace(int B, int Hq, int hd, int max_splits) {
    return (int64_t)B * Hq * max_splits * (hd + 2) * 4;
}

// the argument checks every decode entry point shares (`what`: the entry point, for the error text). Plain forms: q and its
// row stride (<= 0 means head_dim). Fused forms: q = the raw qkv rows, q_stride null.
static int check_decode_args(const char* what, const void* q, int64_t* q_stride, int B, int Hq, int Hkv, int hd, int Smax) {
    GAR_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Hq / Hkv <= 8, "%s: Hq/Hkv must be <= 8", what);
    GAR_CHECK_ARG(Smax % 64 == 0, "%s: Smax must be a multiple of 64", what);
    GAR_CHECK_ARG(hd == 64 || hd == 128, "%s: head_dim %d not built (64, 128)", what, hd);
    if (!q_stride) {
        GAR_CHECK_ARG(((uintptr_t)q & 15) == 0, "%s: qkv must be 16-byte aligned", what);
        return GAR_OK;
    }
    int64_t& qs = *q_stride;
    if (qs <= 0) qs = hd;
    GAR_CHECK_ARG(qs % hd == 0 && ((uintptr_t)q & 15) == 0, "%s: q_stride must be a multiple of head_dim, q 16-byte aligned", what);
    return GAR_OK;
}

// dynamic LDS of a decode block: the four waves' tile regions, then the merge buffer red[4 waves][8 heads][HD + 2] f32
constexpr int decode_lds_bytes(int wave_bytes, int hd) { return 4 * wave_bytes + 4 * 8 * (hd + 2) * 4; }

// one split-KV decode: KERNEL (LDS bytes of dynamic LDS) on the grid (max_splits, Hkv, B), then decode_combine_kernel — with
// one split per (sequence, kv head) the attention kernel normalises and writes O itself, no combine launch. `caches`: the
// kernel's cache pointer arguments, `elem_bytes` the bytes of one cache element.
template <int HD, auto KERNEL, int LDS, class... Caches>
static int launch_split_kv(const char* what, int elem_bytes, const void* q, int64_t q_stride, void* O, int B, int Hq, int Hkv,
                           int Smax, const int32_t* kv_len_dev, const int32_t* kv_start, int max_splits, void* workspace,
                           const decode_qkv_args& fa, gar_stream_t stream, Caches... caches) {
    GAR_CHECK_ARG(workspace && max_splits > 0 && max_splits <= 64, "%s: workspace / max_splits (1..64)", what);
    if ((int64_t)Smax * HD * elem_bytes >= ((int64_t)1 << 31)) {       // one (sequence, kv head) slab has to fit a buffer descriptor
        gar_set_error("%s: Smax %d x head_dim %d exceeds the 2 GiB per-slab range of the DMA-staged kernels", what, Smax, HD);
        return GAR_ERR_UNSUPPORTED;
    }
    static gar_once_per_device attr_once;
    attr_once.run([&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    });
    hipStream_t s = (hipStream_t)stream;
    bf16_t* direct = max_splits == 1 ? (bf16_t*)O : nullptr;
    hipLaunchKernelGGL(KERNEL, dim3(max_splits, Hkv, B), dim3(256), LDS, s, (const bf16_t*)q, caches..., (float*)workspace, Hq, Hkv,
                       Smax, kv_len_dev, kv_start, direct, fa, q_stride);
    if (!direct)
        hipLaunchKernelGGL((decode_combine_kernel<HD>), dim3(Hq, B), dim3(64), 0, s, (const float*)workspace, (bf16_t*)O, Hq, Hkv,
                           max_splits);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

static int launch_decode(const char* what, const void* q, int64_t q_stride, void* Kc, void* Vc, void* O, int B, int Hq, int Hkv,
                         int hd, int Smax, const int32_t* kv_len_dev, const int32_t* kv_start, int max_splits, void* workspace,
                         const decode_qkv_args& fa, gar_stream_t stream) {
    if (hd == 64)
        return launch_split_kv<64, decode_attn_lds_kernel, decode_lds_bytes(16384, 64)>(
            what, 2, q, q_stride, O, B, Hq, Hkv, Smax, kv_len_dev, kv_start, max_splits, workspace, fa, stream, (bf16_t*)Kc, (bf16_t*)Vc);
    return launch_split_kv<128, decode_attn_lds128_kernel, decode_lds_bytes(32768, 128)>(
        what, 2, q, q_stride, O, B, Hq, Hkv, Smax, kv_len_dev, kv_start, max_splits, workspace, fa, stream, (bf16_t*)Kc, (bf16_t*)Vc);
}

extern "C" int gar_attention_decode(int dtype, const void* q, int64_t q_stride, const void* Kc, const void* Vc, void* O, int B,
                                    int Hq, int Hkv, int hd, int Smax, const int32_t* kv_len_dev, const int32_t* kv_start,
                                    int max_splits, void* workspace, gar_stream_t stream) {
    GAR_CHECK_ARG(q && Kc && Vc && O && kv_len_dev, "attention_decode: null pointer");
    if (int e = check_decode_args("attention_decode", q, &q_stride, B, Hq, Hkv, hd, Smax)) return e;
    if (dtype == GAR_F32)   // parity mode: the prefill kernel with q_len = 1 (exact-f32 MFMA), no split; (b, head) rows q_stride apart
        return gar_attention_vrow(dtype, q, Kc, Vc, O, B, Hq, Hkv, hd, 1, (int)(q_stride / hd), 0, Smax, 0, kv_len_dev, kv_start, 0,
                                  stream);
    GAR_CHECK_ARG(dtype == GAR_BF16, "attention_decode: bad dtype");
    const decode_qkv_args none = {nullptr, nullptr, nullptr, 0.f, 0};
    // (the plain form only reads the caches)
    return launch_decode("attention_decode", q, q_stride, const_cast<void*>(Kc), const_cast<void*>(Vc), O, B, Hq, Hkv, hd, Smax,
                         kv_len_dev, kv_start, max_splits, workspace, none, stream);
}

// gar_llm_qkv_post (S = 1) + gar_attention_decode in ONE launch (bf16): see decode_qkv_args. GAR_ERR_UNSUPPORTED (nothing
// launched) in parity mode: the caller keeps the two calls.
extern "C" int gar_attention_decode_qkv(int dtype, const void* qkv, const float* cos, const float* sin, void* Kc, void* Vc,
                                        void* O, int B, int Hq, int Hkv, int hd, int Smax, const int32_t* pos_dev,
                                        const int32_t* left_pad, float q_scale, int qk_strip_order, int max_splits,
                                        void* workspace, gar_stream_t stream) {
    GAR_CHECK_ARG(qkv && cos && sin && Kc && Vc && O && pos_dev, "attention_decode_qkv: null pointer");
    if (int e = check_decode_args("attention_decode_qkv", qkv, nullptr, B, Hq, Hkv, hd, Smax)) return e;
    if (dtype != GAR_BF16) {
        gar_set_error("attention_decode_qkv: bf16 only (parity mode runs gar_llm_qkv_post + gar_attention_decode)");
        return GAR_ERR_UNSUPPORTED;
    }
    const decode_qkv_args fa = {(const bf16_t*)qkv, cos, sin, q_scale, qk_strip_order ? 1 : 0};
    return launch_decode("attention_decode_qkv", nullptr, hd, Kc, Vc, O, B, Hq, Hkv, hd, Smax, pos_dev, left_pad, max_splits,
                         workspace, fa, stream);
}

// ---- gar_attention_decode_fanout: see decode_fan_args --------------------------------------------------------------------
extern "C" int64_t gar_attention_decode_fanout_workspace(int R, int Hq, int hd, int max_splits) {
    return gar_attention_decode_workspace(R, Hq, hd, max_splits + 1);          // the prefix splits' slots and the suffix slot
}

extern "C" int gar_attention_decode_fanout(int dtype, const void* qkv, const float* cos, const float* sin, const void* Kp,
                                           const void* Vp, void* Ksuf, void* Vsuf, void* O, int B, int N, int Hq, int Hkv, int hd,
                                           int Sp, int T, const int32_t* prefix_len_dev, const int32_t* step_dev,
                                           const int32_t* left_pad, float q_scale, int qk_strip_order, int max_splits,
                                           void* workspace, gar_stream_t stream) {
    const char* what = "attention_decode_fanout";
    GAR_CHECK_ARG(qkv && cos && sin && Kp && Vp && Ksuf && Vsuf && O && prefix_len_dev && step_dev, "%s: null pointer", what);
    GAR_CHECK_ARG(N > 0 && (int64_t)B * N <= 65535, "%s: need N >= 1 rows per prompt and B * N <= 65535", what);
    if (int e = check_decode_args(what, qkv, nullptr, B, Hq, Hkv, hd, Sp)) return e;
    GAR_CHECK_ARG(T > 0 && T % 64 == 0, "%s: T must be a positive multiple of 64", what);
    GAR_CHECK_ARG(workspace && max_splits > 0 && max_splits < 64, "%s: workspace / max_splits (1..63)", what);
    if (dtype != GAR_BF16) {
        gar_set_error("%s: 16-bit only (parity mode decodes N copies of the prompt's cache rows with the plain step)", what);
        return GAR_ERR_UNSUPPORTED;
    }
    if ((int64_t)max(Sp, T) * hd * 2 >= ((int64_t)1 << 31)) {
        gar_set_error("%s: %d rows x head_dim %d exceed the 2 GiB per-slab range of the DMA-staged kernels", what, max(Sp, T), hd);
        return GAR_ERR_UNSUPPORTED;
    }
    const int G = Hq / Hkv, spb = 32 / G, ncb = (N + spb - 1) / spb, R = B * N;
    const decode_qkv_args fa = {(const bf16_t*)qkv, cos, sin, q_scale, qk_strip_order ? 1 : 0};
    const decode_fan_args fan = {(bf16_t*)Ksuf, (bf16_t*)Vsuf, prefix_len_dev, step_dev, B, N, T, max_splits};
    const dim3 grid((unsigned)(B * ncb * max_splits + R), Hkv);
    hipStream_t s = (hipStream_t)stream;
    static gar_once_per_device attr_once;
    attr_once.run([&] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_attn_lds_fan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  4 * 16384);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_attn_lds128_fan_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 32768);
    });
    // (the prompt caches are only read: the fan kernels append to the suffix caches)
    if (hd == 64)
        hipLaunchKernelGGL(decode_attn_lds_fan_kernel, grid, dim3(256), 4 * 16384, s, (bf16_t*)const_cast<void*>(Kp),
                           (bf16_t*)const_cast<void*>(Vp), (float*)workspace, Hq, Hkv, Sp, left_pad, fa, fan);
    else
        hipLaunchKernelGGL(decode_attn_lds128_fan_kernel, grid, dim3(256), 4 * 32768, s, (bf16_t*)const_cast<void*>(Kp),
                           (bf16_t*)const_cast<void*>(Vp), (float*)workspace, Hq, Hkv, Sp, left_pad, fa, fan);
    if (hd == 64)
        hipLaunchKernelGGL((decode_combine_kernel<64>), dim3(Hq, R), dim3(64), 0, s, (const float*)workspace, (bf16_t*)O, Hq, Hkv,
                           max_splits + 1);
    else
        hipLaunchKernelGGL((decode_combine_kernel<128>), dim3(Hq, R), dim3(64), 0, s, (const float*)workspace, (bf16_t*)O, Hq, Hkv,
                           max_splits + 1);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// =====================================================================================================================
// FP8 KV cache (GARModel(kv_cache_dtype="fp8"), ABI 16): OCP e4m3fn bytes Kc8 / Vc8 [B, Hkv, Smax, hd] and one f32 scale per
// (sequence, kv head, position) in Ks / Vs [B, Hkv, Smax], K and V apart. A 16-bit vector x of hd values (K after RoPE) is
//   amax = max|x|, inv = 448 / amax, q = e4m3(RNE(x * inv)), scale = amax / 448
//   inv not finite (amax == 0, or amax < 448 / FLT_MAX ~ 1.3e-36 — bf16 reaches it, fp16 cannot): q = 0, scale = 0
// in exactly these f32 operations: (x.float() * inv).to(torch.float8_e4m3fn) restates it byte for byte (|x * inv| <= 448
// rounds inside the format, so the conversion never saturates; the inv = inf case above is excluded, 0 * inf would be NaN). The decode kernels dequantize by scaling, not per element:
// score_j = (q . k8_j) * sk_j, and the softmax weight p_j enters the PV product as p_j * sv_j (the normaliser sums p_j).
// FP8_MAX, pk4_fp8 and fp8x8_to_h16 live in fp8.h (shared with the fp8-weight GEMV of gemm_skinny.hip).
// ---- gar_kv_quantize_fp8: one wave per (position, kv head, sequence); lanes 0..31 quantize the K vector, 32..63 the V vector
template <int HD>
__global__ __launch_bounds__(256) void kv_quantize_fp8_kernel(const bf16_t* __restrict__ K, const bf16_t* __restrict__ V,
                                                              int src_stride, uint8_t* __restrict__ K8, uint8_t* __restrict__ V8,
                                                              float* __restrict__ Ks, float* __restrict__ Vs, int Hkv, int Smax,
                                                              int kv_start, int S) {
    constexpr int E = HD / 32;                  // values per lane
    const int lane = threadIdx.x & 63;
    const int pos = kv_start + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pos >= S) return;                       // (uniform per wave)
    const int kvh = blockIdx.y, b = blockIdx.z;
    const bool isv = lane >= 32;
    const int l = lane & 31;
    const int64_t sl = (int64_t)b * Hkv + kvh;
    const bf16_t* src = (isv ? V : K) + (sl * src_stride + pos) * HD + l * E;
    float x[E];
    if constexpr (E == 2) {
        const unsigned int w = *reinterpret_cast<const unsigned int*>(src);
        x[0] = unpk_lo(w); x[1] = unpk_hi(w);
    } else {
        const u32x2 w = *reinterpret_cast<const u32x2*>(src);
        x[0] = unpk_lo(w[0]); x[1] = unpk_hi(w[0]); x[2] = unpk_lo(w[1]); x[3] = unpk_hi(w[1]);
    }
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) a = fmaxf(a, fabsf(x[e]));
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 64));      // within the 32-lane half
    const float inv = FP8_MAX / a;
    const bool live = inv < INFINITY;           // amax > 0 and 448 / amax finite
    uint8_t* dst = (isv ? V8 : K8) + (sl * Smax + pos) * HD + l * E;
    if constexpr (E == 2) {
        const unsigned int w = live ? (unsigned int)__builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false) : 0u;
        *reinterpret_cast<uint16_t*>(dst) = (uint16_t)(w & 0xffffu);
    } else {
        *reinterpret_cast<unsigned int*>(dst) = live ? pk4_fp8(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv) : 0u;
    }
    if (l == 0) (isv ? Vs : Ks)[sl * Smax + pos] = live ? a / FP8_MAX : 0.f;
}

extern "C" int gar_kv_quantize_fp8(int dtype, const void* K, const void* V, int src_stride, void* Kc8, void* Vc8, float* Ks,
                                   float* Vs, int B, int Hkv, int hd, int Smax, int kv_start, int S, gar_stream_t stream) {
    GAR_CHECK_ARG(K && V && Kc8 && Vc8 && Ks && Vs, "kv_quantize_fp8: null pointer");
    GAR_CHECK_ARG(dtype == GAR_BF16, "kv_quantize_fp8: 16-bit source only (the fp8 cache has no parity mode)");
    GAR_CHECK_ARG(hd == 64 || hd == 128, "kv_quantize_fp8: head_dim %d not built (64, 128)", hd);
    GAR_CHECK_ARG(B > 0 && Hkv > 0 && 0 <= kv_start && kv_start <= S && S <= Smax && S <= src_stride,
                  "kv_quantize_fp8: need 0 <= kv_start <= S <= min(Smax, src_stride)");
    if (kv_start == S) return GAR_OK;
    GAR_CHECK_ARG(((uintptr_t)K & 7) == 0 && ((uintptr_t)V & 7) == 0 && ((uintptr_t)Kc8 & 3) == 0 && ((uintptr_t)Vc8 & 3) == 0,
                  "kv_quantize_fp8: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((S - kv_start + 3) / 4, Hkv, B);
    if (hd == 64)
        hipLaunchKernelGGL(kv_quantize_fp8_kernel<64>, grid, dim3(256), 0, s, (const bf16_t*)K, (const bf16_t*)V, src_stride,
                           (uint8_t*)Kc8, (uint8_t*)Vc8, Ks, Vs, Hkv, Smax, kv_start, S);
    else
        hipLaunchKernelGGL(kv_quantize_fp8_kernel<128>, grid, dim3(256), 0, s, (const bf16_t*)K, (const bf16_t*)V, src_stride,
                           (uint8_t*)Kc8, (uint8_t*)Vc8, Ks, Vs, Hkv, Smax, kv_start, S);
    GAR_CHECK_LAUNCH();
    return GAR_OK;
}

// ---- gar_attention_decode_fp8 / gar_attention_decode_qkv_fp8 ---------------------------------------------------------
// The structure of decode_attn_lds_kernel at half the bytes: every wave DMAs its 64-kv tiles — K tile | V tile (64 rows of
// HD bytes each) and the tile's 64 K | 64 V scales — into a private LDS region, now double-buffered (two tiles in flight per
// wave: HD 64 keeps 2 blocks per CU, HD 128 one, ~130 KiB of loads in flight per CU either way). The scales have three
// buffers, so that a tile's scales are read where they are used, after the K / V buffer has been re-armed (registers). Row r of a tile keeps its 16-byte
// chunk c at position c ^ key(r), key = (r >> 2) & 3 (HD 64) / (r >> 1) & 7 (HD 128): the 32 rows of a fragment read spread
// over 16 chunk positions. K fragments are one ds_read_b64 (8 bytes of a row); V fragments (8 kv of one d column) are eight
// byte reads. Both stay raw bytes in registers until the region is re-armed, then become 16-bit operands in registers.
template <int HD>
__device__ __forceinline__ int fp8_key(int r) { return HD == 64 ? (r >> 2) & 3 : (r >> 1) & 7; }
template <int HD>
__device__ __forceinline__ int fp8_off(int r, int d) { return r * HD + ((((d >> 4) ^ fp8_key<HD>(r)) << 4) | (d & 15)); }

// the step's new key (rotated, rounded to the 16-bit type) and value of (b, kvh): quantized as gar_kv_quantize_fp8 does,
// appended at cache row `pos` with their scales, and patched into the wave's LDS tile (row pos & 63). Every lane calls it.
template <int HD>
__device__ __forceinline__ void append_new_kv_fp8(const decode_qkv_args& fa, uint8_t* Kp, uint8_t* Vp, float* Ksp, float* Vsp,
                                                  char* buf, char* sbuf, int b, int Hq, int Hkv, int kvh, int lane, int pos,
                                                  int rp) {
    constexpr int HALF = HD / 2, TB = 64 * HD;
    const int r = pos & 63;
    const bf16_t* row = fa.raw + (int64_t)b * (Hq + 2 * Hkv) * HD;
    const bool kl = lane < HALF / 8, vl = lane < HD / 8;
    const int i8 = (lane & (HD / 8 - 1)) * 8;
    float x1[8], x2[8], v[8];
    float ka = 0.f, va = 0.f;
    if (kl) {
        const bf16_t* rk = row + (Hq + kvh) * HD;
        float c[8], sv[8];
        ld8(rk + strip_col_d<HD>(i8, fa.strip), x1);
        ld8(rk + strip_col_d<HD>(HALF + i8, fa.strip), x2);
        ld8(fa.cs + (int64_t)rp * HALF + i8, c);
        ld8(fa.sn + (int64_t)rp * HALF + i8, sv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            rope_half_pair(x1[e], x2[e], c[e], sv[e], 1.0f, x1[e], x2[e]);
            x1[e] = unpk_lo(pack_bf2(x1[e], 0.f));             // the 16-bit key gar_attention_decode_qkv would append
            x2[e] = unpk_lo(pack_bf2(x2[e], 0.f));
            ka = fmaxf(ka, fmaxf(fabsf(x1[e]), fabsf(x2[e])));
        }
    }
    if (vl) {
        ld8(row + (Hq + Hkv + kvh) * HD + i8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) va = fmaxf(va, fabsf(v[e]));
    }
#pragma unroll
    for (int o = 1; o < HD / 8; o <<= 1) {
        ka = fmaxf(ka, __shfl_xor(ka, o, 64));
        va = fmaxf(va, __shfl_xor(va, o, 64));
    }
    const float kinv = FP8_MAX / ka, vinv = FP8_MAX / va;
    const bool klive = kinv < INFINITY, vlive = vinv < INFINITY;        // as gar_kv_quantize_fp8
    if (kl) {
        u32x2 w1 = {pk4_fp8(x1[0] * kinv, x1[1] * kinv, x1[2] * kinv, x1[3] * kinv),
                    pk4_fp8(x1[4] * kinv, x1[5] * kinv, x1[6] * kinv, x1[7] * kinv)};
        u32x2 w2 = {pk4_fp8(x2[0] * kinv, x2[1] * kinv, x2[2] * kinv, x2[3] * kinv),
                    pk4_fp8(x2[4] * kinv, x2[5] * kinv, x2[6] * kinv, x2[7] * kinv)};
        const u32x2 z = {0u, 0u};
        if (!klive) { w1 = z; w2 = z; }
        *reinterpret_cast<u32x2*>(Kp + (int64_t)pos * HD + i8) = w1;
        *reinterpret_cast<u32x2*>(Kp + (int64_t)pos * HD + HALF + i8) = w2;
        *reinterpret_cast<u32x2*>(buf + fp8_off<HD>(r, i8)) = w1;
        *reinterpret_cast<u32x2*>(buf + fp8_off<HD>(r, HALF + i8)) = w2;
    }
    if (vl) {
        u32x2 w = {pk4_fp8(v[0] * vinv, v[1] * vinv, v[2] * vinv, v[3] * vinv),
                   pk4_fp8(v[4] * vinv, v[5] * vinv, v[6] * vinv, v[7] * vinv)};
        if (!vlive) w = u32x2{0u, 0u};
        *reinterpret_cast<u32x2*>(Vp + (int64_t)pos * HD + i8) = w;
        *reinterpret_cast<u32x2*>(buf + TB + fp8_off<HD>(r, i8)) = w;
    }
    if (lane == 0) {
        const float sk = klive ? ka / FP8_MAX : 0.f, sv = vlive ? va / FP8_MAX : 0.f;
        Ksp[pos] = sk;
        Vsp[pos] = sv;
        reinterpret_cast<float*>(sbuf)[r] = sk;
        reinterpret_cast<float*>(sbuf + 256)[r] = sv;
    }
    asm volatile("" ::: "memory");          // the fragment reads that follow stay behind the patch
}

template <int HD>
__global__ __launch_bounds__(256, HD == 64 ? 2 : 1) void decode_attn_fp8_kernel(const bf16_t* __restrict__ Q, uint8_t* K8, uint8_t* V8,
                                                                               float* Ks, float* Vs, float* __restrict__ part,
                                                                               int Hq, int Hkv, int kv_stride,
                                                                               const int32_t* __restrict__ kv_len_dev,
                                                                               const int32_t* __restrict__ kv_start,
                                                                               bf16_t* __restrict__ O_direct, const decode_qkv_args fa,
                                                                               int64_t q_stride) {
    constexpr int NKD = HD / 16, NDB = HD / 32;
    constexpr int TB = 64 * HD;                 // bytes of a K (or V) tile
    constexpr int WAVE_LDS = 2 * 2 * TB + 3 * 512;  // [2 stages][K tile | V tile], [3][64 K scales | 64 V scales]
    constexpr int NP = TB / 1024;               // 1-KiB DMA pieces per tile
    constexpr int NPS = 2 * NP + 2;             // DMA instructions per stage
    constexpr int CPR = HD / 16;                // 16-byte chunks per row
    extern __shared__ __attribute__((aligned(16))) char smem[];     // [4 waves][WAVE_LDS] then red
    float (*red)[8][HD + 2] = reinterpret_cast<float (*)[8][HD + 2]>(smem + 4 * WAVE_LDS);
    const int kv_len = kv_len_dev[0] + (fa.raw ? 1 : 0);            // fused: kv_len_dev is the step's position, the new row included
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const int split = blockIdx.x, nsplit = gridDim.x, kvh = blockIdx.y, b = blockIdx.z;
    const int G = Hq / Hkv;
    const int ntiles = (kv_len + 63) / 64;
    const int kv_lo = kv_start ? max(min(kv_start[b], kv_len - 1), 0) : 0;
    const int t_lo = kv_lo >> 6;
    const int per = (ntiles - t_lo + nsplit - 1) / nsplit;
    const int t0 = t_lo + split * per, t1 = min(ntiles, t0 + per);
    const int64_t sl = (int64_t)b * Hkv + kvh;
    uint8_t* Kp = K8 + sl * (int64_t)kv_stride * HD;
    uint8_t* Vp = V8 + sl * (int64_t)kv_stride * HD;
    float* Ksp = Ks + sl * (int64_t)kv_stride;
    float* Vsp = Vs + sl * (int64_t)kv_stride;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc((void*)Kp, 0, kv_stride * HD, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc((void*)Vp, 0, kv_stride * HD, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsKs = __builtin_amdgcn_make_buffer_rsrc((void*)Ksp, 0, kv_stride * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsVs = __builtin_amdgcn_make_buffer_rsrc((void*)Vsp, 0, kv_stride * 4, 0x00020000);
    char* region = smem + wave * WAVE_LDS;
    char* sregion = region + 4 * TB;
    // DMA piece i: rows i * (64 / CPR) + lane / CPR, LDS chunk position lane % CPR <- global chunk position ^ key(row); the
    // key of such a row depends on i only through its parity (HD 128) or not at all (HD 64)
    int offs[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int r = par * (64 / CPR) + lane / CPR;
        offs[par] = r * HD + (((lane % CPR) ^ fp8_key<HD>(r)) << 4);
    }
    auto stage = [&](int t, char* dst, char* sdst) {
        const int tb = t * TB;
#pragma unroll
        for (int i = 0; i < NP; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, LDS_AS(dst + i * 1024), 16, offs[i & 1] + (tb + (i & ~1) * 1024), 0, 0,
                                                     DA_KV_AUX);
#pragma unroll
        for (int i = 0; i < NP; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, LDS_AS(dst + TB + i * 1024), 16, offs[i & 1] + (tb + (i & ~1) * 1024), 0, 0,
                                                     DA_KV_AUX);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsKs, LDS_AS(sdst), 4, (t * 64 + lane) * 4, 0, 0, DA_KV_AUX);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsVs, LDS_AS(sdst + 256), 4, (t * 64 + lane) * 4, 0, 0, DA_KV_AUX);
    };
    bf16x8 qf[NKD];
    const int rp = max(kv_len - 1 - (kv_start ? kv_start[b] : 0), 0);         // fused: RoPE position of the step's token
    if (fa.raw) {
        load_q_rotated<HD>(qf, fa, b, Hq, Hkv, kvh * G + min(l31, G - 1), l31 < G, h, rp);
    } else {
        const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        const bf16_t* qp = Q + ((int64_t)b * Hq + kvh * G + min(l31, G - 1)) * q_stride;
#pragma unroll
        for (int kd = 0; kd < NKD; ++kd)
            qf[kd] = l31 < G ? *reinterpret_cast<const bf16x8*>(qp + kd * 16 + h * 8) : z;
    }
    f32x16 o[NDB];
#pragma unroll
    for (int d = 0; d < NDB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int prow = (l31 & 0x13) | ((l31 & 4) << 1) | ((l31 & 8) >> 1);
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // fragment addresses as lane base + compile-time offset (the swizzle key of a row is a lane part XOR a constant):
    //   K: row blk*32 + prow (key(row + 32) = key(row)), bytes kd*16 + 8h .. +7
    //   V: rows c4*16 + 8h + e, column d*32 + l31: chunk (2d + l31/16) ^ key, key = 2h + e/4 (HD 64) / 4h + e/2 (HD 128)
    int kaddr[NKD], vaddr[2 * NDB];
#pragma unroll
    for (int kd = 0; kd < NKD; ++kd) kaddr[kd] = fp8_off<HD>(prow, kd * 16 + h * 8);
    {
        const int lanepart = (l31 >> 4) ^ (HD == 64 ? 2 * h : 4 * h);
#pragma unroll
        for (int c = 0; c < 2 * NDB; ++c) vaddr[c] = TB + 8 * h * HD + ((lanepart ^ c) << 4) + (l31 & 15);
    }

    int t = t0 + wave;
    if (t < t1) stage(t, region, sregion);
    if (t + 4 < t1) stage(t + 4, region + 2 * TB, sregion + 512);
    for (int it = 0, s3 = 0; t < t1; t += 4, ++it, s3 = s3 == 2 ? 0 : s3 + 1) {
        char* buf = region + (it & 1) * 2 * TB;
        char* sbuf = sregion + s3 * 512;
        if (t + 4 < t1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPS) : "memory");      // tile t in; tile t + 4 may be out
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (fa.raw && t == ntiles - 1)           // the tile that holds the step's own row (nothing behind it in flight)
            append_new_kv_fp8<HD>(fa, Kp, Vp, Ksp, Vsp, buf, sbuf, b, Hq, Hkv, kvh, lane, kv_len - 1, rp);
        u32x2 kr[2][NKD], vr[NDB][4];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kd = 0; kd < NKD; ++kd)
                kr[blk][kd] = *reinterpret_cast<const u32x2*>(buf + kaddr[kd] + blk * 32 * HD);
#pragma unroll
        for (int d = 0; d < NDB; ++d)
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
                unsigned int by[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    by[e] = *reinterpret_cast<const uint8_t*>(buf + vaddr[(2 * d) ^ (HD == 64 ? e >> 2 : e >> 1)] + (c4 * 16 + e) * HD);
                vr[d][c4] = u32x2{by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24),
                                  by[4] | (by[5] << 8) | (by[6] << 16) | (by[7] << 24)};
                __builtin_amdgcn_sched_barrier(0);  // pack as the bytes arrive: 8 VGPRs of bytes live, not 8 x HD / 8
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (t + 8 < t1) stage(t + 8, buf, sregion + (s3 == 0 ? 2 : s3 - 1) * 512);   // re-arm: tile t's bytes are in registers now
        __builtin_amdgcn_sched_barrier(0);
        // [blk][g][half]: scales of kv blk*32 + g*16 + 8h + 4 half + 0..3 (K scales at sbuf, V scales at sbuf + 256)
        auto ld_scales = [&](f32x4 (&sc)[2][2][2], const char* p) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf)
                        sc[blk][g][hf] = *reinterpret_cast<const f32x4*>(p + (blk * 32 + g * 16 + h * 8 + hf * 4) * 4);
        };
        f32x4 sk[2][2][2];
        ld_scales(sk, sbuf);
        const int kv0 = t * 64;
        f32x16 s[2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int kd = 0; kd < NKD; ++kd)
                s[blk] = MFMA_32x32x16(fp8x8_to_h16(kr[blk][kd]), qf[kd], kd == 0 ? zero16 : s[blk]);
        // s[blk][r] is kv kv0 + blk*32 + 16 (r >> 3) + 8h + (r & 7): scale, then mask (a masked row's scale may be anything)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[blk][r] *= sk[blk][r >> 3][(r >> 2) & 1][r & 3];
        __builtin_amdgcn_sched_barrier(0);      // the V scales load behind the K scales' last use (VGPRs)
        f32x4 svs[2][2][2];
        ld_scales(svs, sbuf + 256);
        if (kv0 + 64 > kv_len || kv0 < kv_lo) {
#pragma unroll
            for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kv0 + blk * 32 + ((r >> 3) << 4) + h * 8 + (r & 7);
                    s[blk][r] = (kv < kv_len && kv >= kv_lo) ? s[blk][r] : -INFINITY;
                }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[blk][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        m_run = m_new;
        float ps = 0.f;
        bf16x8 pf[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            float p[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = __builtin_amdgcn_exp2f(s[blk][r] - m_use);
                ps += pr;
                p[r] = pr * svs[blk][r >> 3][(r >> 2) & 1][r & 3];
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                u32x4 w;
                w[0] = cvt_pk_d(p[tt * 8 + 0], p[tt * 8 + 1]);
                w[1] = cvt_pk_d(p[tt * 8 + 2], p[tt * 8 + 3]);
                w[2] = cvt_pk_d(p[tt * 8 + 4], p[tt * 8 + 5]);
                w[3] = cvt_pk_d(p[tt * 8 + 6], p[tt * 8 + 7]);
                pf[blk][tt] = __builtin_bit_cast(bf16x8, w);
            }
        }
        l_run = l_run * alpha + ps;
        pv_update(o, vr, pf, alpha, [](u32x2 w) { return fp8x8_to_h16(w); });
    }
    merge_waves_store<HD>(o, m_run, l_run, red, part, O_direct, tid, wave, l31, h, b, Hq, Hkv, kvh, G, split, nsplit);
}

static int launch_decode_fp8(const char* what, const void* q, int64_t q_stride, void* K8, void* V8, float* Ks, float* Vs, void* O,
                             int B, int Hq, int Hkv, int hd, int Smax, const int32_t* kv_len_dev, const int32_t* kv_start,
                             int max_splits, void* workspace, const decode_qkv_args& fa, gar_stream_t stream) {
    GAR_CHECK_ARG(((uintptr_t)K8 & 15) == 0 && ((uintptr_t)V8 & 15) == 0 && ((uintptr_t)Ks & 15) == 0 && ((uintptr_t)Vs & 15) == 0,
                  "%s: caches and scale planes must be 16-byte aligned", what);
    if (hd == 64)
        return launch_split_kv<64, decode_attn_fp8_kernel<64>, decode_lds_bytes(4 * 64 * 64 + 3 * 512, 64)>(
            what, 1, q, q_stride, O, B, Hq, Hkv, Smax, kv_len_dev, kv_start, max_splits, workspace, fa, stream, (uint8_t*)K8,
            (uint8_t*)V8, Ks, Vs);
    return launch_split_kv<128, decode_attn_fp8_kernel<128>, decode_lds_bytes(4 * 64 * 128 + 3 * 512, 128)>(
        what, 1, q, q_stride, O, B, Hq, Hkv, Smax, kv_len_dev, kv_start, max_splits, workspace, fa, stream, (uint8_t*)K8,
        (uint8_t*)V8, Ks, Vs);
}

extern "C" int64_t gar_attention_decode_fp8_workspace(int B, int Hq, int hd, int max_splits) {
    return gar_attention_decode_workspace(B, Hq, hd, max_splits);
}

extern "C" int gar_attention_decode_fp8(int dtype, const void* q, int64_t q_stride, const void* Kc8, const void* Vc8, const float* Ks,
                                        const float* Vs, void* O, int B, int Hq, int Hkv, int hd, int Smax, const int32_t* kv_len_dev,
                                        const int32_t* kv_start, int max_splits, void* workspace, gar_stream_t stream) {
    GAR_CHECK_ARG(q && Kc8 && Vc8 && Ks && Vs && O && kv_len_dev, "attention_decode_fp8: null pointer");
    GAR_CHECK_ARG(dtype == GAR_BF16, "attention_decode_fp8: 16-bit query only (the fp8 cache has no parity mode)");
    if (int e = check_decode_args("attention_decode_fp8", q, &q_stride, B, Hq, Hkv, hd, Smax)) return e;
    const decode_qkv_args none = {nullptr, nullptr, nullptr, 0.f, 0};
    return launch_decode_fp8("attention_decode_fp8", q, q_stride, const_cast<void*>(Kc8), const_cast<void*>(Vc8),
                             const_cast<float*>(Ks), const_cast<float*>(Vs), O, B, Hq, Hkv, hd, Smax, kv_len_dev, kv_start, max_splits,
                             workspace, none, stream);
}

extern "C" int gar_attention_decode_qkv_fp8(int dtype, const void* qkv, const float* cos, const float* sin, void* Kc8, void* Vc8,
                                            float* Ks, float* Vs, void* O, int B, int Hq, int Hkv, int hd, int Smax,
                                            const int32_t* pos_dev, const int32_t* left_pad, float q_scale, int qk_strip_order,
                                            int max_splits, void* workspace, gar_stream_t stream) {
    GAR_CHECK_ARG(qkv && cos && sin && Kc8 && Vc8 && Ks && Vs && O && pos_dev, "attention_decode_qkv_fp8: null pointer");
    GAR_CHECK_ARG(dtype == GAR_BF16, "attention_decode_qkv_fp8: 16-bit qkv only (the fp8 cache has no parity mode)");
    if (int e = check_decode_args("attention_decode_qkv_fp8", qkv, nullptr, B, Hq, Hkv, hd, Smax)) return e;
    const decode_qkv_args fa = {(const bf16_t*)qkv, cos, sin, q_scale, qk_strip_order ? 1 : 0};
    return launch_decode_fp8("attention_decode_qkv_fp8", nullptr, hd, Kc8, Vc8, Ks, Vs, O, B, Hq, Hkv, hd, Smax, pos_dev,
                             left_pad, max_splits, workspace, fa, stream);
}
