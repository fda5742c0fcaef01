// fp8 KV cache of the fp8 serving path: the cache writer and the expansion back to bf16.  The reader of a decode step is
// attn_decode_kernel over a CacheFp8 (attention.hip): the bf16 kernel's body with DecodeTile<HS, CacheFp8> as its tile.
//
// Scheme (include/dualhyp_hip.h, common.h): per (token, KV group) one K vector (after rope) and one V vector of head_size bf16
// values each become head_size e4m3fn bytes and one int8 exponent e, the smallest with amax <= 448 * 2^e; byte = e4m3fn_rne(x * 2^-e).
// e4m3 * 2^e is exactly representable in bf16, so attention over this cache IS the bf16 attention over its expansion.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------ QKV split + RoPE + fp8 cache
// qkv_rope_cache_kernel (elementwise.hip) with the cache writes replaced: same grid (ceil(n_tok/64), n_groups), 256 threads, the
// same rope step (common.h rope_chunk_pair).  The rotated k rows and the v rows of the block's 64 tokens wait in LDS for their exponents.
template <int HS>
__global__ __launch_bounds__(256) void qkv_rope_cache_kv8_kernel(
    const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ cos, const bf16_t* __restrict__ sin,
    const int32_t* __restrict__ tok_slot, const int32_t* __restrict__ tok_pos, bf16_t* __restrict__ q_out,
    uint8_t* __restrict__ k8, uint8_t* __restrict__ v8, int8_t* __restrict__ k_exp, int8_t* __restrict__ v_exp,
    int n_tok, int n_head, int n_groups, int s_max) {
    constexpr int HALF = HS / 2;
    constexpr int CPH = HALF / 8;              // 16-B chunk pairs per head
    const int g = blockIdx.y;
    const int t0 = blockIdx.x * 64;
    const int q_per_kv = n_head / n_groups;
    const int row_elems = n_groups * (q_per_kv + 2) * HS;
    const int grp_off = g * (q_per_kv + 2) * HS;
    __shared__ __attribute__((aligned(16))) bf16_t rows[2][64][HS + 8];   // [0]: rotated k, [1]: v
    __shared__ int sexp[2][64];

    // phase 1: rotate q heads and k; q -> q_out, k -> LDS
    const int items = 64 * (q_per_kv + 1) * CPH;
    for (int it = threadIdx.x; it < items; it += 256) {
        const int c = it % CPH;
        const int j = (it / CPH) % (q_per_kv + 1);   // 0..q_per_kv-1: q head, q_per_kv: k
        const int tl = it / (CPH * (q_per_kv + 1));
        const int t = t0 + tl;
        if (t >= n_tok) continue;
        const int pos = tok_pos[t];
        const bf16_t* src = qkv + (size_t)t * row_elems + grp_off + j * HS;
        uint4 o1, o2;
        rope_chunk_pair<HS>(src, cos, sin, pos, c * 8, o1, o2);
        if (j < q_per_kv) {
            bf16_t* dst = q_out + ((size_t)t * n_head + g * q_per_kv + j) * HS;
            *reinterpret_cast<uint4*>(dst + c * 8) = o1;
            *reinterpret_cast<uint4*>(dst + HALF + c * 8) = o2;
        } else {
            *reinterpret_cast<uint4*>(&rows[0][tl][c * 8]) = o1;
            *reinterpret_cast<uint4*>(&rows[0][tl][HALF + c * 8]) = o2;
        }
    }
    for (int it = threadIdx.x; it < 64 * (HS / 8); it += 256) {
        const int c = it % (HS / 8), tl = it / (HS / 8);
        const int t = t0 + tl;
        if (t < n_tok)
            *reinterpret_cast<uint4*>(&rows[1][tl][c * 8]) =
                *reinterpret_cast<const uint4*>(qkv + (size_t)t * row_elems + grp_off + (q_per_kv + 1) * HS + c * 8);
    }
    __syncthreads();

    // phase 2: one thread per vector: amax over the bf16 magnitudes (as integers), the exponent, its int8 store
    if (threadIdx.x < 128) {
        const int which = threadIdx.x >> 6, tl = threadIdx.x & 63, t = t0 + tl;
        if (t < n_tok) {
            uint32_t amax = 0;
#pragma unroll
            for (int c = 0; c < HS / 8; ++c) {
                const uint4 u = *reinterpret_cast<const uint4*>(&rows[which][tl][c * 8]);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    amax = max(amax, w[i] & 0x7fffu);
                    amax = max(amax, (w[i] >> 16) & 0x7fffu);
                }
            }
            const int e = kv8_exponent(amax);
            sexp[which][tl] = e;
            (which ? v_exp : k_exp)[((size_t)tok_slot[t] * n_groups + g) * s_max + tok_pos[t]] = (int8_t)e;
        }
    }
    __syncthreads();

    // phase 3: K bytes, 8 aligned channels = one 8-B store into the fragment layout
    for (int it = threadIdx.x; it < 64 * (HS / 8); it += 256) {
        const int c = it % (HS / 8), tl = it / (HS / 8);
        const int t = t0 + tl;
        if (t >= n_tok) continue;
        const uint4 u = *reinterpret_cast<const uint4*>(&rows[0][tl][c * 8]);
        const bf16_t* p = reinterpret_cast<const bf16_t*>(&u);
        const float inv = kv8_pow2(-sexp[0][tl]);
        const uint2 o = make_uint2(kv8_pack4(kv8_scaled(p[0], inv), kv8_scaled(p[1], inv), kv8_scaled(p[2], inv), kv8_scaled(p[3], inv)),
                                   kv8_pack4(kv8_scaled(p[4], inv), kv8_scaled(p[5], inv), kv8_scaled(p[6], inv), kv8_scaled(p[7], inv)));
        uint8_t* kb = k8 + ((size_t)tok_slot[t] * n_groups + g) * s_max * HS;
        *reinterpret_cast<uint2*>(kb + k8_off<HS>(tok_pos[t], c * 8)) = o;
    }
    // V bytes: the 8 bytes of a V^T run belong to 8 tokens (adjacent lanes = adjacent tokens, as in the bf16 kernel)
    for (int it = threadIdx.x; it < 64 * HS; it += 256) {
        const int tl = it & 63, dd = it >> 6;
        const int t = t0 + tl;
        if (t < n_tok) {
            const float y = kv8_scaled(rows[1][tl][dd], kv8_pow2(-sexp[1][tl]));
            v8[((size_t)tok_slot[t] * n_groups + g) * HS * s_max + v8_off<HS>(tok_pos[t], dd)] =
                (uint8_t)__builtin_amdgcn_cvt_pk_fp8_f32(y, 0.f, 0, false);
        }
    }
}

// ------------------------------------------------------------------------------ expansion to the bf16 fragment layout
// grid (s_max / 32 tiles, n_groups, n_seq), 256 threads: tile t of (seq_slot[seq], group) if it holds a position < len, written
// whole (positions >= len of the last tile as +0.0 bits); a thread converts 8 bytes into one 16-B store of the bf16 layout.
template <int HS>
__global__ __launch_bounds__(256) void kv8_expand_kernel(
    const uint8_t* __restrict__ k8, const uint8_t* __restrict__ v8, const int8_t* __restrict__ k_exp, const int8_t* __restrict__ v_exp,
    const int32_t* __restrict__ seq_slot, const int32_t* __restrict__ kv_len, const int32_t* __restrict__ kv_extra,
    bf16_t* __restrict__ k_out, bf16_t* __restrict__ vT_out, int n_groups, int s_max) {
    const int t = blockIdx.x, g = blockIdx.y, seq = blockIdx.z;
    int len = kv_len ? kv_len[seq] + (kv_extra ? kv_extra[seq] : 0) : s_max;
    len = len < s_max ? len : s_max;
    if (t * 32 >= len) return;
    const size_t blk = (size_t)seq_slot[seq] * n_groups + g;
    const uint8_t *kb = k8 + blk * s_max * HS, *vb = v8 + blk * s_max * HS;
    const int8_t *ke = k_exp + blk * s_max, *ve = v_exp + blk * s_max;
    bf16_t *ko = k_out + blk * s_max * HS, *vo = vT_out + blk * s_max * HS;
    for (int it = threadIdx.x; it < 32 * (HS / 8); it += 256) {
        const int key = t * 32 + (it & 31), d0 = (it >> 5) * 8;
        const uint2 b = *reinterpret_cast<const uint2*>(kb + k8_off<HS>(key, d0));
        const float s = kv8_pow2(ke[key]);
        uint4 o;
        kv8_cvt4(b.x, s, s, s, s, o.x, o.y);
        kv8_cvt4(b.y, s, s, s, s, o.z, o.w);
        if (key >= len) o = make_uint4(0, 0, 0, 0);          // zero BITS, whatever stale bytes the position holds
        *reinterpret_cast<uint4*>(ko + kfrag_off<HS>(key, d0)) = o;
    }
    for (int it = threadIdx.x; it < HS * 4; it += 256) {
        const int d = it % HS, s2 = (it / HS) >> 1, lh = (it / HS) & 1;
        const int key0 = t * 32 + 16 * s2 + 4 * lh;          // keys key0 + 0..3 and key0 + 8 + 0..3
        const uint2 b = *reinterpret_cast<const uint2*>(vb + v8_off<HS>(key0, d));
        float s[8];
        kv8_scales4(*reinterpret_cast<const uint32_t*>(ve + key0), s);
        kv8_scales4(*reinterpret_cast<const uint32_t*>(ve + key0 + 8), s + 4);
        uint32_t w[4];
        kv8_cvt4(b.x, s[0], s[1], s[2], s[3], w[0], w[1]);
        kv8_cvt4(b.y, s[4], s[5], s[6], s[7], w[2], w[3]);
#pragma unroll
        for (int j = 0; j < 8; ++j)                              // zero BITS for the keys >= len, whatever stale bytes they hold
            if (key0 + 8 * (j >> 2) + (j & 3) >= len) w[j >> 1] &= (j & 1) ? 0x0000ffffu : 0xffff0000u;
        const uint4 o = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(vo + vfrag_off<HS>(key0, d)) = o;
    }
}

}  // namespace

extern "C" int dh_qkv_rope_cache_kv8(const dh_bf16* qkv, const dh_bf16* cos, const dh_bf16* sin, const int32_t* tok_slot,
                                     const int32_t* tok_pos, dh_bf16* q_out, uint8_t* k8, uint8_t* v8, int8_t* k_exp, int8_t* v_exp,
                                     int n_tok, int n_head, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(qkv && cos && sin && tok_slot && tok_pos && q_out && k8 && v8 && k_exp && v_exp, "dh_qkv_rope_cache_kv8: null argument");
    DH_CHECK(n_tok >= 0 && n_groups > 0 && n_head % n_groups == 0, "dh_qkv_rope_cache_kv8: bad head counts");
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "dh_qkv_rope_cache_kv8: head_size %d unsupported (64, 96 or 128)", hs);
    DH_CHECK(s_max > 0 && s_max % 64 == 0, "dh_qkv_rope_cache_kv8: s_max must be a multiple of 64");
    if (n_tok == 0) return 0;
    dim3 grid(cdiv(n_tok, 64), n_groups), block(256);
    hipStream_t s = (hipStream_t)stream;
    dispatch_hs(hs, [&](auto hs_c) {
        hipLaunchKernelGGL((qkv_rope_cache_kv8_kernel<decltype(hs_c)::value>), grid, block, 0, s, qkv, cos, sin, tok_slot, tok_pos, q_out, k8,
                           v8, k_exp, v_exp, n_tok, n_head, n_groups, s_max);
    });
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_kv8_expand(const uint8_t* k8, const uint8_t* v8, const int8_t* k_exp, const int8_t* v_exp, const int32_t* seq_slot,
                             const int32_t* kv_len, const int32_t* kv_extra, dh_bf16* k_out, dh_bf16* vT_out, int n_seq, int n_groups,
                             int hs, int s_max, void* stream) {
    DH_CHECK(k8 && v8 && k_exp && v_exp && seq_slot && k_out && vT_out, "dh_kv8_expand: null argument");
    DH_CHECK(kv_len || !kv_extra, "dh_kv8_expand: kv_extra without kv_len");
    DH_CHECK(n_groups > 0, "dh_kv8_expand: bad group count");
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "dh_kv8_expand: head_size %d unsupported (64, 96 or 128)", hs);
    DH_CHECK(s_max > 0 && s_max % 64 == 0, "dh_kv8_expand: s_max must be a multiple of 64");
    if (n_seq <= 0) return 0;
    dim3 grid(s_max / 32, n_groups, n_seq), block(256);
    hipStream_t s = (hipStream_t)stream;
    dispatch_hs(hs, [&](auto hs_c) {
        hipLaunchKernelGGL((kv8_expand_kernel<decltype(hs_c)::value>), grid, block, 0, s, k8, v8, k_exp, v_exp, seq_slot, kv_len, kv_extra,
                           k_out, vT_out, n_groups, s_max);
    });
    DH_LAUNCH_CHECK();
    return 0;
}
