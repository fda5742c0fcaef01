// Fused kernels of the single-token decode step.  A decode layer is 7 launches:
//   partial GEMM [Wqkv;A]  ->  attn_decode_fused  ->  partial GEMM [Wproj;A]  ->  finish_norm
//   ->  SwiGLU GEMM  ->  partial GEMM Wmlp  ->  finish_norm (next layer's norm)
// The weight-streaming GEMMs (gemm_skinny.hip) emit fp32 partial sums; the LoRA update, the
// residual add, the rounding to bf16 and the RMSNorm are finished HERE, by the consumer, with
// exactly the reference's rounding points (ger/lora.py:159-166,388-402; ger/model.py:185-186,
// 216-259; ger/rmsnorm.py:17-21).  That removes the separate x·A^T launch and its dependent
// latency from the chain, lets small matrices be split over K across blocks, and folds
// rope + KV-cache append + split-KV attention + combine into one kernel.
#include "common.h"
#include "tuning.h"

// dh_set_tuning 40: the single-token attention kernel.  1 (default): attn_decode_chain_kernel where it applies (hs 64 and one
// finish item per thread); 0: attn_decode_fused_kernel everywhere (the A/B arm; both give the same bits).
int g_attn_chain = 1;
// dh_set_tuning 41: finish_norm requests its independent loads ahead of the hand-over barrier from this many rows on
// (0: never).  Chosen by the row count only.  Default and the sweep behind it: FINISH_HOIST_ROWS below.
int g_finish_hoist_rows = -1;
// dh_set_tuning 43: finish_norm_rows_kernel (several rows per block, loads a row ahead, lora_b in registers) from this many rows
// on; 0: finish_norm_kernel at every row count (the A/B arm; both give the same bits); -1: FINISH_ROWS_MIN below.
int g_finish_rows_min = -1;
// dh_set_tuning 44: rows per block of finish_norm_rows_kernel (0: FINISH_RPB below).
int g_finish_rpb = 0;

#ifdef DH_ATTN_STAMPS   // diagnostic build only (tools/probe_attn_chain.py): 100 MHz timestamps of thread 0 of each block
__device__ unsigned long long g_attn_stamps[4096 * 8];
#define ATTN_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 4096) g_attn_stamps[blockIdx.x * 8 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define ATTN_DRAIN() __builtin_amdgcn_s_waitcnt(0)      // every store of this wave acknowledged
extern "C" int dh_debug_attn_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_stamps), sizeof(g_attn_stamps)) == hipSuccess ? 0 : 1;
}
#else
#define ATTN_STAMP(i)
#define ATTN_DRAIN()
#endif

namespace {

constexpr int DCOLS = 16;   // padded head columns of the attention partials
constexpr int MAXP = 16;    // most K-slices a partial-sum GEMM emits

// --------------------------------------------------------------------------- attention (decode)
// grid (n_seq * n_groups), NW waves (8 at every head size: DH_ATTN_WAVES64 below; hs 96 needs 53 KiB of LDS, two blocks per CU).
// qkv32: [n_part][n_seq][ldq] fp32, ldq = qkv_dim + n_ext; columns [qkv_dim, qkv_dim+48) hold x·A^T of the q/k/v LoRA (when
// lora_b != null).  NW waves share the key tiles of one (sequence, group): at the benchmark's ~544 cached keys (17 tiles) a
// wave walks two tiles and wave 0 three, each after the first behind an exposed HBM round trip.  Sixteen waves at hs 64 (every
// tile requested before the LoRA / rope prologue, one block per CU) and six with two tiles in flight were built in round 3,
// measured slower per 640-row step and are A/B builds only (-DDH_ATTN_WAVES64=16 | 6).  The tile -> wave deal and the combine
// order are a property of the head size, never of the row count, so batch invariance is untouched.  At hs 64 this kernel is the
// A/B arm of attn_decode_chain_kernel below (dh_set_tuning 40) and serves the shapes that kernel does not take.
template <int HS, int PMAX, int NW>
__global__ __launch_bounds__(NW * 64, NW == 16 ? 1 : (NW == 6 ? 3 : (HS == 64 ? 4 : 2))) void attn_decode_fused_kernel(
    const float* __restrict__ qkv32, int n_part, int pairs, int n_seq, int ldq, int qkv_dim,
    const bf16_t* __restrict__ lora_b, float lora_scale, int split0, int split1,
    const bf16_t* __restrict__ cos, const bf16_t* __restrict__ sin, const int32_t* __restrict__ seq_slot,
    const int32_t* __restrict__ kv_len, bf16_t* __restrict__ k_cache, bf16_t* __restrict__ vT_cache,
    bf16_t* __restrict__ y, int n_head, int n_groups, int s_max, float scale) {
    constexpr int KS = HS / 16, DT = HS / 32, HALF = HS / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pair = blockIdx.x, seq = pair / n_groups, g = pair % n_groups;
    const int q_per_kv = n_head / n_groups;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int slot = seq_slot[seq];
    const int len = kv_len[seq], pos = len - 1;          // the new token sits at position len-1
    // LDS carve (all offsets multiples of 16 B)
    bf16_t* sQ = reinterpret_cast<bf16_t*>(smem);                       // [16][HS] rotated queries
    float* sKn = reinterpret_cast<float*>(smem + 16 * HS * 2);          // [HS] new key (bf16 values)
    float* sVn = sKn + HS;                                              // [HS] new value
    float* sXa = sVn + HS;                                              // [48] bf16(x·A^T)
    float* sSn = sXa + 48;                                              // [16] score of the new key
    float* sPm = sSn + 16;                                              // [NW][DCOLS] running max
    float* sPl = sPm + NW * DCOLS;                                      // [NW][DCOLS] running sum
    float* sPo = sPl + NW * DCOLS;                                      // [NW][HS][DCOLS] partial O^T
    constexpr int NT_ = NW * 64;                                        // threads
    ATTN_STAMP(0);

    // ---- request the K / V^T operands of this wave's first PF tiles before anything else: they do
    // not depend on the new token, and their HBM latency hides under the LoRA/rope phase
    // tiles of operands in flight per wave.  8 waves: one (128 VGPRs, two blocks per CU at hs 64); SIX waves (round 3, hs 64): two —
    // three waves per SIMD leave 168 VGPRs, and at ~544 keys (17 tiles = 3 per wave) the third tile's loads are issued right
    // after the first tile is consumed and land under the second: no tile waits for an exposed HBM round trip
    constexpr int PF = NW == 6 ? 2 : 1;
    struct VF { bf16x8 v; };
    struct Tile { bf16x8 kf[KS]; VF vf[DT][2]; };
    Tile tl[PF];
    const bf16_t* kbase = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    const bf16_t* vbase = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    const int n_tiles = (pos + 31) / 32;
    // the caches are in MFMA-fragment order (common.h): a tile is 8 coalesced 1-KiB loads
    auto load_tile = [&](Tile& T, int t) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            T.kf[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kbase + kfrag_blk<HS>(t, ks) + lane * 8));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                T.vf[dt][s2].v = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vbase + vfrag_blk<HS>(t, dt, s2) + lane * 8));
    };
#pragma unroll
    for (int p = 0; p < PF; ++p)
        if (wave + NW * p < n_tiles) load_tile(tl[p], wave + NW * p);

    const float* row0 = qkv32 + (size_t)seq * ldq;
    const size_t pstride = (size_t)n_seq * ldq;
    // all partial loads are issued before the first add (a runtime-trip-count loop would wait
    // for one L2 round trip per partial)
    auto psum = [&](int c) {
        float v[PMAX];
#pragma unroll
        for (int p = 0; p < PMAX; ++p) v[p] = p < n_part ? row0[p * pstride + c] : 0.f;
        // the decode family's summation order (common.h, "K-slice combine"): leaves are added in adjacent PAIRS, the
        // pair sums in index order; a producer that owns two slices per block has already formed the pairs (pairs == 0)
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < PMAX; p += 2) s += v[p] + v[p + 1];
        } else {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s += v[p];
        }
        return s;
    };
    if (lora_b != nullptr && tid < 48) sXa[tid] = rbf(psum(qkv_dim + tid));
    for (int i = tid; i < 16 * HS; i += NT_) sQ[i] = 0;               // zero padding rows of Q
    __syncthreads();
    ATTN_STAMP(1);

    // bf16 value of fused-qkv column c: bf16(bf16(x·W^T) + bf16(bf16(xa·B^T)*s))
    auto finish = [&](int c) -> float {
        float o = rbf(psum(c));
        if (lora_b != nullptr) {
            const int seg = (c >= split0) + (c >= split1);
            const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)c * 16);
            float l = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 bv = b4[h];
                const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                for (int e = 0; e < 8; ++e) l = fmaf(sXa[seg * 16 + h * 8 + e], bf2f(bp[e]), l);
            }
            o = rbf(o + rbf(rbf(l) * lora_scale));
        }
        return o;
    };
    const int gbase = g * (q_per_kv + 2) * HS;
    bf16_t* kdst = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    bf16_t* vdst = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    const int n_rope = (q_per_kv + 1) * HALF;
    for (int it = tid; it < n_rope + HS; it += NT_) {
        if (it < n_rope) {
            const int j = it / HALF, i = it % HALF;
            const float x1 = finish(gbase + j * HS + i), x2 = finish(gbase + j * HS + HALF + i);
            const bf16_t* cp = cos + (size_t)pos * HS;
            const bf16_t* sp = sin + (size_t)pos * HS;
            const bf16_t o1 = f2bf(rbf(x1 * bf2f(cp[i])) + rbf(-x2 * bf2f(sp[i])));
            const bf16_t o2 = f2bf(rbf(x2 * bf2f(cp[HALF + i])) + rbf(x1 * bf2f(sp[HALF + i])));
            if (j < q_per_kv) {
                sQ[j * HS + i] = o1;
                sQ[j * HS + HALF + i] = o2;
            } else {
                sKn[i] = bf2f(o1);
                sKn[HALF + i] = bf2f(o2);
                kdst[kfrag_off<HS>(pos, i)] = o1;
                kdst[kfrag_off<HS>(pos, HALF + i)] = o2;
            }
        } else {
            const int e = it - n_rope;
            const bf16_t v = f2bf(finish(gbase + (q_per_kv + 1) * HS + e));
            sVn[e] = bf2f(v);
            vdst[vfrag_off<HS>(pos, e)] = v;
        }
    }
    __syncthreads();
    ATTN_STAMP(2);

    // score of the new key against each head (it is merged at the combine, so nobody has to
    // read this block's own cache write back)
    for (int h = wave; h < q_per_kv; h += NW) {
        float p = 0.f;
        for (int e = lane; e < HS; e += 64) p += bf2f(sQ[h * HS + e]) * sKn[e];
        p = wave_sum(p);
        if (lane == 0) sSn[h] = p * scale;
    }

    // ---- keys 0 .. pos-1 straight from the cache, 32-key tiles dealt over the 8 waves; the
    // operands of two tiles per wave were requested before the LoRA/rope phase (tl[] above)
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + (lr & 15) * HS + ks * 16 + lh * 8);
    if (lr >= 16) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    auto compute_tile = [&](const Tile& T, int t) {
        const int key0 = t * 32;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.kf[ks], qf[ks], st, 0, 0, 0);
        float m_t = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key_abs = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float sc = st[r] * scale;
            sc = key_abs < pos ? sc : -INFINITY;
            st[r] = sc;
            m_t = fmaxf(m_t, sc);
        }
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float psm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(st[r] - m_new);
            st[r] = p;
            psm += p;
        }
        l_run = l_run * alpha + psm;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (s2 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
                // keys >= pos carry p == 0 and the cache beyond the written prefix is finite
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.vf[dt][s2].v, pf.v, o[dt], 0, 0, 0);
            }
        }
    };
    for (int base = wave; base < n_tiles; base += NW * PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            if (base + NW * p < n_tiles) compute_tile(tl[p], base + NW * p);
            if (base + NW * (PF + p) < n_tiles) load_tile(tl[p], base + NW * (PF + p));    // its set is free again
        }
#ifdef DH_ATTN_STAMPS
        if (base == wave) { asm volatile("" :: "v"(o[0][0])); ATTN_STAMP(3); }
#endif
    }
#ifdef DH_ATTN_STAMPS
    asm volatile("" :: "v"(o[0][0]));
#endif
    ATTN_STAMP(4);
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (lr < q_per_kv) {
        if (lh == 0) {
            sPm[wave * DCOLS + lr] = m_run;
            sPl[wave * DCOLS + lr] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sPo[(wave * HS + d) * DCOLS + lr] = o[dt][r];
            }
    }
    __syncthreads();
    ATTN_STAMP(5);
    // ---- combine the NW wave partials and the new key
    for (int it = tid; it < q_per_kv * HS; it += NT_) {
        const int h = it / HS, d = it % HS;
        const float sn = sSn[h];
        float M = sn;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sPm[w * DCOLS + h]);
        const float pn = __expf(sn - M);
        float L = pn, O = rbf(pn) * sVn[d];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sPm[w * DCOLS + h];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += sPl[w * DCOLS + h] * f;
            O += sPo[(w * HS + d) * DCOLS + h] * f;
        }
        y[(size_t)seq * n_head * HS + (g * q_per_kv + h) * HS + d] = f2bf(O / L);
    }
    ATTN_STAMP(6);
    ATTN_DRAIN();
    ATTN_STAMP(7);
}

// Round 3, one more shape measured and not kept (bit-identical, 82 tests green): every tile after a wave's first streamed through an 8-KiB LDS slot
// private to the wave, filled by LDS-DMA one tile ahead with the second tile's request issued at kernel start (the wave's partial-O block
// aliased into the slot: 69 KiB per block, two blocks per CU as before) — 4.71-4.73 ms per 640-row decode step against 4.58-4.64: the second
// tile's exposed round trip is not what the kernel waits for.
#ifndef DH_ATTN_WAVES64
#define DH_ATTN_WAVES64 8     // A/B builds: 6 (two tiles in flight per wave) and 16 (one block per CU: measured 5.68 vs 4.74 ms per 640-row step)
#endif
template <int HS>
constexpr int attn_fused_waves() { return HS == 64 ? DH_ATTN_WAVES64 : 8; }
template <int HS>
constexpr size_t attn_fused_lds() {
    constexpr int NW = attn_fused_waves<HS>();
    return 16 * HS * 2 + (HS + HS + 48 + 16 + NW * DCOLS + NW * DCOLS + NW * HS * DCOLS) * sizeof(float);
}

constexpr int CHAIN_NW = 8;      // attn_decode_chain_kernel's waves (an A/B build of the parent with 6 or 16 keeps the parent)
template <int HS>
constexpr size_t attn_chain_lds() {
    return 16 * HS * 2 + (HS + HS + 48 + 16 + CHAIN_NW * DCOLS + CHAIN_NW * DCOLS + CHAIN_NW * DCOLS * (HS + 8)) * sizeof(float);
}

// --------------------------------------------------------------------------- attention (decode), short chain
// attn_decode_fused_kernel with the head of each block's dependent chain shortened; the arithmetic, the tile -> wave deal, the
// per-tile update and the combine are that kernel's, statement for statement, so both give the same bits.  What differs is
// when things are asked for:
//   - a thread owns ONE item of the LoRA finish / rope / append phase (the host checks n_rope + HS <= threads), and every load
//     the item needs -- its fp32 partials, its rows of B, its cos / sin, and for 48 threads the x·A^T partials -- is requested
//     before the first barrier.  The old order summed x·A^T, crossed a barrier and only then requested the items' partials:
//     two memory round trips in sequence;
//   - those loads are requested BEFORE the K / V^T tile.  The memory counter retires in order: behind the tile's HBM loads
//     the first barrier also waited for the tile, and the finish phase started after it instead of under it;
//   - Q's padding rows are zeroed in the MFMA operand registers, not in LDS.
template <int HS, int PMAX, int NW>
__global__ __launch_bounds__(NW * 64, HS == 64 ? 4 : 2) void attn_decode_chain_kernel(
    const float* __restrict__ qkv32, int n_part, int pairs, int n_seq, int ldq, int qkv_dim,
    const bf16_t* __restrict__ lora_b, float lora_scale, int split0, int split1,
    const bf16_t* __restrict__ cos, const bf16_t* __restrict__ sin, const int32_t* __restrict__ seq_slot,
    const int32_t* __restrict__ kv_len, bf16_t* __restrict__ k_cache, bf16_t* __restrict__ vT_cache,
    bf16_t* __restrict__ y, int n_head, int n_groups, int s_max, float scale) {
    static_assert(NW == CHAIN_NW, "one tile in flight per wave and the occupancy asked for above are those of the 8-wave form");
    constexpr int KS = HS / 16, DT = HS / 32, HALF = HS / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pair = blockIdx.x, seq = pair / n_groups, g = pair % n_groups;
    const int q_per_kv = n_head / n_groups;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    // LDS carve: attn_decode_fused_kernel's
    bf16_t* sQ = reinterpret_cast<bf16_t*>(smem);                       // [16][HS] rotated queries (rows >= q_per_kv unused)
    float* sKn = reinterpret_cast<float*>(smem + 16 * HS * 2);          // [HS] new key (bf16 values)
    float* sVn = sKn + HS;                                              // [HS] new value
    float* sXa = sVn + HS;                                              // [48] bf16(x·A^T)
    float* sSn = sXa + 48;                                              // [16] score of the new key
    float* sPm = sSn + 16;                                              // [NW][DCOLS] running max
    float* sPl = sPm + NW * DCOLS;                                      // [NW][DCOLS] running sum
    float* sPo = sPl + NW * DCOLS;                                      // [NW][DCOLS][PST] partial O, head-major (see the combine)
    constexpr int PST = HS + 8;                                         // row stride: 8 lr x 2 lh writers of one d land in 16 banks
    constexpr int NT_ = NW * 64;
    ATTN_STAMP(0);

    const int slot = seq_slot[seq];
    const int len = kv_len[seq], pos = len - 1;          // the new token sits at position len-1

    // ---- this thread's finish item and every load it needs.  No load sits under a per-lane condition (a thread without an
    // item asks for a column that exists and drops it): a conditional load is waited for where the branches join.
    const float* row0 = qkv32 + (size_t)seq * ldq;
    const size_t pstride = (size_t)n_seq * ldq;
    auto pload = [&](int c, float (&v)[PMAX]) {
#pragma unroll
        for (int p = 0; p < PMAX; ++p) v[p] = p < n_part ? row0[p * pstride + c] : 0.f;
    };
    // the decode family's summation order (common.h, "K-slice combine"), as in attn_decode_fused_kernel
    auto padd = [&](const float (&v)[PMAX]) {
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < PMAX; p += 2) s += v[p] + v[p + 1];
        } else {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s += v[p];
        }
        return s;
    };
    const int gbase = g * (q_per_kv + 2) * HS;
    const int n_rope = (q_per_kv + 1) * HALF;
    const bool is_rope = tid < n_rope, is_val = !is_rope && tid < n_rope + HS;
    const int rj = tid / HALF, ri = tid % HALF, ve = tid - n_rope;
    const int c1 = is_rope ? gbase + rj * HS + ri : (is_val ? gbase + (q_per_kv + 1) * HS + ve : gbase);
    const int c2 = is_rope ? c1 + HALF : gbase;
    const bool has_xa = lora_b != nullptr && tid < 48;
    float vx[PMAX], v1[PMAX], v2[PMAX];
    uint4 b1[2], b2[2];
    pload(has_xa ? qkv_dim + tid : 0, vx);
    pload(c1, v1);
    pload(c2, v2);
    if (lora_b != nullptr) {
        const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)c1 * 16);
        b1[0] = b4[0]; b1[1] = b4[1];
        b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)c2 * 16);
        b2[0] = b4[0]; b2[1] = b4[1];
    } else {
        b1[0] = b1[1] = b2[0] = b2[1] = uint4{0, 0, 0, 0};
    }
    const bf16_t* cp = cos + (size_t)pos * HS;
    const bf16_t* sp = sin + (size_t)pos * HS;
    const bf16_t cs[4] = {cp[ri], sp[ri], cp[HALF + ri], sp[HALF + ri]};

    // ---- then the K / V^T operands of this wave's first tile (HBM; they land under the finish phase)
    struct VF { bf16x8 v; };
    struct Tile { bf16x8 kf[KS]; VF vf[DT][2]; };
    Tile tl;
    const bf16_t* kbase = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    const bf16_t* vbase = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    const int n_tiles = (pos + 31) / 32;
    auto load_tile = [&](Tile& T, int t) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            T.kf[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kbase + kfrag_blk<HS>(t, ks) + lane * 8));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                T.vf[dt][s2].v = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vbase + vfrag_blk<HS>(t, dt, s2) + lane * 8));
    };
    // unconditional, like the loads above: a wave without a tile asks for the last one there is (tile 0 of the slot's cache
    // when there is none: allocated, finite or not, never used)
    load_tile(tl, wave < n_tiles ? wave : (n_tiles > 0 ? n_tiles - 1 : 0));

    if (has_xa) sXa[tid] = rbf(padd(vx));
    __syncthreads();
    ATTN_STAMP(1);

    // bf16 value of a fused-qkv column c from its summed partials and its rows of B:
    // bf16(bf16(x·W^T) + bf16(bf16(xa·B^T)*s))
    auto finish = [&](const float (&v)[PMAX], int c, const uint4 (&b)[2]) -> float {
        float o = rbf(padd(v));
        if (lora_b != nullptr) {
            const int seg = (c >= split0) + (c >= split1);
            float l = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 bv = b[h];
                const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                for (int e = 0; e < 8; ++e) l = fmaf(sXa[seg * 16 + h * 8 + e], bf2f(bp[e]), l);
            }
            o = rbf(o + rbf(rbf(l) * lora_scale));
        }
        return o;
    };
    bf16_t* kdst = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    bf16_t* vdst = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    if (is_rope) {
        const int j = rj, i = ri;
        const float x1 = finish(v1, c1, b1), x2 = finish(v2, c2, b2);
        const bf16_t o1 = f2bf(rbf(x1 * bf2f(cs[0])) + rbf(-x2 * bf2f(cs[1])));
        const bf16_t o2 = f2bf(rbf(x2 * bf2f(cs[2])) + rbf(x1 * bf2f(cs[3])));
        if (j < q_per_kv) {
            sQ[j * HS + i] = o1;
            sQ[j * HS + HALF + i] = o2;
        } else {
            sKn[i] = bf2f(o1);
            sKn[HALF + i] = bf2f(o2);
            kdst[kfrag_off<HS>(pos, i)] = o1;
            kdst[kfrag_off<HS>(pos, HALF + i)] = o2;
        }
    } else if (is_val) {
        const bf16_t v = f2bf(finish(v1, c1, b1));
        sVn[ve] = bf2f(v);
        vdst[vfrag_off<HS>(pos, ve)] = v;
    }
    __syncthreads();
    ATTN_STAMP(2);

    // score of the new key against each head (merged at the combine)
    for (int h = wave; h < q_per_kv; h += NW) {
        float p = 0.f;
        for (int e = lane; e < HS; e += 64) p += bf2f(sQ[h * HS + e]) * sKn[e];
        p = wave_sum(p);
        if (lane == 0) sSn[h] = p * scale;
    }

    // ---- keys 0 .. pos-1 straight from the cache, 32-key tiles dealt over the NW waves
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + (lr & 15) * HS + ks * 16 + lh * 8);
    if (lr >= q_per_kv) {                                               // padding columns: sQ's rows there were never written
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    auto compute_tile = [&](const Tile& T, int t) {
        const int key0 = t * 32;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.kf[ks], qf[ks], st, 0, 0, 0);
        float m_t = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key_abs = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float sc = st[r] * scale;
            sc = key_abs < pos ? sc : -INFINITY;
            st[r] = sc;
            m_t = fmaxf(m_t, sc);
        }
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float psm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(st[r] - m_new);
            st[r] = p;
            psm += p;
        }
        l_run = l_run * alpha + psm;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (s2 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
                // keys >= pos carry p == 0 and the cache beyond the written prefix is finite
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.vf[dt][s2].v, pf.v, o[dt], 0, 0, 0);
            }
        }
    };
    for (int base = wave; base < n_tiles; base += NW) {
        compute_tile(tl, base);
        if (base + NW < n_tiles) load_tile(tl, base + NW);
#ifdef DH_ATTN_STAMPS
        if (base == wave) { asm volatile("" :: "v"(o[0][0])); ATTN_STAMP(3); }
#endif
    }
#ifdef DH_ATTN_STAMPS
    asm volatile("" :: "v"(o[0][0]));
#endif
    ATTN_STAMP(4);
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (lr < q_per_kv) {
        if (lh == 0) {
            sPm[wave * DCOLS + lr] = m_run;
            sPl[wave * DCOLS + lr] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sPo[(wave * DCOLS + lr) * PST + d] = o[dt][r];
            }
    }
    __syncthreads();
    ATTN_STAMP(5);
    // ---- combine the NW wave partials and the new key.  A wave's lanes walk d of one head: with O head-major they read 64
    // consecutive floats (the d-major layout of attn_decode_fused_kernel puts them 16 floats apart, 4 banks for 64 lanes)
    for (int it = tid; it < q_per_kv * HS; it += NT_) {
        const int h = it / HS, d = it % HS;
        const float sn = sSn[h];
        float M = sn;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sPm[w * DCOLS + h]);
        const float pn = __expf(sn - M);
        float L = pn, O = rbf(pn) * sVn[d];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sPm[w * DCOLS + h];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += sPl[w * DCOLS + h] * f;
            O += sPo[(w * DCOLS + h) * PST + d] * f;
        }
        y[(size_t)seq * n_head * HS + (g * q_per_kv + h) * HS + d] = f2bf(O / L);
    }
    ATTN_STAMP(6);
    ATTN_DRAIN();
    ATTN_STAMP(7);
}

// --------------------------------------------------------------------------- attention (verify)
// attn_decode_fused_kernel for S = D + 1 consecutive positions of a sequence at once (speculative greedy decoding: the last token
// and D drafted ones).  grid (n_seq * n_groups), NW waves; qkv32 rows seq * S + j, j = 0 .. S-1, row j at position pos + j.  The
// S * q_per_kv <= 32 query columns ride in the 32 columns of the MFMA the single-token kernel pays for with q_per_kv <= 16 live.
// Row j produces the bits attn_decode_fused_kernel produces at kv_len = len + j:
//   - same NW, same tile -> wave deal (t % NW), same per-tile update and same combine order; a column's arithmetic never reads
//     another column;
//   - column of row j sees the keys [0, pos + j) as cached keys of their 32-key tiles (mask per column) and merges its own key
//     at the combine from LDS.  Keys [pos, pos + j) are those rows 0 .. j-1 of this block have just appended: the tiles that
//     hold positions >= pos are loaded behind the fence + barrier that follows the append, the tiles wholly below pos keep the
//     early prefetch;
//   - a tile in which a column sees no key (the single-token kernel at that kv_len never walks it) leaves the column's running
//     maximum, sum and accumulator as they are: m_run - m_new would be -inf - -inf there.
// Rows at positions >= p_max (the cache's or the rope table's end; a draft behind the last position that can be generated is
// never accepted) append nothing; their output rows are finite and unused.
template <int HS, int PMAX, int NW>
__global__ __launch_bounds__(NW * 64, 1) void attn_verify_fused_kernel(
    const float* __restrict__ qkv32, int n_part, int pairs, int n_rows, int ldq, int qkv_dim,
    const bf16_t* __restrict__ lora_b, float lora_scale, int split0, int split1,
    const bf16_t* __restrict__ cos, const bf16_t* __restrict__ sin, const int32_t* __restrict__ seq_slot,
    const int32_t* __restrict__ kv_len, bf16_t* __restrict__ k_cache, bf16_t* __restrict__ vT_cache,
    bf16_t* __restrict__ y, int n_head, int n_groups, int s_max, int p_max, int S, float scale) {
    constexpr int KS = HS / 16, DT = HS / 32, HALF = HS / 2, VC = 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pair = blockIdx.x, seq = pair / n_groups, g = pair % n_groups;
    const int q_per_kv = n_head / n_groups, ncol = S * q_per_kv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int slot = seq_slot[seq];
    const int len = kv_len[seq], pos = len - 1;          // row 0 (the last token) sits at position len-1
    const int n_live = min(S, p_max - pos);              // rows whose position exists (>= 1: the caller clamps len to p_max)
    // LDS carve (all offsets multiples of 16 B)
    bf16_t* sQ = reinterpret_cast<bf16_t*>(smem);                       // [32][HS] rotated queries, column = j * q_per_kv + head
    float* sKn = reinterpret_cast<float*>(smem + VC * HS * 2);          // [S][HS] new keys (bf16 values)
    float* sVn = sKn + S * HS;                                          // [S][HS] new values
    float* sXa = sVn + S * HS;                                          // [S][48] bf16(x·A^T)
    float* sSn = sXa + S * 48;                                          // [32] score of a column's own key
    float* sPm = sSn + VC;                                              // [NW][32] running max
    float* sPl = sPm + NW * VC;                                         // [NW][32] running sum
    float* sPo = sPl + NW * VC;                                         // [NW][HS][ncol] partial O^T
    constexpr int NT_ = NW * 64;

    struct VF { bf16x8 v; };
    struct Tile { bf16x8 kf[KS]; VF vf[DT][2]; };
    Tile tl;
    const bf16_t* kbase = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    const bf16_t* vbase = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    const int n_tiles = (pos + n_live - 1 + 31) / 32;    // tiles with a key some live row sees: keys [0, pos + n_live - 1)
    const int t_safe = pos >> 5;                         // tiles below hold positions < pos only: nobody writes them in this launch
    auto load_tile = [&](Tile& T, int t, bool early) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8* p = reinterpret_cast<const bf16x8*>(kbase + kfrag_blk<HS>(t, ks) + lane * 8);
            T.kf[ks] = early ? __builtin_nontemporal_load(p) : *p;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8* p = reinterpret_cast<const bf16x8*>(vbase + vfrag_blk<HS>(t, dt, s2) + lane * 8);
                T.vf[dt][s2].v = early ? __builtin_nontemporal_load(p) : *p;
            }
    };
    if (wave < t_safe) load_tile(tl, wave, true);

    const size_t pstride = (size_t)n_rows * ldq;
    auto psum = [&](int j, int c) {
        const float* row0 = qkv32 + ((size_t)seq * S + j) * ldq;
        float v[PMAX];
#pragma unroll
        for (int p = 0; p < PMAX; ++p) v[p] = p < n_part ? row0[p * pstride + c] : 0.f;
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < PMAX; p += 2) s += v[p] + v[p + 1];
        } else {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s += v[p];
        }
        return s;
    };
    if (lora_b != nullptr)
        for (int i = tid; i < 48 * S; i += NT_) sXa[i] = rbf(psum(i / 48, qkv_dim + i % 48));
    for (int i = tid; i < VC * HS; i += NT_) sQ[i] = 0;               // padding columns and rows without a position
    for (int i = tid; i < 2 * S * HS; i += NT_) sKn[i] = 0.f;         // sKn and sVn are adjacent
    __syncthreads();

    auto finish = [&](int j, int c) -> float {
        float o = rbf(psum(j, c));
        if (lora_b != nullptr) {
            const int seg = (c >= split0) + (c >= split1);
            const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)c * 16);
            float l = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 bv = b4[h];
                const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                for (int e = 0; e < 8; ++e) l = fmaf(sXa[j * 48 + seg * 16 + h * 8 + e], bf2f(bp[e]), l);
            }
            o = rbf(o + rbf(rbf(l) * lora_scale));
        }
        return o;
    };
    const int gbase = g * (q_per_kv + 2) * HS;
    bf16_t* kdst = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    bf16_t* vdst = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    const int n_rope = (q_per_kv + 1) * HALF, per_row = n_rope + HS;
    for (int it0 = tid; it0 < n_live * per_row; it0 += NT_) {
        const int jr = it0 / per_row, it = it0 % per_row, pj = pos + jr;     // pj < p_max <= s_max
        if (it < n_rope) {
            const int j = it / HALF, i = it % HALF;
            const float x1 = finish(jr, gbase + j * HS + i), x2 = finish(jr, gbase + j * HS + HALF + i);
            const bf16_t* cp = cos + (size_t)pj * HS;
            const bf16_t* sp = sin + (size_t)pj * HS;
            const bf16_t o1 = f2bf(rbf(x1 * bf2f(cp[i])) + rbf(-x2 * bf2f(sp[i])));
            const bf16_t o2 = f2bf(rbf(x2 * bf2f(cp[HALF + i])) + rbf(x1 * bf2f(sp[HALF + i])));
            if (j < q_per_kv) {
                sQ[(jr * q_per_kv + j) * HS + i] = o1;
                sQ[(jr * q_per_kv + j) * HS + HALF + i] = o2;
            } else {
                sKn[jr * HS + i] = bf2f(o1);
                sKn[jr * HS + HALF + i] = bf2f(o2);
                kdst[kfrag_off<HS>(pj, i)] = o1;
                kdst[kfrag_off<HS>(pj, HALF + i)] = o2;
            }
        } else {
            const int e = it - n_rope;
            const bf16_t v = f2bf(finish(jr, gbase + (q_per_kv + 1) * HS + e));
            sVn[jr * HS + e] = bf2f(v);
            vdst[vfrag_off<HS>(pj, e)] = v;
        }
    }
    __threadfence_block();      // the appended K / V are visible to the block's later loads of the tiles >= t_safe
    __syncthreads();
    if (wave >= t_safe && wave < n_tiles) load_tile(tl, wave, false);

    // score of each column's own key (merged at the combine, as in the single-token kernel)
    for (int c = wave; c < ncol; c += NW) {
        const float* kn = sKn + (c / q_per_kv) * HS;
        float p = 0.f;
        for (int e = lane; e < HS; e += 64) p += bf2f(sQ[c * HS + e]) * kn[e];
        p = wave_sum(p);
        if (lane == 0) sSn[c] = p * scale;
    }

    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + lr * HS + ks * 16 + lh * 8);
    // the keys this lane's column sees in the cache: [0, p_col)
    const int j_col = lr < ncol ? lr / q_per_kv : 0;
    const int p_col = pos + (j_col < n_live ? j_col : 0);
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    auto compute_tile = [&](const Tile& T, int t) {
        const int key0 = t * 32;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.kf[ks], qf[ks], st, 0, 0, 0);
        float m_t = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key_abs = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float sc = st[r] * scale;
            sc = key_abs < p_col ? sc : -INFINITY;
            st[r] = sc;
            m_t = fmaxf(m_t, sc);
        }
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);
        const bool none = m_new == -INFINITY;               // no key of this column so far: nothing changes
        const float alpha = none ? 1.f : __expf(m_run - m_new);
        m_run = m_new;
        float psm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = none ? 0.f : __expf(st[r] - m_new);
            st[r] = p;
            psm += p;
        }
        l_run = l_run * alpha + psm;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (s2 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.vf[dt][s2].v, pf.v, o[dt], 0, 0, 0);
            }
        }
    };
    for (int base = wave; base < n_tiles; base += NW) {
        compute_tile(tl, base);
        if (base + NW < n_tiles) load_tile(tl, base + NW, false);       // behind the barrier: any tile may be read
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (lr < ncol) {
        if (lh == 0) {
            sPm[wave * VC + lr] = m_run;
            sPl[wave * VC + lr] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sPo[(wave * HS + d) * ncol + lr] = o[dt][r];
            }
    }
    __syncthreads();
    // ---- combine the NW wave partials and each column's own key
    for (int it = tid; it < ncol * HS; it += NT_) {
        const int c = it / HS, d = it % HS, jr = c / q_per_kv, h = c % q_per_kv;
        const float sn = sSn[c];
        float M = sn;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sPm[w * VC + c]);
        const float pn = __expf(sn - M);
        float L = pn, O = rbf(pn) * sVn[jr * HS + d];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sPm[w * VC + c];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += sPl[w * VC + c] * f;
            O += sPo[(w * HS + d) * ncol + c] * f;
        }
        y[((size_t)seq * S + jr) * n_head * HS + (g * q_per_kv + h) * HS + d] = f2bf(O / L);
    }
}
template <int HS>
size_t attn_verify_lds(int S, int ncol) {
    constexpr int NW = attn_fused_waves<HS>();
    return 32 * HS * 2 + (size_t)(2 * S * HS + 48 * S + 32 + 2 * NW * 32 + NW * HS * ncol) * sizeof(float);
}

// --------------------------------------------------------------------------- attention (decode, shared prompt)
// attn_decode_fused_kernel for the N rows of an utterance that share a prompt (sampled candidates, beams): rows u * N + j of qkv32,
// j = 0 .. N-1, belong to utterance u, and every row's slot holds the same bytes in the n_sh = prompt_len[u] / 32 whole 32-key tiles
// of the prompt (dh_engine_fork_slots, dh_engine_copy_prefix).  grid (n_utt * n_cg * n_groups), NW waves: a block serves one KV group
// and one column group, the R <= Gs = 32 / q_per_kv consecutive rows u * N + cg * Gs + jj; query column = jj * q_per_kv + head, as in
// attn_verify_fused_kernel.  Row jj produces the bits attn_decode_fused_kernel produces for it:
//   - tiles t < n_sh are loaded ONCE per block, from the slot of the utterance's row 0, and serve every column; tiles t >= n_sh are
//     private: for each row jj with t < (pos_jj + 31) / 32 the tile comes from the row's own slot and is masked to key < pos_jj for
//     the row's columns and to nothing for every other column;
//   - same NW, same tile -> wave deal (t % NW, shared or private, ascending t within a wave), same per-tile update and same combine
//     order; a column's arithmetic never reads another column, and a tile in which a column sees no key leaves its running maximum,
//     sum and accumulator as they are (attn_verify_fused_kernel's `none` rule);
//   - each row finishes its own q / k / v from its partials, rotates at its own position kv_len - 1, appends to its own slot and
//     merges its own key at the combine from LDS.
// Nothing this launch writes is read back (a row's own position is masked in its own tile), so a wave's first tile is requested
// before the LoRA / rope prologue.
// hs 64 is held to 128 VGPRs (four waves per SIMD, 4 spilled registers): with the 75 KiB of LDS of four rows x eight heads two blocks
// share a CU; hs 96 and 128 run one block per CU (189 / 227 VGPRs, up to 112 / 148 KiB).
// TAB ("Beam KV tile table" of the header; dh_attn_decode_shared_tab_bf16): row jj's private tile t is read from the slot of the sibling
// that the table names, entry [plane][row][t - n_sh], plane (*step - 1) & 1 (null step: 0).  The block's r_max x nt entries go to LDS
// in the prologue as SLOTS — the entry clamped to 0 .. N-1, then seq_slot of that sibling's row — and load_tile does one LDS lookup per
// private tile; a tile at or behind nt is the row's own.  The append, the tile -> wave deal, the per-tile update and the combine are
// the code of TAB = false, whose instantiations take an empty argument and compile to what they were.
template <bool TAB>
struct attn_tab_args {};
template <>
struct attn_tab_args<true> {
    const int32_t* tab;       // [2][n_rows][ld]
    const int32_t* step;      // device step counter, or null
    int ld;                   // row stride = tiles per row
};
template <int HS, int PMAX, int NW, bool TAB = false>
__global__ __launch_bounds__(NW * 64, HS == 64 ? 4 : 2) void attn_shared_fused_kernel(
    const float* __restrict__ qkv32, int n_part, int pairs, int n_rows, int ldq, int qkv_dim,
    const bf16_t* __restrict__ lora_b, float lora_scale, int split0, int split1,
    const bf16_t* __restrict__ cos, const bf16_t* __restrict__ sin, const int32_t* __restrict__ seq_slot,
    const int32_t* __restrict__ kv_len, const int32_t* __restrict__ prompt_len, bf16_t* __restrict__ k_cache,
    bf16_t* __restrict__ vT_cache, bf16_t* __restrict__ y, int n_head, int n_groups, int s_max, int N, int Gs, int n_cg,
    int r_max, float scale, attn_tab_args<TAB> ta) {
    constexpr int KS = HS / 16, DT = HS / 32, HALF = HS / 2, VC = 32, RMAX = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = blockIdx.x % n_groups, ucg = blockIdx.x / n_groups, cg = ucg % n_cg, u = ucg / n_cg;
    const int q_per_kv = n_head / n_groups;
    const int R = min(Gs, N - cg * Gs), ncol = R * q_per_kv;            // this block's rows and live columns
    const int row0 = u * N + cg * Gs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    // LDS carve (all offsets multiples of 16 B); sized by the host for r_max rows and r_max * q_per_kv columns
    bf16_t* sQ = reinterpret_cast<bf16_t*>(smem);                       // [32][HS] rotated queries, column = jj * q_per_kv + head
    float* sKn = reinterpret_cast<float*>(smem + VC * HS * 2);          // [r_max][HS] new keys (bf16 values)
    float* sVn = sKn + r_max * HS;                                      // [r_max][HS] new values
    float* sXa = sVn + r_max * HS;                                      // [r_max][48] bf16(x·A^T)
    float* sSn = sXa + r_max * 48;                                      // [32] score of a column's own key
    float* sPm = sSn + VC;                                              // [NW][32] running max
    float* sPl = sPm + NW * VC;                                         // [NW][32] running sum
    int* sPos = reinterpret_cast<int*>(sPl + NW * VC);                  // [8] position of row jj's new token
    int* sSlot = sPos + RMAX;                                           // [8] its KV slot
    float* sPo = reinterpret_cast<float*>(sSlot + RMAX);                // [NW][HS][ncol] partial O^T
    constexpr int NT_ = NW * 64;
    int* sTab = reinterpret_cast<int*>(sPo + NW * HS * (r_max * q_per_kv));   // TAB: [r_max][nt] slots of the rows' private tiles
    int nt_tab = 0;

    if (tid < RMAX) {
        const int r = row0 + (tid < R ? tid : 0);
        sPos[tid] = tid < R ? kv_len[r] - 1 : 0;
        sSlot[tid] = seq_slot[r];
    }
    if constexpr (TAB) {
        nt_tab = ta.ld;
        const int plane = ta.step ? (*ta.step - 1) & 1 : 0;
        const int32_t* tp = ta.tab + ((size_t)plane * n_rows + row0) * nt_tab;
        for (int i = tid; i < R * nt_tab; i += NT_) {
            int b = tp[i];
            b = b < 0 ? 0 : (b >= N ? N - 1 : b);                       // nothing is trusted to index
            sTab[i] = seq_slot[u * N + b];
        }
    }
    __syncthreads();
    int n_sh = prompt_len[u] / 32;                                      // whole prompt tiles: the same bytes in every row's slot
    n_sh = n_sh < 0 ? 0 : (n_sh > s_max / 32 ? s_max / 32 : n_sh);
    int t_end = n_sh;                                                   // tiles with a key some column sees
    for (int j = 0; j < R; ++j) t_end = max(t_end, (sPos[j] + 31) / 32);
    const size_t blk = (size_t)s_max * HS;                              // elements of a (slot, group) block in either cache
    const size_t sh_off = ((size_t)seq_slot[u * N] * n_groups + g) * blk;

    // ---- this wave's items in walking order: tile t = wave, wave + NW, ...; a shared tile is one item, a private tile one item per
    // row jj that has it
    int it_t = wave, it_j = 0;
    auto settle = [&]() {       // the first item at or behind (it_t, it_j); it_t >= t_end: none left
        while (it_t < t_end) {
            if (it_t < n_sh) { it_j = 0; return; }
            while (it_j < R && it_t >= (sPos[it_j] + 31) / 32) ++it_j;
            if (it_j < R) return;
            it_t += NW;
            it_j = 0;
        }
    };
    auto advance = [&]() {
        if (it_t < n_sh) { it_t += NW; it_j = 0; }
        else ++it_j;
        settle();
    };
    struct VF { bf16x8 v; };
    struct Tile { bf16x8 kf[KS]; VF vf[DT][2]; };
    Tile tl;
    // the caches are in MFMA-fragment order (common.h): a tile is 8 coalesced 1-KiB loads
    auto load_tile = [&](Tile& T, int t, int jj) {
        size_t off;
        if constexpr (TAB) {
            const int j = t - n_sh;
            off = t < n_sh ? sh_off : ((size_t)(j < nt_tab ? sTab[jj * nt_tab + j] : sSlot[jj]) * n_groups + g) * blk;
        } else {
            off = t < n_sh ? sh_off : ((size_t)sSlot[jj] * n_groups + g) * blk;
        }
        const bf16_t* kbase = k_cache + off;
        const bf16_t* vbase = vT_cache + off;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            T.kf[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kbase + kfrag_blk<HS>(t, ks) + lane * 8));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                T.vf[dt][s2].v = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vbase + vfrag_blk<HS>(t, dt, s2) + lane * 8));
    };
    settle();
    if (it_t < t_end) load_tile(tl, it_t, it_j);

    const size_t pstride = (size_t)n_rows * ldq;
    auto psum = [&](int j, int c) {
        const float* rowp = qkv32 + (size_t)(row0 + j) * ldq;
        float v[PMAX];
#pragma unroll
        for (int p = 0; p < PMAX; ++p) v[p] = p < n_part ? rowp[p * pstride + c] : 0.f;
        // the decode family's summation order (common.h, "K-slice combine"), as in attn_decode_fused_kernel
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < PMAX; p += 2) s += v[p] + v[p + 1];
        } else {
#pragma unroll
            for (int p = 0; p < PMAX; ++p) s += v[p];
        }
        return s;
    };
    if (lora_b != nullptr)
        for (int i = tid; i < 48 * R; i += NT_) sXa[i] = rbf(psum(i / 48, qkv_dim + i % 48));
    for (int i = tid; i < VC * HS; i += NT_) sQ[i] = 0;               // padding columns
    __syncthreads();

    // bf16 value of fused-qkv column c of row j: bf16(bf16(x·W^T) + bf16(bf16(xa·B^T)*s))
    auto finish = [&](int j, int c) -> float {
        float o = rbf(psum(j, c));
        if (lora_b != nullptr) {
            const int seg = (c >= split0) + (c >= split1);
            const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)c * 16);
            float l = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint4 bv = b4[h];
                const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                for (int e = 0; e < 8; ++e) l = fmaf(sXa[j * 48 + seg * 16 + h * 8 + e], bf2f(bp[e]), l);
            }
            o = rbf(o + rbf(rbf(l) * lora_scale));
        }
        return o;
    };
    const int gbase = g * (q_per_kv + 2) * HS;
    const int n_rope = (q_per_kv + 1) * HALF, per_row = n_rope + HS;
    for (int it0 = tid; it0 < R * per_row; it0 += NT_) {
        const int jr = it0 / per_row, it = it0 % per_row, pj = sPos[jr];
        const size_t off = ((size_t)sSlot[jr] * n_groups + g) * blk;
        bf16_t* kdst = k_cache + off;
        bf16_t* vdst = vT_cache + off;
        if (it < n_rope) {
            const int j = it / HALF, i = it % HALF;
            const float x1 = finish(jr, gbase + j * HS + i), x2 = finish(jr, gbase + j * HS + HALF + i);
            const bf16_t* cp = cos + (size_t)pj * HS;
            const bf16_t* sp = sin + (size_t)pj * HS;
            const bf16_t o1 = f2bf(rbf(x1 * bf2f(cp[i])) + rbf(-x2 * bf2f(sp[i])));
            const bf16_t o2 = f2bf(rbf(x2 * bf2f(cp[HALF + i])) + rbf(x1 * bf2f(sp[HALF + i])));
            if (j < q_per_kv) {
                sQ[(jr * q_per_kv + j) * HS + i] = o1;
                sQ[(jr * q_per_kv + j) * HS + HALF + i] = o2;
            } else {
                sKn[jr * HS + i] = bf2f(o1);
                sKn[jr * HS + HALF + i] = bf2f(o2);
                kdst[kfrag_off<HS>(pj, i)] = o1;
                kdst[kfrag_off<HS>(pj, HALF + i)] = o2;
            }
        } else {
            const int e = it - n_rope;
            const bf16_t v = f2bf(finish(jr, gbase + (q_per_kv + 1) * HS + e));
            sVn[jr * HS + e] = bf2f(v);
            vdst[vfrag_off<HS>(pj, e)] = v;
        }
    }
    __syncthreads();

    // score of each column's own key (merged at the combine, as in the single-token kernel)
    for (int c = wave; c < ncol; c += NW) {
        const float* kn = sKn + (c / q_per_kv) * HS;
        float p = 0.f;
        for (int e = lane; e < HS; e += 64) p += bf2f(sQ[c * HS + e]) * kn[e];
        p = wave_sum(p);
        if (lane == 0) sSn[c] = p * scale;
    }

    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(sQ + lr * HS + ks * 16 + lh * 8);
    // the row of this lane's column and the keys it sees in the cache: [0, p_col); a padding column sees none
    const int j_col = lr < ncol ? lr / q_per_kv : -1;
    const int p_col = lr < ncol ? sPos[j_col] : 0;
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    // jj < 0: a shared tile, every column's; else row jj's private tile
    auto compute_tile = [&](const Tile& T, int t, int jj) {
        const int key0 = t * 32;
        const int lim = jj < 0 || jj == j_col ? p_col : 0;
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.kf[ks], qf[ks], st, 0, 0, 0);
        float m_t = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key_abs = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float sc = st[r] * scale;
            sc = key_abs < lim ? sc : -INFINITY;
            st[r] = sc;
            m_t = fmaxf(m_t, sc);
        }
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);
        const bool none = m_new == -INFINITY;               // no key of this column so far: nothing changes
        const float alpha = none ? 1.f : __expf(m_run - m_new);
        m_run = m_new;
        float psm = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = none ? 0.f : __expf(st[r] - m_new);
            st[r] = p;
            psm += p;
        }
        l_run = l_run * alpha + psm;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[8 * s2 + 2 * j], st[8 * s2 + 2 * j + 1]);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (s2 == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
                // keys a column does not see carry p == 0 and the cache beyond the written prefix is finite
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(T.vf[dt][s2].v, pf.v, o[dt], 0, 0, 0);
            }
        }
    };
    while (it_t < t_end) {
        const int ct = it_t, cj = it_t < n_sh ? -1 : it_j;
        advance();
        compute_tile(tl, ct, cj);
        if (it_t < t_end) load_tile(tl, it_t, it_j);
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (lr < ncol) {
        if (lh == 0) {
            sPm[wave * VC + lr] = m_run;
            sPl[wave * VC + lr] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                sPo[(wave * HS + d) * ncol + lr] = o[dt][r];
            }
    }
    __syncthreads();
    // ---- combine the NW wave partials and each column's own key
    for (int it = tid; it < ncol * HS; it += NT_) {
        const int c = it / HS, d = it % HS, jr = c / q_per_kv, h = c % q_per_kv;
        const float sn = sSn[c];
        float M = sn;
#pragma unroll
        for (int w = 0; w < NW; ++w) M = fmaxf(M, sPm[w * VC + c]);
        const float pn = __expf(sn - M);
        float L = pn, O = rbf(pn) * sVn[jr * HS + d];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = sPm[w * VC + c];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += sPl[w * VC + c] * f;
            O += sPo[(w * HS + d) * ncol + c] * f;
        }
        y[(size_t)(row0 + jr) * n_head * HS + (g * q_per_kv + h) * HS + d] = f2bf(O / L);
    }
}
template <int HS>
size_t attn_shared_lds(int r_max, int ncol) {
    constexpr int NW = attn_fused_waves<HS>();
    return 32 * HS * 2 + (size_t)(2 * r_max * HS + 48 * r_max + 32 + 2 * NW * 32 + 16 + NW * HS * ncol) * sizeof(float);
}
// the table variant's: the r_max x nt slots behind the partial outputs
template <int HS>
size_t attn_shared_tab_lds(int r_max, int ncol, int nt) {
    return attn_shared_lds<HS>(r_max, ncol) + (size_t)r_max * nt * sizeof(int);
}

// --------------------------------------------------------------------------- finish + norm
// grid (rows), 256 threads.  h32: [n_part][rows][ldh] fp32 partials of x·[W;A]^T (columns
// [d, d+16) = x·A^T when lora_b != null).  Per row:
//   h  = bf16( bf16(sum_p h32) + bf16( bf16(xa·B^T) * s ) )      (LoRA finish, ger/lora.py:159-166)
//   x' = bf16( x + h )                                           (residual, ger/model.py:185-186)
//   xn = RMSNorm(x') with weight w_norm                          (ger/rmsnorm.py:17-21, Q11 flag)
// HOIST: a thread's first column chunk requests the first four partials, the residual and the norm weight ahead of the
// barrier that hands x·A^T over.  Its 8 x 32 B of B stay behind the barrier: hoisted too they cost 64 more VGPRs (214), two
// blocks per CU instead of eight, and 640 rows no longer fit in one round (measured slower at every row count).  Same arithmetic in the same order; chosen by the row count (FINISH_HOIST_ROWS).
template <int MAXC, bool HOIST>
__global__ __launch_bounds__(256) void finish_norm_kernel(const float* __restrict__ h32, int n_part, int pairs, int rows, int ldh,
                                                          const bf16_t* __restrict__ lora_b, float lora_scale,
                                                          const bf16_t* __restrict__ x_resid,
                                                          const bf16_t* __restrict__ w_norm, bf16_t* __restrict__ x_out,
                                                          bf16_t* __restrict__ xn_out, int d, float eps,
                                                          const uint8_t* __restrict__ row_tail) {
    __shared__ float sXa[16];
    __shared__ float sRed[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* hrow = h32 + (size_t)row * ldh;
    const size_t pstride = (size_t)rows * ldh;
    if (lora_b != nullptr && tid < 16) {
        float pv[MAXP];
#pragma unroll
        for (int p = 0; p < MAXP; ++p) pv[p] = p < n_part ? hrow[p * pstride + d + tid] : 0.f;
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < MAXP; p += 2) s += pv[p] + pv[p + 1];
        } else {
#pragma unroll
            for (int p = 0; p < MAXP; ++p) s += pv[p];
        }
        sXa[tid] = rbf(s);
    }
    float4 ha0[4] = {}, ha1[4] = {};
    uint4 hxr = {}, hwu = {};
    if (HOIST && tid * 8 < d) {
        const int c0 = tid * 8;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = q < n_part ? q : 0;
            ha0[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0);
            ha1[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0 + 4);
        }
        hxr = *reinterpret_cast<const uint4*>(x_resid + (size_t)row * d + c0);
        hwu = *reinterpret_cast<const uint4*>(w_norm + c0);
    }
    __syncthreads();
    float v[MAXC][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c0 = (tid + i * 256) * 8;
        if (c0 < d) {
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.f;
            // partials in groups of 4: 8 independent 16-B loads in flight before the adds
            for (int p0 = 0; p0 < n_part; p0 += 4) {
                float4 a0[4], a1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (HOIST && i == 0 && p0 == 0) {
                        a0[q] = ha0[q]; a1[q] = ha1[q];
                        continue;
                    }
                    const int p = p0 + q < n_part ? p0 + q : p0;
                    a0[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0);
                    a1[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0 + 4);
                }
                if (pairs) {      // leaves: adjacent pairs first (a missing partner counts as 0), pair sums in order
#pragma unroll
                    for (int q = 0; q < 4; q += 2) {
                        if (p0 + q < n_part) {
                            const bool two = p0 + q + 1 < n_part;
                            const float4 b0 = two ? a0[q + 1] : float4{0.f, 0.f, 0.f, 0.f}, b1 = two ? a1[q + 1] : float4{0.f, 0.f, 0.f, 0.f};
                            acc[0] += a0[q].x + b0.x; acc[1] += a0[q].y + b0.y; acc[2] += a0[q].z + b0.z; acc[3] += a0[q].w + b0.w;
                            acc[4] += a1[q].x + b1.x; acc[5] += a1[q].y + b1.y; acc[6] += a1[q].z + b1.z; acc[7] += a1[q].w + b1.w;
                        }
                    }
                } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (p0 + q < n_part) {
                        acc[0] += a0[q].x; acc[1] += a0[q].y; acc[2] += a0[q].z; acc[3] += a0[q].w;
                        acc[4] += a1[q].x; acc[5] += a1[q].y; acc[6] += a1[q].z; acc[7] += a1[q].w;
                    }
                }
                }
            }
            const uint4 xr = HOIST && i == 0 ? hxr : *reinterpret_cast<const uint4*>(x_resid + (size_t)row * d + c0);
            const bf16_t* xp = reinterpret_cast<const bf16_t*>(&xr);
            uint4 xo;
            bf16_t* xop = reinterpret_cast<bf16_t*>(&xo);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float o = rbf(acc[e]);
                if (lora_b != nullptr) {
                    const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)(c0 + e) * 16);
                    float l = 0.f;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint4 bv = b4[h];
                        const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                        for (int k = 0; k < 8; ++k) l = fmaf(sXa[h * 8 + k], bf2f(bp[k]), l);
                    }
                    o = rbf(o + rbf(rbf(l) * lora_scale));
                }
                xop[e] = f2bf(bf2f(xp[e]) + o);
                v[i][e] = bf2f(xop[e]);
                ss += rbf(v[i][e] * v[i][e]);
            }
            *reinterpret_cast<uint4*>(x_out + (size_t)row * d + c0) = xo;
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) sRed[wave] = ss;
    __syncthreads();
    ss = sRed[0] + sRed[1] + sRed[2] + sRed[3];
    const float ms = rbf(ss / (float)d);
    const float t = rbf(ms + eps);
    const bool tail = row_tail != nullptr && row_tail[row] != 0;
    const float r = tail ? rbf(1.0f / rbf(sqrtf(t))) : rbf(1.0f / sqrtf(t));
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c0 = (tid + i * 256) * 8;
        if (c0 < d) {
            const uint4 wu = HOIST && i == 0 ? hwu : *reinterpret_cast<const uint4*>(w_norm + c0);
            const bf16_t* wp = reinterpret_cast<const bf16_t*>(&wu);
            uint4 o;
            bf16_t* op = reinterpret_cast<bf16_t*>(&o);
#pragma unroll
            for (int e = 0; e < 8; ++e) op[e] = f2bf(bf2f(wp[e]) * rbf(v[i][e] * r));
            *reinterpret_cast<uint4*>(xn_out + (size_t)row * d + c0) = o;
        }
    }
}

// The same finish for SEVERAL consecutive rows per block (grid = ceil(rows / rpb)), built so that no load waits behind a
// barrier.  A thread keeps its column chunk of finish_norm_kernel (columns (tid + 256 i) * 8 ..), so a row's `ss` order is
// that kernel's, and every statement of the arithmetic is that kernel's too; what changes is when the bytes are asked for:
//   - what a thread needs for its first chunk of row r + 1 (x·A^T partials, the first PF partials, the residual) is
//     requested before the arithmetic of row r, and rows 0 and 1 of a block are both in flight from the start;
//   - its 8 x 32 B of lora_b and its norm weights are loaded ONCE per block and stay in registers (64 + 4 VGPRs) over
//     the block's rows: not one trip to L2 per row behind the hand-over barrier;
//   - x·A^T of row r + 1 is handed over (sXa, double buffered) in front of the ONE barrier of row r, the one of its
//     reduction (sRed, double buffered): a row costs one barrier, and that barrier waits for LDS only.
// Chunks i >= 1 (d > 2048) and partials beyond PF are requested where they are used, as in finish_norm_kernel.
// PF: partials requested a row ahead (1, 4 or 8); XP >= n_part: x·A^T partials threads 0..15 hold a row ahead.  The dispatcher
// takes the smallest PF that covers n_part, but 4 for more than 4 partials with LoRA (8 would not fit in 256 VGPRs beside lora_b).
template <int MAXC, int PF, int XP, bool LORA>
__global__ __launch_bounds__(256) void finish_norm_rows_kernel(const float* __restrict__ h32, int n_part, int pairs, int rows, int ldh,
                                                               const bf16_t* __restrict__ lora_b, float lora_scale,
                                                               const bf16_t* __restrict__ x_resid,
                                                               const bf16_t* __restrict__ w_norm, bf16_t* __restrict__ x_out,
                                                               bf16_t* __restrict__ xn_out, int d, float eps,
                                                               const uint8_t* __restrict__ row_tail, int rpb) {
    __shared__ float sXa[2][16];
    __shared__ float sRed[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * rpb, nrow = min(rpb, rows - row0);
    const size_t pstride = (size_t)rows * ldh;
    const bool own = tid * 8 < d;                // this thread has a first chunk
    struct Pre { float xa[XP]; float4 a0[PF], a1[PF]; uint4 xr; };
    auto request = [&](Pre& P, int row) __attribute__((always_inline)) {
        const float* hrow = h32 + (size_t)row * ldh;
        if (LORA && tid < 16) {
#pragma unroll
            for (int p = 0; p < XP; ++p) P.xa[p] = p < n_part ? hrow[p * pstride + d + tid] : 0.f;
        }
        if (own) {
            const int c0 = tid * 8;
#pragma unroll
            for (int q = 0; q < PF; ++q) {
                const int p = q < n_part ? q : 0;
                P.a0[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0);
                P.a1[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0 + 4);
            }
            P.xr = *reinterpret_cast<const uint4*>(x_resid + (size_t)row * d + c0);
        }
    };
    auto xa_sum = [&](const Pre& P) __attribute__((always_inline)) {       // finish_norm_kernel's, without its trailing + 0.f terms
        float s = 0.f;
        if (pairs) {
#pragma unroll
            for (int p = 0; p < XP; p += 2) s += P.xa[p] + (p + 1 < XP ? P.xa[p + 1] : 0.f);
        } else {
#pragma unroll
            for (int p = 0; p < XP; ++p) s += P.xa[p];
        }
        return rbf(s);
    };
    // G loaded partials p0 .. p0 + G - 1 into acc, in finish_norm_kernel's order
    auto add_group = [&](float (&acc)[8], const float4* a0, const float4* a1, int p0, auto G_) __attribute__((always_inline)) {
        constexpr int G = decltype(G_)::value;
        if (pairs) {      // leaves: adjacent pairs first (a missing partner counts as 0), pair sums in order
#pragma unroll
            for (int q = 0; q < G; q += 2) {
                if (p0 + q < n_part) {
                    const bool two = q + 1 < G && p0 + q + 1 < n_part;
                    const float4 b0 = two ? a0[q + 1 < G ? q + 1 : q] : float4{0.f, 0.f, 0.f, 0.f}, b1 = two ? a1[q + 1 < G ? q + 1 : q] : float4{0.f, 0.f, 0.f, 0.f};
                    acc[0] += a0[q].x + b0.x; acc[1] += a0[q].y + b0.y; acc[2] += a0[q].z + b0.z; acc[3] += a0[q].w + b0.w;
                    acc[4] += a1[q].x + b1.x; acc[5] += a1[q].y + b1.y; acc[6] += a1[q].z + b1.z; acc[7] += a1[q].w + b1.w;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < G; ++q) {
                if (p0 + q < n_part) {
                    acc[0] += a0[q].x; acc[1] += a0[q].y; acc[2] += a0[q].z; acc[3] += a0[q].w;
                    acc[4] += a1[q].x; acc[5] += a1[q].y; acc[6] += a1[q].z; acc[7] += a1[q].w;
                }
            }
        }
    };

    Pre pa, pb;
    request(pa, row0);
    if (nrow > 1) request(pb, row0 + 1);
    uint4 bq[LORA ? 8 : 1][2];                   // lora_b rows of the first chunk's 8 columns
    uint4 hwu = {};
    if (own) {
        if (LORA) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)(tid * 8 + e) * 16);
                bq[e][0] = b4[0];
                bq[e][1] = b4[1];
            }
        }
        hwu = *reinterpret_cast<const uint4*>(w_norm + tid * 8);
    }
    if (LORA && tid < 16) sXa[0][tid] = xa_sum(pa);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    // row row0 + k from P; Q: row k + 1 (requested already), refilled with row k + 2 once it has been handed on
    auto do_row = [&](Pre& P, Pre& Q, int k) __attribute__((always_inline)) {
        const int row = row0 + k, par = k & 1;
        const float* hrow = h32 + (size_t)row * ldh;
        const bool tail = row_tail != nullptr && row_tail[row] != 0;      // asked for here, used behind the barrier
        float v[MAXC][8];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c0 = (tid + i * 256) * 8;
            if (c0 < d) {
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.f;
                if (i == 0) add_group(acc, P.a0, P.a1, 0, std::integral_constant<int, PF>{});
                // partials in groups of 4: 8 independent 16-B loads in flight before the adds
                for (int p0 = i == 0 ? PF : 0; p0 < n_part; p0 += 4) {
                    float4 a0[4], a1[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int p = p0 + q < n_part ? p0 + q : p0;
                        a0[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0);
                        a1[q] = *reinterpret_cast<const float4*>(hrow + p * pstride + c0 + 4);
                    }
                    add_group(acc, a0, a1, p0, std::integral_constant<int, 4>{});
                }
                const uint4 xr = i == 0 ? P.xr : *reinterpret_cast<const uint4*>(x_resid + (size_t)row * d + c0);
                const bf16_t* xp = reinterpret_cast<const bf16_t*>(&xr);
                uint4 xo;
                bf16_t* xop = reinterpret_cast<bf16_t*>(&xo);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float o = rbf(acc[e]);
                    if (LORA) {
                        const uint4* b4 = reinterpret_cast<const uint4*>(lora_b + (size_t)(c0 + e) * 16);
                        float l = 0.f;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            uint4 bv = i == 0 ? bq[e][h] : b4[h];
                            // keeps the block's copy packed: without it the compiler widens all 128 values to fp32 once per block (+64 VGPRs)
                            if (i == 0) asm volatile("" : "+v"(bv.x), "+v"(bv.y), "+v"(bv.z), "+v"(bv.w));
                            const bf16_t* bp = reinterpret_cast<const bf16_t*>(&bv);
#pragma unroll
                            for (int kk = 0; kk < 8; ++kk) l = fmaf(sXa[par][h * 8 + kk], bf2f(bp[kk]), l);
                        }
                        o = rbf(o + rbf(rbf(l) * lora_scale));
                    }
                    xop[e] = f2bf(bf2f(xp[e]) + o);
                    v[i][e] = bf2f(xop[e]);
                    ss += rbf(v[i][e] * v[i][e]);
                }
                *reinterpret_cast<uint4*>(x_out + (size_t)row * d + c0) = xo;
            }
        }
        if (k + 2 < nrow) request(P, row + 2);      // P's registers are free: its row is in v
        ss = wave_sum(ss);
        if (lane == 0) sRed[par][wave] = ss;
        if (LORA && k + 1 < nrow && tid < 16) sXa[par ^ 1][tid] = xa_sum(Q);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        ss = sRed[par][0] + sRed[par][1] + sRed[par][2] + sRed[par][3];
        const float ms = rbf(ss / (float)d);
        const float t = rbf(ms + eps);
        const float r = tail ? rbf(1.0f / rbf(sqrtf(t))) : rbf(1.0f / sqrtf(t));
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c0 = (tid + i * 256) * 8;
            if (c0 < d) {
                const uint4 wu = i == 0 ? hwu : *reinterpret_cast<const uint4*>(w_norm + c0);
                const bf16_t* wp = reinterpret_cast<const bf16_t*>(&wu);
                uint4 o;
                bf16_t* op = reinterpret_cast<bf16_t*>(&o);
#pragma unroll
                for (int e = 0; e < 8; ++e) op[e] = f2bf(bf2f(wp[e]) * rbf(v[i][e] * r));
                *reinterpret_cast<uint4*>(xn_out + (size_t)row * d + c0) = o;
            }
        }
    };
    for (int k = 0; k < nrow; k += 2) {
        do_row(pa, pb, k);
        if (k + 1 < nrow) do_row(pb, pa, k + 1);
    }
}

}  // namespace

extern "C" int dh_attn_decode_fused_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                                         const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                                         const dh_bf16* cos, const dh_bf16* sin, const int32_t* seq_slot,
                                         const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache, dh_bf16* y,
                                         int n_head, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(qkv32 && cos && sin && seq_slot && kv_len && k_cache && vT_cache && y, "dh_attn_decode_fused_bf16: null argument");
    DH_CHECK(n_groups > 0 && n_head % n_groups == 0 && n_head / n_groups <= DCOLS, "dh_attn_decode_fused_bf16: bad head counts");
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "dh_attn_decode_fused_bf16: head_size %d unsupported", hs);
    DH_CHECK(s_max % 64 == 0 && n_part >= 1 && n_part <= MAXP, "dh_attn_decode_fused_bf16: bad s_max / n_part");
    DH_CHECK(qkv_dim == (n_head + 2 * n_groups) * hs, "dh_attn_decode_fused_bf16: qkv_dim mismatch");
    DH_CHECK(lora_b == nullptr || n_ext >= 48, "dh_attn_decode_fused_bf16: LoRA needs the 48 x·A^T columns");
    if (n_seq <= 0) return 0;
    const float scale = 1.0f / sqrtf((float)hs);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(n_seq * n_groups);
#define ATT_LAUNCH(HSV, PM)                                                                                           \
    hipLaunchKernelGGL((attn_decode_fused_kernel<HSV, PM, attn_fused_waves<HSV>()>), grid, dim3(64 * attn_fused_waves<HSV>()), attn_fused_lds<HSV>(), s, qkv32, n_part, pairs, n_seq,  \
                       qkv_dim + n_ext, qkv_dim, lora_b, lora_scale, split0, split1, cos, sin, seq_slot, kv_len, k_cache,  \
                       vT_cache, y, n_head, n_groups, s_max, scale)
#define CHAIN_LAUNCH(PM)                                                                                              \
    hipLaunchKernelGGL((attn_decode_chain_kernel<64, PM, CHAIN_NW>), grid, dim3(64 * CHAIN_NW), attn_chain_lds<64>(), s, qkv32, n_part, pairs, n_seq,  \
                       qkv_dim + n_ext, qkv_dim, lora_b, lora_scale, split0, split1, cos, sin, seq_slot, kv_len, k_cache,  \
                       vT_cache, y, n_head, n_groups, s_max, scale)
    if (hs == 64) {
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<64, 2, attn_fused_waves<64>()>), attn_fused_lds<64>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<64, 8, attn_fused_waves<64>()>), attn_fused_lds<64>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<64, 16, attn_fused_waves<64>()>), attn_fused_lds<64>());
        // the short-chain kernel gives a thread one finish item: (q_per_kv + 1) * 32 + 64 of them
        const bool chain = g_attn_chain != 0 && attn_fused_waves<64>() == CHAIN_NW && (n_head / n_groups + 1) * 32 + 64 <= 64 * CHAIN_NW;
        if (chain) {
            DH_MAX_LDS_ONCE((attn_decode_chain_kernel<64, 2, CHAIN_NW>), attn_chain_lds<64>());
            DH_MAX_LDS_ONCE((attn_decode_chain_kernel<64, 8, CHAIN_NW>), attn_chain_lds<64>());
            DH_MAX_LDS_ONCE((attn_decode_chain_kernel<64, 16, CHAIN_NW>), attn_chain_lds<64>());
            if (n_part <= 2) CHAIN_LAUNCH(2);
            else if (n_part <= 8) CHAIN_LAUNCH(8);
            else CHAIN_LAUNCH(16);
        } else if (n_part <= 2) ATT_LAUNCH(64, 2);
        else if (n_part <= 8) ATT_LAUNCH(64, 8);
        else ATT_LAUNCH(64, 16);
    } else if (hs == 96) {
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<96, 2, 8>), attn_fused_lds<96>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<96, 8, 8>), attn_fused_lds<96>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<96, 16, 8>), attn_fused_lds<96>());
        if (n_part <= 2) ATT_LAUNCH(96, 2);
        else if (n_part <= 8) ATT_LAUNCH(96, 8);
        else ATT_LAUNCH(96, 16);
    } else {
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<128, 2, 8>), attn_fused_lds<128>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<128, 8, 8>), attn_fused_lds<128>());
        DH_MAX_LDS_ONCE((attn_decode_fused_kernel<128, 16, 8>), attn_fused_lds<128>());
        if (n_part <= 2) ATT_LAUNCH(128, 2);
        else if (n_part <= 8) ATT_LAUNCH(128, 8);
        else ATT_LAUNCH(128, 16);
    }
#undef ATT_LAUNCH
#undef CHAIN_LAUNCH
    DH_LAUNCH_CHECK();
    return 0;
}

// the verify step's attention (engine.hip, dh_engine_decode_spec): dh_attn_decode_fused_bf16 for S rows per sequence
int dh_attn_verify_fused_impl(const float* qkv32, int n_part, int pairs, int n_seq, int S, int qkv_dim, int n_ext,
                              const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos,
                              const dh_bf16* sin, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache,
                              dh_bf16* vT_cache, dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int p_max, void* stream) {
    DH_CHECK(qkv32 && cos && sin && seq_slot && kv_len && k_cache && vT_cache && y, "attn_verify_fused: null argument");
    DH_CHECK(n_groups > 0 && n_head % n_groups == 0, "attn_verify_fused: bad head counts");
    DH_CHECK(S >= 2 && S <= 8, "attn_verify_fused: S = %d positions per sequence, 2 .. 8 are served", S);
    DH_CHECK(S * (n_head / n_groups) <= 32, "attn_verify_fused: %d positions x %d heads per group exceed 32 query columns",
             S, n_head / n_groups);
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "attn_verify_fused: head_size %d unsupported", hs);
    DH_CHECK(s_max % 64 == 0 && p_max > 0 && p_max <= s_max && n_part >= 1 && n_part <= MAXP, "attn_verify_fused: bad s_max / p_max / n_part");
    DH_CHECK(qkv_dim == (n_head + 2 * n_groups) * hs, "attn_verify_fused: qkv_dim mismatch");
    DH_CHECK(lora_b == nullptr || n_ext >= 48, "attn_verify_fused: LoRA needs the 48 x·A^T columns");
    if (n_seq <= 0) return 0;
    const float scale = 1.0f / sqrtf((float)hs);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(n_seq * n_groups);
    const int ncol = S * (n_head / n_groups);
#define VER_LAUNCH(HSV, PM)                                                                                           \
    hipLaunchKernelGGL((attn_verify_fused_kernel<HSV, PM, attn_fused_waves<HSV>()>), grid, dim3(64 * attn_fused_waves<HSV>()), attn_verify_lds<HSV>(S, ncol), s, qkv32, n_part, pairs, \
                       n_seq * S, qkv_dim + n_ext, qkv_dim, lora_b, lora_scale, split0, split1, cos, sin, seq_slot, kv_len, k_cache,  \
                       vT_cache, y, n_head, n_groups, s_max, p_max, S, scale)
#define VER_HS(HSV)                                                                                                   \
    do {                                                                                                              \
        DH_MAX_LDS_ONCE((attn_verify_fused_kernel<HSV, 2, attn_fused_waves<HSV>()>), attn_verify_lds<HSV>(8, 32));    \
        DH_MAX_LDS_ONCE((attn_verify_fused_kernel<HSV, 8, attn_fused_waves<HSV>()>), attn_verify_lds<HSV>(8, 32));    \
        DH_MAX_LDS_ONCE((attn_verify_fused_kernel<HSV, 16, attn_fused_waves<HSV>()>), attn_verify_lds<HSV>(8, 32));   \
        if (n_part <= 2) VER_LAUNCH(HSV, 2);                                                                          \
        else if (n_part <= 8) VER_LAUNCH(HSV, 8);                                                                     \
        else VER_LAUNCH(HSV, 16);                                                                                     \
    } while (0)
    if (hs == 64) VER_HS(64);
    else if (hs == 96) VER_HS(96);
    else VER_HS(128);
#undef VER_HS
#undef VER_LAUNCH
    DH_LAUNCH_CHECK();
    return 0;
}

// the op on its own (include/dualhyp_hip.h): what the engine launches, for the op-level tests and other callers
extern "C" int dh_attn_verify_fused_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int S, int qkv_dim, int n_ext,
                                         const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos,
                                         const dh_bf16* sin, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache,
                                         dh_bf16* vT_cache, dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int p_max,
                                         void* stream) {
    return dh_attn_verify_fused_impl(qkv32, n_part, pairs, n_seq, S, qkv_dim, n_ext, lora_b, lora_scale, split0, split1, cos, sin,
                                     seq_slot, kv_len, k_cache, vT_cache, y, n_head, n_groups, hs, s_max, p_max, stream);
}

// launches of attn_shared_fused_kernel this process has issued or captured (dh_attn_shared_launch_count, a test hook)
static int64_t g_attn_shared_launches = 0;
extern "C" int64_t dh_attn_shared_launch_count(void) { return g_attn_shared_launches; }

// dh_attn_decode_fused_bf16 over the same rows, the whole prompt tiles of an utterance streamed once per block of its rows
// (include/dualhyp_hip.h, "Shared-prompt attention"; the engine's step under dh_engine_set_shared_prompt launches it).  tab != null:
// the table variant ("Beam KV tile table"), `name` the entry that refuses.
static int attn_shared_call(const char* name, const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                            const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos, const dh_bf16* sin,
                            const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache, dh_bf16* y, int n_head,
                            int n_groups, int hs, int s_max, int group_rows, const int32_t* prompt_len, const int32_t* tab, int tab_ld,
                            const int32_t* step_dev, void* stream) {
    DH_CHECK(qkv32 && cos && sin && seq_slot && kv_len && k_cache && vT_cache && y, "%s: null argument", name);
    DH_CHECK(prompt_len, "%s: null prompt_len (a device array of n_seq / group_rows int32)", name);
    DH_CHECK(group_rows >= 2 && group_rows <= 8, "%s: group_rows = %d rows per utterance, 2 .. 8 are served", name, group_rows);
    DH_CHECK(n_seq % group_rows == 0, "%s: n_seq = %d rows are not group_rows = %d per utterance", name, n_seq, group_rows);
    DH_CHECK(n_groups > 0 && n_head % n_groups == 0 && n_head / n_groups <= DCOLS, "%s: bad head counts", name);
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "%s: head_size %d unsupported", name, hs);
    DH_CHECK(s_max % 64 == 0 && n_part >= 1 && n_part <= MAXP, "%s: bad s_max / n_part", name);
    DH_CHECK(qkv_dim == (n_head + 2 * n_groups) * hs, "%s: qkv_dim mismatch", name);
    DH_CHECK(lora_b == nullptr || n_ext >= 48, "%s: LoRA needs the 48 x·A^T columns", name);
    DH_CHECK(!tab || (tab_ld >= 1 && tab_ld <= DH_MAX_BEAM_TILES), "%s: a tile table of %d tiles per row, 1 .. %d are served", name, tab_ld,
             DH_MAX_BEAM_TILES);
    if (n_seq <= 0) return 0;
    const float scale = 1.0f / sqrtf((float)hs);
    hipStream_t s = (hipStream_t)stream;
    const int q_per_kv = n_head / n_groups, N = group_rows;
    const int Gs = 32 / q_per_kv, n_cg = (N + Gs - 1) / Gs, r_max = N < Gs ? N : Gs, ncol = r_max * q_per_kv;
    dim3 grid((n_seq / N) * n_cg * n_groups);
    const attn_tab_args<true> ta{tab, step_dev, tab_ld};
#define SHR_LAUNCH(HSV, PM)                                                                                           \
    hipLaunchKernelGGL((attn_shared_fused_kernel<HSV, PM, attn_fused_waves<HSV>()>), grid, dim3(64 * attn_fused_waves<HSV>()), attn_shared_lds<HSV>(r_max, ncol), s, qkv32, n_part, pairs, \
                       n_seq, qkv_dim + n_ext, qkv_dim, lora_b, lora_scale, split0, split1, cos, sin, seq_slot, kv_len, prompt_len, k_cache,  \
                       vT_cache, y, n_head, n_groups, s_max, N, Gs, n_cg, r_max, scale, attn_tab_args<false>{})
#define SHR_TAB_LAUNCH(HSV, PM)                                                                                       \
    hipLaunchKernelGGL((attn_shared_fused_kernel<HSV, PM, attn_fused_waves<HSV>(), true>), grid, dim3(64 * attn_fused_waves<HSV>()), attn_shared_tab_lds<HSV>(r_max, ncol, tab_ld), s, qkv32, n_part, pairs, \
                       n_seq, qkv_dim + n_ext, qkv_dim, lora_b, lora_scale, split0, split1, cos, sin, seq_slot, kv_len, prompt_len, k_cache,  \
                       vT_cache, y, n_head, n_groups, s_max, N, Gs, n_cg, r_max, scale, ta)
#define SHR_HS(HSV)                                                                                                   \
    do {                                                                                                              \
        if (tab) {                                                                                                    \
            DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 2, attn_fused_waves<HSV>(), true>), attn_shared_tab_lds<HSV>(8, 32, DH_MAX_BEAM_TILES));  \
            DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 8, attn_fused_waves<HSV>(), true>), attn_shared_tab_lds<HSV>(8, 32, DH_MAX_BEAM_TILES));  \
            DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 16, attn_fused_waves<HSV>(), true>), attn_shared_tab_lds<HSV>(8, 32, DH_MAX_BEAM_TILES)); \
            if (n_part <= 2) SHR_TAB_LAUNCH(HSV, 2);                                                                  \
            else if (n_part <= 8) SHR_TAB_LAUNCH(HSV, 8);                                                             \
            else SHR_TAB_LAUNCH(HSV, 16);                                                                             \
            break;                                                                                                    \
        }                                                                                                             \
        DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 2, attn_fused_waves<HSV>()>), attn_shared_lds<HSV>(8, 32));    \
        DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 8, attn_fused_waves<HSV>()>), attn_shared_lds<HSV>(8, 32));    \
        DH_MAX_LDS_ONCE((attn_shared_fused_kernel<HSV, 16, attn_fused_waves<HSV>()>), attn_shared_lds<HSV>(8, 32));   \
        if (n_part <= 2) SHR_LAUNCH(HSV, 2);                                                                          \
        else if (n_part <= 8) SHR_LAUNCH(HSV, 8);                                                                     \
        else SHR_LAUNCH(HSV, 16);                                                                                     \
    } while (0)
    if (hs == 64) SHR_HS(64);
    else if (hs == 96) SHR_HS(96);
    else SHR_HS(128);
#undef SHR_HS
#undef SHR_TAB_LAUNCH
#undef SHR_LAUNCH
    DH_LAUNCH_CHECK();
    ++g_attn_shared_launches;
    return 0;
}

extern "C" int dh_attn_decode_shared_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                                          const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos,
                                          const dh_bf16* sin, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache,
                                          dh_bf16* vT_cache, dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int group_rows,
                                          const int32_t* prompt_len, void* stream) {
    return attn_shared_call("dh_attn_decode_shared_bf16", qkv32, n_part, pairs, n_seq, qkv_dim, n_ext, lora_b, lora_scale, split0, split1,
                            cos, sin, seq_slot, kv_len, k_cache, vT_cache, y, n_head, n_groups, hs, s_max, group_rows, prompt_len, nullptr, 0,
                            nullptr, stream);
}

// the same call with the rows' private tiles read through a tile table ("Beam KV tile table" of the header)
extern "C" int dh_attn_decode_shared_tab_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                                              const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos,
                                              const dh_bf16* sin, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache,
                                              dh_bf16* vT_cache, dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int group_rows,
                                              const int32_t* prompt_len, const int32_t* tile_tab, int tab_ld, const int32_t* step_dev,
                                              void* stream) {
    DH_CHECK(tile_tab, "dh_attn_decode_shared_tab_bf16: null tile table (dh_attn_decode_shared_bf16 is the entry without one)");
    return attn_shared_call("dh_attn_decode_shared_tab_bf16", qkv32, n_part, pairs, n_seq, qkv_dim, n_ext, lora_b, lora_scale, split0,
                            split1, cos, sin, seq_slot, kv_len, k_cache, vT_cache, y, n_head, n_groups, hs, s_max, group_rows, prompt_len,
                            tile_tab, tab_ld, step_dev, stream);
}

// finish_norm_kernel<, true> from this many rows on.  tools/sweep_finish.py, d 2048, us per launch, loads behind | ahead of the
// barrier (8 partials + LoRA / 4 pair sums + LoRA / 11 partials, three alternating repeats, spread <= 0.1 us):
//    32 rows   5.6 |  5.6    4.9 |  4.8    3.8 |  3.8        64 rows   5.9 |  5.8    5.0 |  4.9    3.9 | 3.9
//   128 rows   7.0 |  6.7    5.2 |  5.1    5.3 |  4.9       256 rows   8.5 |  8.1    6.3 |  6.0    6.7 | 6.5
//   640 rows  16.0 | 15.8   12.3 | 11.8   12.0 | 11.8
// No difference beyond the spread at 32 and 64 rows; ahead in all three shapes from 128 rows on.
constexpr int FINISH_HOIST_ROWS = 128;
// finish_norm_rows_kernel from this many rows on (0: never), FINISH_RPB rows per block.  tools/sweep_finish.py, d 2048, us per launch,
// finish_norm_kernel (the faster of loads behind | ahead) against 2 / 3 / 4 rows per block, three alternating repeats, spread <= 0.2 us:
//                 4 pair sums + LoRA          6 pair sums               1 partial + LoRA           1 partial
//    32 rows    4.9 |  8.0 10.5 12.8      3.2 |  5.1  6.6  8.1       4.7 |  7.2  9.3 11.2      2.9 | 3.6 4.4 5.2
//   128 rows    5.2 |  8.2 11.1 13.0      3.4 |  5.2  7.0  8.3       4.9 |  7.3  9.4 11.3      3.1 | 3.6 4.5 5.3
//   640 rows   11.7 | 13.8 13.2 15.8      8.4 | 10.1 10.3 11.1       9.6 | 10.8 10.3 12.2      4.5 | 4.8 5.2 6.0
//  2048 rows   31.4 | 27.8 29.3 25.3     24.0 | 25.0 26.0 24.1      22.5 | 20.7 21.2 18.3      8.6 | 9.0 9.2 9.1
// Half the blocks with twice the rows each do not hide more latency than the co-resident one-row blocks do up to 640 rows: behind at
// every shape there.  What the rows kernel saves is lora_b: a thread's 8 x 32 B sit 256 B apart from its neighbour's, 64 cache lines
// per load instruction, and finish_norm_kernel pays that once per row (LoRA costs it 1.8 us at 128 rows, 5.4 at 640, 14 at 2048);
// four rows per block pay it once per four rows.  At 2048 rows, where the partial-sum GEMMs hand over one partial (g_chain_min_rows), a
// layer's two launches take 22.5 + 8.6 against 18.3 + 9.1 us: ahead by 3.7 us, on from there.  MEASUREMENTS.md has the whole table.
constexpr int FINISH_ROWS_MIN = 2048;
constexpr int FINISH_RPB = 4;

extern "C" int dh_finish_norm_bf16(const float* h32, int n_part, int pairs, int rows, int d, int n_ext, const dh_bf16* lora_b,
                                   float lora_scale, const dh_bf16* x_resid, const dh_bf16* w_norm, dh_bf16* x_out,
                                   dh_bf16* xn_out, float eps, const uint8_t* row_tail, void* stream) {
    DH_CHECK(h32 && x_resid && w_norm && x_out && xn_out, "dh_finish_norm_bf16: null argument");
    DH_CHECK(d % 8 == 0 && d <= 8192 && n_part >= 1 && n_part <= MAXP, "dh_finish_norm_bf16: unsupported d=%d", d);
    DH_CHECK(lora_b == nullptr || n_ext >= 16, "dh_finish_norm_bf16: LoRA needs the 16 x·A^T columns");
    DH_CHECK((d + n_ext) % 4 == 0, "dh_finish_norm_bf16: row stride must be a multiple of 4 floats");
    if (rows <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(rows), block(256);
    const int ldh = d + n_ext;
#define LAUNCH(MAXC) do {                                                                                             \
        if (hoist) hipLaunchKernelGGL((finish_norm_kernel<MAXC, true>), grid, block, 0, s, h32, n_part, pairs, rows, ldh, lora_b,  \
                                      lora_scale, x_resid, w_norm, x_out, xn_out, d, eps, row_tail);                  \
        else hipLaunchKernelGGL((finish_norm_kernel<MAXC, false>), grid, block, 0, s, h32, n_part, pairs, rows, ldh, lora_b,       \
                                lora_scale, x_resid, w_norm, x_out, xn_out, d, eps, row_tail);                        \
    } while (0)
    const int multi_rows = g_finish_rows_min >= 0 ? g_finish_rows_min : FINISH_ROWS_MIN;
    if (multi_rows > 0 && rows >= multi_rows) {                   // by the row count only, never by how the rows are packed
        const int rpb = g_finish_rpb > 0 ? g_finish_rpb : FINISH_RPB;
        dim3 mgrid((rows + rpb - 1) / rpb);
#define LAUNCH_ROWS(MAXC, PF, XP, LORA)                                                                                  \
        hipLaunchKernelGGL((finish_norm_rows_kernel<MAXC, PF, XP, LORA>), mgrid, block, 0, s, h32, n_part, pairs, rows, ldh, lora_b,  \
                           lora_scale, x_resid, w_norm, x_out, xn_out, d, eps, row_tail, rpb)
#define LAUNCH_MAXC(MAXC) do {                                                                                        \
        if (lora_b != nullptr) {                                                                                      \
            if (n_part <= 1) LAUNCH_ROWS(MAXC, 1, 1, true);                                                           \
            else if (n_part <= 4) LAUNCH_ROWS(MAXC, 4, 4, true);                                                      \
            else LAUNCH_ROWS(MAXC, 4, MAXP, true);                                                                    \
        } else if (n_part <= 1) LAUNCH_ROWS(MAXC, 1, 1, false);                                                       \
        else if (n_part <= 4) LAUNCH_ROWS(MAXC, 4, 1, false);                                                         \
        else LAUNCH_ROWS(MAXC, 8, 1, false);                                                                          \
    } while (0)
        if (d <= 2048) LAUNCH_MAXC(1);
        else if (d <= 4096) LAUNCH_MAXC(2);
        else LAUNCH_MAXC(4);
#undef LAUNCH_MAXC
#undef LAUNCH_ROWS
        DH_LAUNCH_CHECK();
        return 0;
    }
    const int hoist_rows = g_finish_hoist_rows >= 0 ? g_finish_hoist_rows : FINISH_HOIST_ROWS;
    const bool hoist = hoist_rows > 0 && rows >= hoist_rows;     // by the row count only, never by how the rows are packed
    if (d <= 2048) { LAUNCH(1); }
    else if (d <= 4096) { LAUNCH(2); }
    else { LAUNCH(4); }
#undef LAUNCH
    DH_LAUNCH_CHECK();
    return 0;
}
