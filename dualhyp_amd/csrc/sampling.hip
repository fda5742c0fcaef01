// The tail of the decode loop (generate/base.py:62-80) fused into one kernel per step:
// temperature -> top-k crop (-> nucleus / min-p crop, where asked for) -> softmax -> draw -> append token -> EOS flag.  One 1024-thread
// block per sequence; nothing returns to the host.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t bf16_key(bf16_t v) {
    // monotone map bf16 bits -> uint16 key (larger value = larger key).  -0 takes +0's key: the reference crops with
    // `l < kth`, for which the two zeros are equal, so a zero of either sign at the threshold keeps both
    if ((v & 0x7FFFu) == 0) return 0x8000u;
    return (v & 0x8000u) ? (uint32_t)(~v & 0xFFFFu) : (uint32_t)(v | 0x8000u);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr int NT = 1024;
constexpr bf16_t BF16_NEG_INF = 0xFF80u;

// Token masks (include/dualhyp_hip.h): bit i & 31 of word i >> 5 of the sequence's mask row is set when token i is allowed.  Only
// columns below vocab are ever asked for, so the bits behind them are never read.
__device__ __forceinline__ bool mask_allows(const uint32_t* __restrict__ mrow, int i) { return (mrow[i >> 5] >> (i & 31)) & 1u; }
// the mask byte of the 8 columns 8 c .. 8 c + 7 (a 16-byte load of the row)
__device__ __forceinline__ uint32_t mask_byte(const uint32_t* __restrict__ mrow, int c) { return (mrow[c >> 2] >> ((c & 3) * 8)) & 255u; }

// Penalties (include/dualhyp_hip.h): the columns a sequence's history overrides, as pen_build leaves them in LDS.  bits: the mask row's
// layout, bit t set when id t occurs in the history; pre[w]: the number of set bits in the words before w, so a set bit's rank among
// the set bits — its place in val — is pre[w] plus the set bits below it in its word; val[rank]: a_t.
struct pen_view {
    const uint32_t* bits = nullptr;
    const uint16_t* pre = nullptr;
    const bf16_t* val = nullptr;
};
__device__ __forceinline__ int pen_rank(const pen_view& ov, int t) {
    return (int)ov.pre[t >> 5] + __popc(ov.bits[t >> 5] & ((1u << (t & 31)) - 1u));
}
// column i of the row the pick sees
__device__ __forceinline__ bf16_t pen_value(const pen_view& ov, const bf16_t* __restrict__ lg, int i) {
    bf16_t v = lg[i];                                   // a global load and, for the few overridden columns, an LDS load: never a flat one
    if (mask_allows(ov.bits, i)) v = ov.val[pen_rank(ov, i)];
    return v;
}
// a_t of the header from the raw value and the id's count c: the HF rule, then three separately rounded fp32 operations (the compiler
// contracts a product and a difference into an FMA unless told not to), then the bf16 rounding.  penalised_z: z, the fp32 value in
// front of that rounding, which a boost is added to ("Contextual biasing").
__device__ __forceinline__ float penalised_z(bf16_t raw, int c, const dh_penalty_args& pen) {
#pragma clang fp contract(off)
    const float x = bf2f(raw);
    const float y = x < 0.f ? x * pen.repetition : x / pen.repetition;
    const float p = pen.frequency * (float)c;
    const float d = y - p;
    const float z = d - pen.presence;
    return z;
}
__device__ __forceinline__ bf16_t penalised(bf16_t raw, int c, const dh_penalty_args& pen) { return f2bf(penalised_z(raw, c, pen)); }

// Contextual biasing (include/dualhyp_hip.h): a boost as an unsigned key with the floats' order, so the largest of an id's boosts is an
// integer atomicMax, exact in any order.  A finite boost's key is never 0, which is "no boost".
__device__ __forceinline__ uint32_t bias_key(float b) {
    const uint32_t u = __float_as_uint(b);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float bias_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
// bf16(y + B): one fp32 add, never part of an FMA, then round to nearest even
__device__ __forceinline__ bf16_t boosted(float y, float b) {
#pragma clang fp contract(off)
    const float s = y + b;
    return f2bf(s);
}

// The pick of one sequence's next token from its logits row `lg`, by the whole 1024-thread block; every thread
// returns it.  The draw is keyed by (seed, step, seq).
// MASK: every logit that feeds the pick goes through the sequence's mask row `mrow` first and is bf16 -inf where the token is not
// allowed, so the pick is the unmasked pick on a copy of the row with -inf in those columns.  Off: `mrow` is not read.
// nuc ("Nucleus and min-p" of the header; launch-uniform, off: the sampled branch runs what it always ran): the crop's threshold key is
// raised to that of the kept set K0 n nucleus(K0) n min_p before the sums.  The scheme:
//   m is the maximum of the scaled row (top_k keeps it), w_i = __expf(l_i - m), the term the CDF walk itself adds.
//   min_p  an entry passes iff fl32(l_i - m) >= lmin; the smallest key that passes is a block-wide integer minimum.
//   top_p  masses are fixed-point integers q_i = (uint64)(w_i * 2^40), added with 64-bit integer LDS atomics: exact in any order, and
//          131072 entries of at most 2^40 fit.  Pass 0 histograms the entries of K0 into 256 bins by the high byte of bf16_key, thread 0
//          walks the bins from the top until the mass above a bin plus the bin reaches P = clamp((uint64)(top_p * T_int), 1, T_int),
//          T_int the sum of all bins; pass 1 repeats it on the low byte inside that bin.  The value found is the lowest v with
//          A(v) < P, A the mass strictly above v: ties share a key, so they stay together, and the clamp makes a crossing exist.
// No floating-point sum feeds the threshold, and every entry goes through scaled(i): the kept set is a function of the row's bytes,
// vocab and the parameters, wherever the row lies.
// PEN ("Penalties" of the header; only pick_token_banned asks for it): every read of the row that feeds the pick takes column i's value
// from `ov` where the sequence's history overrides it (pen_value below), so the pick is the PEN = false pick on a copy of the row with
// a_t in those columns.  Off: `ov` is not read, and the code is what it always was.
template <bool MASK, bool PEN = false>
__device__ __forceinline__ int pick_token(const bf16_t* __restrict__ lg, int vocab, float temperature, int top_k,
                                          uint64_t seed, int step, int seq, const uint32_t* __restrict__ mrow,
                                          const dh_nucleus_args nuc = dh_nucleus_args{}, const pen_view ov = pen_view{}) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float s_f[NT / 64];
    __shared__ int s_i[NT / 64];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_sel[2];

    // l = bf16(logit / temperature)   (generate/base.py:62, bf16 tensor / python float)
    auto scaled = [&](int i) -> bf16_t {
        if constexpr (MASK) { if (!mask_allows(mrow, i)) return BF16_NEG_INF; }      // -inf / temperature
        if constexpr (PEN) return f2bf(bf2f(pen_value(ov, lg, i)) / temperature);
        return f2bf(bf2f(lg[i]) / temperature);
    };

    int choice = 0;
    if (top_k == 1) {
        // arg-max, lowest index among equal maxima (NaN never wins: it is not > anything)
        float best = -INFINITY;
        int bi = 0x7fffffff;
        if ((vocab & 7) == 0 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0) {
            // 16-byte loads, all of a thread's requests in flight before the first compare (the 2-byte strided loop took
            // 15.8 us for a 32-row step's 2 MB of logits: one dependent compare chain behind 32 small loads per thread);
            // the tie rule carries the index, so the visiting order is free
            const uint4* lg4 = reinterpret_cast<const uint4*>(lg);
            const int n4 = vocab >> 3;
            for (int c0 = tid; c0 < n4; c0 += 4 * NT) {
                uint4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) q[u] = c0 + u * NT < n4 ? lg4[c0 + u * NT] : uint4{0, 0, 0, 0};
                uint32_t mb[4];
                if constexpr (MASK) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) mb[u] = c0 + u * NT < n4 ? mask_byte(mrow, c0 + u * NT) : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (c0 + u * NT >= n4) break;
                    const bf16_t* e8 = reinterpret_cast<const bf16_t*>(&q[u]);
                    uint32_t ob = 0u;                           // PEN: which of the 8 columns are overridden (mostly none); read here, one
                    if constexpr (PEN) ob = mask_byte(ov.bits, c0 + u * NT);     // at a time: four held across the loads cost registers
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int i = (c0 + u * NT) * 8 + e;
                        bf16_t raw = e8[e];
                        if constexpr (PEN) { if ((ob >> e) & 1u) raw = ov.val[pen_rank(ov, i)]; }
                        float v = bf2f(f2bf(bf2f(raw) / temperature));
                        if constexpr (MASK) { if (!((mb[u] >> e) & 1u)) v = -INFINITY; }
                        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
                    }
                }
            }
        } else {
        for (int i = tid; i < vocab; i += NT) {
            const float v = bf2f(scaled(i));
            if (v > best || (v == best && i < bi)) { best = v; bi = i; }
        }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { s_f[wave] = best; s_i[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NT / 64; ++w)
                if (s_f[w] > best || (s_f[w] == best && s_i[w] < bi)) { best = s_f[w]; bi = s_i[w]; }
            s_i[0] = bi == 0x7fffffff ? 0 : bi;
        }
        __syncthreads();
        choice = s_i[0];
    } else {
        // ---- threshold = k-th largest scaled logit: two-pass radix select on the 16-bit keys
        uint32_t thr_key = 0;
        if (top_k > 0 && top_k < vocab) {
            uint32_t prefix = 0;
            int need = top_k;
            for (int pass = 0; pass < 2; ++pass) {
                for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
                __syncthreads();
                for (int i = tid; i < vocab; i += NT) {
                    const uint32_t k = bf16_key(scaled(i));
                    if (pass == 0) atomicAdd(&s_hist[k >> 8], 1u);
                    else if ((k >> 8) == prefix) atomicAdd(&s_hist[k & 255], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    int b = 255, acc = 0;
                    for (; b > 0; --b) {
                        if (acc + (int)s_hist[b] >= need) break;
                        acc += s_hist[b];
                    }
                    s_sel[0] = b;
                    s_sel[1] = need - acc;
                }
                __syncthreads();
                if (pass == 0) prefix = s_sel[0]; else thr_key = (prefix << 8) | s_sel[0];
                need = s_sel[1];
                __syncthreads();
            }
        }
        // ---- softmax over kept entries (fp32), then inverse-CDF draw in index order
        float mx = -INFINITY;
        for (int i = tid; i < vocab; i += NT) {
            const bf16_t v = scaled(i);
            if (bf16_key(v) >= thr_key) mx = fmaxf(mx, bf2f(v));
        }
        mx = wave_max(mx);
        if (lane == 0) s_f[wave] = mx;
        __syncthreads();
        mx = s_f[0];
        for (int w = 1; w < NT / 64; ++w) mx = fmaxf(mx, s_f[w]);
        __syncthreads();
        if (nuc.on()) {                                    // the same for every thread of the launch
            __shared__ unsigned long long s_mass[256];
            __shared__ unsigned long long s_need;
            __shared__ unsigned s_minkey;
            uint32_t nuc_key = 0;
            if (nuc.top_p < 1.f) {
                uint32_t prefix = 0;
                unsigned long long need = 0;
                for (int pass = 0; pass < 2; ++pass) {
                    for (int i = tid; i < 256; i += NT) s_mass[i] = 0ull;
                    __syncthreads();
                    for (int i = tid; i < vocab; i += NT) {
                        const bf16_t v = scaled(i);
                        const uint32_t k = bf16_key(v);
                        if (k < thr_key) continue;
                        if (pass == 1 && (k >> 8) != prefix) continue;
                        const unsigned long long q = (unsigned long long)(__expf(bf2f(v) - mx) * 1099511627776.0f);   // 2^40
                        if (q) atomicAdd(&s_mass[pass == 0 ? k >> 8 : k & 255], q);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        if (pass == 0) {
                            unsigned long long tot = 0;
                            for (int b = 0; b < 256; ++b) tot += s_mass[b];
                            need = (unsigned long long)((double)nuc.top_p * (double)tot);
                            need = need < 1ull ? 1ull : need > tot ? tot : need;
                        }
                        int b = 255;
                        unsigned long long acc = 0;
                        for (; b > 0; --b) {
                            if (acc + s_mass[b] >= need) break;
                            acc += s_mass[b];
                        }
                        s_sel[0] = b;
                        s_need = need - acc;                   // the mass still wanted inside bin b
                    }
                    __syncthreads();
                    if (pass == 0) prefix = s_sel[0]; else nuc_key = (prefix << 8) | s_sel[0];
                    need = s_need;
                    __syncthreads();
                }
            }
            if (nuc.min_p_on) {
                if (tid == 0) s_minkey = 0xFFFFFFFFu;
                __syncthreads();
                uint32_t lowest = 0xFFFFFFFFu;
                for (int i = tid; i < vocab; i += NT) {
                    const bf16_t v = scaled(i);
                    if (bf2f(v) - mx >= nuc.lmin) lowest = min(lowest, bf16_key(v));
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) lowest = min(lowest, (uint32_t)__shfl_xor((int)lowest, o, 64));
                if (lane == 0) atomicMin(&s_minkey, lowest);
                __syncthreads();
                nuc_key = max(nuc_key, s_minkey);
                __syncthreads();
            }
            thr_key = max(thr_key, nuc_key);
        }
        // contiguous slab per thread so the CDF is in index order
        const int per = (vocab + NT - 1) / NT;
        const int lo = tid * per, hi = min(vocab, lo + per);
        float mine = 0.f;
        for (int i = lo; i < hi; ++i) {
            const bf16_t v = scaled(i);
            if (bf16_key(v) >= thr_key) mine += __expf(bf2f(v) - mx);
        }
        // block exclusive scan of `mine` (wave scan + wave totals)
        float incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_f[wave] = incl;
        __syncthreads();
        float base = 0.f, total = 0.f;
        for (int w = 0; w < NT / 64; ++w) {
            if (w < wave) base += s_f[w];
            total += s_f[w];
        }
        const float excl = base + incl - mine;
        const uint64_t h = mix64(seed ^ mix64(((uint64_t)step << 32) | (uint32_t)seq));
        const float u = (float)(h >> 40) * (1.0f / 16777216.0f) * total;   // in [0, total)
        if (tid == 0) s_i[0] = -1;
        __syncthreads();
        if (mine > 0.f && u >= excl && u < excl + mine) {
            float c = excl;
            int pick = lo;
            for (int i = lo; i < hi; ++i) {
                const bf16_t v = scaled(i);
                if (bf16_key(v) >= thr_key) {
                    pick = i;
                    c += __expf(bf2f(v) - mx);
                    if (u < c) break;
                }
            }
            atomicMax(&s_i[0], pick);
        }
        __syncthreads();
        if (tid == 0 && s_i[0] < 0) {   // rounding left u past the last bin: take the arg-max
            int bi = 0; float best = -INFINITY;
            for (int i = 0; i < vocab; ++i) { const float v = bf2f(scaled(i)); if (v > best) { best = v; bi = i; } }
            s_i[0] = bi;
        }
        __syncthreads();
        choice = s_i[0];
    }
    return choice;
}

// No-repeat n-grams (include/dualhyp_hip.h): the static LDS row of allowed-minus-banned bits, ceil(vocab / 32) words
constexpr int BAN_MAX_VOCAB = 131072;
constexpr int MAX_NGRAM = 8;

// The sequence's pick row under no_repeat_ngram = ngram (1 .. MAX_NGRAM), by the whole block: g[0..m) are the tokens it has generated,
// the row starts from the mask row `mrow` (MASK) or from all ones, loses bit g[i + ngram - 1] for every i in [0, m - ngram] with
// g[i .. i + ngram - 1) == g[m - ngram + 1 .. m), and is the start row again when that left no bit below vocab (the fallback: the pick
// is never taken from an empty set).  Every thread gets the LDS row, in the mask row's layout with the bits at and behind vocab clear;
// it holds until the block's next call, which the caller separates from the pick's last read by a barrier (pick_token ends on one).
// KEEP (the beam candidates, "Beam histories"): the fallback is taken when fewer than `keep` bits are left, not when none is.
// ae ("Automaton constraints" of the header; launch-uniform, off: the start row it always was): the start row is the bits of the state's
// edge tokens ae.tok[ae.lo .. ae.hi), ANDed with the mask row (MASK), or bit ae.eos alone where that leaves none — set with LDS atomicOr
// by every thread at stride NT, so a state may hold more edges than the block has threads; the ban and its fallback then work on it.
struct aut_edges {
    const int32_t* tok = nullptr;                       // null: no automaton
    int lo = 0, hi = 0;                                 // the state's edge range, inside [0, n_edges]
    int eos = 0;                                        // the call's eos_id, in [0, vocab)
};
template <bool MASK, bool KEEP = false>
__device__ __forceinline__ const uint32_t* ban_row(const int64_t* g, int m, int ngram, int vocab, const uint32_t* __restrict__ mrow,
                                                   int keep = 1, const aut_edges ae = aut_edges{}) {
    __shared__ uint32_t s_row[BAN_MAX_VOCAB / 32];
    __shared__ int s_cnt[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (vocab + 31) >> 5;
    const uint32_t tail = (vocab & 31) ? (1u << (vocab & 31)) - 1u : ~0u;
    auto start_word = [&](int w) -> uint32_t {
        uint32_t v = ~0u;
        if constexpr (MASK) v = mrow[w];
        return w == nw - 1 ? v & tail : v;
    };
    // the row's set bits, by the whole block (an integer sum: exact in any order); the caller keeps a barrier between two calls
    auto count_row = [&]() -> int {
        int cnt = 0;
        for (int w = tid; w < nw; w += NT) cnt += __popc(s_row[w]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        cnt = 0;
        for (int w = 0; w < NT / 64; ++w) cnt += s_cnt[w];
        return cnt;
    };
    // the start row, ending on a barrier
    auto fill_start = [&]() {
        if (ae.tok) {                                   // the same for every thread of the launch
            for (int w = tid; w < nw; w += NT) s_row[w] = 0u;
            __syncthreads();
            for (int e = ae.lo + tid; e < ae.hi; e += NT) {
                const int t = ae.tok[e];
                if (t < 0 || t >= vocab) continue;      // the host has refused such an edge
                uint32_t bit = 1u << (t & 31);
                if constexpr (MASK) bit &= mrow[t >> 5];
                if (bit) atomicOr(&s_row[t >> 5], bit);
            }
            __syncthreads();
            if (count_row() == 0) {                     // a dead end, the same for every thread: the EOS alone, mask or not
                if (tid == 0 && ae.eos >= 0 && ae.eos < vocab) s_row[ae.eos >> 5] = 1u << (ae.eos & 31);
                __syncthreads();
            }
        } else {
            for (int w = tid; w < nw; w += NT) s_row[w] = start_word(w);
            __syncthreads();
        }
    };
    fill_start();
    if (ngram == 0 || m < ngram) return s_row;          // the same for every thread: no ban (a penalty alone), or no n-gram is complete yet
    int64_t suf[MAX_NGRAM - 1];                         // the (ngram - 1)-token suffix every candidate is tested against
#pragma unroll
    for (int j = 0; j < MAX_NGRAM - 1; ++j) suf[j] = j < ngram - 1 ? g[m - ngram + 1 + j] : 0;
    for (int i = tid; i <= m - ngram; i += NT) {
        bool eq = true;
#pragma unroll
        for (int j = 0; j < MAX_NGRAM - 1; ++j)
            if (j < ngram - 1 && g[i + j] != suf[j]) eq = false;
        if (eq) {
            const int64_t t = g[i + ngram - 1];
            if (t >= 0 && t < vocab) atomicAnd(&s_row[t >> 5], ~(1u << (t & 31)));
        }
    }
    __syncthreads();
    // everything banned?  popcount of the row (an integer sum: exact in any order)
    const int cnt = count_row();
    bool refill = cnt == 0;                             // the same for every thread
    if constexpr (KEEP) refill = cnt < keep;
    if (refill) fill_start();
    return s_row;
}

// Penalties (include/dualhyp_hip.h): the static LDS tables bound the history, and with it the distinct ids, of a penalised pick
constexpr int PEN_MAX_HISTORY = DH_MAX_PENALTY_HISTORY;
constexpr size_t PEN_LDS_BYTES = (BAN_MAX_VOCAB / 32) * (sizeof(uint32_t) + sizeof(uint16_t)) + PEN_MAX_HISTORY * (sizeof(uint32_t) + sizeof(bf16_t)) +
                                 DH_MAX_BIAS_LEN * sizeof(int32_t);     // and the bias' tail of the generated tokens
static_assert(PEN_MAX_HISTORY <= 65535 && BAN_MAX_VOCAB / 32 == 4 * NT, "pen_build: uint16 ranks, four words of the bit row per thread");

// Contextual biasing (include/dualhyp_hip.h): every thread of the block takes two (entry, depth) pairs, and a history's token two places
static_assert(DH_MAX_BIAS_ENTRIES * DH_MAX_BIAS_LEN == 2 * NT && PEN_MAX_HISTORY == 2 * NT && DH_MAX_BIAS_LEN == 8,
              "pen_build: two pairs and two history places per thread, depth = pair & 7");

// The columns a sequence overrides at a pick, by the whole block, from its generated tokens g[0..m_all):
//   under the penalties `pen` (on or off, launch-uniform) the distinct ids of g below vocab with their counts c_t, each holding
//     a_t = bf16(z), z = penalised_z(lg[t], c_t);
//   under the bias `bias` (n > 0 or off, launch-uniform) the ids its entries propose, each holding bf16(y + B_t): y is z where the id is
//     in the penalised history and float(lg[t]) where not, B_t the largest boost of its proposers.
// pen_view above says where.  Set membership is an LDS atomicOr, a count an integer LDS atomicAdd, a rank a prefix sum of popcounts, B_t
// an integer LDS atomicMax on bias_key: exact whatever order the threads arrive in.  Every writer of an id's value writes the same bits
// from the same operands.  With both on, the counts move to registers and their table holds the boost keys: the tables keep their size.
// Every thread gets the view; it holds until the block's next call.  The host refuses what the tables could not hold
// (check_pick); the clamp only keeps a longer history inside them.
__device__ __forceinline__ pen_view pen_build(const bf16_t* __restrict__ lg, int vocab, const int64_t* g, int m_all, const dh_penalty_args& pen,
                                              const dh_bias_args& bias) {
    // the tables live in the launch's dynamic LDS (PEN_LDS_BYTES, asked for only when a penalty or a bias is on): the n-gram-only
    // launches of the family keep the static LDS, and with it the residency, they had
    extern __shared__ __align__(16) unsigned char s_pen[];
    uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_pen);                 // [BAN_MAX_VOCAB / 32]
    uint32_t* s_cnt = s_bits + BAN_MAX_VOCAB / 32;                          // [PEN_MAX_HISTORY]: counts, then (bias on) boost keys
    uint16_t* s_pre = reinterpret_cast<uint16_t*>(s_cnt + PEN_MAX_HISTORY); // [BAN_MAX_VOCAB / 32]
    bf16_t* s_val = s_pre + BAN_MAX_VOCAB / 32;                             // [PEN_MAX_HISTORY]
    int32_t* s_tail = reinterpret_cast<int32_t*>(s_val + PEN_MAX_HISTORY);  // [DH_MAX_BIAS_LEN - 1]: g[m_all - 7 .. m_all), -1 where none
    __shared__ uint32_t s_wtot[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (vocab + 31) >> 5;
    const bool pen_on = dh_penalty_on(pen), bias_on = bias.n > 0;
    const int m = !pen_on ? 0 : m_all < PEN_MAX_HISTORY ? m_all : PEN_MAX_HISTORY;      // the history the penalties count
    for (int w = tid; w < nw; w += NT) s_bits[w] = 0u;
    for (int i = tid; i < PEN_MAX_HISTORY; i += NT) s_cnt[i] = 0u;
    if (bias_on && tid < DH_MAX_BIAS_LEN - 1) {         // the tail every pair is matched against, read from the token row once
        const int i = m_all - (DH_MAX_BIAS_LEN - 1) + tid;
        int32_t v = -1;                                 // no entry id equals it
        if (i >= 0) {
            const int64_t t = g[i];
            if (t >= 0 && t < vocab) v = (int32_t)t;
        }
        s_tail[tid] = v;
    }
    __syncthreads();
    for (int i = tid; i < m; i += NT) {
        const int64_t t = g[i];
        if (t >= 0 && t < vocab) atomicOr(&s_bits[t >> 5], 1u << (t & 31));
    }
    // pair p = (entry p >> 3, depth k = p & 7) proposes ids[k] when g's last k tokens are ids[0 .. k)
    int bt[2] = {-1, -1};
    uint32_t bk[2] = {0u, 0u};
    if (bias_on) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = tid + j * NT, e = p >> 3, k = p & (DH_MAX_BIAS_LEN - 1);
            if (e >= bias.n || k >= bias.len[e] || k > m_all) continue;
            const int32_t* ids = bias.ids + (size_t)e * DH_MAX_BIAS_LEN;
            bool eq = true;
#pragma unroll
            for (int q = 0; q < DH_MAX_BIAS_LEN - 1; ++q)
                if (q < k && s_tail[DH_MAX_BIAS_LEN - 1 - k + q] != ids[q]) eq = false;
            const int t = ids[k];
            if (eq && t >= 0 && t < vocab) {
                bt[j] = t;
                bk[j] = bias_key(bias.boost[e]);
                atomicOr(&s_bits[t >> 5], 1u << (t & 31));
            }
        }
    }
    __syncthreads();
    // exclusive prefix of the words' popcounts: thread t owns words 4 t .. 4 t + 3, a wave scan, then the wave totals
    uint32_t pc[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pc[j] = 4 * tid + j < nw ? __popc(s_bits[4 * tid + j]) : 0u;
        mine += pc[j];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    uint32_t run = incl - mine;
    for (int w = 0; w < wave; ++w) run += s_wtot[w];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (4 * tid + j < nw) s_pre[4 * tid + j] = (uint16_t)run;
        run += pc[j];
    }
    __syncthreads();
    const pen_view ov{s_bits, s_pre, s_val};
    if (pen_on) {
        for (int i = tid; i < m; i += NT) {
            const int64_t t = g[i];
            if (t >= 0 && t < vocab) atomicAdd(&s_cnt[pen_rank(ov, (int)t)], 1u);
        }
        __syncthreads();
    }
    uint32_t hc[2] = {0u, 0u};                          // pen and bias on: the counts of this thread's two history places
    if (bias_on) {
        if (pen_on) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int i = tid + j * NT;
                if (i < m) {
                    const int64_t t = g[i];
                    if (t >= 0 && t < vocab) hc[j] = s_cnt[pen_rank(ov, (int)t)];
                }
            }
            __syncthreads();
            for (int i = tid; i < PEN_MAX_HISTORY; i += NT) s_cnt[i] = 0u;
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (bt[j] >= 0) atomicMax(&s_cnt[pen_rank(ov, bt[j])], bk[j]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; ++j) {                   // an id outside the penalised history: y = float(raw); one inside is written below
            if (bt[j] >= 0) {
                const int r = pen_rank(ov, bt[j]);
                s_val[r] = boosted(bf2f(lg[bt[j]]), bias_unkey(s_cnt[r]));
            }
        }
        __syncthreads();
    }
    if (pen_on) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + j * NT;
            if (i >= m) continue;
            const int64_t t = g[i];
            if (t >= 0 && t < vocab) {
                const int r = pen_rank(ov, (int)t);
                const uint32_t key = bias_on ? s_cnt[r] : 0u;
                const float z = penalised_z(lg[t], (int)(bias_on ? hc[j] : s_cnt[r]), pen);
                s_val[r] = key ? boosted(z, bias_unkey(key)) : f2bf(z);
            }
        }
        __syncthreads();
    }
    return ov;
}

// Automaton constraints (include/dualhyp_hip.h): the state sequence u is in at a pick behind m generated tokens, and its edge range as
// ban_row takes it.  The host has checked the arrays' host copies; the clamps only keep a read inside the device arrays whatever they hold.
__device__ __forceinline__ aut_edges aut_range(const dh_automaton_args& aut, int q, int64_t eos_id) {     // q in [0, n_states)
    int lo = aut.edge_off[q], hi = aut.edge_off[q + 1];
    hi = hi < 0 ? 0 : hi > aut.n_edges ? aut.n_edges : hi;
    lo = lo < 0 ? 0 : lo > hi ? hi : lo;
    return aut_edges{aut.edge_tok, lo, hi, (int)eos_id};
}
__device__ __forceinline__ aut_edges aut_state(const dh_automaton_args& aut, int u, int m, int64_t eos_id, int& q) {
    q = m == 0 ? aut.init[u] : aut.state[u];
    if (q < 0 || q >= aut.n_states) q = 0;
    return aut_range(aut, q, eos_id);
}
// The transition behind the pick `choice`, by the whole block: state[u] = edge_dst[e] of q's edge on `choice`, or q where it has none.  An
// edge is unique per (state, token), so at most one thread finds it; thread 0 stores the result with a plain vector store.  The read of
// state[u] in aut_state lies behind the row build's and the pick's barriers, and no other block touches the entry.
__device__ __forceinline__ void aut_step(const dh_automaton_args& aut, const aut_edges& ae, int q, int choice, int u) {
    __shared__ int s_next;
    const int tid = threadIdx.x;
    if (tid == 0) s_next = q;
    __syncthreads();
    for (int e = ae.lo + tid; e < ae.hi; e += NT) {
        if (ae.tok[e] == choice) {
            const int d = aut.edge_dst[e];
            if (d >= 0 && d < aut.n_states) s_next = d;
        }
    }
    __syncthreads();
    if (tid == 0) aut.state[u] = s_next;
}
// aut_step's lookup for a verify step's draw mode, which moves the state in registers: every thread gets the state behind `choice` and
// nothing is stored.  The caller keeps a barrier between the return and the block's next call (every pick holds several).
__device__ __forceinline__ int aut_next(const dh_automaton_args& aut, const aut_edges& ae, int q, int choice) {
    __shared__ int s_next;
    const int tid = threadIdx.x;
    if (tid == 0) s_next = q;
    __syncthreads();
    for (int e = ae.lo + tid; e < ae.hi; e += NT) {
        if (ae.tok[e] == choice) {
            const int d = aut.edge_dst[e];
            if (d >= 0 && d < aut.n_states) s_next = d;
        }
    }
    __syncthreads();
    return s_next;
}

// pick_token under no_repeat_ngram: under the row ban_row builds from the sequence's history g[0..m), through the masked paths of
// pick_token (the 16-byte mask_byte loads included), so the pick is the unmasked pick on a copy of the row with -inf in every column that
// the mask disallows or the history bans.  The kernels' BAN = false instantiations call pick_token<MASK> as they always did.
// pen, bias (launch-uniform; ngram may be 0 then): the columns of the history's ids hold a_t, and those of the ids the bias proposes their
// boosted value, as well, through pick_token's PEN paths.  Both off, the pick runs the instantiation it always ran.
// ae (launch-uniform): ban_row's start row is the automaton state's allowed row; everything behind it is unchanged.
template <bool MASK>
__device__ __forceinline__ int pick_token_banned(const bf16_t* __restrict__ lg, int vocab, float temperature, int top_k, uint64_t seed,
                                             int step, int seq, const uint32_t* __restrict__ mrow, const int64_t* g, int m, int ngram,
                                             const dh_nucleus_args nuc = dh_nucleus_args{}, const dh_penalty_args pen = DH_PENALTY_OFF,
                                             const dh_bias_args bias = dh_bias_args{}, const aut_edges ae = aut_edges{}) {
    const uint32_t* row = ban_row<MASK>(g, m, ngram, vocab, mrow, 1, ae);
    if (dh_penalty_on(pen) || bias.n > 0) {             // the same for every thread of the launch
        const pen_view ov = pen_build(lg, vocab, g, m, pen, bias);
        return pick_token<true, true>(lg, vocab, temperature, top_k, seed, step, seq, row, nuc, ov);
    }
    return pick_token<true>(lg, vocab, temperature, top_k, seed, step, seq, row, nuc);
}

// log softmax(lg)[token] of the RAW row (temperature 1, no crop: the model's distribution, not the sampler's) by the whole block;
// every thread returns it.  lp = lg[token] - m - log(sum_i exp(lg[i] - m)), m = max_i lg[i]: bf16 widened to fp32, fp32 sum, expf / logf
// (the fast intrinsics lose the last bits of large arguments).  -inf entries add 0; a -inf token gives -inf.
// The summation order is a function of vocab alone: thread t adds the 8-element chunks t, t + NT, t + 2 NT, .. in index order into one
// chain, a wave adds its 64 chains by the xor butterfly, the 16 wave sums are added by a butterfly too.  (The 16 wave maxima before
// it are read one after the other by every thread: a maximum is exact in any order.)  The 16-byte loads (vocab % 8 == 0
// and an aligned row, as in pick_token) and the scalar loop visit the same elements in the same order, so a row's bits do not depend
// on where it lies, and never on the row index or the row count.
// row_logsum: m and tot = the sum, by the whole block, every thread gets both; logprob_at: the last step; token_logprob: the two.
__device__ __forceinline__ void row_logsum(const bf16_t* __restrict__ lg, int vocab, float& m_out, float& tot_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float s_lp[NT / 64];
    const bool vec = (vocab & 7) == 0 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0;
    const uint4* lg4 = reinterpret_cast<const uint4*>(lg);
    const int n4 = (vocab + 7) >> 3;
    // ---- m = max_i lg[i] (exact in any order)
    float mx = -INFINITY;
    if (vec) {
        for (int c0 = tid; c0 < n4; c0 += 4 * NT) {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = c0 + u * NT < n4 ? lg4[c0 + u * NT] : uint4{0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u, 0xFF80FF80u};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bf16_t* e8 = reinterpret_cast<const bf16_t*>(&q[u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) mx = fmaxf(mx, bf2f(e8[e]));
            }
        }
    } else {
        for (int i = tid; i < vocab; i += NT) mx = fmaxf(mx, bf2f(lg[i]));
    }
    mx = wave_max(mx);
    if (lane == 0) s_lp[wave] = mx;
    __syncthreads();
    mx = s_lp[0];
    for (int w = 1; w < NT / 64; ++w) mx = fmaxf(mx, s_lp[w]);
    __syncthreads();
    // ---- sum_i exp(lg[i] - m): one chain per thread over its chunks, in index order
    auto term = [&](bf16_t b) -> float {
        const float v = bf2f(b);
        return v == -INFINITY ? 0.f : expf(v - mx);
    };
    float sum = 0.f;
    if (vec) {
        for (int c0 = tid; c0 < n4; c0 += 4 * NT) {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = c0 + u * NT < n4 ? lg4[c0 + u * NT] : uint4{0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u * NT >= n4) break;
                const bf16_t* e8 = reinterpret_cast<const bf16_t*>(&q[u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += term(e8[e]);
            }
        }
    } else {
        for (int c = tid; c < n4; c += NT) {
            const int hi = min(vocab, c * 8 + 8);
            for (int i = c * 8; i < hi; ++i) sum += term(lg[i]);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_lp[wave] = sum;
    __syncthreads();
    float tot = s_lp[lane & (NT / 64 - 1)];
#pragma unroll
    for (int o = NT / 128; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    __syncthreads();                       // s_lp is free for the next call
    m_out = mx;
    tot_out = tot;
}

// lp(token) from the row's m and tot: the one expression behind every log-probability this file writes
__device__ __forceinline__ float logprob_at(const bf16_t* __restrict__ lg, int token, float mx, float tot) {
    const float lt = bf2f(lg[token]);
    if (lt == -INFINITY) return -INFINITY;
    return (lt - mx) - logf(tot);
}

__device__ __forceinline__ float token_logprob(const bf16_t* __restrict__ lg, int vocab, int token) {
    float mx, tot;
    row_logsum(lg, vocab, mx, tot);
    return logprob_at(lg, token, mx, tot);
}

constexpr int MAX_TOP = 8;     // MAX_TOP_LOGPROBS of the header

// The k (1 .. min(MAX_TOP, vocab)) alternatives of one row, by the whole block: rank j is the entry at place j when the RAW row is
// ordered by value descending, then by index ascending (-0 == +0; -inf is an ordinary value that ranks last), and its value is
// logprob_at(lg, id_j, mx, tot) with the caller's m and tot, so it is bit-equal to token_logprob(lg, vocab, id_j).  Every thread gets
// pointers to the k ids and values in LDS, valid until the block's next call.
// One pass over the row: an entry's sort key is (bf16_key << 32) | ~index, unique per entry, so the order of a set of entries does
// not depend on the order they were visited in (the 16-byte loads and the scalar loop agree) and no atomic decides anything.  Every
// thread keeps the MAX_TOP largest keys of its own entries, sorted, in registers (0 = none: every real key is above it); k rounds of
// a block-wide maximum over the 1024 list heads, the winner's thread popping its head, merge them.  A NaN is just a key here: ids stay
// inside [0, vocab) as long as k <= vocab.
// MASK (the beam candidates under a token mask): the order is taken over the allowed entries only — the first k allowed ids in the
// raw row's order — and the values are still logprob_at under the raw row's m and tot.  Fewer than k allowed entries leave id 0 in
// the places behind them (the host refuses such a mask).
template <bool MASK>
__device__ __forceinline__ void row_top(const bf16_t* __restrict__ lg, int vocab, int k, float mx, float tot,
                                        const int32_t*& ids_out, const float*& lp_out, const uint32_t* __restrict__ mrow) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ uint64_t s_head[2][NT / 64];
    __shared__ uint64_t s_win[MAX_TOP];
    __shared__ int32_t s_tid[MAX_TOP];
    __shared__ float s_tlp[MAX_TOP];
    uint64_t c[MAX_TOP];
#pragma unroll
    for (int j = 0; j < MAX_TOP; ++j) c[j] = 0;
    auto offer = [&](bf16_t b, int i) {
        uint64_t key = ((uint64_t)bf16_key(b) << 32) | (uint32_t)~(uint32_t)i;
        if (key > c[MAX_TOP - 1]) {
#pragma unroll
            for (int j = 0; j < MAX_TOP; ++j) {                // c stays sorted: the smaller of each pair moves on
                const uint64_t hi = key > c[j] ? key : c[j];
                key = key > c[j] ? c[j] : key;
                c[j] = hi;
            }
        }
    };
    if ((vocab & 7) == 0 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0) {
        const uint4* lg4 = reinterpret_cast<const uint4*>(lg);
        const int n4 = vocab >> 3;
        for (int c0 = tid; c0 < n4; c0 += 4 * NT) {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = c0 + u * NT < n4 ? lg4[c0 + u * NT] : uint4{0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u * NT >= n4) break;
                const bf16_t* e8 = reinterpret_cast<const bf16_t*>(&q[u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if constexpr (MASK) { if (!((mask_byte(mrow, c0 + u * NT) >> e) & 1u)) continue; }
                    offer(e8[e], (c0 + u * NT) * 8 + e);
                }
            }
        }
    } else {
        for (int i = tid; i < vocab; i += NT) {
            if constexpr (MASK) { if (!mask_allows(mrow, i)) continue; }
            offer(lg[i], i);
        }
    }
    for (int r = 0; r < k; ++r) {
        uint64_t best = c[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t ov = __shfl_xor(best, o, 64);
            best = ov > best ? ov : best;
        }
        if (lane == 0) s_head[r & 1][wave] = best;
        __syncthreads();                   // two buffers: round r + 2 writes this one after every thread has passed round r + 1's barrier
        best = s_head[r & 1][0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) best = s_head[r & 1][w] > best ? s_head[r & 1][w] : best;
        if (c[0] == best) {                // keys are unique: one thread (best > 0 while r < vocab)
#pragma unroll
            for (int j = 0; j + 1 < MAX_TOP; ++j) c[j] = c[j + 1];
            c[MAX_TOP - 1] = 0;
        }
        if (tid == 0) s_win[r] = best;
    }
    __syncthreads();
    if (tid < k) {
        const uint32_t i = ~(uint32_t)s_win[tid];
        const int id = i < (uint32_t)vocab ? (int)i : 0;        // k > vocab is refused by the host; never an index outside the row
        s_tid[tid] = id;
        s_tlp[tid] = logprob_at(lg, id, mx, tot);
    }
    __syncthreads();
    ids_out = s_tid;
    lp_out = s_tlp;
}

// What a sampling kernel writes beside a token: LP its log-probability; TOP (with LP) the row's top_n alternatives as well, m and tot
// computed once for both.  Every thread returns lp and, with TOP, the LDS pointers of row_top.
template <bool LP, bool TOP>
__device__ __forceinline__ float row_report(const bf16_t* __restrict__ lg, int vocab, int choice, int top_n,
                                            const int32_t*& ti, const float*& tl) {
    if constexpr (TOP) {
        float mx, tot;
        row_logsum(lg, vocab, mx, tot);
        row_top<false>(lg, vocab, top_n, mx, tot, ti, tl, nullptr);     // the reported alternatives are the raw row's, mask or not
        return logprob_at(lg, choice, mx, tot);
    } else if constexpr (LP) {
        return token_logprob(lg, vocab, choice);
    }
    return 0.f;
}

// top_ids / top_lp ([n_seq, tok_ld, top_n]) at token place `at` = u * tok_ld + n, by the thread that stores the token
__device__ __forceinline__ void store_top(int32_t* __restrict__ top_ids, float* __restrict__ top_lp, size_t at, int top_n,
                                          const int32_t* ti, const float* tl) {
    for (int j = 0; j < top_n; ++j) {
        top_ids[at * top_n + j] = ti[j];
        top_lp[at * top_n + j] = tl[j];
    }
}

// stop_hit (common.h) for a pick stored at place n of the sequence's token row `row` whose prompt is p0 tokens long: the window comes from the
// places before n, which earlier launches wrote
__device__ __forceinline__ bool stop_hit_at(const dh_stop_args& sa, const int64_t* row, int n, int p0, int choice) {
    int w[DH_MAX_STOP_LEN];
    w[0] = choice;
#pragma unroll
    for (int k = 1; k < DH_MAX_STOP_LEN; ++k) w[k] = sa.n_seqs && n - k >= p0 && n - k >= 0 ? (int)row[n - k] : -1;
    return stop_hit(sa, w, n + 1 - p0);
}

template <bool LP, bool TOP = false, bool MASK = false, bool BAN = false>
__global__ __launch_bounds__(NT) void sample_kernel(const bf16_t* __restrict__ logits, int vocab,
                                                    int64_t* __restrict__ tokens, int tok_ld,
                                                    int32_t* __restrict__ length, int32_t* __restrict__ done,
                                                    float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                                    int step_arg, const int32_t* __restrict__ step_dev,
                                                    float* __restrict__ logprobs, int top_n,
                                                    int32_t* __restrict__ top_ids, float* __restrict__ top_lp,
                                                    const uint32_t* __restrict__ mask, int mask_ld, int ngram,
                                                    const int32_t* __restrict__ start, dh_stop_args sa, dh_nucleus_args nuc,
                                                    dh_penalty_args pen, dh_bias_args bias, dh_automaton_args aut) {
    const int seq = blockIdx.x, tid = threadIdx.x;
    if (done[seq]) return;
    const int step = step_dev ? *step_dev : step_arg;   // device counter keeps a captured graph replayable
    int choice;
    if constexpr (BAN) {                                // the history is what lies behind the prompt
        const int p0 = start[seq], m = length[seq] - p0;
        int q = 0;
        aut_edges ae;
        if (aut.on()) ae = aut_state(aut, seq, m, eos_id, q);          // the same for every thread of the launch
        choice = pick_token_banned<MASK>(logits + (size_t)seq * vocab, vocab, temperature, top_k, seed, step, seq,
                                     MASK ? mask + (size_t)seq * mask_ld : nullptr, tokens + (size_t)seq * tok_ld + p0, m, ngram, nuc, pen, bias, ae);
        if (aut.on()) aut_step(aut, ae, q, choice, seq);
    } else {
        choice = pick_token<MASK>(logits + (size_t)seq * vocab, vocab, temperature, top_k, seed, step, seq,
                                  MASK ? mask + (size_t)seq * mask_ld : nullptr, nuc);
    }
    const int32_t* ti = nullptr;
    const float* tl = nullptr;
    const float lp = row_report<LP, TOP>(logits + (size_t)seq * vocab, vocab, choice, top_n, ti, tl);
    if (tid == 0) {
        const int n = length[seq];
        if (n < tok_ld) {
            tokens[(size_t)seq * tok_ld + n] = choice;
            if constexpr (LP) logprobs[(size_t)seq * tok_ld + n] = lp;
            if constexpr (TOP) store_top(top_ids, top_lp, (size_t)seq * tok_ld + n, top_n, ti, tl);
            length[seq] = n + 1;
        }
        if (eos_id >= 0 && choice == eos_id) done[seq] = DH_DONE_EOS;
        else if (sa.on() && n < tok_ld && stop_hit_at(sa, tokens + (size_t)seq * tok_ld, n, sa.n_seqs ? start[seq] : 0, choice))
            done[seq] = DH_DONE_STOP;              // uniform per launch: off, the tail it always was
        else if (n + 1 >= tok_ld) done[seq] = DH_DONE_LENGTH;   // buffer full
    }
}

// sample_kernel over a row list (continuous batching): logits row r belongs to sequence u = row_seq[r] of a token buffer that
// holds every sequence of the call.  The draw is keyed by (seed, tokens generated so far for u, u) — what sample_kernel's
// (seed, step, row) is when all sequences start together — so a sequence's ids do not depend on when or where it was scheduled.
// limit[u] = prompt length + max_new is the sequence's own budget (done = 2 when reached).  Several padding rows may name one
// finished sequence: they return at once.
template <bool LP, bool TOP = false, bool MASK = false, bool BAN = false>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const bf16_t* __restrict__ logits, int vocab,
                                                         int64_t* __restrict__ tokens, int tok_ld,
                                                         int32_t* __restrict__ length, int32_t* __restrict__ done,
                                                         const int32_t* __restrict__ limit,
                                                         const int32_t* __restrict__ row_seq, int n_seq, int max_new,
                                                         float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                                         float* __restrict__ logprobs, int top_n,
                                                         int32_t* __restrict__ top_ids, float* __restrict__ top_lp,
                                                         const uint32_t* __restrict__ mask, int mask_ld, int ngram,
                                                         const int32_t* __restrict__ start, dh_stop_args sa, dh_nucleus_args nuc,
                                                    dh_penalty_args pen, dh_bias_args bias, dh_automaton_args aut) {
    const int u = row_seq[blockIdx.x], tid = threadIdx.x;
    if (u < 0 || u >= n_seq || done[u]) return;
    const int n = length[u], lim = min(limit[u], tok_ld);
    const int step = n - (limit[u] - max_new);          // tokens generated so far
    int choice;
    if constexpr (BAN) {
        const int p0 = start ? start[u] : limit[u] - max_new;           // the prompt length, which limit[u] - max_new is
        int q = 0;
        aut_edges ae;
        if (aut.on()) ae = aut_state(aut, u, n - p0, eos_id, q);       // the sequence's state, not the logits row's
        choice = pick_token_banned<MASK>(logits + (size_t)blockIdx.x * vocab, vocab, temperature, top_k, seed, step, u,
                                     MASK ? mask + (size_t)u * mask_ld : nullptr, tokens + (size_t)u * tok_ld + p0, n - p0, ngram, nuc, pen, bias, ae);
        if (aut.on()) aut_step(aut, ae, q, choice, u);
    } else {
        choice = pick_token<MASK>(logits + (size_t)blockIdx.x * vocab, vocab, temperature, top_k, seed, step, u,
                                  MASK ? mask + (size_t)u * mask_ld : nullptr, nuc);     // the sequence's mask row, not the logits row's
    }
    const int32_t* ti = nullptr;
    const float* tl = nullptr;
    const float lp = row_report<LP, TOP>(logits + (size_t)blockIdx.x * vocab, vocab, choice, top_n, ti, tl);
    if (tid == 0) {
        if (n < lim) {
            tokens[(size_t)u * tok_ld + n] = choice;
            if constexpr (LP) logprobs[(size_t)u * tok_ld + n] = lp;
            if constexpr (TOP) store_top(top_ids, top_lp, (size_t)u * tok_ld + n, top_n, ti, tl);
            length[u] = n + 1;
        }
        if (eos_id >= 0 && choice == eos_id) done[u] = DH_DONE_EOS;
        else if (sa.on() && n < lim && stop_hit_at(sa, tokens + (size_t)u * tok_ld, n, start ? start[u] : limit[u] - max_new, choice))
            done[u] = DH_DONE_STOP;
        else if (n + 1 >= lim) done[u] = DH_DONE_LENGTH;        // budget spent
    }
}

// The tail of a verify step (dh_engine_decode_spec): logits rows u * S + j, j = 0 .. S-1, are those of sequence u's last token and of
// the D = S - 1 drafted tokens behind it (row_ids[u * S + j], j >= 1).  pick_j is the arg-max of row j by pick_token's lowest-index
// rule; it is the sequence's next token as long as every draft before it was right, i.e. row_ids[u * S + i] == pick_{i-1} for
// i = 1 .. j.  The picks are appended one by one exactly as sample_kernel appends its one: nothing behind an EOS (done = 1) or
// behind the sequence's budget limit[u] = prompt length + max_new (done = 2), and a finished sequence is left alone.
// counters: [0] the last step (1-based, *step_dev) at which a sequence was live, [1] drafts verified, [2] drafts appended.
// LP: the log-probability of an appended pick_j, from its own row u * S + j, goes to logprobs beside the token; TOP: that row's
// alternatives too.  MASK: all S positions of sequence u are picked under mask row u.  BAN: position j's history runs up to the picks
// appended at the positions before it in this launch — thread 0's stores, which the barrier at the top of the loop orders before the
// block reads them back (a workgroup-scope fence: the block's waves share the CU's vector cache).
// sa (stop conditions): an appended pick that stops ends the loop with done = 3 exactly where an EOS ends it with 1; every thread decides
// it from its own copy of the window of the last DH_MAX_STOP_LEN generated tokens, never from thread 0's stores of this launch.
// DRAW ("Sampled verification" of the header, dh_engine_decode_spec_draw): pick_j is not the arg-max but the pick of the plain sampled
// step for the token at place n — top_k and the draw keyed by (seed, n - prompt length, u), prompt length = limit[u] - max_new as in
// sample_rows_kernel, under nuc and, with BAN, under pen, bias and aut on the history tokens[u, p0 .. n), this launch's picks included.
// The automaton's state is read once (aut_state), lives in registers and moves along every pick's edge (aut_next); thread 0 stores the
// state behind the last pick.  Everything behind the pick — acceptance, append order, stop window, EOS, budget, counters — is shared.
// DRAW is a template flag and not a launch-uniform argument like nuc and pen in the samplers: a runtime top_k would put the whole
// sampled branch, its 2 KiB of nucleus bins and the five options' arguments into the arg-max instantiations, whose code is pinned to
// what it was (MEASUREMENTS.md, "sampled verification").  Off: draw, nuc, pen, bias and aut are not read.
template <bool LP, bool TOP, bool MASK, bool BAN, bool DRAW>
__device__ __forceinline__ void spec_accept_body(const bf16_t* __restrict__ logits, int vocab, const int64_t* __restrict__ row_ids,
                                                         int S, int64_t* __restrict__ tokens, int tok_ld, int32_t* __restrict__ length,
                                                         int32_t* __restrict__ done, const int32_t* __restrict__ limit,
                                                         float temperature, int64_t eos_id, const int32_t* __restrict__ step_dev,
                                                         int32_t* __restrict__ counters, float* __restrict__ logprobs, int top_n,
                                                         int32_t* __restrict__ top_ids, float* __restrict__ top_lp,
                                                         const uint32_t* __restrict__ mask, int mask_ld, int ngram,
                                                         const int32_t* __restrict__ start, const dh_stop_args& sa,
                                                         const dh_spec_draw& draw, const dh_nucleus_args& nuc, const dh_penalty_args& pen,
                                                         const dh_bias_args& bias, const dh_automaton_args& aut) {
    const int u = blockIdx.x, tid = threadIdx.x;
    if (done[u]) return;
    int n = length[u];
    const int lim = min(limit[u], tok_ld);
    int p0 = 0;
    if constexpr (BAN) p0 = start[u];
    else if (sa.n_seqs) p0 = start[u];
    // the stop window, in every thread's registers: w[k] = the generated token k places before the coming pick, from places that
    // earlier launches wrote; every pick shifts it, so the decision below is the same for every thread without a read-back
    int w[DH_MAX_STOP_LEN];
#pragma unroll
    for (int k = 1; k < DH_MAX_STOP_LEN; ++k) w[k] = sa.n_seqs && n - k >= p0 && n - k >= 0 ? (int)tokens[(size_t)u * tok_ld + n - k] : -1;
    int appended = 0, state = 0, prev = 0;
    int q = 0, plen = 0;                                                  // DRAW: the automaton's state, the prompt length of the draw's key
    aut_edges ae;
    if constexpr (DRAW) {
        plen = limit[u] - draw.max_new;
        if constexpr (BAN) { if (aut.on()) ae = aut_state(aut, u, n - p0, eos_id, q); }     // the same for every thread of the launch
    }
    for (int j = 0; j < S; ++j) {
        if (j > 0) {
            if (row_ids[(size_t)u * S + j] != (int64_t)prev) break;      // the same for every thread
            __syncthreads();                                             // pick_token's shared scratch is free again
        }
        int choice;
        if constexpr (DRAW) {
            if constexpr (BAN) {
                choice = pick_token_banned<MASK>(logits + ((size_t)u * S + j) * vocab, vocab, temperature, draw.top_k, draw.seed, n - plen, u,
                                             MASK ? mask + (size_t)u * mask_ld : nullptr, tokens + (size_t)u * tok_ld + p0, n - p0, ngram, nuc,
                                             pen, bias, ae);
                if (aut.on()) {
                    q = aut_next(aut, ae, q, choice);
                    ae = aut_range(aut, q, eos_id);
                }
            } else {
                choice = pick_token<MASK>(logits + ((size_t)u * S + j) * vocab, vocab, temperature, draw.top_k, draw.seed, n - plen, u,
                                          MASK ? mask + (size_t)u * mask_ld : nullptr, nuc);
            }
        } else if constexpr (BAN)
            choice = pick_token_banned<MASK>(logits + ((size_t)u * S + j) * vocab, vocab, temperature, 1, 0, 0, u,
                                         MASK ? mask + (size_t)u * mask_ld : nullptr, tokens + (size_t)u * tok_ld + p0, n - p0, ngram);
        else
            choice = pick_token<MASK>(logits + ((size_t)u * S + j) * vocab, vocab, temperature, 1, 0, 0, u,
                                      MASK ? mask + (size_t)u * mask_ld : nullptr);
        prev = choice;
        if (n < lim) {                                                    // the same for every thread
            if constexpr (LP) {
                const int32_t* ti = nullptr;
                const float* tl = nullptr;
                const float lp = row_report<LP, TOP>(logits + ((size_t)u * S + j) * vocab, vocab, choice, top_n, ti, tl);
                if (tid == 0) logprobs[(size_t)u * tok_ld + n] = lp;
                if constexpr (TOP) if (tid == 0) store_top(top_ids, top_lp, (size_t)u * tok_ld + n, top_n, ti, tl);
            }
            if (tid == 0) tokens[(size_t)u * tok_ld + n] = choice;
            ++n;
            ++appended;
            if (sa.on() && !(eos_id >= 0 && choice == eos_id)) {          // the same for every thread
                w[0] = choice;
                if (stop_hit(sa, w, n - p0)) { state = DH_DONE_STOP; break; }
#pragma unroll
                for (int k = DH_MAX_STOP_LEN - 1; k > 0; --k) w[k] = w[k - 1];
            }
        }
        if (eos_id >= 0 && choice == eos_id) { state = DH_DONE_EOS; break; }
        if (n >= lim) { state = DH_DONE_LENGTH; break; }                  // budget spent
    }
    if (tid == 0) {
        length[u] = n;
        if (state) done[u] = state;
        if constexpr (DRAW && BAN) { if (aut.on()) aut.state[u] = q; }   // a plain vector store, as aut_step's
        atomicMax(&counters[0], *step_dev);
        atomicAdd(&counters[1], S - 1);
        atomicAdd(&counters[2], appended > 1 ? appended - 1 : 0);
    }
}

template <bool LP, bool TOP = false, bool MASK = false, bool BAN = false>
__global__ __launch_bounds__(NT) void spec_accept_kernel(const bf16_t* __restrict__ logits, int vocab, const int64_t* __restrict__ row_ids,
                                                         int S, int64_t* __restrict__ tokens, int tok_ld, int32_t* __restrict__ length,
                                                         int32_t* __restrict__ done, const int32_t* __restrict__ limit,
                                                         float temperature, int64_t eos_id, const int32_t* __restrict__ step_dev,
                                                         int32_t* __restrict__ counters, float* __restrict__ logprobs, int top_n,
                                                         int32_t* __restrict__ top_ids, float* __restrict__ top_lp,
                                                         const uint32_t* __restrict__ mask, int mask_ld, int ngram,
                                                         const int32_t* __restrict__ start, dh_stop_args sa) {
    spec_accept_body<LP, TOP, MASK, BAN, false>(logits, vocab, row_ids, S, tokens, tok_ld, length, done, limit, temperature, eos_id, step_dev,
                                                counters, logprobs, top_n, top_ids, top_lp, mask, mask_ld, ngram, start, sa, dh_spec_draw{},
                                                dh_nucleus_args{}, DH_PENALTY_OFF, dh_bias_args{}, dh_automaton_args{});
}

template <bool LP, bool TOP = false, bool MASK = false, bool BAN = false>
__global__ __launch_bounds__(NT) void spec_accept_draw_kernel(const bf16_t* __restrict__ logits, int vocab, const int64_t* __restrict__ row_ids,
                                                              int S, int64_t* __restrict__ tokens, int tok_ld, int32_t* __restrict__ length,
                                                              int32_t* __restrict__ done, const int32_t* __restrict__ limit,
                                                              float temperature, int64_t eos_id, const int32_t* __restrict__ step_dev,
                                                              int32_t* __restrict__ counters, float* __restrict__ logprobs, int top_n,
                                                              int32_t* __restrict__ top_ids, float* __restrict__ top_lp,
                                                              const uint32_t* __restrict__ mask, int mask_ld, int ngram,
                                                              const int32_t* __restrict__ start, dh_stop_args sa, dh_spec_draw draw,
                                                              dh_nucleus_args nuc, dh_penalty_args pen, dh_bias_args bias, dh_automaton_args aut) {
    spec_accept_body<LP, TOP, MASK, BAN, true>(logits, vocab, row_ids, S, tokens, tok_ld, length, done, limit, temperature, eos_id, step_dev,
                                               counters, logprobs, top_n, top_ids, top_lp, mask, mask_ld, ngram, start, sa, draw, nuc, pen, bias,
                                               aut);
}

// out[r] = log softmax(logits[r, :])[ids[r]]; an id outside [0, vocab) reads nothing and gives NaN (the Python wrapper refuses it)
__global__ __launch_bounds__(NT) void token_logprobs_kernel(const bf16_t* __restrict__ logits, int vocab, const int64_t* __restrict__ ids,
                                                            float* __restrict__ out) {
    const int r = blockIdx.x;
    const int64_t t = ids[r];
    if (t < 0 || t >= vocab) {                                             // the same for every thread
        if (threadIdx.x == 0) out[r] = __builtin_nanf("");
        return;
    }
    const float lp = token_logprob(logits + (size_t)r * vocab, vocab, (int)t);
    if (threadIdx.x == 0) out[r] = lp;
}

// out_ids / out_lp[r, 0..k) = the k alternatives of logits row r; MASK: the first k among the ids that mask row r / rows_per_mask
// allows, with the raw row's values
template <bool MASK>
__global__ __launch_bounds__(NT) void token_top_logprobs_kernel(const bf16_t* __restrict__ logits, int vocab, int k,
                                                                int32_t* __restrict__ out_ids, float* __restrict__ out_lp,
                                                                const uint32_t* __restrict__ mask, int mask_ld, int rows_per_mask) {
    const int r = blockIdx.x;
    const bf16_t* lg = logits + (size_t)r * vocab;
    const int32_t* ti = nullptr;
    const float* tl = nullptr;
    float mx, tot;
    row_logsum(lg, vocab, mx, tot);
    row_top<MASK>(lg, vocab, k, mx, tot, ti, tl, MASK ? mask + (size_t)(r / rows_per_mask) * mask_ld : nullptr);
    if (threadIdx.x == 0) store_top(out_ids, out_lp, (size_t)r, k, ti, tl);
}

// The candidates of a beam step under no_repeat_ngram (include/dualhyp_hip.h, "Beam histories"): row r = u * rows_per_utt + b of the
// launch is live beam b of utterance u, its history the m = n_steps[u] tokens of row u * W + b of plane (m - 1) & 1 of `hist`
// ([2][n_utt * W][max_new]) — the plane the step before wrote; this launch writes none.  The k = 2 W candidates are
// token_top_logprobs_kernel<true>'s under the LDS row of ban_row: the mask row (MASK) or all ones, minus the banned ids, and the start
// row again where fewer than k ids are left.  A done utterance's rows return at once: nothing reads their candidates.
template <bool MASK>
__global__ __launch_bounds__(NT) void beam_top_hist_kernel(const bf16_t* __restrict__ logits, int vocab, int k,
                                                           int32_t* __restrict__ out_ids, float* __restrict__ out_lp,
                                                           const uint32_t* __restrict__ mask, int mask_ld, int rows_per_utt, int W,
                                                           int max_new, const int64_t* __restrict__ hist, int ngram,
                                                           const int32_t* __restrict__ n_steps, const int32_t* __restrict__ done) {
    const int r = blockIdx.x, u = r / rows_per_utt, b = r % rows_per_utt;
    if (done[u]) return;                                                    // the same for every thread
    int m = n_steps[u];
    m = m < 0 ? 0 : (m > max_new ? max_new : m);                            // never a read outside the row
    const size_t plane = (size_t)(gridDim.x / rows_per_utt) * W * max_new;
    const int64_t* g = hist + (size_t)((m - 1) & 1) * plane + ((size_t)u * W + b) * max_new;
    const bf16_t* lg = logits + (size_t)r * vocab;
    const uint32_t* row = ban_row<MASK, true>(g, m, ngram, vocab, MASK ? mask + (size_t)u * mask_ld : nullptr, k);
    const int32_t* ti = nullptr;
    const float* tl = nullptr;
    float mx, tot;
    row_logsum(lg, vocab, mx, tot);
    row_top<true>(lg, vocab, k, mx, tot, ti, tl, row);
    if (threadIdx.x == 0) store_top(out_ids, out_lp, (size_t)r, k, ti, tl);
}

// the three kernels' variant for the options `c` (a dh_pick_ctl) has on: (logprobs, top_n), top_n > 0 needing the three buffers; the token
// mask, null being the kernel without it (the code it always was); and c.hist(), the history-reading family
#define DH_PICK_VARIANT_MB(kernel, c, M, B) \
    ((c).top_n > 0 ? kernel<true, true, M, B> : (c).logprobs ? kernel<true, false, M, B> : kernel<false, false, M, B>)
#define DH_PICK_VARIANT_B(kernel, c, B) ((c).mask ? DH_PICK_VARIANT_MB(kernel, c, true, B) : DH_PICK_VARIANT_MB(kernel, c, false, B))
#define DH_PICK_VARIANT(kernel, c) ((c).hist() ? DH_PICK_VARIANT_B(kernel, c, true) : DH_PICK_VARIANT_B(kernel, c, false))

int check_mask_ld(const char* name, int vocab, const uint32_t* mask, int mask_ld) {
    DH_CHECK(!mask || mask_ld >= (vocab + 31) / 32, "%s: mask_ld=%d is below the %d words of a %d-token mask row", name, mask_ld,
             (vocab + 31) / 32, vocab);
    return 0;
}

// What the three launchers check of a pick's options.  hist_max: the longest history a pick of the call can see; start_needed: the kernel
// has no other way to the prompt lengths (the row-list kernel has limit - max_new).  A bias itself is checked where it is packed
// (dh_bias_pack); here what depends on the call: with a penalty on, the history's ids and the entries' ids share the tables.
// eos_id, n_seq: the call's, for an automaton — its dead end picks the EOS, and init / state hold an entry per sequence.
int check_pick(const char* name, int vocab, int hist_max, bool start_needed, const dh_pick_ctl& c, int64_t eos_id = -1, int n_seq = 0) {
    const bool pen = dh_penalty_on(c.pen), bias = c.bias.n != 0, aut = c.aut.on();
    DH_CHECK(!aut || c.start, "%s: an automaton needs `start`, the prompt lengths: a sequence is in its start state while it has generated "
             "nothing", name);
    DH_CHECK(!aut || vocab <= BAN_MAX_VOCAB, "%s: an automaton's allowed row is a static LDS row of %d ids; vocab=%d does not fit", name,
             BAN_MAX_VOCAB, vocab);
    DH_CHECK(!aut || (eos_id >= 0 && eos_id < vocab), "%s: an automaton needs an eos_id in [0, %d), got %lld: a dead end ends the sequence "
             "with it", name, vocab, (long long)eos_id);
    DH_CHECK(!aut || c.aut.n_seq == n_seq, "%s: the automaton set holds start states for %d sequences, the call has %d", name, c.aut.n_seq,
             n_seq);
    DH_CHECK(!pen || c.start, "%s: penalties need `start`, the prompt lengths: the history is what lies behind the prompt", name);
    DH_CHECK(!pen || vocab <= BAN_MAX_VOCAB, "%s: penalties keep a sequence's overridden columns in a static LDS row of %d ids; vocab=%d "
             "does not fit", name, BAN_MAX_VOCAB, vocab);
    DH_CHECK(!pen || hist_max <= PEN_MAX_HISTORY, "%s: penalties keep a sequence's distinct ids in static LDS tables of %d entries; a "
             "history of up to %d tokens may not fit", name, PEN_MAX_HISTORY, hist_max);
    DH_CHECK(!bias || c.start, "%s: a bias needs `start`, the prompt lengths: a match never reaches into the prompt", name);
    DH_CHECK(!bias || vocab <= BAN_MAX_VOCAB, "%s: a bias keeps a sequence's overridden columns in a static LDS row of %d ids; vocab=%d does "
             "not fit", name, BAN_MAX_VOCAB, vocab);
    DH_CHECK(!bias || !pen || hist_max + c.bias.n_ids <= PEN_MAX_HISTORY, "%s: penalties and a bias keep a sequence's distinct ids in static "
             "LDS tables of %d entries; a history of up to %d tokens and the entries' %d ids may not fit", name, PEN_MAX_HISTORY, hist_max,
             c.bias.n_ids);
    DH_CHECK(c.stop.n_seqs == 0 || c.start || !start_needed, "%s: stop sequences need `start`, the prompt lengths", name);
    DH_CHECK(c.top_n >= 0 && c.top_n <= MAX_TOP && c.top_n <= vocab, "%s: top_logprobs must be 0 .. min(8, vocab)", name);
    DH_CHECK(c.top_n == 0 || (c.logprobs && c.top_ids && c.top_lp), "%s: top_logprobs needs the logprobs, top_ids and top_lp buffers", name);
    if (int rc = check_mask_ld(name, vocab, c.mask, c.mask_ld)) return rc;
    DH_CHECK(c.ngram >= 0 && c.ngram <= MAX_NGRAM, "%s: no_repeat_ngram=%d is not in 0 .. %d", name, c.ngram, MAX_NGRAM);
    DH_CHECK(c.ngram == 0 || vocab <= BAN_MAX_VOCAB, "%s: no_repeat_ngram keeps a sequence's allowed-minus-banned bits in a static LDS row of "
             "%d ids; vocab=%d does not fit", name, BAN_MAX_VOCAB, vocab);
    DH_CHECK(c.ngram == 0 || c.start || !start_needed, "%s: no_repeat_ngram needs `start`, the prompt lengths", name);
    return 0;
}

// An exported entry's options, as the ABI spells them, to the ctl of its launch, with the packers' checks under the entry's own name.
// The parameters behind `logprobs` are in the order the entries gained them, and an entry passes as many as it has: the rest are off.
// start_implied (the _rows entries): a null start is limit - max_new, which is enough for stop sequences.
int pack_pick(const char* name, bool start_implied, int vocab, dh_pick_ctl& c, float* logprobs, int top_n = 0, int32_t* top_ids = nullptr,
              float* top_lp = nullptr, const uint32_t* mask = nullptr, int mask_ld = 0, int ngram = 0, const int32_t* start = nullptr,
              const dh_stop_spec* stop = nullptr, float top_p = 1.f, float min_p = 0.f, const dh_penalty_args* penalties = nullptr,
              const dh_bias_spec* bias = nullptr, const dh_automaton_spec* automaton = nullptr) {
    if (int rc = dh_automaton_pack(name, automaton, vocab, start != nullptr, c.aut)) return rc;
    if (int rc = dh_bias_pack(name, bias, vocab, start != nullptr, c.bias)) return rc;
    if (int rc = dh_penalty_pack(name, penalties, c.pen)) return rc;
    if (int rc = dh_nucleus_pack(name, top_p, min_p, c.nuc)) return rc;
    if (int rc = dh_stop_pack(name, stop, start_implied || start != nullptr, c.stop)) return rc;
    c.logprobs = logprobs;
    c.top_n = top_n;
    c.top_ids = top_ids;
    c.top_lp = top_lp;
    c.mask = mask;
    c.mask_ld = mask ? mask_ld : 0;
    c.ngram = ngram;
    c.start = start;
    return 0;
}

}  // namespace

int dh_sample_impl(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, int n_seq,
                   float temperature, int top_k, int64_t eos_id, uint64_t seed, int step, const int32_t* step_dev,
                   const dh_pick_ctl& c, void* stream) {
    DH_CHECK(vocab > 0 && tok_ld > 0 && n_seq >= 0, "dh_sample_bf16: bad shape");
    if (int rc = check_pick("dh_sample_bf16", vocab, tok_ld, true, c, eos_id, n_seq)) return rc;
    DH_CHECK(temperature > 0.f, "dh_sample_bf16: temperature must be > 0");
    DH_CHECK(top_k >= 0, "dh_sample_bf16: top_k must be >= 0 (0 = no crop)");
    if (n_seq == 0) return 0;
    // logprobs null: the kernel without the log-probability pass (the code it always was)
    hipLaunchKernelGGL(DH_PICK_VARIANT(sample_kernel, c), dim3(n_seq), dim3(NT), dh_penalty_on(c.pen) || c.bias.n > 0 ? PEN_LDS_BYTES : 0,
                       (hipStream_t)stream,
                       logits, vocab, tokens, tok_ld, length, done, temperature, top_k, eos_id, seed, step, step_dev, c.logprobs, c.top_n,
                       c.top_ids, c.top_lp, c.mask, c.mask_ld, c.ngram, c.start, c.stop, c.nuc, c.pen, c.bias, c.aut);
    DH_LAUNCH_CHECK();
    return 0;
}

// The exported ladder: each entry takes the options of the one before and its own behind them, refuses what only it can refuse, and
// launches with the rest off.
extern "C" int dh_sample_bf16_ex(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                 int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                 int step, void* stream, float* logprobs) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_ex", false, vocab, c, logprobs)) return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_top(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                  int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                  int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_top", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp)) return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_mask(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                   int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                   int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                   const uint32_t* mask, int mask_ld) {
    DH_CHECK(mask, "dh_sample_bf16_mask: null mask (dh_sample_bf16_top is the entry without one)");
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_mask", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld)) return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_ngram(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                    int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                    int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                    const uint32_t* mask, int mask_ld, int ngram, const int32_t* start) {
    DH_CHECK(ngram >= 1, "dh_sample_bf16_ngram: ngram=%d (dh_sample_bf16_mask / dh_sample_bf16_top are the entries without one)", ngram);
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_ngram", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_stop(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                   int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                   int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                   const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_stop", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_nucleus(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                      int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                      int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                      const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                      float top_p, float min_p) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_nucleus", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop, top_p, min_p))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_penalty(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                      int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                      int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                      const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                      float top_p, float min_p, const dh_penalty_args* penalties) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_penalty", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop, top_p, min_p, penalties))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_bias(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                   int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                   int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                   const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                   float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_bias", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop, top_p, min_p, penalties, bias))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16_automaton(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                        int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                        int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                        const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                        float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias,
                                        const dh_automaton_spec* automaton) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_bf16_automaton", false, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop, top_p, min_p, penalties, bias, automaton))
        return rc;
    return dh_sample_impl(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, nullptr, c, stream);
}

extern "C" int dh_sample_bf16(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                              int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                              int step, void* stream) {
    return dh_sample_bf16_ex(logits, vocab, tokens, tok_ld, length, done, n_seq, temperature, top_k, eos_id, seed, step, stream,
                             nullptr);
}

int dh_sample_rows_impl(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                        const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq, int max_new, float temperature,
                        int top_k, int64_t eos_id, uint64_t seed, const dh_pick_ctl& c, void* stream) {
    DH_CHECK(logits && tokens && length && done && limit && row_seq, "dh_sample_rows_bf16: null argument");
    if (int rc = check_pick("dh_sample_rows_bf16", vocab, tok_ld, false, c, eos_id, n_seq)) return rc;
    DH_CHECK(vocab > 0 && tok_ld > 0 && n_rows >= 0 && n_seq > 0 && max_new > 0, "dh_sample_rows_bf16: bad shape");
    DH_CHECK(temperature > 0.f, "dh_sample_rows_bf16: temperature must be > 0");
    DH_CHECK(top_k >= 0, "dh_sample_rows_bf16: top_k must be >= 0 (0 = no crop)");
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(DH_PICK_VARIANT(sample_rows_kernel, c), dim3(n_rows), dim3(NT),
                       dh_penalty_on(c.pen) || c.bias.n > 0 ? PEN_LDS_BYTES : 0, (hipStream_t)stream, logits, vocab, tokens, tok_ld, length,
                       done, limit, row_seq, n_seq, max_new, temperature, top_k, eos_id, seed, c.logprobs, c.top_n, c.top_ids, c.top_lp, c.mask,
                       c.mask_ld, c.ngram, c.start, c.stop, c.nuc, c.pen, c.bias, c.aut);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_sample_rows_bf16_ex(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                      int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                      int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                      float* logprobs) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_ex", true, vocab, c, logprobs)) return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_top(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                       int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                       int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                       float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_top", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp)) return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_mask(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                        int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                        int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                        float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                        int mask_ld) {
    DH_CHECK(mask, "dh_sample_rows_bf16_mask: null mask (dh_sample_rows_bf16_top is the entry without one)");
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_mask", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld)) return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_ngram(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                         int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                         int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                         float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                         int mask_ld, int ngram, const int32_t* start) {
    DH_CHECK(ngram >= 1, "dh_sample_rows_bf16_ngram: ngram=%d (dh_sample_rows_bf16_mask / dh_sample_rows_bf16_top are the entries without one)",
             ngram);
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_ngram", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_stop(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                        int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                        int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                        float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                        int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_stop", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_nucleus(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                           int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                           int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                           float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                           int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop, float top_p,
                                           float min_p) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_nucleus", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram,
                           start, stop, top_p, min_p))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_penalty(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                           int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                           int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                           float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                           int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop, float top_p,
                                           float min_p, const dh_penalty_args* penalties) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_penalty", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram,
                           start, stop, top_p, min_p, penalties))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_bias(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                        int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                        int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                        float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                        int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop, float top_p,
                                        float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_bias", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram, start,
                           stop, top_p, min_p, penalties, bias))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16_automaton(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                             int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                             int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream,
                                             float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp, const uint32_t* mask,
                                             int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop, float top_p,
                                             float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias,
                                             const dh_automaton_spec* automaton) {
    dh_pick_ctl c;
    if (int rc = pack_pick("dh_sample_rows_bf16_automaton", true, vocab, c, logprobs, top_logprobs, top_ids, top_lp, mask, mask_ld, ngram,
                           start, stop, top_p, min_p, penalties, bias, automaton))
        return rc;
    return dh_sample_rows_impl(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new, temperature, top_k,
                               eos_id, seed, c, stream);
}

extern "C" int dh_sample_rows_bf16(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                   int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                   int max_new, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream) {
    return dh_sample_rows_bf16_ex(logits, vocab, tokens, tok_ld, length, done, limit, row_seq, n_rows, n_seq, max_new,
                                  temperature, top_k, eos_id, seed, stream, nullptr);
}

int dh_spec_accept_impl(const dh_bf16* logits, int vocab, const int64_t* row_ids, int S, int64_t* tokens, int tok_ld,
                        int32_t* length, int32_t* done, const int32_t* limit, int n_seq, float temperature, int64_t eos_id,
                        const int32_t* step_dev, int32_t* counters, const dh_pick_ctl& c, void* stream, const dh_spec_draw* draw) {
    // the arg-max kernel reads none of the four: only the draw mode forms a position's history, this launch's own picks included
    DH_CHECK(draw || (!c.nuc.on() && !dh_penalty_on(c.pen) && c.bias.n == 0 && !c.aut.on()),
             "spec_accept: an arg-max verify step takes no nucleus, no penalty, no bias and no automaton");
    DH_CHECK(logits && row_ids && tokens && length && done && limit && step_dev && counters, "spec_accept: null argument");
    if (int rc = check_pick("spec_accept", vocab, tok_ld, true, c, eos_id, n_seq)) return rc;
    DH_CHECK(vocab > 0 && tok_ld > 0 && n_seq >= 0 && S >= 2, "spec_accept: bad shape");
    DH_CHECK(temperature > 0.f, "spec_accept: temperature must be > 0");
    DH_CHECK(!draw || (draw->top_k >= 0 && draw->max_new > 0), "spec_accept: top_k must be >= 0 (0 = no crop) and max_new > 0");
    if (n_seq == 0) return 0;
    if (draw) {                                         // the penalties' dynamic LDS as the penalised sample_kernel launch asks for it
        hipLaunchKernelGGL(DH_PICK_VARIANT(spec_accept_draw_kernel, c), dim3(n_seq), dim3(NT),
                           dh_penalty_on(c.pen) || c.bias.n > 0 ? PEN_LDS_BYTES : 0, (hipStream_t)stream, logits, vocab, row_ids, S, tokens, tok_ld,
                           length, done, limit, temperature, eos_id, step_dev, counters, c.logprobs, c.top_n, c.top_ids, c.top_lp, c.mask,
                           c.mask_ld, c.ngram, c.start, c.stop, *draw, c.nuc, c.pen, c.bias, c.aut);
        DH_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(DH_PICK_VARIANT(spec_accept_kernel, c), dim3(n_seq), dim3(NT), 0,
                       (hipStream_t)stream, logits, vocab, row_ids, S, tokens, tok_ld, length, done, limit, temperature, eos_id, step_dev,
                       counters, c.logprobs, c.top_n, c.top_ids, c.top_lp, c.mask, c.mask_ld, c.ngram, c.start, c.stop);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_token_logprobs_bf16(const dh_bf16* logits, int vocab, const int64_t* ids, float* out, int n_rows, void* stream) {
    DH_CHECK(logits && ids && out, "dh_token_logprobs_bf16: null argument");
    DH_CHECK(vocab > 0 && n_rows >= 0, "dh_token_logprobs_bf16: bad shape");
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(token_logprobs_kernel, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, logits, vocab, ids, out);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_token_top_logprobs_bf16(const dh_bf16* logits, int vocab, int k, int32_t* out_ids, float* out_lp, int n_rows,
                                          void* stream) {
    DH_CHECK(logits && out_ids && out_lp, "dh_token_top_logprobs_bf16: null argument");
    DH_CHECK(vocab > 0 && n_rows >= 0, "dh_token_top_logprobs_bf16: bad shape");
    DH_CHECK(k >= 1 && k <= MAX_TOP && k <= vocab, "dh_token_top_logprobs_bf16: k must be 1 .. min(8, vocab)");
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(token_top_logprobs_kernel<false>, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, logits, vocab, k, out_ids, out_lp,
                       nullptr, 0, 1);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_token_top_logprobs_bf16_mask(const dh_bf16* logits, int vocab, int k, int32_t* out_ids, float* out_lp, int n_rows,
                                               const uint32_t* mask, int mask_ld, int rows_per_mask, void* stream) {
    DH_CHECK(logits && out_ids && out_lp, "dh_token_top_logprobs_bf16_mask: null argument");
    DH_CHECK(mask, "dh_token_top_logprobs_bf16_mask: null mask (dh_token_top_logprobs_bf16 is the entry without one)");
    DH_CHECK(vocab > 0 && n_rows >= 0 && rows_per_mask >= 1, "dh_token_top_logprobs_bf16_mask: bad shape");
    DH_CHECK(k >= 1 && k <= MAX_TOP && k <= vocab, "dh_token_top_logprobs_bf16_mask: k must be 1 .. min(8, vocab)");
    if (int rc = check_mask_ld("dh_token_top_logprobs_bf16_mask", vocab, mask, mask_ld)) return rc;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(token_top_logprobs_kernel<true>, dim3(n_rows), dim3(NT), 0, (hipStream_t)stream, logits, vocab, k, out_ids, out_lp,
                       mask, mask_ld, rows_per_mask);
    DH_LAUNCH_CHECK();
    return 0;
}

// the candidates of a beam step whose rows carry device histories and a ban (beam.hip, dh_beam_select_bf16_hist); the caller has
// checked the shapes, ngram in 1 .. 8 and vocab <= 131072
int dh_beam_top_hist_impl(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new, int32_t* out_ids,
                          float* out_lp, const uint32_t* mask, int mask_ld, const int64_t* hist, int ngram, const int32_t* n_steps,
                          const int32_t* done, void* stream) {
    DH_CHECK(ngram >= 1 && ngram <= MAX_NGRAM && vocab <= BAN_MAX_VOCAB && 2 * W <= MAX_TOP && hist, "dh_beam_select_bf16_hist: bad ban arguments");
    if (mask)
        hipLaunchKernelGGL(beam_top_hist_kernel<true>, dim3(n_utt * rows_per_utt), dim3(NT), 0, (hipStream_t)stream, logits, vocab, 2 * W,
                           out_ids, out_lp, mask, mask_ld, rows_per_utt, W, max_new, hist, ngram, n_steps, done);
    else
        hipLaunchKernelGGL(beam_top_hist_kernel<false>, dim3(n_utt * rows_per_utt), dim3(NT), 0, (hipStream_t)stream, logits, vocab, 2 * W,
                           out_ids, out_lp, nullptr, 0, rows_per_utt, W, max_new, hist, ngram, n_steps, done);
    DH_LAUNCH_CHECK();
    return 0;
}
