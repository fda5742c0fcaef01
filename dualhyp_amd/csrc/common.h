// Shared device/host helpers for libdualhyp_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include <utility>

#include "../../include/dualhyp_hip.h"

typedef uint16_t bf16_t;
typedef __attribute__((ext_vector_type(8))) short bf16x8;    // 8 bf16 = 4 VGPRs (MFMA A/B operand)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;   // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(4))) float f32x4;     // 16x16 MFMA accumulator

// ---- bf16 <-> f32 (round-to-nearest-even, NaN preserving: plain casts, MI355X_MICROARCH
// "Correctness boundaries") ---------------------------------------------------------------
__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {
    __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32 (RNE)
    return __builtin_bit_cast(bf16_t, b);
}
// round an fp32 value to the nearest bf16 and return it as fp32: one rounding point of the
// reference's eager bf16 tensor program
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }

// two values -> one dword of two bf16 (lo in bits 0..15): ONE v_cvt_pk_bf16_f32.  Written as two scalar conversions + shift + or
// the compiler only sometimes finds the packed form (the prefill attention loop had 32 single conversions, 16 shifts and 16
// ors per 32 probabilities); same rounding either way (RNE, the instruction's NaN handling).
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// ---- wave64 reductions ------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// silu(g) = g / (1 + e^-g) for every SwiGLU epilogue (prefill tiles of both sizes, the decode family, fp8, the training
// forward: one formula, so no row depends on which kernel finished it): hardware
// exp2 and reciprocal (about 1 ulp each; the argument product adds |g| * 1e-7 relative).  libm's expf and the IEEE
// division cost ~45 VALU instructions per element, 64 elements per lane: 5.8 us of a 60-us SwiGLU tile
// (tools/probe_gemm256.py).  The value is rounded to bf16 right after: a relative error of a few 1e-7 moves about one
// result in 10^4 by one bf16 ulp, as libm-vs-Sleef differences between the reference's CPU and GPU runs do.
__device__ __forceinline__ float silu_fast(float g) {
#ifdef DH_SILU_EXACT   // A/B builds only
    return g / (1.0f + expf(-g));
#else
    return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-g * 1.44269504088896341f));
#endif
}

// ---- async global -> LDS, 16 B per lane; LDS destination = wave-uniform base + lane*16 ----
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// The saddr form of the same request, written out: uniform base in an SGPR pair + one 32-bit byte offset per lane, LDS destination
// (uniform) through M0.  From the builtin the compiler hoists zero-extended lane offsets out of a loop as 64-bit VGPR pairs and
// issues a v_lshl_add_u64 plus the 64-bit-address form per request; the compiler does not count an asm load (wait with
// explicit s_waitcnt vmcnt) and never waits before a ds_read that may alias its destination.
__device__ __forceinline__ void glds16_saddr(const void* base_uniform, uint32_t lane_off, void* lds_wave_base) {
    const uint32_t lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds_wave_base;
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(lane_off), "s"(base_uniform), "s"(lds) : "memory", "m0");
}

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>) (#pragma unroll gives up on big bodies, and a
// loop that stays a loop indexes register arrays dynamically, i.e. puts them in scratch)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// the same with the non-temporal policy (aux = 2): bytes this CU alone reads once (streamed weights)
__device__ __forceinline__ void glds16_nt(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 2);
}

// ---- full-line loads -> MFMA fragments, in registers ------------------------------------------------------
// A 16-row x 128-B operand block fetched as two requests of full lines (request h: rows 8h..8h+7, lane -> row lane/8,
// 16-B piece lane%8 of the row's line) holds, for the 16x16 MFMA forms whose lane (row r = lane%16, kg = lane/16) wants
// 16-B piece 4t + kg of row r (bf16 x32: t = k-step 0/1 of the line), the 64 pieces of fragment t on the lanes with
// (lane & 4) == 4t of both requests.  One DPP move merges them (DPP bank masks cover lanes in fours), one ds_bpermute
// per dword puts them in fragment order: source lane 8 (r%8) + kg + 4 (r/8) for both fragments.
typedef __attribute__((ext_vector_type(4))) int i32x4;
__device__ __forceinline__ int frag_src_lane(int lane) { return ((lane & 7) << 3) + (lane >> 4) + (((lane >> 3) & 1) << 2); }
__device__ __forceinline__ void lines_to_frags(const i32x4& r0, const i32x4& r1, int fidx, bf16x8& f0, bf16x8& f1) {
    union { i32x4 i; bf16x8 b; } a, b;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int lo = __builtin_amdgcn_update_dpp(r0[d], r1[d], 0x114 /* row_shr:4 */, 0xF, 0xA /* lanes 4-7, 12-15 of a row */, false);
        const int hi = __builtin_amdgcn_update_dpp(r1[d], r0[d], 0x104 /* row_shl:4 */, 0xF, 0x5 /* lanes 0-3, 8-11 */, false);
        a.i[d] = __builtin_amdgcn_ds_bpermute(fidx, lo);
        b.i[d] = __builtin_amdgcn_ds_bpermute(fidx, hi);
    }
    f0 = a.b;
    f1 = b.b;
}

// The inverse, for 16x16 accumulator tiles on their way to memory: two C^T tiles of 16 columns (t = 0 / 1) x 16 rows, lane
// (row r = lane%16, kg = lane/16) holding columns 16t + 4kg..+4 of row r, become two requests of full 128-B lines (r0: rows
// 0..7, r1: rows 8..15; lane -> row lane/8, columns 4 (lane%8)..+4 of the 32).  Stores of 16 rows x 64 B per instruction
// pay per 64-B segment like fragment-shaped loads do.
__device__ __forceinline__ int line_src_lane(int lane) { return ((lane & 3) << 4) | (((lane >> 2) & 1) << 3) | (lane >> 3); }
__device__ __forceinline__ void tiles_to_lines(const f32x4& t0, const f32x4& t1, int lidx, f32x4& r0, f32x4& r1) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int m0 = __builtin_amdgcn_ds_bpermute(lidx, __float_as_int(t0[d]));
        const int m1 = __builtin_amdgcn_ds_bpermute(lidx, __float_as_int(t1[d]));
        r0[d] = __int_as_float(__builtin_amdgcn_update_dpp(m0, m1, 0x114 /* row_shr:4 */, 0xF, 0xA, false));
        r1[d] = __int_as_float(__builtin_amdgcn_update_dpp(m1, m0, 0x104 /* row_shl:4 */, 0xF, 0x5, false));
    }
}

// ---- KV cache in MFMA-fragment order --------------------------------------------------------
// Both caches are stored per (slot, group) as 32-key tiles of HS*32 elements, laid out so that a
// wave-wide contiguous 1-KiB load (lane i <- 16 B at i*16) IS an MFMA operand fragment:
//   K  tile: [ks = d/16][lh = (d/8)&1][lr = key&31][8 d]      A operand of S^T = K.Q^T  (k-step ks)
//   V^T tile: [dt = d/32][s2][lh][lr = d&31][8 keys]          A operand of O^T = V^T.P^T (k-step s2),
//             the 8 keys being 16*s2 + 8*(j>>2) + 4*lh + (j&3), j = 0..7 — the k-order in which the
//             S^T accumulator registers come out (cdna_hip_programming.md §3).
// Offsets below are in elements from the start of the (slot, group) block of s_max*HS elements.
template <int HS>
__device__ __forceinline__ size_t kfrag_off(int key, int d) {
    const int t = key >> 5, lr = key & 31, ks = d >> 4, lh = (d >> 3) & 1, e = d & 7;
    return ((size_t)((t * (HS / 16) + ks) * 2 + lh) * 32 + lr) * 8 + e;
}
template <int HS>
__device__ __forceinline__ size_t vfrag_off(int key, int d) {
    const int t = key >> 5, kk = key & 31, s2 = kk >> 4, r = kk & 15;
    const int j = ((r >> 3) << 2) | (r & 3), lh = (r >> 2) & 1, dt = d >> 5, lr = d & 31;
    return ((size_t)(((t * (HS / 32) + dt) * 2 + s2) * 2 + lh) * 32 + lr) * 8 + j;
}
// start (in elements) of the 1-KiB fragment block of tile t: K k-step ks / V^T (dt, s2); add lane*8
template <int HS> __device__ __forceinline__ size_t kfrag_blk(int t, int ks) { return (size_t)(t * (HS / 16) + ks) * 512; }
template <int HS> __device__ __forceinline__ size_t vfrag_blk(int t, int dt, int s2) { return (size_t)((t * (HS / 32) + dt) * 2 + s2) * 512; }

// ---- rope of one 16-B chunk pair (ger/model.py:349-355) -------------------------------------
// out = bf16( bf16(x*cos) + bf16(rot*sin) ), rot = [-x2, x1]: channels d0..d0+7 (o1) and HS/2 + d0..+7 (o2) of the head row `src`
// at position pos.  Phase 1 of both cache writers (elementwise.hip, kv8.hip); what becomes of o1 / o2 is theirs.
template <int HS>
__device__ __forceinline__ void rope_chunk_pair(const bf16_t* src, const bf16_t* cos, const bf16_t* sin, int pos, int d0, uint4& o1, uint4& o2) {
    constexpr int HALF = HS / 2;
    uint4 a = *reinterpret_cast<const uint4*>(src + d0);
    uint4 b = *reinterpret_cast<const uint4*>(src + HALF + d0);
    uint4 c1 = *reinterpret_cast<const uint4*>(cos + (size_t)pos * HS + d0);
    uint4 c2 = *reinterpret_cast<const uint4*>(cos + (size_t)pos * HS + HALF + d0);
    uint4 s1 = *reinterpret_cast<const uint4*>(sin + (size_t)pos * HS + d0);
    uint4 s2 = *reinterpret_cast<const uint4*>(sin + (size_t)pos * HS + HALF + d0);
    const bf16_t *ap = (const bf16_t*)&a, *bp = (const bf16_t*)&b, *c1p = (const bf16_t*)&c1,
                 *c2p = (const bf16_t*)&c2, *s1p = (const bf16_t*)&s1, *s2p = (const bf16_t*)&s2;
    bf16_t *o1p = (bf16_t*)&o1, *o2p = (bf16_t*)&o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x1 = bf2f(ap[e]), x2 = bf2f(bp[e]);
        o1p[e] = f2bf(rbf(x1 * bf2f(c1p[e])) + rbf(-x2 * bf2f(s1p[e])));
        o2p[e] = f2bf(rbf(x2 * bf2f(c2p[e])) + rbf(x1 * bf2f(s2p[e])));
    }
}

// ---- fp8 KV cache (kv8.hip; attention.hip DecodeTile<HS, CacheFp8>) --------------------------
// One e4m3fn byte per element and one int8 power-of-two exponent per (slot, group, position) vector: value = e4m3 * 2^e
// (include/dualhyp_hip.h states the scheme).  The bytes keep the 32-key tiles above, HS*32 bytes each, and a wave-wide
// contiguous 1-KiB load is still lane i <- 16 B at i*16: a 1-KiB block packs TWO k-step fragments, 8 bytes each per lane
// (lane = 32 lh + lr as above):
//   K  tile: [kp = d/32][lh = (d/8)&1][lr = key&31][hf = (d/16)&1][8 d]   bytes 0..7: fragment ks = 2kp, 8..15: ks = 2kp + 1
//   V^T tile: [dt = d/32][lh][lr = d&31][s2][8 keys]                       bytes 0..7: fragment (dt, s2 = 0), 8..15: (dt, 1),
//             the 8 keys in the order of vfrag_off.
// The exponents are plain [slot][group][position] int8 arrays, one for K and one for V.
// Offsets in bytes from the start of the (slot, group) block of s_max*HS bytes.
template <int HS>
__device__ __forceinline__ size_t k8_off(int key, int d) {
    const int t = key >> 5, lr = key & 31, kp = d >> 5, hf = (d >> 4) & 1, lh = (d >> 3) & 1, e = d & 7;
    return ((size_t)((t * (HS / 32) + kp) * 2 + lh) * 32 + lr) * 16 + hf * 8 + e;
}
template <int HS>
__device__ __forceinline__ size_t v8_off(int key, int d) {
    const int t = key >> 5, kk = key & 31, s2 = kk >> 4, r = kk & 15;
    const int j = ((r >> 3) << 2) | (r & 3), lh = (r >> 2) & 1, dt = d >> 5, lr = d & 31;
    return ((size_t)((t * (HS / 32) + dt) * 2 + lh) * 32 + lr) * 16 + s2 * 8 + j;
}
// start (in bytes) of 1-KiB block b (K: kp, V^T: dt) of tile t; add lane*16
template <int HS> __device__ __forceinline__ size_t kv8_blk(int t, int b) { return (size_t)(t * (HS / 32) + b) * 1024; }

// 2^e as fp32, e in [-126, 127]
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
// the exponent of a vector whose largest magnitude has the bf16 bits `abits` (sign cleared): the smallest e with
// amax <= 448 * 2^e, from the exponent and mantissa fields alone.  amax = 1.f * 2^(E - 127): e = E - 127 - 8 while
// 1.f <= 1.75 (mantissa <= 0x60 of 0x80), one more above; clamped to [-100, 100]; 0 for an all-zero vector.
__device__ __forceinline__ int kv8_exponent(uint32_t abits) {
    if (abits == 0) return 0;
    const int e = (int)(abits >> 7) - 135 + ((abits & 0x7f) > 0x60 ? 1 : 0);
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
// e4m3fn_rne(x * inv) saturated to +-448 (never the NaN encoding), inv = 2^-e: the scaling is exact
__device__ __forceinline__ float kv8_scaled(bf16_t x, float inv) { return fminf(fmaxf(bf2f(x) * inv, -448.0f), 448.0f); }
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);   // OCP e4m3fn on gfx950, round to nearest even
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (uint32_t)v;
}
// four e4m3 bytes of `w` times the four scales -> four bf16 (two dwords).  An e4m3 value has 4 significant bits and
// the scale is a power of two, so the fp32 product is exact and its low 16 bits are zero: truncation is the conversion.
__device__ __forceinline__ void kv8_cvt4(uint32_t w, float s0, float s1, float s2, float s3, uint32_t& lo, uint32_t& hi) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    lo = (__float_as_uint(a[0] * s0) >> 16) | (__float_as_uint(a[1] * s1) & 0xffff0000u);
    hi = (__float_as_uint(b[0] * s2) >> 16) | (__float_as_uint(b[1] * s3) & 0xffff0000u);
}
// the four scales 2^e of the int8 exponents packed in `ew` (byte i = exponent i)
__device__ __forceinline__ void kv8_scales4(uint32_t ew, float* s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = kv8_pow2((int)(int8_t)(ew >> (8 * i)));
}

// ---- host-side error plumbing -------------------------------------------------------------
void dh_set_error(const char* fmt, ...);

#define DH_CHECK(cond, ...)                      \
    do {                                         \
        if (!(cond)) {                           \
            dh_set_error(__VA_ARGS__);           \
            return 1;                            \
        }                                        \
    } while (0)

#define DH_HIP(call)                                                                   \
    do {                                                                               \
        hipError_t _e = (call);                                                        \
        if (_e != hipSuccess) {                                                        \
            dh_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 2;                                                                  \
        }                                                                              \
    } while (0)

#define DH_LAUNCH_CHECK()                                                              \
    do {                                                                               \
        hipError_t _e = hipGetLastError();                                             \
        if (_e != hipSuccess) {                                                        \
            dh_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return 3;                                                                  \
        }                                                                              \
    } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// the runtime head size (which the caller has checked: 64, 96 or 128) as a compile-time constant: f(std::integral_constant<int, HS>{})
template <class F>
inline void dispatch_hs(int hs, F&& f) {
    if (hs == 64) f(std::integral_constant<int, 64>{});
    else if (hs == 96) f(std::integral_constant<int, 96>{});
    else f(std::integral_constant<int, 128>{});
}

// Stop conditions (include/dualhyp_hip.h): a dh_stop_spec as the kernels take it, by value.  set / seqs are the caller's device arrays;
// the sequences' lengths (2 .. 8) ride in the kernel arguments, 4 bits each.  All zero: off, the tail the kernels always had.
struct dh_stop_args {
    const uint32_t* set = nullptr;
    const int32_t* seqs = nullptr;
    uint32_t lens = 0;
    int n_seqs = 0;
    __host__ __device__ bool on() const { return set != nullptr || n_seqs != 0; }
    bool operator==(const dh_stop_args& o) const { return set == o.set && seqs == o.seqs && lens == o.lens && n_seqs == o.n_seqs; }
};
// Stop conditions (include/dualhyp_hip.h): w[0] is the pick that has just been appended, w[k] the generated token k places before it
// (-1 where that place is prompt), m the tokens generated with the pick counted.  True when the pick is in the stop set or the
// generated text now ends on one of the stop sequences.  A few uniform loads behind the pick; it never changes one.  Shared by the
// sampling kernels' tails (sampling.hip) and the beam merge under device histories (beam.hip).
__device__ __forceinline__ bool stop_hit(const dh_stop_args& sa, const int (&w)[DH_MAX_STOP_LEN], int m) {
    const int t = w[0];
    if (sa.set && ((sa.set[t >> 5] >> (t & 31)) & 1u)) return true;
    for (int s = 0; s < sa.n_seqs; ++s) {
        const int L = (int)((sa.lens >> (4 * s)) & 15u);
        if (L > m) continue;                                    // a match never reaches back into the prompt
        const int32_t* q = sa.seqs + s * DH_MAX_STOP_LEN;
        bool eq = true;
#pragma unroll
        for (int k = 0; k < DH_MAX_STOP_LEN; ++k)
            if (k < L && q[L - 1 - k] != w[k]) eq = false;
        if (eq) return true;
    }
    return false;
}
// the checks of every entry that takes a dh_stop_spec (capi.hip); start_ok: the entry has a way to the prompt lengths
int dh_stop_pack(const char* name, const dh_stop_spec* stop, bool start_ok, dh_stop_args& out);

// Nucleus and min-p (include/dualhyp_hip.h): the two parameters as the kernels take them, by value.  top_p is the caller's fp32 value
// (1: off); lmin = (float)log((double)min_p), computed once here on the host, is read only when min_p_on.  The default is off: the
// sampled branch the kernels always had.
struct dh_nucleus_args {
    float top_p = 1.f;
    float lmin = 0.f;
    int min_p_on = 0;
    float min_p = 0.f;                                  // the caller's value, for the key of a captured step
    __host__ __device__ bool on() const { return top_p < 1.f || min_p_on != 0; }
    bool operator==(const dh_nucleus_args& o) const { return top_p == o.top_p && min_p == o.min_p; }
};
// the checks of every entry that takes (top_p, min_p) (capi.hip): top_p in (0, 1], min_p in [0, 1], neither NaN
int dh_nucleus_pack(const char* name, float top_p, float min_p, dh_nucleus_args& out);

// Penalties (include/dualhyp_hip.h): dh_penalty_args goes to the kernels as it is, by value.  Off: nothing reads a history for it.
constexpr dh_penalty_args DH_PENALTY_OFF{1.f, 0.f, 0.f};
__host__ __device__ inline bool dh_penalty_on(const dh_penalty_args& p) { return p.repetition != 1.f || p.frequency != 0.f || p.presence != 0.f; }
inline bool dh_penalty_same(const dh_penalty_args& a, const dh_penalty_args& b) {
    return a.repetition == b.repetition && a.frequency == b.frequency && a.presence == b.presence;
}
// the checks of every entry that takes a dh_penalty_args (capi.hip): null is off; finite, repetition in [1/8, 8], the others in [-8, 8]
int dh_penalty_pack(const char* name, const dh_penalty_args* in, dh_penalty_args& out);

// Contextual biasing (include/dualhyp_hip.h): a dh_bias_spec as the kernels take it, by value: the caller's three device arrays and the
// entry count.  n_ids, the ids in all entries, is the host's, for the limit a penalty shares with it.  n = 0: off.
struct dh_bias_args {
    const int32_t* ids = nullptr;                       // [n, DH_MAX_BIAS_LEN]
    const int32_t* len = nullptr;                       // [n]
    const float* boost = nullptr;                       // [n]
    int n = 0;
    int n_ids = 0;
    bool operator==(const dh_bias_args& o) const { return ids == o.ids && len == o.len && boost == o.boost && n == o.n && n_ids == o.n_ids; }
};
// the checks of every entry that takes a dh_bias_spec (capi.hip), made on the spec's host copies: null or n = 0 is off; 1 ..
// DH_MAX_BIAS_ENTRIES entries of 1 .. DH_MAX_BIAS_LEN ids in [0, vocab), finite boosts, vocab <= 131072; start_ok: the entry was given
// the prompt lengths
int dh_bias_pack(const char* name, const dh_bias_spec* spec, int vocab, bool start_ok, dh_bias_args& out);

// Automaton constraints (include/dualhyp_hip.h): a dh_automaton_spec as the kernels take it, by value: the caller's five device arrays and
// the counts the kernels clamp by.  n_seq is the host's, for the launchers' check of init / state against the call.  edge_off null: off.
struct dh_automaton_args {
    const int32_t* edge_off = nullptr;                  // [n_states + 1]
    const int32_t* edge_tok = nullptr;                  // [n_edges], strictly ascending inside a state
    const int32_t* edge_dst = nullptr;                  // [n_edges]
    const int32_t* init = nullptr;                      // [n_seq]
    int32_t* state = nullptr;                           // [n_seq], the kernels' own
    int n_states = 0;
    int n_edges = 0;
    int n_seq = 0;
    __host__ __device__ bool on() const { return edge_off != nullptr; }
    bool operator==(const dh_automaton_args& o) const {
        return edge_off == o.edge_off && edge_tok == o.edge_tok && edge_dst == o.edge_dst && init == o.init && state == o.state &&
               n_states == o.n_states && n_edges == o.n_edges && n_seq == o.n_seq;
    }
};
// the checks of every entry that takes a dh_automaton_spec (capi.hip), made on the spec's host copies: null is off; offsets monotone from 0
// to n_edges, tokens in [0, vocab) and strictly ascending inside a state, edge_dst and init in [0, n_states), vocab <= 131072; start_ok: the
// entry was given the prompt lengths
int dh_automaton_pack(const char* name, const dh_automaton_spec* spec, int vocab, bool start_ok, dh_automaton_args& out);

// The options of one pick, as the sampling launchers (sampling.hip) take them from the exported entries and from the engine's captured
// steps, which compare them as part of a step's key.  The default is every option off: the kernels the plain entries always launched.  A
// new sampler option is one member here, one line of operator==, and its share of the launchers' check and pack functions.
struct dh_pick_ctl {
    float* logprobs = nullptr;                          // fp32 beside `tokens`: each appended token's log-probability (dh_engine_set_logprobs)
    int top_n = 0;                                      // the row's top_n alternatives as well, into top_ids / top_lp
    int32_t* top_ids = nullptr;                         // ([n_seq, tok_ld, top_n], dh_engine_set_top_logprobs)
    float* top_lp = nullptr;
    const uint32_t* mask = nullptr;                     // [n_seq, mask_ld] words: the sequences' allowed tokens, null = the kernels without
    int mask_ld = 0;                                    // one (dh_engine_set_token_mask)
    int ngram = 0;                                      // no-repeat n-grams, 0 = the kernels without it (dh_engine_set_no_repeat_ngram)
    const int32_t* start = nullptr;                     // [n_seq] prompt lengths: what ngram, stop's sequences, pen, bias and aut count from
    dh_stop_args stop;                                  // the stop test behind the pick (dh_engine_set_stop)
    dh_nucleus_args nuc;                                // top_p / min_p of the sampled branch (dh_engine_set_nucleus)
    dh_penalty_args pen = DH_PENALTY_OFF;               // the three penalties (dh_engine_set_penalties)
    dh_bias_args bias;                                  // the bias entries (dh_engine_set_bias)
    dh_automaton_args aut;                              // the sequences' automata (dh_engine_set_automaton)
    // ngram, pen, bias or an automaton on: the history-reading kernel family
    bool hist() const { return ngram > 0 || dh_penalty_on(pen) || bias.n > 0 || aut.on(); }
    bool operator==(const dh_pick_ctl& o) const {
        return logprobs == o.logprobs && top_n == o.top_n && top_ids == o.top_ids && top_lp == o.top_lp && mask == o.mask &&
               mask_ld == o.mask_ld && ngram == o.ngram && start == o.start && stop == o.stop && nuc == o.nuc &&
               dh_penalty_same(pen, o.pen) && bias == o.bias && aut == o.aut;
    }
};

// the sampling step of the engine's decode graphs (sampling.hip): dh_sample_bf16 with the step counter read from the device, and
// dh_sample_rows_bf16
int dh_sample_impl(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, int n_seq,
                   float temperature, int top_k, int64_t eos_id, uint64_t seed, int step, const int32_t* step_dev,
                   const dh_pick_ctl& ctl, void* stream);
int dh_sample_rows_impl(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                        const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq, int max_new, float temperature,
                        int top_k, int64_t eos_id, uint64_t seed, const dh_pick_ctl& ctl, void* stream);

// the verify step of speculative greedy decoding (engine.hip, dh_engine_decode_spec): its attention (decode_fused.hip) and its
// acceptance kernel (sampling.hip)
int dh_attn_verify_fused_impl(const float* qkv32, int n_part, int pairs, int n_seq, int S, int qkv_dim, int n_ext,
                              const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* cos,
                              const dh_bf16* sin, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* k_cache,
                              dh_bf16* vT_cache, dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int p_max, void* stream);
// draw ("Sampled verification" of the header, dh_engine_decode_spec_draw; null: the arg-max, ctl's nuc, pen, bias and aut off): every
// position draws with top_k and the key (seed, n - (limit - max_new), sequence), under ctl's four as well
struct dh_spec_draw {
    int top_k = 0;
    uint64_t seed = 0;
    int max_new = 0;
};
int dh_spec_accept_impl(const dh_bf16* logits, int vocab, const int64_t* row_ids, int S, int64_t* tokens, int tok_ld,
                        int32_t* length, int32_t* done, const int32_t* limit, int n_seq, float temperature, int64_t eos_id,
                        const int32_t* step_dev, int32_t* counters, const dh_pick_ctl& ctl, void* stream,
                        const dh_spec_draw* draw = nullptr);

// the selection step of beam search (beam.hip, dh_beam_select_bf16), as the engine's captured step calls it
// stop: its set ends a hypothesis as the EOS does, its sequences as well under device histories; hist (nullable, int64
// [2][n_utt * W][max_new], "Beam histories" of the header) with ngram (0: no ban): null is the step without histories, the launches it
// always made
int dh_beam_select_impl(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new, int64_t eos_id, int step,
                        const int32_t* step_dev, const dh_beam_state& st, int32_t* cand_ids, float* cand_lp, const uint32_t* mask,
                        int mask_ld, const dh_stop_args& stop, int32_t* fin_tok, void* stream, int64_t* hist = nullptr, int ngram = 0);
// its candidates under a ban (sampling.hip, beam_top_hist_kernel)
int dh_beam_top_hist_impl(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new, int32_t* out_ids,
                          float* out_lp, const uint32_t* mask, int mask_ld, const int64_t* hist, int ngram, const int32_t* n_steps,
                          const int32_t* done, void* stream);

// the table update and one-tile copy of a beam step under a tile table (beam.hip, beam_retile_kernel; "Beam KV tile table" of the
// header): cache_tab, the engine's device table of n_tabs cache pointers, or null and the pair (c0, c1) with n_tabs = 2
int dh_beam_retile_impl(dh_bf16* const* cache_tab, dh_bf16* c0, dh_bf16* c1, int n_tabs, dh_bf16* scratch, int32_t* tab, int nt,
                        const int32_t* beam_parent, const int32_t* n_steps, const int32_t* plen, const int32_t* step_dev, int step, int rows,
                        int W, int max_new, int n_groups, int hs, int s_max, void* stream);

// hipFuncSetAttribute applies to the CURRENT device, and the launchers are entered from several host threads
// (one engine per thread, dualhyp_amd/pipeline.py): remember per device that the attribute is set.  Two threads
// racing on the first launch both set it, which is harmless.  `kernel` must be parenthesised if it contains commas.
#define DH_MAX_LDS_ONCE(kernel, bytes)                                                                       \
    do {                                                                                                     \
        static std::atomic<uint64_t> _done{0};                                                               \
        int _dev = 0;                                                                                        \
        DH_HIP(hipGetDevice(&_dev));                                                                         \
        const uint64_t _bit = 1ull << (_dev & 63);                                                           \
        if (!(_done.load(std::memory_order_acquire) & _bit)) {                                               \
            DH_HIP(hipFuncSetAttribute((const void*)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
            _done.fetch_or(_bit, std::memory_order_release);                                                 \
        }                                                                                                    \
    } while (0)
