// MXFP6 activations for the MXFP4 serving path (include/dualhyp_hip.h "MXFP6 activations"): csrc/mxfp4.hip's two GEMM kernels with
// the e4m3 activation operand replaced by OCP MX e2m3 blocks (32 consecutive k of a row: 32 six-bit codes and one E8M0 byte, no
// per-token scale), and the two quantisers that produce them.  Every product runs on v_mfma_scale_f32_16x16x128_f8f6f4 with operand
// format e2m1 on the W side (A) and e2m3 on the x side (B), each side's E8M0 byte in its own scale register:
//     y[m,n] = epilogue( bf16( sum_k e2m3(xq[m,k]) * 2^(sx[m,k/32] - 127) * e2m1(wq[n,k]) * 2^(sw[n,k/32] - 127) ) )
// The instruction runs this pair at the e2m1 x e2m1 rate, twice that of any pair with an e4m3 operand (tools/mxfp6_probe.hip,
// MEASUREMENTS.md "MXFP6 activations").
//
// Operand map (tools/mxfp6_probe.hip, one-hot on the GPU, both operand positions; tests/test_hip_mxfp6.py exact integers).  The
// instruction's own k index runs 0..127:
//   e2m3 operand: lane l holds k [32 (l >> 4), +32) of row / column l & 15 in registers 0..5 of the eight (6..7 are not read):
//                 element i = k - 32 (l >> 4) is the six bits 6 i .. 6 i + 5 of the lane's 192, little endian (bit 6 i the low
//                 mantissa bit, bit 6 i + 5 the sign), so an element may straddle two registers; the block's scale is byte 0
//                 (op_sel 0) of the lane's own scale register — one MX block per lane, as the e2m1 operand has it;
//   e2m1 operand: as csrc/mxfp4.hip states it (registers 0..3, k = 32 (l >> 4) + 2 j in the low nibble of byte j).
// Unlike the e4m3 operand, both sides hold the SAME 32 consecutive k per lane: no halves to keep apart.
//
// Physical layout of a quantised activation matrix (the header states it in words): FRAGMENT ORDER, as the weights.  Per group g
// of 16 rows and k-step t of 128, 1536 code bytes as three planes of 512: plane p holds bytes 8 p .. 8 p + 7 of lane l's 24 at
// p * 512 + l * 8 (l = 16 * MX block of the k-step + row of the group); and 64 scale bytes with lane l's at l.  So
//   - the streaming kernel's wave loads an x fragment as three 8-byte requests per lane, each contiguous over the wave, and its
//     scale as one byte: no line -> fragment shuffle (mxfp4.hip: 16 DPP + 16 ds_bpermute per fragment pair and row group);
//   - the tiled kernel's LDS-DMA is a linear copy (a 128-row stage of x is 8 groups x 1536 B = 12 KiB, 3 requests of 16 B per
//     lane and wave) and the fragment comes back as three ds_read_b64 of 64 consecutive 8-byte pieces, conflict-free.
// The tiled kernel's scales go through LDS as in mxfp4.hip, now on both sides: each wave copies the 4 x 64 bytes of ITS four W
// fragments and of ITS four x fragments per k-step.  A stage is W 8 KiB + x 12 KiB + 2 KiB of scales, and still seven requests
// per wave (2 W + 3 x + 2 scale), so the counted vmcnt waits of the 4-stage loop are mxfp4.hip's.
// Rows past M in the last group of 16 exist in the buffer and are never written by the quantisers; they meet only the
// accumulator columns of rows >= M, which are not stored.
//
//   mx6_quant_rows_kernel / mx6_rmsnorm_quant_kernel   bf16 rows (/ RMSNorm of them) -> codes + scale bytes in the layout above
//   gemm_mxfp4a6_kernel         128 x 128 x 128 tiles, 4 waves x (4 x 4) MFMA tiles, 2 or 4 LDS stages
//   gemm_mxfp4a6_skinny_kernel  M <= 128: W streamed HBM -> VGPR once, K dealt over the 8 waves of a block, NG = 1 / 2 / 4
// Both GEMMs fix one fp32 chain per output, independent of the row count (tiled: k ascending in one accumulator; streaming: each
// wave its k-steps ascending, waves added in order).
#include "common.h"
#include "gemm.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) int i32x2;

namespace {

constexpr int MX_STREAM_MAX_ROWS = 128;
constexpr int XBLK = 1536;              // code bytes of one group of 16 rows and one k-step

// A = W: e2m1 (format 4), registers 0..3; B = x: e2m3 (format 2), registers 0..5; ws / xs: the E8M0 byte of each lane's block in byte 0
__device__ __forceinline__ f32x4 mfma_mx46(const i32x4& w, const i32x2& x0, const i32x2& x1, const i32x2& x2, const f32x4& c, int ws, int xs) {
    const i32x8 a{w[0], w[1], w[2], w[3], 0, 0, 0, 0};
    const i32x8 b{x0[0], x0[1], x1[0], x1[1], x2[0], x2[1], 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4 /* A e2m1 */, 2 /* B e2m3 */, 0, ws, 0, xs);
}

// ------------------------------------------------------------------------------ quantisers
// Every step is exact in fp32: e from the exponent field, a = |x| * 2^-e by a power of two (a < 8), round-half-even of a in units of
// the grid step of its binade (1/8 below 2, 1/4 below 4, 1/2 above), which is the index in the ascending grid: the even index is the
// even code.  16 * 2 = 32 would be 8.0: saturated to code 31 (7.5).
// the block's exponent e from its amax (>= 0, finite)
__device__ __forceinline__ int mx6_exponent(float am) {
    const uint32_t ab = __float_as_uint(am);
    int e = (int)(ab >> 23) - 129;                        // floor(log2 amax) - 2; an fp32 subnormal (field 0) clamps
    e = e < -126 ? -126 : e;
    return ab == 0 ? 0 : e;
}
// the codes of eight consecutive elements as 48 bits, element j in bits 6 j .. 6 j + 5; inv = 2^-e
__device__ __forceinline__ uint64_t mx6_piece(const float* v, float inv) {
    uint64_t piece = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float a = fabsf(v[j]) * inv;
        const float units = a < 2.f ? 8.f : (a < 4.f ? 4.f : 2.f);
        const int first = a < 2.f ? 0 : (a < 4.f ? 8 : 16);
        int code = (int)__builtin_rintf(a * units) + first;
        code = code > 31 ? 31 : code;
        if (code != 0 && v[j] < 0.f) code |= 32;
        piece |= (uint64_t)code << (6 * j);
    }
    return piece;
}
// plane p (0..2) of the 192 bits made of four 48-bit pieces
__device__ __forceinline__ uint64_t mx6_plane(int p, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3) {
    return p == 0 ? (p0 | (p1 << 48)) : p == 1 ? ((p1 >> 16) | (p2 << 32)) : ((p2 >> 32) | (p3 << 16));
}

// The fused RMSNorm form, one 256-thread block per row (the order of its sum of squares is dh_rmsnorm_bf16's): thread tid holds the 8 consecutive elements of chunk
// c = tid + 256 i, so the four lanes of a quad hold one MX block (K % 128 == 0: a quad is active as a whole).  The quad agrees on amax,
// each lane packs its eight codes into 48 bits, the quad's 192 bits are exchanged, lanes 0..2 store one 8-byte plane each and lane 3
// the scale byte.
__device__ __forceinline__ void mx6_quant_store(const float (&v)[8], int row, int c, int nk, uint8_t* __restrict__ q, uint8_t* __restrict__ qs) {
    const int lane = threadIdx.x & 63;
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(v[j]));
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    const int e = mx6_exponent(am);
    const uint64_t piece = mx6_piece(v, __uint_as_float((uint32_t)(127 - e) << 23));
    const int q0 = lane & ~3, me = lane & 3;
    const uint64_t p0 = __shfl(piece, q0, 64), p1 = __shfl(piece, q0 + 1, 64), p2 = __shfl(piece, q0 + 2, 64), p3 = __shfl(piece, q0 + 3, 64);
    const uint64_t plane = mx6_plane(me, p0, p1, p2, p3);
    const int b = c >> 2, t = b >> 2, l = 16 * (b & 3) + (row & 15);
    const size_t blk = (size_t)(row >> 4) * nk + t;
    if (me < 3) *reinterpret_cast<uint64_t*>(q + blk * XBLK + me * 512 + l * 8) = plane;
    else qs[blk * 64 + l] = (uint8_t)(e + 127);
}

// The plain quantiser: one thread per MX block and one wave per (group of 16 rows, k-step), lane l = 16 * MX block + row as in the layout,
// so each plane of the fragment block is ONE contiguous 512-B store of the wave and the amax needs no exchange.  (A block per row with
// the quad exchange above, as the fused form has to have it, stores 8-byte pieces 128 B apart: 2.5-2.6 x the time at 49 152 rows and at 128
// rows x 14 336, the same at 32 rows x 4 096; MEASUREMENTS.md "MXFP6 activations".)
__global__ __launch_bounds__(256) void mx6_quant_rows_kernel(const bf16_t* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ qs,
                                                                int rows, int K) {
    const int l = threadIdx.x & 63, nk = K >> 7;
    const int t = blockIdx.y * 4 + (threadIdx.x >> 6), row = blockIdx.x * 16 + (l & 15);
    if (t >= nk || row >= rows) return;
    const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * K + t * 128 + (l >> 4) * 32);
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 u = xr[i];
        const bf16_t* p = reinterpret_cast<const bf16_t*>(&u);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[i * 8 + j] = bf2f(p[j]);
            am = fmaxf(am, fabsf(v[i * 8 + j]));
        }
    }
    const int e = mx6_exponent(am);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
    const uint64_t p0 = mx6_piece(v, inv), p1 = mx6_piece(v + 8, inv), p2 = mx6_piece(v + 16, inv), p3 = mx6_piece(v + 24, inv);
    const size_t blk = (size_t)blockIdx.x * nk + t;
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<uint64_t*>(q + blk * XBLK + p * 512 + l * 8) = mx6_plane(p, p0, p1, p2, p3);
    qs[blk * 64 + l] = (uint8_t)(e + 127);
}

// fp8.hip's rmsnorm_quant_fp8_block_kernel up to the bf16 row (elementwise.hip's rounding points and Q11 flag, the same order of
// the sum of squares for every row count), then the quantiser above in registers
template <int EPT>
__global__ __launch_bounds__(256) void mx6_rmsnorm_quant_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                                bf16_t* __restrict__ xn_out, uint8_t* __restrict__ q,
                                                                uint8_t* __restrict__ qs, int d, float eps,
                                                                const uint8_t* __restrict__ row_tail) {
    constexpr int NC = EPT / 8;
    __shared__ float red[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunk = d >> 3;
    const uint4* xr = reinterpret_cast<const uint4*>(x + (size_t)row * d);
    const uint4* wr = reinterpret_cast<const uint4*>(w);
    float v[NC][8];
    uint4 wu[NC];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        if (c < nchunk) {
            const uint4 u = xr[c];
            wu[i] = wr[c];
            const bf16_t* p = reinterpret_cast<const bf16_t*>(&u);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                v[i][j] = bf2f(p[j]);
                ss += rbf(v[i][j] * v[i][j]);
            }
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    ss = (red[0] + red[1]) + (red[2] + red[3]);
    const float ms = rbf(ss / (float)d);
    const float t = rbf(ms + eps);
    const bool tail = row_tail != nullptr && row_tail[row] != 0;
    const float r = tail ? rbf(1.0f / rbf(sqrtf(t))) : rbf(1.0f / sqrtf(t));
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = tid + i * 256;
        if (c < nchunk) {
            const bf16_t* wp = reinterpret_cast<const bf16_t*>(&wu[i]);
            uint4 o;
            bf16_t* op = reinterpret_cast<bf16_t*>(&o);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                op[j] = f2bf(bf2f(wp[j]) * rbf(v[i][j] * r));
                v[i][j] = bf2f(op[j]);
            }
            if (xn_out) reinterpret_cast<uint4*>(xn_out + (size_t)row * d)[c] = o;
            mx6_quant_store(v[i], row, c, d >> 7, q, qs);
        }
    }
}

// ------------------------------------------------------------------------------ GEMM argument block
struct Mx6Args {
    const uint8_t* x;      // [ceil(M / 16)][K / 128][3][64][8] e2m3 codes in fragment order
    const uint8_t* xs;     // [ceil(M / 16)][K / 128][64] E8M0 bytes in fragment order
    const uint8_t* w;      // [N / 16][K / 128][64][16] nibbles in fragment order
    const uint8_t* w2;     // SWIGLU: fc_2
    const uint8_t* ws;     // [N / 16][K / 128][64] E8M0 bytes in fragment order
    const uint8_t* ws2;
    bf16_t* y;             // [M, N]
    const bf16_t* vec_a;   // ADAPTER scale [N]
    const bf16_t* vec_b;   // ADAPTER bias [N]
    const bf16_t* resid;   // [M, N] or null
    int M, N, K;
    int nb_n, nb_m;
    int gm;                // tiled kernel: m-tiles per band of the tile walk
};

// mxfp4.hip's rounding points without the token scale: round, epilogue
template <int EPI>
__device__ __forceinline__ float mx6_finish(float acc, const Mx6Args& a, int n) {
    float o = rbf(acc);
    if (EPI == DH_EPI_ADAPTER) o = rbf(bf2f(a.vec_a[n]) * rbf(o + bf2f(a.vec_b[n])));
    return o;
}

// ------------------------------------------------------------------------------ tiled kernel
constexpr int W_STAGE = 8 * 1024;       // 8 W fragment blocks (16 rows x 128 k each)
constexpr int X_STAGE = 8 * XBLK;       // 8 x fragment blocks
constexpr int S_STAGE = 4 * 256;        // per wave: the scale bytes of its four W fragments; the same again for its four x fragments
constexpr int STAGE = W_STAGE + X_STAGE + 2 * S_STAGE;

template <int EPI, bool RESID, int NST>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4a6_kernel(Mx6Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // NST x (W blocks, x blocks, W scales, x scales)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wm = wave & 1;
    const int nwg = a.nb_n * a.nb_m;
    int tile;
    {
        const int bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    }
    int tm, tn;
    if (a.gm > 1) {
        const int band = tile / (a.gm * a.nb_n), within = tile - band * (a.gm * a.nb_n);
        const int rows = min(a.gm, a.nb_m - band * a.gm);
        tm = band * a.gm + within % rows; tn = within / rows;
    } else {
        tm = tile / a.nb_n; tn = tile % a.nb_n;
    }
    const int m0 = tm * 128;
    const int n0 = (EPI == DH_EPI_SWIGLU) ? tn * 64 : tn * 128;
    const int nk = a.K >> 7, ngrp = a.N >> 4, mgrp = (a.M + 15) >> 4;

    // W: mxfp4.hip's slots.  LDS slot s = 4 wn' + i holds fragment i of wave row wn' (SWIGLU: i < 2 fc_1, else fc_2); a group past
    // N reads the last one, its outputs are not stored
    auto slot_group = [&](int slot, bool& second) __attribute__((always_inline)) {
        const int swn = slot >> 2, i = slot & 3;
        int g;
        if (EPI == DH_EPI_SWIGLU) { second = i >= 2; g = (n0 >> 4) + swn * 2 + (i & 1); }
        else { second = false; g = (n0 >> 4) + slot; }
        return g < ngrp ? g : ngrp - 1;
    };
    // x: group j of the tile is rows m0 + 16 j; one past the last group of the matrix reads the last one, its outputs are not stored
    auto x_group = [&](int j) __attribute__((always_inline)) {
        const int g = (m0 >> 4) + j;
        return g < mgrp ? g : mgrp - 1;
    };
    const uint8_t* srcW[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        bool second;
        const int g = slot_group(wave * 2 + j, second);
        srcW[j] = (second ? a.w2 : a.w) + (size_t)g * nk * 1024 + lane * 16;
    }
    const uint8_t* srcS;
    {
        bool second;
        const int g = slot_group(wn * 4 + (lane >> 4), second);
        srcS = (second ? a.ws2 : a.ws) + (size_t)g * nk * 64 + (lane & 15) * 4;
    }
    // wave `wave` copies x groups 2 wave and 2 wave + 1 of the tile: 3072 linear bytes, 16 per lane and request
    const uint8_t* srcX[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int off = j * 1024 + lane * 16;
        const int gi = off >= XBLK ? 1 : 0;
        srcX[j] = a.x + (size_t)x_group(wave * 2 + gi) * nk * XBLK + (off - gi * XBLK);
    }
    // and the scale bytes of the four x groups it multiplies: 4 wm .. 4 wm + 3
    const uint8_t* srcXS = a.xs + (size_t)x_group(wm * 4 + (lane >> 4)) * nk * 64 + (lane & 15) * 4;
    auto stage = [&](int buf, int kt) {
        char* sW = smem + buf * STAGE;
        char* sX = sW + W_STAGE;
        char* sS = sX + X_STAGE + wave * 256;
        char* sXS = sX + X_STAGE + S_STAGE + wave * 256;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(srcW[j] + (size_t)kt * 1024, sW + (wave * 2 + j) * 1024);
#pragma unroll
        for (int j = 0; j < 3; ++j) glds16(srcX[j] + (size_t)kt * XBLK, sX + wave * 3072 + j * 1024);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcS + (size_t)kt * 64),
                                         (__attribute__((address_space(3))) void*)sS, 4, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcXS + (size_t)kt * 64),
                                         (__attribute__((address_space(3))) void*)sXS, 4, 0, 0);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, kg = lane >> 4;
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const char* sW = smem + buf * STAGE;
        const char* sX = sW + W_STAGE;
        const char* sS = sX + X_STAGE + wave * 256;
        const char* sXS = sX + X_STAGE + S_STAGE + wave * 256;
        i32x4 fa[4];
        int fs[4], fxs[4];
        i32x2 fb[4][3];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = *reinterpret_cast<const i32x4*>(sW + (wn * 4 + i) * 1024 + lane * 16);
            fs[i] = *reinterpret_cast<const uint8_t*>(sS + i * 64 + lane);
            fxs[i] = *reinterpret_cast<const uint8_t*>(sXS + i * 64 + lane);
#pragma unroll
            for (int p = 0; p < 3; ++p) fb[i][p] = *reinterpret_cast<const i32x2*>(sX + (wm * 4 + i) * XBLK + p * 512 + lane * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma_mx46(fa[i], fb[j][0], fb[j][1], fb[j][2], acc[i][j], fs[i], fxs[j]);
    };
    if constexpr (NST == 2) {
        stage(0, 0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
            compute(cur);
            __syncthreads();
        }
    } else {
        // seven requests per wave and stage, three stages ahead
#pragma unroll
        for (int p = 0; p < NST - 1; ++p)
            if (p < nk) stage(p, p);
        if (2 < nk) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
        else if (1 < nk) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 3 < nk) stage((kt + 3) % NST, kt + 3);
            compute(kt % NST);
            if (kt + 3 < nk) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
            else if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }

    // accumulator element r of tile (i,j): n = nt + 4*kg + r ; m = mt + frow
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + wm * 64 + j * 16 + frow;
        if (m >= a.M) continue;
        if (EPI == DH_EPI_SWIGLU) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = n0 + wn * 32 + i * 16 + 4 * kg;
                if (n >= a.N) continue;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = rbf(acc[i][j][e]);
                    const float u = rbf(acc[i + 2][j][e]);
                    o[e] = rbf(silu_fast(g)) * u;
                }
                *reinterpret_cast<uint2*>(a.y + (size_t)m * a.N + n) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + wn * 64 + i * 16 + 4 * kg;
                if (n >= a.N) continue;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = mx6_finish<EPI>(acc[i][j][e], a, n + e);
                if (RESID) {
                    const uint2 rr = *reinterpret_cast<const uint2*>(a.resid + (size_t)m * a.N + n);
                    const bf16_t* rp = reinterpret_cast<const bf16_t*>(&rr);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = bf2f(rp[e]) + o[e];
                }
                *reinterpret_cast<uint2*>(a.y + (size_t)m * a.N + n) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
            }
        }
    }
}

// ------------------------------------------------------------------------------ streaming kernel (M <= 128)
// gemm_mxfp4_skinny_kernel with the x side read in fragment order: one block = one group of 16 W rows (SWIGLU: of fc_1 and fc_2), K
// dealt round-robin in 128-wide k-steps over the 8 waves, the per-wave fp32 partials meet in LDS and thread t finishes output
// (n = t & 15, m = t >> 4).  Per k-step a lane loads its 16 B of nibbles and its scale byte non-temporally (each byte is needed
// once), and per group of 16 x rows its three 8-byte planes and its scale byte (every block reads them: they stay in L2).
constexpr int ROWS = 16, NW = 8;

template <int EPI, bool RESID, bool OUT32 = false, int NG = 1>
__global__ __launch_bounds__(512, 2) void gemm_mxfp4a6_skinny_kernel(Mx6Args a) {
    constexpr bool SW = EPI == DH_EPI_SWIGLU;
    constexpr int CH = SW ? 2 : 4;                        // k-steps loaded ahead per wave
    __shared__ __attribute__((aligned(16))) float part[NW][32][ROWS];
    __shared__ __attribute__((aligned(16))) float part2[SW ? NW : 1][32][ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * ROWS;
    const int lrow = lane & 15, kg = lane >> 4;
    const int nks = a.K >> 7, mgrp = (a.M + 15) >> 4;
    const size_t gofs = (size_t)blockIdx.x * nks;          // the group's first fragment block
    const uint8_t* wl = a.w + gofs * 1024 + lane * 16;
    const uint8_t* sl = a.ws + gofs * 64 + lane;
    const uint8_t* wl2 = SW ? a.w2 + gofs * 1024 + lane * 16 : nullptr;
    const uint8_t* sl2 = SW ? a.ws2 + gofs * 64 + lane : nullptr;
    // x fragments of row group g: rows 32 g .. 32 g + 15 (h = 0) and 32 g + 16 .. + 31 (h = 1); a group past the last one of the
    // matrix reads the last one, its outputs are not stored
    const uint8_t* xl[NG][2];
    const uint8_t* xsl[NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int grp = g * 2 + h;
            grp = grp < mgrp ? grp : mgrp - 1;
            xl[g][h] = a.x + (size_t)grp * nks * XBLK + lane * 8;
            xsl[g][h] = a.xs + (size_t)grp * nks * 64 + lane;
        }
    auto ldnt = [](const uint8_t* p) __attribute__((always_inline)) { return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p)); };
    auto ldsc = [](const uint8_t* p) __attribute__((always_inline)) { return (int)__builtin_nontemporal_load(p); };
    f32x4 acc_lo[NG], acc_hi[NG], acc2_lo[SW ? NG : 1], acc2_hi[SW ? NG : 1];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        acc_lo[g] = acc_hi[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (SW) acc2_lo[g] = acc2_hi[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int ks0 = wave; ks0 < nks; ks0 += NW * CH) {
        i32x4 wr[CH], wr2[SW ? CH : 1];
        int sc[CH], sc2[SW ? CH : 1];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int ks = ks0 + c * NW;
            if (ks < nks) {
                wr[c] = ldnt(wl + (size_t)ks * 1024);
                sc[c] = ldsc(sl + (size_t)ks * 64);
                if (SW) {
                    wr2[c] = ldnt(wl2 + (size_t)ks * 1024);
                    sc2[c] = ldsc(sl2 + (size_t)ks * 64);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g * 32 >= a.M) break;
            i32x2 xr[CH][2][3];
            int xsc[CH][2];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ks = ks0 + c * NW;
                if (ks < nks) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
#pragma unroll
                        for (int p = 0; p < 3; ++p) xr[c][h][p] = *reinterpret_cast<const i32x2*>(xl[g][h] + (size_t)ks * XBLK + p * 512);
                        xsc[c][h] = (int)xsl[g][h][(size_t)ks * 64];
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ks = ks0 + c * NW;
                if (ks < nks) {
                    acc_lo[g] = mfma_mx46(wr[c], xr[c][0][0], xr[c][0][1], xr[c][0][2], acc_lo[g], sc[c], xsc[c][0]);
                    acc_hi[g] = mfma_mx46(wr[c], xr[c][1][0], xr[c][1][1], xr[c][1][2], acc_hi[g], sc[c], xsc[c][1]);
                    if (SW) {
                        acc2_lo[g] = mfma_mx46(wr2[c], xr[c][0][0], xr[c][0][1], xr[c][0][2], acc2_lo[g], sc2[c], xsc[c][0]);
                        acc2_hi[g] = mfma_mx46(wr2[c], xr[c][1][0], xr[c][1][1], xr[c][1][2], acc2_hi[g], sc2[c], xsc[c][1]);
                    }
                }
            }
        }
    }
    const int tn = tid & 15, tmi = tid >> 4, nn = n0 + tn;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g * 32 >= a.M) break;                          // block-uniform
        if (g > 0) __syncthreads();                        // the previous group's sums have been read
        // C layout: col (m) = lane & 15, rows (n) = 4*(lane>>4) + reg
        *reinterpret_cast<f32x4*>(&part[wave][lrow][kg * 4]) = acc_lo[g];
        *reinterpret_cast<f32x4*>(&part[wave][16 + lrow][kg * 4]) = acc_hi[g];
        if (SW) {
            *reinterpret_cast<f32x4*>(&part2[wave][lrow][kg * 4]) = acc2_lo[g];
            *reinterpret_cast<f32x4*>(&part2[wave][16 + lrow][kg * 4]) = acc2_hi[g];
        }
        __syncthreads();
        const int tm = g * 32 + tmi;
        if (tm >= a.M || nn >= a.N) continue;
        const float* p = &part[0][0][0] + tmi * ROWS + tn;
        float o;
        if (SW) {
            float gt = 0.f, u = 0.f;
            const float* p2 = &part2[0][0][0] + tmi * ROWS + tn;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                gt += p[w * 32 * ROWS];
                u += p2[w * 32 * ROWS];
            }
            gt = rbf(gt);
            u = rbf(u);
            o = rbf(silu_fast(gt)) * u;
        } else {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += p[w * 32 * ROWS];
            o = mx6_finish<EPI>(s, a, nn);
            if (RESID) o = bf2f(a.resid[(size_t)tm * a.N + nn]) + o;
        }
        if (OUT32) reinterpret_cast<float*>(a.y)[(size_t)tm * a.N + nn] = o;     // bf16-exact value as fp32 (fused decode consumer)
        else a.y[(size_t)tm * a.N + nn] = f2bf(o);
    }
}

template <int EPI, bool RESID, int NST>
int launch_tiled_n(const Mx6Args& a, hipStream_t s) {
    constexpr int lds = NST * STAGE;
    DH_MAX_LDS_ONCE((gemm_mxfp4a6_kernel<EPI, RESID, NST>), lds);
    hipLaunchKernelGGL((gemm_mxfp4a6_kernel<EPI, RESID, NST>), dim3(a.nb_n * a.nb_m), dim3(256), lds, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(NST == 4 ? DH_ROUTE_MX4A6_T128_S4 : DH_ROUTE_MX4A6_T128_S2);
    return 0;
}

template <int EPI>
int launch_tiled(Mx6Args a, hipStream_t s) {
    a.gm = 4;
    // as mxfp4.hip: grids smaller than the chip walk K alone -> 4 stages, one block per CU; else 2 stages, two blocks
    if (a.nb_n * a.nb_m < 384) return a.resid ? launch_tiled_n<EPI, true, 4>(a, s) : launch_tiled_n<EPI, false, 4>(a, s);
    return a.resid ? launch_tiled_n<EPI, true, 2>(a, s) : launch_tiled_n<EPI, false, 2>(a, s);
}

template <int EPI, int NG>
int launch_skinny_ng(const Mx6Args& a, hipStream_t s) {
    dim3 grid(a.N / ROWS), block(512);
    if (a.resid) hipLaunchKernelGGL((gemm_mxfp4a6_skinny_kernel<EPI, true, false, NG>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_mxfp4a6_skinny_kernel<EPI, false, false, NG>), grid, block, 0, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(NG == 1 ? DH_ROUTE_MX4A6_STREAM_NG1 : NG == 2 ? DH_ROUTE_MX4A6_STREAM_NG2 : DH_ROUTE_MX4A6_STREAM_NG4);
    return 0;
}

template <int EPI>
int launch_skinny(const Mx6Args& a, hipStream_t s) {
    if (a.M <= 32) return launch_skinny_ng<EPI, 1>(a, s);
    if (a.M <= 64) return launch_skinny_ng<EPI, 2>(a, s);
    return launch_skinny_ng<EPI, 4>(a, s);
}

}  // namespace

extern "C" int dh_quant_rows_mxfp6(const dh_bf16* x, uint8_t* q, uint8_t* qscale, int rows, int K, void* stream) {
    DH_CHECK(x && q && qscale && rows >= 0 && K > 0 && K % 128 == 0, "dh_quant_rows_mxfp6: bad argument (K %% 128 must be 0)");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(mx6_quant_rows_kernel, dim3(cdiv(rows, 16), cdiv(K >> 7, 4)), dim3(256), 0, (hipStream_t)stream, x, q, qscale, rows, K);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_rmsnorm_quant_mxfp6(const dh_bf16* x, const dh_bf16* w, dh_bf16* xn_out, uint8_t* q, uint8_t* qscale, int rows,
                                      int d, float eps, const uint8_t* row_tail, void* stream) {
    DH_CHECK(x && w && q && qscale, "dh_rmsnorm_quant_mxfp6: null argument");
    DH_CHECK(rows >= 0 && d > 0 && d % 128 == 0 && d <= 8192, "dh_rmsnorm_quant_mxfp6: unsupported d=%d (need d %% 128 == 0, d <= 8192)", d);
    if (rows == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if (d <= 2048) hipLaunchKernelGGL((mx6_rmsnorm_quant_kernel<8>), dim3(rows), dim3(256), 0, s, x, w, xn_out, q, qscale, d, eps, row_tail);
    else if (d <= 4096) hipLaunchKernelGGL((mx6_rmsnorm_quant_kernel<16>), dim3(rows), dim3(256), 0, s, x, w, xn_out, q, qscale, d, eps, row_tail);
    else hipLaunchKernelGGL((mx6_rmsnorm_quant_kernel<32>), dim3(rows), dim3(256), 0, s, x, w, xn_out, q, qscale, d, eps, row_tail);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_linear_mxfp4a6_f32(const uint8_t* xq, const uint8_t* x_scale, const uint8_t* wq, const uint8_t* w_scale, float* y32,
                                     int M, int N, int K, void* stream) {
    DH_CHECK(xq && x_scale && wq && w_scale && y32, "dh_linear_mxfp4a6_f32: null operand");
    DH_CHECK(M >= 1 && M <= MX_STREAM_MAX_ROWS && N > 0 && N % 16 == 0 && K > 0 && K % 128 == 0,
             "dh_linear_mxfp4a6_f32: needs 1 <= M <= %d, N %% 16 == 0 and K %% 128 == 0 (M=%d N=%d K=%d)", MX_STREAM_MAX_ROWS, M, N, K);
    Mx6Args a{xq, x_scale, wq, nullptr, w_scale, nullptr, reinterpret_cast<bf16_t*>(y32), nullptr, nullptr, nullptr, M, N, K, 0, 0, 1};
    dim3 grid(N / ROWS), block(512);
    hipStream_t s = (hipStream_t)stream;
    // row groups as launch_skinny: the same kernel (and bits) as dh_linear_mxfp4a6_ex's streaming form, fp32 store
    if (M <= 32) hipLaunchKernelGGL((gemm_mxfp4a6_skinny_kernel<DH_EPI_PLAIN, false, true, 1>), grid, block, 0, s, a);
    else if (M <= 64) hipLaunchKernelGGL((gemm_mxfp4a6_skinny_kernel<DH_EPI_PLAIN, false, true, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_mxfp4a6_skinny_kernel<DH_EPI_PLAIN, false, true, 4>), grid, block, 0, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(M <= 32 ? DH_ROUTE_MX4A6_STREAM_NG1 : M <= 64 ? DH_ROUTE_MX4A6_STREAM_NG2 : DH_ROUTE_MX4A6_STREAM_NG4);
    return 0;
}

// kernel: 0 = by row count (streaming up to 128 rows, tiled above), 1 = tiled, 2 = streaming — dh_linear_mxfp4_ex's selector
extern "C" int dh_linear_mxfp4a6_ex(const uint8_t* xq, const uint8_t* x_scale, const uint8_t* wq, const uint8_t* w_scale, dh_bf16* y,
                                    int M, int N, int K, int epilogue, const uint8_t* w2q, const uint8_t* w2_scale,
                                    const dh_bf16* vec_a, const dh_bf16* vec_b, const dh_bf16* resid, int kernel, void* stream) {
    DH_CHECK(xq && x_scale && wq && w_scale && y, "dh_linear_mxfp4a6: null operand");
    DH_CHECK(kernel >= 0 && kernel <= 2, "dh_linear_mxfp4a6: kernel %d (0 auto, 1 tiled, 2 streaming)", kernel);
    DH_CHECK(kernel != 2 || M <= MX_STREAM_MAX_ROWS, "dh_linear_mxfp4a6: the streaming kernel takes at most %d rows (M=%d)", MX_STREAM_MAX_ROWS, M);
    DH_CHECK(M >= 0 && N > 0 && K > 0 && K % 128 == 0 && N % 16 == 0, "dh_linear_mxfp4a6: bad shape M=%d N=%d K=%d (K %% 128, N %% 16 must be 0)", M, N, K);
    DH_CHECK(epilogue == DH_EPI_PLAIN || epilogue == DH_EPI_SWIGLU || epilogue == DH_EPI_ADAPTER,
             "dh_linear_mxfp4a6: epilogue %d unsupported (LoRA is merged before quantisation)", epilogue);
    DH_CHECK(epilogue != DH_EPI_SWIGLU || (w2q && w2_scale && !resid), "dh_linear_mxfp4a6: SWIGLU needs w2/w2_scale and takes no residual");
    DH_CHECK(epilogue != DH_EPI_ADAPTER || (vec_a && vec_b), "dh_linear_mxfp4a6: ADAPTER needs scale/bias vectors");
    if (M == 0) return 0;
    Mx6Args a{xq, x_scale, wq, w2q, w_scale, w2_scale, y, vec_a, vec_b, resid, M, N, K, 0, 0, 1};
    hipStream_t s = (hipStream_t)stream;
    if (kernel == 2 || (kernel == 0 && M <= MX_STREAM_MAX_ROWS)) {
        switch (epilogue) {
            case DH_EPI_PLAIN: return launch_skinny<DH_EPI_PLAIN>(a, s);
            case DH_EPI_SWIGLU: return launch_skinny<DH_EPI_SWIGLU>(a, s);
            default: return launch_skinny<DH_EPI_ADAPTER>(a, s);
        }
    }
    a.nb_m = cdiv(M, 128);
    a.nb_n = epilogue == DH_EPI_SWIGLU ? cdiv(N, 64) : cdiv(N, 128);
    switch (epilogue) {
        case DH_EPI_PLAIN: return launch_tiled<DH_EPI_PLAIN>(a, s);
        case DH_EPI_SWIGLU: return launch_tiled<DH_EPI_SWIGLU>(a, s);
        default: return launch_tiled<DH_EPI_ADAPTER>(a, s);
    }
}
