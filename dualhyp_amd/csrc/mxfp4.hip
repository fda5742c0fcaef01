// MXFP4 weights for the fp8 serving path (include/dualhyp_hip.h "MXFP4 weights"): a third weight format of csrc/fp8.hip's
// path.  Activations stay e4m3 rows with one fp32 scale per token (dh_quant_rows_fp8 / dh_rmsnorm_quant_fp8); a weight row is
// OCP MX v1.0 MXFP4: blocks of 32 consecutive k, each 32 e2m1 elements and one E8M0 byte.  Every product runs on
// v_mfma_scale_f32_16x16x128_f8f6f4 with operand format e2m1 on the W side (A), e4m3 on the x side (B), the block's E8M0
// byte in the W-side scale register and unit scale on the x side:
//     y[m,n] = bf16( (sum_k xq[m,k] * e2m1[n,k] * 2^(s[n,k/32] - 127)) * x_scale[m] )
// No channel scale: the instruction applies the block scales, the epilogue applies the token's.
//
// Operand map (tools/mxfp4_probe.hip, tests/test_hip_mxfp4.py exact integers).  The instruction's own k index runs 0..127:
//   e2m1 operand: lane l holds k [32 (l >> 4), +32) of row l & 15 in registers 0..3 of the eight (4..7 are not read), element k = 2j
//                 in the low nibble of byte j; the block's scale is byte 0 (op_sel 0) of the lane's own scale register — one MX
//                 block per lane;
//   e4m3 operand: lane l holds k [16 (l >> 4), +16) in registers 0..3 and k [64 + 16 (l >> 4), +16) in registers 4..7.
// Two e4m3 operands may call a lane's 32 bytes "32 consecutive k" (fp8.hip does: both sides are permuted alike); next to an
// e2m1 operand the halves matter, so an x fragment here is the 16-B pieces kg and 4 + kg of the row's 128-B k-step, not 2kg, 2kg + 1.
//
// Physical layout (the header states it in words): weights are stored IN FRAGMENT ORDER.  Per group g of 16 rows and k-step
// ks of 128, 1 KiB of nibbles with lane l's 16 bytes at l * 16, and 64 scale bytes with lane l's at l.  So
//   - the streaming kernel's wave reads its W fragment as ONE contiguous 1-KiB request and its scales as one 64-B request:
//     no line -> fragment shuffle for W (fp8.hip needs DPP + ds_bpermute for it, and still does here for x);
//   - the tiled kernel's global_load_lds (LDS destination = wave base + lane * 16) lands a fragment block as it is read back:
//     ds_read_b128 of 64 consecutive 16-B pieces, conflict-free with NO swizzle.  The W stage is 8 blocks of 1 KiB (128 rows x
//     64 B); the x stage keeps fp8.hip's geometry (rows of 128 B, its swz()).
// Scales in the tiled kernel go through LDS: each wave copies the 4 x 64 scale bytes of ITS four W fragments per k-step with
// one 4-byte global_load_lds into a region of its own.  That keeps every request of a stage in the one counted vmcnt
// stream (7 per wave and stage) and needs no cross-wave ordering; direct global byte loads into registers would sit in the
// same in-order queue as the LDS-DMA requests and make the counted waits depend on where the compiler puts them.
//
//   gemm_mxfp4_kernel         128 x 128 x 128 tiles, 4 waves x (4 x 4) MFMA tiles, 2 or 4 LDS stages (fp8.hip's loop)
//   gemm_mxfp4_skinny_kernel  M <= 128: W streamed HBM -> VGPR once, K dealt over the 8 waves of a block, NG = 1 / 2 / 4
// Both fix one fp32 chain per output, independent of the row count (tiled: k ascending in one accumulator; streaming: each
// wave its k-steps ascending, waves added in order).
#include "common.h"
#include "gemm.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

namespace {

constexpr int UNIT_SCALE = 0x7F7F7F7F;   // four E8M0 bytes of 2^0
constexpr int MX_STREAM_MAX_ROWS = 128;

// A = W: e2m1 (format 4), 16 bytes in registers 0..3; B = x: e4m3 (format 0); ws: the E8M0 byte of the lane's block in byte 0
__device__ __forceinline__ f32x4 mfma_mx4(const i32x4& w, const i32x8& x, const f32x4& c, int ws) {
    const i32x8 a{w[0], w[1], w[2], w[3], 0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, x, c, 4 /* A e2m1 */, 0 /* B e4m3 */, 0, ws, 0, UNIT_SCALE);
}

struct Mx4Args {
    const uint8_t* x;      // [M, K] e4m3
    const uint8_t* w;      // [N/16][K/128][64][16] nibbles in fragment order
    const uint8_t* w2;     // SWIGLU: fc_2
    const uint8_t* ws;     // [N/16][K/128][64] E8M0 bytes in fragment order
    const uint8_t* ws2;
    bf16_t* y;             // [M, N]
    const float* xs;       // [M] activation scales
    const bf16_t* vec_a;   // ADAPTER scale [N]
    const bf16_t* vec_b;   // ADAPTER bias [N]
    const bf16_t* resid;   // [M, N] or null
    int M, N, K;
    int nb_n, nb_m;
    int gm;                // tiled kernel: m-tiles per band of the tile walk
};

// fp8.hip's rounding points: scale, round, epilogue
template <int EPI>
__device__ __forceinline__ float mx4_finish(float acc, float sc, const Mx4Args& a, int n) {
    float o = rbf(acc * sc);
    if (EPI == DH_EPI_ADAPTER) o = rbf(bf2f(a.vec_a[n]) * rbf(o + bf2f(a.vec_b[n])));
    return o;
}

// x tile: 128-B LDS rows, 16-B piece p of row r at piece position p ^ swz(r).  A fragment lane (row, kg) reads pieces kg and 4 + kg,
// so the lanes a ds_read_b128 services together (8 rows with kg = a, 8 with a + 1) ask for pieces that differ by 1: gemm.hip's
// swizzle, not fp8.hip's (built for pieces that differ by 2)
__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// ------------------------------------------------------------------------------ tiled kernel
constexpr int W_STAGE = 8 * 1024;       // 8 fragment blocks (16 rows x 128 k each)
constexpr int X_STAGE = 128 * 128;      // 128 rows of 128 e4m3
constexpr int S_STAGE = 4 * 256;        // per wave: the scale bytes of its four W fragments
constexpr int STAGE = W_STAGE + X_STAGE + S_STAGE;

template <int EPI, bool RESID, int NST>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_kernel(Mx4Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // NST x (W blocks, x tile, scales)
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
    const int nk = a.K >> 7, ngrp = a.N >> 4;

    // LDS slot s = 4 wn' + i holds fragment i of wave row wn': rows n0 + 64 wn' + 16 i (SWIGLU: i < 2 fc_1, else fc_2, rows
    // n0 + 32 wn' + 16 (i & 1)).  A group past N reads the last one; its outputs are not stored.
    auto slot_group = [&](int slot, bool& second) __attribute__((always_inline)) {
        const int swn = slot >> 2, i = slot & 3;
        int g;
        if (EPI == DH_EPI_SWIGLU) { second = i >= 2; g = (n0 >> 4) + swn * 2 + (i & 1); }
        else { second = false; g = (n0 >> 4) + slot; }
        return g < ngrp ? g : ngrp - 1;
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
    const uint8_t* srcX[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = (wave * 4 + j) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ swz(row);
        int m = m0 + row;
        m = m < a.M ? m : a.M - 1;
        srcX[j] = a.x + (size_t)m * a.K + chunk * 16;
    }
    auto stage = [&](int buf, int kt) {
        char* sW = smem + buf * STAGE;
        char* sX = sW + W_STAGE;
        char* sS = sX + X_STAGE + wave * 256;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(srcW[j] + (size_t)kt * 1024, sW + (wave * 2 + j) * 1024);
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(srcX[j] + (size_t)kt * 128, sX + (wave * 4 + j) * 1024);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcS + (size_t)kt * 64),
                                         (__attribute__((address_space(3))) void*)sS, 4, 0, 0);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, kg = lane >> 4;
    const int offB = (wm * 64 + frow) * 128;
    const int c0 = (kg ^ swz(frow)) << 4, c1 = ((4 + kg) ^ swz(frow)) << 4;      // k 16 kg.. and 64 + 16 kg.. of the k-step
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const char* sW = smem + buf * STAGE;
        const char* sX = sW + W_STAGE;
        const char* sS = sX + X_STAGE + wave * 256;
        i32x4 fa[4];
        int fs[4];
        i32x8 fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = *reinterpret_cast<const i32x4*>(sW + (wn * 4 + i) * 1024 + lane * 16);
            fs[i] = *reinterpret_cast<const uint8_t*>(sS + i * 64 + lane);
            const uint4 lo = *reinterpret_cast<const uint4*>(sX + offB + i * 2048 + c0);
            const uint4 hi = *reinterpret_cast<const uint4*>(sX + offB + i * 2048 + c1);
            fb[i] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma_mx4(fa[i], fb[j], acc[i][j], fs[i]);
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
        const float xs = a.xs[m];
        if (EPI == DH_EPI_SWIGLU) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int n = n0 + wn * 32 + i * 16 + 4 * kg;
                if (n >= a.N) continue;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = rbf(acc[i][j][e] * xs);
                    const float u = rbf(acc[i + 2][j][e] * xs);
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
                for (int e = 0; e < 4; ++e) o[e] = mx4_finish<EPI>(acc[i][j][e], xs, a, n + e);
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
// As gemm_fp8_skinny_kernel: one block = one group of 16 W rows (SWIGLU: of fc_1 and fc_2), K dealt round-robin in 128-wide
// k-steps over the 8 waves, the per-wave fp32 partials meet in LDS and thread t finishes output (n = t & 15, m = t >> 4).
// Per k-step a lane loads its 16 B of nibbles and its scale byte, both non-temporal (each byte is needed once); x still
// comes as full 128-B lines turned into fragments in registers (fp8.hip has the reason).
constexpr int ROWS = 16, NW = 8;

template <int EPI, bool RESID, bool OUT32 = false, int NG = 1>
__global__ __launch_bounds__(512, 2) void gemm_mxfp4_skinny_kernel(Mx4Args a) {
    constexpr bool SW = EPI == DH_EPI_SWIGLU;
    constexpr int CH = SW ? 2 : 4;                        // k-steps loaded ahead per wave
    __shared__ __attribute__((aligned(16))) float part[NW][32][ROWS];
    __shared__ __attribute__((aligned(16))) float part2[SW ? NW : 1][32][ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * ROWS;
    const int lrow = lane & 15, kg = lane >> 4;
    const int nks = a.K >> 7;
    const size_t gofs = (size_t)blockIdx.x * nks;          // the group's first fragment block
    const uint8_t* wl = a.w + gofs * 1024 + lane * 16;
    const uint8_t* sl = a.ws + gofs * 64 + lane;
    const uint8_t* wl2 = SW ? a.w2 + gofs * 1024 + lane * 16 : nullptr;
    const uint8_t* sl2 = SW ? a.ws2 + gofs * 64 + lane : nullptr;
    // x lines as in fp8.hip (request h: rows 8h..8h+7, lane -> row lane/8), but lane p of a row's eight takes piece p: fragment lane
    // (row, kg) then finds piece kg in the first merged register set and piece 4 + kg in the second (the e4m3 operand map above)
    const int lr8 = lane >> 3, pc = (lane & 7) * 16;
    const uint8_t* xl4[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            int row = g * 32 + h * 8 + lr8;
            row = row < a.M ? row : a.M - 1;
            xl4[g][h] = a.x + (size_t)row * a.K + pc;
        }
    const int fidx = ((lrow & 7) * 8 + kg + 4 * (lrow >> 3)) * 4;
    auto frag = [&](const i32x4& r0, const i32x4& r1) __attribute__((always_inline)) -> i32x8 {
        i32x8 f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int ev = __builtin_amdgcn_update_dpp(r0[d], r1[d], 0x114 /* row_shr:4 */, 0xF, 0xA /* lanes 4-7, 12-15 */, false);
            const int od = __builtin_amdgcn_update_dpp(r1[d], r0[d], 0x104 /* row_shl:4 */, 0xF, 0x5 /* lanes 0-3, 8-11 */, false);
            f[d] = __builtin_amdgcn_ds_bpermute(fidx, ev);
            f[4 + d] = __builtin_amdgcn_ds_bpermute(fidx, od);
        }
        return f;
    };
    auto ldnt = [](const uint8_t* p) __attribute__((always_inline)) { return __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(p)); };
    auto ldsc = [](const uint8_t* p) __attribute__((always_inline)) { return (int)__builtin_nontemporal_load(p); };
    auto ld = [](const uint8_t* p) __attribute__((always_inline)) { return *reinterpret_cast<const i32x4*>(p); };
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
            i32x4 xr[CH][4];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ks = ks0 + c * NW;
                if (ks < nks) {
#pragma unroll
                    for (int h = 0; h < 4; ++h) xr[c][h] = ld(xl4[g][h] + (size_t)ks * 128);
                }
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int ks = ks0 + c * NW;
                if (ks < nks) {
                    const i32x8 xl = frag(xr[c][0], xr[c][1]), xh = frag(xr[c][2], xr[c][3]);
                    acc_lo[g] = mfma_mx4(wr[c], xl, acc_lo[g], sc[c]);
                    acc_hi[g] = mfma_mx4(wr[c], xh, acc_hi[g], sc[c]);
                    if (SW) {
                        acc2_lo[g] = mfma_mx4(wr2[c], xl, acc2_lo[g], sc2[c]);
                        acc2_hi[g] = mfma_mx4(wr2[c], xh, acc2_hi[g], sc2[c]);
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
        const float xs = a.xs[tm];
        float o;
        if (SW) {
            float gt = 0.f, u = 0.f;
            const float* p2 = &part2[0][0][0] + tmi * ROWS + tn;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                gt += p[w * 32 * ROWS];
                u += p2[w * 32 * ROWS];
            }
            gt = rbf(gt * xs);
            u = rbf(u * xs);
            o = rbf(silu_fast(gt)) * u;
        } else {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) s += p[w * 32 * ROWS];
            o = mx4_finish<EPI>(s, xs, a, nn);
            if (RESID) o = bf2f(a.resid[(size_t)tm * a.N + nn]) + o;
        }
        if (OUT32) reinterpret_cast<float*>(a.y)[(size_t)tm * a.N + nn] = o;     // bf16-exact value as fp32 (fused decode consumer)
        else a.y[(size_t)tm * a.N + nn] = f2bf(o);
    }
}

template <int EPI, bool RESID, int NST>
int launch_tiled_n(const Mx4Args& a, hipStream_t s) {
    constexpr int lds = NST * STAGE;
    DH_MAX_LDS_ONCE((gemm_mxfp4_kernel<EPI, RESID, NST>), lds);
    hipLaunchKernelGGL((gemm_mxfp4_kernel<EPI, RESID, NST>), dim3(a.nb_n * a.nb_m), dim3(256), lds, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(NST == 4 ? DH_ROUTE_MX4_T128_S4 : DH_ROUTE_MX4_T128_S2);
    return 0;
}

template <int EPI>
int launch_tiled(Mx4Args a, hipStream_t s) {
    a.gm = 4;
    // as fp8.hip: grids smaller than the chip walk K alone -> 4 stages, one block per CU; else 2 stages, two blocks
    if (a.nb_n * a.nb_m < 384) return a.resid ? launch_tiled_n<EPI, true, 4>(a, s) : launch_tiled_n<EPI, false, 4>(a, s);
    return a.resid ? launch_tiled_n<EPI, true, 2>(a, s) : launch_tiled_n<EPI, false, 2>(a, s);
}

template <int EPI, int NG>
int launch_skinny_ng(const Mx4Args& a, hipStream_t s) {
    dim3 grid(a.N / ROWS), block(512);
    if (a.resid) hipLaunchKernelGGL((gemm_mxfp4_skinny_kernel<EPI, true, false, NG>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_mxfp4_skinny_kernel<EPI, false, false, NG>), grid, block, 0, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(NG == 1 ? DH_ROUTE_MX4_STREAM_NG1 : NG == 2 ? DH_ROUTE_MX4_STREAM_NG2 : DH_ROUTE_MX4_STREAM_NG4);
    return 0;
}

template <int EPI>
int launch_skinny(const Mx4Args& a, hipStream_t s) {
    if (a.M <= 32) return launch_skinny_ng<EPI, 1>(a, s);
    if (a.M <= 64) return launch_skinny_ng<EPI, 2>(a, s);
    return launch_skinny_ng<EPI, 4>(a, s);
}

}  // namespace

extern "C" int dh_linear_mxfp4_f32(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const uint8_t* w_scale, float* y32,
                                   int M, int N, int K, void* stream) {
    DH_CHECK(xq && x_scale && wq && w_scale && y32, "dh_linear_mxfp4_f32: null operand");
    DH_CHECK(M >= 1 && M <= MX_STREAM_MAX_ROWS && N > 0 && N % 16 == 0 && K > 0 && K % 128 == 0,
             "dh_linear_mxfp4_f32: needs 1 <= M <= %d, N %% 16 == 0 and K %% 128 == 0 (M=%d N=%d K=%d)", MX_STREAM_MAX_ROWS, M, N, K);
    Mx4Args a{xq, wq, nullptr, w_scale, nullptr, reinterpret_cast<bf16_t*>(y32), x_scale, nullptr, nullptr, nullptr, M, N, K, 0, 0, 1};
    dim3 grid(N / ROWS), block(512);
    hipStream_t s = (hipStream_t)stream;
    // row groups as launch_skinny: the same kernel (and bits) as dh_linear_mxfp4_ex's streaming form, fp32 store
    if (M <= 32) hipLaunchKernelGGL((gemm_mxfp4_skinny_kernel<DH_EPI_PLAIN, false, true, 1>), grid, block, 0, s, a);
    else if (M <= 64) hipLaunchKernelGGL((gemm_mxfp4_skinny_kernel<DH_EPI_PLAIN, false, true, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((gemm_mxfp4_skinny_kernel<DH_EPI_PLAIN, false, true, 4>), grid, block, 0, s, a);
    DH_LAUNCH_CHECK();
    dh_gemm_route(M <= 32 ? DH_ROUTE_MX4_STREAM_NG1 : M <= 64 ? DH_ROUTE_MX4_STREAM_NG2 : DH_ROUTE_MX4_STREAM_NG4);
    return 0;
}

// kernel: 0 = by row count (streaming up to 128 rows, tiled above), 1 = tiled, 2 = streaming — dh_linear_fp8_ex's selector
extern "C" int dh_linear_mxfp4_ex(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const uint8_t* w_scale, dh_bf16* y,
                                  int M, int N, int K, int epilogue, const uint8_t* w2q, const uint8_t* w2_scale,
                                  const dh_bf16* vec_a, const dh_bf16* vec_b, const dh_bf16* resid, int kernel, void* stream) {
    DH_CHECK(xq && x_scale && wq && w_scale && y, "dh_linear_mxfp4: null operand");
    DH_CHECK(kernel >= 0 && kernel <= 2, "dh_linear_mxfp4: kernel %d (0 auto, 1 tiled, 2 streaming)", kernel);
    DH_CHECK(kernel != 2 || M <= MX_STREAM_MAX_ROWS, "dh_linear_mxfp4: the streaming kernel takes at most %d rows (M=%d)", MX_STREAM_MAX_ROWS, M);
    DH_CHECK(M >= 0 && N > 0 && K > 0 && K % 128 == 0 && N % 16 == 0, "dh_linear_mxfp4: bad shape M=%d N=%d K=%d (K %% 128, N %% 16 must be 0)", M, N, K);
    DH_CHECK(epilogue == DH_EPI_PLAIN || epilogue == DH_EPI_SWIGLU || epilogue == DH_EPI_ADAPTER,
             "dh_linear_mxfp4: epilogue %d unsupported (LoRA is merged before quantisation)", epilogue);
    DH_CHECK(epilogue != DH_EPI_SWIGLU || (w2q && w2_scale && !resid), "dh_linear_mxfp4: SWIGLU needs w2/w2_scale and takes no residual");
    DH_CHECK(epilogue != DH_EPI_ADAPTER || (vec_a && vec_b), "dh_linear_mxfp4: ADAPTER needs scale/bias vectors");
    if (M == 0) return 0;
    Mx4Args a{xq, wq, w2q, w_scale, w2_scale, y, x_scale, vec_a, vec_b, resid, M, N, K, 0, 0, 1};
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
