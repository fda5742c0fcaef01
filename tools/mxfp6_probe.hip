// Operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m3 operand next to an e2m1 one (whose map tools/mxfp4_probe.hip
// fixed: lane l, register g < 4, nibble i is k = 32 (l >> 4) + 8 g + i), found with exact one-hot data, for both operand
// positions: which bit of which register of a lane's eight stands for which k and which bit of the six-bit code, that
// registers 6..7 are not read, and which k block a lane's scale byte scales.  One wave; every probe is one MFMA with a single
// 1.0 in the e2m1 operand and a single bit in the e2m3 one, and a look at the one output that can move.  A third part times
// MFMA-only loops of four operand pairs (e4m3 x e4m3, e2m1 x e4m3, e2m1 x e2m3, e2m1 x e2m1) on the whole chip.
// hipcc --offload-arch=gfx950 -O3 tools/mxfp6_probe.hip -o tools/bin/mxfp6_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int UNIT = 0x7F7F7F7F;          // four E8M0 bytes of 2^0
constexpr int ONE_E2M1 = 2;

// POS 0: e2m3 is the B operand (column pl & 15 of C, seen at row 0); POS 1: e2m3 is the A operand (row pl & 15, seen at column 0)
template <int POS>
__device__ f32x4 mfma_pair(const i32x8& f6, const i32x8& f4, int s6) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (POS == 0) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f4, f6, z, 4 /* A e2m1 */, 2 /* B e2m3 */, 0, UNIT, 0, s6);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f6, f4, z, 2 /* A e2m3 */, 4 /* B e2m1 */, 0, s6, 0, UNIT);
}

// C[row][col]: lane 16 (row / 4) + col, register row % 4
__device__ float c_at(const f32x4& c, int row, int col) {
    float v = 0.f;
    for (int r = 0; r < 4; ++r) if (r == (row & 3)) v = c[r];
    return __shfl(v, 16 * (row >> 2) + col, 64);
}

// kout[pl * 256 + p], vout[pl * 256 + p]: the k (0..127) of the e2m1 1.0 that bit p (register p / 32, bit p % 32) of lane pl's
// e2m3 operand meets, and the product; k = -1 none (sign bits alone, or a register that is not read), -2 more than one
template <int POS>
__global__ void probe_bits(int* kout, float* vout) {
    const int lane = threadIdx.x;
    for (int pl = 0; pl < 64; ++pl)
        for (int p = 0; p < 256; ++p) {
            i32x8 f6 = {0, 0, 0, 0, 0, 0, 0, 0};
            if (lane == pl) f6[p >> 5] = 1 << (p & 31);
            int found = -1;
            float val = 0.f;
            for (int cand = 0; cand < 128; ++cand) {
                i32x8 f4 = {0, 0, 0, 0, 0, 0, 0, 0};
                if (lane == 16 * (cand >> 5)) f4[(cand >> 3) & 3] = ONE_E2M1 << (4 * (cand & 7));
                const f32x4 c = mfma_pair<POS>(f6, f4, UNIT);
                const float v = POS == 0 ? c_at(c, 0, pl & 15) : c_at(c, pl & 15, 0);
                if (v != 0.f) { found = found == -1 ? cand : -2; val = v; }
            }
            if (lane == 0) { kout[pl * 256 + p] = found; vout[pl * 256 + p] = val; }
        }
}

// sign: sout[pl * 32 + i] = the product when bits 6 i + 3 (1.0) and 6 i + 5 (sign) of lane pl are set and the e2m1 side is all ones
// in every k: -1 expected.  scale: bout[pl * 4 + byte] = the k block (0..3) whose products double when that byte of lane pl's own
// e2m3-side scale register is 2^1 (op_sel 0); -1 none
template <int POS>
__global__ void probe_sign_scale(float* sout, int* bout) {
    const int lane = threadIdx.x;
    i32x8 ones4 = {0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};
    for (int pl = 0; pl < 64; ++pl)
        for (int i = 0; i < 32; ++i) {
            i32x8 f6 = {0, 0, 0, 0, 0, 0, 0, 0};
            if (lane == pl) {
                const int b0 = 6 * i + 3, b1 = 6 * i + 5;
                f6[b0 >> 5] |= 1 << (b0 & 31);
                f6[b1 >> 5] |= 1 << (b1 & 31);
            }
            const f32x4 c = mfma_pair<POS>(f6, ones4, UNIT);
            const float v = POS == 0 ? c_at(c, 0, pl & 15) : c_at(c, pl & 15, 0);
            if (lane == 0) sout[pl * 32 + i] = v;
        }
    // every e2m3 element 1.0: bit 6 i + 3 of the 192
    i32x8 ones6 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 32; ++i) ones6[(6 * i + 3) >> 5] |= 1 << ((6 * i + 3) & 31);
    for (int pl = 0; pl < 64; ++pl)
        for (int byte = 0; byte < 4; ++byte) {
            int found = -1;
            for (int q = 0; q < 4; ++q) {
                i32x8 f4 = {0, 0, 0, 0, 0, 0, 0, 0};
                if ((lane >> 4) == q) f4 = ones4;                                    // ones in k block q only
                const int sc = lane == pl ? (int)(0x7F7F7F7Fu + (1u << (8 * byte))) : UNIT;
                const f32x4 c = mfma_pair<POS>(ones6, f4, sc);
                const float v = POS == 0 ? c_at(c, 0, pl & 15) : c_at(c, pl & 15, 0);
                if (v == 64.f) found = q;                                            // 32 products of 1 * 1, doubled
            }
            if (lane == 0) bout[pl * 4 + byte] = found;
        }
}

// MFMA-only loop: 4 waves per block, 8 independent accumulators per wave, iters x 8 instructions.  The instruction is written in
// assembly with the accumulator in place: through the builtin the compiler gives the narrow operand pairs a destination that
// overlaps the source accumulator two registers off and fills the loop with register copies, which then is what gets timed.
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(6))) int i32x6;
template <int FA, int FB> struct Rate;
#define RATE_PAIR(FA, FB, TA, TB, MODS)                                                                                          \
    template <> struct Rate<FA, FB> {                                                                                            \
        static __device__ __forceinline__ void loop(f32x4 (&acc)[8], int seed, int iters) {                                     \
            TA a;                                                                                                                \
            TB b;                                                                                                                \
            for (int r = 0; r < (int)(sizeof(TA) / 4); ++r) a[r] = r == 0 ? seed : 0;                                            \
            for (int r = 0; r < (int)(sizeof(TB) / 4); ++r) b[r] = 0;                                                            \
            const int unit = UNIT;                                                                                               \
            for (int it = 0; it < iters; ++it)                                                                                   \
                _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                                   \
                    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %3 op_sel_hi:[0,0,0]" MODS              \
                                 : "+v"(acc[j]) : "v"(a), "v"(b), "v"(unit));                                                    \
            asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   /* the last results, before anything reads them */             \
        }                                                                                                                        \
    };
RATE_PAIR(0, 0, i32x8, i32x8, "")
RATE_PAIR(4, 0, i32x4, i32x8, " cbsz:4")
RATE_PAIR(4, 2, i32x4, i32x6, " cbsz:4 blgp:2")
RATE_PAIR(4, 4, i32x4, i32x4, " cbsz:4 blgp:4")

template <int FA, int FB>
__global__ __launch_bounds__(256) void mfma_rate(float* out, int iters) {
    f32x4 acc[8];
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    Rate<FA, FB>::loop(acc, threadIdx.x & 1, iters);
    float s = 0.f;
    for (int j = 0; j < 8; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
    if (s == 12345.f) out[0] = s;
}

template <int FA, int FB>
static int time_pair(const char* name, float* dout) {
    const int blocks = 256 * 4, iters = 512;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 2;
    hipLaunchKernelGGL((mfma_rate<FA, FB>), dim3(blocks), dim3(256), 0, 0, dout, 64);       // warm
    float best = 1e30f, worst = 0.f;
    for (int rep = 0; rep < 5; ++rep) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL((mfma_rate<FA, FB>), dim3(blocks), dim3(256), 0, 0, dout, iters);
        hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess) return 2;
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        best = ms < best ? ms : best;
        worst = ms > worst ? ms : worst;
    }
    const double flop = 2.0 * 16 * 16 * 128 * 8.0 * iters * 4.0 * blocks;
    printf("mfma rate %-14s  %8.3f .. %8.3f ms   %7.1f TFLOP/s at the fastest of 5\n", name, best, worst, flop / (best * 1e-3) * 1e-12);
    return 0;
}

template <int POS>
static int run_map(const char* name) {
    int *dk, *db;
    float *dv, *dsg;
    if (hipMalloc(&dk, 64 * 256 * 4) != hipSuccess || hipMalloc(&dv, 64 * 256 * 4) != hipSuccess ||
        hipMalloc(&dsg, 64 * 32 * 4) != hipSuccess || hipMalloc(&db, 64 * 4 * 4) != hipSuccess) return -1;
    if (hipMemset(dk, 0xff, 64 * 256 * 4) != hipSuccess || hipMemset(db, 0xff, 64 * 4 * 4) != hipSuccess) return -1;
    hipLaunchKernelGGL((probe_bits<POS>), dim3(1), dim3(64), 0, 0, dk, dv);
    hipLaunchKernelGGL((probe_sign_scale<POS>), dim3(1), dim3(64), 0, 0, dsg, db);
    if (hipDeviceSynchronize() != hipSuccess) { printf("probe failed to run\n"); return -1; }
    static int hk[64 * 256], hb[64 * 4];
    static float hv[64 * 256], hsg[64 * 32];
    if (hipMemcpy(hk, dk, sizeof(hk), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hv, dv, sizeof(hv), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hsg, dsg, sizeof(hsg), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hb, db, sizeof(hb), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    // The map csrc/mxfp6.hip relies on: lane l's element i (0..31) is k = 32 (l >> 4) + i of row / column l & 15, its six-bit code
    // at bits 6 i .. 6 i + 5 of the lane's first 192 bits (registers 0..5, little endian); registers 6..7 are not read; scale byte 0
    // of lane l scales exactly that lane's 32 k.
    static const float bitval[6] = {0.125f, 0.25f, 0.5f, 1.f, 2.f, 0.f};
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int p = 0; p < 256; ++p) {
            int wk = -1;
            float wv = 0.f;
            if (p < 192 && p % 6 != 5) { wk = 32 * (l >> 4) + p / 6; wv = bitval[p % 6]; }
            if ((hk[l * 256 + p] != wk || hv[l * 256 + p] != wv) && bad++ < 16)
                printf("%s lane %d bit %d: k %d value %g (expected k %d value %g)\n", name, l, p, hk[l * 256 + p], hv[l * 256 + p], wk, wv);
        }
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < 32; ++i)
            if (hsg[l * 32 + i] != -1.f && bad++ < 32) printf("%s lane %d element %d with the sign bit: %g (expected -1)\n", name, l, i, hsg[l * 32 + i]);
    for (int l = 0; l < 64; ++l)
        for (int b = 0; b < 4; ++b) {
            const int want = b == 0 ? (l >> 4) : -1;
            if (hb[l * 4 + b] != want && bad++ < 48) printf("%s scale lane %d byte %d: k block %d (expected %d)\n", name, l, b, hb[l * 4 + b], want);
        }
    printf("%s lane 17, bits 0..11 -> k:value", name);
    for (int p = 0; p < 12; ++p) printf(" %d:%g", hk[17 * 256 + p], hv[17 * 256 + p]);
    printf("\n%s lane 17, bits 186..197 -> k:value", name);
    for (int p = 186; p < 198; ++p) printf(" %d:%g", hk[17 * 256 + p], hv[17 * 256 + p]);
    printf("\n%s scale bytes of lane 17 -> k block %d %d %d %d\n", name, hb[68], hb[69], hb[70], hb[71]);
    printf("mxfp6 operand map, %s: %d entries differ from the map csrc/mxfp6.hip relies on\n", name, bad);
    hipFree(dk); hipFree(dv); hipFree(dsg); hipFree(db);
    return bad;
}

int main() {
    const int b0 = run_map<0>("e2m3 as B");
    const int b1 = run_map<1>("e2m3 as A");
    if (b0 < 0 || b1 < 0) return 2;
    float* dout;
    if (hipMalloc(&dout, 4) != hipSuccess) return 2;
    // arms alternate, twice over
    for (int round = 0; round < 2; ++round) {
        if (time_pair<0, 0>("e4m3 x e4m3", dout) || time_pair<4, 0>("e2m1 x e4m3", dout) || time_pair<4, 2>("e2m1 x e2m3", dout) ||
            time_pair<4, 4>("e2m1 x e2m1", dout)) return 2;
    }
    return (b0 || b1) ? 1 : 0;
}
