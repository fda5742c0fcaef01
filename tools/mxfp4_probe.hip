// Operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with an e2m1 A operand and an e4m3 B operand, found with exact one-hot data:
// which A registers are read, which e4m3 byte of B each e2m1 nibble of A meets (the k index both stand for), and which row and
// MX block a lane's scale byte scales.  One wave; every probe is one MFMA with a single 1.0 in A and a single 1.0 in B (or all
// ones and one scale byte of 2^1) and a look at the one output that can move.
// hipcc --offload-arch=gfx950 -O3 tools/mxfp4_probe.hip -o tools/bin/mxfp4_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
constexpr int UNIT = 0x7F7F7F7F;          // four E8M0 bytes of 2^0
constexpr int ONE_E2M1 = 2, ONE_E4M3 = 0x38;

// C[row][column 0] of a 16x16 accumulator: lane 16 (row / 4), register row % 4
__device__ float c_row_col0(const f32x4& c, int row) {
    float v = 0.f;
    for (int r = 0; r < 4; ++r) if (r == (row & 3)) v = c[r];
    return __shfl(v, 16 * (row >> 2), 64);
}

// out[pl * 64 + 8 g + i]: the B position (32 kgb + 4 rb + jb: lane 16 kgb = column 0, register rb, byte jb) whose 1.0 meets the 1.0 in
// nibble i of register g of A's lane pl; -1 none (the register is not read), -2 more than one
__global__ void probe_pairs(int* out) {
    const int lane = threadIdx.x;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int pl = 0; pl < 64; ++pl)
        for (int gi = 0; gi < 64; ++gi) {
            i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
            if (lane == pl) a[gi >> 3] = ONE_E2M1 << (4 * (gi & 7));
            int found = -1;
            for (int cand = 0; cand < 128; ++cand) {
                i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
                if (lane == 16 * (cand >> 5)) b[(cand >> 2) & 7] = ONE_E4M3 << (8 * (cand & 3));
                const f32x4 c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 4 /* A e2m1 */, 0 /* B e4m3 */, 0, UNIT, 0, UNIT);
                if (c_row_col0(c, pl & 15) != 0.f) found = found == -1 ? cand : -2;
            }
            if (lane == 0) out[pl * 64 + gi] = found;
        }
}

// out[pl * 4 + byte]: the instruction's 32-wide k block (0..3) of row pl & 15 whose products double when that byte of lane pl's A-side
// scale register is 2^1 (op_sel 0); -1 none
__global__ void probe_scale(int* out) {
    const int lane = threadIdx.x;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    i32x8 a;
    for (int r = 0; r < 8; ++r) a[r] = 0x22222222;                                   // every element 1.0
    for (int pl = 0; pl < 64; ++pl)
        for (int byte = 0; byte < 4; ++byte) {
            int found = -1;
            for (int q = 0; q < 4; ++q) {
                // ones in block q of the instruction's k index: e4m3 lanes 16 kgb.. hold k 16 kgb..+16 (registers 0..3) and 64 + 16 kgb..
                i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
                if (((lane >> 4) >> 1) == (q & 1))
                    for (int r = 0; r < 4; ++r) b[4 * (q >> 1) + r] = 0x38383838;
                const int sc = lane == pl ? (int)(0x7F7F7F7Fu + (1u << (8 * byte))) : UNIT;
                const f32x4 c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, z, 4, 0, 0, sc, 0, UNIT);
                if (c_row_col0(c, pl & 15) == 64.f) found = q;                       // 32 products of 1 * 1, doubled
            }
            if (lane == 0) out[pl * 4 + byte] = found;
        }
}

int main() {
    int *dp, *ds;
    if (hipMalloc(&dp, 64 * 64 * 4) != hipSuccess || hipMalloc(&ds, 64 * 4 * 4) != hipSuccess) return 2;
    if (hipMemset(dp, 0xff, 64 * 64 * 4) != hipSuccess || hipMemset(ds, 0xff, 64 * 4 * 4) != hipSuccess) return 2;
    hipLaunchKernelGGL(probe_pairs, dim3(1), dim3(64), 0, 0, dp);
    hipLaunchKernelGGL(probe_scale, dim3(1), dim3(64), 0, 0, ds);
    if (hipDeviceSynchronize() != hipSuccess) { printf("probe failed to run\n"); return 2; }
    static int hp[64 * 64], hs[64 * 4];
    if (hipMemcpy(hp, dp, sizeof(hp), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hs, ds, sizeof(hs), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    // The map csrc/mxfp4.hip relies on.  With k the instruction's own index 0..127:
    //   e2m1: registers 0..3 only; lane l, register g, nibble i is k = 32 (l >> 4) + 8 g + i of row l & 15;
    //   e4m3: lane l, byte j < 16 is k = 16 (l >> 4) + j, byte j >= 16 is k = 64 + 16 (l >> 4) + j - 16;
    //   scale byte 0 of lane l scales row l & 15, k block l >> 4; bytes 1..3 are not used with op_sel 0.
    int bad = 0;
    for (int l = 0; l < 64; ++l)
        for (int gi = 0; gi < 64; ++gi) {
            int want = -1;
            if (gi < 32) {
                const int k = 32 * (l >> 4) + gi;
                want = k < 64 ? 32 * (k >> 4) + (k & 15) : 32 * ((k - 64) >> 4) + 16 + (k & 15);
            }
            if (hp[l * 64 + gi] != want && bad++ < 16)
                printf("A lane %d reg %d nibble %d meets B position %d (expected %d)\n", l, gi >> 3, gi & 7, hp[l * 64 + gi], want);
        }
    for (int l = 0; l < 64; ++l)
        for (int b = 0; b < 4; ++b) {
            const int want = b == 0 ? (l >> 4) : -1;
            if (hs[l * 4 + b] != want && bad++ < 32) printf("scale lane %d byte %d: k block %d (expected %d)\n", l, b, hs[l * 4 + b], want);
        }
    printf("A lane 17, nibbles 0..31 meet B (lane / 16 : byte):");
    for (int gi = 0; gi < 32; ++gi) printf(" %d:%d", hp[17 * 64 + gi] >> 5, hp[17 * 64 + gi] & 31);
    printf("\nA lane 17, registers 4..7: %d %d %d %d (-1: not read);  scale bytes of lane 17 -> k block %d %d %d %d\n", hp[17 * 64 + 32], hp[17 * 64 + 40],
           hp[17 * 64 + 48], hp[17 * 64 + 56], hs[68], hs[69], hs[70], hs[71]);
    printf("mxfp4 operand map: %d entries differ from the map csrc/mxfp4.hip relies on\n", bad);
    return bad ? 1 : 0;
}
