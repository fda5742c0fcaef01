// Causal GQA attention against the compact KV cache (ger/model.py:261,270-290).
//
// Layout chosen for the MFMA operand maps, not inherited from the reference: both caches are stored
// in MFMA-FRAGMENT ORDER (common.h kfrag_off / vfrag_off): per (slot, group) a sequence of 32-key
// tiles, each tile a run of 1-KiB blocks that are, byte for byte, the A-operand fragments of
//   S^T = K . Q^T   (block (ks): lane i holds K[key i&31][16ks + 8(i>>5) .. +8])
//   O^T = V^T . P^T (block (dt,s2): lane i holds V[8 permuted keys][d = 32dt + (i&31)])
// so a decode wave streams a tile as 8 fully coalesced 1-KiB loads straight into MFMA operands,
// and the prefill kernel copies tiles linearly into LDS and reads them back lane-linear
// (conflict-free ds_read_b128, no swizzle).
// Both products keep the QUERY on the accumulator's lane axis:
//   S^T[key][q] = K · Q^T      A = K rows (16 B of a key row),  B = Q rows (16 B of a q row)
//   O^T[d][q]   = V^T · P^T    A = V^T rows (keys contiguous),  B = the S^T accumulator itself,
//                              converted to bf16 in registers (cdna_hip_programming.md §3
//                              "an accumulator tile as the next MFMA's operand": k-slot j of
//                              lane-half h is key 16s + 8(j>>2) + 4h + (j&3), so the V^T
//                              fragment is two 8-byte runs of 4 keys).
// so the online-softmax statistics (running max m, running sum l) are one scalar per lane, the
// rescale of O is a per-lane multiply, and P never touches LDS.  Softmax is fp32; P is rounded
// to bf16 for the second product; O/l is rounded to bf16 once (as the reference's fused CPU/GPU
// SDPA kernels do).
#include "common.h"
#include "tuning.h"

#ifdef DH_PREFILL_STAMPS   // diagnostic build only (tools/probe_attn_prefill.py): 100 MHz timestamps of lane 0 of wave 0 of each block
// per block 40 slots: 0 entry, 1 metadata read, 2 Q fragments in registers, 3 first stage landed (barrier 0), then for key step
// kt < 8 at 4 + 4 kt: S MFMAs issued, softmax done, last PV issued, barrier passed; 36 last store issued; 37 the wave's HW_ID
// register (bits 8-15: CU, shader array, shader engine), 38 its XCC_ID: which CU the block ran on; 39 its query tile.  Vector
// stores only.
constexpr int PF_STAMP_BLOCKS = 16384, PF_STAMP_SLOTS = 40, PF_STAMP_STEPS = 8;
__device__ unsigned long long g_prefill_stamps[PF_STAMP_BLOCKS * PF_STAMP_SLOTS];
#define PF_STAMP(i)                                                                                                        \
    do {                                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
        if (threadIdx.x == 0 && pf_blk < PF_STAMP_BLOCKS) g_prefill_stamps[pf_blk * PF_STAMP_SLOTS + (i)] = __builtin_amdgcn_s_memrealtime(); \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
    } while (0)
#define PF_STAMP_STEP(kt, j) do { if ((kt) < PF_STAMP_STEPS) PF_STAMP(4 + 4 * (kt) + (j)); } while (0)
#define PF_HAVE(...) asm volatile("" ::__VA_ARGS__)     // the stamp that follows is taken once these values have arrived
extern "C" int dh_debug_prefill_stamps(unsigned long long* out, int clear) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prefill_stamps), sizeof(g_prefill_stamps)) != hipSuccess) return 1;
    if (!clear) return 0;
    void* p = nullptr;
    return hipGetSymbolAddress(&p, HIP_SYMBOL(g_prefill_stamps)) == hipSuccess && hipMemset(p, 0, sizeof(g_prefill_stamps)) == hipSuccess ? 0 : 1;
}
#else
#define PF_STAMP(i)
#define PF_STAMP_STEP(kt, j)
#define PF_HAVE(...)
#endif

// dh_set_tuning 42: waves per block of the prefill attention at head sizes 64 and 128 (0: all q_per_kv heads of a KV group in one
// block, 2 | 4: that many, a group's K / V^T stages copied by q_per_kv / WPB blocks).  Same bits on every arm.  Read at launch.
int g_prefill_wpb = 4;

namespace {

// ------------------------------------------------------------------------------------ prefill
// grid (q tiles of 32, n_groups * (q_per_kv / WPB), n_seq); block = 64 * WPB threads: one wave per query head, the WPB heads
// head = g * q_per_kv + part * WPB + wave of a block share the K / V^T tiles of 64 keys staged in LDS and meet at one barrier per
// key step.  WPB 0: all q_per_kv heads of the group in one block (block size from the launch).  Head size 96 (Phi-3.5,
// multi-head: q_per_kv 1) runs one wave per block: 48 KiB of stages, three blocks per CU by LDS.
// PS: scale is a power of two (head size 64: 1/8), so it is applied to the Q fragments once — exact in bf16 and in the
// fp32 products and sums (barring underflow) — instead of to every score: the loop is bound by its softmax VALU work.
// The register budget follows the waves a SIMD can hold by LDS (160 KiB per CU): 32-KiB blocks at head size 64 are five per CU, so
// four waves per SIMD (128 VGPRs) from four-wave blocks on, as the 16-wave block always had, and two from two-wave blocks; the
// 64-KiB blocks of head size 128 are two per CU.  Without the second argument a small block is handed registers that cost residency.
constexpr int pf_waves_per_simd(int hs, int wpb) { return hs == 64 ? (wpb == 2 ? 2 : 4) : (wpb == 2 ? 1 : 2); }

template <int HS, bool PS, int WPB>
__global__ __launch_bounds__(WPB ? 64 * WPB : HS == 64 ? 1024 : 512, pf_waves_per_simd(HS, WPB)) void attn_prefill_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_cache, const bf16_t* __restrict__ vT_cache,
    const int32_t* __restrict__ seq_slot, const int32_t* __restrict__ q_start, const int32_t* __restrict__ q_len,
    const int32_t* __restrict__ kv_pos0, bf16_t* __restrict__ y, float* __restrict__ lse, int n_head, int n_groups,
    int s_max, float scale) {
    constexpr int KS = HS / 16;   // k-steps of the QK product
    constexpr int DT = HS / 32;   // 32-row tiles of O^T
    constexpr int TILE_B = HS * 32 * 2;   // bytes of one 32-key tile of K (and of V^T)
    // two stages of (two 32-key tiles of K, two of V^T): the tiles of step kt+1 are DMA'd (global_load_lds; the
    // cache is already in fragment order, so the copy is linear) while step kt is multiplied
    // (Round 3, measured and not kept: FOUR stages at head size 64, DMA three steps ahead with counted waits — 217 us per launch against
    //  209: the 40 % of wave cycles parked at waits (tools/pmc_attn_prefill.py: SQ_WAIT_ANY 100.6 M of 251 M) are not DMA latency.
    //  Nor are they instruction count or phase lock-step, as far as two more experiments go: the subtraction and the log2 e
    //  multiplication of the softmax on packed pairs (24 fewer VALU instructions per step) 207-210 us; S of step kt+1 issued in front
    //  of the softmax of step kt (software pipelining inside the wave, bit-identical, one more S tile: 163 VGPRs = one block per
    //  CU 284 us, forced to 128 with 17 spills 277 us).  Round 4: all eight K fragments of a step read in one batch in front of the
    //  eight S MFMAs and the eight V^T fragments in front of the PV MFMAs (sched_barrier; 128 VGPRs, 5 spilled): 200-209 us against 200-203,
    //  tools/time_attn_prefill.py — the operand reads' LDS latency is not it either.
    //  Then the block's life was stamped (-DDH_PREFILL_STAMPS, tools/probe_attn_prefill.py, profiles/prefill_attn_stamps_*.txt) and
    //  the waits turned out to be CUs without work: a CU got one tile index for all its blocks (the comment at qt below), 8 key
    //  steps per block on some CUs and 1 on others, 57 of 209 us with no block at all on the median CU.  With the tile order rotated
    //  and folded the launch is 146 us with the group's 8 heads in one block, 139 us with 4 waves per block (WPB, the default: the
    //  stage is copied twice per group, but the barrier holds 4 waves, not 8, and a CU holds four blocks in four phases) and 168 us
    //  with 2 (five blocks per CU by LDS, four copies of the stage); tools/ab_attn_prefill.py, spreads 1.0-1.3 us; head size 128 at
    //  32 x 1536 tokens, 4 heads per group: 866 / 824 / 1277 us.  On top of the 4-wave blocks the packed subtraction and log2 e
    //  product of round 3 were measured again: 139.2-139.3 us against 139.3, not kept.)
    __shared__ __attribute__((aligned(16))) char sKV[2][4 * TILE_B];

    const int q_per_kv = n_head / n_groups;
    const int parts = WPB ? q_per_kv / WPB : 1;         // blocks per KV group
    const int seq = blockIdx.z, g = blockIdx.y / parts, part = blockIdx.y % parts;
    // Query tile of block x: x is rotated by the block's row (y, z) and then folded, so that the first half of the grid's x walks
    // the tiles down from the last (longest) one and the second half up from tile 0.  Workgroups go to the chip's 8 XCDs round
    // robin by linear id, and inside an XCD to its 32 CUs round robin again: blocks 256 ids apart share a CU.  With x reversed
    // only (as it was) and 16 tiles, XCD k got the tiles 15 - k and 7 - k of every 512-token sequence, and a CU got ONE tile
    // index for all its blocks: 8 key steps per block on some CUs, 1 on others, and the launch lasted as long as the former
    // (tools/probe_attn_prefill.py).  The fold gives x and x + 8, one XCD's blocks of a row, 9 steps together whatever the
    // rotation is; the rotation moves on by one with every row and by one more every 16 rows, so a CU sees every tile index.
    const int row = blockIdx.z * gridDim.y + blockIdx.y;
    const int xr = (blockIdx.x + row + (row >> 4)) % gridDim.x;
    const int half = (gridDim.x + 1) >> 1;
    const int qt = xr < half ? gridDim.x - 1 - xr : xr - half;
#ifdef DH_PREFILL_STAMPS
    const int pf_blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
#endif
    PF_STAMP(0);
#ifdef DH_PREFILL_STAMPS
    if (threadIdx.x == 0 && pf_blk < PF_STAMP_BLOCKS) {
        g_prefill_stamps[pf_blk * PF_STAMP_SLOTS + 37] = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_REG_HW_ID, 32 bits
        g_prefill_stamps[pf_blk * PF_STAMP_SLOTS + 38] = __builtin_amdgcn_s_getreg(20 | (3 << 11));    // HW_REG_XCC_ID, bits 0-3
        g_prefill_stamps[pf_blk * PF_STAMP_SLOTS + 39] = qt;
    }
#endif
    const int qlen = q_len[seq];
    const int q0 = qt * 32;
    if (q0 >= qlen) return;                             // uniform for the whole block
    const int slot = seq_slot[seq], qs = q_start[seq], p0 = kv_pos0[seq] + q0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // uniform: the stage deal below is scalar code, not a lane loop
    const int nwaves = WPB ? WPB : (int)(blockDim.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int head = g * q_per_kv + part * nwaves + wave;
    PF_HAVE("s"(slot), "s"(qs), "s"(p0));
    PF_STAMP(1);

    const bf16_t* kbase = k_cache + ((size_t)slot * n_groups + g) * s_max * HS;
    const bf16_t* vbase = vT_cache + ((size_t)slot * n_groups + g) * HS * s_max;
    // keys beyond the tile's last real query position are never attended (and may not exist)
    const int last_key = min(p0 + 31, kv_pos0[seq] + qlen - 1);
    const int n_tiles = last_key / 64 + 1;
    const int q_abs = p0 + lr;

    // one-KiB groups (64 lanes x 16 B) of a stage dealt over the waves: 2*TILE_B/1024 of K then as many of V^T
    constexpr int GRP = 2 * TILE_B / 1024;
    auto stage = [&](int buf, int kt) __attribute__((always_inline)) {
        const char* gk = reinterpret_cast<const char*>(kbase + (size_t)(2 * kt) * HS * 32);
        const char* gv = reinterpret_cast<const char*>(vbase + (size_t)(2 * kt) * HS * 32);
        auto copy = [&](int gidx) __attribute__((always_inline)) {
            const char* src = gidx < GRP ? gk + gidx * 1024 : gv + (gidx - GRP) * 1024;
            glds16(src + lane * 16, sKV[buf] + gidx * 1024);
        };
        if constexpr (WPB != 0) {                       // 2 GRP is 16, 24 or 32: the same number of groups for every wave, no branches
#pragma unroll
            for (int i = 0; i < 2 * GRP / (WPB ? WPB : 1); ++i) copy(wave + i * WPB);
        } else {
            for (int gidx = wave; gidx < 2 * GRP; gidx += nwaves) copy(gidx);
        }
    };
    // The prologue is ONE round trip: stage 0 is requested as soon as the slot is known, the Q loads follow it, and both are waited
    // for once (it was Q loads, wait, scale, stage 0, wait: two dependent trips per block, and a group now runs q_per_kv / WPB blocks).
    stage(0, 0);

    // Q fragments (B operand): lane holds Q[q0+lr][ks*16 + lh*8 .. +8)
    bf16x8 qf[KS];
    {
        int row = q0 + lr;
        row = row < qlen ? row : qlen - 1;
        const bf16_t* qp = q + ((size_t)(qs + row) * n_head + head) * HS + lh * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // Q and this wave's share of stage 0
        // Q's first use is pinned here, where the wait is: left to the first MFMA (hs 96 / 128 do not scale Q) it would sit behind
        // the DMA of stage 1, and a wait for an ordinary load drains every DMA in front of it
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));
        if (PS) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[ks][e] = (short)f2bf(bf2f((bf16_t)qf[ks][e]) * scale);
        }
    }
    PF_STAMP(2);

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    __syncthreads();
    PF_STAMP(3);
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int key0 = kt * 64;
        // buffer (kt+1)&1 was last read in iteration kt-1, which ended with a barrier
        if (kt + 1 < n_tiles) stage((kt + 1) & 1, kt + 1);
        const char* sK = sKV[kt & 1];
        const char* sV = sK + 2 * TILE_B;

        // ---- S^T = K · Q^T for the two 32-key row tiles
        f32x16 st[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) st[rt][r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (rt * KS + ks) * 1024 + lane * 16);
                st[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], st[rt], 0, 0, 0);
            }
        }
        PF_STAMP_STEP(kt, 0);
        // ---- scale, causal mask (only a tile that reaches past the block's first query can hold masked keys), tile max
        if (!PS) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[rt][r] *= scale;
        }
        if (key0 + 63 > p0) {
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key_abs = key0 + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    st[rt][r] = key_abs <= q_abs ? st[rt][r] : -INFINITY;
                }
        }
        float m_t = -INFINITY;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) m_t = fmaxf(m_t, st[rt][r]);
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);           // finite: key 0 is always visible
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __expf(st[rt][r] - m_new);
                st[rt][r] = p;
                psum += p;
            }
        l_run = l_run * alpha + psum;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {   // the running max moved for some query of the wave
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }

        PF_STAMP_STEP(kt, 1);

        // ---- O^T += V^T · P^T
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
                for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[rt][8 * s + 2 * j], st[rt][8 * s + 2 * j + 1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const bf16x8 vf = *reinterpret_cast<const bf16x8*>(sV + (((rt * DT + dt) * 2 + s) * 1024) + lane * 16);
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf.v, o[dt], 0, 0, 0);
                }
            }
        PF_STAMP_STEP(kt, 2);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's share of the next stage has landed
        __syncthreads();                                    // ... everybody's, and this stage's reads are done
        PF_STAMP_STEP(kt, 3);
    }

    // ---- normalise and store y[q][head*HS + d]
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    if (lse != nullptr && lh == 0 && q0 + lr < qlen)     // log-sum-exp of the scaled scores (training backward)
        lse[(size_t)(qs + q0 + lr) * n_head + head] = m_run + logf(l_tot);
    if (q0 + lr < qlen) {
        bf16_t* yp = y + (size_t)(qs + q0 + lr) * n_head * HS + head * HS;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int d = dt * 32 + 8 * rg + 4 * lh;
                uint2 pk = make_uint2(pack2bf(o[dt][rg * 4 + 0] * inv, o[dt][rg * 4 + 1] * inv),
                                      pack2bf(o[dt][rg * 4 + 2] * inv, o[dt][rg * 4 + 3] * inv));
                *reinterpret_cast<uint2*>(yp + d) = pk;
            }
    }
    PF_STAMP(36);
}

// ------------------------------------------------------------------------------------ decode
// One query per sequence.  The q_per_kv heads of a group sit on the accumulator's lane axis
// (columns >= q_per_kv are zero padding: the step is HBM-bound, the idle MFMA columns are free).
// grid (n_seq*n_groups, NSPLIT); each of the 4*NSPLIT waves of a (sequence, group) pair walks
// 32-key tiles straight from HBM to registers (no LDS: nothing is shared between waves) and
// leaves an (m, l, O^T) partial; attn_decode_combine_kernel merges them.
constexpr int DEC_COLS = 16;   // padded head columns in the partials

// The cache a decode step reads, passed by value: the bf16 fragment caches, or the fp8 bytes and their exponents (common.h k8_off /
// v8_off; written by kv8.hip).  A DecodeTile owns exactly what differs between the two: where a tile lives, how it is loaded, and where
// the A operands of the two MFMAs come from.  Everything else is attn_decode_kernel, once.
struct CacheBf16 {
    const bf16_t *k, *vT;
};
struct CacheFp8 {
    const uint8_t *k8, *v8;
    const int8_t *k_exp, *v_exp;
};

template <int HS, class Cache>
struct DecodeTile;

// one 32-key tile = 8 coalesced 1-KiB loads that ARE the MFMA fragments (K: KS x 16 B, V^T: DT x 2 x 2 x 8 B per lane)
template <int HS>
struct DecodeTile<HS, CacheBf16> {
    static constexpr int KS = HS / 16, DT = HS / 32;
    struct VF { bf16x8 v; };
    struct VScales {};
    const bf16_t *kbase, *vbase;
    bf16x8 kf[KS];
    VF vf[DT][2];

    __device__ __forceinline__ DecodeTile(const CacheBf16& c, int slot, int g, int n_groups, int s_max)
        : kbase(c.k + ((size_t)slot * n_groups + g) * s_max * HS), vbase(c.vT + ((size_t)slot * n_groups + g) * HS * s_max) {}
    __device__ __forceinline__ void load(int t, int lane, int lr, int lh) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            kf[ks] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kbase + kfrag_blk<HS>(t, ks) + lane * 8));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                vf[dt][s].v = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(vbase + vfrag_blk<HS>(t, dt, s) + lane * 8));
    }
    __device__ __forceinline__ bf16x8 k(int ks) const { return kf[ks]; }
    __device__ __forceinline__ VScales v_scales(int) const { return {}; }
    __device__ __forceinline__ bf16x8 v(int dt, int s, const VScales&) const { return vf[dt][s].v; }
};

// A tile is HS/32 + HS/32 coalesced 1-KiB loads of 16 B per lane, each holding two k-step fragments, plus 32 + 32 exponent bytes.
// A fragment becomes bf16 in registers, e4m3 -> fp32 (v_cvt_pk_f32_fp8), times the power-of-two scale of its key, truncated to
// bf16 — all exact, and applied to the OPERAND: the MFMAs see the values the bf16 tile reads from the expanded cache
// (dh_kv8_expand), so the two instantiations agree bit for bit.
template <int HS>
struct DecodeTile<HS, CacheFp8> {
    static constexpr int KS = HS / 16, DT = HS / 32;
    struct VScales { float s[8]; };
    const uint8_t *kbase, *vbase;
    const int8_t *kebase, *vebase;
    i32x4 kb[DT], vb[DT];
    float ksc;               // the A row of this lane is key lr
    uint32_t vew[2][2];      // exponents of the lane's 8 keys of k-step s: keys 16s + 4lh + 0..3, + 8

    __device__ __forceinline__ DecodeTile(const CacheFp8& c, int slot, int g, int n_groups, int s_max) {
        const size_t blk = (size_t)slot * n_groups + g;
        kbase = c.k8 + blk * s_max * HS, vbase = c.v8 + blk * s_max * HS;
        kebase = c.k_exp + blk * s_max, vebase = c.v_exp + blk * s_max;
    }
    __device__ __forceinline__ void load(int t, int lane, int lr, int lh) {
        const int key0 = t * 32;
#pragma unroll
        for (int b = 0; b < DT; ++b) {
            kb[b] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(kbase + kv8_blk<HS>(t, b) + lane * 16));
            vb[b] = __builtin_nontemporal_load(reinterpret_cast<const i32x4*>(vbase + kv8_blk<HS>(t, b) + lane * 16));
        }
        ksc = kv8_pow2(kebase[key0 + lr]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            vew[s][0] = *reinterpret_cast<const uint32_t*>(vebase + key0 + 16 * s + 4 * lh);
            vew[s][1] = *reinterpret_cast<const uint32_t*>(vebase + key0 + 16 * s + 4 * lh + 8);
        }
    }
    __device__ __forceinline__ bf16x8 k(int ks) const {
        union { bf16x8 v; uint32_t u[4]; } kf;
        const int w = (ks & 1) * 2;
        kv8_cvt4((uint32_t)kb[ks >> 1][w], ksc, ksc, ksc, ksc, kf.u[0], kf.u[1]);
        kv8_cvt4((uint32_t)kb[ks >> 1][w + 1], ksc, ksc, ksc, ksc, kf.u[2], kf.u[3]);
        return kf.v;
    }
    __device__ __forceinline__ VScales v_scales(int s) const {
        VScales vs;
        kv8_scales4(vew[s][0], vs.s);
        kv8_scales4(vew[s][1], vs.s + 4);
        return vs;
    }
    __device__ __forceinline__ bf16x8 v(int dt, int s, const VScales& vs) const {
        union { bf16x8 v; uint32_t u[4]; } vf;
        kv8_cvt4((uint32_t)vb[dt][2 * s], vs.s[0], vs.s[1], vs.s[2], vs.s[3], vf.u[0], vf.u[1]);
        kv8_cvt4((uint32_t)vb[dt][2 * s + 1], vs.s[4], vs.s[5], vs.s[6], vs.s[7], vf.u[2], vf.u[3]);
        return vf.v;
    }
};

template <int HS, class Cache>
__global__ __launch_bounds__(256) void attn_decode_kernel(
    const bf16_t* __restrict__ q, const Cache cache, const int32_t* __restrict__ seq_slot, const int32_t* __restrict__ kv_len,
    float* __restrict__ work, int n_head, int n_groups, int s_max, float scale) {
    constexpr int KS = HS / 16, DT = HS / 32;
    const int pair = blockIdx.x, seq = pair / n_groups, g = pair % n_groups;
    const int nw = gridDim.y * 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wg = blockIdx.y * 4 + wave;
    const int lr = lane & 31, lh = lane >> 5;
    const int q_per_kv = n_head / n_groups;
    const int slot = seq_slot[seq], len = kv_len[seq];
    const int n_tiles = (len + 31) / 32;

    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        if (lr < q_per_kv)
            z = *reinterpret_cast<const bf16x8*>(q + ((size_t)seq * n_head + g * q_per_kv + lr) * HS + ks * 16 + lh * 8);
        qf[ks] = z;
    }
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    DecodeTile<HS, Cache> tile(cache, slot, g, n_groups, s_max);

    for (int t = wg; t < n_tiles; t += nw) {
        const int key0 = t * 32;
        // issue all loads of the tile first (keys >= len are masked below; their cache bytes, and exponents, are finite)
        tile.load(t, lane, lr, lh);
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tile.k(ks), qf[ks], st, 0, 0, 0);
        float m_t = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key_abs = key0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float s = st[r] * scale;
            s = key_abs < len ? s : -INFINITY;
            st[r] = s;
            m_t = fmaxf(m_t, s);
        }
        m_t = fmaxf(m_t, __shfl_xor(m_t, 32, 64));
        const float m_new = fmaxf(m_run, m_t);           // finite: key0 < len
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __expf(st[r] - m_new);
            st[r] = p;
            psum += p;
        }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            union { bf16x8 v; uint32_t u[4]; } pf;
#pragma unroll
            for (int j = 0; j < 4; ++j) pf.u[j] = pack2bf(st[8 * s + 2 * j], st[8 * s + 2 * j + 1]);
            const auto vs = tile.v_scales(s);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (s == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                }
                // keys >= len carry p == 0; the cache is zero-initialised so 0 * v stays 0
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tile.v(dt, s, vs), pf.v, o[dt], 0, 0, 0);
            }
        }
    }
    // partial: [pair][wg] -> m[DEC_COLS], l[DEC_COLS], o[HS][DEC_COLS]
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    float* wp = work + ((size_t)pair * nw + wg) * (2 * DEC_COLS + HS * DEC_COLS);
    if (lr < q_per_kv) {
        if (lh == 0) {
            wp[lr] = m_run;
            wp[DEC_COLS + lr] = l_tot;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = dt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                wp[2 * DEC_COLS + d * DEC_COLS + lr] = o[dt][r];
            }
    }
}

template <int HS>
__global__ void attn_decode_combine_kernel(const float* __restrict__ work, bf16_t* __restrict__ y, int n_head,
                                           int n_groups, int nw) {
    const int pair = blockIdx.x, seq = pair / n_groups, g = pair % n_groups;
    const int q_per_kv = n_head / n_groups;
    const int stride = 2 * DEC_COLS + HS * DEC_COLS;
    for (int it = threadIdx.x; it < q_per_kv * HS; it += blockDim.x) {
        const int h = it / HS, d = it % HS;
        const float* wp = work + (size_t)pair * nw * stride;
        float M = -INFINITY;
        for (int w = 0; w < nw; ++w) M = fmaxf(M, wp[w * stride + h]);
        float L = 0.f, O = 0.f;
        for (int w = 0; w < nw; ++w) {
            const float mw = wp[w * stride + h];
            const float f = (mw == -INFINITY) ? 0.f : __expf(mw - M);
            L += wp[w * stride + DEC_COLS + h] * f;
            O += wp[w * stride + 2 * DEC_COLS + d * DEC_COLS + h] * f;
        }
        y[(size_t)seq * n_head * HS + (g * q_per_kv + h) * HS + d] = f2bf(O / L);
    }
}

constexpr int DEC_NSPLIT = 4;

// the split-KV kernel over either cache, then the combine: the checks the two entries share (`name` is the entry's), the grid, the
// head-size dispatch
template <class Cache>
int attn_decode_launch(const char* name, const Cache cache, const dh_bf16* q, const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* y,
                       void* work, int n_seq, int n_head, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(n_groups > 0 && n_head % n_groups == 0 && n_head / n_groups <= DEC_COLS, "%s: bad head counts", name);
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "%s: head_size %d unsupported", name, hs);
    DH_CHECK(work != nullptr, "%s: null workspace", name);
    if (n_seq <= 0) return 0;
    const int pairs = n_seq * n_groups;
    const float scale = 1.0f / sqrtf((float)hs);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(pairs, DEC_NSPLIT), block(256);
    dispatch_hs(hs, [&](auto hs_c) {
        constexpr int HS = decltype(hs_c)::value;
        hipLaunchKernelGGL((attn_decode_kernel<HS, Cache>), grid, block, 0, s, q, cache, seq_slot, kv_len, (float*)work, n_head, n_groups,
                           s_max, scale);
        hipLaunchKernelGGL((attn_decode_combine_kernel<HS>), dim3(pairs), dim3(256), 0, s, (const float*)work, y, n_head, n_groups,
                           DEC_NSPLIT * 4);
    });
    DH_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int dh_attn_prefill_bf16(const dh_bf16* q, const dh_bf16* k_cache, const dh_bf16* vT_cache,
                                    const int32_t* seq_slot, const int32_t* q_start, const int32_t* q_len,
                                    const int32_t* kv_pos0, dh_bf16* y, float* lse, int n_seq, int max_q_len,
                                    int n_head, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(n_groups > 0 && n_head % n_groups == 0 && n_head / n_groups <= 16, "dh_attn_prefill_bf16: bad head counts");
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "dh_attn_prefill_bf16: head_size %d unsupported", hs);
    DH_CHECK(s_max % 64 == 0, "dh_attn_prefill_bf16: s_max must be a multiple of 64");
    DH_CHECK(64 * (n_head / n_groups) <= (hs == 64 ? 1024 : 512), "dh_attn_prefill_bf16: too many query heads per group");
    if (n_seq <= 0 || max_q_len <= 0) return 0;
    const int q_per_kv = n_head / n_groups;
    int wpb = g_prefill_wpb;            // waves per block; 0, head size 96 or a count that does not divide the group: the whole group
    if (hs == 96 || wpb <= 0 || q_per_kv % wpb != 0) wpb = 0;
    dim3 grid(cdiv(max_q_len, 32), wpb ? n_groups * (q_per_kv / wpb) : n_groups, n_seq), block(64 * (wpb ? wpb : q_per_kv));
    const float scale = 1.0f / sqrtf((float)hs);
    hipStream_t s = (hipStream_t)stream;
    dispatch_hs(hs, [&](auto hs_c) {   // head size 64: scale = 1/8, applied to Q; 1/sqrt(96) is not a power of two: scaled per score, as at 128
        constexpr int HS = decltype(hs_c)::value;
        auto launch = [&](auto wpb_c) {
            hipLaunchKernelGGL((attn_prefill_kernel<HS, HS == 64, decltype(wpb_c)::value>), grid, block, 0, s, q, k_cache, vT_cache, seq_slot,
                               q_start, q_len, kv_pos0, y, lse, n_head, n_groups, s_max, scale);
        };
        if constexpr (HS == 96) launch(std::integral_constant<int, 0>{});
        else if (wpb == 4) launch(std::integral_constant<int, 4>{});
        else if (wpb == 2) launch(std::integral_constant<int, 2>{});
        else launch(std::integral_constant<int, 0>{});
    });
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t dh_attn_decode_work_bytes(int n_seq, int n_head, int hs, int s_max) {
    (void)s_max;
    // upper bound over n_groups: pairs <= n_seq * n_head
    return (int64_t)n_seq * n_head * (DEC_NSPLIT * 4) * (2 * DEC_COLS + hs * DEC_COLS) * sizeof(float);
}

extern "C" int dh_attn_decode_bf16(const dh_bf16* q, const dh_bf16* k_cache, const dh_bf16* vT_cache,
                                   const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* y, void* work, int n_seq,
                                   int n_head, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(s_max % 64 == 0, "dh_attn_decode_bf16: s_max must be a multiple of 64");
    return attn_decode_launch("dh_attn_decode_bf16", CacheBf16{k_cache, vT_cache}, q, seq_slot, kv_len, y, work, n_seq, n_head, n_groups,
                              hs, s_max, stream);
}

extern "C" int dh_attn_decode_kv8(const dh_bf16* q, const uint8_t* k8, const uint8_t* v8, const int8_t* k_exp, const int8_t* v_exp,
                                  const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* y, void* work, int n_seq, int n_head,
                                  int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(q && k8 && v8 && k_exp && v_exp && seq_slot && kv_len && y, "dh_attn_decode_kv8: null argument");
    DH_CHECK(s_max > 0 && s_max % 64 == 0, "dh_attn_decode_kv8: s_max must be a multiple of 64");
    return attn_decode_launch("dh_attn_decode_kv8", CacheFp8{k8, v8, k_exp, v_exp}, q, seq_slot, kv_len, y, work, n_seq, n_head, n_groups,
                              hs, s_max, stream);
}
