// Native decoder runtime: owns the KV cache, the activation workspace and the kernel sequence of
// ger/lora.py:504-549 (GPT.forward) + generate/base.py:57-80 (the decode loop) for a packed,
// ragged batch.  Host side is plain C++; the decode step is captured once into a hipGraph and
// replayed, so a generated token costs one graph launch and no host synchronisation.
#include <algorithm>
#include <mutex>
#include <vector>

#include "common.h"
#include "gemm.h"

constexpr int MAX_DECODE_ROWS = 2048;  // single-token calls up to here take the 7-launch streaming path
// Single-token steps over at least this many rows run the layer on the TILED MFMA GEMMs of the prefill (natural
// k order) instead of the K-sliced streaming kernels: from a few hundred rows on the step is no longer weight-
// bandwidth-bound and the partial-sum traffic of the K slices dominates (dh_set_tuning key 10; 0 = never).
int g_decode_tiled_rows = 0;
int g_short_kps = 8;       // k-steps per K-slice of the partial-sum GEMMs when K <= 4096 (dh_set_tuning key 16: 8 or 16)
int g_fuse_qkv_rope = 1;   // dh_set_tuning key 12: 0 = QKV GEMM, then dh_qkv_rope_cache_bf16 (the two-step form)
// dh_set_tuning key 23.  A prefill that is asked for the LAST position's logits only (generate's prompt forward,
// generate/base.py:57-60: `logits[0, -1]`) needs, of the last layer, the K / V rows of every token (they go to the cache) but the
// attention output, projection and MLP of the last token of each sequence alone: the other rows of the last block feed nothing
// (the reference computes and drops them, as it does the lm_head rows — SURVEY Q9).  1 = run those four products on the
// n_seq last rows (same kernels, same chains: the rows' bits do not change); 0 = on every row.
int g_prune_last_layer = 1;

struct dh_engine {
    dh_model_desc d;
    std::vector<dh_layer_weights> layers;
    int max_batch = 0, s_max = 0, max_tokens = 0;
    int row_cap = 0;                                  // rows the single-token-step workspaces hold (logits, part32, dec_ids, ones): max_batch, or what dh_engine_reserve_rows asked for
    int qkv_dim = 0, kv_dim = 0;
    // device memory
    bf16_t *kc = nullptr, *vtc = nullptr;             // [L][B][G][S][HS], [L][B][G][HS][S]; kv8: ONE layer's worth, the prompt attention's scratch
    bool kv8 = false;                                 // fp8 KV cache (dh_engine_create_ex kv_dtype 1; common.h k8_off / v8_off)
    uint8_t *k8 = nullptr, *v8 = nullptr;             // kv8: [L][B][G][S * HS] e4m3 bytes of K and of V^T
    int8_t *ke = nullptr, *ve = nullptr;              // kv8: [L][B][G][S] exponents of the K and of the V vectors
    size_t exp_layer_elems = 0;                       // B * G * S
    bf16_t *x = nullptr, *xn = nullptr, *qkv = nullptr, *qrot = nullptr, *att = nullptr, *xa = nullptr,
           *act = nullptr, *xlast = nullptr, *logits = nullptr;
    int32_t *tok_slot = nullptr, *tok_pos = nullptr, *seq_meta = nullptr;   // seq_meta: 4 x [B], read through seq_meta() below
    int32_t *last_row = nullptr, *step_dev = nullptr;
    // What the dh_engine_set_* calls have set for later steps (common.h describes the members; everything off: the steps the engine always
    // ran).  `set.start` stays null: the four setters that take the [n_seq] prompt lengths each keep their own pointer, null while their
    // option is off, and step_ctl() below gives a step the one it reads.
    dh_pick_ctl set;
    const int32_t *ngram_start = nullptr, *stop_start = nullptr, *pen_start = nullptr, *bias_start = nullptr, *aut_start = nullptr;
    int32_t* stop_fin_tok = nullptr;                    // dh_engine_set_stop: a beam call's [n_utt, W] ending ids
    int64_t* beam_hist = nullptr;                       // dh_engine_set_beam_history: the caller's [2][n_utt * W][max_new] history planes (null: off)
    int beam_hist_ngram = 0;                            // and the beam steps' no_repeat_ngram (0: no ban)
    int shared_rows = 0;                                // dh_engine_set_shared_prompt: rows per utterance (0: off) and the utterances'
    const int32_t* shared_plen = nullptr;               // prompt lengths on the device
    int step_shared_rows = 0;                           // the same two for the step being launched or captured (decode_step sets and
    const int32_t* step_shared_plen = nullptr;          // clears them: a prompt forward of one token per sequence never sees them)
    int32_t* slot_list = nullptr;                       // [B]: the KV slots of a dh_engine_forward_slots call (seq_meta[0..B) stays the identity)
    int32_t* copy_dst = nullptr;                        // [B]: the destination slots of a dh_engine_copy_prefix call
    bf16_t* beam_scratch = nullptr;                     // dh_engine_reserve_beams: [row][2 L x G][tiles][hs * 32], the re-parenting's way station
    size_t beam_scratch_elems = 0;
    int32_t* beam_tab = nullptr;                        // dh_engine_set_beam_tiles: the caller's [2][n_utt * W][beam_tab_nt] tile table (null: off)
    int beam_tab_nt = 0;
    int32_t* step_beam_tab = nullptr;                   // the same two for the step being launched or captured, as step_shared_rows
    int step_beam_tab_nt = 0;
    bf16_t* beam_tile_scratch = nullptr;                // dh_engine_reserve_beam_tiles: [row][2 L x G][hs * 32], the open tile's way station
    size_t beam_tile_scratch_elems = 0;
    int32_t* beam_cand_ids = nullptr;                   // [B, 2 W_max] candidates of a beam step's rows (dh_beam_select_bf16's workspace)
    float* beam_cand_lp = nullptr;
    bf16_t** cache_tab = nullptr;                       // [2 L] device table, written once: K cache of layer l at 2l, V^T cache at 2l + 1
                                                        // (kv8: [4 L], the fp8 bytes like that, then the exponent arrays like that)
    int32_t* last_meta = nullptr;                       // [ones | position of the last token] x [B]: the pruned last layer's attention call
    bf16_t *att_last = nullptr, *xn_last = nullptr, *act_last = nullptr;   // its n_seq-row operands
    uint8_t *row_tail = nullptr, *last_tail = nullptr, *ones = nullptr;   // Q11 rsqrt emulation flags
    int rsqrt_vec = 0, rsqrt_whole = 0;
    int64_t* dec_ids = nullptr;
    void* dec_work = nullptr;
    float* part32 = nullptr;                            // fp32 partial sums of the decode GEMMs
    bool fp8 = false;                                   // e4m3 weights + channel scales (csrc/fp8.hip)
    bool mx4 = false;                                   // fp8 engine whose block weights are MXFP4 (csrc/mxfp4.hip; lm_head stays e4m3)
    uint8_t* xq = nullptr;                              // fp8 mode: quantised activations [max_tokens, max(d, I)]
    float* xscale = nullptr;                            // fp8 mode: their per-token scales [max_tokens]
    bool a6 = false;                                    // MXFP4 engine whose block activations are MXFP6 (csrc/mxfp6.hip; ln_f and lm_head stay e4m3)
    uint8_t* xq6 = nullptr;                             // a6: e2m3 codes of max_tokens rounded up to 16 rows x max(d, I), in fragment order
    uint8_t* xs6 = nullptr;                             // a6: their E8M0 bytes
    int32_t* h_stage = nullptr;                         // pinned staging for the metadata, carved by stage() below
    size_t cache_layer_elems = 0;
    int64_t dev_bytes = 0;
    int64_t row_ws_bytes = 0;                         // the part of dev_bytes that alloc_row_ws holds
    // decode graph
    hipStream_t gstream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_stage = nullptr;
    // captured decode steps, keyed by everything baked into the graph (a few batch sizes alternate in practice)
    // (limit, row_seq, row_slot, n_all, max_new: the row-list step of dh_engine_decode_rows; null / 0 in dh_engine_decode's keys)
    // Every member starts at the value it has in a key whose step does not use it; the entry points assign the rest by name.
    struct GKey {
        int64_t* tokens = nullptr; int tok_ld = 0; int32_t *length = nullptr, *done = nullptr; int n_seq = 0, top_k = 0; float temp = 0.f;
        int64_t eos = 0; uint64_t seed = 0; int rsqrt_vec = 0, tiled_rows = 0;
        const int32_t *limit = nullptr, *row_seq = nullptr, *row_slot = nullptr; int n_all = 0, max_new = 0;
        // dh_engine_decode_spec: D drafts per step (0 in every other key), the scripted drafts, the counters
        int spec = 0; const int64_t* drafts = nullptr; int32_t* counters = nullptr;
        // dh_engine_decode_spec_draw: the step's positions draw (top_k and seed above are then the draw's, as in a plain step's key)
        bool spec_draw = false;
        // the options the step's sampling launch takes (step_ctl): a step captured without one of them is another kernel, or other arguments
        dh_pick_ctl ctl;
        // dh_engine_decode_beam: W beams (0 in every other key) and the call's state arrays; length = n_steps, limit = prompt_len,
        // n_seq = n_utt * W rows; the ending ids of dh_engine_set_stop; the history planes and their ban of dh_engine_set_beam_history
        int beam_w = 0; dh_beam_state beam{}; int32_t* stop_fin_tok = nullptr; int64_t* beam_hist = nullptr; int beam_ngram = 0;
        // the tile table of dh_engine_set_beam_tiles and its tiles per row (null / 0: the re-parenting copy)
        int32_t* beam_tab = nullptr; int beam_tab_nt = 0;
        // dh_engine_set_shared_prompt: rows per utterance (0 in a key whose step runs the single-token attention) and the prompt lengths
        int shared_rows = 0; const int32_t* shared_plen = nullptr;
        bool operator==(const GKey& k) const {
            return tokens == k.tokens && tok_ld == k.tok_ld && length == k.length && done == k.done && n_seq == k.n_seq &&
                   top_k == k.top_k && temp == k.temp && eos == k.eos && seed == k.seed && rsqrt_vec == k.rsqrt_vec &&
                   tiled_rows == k.tiled_rows && limit == k.limit && row_seq == k.row_seq && row_slot == k.row_slot &&
                   n_all == k.n_all && max_new == k.max_new && spec == k.spec && drafts == k.drafts && counters == k.counters &&
                   spec_draw == k.spec_draw &&
                   ctl == k.ctl && beam_w == k.beam_w && stop_fin_tok == k.stop_fin_tok && beam_hist == k.beam_hist &&
                   beam_ngram == k.beam_ngram && beam_tab == k.beam_tab && beam_tab_nt == k.beam_tab_nt && shared_rows == k.shared_rows && shared_plen == k.shared_plen && memcmp(&beam, &k.beam, sizeof(beam)) == 0;         // a struct of pointers: no padding
        }
    };
    struct GEntry { GKey key; hipGraphExec_t exec; uint64_t used; };
    std::vector<GEntry> graphs;
    uint64_t graph_clock = 0;
    const int32_t* seq_slot = nullptr;   // device array: KV slot of sequence / row i of the current call (set by every entry point)
    bool capturing = false;   // no event records inside a stream capture
    bool phase_decode = false; // single-token-per-sequence call: weight-streaming GEMMs + split-KV attention
    bool decode_tiled = false; // ... except that this step's row count put it in the tiled class (g_decode_tiled_rows)
    struct Timing {
        bool on = false;
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[4];
    } tm;
};

namespace {

// the engines dh_engine_create has handed out and dh_engine_destroy has not taken back: dh_engine_copy_prefix looks a handle up
// here before it reads anything through it
std::mutex g_engines_mu;
std::vector<const dh_engine*> g_engines;
bool engine_is_live(const dh_engine* e) {
    std::lock_guard<std::mutex> lock(g_engines_mu);
    return e && std::find(g_engines.begin(), g_engines.end(), e) != g_engines.end();
}

template <typename T>
int dmalloc(dh_engine* e, T** p, size_t n) {
    DH_HIP(hipMalloc((void**)p, n * sizeof(T)));
    e->dev_bytes += (int64_t)(n * sizeof(T));
    return 0;
}

// ---- metadata ----------------------------------------------------------------------------------------------------------------
// Per-sequence arrays of the current call on the device.  seq_slot is the entry point's choice (e->seq_slot); the other three are
// rows 1..3 of e->seq_meta (4 x [max_batch], contiguous: forward_impl uploads them with one copy).  Row 0 is the identity, written
// once at engine creation: sequence i in slot i.
struct SeqMeta {
    const int32_t* seq_slot;
    int32_t *q_start, *q_len;
    int32_t* kv;   // prefill: kv_pos0, the position of a sequence's first query; single-token step: kv_len
};
SeqMeta seq_meta(const dh_engine* e) {
    const int B = e->max_batch;
    return {e->seq_slot, e->seq_meta + B, e->seq_meta + 2 * B, e->seq_meta + 3 * B};
}

// The pinned staging buffer, offsets in int32 for T = max_tokens and B = max_batch:
//   [tok_slot T | tok_pos T | seq_slot, q_start, q_len, kv, last_row: 5 x B | tail flags | last_meta: ones B, last position B]
// The tail flags are bytes (T per-row flags, then B last-row flags) in a region of T + B int32.
struct StageLayout { size_t tok_slot, tok_pos, meta, tail, last_meta, total; };
constexpr StageLayout stage_layout(size_t T, size_t B) {
    StageLayout L{};
    L.tok_slot = 0;
    L.tok_pos = L.tok_slot + T;
    L.meta = L.tok_pos + T;
    L.tail = L.meta + 5 * B;
    L.last_meta = L.tail + T + B;
    L.total = L.last_meta + 2 * B;
    return L;
}
static_assert(stage_layout(4096, 48).total == 3 * 4096 + 8 * 48 && stage_layout(4096, 48).last_meta == 3 * 4096 + 6 * 48,
              "the staging layout is part of nothing public, but its size is what the engine has always pinned");

struct Stage {
    int32_t *tok_slot, *tok_pos;
    int32_t *seq_slot, *q_start, *q_len, *kv, *last_row;   // contiguous rows of B, as in SeqMeta
    uint8_t *row_tail, *last_tail;
    int32_t* last_meta;                                    // [ones | last position] x B
};
Stage stage(const dh_engine* e) {
    const size_t T = e->max_tokens, B = e->max_batch;
    const StageLayout L = stage_layout(T, B);
    int32_t* h = e->h_stage;
    int32_t* m = h + L.meta;
    uint8_t* tail = reinterpret_cast<uint8_t*>(h + L.tail);
    return {h + L.tok_slot, h + L.tok_pos, m, m + B, m + 2 * B, m + 3 * B, m + 4 * B, tail, tail + T, h + L.last_meta};
}

// ---- glue kernels ------------------------------------------------------------------------------------------------------------
// ids of a decode step, positions and lengths derived on device from (tokens, length).  Row r works on sequence u = row_seq[r] (its
// token buffer row, its length) in KV slot row_slot[r]; null lists mean u = slot = r.  A row list entry outside [0, n_all) x
// [0, max_batch) never comes from the entry point's callers; it is mapped to sequence 0 / slot 0, positions that exist, rather than
// trusted.  The length is clamped to the cache AND the token buffer: neither sampling kernel lets `length` pass tok_ld, so the second
// bound only matters for a caller who hands in a length that its own buffer cannot hold.
// step_dev (null: no counter) is the per-step RNG counter of dh_engine_decode's sampling kernel.
__global__ void decode_prep_kernel(const int64_t* __restrict__ tokens, int tok_ld, const int32_t* __restrict__ length,
                                   const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_slot,
                                   int64_t* __restrict__ ids, int32_t* __restrict__ tok_slot, int32_t* __restrict__ tok_pos,
                                   int32_t* __restrict__ kv_len, int32_t* step_dev, int n_rows, int n_all, int max_batch, int s_max) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0 && step_dev) *step_dev += 1;
    if (r < n_rows) {
        int u = r, slot = r;
        if (row_seq) {   // the two lists come together
            u = row_seq[r], slot = row_slot[r];
            u = u < 0 || u >= n_all ? 0 : u;
            slot = slot < 0 || slot >= max_batch ? 0 : slot;
        }
        int n = length[u];
        const int cap = s_max < tok_ld ? s_max : tok_ld;
        n = n < 1 ? 1 : (n > cap ? cap : n);         // never index outside the cache or the token buffer
        ids[r] = tokens[(size_t)u * tok_ld + n - 1];
        tok_slot[r] = slot;
        tok_pos[r] = n - 1;
        kv_len[r] = n;
    }
}

// The same for a verify step of D = S - 1 drafts (dh_engine_decode_spec), one block per sequence: row u * S + j gets the sequence's
// last token (j = 0) or its j-th draft, position len - 1 + j and slot u; kv_len[u] = len.  The length is clamped as above and to the
// rope table; a position behind the cache's end is clamped too (the attention kernel appends nothing for such a row).
// drafts != null: the scripted proposer, drafts[u, i] stands for the i-th generated token of sequence u (limit[u] - max_new = its
// prompt length).  drafts == null: prompt lookup, dualhyp_amd/speculate.py:propose on tokens[u, :len] — for n = ngram_max .. 1 the
// latest earlier occurrence of the last n tokens that a token follows; the drafts are the up to D tokens behind it, padded with the
// last of them (which is then tokens[len - 1]); no occurrence: tokens[len - 1], D times.  An id outside the embedding table is
// replaced by the last token.
__global__ __launch_bounds__(256) void spec_prep_kernel(const int64_t* __restrict__ tokens, int tok_ld, const int32_t* __restrict__ length,
                                                        const int32_t* __restrict__ limit, int max_new, const int64_t* __restrict__ drafts,
                                                        int S, int ngram_max, int64_t* __restrict__ ids, int32_t* __restrict__ tok_slot,
                                                        int32_t* __restrict__ tok_pos, int32_t* __restrict__ kv_len, int32_t* step_dev,
                                                        int cap, int n_vocab) {
    __shared__ int s_best;
    const int u = blockIdx.x, tid = threadIdx.x;
    if (u == 0 && tid == 0) *step_dev += 1;
    int n = length[u];
    n = n < 1 ? 1 : (n > cap ? cap : n);
    const int64_t* row = tokens + (size_t)u * tok_ld;
    int start = -1;                                   // index of the first token to draft
    if (drafts == nullptr) {
        for (int ng = ngram_max < n - 1 ? ngram_max : n - 1; ng >= 1; --ng) {
            if (tid == 0) s_best = -1;
            __syncthreads();
            int best = -1;
            for (int i = tid; i + ng < n; i += 256) {       // an occurrence at i is followed by tokens[i + ng]
                bool ok = true;
                for (int k = 0; k < ng; ++k) ok = ok && row[i + k] == row[n - ng + k];
                if (ok) best = i;
            }
            if (best >= 0) atomicMax(&s_best, best);
            __syncthreads();
            const int b = s_best;
            __syncthreads();
            if (b >= 0) { start = b + ng; break; }
        }
    }
    if (tid < S) {
        const int j = tid;
        int64_t id = row[n - 1];
        if (j > 0) {
            if (drafts != nullptr) {
                const int i = n - 1 + j - (limit[u] - max_new);
                if (i >= 0 && i < max_new) id = drafts[(size_t)u * max_new + i];
            } else if (start >= 0) {
                const int i = start + j - 1;
                id = row[i < n - 1 ? i : n - 1];
            }
            if (id < 0 || id >= n_vocab) id = row[n - 1];
        }
        const int r = u * S + j, pj = n - 1 + j;
        ids[r] = id;
        tok_slot[r] = u;
        tok_pos[r] = pj < cap ? pj : cap - 1;
        if (j == 0) kv_len[u] = n;
    }
}

__global__ void set_i32_kernel(int32_t* p, int32_t v) { *p = v; }
__global__ void iota_i32_kernel(int32_t* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

__global__ void gather_rows_kernel(const bf16_t* __restrict__ src, const int32_t* __restrict__ rows,
                                   bf16_t* __restrict__ dst, int n, int d) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n) return;
    const uint4* s = reinterpret_cast<const uint4*>(src + (size_t)rows[wave] * d);
    uint4* t = reinterpret_cast<uint4*>(dst + (size_t)wave * d);
    for (int c = lane; c < d / 8; c += 64) t[c] = s[c];
}
// Fork of a KV prefix (dh_engine_copy_prefix): the first n_pos / 32 tiles of src_slot's (layer, cache, group) blocks, one contiguous
// run of run16 16-byte units from the start of each block (common.h: 32-key tiles back to back), to the same place of every slot in
// dst_slots.  grid (pieces of 256 units, 2 L tables x groups, shares of the destination list); a thread loads its unit once and
// stores it to each destination of the block's share — all of them, unless the host split the list to fill the chip.
// block_elems = s_max * hs; the host has checked the slots against max_batch and run16 * 8 <= block_elems.
__global__ __launch_bounds__(256) void kv_copy_prefix_kernel(bf16_t* const* __restrict__ cache_tab, const int32_t* __restrict__ dst_slots,
                                                             int n_dst, int dst_per_block, int src_slot, int n_groups,
                                                             size_t block_elems, int run16) {
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (unit >= run16) return;
    const int tab = blockIdx.y / n_groups, g = blockIdx.y % n_groups;
    // a pointer read from memory has no known address space: said to be global, the accesses are global_load / global_store_dwordx4
    typedef __attribute__((address_space(1))) bf16_t gbf16_t;
    typedef __attribute__((address_space(1))) i32x4 gi32x4;
    gbf16_t* base = (gbf16_t*)cache_tab[tab] + (size_t)g * block_elems + (size_t)unit * 8;
    const size_t slot_elems = (size_t)n_groups * block_elems;
    const i32x4 v = *(const gi32x4*)(base + (size_t)src_slot * slot_elems);
    const int d0 = blockIdx.z * dst_per_block, d1 = min(d0 + dst_per_block, n_dst);
    for (int i = d0; i < d1; ++i) *(gi32x4*)(base + (size_t)dst_slots[i] * slot_elems) = v;
}

// Fork of every utterance's prompt cache into its decode slots (dh_engine_fork_slots): slot u * n_copies is utterance u's source; the
// tiles 0 .. ceil(plen[u] / 32) - 1 of its (layer, cache, group) blocks — one contiguous run from the start of each block, tile_units
// 16-byte units per tile — go to the same place of slots u * n_copies + 1 .. u * n_copies + n_copies - 1.  grid (pieces of 256 units
// of the longest prompt's tiles, 2 L tables x groups, utterances x shares of the n_copies - 1 destinations): sized by the host's
// maximum, what there is to do is read from the device — a block whose units lie behind its utterance's last tile returns, and the
// tile count is clamped to the cache_tiles of a block, as beam_reparent_kernel clamps.  A thread loads its unit once and stores it to
// each destination of the block's share.  The host has checked n_utt * n_copies against max_batch.
__global__ __launch_bounds__(256) void kv_fork_slots_kernel(bf16_t* const* __restrict__ cache_tab, const int32_t* __restrict__ plen,
                                                            int n_copies, int shares, int dst_per_block, int n_groups,
                                                            size_t block_elems, int tile_units, int cache_tiles) {
    const int u = blockIdx.z / shares, share = blockIdx.z % shares;
    const int P = plen[u];
    if (P < 1) return;
    int nt = ((P - 1) >> 5) + 1;
    nt = nt < cache_tiles ? nt : cache_tiles;                         // never past the (slot, group) block
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (unit >= nt * tile_units) return;
    const int tab = blockIdx.y / n_groups, g = blockIdx.y % n_groups;
    typedef __attribute__((address_space(1))) bf16_t gbf16_t;
    typedef __attribute__((address_space(1))) i32x4 gi32x4;
    const size_t slot_elems = (size_t)n_groups * block_elems;
    gbf16_t* src = (gbf16_t*)cache_tab[tab] + (size_t)u * n_copies * slot_elems + (size_t)g * block_elems + (size_t)unit * 8;
    const i32x4 v = *(const gi32x4*)src;
    const int d0 = 1 + share * dst_per_block, d1 = min(d0 + dst_per_block, n_copies);
    for (int j = d0; j < d1; ++j) *(gi32x4*)(src + (size_t)j * slot_elems) = v;
}

// The ids of a beam step (dh_engine_decode_beam): row u * W + w feeds beam_tok[u, t - 1, w] at position prompt_len[u] + t - 1 in slot
// u * W + w, t = n_steps[u] — the step about to be taken for a live utterance; a finished one's rows write the position behind their
// last one again, the same bits every time.  t, the prompt length and the position are clamped to the records, the cache and the rope
// table, an id to the embedding table: nothing is trusted to index.
__global__ void beam_prep_kernel(const int32_t* __restrict__ beam_tok, const int32_t* __restrict__ n_steps,
                                 const int32_t* __restrict__ plen, int W, int max_new, int64_t* __restrict__ ids,
                                 int32_t* __restrict__ tok_slot, int32_t* __restrict__ tok_pos, int32_t* __restrict__ kv_len,
                                 int32_t* step_dev, int n_rows, int cap, int n_vocab) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r == 0) *step_dev += 1;
    if (r < n_rows) {
        const int u = r / W, w = r % W;
        int t = n_steps[u], P = plen[u];
        t = t < 1 ? 1 : (t > max_new ? max_new : t);
        P = P < 1 ? 1 : P;
        int pos = P + t - 1;
        pos = pos < cap ? pos : cap - 1;
        int id = beam_tok[((size_t)u * max_new + t - 1) * W + w];
        id = id < 0 || id >= n_vocab ? 0 : id;
        ids[r] = id;
        tok_slot[r] = r;
        tok_pos[r] = pos;
        kv_len[r] = pos + 1;
    }
}

// KV re-parenting of a beam step: behind the selection of step t, slot u * W + w must hold the cache of slot u * W + parent,
// parent = beam_parent[u, t, w], in the tiles prompt_len[u] / 32 .. (prompt_len[u] + t - 1) / 32 that hold generated keys (32-key tiles
// back to back from the start of a (slot, group) block, tile_units 16-byte units each).  Two launches of this kernel through the
// engine's scratch — to_scratch: the parent's tiles into the row's own scratch block; then: that block into the row's own slot — so
// no launch reads what it writes and any parent map is right.  grid (pieces of 256 units of the nt_max tiles, 2 L tables x groups,
// rows): fixed, what there is to do is read from the device.  A row that continues itself, an utterance that did not take step t
// (n_steps[u] != t + 1: finished before) and units behind the row's last tile return at once.
__global__ __launch_bounds__(256) void beam_reparent_kernel(bf16_t* const* __restrict__ cache_tab, bf16_t* __restrict__ scratch,
                                                            const int32_t* __restrict__ beam_parent, const int32_t* __restrict__ n_steps,
                                                            const int32_t* __restrict__ plen, const int32_t* __restrict__ step_dev, int W,
                                                            int max_new, int n_groups, size_t block_elems, int tile_units, int nt_max,
                                                            int cache_tiles, int to_scratch) {
    const int row = blockIdx.z, u = row / W, w = row % W;
    const int step = *step_dev;
    if (step < 1 || step >= max_new || n_steps[u] != step + 1) return;
    const int parent = beam_parent[((size_t)u * max_new + step) * W + w];
    if (parent == w || parent < 0 || parent >= W) return;
    const int P = plen[u];
    if (P < 1) return;
    const int tile0 = P >> 5;
    int nt = ((P + step - 1) >> 5) - tile0 + 1;
    nt = nt < nt_max ? nt : nt_max;
    nt = nt < cache_tiles - tile0 ? nt : cache_tiles - tile0;         // never past the (slot, group) block
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (unit >= nt * tile_units) return;
    const int g = blockIdx.y % n_groups;
    typedef __attribute__((address_space(1))) bf16_t gbf16_t;
    typedef __attribute__((address_space(1))) i32x4 gi32x4;
    gbf16_t* cache = (gbf16_t*)cache_tab[blockIdx.y / n_groups] + (size_t)g * block_elems + ((size_t)tile0 * tile_units + unit) * 8;
    const size_t slot_elems = (size_t)n_groups * block_elems;
    gbf16_t* sc = (gbf16_t*)scratch + (((size_t)row * gridDim.y + blockIdx.y) * nt_max * tile_units + unit) * 8;
    if (to_scratch) *(gi32x4*)sc = *(const gi32x4*)(cache + (size_t)(u * W + parent) * slot_elems);
    else *(gi32x4*)(cache + (size_t)row * slot_elems) = *(const gi32x4*)sc;
}

// dst[i, :] = src[last_row[i], :] for the n_seq sequences of the call
int gather_last_rows(dh_engine* e, const bf16_t* src, bf16_t* dst, int n_seq, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(n_seq, 4)), dim3(256), 0, s, src, e->last_row, dst, n_seq, e->d.n_embd);
    DH_LAUNCH_CHECK();
    return 0;
}

// ---- timing + the dense products ---------------------------------------------------------------------------------------------
// Event pair around what is launched while the object lives (class `which`: 0 prefill GEMMs, 1 decode GEMMs, 2 prefill attention,
// 3 decode attention); nothing when `on` is false, when timing is off or inside a stream capture.
struct TimeScope {
    dh_engine* e; int which; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    TimeScope(dh_engine* e_, int w, hipStream_t s_, bool on = true) : e(e_), which(w), s(s_) {
        if (!on || !e->tm.on || e->capturing) return;
        hipEventCreate(&a); hipEventCreate(&b);
        hipEventRecord(a, s);
    }
    ~TimeScope() {
        if (!a) return;
        hipEventRecord(b, s);
        e->tm.ev[which].push_back({a, b});
    }
};

// kernel choice is a property of the phase, never of the packing (batch invariance)
int phase_kernel(const dh_engine* e) { return e->phase_decode && !e->decode_tiled ? 2 : 1; }
int gemm_class(const dh_engine* e) { return e->phase_decode ? 1 : 0; }

// The bf16 products by epilogue, each ONE launch on the phase's kernel, in the phase's GEMM timing class when `timed`.
// y = x . w^T [+ resid]
int plain(dh_engine* e, const bf16_t* x, const bf16_t* w, bf16_t* y, int M, int N, int K, const bf16_t* resid, hipStream_t s,
          bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    return dh_linear_impl(x, w, y, M, N, K, DH_EPI_PLAIN, nullptr, nullptr, 0, nullptr, e->d.lora_scale, 0, 0, nullptr, nullptr, resid,
                          phase_kernel(e), s);
}
// y = silu(x . w_gate^T) * (x . w_up^T)
int swiglu(dh_engine* e, const bf16_t* x, const bf16_t* w_gate, const bf16_t* w_up, bf16_t* y, int M, int N, int K, hipStream_t s,
           bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    return dh_linear_impl(x, w_gate, y, M, N, K, DH_EPI_SWIGLU, w_up, nullptr, 0, nullptr, e->d.lora_scale, 0, 0, nullptr, nullptr,
                          nullptr, phase_kernel(e), s);
}
// y = x . w^T + scale * xa . lora_b^T per column segment [0, split0) / [split0, split1) / [split1, N), xa = x . A^T already computed
int lora(dh_engine* e, const bf16_t* x, const bf16_t* w, bf16_t* y, int M, int N, int K, const bf16_t* xa, int xa_ld,
         const bf16_t* lora_b, int split0, int split1, hipStream_t s, bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    return dh_linear_impl(x, w, y, M, N, K, DH_EPI_LORA, nullptr, xa, xa_ld, lora_b, e->d.lora_scale, split0, split1, nullptr, nullptr,
                          nullptr, phase_kernel(e), s);
}
// the same for one segment, + resid, with x . A^T left to the library: in the GEMM's K loop where the launch runs on the 4-wave
// 256-tile kernel, else a launch of its own into e->xa (same bits)
int lora_resid(dh_engine* e, const bf16_t* x, const bf16_t* w, bf16_t* y, int M, int N, int K, const bf16_t* lora_a,
               const bf16_t* lora_b, const bf16_t* resid, hipStream_t s, bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    return dh_linear_lora_impl(x, w, y, M, N, K, lora_a, lora_b, e->d.lora_scale, N, N, resid, e->xa, phase_kernel(e), s);
}
// y = (x . w^T) * vec_a + vec_b (the lm_head with the logit adapter)
int adapter(dh_engine* e, const bf16_t* x, const bf16_t* w, bf16_t* y, int M, int N, int K, const bf16_t* vec_a, const bf16_t* vec_b,
            hipStream_t s, bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    return dh_linear_impl(x, w, y, M, N, K, DH_EPI_ADAPTER, nullptr, nullptr, 0, nullptr, e->d.lora_scale, 0, 0, vec_a, vec_b, nullptr,
                          phase_kernel(e), s);
}

// fp8 GEMM kernel by PHASE, never by packing (the two kernels sum K in different fp32 orders): a prefill is tiled even
// when a short prompt runs alone; a single-token step streams the weights up to 128 rows (the bench's four batches per
// decode loop) and is tiled above that — the one documented class boundary of the fp8 decode phase.
inline int fp8_kernel(bool decode, int rows) { return decode && rows <= 128 ? 2 : 1; }

// fp8 product of the M quantised rows in e->xq / e->xscale; the weight pointers of dh_layer_weights address e4m3 bytes in this mode
int linear_fp8(dh_engine* e, const bf16_t* w, const float* ws, bf16_t* y, int M, int N, int K, int epi, const bf16_t* w2,
               const float* w2s, const bf16_t* resid, hipStream_t s, bool timed) {
    TimeScope t(e, gemm_class(e), s, timed);
    if (e->a6)    // MXFP6 activations beside the MXFP4 block weights: the rows are in e->xq6 / e->xs6; same phase rule
        return dh_linear_mxfp4a6_ex(e->xq6, e->xs6, reinterpret_cast<const uint8_t*>(w), reinterpret_cast<const uint8_t*>(ws), y, M, N, K,
                                    epi, reinterpret_cast<const uint8_t*>(w2), reinterpret_cast<const uint8_t*>(w2s), nullptr, nullptr,
                                    resid, fp8_kernel(e->phase_decode, M), s);
    if (e->mx4)   // the block linears of an MXFP4 engine: w addresses nibbles, ws E8M0 bytes; same phase rule
        return dh_linear_mxfp4_ex(e->xq, e->xscale, reinterpret_cast<const uint8_t*>(w), reinterpret_cast<const uint8_t*>(ws), y, M, N, K,
                                  epi, reinterpret_cast<const uint8_t*>(w2), reinterpret_cast<const uint8_t*>(w2s), nullptr, nullptr,
                                  resid, fp8_kernel(e->phase_decode, M), s);
    return dh_linear_fp8_ex(e->xq, e->xscale, reinterpret_cast<const uint8_t*>(w), ws, y, M, N, K, epi,
                            reinterpret_cast<const uint8_t*>(w2), w2s, nullptr, nullptr, resid, fp8_kernel(e->phase_decode, M), s);
}

// the quantisation points of a block: e4m3 rows + token scales into e->xq / e->xscale, or MXFP6 blocks into e->xq6 / e->xs6
int quant_act(dh_engine* e, const bf16_t* x, int rows, int K, hipStream_t s) {
    return e->a6 ? dh_quant_rows_mxfp6(x, e->xq6, e->xs6, rows, K, s) : dh_quant_rows_fp8(x, e->xq, e->xscale, rows, K, s);
}
int norm_quant_act(dh_engine* e, const bf16_t* x, const bf16_t* w, int rows, int d, const uint8_t* rt, hipStream_t s) {
    return e->a6 ? dh_rmsnorm_quant_mxfp6(x, w, nullptr, e->xq6, e->xs6, rows, d, e->d.norm_eps, rt, s)
                 : dh_rmsnorm_quant_fp8(x, w, nullptr, e->xq, e->xscale, rows, d, e->d.norm_eps, rt, s);
}

// ---- the pieces of a layer ---------------------------------------------------------------------------------------------------
// rope + append to layer l's KV cache (quantised into the fp8 cache of a kv8 engine) of the n_tok rows of e->qkv; the rotated queries
// land in e->qrot
int rope_append(dh_engine* e, int l, int n_tok, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const size_t co = (size_t)l * e->cache_layer_elems, eo = (size_t)l * e->exp_layer_elems;
    if (e->kv8)
        return dh_qkv_rope_cache_kv8(e->qkv, D.rope_cos, D.rope_sin, e->tok_slot, e->tok_pos, e->qrot, e->k8 + co, e->v8 + co, e->ke + eo,
                                     e->ve + eo, n_tok, D.n_head, D.n_groups, D.head_size, e->s_max, s);
    return dh_qkv_rope_cache_bf16(e->qkv, D.rope_cos, D.rope_sin, e->tok_slot, e->tok_pos, e->qrot, e->kc + co, e->vtc + co, nullptr, nullptr,
                                  n_tok, D.n_head, D.n_groups, D.head_size, e->s_max, s);
}

// Attention of e->qrot over layer l's cache into e->att: the split-KV kernel of a single-token step or the prefill kernel.
// last_rows (last block of a call that wants the last position's logits only, g_prune_last_layer): attention of each sequence's LAST
// query alone (a one-row tile at position pos0 + len - 1 over the same 64-key steps as in the full call); its n_seq output rows are
// then gathered into e->att_last and the block's input rows into e->xlast, where the block's n_seq-row second half continues.
// fp8 KV cache: a single-token step runs the split-KV kernel over the fp8 cache; for a prompt the call's sequences are expanded into
// the one-layer bf16 scratch (e->kc / e->vtc) first, positions [0, kv_pos0 + q_len), and the prefill kernel runs on that — inside the
// prefill attention's timing class.
int attention(dh_engine* e, int l, int n_seq, int max_q_len, bool last_rows, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const int hs = D.head_size, H = D.n_head, G = D.n_groups;
    const SeqMeta m = seq_meta(e);
    const size_t co = (size_t)l * e->cache_layer_elems, eo = (size_t)l * e->exp_layer_elems;
    const bf16_t *kc = e->kv8 ? e->kc : e->kc + co, *vtc = e->kv8 ? e->vtc : e->vtc + co;
    int rc;
    if (e->phase_decode) {
        TimeScope t(e, 3, s);
        if (e->kv8)
            return dh_attn_decode_kv8(e->qrot, e->k8 + co, e->v8 + co, e->ke + eo, e->ve + eo, m.seq_slot, m.kv, e->att, e->dec_work, n_seq, H,
                                      G, hs, e->s_max, s);
        return dh_attn_decode_bf16(e->qrot, kc, vtc, m.seq_slot, m.kv, e->att, e->dec_work, n_seq, H, G, hs, e->s_max, s);
    }
    if (e->kv8) {
        TimeScope t(e, 2, s);
        if ((rc = dh_kv8_expand(e->k8 + co, e->v8 + co, e->ke + eo, e->ve + eo, m.seq_slot, m.kv, m.q_len, e->kc, e->vtc, n_seq, G, hs,
                                e->s_max, s))) return rc;
    }
    if (last_rows) {
        {
            TimeScope t(e, 2, s);
            if ((rc = dh_attn_prefill_bf16(e->qrot, kc, vtc, m.seq_slot, e->last_row, e->last_meta, e->last_meta + e->max_batch, e->att,
                                           nullptr, n_seq, 1, H, G, hs, e->s_max, s))) return rc;
        }
        if ((rc = gather_last_rows(e, e->att, e->att_last, n_seq, s))) return rc;
        return gather_last_rows(e, e->x, e->xlast, n_seq, s);
    }
    TimeScope t(e, 2, s);
    return dh_attn_prefill_bf16(e->qrot, kc, vtc, m.seq_slot, m.q_start, m.q_len, m.kv, e->att, nullptr, n_seq, max_q_len, H, G, hs,
                                e->s_max, s);
}

// The half of a block behind the attention, in place on `rows` rows: x += proj(att), x += mlp_proj(swiglu(norm_2(x))).  Called on
// every row of the call with timed = true, or on the last rows of the last block (attention() above) with timed = false: those
// n_seq-row launches stream the weights, they are not in the timed class of the large prefill GEMMs, and bench.py does not count their
// FLOPs either.  A last-rows call is a prefill (its longest sequence has more than one token), so both run the tiled kernel.
int post_attention(dh_engine* e, const dh_layer_weights& W, int rows, const bf16_t* att, bf16_t* x, bf16_t* xn, bf16_t* act,
                   const uint8_t* rt, bool timed, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const int d = D.n_embd, I = D.intermediate;
    int rc;
    if ((rc = W.proj_lora_a ? lora_resid(e, att, W.proj_w, x, rows, d, d, W.proj_lora_a, W.proj_lora_b, x, s, timed)
                            : plain(e, att, W.proj_w, x, rows, d, d, x, s, timed))) return rc;
    if ((rc = dh_rmsnorm_bf16(x, nullptr, W.norm_2, xn, nullptr, rows, d, D.norm_eps, rt, s))) return rc;
    if ((rc = swiglu(e, xn, W.fc_1, W.fc_2, act, rows, I, d, s, timed))) return rc;
    return plain(e, act, W.mlp_proj, x, rows, d, I, x, s, timed);
}

// The same in fp8 mode: the activations are quantised per row into e->xq / e->xscale in front of every product (by the norm kernel,
// or by a pass over the attention / SwiGLU output), so a row keeps its bits whichever rows run with it.
int post_attention_fp8(dh_engine* e, const dh_layer_weights& W, int rows, const bf16_t* att, bf16_t* x, bf16_t* act, const uint8_t* rt,
                       bool timed, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const int d = D.n_embd, I = D.intermediate;
    int rc;
    if ((rc = quant_act(e, att, rows, d, s))) return rc;
    if ((rc = linear_fp8(e, W.proj_w, W.proj_ws, x, rows, d, d, DH_EPI_PLAIN, nullptr, nullptr, x, s, timed))) return rc;
    if ((rc = norm_quant_act(e, x, W.norm_2, rows, d, rt, s))) return rc;
    if ((rc = linear_fp8(e, W.fc_1, W.fc_1_ws, act, rows, I, d, DH_EPI_SWIGLU, W.fc_2, W.fc_2_ws, nullptr, s, timed))) return rc;
    if ((rc = quant_act(e, act, rows, I, s))) return rc;
    return linear_fp8(e, W.mlp_proj, W.mlp_proj_ws, x, rows, d, I, DH_EPI_PLAIN, nullptr, nullptr, x, s, timed);
}

// ---- the layer stacks --------------------------------------------------------------------------------------------------------
// The layer stack on n_tok packed tokens whose metadata is already on the device.
// prefill: attention over (seq_slot, q_start, q_len, kv_pos0); decode: one token per sequence.
// prune_last: the last block finishes on the n_seq last rows; their final hidden rows land in e->xlast (where the caller would have
// gathered them) and e->x keeps that block's input.
int run_layers(dh_engine* e, const int64_t* ids, int n_tok, int n_seq, int max_q_len, bool decode, const uint8_t* tail_flags,
               bool prune_last, hipStream_t s) {
    const uint8_t* rt = e->rsqrt_vec > 0 ? tail_flags : nullptr;
    const uint8_t* rtl = e->rsqrt_vec > 0 ? e->last_tail : nullptr;
    e->phase_decode = decode;
    const dh_model_desc& D = e->d;
    const int d = D.n_embd, hs = D.head_size, H = D.n_head, G = D.n_groups;
    int rc;
    if ((rc = dh_embed_bf16(ids, D.wte, e->x, n_tok, d, D.wte_rows, s))) return rc;
    for (int l = 0; l < D.n_layer; ++l) {
        const dh_layer_weights& W = e->layers[l];
        bf16_t* kc = e->kc + (size_t)l * e->cache_layer_elems;
        bf16_t* vtc = e->vtc + (size_t)l * e->cache_layer_elems;
        if ((rc = dh_rmsnorm_bf16(e->x, nullptr, W.norm_1, e->xn, nullptr, n_tok, d, D.norm_eps, rt, s))) return rc;
        // large packed prefills: rope + KV append ride in the QKV GEMM's epilogue (same bits, no pass over the qkv tensor)
        // (not at head size 96: a 96-wide head straddles the 256-column tiles of that epilogue, gemm.hip)
        const bool fuse_qkv = !decode && g_fuse_qkv_rope && hs != 96 && dh_linear_is_big(n_tok, e->qkv_dim, DH_EPI_LORA);
        if (fuse_qkv) {
            // x.A^T: inside the QKV GEMM's K loop (dh_linear_qkv_lora_rope_cache_bf16 decides)
            TimeScope t(e, 0, s);
            if (W.attn_lora_a) {
                if ((rc = dh_linear_qkv_lora_rope_cache_bf16(e->xn, W.attn_w, n_tok, d, W.attn_lora_a, W.attn_lora_b, D.lora_scale,
                                                             D.rope_cos, D.rope_sin, e->tok_slot, e->tok_pos, e->qrot, kc, vtc, H, G,
                                                             hs, e->s_max, e->xa, s))) return rc;
            } else if ((rc = dh_linear_qkv_rope_cache_bf16(e->xn, W.attn_w, n_tok, d, nullptr, 48, nullptr, D.lora_scale, D.rope_cos,
                                                           D.rope_sin, e->tok_slot, e->tok_pos, e->qrot, kc, vtc, H, G, hs,
                                                           e->s_max, s))) return rc;
        } else {
            if (W.attn_lora_a) {   // x.A^T is a launch of its own here, outside the timed class
                if ((rc = plain(e, e->xn, W.attn_lora_a, e->xa, n_tok, 48, d, nullptr, s, false))) return rc;
                if ((rc = lora(e, e->xn, W.attn_w, e->qkv, n_tok, e->qkv_dim, d, e->xa, 48, W.attn_lora_b, d, d + e->kv_dim, s, true)))
                    return rc;
            } else if ((rc = plain(e, e->xn, W.attn_w, e->qkv, n_tok, e->qkv_dim, d, nullptr, s, true))) return rc;
            if ((rc = rope_append(e, l, n_tok, s))) return rc;
        }
        const bool last_rows = prune_last && l == D.n_layer - 1;
        if ((rc = attention(e, l, n_seq, max_q_len, last_rows, s))) return rc;
        if (last_rows) return post_attention(e, W, n_seq, e->att_last, e->xlast, e->xn_last, e->act_last, rtl, false, s);
        if ((rc = post_attention(e, W, n_tok, e->att, e->x, e->xn, e->act, rt, true, s))) return rc;
    }
    return 0;
}

// fp8 serving: the same layer sequence with every dense product on the fp8 MFMA (csrc/fp8.hip).  Activations are
// quantised per token right where they are produced (the norm kernels) or by a pass over the attention / SwiGLU
// output; LoRA is merged into the weights before quantisation, so there is no rank-16 side product.  Prefill and
// decode run the same sequence; the GEMM kernel is pinned by phase (fp8_kernel above).
int run_layers_fp8(dh_engine* e, const int64_t* ids, int n_tok, int n_seq, int max_q_len, bool decode, const uint8_t* tail_flags,
                   bool prune_last, hipStream_t s) {
    const uint8_t* rt = e->rsqrt_vec > 0 ? tail_flags : nullptr;
    const uint8_t* rtl = e->rsqrt_vec > 0 ? e->last_tail : nullptr;
    e->phase_decode = decode;
    const dh_model_desc& D = e->d;
    const int d = D.n_embd, hs = D.head_size, H = D.n_head, G = D.n_groups;
    int rc;
    if ((rc = dh_embed_bf16(ids, D.wte, e->x, n_tok, d, D.wte_rows, s))) return rc;
    for (int l = 0; l < D.n_layer; ++l) {
        const dh_layer_weights& W = e->layers[l];
        bf16_t* kc = e->kc + (size_t)l * e->cache_layer_elems;
        bf16_t* vtc = e->vtc + (size_t)l * e->cache_layer_elems;
        if ((rc = norm_quant_act(e, e->x, W.norm_1, n_tok, d, rt, s))) return rc;
        if (!e->kv8 && decode && n_tok <= 128) {     // every streaming-class step over a bf16 cache (fp8_kernel above): one family, no 32-row boundary
            // one launch for rope + cache append + split-KV attention + combine (decode_fused.hip): the QKV product
            // is handed over as its single fp32 "partial" (values already rounded to bf16), no LoRA (merged)
            const SeqMeta m = seq_meta(e);
            {
                TimeScope t(e, 1, s);
                if (e->a6) rc = dh_linear_mxfp4a6_f32(e->xq6, e->xs6, reinterpret_cast<const uint8_t*>(W.attn_w),
                                                      reinterpret_cast<const uint8_t*>(W.attn_ws), e->part32, n_tok, e->qkv_dim, d, s);
                else if (e->mx4) rc = dh_linear_mxfp4_f32(e->xq, e->xscale, reinterpret_cast<const uint8_t*>(W.attn_w),
                                                     reinterpret_cast<const uint8_t*>(W.attn_ws), e->part32, n_tok, e->qkv_dim, d, s);
                else rc = dh_linear_fp8_f32(e->xq, e->xscale, reinterpret_cast<const uint8_t*>(W.attn_w), W.attn_ws, e->part32,
                                            n_tok, e->qkv_dim, d, s);
                if (rc) return rc;
            }
            TimeScope t(e, 3, s);
            if ((rc = dh_attn_decode_fused_bf16(e->part32, 1, 0, n_seq, e->qkv_dim, 0, nullptr, 0.f, e->qkv_dim, e->qkv_dim,
                                                D.rope_cos, D.rope_sin, m.seq_slot, m.kv, kc, vtc, e->att, H, G, hs,
                                                e->s_max, s))) return rc;
        } else {   // QKV GEMM by the phase rule, (quantised) append, attention over the layer's cache
            if ((rc = linear_fp8(e, W.attn_w, W.attn_ws, e->qkv, n_tok, e->qkv_dim, d, DH_EPI_PLAIN, nullptr, nullptr, nullptr, s, true)))
                return rc;
            if ((rc = rope_append(e, l, n_tok, s))) return rc;
            // the last block of a prompt forward that wants the last position's logits only stays on the phase's (tiled) kernel
            const bool last_rows = prune_last && l == D.n_layer - 1;
            if ((rc = attention(e, l, n_seq, max_q_len, last_rows, s))) return rc;
            if (last_rows) return post_attention_fp8(e, W, n_seq, e->att_last, e->xlast, e->act_last, rtl, false, s);
        }
        if ((rc = post_attention_fp8(e, W, n_tok, e->att, e->x, e->act, rt, true, s))) return rc;
    }
    return 0;
}

// K-slices of 8 (or 16 for long K) k-steps: the row-parallel streaming kernel (gemm_skinny.hip)
int pick_ksplit(int nks) {
    if (nks <= 128) return g_short_kps == 16 && nks % 16 == 0 ? nks / 16 : (nks + 7) / 8;
    if (nks <= 256) return (nks + 15) / 16;
    int ks = 1;
    while (ks < 4 && nks / (16 * ks) >= 2) ks *= 2;
    return ks;
}

// Single-token step for n_seq <= MAX_DECODE_ROWS sequences: 7 launches per layer (decode_fused.hip).  Leaves
// ln_f(x) in e->xn.
// spec_S > 1 (a verify step, dh_engine_decode_spec): the n_seq rows are spec_S consecutive positions of n_seq / spec_S sequences; the
// linears are the same launches over the same rows, the attention is attn_verify_fused_kernel over the sequences.
int run_layers_decode(dh_engine* e, const int64_t* ids, int n_seq, const uint8_t* tail_flags, hipStream_t s, int spec_S = 1) {
    const dh_model_desc& D = e->d;
    const int d = D.n_embd, I = D.intermediate, hs = D.head_size, H = D.n_head, G = D.n_groups;
    const uint8_t* rt = e->rsqrt_vec > 0 ? tail_flags : nullptr;
    const SeqMeta m = seq_meta(e);
    e->phase_decode = true;
    int rc;
    if ((rc = dh_embed_bf16(ids, D.wte, e->x, n_seq, d, D.wte_rows, s))) return rc;
    if ((rc = dh_rmsnorm_bf16(e->x, nullptr, e->layers[0].norm_1, e->xn, nullptr, n_seq, d, D.norm_eps, rt, s))) return rc;
    for (int l = 0; l < D.n_layer; ++l) {
        const dh_layer_weights& W = e->layers[l];
        bf16_t* kc = e->kc + (size_t)l * e->cache_layer_elems;
        bf16_t* vtc = e->vtc + (size_t)l * e->cache_layer_elems;
        // every partial-sum GEMM: the total in one launch (chain), the pair sums from the tiled split-K kernel (more than
        // 128 rows), or the K-slices from the streaming kernel — all in the family's one combine order (dualhyp_hip.h)
        auto partial = [&](const bf16_t* xin, const bf16_t* w, const bf16_t* wext, int N, int ext, int K, int ks, int& np, int& pairs) {
            if (dh_chain_ok(n_seq, N, ext, K, ks)) { np = 1; pairs = 0; return dh_linear_chain_bf16(xin, w, wext, e->part32, n_seq, N, ext, K, ks, s); }
            if (dh_pairs_ok(n_seq, N, ext, K, ks)) { np = (ks + 1) / 2; pairs = 0; return dh_linear_partial_pairs_bf16(xin, w, wext, e->part32, n_seq, N, ext, K, ks, s); }
            np = ks; pairs = 1;
            return dh_linear_partial_bf16(xin, w, wext, e->part32, n_seq, N, ext, K, ks, s);
        };
        int np, pairs;
        const int ext1 = W.attn_lora_a ? 48 : 0;
        if ((rc = partial(e->xn, W.attn_w, W.attn_lora_a, e->qkv_dim, ext1, d, pick_ksplit(d / 32), np, pairs))) return rc;
        if (spec_S > 1) {
            const int p_max = e->s_max < D.block_size ? e->s_max : D.block_size;
            if ((rc = dh_attn_verify_fused_impl(e->part32, np, pairs, n_seq / spec_S, spec_S, e->qkv_dim, ext1, W.attn_lora_b, D.lora_scale,
                                                d, d + e->kv_dim, D.rope_cos, D.rope_sin, m.seq_slot, m.kv, kc, vtc, e->att, H, G, hs,
                                                e->s_max, p_max, s))) return rc;
        } else if (e->step_shared_rows && e->step_beam_tab) {
            if ((rc = dh_attn_decode_shared_tab_bf16(e->part32, np, pairs, n_seq, e->qkv_dim, ext1, W.attn_lora_b, D.lora_scale, d,
                                                     d + e->kv_dim, D.rope_cos, D.rope_sin, m.seq_slot, m.kv, kc, vtc, e->att, H, G, hs,
                                                     e->s_max, e->step_shared_rows, e->step_shared_plen, e->step_beam_tab,
                                                     e->step_beam_tab_nt, e->step_dev, s))) return rc;
        } else if (e->step_shared_rows) {
            if ((rc = dh_attn_decode_shared_bf16(e->part32, np, pairs, n_seq, e->qkv_dim, ext1, W.attn_lora_b, D.lora_scale, d,
                                                 d + e->kv_dim, D.rope_cos, D.rope_sin, m.seq_slot, m.kv, kc, vtc, e->att, H, G, hs,
                                                 e->s_max, e->step_shared_rows, e->step_shared_plen, s))) return rc;
        } else
        if ((rc = dh_attn_decode_fused_bf16(e->part32, np, pairs, n_seq, e->qkv_dim, ext1, W.attn_lora_b, D.lora_scale, d,
                                            d + e->kv_dim, D.rope_cos, D.rope_sin, m.seq_slot, m.kv, kc, vtc, e->att, H, G,
                                            hs, e->s_max, s))) return rc;
        const int ext2 = W.proj_lora_a ? 16 : 0;
        if ((rc = partial(e->att, W.proj_w, W.proj_lora_a, d, ext2, d, pick_ksplit(d / 32), np, pairs))) return rc;
        if ((rc = dh_finish_norm_bf16(e->part32, np, pairs, n_seq, d, ext2, W.proj_lora_b, D.lora_scale, e->x, W.norm_2, e->x,
                                      e->xn, D.norm_eps, rt, s))) return rc;
        if ((rc = swiglu(e, e->xn, W.fc_1, W.fc_2, e->act, n_seq, I, d, s, false))) return rc;
        if ((rc = partial(e->act, W.mlp_proj, nullptr, d, 0, I, pick_ksplit(I / 32), np, pairs))) return rc;
        const bf16_t* next_norm = l + 1 < D.n_layer ? e->layers[l + 1].norm_1 : D.ln_f;
        if ((rc = dh_finish_norm_bf16(e->part32, np, pairs, n_seq, d, 0, nullptr, 0.f, e->x, next_norm, e->x, e->xn,
                                      D.norm_eps, rt, s))) return rc;
    }
    return 0;
}

// ---- layers + logits ---------------------------------------------------------------------------------------------------------
// ln_f + lm_head of `rows` rows of `xrows`; the bf16 ln_f output lands in e->xn (test hook dh_engine_read(0)) in either precision.
// xrows == nullptr: the rows are in e->xn, normalised already (run_layers_decode).
int head(dh_engine* e, const bf16_t* xrows, int rows, bf16_t* logits, const uint8_t* tail_flags, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const uint8_t* rt = e->rsqrt_vec > 0 ? tail_flags : nullptr;
    int rc;
    if (e->fp8) {
        if ((rc = dh_rmsnorm_quant_fp8(xrows, D.ln_f, e->xn, e->xq, e->xscale, rows, D.n_embd, D.norm_eps, rt, s))) return rc;
        TimeScope t(e, gemm_class(e), s);
        return dh_linear_fp8_ex(e->xq, e->xscale, reinterpret_cast<const uint8_t*>(D.lm_head), D.lm_head_ws, logits, rows, D.vocab,
                                D.n_embd, DH_EPI_ADAPTER, nullptr, nullptr, D.adapter_scale, D.adapter_bias, nullptr,
                                fp8_kernel(e->phase_decode, rows), s);
    }
    if (xrows && (rc = dh_rmsnorm_bf16(xrows, nullptr, D.ln_f, e->xn, nullptr, rows, D.n_embd, D.norm_eps, rt, s))) return rc;
    return adapter(e, e->xn, D.lm_head, logits, rows, D.vocab, D.n_embd, D.adapter_scale, D.adapter_bias, s, true);
}

// The model on n_tok packed tokens of n_seq sequences whose ids and metadata are on the device: the layers on the path the call's
// class selects (fp8 / the streaming single-token step / tiled), then ln_f + lm_head on every row (logits_all), on each sequence's
// last row (logits_last), or both.  step: one token per sequence run as a decode step.  prune_last: logits_last alone is wanted and
// the last block ran on the last rows only.  row_flags / last_flags: the rsqrt tail flags of all rows / of the last rows.
int run_model(dh_engine* e, const int64_t* ids, int n_tok, int n_seq, int max_q, bool step, const uint8_t* row_flags,
              const uint8_t* last_flags, bool prune_last, bf16_t* logits_all, bf16_t* logits_last, hipStream_t s) {
    e->decode_tiled = step && g_decode_tiled_rows > 0 && n_seq >= g_decode_tiled_rows;
    const bool streaming = !e->fp8 && step && n_seq <= MAX_DECODE_ROWS && !e->decode_tiled;
    int rc;
    if (e->fp8) rc = run_layers_fp8(e, ids, n_tok, n_seq, max_q, step, row_flags, prune_last, s);
    else if (streaming) rc = run_layers_decode(e, ids, n_seq, row_flags, s);
    else rc = run_layers(e, ids, n_tok, n_seq, max_q, step, row_flags, prune_last, s);
    if (rc) return rc;
    if (prune_last) return head(e, e->xlast, n_seq, logits_last, last_flags, s);   // e->xlast: the last rows' final hidden state
    if (streaming) {   // every row is its sequence's last row, and e->xn holds ln_f of them
        if (logits_all && (rc = head(e, nullptr, n_seq, logits_all, nullptr, s))) return rc;
        return logits_last ? head(e, nullptr, n_seq, logits_last, nullptr, s) : 0;
    }
    if (logits_all && (rc = head(e, e->x, n_tok, logits_all, row_flags, s))) return rc;
    if (logits_last) {
        // head() overwrites xn[0 : n_seq], which is fine after logits_all
        if ((rc = gather_last_rows(e, e->x, e->xlast, n_seq, s))) return rc;
        return head(e, e->xlast, n_seq, logits_last, last_flags, s);
    }
    return 0;
}

// fp32 partial sums of a single-token step over `rows` rows: up to 16 K-slices of the widest product (the fused QKV + x·A^T)
size_t part32_elems(const dh_engine* e, int rows) {
    return (size_t)16 * (rows < 32 ? 32 : (rows < MAX_DECODE_ROWS ? rows : MAX_DECODE_ROWS)) * (e->qkv_dim + 48);
}

// The workspaces a single-token step sizes by its row count (logits, dec_ids, ones, part32).  engine_init and dh_engine_reserve_rows
// both allocate them here, so their sizes are written once.  The engine's pointers change only after all four allocations have
// succeeded: a failure leaves the engine, row_cap and dev_bytes as they were.  The caller has made sure nothing reads the old ones.
int alloc_row_ws(dh_engine* e, int rows) {
    decltype(e->logits) logits = nullptr;
    decltype(e->dec_ids) dec_ids = nullptr;
    decltype(e->ones) ones = nullptr;
    decltype(e->part32) part32 = nullptr;
    const int64_t before = e->dev_bytes;
    int rc = 0;
    rc |= dmalloc(e, &logits, (size_t)rows * e->d.vocab);
    rc |= dmalloc(e, &dec_ids, (size_t)rows);
    rc |= dmalloc(e, &ones, (size_t)rows);
    rc |= dmalloc(e, &part32, part32_elems(e, rows));
    if (!rc && hipMemset(ones, 1, (size_t)rows) != hipSuccess) rc = 2;
    if (rc) {
        hipFree(logits); hipFree(dec_ids); hipFree(ones); hipFree(part32);
        e->dev_bytes = before;
        return 2;
    }
    hipFree(e->logits); hipFree(e->dec_ids); hipFree(e->ones); hipFree(e->part32);
    e->logits = logits; e->dec_ids = dec_ids; e->ones = ones; e->part32 = part32;
    const int64_t bytes = e->dev_bytes - before;
    e->dev_bytes -= e->row_ws_bytes;
    e->row_ws_bytes = bytes;
    e->row_cap = rows;
    return 0;
}

int engine_init(dh_engine* e, const dh_model_desc* desc, int max_batch, int s_max, int max_tokens, int kv_dtype, int weight_dtype, int act_dtype) {
    e->d = *desc;
    e->layers.assign(desc->h_layers, desc->h_layers + desc->n_layer);
    e->d.h_layers = nullptr;
    e->max_batch = max_batch; e->s_max = s_max; e->max_tokens = max_tokens;
    const int d = desc->n_embd, hs = desc->head_size, G = desc->n_groups, H = desc->n_head;
    e->kv_dim = G * hs;
    e->qkv_dim = (H + 2 * G) * hs;
    e->fp8 = e->layers[0].attn_ws != nullptr;
    if (e->fp8) {
        for (const auto& L : e->layers)
            DH_CHECK(L.attn_ws && L.proj_ws && L.fc_1_ws && L.fc_2_ws && L.mlp_proj_ws && !L.attn_lora_a && !L.proj_lora_a,
                     "dh_engine_create: fp8 mode needs every channel-scale pointer and merged LoRA (no lora_a/lora_b)");
        DH_CHECK(desc->lm_head_ws != nullptr, "dh_engine_create: fp8 mode needs lm_head_ws");
        DH_CHECK(d % 128 == 0 && desc->intermediate % 128 == 0, "dh_engine_create: fp8 mode needs n_embd and intermediate %% 128 == 0");
    }
    e->mx4 = weight_dtype == 1;
    DH_CHECK(!e->mx4 || e->fp8, "dh_engine_create_q: MXFP4 weights (weight_dtype 1) need the block-scale pointers (attn_ws != NULL)");
    e->a6 = act_dtype == 1;
    DH_CHECK(!e->a6 || e->mx4, "dh_engine_create_qa: MXFP6 activations (act_dtype 1) need MXFP4 weights (weight_dtype 1): beside an e4m3 "
                               "weight the e2m3 activation runs the MFMA at the fp8 rate, so the pair is refused");
    e->kv8 = kv_dtype == 1;
    DH_CHECK(!e->kv8 || e->fp8, "dh_engine_create_ex: an fp8 KV cache (kv_dtype 1) needs an fp8 engine (channel scales, attn_ws != NULL)");
    e->cache_layer_elems = (size_t)max_batch * G * s_max * hs;
    e->exp_layer_elems = (size_t)max_batch * G * s_max;
    // bf16: K and V^T of every layer.  fp8: a byte per element and an exponent byte per vector of every layer, one layer of bf16
    const size_t kv_bytes = e->kv8 ? 2 * (e->cache_layer_elems + e->exp_layer_elems) * desc->n_layer + 2 * e->cache_layer_elems * sizeof(bf16_t)
                                   : 2 * e->cache_layer_elems * desc->n_layer * sizeof(bf16_t);
    const size_t bf16_layers = e->kv8 ? 1 : desc->n_layer;
    {
        // a multi-head model's KV cache (Phi-3.5: 12 KiB per position and layer) outgrows the device at batch sizes tuned on
        // TinyLlama: refuse before allocating anything, naming the knob
        size_t free_b = 0, total_b = 0;
        DH_HIP(hipMemGetInfo(&free_b, &total_b));
        DH_CHECK(kv_bytes <= free_b,
                 "dh_engine_create: the KV cache of %d sequences x %d positions x %d layers needs %.1f GiB and %.1f GiB are free: "
                 "lower the decode batch (--decode_batch)", max_batch, s_max, desc->n_layer, kv_bytes / 1073741824.0,
                 free_b / 1073741824.0);
    }
    const size_t T = max_tokens;
    int rc = 0;
    rc |= dmalloc(e, &e->kc, e->cache_layer_elems * bf16_layers);
    rc |= dmalloc(e, &e->vtc, e->cache_layer_elems * bf16_layers);
    if (e->kv8) {
        rc |= dmalloc(e, &e->k8, e->cache_layer_elems * desc->n_layer);
        rc |= dmalloc(e, &e->v8, e->cache_layer_elems * desc->n_layer);
        rc |= dmalloc(e, &e->ke, e->exp_layer_elems * desc->n_layer);
        rc |= dmalloc(e, &e->ve, e->exp_layer_elems * desc->n_layer);
    }
    rc |= dmalloc(e, &e->x, T * d);
    rc |= dmalloc(e, &e->xn, T * d);
    rc |= dmalloc(e, &e->qkv, T * e->qkv_dim);
    rc |= dmalloc(e, &e->qrot, T * d);
    rc |= dmalloc(e, &e->att, T * d);
    rc |= dmalloc(e, &e->xa, T * 48);
    rc |= dmalloc(e, &e->act, T * desc->intermediate);
    rc |= dmalloc(e, &e->xlast, (size_t)max_batch * d);
    rc |= dmalloc(e, &e->tok_slot, T);
    rc |= dmalloc(e, &e->tok_pos, T);
    rc |= dmalloc(e, &e->seq_meta, (size_t)4 * max_batch);
    rc |= dmalloc(e, &e->last_row, (size_t)max_batch);
    rc |= dmalloc(e, &e->last_meta, (size_t)2 * max_batch);
    rc |= dmalloc(e, &e->att_last, (size_t)max_batch * d);
    rc |= dmalloc(e, &e->xn_last, (size_t)max_batch * d);
    rc |= dmalloc(e, &e->act_last, (size_t)max_batch * desc->intermediate);
    rc |= dmalloc(e, &e->step_dev, 1);
    rc |= dmalloc(e, &e->slot_list, (size_t)max_batch);
    rc |= dmalloc(e, &e->copy_dst, (size_t)max_batch);
    rc |= dmalloc(e, &e->cache_tab, (size_t)(e->kv8 ? 4 : 2) * desc->n_layer);
    rc |= alloc_row_ws(e, max_batch);
    if (e->fp8) {
        rc |= dmalloc(e, &e->xq, T * (size_t)(desc->intermediate > d ? desc->intermediate : d));
        rc |= dmalloc(e, &e->xscale, T);
    }
    // whole groups of 16 rows: 3/4 byte per element and one scale byte per 32
    const size_t a6_elems = e->a6 ? (T + 15) / 16 * 16 * (size_t)(desc->intermediate > d ? desc->intermediate : d) : 0;
    if (e->a6) {
        rc |= dmalloc(e, &e->xq6, a6_elems / 4 * 3);
        rc |= dmalloc(e, &e->xs6, a6_elems / 32);
    }
    rc |= dmalloc(e, &e->row_tail, T);
    rc |= dmalloc(e, &e->last_tail, (size_t)max_batch);
    const int64_t wb = dh_attn_decode_work_bytes(max_batch, H, hs, s_max);
    if (!rc) { hipError_t he = hipMalloc(&e->dec_work, wb); if (he != hipSuccess) rc = 2; e->dev_bytes += wb; }
    if (rc) { dh_set_error("dh_engine_create: device allocation failed (%s)", dh_last_error()); return 2; }
    // the attention kernels rely on finite (zero) cache contents beyond the written positions
    DH_HIP(hipMemset(e->kc, 0, e->cache_layer_elems * bf16_layers * sizeof(bf16_t)));
    DH_HIP(hipMemset(e->vtc, 0, e->cache_layer_elems * bf16_layers * sizeof(bf16_t)));
    if (e->kv8) {   // zero bytes are 0.0 and zero exponents 2^0
        DH_HIP(hipMemset(e->k8, 0, e->cache_layer_elems * desc->n_layer));
        DH_HIP(hipMemset(e->v8, 0, e->cache_layer_elems * desc->n_layer));
        DH_HIP(hipMemset(e->ke, 0, e->exp_layer_elems * desc->n_layer));
        DH_HIP(hipMemset(e->ve, 0, e->exp_layer_elems * desc->n_layer));
    }
    if (e->a6) {   // the rows past a call's last one in its last group of 16 are read (never into a stored output) and never written
        DH_HIP(hipMemset(e->xq6, 0, a6_elems / 4 * 3));
        DH_HIP(hipMemset(e->xs6, 0, a6_elems / 32));
    }
    DH_HIP(hipMemset(e->step_dev, 0, sizeof(int32_t)));
    {
        const size_t L = desc->n_layer;
        std::vector<bf16_t*> tab((e->kv8 ? 4 : 2) * L);
        for (size_t l = 0; l < L; ++l) {
            if (e->kv8) {   // the copy kernel moves 16-byte units: the element type of the table is nominal
                tab[2 * l] = reinterpret_cast<bf16_t*>(e->k8 + l * e->cache_layer_elems);
                tab[2 * l + 1] = reinterpret_cast<bf16_t*>(e->v8 + l * e->cache_layer_elems);
                tab[2 * L + 2 * l] = reinterpret_cast<bf16_t*>(e->ke + l * e->exp_layer_elems);
                tab[2 * L + 2 * l + 1] = reinterpret_cast<bf16_t*>(e->ve + l * e->exp_layer_elems);
                continue;
            }
            tab[2 * l] = e->kc + l * e->cache_layer_elems;
            tab[2 * l + 1] = e->vtc + l * e->cache_layer_elems;
        }
        DH_HIP(hipMemcpy(e->cache_tab, tab.data(), tab.size() * sizeof(bf16_t*), hipMemcpyHostToDevice));
    }
    DH_HIP(hipHostMalloc((void**)&e->h_stage, stage_layout(T, max_batch).total * sizeof(int32_t)));
    DH_HIP(hipStreamCreateWithFlags(&e->gstream, hipStreamNonBlocking));
    DH_HIP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
    DH_HIP(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
    DH_HIP(hipEventCreateWithFlags(&e->ev_stage, hipEventDisableTiming));
    hipLaunchKernelGGL(iota_i32_kernel, dim3(cdiv(max_batch, 64)), dim3(64), 0, 0, e->seq_meta, max_batch);
    DH_HIP(hipDeviceSynchronize());
    return 0;
}

// h_slots == nullptr: sequence i lives in slot slot_base + i (the identity array written at engine creation);
// else in h_slots[i] (distinct, checked by the caller), uploaded to a device array of this call's own.
// A call of one token per sequence is a decode step and takes the decode kernels — unless prompt_phase says that these
// are prompts: then the kernels are the prefill's, as they are for a one-token prompt packed with longer ones.
int forward_impl(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len, const int32_t* h_pos0, const int32_t* h_slots,
                 int n_seq, int slot_base, bool prompt_phase, dh_bf16* logits_all, dh_bf16* logits_last, void* stream) {
    e->seq_slot = h_slots ? e->slot_list : e->seq_meta + slot_base;
    hipStream_t s = (hipStream_t)stream;
    int n_tok = 0, max_q = 0;
    for (int i = 0; i < n_seq; ++i) {
        DH_CHECK(h_seq_len[i] > 0 && h_pos0[i] >= 0, "dh_engine_forward: sequence %d has length %d at position %d", i, h_seq_len[i], h_pos0[i]);
        DH_CHECK(h_pos0[i] + h_seq_len[i] <= e->s_max, "Cannot forward sequence %d: %d tokens at position %d exceed the KV cache length %d",
                 i, h_seq_len[i], h_pos0[i], e->s_max);
        n_tok += h_seq_len[i];
        max_q = h_seq_len[i] > max_q ? h_seq_len[i] : max_q;
    }
    const bool step = max_q == 1 && !prompt_phase;    // one token per sequence == a decode step
    DH_CHECK(n_tok <= e->max_tokens, "dh_engine_forward: %d tokens exceed the workspace capacity %d", n_tok, e->max_tokens);
    const int B = e->max_batch;
    const Stage h = stage(e);
    const SeqMeta m = seq_meta(e);
    DH_HIP(hipEventSynchronize(e->ev_stage));   // this engine's previous metadata upload must have left the pinned buffer
    int t = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int slot = h_slots ? h_slots[i] : slot_base + i;
        h.seq_slot[i] = slot;
        h.q_start[i] = t;
        h.q_len[i] = h_seq_len[i];
        h.kv[i] = step ? h_pos0[i] + 1 : h_pos0[i];   // single-token call: kv_len
        for (int j = 0; j < h_seq_len[i]; ++j, ++t) { h.tok_slot[t] = slot; h.tok_pos[t] = h_pos0[i] + j; }
        h.last_row[i] = t - 1;
    }
    // Q11: rows torch's CPU bf16 rsqrt would process in its scalar tail loop
    if (e->rsqrt_vec > 0) {
        const int V = e->rsqrt_vec;
        int r = 0;
        for (int i = 0; i < n_seq; ++i) {
            for (int j = 0; j < h_seq_len[i]; ++j, ++r)
                h.row_tail[r] = e->rsqrt_whole ? (r >= n_tok / V * V) : (j >= h_seq_len[i] / V * V);
            h.last_tail[i] = h.row_tail[r - 1];   // ln_f runs on all rows in the reference: the last row keeps its flag
        }
        DH_HIP(hipMemcpyAsync(e->row_tail, h.row_tail, n_tok, hipMemcpyHostToDevice, s));
        DH_HIP(hipMemcpyAsync(e->last_tail, h.last_tail, n_seq, hipMemcpyHostToDevice, s));
    }
    DH_HIP(hipMemcpyAsync(e->tok_slot, h.tok_slot, n_tok * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DH_HIP(hipMemcpyAsync(e->tok_pos, h.tok_pos, n_tok * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // seq_meta[0..B) (slot of sequence i = i) is written once at engine creation and left alone
    if (h_slots) DH_HIP(hipMemcpyAsync(e->slot_list, h.seq_slot, n_seq * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DH_HIP(hipMemcpyAsync(m.q_start, h.q_start, 3 * B * sizeof(int32_t), hipMemcpyHostToDevice, s));   // q_start | q_len | kv
    DH_HIP(hipMemcpyAsync(e->last_row, h.last_row, B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // last-position logits of a multi-token forward only: the last block runs on the sequences' last rows (g_prune_last_layer)
    const bool prune_last = g_prune_last_layer && max_q > 1 && logits_all == nullptr && logits_last != nullptr;
    if (prune_last) {
        for (int i = 0; i < n_seq; ++i) { h.last_meta[i] = 1; h.last_meta[B + i] = h_pos0[i] + h_seq_len[i] - 1; }
        DH_HIP(hipMemcpyAsync(e->last_meta, h.last_meta, 2 * B * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    DH_HIP(hipEventRecord(e->ev_stage, s));
    // one token per sequence == a decode step (what generate()'s loop issues): same kernels as dh_engine_decode
    return run_model(e, ids, n_tok, n_seq, max_q, step, e->row_tail, e->last_tail, prune_last, logits_all, logits_last, s);
}

// One decode step of the rows `k` names: ids / tok_slot / tok_pos / kv_len from a prep kernel, the model over the k.n_seq rows (the
// kernel family is the row count's) with logits in e->logits, one sampled token per live sequence.  k.row_seq == nullptr
// (dh_engine_decode): row r is sequence r in slot r, the draw is keyed by the step counter in step_dev, which the prep kernel
// increments.  Else (dh_engine_decode_rows) the prep and the sampling kernel index the per-sequence arrays through the row list.
// One verify step of k.spec drafts per sequence (dh_engine_decode_spec): the prep kernel proposes and lays out the k.n_seq * S rows,
// the streaming single-token family runs over them with the verify attention, the head gives every row's logits, the acceptance
// kernel appends what the drafts got right plus one — against the arg-max, or, k.spec_draw, against the draw of the plain sampled step.
int verify_step(dh_engine* e, const dh_engine::GKey& k, hipStream_t s) {
    const int S = k.spec + 1, rows = k.n_seq * S;
    const dh_model_desc& D = e->d;
    int cap = e->s_max < k.tok_ld ? e->s_max : k.tok_ld;
    cap = cap < D.block_size ? cap : D.block_size;
    hipLaunchKernelGGL(spec_prep_kernel, dim3(k.n_seq), dim3(256), 0, s, k.tokens, k.tok_ld, k.length, k.limit, k.max_new, k.drafts, S, 3,
                       e->dec_ids, e->tok_slot, e->tok_pos, seq_meta(e).kv, e->step_dev, cap, D.wte_rows);
    DH_LAUNCH_CHECK();
    e->decode_tiled = false;
    int rc;
    if ((rc = run_layers_decode(e, e->dec_ids, rows, nullptr, s, S))) return rc;
    if ((rc = head(e, nullptr, rows, e->logits, nullptr, s))) return rc;
    const dh_spec_draw draw{k.top_k, k.seed, k.max_new};
    return dh_spec_accept_impl(e->logits, D.vocab, e->dec_ids, S, k.tokens, k.tok_ld, k.length, k.done, k.limit, k.n_seq, k.temp, k.eos,
                               e->step_dev, k.counters, k.ctl, s, k.spec_draw ? &draw : nullptr);
}

// tiles that the keys of max_new generated tokens can span, wherever in a tile the prompt ends
int beam_tiles(int max_new) { return (max_new + 30) / 32 + 1; }

// One beam step (dh_engine_decode_beam): prep, the single-token step over the n_utt * W rows, the selection, the re-parenting.
int beam_step(dh_engine* e, const dh_engine::GKey& k, hipStream_t s) {
    const dh_model_desc& D = e->d;
    const int rows = k.n_seq, W = k.beam_w;
    const int cap = e->s_max < D.block_size ? e->s_max : D.block_size;
    hipLaunchKernelGGL(beam_prep_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, s, k.beam.beam_tok, k.length, k.limit, W, k.max_new, e->dec_ids,
                       e->tok_slot, e->tok_pos, seq_meta(e).kv, e->step_dev, rows, cap, D.wte_rows);
    DH_LAUNCH_CHECK();
    int rc;
    if ((rc = run_model(e, e->dec_ids, rows, rows, 1, true, e->ones, e->ones, false, e->logits, nullptr, s))) return rc;
    if ((rc = dh_beam_select_impl(e->logits, D.vocab, rows / W, W, W, k.max_new, k.eos, 0, e->step_dev, k.beam, e->beam_cand_ids,
                                  e->beam_cand_lp, k.ctl.mask, k.ctl.mask_ld, k.ctl.stop, k.stop_fin_tok, s, k.beam_hist, k.beam_ngram))) return rc;
    if (W == 1) return 0;                                   // a single beam continues itself
    if (k.beam_tab)                                         // "Beam KV tile table": the table rows and the one open tile
        return dh_beam_retile_impl(e->cache_tab, nullptr, nullptr, 2 * D.n_layer, e->beam_tile_scratch, k.beam_tab, k.beam_tab_nt,
                                   k.beam.beam_parent, k.length, k.limit, e->step_dev, 0, rows, W, k.max_new, D.n_groups, D.head_size,
                                   e->s_max, s);
    const int tile_units = D.head_size * 4, nt_max = std::min(beam_tiles(k.max_new), e->s_max / 32);
    const dim3 grid(cdiv(nt_max * tile_units, 256), 2 * D.n_layer * D.n_groups, rows);
    for (int to_scratch = 1; to_scratch >= 0; --to_scratch) {
        hipLaunchKernelGGL(beam_reparent_kernel, grid, dim3(256), 0, s, e->cache_tab, e->beam_scratch, k.beam.beam_parent, k.length, k.limit,
                           e->step_dev, W, k.max_new, D.n_groups, (size_t)e->s_max * D.head_size, tile_units, nt_max, e->s_max / 32,
                           to_scratch);
        DH_LAUNCH_CHECK();
    }
    return 0;
}

// The options of a step an entry point is about to launch: what the setters have set, less what the step's kind does not take.  This is
// what the step's sampling launch bakes in, so it is what the step's key compares.
enum StepKind { STEP_DECODE, STEP_DECODE_ROWS, STEP_VERIFY, STEP_BEAM };
dh_pick_ctl step_ctl(const dh_engine* e, StepKind kind, int top_k, bool draw = false) {
    dh_pick_ctl c;
    c.mask = e->set.mask;
    c.mask_ld = e->set.mask_ld;
    c.stop = e->set.stop;
    if (kind == STEP_BEAM) return c;                    // the selection takes the mask and the stop specification, nothing else
    c = e->set;
    const bool argmax_verify = kind == STEP_VERIFY && !draw;            // draw: dh_engine_decode_spec_draw's step keeps what a plain step keeps
    if (argmax_verify) {                                // dh_engine_decode_spec has refused all three
        c.pen = DH_PENALTY_OFF;
        c.bias = dh_bias_args{};
        c.aut = dh_automaton_args{};
    }
    if (argmax_verify || top_k == 1) c.nuc = dh_nucleus_args{};   // the arg-max takes neither parameter: its step is the plain one
    // the prompt lengths of the step's history readers and stop sequences: the setters were given the same numbers
    c.start = c.ngram ? e->ngram_start : dh_penalty_on(c.pen) ? e->pen_start : c.bias.n ? e->bias_start : c.aut.on() ? e->aut_start : e->stop_start;
    return c;
}

// dh_engine_decode and dh_engine_decode_rows (`name`): the penalties' LDS tables, which a bias shares, hold a call's token buffer
int check_pen_tables(const dh_engine* e, const char* name, int tok_ld) {
    const dh_pick_ctl& c = e->set;
    DH_CHECK(!dh_penalty_on(c.pen) || tok_ld <= DH_MAX_PENALTY_HISTORY, "%s: penalties are set and keep a sequence's distinct ids in static "
             "LDS tables of %d entries; tok_ld=%d may not fit", name, DH_MAX_PENALTY_HISTORY, tok_ld);
    DH_CHECK(!dh_penalty_on(c.pen) || c.bias.n == 0 || tok_ld + c.bias.n_ids <= DH_MAX_PENALTY_HISTORY, "%s: penalties and a bias are "
             "set and share static LDS tables of %d entries; tok_ld=%d and the entries' %d ids may not fit", name, DH_MAX_PENALTY_HISTORY,
             tok_ld, c.bias.n_ids);
    return 0;
}

// the same two entries: what an automaton set needs of the call, refused here, before a step is captured or launched
int check_automaton_call(const dh_engine* e, const char* name, int64_t eos_id, int n_seq) {
    const dh_automaton_args& a = e->set.aut;
    DH_CHECK(!a.on() || (eos_id >= 0 && eos_id < e->d.vocab), "%s: an automaton set is set and needs an eos_id in [0, %d), got %lld: a dead "
             "end ends the sequence with it", name, e->d.vocab, (long long)eos_id);
    DH_CHECK(!a.on() || a.n_seq == n_seq, "%s: the automaton set holds start states for %d sequences, the call has %d", name, a.n_seq, n_seq);
    return 0;
}

// What shared-prompt attention needs of the engine (`name`: the setter) and of a call that runs under it (`name`: dh_engine_decode or
// dh_engine_decode_beam, n_seq its rows): the streaming single-token layers over whole utterances.  group_rows == 0: nothing to check.
int check_shared_call(const dh_engine* e, const char* name, int n_seq, int group_rows) {
    if (group_rows == 0) return 0;
    DH_CHECK(!e->fp8, "%s: shared-prompt attention (group_rows=%d) on an fp8 or MXFP4 engine: its step does not run the streaming "
             "layers that launch the kernel; not supported", name, group_rows);
    DH_CHECK(!e->kv8, "%s: shared-prompt attention (group_rows=%d) reads bf16 cache tiles; an fp8 KV cache is not supported", name, group_rows);
    DH_CHECK(e->rsqrt_vec == 0, "%s: shared-prompt attention (group_rows=%d) with the CPU rsqrt emulation, which flags rows by their "
             "place in a call; not supported", name, group_rows);
    DH_CHECK(g_decode_tiled_rows == 0, "%s: shared-prompt attention (group_rows=%d) with dh_set_tuning key 10, which moves steps to the "
             "tiled kernels by row count; not supported", name, group_rows);
    DH_CHECK(n_seq % group_rows == 0, "%s: shared-prompt attention is set for group_rows=%d rows per utterance; %d rows are no multiple",
             name, group_rows, n_seq);
    DH_CHECK(n_seq <= MAX_DECODE_ROWS, "%s: shared-prompt attention (group_rows=%d): %d rows exceed the streaming step's %d", name,
             group_rows, n_seq, MAX_DECODE_ROWS);
    return 0;
}

int plain_step(dh_engine* e, const dh_engine::GKey& k, hipStream_t s);
int decode_step(dh_engine* e, const dh_engine::GKey& k, hipStream_t s) {
    if (k.spec) return verify_step(e, k, s);
    e->step_shared_rows = k.shared_rows;                // what run_layers_decode launches for this step's attention
    e->step_shared_plen = k.shared_plen;
    e->step_beam_tab = k.beam_tab;
    e->step_beam_tab_nt = k.beam_tab_nt;
    const int rc = k.beam_w ? beam_step(e, k, s) : plain_step(e, k, s);
    e->step_shared_rows = 0;
    e->step_shared_plen = nullptr;
    e->step_beam_tab = nullptr;
    e->step_beam_tab_nt = 0;
    return rc;
}

int plain_step(dh_engine* e, const dh_engine::GKey& k, hipStream_t s) {
    const bool rows = k.row_seq != nullptr;
    hipLaunchKernelGGL(decode_prep_kernel, dim3(cdiv(k.n_seq, 64)), dim3(64), 0, s, k.tokens, k.tok_ld, k.length, k.row_seq, k.row_slot,
                       e->dec_ids, e->tok_slot, e->tok_pos, seq_meta(e).kv, rows ? nullptr : e->step_dev, k.n_seq, k.n_all,
                       e->max_batch, e->s_max);
    DH_LAUNCH_CHECK();
    int rc;
    if ((rc = run_model(e, e->dec_ids, k.n_seq, k.n_seq, 1, true, e->ones, e->ones, false, e->logits, nullptr, s))) return rc;
    if (rows)
        return dh_sample_rows_impl(e->logits, e->d.vocab, k.tokens, k.tok_ld, k.length, k.done, k.limit, k.row_seq, k.n_seq, k.n_all,
                                   k.max_new, k.temp, k.top_k, k.eos, k.seed, k.ctl, s);
    return dh_sample_impl(e->logits, e->d.vocab, k.tokens, k.tok_ld, k.length, k.done, k.n_seq, k.temp, k.top_k, k.eos, k.seed, 0,
                          e->step_dev, k.ctl, s);
}

// n_steps launches of the step `key` describes, captured into a hipGraph at its first use (8 graphs are kept)
int launch_steps(dh_engine* e, const dh_engine::GKey& key, int n_steps, hipStream_t s) {
    hipGraphExec_t gexec = nullptr;
    for (auto& g : e->graphs) {
        if (g.key == key) {
            gexec = g.exec;
            g.used = ++e->graph_clock;
            break;
        }
    }
    // hand over from the caller's stream to the engine's capture-capable stream
    DH_HIP(hipEventRecord(e->ev_in, s));
    DH_HIP(hipStreamWaitEvent(e->gstream, e->ev_in, 0));
    if (!gexec) {
        hipGraph_t graph = nullptr;
        DH_HIP(hipStreamBeginCapture(e->gstream, hipStreamCaptureModeThreadLocal));
        e->capturing = true;
        int rc = decode_step(e, key, e->gstream);
        e->capturing = false;
        hipError_t ce = hipStreamEndCapture(e->gstream, &graph);
        if (rc) { if (graph) hipGraphDestroy(graph); return rc; }
        DH_CHECK(ce == hipSuccess && graph, "dh_engine_decode: graph capture failed: %s", hipGetErrorString(ce));
        hipError_t ie = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        DH_CHECK(ie == hipSuccess, "dh_engine_decode: hipGraphInstantiate failed: %s", hipGetErrorString(ie));
        if (e->graphs.size() >= 8) {   // evict the least recently used (its launches are stream-ordered before the destroy)
            size_t lru = 0;
            for (size_t i = 1; i < e->graphs.size(); ++i)
                if (e->graphs[i].used < e->graphs[lru].used) lru = i;
            DH_HIP(hipStreamSynchronize(e->gstream));
            hipGraphExecDestroy(e->graphs[lru].exec);
            e->graphs.erase(e->graphs.begin() + lru);
        }
        e->graphs.push_back({key, gexec, ++e->graph_clock});
    }
    for (int i = 0; i < n_steps; ++i) DH_HIP(hipGraphLaunch(gexec, e->gstream));
    DH_HIP(hipEventRecord(e->ev_out, e->gstream));
    DH_HIP(hipStreamWaitEvent(s, e->ev_out, 0));
    return 0;
}

}  // namespace

extern "C" int dh_engine_create(const dh_model_desc* desc, int max_batch, int s_max, int max_tokens, dh_engine** out) {
    return dh_engine_create_ex(desc, max_batch, s_max, max_tokens, 0, out);
}

extern "C" int dh_engine_create_ex(const dh_model_desc* desc, int max_batch, int s_max, int max_tokens, int kv_dtype, dh_engine** out) {
    return dh_engine_create_q(desc, max_batch, s_max, max_tokens, kv_dtype, 0, out);
}

extern "C" int dh_engine_create_q(const dh_model_desc* desc, int max_batch, int s_max, int max_tokens, int kv_dtype, int weight_dtype,
                                  dh_engine** out) {
    return dh_engine_create_qa(desc, max_batch, s_max, max_tokens, kv_dtype, weight_dtype, 0, out);
}

extern "C" int dh_engine_create_qa(const dh_model_desc* desc, int max_batch, int s_max, int max_tokens, int kv_dtype, int weight_dtype,
                                   int act_dtype, dh_engine** out) {
    DH_CHECK(desc && out, "dh_engine_create: null argument");
    DH_CHECK(act_dtype == 0 || act_dtype == 1, "dh_engine_create_qa: act_dtype %d is neither 0 (e4m3 per token) nor 1 (MXFP6)", act_dtype);
    DH_CHECK(weight_dtype == 0 || weight_dtype == 1, "dh_engine_create_q: weight_dtype %d is neither 0 (as described) nor 1 (MXFP4)", weight_dtype);
    DH_CHECK(kv_dtype == 0 || kv_dtype == 1, "dh_engine_create_ex: kv_dtype %d is neither 0 (bf16) nor 1 (fp8)", kv_dtype);
    DH_CHECK(desc->head_size == 64 || desc->head_size == 96 || desc->head_size == 128, "dh_engine_create: head_size %d unsupported", desc->head_size);
    DH_CHECK(desc->n_head % desc->n_groups == 0, "dh_engine_create: n_head %% n_groups != 0");
    DH_CHECK(desc->n_embd == desc->n_head * desc->head_size, "dh_engine_create: n_embd != n_head*head_size");
    DH_CHECK(desc->n_embd % 64 == 0 && desc->intermediate % 64 == 0 && desc->vocab % 8 == 0, "dh_engine_create: dims must be multiples of 64");
    DH_CHECK(s_max > 0 && s_max % 64 == 0 && s_max <= (desc->block_size + 63) / 64 * 64, "dh_engine_create: s_max=%d must be a multiple of 64 and <= block_size rounded up", s_max);
    DH_CHECK(max_batch > 0 && max_tokens >= max_batch, "dh_engine_create: bad batch/token capacity");
    DH_CHECK(desc->rope_cos && desc->rope_sin && desc->wte && desc->ln_f && desc->lm_head && desc->h_layers, "dh_engine_create: null weight pointer");
    dh_engine* e = new dh_engine();
    const int rc = engine_init(e, desc, max_batch, s_max, max_tokens, kv_dtype, weight_dtype, act_dtype);
    if (rc) { dh_engine_destroy(e); return rc; }   // one cleanup path: nothing allocated so far leaks
    {
        std::lock_guard<std::mutex> lock(g_engines_mu);
        g_engines.push_back(e);
    }
    *out = e;
    return 0;
}

extern "C" void dh_engine_destroy(dh_engine* e) {
    if (!e) return;
    {
        std::lock_guard<std::mutex> lock(g_engines_mu);
        g_engines.erase(std::remove(g_engines.begin(), g_engines.end(), e), g_engines.end());
    }
    for (auto& g : e->graphs) hipGraphExecDestroy(g.exec);
    void* ptrs[] = {e->kc, e->vtc, e->k8, e->v8, e->ke, e->ve, e->x, e->xn, e->qkv, e->qrot, e->att, e->xa, e->act, e->xlast, e->logits,
                    e->tok_slot, e->tok_pos, e->seq_meta, e->last_row, e->last_meta, e->att_last, e->xn_last, e->act_last, e->step_dev, e->slot_list, e->copy_dst, e->cache_tab, e->dec_ids, e->dec_work,
                    e->beam_scratch, e->beam_tile_scratch, e->beam_cand_ids, e->beam_cand_lp,
                    e->row_tail, e->last_tail, e->ones, e->part32, e->xq, e->xscale, e->xq6, e->xs6};
    for (void* p : ptrs)
        if (p) hipFree(p);
    if (e->h_stage) hipHostFree(e->h_stage);
    if (e->gstream) hipStreamDestroy(e->gstream);
    if (e->ev_in) hipEventDestroy(e->ev_in);
    if (e->ev_out) hipEventDestroy(e->ev_out);
    if (e->ev_stage) hipEventDestroy(e->ev_stage);
    for (auto& v : e->tm.ev)
        for (auto& p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    delete e;
}

extern "C" int64_t dh_engine_device_bytes(const dh_engine* e) { return e ? e->dev_bytes : 0; }
extern "C" int dh_engine_read(dh_engine* e, int what, int layer, void* dst, int64_t n_bytes, void* stream) {
    DH_CHECK(e && dst && n_bytes >= 0, "dh_engine_read: bad argument");
    const void* src = nullptr;
    int64_t avail = 0;
    const int64_t cache_bytes = (int64_t)e->cache_layer_elems * sizeof(bf16_t);
    switch (what) {
        case 0: src = e->xn; avail = (int64_t)e->max_tokens * e->d.n_embd * 2; break;
        case 3: src = e->x; avail = (int64_t)e->max_tokens * e->d.n_embd * 2; break;
        case 6: case 7:
            DH_CHECK(e->kv8, "dh_engine_read: selector %d reads an fp8 KV cache; this engine's is bf16 (selectors 1 / 2)", what);
            DH_CHECK(layer >= 0 && layer < e->d.n_layer, "dh_engine_read: layer %d out of range", layer);
            {   // every slot (seq_meta row 0 is the identity), every position
                const int rc = dh_kv8_expand(e->k8 + (size_t)layer * e->cache_layer_elems, e->v8 + (size_t)layer * e->cache_layer_elems,
                                             e->ke + (size_t)layer * e->exp_layer_elems, e->ve + (size_t)layer * e->exp_layer_elems,
                                             e->seq_meta, nullptr, nullptr, e->kc, e->vtc, e->max_batch, e->d.n_groups, e->d.head_size,
                                             e->s_max, stream);
                if (rc) return rc;
            }
            src = what == 6 ? e->kc : e->vtc;
            avail = cache_bytes;
            break;
        case 1: case 2:
            DH_CHECK(!e->kv8, "dh_engine_read: selector %d reads a bf16 KV cache; this engine's is fp8 (selectors 6 / 7)", what);
            DH_CHECK(layer >= 0 && layer < e->d.n_layer, "dh_engine_read: layer %d out of range", layer);
            src = (what == 1 ? e->kc : e->vtc) + (size_t)layer * e->cache_layer_elems;
            avail = cache_bytes;
            break;
        case 9: case 10: case 11: case 12:
            DH_CHECK(e->kv8, "dh_engine_read: selector %d reads an fp8 KV cache's bytes or exponents; this engine's is bf16", what);
            DH_CHECK(layer >= 0 && layer < e->d.n_layer, "dh_engine_read: layer %d out of range", layer);
            if (what <= 10) { src = (what == 9 ? e->k8 : e->v8) + (size_t)layer * e->cache_layer_elems; avail = (int64_t)e->cache_layer_elems; }
            else { src = (what == 11 ? e->ke : e->ve) + (size_t)layer * e->exp_layer_elems; avail = (int64_t)e->exp_layer_elems; }
            break;
        case 4: src = e->dec_ids; avail = (int64_t)e->row_cap * sizeof(int64_t); break;
        case 5: src = seq_meta(e).kv; avail = (int64_t)e->max_batch * sizeof(int32_t); break;
        case 8: src = e->logits; avail = (int64_t)e->row_cap * e->d.vocab * 2; break;       // the last single-token step's rows
        default: DH_CHECK(false, "dh_engine_read: unknown selector %d", what);
    }
    DH_CHECK(n_bytes <= avail, "dh_engine_read: %lld bytes requested, %lld available", (long long)n_bytes, (long long)avail);
    DH_HIP(hipMemcpyAsync(dst, src, n_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int dh_engine_forward(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len, const int32_t* h_pos0,
                                 int n_seq, dh_bf16* logits_all, dh_bf16* logits_last, void* stream) {
    return dh_engine_forward_at(e, ids, h_seq_len, h_pos0, n_seq, 0, logits_all, logits_last, stream);
}

extern "C" int dh_engine_forward_at(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len, const int32_t* h_pos0,
                                    int n_seq, int slot_base, dh_bf16* logits_all, dh_bf16* logits_last, void* stream) {
    DH_CHECK(e && ids && h_seq_len && h_pos0, "dh_engine_forward: null argument");
    DH_CHECK(n_seq > 0 && slot_base >= 0 && slot_base + n_seq <= e->max_batch,
             "dh_engine_forward: sequences [%d, %d) exceed max_batch=%d", slot_base, slot_base + n_seq, e->max_batch);
    return forward_impl(e, ids, h_seq_len, h_pos0, nullptr, n_seq, slot_base, false, logits_all, logits_last, stream);
}

extern "C" int dh_engine_forward_slots(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len, const int32_t* h_pos0,
                                       const int32_t* h_slot, int n_seq, int prompt_phase, dh_bf16* logits_all, dh_bf16* logits_last,
                                       void* stream) {
    DH_CHECK(e && ids && h_seq_len && h_pos0 && h_slot, "dh_engine_forward_slots: null argument");
    DH_CHECK(n_seq > 0 && n_seq <= e->max_batch, "dh_engine_forward_slots: n_seq=%d exceeds max_batch=%d", n_seq, e->max_batch);
    std::vector<char> taken(e->max_batch, 0);
    for (int i = 0; i < n_seq; ++i) {
        DH_CHECK(h_slot[i] >= 0 && h_slot[i] < e->max_batch, "dh_engine_forward_slots: sequence %d names slot %d of %d", i, h_slot[i], e->max_batch);
        DH_CHECK(!taken[h_slot[i]], "dh_engine_forward_slots: slot %d is named twice", h_slot[i]);
        taken[h_slot[i]] = 1;
    }
    return forward_impl(e, ids, h_seq_len, h_pos0, h_slot, n_seq, 0, prompt_phase != 0, logits_all, logits_last, stream);
}

extern "C" int dh_engine_copy_prefix(dh_engine* e, int src_slot, const int32_t* h_dst_slots, int n_dst, int n_pos, void* stream) {
    DH_CHECK(e, "dh_engine_copy_prefix: null engine");
    DH_CHECK(engine_is_live(e), "dh_engine_copy_prefix: %p is not an engine of dh_engine_create (or was destroyed)", (void*)e);
    DH_CHECK(n_pos > 0 && n_pos % 32 == 0 && n_pos <= e->s_max,
             "dh_engine_copy_prefix: n_pos=%d must be a positive multiple of 32 (the cache tile) and <= s_max=%d", n_pos, e->s_max);
    DH_CHECK(src_slot >= 0 && src_slot < e->max_batch, "dh_engine_copy_prefix: source slot %d of %d", src_slot, e->max_batch);
    DH_CHECK(n_dst >= 0 && n_dst < e->max_batch && (h_dst_slots || n_dst == 0),
             "dh_engine_copy_prefix: %d destinations (null list: %d) in an engine of %d slots", n_dst, h_dst_slots == nullptr, e->max_batch);
    std::vector<char> taken(e->max_batch, 0);
    for (int i = 0; i < n_dst; ++i) {
        const int d = h_dst_slots[i];
        DH_CHECK(d >= 0 && d < e->max_batch, "dh_engine_copy_prefix: destination %d names slot %d of %d", i, d, e->max_batch);
        DH_CHECK(d != src_slot, "dh_engine_copy_prefix: the source slot %d is in the destination list", src_slot);
        DH_CHECK(!taken[d], "dh_engine_copy_prefix: slot %d is named twice", d);
        taken[d] = 1;
    }
    if (n_dst == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const Stage h = stage(e);
    DH_HIP(hipEventSynchronize(e->ev_stage));   // the previous metadata upload must have left the pinned buffer
    for (int i = 0; i < n_dst; ++i) h.seq_slot[i] = h_dst_slots[i];
    DH_HIP(hipMemcpyAsync(e->copy_dst, h.seq_slot, n_dst * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DH_HIP(hipEventRecord(e->ev_stage, s));
    const int hs = e->d.head_size, G = e->d.n_groups;
    // one launch per kind of block: `block_elems` 2-byte elements per (slot, group), the first run16 16-byte units of each copied
    auto copy = [&](bf16_t* const* tab, size_t block_elems, int run16) {
        const dim3 grid(cdiv(run16, 256), 2 * e->d.n_layer * G, 1);
        // a short prefix in a shallow model makes few pieces: split the destination list until some 2048 blocks are in flight
        const int shares = std::min<int64_t>(n_dst, std::max<int64_t>(1, 2048 / ((int64_t)grid.x * grid.y)));
        const int dst_per_block = cdiv(n_dst, shares);
        hipLaunchKernelGGL(kv_copy_prefix_kernel, dim3(grid.x, grid.y, cdiv(n_dst, dst_per_block)), dim3(256), 0, s, tab, e->copy_dst,
                           n_dst, dst_per_block, src_slot, G, block_elems, run16);
    };
    if (e->kv8) {   // bytes: n_pos / 32 tiles of hs * 32 bytes; exponents: n_pos bytes (n_pos and s_max are multiples of 32)
        copy(e->cache_tab, (size_t)e->s_max * hs / 2, n_pos * hs / 16);
        copy(e->cache_tab + 2 * e->d.n_layer, (size_t)e->s_max / 2, n_pos / 16);
    } else {
        copy(e->cache_tab, (size_t)e->s_max * hs, n_pos * hs / 8);   // n_pos / 32 tiles of hs * 32 elements
    }
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_engine_fork_slots(dh_engine* e, const int32_t* d_prompt_len, int n_utt, int n_copies, int max_len, void* stream) {
    DH_CHECK(n_copies >= 2 && n_copies <= DH_MAX_SAMPLES,
             "dh_engine_fork_slots: n_copies=%d: an utterance is forked into 2 .. %d slots, its own included", n_copies, DH_MAX_SAMPLES);
    DH_CHECK(max_len >= 1, "dh_engine_fork_slots: max_len=%d: the longest prompt has at least one token (it sizes the grid)", max_len);
    DH_CHECK(e, "dh_engine_fork_slots: null engine");
    DH_CHECK(engine_is_live(e), "dh_engine_fork_slots: %p is not an engine of dh_engine_create (or was destroyed)", (void*)e);
    DH_CHECK(d_prompt_len, "dh_engine_fork_slots: null prompt lengths (a device array of n_utt int32)");
    DH_CHECK(n_utt >= 1 && (int64_t)n_utt * n_copies <= e->max_batch,
             "dh_engine_fork_slots: %d utterances x %d slots exceed the engine's %d", n_utt, n_copies, e->max_batch);
    DH_CHECK(max_len <= e->s_max, "dh_engine_fork_slots: max_len=%d exceeds s_max=%d", max_len, e->s_max);
    hipStream_t s = (hipStream_t)stream;
    const int hs = e->d.head_size, G = e->d.n_groups, max_tiles = cdiv(max_len, 32), n_dst = n_copies - 1;
    // one launch per kind of block: `block_elems` 2-byte elements per (slot, group), tiles of tile_units 16-byte units; nothing here
    // touches the host staging buffer or waits for the stream
    auto fork = [&](bf16_t* const* tab, size_t block_elems, int tile_units) {
        const dim3 grid(cdiv(max_tiles * tile_units, 256), 2 * e->d.n_layer * G, n_utt);
        // short prompts in a shallow model make few pieces: split the destinations until some 2048 blocks are in flight
        const int shares = std::min<int64_t>(n_dst, std::max<int64_t>(1, 2048 / ((int64_t)grid.x * grid.y * grid.z)));
        const int dst_per_block = cdiv(n_dst, shares);
        const int z = cdiv(n_dst, dst_per_block);
        hipLaunchKernelGGL(kv_fork_slots_kernel, dim3(grid.x, grid.y, n_utt * z), dim3(256), 0, s, tab, d_prompt_len, n_copies, z,
                           dst_per_block, G, block_elems, tile_units, e->s_max / 32);
    };
    if (e->kv8) {   // bytes: tiles of hs * 32 bytes; exponents: 32 bytes per tile (s_max is a multiple of 64)
        fork(e->cache_tab, (size_t)e->s_max * hs / 2, hs * 2);
        fork(e->cache_tab + 2 * e->d.n_layer, (size_t)e->s_max / 2, 2);
    } else {
        fork(e->cache_tab, (size_t)e->s_max * hs, hs * 4);           // tiles of hs * 32 elements
    }
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_engine_decode(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, int n_seq,
                                int n_steps, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                int first_step, void* stream) {
    DH_CHECK(e && tokens && length && done, "dh_engine_decode: null argument");
    DH_CHECK(n_seq > 0 && n_seq <= e->max_batch, "dh_engine_decode: n_seq=%d exceeds max_batch=%d", n_seq, e->max_batch);
    DH_CHECK(temperature > 0.f && top_k >= 0, "dh_engine_decode: bad sampling parameters");
    if (int rc = check_pen_tables(e, "dh_engine_decode", tok_ld)) return rc;
    if (int rc = check_automaton_call(e, "dh_engine_decode", eos_id, n_seq)) return rc;
    if (int rc = check_shared_call(e, "dh_engine_decode", n_seq, e->shared_rows)) return rc;
    if (n_steps <= 0) return 0;
    e->seq_slot = e->seq_meta;
    hipStream_t s = (hipStream_t)stream;
    // seq_slot (seq_meta[0..B)) is the identity from engine creation on; nothing here touches the host
    // staging buffer, so the call never waits for the stream (several engines can be driven back to back)
    hipLaunchKernelGGL(set_i32_kernel, dim3(1), dim3(1), 0, s, e->step_dev, (int32_t)first_step);
    DH_LAUNCH_CHECK();
    // rsqrt_vec: `rt = rsqrt_vec > 0 ? flags : nullptr` is resolved while capturing, so it is part of the key
    dh_engine::GKey key;
    key.tokens = tokens; key.tok_ld = tok_ld; key.length = length; key.done = done;
    key.n_seq = n_seq; key.top_k = top_k; key.temp = temperature; key.eos = eos_id; key.seed = seed;
    key.rsqrt_vec = e->rsqrt_vec; key.tiled_rows = g_decode_tiled_rows;
    key.ctl = step_ctl(e, STEP_DECODE, top_k);
    key.shared_rows = e->shared_rows; key.shared_plen = e->shared_plen;
    return launch_steps(e, key, n_steps, s);
}

extern "C" int dh_engine_decode_rows(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, const int32_t* limit,
                                     int n_seq, int max_new_tokens, const int32_t* row_seq, const int32_t* row_slot, int n_rows,
                                     int n_steps, float temperature, int top_k, int64_t eos_id, uint64_t seed, void* stream) {
    DH_CHECK(e && tokens && length && done && limit && row_seq && row_slot, "dh_engine_decode_rows: null argument");
    DH_CHECK(n_rows > 0 && n_rows <= e->max_batch, "dh_engine_decode_rows: n_rows=%d exceeds max_batch=%d", n_rows, e->max_batch);
    DH_CHECK(n_seq > 0 && tok_ld > 0 && max_new_tokens > 0, "dh_engine_decode_rows: bad shape");
    DH_CHECK(temperature > 0.f && top_k >= 0, "dh_engine_decode_rows: bad sampling parameters");
    if (int rc = check_pen_tables(e, "dh_engine_decode_rows", tok_ld)) return rc;
    if (int rc = check_automaton_call(e, "dh_engine_decode_rows", eos_id, n_seq)) return rc;
    DH_CHECK(e->shared_rows == 0, "dh_engine_decode_rows: shared-prompt attention is set (group_rows=%d); a row list names any sequence "
             "in any slot, so a step's rows are not the rows of utterances", e->shared_rows);
    if (n_steps <= 0) return 0;
    e->seq_slot = row_slot;
    // the graph reads row_seq / row_slot when it runs: their contents change between calls, their addresses are part of the key
    dh_engine::GKey key;
    key.tokens = tokens; key.tok_ld = tok_ld; key.length = length; key.done = done;
    key.n_seq = n_rows; key.top_k = top_k; key.temp = temperature; key.eos = eos_id; key.seed = seed;
    key.rsqrt_vec = e->rsqrt_vec; key.tiled_rows = g_decode_tiled_rows;
    key.limit = limit; key.row_seq = row_seq; key.row_slot = row_slot; key.n_all = n_seq; key.max_new = max_new_tokens;
    key.ctl = step_ctl(e, STEP_DECODE_ROWS, top_k);
    return launch_steps(e, key, n_steps, (hipStream_t)stream);
}

extern "C" int dh_engine_reserve_rows(dh_engine* e, int rows) {
    DH_CHECK(e, "dh_engine_reserve_rows: null engine");
    DH_CHECK(rows > 0 && rows <= MAX_DECODE_ROWS && rows <= e->max_tokens,
             "dh_engine_reserve_rows: %d rows (at most %d, and the engine's max_tokens = %d)", rows, MAX_DECODE_ROWS, e->max_tokens);
    if (rows <= e->row_cap) return 0;
    // the captured steps hold the old addresses
    DH_HIP(hipDeviceSynchronize());
    for (auto& g : e->graphs) hipGraphExecDestroy(g.exec);
    e->graphs.clear();
    // on failure the engine keeps its workspaces and row_cap; its steps are captured again when they are next asked for
    if (alloc_row_ws(e, rows)) { dh_set_error("dh_engine_reserve_rows: device allocation failed (%s)", dh_last_error()); return 2; }
    return 0;
}

extern "C" int dh_engine_graph_count(const dh_engine* e, int n_draft) {
    if (!e) return -1;
    int n = 0;
    for (const auto& g : e->graphs) n += n_draft < 0 || g.key.spec == n_draft;
    return n;
}

namespace {
// dh_engine_decode_spec and dh_engine_decode_spec_draw (`name`; draw: the latter, with its top_k and seed)
int decode_spec_call(const char* name, bool draw, dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                     const int32_t* limit, int n_seq, int max_new_tokens, int n_draft, const int64_t* drafts, int32_t* counters, int n_steps,
                     float temperature, int top_k, int64_t eos_id, uint64_t seed, int first_step, void* stream) {
    DH_CHECK(e && tokens && length && done && limit && counters, "%s: null argument", name);
    DH_CHECK(n_seq > 0 && n_seq <= e->max_batch, "%s: n_seq=%d exceeds max_batch=%d", name, n_seq, e->max_batch);
    DH_CHECK(tok_ld > 0 && max_new_tokens > 0 && temperature > 0.f, "%s: bad shape or temperature", name);
    DH_CHECK(top_k >= 0, "%s: top_k must be >= 0 (0 = no crop)", name);
    DH_CHECK(n_draft >= 1 && n_draft <= 7, "%s: n_draft=%d is not in 1..7", name, n_draft);
    const int S = n_draft + 1, q_per_kv = e->d.n_head / e->d.n_groups;
    DH_CHECK(S * q_per_kv <= 32, "%s: %d positions x %d heads per KV group exceed the 32 query columns of the verify attention", name, S, q_per_kv);
    DH_CHECK(n_seq * S <= MAX_DECODE_ROWS, "%s: %d x %d rows exceed the streaming step's %d", name, n_seq, S, MAX_DECODE_ROWS);
    DH_CHECK(n_seq * S <= e->row_cap && n_seq * S <= e->max_tokens,
             "%s: %d rows, the workspaces hold %d (dh_engine_reserve_rows) of max_tokens = %d", name, n_seq * S, e->row_cap, e->max_tokens);
    if (draw) {                                         // the options a plain step takes, under the plain entries' limits
        if (int rc = check_pen_tables(e, name, tok_ld)) return rc;
        if (int rc = check_automaton_call(e, name, eos_id, n_seq)) return rc;
    } else {
        DH_CHECK(!dh_penalty_on(e->set.pen), "%s: penalties are set (repetition=%g, frequency=%g, presence=%g); a verify position's "
                 "history would have to include this launch's own picks", name, (double)e->set.pen.repetition, (double)e->set.pen.frequency,
                 (double)e->set.pen.presence);
        DH_CHECK(e->set.bias.n == 0, "%s: a bias of %d entries is set; a verify position's tail would have to include this "
                 "launch's own picks, so the step would need per-position tables", name, e->set.bias.n);
        DH_CHECK(!e->set.aut.on(), "%s: an automaton set of %d states is set; a verify position's state would depend on the "
                 "picks of this launch's earlier positions", name, e->set.aut.n_states);
    }
    DH_CHECK(e->shared_rows == 0, "%s: shared-prompt attention is set (group_rows=%d); a verify step's rows are "
             "positions of one sequence, not rows of an utterance", name, e->shared_rows);
    DH_CHECK(!e->fp8, "%s: an fp8 engine's step changes its GEMM kernel with the row count; not supported", name);
    DH_CHECK(e->rsqrt_vec == 0, "%s: the CPU rsqrt emulation flags rows by their place in a call; not supported", name);
    DH_CHECK(g_decode_tiled_rows == 0, "%s: dh_set_tuning key 10 moves steps to the tiled kernels by row count; not supported", name);
    if (n_steps <= 0) return 0;
    e->seq_slot = e->seq_meta;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i32_kernel, dim3(1), dim3(1), 0, s, e->step_dev, (int32_t)first_step);
    DH_LAUNCH_CHECK();
    dh_engine::GKey key;                                // rsqrt_vec, tiled_rows: 0, the step reads neither; seed: the draw's, else 0
    key.tokens = tokens; key.tok_ld = tok_ld; key.length = length; key.done = done;
    key.n_seq = n_seq; key.top_k = top_k; key.temp = temperature; key.eos = eos_id; key.seed = seed;
    key.limit = limit; key.n_all = n_seq; key.max_new = max_new_tokens;
    key.spec = n_draft; key.drafts = drafts; key.counters = counters; key.spec_draw = draw;
    key.ctl = step_ctl(e, STEP_VERIFY, top_k, draw);
    return launch_steps(e, key, n_steps, s);
}
}  // namespace

extern "C" int dh_engine_decode_spec(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, const int32_t* limit,
                                     int n_seq, int max_new_tokens, int n_draft, const int64_t* drafts, int32_t* counters, int n_steps,
                                     float temperature, int64_t eos_id, int first_step, void* stream) {
    return decode_spec_call("dh_engine_decode_spec", false, e, tokens, tok_ld, length, done, limit, n_seq, max_new_tokens, n_draft, drafts,
                            counters, n_steps, temperature, 1, eos_id, 0, first_step, stream);
}

extern "C" int dh_engine_decode_spec_draw(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done, const int32_t* limit,
                                          int n_seq, int max_new_tokens, int n_draft, const int64_t* drafts, int32_t* counters, int n_steps,
                                          float temperature, int top_k, int64_t eos_id, uint64_t seed, int first_step, void* stream) {
    return decode_spec_call("dh_engine_decode_spec_draw", true, e, tokens, tok_ld, length, done, limit, n_seq, max_new_tokens, n_draft, drafts,
                            counters, n_steps, temperature, top_k, eos_id, seed, first_step, stream);
}

// dh_engine_reserve_beams and dh_engine_reserve_beam_tiles (`name`): the candidates' workspace, and `need` elements in the scratch
// *scratch of *have elements (`what` it is, for the refusal)
static int reserve_beam_ws(dh_engine* e, const char* name, const char* what, size_t need, bf16_t** scratch, size_t* have) {
    if (e->beam_cand_ids && need <= *have) return 0;
    // the captured steps hold the old addresses
    DH_HIP(hipDeviceSynchronize());
    for (auto& g : e->graphs) hipGraphExecDestroy(g.exec);
    e->graphs.clear();
    if (!e->beam_cand_ids) {
        const size_t n = (size_t)e->max_batch * 2 * DH_MAX_BEAMS;
        if (dmalloc(e, &e->beam_cand_ids, n) || dmalloc(e, &e->beam_cand_lp, n)) {
            dh_set_error("%s: device allocation failed (%s)", name, dh_last_error());
            return 2;
        }
    }
    if (need > *have) {      // on failure the engine keeps the scratch it had
        bf16_t* p = nullptr;
        if (hipMalloc((void**)&p, need * sizeof(bf16_t)) != hipSuccess) {
            (void)hipGetLastError();
            dh_set_error("%s: %.2f GiB of %s scratch could not be allocated", name, need * 2 / 1073741824.0, what);
            return 2;
        }
        hipFree(*scratch);
        e->dev_bytes += (int64_t)((need - *have) * sizeof(bf16_t));
        *scratch = p;
        *have = need;
    }
    return 0;
}

extern "C" int dh_engine_reserve_beams(dh_engine* e, int W, int max_new_tokens) {
    DH_CHECK(e, "dh_engine_reserve_beams: null engine");
    DH_CHECK(W >= 1 && W <= DH_MAX_BEAMS && max_new_tokens > 0, "dh_engine_reserve_beams: W=%d (1 .. %d) beams, %d new tokens", W,
             DH_MAX_BEAMS, max_new_tokens);
    DH_CHECK(!e->kv8 && !e->fp8, "dh_engine_reserve_beams: an fp8 engine has no beam step");
    const int nt_max = std::min(beam_tiles(max_new_tokens), e->s_max / 32);
    const size_t need = W == 1 ? 0 : (size_t)e->max_batch * 2 * e->d.n_layer * e->d.n_groups * nt_max * e->d.head_size * 32;
    return reserve_beam_ws(e, "dh_engine_reserve_beams", "re-parenting", need, &e->beam_scratch, &e->beam_scratch_elems);
}

extern "C" int dh_engine_reserve_beam_tiles(dh_engine* e, int W, int max_new_tokens) {
    DH_CHECK(e, "dh_engine_reserve_beam_tiles: null engine");
    DH_CHECK(W >= 1 && W <= DH_MAX_BEAMS && max_new_tokens > 0, "dh_engine_reserve_beam_tiles: W=%d (1 .. %d) beams, %d new tokens", W,
             DH_MAX_BEAMS, max_new_tokens);
    DH_CHECK(!e->kv8 && !e->fp8, "dh_engine_reserve_beam_tiles: an fp8 engine has no beam step");
    const int nt = std::min(beam_tiles(max_new_tokens), e->s_max / 32);
    DH_CHECK(nt <= DH_MAX_BEAM_TILES, "dh_engine_reserve_beam_tiles: %d new tokens span %d tiles, a tile table holds %d per row",
             max_new_tokens, nt, DH_MAX_BEAM_TILES);
    const size_t need = W == 1 ? 0 : (size_t)e->max_batch * 2 * e->d.n_layer * e->d.n_groups * e->d.head_size * 32;
    return reserve_beam_ws(e, "dh_engine_reserve_beam_tiles", "one-tile", need, &e->beam_tile_scratch, &e->beam_tile_scratch_elems);
}

extern "C" int dh_engine_set_beam_tiles(dh_engine* e, int32_t* tab, int n_tiles) {
    DH_CHECK(e, "dh_engine_set_beam_tiles: null engine");
    DH_CHECK(!tab || (n_tiles >= 1 && n_tiles <= DH_MAX_BEAM_TILES), "dh_engine_set_beam_tiles: n_tiles=%d tiles per row, 1 .. %d are supported",
             n_tiles, DH_MAX_BEAM_TILES);
    DH_CHECK(!tab || !e->fp8, "dh_engine_set_beam_tiles: an fp8 or MXFP4 engine has no beam step; not supported");
    DH_CHECK(!tab || !e->kv8, "dh_engine_set_beam_tiles: the table names bf16 cache tiles; an fp8 KV cache is not supported");
    e->beam_tab = tab;
    e->beam_tab_nt = tab ? n_tiles : 0;
    return 0;
}

extern "C" int dh_engine_decode_beam(dh_engine* e, const dh_beam_state* st, const int32_t* prompt_len, int n_utt, int W,
                                     int max_new_tokens, int n_steps, int64_t eos_id, int first_step, void* stream) {
    DH_CHECK(e && st && prompt_len, "dh_engine_decode_beam: null argument");
    DH_CHECK(st->cum && st->n_steps && st->done && st->beam_tok && st->beam_parent && st->beam_lp && st->beam_cum && st->fin_step &&
             st->fin_parent && st->fin_score && st->fin_lp && st->n_fin, "dh_engine_decode_beam: the beam state has a null array");
    DH_CHECK(W >= 1 && W <= DH_MAX_BEAMS, "dh_engine_decode_beam: W=%d beams, 1 .. %d are supported", W, DH_MAX_BEAMS);
    DH_CHECK(n_utt > 0 && max_new_tokens > 0, "dh_engine_decode_beam: bad shape");
    DH_CHECK(first_step >= 1, "dh_engine_decode_beam: first_step=%d, step 0 is the caller's dh_beam_select_bf16 on the prefill's logits", first_step);
    const int64_t rows = (int64_t)n_utt * W;
    DH_CHECK(rows <= e->max_batch, "dh_engine_decode_beam: %d utterances x %d beams exceed the engine's %d KV slots", n_utt, W, e->max_batch);
    DH_CHECK(rows <= MAX_DECODE_ROWS, "dh_engine_decode_beam: %d x %d rows exceed the streaming step's %d", n_utt, W, MAX_DECODE_ROWS);
    DH_CHECK(rows <= e->row_cap && rows <= e->max_tokens, "dh_engine_decode_beam: %d rows, the workspaces hold %d of max_tokens = %d",
             (int)rows, e->row_cap, e->max_tokens);
    DH_CHECK(e->set.ngram == 0, "dh_engine_decode_beam: no_repeat_ngram=%d is set; a beam's history lives on the host, so the device cannot "
             "form its ban set", e->set.ngram);
    // under device histories (dh_engine_set_beam_history) the two that stay refused are refused for what they would mean, not for where
    // a beam's text lives: a penalised or boosted value would rank the candidates and be summed into the scores
    DH_CHECK(!dh_penalty_on(e->set.pen), "dh_engine_decode_beam: penalties are set (repetition=%g, frequency=%g, presence=%g); %s",
             (double)e->set.pen.repetition, (double)e->set.pen.frequency, (double)e->set.pen.presence,
             e->beam_hist ? "a penalised logit would change what a candidate's rank and a beam's score mean, which beam search does not define"
                          : "a beam's history lives on the host, so the device cannot count it");
    DH_CHECK(e->set.bias.n == 0, "dh_engine_decode_beam: a bias of %d entries is set; %s", e->set.bias.n,
             e->beam_hist ? "a boosted logit would change what a candidate's rank and a beam's score mean, which beam search does not define"
                          : "a beam's history lives on the host, so the device cannot match it");
    DH_CHECK(!e->set.aut.on(), "dh_engine_decode_beam: an automaton set of %d states is set; a re-parented beam would have to take over its "
             "parent's state, which the selection does not carry", e->set.aut.n_states);
    DH_CHECK(e->set.stop.n_seqs == 0 || e->beam_hist, "dh_engine_decode_beam: %d stop sequences are set; a beam's history lives on the host, so the device "
             "cannot match a sequence against it (the stop set alone goes with beam search)", e->set.stop.n_seqs);
    DH_CHECK(!e->set.stop.on() || e->stop_fin_tok, "dh_engine_decode_beam: a stop set is set without beam_fin_tok, the ids that end the pool entries");
    DH_CHECK(e->beam_hist_ngram == 0 || e->d.vocab <= 131072, "dh_engine_decode_beam: vocab=%d exceeds the 131072 ids of the sampler's LDS row "
             "(beam history ngram=%d)", e->d.vocab, e->beam_hist_ngram);
    DH_CHECK(e->d.vocab >= 2 * W, "dh_engine_decode_beam: vocab=%d is below the 2 W = %d candidates of a row", e->d.vocab, 2 * W);
    DH_CHECK(!e->fp8, "dh_engine_decode_beam: an fp8 engine's step changes its GEMM kernel with the row count; not supported");
    DH_CHECK(!e->kv8, "dh_engine_decode_beam: the re-parenting copies bf16 cache tiles; an fp8 KV cache is not supported");
    DH_CHECK(e->rsqrt_vec == 0, "dh_engine_decode_beam: the CPU rsqrt emulation flags rows by their place in a call; not supported");
    DH_CHECK(g_decode_tiled_rows == 0, "dh_engine_decode_beam: dh_set_tuning key 10 moves steps to the tiled kernels by row count; not supported");
    DH_CHECK(e->shared_rows == 0 || e->shared_rows == W, "dh_engine_decode_beam: shared-prompt attention is set for group_rows=%d rows per "
             "utterance, the call has W=%d beams", e->shared_rows, W);
    if (int rc = check_shared_call(e, "dh_engine_decode_beam", (int)rows, e->shared_rows)) return rc;
    const int nt_max = std::min(beam_tiles(max_new_tokens), e->s_max / 32);
    if (e->beam_tab) {                                  // "Beam KV tile table"
        DH_CHECK(W >= 2, "dh_engine_decode_beam: a tile table is set and W=1; a single beam continues itself and has no sibling slot");
        DH_CHECK(e->shared_rows == W, "dh_engine_decode_beam: a tile table is set; its attention is the shared-prompt kernel's variant, which "
                 "needs dh_engine_set_shared_prompt with group_rows = W = %d (it is %d)", W, e->shared_rows);
        DH_CHECK(e->beam_tab_nt == nt_max, "dh_engine_decode_beam: the tile table holds %d tiles per row, %d new tokens in a cache of %d "
                 "positions span %d", e->beam_tab_nt, max_new_tokens, e->s_max, nt_max);
        DH_CHECK(e->beam_cand_ids && (size_t)rows * 2 * e->d.n_layer * e->d.n_groups * e->d.head_size * 32 <= e->beam_tile_scratch_elems,
                 "dh_engine_decode_beam: a tile table is set without its one-tile scratch for W=%d (dh_engine_reserve_beam_tiles)", W);
    } else {
        DH_CHECK(e->beam_cand_ids && (W == 1 || (size_t)rows * 2 * e->d.n_layer * e->d.n_groups * nt_max * e->d.head_size * 32 <= e->beam_scratch_elems),
                 "dh_engine_decode_beam: the re-parenting scratch is too small for W=%d and %d new tokens (dh_engine_reserve_beams)", W, max_new_tokens);
    }
    if (n_steps <= 0) return 0;
    e->seq_slot = e->seq_meta;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(set_i32_kernel, dim3(1), dim3(1), 0, s, e->step_dev, (int32_t)(first_step - 1));   // the prep kernel counts it up
    DH_LAUNCH_CHECK();
    dh_engine::GKey key;                                // tokens, top_k, temp, seed: the selection has none
    key.tok_ld = max_new_tokens; key.length = st->n_steps; key.done = st->done; key.n_seq = (int)rows; key.eos = eos_id;
    key.limit = prompt_len; key.n_all = n_utt; key.max_new = max_new_tokens;
    key.ctl = step_ctl(e, STEP_BEAM, 0);
    key.shared_rows = e->shared_rows; key.shared_plen = e->shared_plen;
    key.beam_w = W; key.beam = *st; key.stop_fin_tok = e->stop_fin_tok; key.beam_hist = e->beam_hist; key.beam_ngram = e->beam_hist_ngram;
    key.beam_tab = e->beam_tab; key.beam_tab_nt = e->beam_tab_nt;
    return launch_steps(e, key, n_steps, s);
}

extern "C" int dh_engine_set_beam_history(dh_engine* e, int64_t* tokens, int ngram) {
    DH_CHECK(e, "dh_engine_set_beam_history: null engine");
    DH_CHECK(ngram >= 0 && ngram <= 8, "dh_engine_set_beam_history: ngram=%d is not in 0 .. 8", ngram);
    DH_CHECK(ngram == 0 || e->d.vocab <= 131072, "dh_engine_set_beam_history: ngram=%d with vocab=%d, which exceeds the 131072 ids of the "
             "sampler's LDS row", ngram, e->d.vocab);
    DH_CHECK(tokens || ngram == 0, "dh_engine_set_beam_history: ngram=%d without the history planes (null tokens)", ngram);
    e->beam_hist = tokens;
    e->beam_hist_ngram = tokens ? ngram : 0;
    return 0;
}

extern "C" int dh_engine_set_logprobs(dh_engine* e, float* buf) {
    DH_CHECK(e, "dh_engine_set_logprobs: null engine");
    e->set.logprobs = buf;
    return 0;
}

extern "C" int dh_engine_set_top_logprobs(dh_engine* e, int k, int32_t* ids, float* lp) {
    DH_CHECK(e, "dh_engine_set_top_logprobs: null engine");
    DH_CHECK(k >= 0 && k <= 8 && k <= e->d.vocab, "dh_engine_set_top_logprobs: k must be 0 .. min(8, vocab)");
    const bool on = k > 0 && ids && lp;
    e->set.top_n = on ? k : 0;
    e->set.top_ids = on ? ids : nullptr;
    e->set.top_lp = on ? lp : nullptr;
    return 0;
}

extern "C" int dh_engine_set_token_mask(dh_engine* e, const uint32_t* mask, int mask_ld) {
    DH_CHECK(e, "dh_engine_set_token_mask: null engine");
    DH_CHECK(!mask || mask_ld >= (e->d.vocab + 31) / 32, "dh_engine_set_token_mask: mask_ld=%d is below the %d words of a %d-token mask row",
             mask_ld, (e->d.vocab + 31) / 32, e->d.vocab);
    e->set.mask = mask;
    e->set.mask_ld = mask ? mask_ld : 0;
    return 0;
}

extern "C" int dh_engine_set_no_repeat_ngram(dh_engine* e, int ngram, const int32_t* start) {
    DH_CHECK(e, "dh_engine_set_no_repeat_ngram: null engine");
    DH_CHECK(ngram >= 0 && ngram <= 8, "dh_engine_set_no_repeat_ngram: ngram=%d is not in 0 .. 8", ngram);
    DH_CHECK(ngram == 0 || start, "dh_engine_set_no_repeat_ngram: ngram=%d needs `start`, the sequences' prompt lengths", ngram);
    DH_CHECK(ngram == 0 || e->d.vocab <= 131072, "dh_engine_set_no_repeat_ngram: vocab=%d exceeds the 131072 ids of the sampler's LDS row",
             e->d.vocab);
    e->set.ngram = ngram;
    e->ngram_start = ngram ? start : nullptr;
    return 0;
}

extern "C" int dh_engine_set_stop(dh_engine* e, const dh_stop_spec* stop, const int32_t* start, int32_t* beam_fin_tok) {
    DH_CHECK(e, "dh_engine_set_stop: null engine");
    dh_stop_args sa;
    if (int rc = dh_stop_pack("dh_engine_set_stop", stop, start != nullptr, sa)) return rc;
    e->set.stop = sa;
    e->stop_start = sa.n_seqs ? start : nullptr;
    e->stop_fin_tok = sa.on() ? beam_fin_tok : nullptr;       // sequences end pool entries too, under device histories
    return 0;
}

extern "C" int dh_engine_set_nucleus(dh_engine* e, float top_p, float min_p) {
    DH_CHECK(e, "dh_engine_set_nucleus: null engine");
    dh_nucleus_args nuc;
    if (int rc = dh_nucleus_pack("dh_engine_set_nucleus", top_p, min_p, nuc)) return rc;
    e->set.nuc = nuc;
    return 0;
}

extern "C" int dh_engine_set_penalties(dh_engine* e, const dh_penalty_args* penalties, const int32_t* start) {
    DH_CHECK(e, "dh_engine_set_penalties: null engine");
    dh_penalty_args pen;
    if (int rc = dh_penalty_pack("dh_engine_set_penalties", penalties, pen)) return rc;
    const bool on = dh_penalty_on(pen);
    DH_CHECK(!on || start, "dh_engine_set_penalties: penalties need `start`, the sequences' prompt lengths");
    DH_CHECK(!on || e->d.vocab <= 131072, "dh_engine_set_penalties: vocab=%d exceeds the 131072 ids of the sampler's LDS row", e->d.vocab);
    e->set.pen = on ? pen : DH_PENALTY_OFF;
    e->pen_start = on ? start : nullptr;
    return 0;
}

extern "C" int dh_engine_set_bias(dh_engine* e, const dh_bias_spec* bias, const int32_t* start) {
    DH_CHECK(e, "dh_engine_set_bias: null engine");
    dh_bias_args ba;
    if (int rc = dh_bias_pack("dh_engine_set_bias", bias, e->d.vocab, start != nullptr, ba)) return rc;
    e->set.bias = ba;
    e->bias_start = ba.n ? start : nullptr;
    return 0;
}

extern "C" int dh_engine_set_automaton(dh_engine* e, const dh_automaton_spec* automaton, const int32_t* start) {
    DH_CHECK(e, "dh_engine_set_automaton: null engine");
    dh_automaton_args aa;
    if (int rc = dh_automaton_pack("dh_engine_set_automaton", automaton, e->d.vocab, start != nullptr, aa)) return rc;
    e->set.aut = aa;
    e->aut_start = aa.on() ? start : nullptr;
    return 0;
}

extern "C" int dh_engine_set_shared_prompt(dh_engine* e, int group_rows, const int32_t* d_prompt_len) {
    DH_CHECK(e, "dh_engine_set_shared_prompt: null engine");
    if (group_rows == 0 || d_prompt_len == nullptr) {
        e->shared_rows = 0;
        e->shared_plen = nullptr;
        return 0;
    }
    DH_CHECK(group_rows >= 2 && group_rows <= DH_MAX_SAMPLES, "dh_engine_set_shared_prompt: group_rows=%d: 2 .. %d rows of an utterance "
             "share a prompt (0 turns it off)", group_rows, DH_MAX_SAMPLES);
    if (int rc = check_shared_call(e, "dh_engine_set_shared_prompt", 0, group_rows)) return rc;
    e->shared_rows = group_rows;
    e->shared_plen = d_prompt_len;
    return 0;
}

extern "C" int dh_engine_set_cpu_rsqrt_emulation(dh_engine* e, int vec_width, int whole_call) {
    DH_CHECK(e && vec_width >= 0, "dh_engine_set_cpu_rsqrt_emulation: bad argument");
    e->rsqrt_vec = vec_width;
    e->rsqrt_whole = whole_call != 0;
    return 0;
}

extern "C" int dh_engine_set_timing(dh_engine* e, int on) {
    DH_CHECK(e, "dh_engine_set_timing: null engine");
    e->tm.on = on != 0;
    for (auto& v : e->tm.ev) {
        for (auto& p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
        v.clear();
    }
    return 0;
}

extern "C" int dh_engine_get_timing(dh_engine* e, int which, double* h_ms, int64_t* h_launches) {
    DH_CHECK(e && which >= 0 && which < 4 && h_ms && h_launches, "dh_engine_get_timing: bad argument");
    DH_HIP(hipDeviceSynchronize());
    double tot = 0;
    for (auto& p : e->tm.ev[which]) {
        float ms = 0;
        DH_HIP(hipEventElapsedTime(&ms, p.first, p.second));
        tot += ms;
    }
    *h_ms = tot;
    *h_launches = (int64_t)e->tm.ev[which].size();
    return 0;
}
