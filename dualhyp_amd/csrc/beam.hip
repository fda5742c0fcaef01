// The selection step of beam search (include/dualhyp_hip.h, "Beam search"): the rows' 2 W candidates by dh_token_top_logprobs_bf16 —
// row_logsum + row_top of sampling.hip, untouched; under a token mask by dh_token_top_logprobs_bf16_mask, the first 2 W allowed ids of
// the raw row's order with the raw row's values — then this file's kernel, one wave per utterance, that merges the at most 32
// candidates, walks them and writes the step's records.  tests/beam_reference.py is the host model.
#include "common.h"

namespace {

constexpr int MAX_W = DH_MAX_BEAMS;
constexpr int MAX_CAND = MAX_W * 2 * MAX_W;
static_assert(2 * MAX_W <= DH_MAX_TOP_LOGPROBS, "a row offers 2 W alternatives");

// Candidate (b, j) = alternative j of live row b, score = cum[b] + lp: one fp32 add.  A row's list is sorted already (value
// descending, then index ascending, and the add of one cum keeps the order), so the order of the definition — score descending, then
// b ascending, then j ascending — is the merge of the rows' lists by their heads, the lower b winning a tie.  Lane 0 does the merge and
// the walk, 2 W places of at most W compares each: nothing here is worth a second lane, and no atomic decides anything.
// hist ("Beam histories" of the header; null: the step without them — lanes 1 .. 63 leave behind the barrier as they always did): int64
// [2][n_utt * W][max_new], plane (step - 1) & 1 holds the live beams' tokens behind the step before, plane step & 1 receives them behind
// this one, so the launch never reads what it writes and any parent map is right.  Before the walk lane c tests whether candidate c
// completes a stop sequence on its own beam's text (stop_hit on the last 7 ids of H(u, step - 1, b) and the candidate, m = step + 1);
// behind it the chosen parents and tokens go through LDS and the wave copies H(parent)[0 .. step) into every live beam's row and
// appends the token.
__global__ __launch_bounds__(64) void beam_merge_kernel(const int32_t* __restrict__ cand_ids, const float* __restrict__ cand_lp,
                                                        int rows_per_utt, int W, int max_new, int64_t eos_id, int step_arg,
                                                        const int32_t* __restrict__ step_dev, dh_beam_state st, dh_stop_args sa,
                                                        int32_t* __restrict__ fin_tok, int64_t* hist) {
    const int u = blockIdx.x, tid = threadIdx.x;
    if (st.done[u]) return;                                          // frozen
    const int step = step_dev ? *step_dev : step_arg;                // device counter keeps a captured graph replayable
    if (step < 0 || step >= max_new) return;                         // never a record outside the arrays
    __shared__ int32_t s_id[MAX_CAND];
    __shared__ float s_lp[MAX_CAND], s_sc[MAX_CAND];
    __shared__ int s_head[MAX_W];
    __shared__ int s_end[MAX_CAND], s_par[MAX_W], s_tok[MAX_W];      // under a history only
    const uint32_t* __restrict__ stop_set = sa.set;
    const bool seqs = hist != nullptr && sa.n_seqs != 0;
    const size_t plane = (size_t)gridDim.x * W * max_new;
    const int64_t* h_rd = hist ? hist + (size_t)((step - 1) & 1) * plane + (size_t)u * W * max_new : nullptr;
    const int K = 2 * W, n = rows_per_utt * K;
    if (tid < n) {
        const int b = tid / K;
        const float lp = cand_lp[(size_t)u * n + tid];
        s_id[tid] = cand_ids[(size_t)u * n + tid];
        s_lp[tid] = lp;
        s_sc[tid] = st.cum[(size_t)u * W + b] + lp;
        if (seqs) {
            int w[DH_MAX_STOP_LEN];
            w[0] = s_id[tid];
#pragma unroll
            for (int k = 1; k < DH_MAX_STOP_LEN; ++k) w[k] = step - k >= 0 ? (int)h_rd[(size_t)b * max_new + step - k] : -1;
            dh_stop_args sq = sa;
            sq.set = nullptr;                                        // the set is the walk's own test
            s_end[tid] = stop_hit(sq, w, step + 1);
        }
    }
    if (tid < MAX_W) s_head[tid] = 0;
    __syncthreads();
    if (tid != 0 && !hist) return;
    if (tid == 0) {
        int n_live = 0, nf = st.n_fin[u];
        const size_t rec = ((size_t)u * max_new + step) * W;
        for (int p = 0; p < K && n_live < W; ++p) {
            int b = -1;
            float best = 0.f;
            for (int r = 0; r < rows_per_utt; ++r) {
                if (s_head[r] >= K) continue;
                const float sc = s_sc[r * K + s_head[r]];
                if (b < 0 || sc > best) { b = r; best = sc; }
            }
            if (b < 0) break;
            const int c = b * K + s_head[b]++;
            // a stop id (include/dualhyp_hip.h, "Stop conditions") ends the hypothesis exactly as the EOS does; fin_tok tells them apart
            const bool ends = (eos_id >= 0 && (int64_t)s_id[c] == eos_id) ||
                              (stop_set && s_id[c] >= 0 && ((stop_set[s_id[c] >> 5] >> (s_id[c] & 31)) & 1u)) || (seqs && s_end[c]);
            if (ends) {
                if (p < W && nf < W) {
                    if (fin_tok) fin_tok[(size_t)u * W + nf] = s_id[c];
                    st.fin_step[(size_t)u * W + nf] = step;
                    st.fin_parent[(size_t)u * W + nf] = b;
                    st.fin_score[(size_t)u * W + nf] = best;
                    st.fin_lp[(size_t)u * W + nf] = s_lp[c];
                    ++nf;
                }
                continue;
            }
            st.beam_parent[rec + n_live] = b;
            st.beam_tok[rec + n_live] = s_id[c];
            st.beam_lp[rec + n_live] = s_lp[c];
            st.beam_cum[rec + n_live] = best;
            st.cum[(size_t)u * W + n_live] = best;                   // every cum was read before the barrier
            if (hist) { s_par[n_live] = b; s_tok[n_live] = s_id[c]; }
            ++n_live;
        }
        for (; n_live < W; ++n_live) {     // rows outside the definition (NaN) can run the lists dry: a beam that continues itself nowhere
            st.beam_parent[rec + n_live] = rows_per_utt == 1 ? 0 : n_live;
            st.beam_tok[rec + n_live] = 0;
            st.beam_lp[rec + n_live] = -INFINITY;
            st.beam_cum[rec + n_live] = -INFINITY;
            st.cum[(size_t)u * W + n_live] = -INFINITY;
            if (hist) { s_par[n_live] = rows_per_utt == 1 ? 0 : n_live; s_tok[n_live] = 0; }
        }
        st.n_fin[u] = nf;
        st.n_steps[u] = step + 1;
        if (nf >= W) st.done[u] = 1;
        else if (step + 1 >= max_new) st.done[u] = 2;                // budget spent
    }
    if (!hist) return;
    __syncthreads();
    int64_t* h_wr = hist + (size_t)(step & 1) * plane + (size_t)u * W * max_new;
    for (int w = 0; w < W; ++w) {
        const int64_t* src = h_rd + (size_t)s_par[w] * max_new;      // a parent is a row of this step: 0 .. rows_per_utt - 1
        int64_t* dst = h_wr + (size_t)w * max_new;
        for (int i = tid; i < step; i += 64) dst[i] = src[i];
        if (tid == 0) dst[step] = s_tok[w];
    }
}

// The KV step of a beam call under a tile table (include/dualhyp_hip.h, "Beam KV tile table"), in place of the re-parenting: behind the
// selection of step t the rows' table rows move from plane (t - 1) & 1 to plane t & 1, and the one OPEN tile, tile0 + cur, of a row
// that continues another beam is copied from the parent's slot — every closed tile stays where it was written.  Two launches through
// the scratch, as the re-parenting: to_scratch, the parents' tile into the row's own scratch block and the table rows (they are read
// from one plane and written to the other); then the block into the row's own slot.  So no launch reads what it writes and any parent
// map is right.  grid (pieces of 256 units of ONE tile, tables x groups, rows): fixed, what there is to do is read from the device.
// cache_tab: the engine's [2 L] table of cache pointers; null: the pair (c0, c1) of dh_beam_retile.  A row that continues itself, a
// tile that just closed, an utterance that did not take step t and a parent outside 0 .. W-1 (taken as the row itself) copy nothing.
__global__ __launch_bounds__(256) void beam_retile_kernel(bf16_t* const* __restrict__ cache_tab, bf16_t* c0, bf16_t* c1,
                                                          bf16_t* __restrict__ scratch, int32_t* tab, int nt,
                                                          const int32_t* __restrict__ beam_parent, const int32_t* __restrict__ n_steps,
                                                          const int32_t* __restrict__ plen, const int32_t* __restrict__ step_dev, int step_arg,
                                                          int W, int max_new, int n_groups, size_t block_elems, int tile_units,
                                                          int cache_tiles, int to_scratch) {
    const int row = blockIdx.z, u = row / W, w = row % W;
    const int step = step_dev ? *step_dev : step_arg;
    if (step < 1) return;                                            // step 0 is the caller's: both planes are its identity
    const int P = plen[u];
    const bool took = step < max_new && n_steps[u] == step + 1 && P >= 1;
    int parent = w, tile0 = 0, cur = 0, nxt = 0;
    if (took) {
        parent = beam_parent[((size_t)u * max_new + step) * W + w];
        parent = parent < 0 || parent >= W ? w : parent;
        tile0 = P >> 5;
        cur = ((P + step - 1) >> 5) - tile0;
        nxt = ((P + step) >> 5) - tile0;
    }
    if (to_scratch && blockIdx.x == 0 && blockIdx.y == 0) {
        const size_t plane = (size_t)gridDim.z * nt;
        const int32_t* old = tab + (size_t)((step - 1) & 1) * plane;
        int32_t* now = tab + (size_t)(step & 1) * plane;
        for (int j = threadIdx.x; j < nt; j += 256) {
            int v = w;                                               // j > cur: a tile no key has reached
            if (!took) v = old[(size_t)row * nt + j];                // frozen rows read the same entries at either parity
            else if (j < cur) v = old[((size_t)u * W + parent) * nt + j];
            else if (j == cur) v = nxt == cur ? w : parent;          // still open: the row's own, copied below; just closed: where it is
            now[(size_t)row * nt + j] = v;
        }
    }
    if (!took || parent == w || nxt != cur) return;
    if (tile0 + cur >= cache_tiles) return;                          // never past the (slot, group) block
    const int unit = blockIdx.x * 256 + threadIdx.x;
    if (unit >= tile_units) return;
    const int g = blockIdx.y % n_groups;
    typedef __attribute__((address_space(1))) bf16_t gbf16_t;
    typedef __attribute__((address_space(1))) i32x4 gi32x4;
    bf16_t* base = cache_tab ? cache_tab[blockIdx.y / n_groups] : (blockIdx.y / n_groups ? c1 : c0);
    gbf16_t* cache = (gbf16_t*)base + (size_t)g * block_elems + ((size_t)(tile0 + cur) * tile_units + unit) * 8;
    const size_t slot_elems = (size_t)n_groups * block_elems;
    gbf16_t* sc = (gbf16_t*)scratch + (((size_t)row * gridDim.y + blockIdx.y) * tile_units + unit) * 8;
    if (to_scratch) *(gi32x4*)sc = *(const gi32x4*)(cache + (size_t)(u * W + parent) * slot_elems);
    else *(gi32x4*)(cache + (size_t)row * slot_elems) = *(const gi32x4*)sc;
}

}  // namespace

int dh_beam_retile_impl(dh_bf16* const* cache_tab, dh_bf16* c0, dh_bf16* c1, int n_tabs, dh_bf16* scratch, int32_t* tab, int nt,
                        const int32_t* beam_parent, const int32_t* n_steps, const int32_t* plen, const int32_t* step_dev, int step, int rows,
                        int W, int max_new, int n_groups, int hs, int s_max, void* stream) {
    const int tile_units = hs * 4;                                   // 16-byte units of a 32-key tile
    const dim3 grid((tile_units + 255) / 256, n_tabs * n_groups, rows);
    for (int to_scratch = 1; to_scratch >= 0; --to_scratch) {
        hipLaunchKernelGGL(beam_retile_kernel, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t* const*)cache_tab, (bf16_t*)c0, (bf16_t*)c1,
                           (bf16_t*)scratch, tab, nt, beam_parent, n_steps, plen, step_dev, step, W, max_new, n_groups, (size_t)s_max * hs,
                           tile_units, s_max / 32, to_scratch);
        DH_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int dh_beam_retile(dh_bf16* k_cache, dh_bf16* vT_cache, dh_bf16* scratch, int32_t* tile_tab, int n_tiles,
                              const int32_t* beam_parent, const int32_t* n_steps, const int32_t* prompt_len, int n_utt, int W,
                              int max_new_tokens, int step, const int32_t* step_dev, int n_groups, int hs, int s_max, void* stream) {
    DH_CHECK(k_cache && vT_cache && scratch && tile_tab && beam_parent && n_steps && prompt_len, "dh_beam_retile: null argument");
    DH_CHECK(W >= 2 && W <= MAX_W, "dh_beam_retile: W=%d beams, 2 .. %d are supported (a single beam continues itself)", W, MAX_W);
    DH_CHECK(n_tiles >= 1 && n_tiles <= DH_MAX_BEAM_TILES, "dh_beam_retile: n_tiles=%d tiles per row, 1 .. %d are supported", n_tiles,
             DH_MAX_BEAM_TILES);
    DH_CHECK(n_utt >= 0 && max_new_tokens > 0 && n_groups > 0, "dh_beam_retile: bad shape");
    DH_CHECK(hs == 64 || hs == 96 || hs == 128, "dh_beam_retile: head_size %d unsupported", hs);
    DH_CHECK(s_max > 0 && s_max % 32 == 0, "dh_beam_retile: s_max=%d is no multiple of the 32 keys of a tile", s_max);
    DH_CHECK(step_dev || (step >= 1 && step < max_new_tokens), "dh_beam_retile: step %d is outside the steps 1 .. %d that re-parent", step,
             max_new_tokens - 1);
    DH_CHECK((int64_t)n_utt * W <= 65535, "dh_beam_retile: %d x %d rows exceed a grid's 65535", n_utt, W);
    if (n_utt == 0) return 0;
    return dh_beam_retile_impl(nullptr, k_cache, vT_cache, 2, scratch, tile_tab, n_tiles, beam_parent, n_steps, prompt_len, step_dev, step,
                               n_utt * W, W, max_new_tokens, n_groups, hs, s_max, stream);
}

int dh_beam_select_impl(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new, int64_t eos_id, int step,
                        const int32_t* step_dev, const dh_beam_state& st, int32_t* cand_ids, float* cand_lp, const uint32_t* mask,
                        int mask_ld, const dh_stop_args& sa, int32_t* fin_tok, void* stream, int64_t* hist, int ngram) {
    DH_CHECK(logits && cand_ids && cand_lp, "dh_beam_select_bf16: null argument");
    DH_CHECK(!sa.on() || fin_tok, "dh_beam_select_bf16: a stop set needs fin_tok, the ids that ended the pool entries");
    DH_CHECK(!mask || mask_ld >= (vocab + 31) / 32, "dh_beam_select_bf16: mask_ld=%d is below the %d words of a %d-token mask row", mask_ld,
             (vocab + 31) / 32, vocab);
    DH_CHECK(st.cum && st.n_steps && st.done && st.beam_tok && st.beam_parent && st.beam_lp && st.beam_cum && st.fin_step &&
             st.fin_parent && st.fin_score && st.fin_lp && st.n_fin, "dh_beam_select_bf16: the beam state has a null array");
    DH_CHECK(W >= 1 && W <= MAX_W, "dh_beam_select_bf16: W=%d beams, 1 .. %d are supported", W, MAX_W);
    DH_CHECK(rows_per_utt == 1 || rows_per_utt == W, "dh_beam_select_bf16: rows_per_utt=%d is neither 1 (step 0) nor W=%d", rows_per_utt, W);
    DH_CHECK(vocab >= 2 * W, "dh_beam_select_bf16: vocab=%d is below the 2 W = %d candidates of a row", vocab, 2 * W);
    DH_CHECK(n_utt >= 0 && max_new > 0, "dh_beam_select_bf16: bad shape");
    DH_CHECK(step_dev || (step >= 0 && step < max_new), "dh_beam_select_bf16: step %d is outside the %d recorded steps", step, max_new);
    DH_CHECK(ngram >= 0 && ngram <= 8, "dh_beam_select_bf16_hist: ngram=%d is not in 0 .. 8", ngram);
    DH_CHECK(ngram == 0 || vocab <= 131072, "dh_beam_select_bf16_hist: ngram=%d keeps a row's allowed-minus-banned bits in a static LDS row "
             "of 131072 ids; vocab=%d does not fit", ngram, vocab);
    DH_CHECK(hist || ngram == 0, "dh_beam_select_bf16_hist: ngram=%d without the history planes (null tokens)", ngram);
    DH_CHECK(hist || sa.n_seqs == 0, "dh_beam_select_bf16_hist: %d stop sequences without the history planes (null tokens)", sa.n_seqs);
    if (n_utt == 0) return 0;
    // mask row u serves every beam row of utterance u
    const int rc = hist && ngram > 0 ? dh_beam_top_hist_impl(logits, vocab, n_utt, rows_per_utt, W, max_new, cand_ids, cand_lp, mask, mask_ld,
                                                             hist, ngram, st.n_steps, st.done, stream)
                   : mask            ? dh_token_top_logprobs_bf16_mask(logits, vocab, 2 * W, cand_ids, cand_lp, n_utt * rows_per_utt, mask,
                                                                       mask_ld, rows_per_utt, stream)
                                     : dh_token_top_logprobs_bf16(logits, vocab, 2 * W, cand_ids, cand_lp, n_utt * rows_per_utt, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(beam_merge_kernel, dim3(n_utt), dim3(64), 0, (hipStream_t)stream, cand_ids, cand_lp, rows_per_utt, W, max_new,
                       eos_id, step, step_dev, st, sa, fin_tok, hist);
    DH_LAUNCH_CHECK();
    return 0;
}

extern "C" int dh_beam_select_bf16(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens,
                                   int64_t eos_id, int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids,
                                   float* cand_lp, void* stream) {
    DH_CHECK(st, "dh_beam_select_bf16: null beam state");
    return dh_beam_select_impl(logits, vocab, n_utt, rows_per_utt, W, max_new_tokens, eos_id, step, step_dev, *st, cand_ids, cand_lp,
                               nullptr, 0, dh_stop_args{}, nullptr, stream);
}

extern "C" int dh_beam_select_bf16_mask(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens,
                                        int64_t eos_id, int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids,
                                        float* cand_lp, const uint32_t* mask, int mask_ld, void* stream) {
    DH_CHECK(st, "dh_beam_select_bf16_mask: null beam state");
    DH_CHECK(mask, "dh_beam_select_bf16_mask: null mask (dh_beam_select_bf16 is the entry without one)");
    return dh_beam_select_impl(logits, vocab, n_utt, rows_per_utt, W, max_new_tokens, eos_id, step, step_dev, *st, cand_ids, cand_lp,
                               mask, mask_ld, dh_stop_args{}, nullptr, stream);
}

extern "C" int dh_beam_select_bf16_stop(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens,
                                        int64_t eos_id, int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids,
                                        float* cand_lp, const uint32_t* mask, int mask_ld, const dh_stop_spec* stop, int32_t* fin_tok,
                                        void* stream) {
    DH_CHECK(st, "dh_beam_select_bf16_stop: null beam state");
    DH_CHECK(!stop || stop->n_seqs == 0, "dh_beam_select_bf16_stop: %d stop sequences; the beams' histories live on the host, so the device "
             "cannot match a sequence against a beam's text (the stop set alone goes with beam search)", stop->n_seqs);
    dh_stop_args sa;
    sa.set = stop ? stop->set : nullptr;
    return dh_beam_select_impl(logits, vocab, n_utt, rows_per_utt, W, max_new_tokens, eos_id, step, step_dev, *st, cand_ids, cand_lp,
                               mask, mask ? mask_ld : 0, sa, fin_tok, stream);
}

extern "C" int dh_beam_select_bf16_hist(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens,
                                        int64_t eos_id, int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids,
                                        float* cand_lp, const uint32_t* mask, int mask_ld, const dh_stop_spec* stop, int32_t* fin_tok,
                                        const dh_beam_hist* hist, void* stream) {
    DH_CHECK(st, "dh_beam_select_bf16_hist: null beam state");
    dh_stop_args sa;
    if (int rc = dh_stop_pack("dh_beam_select_bf16_hist", stop, true, sa)) return rc;     // a beam's text starts at its history's start
    return dh_beam_select_impl(logits, vocab, n_utt, rows_per_utt, W, max_new_tokens, eos_id, step, step_dev, *st, cand_ids, cand_lp,
                               mask, mask ? mask_ld : 0, sa, fin_tok, stream, hist ? hist->tokens : nullptr, hist ? hist->ngram : 0);
}
