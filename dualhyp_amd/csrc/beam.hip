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

}  // namespace

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
