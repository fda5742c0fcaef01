/*
 * dualhyp_hip.h — C ABI of libdualhyp_hip.so: the MI355X (gfx950) implementation of DualHyp's
 * LLM hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 * parameter name starts with `h_`.  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Every function returns 0 on success; on failure it returns non-zero and
 * dh_last_error() describes it (thread-local).  Nothing here allocates unless it says so.
 *
 * The reference has no FFI: its boundary for this path is the Python class API
 * (ger/lora.py GPT.forward, generate/base.py generate).  Each entry point below replaces the
 * tensor program one reference function expands to on CPU/CUDA; the reference file:line is
 * given per function.  INTEGRATION.md shows the ctypes binding a maintainer of the reference
 * would add.
 *
 * dtype: bf16 = uint16_t bit pattern (storage dtype of the reference's bf16-true mode); all
 * accumulation is fp32; results are rounded to bf16 at exactly the points where the
 * reference's eager bf16 tensor program rounds.
 */
#ifndef DUALHYP_HIP_H
#define DUALHYP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t dh_bf16;

/* ABI 6 gained entries without a change to any existing one (so the number stays): dh_token_logprobs_bf16, dh_sample_bf16_ex,
 * dh_sample_rows_bf16_ex and dh_engine_set_logprobs (token log-probabilities); dh_token_top_logprobs_bf16, dh_sample_bf16_top,
 * dh_sample_rows_bf16_top and dh_engine_set_top_logprobs (token alternatives); dh_beam_select_bf16, dh_engine_reserve_beams and
 * dh_engine_decode_beam (beam search); dh_sample_bf16_mask, dh_sample_rows_bf16_mask, dh_token_top_logprobs_bf16_mask,
 * dh_beam_select_bf16_mask and dh_engine_set_token_mask (token masks); dh_sample_bf16_ngram, dh_sample_rows_bf16_ngram and
 * dh_engine_set_no_repeat_ngram (no-repeat n-grams); dh_sample_bf16_stop, dh_sample_rows_bf16_stop, dh_beam_select_bf16_stop and
 * dh_engine_set_stop (stop conditions); dh_sample_bf16_nucleus, dh_sample_rows_bf16_nucleus and dh_engine_set_nucleus (nucleus
 * and min-p sampling); dh_engine_fork_slots (sampled candidates); dh_sample_bf16_penalty, dh_sample_rows_bf16_penalty and
 * dh_engine_set_penalties (penalties); dh_sample_bf16_bias, dh_sample_rows_bf16_bias and dh_engine_set_bias (contextual biasing);
 * dh_beam_select_bf16_hist and dh_engine_set_beam_history (beam histories); dh_sample_bf16_automaton, dh_sample_rows_bf16_automaton and
 * dh_engine_set_automaton (automaton constraints); dh_attn_decode_shared_bf16, dh_attn_shared_launch_count and
 * dh_engine_set_shared_prompt (shared-prompt attention); dh_attn_decode_shared_tab_bf16, dh_beam_retile, dh_engine_set_beam_tiles and
 * dh_engine_reserve_beam_tiles (beam KV tile table). */
#define DH_ABI_VERSION 6

int dh_abi_version(void);
/* Kernel-variant selector for A/B measurements inside one process (bench.py --tune k=v); never needed in production,
 * keys 4, 10 and 16 select a different fp32 summation order (low bits change), no other key changes a result bit.  Keys: 0 decode partial-sum GEMM (0 = K split over the waves of a block,
 * 1 = row-parallel with x staged in LDS); 1 prefill GEMM (0 = always 128x128 tiles, 1..3 = 256x256 loop variants on eight waves, 4 = those with persistent blocks,
 * 5 = the default: 256x256 on four waves with full-line 64-deep stages, round 3);
 * 2 SwiGLU streaming variant; 3 gemm_mid on/off; 4 phase pin of dh_linear_bf16 (0 by shape, 1 tiled, 2 decode);
 * 5 band height of the 256-tile walk; 6 / 7 first row count of the tiled decode kernels (fused epilogues / chain sums);
 * 8 gemm_dt stages; 9 128-tile stages; 10 decode steps from this many rows on the prefill kernels (0 = never);
 * 11 column tiles per wave of the K-sliced kernel; 12 rope + cache append fused into the QKV GEMM (1) or two launches;
 * 13 W through the per-wave LDS ring in gemm_mid (1) or straight to VGPRs; 14 row groups per block of the K-sliced
 * kernel above 128 rows (0 = by grid size, 8, 10); 15 8-wave SwiGLU tile in gemm_dt (0 = from 256 rows, 1 always,
 * -1 never); 16 k-steps per K-slice for K <= 4096 (8 or 16); 17 / 18 / 21 pair-sum decode GEMM (tile width, first row count, sc1 stores);
 * 19 / 20 fp8 tile edge and band height; 22 persistent blocks of the 4-wave prefill GEMM (0 never, 1 where the epilogue loads nothing: default,
 * 2 always); 23 a forward asked for the last position's logits only runs the last block's attention output, projection and MLP on each
 * sequence's last row (1, default) or on every row (0) — same bits either way (dh_engine_forward). */
int dh_set_tuning(int key, int value);
/* Debug aid for tests: a bit mask of the GEMM kernels launched on the calling thread since the last reset, one bit per launch
 * site (enum DhGemmRoute in csrc/gemm.h; tests/gemm_exact_reference.py mirrors the numbering); reset != 0 clears it after
 * the read.  Host side only: a thread-local OR next to each launch.  The quantised GEMMs are recorded as well: dh_linear_fp8*
 * (streaming with 1 / 2 / 4 row groups, the 128-tile with 4 or 2 stages, the 256-tile) and dh_linear_mxfp4* (streaming with
 * 1 / 2 / 4 row groups, tiled with 4 or 2 stages) and dh_linear_mxfp4a6* (the same five, appended after them); the fp32-out entry
 * points record the streaming routes of their bf16 forms. */
uint64_t dh_debug_gemm_routes(int reset);
const char* dh_last_error(void);
/* Name of the first visible device's gcnArch ("gfx950") into buf; fails when no GPU. */
int dh_device_info(char* h_buf, int h_buf_len, int* h_num_cu, int64_t* h_hbm_bytes);

/* ------------------------------------------------------------------ elementwise / layout */

/* out[t,:] = wte[ids[t],:]            — nn.Embedding, ger/lora.py:537 */
int dh_embed_bf16(const int64_t* ids, const dh_bf16* wte, dh_bf16* out, int n_tok, int d,
                  int vocab, void* stream);

/* RMSNorm in the storage dtype — ger/rmsnorm.py:17-21:
 *   ms = bf16(mean_fp32(bf16(x*x))) ; r = bf16(rsqrt(bf16(ms+eps))) ; out = bf16(w*bf16(x*r))
 * If `resid` is non-NULL the input is x := bf16(x + resid) and `sum_out` (if non-NULL)
 * receives that sum (the residual stream update of ger/model.py:185-186).
 * row_tail (nullable, uint8 per row): rows flagged non-zero use r = bf16(1 / bf16(sqrt(t)))
 * instead of bf16(1/sqrt(t)).  That is what the reference's CPU path computes for the rows
 * torch's bf16 rsqrt handles in its scalar tail loop (the last n %% 32 rows of a call on AVX-512
 * hosts, hence every single-token decode call) — SURVEY.md quirk list, DESIGN.md Q11. */
int dh_rmsnorm_bf16(const dh_bf16* x, const dh_bf16* resid, const dh_bf16* w, dh_bf16* out,
                    dh_bf16* sum_out, int rows, int d, float eps, const uint8_t* row_tail,
                    void* stream);

/* Split the fused QKV projection, rotate q and k, append k/v to the KV cache —
 * ger/model.py:216-259.  qkv: [n_tok, n_groups*(q_per_kv+2)*hs] in the group-interleaved layout
 * [q0..q(q_per_kv-1) k v] per group (scripts/convert_hf_checkpoint.py:187-202).
 *   q_out  [n_tok, n_head, hs]            rotated queries
 *   k_cache [n_slots, n_groups, s_max, hs]   (compact GQA cache; the reference's 8x expansion
 *   vT_cache[n_slots, n_groups, hs, s_max]    ger/model.py:225-227 is not materialised)
 * tok_slot[t], tok_pos[t]: cache slot (sequence) and position of token t.
 * k_out / v_out (nullable): plain [n_tok, n_groups, hs] copies of the rotated k and of v, kept by
 * the training forward for the attention backward. */
int dh_qkv_rope_cache_bf16(const dh_bf16* qkv, const dh_bf16* cos, const dh_bf16* sin,
                           const int32_t* tok_slot, const int32_t* tok_pos, dh_bf16* q_out,
                           dh_bf16* k_cache, dh_bf16* vT_cache, dh_bf16* k_out, dh_bf16* v_out,
                           int n_tok, int n_head, int n_groups, int hs, int s_max, void* stream);

/* ------------------------------------------------------------------ GEMMs (MFMA) */

/* Epilogue selector for dh_linear_bf16 */
#define DH_EPI_PLAIN   0   /* y = bf16(acc)                                 F.linear            */
#define DH_EPI_LORA    1   /* y = bf16(bf16(acc) + bf16(bf16(lora_acc)*s))  ger/lora.py:159-166,388-402 */
#define DH_EPI_SWIGLU  2   /* y = bf16(bf16(silu(bf16(acc1))) * bf16(acc2)) ger/model.py:313-315 */
#define DH_EPI_ADAPTER 3   /* y = bf16(scale * bf16(bf16(acc) + bias))      ger/lora.py:70-71   */

/* y[M,N] = epilogue(x[M,K] · W[N,K]^T).  K % 64 == 0, N % 8 == 0.
 *  LORA   : xa [M, xa_ld] = bf16(x·A^T) (from dh_linear_bf16 PLAIN with W=A), lora_b [N,16]
 *           (rank zero-padded to 16).  Output column n uses xa columns
 *           [16*seg, 16*seg+16) with seg = (n >= split0) + (n >= split1): the contiguous
 *           [Q|K|V] placement of ger/lora.py:226-234,343-347 (quirk Q2).  A boundary inside [0, N) must be
 *           a multiple of 32; pass N,N for a single segment (any value >= N means "no such segment").
 *  SWIGLU : w2 [N,K] second weight (fc_2); W is fc_1.
 *  ADAPTER: vec_a = adapter_scale[N], vec_b = adapter_bias[N].
 *  resid  : if non-NULL, y = bf16(resid + y_epilogue)  (residual add of ger/model.py:185-186)
 *  M may be any value >= 1; for M <= 32 a weight-streaming kernel is used, otherwise the tiled MFMA kernels
 *  (the engine additionally pins the kernel family per phase: see DESIGN.md, batch invariance). */
int dh_linear_bf16(const dh_bf16* x, const dh_bf16* w, dh_bf16* y, int M, int N, int K,
                   int epilogue, const dh_bf16* w2, const dh_bf16* xa, int xa_ld,
                   const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                   const dh_bf16* vec_a, const dh_bf16* vec_b, const dh_bf16* resid,
                   void* stream);

/* The fused-QKV projection of a packed prefill with the work of dh_qkv_rope_cache_bf16 in its epilogue
 * (ger/model.py:216-259 after ger/lora.py:367-402): q/k rotated, q -> q_out [M, n_head, hs], k / v appended to the
 * caches; the [M, (n_head+2g)*hs] qkv tensor is never written.  Same arithmetic and rounding points as
 * dh_linear_bf16(EPI_LORA, splits (d, d+g*hs)) followed by dh_qkv_rope_cache_bf16 — bit-identical results.
 * lora_b NULL = no LoRA.  Only for shapes the 256-tile kernel takes (M >= 256 and >= 128 tiles); smaller calls use the
 * two-step form. */
int dh_linear_qkv_rope_cache_bf16(const dh_bf16* x, const dh_bf16* w, int M, int K, const dh_bf16* xa, int xa_ld,
                                  const dh_bf16* lora_b, float lora_scale, const dh_bf16* cos, const dh_bf16* sin,
                                  const int32_t* tok_slot, const int32_t* tok_pos, dh_bf16* q_out, dh_bf16* k_cache,
                                  dh_bf16* vT_cache, int n_head, int n_groups, int hs, int s_max, void* stream);

/* Round 3 (ABI 4): the same two entry points with the LoRA DOWN-projection computed by the library — ger/lora.py:159-166, 388-402:
 *   after = W x ; after_A = lora_A(x) (bf16) ; after_B = lora_B(after_A) ; result = after + scaling * after_B
 * lora_a: [16 * nseg, K] bf16, segment s in rows 16 s .. 16 s + 15 (rank zero-padded to 16; nseg = 1 + (split0 < N) + (split1 < N),
 * 3 for the fused QKV projection).  Where the launch runs on the 4-wave 256-tile kernel and every segment boundary is a multiple of
 * 256 columns, bf16(x . A^T) rides in the GEMM's own K loop (16 more rows per stage, 4 more MFMAs per wave and k-step on the x
 * fragments already in registers, the result handed to the epilogue through LDS): no separate launch, no [M, 16 nseg] tensor, same
 * bits.  Otherwise the library runs dh_linear_bf16(x, lora_a) into xa_work and then the LORA epilogue.  xa_work: [M, 16 nseg] bf16,
 * always required (which path runs is the library's choice). */
int dh_linear_lora_bf16(const dh_bf16* x, const dh_bf16* w, dh_bf16* y, int M, int N, int K, const dh_bf16* lora_a,
                        const dh_bf16* lora_b, float lora_scale, int split0, int split1, const dh_bf16* resid,
                        dh_bf16* xa_work, void* stream);
int dh_linear_qkv_lora_rope_cache_bf16(const dh_bf16* x, const dh_bf16* w, int M, int K, const dh_bf16* lora_a,
                                       const dh_bf16* lora_b, float lora_scale, const dh_bf16* cos, const dh_bf16* sin,
                                       const int32_t* tok_slot, const int32_t* tok_pos, dh_bf16* q_out, dh_bf16* k_cache,
                                       dh_bf16* vT_cache, int n_head, int n_groups, int hs, int s_max, dh_bf16* xa_work,
                                       void* stream);

/* fp32 partial sums for the fused decode consumers below (M <= 4096 rows, weight streaming):
 *   y32[p][m][n] = sum over K-slice p of x[m,:] . W'[n,:],  W' = [w (n_main rows) ; w_ext (n_ext rows)]
 * y32: [ksplit][M][n_main+n_ext] fp32.  w_ext is the rank-padded LoRA A (so x·A^T comes out of the
 * same pass over x as x·W^T and never needs its own launch).  K %% 32 == 0, rows %% 16 == 0.
 * K-slices, in k-steps of 32: where ksplit slices of 8 or 16 k-steps tile K exactly (ceil(K/32/ksplit) = 8 or 16, the shapes the
 * engine uses), slice p is the contiguous run of k-steps [p kps, (p+1) kps).  Any other (K, ksplit <= 8): runs of 8 k-steps dealt
 * round robin, k-step ks in slice (ks / 8) %% ksplit (a slice may be empty: zeros).  The slices always add up to the full product.
 *
 * K-SLICE COMBINE ORDER of the decode family (round 3; one order for every row count, so a row's bits do not depend on
 * how many rows are decoded with it): a slice is one fp32 chain of v_mfma_f32_16x16x32_bf16 from zero, k ascending;
 * ADJACENT slices are added in pairs, (s0 + s1), (s2 + s3), ..., an unpaired last slice stands alone; the pair sums are
 * added in index order.  Producers emit either the slices (dh_linear_partial_bf16: consumers take them with pairs = 1)
 * or the pair sums (dh_linear_partial_pairs_bf16: pairs = 0, half the bytes) or the total (dh_linear_chain_bf16:
 * n_part = 1). */
int dh_linear_partial_bf16(const dh_bf16* x, const dh_bf16* w, const dh_bf16* w_ext, float* y32,
                           int M, int n_main, int n_ext, int K, int ksplit, void* stream);
/* The PAIR SUMS of those ksplit slices, y32: [(ksplit+1)/2][M][n_main+n_ext] fp32, from a tiled split-K kernel (128-row
 * tiles, both operands through LDS, one block per tile and slice pair): y32[j] = slice 2j + slice 2j+1, bit-identical
 * to adding the two partials of dh_linear_partial_bf16.  The decode GEMMs of more than 128 rows (several batches decoded
 * jointly).  Needs K %% 64 == 0, K-slices of 8 or 16 k-steps (ceil(K/32/ksplit)), whole slices. */
int dh_linear_partial_pairs_bf16(const dh_bf16* x, const dh_bf16* w, const dh_bf16* w_ext, float* y32, int M,
                                 int n_main, int n_ext, int K, int ksplit, void* stream);
/* The ksplit slices combined in the family's order (pairs, then pair sums in index order) in one launch (tiled kernel,
 * full K per block): y32 [M][n_main+n_ext] fp32.  Consumers take it with n_part = 1.  Needs K %% 64 == 0 and
 * K-slices of 8 or 16 k-steps (ceil(K/32/ksplit)); other shapes return an error. */
int dh_linear_chain_bf16(const dh_bf16* x, const dh_bf16* w, const dh_bf16* w_ext, float* y32, int M,
                         int n_main, int n_ext, int K, int ksplit, void* stream);

/* LoRA finish + residual add + RMSNorm of one decode row block — ger/lora.py:159-166,
 * ger/model.py:185-186, ger/rmsnorm.py:17-21 in one pass:
 *   h = bf16(bf16(sum_p h32[p]) + bf16(bf16(xa . B^T) * s)) ; x_out = bf16(x_resid + h) ;
 *   xn_out = RMSNorm(x_out; w_norm, eps)      (row_tail: see dh_rmsnorm_bf16)
 * h32: [n_part][rows][d+n_ext] fp32 partials, xa = bf16 of columns [d, d+16); pairs != 0: the partials are SLICES
 * (added in adjacent pairs first), pairs == 0: they are pair sums or the total (added in index order).
 * lora_b == NULL: no LoRA (n_ext = 0).  x_out may alias x_resid. */
int dh_finish_norm_bf16(const float* h32, int n_part, int pairs, int rows, int d, int n_ext,
                        const dh_bf16* lora_b, float lora_scale, const dh_bf16* x_resid,
                        const dh_bf16* w_norm, dh_bf16* x_out, dh_bf16* xn_out, float eps,
                        const uint8_t* row_tail, void* stream);

/* ------------------------------------------------------------------ attention */

/* Causal attention of a packed batch against the KV cache — ger/model.py:261,270-290 with the
 * boolean mask of ger/lora.py:530-531.  Sequence i owns q rows [q_start[i], q_start[i]+q_len[i])
 * of q [n_tok, n_head, hs]; row j of it sits at position kv_pos0[i]+j and attends cache
 * positions 0..kv_pos0[i]+j of slot seq_slot[i].  y: [n_tok, n_head*hs].  scale = 1/sqrt(hs).
 * lse (nullable): [n_tok, n_head] fp32 log-sum-exp of the scaled scores, kept for the backward. */
int dh_attn_prefill_bf16(const dh_bf16* q, const dh_bf16* k_cache, const dh_bf16* vT_cache,
                         const int32_t* seq_slot, const int32_t* q_start, const int32_t* q_len,
                         const int32_t* kv_pos0, dh_bf16* y, float* lse, int n_seq, int max_q_len,
                         int n_head, int n_groups, int hs, int s_max, void* stream);

/* One query token per sequence (decode step): q [n_seq, n_head, hs]; sequence i attends cache
 * positions 0..kv_len[i]-1 of slot seq_slot[i].  work: >= dh_attn_decode_work_bytes(). */
int64_t dh_attn_decode_work_bytes(int n_seq, int n_head, int hs, int s_max);
int dh_attn_decode_bf16(const dh_bf16* q, const dh_bf16* k_cache, const dh_bf16* vT_cache,
                        const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* y, void* work,
                        int n_seq, int n_head, int n_groups, int hs, int s_max, void* stream);

/* The whole attention sub-layer of a decode step in one launch — ger/model.py:216-261 for T = 1:
 * finish the q/k/v LoRA from the fp32 partials of dh_linear_partial_bf16 (columns
 * [qkv_dim, qkv_dim+48) = x.A^T; contiguous [Q|K|V] delta, quirk Q2), rotate q and k at position
 * kv_len-1, append k / v to the caches, attend keys 0..kv_len-1 (split over 8 waves, combined in
 * LDS; the new key is merged from registers), write y [n_seq, n_head*hs].  n_part / pairs: as dh_finish_norm_bf16. */
int dh_attn_decode_fused_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                              const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                              const dh_bf16* cos, const dh_bf16* sin, const int32_t* seq_slot,
                              const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache,
                              dh_bf16* y, int n_head, int n_groups, int hs, int s_max,
                              void* stream);

/* dh_attn_decode_fused_bf16 for S = 2 .. 8 consecutive positions of every sequence in one launch (the verify step of speculative
 * greedy decoding; S * n_head / n_groups <= 32).  qkv32 [n_part][n_seq * S][qkv_dim + n_ext] and y [n_seq * S, n_head*hs]: row
 * seq * S + j is position kv_len[seq] - 1 + j of the sequence, so kv_len[seq] counts row 0's token and nothing of rows 1 .. S-1.
 * Row j gives the bits of a single-token launch at kv_len[seq] + j that follows those of rows 0 .. j-1, and the caches end as
 * after those launches.  Rows at positions >= p_max (0 < p_max <= s_max: the last position the cache and the cos / sin tables
 * serve) append nothing; their rows of y are finite and mean nothing.  The caller keeps kv_len[seq] <= p_max.  Added under ABI 6. */
int dh_attn_verify_fused_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int S, int qkv_dim, int n_ext,
                              const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                              const dh_bf16* cos, const dh_bf16* sin, const int32_t* seq_slot,
                              const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache,
                              dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int p_max,
                              void* stream);

/* ------------------------------------------------------------------ Shared-prompt attention
 * dh_attn_decode_fused_bf16 for rows that share a prompt: the N = group_rows (2 .. 8) rows u * N + j of utterance u — sampled
 * candidates ("Sampled candidates" below) or beams ("Beam search") — whose KV slots hold the same bytes in the whole 32-key tiles of
 * the prompt.  DEFINITION: y and both caches after the call are those of dh_attn_decode_fused_bf16 with the same arguments, bit
 * for bit.  What changes is what is read: with n_sh = prompt_len[u] / 32 (prompt_len: DEVICE int32 [n_seq / N], the array
 * dh_engine_fork_slots takes; kv_len stays per row),
 *   - tiles t < n_sh are read once per block, from the slot of the utterance's row 0 (seq_slot[u * N]), for all of the block's rows;
 *     the other rows' copies of those tiles are never loaded;
 *   - tiles t >= n_sh (the partial last prompt tile and the generated keys) are read from each row's own slot and masked to
 *     key < kv_len - 1 for that row's columns and to nothing for every other column.
 * Column layout: a block serves one KV group and up to Gs = 32 / (n_head / n_groups) consecutive rows of one utterance, row jj's
 * head h in query column jj * (n_head / n_groups) + h of the 32-column MFMA the single-token kernel pays for anyway (N > Gs: several
 * blocks per utterance and group).  It holds by construction: a column's arithmetic never reads another column; tile t goes to wave
 * t % 8, ascending within a wave, as in the single-token kernel; a tile in which a column sees no key leaves its running maximum,
 * sum and accumulator unchanged; each row finishes, rotates and appends its own q / k / v at its own position and merges its own key
 * at the combine.  The caller keeps prompt_len[u] <= kv_len - 1 of every row of u and the rows' tiles < n_sh equal.
 * Refused: group_rows outside 2 .. 8, n_seq % group_rows != 0, a null prompt_len, and what dh_attn_decode_fused_bf16 refuses.
 * Added under ABI 6. */
int dh_attn_decode_shared_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                               const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                               const dh_bf16* cos, const dh_bf16* sin, const int32_t* seq_slot,
                               const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache,
                               dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int group_rows,
                               const int32_t* prompt_len, void* stream);
/* Test hook: launches of the shared-prompt attention kernel this process has issued or captured so far. */
int64_t dh_attn_shared_launch_count(void);

/* ------------------------------------------------------------------ Beam KV tile table
 * An opt-in second way to keep the beams' KV cache ("Beam search" below; dh_engine_set_beam_tiles).  The W beams of an utterance
 * advance in lockstep, so 32-key tile j of every one of its W slots is written during the same steps, and once the position has left
 * a tile no slot's copy of it is written again: a CLOSED tile is immutable.  A hypothesis therefore does not need its closed tiles in
 * its own slot, only to know which sibling's slot holds each; the one OPEN tile, the tile its next key goes into, is private.
 *   Layout.  Utterance u has the W rows r = u * W + w in slots r; P = prompt_len[u], tile0 = P >> 5 (the first tile that is not a
 *     whole prompt tile), NT = min((max_new_tokens + 30) / 32 + 1, s_max / 32) <= DH_MAX_BEAM_TILES tiles that generated keys can
 *     span.  The table is two int32 planes [2][n_utt * W][NT], the caller's, as the history planes are.  Entry [plane][r][j] is a
 *     beam index 0 .. W-1: the sibling whose slot holds tile tile0 + j of row r's hypothesis.  Entries are clamped to 0 .. W-1 before
 *     use.  Both planes start as the identity, [r][j] = w.
 *   Attention of step t (the device step counter reads t): private tile tt >= tile0 of row r is loaded from slot
 *     u * W + tab[(t - 1) & 1][r][tt - tile0]; a tile index at or beyond NT reads the row's own slot.  The shared tiles and the append
 *     into the row's own slot are those of dh_attn_decode_shared_bf16.
 *   Update behind the selection of step t, for the utterances that took it (n_steps[u] == t + 1): cur = ((P + t - 1) >> 5) - tile0,
 *     nxt = ((P + t) >> 5) - tile0, parent = beam_parent[u, t, w], new = plane t & 1, old = plane (t - 1) & 1:
 *       new[r][j] = old[u * W + parent][j]           for j < cur,
 *       new[r][cur] = w if nxt == cur (the tile is still open), else parent (it just closed),
 *       new[r][j] = w                                for j > cur;
 *     when nxt == cur and parent != w, tile tile0 + cur of the parent's slot is copied into the row's slot — every layer, K and V^T,
 *     every group — through a scratch in two launches, so no launch reads what it writes and any parent map is right.  When the tile
 *     just closed nothing is copied.  An utterance that did not take the step copies its old rows to new, so its frozen rows read the
 *     same entries at either parity.  So does an utterance whose prompt_len is below 1 (outside the definition: the re-parenting
 *     copy skips it too), and a parent outside 0 .. W-1 is taken as the row itself.  Invariant: at every step the open tile's entry
 *     is the row itself.
 *   DEFINITION: the keys and values a row's attention sees are those its own slot would hold under the re-parenting copy, so a beam
 *     call under a table records the tokens, parents, log-probabilities, scores and pool of the call without one, bit for bit.
 * dh_attn_decode_shared_tab_bf16: dh_attn_decode_shared_bf16 with the rows' private tiles read through tile_tab (device int32
 * [2][n_seq][tab_ld], tab_ld = NT, 1 .. DH_MAX_BEAM_TILES), plane (*step_dev - 1) & 1; a null step_dev means plane 0.  group_rows is
 * W.  Refused: a null table, tab_ld outside 1 .. DH_MAX_BEAM_TILES, and what dh_attn_decode_shared_bf16 refuses.
 * dh_beam_retile: the update alone, over one K / V^T cache pair ([n_utt * W slots][n_groups][s_max * hs] each, the engine's layout of
 * one layer): step (1 .. max_new_tokens - 1), or step_dev non-null: read from the device; scratch: n_utt * W x 2 x n_groups x hs * 32
 * elements.  Two launches.  Added under ABI 6. */
#define DH_MAX_BEAM_TILES 64
int dh_attn_decode_shared_tab_bf16(const float* qkv32, int n_part, int pairs, int n_seq, int qkv_dim, int n_ext,
                                   const dh_bf16* lora_b, float lora_scale, int split0, int split1,
                                   const dh_bf16* cos, const dh_bf16* sin, const int32_t* seq_slot,
                                   const int32_t* kv_len, dh_bf16* k_cache, dh_bf16* vT_cache,
                                   dh_bf16* y, int n_head, int n_groups, int hs, int s_max, int group_rows,
                                   const int32_t* prompt_len, const int32_t* tile_tab, int tab_ld, const int32_t* step_dev,
                                   void* stream);
int dh_beam_retile(dh_bf16* k_cache, dh_bf16* vT_cache, dh_bf16* scratch, int32_t* tile_tab, int n_tiles,
                   const int32_t* beam_parent, const int32_t* n_steps, const int32_t* prompt_len, int n_utt, int W,
                   int max_new_tokens, int step, const int32_t* step_dev, int n_groups, int hs, int s_max, void* stream);

/* ------------------------------------------------------------------ LoRA fine-tune backward
 * finetune/ger.py:278-285 `fabric.backward(loss / accum)` for the frozen-base / LoRA-only case: the dX
 * GEMMs reuse dh_linear_bf16 on transposed copies of the frozen weights; these are the rest. */

/* LoRA-branch dropout, ger/lora.py:96,165,391 (`nn.Dropout(p=lora_dropout)` in front of lora_A; finetune/ger.py:401 trains at
 * 0.05): y = bf16(x * m), mask = m = keep ? bf16(1 / (1 - p)) : 0, keep drawn per element from Philox4x32-10 keyed by
 * (seed, call_id) and counted by (*step_dev, element): `step_dev` is a DEVICE counter the caller bumps once per micro-step, so
 * a captured hipGraph draws new masks on every replay (null = step 0).  n % 8 == 0.  ABI 5.
 *
 * The draw, completely (tests/dropout_reference.py restates it; tests/test_hip_dropout.py holds the kernel to it bit for bit):
 *   - element i has chunk c = i / 8, half h = (i % 8) / 4 and lane e = i % 4;
 *   - counter = {lo32(c), hi32(c) * 2 + h, lo32(step), hi32(step)}, step = *step_dev (0 when step_dev is null);
 *   - key = {lo32(seed) ^ (call_id * 0x9E3779B9 mod 2^32), (hi32(seed) + call_id) mod 2^32};
 *   - draw = word e of Philox4x32-10 on (counter, key): ten rounds {c0, c1, c2, c3} <- {hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2),
 *     hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)} with M0 = 0xD2511F53, M1 = 0xCD9E8D57, the key bumped by (0x9E3779B9, 0xBB67AE85) after
 *     each round (Random123's philox4x32_10: its known-answer vectors hold);
 *   - keep iff draw >= thresh, thresh = min(floor((double)(float)p * 2^32), 0xffffffff);
 *   - m = bf16_rne(1.0f / (1.0f - p)), the subtraction and the division in fp32.  A kept element is y = bf16_rne(fp32(x) * fp32(m))
 *     and mask = m; a dropped element is +0 in both y and mask (whatever x holds: -0, inf, NaN).
 * So P(keep) = 1 - thresh / 2^32, and E[mask] = (1 - p) * m is 1.00195 at p = 0.05 (m = 1.0546875), not 1: m is rounded to bf16 as
 * torch's bf16 dropout rounds it.  n % 8 != 0, p < 0, p >= 1 and a NaN p are refused and nothing is written. */
int dh_dropout_bf16(const dh_bf16* x, dh_bf16* y, dh_bf16* mask, int64_t n, float p, uint64_t seed, uint32_t call_id,
                    const uint64_t* step_dev, void* stream);
/* act = bf16(bf16(silu(g)) * u) from stored g, u (training forward keeps both; ger/model.py:315) */
int dh_swiglu_fwd_bf16(const dh_bf16* g, const dh_bf16* u, dh_bf16* act, int64_t n, void* stream);
/* y = bf16(bf16(x . W^T) * mul), mul [M, N] bf16 (round 4, ABI 6): a plain GEMM that applies an elementwise multiplier where it
 * rounds — the bits of dh_linear_bf16 followed by a bf16 multiply (the LoRA-branch dropout mask in the fine-tune's backward).
 * Large shapes only: M >= 256, N >= 256, ceil(M/256) * ceil(N/256) >= 128. */
int dh_linear_mul_bf16(const dh_bf16* x, const dh_bf16* w, dh_bf16* y, int M, int N, int K,
                       const dh_bf16* mul, void* stream);
/* Training forward of fc_1 / fc_2 in one launch (round 4, ABI 6): act = bf16(bf16(silu(g)) * u) with g = bf16(x.W1^T), u = bf16(x.W2^T)
 * also stored ([M, I] each) for the backward — the bits of two dh_linear_bf16 launches + dh_swiglu_fwd_bf16 (ger/model.py:313-315). */
int dh_linear_swiglu_train_bf16(const dh_bf16* x, const dh_bf16* w1, const dh_bf16* w2, dh_bf16* act,
                                dh_bf16* g, dh_bf16* u, int M, int I, int K, void* stream);
/* dgu[rows, 2I] = [dact*u*silu'(g) | dact*silu(g)]   (backward of ger/model.py:315) */
int dh_swiglu_bwd_bf16(const dh_bf16* dact, const dh_bf16* g, const dh_bf16* u, dh_bf16* dgu, int rows,
                       int I, void* stream);
/* dx = d(RMSNorm)/dx . dy (+ dres)   (backward of ger/rmsnorm.py:17-21; fp32 internally) */
int dh_rmsnorm_bwd_bf16(const dh_bf16* dy, const dh_bf16* x, const dh_bf16* w, const dh_bf16* dres,
                        dh_bf16* dx, int rows, int d, float eps, void* stream);
/* conjugate rotation of dq / dk, pass-through of dv, scattered back into the fused-qkv layout
 * (backward of ger/model.py:216-246; cf. ger/fused_rotary_embedding.py:49-90) */
int dh_qkv_rope_bwd_bf16(const dh_bf16* dq, const dh_bf16* dk, const dh_bf16* dv, const dh_bf16* cos,
                         const dh_bf16* sin, const int32_t* tok_pos, dh_bf16* dqkv, int n_tok,
                         int n_head, int n_groups, int hs, void* stream);
/* out[M,N] (+)= scale * a[T,M]^T . b[T,N]   (LoRA dA / dB: contraction over tokens), fp32 out.  work (nullable):
 * >= dh_tn_accum_work_bytes(T, M, N) bytes of scratch; with it a long token loop (packed micro-batches: T > 1024) is split
 * into 512-token chunks over the grid and the chunk sums are added in index order by a second launch (deterministic). */
int64_t dh_tn_accum_work_bytes(int T, int M, int N);
int dh_tn_accum_f32(const dh_bf16* a, int lda, const dh_bf16* b, int ldb, float* out, int ldo, int T,
                    int M, int N, float scale, int accumulate, void* work, void* stream);
/* The same contraction for the three LoRA-B gradients of a fused QKV projection in one launch (round 4, ABI 6):
 * out[m][n] (+)= scale * sum_t a[t][m] * b[t][16 seg(m) + n], n < 16, seg(m) = (m >= seg0) + (m >= seg1); seg0 <= seg1 multiples of 128,
 * b [T, >= 48]; work as dh_tn_accum_work_bytes(T, M, 16). */
int dh_tn_accum_seg_f32(const dh_bf16* a, int lda, const dh_bf16* b, int ldb, float* out, int ldo, int T,
                        int M, int seg0, int seg1, float scale, int accumulate, void* work, void* stream);
/* out[row] = sum_d a[row,d]*b[row,d]   (softmax-backward row term D = rowsum(dO*O)) */
int dh_rowdot_f32(const dh_bf16* a, const dh_bf16* b, float* out, int64_t rows, int hs, void* stream);
/* src [n_tok, heads, hs] -> dst (heads * hs * n_pad elements, zero-initialised by the caller): the token-contiguous copy the
 * backward kernels take as a transposed MFMA operand, in FRAGMENT ORDER (csrc/attention_bwd.hip: tfrag_off — per head and 32-token
 * tile the 2 x hs/32 fragments of v_mfma_f32_32x32x16_bf16, 64 lanes x 8 values each, so a wave's fragment is one contiguous 1-KiB
 * load); sequence i starts at padded token pad_start[i] (multiple of 32). */
int dh_transpose_pad_bf16(const dh_bf16* src, dh_bf16* dst, const int32_t* tok_seq,
                          const int32_t* q_start, const int32_t* pad_start, int n_tok, int heads,
                          int hs, int n_pad, void* stream);
/* The same copy from the INVERSE map (round 4, ABI 6): pad_tok[p] = token of padded position p, or -1 for padding (written as
 * zeros: dst needs no memset).  16-byte accesses both ways; one block per padded 32-token tile and head.  src, dst 16-byte aligned. */
int dh_transpose_frag_bf16(const dh_bf16* src, dh_bf16* dst, const int32_t* pad_tok, int heads, int hs,
                           int n_pad, void* stream);
/* Causal GQA attention backward (no KV cache; ger/model.py:287-289 under autograd): dq [n_tok,H,hs],
 * dk / dv [n_tok,G,hs] from q, k, v (rotated, plain), dout, lse (dh_attn_prefill_bf16) and
 * dsum = rowsum(dout*out); qT / doT / kT from dh_transpose_pad_bf16 / dh_transpose_frag_bf16 (those dh_attn_bwd_transposes names). */
/* Which transposed copies dh_attn_bwd_bf16 reads for a shape (round 4, ABI 6): bit 0 = qT and doT, bit 1 = kT; the others may be null.
 * (hs 64: the dk/dv kernel stages q / dO tiles in LDS and reads them transposed there — ds_read_b64_tr_b16 — so only kT is needed.) */
int dh_attn_bwd_transposes(int n_head, int n_groups, int hs, int n_pad);
int dh_attn_bwd_bf16(const dh_bf16* q, const dh_bf16* k, const dh_bf16* v, const dh_bf16* dout,
                     const dh_bf16* qT, const dh_bf16* doT, const dh_bf16* kT, const float* lse,
                     const float* dsum, const int32_t* q_start, const int32_t* q_len,
                     const int32_t* pad_start, dh_bf16* dq, dh_bf16* dk, dh_bf16* dv, int n_seq,
                     int max_q_len, int n_head, int n_groups, int hs, int n_pad, void* stream);

/* ------------------------------------------------------------------ token sampling */

/* Token-level cross entropy, ignore_index = -1 — ger/utils.py:424-463 (F.cross_entropy on the
 * autocast-upcast logits): loss[r] = logsumexp(logits[r,:]) - logits[r,target[r]] in fp32, 0 for
 * ignored rows (target outside [0, vocab)); lse[r] is kept for the backward.  logits: [rows, vocab]
 * bf16 (is_f32 = 0) or fp32 (is_f32 = 1).  The caller picks the normalisation (quirk Q5: chunked
 * variants divide by ALL rows, chunk_size = 0 by the valid rows). */
int dh_cross_entropy_fwd(const void* logits, int is_f32, const int64_t* targets, float* loss,
                         float* lse, int rows, int vocab, void* stream);
/* dlogits[r,c] = grad_row[r] * (softmax(logits[r,:])[c] - [c == target[r]]), 0 for ignored rows;
 * same dtype as logits. */
int dh_cross_entropy_bwd(const void* logits, int is_f32, const int64_t* targets, const float* lse,
                         const float* grad_row, void* dlogits, int rows, int vocab, void* stream);

/* RelPrompt reliability predictor — ger/relprompt.py:126-147 (NoiseMaskClassifier).  The two k=3 convolutions
 * are dh_linear_bf16 over the matrix built here: out [B*T, ld] with out[b,t, dk*C + c] = x[b, t+dk-1, c]
 * (zero outside the sequence, through ReLU if relu != 0), a column of ones at 3C (the bias rides the fp32
 * accumulation as the weight's column 3C) and zero padding up to ld (multiple of 64 for the GEMM). */
int dh_im2col3_bf16(const dh_bf16* x, dh_bf16* out, int B, int T, int C, int ld, int relu, void* stream);
/* ReLU -> AvgPool1d(pool, stride pool, ceil_mode: a short last window averages its own elements) ->
 * Linear(H -> 3): h [B,T,H] pre-activation, w [3,H], bias [3], out [B, ceil(T/pool), 3]. */
int dh_pool_head_bf16(const dh_bf16* h, const dh_bf16* w, const dh_bf16* bias, dh_bf16* out, int B, int T,
                      int H, int pool, void* stream);
/* Training of the reliability predictors — finetune/relprompt.py:356-387 (the mask cross entropy back-propagates
 * into conv1 / conv2 / classifier; ger/relprompt.py:79-119 keeps them trainable).
 * dh_pool_head_bwd_bf16: backward of ReLU -> AvgPool1d(pool, ceil) -> Linear(H, 3): dlogits fp32 [B, P, 3] ->
 *   dh bf16 [B,T,H] (gradient of the PRE-activation h) and pooled bf16 [B*P, H] (the Linear's input, recomputed
 *   exactly as dh_pool_head_bf16 forms it; the caller contracts it with dlogits for the Linear's weight gradient).
 * dh_col2im3_bf16: backward of dh_im2col3_bf16 fused with what precedes it: dx[b,t,c] = [pre[b,t,c] > 0] *
 *   mask[b,t,c] * sum_dk dcol[b, t+1-dk, dk*C + c]; pre (ReLU input) and mask (scaled dropout mask) may be NULL. */
int dh_pool_head_bwd_bf16(const dh_bf16* h, const dh_bf16* w, const float* dlogits, dh_bf16* dh, dh_bf16* pooled,
                          int B, int T, int H, int pool, void* stream);
int dh_col2im3_bf16(const dh_bf16* dcol, const dh_bf16* pre, const dh_bf16* mask, dh_bf16* dx, int B, int T, int C,
                    int ld, void* stream);

/* One decode-loop tail per sequence — generate/base.py:62-80:
 *   l = logits/temperature (bf16) ; keep l >= k-th largest ; softmax ; multinomial.
 * top_k == 1 is resolved as arg-max with the LOWEST index among equal maxima (the reference
 * breaks bf16 ties with the torch RNG, quirk Q6).  top_k == 0 means no cropping; entries equal
 * to the k-th largest are all kept, and -0 == +0 there as in the reference's `l < kth`.
 * For top_k != 1 the draw is the inverse CDF, in ascending token order, of the fp32 softmax over
 * the kept entries at the uniform
 *   u = (mix64(seed ^ mix64(((uint64_t)step << 32) | (uint32_t)seq)) >> 40) / 2^24      in [0, 1)
 *   mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)   (splitmix64, mod 2^64;
 *             mix64(0) == 0xE220A8397B1DCDAF)
 * with seq the row of `logits`.  The stream is part of the contract: seeded ids stay the same
 * across versions (tests/sampling_reference.py is the host model).  NaN logits are not supported.
 *   tokens [n_seq, tok_ld] int64 : token buffer per sequence (prompt + generated)
 *   length [n_seq] int32         : tokens currently valid; the new id goes to
 *                                  tokens[i, length[i]] and length[i] is incremented
 *   done   [n_seq] int32         : set to 1 when the new id == eos_id (eos_id < 0: never);
 *                                  finished sequences are left untouched.
 * No host synchronisation: the reference's per-token `if idx_next == eos_id`
 * (generate/base.py:79) becomes the device-side flag. */
int dh_sample_bf16(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                   int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                   uint64_t seed, int step, void* stream);

/* dh_sample_bf16 over a row list (continuous batching, dualhyp_amd/generate.py: generate_stream): logits row r
 * belongs to sequence u = row_seq[r] (device int32 [n_rows]) of per-sequence arrays that hold all n_seq sequences
 * of a call: tokens [n_seq, tok_ld], length / done / limit [n_seq].  limit[u] = prompt length + max_new_tokens is
 * the sequence's own budget: done[u] = 1 on eos_id, 2 once length[u] reaches limit[u]; rows whose sequence has
 * done != 0 return at once (several padding rows may name one finished sequence).  The top_k != 1 draw is keyed
 * by (seed, tokens generated so far = length[u] - (limit[u] - max_new_tokens), u): for the sequences of one call
 * that is dh_sample_bf16's (seed, step, row) when all of them start together, so ids do not depend on the schedule. */
int dh_sample_rows_bf16(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                        int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                        int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                        void* stream);

/* Token log-probabilities.  ONE definition for every entry below: under a logits row l (bf16, vocab columns, what the sampler reads)
 *   lp(t) = l[t] - m - log(sum_i exp(l[i] - m)),  m = max_i l[i]
 * of the RAW row — temperature 1, no top-k crop, whatever the call samples with: the model's distribution, not the sampler's.  The
 * bf16 values are widened to fp32, the sum and the result are fp32 (expf / logf, not the fast intrinsics).  -inf entries add 0, a
 * -inf token gives -inf, NaN logits are not supported.  One 1024-thread block per row; thread t adds the 8-element chunks t,
 * t + 1024, .. of the row in index order, the 1024 chains are added by a fixed butterfly: the order is a function of vocab alone, so
 * equal row contents give equal bits at any row index, row count or address.  |lp - exact| <= 2e-5 + 2.4e-7 |lp| up to vocab 128256. */

/* out[r] (fp32, [n_rows]) = lp(ids[r]) under logits row r.  ids: device int64 [n_rows]; an id outside [0, vocab) reads nothing and
 * gives NaN (the caller checks its ids: dualhyp_amd.ops.token_logprobs raises). */
int dh_token_logprobs_bf16(const dh_bf16* logits, int vocab, const int64_t* ids, float* out, int n_rows, void* stream);
/* dh_sample_bf16 / dh_sample_rows_bf16 with logprobs (nullable; fp32 [n_seq, tok_ld], the shape of `tokens`): the thread that stores
 * tokens[u, n] also stores logprobs[u, n] = lp(that token) under the row it was picked from; nothing is written where no token is
 * appended (finished sequence, budget, buffer full).  Null: the old entries, which call these with null — the kernels they always ran. */
int dh_sample_bf16_ex(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                      int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                      uint64_t seed, int step, void* stream, float* logprobs);
int dh_sample_rows_bf16_ex(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                           int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                           int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                           void* stream, float* logprobs);

/* Token alternatives.  ONE definition for every entry below: for a logits row l (bf16, vocab columns) and 1 <= K <= min(8, vocab)
 * (DH_MAX_TOP_LOGPROBS), alternative j = 0 .. K-1 is
 *   id_j = the index at rank j when the entries of l are ordered by value descending, then by index ascending,
 *   lp_j = lp(id_j) of "Token log-probabilities" above: (l[id_j] - m) - logf(tot) with the row's one m and one tot, summed in the
 *          same order, so lp_j is bit-equal to what dh_token_logprobs_bf16 gives for (l, id_j).
 * Values compare as numbers: -0 == +0, so two zeros tie and the lower index goes first; -inf entries are ordinary values that rank
 * last (lp = -inf).  The order is over the RAW row — temperature 1, no top-k crop: the model's distribution, not the sampler's
 * bf16(l / temperature), which can merge distinct raw values into ties.  Rows that hold a NaN are outside the definition (their
 * log-sum is NaN already); their ids are still inside [0, vocab).  A row's result depends on its bytes and on vocab alone: not on
 * the row index, the row count, the row's alignment or the sampler's parameters.  The selection is one more pass over the row in
 * the block that holds it: every entry has the unique sort key (value key, ~index), each thread keeps its 8 largest, and K
 * block-wide maxima merge them — no atomic decides anything.  m and tot are computed once per row for the chosen token and the K
 * alternatives. */
#define DH_MAX_TOP_LOGPROBS 8

/* out_ids (int32) / out_lp (fp32), both [n_rows, k]: the k alternatives of every logits row. */
int dh_token_top_logprobs_bf16(const dh_bf16* logits, int vocab, int k, int32_t* out_ids, float* out_lp, int n_rows, void* stream);
/* dh_sample_bf16_ex / dh_sample_rows_bf16_ex with the alternatives' buffers top_ids (int32) and top_lp (fp32), both
 * [n_seq, tok_ld, top_logprobs]: the thread that stores tokens[u, n] also stores top_ids[u, n, 0..K) and top_lp[u, n, 0..K), the
 * alternatives of the row the token was picked from; nothing is written where no token is.  top_logprobs = 0 (the buffers may then
 * be null) is the _ex entry; top_logprobs > 0 needs logprobs, top_ids and top_lp. */
int dh_sample_bf16_top(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                       int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                       uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp);
int dh_sample_rows_bf16_top(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                            int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                            int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                            void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp);

/* Beam search.  ONE definition for the entries below; tests/beam_reference.py is its host model.
 * An utterance holds up to W live beams, 1 <= W <= DH_MAX_BEAMS (2 W <= DH_MAX_TOP_LOGPROBS), each with a cumulative score cum
 * (fp32).  A step takes one raw bf16 logits row per live beam; step 0 has ONE live beam, the prompt's last-position row, cum = 0.
 *   Candidates of row b: its 2 W alternatives of "Token alternatives" above — ids in that order (value descending, then index
 *     ascending), lp bit-equal to dh_token_logprobs_bf16.  Candidate (b, j) has score = cum[b] + lp_j, one fp32 add.  Rows are
 *     finite: NaN / -inf logits are outside the definition (ids still stay inside [0, vocab)); vocab >= 2 W.
 *   Order: by score descending, then beam b ascending, then rank j ascending.  Within a row the score does not increase with j, so
 *     the best 2 W of all W * vocab continuations are among these W * 2 W candidates.
 *   Walk the first 2 W candidates in that order, p = 0, 1, .. being the place in the walk:
 *     token == eos_id and p < W:  (step, parent b, score, lp_j) is appended to the utterance's finished pool if it holds fewer than W;
 *     token == eos_id and p >= W: dropped;
 *     any other token: the next live beam, in walk order — (parent b, token, lp_j, cum' = score) is recorded;
 *     stop once W live beams are chosen (a row holds eos_id once, so at most W of the 2 W candidates are EOS).
 *   End: done = 1 when the pool holds W entries; else done = 2 after the step that appends generated token number max_new_tokens.
 *     The step that ends an utterance still records its W live beams.  eos_id < 0: never finished early.  An utterance with
 *     done != 0 is left alone: its state and records are frozen.
 * Histories are never gathered on the device: the records below are per step, and the host backtracks through beam_parent
 * (dualhyp_amd/beam.py), completes a pool that holds fewer than W entries with the live beams in live order (marked unfinished)
 * and ranks the pool by sum_logprob / n ** length_penalty in Python floats, n = generated tokens with the EOS counted,
 * descending, stable on pool order.  No powf runs on the device.
 *
 * Beam histories (opt-in: dh_beam_select_bf16_hist, dh_engine_set_beam_history; without them every entry launches what it always
 * launched).  H(u, t, w) is the list of tokens that live beam w of utterance u has generated behind the selection of step t:
 *   H(u, t, w) = H(u, t - 1, beam_parent[u, t, w]) + [beam_tok[u, t, w]], H(u, -1, .) = [].  It holds t + 1 ids, never a prompt
 *   token, and equals the host's backtracking read through beam_tok.  Pool entries and frozen (done) utterances have no device
 *   history: nothing reads one.
 *   Storage: two int64 planes [2][n_utt * W][max_new_tokens]; plane t & 1 holds H(., t, .) behind step t.  A step reads plane
 *     (t - 1) & 1 and writes plane t & 1, so no launch reads what it writes and any parent map (swap, fan-out, identity) is right; the
 *     parity comes from the step the launch reads on the device, so a captured chain stays replayable.
 *   Ban: with ngram = N in 1 .. 8 the candidates of row (u, b) at step t >= 1 are the first 2 W ids, in the raw row's order (value
 *     descending, then index ascending), among the ids that mask row u allows (all ids without a mask) and that are not in the ban set
 *     of the no-repeat n-gram definition below for g = H(u, t - 1, b); each keeps the raw row's log-probability, bit-equal to dh_token_logprobs_bf16.
 *     If fewer than 2 W such ids exist the ban is ignored for that row at that step (the mask alone guarantees 2 W): the beam form of
 *     "the pick is never taken from an empty set".  Step 0 has an empty history and no ban.  Everything behind the candidates —
 *     score add, merge order, walk, pool — is unchanged: the candidates are, bit for bit, dh_token_top_logprobs_bf16_mask(...,
 *     rows_per_mask = 1) under a per-row mask with the banned bits cleared.  vocab <= 131072 (the sampler's LDS row).
 *   Stop sequences: a candidate (b, j) with id x ends its hypothesis into the pool — the EOS's place rule, score and pool order —
 *     when x is in the stop set, as without histories, or when H(u, t - 1, b) + [x] ends on one of the stop sequences (the stop
 *     definition below, m = t + 1: a match never reaches behind the hypothesis' first generated token, nor into another beam's
 *     text).  fin_tok receives x, x stays in the hypothesis' tokens, finish_reason is "stop"; the EOS wins where both hold.
 *   What stays refused under beam search, histories or not, are the penalties and a bias: a penalised or boosted value would have to rank the candidates and enter
 *     the scores, which this definition does not say. */
#define DH_MAX_BEAMS 4
/* Device arrays of one beam search call (n_utt utterances, W beams, max_new_tokens steps).  The caller zeroes cum, n_steps, done
 * and n_fin; the other arrays are written where something is recorded and nowhere else. */
typedef struct dh_beam_state {
    float* cum;             /* [n_utt, W]  cumulative score of the live beams */
    int32_t* n_steps;       /* [n_utt]     steps recorded so far = generated tokens of every live beam */
    int32_t* done;          /* [n_utt]     0 live, 1 pool full, 2 budget spent */
    int32_t* beam_tok;      /* [n_utt, max_new_tokens, W]  token of live beam w chosen at step t */
    int32_t* beam_parent;   /* [n_utt, max_new_tokens, W]  the live beam of step t - 1 it continues (0 at step 0) */
    float* beam_lp;         /* [n_utt, max_new_tokens, W]  that token's log-probability under its parent's row */
    float* beam_cum;        /* [n_utt, max_new_tokens, W]  the beam's cumulative score behind that token */
    int32_t* fin_step;      /* [n_utt, W]  pool: the step whose EOS finished the hypothesis, */
    int32_t* fin_parent;    /* [n_utt, W]        the live beam of step fin_step - 1 it ends, */
    float* fin_score;       /* [n_utt, W]        its score, the EOS included, */
    float* fin_lp;          /* [n_utt, W]        and the EOS's log-probability under the parent's row (score = cum[parent] + fin_lp) */
    int32_t* n_fin;         /* [n_utt]     entries in the pool */
} dh_beam_state;
/* One step of every utterance with done == 0.  logits: [n_utt * rows_per_utt, vocab], rows_per_utt = 1 (step 0: the one live beam
 * is beam 0) or W (row u * W + b is live beam b of utterance u).  step (0 .. max_new_tokens - 1) indexes the records; step_dev
 * non-null: read from the device instead (a captured graph stays replayable).  cand_ids (int32) / cand_lp (fp32), both
 * [n_utt * rows_per_utt, 2 W]: workspace, left holding the rows' candidates.  Two launches: dh_token_top_logprobs_bf16 over the
 * rows (the per-row part is exactly that entry), then one wave per utterance that merges at most 32 candidates and walks them —
 * no atomic decides anything. */
int dh_beam_select_bf16(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens, int64_t eos_id,
                        int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids, float* cand_lp, void* stream);

/* Token masks (constrained decoding).  ONE definition for every entry below.
 * A token mask is a device array of 32-bit words [n_seq, mask_ld], mask_ld >= ceil(vocab / 32): bit i & 31 of word i >> 5 of row u is
 * set when token i is allowed for sequence u.  Bits at or beyond vocab are ignored, whatever they hold.  A null mask means the
 * feature is off: the entries without `_mask`, and the kernels they always ran.  The mask is only read.
 *   The mask belongs to the sampler, as top_k and temperature do.  A disallowed column takes part in the pick as if its logit were
 *     bf16 -inf (0xFF80): it is never the arg-max (on ties the lowest ALLOWED index wins), it does not count toward the top_k
 *     threshold (the k largest among the allowed ids are kept), and it adds 0 to the sampler's softmax.  For any row with at least
 *     one allowed logit above -inf the picked id equals what the entry without a mask picks on a copy of the row with 0xFF80 in every
 *     disallowed column — for top_k 1, k and none, and for the same (seed, step, seq) draw.  A row whose allowed logits are all -inf
 *     is outside the definition, as NaN is: it still produces an id in [0, vocab) and writes nothing else.
 *   Log-probabilities stay the model's: logprobs[u, n] is lp(picked id) of "Token log-probabilities" under the RAW row, with the
 *     same m and the same sum, and top_ids / top_lp are the raw row's alternatives, allowed or not — scores still compare with
 *     dh_token_logprobs_bf16 and with unconstrained runs.
 *   Which mask row a kernel reads: dh_sample_* row u of the block's sequence; dh_sample_rows_* row row_seq[r]; a verify step
 *     (dh_engine_decode_spec) row u for all D + 1 positions of sequence u; beam search row u of the utterance for all W beams.
 *   Beam candidates under a mask: the 2 W candidates of a beam row are the first 2 W ALLOWED ids in the raw row's order (value
 *     descending, index ascending, -0 == +0), each with the raw row's log-probability, bit-equal to dh_token_logprobs_bf16 for the
 *     id.  Every utterance's row allows at least 2 W ids below vocab (the caller checks: dualhyp_amd.constrain.check_mask).  The
 *     merge, the walk, the pool and the re-parenting are unchanged. */

/* dh_sample_bf16_top / dh_sample_rows_bf16_top under a mask (non-null; mask_ld >= ceil(vocab / 32), refused before any launch). */
int dh_sample_bf16_mask(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                        int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                        uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                        const uint32_t* mask, int mask_ld);
int dh_sample_rows_bf16_mask(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                             int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                             int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                             void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                             const uint32_t* mask, int mask_ld);
/* dh_token_top_logprobs_bf16 over the allowed ids: out_ids[r, 0..k) are the first k ids that mask row r / rows_per_mask allows, in
 * the raw row's order; out_lp are their raw log-probabilities.  A row that allows fewer than k ids leaves id 0 behind them. */
int dh_token_top_logprobs_bf16_mask(const dh_bf16* logits, int vocab, int k, int32_t* out_ids, float* out_lp, int n_rows,
                                    const uint32_t* mask, int mask_ld, int rows_per_mask, void* stream);
/* dh_beam_select_bf16 with the candidates taken under mask [n_utt, mask_ld] (see "Beam candidates under a mask"). */
int dh_beam_select_bf16_mask(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens, int64_t eos_id,
                             int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids, float* cand_lp,
                             const uint32_t* mask, int mask_ld, void* stream);

/* No-repeat n-grams (no_repeat_ngram_size of the text-generation stacks; extends the decode loop of generate/base.py:62-80).  ONE
 * definition for every entry below.
 * For a sequence, g[0 .. m) are the tokens it has GENERATED so far: tokens[u, start[u] .. length[u]), start[u] its prompt length.  The
 * prompt is excluded on purpose: a correction copies its prompt, so the prompt's n-grams stay free.  For n = ngram in 1 .. 8 the ban
 * set of the step is
 *     { g[i + n - 1] : 0 <= i <= m - n,  g[i .. i + n - 1) == g[m - n + 1 .. m) },
 * every token that would complete an n-gram the generated text already holds.  It is empty while m < n (the first pick of a prompt,
 * m = 0, is never affected); for n = 1 it is every id generated so far.  ngram = 0 means the feature is off: the entries without
 * `_ngram`, and the kernels they always ran.
 *   The ban belongs to the sampler, exactly as the mask does: the picked id is, bit for bit, what the entry without mask and ban
 *     picks on a copy of the row with 0xFF80 in every column that the token mask (if any) disallows or the ban set holds — for the
 *     arg-max, the top_k threshold and the softmax draw alike, and for the same (seed, step, seq) draw.
 *   One fallback: when every id the step would otherwise allow (the mask row's ids below vocab; every id without a mask) is banned,
 *     the ban set is ignored at that step.  The pick is never taken from an empty set.
 *   Log-probabilities and top_ids / top_lp stay the RAW row's, as under a mask.
 *   Where it is computed: inside the sampling kernel, by the sequence's own 1024-thread block, from the token buffer — no launch and
 *     no read-back of its own.  The allowed-minus-banned bits of the row live in a static LDS row of 131072 ids (16 KB); a larger
 *     vocab is refused.  A verify step's position j sees the picks the same launch appended before it. */

/* dh_sample_bf16_mask / dh_sample_rows_bf16_mask with ngram in 1 .. 8 (generate/base.py:62-80).  mask: nullable here (null: every
 * id is allowed, mask_ld is ignored).  start: int32 [n_seq], the prompt lengths; dh_sample_rows_bf16_ngram takes null for
 * limit[u] - max_new_tokens, which is the same number. */
int dh_sample_bf16_ngram(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                         int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                         uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                         const uint32_t* mask, int mask_ld, int ngram, const int32_t* start);
int dh_sample_rows_bf16_ngram(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                              int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                              int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                              void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                              const uint32_t* mask, int mask_ld, int ngram, const int32_t* start);

/* Stop conditions (the "stop" of the serving interfaces; extends the decode loop of generate/base.py:62-80).  ONE definition for every
 * entry below.
 * A stop specification (dh_stop_spec) of a call holds
 *   a stop SET: one row of ceil(vocab / 32) words in the token masks' bit layout — bit i & 31 of word i >> 5 is set when id i stops
 *     a sequence — shared by all sequences of the call, and
 *   up to DH_MAX_STOP_SEQS stop SEQUENCES of 2 .. DH_MAX_STOP_LEN ids each: int32 [n_seqs, DH_MAX_STOP_LEN] on the device, row i's
 *     first h_seq_len[i] entries, and the lengths on the HOST (they are checked before a launch and travel in the kernel arguments).
 *     A sequence of one id belongs in the set.
 * For a sequence, g[0 .. m) are the tokens it has GENERATED: tokens[u, start[u] .. length[u]), start[u] its prompt length.  The prompt
 * is excluded, as for no-repeat n-grams: a DualHyp prompt is full of newlines and "###".  After a pick t has been appended, so that
 * g[m - 1] = t, the stop condition holds when t is in the stop set, or when g[m - L .. m) == s for some stop sequence s of length
 * L <= m (a match never reaches back into the prompt).
 *   The end states, in this order: t == eos_id gives done = DH_DONE_EOS; otherwise the stop condition gives done = DH_DONE_STOP, also
 *     when that token took the last place of the budget or the buffer; otherwise the budget or buffer rule gives DH_DONE_LENGTH.
 *   The stopping token is an ordinary produced token: appended, with its log-probability and alternatives beside it, and left in the
 *     result (only the EOS is cut, quirk Q7).  The test is on the picked id, after mask and ban, and never changes a pick: a stopped
 *     call's tokens, log-probabilities and alternatives are, bit for bit, the unstopped call's up to and including the first place at
 *     which the condition holds, and nothing comes behind it.
 *   A null specification (a null pointer, or set == null and n_seqs == 0) is off: the entries, launches and bits without it.
 *   Where it is computed: in the tail of the sampling kernels, a few loads behind the pick; the branch is uniform per launch.  A verify
 *     step keeps the last DH_MAX_STOP_LEN generated tokens in registers, so a pick that stops ends the step where an EOS would.
 *   Beam search takes the stop set only: a candidate whose id is in the set ends its hypothesis into the pool exactly as the EOS does
 *     (place rule, score, pool order), and fin_tok[u, k] receives the id that ended pool entry k.  Stop sequences are refused there:
 *     the beams' histories live on the host — unless the caller keeps them on the device ("Beam histories" of "Beam search":
 *     dh_beam_select_bf16_hist, dh_engine_set_beam_history), where a sequence ends the hypothesis whose own text completes it. */
#define DH_MAX_STOP_SEQS 8
#define DH_MAX_STOP_LEN 8
/* the values of `done` (0: live) */
#define DH_DONE_EOS 1
#define DH_DONE_LENGTH 2
#define DH_DONE_STOP 3
typedef struct dh_stop_spec {
    const uint32_t* set;        /* device, ceil(vocab / 32) words; null: no stop ids */
    const int32_t* seqs;        /* device, [n_seqs, DH_MAX_STOP_LEN] */
    const int32_t* h_seq_len;   /* host, [n_seqs], each 2 .. DH_MAX_STOP_LEN */
    int n_seqs;                 /* 0 .. DH_MAX_STOP_SEQS */
} dh_stop_spec;

/* dh_sample_bf16_ngram / dh_sample_rows_bf16_ngram with a stop specification; here mask is nullable and ngram may be 0, so with
 * stop == null each is the entry it extends.  start: the prompt lengths, shared with ngram; stop sequences need it
 * (dh_sample_rows_bf16_stop takes null for limit[u] - max_new_tokens).  Refused without a launch: more than DH_MAX_STOP_SEQS
 * sequences, a length outside 2 .. DH_MAX_STOP_LEN, sequences where no start can be had. */
int dh_sample_bf16_stop(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                        int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                        uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                        const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop);
int dh_sample_rows_bf16_stop(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                             int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                             int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                             void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                             const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop);
/* dh_beam_select_bf16_mask (mask nullable) with the stop set of `stop`; fin_tok: int32 [n_utt, W] beside st->fin_step, needed with a
 * set.  stop == null: dh_beam_select_bf16 / dh_beam_select_bf16_mask.  A specification with sequences is refused. */
int dh_beam_select_bf16_stop(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens, int64_t eos_id,
                             int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids, float* cand_lp,
                             const uint32_t* mask, int mask_ld, const dh_stop_spec* stop, int32_t* fin_tok, void* stream);
/* The history planes of a beam search call ("Beam histories" of "Beam search"): tokens, device int64 [2][n_utt * W][max_new_tokens],
 * needs no initialisation; ngram 0 (no ban) .. 8. */
typedef struct dh_beam_hist {
    int64_t* tokens;
    int ngram;
} dh_beam_hist;
/* dh_beam_select_bf16_stop (mask, stop and fin_tok nullable as there) over device histories: the step reads plane (step - 1) & 1 of
 * hist->tokens and writes plane step & 1, its candidates are taken under the ban of hist->ngram, and `stop` may carry sequences
 * (fin_tok is needed with a set or with sequences).  hist == null: dh_beam_select_bf16_stop's launches, and sequences are refused.
 * Refused before any launch, with the value in the message: ngram outside 0 .. 8; vocab above 131072 with ngram > 0; null tokens with
 * ngram > 0 or with sequences. */
int dh_beam_select_bf16_hist(const dh_bf16* logits, int vocab, int n_utt, int rows_per_utt, int W, int max_new_tokens, int64_t eos_id,
                             int step, const int32_t* step_dev, const dh_beam_state* st, int32_t* cand_ids, float* cand_lp,
                             const uint32_t* mask, int mask_ld, const dh_stop_spec* stop, int32_t* fin_tok, const dh_beam_hist* hist,
                             void* stream);

/* Nucleus and min-p (the "top_p" and "min_p" of the serving interfaces; the sampler of generate/base.py:62-80 has temperature and top_k
 * only).  ONE definition for every entry below.
 * The row is the one the sampler already draws from: l_i = bf16(logit_i / temperature), bf16 -inf where the token mask disallows or the
 * n-gram ban bans; -0 == +0; m = max l; w_i = exp(l_i - m).  K0 is the set top_k keeps: ties at the k-th value are all kept, top_k = 0
 * keeps all.
 *   min_p in [0, 1], 0 = off: i is kept iff fl32(l_i - m) >= lmin, lmin = (float)log((double)min_p) computed once on the host inside the
 *     C entry; the subtraction is one fp32 IEEE subtraction and the comparison is >=, so min_p = 1 keeps exactly the entries equal to
 *     the maximum.  The test is relative to the best token: it depends on no normalisation.
 *   top_p in (0, 1], 1 = off; the value used is the fp32 one passed.  For a value v among the entries of K0, A(v) is the mass (sum of w)
 *     of the entries of K0 strictly above v and T the mass of K0: v is kept iff A(v) < top_p * T.  So the best value is always kept, and
 *     the value whose mass crosses top_p is kept WHOLE: ties stay together.  This differs from the text-generation stacks, which sort
 *     and cut by position, so that of two equal logits at the crossing one may stay and one may go.
 *   Kept set = K0 n nucleus of K0 n min_p.  Every part is a threshold on the value, so the kept set is again one threshold: the
 *     existing crop and the existing CDF walk (ascending index, slab per thread, the same fp32 sums) draw from it.
 *   Equivalence: for the same (seed, step, seq) the pick equals, bit for bit, what dh_sample_bf16_mask picks with top_k off under a mask
 *     that allows exactly the kept set (a masked entry adds 0.f to the same sums).
 *   top_k == 1, the arg-max: both parameters are accepted and do nothing (the arg-max is always kept).  Verify steps and beam search
 *     take neither.  Log-probabilities and alternatives stay the raw row's, as under a mask.
 *   Determinism: a row's kept set is a function of the row's bytes, vocab and the parameters; not of the row index, the row count, the
 *     alignment (the 16-byte and the scalar paths agree) or timing.  The kernel adds the masses as fixed-point integers
 *     (uint64)(w_i * 2^40) with integer atomics, exact in any order; no floating-point atomic feeds the threshold (sampling.hip).
 *   The device's exp is not the host's to the last bit, so the kept set is decided only where no A(v) / T lies within a band of
 *     2^-18 + 2^-22 of top_p (tests/nucleus_reference.py derives it); inside the band either neighbour is a correct answer.  NaN rows and
 *     rows whose allowed logits are all -inf stay outside the definition, as they are for the sampler; they still give an id in
 *     [0, vocab). */

/* dh_sample_bf16_stop / dh_sample_rows_bf16_stop with top_p and min_p; mask, ngram and stop stay nullable / 0, so with top_p = 1 and
 * min_p = 0 each is the entry it extends.  Refused without a launch, with the value in the message: top_p outside (0, 1] or NaN, min_p
 * outside [0, 1] or NaN. */
int dh_sample_bf16_nucleus(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                           int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                           uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                           const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                           float top_p, float min_p);
int dh_sample_rows_bf16_nucleus(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                float top_p, float min_p);

/* Penalties (the "repetition_penalty" of the Hugging Face stacks, the "frequency_penalty" and "presence_penalty" of the OpenAI-style
 * servers): value controls that make a token less likely because the sequence has already produced it.  ONE definition for every entry
 * below.  The parameters are per call:
 *   repetition = theta, finite, in [1/8, 8]; 1 = off.
 *   frequency = alpha_f and presence = alpha_p, finite, in [-8, 8]; 0 = off.
 * All three off is the call it always was: nothing is set and the kernels are the ones without a penalty.
 * The history of sequence u at a pick is H = tokens[u, start[u] : length[u]], the tokens it has generated; the prompt is excluded, for the
 * reason no_repeat_ngram excludes it (a correction copies its prompt).  c_t is the number of times id t occurs in H.
 * The pick is, bit for bit, the existing pick — the same temperature, top_k, top_p, min_p, mask, n-gram ban, seed, step and row — on a
 * copy of the logits row in which every column t with c_t > 0 and 0 <= t < vocab holds a_t; every other column is unchanged:
 *   x   = fp32(row[t])                       (bf16 widened)
 *   y   = x < 0 ? fl32(x * theta) : fl32(x / theta)   (the HF rule; NaN and +-0 take the division; IEEE division)
 *   p   = fl32(alpha_f * (float)c_t)
 *   z   = fl32(fl32(y - p) - alpha_p)        (three separately rounded fp32 operations: no FMA contraction)
 *   a_t = bf16 round-to-nearest-even of z
 *   Temperature is applied afterwards, by the sampler's l = bf16(a / temperature): the double rounding is part of the definition.
 *   Masks and bans: a column the mask disallows or the n-gram ban removes is -inf whatever a_t is; the ban's "everything banned"
 *     fallback works on bits and is untouched.
 *   Log-probabilities and alternatives stay the raw row's, as under every other control.  Stop conditions never change a pick.
 *   The prefill's first pick has an empty history: it is the plain pick.
 *   Verify steps (a position's history would have to include the launch's own picks) and beam steps (a beam's history lives on the
 *     host) take no penalty: dh_engine_decode_spec and dh_engine_decode_beam refuse while penalties are set.
 *   The logits buffer is read only.  The sequence's block finds the distinct ids of H and their counts with integer LDS atomics (exact
 *     in any order), computes one a_t per distinct id, and every read of the row that feeds the pick takes an overridden column from
 *     LDS (sampling.hip).  The tables are static: a call whose history could pass DH_MAX_PENALTY_HISTORY tokens (tok_ld above it), or
 *     whose vocab is above 131072, is refused before anything is launched. */
#define DH_MAX_PENALTY_HISTORY 2048
typedef struct dh_penalty_args {
    float repetition;           /* theta: 1 = off */
    float frequency;            /* alpha_f: 0 = off */
    float presence;             /* alpha_p: 0 = off */
} dh_penalty_args;

/* dh_sample_bf16_nucleus / dh_sample_rows_bf16_nucleus with the penalties; mask, ngram, stop, top_p and min_p stay nullable / 0 / 1 / 0,
 * and `penalties` null or all off makes each the entry it extends.  `start` is needed when a penalty is on.  Refused without a launch,
 * with the value in the message: a parameter outside its range or NaN, a penalty without start, tok_ld above DH_MAX_PENALTY_HISTORY. */
int dh_sample_bf16_penalty(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                           int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                           uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                           const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                           float top_p, float min_p, const dh_penalty_args* penalties);
int dh_sample_rows_bf16_penalty(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                float top_p, float min_p, const dh_penalty_args* penalties);

/* Contextual biasing (the "hot words" of the speech stacks; with one-id entries the "logit_bias" of the text-generation servers): a list
 * of phrases whose continuations get a logit bonus while decoding.  ONE definition for every entry below.
 * The bias specification (dh_bias_spec) of a call is shared by all its sequences and holds 1 .. DH_MAX_BIAS_ENTRIES entries.  Entry e is
 *   len_e in 1 .. DH_MAX_BIAS_LEN token ids, each in [0, vocab), and one finite fp32 boost b_e of either sign: on the device an int32
 *   [n, DH_MAX_BIAS_LEN] table (row e's first len_e places count), the int32 lengths and the fp32 boosts; the host copies of the three are
 *   what the argument checks read.  A one-id entry is a plain logit bias.  Null or n = 0 is off: the call it always was.
 * Which ids are boosted at a pick: let g[0..m) = tokens[u, start[u] : length[u]] be what sequence u has generated; the prompt is excluded,
 *   as for no_repeat_ngram and the penalties (a correction copies its prompt, so the prompt neither starts nor continues a match).
 *   Entry e PROPOSES id ids_e[k] at depth k (0 <= k < len_e) when k <= m and g[m-k .. m) == ids_e[0 .. k).  Depth 0 always matches: the
 *   first id of every entry is always proposed.  A whole emitted phrase proposes nothing further (k < len_e); matching starts again
 *   from depth 0.  There is NO FAILURE ARC: a bonus that was given is not taken back when the phrase is abandoned, and the boost does not
 *   grow with the depth.
 *   The boost of id t is B_t, the maximum of b_e over all (e, k) that propose t.  A maximum is exact in any order: the sequence's block
 *   takes it with an integer atomic max on an order-preserving key of the float; no floating-point atomic and no order-dependent sum
 *   decides anything.
 * What the pick sees: the pick is, bit for bit, the existing pick (the arg-max and the seeded draw alike) on a copy of the logits row in
 *   which every column t with a boost holds bf16(y + B_t): one fp32 add, never contracted, then round to nearest even.  y is the fp32
 *   value the column held just in front of its final bf16 rounding: fp32(row[t]) when t is not in the penalised history (no penalty is
 *   on, or c_t = 0: an id that is boosted but never generated takes no penalty, not even the repetition rule at a count of 0), and the z
 *   of "Penalties" when it is.  The boost is applied before temperature, top_k, top_p and min_p.  A column the mask disallows or the
 *   n-gram ban removes stays -inf; a raw -inf stays -inf and a NaN a NaN.  Log-probabilities and alternatives stay the raw row's.  Stop
 *   conditions never change a pick.  The logits buffer is read only.
 *   Verify steps (a position's tail would have to include the launch's own picks) and beam steps (a beam's history lives on the host)
 *   take no bias: dh_engine_decode_spec and dh_engine_decode_beam refuse while one is set.
 * Refused before any launch, with the value in the message: vocab above 131072, more than DH_MAX_BIAS_ENTRIES entries, a length outside
 *   1 .. DH_MAX_BIAS_LEN, an id outside the vocabulary, a boost that is not finite, a bias without `start`, and, with a penalty on, tok_ld
 *   plus the number of ids in all entries above DH_MAX_PENALTY_HISTORY (the ids share the penalties' tables, which keep their size; a
 *   bias alone always fits, 256 x 8 = 2048). */
#define DH_MAX_BIAS_ENTRIES 256
#define DH_MAX_BIAS_LEN 8
typedef struct dh_bias_spec {
    const int32_t* ids;         /* device, [n, DH_MAX_BIAS_LEN] */
    const int32_t* len;         /* device, [n], each 1 .. DH_MAX_BIAS_LEN */
    const float* boost;         /* device, [n], finite */
    const int32_t* h_ids;       /* host copies of the three: what the checks read */
    const int32_t* h_len;
    const float* h_boost;
    int n;                      /* 0 (off) .. DH_MAX_BIAS_ENTRIES */
} dh_bias_spec;

/* dh_sample_bf16_penalty / dh_sample_rows_bf16_penalty with the bias; everything else stays nullable / 0 / 1 / 0, and `bias` null or
 * without an entry makes each the entry it extends.  `start` is needed when a bias is given, by both. */
int dh_sample_bf16_bias(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                        int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                        uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                        const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                        float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias);
int dh_sample_rows_bf16_bias(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                             int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                             int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                             void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                             const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                             float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias);

/* Automaton constraints (the general form of a token mask: the allowed set changes with every token): one deterministic finite automaton
 * per sequence, walked on the device inside the sampling kernels.  ONE definition for every entry below.
 * The automaton set (dh_automaton_spec) of a call has S states, numbered globally over all of the call's automata, in CSR form:
 *   edge_off int32 [S + 1], edge_tok int32 [E], edge_dst int32 [E], init int32 [n_seq] (each sequence's start state) and state int32
 *   [n_seq], which lives on the device, is written by the kernels and is never initialised by the caller.  Inside a state the edge tokens
 *   are strictly ascending, so the automaton is deterministic and an edge is unique per (state, token); edge_dst lies in [0, S).  "This
 *   state may end the text" is an ordinary edge whose token is the call's eos_id; its destination is ignored.  Null is off: the call it
 *   always was.
 * State at a pick: m = length[u] - start[u] is the number of tokens sequence u has generated (start: the prompt lengths the other history
 *   readers take); q = m == 0 ? init[u] : state[u].  So the prefill's first pick and a refilled row need no reset launch.
 * Allowed row:
 *   1. R0 = the bits edge_tok[e], e in [edge_off[q], edge_off[q + 1]).
 *   2. With a token mask, R0 is ANDed with the sequence's mask row.  Bits at or behind vocab are clear.
 *   3. If R0 holds no bit, R0 = {eos_id} alone: a dead end, the sequence ends.  The mask is ignored here, so a pick is never taken from an
 *      empty set.
 *   4. no_repeat_ngram then bans on R0 by its own rule, its fallback included: a ban that would empty the row is ignored.
 *   5. The pick is, bit for bit, the masked pick ("Token masks") under that row: the arg-max, the threshold / nucleus / min-p passes, the
 *      CDF walk, and penalties and a bias through their override path.
 *   6. Log-probabilities and alternatives stay the raw row's.
 * Transition: for pick c, state[u] = edge_dst[e] of the edge of q with edge_tok[e] == c; without one (the dead-end EOS) state[u] = q.  A
 *   sequence that is done is left alone.  The sequence's block builds the row with integer LDS atomics, exact in any order, and one thread
 *   stores the new state behind the pick; the launch is the one the call made anyway.
 * Refused before any launch, with the value in the message: eos_id < 0 or >= vocab, vocab above 131072 (the LDS row's bound, as for the
 *   ban), a null `start`, offsets that are not monotone from 0 to E, a token outside [0, vocab) or not strictly ascending inside its state,
 *   an edge_dst or an init outside [0, S), and n_seq other than the call's sequences.  Verify steps (a position's state would depend on
 *   picks of the same launch) and beam steps (a re-parented beam would need its parent's state) take no automaton: dh_engine_decode_spec
 *   and dh_engine_decode_beam refuse while one is set. */
typedef struct dh_automaton_spec {
    const int32_t* edge_off;    /* device, [n_states + 1] */
    const int32_t* edge_tok;    /* device, [n_edges] */
    const int32_t* edge_dst;    /* device, [n_edges] */
    const int32_t* init;        /* device, [n_seq] */
    int32_t* state;             /* device, [n_seq]: the kernels' own */
    const int32_t* h_edge_off;  /* host copies of the first four: what the checks read */
    const int32_t* h_edge_tok;
    const int32_t* h_edge_dst;
    const int32_t* h_init;
    int n_states;
    int n_edges;
    int n_seq;
} dh_automaton_spec;

/* dh_sample_bf16_bias / dh_sample_rows_bf16_bias with the automaton set; everything else stays nullable / 0 / 1 / 0, and `automaton` null
 * makes each the entry it extends.  `start` and an eos_id in [0, vocab) are needed when one is given, by both. */
int dh_sample_bf16_automaton(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                             int32_t* done, int n_seq, float temperature, int top_k, int64_t eos_id,
                             uint64_t seed, int step, void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                             const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                             float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias,
                             const dh_automaton_spec* automaton);
int dh_sample_rows_bf16_automaton(const dh_bf16* logits, int vocab, int64_t* tokens, int tok_ld, int32_t* length,
                                  int32_t* done, const int32_t* limit, const int32_t* row_seq, int n_rows, int n_seq,
                                  int max_new_tokens, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                                  void* stream, float* logprobs, int top_logprobs, int32_t* top_ids, float* top_lp,
                                  const uint32_t* mask, int mask_ld, int ngram, const int32_t* start, const dh_stop_spec* stop,
                                  float top_p, float min_p, const dh_penalty_args* penalties, const dh_bias_spec* bias,
                                  const dh_automaton_spec* automaton);

/* ------------------------------------------------------------------ fp8 serving path (csrc/fp8.hip)
 * W8A8 with OCP e4m3fn: q = fp8_rne(v * (448 / amax)), scale = amax / 448 per row (amax >= 1e-12, fp32 arithmetic);
 * weights are quantised per output channel ahead of time (dualhyp_amd.quant, after merge_lora_weights), activations
 * per token by the two kernels below.  The CPU restatement is oracle/ger_oracle.py: quantize_rows_fp8 / linear_fp8. */

/* q[r,:] e4m3 [rows, K], scale[r] fp32 from bf16 rows.  K %% 8 == 0. */
int dh_quant_rows_fp8(const dh_bf16* x, uint8_t* q, float* scale, int rows, int K, void* stream);
/* dh_rmsnorm_bf16 (no residual) whose bf16 output row is quantised in registers; xn_out (nullable) receives the bf16 row. */
int dh_rmsnorm_quant_fp8(const dh_bf16* x, const dh_bf16* w, dh_bf16* xn_out, uint8_t* q, float* scale, int rows, int d,
                         float eps, const uint8_t* row_tail, void* stream);
/* y[M,N] bf16 = epilogue( bf16( (xq . wq^T in fp32) * (x_scale[m] * w_scale[n]) ) ) on the block-scaled fp8 MFMA
 * (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales).  K %% 128 == 0, N %% 4 == 0.  Epilogues: DH_EPI_PLAIN
 * (+ resid), DH_EPI_SWIGLU (w2q / w2_scale = fc_2), DH_EPI_ADAPTER (vec_a scale, vec_b bias).  M <= 128 streams the
 * weights once (decode), larger M runs 128 x 128 x 128 tiles. */
int dh_linear_fp8(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const float* w_scale, dh_bf16* y, int M, int N,
                  int K, int epilogue, const uint8_t* w2q, const float* w2_scale, const dh_bf16* vec_a, const dh_bf16* vec_b,
                  const dh_bf16* resid, void* stream);
/* dh_linear_fp8 with the kernel pinned: 0 = by row count (as above), 1 = tiled, 2 = streaming (M <= 128).  The two kernels
 * add the K products in different fp32 orders; the engine pins by PHASE (prefill tiled whatever the packing, single-token
 * steps streaming up to 128 rows) so that a sequence's bits do not depend on what is packed with it. */
int dh_linear_fp8_ex(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const float* w_scale, dh_bf16* y, int M, int N,
                     int K, int epilogue, const uint8_t* w2q, const float* w2_scale, const dh_bf16* vec_a, const dh_bf16* vec_b,
                     const dh_bf16* resid, int kernel, void* stream);

/* dh_linear_fp8 PLAIN (streaming kernel) for 1 <= M <= 128 with the bf16-rounded result written as fp32 [M, N]: the single "partial" the
 * fused decode-attention kernel (dh_attn_decode_fused_bf16, n_part = 1, no LoRA) consumes. */
int dh_linear_fp8_f32(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const float* w_scale, float* y32, int M,
                      int N, int K, void* stream);

/* ------------------------------------------------------------------ MXFP4 weights (csrc/mxfp4.hip)
 * A third weight format of the fp8 serving path: activations stay e4m3 rows with one fp32 scale per token (the two
 * quantisation kernels above); the weights are OCP MX v1.0 MXFP4.
 * Format.  A weight row W[n, :] (K % 128 == 0) is cut into blocks of 32 consecutive k.  Block b has one E8M0 byte s with
 * value 2^(s - 127) and 32 e2m1 elements: 4 bits each, bit 3 the sign, bits 2..1 the exponent, bit 0 the mantissa; codes
 * 0..7 are the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.
 * Quantiser (dualhyp_amd.quant.quantize_blocks_mxfp4; tests/mxfp4_reference.py is its fp64 restatement).  amax = max |block|.
 * amax == 0: s = 127, every element +0.  Otherwise e = floor(log2(amax)) - 2, clamped so that s = e + 127 lies in [1, 254];
 * element = v * 2^-e rounded to the nearest e2m1 value, ties to the even mantissa, saturated at +-6 (0.25 -> 0, 0.75 -> 1,
 * 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4, >= 6 -> 6); the sign bit is that of v unless the element rounds to zero,
 * which is always stored as +0 (code 0).  Inputs are the merged bf16 weights widened to fp32; every
 * step is exact or a single rounding.
 * Product.  y[m, n] = bf16( (sum_k xq[m, k] * e2m1[n, k] * 2^(s[n, k / 32] - 127)) * x_scale[m] ), fp32 accumulation, then the
 * epilogues and bf16 rounding points of dh_linear_fp8.  No channel scale: v_mfma_scale_f32_16x16x128_f8f6f4 applies the
 * block scales (operand format e2m1 on the W side, unit scale on the x side).  Every product is exact in fp32; each kernel
 * fixes one summation order per output, independent of the row count.
 * Physical layout (what wq / w_scale address; N % 16 == 0).  Rows are taken in groups of 16 and k in steps of 128.  For
 * group g = n / 16 and k-step t = k / 128 there is one block of 1024 nibble bytes at byte offset (g * (K / 128) + t) * 1024
 * of wq and one block of 64 scale bytes at byte offset (g * (K / 128) + t) * 64 of w_scale.  Inside a block, index
 * l = 16 * q + r (r = n % 16 the row of the group, q = (k % 128) / 32 the MX block of the k-step) selects 16 consecutive
 * nibble bytes at l * 16 and the scale byte at l.  Nibble byte j (0..15) of those 16 holds element k = 128 t + 32 q + 2 j in
 * its low four bits and element k + 1 in its high four bits.  The scale byte at l is s of row n, MX block 4 t + q.
 * So wq has N * K / 2 bytes and w_scale N * K / 32.  dualhyp_amd.quant.pack_mxfp4 writes this layout. */

/* dh_linear_fp8_ex with MXFP4 weights: wq / w2q the nibble bytes, w_scale / w2_scale the E8M0 bytes, both in the layout
 * above.  K % 128 == 0, N % 16 == 0.  Epilogues and the kernel selector (0 by row count, 1 tiled, 2 streaming with M <= 128)
 * as dh_linear_fp8_ex. */
int dh_linear_mxfp4_ex(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const uint8_t* w_scale, dh_bf16* y, int M,
                       int N, int K, int epilogue, const uint8_t* w2q, const uint8_t* w2_scale, const dh_bf16* vec_a,
                       const dh_bf16* vec_b, const dh_bf16* resid, int kernel, void* stream);
/* dh_linear_fp8_f32's counterpart: PLAIN on the streaming kernel, 1 <= M <= 128, the bf16-rounded result as fp32 [M, N]. */
int dh_linear_mxfp4_f32(const uint8_t* xq, const float* x_scale, const uint8_t* wq, const uint8_t* w_scale, float* y32, int M,
                        int N, int K, void* stream);

/* ------------------------------------------------------------------ MXFP6 activations (csrc/mxfp6.hip)
 * An opt-in activation format beside MXFP4 weights: the activations are OCP MX v1.0 MXFP6 (e2m3) instead of e4m3 rows, and
 * the e2m1 x e2m3 operand pair runs v_mfma_scale_f32_16x16x128_f8f6f4 at twice the rate of any pair with an e4m3 operand.
 * Element.  e2m3: six bits, bit 5 the sign, bits 4..3 the exponent E, bits 2..0 the mantissa m.  Magnitude m / 8 for E = 0,
 * else (1 + m / 8) * 2^(E - 1): 32 magnitudes 0 .. 7.5, strictly increasing in the low five bits.  No infinity, no NaN.
 * Block.  32 consecutive k of one activation row share one E8M0 byte s with value 2^(s - 127).  There is no per-token scale.
 * Quantiser (dualhyp_amd.quant.quantize_blocks_mxfp6; tests/mxfp6_reference.py is its fp64 restatement), for a bf16 row with
 * K % 128 == 0, every step exact in fp32, the exponent from the exponent field.  amax = max |x| over the block.  amax == 0:
 * s = 127, every code 0.  Otherwise e = floor(log2(amax)) - 2 clamped to [-126, 127], s = e + 127, a = |x| * 2^-e (bf16
 * subnormals are the values they are).  The magnitude is the grid value nearest to a, ties to the even code; an a above 7.5
 * saturates to 7.5 (reachable: an amax with mantissa above 1.875 would round to 8).  The sign bit is set only with a non-zero
 * magnitude code: -0 is never produced.  Non-finite inputs are outside the contract.
 * Product.  y[m, n] = epilogue( bf16( sum_k e2m3(xq[m, k]) * 2^(sx[m, k / 32] - 127) * e2m1(wq[n, k]) * 2^(sw[n, k / 32] - 127) ) ),
 * fp32 accumulation, then the epilogues and bf16 rounding points of dh_linear_mxfp4_ex without the multiply by x_scale[m].
 * The instruction applies both block scales; every product is exact in fp32; each kernel fixes one summation order per
 * output, independent of the row count (tiled: k ascending in one accumulator; streaming: each wave's k-steps ascending,
 * waves added in order).
 * Physical layout of a quantised activation matrix of M rows (what xq / x_scale address): fragment order, as the weights.
 * Rows are taken in groups of 16 and k in steps of 128; there are G = ceil(M / 16) groups, the last one complete in the
 * buffer whatever M is.  For group g = m / 16 and k-step t = k / 128 there is one block of 1536 code bytes at byte offset
 * (g * (K / 128) + t) * 1536 of xq and one block of 64 scale bytes at byte offset (g * (K / 128) + t) * 64 of x_scale.
 * Inside a block, index l = 16 * q + r (r = m % 16 the row of the group, q = (k % 128) / 32 the MX block of the k-step)
 * selects 24 code bytes and the scale byte at l.  The 24 bytes are the block's 32 codes as one little-endian 192-bit
 * number, element i = k % 32 in bits 6 i .. 6 i + 5 (byte j holds bits 8 j .. 8 j + 7); they are stored as three planes of
 * 512 bytes: bytes 8 p .. 8 p + 7 of the 24 are at p * 512 + l * 8 of the block, p = 0, 1, 2.  The scale byte at l is s of row
 * m, MX block 4 t + q.  So xq has G * 16 * K * 3 / 4 bytes and x_scale G * 16 * K / 32.  The bytes of rows >= M in the last
 * group are never written by the quantisers and never reach an output of a row < M.  dualhyp_amd.quant.pack_mxfp6 writes
 * this layout.  (The operand map behind it, found on the hardware by tools/mxfp6_probe.hip, is in csrc/mxfp6.hip.) */

/* dh_quant_rows_fp8's counterpart: bf16 rows [rows, K] -> codes q and scale bytes qscale in the layout above.  K % 128 == 0. */
int dh_quant_rows_mxfp6(const dh_bf16* x, uint8_t* q, uint8_t* qscale, int rows, int K, void* stream);
/* dh_rmsnorm_quant_fp8's counterpart: quantises, bit for bit, the bf16 row dh_rmsnorm_bf16 produces; xn_out (nullable)
 * receives that row.  d % 128 == 0, d <= 8192. */
int dh_rmsnorm_quant_mxfp6(const dh_bf16* x, const dh_bf16* w, dh_bf16* xn_out, uint8_t* q, uint8_t* qscale, int rows, int d,
                           float eps, const uint8_t* row_tail, void* stream);
/* dh_linear_mxfp4_ex with MXFP6 activations: xq / x_scale in the layout above, everything else (weights, K % 128 == 0,
 * N % 16 == 0, epilogues, kernel selector, refusals) as dh_linear_mxfp4_ex. */
int dh_linear_mxfp4a6_ex(const uint8_t* xq, const uint8_t* x_scale, const uint8_t* wq, const uint8_t* w_scale, dh_bf16* y, int M,
                         int N, int K, int epilogue, const uint8_t* w2q, const uint8_t* w2_scale, const dh_bf16* vec_a,
                         const dh_bf16* vec_b, const dh_bf16* resid, int kernel, void* stream);
/* dh_linear_mxfp4_f32's counterpart: PLAIN on the streaming kernel, 1 <= M <= 128, the bf16-rounded result as fp32 [M, N]. */
int dh_linear_mxfp4a6_f32(const uint8_t* xq, const uint8_t* x_scale, const uint8_t* wq, const uint8_t* w_scale, float* y32, int M,
                          int N, int K, void* stream);

/* ------------------------------------------------------------------ fp8 KV cache (csrc/kv8.hip, csrc/attention.hip)
 * Scheme.  Each KV group of each token has one K vector (after rope: the bf16 values dh_qkv_rope_cache_bf16 caches) and one V
 * vector of hs elements.  amax = max |x|; e = the smallest integer with amax <= 448 * 2^e (amax = m * 2^ex, m in [0.5, 1):
 * e = ex - 9 if m <= 0.875, else ex - 8; from the exponent and mantissa fields, no logarithm), clamped to [-100, 100], 0 when
 * amax == 0; byte = e4m3fn_rne(x * 2^-e), saturated to +-448, never the NaN encoding.  The dequantised value e4m3 * 2^e has
 * 4 significant bits and an exponent in range: it is exactly representable in bf16, so attention over this cache is, bit for
 * bit, the bf16 attention over its expansion.  Zero bytes with zero exponents are 0.0: the cache is zero-initialised like
 * the bf16 one.  The CPU restatement is tests/kv8_reference.py.
 * Layout.  k8 / v8: uint8, per (slot, group) a block of s_max * hs bytes in 32-key tiles of hs * 32 bytes; a tile is hs / 32
 * blocks of 1 KiB, lane i <- 16 B at i * 16, holding two MFMA A-operand fragments of 8 bytes per lane (csrc/common.h
 * k8_off / v8_off; dualhyp_amd.ops.kv8_unpack is the host index math).  k_exp / v_exp: int8 [max_batch, g, s_max].
 * hs 64, 96 or 128; s_max % 64 == 0. */

/* dh_qkv_rope_cache_bf16 with the cache writes replaced: q_out is bit for bit that op's, k (after rope) and v of every
 * token go to the fp8 cache at (tok_slot, tok_pos). */
int dh_qkv_rope_cache_kv8(const dh_bf16* qkv, const dh_bf16* cos, const dh_bf16* sin, const int32_t* tok_slot,
                          const int32_t* tok_pos, dh_bf16* q_out, uint8_t* k8, uint8_t* v8, int8_t* k_exp, int8_t* v_exp,
                          int n_tok, int n_head, int n_groups, int hs, int s_max, void* stream);
/* dh_attn_decode_bf16 reading the fp8 cache: fragments become bf16 in registers (exactly), same walk, same partials
 * (`work`: dh_attn_decode_work_bytes), same combine — bit for bit dh_attn_decode_bf16 over the dh_kv8_expand of the cache. */
int dh_attn_decode_kv8(const dh_bf16* q, const uint8_t* k8, const uint8_t* v8, const int8_t* k_exp, const int8_t* v_exp,
                       const int32_t* seq_slot, const int32_t* kv_len, dh_bf16* y, void* work, int n_seq, int n_head,
                       int n_groups, int hs, int s_max, void* stream);
/* Dequantises positions [0, n_i) of slot seq_slot[i], i < n_seq, into bf16 K / V^T buffers [max_batch, g, s_max, hs] /
 * [max_batch, g, hs, s_max] in the fragment layout of the bf16 cache (same slot).  n_i = kv_len[i] + kv_extra[i] (kv_extra
 * NULL: kv_len[i]; both NULL: s_max), at most s_max.  Whole 32-key tiles are written, positions >= n_i of the last one as
 * +0.0 (zero bits); tiles behind it are left alone. */
int dh_kv8_expand(const uint8_t* k8, const uint8_t* v8, const int8_t* k_exp, const int8_t* v_exp, const int32_t* seq_slot,
                  const int32_t* kv_len, const int32_t* kv_extra, dh_bf16* k_out, dh_bf16* vT_out, int n_seq, int n_groups,
                  int hs, int s_max, void* stream);

/* ------------------------------------------------------------------ decoder engine
 * Native runtime that owns the kernel sequence of ger/lora.py:504-549 for a whole batch:
 * embed -> n_layer x [norm_1, qkv(+LoRA), rope+cache, attention, proj(+LoRA)+residual,
 * norm_2, fc_1/fc_2+SwiGLU, proj+residual] -> ln_f -> lm_head, with the decode step captured
 * in a hipGraph.  Weights are NOT copied: the table holds device pointers owned by the caller
 * (the torch parameters of dualhyp_amd.GPT). */

typedef struct dh_layer_weights {
    const dh_bf16* norm_1;      /* [d]                                         */
    const dh_bf16* norm_2;      /* [d]                                         */
    const dh_bf16* attn_w;      /* [(n_head+2g)*hs, d]  attn.attn.linear.weight */
    const dh_bf16* attn_lora_a; /* [48, d]  rank padded to 16 per q/k/v; NULL = no LoRA */
    const dh_bf16* attn_lora_b; /* [(n_head+2g)*hs, 16]                        */
    const dh_bf16* proj_w;      /* [d, d]               attn.proj.linear.weight */
    const dh_bf16* proj_lora_a; /* [16, d] or NULL                             */
    const dh_bf16* proj_lora_b; /* [d, 16]                                     */
    const dh_bf16* fc_1;        /* [I, d]                                      */
    const dh_bf16* fc_2;        /* [I, d]                                      */
    const dh_bf16* mlp_proj;    /* [d, I]                                      */
    /* fp8 serving (BASELINE config 5; merged-LoRA path of ger/lora.py:152-157,349-365,707-711): when attn_ws is
     * non-NULL every *_ws must be, the five weight pointers above then address OCP e4m3 bytes [N, K] produced by
     * dualhyp_amd.quant (LoRA already merged: attn_lora_* / proj_lora_* NULL) and these are the fp32 scales per
     * output channel, [N] each. */
    const float* attn_ws;
    const float* proj_ws;
    const float* fc_1_ws;
    const float* fc_2_ws;
    const float* mlp_proj_ws;
} dh_layer_weights;

typedef struct dh_model_desc {
    int32_t n_layer, n_head, n_groups, head_size, n_embd, intermediate, vocab, block_size;
    float norm_eps;
    float lora_scale;           /* alpha / r */
    const dh_bf16* wte;         /* [vocab_rows, d] (vocab_rows >= vocab: RelPrompt adds rows) */
    int32_t wte_rows;
    const dh_bf16* ln_f;        /* [d] */
    const dh_bf16* rope_cos;    /* [block_size, head_size] bf16 tables of ger/model.py:319-346 as built by */
    const dh_bf16* rope_sin;    /*   GPT.build_rope_cache (base 10000, quirk Q1); made once by the host     */
    const dh_bf16* lm_head;     /* [vocab, d] */
    const dh_bf16* adapter_scale; /* [vocab] */
    const dh_bf16* adapter_bias;  /* [vocab] */
    const dh_layer_weights* h_layers; /* host array [n_layer] (copied) */
    const float* lm_head_ws;    /* fp8 serving: [vocab] channel scales, lm_head then addresses e4m3 bytes; else NULL */
} dh_model_desc;

typedef struct dh_engine dh_engine;

/* Allocates KV cache [n_layer][max_batch, g, s_max, hs] x2, activations for up to
 * max_tokens packed tokens and the decode-graph state.  head_size 64, 96 or 128 (every attention
 * entry point takes the same three; dh_linear_qkv_*rope_cache_bf16 only 64 and 128).  Fails before
 * allocating when the KV cache alone exceeds the device's free memory. */
int dh_engine_create(const dh_model_desc* h_desc, int max_batch, int s_max, int max_tokens,
                     dh_engine** h_out);
/* dh_engine_create with the KV cache's element type: kv_dtype 0 = bf16 (dh_engine_create itself), 1 = fp8 (the scheme and
 * layout of "fp8 KV cache" above).  kv_dtype 1 needs an fp8 engine (attn_ws != NULL).  It allocates, per layer, k8 / v8
 * [max_batch, g, s_max * hs] bytes and k_exp / v_exp [max_batch, g, s_max] int8, plus ONE layer's worth of bf16 K / V^T
 * [max_batch, g, s_max, hs] that every layer's prompt attention reuses: a prompt forward writes the fp8 cache
 * (dh_qkv_rope_cache_kv8), expands the call's sequences into that scratch (dh_kv8_expand) and runs dh_attn_prefill_bf16 on
 * it, so a prompt token attends to the values the decode steps (dh_attn_decode_kv8) will read; the <= 128-row fused decode
 * launch is not used.  With n = max_batch * g * s_max, dh_engine_device_bytes is smaller than the bf16 engine's of the same
 * capacity by n_layer * n * (2 hs - 2) - 4 * n * hs - 16 * n_layer bytes (the scratch, and 2 n_layer more pointers in the
 * table dh_engine_copy_prefix reads).  A kv_dtype 0 engine runs the launches of dh_engine_create's. */
int dh_engine_create_ex(const dh_model_desc* h_desc, int max_batch, int s_max, int max_tokens, int kv_dtype,
                        dh_engine** h_out);
/* dh_engine_create_ex with the block weights' format: weight_dtype 0 = as the descriptor says (bf16, or e4m3 with channel
 * scales when attn_ws != NULL: dh_engine_create_ex itself), 1 = MXFP4.  With weight_dtype 1 the five block weight pointers of
 * every dh_layer_weights address nibble bytes and the *_ws pointers (cast to const float*) address E8M0 bytes, both in the
 * layout of "MXFP4 weights" above; lm_head stays e4m3 with lm_head_ws channel scales.  Such an engine is an fp8 engine in
 * every other respect (layer sequence, activation buffers, the refusals of beam and verify steps, kv_dtype 1 allowed); it
 * needs n_embd and intermediate % 128 == 0 and merged LoRA. */
int dh_engine_create_q(const dh_model_desc* h_desc, int max_batch, int s_max, int max_tokens, int kv_dtype, int weight_dtype,
                       dh_engine** h_out);
/* dh_engine_create_q with the block activations' format: act_dtype 0 = e4m3 rows with one scale per token (dh_engine_create_q
 * itself), 1 = MXFP6 ("MXFP6 activations" above).  act_dtype 1 is accepted with weight_dtype 1 only: beside an e4m3 weight an
 * e2m3 activation runs the MFMA at the fp8 rate, and that pair is refused with this reason.  Such an engine runs the fp8 layer
 * sequence with its four quantisation points per block on dh_rmsnorm_quant_mxfp6 / dh_quant_rows_mxfp6 and its block linears
 * on dh_linear_mxfp4a6_ex / _f32 (the fp32-out QKV form in front of the fused decode attention included); the final norm,
 * lm_head and the adapter stay e4m3.  The phase-pinned kernel choice, the 128-row class boundary, kv_dtype 1 and every refusal
 * of an fp8 engine are dh_engine_create_q's.  The code and scale buffers hold max_tokens rounded up to 16 rows and are counted
 * in dh_engine_device_bytes. */
int dh_engine_create_qa(const dh_model_desc* h_desc, int max_batch, int s_max, int max_tokens, int kv_dtype, int weight_dtype,
                        int act_dtype, dh_engine** h_out);
void dh_engine_destroy(dh_engine* e);
int64_t dh_engine_device_bytes(const dh_engine* e);

/* Forward of a packed batch through the KV cache (ger/lora.py:504-549 with input_pos):
 *   h_seq_len[i] tokens for slot i (i < n_seq) starting at cache position h_pos0[i];
 *   ids: packed [sum(seq_len)] int64 on device.
 * logits_all != NULL : [n_tok, vocab] logits of every position (reference behaviour, Q9)
 * logits_last != NULL: [n_seq, vocab] logits of each sequence's last position only.  With logits_all == NULL (generate's
 *   prompt forward reads `logits[0, -1]`, generate/base.py:57-60) the last block's attention output, projection and MLP run on
 *   those n_seq rows alone — K and V of every token still go to the cache; the logits and the caches are bit-equal to the
 *   all-rows run (dh_set_tuning key 23; tests/test_hip_edges.py).  The hidden rows dh_engine_read(3) returns are then those
 *   of the last block's INPUT. */
int dh_engine_forward(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len,
                      const int32_t* h_pos0, int n_seq, dh_bf16* logits_all,
                      dh_bf16* logits_last, void* stream);
/* Same, with sequence i of the call living in KV-cache slot slot_base + i: several batches are
 * prefilled one after the other into one engine and then decoded together (dh_engine_decode over
 * all occupied slots; rows of a larger decode call equal the same rows decoded alone). */
int dh_engine_forward_at(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len,
                         const int32_t* h_pos0, int n_seq, int slot_base, dh_bf16* logits_all,
                         dh_bf16* logits_last, void* stream);
/* Same, with sequence i of the call living in KV-cache slot h_slot[i] (host array): distinct slots in
 * [0, max_batch), in any order — a prefill into whichever slots finished sequences have freed while the other
 * slots hold live ones.  The slot list goes to a device array of the call's own; h_slot[i] = base + i gives the
 * bits of dh_engine_forward_at(base), logits and caches.
 * prompt_phase: dh_engine_forward(_at) takes a call of one token per sequence for a decode step and runs the decode
 * kernels, so a one-token PROMPT forwarded alone and the same prompt packed with longer ones go through different
 * kernel families (different fp32 summation orders).  prompt_phase = 1 says the call is a prompt forward whatever
 * its lengths: prefill kernels, the bits the sequences have in any pack with a longer prompt.  0 = as forward_at. */
int dh_engine_forward_slots(dh_engine* e, const int64_t* ids, const int32_t* h_seq_len,
                            const int32_t* h_pos0, const int32_t* h_slot, int n_seq, int prompt_phase,
                            dh_bf16* logits_all, dh_bf16* logits_last, void* stream);

/* Fork a KV prefix: cache positions [0, n_pos) of slot src_slot, K and V^T of every layer and group, are copied
 * into each of the n_dst slots of h_dst_slots (host array) by one launch on `stream`.  Replaces the per-utterance
 * recomputation of inference/ger.py:60-83, where every prompt's instruction sentences and "### ... Best-hypothesis:"
 * header go through all layers again: K and V at a position depend on the tokens at or before it alone, and a
 * prefill row's bits do not depend on what it is packed with, so sequences that open with the same n_pos tokens
 * hold the same bits there.  Forward the shared tokens once into src_slot, fork them, then forward each
 * sequence's remaining tokens with h_pos0 = n_pos (dh_engine_forward_slots, prompt_phase = 1): caches and logits
 * equal those of the whole prompts' forward.
 * n_pos is a multiple of 32, the cache tile (the caches store 32-key tiles back to back from the start of a
 * (slot, group) block, so the copy is one contiguous run of n_pos * head_size elements per block at every head
 * size), 0 < n_pos <= s_max.  Slots are in [0, max_batch); the destinations are distinct and exclude src_slot.
 * Positions >= n_pos of the destinations and every other slot keep their contents.  The cache is bf16 in bf16
 * and fp8 engines alike, unless the engine was made with kv_dtype 1 (dh_engine_create_ex): then the fp8 bytes (runs of
 * n_pos * head_size bytes) and the exponents (n_pos bytes per block) are copied, by two launches.  n_dst = 0 is a no-op. */
int dh_engine_copy_prefix(dh_engine* e, int src_slot, const int32_t* h_dst_slots, int n_dst, int n_pos,
                          void* stream);

/* ---- Sampled candidates ----------------------------------------------------------------------------------------------------
 * N candidates per utterance from one prefill (dualhyp_amd/generate.py:sample_batch).  DEFINITION: sample j of utterance u is row
 * u * N + j of a dh_engine_decode run over the prompt list with every prompt repeated N times — the same ids, log-probabilities,
 * alternatives and done flags, bit for bit.  It holds by construction: the draw is keyed by (seed, step, row), the decode steps are
 * dh_engine_decode over n_utt * N rows, and a forked slot holds the bytes a prefill of its own would have written, because a
 * prefill row's bits do not depend on the rows beside it.  So utterance u is prefilled once, into slot u * N, and
 * dh_engine_fork_slots copies its prompt cache into the N - 1 slots behind.
 *
 * For every utterance u < n_utt the 32-key tiles 0 .. ceil(prompt_len[u] / 32) - 1 of slot u * n_copies — K and V^T of every layer
 * and group — are copied into slots u * n_copies + 1 .. u * n_copies + n_copies - 1, by ONE launch on `stream` over all utterances
 * (an engine made with kv_dtype 1: two launches, the fp8 bytes and then the exponents, as dh_engine_copy_prefix splits them).
 * d_prompt_len is a DEVICE array of n_utt int32 and is read by the kernel: the call makes no host synchronisation and no upload,
 * and it can be captured.  max_len, the host's maximum of the lengths (1 .. s_max), only sizes the grid: a length above it is the
 * caller's error and is copied as far as the grid reaches, a length < 1 copies nothing, and the tile count is clamped to the cache
 * on the device, so no length writes outside a slot's blocks.
 * n_copies is N, 2 .. DH_MAX_SAMPLES, and n_utt * n_copies <= max_batch.  Positions at or behind a prompt's end inside its last
 * tile carry the source's bytes (the decode steps overwrite them before causality lets anything read them); every tile behind,
 * the source slots and the slots at or above n_utt * n_copies keep their contents. */
#define DH_MAX_SAMPLES 8
int dh_engine_fork_slots(dh_engine* e, const int32_t* d_prompt_len, int n_utt, int n_copies, int max_len, void* stream);

/* Reproduce the rsqrt rounding of the reference's CPU path (see dh_rmsnorm_bf16 row_tail):
 * vec_width = lanes of torch's bf16 vector loop on the reference host (32 on AVX-512, 16 on
 * AVX2), 0 = off (every row uses bf16(1/sqrt(t)), as a GPU run of the reference would).
 * whole_call = 1: the tail is the last n_tok %% vec_width rows of the packed call (what
 * GPT.forward(idx[B,T]) does); 0: per sequence (B independent batch-1 calls, generate()).
 * Decode steps are single-token calls, i.e. always tail rows.  Default: off. */
int dh_engine_set_cpu_rsqrt_emulation(dh_engine* e, int vec_width, int whole_call);

/* The decode loop of generate/base.py:57-80 for n_seq sequences at once, entirely on device:
 * tokens [n_seq, tok_ld] holds the prompts (length[i] valid ids each, already prefilled
 * through position length[i]-2; the last prompt token's logits are `logits_last` of the
 * prefill and must have been sampled already, i.e. length includes the first new token).
 * Runs `n_steps` x { forward(one token/seq at position length-1) ; sample }.  Sequences with
 * done[i] != 0 keep stepping harmlessly but their tokens/length are frozen. */
int dh_engine_decode(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                     int n_seq, int n_steps, float temperature, int top_k, int64_t eos_id,
                     uint64_t seed, int first_step, void* stream);

/* dh_engine_decode over a ROW LIST: n_steps x { forward of n_rows rows ; dh_sample_rows_bf16 }.  Row r works on
 * sequence row_seq[r] (its row of tokens, its length / done / limit entry: arrays over all n_seq sequences of the
 * call, as in dh_sample_rows_bf16) in KV slot row_slot[r].  row_seq and row_slot are device int32 arrays that the
 * captured step reads when it runs: the caller rewrites their contents between calls (sequences retire, others
 * take their slots) and keeps their addresses, which are part of the graph key together with n_rows.  Layers,
 * kernel family and rounding are those of dh_engine_decode at n_rows rows.  A padding row names a sequence with
 * done != 0 and the slot that sequence owns (it recomputes that sequence's last position in place, as finished
 * rows of dh_engine_decode do); live rows name distinct slots. */
int dh_engine_decode_rows(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                          const int32_t* limit, int n_seq, int max_new_tokens, const int32_t* row_seq,
                          const int32_t* row_slot, int n_rows, int n_steps, float temperature, int top_k,
                          int64_t eos_id, uint64_t seed, void* stream);

/* Speculative greedy decoding: the loop of generate/base.py:57-80 with top_k = 1, n_draft + 1 positions of every
 * sequence per step.  A step feeds each sequence's last token and n_draft drafted tokens behind it (S = n_draft + 1
 * rows per sequence through the single-token-step kernels, one attention launch per layer over the S positions),
 * takes the arg-max of every row and appends pick_0 .. pick_a, a = the number of leading drafts j with
 * draft_j == pick_{j-1}: the ids are those of dh_engine_decode with top_k = 1, bit for bit, whatever the drafts
 * (a row's bits do not depend on the rows beside it, rejected positions of the cache are overwritten before
 * causality lets anything read them).
 * tokens / length / done as in dh_engine_decode; limit[i] = prompt length + max_new_tokens is sequence i's budget
 * (done = 2 when reached, as in dh_sample_rows_bf16; nothing is written at or behind it).
 * drafts (device, [n_seq, max_new_tokens], may be null): drafts[i, k] is proposed as the k-th generated token of
 * sequence i.  Null: prompt lookup on tokens[i, :length[i]] — the tokens behind the latest earlier occurrence of
 * the last 3, 2 or 1 tokens (dualhyp_amd/speculate.py:propose is the specification).
 * counters (device int32[3], zeroed by the caller): [0] steps until the last sequence finished (counted from
 * first_step), [1] drafts verified, [2] drafts appended.
 * Needs n_draft in 1..7, (n_draft + 1) * n_head / n_groups <= 32, n_seq * (n_draft + 1) <= 2048 rows reserved with
 * dh_engine_reserve_rows, a bf16 engine without the CPU rsqrt emulation, and positions up to length + n_draft - 1
 * in the cache (rows behind its end are computed and dropped). */
int dh_engine_decode_spec(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                          const int32_t* limit, int n_seq, int max_new_tokens, int n_draft, const int64_t* drafts,
                          int32_t* counters, int n_steps, float temperature, int64_t eos_id, int first_step,
                          void* stream);
/* Sampled verification: dh_engine_decode_spec whose positions DRAW where its positions take the arg-max, so that a sampled call
 * (any top_k, with top_p / min_p, the penalties, a bias and an automaton where they are set) can speculate.
 *   The key.  Position j of sequence u picks from logits row u * S + j exactly as the plain step picks a sequence's next token:
 *   temperature, top_k, the mask row u, and the draw keyed by (seed, step, seq) with step = n - prompt length, n the sequence's
 *   length at that position counting the picks this launch appended before it, prompt length = limit[u] - max_new_tokens, and
 *   seq = u.  That is the key dh_engine_decode uses for the token at place n (its step counter is the number of tokens generated so
 *   far, its row index the sequence), and dh_sample_rows_bf16's.
 *   The history.  The no-repeat ban, the penalties' counts and the bias' proposals of position j are formed from
 *   tokens[u, start[u] .. n), this launch's own picks included (thread 0's stores, read back behind a barrier); the automaton's
 *   state is read once, carried across the positions and moved along every appended pick's edge, and state[u] behind the launch is
 *   the state behind the last appended pick.
 *   The equality.  A verify step's logits rows are, position by position, the bits of single-token steps as long as every earlier
 *   draft was right, and the pick is a function of (row bytes, options, key, history) alone.  With draft_j accepted exactly when
 *   draft_j == pick_{j-1}, the appended ids, log-probabilities, alternatives, done flags and automaton states are therefore those of
 *   dh_engine_decode with the same top_k, seed and options, bit for bit, whatever is drafted; the drafts only decide how many tokens
 *   a step yields.  top_k = 1 is dh_engine_decode_spec's arg-max (the draw is not consulted).
 * Arguments, counters, the acceptance rule, the append order, EOS / stop / budget handling and the refusals (fp8 / MXFP4 engines, the
 * CPU rsqrt emulation, dh_set_tuning key 10, shared-prompt attention, the shape limits) are dh_engine_decode_spec's; top_k >= 0 and
 * seed are dh_engine_decode's.  The options dh_engine_set_nucleus, dh_engine_set_penalties, dh_engine_set_bias and
 * dh_engine_set_automaton have set are applied (under the table limits of dh_engine_decode: tok_ld, plus the bias' ids, at most
 * DH_MAX_PENALTY_HISTORY with penalties on; an automaton needs its eos_id and n_seq).  top_k, seed and every option are part of the
 * captured step's key, and a step of this entry never replays one of dh_engine_decode_spec, or the reverse. */
int dh_engine_decode_spec_draw(dh_engine* e, int64_t* tokens, int tok_ld, int32_t* length, int32_t* done,
                               const int32_t* limit, int n_seq, int max_new_tokens, int n_draft, const int64_t* drafts,
                               int32_t* counters, int n_steps, float temperature, int top_k, int64_t eos_id, uint64_t seed,
                               int first_step, void* stream);
/* Size the per-row workspaces of the single-token steps (logits, fp32 partial sums, ids) for `rows` rows
 * (<= 2048 and <= max_tokens) where dh_engine_create sized them for max_batch: a verify step has
 * n_seq * (n_draft + 1) rows and the KV cache stays at max_batch slots.  Growing drops the captured steps.
 * If the larger workspaces cannot be allocated the call fails and the engine keeps the ones it had. */
int dh_engine_reserve_rows(dh_engine* e, int rows);
/* Beam search inside the engine (see "Beam search" above): n_steps x { prep ; forward of n_utt * W rows ; dh_beam_select ; KV
 * re-parenting }, one linear chain captured on the engine's stream and replayed as dh_engine_decode's step is.  Row u * W + w
 * feeds beam_tok[u, t - 1, w] at position prompt_len[u] + t - 1 in KV slot u * W + w, t = n_steps[u]; the rows of an utterance
 * with done != 0 keep stepping with frozen state (they write the position behind their last one, again and again).  After the
 * selection slot u * W + w must hold the cache of slot u * W + beam_parent[u, t, w]: every layer, K and V^T, the 32-key tiles
 * prompt_len[u] / 32 .. (prompt_len[u] + t - 1) / 32 (the tiles below are equal in all W slots already) are copied through the
 * engine's scratch by two launches — parents' tiles to the scratch, scratch to the own slot — so any parent map (swap, fan-out,
 * identity) is right; rows that continue themselves skip both.  parent, prompt_len and the step are read from device memory: the
 * captured grid is fixed.
 * Before the call: the prompts prefilled into slots u * W and forked into the W - 1 slots behind (dh_engine_copy_prefix), step 0
 * taken by dh_beam_select_bf16 on the prefill's last-position logits (rows_per_utt = 1); first_step >= 1 is the index of the call's
 * first step, i.e. the steps taken so far.
 * prompt_len: device int32 [n_utt].  Needs n_utt * W <= max_batch slots and <= 2048 rows of workspace, prompt_len + max_new_tokens
 * positions in the cache, dh_engine_reserve_beams, and a bf16 engine without the CPU rsqrt emulation (an fp8 engine's step changes
 * its GEMM kernel with the row count). */
int dh_engine_decode_beam(dh_engine* e, const dh_beam_state* st, const int32_t* prompt_len, int n_utt, int W, int max_new_tokens,
                          int n_steps, int64_t eos_id, int first_step, void* stream);
/* Size the re-parenting scratch — max_batch rows x every layer's K and V^T x groups x the (max_new_tokens + 30) / 32 + 1 tiles
 * generated keys can span — and the candidates' workspace for dh_engine_decode_beam calls of up to W beams and max_new_tokens
 * steps.  W = 1 needs no tile scratch.  Growing drops the captured steps; on failure the engine keeps what it had. */
int dh_engine_reserve_beams(dh_engine* e, int W, int max_new_tokens);
/* The buffer (device fp32 [n_seq, tok_ld], the shape of `tokens`; null = off, the default) into which later dh_engine_decode,
 * dh_engine_decode_rows and dh_engine_decode_spec calls write the log-probability of every token they append, beside the token
 * (see "Token log-probabilities" above; a verify step's pick j is scored under its own logits row).  The pointer is part of the
 * captured step's key: a step captured without it is never replayed with it, and the reverse, and with it off the steps hold the
 * kernels they always held.  The caller keeps the buffer alive while it is set. */
int dh_engine_set_logprobs(dh_engine* e, float* buf);
/* The buffers (device int32 ids and fp32 lp, both [n_seq, tok_ld, k]; k = 0 or a null pointer = off, the default) into which later
 * dh_engine_decode, dh_engine_decode_rows and dh_engine_decode_spec calls write the k alternatives of every token they append (see
 * "Token alternatives" above; a verify step's pick j gets those of its own logits row).  It goes with dh_engine_set_logprobs: a
 * decode call with k > 0 and no logprobs buffer fails.  k and both pointers are part of the captured step's key, exactly as the
 * logprobs pointer is.  The caller keeps the buffers alive while they are set. */
int dh_engine_set_top_logprobs(dh_engine* e, int k, int32_t* ids, float* lp);
/* The token mask (device words [n_seq, mask_ld], mask_ld >= ceil(vocab / 32); null = off, the default) under which later
 * dh_engine_decode, dh_engine_decode_rows, dh_engine_decode_spec and dh_engine_decode_beam calls pick their tokens and beam
 * candidates (see "Token masks" above: row u is sequence u's, or utterance u's).  The pointer and mask_ld are part of the captured
 * step's key, exactly as the logprobs pointer is: with the mask unset a decode call runs the graphs it always ran.  The caller
 * keeps the mask alive, and may change its contents between calls, while it is set. */
int dh_engine_set_token_mask(dh_engine* e, const uint32_t* mask, int mask_ld);
/* No-repeat n-grams (see above; generate/base.py:62-80) for later dh_engine_decode, dh_engine_decode_rows and dh_engine_decode_spec
 * calls: ngram in 1 .. 8 with start, device int32 [n_seq] prompt lengths of the calls' sequences; ngram = 0 = off, the default.
 * (ngram, start) is part of the captured step's key, beside the mask: with it unset a decode call runs the graphs it always ran.
 * dh_engine_decode_beam refuses to run while it is set: beam histories live on the host (a beam call's ban is
 * dh_engine_set_beam_history's own ngram, formed on the device histories).  The caller keeps start alive while set. */
int dh_engine_set_no_repeat_ngram(dh_engine* e, int ngram, const int32_t* start);
/* The stop specification (see "Stop conditions" above; null = off, the default) for later dh_engine_decode, dh_engine_decode_rows,
 * dh_engine_decode_spec and dh_engine_decode_beam calls.  start: device int32 [n_seq] prompt lengths, needed with stop sequences (the
 * same numbers as dh_engine_set_no_repeat_ngram's, which win where both are set); beam_fin_tok: device int32 [n_utt, W], needed by a
 * beam call under a stop set (and under stop sequences, which a beam call refuses unless dh_engine_set_beam_history is set).  The specification is copied (the lengths) and pointed to
 * (the device arrays, which the caller keeps alive while set); it is part of the captured step's key, beside the mask and (ngram,
 * start): with it unset a decode call runs the graphs it always ran. */
int dh_engine_set_stop(dh_engine* e, const dh_stop_spec* stop, const int32_t* start, int32_t* beam_fin_tok);
/* Device histories for later dh_engine_decode_beam calls ("Beam histories" of "Beam search"): tokens, device int64
 * [2][n_utt * W][max_new_tokens] (null = off, the default, and clears ngram), and the beam steps' no_repeat_ngram, 0 .. 8.  The
 * caller's step 0 (dh_beam_select_bf16_hist) has written plane 0.  While set, dh_engine_decode_beam bans under ngram and accepts the
 * stop sequences of dh_engine_set_stop (called with the utterances' prompt lengths as start and with beam_fin_tok).
 * dh_engine_set_no_repeat_ngram being set stays a refusal for beam calls, and penalties and a bias stay refused.  The pointer and ngram
 * are part of a beam step's key: with it unset a beam call runs the graphs, and refuses what, it always did.  Refused: ngram outside
 * 0 .. 8, vocab above 131072 with ngram > 0, null tokens with ngram > 0.  The caller keeps the planes alive while set. */
int dh_engine_set_beam_history(dh_engine* e, int64_t* tokens, int ngram);
/* top_p and min_p (see "Nucleus and min-p" above; 1 and 0 = off, the default) for later dh_engine_decode and dh_engine_decode_rows
 * calls with top_k != 1, and for dh_engine_decode_spec_draw's.  Both values are part of the captured step's key, beside the mask, (ngram, start) and the stop specification:
 * with them unset, or with top_k == 1, a decode call runs the graphs it always ran.  Arg-max verify steps and beam steps take neither.  Refused like
 * dh_sample_bf16_nucleus. */
int dh_engine_set_nucleus(dh_engine* e, float top_p, float min_p);
/* The penalties (see "Penalties" above; null or all off clears them, the default) for later dh_engine_decode and dh_engine_decode_rows
 * calls, with any top_k.  `start` ([n_seq] int32 on the device, needed when a penalty is on) is the array dh_engine_set_no_repeat_ngram
 * and dh_engine_set_stop take and holds the same numbers; the caller keeps it alive while set.  The values and `start` are part of the
 * captured step's key: with them unset a decode call runs the graphs it always ran.  While set, dh_engine_decode_spec (not dh_engine_decode_spec_draw, which applies it) and
 * dh_engine_decode_beam refuse, and a decode call with tok_ld above DH_MAX_PENALTY_HISTORY is refused before anything is launched.
 * Refused like dh_sample_bf16_penalty. */
int dh_engine_set_penalties(dh_engine* e, const dh_penalty_args* penalties, const int32_t* start);
/* The bias (see "Contextual biasing" above; null or no entry clears it, the default) for later dh_engine_decode and dh_engine_decode_rows
 * calls.  The spec's device arrays and `start` ([n_seq] int32 on the device, the array the other history readers take) are the caller's to
 * keep alive while set; the host copies are read here only.  The pointers, the counts and `start` are part of the captured step's key:
 * with none set a decode call runs the graphs it always ran.  While set, dh_engine_decode_spec (not dh_engine_decode_spec_draw, which applies it) and dh_engine_decode_beam refuse, and,
 * with penalties set as well, so does a decode call whose tok_ld plus the entries' ids pass DH_MAX_PENALTY_HISTORY.  Refused like
 * dh_sample_bf16_bias. */
int dh_engine_set_bias(dh_engine* e, const dh_bias_spec* bias, const int32_t* start);
/* The automaton set (see "Automaton constraints" above; null clears it, the default) for later dh_engine_decode and dh_engine_decode_rows
 * calls.  The spec's device arrays, `state` among them, and `start` ([n_seq] int32 on the device, the array the other history readers
 * take) are the caller's to keep alive while set; the host copies are read here only.  The pointers, the counts and `start` are part of
 * the captured step's key: with none set a decode call runs the graphs it always ran.  While set, dh_engine_decode_spec (not dh_engine_decode_spec_draw, which applies it) and
 * dh_engine_decode_beam refuse, and a decode call refuses an eos_id outside [0, vocab) or a sequence count other than the spec's n_seq.
 * Refused like dh_sample_bf16_automaton. */
int dh_engine_set_automaton(dh_engine* e, const dh_automaton_spec* automaton, const int32_t* start);
/* Shared-prompt attention (see above; group_rows = 0 or a null d_prompt_len turns it off, the default) for later dh_engine_decode and
 * dh_engine_decode_beam calls: their rows u * group_rows + j are the candidates or beams of utterance u, in slots that
 * dh_engine_fork_slots or dh_engine_copy_prefix has filled from slot u * group_rows, and d_prompt_len is the DEVICE int32
 * [n_seq / group_rows] array of the utterances' prompt lengths.  While set, the step's layers launch dh_attn_decode_shared_bf16 where
 * they launched dh_attn_decode_fused_bf16; every other launch of the step, and every bit it produces, is unchanged.  (group_rows,
 * d_prompt_len) is part of the captured step's key: with it unset a decode call runs the graphs it always ran.  The caller keeps
 * d_prompt_len alive while set.
 * Refused here, with the reason: group_rows outside 2 .. 8; an fp8 or MXFP4 engine (its step does not run the streaming layers) and an
 * fp8 KV cache; the CPU rsqrt emulation; dh_set_tuning key 10 (steps moved to the tiled kernels by row count).  Refused by the calls
 * while it is set, for the same reasons and: dh_engine_decode_spec (a verify step's rows are positions of one sequence),
 * dh_engine_decode_rows (a row list names any sequence in any slot), a row count that is no multiple of group_rows or above the
 * streaming step's 2048, and a beam call whose W is not group_rows. */
int dh_engine_set_shared_prompt(dh_engine* e, int group_rows, const int32_t* d_prompt_len);
/* The tile table ("Beam KV tile table" above; null = off, the default) for later dh_engine_decode_beam calls: tab, device int32
 * [2][n_utt * W][n_tiles], both planes the identity, n_tiles = min((max_new_tokens + 30) / 32 + 1, s_max / 32) of the calls.  While
 * set, a beam step's attention is dh_attn_decode_shared_tab_bf16 and its re-parenting is the table update with the one-tile copy;
 * every other launch of the step is unchanged.  The pointer and n_tiles are part of a beam step's key, as the history planes are: with
 * it unset a beam call runs the graphs it always ran.  While set, dh_engine_decode_beam needs dh_engine_set_shared_prompt with
 * group_rows = W and dh_engine_reserve_beam_tiles, and refuses otherwise with the reason.  Refused here: n_tiles outside
 * 1 .. DH_MAX_BEAM_TILES with a table; an fp8 or MXFP4 engine and an fp8 KV cache.  The caller keeps the planes alive while set. */
int dh_engine_set_beam_tiles(dh_engine* e, int32_t* tab, int n_tiles);
/* dh_engine_reserve_beams for calls under a tile table: the candidates' workspace and a scratch of ONE tile per (row, layer's K and
 * V^T, group) — max_batch x 2 L x G x hs * 32 elements, whatever max_new_tokens is (it is checked: its tiles must not exceed
 * DH_MAX_BEAM_TILES).  W = 1 needs no scratch.  Growing drops the captured steps; on failure the engine keeps what it had. */
int dh_engine_reserve_beam_tiles(dh_engine* e, int W, int max_new_tokens);
/* Test hook, like dh_engine_read: the number of captured steps kept for n_draft drafts (0: dh_engine_decode /
 * dh_engine_decode_rows; -1: all).  Nothing on the serving path calls it. */
int dh_engine_graph_count(const dh_engine* e, int n_draft);

/* Test hook: copy engine state to `dst` (device memory, n_bytes) on `stream`.
 *   what 0: ln_f(x) of the last dh_engine_forward called with logits_all only, [n_tok, d]
 *   what 1: K   cache of `layer`  [max_batch, g, s_max, hs]
 *   what 2: V^T cache of `layer`  [max_batch, g, hs, s_max]
 *   what 3: residual stream x after the last layer of the last forward, [n_tok, d]
 *   what 4: int64 ids of the last step's rows (a verify step: row i * S + j = last token, then the drafts)
 *   what 5: int32 kv_len of the last step's sequences (a verify step: the lengths its drafts were proposed from)
 *   what 6 / 7: an fp8-KV engine's K / V^T cache of `layer` EXPANDED to bf16 (every slot, every position), in the form of
 *               what 1 / 2; overwrites the engine's one-layer scratch.  what 1 / 2 are refused by an fp8-KV engine.
 *   what 8: the bf16 logits rows of the last single-token step, [n_rows, vocab]
 *   what 9 / 10: an fp8-KV engine's K / V^T bytes of `layer` as stored, [max_batch, g, s_max * hs] uint8
 *   what 11 / 12: its K / V exponents of `layer` as stored, [max_batch, g, s_max] int8 */
int dh_engine_read(dh_engine* e, int what, int layer, void* dst, int64_t n_bytes, void* stream);
/* HIP-event timing of the dominant kernels inside the last forward/decode call (bench.py
 * roofline): returns accumulated milliseconds and launch count for kernel class `which`
 * (0 = prefill GEMM, 1 = decode weight-streaming GEMM, 2 = prefill attention,
 *  3 = decode attention); enable with dh_engine_set_timing(e, 1). */
int dh_engine_set_timing(dh_engine* e, int on);
int dh_engine_get_timing(dh_engine* e, int which, double* h_ms, int64_t* h_launches);

#ifdef __cplusplus
}
#endif
#endif /* DUALHYP_HIP_H */
