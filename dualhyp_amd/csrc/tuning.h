// Every knob dh_set_tuning (capi.hip) can set, declared once: the file that defines a knob includes this header too, so a
// definition whose type or name drifts from the table's is a compile error.  Defaults and meanings are at the definitions.
#pragma once

extern int g_gemm128_stages, g_gemm_variant, g_tail_split, g_linear_phase;               // gemm.hip
extern int g_gemm_gm, g_w4_persist, g_w4_fast_epi, g_w4_persist_qkv, g_w4_persist_lora;   // gemm256.hip
extern int g_mid, g_mid_wlds;                                                             // gemm_mid.hip
extern int g_dt_stages, g_dt_wide, g_dt_min_rows, g_chain_min_rows, g_pairs_wn, g_pairs_wt;   // gemm_dt.hip
extern int g_pairs_min_rows, g_skinny_n;                                                  // gemm_skinny.hip
// gemm_skinny.hip as well; file-local until the table moved out of that file, and still not in the library's dynamic symbol table
__attribute__((visibility("hidden"))) extern int g_skinny_variant, g_swiglu2, g_rows_ct, g_rows_ng;
extern int g_fp8_tile, g_fp8_gm;                                                          // fp8.hip
extern int g_decode_tiled_rows, g_short_kps, g_fuse_qkv_rope, g_prune_last_layer;         // engine.hip
extern int g_attn_bwd_dkdv_img, g_attn_bwd_dq_group;                                      // attention_bwd.hip
extern int g_tn_mfma;                                                                     // train_kernels.hip
extern int g_attn_chain, g_finish_hoist_rows, g_finish_rows_min, g_finish_rpb;                                            // decode_fused.hip
extern int g_prefill_wpb;                                                                 // attention.hip
