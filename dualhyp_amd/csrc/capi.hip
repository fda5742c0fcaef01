// Error plumbing, device info and the tuning switchboard of the C ABI.
#include "common.h"
#include "tuning.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

void dh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* dh_last_error(void) { return g_err; }
extern "C" int dh_abi_version(void) { return DH_ABI_VERSION; }

// dh_stop_spec -> what the kernels take by value, with the header's argument checks ("Stop conditions"): nothing is launched
int dh_stop_pack(const char* name, const dh_stop_spec* stop, bool start_ok, dh_stop_args& out) {
    out = dh_stop_args{};
    if (!stop) return 0;
    DH_CHECK(stop->n_seqs >= 0 && stop->n_seqs <= DH_MAX_STOP_SEQS, "%s: %d stop sequences, at most %d are supported", name, stop->n_seqs,
             DH_MAX_STOP_SEQS);
    DH_CHECK(stop->n_seqs == 0 || (stop->seqs && stop->h_seq_len), "%s: %d stop sequences without their ids or their lengths", name,
             stop->n_seqs);
    uint32_t lens = 0;
    for (int i = 0; i < stop->n_seqs; ++i) {
        const int L = stop->h_seq_len[i];
        DH_CHECK(L >= 2 && L <= DH_MAX_STOP_LEN, "%s: stop sequence %d has %d tokens, 2 .. %d are supported (one token belongs in the stop set)",
                 name, i, L, DH_MAX_STOP_LEN);
        lens |= (uint32_t)L << (4 * i);
    }
    DH_CHECK(stop->n_seqs == 0 || start_ok, "%s: stop sequences need `start`, the prompt lengths: a match never reaches into the prompt", name);
    out.set = stop->set;
    out.seqs = stop->n_seqs ? stop->seqs : nullptr;
    out.lens = lens;
    out.n_seqs = stop->n_seqs;
    return 0;
}

// (top_p, min_p) -> what the kernels take by value, with the header's argument checks ("Nucleus and min-p"): nothing is launched
int dh_nucleus_pack(const char* name, float top_p, float min_p, dh_nucleus_args& out) {
    out = dh_nucleus_args{};
    DH_CHECK(top_p > 0.f && top_p <= 1.f, "%s: top_p=%g is not in (0, 1] (1 = off)", name, (double)top_p);      // false for a NaN
    DH_CHECK(min_p >= 0.f && min_p <= 1.f, "%s: min_p=%g is not in [0, 1] (0 = off)", name, (double)min_p);
    out.top_p = top_p;
    out.min_p = min_p;
    out.min_p_on = min_p > 0.f;
    out.lmin = out.min_p_on ? (float)log((double)min_p) : 0.f;
    return 0;
}

// dh_penalty_args checked, with the header's ranges ("Penalties"): nothing is launched.  Null is off.  Every comparison is false for a NaN.
int dh_penalty_pack(const char* name, const dh_penalty_args* in, dh_penalty_args& out) {
    out = DH_PENALTY_OFF;
    if (!in) return 0;
    DH_CHECK(in->repetition >= 0.125f && in->repetition <= 8.f, "%s: repetition=%g is not in [1/8, 8] (1 = off)", name, (double)in->repetition);
    DH_CHECK(in->frequency >= -8.f && in->frequency <= 8.f, "%s: frequency=%g is not in [-8, 8] (0 = off)", name, (double)in->frequency);
    DH_CHECK(in->presence >= -8.f && in->presence <= 8.f, "%s: presence=%g is not in [-8, 8] (0 = off)", name, (double)in->presence);
    out = *in;
    return 0;
}

// dh_bias_spec -> what the kernels take by value, with the header's argument checks ("Contextual biasing"), made on the host copies:
// nothing is launched.  Null or no entry is off.
int dh_bias_pack(const char* name, const dh_bias_spec* spec, int vocab, bool start_ok, dh_bias_args& out) {
    out = dh_bias_args{};
    if (!spec || spec->n == 0) return 0;
    DH_CHECK(spec->n > 0 && spec->n <= DH_MAX_BIAS_ENTRIES, "%s: %d bias entries, 1 .. %d are supported", name, spec->n, DH_MAX_BIAS_ENTRIES);
    DH_CHECK(spec->ids && spec->len && spec->boost && spec->h_ids && spec->h_len && spec->h_boost,
             "%s: %d bias entries without their ids, lengths or boosts (device arrays and host copies)", name, spec->n);
    DH_CHECK(vocab <= 131072, "%s: a bias keeps a sequence's overridden columns in an LDS row of 131072 ids; vocab=%d does not fit", name, vocab);
    int n_ids = 0;
    for (int e = 0; e < spec->n; ++e) {
        const int L = spec->h_len[e];
        DH_CHECK(L >= 1 && L <= DH_MAX_BIAS_LEN, "%s: bias entry %d has %d ids, 1 .. %d are supported", name, e, L, DH_MAX_BIAS_LEN);
        for (int k = 0; k < L; ++k) {
            const int t = spec->h_ids[e * DH_MAX_BIAS_LEN + k];
            DH_CHECK(t >= 0 && t < vocab, "%s: bias entry %d holds id %d, outside the vocabulary of %d", name, e, t, vocab);
        }
        const float b = spec->h_boost[e];
        DH_CHECK(b - b == 0.f, "%s: bias entry %d has the boost %g, which is not finite", name, e, (double)b);      // false for inf and NaN
        n_ids += L;
    }
    DH_CHECK(start_ok, "%s: a bias needs `start`, the prompt lengths: a match never reaches into the prompt", name);
    out.ids = spec->ids;
    out.len = spec->len;
    out.boost = spec->boost;
    out.n = spec->n;
    out.n_ids = n_ids;
    return 0;
}

// dh_automaton_spec -> what the kernels take by value, with the header's argument checks ("Automaton constraints"), made on the host
// copies: nothing is launched.  Null is off.  What depends on the call (eos_id, the sequence count) is the launchers' check_pick's.
int dh_automaton_pack(const char* name, const dh_automaton_spec* spec, int vocab, bool start_ok, dh_automaton_args& out) {
    out = dh_automaton_args{};
    if (!spec) return 0;
    const int S = spec->n_states, E = spec->n_edges;
    DH_CHECK(S >= 1 && E >= 0 && spec->n_seq >= 1, "%s: an automaton set of %d states, %d edges and %d sequences", name, S, E, spec->n_seq);
    DH_CHECK(spec->edge_off && spec->edge_tok && spec->edge_dst && spec->init && spec->state && spec->h_edge_off && spec->h_edge_tok &&
             spec->h_edge_dst && spec->h_init, "%s: an automaton set without its offsets, tokens, destinations, start states or state "
             "buffer (device arrays and host copies)", name);
    DH_CHECK(vocab <= 131072, "%s: an automaton's allowed row is an LDS row of 131072 ids; vocab=%d does not fit", name, vocab);
    DH_CHECK(spec->h_edge_off[0] == 0 && spec->h_edge_off[S] == E, "%s: the edge offsets run from %d to %d, not from 0 to the %d edges", name,
             spec->h_edge_off[0], spec->h_edge_off[S], E);
    for (int q = 0; q < S; ++q)
        DH_CHECK(spec->h_edge_off[q] <= spec->h_edge_off[q + 1] && spec->h_edge_off[q + 1] <= E, "%s: the edge offsets are not monotone at "
                 "state %d (%d, then %d, of %d edges)", name, q, spec->h_edge_off[q], spec->h_edge_off[q + 1], E);
    for (int q = 0; q < S; ++q) {
        const int lo = spec->h_edge_off[q], hi = spec->h_edge_off[q + 1];
        for (int e = lo; e < hi; ++e) {
            const int t = spec->h_edge_tok[e], d = spec->h_edge_dst[e];
            DH_CHECK(t >= 0 && t < vocab, "%s: state %d has an edge on token %d, outside the vocabulary of %d", name, q, t, vocab);
            DH_CHECK(e == lo || spec->h_edge_tok[e - 1] < t, "%s: the edge tokens of state %d are not strictly ascending (%d, then %d)", name,
                     q, spec->h_edge_tok[e > lo ? e - 1 : e], t);
            DH_CHECK(d >= 0 && d < S, "%s: an edge of state %d leads to state %d, outside the %d states", name, q, d, S);
        }
    }
    for (int u = 0; u < spec->n_seq; ++u)
        DH_CHECK(spec->h_init[u] >= 0 && spec->h_init[u] < S, "%s: sequence %d starts in state %d, outside the %d states", name, u,
                 spec->h_init[u], S);
    DH_CHECK(start_ok, "%s: an automaton needs `start`, the prompt lengths: a sequence is in its start state while it has generated nothing",
             name);
    out.edge_off = spec->edge_off;
    out.edge_tok = spec->edge_tok;
    out.edge_dst = spec->edge_dst;
    out.init = spec->init;
    out.state = spec->state;
    out.n_states = S;
    out.n_edges = E;
    out.n_seq = spec->n_seq;
    return 0;
}

extern "C" int dh_device_info(char* h_buf, int h_buf_len, int* h_num_cu, int64_t* h_hbm_bytes) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    DH_CHECK(e == hipSuccess && n > 0, "no HIP device visible (%s)", hipGetErrorString(e));
    int dev = 0;
    DH_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    DH_HIP(hipGetDeviceProperties(&p, dev));
    if (h_buf && h_buf_len > 0) {
        strncpy(h_buf, p.gcnArchName, h_buf_len - 1);
        h_buf[h_buf_len - 1] = 0;
    }
    if (h_num_cu) *h_num_cu = p.multiProcessorCount;
    if (h_hbm_bytes) *h_hbm_bytes = (int64_t)p.totalGlobalMem;
    return 0;
}

// ---- dh_set_tuning: one row per key ------------------------------------------------------------------------------------------
// A/B switches and forced kernel choices for tools, tests and bench.py --tune, addressed by number.  A value outside a row's
// filter leaves the knob alone and is refused like an unknown key.
namespace {

enum Accept { ANY, BOOL /* stored as value != 0 */, RANGE /* a <= value <= b */, ONE_OF /* value is a, b or c */ };
struct TuningRow { int key; int* knob; Accept accept; int a, b, c; };
constexpr int NO_MAX = 0x7fffffff;

const TuningRow TUNING[] = {
    {0, &g_skinny_variant, ANY, 0, 0, 0},
    {1, &g_gemm_variant, ANY, 0, 0, 0},
    {2, &g_swiglu2, ANY, 0, 0, 0},
    {3, &g_mid, ANY, 0, 0, 0},
    {4, &g_linear_phase, ANY, 0, 0, 0},
    {5, &g_gemm_gm, RANGE, 0, NO_MAX, 0},
    {6, &g_dt_min_rows, RANGE, 1, NO_MAX, 0},
    {7, &g_chain_min_rows, RANGE, 1, NO_MAX, 0},
    {8, &g_dt_stages, ANY, 0, 0, 0},
    {9, &g_gemm128_stages, ANY, 0, 0, 0},
    {10, &g_decode_tiled_rows, RANGE, 0, NO_MAX, 0},
    {11, &g_rows_ct, RANGE, 0, NO_MAX, 0},
    {12, &g_fuse_qkv_rope, ANY, 0, 0, 0},
    {13, &g_mid_wlds, ANY, 0, 0, 0},
    {14, &g_rows_ng, ONE_OF, 0, 8, 10},
    {15, &g_dt_wide, ANY, 0, 0, 0},
    {16, &g_short_kps, ONE_OF, 8, 16, 16},
    {17, &g_pairs_wn, ONE_OF, 0, 2, 4},
    {18, &g_pairs_min_rows, RANGE, 1, NO_MAX, 0},
    {19, &g_fp8_tile, ONE_OF, 0, 128, 256},
    {20, &g_fp8_gm, RANGE, 0, 64, 0},
    {21, &g_pairs_wt, BOOL, 0, 0, 0},
    {22, &g_w4_persist, RANGE, 0, 2, 0},
    {23, &g_prune_last_layer, BOOL, 0, 0, 0},
    {24, &g_w4_fast_epi, ANY, 0, 0, 0},   // only bit 2 selects anything today (gemm256.hip)
    {25, &g_w4_persist_qkv, BOOL, 0, 0, 0},
    {26, &g_tn_mfma, BOOL, 0, 0, 0},
    {27, &g_attn_bwd_dq_group, BOOL, 0, 0, 0},
    {28, &g_tail_split, BOOL, 0, 0, 0},
    {29, &g_attn_bwd_dkdv_img, BOOL, 0, 0, 0},
    {30, &g_w4_persist_lora, BOOL, 0, 0, 0},
    {31, &g_skinny_n, BOOL, 0, 0, 0},
    // 32 stays unassigned: it is the key tests/test_capi.py uses as the unknown one
    {40, &g_attn_chain, BOOL, 0, 0, 0},
    {41, &g_finish_hoist_rows, RANGE, -1, NO_MAX, 0},   // -1: the built-in crossover
    {42, &g_prefill_wpb, ONE_OF, 0, 2, 4},
    {43, &g_finish_rows_min, RANGE, -1, NO_MAX, 0},     // -1: the built-in crossover
    {44, &g_finish_rpb, RANGE, 0, 64, 0},               // 0: the built-in count
};

}  // namespace

extern "C" int dh_set_tuning(int key, int value) {
    for (const TuningRow& r : TUNING) {
        if (r.key != key) continue;
        if (r.accept == RANGE && (value < r.a || value > r.b)) break;
        if (r.accept == ONE_OF && value != r.a && value != r.b && value != r.c) break;
        *r.knob = r.accept == BOOL ? value != 0 : value;
        return 0;
    }
    dh_set_error("dh_set_tuning: unknown key %d", key);
    return 1;
}
