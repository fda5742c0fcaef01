"""Stop conditions in the sampling kernels, through ops.sample and ops.sample_rows (include/dualhyp_hip.h, "Stop conditions").  Exact.

Hand-built logits rows whose arg-max is scripted step by step: a sequence's row at step t is small noise with a peak at the scripted
id.  Every case runs twice from the same rows, without and with the specification; the stopped run must be the unstopped run up to
and including the first position at which dualhyp_amd.stop.first_stop says the condition holds — token, log-probability and
alternatives — with done = 3 from exactly that step on and nothing written behind it, and the cases then state where that is."""
import ctypes as C

import pytest
import torch

from dualhyp_amd import _lib, ops
from dualhyp_amd.stop import compile_stop, first_stop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 3
VOCABS = (515, 4096)            # 515: no multiple of 8 (the scalar loops) or 32 (a partial last word of the set)
ENTRIES = ("sample", "sample_rows")
GREEDY = dict(temperature=1.0, top_k=1)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def rows_for(V, scripts, t, seed):
    """bf16 [B, V]: noise in about [-2, 2] and, where the script names an id for step t, a peak on it"""
    g = torch.Generator().manual_seed(seed * 1000 + t)
    lg = torch.randn((len(scripts), V), generator=g) * 0.6
    for u, s in enumerate(scripts):
        if s is not None and t < len(s):
            lg[u, s[t]] = 9.0
    return lg.to(torch.bfloat16).to(DEV)


def drive(entry, V, prompts, scripts, steps, stop, eos=None, seed=5, kw=GREEDY, room=0):
    """`steps` sampler calls over len(prompts) sequences whose budget is steps + room tokens -> the final state and done after every call"""
    B = len(prompts)
    lens = [len(p) for p in prompts]
    assert entry == "sample_rows" or len(set(lens)) == 1 or room > 0, "sample()'s budget is the buffer: equal prompts end together"
    max_new = steps + room
    tok_ld = max(lens) + max_new
    tokens = torch.zeros((B, tok_ld), dtype=torch.int64)
    for u, p in enumerate(prompts):
        tokens[u, :len(p)] = torch.tensor(p, dtype=torch.int64)
    tokens = tokens.to(DEV)
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    start = length.clone()
    done = torch.zeros(B, dtype=torch.int32, device=DEV)
    lp = torch.full((B, tok_ld), float("nan"), dtype=torch.float32, device=DEV)
    top = (torch.full((B, tok_ld, K), -1, dtype=torch.int32, device=DEV), torch.full((B, tok_ld, K), float("nan"), dtype=torch.float32, device=DEV))
    limit = torch.tensor([n + max_new for n in lens], dtype=torch.int32, device=DEV)
    order = list(range(B))[::-1]                      # the row list names the sequences backwards: row r is sequence B - 1 - r
    row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
    history = []
    for t in range(steps):
        lg = rows_for(V, scripts, t, seed)
        if entry == "sample":
            ops.sample(lg, tokens, length, done, eos_id=eos, seed=seed, step=t, logprobs=lp, top_logprobs=top, stop=stop,
                       start=start if stop is not None else None, **kw)
        else:
            # start None: the prompt lengths are limit - max_new_tokens
            ops.sample_rows(lg[order].contiguous(), tokens, length, done, limit, row_seq, max_new, eos_id=eos, seed=seed, logprobs=lp,
                            top_logprobs=top, stop=stop, **kw)
        history.append(done.tolist())
    return dict(tokens=tokens.cpu(), length=length.tolist(), done=done.tolist(), lp=lp.cpu(), top_ids=top[0].cpu(), top_lp=top[1].cpu(),
                history=history, lens=lens)


def check(entry, V, prompts, scripts, steps, ids, seqs, eos=None, seed=5, kw=GREEDY, room=0):
    """the unstopped and the stopped run of one case, compared as the module's docstring says -> (first stops, done) per sequence"""
    spec = compile_stop(ids, seqs, V, DEV)
    off = drive(entry, V, prompts, scripts, steps, None, eos, seed, kw, room)
    on = drive(entry, V, prompts, scripts, steps, spec, eos, seed, kw, room)
    stops = []
    for u, p in enumerate(off["lens"]):
        g = off["tokens"][u, p:off["length"][u]].tolist()
        fs = first_stop(g, spec)
        if fs is not None and eos is not None and g[fs] == eos:
            fs = None                                                   # the EOS wins; the unstopped run ended there too
        stops.append(fs)
        n = off["length"][u] if fs is None else p + fs + 1
        what = f"{entry} V={V} sequence {u}: first stop {fs}, unstopped {g}"
        assert on["length"][u] == n, what
        assert on["done"][u] == (off["done"][u] if fs is None else 3), what
        assert torch.equal(on["tokens"][u, :n], off["tokens"][u, :n]) and not on["tokens"][u, n:].any(), what
        assert same_bits(on["lp"][u, p:n], off["lp"][u, p:n]) and bool(on["lp"][u, n:].isnan().all()), what
        assert torch.equal(on["top_ids"][u, p:n], off["top_ids"][u, p:n]) and bool((on["top_ids"][u, n:] == -1).all()), what
        assert same_bits(on["top_lp"][u, p:n], off["top_lp"][u, p:n]) and bool(on["top_lp"][u, n:].isnan().all()), what
        assert not on["lp"][u, p:n].isnan().any() and bool((on["top_ids"][u, p:n] >= 0).all()), what
        # done = 3 from exactly the stopping call on; before it the flags are the unstopped run's
        for t, (a, b) in enumerate(zip(on["history"], off["history"])):
            assert a[u] == (3 if fs is not None and t >= fs else b[u]), f"{what}: done after call {t}"
    return stops, on["done"]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_stop_set_at_the_scripted_step(entry, V):
    S_, T_ = V - 1, 33                           # the last id (the set's partial last word at 515), and one in word 1
    prompts = [[7, S_, 9], [S_, S_, S_], [1, 2, 3], [4, 5, 6]]         # a stop id in a prompt stops nothing
    scripts = [[10, 11, S_, 12, 13, 14], [20, 21, 22, 23, 24, 25], [S_, 30, 31, 32, 33, 34], [40, 41, 42, 43, T_, S_]]
    stops, done = check(entry, V, prompts, scripts, 6, [S_, T_], [], room=2)
    assert stops == [2, None, 0, 4] and done == [3, 0, 3, 3]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_eos_wins_and_the_last_budget_place_is_a_stop(entry, V):
    E_, S_ = 77, 300
    prompts = [[1, 2], [3, 4], [5, 6], [7, 8]]
    # the EOS is a stop id too: done = 1; a stop id on the last place of the budget: 3, not 2; no stop at all: 2; a plain stop
    scripts = [[10, E_, 11, 12], [20, 21, 22, S_], [30, 31, 32, 33], [40, S_, 41, 42]]
    stops, done = check(entry, V, prompts, scripts, 4, [E_, S_], [], eos=E_)
    assert stops == [None, 3, None, 1] and done == [1, 3, 2, 3]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_stop_sequences(entry, V):
    A_, B_, X_ = 100, 200, 400
    eight = list(range(40, 48))
    seqs = [[A_, B_], [X_, X_, B_], eight]
    prompts = [[5, 6, A_],              # A B would match only across the prompt boundary: it does not fire, the later A B does
               [7, X_, X_],             # likewise X X B
               [8, 9, 10],              # overlap: X X B in X X X B
               eight[:3],               # the first three of the eight in the prompt, the other five generated: no match
               [11, 12, 13]]            # one token, then all eight
    scripts = [[B_, 20, A_, B_, 21, 22, 23, 24, 25, 26], [B_, 30, 31, 32, 33, 34, 35, 36, 37, 38], [X_, X_, X_, B_, 50, 51, 52, 53, 54, 55],
               eight[3:] + [60, 61, 62, 63, 64], [70] + eight + [71]]
    stops, done = check(entry, V, prompts, scripts, 10, [], seqs, room=1)
    assert stops == [3, None, 3, None, 8] and done == [3, 0, 3, 0, 3]
    # a sequence that ends on the last place of the budget, and the set beside the sequences
    stops, done = check(entry, V, [[1, 2, 3]] * 3, [[20, 21, A_, B_], [A_, 22, 23, B_], [24, 5, A_, B_]], 4, [5], [[A_, B_]])
    assert stops == [3, None, 1] and done == [3, 2, 3]


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_sampled_picks_stop_where_the_unstopped_draw_says(entry, V):
    """top_k = 5 with a seed and no scripted peak: the specification is taken from the unstopped draw's own ids"""
    kw = dict(temperature=0.8, top_k=5)
    prompts = [[1, 2, 3]] * 6
    free = drive(entry, V, prompts, [None] * 6, 8, None, seed=9, kw=kw)
    g = [free["tokens"][u, 3:11].tolist() for u in range(6)]
    assert len({tuple(x) for x in g}) > 1, "the draw is keyed by the sequence"
    ids, seqs = [g[0][2], g[1][5]], [g[2][3:5], g[3][0:3]]
    stops, done = check(entry, V, prompts, [None] * 6, 8, ids, seqs, seed=9, kw=kw)
    assert stops[0] is not None and stops[0] <= 2 and stops[1] is not None and stops[1] <= 5 and stops[2] is not None and stops[2] <= 4
    assert stops[3] is not None and stops[3] <= 2 and len({s for s in stops if s is not None}) >= 2
    assert all(d == (3 if s is not None else 2) for s, d in zip(stops, done))


@pytest.mark.parametrize("V", VOCABS)
def test_a_null_specification_is_the_entry_without_one(V):
    """dh_sample_bf16_stop / dh_sample_rows_bf16_stop called with stop = null against ops.sample / ops.sample_rows, which call the
    entries they always called: the same bits, greedy and sampled"""
    lib = _lib.load()
    B, steps = 4, 5
    for kw, seed in ((GREEDY, 3), (dict(temperature=0.7, top_k=5), 11)):
        for entry in ENTRIES:
            want = drive(entry, V, [[1, 2, 3]] * B, [None] * B, steps, None, eos=17, seed=seed, kw=kw)
            tok_ld = 3 + steps
            tokens = torch.zeros((B, tok_ld), dtype=torch.int64)
            tokens[:, :3] = torch.tensor([1, 2, 3])
            tokens = tokens.to(DEV)
            length = torch.full((B,), 3, dtype=torch.int32, device=DEV)
            done = torch.zeros(B, dtype=torch.int32, device=DEV)
            lp = torch.full((B, tok_ld), float("nan"), dtype=torch.float32, device=DEV)
            t_ids = torch.full((B, tok_ld, K), -1, dtype=torch.int32, device=DEV)
            t_lp = torch.full((B, tok_ld, K), float("nan"), dtype=torch.float32, device=DEV)
            limit = torch.full((B,), 3 + steps, dtype=torch.int32, device=DEV)
            order = list(range(B))[::-1]
            row_seq = torch.tensor(order, dtype=torch.int32, device=DEV)
            stream = torch.cuda.current_stream().cuda_stream
            for t in range(steps):
                lg = rows_for(V, [None] * B, t, seed)
                if entry == "sample":
                    _lib.check(lib.dh_sample_bf16_stop(lg.data_ptr(), V, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(), B,
                                                       kw["temperature"], kw["top_k"], 17, seed, t, stream, lp.data_ptr(), K, t_ids.data_ptr(),
                                                       t_lp.data_ptr(), None, 0, 0, None, None))
                else:
                    lg = lg[order].contiguous()
                    _lib.check(lib.dh_sample_rows_bf16_stop(lg.data_ptr(), V, tokens.data_ptr(), tok_ld, length.data_ptr(), done.data_ptr(),
                                                            limit.data_ptr(), row_seq.data_ptr(), B, B, steps, kw["temperature"], kw["top_k"],
                                                            17, seed, stream, lp.data_ptr(), K, t_ids.data_ptr(), t_lp.data_ptr(), None, 0, 0,
                                                            None, None))
                torch.cuda.synchronize()        # lg is this iteration's
            what = f"{entry} V={V} {kw}"
            assert torch.equal(tokens.cpu(), want["tokens"]) and length.tolist() == want["length"] and done.tolist() == want["done"], what
            assert same_bits(lp.cpu(), want["lp"]) and torch.equal(t_ids.cpu(), want["top_ids"]) and same_bits(t_lp.cpu(), want["top_lp"]), what
    # an empty specification is null too
    empty = _lib.StopSpec(None, None, None, 0)
    lg = rows_for(V, [[5]], 0, 1)
    tokens = torch.zeros((1, 4), dtype=torch.int64, device=DEV)
    length = torch.ones(1, dtype=torch.int32, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(lib.dh_sample_bf16_stop(lg.data_ptr(), V, tokens.data_ptr(), 4, length.data_ptr(), done.data_ptr(), 1, 1.0, 1, -1, 0, 0,
                                       torch.cuda.current_stream().cuda_stream, None, 0, None, None, None, 0, 0, None, C.byref(empty)))
    assert tokens.tolist() == [[0, 5, 0, 0]] and done.tolist() == [0]


def test_ops_refusals():
    V = 515
    lg = rows_for(V, [[5]], 0, 1)
    tokens = torch.zeros((1, 4), dtype=torch.int64, device=DEV)
    length = torch.ones(1, dtype=torch.int32, device=DEV)
    done = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="need start"):
        ops.sample(lg, tokens, length, done, stop=compile_stop([], [[1, 2]], V, DEV), **GREEDY)
    with pytest.raises(ValueError, match="compiled for"):
        ops.sample(lg, tokens, length, done, stop=compile_stop([1], [], V + 1, DEV), **GREEDY)
    with pytest.raises(_lib.DualHypHipError, match="GPU"):
        ops.sample(lg, tokens, length, done, stop=compile_stop([1], [], V), **GREEDY)
    with pytest.raises(TypeError):
        ops.sample(lg, tokens, length, done, stop=[1], **GREEDY)
    assert tokens.tolist() == [[0, 0, 0, 0]] and done.tolist() == [0]
