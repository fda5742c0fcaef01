"""The crafted cases of the beam-history checks, built on the CPU: per step one bf16 logits block that does not depend on what the
beams chose, so a case's reference run (tests/beam_history_reference.py) needs only a `top` function — the rows' first 2 W ids under a
per-row bool mask, with their log-probabilities.  cpu_top is torch's fp32 log-softmax (the CPU tests: which events a case holds);
the GPU tests pass ops.token_top_logprobs, which is pinned by its own tests, so the reference sees the device's own fp32 values.

Rows are coarse (multiples of 1/4: ties inside a row and between rows) with a few boosted ids from a small pool per utterance, so
beams repeat tokens and n-grams within a dozen steps whatever the vocabulary size."""
from typing import Callable, List, Optional, Sequence

import torch

import beam_history_reference as HR

N_UTT = 3
STEPS = 10
EVENTS = ("swap", "fanout", "ban_kept", "fallback", "seq_end_reparented", "near_match")


def pack_bool(allow: torch.Tensor) -> torch.Tensor:
    """bool [rows, vocab] -> the int32 words of a token mask (bit i & 31 of word i >> 5)"""
    rows, vocab = allow.shape
    words = (vocab + 31) // 32
    pad = torch.zeros((rows, words * 32), dtype=torch.int64)
    pad[:, :vocab] = allow.to(torch.int64)
    w = (pad.view(rows, words, 32) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def cpu_top(logits: torch.Tensor, k: int, allow: Optional[torch.Tensor]):
    """(ids, lps) as nested lists: the first k allowed ids of every row by value descending, then index ascending (a stable sort),
    with log_softmax of the raw row in fp32"""
    vals = logits.float()
    lp = torch.log_softmax(vals, -1)
    if allow is not None:
        vals = vals.masked_fill(~allow, float("-inf"))
    idx = torch.sort(vals, dim=-1, descending=True, stable=True).indices[:, :k]
    return idx.tolist(), lp.gather(1, idx).tolist()


def craft_logits(seed: int, W: int, vocab: int, steps: int = STEPS) -> List[torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    pools = [torch.randperm(vocab, generator=g)[:min(vocab, 2 * W + 3)] for _ in range(N_UTT)]
    out = []
    for t in range(steps):
        rpu = 1 if t == 0 else W
        x = torch.randint(-8, 9, (N_UTT * rpu, vocab), generator=g).float() / 4
        for r in range(N_UTT * rpu):
            pool = pools[r // rpu]
            pick = pool[torch.randperm(pool.numel(), generator=g)[:min(pool.numel(), 2 * W + 1)]]
            x[r, pick] += 6 + torch.randint(0, 8, (pick.numel(),), generator=g).float() / 2
        out.append(x.to(torch.bfloat16))
    return out


def craft_allow(seed: int, W: int, vocab: int) -> torch.Tensor:
    """bool [N_UTT, vocab]: about three ids in four allowed, never fewer than 2 W; at vocab = 2 W + 1 one id is taken away"""
    g = torch.Generator().manual_seed(seed + 7)
    allow = torch.rand((N_UTT, vocab), generator=g) < 0.75
    for u in range(N_UTT):
        if vocab <= 2 * W + 1:
            allow[u] = True
            allow[u, int(torch.randint(0, vocab, (1,), generator=g))] = False
        elif int(allow[u].sum()) < 2 * W:
            allow[u] = True
    return allow


class Run:
    """A case's reference run, one step at a time"""

    def __init__(self, logits: Sequence[torch.Tensor], W: int, vocab: int, ngram: int, allow: Optional[torch.Tensor], stop_ids=(),
                 stop_seqs=(), eos: Optional[int] = None, top: Callable = cpu_top, max_new: Optional[int] = None) -> None:
        self.logits, self.W, self.vocab, self.ngram, self.allow, self.top = logits, W, vocab, ngram, allow, top
        self.max_new = max_new or len(logits)
        self.allow_sets = None if allow is None else [set(torch.nonzero(a).flatten().tolist()) for a in allow]
        self.utts = [HR.HistUtterance(W, self.max_new, eos, stop_ids, stop_seqs, ngram) for _ in range(N_UTT)]
        self.t = 0

    def advance(self) -> dict:
        """one step of every live utterance -> the rows' mask (bool [rows, vocab], None: everything allowed), their candidates and which
        utterances took the step"""
        t, W = self.t, self.W
        rpu = 1 if t == 0 else W
        live = [not u.done for u in self.utts]
        rowmask = None
        if self.allow is not None or self.ngram:
            base = self.allow if self.allow is not None else torch.ones((N_UTT, self.vocab), dtype=torch.bool)
            rowmask = base.repeat_interleave(rpu, 0).clone()
            for u, ut in enumerate(self.utts):
                for b in range(rpu if live[u] else 0):
                    ban = ut.row_ban(b, self.vocab, None if self.allow_sets is None else self.allow_sets[u])
                    if ban:
                        rowmask[u * rpu + b, sorted(ban)] = False
        ids, lps = self.top(self.logits[t], 2 * W, rowmask)
        for u, ut in enumerate(self.utts):
            if live[u]:
                ut.step([list(zip(ids[u * rpu + b], lps[u * rpu + b])) for b in range(rpu)])
        self.t = t + 1
        return dict(rowmask=rowmask, ids=ids, lps=lps, live=live, rpu=rpu)

    def finish(self) -> "Run":
        while self.t < len(self.logits):
            self.advance()
        return self

    def events(self) -> dict:
        return {k: sum(u.events[k] for u in self.utts) for k in EVENTS}


def pick_sequences(dry: Run, lens=(2, 3)) -> List[List[int]]:
    """stop sequences for a case, read off its run without any: for each length the text's end of a live beam chosen at a step t whose
    parent had itself continued ANOTHER beam at step t - 1 (the ids before the last arrived through a re-parented row), and one
    sequence (z, x) with x a first token of utterance 0: a near-match at step 0 that only an id from before the text's start could
    complete"""
    seqs: List[List[int]] = []
    for L in lens:
        found = None
        for ut in dry.utts:
            for t in range(max(1, L - 1), ut.n_steps):
                for w, r in enumerate(ut.records[t]):
                    b = r["parent"]
                    if ut.records[t - 1][b]["parent"] != b:
                        text = HR.R.backtrack_tokens(ut.records, t - 1, b) + [r["tok"]]
                        if found is None and text[-L:] not in seqs:
                            found = text[-L:]
        if found is not None:
            seqs.append(found)
    x = dry.utts[0].records[0][0]["tok"]
    seqs.append([(x + 1) % dry.vocab, x])
    return seqs


def case_seed(W: int, vocab: int, ngram: int, masked: bool, with_seqs: bool) -> int:
    return 1000 * W + 100 * ngram + 10 * masked + with_seqs + vocab % 977


def build(W: int, vocab: int, ngram: int, masked: bool, with_seqs: bool, top: Callable = cpu_top) -> dict:
    """the inputs of one case: logits per step, the utterances' mask (bool, or None) and its stop sequences (picked from a run
    without them under the same `top`)"""
    seed = case_seed(W, vocab, ngram, masked, with_seqs)
    logits = craft_logits(seed, W, vocab)
    allow = craft_allow(seed, W, vocab) if masked else None
    seqs = pick_sequences(Run(logits, W, vocab, ngram, allow, top=top).finish()) if with_seqs else []
    return dict(W=W, vocab=vocab, ngram=ngram, logits=logits, allow=allow, stop_seqs=seqs)


def small_cases():
    """(W, vocab, ngram, masked, with_seqs) of the cases whose events the coverage checks count: vocab = 2 W + 1 and 40"""
    return [(W, v, n, m, s) for W in (1, 2, 3, 4) for v in (2 * W + 1, 40) for n in (1, 2, 3) for m in (False, True) for s in (False, True)]
