"""Host model of beam search as include/dualhyp_hip.h defines it ("Beam search"): plain Python over candidate lists, fp32 adds by
numpy.  It knows nothing of the device code: the candidates are sorted whole (no merge of sorted lists), histories are kept as lists
(no backtracking), so the device's selection kernel, its records and the host's backtracking are each checked against another
construction.

An Utterance holds up to W live beams.  step(rows) takes one candidate list per live beam — rows[b] = 2 W (token, lp) pairs in the
order of "Token alternatives" — and applies the definition:
  score(b, j) = cum[b] + lp_j, one fp32 add;
  order: score descending, then b ascending, then j ascending; walk the first 2 W, p = 0, 1, ..:
    EOS and p < W: into the pool if it holds fewer than W; EOS and p >= W: dropped; any other token: the next live beam;
    stop once W live beams are chosen;
  done = 1 when the pool holds W entries, else done = 2 after step number max_new - 1; a done utterance ignores further steps.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

f32 = np.float32


class Utterance:
    def __init__(self, W: int, max_new: int, eos_id: Optional[int] = None) -> None:
        assert 1 <= W <= 4 and max_new > 0
        self.W, self.max_new, self.eos = W, max_new, eos_id
        self.cum: List[np.float32] = [f32(0.0)]          # step 0: one live beam, the prompt
        self.hist: List[Tuple[List[int], List[np.float32]]] = [([], [])]    # per live beam: its tokens and their lps
        self.pool: List[dict] = []                       # finished hypotheses in the order they were appended
        self.done = 0
        self.n_steps = 0
        self.records: List[List[dict]] = []              # per step: the W live beams chosen, in walk order

    def ordered(self, rows: Sequence[Sequence[Tuple[int, float]]]) -> List[dict]:
        assert len(rows) == len(self.cum) and all(len(r) == 2 * self.W for r in rows)
        cands = [dict(b=b, j=j, tok=int(t), lp=f32(lp), score=f32(f32(self.cum[b]) + f32(lp)))
                 for b, row in enumerate(rows) for j, (t, lp) in enumerate(row)]
        return sorted(cands, key=lambda c: (-float(c["score"]), c["b"], c["j"]))

    def step(self, rows) -> None:
        if self.done:
            return
        W, t = self.W, self.n_steps
        live = []
        for p, c in enumerate(self.ordered(rows)[:2 * W]):
            if self.eos is not None and self.eos >= 0 and c["tok"] == self.eos:
                if p < W and len(self.pool) < W:
                    toks, lps = self.hist[c["b"]]
                    self.pool.append(dict(step=t, parent=c["b"], score=c["score"], lp=c["lp"], tokens=list(toks),
                                          token_logprobs=list(lps) + [c["lp"]], finished=True))
                continue
            live.append(c)
            if len(live) == W:
                break
        assert len(live) == W, "a row holds the EOS once: W of the 2 W candidates are never all EOS"
        self.records.append([dict(parent=c["b"], tok=c["tok"], lp=c["lp"], cum=c["score"]) for c in live])
        self.hist = [(self.hist[c["b"]][0] + [c["tok"]], self.hist[c["b"]][1] + [c["lp"]]) for c in live]
        self.cum = [c["score"] for c in live]
        self.n_steps = t + 1
        if len(self.pool) >= W:
            self.done = 1
        elif self.n_steps >= self.max_new:
            self.done = 2

    def completed_pool(self) -> List[dict]:
        """the pool, then the live beams in live order, marked unfinished, while it holds fewer than W entries"""
        pool = [dict(tokens=h["tokens"], token_logprobs=h["token_logprobs"], sum_logprob=float(h["score"]), finished=True) for h in self.pool]
        for w in range(len(self.hist)):
            if len(pool) >= self.W or self.n_steps == 0:
                break
            pool.append(dict(tokens=list(self.hist[w][0]), token_logprobs=list(self.hist[w][1]), sum_logprob=float(self.cum[w]),
                             finished=False))
        return pool

    def ranked(self, length_penalty: float = 1.0) -> List[dict]:
        return rank(self.completed_pool(), length_penalty)


def rank(pool: Sequence[dict], length_penalty: float = 1.0) -> List[dict]:
    """by sum_logprob / n ** length_penalty in Python floats, n = generated tokens with the EOS counted; descending, stable on pool
    order (an insertion sort that moves an entry only past strictly smaller ones)"""
    out: List[dict] = []
    keys: List[float] = []
    for h in pool:
        k = float(h["sum_logprob"]) / float(len(h["token_logprobs"])) ** float(length_penalty)
        i = len(out)
        while i > 0 and keys[i - 1] < k:
            i -= 1
        out.insert(i, h)
        keys.insert(i, k)
    return out


def backtrack_tokens(records: Sequence[Sequence[dict]], step: int, beam: int) -> List[int]:
    """tokens of the hypothesis that is live beam `beam` at step `step`, read backwards through the records' parents"""
    toks = []
    b = beam
    for t in range(step, -1, -1):
        toks.append(records[t][b]["tok"])
        b = records[t][b]["parent"]
    return toks[::-1]


def host_state(utts, W, max_new):
    """the host copy of a device state (dualhyp_amd.beam.BeamState.host()) that holds what the reference utterances recorded: zeros
    where nothing was, lists as .tolist() gives them"""
    n = len(utts)
    h = dict(n_steps=[u.n_steps for u in utts], done=[u.done for u in utts], n_fin=[len(u.pool) for u in utts],
             cum=[[float(c) for c in u.cum] + [0.0] * (W - len(u.cum)) for u in utts])
    for name in ("fin_step", "fin_parent", "fin_score", "fin_lp"):
        h[name] = [[0] * W for _ in range(n)]
    for name in ("beam_tok", "beam_parent", "beam_lp", "beam_cum"):
        h[name] = [[[0] * W for _ in range(max_new)] for _ in range(n)]
    for i, u in enumerate(utts):
        for k, p in enumerate(u.pool):
            h["fin_step"][i][k], h["fin_parent"][i][k] = p["step"], p["parent"]
            h["fin_score"][i][k], h["fin_lp"][i][k] = float(p["score"]), float(p["lp"])
        for t, rec in enumerate(u.records):
            for w, r in enumerate(rec):
                h["beam_tok"][i][t][w], h["beam_parent"][i][t][w] = r["tok"], r["parent"]
                h["beam_lp"][i][t][w], h["beam_cum"][i][t][w] = float(r["lp"]), float(r["cum"])
    return h
