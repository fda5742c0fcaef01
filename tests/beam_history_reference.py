"""Host model of beam search over device histories (include/dualhyp_hip.h, "Beam histories"): tests/beam_reference.py's utterance with
  per-beam histories — beam_reference keeps them as lists already; here they are what the ban and the stop sequences read;
  the banned candidate list of a row — the full row ordered by (-value, index), filtered by the mask and by ngram.banned of the
    beam's own history, the ban dropped when it leaves fewer than 2 W ids;
  the stop-sequence rule — a candidate x of beam b ends its hypothesis when x is in the stop set or when H(b) + [x] ends on a stop
    sequence, never reaching behind the hypothesis' first generated token; the EOS wins where both hold.
Plain Python: it knows nothing of planes, parities or kernels."""
from typing import Iterable, List, Optional, Sequence, Set

import beam_reference as R
from dualhyp_amd.ngram import banned


def effective_ban(hist: Sequence[int], vocab: int, W: int, ngram: int, allowed: Optional[Set[int]] = None) -> Set[int]:
    """the ids the ban takes from a row: ngram.banned of `hist` among the ids the mask allows (`allowed`, ids in [0, vocab); None:
    all of them) — or nothing when that would leave fewer than 2 W ids (the fallback)"""
    if not ngram:
        return set()
    cut = {i for i in banned(list(hist), ngram) if 0 <= i < vocab and (allowed is None or i in allowed)}
    n = vocab if allowed is None else len(allowed)
    return cut if n - len(cut) >= 2 * W else set()


def candidates(values: Sequence[float], hist: Sequence[int], W: int, ngram: int, allowed: Optional[Set[int]] = None) -> List[int]:
    """the 2 W candidate ids of a row whose raw values are `values`: the first 2 W ids that the mask allows and the ban leaves, in the
    raw row's order, value descending (-0 == +0 as floats compare), then index ascending"""
    ban = effective_ban(hist, len(values), W, ngram, allowed)
    order = sorted(range(len(values)), key=lambda i: (-float(values[i]), i))
    return [i for i in order if (allowed is None or i in allowed) and i not in ban][:2 * W]


class HistUtterance(R.Utterance):
    def __init__(self, W: int, max_new: int, eos_id: Optional[int] = None, stop_ids: Iterable[int] = (),
                 stop_seqs: Iterable[Sequence[int]] = (), ngram: int = 0) -> None:
        super().__init__(W, max_new, eos_id)
        self.stop_ids = set(int(t) for t in stop_ids)
        self.stop_seqs = [tuple(int(t) for t in s) for s in stop_seqs]
        assert all(2 <= len(s) <= 8 for s in self.stop_seqs) and len(self.stop_seqs) <= 8
        self.ngram = ngram
        self.events = dict(swap=0, fanout=0, ban_kept=0, fallback=0, seq_end_reparented=0, near_match=0, eos_and_seq=0)

    # ---- what a row may offer ----
    def history(self, b: int) -> List[int]:
        return list(self.hist[b][0])

    def row_ban(self, b: int, vocab: int, allowed: Optional[Set[int]] = None) -> Set[int]:
        """effective_ban of live beam b's row — and the events of the coverage checks: a non-empty ban that was kept, a row that
        fell back"""
        h = self.history(b)
        ban = effective_ban(h, vocab, self.W, self.ngram, allowed)
        if self.ngram and not self.done:
            if ban:
                self.events["ban_kept"] += 1
            elif any(0 <= i < vocab and (allowed is None or i in allowed) for i in banned(h, self.ngram)):
                self.events["fallback"] += 1
        return ban

    # ---- what ends a hypothesis ----
    def seq_hit(self, b: int, tok: int) -> bool:
        text = self.history(b) + [tok]
        for s in self.stop_seqs:
            if len(s) <= len(text) and tuple(text[len(text) - len(s):]) == s:
                return True
            if len(s) > len(text) and tuple(text) == s[len(s) - len(text):]:
                self.events["near_match"] += 1          # the text is the sequence's tail: only ids from before its start would complete it
        return False

    def step(self, rows) -> None:
        if self.done:
            return
        W, t = self.W, self.n_steps
        live = []
        for p, c in enumerate(self.ordered(rows)[:2 * W]):
            is_eos = self.eos is not None and self.eos >= 0 and c["tok"] == self.eos
            by_seq = self.seq_hit(c["b"], c["tok"])
            if is_eos or c["tok"] in self.stop_ids or by_seq:
                if p < W and len(self.pool) < W:
                    toks, lps = self.hist[c["b"]]
                    self.pool.append(dict(step=t, parent=c["b"], score=c["score"], lp=c["lp"], tok=c["tok"],
                                          tokens=list(toks) + ([] if is_eos else [c["tok"]]), token_logprobs=list(lps) + [c["lp"]],
                                          finished=True, finish_reason="eos" if is_eos else "stop"))
                    self.events["eos_and_seq"] += is_eos and by_seq
                    if by_seq and not is_eos and c["tok"] not in self.stop_ids and t >= 1 and self.records[t - 1][c["b"]]["parent"] != c["b"]:
                        self.events["seq_end_reparented"] += 1
                continue
            live.append(c)
            if len(live) == W:
                break
        assert len(live) == W, "the test's rows leave W candidates that end nothing"
        parents = [c["b"] for c in live]
        if t >= 1 and any(p != w for w, p in enumerate(parents)) and sorted(parents) == list(range(W)):
            self.events["swap"] += 1                    # a permutation that moves something: no launch may read what it writes
        if t >= 1 and len(set(parents)) < W:
            self.events["fanout"] += 1
        self.records.append([dict(parent=c["b"], tok=c["tok"], lp=c["lp"], cum=c["score"]) for c in live])
        self.hist = [(self.hist[c["b"]][0] + [c["tok"]], self.hist[c["b"]][1] + [c["lp"]]) for c in live]
        self.cum = [c["score"] for c in live]
        self.n_steps = t + 1
        if len(self.pool) >= W:
            self.done = 1
        elif self.n_steps >= self.max_new:
            self.done = 2

    def completed_pool(self) -> List[dict]:
        pool = [dict(tokens=h["tokens"], token_logprobs=h["token_logprobs"], sum_logprob=float(h["score"]), finished=True,
                     finish_reason=h["finish_reason"]) for h in self.pool]
        for w in range(len(self.hist)):
            if len(pool) >= self.W or self.n_steps == 0:
                break
            pool.append(dict(tokens=list(self.hist[w][0]), token_logprobs=list(self.hist[w][1]), sum_logprob=float(self.cum[w]),
                             finished=False, finish_reason="length"))
        return pool

    def fin_tok(self) -> List[int]:
        return [h["tok"] for h in self.pool] + [-1] * (self.W - len(self.pool))
