"""Host model of beam search under a stop set (include/dualhyp_hip.h, "Stop conditions"): tests/beam_reference.py's utterance with one
change — a candidate whose id is in the stop set ends its hypothesis into the pool exactly as the EOS does (place rule, score, pool
order), and the pool entry remembers the id.  A stopped hypothesis keeps that id in its tokens; one that met the EOS does not."""
from typing import Iterable, List, Optional

import beam_reference as R


class StopUtterance(R.Utterance):
    def __init__(self, W: int, max_new: int, eos_id: Optional[int] = None, stop_ids: Iterable[int] = ()) -> None:
        super().__init__(W, max_new, eos_id)
        self.stop_ids = set(int(t) for t in stop_ids)

    def ends(self, tok: int) -> bool:
        return (self.eos is not None and self.eos >= 0 and tok == self.eos) or tok in self.stop_ids

    def step(self, rows) -> None:
        if self.done:
            return
        W, t = self.W, self.n_steps
        live = []
        for p, c in enumerate(self.ordered(rows)[:2 * W]):
            if self.ends(c["tok"]):
                if p < W and len(self.pool) < W:
                    toks, lps = self.hist[c["b"]]
                    is_eos = self.eos is not None and c["tok"] == self.eos          # the EOS wins where an id is both
                    self.pool.append(dict(step=t, parent=c["b"], score=c["score"], lp=c["lp"], tok=c["tok"],
                                          tokens=list(toks) + ([] if is_eos else [c["tok"]]), token_logprobs=list(lps) + [c["lp"]],
                                          finished=True, finish_reason="eos" if is_eos else "stop"))
                continue
            live.append(c)
            if len(live) == W:
                break
        assert len(live) == W, "the test's rows leave W candidates that end nothing"
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
        """the ids that ended the pool entries, -1 behind them: BeamState.fin_tok of the utterance"""
        return [h["tok"] for h in self.pool] + [-1] * (self.W - len(self.pool))
