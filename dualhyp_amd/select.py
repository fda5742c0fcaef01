"""Selection among the sampled candidates of one utterance (generate.sample_batch): host only, plain Python.

select(candidates, texts, how) returns (the chosen index, every candidate's selection key).  how:
  avg_logprob   the highest avg_logprob; ties go to the lower index.  The key is the value.
  sum_logprob   likewise on sum_logprob.
  mbr           minimum Bayes risk under word edit distance, every other sample standing in as a reference: candidate i's risk is
                    sum_{j != i} edits(ref = words_j, hyp = words_i) / max(1, sum_{j != i} len(words_j)),
                edits = substitutions + deletions + insertions of wer.edit_counts, words = wer's post-normalisation (lower case,
                without . , - ? ') split on whitespace.  Equal texts stay separate samples — that is how agreement counts.  The
                lowest risk wins; ties go to the higher avg_logprob, then to the lower index.  The key is the risk.
A candidate whose score is not finite (NaN, an infinity, None) ranks last under the two log-probability rules, and loses an mbr tie
to every finite one.
"""
from __future__ import annotations

import math
from typing import Any, List, Mapping, Optional, Sequence, Tuple

from .wer import _words, edit_counts, post_normalize

HOW = ("avg_logprob", "sum_logprob", "mbr")


def words(text: str) -> List[str]:
    """The words the risk is counted on: wer.post_normalize, then wer's whitespace split."""
    return _words(post_normalize(text))


def _score(v: Any) -> float:
    """A score to maximise; whatever is not a finite number ranks last."""
    try:
        v = float(v)
    except (TypeError, ValueError):
        return -math.inf
    return v if math.isfinite(v) else -math.inf


def mbr_risks(texts: Sequence[str]) -> List[float]:
    """risk[i] of the definition above for every text."""
    w = [words(t) for t in texts]
    risks = []
    for i in range(len(w)):
        errors = sum(sum(edit_counts(w[j], w[i])) for j in range(len(w)) if j != i)
        risks.append(errors / max(1, sum(len(w[j]) for j in range(len(w)) if j != i)))
    return risks


def select(candidates: Sequence[Mapping[str, Any]], texts: Optional[Sequence[str]], how: str) -> Tuple[int, List[float]]:
    """(index of the chosen candidate, the selection key of every candidate).  candidates: dicts with 'avg_logprob' and
    'sum_logprob' (sample_batch's); texts: their decoded answers, needed by 'mbr' only."""
    if how not in HOW:
        raise ValueError(f"select: how is one of {', '.join(HOW)}, not {how!r}")
    n = len(candidates)
    if n == 0:
        raise ValueError("select: no candidates")
    if how == "mbr":
        if texts is None or len(texts) != n:
            raise ValueError(f"select: mbr needs one text per candidate ({n}), got {None if texts is None else len(texts)}")
        keys = mbr_risks(texts)
        best = min(range(n), key=lambda i: (keys[i], -_score(candidates[i].get("avg_logprob")), i))
        return best, keys
    keys = [candidates[i].get(how) for i in range(n)]
    best = min(range(n), key=lambda i: (-_score(keys[i]), i))
    return best, keys
