"""Host side of beam search (generate.beam_search_batch): the argument checks, the device state of a call, and what the host does
with the device's per-step records — backtracking, completing the pool and ranking it.

The selection itself runs on the device (dh_beam_select_bf16; include/dualhyp_hip.h, "Beam search", is the definition and
tests/beam_reference.py its host model).  Histories are never gathered there: a step records, per live beam, the token, the beam of
the step before that it continues, the token's log-probability and the cumulative score; a hypothesis is read off backwards.  With history="device" the device keeps
the live beams' tokens as well (BeamState.history_buffer(); "Beam histories" of the header), for its own ban and stop-sequence tests;
the host still reads hypotheses off the records.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch

MAX_BEAMS = 4             # DH_MAX_BEAMS: a row offers 2 W <= DH_MAX_TOP_LOGPROBS candidates
MAX_BEAM_ROWS = 2048      # the streaming single-token step's row limit (engine.hip MAX_DECODE_ROWS)

MAX_BEAM_TILES = 64       # DH_MAX_BEAM_TILES: tiles per row of a tile table
KV_MODES = ("copy", "table")        # beam_search_batch(kv=), --beam_kv

HISTORIES = ("host", "device")      # beam_search_batch(history=), --beam_history
# the closing clause of the two refusals that device histories lift (no_repeat_ngram, stop sequences)
HISTORY_HINT = '; history="device" (--beam_history device) keeps the beams\' histories on the device and lifts this'

_I32 = ("n_steps", "done", "n_fin", "fin_step", "fin_parent", "beam_tok", "beam_parent")
_F32 = ("cum", "fin_score", "fin_lp", "beam_lp", "beam_cum")


def check_arguments(model, num_beams, n_utt: int) -> int:
    """W of a beam_search_batch call, or a ValueError that says why this call cannot run.  Nothing here touches the GPU."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= MAX_BEAMS:
        raise ValueError(f"num_beams is the number of beams per utterance, 1..{MAX_BEAMS}, not {num_beams!r}")
    W = num_beams
    if n_utt * W > MAX_BEAM_ROWS:
        raise ValueError(f"num_beams={W}: {n_utt} utterances x {W} beams exceed the {MAX_BEAM_ROWS} rows of a streaming decode step")
    if model.config.padded_vocab_size < 2 * W:
        raise ValueError(f"num_beams={W}: a row offers 2 W = {2 * W} candidates, the vocabulary has {model.config.padded_vocab_size}")
    from .relprompt import GPT as RelGPT
    if getattr(model, "fp8", False) or getattr(model, "kv_cache_dtype", "bf16") == "fp8":
        raise ValueError(f"num_beams={W}: an fp8 model's decode step changes its GEMM kernel with the row count, so a beam's bits would "
                         "depend on the beams beside it; beam search runs on bf16 engines")
    if isinstance(model, RelGPT):
        raise ValueError(f"num_beams={W}: the RelPrompt decoder's prompts carry spliced reliability embeddings")
    if model.cpu_rsqrt_vec_width != 0:
        raise ValueError(f"num_beams={W}: cpu_rsqrt_vec_width != 0 flags rows by their index within a call; a beam step has other rows")
    return W


def beam_tiles(max_new: int, s_max: int) -> int:
    """NT of a tile table: the 32-key tiles that the keys of max_new generated tokens can span, wherever in a tile the prompt ends,
    held to the tiles of a cache of s_max positions (the engine's beam_tiles)."""
    return min((int(max_new) + 30) // 32 + 1, int(s_max) // 32)


def check_kv(kv, W: int, shared_prompt: bool, flag: str = 'kv="table"', needs: str = "shared_prompt=True") -> str:
    """kv of a beam_search_batch call ("copy" or "table"), or a ValueError that says why "table" cannot run."""
    if kv not in KV_MODES:
        raise ValueError(f'kv is "copy" or "table", not {kv!r}')
    if kv == "table":
        if W < 2:
            raise ValueError(f"{flag} names, per tile, the sibling beam whose KV slot holds it; num_beams={W} has no sibling (it needs "
                             "num_beams >= 2)")
        if not shared_prompt:
            raise ValueError(f"{flag} reads the beams' private tiles inside the shared-prompt attention kernel; it needs {needs}")
    return kv


def resolve_slot(plane, row: int, pos: int, prompt_len: int, W: int) -> int:
    """The KV slot that holds position `pos` of row `row`'s hypothesis under a tile table plane ("Beam KV tile table" of the header):
    plane is [rows][NT] (nested lists or a CPU tensor).  A position in a whole prompt tile is read from slot u * W; a tile at or beyond
    NT, like an entry outside 0 .. W-1 once clamped, from what the attention kernel reads."""
    u, tile0, tile = row // W, prompt_len >> 5, pos >> 5
    if tile < tile0:
        return u * W
    j = tile - tile0
    if j >= len(plane[row]):
        return row
    return u * W + min(max(int(plane[row][j]), 0), W - 1)


def check_length_penalty(length_penalty) -> float:
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or length_penalty != length_penalty:
        raise ValueError(f"length_penalty is a number, not {length_penalty!r}")
    return float(length_penalty)


class BeamState:
    """dh_beam_state of one call: n_utt utterances, W beams, max_new steps.  Two zeroed device blocks (int32, float32), the arrays
    are views into them, so the whole state comes back with two copies (host())."""

    def __init__(self, n_utt: int, W: int, max_new: int, device) -> None:
        assert n_utt > 0 and 1 <= W <= MAX_BEAMS and max_new > 0
        self.n_utt, self.W, self.max_new, self.device = n_utt, W, max_new, torch.device(device)
        shapes = dict(n_steps=(n_utt,), done=(n_utt,), n_fin=(n_utt,), fin_step=(n_utt, W), fin_parent=(n_utt, W),
                      beam_tok=(n_utt, max_new, W), beam_parent=(n_utt, max_new, W), cum=(n_utt, W), fin_score=(n_utt, W),
                      fin_lp=(n_utt, W), beam_lp=(n_utt, max_new, W), beam_cum=(n_utt, max_new, W))
        self.shapes = shapes
        self._blocks = {}
        for names, dtype in ((_I32, torch.int32), (_F32, torch.float32)):
            sizes = [int(torch.Size(shapes[n]).numel()) for n in names]
            block = torch.zeros(sum(sizes), dtype=dtype, device=self.device)
            self._blocks[dtype] = block
            for n, v in zip(names, block.split(sizes)):
                setattr(self, n, v.view(shapes[n]))
        self._c = None
        self.fin_tok = None         # int32 [n_utt, W] beside fin_step, under a stop set only: the id that ended pool entry k
        self.history = None         # int64 [2, n_utt, W, max_new], under device histories only (history_buffer)
        self.tiles = None           # int32 [2, n_utt, W, NT], under a tile table only (tile_table)

    def fin_tok_buffer(self) -> torch.Tensor:
        """fin_tok, made at its first use (-1: no entry): what dh_beam_select_bf16_stop and dh_engine_set_stop write."""
        if self.fin_tok is None:
            self.fin_tok = torch.full((self.n_utt, self.W), -1, dtype=torch.int32, device=self.device)
        return self.fin_tok

    def history_buffer(self) -> torch.Tensor:
        """The history planes, made at their first use: int64 [2, n_utt, W, max_new], plane t & 1 holding the live beams' tokens behind
        step t ("Beam histories" of the header): what dh_beam_select_bf16_hist and dh_engine_set_beam_history read and write."""
        if self.history is None:
            self.history = torch.zeros((2, self.n_utt, self.W, self.max_new), dtype=torch.int64, device=self.device)
        return self.history

    def tile_table(self, n_tiles: int) -> torch.Tensor:
        """The tile table, made at its first use: int32 [2, n_utt, W, n_tiles], both planes the identity ([.., w, j] = w); plane
        t & 1 names, behind step t, the sibling whose slot holds each tile of a row's hypothesis ("Beam KV tile table" of the header):
        what dh_engine_set_beam_tiles takes."""
        if self.tiles is None:
            assert 1 <= n_tiles <= MAX_BEAM_TILES
            w = torch.arange(self.W, dtype=torch.int32, device=self.device)
            self.tiles = w.view(1, 1, self.W, 1).expand(2, self.n_utt, self.W, n_tiles).contiguous()
        assert self.tiles.size(3) == n_tiles
        return self.tiles

    def c_struct(self):
        from . import _lib
        if self._c is None:
            self._c = _lib.BeamState(**{n: getattr(self, n).data_ptr() for n, _ in _lib.BeamState._fields_})
        return self._c

    def host(self) -> Dict[str, list]:
        """Every array as nested Python lists: two device-to-host copies (the first synchronises the stream)."""
        out = {}
        for names, dtype in ((_I32, torch.int32), (_F32, torch.float32)):
            block = self._blocks[dtype].cpu()
            sizes = [int(torch.Size(self.shapes[n]).numel()) for n in names]
            for n, v in zip(names, block.split(sizes)):
                out[n] = v.view(self.shapes[n]).tolist()      # a Python float holds an fp32 value exactly
        if self.fin_tok is not None:                          # a call under a stop set: one small copy more
            out["fin_tok"] = self.fin_tok.tolist()
        if self.history is not None:                          # device histories: per utterance the plane its last step wrote,
            planes = self.history.cpu()                       # [W][max_new], the first n_steps ids of a row are the beam's tokens
            out["history"] = [planes[(int(n) - 1) & 1, u].tolist() for u, n in enumerate(out["n_steps"])]
        if self.tiles is not None:                            # a tile table: per utterance the plane its last step wrote, [W][NT]
            planes = self.tiles.cpu()
            out["tiles"] = [planes[(int(n) - 1) & 1, u].tolist() for u, n in enumerate(out["n_steps"])]
        return out


def backtrack(beam_parent, step: int, beam: int) -> List[int]:
    """The live beams a hypothesis went through: path[t] is its beam index at step t, t = 0 .. step, for the hypothesis that is live
    beam `beam` at step `step`.  beam_parent[t][w] is the beam of step t - 1 that beam w of step t continues."""
    path = [0] * (step + 1)
    b = int(beam)
    for t in range(step, -1, -1):
        path[t] = b
        b = int(beam_parent[t][b])
    return path


def hypotheses(h: Dict[str, list], u: int, W: int, length_penalty: float = 1.0, eos_id=None) -> List[dict]:
    """The ranked hypotheses of utterance u from the host copy `h` of a finished call's state (BeamState.host()): the pool, completed
    with the live beams in live order (unfinished) while it holds fewer than W entries, ranked by sum_logprob / n ** length_penalty
    in Python floats — n the generated tokens, the EOS counted — descending, stable on pool order.  Each entry: tokens (generated,
    without the EOS), token_logprobs (float32 tensor, the EOS's included), sum_logprob (the device's fp32 cumulative score, as a
    float), finished, and finish_reason: "eos" for a pool entry that ended on the EOS, "stop" for one that ended on a stop id (h holds
    fin_tok then — a call under a stop set — and the id differs from eos_id; the stop id stays in tokens and counts in n), "length" for
    a live beam."""
    n_steps, n_fin = int(h["n_steps"][u]), int(h["n_fin"][u])
    tok, par, lp = h["beam_tok"][u], h["beam_parent"][u], h["beam_lp"][u]
    pool = []

    def read(step, beam):
        path = backtrack(par, step, beam) if step >= 0 else []
        return [int(tok[t][b]) for t, b in enumerate(path)], [lp[t][b] for t, b in enumerate(path)]

    for i in range(min(n_fin, W)):
        s = int(h["fin_step"][u][i])
        toks, lps = read(s - 1, int(h["fin_parent"][u][i]))
        reason = "eos"
        if "fin_tok" in h and (eos_id is None or int(h["fin_tok"][u][i]) != int(eos_id)):     # the EOS wins where an id is both
            reason = "stop"
            toks = toks + [int(h["fin_tok"][u][i])]
        pool.append(dict(tokens=toks, token_logprobs=torch.tensor(lps + [h["fin_lp"][u][i]], dtype=torch.float32),
                         sum_logprob=float(h["fin_score"][u][i]), finished=True, finish_reason=reason))
    for w in range(W):
        if len(pool) >= W or n_steps == 0:
            break
        toks, lps = read(n_steps - 1, w)
        pool.append(dict(tokens=toks, token_logprobs=torch.tensor(lps, dtype=torch.float32), sum_logprob=float(h["beam_cum"][u][n_steps - 1][w]), finished=False,
                         finish_reason="length"))
    return rank(pool, length_penalty)


def rank(pool: Sequence[dict], length_penalty: float = 1.0) -> List[dict]:
    """pool ordered by sum_logprob / n ** length_penalty, n = len(token_logprobs), descending, stable on pool order (sorted with
    reverse=True keeps equal elements in their original order)."""
    def key(hyp):
        return hyp["sum_logprob"] / float(max(len(hyp["token_logprobs"]), 1)) ** float(length_penalty)
    return sorted(pool, key=key, reverse=True)
