"""Plain-Python model of the beam KV tile table (include/dualhyp_hip.h, "Beam KV tile table"): the table update behind a selection,
the resolution of a (row, position) to the slot that holds it, and a toy cache — slot -> tile -> 32 keys — on which the re-parenting
copy and the table scheme run side by side.  Nothing here imports the package: the tests compare the package's helpers and the
device's planes with it."""
from __future__ import annotations

import copy
from typing import List, Optional, Sequence, Tuple

TILE = 32


def n_tiles(max_new: int, s_max: int) -> int:
    """NT: the tiles that the keys of max_new generated tokens can span, wherever in a tile the prompt ends, held to the cache."""
    return min((max_new + 30) // 32 + 1, s_max // 32)


def identity(n_utt: int, W: int, NT: int) -> List[List[List[int]]]:
    """Both planes [2][n_utt * W][NT] as they start: entry [r][j] = w."""
    return [[[r % W] * NT for r in range(n_utt * W)] for _ in range(2)]


def update(planes, t: int, u: int, W: int, P: int, parents: Optional[Sequence[int]]) -> List[Tuple[int, int, int]]:
    """The update behind the selection of step t >= 1 for utterance u, in place: plane t & 1 from plane (t - 1) & 1.  parents[w] is
    beam_parent[u, t, w]; None: the utterance did not take the step and its rows move over unchanged.  Returns the tile copies that go
    with it, (destination row, source row, absolute tile), all read before any is written."""
    old, new = planes[(t - 1) & 1], planes[t & 1]
    NT = len(old[0])
    if parents is None:
        for w in range(W):
            new[u * W + w] = list(old[u * W + w])
        return []
    tile0 = P >> 5
    cur, nxt = ((P + t - 1) >> 5) - tile0, ((P + t) >> 5) - tile0
    rows, copies = [], []
    for w in range(W):
        p = parents[w]
        row = [w] * NT
        for j in range(min(cur, NT)):
            row[j] = old[u * W + p][j]
        if cur < NT:
            row[cur] = w if nxt == cur else p
        if nxt == cur and p != w:
            copies.append((u * W + w, u * W + p, tile0 + cur))
        rows.append(row)
    for w in range(W):
        new[u * W + w] = rows[w]
    return copies


def resolve(plane, row: int, pos: int, P: int, W: int) -> int:
    """The slot that holds position pos of row's hypothesis: slot u * W for a whole prompt tile, else the sibling the plane names."""
    u, tile0, tile = row // W, P >> 5, pos >> 5
    if tile < tile0:
        return u * W
    j = tile - tile0
    if j >= len(plane[row]):
        return row
    return u * W + min(max(plane[row][j], 0), W - 1)


class ToyCache:
    """slot -> tile -> 32 keys (None: never written) of ONE utterance's W slots.  A key is any hashable value."""

    def __init__(self, W: int, tiles: int) -> None:
        self.W, self.tiles = W, tiles
        self.slot = [[[None] * TILE for _ in range(tiles)] for _ in range(W)]

    def write(self, w: int, pos: int, key) -> None:
        self.slot[w][pos >> 5][pos & 31] = key

    def read(self, w: int, pos: int):
        return self.slot[w][pos >> 5][pos & 31]

    def copy_tiles(self, moves: Sequence[Tuple[int, int, int]]) -> None:
        """(destination beam, source beam, tile) moves, every source read before any destination is written (the scratch)."""
        held = [(d, t, list(self.slot[s][t])) for d, s, t in moves]
        for d, t, keys in held:
            self.slot[d][t] = keys


def simulate(W: int, P: int, parent_seq: Sequence[Optional[Sequence[int]]], NT: int, check) -> dict:
    """One utterance under both schemes.  Step 0 is the caller's (every beam continues the prompt); parent_seq[t - 1] is the parent map
    of step t = 1, 2, ... or None from the step at which the utterance stops taking steps (it stays None from there on).  At every
    step `check(t, copy_cache, table_cache, planes, n_steps)` is called behind the update.  Returns the counts of what happened."""
    tiles = ((P + len(parent_seq) + 1) >> 5) + 1
    cc, tc = ToyCache(W, tiles), ToyCache(W, tiles)
    for w in range(W):
        for i in range(P):
            cc.write(w, i, ("p", i))
            tc.write(w, i, ("p", i))
    planes = identity(1, W, NT)
    tile0 = P >> 5
    n_steps = 1                                  # step 0 is taken
    stats = dict(open_copies=0, closed_reads=0, frozen_steps=0)
    for t, parents in enumerate(parent_seq, start=1):
        took = parents is not None
        # the step's attention: row w appends the key of beam w of the step before (a frozen row: the same key at the same place again)
        pos = P + (t if took else n_steps) - 1
        for w in range(W):
            key = ("g", pos - P, w)
            cc.write(w, pos, key)
            tc.write(w, pos, key)
        rd = planes[(t - 1) & 1]
        for w in range(W):                       # what the attention reads: the same keys under either scheme
            for i in range(pos + 1):
                s = resolve(rd, w, i, P, W)
                assert tc.read(s, i) == cc.read(w, i), (t, w, i, s)
                if (i >> 5) >= tile0 and s != w:
                    stats["closed_reads"] += 1
        if took:
            last = (P + t - 1) >> 5
            cc.copy_tiles([(w, p, tl) for w, p in enumerate(parents) if p != w for tl in range(tile0, last + 1)])
            n_steps = t + 1
        else:
            stats["frozen_steps"] += 1
        moves = update(planes, t, 0, W, P, parents)
        tc.copy_tiles([(d, s, tl) for d, s, tl in moves])
        stats["open_copies"] += len(moves)
        check(t, cc, tc, planes, n_steps)
    return stats


def text(cache: ToyCache, plane, w: int, P: int, n: int, W: int) -> list:
    """positions 0 .. n - 1 of row w's hypothesis read through a plane (None: the row's own slot)"""
    return [cache.read(w if plane is None else resolve(plane, w, i, P, W), i) for i in range(n)]


def clone(planes):
    return copy.deepcopy(planes)
