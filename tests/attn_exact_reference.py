"""Exact inputs and an fp64 reference for the forward attention kernels (CPU only; imports nothing from the package).

The inputs are chosen so that the result of causal GQA attention does not depend on summation order, tile size, split count or
exp accuracy, only on WHICH keys are attended and HOW OFTEN each is counted:

  keys     position j of a (slot, group) carries an integer weight w_j as two base-16 digits in two channels,
           k[c0] = sign * (|w_j| // 16), k[c0 + 1] = sign * (|w_j| % 16); every other channel is 0.  Two weight channel pairs:
           recency w_j = j in channels (0, 1), target w_j = -|j - t| in channels (2, 3), t drawn per (sequence, group).
  queries  q[c0] = 16 G, q[c0 + 1] = G with G = 2048 (or their negatives, or all zeros): the score is +- G * scale * w_j, and keys
           whose weights differ by 1 are G * scale >= 181 apart, so the loser's exp is 0 in fp32 and below 1e-78 in fp64: the
           softmax is one-hot and y is the winner's V row bit for bit.
  values   v[j][d] random integers in [-8, 8], rows pairwise distinct inside a (slot, group): any sum of them is exact in fp32.
  heads    the heads of a KV group cycle through four families, family = head_in_group % 4 (with fewer than four heads per group the
           cycle also advances with the group, so that a multi-head layout still holds every family):
             recency  + on (0, 1): the last visible key        primacy  - on (0, 1): key 0
             target   + on (2, 3): key min(t, last visible)    uniform  zeros: every visible key with p = 1, y = sum / n
  decoys   every cache position that is no real key -- behind the sequence, under the rows a call is about to append, in free
           slots -- holds a key that continues the recency weights (w_j = j: the highest scores of the slot), the same weight in the
           target channels (positive: above every real target weight) and its own distinct V row.  A kernel that reads one key too
           far, or the stale row and not the appended one, selects a decoy.

The reference is plain attention in fp64 with a per-(query, key) multiplicity (0 = masked), rounded to bf16 once.  Uniform heads can
differ from a kernel's fp32 S * (1 / n) or S / n only where the exact quotient sits on a bf16 rounding boundary: elements closer
than 2^-20 relative to a boundary are TIES, either bf16 neighbour is accepted there, and the builder asserts that at most 1 % of a
case's uniform elements are ties.  `compare` is the one set of checks both the GPU tests and the CPU mutants go through."""
import math

import torch

G_Q = 2048                      # query digit weight: powers of two stay exact in bf16, also after the in-kernel Q * 1/8 at hs 64
FAMILIES = ("recency", "primacy", "target", "uniform")
TIE_REL = 2.0 ** -20
TIE_SHARE_MAX = 0.01
LSE_ULPS, LSE_FLOOR = 4, 2.0 ** -22
V_MAX = 8

# the cases of tests/test_hip_attn_exact.py (lengths where the tile -> wave deal changes: 32 and 64 keys per tile / stage, 256 keys =
# one tile for each of the fused kernels' 8 waves, 512 = one for each of the split-KV kernel's 16)
PREFILL_LAYOUTS = ((64, 8, 1), (64, 6, 1), (128, 8, 2), (96, 4, 4))
DECODE_LAYOUTS = ((64, 8, 2), (64, 16, 1), (128, 8, 2), (96, 4, 4))
PACKED_LENS = (1, 31, 32, 33, 63, 64, 65, 130, 200)
CONT_POS0 = (1, 31, 32, 40, 63, 64, 65, 100)
CONT_QLEN = (1, 31, 33, 50)
DECODE_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 545, 576)
FUSED_LENS = DECODE_LENS + (255, 256, 257, 289)


def family_of(head_in_group: int, group: int, q_per_kv: int) -> int:
    return (head_in_group + (group if q_per_kv < 4 else 0)) % 4


def digits(w: torch.Tensor) -> torch.Tensor:
    """Integer weights [...] -> the two channel values [..., 2]."""
    a, s = w.abs(), torch.sign(w)
    return torch.stack([s * (a // 16), s * (a % 16)], dim=-1)


def attention_fp64(q, k, v, count, scale):
    """Plain GQA attention in fp64.  q [T, H, hs], k / v [G, S, hs], count [T, S] or [T, H, S]: how often query t counts key s
    (0 = masked).  -> y [T, H, hs] fp64, lse [T, H] fp64 (log of the counted sum of exp(score))."""
    T, H, hs = q.shape
    Gn = k.shape[0]
    qpk = H // Gn
    s = torch.einsum("tgqd,gsd->tgqs", q.double().view(T, Gn, qpk, hs), k.double()) * scale
    c = count.double()
    c = c[:, None, None, :] if c.dim() == 2 else c.view(T, Gn, qpk, -1)
    s = torch.where(c > 0, s, torch.full_like(s, -math.inf))
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - m) * c
    l = p.sum(-1, keepdim=True)
    y = torch.einsum("tgqs,gsd->tgqd", p, v.double()) / l          # normalised once, at the end: an exact sum stays exact
    return y.reshape(T, H, hs), (m + torch.log(l)).reshape(T, H)


def bf16_neighbours(x: torch.Tensor):
    """fp64 x -> (lo, hi, rel): the bf16 numbers around x (lo <= |x| <= hi, signed like x) and the relative distance of x to the
    rounding boundary between them (1 where x is 0)."""
    a = x.abs()
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** -120)))
    ulp = torch.exp2(e - 7)
    n = torch.floor(a / ulp)
    lo, hi = n * ulp, (n + 1) * ulp
    rel = ((a - (lo + hi) / 2).abs() / a.clamp_min(2.0 ** -120))
    rel = torch.where(a == 0, torch.ones_like(rel), rel)
    sg = torch.sign(x)
    return sg * lo, sg * hi, rel


def tie_mask(y64: torch.Tensor) -> torch.Tensor:
    return bf16_neighbours(y64)[2] < TIE_REL


def ulp32(x: torch.Tensor) -> torch.Tensor:
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


class Case:
    """One launch's worth of exact inputs.  seqs: (slot, cached, new, decode) per sequence: `cached` real keys are in the cache at
    positions 0 .. cached - 1; `new` tokens at cached .. cached + new - 1 arrive as qkv rows (each with a query at its position);
    decode: no new token, one query at position cached - 1.  Everything else in every slot is a decoy."""

    def __init__(self, name, hs, n_head, n_groups, seqs, s_max, n_slots, seed):
        self.name, self.hs, self.n_head, self.n_groups, self.s_max, self.n_slots = name, hs, n_head, n_groups, s_max, n_slots
        self.qpk = n_head // n_groups
        self.width = (n_head + 2 * n_groups) * hs
        self.scale = 1.0 / math.sqrt(hs)
        self.seqs = [tuple(s) for s in seqs]
        gen = torch.Generator().manual_seed(seed)
        Gn, S = n_groups, s_max
        assert S % 64 == 0 and S < 4096 and len({s[0] for s in self.seqs}) == len(self.seqs) <= n_slots
        self.family = torch.tensor([[family_of(h, g, self.qpk) for h in range(self.qpk)] for g in range(Gn)])      # [G, qpk]
        # ---- the world before the call: decoys everywhere, real keys at 0 .. cached - 1
        pos = torch.arange(S)
        self.world_wrec = pos.expand(n_slots, Gn, S).clone()
        self.world_wtgt = pos.expand(n_slots, Gn, S).clone()
        max_new = max(s[2] for s in self.seqs)
        self.world_v = self._distinct_rows(gen, n_slots, Gn, S + max_new)   # rows S .. of a (slot, group): the new tokens' values
        self.t = torch.zeros(len(self.seqs), Gn, dtype=torch.long)
        self.total = []
        for i, (slot, cached, new, decode) in enumerate(self.seqs):
            L = cached + new
            assert 1 <= L <= S and (new == 0) == bool(decode) and cached >= (1 if decode else 0)
            self.total.append(L)
            for g in range(Gn):
                # targets in every 32-key tile and on tile edges: first / last / middle / a random tile in turn, offset 0 / 31 / random
                n_t = (L - 1) // 32 + 1
                tile = (0, n_t - 1, n_t // 2, int(torch.randint(n_t, (1,), generator=gen)))[(i + g) % 4]
                off = (0, 31, int(torch.randint(32, (1,), generator=gen)))[(i // 4 + g) % 3]
                self.t[i, g] = min(tile * 32 + off, L - 1)
                self.world_wtgt[slot, g, :cached] = -(pos[:cached] - self.t[i, g]).abs()
        self.world_k = self._keys(self.world_wrec, self.world_wtgt)                                                   # [slots, G, S, hs]
        # ---- new tokens and queries
        self.new_k, self.new_v, self.q, self.q_pos = [], [], [], []
        fam_q = torch.zeros(4, hs, dtype=torch.float64)
        fam_q[0, 0], fam_q[0, 1] = 16 * G_Q, G_Q
        fam_q[1, 0], fam_q[1, 1] = -16 * G_Q, -G_Q
        fam_q[2, 2], fam_q[2, 3] = 16 * G_Q, G_Q
        q_one = fam_q[self.family.reshape(-1)]                                                                           # [H, hs]
        for i, (slot, cached, new, decode) in enumerate(self.seqs):
            p = torch.arange(cached, cached + new)
            wt = torch.stack([-(p - self.t[i, g]).abs() for g in range(Gn)])                                          # [G, new]
            self.new_k.append(self._keys(p.expand(Gn, new), wt))
            self.new_v.append(self.world_v[slot][:, S:S + new].clone())
            qp = torch.tensor([cached - 1]) if decode else p
            self.q_pos.append(qp)
            self.q.append(q_one.expand(len(qp), n_head, hs).clone())
        self.world_v = self.world_v[:, :, :S].contiguous()
        self.n_q = sum(len(p) for p in self.q_pos)
        self._final = None
        self._expected = None
        self._self_check()

    # ------------------------------------------------------------------ construction helpers
    def _distinct_rows(self, gen, a, b, n):
        return torch.randint(-V_MAX, V_MAX + 1, (a, b, n, self.hs), generator=gen).double()      # distinctness: _self_check

    def _keys(self, wrec, wtgt):
        k = torch.zeros(*wrec.shape, self.hs, dtype=torch.float64)
        k[..., 0:2] = digits(wrec).double()
        k[..., 2:4] = digits(wtgt).double()
        return k

    def final_cache(self):
        """Plain K and V [slots, G, S, hs] (fp64 integers) after the call's appends."""
        if self._final is None:
            k, v = self.world_k.clone(), self.world_v.clone()
            for i, (slot, cached, new, _) in enumerate(self.seqs):
                k[slot, :, cached:cached + new] = self.new_k[i]
                v[slot, :, cached:cached + new] = self.new_v[i]
            self._final = (k, v)
        return self._final

    def _self_check(self):
        exact = lambda x: torch.equal(x.bfloat16().double(), x)
        k, v = self.final_cache()
        assert exact(k) and exact(self.world_k) and exact(v) and exact(self.world_v) and all(exact(q) for q in self.q), "not exact in bf16"
        assert k.abs().max() < 256 and v.abs().max() <= V_MAX
        # exp(-G * scale) is 0 in fp32: a key one weight below the winner contributes nothing
        assert G_Q * self.scale >= 181 and torch.exp(torch.tensor(-G_Q * self.scale, dtype=torch.float32)).item() == 0.0
        for i, (slot, cached, new, _) in enumerate(self.seqs):
            for g in range(self.n_groups):
                # V rows pairwise distinct inside the (slot, group): the world (with the stale rows) and the new rows together
                rows = torch.cat([self.world_v[slot, g], self.new_v[i][g]])
                assert torch.unique(rows, dim=0).shape[0] == rows.shape[0], f"{self.name}: V rows of slot {slot} group {g} repeat"
                # the winner of every one-hot family is unique with a weight gap of at least 1 over each query's visible keys
                wrec = k[slot, g, :, 0] * 16 + k[slot, g, :, 1]
                wtgt = k[slot, g, :, 2] * 16 + k[slot, g, :, 3]
                for w in (wrec, -wrec, wtgt):
                    vis = torch.arange(self.s_max)[None, :] <= self.q_pos[i][:, None]
                    top = torch.where(vis, w[None, :], torch.full((1, 1), -math.inf, dtype=torch.float64)).topk(2, dim=1).values
                    assert (top[:, 0] - top[:, 1] >= 1).all(), f"{self.name}: no unique winner in slot {slot} group {g}"

    # ------------------------------------------------------------------ what the ops take
    def cos_sin(self):
        return torch.ones(self.s_max, self.hs, dtype=torch.bfloat16), torch.zeros(self.s_max, self.hs, dtype=torch.bfloat16)

    def _rows(self, q, k, v):
        """q [n, H, hs], k / v [G, n, hs] -> interleaved rows [n, (H + 2 G) hs] bf16: per group its q heads, then k, then v."""
        n = k.shape[1]
        r = torch.zeros(n, self.n_groups, self.qpk + 2, self.hs, dtype=torch.float64)
        if q is not None:
            r[:, :, :self.qpk] = q.view(n, self.n_groups, self.qpk, self.hs)
        r[:, :, self.qpk] = k.transpose(0, 1)
        r[:, :, self.qpk + 1] = v.transpose(0, 1)
        return r.view(n, self.width).bfloat16()

    def fill_rows(self):
        """(qkv, tok_slot, tok_pos): the world, every position of every slot, to be written through the cache-append op."""
        S = self.s_max
        qkv = torch.cat([self._rows(None, self.world_k[s], self.world_v[s]) for s in range(self.n_slots)])
        slot = torch.arange(self.n_slots, dtype=torch.int32).repeat_interleave(S)
        return qkv, slot, torch.arange(S, dtype=torch.int32).repeat(self.n_slots)

    def token_rows(self):
        """(qkv, tok_slot, tok_pos, seq_slot, q_start, q_len, kv_pos0) of the new tokens, packed in sequence order."""
        rows, slot, pos, meta, t0 = [], [], [], [], 0
        for i, (s, cached, new, _) in enumerate(self.seqs):
            rows.append(self._rows(self.q[i], self.new_k[i], self.new_v[i]))
            slot += [s] * new
            pos += list(range(cached, cached + new))
            meta.append((s, t0, new, cached))
            t0 += new
        i32 = lambda x: torch.tensor(x, dtype=torch.int32)
        m = list(zip(*meta))
        return torch.cat(rows), i32(slot), i32(pos), i32(m[0]), i32(m[1]), i32(m[2]), i32(m[3])

    def queries(self):
        """[n_q, H, hs] bf16, the queries in sequence order (rope is the identity, so these are also the rotated queries)."""
        return torch.cat(self.q).bfloat16()

    def seq_slot(self):
        return torch.tensor([s[0] for s in self.seqs], dtype=torch.int32)

    def kv_len(self):
        return torch.tensor(self.total, dtype=torch.int32)

    # ------------------------------------------------------------------ the reference
    def counts(self, i):
        """[n_q of sequence i, S]: 1 where the key is visible to the query (causal: key <= query position)."""
        return (torch.arange(self.s_max)[None, :] <= self.q_pos[i][:, None]).double()

    def reference(self, mutate=None):
        """fp64 y [n_q, H, hs] and lse [n_q, H] of the whole case.  mutate(i, q, k, v, count) -> (q, k, v, count) may distort
        sequence i's operands (the CPU mutants); None is the truth."""
        K, V = self.final_cache()
        ys, ls = [], []
        for i, (slot, *_r) in enumerate(self.seqs):
            q, k, v, c = self.q[i], K[slot], V[slot], self.counts(i)
            if mutate is not None:
                q, k, v, c = mutate(i, q, k, v, c)
            y, l = attention_fp64(q, k, v, c, self.scale)
            ys.append(y)
            ls.append(l)
        return torch.cat(ys), torch.cat(ls)

    def expected(self):
        """dict: y64, y (bf16), lo / hi (the bf16 neighbours of y64), tie (bool), lse (fp64), tie_share (of the uniform elements)."""
        if self._expected is None:
            y64, lse = self.reference()
            lo, hi, rel = bf16_neighbours(y64)
            tie = rel < TIE_REL
            uni = (self.family.reshape(-1) == 3)
            share = tie[:, uni].double().mean().item() if uni.any() else 0.0
            assert not tie[:, ~uni].any(), f"{self.name}: a one-hot head sits on a rounding boundary"
            assert share <= TIE_SHARE_MAX, f"{self.name}: {share:.3%} of the uniform quotients are ties"
            self._expected = dict(y64=y64, y=y64.bfloat16(), lo=lo.bfloat16(), hi=hi.bfloat16(), tie=tie, lse=lse, tie_share=share)
        return self._expected

    # ------------------------------------------------------------------ the checks
    def _where(self, row):
        t0 = 0
        for i, qp in enumerate(self.q_pos):
            if row < t0 + len(qp):
                return i, int(qp[row - t0])
            t0 += len(qp)
        raise IndexError(row)

    def _lookup(self, i, g, vec):
        """Which key of sequence i's slot holds this V row: its position among the final rows, 'stale j' among the rows the call
        overwrote, or None."""
        slot, cached, new, _ = self.seqs[i]
        K, V = self.final_cache()
        hit = (V[slot, g] == vec.double()[None, :]).all(dim=1).nonzero().flatten().tolist()
        if hit:
            j = hit[0]
            return f"key {j}" + (" (a decoy)" if j >= cached + new else "")
        hit = (self.world_v[slot, g, cached:cached + new] == vec.double()[None, :]).all(dim=1).nonzero().flatten().tolist()
        return f"the stale row under key {cached + hit[0]}" if hit else "no single key's row"

    def _winner(self, i, g, fam, p):
        return (p, 0, min(int(self.t[i, g]), p))[fam]

    def compare(self, y, lse=None, limit=6):
        """-> list of messages, empty when y [n_q, H * hs] bf16 (and lse [n_q, H] fp32) pass: torch.equal off the ties, either
        bf16 neighbour on them, lse within 4 fp32 ulps of the fp64 value (floor 2^-22)."""
        E = self.expected()
        y = y.detach().cpu().view(self.n_q, self.n_head, self.hs)
        ok = torch.where(E["tie"], (y == E["lo"]) | (y == E["hi"]), y == E["y"])
        bad = (~ok).any(dim=2)
        msgs = []
        if lse is not None:
            lse = lse.detach().cpu().double().view(self.n_q, self.n_head)
            gate = torch.maximum(LSE_ULPS * ulp32(E["lse"]), torch.tensor(LSE_FLOOR, dtype=torch.float64))
            bad_l = ~((lse - E["lse"]).abs() <= gate)          # NaN fails
        else:
            bad_l = torch.zeros_like(bad)
        n_bad = int((bad | bad_l).sum())
        for row, head in (bad | bad_l).nonzero().tolist():
            if len(msgs) >= limit:
                break
            i, p = self._where(row)
            slot, cached, new, _ = self.seqs[i]
            g, fam = head // self.qpk, int(self.family.reshape(-1)[head])
            at = (f"{self.name}: seq {i} (slot {slot}, kv_len {self.total[i]}, kv_pos0 {cached}) query position {p} head {head} "
                  f"(group {g}, {FAMILIES[fam]}, t = {int(self.t[i, g])})")
            if bad[row, head]:
                if fam == 3:
                    S = E["y64"][row, head] * (p + 1)
                    big = S.abs() >= 4
                    n_got = (S[big] / y[row, head].double()[big]).median().item() if big.any() else float("nan")
                    msgs.append(f"{at}: y is not sum / n of the {p + 1} visible keys; {int((~ok[row, head]).sum())} of {self.hs} elements "
                                f"differ, the output is the sum over about {n_got:.2f} keys")
                else:
                    msgs.append(f"{at}: y equals {self._lookup(i, g, y[row, head])}, should equal key {self._winner(i, g, fam, p)}")
            if bad_l[row, head]:
                msgs.append(f"{at}: lse {lse[row, head].item():.9g}, fp64 {E['lse'][row, head].item():.9g} "
                            f"({((lse[row, head] - E['lse'][row, head]).abs() / ulp32(E['lse'][row, head])).item():.1f} fp32 ulps)")
        if n_bad > len(msgs):
            msgs.append(f"{self.name}: {n_bad} (query, head) pairs fail in all")
        return msgs


# ---------------------------------------------------------------------- the cases
def _perm(n, n_slots, seed):
    return torch.randperm(n_slots, generator=torch.Generator().manual_seed(seed))[:n].tolist()


def prefill_packed_case(hs, n_head, n_groups, seed=1):
    """One packed call: every query's recency head selects its own position, so every key of every tile is selected once."""
    n_slots = len(PACKED_LENS) + 2                       # two free slots, filled with decoys like the rest
    slots = _perm(len(PACKED_LENS), n_slots, seed)
    return Case(f"prefill packed hs{hs} {n_head}/{n_groups}", hs, n_head, n_groups, [(s, 0, n, False) for s, n in zip(slots, PACKED_LENS)],
                256, n_slots, seed)


def prefill_continuation_case(hs, n_head, n_groups, seed=2):
    """Chunks behind cached keys: unaligned mask starts, chunks that end inside a 64-key tile, q_len below the 32-query tile."""
    pairs = [(p0, n) for p0 in CONT_POS0 for n in CONT_QLEN]
    n_slots = len(pairs) + 1
    slots = _perm(len(pairs), n_slots, seed)
    return Case(f"prefill continuation hs{hs} {n_head}/{n_groups}", hs, n_head, n_groups,
                [(s, p0, n, False) for s, (p0, n) in zip(slots, pairs)], 256, n_slots, seed)


def decode_case(hs, n_head, n_groups, seed=3):
    n = len(DECODE_LENS)
    slots = list(range(n))[::-1]                        # a reversed permutation; slot n stays free
    return Case(f"decode hs{hs} {n_head}/{n_groups}", hs, n_head, n_groups, [(s, L, 0, True) for s, L in zip(slots, DECODE_LENS)], 640, n + 1, seed)


def fused_case(hs, n_head, n_groups, seed=4):
    """The single-token step: kv_len - 1 cached keys, the new token (its q, k, v) in the call, a stale decoy under it."""
    n = len(FUSED_LENS)
    slots = list(range(n))[::-1]
    return Case(f"fused step hs{hs} {n_head}/{n_groups}", hs, n_head, n_groups, [(s, L - 1, 1, False) for s, L in zip(slots, FUSED_LENS)], 640, n + 1, seed)
