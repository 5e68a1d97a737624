"""Helpers of the exact attention parity tests (test_attn_exact_host.py, test_gpu_attn_exact.py). Torch only, no GPU needed.

The idea: the attention ops take the query columns pre-scaled into the exp2 domain (test_gpu_ops._attn_prescale), so a test
may choose q_hat itself. Here q_hat and k hold small integers such that every score q_hat . k is one of -512, -256, 0, 256,
512, and for every (row, head) the visible maximum is attained by exactly 1, 2 or 4 keys (the row's TIE SET) while every
other visible key scores at least 256 lower: its weight 2^-256 is zero in fp32 and in bf16 under any exp2, any rescale order
and any packing. The true function is then P = 2^-a on the tie set, o = a mean of 1, 2 or 4 integer rows of v,
lse2 = max + a, dS = 2^-a (x_j - mean x) with x_j = dO_i . v_j, dv_j = sum of 2^-a dO_i over the rows whose tie set holds j.
Every value a bf16-MFMA flash kernel rounds on the way (P, O, dS) is a bf16 number, so the stored bf16 o, dv and (at head_dim
64, whose only factor is 1/8) dq must equal the bf16 rounding of an fp64 reference BIT FOR BIT; dk carries one rounding by
LN2 and dq at head_dim 128 one by 1/sqrtf(128): one bf16 ulp.

The adversarial part: the code a row's tie set shares is also carried by the key just behind the diagonal (key i + 1) and by
the last key of the previous segment (key seg_start - 1). One leaked key turns a weight 1/2^a into 1/(2^a + 1).

Codes. H = the 32 x 32 Hadamard matrix. Code c = (s1, s2, a < 16, b < 16) is the 64-vector [s1 H[a], s2 H[b]], s = +-1: two
codes score 64 when all four agree and at most 32 otherwise (1024 codes). A key is its code plus +-H[r] +- H[r'], 16 <= r, r'
< 32, in each half: no query has a component there, so the scores do not see it, but tied keys differ as vectors (without it
dq = sum_j dS_ij k_j = k sum_j dS_ij = 0 identically). A query is 8 x its code. At head_dim 128 the 64 columns are repeated
and the query is 4 x its code: the same scores.

make_case builds the codes SEQUENTIALLY, keeping per KV head and segment the count of every code as the row index advances:
  * key s of a segment (s > 0) copies the code of key s - 1 on every KV head: the segment-start shadow of all rows of the
    segment. That code is then left alone in this segment (its count stays 1, or 2 where the next rule forces a copy of it).
  * keys of COPY parity (odd keys on even KV heads, even keys on odd ones; `flip` swaps the parities - a single KV head takes
    two cases, flip 0 and 1) copy a code whose count in the window of the row before them is 1, 2 or 4: the diagonal shadow
    of that row. The key before a copy key is of the other parity and new, so such a code always exists.
  * keys of the other parity take a code the segment has not seen, or now and then raise a code of count 3 to 4.
  * per row, one head of a KV group whose key i + 1 is a copy takes that key's code, one head takes the code of key
    seg_start - 1, every other head takes a code with 2 or 4 visible members (1 where none exists) that has a member in a
    key tile the row's 16-row fragment has not linked to yet.
check_conditions proves the six conditions of the case on the finished tensors alone (scores, not the bookkeeping)."""
import random
from types import SimpleNamespace

import torch

LOG2E = 1.4426950408889634
GAP = 160           # every non-tied visible key scores at least this much lower (2^-160 < the smallest fp32 and bf16 denormal)
GUARD = 128         # rows of a NaN / sentinel band
NCODE = 1024
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _hadamard(n):
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


H32 = _hadamard(32)


def code_vectors(ids):
    """int64 [...] code ids (sign 1, sign 2, a, b: 1 + 1 + 4 + 4 bits) -> fp64 [..., 64]."""
    s1, s2 = (1 - 2 * ((ids >> 9) & 1)).double(), (1 - 2 * ((ids >> 8) & 1)).double()
    return torch.cat([s1[..., None] * H32[(ids >> 4) & 15], s2[..., None] * H32[ids & 15]], -1)


def key_extras(M):
    """fp64 [M][64]: per key, +-H[r] +- H[r'] (16 <= r != r' < 32) in each half. Queries live on H[0..15], so no score sees
    it; it makes tied keys differ in (nearly) every column, and every key element odd (-3, -1, 1, 3)."""
    j = torch.arange(M)
    halves = []
    for t in range(2):
        r = (5 * j + 3 * t + j // 16) % 16
        r2 = (r + 1 + (j // 7 + t) % 15) % 16
        sa, sb = 1 - 2 * ((j // 3 + t) % 2), 1 - 2 * ((j // 5 + j // 16) % 2)
        halves.append(sa.double()[:, None] * H32[16 + r] + sb.double()[:, None] * H32[16 + r2])
    return torch.cat(halves, -1)


def seg_tables(seg_lens):
    starts, ends, s = [], [], 0
    for n in seg_lens:
        starts += [s] * n
        ends += [s + n] * n
        s += n
    return torch.tensor(starts, dtype=torch.int32), torch.tensor(ends, dtype=torch.int32)


def bf16_round(t):
    return t.to(F32).to(BF16).double()


def is_bf16(t):
    return bool((bf16_round(t) == t).all())


# ------------------------------------------------------------------------------------------------ the generator
class _Window:
    """Codes of one KV head inside the current segment: count and member keys per code, lazily cleaned pools per count."""

    def __init__(self, rng, first_fresh):
        self.rng, self.next_fresh = rng, first_fresh
        self.reset(None)

    def reset(self, reserved):
        self.cnt, self.mem, self.pool, self.reserved = {}, {}, {1: [], 2: [], 3: [], 4: []}, reserved
        self.copies = self.news = 0

    def add(self, key, code):
        n = self.cnt.get(code, 0) + 1
        self.cnt[code] = n
        self.mem.setdefault(code, []).append(key)
        if n <= 4:
            self.pool[n].append(code)

    def pick(self, n):
        """A random code of count n other than the reserved one, or None."""
        p = self.pool[n]
        while p:
            i = self.rng.randrange(len(p))
            c = p[i]
            if self.cnt.get(c) == n and c != self.reserved:
                return c
            p[i] = p[-1]
            p.pop()
        return None

    def fresh(self):
        assert len(self.cnt) < NCODE, "the segment has used every code"
        while True:
            c = self.next_fresh
            self.next_fresh = (c + 1) % NCODE
            if c not in self.cnt:
                return c


COPY_PLAN = (1, 2, 1, 2, 1, 4)   # count of the code a copy key raises, in turn: pairs, triples (to become fours), fives


def _codes(seg_lens, nH, nKV, seed, flip):
    """Key codes [nKV][M], query codes [M][nH] and the bookkeeping's tie sets {(row, head): keys} (python ints)."""
    M, G = sum(seg_lens), nH // nKV
    seg_s = seg_tables(seg_lens)[0].tolist()
    rng = random.Random(1000 * seed + flip)
    win = [_Window(rng, (seed * 131 + kv * 397) % NCODE) for kv in range(nKV)]
    kcode = [[0] * M for _ in range(nKV)]
    qcode = [[0] * nH for _ in range(M)]
    ties = {}

    def is_copy(key, kv):
        return (key + kv + flip) % 2 == 1

    for kv in range(nKV):
        kcode[kv][0] = win[kv].fresh()
        win[kv].add(0, kcode[kv][0])
    frag, linked = -1, set()
    for i in range(M):
        s = seg_s[i]
        # ---- the code of key i + 1, decided on the window of row i (it joins the window after row i's queries are chosen)
        if i + 1 < M:
            for kv in range(nKV):
                w = win[kv]
                if seg_s[i + 1] == i + 1:
                    c = kcode[kv][i]
                    assert not is_copy(i + 1, kv) or w.cnt[c] in (1, 2, 4), \
                        f"row {i} kv head {kv}: the code of the last key of segment {s} has {w.cnt[c]} visible members"
                elif is_copy(i + 1, kv):
                    want = COPY_PLAN[w.copies % len(COPY_PLAN)]
                    w.copies += 1
                    c = None
                    for n in (want, 1, 2, 4):
                        c = w.pick(n) if c is None else c
                    if c is None and w.cnt.get(w.reserved) in (1, 2, 4):
                        c = w.reserved
                    assert c is not None, f"row {i} kv head {kv}: no code with 1, 2 or 4 visible members to copy"
                else:
                    w.news += 1
                    c = w.pick(3) if w.news % 3 == 0 else None
                    c = w.fresh() if c is None else c
                kcode[kv][i + 1] = c
        # ---- the queries of row i
        if i // 16 != frag:
            frag, linked = i // 16, set()
        first_tile, last_tile = s // 64, i // 64
        diag_heads = [h for h in range(nH) if i + 1 < M and is_copy(i + 1, h // G)]
        d_head = diag_heads[i % len(diag_heads)] if diag_heads else -1
        rest = [h for h in range(nH) if h != d_head]
        rest = rest[i % len(rest):] + rest[: i % len(rest)] if rest else rest
        s_head = rest[0] if s > 0 and rest else -1
        for h in ([d_head] if d_head >= 0 else []) + rest:
            w = win[h // G]
            c = None
            if h == d_head:
                c = kcode[h // G][i + 1]
            elif h == s_head and w.cnt.get(w.reserved) in (1, 2, 4):
                c = w.reserved
            if c is None:  # a far code: 4 or 2 members (in turn) in a key tile this fragment has no link to yet
                tiles = [t for t in range(first_tile, last_tile + 1) if t not in linked]
                if not tiles:
                    tiles = list(range(first_tile, last_tile + 1))
                t = tiles[(i + h) % len(tiles)]
                lo, hi = max(s, 64 * t), min(i, 64 * t + 63)
                off = rng.randrange(hi - lo + 1)
                prefer = ((4,), (2,), (2, 4), (1,)) if (i + h) % 2 else ((2,), (4,), (2, 4), (1,))
                for ok in prefer:
                    for d in range(hi - lo + 1):
                        cand = kcode[h // G][lo + (off + d) % (hi - lo + 1)]
                        if w.cnt[cand] in ok:
                            c = cand
                            break
                    if c is not None:
                        break
                if c is None:  # the tile holds only codes of 3 or 5+ members: any usable code of the window
                    for n in (2, 4, 1):
                        c = w.pick(n) if c is None else c
                    if c is None and w.cnt.get(w.reserved) in (1, 2, 4):
                        c = w.reserved
            assert c is not None and w.cnt.get(c) in (1, 2, 4), f"row {i} head {h}: no code with 1, 2 or 4 visible members"
            qcode[i][h] = c
            ties[(i, h)] = tuple(w.mem[c])
            linked.update(k // 64 for k in w.mem[c])
        # ---- key i + 1 joins (a new segment starts with an empty window and its first key's code reserved)
        if i + 1 < M:
            for kv in range(nKV):
                if seg_s[i + 1] == i + 1:
                    win[kv].reset(kcode[kv][i + 1])
                win[kv].add(i + 1, kcode[kv][i + 1])
    return kcode, qcode, ties


def make_d_o(M, nH, hd, density, seed):
    """Sparse {-1, 0, 1}; every (row, head) keeps at least one non-zero (a row of zeros would hide its links from dv)."""
    g = torch.Generator().manual_seed(7000 + seed)
    d = (torch.randint(0, 2, (M, nH, hd), generator=g) * 2 - 1) * (torch.rand(M, nH, hd, generator=g) < density)
    empty = (d != 0).sum(-1) == 0
    r, h = torch.arange(M)[:, None], torch.arange(nH)[None, :]
    col, sign = ((7 * r + 13 * h) % hd).expand(M, nH), (1 - 2 * ((r + h) % 2)).expand(M, nH)
    d[empty, col[empty]] = sign[empty]
    return d.double().reshape(M, nH * hd)


def make_case(seg_lens, nH, nKV, hd, seed, flip=0):
    """The exact-attention case: .qkv_dev fp64 [M][(nH + 2 nKV) hd] (bf16-exact; query columns = q_hat), .qkv_ref (queries
    q_hat / c2: what the fp64 reference takes), .d_o [M][nH hd], .seg_start / .seg_end int32 [M], .ties {(row, head): keys},
    .tie_size int64 [M][nH], .exact = exact_values(...) of the finished case. Asserts its own conditions as far as the
    bookkeeping knows them; check_conditions proves all six on the tensors."""
    assert hd in (64, 128) and nH % nKV == 0
    M, rep = sum(seg_lens), hd // 64
    kcode, qcode, ties = _codes(seg_lens, nH, nKV, seed, flip)
    g = torch.Generator().manual_seed(100 + seed)
    k = code_vectors(torch.tensor(kcode).t().contiguous()) + key_extras(M)[:, None, :]   # [M][nKV][64]
    q = (8 // rep) * code_vectors(torch.tensor(qcode))              # [M][nH][64]
    v = torch.randint(-2, 3, (M, nKV, hd), generator=g).double()
    c = SimpleNamespace(seg_lens=list(seg_lens), nH=nH, nKV=nKV, hd=hd, seed=seed, flip=flip, M=M, ld=(nH + 2 * nKV) * hd)
    c.seg_start, c.seg_end = seg_tables(seg_lens)
    c.qkv_dev = torch.cat([q.repeat(1, 1, rep).reshape(M, -1), k.repeat(1, 1, rep).reshape(M, -1), v.reshape(M, -1)], 1)
    c.qkv_ref = c.qkv_dev.clone()
    c.qkv_ref[:, : nH * hd] /= hd ** -0.5 * LOG2E
    c.ties = ties
    c.tie_size = torch.tensor([[len(ties[(i, h)]) for h in range(nH)] for i in range(M)])
    for density in (1 / 8, 1 / 16):   # condition 6: thin d_o rather than accept a dS that bf16 cannot hold
        c.d_o, c.density = make_d_o(M, nH, hd, density, seed), density
        c.exact = exact_values(c)
        if c.exact.ds_is_bf16:
            break
    assert c.exact.ds_is_bf16, f"{describe(c)}: dS is not bf16-exact even at d_o density 1/16, first at {c.exact.ds_first_bad}"
    return c


def describe(c):
    lens = c.seg_lens if len(c.seg_lens) <= 10 else f"{c.seg_lens[:3]}..{c.seg_lens[-2:]} ({len(c.seg_lens)} segments)"
    return f"segments {lens} M={c.M} nH={c.nH} nKV={c.nKV} head_dim={c.hd} seed={c.seed} flip={c.flip}"


# ------------------------------------------------------------------------------------------------ exact arithmetic
def split_heads(c, x=None):
    x = c.qkv_dev if x is None else x
    a, b = c.nH * c.hd, (c.nH + c.nKV) * c.hd
    return (x[:, :a].reshape(c.M, c.nH, c.hd).transpose(0, 1), x[:, a:b].reshape(c.M, c.nKV, c.hd).transpose(0, 1),
            x[:, b:].reshape(c.M, c.nKV, c.hd).transpose(0, 1))


def visible(c):
    i = torch.arange(c.M)
    return (i[None, :] <= i[:, None]) & (i[None, :] >= c.seg_start.long()[:, None])


def exact_values(c, round_bf16=False, leak=(), drop=()):
    """The function on the device operands in the exp2 domain, in fp64: scores are integers, so every step is exact dyadic
    arithmetic. round_bf16: the roundings ANY bf16-MFMA flash kernel makes (P, O and dS to bf16 before their second
    products; test_gpu_attn_block._attn_emu64's idea, nothing of the code under test). leak: (row, key) pairs made visible
    in every head; drop: (16-row fragment, 64-key tile) pairs whose P and dS block is left out of the backward products - the two
    defects the host test plants. Returns o [M][nH hd], lse2 [M][nH], dq, dk, dv (dq without its head_dim^-0.5, dk without
    its ln 2: the dyadic parts) and whether every dS was a bf16 number."""
    q, k, v = split_heads(c)
    G, M, hd = c.nH // c.nKV, c.M, c.hd
    mask = visible(c).clone()
    for r, j in leak:
        mask[r, j] = True
    d_o = c.d_o.reshape(M, c.nH, hd).transpose(0, 1)
    rnd = bf16_round if round_bf16 else (lambda t: t)
    out = SimpleNamespace(o=torch.empty(M, c.nH, hd, dtype=F64), lse2=torch.empty(M, c.nH, dtype=F64),
                          dq=torch.empty(M, c.nH, hd, dtype=F64), dk=torch.zeros(M, c.nKV, hd, dtype=F64),
                          dv=torch.zeros(M, c.nKV, hd, dtype=F64), ds_is_bf16=True, ds_first_bad=None)
    for h in range(c.nH):
        kv = h // G
        s = (q[h] @ k[kv].t()).masked_fill(~mask, -float("inf"))
        mx = s.amax(-1, keepdim=True)
        pu = torch.exp2(s - mx)
        pu = torch.where(s - mx <= -GAP, torch.zeros_like(pu), pu)   # below every denormal of fp32 and bf16: zero on the device
        l = pu.sum(-1, keepdim=True)
        oh = (rnd(pu) @ v[kv]) / l
        p = pu / l
        ds = p * (d_o[h] @ v[kv].t() - (d_o[h] * rnd(oh)).sum(-1, keepdim=True))
        bad = bf16_round(ds) != ds
        if out.ds_is_bf16 and bool(bad.any()):
            r, j = [int(x) for x in bad.nonzero()[0]]
            out.ds_is_bf16, out.ds_first_bad = False, f"row {r} head {h} key {j}: dS = {float(ds[r, j])!r}"
        pb, dsb = rnd(p), rnd(ds)
        if drop:
            pb, dsb = pb.clone(), dsb.clone()
            for f, t in drop:
                pb[16 * f:16 * f + 16, 64 * t:64 * t + 64] = 0
                dsb[16 * f:16 * f + 16, 64 * t:64 * t + 64] = 0
        out.o[:, h], out.lse2[:, h] = oh, (mx + torch.log2(l))[:, 0]
        out.dq[:, h] = dsb @ k[kv]
        out.dk[:, kv] += dsb.t() @ q[h]
        out.dv[:, kv] += pb.t() @ d_o[h]
    for name in ("o", "dq", "dk", "dv"):
        setattr(out, name, getattr(out, name).reshape(M, -1))
    return out


def dq_factor(hd):
    """What the dQ kernel multiplies by: 1/8 (exact) or the fp32 number 1/sqrtf(128)."""
    return float(torch.tensor(1.0, dtype=F32) / torch.tensor(float(hd), dtype=F32).sqrt())


# ------------------------------------------------------------------------------------------------ the six conditions
def check_conditions(cases):
    """cases: the make_case results that share shape and heads (more than one where a single KV head needs both parities).
    Proves conditions 1-6 on the tensors, naming the first offending row; returns the figures the profile quotes."""
    c0 = cases[0]
    M, nH, G, hd = c0.M, c0.nH, c0.nH // c0.nKV, c0.hd
    vis = visible(c0)
    seg_s = c0.seg_start.long()
    rows = torch.arange(M)
    diag_ok, seg_ok = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
    nf, nt = (M + 15) // 16, (M + 63) // 64
    pair_vis = torch.zeros(nf, nt, dtype=torch.bool)
    pair_vis.index_put_((rows[:, None].expand(M, M)[vis] // 16, rows[None, :].expand(M, M)[vis] // 64), torch.tensor(True))
    pair_link = torch.zeros(nf, nt, dtype=torch.bool)
    sizes, can_tie, tied = {1: 0, 2: 0, 4: 0}, 0, 0
    for c in cases:
        assert (c.M, c.nH, c.nKV, c.hd, c.seg_lens) == (c0.M, c0.nH, c0.nKV, c0.hd, c0.seg_lens)
        tag = describe(c)
        # 1: every operand a bf16 number, every score an integer below 2^24
        for name, t in (("qkv", c.qkv_dev), ("d_o", c.d_o)):
            assert is_bf16(t), f"{tag}: {name} is not bf16-exact"
        q, k, _ = split_heads(c)
        for h in range(nH):
            s = q[h] @ k[h // G].t()
            assert bool((s == s.round()).all()) and float(s.abs().max()) < 2 ** 24, f"{tag}: head {h}: scores are not integers < 2^24"
            # 2: the visible maximum is attained 1, 2 or 4 times, everything else at least GAP lower
            sm = s.masked_fill(~vis, -float("inf"))
            mx = sm.amax(-1, keepdim=True)
            tie = sm == mx
            n = tie.sum(-1)
            bad = ~((n == 1) | (n == 2) | (n == 4))
            assert not bool(bad.any()), f"{tag}: row {int(bad.nonzero()[0])} head {h}: {int(n[bad][0])} keys attain the maximum"
            second = sm.masked_fill(tie, -float("inf")).amax(-1)
            bad = second > mx[:, 0] - GAP
            assert not bool(bad.any()), (f"{tag}: row {int(bad.nonzero()[0])} head {h}: the next visible score is only "
                                         f"{float((mx[:, 0] - second)[bad][0])} below the maximum")
            for r in range(M):   # the table of links is what the scores say
                assert tuple(tie[r].nonzero()[:, 0].tolist()) == c.ties[(r, h)], f"{tag}: row {r} head {h}: tie table differs from the scores"
            for a in sizes:
                sizes[a] += int((n == a).sum())
            two_keys = rows > seg_s   # a row that sees one key cannot tie
            can_tie, tied = can_tie + int(two_keys.sum()), tied + int((two_keys & (n > 1)).sum())
            # 3: key i + 1 and key seg_start - 1 score the row's maximum too (they carry the tie code)
            nxt = rows + 1 < M
            diag_ok[nxt] |= s[rows[nxt], rows[nxt] + 1] == mx[nxt, 0]
            prev = seg_s > 0
            seg_ok[prev] |= s[rows[prev], seg_s[prev] - 1] == mx[prev, 0]
            # 4: links per (16-row fragment, 64-key tile)
            r_, k_ = tie.nonzero(as_tuple=True)
            pair_link.index_put_((r_ // 16, k_ // 64), torch.tensor(True))
        # 6: every dS of the true function is a bf16 number
        assert c.exact.ds_is_bf16, f"{tag}: {c.exact.ds_first_bad}"
    bad = (rows + 1 < M) & ~diag_ok
    assert not bool(bad.any()), f"{describe(c0)}: row {int(bad.nonzero()[0])}: no head's tie code is carried by key i + 1"
    bad = (seg_s > 0) & ~seg_ok
    assert not bool(bad.any()), f"{describe(c0)}: row {int(bad.nonzero()[0])}: no head's tie code is carried by key seg_start - 1"
    bad = pair_vis & ~pair_link
    assert not bool(bad.any()), (f"{describe(c0)}: fragment {int(bad.nonzero()[0][0])} x key tile {int(bad.nonzero()[0][1])} "
                                 f"has visible (row, key) pairs but no link in any head")
    # 5: at least half of the (row, head) pairs are ties - of those that see two keys or more (the first row of a segment
    # cannot tie; a case of one-token segments has no such pair and nothing to hold)
    tie_share = tied / can_tie if can_tie else 1.0
    assert tie_share >= 0.5, f"{describe(c0)}: only {tie_share:.3f} of the (row, head) pairs that see two keys are ties"
    return SimpleNamespace(pairs=int(pair_vis.sum()), sizes=sizes, tie_share=tie_share, density=[c.density for c in cases],
                           nonzero={n: float((getattr(c0.exact, n) != 0).double().mean()) for n in ("dq", "dk", "dv")})


# ------------------------------------------------------------------------------------------------ expectations
def snap_dyadic(name, ref64, bits=20):
    """The fp64 reference works in the natural-log domain on q_hat / c2, so a value that is exactly dyadic (or exactly zero)
    comes back with fp64 noise around it. Snap to multiples of 2^-bits and ASSERT that the reference was within noise of
    that grid - a condition on the reference, not a tolerance on the kernel. + 0.0: zeros are +0, as accumulators that
    start at +0 leave them."""
    s = torch.round(ref64 * 2.0 ** bits) / 2.0 ** bits + 0.0
    err = float((ref64 - s).abs().max())
    assert err <= 1e-9, f"{name}: the fp64 reference is {err:.3e} off the dyadic grid 2^-{bits}"
    return s


def zero_noise(name, ref64):
    """For the outputs with an irrational factor: reference values within fp64 noise of zero ARE zero (nothing lies between:
    the smallest non-zero magnitude of these tensors is 2^-12)."""
    z = ref64.abs() < 1e-9
    assert not bool(((ref64.abs() >= 1e-9) & (ref64.abs() < 2.0 ** -12)).any()), f"{name}: reference values between noise and 2^-12"
    return torch.where(z, torch.zeros_like(ref64), ref64)


def expectations(c, ref64, device="cpu"):
    """What the kernels must store, from the plain fp64 reference `ref64` (test_gpu_attn_block._attn_ref64: masked softmax
    attention and autograd, segment by segment, no tiling) on the case's reference inputs. .o, .dv and at head_dim 64 .dq
    are the bf16 numbers to compare bits with; .lse2 is fp64 (an integer); .dk_ref and at head_dim 128 .dq_ref are fp64,
    held within one bf16 ulp."""
    o, lse, dx = ref64(c.qkv_ref.to(device), c.d_o.to(device), c.seg_lens, c.nH, c.nKV, c.hd)
    o, lse, dx = o.cpu(), lse.cpu(), dx.cpu()
    a, b = c.nH * c.hd, (c.nH + c.nKV) * c.hd
    tag = describe(c)
    e = SimpleNamespace(o=snap_dyadic(f"{tag} o", o).to(BF16), lse2=snap_dyadic(f"{tag} lse2", lse),
                        dv=snap_dyadic(f"{tag} dv", dx[:, b:]).to(BF16), dk_ref=zero_noise(f"{tag} dk", dx[:, a:b]), dq=None, dq_ref=None)
    if c.hd == 64:
        e.dq = snap_dyadic(f"{tag} dq", dx[:, :a]).to(BF16)
    else:
        e.dq_ref = zero_noise(f"{tag} dq", dx[:, :a])
    return e


def bf16_ulp(x64):
    """Spacing of the bf16 numbers in the binade of each value."""
    _, e = torch.frexp(x64.abs().double())
    e = torch.where(x64 == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))
    return torch.ldexp(torch.ones_like(x64, dtype=F64), e - 8)


def f32_ulp(x64):
    _, e = torch.frexp(x64.abs().double())
    e = torch.where(x64 == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))
    return torch.ldexp(torch.ones_like(x64, dtype=F64), e - 24)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------ failure messages
def _segment_of(c, row):
    s = int(c.seg_start[row])
    return c.seg_start.unique().tolist().index(s), row - s


def _dkv_chunks(c, key_tile, nch_max):
    """The query tiles (64 rows) that can see the key tile and how the backward cuts them into chunks (for the message only)."""
    qt_begin = key_tile
    qt_end = (int(c.seg_end[min(64 * key_tile + 63, c.M - 1)]) - 1) // 64
    n = qt_end - qt_begin + 1
    cs = (n + nch_max - 1) // nch_max
    return qt_begin, qt_end, cs


def locate(c, kind, row, col, nch=4, jq=1):
    """Where element (row, col) of tensor `kind` (o, lse2, dq: query rows; dk, dv: key rows) lives: segment, tiles, tie set."""
    per_key = kind in ("dk", "dv")
    head = col if kind == "lse2" else col // c.hd
    si, pos = _segment_of(c, row)
    where = f"row {row}, {'kv head' if per_key else 'head'} {head}, column {col if kind == 'lse2' else col % c.hd}; segment {si} (length {c.seg_lens[si]}), position {pos}"
    if not per_key:
        tile = f"forward tile {row // 128} (128 rows), wave {row % 128 // 32}" if kind in ("o", "lse2") else f"dQ tile {row // (64 * jq)} ({64 * jq} rows)"
        tie = c.ties.get((row, head), ())
        return (f"{where}; {tile}, 16-row fragment {row // 16}; tie set of the row: keys {list(tie)} in key tiles "
                f"{sorted({k // 64 for k in tie})} (key i+1 = {row + 1}, key seg_start-1 = {int(c.seg_start[row]) - 1})")
    G = c.nH // c.nKV
    qb, qe, cs = _dkv_chunks(c, row // 64, nch)
    links = [(r, h) for h in range(head * G, head * G + G) for r in range(row, int(c.seg_end[row])) if row in c.ties[(r, h)]]
    shown = ", ".join(f"row {r} head {h} (query tile {r // 64}, chunk {(r // 64 - qb) // cs}, 1/{len(c.ties[(r, h)])})" for r, h in links[:6])
    per_tile = {}
    for r, _ in links:
        per_tile[r // 64] = per_tile.get(r // 64, 0) + 1
    return (f"{where}; key tile {row // 64}, wave {row % 64 // 16}; its query tiles {qb}..{qe} in chunks of {cs} (attn_nch {nch}); "
            f"{len(links)} rows point at this key, per query tile {per_tile}: {shown}{' ...' if len(links) > 6 else ''}")


def assert_bits(name, c, kind, got, exp, **launch):
    """got: device or host [M][cols]; exp: the exact expectation in got's dtype. Bitwise."""
    bad = bits(got.cpu()) != bits(exp.cpu())
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        r, col = i // got.shape[1], i % got.shape[1]
        rows_bad = int(bad.any(1).sum())
        raise AssertionError(f"{name}: {n} of {got.numel()} elements ({rows_bad} rows) differ from the exact result; first at "
                             f"{locate(c, kind, r, col, **launch)}: got {float(got[r, col])!r}, expected {float(exp[r, col])!r}")


def assert_within(name, c, kind, got, ref64, ulp, **launch):
    """|got - ref| <= ulp elementwise (ulp: tensor), exactly zero where ref is zero. Returns the share of elements that are
    not bit-equal to the rounded reference (bf16 outputs) for the profile."""
    g = got.double().cpu()
    err = (g - ref64).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    bad = (err > ulp) | ((ref64 == 0) & (g != 0))
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        r, col = i // g.shape[1], i % g.shape[1]
        raise AssertionError(f"{name}: {n} of {g.numel()} elements are further than the bar from the reference; first at "
                             f"{locate(c, kind, r, col, **launch)}: got {float(g[r, col])!r}, reference {float(ref64[r, col])!r}, "
                             f"bar {float(ulp[r, col]):.3e}")
    return float((err > 0).double().mean())


# ------------------------------------------------------------------------------------------------ buffers
def poisoned(t, dtype, device):
    """The operand inside a larger buffer whose GUARD rows before and behind it are NaN (a 1-D operand counts elements)."""
    buf = torch.full((t.shape[0] + 2 * GUARD,) + tuple(t.shape[1:]), float("nan"), dtype=dtype, device=device)
    payload = buf[GUARD:GUARD + t.shape[0]]
    payload.copy_(t.to(dtype))
    assert payload.is_contiguous() and payload.data_ptr() % 16 == 0
    return payload


def guarded(shape, dtype, device, sentinel=-7.0):
    """A NaN payload (every element must be written) between two bands of GUARD sentinel rows; returns (payload, check)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    buf = torch.full((shape[0] + 2 * GUARD,) + shape[1:], sentinel, dtype=dtype, device=device)
    payload = buf[GUARD:GUARD + shape[0]]
    payload.fill_(float("nan"))
    assert payload.is_contiguous() and payload.data_ptr() % 16 == 0

    def check(name):
        for band, lo in (("leading", 0), ("trailing", GUARD + shape[0])):
            wrong = (buf[lo:lo + GUARD] != sentinel).reshape(-1).nonzero()
            assert not wrong.numel(), (f"{name}: {wrong.shape[0]} element(s) of the {band} guard band overwritten, first at band "
                                       f"element {int(wrong[0])}: {buf[lo:lo + GUARD].reshape(-1)[int(wrong[0])].item()}")

    return payload, check


# ------------------------------------------------------------------------------------------------ the cases
def _many_short():
    return [(3 * i) % 7 + 1 for i in range(40)] + [257]


SHAPES = {   # name: segment lengths (profiles/attn_exact.md says which code path each is the smallest to reach)
    "one_token": [1],
    "minimal_segments": [2, 1, 3],
    "residue_63": [63, 65],
    "aligned_boundaries": [64, 64, 1, 127],
    "third_key_tile": [129],
    "five_query_tiles": [300],
    "many_short": _many_short(),
    "ragged_1433": [200, 333, 1, 2, 63, 65, 129, 640],
    "sixteen_key_tiles": [1024, 37, 100, 5, 130],
}
LAST_THREE = ("many_short", "ragged_1433", "sixteen_key_tiles")
LAUNCH_SHAPES = ("five_query_tiles",) + LAST_THREE     # cases 6 to 9
HEADS_EVERYWHERE = (4, 2, 64)
HEADS_LAST_THREE = ((4, 2, 128), (7, 1, 64), (3, 3, 64), (3, 3, 128), (6, 1, 128))


def case_ids():
    """(shape name, nH, nKV, head_dim) of every exact case the GPU file runs."""
    ids = [(name,) + HEADS_EVERYWHERE for name in SHAPES]
    ids += [(name,) + heads for name in LAST_THREE for heads in HEADS_LAST_THREE]
    return ids


_CASES = {}


def cases_of(name, nH, nKV, hd):
    """The generated inputs of one case id, made once per process: one case, or two (flip 0, 1) for a single KV head."""
    key = (name, nH, nKV, hd)
    if key not in _CASES:
        seed = list(SHAPES).index(name) + 1
        _CASES[key] = [make_case(SHAPES[name], nH, nKV, hd, seed, flip) for flip in ((0, 1) if nKV == 1 else (0,))]
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ deferred-max schedule cases
SCHEDULE_SEGMENTS = {"aligned": [1024, 300], "mid_tile": [1000, 300]}
SCHEDULE_PROFILES = {   # key level sigma(position in segment, key index)
    "plus8_per_tile": lambda p, j: 8 * (j // 64),            # every tile exceeds the running max by exactly 8 at m_i = 1: stays
    "plus9_per_tile": lambda p, j: 9 * (j // 64),            # ... by 9: moves
    "minus8_per_tile": lambda p, j: 248 - 8 * (j // 64),     # falls for m_i > 0, rises for m_i = -1
    "low_then_high": lambda p, j: torch.where(p < 70, -250, 250),   # first visible key hundreds below zero
    "high_then_low": lambda p, j: torch.where(p < 70, 250, -250),
    "spread_in_tile": lambda p, j: 8 * (j // 64) + ((37 * j) % 17 - 8),
}


def make_schedule_case(profile, segments):
    """One KV head, two query heads, head_dim 64: q_hat[i][h] = m e_0 with m cycling through 1, 2, -1 along (i + h), k_j =
    sigma_j e_0, so score(i, j) = m sigma_j - rows of one wave rise, rise twice as fast or fall over the same keys. v holds
    integers 1..4: all positive, so o = sum p v / l has no cancellation and its fp32 evaluation is relatively accurate to
    about (keys) x 2^-24, far inside the half bf16 ulp that separates "within one ulp" from "rounded elsewhere"."""
    seg_lens, nH, nKV, hd = SCHEDULE_SEGMENTS[segments], 2, 1, 64
    M = sum(seg_lens)
    c = SimpleNamespace(seg_lens=seg_lens, nH=nH, nKV=nKV, hd=hd, M=M, ld=(nH + 2 * nKV) * hd, seed=0, flip=0)
    c.seg_start, c.seg_end = seg_tables(seg_lens)
    j = torch.arange(M)
    sigma = SCHEDULE_PROFILES[profile](j - c.seg_start.long(), j)
    assert int(sigma.abs().max()) <= 256
    m = torch.tensor([1, 2, -1])[(j[:, None] + torch.arange(nH)[None, :]) % 3]
    q = torch.zeros(M, nH, hd, dtype=F64)
    q[:, :, 0] = m.double()
    k = torch.zeros(M, nKV, hd, dtype=F64)
    k[:, 0, 0] = sigma.double()
    v = torch.randint(1, 5, (M, nKV, hd), generator=torch.Generator().manual_seed(5)).double()
    c.qkv_dev = torch.cat([q.reshape(M, -1), k.reshape(M, -1), v.reshape(M, -1)], 1)
    assert is_bf16(c.qkv_dev)
    c.qkv_ref = c.qkv_dev.clone()
    c.qkv_ref[:, : nH * hd] /= hd ** -0.5 * LOG2E
    c.d_o = torch.zeros(M, nH * hd, dtype=F64)
    c.ties = {}
    return c
