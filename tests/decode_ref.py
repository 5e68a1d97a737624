"""Plain torch fp64 restatement of the KV-cached decode kernels (gemm_skinny, attn_decode; slamkit_amd/csrc/kernels.h) and the
inputs that make their edge cases visible. CPU only: nothing here touches a device. Shared by tests/test_decode_ref_host.py
(the helpers themselves, and the condition the needle inputs must meet) and tests/test_gpu_decode_edges.py (the kernels).

Two kinds of input:
 * integer GEMM operands whose every partial sum is below 2^24, so an fp32 accumulation in any order, split or tile is exact
   and the kernel's output is compared bit for bit;
 * "needle" KV caches: a few keys at the positions where an index can be off by one (0, pos - 1, pos, every split boundary,
   the wave / slot stride boundaries) carry K = 0 and a large V pattern of their own. Their score is exactly 0 for every query,
   their weight in the output is large, and each one owns a set of output columns, so a dropped, doubled or misplaced
   boundary key moves the row's output by an order of magnitude more than the tolerance. Every cache row the kernel may not
   read is NaN."""
import math

import torch

from oracle import slam_oracle as O

LOG2E = 1.4426950408889634
# The needles' V value. A needle owns hd / R output columns (one, for the 37 needles of a 1088-key row at hd 64), so losing it
# moves a head's output by at most about 1 / sqrt(hd) = 0.125 relative; at 4096 the randn keys with the largest scores still
# carry enough weight to pull some heads down to 0.04, at 2^18 every configuration of the GPU test stays above 0.12
# (tests/test_decode_ref_host.py asserts >= 0.1). bf16-exact, and (c - bias) + bias still rounds to c in bf16.
NEEDLE_C = 262144.0


# ---- gemm_skinny ------------------------------------------------------------------------------------------------------------
def skinny_int_case(M, N, K, seed):
    """Integer-valued bf16 operands: X [M][K], W [N][K] in [-3, 3], bias [N], resid [M][N] in [-8, 8], and the exact int64
    product xw = X W^T. |xw + bias + resid| <= 9 K + 16, which must stay below 2^24 (skinny_exact asserts it)."""
    assert 9 * K + 16 < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    Xi = torch.randint(-3, 4, (M, K), generator=g)
    Wi = torch.randint(-3, 4, (N, K), generator=g)
    bi = torch.randint(-8, 9, (N,), generator=g)
    ri = torch.randint(-8, 9, (M, N), generator=g)
    return dict(M=M, N=N, K=K, X=Xi.to(torch.bfloat16), W=Wi.to(torch.bfloat16), bias=bi.to(torch.bfloat16),
                resid=ri.to(torch.bfloat16), xw=Xi @ Wi.t(), bias_i=bi, resid_i=ri)


def skinny_exact(case, use_bias, use_resid):
    """int64 X W^T (+ bias) (+ resid)."""
    r = case["xw"].clone()
    if use_bias:
        r = r + case["bias_i"][None, :]
    if use_resid:
        r = r + case["resid_i"]
    assert int(r.abs().max()) < 2 ** 24
    return r


# ---- attn_decode ------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def attn_decode_chunk(B, nH, nKV, hd, kv_bound, part_bytes=None):
    """Keys per split, restated from attn_decode_chunk (decode.hip): multiples of 64 aiming at about 512 blocks over
    (splits, KV heads, rows), doubled while the fp32 partials [B][nH][ns][hd + 2] exceed part_bytes. -1: no room for one split."""
    target = max(512 // (B * nKV), 1)
    chunk = max(_cdiv(_cdiv(kv_bound, target), 64) * 64, 64)
    if part_bytes is None:
        return chunk
    while B * nH * _cdiv(kv_bound, chunk) * (hd + 2) * 4 > part_bytes:
        if chunk >= kv_bound:
            return -1
        chunk *= 2
    return chunk


def _rope(x, pos, hd, theta):
    """rotate-half RoPE of x [heads][hd] (fp64) at one position."""
    cos, sin = O.rope_cos_sin(torch.tensor([[int(pos)]]), hd, theta)
    cos, sin = cos[0, 0].double(), sin[0, 0].double()
    return x * cos + O.rotate_half(x) * sin


def _bf16(x):
    return x.to(torch.float32).to(torch.bfloat16)


def _row_ref(qkv, bias, pos, kc, vc, nH, nKV, hd, theta, drop=None):
    """One batch row: o [nH][hd] fp64, k_new / v_new [nKV][hd] bf16. drop: a key index left out of the softmax."""
    G = nH // nKV
    x = qkv.double()
    if bias is not None:
        x = x + bias.double()
    x = x.view(nH + 2 * nKV, hd)
    q = _bf16(_rope(x[:nH], pos, hd, theta) * (hd ** -0.5 * LOG2E)).double()
    k_new = _bf16(_rope(x[nH:nH + nKV], pos, hd, theta))
    v_new = _bf16(x[nH + nKV:])
    K = kc[:, :pos + 1].double().clone()  # [nKV][pos + 1][hd]
    V = vc[:, :pos + 1].double().clone()
    K[:, pos] = k_new.double()
    V[:, pos] = v_new.double()
    s = torch.einsum("kgd,kjd->kgj", q.view(nKV, G, hd), K)  # log2 domain; head h = k G + g reads KV head k
    if drop is not None:
        s[..., drop] = -math.inf
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = torch.einsum("kgj,kjd->kgd", p, V) / p.sum(-1, keepdim=True)
    return o.reshape(nH, hd), k_new, v_new


def attn_decode_ref(qkv, bias, lens, kc, vc, nH, nKV, hd, theta):
    """The contract of attn_decode in fp64. qkv fp32 [B][(nH + 2 nKV) hd] without bias, bias bf16 or None, kc / vc bf16
    [B][nKV][cap][hd]. Bias, rotate-half RoPE at position lens[b], q scaled by hd^-0.5 log2(e) and rounded once to bf16, the new
    k / v rounded once to bf16 and placed at row lens[b], softmax in the log2 domain over keys 0 .. lens[b].
    Returns o [B][nH][hd] (fp64), k_new, v_new [B][nKV][hd] (bf16). Cache rows above lens[b] are never read."""
    B = qkv.shape[0]
    out = [_row_ref(qkv[b], bias, int(lens[b]), kc[b], vc[b], nH, nKV, hd, theta) for b in range(B)]
    return torch.stack([r[0] for r in out]), torch.stack([r[1] for r in out]), torch.stack([r[2] for r in out])


def needle_positions(pos, hd, chunk_hint):
    """Sorted key positions in [0, pos] at which an index can be off by one."""
    slots = 64 // (hd // 8)
    want = [0, pos - 1, pos, 63, 64, 4 * slots - 1, 4 * slots]
    for k in range(1, pos // chunk_hint + 1):
        want += [k * chunk_hint - 1, k * chunk_hint]
    return sorted({p for p in want if 0 <= p <= pos})


def needle_case(B, nH, nKV, hd, lens, chunk_hint, seed, cap=None, theta=None, c=None, new_token_needle=True):
    """Inputs of one attn_decode call: qkv = 2 randn (fp32), bias = 0.5 randn (bf16), caches = randn (bf16), then
     (a) every cache row >= lens[b] is NaN: the kernel writes row lens[b] before it uses it and reads nothing above;
     (b) needle r of the row's R needles (needle_positions) has K = 0 and V = 0 except V[..., r::R] = c, in every KV head.
    The needle at lens[b] is the new token: the k columns of qkv are -bias (RoPE of 0 is 0), the v columns the pattern - bias.
    new_token_needle = False leaves the new token gaussian (its rotated K is then worth comparing)."""
    c = NEEDLE_C if c is None else c
    assert len(lens) == B and nH % nKV == 0
    cap = cap if cap is not None else -(-(max(lens) + 1) // 64) * 64 + 64
    assert max(lens) < cap
    theta = theta if theta is not None else (10000.0 if hd == 64 else 1e6)
    QKV = (nH + 2 * nKV) * hd
    g = torch.Generator().manual_seed(seed)
    kc = torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, nKV, cap, hd, generator=g).to(torch.bfloat16)
    qkv = torch.randn(B, QKV, generator=g) * 2
    bias = (torch.randn(QKV, generator=g) * 0.5).to(torch.bfloat16)
    bf = bias.float().view(nH + 2 * nKV, hd)
    x = qkv.view(B, nH + 2 * nKV, hd)
    needles = []
    for b in range(B):
        pos = int(lens[b])
        ns = needle_positions(pos, hd, chunk_hint)
        R = len(ns)
        assert R <= hd
        for r, j in enumerate(ns):
            pat = torch.zeros(hd)
            pat[r::R] = c
            if j == pos and not new_token_needle:
                continue
            if j == pos:
                x[b, nH:nH + nKV] = -bf[nH:nH + nKV]
                x[b, nH + nKV:] = pat[None, :] - bf[nH + nKV:]
            else:
                kc[b, :, j] = 0
                vc[b, :, j] = pat.to(torch.bfloat16)
        kc[b, :, pos:] = math.nan
        vc[b, :, pos:] = math.nan
        needles.append(ns)
    return dict(B=B, nH=nH, nKV=nKV, hd=hd, cap=cap, theta=theta, chunk_hint=chunk_hint, lens=torch.tensor(lens, dtype=torch.int32),
                qkv=qkv.contiguous(), bias=bias, kc=kc, vc=vc, needles=needles)


def case_ref(case):
    c = case
    return attn_decode_ref(c["qkv"], c["bias"], c["lens"], c["kc"], c["vc"], c["nH"], c["nKV"], c["hd"], c["theta"])


def needle_sensitivity(case):
    """Reference only: for every row and every needle the fp64 reference is recomputed with that one key masked out; returns
    the smallest relative L2 change of any (row, head) output. Rows with a single key are left out (no key remains)."""
    c = case
    worst = math.inf
    for b in range(c["B"]):
        pos = int(c["lens"][b])
        if pos == 0:
            continue
        args = (c["qkv"][b], c["bias"], pos, c["kc"][b], c["vc"][b], c["nH"], c["nKV"], c["hd"], c["theta"])
        o = _row_ref(*args)[0]
        for j in c["needles"][b]:
            od = _row_ref(*args, drop=j)[0]
            rel = (od - o).norm(dim=-1) / o.norm(dim=-1)
            worst = min(worst, float(rel.min()))
    return worst


# ---- the attn_decode cases of tests/test_gpu_decode_edges.py ------------------------------------------------------------------
RAGGED_LENS = [1087, 0, 1, 63, 64, 65, 511, 640]
RAGGED_BOUND, RAGGED_CAP = 1088, 1152
ATTN_TOL = 1e-2  # per (row, head) relative L2 error of o

# (hd, G, nKV): every instantiation of attn_decode_kernel, G = 1 also as OPT-125m's 12 / 12 heads
INSTANCES = [(hd, G, 2) for hd in (64, 128) for G in range(1, 9)] + [(64, 1, 12), (128, 1, 12)]
# (hd, G): the ragged batch again under workspaces sized for kv_bound 64, 256 and the real bound
LIMITED = [(64, 7), (128, 6), (64, 1)]
LIMITED_BOUNDS = [64, 256, RAGGED_BOUND]


def attn_op_head(B, hd):
    """Bytes slam_op_attn_decode keeps ahead of the split partials (positions and RoPE tables, 256-byte aligned)."""
    return ((B * 8 + 255) & ~255) + ((4 * B * (hd // 2) * 4 + 255) & ~255)


def attn_op_workspace(B, nH, nKV, hd, kv_bound):
    """slam_op_attn_decode_workspace restated (the GPU test asserts the library agrees)."""
    chunk = attn_decode_chunk(B, nH, nKV, hd, kv_bound)
    return attn_op_head(B, hd) + B * nH * _cdiv(kv_bound, chunk) * (hd + 2) * 4


def ragged_case(hd, G, nKV, chunk):
    return needle_case(len(RAGGED_LENS), G * nKV, nKV, hd, RAGGED_LENS, chunk, seed=1000 * hd + 10 * G + nKV, cap=RAGGED_CAP)


def limited_chunk(hd, G, ws_bound):
    """The chunk attn_decode takes for the ragged batch when the op's workspace was sized for kv_bound = ws_bound."""
    B, nKV = len(RAGGED_LENS), 2
    room = attn_op_workspace(B, G * nKV, nKV, hd, ws_bound) - attn_op_head(B, hd)
    return attn_decode_chunk(B, G * nKV, nKV, hd, RAGGED_BOUND, room)


MANY_ROWS = {
    # B nKV > 512: one split, one block per (row, KV head)
    "b64-mha": dict(B=64, nH=12, nKV=12, hd=64, lens=[0, 299] * 32, kv_bound=300, cap=320),
    "b33-gqa": dict(B=33, nH=14, nKV=2, hd=64, lens=[(37 * i) % 300 for i in range(33)], kv_bound=300, cap=320),
}


def many_rows_case(name):
    m = MANY_ROWS[name]
    chunk = attn_decode_chunk(m["B"], m["nH"], m["nKV"], m["hd"], m["kv_bound"])
    return needle_case(m["B"], m["nH"], m["nKV"], m["hd"], m["lens"], chunk, seed=len(name) + m["B"], cap=m["cap"])
