"""-m gpu parity tests of the attention block as the training step runs it: attention forward + backward at the step's own
launch sizes (M = 8192 / 16,384, segments up to 8192, ragged M), the rotated backward (slam_op_attn_bwd_rope), the fused
QKV projection (slam_op_gemm_nt_rope) and the bias-gradient column sums (slam_op_colsum).

Reference for everything: plain PyTorch in fp64 ON THE DEVICE on the same bf16-representable inputs. Attention is computed
segment by segment (a segment attends to nothing else, so the full masked M x M product and the per-segment causal product
are the same function) with as many heads per batch as fit 2 GB of fp64 scores; gradients come from autograd. The query
pre-scale is handled by test_gpu_ops._attn_prescale. The transpose rotation of B2 is autograd through the fp64 forward
rotation, not a restatement of the kernels' store code.

Attention tolerances are those of test_gpu_ops.test_attention_fwd_bwd (fwd 6e-3 rel-RMS / 3e-2 of the abs-max; bwd
1.5e-2 / 6e-2; lse 1e-4), held globally AND per slice: rel-RMS on every slice of >= 64 rows, the max-abs criterion on every
slice against that slice's own reference abs-max. A slice is one head of one segment, and a segment of 192 rows or more is
cut further into blocks of 128 rows counted from its start (a last piece under 64 rows stays with the block before it):
gradients deep inside a long segment are much smaller than at its start, and a wrong fragment there would hide behind the
segment's first rows. One wrong 16-row fragment of one head fails, wherever it is.

The 2x-emulation rule. Where segments shorter than 64 rows exist (the ragged cases, configs[3] packed) a slice's max-abs bar
is max(the bar above, 2 x the error of _attn_emu64 on that slice): _attn_emu64 is the same fp64 function with the roundings
any bf16-MFMA flash kernel makes (P, O and dS to bf16 before their second products) and no part of the code under test. It is
needed for one kind of slice: dq of a two-token segment is p0 p1 (dP0 - dP1) (k0 - k1) / sqrt(hd), small when one key takes
nearly all the weight, while D = rowsum(dO * O) carries the 2^-9 rounding of the stored O. Measured on an MI355X: ragged
head_dim 64, segment 45 (2 tokens), head 1, dq: kernel 6.614e-2 of the slice's abs-max, emulation 6.614e-2, so the bar of that
slice is 1.323e-1 (6.647e-2 / 6.476e-2 and the same factor after the dense / packed transpose rotation; after the dense
rotation the emulation of one more slice exceeds 3e-2 and raises that slice's bar too). Every other slice of every case is held
to the fixed bar; the largest worst-slice value reported by the other cases is 2.4e-2 (ragged head_dim 128, dq / dk of 2-token
segments).

ZERO_FLOOR: a slice whose exact value is zero has no abs-max to be relative to. That happens by construction: dq and dk of a
one-token segment are exactly 0 (a softmax over one key is constant), while the kernels return the fp32 cancellation residue
of dP - D, two fp32 sums of head_dim products added in different orders (each within head_dim * 2^-24 = 7.6e-6 of
sum |dO v|). Such slices are held to max_tol * 2^-10 of the TENSOR's abs-max (5.9e-5 of it for the backward): three orders of
magnitude under the global criterion, two above the residue. The floor acts only on slices whose own abs-max is below 2^-10
of the tensor's."""
import random
from itertools import product
from types import SimpleNamespace

import pytest
import torch

from oracle import slam_oracle as O
from tests.gpu_util import dev_bf16, lib, ptr, rnd, stream, sync
from tests.test_gpu_ops import _attn_case, _attn_prescale

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
GUARD = 128          # canary rows behind every output
SENT = -7.0          # canary value
ZERO_FLOOR = 2.0 ** -10
FWD_TOL, BWD_TOL, LSE_TOL = (6e-3, 3e-2), (1.5e-2, 6e-2), (1e-4, None)


def _configs3_lengths():
    """16,384 packed tokens: lengths drawn from U{64..2048} (fixed seed) plus one of exactly 2048 and one of 1; the last draw is
    cut to what is left."""
    r = random.Random(1234)
    lens, left = [2048, 1], 16384 - 2049
    while left > 0:
        n = min(r.randint(64, 2048), left)
        lens.append(n)
        left -= n
    r.shuffle(lens)
    return lens


def _ragged_lengths():
    """4999 tokens (M % 64 = 7, M % 128 = 7): boundaries at many residues mod 64, lengths 1, 63, 65, 1500 and a run of 40
    segments of 1..7 tokens (key tiles that hold many segments)."""
    lens = [37, 1, 63, 65, 1500, 100, 5, 130, 64, 129, 200, 31] + [(3 * i) % 7 + 1 for i in range(40)] + [257, 99, 511, 77, 640, 13]
    lens.append(4999 - sum(lens))
    assert lens[-1] > 0
    return lens


CASES = {  # name: (segment lengths, nH, nKV, head_dim)
    "slam358m_step": ([1024] * 8, 14, 2, 64),
    "configs3_packed": (_configs3_lengths(), 12, 2, 128),
    "long_single": ([8192], 7, 1, 64),
    "opt125m_step": ([1024] * 8, 12, 12, 64),
    "opt1p3b_heads": ([1024] * 2, 32, 32, 64),
    "ragged_hd64": (_ragged_lengths(), 4, 2, 64),
    "ragged_hd128": (_ragged_lengths(), 4, 2, 128),
}
_CACHE = {}


# ----------------------------------------------------------------------------------------- fp64 reference
def _attn_ref64(x, d_o, segs, nH, nKV, hd):
    """x: fp64 device [M][(nH + 2 nKV) hd] (queries unscaled), d_o: fp64 device [M][nH hd]. Returns o [M][nH hd],
    lse2 [M][nH] (log2 domain) and d(x), all fp64."""
    M, G = x.shape[0], nH // nKV
    x = x.clone().requires_grad_(True)
    o = torch.empty(M, nH, hd, dtype=torch.float64, device=x.device)
    lse = torch.empty(M, nH, dtype=torch.float64, device=x.device)
    s0 = 0
    for n in segs:
        do = d_o[s0:s0 + n].view(n, nH, hd).transpose(0, 1)
        causal = torch.ones(n, n, dtype=torch.bool, device=x.device).tril_()
        hb = max(1, min(nH, 2 ** 28 // (n * n)))  # heads per batch: at most 2 GB of fp64 scores
        for h0 in range(0, nH, hb):
            h1 = min(nH, h0 + hb)
            xs = x[s0:s0 + n]
            q = xs[:, : nH * hd].view(n, nH, hd).transpose(0, 1)
            k = xs[:, nH * hd: (nH + nKV) * hd].view(n, nKV, hd).transpose(0, 1)
            v = xs[:, (nH + nKV) * hd:].view(n, nKV, hd).transpose(0, 1)
            kv = torch.arange(h0, h1, device=x.device) // G
            s = (q[h0:h1] @ k[kv].transpose(1, 2)) * hd ** -0.5
            s = s.masked_fill(~causal, float("-inf"))
            l = torch.logsumexp(s, -1)
            oh = torch.exp(s - l[..., None]) @ v[kv]
            (oh * do[h0:h1]).sum().backward()
            o[s0:s0 + n, h0:h1] = oh.detach().transpose(0, 1)
            lse[s0:s0 + n, h0:h1] = l.detach().t() * LOG2E
        s0 += n
    return o.view(M, nH * hd), lse, x.grad


def _bf16(t):
    return t.to(torch.bfloat16).double()


def _attn_emu64(x, d_o, segs, nH, nKV, hd):
    """The yardstick of the 2x rule (module docstring): the same function in fp64 with the roundings ANY bf16-MFMA flash
    kernel makes and nothing of the code under test - P to bf16 before P V and P^T dO, O to bf16 (the backward reads the stored
    O for D = rowsum(dO * O)), dS to bf16 before dS K and dS^T Q. Returns o and d(x), unrounded (callers round once, last)."""
    M, G, a, b = x.shape[0], nH // nKV, nH * hd, (nH + nKV) * hd
    o = torch.empty(M, nH, hd, dtype=torch.float64, device=x.device)
    dx = torch.zeros_like(x)
    s0 = 0
    for n in segs:
        r = slice(s0, s0 + n)
        causal = torch.ones(n, n, dtype=torch.bool, device=x.device).tril_()
        hb = max(1, min(nH, 2 ** 28 // (n * n)))
        for h0 in range(0, nH, hb):
            h1 = min(nH, h0 + hb)
            kv = torch.arange(h0, h1, device=x.device) // G
            q = x[r, :a].view(n, nH, hd).transpose(0, 1)[h0:h1]
            k = x[r, a:b].view(n, nKV, hd).transpose(0, 1)[kv]
            v = x[r, b:].view(n, nKV, hd).transpose(0, 1)[kv]
            do = d_o[r].view(n, nH, hd).transpose(0, 1)[h0:h1]
            s = ((q @ k.transpose(1, 2)) * hd ** -0.5).masked_fill(~causal, float("-inf"))
            pu = torch.exp(s - s.amax(-1, keepdim=True))
            l = pu.sum(-1, keepdim=True)
            oh = (_bf16(pu) @ v) / l
            p = pu / l
            ds = p * (do @ v.transpose(1, 2) - (do * _bf16(oh)).sum(-1, keepdim=True))
            o[r, h0:h1] = oh.transpose(0, 1)
            dx[r, :a].view(n, nH, hd)[:, h0:h1] = ((_bf16(ds) @ k) * hd ** -0.5).transpose(0, 1)
            dx[r, a:b].view(n, nKV, hd).index_add_(1, kv, ((_bf16(ds).transpose(1, 2) @ q) * hd ** -0.5).transpose(0, 1))
            dx[r, b:].view(n, nKV, hd).index_add_(1, kv, (_bf16(p).transpose(1, 2) @ do).transpose(0, 1))
        s0 += n
    return o.view(M, a), dx


def _rope64(x, pos, theta):
    """rotate-half RoPE in fp64 on x [M][heads][hd] at integer positions pos [M] (oracle.rotate_half convention)."""
    hd = x.shape[-1]
    inv = theta ** (-torch.arange(0, hd, 2, dtype=torch.float64, device=x.device) / hd)
    ang = pos.double()[:, None] * inv[None]
    emb = torch.cat([ang, ang], -1)[:, None, :]
    return x * emb.cos() + O.rotate_half(x) * emb.sin()


def _rope64_transpose(d, pos, theta, heads):
    """Gradient of the pre-RoPE tensor from the gradient d [M][heads * hd] of the rotated one: autograd through _rope64."""
    M = d.shape[0]
    x = torch.zeros(M, heads, d.shape[1] // heads, dtype=torch.float64, device=d.device, requires_grad=True)
    (g,) = torch.autograd.grad(_rope64(x, pos, theta), x, d.view_as(x))
    return g.reshape(M, -1)


# ----------------------------------------------------------------------------------------- checks
BLOCK = 128


def _slices(segs):
    """Row slices of the per-slice criteria (module docstring): [(segment, first row inside it, rows)], slice index per row."""
    desc, ids = [], []
    for si, n in enumerate(segs):
        nb = n // BLOCK + (1 if n % BLOCK >= 64 or n < BLOCK else 0)
        for bi in range(nb):
            lo = bi * BLOCK
            rows = (n if bi == nb - 1 else lo + BLOCK) - lo
            ids += [len(desc)] * rows
            desc.append((si, lo, rows))
    return desc, torch.tensor(ids), torch.tensor([d[2] for d in desc])


def _slice_check(name, got, ref, c, nh, tol, emu=None):
    """got / ref: device [M][nh * w]. Global rel-RMS / max-abs like gpu_util.check, then the same per (slice, head).
    emu (the _attn_emu64 value of the same tensor, optional): a slice's max-abs bar is max(max_tol, 2 x the emulation's own
    max-abs / abs-max on that slice)."""
    rms_tol, max_tol = tol
    M, nseg = c.M, len(c.slices)
    w = ref.shape[1] // nh
    g, r = got.double().reshape(M, nh, w), ref.reshape(M, nh, w)
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    e = g - r
    e2, r2, ea, ra = e.pow(2).sum(-1), r.pow(2).sum(-1), e.abs().amax(-1), r.abs().amax(-1)

    def z():
        return torch.zeros(nseg, nh, dtype=torch.float64, device=g.device)
    se2, sr2 = z().index_add_(0, c.slice_id, e2), z().index_add_(0, c.slice_id, r2)
    idx = c.slice_id[:, None].expand(M, nh)
    sea, sra = z().scatter_reduce_(0, idx, ea, "amax"), z().scatter_reduce_(0, idx, ra, "amax")
    g_rel, g_max, g_scale = (e2.sum() / r2.sum()).sqrt(), ea.max(), ra.max()
    s_rel = torch.where(c.slice_len[:, None] >= 64, (se2 / sr2.clamp_min(1e-300)).sqrt(), torch.zeros_like(se2))
    s_scale = torch.maximum(sra, ZERO_FLOOR * g_scale).clamp_min(1e-6)
    s_ratio = sea / s_scale
    s_bar = torch.full_like(s_ratio, max_tol if max_tol is not None else float("inf"))
    raised = ""
    if emu is not None and max_tol is not None:
        ee = (_bf16(emu).reshape(M, nh, w) - r).abs().amax(-1)
        e_ratio = z().scatter_reduce_(0, idx, ee, "amax") / s_scale
        s_bar = torch.maximum(s_bar, 2 * e_ratio)
        n_up, i_up = int((s_bar > max_tol).sum()), int(e_ratio.argmax())
    i_rel, i_ratio = int(s_rel.argmax()), int((s_ratio / s_bar).argmax())
    g_rel, g_max, g_scale, w_rel, w_ratio, w_bar = [float(t) for t in (g_rel, g_max, g_scale, s_rel.flatten()[i_rel],
                                                                        s_ratio.flatten()[i_ratio], s_bar.flatten()[i_ratio])]

    def where(i):
        si, lo, rows = c.slices[i // nh]
        return f"seg {si} (len {c.segs[si]}) rows {lo}..{lo + rows - 1} head {i % nh}"
    if emu is not None and max_tol is not None and n_up:
        raised = f"; {n_up} slice bar(s) raised by the 2x-emulation rule, emulation max_abs/absmax={float(e_ratio.flatten()[i_up]):.3e} at {where(i_up)}"
    print(f"[parity] {name}: rel_rms={g_rel:.3e} max_abs={g_max:.3e} ref_absmax={g_scale:.3e} | worst slice rel_rms={w_rel:.3e} "
          f"at {where(i_rel)}; worst slice max_abs/absmax={w_ratio:.3e} (bar {w_bar:.3e}) at {where(i_ratio)}{raised}")
    assert g_rel <= rms_tol, f"{name}: rel rms {g_rel:.3e} > {rms_tol}"
    assert w_rel <= rms_tol, f"{name}: slice {where(i_rel)}: rel rms {w_rel:.3e} > {rms_tol}"
    if max_tol is not None:
        assert g_max <= max_tol * max(g_scale, 1e-6), f"{name}: max abs {g_max:.3e} > {max_tol} * {g_scale:.3e}"
        assert w_ratio <= w_bar, f"{name}: slice {where(i_ratio)}: max abs / slice abs-max {w_ratio:.3e} > {w_bar:.3e}"


def _dcheck(name, got, ref, rms_tol, max_tol):
    """gpu_util.check on device tensors (no host copy of the operands)."""
    g, r = got.double(), ref.double()
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    rel = float(((g - r).pow(2).mean().sqrt()) / (r.pow(2).mean().sqrt() + 1e-30))
    m, scale = float((g - r).abs().max()), float(r.abs().max())
    print(f"[parity] {name}: rel_rms={rel:.3e} max_abs={m:.3e} ref_absmax={scale:.3e}")
    assert rel <= rms_tol, f"{name}: rel rms {rel:.3e} > {rms_tol}"
    assert m <= max_tol * max(scale, 1e-6), f"{name}: max abs {m:.3e} > {max_tol} * {scale:.3e}"


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _guarded(rows, cols, dtype):
    """[rows + GUARD][cols]: NaN body (every element must be written), sentinel canary rows behind it."""
    t = torch.full((rows + GUARD, cols), SENT, dtype=dtype, device="cuda")
    t[:rows] = float("nan")
    return t


def _guard_ok(t, rows):
    return bool((t[rows:] == SENT).all())


# ----------------------------------------------------------------------------------------- attention cases
def _case(name):
    if name in _CACHE:
        return _CACHE[name]
    segs, nH, nKV, hd = CASES[name]
    M, ld, qkv, seg_s, seg_e = _attn_case(segs, nH, nKV, seed=len(segs), hd=hd)
    d_o = rnd(M, nH * hd, seed=9)
    qkv_dev, qkv_ref = _attn_prescale(qkv, nH, hd)
    c = SimpleNamespace(name=name, segs=segs, nH=nH, nKV=nKV, hd=hd, M=M, ld=ld)
    c.qd, c.dod, c.ss, c.se = dev_bf16(qkv_dev), dev_bf16(d_o), seg_s.cuda(), seg_e.cuda()
    c.slices, slice_id, slice_len = _slices(segs)
    c.slice_id, c.slice_len = slice_id.cuda(), slice_len.cuda()
    c.o_ref, c.lse_ref, c.dqkv_ref = _attn_ref64(qkv_ref.cuda().double(), d_o.cuda().double(), segs, nH, nKV, hd)
    c.o_emu = c.dqkv_emu = None
    if min(segs) < 64:  # short slices: the 2x-emulation rule may apply (module docstring)
        c.o_emu, c.dqkv_emu = _attn_emu64(qkv_ref.cuda().double(), d_o.cuda().double(), segs, nH, nKV, hd)
    c.out = None
    _CACHE[name] = c
    return c


def _fwd(c):
    o, lse = _guarded(c.M, c.nH * c.hd, torch.bfloat16), _guarded(c.nH * c.M, 1, torch.float32)
    assert lib().slam_op_attn_fwd(ptr(c.qd), ptr(o), ptr(lse), ptr(c.ss), c.M, c.nH, c.nKV, c.hd, stream()) == 0
    sync()
    return o, lse


def _bwd(c, o, lse, rope=None):
    """rope = None: slam_op_attn_bwd; else (position_ids or None, T, theta): slam_op_attn_bwd_rope."""
    L = lib()
    nws = L.slam_op_attn_bwd_workspace(c.M, c.nH, c.hd) // 4
    ws = _guarded(nws, 1, torch.float32)
    dqkv = _guarded(c.M, c.ld, torch.bfloat16)
    if rope is None:
        rc = L.slam_op_attn_bwd(ptr(c.qd), ptr(o), ptr(c.dod), ptr(lse), ptr(dqkv), ptr(ws), ptr(c.ss), ptr(c.se),
                                c.M, c.nH, c.nKV, c.hd, stream())
        tab = None
    else:
        pos, T, theta = rope
        tab = _guarded(2 * c.M * (c.hd // 2), 1, torch.float32)
        rc = L.slam_op_attn_bwd_rope(ptr(c.qd), ptr(o), ptr(c.dod), ptr(lse), ptr(dqkv), ptr(ws), ptr(c.ss), ptr(c.se),
                                     ptr(pos), T, theta, c.M, c.nH, c.nKV, c.hd, ptr(tab), stream())
    sync()
    assert rc == 0
    assert _guard_ok(dqkv, c.M), "attention backward wrote behind dqkv"
    assert _guard_ok(ws, nws), "attention backward wrote behind its workspace"
    assert tab is None or _guard_ok(tab, 2 * c.M * (c.hd // 2)), "rope tables written behind their workspace"
    return dqkv


def _outputs(c):
    """o, lse and dqkv of the default launch shapes (computed once per case)."""
    if c.out is None:
        o, lse = _fwd(c)
        c.out = (o, lse, _bwd(c, o, lse))
    return c.out


def _check_bwd(c, tag, dqkv, rot=None):
    """rot (optional): fp64 map (d [M][heads * hd], heads) -> transpose-rotated d, applied to the reference dq / dk."""
    nH, nKV, hd, M = c.nH, c.nKV, c.hd, c.M
    a, b = nH * hd, (nH + nKV) * hd
    for what, lo, hi, heads in (("dq", 0, a, nH), ("dk", a, b, nKV), ("dv", b, c.ld, nKV)):
        ref = c.dqkv_ref[:, lo:hi].contiguous()
        emu = None if c.dqkv_emu is None else c.dqkv_emu[:, lo:hi].contiguous()
        if rot is not None and what != "dv":
            ref, emu = rot(ref, heads), None if emu is None else rot(emu, heads)
        _slice_check(f"{tag} {what}", dqkv[:M, lo:hi], ref, c, heads, BWD_TOL, emu)


# ----------------------------------------------------------------------------------------- B1
@pytest.mark.parametrize("name", list(CASES))
def test_attention_at_step_shapes(name):
    """slam_op_attn_fwd / slam_op_attn_bwd at the step's shapes against fp64, globally and per slice (module docstring); two runs
    bit-identical; canary rows behind o, lse, dqkv and the backward workspace untouched (the ragged cases have M % 64 != 0)."""
    c = _case(name)
    M, nH = c.M, c.nH
    o, lse = _fwd(c)
    assert _guard_ok(o, M) and _guard_ok(lse, nH * M), "attention forward wrote behind its outputs"
    _slice_check(f"{name} attn fwd o", o[:M], c.o_ref, c, nH, FWD_TOL, c.o_emu)
    _slice_check(f"{name} attn lse2", lse[: nH * M].view(nH, M).t(), c.lse_ref, c, nH, LSE_TOL)
    dqkv = _bwd(c, o, lse)
    _check_bwd(c, f"{name} attn bwd", dqkv)
    o2, lse2 = _fwd(c)
    assert torch.equal(_bits(o), _bits(o2)) and torch.equal(_bits(lse), _bits(lse2)), "attention forward is not bit-reproducible"
    assert torch.equal(_bits(dqkv), _bits(_bwd(c, o, lse))), "attention backward is not bit-reproducible"
    c.out = (o, lse, dqkv)


@pytest.mark.parametrize("nH,nKV,hd", [(12, 2, 128), (14, 2, 64)])
def test_attention_segment_permutation_is_exact(nH, nKV, hd):
    """Segment lengths that are multiples of 128: every tile walk depends only on offsets relative to a 128-aligned segment
    start and the chunk partials are added in chunk order, so permuting the segments permutes o, lse and dqkv bit for bit
    (whatever the heaviest-first block order and the XCD grouping do with the launch)."""
    segs, perm = [1024, 256, 2048, 128, 640], [3, 0, 4, 2, 1]
    M, ld, qkv, seg_s, seg_e = _attn_case(segs, nH, nKV, seed=7, hd=hd)
    d_o = rnd(M, nH * hd, seed=9)
    qkv, _ = _attn_prescale(qkv, nH, hd)
    starts = [sum(segs[:i]) for i in range(len(segs))]
    rows = torch.cat([torch.arange(starts[i], starts[i] + segs[i]) for i in perm])  # row of the original at each permuted row
    segs_p = [segs[i] for i in perm]
    _, _, _, seg_s_p, seg_e_p = _attn_case(segs_p, nH, nKV, seed=7, hd=hd)
    outs = []
    for q_, do_, ss_, se_ in ((qkv, d_o, seg_s, seg_e), (qkv[rows], d_o[rows], seg_s_p, seg_e_p)):
        c = SimpleNamespace(M=M, ld=ld, nH=nH, nKV=nKV, hd=hd, qd=dev_bf16(q_), dod=dev_bf16(do_), ss=ss_.cuda(), se=se_.cuda())
        o, lse = _fwd(c)
        outs.append((o[:M], lse[: nH * M].view(nH, M), _bwd(c, o, lse)[:M]))
    r = rows.cuda()
    (o0, l0, d0), (o1, l1, d1) = outs
    assert torch.equal(_bits(o0[r]), _bits(o1)), "o"
    assert torch.equal(_bits(l0[:, r].contiguous()), _bits(l1.contiguous())), "lse"
    assert torch.equal(_bits(d0[r]), _bits(d1)), "dqkv"


@pytest.mark.parametrize("name", ["slam358m_step", "long_single"])
def test_attention_bwd_launch_shapes_at_step_shapes(name):
    """Every backward launch shape (attn_jq 1 / 2 x attn_nch 1..4) at M = 8192: against fp64 per slice, and bit-reproducible."""
    c = _case(name)
    o, lse, _ = _outputs(c)
    L = lib()
    try:
        for jq, nch in product((1, 2), (1, 2, 3, 4)):
            assert L.slam_set_option(None, b"attn_jq", jq) == 0 and L.slam_set_option(None, b"attn_nch", nch) == 0
            d1, d2 = _bwd(c, o, lse), _bwd(c, o, lse)
            assert torch.equal(_bits(d1), _bits(d2)), f"jq={jq} nch={nch}: attention backward is not bit-reproducible"
            _check_bwd(c, f"{name} jq={jq} nch={nch} attn bwd", d1)
    finally:
        for k, v in (("attn_jq", 1), ("attn_kw", 1), ("attn_nch", 4)):
            L.slam_set_option(None, k.encode(), v)


def test_attention_plan_refuses_work_lists_beyond_lds():
    """attn_plan ranks its work list (11 ints per 128 rows) in one block's 48 KB of LDS: M = 143,360 needs 12,320 ints and
    must be refused with an error code, not launched."""
    M, nH, nKV, hd = 143360, 1, 1, 64
    qkv = torch.zeros(M, 3 * hd, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(M, hd, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(M, dtype=torch.float32, device="cuda")
    ss = torch.zeros(M, dtype=torch.int32, device="cuda")
    rc = lib().slam_op_attn_fwd(ptr(qkv), ptr(o), ptr(lse), ptr(ss), M, nH, nKV, hd, stream())
    sync()
    assert rc != 0


# ----------------------------------------------------------------------------------------- B2
def _packed_positions(segs):
    return torch.cat([torch.arange(n) for n in segs]).cuda()


@pytest.mark.parametrize("name", ["ragged_hd64", "ragged_hd128", "slam358m_step", "configs3_packed"])
def test_attention_bwd_rotated(name):
    """slam_op_attn_bwd_rope - the backward slam_backward runs: dq is rotated back in the dQ kernel's store, dk in the
    chunk-reduce kernel. dq / dk against the fp64 dq / dk taken through the transpose rotation in fp64 (B1 tolerances, per
    slice), dense (positions m % T) and packed (positions restarting per segment); the dv columns equal slam_op_attn_bwd's
    bit for bit; with all positions 0 (cos = 1, sin = 0: OPT's identity tables) the whole output equals slam_op_attn_bwd's
    as values (a * 1 + b * 0 returns a; a zero may change its sign)."""
    c = _case(name)
    o, lse, plain = _outputs(c)
    M, nH, nKV, hd = c.M, c.nH, c.nKV, c.hd
    b = (nH + nKV) * hd
    theta = 1e4 if hd == 64 else 1e6
    T = 1024 if name == "slam358m_step" else M  # dense: the row length of the batch
    variants = [("dense", None, torch.arange(M, device="cuda") % T), ("packed", _packed_positions(c.segs), None)]
    for tag, ids, pos in variants:
        pos = ids if pos is None else pos
        d = _bwd(c, o, lse, rope=(ids, T, theta))
        _check_bwd(c, f"{name} rotated {tag} attn bwd", d, rot=lambda t, heads: _rope64_transpose(t, pos, theta, heads))
        assert torch.equal(_bits(d[:M, b:]), _bits(plain[:M, b:])), f"{tag}: dv differs from slam_op_attn_bwd's"
    zeros = torch.zeros(M, dtype=torch.int64, device="cuda")
    d = _bwd(c, o, lse, rope=(zeros, T, theta))
    assert torch.equal(d[:M], plain[:M]), "identity tables: output differs from slam_op_attn_bwd's"


# ----------------------------------------------------------------------------------------- B3
def _drnd(*shape, seed, scale=1.0, offset=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(*shape, generator=g, device="cuda") * scale
    return (x if offset is None else x + offset).to(torch.bfloat16)


@pytest.mark.parametrize("M,N,K,q_heads,rope_heads,zero_pos", [
    (8192, 1152, 896, 14, 16, False), (8192, 2304, 768, 12, 24, False), (8192, 2304, 768, 12, 24, True),
    (8192, 6144, 2048, 32, 64, False), (300, 384, 256, 2, 4, False), (74, 384, 256, 2, 4, False)])
def test_gemm_nt_rope(M, N, K, q_heads, rope_heads, zero_pos):
    """The fused QKV projection against fp64 rope(X W^T + b), query heads times 64^-0.5 * log2(e), V columns unrotated, at
    test_gemm_nt's tolerance (4e-3 rel-RMS, 2e-2 of the abs-max: one rounding of an fp32 value) on the q, k and v column
    groups separately. The rotation exists three times in gemm.hip: gemm_mf32 = 0 / gemm_256 = 0 runs the 16x16x32 epilogue
    of the 128 x 128 kernel, gemm_mf32 = 1 / gemm_256 = 0 its 32x32x16 epilogue, gemm_256 = 2 the 256 x 256 kernel where M and
    N are multiples of 256 and there are >= 256 tiles (N = 2304 and 6144: 288 and 768 tiles; the other shapes stay on the 128 x 128
    kernel). Dense positions (m % M: up to
    8191, where the fp32 angle of the table is least accurate) and position_ids (restarting segments, then a run counting down
    from 8191); all-zero positions = OPT's identity rotation. NaN-prefilled output, canary rows behind row M."""
    X, W, bias = _drnd(M, K, seed=1), _drnd(N, K, seed=2, scale=0.05), _drnd(N, seed=3)
    Yl = X.double() @ W.double().t() + bias.double()
    qscale = 64 ** -0.5 * LOG2E
    theta = 10000.0
    h = M // 2
    ids = torch.cat([torch.arange(n) for n in (h // 3, 1, h - h // 3 - 1)] + [8191 - torch.arange(M - h)]).cuda()
    if zero_pos:
        variants = [("zero", torch.zeros(M, dtype=torch.int64, device="cuda"))]
    else:
        variants = [("dense", None), ("packed", ids)]
    nq, nr = q_heads * 64, rope_heads * 64
    L = lib()
    tab = _guarded(4 * M * 32, 1, torch.float32)
    try:
        for tag, pid in variants:
            pos = torch.arange(M, device="cuda") if pid is None else pid
            ref = Yl.clone().view(M, N // 64, 64)
            ref[:, :rope_heads] = _rope64(ref[:, :rope_heads], pos, theta)
            ref[:, :q_heads] *= qscale
            ref = ref.view(M, N)
            for mf32, g256 in product((0, 1), (0, 2)):
                assert L.slam_set_option(None, b"gemm_mf32", mf32) == 0 and L.slam_set_option(None, b"gemm_256", g256) == 0
                Y = _guarded(M, N, torch.bfloat16)
                rc = L.slam_op_gemm_nt_rope(ptr(X), ptr(W), ptr(Y), ptr(bias), ptr(pid), theta, q_heads, rope_heads, M, M, N, K,
                                            ptr(tab), stream())
                sync()
                assert rc == 0
                assert _guard_ok(Y, M) and _guard_ok(tab, 4 * M * 32), "gemm_nt_rope wrote behind its output or tables"
                name = f"gemm_nt_rope {M}x{N}x{K} {tag} mf32={mf32} gemm_256={g256}"
                _dcheck(f"{name} q", Y[:M, :nq], ref[:, :nq], 4e-3, 2e-2)
                _dcheck(f"{name} k", Y[:M, nq:nr], ref[:, nq:nr], 4e-3, 2e-2)
                _dcheck(f"{name} v", Y[:M, nr:], ref[:, nr:], 4e-3, 2e-2)
    finally:
        L.slam_set_option(None, b"gemm_mf32", 0)
        L.slam_set_option(None, b"gemm_256", 1)


# ----------------------------------------------------------------------------------------- B4
@pytest.mark.parametrize("M,N,ld", [(8192, 1152, 0), (16384, 2048, 0), (8192, 2304, 0), (8192, 3072, 0), (8192, 8192, 0), (8192, 768, 0),
                                    (4099, 896, 0), (1, 256, 0), (15, 256, 0), (17, 264, 0), (333, 1160, 0), (4099, 896, 1160)])
def test_colsum(M, N, ld):
    """slam_op_colsum (colsum_bf16 into partial rows + colsum_finish_many: every bias gradient of the backward) against fp64
    column sums of inputs with a per-column offset (the mean matters: a dropped row shows), 1e-5 rel-RMS - the bar
    test_layernorm_fwd_bwd holds an fp32 column reduction over 8192 bf16 rows to. ld > N: a column window of a wider matrix.
    accumulate = 0 onto a 7.0-prefilled output, then 1 onto the result (== 2x); bit-identical across two runs; the elements
    behind out[N] and behind the workspace untouched."""
    ld = ld or N
    c0 = 136 if ld > N else 0  # first column of the window
    off = ((torch.arange(ld, device="cuda") % 7) - 3).float() * 0.25
    Xw = _drnd(M, ld, seed=11, offset=off)
    X = Xw[:, c0:]
    ref = Xw[:, c0:c0 + N].double().sum(0)
    L = lib()
    nws = L.slam_op_colsum_workspace(M, N) // 4
    assert nws > 0
    outs = []
    for run in range(2):
        ws = _guarded(nws, 1, torch.float32)
        out = torch.full((N + GUARD,), 7.0, dtype=torch.float32, device="cuda")
        out[N:] = SENT
        assert L.slam_op_colsum(ptr(X), ld, M, N, ptr(out), 0, ptr(ws), stream()) == 0
        sync()
        first = out.clone()
        assert L.slam_op_colsum(ptr(X), ld, M, N, ptr(out), 1, ptr(ws), stream()) == 0
        sync()
        assert _guard_ok(out, N) and _guard_ok(ws, nws), "colsum wrote behind its output or workspace"
        outs.append((first, out))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1])), \
        "colsum is not bit-reproducible"
    _dcheck(f"colsum {M}x{N} ld={ld}", outs[0][0][:N], ref, 1e-5, 1e-4)
    _dcheck(f"colsum accumulate {M}x{N} ld={ld}", outs[0][1][:N], 2 * ref, 1e-5, 1e-4)
