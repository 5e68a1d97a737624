"""Float64 restatement of HF's Adafactor over a flat buffer and a segment table, an fp32 emulation that sums in the kernels' stated
order, the synthetic table of the GPU tests and the per-element acceptance bound. numpy only: nothing here needs a GPU.

THE DEFINITION (transformers.optimization.Adafactor as Trainer builds it: scale_parameter = False, relative_step = False, beta1 =
None, eps = (1e-30, 1e-3), clip_threshold = 1, decay_rate = -0.8), per segment at step t (1-based):

    g = grad * cs      beta = 1 - t^decay_rate      s = g^2 + eps1
    matrix [R][C]:  row <- beta row + (1 - beta) mean_c s     col <- beta col + (1 - beta) mean_r s
                    u = g rsqrt(row / mean(row)) rsqrt(col)
    vector:         v <- beta v + (1 - beta) s                u = g rsqrt(v)
    d = max(1, sqrt(mean u^2) / clip_threshold)      p <- p - wd lr p      p <- p - lr u / d

A table entry is (offset, rows, cols, factored, pattern) - include/slam_engine.h SlamAdafactorSegment: pattern 0 = contiguous
rows, 1 / 2 = groups of 32 rows every 64 behind `offset`, phase 0 / 32. The state buffer holds, per segment in table order and
without gaps, rows + cols floats (row factors, then column factors) when factored, cols when not. u does not depend on p
(scale_parameter is off), so the state trajectory is a function of the gradients alone.

THE BOUND. eps = 2^-24 is the unit roundoff of fp32. Every quantity the kernels sum is positive, so a sum in which a term passes
through at most A additions has a relative error of at most A eps on top of its terms' (first order; the second-order terms
are below 1e-3 of the first at the lengths that occur). With the tile of csrc/adafactor.hip (256 rows x 256 columns; n_rb, n_cb
= the segment's row and column blocks) and the orders stated at the top of that file:

    s                      4     the product g cs, its square, the fused add of eps1, eps1's own rounding to fp32
    row sum                A_row = 7 + 5 + (n_cb - 1)      8 values in a thread, the 5 butterfly levels, the column blocks
    column sum             A_col = 31 + 7 + (n_rb - 1)     32 rows in a thread, the 8 threads of a column, the row blocks
    factor after step t    E_row = 4 + A_row + 4 + t       (E_col alike) the division by the length, beta and 1 - beta rounded
                                                           to fp32, the product and the fused add; a convex combination of positive
                                                           numbers keeps the larger relative error of the two and adds the blend's
                                                           own rounding - one eps per step on the old factor, hence + t
    mean of the rows       E_mean = E_row + (ceil(R / 256) - 1) + 8 + 1
    row factor rsqrt(row / mean)   E_rf = (E_row + E_mean + 1) / 2 + 2      the square root halves, then its rounding and the division's
    column factor          E_cf = E_col / 2 + 2
    u                      E_u = E_rf + E_cf + 3           the product of the factors, g cs, their product
    vector                 E_v = 4 + 4 + t,  E_u = E_v / 2 + 2 + 2
    sum of u^2, one tile   2 E_u + 1 + 255 + 6 + 3         256 values in a thread, the 6 butterfly levels, the 4 waves; the tiles
                                                           are added in fp64 (nothing at this scale)
    d                      E_d = (2 E_u + 265) / 2 + 3     square root, the rounding to fp32, the division by clip_threshold
    lr u / d               E_upd = E_u + E_d + 3           the division, the product, lr rounded to fp32

    |p_gpu - p_ref| <= eps (E_upd |lr u / d| + 3 |p| + 3 |wd lr p|)       one step, from the stored p

(the decay's fused multiply-add and the final subtraction each round once at the size of p; wd lr is rounded to fp32.) max(1, .) is
1-Lipschitz, so E_d holds across its kink. A bf16 parameter store adds nothing to the bound: the stored value must lie between
the bf16 roundings of ref - bound and ref + bound (stochastic rounding: between the bf16 neighbours of that interval). The state
is held to E_row eps / E_col eps / E_v eps relative. The bound is a property of the kernels' stated orders and never moves because
a run was outside it: tests/test_adafactor_host.py puts the fp32 emulation below through it on the GPU tests' own inputs and
requires zero violations, every element included."""
import math

import numpy as np

EPS32 = 2.0 ** -24
TILE_R, TILE_C = 256, 256
HF_DEFAULTS = dict(eps1=1e-30, clip_threshold=1.0, decay_rate=-0.8)


# ------------------------------------------------------------------------------------------------ table helpers
def seg_state_floats(ent):
    _, rows, cols, factored, _ = ent
    return rows + cols if factored else cols


def state_offsets(table):
    offs, o = [], 0
    for ent in table:
        offs.append(o)
        o += seg_state_floats(ent)
    return offs, o


def seg_index(ent):
    """int64 [rows][cols]: the flat index of every element of a segment"""
    off, rows, cols, _, pattern = ent
    r = np.arange(rows, dtype=np.int64)
    prow = r if pattern == 0 else (r // 32) * 64 + (32 if pattern == 2 else 0) + r % 32
    return off + prow[:, None] * cols + np.arange(cols, dtype=np.int64)[None, :]


def covered(table, n):
    m = np.zeros(n, dtype=bool)
    for ent in table:
        idx = seg_index(ent).reshape(-1)
        assert not m[idx].any(), "segments overlap"
        m[idx] = True
    return m


def beta_of(t, decay_rate=-0.8):
    return 1.0 - math.pow(float(t), decay_rate)


# ------------------------------------------------------------------------------------------------ bf16
def bf16_rne(x64):
    """float64 -> the float64 value of the nearest bfloat16 (ties to even), through fp32 (exact for fp32-representable input and
    a correct rounding for everything the tests hand over: |x| far from the fp32 limits)"""
    x32 = np.asarray(x64, dtype=np.float64).astype(np.float32)
    b = x32.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_floor_ceil(x64):
    r = bf16_rne(x64)
    b = r.astype(np.float32).view(np.uint32)
    pos = r >= 0
    up = np.where(pos, b + 0x10000, b - 0x10000).astype(np.uint32).view(np.float32).astype(np.float64)
    dn = np.where(pos, b - 0x10000, b + 0x10000).astype(np.uint32).view(np.float32).astype(np.float64)
    zero = r == 0
    tiny = float(np.uint32(0x00010000).view(np.float32))
    up, dn = np.where(zero, tiny, up), np.where(zero, -tiny, dn)
    return np.where(r > x64, dn, r), np.where(r < x64, up, r)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def step_f64(p, g, state, table, t, lr, cs=1.0, wd=0.0, eps1=1e-30, clip_threshold=1.0, decay_rate=-0.8, want_terms=False):
    """One step over float64 arrays p, g [n] and state [state floats] -> (p', state'). wd: a number, or one per segment. Elements
    outside the table keep their values. want_terms: also the per-element float64 arrays (|lr u / d|, |p|, |wd lr p|) of the bound
    and the per-segment d."""
    p, state = np.array(p, dtype=np.float64), np.array(state, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    beta = beta_of(t, decay_rate)
    offs, _ = state_offsets(table)
    upd_abs, dec_abs, ds = np.zeros_like(p), np.zeros_like(p), []
    for k, ent in enumerate(table):
        _, rows, cols, factored, _ = ent
        idx = seg_index(ent)
        ge = g[idx] * cs
        s = ge * ge + eps1
        so = offs[k]
        if factored:
            row = beta * state[so:so + rows] + (1.0 - beta) * s.mean(axis=1)
            col = beta * state[so + rows:so + rows + cols] + (1.0 - beta) * s.mean(axis=0)
            state[so:so + rows], state[so + rows:so + rows + cols] = row, col
            u = ge / np.sqrt(row / row.mean())[:, None] / np.sqrt(col)[None, :]
        else:
            v = beta * state[so:so + cols] + (1.0 - beta) * s[0]
            state[so:so + cols] = v
            u = ge / np.sqrt(v)[None, :]
        d = max(1.0, math.sqrt(float(np.mean(u * u))) / clip_threshold)
        w = float(wd[k]) if np.ndim(wd) else float(wd)
        p0 = p[idx]
        dec = w * lr * p0
        upd = lr * u / d
        p[idx] = (p0 - dec) - upd
        upd_abs[idx], dec_abs[idx] = np.abs(upd), np.abs(dec)
        ds.append(d)
    if want_terms:
        return p, state, (upd_abs, dec_abs, np.array(ds))
    return p, state


def named_step_f64(params, grads, state, t, lr, cs=1.0, wd=0.0, decayed=None):
    """The same step over {HF name: float64 array} (1-D: a vector, 2-D: factored) in place; state: {name: float64 factors} as
    step_f64 lays them out per segment (created on first use). decayed(name) -> bool picks the tensors wd applies to."""
    for k, p in params.items():
        shp = p.shape
        ent = (0, shp[0], shp[1], 1, 0) if p.ndim == 2 else (0, 1, shp[0], 0, 0)
        st = state.setdefault(k, np.zeros(seg_state_floats(ent)))
        w = wd if decayed is None or decayed(k) else 0.0
        pn, sn = step_f64(p.reshape(-1), np.asarray(grads[k], dtype=np.float64).reshape(-1), st, [ent], t, lr, cs=cs, wd=w)
        p[...] = pn.reshape(shp)
        st[...] = sn


# ------------------------------------------------------------------------------------------------ the bound
def seg_budget(ent, t):
    """(E_upd, [E of the segment's state floats]) in units of eps for a segment at step t: the derivation of the module docstring"""
    _, rows, cols, factored, _ = ent
    n_rb, n_cb = -(-rows // TILE_R), -(-cols // TILE_C)
    if factored:
        e_row = 4 + (7 + 5 + n_cb - 1) + 4 + t
        e_col = 4 + (31 + 7 + n_rb - 1) + 4 + t
        e_mean = e_row + (-(-rows // 256) - 1) + 8 + 1
        e_rf = (e_row + e_mean + 1) / 2 + 2
        e_cf = e_col / 2 + 2
        e_u = e_rf + e_cf + 3
        e_state = np.concatenate([np.full(rows, float(e_row)), np.full(cols, float(e_col))])
    else:
        e_v = 4 + 4 + t
        e_u = e_v / 2 + 2 + 2
        e_state = np.full(cols, float(e_v))
    e_d = (2 * e_u + 265) / 2 + 3
    return e_u + e_d + 3, e_state


def bounds(table, t, n, terms, p_ref):
    """Per-element bound on p' (float64 [n], 0 outside the table) and the relative bound of every state float, for step t; terms:
    step_f64's, p_ref its p'"""
    upd_abs, dec_abs, _ = terms
    b, st = np.zeros(n), []
    for ent in table:
        idx = seg_index(ent)
        e_upd, e_state = seg_budget(ent, t)
        b[idx] = EPS32 * (e_upd * upd_abs[idx] + 3.0 * np.abs(p_ref[idx]) + 3.0 * dec_abs[idx])
        st.append(e_state * EPS32)
    return b, np.concatenate(st)


def violations_f32(got, ref, bound, where):
    """number of elements of `where` with |got - ref| > bound; NaN counts"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return int((~(err <= bound) & where).sum())


def violations_bf16(got, ref, bound, where, sr=False):
    got = np.asarray(got, dtype=np.float64)
    if sr:
        lo, hi = bf16_floor_ceil(ref - bound)[0], bf16_floor_ceil(ref + bound)[1]
    else:
        lo, hi = bf16_rne(ref - bound), bf16_rne(ref + bound)
    return int((~((lo <= got) & (got <= hi)) & where).sum())


# ------------------------------------------------------------------------------------------------ fp32 emulation, kernel order
F = np.float32


def _seq_sum(x, axis):
    """left-to-right fp32 sum along `axis`"""
    x = np.moveaxis(x, axis, 0)
    acc = x[0].copy()
    for k in range(1, x.shape[0]):
        acc = acc + x[k]
    return acc


def _fold(x, axis):
    """the xor butterfly / halving tree along `axis` (a power of two): halves added until one value is left"""
    x = np.moveaxis(x, axis, 0)
    while x.shape[0] > 1:
        h = x.shape[0] // 2
        x = x[:h] + x[h:]
    return x[0]


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64"""
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def step_f32_emulated(p, g, state, table, t, lr, cs=1.0, wd=0.0, eps1=1e-30, clip_threshold=1.0, decay_rate=-0.8):
    """The step in fp32, every sum in the order csrc/adafactor.hip states: fp32 arrays in, (p', state') fp32 out."""
    p, state = np.array(p, dtype=F), np.array(state, dtype=F)
    g = np.asarray(g, dtype=F)
    beta64 = beta_of(t, decay_rate)
    beta, omb = F(beta64), F(1.0 - beta64)
    lr32, cs32, eps32, clip32 = F(lr), F(cs), F(eps1), F(clip_threshold)
    offs, _ = state_offsets(table)
    for k, ent in enumerate(table):
        _, rows, cols, factored, _ = ent
        idx = seg_index(ent)
        n_rb, n_cb = -(-rows // TILE_R), -(-cols // TILE_C)
        Rp, Cp = n_rb * TILE_R, n_cb * TILE_C
        ge = g[idx] * cs32
        s = np.zeros((Rp, Cp), dtype=F)
        s[:rows, :cols] = _fma32(ge, ge, eps32)
        so = offs[k]
        if factored:
            # rows: 8 values of a thread left to right, the 32 lanes of the row by the butterfly, the column blocks in order
            rp = _fold(_seq_sum(s.reshape(Rp, n_cb, 32, 8), 3), 2)
            rsum = _seq_sum(rp, 1)[:rows]
            # columns: a thread's rows i = 0 .. 31 (row = rb 256 + rs + 8 i), the 8 threads rs in order, the row blocks in order
            cpart = _seq_sum(_seq_sum(s.reshape(n_rb, 32, 8, Cp), 1), 1)
            csum = _seq_sum(cpart, 0)[:cols]
            row = _fma32(np.full(rows, beta), state[so:so + rows], omb * (rsum / F(cols)))
            col = _fma32(np.full(cols, beta), state[so + rows:so + rows + cols], omb * (csum / F(rows)))
            state[so:so + rows], state[so + rows:so + rows + cols] = row, col
            rpad = np.zeros(-(-rows // 256) * 256, dtype=F)
            rpad[:rows] = row
            mean = _fold(_seq_sum(rpad.reshape(-1, 256), 0), 0) / F(rows)
            rf = F(1.0) / np.sqrt(row / mean)
            cf = F(1.0) / np.sqrt(col)
            u = (rf[:, None] * cf[None, :]) * ge
        else:
            v = _fma32(np.full(cols, beta), state[so:so + cols], omb * s[0, :cols])
            state[so:so + cols] = v
            u = (F(1.0) / np.sqrt(v))[None, :] * ge
        uu = np.zeros((Rp, Cp), dtype=F)
        uu[:rows, :cols] = u * u
        # a tile: thread (rs, cg) adds rows i in order and the 8 values of a row left to right; lanes by the butterfly (a wave =
        # two rs of 32 cg), the 4 waves in order; the tiles in fp64
        x = uu.reshape(n_rb, 32, 8, n_cb, 32, 8).transpose(0, 3, 2, 4, 1, 5).reshape(n_rb, n_cb, 8, 32, 256)
        th = _seq_sum(x, 4).reshape(n_rb, n_cb, 4, 64)
        tiles = _seq_sum(_fold(th, 3), 2)
        rms = F(math.sqrt(float(tiles.astype(np.float64).sum()) / (rows * cols)))
        d = max(F(1.0), rms / clip32)
        w = F(wd[k]) if np.ndim(wd) else F(wd)
        p0 = p[idx]
        pd = _fma32(np.full(p0.shape, -(w * lr32)), p0, p0)
        p[idx] = pd - (u / d) * lr32
    return p, state


# ------------------------------------------------------------------------------------------------ the HF fixture's models and inputs
# One decoder layer of the narrowest body the engine takes per family: the fixture stores float64 parameters per HF name, and a
# committed file stays below 1 MiB. The tied Qwen2 keeps the 502-row vocabulary (a 512-row slot with 10 pad rows).
_QWEN = dict(num_hidden_layers=1, hidden_size=64, num_attention_heads=1, num_key_value_heads=1, head_dim=64, intermediate_size=64,
             rms_norm_eps=1e-6, rope_theta=10000.0, initializer_range=0.02)
FAMILIES = {
    "qwen2_tied": (dict(_QWEN, tie_word_embeddings=True), 502),
    "qwen2_untied": (dict(_QWEN, tie_word_embeddings=False), 48),
    "opt": (dict(model_type="opt", num_hidden_layers=1, hidden_size=64, num_attention_heads=1, ffn_dim=64, max_position_embeddings=30,
                 init_std=0.02, tie_word_embeddings=True), 48),
    "qwen3": (dict(_QWEN, model_type="qwen3", tie_word_embeddings=True), 48),
}
HF_STEPS, HF_LR, HF_WD, HF_CS = 3, 2.0 ** -6, 0.125, 0.375     # exact in fp32: HF's doubles and the engine's floats are one number


def hash_values(n, seed, scale):
    """n reproducible float64 values k / 128 * scale, k an integer in [-128, 127] (exact in bf16 for a power-of-two scale), from
    splitmix64 of (seed, index): integer arithmetic only, the same on every platform"""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(56)).astype(np.float64) - 128.0) / 128.0 * scale


def hf_inputs(names_shapes):
    """{name: (p0, [g_1 .. g_HF_STEPS])} float64 arrays of bf16-exact values for the fixture's parameter list; the gradient scale
    moves with the name and the step so that the update clip bites on some tensors and not on others"""
    out = {}
    for k, (name, shape) in enumerate(names_shapes):
        n = int(np.prod(shape))
        p0 = hash_values(n, 7 * k + 1, 2.0 ** -4).reshape(shape)
        gs = [hash_values(n, 1000 * (t + 1) + k, 2.0 ** (-3 - (k % 3) * 2 + (t if k % 2 else -t))).reshape(shape) for t in range(HF_STEPS)]
        out[name] = (p0, gs)
    return out


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def synthetic_table():
    """The smallest shapes at which the indexing can go wrong, laid over one flat buffer with guard gaps between the slots ->
    (table, names, n, pad) - pad: the elements of the 512-row slot behind the 502 x 64 matrix."""
    table, names = [], []
    o = 64                                        # a guard in front

    def add(name, rows, cols, factored, pattern=0, at=None):
        table.append((o if at is None else at, rows, cols, int(factored), pattern))
        names.append(name)

    add("embed 502x64 in a 512-row slot", 502, 64, True)
    pad = (o + 502 * 64, o + 512 * 64)
    o += 512 * 64 + 64
    add("gate 96x72", 96, 72, True, 1)
    add("up 96x72", 96, 72, True, 2)
    o += 192 * 72 + 64
    for nm, r in (("q 128x72", 128), ("k 64x72", 64), ("v 64x72", 64)):
        add(nm, r, 72, True)
        o += r * 72
    o += 64
    add("wide 96x2056", 96, 2056, True)
    o += 96 * 2056 + 64
    add("tall 2050x8", 2050, 8, True)
    o += 2050 * 8 + 64
    for nm, c in (("vec 8", 8), ("vec 72", 72), ("vec 200", 200)):
        add(nm, 1, c, False)
        o += c + 8
    for nm, c in (("bias q 128", 128), ("bias k 64", 64), ("bias v 64", 64)):
        add(nm, 1, c, False)
        o += c
    o += 64
    return table, names, o, pad


SYN_LR, SYN_WD, SYN_CS = 2.0 ** -6, 0.125, 0.375      # exact in fp32; a clip coefficient != 1


def synthetic_inputs(n, steps=3, seed=0, bf16_values=False):
    """p0 and `steps` fresh gradients for a buffer of n elements, float64 arrays of fp32- (bf16_values: bf16-) representable numbers.
    The gradient scale differs per 1000-element stretch so that some segments have RMS(u) above and some below the clip."""
    rng = np.random.default_rng(seed)
    rnd = bf16_rne if bf16_values else (lambda x: x.astype(np.float32).astype(np.float64))
    p0 = rnd(0.05 * rng.standard_normal(n))
    gs = [rnd(rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1, size=n // 8 + 1).repeat(8)[:n]) for _ in range(steps)]
    return p0, gs
