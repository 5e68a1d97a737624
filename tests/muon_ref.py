"""The Muon rule of include/slam_engine.h (slam_muon_step) restated on the CPU: torch.optim.Muon as torch 2.10 defines it, with
the bf16 / fp32 roundings at exactly the stated points and the products accumulated in float64 (or, for the tolerance, in float32
over a permuted contraction order).

    prepare_f32   B <- mu B + (1 - mu) g, U, X = bf16(U): fp32, every operation rounded by itself - the engine's bits
    orthogonalize X / max(bf16(|X|), bf16(eps)), then ns_steps x { A = X X^T; P = b A + c A A; X <- a X + P X }, each product
                  rounded to bf16 once after its epilogue
    apply_f32     p <- p (1 - lr wd); p <- p - lr_adj O: fp32, every operation rounded by itself - the engine's bits
    bar           max(4 s, 2^-8), s = relative Frobenius distance between the float64 and the permuted-float32 restatement ON THE
                  SAME INPUT: the engine's MFMA order is a third summation order, and a tiny matrix flips almost no rounding
"""
import math

import numpy as np
import torch

A, B, C = 3.4445, -4.7750, 2.0315
EPS = 1e-7
F32 = np.float32


def bf16(x) -> np.ndarray:
    """Round to bf16 (nearest even), returned as float32 values."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).bfloat16().float().numpy()


def bf16_bits(x) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).bfloat16().view(torch.int16).numpy()


def lr_ratio(adjust, rows, cols) -> float:
    if adjust == "match_rms_adamw":
        return 0.2 * math.sqrt(max(rows, cols))
    if adjust == "original":
        return math.sqrt(max(1, rows / cols))
    assert adjust is None, adjust
    return 1.0


def prepare_f32(g, buf, cs=1.0, mu=0.95, nesterov=True):
    """(new momentum buffer fp32, X = bf16(U) as float32) for one matrix; g / buf float32 arrays, cs the clip coefficient."""
    mu32, omm32 = F32(mu), F32(1.0 - mu)
    gg = (np.asarray(g, F32) * F32(cs)).astype(F32)
    y = (omm32 * gg).astype(F32)
    bn = ((mu32 * np.asarray(buf, F32)).astype(F32) + y).astype(F32)
    u = (y + (mu32 * bn).astype(F32)).astype(F32) if nesterov else bn
    return bn, bf16(u)


def _mm(x, y, acc, perm_seed):
    """x @ y: float64 accumulation, or float32 accumulation over a permuted contraction order."""
    if acc == "f64":
        return x.astype(np.float64) @ y.astype(np.float64)
    perm = np.random.default_rng(perm_seed).permutation(x.shape[1])
    return (np.ascontiguousarray(x[:, perm], F32) @ np.ascontiguousarray(y[perm, :], F32)).astype(np.float64)


def orthogonalize(x, ns_steps=5, coef=(A, B, C), eps=EPS, acc="f64", normalise=True, perm_seed=0):
    """The orthogonalised update O [rows][cols] (bf16 values as float32) of X [rows][cols] (bf16 values)."""
    x = np.asarray(x, F32)
    rows, cols = x.shape
    if rows > cols:
        x = np.ascontiguousarray(x.T)
    a, b, c = (F32(v) for v in coef)
    if normalise:
        nrm = max(bf16(F32(math.sqrt(float((x.astype(np.float64) ** 2).sum()))))[()], bf16(F32(eps))[()])
        x = bf16((x / F32(nrm)).astype(F32))
    for it in range(ns_steps):
        g = bf16(_mm(x, x.T, acc, perm_seed + 3 * it))
        p = bf16(np.float64(b) * g + np.float64(c) * _mm(g, g, acc, perm_seed + 3 * it + 1))
        x = bf16(np.float64(a) * x + _mm(p, x, acc, perm_seed + 3 * it + 2))
    return np.ascontiguousarray(x.T) if rows > cols else x


def rel_dist(x, ref) -> float:
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def bar(x, ns_steps=5, coef=(A, B, C), eps=EPS):
    """(bar, s, O_f64) for the input X: max(4 s, 2^-8)."""
    o64 = orthogonalize(x, ns_steps, coef, eps, "f64")
    s = rel_dist(orthogonalize(x, ns_steps, coef, eps, "f32perm"), o64)
    return max(4.0 * s, 2.0 ** -8), s, o64


def apply_f32(p, o, lr, wd, adjust, rows, cols):
    """p (float32) after the apply; o = bf16 values as float32."""
    decay, lr_adj = F32(1.0 - lr * wd), F32(lr * lr_ratio(adjust, rows, cols))
    d = (np.asarray(p, F32) * decay).astype(F32)
    return (d - (lr_adj * np.asarray(o, F32)).astype(F32)).astype(F32)


def step(p, g, buf, lr, wd=0.0, mu=0.95, nesterov=True, ns_steps=5, adjust="match_rms_adamw", cs=1.0, acc="f64"):
    """One Muon step of one matrix: (p', buf', O)."""
    rows, cols = p.shape
    buf, x = prepare_f32(g, buf, cs, mu, nesterov)
    o = orthogonalize(x, ns_steps, acc=acc)
    return apply_f32(p, o, lr, wd, adjust, rows, cols), buf, o


def seg_rows(entry):
    """Flat indices [rows][cols] of a Muon table row (offset, rows, cols, pattern)."""
    off, rows, cols, pat = entry
    r = np.arange(rows)
    prow = r if pat == 0 else (r // 32) * 64 + (0 if pat == 1 else 32) + r % 32
    return off + prow[:, None] * cols + np.arange(cols)[None, :]


def packed(x):
    """[n][m] image of an HF matrix: itself, or its transpose when rows > cols."""
    return np.ascontiguousarray(x.T) if x.shape[0] > x.shape[1] else np.ascontiguousarray(x)
