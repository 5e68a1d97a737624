"""numpy restatement of slam_spec_accept (include/slam_engine.h) and of one whole round of assisted generation given the
target's logits of the chunk: the draws come from tests/sampling_ref.py. Shared by tests/test_spec_host.py (hand-worked rows) and
tests/test_gpu_spec.py (the kernel and generate(assistant_model=) against it)."""
import numpy as np

from tests import sampling_ref as R

STATS = ("live", "max_lens_t", "max_lens_d", "emitted", "accepted")


def accept(chunk, tgt, n_new, done, prompt_len, out, K, max_new, pad_id, eos_ids):
    """One slam_spec_accept launch on copies of the arrays. chunk, tgt: int64 [B, K + 1]; n_new, prompt_len: int32 [B]; done:
    uint8 [B]; out: int64 [B, >= max_new]. Returns a dict of every array the kernel writes."""
    chunk, out = np.array(chunk, dtype=np.int64), np.array(out, dtype=np.int64)
    tgt = np.asarray(tgt, dtype=np.int64)
    n_new, done = np.array(n_new, dtype=np.int32), np.array(done, dtype=np.uint8)
    B = chunk.shape[0]
    assert chunk.shape == tgt.shape == (B, K + 1)
    lens_t, lens_d = np.zeros(B, np.int32), np.zeros(B, np.int32)
    draft_ids = np.zeros((B, 2), np.int64)
    draft_new_lens, tgt_new_lens = np.zeros(B, np.int32), np.zeros(B, np.int32)
    emitted = accepted = 0
    eos = set(int(e) for e in eos_ids)
    for b in range(B):
        nn = min(max(int(n_new[b]), 0), max_new)
        dn = bool(done[b])
        m = nacc = 0
        if not dn:
            while nacc < K and chunk[b, nacc + 1] == tgt[b, nacc]:
                nacc += 1
            m = min(nacc + 1, max_new - nn)
            for i in range(m):
                if int(tgt[b, i]) in eos:
                    m, dn = i + 1, True
                    break
            if nn + m >= max_new:
                dn = True
            out[b, nn:nn + m] = tgt[b, :m]
            emitted += m
            accepted += min(m, nacc)
        lag = int(m == K + 1)
        last = tgt[b, m - 1] if m > 0 else chunk[b, 0]
        d_k = chunk[b, K]
        n_new[b] = nn + m
        lens_t[b] = int(prompt_len[b]) + nn + m - 1
        lens_d[b] = lens_t[b] - lag
        chunk[b, 0] = last
        draft_ids[b] = (d_k, tgt[b, K]) if lag else (last, pad_id)
        draft_new_lens[b] = 0 if dn else 1 + lag
        tgt_new_lens[b] = 0 if dn else K + 1
        done[b] = int(dn)
    stats = np.array([int((done == 0).sum()), int(lens_t.max()), int(lens_d.max()), emitted, accepted], np.int32)
    return dict(chunk=chunk, n_new=n_new, done=done, out=out, lens_t=lens_t, lens_d=lens_d, draft_ids=draft_ids,
                draft_new_lens=draft_new_lens, tgt_new_lens=tgt_new_lens, stats=stats)


def target_tokens(logits_all, n_new, rows, banned, do_sample, top_k, temperature, top_p, seed, row_ids=None):
    """tgt [len(rows), K + 1] of slam_sample_tokens_at(group = K + 1, steps = n_new) on logits_all [B, K + 1, V] for the rows
    listed: column j is drawn with row id row_ids[b] (default b) at step n_new[b] + j, by the fp64 restatement. Also returns
    excluded [len(rows), K + 1]: the draws within 1e-5 of a boundary of the cumulative weights or of the top-p threshold (the
    exclusion of tests/test_gpu_sampling.py); greedy excludes nothing."""
    K1 = logits_all.shape[1]
    tgt = np.zeros((len(rows), K1), np.int64)
    excl = np.zeros((len(rows), K1), bool)
    for i, b in enumerate(rows):
        r = b if row_ids is None else int(row_ids[b])
        for j in range(K1):
            x = logits_all[b, j]
            if not do_sample:
                tgt[i, j] = R.greedy(x, banned)
                continue
            tok, dist, margin = R.sample_row(x, banned, top_k, temperature, top_p, seed, [r], [int(n_new[b]) + j], fp64=True)
            tgt[i, j] = tok[0, 0]
            excl[i, j] = dist[0, 0] <= 1e-5 or margin <= 1e-5
    return tgt, excl
