"""CPU tier of slam_extend (k tokens per row appended to a live KV cache) and of generate(prefill_chunk=): the three new
symbols are declared, exported and bound; every refusal that does not need a prefilled cache comes back with its code before
anything reaches the device (fake pointers, as in test_kv_abi.py; the batch-mismatch refusal needs a prefill and is checked in
test_gpu_extend.py); the workspace of a chunked prefill is smaller by host arithmetic; a bad prefill_chunk is a ValueError."""
import ctypes as C

import pytest

from slamkit_amd import engine as E

NEW = ["slam_extend", "slam_op_attn_extend", "slam_op_attn_extend_workspace"]
SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
OPT = (2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0)
E_INVAL, E_STATE, E_NOMEM = -1, -2, -3


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    assert hasattr(E.Engine, "extend")


def test_extend_refused_before_a_launch():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch

    def call(hh=h, ids=fake, new_lens=fake, lens=fake, B=2, T=16, logits=fake):
        return lib.slam_extend(hh, ids, new_lens, lens, B, T, logits, None)

    assert call(hh=None) == E_INVAL
    assert call(ids=None) == E_INVAL
    assert call(new_lens=None) == E_INVAL
    assert call(lens=None) == E_INVAL
    assert call(logits=None) == E_INVAL
    assert call(B=0) == E_INVAL
    assert call(B=-2) == E_INVAL
    assert call(T=0) == E_INVAL
    assert call(T=-1) == E_INVAL
    assert call() == E_STATE  # nothing bound
    assert b"params" in lib.slam_last_error(h) and b"workspace" in lib.slam_last_error(h)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert call() == E_STATE  # parameters but no workspace
    assert b"workspace" in lib.slam_last_error(h)
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert call() == E_STATE  # no cache
    assert b"cache" in lib.slam_last_error(h)
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 200, 64), 200, 64) == 0
    assert call(B=2, T=129) == E_NOMEM  # B T above the 256 workspace tokens
    assert call(B=129, T=1) == E_NOMEM  # 2 B tokens of decode scratch
    assert call(B=2, T=65) == E_STATE  # a chunk longer than the capacity can never fit
    assert b"capacity" in lib.slam_last_error(h)
    assert call() == E_STATE  # no prefill
    assert b"prefill" in lib.slam_last_error(h)
    eng.close()


def test_extend_refuses_opt():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*OPT), 1, 128)
    h = eng.h
    fake = C.c_void_p(1 << 20)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert lib.slam_extend(h, fake, fake, fake, 2, 16, fake, None) == E_INVAL
    msg = lib.slam_last_error(h)
    assert lib.slam_prefill(h, fake, fake, 2, 16, fake, None) == E_INVAL
    assert msg == lib.slam_last_error(h) and b"Qwen2" in msg  # the prefill's message
    eng.close()


def test_op_refusals_and_workspace_arithmetic():
    lib = E.load_library()
    fake = C.c_void_p(1 << 20)

    def call(qkv=fake, base=fake, new=fake, k=fake, v=fake, o=fake, B=3, T=16, nH=14, nKV=2, hd=64, cap=128, bound=128):
        return lib.slam_op_attn_extend(qkv, base, new, k, v, o, None, 0, B, T, nH, nKV, hd, cap, bound, None)

    for kw in (dict(qkv=None), dict(base=None), dict(new=None), dict(k=None), dict(v=None), dict(o=None), dict(B=0), dict(T=0),
               dict(hd=96), dict(nH=18), dict(nH=13), dict(bound=0), dict(bound=129)):
        assert call(**kw) == E_INVAL, kw
    # a launch that fills the chip from its query tiles takes one split and needs no partials; a single token splits its keys
    assert lib.slam_op_attn_extend_workspace(8, 512, 14, 2, 64, 2048) == 0
    n = lib.slam_op_attn_extend_workspace(3, 1, 14, 2, 64, 8192)
    assert n > 0 and n % (3 * 14 * (64 + 4) * 4) == 0
    assert lib.slam_op_attn_extend_workspace(0, 16, 14, 2, 64, 128) == 0


def test_chunked_prefill_binds_a_smaller_workspace():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    B, T, Cc, n = 8, 2048, 512, 8
    chunked = lib.slam_workspace_bytes(eng.h, max(B * min(T, Cc), 2 * B * n))
    oneshot = lib.slam_workspace_bytes(eng.h, max(B * T, 2 * B * n))
    assert 0 < chunked < oneshot
    eng.close()


@pytest.mark.parametrize("bad", [0, -3, 2.0, "4", True])
def test_generate_rejects_bad_prefill_chunk(bad):
    import torch
    from slamkit_amd.model.unit_lm import UnitLM
    m = UnitLM.__new__(UnitLM)  # host-only: the argument is checked before the model is touched
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.generate(input_ids=torch.zeros(1, 4, dtype=torch.long), max_new_tokens=2, prefill_chunk=bad)
