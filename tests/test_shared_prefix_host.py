"""Host side of the shared-prompt cache (slam_kv_share): the prompt store's size, every refusal that needs no device, through
the library in the style of tests/test_kv_abi.py, and generate's ValueErrors on a UnitLM that has no engine at all."""
import ctypes as C
import types

import pytest
import torch

from slamkit_amd import engine as E

SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
CFG3 = (28, 1536, 12, 2, 128, 8960, 152576, 0, 1e-6, 1000000.0)
E_INVAL, E_STATE, E_NOMEM = -1, -2, -3


def test_prefix_bytes():
    lib = E.load_library()
    for d in (SLAM, CFG3):
        eng = E.Engine(E.SlamModelDesc(*d))
        L, nKV, hd = d[0], d[3], d[4]
        for P, cap in ((1, 64), (8, 2048), (3, 1)):
            assert eng.kv_prefix_bytes(P, cap) == L * 2 * P * nKV * cap * hd * 2 + 4 * P
        assert eng.kv_prefix_bytes(0, 64) == 0 and eng.kv_prefix_bytes(1, 0) == 0
        eng.close()
    assert lib.slam_kv_prefix_bytes(None, 1, 64) == 0
    opt = E.Engine(E.SlamModelDesc(2, 256, 4, 4, 64, 512, 502, 0, 1e-5, 10000.0), arch=1, n_positions=64)
    assert opt.kv_prefix_bytes(1, 64) == 0
    assert lib.slam_bind_kv_prefix(opt.h, C.c_void_p(1 << 20), 1 << 30, 1, 64) == E_INVAL and b"OPT" in lib.slam_last_error(opt.h)
    opt.close()


def test_refusals_without_a_device():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch
    need = lib.slam_kv_prefix_bytes(h, 2, 64)
    for args in ((None, fake, need, 2, 64), (h, fake, need, 0, 64), (h, fake, need, 2, 0), (h, C.c_void_p(769), need, 2, 64)):
        assert lib.slam_bind_kv_prefix(*args) == E_INVAL, args  # NULL engine, bad sizes, misaligned
    assert lib.slam_bind_kv_prefix(h, fake, need - 1, 2, 64) == E_NOMEM
    assert lib.slam_prefill_prefix(None, fake, fake, 1, 8, fake, None) == lib.slam_prefill_prefix(h, fake, fake, 0, 8, fake, None) == E_INVAL
    assert lib.slam_prefill_prefix(h, fake, fake, 1, 8, fake, None) == E_STATE  # no params, no workspace
    for args in ((None, 2, fake), (h, 2, None), (h, 0, fake)):
        assert lib.slam_kv_share(*args, None, None) == E_INVAL, args
    assert lib.slam_kv_share(h, 2, fake, None, None) == E_STATE and b"KV cache" in lib.slam_last_error(h)
    assert lib.slam_bind_params(h, fake, None) == 0
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert lib.slam_prefill_prefix(h, fake, fake, 1, 8, fake, None) == E_STATE and b"prompt store" in lib.slam_last_error(h)
    # an FP8 ordinary cache is refused whatever the store's state; a bf16 one then asks for the store and its prefill
    assert lib.slam_bind_kv_cache_ex(h, fake, lib.slam_kv_cache_bytes_ex(h, 4, 64, 1), 4, 64, 1) == 0
    assert lib.slam_kv_share(h, 2, fake, None, None) == E_INVAL and b"bf16" in lib.slam_last_error(h)
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 4, 64), 4, 64) == 0
    assert lib.slam_kv_share(h, 2, fake, None, None) == E_STATE and b"prompt store" in lib.slam_last_error(h)
    assert lib.slam_bind_kv_prefix(h, fake, need, 2, 64) == 0
    assert lib.slam_kv_share(h, 2, fake, None, None) == E_STATE and b"slam_prefill_prefix" in lib.slam_last_error(h)
    assert lib.slam_prefill_prefix(h, fake, fake, 3, 8, fake, None) == E_INVAL  # more prompts than the store holds
    assert lib.slam_prefill_prefix(h, fake, fake, 1, 65, fake, None) == E_INVAL  # longer than its capacity
    assert lib.slam_bind_kv_prefix(h, None, 0, 0, 0) == 0  # unbound again
    assert lib.slam_prefill_prefix(h, fake, fake, 1, 8, fake, None) == E_STATE
    # the single-op door: a bound above its capacity, and a workspace without room for one split of each part
    args = lambda nws, pb: (fake, None, fake, fake, 3, fake, fake, 64, fake, fake, 64, fake, fake, nws, 3, 14, 2, 64, pb, 2, 1e4, None)  # noqa: E731
    full = lib.slam_op_attn_decode_shared_workspace(3, 3, 14, 2, 64, 33, 2)
    assert full == ((9 * 8 + 255) & ~255) + ((4 * 9 * 32 * 4 + 255) & ~255) + 9 * 14 * 2 * 66 * 4  # one split each at these bounds
    assert lib.slam_op_attn_decode_shared(*args(full, 65)) == E_INVAL and lib.slam_op_attn_decode_shared(*args(full - 4, 33)) == E_NOMEM
    eng.close()


def test_generate_refusals_need_no_engine():
    from slamkit_amd.model import UnitLM
    m = object.__new__(UnitLM)  # no engine, no parameters: every refusal below comes before the first engine call
    object.__setattr__(m, "config", types.SimpleNamespace(is_opt=False, eos_token_id=None, pad_token_id=None))
    ids = torch.ones(2, 4, dtype=torch.long)
    assert UnitLM.share_prompt_cache is False
    for kw in (dict(kv_cache_dtype="fp8_e4m3"), dict(prefill_chunk=2), dict(assistant_model=m), dict(prompt_lookup_num_tokens=2)):
        with pytest.raises(ValueError, match="share_prompt_cache"):
            UnitLM.generate(m, ids, max_new_tokens=2, share_prompt_cache=True, **kw)
    with pytest.raises(ValueError, match="share_prompt_cache"):  # generation_config switches it on too
        UnitLM.generate(m, ids, max_new_tokens=2, prefill_chunk=2, generation_config=types.SimpleNamespace(share_prompt_cache=True))
