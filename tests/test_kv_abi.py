"""CPU tier of the KV-cached generation ABI: the new entry points are exported and bound, the cache size follows the stated
layout, and prefill / decode on an engine without the buffers they need are refused before anything reaches the device."""
import ctypes as C

from slamkit_amd import engine as E

NEW = ["slam_kv_cache_bytes", "slam_bind_kv_cache", "slam_prefill", "slam_decode_step", "slam_op_gemm_skinny",
       "slam_op_gemm_skinny_workspace", "slam_op_attn_decode", "slam_op_attn_decode_workspace"]
SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
CFG3 = (28, 1536, 12, 2, 128, 8960, 152576, 0, 1e-6, 1000000.0)


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n


def test_kv_cache_bytes_layout():
    for d in (SLAM, CFG3):
        eng = E.Engine(E.SlamModelDesc(*d))
        L, nKV, hd = d[0], d[3], d[4]
        for B, cap in ((1, 64), (8, 448), (3, 8192)):
            assert eng.kv_cache_bytes(B, cap) == L * 2 * B * nKV * cap * hd * 2
        eng.close()
    assert E.Engine(E.SlamModelDesc(*SLAM)).kv_cache_bytes(1, 1) == 12288
    assert E.Engine(E.SlamModelDesc(*CFG3)).kv_cache_bytes(1, 1) == 28672


def test_prefill_and_decode_refused_without_state():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch
    assert lib.slam_decode_step(None, fake, fake, 1, fake, None) == E_INVAL
    assert lib.slam_decode_step(h, None, fake, 1, fake, None) == E_INVAL
    assert lib.slam_decode_step(h, fake, fake, 1, fake, None) == E_STATE  # nothing bound
    assert lib.slam_prefill(h, fake, fake, 1, 8, fake, None) == E_STATE
    assert lib.slam_prefill(h, fake, fake, 0, 8, fake, None) == E_INVAL
    assert lib.slam_kv_cache_bytes(h, 0, 64) == 0
    assert lib.slam_bind_kv_cache(h, C.c_void_p(256 * 3 + 1), 1 << 30, 1, 64) == E_INVAL  # misaligned
    assert lib.slam_bind_kv_cache(h, fake, 100, 1, 64) == -3  # too small
    # params, workspace and cache bound (host-side bookkeeping only), no prefill yet
    assert lib.slam_bind_params(h, fake, None) == 0
    nws = lib.slam_workspace_bytes(h, 256)
    assert lib.slam_bind_workspace(h, fake, nws, 256) == 0
    assert lib.slam_decode_step(h, fake, fake, 1, fake, None) == E_STATE  # no cache
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 2, 64), 2, 64) == 0
    assert lib.slam_decode_step(h, fake, fake, 2, fake, None) == E_STATE  # no prefill
    assert b"prefill" in lib.slam_last_error(h)
    assert lib.slam_prefill(h, fake, fake, 3, 8, fake, None) == E_INVAL  # more rows than the cache holds
    assert lib.slam_prefill(h, fake, fake, 1, 65, fake, None) == E_INVAL  # longer than its capacity
    eng.close()


E_INVAL, E_STATE = -1, -2
