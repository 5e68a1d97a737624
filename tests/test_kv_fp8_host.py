"""Host side of the FP8 KV cache: the sizes slam_kv_cache_bytes_ex reports and the new names of the C ABI."""
import fnmatch
import os
import re

import pytest

from slamkit_amd import engine as E
from tests import kv8_ref as K8

NEW = ["slam_kv_cache_bytes_ex", "slam_bind_kv_cache_ex", "slam_op_kv_scatter_fp8", "slam_op_kv_extend_scatter_fp8",
       "slam_op_attn_decode_fp8", "slam_op_attn_extend_fp8"]


def test_new_symbols_in_header_and_export_map():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert set(NEW) <= set(E.header_symbols())
    hdr = open(os.path.join(root, "include", "slam_engine.h")).read()
    assert re.search(r"#define SLAM_KV_BF16 0\b", hdr) and re.search(r"#define SLAM_KV_FP8_E4M3 1\b", hdr)
    m = open(os.path.join(root, "slamkit_amd", "csrc", "exports.map")).read()
    pats = re.findall(r"([A-Za-z_*][\w*]*);", m[m.index("global:"):m.index("local:")])
    assert all(any(fnmatch.fnmatchcase(s, p) for p in pats) for s in NEW), pats


@pytest.mark.parametrize("hd,nKV,L", [(64, 2, 2), (128, 4, 3)])
def test_cache_sizes(hd, nKV, L):
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(L, 2 * nKV * hd, 2 * nKV, nKV, hd, 256, 512, 0, 1e-6, 10000.0))
    for bmax, cap in ((1, 64), (6, 320)):
        bf, f8 = eng.kv_cache_bytes(bmax, cap), eng.kv_cache_bytes(bmax, cap, "fp8_e4m3")
        vectors = L * 2 * bmax * nKV * cap
        assert bf == eng.kv_cache_bytes(bmax, cap, "bfloat16") == lib.slam_kv_cache_bytes(eng.h, bmax, cap) == vectors * 2 * hd
        assert f8 == vectors * (hd + 1) == K8.cache_bytes(L, bmax, nKV, cap, hd)
        assert lib.slam_kv_cache_bytes_ex(eng.h, bmax, cap, 2) == 0
    with pytest.raises(ValueError, match="bfloat16.*fp8_e4m3"):
        eng.kv_cache_bytes(1, 64, "int8")
