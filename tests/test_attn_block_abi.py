"""CPU tier of the attention-block op entries (slam_op_gemm_nt_rope, slam_op_attn_bwd_rope, slam_op_colsum): the names are
exported and bound, the column-sum workspace follows its stated layout, and null pointers / refused shapes return an error
code before anything reaches the device (the fake pointers below are never dereferenced)."""
import ctypes as C

from slamkit_amd import engine as E

NEW = ["slam_op_gemm_nt_rope", "slam_op_attn_bwd_rope", "slam_op_colsum_workspace", "slam_op_colsum"]
E_INVAL = -1
FAKE = C.c_void_p(1 << 20)


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n


def test_colsum_workspace_layout():
    """colsum_blocks(M) = min(128, ceil(M / 64)) partial rows of N floats."""
    lib = E.load_library()
    for M, N, rows in ((1, 256, 1), (64, 8, 1), (65, 8, 2), (4099, 896, 65), (8192, 1152, 128), (16384, 2048, 128)):
        assert lib.slam_op_colsum_workspace(M, N) == rows * N * 4
    assert lib.slam_op_colsum_workspace(0, 256) == 0
    assert lib.slam_op_colsum_workspace(64, 0) == 0


def test_colsum_refuses_before_launch():
    lib = E.load_library()
    f = FAKE
    assert lib.slam_op_colsum(None, 256, 8, 256, f, 0, f, None) == E_INVAL
    assert lib.slam_op_colsum(f, 256, 8, 256, None, 0, f, None) == E_INVAL
    assert lib.slam_op_colsum(f, 256, 8, 256, f, 0, None, None) == E_INVAL
    assert lib.slam_op_colsum(f, 256, 0, 256, f, 0, f, None) == E_INVAL
    assert lib.slam_op_colsum(f, 260, 8, 260, f, 0, f, None) == E_INVAL   # N % 8: the kernel reads 16-byte chunks
    assert lib.slam_op_colsum(f, 260, 8, 256, f, 0, f, None) == E_INVAL   # ld % 8
    assert lib.slam_op_colsum(f, 128, 8, 256, f, 0, f, None) == E_INVAL   # ld < N


def test_gemm_nt_rope_refuses_before_launch():
    lib = E.load_library()
    f = FAKE

    def call(X=f, W=f, Y=f, bias=f, pos=None, q=2, r=3, M=128, T=128, N=384, K=256, tab=f):
        return lib.slam_op_gemm_nt_rope(X, W, Y, bias, pos, 10000.0, q, r, M, T, N, K, tab, None)
    assert call(X=None) == E_INVAL and call(W=None) == E_INVAL and call(Y=None) == E_INVAL and call(tab=None) == E_INVAL
    assert call(K=224) == E_INVAL      # K % 64: the engine's unfused path
    assert call(N=448) == E_INVAL      # N % 128
    assert call(M=0) == E_INVAL
    assert call(T=0) == E_INVAL        # m % T without position_ids
    assert call(q=4, r=3) == E_INVAL   # more query heads than rotated heads
    assert call(q=2, r=7) == E_INVAL   # rotated heads beyond the N columns


def test_attn_bwd_rope_refuses_before_launch():
    lib = E.load_library()
    f = FAKE

    def call(ptrs=(f,) * 8, pos=None, T=64, M=64, nH=4, nKV=2, hd=64, tab=f):
        return lib.slam_op_attn_bwd_rope(*ptrs, pos, T, 10000.0, M, nH, nKV, hd, tab, None)
    for i in range(8):  # qkv, o, d_o, lse2, dqkv, ws, seg_start, seg_end
        assert call(ptrs=tuple(None if j == i else f for j in range(8))) == E_INVAL, i
    assert call(tab=None) == E_INVAL
    assert call(hd=96) == E_INVAL
    assert call(nH=5) == E_INVAL       # nH % nKV
    assert call(M=0) == E_INVAL
    assert call(T=0) == E_INVAL
