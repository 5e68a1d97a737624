"""CPU tier of n samples per prompt (slam_kv_repeat) and of the token log-probabilities (slam_token_logprobs): the symbols
are declared, exported and bound; every documented refusal comes back before anything reaches the device (fake pointers, as in
test_kv_abi.py); the workspace size is host arithmetic; and the float32 restatement of the kernel's summation order
(tests/logprob_ref.py) agrees with the float64 reference on the GPU test's inputs.

Largest |float32 restatement - float64| over those inputs: 1.165e-06 (measured here; the GPU tolerance is 10 x this value,
computed from the restatement at run time, never from the kernel). A priori the restatement's sum has at most
8 + 6 + 3 + 75 roundings behind any term (93 x 2^-24 = 5.6e-6 relative, which is its absolute effect on log S) and the last
three operations round values below 64 (3 x 3.8e-6): the bound asserted below, 2e-5, follows from the float32 format alone."""
import ctypes as C

import numpy as np

from slamkit_amd import engine as E
from tests import logprob_ref as R

NEW = ["slam_kv_repeat", "slam_token_logprobs", "slam_token_logprobs_workspace_bytes"]
SLAM = (24, 896, 14, 2, 64, 4864, 502, 0, 1e-6, 10000.0)
E_INVAL, E_STATE = -1, -2


def test_new_symbols_exported_and_bound():
    lib = E.load_library()
    for n in NEW:
        assert n in E.header_symbols(), n
        assert hasattr(lib, n), n
        assert n in lib._slam_signatures, n
    assert hasattr(E.Engine, "kv_repeat") and hasattr(E, "token_logprobs") and hasattr(E, "token_logprobs_workspace_bytes")


def test_kv_repeat_refused_before_a_launch():
    lib = E.load_library()
    eng = E.Engine(E.SlamModelDesc(*SLAM))
    h = eng.h
    fake = C.c_void_p(1 << 20)  # never dereferenced: every call below must return before a launch
    assert lib.slam_kv_repeat(None, 2, fake, fake, None) == E_INVAL
    assert lib.slam_kv_repeat(h, 0, fake, fake, None) == E_INVAL
    assert lib.slam_kv_repeat(h, -3, fake, fake, None) == E_INVAL
    assert lib.slam_kv_repeat(h, 2, None, fake, None) == E_INVAL
    assert lib.slam_kv_repeat(h, 2, fake, None, None) == E_STATE  # no cache bound
    assert lib.slam_kv_repeat(h, 1, fake, None, None) == E_STATE  # n = 1 is a no-op only where the call is legal
    assert lib.slam_bind_params(h, fake, None) == 0
    assert lib.slam_bind_workspace(h, fake, lib.slam_workspace_bytes(h, 256), 256) == 0
    assert lib.slam_bind_kv_cache(h, fake, lib.slam_kv_cache_bytes(h, 4, 64), 4, 64) == 0
    assert lib.slam_kv_repeat(h, 2, fake, fake, None) == E_STATE  # no prefill
    assert b"prefill" in lib.slam_last_error(h)
    eng.close()


def test_token_logprobs_refused_before_a_launch():
    lib = E.load_library()
    fake = C.c_void_p(1 << 20)
    B, V = 3, 5000
    need = lib.slam_token_logprobs_workspace_bytes(B, V)

    def call(logits=fake, B=B, V=V, tokens=fake, out=fake, ws=fake, nb=need):
        return lib.slam_token_logprobs(logits, B, V, tokens, None, None, out, 1, 0, ws, nb, None)

    assert call(logits=None) == E_INVAL
    assert call(tokens=None) == E_INVAL
    assert call(out=None) == E_INVAL
    assert call(B=0) == E_INVAL
    assert call(B=-1) == E_INVAL
    assert call(V=0) == E_INVAL
    assert call(nb=need - 1) == E_INVAL
    assert call(nb=0) == E_INVAL
    assert call(ws=None) == E_INVAL


def test_token_logprobs_workspace_is_host_arithmetic():
    lib = E.load_library()
    for B, V in ((1, 1), (3, 502), (64, 2048), (64, 2049), (64, 152167)):
        n = lib.slam_token_logprobs_workspace_bytes(B, V)
        assert n > 0 and n == E.token_logprobs_workspace_bytes(B, V)
        assert n >= B * -(-V // 2048) * 8  # one (max, sum) pair per chunk of the sampler's size
    for B, V in ((0, 502), (-1, 502), (3, 0), (3, -7)):
        assert lib.slam_token_logprobs_workspace_bytes(B, V) == 0


def test_restatement_matches_fp64_reference():
    cases = R.op_cases()
    err = R.restatement_error(cases)
    print(f"[logprob] largest |float32 restatement - float64| over the GPU test's inputs: {err:.3e}")
    assert 0.0 < err <= 2e-5, err
    # the conventions, on values that can be checked by hand
    x = np.array([[0.0, 0.0, np.nan, -np.inf], [np.inf, 1.0, 2.0, 3.0]], np.float32)
    for f in (R.logprob_f32, R.logprob_f64):
        got = f(x, [1, 0])
        assert abs(float(got[0]) + np.log(2.0)) < 1e-6 and float(got[1]) == 0.0
        assert f(x, [2, 7]).tolist() == [-np.inf, 0.0]  # a NaN entry, an id outside the row
    # more than one chunk: the chunk-order combination agrees with the plain definition
    g = np.random.default_rng(1)
    y = (g.standard_normal((1, 5000)) * 4).astype(np.float32)
    assert abs(float(R.logprob_f32(y, [4999])[0]) - float(R.logprob_f64(y, [4999])[0])) <= 2e-5
