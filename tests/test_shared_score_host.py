"""Host-only: score_continuations(share_prompt_cache=...) - its two refusals, raised without an engine, and the engine calls of
both routes with their sizes, recorded from an engine stand-in on the CPU."""
import pytest
import torch

from slamkit_amd.model import generation
from tests.test_spec_host import _host_model


def test_share_prompt_cache_refusals():
    m = _host_model()
    kw = dict(input_ids=torch.ones(2, 4, dtype=torch.long), continuations=torch.ones(4, 3, dtype=torch.long), num_per_prompt=2)
    with pytest.raises(ValueError, match="share_prompt_cache.*fp8_e4m3"):
        m.score_continuations(share_prompt_cache=True, kv_cache_dtype="fp8_e4m3", **kw)
    m.kv_cache_dtype = "fp8_e4m3"  # the model attribute resolves the same way
    with pytest.raises(ValueError, match="share_prompt_cache.*fp8_e4m3"):
        m.score_continuations(share_prompt_cache=True, **kw)
    m.kv_cache_dtype = "bfloat16"
    with pytest.raises(ValueError, match="share_prompt_cache.*prefill_chunk"):
        m.score_continuations(share_prompt_cache=True, prefill_chunk=2, **kw)


class _Recorder:
    """Every engine method: records (name, the int / None / str arguments) and returns 64 (a byte count where one is asked)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name,) + tuple(x for x in a if x is None or isinstance(x, (int, str))))
            return 64
        return call


@pytest.mark.parametrize("share", [False, True])
def test_engine_calls_of_both_routes(monkeypatch, share):
    m = _host_model()
    m.engine, m._ensure_workspace = _Recorder(), lambda tokens: None
    m.share_prompt_cache = True  # generate's attribute: score_continuations reads its own argument only
    for name in ("token_logprobs", "token_logprobs_workspace_bytes"):
        monkeypatch.setattr(generation.E, name, lambda *a, **k: 64)
    B, n, T, Tc = 2, 3, 70, 9
    out = m.score_continuations(torch.ones(B, T, dtype=torch.long), continuations=torch.ones(B * n, Tc, dtype=torch.long),
                                num_per_prompt=n, score_chunk=5, **({"share_prompt_cache": True} if share else {}))
    assert out.shape == (B * n, Tc)
    blocks = [("extend_score", B * n, 5, None), ("extend_score", B * n, 4, None)]  # None: no argmax asked
    if share:
        want = [("kv_prefix_bytes", B, 128), ("bind_kv_prefix", B, 128), ("kv_cache_bytes", B * n, 64, "bfloat16"),
                ("bind_kv_cache", B * n, 64, "bfloat16"), ("prefill_prefix", B, T), ("kv_share", n)] + blocks + [("bind_kv_prefix", None)]
    else:  # the calls and sizes of the route as it was
        want = [("kv_cache_bytes", B * n, 128, "bfloat16"), ("bind_kv_cache", B * n, 128, "bfloat16"), ("prefill", B, T),
                ("kv_repeat", n)] + blocks
    assert m.engine.calls == want
