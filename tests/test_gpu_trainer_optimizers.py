"""-m gpu: SLAMTrainer._update against the engine calls it stands for, written out here as the trainer made them before it held an
optimizer object: grad_norm, then the kind's step calls (and refresh_transposed under Muon), on a second identically seeded
model fed the same gradients. Two steps; parameters, master, transposed images, norm_out and every state tensor bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
LR, WD, CLIP = 1e-3, 0.01, 0.5


def _model():
    from slamkit_amd.model import UnitLM, UnitLMConfig
    base = dict(num_hidden_layers=2, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                intermediate_size=512, rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    return UnitLM(UnitLMConfig(base_model_name="local", base_config=base, vocab_size=502, max_tokens=64), seed=3)


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


class _WrittenOut:
    """The state the trainer allocated and the calls it made, per kind, in their order."""

    def __init__(self, m, optim, osd):
        from slamkit_amd.trainer.slam_trainer import muon_adamw_runs
        self.m, self.optim, eng, dev, n = m, optim, m.engine, m.device, m.engine.n_params
        if osd == "bfloat16":
            m.drop_master()
        self.bf16 = osd == "bfloat16"
        mdt = BF16 if self.bf16 else torch.float32
        self.norm_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.state, self.t = {}, 0
        if optim == "adafactor":
            n_state, ws = eng.adafactor_set_segments([s.entry for s in m.hf_param_segments()])
            self.state["adafactor_state"] = torch.zeros(n_state, dtype=torch.float32, device=dev)
            self.ws = torch.empty(ws, dtype=torch.uint8, device=dev)
            eng.adafactor_bind_workspace(self.ws)
            return
        if optim == "muon":
            entries = [s.muon_entry for s in m.hf_muon_segments()]
            n_mom, ws = eng.muon_set_segments(entries)
            self.state["muon_momentum"] = torch.zeros(n_mom, dtype=torch.float32, device=dev)
            self.ws = torch.empty(ws + 256, dtype=torch.uint8, device=dev)
            pad = (-self.ws.data_ptr()) % 256
            eng.muon_bind_workspace(self.ws[pad:pad + ws])
            self.runs = muon_adamw_runs(entries, n)
            n = sum(c for _, c, _ in self.runs)
        self.state["exp_avg"] = torch.zeros(n, dtype=mdt, device=dev)
        self.state["exp_avg_sq"] = torch.zeros(n, dtype=mdt, device=dev)

    def update(self, zero_grad):
        eng, s = self.m.engine, self.state
        master = None if self.bf16 else self.m.flat_master
        eng.grad_norm(CLIP, self.norm_out)
        self.t += 1
        if self.optim == "adafactor":
            eng.adafactor_step(master, s["adafactor_state"], self.norm_out, LR, self.t, weight_decay=WD, zero_grad=zero_grad)
        elif self.optim == "muon":
            eng.muon_step(master, s["muon_momentum"], self.norm_out, LR, self.t, weight_decay=WD, momentum=0.95, nesterov=True,
                          ns_steps=5, adjust_lr="match_rms_adamw", zero_grad=zero_grad)
            for off, cnt, so in self.runs:
                eng.adamw_range(off, cnt, master, s["exp_avg"], s["exp_avg_sq"], self.norm_out, LR, 0.9, 0.999, 1e-8, WD, self.t,
                                zero_grad=zero_grad, state_offset=so)
            eng.refresh_transposed()
        elif self.bf16:
            eng.adamw_step_bf16(s["exp_avg"], s["exp_avg_sq"], self.norm_out, LR, 0.9, 0.999, 1e-8, WD, self.t, zero_grad=zero_grad)
        else:
            eng.adamw_step(master, s["exp_avg"], s["exp_avg_sq"], self.norm_out, LR, 0.9, 0.999, 1e-8, WD, self.t, zero_grad=zero_grad)


@pytest.mark.parametrize("osd", ["float32", "bfloat16"])
@pytest.mark.parametrize("optim", ["adamw_torch", "adafactor", "muon"])
def test_update_is_the_written_out_engine_calls(optim, osd):
    from slamkit_amd.trainer import SLAMTrainer, SLAMTrainingArguments
    mt, mr = _model(), _model()
    a = SLAMTrainingArguments(optim=optim, optim_state_dtype=osd, logging_steps=0, max_grad_norm=CLIP, weight_decay=WD,
                              output_dir="/tmp/unused")
    assert (a.adam_beta1, a.adam_beta2, a.adam_epsilon) == (0.9, 0.999, 1e-8)
    assert (a.muon_momentum, a.muon_nesterov, a.muon_ns_steps, a.muon_adjust_lr) == (0.95, True, 5, "match_rms_adamw")
    tr = SLAMTrainer(model=mt, args=a)
    ref = _WrittenOut(mr, optim, osd)
    n = mt.engine.n_params
    gen = torch.Generator().manual_seed(17)
    for t in range(2):
        g = (torch.randn(n, generator=gen) * 0.02).to(mt.device)
        for m in (mt, mr):
            m.engine.set_option("grad_norm_partials", 0)   # the norm reads the buffer: no backward wrote partial sums
            m.flat_grads.copy_(g)
        tr._update(LR, zero_grad=t == 0)
        ref.update(zero_grad=t == 0)
    torch.cuda.synchronize()
    assert tr.opt_step == 2 and 0 < float(tr.norm_out[1]) < 1
    assert torch.equal(bits(tr.norm_out), bits(ref.norm_out))
    assert torch.equal(bits(mt.flat_params), bits(mr.flat_params)) and torch.equal(bits(mt._weights), bits(mr._weights))
    assert torch.equal(bits(mt.flat_grads), bits(mr.flat_grads))
    if mt.flat_params_t is not None:
        assert torch.equal(bits(mt.flat_params_t), bits(mr.flat_params_t))
    got = {k: getattr(tr, k) for k in ("exp_avg", "exp_avg_sq", "adafactor_state", "muon_momentum") if getattr(tr, k, None) is not None}
    assert sorted(got) == sorted(ref.state)
    for k, v in ref.state.items():
        assert v.dtype == got[k].dtype and torch.equal(bits(got[k]), bits(v)), k
        assert float(v.float().abs().max()) > 0, k
