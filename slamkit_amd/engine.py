"""ctypes binding of libslam_engine.so (include/slam_engine.h).

PyTorch-ROCm is plumbing here: it owns device memory and streams; every compute call goes
through the C ABI with raw device pointers. There is NO CPU or eager fallback: if the HIP
library is missing the import of :func:`load_library` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libslam_engine.so")
_lib = None

BUCKET_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)
MODEL_UNTIED_HEAD = 1  # SLAM_MODEL_UNTIED_HEAD


class SlamModelDesc(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32), ("hidden", C.c_int32), ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("intermediate", C.c_int32), ("vocab", C.c_int32), ("pad_token_id", C.c_int32),
        ("rms_eps", C.c_float), ("rope_theta", C.c_float),
    ]


class SlamTensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("offset", C.c_int64), ("rows", C.c_int64), ("cols", C.c_int64)]


class SlamAdafactorSegment(C.Structure):
    """One HF parameter laid over the flat buffer (slam_adafactor_set_segments). pattern 0: contiguous rows; 1 / 2: groups of
    32 rows every 64 behind `offset`, phase 0 / 32 (gate_proj / up_proj inside wgu)."""
    _fields_ = [("offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("factored", C.c_int32), ("pattern", C.c_int32)]


class SlamMuonSegment(C.Structure):
    """One Muon matrix over the flat buffer (slam_muon_set_segments); offset / rows / cols / pattern as SlamAdafactorSegment's."""
    _fields_ = [("offset", C.c_int64), ("rows", C.c_int32), ("cols", C.c_int32), ("pattern", C.c_int32), ("reserved", C.c_int32)]


class SlamMuonClass(C.Structure):
    """One shape class of the Muon table and where the bound workspace holds its packed matrices and partials."""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("count", C.c_int32),
                ("parts", C.c_int32), ("x_byte_offset", C.c_int64), ("part_byte_offset", C.c_int64)]


MUON_ADJUST_LR = {None: 0, "original": 1, "match_rms_adamw": 2}  # slam_muon_step's adjust_lr
MUON_NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)               # torch.optim.Muon's defaults
MUON_EPS = 1e-7


class SlamSampleDesc(C.Structure):
    _fields_ = [
        ("do_sample", C.c_int32), ("top_k", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
        ("seed", C.c_uint64), ("step", C.c_uint32), ("pad_id", C.c_int32), ("n_eos", C.c_int32),
    ]


class SlamWarpDesc(C.Structure):
    """The second half of HF's warper chain for slam_sample_tokens_warped; the defaults are "all off"."""
    _fields_ = [("min_p", C.c_float), ("typical_p", C.c_float), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float)]

    def __init__(self, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        super().__init__(min_p, typical_p, epsilon_cutoff, eta_cutoff)

    @property
    def active(self) -> bool:
        return self.min_p > 0 or self.typical_p < 1 or self.epsilon_cutoff > 0 or self.eta_cutoff > 0


class SlamConstrainDesc(C.Structure):
    _fields_ = [
        ("step", C.c_int32), ("no_repeat_ngram", C.c_int32), ("n_per_prompt", C.c_int32), ("prompt_stride", C.c_int32),
        ("ban_eos", C.c_int32), ("n_eos", C.c_int32), ("n_begin", C.c_int32), ("n_seqs", C.c_int32), ("n_seq_tokens", C.c_int32),
    ]


CONSTRAIN_MAX_SEQS = 256     # SLAM_CONSTRAIN_MAX_SEQS: multi-token bad word sequences per call
CONSTRAIN_MAX_SEQ_LEN = 16   # SLAM_CONSTRAIN_MAX_SEQ_LEN: tokens per sequence
CONSTRAIN_MAX_BEGIN = 256    # SLAM_CONSTRAIN_MAX_BEGIN: begin_suppress ids


def header_symbols() -> List[str]:
    """Every function name declared in include/slam_engine.h (used by the export test)."""
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slam_engine.h")
    txt = open(hdr).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", txt)) - {"slam_bucket_cb"})


def load_library(path: Optional[str] = None):
    """Load the HIP engine; raises OSError (loudly) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SLAM_ENGINE_LIB", _LIB_PATH)
    # PyTorch-ROCm first: its wheel carries its own libamdhip64; the engine library must bind to THAT runtime instance (the one
    # that owns the device memory and streams it is handed), not to a second copy loaded from /opt/rocm before torch came up
    # (kernel launches then fail with hipErrorNoDevice)
    import torch  # noqa: F401
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `python -m slamkit_amd.csrc.build` "
                      f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(p)
    vp, i32, i64, f32, f64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
    sig = {
        "slam_engine_create": (C.c_int, [C.POINTER(SlamModelDesc), C.POINTER(vp)]),
        "slam_engine_create_arch": (C.c_int, [C.POINTER(SlamModelDesc), i32, i32, C.POINTER(vp)]),
        "slam_engine_create_ex": (C.c_int, [C.POINTER(SlamModelDesc), i32, i32, i32, C.POINTER(vp)]),
        "slam_engine_destroy": (None, [vp]),
        "slam_last_error": (C.c_char_p, [vp]),
        "slam_version": (C.c_char_p, []),
        "slam_param_count": (i64, [vp]),
        "slam_tensor_count": (i32, [vp]),
        "slam_tensor_info": (C.c_int, [vp, i32, C.POINTER(SlamTensorInfo)]),
        "slam_bind_params": (C.c_int, [vp, vp, vp]),
        "slam_bind_params_t": (C.c_int, [vp, vp]),
        "slam_refresh_transposed": (C.c_int, [vp, vp]),
        "slam_workspace_bytes": (sz, [vp, i64]),
        "slam_bind_workspace": (C.c_int, [vp, vp, sz, i64]),
        "slam_forward": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, f64, vp, vp, vp]),
        "slam_unpadded_scratch_bytes": (sz, [i32, i32]),
        "slam_forward_unpadded": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp, sz, f64, vp, vp, vp]),
        "slam_forward_unpadded_spans": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, f64, vp, vp, vp]),
        "slam_last_forward_tokens": (i64, [vp]),
        "slam_seq_loglik_unpadded": (C.c_int, [vp, i32, vp, vp, vp]),
        "slam_scale_loss_unpadded": (C.c_int, [vp, vp, i32, vp]),
        "slam_op_unpad_pack": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "slam_op_unpad_pack_spans": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, sz, vp]),
        "slam_backward": (C.c_int, [vp, f32, i32, BUCKET_CB, vp, vp]),
        "slam_kv_cache_bytes": (sz, [vp, i32, i32]),
        "slam_bind_kv_cache": (C.c_int, [vp, vp, sz, i32, i32]),
        "slam_prefill": (C.c_int, [vp, vp, vp, i32, i32, vp, vp]),
        "slam_decode_step": (C.c_int, [vp, vp, vp, i32, vp, vp]),
        "slam_sample_workspace_bytes": (sz, [i32, i32, i32]),
        "slam_sample_tokens": (C.c_int, [vp, i32, i32, vp, C.POINTER(SlamSampleDesc), vp, vp, vp, vp, vp, i64, vp, sz, vp]),
        "slam_constrain_scores": (C.c_int, [vp, vp, i32, i32, C.POINTER(SlamConstrainDesc), vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        "slam_kv_repeat": (C.c_int, [vp, i32, vp, vp, vp]),
        "slam_extend": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, vp]),
        "slam_extend_score": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
        "slam_extend_logits": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, vp]),
        "slam_kv_rewind": (C.c_int, [vp, i32]),
        "slam_sample_tokens_at": (C.c_int, [vp, i32, i32, vp, C.POINTER(SlamSampleDesc), vp, vp, vp, vp, vp, i64, vp, sz, vp, i32,
                                            i32, vp]),
        "slam_sample_tokens_warped": (C.c_int, [vp, i32, i32, vp, C.POINTER(SlamSampleDesc), vp, vp, vp, vp, vp, i64, vp, sz, vp,
                                                i32, i32, C.POINTER(SlamWarpDesc), vp]),
        "slam_spec_accept": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "slam_ngram_propose": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, i64, vp, vp, i64, vp, vp, vp, i32, vp, vp]),
        "slam_token_logprobs_workspace_bytes": (sz, [i32, i32]),
        "slam_token_logprobs": (C.c_int, [vp, i32, i32, vp, vp, vp, vp, i64, i32, vp, sz, vp]),
        "slam_cfg_workspace_bytes": (sz, [i32, i32]),
        "slam_cfg_scores": (C.c_int, [vp, i32, i32, f32, vp, vp, sz, vp]),
        "slam_cfg_mirror_tokens": (C.c_int, [vp, i32, vp]),
        "slam_bucket_stream": (vp, [vp]),
        "slam_set_logit_mask": (C.c_int, [vp, vp]),
        "slam_padded_vocab": (i32, [vp]),
        "slam_seq_loglik": (C.c_int, [vp, vp, i32, i32, vp, vp, vp]),
        "slam_scale_loss_rows": (C.c_int, [vp, vp, i32, i32, vp]),
        "slam_set_label_smoothing": (C.c_int, [vp, f32]),
        "slam_set_neftune": (C.c_int, [vp, f32, i64]),
        "slam_grad_norm": (C.c_int, [vp, f32, vp, vp]),
        "slam_adamw_step": (C.c_int, [vp, vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_adamw_step_bf16": (C.c_int, [vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_adamw_step_bf16_moments": (C.c_int, [vp, vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_adamw_range_bf16_moments": (C.c_int, [vp, i64, i64, vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_grad_chunk_elems": (i64, []),
        "slam_grad_sumsq_chunks": (C.c_int, [vp, i64, i64, vp, vp]),
        "slam_grad_norm_from_chunks": (C.c_int, [vp, vp, f32, vp, vp]),
        "slam_adamw_range": (C.c_int, [vp, i64, i64, vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_adamw_range_bf16": (C.c_int, [vp, i64, i64, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_set_decay_mask": (C.c_int, [vp, vp, i32]),
        "slam_adafactor_set_segments": (C.c_int, [vp, C.POINTER(SlamAdafactorSegment), i32]),
        "slam_adafactor_sizes": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
        "slam_adafactor_bind_workspace": (C.c_int, [vp, vp, sz]),
        "slam_adafactor_step": (C.c_int, [vp, vp, vp, vp, f64, f64, f64, f64, f64, i32, i32, vp]),
        "slam_muon_set_segments": (C.c_int, [vp, C.POINTER(SlamMuonSegment), i32]),
        "slam_muon_sizes": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]),
        "slam_muon_bind_workspace": (C.c_int, [vp, vp, sz]),
        "slam_muon_class_count": (i32, [vp]),
        "slam_muon_class_info": (C.c_int, [vp, i32, C.POINTER(SlamMuonClass)]),
        "slam_muon_step": (C.c_int, [vp, vp, vp, vp, f64, f64, f64, i32, i32, f64, f64, f64, f64, i32, i32, i32, vp]),
        "slam_op_muon_prepare": (C.c_int, [vp, vp, vp, f64, i32, i32, vp]),
        "slam_op_muon_ns_workspace": (sz, [i32, i32, i32]),
        "slam_op_muon_ns": (C.c_int, [vp, i32, i32, i32, i64, vp, i32, i32, f64, f64, f64, f64, vp, sz, vp]),
        "slam_op_muon_apply": (C.c_int, [vp, vp, vp, f64, f64, i32, i32, vp]),
        "slam_op_muon_syrk": (C.c_int, [vp, vp, vp, i32, i32, i32, i64, i64, i64, f32, f32, vp]),
        "slam_op_muon_mm": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i64, i64, i64, i64, f32, f32, vp]),
        "slam_add_param_wait": (C.c_int, [vp, i64, i64, vp]),
        "slam_param_wait_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "slam_param_wait_untimed": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "slam_comm_unique_id": (C.c_int, [vp, C.c_int32]),
        "slam_comm_init": (C.c_int, [vp, vp, C.c_int32, C.c_int32]),
        "slam_comm_destroy": (C.c_int, [vp]),
        "slam_allreduce_grads_async": (C.c_int, [vp, i64, i64, C.c_int32, vp]),
        "slam_comm_finish": (C.c_int, [vp, vp]),
        "slam_reduce_scatter_grads_async": (C.c_int, [vp, i64, i64, C.c_int32, vp]),
        "slam_allgather_params_async": (C.c_int, [vp, i64, i64, vp]),
        "slam_gateup_launch_ms": (C.c_int, [vp, C.POINTER(C.c_float), C.c_int32]),
        "slam_family_ms": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]),
        "slam_family_name": (C.c_char_p, [C.c_int32]),
        "slam_pack_grads_bf16": (C.c_int, [vp, i64, i64, vp, vp]),
        "slam_unpack_grads_bf16": (C.c_int, [vp, i64, i64, vp, vp]),
        "slam_set_grad_image": (C.c_int, [vp, vp]),
        "slam_join": (C.c_int, [vp, vp]),
        "slam_zero_grads": (C.c_int, [vp, vp]),
        "slam_cast_params": (C.c_int, [vp, vp, vp]),
        "slam_set_option": (C.c_int, [vp, C.c_char_p, i64]),
        "slam_op_gemm_nt": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_nt_swiglu": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_nt_dswiglu": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_nn": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_tn_workspace": (sz, [C.c_int, C.c_int, C.c_int]),
        "slam_op_gemm_tn": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "slam_op_gemm_tn_image": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
        "slam_op_gemm_skinny_workspace": (sz, [C.c_int, C.c_int, C.c_int]),
        "slam_op_gemm_skinny": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp]),
        "slam_op_w8_bytes": (sz, [C.c_int, C.c_int]),
        "slam_op_w8_exps_offset": (sz, [C.c_int, C.c_int]),
        "slam_op_quantize_rows_fp8": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_dequantize_rows_fp8": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_gemm_skinny_w8": (C.c_int, [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp]),
        "slam_decode_w8_bytes": (sz, [vp, i32]),
        "slam_bind_decode_w8": (C.c_int, [vp, vp, sz, i32]),
        "slam_quantize_decode_w8": (C.c_int, [vp, vp]),
        "slam_decode_w8_state": (C.c_int, [vp]),
        "slam_decode_w8_launches": (i64, [vp]),
        "slam_op_score_rows_workspace": (sz, [C.c_int, C.c_int]),
        "slam_op_score_rows": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, sz, vp]),
        "slam_op_attn_decode_workspace": (sz, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "slam_op_attn_decode": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          f32, vp]),
        "slam_op_attn_extend_workspace": (sz, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "slam_op_attn_extend": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, sz, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, vp]),
        "slam_op_rmsnorm_fwd": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
        "slam_op_rmsnorm_bwd_workspace": (sz, [C.c_int, C.c_int]),
        "slam_op_rmsnorm_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_layernorm_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, f32, vp]),
        "slam_op_layernorm_bwd_workspace": (sz, [C.c_int, C.c_int]),
        "slam_op_layernorm_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_embed_pos_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_nt_relu": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_gemm_nt_drelu": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_relu_bwd": (C.c_int, [vp, vp, i64, vp]),
        "slam_op_rope": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, f32, C.c_int, vp, vp]),
        "slam_op_qknorm_rope_fwd": (C.c_int, [vp, vp, vp, vp, f32, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
        "slam_op_qknorm_bwd_workspace": (sz, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "slam_op_qknorm_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_qknorm_rows_f32": (C.c_int, [vp, vp, vp, f32, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_swiglu_fwd": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_swiglu_bwd": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_attn_fwd": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_attn_bwd_workspace": (sz, [C.c_int, C.c_int, C.c_int]),
        "slam_op_attn_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_attn_bwd_rope": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, f32, C.c_int, C.c_int, C.c_int, C.c_int,
                                            vp, vp]),
        "slam_op_gemm_nt_rope": (C.c_int, [vp, vp, vp, vp, vp, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "slam_op_colsum_workspace": (sz, [C.c_int, C.c_int]),
        "slam_op_colsum": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
        "slam_op_cross_entropy": (C.c_int, [vp, vp, f64, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_cross_entropy_smooth": (C.c_int, [vp, vp, f64, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp]),
        "slam_op_copy_cols": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_unpad_logits": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_unpad_logits_spans": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_scale_bf16": (C.c_int, [vp, i64, f32, vp]),
        "slam_op_scale_rows_bf16": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_scale_rows_unpadded_bf16": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp]),
        "slam_op_embed_bwd_workspace": (sz, [C.c_int, C.c_int]),
        "slam_op_embed_bwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "slam_op_sr_round_bf16": (C.c_int, [vp, vp, i64, i64, i64, i32, i32, vp]),
        "slam_op_dropout_add": (C.c_int, [vp, vp, C.c_int, C.c_int, i32, i64, i64, i32, i64, vp]),
        "slam_op_dropout_bwd": (C.c_int, [vp, vp, C.c_int, C.c_int, i32, i64, i64, i32, i64, vp]),
        "slam_op_embed_fwd": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
        "slam_op_embed_noise_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32, i64, i64, i64,
                                              vp]),
    }
    for name, (res, args) in sig.items():
        if path is not None and not hasattr(lib, name):
            continue  # an explicitly named OTHER build (A/B tooling against an older library): bind what it has
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    lib._slam_signatures = sig
    if path is None:
        _lib = lib
    return lib


def _ptr(t) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


class _Shifted:
    """t[a:b] of this = t[a + shift : b + shift] of the tensor (Engine.adamw_range with compact moments)."""

    def __init__(self, t, shift):
        self.t, self.shift, self.dtype = t, shift, t.dtype

    def __getitem__(self, sl):
        return self.t[sl.start + self.shift: sl.stop + self.shift]


def current_stream_ptr() -> int:
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


class EngineError(RuntimeError):
    pass


def muon_ns_workspace_bytes(batch: int, n: int, m: int) -> int:
    """Bytes of the scratch slam_op_muon_ns needs for `batch` packed [n][m] matrices (0: a shape it refuses)."""
    return int(load_library().slam_op_muon_ns_workspace(int(batch), int(n), int(m)))


def muon_ns(x, batch: int, n: int, m: int, stride: int, ws, ns_steps=5, ns_coefficients=MUON_NS_COEFFICIENTS, eps=MUON_EPS,
            partials=None, parts: int = 0, stream: Optional[int] = None):
    """slam_op_muon_ns: Newton-Schulz on `batch` packed bf16 [n][m] matrices (n <= m) at `stride` elements, in place. ws: a
    256-byte aligned device tensor of muon_ns_workspace_bytes; partials: the fp32 sum-of-squares partials (`parts` a matrix) of
    slam_op_muon_prepare, or None to have them taken here."""
    a, b, c = ns_coefficients
    rc = load_library().slam_op_muon_ns(_ptr(x), int(batch), int(n), int(m), int(stride), _ptr(partials), int(parts), int(ns_steps),
                                        float(a), float(b), float(c), float(eps), _ptr(ws), ws.numel() * ws.element_size(),
                                        stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_muon_ns failed ({rc})")


def muon_syrk(x, r, c, batch: int, n: int, m: int, stride_x: int, stride_r: int, stride_c: int, alpha: float, beta: float,
              stream: Optional[int] = None):
    """slam_op_muon_syrk: C[i] = beta R[i] + alpha X[i] X[i]^T (bf16 [n][n] from [n][m]); r = None: no R."""
    rc = load_library().slam_op_muon_syrk(_ptr(x), _ptr(r), _ptr(c), int(batch), int(n), int(m), int(stride_x), int(stride_r),
                                          int(stride_c), float(alpha), float(beta),
                                          stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_muon_syrk failed ({rc})")


def muon_mm(p, x, r, y, batch: int, n: int, m: int, stride_p: int, stride_x: int, stride_r: int, stride_y: int, alpha: float,
            beta: float, stream: Optional[int] = None):
    """slam_op_muon_mm: Y[i] = beta R[i] + alpha P[i] X[i] (P [n][n], X / R / Y [n][m], bf16); r = None: no R."""
    rc = load_library().slam_op_muon_mm(_ptr(p), _ptr(x), _ptr(r), _ptr(y), int(batch), int(n), int(m), int(stride_p), int(stride_x),
                                        int(stride_r), int(stride_y), float(alpha), float(beta),
                                        stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_muon_mm failed ({rc})")


def sample_workspace_bytes(B: int, vocab: int, top_k: int) -> int:
    """Bytes of device workspace slam_sample_tokens needs (host arithmetic; top_k = 1 for greedy)."""
    return int(load_library().slam_sample_workspace_bytes(int(B), int(vocab), int(top_k)))


def sample_tokens(logits, desc: SlamSampleDesc, next_ids, ws, banned=None, row_ids=None, eos_ids=None, done=None, out=None,
                  stream: Optional[int] = None):
    """slam_sample_tokens: next_ids[b] (int64 [B]) = the token chosen from row b of the fp32 logits [B, vocab] under `desc`
    (greedy or temperature / top-k / top-p with the stateless Philox draw of (seed, row id, step)). banned uint8 [vocab], row_ids
    int64 [B], eos_ids int32 [n_eos], done uint8 [B] (read and set), out int64 [B, stride] (column desc.step is written), ws a
    uint8 tensor of sample_workspace_bytes(...): device tensors, None where optional. Only enqueues work."""
    B, V = logits.shape
    rc = load_library().slam_sample_tokens(_ptr(logits), B, V, _ptr(banned), C.byref(desc), _ptr(row_ids), _ptr(eos_ids),
                                          _ptr(done), _ptr(next_ids), _ptr(out), out.stride(0) if out is not None else 0,
                                          _ptr(ws), ws.numel() * ws.element_size(),
                                          stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_sample_tokens failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def sample_tokens_at(logits, desc: SlamSampleDesc, next_ids, ws, steps=None, group: int = 1, out_col: int = 0, banned=None,
                     row_ids=None, eos_ids=None, done=None, out=None, stream: Optional[int] = None):
    """slam_sample_tokens_at: sample_tokens for rows at different steps. Row b of the fp32 logits [B, vocab] is column
    b % group of sequence b // group: it draws with row id row_ids[b // group] (default b // group) at step
    desc.step + steps[b // group] + b % group, and out[b, out_col] receives the token. steps: int32 / uint32 [B // group]
    (non-negative), None = zeros. next_ids / done are indexed by b. Only enqueues work."""
    B, V = logits.shape
    rc = load_library().slam_sample_tokens_at(_ptr(logits), B, V, _ptr(banned), C.byref(desc), _ptr(row_ids), _ptr(eos_ids),
                                             _ptr(done), _ptr(next_ids), _ptr(out), out.stride(0) if out is not None else 0,
                                             _ptr(ws), ws.numel() * ws.element_size(), _ptr(steps), int(group), int(out_col),
                                             stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_sample_tokens_at failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def sample_tokens_warped(logits, desc: SlamSampleDesc, next_ids, ws, warp: Optional[SlamWarpDesc], steps=None, group: int = 1,
                         out_col: Optional[int] = None, banned=None, row_ids=None, eos_ids=None, done=None, out=None,
                         stream: Optional[int] = None):
    """slam_sample_tokens_warped: sample_tokens_at with min_p / typical_p / epsilon_cutoff / eta_cutoff (`warp`, a
    SlamWarpDesc; None or all off = sample_tokens_at itself) applied to the ranked top-k candidates behind top-p.
    out_col=None writes column desc.step, which with steps=None and group=1 makes this sample_tokens' call. Only enqueues work."""
    B, V = logits.shape
    rc = load_library().slam_sample_tokens_warped(_ptr(logits), B, V, _ptr(banned), C.byref(desc), _ptr(row_ids), _ptr(eos_ids),
                                                 _ptr(done), _ptr(next_ids), _ptr(out), out.stride(0) if out is not None else 0,
                                                 _ptr(ws), ws.numel() * ws.element_size(), _ptr(steps), int(group),
                                                 int(desc.step if out_col is None else out_col),
                                                 C.byref(warp) if warp is not None else None,
                                                 stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_sample_tokens_warped failed ({rc})" + (": invalid argument" if rc == -1 else ""))


SPEC_MAX_ROWS = 1024  # slam_spec_accept: one block, a thread per row
SPEC_MAX_K = 15       # proposals per round
SPEC_STATS = ("live", "max_lens_t", "max_lens_d", "emitted", "accepted")


def spec_accept(chunk, tgt, K: int, max_new: int, pad_id: int, eos_ids, prompt_len, n_new, done, out, lens_t, lens_d, draft_ids,
                draft_new_lens, tgt_new_lens, stats, stream: Optional[int] = None):
    """slam_spec_accept: the acceptance rule of one round of assisted generation for all B rows in one launch (the contract is
    in include/slam_engine.h). chunk / tgt int64 [B, K + 1]; prompt_len / n_new / lens_t / lens_d / draft_new_lens /
    tgt_new_lens int32 [B]; done uint8 [B]; out int64 [B, >= max_new]; draft_ids int64 [B, 2]; stats int32 [5] (SPEC_STATS);
    eos_ids int32 or None. Only enqueues work."""
    B = chunk.shape[0]
    rc = load_library().slam_spec_accept(_ptr(chunk), _ptr(tgt), B, int(K), int(max_new), int(pad_id), _ptr(eos_ids),
                                        0 if eos_ids is None else int(eos_ids.numel()), _ptr(prompt_len), _ptr(n_new), _ptr(done),
                                        _ptr(out), out.stride(0), _ptr(lens_t), _ptr(lens_d), _ptr(draft_ids),
                                        _ptr(draft_new_lens), _ptr(tgt_new_lens), _ptr(stats),
                                        stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_spec_accept failed ({rc})" + (": invalid argument" if rc == -1 else ""))


NGRAM_MAX = 16  # slam_ngram_propose: the longest n-gram matched (SLAM_NGRAM_MAX)
NGRAM_STATS = ("rows", "proposed")


def ngram_propose(chunk, n_prop, max_ngram: int, fill_id: int, prompt, prompt_len, new, n_new, done, eos_ids=None, stats=None,
                  stream: Optional[int] = None):
    """slam_ngram_propose: prompt-lookup proposals for all B rows (the contract is in include/slam_engine.h). chunk int64
    [B, K + 1] (columns 1 .. K are written, column 0 never); n_prop / prompt_len / n_new int32 [B]; prompt int64 [B, stride]
    right-padded; new int64 [B, stride] (the out buffer of spec_accept); done uint8 [B]; eos_ids int32 or None; stats int32 [2]
    (NGRAM_STATS) or None. Only enqueues work."""
    B, K1 = chunk.shape
    rc = load_library().slam_ngram_propose(_ptr(chunk), _ptr(n_prop), B, K1 - 1, int(max_ngram), int(fill_id), _ptr(prompt),
                                          prompt.stride(0), _ptr(prompt_len), _ptr(new), new.stride(0), _ptr(n_new), _ptr(done),
                                          _ptr(eos_ids), 0 if eos_ids is None else int(eos_ids.numel()), _ptr(stats),
                                          stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_ngram_propose failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def constrain_scores(logits, scores, desc: SlamConstrainDesc, prompt, prompt_len, new=None, done=None, eos_ids=None,
                     begin_ids=None, seq_tokens=None, seq_offsets=None, stream: Optional[int] = None):
    """slam_constrain_scores: scores[b] (fp32 [B, vocab]; may be `logits` itself) = row b of the fp32 logits with -inf at every
    token that row's history bans under `desc` (no-repeat n-gram, bad word sequences, ban_eos, begin_suppress). prompt int64
    [B / n_per_prompt, stride] right-padded, prompt_len int32 (a copy taken before decoding), new int64 [B, stride] (the
    sampler's out buffer; columns < desc.step are read), done uint8 [B], eos_ids / begin_ids / seq_tokens / seq_offsets int32:
    device tensors, None where unused. desc.prompt_stride is set from `prompt`. Only enqueues work."""
    B, V = logits.shape
    desc.prompt_stride = int(prompt.stride(0))
    rc = load_library().slam_constrain_scores(_ptr(logits), _ptr(scores), B, V, C.byref(desc), _ptr(prompt), _ptr(prompt_len),
                                             _ptr(new), new.stride(0) if new is not None else 0, _ptr(done), _ptr(eos_ids),
                                             _ptr(begin_ids), _ptr(seq_tokens), _ptr(seq_offsets),
                                             stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_constrain_scores failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def token_logprobs_workspace_bytes(B: int, vocab: int) -> int:
    """Bytes of device workspace slam_token_logprobs needs (host arithmetic)."""
    return int(load_library().slam_token_logprobs_workspace_bytes(int(B), int(vocab)))


def token_logprobs(logits, tokens, out, column: int, ws, done=None, finished=None, stream: Optional[int] = None):
    """slam_token_logprobs: out[b, column] (fp32 [B, stride]) = the log-softmax of row b of the raw fp32 logits [B, vocab] at
    tokens[b] (int64 [B]); 0.0 for rows with finished[b] set, after which finished[b] = done[b] (both uint8 [B], None where
    unused). ws: a uint8 tensor of token_logprobs_workspace_bytes(B, vocab). Only enqueues work."""
    B, V = logits.shape
    rc = load_library().slam_token_logprobs(_ptr(logits), B, V, _ptr(tokens), _ptr(done), _ptr(finished), _ptr(out),
                                           out.stride(0), int(column), _ptr(ws), ws.numel() * ws.element_size(),
                                           stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_token_logprobs failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def cfg_workspace_bytes(B: int, vocab: int) -> int:
    """Bytes of device workspace slam_cfg_scores needs for B guided sequences (host arithmetic; 0 for invalid arguments)."""
    return int(load_library().slam_cfg_workspace_bytes(int(B), int(vocab)))


def cfg_scores(logits, guidance_scale: float, scores, ws, stream: Optional[int] = None):
    """slam_cfg_scores: scores[b] (fp32 [B, vocab], no overlap with logits) = g (a - u) + u, a the log-softmax of row b of the
    fp32 logits [2 B, vocab] (conditional) and u that of row B + b (unconditional). ws: a uint8 tensor of
    cfg_workspace_bytes(B, vocab). Only enqueues work."""
    B2, V = logits.shape
    if B2 % 2 or tuple(scores.shape) != (B2 // 2, V) or not (logits.is_contiguous() and scores.is_contiguous()):
        raise ValueError(f"cfg_scores: contiguous logits [2 B, V] and scores [B, V] (got {list(logits.shape)}, {list(scores.shape)})")
    rc = load_library().slam_cfg_scores(_ptr(logits), B2 // 2, V, float(guidance_scale), _ptr(scores), _ptr(ws),
                                       ws.numel() * ws.element_size(), stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_cfg_scores failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def cfg_mirror_tokens(next_ids, stream: Optional[int] = None):
    """slam_cfg_mirror_tokens: next_ids[B + b] = next_ids[b] on an int64 [2 B] device tensor. Only enqueues work."""
    n = int(next_ids.numel())
    if n % 2 or not next_ids.is_contiguous():
        raise ValueError(f"cfg_mirror_tokens: a contiguous int64 tensor of 2 B entries (got {n})")
    rc = load_library().slam_cfg_mirror_tokens(_ptr(next_ids), n // 2, stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_cfg_mirror_tokens failed ({rc})" + (": invalid argument" if rc == -1 else ""))


SCORE_CHUNK = 512  # SLAM_SCORE_CHUNK: vocabulary columns per chunk of slam_op_score_rows


def score_rows_workspace_bytes(M: int, vocab: int) -> int:
    """Bytes of device workspace slam_op_score_rows needs (host arithmetic; 0 for invalid sizes)."""
    return int(load_library().slam_op_score_rows_workspace(int(M), int(vocab)))


def score_rows(X, W, targets, lp, argmax=None, colmask=None, ws=None, stream: Optional[int] = None):
    """slam_op_score_rows: the LM head fused with the row statistics. X bf16 [M, K], W bf16 [V, K], targets int64 [M] (-100: no
    target): lp[m] (fp32 [M]) = the log-softmax of row m's fp32 scores at targets[m], argmax[m] (int64 [M], optional) = the
    lowest id of the largest score. colmask uint8 [>= V]: non-zero = the column counts as -inf. ws: a uint8 tensor of
    score_rows_workspace_bytes(M, V) (allocated here when None). Only enqueues work; returns ws."""
    import torch
    M, K = X.shape
    V = W.shape[0]
    if ws is None:
        ws = torch.empty(max(score_rows_workspace_bytes(M, V), 16), dtype=torch.uint8, device=X.device)
    rc = load_library().slam_op_score_rows(_ptr(X), _ptr(W), _ptr(targets), _ptr(colmask), _ptr(lp), _ptr(argmax), M, V, K,
                                          _ptr(ws), ws.numel() * ws.element_size(),
                                          stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_score_rows failed ({rc})" + (": invalid argument" if rc == -1 else ""))
    return ws


def unpadded_scratch_bytes(B: int, T: int) -> int:
    """Bytes of device scratch slam_forward_unpadded / slam_op_unpad_pack need for a [B, T] batch (host arithmetic)."""
    return int(load_library().slam_unpadded_scratch_bytes(int(B), int(T)))


def unpadded_scratch_views(scratch, B: int, T: int) -> Dict[str, "object"]:
    """The arrays of the packed batch inside `scratch` (a uint8 device tensor, 256-byte aligned), as include/slam_engine.h lays
    them out: ids, labels, position_ids int64 [Mmax]; seg_start, seg_end, row int32 [Mmax]; off int32 [B + 1]."""
    import torch
    mm = -(-(B * T) // 64) * 64
    out, o = {}, 0
    for name, dt, n in (("ids", torch.int64, mm), ("labels", torch.int64, mm), ("position_ids", torch.int64, mm),
                        ("seg_start", torch.int32, mm), ("seg_end", torch.int32, mm), ("row", torch.int32, mm),
                        ("off", torch.int32, B + 1)):
        nb = n * (8 if dt == torch.int64 else 4)
        out[name] = scratch[o:o + nb].view(dt)
        o += nb
    return out


def unpad_pack(ids, labels, lens, B: int, T: int, M_packed: int, pad_id: int, scratch, stream: Optional[int] = None):
    """slam_op_unpad_pack: the pack kernel of the padding-free forward on its own (ids / labels int64 [B, T], lens int32 [B],
    all device tensors; labels may be None). Read the result with unpadded_scratch_views."""
    rc = load_library().slam_op_unpad_pack(_ptr(ids), _ptr(labels), _ptr(lens), int(B), int(T), int(M_packed), int(pad_id),
                                           _ptr(scratch), scratch.numel() * scratch.element_size(),
                                           stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_unpad_pack failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def unpad_pack_spans(ids, labels, starts, lens, B: int, T: int, M_packed: int, pad_id: int, scratch,
                     stream: Optional[int] = None):
    """slam_op_unpad_pack_spans: unpad_pack for span batches - row b's real tokens are the columns starts[b] .. starts[b] +
    lens[b] - 1 (starts int32 [B] on the device; None = right padding, slam_op_unpad_pack's own launch)."""
    rc = load_library().slam_op_unpad_pack_spans(_ptr(ids), _ptr(labels), _ptr(starts), _ptr(lens), int(B), int(T),
                                                 int(M_packed), int(pad_id), _ptr(scratch),
                                                 scratch.numel() * scratch.element_size(),
                                                 stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_unpad_pack_spans failed ({rc})" + (": invalid argument" if rc == -1 else ""))


def unpad_logits_spans(src, dst, off, starts, B: int, T: int, M_packed: int, stream: Optional[int] = None):
    """slam_op_unpad_logits_spans: packed bf16 logits src [M_packed, Vp] back to dst [B, T, V] - row b's real columns from
    starts[b] on (int32 [B] on the device, None = 0), exact zeros elsewhere. off: int32 [B + 1], as the pack leaves it."""
    rc = load_library().slam_op_unpad_logits_spans(_ptr(src), int(src.shape[-1]), _ptr(dst), int(dst.shape[-1]), _ptr(off),
                                                   _ptr(starts), int(B), int(T), int(M_packed),
                                                   stream if stream is not None else current_stream_ptr())
    if rc != 0:
        raise EngineError(f"slam_op_unpad_logits_spans failed ({rc})" + (": invalid argument" if rc == -1 else ""))


@dataclass
class TensorSpec:
    name: str
    offset: int
    rows: int
    cols: int

    @property
    def numel(self) -> int:
        return self.rows * self.cols


class Engine:
    """Thin owner of a SlamEngine handle plus the torch tensors it borrows."""

    def __init__(self, desc: SlamModelDesc, arch: int = 0, n_positions: int = 0, flags: int = 0):
        """arch 0 = Qwen2, 1 = OPT (n_positions = max_position_embeddings), 3 = Qwen3; flags: MODEL_UNTIED_HEAD
        (slam_engine_create_ex)."""
        self.lib = load_library()
        self.desc = desc
        self.arch = arch
        self.flags = flags
        h = C.c_void_p()
        rc = self.lib.slam_engine_create_ex(C.byref(desc), arch, n_positions, flags, C.byref(h))
        if rc != 0:
            raise EngineError(f"slam_engine_create_ex failed ({rc}): unsupported model description")
        self.h = h
        self.n_params = int(self.lib.slam_param_count(h))
        self.tensors: Dict[str, TensorSpec] = {}
        info = SlamTensorInfo()
        for i in range(self.lib.slam_tensor_count(h)):
            self._ck(self.lib.slam_tensor_info(h, i, C.byref(info)))
            self.tensors[info.name.decode()] = TensorSpec(info.name.decode(), info.offset, info.rows, info.cols)
        self._keep = {}

    def _ck(self, rc: int):
        if rc != 0:
            msg = self.lib.slam_last_error(self.h)
            raise EngineError(f"engine call failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.slam_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- binding ------------------------------------------------------------------------------
    def bind_params(self, params_bf16, grads_f32=None):
        import torch
        assert params_bf16.dtype == torch.bfloat16 and params_bf16.numel() == self.n_params and params_bf16.is_cuda
        if grads_f32 is not None:
            assert grads_f32.dtype == torch.float32 and grads_f32.numel() == self.n_params
        self._keep["params"], self._keep["grads"] = params_bf16, grads_f32
        self._ck(self.lib.slam_bind_params(self.h, _ptr(params_bf16), _ptr(grads_f32)))

    def bind_params_t(self, params_t_bf16):
        self._keep["params_t"] = params_t_bf16
        self._ck(self.lib.slam_bind_params_t(self.h, _ptr(params_t_bf16)))

    def refresh_transposed(self, stream=None):
        self._ck(self.lib.slam_refresh_transposed(self.h, stream if stream is not None else current_stream_ptr()))

    # -- FP8 copy of the decode projections (slam_bind_decode_w8 in the header) ------------------------------------------------
    def decode_w8_bytes(self, include_head: bool = False) -> int:
        """0: the engine refuses the path (OPT, or a K that is no multiple of 64)."""
        return int(self.lib.slam_decode_w8_bytes(self.h, int(bool(include_head))))

    def bind_decode_w8(self, buf, include_head: bool = False):
        """buf: uint8 device tensor of decode_w8_bytes(include_head); None unbinds."""
        self._keep["w8"] = buf
        n = 0 if buf is None else buf.numel() * buf.element_size()
        self._ck(self.lib.slam_bind_decode_w8(self.h, _ptr(buf), n, int(bool(include_head))))

    def quantize_decode_w8(self, stream=None):
        self._ck(self.lib.slam_quantize_decode_w8(self.h, stream if stream is not None else current_stream_ptr()))

    def decode_w8_state(self) -> int:
        return int(self.lib.slam_decode_w8_state(self.h))

    def decode_w8_launches(self) -> int:
        return int(self.lib.slam_decode_w8_launches(self.h))

    def workspace_bytes(self, max_tokens: int) -> int:
        return int(self.lib.slam_workspace_bytes(self.h, max_tokens))

    def bind_workspace(self, ws, max_tokens: int):
        self._keep["ws"] = ws
        self._ck(self.lib.slam_bind_workspace(self.h, _ptr(ws), ws.numel() * ws.element_size(), max_tokens))

    def set_option(self, key: str, value: int):
        self._ck(self.lib.slam_set_option(self.h, key.encode(), int(value)))

    # -- residual dropout (OPT; options "dropout_thr16" / "dropout_seed" / "dropout_call_next") --------------------------------
    def set_dropout(self, thr16: int, seed: Optional[int] = None):
        """thr16 = round(p * 65536); a change between zero and non-zero unbinds the workspace (bind one again)."""
        self.set_option("dropout_thr16", int(thr16))
        if seed is not None:
            self.set_dropout_seed(seed)

    def set_dropout_seed(self, seed: int):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF  # 64 unsigned bits, passed as the int64 with the same bits
        self.set_option("dropout_seed", seed - (1 << 64) if seed >= (1 << 63) else seed)

    def arm_dropout(self, call: int):
        """The next forward (only) drops, with this call number."""
        self.set_option("dropout_call_next", int(call))

    # -- NEFTune (slam_set_neftune, option "neftune_call_next") ---------------------------------------------------------------
    def set_neftune(self, alpha: float, seed: int = 0):
        """alpha = HF's neftune_noise_alpha (0 = off; EngineError when negative or not finite); seed: 64 bits. Adds no buffer."""
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF  # 64 unsigned bits, passed as the int64 with the same bits
        self._ck(self.lib.slam_set_neftune(self.h, float(alpha), seed - (1 << 64) if seed >= (1 << 63) else seed))

    def arm_neftune(self, call: int):
        """The next forward (only) draws embedding noise, with this call number."""
        self.set_option("neftune_call_next", int(call))

    # -- step ---------------------------------------------------------------------------------
    def forward(self, ids, labels=None, position_ids=None, seg_start=None, seg_end=None, B=1, T=1,
                num_items: float = 0.0, loss_out=None, logits_out=None, stream: Optional[int] = None):
        self._ck(self.lib.slam_forward(self.h, _ptr(ids), _ptr(labels), _ptr(position_ids), _ptr(seg_start),
                                       _ptr(seg_end), B, T, float(num_items), _ptr(loss_out), _ptr(logits_out),
                                       stream if stream is not None else current_stream_ptr()))

    def forward_unpadded(self, ids, labels, lens, B: int, T: int, M_packed: int, scratch, num_items: float = 0.0,
                         loss_out=None, logits_out=None, stream: Optional[int] = None):
        """slam_forward_unpadded: the right-padded [B, T] batch run as B segments of M_packed packed tokens. lens int32 [B] on
        the device; scratch: uint8 device tensor of unpadded_scratch_bytes(B, T), 256-byte aligned, kept alive here (the
        engine borrows it until backward)."""
        self._keep["unpad_scratch"] = scratch
        self._ck(self.lib.slam_forward_unpadded(self.h, _ptr(ids), _ptr(labels), _ptr(lens), B, T, int(M_packed), _ptr(scratch),
                                                scratch.numel() * scratch.element_size(), float(num_items), _ptr(loss_out),
                                                _ptr(logits_out), stream if stream is not None else current_stream_ptr()))

    def forward_unpadded_spans(self, ids, labels, starts, lens, B: int, T: int, M_packed: int, scratch, num_items: float = 0.0,
                               loss_out=None, logits_out=None, stream: Optional[int] = None):
        """slam_forward_unpadded_spans: forward_unpadded for a span batch - row b's real tokens are the columns starts[b] ..
        starts[b] + lens[b] - 1 (starts int32 [B] on the device, read inside the call only; None = right padding)."""
        self._keep["unpad_scratch"] = scratch
        self._ck(self.lib.slam_forward_unpadded_spans(self.h, _ptr(ids), _ptr(labels), _ptr(starts), _ptr(lens), B, T,
                                                      int(M_packed), _ptr(scratch), scratch.numel() * scratch.element_size(),
                                                      float(num_items), _ptr(loss_out), _ptr(logits_out),
                                                      stream if stream is not None else current_stream_ptr()))

    def last_forward_tokens(self) -> int:
        """Token rows the last forward executed: B * T of a padded call, M_packed of an unpadded one (0 without a forward)."""
        return int(self.lib.slam_last_forward_tokens(self.h))

    def seq_loglik_unpadded(self, B, ll_out, cnt_out, stream=None):
        self._ck(self.lib.slam_seq_loglik_unpadded(self.h, B, _ptr(ll_out), _ptr(cnt_out),
                                                   stream if stream is not None else current_stream_ptr()))

    def scale_loss_unpadded(self, seq_coef, B, stream=None):
        self._ck(self.lib.slam_scale_loss_unpadded(self.h, _ptr(seq_coef), B,
                                                   stream if stream is not None else current_stream_ptr()))

    def backward(self, grad_scale: float = 1.0, bucket_layers: int = 0,
                 bucket_cb: Optional[Callable[[int, int], None]] = None, stream: Optional[int] = None, final: int = 0):
        """final (option "grad_final_next"): 1 = last backward of its optimizer step (the final-value stores emit the
        gradient-norm partials), 2 = the same with the final values kept in bf16 only, in the set_grad_image buffer."""
        if final:
            self.set_option("grad_final_next", int(final))
        if bucket_cb is None:
            cb = C.cast(None, BUCKET_CB)
        else:
            # third argument: the stream the range is complete on (slam_bucket_stream; None = the backward stream)
            cb = BUCKET_CB(lambda _u, off, cnt: bucket_cb(int(off), int(cnt), self.lib.slam_bucket_stream(self.h)))
        self._ck(self.lib.slam_backward(self.h, float(grad_scale), int(bucket_layers), cb, None,
                                        stream if stream is not None else current_stream_ptr()))

    # -- KV-cached generation ---------------------------------------------------------------------
    def kv_cache_bytes(self, max_batch: int, capacity: int) -> int:
        return int(self.lib.slam_kv_cache_bytes(self.h, max_batch, capacity))

    def bind_kv_cache(self, cache, max_batch: int, capacity: int):
        """cache: a 256-byte aligned device buffer of kv_cache_bytes(max_batch, capacity) bytes, kept alive here."""
        self._keep["kv"] = cache
        self._ck(self.lib.slam_bind_kv_cache(self.h, _ptr(cache), cache.numel() * cache.element_size(), max_batch, capacity))

    def prefill(self, ids, lens, B: int, T: int, logits_out, stream: Optional[int] = None):
        """ids int64 [B, T] (right-padded), lens int32 [B]: fills the cache, fp32 logits [B, vocab] of each last prompt token."""
        self._ck(self.lib.slam_prefill(self.h, _ptr(ids), _ptr(lens), B, T, _ptr(logits_out),
                                       stream if stream is not None else current_stream_ptr()))

    def decode_step(self, ids, lens, B: int, logits_out, stream: Optional[int] = None):
        """ids int64 [B]: one token per row at position lens[b]; fp32 logits [B, vocab]; lens += 1 on the device."""
        self._ck(self.lib.slam_decode_step(self.h, _ptr(ids), _ptr(lens), B, _ptr(logits_out),
                                           stream if stream is not None else current_stream_ptr()))

    def kv_repeat(self, n: int, lens, logits=None, stream: Optional[int] = None):
        """After a prefill of B rows (no decode step yet): cache row b -> rows b n .. b n + n - 1, lens (int32 [B n], first B
        filled) and the optional fp32 logits [B n, vocab] likewise; the decode batch becomes B n."""
        self._ck(self.lib.slam_kv_repeat(self.h, int(n), _ptr(lens), _ptr(logits),
                                         stream if stream is not None else current_stream_ptr()))

    def extend(self, ids, new_lens, lens, B: int, T: int, logits_out, stream: Optional[int] = None):
        """slam_extend: ids int64 [B, T] (right-padded), new_lens int32 [B] (0 .. T real tokens per row), lens int32 [B] (the
        rows' key counts): appends the chunk behind the cached keys, fp32 logits [B, vocab] of each row's last new token (rows
        with new_lens 0 keep theirs), lens += new_lens on the device."""
        self._ck(self.lib.slam_extend(self.h, _ptr(ids), _ptr(new_lens), _ptr(lens), B, T, _ptr(logits_out),
                                      stream if stream is not None else current_stream_ptr()))

    def extend_score(self, ids, new_lens, lens, B: int, T: int, logits_out, lp_out, argmax_out=None,
                     stream: Optional[int] = None):
        """slam_extend_score: slam_extend (same cache, lens and logits_out bits) that also scores the chunk. lp_out fp32 [B, T]:
        column t, 1 <= t < new_lens[b], = the log-prob of ids[b, t] given the cache and ids[b, :t]; columns at or beyond
        max(1, new_lens[b]) = 0; column 0 is left to the caller (token_logprobs on the logits the rows held before the call).
        argmax_out int64 [B, T], optional: the greedy next token after position t (t < new_lens[b]), else -1."""
        self._ck(self.lib.slam_extend_score(self.h, _ptr(ids), _ptr(new_lens), _ptr(lens), B, T, _ptr(logits_out),
                                            _ptr(lp_out), _ptr(argmax_out),
                                            stream if stream is not None else current_stream_ptr()))

    def extend_logits(self, ids, new_lens, lens, B: int, T: int, logits_all, stream: Optional[int] = None):
        """slam_extend_logits: slam_extend (same cache and lens bits) that writes the fp32 logits of EVERY real chunk position:
        logits_all fp32 [B, T, vocab]; rows t >= new_lens[b] keep their bits. Only enqueues work."""
        self._ck(self.lib.slam_extend_logits(self.h, _ptr(ids), _ptr(new_lens), _ptr(lens), B, T, _ptr(logits_all),
                                             stream if stream is not None else current_stream_ptr()))

    def kv_rewind(self, hi: int):
        """slam_kv_rewind: lower the host bound of the cached lengths to hi (host only; the caller has lowered lens itself)."""
        self._ck(self.lib.slam_kv_rewind(self.h, int(hi)))

    def set_logit_mask(self, mask_u8=None):
        """mask_u8: uint8 device tensor of padded_vocab() bytes (non-zero = column outside the softmax) or None."""
        self._ck(self.lib.slam_set_logit_mask(self.h, _ptr(mask_u8) if mask_u8 is not None else None))

    def padded_vocab(self) -> int:
        return int(self.lib.slam_padded_vocab(self.h))

    def set_label_smoothing(self, eps: float):
        """slam_set_label_smoothing: epsilon in [0, 1) of the loss of every following forward with labels, until changed
        (0 = the plain loss kernels). EngineError outside the range."""
        self._ck(self.lib.slam_set_label_smoothing(self.h, float(eps)))

    def seq_loglik(self, labels, B, T, ll_out, cnt_out, stream=None):
        self._ck(self.lib.slam_seq_loglik(self.h, _ptr(labels), B, T, _ptr(ll_out), _ptr(cnt_out),
                                          stream if stream is not None else current_stream_ptr()))

    def scale_loss_rows(self, seq_coef, B, T, stream=None):
        self._ck(self.lib.slam_scale_loss_rows(self.h, _ptr(seq_coef), B, T,
                                               stream if stream is not None else current_stream_ptr()))

    def grad_norm(self, max_norm: float, norm_out, stream=None):
        self._ck(self.lib.slam_grad_norm(self.h, float(max_norm), _ptr(norm_out),
                                         stream if stream is not None else current_stream_ptr()))

    def adamw_step(self, master, exp_avg, exp_avg_sq, norm_out, lr, beta1, beta2, eps, weight_decay, step,
                   zero_grad=True, stream=None):
        import torch
        if exp_avg.dtype == torch.bfloat16:  # fp32 master + bf16 moments
            self._ck(self.lib.slam_adamw_step_bf16_moments(self.h, _ptr(master), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(norm_out),
                                                           float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                                           int(step), int(bool(zero_grad)),
                                                           stream if stream is not None else current_stream_ptr()))
            return
        self._ck(self.lib.slam_adamw_step(self.h, _ptr(master), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(norm_out),
                                          float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                          int(step), int(bool(zero_grad)),
                                          stream if stream is not None else current_stream_ptr()))

    def adamw_step_bf16(self, exp_avg, exp_avg_sq, norm_out, lr, beta1, beta2, eps, weight_decay, step, zero_grad=True,
                        stream=None):
        """bf16 parameters + bf16 moments, updated in place (the recipe's optimizer precision)."""
        import torch
        assert exp_avg.dtype == torch.bfloat16 and exp_avg_sq.dtype == torch.bfloat16
        self._ck(self.lib.slam_adamw_step_bf16(self.h, _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(norm_out), float(lr),
                                               float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                               int(bool(zero_grad)),
                                               stream if stream is not None else current_stream_ptr()))

    # -- sharded optimizer step (data-parallel "rs_ag") ----------------------------------------------------
    def grad_chunk_info(self):
        """(elements per gradient-norm chunk, number of chunks of the flat buffer)."""
        c = int(self.lib.slam_grad_chunk_elems())
        return c, (self.n_params + c - 1) // c

    def grad_sumsq_chunks(self, offset: int, count: int, chunk_sums, stream=None):
        self._ck(self.lib.slam_grad_sumsq_chunks(self.h, int(offset), int(count), _ptr(chunk_sums),
                                                 stream if stream is not None else current_stream_ptr()))

    def grad_norm_from_chunks(self, chunk_sums, max_norm: float, norm_out, stream=None):
        self._ck(self.lib.slam_grad_norm_from_chunks(self.h, _ptr(chunk_sums), float(max_norm), _ptr(norm_out),
                                                     stream if stream is not None else current_stream_ptr()))

    def adamw_range(self, offset: int, count: int, master, exp_avg, exp_avg_sq, norm_out, lr, beta1, beta2, eps, weight_decay,
                    step, zero_grad=False, stream=None, state_offset=None):
        """AdamW on elements [offset, offset + count): master / exp_avg / exp_avg_sq are FULL-SIZE flat tensors here (the
        range's slices are passed down); master = None selects the bf16-state form. state_offset: the moments are COMPACT
        tensors instead, and the range's moments start at that element of them (optim = "muon": no moments for Muon's elements)."""
        import torch
        o, n = int(offset), int(count)
        if state_offset is not None:
            so = int(state_offset)
            exp_avg, exp_avg_sq = _Shifted(exp_avg, so - o), _Shifted(exp_avg_sq, so - o)
        st = stream if stream is not None else current_stream_ptr()
        if master is None:
            self._ck(self.lib.slam_adamw_range_bf16(self.h, o, n, _ptr(exp_avg[o:o + n]), _ptr(exp_avg_sq[o:o + n]), _ptr(norm_out),
                                                    float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                                    int(step), int(bool(zero_grad)), st))
        elif exp_avg.dtype == torch.bfloat16:
            self._ck(self.lib.slam_adamw_range_bf16_moments(self.h, o, n, _ptr(master[o:o + n]), _ptr(exp_avg[o:o + n]),
                                                            _ptr(exp_avg_sq[o:o + n]), _ptr(norm_out), float(lr), float(beta1),
                                                            float(beta2), float(eps), float(weight_decay), int(step),
                                                            int(bool(zero_grad)), st))
        else:
            self._ck(self.lib.slam_adamw_range(self.h, o, n, _ptr(master[o:o + n]), _ptr(exp_avg[o:o + n]), _ptr(exp_avg_sq[o:o + n]),
                                               _ptr(norm_out), float(lr), float(beta1), float(beta2), float(eps),
                                               float(weight_decay), int(step), int(bool(zero_grad)), st))

    def set_decay_mask(self, flags=None):
        """slam_set_decay_mask: flags = one truthy / falsy value per engine tensor, in `tensors` order (falsy = weight_decay does
        not apply to that tensor); None clears the mask (every tensor is decayed again)."""
        if flags is None:
            self._ck(self.lib.slam_set_decay_mask(self.h, None, len(self.tensors)))
            return
        buf = (C.c_uint8 * len(flags))(*[1 if f else 0 for f in flags])
        self._ck(self.lib.slam_set_decay_mask(self.h, buf, len(flags)))

    # -- Adafactor (HF Trainer's optim = "adafactor") -------------------------------------------------------
    def adafactor_set_segments(self, segments=None):
        """slam_adafactor_set_segments: `segments` = [(offset, rows, cols, factored, pattern)] - one HF parameter each
        (UnitLM.hf_param_segments() yields them behind the name); None clears the table. Returns (state floats, workspace
        bytes) of the new table ((0, 0) when cleared)."""
        if not segments:
            self._ck(self.lib.slam_adafactor_set_segments(self.h, None, 0))
            return 0, 0
        buf = (SlamAdafactorSegment * len(segments))(*[SlamAdafactorSegment(int(o), int(r), int(c), int(bool(f)), int(p))
                                                       for o, r, c, f, p in segments])
        self._ck(self.lib.slam_adafactor_set_segments(self.h, buf, len(segments)))
        return self.adafactor_sizes()

    def adafactor_sizes(self):
        """(floats of the fp32 state buffer, bytes of the workspace) for the segment table that is set."""
        n, b = C.c_int64(0), C.c_size_t(0)
        self._ck(self.lib.slam_adafactor_sizes(self.h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def adafactor_bind_workspace(self, ws=None):
        """ws: a device tensor of at least the workspace bytes, 16-byte aligned (kept alive here); None unbinds."""
        self._keep["adafactor_ws"] = ws
        self._ck(self.lib.slam_adafactor_bind_workspace(self.h, _ptr(ws), 0 if ws is None else ws.numel() * ws.element_size()))

    def adafactor_step(self, master, state, norm_out, lr, step, weight_decay=0.0, eps1=1e-30, clip_threshold=1.0,
                       decay_rate=-0.8, zero_grad=True, stream=None):
        """slam_adafactor_step: master = the fp32 master weights, or None when the bf16 parameters are the only copy; state =
        the fp32 factor buffer of adafactor_sizes(); the defaults are HF Adafactor's."""
        self._ck(self.lib.slam_adafactor_step(self.h, _ptr(master), _ptr(state), _ptr(norm_out), float(lr), float(eps1),
                                              float(clip_threshold), float(decay_rate), float(weight_decay), int(step),
                                              int(bool(zero_grad)), stream if stream is not None else current_stream_ptr()))

    # -- Muon (optim = "muon") ----------------------------------------------------------------------------
    def muon_set_segments(self, segments=None):
        """slam_muon_set_segments: `segments` = [(offset, rows, cols, pattern)] - one decoder matrix each
        (UnitLM.hf_muon_segments() yields them behind the name); None clears the table. Returns (momentum floats, workspace
        bytes) of the new table ((0, 0) when cleared)."""
        if not segments:
            self._ck(self.lib.slam_muon_set_segments(self.h, None, 0))
            return 0, 0
        buf = (SlamMuonSegment * len(segments))(*[SlamMuonSegment(int(o), int(r), int(c), int(p), 0) for o, r, c, p in segments])
        self._ck(self.lib.slam_muon_set_segments(self.h, buf, len(segments)))
        return self.muon_sizes()

    def muon_sizes(self):
        """(floats of the fp32 momentum buffer, bytes of the workspace) for the segment table that is set."""
        n, b = C.c_int64(0), C.c_size_t(0)
        self._ck(self.lib.slam_muon_sizes(self.h, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def muon_bind_workspace(self, ws=None):
        """ws: a device tensor of at least the workspace bytes, 256-byte aligned (kept alive here); None unbinds."""
        self._keep["muon_ws"] = ws
        self._ck(self.lib.slam_muon_bind_workspace(self.h, _ptr(ws), 0 if ws is None else ws.numel() * ws.element_size()))

    def muon_classes(self):
        """The shape classes of the table: [SlamMuonClass]."""
        out = []
        for i in range(int(self.lib.slam_muon_class_count(self.h))):
            c = SlamMuonClass()
            self._ck(self.lib.slam_muon_class_info(self.h, i, C.byref(c)))
            out.append(c)
        return out

    def muon_step(self, master, momentum_buf, norm_out, lr, step, weight_decay=0.0, momentum=0.95, nesterov=True, ns_steps=5,
                  ns_coefficients=MUON_NS_COEFFICIENTS, eps=MUON_EPS, adjust_lr="match_rms_adamw", zero_grad=True, stream=None):
        """slam_muon_step: master = the fp32 master weights, or None when the bf16 parameters are the only copy; momentum_buf =
        the fp32 buffer of muon_sizes(). Updates the Muon matrices only: the caller runs adamw_range over the rest."""
        a, b, c = ns_coefficients
        self._ck(self.lib.slam_muon_step(self.h, _ptr(master), _ptr(momentum_buf), _ptr(norm_out), float(lr), float(weight_decay),
                                         float(momentum), int(bool(nesterov)), int(ns_steps), float(a), float(b), float(c),
                                         float(eps), MUON_ADJUST_LR[adjust_lr], int(step), int(bool(zero_grad)),
                                         stream if stream is not None else current_stream_ptr()))

    def op_muon_prepare(self, momentum_buf, norm_out, momentum=0.95, nesterov=True, zero_grad=False, stream=None):
        self._ck(self.lib.slam_op_muon_prepare(self.h, _ptr(momentum_buf), _ptr(norm_out), float(momentum), int(bool(nesterov)),
                                               int(bool(zero_grad)), stream if stream is not None else current_stream_ptr()))

    def op_muon_apply(self, master, o_packed, lr, step, weight_decay=0.0, adjust_lr="match_rms_adamw", stream=None):
        self._ck(self.lib.slam_op_muon_apply(self.h, _ptr(master), _ptr(o_packed), float(lr), float(weight_decay),
                                             MUON_ADJUST_LR[adjust_lr], int(step),
                                             stream if stream is not None else current_stream_ptr()))

    def add_param_wait(self, offset: int, count: int, event):
        """event: a recorded torch.cuda.Event; kept alive here until the next forward consumed it."""
        self._keep.setdefault("param_events", []).append(event)
        if len(self._keep["param_events"]) > 256:
            del self._keep["param_events"][:128]
        self._ck(self.lib.slam_add_param_wait(self.h, int(offset), int(count), C.c_void_p(int(event.cuda_event))))

    def param_wait_ms(self) -> float:
        out = C.c_float(0.0)
        self._ck(self.lib.slam_param_wait_ms(self.h, C.byref(out)))
        return float(out.value)

    def param_wait_untimed(self) -> int:
        """Parameter waits since the last call that the engine could not time (0 = param_wait_ms() was complete)."""
        out = C.c_int64(0)
        self._ck(self.lib.slam_param_wait_untimed(self.h, C.byref(out)))
        return int(out.value)

    def gateup_launch_ms(self, n_layers: int):
        """Durations (ms) of the gate|up projection launches of the last forward (option time_gateup = 1)."""
        out = (C.c_float * n_layers)()
        self._ck(self.lib.slam_gateup_launch_ms(self.h, out, n_layers))
        return [float(v) for v in out]

    def family_ms(self, capacity: int = 4096):
        """[(family name, ms)] of the last forward + backward in launch order (option time_families = 1)."""
        fam = (C.c_int32 * capacity)()
        ms = (C.c_float * capacity)()
        n = C.c_int32(0)
        self._ck(self.lib.slam_family_ms(self.h, fam, ms, capacity, C.byref(n)))
        return [(self.lib.slam_family_name(int(fam[i])).decode(), float(ms[i])) for i in range(n.value)]

    def pack_grads_bf16(self, offset: int, count: int, dst_bf16, stream=None):
        """dst_bf16[0:count] = bf16(grads[offset:offset+count]); dst_bf16: a bf16 device tensor (view) of >= count elements."""
        self._ck(self.lib.slam_pack_grads_bf16(self.h, int(offset), int(count), _ptr(dst_bf16),
                                               stream if stream is not None else current_stream_ptr()))

    def set_grad_image(self, grads_bf16):
        """The next backward also writes every final gradient value into `grads_bf16` (bf16, n_params elements; None = off)."""
        if grads_bf16 is not None:
            import torch
            assert grads_bf16.dtype == torch.bfloat16 and grads_bf16.numel() == self.n_params and grads_bf16.is_cuda
        self._keep["grad_image"] = grads_bf16
        self._ck(self.lib.slam_set_grad_image(self.h, _ptr(grads_bf16)))

    def unpack_grads_bf16(self, offset: int, count: int, src_bf16, stream=None):
        self._ck(self.lib.slam_unpack_grads_bf16(self.h, int(offset), int(count), _ptr(src_bf16),
                                                 stream if stream is not None else current_stream_ptr()))

    # ---- engine-side gradient exchange (RCCL looked up at run time; include/slam_engine.h slam_comm_*) --------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128 bytes from ncclGetUniqueId (rank 0 calls this and ships them to every rank)."""
        buf = C.create_string_buffer(128)
        rc = load_library().slam_comm_unique_id(buf, 128)
        if rc != 0:
            raise RuntimeError(f"slam_comm_unique_id failed with {rc}" + (" (librccl.so.1 not found)" if rc == -4 else ""))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        self._ck(self.lib.slam_comm_init(self.h, C.create_string_buffer(unique_id, 128), int(rank), int(world)))

    def comm_destroy(self):
        self._ck(self.lib.slam_comm_destroy(self.h))

    def allreduce_grads_async(self, offset: int, count: int, bf16_exchange: bool = False, ready_stream=None):
        """Sum grads[offset:offset+count] over the communicator on the engine's communication stream, after the work
        enqueued so far on `ready_stream` (raw handle; None = torch's current stream)."""
        self._ck(self.lib.slam_allreduce_grads_async(self.h, int(offset), int(count), int(bool(bf16_exchange)),
                                                     ready_stream if ready_stream else current_stream_ptr()))

    def reduce_scatter_grads_async(self, offset: int, count: int, bf16_exchange: bool = False, ready_stream=None):
        """Reduce-scatter grads[offset:offset+count] over the communicator: this rank ends up with the summed shard
        [offset + rank * count / world, ...) (engine communication stream, behind `ready_stream`)."""
        self._ck(self.lib.slam_reduce_scatter_grads_async(self.h, int(offset), int(count), int(bool(bf16_exchange)),
                                                          ready_stream if ready_stream else current_stream_ptr()))

    def allgather_params_async(self, offset: int, count: int, ready_stream=None):
        """All-gather the bf16 parameters of the bucket from their owners; the next forward waits per bucket."""
        self._ck(self.lib.slam_allgather_params_async(self.h, int(offset), int(count),
                                                      ready_stream if ready_stream else current_stream_ptr()))

    def comm_finish(self, stream=None):
        self._ck(self.lib.slam_comm_finish(self.h, stream if stream is not None else current_stream_ptr()))

    def zero_grads(self, stream=None):
        self._ck(self.lib.slam_zero_grads(self.h, stream if stream is not None else current_stream_ptr()))

    def join(self, stream=None):
        """Order `stream` after a pending overlapped optimizer step (call before reading the flat buffers with torch)."""
        self._ck(self.lib.slam_join(self.h, stream if stream is not None else current_stream_ptr()))

    def cast_params(self, master, stream=None):
        self._ck(self.lib.slam_cast_params(self.h, _ptr(master),
                                           stream if stream is not None else current_stream_ptr()))
