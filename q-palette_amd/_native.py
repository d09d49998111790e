"""ctypes binding of libqpal_hip.so (C-ABI: include/qpal.h).

The HIP library is the product: there is no fallback.  ``lib()`` raises if it has not been built
(``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C q-palette_amd/csrc``)."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("QPAL_LIB") or os.path.join(_HERE, "libqpal_hip.so")  # QPAL_LIB: perf experiments only
_lib = None

QPAL_SPLIT_NONE, QPAL_SPLIT_ROWS, QPAL_SPLIT_COLS = 0, 1, 2

_P, _I, _F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class TcqJob(ctypes.Structure):
    """qpal_tcq_job (include/qpal.h)"""
    _fields_ = [("out", _P), ("c1", _P), ("c2", _P), ("x", _P), ("tlut", _P), ("m", _I), ("k", _I),
                ("out_zeroed", _I), ("wscale", _P), ("oscale", _F), ("ldo", ctypes.c_long),
                ("x_had", _I), ("x_post", _F), ("x_su", _P), ("kv", _I),
                ("x_f32", _P),
                ("x_rms_eps", _F), ("x_rms_w", _P), ("accumulate", _I), ("kv2", _I), ("act_out", _P), ("x_hadk", _P), ("x_K", _I), ("act_su", _P)]


class LutJob(ctypes.Structure):
    """qpal_lut_job (include/qpal.h)"""
    _fields_ = [("out", _P), ("qweight", _P), ("x", _P), ("lut", _P), ("m", _I), ("k", _I), ("out_zeroed", _I),
                ("wscale", _P), ("oscale", _F), ("ldo", ctypes.c_long), ("x_had", _I), ("x_post", _F), ("x_su", _P),
                ("x_f32", _P),
                ("x_rms_eps", _F), ("x_rms_w", _P), ("accumulate", _I), ("act_out", _P), ("x_hadk", _P), ("x_K", _I), ("act_su", _P)]


class StopBankStruct(ctypes.Structure):
    """qpal_stop_bank (include/qpal.h)"""
    _fields_ = [(n, _P) for n in ("trans", "out_len", "n_states", "set_id", "ac_state", "stop_ids", "n_ids", "max_tokens", "min_tokens",
                                  "n_gen", "gen_bytes", "out", "reason", "text_len", "hit", "end_pos")] + [
        (n, _I) for n in ("sets", "max_states", "id_slots", "cap")]


class MoeProj(ctypes.Structure):
    """qpal_moe_proj (include/qpal.h)"""
    _fields_ = [("c1", _P), ("c2", _P), ("wscale", _P), ("m", _I), ("kv", _I), ("kv2", _I), ("out_col", _I)]


class MoeRouter(ctypes.Structure):
    """qpal_moe_router (include/qpal.h)"""
    _fields_ = [("scoring", _I), ("n_group", _I), ("topk_group", _I), ("group_score", _I), ("renorm", _I), ("routed_scale", _F),
                ("select_bias", _P), ("shared_gate", _P), ("shared_gate_out", _P)]


PEER_WS_BYTES_PER_SLOT = 256
IPC_HANDLE_BYTES = 64


_SIGNATURES = {
    "qpal_tcq_gemv_multi": [ctypes.POINTER(TcqJob), _I, _I, _I, _I, _I, _I, _P, ctypes.c_long, _P],
    "qpal_lut_tc_gemv_multi": [ctypes.POINTER(LutJob), _I, _I, _I, _I, _P, ctypes.c_long, _P],
    "qpal_tcq_gemv": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    "qpal_tcq_dequant": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    "qpal_lut_tc_gemv": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "qpal_lut_tc_dequant": [_P, _P, _P, _I, _I, _I, _I, _P],
    "qpal_lut_simt_gemv": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "qpal_lut_simt_dequant": [_P, _P, _P, _I, _I, _I, _I, _P],
    "qpal_tc_to_simt": [_P, _P, _I, _I, _I, _I, _P],
    "qpal_plan_gemv": [ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), _I, _I, _I, ctypes.POINTER(_I), _I],
    "qpal_can_fuse_rotation": [_I, _I],
    "qpal_can_fuse_rotation_k": [_I, _I, _I],
    "qpal_pack_tcq": [_P, _P, _I, _I, _I],
    "qpal_pack_tcq_states": [_P, _P, _I, _I, _I],
    "qpal_pack_lut_tc": [_P, _P, _I, _I, _I, _I],
    "qpal_pack_lut_simt": [_P, _P, _I, _I, _I, _I],
    "qpal_hadamard": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _P],
    "qpal_hadamard_rms": [_P, _P, _P, _F, _P, _P, _I, _I, _I, _F, _P],
    "qpal_hadamard_f32": [_P, _P, _P, _P, _I, _I, _I, _I, _F, _P],
    "qpal_rope_kv": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, ctypes.c_long, _P],
    "qpal_attn_decode": [_P, _P, _P, _P, _P, _I, _I, _I, ctypes.c_long, _F, _P],
    "qpal_attn_rope_decode": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, ctypes.c_long, _F, _P, ctypes.c_long, _P],
    "qpal_attn_ws_bytes": [_I, _I, _I, ctypes.c_long],
    "qpal_attn_rope_decode_batch": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _I, _I, _I, _I, ctypes.c_long, _F,
                                    _P, ctypes.c_long, _P],
    "qpal_attn_batch_ws_bytes": [_I, _I, _I, _I, ctypes.c_long],
    "qpal_attn_rope_prefill": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _I, _I, _I, _I, ctypes.c_long, _F,
                               _P, ctypes.c_long, _P],
    "qpal_attn_prefill_ws_bytes": [_I, _I, _I, _I, ctypes.c_long],
    "qpal_attn_rope_decode_batch_kv8": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _I, _I, _I, _I, ctypes.c_long,
                                        _F, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_kv8": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _I, _I, _I, _I, ctypes.c_long, _F,
                                   _P, ctypes.c_long, _P],
    "qpal_attn_rope_decode_batch_paged": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _I, _I, _I, _I,
                                          _I, _I, _I, _I, _F, _P, ctypes.c_long, _P],
    "qpal_attn_prefix_ws_bytes": [_I, _I, _I, _I, _I, ctypes.c_long],
    "qpal_attn_rope_decode_batch_shared": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _I, _I, _I, _I,
                                           _P, _P, _P, _I, _I, _I, _I, _I, _F, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_paged": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _I, _I, _I, _I,
                                     _I, _I, _I, _I, _F, _P, ctypes.c_long, _P],
    "qpal_attn_ragged_ws_bytes": [_I, _I, _I, _I, _I, ctypes.c_long],
    "qpal_attn_rope_prefill_ragged": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I,
                                      ctypes.c_long, _F, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_ragged_paged": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _P, _P, ctypes.c_long, _I,
                                            _I, _I, _I, _I, _I, _I, _I, _I, _I, _F, _P, ctypes.c_long, _P],
    "qpal_attn_rope_decode_batch_window": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _I, _I, _I, _I,
                                           _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_window": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _I, _I, _I, _I,
                                      _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_ragged_window": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _P, _P, ctypes.c_long, _I,
                                             _I, _I, _I, _I, _I, _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _P, ctypes.c_long, _P],
    "qpal_attn_rope_decode_batch_score": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _I, _I, _I, _I,
                                          _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _F, _P, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_score": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _I, _I, _I, _I,
                                     _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _F, _P, _P, ctypes.c_long, _P],
    "qpal_attn_rope_prefill_ragged_score": [_P, _P, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _P, _P, _P, _P, ctypes.c_long, _I,
                                            _I, _I, _I, _I, _I, _I, _I, _I, _I, ctypes.c_long, _F, ctypes.c_long, _F, _P, _P, ctypes.c_long,
                                            _P],
    "qpal_lm_head_argmax": [_P, _P, _F, _P, _P, _P, _P, ctypes.c_long, _I, _I, _P],
    "qpal_lm_head_ws_bytes": [_I],
    "qpal_lm_head_logits": [_P, ctypes.c_long, _P, _F, _P, _P, ctypes.c_long, _I, _I, _I, _P],
    "qpal_sample": [_P, ctypes.c_long, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "qpal_sample_trunc": [_P, ctypes.c_long, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "qpal_token_logprob": [_P, ctypes.c_long, _I, _I, _P, _P, _P, _P, _P, _P],
    "qpal_top_logprob": [_P, ctypes.c_long, _I, _I, _I, _P, _P, _P, _P, _P],
    "qpal_spec_draft": [_P, ctypes.c_long, _P, _P, _P, _P, _I, _I, _I, _I, _I, ctypes.c_long, _P, _P, _P, _P, _P, _P, _P, _P],
    "qpal_spec_accept": [_P, _P, _P, _P, _P, ctypes.c_long, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    "qpal_logit_process": [_P, ctypes.c_long, _P, ctypes.c_long, _I, _I, _P, _P, _I, _P, ctypes.c_long, _P, _P, _P, _P, ctypes.c_long, _P,
                           _P, _P, _P, _I, _P, _P, _P],
    "qpal_logit_observe": [_P, ctypes.c_long, _I, _I, _P, _I, _P, _P, _I, _P],
    "qpal_grammar_compile": [_P, _P, _I, _P, _P, _I, _I, _I, _P, ctypes.c_long, _P],
    "qpal_grammar_rows": [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P],
    "qpal_grammar_mask": [_P, ctypes.c_long, _I, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P, ctypes.c_long, _P],
    "qpal_grammar_advance": [_P, _P, _P, _I, _I, _P, _P, _I, _I, _I, _P, _P, _I, _P, _I, _P, _P, _P],
    "qpal_stop_advance": [ctypes.POINTER(StopBankStruct), _P, _P, _I, _I, _I, _P, _I, _P, _P, _P, _P, _P, ctypes.c_long, _P],
    "qpal_stop_mask": [_P, ctypes.c_long, _I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P],
    "qpal_peer_gather": [_P, ctypes.c_long, _I, ctypes.POINTER(_P), ctypes.POINTER(_P), _I, _I, _P],
    "qpal_peer_alloc": [ctypes.POINTER(_P), ctypes.c_long, _I],
    "qpal_peer_free": [_P],
    "qpal_ipc_export": [_P, ctypes.c_char_p],
    "qpal_ipc_open": [ctypes.c_char_p, ctypes.POINTER(_P)],
    "qpal_ipc_close": [_P],
    "qpal_calib_stream_read": [ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_long), _I, _P, _I, _P],
    "qpal_calib_decode_rate": [_P, _P, _I, _I, _I, _I, _P],
    "qpal_tcq_viterbi": [_P, _P, _P, _P, _I, _I, _I, _P, _P],
    "qpal_tcq_viterbi_ws_bytes": [_I],
    "qpal_vq_encode": [_P, _P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P],
    "qpal_hessian_accum": [_P, _P, _P, ctypes.c_long, _I, _I, _P],
    "qpal_lora_apply": [_P, ctypes.c_long, _P, _I, _F, _P, _P, _P, ctypes.POINTER(_I), ctypes.POINTER(_I), _I, _P, _I, _I, _I, _I, _P],
    "qpal_qkv_prep": [_P, _P, _P, ctypes.c_long, _I, _I, _I, _I, _P, _P, _P, _F, _P],
    "qpal_norm_add": [_P, ctypes.c_long, _P, ctypes.c_long, _P, _F, _I, _I, _P],
    "qpal_glu_gelu_tanh": [_P, ctypes.c_long, _P, ctypes.c_long, _I, _I, _P],
    "qpal_logit_cap": [_P, ctypes.c_long, _I, _I, _F, _P],
    "qpal_moe_max_groups": [_I, _I, _I],
    "qpal_moe_route_ws_bytes": [_I, _I, _I],
    "qpal_moe_route": [_P, ctypes.c_long, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P],
    "qpal_moe_gemv": [_P, ctypes.c_long, _I, ctypes.POINTER(MoeProj), _I, _P, ctypes.c_long, _I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I,
                      _F, _P],
    "qpal_moe_combine": [_P, ctypes.c_long, _P, ctypes.c_long, _P, _P, _I, _I, _I, _I, _I, _P],
    "qpal_moe_route_ex": [_P, ctypes.c_long, _P, _F, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P,
                          ctypes.POINTER(MoeRouter), _P],
    "qpal_moe_combine_shared": [_P, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, ctypes.c_long, _P, _I, _I, _I, _I, _I, _P],
}

HESSIAN_TILE = 128  # QPAL_HESSIAN_TILE


class QpalError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP translation unit for gfx950 and link libqpal_hip.so (cross-compiles on CPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j", str(min(8, os.cpu_count() or 1))]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise QpalError(
                f"{SO_PATH} is missing: the HIP extension is the only implementation of this path "
                "(no CPU fallback). Build it with __graft_entry__.build() or `make -C q-palette_amd/csrc`.")
        l = ctypes.CDLL(SO_PATH)
        for name, args in _SIGNATURES.items():
            if os.environ.get("QPAL_LIB") and not hasattr(l, name):
                continue  # (perf experiments: an older build of the library beside the current host code)
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = _I
        l.qpal_error_string.argtypes = [_I]
        l.qpal_error_string.restype = ctypes.c_char_p
        l.qpal_version.restype = _I
        l.qpal_attn_ws_bytes.restype = ctypes.c_long
        l.qpal_attn_batch_ws_bytes.restype = ctypes.c_long
        l.qpal_attn_prefill_ws_bytes.restype = ctypes.c_long
        l.qpal_attn_prefix_ws_bytes.restype = ctypes.c_long
        l.qpal_attn_ragged_ws_bytes.restype = ctypes.c_long
        l.qpal_lm_head_ws_bytes.restype = ctypes.c_long
        l.qpal_tcq_viterbi_ws_bytes.restype = ctypes.c_long
        l.qpal_moe_route_ws_bytes.restype = ctypes.c_long
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().qpal_error_string(rc).decode()
        raise QpalError(f"{what} failed: {msg} (code {rc})")


def exported_symbols():
    return list(_SIGNATURES) + ["qpal_error_string", "qpal_version"]
