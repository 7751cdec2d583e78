"""ctypes binding of the C ABI (include/mila_cdna4.h) for tests and bench plumbing.

PyTorch is used only to own device memory and streams: every compute call goes through
libmila_cdna4.so.  Loading fails loudly when the shared object is missing -- there is no
fallback path of any kind.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmila_cdna4.so")

MILA_OK = 0
MILA_E_INVALID_ARGUMENT = -1
MILA_E_UNSUPPORTED = -2
MILA_E_RUNTIME = -3
MILA_E_SCRATCH_TOO_SMALL = -4

FMT_BF16, FMT_FP8, FMT_FP4 = 0, 1, 2


class MilaError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("mila_cdna4 error %d: %s" % (code, text))
        self.code = code


class InvalidArgument(MilaError, ValueError):
    """reference: std::invalid_argument"""


class KvForkLayer(C.Structure):
    """mila_kv_fork_layer: one layer's record for kv_rows_fork_layers_bf16 (K and V: device addresses)"""
    _fields_ = [("K", C.c_void_p), ("V", C.c_void_p), ("NKV", C.c_int32), ("capacity", C.c_int32), ("HS", C.c_int32), ("reserved", C.c_int32)]


class KvForkLayerFp8(C.Structure):
    """mila_kv_fork_layer_fp8: one layer's record for kv_rows_fork_layers_kvfp8 (K8 / V8 bytes and Ks / Vs scales: device addresses)"""
    _fields_ = [("K8", C.c_void_p), ("V8", C.c_void_p), ("Ks", C.c_void_p), ("Vs", C.c_void_p), ("NKV", C.c_int32), ("capacity", C.c_int32), ("HS", C.c_int32),
                ("reserved", C.c_int32)]


class KvForkLayerBand(C.Structure):
    """mila_kv_fork_layer_band: one layer's record for kv_rows_fork_layers_band_bf16 (window > 0: a ring layer; 0: a flat one)"""
    _fields_ = [("K", C.c_void_p), ("V", C.c_void_p), ("NKV", C.c_int32), ("capacity", C.c_int32), ("HS", C.c_int32), ("window", C.c_int32)]


_lib = None
EXPERIMENTS_PATH = os.path.join(_HERE, "lib", "libmila_cdna4_experiments.so")


class _Libs:
    """the product library, with libmila_cdna4_experiments.so (csrc/experiments/: decode chain + engine, tests / tools only) behind it: a symbol the
    product does not export is looked up there, and only then is that library loaded"""

    def __init__(self, main):
        self.__dict__["_main"] = main
        self.__dict__["_exp"] = None

    def __getattr__(self, name):
        try:
            return getattr(self._main, name)
        except AttributeError:
            if not name.startswith("mila_cdna4_"):
                raise
        if self._exp is None:
            if not os.path.exists(EXPERIMENTS_PATH):
                raise AttributeError("%s: not exported by libmila_cdna4.so, and %s is missing" % (name, EXPERIMENTS_PATH))
            exp = C.CDLL(EXPERIMENTS_PATH)
            exp.mila_cdna4_decode_chain_scratch_bytes.restype = C.c_size_t
            exp.mila_cdna4_decode_engine_scratch_bytes.restype = C.c_size_t
            self.__dict__["_exp"] = exp
        return getattr(self._exp, name)


def load():
    """Load libmila_cdna4.so (import torch first so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -m mila_amd.build` (hipcc --offload-arch=gfx950); "
                          "there is no fallback path" % LIB_PATH)
    try:
        import torch  # noqa: F401  (loads torch's libamdhip64 first so there is one runtime in-process)
    except Exception:
        pass
    main = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)      # global: the experiments library resolves the shared runtime helpers against it
    main.mila_cdna4_last_error.restype = C.c_char_p
    main.mila_cdna4_attn_decode_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_gemm_staging_bytes.restype = C.c_size_t
    main.mila_cdna4_gemm_workspace_bytes.restype = C.c_size_t
    main.mila_cdna4_gemm_fp8_workspace_bytes.restype = C.c_size_t
    main.mila_cdna4_sample_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_gemm_w4a8_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_gemm_w8a8_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_sample_stochastic_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_attn_decode_ticket_count.restype = C.c_size_t
    main.mila_cdna4_mha_decode_scratch_bytes.restype = C.c_size_t
    main.mila_cdna4_attn_decode_chain_scratch_bytes.restype = C.c_size_t
    # the FP8 KV cache (PerChannelKvFp8<>, csrc/attention_kvfp8.hip): K8 / V8 [B, NKV, capacity, HS] e4m3 + Ks / Vs [B, NKV, capacity] fp32
    p, i, f, z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    main.mila_cdna4_kv_write_fp8.argtypes = [p, p, p, p, p, p, i, i, i, i, i, i, p]                               # K8 V8 Ks Vs k v | B chunk NKV HS start_pos capacity | stream
    main.mila_cdna4_attn_decode_kvfp8.argtypes = [p, p, p, p, p, p, p, z, i, i, i, i, i, i, i, f, p]              # Y Q K8 V8 Ks Vs scratch bytes | B NH NKV HS capacity len window | scale
    main.mila_cdna4_kv_write_fp8_devpos.argtypes = [p, p, p, p, p, p, i, i, i, p, i, p]                           # K8 V8 Ks Vs k v | B NKV HS | position_dev | capacity | stream
    main.mila_cdna4_attn_decode_kvfp8_devpos.argtypes = [p, p, p, p, p, p, p, z, i, i, i, i, i, p, i, i, f, p]    # Y Q K8 V8 Ks Vs scratch bytes | B NH NKV HS capacity | position_dev | max_len window | scale
    main.mila_cdna4_attn_decode_kvfp8_plan_describe.argtypes = [i, i, i, i, i, i, i, p, z]                        # B NH NKV HS capacity window len_hint | buf cap
    main.mila_cdna4_attn_decode_kvfp8_plan_describe.restype = z
    main.mila_cdna4_attn_prefill_plan_describe.argtypes = [i, i, i, i, i, i, p, z]                                # HS NH NKV chunk pos_offset window | buf cap
    main.mila_cdna4_attn_prefill_plan_describe.restype = z
    # the stochastic sampler's radix pipeline (csrc/sampling.hip: run_radix)
    main.mila_cdna4_sample_radix_scratch_bytes.argtypes = [i]
    main.mila_cdna4_sample_radix_scratch_bytes.restype = z
    main.mila_cdna4_sample_radix_fp32.argtypes = [p, p, i, f, f, i, f, f, p, z, p]                                # logits token_out | vocab softcap temperature top_k top_p r | scratch bytes
    main.mila_cdna4_sample_radix_bf16.argtypes = [p, p, i, f, f, i, f, f, p, z, p]
    main.mila_cdna4_sample_radix_advance_fp32.argtypes = [p, p, i, f, f, i, f, p, i, p, z, p, p, p, i, p]         # ... top_p | draws draws_size | scratch bytes | position_dev seq_dev ring ring_size
    main.mila_cdna4_sample_radix_plan_describe.argtypes = [i, i, f, p, z]                                         # vocab top_k top_p | buf cap
    main.mila_cdna4_sample_radix_plan_describe.restype = z
    main.mila_cdna4_sample_radix_rows_scratch_bytes.argtypes = [i, i]                                             # rows vocab
    main.mila_cdna4_sample_radix_rows_scratch_bytes.restype = z
    main.mila_cdna4_sample_radix_rows_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, z, p]                     # logits logits_stride token_out | rows vocab softcap temperature top_k top_p | draws | scratch bytes
    main.mila_cdna4_sample_radix_rows_advance_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, z, p, p, p]       # ... | scratch bytes | positions_dev active_dev
    main.mila_cdna4_sample_radix_chain_accept_fp32.argtypes = [p, p, p, z, i, i, f, f, i, f, p, p, z, p, p]       # tok result logits logits_stride | T vocab softcap temperature top_k top_p | draws | scratch bytes | position_dev
    # sampling filters (csrc/sampling.hip: the filtered instantiations and the token table)
    main.mila_cdna4_token_table_bytes.argtypes = [i]
    main.mila_cdna4_token_table_bytes.restype = z
    main.mila_cdna4_token_table_clear.argtypes = [p, z, i, i, p]                                                  # table table_stride row vocab
    main.mila_cdna4_token_table_mark_prompt.argtypes = [p, z, i, i, p, i, p]                                      # table table_stride row vocab | tokens_dev n
    main.mila_cdna4_sample_filters_describe.argtypes = [i, i, f, p, i, p, z]                                      # vocab top_k top_p | filters with_table | buf cap
    main.mila_cdna4_sample_filters_describe.restype = z
    main.mila_cdna4_sample_radix_filtered_fp32.argtypes = [p, p, i, f, f, i, f, f, p, p, p, z, p]                 # ... top_p r | filters table | scratch bytes
    main.mila_cdna4_sample_radix_filtered_advance_fp32.argtypes = [p, p, i, f, f, i, f, p, i, p, p, p, z, p, p, p, i, p]     # ... draws draws_size | filters table | scratch bytes | position_dev seq_dev ring ring_size
    main.mila_cdna4_sample_radix_filtered_rows_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, p, z, p, z, p]   # ... draws | filters table table_stride | scratch bytes
    main.mila_cdna4_sample_radix_filtered_rows_advance_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, p, z, p, z, p, p, p]        # ... | positions_dev active_dev
    main.mila_cdna4_sample_argmax_filtered_fp32.argtypes = [p, p, i, f, p, p, p, z, p]                            # logits token_out | vocab softcap | filters table | scratch bytes
    main.mila_cdna4_sample_argmax_filtered_advance_fp32.argtypes = [p, p, i, f, p, p, p, z, p, p, p, i, p]        # ... | position_dev seq_dev ring ring_size
    main.mila_cdna4_sample_argmax_filtered_rows_advance_fp32.argtypes = [p, z, p, i, i, f, p, p, z, p, z, p, p, p]       # logits logits_stride token_out | rows vocab softcap | filters table table_stride | scratch bytes | positions_dev active_dev
    # logit bias (csrc/sampling.hip: the bias table and the biased siblings of the filtered entries: `bias bias_stride` behind the table arguments)
    main.mila_cdna4_token_bias_bytes.argtypes = [i]
    main.mila_cdna4_token_bias_bytes.restype = z
    main.mila_cdna4_token_bias_fill.argtypes = [p, z, i, i, f, p]                                                 # bias bias_stride row vocab | value
    main.mila_cdna4_token_bias_set.argtypes = [p, z, i, i, p, p, i, p]                                            # bias bias_stride row vocab | ids_dev values_dev n
    main.mila_cdna4_sample_radix_biased_fp32.argtypes = [p, p, i, f, f, i, f, f, p, p, p, z, p, z, p]             # ... top_p r | filters table | bias bias_stride | scratch bytes
    main.mila_cdna4_sample_radix_biased_advance_fp32.argtypes = [p, p, i, f, f, i, f, p, i, p, p, p, z, p, z, p, p, p, i, p]
    main.mila_cdna4_sample_radix_biased_rows_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, p, z, p, z, p, z, p]
    main.mila_cdna4_sample_radix_biased_rows_advance_fp32.argtypes = [p, z, p, i, i, f, f, i, f, p, p, p, z, p, z, p, z, p, p, p]
    main.mila_cdna4_sample_argmax_biased_fp32.argtypes = [p, p, i, f, p, p, p, z, p, z, p]
    main.mila_cdna4_sample_argmax_biased_advance_fp32.argtypes = [p, p, i, f, p, p, p, z, p, z, p, p, p, i, p]
    main.mila_cdna4_sample_argmax_biased_rows_advance_fp32.argtypes = [p, z, p, i, i, f, p, p, z, p, z, p, z, p, p, p]
    # token automaton (csrc/sampling.hip: the effective table of a grammar-constrained row and the state step behind the sampler tail)
    main.mila_cdna4_token_automaton_bytes.argtypes = [i, i, i]                                                    # vocab S C
    main.mila_cdna4_token_automaton_bytes.restype = z
    main.mila_cdna4_token_automaton_compose.argtypes = [p, z, p, z, p, p, i, i, p, i, i, p]                       # eff eff_stride base base_stride | class_of next S C | state_dev | rows vocab
    main.mila_cdna4_token_automaton_step.argtypes = [p, z, p, z, p, p, i, i, p, p, p, p, i, i, p]                 # ... state_dev token_dev active_dev ticket_dev | rows vocab
    # the constrained chain step: the automaton's chain forms and the chain tails with a bias
    main.mila_cdna4_token_automaton_chain_compose.argtypes = [p, z, p, z, p, p, i, i, p, p, p, i, i, p]           # ... state_dev tok_dev chain_states | T vocab
    main.mila_cdna4_token_automaton_chain_step.argtypes = [p, z, p, z, p, p, i, i, p, p, p, p, i, p, i, p]        # ... state_dev tok_dev chain_states result_dev T ticket_dev | vocab
    main.mila_cdna4_sample_radix_biased_chain_accept_fp32.argtypes = [p, p, p, z, i, i, f, f, i, f, p, p, z, p, z, p, p]   # ... top_p | draws | bias bias_stride | scratch bytes | position_dev
    main.mila_cdna4_sample_argmax_biased_chain_accept_fp32.argtypes = [p, p, p, z, i, i, f, p, z, p, z, p, p]     # tok result logits logits_stride | T vocab softcap | bias bias_stride | scratch bytes | position_dev
    # row requests (csrc/sampling.hip: the sampler parameters and the automaton image of each row in device memory)
    main.mila_cdna4_sample_row_params_bytes.argtypes = [i]                                                        # rows
    main.mila_cdna4_sample_row_params_bytes.restype = z
    main.mila_cdna4_sample_row_params_set.argtypes = [p, i, p, p]                                                 # params_dev row params
    main.mila_cdna4_sample_radix_requests_rows_fp32.argtypes = [p, z, p, i, i, f, p, p, p, z, p, z, p, z, p]      # logits logits_stride token_out | rows vocab softcap | params_dev draws | table table_stride | bias bias_stride | scratch bytes
    main.mila_cdna4_sample_radix_requests_rows_advance_fp32.argtypes = [p, z, p, i, i, f, p, p, p, z, p, z, p, z, p, p, p]   # ... | positions_dev active_dev
    main.mila_cdna4_sample_argmax_requests_rows_fp32.argtypes = [p, z, p, i, i, f, p, p, z, p, z, p, z, p]        # logits logits_stride token_out | rows vocab softcap | params_dev | table table_stride | bias bias_stride | scratch bytes
    main.mila_cdna4_sample_argmax_requests_rows_advance_fp32.argtypes = [p, z, p, i, i, f, p, p, z, p, z, p, z, p, p, p]
    main.mila_cdna4_token_automaton_rows_bytes.argtypes = [i]
    main.mila_cdna4_token_automaton_rows_bytes.restype = z
    main.mila_cdna4_token_automaton_rows_set.argtypes = [p, i, p, p, i, i, i, p]                                  # desc_dev row | class_of next S C vocab
    main.mila_cdna4_token_automaton_rows_compose.argtypes = [p, z, p, z, p, p, i, i, p]                           # eff eff_stride base base_stride | desc_dev state_dev | rows vocab
    main.mila_cdna4_token_automaton_rows_step.argtypes = [p, z, p, z, p, p, p, p, p, i, i, p]                     # ... desc_dev state_dev token_dev active_dev ticket_dev | rows vocab
    # a shared prefill's device primitive (csrc/kv_rows_fork.hip)
    main.mila_cdna4_kv_rows_fork_bf16.argtypes = [p, p, i, i, i, i, i, i, i, p]                                   # K V | rows NKV capacity HS | src dst_mask len
    main.mila_cdna4_kv_rows_fork_layers_bf16.argtypes = [p, i, i, i, i, i, p]                                     # layers (host records) n_layers | rows src dst_mask len
    main.mila_cdna4_kv_rows_fork_layers_kvfp8.argtypes = [p, i, i, i, i, i, p]                                    # layers (host fp8 records) n_layers | rows src dst_mask len
    main.mila_cdna4_kv_rows_fork_layers_band_bf16.argtypes = [p, i, i, i, i, i, p]                                # layers (host band records) n_layers | rows src dst_mask len
    # token log-probabilities (csrc/logprobs.hip)
    main.mila_cdna4_token_logprobs_scratch_bytes.argtypes = [i, i, i]                                             # rows vocab top_n
    main.mila_cdna4_token_logprobs_scratch_bytes.restype = z
    main.mila_cdna4_token_logprobs_rows_fp32.argtypes = [p, z, p, i, i, f, i, p, p, p, p, p, p, z, p]             # logits logits_stride tokens_dev | rows vocab softcap top_n | active_dev count_dev | logprob_out top_ids_out top_logprobs_out | scratch bytes
    main.mila_cdna4_token_logprobs_publish_fp32.argtypes = [p, p, i, f, i, p, p, i, p, z, p]                      # logits token_dev | vocab softcap top_n | seq_dev ring ring_size | scratch bytes
    # prompt log-probabilities (csrc/lm_head_score.hip)
    main.mila_cdna4_lm_head_score_scratch_bytes.argtypes = [i, i]                                                 # rows vocab
    main.mila_cdna4_lm_head_score_scratch_bytes.restype = z
    main.mila_cdna4_lm_head_score_bf16.argtypes = [p, z, p, p, i, i, i, p, i, f, p, p, p, p, z, p]                # x x_stride W scales fmt | K vocab | targets_dev rows softcap | logprob_out argmax_out argmax_logprob_out | scratch bytes
    main.mila_cdna4_kv_dequant_fp8_bf16.argtypes = [p, p, p, p, p, p, i, i, i, i, i, i, p]                        # Kc Vc K8 V8 Ks Vs | B NKV HS capacity first_pos count
    main.mila_cdna4_attn_prefill_kvfp8_scratch_bytes.argtypes = [i, i, i, i]                                      # B NKV HS capacity
    main.mila_cdna4_attn_prefill_kvfp8_scratch_bytes.restype = z
    main.mila_cdna4_attn_prefill_kvfp8.argtypes = [p, p, p, p, p, p, p, z, i, i, i, i, i, i, i, i, f, p]          # Y Q K8 V8 Ks Vs scratch bytes | B chunk NH NKV HS capacity pos_offset window | scale
    i64 = C.c_int64
    main.mila_cdna4_fused_qkv_post_kvfp8.argtypes = [p] * 13 + [i, i, i, i, i, f, p]                              # q_out K8 V8 Ks Vs q k v_src qw kw vw cos sin | NH NKV HS position capacity | eps
    main.mila_cdna4_fused_qkv_post_kvfp8_prefill.argtypes = [p] * 8 + [i64] + [p] * 5 + [i, i, i, i, i, i, f, p]  # q_out K8 V8 Ks Vs q k v_src | stride | qw kw vw cos sin | T NH NKV HS pos_offset capacity | eps
    main.mila_cdna4_fused_qkv_post_kvfp8_devpos.argtypes = [p] * 13 + [i, i, i, p, i, f, p]                       # ... | NH NKV HS | position_dev | capacity | eps
    # the FP8 KV cache under a rows step: row b at positions_dev[b] on its own caches
    main.mila_cdna4_fused_qkv_post_kvfp8_rows_devpos.argtypes = [p] * 8 + [i64] + [p] * 5 + [i, i, i, i, p, i, f, p]   # q_out K8 V8 Ks Vs q k v_src | stride | qw kw vw cos sin | B NH NKV HS | positions_dev | capacity | eps
    main.mila_cdna4_attn_decode_kvfp8_rows.argtypes = [p, p, p, p, p, p, p, z, i, i, i, i, i, p, i, i, f, p]      # Y Q K8 V8 Ks Vs scratch bytes | B NH NKV HS capacity | positions_dev | max_len window | scale
    _lib = _Libs(main)
    return _lib


class fused_matvec_args(C.Structure):
    _fields_ = [("y", C.c_void_p), ("x", C.c_void_p), ("W", C.c_void_p), ("scales", C.c_void_p),
                ("norm_w", C.c_void_p), ("post_w", C.c_void_p), ("res", C.c_void_p), ("res_out", C.c_void_p),
                ("post_scale", C.c_float), ("eps", C.c_float), ("fmt", C.c_int), ("K", C.c_int),
                ("N", C.c_int), ("group", C.c_int), ("geglu", C.c_int), ("f32_out", C.c_int),
                ("argmax_scratch", C.c_void_p), ("argmax_scratch_bytes", C.c_size_t), ("argmax_blocks", C.POINTER(C.c_int))]


class matvec_rows_args(C.Structure):
    """mila_matvec_rows_args: `a` holds row 0's pointers, row b is b strides (in elements) further"""
    _fields_ = [("a", fused_matvec_args), ("bias", C.c_void_p), ("rows", C.c_int),
                ("x_stride", C.c_int64), ("y_stride", C.c_int64), ("res_stride", C.c_int64), ("res_out_stride", C.c_int64)]


class decode_chain_args(C.Structure):
    _fields_ = [("attn", C.c_void_p), ("res", C.c_void_p), ("res_out", C.c_void_p), ("y", C.c_void_p),
                ("W_o", C.c_void_p), ("s_o", C.c_void_p), ("W_gate_up", C.c_void_p), ("s_gate_up", C.c_void_p),
                ("W_down", C.c_void_p), ("s_down", C.c_void_p), ("W_next", C.c_void_p), ("s_next", C.c_void_p),
                ("post_attn_w", C.c_void_p), ("pre_ffn_w", C.c_void_p), ("post_ffn_w", C.c_void_p),
                ("next_norm_w", C.c_void_p), ("layer_scalar", C.c_float), ("eps", C.c_float),
                ("fmt", C.c_int), ("group", C.c_int), ("next_fmt", C.c_int), ("next_group", C.c_int),
                ("f32_out", C.c_int), ("D", C.c_int), ("F", C.c_int), ("K_attn", C.c_int), ("N_next", C.c_int),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


def _ptr(t):
    """device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    assert t.is_contiguous(), "the C ABI takes dense tensors"
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def tune(name, value):
    """set a named tuning variable (csrc/internal.h; the process must have set MILA_CDNA4_TUNING=1 before the library loaded)"""
    check(load().mila_cdna4_tune(name.encode(), C.c_int(int(value))))


def tune_reset():
    check(load().mila_cdna4_tune_reset())


def last_form():
    """the kernel forms this thread's Linear / attention entry points ran since the previous call, as a list; clears the record"""
    lib = load()
    lib.mila_cdna4_last_form.restype = C.c_size_t
    buf = C.create_string_buffer(512)
    lib.mila_cdna4_last_form(buf, C.c_size_t(512))
    return [f for f in buf.value.decode().split("+") if f]


PLAN_ENTRIES = ["gemm_bf16", "gemm_bf16_ws", "gemm_geglu_bf16", "gemm_fp8_scaled", "gemm_fp8_scaled_ws", "gemm_geglu_fp8_scaled"]


def gemm_plan(entry, M, K, N):
    """the prefill GEMM plan (csrc/gemm_plan.hip) of an entry point -- an index into, or a name of, PLAN_ENTRIES; N = F for the GeGLU entries -- as a list of
    (form, row0, rows, col0, cols, S): one kernel-form launch per rectangle of the output, S > 0 on split-K steps; the column-split marker comes first, with rows == 0.
    Needs no GPU."""
    lib = load()
    lib.mila_cdna4_gemm_plan_describe.restype = C.c_size_t
    buf = C.create_string_buffer(8192)
    need = lib.mila_cdna4_gemm_plan_describe(PLAN_ENTRIES.index(entry) if isinstance(entry, str) else int(entry), int(M), int(K), int(N), buf, C.c_size_t(len(buf)))
    assert need <= len(buf), "plan text of %d bytes" % need
    return [(f[0],) + tuple(int(v) for v in f[1:]) for f in (item.split(":") for item in buf.value.decode().split("+") if item)]


PLAN_FIELDS = ("form", "splits", "band_max", "heads_per_group", "head_groups", "flat", "prologue", "partial_floats", "scratch_need")


def attn_decode_plan(B, NH, NKV, HS, capacity, window, len_hint=0, fused=False, hooks=False):
    """the decode-attention plan (csrc/attention.hip: plan_decode) of a shape as a dict of PLAN_FIELDS: len_hint = the live-length bound the launch is for (0 = the capacity),
    fused = a fused entry, hooks = the entry uses tickets, no_combine or warm ranges.  Needs no GPU."""
    lib = load()
    lib.mila_cdna4_attn_decode_plan_describe.restype = C.c_size_t
    buf = C.create_string_buffer(256)
    need = lib.mila_cdna4_attn_decode_plan_describe(int(B), int(NH), int(NKV), int(HS), int(capacity), int(window), int(len_hint), int(fused), int(hooks), buf, C.c_size_t(len(buf)))
    assert 0 < need <= len(buf), "no plan for this shape" if not need else "plan text of %d bytes" % need
    f = buf.value.decode().split(":")
    return dict(zip(PLAN_FIELDS, [f[0]] + [int(v) for v in f[1:]]))


def attn_decode_kvfp8_plan(B, NH, NKV, HS, capacity, window, len_hint=0):
    """the plan attn_decode_kvfp8 / attn_decode_kvfp8_devpos launch from (csrc/attention.hip: plan_decode for the fp8 KV cache) as a dict of PLAN_FIELDS; form is
    attn_decode_kvfp8 or attn_decode_kvfp8_mfma.  Needs no GPU."""
    buf = C.create_string_buffer(256)
    need = load().mila_cdna4_attn_decode_kvfp8_plan_describe(int(B), int(NH), int(NKV), int(HS), int(capacity), int(window), int(len_hint), buf, C.c_size_t(len(buf)))
    assert 0 < need <= len(buf), "no plan for this shape" if not need else "plan text of %d bytes" % need
    f = buf.value.decode().split(":")
    return dict(zip(PLAN_FIELDS, [f[0]] + [int(v) for v in f[1:]]))


PREFILL_PLAN_FIELDS = ("form", "HB", "DS", "NW", "QROWS", "n_qtiles", "n_hblk", "n_items")


def attn_prefill_plan(HS, NH, NKV, chunk, pos_offset=0, window=0):
    """the plan attn_prefill_bf16 launches a chunk from (csrc/attention_prefill.hip: plan_prefill, under the current flash.form) as a dict of PREFILL_PLAN_FIELDS: HB heads x
    DS d-shares on NW waves per workgroup of QROWS query rows, n_items = n_qtiles * n_hblk workgroups per batch row.  Needs no GPU."""
    buf = C.create_string_buffer(256)
    need = load().mila_cdna4_attn_prefill_plan_describe(int(HS), int(NH), int(NKV), int(chunk), int(pos_offset), int(window), buf, C.c_size_t(len(buf)))
    assert 0 < need <= len(buf), "no plan for this shape" if not need else "plan text of %d bytes" % need
    f = buf.value.decode().split(":")
    return dict(zip(PREFILL_PLAN_FIELDS, [f[0]] + [int(v) for v in f[1:]]))


MATVEC_ROWS_PLAN_FIELDS = ("R", "U", "xc", "lds_bytes", "workgroups")


def matvec_rows_plan(fmt, K, N, geglu=False, f32_out=False, rows=1):
    """the launch of a decode Linear on `rows` input vectors (csrc/matvec_rows.hip: plan_rows; rows = 1: the one-row kernels of csrc/matvec.hip) as a dict of
    MATVEC_ROWS_PLAN_FIELDS, or None for what the entry refuses.  Needs no GPU."""
    lib = load()
    lib.mila_cdna4_matvec_rows_plan_describe.restype = C.c_size_t
    buf = C.create_string_buffer(128)
    need = lib.mila_cdna4_matvec_rows_plan_describe(int(fmt), int(K), int(N), int(bool(geglu)), int(bool(f32_out)), int(rows), buf, C.c_size_t(len(buf)))
    if not need:
        return None
    assert need <= len(buf), "plan text of %d bytes" % need
    return dict(zip(MATVEC_ROWS_PLAN_FIELDS, [int(v) for v in buf.value.decode().split(":")]))


def row_kernel_form(op, outer, dim, inner=1):
    """the kernel a row entry launches at a shape (csrc/row_kernel_plan.h), e.g. row_kernel_form("rmsnorm_bf16", 4, 3840) == "rmsnorm_block"; dim = K of
    quantize_fp8_per_token, HS of rope_forward_bf16 and the fused_qkv_post entries.  None for an unknown entry or a shape it refuses.  Needs no GPU."""
    lib = load()
    lib.mila_cdna4_row_kernel_form.restype = C.c_size_t
    buf = C.create_string_buffer(64)
    need = lib.mila_cdna4_row_kernel_form(op.encode(), int(outer), int(dim), int(inner), buf, C.c_size_t(len(buf)))
    if not need:
        return None
    assert need <= len(buf), "form name of %d bytes" % need
    return buf.value.decode()


def row_kernel_forms():
    """every name row_kernel_form can return"""
    lib = load()
    lib.mila_cdna4_row_kernel_forms.restype = C.c_size_t
    buf = C.create_string_buffer(2048)
    need = lib.mila_cdna4_row_kernel_forms(buf, C.c_size_t(len(buf)))
    assert 0 < need <= len(buf), "form list of %d bytes" % need
    return buf.value.decode().split("+")


RADIX_PLAN_FIELDS = ("launches", "k_passes", "p_passes", "scratch_need")


def sample_radix_plan(vocab, top_k, top_p):
    """what a sample_radix_* call launches (csrc/sampling.hip: plan_radix) as a dict of RADIX_PLAN_FIELDS: kernel launches, digit passes of the top-k and of the
    nucleus search (0 = that truncation is off), scratch bytes.  Needs no GPU."""
    buf = C.create_string_buffer(128)
    need = load().mila_cdna4_sample_radix_plan_describe(int(vocab), int(top_k), float(top_p), buf, C.c_size_t(len(buf)))
    assert 0 < need <= len(buf), "no plan for these arguments" if not need else "plan text of %d bytes" % need
    return dict(zip(RADIX_PLAN_FIELDS, [int(v) for v in buf.value.decode().split(":")]))


def sample_radix_scratch_bytes(vocab):
    return int(load().mila_cdna4_sample_radix_scratch_bytes(int(vocab)))


def sample_radix(logits, token_out, softcap, temperature, top_k, top_p, r, scratch, bf16=False):
    """token_out[0] <- the radix pipeline's sample from `logits` (fp32, or bf16 bits with bf16=True) at the draw r, on the current torch stream"""
    call("sample_radix_bf16" if bf16 else "sample_radix_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), float(r),
         scratch, C.c_size_t(scratch.numel() * scratch.element_size()))


def sample_radix_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, scratch, position_dev, seq_dev, ring=None):
    """the graph form's call: the draw is draws[(*seq_dev + 1) % len(draws)]; bumps *position_dev and *seq_dev, publishes seq << 32 | token into `ring` when given"""
    call("sample_radix_advance_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), draws, int(draws.numel()),
         scratch, C.c_size_t(scratch.numel() * scratch.element_size()), position_dev, seq_dev, ring, 0 if ring is None else int(ring.numel()))


def sample_radix_rows_scratch_bytes(rows, vocab):
    return int(load().mila_cdna4_sample_radix_rows_scratch_bytes(int(rows), int(vocab)))


def _radix_rows_head(logits, vocab):
    """(logits_stride, vocab) of a [rows, stride] fp32 tensor whose rows hold `vocab` logits each (default: all of the row)"""
    assert logits.dim() == 2
    return C.c_size_t(int(logits.shape[1])), int(logits.shape[1] if vocab is None else vocab)


def sample_radix_rows(logits, token_out, softcap, temperature, top_k, top_p, draws, scratch, vocab=None):
    """token_out[b] <- the radix pipeline's sample from row b of `logits` [rows, stride] (fp32) at the draw draws[b]; nothing is advanced"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_rows_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         scratch, C.c_size_t(scratch.numel() * scratch.element_size()))


def sample_radix_rows_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, scratch, positions_dev, active_dev, vocab=None):
    """the rows step's stochastic tail: token and position bump of every row whose active word is not 0"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         scratch, C.c_size_t(scratch.numel() * scratch.element_size()), positions_dev, active_dev)


def sample_radix_chain_accept(tok, result, logits, softcap, temperature, top_k, top_p, draws, scratch, position_dev, vocab=None):
    """the chain step's stochastic tail: accept the longest prefix of the drafts tok[1 ..] that the samples s_t (row t at draws[t]) confirm"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_chain_accept_fp32", tok, result, logits, stride, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         scratch, C.c_size_t(scratch.numel() * scratch.element_size()), position_dev)


class sample_filters(C.Structure):
    """mila_sample_filters: read on the host at enqueue"""
    _fields_ = [("min_p", C.c_float), ("repetition_penalty", C.c_float), ("presence_penalty", C.c_float), ("frequency_penalty", C.c_float)]


def _filters_arg(filters):
    """None (neutral), a sample_filters, or (min_p, repetition_penalty, presence_penalty, frequency_penalty) -> what ctypes passes for `const mila_sample_filters*`"""
    if filters is None:
        return None
    if not isinstance(filters, sample_filters):
        filters = sample_filters(*[float(v) for v in filters])
    return C.byref(filters)


def _nbytes(t):
    return C.c_size_t(t.numel() * t.element_size())


SAMPLE_FILTERS_FIELDS = RADIX_PLAN_FIELDS + ("scale_filtered", "mask_filtered")


def sample_filters_plan(vocab, top_k, top_p, filters=None, with_table=False):
    """what a sample_radix_filtered_* call launches (csrc/sampling.hip: plan_radix) as a dict of SAMPLE_FILTERS_FIELDS: sample_radix_plan's fields and whether the scale
    / the mask launch is the filtered instantiation; None for filters the entries refuse.  Needs no GPU."""
    buf = C.create_string_buffer(128)
    need = load().mila_cdna4_sample_filters_describe(int(vocab), int(top_k), float(top_p), _filters_arg(filters), int(bool(with_table)), buf, C.c_size_t(len(buf)))
    if not need:
        return None
    assert need <= len(buf), "plan text of %d bytes" % need
    return dict(zip(SAMPLE_FILTERS_FIELDS, [int(v) for v in buf.value.decode().split(":")]))


def token_table_bytes(vocab):
    return int(load().mila_cdna4_token_table_bytes(int(vocab)))


def _table_head(table, row):
    """(table_stride, vocab) of a [rows, vocab] or [vocab] int32 table tensor"""
    assert table.dim() in (1, 2) and table.element_size() == 4
    assert 0 <= row < (table.shape[0] if table.dim() == 2 else 1)
    return C.c_size_t(int(table.shape[-1])), int(table.shape[-1])


def token_table_clear(table, row=0):
    stride, V = _table_head(table, row)
    call("token_table_clear", table, stride, int(row), V)


def token_table_mark_prompt(table, tokens_dev, row=0, n=None):
    """bit 31 of row `row`'s words of the ids in tokens_dev (int32, on the device): into a cleared table"""
    stride, V = _table_head(table, row)
    call("token_table_mark_prompt", table, stride, int(row), V, tokens_dev, int(tokens_dev.numel() if n is None else n))


def sample_radix_filtered(logits, token_out, softcap, temperature, top_k, top_p, r, filters, table, scratch):
    """sample_radix with the filters (None / sample_filters / 4-tuple) and the token table (int32 [vocab] or None): the table word of the sample goes up by one"""
    call("sample_radix_filtered_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), float(r),
         _filters_arg(filters), table, scratch, _nbytes(scratch))


def sample_radix_filtered_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, scratch, position_dev, seq_dev, ring=None):
    call("sample_radix_filtered_advance_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), draws, int(draws.numel()),
         _filters_arg(filters), table, scratch, _nbytes(scratch), position_dev, seq_dev, ring, 0 if ring is None else int(ring.numel()))


def _tables_stride(table):
    return C.c_size_t(0 if table is None else int(table.shape[-1]))


def sample_radix_filtered_rows(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, scratch, vocab=None):
    """sample_radix_rows with the filters and the tables [rows, vocab] (row b's table is table[b])"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_filtered_rows_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         _filters_arg(filters), table, _tables_stride(table), scratch, _nbytes(scratch))


def sample_radix_filtered_rows_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, scratch, positions_dev, active_dev, vocab=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_filtered_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         _filters_arg(filters), table, _tables_stride(table), scratch, _nbytes(scratch), positions_dev, active_dev)


def sample_argmax_filtered(logits, token_out, softcap, filters, table, scratch):
    """the penalized greedy sampler: argmax of the adjusted logits x3, ties to the lower id; the table word of the token goes up by one"""
    call("sample_argmax_filtered_fp32", logits, token_out, int(logits.numel()), float(softcap), _filters_arg(filters), table, scratch, _nbytes(scratch))


def sample_argmax_filtered_advance(logits, token_out, softcap, filters, table, scratch, position_dev, seq_dev=None, ring=None):
    call("sample_argmax_filtered_advance_fp32", logits, token_out, int(logits.numel()), float(softcap), _filters_arg(filters), table, scratch, _nbytes(scratch),
         position_dev, seq_dev, ring, 0 if ring is None else int(ring.numel()))


def sample_argmax_filtered_rows_advance(logits, token_out, softcap, filters, table, scratch, positions_dev, active_dev, vocab=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_argmax_filtered_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), _filters_arg(filters), table, _tables_stride(table),
         scratch, _nbytes(scratch), positions_dev, active_dev)


# ---- logit bias: a float32 table [vocab] or [rows, vocab] on the device; the biased entries take `bias` (None: the filtered entry) and `bias_stride` (None: 0 for a
# one-dimensional table, which every row then shares, else the row length)
def token_bias_bytes(vocab):
    return int(load().mila_cdna4_token_bias_bytes(int(vocab)))


def token_bias_fill(bias, value, row=0):
    """every value of row `row` of the bias table becomes `value` (finite or -inf)"""
    stride, V = _table_head(bias, row)
    call("token_bias_fill", bias, stride, int(row), V, float(value))


def token_bias_set(bias, ids_dev, values_dev, row=0, n=None):
    """bias[row][ids[j]] = values[j] for n ids / values on the device (int32 / float32); ids outside the vocabulary are skipped"""
    stride, V = _table_head(bias, row)
    call("token_bias_set", bias, stride, int(row), V, ids_dev, values_dev, int(ids_dev.numel() if n is None else n))


def _bias_stride(bias, bias_stride):
    if bias_stride is None:
        bias_stride = 0 if bias is None or bias.dim() == 1 else int(bias.shape[-1])
    return C.c_size_t(int(bias_stride))


def sample_radix_biased(logits, token_out, softcap, temperature, top_k, top_p, r, filters, table, bias, scratch, bias_stride=None):
    """sample_radix_filtered with the bias table (float32 [vocab], or None: the filtered entry)"""
    call("sample_radix_biased_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), float(r),
         _filters_arg(filters), table, bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch))


def sample_radix_biased_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, bias, scratch, position_dev, seq_dev, ring=None, bias_stride=None):
    call("sample_radix_biased_advance_fp32", logits, token_out, int(logits.numel()), float(softcap), float(temperature), int(top_k), float(top_p), draws, int(draws.numel()),
         _filters_arg(filters), table, bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), position_dev, seq_dev, ring, 0 if ring is None else int(ring.numel()))


def sample_radix_biased_rows(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, bias, scratch, vocab=None, bias_stride=None):
    """sample_radix_filtered_rows with the bias tables: [rows, vocab] (row b's is bias[b]) or [vocab] (shared: bias_stride 0)"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_biased_rows_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         _filters_arg(filters), table, _tables_stride(table), bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch))


def sample_radix_biased_rows_advance(logits, token_out, softcap, temperature, top_k, top_p, draws, filters, table, bias, scratch, positions_dev, active_dev, vocab=None,
                                     bias_stride=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_biased_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         _filters_arg(filters), table, _tables_stride(table), bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), positions_dev, active_dev)


def sample_argmax_biased(logits, token_out, softcap, filters, table, bias, scratch, bias_stride=None):
    """the greedy sampler over the biased and penalized logits x3, ties to the lower id (table None: no penalties, no update)"""
    call("sample_argmax_biased_fp32", logits, token_out, int(logits.numel()), float(softcap), _filters_arg(filters), table, bias, _bias_stride(bias, bias_stride), scratch,
         _nbytes(scratch))


def sample_argmax_biased_advance(logits, token_out, softcap, filters, table, bias, scratch, position_dev, seq_dev=None, ring=None, bias_stride=None):
    call("sample_argmax_biased_advance_fp32", logits, token_out, int(logits.numel()), float(softcap), _filters_arg(filters), table, bias, _bias_stride(bias, bias_stride),
         scratch, _nbytes(scratch), position_dev, seq_dev, ring, 0 if ring is None else int(ring.numel()))


def sample_argmax_biased_rows_advance(logits, token_out, softcap, filters, table, bias, scratch, positions_dev, active_dev, vocab=None, bias_stride=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_argmax_biased_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), _filters_arg(filters), table, _tables_stride(table),
         bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), positions_dev, active_dev)


# ---- token automaton: class_of [vocab] and next [S, C] are 16-bit tensors on the device, state / token / active int32 [rows], ticket int32 [rows] (zero between
# launches); eff float32 [rows, vocab] (or [vocab] for one row); base None (zeros), [vocab] (shared: base_stride 0) or [rows, vocab]
TOKEN_AUTOMATON_FORBIDDEN = 0xFFFF


def token_automaton_bytes(vocab, num_states, num_classes):
    return int(load().mila_cdna4_token_automaton_bytes(int(vocab), int(num_states), int(num_classes)))


def _automaton_head(eff, base, class_of, next_table):
    assert class_of.element_size() == 2 and next_table.element_size() == 2 and next_table.dim() == 2
    rows, V = (1, int(eff.shape[0])) if eff.dim() == 1 else (int(eff.shape[0]), int(eff.shape[1]))
    assert int(class_of.numel()) == V
    base_stride = 0 if base is None or base.dim() == 1 else int(base.shape[-1])
    return rows, V, C.c_size_t(V), C.c_size_t(base_stride), int(next_table.shape[0]), int(next_table.shape[1])


def token_automaton_compose(eff, base, class_of, next_table, state_dev):
    """eff[b][i] = base[b][i] where next[state[b], class_of[i]] is not FORBIDDEN, else -inf; the state stays"""
    rows, V, es, bs, S, Cn = _automaton_head(eff, base, class_of, next_table)
    call("token_automaton_compose", eff, es, base, bs, class_of, next_table, S, Cn, state_dev, rows, V)


def token_automaton_step(eff, base, class_of, next_table, state_dev, token_dev, ticket_dev, active_dev=None):
    """every active row's state advanced by token_dev[b] (a forbidden token leaves it), eff[b] composed for the new state: one launch"""
    rows, V, es, bs, S, Cn = _automaton_head(eff, base, class_of, next_table)
    call("token_automaton_step", eff, es, base, bs, class_of, next_table, S, Cn, state_dev, token_dev, active_dev, ticket_dev, rows, V)


def _automaton_chain_head(eff, base, class_of, next_table):
    """the chain forms: eff float32 [rows >= T, eff_stride] (the first class_of.numel() floats of a row are its table), base None, [vocab] or [rows, base_stride]"""
    assert class_of.element_size() == 2 and next_table.element_size() == 2 and next_table.dim() == 2 and eff.dim() == 2
    base_stride = 0 if base is None or base.dim() == 1 else int(base.shape[-1])
    return int(class_of.numel()), C.c_size_t(int(eff.shape[1])), C.c_size_t(base_stride), int(next_table.shape[0]), int(next_table.shape[1])


def token_automaton_chain_compose(eff, base, class_of, next_table, state_dev, tok_dev, chain_states, T):
    """rows 1 .. T - 1 of eff composed for the states behind the drafts tok[1 ..], the states q_0 .. q_{T-1} to chain_states; row 0 and the state word stay"""
    V, es, bs, S, Cn = _automaton_chain_head(eff, base, class_of, next_table)
    call("token_automaton_chain_compose", eff, es, base, bs, class_of, next_table, S, Cn, state_dev, tok_dev, chain_states, int(T), V)


def token_automaton_chain_step(eff, base, class_of, next_table, state_dev, tok_dev, chain_states, result_dev, T, ticket_dev):
    """behind the accept tail: the state word = chain_states[result[0] - 1] advanced by tok[0], eff row 0 composed for it"""
    V, es, bs, S, Cn = _automaton_chain_head(eff, base, class_of, next_table)
    call("token_automaton_chain_step", eff, es, base, bs, class_of, next_table, S, Cn, state_dev, tok_dev, chain_states, result_dev, int(T), ticket_dev, V)


def sample_radix_biased_chain_accept(tok, result, logits, softcap, temperature, top_k, top_p, draws, bias, scratch, position_dev, vocab=None, bias_stride=None):
    """sample_radix_chain_accept with the bias tables: [T, stride] (row t's is bias[t]), [vocab] (shared: bias_stride 0) or None (the unbiased entry)"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_biased_chain_accept_fp32", tok, result, logits, stride, int(logits.shape[0]), V, float(softcap), float(temperature), int(top_k), float(top_p), draws,
         bias, _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), position_dev)


def sample_argmax_biased_chain_accept(tok, result, logits, softcap, bias, scratch, position_dev, vocab=None, bias_stride=None):
    """the greedy chain tail from the logits: row t's argmax over the capped logits plus its bias table, then the chain's acceptance rule"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_argmax_biased_chain_accept_fp32", tok, result, logits, stride, int(logits.shape[0]), V, float(softcap), bias, _bias_stride(bias, bias_stride), scratch,
         _nbytes(scratch), position_dev)


# ---- row requests: the sampler parameters of each row as a 32-byte record in device memory (params_dev: a uint8 / int32 tensor of sample_row_params_bytes(rows)
# bytes), written by a host-validated setter; the requests entries read row b's record, table[b] (only where the record has a penalty) and bias[b]
class sample_row_params(C.Structure):
    """mila_sample_row_params: temperature <= 0 = greedy; inv_rep is the setter's to write"""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("min_p", C.c_float), ("repetition_penalty", C.c_float), ("inv_rep", C.c_float),
                ("presence_penalty", C.c_float), ("frequency_penalty", C.c_float)]


class token_automaton_row(C.Structure):
    """mila_token_automaton_row: the image of one row; class_of NULL = the row has no automaton"""
    _fields_ = [("class_of", C.c_void_p), ("next", C.c_void_p), ("S", C.c_int32), ("C", C.c_int32)]


def sample_row_params_bytes(rows):
    return int(load().mila_cdna4_sample_row_params_bytes(int(rows)))


def sample_row_params_set(params_dev, row, temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """params_dev[row] <- the validated record, in stream order"""
    rec = sample_row_params(float(temperature), int(top_k), float(top_p), float(min_p), float(repetition_penalty), 0.0, float(presence_penalty), float(frequency_penalty))
    call("sample_row_params_set", params_dev, int(row), C.byref(rec))


def sample_radix_requests_rows(logits, token_out, softcap, params_dev, draws, table, bias, scratch, vocab=None, bias_stride=None):
    """the stochastic rows of a requests call: token_out[b] <- row b's sample under ITS record at draws[b]; a greedy row's word is not touched"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_requests_rows_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), params_dev, draws, table, _tables_stride(table), bias,
         _bias_stride(bias, bias_stride), scratch, _nbytes(scratch))


def sample_radix_requests_rows_advance(logits, token_out, softcap, params_dev, draws, table, bias, scratch, positions_dev, active_dev, vocab=None, bias_stride=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_radix_requests_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), params_dev, draws, table, _tables_stride(table), bias,
         _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), positions_dev, active_dev)


def sample_argmax_requests_rows(logits, token_out, softcap, params_dev, table, bias, scratch, vocab=None, bias_stride=None):
    """the greedy rows of a requests call: token_out[b] <- argmax of row b's adjusted logits, ties to the lower id; a stochastic row's word is not touched"""
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_argmax_requests_rows_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), params_dev, table, _tables_stride(table), bias,
         _bias_stride(bias, bias_stride), scratch, _nbytes(scratch))


def sample_argmax_requests_rows_advance(logits, token_out, softcap, params_dev, table, bias, scratch, positions_dev, active_dev, vocab=None, bias_stride=None):
    stride, V = _radix_rows_head(logits, vocab)
    call("sample_argmax_requests_rows_advance_fp32", logits, stride, token_out, int(logits.shape[0]), V, float(softcap), params_dev, table, _tables_stride(table), bias,
         _bias_stride(bias, bias_stride), scratch, _nbytes(scratch), positions_dev, active_dev)


def token_automaton_rows_bytes(rows):
    return int(load().mila_cdna4_token_automaton_rows_bytes(int(rows)))


def token_automaton_rows_set(desc_dev, row, class_of, next_table, vocab=None):
    """desc_dev[row] <- the image (class_of [vocab], next [S, C], 16-bit tensors on the device), or the null descriptor when both are None; in stream order"""
    if class_of is None and next_table is None:
        call("token_automaton_rows_set", desc_dev, int(row), None, None, 0, 0, 0)
        return
    assert class_of.element_size() == 2 and next_table.element_size() == 2 and next_table.dim() == 2
    call("token_automaton_rows_set", desc_dev, int(row), class_of, next_table, int(next_table.shape[0]), int(next_table.shape[1]),
         int(class_of.numel() if vocab is None else vocab))


def _automaton_rows_head(eff, base, vocab):
    assert eff.dim() == 2
    base_stride = 0 if base is None or base.dim() == 1 else int(base.shape[-1])
    return int(eff.shape[0]), int(eff.shape[1] if vocab is None else vocab), C.c_size_t(int(eff.shape[1])), C.c_size_t(base_stride)


def token_automaton_rows_compose(eff, base, desc_dev, state_dev, vocab=None):
    """token_automaton_compose with row b's image from desc_dev[b]; a row with the null descriptor is not touched"""
    rows, V, es, bs = _automaton_rows_head(eff, base, vocab)
    call("token_automaton_rows_compose", eff, es, base, bs, desc_dev, state_dev, rows, V)


def token_automaton_rows_step(eff, base, desc_dev, state_dev, token_dev, ticket_dev, active_dev=None, vocab=None):
    """token_automaton_step with row b's image from desc_dev[b]; a row with the null descriptor or a zero active word is not touched"""
    rows, V, es, bs = _automaton_rows_head(eff, base, vocab)
    call("token_automaton_rows_step", eff, es, base, bs, desc_dev, state_dev, token_dev, active_dev, ticket_dev, rows, V)


TOKEN_LOGPROBS_MAX_TOP = 20


def token_logprobs_record_words():
    return int(load().mila_cdna4_token_logprobs_record_words())


def token_logprobs_scratch_bytes(rows, vocab, top_n):
    return int(load().mila_cdna4_token_logprobs_scratch_bytes(int(rows), int(vocab), int(top_n)))


def token_logprobs_rows(logits, tokens_dev, softcap, top_n, logprob_out, top_ids_out, top_logprobs_out, scratch, active_dev=None, count_dev=None, vocab=None):
    """logprob_out[b] <- the log-probability of tokens_dev[b] under row b of `logits` [rows, stride] (fp32), top_ids_out / top_logprobs_out [rows, top_n] <- the top_n
    alternatives (None when top_n == 0); a row whose active word is 0, or whose index is >= *count_dev, is left untouched"""
    stride, V = _radix_rows_head(logits, vocab)
    call("token_logprobs_rows_fp32", logits, stride, tokens_dev, int(logits.shape[0]), V, float(softcap), int(top_n), active_dev, count_dev, logprob_out, top_ids_out,
         top_logprobs_out, scratch, C.c_size_t(scratch.numel() * scratch.element_size()))


def token_logprobs_publish(logits, token_dev, softcap, top_n, seq_dev, ring, scratch, ring_size=None):
    """the one-row form: one record of token_logprobs_record_words() 32-bit words into slot *seq_dev % ring_size of the host-visible `ring`, the tag word last"""
    words = token_logprobs_record_words()
    call("token_logprobs_publish_fp32", logits, token_dev, int(logits.numel()), float(softcap), int(top_n), seq_dev, ring,
         int(ring.numel() // words) if ring_size is None else int(ring_size), scratch, C.c_size_t(scratch.numel() * scratch.element_size()))


LM_HEAD_SCORE_TILE = 128
LM_HEAD_SCORE_MAX_SLABS = 256


def lm_head_score_slab(vocab):
    """the slab rule of lm_head_score (include/mila_cdna4.h), restated: vocabulary columns per slab -- a function of vocab alone"""
    tiles = -(-int(vocab) // LM_HEAD_SCORE_TILE)
    return LM_HEAD_SCORE_TILE * -(-tiles // LM_HEAD_SCORE_MAX_SLABS)


def lm_head_score_scratch_bytes(rows, vocab):
    return int(load().mila_cdna4_lm_head_score_scratch_bytes(int(rows), int(vocab)))


def lm_head_score(x, W, scales, targets_dev, softcap, logprob_out, argmax_out=None, argmax_logprob_out=None, scratch=None, rows=None):
    """logprob_out[r] <- log-probability of targets_dev[r] under softmax(softcap(x[r] @ W^T)); x [rows, K] bf16 (any row stride), W [vocab, K] bf16, or e4m3 bytes with
    per-row `scales`; argmax_out / argmax_logprob_out (both or neither) <- the greedy token and its log-probability.  No logits are stored."""
    rows = int(x.shape[0]) if rows is None else int(rows)
    K, V = int(x.shape[1]), int(W.shape[0])
    if scratch is None:
        import torch
        scratch = torch.empty(max(lm_head_score_scratch_bytes(rows, V), 16), dtype=torch.uint8, device=x.device)
    assert x.stride(1) == 1
    call("lm_head_score_bf16", C.c_void_p(x.data_ptr()), C.c_size_t(int(x.stride(0))), W, scales, 0 if scales is None else 1, K, V, targets_dev, rows, float(softcap), logprob_out, argmax_out,
         argmax_logprob_out, scratch, C.c_size_t(scratch.numel() * scratch.element_size()))


def prefill_form_name(plan, HS):
    """what last_form() reports for a launch from this plan: the form and its instantiation"""
    return plan["form"] if plan["form"] == "attn_generic" else "%s_hs%d_hb%d_ds%d_nw%d" % (plan["form"], HS, plan["HB"], plan["DS"], plan["NW"])


def check(rc):
    if rc == MILA_OK:
        return
    text = load().mila_cdna4_last_error().decode()
    if rc == MILA_E_INVALID_ARGUMENT:
        raise InvalidArgument(rc, text)
    raise MilaError(rc, text)


def call(name, *args):
    """call mila_cdna4_<name>(*args, current torch stream) and raise on a non-zero status."""
    fn = getattr(load(), "mila_cdna4_" + name)
    conv = []
    for a in args:
        if a is None or isinstance(a, (C.c_void_p, C.c_float, C.c_int, C.c_int64, C.c_size_t)):
            conv.append(a)
        elif isinstance(a, float):
            conv.append(C.c_float(a))
        elif isinstance(a, int):
            conv.append(C.c_int(a))
        elif hasattr(a, "data_ptr"):
            conv.append(_ptr(a))
        else:
            conv.append(a)
    check(fn(*conv, _stream()))


EXPORTED = [
    "last_error", "abi_version", "device_count", "set_device", "device_info", "stream_create",
    "stream_destroy", "stream_synchronize", "malloc", "free", "host_alloc_pinned", "host_free_pinned",
    "memcpy_h2d", "memcpy_d2h", "memcpy_d2d", "memset_zero",
    "matvec_bf16", "matvec_bf16_qfp8", "matvec_bf16_qfp4", "matvec_f32out",
    "gemm_bf16", "gemm_gelu_bf16", "gemm_workspace_bytes", "gemm_bf16_ws", "gemm_bf16_w8a16", "gemm_bf16_w4a16", "gemm_staging_bytes", "gemm_bf16_w8a16_staged", "gemm_bf16_w4a16_staged",
    "fp4_weight_fp8_scale", "upcast_fp4_to_fp8", "quantize_fp8_per_token", "gemm_fp8_applicable", "gemm_fp8_scaled", "gemm_fp8_workspace_bytes", "gemm_fp8_scaled_ws",
    "gemm_w4a8_scratch_bytes", "gemm_bf16_w4a8", "gemm_geglu_w4a8_applicable", "gemm_geglu_bf16_w4a8",
    "gemm_geglu_applicable", "gemm_geglu_preferred", "gemm_geglu_bf16", "gemm_geglu_bf16_w8a16_staged", "gemm_geglu_bf16_w4a16_staged",
    "quantize_fp8_per_channel", "quantize_fp4_per_group",
    "kv_write_bf16", "attn_decode_scratch_bytes", "attn_decode_bf16", "attn_prefill_bf16", "attn_prefill_plan_describe", "mha_bf16", "mha_kv_write_bf16", "mha_decode_scratch_bytes", "mha_decode_bf16",
    "rmsnorm_bf16", "rmsnorm_fp32", "layernorm_bf16", "layernorm_fp32", "softmax_fp32", "softmax_bf16",
    "gelu_bf16", "gelu_fp32", "geglu_bf16", "residual_bf16", "residual_fp32",
    "rope_build_cache", "rope_forward_bf16",
    "embedding_gather_bf16", "embedding_gather_bf16_qfp8", "lpe_bf16", "split3_bf16", "scale_bf16",
    "convert_f32_to_bf16", "convert_bf16_to_f32", "fill_uniform_bf16",
    "sample_scratch_bytes", "sample_argmax_fp32", "sample_argmax_bf16",
    "sample_stochastic_scratch_bytes", "sample_stochastic_fp32", "sample_stochastic_bf16",
    "sample_radix_scratch_bytes", "sample_radix_fp32", "sample_radix_bf16", "sample_radix_advance_fp32", "sample_radix_plan_describe",
    "fused_norm_matvec", "fused_qkv_post", "fused_qkv_post_prefill", "fused_tail_norm_bf16", "fused_tail_norm_quant_bf16",
    "attn_decode_bf16_devpos", "fused_qkv_post_devpos", "advance_position", "advance_position_snapshot", "snapshot_token", "sample_argmax_advance_fp32", "sample_argmax_final_advance", "fused_attn_decode_batch_bf16", "fused_attn_decode_bf16",
    "attn_decode_band_bucket", "dequantize_to_bf16", "gemm_geglu_fp8_scaled",
    "gemm_fp8_w8a8_ws", "gemm_geglu_fp8_w8a8", "gemm_w8a8_scratch_bytes", "gemm_bf16_w8a8", "gemm_geglu_bf16_w8a8",
    "matvec_fp32", "gemm_fp32", "mha_fp32", "mha_kv_write_fp32", "mha_decode_fp32", "lpe_fp32", "rope_forward_fp32",
    "kv_write_fp8", "attn_decode_kvfp8", "kv_dequant_fp8_bf16", "attn_prefill_kvfp8_scratch_bytes", "attn_prefill_kvfp8",
    "kv_write_fp8_devpos", "attn_decode_kvfp8_devpos", "attn_decode_kvfp8_plan_describe",
    "fused_qkv_post_kvfp8", "fused_qkv_post_kvfp8_prefill", "fused_qkv_post_kvfp8_devpos",
    "matvec_rows", "fused_attn_decode_rows_bf16", "sample_argmax_rows_final_advance", "advance_positions_rows",
    "fused_attn_decode_chain_bf16", "attn_decode_chain_scratch_bytes", "fused_qkv_post_rows_devpos", "sample_argmax_chain_accept",
    "sample_radix_rows_scratch_bytes", "sample_radix_rows_fp32", "sample_radix_rows_advance_fp32", "sample_radix_chain_accept_fp32",
    "token_logprobs_record_words", "token_logprobs_scratch_bytes", "token_logprobs_rows_fp32", "token_logprobs_publish_fp32",
    "lm_head_score_scratch_bytes", "lm_head_score_bf16",
    "token_table_bytes", "token_table_clear", "token_table_mark_prompt", "sample_filters_describe",
    "sample_radix_filtered_fp32", "sample_radix_filtered_advance_fp32", "sample_radix_filtered_rows_fp32", "sample_radix_filtered_rows_advance_fp32",
    "sample_argmax_filtered_fp32", "sample_argmax_filtered_advance_fp32", "sample_argmax_filtered_rows_advance_fp32",
    "token_bias_bytes", "token_bias_fill", "token_bias_set",
    "sample_radix_biased_fp32", "sample_radix_biased_advance_fp32", "sample_radix_biased_rows_fp32", "sample_radix_biased_rows_advance_fp32",
    "sample_argmax_biased_fp32", "sample_argmax_biased_advance_fp32", "sample_argmax_biased_rows_advance_fp32",
    "token_automaton_bytes", "token_automaton_compose", "token_automaton_step",
    "token_automaton_chain_compose", "token_automaton_chain_step", "sample_radix_biased_chain_accept_fp32", "sample_argmax_biased_chain_accept_fp32",
    "sample_row_params_bytes", "sample_row_params_set", "sample_radix_requests_rows_fp32", "sample_radix_requests_rows_advance_fp32",
    "sample_argmax_requests_rows_fp32", "sample_argmax_requests_rows_advance_fp32",
    "token_automaton_rows_bytes", "token_automaton_rows_set", "token_automaton_rows_compose", "token_automaton_rows_step",
    "kv_rows_fork_bf16", "kv_rows_fork_layers_bf16",
    "fused_qkv_post_kvfp8_rows_devpos", "attn_decode_kvfp8_rows", "kv_rows_fork_layers_kvfp8",
    "kv_rows_fork_layers_band_bf16",
]

# csrc/internal.h: test / tuning hooks and the measured-slower experiments -- exported, but not part of the drop-in ABI
INTERNAL = [
    "tune", "tune_get", "tune_reset", "tune_list", "last_form", "gemm_plan_describe", "attn_decode_plan_describe", "matvec_rows_plan_describe",
    "row_kernel_form", "row_kernel_forms",
    "decode_engine_debug",
    "selftest_decode", "selftest_wave_reduce", "selftest_mfma_fp8", "stream_copy", "stream_read",
    "attn_decode_split_count", "fused_attn_decode_partials_bf16", "matvec_attn_combine",
    "decode_chain_scratch_bytes", "decode_chain_init", "decode_chain_status", "decode_chain",
    "decode_engine_scratch_bytes", "decode_engine_init", "decode_engine_status", "decode_engine_applicable", "decode_engine",
    "attn_decode_ticket_count", "fused_attn_decode_onepass_bf16", "prefetch_l3", "fused_attn_decode_ex",
    "exp_gemm4w_bf16", "exp_gemm4w_geglu_bf16",
]
# ... of which these live in libmila_cdna4_experiments.so
EXPERIMENTS_LIB = [
    "decode_chain_scratch_bytes", "decode_chain_init", "decode_chain_status", "decode_chain",
    "decode_engine_scratch_bytes", "decode_engine_init", "decode_engine_status", "decode_engine_applicable", "decode_engine", "decode_engine_debug",
    "exp_gemm4w_bf16", "exp_gemm4w_geglu_bf16",
]
