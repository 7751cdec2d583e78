"""ctypes binding of libmila_host.so: the C++ host mirror's model runners (GemmaTransformer<TWeightQuant>
on DeviceType::Rocm).  Used by bench.py and the model-level tests; loading fails loudly if the
library is missing."""
import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmila_host.so")
POLICIES = {"bf16": 0, "fp8": 1, "fp4": 2}
_lib = None


class GemmaConfigC(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("vocab_size", "embedding_dim", "num_layers", "num_heads", "num_kv_heads",
                                         "head_dim", "hidden_dim", "global_head_dim", "num_global_kv_heads", "window",
                                         "sliding_window_pattern", "global_rotary_dim", "bounded_local_kv", "kv_fp8")]


GEMMA4_12B = dict(vocab_size=262144, embedding_dim=3840, num_layers=48, num_heads=16, num_kv_heads=8, head_dim=256,
                  hidden_dim=15360, global_head_dim=512, num_global_kv_heads=1, window=1024, sliding_window_pattern=6,
                  global_rotary_dim=128)


def load():
    global _lib
    if _lib is None:
        capi.load()      # libmila_cdna4 first (and torch's HIP runtime before both)
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -m mila_amd.build`; there is no fallback path" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.mila_host_last_error.restype = C.c_char_p
        _lib.mila_gemma_create.restype = C.c_void_p
        _lib.mila_gemma_create.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_uint64, C.c_int]
        _lib.mila_gemma_destroy.argtypes = [C.c_void_p]
        _lib.mila_gemma_init_synthetic.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        _lib.mila_gemma_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        _lib.mila_gemma_decode.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int, C.c_void_p]
        _lib.mila_gemma_time_decode.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.mila_gemma_time_dominant_kernel.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib.mila_gemma_time_prefill.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        _lib.mila_gemma_info.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        _lib.mila_gemma_generate.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        _lib.mila_gemma_generate_sampled.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint32, C.c_void_p]      # ... mode pipeline | temperature top_k top_p seed | out
        _lib.mila_gemma_set_fp8_activation_prefill.argtypes = [C.c_void_p, C.c_int]
        _lib.mila_gemma_set_fused_prefill.argtypes = [C.c_void_p, C.c_int]
        _lib.mila_gemma_set_resident_prefill_weights.argtypes = [C.c_void_p, C.c_int]
        _lib.mila_gemma_save_safetensors.argtypes = [C.c_void_p, C.c_char_p]
        _lib.mila_gemma_load_safetensors.argtypes = [C.c_void_p, C.c_char_p]
        _lib.mila_gemma_save_milabin.argtypes = [C.c_void_p, C.c_char_p]
        _lib.mila_gemma_load_pretrained.argtypes = [C.c_void_p, C.c_char_p]
        _lib.mila_pretrained_list.restype = C.c_int64
        _lib.mila_pretrained_list.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
        _lib.mila_pretrained_to_milabin.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        _lib.mila_pretrained_metadata_roundtrip.restype = C.c_int64
        _lib.mila_pretrained_metadata_roundtrip.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
        _lib.mila_safetensors_list.restype = C.c_int64
        _lib.mila_safetensors_list.argtypes = [C.c_char_p, C.c_char_p, C.c_int64]
        _lib.mila_safetensors_copy.argtypes = [C.c_char_p, C.c_char_p]
        _lib.mila_gpt_last_error.restype = C.c_char_p
        _lib.mila_gpt_create.restype = C.c_void_p
        _lib.mila_gpt_create.argtypes = [C.c_int64] * 7
        _lib.mila_gpt_destroy.argtypes = [C.c_void_p]
        _lib.mila_gpt_parameter_count.restype = C.c_int64
        _lib.mila_gpt_parameter_count.argtypes = [C.c_void_p]
        _lib.mila_gpt_load_parameter.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        _lib.mila_gpt_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def _check(rc):
    if rc != 0:
        text = load().mila_host_last_error().decode()
        if rc == capi.MILA_E_INVALID_ARGUMENT:
            raise ValueError(text)
        raise RuntimeError(text)


def _logprobs_n(n):
    """the top-n of a logprobs argument: 0 .. 20 (0 = the chosen token's log-probability only)"""
    n = int(n)
    if n < 0 or n > capi.TOKEN_LOGPROBS_MAX_TOP:
        raise ValueError("logprobs must be 0 .. %d (got %d)" % (capi.TOKEN_LOGPROBS_MAX_TOP, n))
    return n


def _filters(min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """the sampling filters as (min_p, repetition_penalty, presence_penalty, frequency_penalty) floats; ValueError for what the C ABI refuses with
    MILA_E_INVALID_ARGUMENT (include/mila_cdna4.h: sampling filters): a non-finite value, repetition_penalty <= 0, min_p outside [0, 1)"""
    f = tuple(float(v) for v in (min_p, repetition_penalty, presence_penalty, frequency_penalty))
    if not all(np.isfinite(v) for v in f):
        raise ValueError("sampling filters must be finite (got min_p=%g repetition_penalty=%g presence_penalty=%g frequency_penalty=%g)" % f)
    if f[1] <= 0.0:
        raise ValueError("repetition_penalty must be > 0 (got %g)" % f[1])
    if not 0.0 <= f[0] < 1.0:
        raise ValueError("min_p must be in [0, 1) (got %g)" % f[0])
    return f


class TokenBiasRequestC(C.Structure):
    """mila_token_bias_request (host/src/gemma_runner.cpp): the four bias controls of a generate request, by pointer"""
    _fields_ = [("bias_ids", C.c_void_p), ("bias_values", C.c_void_p), ("n_bias", C.c_int64), ("banned", C.c_void_p), ("n_banned", C.c_int64),
                ("allowed", C.c_void_p), ("n_allowed", C.c_int64), ("min_tokens", C.c_int32)]


def _id_list(ids, what, vocab):
    out = []
    for t in ids:
        if isinstance(t, (bool, float)) or int(t) != t:
            raise ValueError("%s: token id %r is not an integer" % (what, t))
        t = int(t)
        if t < 0 or (vocab is not None and t >= vocab):
            raise ValueError("%s: token id %d outside the vocabulary" % (what, t))
        out.append(t)
    return out


def _bias_request(logit_bias=None, banned_tokens=(), allowed_tokens=(), min_tokens=0, stop_tokens=(), max_new_tokens=None, vocab=None):
    """the bias controls of a request, checked as Mila/TokenBias.h: composeTokenBias checks them (ValueError before any call): an id outside the vocabulary, a NaN or
    infinite logit_bias value, an id twice in logit_bias, no token left with a finite value (with an explicit stop set: before the min_tokens restore too),
    min_tokens < 0 or above max_new_tokens.  -> None when the request has none of them, else (TokenBiasRequestC, the arrays it points into)."""
    items = list(logit_bias.items()) if hasattr(logit_bias, "items") else list(logit_bias or ())
    ids = _id_list([k for k, _ in items], "logit_bias", vocab)
    if len(set(ids)) != len(ids):
        raise ValueError("logit_bias: an id occurs twice")
    vals = [float(v) for _, v in items]
    for t, v in zip(ids, vals):
        if not np.isfinite(v):
            raise ValueError("logit_bias: the value of id %d is not finite" % t)
    banned = _id_list(banned_tokens, "banned_tokens", vocab)
    allowed = _id_list(allowed_tokens, "allowed_tokens", vocab)
    if isinstance(min_tokens, (bool, float)) or int(min_tokens) != min_tokens or int(min_tokens) < 0:
        raise ValueError("min_tokens must be an integer >= 0 (got %r)" % (min_tokens,))
    min_tokens = int(min_tokens)
    if max_new_tokens is not None and min_tokens > int(max_new_tokens):
        raise ValueError("min_tokens %d exceeds max_new_tokens %d" % (min_tokens, int(max_new_tokens)))
    held = set(_id_list(stop_tokens, "stop_tokens", vocab)) if min_tokens > 0 else set()
    for forbidden, when in ((set(banned), ""), (set(banned) | held, " before the min_tokens restore")):
        if allowed:
            left = len(set(allowed) - forbidden)
        else:
            left = None if vocab is None else vocab - len(forbidden)
        if left is not None and left <= 0:
            raise ValueError("no token is left with a finite bias%s" % when)
    if not (ids or banned or allowed or min_tokens):
        return None
    arrays = (np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float32), np.ascontiguousarray(banned, dtype=np.int32),
              np.ascontiguousarray(allowed, dtype=np.int32))
    ptr = [a.ctypes.data if a.size else None for a in arrays]
    return TokenBiasRequestC(ptr[0], ptr[1], arrays[0].size, ptr[2], arrays[2].size, ptr[3], arrays[3].size, min_tokens), arrays


class TokenAutomatonRequestC(C.Structure):
    """mila_token_automaton_request (host/src/gemma_runner.cpp): GenerateParams::automaton by pointer"""
    _fields_ = [("class_of", C.c_void_p), ("vocab", C.c_int64), ("next", C.c_void_p), ("num_states", C.c_int32), ("num_classes", C.c_int32), ("start", C.c_int32)]


class TokenAutomaton:
    """Mila/TokenAutomaton.h: a deterministic automaton over token ids in the compressed form the device reads -- class_of [vocab] uint16 (token id -> class) and
    next [num_states, num_classes] uint16 (state x class -> next state, FORBIDDEN = 0xFFFF: the token may not be emitted in that state).  The constructor checks
    what TokenAutomaton::validate checks (ValueError); the dead-end check needs the request's bias table and runs in generate()."""
    FORBIDDEN = 0xFFFF
    MAX_NEXT_BYTES = 256 << 20

    def __init__(self, class_of, next_table, start=0):
        class_of, next_table = np.asarray(class_of), np.asarray(next_table)
        if class_of.ndim != 1 or next_table.ndim != 2 or class_of.size < 1:
            raise ValueError("TokenAutomaton: class_of must be [vocab] and next [num_states, num_classes]")
        S, Cn = (int(d) for d in next_table.shape)
        if not 1 <= S <= 65535:
            raise ValueError("TokenAutomaton: num_states %d outside 1 .. 65535" % S)
        if not 1 <= Cn <= 65535:
            raise ValueError("TokenAutomaton: num_classes %d outside 1 .. 65535" % Cn)
        if S * Cn * 2 > self.MAX_NEXT_BYTES:
            raise ValueError("TokenAutomaton: the transition table exceeds 256 MiB")
        if isinstance(start, (bool, float)) or int(start) != start or not 0 <= int(start) < S:
            raise ValueError("TokenAutomaton: start %r is not a state" % (start,))
        if class_of.dtype.kind not in "iu" or next_table.dtype.kind not in "iu":
            raise ValueError("TokenAutomaton: class_of and next must be integer arrays")
        if class_of.min() < 0 or class_of.max() >= Cn:
            raise ValueError("TokenAutomaton: a class_of entry is not a class (0 .. %d)" % (Cn - 1))
        nt = next_table.astype(np.int64)
        if ((nt != self.FORBIDDEN) & ((nt < 0) | (nt >= S))).any():
            raise ValueError("TokenAutomaton: a next entry is neither a state (0 .. %d) nor FORBIDDEN" % (S - 1))
        self.class_of = np.ascontiguousarray(class_of, dtype=np.uint16)
        self.next = np.ascontiguousarray(next_table, dtype=np.uint16)
        self.start = int(start)

    vocab = property(lambda self: int(self.class_of.size))
    num_states = property(lambda self: int(self.next.shape[0]))
    num_classes = property(lambda self: int(self.next.shape[1]))

    @classmethod
    def from_transitions(cls, vocab, num_states, transitions, start=0):
        """{state: {token: next state}} (what is not listed is forbidden) -> the compressed form: tokens whose columns of the dense [num_states, vocab] table are
        identical share a class, numbered in the order of their first token"""
        vocab, num_states = int(vocab), int(num_states)
        if vocab < 1 or not 1 <= num_states <= 65535:
            raise ValueError("TokenAutomaton.from_transitions: vocab %d / num_states %d out of range" % (vocab, num_states))
        dense = np.full((num_states, vocab), cls.FORBIDDEN, dtype=np.uint16)
        for s_, row in transitions.items():
            if not 0 <= int(s_) < num_states:
                raise ValueError("TokenAutomaton.from_transitions: state %r is not a state" % (s_,))
            for t, n in row.items():
                if not 0 <= int(t) < vocab:
                    raise ValueError("TokenAutomaton.from_transitions: token id %r outside the vocabulary" % (t,))
                if not 0 <= int(n) < num_states:
                    raise ValueError("TokenAutomaton.from_transitions: next state %r is not a state" % (n,))
                dense[int(s_), int(t)] = int(n)
        return cls.from_dense(dense, start)

    @classmethod
    def from_dense(cls, dense, start=0):
        """a dense [num_states, vocab] table of next states / FORBIDDEN -> the compressed form"""
        dense = np.ascontiguousarray(dense, dtype=np.uint16)
        cols, first, inverse = np.unique(dense.T, axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")              # classes in the order of their first token
        rank = np.empty(len(order), dtype=np.int64)
        rank[order] = np.arange(len(order))
        return cls(rank[np.asarray(inverse).reshape(-1)], cols[order].T, start)

    def dense(self):
        """-> the [num_states, vocab] table this automaton compresses"""
        return self.next[:, self.class_of]

    def step(self, state, token):
        n = int(self.next[state, self.class_of[token]])
        return state if n == self.FORBIDDEN else n

    def allowed(self, state):
        """-> bool [vocab]: the tokens the automaton allows in `state`"""
        return self.next[state, self.class_of] != self.FORBIDDEN

    def forced_tokens(self, banned=()):
        """TokenAutomaton::forcedTokens -> int32 [num_states]: the ONE token a state allows (a transition, and not in `banned`), else -1.  Such a token is known
        before the model runs: the speculative loop of generate(speculate_constrained=True) drafts it for free.  Host only."""
        lib = load()
        lib.mila_token_automaton_forced_tokens.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        ban = np.ascontiguousarray(list(banned), dtype=np.int32)
        out = np.zeros(self.num_states, dtype=np.int32)
        areq = self._request()
        _check(lib.mila_token_automaton_forced_tokens(C.byref(areq), ban.ctypes.data if ban.size else None, int(ban.size), out.ctypes.data))
        return out

    def _request(self):
        return TokenAutomatonRequestC(self.class_of.ctypes.data, self.vocab, self.next.ctypes.data, self.num_states, self.num_classes, self.start)


class GemmaRowRequestC(C.Structure):
    """mila_gemma_row_request (host/src/gemma_runner.cpp): one row of GemmaModel::generateRequests"""
    _fields_ = [("prompt", C.c_void_p), ("n_prompt", C.c_int64), ("stop_tokens", C.c_void_p), ("n_stop", C.c_int64), ("bias", C.c_void_p), ("automaton", C.c_void_p),
                ("seed", C.c_uint64), ("temperature", C.c_float), ("top_p", C.c_float), ("filters", C.c_float * 4), ("top_k", C.c_int32), ("max_new", C.c_int32),
                ("logprobs", C.c_int32), ("speculative", C.c_int32)]


ROW_REQUEST_KEYS = ("prompt", "seed", "max_new_tokens", "stop_tokens", "temperature", "top_k", "top_p", "logprobs", "min_p", "repetition_penalty", "presence_penalty",
                    "frequency_penalty", "logit_bias", "banned_tokens", "allowed_tokens", "min_tokens", "automaton", "speculative_sampling", "speculate_constrained", "draft_hint")


class Gemma:
    """GemmaTransformer<policy> with synthetic weights on cuda:0."""

    MODES = {"reference": 0, "fused": 1, "graph": 2}

    def __init__(self, policy="bf16", config=None, max_seq=4096, max_prefill=1, seed=1234, device=None, profile=None, kv_fp8=False, max_batch=None, draft_tokens=None,
                 kv_fp8_rows=False, bounded_local_kv_rows=False):
        """device: HIP device ordinal; default = this process's LOCAL_RANK (one replica per GPU under torch.distributed.run).
        profile: synthetic-parameter multipliers {linear_gain, qk_norm_center, post_norm_center, layer_scalar, table_gain}
        (GemmaTransformer::SyntheticProfile; None = the unit-scale generator of SURVEY.md section 8d)
        kv_fp8: PerChannelKvFp8<> on every layer -- e4m3 K / V + one fp32 scale per KV head per cached token (also: config["kv_fp8"] = 1)
        max_batch: GemmaConfig::max_batch (1 .. 4) through mila_gemma_create_rows -- independent sequences per decode step (prefill_row / decode_rows); None = the
        one-sequence model of mila_gemma_create
        draft_tokens: GemmaConfig::draft_tokens (0 .. 3) through mila_gemma_create_chain -- the chain step (decode_chain) verifies that many drafted tokens; 0 builds
        the plain model through the same entry; None = not through that entry
        kv_fp8_rows: GemmaConfig::kv_fp8_rows through mila_gemma_create_rows_kv -- the FP8 KV cache (implied) on a model of max_batch 1 .. 4, one cache per row; plain
        kv_fp8 with max_batch > 1 stays refused
        bounded_local_kv_rows: GemmaConfig::bounded_local_kv_rows through mila_gemma_create_rows_ring -- rings (bounded_local_kv, implied) on the sliding-window layers
        of a model of max_batch 1 .. 4, one ring per row, forks of the live band; plain bounded_local_kv with max_batch > 1 stays refused"""
        lib = load()
        if device is None:
            from .replicas import local_device
            device = local_device()
        self.device = device
        self.cfg = dict(GEMMA4_12B if config is None else config)
        self.cfg.setdefault("bounded_local_kv", 0)      # 1: SlidingWindowKvCache on the sliding-window layers
        self.cfg.setdefault("kv_fp8", 0)                # 1: the FP8 KV cache (GemmaConfig::kv_fp8)
        if kv_fp8:
            self.cfg["kv_fp8"] = 1
        c = GemmaConfigC(**self.cfg)
        self.vocab = self.cfg["vocab_size"]
        self.max_batch = 1 if max_batch is None else int(max_batch)
        self.draft_tokens = 0 if draft_tokens is None else int(draft_tokens)
        self.kv_fp8_rows = bool(kv_fp8_rows)
        self.bounded_local_kv_rows = bool(bounded_local_kv_rows)
        if bounded_local_kv_rows:
            if kv_fp8_rows or self.cfg["kv_fp8"]:
                raise ValueError("Gemma: bounded_local_kv_rows cannot be combined with kv_fp8 / kv_fp8_rows (FP8 rings are not built)")
            if draft_tokens:
                raise ValueError("Gemma: draft_tokens cannot be combined with bounded_local_kv_rows (the chain over rings is not built)")
            lib.mila_gemma_create_rows_ring.restype = C.c_void_p
            lib.mila_gemma_create_rows_ring.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_int]
            self.h = lib.mila_gemma_create_rows_ring(POLICIES[policy], C.byref(c), max_seq, max_prefill, self.max_batch, 1, seed, device)
        elif kv_fp8_rows:
            if draft_tokens:
                raise ValueError("Gemma: draft_tokens cannot be combined with kv_fp8_rows (the chain over the FP8 KV cache is not built)")
            lib.mila_gemma_create_rows_kv.restype = C.c_void_p
            lib.mila_gemma_create_rows_kv.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_int]
            self.h = lib.mila_gemma_create_rows_kv(POLICIES[policy], C.byref(c), max_seq, max_prefill, self.max_batch, 1, seed, device)
        elif draft_tokens is not None:
            lib.mila_gemma_create_chain.restype = C.c_void_p
            lib.mila_gemma_create_chain.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int]
            self.h = lib.mila_gemma_create_chain(POLICIES[policy], C.byref(c), max_seq, max_prefill, self.max_batch, self.draft_tokens, seed, device)
        elif max_batch is None:
            self.h = lib.mila_gemma_create(POLICIES[policy], C.byref(c), max_seq, max_prefill, seed, device)
        else:
            lib.mila_gemma_create_rows.restype = C.c_void_p
            lib.mila_gemma_create_rows.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_int]
            self.h = lib.mila_gemma_create_rows(POLICIES[policy], C.byref(c), max_seq, max_prefill, self.max_batch, seed, device)
        if not self.h:
            text = lib.mila_host_last_error().decode()
            raise (ValueError if text.startswith("invalid_argument") else RuntimeError)("mila_gemma_create: " + text)
        if profile is not None:
            p = (C.c_float * 5)(*[float(profile[k]) for k in ("linear_gain", "qk_norm_center", "post_norm_center", "layer_scalar", "table_gain")])
            _check(lib.mila_gemma_init_synthetic(self.h, seed, p))

    def close(self):
        if self.h:
            load().mila_gemma_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rewind(self, position):
        """GemmaTransformer::rewindKvCache(position): True when every block accepted (False beyond the fill, or when a bounded ring has evicted what is needed)"""
        lib = load()
        lib.mila_gemma_rewind.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        ok = C.c_int()
        _check(lib.mila_gemma_rewind(self.h, int(position), C.byref(ok)))
        return bool(ok.value)

    def prefill_from(self, tokens, offset):
        """GemmaTransformer::prefillFrom: positions [0, offset) stay resident, tokens[offset:] are prefilled at their positions; logits of the last position"""
        lib = load()
        lib.mila_gemma_prefill_from.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.vocab, dtype=np.float32)
        _check(lib.mila_gemma_prefill_from(self.h, t.ctypes.data, t.size, int(offset), out.ctypes.data))
        return out

    def set_prefill_overlap(self, on):
        """prefill: the chunk's two halves as two kernel sequences on two streams (the second half's attention waits for the first half's K / V rows);
        bf16 and resident-fp8 policies, T % 512 == 0.  Identical bits."""
        lib = load()
        lib.mila_gemma_set_prefill_overlap.argtypes = [C.c_void_p, C.c_int]
        _check(lib.mila_gemma_set_prefill_overlap(self.h, int(bool(on))))

    def save_safetensors(self, path):
        """every parameter in its storage form (bf16, or e4m3 / packed e2m1 + fp32 scales) as a SafeTensors file"""
        _check(load().mila_gemma_save_safetensors(self.h, str(path).encode()))

    def load_safetensors(self, path):
        """load every parameter from a SafeTensors file; bf16 Linear weights are quantized on load under a quantized policy"""
        _check(load().mila_gemma_load_safetensors(self.h, str(path).encode()))

    def save_milabin(self, path):
        """the same tensors in the reference's MILA .bin container (what fromPretrained streams)"""
        _check(load().mila_gemma_save_milabin(self.h, str(path).encode()))

    def load_pretrained(self, path):
        """load every parameter from a MILA .bin or a SafeTensors artifact (sniffed by the leading magic)"""
        _check(load().mila_gemma_load_pretrained(self.h, str(path).encode()))

    def set_resident_prefill_weights(self, on):
        """quantized policies: keep the prefill staging of every layer Linear (fp8 -> bf16, fp4 -> e4m3) resident in HBM (default)
        or re-stage it into scratch on every forward as the reference does; identical bits"""
        _check(load().mila_gemma_set_resident_prefill_weights(self.h, int(bool(on))))

    def memory_stats(self):
        """GemmaTransformer::getRequiredMemory() (from the configuration alone) beside getMemoryStats() (what the built model holds), and the context's scratch high-water
        mark: {"required": {...}, "actual": {...}, "scratch_bytes": n} with device_parameter_bytes / device_state_bytes / host_state_bytes"""
        lib = load()
        lib.mila_gemma_memory_stats.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_double * 7)()
        _check(lib.mila_gemma_memory_stats(self.h, out))
        keys = ("device_parameter_bytes", "device_state_bytes", "host_state_bytes")
        return {"required": {k: int(out[i]) for i, k in enumerate(keys)}, "actual": {k: int(out[3 + i]) for i, k in enumerate(keys)}, "scratch_bytes": int(out[6])}

    def graph_node_count(self):
        """nodes of the captured decode graph = launches per token on the graph path (0 before the first graph-mode step)"""
        lib = load()
        lib.mila_gemma_graph_node_count.argtypes = [C.c_void_p, C.c_void_p]
        out = C.c_int64()
        _check(lib.mila_gemma_graph_node_count(self.h, C.byref(out)))
        return out.value

    def graph_capture_count(self):
        """captures of the decode graph so far: the first graph-mode step, and one for every re-capture (a position in another live-length bucket, another sampler setting)"""
        lib = load()
        lib.mila_gemma_graph_capture_count.argtypes = [C.c_void_p, C.c_void_p]
        out = C.c_int64()
        _check(lib.mila_gemma_graph_capture_count(self.h, C.byref(out)))
        return out.value

    def resident_staging_bytes(self):
        """bytes of op-owned prefill staging the layer Linears hold right now (fp8 policy: bf16 copies -- 0 while W8A8 is on; fp4 policy: e4m3 copies)"""
        lib = load()
        lib.mila_gemma_resident_staging_bytes.argtypes = [C.c_void_p, C.c_void_p]
        out = C.c_double()
        _check(lib.mila_gemma_resident_staging_bytes(self.h, C.byref(out)))
        return out.value

    def set_fp8_activation_prefill(self, on):
        """fp4 policy: W4A8 prefill on the fp8 matrix cores (default, the reference's default) or the exact-weight bf16 fallback.
        fp8 policy: the OPT-IN W8A8 prefill (the policy's e4m3 weights + per-channel scales on the fp8 matrix cores, per-token e4m3 activations, no bf16 copy of the
        weights; default off -- the reference's arithmetic for PerChannelFp8<> is W8A16)"""
        _check(load().mila_gemma_set_fp8_activation_prefill(self.h, int(bool(on))))

    def set_fused_prefill(self, on):
        """prefill with the fused glue kernels (default, when 1024 < D <= 8192) or one launch per reference op; same bits"""
        _check(load().mila_gemma_set_fused_prefill(self.h, int(bool(on))))

    def prefill(self, tokens, position_offset=0):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.vocab, dtype=np.float32)
        _check(load().mila_gemma_prefill(self.h, t.ctypes.data, t.size, position_offset, out.ctypes.data))
        return out

    def prefill_scored(self, tokens, targets, position_offset=0, first_row=0, argmax=True):
        """prefill() that also scores the chunk (GemmaTransformer::prefillScored): targets[r] = the token whose log-probability row r reports (one per row of the
        chunk, the last included; -1 = none: NaN).  Returns (logits of the last row as prefill() returns them, logprob [T - first_row], argmax, argmax_logprob) --
        the last two None without argmax.  The logits of the scored rows are never formed."""
        lib = load()
        lib.mila_gemma_prefill_scored.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.size != t.size:
            raise ValueError("prefill_scored: one target per token of the chunk")
        n = max(int(t.size) - int(first_row), 0)
        out = np.empty(self.vocab, dtype=np.float32)
        lp = np.empty(n, dtype=np.float32)
        am = np.empty(n, dtype=np.int32) if argmax else None
        alp = np.empty(n, dtype=np.float32) if argmax else None
        _check(lib.mila_gemma_prefill_scored(self.h, t.ctypes.data, t.size, int(position_offset), tg.ctypes.data, int(first_row), lp.ctypes.data,
                                             am.ctypes.data if argmax else None, alp.ctypes.data if argmax else None, out.ctypes.data))
        return out, lp, am, alp

    def time_score(self, T, reps=1, first_row=0):
        """device ms of one prefillScored() of T tokens with rows [first_row, T) scored (time_prefill's shape)"""
        lib = load()
        lib.mila_gemma_time_score.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        lib.mila_gemma_time_score_from.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        out = C.c_double()
        if first_row:
            _check(lib.mila_gemma_time_score_from(self.h, int(T), int(first_row), int(reps), C.byref(out)))
        else:
            _check(lib.mila_gemma_time_score(self.h, int(T), int(reps), C.byref(out)))
        return out.value

    def decode(self, token, position, mode="fused", logprobs=None):
        """one decode step; the logits.  logprobs = n (0 .. 20): the step is followed by the greedy sampler and the token log-probability launches (in graph mode
        they are the captured step's tail), and the call returns (logits, token, logprob, top_ids [n], top_logprobs [n]) -- the greedy token of these logits, its
        log-probability under the model's distribution and the n most probable tokens"""
        out = np.empty(self.vocab, dtype=np.float32)
        if logprobs is not None:
            lib = load()
            lib.mila_gemma_decode_logprobs.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 5
            n = _logprobs_n(logprobs)
            tok, lp, ids, tlp = C.c_int32(), C.c_float(), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
            _check(lib.mila_gemma_decode_logprobs(self.h, int(token), int(position), self.MODES[mode], n, out.ctypes.data, C.addressof(tok), C.addressof(lp),
                                                  ids.ctypes.data, tlp.ctypes.data))
            return out, tok.value, np.float32(lp.value), ids, tlp
        _check(load().mila_gemma_decode(self.h, int(token), int(position), self.MODES[mode], out.ctypes.data))
        return out

    def set_step_logprobs(self, n=None):
        """token log-probabilities (top n, 0 .. 20) in every step that follows -- the timing loops time_decode / time_decode_rows / time_decode_chain among them;
        None turns them off.  (decode / decode_rows / decode_chain set them per call from their logprobs argument.)"""
        lib = load()
        lib.mila_gemma_set_step_logprobs.argtypes = [C.c_void_p, C.c_int]
        _check(lib.mila_gemma_set_step_logprobs(self.h, -1 if n is None else _logprobs_n(n)))

    def set_sampling_filters(self, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
        """the sampling filters of the step-level calls that follow (GemmaTransformer::setSamplingFilters for the greedy samplers; the stochastic ones get them with
        their parameters): decode_rows, the timing loops, generate / generate_sampled without filter keywords.  No arguments = neutral.  Penalties act on the token
        table of set_token_table()."""
        lib = load()
        lib.mila_gemma_set_sampling_filters.argtypes = [C.c_void_p, C.c_void_p]
        f = (C.c_float * 4)(*_filters(min_p, repetition_penalty, presence_penalty, frequency_penalty))
        _check(lib.mila_gemma_set_sampling_filters(self.h, f))

    def set_token_table(self, row, prompt):
        """a new request on row `row` (0: the one-sequence interface): counts to zero, the prompt tokens' flags set"""
        lib = load()
        lib.mila_gemma_set_token_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        ids = np.ascontiguousarray(prompt, dtype=np.int32)
        _check(lib.mila_gemma_set_token_table(self.h, int(row), ids.ctypes.data if ids.size else None, ids.size))

    def token_table(self, row=0):
        """row `row`'s table words (uint32 [vocab]): bit 31 = in the prompt, bits 0 .. 30 = times generated"""
        lib = load()
        lib.mila_gemma_read_token_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        out = np.zeros(self.vocab, dtype=np.uint32)
        _check(lib.mila_gemma_read_token_table(self.h, int(row), out.ctypes.data))
        return out

    def set_token_bias(self, bias=None, fill=0.0, update=False):
        """the bias table of every sampler of the step-level calls that follow (GemmaTransformer::setTokenBias; include/mila_cdna4.h: logit bias): every value
        `fill` (finite or -inf), then bias[id] (finite or -inf) at each id of the dict / (id, value) list.  update=True changes the listed entries of a table that is
        on and leaves the rest.  bias=None turns the bias off.  Turning it on or off re-captures a graph once; changing the contents never does."""
        lib = load()
        lib.mila_gemma_set_token_bias.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        if bias is None:
            _check(lib.mila_gemma_set_token_bias(self.h, 0.0, None, None, -1, 1))
            return
        items = list(bias.items()) if hasattr(bias, "items") else list(bias)
        ids = _id_list([k for k, _ in items], "set_token_bias", self.vocab)
        if len(set(ids)) != len(ids):
            raise ValueError("set_token_bias: an id occurs twice")
        vals = [float(v) for _, v in items]
        for v in vals + [float(fill)]:
            if np.isnan(v) or v == float("inf"):
                raise ValueError("set_token_bias: a bias value must be finite or -inf (got %g)" % v)
        i32, f32 = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float32)
        _check(lib.mila_gemma_set_token_bias(self.h, float(fill), i32.ctypes.data if i32.size else None, f32.ctypes.data if f32.size else None, i32.size, 0 if update else 1))

    def token_bias(self):
        """-> (the bias table, float32 [vocab]; whether the bias is on)"""
        lib = load()
        lib.mila_gemma_read_token_bias.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        out, on = np.zeros(self.vocab, dtype=np.float32), C.c_int32()
        _check(lib.mila_gemma_read_token_bias(self.h, out.ctypes.data, C.byref(on)))
        return out, bool(on.value)

    def set_token_automaton(self, automaton):
        """the token automaton of every one-row sampler of the step-level calls that follow (GemmaTransformer::setTokenAutomaton; include/mila_cdna4.h: token
        automaton): validated, uploaded, turned on and reset to its start state.  None turns it off.  Turning it on or off re-captures a graph once; replacing one by
        another of the same size, or resetting it, never does."""
        lib = load()
        lib.mila_gemma_set_token_automaton.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int]
        if automaton is None:
            _check(lib.mila_gemma_set_token_automaton(self.h, None, 0, None, 0, 0, 0))
            return
        a = automaton
        _check(lib.mila_gemma_set_token_automaton(self.h, a.class_of.ctypes.data, a.vocab, a.next.ctypes.data, a.num_states, a.num_classes, a.start))

    def reset_token_automaton(self):
        """the state back to the automaton's start state, the effective table composed for it (GemmaTransformer::resetTokenAutomaton)"""
        lib = load()
        lib.mila_gemma_reset_token_automaton.argtypes = [C.c_void_p]
        _check(lib.mila_gemma_reset_token_automaton(self.h))

    def token_automaton_state(self, table=False):
        """-> the automaton's state word, read synchronously; table=True: (state, the effective table float32 [vocab])"""
        lib = load()
        lib.mila_gemma_token_automaton_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        st, on = C.c_int32(), C.c_int32()
        eff = np.zeros(self.vocab, dtype=np.float32) if table else None
        _check(lib.mila_gemma_token_automaton_state(self.h, C.byref(st), C.byref(on), eff.ctypes.data if table else None))
        return (int(st.value), eff) if table else int(st.value)

    def _with_filters(self, filters, fn):
        """fn() under the given filter keywords, neutral again afterwards; no keywords: whatever set_sampling_filters() left"""
        if not filters:
            return fn()
        self.set_sampling_filters(**filters)
        try:
            return fn()
        finally:
            self.set_sampling_filters()

    def generate(self, first_token, start_position, n_tokens, mode="graph", **penalties):
        """greedy autoregressive generation with the device sampler; returns the sampled token ids.  penalties: repetition_penalty, presence_penalty,
        frequency_penalty -- argmax of the adjusted logits, from and into the token table of set_token_table(0, prompt)"""
        if "min_p" in penalties:
            raise TypeError("Gemma.generate: min_p does not change a greedy request")
        out = np.empty(n_tokens, dtype=np.int32)
        self._with_filters(penalties, lambda: _check(load().mila_gemma_generate(self.h, int(first_token), int(start_position), int(n_tokens), self.MODES[mode], out.ctypes.data)))
        return out

    PIPELINES = {"search": 0, "radix": 1}

    def generate_sampled(self, first_token, start_position, n_tokens, temperature=1.0, top_k=0, top_p=1.0, seed=0, mode="fused", pipeline="search", **filters):
        """multinomial generation (softcap + temperature + top-k + top-p on the device, uniform draws from a host mt19937).  pipeline: "search" = sample_stochastic_*,
        "radix" = sample_radix_*; mode "graph" (radix only) runs the sampler as the tail of the captured step, its draws and tokens travelling through host-visible rings.
        filters (radix only): min_p, repetition_penalty, presence_penalty, frequency_penalty; the penalties read and update the token table of set_token_table(0, prompt)"""
        out = np.empty(n_tokens, dtype=np.int32)
        self._with_filters(filters, lambda: _check(load().mila_gemma_generate_sampled(self.h, int(first_token), int(start_position), int(n_tokens), self.MODES[mode],
                                                                                      self.PIPELINES[pipeline], float(temperature), int(top_k), float(top_p), int(seed), out.ctypes.data)))
        return out

    # ---- batched decode: rows of independent sequences (max_batch > 1) ----
    def prefill_row(self, b, tokens, offset=0):
        """prefill `tokens` at positions offset .. into row b's KV caches (the B = 1 prefill on the selected cache row); the last position's logits"""
        lib = load()
        lib.mila_gemma_prefill_row.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.vocab, dtype=np.float32)
        _check(lib.mila_gemma_prefill_row(self.h, int(b), t.ctypes.data, t.size, int(offset), out.ctypes.data))
        return out

    def set_active(self, b, active, token=None):
        """row b's active word (an inactive row keeps its token, its position and its caches through every step) and, when given, the token its next step embeds"""
        lib = load()
        lib.mila_gemma_set_active.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32]
        _check(lib.mila_gemma_set_active(self.h, int(b), int(bool(active)), -1 if token is None else int(token)))

    def reset_row(self, b):
        """forget row b: position 0, inactive"""
        lib = load()
        lib.mila_gemma_reset_row.argtypes = [C.c_void_p, C.c_int]
        _check(lib.mila_gemma_reset_row(self.h, int(b)))

    def rewind_row(self, b, position, written):
        """GemmaTransformer::rewindKvCacheRow: row b goes on from `position`, given that `written` positions were appended to it -> True; False when it is out of
        range or, on a bounded_local_kv_rows model, when the row's rings no longer hold what a continuation from `position` reads (nothing changed: prefill from 0)"""
        lib = load()
        lib.mila_gemma_rewind_row.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        ok = C.c_int(0)
        _check(lib.mila_gemma_rewind_row(self.h, int(b), int(position), int(written), C.byref(ok)))
        return bool(ok.value)

    def fork_row(self, src, dst_mask, length):
        """GemmaTransformer::forkRow: a shared prefill -- directly behind prefill_row(src, tokens of `length`), row src's cache prefix [0, length) of every layer, its
        logits and its position into the rows of dst_mask (bit r = row r)"""
        lib = load()
        lib.mila_gemma_fork_row.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int64, C.c_int]
        _check(lib.mila_gemma_fork_row(self.h, int(src), int(dst_mask), int(length), 1))

    def fork_row_prefix(self, src, dst_mask, length):
        """GemmaTransformer::forkRowPrefix: a shared prefix -- the caches only, [0, length) of every layer, from ANY row at a position >= length (it may have stepped)
        into the rows of dst_mask; no logits, no position: prefill_row(dst, suffix, offset=length) follows.  One launch for all layers."""
        lib = load()
        lib.mila_gemma_fork_row.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int64, C.c_int]
        _check(lib.mila_gemma_fork_row(self.h, int(src), int(dst_mask), int(length), 0))

    def decode_rows(self, B, max_position, mode="graph", greedy=True, sampling=None, draws=None, logprobs=None):
        """one step over rows 0 .. B - 1, eager ("fused") or as a graph replay; greedy: the step ends with the rows sampler tail.  max_position: the largest
        position among the active rows.  Returns (logits [B, vocab], tokens [B], positions [B]) as they stand AFTER the step.
        sampling = (temperature, top_k, top_p) with draws = B uniform draws (greedy is then ignored): the step ends with the radix sampler over the rows, row b
        sampling at draws[b] -- next token and position bump of every active row."""
        lib = load()
        lib.mila_gemma_decode_rows.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        logits, toks, pos = np.empty((B, self.vocab), dtype=np.float32), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32)
        if (sampling is None) != (draws is None):
            raise ValueError("Gemma.decode_rows: sampling and draws go together")
        if logprobs is not None:
            # ... additionally (logprob [B], top_ids [B, n], top_logprobs [B, n]) of the tokens the tail chose; an inactive row's entries are stale
            lib.mila_gemma_decode_rows_logprobs.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_int] + [C.c_void_p] * 6
            n = _logprobs_n(logprobs)
            d = None if draws is None else np.ascontiguousarray(draws, dtype=np.float32)
            if d is not None and d.size != B:
                raise ValueError("Gemma.decode_rows: one draw per row")
            t, k, p = (1.0, 0, 1.0) if sampling is None else sampling
            lp, ids, tlp = np.empty(B, dtype=np.float32), np.empty((B, n), dtype=np.int32), np.empty((B, n), dtype=np.float32)
            _check(lib.mila_gemma_decode_rows_logprobs(self.h, int(B), int(max_position), {"fused": 1, "graph": 2}[mode], int(bool(greedy)), float(t), int(k), float(p),
                                                       None if d is None else d.ctypes.data, n, logits.ctypes.data, toks.ctypes.data, pos.ctypes.data,
                                                       lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data))
            return logits, toks, pos, lp, ids, tlp
        if sampling is not None:
            lib.mila_gemma_decode_rows_sampled.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            d = np.ascontiguousarray(draws, dtype=np.float32)
            if d.size != B:
                raise ValueError("Gemma.decode_rows: one draw per row")
            t, k, p = sampling
            _check(lib.mila_gemma_decode_rows_sampled(self.h, int(B), int(max_position), {"fused": 1, "graph": 2}[mode], float(t), int(k), float(p), d.ctypes.data,
                                                      logits.ctypes.data, toks.ctypes.data, pos.ctypes.data))
            return logits, toks, pos
        _check(lib.mila_gemma_decode_rows(self.h, int(B), int(max_position), {"fused": 1, "graph": 2}[mode], int(bool(greedy)), logits.ctypes.data, toks.ctypes.data, pos.ctypes.data))
        return logits, toks, pos

    def set_rows_requests(self, requests=None, draws=None):
        """ROW REQUESTS for the rows steps that follow (GemmaTransformer::setRowsRequests; include/mila_cdna4.h: row requests): requests = one dict per row with any of
        temperature (<= 0: greedy; default 0), top_k, top_p, min_p, repetition_penalty, presence_penalty, frequency_penalty.  The parameters go into records in device
        memory: decode_rows / time_decode_rows then end in the requests tails whatever their greedy / sampling arguments say (decode_rows(sampling=(1, 0, 1),
        draws=...) still delivers one draw per row), and rows_graph_info()["captures"] moves only when a CLASS fact changes -- whether there are greedy rows,
        stochastic rows, a constrained row, a row with an automaton, a penalized row.  None clears the requests."""
        lib = load()
        lib.mila_gemma_set_rows_requests.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        if not requests:
            _check(lib.mila_gemma_set_rows_requests(self.h, None, 0, None))
            return
        rows = []
        for q in requests:
            unknown = set(q) - {"temperature", "top_k", "top_p", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty"}
            if unknown:
                raise ValueError("set_rows_requests: unknown keys %s" % sorted(unknown))
            rows.append([q.get("temperature", 0.0), q.get("top_k", 0), q.get("top_p", 1.0), q.get("min_p", 0.0), q.get("repetition_penalty", 1.0), q.get("presence_penalty", 0.0),
                         q.get("frequency_penalty", 0.0)])
        p = np.ascontiguousarray(rows, dtype=np.float32)
        d = None if draws is None else np.ascontiguousarray(draws, dtype=np.float32)
        if d is not None and d.size != len(rows):
            raise ValueError("set_rows_requests: one draw per row")
        _check(lib.mila_gemma_set_rows_requests(self.h, p.ctypes.data, len(rows), None if d is None else d.ctypes.data))

    def set_row_token_bias(self, row, bias=None, fill=0.0):
        """row `row`'s bias table for the requests samplers (set_token_bias's arguments, per row); None: no bias.  A row with an automaton: set the automaton first."""
        lib = load()
        lib.mila_gemma_set_row_token_bias.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int64]
        if bias is None:
            _check(lib.mila_gemma_set_row_token_bias(self.h, int(row), 0.0, None, None, -1))
            return
        items = list(bias.items()) if hasattr(bias, "items") else list(bias)
        ids = np.ascontiguousarray(_id_list([k for k, _ in items], "set_row_token_bias", self.vocab), dtype=np.int32)
        if len(set(ids.tolist())) != ids.size:
            raise ValueError("set_row_token_bias: an id occurs twice")
        vals = np.ascontiguousarray([v for _, v in items], dtype=np.float32)
        _check(lib.mila_gemma_set_row_token_bias(self.h, int(row), float(fill), ids.ctypes.data if ids.size else None, vals.ctypes.data if ids.size else None, int(ids.size)))

    def set_row_token_automaton(self, row, automaton):
        """row `row`'s automaton for the requests step (set_token_automaton's, per row): validated, uploaded, at its start state; None: the row has none"""
        lib = load()
        lib.mila_gemma_set_row_token_automaton.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int]
        if automaton is None:
            _check(lib.mila_gemma_set_row_token_automaton(self.h, int(row), None, 0, None, 0, 0, 0))
            return
        a = automaton
        _check(lib.mila_gemma_set_row_token_automaton(self.h, int(row), a.class_of.ctypes.data, a.vocab, a.next.ctypes.data, a.num_states, a.num_classes, a.start))

    def row_token_automaton_state(self, row, table=False):
        """-> row `row`'s automaton state (None: the row has no automaton), read synchronously; table=True: (state, the row's effective table float32 [vocab])"""
        lib = load()
        lib.mila_gemma_row_token_automaton_state.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        st, on = C.c_int32(), C.c_int32()
        eff = np.zeros(self.vocab, dtype=np.float32) if table else None
        _check(lib.mila_gemma_row_token_automaton_state(self.h, int(row), C.byref(st), C.byref(on), eff.ctypes.data if table else None))
        state = int(st.value) if on.value else None
        return (state, eff) if table else state

    def rows_graph_info(self):
        """{"captures": captures of the rows graph so far, "nodes": kernel nodes of the captured rows step}"""
        lib = load()
        lib.mila_gemma_rows_graph_info.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int64 * 2)()
        _check(lib.mila_gemma_rows_graph_info(self.h, out))
        return {"captures": out[0], "nodes": out[1]}

    def set_step_sampling(self, which, sampling=None, draws=None):
        """the sampler tail of the "rows" or the "chain" step for the timing loops that follow: sampling = (temperature, top_k, top_p) with one uniform draw per row;
        None clears it.  (decode_rows / decode_chain set it per call from their own arguments.)"""
        lib = load()
        lib.mila_gemma_set_step_sampling.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_int]
        if sampling is None:
            _check(lib.mila_gemma_set_step_sampling(self.h, {"rows": 0, "chain": 1}[which], 1.0, 0, 1.0, None, 0))
            return
        d = np.ascontiguousarray(draws, dtype=np.float32)
        t, k, p = sampling
        _check(lib.mila_gemma_set_step_sampling(self.h, {"rows": 0, "chain": 1}[which], float(t), int(k), float(p), d.ctypes.data, int(d.size)))

    def time_decode_rows(self, B, start_position, steps, warmup, greedy=True):
        """`steps` graph replays of a B-row step, every row active from start_position: the greedy step, or (greedy=False) the one that ends in the stochastic tail
        set_step_sampling("rows", ...) chose -- at the logits and the position bump when none is set"""
        lib = load()
        lib.mila_gemma_time_decode_rows.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        lib.mila_gemma_time_decode_rows_stochastic.argtypes = lib.mila_gemma_time_decode_rows.argtypes
        out = (C.c_double * 2)()
        if not greedy:
            _check(lib.mila_gemma_time_decode_rows_stochastic(self.h, int(B), int(start_position), int(steps), int(warmup), out))
            return {"wall_ms_per_step": out[0], "device_ms_per_step": out[1]}
        _check(lib.mila_gemma_time_decode_rows(self.h, int(B), int(start_position), int(steps), int(warmup), out))
        return {"wall_ms_per_step": out[0], "device_ms_per_step": out[1]}

    # ---- chain decode: consecutive positions of one sequence (draft_tokens > 0) ----
    def decode_chain(self, tokens, position, mode="graph", sampling=None, draws=None, logprobs=None):
        """one chain step: tokens[0] is decoded at `position`, tokens[1:] are drafts for the positions behind it (2 <= len(tokens) <= draft_tokens + 1), eager
        ("fused") or as a graph replay.  Returns (logits [T, vocab], count, accepted tokens [count], new position): the longest correct draft prefix is accepted,
        so accepted[i] is the greedy token after tokens[:i + 1] and the position advances by count.
        sampling = (temperature, top_k, top_p) with draws = T uniform draws: the drafts are verified against SAMPLES -- accepted[i] is the radix sampler's token from
        row i's logits at draws[i], and a draft is accepted exactly when it equals that sample."""
        lib = load()
        lib.mila_gemma_chain_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        T = int(t.size)
        logits, out = np.empty((T, self.vocab), dtype=np.float32), np.zeros(T + 2, dtype=np.int32)
        if (sampling is None) != (draws is None):
            raise ValueError("Gemma.decode_chain: sampling and draws go together")
        if logprobs is not None:
            # ... additionally (logprob [count], top_ids [count, n], top_logprobs [count, n]) of the accepted tokens
            lib.mila_gemma_chain_decode_logprobs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_int] + [C.c_void_p] * 5
            n = _logprobs_n(logprobs)
            d = None if draws is None else np.ascontiguousarray(draws, dtype=np.float32)
            if d is not None and d.size != T:
                raise ValueError("Gemma.decode_chain: one draw per row")
            tt, k, p = (1.0, 0, 1.0) if sampling is None else sampling
            lp, ids, tlp = np.empty(T, dtype=np.float32), np.empty((T, n), dtype=np.int32), np.empty((T, n), dtype=np.float32)
            _check(lib.mila_gemma_chain_decode_logprobs(self.h, t.ctypes.data, T, int(position), {"fused": 1, "graph": 2}[mode], float(tt), int(k), float(p),
                                                        None if d is None else d.ctypes.data, n, logits.ctypes.data, out.ctypes.data, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data))
            count = int(out[0])
            return logits, count, out[1:1 + count].tolist(), int(out[T + 1]), lp[:count], ids[:count], tlp[:count]
        if sampling is not None:
            lib.mila_gemma_chain_decode_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
            d = np.ascontiguousarray(draws, dtype=np.float32)
            if d.size != T:
                raise ValueError("Gemma.decode_chain: one draw per row")
            tt, k, p = sampling
            _check(lib.mila_gemma_chain_decode_sampled(self.h, t.ctypes.data, T, int(position), {"fused": 1, "graph": 2}[mode], float(tt), int(k), float(p), d.ctypes.data,
                                                       logits.ctypes.data, out.ctypes.data))
            count = int(out[0])
            return logits, count, out[1:1 + count].tolist(), int(out[T + 1])
        _check(lib.mila_gemma_chain_decode(self.h, t.ctypes.data, T, int(position), {"fused": 1, "graph": 2}[mode], logits.ctypes.data, out.ctypes.data))
        count = int(out[0])
        return logits, count, out[1:1 + count].tolist(), int(out[T + 1])

    def chain_graph_info(self):
        """{"captures": captures of the chain graph so far, "nodes": kernel nodes of the captured chain step, "rows": its row count}"""
        lib = load()
        lib.mila_gemma_chain_graph_info.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int64 * 3)()
        _check(lib.mila_gemma_chain_graph_info(self.h, out))
        return {"captures": out[0], "nodes": out[1], "rows": out[2]}

    def time_decode_chain(self, T, start_position, steps, warmup):      # (the tail follows set_step_sampling("chain", ...))
        """`steps` graph replays of a T-row chain step from start_position (every step advances by what it accepts)"""
        lib = load()
        lib.mila_gemma_time_chain_decode.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        out = (C.c_double * 2)()
        _check(lib.mila_gemma_time_chain_decode(self.h, int(T), int(start_position), int(steps), int(warmup), out))
        return {"wall_ms_per_step": out[0], "device_ms_per_step": out[1]}

    def time_decode(self, start_position, steps, warmup, mode="graph"):
        out = (C.c_double * 2)()
        _check(load().mila_gemma_time_decode(self.h, start_position, steps, warmup, self.MODES[mode], out))
        return {"wall_ms_per_step": out[0], "device_ms_per_step": out[1]}

    def time_dominant_kernel(self, rounds=3):
        out = (C.c_double * 2)()
        _check(load().mila_gemma_time_dominant_kernel(self.h, rounds, out))
        return {"avg_us": out[0], "bytes": out[1]}

    def time_prefill(self, T, reps=1):
        out = C.c_double()
        _check(load().mila_gemma_time_prefill(self.h, T, reps, C.byref(out)))
        return out.value

    def time_prefill_chunked(self, total_T):
        """device ms of a total_T-token prompt prefilled from an empty cache in chunks of the built prefill size (GemmaTransformer::prefillFrom); the caches
        hold total_T positions afterwards"""
        lib = load()
        lib.mila_gemma_time_prefill_chunked.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        out = C.c_double()
        _check(lib.mila_gemma_time_prefill_chunked(self.h, int(total_T), C.byref(out)))
        return out.value

    def component_names(self):
        """names of the model's components in construction order (each block, its children, temb, rmsn_final, lm_head)"""
        lib = load()
        lib.mila_gemma_component_names.restype = C.c_int64
        lib.mila_gemma_component_names.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        need = lib.mila_gemma_component_names(self.h, None, 0)
        if need < 0:
            raise RuntimeError(lib.mila_host_last_error().decode())
        buf = C.create_string_buffer(need)
        lib.mila_gemma_component_names(self.h, buf, need)
        return buf.value.decode().split("\n")[:-1]

    def info(self, context):
        out = (C.c_double * 4)()
        _check(load().mila_gemma_info(self.h, context, out))
        return {"decode_bytes_per_token": out[0], "weight_bytes": out[1], "linear_params": out[2], "table_params": out[3]}


def validate_gemma_config(config=None, max_batch=1, draft_tokens=0, kv_fp8=False, kv_fp8_rows=False, bounded_local_kv_rows=False):
    """GemmaConfig::validate() on the configuration Gemma(..., max_batch=, draft_tokens=, kv_fp8_rows=, bounded_local_kv_rows=) would build, without a device: raises
    ValueError with its message"""
    lib = load()
    lib.mila_gemma_validate_config.argtypes = [C.POINTER(GemmaConfigC), C.c_int64, C.c_int64]
    lib.mila_gemma_validate_config_kv.argtypes = [C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int]
    cfg = dict(GEMMA4_12B if config is None else config)
    cfg.setdefault("bounded_local_kv", 0)
    cfg.setdefault("kv_fp8", 0)
    if kv_fp8:
        cfg["kv_fp8"] = 1
    c = GemmaConfigC(**cfg)
    if bounded_local_kv_rows:
        lib.mila_gemma_validate_config_ring.argtypes = [C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int, C.c_int]
        _check(lib.mila_gemma_validate_config_ring(C.byref(c), int(max_batch), int(draft_tokens), int(bool(kv_fp8_rows)), 1))
        return
    if kv_fp8_rows:
        _check(lib.mila_gemma_validate_config_kv(C.byref(c), int(max_batch), int(draft_tokens), 1))
        return
    _check(lib.mila_gemma_validate_config(C.byref(c), int(max_batch), int(draft_tokens)))


def prompt_lookup_draft(history, k):
    """the default drafter of the speculative generate() (promptLookupDraft): for n = 3, 2, 1 the latest earlier occurrence of the last n tokens of `history`
    decides, and the up-to-k tokens that followed it are proposed; no occurrence proposes nothing.  Pure host code."""
    lib = load()
    lib.mila_gemma_prompt_lookup_draft.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    h = np.ascontiguousarray(history, dtype=np.int32)
    out = np.zeros(max(int(k), 1), dtype=np.int32)
    n = lib.mila_gemma_prompt_lookup_draft(h.ctypes.data if h.size else None, int(h.size), int(k), out.ctypes.data)
    return out[:n].tolist()


GENERATE_STATUS = {0: "stop", 1: "length", 2: "context_limit", 3: "cancelled"}      # GenerateStatus / to_string (Core/GenerateStatus.ixx)


class GemmaModel:
    """GemmaModel<Rocm, BF16> (Models/GemmaModel.ixx): fromPretrained / fromSynthetic, then generate()."""

    def __init__(self, handle, device):
        self.h, self.device = handle, device

    @staticmethod
    def _bind():
        lib = load()
        lib.mila_gemma_model_from_pretrained.restype = C.c_void_p
        lib.mila_gemma_model_from_pretrained.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]
        lib.mila_gemma_model_from_pretrained_kv.restype = C.c_void_p
        lib.mila_gemma_model_from_pretrained_kv.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int]
        lib.mila_gemma_model_synthetic.restype = C.c_void_p
        lib.mila_gemma_model_synthetic.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_int]
        lib.mila_gemma_model_destroy.argtypes = [C.c_void_p]
        lib.mila_gemma_model_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64,
                                                  C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        return lib

    @staticmethod
    def _raise(lib, what):
        text = lib.mila_host_last_error().decode()
        raise (ValueError if text.startswith("invalid_argument") else RuntimeError)(what + ": " + text)

    @classmethod
    def from_pretrained(cls, path, policy="bf16", context=4096, prefill_chunk=0, bounded_local_kv=False, device=0, kv_fp8=False):
        """GemmaModel::fromPretrained(path, GemmaModelConfig(context).withWeightQuantization(policy)): the geometry comes from the artifact"""
        lib = cls._bind()
        h = lib.mila_gemma_model_from_pretrained_kv(str(path).encode(), POLICIES[policy], context, prefill_chunk, int(bool(bounded_local_kv)), int(bool(kv_fp8)), device)
        if not h:
            cls._raise(lib, "GemmaModel.from_pretrained")
        return cls(h, device)

    @classmethod
    def synthetic(cls, policy="bf16", config=None, context=4096, prefill_chunk=0, seed=1234, profile=None, device=0, kv_fp8=False, max_batch=None, draft_tokens=None,
                  kv_fp8_rows=False, bounded_local_kv_rows=False):
        """kv_fp8_rows: GemmaModelConfig::withKvFp8Rows -- the FP8 KV cache (implied) on a model of max_batch 1 .. 4 (generate_batch / generate_requests / serve_requests
        over FP8 rows); plain kv_fp8 with max_batch > 1 stays refused
        bounded_local_kv_rows: GemmaModelConfig::withBoundedLocalKvRows -- rings (bounded_local_kv, implied) on the sliding-window layers of a model of max_batch 1 .. 4:
        the same calls over rows that keep window + prefill_chunk - 1 positions per sliding-window layer; plain bounded_local_kv with max_batch > 1 stays refused"""
        lib = cls._bind()
        cfg = dict(GEMMA4_12B if config is None else config)
        cfg.setdefault("bounded_local_kv", 0)
        cfg.setdefault("kv_fp8", 0)
        if kv_fp8:
            cfg["kv_fp8"] = 1
        c = GemmaConfigC(**cfg)
        p = None
        if profile is not None:
            p = (C.c_float * 5)(*[float(profile[k]) for k in ("linear_gain", "qk_norm_center", "post_norm_center", "layer_scalar", "table_gain")])
        if bounded_local_kv_rows:
            if kv_fp8_rows or cfg["kv_fp8"]:
                raise ValueError("GemmaModel.synthetic: bounded_local_kv_rows cannot be combined with kv_fp8 / kv_fp8_rows")
            if draft_tokens:
                raise ValueError("GemmaModel.synthetic: draft_tokens cannot be combined with bounded_local_kv_rows")
            lib.mila_gemma_model_synthetic_rows_ring.restype = C.c_void_p
            lib.mila_gemma_model_synthetic_rows_ring.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_void_p, C.c_int]
            h = lib.mila_gemma_model_synthetic_rows_ring(POLICIES[policy], C.byref(c), context, prefill_chunk, 1 if max_batch is None else int(max_batch), 1, seed, p, device)
        elif kv_fp8_rows:
            if draft_tokens:
                raise ValueError("GemmaModel.synthetic: draft_tokens cannot be combined with kv_fp8_rows")
            lib.mila_gemma_model_synthetic_rows_kv.restype = C.c_void_p
            lib.mila_gemma_model_synthetic_rows_kv.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_uint64, C.c_void_p, C.c_int]
            h = lib.mila_gemma_model_synthetic_rows_kv(POLICIES[policy], C.byref(c), context, prefill_chunk, 1 if max_batch is None else int(max_batch), 1, seed, p, device)
        elif draft_tokens is not None:      # GemmaModelConfig::withDraftTokens: greedy generate() verifies up to draft_tokens drafted tokens per step
            if max_batch is not None:
                raise ValueError("GemmaModel.synthetic: draft_tokens cannot be combined with max_batch")
            lib.mila_gemma_model_synthetic_chain.restype = C.c_void_p
            lib.mila_gemma_model_synthetic_chain.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_int]
            h = lib.mila_gemma_model_synthetic_chain(POLICIES[policy], C.byref(c), context, prefill_chunk, int(draft_tokens), seed, p, device)
        elif max_batch is None:
            h = lib.mila_gemma_model_synthetic(POLICIES[policy], C.byref(c), context, prefill_chunk, seed, p, device)
        else:      # GemmaModelConfig::withMaxBatch: a model generate_batch() can run on
            lib.mila_gemma_model_synthetic_rows.restype = C.c_void_p
            lib.mila_gemma_model_synthetic_rows.argtypes = [C.c_int, C.POINTER(GemmaConfigC), C.c_int64, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_int]
            h = lib.mila_gemma_model_synthetic_rows(POLICIES[policy], C.byref(c), context, prefill_chunk, int(max_batch), seed, p, device)
        if not h:
            cls._raise(lib, "GemmaModel.synthetic")
        return cls(h, device)

    def score(self, tokens, first=1, argmax=False):
        """GemmaModel::score: the log-probability of every token first .. n - 1 given the tokens before it, from the prefill (chunked by the model's prefill chunk,
        with KV prefix reuse up to first - 1).  Returns a dict: logprob [n - first] float32, sum (float64, summed on the host), reused_prefix, and with argmax the
        greedy token of every scored position and its log-probability (argmax, argmax_logprob).  ValueError for what the model refuses before anything is enqueued."""
        lib = load()
        lib.mila_gemma_model_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        n = max(int(t.size) - int(first), 0) if int(first) >= 1 else 0
        lp = np.empty(n, dtype=np.float32)
        am = np.empty(n, dtype=np.int32) if argmax else None
        alp = np.empty(n, dtype=np.float32) if argmax else None
        total, reused = C.c_double(), C.c_int64()
        if lib.mila_gemma_model_score(self.h, t.ctypes.data, t.size, int(first), lp.ctypes.data, am.ctypes.data if argmax else None, alp.ctypes.data if argmax else None,
                                      C.byref(total), C.byref(reused)) != 0:
            self._raise(lib, "GemmaModel.score")
        out = {"logprob": lp, "sum": total.value, "reused_prefix": int(reused.value)}
        if argmax:
            out["argmax"], out["argmax_logprob"] = am, alp
        return out

    def generate(self, prompt, max_new_tokens=None, stop_tokens=(), temperature=1.0, top_k=1, top_p=1.0, seed=None, cancel_after=None, draft_hint=None,
                 speculative_sampling=False, logprobs=None, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None,
                 banned_tokens=(), allowed_tokens=(), min_tokens=0, automaton=None, speculate_constrained=False):
        """_generate() with the sampling filters (GenerateParams::sampling.min_p / .repetition_penalty / .presence_penalty / .frequency_penalty): the penalties read a
        token table on the device that starts from the whole prompt and counts every generated token; greedy with a penalty = argmax of the adjusted logits; a request
        with any filter set takes the plain loop on a draft_tokens model too.  Log-probabilities are those of the unpenalized logits.  With every filter neutral this
        is _generate(), entry for entry.
        logit_bias ({id: finite value}), banned_tokens, allowed_tokens (a closed answer set; a ban wins) and min_tokens (no stop token among the first min_tokens
        samples) are GenerateParams' fields of those names: one bias table on the device, added to the capped logit by every sampler of the request; a request with
        any of them takes the plain loop on a draft_tokens model (unless speculate_constrained is set, below).  Log-probabilities stay those of the unbiased logits.
        automaton (a TokenAutomaton; GenerateParams::automaton): grammar-constrained decoding -- the state advances on the device with every sampled token and the
        samplers see -inf wherever the state forbids a token.  Refused (ValueError, before anything runs): a reachable state with no token that has both a transition
        and a finite bias, and min_tokens > 0 beside an automaton.  The return value gains a last element: the state the request ended in (the state after its last
        sample, a stop token included).
        speculate_constrained (GenerateParams::speculate_constrained; a draft_tokens model, greedy or speculative_sampling, no penalties / min-p): a request with a bias
        and / or an automaton takes the speculative loop -- the tokens its automaton forces are drafted for free, the rest by draft_hint / the prompt lookup.  Tokens,
        finish reason, final state and generator state are the plain loop's; speculation_stats_forced() reports the forced tokens.  Not with cancel_after."""
        f = _filters(min_p, repetition_penalty, presence_penalty, frequency_penalty)
        bias = _bias_request(logit_bias, banned_tokens, allowed_tokens, min_tokens, stop_tokens, max_new_tokens, self.vocab_size())
        if automaton is not None and not isinstance(automaton, TokenAutomaton):
            raise ValueError("GemmaModel.generate: automaton must be a host.TokenAutomaton")
        if f == _filters() and bias is None and automaton is None:
            return self._generate(prompt, max_new_tokens, stop_tokens, temperature, top_k, top_p, seed, cancel_after, draft_hint, speculative_sampling, logprobs)
        lib = load()
        pr = np.ascontiguousarray(prompt, dtype=np.int32)
        st = np.ascontiguousarray(list(stop_tokens), dtype=np.int32)
        cap = int(max_new_tokens) if max_new_tokens is not None else 1 << 16
        out = np.zeros(max(cap, 1), dtype=np.int32)
        n, status, reused, n_lp = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
        top_n = -1 if logprobs is None else _logprobs_n(logprobs)
        width = max(top_n, 1)
        lp, ids, tlp = np.zeros(len(out), dtype=np.float32), np.zeros((len(out), width), dtype=np.int32), np.zeros((len(out), width), dtype=np.float32)
        fl = (C.c_float * 4)(*f)
        head = [self.h, pr.ctypes.data, len(pr), -1 if max_new_tokens is None else int(max_new_tokens), st.ctypes.data if len(st) else None, len(st), float(temperature),
                int(top_k), float(top_p), -1 if seed is None else int(seed)]
        head_types = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64]
        tail = [top_n, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data, C.byref(n_lp), fl, None if bias is None else C.byref(bias[0])]
        tail_types = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        spec_entry, plain_entry = lib.mila_gemma_model_generate_spec_biased, lib.mila_gemma_model_generate_biased
        if automaton is not None:      # the entries with the automaton request behind the bias request
            areq = automaton._request()
            tail, tail_types = tail + [C.byref(areq)], tail_types + [C.c_void_p]
            spec_entry, plain_entry = lib.mila_gemma_model_generate_spec_automaton, lib.mila_gemma_model_generate_automaton
        if speculate_constrained:      # the entry with the flag behind the automaton request (None: none)
            if automaton is None:
                tail, tail_types = tail + [None], tail_types + [C.c_void_p]
            tail, tail_types = tail + [1], tail_types + [C.c_int]
            spec_entry = lib.mila_gemma_model_generate_spec_constrained
        if speculative_sampling or draft_hint is not None or speculate_constrained:
            if cancel_after is not None:
                raise ValueError("GemmaModel.generate: draft_hint / speculative_sampling / speculate_constrained cannot be combined with cancel_after")
            hint = np.ascontiguousarray([] if draft_hint is None else draft_hint, dtype=np.int32)
            stats = (C.c_int64 * 4)()
            spec_entry.argtypes = head_types + [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + tail_types
            _check(spec_entry(*head, hint.ctypes.data if hint.size else None, int(hint.size), int(bool(speculative_sampling)), out.ctypes.data,
                                                               len(out), C.byref(n), C.byref(status), stats, *tail))
        else:
            plain_entry.argtypes = head_types + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + tail_types
            _check(plain_entry(*head, out.ctypes.data, len(out), C.byref(n), C.byref(status), C.byref(reused),
                                                          -1 if cancel_after is None else int(cancel_after), *tail))
        res = (out[:min(n.value, len(out))].tolist(), GENERATE_STATUS[status.value], reused.value)
        if logprobs is not None:
            res = res + ([(np.float32(lp[i]), ids[i, :top_n].copy(), tlp[i, :top_n].copy()) for i in range(min(n_lp.value, len(out)))],)
        return res if automaton is None else res + (self.last_automaton_state(),)

    def last_automaton_state(self):
        """GemmaModel::lastAutomatonState(): the automaton state the last generate() ended in, None when that request had no automaton"""
        lib = load()
        lib.mila_gemma_model_last_automaton_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        st, has = C.c_int32(), C.c_int32()
        _check(lib.mila_gemma_model_last_automaton_state(self.h, C.byref(st), C.byref(has)))
        return int(st.value) if has.value else None

    def _generate(self, prompt, max_new_tokens=None, stop_tokens=(), temperature=1.0, top_k=1, top_p=1.0, seed=None, cancel_after=None, draft_hint=None,
                  speculative_sampling=False, logprobs=None):
        """-> (tokens passed to on_token, finish reason as GenerateStatus's to_string, prompt tokens served from the KV caches).
        logprobs = n (0 .. 20; GenerateParams::logprobs): a fourth element, a list of (logprob, top_ids [n], top_logprobs [n]) per emitted token -- its
        log-probability under the model's distribution (no temperature, no truncation) and the n most probable tokens, computed on the device inside the step.
        top_k = 1 is greedy (SamplingParams); seed reseeds the host RNG that draws the sampler's uniform; cancel_after = n raises the client's stop request
        from inside on_token once n tokens were delivered.
        draft_hint (tests and tools; a draft_tokens model): the tokens expected to follow the prompt -- the drafter of the speculative loop reads its proposals from
        there in place of the prompt lookup; the output is the plain greedy output whatever the hint holds.  speculation_stats() tells what the loop did.
        speculative_sampling (GenerateParams::speculative_sampling; a draft_tokens model): a stochastic request takes the speculative loop too, each draft
        verified against the sample the plain loop would take at that token -- the output is the plain stochastic output for the same seed."""
        lib = load()
        pr = np.ascontiguousarray(prompt, dtype=np.int32)
        st = np.ascontiguousarray(list(stop_tokens), dtype=np.int32)
        cap = int(max_new_tokens) if max_new_tokens is not None else 1 << 16
        out = np.zeros(max(cap, 1), dtype=np.int32)
        n, status, reused = C.c_int64(), C.c_int32(), C.c_int64()
        if logprobs is not None:
            # GenerateParams::logprobs: the return tuple gains a list of (logprob, top_ids, top_logprobs), one entry per emitted token
            top_n = _logprobs_n(logprobs)
            lp, ids, tlp = np.zeros(len(out), dtype=np.float32), np.zeros((len(out), top_n), dtype=np.int32), np.zeros((len(out), top_n), dtype=np.float32)
            n_lp = C.c_int64()
            tail = [top_n, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data, C.byref(n_lp)]
            tail_types = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            head = [self.h, pr.ctypes.data, len(pr), -1 if max_new_tokens is None else int(max_new_tokens), st.ctypes.data if len(st) else None, len(st), float(temperature),
                    int(top_k), float(top_p), -1 if seed is None else int(seed)]
            head_types = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64]
            if speculative_sampling or draft_hint is not None:
                if cancel_after is not None:
                    raise ValueError("GemmaModel.generate: draft_hint / speculative_sampling cannot be combined with cancel_after")
                hint = np.ascontiguousarray([] if draft_hint is None else draft_hint, dtype=np.int32)
                stats = (C.c_int64 * 4)()
                lib.mila_gemma_model_generate_spec_logprobs.argtypes = head_types + [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + tail_types
                _check(lib.mila_gemma_model_generate_spec_logprobs(*head, hint.ctypes.data if hint.size else None, int(hint.size), int(bool(speculative_sampling)), out.ctypes.data,
                                                                   len(out), C.byref(n), C.byref(status), stats, *tail))
            else:
                lib.mila_gemma_model_generate_logprobs.argtypes = head_types + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + tail_types
                _check(lib.mila_gemma_model_generate_logprobs(*head, out.ctypes.data, len(out), C.byref(n), C.byref(status), C.byref(reused),
                                                              -1 if cancel_after is None else int(cancel_after), *tail))
            entries = [(np.float32(lp[i]), ids[i].copy(), tlp[i].copy()) for i in range(min(n_lp.value, len(out)))]
            return out[:min(n.value, len(out))].tolist(), GENERATE_STATUS[status.value], reused.value, entries
        if speculative_sampling:
            if cancel_after is not None:
                raise ValueError("GemmaModel.generate: speculative_sampling cannot be combined with cancel_after")
            lib.mila_gemma_model_generate_spec_sampling.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64,
                                                                    C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            hint = np.ascontiguousarray([] if draft_hint is None else draft_hint, dtype=np.int32)
            stats = (C.c_int64 * 4)()
            _check(lib.mila_gemma_model_generate_spec_sampling(self.h, pr.ctypes.data, len(pr), -1 if max_new_tokens is None else int(max_new_tokens),
                                                               st.ctypes.data if len(st) else None, len(st), float(temperature), int(top_k), float(top_p),
                                                               -1 if seed is None else int(seed), hint.ctypes.data if hint.size else None, int(hint.size), 1,
                                                               out.ctypes.data, len(out), C.byref(n), C.byref(status), stats))
            return out[:min(n.value, len(out))].tolist(), GENERATE_STATUS[status.value], 0
        if draft_hint is not None:
            if cancel_after is not None:
                raise ValueError("GemmaModel.generate: draft_hint cannot be combined with cancel_after")
            lib.mila_gemma_model_generate_spec.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int64, C.c_void_p, C.c_int64,
                                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            hint = np.ascontiguousarray(draft_hint, dtype=np.int32)
            stats = (C.c_int64 * 4)()
            _check(lib.mila_gemma_model_generate_spec(self.h, pr.ctypes.data, len(pr), -1 if max_new_tokens is None else int(max_new_tokens), st.ctypes.data if len(st) else None, len(st),
                                                      float(temperature), int(top_k), float(top_p), -1 if seed is None else int(seed), hint.ctypes.data if hint.size else None,
                                                      int(hint.size), out.ctypes.data, len(out), C.byref(n), C.byref(status), stats))
            return out[:min(n.value, len(out))].tolist(), GENERATE_STATUS[status.value], 0
        _check(lib.mila_gemma_model_generate(self.h, pr.ctypes.data, len(pr), -1 if max_new_tokens is None else int(max_new_tokens), st.ctypes.data if len(st) else None, len(st),
                                             float(temperature), int(top_k), float(top_p), -1 if seed is None else int(seed), out.ctypes.data, len(out), C.byref(n), C.byref(status),
                                             C.byref(reused), -1 if cancel_after is None else int(cancel_after)))
        return out[:min(n.value, len(out))].tolist(), GENERATE_STATUS[status.value], reused.value

    def vocab_size(self):
        lib = load()
        lib.mila_gemma_model_vocab_size.restype = C.c_int64
        lib.mila_gemma_model_vocab_size.argtypes = [C.c_void_p]
        return int(lib.mila_gemma_model_vocab_size(self.h))

    def speculation_stats(self):
        """GemmaModel::lastSpeculation() of the last generate(): {"steps", "chain_steps", "drafted", "accepted"} -- decode steps in all, those that were chain
        steps, the drafter's tokens those carried (padding not counted) and how many of them were accepted"""
        lib = load()
        lib.mila_gemma_model_speculation_stats.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int64 * 4)()
        _check(lib.mila_gemma_model_speculation_stats(self.h, out))
        return dict(zip(("steps", "chain_steps", "drafted", "accepted"), [int(v) for v in out]))

    def speculation_stats_forced(self):
        """speculation_stats() plus "forced" and "forced_accepted": the drafted tokens that the automaton forced (generate(speculate_constrained=True)) and how many
        of those were accepted"""
        lib = load()
        lib.mila_gemma_model_speculation_stats_forced.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int64 * 6)()
        _check(lib.mila_gemma_model_speculation_stats_forced(self.h, out))
        return dict(zip(("steps", "chain_steps", "drafted", "accepted", "forced", "forced_accepted"), [int(v) for v in out]))

    def generate_batch(self, prompts, max_new_tokens=None, stop_tokens=(), temperature=1.0, top_k=1, top_p=1.0, seed=0, logprobs=None, min_p=0.0, repetition_penalty=1.0,
                       presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, banned_tokens=(), allowed_tokens=(), min_tokens=0, automaton=None):
        """_generate_batch() with the sampling filters of generate(), shared by the rows; every row has its own token table.  logit_bias / banned_tokens /
        allowed_tokens / min_tokens as in generate(): one bias table shared by the rows, which step in lockstep.  automaton: refused (GemmaModel::generateBatch)."""
        if automaton is not None:
            raise ValueError("GemmaModel.generate_batch: automaton is not built: one state per row in generateBatch")
        f = _filters(min_p, repetition_penalty, presence_penalty, frequency_penalty)
        bias = _bias_request(logit_bias, banned_tokens, allowed_tokens, min_tokens, stop_tokens, max_new_tokens, self.vocab_size())
        if f == _filters() and bias is None:
            return self._generate_batch(prompts, max_new_tokens, stop_tokens, temperature, top_k, top_p, seed, logprobs)
        lib = load()
        lib.mila_gemma_model_generate_rows_biased.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64,
                                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                              C.c_void_p]
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if len(prompts) else np.zeros(0), dtype=np.int32)
        offs = np.ascontiguousarray(np.cumsum([0] + [len(p) for p in prompts]), dtype=np.int64)
        st = np.ascontiguousarray(list(stop_tokens), dtype=np.int32)
        cap = int(max_new_tokens) if max_new_tokens is not None else 1 << 16
        out = np.zeros((max(len(prompts), 1), max(cap, 1)), dtype=np.int32)
        counts, status, lp_counts = (np.zeros(max(len(prompts), 1), dtype=t) for t in (np.int64, np.int32, np.int64))
        top_n = -1 if logprobs is None else _logprobs_n(logprobs)
        width = max(top_n, 1)
        lp, ids, tlp = np.zeros(out.shape, dtype=np.float32), np.zeros(out.shape + (width,), dtype=np.int32), np.zeros(out.shape + (width,), dtype=np.float32)
        fl = (C.c_float * 4)(*f)
        _check(lib.mila_gemma_model_generate_rows_biased(self.h, flat.ctypes.data, offs.ctypes.data, len(prompts), -1 if max_new_tokens is None else int(max_new_tokens),
                                                           st.ctypes.data if len(st) else None, len(st), float(temperature), int(top_k), float(top_p), int(seed), out.ctypes.data,
                                                           out.shape[1], counts.ctypes.data, status.ctypes.data, top_n, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data,
                                                           lp_counts.ctypes.data, fl, None if bias is None else C.byref(bias[0])))
        rows = [(out[b, :min(int(counts[b]), out.shape[1])].tolist(), GENERATE_STATUS[int(status[b])]) for b in range(len(prompts))]
        if logprobs is None:
            return rows
        return [rows[b] + ([(np.float32(lp[b, i]), ids[b, i, :top_n].copy(), tlp[b, i, :top_n].copy()) for i in range(min(int(lp_counts[b]), out.shape[1]))],) for b in range(len(prompts))]

    def _row_requests(self, requests, logprobs, who):
        """the GemmaRowRequestC array of generate_requests / serve_requests (who: what the refusals call a request, with its number) -> (array, what it points into, top_n)"""
        n = len(requests)
        keep, rq = [], (GemmaRowRequestC * max(n, 1))()
        vocab = self.vocab_size()
        top_n = -1 if logprobs is None else _logprobs_n(logprobs)
        for b, q in enumerate(requests):
            unknown = set(q) - set(ROW_REQUEST_KEYS)
            if unknown:
                raise ValueError("%s %d: unknown keys %s" % (who, b, sorted(unknown)))
            try:
                f = _filters(q.get("min_p", 0.0), q.get("repetition_penalty", 1.0), q.get("presence_penalty", 0.0), q.get("frequency_penalty", 0.0))
                bias = _bias_request(q.get("logit_bias"), q.get("banned_tokens", ()), q.get("allowed_tokens", ()), q.get("min_tokens", 0), q.get("stop_tokens", ()),
                                     q.get("max_new_tokens"), vocab)
                own = q.get("logprobs", logprobs)
                own = -1 if own is None else _logprobs_n(own)
            except ValueError as e:
                raise ValueError("%s %d: %s" % (who, b, e)) from None
            automaton = q.get("automaton")
            if automaton is not None and not isinstance(automaton, TokenAutomaton):
                raise ValueError("%s %d: automaton must be a host.TokenAutomaton" % (who, b))
            pr = np.ascontiguousarray(q.get("prompt", ()), dtype=np.int32)
            st = np.ascontiguousarray(list(q.get("stop_tokens", ())), dtype=np.int32)
            areq = None if automaton is None else automaton._request()
            keep.append((pr, st, bias, areq, automaton))
            r = rq[b]
            r.prompt, r.n_prompt = pr.ctypes.data if pr.size else None, int(pr.size)
            r.stop_tokens, r.n_stop = st.ctypes.data if st.size else None, int(st.size)
            r.bias = None if bias is None else C.addressof(bias[0])
            r.automaton = None if areq is None else C.addressof(areq)
            r.seed = int(q.get("seed", 0))
            r.temperature, r.top_k, r.top_p = float(q.get("temperature", 1.0)), int(q.get("top_k", 1)), float(q.get("top_p", 1.0))
            r.filters = (C.c_float * 4)(*f)
            mx = q.get("max_new_tokens")
            r.max_new = -1 if mx is None else int(mx)
            r.logprobs = own
            r.speculative = (1 if q.get("speculative_sampling") else 0) | (2 if q.get("speculate_constrained") else 0) | (4 if q.get("draft_hint") is not None else 0)
        return rq, keep, top_n

    def generate_requests(self, requests, logprobs=None):
        """GemmaModel::generateRequests: up to max_batch requests that need NOT agree, request b in row b.  requests: a list of dicts with generate()'s keyword names
        (max_new_tokens, stop_tokens, temperature, top_k, top_p, min_p, repetition_penalty, presence_penalty, frequency_penalty, logit_bias, banned_tokens,
        allowed_tokens, min_tokens, automaton) plus "prompt" and "seed" (the row's generator; default 0).  Row b gives what generate() gives for request b alone on
        a one-sequence model after the same seed.  logprobs: ONE n for the call; a row's own "logprobs" key that differs is refused, as are the speculative keys
        (speculative_sampling, speculate_constrained, draft_hint).  -> per row what generate_batch returns -- (tokens, finish reason[, log-probability entries]) --
        plus, for a row with an automaton, the state it ended in as a last element."""
        lib = load()
        n = len(requests)
        rq, keep, top_n = self._row_requests(requests, logprobs, "GemmaModel.generate_requests: row")
        caps = [int(q["max_new_tokens"]) if q.get("max_new_tokens") is not None else 1 << 16 for q in requests]
        cap = max(caps + [1])
        out = np.zeros((max(n, 1), cap), dtype=np.int32)
        counts, status, lp_counts, states, has_state = (np.zeros(max(n, 1), dtype=t) for t in (np.int64, np.int32, np.int64, np.int32, np.int32))
        width = max(top_n, 1)
        with_lp = top_n >= 0
        lp, ids, tlp = (np.zeros(out.shape if with_lp else (1, 1), dtype=np.float32), np.zeros((out.shape if with_lp else (1, 1)) + (width,), dtype=np.int32),
                        np.zeros((out.shape if with_lp else (1, 1)) + (width,), dtype=np.float32))
        lib.mila_gemma_model_generate_requests.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        _check(lib.mila_gemma_model_generate_requests(self.h, C.addressof(rq), n, out.ctypes.data, cap, counts.ctypes.data, status.ctypes.data,
                                                      lp.ctypes.data if with_lp else None, ids.ctypes.data if with_lp else None, tlp.ctypes.data if with_lp else None,
                                                      lp_counts.ctypes.data, states.ctypes.data, has_state.ctypes.data))
        rows = []
        for b in range(n):
            row = (out[b, :min(int(counts[b]), cap)].tolist(), GENERATE_STATUS[int(status[b])])
            if with_lp:
                row = row + ([(np.float32(lp[b, i]), ids[b, i, :top_n].copy(), tlp[b, i, :top_n].copy()) for i in range(min(int(lp_counts[b]), cap))],)
            if requests[b].get("automaton") is not None:
                row = row + (int(states[b]) if has_state[b] else None,)
            rows.append(row)
        return rows

    def serve_requests(self, requests, logprobs=None):
        """GemmaModel::serveRequests: generate_requests for ANY number of requests (>= 1) on a max_batch > 1 model -- a FIFO queue in front of the rows step: a request
        enters the lowest free row, a row whose request has ended goes to the next waiting one before the next step, and requests admitted together with an identical
        prompt share one prefill (the others fork the first one's KV rows and logits).  requests: generate_requests' dicts; a dict may also carry "n": k (k >= 1),
        expanded here into k consecutive requests with seeds seed, seed + 1, ..., seed + k - 1 (generate_batch's convention).  Request i gives what generate() gives
        for it alone on a one-sequence model after its seed, wherever and whenever it ran.  Refusals number the requests AFTER the expansion, as the results do.
        -> (rows, stats): rows[i] = what generate_requests returns for a row; stats = {"steps": rows steps replayed, "prefills", "prefill_tokens", "forks",
        "captures": rows-graph captures during the call, "rows": the row each request ran in, "admitted_at": the steps replayed before each admission,
        "finish_order": the position of each request's end among the call's, "admission_ms": host milliseconds the admissions spent in their
        {"setters", "prefill", "fork", "first_sample"}}."""
        return self._serve(requests, logprobs, None)

    def serve_requests_prefix(self, requests, logprobs=None, prefix_cache=True, min_prefix=1):
        """GemmaModel::serveRequests( ..., ServeParams{ prefix_cache, min_prefix } ): serve_requests with THE PREFIX CACHE.  Every row keeps a claim -- the tokens whose
        KV its caches hold -- beyond its request, until the row is written; an admission takes the longest prefix L <= len - 1 of its prompt that any row holds (a live
        one, a retired one, its own) by one fork of that prefix (none in place) and prefills only prompt[L:].  The claims live in the model: a later call reuses them;
        generate, generate_batch, generate_requests, score, a serve_requests without the cache and any failing serving call clear them (clear_prefix_cache(): by
        hand; prefix_cache_lengths(): what is held).  Request i gives what generate() gives for it on a one-sequence model on which its donors' requests ran before
        it, generate() itself reusing L positions.  min_prefix: the shortest prefix worth reusing (>= 1).  prefix_cache=False: serve_requests, the same stats dict.
        With the cache on, stats gains "reused_tokens" and "donor_row" per request (-1: none; the own row: in place; a whole fork of an identical prompt: its length
        and that row) and the totals "prefix_forks" and "prefix_in_place"; "prefill_tokens" counts the tokens actually prefilled.  (An entry of its own:
        serve_requests keeps its signature.)"""
        if isinstance(min_prefix, bool) or not isinstance(min_prefix, (int, np.integer)) or min_prefix < 1:
            raise ValueError("GemmaModel.serve_requests_prefix: min_prefix must be an integer >= 1 (got %r)" % (min_prefix,))
        return self._serve(requests, logprobs, (bool(prefix_cache), int(min_prefix)))

    def clear_prefix_cache(self):
        """GemmaModel::clearPrefixCache: forget what the rows hold"""
        lib = load()
        lib.mila_gemma_model_clear_prefix_cache.argtypes = [C.c_void_p]
        _check(lib.mila_gemma_model_clear_prefix_cache(self.h))

    def prefix_cache_lengths(self):
        """GemmaModel::prefixCacheLengths: per row, the number of cache positions the prefix cache knows the tokens of"""
        lib = load()
        lib.mila_gemma_model_prefix_cache_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        out, rows = (C.c_int64 * 4)(), C.c_int32(0)
        _check(lib.mila_gemma_model_prefix_cache_lengths(self.h, out, C.byref(rows)))
        return [int(out[r]) for r in range(rows.value)]

    def _serve(self, requests, logprobs, prefix):
        """serve_requests (prefix None) / serve_requests_prefix (prefix = (prefix_cache, min_prefix))"""
        lib = load()
        flat = []
        for q in requests:
            q = dict(q)
            k = q.pop("n", 1)
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
                raise ValueError("GemmaModel.serve_requests: request %d: n must be an integer >= 1 (got %r)" % (len(flat), k))
            seed = int(q.get("seed", 0))
            for j in range(int(k)):
                flat.append(dict(q, seed=seed + j) if k > 1 else q)
        n = len(flat)
        rq, keep, top_n = self._row_requests(flat, logprobs, "GemmaModel.serve_requests: request")
        caps = [int(q["max_new_tokens"]) if q.get("max_new_tokens") is not None else 1 << 16 for q in flat]
        cap = max(caps + [1])
        out = np.zeros((max(n, 1), cap), dtype=np.int32)
        counts, status, lp_counts, states, has_state, rows_of, finish = (np.zeros(max(n, 1), dtype=t) for t in (np.int64, np.int32, np.int64, np.int32, np.int32, np.int32, np.int32))
        admitted, totals, times = np.zeros(max(n, 1), dtype=np.int64), np.zeros(5, dtype=np.int64), np.zeros(4, dtype=np.float64)
        width = max(top_n, 1)
        with_lp = top_n >= 0
        lp, ids, tlp = (np.zeros(out.shape if with_lp else (1, 1), dtype=np.float32), np.zeros((out.shape if with_lp else (1, 1)) + (width,), dtype=np.int32),
                        np.zeros((out.shape if with_lp else (1, 1)) + (width,), dtype=np.float32))
        args = (self.h, C.addressof(rq), n, out.ctypes.data, cap, counts.ctypes.data, status.ctypes.data, lp.ctypes.data if with_lp else None,
                ids.ctypes.data if with_lp else None, tlp.ctypes.data if with_lp else None, lp_counts.ctypes.data, states.ctypes.data, has_state.ctypes.data,
                rows_of.ctypes.data, admitted.ctypes.data, finish.ctypes.data, totals.ctypes.data, times.ctypes.data)
        if prefix is None:
            lib.mila_gemma_model_serve_requests.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 13
            _check(lib.mila_gemma_model_serve_requests(*args))
        else:
            reused, donor, prefix_totals = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(2, dtype=np.int64)
            lib.mila_gemma_model_serve_requests_prefix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64] + [C.c_void_p] * 13 + [C.c_int, C.c_int] + [C.c_void_p] * 3
            _check(lib.mila_gemma_model_serve_requests_prefix(*args, int(prefix[0]), prefix[1], reused.ctypes.data, donor.ctypes.data, prefix_totals.ctypes.data))
        rows = []
        for b in range(n):
            row = (out[b, :min(int(counts[b]), cap)].tolist(), GENERATE_STATUS[int(status[b])])
            if with_lp:
                row = row + ([(np.float32(lp[b, i]), ids[b, i, :top_n].copy(), tlp[b, i, :top_n].copy()) for i in range(min(int(lp_counts[b]), cap))],)
            if flat[b].get("automaton") is not None:
                row = row + (int(states[b]) if has_state[b] else None,)
            rows.append(row)
        stats = {"steps": int(totals[0]), "prefills": int(totals[1]), "prefill_tokens": int(totals[2]), "forks": int(totals[3]), "captures": int(totals[4]),
                 "rows": rows_of[:n].tolist(), "admitted_at": admitted[:n].tolist(), "finish_order": finish[:n].tolist(),
                 "admission_ms": dict(zip(("setters", "prefill", "fork", "first_sample"), (float(t) for t in times)))}
        if prefix is not None and prefix[0]:
            stats.update(reused_tokens=reused[:n].tolist(), donor_row=donor[:n].tolist(), prefix_forks=int(prefix_totals[0]), prefix_in_place=int(prefix_totals[1]))
        return rows, stats

    def rows_graph_info(self):
        """{"captures": captures of the model's rows graph so far, "nodes": kernel nodes of the captured rows step}"""
        lib = load()
        lib.mila_gemma_model_rows_graph_info.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_int64 * 2)()
        _check(lib.mila_gemma_model_rows_graph_info(self.h, out))
        return {"captures": int(out[0]), "nodes": int(out[1])}

    def _generate_batch(self, prompts, max_new_tokens=None, stop_tokens=(), temperature=1.0, top_k=1, top_p=1.0, seed=0, logprobs=None):
        """GemmaModel::generateBatch: up to max_batch prompts at once, prompt b in row b -> [(tokens, finish reason)] per prompt, by generate()'s rules.  Row b samples
        from its own generator seeded seed + b."""
        lib = load()
        lib.mila_gemma_model_generate_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_uint64,
                                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]) if len(prompts) else np.zeros(0), dtype=np.int32)
        offs = np.ascontiguousarray(np.cumsum([0] + [len(p) for p in prompts]), dtype=np.int64)
        st = np.ascontiguousarray(list(stop_tokens), dtype=np.int32)
        cap = int(max_new_tokens) if max_new_tokens is not None else 1 << 16
        out = np.zeros((max(len(prompts), 1), max(cap, 1)), dtype=np.int32)
        counts, status = np.zeros(max(len(prompts), 1), dtype=np.int64), np.zeros(max(len(prompts), 1), dtype=np.int32)
        if logprobs is not None:
            # ... with a list of (logprob, top_ids, top_logprobs) per emitted token as a third element of every prompt's tuple
            top_n = _logprobs_n(logprobs)
            lib.mila_gemma_model_generate_rows_logprobs.argtypes = lib.mila_gemma_model_generate_rows.argtypes + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lp, ids, tlp = np.zeros(out.shape, dtype=np.float32), np.zeros(out.shape + (top_n,), dtype=np.int32), np.zeros(out.shape + (top_n,), dtype=np.float32)
            lp_counts = np.zeros(max(len(prompts), 1), dtype=np.int64)
            _check(lib.mila_gemma_model_generate_rows_logprobs(self.h, flat.ctypes.data, offs.ctypes.data, len(prompts), -1 if max_new_tokens is None else int(max_new_tokens),
                                                               st.ctypes.data if len(st) else None, len(st), float(temperature), int(top_k), float(top_p), int(seed), out.ctypes.data,
                                                               out.shape[1], counts.ctypes.data, status.ctypes.data, top_n, lp.ctypes.data, ids.ctypes.data, tlp.ctypes.data,
                                                               lp_counts.ctypes.data))
            return [(out[b, :min(int(counts[b]), out.shape[1])].tolist(), GENERATE_STATUS[int(status[b])],
                     [(np.float32(lp[b, i]), ids[b, i].copy(), tlp[b, i].copy()) for i in range(min(int(lp_counts[b]), out.shape[1]))]) for b in range(len(prompts))]
        _check(lib.mila_gemma_model_generate_rows(self.h, flat.ctypes.data, offs.ctypes.data, len(prompts), -1 if max_new_tokens is None else int(max_new_tokens),
                                                  st.ctypes.data if len(st) else None, len(st), float(temperature), int(top_k), float(top_p), int(seed), out.ctypes.data,
                                                  out.shape[1], counts.ctypes.data, status.ctypes.data))
        return [(out[b, :min(int(counts[b]), out.shape[1])].tolist(), GENERATE_STATUS[int(status[b])]) for b in range(len(prompts))]

    def close(self):
        if self.h:
            load().mila_gemma_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Gpt:
    """GptTransformer (GPT-2) on cuda:0; parameters in the order of oracle orc_cpu_gpt2_forward.
    precision "bf16" (BASELINE config 2): parameters and logits are bf16 bit patterns (uint16); "fp32" (BASELINE config 1's model on the device, through the FP32 rows
    of Linear / LayerNorm / MHA / GELU / Residual / LPE): float32 parameters and logits."""

    def __init__(self, vocab, max_seq, C_, L, NH, B, T, precision="bf16"):
        lib = load()
        lib.mila_gpt_create_p.restype = C.c_void_p
        lib.mila_gpt_create_p.argtypes = [C.c_int] + [C.c_int64] * 7
        self.shape = (B, T, vocab)
        self.precision = precision
        self.dtype = {"bf16": np.uint16, "fp32": np.float32}[precision]
        self.h = lib.mila_gpt_create_p({"bf16": 0, "fp32": 1}[precision], vocab, max_seq, C_, L, NH, B, T)
        if not self.h:
            raise (ValueError if b"invalid_argument" in lib.mila_gpt_last_error() else RuntimeError)(lib.mila_gpt_last_error().decode())

    def component_names(self):
        """names of the model's components in construction order (lenc, each block and its children, ln_final, lm_head)"""
        lib = load()
        lib.mila_gpt_component_names.restype = C.c_int64
        lib.mila_gpt_component_names.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        need = lib.mila_gpt_component_names(self.h, None, 0)
        if need < 0:
            raise RuntimeError(lib.mila_gpt_last_error().decode())
        buf = C.create_string_buffer(need)
        lib.mila_gpt_component_names(self.h, buf, need)
        return buf.value.decode().split("\n")[:-1]

    def memory_stats(self):
        """GptTransformer::getRequiredMemory() beside getMemoryStats(): {"required": {...}, "actual": {...}} with device_parameter_bytes / device_state_bytes"""
        lib = load()
        lib.mila_gpt_memory_stats.argtypes = [C.c_void_p, C.c_void_p]
        out = (C.c_double * 4)()
        if lib.mila_gpt_memory_stats(self.h, out):
            raise RuntimeError(lib.mila_gpt_last_error().decode())
        return {"required": {"device_parameter_bytes": int(out[0]), "device_state_bytes": int(out[1])}, "actual": {"device_parameter_bytes": int(out[2]), "device_state_bytes": int(out[3])}}

    def load_parameters(self, params_bf16_bits):
        lib = load()
        assert len(params_bf16_bits) == lib.mila_gpt_parameter_count(self.h)
        for i, p in enumerate(params_bf16_bits):
            p = np.ascontiguousarray(p, dtype=self.dtype)
            rc = lib.mila_gpt_load_parameter(self.h, i, p.ctypes.data, p.nbytes)
            if rc:
                raise ValueError(lib.mila_gpt_last_error().decode())

    def forward(self, tokens):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.shape, dtype=self.dtype)
        ms = C.c_double()
        rc = load().mila_gpt_forward(self.h, t.ctypes.data, out.ctypes.data, C.byref(ms))
        if rc < 0:
            raise RuntimeError(load().mila_gpt_last_error().decode())
        if rc > 0:
            raise IndexError("token index outside vocabulary range (flat position %d)" % (rc - 1))
        self.last_ms = ms.value
        return out

    def forward_timed(self, tokens):
        """forward() without the logits copy to the host (823 MB at config 2): device time in self.last_ms"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        ms = C.c_double()
        rc = load().mila_gpt_forward(self.h, t.ctypes.data, None, C.byref(ms))
        if rc:
            raise RuntimeError(load().mila_gpt_last_error().decode() if rc < 0 else "token index outside the vocabulary")
        self.last_ms = ms.value
        return ms.value

    def prefill(self, tokens):
        """GptTransformer::prefill: tokens [B, T' <= T] -> logits [B, V] (bf16 bits) of the last position; every block's KV cache is filled"""
        lib = load()
        lib.mila_gpt_prefill.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        assert t.ndim == 2 and t.shape[0] == self.shape[0]
        out = np.empty((self.shape[0], self.shape[2]), dtype=self.dtype)
        rc = lib.mila_gpt_prefill(self.h, t.ctypes.data, t.shape[1], out.ctypes.data)
        if rc:
            text = lib.mila_gpt_last_error().decode()
            raise (ValueError if rc == capi.MILA_E_INVALID_ARGUMENT else RuntimeError)(text)
        return out

    def decode(self, tokens, position):
        """GptTransformer::decode: one token per sequence [B] at absolute `position` -> logits [B, V] (bf16 bits)"""
        lib = load()
        lib.mila_gpt_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        t = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)
        assert t.size == self.shape[0]
        out = np.empty((self.shape[0], self.shape[2]), dtype=self.dtype)
        rc = lib.mila_gpt_decode(self.h, t.ctypes.data, int(position), out.ctypes.data)
        if rc:
            text = lib.mila_gpt_last_error().decode()
            raise (ValueError if rc == capi.MILA_E_INVALID_ARGUMENT else RuntimeError)(text)
        return out

    def close(self):
        if self.h:
            load().mila_gpt_destroy(self.h)
            self.h = None


def safetensors_list(path):
    """host-only: [(name, dtype, nbytes, shape)], {metadata} of a SafeTensors file as the C++ reader sees it"""
    lib = load()
    need = lib.mila_safetensors_list(str(path).encode(), None, 0)
    if need < 0:
        _check(int(need))
    buf = C.create_string_buffer(int(need) + 1)
    lib.mila_safetensors_list(str(path).encode(), buf, int(need) + 1)
    tensors, meta = [], {}
    for line in buf.value.decode().splitlines():
        if line.startswith("# "):
            k, v = line[2:].split("=", 1)
            meta[k] = v
        else:
            name, dtype, nbytes, shape = (line.split(" ") + [""])[:4]
            tensors.append((name, dtype, int(nbytes), tuple(int(d) for d in shape.split(",") if d)))
    return tensors, meta


def safetensors_copy(src, dst):
    """host-only: rewrite src as dst through the C++ reader and writer"""
    _check(load().mila_safetensors_copy(str(src).encode(), str(dst).encode()))


def _text_call(fn, *args):
    need = fn(*args, None, 0)
    if need < 0:
        _check(int(need))
    buf = C.create_string_buffer(int(need) + 1)
    fn(*args, buf, int(need) + 1)
    return buf.value.decode()


def component_scenarios(device=0):
    """the leaf components (Residual, Swiglu<Gelu>, Rope, GroupedQueryAttention, TokenEmbedding + the tied Linear) used standalone on the GPU,
    checked against the launchers they resolve to, with the reference's lifecycle errors; raises with the failing scenario's name"""
    lib = load()
    lib.mila_component_scenarios.argtypes = [C.c_int]
    _check(lib.mila_component_scenarios(device))


def pretrained_list(path):
    """host-only: ([(name, dtype, nbytes, shape)] in ascending file-offset order, {container, mila_quantization, mila_config})
    of a MILA .bin or SafeTensors file as the C++ PretrainedModelReader sees it"""
    tensors, meta = [], {}
    for line in _text_call(load().mila_pretrained_list, str(path).encode()).splitlines():
        if line.startswith("# "):
            k, v = line[2:].split("=", 1)
            meta[k] = v
        else:
            name, dtype, nbytes, shape = (line.split(" ") + [""])[:4]
            tensors.append((name, dtype, int(nbytes), tuple(int(d) for d in shape.split(",") if d)))
    return tensors, meta


def pretrained_to_milabin(src, dst, metadata_json=None):
    """host-only: rewrite a SafeTensors (or MILA) file as a MILA .bin through the C++ reader and writer"""
    _check(load().mila_pretrained_to_milabin(str(src).encode(), str(dst).encode(), None if metadata_json is None else metadata_json.encode()))


def pretrained_metadata_roundtrip(json_text):
    """host-only: toMetadataJSON(parseMetadataJSON(text))"""
    return _text_call(load().mila_pretrained_metadata_roundtrip, json_text.encode())


class LinearComponent:
    """ONE Linear<Rocm, BF16, policy> of the host mirror (libmila_host: host/src/linear_runner.cpp): load a weight as the reference's loadParameter does (bf16 blob ->
    quantize-on-load under a quantized policy, or the policy's storage form + weight_scale), then forward() at any row count through RocmLinearOp::forward."""

    def __init__(self, policy, K, N, max_rows, bias=False, device=0):
        lib = load()
        lib.mila_linear_create.restype = C.c_void_p
        lib.mila_linear_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int]
        lib.mila_linear_destroy.argtypes = [C.c_void_p]
        lib.mila_linear_load.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
        lib.mila_linear_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mila_linear_set.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.mila_linear_forward.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.mila_linear_last_error.restype = C.c_char_p
        self.K, self.N, self.policy = K, N, policy
        self.h = lib.mila_linear_create(POLICIES[policy], K, N, max_rows, int(bool(bias)), device)
        if not self.h:
            raise RuntimeError(lib.mila_linear_last_error().decode())

    def _check(self, rc):
        if rc:
            text = load().mila_linear_last_error().decode()
            raise (ValueError if rc == capi.MILA_E_INVALID_ARGUMENT else (TypeError if rc == capi.MILA_E_UNSUPPORTED else RuntimeError))(text)

    def load(self, name, blob):
        b = np.ascontiguousarray(blob)
        self._check(load().mila_linear_load(self.h, name.encode(), b.ctypes.data, b.nbytes))

    def read(self):
        """(stored weight bytes as uint8, scales as float32 or None)"""
        lib = load()
        wb, sb = C.c_int64(), C.c_int64()
        self._check(lib.mila_linear_read(self.h, None, C.byref(wb), None, C.byref(sb)))
        w = np.empty(wb.value, dtype=np.uint8)
        s = np.empty(sb.value // 4, dtype=np.float32)
        self._check(lib.mila_linear_read(self.h, w.ctypes.data, None, s.ctypes.data if sb.value else None, None))
        return w, (s if sb.value else None)

    def set(self, fp8_activation_prefill=None, resident=None):
        self._check(load().mila_linear_set(self.h, -1 if fp8_activation_prefill is None else int(bool(fp8_activation_prefill)), -1 if resident is None else int(bool(resident))))

    def forward(self, x_bf16_bits):
        x = np.ascontiguousarray(x_bf16_bits, dtype=np.uint16)
        M = x.size // self.K
        y = np.empty((M, self.N), dtype=np.uint16)
        self._check(load().mila_linear_forward(self.h, M, x.ctypes.data, y.ctypes.data))
        return y

    def close(self):
        if self.h:
            load().mila_linear_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def linear_install_shared_probe(policy, which):
    """Linear<policy>::installSharedWeight( nullptr ) (which 0) / ( nullptr, nullptr ) (which 1) on an unbuilt component: returns "logic_error", "invalid_argument" or "ok" """
    lib = load()
    lib.mila_linear_install_shared_probe.argtypes = [C.c_int, C.c_int]
    rc = lib.mila_linear_install_shared_probe(POLICIES[policy], which)
    return {0: "ok", capi.MILA_E_UNSUPPORTED: "logic_error", capi.MILA_E_INVALID_ARGUMENT: "invalid_argument"}.get(rc, "error %d" % rc)


class Sampler:
    """RocmSamplingOp (counterpart of CudaSamplingOp<FP32>): sample() = forward + readback; sample_enqueued() = enqueueForward + awaitToken; await_token() alone raises TypeError
    (std::logic_error) when nothing is outstanding"""

    def __init__(self, vocab, softcap=0.0, device=0):
        lib = load()
        lib.mila_sampler_create.restype = C.c_void_p
        lib.mila_sampler_create.argtypes = [C.c_int64, C.c_float, C.c_int]
        lib.mila_sampler_destroy.argtypes = [C.c_void_p]
        lib.mila_sampler_set_logits.argtypes = [C.c_void_p, C.c_void_p]
        lib.mila_sampler_sample.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_void_p]
        lib.mila_sampler_sample_filtered.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        lib.mila_sampler_set_token_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.mila_sampler_read_token_table.argtypes = [C.c_void_p, C.c_void_p]
        lib.mila_linear_last_error.restype = C.c_char_p
        self.vocab = vocab
        self.h = lib.mila_sampler_create(vocab, softcap, device)
        if not self.h:
            raise RuntimeError(lib.mila_linear_last_error().decode())

    def set_logits(self, logits):
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        assert lg.size == self.vocab
        self._keep = lg          # the copy is asynchronous on the context stream
        if load().mila_sampler_set_logits(self.h, lg.ctypes.data):
            raise RuntimeError(load().mila_linear_last_error().decode())

    @staticmethod
    def _raise(rc):
        text = load().mila_linear_last_error().decode()
        raise (TypeError if rc == capi.MILA_E_UNSUPPORTED else (ValueError if rc == capi.MILA_E_INVALID_ARGUMENT else RuntimeError))(text)

    def _run(self, mode, temperature, top_k, top_p, r, filters=None):
        tok = C.c_int32()
        if filters is None or filters == _filters():
            rc = load().mila_sampler_sample(self.h, mode, temperature, top_k, top_p, r, C.byref(tok))
        else:
            f = (C.c_float * 4)(*filters)
            rc = load().mila_sampler_sample_filtered(self.h, mode, temperature, top_k, top_p, r, f, C.byref(tok))
        if rc:
            self._raise(rc)
        return tok.value

    def sample(self, temperature=1.0, top_k=0, top_p=1.0, r=0.5, **filters):
        """filters: min_p, repetition_penalty, presence_penalty, frequency_penalty (penalties need set_token_table() first; the sampled token is counted there)"""
        return self._run(0, temperature, top_k, top_p, r, _filters(**filters))

    def sample_enqueued(self, temperature=1.0, top_k=0, top_p=1.0, r=0.5, **filters):
        return self._run(1, temperature, top_k, top_p, r, _filters(**filters))

    def set_token_table(self, prompt):
        """a new request: counts to zero, the prompt tokens' flags set"""
        ids = np.ascontiguousarray(prompt, dtype=np.int32)
        rc = load().mila_sampler_set_token_table(self.h, ids.ctypes.data, ids.size)
        if rc:
            self._raise(rc)

    def token_table(self):
        """the table's words (uint32 [vocab]): bit 31 = in the prompt, bits 0 .. 30 = times generated"""
        out = np.zeros(self.vocab, dtype=np.uint32)
        rc = load().mila_sampler_read_token_table(self.h, out.ctypes.data)
        if rc:
            self._raise(rc)
        return out

    def await_token(self):
        return self._run(2, 0.0, 0, 1.0, 0.0)

    def close(self):
        if self.h:
            load().mila_sampler_destroy(self.h)
            self.h = None


class activation_tap:
    """context manager: records the per-token e4m3 activations (bytes + scales) every Linear on an fp8 x fp8 prefill path consumed while it is open
    (Compute::ActivationTap; test instrument) -> .records = [(M, K, N, x8 [M, K] uint8, ts [M] float32)] in call order"""

    def __enter__(self):
        lib = load()
        lib.mila_linear_tap_count.restype = C.c_int64
        lib.mila_linear_tap_get.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mila_linear_tap_begin()
        self.records = []
        return self

    def __exit__(self, *exc):
        lib = load()
        lib.mila_linear_tap_end()
        for i in range(lib.mila_linear_tap_count()):
            dims = (C.c_int32 * 3)()
            lib.mila_linear_tap_get(i, dims, None, None)
            M, K, N = dims[0], dims[1], dims[2]
            x8, ts = np.empty((M, K), dtype=np.uint8), np.empty(M, dtype=np.float32)
            lib.mila_linear_tap_get(i, None, x8.ctypes.data, ts.ctypes.data)
            self.records.append((M, K, N, x8, ts))
        return False


KV_POLICIES = {"none": 0, "sliding_window": 1, "fp8": 2}


class GqaOpConfigC(C.Structure):
    _fields_ = [("num_heads", C.c_int64), ("num_kv_heads", C.c_int64), ("head_dim", C.c_int64), ("window", C.c_int64), ("attention_scale", C.c_float)]


class GqaComponent:
    """ONE GroupedQueryAttention<Rocm, BF16, kv_policy> of the host mirror (libmila_host: host/src/gqa_runner.cpp) over its op-owned KV cache: kv_policy "none"
    (NoKvCompression), "sliding_window" (SlidingWindowKvCache) or "fp8" (PerChannelKvFp8<>: e4m3 K / V + one fp32 scale per KV head per cached token).  q / k / v and
    the outputs are bf16 bit patterns (uint16 numpy)."""

    def __init__(self, kv_policy, num_heads, num_kv_heads, head_dim, window=0, attention_scale=0.0, batch=1, max_seq=1024, prefill_chunk=0, device=0):
        lib = load()
        vp, i64 = C.c_void_p, C.c_int64
        lib.mila_gqa_create.restype = vp
        lib.mila_gqa_create.argtypes = [C.c_int, C.POINTER(GqaOpConfigC), i64, i64, i64, C.c_int]
        lib.mila_gqa_destroy.argtypes = [vp]
        lib.mila_gqa_init_cache.argtypes = [vp]
        lib.mila_gqa_prefill.argtypes = [vp, vp, vp, vp, i64, i64, vp]
        lib.mila_gqa_decode.argtypes = [vp, vp, vp, vp, i64, vp]
        lib.mila_gqa_decode_at.argtypes = [vp, vp, vp, vp, i64, i64, vp]
        lib.mila_gqa_note_cache_length.argtypes = [vp, i64]
        lib.mila_gqa_rewind.argtypes = [vp, i64]
        lib.mila_gqa_state_bytes.argtypes = [vp, vp]
        lib.mila_gqa_read_cache.argtypes = [vp, vp, vp, vp, vp]
        lib.mila_gqa_fused_surface_probe.argtypes = [vp, C.c_int]
        self.kv_policy, self.B, self.NH, self.NKV, self.HS = kv_policy, batch, num_heads, num_kv_heads, head_dim
        cfg = GqaOpConfigC(num_heads, num_kv_heads, head_dim, window, attention_scale)
        self.h = lib.mila_gqa_create(KV_POLICIES[kv_policy], C.byref(cfg), batch, max_seq, prefill_chunk, device)
        if not self.h:
            text = lib.mila_host_last_error().decode()
            raise (ValueError if text.startswith("invalid_argument") else RuntimeError)(text)

    @staticmethod
    def _check(rc):
        if rc:
            text = load().mila_host_last_error().decode()
            raise (ValueError if rc == capi.MILA_E_INVALID_ARGUMENT else (TypeError if rc == capi.MILA_E_UNSUPPORTED else RuntimeError))(text)

    @staticmethod
    def _rows(a):
        return np.ascontiguousarray(a, dtype=np.uint16)

    def init_cache(self):
        self._check(load().mila_gqa_init_cache(self.h))

    def prefill(self, q, k, v, position):
        """q [B, T, NH*HS], k / v [B, T, NKV*HS] at absolute positions position .. position + T - 1 -> [B, T, NH*HS]"""
        q, k, v = self._rows(q), self._rows(k), self._rows(v)
        T = q.size // (self.B * self.NH * self.HS)
        y = np.empty((self.B, T, self.NH * self.HS), dtype=np.uint16)
        self._check(load().mila_gqa_prefill(self.h, q.ctypes.data, k.ctypes.data, v.ctypes.data, T, position, y.ctypes.data))
        return y

    def decode(self, q, k, v, position):
        """one token per sequence: q [B, NH*HS], k / v [B, NKV*HS] -> [B, NH*HS]"""
        q, k, v = self._rows(q), self._rows(k), self._rows(v)
        y = np.empty((self.B, self.NH * self.HS), dtype=np.uint16)
        self._check(load().mila_gqa_decode(self.h, q.ctypes.data, k.ctypes.data, v.ctypes.data, position, y.ctypes.data))
        return y

    def decode_at(self, q, k, v, position, max_len):
        """decode() with the position read from DEVICE memory by the kernels (the op's decodeAt; fp8 policy only): max_len bounds the live length inside its band
        bucket.  state()["length"] does not move: follow up with note_cache_length(position + 1)"""
        q, k, v = self._rows(q), self._rows(k), self._rows(v)
        y = np.empty((self.B, self.NH * self.HS), dtype=np.uint16)
        self._check(load().mila_gqa_decode_at(self.h, q.ctypes.data, k.ctypes.data, v.ctypes.data, position, max_len, y.ctypes.data))
        return y

    def note_cache_length(self, length):
        self._check(load().mila_gqa_note_cache_length(self.h, length))

    def rewind(self, length):
        self._check(load().mila_gqa_rewind(self.h, length))

    def state(self):
        """dict: op_state_bytes, op_required_state_bytes, component_state_bytes, component_required_state_bytes, capacity, length"""
        out = (C.c_int64 * 6)()
        self._check(load().mila_gqa_state_bytes(self.h, out))
        return dict(zip(("op_state_bytes", "op_required_state_bytes", "component_state_bytes", "component_required_state_bytes", "capacity", "length"), list(out)))

    def read_cache(self):
        """fp8 policy: (K8, V8 uint8 [B, NKV, capacity, HS], Ks, Vs float32 [B, NKV, capacity]); bf16 policies: (K, V uint16 [B, NKV, capacity, HS], None, None)"""
        cap = self.state()["capacity"]
        shape = (self.B, self.NKV, cap, self.HS)
        if self.kv_policy == "fp8":
            k8, v8 = np.empty(shape, dtype=np.uint8), np.empty(shape, dtype=np.uint8)
            ks, vs = np.empty(shape[:3], dtype=np.float32), np.empty(shape[:3], dtype=np.float32)
            self._check(load().mila_gqa_read_cache(self.h, k8.ctypes.data, v8.ctypes.data, ks.ctypes.data, vs.ctypes.data))
            return k8, v8, ks, vs
        k, v = np.empty(shape, dtype=np.uint16), np.empty(shape, dtype=np.uint16)
        self._check(load().mila_gqa_read_cache(self.h, k.ctypes.data, v.ctypes.data, None, None))
        return k, v, None, None

    def fused_surface_probe(self, which):
        """call prefillFromCache / keyCache / valueCache (the methods the fused q/k/v entries use); raises TypeError (std::logic_error) under the fp8 policy"""
        self._check(load().mila_gqa_fused_surface_probe(self.h, {"prefillFromCache": 0, "keyCache": 1, "valueCache": 2}[which]))

    def close(self):
        if self.h:
            load().mila_gqa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
