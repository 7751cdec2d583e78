"""GPU: the chain step in the Gemma model (GemmaConfig::draft_tokens > 0) -- the token about to be decoded and up to three drafted successors in one pass over the
weights, on the ONE KV cache.  The oracle is exact: a draft_tokens = 0 model with the same seed decoding the same sequence alone through the fused step gives the true
continuation and the logits at every position; every chain row fed a correct token must have those logits BIT FOR BIT, the accepted run must be the longest correct
draft prefix, and a rejected draft's stale cache rows must do no harm to the steps that follow."""
import numpy as np
import pytest

from mila_amd import host
from test_gemma_host_gpu import MAX_SEQ, MEDIUM, SMALL

pytestmark = pytest.mark.gpu

SEED = 7
PROMPT = [3, 512, 77, 1023, 0, 42, 256, 8, 640]
STEPS = 30      # positions 9 .. 38 of the 64


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


_truth_cache = {}


def _truth(policy, cfg_name, cfg):
    """(prefill logits, tokens tok[0 ..], logits[i] = the alone step of tok[i] at position len(PROMPT) + i), computed once per (policy, geometry)"""
    key = (policy, cfg_name)
    if key not in _truth_cache:
        g = host.Gemma(policy, cfg, max_seq=MAX_SEQ, max_prefill=16, seed=SEED)
        try:
            pre = g.prefill(PROMPT)
            toks, logits = [int(np.argmax(pre))], []
            for i in range(STEPS):
                logits.append(g.decode(toks[-1], len(PROMPT) + i, "fused"))
                toks.append(int(np.argmax(logits[-1])))
        finally:
            g.close()
        _truth_cache[key] = (pre, toks, logits)
    return _truth_cache[key]


def _chain_equals_alone(policy, cfg_name, cfg):
    pre, tok, want = _truth(policy, cfg_name, cfg)
    vocab, P = cfg["vocab_size"], len(PROMPT)
    models = {m: host.Gemma(policy, cfg, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3) for m in ("fused", "graph")}
    try:
        for g in models.values():
            assert _same(g.prefill(PROMPT), pre)
        i = 0      # index of the token about to be decoded

        def step(T, corrupt, what):
            nonlocal i
            tokens = tok[i:i + T]
            if corrupt is not None:
                tokens[corrupt + 1] = (tokens[corrupt + 1] + 1) % vocab
            good = T if corrupt is None else corrupt + 1      # rows fed correct tokens = the accepted run
            out = {m: g.decode_chain(tokens, P + i, m) for m, g in models.items()}
            for m, (logits, count, accepted, new_pos) in out.items():
                w = "%s (%s, token index %d)" % (what, m, i)
                for t in range(good):
                    assert _same(logits[t], want[i + t]), "%s: row %d differs from the alone step at that position" % (w, t)
                assert count == good and accepted == tok[i + 1:i + 1 + good] and new_pos == P + i + good, (w, count, accepted, new_pos)
            assert _same(out["fused"][0], out["graph"][0]), "%s: the eager chain step differs from the graph replay" % what
            i += good

        step(4, None, "true drafts")
        for j in (0, 1, 2):
            step(4, j, "draft %d corrupted" % j)
            step(4, None, "true drafts behind the stale rows of corrupted draft %d" % j)      # the rejected rows are overwritten before anything reads them
        info = {m: g.chain_graph_info() for m, g in models.items()}
        assert info["graph"]["captures"] == 1 and info["graph"]["rows"] == 4 and info["graph"]["nodes"] > 0, info
        assert info["fused"]["captures"] == 0
        # shorter chains on the same model: rows 2 and 3 of the buffers are not part of the step; another T is another capture
        step(2, None, "T = 2")
        step(3, 1, "T = 3, the last draft corrupted")
        step(3, None, "T = 3")
        assert models["graph"].chain_graph_info()["captures"] == 3
        assert i < STEPS
        # the one-row step of a chain model goes on from there: the same position word, the same cache
        for m, g in models.items():
            assert _same(g.decode(tok[i], P + i, "graph" if m == "graph" else "fused"), want[i]), m
    finally:
        for g in models.values():
            g.close()


@pytest.mark.parametrize("policy", ["bf16", "fp8", "fp4"])
def test_chain_rows_equal_the_alone_steps_and_the_longest_correct_prefix_is_accepted(policy):
    _chain_equals_alone(policy, "SMALL", SMALL)


def test_chain_rows_equal_the_alone_steps_with_more_than_one_weight_step_per_row():
    """the MEDIUM geometry (D 1280, F 2560): the Linears see more than one pipeline step per weight row"""
    _chain_equals_alone("bf16", "MEDIUM", MEDIUM)


def test_draft_tokens_zero_is_the_model_it_was_and_required_memory_is_actual():
    plain = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED)
    zero = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=0)
    three = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=3)
    one = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=1)
    try:
        sp, s0, s3, s1 = plain.memory_stats(), zero.memory_stats(), three.memory_stats(), one.memory_stats()
        assert sp["actual"] == s0["actual"] and sp["required"] == s0["required"]
        for s in (s1, s3):
            assert s["required"]["device_state_bytes"] == s["actual"]["device_state_bytes"] > sp["actual"]["device_state_bytes"]
            assert s["actual"]["device_parameter_bytes"] == sp["actual"]["device_parameter_bytes"]
        # no extra caches
        kv_bytes = sum(2 * 2 * (SMALL["num_global_kv_heads"] * SMALL["global_head_dim"] if (l + 1) % SMALL["sliding_window_pattern"] == 0 else SMALL["num_kv_heads"] * SMALL["head_dim"]) * MAX_SEQ
                       for l in range(SMALL["num_layers"]))
        rows4 = host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, max_batch=4)
        try:
            s4 = rows4.memory_stats()
        finally:
            rows4.close()
        grow3, grow4 = s3["actual"]["device_state_bytes"] - sp["actual"]["device_state_bytes"], s4["actual"]["device_state_bytes"] - sp["actual"]["device_state_bytes"]
        assert s1["actual"]["device_state_bytes"] < s3["actual"]["device_state_bytes"]
        # the four-row batched model pays three more sets of caches; the four-row chain model none -- it holds the same rows buffers plus the roped q rows behind the
        # attention partials (4 rows x 4 heads x 128 x 2 bytes) and its five result words
        assert grow4 - grow3 == 3 * kv_bytes - (4 * 4 * 128 * 2 + 5 * 4), (grow3, grow4, kv_bytes)
        a, b = plain.decode(5, 0, "graph"), zero.decode(5, 0, "graph")
        assert _same(a, b) and plain.graph_node_count() == zero.graph_node_count() > 0
        assert _same(three.decode(5, 0, "graph"), a) and three.graph_node_count() == plain.graph_node_count()      # the one-row path of a chain model is the same path
        with pytest.raises(RuntimeError):
            zero.decode_chain([5, 6], 0)      # no chain on a model without draft tokens
        with pytest.raises(ValueError):
            one.decode_chain([5, 6, 7], 0)    # more rows than draft_tokens + 1
        with pytest.raises(ValueError):
            three.decode_chain([5], 0)        # a chain step has at least one draft
        with pytest.raises(ValueError):
            three.decode_chain([5, 6, 7], MAX_SEQ - 2)      # the last row would pass the sequence length
        with pytest.raises(RuntimeError):
            three.decode_rows(2, 0)           # ... and no independent rows on a chain model
        for bad in (-1, 4):
            with pytest.raises(ValueError):
                host.Gemma("bf16", SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=bad)
        for kw in (dict(max_batch=2), dict(kv_fp8=True), dict(config=dict(SMALL, bounded_local_kv=1))):
            args = dict(config=SMALL, max_seq=MAX_SEQ, max_prefill=16, seed=SEED, draft_tokens=2)
            args.update(kw)
            with pytest.raises(ValueError):
                host.Gemma("bf16", **args)
    finally:
        for x in (plain, zero, three, one):
            x.close()
