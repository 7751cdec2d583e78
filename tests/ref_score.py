"""The oracle composition of prompt scoring: every position's log-probabilities, from RefGemma's public pieces (embed, block, rms, linear( .., round_out=False )) and a
float64 log-softmax of the capped logits.  The head is the decode head's arithmetic at every row (round_out=False: fp32 logits, an e4m3 table summed first and scaled
after), which is the contract of the scoring lm_head."""
import numpy as np

from test_token_logprobs_gpu import BAR as BAR_LOGPROB

SOFTCAP = 30.0      # GemmaConfig::final_logit_softcapping of the synthetic models


def oracle_scores(ref, tokens, max_seq, softcap=SOFTCAP):
    """(log-probabilities [T, V] float64, raw logits [T, V]) of `tokens` prefilled at position 0 through the oracle `ref`"""
    x = ref.embed(np.asarray(tokens, dtype=np.int64))
    for L in ref.layers:
        x = ref.block(x, L, 0, max_seq)
    normed = ref.rms(x, ref.final_norm)
    logits = np.asarray(ref.linear(normed, ref.table, round_out=False), dtype=np.float64)
    z = softcap * np.tanh(logits / softcap) if softcap > 0 else logits
    m = z.max(axis=1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(axis=1, keepdims=True)), logits


def logprob_bar(logit_bar, logits, softcap=SOFTCAP):
    """softcap and log-sum-exp are 1-Lipschitz in the max norm: logits within logit_bar * max |logit| of the oracle's move z_t and log S by at most that much each"""
    return 2.0 * logit_bar * float(np.abs(logits).max()) + BAR_LOGPROB[softcap]


def clear_rows(ref_lp, bound):
    """rows whose two most probable tokens are more than `bound` apart in the oracle: only there is the argmax decided"""
    top2 = np.partition(ref_lp, ref_lp.shape[1] - 2, axis=1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]) > bound
