"""The radix pipeline of the stochastic sampler (sample_radix_fp32 / _bf16 / _advance_fp32) against the restated reference semantics (oracle/mila_oracle.c:
orc_sample_stochastic) and against the 16-ary search pipeline it stands beside (sample_stochastic_*).  Integer output: a token is right or wrong.  A draw is held
to the oracle when it is decisive by the rule tests/test_ops_gpu.py uses for the first pipeline: the top-k cut is not a near tie (margin 0 > 1e-6) and the CDF bracket
of the chosen token is not within 2e-3 of the total of flipping (a nucleus-boundary flip moves the total by one boundary token's probability, far below that)."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
from gpu_util import dev_f32, dev_i32, dev_u16, host
from mila_amd import capi

pytestmark = pytest.mark.gpu

DRAWS = [0.0, 0.999999] + [(i + 0.5) / 23.0 for i in range(23)]
CASES = [(262144, 30.0, 0.8, 64, 0.95), (262144, 30.0, 0.7, 0, 0.9), (262144, 0.0, 1.0, 40, 1.0), (262144, 30.0, 1.3, 0, 1.0), (50257, 0.0, 0.9, 200, 0.8),
         (4097, 0.0, 0.7, 2048, 0.97), (2049, 30.0, 0.8, 64, 0.95), (1000, 30.0, 0.5, 5, 0.99), (300, 0.0, 1.0, 299, 0.999), (257, 0.0, 1.0, 3, 0.9), (65, 0.0, 1.0, 8, 0.5)]


@functools.lru_cache(maxsize=None)
def _scratch(V, radix):
    import torch
    lib = capi.load()
    nb = lib.mila_cdna4_sample_radix_scratch_bytes(V) if radix else lib.mila_cdna4_sample_stochastic_scratch_bytes(V)
    return torch.empty(nb, dtype=torch.uint8, device="cuda"), nb


class _Sampler:
    """one logits vector on the device, sampled through either pipeline"""

    def __init__(self, logits, bf16=False):
        self.V, self.bf16 = logits.size, bf16
        self.dev = dev_u16(orc.to_bf16_bits(logits)) if bf16 else dev_f32(logits)
        self.tok = dev_i32(np.array([-1]))

    def _run(self, entry, radix, softcap, t, k, p, r):
        scratch, nb = _scratch(self.V, radix)
        self.tok.fill_(-1)
        capi.call(entry + ("_bf16" if self.bf16 else "_fp32"), self.dev, self.tok, self.V, float(softcap), float(t), int(k), float(p), float(r), scratch, C.c_size_t(nb))
        return int(host(self.tok)[0])

    def radix(self, softcap, t, k, p, r):
        return self._run("sample_radix", True, softcap, t, k, p, r)

    def search(self, softcap, t, k, p, r):
        return self._run("sample_stochastic", False, softcap, t, k, p, r)


def _radix(v, softcap, t, k, p, r):
    return _Sampler(np.asarray(v, dtype=np.float32)).radix(softcap, t, k, p, r)


def test_reference_scenarios_through_the_radix_entry():
    """the reference's own expectations (Tests/Dnn/Samplers/Sampling.Cuda.cpp:152-262, :387-401): every scenario of test_stochastic_sampler_reference_scenarios"""
    f = lambda v: np.array(v, dtype=np.float32)
    assert _radix(f([8, 2, 3, 4, 5, 6, 7, 1]), 0, 1.0, 1, 1.0, 0.99) == 0
    assert _radix(f([1, 2, 3, 4, 5, 6, 7, 8]), 0, 1.0, 0, 1.0, 0.0) == 0
    assert _radix(f([1, 2, 3, 4, 5, 6, 7, 8]), 0, 1.0, 0, 1.0, 0.999999) == 7
    two, peak = _Sampler(f([1, 2, 3, 4, 5, 6, 70, 80])), _Sampler(f([0, 0, 0, 0, 0, 0, 0, 20]))
    for i in range(20):
        assert two.radix(0, 1.0, 2, 1.0, i / 20.0) in (6, 7)
        assert peak.radix(0, 1.0, 0, 0.5, i / 20.0) == 7
    V = 262144
    zeros = _Sampler(np.zeros(V, dtype=np.float32))
    assert zeros.radix(0, 1.0, 0, 1.0, 0.0) == 0
    assert zeros.radix(0, 1.0, 0, 1.0, 0.999999) == V - 1
    tie = _Sampler(f([5, 3, 3, 1]))
    assert all(tie.radix(0, 1.0, 2, 1.0, r) == 0 for r in (0.0, 0.5, 0.99))                       # tie across the top-k boundary
    cap = _Sampler(f([1000, 990]))
    assert [cap.radix(30.0, 1.0, 0, 1.0, r) for r in (0.25, 0.75)] == [0, 1]                      # softcap before temperature
    assert [cap.radix(0.0, 1.0, 0, 1.0, r) for r in (0.25, 0.75)] == [0, 0]
    with pytest.raises(capi.InvalidArgument):
        _radix(f([1, 2]), 0, 0.0, 0, 1.0, 0.5)                                                    # temperature <= 0: use the greedy entry


@pytest.mark.parametrize("V", [8, 1000, 262144])
def test_all_equal_logits_with_top_k(V):
    """nothing is strictly above the (k+1)-th largest: no survivor, the walk ends at vocab - 1 -- in the oracle, in the search pipeline and here"""
    lg = np.full(V, 1.5, dtype=np.float32)
    s = _Sampler(lg)
    for r in (0.0, 0.3, 0.999999):
        want = orc.sample_stochastic(lg, 0.0, 1.0, 5, 1.0, r)[0]
        assert s.radix(0.0, 1.0, 5, 1.0, r) == want == s.search(0.0, 1.0, 5, 1.0, r)
    assert s.radix(0.0, 1.0, 5, 0.9, 0.5) == orc.sample_stochastic(lg, 0.0, 1.0, 5, 0.9, 0.5)[0]


def _logits(V, k):
    rng = np.random.default_rng(V + k)
    lg = (rng.standard_normal(V) * 4.0).astype(np.float32)
    lg[rng.integers(0, V, 8)] += 9.0                      # a few strong candidates, like real logits
    return lg


def _sweep(lg, V, softcap, t, k, p, bf16=False):
    s = _Sampler(lg, bf16)
    full = (k == 0 and p >= 1.0)
    if full:
        # untruncated multinomial over the whole vocabulary: every token's probability is ~1e-5, no draw is "decisive"; the reference's own check
        # (Sampling.Cuda.cpp:307-362): the chosen token's CDF bracket contains r * total within a slack
        x = lg.astype(np.float32)
        if softcap > 0:
            x = np.float32(softcap) * np.tanh(x / np.float32(softcap))
        x = (x / np.float32(t)).astype(np.float64)
        e = np.exp(x - x.max())
        cum = np.cumsum(e)
        total, slack = cum[-1], 1e-4 * cum[-1]
    decisive = 0
    for r in DRAWS:
        got = s.radix(softcap, t, k, p, r)
        assert got == s.radix(softcap, t, k, p, r), "r=%g: two launches, two tokens" % r
        assert 0 <= got < V
        if full:
            target = r * total
            assert cum[got] >= target - slack and cum[got] - e[got] <= target + slack, "r=%g: token %d outside its CDF bracket" % (r, got)
            decisive += 1
            continue
        tok, m = orc.sample_stochastic(lg, softcap, t, k, p, r)
        if m[0] > 1e-6 and m[2] > 2e-3:
            assert got == tok, "r=%g: %d != oracle %d (margins %s)" % (r, got, tok, m)
            assert got == s.search(softcap, t, k, p, r), "r=%g: the two pipelines differ on a decisive draw" % r
            decisive += 1
    print("V=%d softcap=%g t=%g k=%d p=%g%s: %d of %d draws decisive" % (V, softcap, t, k, p, " bf16" if bf16 else "", decisive, len(DRAWS)))
    assert decisive >= 12, "too few decisive draws (%d)" % decisive


@pytest.mark.parametrize("V,softcap,t,k,p", CASES)
def test_radix_sampler_matches_the_oracle_and_the_search_pipeline(V, softcap, t, k, p):
    _sweep(_logits(V, k), V, softcap, t, k, p)


@pytest.mark.parametrize("V,softcap,t,k,p", [CASES[1], CASES[9]])
def test_radix_sampler_on_bf16_logits(V, softcap, t, k, p):
    """bf16-rounded logits through sample_radix_bf16.  Eight significant bits make the k-th and (k+1)-th largest of a large vocabulary EQUAL (the oracle's top-k margin is
    0 on the k = 64 / 40 / 200 / 5 cases: no draw is decisive there, whatever the sampler), so the bf16 sweep runs on the full-vocabulary nucleus case and on the
    k = 3 of 257 case, where the oracle alone finds 18 and 23 of the 25 draws decisive."""
    _sweep(orc.from_bf16_bits(orc.to_bf16_bits(_logits(V, k))), V, softcap, t, k, p, bf16=True)


@pytest.mark.parametrize("V,softcap,t,k,p", [(262144, 30.0, 0.8, 64, 0.95), (1000, 30.0, 0.5, 5, 0.99), (65, 0.0, 1.0, 0, 1.0)])
def test_the_advance_form_draws_from_the_ring_bumps_and_publishes(V, softcap, t, k, p):
    import torch
    lg = _logits(V, k)
    s = _Sampler(lg)
    scratch, _ = _scratch(V, True)
    ILLEGAL = 2.0
    r1, r2 = 0.37, 0.81
    want1, want2 = s.radix(softcap, t, k, p, r1), s.radix(softcap, t, k, p, r2)
    tok, pos = dev_i32(np.array([-1])), dev_i32(np.array([41]))
    seq = torch.tensor([6], dtype=torch.int64, device="cuda")
    ring = torch.zeros(8, dtype=torch.int64, device="cuda")
    draws = torch.full((8,), ILLEGAL, dtype=torch.float32, device="cuda")
    draws[7] = r1                                         # sample number 7 reads slot 7 % 8
    capi.sample_radix_advance(s.dev, tok, softcap, t, k, p, draws, scratch, pos, seq, ring)
    assert int(host(tok)[0]) == want1 and int(host(pos)[0]) == 42 and int(seq.item()) == 7
    assert int(ring[7].item()) == (7 << 32) | want1
    assert int(ring.abs().sum().item()) == int(ring[7].item())                                    # the other slots are untouched
    draws.fill_(ILLEGAL)
    draws[0] = r2                                         # the second call takes the next slot: 8 % 8
    capi.sample_radix_advance(s.dev, tok, softcap, t, k, p, draws, scratch, pos, seq, ring)
    assert int(host(tok)[0]) == want2 and int(host(pos)[0]) == 43 and int(seq.item()) == 8
    assert int(ring[0].item()) == (8 << 32) | want2 and int(ring[7].item()) == (7 << 32) | want1
    assert int(ring[1:7].abs().sum().item()) == 0
    # without a ring: token, position and sequence number only
    draws.fill_(ILLEGAL)
    draws[1] = r1
    before = ring.clone()
    tok.fill_(-1)
    capi.sample_radix_advance(s.dev, tok, softcap, t, k, p, draws, scratch, pos, seq, None)
    assert int(host(tok)[0]) == want1 and int(host(pos)[0]) == 44 and int(seq.item()) == 9
    assert torch.equal(ring, before)
    with pytest.raises(capi.InvalidArgument):
        capi.sample_radix_advance(s.dev, tok, softcap, t, k, p, draws, scratch, pos, None, None)  # the draw slot follows the sequence counter
