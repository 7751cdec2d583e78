"""Bit-identity of the wave-per-position decode kernels (attn_decode_kernel, attn_decode_kvfp8_kernel) with the build tests/golden/attn_decode_digests.json was recorded
from (tools/record_attn_decode_digests.py): every case of tests/attn_decode_digest_cases.py -- every launch-index class at every length on both caches, the <512, 4>
instantiation, the device-position entries, the fused prologue with its appended rows, the one-pass tail, the partials, the warm blocks, the ring -- leaves the same
bytes behind.  The float64 parity tests bound the error of these kernels; this one says that a change meant to keep their arithmetic kept it.

Code generation may contract or reorder floating-point expressions differently under another compiler: the fixture names the `hipcc --version` it was recorded under,
and under any other the test skips."""
import functools
import json
import os

import pytest

import attn_decode_digest_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_decode_digests.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, cases.toolchain()


def test_the_fixture_covers_exactly_the_cases():
    assert sorted(_golden()[0]["digests"]) == sorted(cases.NAMES)


@pytest.mark.parametrize("name", cases.NAMES)
def test_decode_outputs_keep_the_recorded_bits(name):
    g, toolchain = _golden()
    if toolchain != g["toolchain"]:
        pytest.skip("the digests were recorded under another compiler: %r, this build's is %r" % (g["toolchain"].splitlines()[:1], toolchain.splitlines()[:1]))
    assert cases.run(name) == g["digests"][name], "%s: the output bytes differ from the recorded build's" % name
