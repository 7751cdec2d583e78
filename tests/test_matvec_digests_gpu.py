"""Bit-identity of the decode Linear (matvec_kernel in csrc/matvec.hip, matvec_rows_kernel in csrc/matvec_rows.hip) with the build tests/golden/matvec_digests.json was recorded
from (tools/record_matvec_digests.py): every case of tests/matvec_digest_cases.py -- plain with bias, norm prologue, sandwich tail + GeGLU, fp32 logits with the
sampler's partials and a one-workgroup grid, in three weight formats, through the one-row entries and through matvec_rows at 2 .. 4 rows -- leaves the same bytes behind.
test_matvec_rows_gpu.py says that the rows entry agrees with the one-row entry; this one says that both still compute what they computed when the fixture was recorded.

The fixture names the `hipcc --version` it was recorded under; a failure under another compiler says so in its message."""
import functools
import json
import os

import pytest

import matvec_digest_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matvec_digests.json")


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_exactly_the_cases():      # (no GPU: a stale fixture shows in the CPU run)
    assert sorted(_golden()["digests"]) == sorted(cases.NAMES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.NAMES)
def test_matvec_outputs_keep_the_recorded_bits(name):
    g = _golden()
    got = cases.run(name)
    if got != g["digests"][name]:
        other = cases.toolchain() != g["toolchain"]
        pytest.fail("%s: the output bytes differ from the recorded build's%s" % (name, " (this build's compiler is not the one the fixture names)" if other else ""))
