"""Record tests/golden/matvec_digests.json: the SHA-256 of the output bytes of every case of tests/matvec_digest_cases.py on the GPU, and the `hipcc --version`
text of the compiler that built the library.  tests/test_matvec_digests_gpu.py holds every later build to these digests, so run this from a build whose decode
Linear kernels are the ones to preserve -- BEFORE a refactor of them, never after it.
    python tools/record_matvec_digests.py [--out FILE]"""
import os
os.environ.setdefault("MILA_CDNA4_TUNING", "1")      # (the one-workgroup cases run under a tuning)
import argparse
import json
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matvec_digest_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "matvec_digests.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_matvec_digests: no GPU")
    toolchain = cases.toolchain()
    if not toolchain:
        raise SystemExit("record_matvec_digests: cannot run hipcc --version")
    digests = {name: cases.run(name) for name in cases.NAMES}
    with open(a.out, "w") as f:
        json.dump({"toolchain": toolchain, "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d digests -> %s" % (len(digests), a.out))


if __name__ == "__main__":
    main()
