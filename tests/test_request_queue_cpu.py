"""CPU-only: the scheduling rule of GemmaModel::serveRequests (Mila/RequestQueue.h) driven without a device -- tests/cpp/request_queue.cpp, a stand-alone program with
its own main that includes only that header, compiled with the host compiler and -fsanitize=address,undefined and run directly -- and the Python surface of the queue
(host.GemmaModel.serve_requests: the "n" expansion and its refusals come before any model call)."""
import inspect
import os
import subprocess

import pytest

from mila_amd import build, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_scheduler_alone_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "request_queue.cpp")
    exe = str(tmp_path / "request_queue")
    cmd = [build.HOSTCXX, "-std=c++23", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "mila_amd", "host", "include"), src, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "request queue OK" in r.stdout, r.stdout


def test_the_header_stands_alone():
    """no device call and no project header behind the scheduling rule"""
    text = open(os.path.join(ROOT, "mila_amd", "host", "include", "Mila", "RequestQueue.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert "mila_cdna4_" not in text


class _Unbuilt(host.GemmaModel):
    """serve_requests up to its first use of the model"""
    def __init__(self):
        self.h = None
        self.seen = None

    def vocab_size(self):
        return 1024

    def _row_requests(self, flat, logprobs, who):
        self.seen = (flat, who)
        raise RuntimeError("reached the model")


def test_n_expands_into_consecutive_seeds_before_the_model_is_asked():
    m = _Unbuilt()
    with pytest.raises(RuntimeError, match="reached the model"):
        m.serve_requests([dict(prompt=[1, 2], seed=5, n=3, temperature=0.9), dict(prompt=[3]), dict(prompt=[4], n=1, seed=2), dict(prompt=[9], n=2)])
    flat, who = m.seen
    assert [(q["prompt"], q.get("seed", 0)) for q in flat] == [([1, 2], 5), ([1, 2], 6), ([1, 2], 7), ([3], 0), ([4], 2), ([9], 0), ([9], 1)]
    assert all("n" not in q for q in flat) and flat[0]["temperature"] == 0.9 and "request" in who
    for bad in (0, -1, 1.5, "2", True, None):
        m.seen = None
        with pytest.raises(ValueError, match="request 1: n must be"):
            m.serve_requests([dict(prompt=[1]), dict(prompt=[2], n=bad)])
        assert m.seen is None
    assert "n" not in host.ROW_REQUEST_KEYS      # generate_requests still refuses it as an unknown key
    assert list(inspect.signature(host.GemmaModel.serve_requests).parameters) == ["self", "requests", "logprobs"]
