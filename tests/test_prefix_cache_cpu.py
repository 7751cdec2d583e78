"""CPU-only: the prefix-reuse rule of GemmaModel::serveRequests (Mila/PrefixCache.h) driven without a device -- tests/cpp/prefix_cache.cpp, a stand-alone program with its
own main that includes only that header, compiled with the host compiler and -fsanitize=address,undefined and run directly: a shadow cache per row (cell p = a hash of
tokens[0 .. p]) under a fixed-seed schedule of admissions, steps, retirements and aborted admissions, and the named cases of the rule."""
import os
import subprocess

from mila_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_alone_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "prefix_cache.cpp")
    exe = str(tmp_path / "prefix_cache")
    cmd = [build.HOSTCXX, "-std=c++23", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "mila_amd", "host", "include"), src, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "prefix cache OK" in r.stdout, r.stdout


def test_the_header_stands_alone():
    """no device call and no project header behind the rule"""
    text = open(os.path.join(ROOT, "mila_amd", "host", "include", "Mila", "PrefixCache.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") for i in includes), includes
    assert "mila_cdna4_" not in text
