"""CPU-only: the prefix-reuse rule with a valid-from bound (Mila/PrefixCache.h, RINGS) driven without a device -- tests/cpp/prefix_cache_ring.cpp, a stand-alone program
with its own main that includes only that header, compiled with the host compiler and -fsanitize=address,undefined and run directly: per row a flat shadow cache and a
ring of (position, hash) cells at window 8 and capacities 11, 16 and 23, under a fixed-seed schedule of admissions, band forks, chunked suffix prefills, steps (the stale
write of rows that are not live included), retirements, aborted admissions and rewinds; the named cases of the rule; the 0 / 0 geometry against the flat rule; and one
run with the bound off that must see stale cells."""
import os
import subprocess

from mila_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_ring_rule_alone_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "prefix_cache_ring.cpp")
    exe = str(tmp_path / "prefix_cache_ring")
    cmd = [build.HOSTCXX, "-std=c++23", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "mila_amd", "host", "include"), src, "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "prefix cache ring OK" in r.stdout, r.stdout
