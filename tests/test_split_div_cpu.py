"""csrc/split_div.h: the multiply-shift that replaces decode attention's (band + splits - 1) / splits.  The header is plain C++, so a small stand-alone host program
(no GPU, no HIP) compares split_div with the machine's own division: exhaustively for every numerator below 2^22 + 256 -- a band of four million keys, 128 times the
largest band bucket any test here decodes -- at every divisor the wave-per-position kernel is launched with (1 .. 64 splits; 65 .. 256 below 2^16 only), and on a coarse
sweep with the neighbours of multiples up to 2^31 - 1, the range the header's proof covers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCXX = os.environ.get("HOSTCXX", "/opt/rocm/lib/llvm/bin/clang++")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "split_div.h"
int main()
{
    using namespace mila;
    for (uint32_t d = 1; d <= 256; ++d)
    {
        const SplitDiv c = split_div_make(d);
        if (d > 1 && c.mul == 0) { std::printf("d=%u: no multiplier\n", d); return 1; }
        for (uint32_t n = 0; n < (d <= 64 ? (1u << 22) + 256u : (1u << 16)); ++n)
            if (split_div(n, c) != n / d) { std::printf("d=%u n=%u: %u != %u\n", d, n, split_div(n, c), n / d); return 1; }
        // up to 2^31 - 1: a coarse sweep, and the three numerators around every 4099th multiple of d
        for (uint64_t n = 0; n < (1ull << 31); n += 65521)
            if (split_div((uint32_t)n, c) != (uint32_t)n / d) { std::printf("d=%u n=%llu\n", d, (unsigned long long)n); return 1; }
        for (uint64_t m = 1; m * d < (1ull << 31); m += 4099)
            for (int k = -1; k <= 1; ++k)
            {
                const uint64_t n = m * d + k;
                if (n < (1ull << 31) && split_div((uint32_t)n, c) != (uint32_t)n / d) { std::printf("d=%u n=%llu\n", d, (unsigned long long)n); return 1; }
            }
        const uint32_t top = 0x7fffffffu;
        for (uint32_t n = top - 1024; n <= top && n >= top - 1024; ++n)
        {
            if (split_div(n, c) != n / d) { std::printf("d=%u n=%u\n", d, n); return 1; }
            if (n == top) break;
        }
    }
    std::printf("split_div OK\n");
    return 0;
}
"""


def test_split_div_equals_the_division_for_every_band_and_split_count(tmp_path):
    src = tmp_path / "split_div_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "split_div_check"
    subprocess.check_call([HOSTCXX, "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "mila_amd", "csrc"), str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "split_div OK", p.stdout
