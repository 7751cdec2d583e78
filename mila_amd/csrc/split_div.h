// Exact unsigned division by a launch constant without a divide: decode attention cuts its live band into `splits` chunks of ceil(band / splits) positions, and that
// quotient stands between the arrival of the position word and the first K/V request.  The host computes (mul, shift) once per launch, the kernel does one 32 x 32 -> high
// 32 multiply and a shift.  Plain C++ (no HIP header): tests/test_split_div_cpu.py compiles it into a stand-alone program that checks every quotient.
//
// For d >= 2 let s = ceil(log2 d) - 1 (so 2^s < d <= 2^(s+1)) and m = ceil(2^(32+s) / d).  Then m <= 2^31 for a power of two and m < 2^32 otherwise, and with
// e = m d - 2^(32+s) (0 <= e < d <= 2^(s+1)):  n m / 2^(32+s) = n / d + n e / (d 2^(32+s)), and the error term is below 1 / d whenever n e < 2^(32+s), which holds for
// every n < 2^31.  So floor(n m / 2^(32+s)) == floor(n / d) for all 0 <= n < 2^31.  d == 1 has no such m below 2^32: mul == 0 marks it and the quotient is n itself.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MILA_SPLIT_DIV_FN __host__ __device__ inline
#else
#define MILA_SPLIT_DIV_FN inline
#endif

namespace mila {

struct SplitDiv
{
    uint32_t mul;       // 0: the divisor is 1
    uint32_t shift;
};

MILA_SPLIT_DIV_FN SplitDiv split_div_make(uint32_t d)
{
    if (d <= 1u) return SplitDiv{0u, 0u};
    uint32_t s = 0;
    while ((2u << s) < d) ++s;                                  // 2^s < d <= 2^(s+1)
    const uint64_t p = (uint64_t)1 << (32 + s);
    return SplitDiv{(uint32_t)((p + d - 1) / d), s};
}

// floor(n / d) for the d of split_div_make, 0 <= n < 2^31
MILA_SPLIT_DIV_FN uint32_t split_div(uint32_t n, SplitDiv c)
{
    const uint32_t hi = (uint32_t)(((uint64_t)n * c.mul) >> 32);      // one s_mul_hi_u32 on the device
    return c.mul ? hi >> c.shift : n;
}

}  // namespace mila
