"""The oracle's Linear compositions with the inner sum done by float64 BLAS: the fast twin of oracle/mila_oracle.c's scalar double loops (orc.linear_bf16w, orc.linear_fp8w,
orc.linear_fp8a_fp8w), so that a test can afford EVERY element of a full prefill shape instead of a handful of rows.  Plain numpy; nothing here touches a GPU.

Why float64 BLAS is a valid stand-in (pinned by tests/test_oracle_kats.py, the C oracle stays the definition):
  * fp8 x fp8: an e4m3 value has 4 significant bits and an exponent in [-9, 8], so a product has <= 8 significant bits with its lowest bit at >= 2^-18 and its
    magnitude <= 448^2 < 2^18; a sum of 15360 of them needs < 18 + 18 + 14 = 50 bits: every partial sum in ANY order is exact in a double.  The matmul equals the
    oracle's loop bit for bit and does not depend on how BLAS blocks K.
  * bf16 x bf16: products are exact (16 bits), the sum is not; BLAS and the oracle differ by summation order at the 2^-53 level, which the oracle's final (float) cast
    hides except at a rounding boundary (one fp32 ulp).

Everything is computed slab by slab over N so that nothing larger than a few hundred MB is alive."""
import numpy as np

SLAB_BYTES = 192 << 20          # float64 weight slab + its output slab stay under this


def bf16_bits_to_f64(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _e4m3_lut():
    """OCP e4m3fn: 1-4-3, bias 7, no infinities, S.1111.111 = NaN (the oracle's orc_e4m3_to_f32; checked against it in test_oracle_kats)"""
    lut = np.empty(256, dtype=np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (8 + m) * 2.0 ** (e - 10)
        lut[c] = -v if c & 0x80 else v
    return lut


E4M3 = _e4m3_lut()


def e4m3_to_f64(q):
    return E4M3[np.asarray(q, dtype=np.uint8)]


def _slabs(N, K, M):
    step = max(128, (SLAB_BYTES // (8 * (K + M))) // 128 * 128)
    for n0 in range(0, N, step):
        yield n0, min(N, n0 + step)


def _matmul(Xd, decode_w, W, col_scale=None, absolute=False):
    """float64 [M, N] = Xd @ decode(W[n0:n1]).T, slab by slab over N; col_scale[n] multiplies the finished sums (one double multiplication, as the oracle's loops do)"""
    M, K = Xd.shape
    N = W.shape[0]
    if absolute:
        Xd = np.abs(Xd)
    out = np.empty((M, N), dtype=np.float64)
    for n0, n1 in _slabs(N, K, M):
        Wd = decode_w(W[n0:n1])
        if absolute:
            Wd = np.abs(Wd)
        np.matmul(Xd, Wd.T, out=out[:, n0:n1])
    if col_scale is not None:
        out *= np.abs(col_scale)[None, :] if absolute else col_scale[None, :]
    return out


def _add_bias(out, bias_bits):
    if bias_bits is not None:
        out += bf16_bits_to_f64(bias_bits)[None, :]
    return out


def _x64(X):
    return np.ascontiguousarray(X, dtype=np.float32).astype(np.float64).reshape(-1, np.shape(X)[-1])


# ---- the oracle's namesakes -------------------------------------------------------------------------------------------------------------------------------------
def linear_bf16w(X, W_bits, bias_bits=None):
    """orc.linear_bf16w in float64: sum_k x[m, k] * bf16(W[n, k]) (+ bias[n])"""
    return _add_bias(_matmul(_x64(X), bf16_bits_to_f64, np.asarray(W_bits, dtype=np.uint16)), bias_bits)


def dequant_fp8_bf16_bits(q, s):
    """bf16 bits of the dequantized weight, e4m3(q) * s[n] in fp32 then RNE: what the W8A16 staging pass writes (orc.to_bf16_bits(orc.dequant_fp8(q, s)))"""
    w = (E4M3[np.asarray(q, dtype=np.uint8)].astype(np.float32) * np.asarray(s, dtype=np.float32)[:, None]).astype(np.float32)
    u = w.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def linear_fp8w(X, q, s, bias_bits=None, staged=False):
    """W8A16.  staged = False: the decode form, orc.linear_fp8w: scale[n] applied once after the sum.  staged = True: the prefill form, the bf16 GEMM on
    bf16(dequantized weight) (orc.linear_bf16w(X, orc.to_bf16_bits(orc.dequant_fp8(q, s))))"""
    q = np.asarray(q, dtype=np.uint8)
    if staged:
        return linear_bf16w(X, dequant_fp8_bf16_bits(q, s), bias_bits)
    return _add_bias(_matmul(_x64(X), e4m3_to_f64, q, np.asarray(s, dtype=np.float32).astype(np.float64)), bias_bits)


def linear_fp8a_fp8w(Xq, ts, Wq, w_row_scale=None, w_tensor_scale=1.0, bias_bits=None):
    """orc.linear_fp8a_fp8w in float64: (sum_k e4m3(Xq) e4m3(Wq)) * ws * ts[m] (+ bias[n]), ws = w_row_scale[n] or w_tensor_scale; the sum is exact, the two scale
    multiplications round in the oracle's order"""
    Xd = e4m3_to_f64(Xq)
    Wq = np.asarray(Wq, dtype=np.uint8)
    if w_row_scale is not None:
        ws = np.asarray(w_row_scale, dtype=np.float32).astype(np.float64)
    else:
        ws = np.full(Wq.shape[0], np.float64(np.float32(w_tensor_scale)))
    out = _matmul(Xd, e4m3_to_f64, Wq, ws)
    out *= np.asarray(ts, dtype=np.float32).astype(np.float64)[:, None]
    return _add_bias(out, bias_bits)


# ---- the magnitude an accumulation error is measured against ----------------------------------------------------------------------------------------------------
def _operand_f64(kind, X, W, scales):
    """(Xd, decode, W, col_scale, row_scale) of one of the three forms above"""
    if kind == "bf16":
        return _x64(X), bf16_bits_to_f64, np.asarray(W, dtype=np.uint16), None, None
    if kind == "fp8w":
        return _x64(X), e4m3_to_f64, np.asarray(W, dtype=np.uint8), np.asarray(scales[0], dtype=np.float64), None
    if kind == "fp8a_fp8w":
        ts, ws = scales
        N = np.shape(W)[0]
        ws = np.full(N, float(ws)) if np.ndim(ws) == 0 else np.asarray(ws, dtype=np.float64)
        return e4m3_to_f64(X), e4m3_to_f64, np.asarray(W, dtype=np.uint8), ws, np.asarray(ts, dtype=np.float64)
    raise ValueError(kind)


def abs_products(kind, X, W, scales=(), at=None):
    """sum_k |x[m, k] w[n, k]| times the |scales| of the form `kind` ("bf16": X float, W bf16 bits; "fp8w": X float, W e4m3, scales = (s[N],); "fp8a_fp8w": X e4m3,
    W e4m3, scales = (ts[M], ws[N] or a scalar)): the size of the terms a GEMM sums, from which the slack for its fp32 accumulation is taken.
    at = None: the whole [M, N] matrix (a second matmul).  at = (m_idx, n_idx): only those elements, as a vector -- what a comparison needs once it knows which few
    elements are in question."""
    Xd, dec, Wc, cs, rs = _operand_f64(kind, X, W, scales)
    if at is None:
        out = _matmul(Xd, dec, Wc, cs, absolute=True)
        if rs is not None:
            out *= np.abs(rs)[:, None]
        return out
    m_idx, n_idx = (np.asarray(a, dtype=np.int64) for a in at)
    out = np.empty(m_idx.size, dtype=np.float64)
    Xa = np.abs(Xd)
    K = Xd.shape[1]
    step = max(1, (64 << 20) // (8 * K))
    for i in range(0, m_idx.size, step):
        mi, ni = m_idx[i:i + step], n_idx[i:i + step]
        out[i:i + step] = np.einsum("ik,ik->i", Xa[mi], np.abs(dec(Wc[ni])))
    if cs is not None:
        out *= np.abs(cs)[n_idx]
    if rs is not None:
        out *= np.abs(rs)[m_idx]
    return out
