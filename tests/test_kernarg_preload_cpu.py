"""CPU-only: the captured decode step's kernels are built with kernarg preload (mila_amd/build.py: PRELOAD_FLAGS) and their signatures lead with plain arguments, so the
dispatcher hands them their first addresses in SGPRs.  Read from the kernel descriptors of the gfx950 code objects inside the built libmila_cdna4.so: a by-value struct
in front, or a lost build flag, shows as a preload length of 0."""
import re
import struct

import pytest

from mila_amd import build, capi

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(blob):
    """the gfx950 ELF images of every offload bundle in the library (one bundle per translation unit)"""
    out = []
    for m in re.finditer(re.escape(BUNDLE_MAGIC), blob):
        base = m.start()
        (n,) = struct.unpack_from("<Q", blob, base + 24)
        at = base + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, at)
            triple = blob[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[base + off:base + off + size])
    return out


def _kernel_descriptors(elf):
    """{kernel symbol: (kernarg preload length in dwords, user SGPR count)} of one ELF64 code object, from its <kernel>.kd symbols (64-byte kernel descriptors)"""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2, "not an ELF64 code object (compressed bundle?)"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]      # name type flags addr offset size link info align entsize
    out = {}
    for s in secs:
        if s[1] != 2:      # SHT_SYMTAB
            continue
        strtab = secs[s[6]]
        for j in range(s[5] // 24):
            name_off, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + j * 24)
            end = elf.index(b"\0", strtab[4] + name_off)
            name = elf[strtab[4] + name_off:end].decode()
            if not name.endswith(".kd") or size != 64 or shndx == 0 or shndx >= shnum:
                continue
            sec = secs[shndx]
            kd = elf[sec[4] + value - sec[3]:sec[4] + value - sec[3] + 64]
            rsrc2, = struct.unpack_from("<I", kd, 52)
            preload, = struct.unpack_from("<H", kd, 58)
            out[name[:-3]] = (preload & 0x7F, (rsrc2 >> 1) & 0x1F)
    return out


@pytest.fixture(scope="module")
def descriptors():
    build.build()
    kds = {}
    for elf in _code_objects(open(capi.LIB_PATH, "rb").read()):
        kds.update(_kernel_descriptors(elf))
    assert len(kds) > 100, len(kds)
    return kds


# mangled-name fragments: <length><name> as the Itanium ABI writes a function name inside namespace mila
STEP_KERNELS = ["13matvec_kernel", "18attn_decode_kernel", "23attn_decode_mfma_kernel", "19kv_write_fp8_kernel", "24attn_decode_kvfp8_kernel", "29attn_decode_kvfp8_mfma_kernel",
                "19attn_combine_kernel", "24attn_combine_many_kernel", "27argmax_final_advance_kernel"]


@pytest.mark.parametrize("kernel", STEP_KERNELS)
def test_decode_step_kernels_preload_their_leading_arguments(descriptors, kernel):
    mine = {k: v for k, v in descriptors.items() if k.startswith("_ZN4mila" + kernel)}
    assert mine, kernel
    for name, (preload, user_sgprs) in mine.items():
        assert preload > 0, (name, preload)
        # kernarg pointer (and whatever else the kernel enables) + the preloaded dwords: the hardware has 16 user SGPRs
        assert preload + 2 <= user_sgprs <= 16, (name, preload, user_sgprs)


def test_the_matvec_and_attention_leads_are_whole(descriptors):
    """every instantiation preloads its whole leading block: 11 dwords for the matvecs (W, x, norm_w, res, K, N, workgroups), 14 for the bf16-cache attention (pos_dev, K, V,
    q_raw + six integers), 13 for the fp8-cache attention -- so no first load waits for the kernarg segment"""
    want = {"13matvec_kernel": 11, "18attn_decode_kernel": 14, "23attn_decode_mfma_kernel": 14, "24attn_decode_kvfp8_kernel": 13, "29attn_decode_kvfp8_mfma_kernel": 13,
            "19kv_write_fp8_kernel": 14}
    for kernel, n in want.items():
        got = {k: v[0] for k, v in descriptors.items() if k.startswith("_ZN4mila" + kernel)}
        assert got and set(got.values()) == {n}, (kernel, n, sorted(set(got.values())))
