"""CPU: the register budget of the quadrant-phase screening GEMM, read from the built library.

screen_gemm_qp2_kernel is designed for two waves per SIMD with no scratch: 256 VGPRs per lane and
a private segment of 0 bytes (a spill reload inside the K-loop waits for the whole operand stream,
DESIGN section 4). This reads the gfx950 code objects out of libebert.so's fat binary and the
kernels' metadata notes with llvm-readelf (metadata only, no instruction text) and asserts both for
every instantiation: store / filter / pool x f16 / bf16 x even / odd K-tile count, and the four
zero-C filter instantiations."""
import os
import re
import struct
import subprocess

from robot_ebert_amd import _lib

READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
KEY_RX = re.compile(r"^    \.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_count|"
                    r"agpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\S+)\s*$")


def _gfx950_code_objects(path):
    """The device ELF images of every offload bundle in the library (one per .hip file)."""
    blob = open(path, "rb").read()
    at = blob.find(MAGIC)
    while at >= 0:
        (entries,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(entries):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def _kernels(elf_path):
    """{kernel name: {key: int}} from the amdhsa.kernels metadata note of one code object."""
    out = subprocess.run([READELF, "--notes", elf_path], check=True, capture_output=True,
                         text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        if line.startswith("  - ."):          # first key of the next kernel's map
            cur = {}
            line = "    " + line[4:]
        m = KEY_RX.match(line)
        if m and cur is not None:
            if m.group(1) == "name":
                kernels[m.group(2)] = cur
            else:
                cur[m.group(1)] = int(m.group(2))
    return kernels


def test_qp2_kernels_have_no_scratch_and_two_waves_per_simd(tmp_path):
    _lib.load()
    assert os.path.exists(READELF), READELF
    qp2 = {}
    for i, image in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        elf = tmp_path / f"co{i}.elf"
        elf.write_bytes(image)
        for name, k in _kernels(str(elf)).items():
            if "screen_gemm_qp2_kernel" in name:
                qp2[name] = k
    # template arguments <BF16, EPI, ODD, ZC> as mangled: Lb.ELi.ELb.ELb.E
    args = {re.search(r"ILb([01])ELi([012])ELb([01])ELb([01])E", n).groups() for n in qp2}
    want = {(bf, epi, odd, "0") for bf in "01" for epi in "012" for odd in "01"}
    want |= {(bf, "1", odd, "1") for bf in "01" for odd in "01"}
    assert args == want and len(qp2) == len(want), sorted(qp2)
    for name, k in sorted(qp2.items()):
        print(name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, (name, k)
