"""What the compiled scan_kernel<D> must keep, read from the listing (CPU only: hipcc cross-compiles).  scan.hip is compiled as
msk144cudecoder_amd/build.py compiles it; for D = 1..8 the kernel's metadata must show
  * at most 80 VGPRs: three 8-wave workgroups per CU are six waves per SIMD, 512 / 6 = 85 registers, allocated in eights;
  * no scratch;
  * at most 53 248 B of LDS (160 KB / 3), so that three workgroups fit a CU.
The moves and add-zero forms of scan_kernel<6> are counted and reported, not asserted: they are what a diet of the listing is
judged by (before the correlation was written in two-float vectors: 232 v_mov_b32 + 15 v_pk_mov_b32 and 33 additions of zero)."""
import os
import re
import subprocess
import tempfile

import pytest

from msk144cudecoder_amd import build as B

MAX_VGPRS = 80
MAX_LDS_BYTES = 53248


@pytest.fixture(scope="module")
def listing():
    extra = next(e for s, e in B.SOURCES if s == "scan.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "scan.s")
        cmd = [B._hipcc()] + [f for f in B.COMMON if f != "-fPIC"] + list(extra) + ["-I", B._CSRC, "--cuda-device-only", "-S", os.path.join(B._CSRC, "scan.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        return open(out).read()


def kernel_metadata(text):
    """{D: dict(vgprs, scratch, lds)} from the amdhsa.kernels metadata of every scan_kernel<D>."""
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"scan_kernelILi(\d+)E", name)
        if not m:
            continue
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
        out[int(m.group(1))] = dict(vgprs=field("vgpr_count"), scratch=field("private_segment_fixed_size"), lds=field("group_segment_fixed_size"),
                                    spills=field("vgpr_spill_count") + field("sgpr_spill_count"))
    return out


def kernel_body(text, depth):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*scan_kernelILi%dE\w*:" % depth, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def test_every_depth_keeps_three_workgroups_per_cu(listing):
    meta = kernel_metadata(listing)
    assert sorted(meta) == list(range(1, 9)), sorted(meta)
    for depth, m in sorted(meta.items()):
        print("scan_kernel<%d>:" % depth, m)
        assert m["vgprs"] <= MAX_VGPRS, (depth, m)
        assert m["scratch"] == 0 and m["spills"] == 0, (depth, m)
        assert m["lds"] <= MAX_LDS_BYTES, (depth, m)


def test_report_moves_and_zero_adds_of_depth_6(listing, record_property):
    body = kernel_body(listing, 6)
    ops = [re.match(r"\s+([a-z_0-9]+)", l).group(1) for l in body if re.match(r"\s+[a-z]", l)]
    moves = sum(op.startswith("v_mov_b32") for op in ops)
    pk_moves = sum(op.startswith("v_pk_mov_b32") for op in ops)
    zero_adds = sum(1 for l in body if re.match(r"\s+v_(pk_)?add_f32(_e\d+)?\s+v[\d\[\]:]+,\s*(0,\s*v|v[\d\[\]:]+,\s*0\b)", l))
    valu = sum(op.startswith("v_") for op in ops)
    print("scan_kernel<6>: %d VALU instructions, v_mov_b32 %d, v_pk_mov_b32 %d, add-zero forms %d" % (valu, moves, pk_moves, zero_adds))
    for key, value in (("valu", valu), ("v_mov_b32", moves), ("v_pk_mov_b32", pk_moves), ("add_zero", zero_adds)):
        record_property("scan_kernel_6_" + key, value)
    assert valu > 0
