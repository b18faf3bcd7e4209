"""Register and scratch budget of the stage kernels, read from the metadata of the shipped build's final ISA.

The fp32 stage kernels run at the occupancy their launch shapes are sized for: a change that costs a kernel
a wave per SIMD, or that makes it spill, loses more than any prefetch depth returns.  So every kernel keeps at least the
occupancy its VGPR count gave it before the closing convs got their deeper weight rings, and no kernel uses scratch --
dec_s1, which spilled 12 B per lane at the 128-VGPR cap, included.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "lyra_amd", "csrc")

# kernel -> (VGPRs before the deeper rings, scratch bytes per lane allowed now)
BUDGET = {
    "enc_s0_kernel": (124, 0),
    "enc_s1_kernel": (77, 0),
    "enc_s2_xn_kernel": (96, 0),
    "dec_s0_xn_kernel": (110, 0),
    "dec_s1_kernel": (128, 0),
    "dec_s2_kernel": (120, 0),
    "rvq_encode_kernel": (114, 0),   # 106 + 8 accumulation registers
    # the side kernels whose bodies are the device functions of resample_pass.h, logmel_stages.h, span_noise_scan.h and
    # cng_frame.h: the VGPRs each had while those bodies were text included into it
    "resample_kernel": (99, 0),
    "resample_rates_kernel": (105, 0),
    "resample_streams_kernel": (64, 0),
    "resample_streams_out_kernel": (101, 0),
    "span_resample_kernel": (97, 0),
    "span_resample_rates_kernel": (99, 0),
    "span_resample_packed_kernel": (99, 0),
    "ds_splice_kernel": (61, 0),
    "ds_splice_streams_kernel": (69, 0),
    "logmel_kernel": (62, 0),
    "logmel_masked_kernel": (62, 0),
    "logmel_rates_kernel": (68, 0),
    "logmel_streams_kernel": (68, 0),
    "span_logmel_kernel": (57, 0),
    "span_logmel_map_kernel": (57, 0),
    "span_logmel_rates_kernel": (57, 0),
    "span_noise_scan_kernel": (101, 0),
    "span_noise_scan_rates_kernel": (101, 0),
    "span_lossy_scan_kernel": (105, 0),
    "cng_kernel": (68, 0),
    "span_cng_kernel": (96, 0),
    "lossy_mix_kernel": (21, 0),
}


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def kernel_metadata(path):
    """{kernel: (vgpr_count, private_segment_fixed_size)} from the amdhsa.kernels notes of one .s file."""
    out = {}
    txt = open(path).read()
    for blk in re.split(r"\n\s+- \.agpr_count:", txt)[1:]:
        blk = blk.split("amdhsa.target")[0]
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN4lyra\d+([a-z0-9_]+_kernel)E", name)
        out[m.group(1) if m else name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                                          int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    return out


@pytest.fixture(scope="module")
def metadata():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    r = subprocess.run(["make", "-C", CSRC, "-j4", "ODIR=obj_asm", "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = os.path.join(CSRC, "obj_asm")
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".s"):
            out.update(kernel_metadata(os.path.join(d, f)))
    return out


def test_the_expected_kernels_were_found(metadata):
    missing = sorted(set(BUDGET) - set(metadata))
    assert not missing, f"not in the build's metadata: {missing} (found {sorted(metadata)})"


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_occupancy_and_scratch_budget(metadata, kernel):
    assert kernel in metadata, f"{kernel} not in the build's metadata"
    vgprs, scratch = metadata[kernel]
    parent_vgprs, scratch_allowed = BUDGET[kernel]
    print(f"{kernel}: {vgprs} VGPRs ({waves_per_simd(vgprs)} waves/SIMD; before: {parent_vgprs} = "
          f"{waves_per_simd(parent_vgprs)}), scratch {scratch} B")
    assert waves_per_simd(vgprs) >= waves_per_simd(parent_vgprs)
    assert scratch <= scratch_allowed


def test_the_occupancy_rule():
    assert [waves_per_simd(v) for v in (128, 124, 104, 96, 80, 77, 64)] == [4, 4, 4, 5, 6, 6, 8]
