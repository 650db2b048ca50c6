"""Static check of the split-context prefill kernel (CPU: hipcc cross-compiles, nothing runs): every
instantiation (head_dim 64 / 128, GQA group 1..16, one or two tiles per wave) compiles for gfx950
without scratch and without spills.  A wave keeps two K/V chunks, its q fragments and NT accumulator
tiles in registers; an epilogue that indexes the tiles at run time would push them to scratch."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_prefill_split_kernel_has_no_scratch(tmp_path):
    from distributed_llms_amd.csrc.build import kernel_flags
    src = ROOT / "distributed_llms_amd" / "csrc" / "kernels" / "attention.hip"
    out = tmp_path / "attention.s"
    subprocess.run([HIPCC, *kernel_flags(str(src)), "--offload-device-only", "-S", str(src), f"-I{src.parent}",
                    "-o", str(out)], check=True, capture_output=True, timeout=1800)
    s = out.read_text()
    names = re.findall(r"^\s*\.amdhsa_kernel (\w*attn_prefill_split_kernel\w*)", s, re.M)
    assert len(names) == 2 * 5 * 2, names
    entries = re.split(r"\n  - \.", s[s.index("amdhsa.kernels:"):])
    for name in names:
        meta = s[s.index(".amdhsa_kernel " + name):]
        meta = meta[: meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, name
        entry = [e for e in entries if re.search(r"\.name:\s+" + name + r"\s", e)]
        assert len(entry) == 1, name
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry[0]).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry[0]).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", entry[0]).group(1)) == 0, name
