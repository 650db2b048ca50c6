"""Static check of the log-probability kernel (CPU: hipcc cross-compiles, nothing runs): its
resource metadata shows no scratch.  The kernel keeps a whole row's keys in 64 VGPRs per thread
at 1024 threads per workgroup (128 VGPRs at most); a pass that lets the compiler keep per-entry
values live across passes or rounds spills."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_token_logprobs_kernel_has_no_scratch(tmp_path):
    from distributed_llms_amd.csrc.build import kernel_flags
    src = ROOT / "distributed_llms_amd" / "csrc" / "kernels" / "sampler.hip"
    out = tmp_path / "sampler.s"
    subprocess.run([HIPCC, *kernel_flags(str(src)), "--offload-device-only", "-S", str(src), f"-I{src.parent}",
                    "-o", str(out)], check=True, capture_output=True, timeout=900)
    s = out.read_text()
    names = re.findall(r"^\s*\.amdhsa_kernel (\w*token_logprobs_kernel\w*)", s, re.M)
    assert len(names) == 1, names
    meta = s[s.index(".amdhsa_kernel " + names[0]):]
    meta = meta[: meta.index(".end_amdhsa_kernel")]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    # the same from the code object's metadata, with the register budget of a 1024-thread workgroup
    entries = re.split(r"\n  - \.", s[s.index("amdhsa.kernels:"):])
    entry = [e for e in entries if re.search(r"\.name:\s+" + names[0] + r"\s", e)]
    assert len(entry) == 1
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry[0]).group(1)) == 0
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry[0]).group(1)) == 0
    assert int(re.search(r"\.vgpr_count:\s*(\d+)", entry[0]).group(1)) <= 128
