"""Static check of the multi-LoRA kernels (CPU: hipcc cross-compiles, nothing runs): both compile
for gfx950 and their resource metadata shows no scratch and no spills."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNELS = ("lora_shrink_kernel", "lora_expand_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lora_kernels_have_no_scratch(tmp_path):
    from distributed_llms_amd.csrc.build import kernel_flags
    src = ROOT / "distributed_llms_amd" / "csrc" / "kernels" / "lora.hip"
    out = tmp_path / "lora.s"
    subprocess.run([HIPCC, *kernel_flags(str(src)), "--offload-device-only", "-S", str(src), f"-I{src.parent}",
                    "-o", str(out)], check=True, capture_output=True, timeout=900)
    s = out.read_text()
    assert "v_mfma_f32_16x16x32_bf16" in s
    entries = re.split(r"\n  - \.", s[s.index("amdhsa.kernels:"):])
    for kernel in KERNELS:
        names = re.findall(r"^\s*\.amdhsa_kernel (\w*" + kernel + r"\w*)", s, re.M)
        assert len(names) == 1, (kernel, names)
        meta = s[s.index(".amdhsa_kernel " + names[0]):]
        meta = meta[: meta.index(".end_amdhsa_kernel")]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, kernel
        entry = [e for e in entries if re.search(r"\.name:\s+" + names[0] + r"\s", e)]
        assert len(entry) == 1, kernel
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", entry[0]).group(1)) == 0, kernel
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", entry[0]).group(1)) == 0, kernel
        assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", entry[0]).group(1)) == 0, kernel
