"""Static checks of the decode attention kernel's chunk loads in the compiled gfx950 code (CPU: hipcc
cross-compiles, nothing runs).

The decode wave loads every KV chunk with buffer loads whose descriptors end behind the admissible rows
(attention.hip load_chunk_rows), so a partly filled last block costs only its keys' bytes.  That only pays
while the depth-2 chunk pipeline stays intact, and three forms of it did not compile that way: lane offsets
hoisted out of the chunk loop spilled, a descriptor word computed on the VALU put a waterfall loop round
every load, and a separate tail loader behind a wave-uniform branch drained vmcnt(0) before its loads."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def decode_kernels(tmp_path_factory):
    from distributed_llms_amd.csrc.build import kernel_flags
    src = ROOT / "distributed_llms_amd" / "csrc" / "kernels" / "attention.hip"
    out = tmp_path_factory.mktemp("asm") / "attn.s"
    subprocess.run([HIPCC, *kernel_flags(str(src)), "--offload-device-only", "-S", str(src), f"-I{src.parent}",
                    "-o", str(out)], check=True, capture_output=True, timeout=900)
    s = out.read_text()
    kernels = []
    for name in re.findall(r"^(_ZN4dllm18attn_decode_kernel\w+):", s, re.M):
        start = s.index(name + ":")
        kernels.append((name, s[start: s.index(".Lfunc_end", start)], s[s.index(".amdhsa_kernel " + name):][:4000]))
    assert len(kernels) >= 30
    return kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_decode_kernels_keep_two_waves_per_simd(decode_kernels):
    """No scratch, and at most 256 registers (VGPRs + AGPRs of the unified file: 512 per SIMD lane over the
    two waves the launch bounds ask for)."""
    for name, _, meta in decode_kernels:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 256, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_chunk_loads_are_straight_runs_of_buffer_loads(decode_kernels):
    """Every chunk load site (three per kernel: the first chunk, the next one, the one after) is one run of
    2 * D/32 + D/16 nontemporal 16-byte buffer loads in one basic block -- no waterfall loop round a load
    (s_and_saveexec), no branch, and no vmcnt(0) inside the run (the scheduler may interleave the previous
    chunk's MFMAs and their counted waits) or in the instructions leading up to it; the constants of the
    fragments sit in the immediate offsets (one lane-offset register for K, one for V^T)."""
    for name, body, _ in decode_kernels:
        d = int(re.search(r"attn_decode_kernelILi(\d+)E", name).group(1))
        per_site = 2 * (d // 32) + d // 16
        lines = [l.strip() for l in body.split("\n") if l.strip() and not l.strip().startswith(";")]
        idx = [i for i, l in enumerate(lines) if l.startswith("buffer_load_dwordx4")]
        assert len(idx) == 3 * per_site, (name, len(idx))
        assert all(" nt" in lines[i] and "offen" in lines[i] for i in idx), name
        for site in range(3):
            run = idx[site * per_site: (site + 1) * per_site]
            between = lines[run[0]: run[-1] + 1]
            assert not [l for l in between if "vmcnt(0)" in l or l.startswith(("s_cbranch", "s_and_saveexec"))
                        or l.startswith(".LBB")], (name, site)
            lead = lines[max(0, run[0] - 24): run[0]]
            assert not [l for l in lead if "vmcnt(0)" in l], (name, site, "drain ahead of the chunk loads")
            assert len({l.split(",")[1].strip() for l in between if l.startswith("buffer_load")}) <= 3, (name, site)
