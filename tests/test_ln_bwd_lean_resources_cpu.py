"""The register budget of the lean LayerNorm backward kernel, from the compiler's own report: csrc/layernorm.hip compiled for the device with
build.py's flags plus -Rpass-analysis=kernel-resource-usage.  ln_bwd2_kernel<4, 3, false, true> (D = 384, no LayerScale) runs beside the
weight-gradient kernel of the side stream, whose resident workgroup leaves 192 VGPRs per SIMD lane and 64 KiB of a CU's LDS: two waves per
SIMD of the lean form fit only within 96 VGPRs, and two of its workgroups only within 8 KiB of LDS each; AGPRs or scratch would undo the point."""
import os
import re
import subprocess

import pytest

from protopformer_amd import build as ppf_build

SRC = os.path.join(ppf_build.SRC, "layernorm.hip")
LEAN = "ln_bwd2_kernelILi4ELi3ELb0ELb1EE"            # <V = 4, NJ = 3, LS = false, LEAN = true> in the mangled name
PARENT = "ln_bwd2_kernelILi4ELi3ELb0ELb0EE"


def _report(tmp_path):
    r = subprocess.run([ppf_build.HIPCC] + ppf_build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC,
                        "-o", str(tmp_path / "layernorm.dev.o")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


@pytest.mark.skipif(not os.path.exists(ppf_build.HIPCC), reason="no hipcc: the resource report needs the device compiler")
def test_lean_ln_bwd_resource_budget(tmp_path):
    rep = _report(tmp_path)
    lean = [v for k, v in rep.items() if LEAN in k]
    parent = [v for k, v in rep.items() if PARENT in k]
    assert len(lean) == 1 and len(parent) == 1, f"instantiations found: {[k for k in rep if 'ln_bwd2_kernelILi4ELi3' in k]}"
    lean, parent = lean[0], parent[0]
    print("lean:", lean)
    print("parent:", parent)
    assert int(lean["VGPRs"]) <= 96, lean
    assert int(lean["AGPRs"]) == 0, lean
    assert int(lean["ScratchSize"]) == 0 and int(lean["VGPRs Spill"]) == 0 and int(lean["SGPRs Spill"]) == 0, lean
    assert lean["Dynamic Stack"] == "False", lean
    assert int(lean["TotalSGPRs"]) <= 80, lean
    assert int(lean["LDS Size"]) <= 8192, lean
