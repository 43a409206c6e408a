"""The scene-edit rule of ppf_synth_edit, checked on the host: tests/synth_edit_check.cpp includes the kernel's own header
(protopformer_amd/csrc/synth_plan.h), is built with the host compiler under AddressSanitizer + UBSan as a stand-alone program, and holds
the word-by-word rule to a naive second implementation over every op, every part and distractor, every mask and the invalid cases."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_synth_edit_rule(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "synth_edit_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "protopformer_amd", "csrc"),
            os.path.join(ROOT, "tests", "synth_edit_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                        # a host compiler without the sanitizer runtimes: the checks themselves do not need them
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "synth edit: ok" in run.stdout


def test_python_mirrors_the_edit_ops():
    """data.py mirrors the op numbers by hand."""
    import re
    from protopformer_amd import data as D
    src = open(os.path.join(ROOT, "protopformer_amd", "csrc", "synth_plan.h")).read()

    def const(name):
        return int(re.search(r"\b" + name + r"\s*=\s*(\d+)\s*[;,]", src).group(1))
    assert (D.EDIT_COPY, D.EDIT_PARTS_OFF, D.EDIT_DISTRACTORS_OFF, D.EDIT_BACKGROUND, D.EDIT_PART_ATTR) == tuple(
        const("SYNTH_EDIT_" + n) for n in ("COPY", "PARTS_OFF", "DISTRACTORS_OFF", "BACKGROUND", "PART_ATTR"))
