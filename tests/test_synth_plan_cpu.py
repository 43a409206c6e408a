"""What the PartsWorld kernels and the host share, checked on the host: tests/synth_plan_check.cpp includes the kernels' own header
(protopformer_amd/csrc/synth_plan.h), is built with the host compiler under AddressSanitizer + UBSan as a stand-alone program, and checks
the scene table's layout, the class-table rule, the object and slot geometry at the extreme draws of every frame side, the four shapes
and the spec rules."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_synth_plan(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "synth_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "protopformer_amd", "csrc"),
            os.path.join(ROOT, "tests", "synth_plan_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                        # a host compiler without the sanitizer runtimes: the checks themselves do not need them
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "synth plan: ok" in run.stdout


def test_python_mirrors_the_plan():
    """data.py mirrors the header's constants by hand: the ones a mismatch of which no referee-against-kernel test on a GPU would be
    needed to find."""
    import re
    from protopformer_amd import _lib, data as D
    src = open(os.path.join(ROOT, "protopformer_amd", "csrc", "synth_plan.h")).read()

    def const(name):
        return int(re.search(r"\b" + name + r"\s*=\s*(0x[0-9A-Fa-f]+|\d+)u?\s*[;,]", src).group(1), 0)
    assert D.SYNTH_WORDS == _lib.DEFINES["PPF_SYNTH_WORDS"] == const("SYNTH_WORDS")
    assert (D.SYNTH_STREAM_SCENE, D.SYNTH_STREAM_NOISE) == (const("SYNTH_STREAM_SCENE"), const("SYNTH_STREAM_NOISE"))
    assert (D.SYNTH_ITEM_PART0, D.SYNTH_ITEM_DIST0, D.SYNTH_ITEM_NODE0) == (const("SYNTH_ITEM_PART0"), const("SYNTH_ITEM_DIST0"), const("SYNTH_ITEM_NODE0"))
    assert 0xC0000000 < D.SYNTH_STREAM_SCENE < D.SYNTH_STREAM_NOISE <= 0xFFFFFFFF
    assert D.SYNTH_PART0 + 8 * D.SYNTH_PRIM_WORDS == D.SYNTH_DIST0 and D.SYNTH_DIST0 + 8 * D.SYNTH_PRIM_WORDS == D.SYNTH_NODE0
    assert D.SYNTH_NODE0 + 81 <= D.SYNTH_WORDS
    cells = int(re.search(r"0x([0-9A-Fa-f]{8})u >> \(4 \* k\)", src).group(1), 16)
    assert tuple((cells >> (4 * k)) & 15 for k in range(8)) == D.SYNTH_SLOT_CELLS
