"""The host's share of ppf_resize_crop_u8, checked on the host: tests/device_data_plan_check.cpp includes the kernels' own header
(protopformer_amd/csrc/device_data_plan.h), is built with the host compiler under AddressSanitizer + UBSan as a stand-alone program,
checks the plan validation and the workspace layout, and prints the integer taps of a table of cases, which are compared here with the
numpy referee data.resample_taps (held to Pillow by tests/test_device_data_cpu.py)."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_device_data_plan(tmp_path):
    from protopformer_amd import data as D
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "device_data_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "protopformer_amd", "csrc"),
            "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "device_data_plan_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                        # a host compiler without the sanitizer runtimes: the checks themselves do not need them
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "device data plan: ok" in run.stdout
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("taps ")]
    assert len(lines) == 2 * (5 * 16 + 12 + 256)
    cache = {}
    for ln in lines:
        head, tail = ln[5:].split(" : ")
        filt, size, in0, in1, out, xx = head.split()
        key = (int(filt), int(size), float(in0), float(in1), int(out))
        if key not in cache:
            cache[key] = D.resample_taps(key[1], key[2], key[3], key[4], 0, key[4], filter=key[0])
        xmin, k = cache[key][int(xx)]
        got = [int(v) for v in tail.split()]
        assert got[0] == xmin and np.array_equal(got[1:], k), ln
