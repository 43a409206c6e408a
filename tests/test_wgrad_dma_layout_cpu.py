"""The LDS-DMA piece mapping of wgrad8_kernel, checked on the host: tests/wgrad_dma_layout_check.cpp includes the kernel's own index header
(protopformer_amd/csrc/gemm_layout.h), is built with the host compiler under AddressSanitizer + UBSan as a stand-alone program, and walks every
piece of both tile widths and every source / destination address of the shapes tests/test_gpu_wgrad_dma.py runs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_wgrad_dma_layout(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "wgrad_dma_layout_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "protopformer_amd", "csrc"),
            os.path.join(ROOT, "tests", "wgrad_dma_layout_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                        # a host compiler without the sanitizer runtimes: the checks themselves do not need them
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "wgrad DMA layout: ok" in run.stdout
    assert run.stdout.count("K tiles checked") == 4          # the K % 64 != 0 case has no DMA addresses to check
    # pick_splitk / k_slice: non-empty, disjoint, 64-aligned slices that cover [0, K) for K = 8 .. 4096 and every (M, N) of test_gpu_gemm_paths.py
    assert "K slicing:" in run.stdout and "FAIL" not in run.stdout
