"""The launch rule of the C-ABI library, checked on its sources: kernels are launched and copies enqueued only through the helpers of
csrc/ppf_launch.h, so every launch gets its dynamic-LDS opt-in and its error check, and an armed ppf_stream_wait_stream never waits on a
kernel that is no longer its stream's last operation."""
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "protopformer_amd", "csrc")
ALLOWED = {"ppf_launch.h"}
RAW = ("hipFuncSetAttribute", "hipMemsetAsync", "hipMemcpyAsync", "hipMemcpy2DAsync", "<<<", "hipLaunchKernelGGL", "PPF_LAUNCH_CHECK")


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 14 and ALLOWED <= {os.path.basename(f) for f in files}
    return {os.path.basename(f): open(f).read() for f in files}


def test_raw_launch_plumbing_only_in_the_launch_header():
    bad = [(name, word) for name, text in _sources().items() if name not in ALLOWED for word in RAW if word in text]
    assert not bad, f"raw runtime calls outside ppf_launch.h (use ppf_launch / ppf_memset_async / ppf_memcpy*_async): {bad}"


def test_helpers_wrap_each_raw_call():
    text = _sources()["ppf_launch.h"]
    for word in RAW[:4]:
        assert text.count(word + "(") == 1, word
    assert text.count("<<<") == 1


def test_cu_count_queried_in_one_place():
    assert sum(text.count("hipDeviceAttributeMultiprocessorCount") for text in _sources().values()) == 1


def test_no_per_site_attribute_flags_left():
    assert not [name for name, text in _sources().items() if "static bool attr_set" in text or "attr_lds" in text]
