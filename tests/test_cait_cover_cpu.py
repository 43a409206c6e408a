"""CPU-side checks of the talking-heads cover: there is one path, the retired fallback entry points are gone from the header and the
library, and a shape the kernels do not cover is refused by name (cait.require_th_cover) from the two host predicates alone."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
RETIRED = ["ppf_th_scores", "ppf_th_dwl", "ppf_th_softmax_mix", "ppf_th_softmax_bwd", "ppf_gemm_bf16_batched"]
COVERED = [(4, 196, 192), (2, 16, 96)]                 # cait_xxs24; the micro fixture


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    return ctypes.CDLL(build(verbose=False))


def test_retired_entry_points_are_gone(lib):
    declared = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in RETIRED:
        assert not re.search(r"\b" + name + r"\b", declared), f"{name} is still declared in ppf_hip.h"
        assert not hasattr(lib, name), f"{name} is still exported by the library"


def test_ops_has_no_switch_and_no_batched_gemm():
    from protopformer_amd import ops
    src = inspect.getsource(ops)
    assert "PPF_TH_FUSED" not in src and "gemm_batched" not in src


@pytest.mark.parametrize("H,N,D", COVERED)
def test_registered_shapes_are_covered(lib, H, N, D):
    from protopformer_amd.cait import require_th_cover
    assert lib.ppf_th_fused_supported(H, N, D) == 1 and lib.ppf_th_grads_supported(H, N, D) == 1
    require_th_cover(H, N, D, training=False)
    require_th_cover(H, N, D, training=True)


@pytest.mark.parametrize("H,N,D,training", [(4, 196, 256, False), (4, 196, 256, True),      # K + V images of 4 x 64-wide heads: 196 KiB
                                            (8, 196, 384, False), (8, 196, 384, True),      # cait_s24's eight heads
                                            (4, 210, 192, True)])                           # th_grads stops at 208 tokens
def test_uncovered_shape_is_refused_by_name(H, N, D, training):
    from protopformer_amd.cait import require_th_cover
    with pytest.raises(ValueError) as e:
        require_th_cover(H, N, D, training=training)
    msg = str(e.value)
    assert f"H={H}" in msg and f"N={N}" in msg and f"D={D}" in msg
    assert "32, 48 or 64" in msg and "2 or 4 heads" in msg and "160 KiB" in msg and "208" in msg and "224" in msg


def test_inference_is_covered_up_to_224_tokens():
    from protopformer_amd.cait import require_th_cover
    require_th_cover(4, 210, 192, training=False)
