"""CPU-side checks of the device interpretability path: the ppf_act_* entry points are declared, exported and bound with the argument
types the wrappers pass; their shape validation answers before any device call; the host path of the consistency score is what it was;
the helper that picks the percentile's two ranks agrees with numpy."""
import ctypes
import inspect
import os
import types

import numpy as np
import pytest
import torch

from protopformer_amd import interpret as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> the spec the wrappers in ops.py pass (p pointer, i int32, s stream appended by _lib.call)
SPECS = {"ppf_act_upsample": "ppiiis", "ppf_act_peak": "piiipppiiips", "ppf_act_part_table": "piipiiips", "ppf_act_order_stats": "piiiiips",
         "ppf_act_box": "ppiiips"}


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(SPECS))
def test_entry_points_declared_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    assert _lib.SIGS.get(name) == SPECS[name], f"{name}: parsed from include/ppf_hip.h as {_lib.SIGS.get(name)}"
    assert _lib._RESTYPE[name] is ctypes.c_int
    assert hasattr(lib, name), f"{name} is not exported by the built library"


def test_abi_number_is_the_parent_s(lib):
    """Additions only: by the header's rule the number moves when an entry point changes its parameter list or meaning."""
    from protopformer_amd import _lib
    assert lib.ppf_abi_version() == _lib.EXPECTED_ABI == 10


def _call(lib, name, *args):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn(*args, None), lib.ppf_last_error().decode()


D = 4096          # an aligned non-null address, never dereferenced on a rejected shape


@pytest.mark.parametrize("name,args,word", [
    ("ppf_act_upsample", (D, D, 3, 14, 0), "S=0"), ("ppf_act_upsample", (D, D, 3, 0, 224), "g=0"), ("ppf_act_upsample", (D, D, 0, 14, 224), "M=0"),
    ("ppf_act_upsample", (D, D, 3, 65, 224), "g=65"), ("ppf_act_upsample", (D, D, 3, 14, 1025), "S=1025"),
    ("ppf_act_upsample", (D, D, 3, 64, 1024), "LDS"),
    ("ppf_act_peak", (D, 3, 14, -1, D, D, None, 0, 0, 0, None), "S=-1"),
    ("ppf_act_peak", (D, 30, 14, 224, D, D, D, 7, 15, 36, D), "maps_per_img=7"),
    ("ppf_act_part_table", (D, 30, 224, D, 10, 0, 36, D), "n_parts=0"),
    ("ppf_act_order_stats", (D, 3, 0, 224, 0, 1, D), "g=0"), ("ppf_act_box", (D, D, 3, 14, 0, D), "S=0")])
def test_shape_validation_without_device(lib, name, args, word):
    rc, msg = _call(lib, name, *args)
    assert rc == -1, f"{name}{args}: rc={rc} ({msg})"                 # PPF_ERR_SHAPE
    assert name in msg and word in msg, msg


@pytest.mark.parametrize("name,args,word", [("ppf_act_order_stats", (D, 3, 14, 224, 5, 7, D), "k_lo=5 k_hi=7"),
                                            ("ppf_act_order_stats", (D, 3, 14, 224, 50175, 50176, D), "k_hi=50176"),
                                            ("ppf_act_peak", (D, 30, 14, 224, D, D, D, 10, 15, 36, None), "both"),
                                            ("ppf_act_part_table", (D, 30, 224, D, 10, 15, -1, D), "half_size=-1")])
def test_argument_validation_without_device(lib, name, args, word):
    rc, msg = _call(lib, name, *args)
    assert rc == -3 and name in msg and word in msg, (rc, msg)      # PPF_ERR_ARG


def test_wrappers_refuse_host_tensors_with_the_shape_error():
    for fn in (I.upsample_cubic_device, I.activation_peaks, I.high_activation_boxes):
        with pytest.raises(RuntimeError, match=r"rc=-1.*CUDA"):
            fn(torch.zeros(2, 4, 4), 8)
        with pytest.raises(RuntimeError, match=r"rc=-1.*CUDA"):
            fn(np.zeros((2, 4, 4), dtype=np.float32), 8)


def test_new_names_and_keyword_defaults():
    for name in ("upsample_cubic_device", "activation_peaks", "high_activation_boxes"):
        assert callable(getattr(I, name))
    assert inspect.signature(I.high_activation_boxes).parameters["percentile"].default == 95
    for fn in (I.consistency_score, I.consistency_from_outputs):
        prm = inspect.signature(fn).parameters
        assert prm["device"].default is False and list(prm)[-1] == "device"      # appended: positional callers are unaffected
    from protopformer_amd import ops
    for name in ("act_upsample", "act_peak", "act_part_table", "act_order_stats", "act_box"):
        assert callable(getattr(ops, name))


def test_host_path_without_the_keyword_is_what_it_was():
    """consistency_from_outputs without device= on the golden inputs: the stored score, flags and fractions, and a numpy grid."""
    import mini_trees as M
    z = np.load(os.path.join(ROOT, "tests", "golden", "interp_consistency.npz"))
    locs = {}
    for i, pid, x, y in z["parts_locs"].tolist():
        locs.setdefault(i, []).append([pid, x, y])
    sizes = {int(i): M.cub_size(int(i)) for i in z["ids"]}
    score, effects, max_parts, grid = I.consistency_from_outputs(z["attn"], z["acts"], z["targets"], z["ids"], types.SimpleNamespace(id_to_part_loc=locs),
                                                                 sizes, int(z["k"]), int(z["img_size"]), int(z["targets"].max()) + 1)
    assert score == pytest.approx(float(z["score"]), abs=1e-12) and effects == z["class_proto_effect"].tolist()
    assert np.allclose(max_parts, z["class_max_part"], atol=1e-12)
    assert isinstance(grid, np.ndarray) and np.array_equal(grid, z["grid_acts"])


@pytest.mark.parametrize("n", [25, 49, 196, 50176])
@pytest.mark.parametrize("percentile", [0, 5, 37.5, 50, 95, 99.9, 100])
def test_percentile_ranks_reproduce_numpy(n, percentile):
    """np.percentile of the two selected order statistics at the returned fraction equals np.percentile of all n values."""
    a = np.random.default_rng(n).random(n).astype(np.float32)
    a[: n // 3] = a[0]                                             # a run of equal values
    lo, hi, frac = I.percentile_ranks(n, percentile)
    assert 0 <= lo <= hi <= min(lo + 1, n - 1) and 0.0 <= frac <= 1.0
    s = np.sort(a)
    pair = np.array([s[lo], s[hi]], dtype=np.float32)
    thr, want = np.percentile(pair, frac * 100.0), np.percentile(a, percentile)
    assert np.array_equal(a >= thr, a >= want), (lo, hi, frac, float(thr), float(want))
