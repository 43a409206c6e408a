"""CPU-side checks of the prototype bank: the ppf_proto_topk_merge entry point is declared, exported and bound with one parameter
list; its shape validation answers before any device call; patch_box and the JSON report give known answers."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
NAMES = ("ppf_proto_topk_merge", "ppf_proto_topk_init")


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppf_hip.h"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert name in _lib.SIGS and len(_lib.SIGS[name]) == nargs


def _merge(lib, B=4, P=5, K=10, Dp=8, k=9):
    """Call the entry point with its real argument types and pointers that are never dereferenced on a rejected shape."""
    from protopformer_amd import _lib
    fn = getattr(lib, "ppf_proto_topk_merge")
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS["ppf_proto_topk_merge"]]
    d = 4096                                                    # an aligned non-null address
    return fn(d, d, d, k, d, (1 + k) * Dp, 1, Dp, d, d, 2, B, P, K, d, d, d, d, None)


@pytest.mark.parametrize("kw,word", [(dict(K=65), "K=65"), (dict(K=0), "K=0"), (dict(B=0), "B=0"), (dict(B=1025), "B=1025"), (dict(Dp=6), "Dp=6"),
                                     (dict(P=0), "P=0")])
def test_shape_validation_without_device(lib, kw, word):
    rc = _merge(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert rc == -1, f"{kw}: rc={rc}"                           # PPF_ERR_SHAPE
    assert "ppf_proto_topk_merge" in msg and word in msg, msg


def test_abi_version_unchanged(lib):
    from protopformer_amd import _lib
    assert lib.ppf_abi_version() == 10 == _lib.EXPECTED_ABI       # additions only: no existing entry point changed


def test_patch_box_known_answers():
    from protopformer_amd.interpret import patch_box
    assert patch_box(0, 14, 16) == (0, 0, 16, 16)
    assert patch_box(195, 14, 16) == (13 * 16, 13 * 16, 14 * 16, 14 * 16)
    assert patch_box(15, 14, 16) == (16, 16, 32, 32)              # row 1, column 1
    assert patch_box(13, 14, 16) == (208, 0, 224, 16)             # row 0, column 13: (x0, y0, x1, y1)
    with pytest.raises(ValueError):
        patch_box(196, 14, 16)
    with pytest.raises(ValueError):
        patch_box(-1, 14, 16)


def _hand_made_result():
    inf = np.float32(-np.inf)
    local = dict(values=np.array([[3.5, 1.25], [2.0, inf], [inf, inf], [0.5, 0.25]], dtype=np.float32),
                 image_ids=np.array([[7, 3], [11, -1], [-1, -1], [3, 7]], dtype=np.int32),
                 grid_pos=np.array([[0, 195], [14, -1], [-1, -1], [27, 1]], dtype=np.int32), filled=np.array([2, 1, 0, 2], dtype=np.int32))
    glob = dict(values=np.array([[9.0, 8.0], [inf, inf]], dtype=np.float32), image_ids=np.array([[3, 7], [-1, -1]], dtype=np.int32),
                grid_pos=np.full((2, 2), -1, dtype=np.int32), filled=np.array([2, 0], dtype=np.int32))
    return {"local": local, "global": glob}


def test_json_report_keys_and_values(tmp_path):
    from protopformer_amd.bank import write_bank
    index = {3: ("/data/a.jpg", 0), 7: ("/data/b.jpg", 0), 11: ("/data/c.jpg", 0)}
    npz, js = write_bank(str(tmp_path), _hand_made_result(), index, {"local": 2, "global": 1}, 14, 16)
    assert os.path.basename(npz) == "prototype_bank.npz" and os.path.basename(js) == "prototype_bank.json"
    doc = json.load(open(js))
    assert set(doc) == {"topk", "side", "patch_size", "prototypes"} and doc["topk"] == 2 and doc["side"] == 14 and doc["patch_size"] == 16
    protos = doc["prototypes"]
    assert [(p["branch"], p["prototype"], p["class"]) for p in protos] == [("local", 0, 0), ("local", 1, 0), ("local", 2, 1), ("local", 3, 1),
                                                                          ("global", 0, 0), ("global", 1, 1)]
    for p in protos:
        assert set(p) == {"branch", "prototype", "class", "entries"}
        for r, e in enumerate(p["entries"]):
            assert set(e) == {"rank", "image_id", "image", "label", "activation", "grid_row", "grid_col", "box"} and e["rank"] == r
    assert [len(p["entries"]) for p in protos] == [2, 1, 0, 2, 2, 0]                  # unfilled slots are not listed
    e = protos[0]["entries"][1]
    assert e == dict(rank=1, image_id=3, image="/data/a.jpg", label=0, activation=1.25, grid_row=13, grid_col=13, box=[208, 208, 224, 224])
    e = protos[1]["entries"][0]
    assert (e["grid_row"], e["grid_col"], e["box"]) == (1, 0, [0, 16, 16, 32])
    g = protos[4]["entries"][0]
    assert g["grid_row"] is None and g["grid_col"] is None and g["box"] is None and g["activation"] == 9.0 and g["image"] == "/data/a.jpg"
    z = np.load(npz)
    assert set(z.files) == {f"{b}_{k}" for b in ("local", "global") for k in ("values", "image_ids", "grid_pos", "filled")}
    assert np.array_equal(z["local_image_ids"], _hand_made_result()["local"]["image_ids"])


def test_tool_parser_extends_the_training_parser():
    from protopformer_amd.bank import get_args_parser
    a = get_args_parser().parse_args(["--data_set", "CUB2011U", "--resume", "x.pth", "--topk", "3", "--all-classes", "--gallery", "--project",
                                      "--save-projected", "p.pth", "--split", "test", "--prototype_shape", "400", "64", "1", "1"])
    assert (a.resume, a.topk, a.all_classes, a.gallery, a.project, a.save_projected, a.split) == ("x.pth", 3, True, True, True, "p.pth", "test")
    assert a.prototype_shape == [400, 64, 1, 1] and a.base_architecture == "deit_tiny_patch16_224"
