"""CPU-side checks of the spatial-alignment pass: ppf_col2im_patch_f32, ppf_grad_box_mass and ppf_pgd_step_box are declared, exported
and bound with one parameter list each and answer their limits through the error channel before any device call; the numpy referees
(interpret.box_mass_host / gradient_locality / pgd_step_box with device=False) agree with a brute-force loop; the attack's constants, the
summary and the tool's parser give known answers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_col2im_patch_f32": "ppiiiiis", "ppf_grad_box_mass": "ppiiiippps", "ppf_pgd_step_box": "ppppppppfiiiis"}


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(SPECS))
def test_declared_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppf_hip.h"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == len(SPECS[name]) and _lib.SIGS[name] == SPECS[name]
    assert lib.ppf_abi_version() == _lib.EXPECTED_ABI               # additions: no existing entry point changed


def _fn(lib, name):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn


D = 4096                                                              # an aligned non-null address, never dereferenced on a rejected call


def _col2im(lib, cols=D, img=D, B=2, C=3, H=32, W=48, patch=16):
    return _fn(lib, "ppf_col2im_patch_f32")(cols, img, B, C, H, W, patch, None)


def _mass(lib, g=D, box=D, R=5, C=3, H=20, W=28, inside=D, total=D):
    return _fn(lib, "ppf_grad_box_mass")(g, box, R, C, H, W, inside, total, None, None)


def _step(lib, x=D, box=D, alpha=D, direction=-1.0, R=5, C=3, H=20, W=28):
    return _fn(lib, "ppf_pgd_step_box")(x, D, D, box, alpha, D, D, D, direction, R, C, H, W, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_col2im, dict(B=0), -1, "B=0"), (_col2im, dict(H=40), -1, "H=40"), (_col2im, dict(W=40), -1, "W=40"), (_col2im, dict(patch=0), -1, "patch=0"),
    (_col2im, dict(cols=None), -3, "cols"), (_col2im, dict(img=None), -3, "img"),
    (_mass, dict(R=0), -1, "R=0"), (_mass, dict(C=0), -1, "C=0"), (_mass, dict(C=4, H=32768, W=32768), -1, "H=32768"), (_mass, dict(g=None), -3, "g,"),
    (_mass, dict(box=None), -3, "box"), (_mass, dict(total=None), -3, "total"), (_mass, dict(box=D + 4), -2, "box"),
    (_step, dict(R=0), -1, "R=0"), (_step, dict(W=0), -1, "W=0"), (_step, dict(direction=0.5), -3, "dir=0.5"), (_step, dict(x=None), -3, "x,"),
    (_step, dict(alpha=None), -3, "alpha3"), (_step, dict(box=D + 8), -2, "box")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_"), msg


# ------------------------------------------------------------------------------------------------ the numpy referees
def _case(seed=0, R=2, C=3, H=8, W=12):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((R, C, H, W)).astype(np.float32)
    g[0, 0, 0, 0], g[0, 1, 3, 5], g[1, 2, 7, 11], g[1, 0, 2, 2], g[0, 2, 4, 4] = np.nan, np.inf, -np.inf, 0.0, -0.0
    x0 = rng.uniform(-1.75, 2.2, g.shape).astype(np.float32)          # valid pixels (lo <= -1.80, hi >= 2.24), some within eps of lo / hi
    x = (x0 + rng.uniform(-0.2, 0.2, g.shape)).astype(np.float32)
    boxes = np.array([[2, 7, 3, 10], [0, 8, 11, 12]], dtype=np.int32)
    return g, x, x0, boxes


def test_box_mass_referee_agrees_with_a_loop():
    from protopformer_amd.interpret import box_mass_host, gradient_locality
    g, _, _, boxes = _case()
    inside, total, bad = box_mass_host(g, boxes)
    assert inside.dtype == total.dtype == np.float64 and bad.dtype == np.int32 and bad.tolist() == [2, 1]
    for r in range(2):
        ti = tt = 0.0
        for c in range(3):
            for y in range(8):
                for x in range(12):
                    v = float(g[r, c, y, x])
                    if not np.isfinite(v):
                        continue
                    tt += abs(v)
                    if boxes[r, 0] <= y < boxes[r, 1] and boxes[r, 2] <= x < boxes[r, 3]:
                        ti += abs(v)
        assert abs(inside[r] - ti) <= 288 * 2.0 ** -52 * ti and abs(total[r] - tt) <= 288 * 2.0 ** -52 * tt
    i2, t2, share = gradient_locality(g, boxes, device=False)
    assert np.array_equal(i2, inside) and np.array_equal(t2, total) and np.array_equal(share, inside / total)
    z = gradient_locality(np.zeros_like(g), boxes, device=False)
    assert (z[1] == 0).all() and np.isnan(z[2]).all()
    e = gradient_locality(g, np.array([[3, 3, 0, 12], [-5, 99, -5, 99]], dtype=np.int32), device=False)     # empty; larger than the image
    assert e[0][0] == 0 and e[2][0] == 0 and e[0][1] == e[1][1] and e[2][1] == 1


@pytest.mark.parametrize("direction", [1, -1])
def test_pgd_step_referee_agrees_with_a_loop(direction):
    from protopformer_amd.interpret import attack_bounds, pgd_step_box
    g, x, x0, boxes = _case(seed=1)
    a, e, lo, hi = attack_bounds(8 / 255, None, 10)
    got = pgd_step_box(x, x0, g, boxes, a, e, lo, hi, direction, device=False)
    assert got.dtype == np.float32 and got.shape == x.shape
    f = np.float32
    for r in range(2):
        for c in range(3):
            for y in range(8):
                for xx in range(12):
                    if boxes[r, 0] <= y < boxes[r, 1] and boxes[r, 2] <= xx < boxes[r, 3]:
                        want = x0[r, c, y, xx]
                    else:
                        v = g[r, c, y, xx]
                        s = f(1) if v > 0 else f(-1) if v < 0 else f(0)
                        moved = f(x[r, c, y, xx] + f(f(direction) * a[c]) * s)
                        lower, upper = max(f(x0[r, c, y, xx] - e[c]), lo[c]), min(f(x0[r, c, y, xx] + e[c]), hi[c])
                        want = min(max(moved, lower), upper)
                    assert got[r, c, y, xx].view(np.int32) == f(want).view(np.int32), (r, c, y, xx)
    out = np.abs(got.astype(np.float64) - x0)                        # x0 +- eps is rounded once: half an ulp of a value below 4
    assert (out <= e.reshape(1, 3, 1, 1) + 2.0 ** -23).all() and (got >= lo.reshape(1, 3, 1, 1)).all() and (got <= hi.reshape(1, 3, 1, 1)).all()
    with pytest.raises(ValueError, match="direction"):
        pgd_step_box(x, x0, g, boxes, a, e, lo, hi, 0, device=False)


def test_attack_constants():
    from protopformer_amd.data import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
    from protopformer_amd.interpret import attack_bounds
    a, e, lo, hi = attack_bounds(8 / 255, None, 10)
    std, mean = np.asarray(IMAGENET_DEFAULT_STD), np.asarray(IMAGENET_DEFAULT_MEAN)
    assert all(v.dtype == np.float32 and v.shape == (3,) for v in (a, e, lo, hi))
    assert np.array_equal(e, (8 / 255 / std).astype(np.float32)) and np.array_equal(a, (2.5 * (8 / 255) / 10 / std).astype(np.float32))
    assert np.array_equal(lo, (-mean / std).astype(np.float32)) and np.array_equal(hi, ((1 - mean) / std).astype(np.float32))
    assert np.array_equal(attack_bounds(8 / 255, 1 / 255, 3)[0], (1 / 255 / std).astype(np.float32))
    for bad in (dict(eps=-1.0, alpha=None, steps=3), dict(eps=0.1, alpha=None, steps=0)):
        with pytest.raises(ValueError, match="misalignment_attack"):
            attack_bounds(**bad)


def test_boxes_around_a_peak_are_clipped_and_half_open():
    from protopformer_amd.interpret import _boxes_host
    assert _boxes_host(np.array([[0, 63], [30, 30], [5, 60]]), 36, 64).tolist() == [[0, 36, 27, 64], [0, 64, 0, 64], [0, 41, 24, 64]]
    assert _boxes_host(np.array([[100, 120]]), 36, 224).tolist() == [[64, 136, 84, 156]]


def test_summary_leaves_nan_rows_out_of_their_mean():
    import torch
    from protopformer_amd.interpret import ALIGNMENT_STATS, alignment_summary
    assert ALIGNMENT_STATS == ("share", "area", "pac", "plc", "left_box")
    nan = float("nan")
    stats = torch.tensor([[0.5, 0.25, 0.5, 4.0, 1.0], [nan, 0.25, 0.0, 0.0, 0.0], [0.25, 0.5, nan, nan, nan]], dtype=torch.float64)
    s = alignment_summary(torch.tensor([7, 2, 7], dtype=torch.int32), stats)
    assert s["rows"] == 3 and s["overall"] == dict(mean_share=0.375, mean_area=1 / 3, mean_pac=0.25, mean_plc=2.0, mean_left_box=0.5,
                                                   share_over_area=0.375 / (1 / 3))
    assert list(s["per_prototype"]) == [2, 7] and s["per_prototype"][7] == dict(mean_share=0.375, mean_area=0.375, mean_pac=0.5, mean_plc=4.0,
                                                                                mean_left_box=1.0, share_over_area=1.0, rows=2)
    assert np.isnan(s["per_prototype"][2]["mean_share"]) and s["per_prototype"][2]["rows"] == 1


def test_regroup_gives_the_same_passes_for_every_loader_batch_size():
    import torch
    from protopformer_amd.tooling import regroup, take_images
    x = torch.arange(7.0).reshape(7, 1)
    for bs in (1, 2, 3, 7):                                # composed as spatial_alignment composes it
        loader = [(x[i:i + bs], None) for i in range(0, 7, bs)]
        passes = [p.cpu().reshape(-1).tolist() for p, in regroup(((v.float(),) for v, in take_images(((b[0],) for b in loader), 0)), 4)]
        assert passes == [[0, 1, 2, 3], [4, 5, 6]]


# ------------------------------------------------------------------------------------------------ the tool's parser
def test_tool_parser_has_the_model_and_data_flags_of_train():
    from protopformer_amd.alignment import get_args_parser
    from protopformer_amd.train import get_args_parser as train_parser
    own = {o: a for a in get_args_parser()._actions for o in a.option_strings}
    shared = [(o, a) for a in train_parser()._actions for o in a.option_strings]
    assert len(shared) > 40
    for o, a in shared:
        assert o in own and own[o].dest == a.dest, f"{o} of train.py is missing"
        assert own[o].default == (0 if a.dest == "seed" else a.default), o
    a = get_args_parser().parse_args([])
    assert (a.resume, a.split, a.protos_per_image, a.half_size, a.attack_steps, a.eps, a.attack, a.max_images, a.precise) == (
        "", "test", 3, 36, 10, 8.0, True, 0, False)
    a = get_args_parser().parse_args(["--resume", "x.pth", "--split", "train", "--protos_per_image", "2", "--half_size", "20", "--attack_steps", "4",
                                      "--eps", "4", "--no-attack", "--max_images", "5", "--precise", "--output_dir", "o"])
    assert (a.resume, a.split, a.protos_per_image, a.half_size, a.attack_steps, a.eps, a.attack, a.max_images, a.precise, a.output_dir) == (
        "x.pth", "train", 2, 20, 4, 4.0, False, 5, True, "o")


def test_tool_record_is_plain_json():
    import json
    from protopformer_amd.alignment import get_args_parser, summarize
    res = dict(images=2, rows=3, overall=dict(mean_share=0.4, mean_pac=float("nan")), per_prototype={7: dict(mean_share=0.5, rows=2), 2: dict(mean_share=float("nan"), rows=1)})
    doc = json.loads(json.dumps(summarize(res, get_args_parser().parse_args([])), allow_nan=False))
    assert doc["images"] == 2 and doc["rows"] == 3 and doc["overall"] == dict(mean_share=0.4, mean_pac=None)
    assert list(doc["per_prototype"]) == ["2", "7"] and doc["per_prototype"]["2"]["mean_share"] is None and doc["settings"]["eps_255"] == 8.0
