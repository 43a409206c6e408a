"""'This looks like that, because ...' on the host: known answers of the numpy referees (interpret.color_affine, gray_sum,
contrast_offset, bilateral, warp_nodes_from_ids, warp_apply, because_score), the global-importance arithmetic on hand-made rows, and
the tool's argument parser.  The referees ARE the definition the kernels of csrc/because.hip are held to (tests/test_gpu_because.py)."""
import math

import numpy as np
import pytest

from protopformer_amd import interpret as I

ZERO3, ONE3 = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def pixels(shape, seed=0):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def luma64(v):
    return sum(w * v[:, k].astype(np.float64) for k, w in enumerate(I.LUMA_WEIGHTS))


# ------------------------------------------------------------------------------------------------ colour
def test_saturation_zero_gives_three_bit_equal_channels():
    x = pixels((2, 3, 9, 11))
    m = I.saturation_matrix(0.0)
    assert same_bits(m[0], m[1]) and same_bits(m[1], m[2]) and same_bits(m[0], np.asarray(I.LUMA_WEIGHTS, dtype=np.float32))
    out = I.color_affine(x, m, ZERO3, ONE3, device=False)
    assert out.dtype == np.float32 and same_bits(out[:, 0], out[:, 1]) and same_bits(out[:, 1], out[:, 2])
    assert np.abs(out[:, 0] - luma64(x)).max() <= 2.0 ** -22
    assert same_bits(I.saturation_matrix(1.0), np.eye(3, dtype=np.float32))


def test_contrast_zero_gives_the_constant_image_of_the_offset_rule():
    x = pixels((3, 3, 8, 12), 1)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    xn = ((x - np.float32(mean).reshape(1, 3, 1, 1)) / np.float32(std).reshape(1, 3, 1, 1)).astype(np.float32)
    total = I.gray_sum(xn, mean, std, device=False)
    assert total.dtype == np.int32 and total.shape == (3,)
    off = I.contrast_offset(total, (8, 12), 0.0, device=False)
    want = ((total.astype(np.float32) / np.float32(96)).astype(np.float32) / np.float32(255)).astype(np.float32)      # fl(1 * m) = m
    assert off.shape == (3, 3) and same_bits(off, np.repeat(want[:, None], 3, axis=1))
    assert np.abs(want - luma64(I._denorm(xn, mean, std)).mean((1, 2))).max() < 1 / 255                               # the mean luma, to the 8-bit grid
    out = I.color_affine(xn, I.contrast_matrix(0.0), mean, std, offset=off, device=False)
    const = ((off - np.float32(mean)) / np.float32(std)).astype(np.float32)                                           # the offset, normalised again
    assert same_bits(out, np.broadcast_to(const[:, :, None, None], out.shape).copy())
    # contrast 1: the identity on pixels inside [0, 1]
    back = I.color_affine(x, I.contrast_matrix(1.0), ZERO3, ONE3, offset=I.contrast_offset(total, (8, 12), 1.0, device=False), device=False)
    assert same_bits(back, x)


def test_hue_zero_is_the_identity_and_a_turn_keeps_the_luma():
    x = pixels((4, 3, 16, 16), 2)
    assert np.abs(I.hue_matrix(0.0) - np.eye(3)).max() <= 2.0 ** -22
    assert np.abs(I.color_affine(x, I.hue_matrix(0.0), ZERO3, ONE3, device=False) - x).max() <= 2.0 ** -22
    for theta in (math.pi / 3, math.pi):
        m = I.hue_matrix(theta)
        raw = np.einsum("kc,bchw->bkhw", m.astype(np.float64), x.astype(np.float64))
        free = ((raw > 0) & (raw < 1)).all(axis=1)                                       # the pixels no channel of which clamps
        out = I.color_affine(x, m, ZERO3, ONE3, device=False)
        assert 0.3 < free.mean() < 1.0 and not np.array_equal(out, x)
        assert np.abs(luma64(out) - luma64(x))[free].max() <= 2.0 ** -22, theta
    # at a half turn about 15 % of the channel values of uniformly random pixels leave [0, 1] and are clamped -- 43 % of the pixels
    # in at least one channel (the README says so; measured on 200 000 pixels: 0.155 and 0.432)
    outside = (raw <= 0) | (raw >= 1)
    assert 0.10 < outside.mean() < 0.20 and 0.35 < 1.0 - free.mean() < 0.52


def test_gray_sum_of_an_all_ones_image():
    for shape in ((1, 3, 5, 7), (2, 3, 32, 32)):
        assert I.gray_sum(np.ones(shape, dtype=np.float32), ZERO3, ONE3, device=False).tolist() == [255 * shape[2] * shape[3]] * shape[0]
    assert I.gray_sum(np.zeros((1, 3, 4, 4), dtype=np.float32), ZERO3, ONE3, device=False).tolist() == [0]
    assert I.gray_sum(np.full((1, 3, 4, 4), np.nan, dtype=np.float32), ZERO3, ONE3, device=False).tolist() == [0]     # the clamp sends NaN to 0


# ------------------------------------------------------------------------------------------------ texture
def test_bilateral_with_delta_tables_is_the_exact_identity():
    x = pixels((2, 3, 10, 13), 3)
    for r in (1, 3):
        ws = np.zeros((2 * r + 1, 2 * r + 1), dtype=np.float32)
        ws[r, r] = 1.0
        wr = np.zeros(256, dtype=np.float32)
        wr[0] = 1.0
        assert same_bits(I.bilateral(x, ws, wr, ZERO3, ONE3, device=False), x)
        assert same_bits(I.bilateral(x, ws, np.ones(256, dtype=np.float32), ZERO3, ONE3, device=False), x)            # centre-only ws alone


def test_bilateral_keeps_both_sides_of_a_step_exact():
    x = np.full((1, 3, 12, 16), 0.25, dtype=np.float32)
    x[:, :, :, 8:] = 0.75
    wr = np.zeros(256, dtype=np.float32)
    wr[0] = 1.0                                                                          # the 8-bit lumas are 64 and 191: nothing crosses the edge
    for r, w in ((1, 1.0), (3, 0.5), (8, 0.25)):
        out = I.bilateral(x, np.full((2 * r + 1, 2 * r + 1), w, dtype=np.float32), wr, ZERO3, ONE3, device=False)
        assert same_bits(out, x), r
    # a wide range table smooths across the edge: the filter is not a no-op
    blur = I.bilateral(x, np.ones((3, 3), dtype=np.float32), np.ones(256, dtype=np.float32), ZERO3, ONE3, device=False)
    assert 0.25 < blur[0, 0, 5, 7] < 0.75 and blur[0, 0, 5, 0] == np.float32(0.25)
    ws, wrg = I.bilateral_tables(2, 1.5, 20.0)
    assert ws.shape == (5, 5) and ws[2, 2] == 1 and wrg[0] == 1 and np.all(np.diff(wrg) <= 0) and same_bits(ws, ws.T)
    with pytest.raises(ValueError, match="ws must hold"):
        I.bilateral(x, np.ones(8, dtype=np.float32), wr, ZERO3, ONE3, device=False)


# ------------------------------------------------------------------------------------------------ shape
def test_warp_amplitude_zero_is_the_identity():
    x = np.random.default_rng(4).standard_normal((2, 3, 20, 20)).astype(np.float32)
    x[0, 0, 0, :4] = (-0.0, np.inf, -np.inf, np.nan)
    for s in (2, 4):
        nodes = I.warp_nodes_from_ids(np.array([3, 2 ** 40 + 1]), s, 0, seed=5, device=False)
        assert nodes.shape == (2, (s + 1) ** 2, 2) and nodes.dtype == np.int32 and not nodes.any()
        assert same_bits(I.warp_apply(x, nodes, s, 0, device=False), x)


def test_warp_is_a_smooth_resampling():
    x = np.random.default_rng(5).standard_normal((1, 2, 20, 20)).astype(np.float32)
    # one whole pixel to the right everywhere: every pixel takes its right neighbour, the last column itself
    nodes = np.zeros((1, 9, 2), dtype=np.int32)
    nodes[..., 1] = 256
    out = I.warp_apply(x, nodes, 2, 256, device=False)
    assert same_bits(out[..., :-1], x[..., 1:]) and same_bits(out[..., -1], x[..., -1])
    # half a pixel down: the mean of two rows, exactly
    nodes = np.zeros((1, 9, 2), dtype=np.int32)
    nodes[..., 0] = 128
    out = I.warp_apply(x, nodes, 2, 256, device=False)
    assert same_bits(out[:, :, :-1], (np.float32(0.5) * x[:, :, :-1] + np.float32(0.5) * x[:, :, 1:]).astype(np.float32))
    # a node value outside the amplitude is clamped into it
    nodes[..., 0] = 9999
    assert same_bits(I.warp_apply(x, nodes, 2, 128, device=False), out)
    # a linear ramp stays inside its range under random nodes, amplitude above the node spacing included
    ramp = np.broadcast_to(np.arange(20, dtype=np.float32)[None, None, None, :], (1, 1, 20, 20)).copy()
    for s, amp in ((4, 3 * 256), (3, 12 * 256)):
        w = I.warp_apply(ramp, I.warp_nodes_from_ids([7], s, amp, device=False), s, amp, device=False)
        assert w.min() >= 0 and w.max() <= 19 and not np.array_equal(w, ramp)


def test_warp_nodes_do_not_depend_on_the_batch():
    ids = np.array([0, 5, 2 ** 32 + 5, 2 ** 40 + 123], dtype=np.int64)
    amp = 6 * 256
    full = I.warp_nodes_from_ids(ids, 4, amp, seed=9, device=False)
    assert full.shape == (4, 25, 2) and np.abs(full).max() <= amp and np.abs(full).max() > amp // 2
    for order in ([3, 1], [2], [1, 2, 0, 3]):
        assert np.array_equal(I.warp_nodes_from_ids(ids[order], 4, amp, seed=9, device=False), full[order])
    assert not np.array_equal(full[1], full[2])                                          # ids that agree in their low 32 bits
    assert not np.array_equal(I.warp_nodes_from_ids(ids, 4, amp, seed=10, device=False), full)
    # the draws are the library's Philox, counter (node, 2^31, id low, id high)
    w = I.philox4x32_10(np.array([[7, 0x80000000, 123, 2 ** 8]], dtype=np.uint64), np.array([9, 0], dtype=np.uint64))[0]
    assert full[3, 7].tolist() == [((int(w[0]) >> 8) * (2 * amp + 1) >> 24) - amp, ((int(w[1]) >> 8) * (2 * amp + 1) >> 24) - amp]
    with pytest.raises(ValueError, match="cells"):
        I.warp_nodes_from_ids(ids, 17, amp, device=False)


# ------------------------------------------------------------------------------------------------ score
def test_because_score_rows():
    B, P, T, G = 2, 5, 4, 9
    rng = np.random.default_rng(6)
    act_full = rng.random((B, P, T), dtype=np.float32)
    act_max = act_full.max(-1)
    idx = np.array([[0, 3, 4, 8], [1, 2, 99, -1]], dtype=np.int32)                       # image 1 carries two entries outside the grid
    act_full[0, 2, 1] = np.nan
    protos = np.array([[0, 2, 4, 7], [1, 3, 3, -1]], dtype=np.int32)
    cells = np.array([[4, 3, 5, 0], [2, 99, -1, 1]], dtype=np.int32)
    same, best, lost = I.because_score(act_max, protos, G, act_full=act_full, idx=idx, cells=cells, device=False)
    assert same.dtype == np.float32 and best.dtype == np.float32 and lost.dtype == np.int32
    assert lost.tolist() == [[0, 0, 1, 1], [0, 1, 1, 1]]
    assert same[0, 0] == act_full[0, 0, 2] and np.isnan(same[0, 1]) and same[0, 2] == 0 and same[0, 3] == 0       # kept, NaN kept, lost, bad prototype
    assert same[1, 0] == act_full[1, 1, 1] and same[1, 1] == 0 and same[1, 2] == 0                                 # kept, out of range twice
    assert same_bits(best[0, :3], act_max[0, [0, 2, 4]]) and np.isnan(best[0, 3]) and np.isnan(best[1, 3])
    g_same, g_best, g_lost = I.because_score(act_max, protos, device=False)              # the global branch: best only
    assert g_same is None and g_lost is None and same_bits(g_best, best)


# ------------------------------------------------------------------------------------------------ global importance
def test_global_importance_on_hand_made_rows():
    names = ("hue", "texture", "shape")
    ids = np.array([11, 10, 12])                                                         # rows arrive out of id order
    protos = np.array([[0, 1], [0, 1], [0, 2]])
    base = np.array([[2.0, 1.0], [1.0, 0.0], [3.0, 0.0]])
    same = np.array([[[1.0, 1.0], [1.0, 0.0], [0.0, 0.0]],                               # hue
                     [[2.0, 0.5], [0.0, 0.0], [3.0, 0.0]],                               # texture
                     [[1.0, 1.0], [1.0, 0.0], [0.0, 0.0]]])                              # shape: the same numbers as hue
    best = same + 0.5
    lost = np.zeros((3, 3, 2), dtype=np.int32)
    lost[0, 2, 0] = 1
    r = I.importance_from_rows(ids, protos, base, same, best, lost, names)
    p0 = r["per_prototype"][0]
    assert p0["rows"] == 3
    assert p0["importance"]["hue"] == (1 * 0 + 2 * 1 + 3 * 3) / 6 and p0["importance"]["texture"] == (1 * 1 + 0 + 0) / 6
    assert p0["mean"]["hue"] == (0 + 1 + 3) / 3 and p0["lost"]["hue"] == 1 / 3 and p0["lost"]["texture"] == 0
    assert p0["importance_best"]["hue"] == (1 * -0.5 + 2 * 0.5 + 3 * 2.5) / 6
    assert p0["dominant"] == "hue"                                                       # hue ties with shape: the earlier name
    p1 = r["per_prototype"][1]
    assert p1["rows"] == 2 and p1["importance"] == dict(hue=0.0, texture=0.5, shape=0.0) and p1["dominant"] == "texture"
    p2 = r["per_prototype"][2]                                                           # sum g == 0: null, the mean is still defined
    assert p2["rows"] == 1 and p2["importance"] == dict.fromkeys(names) and p2["dominant"] is None and p2["mean"]["hue"] == 0.0
    assert r["overall"]["rows"] == 6 and r["overall"]["importance"]["hue"] == 11 / 7 and r["overall"]["dominant"] == "hue"
    empty = I.importance_from_rows(np.zeros(0), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((3, 0, 2)), np.zeros((3, 0, 2)), np.zeros((3, 0, 2)), names)
    assert empty["per_prototype"] == {} and empty["overall"]["rows"] == 0 and empty["overall"]["importance"] == dict.fromkeys(names)
    assert empty["overall"]["mean"] == dict.fromkeys(names) and empty["overall"]["dominant"] is None
    # the global branch has no cells: best stands in for same, the lost share is null
    g = I.importance_from_rows(ids, protos, base, None, best, None, names)
    assert g["per_prototype"][0]["importance"] == g["per_prototype"][0]["importance_best"] == p0["importance_best"]
    assert g["per_prototype"][0]["lost"] == dict.fromkeys(names)


def test_parameters_and_matrices():
    p = I.because_params(dict(radius=2, amplitude=3.5))
    assert p["radius"] == 2 and p["amplitude"] == 3.5 and p["hue"] == I.BECAUSE_DEFAULTS["hue"] and p["mean"].dtype == np.float32
    assert I.because_params(p)["radius"] == 2                                            # idempotent
    for bad in (dict(radius=9), dict(cells=0), dict(sigma_range=0.0), dict(amplitude=200), dict(colour=1)):
        with pytest.raises(ValueError):
            I.because_params(bad)
    assert I.warp_amplitude(6.0) == 1536
    x = pixels((2, 3, 12, 12), 8)
    for name in I.CHARACTERISTICS:
        out = I.because_perturb(x, name, dict(mean=ZERO3, std=ONE3, radius=2), seed=1, image_ids=[4, 2 ** 33], device=False)
        assert out.shape == x.shape and out.dtype == np.float32 and np.isfinite(out).all() and not np.array_equal(out, x), name
    with pytest.raises(ValueError, match="characteristics"):
        I.because_perturb(x, "size", device=False)


def test_tool_argument_parser():
    from protopformer_amd import because as tool
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--output_dir", "out"])
    assert args.split == "train" and args.characteristics == list(I.CHARACTERISTICS) and args.protos == "own" and args.protos_per_image == 3
    assert args.seed == 0 and args.max_images == 0 and not args.per_image and args.save_images == 0 and args.pass_images == 16
    d = I.BECAUSE_DEFAULTS
    assert tool.params_from_args(args) == {k: d[k] for k in ("hue", "saturation", "contrast", "radius", "sigma_space", "sigma_range", "cells", "amplitude")}
    I.because_params(tool.params_from_args(args))
    args = tool.get_args_parser().parse_args(["--characteristics", "texture", "shape", "--protos", "top", "--protos_per_image", "2", "--per-image",
                                              "--save-images", "4", "--hue_turn", "0.25", "--texture_radius", "8", "--shape_amplitude", "2.5",
                                              "--split", "test", "--max_images", "10"])
    assert args.characteristics == ["texture", "shape"] and args.protos == "top" and args.per_image and args.save_images == 4
    p = tool.params_from_args(args)
    assert p["hue"] == 0.25 and p["radius"] == 8 and p["amplitude"] == 2.5 and args.split == "test" and args.max_images == 10
    with pytest.raises(SystemExit):
        tool.get_args_parser().parse_args(["--characteristics", "size"])
    help_text = tool.get_args_parser().format_help()
    assert "not a tuned value" in help_text
