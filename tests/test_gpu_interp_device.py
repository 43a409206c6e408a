"""Interpretability post-processing on the GPU (csrc/interp.hip through interpret.upsample_cubic_device / activation_peaks /
high_activation_boxes and consistency_from_outputs(device=True)) against the host functions of interpret.py, which are the referee and
are called here.  Every comparison is exact: the kernels repeat resize_cubic's fp64 arithmetic operation for operation, so the maps
must agree bit for bit (compared as int32 patterns), and peaks, boxes and part tables as integers.

Inputs are seeded fp32 maps passed through log((d + 1) / (d + 1e-4)) of positive noise, like real activations.  Host references are
computed once per shape and shared."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from protopformer_amd import interpret as I

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(14, 224), (9, 224), (3, 7), (1, 5), (14, 14)]      # integer ratio, non-integer ratio, tiny, every tap clamped, identity
COUNTS = [1, 130]                                             # one map; more maps than one wave of workgroups, not a multiple of anything


def bits(t):
    return t.contiguous().view(torch.int32)


def activation_like(shape, seed):
    d = np.random.default_rng(seed).random(shape, dtype=np.float32) * 4.0
    return np.log((d + 1) / (d + np.float32(1e-4))).astype(np.float32)


def constructed(g):
    """The constructed maps: a single hot cell, all zero, constant, the largest cell in a corner on top of noise."""
    hot = np.zeros((g, g), dtype=np.float32); hot[g // 2, g // 3] = 7.25
    corner = activation_like((g, g), 99); corner[g - 1, g - 1] = corner.max() + 3.0
    corner0 = activation_like((g, g), 98); corner0[0, g - 1] = corner0.max() + 3.0
    return np.stack([hot, np.zeros((g, g), dtype=np.float32), np.full((g, g), 3.5, dtype=np.float32), corner, corner0])


@functools.lru_cache(maxsize=None)
def host_case(M, g, S):
    """(maps (M, g, g) fp32, resize_cubic of each (M, S, S) fp32); read-only for the tests that share it."""
    maps = activation_like((M, g, g), 1000 * g + S + M)
    up = np.stack([I.resize_cubic(m, S) for m in maps])
    maps.setflags(write=False); up.setflags(write=False)
    return maps, up


@functools.lru_cache(maxsize=None)
def host_constructed(g, S):
    maps = constructed(g)
    up = np.stack([I.resize_cubic(m, S) for m in maps])
    maps.setflags(write=False); up.setflags(write=False)
    return maps, up


def host_peaks(up):
    val = np.array([u.max() for u in up], dtype=np.float32)
    yx = np.array([[int(t[0]) for t in np.where(u == u.max())] for u in up], dtype=np.int32)
    return val, yx


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the shared references are read-only


# ------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("g,S", SHAPES)
def test_upsample_is_bit_identical_to_resize_cubic(g, S, M):
    maps, up = host_case(M, g, S)
    out = I.upsample_cubic_device(dev(maps), S)
    assert out.shape == (M, S, S) and out.dtype == torch.float32
    assert torch.equal(bits(out.cpu()), bits(torch.from_numpy(up.copy()))), \
        f"{int((bits(out.cpu()) != bits(torch.from_numpy(up.copy()))).sum())} of {up.size} values differ"


def test_upsample_keeps_leading_dimensions_and_constructed_maps():
    maps, up = host_constructed(14, 224)
    out = I.upsample_cubic_device(dev(maps).reshape(1, 5, 14, 14), 224)
    assert out.shape == (1, 5, 224, 224)
    assert torch.equal(bits(out.cpu()).reshape(5, 224, 224), bits(torch.from_numpy(up.copy())))


def test_upsample_past_two_to_the_31_elements():
    """42 900 maps of 224 x 224 are 2.15e9 output values: the offsets of the last maps do not fit 32 bits."""
    M, g, S = 42900, 14, 224
    assert M * S * S > 2 ** 31
    head, _ = host_case(130, g, S)
    maps = np.concatenate([np.zeros((M - 130, g, g), dtype=np.float32), head])
    maps[:3] = head[:3]
    out = I.upsample_cubic_device(dev(maps), S)
    _, up = host_case(130, g, S)
    got_last, got_first = out[M - 130:].cpu(), out[:3].cpu()
    middle_is_zero = bool((out[M // 2] == 0).all())
    del out
    torch.cuda.empty_cache()
    assert torch.equal(bits(got_last), bits(torch.from_numpy(up.copy())))
    assert torch.equal(bits(got_first), bits(torch.from_numpy(up[:3].copy()))) and middle_is_zero


# ------------------------------------------------------------------------------------------------ peak
@pytest.mark.parametrize("M", COUNTS)
@pytest.mark.parametrize("g,S", SHAPES)
def test_peak_matches_first_argmax_of_the_host_map(g, S, M):
    maps, up = host_case(M, g, S)
    val, yx = I.activation_peaks(dev(maps), S)
    ref_val, ref_yx = host_peaks(up)
    assert val.shape == (M,) and yx.shape == (M, 2) and yx.dtype == torch.int32
    assert np.array_equal(yx.cpu().numpy(), ref_yx)
    assert np.array_equal(val.cpu().numpy(), ref_val)


@pytest.mark.parametrize("g,S", [(14, 224), (7, 224), (14, 14), (3, 7)])
def test_peak_constructed_cases(g, S):
    maps, up = host_constructed(g, S)
    val, yx = I.activation_peaks(dev(maps), S)
    ref_val, ref_yx = host_peaks(up)
    ties = [int((u == u.max()).sum()) for u in up]
    print(f"g={g} S={S}: entries equal to the maximum per constructed map {ties}, host peaks {ref_yx.tolist()}")
    assert np.array_equal(yx.cpu().numpy(), ref_yx), (yx.cpu().numpy().tolist(), ref_yx.tolist(), ties)
    assert np.array_equal(val.cpu().numpy(), ref_val)
    assert yx[1].tolist() == [0, 0] and float(val[1]) == 0.0              # all zero: every entry ties, the first wins


# ------------------------------------------------------------------------------------------------ part table
def part_lists(ref_yx, ppc, half, S, seed):
    """Per image [(part id, x, y)]: none, one, and all 15 -- the eight points on and one pixel outside the four edges of the box around
    the image's FIRST prototype's peak, then random points."""
    rng = np.random.default_rng(seed)
    n_img = ref_yx.shape[0] // ppc
    out = []
    for j in range(n_img):
        my, mx = (int(v) for v in ref_yx[j * ppc])
        y0, y1, x0, x1 = max(0, my - half), min(S, my + half), max(0, mx - half), min(S, mx + half)
        edge = [(mx, y0), (mx, y0 - 1), (mx, y1), (mx, y1 + 1), (x0, my), (x0 - 1, my), (x1, my), (x1 + 1, my)]
        rnd = [(int(rng.integers(0, S)), int(rng.integers(0, S))) for _ in range(7)]
        full = [(p, x, y) for p, (x, y) in enumerate(edge + rnd)]
        out.append([[], [full[int(rng.integers(0, 15))]], full, full[::-1]][j % 4])
    return out


@pytest.mark.parametrize("half", [36, 200])
def test_part_table_equals_prototype_part_table(half):
    ppc, n_img, g, S, n_parts = 10, 4, 14, 224, 15
    maps, up = host_case(130, g, S)
    maps, up = maps[:n_img * ppc], up[:n_img * ppc]                               # 40 maps
    _, ref_yx = host_peaks(up)
    lists = part_lists(ref_yx, ppc, half, S, seed=half)
    assert sorted(len(l) for l in lists) == [0, 1, 15, 15]
    ref = np.stack([I.prototype_part_table(maps[j * ppc:(j + 1) * ppc], lists[j], S, half, n_parts) for j in range(n_img)])
    assert 0 < ref.sum() < ref.size
    plist = np.zeros((n_img, n_parts, 3), dtype=np.int32)
    for j, l in enumerate(lists):
        for p, x, y in l:
            plist[j, p] = (1, x, y)
    from protopformer_amd import ops
    val, yx, fused = ops.act_peak(dev(maps), S, dev(plist), half)
    alone = ops.act_part_table(yx, S, dev(plist), half)
    assert fused.dtype == torch.uint8 and fused.shape == (n_img * ppc, n_parts)
    assert np.array_equal(fused.cpu().numpy().reshape(n_img, ppc, n_parts), ref.astype(np.uint8))
    assert torch.equal(fused, alone)
    # the eight edge points of the image with all 15 parts, for its first prototype: on the edge inside, one pixel further outside
    assert ref[2, 0, :8].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ box
def box_maps(g):
    one_off = np.full((g, g), 1.25, dtype=np.float32); one_off[g // 2, 0] = 2.0
    one_low = np.full((g, g), 1.25, dtype=np.float32); one_low[0, g // 2] = 0.5
    return np.concatenate([activation_like((6, g, g), 7 + g), constructed(g), np.stack([one_off, one_low])])


@pytest.mark.parametrize("percentile", [95, 50, 100, 0])
@pytest.mark.parametrize("g,S", [(14, 224), (9, 224), (3, 7), (1, 5), (14, 14)])
def test_box_equals_find_high_activation_crop(g, S, percentile):
    maps = box_maps(g)
    ref = np.array([I.find_high_activation_crop(I.resize_cubic(m, S), percentile) for m in maps], dtype=np.int32)
    box = I.high_activation_boxes(dev(maps), S, percentile)
    assert box.shape == (len(maps), 4) and box.dtype == torch.int32
    assert np.array_equal(box.cpu().numpy(), ref), (box.cpu().numpy().tolist(), ref.tolist())
    if percentile == 0:
        assert (ref == np.array([0, S, 0, S])).all()                              # the threshold is the minimum: every pixel passes


def test_order_statistics_are_exact():
    """ppf_act_order_stats against a sort of the host map, at ranks that sit inside runs of equal values and at both ends."""
    from protopformer_amd import ops
    g, S = 14, 224
    maps = box_maps(g)
    srt = np.stack([np.sort(I.resize_cubic(m, S).reshape(-1)) for m in maps])
    for lo, hi in [(0, 0), (0, 1), (S * S - 1, S * S - 1), (S * S - 2, S * S - 1), (25087, 25088), (47666, 47667), (12345, 12345)]:
        got = ops.act_order_stats(dev(maps), S, lo, hi).cpu().numpy()
        assert np.array_equal(got, srt[:, [lo, hi]]), (lo, hi)


# ------------------------------------------------------------------------------------------------ repeats
def test_two_consecutive_calls_are_bit_identical():
    maps, _ = host_case(130, 14, 224)
    d = dev(maps)
    a, b = I.upsample_cubic_device(d, 224), I.upsample_cubic_device(d, 224)
    assert torch.equal(bits(a), bits(b))
    (v0, p0), (v1, p1) = I.activation_peaks(d, 224), I.activation_peaks(d, 224)
    assert torch.equal(bits(v0), bits(v1)) and torch.equal(p0, p1)
    assert torch.equal(I.high_activation_boxes(d, 224, 95), I.high_activation_boxes(d, 224, 95))


# ------------------------------------------------------------------------------------------------ end to end
def test_consistency_device_equals_host_on_the_golden_inputs():
    import mini_trees as M
    z = np.load(os.path.join(HERE, "golden", "interp_consistency.npz"))
    locs = {}
    for i, pid, x, y in z["parts_locs"].tolist():
        locs.setdefault(i, []).append([pid, x, y])
    parts = types.SimpleNamespace(id_to_part_loc=locs)
    sizes = {int(i): M.cub_size(int(i)) for i in z["ids"]}
    args = (z["attn"], z["acts"], z["targets"], z["ids"], parts, sizes, int(z["k"]), int(z["img_size"]))
    nc = int(z["targets"].max()) + 1
    host = I.consistency_from_outputs(*args, num_classes=nc)
    devr = I.consistency_from_outputs(*args, num_classes=nc, device=True)
    assert devr[0] == host[0] == pytest.approx(float(z["score"]), abs=1e-12)
    assert devr[1] == host[1] == z["class_proto_effect"].tolist()
    assert devr[2] == host[2]
    assert devr[3].is_cuda and np.array_equal(devr[3].cpu().numpy(), host[3])


def random_eval(B=64, ppc=10, k=81, n=196, classes=8, seed=3):
    rng = np.random.default_rng(seed)
    s = int(round(k ** 0.5))
    attn = rng.random((B, n), dtype=np.float32)
    acts = activation_like((B, ppc, s, s), seed + 1)
    targets = rng.integers(0, classes, B)
    ids = np.arange(100, 100 + B)
    sizes = {int(i): (int(rng.integers(200, 500)), int(rng.integers(150, 400))) for i in ids}
    locs = {}
    for i in ids:
        w, h = sizes[int(i)]
        locs[int(i)] = [[p, float(rng.random() * (w - 1)), float(rng.random() * (h - 1))] for p in range(1, 16) if rng.random() < 0.7]
    return attn, acts, targets, ids, types.SimpleNamespace(id_to_part_loc=locs), sizes, k, classes


def test_consistency_device_equals_host_with_reserved_tokens():
    """64 random images, 81 of 196 tokens reserved: expand_to_grid runs on the device."""
    attn, acts, targets, ids, parts, sizes, k, classes = random_eval()
    host = I.consistency_from_outputs(attn, acts, targets, ids, parts, sizes, k, 224, num_classes=classes)
    devr = I.consistency_from_outputs(attn, acts, targets, ids, parts, sizes, k, 224, num_classes=classes, device=True)
    assert devr[0] == host[0] and devr[1] == host[1] and devr[2] == host[2]
    assert len(host[1]) == classes * 10 and 0 < sum(host[1]) + sum(m > 0 for m in host[2])
    assert np.array_equal(devr[3].cpu().numpy(), host[3])


def test_consistency_score_device_keyword_through_a_loader():
    """consistency_score's own loop (gather of the class's prototypes, one launch per batch) with a stand-in for the model."""
    attn, acts, targets, ids, parts, sizes, k, classes = random_eval(B=24, seed=11)
    ppc, s = acts.shape[1], acts.shape[2]
    full = np.zeros((24, classes * ppc, s, s), dtype=np.float32)
    for b in range(24):
        full[b, targets[b] * ppc:(targets[b] + 1) * ppc] = acts[b]
    store = (torch.from_numpy(attn).cuda(), torch.from_numpy(full).cuda())

    class Net:
        num_prototypes_per_class, reserve_token_nums, img_size = ppc, [k], 224

        def eval(self):
            return self

        def push_forward(self, x):
            rows = x.long()
            return store[0][rows], store[1][rows]

    loader = [(torch.arange(b, b + 8).cuda(), torch.from_numpy(targets[b:b + 8]), torch.from_numpy(ids[b:b + 8])) for b in range(0, 24, 8)]
    host = I.consistency_score(Net(), loader, parts, sizes, num_classes=classes)
    assert I.consistency_score(Net(), loader, parts, sizes, num_classes=classes, device=True) == host
    assert host == I.consistency_from_outputs(attn, acts, targets, ids, parts, sizes, k, 224, num_classes=classes)[0]


# ------------------------------------------------------------------------------------------------ errors
@pytest.mark.parametrize("fn", [I.upsample_cubic_device, I.activation_peaks, I.high_activation_boxes])
def test_bad_inputs_raise_the_shape_error_instead_of_launching(fn):
    good = torch.zeros((2, 4, 4), device="cuda")
    for size in (0, -3):
        with pytest.raises(RuntimeError, match=r"rc=-1.*S=" + str(size)):
            fn(good, size)
    with pytest.raises(RuntimeError, match=r"rc=-1.*g=0"):
        fn(torch.zeros((2, 0, 0), device="cuda"), 8)
    with pytest.raises(RuntimeError, match=r"rc=-1.*contiguous"):
        fn(torch.zeros((2, 4, 8), device="cuda")[:, :, ::2], 8)
    with pytest.raises(RuntimeError, match=r"rc=-1.*fp32"):
        fn(torch.zeros((2, 4, 4), device="cuda", dtype=torch.float64), 8)
    with pytest.raises(RuntimeError, match=r"rc=-1.*g=65"):
        fn(torch.zeros((1, 65, 65), device="cuda"), 8)
    torch.cuda.synchronize()
