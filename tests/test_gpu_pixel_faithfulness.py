"""Deletion / insertion curves per pixel on the GPU: ppf_pixel_order, ppf_pixel_random, ppf_pixel_perturb and ppf_gauss_blur
(csrc/pixel_faithful.hip) against the numpy referees of interpret.py (pixel_order_from_scores, pixel_random_scores, perturb_pixels,
gauss_blur with device=False), interpret.faithfulness_curves with resolution="pixel" and baseline="blur" through the micro models against
the referee pipeline, and the command-line tool on the miniature CUB tree.

Ranks, random scores, perturbed images and blurred planes are compared bit for bit (a NaN matching any NaN); the class probabilities in
between come from the model's forward and ppf_class_prob and are held to that kernel's bound (test_gpu_faithfulness.prob_reference)."""
import json
import os

import numpy as np
import pytest
import torch

import test_gpu_faithfulness as cellpath
from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

same_bits, prob_reference, forward_logits = cellpath.same_bits, cellpath.prob_reference, cellpath.forward_logits


# ------------------------------------------------------------------------------------------------ 1. ppf_pixel_order
ORDER_SHAPES = [(3, 1), (2, 63), (2, 64), (2, 65), (3, 1024), (2, 2304), (5, 4096), (1, 50176), (2, 65536)]


def device_rank(score, classes):
    from protopformer_amd.interpret import pixel_order_from_scores
    out = pixel_order_from_scores(torch.from_numpy(score).cuda(), torch.from_numpy(classes).cuda(), device=True)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_rank(score, classes, what):
    from protopformer_amd.interpret import pixel_order_from_scores
    got, ref = device_rank(score, classes), pixel_order_from_scores(score, classes, device=False)
    assert got.shape == ref.shape == score.shape and got.dtype == np.int32
    assert np.array_equal(got, ref), f"{what}: rank differs from the referee in {int((got != ref).sum())} places"
    valid = classes >= 0
    assert (np.sort(got[valid], axis=-1) == np.arange(score.shape[-1])).all(), f"{what}: a valid row is not a permutation"
    assert (got[~valid] == -1).all(), f"{what}: a row without a class is not all -1"
    assert np.array_equal(device_rank(score, classes), got), f"{what}: the same call twice gives other bits"
    return got


def adversarial_rows(n, rng):
    """Rows that a sort gets wrong first: all equal, all NaN, NaN mixed in, signed zeros, infinities, denormals, sorted both ways."""
    normal = rng.standard_normal(n).astype(np.float32)
    mixed = normal.copy()
    mixed[rng.random(n) < 0.3] = np.nan
    zeros = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    infs = rng.choice(np.array([np.inf, -np.inf, 0.0, 1.0, -1.0, np.nan], dtype=np.float32), n)
    den = (rng.integers(-3, 4, n) * np.float32(1e-45)).astype(np.float32)                      # +-denormals and zeros: ties and sign changes
    asc = np.sort(normal)
    return np.stack([np.full(n, 2.5, dtype=np.float32), np.full(n, np.nan, dtype=np.float32), mixed, zeros, infs, den, asc, asc[::-1].copy()])


@pytest.mark.parametrize("R,n", ORDER_SHAPES, ids=[f"R{r}_n{n}" for r, n in ORDER_SHAPES])
def test_pixel_order_equals_the_referee_bit_for_bit(R, n):
    rng = np.random.default_rng(R * 100003 + n)
    classes = rng.integers(0, 10, R).astype(np.int32)
    if R >= 2:
        classes[1] = -1                                                                       # a row whose class could not be picked
    check_rank(rng.standard_normal((R, n)).astype(np.float32), classes, "normal scores")
    check_rank((rng.integers(0, 7, (R, n)) / np.float32(4) - 1).astype(np.float32), classes, "seven distinct values")
    rows = adversarial_rows(n, rng)
    cls = np.zeros(rows.shape[0], dtype=np.int32)
    got = check_rank(rows, cls, "adversarial rows")
    assert np.array_equal(got[0], np.arange(n)) and np.array_equal(got[1], np.arange(n)) and np.array_equal(got[3], np.arange(n))   # ties: pixel order


def test_pixel_order_of_more_rows_than_workgroups_and_refusals():
    from protopformer_amd import ops
    rng = np.random.default_rng(7)
    R, n = 300, 130                                                                           # the launch has 256 workgroups: 44 of them take two rows
    check_rank((rng.integers(0, 50, (R, n)) / np.float32(8)).astype(np.float32), rng.integers(-1, 5, R).astype(np.int32), "300 rows")
    with pytest.raises(RuntimeError, match="ppf_pixel_order.*n=65537"):
        ops.pixel_order(torch.zeros((1, 65537), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="classes must be torch.int32"):
        ops.pixel_order(torch.zeros((1, 8), device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. ppf_pixel_random
def test_pixel_random_equals_the_numpy_philox_whatever_the_batch():
    from protopformer_amd.interpret import pixel_random_scores
    ids = np.array([0, 5, (1 << 40) + 3, (1 << 62) + 11, 5], dtype=np.int64)
    n, seed = 4099, (1 << 33) + 9
    ref = pixel_random_scores(ids, n, seed=seed, device=False)
    dev = lambda i: pixel_random_scores(torch.from_numpy(np.ascontiguousarray(i)).cuda(), n, seed=seed, device=True).cpu().numpy()
    got = dev(ids)
    assert got.shape == ref.shape == (5, n) and got.dtype == np.float32 and np.array_equal(got.view(np.int32), ref.view(np.int32))
    assert ((got >= 0) & (got < 1)).all() and np.array_equal(got[1], got[4]) and not np.array_equal(got[0], got[1])
    assert not np.array_equal(got[2], dev(np.array([3], dtype=np.int64))[0]), "the high word of the image id is not in the counter"
    perm = np.array([3, 0, 2])
    assert np.array_equal(dev(ids[perm]), got[perm]) and np.array_equal(np.concatenate([dev(ids[:2]), dev(ids[2:])]), got)
    other = pixel_random_scores(torch.from_numpy(ids).cuda(), n, seed=seed + 1, device=True).cpu().numpy()
    assert not np.array_equal(other, got)


# ------------------------------------------------------------------------------------------------ 3. ppf_pixel_perturb
@pytest.mark.parametrize("B,M,H,W", [(2, 2, 32, 32), (2, 3, 64, 64), (1, 1, 224, 224), (2, 2, 6, 20)], ids=["32", "64", "224", "6x20"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_pixel_perturb_equals_numpy(B, M, H, W, tensor_baseline):
    from protopformer_amd.interpret import perturb_pixels
    rng = np.random.default_rng(H * 7 + W + B)
    n = H * W
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else -0.375
    rank = np.stack([np.stack([rng.permutation(n) for _ in range(M)]) for _ in range(B)]).astype(np.int32)
    if B > 1:
        rank[1, 0] = -1
    counts = [0, n // 3, n]                                                                   # S = 3: the two ends and a step between
    for insertion in (False, True):
        ref = perturb_pixels(x, rank, counts, insertion=insertion, baseline=base, device=False)
        got = perturb_pixels(torch.from_numpy(x).cuda(), torch.from_numpy(rank).cuda(), counts, insertion=insertion,
                             baseline=torch.from_numpy(base).cuda() if tensor_baseline else base, device=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == ref.shape == (3, B, M, 3, H, W)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), f"insertion={insertion}: differs from numpy"
        if B > 1:
            assert np.array_equal(got[:, 1, 0], np.broadcast_to(x[1], got[:, 1, 0].shape))   # the -1 row copies x
        full, none = (got[2], got[0]) if insertion else (got[0], got[2])
        assert np.array_equal(full[0, M - 1], x[0]), "the untouched end is not x"
        assert np.array_equal(none[0, M - 1], np.broadcast_to(np.float32(base) if not tensor_baseline else base[0], x[0].shape)), "the emptied end is not the baseline"
        mid = got[1, 0, M - 1]
        changed = (mid != x[0]).any(0)
        assert int(changed.sum()) <= (n // 3 if not insertion else n - n // 3)


def test_pixel_perturb_refuses_odd_widths_and_unaligned_views():
    from protopformer_amd import ops
    counts = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    x = torch.zeros((1, 3, 8, 30), device="cuda")
    with pytest.raises(RuntimeError, match="ppf_pixel_perturb.*multiple of 4"):
        ops.pixel_perturb(x, torch.zeros((1, 1, 240), dtype=torch.int32, device="cuda"), counts)
    flat = torch.zeros(3 * 32 * 32 + 1, device="cuda")
    rank = torch.zeros((1, 1, 1024), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ppf_pixel_perturb.*16-byte aligned"):
        ops.pixel_perturb(flat[1:].view(1, 3, 32, 32), rank, counts)
    with pytest.raises(ValueError, match="rank must be an int32 CUDA tensor"):
        ops.pixel_perturb(flat[:-1].view(1, 3, 32, 32), torch.zeros((1, 1, 64), dtype=torch.int32, device="cuda"), counts)
    with pytest.raises(RuntimeError, match="ppf_pixel_perturb.*M=9"):
        ops.pixel_perturb(flat[:-1].view(1, 3, 32, 32), torch.zeros((1, 9, 1024), dtype=torch.int32, device="cuda"), counts)


# ------------------------------------------------------------------------------------------------ 4. ppf_gauss_blur
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 9), (1, 32, 32), (3, 224, 224), (2, 17, 130)], ids=["1x1", "7x9", "32", "3x224", "17x130"])
@pytest.mark.parametrize("radius", [1, 5, 16])
def test_gauss_blur_equals_the_referee_bit_for_bit(shape, radius):
    from protopformer_amd.interpret import gauss_blur
    rng = np.random.default_rng(shape[1] * 31 + radius)
    x = rng.standard_normal(shape).astype(np.float32)
    if shape[1] > 1:
        x[0, 0, 0], x[-1, -1, -1], x[0, shape[1] // 2, shape[2] // 2] = -0.0, 1e-42, 3e38       # a signed zero, a denormal, products near overflow
    for sigma in (5.0, 0.8):
        ref = gauss_blur(x, sigma=sigma, radius=radius, device=False)
        got = gauss_blur(torch.from_numpy(x).cuda(), sigma=sigma, radius=radius, device=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == ref.shape == shape and got.dtype == np.float32
        assert same_bits(got, ref), f"{shape} r={radius} sigma={sigma}: {int((got.view(np.int32) != ref.view(np.int32)).sum())} elements differ"


def test_gauss_blur_skips_taps_outside_the_plane_and_refuses_bad_radii():
    from protopformer_amd import ops
    from protopformer_amd.interpret import gauss_blur
    x = np.ones((1, 5, 12), dtype=np.float32)
    x[0, 0, 0], x[0, 4, 11] = np.inf, np.nan                       # an infinity at the border: a zero border that was multiplied in would make NaN
    ref = gauss_blur(x, radius=3, device=False)
    got = gauss_blur(torch.from_numpy(x).cuda(), radius=3, device=True).cpu().numpy()
    assert same_bits(got, ref) and np.isinf(got[0, 0, 0]) and np.isnan(got[0, 4, 11]) and np.isfinite(got[0, 2, 5])
    with pytest.raises(RuntimeError, match="ppf_gauss_blur.*r=17"):
        ops.gauss_blur(torch.zeros((1, 8, 8), device="cuda"), torch.zeros(35, device="cuda"))
    with pytest.raises(ValueError, match="taps must be"):
        ops.gauss_blur(torch.zeros((1, 8, 8), device="cuda"), torch.zeros(4, device="cuda"))


# ------------------------------------------------------------------------------------------------ 5. through the micro models
def referee_scores(m, r, coe, classes, order, size, ids, seed):
    """The [B, M, n] pixel scores of the referee pipeline for 'evidence', 'attention' and 'random' from the branch outputs r."""
    from protopformer_amd.interpret import cell_order_from_outputs, pixel_random_scores, resize_cubic
    B, M = classes.shape
    G = int(m.num_patches)
    side = int(round(G ** 0.5))
    if order == "random":
        return np.repeat(pixel_random_scores(ids, size * size, seed=seed, device=False)[:, None], M, axis=1)
    if order == "attention":
        attn = r.cls_attn.reshape(B, side, side).float().cpu().numpy()
        return np.repeat(np.stack([resize_cubic(a, size) for a in attn]).reshape(B, 1, -1), M, axis=1)
    _, _, cell = cell_order_from_outputs(r.act_full, r.idx, r.cls_attn, m.last_layer.weight.detach(), 1.0 - coe, classes, G, device=False)
    idx = r.idx.cpu().numpy()
    grid = np.zeros((B, M, G), dtype=np.float32)
    for b in range(B):
        keep = idx[b][(idx[b] >= 0) & (idx[b] < G)]
        grid[b][:, keep] = cell[b][:, keep]
    return np.stack([resize_cubic(g.reshape(side, side), size) for g in grid.reshape(B * M, G)]).reshape(B, M, -1)


@pytest.fixture(scope="module", params=["micro_deit.npz", "micro_cait.npz"])
def model_case(request):
    sd, cfg, z = micro(request.param)
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda()
    with torch.no_grad():
        r = m._branches(x, want_dist=False)
    return dict(name=request.param, m=m, x=x, img=z["img"], r=r, coe=cfg["global_coe"])


@pytest.mark.parametrize("order", ["evidence", "attention", "random"])
def test_pixel_curves_equal_the_referee_pipeline(model_case, order):
    from protopformer_amd.interpret import default_counts, faithfulness_curves, gauss_blur, perturb_pixels, pixel_order_from_scores
    m, x, img, r, name = (model_case[k] for k in ("m", "x", "img", "r", "name"))
    B, M, size = x.shape[0], 2, x.shape[2]
    n, bs, ids, seed = size * size, B * 2, np.array([5, 6, (1 << 41) + 7, 8], dtype=np.int64)[:B], 3
    assert n == 4096
    f = faithfulness_curves(m, x, top_classes=M, batch_size=bs, order=order, resolution="pixel", seed=seed, image_ids=ids)
    assert f.resolution == "pixel" and f.order is None and f.grid_cells == n
    h = f.cpu()
    counts = default_counts(n)
    S = len(counts)
    assert np.array_equal(h.counts, counts) and counts[0] == 0 and counts[-1] == n and h.classes.shape == (B, M) and (h.classes >= 0).all()
    score = referee_scores(m, r, model_case["coe"], h.classes, order, size, ids, seed)
    rank = pixel_order_from_scores(score, h.classes, device=False)
    assert h.score.shape == (B, M, n) and same_bits(h.score, score), f"{name} {order}: the pixel scores differ from the referee pipeline"
    assert h.rank.shape == (B, M, n) and np.array_equal(h.rank, rank), f"{name} {order}: the ranks differ from the referee order of the scores"
    cls = h.classes.reshape(-1)
    p_clean, b_clean = prob_reference(forward_logits(m, np.repeat(img, M, axis=0), bs), cls)
    worst = 0.0
    for mode in ("deletion", "insertion"):
        imgs = perturb_pixels(img, rank, counts, insertion=mode == "insertion", device=False)
        ref, bound = prob_reference(forward_logits(m, imgs.reshape((-1,) + imgs.shape[3:]), bs), np.tile(cls, S))
        got = h.curves[mode].transpose(2, 0, 1).reshape(-1).astype(np.float64)                # [S, B, M]
        rel = np.abs(got - ref) / ref
        worst = max(worst, float((rel / bound).max()))
        assert (rel <= bound).all(), f"{name} {order} {mode}: off the referee pipeline by {(rel / bound).max():.2f} bounds"
        ends = h.curves[mode].reshape(B * M, S).astype(np.float64)
        full = ends[:, 0] if mode == "deletion" else ends[:, -1]
        assert (np.abs(full - p_clean) <= b_clean * p_clean).all(), f"{name} {order} {mode}: the untouched end is not the clean probability"
    print(f"{name} {order}: largest curve error / bound = {worst:.3f}")
    auc = h.auc()
    assert auc["deletion"].shape == (B, M) and ((auc["deletion"] >= 0) & (auc["deletion"] <= 1)).all()
    # a scratch bound of one step gives the same curves
    one = faithfulness_curves(m, x, classes=h.classes, batch_size=bs, order=order, resolution="pixel", seed=seed, image_ids=ids, scratch_bytes=1)
    assert all(torch.equal(one.curves[k], f.curves[k]) for k in f.curves) and torch.equal(one.rank, f.rank)
    if order != "evidence":
        return
    # baseline="blur": the emptied end is the probability of gauss_blur(x)
    g = faithfulness_curves(m, x, classes=h.classes, batch_size=bs, order=order, resolution="pixel", baseline="blur").cpu()
    blurred = gauss_blur(img, device=False)
    p_blur, b_blur = prob_reference(forward_logits(m, np.repeat(blurred, M, axis=0), bs), cls)
    for mode, end in (("deletion", -1), ("insertion", 0)):
        none = g.curves[mode].reshape(B * M, S)[:, end].astype(np.float64)
        assert (np.abs(none - p_blur) <= b_blur * p_blur).all(), f"{name} {mode}: the emptied end is not the probability of the blurred image"
    assert np.array_equal(g.rank, h.rank)
    assert not m.training


def test_blur_baseline_on_the_cell_path_is_the_blurred_tensor(model_case):
    from protopformer_amd.interpret import faithfulness_curves, gauss_blur
    m, x = model_case["m"], model_case["x"]
    kw = dict(top_classes=2, batch_size=x.shape[0] * 2, order="attention")
    a = faithfulness_curves(m, x, baseline="blur", blur=dict(radius=3), **kw)
    b = faithfulness_curves(m, x, baseline=gauss_blur(x, radius=3), **kw)
    plain = faithfulness_curves(m, x, **kw)
    assert a.resolution == "cell" and all(torch.equal(a.curves[k].view(torch.int32), b.curves[k].view(torch.int32)) for k in a.curves)
    assert torch.equal(a.order, b.order) and not torch.equal(a.curves["deletion"], plain.curves["deletion"])
    with pytest.raises(ValueError, match="baseline must be"):
        faithfulness_curves(m, x, baseline="mean", **kw)
    with pytest.raises(ValueError, match="resolution must be"):
        faithfulness_curves(m, x, resolution="patch", **kw)


@pytest.mark.parametrize("order,kw", [("rise", dict(rise=dict(masks=8, cells=2))), ("ig", dict(ig=dict(steps=2)))], ids=["rise", "ig"])
def test_pixel_rank_of_rise_and_ig_is_the_referee_order_of_the_map_they_carry(model_case, order, kw):
    from protopformer_amd.interpret import faithfulness_curves, pixel_order_from_scores
    m, x, name = model_case["m"], model_case["x"], model_case["name"]
    B, M = x.shape[0], 2
    h = faithfulness_curves(m, x, top_classes=M, batch_size=B, order=order, resolution="pixel", counts=[0, 2048, 4096], **kw).cpu()
    if order == "rise":
        smap = h.rise.saliency
    else:
        a = h.ig.attribution
        smap = (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]                                         # fp32 numpy: two rounded adds
    assert smap.dtype == np.float32 and same_bits(h.score, smap.reshape(B, M, -1)), f"{name}: the score is not the map the result carries"
    assert np.array_equal(h.rank, pixel_order_from_scores(h.score, h.classes, device=False)), f"{name} {order}: not the referee order"


# ------------------------------------------------------------------------------------------------ 6. the tool
def test_tool_at_pixel_resolution_from_a_blurred_canvas(tmp_path):
    import mini_trees
    from protopformer_amd import faithfulness as tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    tree, out, out2 = str(tmp_path / "data"), str(tmp_path / "out"), str(tmp_path / "out2")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    common = ["--data_set", "CUB2011U", "--data_path", tree, "--resume", ck, "--steps", "4", "--max_images", "4", *cellpath.MODEL_FLAGS]
    doc = json.load(open(tool.main(tool.get_args_parser().parse_args(["--output_dir", out, "--resolution", "pixel", "--baseline", "blur", *common]))))
    assert doc["images"] == 4 and doc["counts"] == [0, 12544, 25088, 37632, 50176] and doc["grid_cells"] == 50176
    assert doc["resolution"] == "pixel" and doc["baseline"] == "blur" and doc["blur"] == {"sigma": 5.0, "radius": 5}
    assert set(doc["orders"]) == set(cellpath.MODES) and set(doc["vs_random"]) == {"evidence", "attention"}
    for v in doc["vs_random"].values():
        assert set(v) == {"deletion_auc_minus_random", "insertion_auc_minus_random", "informative"}
    for v in doc["orders"].values():
        assert len(v["deletion"]["curve"]) == 5 and 0.0 <= v["deletion"]["auc"] <= 1.0 and 0.0 <= v["insertion"]["auc"] <= 1.0
    ends = [v["deletion"]["curve"][0] for v in doc["orders"].values()] + [v["insertion"]["curve"][-1] for v in doc["orders"].values()]
    assert max(ends) - min(ends) <= 1e-4 * max(ends)                                         # the untouched image, whatever the order
    plain = json.load(open(tool.main(tool.get_args_parser().parse_args(["--output_dir", out2, *common]))))
    assert not {"resolution", "baseline", "blur"} & set(plain) and plain["counts"] == [0, 49, 98, 147, 196] and plain["grid_cells"] == 196
    assert list(plain) == ["images", "counts", "grid_cells", "orders", "vs_random"]
