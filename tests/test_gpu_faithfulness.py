"""Faithfulness on the GPU: ppf_cell_order, ppf_patch_perturb and ppf_class_prob against the numpy referees of interpret.py
(cell_order_from_outputs / perturb_patches with device=False, fp64 softmax), interpret.faithfulness_curves through the micro models
against the referee pipeline, and the command-line tool on the miniature CUB tree.

Orders, ranks and perturbed images are compared bit for bit; so are the scores wherever the arithmetic fixes them (inputs whose fp64
sums are exact in any order; the attention and the random order).  NaN scores are compared as NaN: the payload of a NaN that an
inf - inf produces is the processor's.  On random real inputs the evidence score is held to the any-order fp64 summation bound
1.01 * P * 2^-53 * sum|term| plus one fp32 rounding of math.fsum, and the order to the sort of the RETURNED scores.  ppf_class_prob is
held to a relative error of (C + 8 + 2 max|l - max l|) * 2^-24: an any-order fp32 sum of C terms, expf's 2 ulp, and the rounded
exponent argument (the kernel sums in fp64, inside the bound)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro, report

pytestmark = pytest.mark.gpu

MODES = ("evidence", "attention", "random")


# ------------------------------------------------------------------------------------------------ generators and comparisons
def make_case(B, P, C, T, G, M, seed, exact=True):
    """Branch outputs as CPU numpy arrays.  exact: activations in multiples of 1/8 below 8, weights in multiples of 1/4 in [-1, 1], scale
    0.5 and attention in multiples of 1/64 -- every sum is exact in any order and ties are frequent; else plain random values."""
    rng = np.random.default_rng(seed)
    if exact:
        act = (rng.integers(0, 64, (B, P, T)) / 8).astype(np.float32)
        w = (rng.integers(-4, 5, (C, P)) / 4).astype(np.float32)
        attn = (rng.integers(0, 16, (B, G)) / 64).astype(np.float32)
        scale = 0.5
    else:
        act = (rng.random((B, P, T)) * 6).astype(np.float32)
        w = np.where(rng.random((C, P)) < 0.25, rng.standard_normal((C, P)), -0.5).astype(np.float32)
        attn = rng.random((B, G)).astype(np.float32)
        scale = 0.7
    idx = np.stack([np.sort(rng.permutation(G)[:T]) for _ in range(B)]).astype(np.int32)
    return dict(act_full=act, idx=idx, token_attn=attn, weight=w, scale=scale, classes=rng.integers(0, C, (B, M)).astype(np.int32), grid_cells=G)


def run_order(c, mode, device, **kw):
    from protopformer_amd.interpret import cell_order_from_outputs
    a = {k: (torch.from_numpy(v).cuda() if device and isinstance(v, np.ndarray) else v) for k, v in {**c, **kw}.items()}
    out = cell_order_from_outputs(mode=mode, device=device, **a)
    if device:
        torch.cuda.synchronize()
        out = tuple(t.cpu().numpy() for t in out)
    return out


def same_bits(a, b):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def check_order(c, mode, what, **kw):
    got, ref = run_order(c, mode, True, **kw), run_order(c, mode, False, **kw)
    for name, g, r in zip(("order", "rank", "score"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype, f"{what} {mode}: {name} is {g.shape} {g.dtype}"
    assert same_bits(got[2], ref[2]), f"{what} {mode}: the score bits differ from the referee"
    assert np.array_equal(got[0], ref[0]), f"{what} {mode}: order differs from the referee"
    assert np.array_equal(got[1], ref[1]), f"{what} {mode}: rank differs from the referee"
    return got


def order_of_scores(score, tier):
    """The contract's sort of given scores [G]: tier ascending, NaN last within the tier, score descending, smaller cell."""
    nan = np.isnan(score)
    return np.lexsort((np.arange(score.size), np.where(nan, np.float32(0), -score), nan, tier))


# ------------------------------------------------------------------------------------------------ 1. ppf_cell_order, exact cases
@pytest.mark.parametrize("B,P,C,T,G,M", [(3, 12, 4, 9, 16, 2), (2, 40, 5, 81, 196, 1), (1, 2000, 200, 81, 196, 8), (2, 12, 4, 196, 196, 2), (3, 12, 4, 1, 16, 2),
                                         (2, 67, 4, 9, 16, 2), (2, 30, 4, 300, 1024, 3)],
                         ids=["small", "T81_G196", "P2000_M8", "T_eq_G", "T1", "P67", "G1024"])
@pytest.mark.parametrize("mode", MODES)
def test_cell_order_equals_the_referee_bit_for_bit(B, P, C, T, G, M, mode):
    c = make_case(B, P, C, T, G, M, seed=B + P + T)
    order, rank, score = check_order(c, mode, f"B={B} P={P} T={T} G={G} M={M}", seed=5, image_ids=np.arange(100, 100 + B))
    assert (np.sort(order, axis=-1) == np.arange(G)).all() and (np.take_along_axis(rank, order, -1) == np.arange(G)).all()
    if mode == "evidence":
        for b in range(B):
            assert (np.sort(order[b, :, :T], axis=-1) == c["idx"][b]).all()           # the reserved cells come first (nothing else when T == G)


def test_cell_order_adversarial_rows():
    inf = np.float32(np.inf)
    c = make_case(4, 12, 4, 9, 16, 3, seed=1)
    c["act_full"][0, :, 0], c["act_full"][0, 3, 1], c["act_full"][0, 5, 2] = np.nan, inf, -inf          # NaN, +inf and -inf evidence
    c["weight"][:, 3], c["weight"][:, 5] = 1.0, 0.5                                                       # (no inf * 0)
    unres = np.setdiff1d(np.arange(16), c["idx"][0])
    c["token_attn"][0, unres[:4]] = (np.nan, inf, -inf, np.nan)
    c["idx"][1] = (2, 2, 5, -1, 16, 99, 5, 7, 2)                                                          # repeated cells, entries off the grid
    c["classes"][2] = (-1, 4, 1 << 30)                                                                    # classes -1 and >= C
    c["classes"][1, 1] = -7
    c["act_full"][3], c["weight"][:], c["token_attn"][3] = 1.0, 1.0, 0.25                                 # all scores equal
    for mode in MODES:
        order, rank, score = check_order(c, mode, "adversarial", seed=1, image_ids=np.array([3, 1, 4, 1]))
        assert (order[2] == -1).all() and (rank[2] == -1).all() and (score[2] == 0).all() and (order[1, 1] == -1).all()
        assert (order[1, 0] >= 0).all() and (order[3] >= 0).all()
        if mode == "attention":
            assert (order[3] == np.arange(16)).all()
            assert order[0, 0, 0] == unres[1] and order[0, 0, -3:].tolist() == [unres[2], unres[0], unres[3]]     # +inf first; -inf, then the NaNs by cell
        if mode == "evidence":
            res = c["idx"][3].tolist()
            assert (order[3] == np.array(res + [g for g in range(16) if g not in res])).all()
            assert set(order[1, 0, :3].tolist()) == {2, 5, 7} and (np.sort(order[1, 0, 3:]) == np.setdiff1d(np.arange(16), [2, 5, 7])).all()
            r0 = c["idx"][0]
            assert order[0, 0, 0] == r0[1] and order[0, 0, 7:9].tolist() == [r0[2], r0[0]]                        # +inf, ..., -inf, NaN within tier 0
            assert order[0, 0, 9] == unres[1] and order[0, 0, -3:].tolist() == [unres[2], unres[0], unres[3]]


# ------------------------------------------------------------------------------------------------ 2. ppf_cell_order, random real inputs
@pytest.mark.parametrize("B,P,C,T,G,M", [(2, 300, 10, 9, 16, 2), (1, 2000, 200, 81, 196, 2), (2, 67, 4, 25, 36, 3)], ids=["P300", "P2000", "P67"])
def test_cell_order_scores_within_the_fp64_bound_and_order_is_the_sort_of_the_scores(B, P, C, T, G, M):
    c = make_case(B, P, C, T, G, M, seed=P, exact=False)
    order, rank, score = run_order(c, "evidence", True)
    w = (np.float32(c["scale"]) * c["weight"]).astype(np.float32).astype(np.float64)
    worst = 0.0
    for b in range(B):
        tier = np.ones(G, dtype=np.int64)
        tier[c["idx"][b]] = 0
        for m in range(M):
            terms = w[c["classes"][b, m]][:, None] * c["act_full"][b].astype(np.float64)               # [P, T], every product exact
            for t in range(T):
                exact = math.fsum(terms[:, t])
                bound = 1.01 * P * 2.0 ** -53 * float(np.abs(terms[:, t]).sum())
                bound += 2.0 ** -24 * (abs(exact) + bound)                                              # the one rounding to fp32
                err = abs(float(score[b, m, c["idx"][b, t]]) - exact)
                worst = max(worst, err / bound)
                assert err <= bound, (b, m, t, err, bound)
            rest = tier == 1
            assert np.array_equal(score[b, m, rest], c["token_attn"][b, rest])
            assert np.array_equal(order[b, m], order_of_scores(score[b, m], tier)), (b, m)
            assert (rank[b, m, order[b, m]] == np.arange(G)).all()
    print(f"P={P}: largest score error / bound = {worst:.3f}")
    report(f"cell_order_score_P{P}", err_over_bound=worst)


# ------------------------------------------------------------------------------------------------ 3. ppf_cell_order, random mode
def test_random_order_depends_on_seed_image_and_cell_alone():
    G, C = 196, 7
    ids = np.array([12, 1 << 40, 7, 99, 3], dtype=np.int64)
    c = dict(act_full=None, idx=None, token_attn=None, weight=np.ones((C, 4), dtype=np.float32), scale=1.0, classes=np.zeros((5, 2), dtype=np.int32), grid_cells=G)
    five = check_order(c, "random", "B=5", seed=(1 << 35) + 11, image_ids=ids)
    assert np.array_equal(five[0][:, 0], five[0][:, 1])                                       # the class does not enter
    assert len({tuple(r) for r in five[0][:, 0].tolist()}) == 5                               # every image its own order
    for j in (0, 1, 4):
        one = check_order({**c, "classes": np.zeros((1, 2), dtype=np.int32)}, "random", "B=1", seed=(1 << 35) + 11, image_ids=ids[j:j + 1])
        assert all(np.array_equal(one[k][0], five[k][j]) for k in range(3))
    perm = np.array([3, 0, 4, 2, 1])
    moved = check_order(c, "random", "permuted", seed=(1 << 35) + 11, image_ids=ids[perm])
    assert all(np.array_equal(moved[k], five[k][perm]) for k in range(3))
    other = run_order(c, "random", True, seed=12, image_ids=ids)
    assert not np.array_equal(other[0], five[0]) and ((five[2] >= 0) & (five[2] < 1)).all()


# ------------------------------------------------------------------------------------------------ 4. ppf_patch_perturb
@pytest.mark.parametrize("size,G", [(64, 16), (224, 196), (32, 64)], ids=["64_G16", "224_G196", "32_G64_patch4"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_patch_perturb_equals_numpy(size, G, tensor_baseline):
    from protopformer_amd.interpret import perturb_patches
    rng = np.random.default_rng(size + G)
    B, M = 2, 2
    x = rng.standard_normal((B, 3, size, size)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else -0.375
    rank = np.stack([np.stack([rng.permutation(G) for _ in range(M)]) for _ in range(B)]).astype(np.int32)
    rank[1, 0] = -1
    counts = [0, 1, 5, G]
    for insertion in (False, True):
        ref = perturb_patches(x, rank, counts, insertion=insertion, baseline=base, device=False)
        got = perturb_patches(torch.from_numpy(x).cuda(), torch.from_numpy(rank).cuda(), counts, insertion=insertion,
                              baseline=torch.from_numpy(base).cuda() if tensor_baseline else base, device=True)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        assert got.shape == ref.shape == (4, B, M, 3, size, size)
        assert np.array_equal(got.view(np.int32), ref.view(np.int32)), f"insertion={insertion}: differs from numpy"
        assert np.array_equal(got[:, 1, 0], np.broadcast_to(x[1], got[:, 1, 0].shape))       # the -1 row copies x
        assert np.array_equal(got[3 if insertion else 0, 0, 0], x[0])


def test_patch_perturb_refuses_a_patch_width_of_two_and_wrong_operands():
    from protopformer_amd import ops
    x = torch.zeros((1, 3, 32, 32), device="cuda")
    counts = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="ppf_patch_perturb.*patch width 2"):
        ops.patch_perturb(x, torch.zeros((1, 1, 256), dtype=torch.int32, device="cuda"), counts)
    rank = torch.zeros((1, 1, 64), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="counts must be torch.int32"):
        ops.patch_perturb(x, rank, counts.long())
    with pytest.raises(ValueError, match="x must be a CUDA tensor"):
        ops.patch_perturb(x.cpu(), rank, counts)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.patch_perturb(x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), rank, counts)
    with pytest.raises(ValueError, match="baseline must be"):
        ops.patch_perturb(x, rank, counts, baseline=torch.zeros((1, 3, 32, 16), device="cuda"))
    with pytest.raises(RuntimeError, match="ppf_cell_order.*G=1025"):
        ops.cell_order(torch.zeros((1, 1), dtype=torch.int32, device="cuda"), 1025, "attention", token_attn=torch.zeros((1, 1025), device="cuda"))
    with pytest.raises(ValueError, match="cls must be torch.int32"):
        ops.class_prob(torch.zeros((2, 3), device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------ 5. ppf_class_prob
def prob_reference(logits, cls):
    """(fp64 softmax probability of the class per row, the relative bound (C + 8 + 2 max|l - max l|) * 2^-24 per row)."""
    l = np.asarray(logits, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = l - l.max(axis=1, keepdims=True)
        e = np.exp(d)
        p = e[np.arange(l.shape[0]), np.clip(cls, 0, l.shape[1] - 1)] / e.sum(axis=1)
        bound = (l.shape[1] + 8 + 2 * np.abs(d).max(axis=1)) * 2.0 ** -24
    return p, bound


@pytest.mark.parametrize("C", [2, 10, 200, 1000])
def test_class_prob_against_fp64(C):
    from protopformer_amd import ops
    rng = np.random.default_rng(C)
    R = 67                                                                                    # no multiple of the rows of a workgroup
    logits = (rng.random((R, C)) * 32 - 16).astype(np.float32)
    logits[1] = 3.0                                                                           # a flat row: 1 / C
    cls = rng.integers(0, C, R).astype(np.int32)
    cls[0], cls[2] = C - 1, 0
    got = ops.class_prob(torch.from_numpy(logits).cuda(), torch.from_numpy(cls).cuda()).cpu().numpy()
    ref, bound = prob_reference(logits, cls)
    rel = np.abs(got.astype(np.float64) - ref) / ref
    print(f"C={C}: largest relative error / bound = {(rel / bound).max():.3f}")
    report(f"class_prob_C{C}", err_over_bound=(rel / bound).max())
    assert got.dtype == np.float32 and (rel <= bound).all(), (rel / bound).max()
    # NaN rows and classes outside [0, C) give NaN, and only there
    logits[5, C // 2], cls[7], cls[9] = np.nan, -1, C
    got = ops.class_prob(torch.from_numpy(logits).cuda(), torch.from_numpy(cls).cuda()).cpu().numpy()
    bad = np.zeros(R, dtype=bool)
    bad[[5, 7, 9]] = True
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()


# ------------------------------------------------------------------------------------------------ 6. through the micro models
def forward_logits(m, imgs, bs):
    """The model's eval logits of imgs [N, 3, H, W] (host array), forwarded in consecutive sub-batches of bs images."""
    with torch.no_grad():
        parts = [m._branches(torch.from_numpy(np.ascontiguousarray(imgs[i:i + bs])).cuda(), want_dist=False).logits for i in range(0, len(imgs), bs)]
        return torch.cat(parts).cpu().numpy()


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_curves_equal_the_referee_pipeline(fixture):
    from protopformer_amd.interpret import cell_order_from_outputs, default_counts, faithfulness_curves, perturb_patches
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda()
    B, M, G, coe = x.shape[0], 2, 16, cfg["global_coe"]
    bs = B * M                                                       # a sub-batch is one step: every (sample, class) image at one count
    f = faithfulness_curves(m, x, top_classes=M, batch_size=bs)
    h = f.cpu()
    counts = default_counts(G)
    S = len(counts)
    assert np.array_equal(h.counts, counts) and h.classes.shape == (B, M) and (h.classes >= 0).all() and set(h.curves) == {"deletion", "insertion"}
    with torch.no_grad():
        r = m._branches(x, want_dist=False)
    attn, idx, act_full, logits = r.cls_attn, r.idx, r.act_full, r.logits
    assert np.array_equal(h.classes[:, 0], logits.argmax(1).cpu().numpy())
    order, rank, score = cell_order_from_outputs(act_full, idx, attn, m.last_layer.weight.detach(), 1.0 - coe, h.classes, G, device=False)
    assert np.array_equal(h.order, order) and np.array_equal(h.rank, rank) and same_bits(h.score, score), f"{fixture}: the order differs from the referee"
    clean = forward_logits(m, np.repeat(z["img"], M, axis=0), bs)                          # the batch of step 'nothing removed': each image M times
    blank = forward_logits(m, np.zeros((bs,) + z["img"].shape[1:], dtype=np.float32), bs)   # the batch of step 'everything removed'
    cls = h.classes.reshape(-1)
    p_clean, b_clean = prob_reference(clean, cls)
    p_blank, b_blank = prob_reference(blank, cls)
    worst = 0.0
    for mode in ("deletion", "insertion"):
        imgs = perturb_patches(z["img"], rank, counts, insertion=mode == "insertion", device=False)
        ref_logits = forward_logits(m, imgs.reshape((-1,) + imgs.shape[3:]), bs)
        ref, bound = prob_reference(ref_logits, np.tile(cls, S))
        got = h.curves[mode].transpose(2, 0, 1).reshape(-1).astype(np.float64)            # [S, B, M]
        rel = np.abs(got - ref) / ref
        worst = max(worst, float((rel / bound).max()))
        assert (rel <= bound).all(), f"{fixture} {mode}: off the referee pipeline by {(rel / bound).max():.2f} bounds"
        ends = h.curves[mode].reshape(bs, S).astype(np.float64)
        full, none = (ends[:, 0], ends[:, -1]) if mode == "deletion" else (ends[:, -1], ends[:, 0])
        assert (np.abs(full - p_clean) <= b_clean * p_clean).all(), f"{fixture} {mode}: the untouched end is not the unperturbed probability"
        assert (np.abs(none - p_blank) <= b_blank * p_blank).all(), f"{fixture} {mode}: the emptied end is not the all-baseline probability"
    ends_bitwise = bool(np.array_equal(h.curves["deletion"][..., 0].view(np.int32), h.curves["insertion"][..., -1].view(np.int32)) and
                        np.array_equal(h.curves["deletion"][..., -1].view(np.int32), h.curves["insertion"][..., 0].view(np.int32)))
    print(f"{fixture}: largest curve error / bound = {worst:.3f}; the curves' ends bitwise equal across the modes: {ends_bitwise}")
    report(f"faithfulness_curves_{fixture}", err_over_bound=worst, ends_bitwise_equal=ends_bitwise)
    again = faithfulness_curves(m, x, top_classes=M, batch_size=bs)
    assert all(torch.equal(again.curves[k], f.curves[k]) for k in f.curves) and torch.equal(again.order, f.order) and torch.equal(again.score, f.score)
    auc = h.auc()
    assert auc["deletion"].shape == (B, M) and auc["deletion"].dtype == np.float64 and ((auc["deletion"] >= 0) & (auc["deletion"] <= 1)).all()
    # other orders, given classes, a tensor baseline and a scratch bound of one step: the same ends
    g = faithfulness_curves(m, x, classes=h.classes, order="random", image_ids=[5, 6, 7, 8], baseline=torch.zeros_like(x), batch_size=bs, scratch_bytes=1).cpu()
    assert (np.abs(g.curves["deletion"].reshape(bs, S)[:, 0].astype(np.float64) - p_clean) <= b_clean * p_clean).all()
    assert not np.array_equal(g.order, h.order) and (np.sort(g.order, -1) == np.arange(G)).all()
    assert (np.abs(g.curves["deletion"].reshape(bs, S)[:, -1].astype(np.float64) - p_blank) <= b_blank * p_blank).all()
    assert not m.training


# ------------------------------------------------------------------------------------------------ 7. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def test_tool_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd import data as D
    from protopformer_amd import faithfulness as tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    tree, out = str(tmp_path / "data"), str(tmp_path / "out")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", out, "--resume", ck, "--steps", "4",
                                              "--max_images", "6", "--per-image", *MODEL_FLAGS])
    path = tool.main(args)
    doc = json.load(open(path))
    assert path == os.path.join(out, "faithfulness.json") and doc["images"] == 6 and doc["counts"] == [0, 49, 98, 147, 196] and doc["grid_cells"] == 196
    assert set(doc["orders"]) == set(MODES) and all(set(v) == {"deletion", "insertion"} for v in doc["orders"].values())
    assert set(doc["vs_random"]) == {"evidence", "attention"}
    for v in doc["vs_random"].values():
        assert set(v) == {"deletion_auc_minus_random", "insertion_auc_minus_random", "informative"}
    # the unperturbed probability of the same six images, through the same loader and the same batches
    view = D.build_view_transform(args)
    ds, _ = D.build_dataset(False, args, transform=view)
    ds.return_id = True
    seen, probs, worst, ids = 0, [], 0.0, []
    m.eval()
    for x, y, i in D.DeviceLoader(ds, 4, torch.device("cuda"), D.GpuFinisher(re_prob=0.0), shuffle=False, num_workers=0):
        x, i = x[:6 - seen], i[:6 - seen]
        with torch.no_grad():
            logits = m._branches(x.float().contiguous(), want_dist=False).logits.cpu().numpy()
        p, b = prob_reference(logits, logits.argmax(1))
        probs += p.tolist(); ids += torch.as_tensor(i).tolist()
        worst = max(worst, float(b.max()))
        seen += x.shape[0]
        if seen >= 6:
            break
    mean = float(np.mean(probs))
    z = np.load(os.path.join(out, "faithfulness.npz"))
    assert z["image_ids"].tolist() == ids and z["classes"].shape == (6, 1) and z["counts"].tolist() == doc["counts"]
    test_ids = [i for i, c, t in mini_trees.CUB_ROWS if t == 0 and i not in mini_trees.CUB_NO_LABEL]
    assert set(ids) <= set(test_ids) and len(set(ids)) == 6
    for order in MODES:
        d, i = doc["orders"][order]["deletion"], doc["orders"][order]["insertion"]
        assert len(d["curve"]) == len(i["curve"]) == 5 and 0.0 <= d["auc"] <= 1.0 and 0.0 <= i["auc"] <= 1.0
        assert abs(d["curve"][0] - mean) <= worst * mean and abs(i["curve"][-1] - mean) <= worst * mean, (order, d["curve"][0], i["curve"][-1], mean)
        assert abs(d["curve"][-1] - i["curve"][0]) <= 2 * worst * d["curve"][-1]                                   # both are the all-baseline image
        assert z[f"{order}_deletion"].shape == (6, 1, 5)
        assert np.allclose(z[f"{order}_deletion"].astype(np.float64).mean((0, 1)), d["curve"], rtol=1e-12, atol=0)
    ev = doc["vs_random"]["evidence"]
    assert ev["deletion_auc_minus_random"] == doc["orders"]["evidence"]["deletion"]["auc"] - doc["orders"]["random"]["deletion"]["auc"]
