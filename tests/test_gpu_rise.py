"""RISE saliency on the GPU: ppf_rise_nodes, ppf_rise_apply and ppf_rise_accumulate against the numpy referees of interpret.py
(rise_nodes_from_ids / rise_apply / rise_accumulate with device=False), interpret.rise_saliency and the 'rise' order of
faithfulness_curves through the micro models against the referee pipeline, and the command-line tool on the miniature CUB tree.

The masks are integer-exact (the contract in include/ppf_hip.h), so node tables, masked images, saliency maps and cell scores are
compared bit for bit.  The class probabilities in between come from the model's forward and ppf_class_prob and are held to that
kernel's bound, a relative error of (C + 8 + 2 max|l - max l|) * 2^-24 (tests/test_gpu_faithfulness.py)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

IDS = np.array([5, (1 << 40) + 3, 0], dtype=np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def tables(ids, H, s, N, p=0.5, seed=0):
    from protopformer_amd.interpret import rise_nodes_from_ids
    return rise_nodes_from_ids(ids, H, N, s, p, seed, device=False)


# ------------------------------------------------------------------------------------------------ 1. ppf_rise_nodes
@pytest.mark.parametrize("s", [2, 3, 7, 14])
@pytest.mark.parametrize("N", [1, 65, 300])
def test_nodes_equal_the_referee(N, s):
    from protopformer_amd.interpret import rise_nodes_from_ids
    H = 224 if s == 7 else 32 if s == 3 else 64 if s == 2 else 56
    for p, seed in ((0.5, (1 << 35) + 11), (0.125, 3)):
        nodes, shift = rise_nodes_from_ids(dev(IDS), H, N, s, p, seed)
        ref_nodes, ref_shift = tables(IDS, H, s, N, p, seed)
        assert nodes.dtype == torch.uint8 and shift.dtype == torch.int32 and tuple(nodes.shape) == (3, N, (s + 2) ** 2) and tuple(shift.shape) == (3, N, 2)
        assert np.array_equal(nodes.cpu().numpy(), ref_nodes), f"N={N} s={s} p={p}: nodes differ from the referee"
        assert np.array_equal(shift.cpu().numpy(), ref_shift), f"N={N} s={s} p={p}: shifts differ from the referee"
    one = rise_nodes_from_ids(dev(IDS[1:2]), H, N, s, 0.125, 3)                                   # the batch does not enter
    assert torch.equal(one[0][0], nodes[1]) and torch.equal(one[1][0], shift[1])


# ------------------------------------------------------------------------------------------------ 2. ppf_rise_apply
@pytest.mark.parametrize("H,s,N,n0,Nc", [(32, 3, 7, 0, 7), (32, 3, 7, 2, 5), (64, 2, 6, 1, 4), (64, 4, 6, 3, 3), (224, 7, 5, 1, 3), (32, 3, 530, 9, 521)],
                         ids=["32_s3_all", "32_s3_tail", "64_s2_middle", "64_s4_tail", "224_s7_Nc3", "two_lds_stages"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_apply_equals_the_referee_bit_for_bit(H, s, N, n0, Nc, tensor_baseline):
    from protopformer_amd.interpret import rise_apply
    rng = np.random.default_rng(H + s + N)
    B, Cc = (1, 2) if N > 500 else (2, 3)                       # a channel count below, and at, what a thread owns
    x = rng.standard_normal((B, Cc, H, H)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else -0.375
    nodes, shift = tables(IDS[:B], H, s, N, seed=7)
    assert (shift[:, n0:n0 + Nc] % 2 == 1).any()                                                 # odd shifts: vectors straddle node boundaries
    ref = rise_apply(x, nodes, shift, s, n0, Nc, base, device=False)
    got = rise_apply(dev(x), dev(nodes), dev(shift), s, n0, Nc, dev(base) if tensor_baseline else base)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == ref.shape == (Nc, B, Cc, H, H)
    assert np.array_equal(bits(got), bits(ref)), f"{int((bits(got) != bits(ref)).sum())} of {got.size} elements differ from the referee"


def test_apply_other_channel_counts_out_buffer_and_all_nodes_on():
    from protopformer_amd import ops
    from protopformer_amd.interpret import rise_apply
    rng = np.random.default_rng(1)
    H, s = 32, 3
    nodes, shift = tables(IDS, H, s, 4)
    for Cc in (1, 4, 7):                                        # one thread owns three channels: a partial and several groups
        x = rng.standard_normal((3, Cc, H, H)).astype(np.float32)
        got = rise_apply(dev(x), dev(nodes), dev(shift), s, baseline=0.5).cpu().numpy()
        assert np.array_equal(bits(got), bits(rise_apply(x, nodes, shift, s, baseline=0.5, device=False))), f"Cc={Cc}"
    x = dev(rng.standard_normal((3, 3, H, H)).astype(np.float32))
    buf = torch.full((6, 3, 3, H, H), 7.0, device="cuda")
    out = ops.rise_apply(x, dev(nodes), dev(shift), s, 1, 2, 0.0, out=buf[:2])
    assert out.data_ptr() == buf.data_ptr() and bool((buf[2:] == 7.0).all())                    # nothing past the chunk is written
    assert torch.equal(out, ops.rise_apply(x, dev(nodes), dev(shift), s, 1, 2, 0.0))
    full, sh = tables(IDS, H, s, 2, p=1.0)
    assert torch.equal(ops.rise_apply(x, dev(full), dev(sh), s, baseline=3.0), torch.stack([x, x]))
    with pytest.raises(RuntimeError, match="ppf_rise_apply.*n0=3"):
        ops.rise_apply(x, dev(nodes), dev(shift), s, 3, 2)
    with pytest.raises(ValueError, match="nodes must be torch.uint8"):
        ops.rise_apply(x, dev(nodes).int(), dev(shift), s)
    with pytest.raises(ValueError, match="shift must be"):
        ops.rise_apply(x, dev(nodes), dev(shift)[:, :3], s)
    with pytest.raises(ValueError, match="out must be"):
        ops.rise_apply(x, dev(nodes), dev(shift), s, 0, 2, out=buf[:3])


# ------------------------------------------------------------------------------------------------ 3. ppf_rise_accumulate
@pytest.mark.parametrize("H,s,G,N,M", [(32, 3, 64, 9, 3), (64, 4, 16, 9, 2), (224, 7, 196, 8, 2), (32, 3, 64, 1100, 2), (64, 2, 16, 1, 1), (32, 3, 16, 5, 8),
                                       (64, 4, 1024, 4, 1)],
                         ids=["32_s3_G64", "64_s4_G16", "224_s7_G196", "three_lds_stages", "N1_M1", "M8", "G1024_patch2"])
def test_accumulate_equals_the_ascending_fp64_sum_bit_for_bit(H, s, G, N, M):
    from protopformer_amd.interpret import rise_accumulate
    rng = np.random.default_rng(H + G + N)
    B, p = (2, 0.375) if N > 1000 else (3, 0.5)
    nodes, shift = tables(IDS[:B], H, s, N, p=p, seed=11)
    prob = rng.random((N, B, M)).astype(np.float32)
    ref_sal, ref_cell = rise_accumulate(nodes, shift, prob, H, s, G, p, device=False)
    sal, cell = rise_accumulate(dev(nodes), dev(shift), dev(prob), H, s, G, p)
    torch.cuda.synchronize()
    sal, cell = sal.cpu().numpy(), cell.cpu().numpy()
    assert sal.shape == (B, M, H, H) and cell.shape == (B, M, G)
    assert np.array_equal(bits(sal), bits(ref_sal)), f"sal: {int((bits(sal) != bits(ref_sal)).sum())} of {sal.size} elements differ from the referee"
    assert np.array_equal(bits(cell), bits(ref_cell)), f"cell: {int((bits(cell) != bits(ref_cell)).sum())} of {cell.size} elements differ from the referee"


def test_accumulate_nan_probability_marks_its_row_alone():
    from protopformer_amd.interpret import rise_accumulate
    H, s, G, N, B, M = 32, 3, 64, 6, 3, 3
    nodes, shift = tables(IDS, H, s, N)
    prob = np.random.default_rng(0).random((N, B, M)).astype(np.float32)
    clean = [t.cpu().numpy() for t in rise_accumulate(dev(nodes), dev(shift), dev(prob), H, s, G)]
    prob[:, 1, 2] = np.nan                                                                        # an invalid class: its whole column
    prob[4, 2, 0] = np.nan                                                                        # a single NaN
    sal, cell = (t.cpu().numpy() for t in rise_accumulate(dev(nodes), dev(shift), dev(prob), H, s, G))
    bad = np.zeros((B, M), dtype=bool)
    bad[1, 2] = bad[2, 0] = True
    assert np.isnan(sal[bad]).all() and np.isnan(cell[bad]).all()
    assert np.array_equal(bits(sal[~bad]), bits(clean[0][~bad])) and np.array_equal(bits(cell[~bad]), bits(clean[1][~bad]))
    ref = rise_accumulate(nodes, shift, prob, H, s, G, device=False)
    assert same_bits(sal, ref[0]) and same_bits(cell, ref[1])


# ------------------------------------------------------------------------------------------------ 4. through the micro models
def prob_reference(logits, cls):
    """(fp64 softmax probability of the class per row, the relative bound (C + 8 + 2 max|l - max l|) * 2^-24 per row)."""
    l = np.asarray(logits, dtype=np.float64)
    d = l - l.max(axis=1, keepdims=True)
    e = np.exp(d)
    return e[np.arange(l.shape[0]), cls] / e.sum(axis=1), (l.shape[1] + 8 + 2 * np.abs(d).max(axis=1)) * 2.0 ** -24


def forward_logits(m, imgs, bs):
    """The model's eval logits of imgs [R, 3, H, W] (host array), forwarded in consecutive sub-batches of bs images."""
    with torch.no_grad():
        return torch.cat([m._branches(dev(imgs[i:i + bs]), want_dist=False).logits for i in range(0, len(imgs), bs)]).cpu().numpy()


@pytest.fixture(scope="module", params=["micro_deit.npz", "micro_cait.npz"])
def model_case(request):
    """One model, one rise_saliency call and its host copy, shared by the tests below and left unchanged."""
    from protopformer_amd.interpret import rise_saliency
    sd, cfg, z = micro(request.param)
    m = build_micro(cfg, sd).eval()
    x = dev(z["img"])
    r = rise_saliency(m, x, top_classes=2, masks=24, cells=2, batch_size=x.shape[0])
    return dict(name=request.param, m=m, x=x, img=z["img"], r=r, h=r.cpu())


def test_rise_saliency_equals_the_referee_pipeline(model_case):
    from protopformer_amd.interpret import rise_accumulate, rise_apply
    m, img, h, name = model_case["m"], model_case["img"], model_case["h"], model_case["name"]
    B, M, N, G, s, H = img.shape[0], 2, 24, 16, 2, 64
    assert h.saliency.shape == (B, M, H, H) and h.cell.shape == (B, M, G) and h.prob.shape == (N, B, M) and h.classes.shape == (B, M)
    ref_nodes, ref_shift = tables(np.arange(B), H, s, N)
    assert np.array_equal(h.nodes, ref_nodes) and np.array_equal(h.shift, ref_shift), f"{name}: the node tables differ from the referee"
    logits = forward_logits(m, img, B)
    assert (h.classes >= 0).all() and np.array_equal(h.classes[:, 0], logits.argmax(1))
    imgs = rise_apply(img, ref_nodes, ref_shift, s, device=False)                                # [N, B, 3, H, W]: a sub-batch is one mask
    ref_logits = forward_logits(m, imgs.reshape((-1,) + imgs.shape[2:]), B)
    worst = 0.0
    for k in range(M):
        ref, bound = prob_reference(ref_logits, np.tile(h.classes[:, k], N))
        rel = np.abs(h.prob[:, :, k].reshape(-1).astype(np.float64) - ref) / ref
        worst = max(worst, float((rel / bound).max()))
        assert (rel <= bound).all(), f"{name} class column {k}: off the referee pipeline by {(rel / bound).max():.2f} bounds"
    print(f"{name}: largest probability error / bound = {worst:.3f}")
    sal, cell = rise_accumulate(ref_nodes, ref_shift, h.prob, H, s, G, device=False)
    assert np.array_equal(bits(h.saliency), bits(sal)), f"{name}: the saliency differs from the referee fed the returned probabilities"
    assert np.array_equal(bits(h.cell), bits(cell)), f"{name}: the cell scores differ from the referee fed the returned probabilities"
    assert np.isfinite(h.saliency).all() and (h.saliency >= 0).all() and h.saliency.std() > 0


def test_rise_saliency_repeats_and_does_not_depend_on_the_chunk_or_the_mode(model_case):
    from protopformer_amd.interpret import Rise, rise_saliency
    m, x, r = model_case["m"], model_case["x"], model_case["r"]
    kw = dict(top_classes=2, masks=24, cells=2, batch_size=x.shape[0])
    for what, other in (("a second call", rise_saliency(m, x, **kw)), ("one mask per chunk", rise_saliency(m, x, scratch_bytes=1, **kw))):
        for f in Rise.FIELDS:
            assert torch.equal(getattr(other, f), getattr(r, f)), f"{what}: {f} differs"
    assert not m.training
    m.train()
    try:
        again = rise_saliency(m, x, **kw)
        assert m.training, "the model was found in train mode and must be left in it"
    finally:
        m.eval()
    assert torch.equal(again.prob, r.prob) and torch.equal(again.saliency, r.saliency)           # eval-mode forwards either way
    # an image's result depends on its id, not on its place: the first two images alone, in reverse order
    part = rise_saliency(m, x[:2].flip(0), classes=r.classes[:2].flip(0), image_ids=[1, 0], masks=24, cells=2, batch_size=2)
    assert torch.equal(part.nodes, r.nodes[:2].flip(0)) and torch.equal(part.shift, r.shift[:2].flip(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rise_saliency(m, x.cpu())


def order_of_scores(score):
    """The contract's sort of given scores [G]: NaN last, score descending, smaller cell."""
    nan = np.isnan(score)
    return np.lexsort((np.arange(score.size), np.where(nan, np.float32(0), -score), nan))


def test_the_rise_order_of_the_faithfulness_curves(model_case):
    from protopformer_amd.interpret import default_counts, faithfulness_curves
    m, x, img, h, name = model_case["m"], model_case["x"], model_case["img"], model_case["h"], model_case["name"]
    B, M, G = img.shape[0], 2, 16
    f = faithfulness_curves(m, x, top_classes=M, batch_size=B, order="rise", rise=dict(masks=24, cells=2))
    assert f.rise is not None and torch.equal(f.score, f.rise.cell), "score must be Rise.cell, bit for bit"
    g = f.cpu()
    assert np.array_equal(bits(g.score), bits(g.rise.cell)) and np.array_equal(bits(g.rise.cell), bits(h.cell)), f"{name}: not the cells of rise_saliency"
    assert np.array_equal(g.classes, h.classes) and np.array_equal(g.counts, default_counts(G)) and set(g.curves) == {"deletion", "insertion"}
    for b in range(B):
        for k in range(M):
            assert np.array_equal(g.order[b, k], order_of_scores(g.score[b, k])), (b, k)
            assert (g.rank[b, k, g.order[b, k]] == np.arange(G)).all()
    S = len(g.counts)
    cls = g.classes.reshape(-1)
    # a step's images are ordered (sample, class) and were forwarded in sub-batches of B, as here
    p_clean, b_clean = prob_reference(forward_logits(m, np.repeat(img, M, axis=0), B), cls)
    p_blank, b_blank = prob_reference(forward_logits(m, np.zeros((B * M,) + img.shape[1:], dtype=np.float32), B), cls)
    for mode in ("deletion", "insertion"):
        ends = g.curves[mode].reshape(B * M, S).astype(np.float64)
        full, none = (ends[:, 0], ends[:, -1]) if mode == "deletion" else (ends[:, -1], ends[:, 0])
        assert (np.abs(full - p_clean) <= b_clean * p_clean).all(), f"{name} {mode}: the untouched end is not the unperturbed probability"
        assert (np.abs(none - p_blank) <= b_blank * p_blank).all(), f"{name} {mode}: the emptied end is not the all-baseline probability"
    other = faithfulness_curves(m, x, top_classes=M, batch_size=B)                               # the default order is untouched and carries no Rise
    assert other.rise is None and not torch.equal(other.score, f.score)
    with pytest.raises(ValueError, match="mode must be one of"):
        faithfulness_curves(m, x, order="occlusion")


# ------------------------------------------------------------------------------------------------ 5. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def test_tool_with_the_rise_order_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
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
                                              "--max_images", "6", "--orders", "evidence", "random", "rise", "--rise_masks", "8", *MODEL_FLAGS])
    doc = json.load(open(tool.main(args)))
    assert doc["images"] == 6 and doc["counts"] == [0, 49, 98, 147, 196] and doc["grid_cells"] == 196
    assert list(doc["orders"]) == ["evidence", "random", "rise"] and all(set(v) == {"deletion", "insertion"} for v in doc["orders"].values())
    assert set(doc["vs_random"]) == {"evidence", "rise"}
    for v in doc["vs_random"].values():
        assert set(v) == {"deletion_auc_minus_random", "insertion_auc_minus_random", "informative"}
    rise, ev = doc["orders"]["rise"], doc["orders"]["evidence"]
    for mode in ("deletion", "insertion"):
        assert len(rise[mode]["curve"]) == 5 and 0.0 <= rise[mode]["auc"] <= 1.0
    # the ends do not depend on the order: nothing removed / everything removed (fp32 probabilities of the same images; the bound of
    # ppf_class_prob at C = 200 with logits within 16 of their maximum is below 2e-5 relative)
    for a, b in ((rise["deletion"]["curve"][0], ev["deletion"]["curve"][0]), (rise["insertion"]["curve"][-1], ev["insertion"]["curve"][-1]),
                 (rise["deletion"]["curve"][-1], ev["deletion"]["curve"][-1]), (rise["insertion"]["curve"][0], ev["insertion"]["curve"][0])):
        assert abs(a - b) <= 4e-5 * abs(b), (a, b)
    assert not os.path.exists(os.path.join(out, "faithfulness.npz"))
