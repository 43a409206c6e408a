"""'This looks like that, because ...' on the device: every kernel of csrc/because.hip against its numpy referee, bit for bit
(np.array_equal on the bit patterns); interpret.because end to end on the two micro fixtures against the referee pipeline; the tool on
the miniature CUB tree at two loader batch sizes.  Shapes are the smallest that can still go wrong: B = 3 with an image id above 2^40;
H = W = 32 (16-byte path) and 20 (W % 4 != 0: scalar path, partial tiles); 12 with r = 8 (a window wider than the image); 33 x 17 (one
pixel past the 32 x 16 tile of the bilateral filter in both directions) and 32 x 16 (the tile exactly); unaligned views; both
normalisations; the output inside a larger buffer with sentinels on both sides."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
NORMS = {"unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "imagenet": IMAGENET}
IDS = [5, 2 ** 40 + 17, 2 ** 32 + 5]
SENTINEL = -12345.0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def images(shape, norm, seed=0, specials=True):
    """Normalised images whose de-normalised pixels leave [0, 1] on both sides now and then; with a NaN and both infinities."""
    mean, std = (np.float32(v).reshape(1, 3, 1, 1) for v in NORMS[norm])
    rng = np.random.default_rng(seed)
    v = rng.random(shape, dtype=np.float32) * np.float32(1.3) - np.float32(0.15)
    x = ((v - mean) / std).astype(np.float32)
    if specials:
        x[0, 0, 0, 0], x[0, 1, 1, 1], x[0, 2, 2, 2] = np.nan, np.inf, -np.inf
    return x


def placed(x, offset):
    """(view of x on the device that starts `offset` floats into its allocation, an output view placed alike inside sentinels, the flat
    output buffer).  offset 0 or 4: 16-byte aligned; 1: the scalar path."""
    n = x.size
    src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    src[offset:offset + n] = torch.from_numpy(x).reshape(-1).cuda()
    flat = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    return src[offset:offset + n].view(x.shape), flat[offset:offset + n].view(x.shape), flat


def check_placed(flat, offset, n, want):
    got = flat.cpu().numpy()
    assert (got[:offset] == SENTINEL).all() and (got[offset + n:] == SENTINEL).all(), "written outside the output view"
    assert same_bits(got[offset:offset + n].reshape(want.shape), want)


SHAPES = [((3, 3, 32, 32), 4), ((3, 3, 20, 20), 0), ((3, 3, 32, 32), 1), ((2, 3, 17, 33), 0)]


# ------------------------------------------------------------------------------------------------ colour
@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("shape,offset", SHAPES)
def test_color_affine_matches_the_referee(shape, offset, norm):
    from protopformer_amd import interpret as I
    mean, std = NORMS[norm]
    x = images(shape, norm, seed=offset)
    xd, out, flat = placed(x, offset)
    off = np.random.default_rng(1).random((shape[0], 3), dtype=np.float32) * np.float32(0.4) - np.float32(0.2)
    for m, o in ((I.saturation_matrix(0.0), None), (I.saturation_matrix(0.3), None), (I.hue_matrix(np.pi), None), (I.hue_matrix(1.0), None),
                 (I.contrast_matrix(0.25), off), (I.contrast_matrix(0.0), off)):
        flat.fill_(SENTINEL)
        got = I.color_affine(xd, m, mean, std, offset=None if o is None else torch.from_numpy(o).cuda(), out=out)
        assert got.data_ptr() == out.data_ptr()
        check_placed(flat, offset, x.size, I.color_affine(x, m, mean, std, offset=o, device=False))
    grey = I.color_affine(xd, I.saturation_matrix(0.0), mean, std).cpu().numpy()
    if norm == "unit":
        assert same_bits(grey[:, 0], grey[:, 1]) and same_bits(grey[:, 1], grey[:, 2])


@pytest.mark.parametrize("norm", sorted(NORMS))
def test_gray_sum_and_contrast_offset_match_the_referee(norm):
    from protopformer_amd import interpret as I
    mean, std = NORMS[norm]
    for shape, offset in SHAPES + [((2, 3, 96, 96), 0)]:                                 # the last: several workgroups per image
        x = images(shape, norm, seed=7)
        xd, _, _ = placed(x, offset)
        total = I.gray_sum(xd, mean, std)
        want = I.gray_sum(x, mean, std, device=False)
        assert total.dtype == torch.int32 and np.array_equal(total.cpu().numpy(), want), (shape, offset)
        for f in (0.0, 0.25, 1.0):
            assert same_bits(I.contrast_offset(total, shape[2:], f).cpu().numpy(), I.contrast_offset(want, shape[2:], f, device=False))
    ones = torch.ones((2, 3, 20, 20), dtype=torch.float32, device="cuda")
    assert I.gray_sum(ones, *NORMS["unit"]).tolist() == [255 * 400] * 2
    # the whole contrast perturbation, device against referee
    x = images((3, 3, 20, 20), norm, seed=8)
    p = dict(mean=mean, std=std)
    assert same_bits(I.because_perturb(torch.from_numpy(x).cuda(), "contrast", p).cpu().numpy(), I.because_perturb(x, "contrast", p, device=False))


# ------------------------------------------------------------------------------------------------ texture
@pytest.mark.parametrize("r", [1, 3, 8])
@pytest.mark.parametrize("shape,offset,norm", [((3, 3, 32, 32), 4, "imagenet"), ((3, 3, 20, 20), 0, "unit"), ((2, 3, 12, 12), 1, "imagenet"),
                                               ((2, 3, 17, 33), 0, "unit"), ((2, 3, 16, 32), 4, "imagenet")])
def test_bilateral_matches_the_referee(shape, offset, norm, r):
    from protopformer_amd import interpret as I
    mean, std = NORMS[norm]
    x = images(shape, norm, seed=r)
    xd, out, flat = placed(x, offset)
    for ws, wr in (I.bilateral_tables(r, 0.6 * r + 0.5, 25.0), I.bilateral_tables(r, 2.0, 4.0)):
        flat.fill_(SENTINEL)
        I.bilateral(xd, ws, wr, mean, std, out=out)
        check_placed(flat, offset, x.size, I.bilateral(x, ws, wr, mean, std, device=False))
    # known answers on the device too: the delta tables are the identity on pixels inside [0, 1]
    v = np.random.default_rng(2).random(shape, dtype=np.float32)
    ws = np.zeros((2 * r + 1, 2 * r + 1), dtype=np.float32)
    ws[r, r] = 1.0
    wr = np.zeros(256, dtype=np.float32)
    wr[0] = 1.0
    assert same_bits(I.bilateral(torch.from_numpy(v).cuda(), ws, wr, *NORMS["unit"]).cpu().numpy(), v)
    step = np.full(shape, 0.25, dtype=np.float32)
    step[..., shape[3] // 2:] = 0.75
    full = np.full((2 * r + 1, 2 * r + 1), 0.5, dtype=np.float32)
    assert same_bits(I.bilateral(torch.from_numpy(step).cuda(), full, wr, *NORMS["unit"]).cpu().numpy(), step)


def test_bilateral_refuses_what_it_cannot_do():
    from protopformer_amd import ops
    x = torch.zeros((1, 3, 8, 8), dtype=torch.float32, device="cuda")
    wr = np.ones(256, dtype=np.float32)
    with pytest.raises(RuntimeError, match="radius"):
        ops.bilateral(x, np.ones(19 * 19, dtype=np.float32), wr, 9, *IMAGENET)
    with pytest.raises(RuntimeError, match="out must not be x"):
        ops.bilateral(x, np.ones(9, dtype=np.float32), wr, 1, *IMAGENET, out=x)
    with pytest.raises(RuntimeError, match="finite"):
        ops.bilateral(x, np.full(9, np.nan, dtype=np.float32), wr, 1, *IMAGENET)


# ------------------------------------------------------------------------------------------------ shape
@pytest.mark.parametrize("H,s,offset", [(32, 2, 4), (32, 4, 1), (20, 4, 0), (22, 4, 0), (20, 2, 0)])
def test_warp_matches_the_referee(H, s, offset):
    from protopformer_amd import interpret as I
    c = -(-H // s)
    x = np.random.default_rng(H + s).standard_normal((3, 3, H, H)).astype(np.float32)
    xd, out, flat = placed(x, offset)
    ids = torch.tensor(IDS, dtype=torch.int64)
    for amp in (0, 256 * c // 3, 256 * c + 77, 256 * 3 * c):                             # none, below the node spacing, above it, far above
        nodes = I.warp_nodes_from_ids(ids, s, amp, seed=11)
        want_nodes = I.warp_nodes_from_ids(IDS, s, amp, seed=11, device=False)
        assert nodes.dtype == torch.int32 and np.array_equal(nodes.cpu().numpy(), want_nodes)
        flat.fill_(SENTINEL)
        I.warp_apply(xd, nodes, s, amp, out=out)
        want = I.warp_apply(x, want_nodes, s, amp, device=False)
        check_placed(flat, offset, x.size, want)
        assert same_bits(want, x) == (amp == 0)
    # an image warps the same way in every batch
    alone = I.warp_nodes_from_ids(torch.tensor(IDS[1:2], dtype=torch.int64), s, 500, seed=11).cpu().numpy()
    assert np.array_equal(alone[0], I.warp_nodes_from_ids(IDS, s, 500, seed=11, device=False)[1])
    # amplitude 0 copies -0, infinities and NaN as they are
    x[0, 0, 0, :4] = (-0.0, np.inf, -np.inf, np.nan)
    xs = torch.from_numpy(x).cuda()
    zero = torch.zeros((3, (s + 1) ** 2, 2), dtype=torch.int32, device="cuda")
    assert same_bits(I.warp_apply(xs, zero, s, 0).cpu().numpy(), x)
    # a foreign table is clamped into the amplitude, as the referee's
    wild = torch.full((3, (s + 1) ** 2, 2), 10 ** 6, dtype=torch.int32, device="cuda")
    x[0, 0, 0, :4] = 0
    xs = torch.from_numpy(x).cuda()
    assert same_bits(I.warp_apply(xs, wild, s, 300).cpu().numpy(), I.warp_apply(x, wild.cpu().numpy(), s, 300, device=False))


# ------------------------------------------------------------------------------------------------ score
def test_because_score_matches_the_referee():
    from protopformer_amd import interpret as I
    B, P, T, G, K = 3, 20, 9, 16, 6
    rng = np.random.default_rng(3)
    act_full = rng.random((B, P, T), dtype=np.float32)
    act_full[0, 3, 2] = np.nan
    act_max = np.nanmax(act_full, axis=-1)
    idx = np.stack([np.sort(rng.permutation(G)[:T]) for _ in range(B)]).astype(np.int32)
    idx[1, 4], idx[1, 5] = -1, G + 3                                                     # entries outside the grid are skipped
    protos = rng.integers(0, P, (B, K)).astype(np.int32)
    cells = np.stack([rng.choice(idx[b], K) for b in range(B)]).astype(np.int32)         # kept rows ...
    protos[0, 0], cells[0, 0] = 3, idx[0, 2]                                             # ... one of them the NaN
    cells[0, 1] = next(g for g in range(G) if g not in idx[0])                           # lost: the cell is no longer reserved
    cells[1, 0], cells[1, 1], cells[1, 2] = -1, G + 3, -5                                # out of range, two of them present in idx
    protos[2, 0], protos[2, 1] = -1, P                                                   # prototypes outside the branch
    dev = lambda a: torch.from_numpy(a).cuda()
    want = I.because_score(act_max, protos, G, act_full=act_full, idx=idx, cells=cells, device=False)
    got = I.because_score(dev(act_max), dev(protos), G, act_full=dev(act_full), idx=dev(idx), cells=dev(cells))
    assert want[2].sum() >= 6 and (want[2] == 0).sum() >= 6 and np.isnan(want[0][0, 0]) and want[2][0, 0] == 0
    for g, w in zip(got, want):
        assert same_bits(g.cpu().numpy(), w)
    g_same, g_best, g_lost = I.because_score(dev(act_max), dev(protos))                  # the global branch: best only
    assert g_same is None and g_lost is None and same_bits(g_best.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_because_end_to_end_equals_the_referee_pipeline(fixture):
    from protopformer_amd import interpret as I
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda().float().contiguous()
    B = x.shape[0]
    fields = ("act_full", "idx", "act_max_local", "act_max_global", "logits", "argmax")
    a, b = m.eval_branches(x), m.eval_branches(x)
    for k in fields:                                                                     # the precondition: the eval forward is deterministic
        assert torch.equal(getattr(a, k), getattr(b, k)), f"two eval forwards of the same input differ in {k}"
    ids = [2 ** 40 + 3 + i for i in range(B)]
    params = dict(radius=3, cells=4, amplitude=3.0)
    res = I.because(m, x, seed=3, image_ids=ids, batch_size=2, params=params)
    h = res.cpu()
    n, ppc, T = len(I.CHARACTERISTICS), cfg["protos_per_class"], cfg["reserve_k"]
    G = (cfg["img"] // 16) ** 2
    # the rows of the clean forward
    pred = a.logits.argmax(1).cpu().numpy()
    protos = (pred[:, None] * ppc + np.arange(ppc)[None, :]).astype(np.int32)
    am, ix, base = a.argmax.cpu().numpy(), a.idx.cpu().numpy(), a.act_max_local.cpu().numpy()
    cell = np.take_along_axis(ix, np.take_along_axis(am, protos, 1), 1).astype(np.int32)
    assert np.array_equal(h.protos, protos) and np.array_equal(h.cell, cell) and same_bits(h.base, np.take_along_axis(base, protos, 1))
    assert h.same.shape == h.best.shape == h.lost.shape == (n, B, ppc) and h.characteristics == I.CHARACTERISTICS
    # the referee pipeline: referee images uploaded, the same forward in the same sub-batches, the numpy score
    xh = x.cpu().numpy()
    with m.eval_mode(), torch.no_grad():
        for i, name in enumerate(I.CHARACTERISTICS):
            ref_img = I.because_perturb(xh, name, params, seed=3, image_ids=ids, device=False)
            dev_img = I.because_perturb(x, name, params, seed=3, image_ids=ids)
            assert same_bits(dev_img.cpu().numpy(), ref_img), name
            act_full, idx, act_l, _ = I._because_forward(m, torch.from_numpy(ref_img).cuda(), 2)
            same, best, lost = I.because_score(act_l.cpu().numpy(), protos, G, act_full=act_full.cpu().numpy(), idx=idx.cpu().numpy(), cells=cell,
                                               device=False)
            assert same_bits(h.same[i], same) and same_bits(h.best[i], best) and np.array_equal(h.lost[i], lost), name
    assert (h.lost == 0).any(), "no kept row: the test shows nothing about `same`"
    print(f"{fixture}: kept rows {(h.lost == 0).sum()} of {h.lost.size}; mean local importance of the kept rows per characteristic "
          f"{[float(h.local()[i][h.lost[i] == 0].mean()) if (h.lost[i] == 0).any() else None for i in range(n)]}")
    assert same_bits(h.local(), (h.base[None] - h.same).astype(np.float32))
    rec = h.report(0)
    assert len(rec) == ppc and set(rec[0]) == {"prototype", "cell", "activation", "characteristics"} and set(rec[0]["characteristics"]) == set(I.CHARACTERISTICS)
    json.dumps(rec)
    # a scratch buffer of one image (so forwards of one image each) and chosen prototypes: the same clean rows
    one = I.because(m, x, protos=protos[:, :1], seed=3, image_ids=ids, params=params, scratch_bytes=1, characteristics=("texture", "shape")).cpu()
    assert one.same.shape == (2, B, 1) and np.array_equal(one.cell, cell[:, :1]) and same_bits(one.base, h.base[:, :1])
    # the global branch has no cells
    g = I.because(m, x, branch="global", seed=3, image_ids=ids, characteristics=("hue",)).cpu()
    assert g.same is None and g.lost is None and g.best.shape[:2] == (1, B) and (g.cell == -1).all() and np.isfinite(g.local()).all()
    with pytest.raises(ValueError, match="characteristics"):
        I.because(m, x, characteristics=("size",))
    with pytest.raises(RuntimeError, match="CUDA"):
        I.because(m, x.cpu())


def test_importance_over_a_loader_does_not_depend_on_its_batch_size():
    from protopformer_amd import interpret as I
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda().float()
    x6 = torch.cat([x, x.flip(3), x.flip(2)])[:6].contiguous()
    y6 = torch.arange(6) % cfg["num_classes"]
    ids6 = torch.tensor([9, 2 ** 40, 3, 4, 2 ** 33, 1], dtype=torch.int64)
    loader = lambda bs: [(x6[i:i + bs], y6[i:i + bs], ids6[i:i + bs]) for i in range(0, 6, bs)]
    kw = dict(characteristics=("saturation", "shape"), params=dict(cells=2, amplitude=2.0), seed=1, pass_images=4)
    r2, r3 = (I.characteristic_importance(m, loader(bs), per_image=True, **kw) for bs in (2, 3))
    rows2, rows3 = r2.pop("rows"), r3.pop("rows")
    assert r2 == r3 and r2["images"] == 6 and r2["overall"]["rows"] == 6 * cfg["protos_per_class"]
    assert all(np.array_equal(bits(rows2[k]), bits(rows3[k])) for k in rows2)
    assert np.array_equal(rows2["image_ids"], ids6.numpy()) and np.array_equal(rows2["protos"][:, 0], y6.numpy() * cfg["protos_per_class"])
    want = I.importance_from_rows(rows2["image_ids"], rows2["protos"], rows2["base"], rows2["same"], rows2["best"], rows2["lost"], kw["characteristics"])
    assert want["overall"] == r2["overall"] and want["per_prototype"] == r2["per_prototype"]
    top = I.characteristic_importance(m, loader(3), protos="top", protos_per_image=1, max_images=5, **kw)
    assert top["images"] == 5 and top["overall"]["rows"] == 5
    with pytest.raises(ValueError, match="no image"):
        I.characteristic_importance(m, [], **kw)


# ------------------------------------------------------------------------------------------------ the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--num_workers", "0"]


def test_tool_on_the_miniature_cub_tree_at_two_batch_sizes(tmp_path):
    import mini_trees
    from protopformer_amd import because as tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    tree = str(tmp_path / "data")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    docs = []
    for bs in (2, 3):
        out = str(tmp_path / f"out{bs}")
        extra = ["--per-image", "--save-images", "2"] if bs == 2 else []
        args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", out, "--resume", ck, "--max_images", "6",
                                                  "--pass_images", "4", "--batch_size", str(bs), "--texture_radius", "2", *extra, *MODEL_FLAGS])
        path = tool.main(args)
        assert path == os.path.join(out, "because.json")
        docs.append(json.load(open(path)))
    a, b = docs
    assert a == b, "the loader's batch size changed because.json"
    names = ["hue", "saturation", "contrast", "texture", "shape"]
    assert a["images"] == 6 and a["rows"] == 12 and a["characteristics"] == names and a["branch"] == "local"
    assert a["settings"]["split"] == "train" and a["settings"]["radius"] == 2 and a["settings"]["protos"] == "own"
    assert set(a["overall"]) == {"rows", "importance", "mean", "importance_best", "lost", "dominant"} and a["overall"]["dominant"] in names
    assert all(isinstance(a["overall"]["importance"][k], float) and 0 <= a["overall"]["lost"][k] <= 1 for k in names)
    assert sum(v["rows"] for v in a["per_prototype"].values()) == 12 and all(0 <= int(p) < 400 for p in a["per_prototype"])
    rows = np.load(os.path.join(str(tmp_path / "out2"), "because.npz"))
    assert rows["same"].shape == (5, 6, 2) and rows["image_ids"].shape == (6,) and rows["characteristics"].tolist() == names
    views = sorted(os.listdir(os.path.join(str(tmp_path / "out2"), "views")))
    assert len(views) == 2 * 6 and all(v.endswith(".jpg") for v in views)
