"""Local analysis on the GPU: ppf_explain_topk against the numpy referee (interpret.explain_from_outputs(device=False)), adversarial
inputs, the maps against interpret.expand_to_grid, interpret.explain through the micro models, and the command-line tool.

The kernel performs the referee's two fp32 products and then only moves values, so classes, prototypes, cells, contributions,
activations and maps are compared bit for bit.  The evidence sums are held to the fp32 any-order summation bound
1.01 * P * 2**-24 * sum|contribution| of the fp64 sum (the kernel sums in fp64 and rounds once, far inside it)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import assert_elementwise, build_micro, micro

pytestmark = pytest.mark.gpu

EXACT = ("classes", "class_logits", "prototypes", "cells", "contributions", "activations", "maps")


# ------------------------------------------------------------------------------------------------ generators and the comparison
def make_case(B, P, C, T, G, seed, local=True):
    """Synthetic branch outputs (CPU tensors): activations quantised to 1/8 on even seeds (frequent ties) and plain random on odd ones,
    last-layer weights 1 for the class's own prototypes and -0.5 elsewhere with a random quarter perturbed, logits quantised to 1/4
    (tied classes), and for the local branch argmax [B, P], ascending distinct cells idx [B, T] of a G-cell grid and act_full [B, P, T]."""
    g = torch.Generator().manual_seed(seed)
    ppc = P // C
    act = torch.randint(0, 40, (B, P), generator=g).float() / 8.0 if seed % 2 == 0 else torch.rand((B, P), generator=g) * 6.0
    w = torch.where((torch.arange(P) // ppc)[None, :] == torch.arange(C)[:, None], torch.tensor(1.0), torch.tensor(-0.5))
    w = torch.where(torch.rand((C, P), generator=g) < 0.25, torch.randn((C, P), generator=g), w)
    c = dict(act=act, weight=w.contiguous(), logits=torch.randint(-20, 20, (B, C), generator=g).float() / 4.0, ppc=ppc, scale=1.0 - 0.3, G=G,
             argmax=None, idx=None, act_full=None)
    if local:
        c["argmax"] = torch.randint(0, T, (B, P), generator=g).to(torch.int32)
        c["idx"] = torch.stack([torch.randperm(G, generator=g)[:T].sort().values for _ in range(B)]).to(torch.int32)
        c["act_full"] = torch.rand((B, P, T), generator=g)
    return c


def both(c, K, classes=None, top_classes=1, sign=1, maps=False):
    """(kernel outputs as numpy, referee outputs) of one case."""
    from protopformer_amd.interpret import explain_from_outputs
    dev = lambda t: None if t is None else t.cuda()
    kw = dict(top_classes=top_classes, sign=sign, grid_cells=c["G"], maps=maps)
    got = explain_from_outputs(dev(c["act"]), dev(c["weight"]), c["scale"], c["ppc"], dev(c["logits"]), K, classes=dev(classes), argmax=dev(c["argmax"]),
                               idx=dev(c["idx"]), act_full=dev(c["act_full"]), device=True, **kw)
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in got.items()}
    ref = explain_from_outputs(c["act"], c["weight"], c["scale"], c["ppc"], c["logits"], K, classes=classes, argmax=c["argmax"], idx=c["idx"],
                               act_full=c["act_full"], device=False, **kw)
    return got, ref


def bits(a):
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def evidence_truth(c, classes):
    """fp64 sums of the fp32 contributions, split own / other, and the two masses sum|contribution|: [B, M, 2] each (NaN where a term is)."""
    act, w = c["act"].numpy(), (np.float32(c["scale"]) * c["weight"].numpy()).astype(np.float32)
    B, M = classes.shape
    total, mass = np.zeros((B, M, 2)), np.zeros((B, M, 2))
    with np.errstate(all="ignore"):
        for b in range(B):
            for m in range(M):
                if classes[b, m] < 0:
                    continue
                ctr = (act[b] * w[classes[b, m]]).astype(np.float64)
                own = np.arange(act.shape[1]) // c["ppc"] == classes[b, m]
                total[b, m], mass[b, m] = (ctr[own].sum(), ctr[~own].sum()), (np.abs(ctr[own]).sum(), np.abs(ctr[~own]).sum())
    return total, mass


def check(c, K, what="", **kw):
    got, ref = both(c, K, **kw)
    for k in EXACT:
        if ref[k] is None:
            assert got[k] is None, f"{what}: {k} should be None"
            continue
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, f"{what}: {k} is {got[k].shape} {got[k].dtype}"
        assert np.array_equal(bits(got[k]), bits(ref[k])), f"{what}: {k} differs from the referee"
    P = c["act"].shape[1]
    total, mass = evidence_truth(c, ref["classes"])
    finite = np.isfinite(total)
    assert np.array_equal(np.isfinite(got["evidence"]), finite), f"{what}: evidence is finite where the fp64 sum is not, or the reverse"
    with np.errstate(invalid="ignore"):
        err = np.abs(np.where(finite, got["evidence"].astype(np.float64) - total, 0.0))
    bound = 1.01 * P * 2.0 ** -24 * mass
    print(f"{what}: evidence max err {err.max():.3e}, smallest bound {bound[finite].min() if finite.any() else 0:.3e}")
    assert (err <= np.where(finite, bound, 0.0)).all(), f"{what}: evidence off by {err.max():.3e}"
    return got, ref


# ------------------------------------------------------------------------------------------------ 1. kernel against the referee
@pytest.mark.parametrize("sign", [1, -1], ids=["for", "against"])
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("K", [1, 5, 20, 64])
def test_small_shape_every_k_m_sign(K, M, sign):
    """(B, P, C, T, G) = (3, 20, 10, 9, 16); the kernel picks the classes from tied logits; K = 64 > P leaves unfilled slots."""
    c = make_case(3, 20, 10, 9, 16, seed=K + M)
    got, _ = check(c, K, f"K={K} M={M} sign={sign}", top_classes=M, sign=sign, maps=True)
    assert (got["classes"] >= 0).all() and ((got["prototypes"] >= 0).sum(-1) == min(K, 20)).all()
    if K > 20:
        assert (got["contributions"][..., 20:] == -np.inf).all() and (got["cells"][..., 20:] == -1).all() and (got["maps"][:, :, 20:] == 0).all()


@pytest.mark.parametrize("B,P,C,T,G,K,M", [(2, 130, 10, 4, 9, 7, 3), (2, 2000, 200, 81, 196, 10, 5), (65, 64, 8, 1, 4, 6, 3)],
                         ids=["P130_ppc13", "P2000", "65_lists_T1"])
@pytest.mark.parametrize("given", [False, True], ids=["picked", "given"])
def test_other_shapes(B, P, C, T, G, K, M, given):
    """P no multiple of 64 with ppc = 13; the real prototype count; more lists than a workgroup of four waves would hold, with T = 1."""
    c = make_case(B, P, C, T, G, seed=B + P + (1 if given else 0))
    classes = torch.randint(0, C, (B, M), generator=torch.Generator().manual_seed(5)).to(torch.int32) if given else None
    for sign in (1, -1):
        check(c, K, f"B={B} P={P} given={given} sign={sign}", classes=classes, top_classes=M, sign=sign, maps=True)


def test_global_branch_form():
    """NULL argmax / idx / act_full / maps: the cells are all -1 and no map comes back."""
    c = make_case(5, 40, 10, 1, 1, seed=8, local=False)
    got, _ = check(c, 12, "global", top_classes=4)
    assert got["maps"] is None and (got["cells"] == -1).all() and (got["prototypes"] >= 0).all()


# ------------------------------------------------------------------------------------------------ 2. adversarial inputs
def test_equal_activations_and_weights_come_out_by_ascending_id():
    c = make_case(2, 130, 10, 4, 9, seed=2)
    c["act"][:] = 1.5
    c["weight"][:] = 1.0
    for sign in (1, -1):
        got, _ = check(c, 64, f"all equal, sign={sign}", top_classes=2, sign=sign, maps=True)
        assert (got["prototypes"] == np.arange(64)).all()


def test_tied_logits_pick_the_smaller_class_id():
    c = make_case(3, 20, 10, 9, 16, seed=4)
    c["logits"][0, :] = 2.0                                     # all tied: 0, 1, 2, 3
    c["logits"][1, :] = torch.tensor([1.0, 7.0, 7.0, 1.0, 7.0, 0.0, 1.0, 1.0, -3.0, 7.0])
    c["logits"][2, :] = float("nan")
    c["logits"][2, 6] = float("-inf")                            # one pickable class: the other slots have none
    got, _ = check(c, 5, "tied logits", top_classes=4, maps=True)
    assert got["classes"].tolist() == [[0, 1, 2, 3], [1, 2, 4, 9], [6, -1, -1, -1]]
    assert (got["prototypes"][2, 1:] == -1).all() and (got["evidence"][2, 1:] == 0).all() and (got["maps"][2, 1:] == 0).all()
    assert got["class_logits"][2].tolist() == [float("-inf")] * 4 and (got["prototypes"][2, 0] >= 0).all()


def test_nan_and_inf_activations_are_never_listed_but_stay_in_the_evidence():
    c = make_case(3, 20, 10, 9, 16, seed=6)
    c["act"][0, 3] = float("nan")
    c["act"][0, 11] = float("inf")
    c["act"][2, 5] = float("-inf")
    got, _ = check(c, 20, "planted NaN / inf", top_classes=8, maps=True)
    assert not np.isin(got["prototypes"][0], (3, 11)).any() and not (got["prototypes"][2] == 5).any()
    assert ((got["prototypes"][0] >= 0).sum(-1) == 18).all() and ((got["prototypes"][1] >= 0).sum(-1) == 20).all()
    assert np.isfinite(got["contributions"][got["prototypes"] >= 0]).all()
    assert not np.isfinite(got["evidence"][0]).all(-1).any() and not np.isfinite(got["evidence"][2]).all(-1).any()
    assert np.isfinite(got["evidence"][1]).all()                # ... for the planted rows only


def test_classes_out_of_range_give_unfilled_rows_and_touch_nothing_else():
    c = make_case(3, 20, 10, 9, 16, seed=10)
    classes = torch.tensor([[3, -1, 9], [10, 0, 0], [5, 6, 1 << 30]], dtype=torch.int32)
    got, _ = check(c, 6, "classes out of range", classes=classes, maps=True)
    bad = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], dtype=bool)
    assert (got["classes"][bad] == -1).all() and np.array_equal(got["classes"][~bad], classes.numpy()[~bad])
    assert (got["prototypes"][bad] == -1).all() and (got["cells"][bad] == -1).all() and (got["contributions"][bad] == -np.inf).all()
    assert (got["evidence"][bad] == 0).all() and (got["maps"][bad] == 0).all() and (got["class_logits"][bad] == -np.inf).all()
    assert (got["prototypes"][~bad] >= 0).all()
    clean, _ = both(c, 6, classes=torch.tensor([[3, 3, 9], [0, 0, 0], [5, 6, 6]], dtype=torch.int32), maps=True)
    for k in ("prototypes", "contributions", "cells", "evidence", "maps"):
        assert np.array_equal(bits(clean[k])[~bad], bits(got[k])[~bad]), f"{k}: a valid row changed next to an invalid one"


def test_argmax_outside_the_reserved_tokens_gives_no_cell():
    c = make_case(3, 20, 10, 9, 16, seed=12)
    c["argmax"][0, 4], c["argmax"][1, 7], c["argmax"][2, 0] = 9, -1, 1 << 30
    got, _ = check(c, 20, "argmax == T", top_classes=2, maps=True)
    for b, p in ((0, 4), (1, 7), (2, 0)):
        assert (got["cells"][b][got["prototypes"][b] == p] == -1).all()
    assert ((got["cells"] == -1).sum(-1) == 1).all()


# ------------------------------------------------------------------------------------------------ 3. the maps
def test_maps_equal_expand_to_grid_of_the_selected_prototypes():
    from protopformer_amd.interpret import expand_to_grid
    B, P, C, T, G, K = 3, 20, 10, 9, 16, 24
    c = make_case(B, P, C, T, G, seed=14)
    got, _ = check(c, K, "maps", top_classes=3, maps=True)
    attn = torch.zeros(B, G)
    attn.scatter_(1, c["idx"].long(), 1.0 + torch.rand(B, T))                      # reserved_indices(attn, T) == idx
    grid = expand_to_grid(c["act_full"], attn, T).reshape(B, P, G).numpy()
    for b in range(B):
        for m in range(3):
            for k in range(K):
                p = got["prototypes"][b, m, k]
                want = grid[b, p] if p >= 0 else np.zeros(G, dtype=np.float32)
                assert np.array_equal(bits(got["maps"][b, m, k]), bits(want)), (b, m, k, p)
    assert (got["prototypes"][..., P:] == -1).all() and (got["maps"][:, :, :P] != 0).sum(-1).min() == T


def test_binding_rejects_what_the_kernel_cannot_take():
    from protopformer_amd import ops
    c = make_case(3, 20, 10, 9, 16, seed=1)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    with pytest.raises(RuntimeError, match="ppf_explain_topk.*K=65"):
        ops.explain_topk(d["act"], d["weight"], 0.5, 2, d["logits"], 65)
    with pytest.raises(RuntimeError, match="ppf_explain_topk.*M=9"):
        ops.explain_topk(d["act"], d["weight"], 0.5, 2, d["logits"], 5, top_classes=9)
    with pytest.raises(ValueError, match="argmax and idx"):
        ops.explain_topk(d["act"], d["weight"], 0.5, 2, d["logits"], 5, argmax=d["argmax"])
    with pytest.raises(ValueError, match="maps need"):
        ops.explain_topk(d["act"], d["weight"], 0.5, 2, d["logits"], 5, want_maps=True)


# ------------------------------------------------------------------------------------------------ 4. through the micro models
def _reference(z, coe):
    """From the fixture's eval outputs: pooled activations [B, P], their arg-max token and whether it is clear of the runner-up by more
    than 1e-3 relative, and the reserved cells [B, k]."""
    from protopformer_amd.interpret import reserved_indices
    d = z["eval/distances"].astype(np.float64)
    a = np.log((d + 1) / (d + 1e-4)).reshape(d.shape[0], d.shape[1], -1)
    top2 = np.sort(a, axis=-1)[..., ::-1][..., :2]
    clear = (top2[..., 0] - top2[..., 1]) > 1e-3 * np.abs(top2[..., 0])
    cells = reserved_indices(torch.from_numpy(z["eval/cls_token_attn"]), a.shape[-1]).numpy()
    return a.max(-1), a.argmax(-1), clear, cells


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_explain_on_the_fp32_path_against_the_fixture(fixture):
    from protopformer_amd.interpret import explain
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd)
    m.precise = True
    coe, P = cfg["global_coe"], cfg["num_prototypes"]
    x, labels = torch.from_numpy(z["img"]).cuda(), z["label"].astype(np.int64)
    h = explain(m, x, classes=labels.tolist(), topk=P).cpu()
    assert h.classes[:, 0].tolist() == labels.tolist() and (np.sort(h.prototypes[:, 0], axis=-1) == np.arange(P)).all()
    order = np.argsort(h.prototypes[:, 0], axis=-1)                                # the lists reordered by prototype id
    contrib = np.take_along_axis(h.contributions[:, 0], order, -1)
    cells = np.take_along_axis(h.cells[:, 0], order, -1)
    act_ref, argmax_ref, clear, cells_ref = _reference(z, coe)
    W = z["sd/last_layer.weight"].astype(np.float64)
    assert_elementwise(contrib, (1.0 - coe) * act_ref * W[labels], 1e-3, f"{fixture}: local contributions")
    rows = np.arange(len(labels))
    assert_elementwise(h.local["evidence"][:, 0].astype(np.float64).sum(-1), (1.0 - coe) * z["eval/logits_local"][rows, labels].astype(np.float64), 1e-3,
                       f"{fixture}: local evidence")
    assert_elementwise(h.global_["evidence"][:, 0].astype(np.float64).sum(-1), coe * z["eval/logits_global"][rows, labels].astype(np.float64), 1e-3,
                       f"{fixture}: global evidence")
    print(f"{fixture}: {int((~clear).sum())} of {clear.size} (sample, prototype) pairs are near-ties of the max-pool")
    assert (~clear).sum() <= 4
    want = np.take_along_axis(cells_ref, argmax_ref, -1)
    assert np.array_equal(cells[clear], want[clear]), f"{fixture}: cells differ from the reference's arg-max cells"
    assert h.maps.shape == (4, 1, P, 4, 4) and h.boxes.shape == (4, 1, P, 4) and (h.global_["cells"] == -1).all()


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_explain_on_the_default_path_equals_the_referee_on_its_own_tensors(fixture):
    from protopformer_amd.interpret import explain, explain_from_outputs, high_activation_boxes
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd)
    coe, K, M = cfg["global_coe"], 5, 3
    x = torch.from_numpy(z["img"]).cuda()
    m.train()
    ex = explain(m, x, top_classes=M, topk=K)
    assert m.training, "explain must leave the training flag as it found it"
    m.eval()
    with torch.no_grad():
        r = m._branches(x, want_dist=False)
    idx, act_full, logits, act_l, act_g, argmax = r.idx, r.act_full, r.logits, r.act_max_local, r.act_max_global, r.argmax
    h = ex.cpu()
    ref_l = explain_from_outputs(act_l, m.last_layer.weight, 1.0 - coe, m.num_prototypes_per_class, logits, K, top_classes=M, argmax=argmax, idx=idx,
                                 act_full=act_full, grid_cells=m.num_patches, maps=True, device=False)
    ref_g = explain_from_outputs(act_g, m.last_layer_global.weight, coe, m.global_proto_per_class, logits, K, classes=ref_l["classes"], device=False)
    for name, got, ref in (("local", h.local, ref_l), ("global", h.global_, ref_g)):
        for k in EXACT:
            if ref[k] is not None:
                assert np.array_equal(bits(got[k].reshape(ref[k].shape)), bits(ref[k])), f"{fixture} {name}: {k} differs from the referee"
    assert h.global_["maps"] is None and h.global_["boxes"] is None
    assert np.array_equal(h.classes[:, 0], logits.argmax(1).cpu().numpy())
    # local + global evidence is the logit: the summation bound of both branches plus 1e-6 for the product kernel's own rounding
    W_l, W_g = m.last_layer.weight.detach().cpu().numpy(), m.last_layer_global.weight.detach().cpu().numpy()
    a_l, a_g = act_l.cpu().numpy().astype(np.float64), act_g.cpu().numpy().astype(np.float64)
    for b in range(x.shape[0]):
        for j in range(M):
            c = int(h.classes[b, j])
            mass = (1.0 - coe) * np.abs(a_l[b] * W_l[c]).sum() + coe * np.abs(a_g[b] * W_g[c]).sum()
            total = h.local["evidence"][b, j].astype(np.float64).sum() + h.global_["evidence"][b, j].astype(np.float64).sum()
            bound = 1.01 * (W_l.shape[1] + W_g.shape[1]) * 2.0 ** -24 * mass + 1e-6
            assert abs(total - float(h.class_logits[b, j])) <= bound, (fixture, b, j, total, float(h.class_logits[b, j]), bound)
    assert np.array_equal(h.boxes, high_activation_boxes(ex.maps, m.img_size).cpu().numpy())
    # weights are the raw last-layer entries of the listed pairs
    assert np.array_equal(h.weights, W_l[h.classes[:, :, None], h.prototypes])
    off = explain(m, x, top_classes=M, topk=K, maps=False)
    assert off.maps is None and off.boxes is None and not m.training
    assert torch.equal(off.prototypes, ex.prototypes) and torch.equal(off.global_["contributions"], ex.global_["contributions"])
    against = explain(m, x, classes=ex.classes, topk=K, against=True, maps=False).cpu()
    assert (np.diff(against.contributions, axis=-1) >= 0).all() and (np.diff(h.contributions, axis=-1) <= 0).all()
    with pytest.raises(ValueError, match="classes must lie in"):
        explain(m, x, classes=[0, 1, 2, cfg["num_classes"]])


# ------------------------------------------------------------------------------------------------ 5. the tool
def test_tool_on_a_four_image_loader(tmp_path):
    from protopformer_amd import explain as tool
    from protopformer_amd.bank import write_bank
    from protopformer_amd.interpret import explain, nearest_patches
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    x, y, ids = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda(), torch.tensor([31, 7, 19, 4])
    bank = nearest_patches(m, [(x, y, ids)], topk=2, class_specific=False)
    npz, _ = write_bank(str(tmp_path / "bank"), bank.result(), {}, bank.ppc, bank.side, m.img_size // bank.side)
    out = str(tmp_path / "out")
    args = tool.get_args_parser().parse_args(["--output_dir", out, "--topk", "3", "--top_classes", "2", "--bank", npz, "--render"])
    path = tool.main(args, model=m, loader=[(x, y, ids)])
    lines = [json.loads(l) for l in open(path)]
    ex = explain(m, x, top_classes=2, topk=3)
    assert path == os.path.join(out, "explanations.jsonl") and len(lines) == 4
    assert [r["image_id"] for r in lines] == ids.tolist() and [r["label"] for r in lines] == z["label"].tolist()
    assert [r["classes"][0]["local"]["prototypes"][0]["prototype"] for r in lines] == ex.prototypes[:, 0, 0].tolist()
    assert [r["classes"][0]["class"] for r in lines] == ex.classes[:, 0].tolist()
    for r in lines:
        assert len(r["classes"]) == 2
        for c in r["classes"]:
            for br in ("local", "global"):
                assert len(c[br]["prototypes"]) == 3 and all(len(e["nearest"]) == 2 for e in c[br]["prototypes"])
            e = c["local"]["prototypes"][0]
            assert e["patch_box"] == [e["cell"] % 4 * 16, e["cell"] // 4 * 16, e["cell"] % 4 * 16 + 16, e["cell"] // 4 * 16 + 16]
            assert len(e["activation_box"]) == 4 and {n["image_id"] for n in e["nearest"]} <= set(ids.tolist())
            for rank in range(3):
                assert os.path.isfile(os.path.join(out, f"img_{r['image_id']}", f"class{c['class']}_rank{rank}.jpg"))
    from PIL import Image
    assert Image.open(os.path.join(out, "img_31", f"class{lines[0]['classes'][0]['class']}_rank0.jpg")).size == (64, 64)
