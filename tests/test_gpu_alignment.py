"""Spatial alignment on the GPU: ppf_grad_box_mass against numpy fp64 within the any-order summation bound, ppf_pgd_step_box against
the numpy referee bit for bit, interpret.prototype_boxes against the host's resize_cubic peak, gradient_locality on the device against
its referee, misalignment_attack against the referee's step and its own constraints, spatial_alignment against the per-pass results
combined on the host and across loader batch sizes, and the command-line tool on the miniature CUB tree.

Bounds.  The sums of ppf_grad_box_mass are sums of n = C*H*W non-negative fp64 terms, each exact: any summation order is within
(n - 1) * 2^-52 relative of the exact sum (derived, not measured).  ppf_pgd_step_box rounds every operation once in fp32, as numpy does:
no tolerance."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

R, C, H, W = 5, 3, 20, 28
BOXES = np.array([[4, 4, 3, 20],           # empty: y0 == y1
                  [0, H, 0, W],            # the full image
                  [7, 8, 11, 12],          # a single pixel
                  [13, H, 19, W],          # touches the bottom-right border
                  [3, 10, 5, 16]],         # interior, odd extents (7 x 11)
                 dtype=np.int32)


def _inside_mask(boxes, h, w):
    ys, xs = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    return (ys >= boxes[:, 0, None, None]) & (ys < boxes[:, 1, None, None]) & (xs >= boxes[:, 2, None, None]) & (xs < boxes[:, 3, None, None])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return bool((a.view(np.int32) == b.view(np.int32)).all())


# ------------------------------------------------------------------------------------------------ 1. ppf_grad_box_mass
@pytest.mark.parametrize("w", [W, W - 1], ids=["W28", "W27"])
def test_grad_box_mass_against_numpy_fp64(w):
    from protopformer_amd import ops
    rng = np.random.default_rng(3)
    g = (rng.standard_normal((R, C, H, w)) * np.exp(rng.uniform(-8, 8, (R, C, H, w)))).astype(np.float32)
    g[1, 2, 5, 6], g[4, 0, 4, 7], g[4, 1, 19, 0] = np.nan, np.inf, -np.inf          # one NaN (row 1), one inf inside and one outside the box (row 4)
    boxes = BOXES.copy()
    boxes[:, 3] = np.minimum(boxes[:, 3], w)
    gd, bd = torch.from_numpy(g).cuda(), torch.from_numpy(boxes).cuda()
    inside, total, bad = ops.grad_box_mass(gd, bd)
    torch.cuda.synchronize()
    assert inside.dtype == total.dtype == torch.float64 and bad.dtype == torch.int32 and inside.shape == total.shape == bad.shape == (R,)
    fin = np.isfinite(g)
    m = _inside_mask(boxes, H, w)[:, None] & fin
    n = C * H * w
    bound = (n - 1) * 2.0 ** -52
    for r in range(R):
        ti = math.fsum(np.abs(g[r][m[r]]).astype(np.float64).tolist())               # the exact sums, rounded once
        tt = math.fsum(np.abs(g[r][fin[r]]).astype(np.float64).tolist())
        assert abs(float(total[r]) - tt) <= bound * tt, f"row {r}: total off by {abs(float(total[r]) - tt) / tt / bound:.3f} bounds"
        assert abs(float(inside[r]) - ti) <= bound * ti, f"row {r}: inside off"
    assert float(inside[0]) == 0.0 and float(inside[1]) == float(total[1])              # the empty box; the full image
    assert bad.cpu().tolist() == [0, 1, 0, 0, 2]
    again = ops.grad_box_mass(gd, bd)
    assert all(torch.equal(a, b) for a, b in zip((inside, total, bad), again)), "a repeated launch differs"
    i2, t2, none = ops.grad_box_mass(gd, bd, want_nonfinite=False)                       # the counter is optional
    assert none is None and torch.equal(i2, inside) and torch.equal(t2, total)
    with pytest.raises(ValueError, match="box must be"):
        ops.grad_box_mass(gd, bd[:, :3].contiguous())
    with pytest.raises(ValueError, match="g must be"):
        ops.grad_box_mass(gd.double(), bd)


def test_gradient_locality_of_a_zero_gradient_is_nan():
    from protopformer_amd.interpret import gradient_locality
    g = torch.zeros(2, 3, 8, 8, device="cuda")
    g[1, 0, 2, 2] = -2.0
    inside, total, share = gradient_locality(g, torch.tensor([[0, 4, 0, 4], [0, 4, 0, 4]], dtype=torch.int32, device="cuda"))
    assert total.tolist() == [0.0, 2.0] and inside.tolist() == [0.0, 2.0] and math.isnan(float(share[0])) and float(share[1]) == 1.0


# ------------------------------------------------------------------------------------------------ 2. ppf_pgd_step_box
def _pgd_case(w, seed=5):
    from protopformer_amd.interpret import attack_bounds
    rng = np.random.default_rng(seed)
    a, e, lo, hi = attack_bounds(8 / 255, None, 10)
    x0 = rng.uniform(-1.75, 2.2, (R, C, H, w)).astype(np.float32)                       # valid pixels, some within eps of lo / hi: those clamps act
    off = rng.uniform(-1, 1, x0.shape).astype(np.float32) * e.reshape(1, C, 1, 1)
    at_edge = rng.random(x0.shape)
    x = np.where(at_edge < 0.2, x0 + e.reshape(1, C, 1, 1), np.where(at_edge < 0.4, x0 - e.reshape(1, C, 1, 1), x0 + off)).astype(np.float32)
    g = rng.standard_normal(x0.shape).astype(np.float32)
    kind = rng.random(x0.shape)
    g[kind < 0.1], g[(kind >= 0.1) & (kind < 0.2)], g[(kind >= 0.2) & (kind < 0.3)] = 0.0, -0.0, np.nan
    g[0, 0, 0, 0], g[0, 0, 0, 1] = np.inf, -np.inf
    boxes = BOXES.copy()
    boxes[:, 3] = np.minimum(boxes[:, 3], w)
    return x, x0, g, boxes, (a, e, lo, hi)


@pytest.mark.parametrize("direction", [1, -1], ids=["ascend", "descend"])
@pytest.mark.parametrize("w", [W, W - 1], ids=["W28_vector", "W27_scalar"])
def test_pgd_step_box_equals_numpy_bit_for_bit(w, direction):
    from protopformer_amd.interpret import pgd_step_box
    x, x0, g, boxes, consts = _pgd_case(w)
    want = pgd_step_box(x, x0, g, boxes, *consts, direction, device=False)
    dev = [torch.from_numpy(v).cuda() for v in (x, x0, g, boxes) + consts]
    got = pgd_step_box(*dev, direction)
    torch.cuda.synchronize()
    assert got.data_ptr() == dev[0].data_ptr(), "the step is in place"
    got = got.cpu().numpy()
    assert same_bits(got, want), f"{int((got.view(np.int32) != want.view(np.int32)).sum())} elements differ from the referee"
    m = np.broadcast_to(_inside_mask(boxes, H, w)[:, None], x.shape)
    assert same_bits(got[m], x0[m]) and m[1].all() and not m[0].any()                   # inside every box the original pixel, bit for bit
    a, e, lo, hi = (v.reshape(1, C, 1, 1) for v in consts)
    out = ~m
    assert ((got >= np.maximum(x0 - e, lo)) & (got <= np.minimum(x0 + e, hi)))[out].all()
    assert (got == np.minimum(x0 + e, hi))[out].any() and (got == np.maximum(x0 - e, lo))[out].any() and (got == hi)[out].any() and (got == lo)[out].any()
    still = out & ((g == 0) | np.isnan(g)) & (np.abs(x.astype(np.float64) - x0) < e * 0.99) & (x > lo) & (x < hi)
    assert still.any() and same_bits(got[still], x[still])                              # sign(+-0) = sign(NaN) = 0: no move
    from protopformer_amd import ops
    with pytest.raises(ValueError, match="direction"):
        ops.pgd_step_box(*dev, 0)
    with pytest.raises(ValueError, match="alpha must be"):
        ops.pgd_step_box(*dev[:4], dev[4][:2].contiguous(), *dev[5:], 1)


# ------------------------------------------------------------------------------------------------ 3. through the micro models
def _six_images(z):
    x = torch.from_numpy(z["img"])
    return torch.cat([x, x.flip(-1)])[:6].contiguous()


def _top_protos(m, outs, K):
    ppc = m.num_prototypes_per_class
    own = outs["logits"].argmax(1)[:, None] * ppc + torch.arange(ppc, device="cuda")[None, :]
    return own.gather(1, torch.sort(outs["act_max"].gather(1, own), dim=1, descending=True, stable=True)[1][:, :K]).to(torch.int32)


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_prototype_boxes_equal_the_host_peak(fixture):
    from protopformer_amd.interpret import _eval_outputs, expand_to_grid, prototype_boxes, resize_cubic
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda()
    with torch.no_grad():
        outs = _eval_outputs(m, x)
    B, K, k, S = x.shape[0], 2, cfg["reserve_k"], cfg["img"]
    protos = _top_protos(m, outs, K)
    for half in (36, 10):
        boxes = prototype_boxes(m, outs, protos, half_size=half)
        assert boxes.shape == (B * K, 4) and boxes.dtype == torch.int32 and boxes.is_cuda
        s = int(round(k ** 0.5))
        grid = expand_to_grid(outs["act_full"].reshape(B, -1, s, s).cpu(), outs["token_attn"].cpu(), k).numpy()
        want = []
        for b in range(B):
            for p in protos[b].tolist():
                up = resize_cubic(grid[b, p], S)
                ys, xs = np.where(up == up.max())
                y, xx = int(ys[0]), int(xs[0])
                want.append([max(0, y - half), min(S, y + half), max(0, xx - half), min(S, xx + half)])
        assert boxes.cpu().tolist() == want, f"{fixture} half_size={half}"
    one = prototype_boxes(m, outs, protos[:, 0], half_size=10)                          # [B] prototypes: one row per image
    assert torch.equal(one, prototype_boxes(m, outs, protos, half_size=10)[::K])


@pytest.mark.parametrize("precise", [False, True], ids=["bf16", "fp32"])
def test_gradient_locality_device_against_the_referee(precise):
    from protopformer_amd.interpret import _eval_outputs, gradient_locality, input_gradient, prototype_boxes
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).eval()
    m.precise = precise
    x = torch.from_numpy(z["img"]).cuda()
    with torch.no_grad():
        outs = _eval_outputs(m, x)
    protos = _top_protos(m, outs, 1)
    boxes = prototype_boxes(m, outs, protos, half_size=12)
    grad, val = input_gradient(m, x, ("proto", "local", protos.reshape(-1)))
    inside, total, share = gradient_locality(grad, boxes)
    ri, rt, rs = gradient_locality(grad, boxes, device=False)
    n = grad[0].numel()
    for got, ref in ((inside, ri), (total, rt)):
        assert got.dtype == torch.float64 and np.all(np.abs(got.cpu().numpy() - ref) <= (n - 1) * 2.0 ** -51 * ref)      # both sides any-order sums
    assert np.allclose(share.cpu().numpy(), rs, rtol=1e-12, atol=0) and (rt > 0).all() and ((rs >= 0) & (rs <= 1)).all()
    area = ((boxes[:, 1] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 2])).double().cpu().numpy() / (64 * 64)
    print(f"micro DeiT ({'fp32' if precise else 'bf16'}): gradient share inside the box {rs.round(4).tolist()} against its area {area.round(4).tolist()}")


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_misalignment_attack_steps_and_constraints(fixture):
    from protopformer_amd.interpret import _eval_outputs, attack_bounds, input_gradient, misalignment_attack, pgd_step_box, prototype_boxes
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd).eval()
    _, _, lo3, hi3 = attack_bounds(8 / 255, None, 1, "cuda")
    x = torch.from_numpy(z["img"]).cuda()                                               # the fixture's images are normal deviates:
    x = torch.minimum(torch.maximum(x, lo3.reshape(1, 3, 1, 1)), hi3.reshape(1, 3, 1, 1)).contiguous()      # ... as valid normalised pixels
    with torch.no_grad():
        outs = _eval_outputs(m, x)
    K = 2
    protos = _top_protos(m, outs, K)
    boxes = prototype_boxes(m, outs, protos, half_size=12)
    rows, x_rows = protos.reshape(-1), x.repeat_interleave(K, dim=0).contiguous()
    # one step = the referee's step on input_gradient's output
    r1 = misalignment_attack(m, x, protos, boxes, steps=1, return_images=True)
    g, v = input_gradient(m, x_rows, ("proto", "local", rows))
    consts = attack_bounds(8 / 255, None, 1)
    want = pgd_step_box(x_rows.cpu().numpy(), x_rows.cpu().numpy(), g.cpu().numpy(), boxes.cpu().numpy(), *consts, -1, device=False)
    assert same_bits(r1["images"].cpu().numpy(), want), f"{fixture}: one attack step differs from the referee's step"
    assert float((r1["act_before"] - v).abs().max()) <= 1e-3 * float(v.abs().max())        # an eval forward against one that saves for backward
    assert r1["images"].shape == x_rows.shape and torch.equal(r1["protos"], rows)
    # three steps: inside the eps-ball and the pixel range, the box untouched
    r3 = misalignment_attack(m, x, protos, boxes, steps=3, return_images=True)
    a, e, lo, hi = (c.reshape(1, 3, 1, 1) for c in attack_bounds(8 / 255, None, 3))
    got, x0 = r3["images"].cpu().numpy(), x_rows.cpu().numpy()
    inside = np.broadcast_to(_inside_mask(boxes.cpu().numpy(), 64, 64)[:, None], got.shape)
    assert same_bits(got[inside], x0[inside]) and inside.any() and not inside.all()
    assert ((got >= np.maximum(x0 - e, lo)) & (got <= np.minimum(x0 + e, hi))).all() and (got != x0).any()
    assert (np.abs(got.astype(np.float64) - x0) <= e + 2.0 ** -23).all()
    for key, dt in (("act_before", torch.float32), ("act_after", torch.float32), ("pac", torch.float64), ("plc", torch.int32), ("left_box", torch.bool)):
        assert r3[key].shape == (x.shape[0] * K,) and r3[key].dtype == dt and r3[key].is_cuda, key
    pac = ((r3["act_before"].double() - r3["act_after"].double()) / r3["act_before"].double().abs())
    assert torch.equal(r3["pac"], pac) and torch.equal(r3["plc"], (r3["peak_after"] - r3["peak_before"]).abs().max(1)[0].to(torch.int32))
    with torch.no_grad():
        after = _eval_outputs(m, r3["images"])["act_max"].gather(1, rows.long()[:, None]).reshape(-1)
    assert torch.equal(after, r3["act_after"]) and "images" not in misalignment_attack(m, x, protos, boxes, steps=1)
    print(f"{fixture}: activation before {r3['act_before'].tolist()} after three steps {r3['act_after'].tolist()} PLC {r3['plc'].tolist()}")
    assert all(p.grad is None for p in m.parameters()) and not m.training
    # a seeded start stays inside the same constraints
    rs = misalignment_attack(m, x, protos, boxes, steps=1, seed=3, return_images=True)["images"].cpu().numpy()
    e1 = attack_bounds(8 / 255, None, 1)[1].reshape(1, 3, 1, 1)
    assert same_bits(rs[inside], x0[inside]) and ((rs >= np.maximum(x0 - e1, lo)) & (rs <= np.minimum(x0 + e1, hi))).all() and not same_bits(rs, r1["images"].cpu().numpy())


def _loader(x6, bs):
    return [(x6[i:i + bs], torch.zeros(min(bs, 6 - i), dtype=torch.int64)) for i in range(0, 6, bs)]


def test_spatial_alignment_over_a_loader():
    """Equals the per-pass rows combined on the host; the same for loader batch sizes 2 and 3.  The rows of a pass depend on what shares
    the pass with them only through the kernels' batch-dependent tiling, so the ORDER HAD TO BE FIXED: the images are regrouped into
    passes of pass_images images whatever the loader's batch size (interpret._regroup), the rows are kept in pair order and summed
    once at the end."""
    from protopformer_amd.interpret import ALIGNMENT_STATS, alignment_rows, spatial_alignment
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).eval()
    x6 = _six_images(z)
    kw = dict(protos_per_image=2, half_size=12, attack_steps=2)
    res = spatial_alignment(m, _loader(x6, 2), pass_images=2, **kw)
    assert res["images"] == 6 and res["rows"] == 12 and set(res["overall"]) == {"mean_" + k for k in ALIGNMENT_STATS} | {"share_over_area"}
    ids, stats = zip(*[alignment_rows(m, x6[i:i + 2].cuda(), 2, 12, True, 2) for i in range(0, 6, 2)])
    ids, stats = torch.cat(ids).cpu().numpy(), torch.cat(stats).cpu().numpy()
    assert stats.shape == (12, 5) and stats.dtype == np.float64 and not np.isnan(stats).any()
    for j, k in enumerate(ALIGNMENT_STATS):
        want = math.fsum(stats[:, j].tolist()) / 12
        assert abs(res["overall"]["mean_" + k] - want) <= 12 * 2.0 ** -52 * np.abs(stats[:, j]).sum() / 12, k
    assert abs(res["overall"]["share_over_area"] - res["overall"]["mean_share"] / res["overall"]["mean_area"]) <= 1e-15
    assert sorted(res["per_prototype"]) == sorted(set(ids.tolist())) and sum(v["rows"] for v in res["per_prototype"].values()) == 12
    for p, v in res["per_prototype"].items():
        sel = ids == p
        for j, k in enumerate(ALIGNMENT_STATS):
            want = math.fsum(stats[sel, j].tolist()) / int(sel.sum())
            assert abs(v["mean_" + k] - want) <= 12 * 2.0 ** -52 * np.abs(stats[sel, j]).sum() and v["rows"] == int(sel.sum()), (p, k)
    assert 0 < res["overall"]["mean_area"] <= 1 and 0 <= res["overall"]["mean_share"] <= 1 and 0 <= res["overall"]["mean_left_box"] <= 1
    # any loader batch size gives the same passes, so the same result, bit for bit; a pass may straddle two loader batches
    for pass_images in (4, 16):
        a, b = (spatial_alignment(m, _loader(x6, bs), pass_images=pass_images, **kw) for bs in (2, 3))
        assert a == b, f"pass_images={pass_images}: loader batch sizes 2 and 3 disagree"
    no_attack = spatial_alignment(m, _loader(x6, 3), attack=False, max_images=5, **kw)
    assert no_attack["images"] == 5 and no_attack["rows"] == 10 and math.isnan(no_attack["overall"]["mean_pac"]) and no_attack["overall"]["mean_share"] >= 0
    with pytest.raises(ValueError, match="no image"):
        spatial_alignment(m, [], **kw)


# ------------------------------------------------------------------------------------------------ 4. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def test_tool_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd import alignment as tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    tree, out = str(tmp_path / "data"), str(tmp_path / "out")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", out, "--resume", ck, "--attack_steps", "2",
                                              "--max_images", "6", "--protos_per_image", "2", *MODEL_FLAGS])
    path = tool.main(args)
    doc = json.load(open(path))
    assert path == os.path.join(out, "alignment.json") and doc["images"] == 6 and doc["rows"] == 12
    assert doc["settings"] == dict(protos_per_image=2, half_size=36, attack=True, attack_steps=2, eps_255=8.0, precise=False, split="test")
    keys = {"mean_share", "mean_area", "share_over_area", "mean_pac", "mean_plc", "mean_left_box"}
    assert set(doc["overall"]) == keys and all(isinstance(v, float) for v in doc["overall"].values())
    assert 0 <= doc["overall"]["mean_share"] <= 1 and 0 < doc["overall"]["mean_area"] <= (72 * 72) / (224 * 224) + 1e-12 and 0 <= doc["overall"]["mean_left_box"] <= 1
    assert 1 <= len(doc["per_prototype"]) <= 12 and sum(v["rows"] for v in doc["per_prototype"].values()) == 12
    assert all(set(v) == keys | {"rows"} and 0 <= int(p) < 400 for p, v in doc["per_prototype"].items())
