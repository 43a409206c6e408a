"""Row (a)16 and (f)1/(f)2 on the GPU: the fused AdamW + EMA against the reference fixture's `step/*` tensors and torch.optim.AdamW,
gradient clipping, checkpoint save / resume in the reference's dict layout, DropPath draws, the captured-graph step, and the
host-side guards (flat store rebuilt under an optimizer, compatibility wrapper shapes)."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import assert_close, build_micro, check_param_tensors, micro, rel_err
from oracle import ppf_oracle as O

pytestmark = pytest.mark.gpu


def _load_ref_grads(m, z):
    """Write the REFERENCE gradients of the micro fixture into the flat gradient buffer (full tensors; sampled ones stay zero and
    are skipped by the comparison)."""
    st = m.flat_store()
    st.zero_grad()
    full = []
    for name, p, o, n in st.entries:
        if f"grad/{name}" in z.files:
            st.grads[o:o + n].copy_(torch.from_numpy(z[f"grad/{name}"]).reshape(-1))
            full.append(name)
    return full


@pytest.mark.parametrize("name", ["micro_deit.npz", "micro_cait.npz"])
def test_fused_adamw_step_matches_reference_fixture(name):
    """Feed the reference's own gradients to FlatAdamW (reference param groups, create_optimizer.py:31-39) and compare every fully
    stored parameter after ONE step with the fixture's `step/*` (torch.optim.AdamW on the reference model); check the EMA copy."""
    from protopformer_amd.engine import FlatAdamW
    sd, cfg, z = micro(name)
    m = build_micro(cfg, sd).train()
    opt = FlatAdamW(m, weight_decay=0.05, ema_decay=0.99996)
    p0 = m.flat_store().params.clone()
    full = _load_ref_grads(m, z)
    assert len(full) > 20
    opt.step()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    for nm in full:
        assert_close(named[nm], z[f"step/{nm}"], rtol=1e-6, atol=1e-7, what=f"step/{nm}")
    # EMA (timm ModelEma, main.py:358-362): ema = d * ema + (1 - d) * p_new, ema_0 = p_0
    st = m.flat_store()
    expect = 0.99996 * p0.double() + (1 - 0.99996) * st.params.double()
    assert_close(opt.ema, expect, rtol=1e-6, atol=1e-8, what="EMA after one step")
    ema_sd = opt.ema_state_dict()
    assert set(ema_sd) == set(m.state_dict()) and torch.equal(ema_sd["last_layer.weight"], m.last_layer.weight)
    # the bf16 shadow was re-emitted by the same kernel
    assert torch.equal(st.bf16.float(), st.params.bfloat16().float())


def test_hip_train_step_vs_reference_step_fixture():
    """The whole HIP step (bf16 backbone) vs the fixture's post-step parameters: AdamW's first step is lr*g/(|g|+eps), so only
    entries whose reference gradient is clearly non-zero are comparable (a bf16-level error cannot flip their sign)."""
    from protopformer_amd.engine import FlatAdamW, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    opt = FlatAdamW(m, weight_decay=0.05)
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    loss, cov, mean = train_one_step(m, CrossEntropyLoss(), img, label, opt, epoch=20)
    assert rel_err(loss, z["train/loss"]) < 1e-4          # measured 1.9e-6 (bf16 backbone, fp32 losses)
    named = {k: v for k, v in m.named_parameters() if v.requires_grad}
    ok = tot = tensors = 0
    for nm, p in named.items():
        if f"step/{nm}" not in z.files:
            continue
        gref = torch.from_numpy(z[f"grad/{nm}"])
        strong = gref.abs() > 0.2 * gref.abs().max()
        if int(strong.sum()) == 0:
            continue
        ref = torch.from_numpy(z[f"step/{nm}"])[strong].double()
        got = p.detach().cpu()[strong].double()
        ok += int(((got - ref).abs() <= 2e-5 + 1e-4 * ref.abs()).sum()); tot += int(strong.sum()); tensors += 1
    # arg-max routing flips of the max-pool (documented in test_gpu_e2e.py) may move a few prototype-gradient entries
    assert tensors > 20 and ok >= 0.98 * tot, (ok, tot, tensors)


def test_adamw_state_dict_interops_with_torch_adamw_and_checkpoint_round_trip(tmp_path):
    """optimizer.state_dict() is torch.optim.AdamW's format (a reference --resume file loads, main.py:400-405); save_checkpoint /
    load_checkpoint write and read the reference's dict layout; a resumed run continues bit-identically."""
    from protopformer_amd.engine import (CosineLRScheduler, FlatAdamW, load_checkpoint, save_checkpoint, train_one_step)
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    crit = CrossEntropyLoss()
    a = build_micro(cfg, sd).train()
    opt_a = FlatAdamW(a, weight_decay=0.05, ema_decay=0.999)
    sch_a = CosineLRScheduler(opt_a, t_initial=200, lr_min=1e-5, warmup_lr_init=1e-4, warmup_t=5)
    for ep in range(2):
        train_one_step(a, crit, img, label, opt_a, epoch=20)
        sch_a.step(ep)
    # ---- torch.optim.AdamW reads our optimizer state and takes the same next step
    osd = opt_a.state_dict()
    ref_params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in a.named_parameters() if v.requires_grad}
    topt = torch.optim.AdamW(O.adamw_groups(ref_params), weight_decay=0.05, eps=1e-8)
    topt.load_state_dict({"state": {k: {kk: (vv.cpu() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} for k, v in osd["state"].items()},
                          "param_groups": [{k: v for k, v in g.items()} for g in osd["param_groups"]]})
    assert [g["lr"] for g in topt.param_groups] == [g["lr"] for g in opt_a.param_groups]
    path = str(tmp_path / "checkpoints" / "checkpoint-1.pth")
    save_checkpoint(path, a, opt_a, sch_a, epoch=1, args={"base_architecture": "micro"})
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) >= {"model", "optimizer", "lr_scheduler", "epoch", "model_ema"} and ck["epoch"] == 1
    assert set(ck["model"]) == set(sd) and set(ck["model_ema"]) == set(sd)
    assert set(ck["optimizer"]) == {"state", "param_groups"} and len(ck["optimizer"]["param_groups"]) == 4
    # ---- "new process": fresh model / optimizer / scheduler objects with different initial values
    sd_b = {k: (v + 0.01 if v.dtype.is_floating_point and k not in O.FROZEN_KEYS else v) for k, v in sd.items()}
    b = build_micro(cfg, sd_b).train()
    opt_b = FlatAdamW(b, weight_decay=0.05, ema_decay=0.999)
    sch_b = CosineLRScheduler(opt_b, t_initial=7, warmup_t=1)
    start = load_checkpoint(path, b, opt_b, sch_b)
    assert start == 2 and opt_b.step_count == opt_a.step_count == 2
    assert torch.equal(b.flat_store().params, a.flat_store().params) and torch.equal(opt_b.exp_avg, opt_a.exp_avg)
    assert torch.equal(opt_b.exp_avg_sq, opt_a.exp_avg_sq) and torch.equal(opt_b.ema, opt_a.ema)
    assert [g["lr"] for g in opt_b.param_groups] == [g["lr"] for g in opt_a.param_groups]
    la = train_one_step(a, crit, img, label, opt_a, epoch=20)[0]
    lb = train_one_step(b, crit, img, label, opt_b, epoch=20)[0]
    assert float(la) == float(lb), "resumed run must reproduce the next step's loss bit for bit"
    assert torch.equal(b.flat_store().params, a.flat_store().params)
    sch_a.step(2); sch_b.step(2)
    assert [g["lr"] for g in opt_b.param_groups] == [g["lr"] for g in opt_a.param_groups]
    # strict=False load of a backbone-only dict, as main_visualize.py:289
    part = {k: v for k, v in ck["model"].items() if k.startswith("features.")}
    torch.save({"model": part}, str(tmp_path / "part.pth"))
    assert load_checkpoint(str(tmp_path / "part.pth"), b, strict=False) == 0


def test_torch_adamw_next_step_equals_fused_kernel():
    from protopformer_amd.engine import FlatAdamW
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    opt = FlatAdamW(m, weight_decay=0.05)
    ref_params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters() if v.requires_grad}
    topt = torch.optim.AdamW(O.adamw_groups(ref_params), weight_decay=0.05, eps=1e-8)
    g = torch.Generator().manual_seed(0)
    st = m.flat_store()
    for it in range(3):
        st.zero_grad()
        for name, p, o, n in st.entries:
            gr = 0.01 * torch.randn(p.shape, generator=g)
            st.grads[o:o + n].copy_(gr.reshape(-1))
            ref_params[name].grad = gr
        opt.step(); topt.step()
        if it == 1:                                     # hand the state over mid-run: torch -> fused kernel
            opt.load_state_dict(topt.state_dict())
            assert opt.step_count == 2
    for name, p in m.named_parameters():
        if p.requires_grad:
            assert_close(p, ref_params[name].detach(), rtol=2e-6, atol=2e-7, what=name)


def test_clip_grad_norm_matches_torch():
    from protopformer_amd.engine import FlatAdamW
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    opt = FlatAdamW(m, weight_decay=0.05)
    st = m.flat_store()
    g = torch.Generator().manual_seed(4)
    grads = torch.randn(st.total, generator=g)
    mask = torch.zeros(st.total)                        # alignment padding between segments carries no gradient
    for name, p, o, n in st.entries:
        mask[o:o + n] = 1
    grads *= mask
    st.grads.copy_(grads)
    p0 = st.params.clone()
    opt.clip_grad_norm(0.5)
    opt.step()
    torch.cuda.synchronize()
    norm = float(grads.double().norm())
    assert float(opt.grad_norm) == pytest.approx(norm, rel=1e-5)
    coef = min(1.0, 0.5 / (norm + 1e-6))
    pr = p0.cpu().clone().requires_grad_(True)
    # one AdamW step of a single group is scale-free in g except through eps: compare against the clipped gradient explicitly
    ref = torch.optim.AdamW([{"params": [pr], "lr": 1e-4, "weight_decay": 1e-3}], eps=1e-8)
    pr.grad = grads * coef
    ref.step()
    lo, hi = opt.param_groups[0]["begin"], opt.param_groups[0]["end"]
    assert_close(st.params[lo:hi], pr.detach()[lo:hi], rtol=1e-6, atol=1e-8, what="clipped step (features group)")
    assert float(opt._hyper[19]) == pytest.approx(coef, rel=1e-5)
    # a later step WITHOUT clipping must not inherit the coefficient (it is reset with the step's other scalars)
    st.grads.copy_(grads)
    p1 = st.params.clone()
    opt.step()
    torch.cuda.synchronize()
    assert float(opt._hyper[19]) == 1.0
    pr2 = p1.cpu().clone().requires_grad_(True)
    ref2 = torch.optim.AdamW([{"params": [pr2], "lr": 1e-4, "weight_decay": 1e-3}], eps=1e-8)
    ref2.load_state_dict(ref.state_dict())
    pr2.grad = grads.clone()
    ref2.step()
    assert_close(st.params[lo:hi], pr2.detach()[lo:hi], rtol=1e-6, atol=1e-8, what="unclipped step after a clipped one")


def test_topk_sorted_direct():
    """ppf_topk_sorted (get_PPC_loss on a cache miss, protopformer.py:273-274): ascending indices of the k largest, bit-exact."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(8)
    for B, n, k in ((7, 196, 81), (3, 196, 121), (5, 16, 9), (2, 256, 256), (4, 197, 1)):
        s = torch.rand(B, n, generator=g)
        got = ops.topk_sorted(s.cuda(), k).cpu().long()
        ref = s.topk(k, dim=-1)[1].sort(dim=-1)[0]
        assert torch.equal(got, ref), (B, n, k)
    # PPNet.get_PPC_loss with a rollout tensor that is NOT the cached one takes this path and must give the same loss
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    logits, aux = m(img)
    c1 = m.get_PPC_loss(aux[2], aux[3], aux[4], label)
    c2 = m.get_PPC_loss(aux[2], aux[3].clone(), aux[4], label)
    assert float(c1[0]) == float(c2[0]) and float(c1[1]) == float(c2[1])


def test_droppath_draws_distribution_and_stream():
    """timm DropPath: per-sample factor floor(keep + U)/keep in {0, 1/keep}, P(keep) = keep; fresh draws every call; the
    sequence is a function of (seed, step counter) only."""
    from protopformer_amd import backbone
    rates = [0.0, 0.0] + [r for i in range(1, 12) for r in (0.1 * i / 11,) * 2]
    B = 4096
    backbone._KEEP_CACHE.clear()
    torch.manual_seed(1234)
    s1, index = backbone.droppath_scales(rates, B, torch.device("cuda"), True)
    s2, _ = backbone.droppath_scales(rates, B, torch.device("cuda"), True)
    assert index[0] == -1 and index[1] == -1 and s1.shape == (22, B)
    assert not torch.equal(s1, s2), "consecutive steps must draw fresh masks"
    s = s1.cpu()
    for slot in range(2, 24):
        keep = 1.0 - rates[slot]
        row = s[index[slot]]
        vals = torch.unique(row)
        assert all(abs(float(v)) < 1e-12 or abs(float(v) - 1.0 / keep) < 1e-6 for v in vals), (slot, vals)
        frac = float((row > 0).float().mean())
        sigma = math.sqrt(keep * (1 - keep) / B)
        assert abs(frac - keep) < 5 * sigma + 1e-9, (slot, frac, keep)
        assert abs(float(row.mean()) - 1.0) < 5 * sigma / keep + 1e-9              # E[factor] = 1
    # rows of different slots are independent draws
    assert not torch.equal(s[0] > 0, s[1] > 0)
    # same seed, restarted counter -> same sequence
    backbone._KEEP_CACHE.clear()
    torch.manual_seed(1234)
    r1, _ = backbone.droppath_scales(rates, B, torch.device("cuda"), True)
    assert torch.equal(r1, s1)
    assert backbone.droppath_scales(rates, B, torch.device("cuda"), False)[0] is None     # eval: identity
    backbone._KEEP_CACHE.clear()


def test_optimizer_survives_noop_move_and_rejects_rebuilt_store():
    """model.cuda() on a CUDA model must keep the flat store; a real re-materialisation must make the optimizer fail loudly."""
    from protopformer_amd.engine import FlatAdamW, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    opt = FlatAdamW(m, weight_decay=0.05)
    store = m.flat_store()
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    m = m.cuda().float().to("cuda")
    assert m.flat_store() is store
    p_before = store.params.clone()
    train_one_step(m, CrossEntropyLoss(), img, label, opt, epoch=20)
    assert not torch.equal(store.params, p_before), "the step must update the store the model computes with"
    m.double()                                          # re-materialises every parameter
    with pytest.raises(RuntimeError, match="flat parameter store was rebuilt|kernel operands|expected"):
        opt.step()


def test_compat_wrapper_returns_all_tokens():
    """forward_feature_mask_train_direct must return [B, 1+Np, D] like the reference (deit:209-240)."""
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).eval()
    img = torch.from_numpy(z["img"]).cuda()
    cls_e, x_e = m.features.forward_feature_patch_embed_all(img)
    x, (cls_attn, _) = m.features.forward_feature_mask_train_direct(cls_e, x_e, None, m.reserve_layer_nums)
    Np = (cfg["img"] // 16) ** 2
    assert x.shape == (img.shape[0], 1 + Np, cfg["dim"]) and cls_attn.shape == (img.shape[0], Np)
    # the reference's conv_features gather (protopformer.py:156-162) on it reproduces the model's own reserved tokens
    idx = cls_attn.topk(cfg["reserve_k"], dim=-1)[1].sort(dim=-1)[0]
    img_tok = torch.gather(x[:, 1:], 1, idx[:, :, None].expand(-1, -1, x.shape[-1]))
    assert torch.isfinite(img_tok).all()


def test_graphed_step_equals_eager_step():
    """engine.GraphedTrainStep: the captured + replayed step gives bit-identical losses and parameters to the eager step, follows
    lr changes made between replays, and advances the AdamW step count."""
    from protopformer_amd.engine import FlatAdamW, GraphedTrainStep, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    crit = CrossEntropyLoss()
    a = build_micro(cfg, sd).train(); opt_a = FlatAdamW(a, weight_decay=0.05, ema_decay=0.999)
    b = build_micro(cfg, sd).train(); opt_b = FlatAdamW(b, weight_decay=0.05, ema_decay=0.999)
    gs = GraphedTrainStep(b, crit, opt_b, epoch=20, warmup=2, max_norm=1.0)
    la, lb = [], []
    for it in range(7):
        if it == 5:                                     # a scheduler changes the learning rates between replays
            for g in opt_a.param_groups + opt_b.param_groups:
                g["lr"] = g["lr"] * 0.5
        la.append(float(train_one_step(a, crit, img, label, opt_a, epoch=20, max_norm=1.0)[0]))
        lb.append(float(gs(img, label)[0]))
    assert gs.graph is not None and opt_b.step_count == opt_a.step_count == 7
    assert la == lb, (la, lb)
    assert torch.equal(a.flat_store().params, b.flat_store().params) and torch.equal(opt_a.ema, opt_b.ema)
    assert la[-1] < la[0]
    # a new batch goes through the static input buffers
    img2 = img.flip(0).contiguous(); label2 = label.flip(0).contiguous()
    l2a = float(train_one_step(a, crit, img2, label2, opt_a, epoch=20, max_norm=1.0)[0])
    l2b = float(gs(img2, label2)[0])
    assert l2a == l2b


@pytest.mark.parametrize("arch", ["deit", "cait", "deit-bottleneck"])
def test_replayed_step_equals_eager_step(arch):
    """engine.ReplayedTrainStep (recorded command list) against the eager step: same losses and bit-identical parameters, moments and EMA
    after warm-up + recording + 3 replays with changing batches, clipping on, DropPath on (device-side counter), lr changed between steps
    (live optimizer scalars)."""
    from protopformer_amd import backbone
    from protopformer_amd.engine import FlatAdamW, ReplayedTrainStep, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss, construct_PPNet
    addon = "bottleneck" if arch.endswith("bottleneck") else "regular"      # (the reference's default head: 192 -> 96 -> 96 -> 64 -> 64 here)
    arch = arch.split("-")[0]
    name = "deit_tiny_patch16_224" if arch == "deit" else "cait_xxs24_224"
    layer, k = (11, 81) if arch == "deit" else (1, 121)

    def make():
        backbone._KEEP_CACHE.clear()
        torch.manual_seed(3)
        m = construct_PPNet(name, pretrained=False, img_size=224, prototype_shape=(200, 64, 1, 1), num_classes=20, reserve_layers=[layer],
                            reserve_token_nums=[k], use_global=True, use_ppc_loss=True, global_proto_per_class=5, add_on_layers_type=addon).cuda().train()
        if arch == "cait":                        # DropPath replay is covered bit for bit by the DeiT variant; CaiT's check below needs equal draws
            for blk in list(m.features.blocks) + list(m.features.blocks_token_only):
                blk.drop_path_rate = 0.0
        return m, FlatAdamW(m, weight_decay=0.05, ema_decay=0.999)

    g = torch.Generator(device="cuda").manual_seed(9)
    batches = [(torch.randn(6, 3, 224, 224, device="cuda", generator=g), torch.randint(0, 20, (6,), device="cuda", generator=g)) for _ in range(6)]
    crit = CrossEntropyLoss()
    a, opt_a = make()
    la = []
    for i, (x, y) in enumerate(batches):
        for grp in opt_a.param_groups:
            grp["lr"] = grp["initial_lr"] * (1.0 - 0.1 * i)
        la.append(float(train_one_step(a, crit, x, y, opt_a, epoch=20, max_norm=1.0)[0]))
    b, opt_b = make()
    rs = ReplayedTrainStep(b, crit, opt_b, epoch=20, max_norm=1.0, warmup=2)
    lb = []
    for i, (x, y) in enumerate(batches):
        for grp in opt_b.param_groups:
            grp["lr"] = grp["initial_lr"] * (1.0 - 0.1 * i)
        lb.append(float(rs(x, y)[0]))
    torch.cuda.synchronize()
    assert rs.rec is not None and len(rs.rec.cmds) > 100
    # bit-identical for both backbones: every reduction of the step has a fixed order (CaiT's proj_l / proj_w gradients were fp32 atomics
    # until the fused talking-heads kernels of round 3 replaced them by per-workgroup partial rows + an ordered sum)
    assert la == lb, (la, lb)
    assert torch.equal(a.flat_store().params, b.flat_store().params) and torch.equal(opt_a.exp_avg, opt_b.exp_avg) and torch.equal(opt_a.ema, opt_b.ema)
    # a batch of another size (the short last batch of an epoch) runs eagerly on the same state and leaves the recorded list usable
    xs, ys = batches[0][0][:4].contiguous(), batches[0][1][:4].contiguous()
    l_a = float(train_one_step(a, crit, xs, ys, opt_a, epoch=20, max_norm=1.0)[0]); l_b = float(rs(xs, ys)[0])
    x, y = batches[1]
    l_a2 = float(train_one_step(a, crit, x, y, opt_a, epoch=20, max_norm=1.0)[0]); l_b2 = float(rs(x, y)[0])
    torch.cuda.synchronize()
    assert math.isfinite(l_b) and math.isfinite(l_b2) and opt_a.step_count == opt_b.step_count == 8
    if arch == "cait":                            # DropPath off: the interleaved eager / replayed steps see the same (no) draws
        assert l_a == l_b and l_a2 == l_b2 and torch.equal(a.flat_store().params, b.flat_store().params)


@pytest.mark.parametrize("kind", ["replayed", "graphed"])
def test_frozen_step_recasts_the_shadow_after_load_state_dict(kind):
    """A recorded / captured step does not contain the fp32 -> bf16 weight cast (the shadow was fresh when it was frozen).  After
    model.load_state_dict() between two steps the next frozen step must run on the NEW weights, like the eager step does."""
    from protopformer_amd.engine import FlatAdamW, GraphedTrainStep, ReplayedTrainStep, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    crit = CrossEntropyLoss()
    sd2 = {k: (v * 1.25 if v.dtype.is_floating_point and "last_layer" not in k and k != "ones" else v) for k, v in sd.items()}
    a = build_micro(cfg, sd).train(); opt_a = FlatAdamW(a, weight_decay=0.05)
    b = build_micro(cfg, sd).train(); opt_b = FlatAdamW(b, weight_decay=0.05)
    step = (ReplayedTrainStep if kind == "replayed" else GraphedTrainStep)(b, crit, opt_b, epoch=20, warmup=1)
    for _ in range(3):                                   # warm-up, freeze, one replay
        la = float(train_one_step(a, crit, img, label, opt_a, epoch=20)[0]); lb = float(step(img, label)[0])
        assert la == lb
    a.load_state_dict(sd2); b.load_state_dict(sd2)
    assert not b.flat_store().bf16_fresh
    la = float(train_one_step(a, crit, img, label, opt_a, epoch=20)[0]); lb = float(step(img, label)[0])
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    assert torch.equal(a.flat_store().params, b.flat_store().params)


def test_nonfinite_loss_skips_the_update_and_raises_the_flag():
    """tools/engine_proto.py:66-70 (exit in front of optimizer.step() when the loss is NaN / inf), evaluated on the device every step: the
    optimizer kernel leaves parameters, moments, EMA and the bf16 shadow untouched and raises optimizer.nonfinite; train_one_epoch reads
    the flag at its logging cadence and stops."""
    from protopformer_amd.engine import FlatAdamW, train_one_epoch, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    crit = CrossEntropyLoss()
    m = build_micro(cfg, sd).train(); opt = FlatAdamW(m, weight_decay=0.05, ema_decay=0.999)
    train_one_step(m, crit, img, label, opt, epoch=20)
    assert int(opt.nonfinite) == 0
    st = m.flat_store()
    before = (st.params.clone(), st.bf16.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone())
    good = m.last_layer.weight.data.clone()
    m.last_layer.weight.data.fill_(float("nan"))              # frozen class-connection weights: logits, hence the loss, become NaN
    loss, _, _ = train_one_step(m, crit, img, label, opt, epoch=20)
    m.last_layer.weight.data.copy_(good)
    assert not math.isfinite(float(loss)) and int(opt.nonfinite) == 1
    after = (st.params, st.bf16, opt.exp_avg, opt.exp_avg_sq, opt.ema)
    assert all(torch.equal(a_, b_) for a_, b_ in zip(before, after))
    # the epoch loop stops at its next log read, even if that step's own loss is finite again
    logs = []
    with pytest.raises(SystemExit):
        train_one_epoch(m, crit, [(img, label)] * 3, opt, "cuda", epoch=20, log_every=2, logger=logs.append)
    assert any("stopping training" in s for s in logs)
    # the raised flag also stops an epoch that never reaches a log read, and no checkpoint is written from that state (round 5)
    from protopformer_amd.engine import save_checkpoint
    logs2 = []
    with pytest.raises(SystemExit):
        train_one_epoch(m, crit, [(img, label)], opt, "cuda", epoch=20, log_every=1000, logger=logs2.append)
    assert any("stopping training" in s for s in logs2)
    import tempfile, os
    with tempfile.TemporaryDirectory() as d:
        with pytest.raises(RuntimeError, match="non-finite"):
            save_checkpoint(os.path.join(d, "ck.pth"), m, opt, None, 0)
        assert not os.path.exists(os.path.join(d, "ck.pth"))


def test_block_row_ppc_gradient_equals_dense_exchange_also_when_shared():
    """get_PPC_loss hands the prototype layer its gradient as [B, ppc, T] block rows behind a zero-stride placeholder of the dense shape
    (protopformer.PPCLossFn / ProtoLayerFn): parameter gradients equal those of the dense exchange to rounding -- also in a graph in which
    autograd combines that gradient with another consumer's (the placeholder is zeros, the parked rows are folded into the dense sum)."""
    from protopformer_amd import protopformer as P
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    crit = CrossEntropyLoss()

    def grads(rows, shared=False):
        old, P._PROTO_ROWS = P._PROTO_ROWS, rows
        try:
            m = build_micro(cfg, sd).train()
            torch.manual_seed(0)
            logits, aux = m(img)
            cov, mean = m.get_PPC_loss(aux[2], aux[3], aux[4], label)
            loss = crit(logits, label) + 0.1 * cov + 0.1 * mean
            if shared:                                        # a second consumer of the activation map
                loss = loss + 1e-3 * (aux[2] * aux[2]).sum()
            loss.backward()
            torch.cuda.synchronize()
            assert not P._PENDING_ROWS
            return m, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        finally:
            P._PROTO_ROWS = old

    for shared in (False, True):
        _, g_rows = grads(True, shared)
        _, g_dense = grads(False, shared)
        assert g_rows.keys() == g_dense.keys() and "prototype_vectors" in g_rows
        for n in g_rows:
            assert_close(g_rows[n], g_dense[n], rtol=2e-3, atol=2e-5 * float(g_dense[n].abs().max()) + 1e-12,
                         what=f"grad {n}: block rows vs dense (shared={shared})")
