"""Integrated gradients on the GPU: ppf_ig_point, ppf_ig_accumulate and ppf_ig_finish against the numpy referees of interpret.py
(ig_point / ig_accumulate / ig_finish with device=False), interpret.integrated_gradients and the 'ig' order of faithfulness_curves
through the micro models against the referee pipeline, and the two command-line tools on the miniature CUB tree.

The three kernels are plain fp32 with one rounding per operation (the contract in include/ppf_hip.h), so path points, accumulators and
attributions are compared bit for bit.  The fp64 cell sums have a fixed but unspecified order and are held to the any-order bound
C * patch^2 * 2^-53 * sum |attr| against np.sum, the bound ppf_grad_box_mass is held to.  The completeness gap of the models is printed,
not gated: the token reservation's top-k makes them discontinuous along the path."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro, report

pytestmark = pytest.mark.gpu

POISON = float.fromhex("0x1.5p+100")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def cells_within_bound(cell64, attr, patch, what):
    """cell64 [B, M, G] against the fp64 np.sum of the host attribution attr [B, M, C, H, W] per cell, within C * patch^2 * 2^-53 * sum |attr|."""
    B, M, C, H, W = attr.shape
    a = attr.reshape(B, M, C, H // patch, patch, W // patch, patch).astype(np.float64)
    ref, mass = a.sum(axis=(2, 4, 6)).reshape(B, M, -1), np.abs(a).sum(axis=(2, 4, 6)).reshape(B, M, -1)
    err = np.abs(np.asarray(cell64, dtype=np.float64) - ref)
    bound = C * patch * patch * 2.0 ** -53 * mass
    assert (err <= bound).all(), f"{what}: cell sums off np.sum by {(err / np.maximum(bound, 1e-300)).max():.2f} bounds"
    return float((err / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------------------------------------ 1. ppf_ig_point
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 2 * 3 * 64 * 64])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_point_equals_the_referee_bit_for_bit(n, tensor_baseline):
    from protopformer_amd.interpret import ig_point
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    base = rng.standard_normal(n).astype(np.float32) if tensor_baseline else -0.375
    xd, bd = dev(x), dev(base) if tensor_baseline else base
    for alpha in (0.0, 1.0, 1 / 3, 0.999):
        got = ig_point(xd, alpha, bd).cpu().numpy()
        assert np.array_equal(bits(got), bits(ig_point(x, alpha, base, device=False))), f"n={n} alpha={alpha}"
    assert np.array_equal(ig_point(xd, 0.0, bd).cpu().numpy(), np.broadcast_to(np.float32(base), x.shape))       # alpha 0: the baseline
    assert torch.equal(ig_point(xd, 1.0, 0.0), xd)                                                               # alpha 1 from 0: x


def test_point_on_an_unaligned_view_and_into_an_out_buffer():
    from protopformer_amd import ops
    from protopformer_amd.interpret import ig_point
    rng = np.random.default_rng(7)
    n = 1028                                                                                      # a multiple of 4: only the address forces the scalar path
    store, base_store = dev(rng.standard_normal(n + 1).astype(np.float32)), dev(rng.standard_normal(n + 1).astype(np.float32))
    x, base = store[1:], base_store[1:]                                                           # one element into their buffers: 4-byte aligned only
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    ref = ig_point(x.cpu().numpy(), 1 / 3, base.cpu().numpy(), device=False)
    assert np.array_equal(bits(ig_point(x, 1 / 3, base).cpu().numpy()), bits(ref))
    assert np.array_equal(bits(ig_point(x, 1 / 3, base.clone()).cpu().numpy()), bits(ref))        # x alone unaligned
    buf = torch.full((n + 9,), POISON, device="cuda")
    out = ops.ig_point(x, 1 / 3, base, out=buf[1:n + 1])                                          # the out buffer unaligned too
    assert out.data_ptr() == buf.data_ptr() + 4 and np.array_equal(bits(out.cpu().numpy()), bits(ref))
    assert float(buf[0]) == POISON and bool((buf[n + 1:] == POISON).all())                        # nothing around it is written
    img = dev(rng.standard_normal((2, 3, 8, 8)).astype(np.float32))
    assert ops.ig_point(img, 0.5, 0.25).shape == img.shape
    with pytest.raises(ValueError, match="x must be torch.float32"):
        ops.ig_point(img.double(), 0.5)
    with pytest.raises(ValueError, match="x must be contiguous"):
        ops.ig_point(img[:, :, ::2], 0.5)
    with pytest.raises(ValueError, match="baseline must be"):
        ops.ig_point(img, 0.5, img[:1])
    with pytest.raises(ValueError, match="out must be"):
        ops.ig_point(img, 0.5, out=buf[:5])


# ------------------------------------------------------------------------------------------------ 2. ppf_ig_accumulate
def test_accumulate_five_steps_into_a_strided_poisoned_buffer():
    from protopformer_amd.interpret import ig_accumulate, ig_rule
    rng = np.random.default_rng(11)
    R, n = 3, 1027
    _, weights = ig_rule(4, "trapezoid")                                                          # five steps, two weights
    store = torch.full((R, 2 * n), POISON, device="cuda")
    acc = store[:, :n]                                                                            # acc_stride = 2 n: odd rows start unaligned
    assert acc.stride(0) == 2 * n and not acc.is_contiguous()
    ref = None
    for s, w in enumerate(weights.tolist()):
        g = rng.standard_normal((R, n)).astype(np.float32)
        ref = ig_accumulate(g, w, ref, first=s == 0, device=False)
        out = ig_accumulate(dev(g), w, acc, first=s == 0)
        assert out.data_ptr() == store.data_ptr()
        assert np.array_equal(bits(acc.cpu().numpy()), bits(ref)), f"step {s}"
    assert bool((store[:, n:] == POISON).all()), "the gaps between the rows keep their poison"


@pytest.mark.parametrize("R,n,stride", [(3, 1028, 2 * 1028), (2, 3 * 64 * 64, 2 * 3 * 64 * 64), (1, 5, 5), (4, 1028, 1028)],
                         ids=["vector_strided", "class_column", "one_short_row", "contiguous"])
def test_accumulate_vector_path_and_nan(R, n, stride):
    from protopformer_amd.interpret import ig_accumulate
    rng = np.random.default_rng(R + n)
    store = torch.full((R, stride), POISON, device="cuda")
    acc = store[:, :n]
    g0, g1 = rng.standard_normal((R, n)).astype(np.float32), rng.standard_normal((R, n)).astype(np.float32)
    g1[R - 1, n // 2] = np.nan
    ref = ig_accumulate(g1, 0.75, ig_accumulate(g0, 0.25, None, first=True, device=False), device=False)
    ig_accumulate(dev(g0), 0.25, acc, first=True)
    ig_accumulate(dev(g1), 0.75, acc)
    got = acc.cpu().numpy()
    assert np.isnan(got[R - 1, n // 2]) and int(np.isnan(got).sum()) == 1                         # the NaN stays in its element
    assert same_bits(got, ref)
    if stride > n:
        assert bool((store[:, n:] == POISON).all())


def test_accumulate_refuses_other_layouts():
    from protopformer_amd import ops
    g = torch.zeros((2, 3, 4, 4), device="cuda")
    both = torch.zeros((2, 2, 3, 4, 4), device="cuda")
    ops.ig_accumulate(g, 1.0, both[:, 1], first=True)                                             # one class column is the intended target
    with pytest.raises(ValueError, match="rows of acc must be contiguous"):
        ops.ig_accumulate(g, 1.0, torch.zeros((2, 3, 4, 8), device="cuda")[..., ::2])
    with pytest.raises(ValueError, match="acc must be an fp32 CUDA tensor"):
        ops.ig_accumulate(g, 1.0, both[:, 1, :2])
    with pytest.raises(ValueError, match="acc must be an fp32 CUDA tensor"):
        ops.ig_accumulate(g, 1.0, both[:, 1].double())
    with pytest.raises(ValueError, match="g must be contiguous"):
        ops.ig_accumulate(both[:, 1], 1.0, g)


# ------------------------------------------------------------------------------------------------ 3. ppf_ig_finish
FINISH_SHAPES = [(2, 1, 3, 32, 32, 16), (1, 2, 3, 16, 16, 16), (2, 3, 1, 12, 18, 6), (3, 8, 3, 64, 64, 16), (1, 1, 3, 224, 224, 16)]


@pytest.mark.parametrize("B,M,C,H,W,patch", FINISH_SHAPES, ids=["2x2_grid", "one_cell", "scalar_non_square", "M8_64", "224"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_finish_equals_the_referee(B, M, C, H, W, patch, tensor_baseline):
    from protopformer_amd.interpret import ig_finish
    rng = np.random.default_rng(H + W + M)
    acc = rng.standard_normal((B, M, C, H, W)).astype(np.float32)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else 0.375
    G = (H // patch) * (W // patch)
    ref_attr, ref_cell = ig_finish(acc, x, base, patch, device=False)
    accd, xd, bd = dev(acc), dev(x), dev(base) if tensor_baseline else base
    attr, cell64 = ig_finish(accd, xd, bd, patch)
    assert attr.dtype == torch.float32 and tuple(attr.shape) == acc.shape and cell64.dtype == torch.float64 and tuple(cell64.shape) == (B, M, G)
    got = attr.cpu().numpy()
    assert np.array_equal(bits(got), bits(ref_attr)), f"{int((bits(got) != bits(ref_attr)).sum())} of {got.size} attributions differ from the referee"
    worst = cells_within_bound(cell64.cpu().numpy(), got, patch, "device")
    assert np.array_equal(ref_cell.shape, (B, M, G))
    print(f"cell sums: largest error / bound = {worst:.3f}")
    again = ig_finish(accd, xd, bd, patch)
    assert torch.equal(again[0], attr) and torch.equal(again[1].view(torch.int64), cell64.view(torch.int64)), "a second run must be bit-identical"


def test_finish_nan_marks_its_own_cell_and_the_limits_launch_nothing():
    from protopformer_amd import _lib, ops
    rng = np.random.default_rng(5)
    B, M, C, H, W, patch = 2, 2, 3, 32, 32, 16
    acc = rng.standard_normal((B, M, C, H, W)).astype(np.float32)
    x = dev(rng.standard_normal((B, C, H, W)).astype(np.float32))
    clean = ops.ig_finish(dev(acc), x, 0.0, patch)[1].cpu().numpy()
    acc[1, 0, 2, 17, 3] = np.nan                                                                  # cell (1, 0) = 2 of sample 1, class column 0
    cell = ops.ig_finish(dev(acc), x, 0.0, patch)[1].cpu().numpy()
    bad = np.zeros((B, M, 4), dtype=bool)
    bad[1, 0, 2] = True
    assert np.isnan(cell[bad]).all() and np.array_equal(cell[~bad].view(np.int64), clean[~bad].view(np.int64))
    rec = _lib.start_recording()
    try:
        with pytest.raises(RuntimeError, match=r"ppf_ig_finish failed \(rc=-1\): ppf_ig_finish: M=9"):
            ops.ig_finish(torch.zeros((1, 9, 1, 16, 16), device="cuda"), torch.zeros((1, 1, 16, 16), device="cuda"), 0.0, 16)
        with pytest.raises(RuntimeError, match=r"ppf_ig_finish failed \(rc=-1\): ppf_ig_finish: patch=16 does not divide H=24"):
            ops.ig_finish(torch.zeros((1, 1, 1, 24, 32), device="cuda"), torch.zeros((1, 1, 24, 32), device="cuda"), 0.0, 16)
    finally:
        _lib.stop_recording()
    assert not rec.cmds, "a refused call must not reach the stream"
    with pytest.raises(ValueError, match="x must be"):
        ops.ig_finish(dev(acc), x[:1], 0.0, patch)
    with pytest.raises(ValueError, match="acc must be contiguous"):
        ops.ig_finish(dev(acc)[..., ::2], x[..., ::2], 0.0, patch)


# ------------------------------------------------------------------------------------------------ 4. through the micro models
STEPS, M_TOP = 4, 2


def host_logits(m, imgs):
    with torch.no_grad():
        return m.eval_branches(imgs if isinstance(imgs, torch.Tensor) else dev(imgs)).logits.cpu().numpy()


@pytest.fixture(scope="module", params=[("micro_deit.npz", False), ("micro_deit.npz", True), ("micro_cait.npz", False), ("micro_cait.npz", True)],
                ids=["deit_bf16", "deit_fp32", "cait_bf16", "cait_fp32"])
def model_case(request):
    """One model in one mode, one integrated_gradients call and its host copy, shared by the tests below and left unchanged."""
    from protopformer_amd.interpret import integrated_gradients
    name, precise = request.param
    sd, cfg, z = micro(name)
    m = build_micro(cfg, sd).eval()
    m.precise = precise
    x = dev(z["img"])
    r = integrated_gradients(m, x, top_classes=M_TOP, steps=STEPS)
    return dict(name=f"{name} {'fp32' if precise else 'bf16'}", m=m, x=x, img=z["img"], cfg=cfg, r=r, h=r.cpu())


def test_the_image_gradient_repeats_bit_for_bit_in_every_path(model_case):
    """What the pipeline comparison below rests on, in all four paths (tests/test_gpu_input_grad.py asserts it for the micro DeiT): the
    fp32 mode's talking-heads backward of CaiT adds dK / dV in a fixed order for this."""
    from protopformer_amd.interpret import input_gradient
    m, x, h, name = model_case["m"], model_case["x"], model_case["h"], model_case["name"]
    runs = [input_gradient(m, x, ("logit", h.targets[:, 0])) for _ in range(3)]
    for g, v in runs[1:]:
        assert torch.equal(g.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(v, runs[0][1]), f"{name}: the image gradient does not repeat"
    assert float(runs[0][0].abs().max()) > 0


def test_integrated_gradients_equal_the_referee_pipeline(model_case):
    from protopformer_amd.interpret import ig_accumulate, ig_finish, ig_point, ig_rule, input_gradient
    m, img, h, name = model_case["m"], model_case["img"], model_case["h"], model_case["name"]
    B, H, G = img.shape[0], img.shape[2], 16
    assert h.attribution.shape == (B, M_TOP, 3, H, H) and h.cell.shape == (B, M_TOP, G) and h.total.shape == (B, M_TOP) and h.total.dtype == np.float64
    assert h.value.shape == h.value_base.shape == (B, M_TOP) and h.targets.shape == (B, M_TOP) and h.targets.dtype == np.int32
    alphas, weights = ig_rule(STEPS, "midpoint")
    assert np.array_equal(h.alphas, alphas) and np.array_equal(h.weights, weights)
    acc = [None] * M_TOP
    for s, (a, w) in enumerate(zip(alphas.tolist(), weights.tolist())):
        point = dev(ig_point(img, a, 0.0, device=False))                                         # the host-made path point, one sample group of B
        for k in range(M_TOP):
            g, _ = input_gradient(m, point, ("logit", h.targets[:, k]))
            acc[k] = ig_accumulate(g.cpu().numpy(), w, acc[k], first=s == 0, device=False)
    attr, cell64 = ig_finish(np.stack(acc, axis=1), img, 0.0, H // 4, device=False)
    assert np.array_equal(bits(h.attribution), bits(attr)), f"{name}: the attribution differs from the referee pipeline"
    # cell = the device's fp64 cell sums rounded once to fp32, total = those sums added up: both against the referee's np.sum
    a64 = h.attribution.reshape(B, M_TOP, 3, 4, H // 4, 4, H // 4).astype(np.float64)
    bound = 3 * (H // 4) ** 2 * 2.0 ** -53 * np.abs(a64).sum(axis=(2, 4, 6)).reshape(B, M_TOP, G)
    assert (np.abs(h.cell.astype(np.float64) - cell64) <= bound + 2.0 ** -24 * np.abs(cell64)).all(), f"{name}: cell sums off the referee"
    assert (np.abs(h.total - cell64.sum(-1)) <= bound.sum(-1) + G * 2.0 ** -53 * np.abs(cell64).sum(-1)).all(), f"{name}: total off the referee"
    assert np.isfinite(h.attribution).all() and h.attribution.std() > 0


def test_value_value_base_and_delta(model_case):
    m, x, r, h, name = model_case["m"], model_case["x"], model_case["r"], model_case["h"], model_case["name"]
    B = x.shape[0]
    logits, blank = host_logits(m, x), host_logits(m, torch.zeros_like(x))
    rows = np.arange(B)[:, None]
    assert (h.targets >= 0).all() and np.array_equal(h.targets[:, 0], logits.argmax(1))
    assert np.array_equal(bits(h.value), bits(logits[rows, h.targets])), f"{name}: value is not the eval logit of x"
    assert np.array_equal(bits(h.value_base), bits(blank[rows, h.targets])), f"{name}: value_base is not the eval logit of the baseline image"
    want = h.total - (h.value.astype(np.float64) - h.value_base.astype(np.float64))
    assert np.array_equal(h.delta(), want) and np.array_equal(r.delta().cpu().numpy(), want)
    cells = h.cell.astype(np.float64)
    assert (np.abs(h.total - cells.sum(-1)) <= 16 * 2.0 ** -24 * np.abs(cells).sum(-1)).all()     # total = the sum of the cells before their fp32 rounding
    rel = np.abs(want) / np.abs(h.value.astype(np.float64) - h.value_base.astype(np.float64))
    print(f"{name}: completeness gap at {STEPS} midpoint steps: |delta| / |value - value_base| mean {rel.mean():.4f} worst {rel.max():.4f}")
    report(f"ig_delta_{name.replace(' ', '_')}", steps=STEPS, mean_rel=float(rel.mean()), worst_rel=float(rel.max()), worst_abs=float(np.abs(want).max()))


def test_repeats_side_effects_and_the_guard(model_case):
    from protopformer_amd.interpret import IntegratedGradients, integrated_gradients
    m, x, r = model_case["m"], model_case["x"], model_case["r"]
    again = integrated_gradients(m, x, top_classes=M_TOP, steps=STEPS)
    for f in IntegratedGradients.FIELDS:
        a, b = getattr(again, f), getattr(r, f)
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"a second call: {f} differs"
    assert not m.training and all(p.grad is None for p in m.parameters())
    m.train()
    try:
        integrated_gradients(m, x, top_classes=1, steps=1)
        assert m.training, "the model was found in train mode and must be left in it"
    finally:
        m.eval()
    assert all(p.grad is None for p in m.parameters())
    pname, p = next(iter(m.named_parameters()))
    pending = torch.zeros_like(p)
    pending.view(-1)[0] = 0.5
    p.grad = pending
    try:
        with pytest.raises(RuntimeError, match=r"integrated_gradients: 1 parameters already hold a .grad \(" + pname.replace(".", r"\.")):
            integrated_gradients(m, x, steps=1)
        assert p.grad is pending and float(pending.view(-1)[0]) == 0.5                            # refused before anything ran
    finally:
        p.grad = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        integrated_gradients(m, x.cpu())
    for bad in (("logit",), ("proto", "both", [0] * x.shape[0]), ("logit", [0] * (x.shape[0] + 1)), ("logit", [10 ** 6] * x.shape[0])):
        with pytest.raises(ValueError):
            integrated_gradients(m, x, target=bad, steps=1)
    with pytest.raises(ValueError, match=r"outside \[1, 8\]"):
        integrated_gradients(m, x, target=("logit", np.zeros((x.shape[0], 9), dtype=np.int64)), steps=1)
    with pytest.raises(ValueError, match="rule must be one of"):
        integrated_gradients(m, x, rule="simpson")


def test_one_endpoint_step_is_gradient_times_input_and_the_groups_are_kept(model_case):
    from protopformer_amd.interpret import input_gradient, integrated_gradients
    m, x, cfg = model_case["m"], model_case["x"], model_case["cfg"]
    B = x.shape[0]
    protos = torch.arange(B) * cfg["protos_per_class"] + 1
    one = integrated_gradients(m, x, target=("proto", "local", protos), steps=1, rule="endpoint", baseline=0.0)
    g, v = input_gradient(m, x, ("proto", "local", protos))
    assert one.target == ("proto", "local") and tuple(one.attribution.shape) == (B, 1) + tuple(x.shape[1:])
    assert torch.equal(one.attribution[:, 0].view(torch.int32), (g * x).view(torch.int32)), "gradient x input, bit for bit"
    assert torch.allclose(one.value[:, 0], v, rtol=1e-5, atol=0)                                  # a forward without a graph against one that saves for backward
    # sample groups of two: each group is its own input_gradient call, as here
    two = integrated_gradients(m, x, target=("proto", "local", protos), steps=1, rule="endpoint", batch_size=2)
    parts = torch.cat([input_gradient(m, x[b:b + 2], ("proto", "local", protos[b:b + 2]))[0] for b in range(0, B, 2)])
    assert torch.equal(two.attribution[:, 0].view(torch.int32), (parts * x).view(torch.int32))
    base = torch.full_like(x, 0.25)
    t = integrated_gradients(m, x, target=("logit", [1] * B), steps=2, rule="trapezoid", baseline=base)
    c = integrated_gradients(m, x, target=("logit", [1] * B), steps=2, rule="trapezoid", baseline=0.25)
    assert t.alphas.tolist() == [0.0, 0.5, 1.0] and torch.equal(t.attribution, c.attribution) and torch.equal(t.value_base, c.value_base)


def order_of_scores(score):
    """The contract's sort of given scores [G]: NaN last, score descending, smaller cell."""
    nan = np.isnan(score)
    return np.lexsort((np.arange(score.size), np.where(nan, np.float32(0), -score), nan))


def prob_reference(logits, cls):
    """(fp64 softmax probability of the class per row, the relative bound (C + 8 + 2 max|l - max l|) * 2^-24 per row)."""
    l = np.asarray(logits, dtype=np.float64)
    d = l - l.max(axis=1, keepdims=True)
    e = np.exp(d)
    return e[np.arange(l.shape[0]), cls] / e.sum(axis=1), (l.shape[1] + 8 + 2 * np.abs(d).max(axis=1)) * 2.0 ** -24


def forward_logits(m, imgs, bs):
    with torch.no_grad():
        return torch.cat([m._branches(dev(imgs[i:i + bs]), want_dist=False).logits for i in range(0, len(imgs), bs)]).cpu().numpy()


def test_the_ig_order_of_the_faithfulness_curves(model_case):
    from protopformer_amd.interpret import default_counts, faithfulness_curves
    m, x, img, h, name = model_case["m"], model_case["x"], model_case["img"], model_case["h"], model_case["name"]
    B, M, G = img.shape[0], M_TOP, 16
    f = faithfulness_curves(m, x, top_classes=M, batch_size=B, order="ig", ig=dict(steps=STEPS))
    assert f.ig is not None and f.rise is None and torch.equal(f.score.view(torch.int32), f.ig.cell.view(torch.int32)), "score must be .ig.cell, bit for bit"
    g = f.cpu()
    assert np.array_equal(bits(g.score), bits(g.ig.cell)) and np.array_equal(bits(g.ig.cell), bits(h.cell)), f"{name}: not the cells of integrated_gradients"
    assert np.array_equal(g.classes, h.targets) and np.array_equal(g.counts, default_counts(G)) and set(g.curves) == {"deletion", "insertion"}
    for b in range(B):
        for k in range(M):
            assert np.array_equal(g.order[b, k], order_of_scores(g.score[b, k])), (b, k)
            assert (g.rank[b, k, g.order[b, k]] == np.arange(G)).all()
    S = len(g.counts)
    cls = g.classes.reshape(-1)
    p_clean, b_clean = prob_reference(forward_logits(m, np.repeat(img, M, axis=0), B), cls)
    p_blank, b_blank = prob_reference(forward_logits(m, np.zeros((B * M,) + img.shape[1:], dtype=np.float32), B), cls)
    for mode in ("deletion", "insertion"):
        ends = g.curves[mode].reshape(B * M, S).astype(np.float64)
        full, none = (ends[:, 0], ends[:, -1]) if mode == "deletion" else (ends[:, -1], ends[:, 0])
        assert (np.abs(full - p_clean) <= b_clean * p_clean).all(), f"{name} {mode}: the untouched end is not the unperturbed probability"
        assert (np.abs(none - p_blank) <= b_blank * p_blank).all(), f"{name} {mode}: the emptied end is not the all-baseline probability"
    assert all(p.grad is None for p in m.parameters())
    other = faithfulness_curves(m, x, top_classes=M, batch_size=B)                               # the default order is untouched and carries nothing
    assert other.ig is None and other.rise is None and not torch.equal(other.score, f.score)
    with pytest.raises(ValueError, match="mode must be one of"):
        faithfulness_curves(m, x, order="smoothgrad")


# ------------------------------------------------------------------------------------------------ 5. the tools
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


@pytest.fixture(scope="module")
def cub_case(tmp_path_factory):
    import mini_trees
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    root = tmp_path_factory.mktemp("ig_tools")
    tree = str(root / "data")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(root / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    return dict(root=root, tree=tree, ck=ck)


def test_faithfulness_tool_with_the_ig_order_on_the_miniature_cub_tree(cub_case):
    from protopformer_amd import faithfulness as tool
    out = str(cub_case["root"] / "faith")
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", cub_case["tree"], "--output_dir", out, "--resume", cub_case["ck"],
                                              "--steps", "4", "--max_images", "6", "--orders", "evidence", "random", "ig", "--ig_steps", "2", *MODEL_FLAGS])
    doc = json.load(open(tool.main(args)))
    assert doc["images"] == 6 and doc["counts"] == [0, 49, 98, 147, 196] and doc["grid_cells"] == 196
    assert list(doc["orders"]) == ["evidence", "random", "ig"] and all(set(v) == {"deletion", "insertion"} for v in doc["orders"].values())
    assert set(doc["vs_random"]) == {"evidence", "ig"}
    for v in doc["vs_random"].values():
        assert set(v) == {"deletion_auc_minus_random", "insertion_auc_minus_random", "informative"}
    ig, ev = doc["orders"]["ig"], doc["orders"]["evidence"]
    for mode in ("deletion", "insertion"):
        assert len(ig[mode]["curve"]) == 5 and 0.0 <= ig[mode]["auc"] <= 1.0
    # the ends do not depend on the order (the tolerance of the RISE tool test: ppf_class_prob's bound at C = 200 is below 2e-5 relative)
    for a, b in ((ig["deletion"]["curve"][0], ev["deletion"]["curve"][0]), (ig["insertion"]["curve"][-1], ev["insertion"]["curve"][-1]),
                 (ig["deletion"]["curve"][-1], ev["deletion"]["curve"][-1]), (ig["insertion"]["curve"][0], ev["insertion"]["curve"][0])):
        assert abs(a - b) <= 4e-5 * abs(b), (a, b)


def test_attribute_tool_on_the_miniature_cub_tree(cub_case):
    from protopformer_amd import attribute as tool
    out = str(cub_case["root"] / "attr")
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", cub_case["tree"], "--output_dir", out, "--resume", cub_case["ck"],
                                              "--steps", "4", "--max_images", "6", "--save-maps", *MODEL_FLAGS])
    doc = json.load(open(tool.main(args)))
    assert doc["images"] == 6 == len(doc["per_image"]) and doc["grid_cells"] == 196 and doc["patch"] == 16
    assert doc["settings"]["steps"] == 4 and doc["settings"]["rule"] == "midpoint" and doc["mean_relative_gap"] >= 0
    assert len({r["image_id"] for r in doc["per_image"]}) == 6
    for r in doc["per_image"]:
        (col,) = r["classes"]
        assert all(np.isfinite(col[k]) for k in ("value", "value_base", "total", "delta"))
        assert abs(col["delta"] - (col["total"] - (col["value"] - col["value_base"]))) <= 1e-12 * max(1.0, abs(col["total"]))
        scores = [c["score"] for c in col["cells"]]
        assert len(scores) == 10 and scores == sorted(scores, reverse=True)
        x0, y0, x1, y1 = col["cells"][0]["box"]
        assert (x1 - x0, y1 - y0) == (16, 16) and 0 <= x0 < 224 and 0 <= y0 < 224
    z = np.load(os.path.join(out, "attributions.npz"))
    assert z["cell"].shape == (6, 1, 196) and z["cell"].dtype == np.float32 and z["map"].shape == (6, 1, 224, 224) and z["image_ids"].shape == (6,)
    assert np.isfinite(z["cell"]).all() and np.array_equal(z["classes"][:, 0], [r["classes"][0]["target"] for r in doc["per_image"]])
    best = [r["classes"][0]["cells"][0] for r in doc["per_image"]]
    assert [c["cell"] for c in best] == z["cell"][:, 0].argmax(-1).tolist()
    # a cell's score is the sum of its pixels' attributions over the channels (fp32 map sums against the fp64 cell sums)
    cells_of_map = z["map"].reshape(6, 1, 14, 16, 14, 16).astype(np.float64).sum(axis=(3, 5)).reshape(6, 1, 196)
    mass = np.abs(z["map"]).reshape(6, 1, 14, 16, 14, 16).astype(np.float64).sum(axis=(3, 5)).reshape(6, 1, 196)
    assert (np.abs(cells_of_map - z["cell"]) <= 4 * 2.0 ** -24 * mass).all()                      # two roundings of the channel sum, one of the cell
