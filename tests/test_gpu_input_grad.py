"""The gradient with respect to the image on the GPU: ppf_col2im_patch_f32 inverts the im2col kernels bit for bit; the fp32 verification
mode's image gradient is held to autograd of the CPU oracle at the north-star tolerance (1e-3, element by element) for the training
loss, a class logit and a local / global prototype activation on the three reference-generated micro fixtures; the bf16 product path
is gated on the per-sample cosine against the fp32 mode; repeats are bit-identical; without a gradient request nothing is launched and
nothing changes; interpret.input_gradient refuses to run over pending parameter gradients and leaves none behind."""
import functools

import pytest
import torch

from helpers import assert_elementwise, build_micro, micro, rel_err, report
from oracle import ppf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-3          # BASELINE.json north_star: "within 1e-3 rel fp32", the tolerance every parameter gradient is held to
FIXTURES = ["micro_deit.npz", "micro_cait.npz", "micro_deit_bottleneck.npz"]
TARGETS = ("loss", "logit", "proto_local", "proto_global")

# Per-sample cosine of the product path's image gradient against the fp32 mode's (the reference for this number is the fp32 mode, never
# the path under test), measured on an MI355X over the three fixtures and the four targets (profiles/alignment_cost.txt): the worst is
# COS_WORST; the gate is 1 - 4 * (1 - worst), as the project's parameter-gradient cosines were set.
# Measured (min over targets and samples): micro_deit 0.99995438 (d proto_global), micro_cait 0.99996608; micro_deit_bottleneck 0.93967216
# (d proto_global; d loss 0.96035946, d logit 0.97662056, d proto_local 0.99998447).  The bottleneck head has ReLU layers: the bf16
# backbone moves a few pre-activations across zero and whole units gate their gradient differently -- the property
# test_gpu_e2e.py::test_micro_deit_bottleneck_head_product_path_against_reference_fixture records for the parameter gradients (per-tensor
# cosines 0.93-0.98 there).  So the heads get a gate each, by the same rule from their own worst.
COS_WORST = {"regular": 0.99995438, "bottleneck": 0.93967216}
COS_GATE = {k: 1.0 - 4.0 * (1.0 - v) for k, v in COS_WORST.items()}          # 0.99981752 and 0.75868864


# ------------------------------------------------------------------------------------------------ col2im
@pytest.mark.parametrize("B,C,H,W,p", [(2, 3, 32, 48, 16), (1, 3, 16, 16, 16), (2, 1, 12, 18, 6)], ids=["2x3_patches", "one_patch", "scalar_path"])
def test_col2im_inverts_im2col_bit_for_bit(B, C, H, W, p):
    from protopformer_amd import ops
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H)).cuda()
    cols = ops.im2col_patch_f32(x, p)
    assert cols.shape == (B * (H // p) * (W // p), C * p * p)
    back = ops.col2im_patch(cols, B, C, H, W, p)
    assert back.shape == x.shape and back.dtype == torch.float32 and torch.equal(back.view(torch.int32), x.view(torch.int32))
    if p % 8 == 0:                                              # the bf16 im2col writes the same column order
        xb = x.bfloat16().float()
        assert torch.equal(ops.col2im_patch(ops.im2col_patch(xb, p).float(), B, C, H, W, p), xb)
    # the columns of one patch are (c, py, px): patch (gy, gx) = (0, 1) of sample 0 is x[0, :, 0:p, p:2p]
    if W // p > 1:
        assert torch.equal(cols[1].reshape(C, p, p), x[0, :, 0:p, p:2 * p])
    with pytest.raises(ValueError, match="cols must be"):
        ops.col2im_patch(cols[:-1], B, C, H, W, p)
    with pytest.raises(ValueError, match="patch must divide"):
        ops.col2im_patch(cols, B, C, H + 1, W, p)


# ------------------------------------------------------------------------------------------------ the oracle's image gradients, once per fixture
def _targets(z, cfg):
    label = torch.from_numpy(z["label"]).long()
    return label, label * cfg["protos_per_class"] + 1, label * cfg["global_per_class"]            # class, local prototype, global prototype per sample


@functools.lru_cache(maxsize=None)
def oracle_gradients(fixture):
    """Autograd of the CPU oracle with img.requires_grad_(): the image gradient of (a) the fixture's training loss in train mode and, in
    eval mode, of (b) one class logit and (c) one local and one global prototype activation per sample; with the reserved indices."""
    sd, cfg, z = micro(fixture)
    label, pl, pg = _targets(z, cfg)
    rows = torch.arange(label.shape[0])
    out = {}
    img = torch.from_numpy(z["img"]).clone().requires_grad_()
    o = O.ppnet_forward({k: v.clone() for k, v in sd.items()}, img, cfg, train=True)
    _, parts = O.train_loss(o, label, cfg, with_ppc=True)
    out["loss"] = torch.autograd.grad(parts["ce"] + 0.1 * parts["ppc_cov"] + 0.5 * parts["ppc_mean"], img)[0]
    out["idx_train"] = o["reserve_idx"].long()
    img = torch.from_numpy(z["img"]).clone().requires_grad_()
    params = {k: v.clone() for k, v in sd.items()}
    o = O.ppnet_forward(params, img, cfg, train=False)
    out["idx_eval"] = o["reserve_idx"].long()
    B, P = label.shape[0], cfg["num_prototypes"]
    act_l = o["total_proto_act"].reshape(B, P, -1).max(-1)[0]
    act_g = O.proto_activations(o["cls_tokens"], params["prototype_vectors_global"])[0]
    vals = dict(logit=o["logits"][rows, label], proto_local=act_l[rows, pl], proto_global=act_g[rows, pg])
    for k, v in vals.items():
        out[k] = torch.autograd.grad(v.sum(), img, retain_graph=True)[0]
        out["value_" + k] = v.detach()
    return out


def model_gradients(m, z, cfg, precise):
    """The same four image gradients from the model: (a) by a plain backward through PPNet.forward in train mode with img.requires_grad_(),
    (b) and (c) through interpret.input_gradient.  Returns (gradients, values, reserved indices of the train forward); the model keeps the
    parameter gradients of (a)."""
    from protopformer_amd.interpret import input_gradient
    from protopformer_amd.protopformer import CrossEntropyLoss
    m.precise = precise
    label, pl, pg = _targets(z, cfg)
    x = torch.from_numpy(z["img"]).cuda()
    grads, vals = {}, {}
    for key, target in (("logit", ("logit", label)), ("proto_local", ("proto", "local", pl)), ("proto_global", ("proto", "global", pg))):
        grads[key], vals[key] = input_gradient(m, x, target)
        assert grads[key].shape == x.shape and grads[key].dtype == torch.float32 and vals[key].shape == (x.shape[0],)
        assert all(p.grad is None for p in m.parameters()) and not x.requires_grad
    m.train()
    xg = x.clone().requires_grad_()
    logits, aux = m(xg)
    ce = CrossEntropyLoss()(logits, label.cuda())
    cov, mean = m.get_PPC_loss(aux[2], aux[3], aux[4], label.cuda())
    (ce + 0.1 * cov + 0.5 * mean).backward()
    torch.cuda.synchronize()
    grads["loss"] = xg.grad
    return grads, vals, m._ppc_cache[1].cpu().long()


@pytest.mark.parametrize("fixture", FIXTURES)
def test_precise_image_gradient_matches_autograd_of_the_oracle(fixture):
    sd, cfg, z = micro(fixture)
    ref = oracle_gradients(fixture)
    m = build_micro(cfg, sd)
    grads, vals, idx = model_gradients(m, z, cfg, precise=True)
    assert torch.equal(idx, ref["idx_train"]) and torch.equal(ref["idx_eval"], ref["idx_train"]), "reserved-token indices must be bit-exact"
    with torch.no_grad():
        m.eval()
        assert torch.equal(m._tokens(torch.from_numpy(z["img"]).cuda())[2].cpu().long(), ref["idx_eval"])
    worst = {}
    for key in TARGETS:
        assert float(ref[key].abs().max()) > 0, key
        worst[key] = rel_err(grads[key], ref[key])
        print(f"{fixture} fp32 mode d {key} / d image: rel err {worst[key]:.3e}")
    report(f"input_grad_precise_{fixture}", **worst)
    for key in TARGETS:
        assert_elementwise(grads[key], ref[key], TOL, f"{fixture}: d {key} / d image")
        if key != "loss":
            assert rel_err(vals[key], ref["value_" + key]) < TOL, key
    # (a) ran with the image gradient attached to the end of the backward: every parameter gradient still matches the fixture
    n = 0
    for name, p in m.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        g = p.grad.detach().float().cpu().reshape(-1)
        if f"grad/{name}" in z.files:
            r = torch.from_numpy(z[f"grad/{name}"]).reshape(-1)
        else:
            g, r = g[torch.from_numpy(z[f"grad_idx/{name}"])], torch.from_numpy(z[f"grad_val/{name}"])
        if float(r.abs().max()) < 1e-7:
            assert float(g.abs().max()) < 1e-6, name
            continue
        assert_elementwise(g, r, TOL, f"{fixture} grad/{name} with the image gradient requested")
        n += 1
    assert n >= 20, n


def _cosines(a, b):
    a, b = a.double().reshape(a.shape[0], -1).cpu(), b.double().reshape(b.shape[0], -1).cpu()
    return ((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).tolist()


@pytest.mark.parametrize("fixture", FIXTURES)
def test_product_path_image_gradient_points_where_the_fp32_mode_does(fixture):
    """Per-sample cosine of the bf16 product path's image gradient against the fp32 verification mode's, same inputs and the same four
    targets.  Measured on an MI355X (worst over targets and samples): regular head 0.99995438 (micro_deit; micro_cait 0.99996608), bottleneck
    head 0.93967216 (ReLU units flipped by bf16 rounding, see COS_WORST above); gates 1 - 4 * (1 - worst) = 0.99981752 and 0.75868864
    (profiles/alignment_cost.txt)."""
    sd, cfg, z = micro(fixture)
    g32, _, idx32 = model_gradients(build_micro(cfg, sd), z, cfg, precise=True)
    g16, _, idx16 = model_gradients(build_micro(cfg, sd), z, cfg, precise=False)
    assert torch.equal(idx16, idx32), "the fixtures are tie-free at the reservation boundary: both paths reserve the same tokens"
    cos = {key: _cosines(g16[key], g32[key]) for key in TARGETS}
    for key in TARGETS:
        print(f"{fixture} bf16 vs fp32 cosine of d {key} / d image per sample: " + " ".join(f"{c:.6f}" for c in cos[key]))
    report(f"input_grad_cosine_{fixture}", **{key: min(c) for key, c in cos.items()})
    gate = COS_GATE[cfg["add_on"]]
    for key in TARGETS:
        assert min(cos[key]) >= gate, f"{fixture} {key}: cosine {min(cos[key]):.6f} below the gate {gate:.6f}"


@pytest.mark.parametrize("precise", [False, True], ids=["bf16", "fp32"])
def test_repeated_input_gradients_are_bit_identical(precise):
    from protopformer_amd.interpret import input_gradient
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    m.precise = precise
    x = torch.from_numpy(z["img"]).cuda()
    label, pl, _ = _targets(z, cfg)
    for target in (("logit", label), ("proto", "local", pl)):
        (g1, v1), (g2, v2) = input_gradient(m, x, target), input_gradient(m, x, target)
        assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(v1, v2), target[:-1]
        assert float(g1.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    # samples are independent: row b of the batch's gradient is sample b's own gradient (same kernels at both batch sizes in the fp32 mode)
    if precise:
        g_all, _ = input_gradient(m, x, ("logit", label))
        g_one, _ = input_gradient(m, x[1:2], ("logit", label[1:2]))
        assert_elementwise(g_one[0], g_all[1], 1e-5, "sample 1 alone against its row of the batch")


def _recorded_step(m, x, label, with_image_grad):
    """One train forward + backward with every library call recorded: (loss, entry-point names in launch order)."""
    from protopformer_amd import _lib
    from protopformer_amd.protopformer import CrossEntropyLoss
    xg = x.clone().requires_grad_(with_image_grad)
    rec = _lib.start_recording()
    try:
        logits, aux = m(xg)
        ce = CrossEntropyLoss()(logits, label)
        cov, mean = m.get_PPC_loss(aux[2], aux[3], aux[4], label)
        loss = ce + 0.1 * cov + 0.5 * mean
        loss.backward()
    finally:
        _lib.stop_recording()
    torch.cuda.synchronize()
    return loss.detach(), [c[3] for c in rec.cmds if c[0] == _lib.Recorder.CALL], xg


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
@pytest.mark.parametrize("precise", [False, True], ids=["bf16", "fp32"])
def test_no_new_launch_without_a_gradient_request(fixture, precise):
    sd, cfg, z = micro(fixture)
    x, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    runs = {}
    for want in (False, True):
        m = build_micro(cfg, sd).train()
        m.precise = precise
        loss, names, xg = _recorded_step(m, x, label, want)
        runs[want] = (loss, names, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, xg.grad)
    (l0, n0, g0, x0), (l1, n1, g1, x1) = runs[False], runs[True]
    assert x0 is None and x1 is not None and x1.shape == x.shape
    assert "ppf_col2im_patch_f32" not in n0 and n1.count("ppf_col2im_patch_f32") == 1
    # the image gradient is exactly two launches at the end of the backward (its GEMM and col2im); everything else is the same list
    extra = ["ppf_sgemm", "ppf_col2im_patch_f32"] if precise else ["ppf_gemm_bf16", "ppf_col2im_patch_f32"]
    at = n1.index("ppf_col2im_patch_f32")
    assert n1[at - 1:at + 1] == extra and n1[:at - 1] + n1[at + 1:] == n0, (len(n0), len(n1))
    assert torch.equal(l0, l1) and set(g0) == set(g1)
    if precise:                                                  # fp32 mode: weight gradients by fp32 atomics in places, equal to rounding
        for n in g0:
            assert rel_err(g1[n], g0[n]) < 1e-5 or float(g0[n].abs().max()) < 1e-7, n
    else:
        assert all(torch.equal(g0[n], g1[n]) for n in g0), "the product path's parameter gradients changed with the image gradient requested"


def test_replayed_train_step_records_the_eager_list():
    """The recorded and replayed training step issues what an eager step issues: its input never requires a gradient, so neither list
    holds the image gradient's launches (measured on the micro DeiT: 186 library calls in both;
    test_no_new_launch_without_a_gradient_request shows that a backward without the request is the one with it minus its two launches)."""
    from protopformer_amd import _lib
    from protopformer_amd.engine import FlatAdamW, ReplayedTrainStep, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    x, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    m = build_micro(cfg, sd).train()
    step = ReplayedTrainStep(m, CrossEntropyLoss(), FlatAdamW(m), epoch=20, warmup=1)
    for _ in range(3):                                           # eager, recorded, replayed
        loss = step(x, label)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    replayed = [c[3] for c in step.rec.cmds if c[0] == _lib.Recorder.CALL]
    m2 = build_micro(cfg, sd).train()
    opt2 = FlatAdamW(m2)
    train_one_step(m2, CrossEntropyLoss(), x, label, opt2, epoch=20)                 # the warm-up step, as above
    rec = _lib.start_recording()
    try:
        train_one_step(m2, CrossEntropyLoss(), x, label, opt2, epoch=20)
    finally:
        _lib.stop_recording()
    eager = [c[3] for c in rec.cmds if c[0] == _lib.Recorder.CALL]
    print(f"micro DeiT train step: {len(replayed)} recorded library calls")
    assert replayed == eager and len(replayed) > 50
    assert "ppf_col2im_patch_f32" not in replayed
    Np, K = (cfg["img"] // 16) ** 2, 3 * 16 * 16
    wide = [c for c in step.rec.cmds if c[0] == _lib.Recorder.CALL and c[3] == "ppf_gemm_bf16" and c[2][3:5] == (x.shape[0] * Np, K)
            and c[2][9:11] == (0, 1)]                            # dtok [B*Np, D] . W [D, C*p*p]: (trans_a, trans_b) = (0, 1)
    assert not wide, "a GEMM with the shape of the embed input gradient is in the training step"


def test_input_gradient_guards_the_parameter_gradients():
    from protopformer_amd.interpret import input_gradient
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    x = torch.from_numpy(z["img"]).cuda()
    label = torch.from_numpy(z["label"])
    p = m.features.norm.weight
    pending = torch.zeros_like(p)
    pending[3] = 0.5
    p.grad = pending
    with pytest.raises(RuntimeError, match=r"1 parameters already hold a .grad \(features.norm.weight"):
        input_gradient(m, x, ("logit", label))
    assert p.grad is pending and float(pending[3]) == 0.5       # refused before anything ran: the pending gradient is untouched
    p.grad = None
    # a training step in flight: every parameter holds its gradient
    from protopformer_amd.protopformer import CrossEntropyLoss
    m.train()
    CrossEntropyLoss()(m(x)[0], label.cuda()).backward()
    with pytest.raises(RuntimeError, match="already hold a .grad"):
        input_gradient(m, x, ("logit", label))
    kept = m.features.norm.weight.grad
    assert kept is not None and float(kept.abs().max()) > 0
    m.zero_grad(set_to_none=True)
    m.eval()
    # the zero-filled views the flat store attaches when it is built hold nothing: not a pending gradient
    fresh = build_micro(cfg, sd)
    with torch.no_grad():
        fresh.eval()
        fresh._branches(x, want_dist=False)
    assert all(q.grad is not None and not bool(q.grad.any()) for q in fresh.features.parameters())
    input_gradient(fresh, x, ("logit", label))
    assert all(q.grad is None for q in fresh.parameters())
    was = m.training
    g, v = input_gradient(m, x, ("logit", label))
    assert all(q.grad is None for q in m.parameters()) and m.training == was and x.grad is None
    with torch.no_grad():
        m.eval()
        logits = m._branches(x, want_dist=False).logits
    assert rel_err(v, logits[torch.arange(4), label.cuda()]) < TOL               # the value is the eval logit (a forward that saves for backward)
    for bad in (("logit",), ("proto", "both", label), ("logits", label), ("logit", label[:2]), ("logit", label + 1000)):
        with pytest.raises(ValueError):
            input_gradient(m, x, bad)
    with pytest.raises(RuntimeError, match="CUDA"):
        input_gradient(m, x.cpu(), ("logit", label))
    assert all(q.grad is None for q in m.parameters())
