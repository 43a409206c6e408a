"""KernelSHAP on the GPU: ppf_shap_coalitions, ppf_shap_apply, ppf_shap_gram and ppf_shap_solve against the numpy referees of interpret.py
(shap_coalitions_from_ids / shap_apply / shap_gram / shap_solve with device=False), interpret.kernel_shap and the 'shap' order of
faithfulness_curves through the micro models against the referee pipeline, and the command-line tool on the miniature CUB tree.

Coalitions, masked images, the Gram matrix and the right-hand sides are compared bit for bit (the contract in include/ppf_hip.h).  The
solve is fp64 Cholesky on both sides but not the same program, so it is held to a forward-error bound of the factorisation,
E = d * cond_2(A) * 2^-52 * max|phi_ref|: max|phi - phi_ref| <= E and |sum phi - delta| <= d * E.  The class probabilities in between come
from the model's forward and ppf_class_prob and are held to that kernel's bound, a relative error of (C + 8 + 2 max|l - max l|) * 2^-24
(tests/test_gpu_faithfulness.py).

Measured on the MI355X (largest error over the bound E, printed by the tests): see profiles/shap_cost.txt."""
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


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def words(coal):
    """The uint32 coalition words of a device tensor (held as int32) or of a referee's array."""
    a = coal.cpu().numpy() if isinstance(coal, torch.Tensor) else np.asarray(coal)
    return np.ascontiguousarray(a).view(np.uint32)


def coalitions(ids, s, N, seed=0):
    from protopformer_amd.interpret import shap_coalitions_from_ids
    return shap_coalitions_from_ids(ids, s, N, seed, device=False)


def solve_bound(A, phi_ref):
    """E per image [B]: d * cond_2(A) * 2^-52 * max|phi_ref| over the image's finite rows."""
    d = A.shape[1]
    return np.array([d * np.linalg.cond(A[b].astype(np.float64)) * 2.0 ** -52 * np.nanmax(np.abs(phi_ref[b])) for b in range(A.shape[0])])


# ------------------------------------------------------------------------------------------------ 1. ppf_shap_coalitions
@pytest.mark.parametrize("s,N", [(2, 2), (2, 16), (4, 64), (7, 10), (14, 6)])
def test_coalitions_equal_the_referee(s, N):
    from protopformer_amd.interpret import shap_coalitions_from_ids
    for seed in ((1 << 35) + 11, 3):
        coal = shap_coalitions_from_ids(dev(IDS), s, N, seed)                                    # IDS holds an id above 2^40
        assert coal.dtype == torch.int32 and tuple(coal.shape) == (3, N, (s * s + 31) // 32)
        assert np.array_equal(words(coal), coalitions(IDS, s, N, seed)), f"s={s} N={N} seed={seed}: coalitions differ from the referee"
    one = shap_coalitions_from_ids(dev(IDS[1:2]), s, N, 3)                                        # the batch does not enter
    assert torch.equal(one[0], coal[1])


def test_coalitions_refuse_a_bad_table_and_bad_sizes():
    from protopformer_amd import ops
    from protopformer_amd.interpret import shap_size_table
    ids, t = dev(IDS), shap_size_table(16)
    for bad in (t[:-1], t[::-1].copy(), np.concatenate([t[:-1], [t[-1] - 1]]), t.astype(np.float64)):
        with pytest.raises(ValueError, match="table must hold 15 non-decreasing integers that end at 2\\^24"):
            ops.shap_coalitions(ids, 4, 8, bad)
    with pytest.raises(RuntimeError, match="ppf_shap_coalitions.*N=7"):
        ops.shap_coalitions(ids, 4, 7, t)
    with pytest.raises(RuntimeError, match="ppf_shap_coalitions.*s=15"):
        ops.shap_coalitions(ids, 15, 8, np.concatenate([np.zeros(223, dtype=np.int32), [1 << 24]]))


# ------------------------------------------------------------------------------------------------ 2. ppf_shap_apply
@pytest.mark.parametrize("H,s,N,n0,Nc", [(32, 2, 6, 0, 6), (32, 2, 6, 2, 3), (64, 4, 8, 1, 5), (224, 7, 4, 1, 3), (224, 14, 4, 0, 2), (32, 2, 1030, 3, 1027)],
                         ids=["32_s2_all", "32_s2_middle", "64_s4_middle", "224_s7_Nc3", "224_s14_Nc2", "three_lds_stages"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_apply_equals_the_referee_bit_for_bit(H, s, N, n0, Nc, tensor_baseline):
    from protopformer_amd.interpret import shap_apply
    rng = np.random.default_rng(H + s + N)
    B, Cc = (1, 2) if N > 1000 else (2, 3)
    x = rng.standard_normal((B, Cc, H, H)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else -0.375
    coal = coalitions(IDS[:B], s, N, seed=7)
    ref = shap_apply(x, coal, s, n0, Nc, base, device=False)
    got = shap_apply(dev(x), dev(coal.view(np.int32)), s, n0, Nc, dev(base) if tensor_baseline else base)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.shape == ref.shape == (Nc, B, Cc, H, H)
    assert np.array_equal(bits(got), bits(ref)), f"{int((bits(got) != bits(ref)).sum())} of {got.size} elements differ from the referee"


def test_apply_other_channel_counts_out_buffer_and_refusals():
    from protopformer_amd import ops
    from protopformer_amd.interpret import shap_apply
    rng = np.random.default_rng(1)
    H, s = 32, 2
    coal = coalitions(IDS, s, 4)
    cd = dev(coal.view(np.int32))
    for Cc in (1, 4, 7):
        x = rng.standard_normal((3, Cc, H, H)).astype(np.float32)
        got = shap_apply(dev(x), cd, s, baseline=0.5).cpu().numpy()
        assert np.array_equal(bits(got), bits(shap_apply(x, coal, s, baseline=0.5, device=False))), f"Cc={Cc}"
    x = dev(rng.standard_normal((3, 3, H, H)).astype(np.float32))
    buf = torch.full((6, 3, 3, H, H), 7.0, device="cuda")
    out = ops.shap_apply(x, cd, s, 1, 2, 0.0, out=buf[:2])
    assert out.data_ptr() == buf.data_ptr() and bool((buf[2:] == 7.0).all())                    # nothing past the chunk is written
    assert torch.equal(out, ops.shap_apply(x, cd, s, 1, 2, 0.0))
    pair = ops.shap_apply(x, cd, s, 0, 2, 3.0)                                                    # a pair covers the image exactly once
    assert torch.equal(torch.where(pair[0] == 3.0, pair[1], pair[0]), x)
    with pytest.raises(RuntimeError, match="ppf_shap_apply.*n0=3"):
        ops.shap_apply(x, cd, s, 3, 2)
    with pytest.raises(RuntimeError, match="ppf_shap_apply.*multiple of 4"):
        ops.shap_apply(x[:, :, :24, :24].contiguous(), dev(coalitions(IDS, 4, 4).view(np.int32)), 4)   # 24 / 4 = 6 pixels per player
    with pytest.raises(ValueError, match="coal must be torch.int32"):
        ops.shap_apply(x, cd.float(), s)
    with pytest.raises(ValueError, match="coal must be"):
        ops.shap_apply(x, cd[:2], s)
    with pytest.raises(ValueError, match="out must be"):
        ops.shap_apply(x, cd, s, 0, 2, out=buf[:3])


# ------------------------------------------------------------------------------------------------ 3. ppf_shap_gram
@pytest.mark.parametrize("s,N,M", [(2, 2, 1), (2, 64, 8), (7, 66, 8), (14, 64, 1), (14, 2050, 1), (7, 2050, 8), (2, 2050, 8)],
                         ids=["d4_N2_M1", "d4_N64_M8", "d49_N66_M8", "d196_N64_M1", "d196_N2050_M1", "d49_N2050_M8", "d4_N2050_M8"])
def test_gram_and_right_hand_sides_equal_the_numpy_loop_bit_for_bit(s, N, M):
    from protopformer_amd.interpret import shap_gram
    rng = np.random.default_rng(s + N + M)
    B, d = 2, s * s
    coal = coalitions(IDS[:B], s, N, seed=5)
    val, v0 = rng.standard_normal((N, B, M)).astype(np.float32), rng.standard_normal((B, M)).astype(np.float32)
    ref_A, ref_b = shap_gram(coal, val, v0, s, device=False)
    A, bvec = shap_gram(dev(coal.view(np.int32)), dev(val), dev(v0), s)
    torch.cuda.synchronize()
    assert A.dtype == torch.int32 and bvec.dtype == torch.float64 and tuple(A.shape) == (B, d, d) and tuple(bvec.shape) == (B, M, d)
    A, bvec = A.cpu().numpy(), bvec.cpu().numpy()
    assert np.array_equal(A, ref_A), f"A: {int((A != ref_A).sum())} of {A.size} entries differ from Z^T Z"
    assert np.array_equal(bits64(bvec), bits64(ref_b)), f"bvec: {int((bits64(bvec) != bits64(ref_b)).sum())} of {bvec.size} sums differ from the referee"


# ------------------------------------------------------------------------------------------------ 4. ppf_shap_solve
def additive_game(s, N, B, M, seed):
    """An additive game v(z) = v0 + w . z whose values fp32 holds exactly (weights and v0 on a grid of 2^-10): phi = w."""
    from protopformer_amd.interpret import shap_members
    rng = np.random.default_rng(seed)
    coal = coalitions(IDS[:B], s, N, seed=2)
    z = shap_members(coal, s).astype(np.float64)
    w = np.round(rng.standard_normal((B, M, s * s)) * 64) / 1024
    v0 = (np.round(rng.standard_normal((B, M)) * 64) / 1024).astype(np.float32)
    val = (v0.astype(np.float64)[None] + np.einsum("bnd,bmd->nbm", z, w)).astype(np.float32)
    v1 = (v0.astype(np.float64) + w.sum(-1)).astype(np.float32)
    return coal, val, v0, v1, w


@pytest.mark.parametrize("s,N,G", [(2, 16, 16), (4, 64, 16), (7, 512, 196), (14, 2048, 196)], ids=["d4", "d16", "d49", "d196"])
def test_solve_within_the_cholesky_bound_of_the_fp64_referee(s, N, G):
    from protopformer_amd.interpret import shap_gram, shap_solve
    B, M, d = 2, 3, s * s
    coal, val, v0, v1, w = additive_game(s, N, B, M, seed=N)
    rng = np.random.default_rng(d)
    val[:, :, 2] = rng.standard_normal((N, B)).astype(np.float32)                                 # the third class: no additive game, any values
    A, bvec = shap_gram(dev(coal.view(np.int32)), dev(val), dev(v0), s)
    phi, cell, bad = shap_solve(A, bvec, dev(v0), dev(v1), s, G)
    again = shap_solve(A, bvec, dev(v0), dev(v1), s, G)
    torch.cuda.synchronize()
    assert phi.dtype == torch.float64 and cell.dtype == torch.float32 and bad.dtype == torch.int32
    assert tuple(phi.shape) == (B, M, d) and tuple(cell.shape) == (B, M, G) and bad.tolist() == [0] * B
    for a, b in zip((phi, cell, bad), again):
        assert torch.equal(a, b), "two calls must give identical bits"
    A_h, phi, cell = A.cpu().numpy(), phi.cpu().numpy(), cell.cpu().numpy()
    ref_phi, ref_cell, ref_bad = shap_solve(A_h, bvec.cpu().numpy(), v0, v1, s, G, device=False)  # on the device's own A and bvec
    assert not ref_bad.any()
    E = solve_bound(A_h, ref_phi)
    err = np.abs(phi - ref_phi).max(axis=(1, 2))
    delta = v1.astype(np.float64) - v0.astype(np.float64)
    gap = np.abs(phi.sum(-1) - delta).max(axis=1)
    off = np.abs(phi[:, :2] - w[:, :2]).max(axis=(1, 2))
    print(f"d={d} N={N}: max|phi - ref| / E = {(err / E).max():.3e}, |sum phi - delta| / (d E) = {(gap / (d * E)).max():.3e}, "
          f"|phi - w| / E = {(off / E).max():.3e}, E = {E.max():.3e}")
    assert (err <= E).all(), f"phi is off the fp64 referee by {(err / E).max():.3f} bounds"
    assert (gap <= d * E).all(), f"the attributions miss delta by {(gap / (d * E)).max():.3f} bounds"
    assert (off <= E).all(), f"the weights of the additive game are missed by {(off / E).max():.3f} bounds"
    side, r = int(G ** 0.5), int(G ** 0.5) // s
    g = np.arange(G)
    player = (g // side // r) * s + (g % side) // r
    assert np.array_equal(bits(cell), bits((phi[:, :, player] / float(r * r)).astype(np.float32))), "cell must be (float)(phi / r^2) of the returned phi"


def test_solve_marks_a_singular_image_and_a_nan_row_alone():
    from protopformer_amd import ops
    rng = np.random.default_rng(0)
    s, M, G = 2, 2, 16
    val = rng.standard_normal((32, 1, M)).astype(np.float32)
    v0, v1 = np.zeros((2, M), dtype=np.float32), np.ones((2, M), dtype=np.float32)
    few = ops.shap_gram(dev(coalitions(IDS[:1], s, 2).view(np.int32)), dev(val[:2]), dev(v0[:1]), s)      # d = 4 from N = 2: rank 2
    many = ops.shap_gram(dev(coalitions(IDS[1:2], s, 32).view(np.int32)), dev(val), dev(v0[:1]), s)
    A, bvec = torch.cat([few[0], many[0]]), torch.cat([few[1], many[1]])
    phi, cell, bad = ops.shap_solve(A, bvec, dev(v0), dev(v1), s, G)
    assert bad.tolist() == [1, 0]
    assert bool(phi[0].isnan().all()) and bool(cell[0].isnan().all()) and bool(phi[1].isfinite().all()) and bool(cell[1].isfinite().all())
    alone = ops.shap_solve(many[0], many[1], dev(v0[:1]), dev(v1[:1]), s, G)
    assert torch.equal(alone[0][0], phi[1]) and torch.equal(alone[1][0], cell[1]), "the singular neighbour must not change an image's bits"
    # one NaN value: its (image, class) row is NaN, no other
    val2 = np.repeat(val, 2, axis=1)
    val2[7, 1, 1] = np.nan
    coal = dev(coalitions(IDS[:2], s, 32).view(np.int32))
    clean = ops.shap_solve(*ops.shap_gram(coal, dev(np.repeat(val, 2, axis=1)), dev(v0), s), dev(v0), dev(v1), s, G)
    dirty = ops.shap_solve(*ops.shap_gram(coal, dev(val2), dev(v0), s), dev(v0), dev(v1), s, G)
    assert dirty[2].tolist() == [0, 0] and clean[2].tolist() == [0, 0]
    row = torch.zeros((2, M), dtype=torch.bool, device="cuda")
    row[1, 1] = True
    for d_, c_ in zip(dirty[:2], clean[:2]):
        assert bool(d_[row].isnan().all()) and torch.equal(d_[~row], c_[~row])
    inf = dev(v1.copy())
    inf[0, 0] = float("inf")                                                                      # a delta that is not finite
    phi = ops.shap_solve(*ops.shap_gram(coal, dev(np.repeat(val, 2, axis=1)), dev(v0), s), dev(v0), inf, s, G)[0]
    assert bool(phi[0, 0].isnan().all()) and torch.equal(phi[0, 1], clean[0][0, 1]) and torch.equal(phi[1], clean[0][1])
    with pytest.raises(RuntimeError, match="ppf_shap_solve.*do not divide"):
        ops.shap_solve(*many, dev(v0[:1]), dev(v1[:1]), s, 9)


# ------------------------------------------------------------------------------------------------ 5. through the micro models
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


@pytest.fixture(scope="module", params=[("micro_deit.npz", 2, 16), ("micro_deit.npz", 4, 64), ("micro_cait.npz", 2, 16), ("micro_cait.npz", 4, 64)],
                ids=["deit_s2", "deit_s4", "cait_s2", "cait_s4"])
def model_case(request):
    """One model, one kernel_shap call, its host copy and the referee pipeline's logits, shared by the tests below and left unchanged."""
    from protopformer_amd.interpret import kernel_shap, shap_apply
    name, s, N = request.param
    sd, cfg, z = micro(name)
    m = build_micro(cfg, sd).eval()
    x = dev(z["img"])
    B = x.shape[0]
    kw = dict(top_classes=2, samples=N, cells=s, batch_size=B)
    r = kernel_shap(m, x, **kw)
    ref_coal = coalitions(np.arange(B), s, N)
    imgs = shap_apply(z["img"], ref_coal, s, device=False)                                        # [N, B, 3, H, W]: a sub-batch is one sample
    ref_logits = forward_logits(m, imgs.reshape((-1,) + imgs.shape[2:]), B)
    end_logits = forward_logits(m, np.concatenate([z["img"], np.zeros_like(z["img"])]), B)
    return dict(name=f"{name} s={s}", m=m, x=x, img=z["img"], r=r, h=r.cpu(), s=s, N=N, kw=kw, ref_coal=ref_coal, ref_logits=ref_logits,
                end_logits=end_logits)


def test_kernel_shap_equals_the_referee_pipeline(model_case):
    from protopformer_amd.interpret import shap_gram, shap_solve
    img, h, name, s, N = model_case["img"], model_case["h"], model_case["name"], model_case["s"], model_case["N"]
    B, M, G, d = img.shape[0], 2, 16, s * s
    assert h.phi.shape == (B, M, d) and h.cell.shape == (B, M, G) and h.value.shape == (N, B, M) and h.classes.shape == (B, M)
    assert h.value_base.shape == h.value_full.shape == (B, M) and h.gram.shape == (B, d, d) and h.bvec.shape == (B, M, d) and h.bad.tolist() == [0] * B
    assert (h.cells, h.kind) == (s, "prob")
    assert np.array_equal(words(h.coal), model_case["ref_coal"]), f"{name}: the coalitions differ from the referee"
    assert (h.classes >= 0).all() and np.array_equal(h.classes[:, 0], model_case["end_logits"][:B].argmax(1))
    worst = 0.0
    for k in range(M):
        for got, logits, reps in ((h.value[:, :, k], model_case["ref_logits"], N), (np.stack([h.value_full[:, k], h.value_base[:, k]]),
                                                                                   model_case["end_logits"], 2)):
            ref, bound = prob_reference(logits, np.tile(h.classes[:, k], reps))
            rel = np.abs(got.reshape(-1).astype(np.float64) - ref) / ref
            worst = max(worst, float((rel / bound).max()))
            assert (rel <= bound).all(), f"{name} class column {k}: off the referee pipeline by {(rel / bound).max():.2f} bounds"
    print(f"{name}: largest probability error / bound = {worst:.3f}")
    A, bvec = shap_gram(model_case["ref_coal"], h.value, h.value_base, s, device=False)
    assert np.array_equal(h.gram, A), f"{name}: the Gram matrix differs from Z^T Z"
    assert np.array_equal(bits64(h.bvec), bits64(bvec)), f"{name}: the right-hand sides differ from the referee fed the returned values"
    phi, cell, bad = shap_solve(h.gram, h.bvec, h.value_base, h.value_full, s, G, device=False)
    assert not bad.any()
    E = solve_bound(h.gram, phi)
    err, gap = np.abs(h.phi - phi).max(axis=(1, 2)), np.abs(h.delta()).max(axis=1)
    print(f"{name}: max|phi - ref| / E = {(err / E).max():.3e}, |delta()| / (d E) = {(gap / (d * E)).max():.3e}, E = {E.max():.3e}")
    assert (err <= E).all() and (gap <= d * E).all(), f"{name}: phi off by {(err / E).max():.3f} bounds, delta by {(gap / (d * E)).max():.3f}"
    side, r = 4, 4 // s
    g = np.arange(G)
    player = (g // side // r) * s + (g % side) // r
    assert np.array_equal(bits(h.cell), bits((h.phi[:, :, player] / float(r * r)).astype(np.float32)))
    assert np.isfinite(h.phi).all() and h.phi.std() > 0


def test_kernel_shap_repeats_and_does_not_depend_on_the_chunk_or_the_mode(model_case):
    from protopformer_amd.interpret import Shap, kernel_shap
    m, x, r, kw, s, N = model_case["m"], model_case["x"], model_case["r"], model_case["kw"], model_case["s"], model_case["N"]
    for what, other in (("a second call", kernel_shap(m, x, **kw)), ("one sample per chunk", kernel_shap(m, x, scratch_bytes=1, **kw))):
        for f in Shap.FIELDS:
            assert torch.equal(getattr(other, f), getattr(r, f)), f"{what}: {f} differs"
    assert not m.training
    m.train()
    try:
        again = kernel_shap(m, x, **kw)
        assert m.training, "the model was found in train mode and must be left in it"
    finally:
        m.eval()
    for f in Shap.FIELDS:                                                                         # eval-mode forwards either way
        assert torch.equal(getattr(again, f), getattr(r, f)), f"train mode: {f} differs"
    # an image's coalitions, and with them its Gram matrix, depend on its id, not on its place: the first two images alone, reversed
    part = kernel_shap(m, x[:2].flip(0), classes=r.classes[:2].flip(0), image_ids=[1, 0], samples=N, cells=s, batch_size=2)
    assert torch.equal(part.coal, r.coal[:2].flip(0)) and torch.equal(part.gram, r.gram[:2].flip(0)) and torch.equal(part.classes, r.classes[:2].flip(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernel_shap(m, x.cpu(), **kw)
    with pytest.raises(ValueError, match="below 4 \\* cells\\^2"):
        kernel_shap(m, x, samples=4 * s * s - 2, cells=s)


def test_kernel_shap_of_the_class_logit(model_case):
    from protopformer_amd.interpret import kernel_shap, shap_gram
    m, x, h, s, N, name = model_case["m"], model_case["x"], model_case["h"], model_case["s"], model_case["N"], model_case["name"]
    B = x.shape[0]
    g = kernel_shap(m, x, value="logit", **model_case["kw"]).cpu()
    assert g.kind == "logit"
    assert np.array_equal(g.classes, h.classes) and np.array_equal(g.coal, h.coal)
    for k in range(2):
        cls = g.classes[:, k]
        assert np.array_equal(bits(g.value[:, :, k]), bits(model_case["ref_logits"][np.arange(N * B), np.tile(cls, N)].reshape(N, B))), f"{name}: column {k}"
        assert np.array_equal(bits(g.value_full[:, k]), bits(model_case["end_logits"][np.arange(B), cls]))
        assert np.array_equal(bits(g.value_base[:, k]), bits(model_case["end_logits"][B + np.arange(B), cls]))
    A, bvec = shap_gram(model_case["ref_coal"], g.value, g.value_base, s, device=False)
    assert np.array_equal(g.gram, A) and np.array_equal(bits64(g.bvec), bits64(bvec)) and g.bad.tolist() == [0] * B


def order_of_scores(score):
    """The contract's sort of given scores [G]: NaN last, score descending, smaller cell."""
    nan = np.isnan(score)
    return np.lexsort((np.arange(score.size), np.where(nan, np.float32(0), -score), nan))


def test_the_shap_order_of_the_faithfulness_curves(model_case):
    from protopformer_amd.interpret import default_counts, faithfulness_curves
    m, x, img, h, name, s, N = (model_case[k] for k in ("m", "x", "img", "h", "name", "s", "N"))
    B, M, G = img.shape[0], 2, 16
    f = faithfulness_curves(m, x, top_classes=M, batch_size=B, order="shap", shap=dict(samples=N, cells=s))
    assert f.shap is not None and f.rise is None and f.ig is None and torch.equal(f.score, f.shap.cell), "score must be Shap.cell, bit for bit"
    g = f.cpu()
    assert np.array_equal(bits(g.score), bits(g.shap.cell)) and np.array_equal(bits(g.shap.cell), bits(h.cell)), f"{name}: not the cells of kernel_shap"
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
    other = faithfulness_curves(m, x, top_classes=M, batch_size=B)                               # the default order is untouched and carries no Shap
    assert other.shap is None and other.rise is None and not torch.equal(other.score, f.score)
    with pytest.raises(ValueError, match="'shap' order is defined at resolution='cell' only"):
        faithfulness_curves(m, x, top_classes=M, batch_size=B, order="shap", resolution="pixel", shap=dict(samples=N, cells=s))


# ------------------------------------------------------------------------------------------------ 6. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def test_tool_with_the_shap_order_on_the_miniature_cub_tree(tmp_path):
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
                                              "--max_images", "6", "--orders", "evidence", "random", "shap", "--shap_samples", "16", "--shap_cells", "2",
                                              *MODEL_FLAGS])
    doc = json.load(open(tool.main(args)))
    assert doc["images"] == 6 and doc["counts"] == [0, 49, 98, 147, 196] and doc["grid_cells"] == 196
    assert list(doc["orders"]) == ["evidence", "random", "shap"] and all(set(v) == {"deletion", "insertion"} for v in doc["orders"].values())
    assert set(doc["vs_random"]) == {"evidence", "shap"}
    for v in doc["vs_random"].values():
        assert set(v) == {"deletion_auc_minus_random", "insertion_auc_minus_random", "informative"}
    shap, ev = doc["orders"]["shap"], doc["orders"]["evidence"]
    for mode in ("deletion", "insertion"):
        assert len(shap[mode]["curve"]) == 5 and 0.0 <= shap[mode]["auc"] <= 1.0
    # the ends do not depend on the order: nothing removed / everything removed (fp32 probabilities of the same images; the bound of
    # ppf_class_prob at C = 200 with logits within 16 of their maximum is below 2e-5 relative)
    for a, b in ((shap["deletion"]["curve"][0], ev["deletion"]["curve"][0]), (shap["insertion"]["curve"][-1], ev["insertion"]["curve"][-1]),
                 (shap["deletion"]["curve"][-1], ev["deletion"]["curve"][-1]), (shap["insertion"]["curve"][0], ev["insertion"]["curve"][0])):
        assert abs(a - b) <= 4e-5 * abs(b), (a, b)
    assert not os.path.exists(os.path.join(out, "faithfulness.npz"))
