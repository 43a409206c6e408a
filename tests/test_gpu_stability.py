"""The stability score on the GPU: ppf_add_gauss_noise against a numpy Philox4x32-10 + fp64 Box-Muller written from the definition
in include/ppf_hip.h, ppf_part_meter_update / interpret.PartMeter against the host reductions of interpret.py (the referee, called
here), and interpret.interpretability_scores through a stand-in model and through the micro DeiT PPNet on a miniature CUB tree.
Everything but the noise values is compared exactly.  Host references are computed once and shared."""
import functools
import types

import numpy as np
import pytest
import torch

from protopformer_amd import interpret as I

pytestmark = pytest.mark.gpu

MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ the host model of the noise
def philox4x32_10(c, k):
    """Philox4x32-10 (Salmon et al. 2011) on arrays: c = four and k = two uint64 arrays holding 32-bit words -> four such arrays."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in c)
    k0, k1 = (np.asarray(v, dtype=np.uint64) for v in k)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2                     # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return c0, c1, c2, c3


def model_noise(seed, image_id, n_per_img):
    """The n_per_img standard normals of one image in fp64: key = seed, counter = (e/4 low, e/4 high, id low, id high), two Box-Muller
    pairs per call, uniforms on the 24-bit grid."""
    q = np.arange((n_per_img + 3) // 4, dtype=np.uint64)
    one = np.ones_like(q)
    r = philox4x32_10((q & MASK, q >> np.uint64(32), one * np.uint64(image_id & 0xFFFFFFFF), one * np.uint64((image_id >> 32) & 0xFFFFFFFF)),
                      (one * np.uint64(seed & 0xFFFFFFFF), one * np.uint64((seed >> 32) & 0xFFFFFFFF)))
    r = [(v >> np.uint64(8)).astype(np.float64) for v in r]
    u0, u1, u2, u3 = (r[0] + 0.5) / 2 ** 24, r[1] / 2 ** 24, (r[2] + 0.5) / 2 ** 24, r[3] / 2 ** 24
    m0, m1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    n = np.stack([m0 * np.cos(2 * np.pi * u1), m0 * np.sin(2 * np.pi * u1), m1 * np.cos(2 * np.pi * u3), m1 * np.sin(2 * np.pi * u3)], axis=1)
    return n.reshape(-1)[:n_per_img]


def test_host_philox_known_answers():
    """The model itself against the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)."""
    def one(c, k):
        return [int(v[0]) for v in philox4x32_10([[w] for w in c], [[w] for w in k])]
    assert one((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert one((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert one((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def bits(t):
    return t.contiguous().view(torch.int32)


def offset_batch(shape, offset, fill=None):
    """A contiguous fp32 CUDA tensor of `shape` whose first element lies `offset` floats into its allocation (offset 1: 4-byte but not
    16-byte aligned)."""
    n = int(np.prod(shape))
    base = torch.zeros(n + offset, dtype=torch.float32, device="cuda")
    t = base[offset:].view(shape)
    if fill is not None:
        t.copy_(fill)
    assert t.is_contiguous() and (t.data_ptr() % 16 == 0) == (offset % 4 == 0)
    return t


# ------------------------------------------------------------------------------------------------ 1. noise against the model
@pytest.mark.parametrize("shape,offset", [((3, 3, 8, 8), 0), ((3, 3, 5, 5), 0), ((3, 3, 5, 5), 1), ((3, 3, 8, 8), 1)],
                         ids=["192-vector", "75-tail", "75-unaligned", "192-unaligned"])
def test_noise_matches_the_host_model(shape, offset):
    """Bound 1e-5: |m| <= sqrt(50 ln 2) ~ 5.9, logf / sincospif / sqrtf are good to a few ulp each, so the error stays below 1e-6; the
    bound carries a 10x margin.  A fast-intrinsic logarithm misses it near u0 -> 1."""
    from protopformer_amd import ops
    id_list, seed = [5, 2 ** 33 + 1, 5], 1234
    n_per = int(np.prod(shape[1:]))
    ids = torch.tensor(id_list, dtype=torch.int64, device="cuda")
    zero = offset_batch(shape, offset)
    out = ops.add_gauss_noise(zero, ids, 1.0, seed)
    assert out.shape == zero.shape and out.dtype == torch.float32 and float(zero.abs().max()) == 0.0
    got = out.cpu().numpy().reshape(3, n_per)
    model = np.stack([model_noise(seed, i, n_per) for i in id_list])
    err = np.abs(got.astype(np.float64) - model).max()
    print(f"shape {shape} offset {offset}: max |kernel - fp64 model| = {err:.3e}, max |n| = {np.abs(model).max():.3f}")
    assert err <= 1e-5
    assert np.array_equal(got[0].view(np.int32), got[2].view(np.int32))                    # the same id: the same noise, wherever it sits
    low = ops.add_gauss_noise(zero, torch.tensor([5, 1, 5], dtype=torch.int64, device="cuda"), 1.0, seed).cpu().numpy().reshape(3, n_per)
    assert not np.array_equal(got[1], low[1]) and np.array_equal(got[0], low[0])            # the high word of the id is used
    # x + sigma * n: one fused multiply-add, within one ulp of the fp64 value
    xh = np.random.default_rng(7).standard_normal(shape).astype(np.float32)
    x = offset_batch(shape, offset, torch.from_numpy(xh).cuda())
    noisy = ops.add_gauss_noise(x, ids, 0.2, seed)
    ref = xh.reshape(3, n_per).astype(np.float64) + np.float64(np.float32(0.2)) * got.astype(np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(noisy.cpu().numpy().reshape(3, n_per).astype(np.float64) - ref) <= ulp).all()
    assert np.array_equal(x.cpu().numpy(), xh)                                              # out of place: x untouched
    same = ops.add_gauss_noise(x, ids, 0.2, seed, out=x)
    assert same.data_ptr() == x.data_ptr() and torch.equal(bits(x), bits(noisy))            # in place: the same bits


# ------------------------------------------------------------------------------------------------ 2. independence of batching
def test_noise_does_not_depend_on_batching():
    id_list = [3, 17, 2 ** 40, 0, 99, 100, 101, 7, 2 ** 31, 12345, 6, 2 ** 32]
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((12, 3, 8, 8)).astype(np.float32)).cuda()
    ids = torch.tensor(id_list, dtype=torch.int64, device="cuda")
    whole = I.add_input_noise(x, ids, std=0.2, seed=9)
    perm = torch.tensor([4, 11, 0, 7, 2, 9, 5, 1, 10, 3, 8, 6], device="cuda")
    split = torch.empty_like(whole)
    for sel in (perm[:5], perm[5:]):
        split[sel] = I.add_input_noise(x[sel].contiguous(), ids[sel].contiguous(), std=0.2, seed=9)
    assert torch.equal(bits(whole), bits(split))
    assert torch.equal(bits(whole), bits(I.add_input_noise(x, id_list, std=0.2, seed=9)))  # a second call; ids from a host list
    other = I.add_input_noise(x, ids, std=0.2, seed=10)
    assert bool((bits(other) != bits(whole)).reshape(12, -1).any(dim=1).all())              # another seed changes every row
    # more images than the launch has workgroup rows (2048): the kernel strides over them, differently in the whole and in the halves
    many = torch.arange(5000, 7100, device="cuda")
    z = torch.zeros((2100, 10), device="cuda")
    big = I.add_input_noise(z, many, std=1.0, seed=9)
    halves = torch.cat([I.add_input_noise(z[:1050], many[:1050], std=1.0, seed=9), I.add_input_noise(z[1050:], many[1050:], std=1.0, seed=9)])
    assert torch.equal(bits(big), bits(halves))
    assert np.abs(big[2099].cpu().numpy().astype(np.float64) - model_noise(9, 7099, 10)).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ 3. moments
def test_noise_moments():
    """64 x 3 x 32 x 32 = 196 608 draws: mean, standard deviation and lag-1 correlation along the element index within five standard
    errors (1 / sqrt(n), 1 / sqrt(2 n), 1 / sqrt(n))."""
    from protopformer_amd import ops
    x = torch.zeros((64, 3, 32, 32), device="cuda")
    v = ops.add_gauss_noise(x, torch.arange(1000, 1064, device="cuda"), 1.0, 77).cpu().numpy().astype(np.float64).reshape(64, -1)
    n = v.size
    assert n == 196608 and np.isfinite(v).all()
    mean, std = v.mean(), v.std()
    lag1 = ((v[:, :-1] - mean) * (v[:, 1:] - mean)).mean() / v.var()
    print(f"mean {mean:.3e} (bound {5 / np.sqrt(n):.3e}), std - 1 {std - 1:.3e} (bound {5 / np.sqrt(2 * n):.3e}), lag-1 {lag1:.3e}")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(std - 1) <= 5 / np.sqrt(2 * n) and abs(lag1) <= 5 / np.sqrt(n)


# ------------------------------------------------------------------------------------------------ 4. / 5. the meter
def activation_like(shape, seed):
    d = np.random.default_rng(seed).random(shape, dtype=np.float32) * 4.0
    return np.log((d + 1) / (d + np.float32(1e-4))).astype(np.float32)


NOISE_AMPLITUDE = 1.2        # chosen on the CPU: the host referee alone finds 49 % of the (image, prototype) rows unchanged at this amplitude


def random_eval(B=64, ppc=10, k=81, n=196, classes=9, seed=3):
    """test_gpu_interp_device.random_eval with a noisy second pass: 9 classes of which class 4 has no image, image 0 without a visible
    part; the noisy pass perturbs the activations (and, slightly, the rollout scores: it is expanded by its own reserved tokens)."""
    rng = np.random.default_rng(seed)
    s = int(round(k ** 0.5))
    attn = rng.random((B, n), dtype=np.float32)
    acts = activation_like((B, ppc, s, s), seed + 1)
    targets = rng.integers(0, classes - 1, B)
    targets[targets >= 4] += 1
    ids = np.arange(100, 100 + B)
    sizes = {int(i): (int(rng.integers(200, 500)), int(rng.integers(150, 400))) for i in ids}
    locs = {}
    for i in ids:
        w, h = sizes[int(i)]
        locs[int(i)] = [[p, float(rng.random() * (w - 1)), float(rng.random() * (h - 1))] for p in range(1, 16) if rng.random() < 0.7]
    locs[int(ids[0])] = []
    acts_noisy = (acts + NOISE_AMPLITUDE * rng.standard_normal(acts.shape)).astype(np.float32)
    attn_noisy = (attn + 0.002 * rng.standard_normal(attn.shape)).astype(np.float32)
    return attn, acts, attn_noisy, acts_noisy, targets, ids, types.SimpleNamespace(id_to_part_loc=locs), sizes, k, classes


@functools.lru_cache(maxsize=None)
def meter_case():
    """The inputs and what the host referees make of them; computed once, read-only."""
    attn, acts, attn_noisy, acts_noisy, targets, ids, parts, sizes, k, classes = case = random_eval()
    cons = I.consistency_from_outputs(attn, acts, targets, ids, parts, sizes, k, 224, num_classes=classes)[:3]
    stab = I.stability_from_outputs(attn, acts, attn_noisy, acts_noisy, targets, ids, parts, sizes, k, 224, num_classes=classes)
    return case, cons, stab


def device_tables(case):
    attn, acts, attn_noisy, acts_noisy, targets, ids, parts, sizes, k, classes = case
    plist = torch.from_numpy(I._part_list(ids, parts, sizes, 224, 15)[0]).cuda()
    dev = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    clean = I._tables_for_parts(I._grid_on_device(dev(attn), dev(acts), k), plist, 224, 36)
    noisy = I._tables_for_parts(I._grid_on_device(dev(attn_noisy), dev(acts_noisy), k), plist, 224, 36)
    return clean, noisy, plist, torch.from_numpy(targets.astype(np.int64)).cuda()


def test_meter_equals_the_host_reductions():
    case, cons, stab = meter_case()
    targets, classes = case[4], case[9]
    counts = np.bincount(targets, minlength=classes)
    assert counts[4] == 0 and (np.delete(counts, 4) > 0).all() and len(stab[1]) == 8 * 10
    # not vacuous: on the HOST values, the share of (image, prototype) rows the noise left unchanged
    share = float(np.sum(np.asarray(stab[1]).reshape(8, 10) * np.delete(counts, 4)[:, None]) / (64 * 10))
    print(f"host: stable share {share:.3f}, stability {stab[0]:.4f}, consistency {cons[0]:.4f}")
    assert 0.1 <= share <= 0.9
    clean, noisy, plist, labels = device_tables(case)
    meter = I.PartMeter(classes, 10, 15, "cuda")
    meter.update(clean, plist, labels, noisy)
    r = meter.result()
    assert (r["consistency"], r["effects"], r["max_parts"]) == cons
    assert (r["stability"], r["stable_fraction"]) == stab
    assert r["images"] == counts.tolist()
    attn, acts, attn_noisy, acts_noisy, targets, ids, parts, sizes, k, classes = case
    assert I.stability_from_outputs(attn, acts, attn_noisy, acts_noisy, targets, ids, parts, sizes, k, 224, num_classes=classes, device=True) == stab
    # a label of C: counted in `bad`, nothing else touched, result() raises
    before = meter.buf.clone()
    wrong = labels[:3].clone(); wrong[1] = classes
    lone = I.PartMeter(classes, 10, 15, "cuda")
    lone.update(clean[:3].contiguous(), plist[:3].contiguous(), wrong, noisy[:3].contiguous())
    assert int(lone.bad) == 1 and int(lone.images.sum()) == 2
    with pytest.raises(ValueError, match=r"1 labels lie outside \[0, 9\)"):
        lone.result()
    assert torch.equal(meter.buf, before)


def test_meter_does_not_depend_on_batching():
    case, cons, _ = meter_case()
    clean, noisy, plist, labels = device_tables(case)
    whole = I.PartMeter(9, 10, 15, "cuda")
    whole.update(clean, plist, labels, noisy)
    eights, shuffled, plain = I.PartMeter(9, 10, 15, "cuda"), I.PartMeter(9, 10, 15, "cuda"), I.PartMeter(9, 10, 15, "cuda")
    perm = torch.from_numpy(np.random.default_rng(0).permutation(64)).cuda()
    for b in range(0, 64, 8):
        eights.update(clean[b:b + 8].contiguous(), plist[b:b + 8].contiguous(), labels[b:b + 8].contiguous(), noisy[b:b + 8].contiguous())
        sel = perm[b:b + 8]
        plain.update(clean[sel].contiguous(), plist[sel].contiguous(), labels[sel].contiguous())
    shuffled.update(clean[perm].contiguous(), plist[perm].contiguous(), labels[perm].contiguous(), noisy[perm].contiguous())
    assert torch.equal(whole.buf, eights.buf) and torch.equal(whole.buf, shuffled.buf)
    r = plain.result()
    assert r["stability"] is None and r["stable_fraction"] is None and (r["consistency"], r["effects"], r["max_parts"]) == cons
    with pytest.raises(ValueError, match="every update or with none"):
        plain.update(clean, plist, labels, noisy)
    whole.reset()
    assert int(whole.buf.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ 6. through a loader, stand-in model
CONTRAST = 1.0               # chosen on the CPU (numpy model of the noise): 58 % of the (image, prototype) rows survive std 0.2


class StandIn:
    """push_forward as a deterministic, batch-size independent torch function of x (B, 3, 28, 28): rollout scores = channel 0 pooled to
    the 7 x 7 patch grid, activations of the 16 reserved tokens = the three channels pooled to 4 x 4 and mixed with fixed per-prototype
    weights, element by element (no GEMM: its summation order could depend on the batch size)."""
    num_prototypes_per_class, reserve_token_nums, img_size = 3, [16], 56

    def __init__(self, classes, device):
        w = np.random.default_rng(5).standard_normal((classes * 3, 3)).astype(np.float32)
        self.w = torch.from_numpy(w).to(device)

    def eval(self):
        return self

    def push_forward(self, x):
        pooled = torch.nn.functional.avg_pool2d(x, 7)                                        # (B, 3, 4, 4)
        w = self.w[None, :, :, None, None]
        acts = w[:, :, 0] * pooled[:, None, 0] + w[:, :, 1] * pooled[:, None, 1] + w[:, :, 2] * pooled[:, None, 2]
        return torch.nn.functional.avg_pool2d(x[:, 0], 4).reshape(x.shape[0], -1), acts


def standin_case(classes=4, B=24, seed=21):
    rng = np.random.default_rng(seed)
    x = (CONTRAST * rng.standard_normal((B, 3, 28, 28))).astype(np.float32)
    targets = np.arange(B) % classes
    ids = rng.permutation(np.arange(1000, 1000 + B))
    sizes = {int(i): (int(rng.integers(100, 300)), int(rng.integers(80, 200))) for i in ids}
    locs = {}
    for i in ids:
        w, h = sizes[int(i)]
        locs[int(i)] = [[p, float(rng.random() * (w - 1)), float(rng.random() * (h - 1))] for p in range(1, 16) if rng.random() < 0.7]
    return x, targets, ids, types.SimpleNamespace(id_to_part_loc=locs), sizes, classes


def loader_of(x, targets, ids, batch):
    return [(torch.from_numpy(x[b:b + batch]).cuda(), torch.from_numpy(targets[b:b + batch]), torch.from_numpy(ids[b:b + batch]))
            for b in range(0, len(ids), batch)]


def test_interpretability_scores_through_a_loader():
    x, targets, ids, parts, sizes, classes = standin_case()
    net = StandIn(classes, "cuda")
    kw = dict(num_classes=classes, half_size=12, noise_std=0.2, seed=3)
    host = I.interpretability_scores(net, loader_of(x, targets, ids, 8), parts, sizes, device=False, **kw)
    assert sorted(host) == ["consistency", "effects", "max_parts", "stability", "stable_fraction"]
    share = float(np.sum(np.asarray(host["stable_fraction"]).reshape(classes, 3) * np.bincount(targets, minlength=classes)[:, None]) / (24 * 3))
    print(f"host: stable share {share:.3f}, stability {host['stability']:.4f}, consistency {host['consistency']:.4f}")
    assert 0.1 <= share <= 0.9
    dev8 = I.interpretability_scores(net, loader_of(x, targets, ids, 8), parts, sizes, device=True, **kw)
    dev24 = I.interpretability_scores(net, loader_of(x, targets, ids, 24), parts, sizes, device=True, **kw)
    assert dev8 == host and dev24 == dev8
    assert host["consistency"] == I.consistency_score(net, loader_of(x, targets, ids, 8), parts, sizes, num_classes=classes, half_size=12)
    still = I.interpretability_scores(net, loader_of(x, targets, ids, 8), parts, sizes, device=True, **dict(kw, noise_std=0.0))
    assert still["stability"] == 1.0 and still["stable_fraction"] == [1.0] * (classes * 3) and still["effects"] == host["effects"]
    off = I.interpretability_scores(net, loader_of(x, targets, ids, 8), parts, sizes, device=True, stability=False, **kw)
    assert off["stability"] is None and off["stable_fraction"] is None and off["max_parts"] == host["max_parts"]


# ------------------------------------------------------------------------------------------------ 7. the real model
def test_interpretability_scores_of_the_micro_model(tmp_path):
    """The micro DeiT PPNet (64 x 64 inputs, 10 classes x 2 prototypes, 9 of 16 tokens reserved) over the test split of the miniature CUB
    tree, read through Cub2011(return_id=True), DeviceLoader and CubParts."""
    import mini_trees as M
    from helpers import build_micro, micro
    from protopformer_amd import data as D
    meta = M.build_cub(str(tmp_path))
    sd, cfg, _ = micro("micro_deit.npz")
    m = build_micro(cfg, sd).eval()
    ds = D.Cub2011(str(tmp_path), train=False, transform=D.build_view_transform(types.SimpleNamespace(input_size=64), square=True), return_id=True)
    assert len(ds) == 12
    loader = D.DeviceLoader(ds, 5, torch.device("cuda"), D.GpuFinisher(re_prob=0.0), num_workers=0)
    parts = I.CubParts(meta)
    sizes = {i: M.cub_size(i) for i, _, _ in M.CUB_ROWS}
    kw = dict(num_classes=10, half_size=10, noise_std=0.2, seed=1)
    dev = I.interpretability_scores(m, loader, parts, sizes, device=True, **kw)
    host = I.interpretability_scores(m, loader, parts, sizes, device=False, **kw)
    again = I.interpretability_scores(m, loader, parts, sizes, device=True, **kw)
    print(f"micro model: consistency {dev['consistency']:.4f}, stability {dev['stability']:.4f}")
    assert dev == host and again == dev
    assert len(dev["effects"]) == len(dev["stable_fraction"]) == 4 * 2 and 0.0 <= dev["stability"] <= 1.0


# ------------------------------------------------------------------------------------------------ 8. bad inputs
def test_bad_inputs_are_refused_before_anything_is_launched():
    from protopformer_amd import ops
    x = torch.zeros((2, 3, 4, 8), device="cuda")
    ids = torch.tensor([1, 2], device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        ops.add_gauss_noise(x[:, :, :, ::2], ids, 0.2, 0)
    with pytest.raises(ValueError, match="int64"):
        ops.add_gauss_noise(x, ids.int(), 0.2, 0)
    with pytest.raises(ValueError, match="int64"):
        ops.add_gauss_noise(x, ids.cpu(), 0.2, 0)
    for sigma in (float("nan"), float("inf"), -0.5):
        with pytest.raises(RuntimeError, match=r"rc=-1.*sigma"):
            ops.add_gauss_noise(x, ids, sigma, 0)
    with pytest.raises(RuntimeError, match=r"rc=-1.*B=0"):
        ops.add_gauss_noise(x[:0], ids[:0], 0.2, 0)
    with pytest.raises(RuntimeError, match=r"rc=-1.*n_per_img=0"):
        ops.add_gauss_noise(torch.zeros((2, 0), device="cuda"), ids, 0.2, 0)
    meter = I.PartMeter(4, 2, 15, "cuda")
    tables = torch.zeros((3, 2, 15), dtype=torch.uint8, device="cuda")
    plist = torch.zeros((3, 15, 3), dtype=torch.int32, device="cuda")
    labels = torch.zeros(3, dtype=torch.int64, device="cuda")
    for bad in ((tables.int(), plist, labels), (tables, plist[:2], labels), (tables, plist, labels.int()), (tables[:, :, ::3], plist, labels),
                (tables, plist, labels, tables[:2])):
        with pytest.raises(ValueError, match="part_meter_update"):
            meter.update(*bad)
    torch.cuda.synchronize()
    assert int(meter.buf.abs().sum()) == 0 and float(x.abs().max()) == 0.0
