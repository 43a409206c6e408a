"""Part interventions on the GPU: ppf_synth_edit against the numpy referee bit for bit, ppf_part_mass against math.fsum within the
any-order fp64 bound on both load paths, data.partsworld_view against the eval loader, part_interventions against the referee pipeline
(numpy edit, numpy render, the CPU loader's square transform, the same model), part_attribution against the part_mass referee, and the
partcheck tool end to end on the 12-image world.

Bound of ppf_part_mass: a bin is a sum of n non-negative fp64 terms, each exact (an fp32 score widened); any summation order is within
(n - 1) * 2^-53 * sum |s| of the exact sum to first order, and math.fsum is the exactly rounded sum, one more 2^-53: n * 2^-53 * sum |s|,
the bound ppf_grad_box_mass is held to."""
import json
import math
import os

import numpy as np
import pytest
import torch

from protopformer_amd import data as D
from protopformer_amd import interpret as I
from protopformer_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORLD = dict(classes=4, parts=4, distractors=3, n_train=32, n_test=12, seed=5, noise=8, grid=4)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _world_spec():
    return D.PartsWorldSpec(height=80, width=96, **WORLD)


def _micro_model():
    """The micro DeiT of tests/helpers.py (64 x 64 inputs, 10 classes: the 4 of the world are its first 4)."""
    from helpers import build_micro, micro
    sd, cfg, _ = micro("micro_deit.npz")
    return build_micro(cfg, sd)


def _args(spec, **kw):
    import types
    return types.SimpleNamespace(input_size=64, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="PartsWorld", data_path="", batch_size=4,
                                 num_workers=0, reprob=0.25, partsworld=spec, **kw)


# ------------------------------------------------------------------------------------------------ ppf_synth_edit
def _edit_pool(K, Dn):
    valid = [(D.EDIT_COPY, 0), (D.EDIT_PARTS_OFF, 1), (D.EDIT_PARTS_OFF, (1 << K) - 1), (D.EDIT_DISTRACTORS_OFF, (1 << Dn) - 1), (D.EDIT_DISTRACTORS_OFF, 0),
             (D.EDIT_BACKGROUND, 0x808080), (D.EDIT_BACKGROUND, 0xFFFFFF), (D.EDIT_PART_ATTR, (K - 1) | 23 << 8), (D.EDIT_PART_ATTR, 0 | 5 << 8)]
    invalid = [(5, 0), (-1, 1), (D.EDIT_PARTS_OFF, 1 << K), (D.EDIT_DISTRACTORS_OFF, 1 << Dn), (D.EDIT_PART_ATTR, K | 1 << 8), (D.EDIT_PART_ATTR, 0 | 24 << 8),
               (D.EDIT_BACKGROUND, 0x1000000), (D.EDIT_PARTS_OFF, -1)]
    return valid + invalid


@pytest.mark.parametrize("K,Dn", [(1, 0), (8, 8)])
@pytest.mark.parametrize("E", [1, 11])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_edit_kernel_equals_referee(B, E, K, Dn):
    spec = D.PartsWorldSpec(height=48, width=48, classes=20, parts=K, distractors=Dn, n_train=64, n_test=8, seed=3, noise=8, grid=3)
    ids = np.arange(B, dtype=np.int64) * 3 + 1
    scene = D.partsworld_scene_from_ids(spec, ids)
    pool = _edit_pool(K, Dn)
    edits = np.array([[pool[(b * E + e + B) % len(pool)] for e in range(E)] for b in range(B)], dtype=np.int32)
    if B * E >= len(pool):
        assert {tuple(e) for e in edits.reshape(-1, 2).tolist()} == set(pool)  # every op and every invalid kind is in the table
    want_out, want_changed = D.partsworld_edit(spec, scene, edits)
    out, changed = D.partsworld_edit(spec, _dev(scene), _dev(edits), device=True, check=False)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (B, E, D.SYNTH_WORDS) and changed.dtype == torch.int32
    assert np.array_equal(out.cpu().numpy(), want_out) and np.array_equal(changed.cpu().numpy(), want_changed)
    if (want_changed < 0).any():
        with pytest.raises(ValueError, match="invalid edits"):
            ops.synth_edit(spec, _dev(scene), _dev(edits))


def test_edit_kernel_leaves_the_guards_alone():
    spec = D.PartsWorldSpec(height=48, width=48, classes=20, parts=8, distractors=8, n_train=64, n_test=8, seed=3, noise=8, grid=3)
    ids = np.arange(5, dtype=np.int64)
    scene = D.partsworld_scene_from_ids(spec, ids)
    pool = _edit_pool(8, 8)
    edits = np.array([[pool[(3 * b + e) % 9] for e in range(4)] for b in range(5)], dtype=np.int32)      # valid ones
    n, guard = 5 * 4 * D.SYNTH_WORDS, 64
    buf = torch.full((guard + n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out, changed = ops.synth_edit(spec, _dev(scene), _dev(edits), out=buf[guard:guard + n])
    assert out.data_ptr() == buf.data_ptr() + 4 * guard
    want_out, want_changed = D.partsworld_edit(spec, scene, edits)
    assert np.array_equal(buf[guard:guard + n].cpu().numpy(), want_out.reshape(-1)) and np.array_equal(changed.cpu().numpy(), want_changed)
    assert bool((buf[:guard] == 0x5A5A5A5A).all()) and bool((buf[guard + n:] == 0x5A5A5A5A).all())
    with pytest.raises(ValueError, match="edits must be"):
        ops.synth_edit(spec, _dev(scene), _dev(edits[:4]))
    with pytest.raises(RuntimeError, match="E=0"):
        ops.synth_edit(spec, _dev(scene), _dev(edits[:, :0]))


# ------------------------------------------------------------------------------------------------ ppf_part_mass
def _mass_case(S, H, W, R, rpi, K, seed):
    rng = np.random.default_rng(seed)
    score = (rng.standard_normal((R, S, S)) * np.exp(rng.uniform(-6, 6, (R, S, S)))).astype(np.float32)
    flat = score.reshape(-1)
    if flat.size >= 8:
        at = rng.choice(flat.size, size=4, replace=False)
        flat[at] = [np.nan, np.inf, -np.inf, -0.0]
    pm = rng.integers(0, 3 + K, (R // rpi, H, W)).astype(np.uint8)
    pm[0, H // 2, W // 3] = 200                                               # a code above 2 + K: counted in nonfinite when a view pixel lands on it
    return score, pm


def _check_mass(score_dev, score, pm, rpi, K):
    R, S = score.shape[:2]
    pos, neg, count, bad = ops.part_mass(score_dev, _dev(pm), rpi, K)
    again = ops.part_mass(score_dev, _dev(pm), rpi, K)
    for a, b in zip((pos, neg, count, bad), again):
        assert torch.equal(a, b)                                               # a fixed order: bit-identical from run to run
    assert pos.dtype == torch.float64 and count.dtype == torch.int32 and tuple(pos.shape) == (R, 3 + K) and tuple(bad.shape) == (R,)
    pos, neg, count, bad = (t.cpu().numpy() for t in (pos, neg, count, bad))
    view = D.partsworld_view_partmap(pm, S)
    worst = 0.0
    for r in range(R):
        code, s = view[r // rpi].reshape(-1), score[r].reshape(-1)
        fin = np.isfinite(s)
        assert bad[r] == int((~fin | (code >= 3 + K)).sum())
        for c in range(3 + K):
            v = [float(x) for x in s[(code == c) & fin]]
            n = int((code == c).sum())
            assert count[r, c] == n
            bound = n * 2.0 ** -53 * math.fsum(abs(x) for x in v)
            dp, dn = abs(pos[r, c] - math.fsum(x for x in v if x > 0)), abs(neg[r, c] - math.fsum(-x for x in v if x < 0))
            assert dp <= bound and dn <= bound, (r, c, dp, dn, bound)
            worst = max(worst, (max(dp, dn) / bound) if bound else 0.0)
    rp, rn, rc, rb = I.part_mass(score, pm, rpi, K, device=False)
    assert np.array_equal(rc, count) and np.array_equal(rb, bad)
    print(f"S={S} R={R} K={K}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("S,H,W,R,rpi,K", [(1, 32, 32, 1, 1, 4), (7, 37, 48, 6, 3, 1), (64, 80, 96, 10, 2, 4), (224, 256, 256, 2, 1, 8), (64, 80, 96, 2, 1, 8)])
def test_part_mass_against_fsum(S, H, W, R, rpi, K):
    score, pm = _mass_case(S, H, W, R, rpi, K, seed=S + K)
    _check_mass(_dev(score), score, pm, rpi, K)


def test_part_mass_unaligned_view_takes_the_scalar_path():
    score, pm = _mass_case(8, 32, 48, 3, 1, 4, seed=2)
    buf = torch.zeros(score.size + 4, dtype=torch.float32, device=DEV)
    for shift in (1, 3):                                                       # S % 4 == 0, the pointer 4 and 12 bytes off a 16-byte boundary
        view = buf[shift:shift + score.size].view(3, 8, 8)
        view.copy_(_dev(score))
        assert view.data_ptr() % 16 != 0
        _check_mass(view, score, pm, 1, 4)


def test_part_mass_all_nan_row_and_refusals():
    S, K = 12, 4
    score = torch.full((2, S, S), float("nan"), device=DEV)
    score[1] = 1.0
    pm = torch.zeros((2, 16, 16), dtype=torch.uint8, device=DEV)
    pos, neg, count, bad = ops.part_mass(score, pm, 1, K)
    assert not pos[0].any() and not neg[0].any() and int(bad[0]) == S * S and int(bad[1]) == 0
    assert count[0].tolist() == [S * S] + [0] * (2 + K) and float(pos[1, 0]) == S * S
    assert ops.part_mass(score, pm, 1, K, want_nonfinite=False)[3] is None
    for kw, word in ((dict(K=0), r"K=0 parts outside \[1, 8\]"), (dict(K=9), r"K=9 parts outside \[1, 8\]"), (dict(rpi=0), r"rows_per_img=0"),
                     (dict(rpi=3), r"R % rows_per_img")):
        with pytest.raises(RuntimeError, match=word):
            ops.part_mass(score, pm, kw.get("rpi", 1), kw.get("K", K))
    with pytest.raises(RuntimeError, match=r"S=0 \(S >= 1\)"):
        ops.part_mass(torch.empty((1, 0, 0), device=DEV), pm[:1], 1, K)
    lib = ops._lib.lib()
    assert lib.ppf_part_mass(None, None, 1, 1, 46341, 16, 16, K, None, None, None, None, None) == -1
    assert "S * S exceeds 2^31 - 1" in lib.ppf_last_error().decode()
    assert lib.ppf_part_mass(None, None, 1, 1, 46340, 16, 16, K, None, None, None, None, None) == -3      # the shape passes; the null pointers do not
    with pytest.raises(ValueError, match="partmap must be"):
        ops.part_mass(score, pm[:1], 1, K)


# ------------------------------------------------------------------------------------------------ partsworld_view
@pytest.fixture(scope="module")
def world():
    spec = _world_spec()
    ds = D.PartsWorld(spec, train=False, return_id=True)
    return spec, ds, D.DeviceDataset(ds, DEV)


@pytest.mark.parametrize("batch_size", [3, 8])
def test_view_of_copy_edits_equals_the_eval_loader(world, batch_size):
    spec, ds, dd = world
    loader = D.DeviceAugLoader(dd, batch_size, D.GpuFinisher(re_prob=0.0), False, _args(spec), square=True)
    n, ws = 0, torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for x, y, ids in loader:
        ids = ids.to(DEV)
        scene = ops.synth_scene(spec, ids)
        rows, changed = ops.synth_edit(spec, scene, torch.zeros((len(ids), 1, 2), dtype=torch.int32, device=DEV))
        assert torch.equal(rows[:, 0], scene) and not changed.any()
        frames = ops.synth_render(spec, rows[:, 0].contiguous(), ids)
        view = D.partsworld_view(spec, frames, 64, D.GpuFinisher(re_prob=0.0), workspace=ws)
        assert view.dtype == torch.float32 and tuple(view.shape) == (len(ids), 3, 64, 64) and torch.equal(view, x)
        n += len(ids)
    assert n == 12
    with pytest.raises(RuntimeError, match="uint8 CUDA tensor"):
        D.partsworld_view(spec, frames.cpu(), 64, D.GpuFinisher(re_prob=0.0))


# ------------------------------------------------------------------------------------------------ part_interventions
@pytest.fixture(scope="module")
def referee(world):
    """The referee pipeline for the first 6 test images and the standard edit list, computed once: numpy edit, numpy render, the CPU
    loader's square transform; the finisher and the model are applied by the tests."""
    spec, ds, _ = world
    ids = ds.ids[:6]
    scene = D.partsworld_scene_from_ids(spec, ids)
    K, C = spec.parts, spec.classes
    std = np.tile(np.array(I.standard_edits(spec), dtype=np.int32)[None], (len(ids), 1, 1))
    rows, changed = D.partsworld_edit(spec, scene, std)
    table = D.partsworld_class_table(spec)
    cf, cf_changed = scene.copy(), np.zeros(len(ids), dtype=np.int32)
    for k in range(K):
        e = np.array([[[D.EDIT_PART_ATTR, k | int(table[(i % C + 1) % C, k]) << 8]] for i in ids], dtype=np.int32)
        o, c = D.partsworld_edit(spec, cf, e)
        cf, cf_changed = o[:, 0], np.maximum(cf_changed, c[:, 0])
    rows, changed = np.concatenate([rows, cf[:, None]], axis=1), np.concatenate([changed, cf_changed[:, None]], axis=1)
    E = rows.shape[1]
    frames = D.partsworld_render(spec, rows.reshape(len(ids) * E, -1), np.repeat(ids, E))
    from PIL import Image
    t = D.build_view_transform(_args(spec), square=True)
    views = np.stack([t(Image.fromarray(f)) for f in frames])                  # uint8 [B * E, 64, 64, 3]
    return ids, scene, rows, changed, views


def test_part_interventions_equal_the_referee_pipeline(world, referee):
    spec, _, _ = world
    ids, scene, rows, changed, views = referee
    B, E = changed.shape
    assert E == spec.parts + 5
    m = _micro_model().eval()
    for value in ("prob", "logit"):
        got = I.part_interventions(m, spec, ids, value=value)
        assert isinstance(got, I.Interventions) and got.value.is_cuda and tuple(got.value.shape) == (B, E, 1) and got.kind == value
        host = got.cpu()
        assert np.array_equal(host.scene, scene) and np.array_equal(host.changed, changed)
        assert host.edits[:, :-1].tolist() == [[list(e) for e in I.standard_edits(spec)]] * B
        assert host.edits[:, -1].tolist() == [[I.EDIT_COUNTERFACTUAL, int((i % 4 + 1) % 4)] for i in ids]
        assert changed[:, 0].tolist() == [0] * B and changed[4, 1:5].sum() == 1
        with torch.no_grad():
            x = D.GpuFinisher(re_prob=0.0)(_dev(views))
            logits = torch.cat([r.logits for r in I.forward_groups(m, x, B)]).contiguous()
            cls = logits.reshape(B, E, -1)[:, 0].argmax(1).to(torch.int32)
            assert np.array_equal(host.classes[:, 0], cls.cpu().numpy())       # the predicted class of the unedited image
            cols = cls[:, None].expand(B, E).reshape(-1).contiguous()
            want = ops.class_prob(logits, cols) if value == "prob" else logits.gather(1, cols.long()[:, None])[:, 0]
        assert np.array_equal(host.value[:, :, 0], want.reshape(B, E).cpu().numpy())
        assert np.array_equal(host.pred, logits.argmax(1).reshape(B, E).cpu().numpy())
        # v[COPY] is the plain forward of the loader's view
        small = I.part_interventions(m, spec, ids, value=value, classes=host.classes, scratch_bytes=80 * 96 * 3 * 5, batch_size=4)
        assert torch.equal(small.value, got.value) and torch.equal(small.pred, got.pred) and torch.equal(small.changed, got.changed)
    with pytest.raises(ValueError, match="value must be"):
        I.part_interventions(m, spec, ids, value="margin")
    with pytest.raises(ValueError, match="invalid edits"):
        I.part_interventions(m, spec, ids, edits=np.tile(np.array([[[1, 1 << 4]]], dtype=np.int32), (B, 1, 1)))


def test_copy_value_is_the_plain_forward(world):
    spec, ds, dd = world
    m = _micro_model().eval()
    loader = D.DeviceAugLoader(dd, 12, D.GpuFinisher(re_prob=0.0), False, _args(spec), square=True)
    x, y, ids = next(iter(loader))
    got = I.part_interventions(m, spec, ids, classes=y.to(torch.int32), edits=np.zeros((12, 1, 2), dtype=np.int32))
    with torch.no_grad():
        logits = m.eval_branches(x).logits.contiguous()
    assert torch.equal(got.value[:, 0, 0], ops.class_prob(logits, y.to(torch.int32).contiguous()))
    assert torch.equal(got.pred[:, 0], logits.argmax(1).to(torch.int32))


# ------------------------------------------------------------------------------------------------ part_attribution
@pytest.mark.parametrize("order", ["evidence", "random"])
def test_part_attribution_equals_the_referee(world, order):
    spec, ds, dd = world
    m = _micro_model().eval()
    loader = D.DeviceAugLoader(dd, 5, D.GpuFinisher(re_prob=0.0), False, _args(spec), square=True)
    x, y, ids = next(iter(loader))
    K, S = spec.parts, 64
    with torch.no_grad():
        outs = I._eval_outputs(m, x)
        cls = torch.stack([y.to(torch.int32), ((y + 1) % 4).to(torch.int32)], dim=1).contiguous()      # two class columns
        score = I.pixel_scores(m, x, outs, cls, order, image_ids=ids.to(DEV), seed=3)
    pos, neg, count, bad = I.part_attribution(m, x, ids, spec, cls, order, seed=3)
    assert tuple(pos.shape) == (10, 3 + K) and (count.sum(1) == S * S).all() and not bad.any()
    maps = D.partsworld_render(spec, D.partsworld_scene_from_ids(spec, ids), ids, partmap=True)[1]
    s = score.cpu().numpy()
    rp, rn, rc, rb = I.part_mass(s, maps, 2, K, device=False)
    assert np.array_equal(count.cpu().numpy(), rc)
    view = D.partsworld_view_partmap(maps, S)
    for r in range(10):
        for c in range(3 + K):
            bound = rc[r, c] * 2.0 ** -53 * float(np.abs(s.reshape(10, S, S)[r][view[r // 2] == c]).astype(np.float64).sum())     # the referee's sums are math.fsum's
            assert abs(float(pos[r, c]) - rp[r, c]) <= bound and abs(float(neg[r, c]) - rn[r, c]) <= bound
    with pytest.raises(ValueError, match="'shap'"):
        I.part_attribution(m, x, ids, spec, cls, "shap")


# ------------------------------------------------------------------------------------------------ the tool
def _json_round_trip(doc):
    from protopformer_amd.tooling import json_clean
    return json.loads(json.dumps(json_clean(doc)))


def test_partcheck_tool_end_to_end(tmp_path):
    from protopformer_amd import partcheck as tool
    from protopformer_amd import tooling
    spec = _world_spec()
    m = _micro_model()
    docs = []
    for bs in (5, 12):
        args = tool.get_args_parser().parse_args(["--data_set", "PartsWorld", "--output_dir", str(tmp_path / f"bs{bs}"), "--input_size", "64", "--batch_size",
                                                  str(bs), "--num_workers", "0", "--orders", "evidence", "random", "--per-image"])
        args.partsworld, args.device_data = spec, True
        docs.append(json.load(open(tool.main(args, model=m))))
    assert docs[0] == docs[1]                                                  # passes of pass_images images, whatever the loader's batch size
    doc = docs[0]
    ds, nb, loader = tooling.eval_loader(args, torch.device(DEV), square=True)
    want = I.part_agreement(m, loader, spec, orders=("evidence", "random"), rise=dict(masks=512, cells=7, p=0.5), ig=dict(steps=32, rule="midpoint"))
    assert doc == _json_round_trip(tool.summarize(want, args))
    assert doc["images"] == 12 and doc["parts"] == 4 and doc["spec"] == spec.to_dict() and set(doc["per_order"]) == {"evidence", "random"}
    assert all(o["undefined"] == 1 and o["defined"] == 11 for o in doc["per_order"].values())
    assert sum(doc["model"]["importance_images"]) == 38                      # the visible parts of the 12 images
    assert doc["model"]["discriminative_parts"] == [0] and doc["settings"]["pass_images"] == 16
    for o in doc["per_order"].values():
        assert sum(o["area_share"].values()) == pytest.approx(1.0, abs=1e-12)
        assert all(o["part_deletion"][k] is not None for k in ("order", "oracle", "reverse"))
    npz = np.load(os.path.join(str(tmp_path / "bs12"), "partcheck.npz"))
    assert npz["value"].shape == (12, 9) and npz["evidence.pos"].shape == (12, 7) and sorted(npz["image_ids"].tolist()) == ds.ids.tolist()
