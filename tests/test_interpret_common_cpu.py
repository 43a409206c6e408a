"""What the interpretability passes share: the prototype pick (select_prototypes) against a plain numpy loop, the K each pass's clamp
rule gives, and the record base every result record stands on (one host read, fields and settings kept).  No GPU: CPU tensors only."""
import types

import numpy as np
import pytest
import torch

from protopformer_amd import interpret as I

B, C, PPC = 3, 4, 3
NAN = float("nan")


def _pick_reference(mode, ppc, classes, act=None, k=None, num_classes=None):
    """The pick written out: ids c * ppc + j of one class per image; 'top': larger activation first, equal ones by the smaller id, a NaN
    before every number (torch.sort's documented order: NaN compares greater than any number), then the first k."""
    rows = []
    for b, c in enumerate(classes):
        c = min(max(int(c), 0), num_classes - 1) if mode == "own" else int(c)
        ids = [c * ppc + j for j in range(ppc)]
        if mode == "top":
            ids = sorted(ids, key=lambda p: (0 if np.isnan(act[b, p]) else 1, -act[b, p] if not np.isnan(act[b, p]) else 0.0, p))[:k]
        rows.append(ids)
    return np.asarray(rows, dtype=np.int64).reshape(len(classes), -1)


def _activations(ppc):
    act = np.arange(B * C * ppc, dtype=np.float32).reshape(B, C * ppc) % 7
    act[0, 1 * ppc:2 * ppc] = 2.5                    # image 0, class 1: all equal -- the smaller id first
    act[1, 2 * ppc + ppc - 1] = NAN                  # image 1, class 2: one NaN
    act[2, 0], act[2, ppc - 1] = 4.0, 4.0            # image 2, class 0: the first and the last equal
    logits = np.full((B, C), -1.0, dtype=np.float32)
    logits[0, 1], logits[1, 2], logits[2, 0] = 3.0, 2.0, 1.0
    return act, logits


@pytest.mark.parametrize("ppc", [PPC, 2])            # 2: the global branch's shape, ppc derived from the activations' width
@pytest.mark.parametrize("k", [0, 1, PPC, PPC + 2])
def test_select_prototypes_top_against_the_loop(ppc, k):
    act, logits = _activations(ppc)
    ppc_derived = act.shape[1] // C
    pred = torch.from_numpy(logits).argmax(1)
    got = I.select_prototypes("top", ppc_derived, pred, torch.from_numpy(act), k)
    want = _pick_reference("top", ppc, pred.tolist(), act, k)
    assert got.dtype == torch.int64 and got.shape == (B, min(k, ppc)) and np.array_equal(got.numpy(), want)
    if k >= ppc:
        assert got[0].tolist() == [ppc, ppc + 1, ppc + 2][:ppc]                                  # equal activations: id order
        assert got[1, 0] == 2 * ppc + ppc - 1                                                    # the NaN where torch.sort puts it: first
    everyone = I.select_prototypes("predicted", ppc_derived, pred)
    assert np.array_equal(everyone.numpy(), _pick_reference("predicted", ppc, pred.tolist()))


@pytest.mark.parametrize("ppc", [PPC, 2])
def test_select_prototypes_own_clamps_the_label(ppc):
    labels = torch.tensor([-3, C + 5, 2])
    got = I.select_prototypes("own", ppc, labels, num_classes=C)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), _pick_reference("own", ppc, labels.tolist(), num_classes=C))
    assert got[0].tolist() == list(range(ppc)) and got[1].tolist() == list(range((C - 1) * ppc, C * ppc))
    with pytest.raises(ValueError, match="mode"):
        I.select_prototypes("best", ppc, labels)


# K per pass for k in (0, 1, ppc, ppc + 2) at ppc = 3, written down from the three passes' code before the pick was shared: alignment_rows
# and characteristic_importance take min(k, ppc), focus_from_outputs max(1, min(k, ppc)).
K_TODAY = {"alignment_rows": [0, 1, 3, 3], "characteristic_importance": [0, 1, 3, 3], "focus_from_outputs": [1, 1, 3, 3]}


class _Picked(Exception):
    pass


def _standin():
    act, logits = _activations(PPC)
    record = types.SimpleNamespace(cls_attn=torch.rand(B, 16), idx=torch.arange(9).repeat(B, 1), act_full=torch.rand(B, C * PPC, 9), logits=torch.from_numpy(logits),
                                   act_max_local=torch.from_numpy(act), act_max_global=torch.from_numpy(act), argmax=torch.zeros(B, C * PPC, dtype=torch.int64),
                                   logits_global=torch.from_numpy(logits))
    return types.SimpleNamespace(eval_branches=lambda x: record, num_prototypes_per_class=PPC, last_layer=types.SimpleNamespace(weight=torch.rand(C, C * PPC)),
                                 prototype_vectors_global=torch.rand(C * PPC, 4))


@pytest.mark.parametrize("who", sorted(K_TODAY))
def test_every_pass_keeps_its_clamp_of_k(monkeypatch, who):
    seen = []

    def recording(mode, ppc, classes, act_max=None, k=None, num_classes=None):
        seen.append(k)
        raise _Picked()
    monkeypatch.setattr(I, "select_prototypes", recording)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)                       # the passes move their batch to the GPU first
    net, x = _standin(), torch.zeros(B, 3, 64, 64)
    for k in (0, 1, PPC, PPC + 2):
        with pytest.raises(_Picked):
            if who == "alignment_rows":
                I.alignment_rows(net, x, protos_per_image=k)
            elif who == "characteristic_importance":
                I.characteristic_importance(net, [(x, torch.zeros(B, dtype=torch.int64))], protos="top", protos_per_image=k)
            else:
                outs = I._eval_outputs(net, x)
                I.focus_from_outputs(outs, torch.zeros(B, 4, dtype=torch.int32), net.last_layer.weight, 0.5, PPC, 9, 64, protos="top", protos_per_image=k, device=False)
    assert seen == K_TODAY[who]


# ------------------------------------------------------------------------------------------------ the record base
def _t(*shape, dtype=torch.float32):
    n = int(np.prod(shape))
    return (torch.arange(n, dtype=torch.float64).reshape(shape) * 1.25 - 3).to(dtype)


def _rise():
    return I.Rise(_t(1, 1, 4, 4), _t(1, 1, 4), _t(2, 1, 1), _t(1, 2, 2, dtype=torch.int32), _t(1, 1, dtype=torch.int32), _t(1, 2, 9, dtype=torch.uint8), 7, 0.25)


def _ig():
    return I.IntegratedGradients(_t(1, 2, 3, 4, 4), _t(1, 2, 1), _t(1, 2, dtype=torch.float64), _t(1, 2), _t(1, 2), _t(1, 2, dtype=torch.int32), _t(3), _t(3),
                                 ["proto", "local"], 3, "midpoint")


def _because(local=True):
    return I.Because(_t(2, 3), _t(2, 3, dtype=torch.int32), _t(5, 2, 3) if local else None, _t(5, 2, 3), _t(5, 2, 3, dtype=torch.int32) if local else None,
                     _t(2, 3, dtype=torch.int32), ["hue", "shape"], "local" if local else "global")


def _focus(protos=True):
    f = {k: _t(2, 3) for k in I.FOCUS_FIELDS}
    f.update(inside=_t(2, 3, dtype=torch.float64), hit=_t(2, 3, dtype=torch.int32), global_ev=None, labels=_t(2, dtype=torch.int64), protos=_t(2, 3, dtype=torch.int32) if protos else None)
    return I.Focus(**f, img_size=64, grid_side=4, patch=16, mode="own", percentile=90)


def _faithfulness(nested=True):
    return I.Faithfulness({"deletion": _t(1, 1, 3), "insertion": _t(1, 1, 3) + 1}, _t(3, dtype=torch.int32), _t(1, 1, dtype=torch.int32), None, _t(1, 1, 4, dtype=torch.int32),
                          _t(1, 1, 4), 4, rise=_rise() if nested else None, ig=_ig() if nested else None, resolution="pixel")


def _explanation():
    return I.Explanation(dict(classes=_t(2, 1, dtype=torch.int32), maps=_t(2, 1, 3, 2, 2)), dict(classes=_t(2, 1, dtype=torch.int32)), {"local": 2, "global": 1},
                         {"local": 0.75, "global": 0.25}, 2, 16, 32)


RECORDS = {"Explanation": (_explanation, 1, dict(ppc={"local": 2, "global": 1}, scale={"local": 0.75, "global": 0.25}, side=2, patch_size=16, img_size=32, against=False)),
           "Rise": (_rise, 1, dict(cells=7, p=0.25)), "IntegratedGradients": (_ig, 1, dict(target=("proto", "local"), steps=3, rule="midpoint")),
           "Because": (_because, 1, dict(characteristics=("hue", "shape"), branch="local")),
           "Because, global branch": (lambda: _because(False), 1, dict(characteristics=("hue", "shape"), branch="global")),
           "Focus": (_focus, 1, dict(img_size=64, grid_side=4, patch=16, mode="own", percentile=90)),
           "Focus without protos": (lambda: _focus(False), 1, dict(img_size=64, grid_side=4, patch=16, mode="own", percentile=90)),
           "Faithfulness": (_faithfulness, 3, dict(grid_cells=4, resolution="pixel")),
           "Faithfulness alone": (lambda: _faithfulness(False), 1, dict(grid_cells=4, resolution="pixel", rise=None, ig=None))}


def _same_bits(host, dev, what):
    if dev is None:
        assert host is None, f"{what}: None became {type(host)}"
    elif isinstance(dev, dict):
        assert list(host) == list(dev)
        for k in dev:
            _same_bits(host[k], dev[k], f"{what}[{k}]")
    else:
        want = dev.numpy()
        assert isinstance(host, np.ndarray) and host.dtype == want.dtype and host.shape == want.shape and host.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_record_goes_to_the_host_in_one_read(monkeypatch, name):
    make, reads, meta = RECORDS[name]
    r = make()
    assert not r.on_host                                   # also when the field the class used to test is None (Focus.protos, Faithfulness.order)
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    h = r.cpu()
    monkeypatch.undo()
    assert len(calls) == reads, f"{len(calls)} host reads"
    assert type(h) is type(r) and h.on_host and h.cpu() is h
    for k, v in r.fields().items():
        _same_bits(getattr(h, k), v, f"{name}.{k}")
    for k, v in meta.items():
        assert getattr(h, k) == v and type(getattr(h, k)) is type(v), k
    if name.startswith("Faithfulness") and r.rise is not None:
        assert h.rise.on_host and h.ig.on_host and h.rise.cells == 7 and h.ig.target == ("proto", "local")
        _same_bits(h.rise.nodes, r.rise.nodes, "rise.nodes")
        _same_bits(h.ig.total, r.ig.total, "ig.total")
        assert set(h.auc()) == {"deletion", "insertion"}


def test_record_construction_by_position_and_by_name():
    r = _rise()
    again = I.Rise(r.saliency, r.cell, r.prob, r.shift, classes=r.classes, nodes=r.nodes, cells=7.0, p=1)
    assert again.cells == 7 and isinstance(again.cells, int) and isinstance(again.p, float) and again.nodes is r.nodes
    with pytest.raises(TypeError):
        I.Rise(r.saliency, r.cell)
    with pytest.raises(TypeError):
        I.Rise(*[None] * 6, 7, 0.5, cells=3)
    with pytest.raises(TypeError):
        I.Rise(*[None] * 6, 7, 0.5, 1)
    assert I.Rise(*[None] * 6, 7, 0.5).on_host
    f = I.Faithfulness({}, None, None, None, None, None, 9)
    assert (f.grid_cells, f.rise, f.ig, f.resolution) == (9, None, None, "cell")
