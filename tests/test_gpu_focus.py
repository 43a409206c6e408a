"""Foreground focus on the GPU: ppf_act_focus against ops.act_peak bit for bit and against the numpy referee, ppf_focus_box_terms and
ppf_reserve_focus against their integer referees, ppf_evidence_focus against the fp64 sums of the same fp32 products, focus_rows against
the referee pipeline on host copies of the same forward's outputs, and the command-line tool on the miniature CUB tree.

Bounds (derived, not measured).  Every fp64 sum here adds n terms that are exact in fp64 (fp32 values, or exact products of them), so
any summation order is within (n - 1) * u * sum|terms| of the exact sum, to first order, with u = 2^-53; as tests/test_gpu_alignment.py
does for ppf_grad_box_mass, the gates are (n - 1) * 2^-52 against an exactly rounded sum (math.fsum) and (n - 1) * 2^-51 between the
kernel and the numpy referee, which are two any-order sums.  n = S^2 for the maps, g^2 for the rollout scores, P for the evidence."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _within(got, ref, n, scale=None, ulps=2.0 ** -51):
    """|got - ref| <= (n - 1) * ulps * scale elementwise (scale: the sum of the terms' magnitudes; default |ref|)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref) if scale is None else np.asarray(scale, dtype=np.float64)
    return bool((np.abs(got - ref) <= max(n - 1, 0) * ulps * scale).all())


# ------------------------------------------------------------------------------------------------ 1. ppf_act_focus
def _maps(g, M, seed):
    """M maps on a g x g grid: random ones, then one of each kind the contract names."""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((M, g, g)) * np.exp(rng.uniform(-3, 3, (M, 1, 1)))).astype(np.float32)
    a[1] = -1.0 - 0.1 * rng.random((g, g)).astype(np.float32)          # all negative and flat enough that no cubic overshoot is positive: sums exactly 0
    a[2] = 1.75                                                        # constant
    a[3] = 0.0                                                         # a symmetric blob: the same value at mirrored cells (an exact tie when g > 1)
    a[3, 0, g - 1] = a[3, g - 1, 0] = 3.0
    a[4, 0, 0] = np.nan                                                # non-finite entries
    a[5, 0, 0], a[5, g - 1, g - 1] = 2.0, np.inf                      # (the non-finite entry last: at g = 1 it is the map)
    a[6, 0, g - 1], a[6, g // 2, g // 2] = 1.0, -np.inf
    a[7] = np.nan                                                      # only NaNs
    a[8, 0, 0], a[8, g - 1, 0] = np.inf, -np.inf
    return a


def _host_maps(grids, S):
    from protopformer_amd.interpret import resize_cubic
    with np.errstate(invalid="ignore"):
        return [resize_cubic(m, S) for m in grids]


def _host_peak(up):
    seen = ~np.isnan(up)
    top = up[seen].max() if seen.any() else np.float32(-np.inf)
    ys, xs = np.where(up == top)
    return (int(ys[0]), int(xs[0])) if ys.size else (0, 0)


def _boxes(ups, per, S, seed):
    """One box per image (`per` maps each): the kinds the contract names, several of them placed at the peak of the image's first map."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(len(ups) // per):
        y, x = _host_peak(ups[j * per])
        kind = j % 8
        out.append([[0, S, 0, S],                                      # the whole image
                    [3, 3, 0, S],                                      # empty
                    [y, y + 1, x, x + 1],                              # one pixel: the peak's
                    [-5, S + 9, -(1 << 30), (1 << 30)],                # negative and beyond-S corners
                    [0, y, 0, S],                                      # y1 equals the peak's row: excluded
                    [0, S, 0, x],                                      # x1 equals the peak's column: excluded
                    [0, y + 1, 0, x + 1],                              # y1 - 1 and x1 - 1 equal the peak's coordinates: included
                    [S, 0, S, 0]][kind] if kind < 7 or j % 16 == 7 else sorted(rng.integers(-2, S + 3, 2).tolist()) + sorted(rng.integers(-2, S + 3, 2).tolist()))
    return np.array(out, dtype=np.int32)


def _check_act_focus(grids, boxes, S, exact_rows):
    from protopformer_amd import ops
    from protopformer_amd.interpret import act_focus
    M, per = grids.shape[0], grids.shape[0] // boxes.shape[0]
    gd, bd = _dev(grids), _dev(boxes)
    got = ops.act_focus(gd, S, bd)
    pv, pyx, _ = ops.act_peak(gd, S)
    again = ops.act_focus(gd, S, bd)
    torch.cuda.synchronize()
    dt = dict(peak_val=torch.float32, peak_yx=torch.int32, hit=torch.int32, inside=torch.float64, total=torch.float64, nonfinite=torch.int32)
    assert all(got[k].dtype == dt[k] and got[k].is_cuda and got[k].shape[0] == M for k in dt)
    assert all(torch.equal(got[k].view(torch.int64) if got[k].dtype == torch.float64 else got[k].view(torch.int32),
                           again[k].view(torch.int64) if got[k].dtype == torch.float64 else again[k].view(torch.int32)) for k in dt), "a repeated launch differs"
    assert torch.equal(got["peak_val"].view(torch.int32), pv.view(torch.int32)) and torch.equal(got["peak_yx"], pyx), "the peak differs from ppf_act_peak"
    ref = act_focus(grids, S, boxes, device=False)
    h = {k: v.cpu().numpy() for k, v in got.items()}
    assert (_bits(h["peak_val"]) == _bits(ref["peak_val"])).all() and np.array_equal(h["peak_yx"], ref["peak_yx"])
    assert np.array_equal(h["hit"], ref["hit"]) and np.array_equal(h["nonfinite"], ref["nonfinite"])
    n = S * S
    for k in ("inside", "total"):
        print(f"{k}: max |device - referee| / ((n - 1) 2^-51 referee) = "
              f"{float(np.max(np.abs(h[k] - ref[k]) / np.maximum((n - 1) * 2.0 ** -51 * ref[k], 1e-300))):.2e}")
        assert _within(h[k], ref[k], n), f"{k} outside the any-order bound of the referee"
    assert (h["inside"] <= h["total"]).all() and (h["inside"] >= 0).all()
    ob = np.clip(boxes.astype(np.int64), 0, S)
    for m in exact_rows:                                               # against the exactly rounded sums
        up = _host_maps(grids[m:m + 1], S)[0]
        with np.errstate(invalid="ignore"):
            pos = np.where(np.isfinite(up) & (up > 0), up, np.float32(0)).astype(np.float64)
        y0, y1, x0, x1 = ob[m // per]
        tt, ti = math.fsum(pos.reshape(-1).tolist()), math.fsum(pos[y0:max(y0, y1), x0:max(x0, x1)].reshape(-1).tolist())
        assert abs(h["total"][m] - tt) <= (n - 1) * 2.0 ** -52 * tt and abs(h["inside"][m] - ti) <= (n - 1) * 2.0 ** -52 * ti, m
    none = ops.act_focus(gd, S, bd, want_nonfinite=False)              # the counter is optional
    assert none["nonfinite"] is None and torch.equal(none["inside"], got["inside"]) and torch.equal(none["hit"], got["hit"])
    return h, ref


@pytest.mark.parametrize("per", [1, 3])
@pytest.mark.parametrize("g,S", [(1, 1), (3, 7), (4, 64), (14, 222), (14, 224)])
def test_act_focus_against_act_peak_and_the_referee(g, S, per):
    M = 24
    grids = _maps(g, M, seed=10 * g + S)
    ups = _host_maps(grids, S)
    boxes = _boxes(ups, per, S, seed=S + per)
    h, ref = _check_act_focus(grids, boxes, S, exact_rows=range(0, M, 5))
    assert h["inside"][1] == 0.0 and h["total"][1] == 0.0, "an all-negative map has no positive mass"
    assert h["peak_yx"][7].tolist() == [0, 0] and h["peak_val"][7] == -np.inf and h["nonfinite"][7] == S * S and h["total"][7] == 0.0
    assert h["nonfinite"][4] > 0 and h["nonfinite"][5] > 0 and h["nonfinite"][0] == 0
    if g > 1 and S > 1:
        up = ups[3]
        assert int((up == up.max()).sum()) >= 2, "the blob's peak is an exact tie"
    if per == 1:                                                       # box j belongs to map j: the kinds placed at that map's own peak
        assert h["hit"][0] == 1 and h["inside"][0] == h["total"][0] and h["hit"][1] == 0 and h["hit"][3] == 1 and h["inside"][3] == h["total"][3]
        assert h["hit"][2] == 1 and h["hit"][4] == 0 and h["hit"][5] == 0 and h["hit"][6] == 1
        assert h["hit"][7] == 0 and h["inside"][7] == 0.0              # the inverted box is empty


def test_act_focus_with_more_rows_than_workgroup_slots():
    g, S, M, per = 4, 16, 3000, 3
    rng = np.random.default_rng(7)
    grids = rng.standard_normal((M, g, g)).astype(np.float32)
    grids[::97, 1, 2] = np.nan
    lo = rng.integers(-2, S, (M // per, 2))
    boxes = np.stack([lo[:, 0], lo[:, 0] + rng.integers(0, S, M // per), lo[:, 1], lo[:, 1] + rng.integers(0, S, M // per)], axis=1).astype(np.int32)
    h, _ = _check_act_focus(grids, boxes, S, exact_rows=(0, 1499, 2999))
    assert 0 < h["hit"].sum() < M


def test_act_focus_refuses_what_the_c_side_cannot_see():
    from protopformer_amd import ops
    grids, obj = torch.zeros(6, 4, 4, device="cuda"), torch.zeros(2, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="obj must be"):
        ops.act_focus(grids, 16, obj.long())
    with pytest.raises(ValueError, match="obj must be"):
        ops.act_focus(grids, 16, obj.cpu())
    with pytest.raises(ValueError, match="obj must be"):
        ops.act_focus(grids, 16, torch.zeros(2, 5, dtype=torch.int32, device="cuda")[:, :4])
    with pytest.raises(ValueError, match="do not divide"):
        ops.act_focus(grids, 16, torch.zeros(4, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="fp32"):
        ops.act_focus(grids.double(), 16, obj)
    with pytest.raises(RuntimeError, match="LDS"):
        ops.act_focus(torch.zeros(1, 64, 64, device="cuda"), 1024, obj[:1])


# ------------------------------------------------------------------------------------------------ 2. the integer kernels
@pytest.mark.parametrize("S,per", [(1, 1), (64, 3), (224, 1)])
def test_focus_box_terms_equal_the_referee(S, per):
    from protopformer_amd.interpret import focus_box_terms
    rng = np.random.default_rng(S)
    M = 300 * per                                                      # more than one workgroup
    box = np.sort(rng.integers(-3, S + 4, (M, 2, 2)), axis=2).reshape(M, 4).astype(np.int32)
    box[0], box[1], box[2] = (0, 1, 0, 1), (0, S, 0, S), (5, 5, 0, S)                              # nothing passed; the whole image; empty
    obj = np.sort(rng.integers(-3, S + 4, (M // per, 2, 2)), axis=2).reshape(-1, 4).astype(np.int32)
    obj[0], obj[1 % len(obj)] = (0, S, 0, S), (S, 0, S, 0)
    got = focus_box_terms(_dev(box), _dev(obj), S)
    assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), focus_box_terms(box, obj, S, device=False))
    t = got.cpu().numpy().astype(np.int64)
    assert (t[:, 3] == t[:, 1] + t[:, 2] - t[:, 0]).all() and (t[:, 0] <= np.minimum(t[:, 1], t[:, 2])).all() and t.max() <= S * S and t[:, 0].max() > 0


@pytest.mark.parametrize("g,patch", [(1, 1), (1, 16), (4, 1), (4, 16), (14, 1), (14, 16)])
def test_reserve_focus_equals_the_referee(g, patch):
    from protopformer_amd import ops
    from protopformer_amd.interpret import reserve_focus
    rng = np.random.default_rng(100 * g + patch)
    B, G, S = 9, g * g, g * patch
    T = max(1, min(G, 81) + 3)
    idx = rng.integers(0, G, (B, T)).astype(np.int32)                  # cells drawn with replacement: duplicates
    idx[0, 0], idx[1, -1], idx[2, T // 2] = -1, G, G + 7               # entries out of range
    idx[3] = idx[3, 0]                                                 # one cell T times
    obj = np.sort(rng.integers(-2, S + 3, (B, 2, 2)), axis=2).reshape(B, 4).astype(np.int32)          # boxes that cut cells when patch > 1
    obj[4], obj[5], obj[6] = (0, S, 0, S), (S // 2, S // 2, 0, S), (-9, 1 << 30, -9, 1 << 30)
    ta = rng.random((B, G)).astype(np.float32) * np.exp(rng.uniform(-6, 6, (B, G))).astype(np.float32)
    ta[7, 0], ta[8, G - 1], ta[8, 0] = np.nan, np.inf, -np.inf
    out, attn = reserve_focus(_dev(idx), _dev(obj), g, patch, _dev(ta))
    out2, attn2 = reserve_focus(_dev(idx), _dev(obj), g, patch, _dev(ta))
    ro, ra = reserve_focus(idx, obj, g, patch, ta, device=False)
    assert out.dtype == torch.int32 and attn.dtype == torch.float64 and np.array_equal(out.cpu().numpy(), ro)
    assert torch.equal(out, out2) and torch.equal(attn.view(torch.int64), attn2.view(torch.int64)), "a repeated launch differs"
    mass = np.where(np.isfinite(ta), np.abs(ta), 0).astype(np.float64).sum(1)
    assert _within(attn.cpu().numpy(), ra, G, mass[:, None])
    o = out.cpu().numpy()
    assert o[4].tolist() == [T * patch * patch, T, G, T] and o[5].tolist() == [0, 0, 0, T] and o[6, 2] == G and o[0, 3] == T - 1 and o[2, 3] == T - 1
    assert float(attn[4, 0]) == float(attn[4, 1])
    only, none = reserve_focus(_dev(idx), _dev(obj), g, patch)         # the scores are optional
    assert none is None and torch.equal(only, out)
    with pytest.raises(ValueError, match="token_attn must be"):
        ops.reserve_focus(_dev(idx), _dev(obj), g, patch, _dev(ta[:, :-1]) if G > 1 else _dev(ta).double())
    with pytest.raises(ValueError, match="obj must be"):
        ops.reserve_focus(_dev(idx), _dev(obj[:-1]), g, patch)


# ------------------------------------------------------------------------------------------------ 3. ppf_evidence_focus
def _evidence_case(P, ppc, M, seed, T=9, g=4, patch=16, B=5):
    rng = np.random.default_rng(seed)
    C = P // ppc
    act = (rng.random((B, P)) * 6).astype(np.float32)
    w = (np.where(np.arange(P)[None, :] // ppc == np.arange(C)[:, None], 1.0, -0.5) + 0.05 * rng.standard_normal((C, P))).astype(np.float32)
    idx = np.stack([rng.permutation(g * g)[:T] for _ in range(B)]).astype(np.int32)
    idx[0, 0], idx[1, 1] = -1, g * g                                   # cells outside the grid: not located
    argmax = rng.integers(0, T, (B, P)).astype(np.int32)
    argmax[2, 0], argmax[3, P - 1] = -1, T                             # an argmax out of range on either side
    cls = rng.integers(0, C, (B, M)).astype(np.int32)
    cls[0, 0], cls[1, M - 1] = -1, C                                   # classes outside [0, C)
    S = g * patch
    obj = np.sort(rng.integers(0, S + 1, (B, 2, 2)), axis=2).reshape(B, 4).astype(np.int32)
    obj[4] = (0, S, 0, S)
    return act, w, idx, argmax, cls, obj, C


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("P,ppc", [(1, 1), (7, 1), (2000, 10)])
def test_evidence_focus_against_the_referee(P, ppc, M):
    from protopformer_amd.interpret import evidence_focus
    act, w, idx, argmax, cls, obj, C = _evidence_case(P, ppc, M, seed=P + M)
    scale, g, patch = 0.7, 4, 16
    dev = [_dev(v) for v in (act, w)]
    ev, cnt = evidence_focus(dev[0], dev[1], scale, ppc, _dev(cls), _dev(obj), g, patch, _dev(idx), _dev(argmax))
    ev2, cnt2 = evidence_focus(dev[0], dev[1], scale, ppc, _dev(cls), _dev(obj), g, patch, _dev(idx), _dev(argmax))
    re, rc = evidence_focus(act, w, scale, ppc, cls, obj, g, patch, idx, argmax, device=False)
    mass, _ = evidence_focus(np.abs(act), np.abs(w), scale, ppc, cls, obj, g, patch, idx, argmax, device=False)     # fl(|a| * fl(s * |w|)) = |term|
    assert ev.dtype == torch.float64 and cnt.dtype == torch.int32 and ev.shape == cnt.shape == (act.shape[0], M, 4)
    assert np.array_equal(cnt.cpu().numpy(), rc) and torch.equal(cnt, cnt2) and torch.equal(ev.view(torch.int64), ev2.view(torch.int64))
    assert _within(ev.cpu().numpy(), re, P, mass)
    valid = (cls >= 0) & (cls < C)
    assert (rc.sum(2) == np.where(valid, P, 0)).all() and not ev.cpu().numpy()[~valid].any()
    # the four sums together are the branch's share of the logit
    w32 = (np.float32(scale) * w).astype(np.float32)
    for b in range(act.shape[0]):
        for m in range(M):
            if valid[b, m]:
                logit = math.fsum((act[b] * w32[cls[b, m]]).astype(np.float64).tolist())
                assert abs(float(ev[b, m].sum()) - logit) <= (P + 3) * 2.0 ** -52 * float(mass[b, m].sum())


def test_evidence_focus_without_an_argmax_and_with_a_nan():
    from protopformer_amd.interpret import evidence_focus
    act, w, idx, argmax, cls, obj, C = _evidence_case(70, 10, 2, seed=3)
    g, patch = 4, 16
    cls[0, 0] = 2
    # argmax None with T = 1: every prototype sits at idx[b][0] (idx[0][0] = -1: nothing located in image 0)
    i1 = np.ascontiguousarray(idx[:, :1])
    ev, cnt = evidence_focus(_dev(act), _dev(w), 0.5, 10, _dev(cls), _dev(obj), g, patch, _dev(i1), None)
    re, rc = evidence_focus(act, w, 0.5, 10, cls, obj, g, patch, i1, None, device=False)
    mass, _ = evidence_focus(np.abs(act), np.abs(w), 0.5, 10, cls, obj, g, patch, i1, None, device=False)
    assert np.array_equal(cnt.cpu().numpy(), rc) and _within(ev.cpu().numpy(), re, 70, mass)
    assert rc[0, 0].tolist() == [0, 10, 0, 60] and rc[4, 0].tolist() == [10, 0, 60, 0]               # not located; the whole image
    # a NaN and an inf activation: the sums hold them where the referee's do
    act[2, 5], act[3, 11] = np.nan, np.inf
    ev, cnt = evidence_focus(_dev(act), _dev(w), 0.5, 10, _dev(cls), _dev(obj), g, patch, _dev(idx), _dev(argmax))
    re, rc = evidence_focus(act, w, 0.5, 10, cls, obj, g, patch, idx, argmax, device=False)
    e = ev.cpu().numpy()
    fin = np.isfinite(re)
    assert np.array_equal(cnt.cpu().numpy(), rc) and np.array_equal(np.isnan(e), np.isnan(re)) and np.isnan(re[2]).any() and not fin[3].all()
    assert np.array_equal(e[~fin & ~np.isnan(re)], re[~fin & ~np.isnan(re)])                          # +-inf, the same sign
    with np.errstate(invalid="ignore"):
        mass, _ = evidence_focus(np.abs(act), np.abs(w), 0.5, 10, cls, obj, g, patch, idx, argmax, device=False)
    assert _within(e[fin], re[fin], 70, mass[fin])


# ------------------------------------------------------------------------------------------------ 4. through the micro models
INT_FIELDS = ("protos", "classes", "peak_yx", "hit", "nonfinite", "box", "terms", "reserve", "cnt", "obj", "labels")


def _micro_case(fixture):
    sd, cfg, z = micro(fixture)
    m = build_micro(cfg, sd).eval()
    x = torch.from_numpy(z["img"]).cuda()
    B, S = x.shape[0], cfg["img"]
    rng = np.random.default_rng(11)
    obj = np.sort(rng.integers(0, S + 1, (B, 2, 2)), axis=2).reshape(B, 4).astype(np.int32)
    obj[0], obj[B - 1] = (0, S, 0, S), (S // 2, S // 2, 0, S)          # the whole image; empty
    return m, cfg, x, torch.from_numpy(obj).cuda(), torch.from_numpy(z["label"]).cuda().long()


def _hold_to_referee(f, r, cfg, weight_abs_run):
    S, G, P = cfg["img"], (cfg["img"] // 16) ** 2, cfg["num_prototypes"]
    for k in INT_FIELDS:
        assert np.array_equal(getattr(f, k), getattr(r, k)), k
    assert (_bits(f.peak_val) == _bits(r.peak_val)).all()
    assert _within(f.inside, r.inside, S * S) and _within(f.total, r.total, S * S)
    assert _within(f.attn, r.attn, G) and _within(f.ev, r.ev, P, weight_abs_run) and np.array_equal(f.global_ev, r.global_ev)


@pytest.mark.parametrize("mode", ["own", "top"])
@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_focus_rows_against_the_referee_pipeline(fixture, mode):
    from protopformer_amd.interpret import evidence_focus, focus_from_outputs, focus_rows
    m, cfg, x, obj, labels = _micro_case(fixture)
    seen = {}
    forward = m.eval_branches
    m.eval_branches = lambda images: seen.setdefault("record", forward(images))       # keep the record of the forward focus_rows runs
    try:
        dev = focus_rows(m, x, obj, labels, protos=mode, protos_per_image=2, percentile=90)
    finally:
        del m.eval_branches
    r = seen["record"]
    B, ppc, coe = x.shape[0], cfg["protos_per_class"], cfg["global_coe"]
    K = ppc if mode == "own" else min(2, ppc)
    assert dev.protos.is_cuda and dev.protos.shape == (B, K) and dev.inside.dtype == torch.float64 and not dev.on_host
    f = dev.cpu()
    assert f.on_host and (f.img_size, f.grid_side, f.patch, f.mode, f.percentile) == (cfg["img"], cfg["img"] // 16, 16, mode, 90)
    outs = dict(token_attn=r.cls_attn.reshape(B, -1).float().contiguous(), idx=r.idx.contiguous(), act_full=r.act_full.contiguous(),
                logits=r.logits.contiguous(), act_max=r.act_max_local.contiguous(), argmax=r.argmax, logits_global=r.logits_global)
    host = {k: (None if v is None else v.detach().cpu()) for k, v in outs.items()}
    w = m.last_layer.weight.detach()
    ref = focus_from_outputs(host, obj.cpu(), w.cpu(), 1.0 - coe, ppc, cfg["reserve_k"], cfg["img"], labels.cpu(), mode, 2, 90, coe, device=False)
    mass, _ = evidence_focus(host["act_max"].abs(), w.cpu().abs(), 1.0 - coe, ppc, f.classes[:, None], obj.cpu(), f.grid_side, 16, host["idx"], host["argmax"],
                             device=False)
    _hold_to_referee(f, ref, cfg, mass.reshape(B, 4))
    assert (f.hit[0] == 1).all() and (f.inside[0] == f.total[0]).all() and (f.hit[B - 1] == 0).all() and (f.inside[B - 1] == 0).all()
    assert (f.cnt.sum(1) == cfg["num_prototypes"]).all() and (f.reserve[:, 3] == cfg["reserve_k"]).all() and f.classes.tolist() == r.logits.argmax(1).tolist()
    local = r.logits_local.double().cpu().numpy()[np.arange(B), f.classes] * (1.0 - coe)
    assert np.allclose(f.ev.sum(1), local, rtol=1e-5, atol=1e-5)                                      # the four sums: the local branch's share of the logit
    # batch independence on the collected outputs: the two halves through the kernels give the rows of the whole, bit for bit
    whole = focus_from_outputs(outs, obj, w.contiguous(), 1.0 - coe, ppc, cfg["reserve_k"], cfg["img"], labels, mode, 2, 90, coe).cpu()
    h = B // 2
    parts = [focus_from_outputs({k: (None if v is None else v[s].contiguous()) for k, v in outs.items()}, obj[s].contiguous(), w.contiguous(), 1.0 - coe, ppc,
                                cfg["reserve_k"], cfg["img"], labels[s], mode, 2, 90, coe).cpu() for s in (slice(0, h), slice(h, B))]
    for k, v in whole.fields().items():
        joined = np.concatenate([getattr(p, k) for p in parts])
        assert joined.dtype == v.dtype and joined.tobytes() == v.tobytes(), f"{k}: the halves differ from the whole"
        assert v.tobytes() == getattr(f, k).tobytes(), f"{k}: focus_rows differs from focus_from_outputs on its own forward's outputs"


def test_foreground_focus_over_a_loader():
    from protopformer_amd.interpret import focus_summary, foreground_focus, scaled_boxes
    m, cfg, x, _, labels = _micro_case("micro_deit.npz")
    B, S = x.shape[0], cfg["img"]
    ids = torch.tensor([40, 7, 19, 3][:B] + list(range(100, 100 + max(0, B - 4))))
    boxes = {int(i): (3 + j, 5, 40 + 5 * j, 30 + 9 * j) for j, i in enumerate(ids)}
    sizes = {int(i): (80 + 8 * j, 64 + j) for j, i in enumerate(ids)}
    loader = [(x[i:i + 3], labels[i:i + 3], ids[i:i + 3]) for i in range(0, B, 3)]
    res = foreground_focus(m, loader, boxes, sizes, protos="own", percentile=90, per_image=True)
    rows = res.pop("per_image")
    assert res["images"] == B and res["rows"] == B * cfg["protos_per_class"] and rows["image_ids"].tolist() == ids.tolist()
    assert np.array_equal(rows["obj"], scaled_boxes(ids.tolist(), boxes, sizes, S)) and rows["labels"].tolist() == labels.tolist()
    assert res["settings"] == dict(protos="own", protos_per_image=3, percentile=90, img_size=S, patch=16)
    want = focus_summary(rows, S, 16)
    assert {k: res[k] for k in want} == want
    o = res["overall"]
    assert 0 <= o["prototype_maps"]["pointing"] <= 1 and 0 < o["prototype_maps"]["chance"] <= 1 and 0 <= o["reservation"]["reserved_on_object"] <= 1
    assert o["prototype_maps"]["energy_rows"] + o["prototype_maps"]["zero_total_rows"] == res["rows"]
    assert sorted(res["per_prototype"]) == sorted(set(rows["protos"].reshape(-1).tolist())) and sorted(res["per_class"]) == sorted(set(labels.tolist()))
    top = foreground_focus(m, loader, boxes, sizes, protos="top", protos_per_image=1, max_images=B - 1)
    assert top["images"] == B - 1 and top["rows"] == B - 1 and top["per_prototype"] is None and "per_image" not in top
    with pytest.raises(ValueError, match="no image"):
        foreground_focus(m, [], boxes, sizes)
    with pytest.raises(RuntimeError, match="CUDA/HIP batch"):
        from protopformer_amd.interpret import focus_rows
        focus_rows(m, x.cpu(), torch.zeros(B, 4, dtype=torch.int32), labels)


# ------------------------------------------------------------------------------------------------ 5. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def test_tool_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd import focus as tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    from protopformer_amd.interpret import scaled_boxes
    from protopformer_amd.protopformer import construct_PPNet
    tree, out = str(tmp_path / "data"), str(tmp_path / "out")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1, add_on_layers_type="regular").cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    args = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", out, "--resume", ck, "--max_images", "6",
                                              "--per-image", *MODEL_FLAGS])
    path = tool.main(args)
    doc = json.load(open(path))
    assert path == os.path.join(out, "focus.json") and doc["images"] == 6 and doc["rows"] == 12
    assert doc["settings"] == dict(protos="own", protos_per_image=3, percentile=95.0, img_size=224, patch=16, split="test", data_set="CUB2011U",
                                   boxes="bounding_boxes.txt")
    assert set(doc["overall"]) == {"prototype_maps", "reservation", "evidence"} and len(doc["per_prototype"]) >= 2
    pm, rv = doc["overall"]["prototype_maps"], doc["overall"]["reservation"]
    assert pm["rows"] == 12 and 0 <= pm["pointing"] <= 1 and 0 < pm["chance"] < 1 and rv["images"] == 6 and abs(rv["chance"] - pm["chance"]) < 1e-12
    assert 0 <= rv["reserved_on_object"] <= 1 and 0 <= rv["object_recall"] <= 1 and 0 <= rv["attention_on_object"] <= 1
    z = np.load(os.path.join(out, "focus.npz"))
    ids = z["image_ids"].tolist()
    test_ids = [i for i, _, t in sorted(mini_trees.CUB_ROWS) if t == 0 and i not in mini_trees.CUB_NO_LABEL]
    assert len(ids) == 6 and set(ids) <= set(test_ids) and z["protos"].shape == (6, 2) and z["inside"].dtype == np.float64
    boxes = {i: (10 + i, 5 + i, 10 + i + 60 + 2 * i, 5 + i + 40 + i) for i in ids}                    # bounding_boxes.txt of the tree: x, y, width, height
    assert np.array_equal(z["obj"], scaled_boxes(ids, boxes, {i: mini_trees.cub_size(i) for i in ids}, 224))
