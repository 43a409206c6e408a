"""Prototype bank on the GPU: ppf_proto_topk_merge against a host referee (exact), order / batch-size invariance at kernel level, the
bank through the micro models, projection, and the command-line tool on the miniature CUB tree.

The referee is a stable sort by (-value, image id) over the concatenated candidates in torch on the CPU.  The kernel only moves the
fp32 values it was given, so every comparison is exact (torch.equal on the bit patterns), never a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = 32
SENTINEL = -7.0                                   # best_feat rows the kernel must leave alone keep this value


# ------------------------------------------------------------------------------------------------ referee and generators
def referee(act, ids, labels, ppc, K, pos=None):
    """act [N, P] fp32, ids [N], labels [N] (CPU).  Returns val [P, K], img [P, K], pos [P, K], src [P] (row of the rank-0 candidate in
    the concatenation, -1 when the list is empty).  A candidate is offered to prototype p when ppc == 0 or label == p // ppc; NaN is
    never admitted; unfilled slots are -inf / -1 / -1."""
    N, P = act.shape
    by_id = torch.argsort(ids, stable=True)                                        # secondary key first ...
    v = act[by_id].clone()
    if ppc > 0:
        offered = labels[by_id][:, None] == (torch.arange(P) // ppc)[None, :]
        v[~offered] = float("-inf")
    v[torch.isnan(v)] = float("-inf")
    order = torch.sort(-v, dim=0, stable=True).indices[:K]                          # ... then a stable sort by -value: [K, P]
    if order.shape[0] < K:
        order = torch.cat([order, order[-1:].expand(K - order.shape[0], P)])       # fewer candidates than K: the padding is masked below
        pad = torch.arange(K)[:, None] >= N
    else:
        pad = torch.zeros(K, 1, dtype=torch.bool)
    val = torch.gather(v, 0, order)
    val = torch.where(pad.expand(K, P), torch.full_like(val, float("-inf")), val)
    empty = val == float("-inf")
    rows = by_id[order]                                                             # [K, P] rows of the concatenation
    img = torch.where(empty, torch.full_like(rows, -1), ids[rows]).to(torch.int32)
    if pos is None:
        gp = torch.full((K, P), -1, dtype=torch.int32)
    else:
        gp = torch.where(empty, torch.full_like(rows, -1), torch.gather(pos.long(), 0, rows)).to(torch.int32)
    src = torch.where(empty[0], torch.full_like(rows[0], -1), rows[0])
    return val.t().contiguous(), img.t().contiguous(), gp.t().contiguous(), src


def make_candidates(N, P, k, n_classes, seed, local=True, grid=None):
    """Synthetic candidates: activations quantised to 1/8 (frequent ties), unique shuffled image ids, tokens, and for the local branch
    argmax [N, P] and ascending reserved-token indices idx [N, k] in a grid of `grid` cells."""
    g = torch.Generator().manual_seed(seed)
    act = torch.randint(0, 40, (N, P), generator=g).float() / 8.0
    ids = (torch.randperm(N, generator=g) * 3 + 5).to(torch.int32)
    labels = torch.randint(0, n_classes, (N,), generator=g)
    tok = torch.rand((N, 1 + k, DP), generator=g)
    argmax = idx = None
    if local:
        grid = grid or (196 if k == 81 else 16)
        argmax = torch.randint(0, k, (N, P), generator=g).to(torch.int32)
        idx = torch.stack([torch.randperm(grid, generator=g)[:k].sort().values for _ in range(N)]).to(torch.int32)
    return dict(act=act, ids=ids, labels=labels, tok=tok, argmax=argmax, idx=idx)


def grid_pos(c):
    return torch.gather(c["idx"].long(), 1, c["argmax"].long()) if c["argmax"] is not None else None


def new_state(P, K):
    from protopformer_amd import ops
    s = dict(val=torch.empty((P, K), dtype=torch.float32, device="cuda"), img=torch.empty((P, K), dtype=torch.int32, device="cuda"),
             pos=torch.empty((P, K), dtype=torch.int32, device="cuda"), best_feat=torch.full((P, DP), SENTINEL, device="cuda"))
    ops.proto_topk_init(s["val"], s["img"], s["pos"])
    return s


def feed(state, c, rows, ppc):
    """One launch over the rows `rows` of the candidate set c."""
    from protopformer_amd import ops
    d = lambda t: None if t is None else t[rows].contiguous().cuda()
    ops.proto_topk_merge(d(c["act"]), d(c["argmax"]), d(c["idx"]), d(c["tok"]), 1 if c["argmax"] is not None else 0, d(c["labels"]), d(c["ids"]),
                         ppc, state["val"], state["img"], state["pos"], state["best_feat"])


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def check_against_referee(state, c, ppc, K, what=""):
    val, img, pos, src = referee(c["act"], c["ids"].long(), c["labels"], ppc, K, grid_pos(c))
    assert torch.equal(bits(state["val"]), bits(val)), f"{what}: val differs from the referee"
    assert torch.equal(state["img"].cpu(), img), f"{what}: img differs from the referee"
    assert torch.equal(state["pos"].cpu(), pos), f"{what}: pos differs from the referee"
    P = val.shape[0]
    want = torch.full((P, DP), SENTINEL)
    for p in range(P):
        n = int(src[p])
        if n >= 0:
            want[p] = c["tok"][n, 1 + int(c["argmax"][n, p])] if c["argmax"] is not None else c["tok"][n, 0]
    assert torch.equal(bits(state["best_feat"]), bits(want)), f"{what}: best_feat is not the rank-0 candidate's token"
    return val, img


# ------------------------------------------------------------------------------------------------ 1. kernel against the referee
CASES = [(7, 5, 1, 9), (64, 64, 10, 81), (256, 2000, 10, 81), (300, 130, 64, 81), (1024, 33, 3, 9)]


@pytest.mark.parametrize("local", [True, False], ids=["argmax", "noargmax"])
@pytest.mark.parametrize("class_specific", [True, False], ids=["class", "all"])
@pytest.mark.parametrize("B,P,K,k", CASES)
def test_kernel_against_referee(B, P, K, k, class_specific, local):
    """Two launches of B candidates each (the second merges into the first's lists), one NaN candidate row and one single NaN."""
    ppc = {5: 2, 64: 4, 2000: 10, 130: 10, 33: 3}[P] if class_specific else 0
    n_classes = -(-P // ppc) if ppc else 7
    c = make_candidates(2 * B, P, k, n_classes, seed=B + P + K, local=local)
    c["act"][1, :] = float("nan")
    c["act"][B + 2, 0] = float("nan")
    state = new_state(P, K)
    feed(state, c, slice(0, B), ppc)
    feed(state, c, slice(B, 2 * B), ppc)
    val, img = check_against_referee(state, c, ppc, K, f"B={B} P={P} K={K} k={k} ppc={ppc} local={local}")
    assert not torch.isnan(val).any() and int(c["ids"][1]) not in set(img.reshape(-1).tolist())        # the NaN row was never admitted
    if class_specific and (B, P, K) in ((64, 64, 10), (300, 130, 64)):
        assert bool((img == -1).any()), "this case has classes with fewer than K images: some slots must stay unfilled"


def test_kernel_ties_and_unfilled_slots_known_answer():
    """Hand-made: 5 images, 2 prototypes of classes 0 / 1, K = 3; equal activations are ordered by smaller image id, class 1 has one image."""
    act = torch.tensor([[2.0, 9.0], [2.0, 9.0], [3.0, 9.0], [2.0, 1.5], [float("nan"), 9.0]])
    c = dict(act=act, ids=torch.tensor([40, 10, 30, 20, 5], dtype=torch.int32), labels=torch.tensor([0, 0, 0, 1, 0]),
             tok=torch.arange(5 * 2 * DP, dtype=torch.float32).reshape(5, 2, DP), argmax=None, idx=None)
    state = new_state(2, 3)
    feed(state, c, slice(0, 5), 1)
    assert state["val"].cpu().tolist() == [[3.0, 2.0, 2.0], [1.5, float("-inf"), float("-inf")]]
    assert state["img"].cpu().tolist() == [[30, 10, 40], [20, -1, -1]]
    assert state["pos"].cpu().tolist() == [[-1, -1, -1], [-1, -1, -1]]
    assert torch.equal(state["best_feat"].cpu(), torch.stack([c["tok"][2, 0], c["tok"][3, 0]]))


# ------------------------------------------------------------------------------------------------ 2. order and batch-size invariance
def test_kernel_order_and_batch_size_invariance():
    N, P, K, k = 1000, 200, 10, 81
    c = make_candidates(N, P, k, 20, seed=77)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(3))
    states = []
    for rows in ([slice(b, min(N, b + 256)) for b in range(0, N, 256)], [perm[b:b + 100] for b in range(0, N, 100)], [slice(0, N)]):
        s = new_state(P, K)
        for r in rows:
            feed(s, c, r, 10)
        states.append(s)
    check_against_referee(states[0], c, 10, K, "batches of 256")
    for name in ("val", "img", "pos", "best_feat"):
        a = bits(states[0][name])
        assert torch.equal(a, bits(states[1][name])), f"{name}: batches of 256 in order vs batches of 100 shuffled"
        assert torch.equal(a, bits(states[2][name])), f"{name}: batches of 256 vs one batch of 1000"


def test_binding_rejects_bad_shapes_on_device():
    from protopformer_amd import ops
    c = make_candidates(8, 4, 9, 2, seed=1)
    with pytest.raises(RuntimeError, match="ppf_proto_topk_init.*K=65"):
        ops.proto_topk_init(torch.empty((4, 65), device="cuda"), torch.empty((4, 65), dtype=torch.int32, device="cuda"),
                            torch.empty((4, 65), dtype=torch.int32, device="cuda"))
    s = new_state(4, 3)
    with pytest.raises(ValueError, match="argmax and idx"):
        ops.proto_topk_merge(c["act"].cuda(), c["argmax"].cuda(), None, c["tok"].cuda(), 1, c["labels"].cuda(), c["ids"].cuda(), 2,
                             s["val"], s["img"], s["pos"], s["best_feat"])


# ------------------------------------------------------------------------------------------------ 3. through the model
def _batches(cfg, n=3, B=6, classes=None, seed=11):
    g = torch.Generator().manual_seed(seed)
    classes = cfg["num_classes"] if classes is None else classes
    out = []
    for i in range(n):
        x = torch.randn((B, 3, cfg["img"], cfg["img"]), generator=g).cuda()
        y = torch.randint(0, classes, (B,), generator=g).cuda()
        ids = torch.arange(100 + i * B, 100 + (i + 1) * B).flip(0)                  # unique, not ascending inside a batch
        out.append((x, y, ids))
    return out


def _capture(m, batches):
    """The referee's inputs: the tensors of the same _branches calls, concatenated on the CPU."""
    m.eval()
    rows = []
    with torch.no_grad():
        for x, y, ids in batches:
            r = m._branches(x, want_dist=False)
            rows.append(dict(f=r.f.cpu(), idx=r.idx.cpu(), act_l=r.act_max_local.cpu(), act_g=r.act_max_global.cpu(), argmax=r.argmax.cpu(), y=y.cpu(),
                             ids=ids))
    return {k: torch.cat([r[k] for r in rows]) for k in rows[0]}


@pytest.mark.parametrize("class_specific", [True, False], ids=["class", "all"])
@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_bank_update_through_the_model(fixture, class_specific):
    from protopformer_amd.bank import PrototypeBank
    sd, cfg, _ = micro(fixture)
    m = build_micro(cfg, sd)
    batches = _batches(cfg)
    bank = PrototypeBank(m, topk=3, class_specific=class_specific)
    for x, y, ids in batches:
        bank.update(x, y, ids)
    res = bank.result()
    cap = _capture(m, batches)
    for br, act, t0 in (("local", cap["act_l"], 1), ("global", cap["act_g"], 0)):
        ppc = bank.ppc[br] if class_specific else 0
        pos = torch.gather(cap["idx"].long(), 1, cap["argmax"].long()) if br == "local" else None
        val, img, gp, src = referee(act, cap["ids"], cap["y"], ppc, 3, pos)
        r = res[br]
        assert np.array_equal(r["values"].view(np.int32), val.numpy().view(np.int32)), f"{fixture} {br}: values"
        assert np.array_equal(r["image_ids"], img.numpy()) and np.array_equal(r["grid_pos"], gp.numpy()), f"{fixture} {br}: ids / positions"
        assert np.array_equal(r["filled"], (img >= 0).sum(1).numpy())
        bf = bank.state[br]["best_feat"].cpu()
        for p in range(val.shape[0]):
            n = int(src[p])
            if n >= 0:
                tok = cap["f"][n, 1 + int(cap["argmax"][n, p])] if br == "local" else cap["f"][n, 0]
                assert torch.equal(bits(bf[p]), bits(tok)), f"{fixture} {br}: best_feat[{p}]"
    assert res["local"]["grid_pos"].max() < m.num_patches
    assert (res["global"]["grid_pos"] == -1).all()
    # the bank's own state survives a save / load round trip
    other = PrototypeBank(m, topk=3, class_specific=class_specific)
    other.load_state_dict(bank.state_dict())
    again = other.result()
    assert all(np.array_equal(again[b][k], res[b][k]) for b in res for k in res[b])


def test_nearest_patches_assigns_running_ids():
    from protopformer_amd.interpret import nearest_patches
    sd, cfg, _ = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    batches = _batches(cfg)
    bank = nearest_patches(m, [(x, y) for x, y, _ in batches], topk=2, class_specific=False)
    ids = bank.result()["local"]["image_ids"]
    assert ids.min() >= 0 and ids.max() < 18 and (bank.result()["local"]["filled"] == 2).all()
    with_ids = nearest_patches(m, batches, topk=2, class_specific=False)
    got = with_ids.result()["local"]["image_ids"]
    assert got.min() >= 100 and got.max() < 118


# ------------------------------------------------------------------------------------------------ 4. projection
def test_projection():
    from protopformer_amd.bank import PrototypeBank
    from protopformer_amd.engine import FlatAdamW, train_one_step
    from protopformer_amd.protopformer import CrossEntropyLoss
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    opt = FlatAdamW(m, weight_decay=0.05)
    store = m.flat_store()
    batches = _batches(cfg, classes=cfg["num_classes"] - 2)                         # the last two classes see no image: unfilled prototypes
    bank = PrototypeBank(m, topk=3, class_specific=True)
    for x, y, ids in batches:
        bank.update(x, y, ids)
    before = bank.result()
    old = {n: getattr(m, n).detach().clone() for n in ("prototype_vectors", "prototype_vectors_global")}
    n = bank.project_(m)
    assert n == int((before["local"]["filled"] > 0).sum() + (before["global"]["filled"] > 0).sum())
    assert m.flat_store() is store and not store.bf16_fresh, "project_ must keep the flat store and invalidate its bf16 shadows"
    for br, name in (("local", "prototype_vectors"), ("global", "prototype_vectors_global")):
        new, bf = getattr(m, name).detach().reshape(bank.num[br], -1), bank.state[br]["best_feat"]
        filled = torch.from_numpy(before[br]["filled"] > 0).cuda()
        assert bool(filled.any()) and not bool(filled.all())
        assert torch.equal(bits(new[filled]), bits(bf[filled])), f"{name}: projected prototypes must equal best_feat bit for bit"
        assert torch.equal(bits(new[~filled]), bits(old[name].reshape(bank.num[br], -1)[~filled])), f"{name}: unfilled prototypes changed"
    fresh = PrototypeBank(m, topk=3, class_specific=True)
    for x, y, ids in batches:
        fresh.update(x, y, ids)
    after = fresh.result()["local"]
    b = before["local"]
    for p in np.nonzero(b["filled"] > 0)[0]:
        print(f"prototype {p}: rank 0 image {b['image_ids'][p, 0]} -> {after['image_ids'][p, 0]}, cell {b['grid_pos'][p, 0]} -> "
              f"{after['grid_pos'][p, 0]}, value {b['values'][p, 0]:.6f} -> {after['values'][p, 0]:.6f}")
    for p in np.nonzero(b["filled"] > 0)[0]:
        assert after["image_ids"][p, 0] == b["image_ids"][p, 0], f"prototype {p}: rank 0 moved to another image after projection"
        assert after["grid_pos"][p, 0] == b["grid_pos"][p, 0], f"prototype {p}: rank 0 moved to another patch after projection"
        assert after["values"][p, 0] >= b["values"][p, 0], f"prototype {p}: the projected prototype is further from its own patch"
    # a training step on the projected model: the optimizer built before the projection still owns the store
    m.train()
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    p_before = store.params.clone()
    loss, *_ = train_one_step(m, CrossEntropyLoss(), img, label, opt, epoch=20)
    assert np.isfinite(float(loss)) and not torch.equal(store.params, p_before)


# ------------------------------------------------------------------------------------------------ 5. the tool
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def _construct():
    from protopformer_amd.protopformer import construct_PPNet
    return construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200,
                           reserve_layers=[11], reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1,
                           add_on_layers_type="regular")


def test_tool_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    tree, out = str(tmp_path / "data"), str(tmp_path / "out")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = _construct().cuda()
    ck = str(tmp_path / "init.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    del m
    cmd = [sys.executable, "-m", "protopformer_amd.bank", "--data_set", "CUB2011U", "--data_path", tree, "--output_dir", out, "--resume", ck,
           "--topk", "3", "--gallery", "--project", *MODEL_FLAGS]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(os.path.join(out, "prototype_bank.npz"))
    doc = json.load(open(os.path.join(out, "prototype_bank.json")))
    assert z["local_values"].shape == (400, 3) and z["global_values"].shape == (200, 3) and doc["topk"] == 3 and doc["side"] == 14
    train_rows = {i: c - 1 for i, c, t in mini_trees.CUB_ROWS if t == 1 and i not in mini_trees.CUB_NO_LABEL}
    n_entries = 0
    for p in doc["prototypes"]:
        for e in p["entries"]:
            n_entries += 1
            assert os.path.isfile(e["image"]) and os.path.abspath(e["image"]).startswith(os.path.abspath(tree)), e
            assert e["label"] == p["class"] == train_rows[e["image_id"]], (p["branch"], p["prototype"], e)
            if p["branch"] == "local":
                assert 0 <= e["grid_row"] < 14 and 0 <= e["grid_col"] < 14 and e["box"] == [e["grid_col"] * 16, e["grid_row"] * 16,
                                                                                           e["grid_col"] * 16 + 16, e["grid_row"] * 16 + 16]
    # 4 classes with 3 training images each, 2 local + 1 global prototype per class, K = 3: every list of those classes is full
    assert n_entries == 4 * 3 * 3 and int(z["local_filled"].sum()) == 4 * 2 * 3 and int(z["global_filled"].sum()) == 4 * 3
    jpgs = [os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs if f.endswith(".jpg")]
    assert len(jpgs) == 4 * 2 * 3 and os.path.isfile(os.path.join(out, "proto_0", "rank0.jpg"))
    from PIL import Image
    assert Image.open(os.path.join(out, "proto_0", "rank0.jpg")).size == (224, 224)
    # the projected checkpoint: the reference's format and key set, loads strictly into a freshly constructed model
    saved = torch.load(os.path.join(out, "checkpoints", "projected.pth"), map_location="cpu", weights_only=False)
    assert {"model", "optimizer", "lr_scheduler", "epoch", "model_ema", "args"} <= set(saved)
    fresh = _construct()
    ref_sd, _, _ = micro("micro_deit.npz")
    head = lambda keys: {k for k in keys if not k.startswith("features.")}
    assert set(saved["model"]) == set(fresh.state_dict()) and head(saved["model"]) == head(ref_sd)
    fresh.load_state_dict(saved["model"], strict=True)
    init = torch.load(ck, map_location="cpu", weights_only=False)["model"]
    changed = (saved["model"]["prototype_vectors"] != init["prototype_vectors"]).reshape(400, -1).any(1)
    assert changed[:8].all() and not changed[8:].any(), "exactly the prototypes of the four classes with images are projected"
    assert all(torch.equal(saved["model"][k], init[k]) for k in init if not k.startswith("prototype_vectors"))
