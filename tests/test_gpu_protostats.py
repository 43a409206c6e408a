"""Prototype statistics on the GPU: ppf_proto_stats_update against the numpy referee protostats.stats_from_outputs (exact: integer
tables, np.array_equal), batching invariance and accumulation into pre-filled tables, the global branch, rejected shapes, PrototypeStats
through the micro models with a save / load in the middle, prune_, and the command-line tool on the miniature CUB tree.

The activations are multiples of 1/8 over a range of width 4, so for every bin count used here many of them lie exactly on a bin edge;
others lie below lo and above hi, and +-inf, NaN and -0.0 are planted at known places."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close, build_micro, micro

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI, GRID = 0.5, 4.5, 16
NAMES = ("hist", "nan_count", "coloc", "images", "bad")


# ------------------------------------------------------------------------------------------------ generator, device runner
def make_case(B, P, ppc, T, seed):
    rng = np.random.default_rng(seed)
    C = P // ppc
    act = (rng.integers(-4, 44, size=(B, P)) / 8.0).astype(np.float32)              # -0.5 .. 5.375 in steps of 1/8
    flat = act.reshape(-1)
    planted = {0: np.inf, 1: -np.inf, 2: np.nan, 3: -0.0, flat.size - 1: np.nan, flat.size // 2: np.inf, flat.size // 3: LO, flat.size // 5: HI}
    for pos, v in planted.items():
        flat[pos] = v
    labels = rng.integers(0, C, size=B).astype(np.int64)
    argmax = rng.integers(0, T, size=(B, P)).astype(np.int32)
    idx = np.stack([np.sort(rng.permutation(GRID)[:T]) for _ in range(B)]).astype(np.int32)
    for b in range(B):                                                                # invalid cells among the own-class prototypes
        first = int(labels[b]) * ppc
        if b % 3 == 0:
            argmax[b, first + b % ppc] = -1 if b % 2 else T
    if B >= 3:
        labels[B // 2], labels[B - 1] = -1, C                                         # both must land in bad and add nothing else
        flat_b = act[B // 2]
        flat_b[:] = np.nan                                                            # ... not even a NaN count
    return dict(act=act, argmax=argmax, idx=idx, labels=labels, ppc=ppc, T=T, B=B, P=P)


def sentinel(shape):
    return (np.arange(int(np.prod(shape)), dtype=np.int32) % 7 + 1).reshape(shape)


def new_tables(P, ppc, NB, fill):
    shapes = dict(hist=(P, 2, NB), nan_count=(P, 2), coloc=(P, ppc), images=(P // ppc,), bad=(1,))
    return {k: torch.from_numpy(sentinel(s) if fill else np.zeros(s, dtype=np.int32)).cuda() for k, s in shapes.items()}


def feed(tables, c, rows, NB, local=True):
    from protopformer_amd import ops
    from protopformer_amd.protostats import inv_width_of
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).cuda()
    ops.proto_stats_update(d(c["act"]), d(c["argmax"]) if local else None, d(c["idx"]) if local else None, d(c["labels"]), c["ppc"], LO,
                           float(inv_width_of(NB, LO, HI)), tables["hist"], tables["nan_count"], tables["coloc"] if local else None, tables["images"],
                           tables["bad"])


def host(tables):
    return {k: v.cpu().numpy() for k, v in tables.items()}


def referee(c, NB, local=True):
    from protopformer_amd.protostats import stats_from_outputs
    return stats_from_outputs(c["act"], c["argmax"] if local else None, c["idx"] if local else None, c["labels"], c["ppc"], NB, LO, HI)


# ------------------------------------------------------------------------------------------------ 1. kernel against the referee
CASES = [(37, 130, 5, 16, 9), (37, 64, 64, 16, 9), (37, 128, 64, 16, 9), (37, 130, 1, 16, 9), (1, 130, 5, 16, 9), (1024, 130, 5, 16, 9),
         (37, 130, 5, 8, 9), (37, 130, 5, 128, 9)]


@pytest.mark.parametrize("B,P,ppc,NB,T", CASES)
def test_kernel_against_referee(B, P, ppc, NB, T):
    c = make_case(B, P, ppc, T, seed=B + P + ppc + NB)
    tables = new_tables(P, ppc, NB, fill=False)
    feed(tables, c, slice(0, B), NB)
    got, want = host(tables), referee(c, NB)
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), f"B={B} P={P} ppc={ppc} NB={NB}: {k} differs from the referee"
    # the case holds what it claims to hold
    n_bad = 2 if B >= 3 else 0
    assert int(want["bad"][0]) == n_bad and int(want["images"].sum()) == B - n_bad
    assert int(want["hist"].sum()) + int(want["nan_count"].sum()) == (B - n_bad) * P
    assert int(want["nan_count"].sum()) >= 1 and int(want["hist"][:, :, 0].sum()) > 0 and int(want["hist"][:, :, NB - 1].sum()) > 0
    if B == 37:
        diag = want["coloc"][np.arange(P), np.arange(P) % ppc]
        own = want["hist"][:, 0].sum(axis=1) + want["nan_count"][:, 0]
        assert (diag <= own).all() and (diag < own).any(), "an invalid argmax must be missing from the diagonal"
        if ppc > 1:
            assert int(want["coloc"].sum()) > int(diag.sum()), "the case must hold co-located pairs off the diagonal"


# ------------------------------------------------------------------------------------------------ 2. invariance, accumulation
def test_batching_invariance_and_accumulation():
    B, P, ppc, NB, T = 37, 130, 5, 16, 9
    c = make_case(B, P, ppc, T, seed=7)
    want = referee(c, NB)
    runs = []
    for parts in ([slice(0, 37)], [slice(0, 5), slice(5, 37)], [np.arange(36, 4, -1), np.arange(4, -1, -1)]):
        tables = new_tables(P, ppc, NB, fill=True)
        for rows in parts:
            feed(tables, c, rows, NB)
        runs.append(host(tables))
    for k in NAMES:
        assert np.array_equal(runs[0][k], sentinel(want[k].shape) + want[k]), f"{k}: the launch must add to what the table held"
        assert np.array_equal(runs[0][k], runs[1][k]), f"{k}: one batch vs 5 + 32"
        assert np.array_equal(runs[0][k], runs[2][k]), f"{k}: one batch vs 32 + 5 reversed"


def test_global_branch_leaves_coloc_alone():
    B, P, ppc, NB, T = 37, 130, 5, 16, 9
    c = make_case(B, P, ppc, T, seed=9)
    tables = new_tables(P, ppc, NB, fill=True)
    feed(tables, c, slice(0, B), NB, local=False)
    got, want = host(tables), referee(c, NB, local=False)
    assert want["coloc"] is None and np.array_equal(got["coloc"], sentinel((P, ppc)))
    for k in ("hist", "nan_count", "images", "bad"):
        assert np.array_equal(got[k], sentinel(want[k].shape) + want[k]), k
    assert int(want["hist"].sum()) > 0 and int(want["nan_count"].sum()) > 0 and int(want["images"].sum()) == B - 2


def test_device_form_slices_batches_above_1024():
    """stats_from_outputs(device=True) is the kernel behind the referee's signature; 1100 samples go as 1024 + 76."""
    from protopformer_amd.protostats import stats_from_outputs
    B, P, ppc, NB, T = 1100, 64, 4, 16, 9
    c = make_case(B, P, ppc, T, seed=21)
    d = lambda a: torch.from_numpy(a).cuda()
    got = stats_from_outputs(d(c["act"]), d(c["argmax"]), d(c["idx"]), d(c["labels"]), ppc, NB, LO, HI, device=True)
    want = referee(c, NB)
    for k in NAMES:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert int(want["images"].sum()) == B - 2


# ------------------------------------------------------------------------------------------------ 3. rejected shapes
@pytest.mark.parametrize("what,B,P,ppc,NB,lo,w", [("ppc=65", 4, 130, 65, 16, LO, 4.0), ("NB=7", 4, 130, 5, 7, LO, 4.0), ("NB=129", 4, 130, 5, 129, LO, 4.0),
                                                  ("P=130", 4, 130, 4, 16, LO, 4.0), ("B=1025", 1025, 130, 5, 16, LO, 4.0),
                                                  ("lo=inf", 4, 130, 5, 16, float("inf"), 4.0), ("lo=nan", 4, 130, 5, 16, float("nan"), 4.0),
                                                  ("inv_width=0", 4, 130, 5, 16, LO, 0.0), ("inv_width=-4", 4, 130, 5, 16, LO, -4.0)])
def test_rejected_shapes_leave_the_tables_unchanged(what, B, P, ppc, NB, lo, w):
    from protopformer_amd import ops
    shapes = dict(hist=(P, 2, NB), nan_count=(P, 2), coloc=(P, ppc), images=(max(P // ppc, 1),), bad=(1,))
    tables = {k: torch.from_numpy(sentinel(s)).cuda() for k, s in shapes.items()}
    act = torch.ones((B, P), device="cuda")
    argmax, idx = torch.zeros((B, P), dtype=torch.int32, device="cuda"), torch.zeros((B, 9), dtype=torch.int32, device="cuda")
    labels = torch.zeros(B, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="ppf_proto_stats_update.*" + what.replace("+", r"\+")):
        ops.proto_stats_update(act, argmax, idx, labels, ppc, lo, w, tables["hist"], tables["nan_count"], tables["coloc"], tables["images"], tables["bad"])
    torch.cuda.synchronize()
    for k, s in shapes.items():
        assert np.array_equal(tables[k].cpu().numpy(), sentinel(s)), f"{what}: {k} changed"


def test_binding_refuses_what_the_entry_point_cannot_see():
    from protopformer_amd import ops
    t = new_tables(10, 2, 16, fill=False)
    act, lab = torch.ones((4, 10), device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    am, idx = torch.zeros((4, 10), dtype=torch.int32, device="cuda"), torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="argmax and idx"):
        ops.proto_stats_update(act, am, None, lab, 2, 0.0, 1.0, t["hist"], t["nan_count"], t["coloc"], t["images"], t["bad"])
    with pytest.raises(ValueError, match="coloc"):
        ops.proto_stats_update(act, am, idx, lab, 2, 0.0, 1.0, t["hist"], t["nan_count"], None, t["images"], t["bad"])
    with pytest.raises(ValueError, match="images"):
        ops.proto_stats_update(act, am, idx, lab, 2, 0.0, 1.0, t["hist"], t["nan_count"], t["coloc"], t["bad"], t["bad"])
    with pytest.raises(ValueError, match="label"):
        ops.proto_stats_update(act, am, idx, lab.int(), 2, 0.0, 1.0, t["hist"], t["nan_count"], t["coloc"], t["images"], t["bad"])
    assert all(int(v.abs().sum()) == 0 for v in t.values())


# ------------------------------------------------------------------------------------------------ 4. through the models
def _batches(cfg, sizes=(6, 3, 5), seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((B, 3, cfg["img"], cfg["img"]), generator=g).cuda(), torch.randint(0, cfg["num_classes"], (B,), generator=g).cuda())
            for B in sizes]


def _capture(m, batches):
    m.eval()
    rows = []
    with torch.no_grad():
        for x, y in batches:
            r = m._branches(x, want_dist=False)
            rows.append(dict(idx=r.idx.cpu(), act_l=r.act_max_local.cpu(), act_g=r.act_max_global.cpu(), argmax=r.argmax.cpu(), y=y.cpu()))
    return {k: torch.cat([r[k] for r in rows]).numpy() for k in rows[0]}


def _same(a, b):
    return all((a[br][k] is None and b[br][k] is None) or np.array_equal(a[br][k], b[br][k]) for br in ("local", "global") for k in NAMES)


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_stats_update_through_the_model(fixture):
    from protopformer_amd.protostats import PrototypeStats, stats_from_outputs
    sd, cfg, _ = micro(fixture)
    m = build_micro(cfg, sd)
    batches = _batches(cfg)
    stats = PrototypeStats(m, bins=16)
    for x, y in batches:
        stats.update(x, y)
    res = stats.result()
    cap = _capture(m, batches)
    for br, act, am, idx in (("local", cap["act_l"], cap["argmax"], cap["idx"]), ("global", cap["act_g"], None, None)):
        want = stats_from_outputs(act, am, idx, cap["y"], stats.ppc[br], 16, stats.lo, stats.hi)
        for k in NAMES:
            assert (want[k] is None and res[br][k] is None) or np.array_equal(res[br][k], want[k]), f"{fixture} {br}: {k}"
        assert int(res[br]["images"].sum()) == 14 and int(res[br]["bad"][0]) == 0
        assert int(res[br]["hist"].sum()) + int(res[br]["nan_count"].sum()) == 14 * stats.num[br]
    assert int(res["local"]["coloc"].sum()) > 0
    # a save / load between two batches changes nothing
    first = PrototypeStats(m, bins=16)
    for x, y in batches[:2]:
        first.update(x, y)
    resumed = PrototypeStats(m, bins=16)
    resumed.load_state_dict(first.state_dict())
    resumed.update(*batches[2])
    assert _same(resumed.result(), res)
    with pytest.raises(ValueError, match="bins"):
        PrototypeStats(m, bins=32).load_state_dict(first.state_dict())


# ------------------------------------------------------------------------------------------------ 5. pruning
def test_prune():
    from protopformer_amd.protostats import prune_
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd)
    store = m.flat_store()
    x = torch.from_numpy(z["img"]).cuda()
    Pl, Pg = m.num_prototypes, m.num_prototypes_global
    keep = {"local": np.arange(Pl) % 3 != 1, "global": np.arange(Pg) % 4 != 0}
    before = {"local": m.last_layer.weight.detach().clone(), "global": m.last_layer_global.weight.detach().clone()}
    dropped = prune_(m, keep)
    assert dropped == {"local": int((~keep["local"]).sum()), "global": int((~keep["global"]).sum())} and min(dropped.values()) > 0
    assert m.flat_store() is store and not store.bf16_fresh, "prune_ must keep the flat store and invalidate its bf16 shadows"
    after = {"local": m.last_layer.weight.detach(), "global": m.last_layer_global.weight.detach()}
    for br in ("local", "global"):
        k = torch.from_numpy(keep[br]).cuda()
        assert after[br].shape == before[br].shape
        assert bool((after[br][:, ~k] == 0).all()), f"{br}: the dropped columns must be exactly zero"
        assert torch.equal(after[br][:, k].view(torch.int32), before[br][:, k].view(torch.int32)), f"{br}: the kept columns must be bit-equal"
        assert bool((before[br][:, ~k] != 0).any())
    m.eval()
    with torch.no_grad():
        r = m._branches(x, want_dist=False)
        logits, act_l, act_g = r.logits, r.act_max_local, r.act_max_global
    coe = float(m.global_coe)
    wl = (before["local"] * torch.from_numpy(keep["local"]).cuda()).double().cpu()
    wg = (before["global"] * torch.from_numpy(keep["global"]).cuda()).double().cpu()
    want = coe * act_g.double().cpu() @ wg.t() + (1.0 - coe) * act_l.double().cpu() @ wl.t()
    assert_close(logits, want, rtol=1e-4, atol=1e-3, what="pruned logits")              # the bound of test_cross_entropy_and_frozen_head's product
    # the pruned state dict in an unmodified model
    fresh = build_micro(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    fresh.eval()
    with torch.no_grad():
        again = fresh._branches(x, want_dist=False).logits
    assert torch.equal(again.view(torch.int32), logits.view(torch.int32)), "the pruned checkpoint must give bit-identical logits"


# ------------------------------------------------------------------------------------------------ 6. the tools
MODEL_FLAGS = ["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1", "--reserve_layers", "11",
               "--reserve_token_nums", "81", "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "1", "--input_size", "224",
               "--batch_size", "4", "--num_workers", "0"]


def _construct():
    from protopformer_amd.protopformer import construct_PPNet
    return construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[400, 64, 1, 1], num_classes=200,
                           reserve_layers=[11], reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=1,
                           add_on_layers_type="regular")


def test_tools_on_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd import explain as explain_tool
    from protopformer_amd.engine import FlatAdamW, save_checkpoint
    tree, out = str(tmp_path / "data"), str(tmp_path / "out")
    mini_trees.build_cub(tree)
    torch.manual_seed(5)
    m = _construct().cuda()
    ck, pruned = str(tmp_path / "init.pth"), str(tmp_path / "pruned.pth")
    save_checkpoint(ck, m, FlatAdamW(m), None, 0)
    del m
    data = ["--data_set", "CUB2011U", "--data_path", tree, "--resume", ck]
    cmd = [sys.executable, "-m", "protopformer_amd.protostats", *data, "--output_dir", out, "--bins", "16", "--prune", "--save-pruned", pruned, *MODEL_FLAGS]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    npz = os.path.join(out, "prototype_stats.npz")
    z = np.load(npz)
    doc = json.load(open(os.path.join(out, "prototype_stats.json")))
    n_train = len([i for i, c, t in mini_trees.CUB_ROWS if t == 1 and i not in mini_trees.CUB_NO_LABEL])
    assert z["local_hist"].shape == (400, 2, 16) and z["global_hist"].shape == (200, 2, 16) and z["local_coloc"].shape == (400, 2)
    assert int(z["bins"]) == 16 and float(z["lo"]) == 0.0 and doc["bins"] == 16 and doc["images"] == {"local": n_train, "global": n_train}
    assert int(z["local_hist"].sum()) + int(z["local_nan_count"].sum()) == n_train * 400
    assert int(z["global_hist"].sum()) + int(z["global_nan_count"].sum()) == n_train * 200
    assert z["local_images"][:4].tolist() == [3, 3, 3, 3] and int(z["local_images"].sum()) == n_train
    assert len(doc["prototypes"]) == 600 and sum(p["own_images"] + p["other_images"] + p["nan_own"] + p["nan_other"] for p in doc["prototypes"]) == n_train * 600
    assert all(p["auroc"] is None for p in doc["prototypes"] if p["class"] >= 4) and all(p["auroc"] is not None for p in doc["prototypes"] if p["class"] < 4)
    # the keep decision, both accuracies, and the pruned checkpoint in a freshly constructed model
    pr = doc["prune"]
    assert 0.0 <= pr["acc1_before"] <= 100.0 and 0.0 <= pr["acc1_after"] <= 100.0 and pr["checkpoint"] == pruned
    keep_l, keep_g = np.array(pr["keep"]["local"]), np.array(pr["keep"]["global"])
    assert keep_l.shape == (400,) and keep_g.shape == (200,) and pr["dropped"] == {"local": int((~keep_l).sum()), "global": int((~keep_g).sum())}
    assert keep_l.reshape(200, 2).any(axis=1).all() and keep_g.all(), "min_keep = 1: every class keeps a prototype in each branch"
    assert set(pr["reasons"]["local"]) == {str(p) for p in np.nonzero(~keep_l)[0]} and pr["dropped"]["local"] >= 196
    saved = torch.load(pruned, map_location="cpu", weights_only=False)
    init = torch.load(ck, map_location="cpu", weights_only=False)["model"]
    fresh = _construct()
    fresh.load_state_dict(saved["model"], strict=True)
    wl = saved["model"]["last_layer.weight"]
    assert bool((wl[:, ~keep_l] == 0).all()) and torch.equal(wl[:, keep_l], init["last_layer.weight"][:, keep_l])
    assert all(torch.equal(saved["model"][k], init[k]) for k in init if not k.startswith("last_layer"))
    # explain on the same tree: --stats adds the two percentiles and nothing else
    lines = {}
    for tag, extra in (("plain", []), ("stats", ["--stats", npz])):
        args = explain_tool.get_args_parser().parse_args([*data, "--output_dir", str(tmp_path / tag), "--topk", "3", "--max_images", "6", *extra, *MODEL_FLAGS])
        lines[tag] = [json.loads(l) for l in open(explain_tool.main(args))]
    assert len(lines["plain"]) == len(lines["stats"]) == 6
    seen = 0
    for rec in lines["stats"]:
        for c in rec["classes"]:
            for br in ("local", "global"):
                for e in c[br]["prototypes"]:
                    pa, po = e.pop("percentile_all"), e.pop("percentile_own")
                    # the explained images are among the recorded ones: their own bin is never empty; a class may have no image at all
                    assert 0.0 < pa < 1.0 and (np.isnan(po) or 0.0 <= po <= 1.0), (pa, po, e)
                    seen += 1
    assert seen == 6 * 2 * 3 and not any("percentile_all" in json.dumps(r) for r in lines["plain"])
    assert json.dumps(lines["stats"]) == json.dumps(lines["plain"]), "without the new keys the two runs must be identical"
