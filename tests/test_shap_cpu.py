"""The numpy referees of the KernelSHAP pass (interpret.shap_* with device=False) held to the contract of include/ppf_hip.h, the refusals
of kernel_shap, and the order tuples of the faithfulness test.  No GPU: the kernels are held to these referees in tests/test_gpu_shap.py."""
import types

import numpy as np
import pytest
import torch

IDS = np.array([5, (1 << 40) + 3, 0], dtype=np.int64)


def coalitions(ids, s, N, seed=0):
    from protopformer_amd.interpret import shap_coalitions_from_ids
    return shap_coalitions_from_ids(ids, s, N, seed, device=False)


@pytest.mark.parametrize("d", [4, 9, 16, 49, 196])
def test_size_table_is_the_shapley_kernels_distribution(d):
    from protopformer_amd.interpret import shap_size_table
    t = shap_size_table(d)
    assert t.dtype == np.int32 and t.shape == (d - 1,)
    assert (np.diff(t.astype(np.int64)) >= 0).all() and t[-1] == 1 << 24 and t[0] > 0
    w = 1.0 / (np.arange(1, d) * (d - np.arange(1, d)))
    assert np.abs(t - np.cumsum(w) / w.sum() * 2.0 ** 24).max() <= 0.5 + 2.0 ** -20           # round to nearest of the fp64 form
    for bad in (3, 197):
        with pytest.raises(ValueError, match="outside"):
            shap_size_table(bad)


@pytest.mark.parametrize("s,N", [(2, 2), (2, 16), (4, 64), (7, 10), (14, 6), (3, 400)])
def test_coalitions_sizes_complements_and_popcounts(s, N):
    from protopformer_amd.interpret import philox4x32_10, shap_members, shap_size_table
    d, seed = s * s, (1 << 35) + 11
    coal = coalitions(IDS, s, N, seed)
    assert coal.dtype == np.uint32 and coal.shape == (3, N, (d + 31) // 32)
    z = shap_members(coal, s)
    assert z.shape == (3, N, d) and (z[:, 0::2] != z[:, 1::2]).all(), "odd coalitions must be the exact complements of the even ones"
    # unused bits are zero: packing the unpacked bits again gives the words back
    again = np.zeros(coal.shape[:2] + (coal.shape[2] * 32,), dtype=np.uint64)
    again[..., :d] = z
    assert np.array_equal((again.reshape(coal.shape + (32,)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32), coal)
    # the drawn size, from the contract's words: call 0xFFFFFFFF of pair j, u = w.x >> 8, size = 1 + #{t <= d - 3 : table[t] <= u}
    table = shap_size_table(d).astype(np.int64)
    for b, i in enumerate(IDS.astype(np.uint64)):
        ctr = np.array([[0xFFFFFFFF, 0x80000001 + j, int(i) & 0xFFFFFFFF, int(i) >> 32] for j in range(N // 2)], dtype=np.uint64)
        u = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))[:, 0] >> np.uint32(8)
        size = 1 + (table[None, :d - 2] <= u.astype(np.int64)[:, None]).sum(1)
        assert ((size >= 1) & (size <= d - 1)).all()
        assert np.array_equal(z[b, 0::2].sum(-1), size), "the popcount of an even coalition is its drawn size"
        assert np.array_equal(z[b, 1::2].sum(-1), d - size)


def test_members_are_the_smallest_keys_and_sizes_follow_the_table():
    from protopformer_amd.interpret import philox4x32_10, shap_members, shap_size_table
    s, N, seed = 3, 2000, 9
    d = s * s
    z = shap_members(coalitions(IDS[:1], s, N, seed), s)[0, 0::2]                                # [1000, 9]
    ctr = np.array([[[k, 0x80000001 + j, 5, 0] for k in range(3)] for j in range(N // 2)], dtype=np.uint64)
    keys = philox4x32_10(ctr, np.array([seed, 0], dtype=np.uint64)).reshape(N // 2, 12)[:, :d]    # word q % 4 of call q / 4
    for j in range(0, N // 2, 37):
        order = sorted(range(d), key=lambda q: (int(keys[j, q]), q))
        assert set(np.nonzero(z[j])[0]) == set(order[: int(z[j].sum())])
    # the empirical size distribution against the table's, 1000 draws: each frequency within 5 standard deviations
    p = np.diff(np.concatenate([[0], shap_size_table(d)])) / 2.0 ** 24
    freq = np.bincount(z.sum(-1), minlength=d)[1:d] / (N // 2)
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / (N // 2))).all(), (freq, p)
    # every player is held about half the time (paired sampling makes it exactly half over a pair)
    both = shap_members(coalitions(IDS[:1], s, N, seed), s)[0]
    assert (both.sum(0) == N // 2).all()


def test_a_coalition_depends_on_the_id_not_on_the_batch_place():
    a = coalitions(IDS, 4, 32, seed=3)
    b = coalitions(IDS[::-1].copy(), 4, 32, seed=3)
    assert np.array_equal(a, b[::-1])
    assert np.array_equal(coalitions(IDS[1:2], 4, 32, seed=3)[0], a[1]), "ids above 2^40"
    assert not np.array_equal(a[1], coalitions(np.array([3], dtype=np.int64), 4, 32, seed=3)[0]), "the high word of the id must enter"
    assert not np.array_equal(a, coalitions(IDS, 4, 32, seed=4))
    assert np.array_equal(coalitions(IDS, 4, 64, seed=3)[:, :32], a), "a coalition does not depend on the number of samples"
    for bad_s, bad_n, word in ((1, 8, "cells"), (15, 8, "cells"), (4, 7, "samples"), (4, 0, "samples")):
        with pytest.raises(ValueError, match=word):
            coalitions(IDS, bad_s, bad_n)


@pytest.mark.parametrize("s,N,M", [(2, 2, 1), (4, 64, 3), (7, 66, 8)])
def test_gram_is_ZtZ_and_bvec_the_ascending_selected_sum(s, N, M):
    from protopformer_amd.interpret import shap_gram, shap_members
    rng = np.random.default_rng(s + N)
    coal = coalitions(IDS[:2], s, N, seed=1)
    z = shap_members(coal, s)
    val, v0 = rng.standard_normal((N, 2, M)).astype(np.float32), rng.standard_normal((2, M)).astype(np.float32)
    A, bvec = shap_gram(coal, val, v0, s, device=False)
    assert A.dtype == np.int32 and bvec.dtype == np.float64 and A.shape == (2, s * s, s * s) and bvec.shape == (2, M, s * s)
    for b in range(2):
        Z = z[b].astype(np.int64)
        assert np.array_equal(A[b], Z.T @ Z)
        for m in range(M):
            for i in range(0, s * s, 5):
                acc = 0.0
                for n in range(N):
                    if z[b, n, i]:
                        acc = acc + (float(val[n, b, m]) - float(v0[b, m]))
                assert acc == bvec[b, m, i]


@pytest.mark.parametrize("s,N,G", [(2, 16, 16), (4, 64, 16), (7, 512, 196), (14, 2048, 196)])
def test_solve_recovers_the_weights_of_an_additive_game(s, N, G):
    from protopformer_amd.interpret import shap_gram, shap_members, shap_solve
    rng = np.random.default_rng(N)
    d, B, M = s * s, 2, 2
    coal = coalitions(IDS[:B], s, N, seed=2)
    z = shap_members(coal, s).astype(np.float64)
    # values that fp32 holds exactly: weights and v0 on a grid of 2^-10, so the game is additive to the last bit
    w = np.round(rng.standard_normal((B, M, d)) * 64) / 1024
    v0 = (np.round(rng.standard_normal((B, M)) * 64) / 1024).astype(np.float32)
    val = (v0.astype(np.float64)[None] + np.einsum("bnd,bmd->nbm", z, w)).astype(np.float32)
    v1 = (v0.astype(np.float64) + w.sum(-1)).astype(np.float32)
    A, bvec = shap_gram(coal, val, v0, s, device=False)
    phi, cell, bad = shap_solve(A, bvec, v0, v1, s, G, device=False)
    assert not bad.any() and phi.shape == (B, M, d) and cell.shape == (B, M, G) and cell.dtype == np.float32
    E = d * max(np.linalg.cond(A[b].astype(np.float64)) for b in range(B)) * 2.0 ** -52 * np.abs(w).max()
    assert np.abs(phi - w).max() <= E, (np.abs(phi - w).max(), E)
    assert np.abs(phi.sum(-1) - w.sum(-1)).max() <= d * E
    side, r = int(G ** 0.5), int(G ** 0.5) // s
    g = np.arange(G)
    player = (g // side // r) * s + (g % side) // r
    assert np.array_equal(cell.view(np.int32), (phi[:, :, player] / float(r * r)).astype(np.float32).view(np.int32))
    assert np.allclose(cell.astype(np.float64).sum(-1), phi.sum(-1), rtol=0, atol=G * 2.0 ** -24 * np.abs(phi).max())


def test_solve_marks_singular_images_and_nan_rows_alone():
    from protopformer_amd.interpret import shap_gram, shap_solve
    rng = np.random.default_rng(0)
    s, M = 2, 2
    few, many = coalitions(IDS[:1], s, 2), coalitions(IDS[:1], s, 32)
    val = rng.standard_normal((32, 1, M)).astype(np.float32)
    v0, v1 = np.zeros((1, M), dtype=np.float32), np.ones((1, M), dtype=np.float32)
    phi, cell, bad = shap_solve(*shap_gram(few, val[:2], v0, s, device=False), v0, v1, s, 16, device=False)
    assert bad.tolist() == [1] and np.isnan(phi).all() and np.isnan(cell).all()                   # two samples cannot determine four players
    val[7, 0, 1] = np.nan
    phi, cell, bad = shap_solve(*shap_gram(many, val, v0, s, device=False), v0, v1, s, 16, device=False)
    assert bad.tolist() == [0] and np.isnan(phi[0, 1]).all() and np.isnan(cell[0, 1]).all() and np.isfinite(phi[0, 0]).all()


def test_apply_selects_x_inside_the_coalition():
    from protopformer_amd.interpret import shap_apply, shap_members
    rng = np.random.default_rng(3)
    s, N, H = 2, 6, 32
    coal = coalitions(IDS[:2], s, N)
    z = shap_members(coal, s)
    x, base = rng.standard_normal((2, 3, H, H)).astype(np.float32), rng.standard_normal((2, 3, H, H)).astype(np.float32)
    out = shap_apply(x, coal, s, 1, 4, base, device=False)
    assert out.shape == (4, 2, 3, H, H)
    for k in range(4):
        for b in range(2):
            for q in range(4):
                ys, xs = slice((q // 2) * 16, (q // 2) * 16 + 16), slice((q % 2) * 16, (q % 2) * 16 + 16)
                want = x if z[b, 1 + k, q] else base
                assert np.array_equal(out[k, b, :, ys, xs], want[b, :, ys, xs])
    both = shap_apply(x, coal, s, baseline=0.25, device=False)
    assert np.array_equal(np.where(both[0::2] == 0.25, both[1::2], both[0::2]), np.broadcast_to(x, (3,) + x.shape)), "a pair covers the image once"
    with pytest.raises(ValueError, match="outside"):
        shap_apply(x, coal, s, 4, 3, device=False)
    with pytest.raises(ValueError, match="multiple of 4"):
        shap_apply(x[:, :, :30, :30], coal, s, device=False)


def test_kernel_shap_refuses_by_name_before_anything_runs():
    from protopformer_amd.interpret import SHAP_DEFAULTS, Shap, kernel_shap
    assert SHAP_DEFAULTS == dict(samples=512, cells=7, value="prob")
    net = types.SimpleNamespace(num_patches=16)                                                   # nothing of a model is touched before the refusals
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernel_shap(net, x, samples=16, cells=2)
    with pytest.raises(ValueError, match="samples=17 must be even"):
        kernel_shap(net, x, samples=17, cells=2)
    with pytest.raises(ValueError, match=r"samples=14 is below 4 \* cells\^2 = 16"):
        kernel_shap(net, x, samples=14, cells=2)
    with pytest.raises(ValueError, match="cells=3 does not divide the grid side 4"):
        kernel_shap(net, x, samples=64, cells=3)
    with pytest.raises(ValueError, match="value must be one of"):
        kernel_shap(net, x, samples=16, cells=2, value="margin")
    assert Shap.FIELDS == ("phi", "cell", "value", "value_base", "value_full", "gram", "bvec", "bad", "classes", "coal") and set(Shap.META) == {"cells", "kind"}
    r = Shap(np.ones((1, 1, 4)), None, None, np.array([[0.5]], dtype=np.float32), np.array([[4.25]], dtype=np.float32), None, None, None, None, None, 2, "prob")
    assert r.delta().tolist() == [[0.25]]


def test_order_tuples_and_the_tools_flags():
    from protopformer_amd import faithfulness as tool
    from protopformer_amd.interpret import EXTRA_ORDERS, GAME_ORDERS, GRADIENT_ORDERS, ORDER_MODES, Faithfulness
    assert ORDER_MODES == ("evidence", "attention", "random") and EXTRA_ORDERS == ("rise",) and GRADIENT_ORDERS == ("ig",) and GAME_ORDERS == ("shap",)
    assert Faithfulness.META["shap"] is None and Faithfulness.DEFAULTS["shap"] is None
    f = Faithfulness({}, None, None, None, None, None, 16)
    assert f.shap is None and f.rise is None and f.ig is None and f.resolution == "cell"
    p = tool.get_args_parser()
    need = ["--data_set", "CUB2011U", "--data_path", "x", "--output_dir", "y"]
    a = p.parse_args(need)
    assert a.orders == ["evidence", "attention", "random"] and (a.shap_samples, a.shap_cells, a.shap_value) == (512, 7, "prob")
    a = p.parse_args(need + ["--orders", "evidence", "shap", "--shap_samples", "16", "--shap_cells", "2", "--shap_value", "logit"])
    assert a.orders == ["evidence", "shap"] and (a.shap_samples, a.shap_cells, a.shap_value) == (16, 2, "logit")
