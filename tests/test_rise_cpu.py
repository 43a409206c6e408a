"""CPU-side checks of the RISE saliency pass: ppf_rise_nodes, ppf_rise_apply and ppf_rise_accumulate are declared once, exported and bound
with one parameter list each and answer their limits through the error channel, naming the offending value, before any device call;
the numpy referees (interpret.rise_nodes_from_ids / rise_masks / rise_apply / rise_accumulate with device=False) keep the properties of
the mask contract in include/ppf_hip.h; the faithfulness tool's parser takes the 'rise' order and its three flags and keeps its defaults."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_rise_nodes": "pLiiiiipps", "ppf_rise_apply": "pppiiiipfiiiips", "ppf_rise_accumulate": "pppiiiiiiiipps"}


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(SPECS))
def test_declared_once_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = re.findall(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert len(found) == 1, f"{name} is declared {len(found)} times in include/ppf_hip.h"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    nargs = len([a for a in found[0].split(",") if a.strip()])
    assert nargs == len(SPECS[name]) and _lib.SIGS[name] == SPECS[name]
    assert lib.ppf_abi_version() == 10 == _lib.EXPECTED_ABI          # additions: no existing entry point changed
    hip = open(os.path.join(ROOT, "protopformer_amd", "csrc", "rise.hip")).read()
    assert len(re.findall(r"^int " + name + r"\(", hip, flags=re.M)) == 1 and "<<<" not in hip and "ppf_launch<" in hip


def _fn(lib, name):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn


D = 4096                                                              # an aligned non-null address, never dereferenced on a rejected shape
FULL = 1 << 24


def _nodes(lib, ids=D, thr=FULL // 2, B=2, N=8, s=7, H=224, nodes=D, shift=D):
    return _fn(lib, "ppf_rise_nodes")(ids, 0, thr, B, N, s, H, nodes, shift, None)


def _apply(lib, x=D, nodes=D, shift=D, N=8, n0=0, Nc=4, s=7, B=2, Cc=3, H=224, W=224, out=D):
    return _fn(lib, "ppf_rise_apply")(x, nodes, shift, N, n0, Nc, s, None, 0.0, B, Cc, H, W, out, None)


def _acc(lib, nodes=D, shift=D, prob=D, B=2, N=8, M=2, s=7, thr=FULL // 2, H=224, W=224, G=196, sal=D, cell=D):
    return _fn(lib, "ppf_rise_accumulate")(nodes, shift, prob, B, N, M, s, thr, H, W, G, sal, cell, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_nodes, dict(s=0), -1, "s=0"), (_nodes, dict(s=15), -1, "s=15"), (_nodes, dict(N=0), -1, "N=0"), (_nodes, dict(thr=0), -3, "thr=0"),
    (_nodes, dict(thr=FULL + 1), -3, f"thr={FULL + 1}"), (_nodes, dict(B=0), -1, "B=0"), (_nodes, dict(H=8192, s=1), -1, "c=8192"),
    (_nodes, dict(ids=None), -3, "null pointer"), (_nodes, dict(nodes=None), -3, "null pointer"), (_nodes, dict(shift=None), -3, "null pointer"),
    (_apply, dict(s=0), -1, "s=0"), (_apply, dict(s=15), -1, "s=15"), (_apply, dict(H=224, W=220), -1, "W=220"), (_apply, dict(H=30, W=30), -1, "W=30"),
    (_apply, dict(N=0), -1, "N=0"), (_apply, dict(n0=6, Nc=4), -1, "n0=6"), (_apply, dict(Nc=0), -1, "Nc=0"), (_apply, dict(n0=-1), -1, "n0=-1"),
    (_apply, dict(Cc=0), -1, "Cc=0"), (_apply, dict(x=D + 4), -2, "16-byte"), (_apply, dict(out=D + 8), -2, "16-byte"),
    (_apply, dict(x=None), -3, "null pointer"), (_apply, dict(nodes=None), -3, "null pointer"), (_apply, dict(shift=None), -3, "null pointer"),
    (_apply, dict(out=None), -3, "null pointer"),
    (_acc, dict(s=0), -1, "s=0"), (_acc, dict(s=15), -1, "s=15"), (_acc, dict(H=224, W=220), -1, "W=220"), (_acc, dict(H=30, W=30), -1, "H=30"),
    (_acc, dict(N=0), -1, "N=0"), (_acc, dict(thr=0), -3, "thr=0"), (_acc, dict(thr=FULL + 1), -3, f"thr={FULL + 1}"), (_acc, dict(M=9), -1, "M=9"),
    (_acc, dict(M=0), -1, "M=0"), (_acc, dict(G=15), -1, "G=15"), (_acc, dict(G=25), -1, "side 5"), (_acc, dict(G=1600, H=160, W=160), -1, "G=1600"),
    (_acc, dict(H=4096, W=4096, s=1, G=1), -1, "2^29"), (_acc, dict(sal=D + 4), -2, "16-byte"),
    (_acc, dict(nodes=None), -3, "null pointer"), (_acc, dict(prob=None), -3, "null pointer"), (_acc, dict(cell=None), -3, "null pointer")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_rise_"), msg


# ------------------------------------------------------------------------------------------------ the referees
SHAPES = [(64, 2), (64, 4), (224, 7), (32, 3), (56, 14)]               # (H, s): c = 32, 16, 32, 11 (no multiple of 4), 4


def _tables(ids, H, s, N=6, p=0.5, seed=0):
    from protopformer_amd.interpret import rise_nodes_from_ids
    return rise_nodes_from_ids(np.asarray(ids, dtype=np.int64), H, N, s, p, seed, device=False)


def test_threshold_is_the_rounded_probability():
    from protopformer_amd.interpret import rise_threshold
    assert (rise_threshold(0.5), rise_threshold(1.0), rise_threshold(2.0 ** -24), rise_threshold(0.1)) == (1 << 23, 1 << 24, 1, 1677722)
    for bad in (0.0, 1.0 + 2.0 ** -20, -0.5):
        with pytest.raises(ValueError, match="thr="):
            rise_threshold(bad)


def test_nodes_depend_on_seed_image_and_mask_alone():
    from protopformer_amd.interpret import philox4x32_10
    big = (1 << 32) + 7
    a_nodes, a_shift = _tables([5, big, 0], 32, 3, seed=9)
    assert a_nodes.shape == (3, 6, 25) and a_nodes.dtype == np.uint8 and a_shift.shape == (3, 6, 2) and a_shift.dtype == np.int32
    assert set(np.unique(a_nodes).tolist()) == {0, 1}
    b_nodes, b_shift = _tables([big, 9, 9, 5], 32, 3, seed=9)                                  # another batch, other positions
    assert np.array_equal(a_nodes[1], b_nodes[0]) and np.array_equal(a_shift[1], b_shift[0])
    assert np.array_equal(a_nodes[0], b_nodes[3]) and np.array_equal(a_shift[0], b_shift[3])
    assert np.array_equal(b_nodes[1], b_nodes[2]) and not np.array_equal(a_nodes[0], a_nodes[1])
    assert not np.array_equal(_tables([big], 32, 3, seed=9)[0], _tables([big & 0xFFFFFFFF], 32, 3, seed=9)[0])     # the high word enters
    more = _tables([5, big, 0], 32, 3, N=9, seed=9)
    assert np.array_equal(more[0][:, :6], a_nodes) and np.array_equal(more[1][:, :6], a_shift)  # mask n does not depend on N
    assert not np.array_equal(_tables([5, big, 0], 32, 3, seed=10)[0], a_nodes)
    assert not np.array_equal(_tables([5, big, 0], 32, 3, seed=9 + (1 << 32))[0], a_nodes)      # the seed's high word enters
    # the contract, word for word: node q of mask n is bit (word[q % 4] of call q / 4) >> 8 < thr; the shift is call 0xFFFFFFFF
    key = np.array([9, 0], dtype=np.uint64)
    w = philox4x32_10(np.array([17 // 4, 1 + 4, big & 0xFFFFFFFF, big >> 32], dtype=np.uint64), key)
    assert a_nodes[1, 4, 17] == int((int(w[17 % 4]) >> 8) < (1 << 23))
    w = philox4x32_10(np.array([0xFFFFFFFF, 1 + 4, big & 0xFFFFFFFF, big >> 32], dtype=np.uint64), key)
    assert a_shift[1, 4].tolist() == [((int(w[0]) >> 8) * 11) >> 24, ((int(w[1]) >> 8) * 11) >> 24]


@pytest.mark.parametrize("H,s", SHAPES)
def test_mask_numerators_keep_the_contract(H, s):
    from protopformer_amd.interpret import rise_apply, rise_masks
    c = -(-H // s)
    nodes, shift = _tables([3, 1 << 40], H, s, N=12, seed=H)
    assert (shift >= 0).all() and (shift < c).all() and len(np.unique(shift)) > 1
    K = rise_masks(nodes, shift, H, s)
    assert K.shape == (2, 12, H, H) and K.dtype == np.int32 and K.min() >= 0 and K.max() <= c * c
    # the definition, pixel by pixel, on a sample of pixels
    rng = np.random.default_rng(s)
    g = nodes.reshape(2, 12, s + 2, s + 2).astype(np.int64)
    for b, n, y, x in zip(rng.integers(0, 2, 40), rng.integers(0, 12, 40), rng.integers(0, H, 40), rng.integers(0, H, 40)):
        uy, ux = y + shift[b, n, 0], x + shift[b, n, 1]
        i, ry, j, rx = uy // c, uy % c, ux // c, ux % c
        assert i + 1 <= s + 1 and j + 1 <= s + 1
        want = (c - ry) * ((c - rx) * g[b, n, i, j] + rx * g[b, n, i, j + 1]) + ry * ((c - rx) * g[b, n, i + 1, j] + rx * g[b, n, i + 1, j + 1])
        assert K[b, n, y, x] == want
    # every node on: K == c^2 everywhere and apply returns x, whatever the baseline
    full, sh = _tables([3, 1 << 40], H, s, N=3, p=1.0, seed=H)
    assert full.min() == 1 and (rise_masks(full, sh, H, s) == c * c).all()
    x = rng.standard_normal((2, 3, H, H)).astype(np.float32)
    out = rise_apply(x, full, sh, s, baseline=rng.standard_normal(x.shape).astype(np.float32), device=False)
    assert out.shape == (3, 2, 3, H, H) and out.dtype == np.float32 and all(np.array_equal(o, x) for o in out)


def test_apply_referee_blends_with_one_rounding_per_operation():
    from protopformer_amd.interpret import rise_apply, rise_masks
    H, s, c = 32, 3, 11
    nodes, shift = _tables([8, 2], H, s, N=5, seed=4)
    rng = np.random.default_rng(0)
    x, base = rng.standard_normal((2, 2, H, H)).astype(np.float32), rng.standard_normal((2, 2, H, H)).astype(np.float32)
    out = rise_apply(x, nodes, shift, s, n0=1, count=3, baseline=base, device=False)
    m = (rise_masks(nodes, shift, H, s)[:, 1:4].astype(np.float32) / np.float32(c * c)).transpose(1, 0, 2, 3)[:, :, None]
    assert out.shape == (3, 2, 2, H, H)
    assert np.array_equal(out, (m * x[None]).astype(np.float32) + ((np.float32(1) - m).astype(np.float32) * base[None]).astype(np.float32))
    const = rise_apply(x, nodes, shift, s, n0=4, baseline=-0.375, device=False)              # to the last mask
    assert const.shape == (1, 2, 2, H, H) and np.array_equal(const, rise_apply(x, nodes, shift, s, 4, 1, np.full_like(x, -0.375), device=False))
    for bad in (dict(n0=5), dict(n0=3, count=3), dict(n0=-1, count=1)):
        with pytest.raises(ValueError, match="outside"):
            rise_apply(x, nodes, shift, s, baseline=0.0, device=False, **bad)


@pytest.mark.parametrize("H,s,G", [(32, 3, 64), (64, 4, 16), (64, 2, 16), (224, 7, 196)])
def test_accumulate_referee_identities(H, s, G):
    from protopformer_amd.interpret import rise_accumulate, rise_masks, rise_threshold
    c, side, p, N = -(-H // s), int(G ** 0.5), 0.375, 5
    patch = H // side
    nodes, shift = _tables([4, 1 << 33], H, s, N=N, p=p, seed=G)
    K = rise_masks(nodes, shift, H, s).astype(np.int64)
    ones = np.ones((N, 2, 2), dtype=np.float32)
    sal, cell = rise_accumulate(nodes, shift, ones, H, s, G, p, device=False)
    assert sal.shape == (2, 2, H, H) and cell.shape == (2, 2, G) and sal.dtype == cell.dtype == np.float32
    keep = rise_threshold(p) / 2.0 ** 24
    mean_mask = K.sum(1) / (N * c * c)                                                           # exact in fp64: integers below 2^53
    assert np.array_equal(sal[:, 0], (mean_mask / keep).astype(np.float32)) and np.array_equal(sal[:, 0], sal[:, 1])
    W = K.reshape(2, N, side, patch, side, patch).sum((3, 5)).reshape(2, N, G)                   # W == K summed over the cell
    for b, n, g in ((0, 0, 0), (1, N - 1, G - 1), (1, 2, G // 2)):
        gy, gx = divmod(g, side)
        assert W[b, n, g] == K[b, n, gy * patch:(gy + 1) * patch, gx * patch:(gx + 1) * patch].sum()
    assert W.max() <= patch * patch * c * c
    assert np.array_equal(cell[:, 0], (W.sum(1) / (N * keep * c * c * patch * patch)).astype(np.float32))
    # the fp64 sum runs over n ascending, one rounding at the end; a NaN probability makes its row NaN, and only that row
    prob = np.random.default_rng(G).random((N, 2, 2)).astype(np.float32)
    sal, cell = rise_accumulate(nodes, shift, prob, H, s, G, p, device=False)
    acc = np.zeros((H, H))
    for n in range(N):
        acc = acc + float(prob[n, 1, 0]) * K[1, n].astype(np.float64)
    assert np.array_equal(sal[1, 0], (acc / (N * keep * (c * c))).astype(np.float32))
    prob[2, 0, 1] = np.nan
    sal2, cell2 = rise_accumulate(nodes, shift, prob, H, s, G, p, device=False)
    assert np.isnan(sal2[0, 1]).all() and np.isnan(cell2[0, 1]).all()
    rest = np.ones((2, 2), dtype=bool)
    rest[0, 1] = False
    assert np.array_equal(sal2[rest], sal[rest]) and np.array_equal(cell2[rest], cell[rest])


def test_a_planted_scorer_is_found():
    """The scorer is the mean mask value inside a box: the saliency is larger inside the box than outside it."""
    from protopformer_amd.interpret import rise_accumulate, rise_masks
    H, s, G, N = 64, 4, 16, 200
    c = 16
    nodes, shift = _tables([1, 2], H, s, N=N, seed=2)
    K = rise_masks(nodes, shift, H, s)
    box = np.zeros((H, H), dtype=bool)
    box[8:28, 36:60] = True
    prob = (K[:, :, box].mean(-1) / (c * c)).astype(np.float32).T[:, :, None]                    # [N, B, 1]
    sal, cell = rise_accumulate(nodes, shift, prob, H, s, G, 0.5, device=False)
    for b in range(2):
        assert sal[b, 0][box].mean() > sal[b, 0][~box].mean() * 1.05
        peak = np.unravel_index(sal[b, 0].argmax(), (H, H))
        assert box[peak], peak
    assert int(cell[0, 0].argmax()) in (2, 3, 6, 7)                                              # the cells the box covers


def test_referees_refuse_what_the_kernels_refuse():
    from protopformer_amd.interpret import rise_accumulate, rise_masks, rise_nodes_from_ids
    for kw in (dict(size=64, cells=0), dict(size=64, cells=15), dict(size=30, cells=3), dict(size=64, cells=3, masks=0)):
        with pytest.raises(ValueError, match="rise"):
            rise_nodes_from_ids(np.arange(2), device=False, **{"masks": 4, **kw})
    nodes, shift = _tables([0], 64, 4)
    with pytest.raises(ValueError, match="shifts outside"):
        rise_masks(nodes, shift + 16, 64, 4)
    for kw in (dict(grid_cells=15), dict(grid_cells=9)):
        with pytest.raises(ValueError, match="square grid whose side divides"):
            rise_accumulate(nodes, shift, np.ones((6, 1, 1), dtype=np.float32), 64, 4, device=False, **kw)
    with pytest.raises(ValueError, match=r"M=9"):
        rise_accumulate(nodes, shift, np.ones((6, 1, 9), dtype=np.float32), 64, 4, 16, device=False)


def test_rise_saliency_has_no_cpu_fallback():
    import torch
    from protopformer_amd.interpret import EXTRA_ORDERS, ORDER_MODES, rise_saliency
    assert ORDER_MODES == ("evidence", "attention", "random") and EXTRA_ORDERS == ("rise",)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rise_saliency(None, torch.zeros(1, 3, 64, 64))


def test_result_object_on_the_host():
    from protopformer_amd.interpret import Rise
    r = Rise(np.zeros((1, 1, 4, 4), np.float32), np.zeros((1, 1, 4), np.float32), np.zeros((2, 1, 1), np.float32), np.zeros((1, 2, 2), np.int32),
             np.zeros((1, 1), np.int32), np.zeros((1, 2, 9), np.uint8), 1, 0.5)
    assert r.on_host and r.cpu() is r and (r.cells, r.p) == (1, 0.5)


# ------------------------------------------------------------------------------------------------ the tool's parser
def test_tool_parser_takes_the_rise_order_and_keeps_its_defaults():
    from protopformer_amd.faithfulness import get_args_parser
    a = get_args_parser().parse_args([])
    assert a.orders == ["evidence", "attention", "random"] and (a.rise_masks, a.rise_cells, a.rise_p) == (512, 7, 0.5)
    a = get_args_parser().parse_args(["--orders", "evidence", "random", "rise", "--rise_masks", "8", "--rise_cells", "4", "--rise_p", "0.25"])
    assert a.orders == ["evidence", "random", "rise"] and (a.rise_masks, a.rise_cells, a.rise_p) == (8, 4, 0.25)
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--orders", "occlusion"])
