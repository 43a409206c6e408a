"""CPU-side checks of the per-pixel faithfulness pass: the four entry points of csrc/pixel_faithful.hip are declared, exported and bound
and answer their limits through the error channel before any device call; the numpy referees of interpret.py keep their contracts (the
pixel order against a brute-force count, the blur against an fp64 direct 2-D convolution, the perturbation identities); the taps, the
default counts and the tool's parser give known answers; tests/pixel_key_check.cpp, a stand-alone host program built under
AddressSanitizer + UBSan, checks the composite key of the order."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_order_keys_cpu import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_pixel_order": "ppiippzs", "ppf_pixel_random": "pLiips", "ppf_pixel_perturb": "pppiipfiiiiips", "ppf_gauss_blur": "ppiiiips",
         "ppf_pixel_order_scratch_bytes": "ii"}


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(SPECS))
def test_declared_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppf_hip.h"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    assert _lib.SIGS[name] == SPECS[name]
    assert lib.ppf_abi_version() == 10 == _lib.EXPECTED_ABI          # additions: no existing entry point changed


def _fn(lib, name, restype=ctypes.c_int):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn


D = 4096                                                              # an aligned non-null address, never dereferenced on a rejected shape


def _order(lib, R=2, n=64, scratch=D, nbytes=1 << 40):
    return _fn(lib, "ppf_pixel_order")(D, D, R, n, D, scratch, nbytes, None)


def _random(lib, B=2, n=64):
    return _fn(lib, "ppf_pixel_random")(D, 0, B, n, D, None)


def _perturb(lib, S=3, insertion=0, B=2, M=1, Cc=3, H=8, W=8, x=D, rank=D):
    return _fn(lib, "ppf_pixel_perturb")(x, rank, D, S, insertion, None, 0.0, B, M, Cc, H, W, D, None)


def _blur(lib, r=5, R=3, H=8, W=8, out=2 * D):
    return _fn(lib, "ppf_gauss_blur")(D, D, r, R, H, W, out, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_order, dict(n=0), -1, "n=0"), (_order, dict(n=65537), -1, "n=65537"), (_order, dict(R=0), -1, "R=0"), (_order, dict(nbytes=2047), -3, "2048"),
    (_order, dict(scratch=None), -3, "null"), (_order, dict(scratch=D + 2), -2, "4-byte"),
    (_random, dict(B=0), -1, "B=0"), (_random, dict(n=65537), -1, "n=65537"),
    (_perturb, dict(W=10), -1, "multiple of 4"), (_perturb, dict(W=0), -1, "W=0"), (_perturb, dict(M=9), -1, "M=9"), (_perturb, dict(M=0), -1, "M=0"),
    (_perturb, dict(S=0), -1, "S=0"), (_perturb, dict(insertion=2), -3, "insertion=2"), (_perturb, dict(x=D + 4), -2, "16-byte"),
    (_perturb, dict(rank=D + 8), -2, "16-byte"),
    (_blur, dict(r=0), -1, "r=0"), (_blur, dict(r=17), -1, "r=17"), (_blur, dict(H=0), -1, "H=0"), (_blur, dict(R=65536), -1, "R=65536"),
    (_blur, dict(out=D), -3, "out must not be x")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_"), msg


def test_scratch_bytes(lib):
    fn = _fn(lib, "ppf_pixel_order_scratch_bytes", ctypes.c_size_t)
    assert fn(1, 50176) == 16 * 50176 and fn(7, 100) == 7 * 1600 and fn(256, 65536) == fn(100000, 65536) == 256 * 16 * 65536
    assert fn(0, 10) == fn(1, 0) == fn(1, 65537) == 0


# ------------------------------------------------------------------------------------------------ the order referee
def _adversarial(n, rng):
    normal = rng.standard_normal(n).astype(np.float32)
    mixed = normal.copy()
    mixed[rng.random(n) < 0.3] = np.nan
    zeros = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    infs = rng.choice(np.array([np.inf, -np.inf, 0.0, 1.0, -1.0, np.nan], dtype=np.float32), n)
    den = (rng.integers(-3, 4, n) * np.float32(1e-45)).astype(np.float32)
    asc = np.sort(normal)
    seven = (rng.integers(0, 7, n) / np.float32(4) - 1).astype(np.float32)
    return np.stack([np.full(n, 2.5, dtype=np.float32), np.full(n, np.nan, dtype=np.float32), mixed, zeros, infs, den, asc, asc[::-1].copy(), seven, normal])


def _score_key(v):
    """order_keys.h's score_key, in numpy."""
    v = np.where(v == 0, np.float32(0), v).astype(np.float32)
    u = v.view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0), k).astype(np.uint64)


@pytest.mark.parametrize("n", [1, 2, 63, 200])
def test_order_referee_against_a_brute_force_count(n):
    from protopformer_amd.interpret import pixel_order_from_scores
    rows = _adversarial(n, np.random.default_rng(n))
    cls = np.zeros(rows.shape[0], dtype=np.int32)
    cls[-1] = -1
    rank = pixel_order_from_scores(rows, cls, device=False)
    assert rank.shape == rows.shape and rank.dtype == np.int32 and (rank[-1] == -1).all()
    for r in range(rows.shape[0] - 1):
        k, i = _score_key(rows[r]), np.arange(n)
        before = (k[None, :] > k[:, None]) | ((k[None, :] == k[:, None]) & (i[None, :] < i[:, None]))      # [i, j]: j comes before i
        assert np.array_equal(rank[r], before.sum(1)), f"row {r}"
        assert np.array_equal(np.sort(rank[r]), i)
    lead = pixel_order_from_scores(rows[:6].reshape(2, 3, n), np.zeros((2, 3), dtype=np.int32), device=False)
    assert lead.shape == (2, 3, n) and np.array_equal(lead.reshape(6, n), rank[:6])


# ------------------------------------------------------------------------------------------------ the blur referee and the taps
@pytest.mark.parametrize("sigma,radius", [(5.0, 5), (1.0, 1), (3.0, 16), (0.5, 4)])
def test_gauss_taps(sigma, radius):
    from protopformer_amd.interpret import gauss_taps
    w = gauss_taps(sigma, radius)
    assert w.dtype == np.float32 and w.shape == (2 * radius + 1,) and np.array_equal(w, w[::-1]) and (w > 0).all() and w.argmax() == radius
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    ref = np.exp(-d * d / (2 * sigma * sigma))
    assert np.array_equal(w, (ref / ref.sum()).astype(np.float32))
    for bad in (dict(radius=0), dict(radius=17), dict(sigma=0.0)):
        with pytest.raises(ValueError, match="gauss_taps"):
            gauss_taps(**{**dict(sigma=sigma, radius=radius), **bad})


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 9), (1, 32, 32), (1, 40, 23)])
@pytest.mark.parametrize("radius", [1, 5, 16])
def test_blur_referee_against_a_direct_fp64_convolution(shape, radius):
    from protopformer_amd.interpret import gauss_blur, gauss_taps
    rng = np.random.default_rng(shape[1] + radius)
    x = rng.standard_normal(shape).astype(np.float32)
    got = gauss_blur(x, sigma=2.5, radius=radius, device=False)
    assert got.shape == shape and got.dtype == np.float32
    w = gauss_taps(2.5, radius).astype(np.float64)
    k2 = np.outer(w, w)                                                                       # [dy, dx]
    _, H, W = shape
    pad = np.zeros((shape[0], H + 2 * radius, W + 2 * radius))
    pad[:, radius:radius + H, radius:radius + W] = x
    ref, mag = np.zeros(shape), np.zeros(shape)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            ref += k2[dy, dx] * pad[:, dy:dy + H, dx:dx + W]
            mag += k2[dy, dx] * np.abs(pad[:, dy:dy + H, dx:dx + W])
    bound = (2 * (2 * radius + 1) + 2) * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(gauss_blur(x[0], sigma=2.5, radius=radius, device=False), got[0])   # any leading shape


def test_blur_referee_skips_what_lies_outside():
    from protopformer_amd.interpret import gauss_blur
    x = np.ones((4, 6), dtype=np.float32)
    x[0, 0] = np.inf
    out = gauss_blur(x, radius=2, device=False)
    assert np.isinf(out[0, 0]) and not np.isnan(out).any() and np.isfinite(out[3, 5]) and out[3, 5] < 1.0      # a zero border darkens the corner
    z = gauss_blur(np.full((3, 3), -0.0, dtype=np.float32), radius=1, device=False)
    assert not np.signbit(z).any()                                                            # the sums start from +0


# ------------------------------------------------------------------------------------------------ random scores, perturbation, counts, parser
def test_random_scores_are_a_function_of_seed_id_and_pixel():
    from protopformer_amd.interpret import philox4x32_10, pixel_random_scores
    ids = np.array([3, (1 << 40) + 3, 9], dtype=np.int64)
    s = pixel_random_scores(ids, 50, seed=(7 << 32) + 1, device=False)
    assert s.shape == (3, 50) and s.dtype == np.float32 and ((s >= 0) & (s < 1)).all() and not np.array_equal(s[0], s[1])
    assert np.array_equal(pixel_random_scores(ids[::-1].copy(), 50, seed=(7 << 32) + 1, device=False), s[::-1])
    word = philox4x32_10(np.array([17, 0x80000000, 3, 1 << 8], dtype=np.uint64), np.array([1, 7], dtype=np.uint64))[0]
    assert s[1, 17] == np.float32(int(word) >> 8) * np.float32(2.0 ** -24)


def test_perturb_referee_identities():
    from protopformer_amd.interpret import perturb_pixels, pixel_order_from_scores
    rng = np.random.default_rng(1)
    B, M, H, W = 2, 2, 4, 8
    x, base = rng.standard_normal((B, 3, H, W)).astype(np.float32), rng.standard_normal((B, 3, H, W)).astype(np.float32)
    rank = pixel_order_from_scores(rng.standard_normal((B, M, H * W)).astype(np.float32), np.array([[0, 1], [-1, 2]], dtype=np.int32), device=False)
    counts = [0, 5, 32]
    d = perturb_pixels(x, rank, counts, baseline=base, device=False)
    i = perturb_pixels(x, rank, counts, insertion=True, baseline=base, device=False)
    assert d.shape == i.shape == (3, B, M, 3, H, W)
    assert np.array_equal(d[0, 0, 0], x[0]) and np.array_equal(d[2, 0, 1], base[0]) and np.array_equal(i[0, 0, 0], base[0]) and np.array_equal(i[2, 0, 1], x[0])
    assert np.array_equal(d[:, 1, 0], np.broadcast_to(x[1], (3, 3, H, W))) and np.array_equal(i[:, 1, 0], d[:, 1, 0])        # the -1 row
    removed = (d[1, 0, 0] != x[0]).all(0)
    assert removed.sum() == 5 and np.array_equal(removed.reshape(-1), rank[0, 0] < 5)
    assert np.array_equal(np.where(removed, i[1, 0, 0], d[1, 0, 0]), x[0])                    # deletion and insertion split x between them
    with pytest.raises(ValueError, match="rank must be"):
        perturb_pixels(x, rank[:, :, :16], counts, device=False)


def test_default_counts_at_pixel_resolution_and_parser_defaults():
    from protopformer_amd.faithfulness import get_args_parser, summarize
    from protopformer_amd.interpret import BLUR_DEFAULTS, RESOLUTIONS, Faithfulness, default_counts
    c = default_counts(50176, 14)
    assert c.dtype == np.int32 and c[0] == 0 and c[-1] == 50176 and len(c) == 15 and (np.diff(c) > 0).all()
    assert default_counts(50176, 4).tolist() == [0, 12544, 25088, 37632, 50176]
    p = get_args_parser()
    assert (p.get_default("resolution"), p.get_default("baseline")) == ("cell", "mean") == (RESOLUTIONS[0], "mean")
    assert (p.get_default("blur_sigma"), p.get_default("blur_radius")) == (5.0, 5) == (BLUR_DEFAULTS["sigma"], BLUR_DEFAULTS["radius"])
    res = dict(images=1, counts=[0, 2], grid_cells=2, orders={"random": {"deletion": dict(curve=[1.0, 0.0], auc=0.5)}})
    assert list(summarize(res)) == ["images", "counts", "grid_cells", "orders", "vs_random"]
    assert list(summarize(res, dict(resolution="pixel")))[-1] == "resolution"
    f = Faithfulness({"deletion": np.array([[[1.0, 0.5, 0.0]]], dtype=np.float32)}, np.array([0, 2, 4], dtype=np.int32), np.zeros((1, 1), dtype=np.int32), None,
                     np.zeros((1, 1, 4), dtype=np.int32), np.zeros((1, 1, 4), dtype=np.float32), 4, resolution="pixel")
    assert f.resolution == "pixel" and f.order is None and f.auc()["deletion"][0, 0] == 0.5   # the area over counts / (H * W)


# ------------------------------------------------------------------------------------------------ the composite key, on the host
def test_pixel_order_key(tmp_path):
    cxx = _host_compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "pixel_key_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "protopformer_amd", "csrc"),
            os.path.join(ROOT, "tests", "pixel_key_check.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:                        # a host compiler without the sanitizer runtimes: the checks themselves do not need them
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "pixel order key: ok" in run.stdout
