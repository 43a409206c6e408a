"""Cost of the 'this looks like that, because' pass (interpret.because) on one MI355X -- profiles/because_cost.txt.

    python scripts/bench_because.py [--batch 256 --reps 10 --rounds 3 --radius 4] [--out profiles/because_cost.txt]

At the deit_small shape (3 x 224 x 224 images, batch 256, 81 reserved tokens, 2000 prototypes, 10 rows per image) it measures
  * every kernel of csrc/because.hip: HIP events around every single launch, queued behind a running matrix product so that the host's
    enqueue time is not in the figure (bench_common.timed);
  * the yardsticks of the colour and warp kernels in the same run, alternating with them round by round: a device copy of the batch and
    ppf_patch_perturb writing the same bytes; the ratios to both are reported;
  * the bilateral filter at r = 1, --radius and 8: taps per second, and the LDS-array cycles its reads need at the least (per tap and
    wave of 128 pixels two 16-byte slot reads, two range-table look-ups and one broadcast spatial weight: 14 cycles) against the cycles
    the compute units had at the clock ppf_device_info reports -- the share says how far the LDS is from being the bound;
  * the torch alternative on the device: an einsum for the colour transform, F.grid_sample for the warp, an unfold-based bilateral
    filter at the largest batch that fits 4 GiB of unfolded windows;
  * for scale: PPNet.push_forward of the batch, and the share of the five perturbations and five score launches in a whole pass (one
    clean and five perturbed forwards).
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import ctypes
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import push_forward_row, row, timed      # noqa: E402

GRID, IMG, T, P, K = 196, 224, 81, 2000, 10


def device_clock():
    """(compute units, MHz) as ppf_device_info reports them."""
    from protopformer_amd import _lib
    cu, mhz, name = ctypes.c_int(), ctypes.c_int(), ctypes.create_string_buffer(64)
    _lib.lib().ppf_device_info(ctypes.byref(cu), ctypes.byref(mhz), name, 64)
    return cu.value, mhz.value


def kernels(B, reps, rounds, radius):
    import torch.nn.functional as F
    from protopformer_amd import interpret as I, ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1028)
    x = torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    out = torch.empty_like(x)
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    p = I.because_params()
    mean, std = p["mean"], p["std"]
    img = x[0].numel() * 4
    moved = 2 * B * img
    shape = f"B={B} 3x{IMG}x{IMG}"
    rows = []
    hue, A, s = I.hue_matrix(np.pi), I.warp_amplitude(p["amplitude"]), p["cells"]
    nodes = ops.warp_nodes(ids, s, A, 7)
    rank = torch.zeros((B, 1, GRID), device=dev, dtype=torch.int32)
    counts = torch.full((1,), GRID // 2, device=dev, dtype=torch.int32)
    pout = out.view(1, B, 1, 3, IMG, IMG)
    cands = {"ppf_color_affine (hue)": lambda: ops.color_affine(x, hue, mean, std, out=out),
             "ppf_warp_apply": lambda: ops.warp_apply(x, nodes, s, A, out=out),
             "yardstick: device copy of the batch": lambda: out.copy_(x),
             "yardstick: ppf_patch_perturb, deletion, constant baseline, same bytes written": lambda: ops.patch_perturb(x, rank, counts, False, 0.0, out=pout)}
    med = {k: [] for k in cands}
    for r in range(rounds):                                                     # alternating: every round times each candidate once
        for k, fn in cands.items():
            t = timed(fn, reps)
            med[k].append(t["us_median"])
            rows.append(row(f"round {r}: {k}, {shape}", t, moved))
    m = {k: float(np.median(v)) for k, v in med.items()}
    names = list(cands)
    for k in names[:2]:
        rows.append(dict(what=f"{k} against the yardsticks, medians of the rounds' medians", us=m[k], copy_us=m[names[2]], patch_perturb_us=m[names[3]],
                         time_over_copy=round(m[k] / m[names[2]], 3), time_over_patch_perturb=round(m[k] / m[names[3]], 3)))
    off = torch.zeros((B, 3), device=dev)
    t_off = timed(lambda: ops.color_affine(x, I.contrast_matrix(0.25), mean, std, offset=off, out=out), reps)
    rows.append(row(f"ppf_color_affine with offset (contrast), {shape}", t_off, moved))
    t_sum = timed(lambda: ops.gray_sum(x, mean, std), reps)
    rows.append(row(f"ppf_gray_sum (memset + launch), {shape}", t_sum, B * img))
    total = ops.gray_sum(x, mean, std)
    t_co = timed(lambda: ops.contrast_offset(total, (IMG, IMG), 0.75), reps)
    rows.append(row(f"ppf_contrast_offset, B={B}", t_co, B * 16))
    t_nodes = timed(lambda: ops.warp_nodes(ids, s, A, 7), reps)
    rows.append(row(f"ppf_warp_nodes, s={s} B={B}", t_nodes, B * (s + 1) ** 2 * 8 + B * 8))
    cu, mhz = device_clock()
    t_bil = {}
    for r in sorted({1, int(radius), 8}):
        ws, wr = I.bilateral_tables(r, p["sigma_space"], p["sigma_range"])
        t = timed(lambda: ops.bilateral(x, ws, wr, r, mean, std, out=out), max(3, reps // 2))
        taps = B * IMG * IMG * (2 * r + 1) ** 2
        # a wave serves 128 pixels (two per lane); per tap it issues two ds_read_b128 (4 LDS-array cycles each), two ds_read_b32 look-ups in
        # the range table (2 each, more where lanes meet on a bank) and one broadcast ds_read_b32 of the spatial weight (2): 14 cycles
        lds_cycles = taps / 128 * 14
        sec = t["us_median"] * 1e-6
        t_bil[r] = t
        rows.append(row(f"ppf_bilateral r={r}, {shape}", t, moved, taps=taps, gtaps_per_s=round(taps / sec / 1e9, 1),
                        lds_array_cycles_min=int(lds_cycles), lds_array_cycles_available=int(cu * mhz * 1e6 * sec),
                        share_of_lds_cycles=round(lds_cycles / (cu * mhz * 1e6 * sec), 3), hbm_share_of_8_tb_per_s=round(moved / sec / 8e12, 3), cus=cu, mhz=mhz))
    act_full, idx = torch.rand((B, P, T), device=dev, generator=g), torch.rand((B, GRID), device=dev, generator=g).argsort(-1)[:, :T].to(torch.int32).contiguous()
    act_max = act_full.amax(-1)
    protos = torch.randint(0, P, (B, K), device=dev, generator=g, dtype=torch.int32)
    cells = torch.randint(0, GRID, (B, K), device=dev, generator=g, dtype=torch.int32)
    t_score = timed(lambda: ops.because_score(act_max, protos, GRID, act_full=act_full, idx=idx, cells=cells), reps)
    rows.append(row(f"ppf_because_score, B={B} K={K} P={P} T={T}", t_score, B * K * (T * 4 + 24)))
    # the torch alternatives, on the device
    m64 = torch.from_numpy(hue).to(dev)
    mean_t, std_t = (torch.from_numpy(v).to(dev).reshape(1, 3, 1, 1) for v in (mean, std))
    t = timed(lambda: torch.sub(torch.einsum("kc,bchw->bkhw", m64, (x * std_t + mean_t).clamp(0, 1)).clamp(0, 1), mean_t).div_(std_t), min(reps, 5), warm=1)
    rows.append(dict(what=f"torch alternative, colour: de-normalise, clamp, einsum, clamp, normalise, {shape}", **t))
    base = torch.stack(torch.meshgrid(torch.linspace(-1, 1, IMG, device=dev), torch.linspace(-1, 1, IMG, device=dev), indexing="ij")[::-1], -1)
    coarse = torch.rand((B, 2, s + 1, s + 1), device=dev, generator=g) * 0.05

    def grid_sample():
        flow = F.interpolate(coarse, size=(IMG, IMG), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        return F.grid_sample(x, base[None] + flow, mode="bilinear", padding_mode="border", align_corners=True)
    t = timed(grid_sample, min(reps, 5), warm=1)
    rows.append(dict(what=f"torch alternative, warp: F.interpolate of the node field + F.grid_sample, {shape}", **t))
    r = int(radius)
    D2 = (2 * r + 1) ** 2
    Bu = max(1, min(B, (4 << 30) // (4 * IMG * IMG * D2 * 4)))
    ws_t = torch.from_numpy(I.bilateral_tables(r, p["sigma_space"], p["sigma_range"])[0]).to(dev).reshape(1, 1, D2, 1)
    xs = x[:Bu].clamp(0, 1)

    def unfold_filter():
        y = (0.299 * xs[:, 0] + 0.587 * xs[:, 1] + 0.114 * xs[:, 2])[:, None]
        cols = F.unfold(torch.cat([xs, y], 1), 2 * r + 1, padding=r).reshape(Bu, 4, D2, IMG * IMG)
        w = ws_t * torch.exp(-((cols[:, 3:] - y.reshape(Bu, 1, 1, -1)) * 255) ** 2 / (2 * p["sigma_range"] ** 2))
        return (w * cols[:, :3]).sum(2) / w.sum(2)
    t = timed(unfold_filter, 3, warm=1)
    rows.append(dict(what=f"torch alternative, texture: unfold-based bilateral filter r={r} at batch {Bu} (zero padding counts as taps)", **t,
                     us_per_image=round(t["us_median"] / Bu, 2), ppf_bilateral_us_per_image=round(t_bil[r]["us_median"] / B, 2)))
    del out, act_full
    torch.cuda.empty_cache()
    fwd = push_forward_row(B, 5, f"for scale: PPNet.push_forward, deit_small {P}x384, batch {B}")
    rows.append(fwd)
    own_us = (3 * m[names[0]] + t_sum["us_median"] + t_co["us_median"] + t_bil[r]["us_median"] + t_nodes["us_median"] + m[names[1]] + 5 * t_score["us_median"])
    rows.append(dict(what=f"share: the perturbation and score kernels of one pass (three colour transforms, the luma sum and offset, the filter at r={r}, the "
                          f"warp, five scores) against its six forwards of batch {B} (push_forward as the forward)",
                     kernels_ms=round(own_us / 1e3, 3), forwards_ms=round(6 * fwd["ms_median"], 2), share_percent=round(100 * own_us / 1e3 / (6 * fwd["ms_median"]), 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "because_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_because.py measures on the GPU; none found")
    rows = kernels(a.batch, a.reps, a.rounds, a.radius)
    head = [f"# 'this looks like that, because' cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_because.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
