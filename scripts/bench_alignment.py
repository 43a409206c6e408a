"""Cost of the image gradient and the spatial-alignment pass on one MI355X -- profiles/alignment_cost.txt.

    python scripts/bench_alignment.py [--batch 256 --reps 20] [--out profiles/alignment_cost.txt]

At the deit_small shape (2000 prototypes of width 384, 200 classes, 81 reserved tokens, 3 x 224 x 224 images, batch 256) it measures
  * the two launches an image gradient adds to a backward -- the embed input-gradient product dcols = dtok W (bf16 operands, fp32 out)
    and ppf_col2im_patch_f32 --, ppf_grad_box_mass and ppf_pgd_step_box on a batch of images: HIP events around every single launch,
    queued behind a running matrix product so that the host's enqueue time is not in the figure, `reps` launches after 3 warm-up
    launches; the bytes each launch moves (computed from the shapes) and the GB/s of the median launch; for scale a device-to-device
    copy of the same bytes;
  * one forward plus backward of the model per attack step (interpret.input_gradient of a prototype activation), the same backward
    without the image gradient (a plain tensor as the input), and the time of the weight-gradient launches inside that backward
    (ppf_gemm_probe: events around every weight-gradient GEMM on its own stream) -- what an input-only backward would not launch;
  * the per-sample cosines of the bf16 product path's image gradient against the fp32 verification mode on the three micro fixtures, the
    figures the gate of tests/test_gpu_input_grad.py is derived from.
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

from bench_common import deit_small_ppnet, row, timed      # noqa: E402

P, D, IMG, PATCH = 2000, 384, 224, 16


def kernels(B, reps):
    from protopformer_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1028)
    Np, K = (IMG // PATCH) ** 2, 3 * PATCH * PATCH
    M = B * Np
    rows = []
    dtok = torch.randn((M, D), device=dev, generator=g).bfloat16()
    w16 = torch.randn((D, K), device=dev, generator=g).bfloat16()
    dcols = torch.empty((M, K), device=dev)
    t = timed(lambda: ops.gemm(dtok, w16, trans_b=True, epi=ops.EPI_F32, out=dcols), reps)
    rows.append(row(f"embed input-gradient GEMM dcols[{M}, {K}] = dtok[{M}, {D}] . W[{D}, {K}] (bf16 operands, fp32 out)", t,
                    M * D * 2 + D * K * 2 + M * K * 4, gflop=round(2.0 * M * K * D / 1e9, 2),
                    tflops_at_median=round(2.0 * M * K * D / t["us_median"] / 1e6, 1)))
    t = timed(lambda: ops.col2im_patch(dcols, B, 3, IMG, IMG, PATCH), reps)
    rows.append(row(f"ppf_col2im_patch_f32, B={B} 3x{IMG}x{IMG} patch {PATCH} (allocation of the image inside)", t, 2 * M * K * 4))
    x0 = torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    x, grad = x0.clone(), torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    peak = torch.randint(0, IMG, (B, 2), device=dev, generator=g)
    box = torch.stack([(peak[:, 0] - 36).clamp(min=0), (peak[:, 0] + 36).clamp(max=IMG), (peak[:, 1] - 36).clamp(min=0), (peak[:, 1] + 36).clamp(max=IMG)],
                      1).to(torch.int32).contiguous()
    img_bytes = x.numel() * 4
    t = timed(lambda: ops.grad_box_mass(grad, box), reps)
    rows.append(row(f"ppf_grad_box_mass, R={B} 3x{IMG}x{IMG}, boxes of 72 x 72 (three small allocations inside)", t, img_bytes, workgroups=B,
                    threads_per_workgroup=512))
    from protopformer_amd.interpret import attack_bounds
    consts = attack_bounds(8 / 255, None, 10, dev)
    t = timed(lambda: ops.pgd_step_box(x, x0, grad, box, *consts, -1), reps)
    rows.append(row(f"ppf_pgd_step_box, R={B} 3x{IMG}x{IMG} (reads x, x0, g; writes x)", t, 4 * img_bytes))
    dst = torch.empty_like(x)
    t = timed(lambda: dst.copy_(x), reps)
    rows.append(row(f"for scale: device-to-device copy of one batch of images ({img_bytes} bytes read, as many written)", t, 2 * img_bytes))
    big = torch.empty((2, B, 3, IMG, IMG), device=dev)
    big2 = torch.empty_like(big)
    t = timed(lambda: big2.copy_(big), reps)
    rows.append(row("for scale: device-to-device copy of two batches of images (the 4 x image bytes ppf_pgd_step_box moves)", t, 4 * img_bytes))
    return rows


def model_rows(B, runs):
    """Forward and backward of deit_small with and without the image gradient, and the weight-gradient launches inside the backward."""
    from protopformer_amd import _lib
    from protopformer_amd.interpret import input_gradient
    dev = torch.device("cuda")
    m = deit_small_ppnet()
    x = torch.randn(B, 3, IMG, IMG, device=dev)
    protos = torch.randint(0, P, (B,), device=dev)

    def fwd_bwd(want_image_grad, probe=False):
        """(forward ms, backward ms, weight-gradient kernel ms inside the backward or None) of the summed prototype activations."""
        xg = x.clone().requires_grad_(want_image_grad)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        with torch.enable_grad():
            value = m._branches(xg, want_dist=False).act_max_local.gather(1, protos[:, None]).sum()
        ev[1].record()
        if probe:
            _lib.call("ppf_gemm_probe", 1)
        value.backward()
        ev[2].record()
        torch.cuda.synchronize()
        wg = None
        if probe:
            _lib.call("ppf_gemm_probe", 0)
            c_ms, c_n, c_fl, c_by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            _lib.call("ppf_gemm_probe_read", ctypes.addressof(c_ms), ctypes.addressof(c_n), ctypes.addressof(c_fl), ctypes.addressof(c_by))
            wg = (c_ms.value, int(c_n.value))
        for p in m.parameters():
            p.grad = None
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), wg

    rows = []
    for want in (False, True):
        for _ in range(2):
            fwd_bwd(want)
        f, b = zip(*[fwd_bwd(want)[:2] for _ in range(runs)])
        rows.append(dict(what=f"deit_small 2000x384 batch {B}, eval mode, backward of the summed prototype activations, host-enqueued: "
                              + ("WITH the image gradient (+ GEMM + col2im)" if want else "without the image gradient"),
                         runs=runs, forward_ms_median=round(float(np.median(f)), 3), backward_ms_median=round(float(np.median(b)), 3),
                         backward_ms_min=round(min(b), 3), backward_ms_max=round(max(b), 3)))
    _, b, wg = fwd_bwd(True, probe=True)
    rows.append(dict(what="weight-gradient GEMM launches inside that backward (ppf_gemm_probe: events around each on its own stream; they overlap "
                          "the main stream, so this is kernel time, not critical-path time): what an input-only backward would not launch",
                     backward_ms=round(b, 3), weight_gradient_kernel_ms=round(wg[0], 3), weight_gradient_launches=wg[1],
                     share_of_backward_wall_time=round(wg[0] / b, 3)))
    for _ in range(2):
        input_gradient(m, x, ("proto", "local", protos))
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); input_gradient(m, x, ("proto", "local", protos)); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    rows.append(dict(what=f"interpret.input_gradient, batch {B}: one forward + backward, the cost of one attack step (ppf_pgd_step_box on top)", runs=runs,
                     ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3)))
    return rows


def cosine_rows():
    """bf16 product path against the fp32 verification mode on the micro fixtures: per-sample cosine of the image gradient, four targets."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_micro, micro
    from protopformer_amd.interpret import input_gradient
    from protopformer_amd.protopformer import CrossEntropyLoss
    rows = []
    for fixture in ("micro_deit.npz", "micro_cait.npz", "micro_deit_bottleneck.npz"):
        sd, cfg, z = micro(fixture)
        x, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
        grads = {}
        for precise in (True, False):
            m = build_micro(cfg, sd)
            m.precise = precise
            g = {"logit": input_gradient(m, x, ("logit", label))[0],
                 "proto_local": input_gradient(m, x, ("proto", "local", label * cfg["protos_per_class"] + 1))[0],
                 "proto_global": input_gradient(m, x, ("proto", "global", label * cfg["global_per_class"]))[0]}
            m.train()
            xg = x.clone().requires_grad_()
            logits, aux = m(xg)
            cov, mean = m.get_PPC_loss(aux[2], aux[3], aux[4], label)
            (CrossEntropyLoss()(logits, label) + 0.1 * cov + 0.5 * mean).backward()
            g["loss"] = xg.grad
            grads[precise] = g
        cos = {}
        for k in grads[True]:
            a, b = grads[False][k].double().flatten(1), grads[True][k].double().flatten(1)
            cos[k] = [round(float(c), 8) for c in (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))]
        worst = min(min(v) for v in cos.values())
        rows.append(dict(what=f"image gradient, bf16 product path against the fp32 mode, {fixture} ({cfg['add_on']} head): cosine per sample", **cos,
                         worst=worst, gate_1_minus_4x=round(1.0 - 4.0 * (1.0 - worst), 8)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "alignment_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_alignment.py measures on the GPU; none found")
    rows = kernels(a.batch, a.reps)
    torch.cuda.empty_cache()
    rows += model_rows(a.batch, 5)
    torch.cuda.empty_cache()
    rows += cosine_rows()
    head = [f"# image gradient and spatial-alignment cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_alignment.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside); model rows: events around "
            "the host-enqueued forward / backward"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
