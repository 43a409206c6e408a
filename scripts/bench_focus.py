"""Cost of the foreground-focus pass on one MI355X -- profiles/focus_cost.txt.

    python scripts/bench_focus.py [--batch 256 --reps 20] [--out profiles/focus_cost.txt]

At the deit_small shape (2000 prototypes, 200 classes, 81 of 196 tokens reserved, 224 x 224 images, batch 256, ten maps per image:
2560 maps 14 x 14 -> 224 x 224) it measures, with HIP events around single launches queued behind a running matrix product (`reps`
launches after 3 warm-up launches; the wrappers' small output allocations are inside the pair),
  * ppf_act_focus next to ppf_act_peak and ppf_act_upsample on the same maps -- the yardstick: the same up-sample, plus two fp64
    accumulators and a box test per element; if ppf_act_focus takes more than ppf_act_peak plus ppf_act_upsample the fusion has failed
    its purpose, and the row `verdict` says so;
  * the unfused device alternative: interpret.upsample_cubic_device followed by torch clamps, masks and sums;
  * ppf_focus_box_terms, ppf_reserve_focus and ppf_evidence_focus;
  * PPNet.push_forward of one batch and the whole pass on that batch's outputs (interpret.focus_from_outputs: events around the
    host-enqueued call, which includes the read-back of high_activation_boxes), and the share of the forward the pass adds.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import deit_small_ppnet, push_forward_row, row, timed      # noqa: E402

P, C, PPC, IMG, PATCH, G_SIDE, RESERVED = 2000, 200, 10, 224, 16, 14, 81


def _boxes(n, gen, dev):
    lo = torch.randint(0, IMG // 2, (n, 2), device=dev, generator=gen)
    ext = torch.randint(IMG // 4, IMG // 2 + 1, (n, 2), device=dev, generator=gen)
    return torch.stack([lo[:, 0], lo[:, 0] + ext[:, 0], lo[:, 1], lo[:, 1] + ext[:, 1]], 1).to(torch.int32).contiguous()


def kernels(B, reps):
    from protopformer_amd import ops
    from protopformer_amd.interpret import expand_to_grid, upsample_cubic_device
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1028)
    M, G, s = B * PPC, G_SIDE * G_SIDE, int(round(RESERVED ** 0.5))
    attn = torch.rand((B, G), device=dev, generator=gen)
    acts = torch.rand((B, PPC, s, s), device=dev, generator=gen) * 5.0
    maps = expand_to_grid(acts, attn, RESERVED).reshape(M, G_SIDE, G_SIDE).contiguous()     # what the pass up-samples: 81 of 196 cells non-zero
    obj = _boxes(B, gen, dev)
    map_bytes, up_bytes = M * G * 4, M * IMG * IMG * 4
    rows = []
    t_peak = timed(lambda: ops.act_peak(maps, IMG), reps)
    rows.append(row(f"ppf_act_peak, {M} maps {G_SIDE}x{G_SIDE} -> {IMG}x{IMG} (the yardstick: the same up-sample, peak only)", t_peak, map_bytes))
    t_up = timed(lambda: ops.act_upsample(maps, IMG), reps)
    rows.append(row(f"ppf_act_upsample of the same maps (writes the {up_bytes} bytes of up-sampled maps)", t_up, map_bytes + up_bytes))
    t_focus = timed(lambda: ops.act_focus(maps, IMG, obj), reps)
    rows.append(row(f"ppf_act_focus of the same maps, {PPC} maps per image, one object box per image: peak, hit, fp64 inside / total, non-finite count",
                    t_focus, map_bytes, over_act_peak=round(t_focus["us_median"] / t_peak["us_median"], 3)))
    ys, xs = torch.arange(IMG, device=dev)[None, :, None], torch.arange(IMG, device=dev)[None, None, :]
    ob = obj.repeat_interleave(PPC, dim=0)

    def unfused():
        up = upsample_cubic_device(maps, IMG)
        pos = torch.where(torch.isfinite(up), up, torch.zeros_like(up)).clamp(min=0).double()
        mask = (ys >= ob[:, 0, None, None]) & (ys < ob[:, 1, None, None]) & (xs >= ob[:, 2, None, None]) & (xs < ob[:, 3, None, None])
        val, at = up.flatten(1).max(1)
        return val, at, (pos * mask).sum((1, 2)), pos.sum((1, 2))
    t_un = timed(unfused, reps)
    rows.append(row("the unfused device alternative: upsample_cubic_device, then torch isfinite / where / clamp / double, a box mask, two sums and a max "
                    "(several launches; the up-sampled maps pass through memory)", t_un, map_bytes + up_bytes,
                    over_act_focus=round(t_un["us_median"] / t_focus["us_median"], 2)))
    limit = t_peak["us_median"] + t_up["us_median"]
    rows.append(dict(what="verdict: ppf_act_focus against ppf_act_peak + ppf_act_upsample of the same maps in this run (medians)",
                     act_focus_us=t_focus["us_median"], act_peak_plus_act_upsample_us=round(limit, 2),
                     fusion_serves_its_purpose=bool(t_focus["us_median"] <= limit)))
    box = _boxes(M, gen, dev)
    t = timed(lambda: ops.focus_box_terms(box, obj, IMG), reps)
    rows.append(row(f"ppf_focus_box_terms, {M} boxes against {B} object boxes", t, M * 32 + B * 16))
    idx = torch.topk(attn, RESERVED, dim=1)[1].sort(dim=1)[0].to(torch.int32).contiguous()
    t = timed(lambda: ops.reserve_focus(idx, obj, G_SIDE, PATCH, attn), reps)
    rows.append(row(f"ppf_reserve_focus, B={B}, {RESERVED} reserved cells of {G}, with the rollout scores", t, B * (RESERVED * 4 + G * 4 + 16 + 32)))
    act_max = torch.rand((B, P), device=dev, generator=gen) * 5.0
    argmax = torch.randint(0, RESERVED, (B, P), device=dev, generator=gen).to(torch.int32)
    weight = torch.where(torch.arange(P, device=dev)[None, :] // PPC == torch.arange(C, device=dev)[:, None], 1.0, -0.5).contiguous()
    cls = torch.randint(0, C, (B, 1), device=dev, generator=gen).to(torch.int32)
    t = timed(lambda: ops.evidence_focus(act_max, weight, 0.5, PPC, cls, obj, G_SIDE, PATCH, idx=idx, argmax=argmax), reps)
    rows.append(row(f"ppf_evidence_focus, B={B} P={P} C={C}, one class per image (one wave per row)", t, B * (P * 12 + 48)))
    return rows


def pass_rows(B, runs):
    """The whole pass on one batch's outputs next to the forward that made them."""
    from protopformer_amd.interpret import _eval_outputs, focus_from_outputs
    dev = torch.device("cuda")
    rows = [push_forward_row(B, runs, f"PPNet.push_forward, deit_small {P}x384, batch {B} (the forward the pass follows)")]
    torch.cuda.empty_cache()
    m = deit_small_ppnet()
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, 3, IMG, IMG, device=dev, generator=gen)
    obj, labels = _boxes(B, gen, dev), torch.randint(0, C, (B,), device=dev, generator=gen)
    with torch.no_grad():
        outs = _eval_outputs(m, x)
    w, coe = m.last_layer.weight.detach().contiguous(), float(m.global_coe)
    for mode, per in (("own", PPC), ("top", 3)):
        call = lambda: focus_from_outputs(outs, obj, w, 1.0 - coe, PPC, RESERVED, IMG, labels, mode, 3, 95, coe)
        for _ in range(3):
            call()
        ms = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        fwd = rows[0]["ms_median"]
        rows.append(dict(what=f"interpret.focus_from_outputs on that batch's outputs, protos='{mode}' ({per} maps per image = {B * per} maps): selection, "
                              "expand_to_grid, ppf_act_focus, order statistics + threshold read-back + boxes, box terms, reservation, evidence; host-enqueued",
                         runs=runs, ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3),
                         share_of_push_forward=round(float(np.median(ms)) / fwd, 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "focus_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focus.py measures on the GPU; none found")
    rows = kernels(a.batch, a.reps)
    torch.cuda.empty_cache()
    rows += pass_rows(a.batch, 5)
    head = [f"# foreground-focus cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_focus.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside); pass rows: events around "
            "the host-enqueued call"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
