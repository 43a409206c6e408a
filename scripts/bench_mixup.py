"""Cost of Mixup / CutMix and the soft-target cross-entropy on one MI355X (profiles/mixup_cost.txt).

    python scripts/bench_mixup.py kernels [--iters N]        ppf_mixup_apply at B = 256, 224^2 (blend, CutMix), ppf_mixup_target and
                                                            ppf_soft_cross_entropy at 256 x 200: host-clock time per call over N calls
                                                            ending in a synchronise; run it under `rocprofv3 --kernel-trace --stats`
                                                            for the kernel times
    python scripts/bench_mixup.py step [--steps K --rounds R]
                                                            replayed deit_small bs256 step (engine.ReplayedTrainStep), plain (int labels,
                                                            CrossEntropyLoss) against Mixup(0.8, 1.0, smoothing 0.1) + SoftTargetCrossEntropy
                                                            in alternating rounds on the same box; PPC off in both (Mixup refuses it)

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np      # noqa: E402
import torch            # noqa: E402


def _timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def kernels(iters):
    from protopformer_amd import mixup as M
    from protopformer_amd import ops
    dev = torch.device("cuda")
    B, H, W, C = 256, 224, 224, 200
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, 3, H, W, device=dev, generator=g)
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    stream_bytes = 2 * x.numel() * 4                    # every element read once and written once (blend)
    blend = np.zeros((B, M.MIX_WORDS), np.int32)
    blend[:, M.KIND] = M.BLEND
    blend[:, M.WSELF], blend[:, M.WOTHER] = M._bits(0.7), M._bits(0.3)
    box = blend.copy()
    box[:, M.KIND] = M.BOX
    box[:, M.YL:M.XH + 1] = [56, 168, 56, 168]          # lam = 0.75: a quarter of every image
    table_dev = torch.empty(B * M.MIX_WORDS, dtype=torch.int32, device=dev)
    for name, table in (("ppf_mixup_apply blend", blend), ("ppf_mixup_apply cutmix 112x112", box)):
        host = torch.from_numpy(table.reshape(-1).copy()).pin_memory()
        us = _timed(lambda: ops.mixup_apply(x, host, table_dev), iters)
        out = dict(what=name, shape=[B, 3, H, W], us_per_call_host_clock=round(us, 2))
        if table is blend:
            out["stream_gb_per_s_host_clock"] = round(stream_bytes / us / 1e3, 1)
        print(json.dumps(out), flush=True)
    us = _timed(lambda: ops.mixup_target(y, table_dev, C, 0.1 / C, 0.9 + 0.1 / C), iters)
    print(json.dumps(dict(what="ppf_mixup_target", shape=[B, C], us_per_call_host_clock=round(us, 2))), flush=True)
    logits = torch.randn(B, C, device=dev, generator=g)
    t = torch.softmax(torch.randn(B, C, device=dev, generator=g), 1)
    us = _timed(lambda: ops.soft_cross_entropy(logits, target=t), iters)
    print(json.dumps(dict(what="ppf_soft_cross_entropy dense", shape=[B, C], us_per_call_host_clock=round(us, 2))), flush=True)
    us = _timed(lambda: ops.soft_cross_entropy(logits, label=y, smoothing=0.1), iters)
    print(json.dumps(dict(what="ppf_soft_cross_entropy label smoothing", shape=[B, C], us_per_call_host_clock=round(us, 2))), flush=True)
    us = _timed(lambda: ops.cross_entropy(logits, y), iters)
    print(json.dumps(dict(what="ppf_cross_entropy (int labels, for comparison)", shape=[B, C], us_per_call_host_clock=round(us, 2))), flush=True)
    mix = M.Mixup(0.8, 1.0, label_smoothing=0.1, num_classes=C)
    np.random.seed(0)
    us = _timed(lambda: mix(x, y), iters)
    print(json.dumps(dict(what="Mixup.__call__ (draw + upload + apply + target), mode batch", shape=[B, 3, H, W], us_per_call_host_clock=round(us, 2))),
          flush=True)


def step(steps, rounds):
    from protopformer_amd.engine import FlatAdamW, ReplayedTrainStep
    from protopformer_amd.mixup import Mixup, SoftTargetCrossEntropy
    from protopformer_amd.protopformer import CrossEntropyLoss, construct_PPNet
    dev = torch.device("cuda")
    B, C = 256, 200

    def make(crit):
        torch.manual_seed(1028)
        m = construct_PPNet("deit_small_patch16_224", pretrained=False, img_size=224, prototype_shape=(2000, 384, 1, 1), num_classes=C,
                            reserve_layers=[11], reserve_token_nums=[81], use_global=True, use_ppc_loss=False, global_proto_per_class=10,
                            add_on_layers_type="regular").to(dev).train()
        opt = FlatAdamW(m, weight_decay=0.05, ema_decay=0.99996)
        return ReplayedTrainStep(m, crit, opt, epoch=20, use_ppc_loss=False, warmup=2, adopt_inputs=True)

    g = torch.Generator(device=dev).manual_seed(1028)
    img = torch.randn(B, 3, 224, 224, device=dev, generator=g)
    label = torch.randint(0, C, (B,), device=dev, generator=g)
    img_m = img.clone()
    plain = make(CrossEntropyLoss())
    mixed = make(SoftTargetCrossEntropy())
    mix = Mixup(0.8, 1.0, label_smoothing=0.1, num_classes=C)
    np.random.seed(0)
    runs = {"plain": lambda: plain(img, label), "mixup+soft_ce": lambda: mixed(*mix(img_m, label))}
    for fn in runs.values():                             # warm-up, recording, first replays
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = fn()[0]
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)
            assert torch.isfinite(loss).all(), k
    out = {k: dict(ms_per_step=[round(v, 3) for v in vs], median=round(float(np.median(vs)), 3)) for k, vs in ms.items()}
    out["delta_pct_median"] = round((out["mixup+soft_ce"]["median"] / out["plain"]["median"] - 1.0) * 100.0, 2)
    print(json.dumps(dict(what="replayed deit_small bs256 step, PPC off", steps_per_round=steps, rounds=rounds, **out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "step"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py measures on the GPU; none found")
    if a.mode == "kernels":
        kernels(a.iters)
    else:
        step(a.steps, a.rounds)


if __name__ == "__main__":
    main()
