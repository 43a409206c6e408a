"""What the scripts/bench_*.py drivers share: the two ways they time launches with HIP events, the row format, and the deit_small
PPNet they measure for scale.  Numbers of different drivers are comparable because they come from the same code here.

  timed(fn, reps, warm)        one event pair per call, each call queued behind a running 4096^2 matrix product with a synchronise on
                               each side, so that the host's enqueue time is not in the figure: single launches of microseconds
  timed_back_to_back(fns, ..)  event pairs made beforehand, the calls enqueued back to back on an otherwise idle stream, several
                               candidates alternating inside every repetition: the host's enqueue time is in the figure
The two are different methods; a driver keeps the one its profile under profiles/ was written with."""
import numpy as np
import torch


def timed(fn, reps, warm=3):
    """Median / min / max microseconds of fn(), one event pair per call, each call queued behind a running matrix product."""
    busy = torch.randn((4096, 4096), device="cuda")
    us = []
    for rep in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.mm(busy, busy)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            us.append(e0.elapsed_time(e1) * 1e3)
    return dict(launches_timed=len(us), us_median=round(float(np.median(us)), 2), us_min=round(min(us), 2), us_max=round(max(us), 2))


def timed_back_to_back(fns, reps):
    """{name: [ms per repetition]}: after 3 warm-up calls of each, every repetition times each function once, in turn (event pair
    around the single call, all pairs made before the first call)."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    torch.cuda.synchronize()
    for r in range(reps):
        for k, fn in fns.items():
            ev[k][r][0].record(); fn(); ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}


def row(what, t, nbytes, **extra):
    return dict(what=what, **t, bytes_moved=int(nbytes), gb_per_s_at_median=round(nbytes / t["us_median"] / 1e3, 1), **extra)


def deit_small_ppnet(*, prototypes=2000, proto_dim=384, classes=200, img_size=224, reserved=81, seed=1028):
    """The seeded, unpretrained deit_small PPNet of the flagship shape on the GPU, in eval mode."""
    from protopformer_amd.protopformer import construct_PPNet
    torch.manual_seed(seed)
    return construct_PPNet("deit_small_patch16_224", pretrained=False, img_size=img_size, prototype_shape=(prototypes, proto_dim, 1, 1),
                           num_classes=classes, reserve_layers=[11], reserve_token_nums=[reserved], use_global=True, use_ppc_loss=True,
                           global_proto_per_class=10, add_on_layers_type="regular").to(torch.device("cuda")).eval()


def push_forward_ms(B, reps, **ppnet):
    """Milliseconds of `reps` PPNet.push_forward calls of deit_small_ppnet(**ppnet) on a random batch of B images, after 3 warm-up
    calls: events around the host-enqueued call."""
    m = deit_small_ppnet(**ppnet)
    x = torch.randn(B, 3, m.img_size, m.img_size, device="cuda")
    for _ in range(3):
        m.push_forward(x)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); m.push_forward(x); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def push_forward_row(B, reps, what, **ppnet):
    ms = push_forward_ms(B, reps, **ppnet)
    return dict(what=what, runs=reps, ms_median=round(float(np.median(ms)), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3))
