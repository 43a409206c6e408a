"""The launch sequence of one train step as text: one line per entry of the recorded command list (engine.ReplayedTrainStep.rec.cmds).
Two trees that enqueue the same step -- same entry points, arguments, streams, buffer reuse -- write byte-identical files, so a host-side
refactor is checked by comparing hashes (run both trees against one library build: PPF_LIB_PATH).

    python scripts/gpu/launch_trace.py micro_deit|micro_cait|micro_deit_bottleneck|deit_small|deit_tiny|cait_xxs24 OUT.txt

micro_*: the fixture models of tests/golden; the others: bench.py's configurations at their batch sizes.  PPF_* switches apply as usual.
Line format: kind, entry point, then the arguments in order.  A pointer argument is the ordinal of its address's first appearance in the
list (the recording keeps every tensor alive, so equal ordinals mean the same buffer; None stays None), a stream is `main` (the stream
the step was recorded on) or `side`, everything else is printed verbatim.  Prints the file's sha256."""
import hashlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch

from protopformer_amd import _lib
from protopformer_amd.engine import FlatAdamW, ReplayedTrainStep
from protopformer_amd.protopformer import CrossEntropyLoss


def build(name):
    if name.startswith("micro_"):
        from helpers import build_micro, micro
        sd, cfg, z = micro(name + ".npz")
        torch.manual_seed(0)
        model = build_micro(cfg, sd).train()
        return model, FlatAdamW(model, weight_decay=0.05, ema_decay=0.999), torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    import bench
    cfg = dict(bench.CONFIGS[name], addon="regular")
    device = torch.device("cuda", 0)
    model, opt, _, _ = bench.build(cfg, device, seed=1028)
    g = torch.Generator(device=device).manual_seed(1028)
    img = torch.randn(cfg["batch"], 3, 224, 224, device=device, generator=g)
    return model, opt, img, torch.randint(0, cfg["C"], (cfg["batch"],), device=device, generator=g)


def lines(rec):
    ordinal = {}
    stream = lambda s: "main" if s == rec.main_stream else "side"
    for c in rec.cmds:
        if c[0] == _lib.Recorder.CALL:
            _, _, args, name = c
            _, ptr_pos, has_stream, arity = _lib._FAST[name]
            out = []
            for i, v in enumerate(args):
                if (name.startswith("ppf_stream_") and i in ptr_pos) or (has_stream and i == arity - 1):
                    out.append(stream(v))
                elif i in ptr_pos:
                    out.append("None" if v is None else "@%d" % ordinal.setdefault(v, len(ordinal)))
                else:
                    out.append(repr(v))
            yield "CALL %s %s" % (name, " ".join(out))
        elif c[0] == _lib.Recorder.MARK:
            yield "MARK %s slot%d" % (stream(c[1]), c[2])
        elif c[0] == _lib.Recorder.WAIT:
            yield "WAIT %s slot%d" % (stream(c[2]), c[3])
        else:
            yield "LIVE"


def main():
    name, out_path = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    model, opt, img, label = build(name)
    step = ReplayedTrainStep(model, CrossEntropyLoss(), opt, epoch=20, use_ppc_loss=True, warmup=2, adopt_inputs=True)
    for _ in range(3):                                   # two eager steps, then the recorded one
        step(img, label)
    torch.cuda.synchronize()
    text = "".join(l + "\n" for l in lines(step.rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print("LAUNCH_TRACE %s %d entries sha256 %s" % (name, len(step.rec.cmds), hashlib.sha256(text.encode()).hexdigest()), flush=True)


if __name__ == "__main__":
    main()
