"""Cost of rendering PartsWorld on the device (csrc/synth.hip), reported not gated: ppf_synth_render for 256 frames of 256 x 256 next to
a device fill and a device copy of the same bytes in the same run, ppf_synth_scene, the numpy referee per frame, and building the
resident default set (5 120 frames).  Event pairs of scripts/bench_common.py.

    python scripts/bench_partsworld.py [--reps 20] [--out profiles/partsworld_cost.txt]
    python -m protopformer_amd.build --variant synthko PPF_SYNTH_KNOCKOUT=1        # beforehand, for the knockout row
    python scripts/bench_partsworld.py --knockout-lib protopformer_amd/lib/libppf_hip_synthko.so

The knockout build renders a flat background and no primitive: what is left is the scene staging, the noise and the stores.  It runs in a
child process (the library is chosen when the binding loads); it is a measurement, not a result."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def render_rows(reps, tag=""):
    import torch
    from bench_common import row, timed
    from protopformer_amd import data as D
    from protopformer_amd import ops
    rows = []
    ids = torch.arange(256, dtype=torch.int64, device="cuda")
    for noise in (8, 0):
        spec = D.PartsWorldSpec(noise=noise)
        scene = ops.synth_scene(spec, ids)
        out = torch.empty((256, 256, 256, 3), dtype=torch.uint8, device="cuda")
        rows.append(row(f"ppf_synth_render{tag} 256 x 256 x 256 x 3, noise {noise}", timed(lambda: ops.synth_render(spec, scene, ids, out=out), reps), out.numel()))
    if not tag:
        src = torch.empty_like(out)
        rows.append(row("device fill of the same bytes (Tensor.fill_)", timed(lambda: out.fill_(7), reps), out.numel()))
        rows.append(row("device copy of the same bytes (Tensor.copy_, read + write)", timed(lambda: out.copy_(src), reps), 2 * out.numel()))
        spec = D.PartsWorldSpec()
        rows.append(row("ppf_synth_scene 256 ids", timed(lambda: ops.synth_scene(spec, ids), reps), 256 * 4 * D.SYNTH_WORDS))
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "partsworld_cost.txt"))
    p.add_argument("--knockout-lib", default="", help="a library built with -DPPF_SYNTH_KNOCKOUT=1 (python -m protopformer_amd.build --variant)")
    p.add_argument("--rows-only", default="", help="internal: print the render rows as JSON under this tag and exit")
    args = p.parse_args()
    if args.rows_only:
        print("ROWS " + json.dumps(render_rows(args.reps, args.rows_only)))
        return
    import numpy as np
    import torch
    from protopformer_amd import data as D
    rows = render_rows(args.reps)
    if args.knockout_lib:
        env = dict(os.environ, PPF_LIB_PATH=os.path.abspath(args.knockout_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-only", " [knockout: flat background, no primitive]", "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=600, check=True)
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    spec = D.PartsWorldSpec()
    ids = np.arange(8, dtype=np.int64)
    per = []
    for _ in range(3):
        t0 = time.perf_counter()
        D.partsworld_render(spec, D.partsworld_scene_from_ids(spec, ids), ids)
        per.append((time.perf_counter() - t0) / len(ids) * 1e3)
    rows.append(dict(what="numpy referee, scene + render, per 256 x 256 frame (8 frames, 3 runs)", ms_median=round(float(np.median(per)), 2),
                     ms_min=round(min(per), 2), ms_max=round(max(per), 2)))
    build = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dds = [D.DeviceDataset(D.PartsWorld(spec, train=train), "cuda") for train in (True, False)]
        torch.cuda.synchronize()
        build.append((time.perf_counter() - t0) * 1e3)
        nbytes = sum(d.flat.numel() for d in dds)
        del dds
    rows.append(dict(what="resident default set: DeviceDataset of 4096 train + 1024 test frames, wall clock, first run includes the allocation",
                     runs_ms=[round(v, 1) for v in build], bytes=int(nbytes)))
    name = torch.cuda.get_device_name(0)
    with open(args.out, "w") as f:
        f.write(f"# scripts/bench_partsworld.py --reps {args.reps} on {name}\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
