"""tests/golden/train_args.json from the REFERENCE's own argument parser, run in the build container:

    python tests/golden/make_golden_args.py [OUT.json]

Imports /root/reference/main.py (its module level only builds nothing: the parser is a function) and writes, for every action of
main.get_args_parser(), {dest: {"default": ..., "type": name of the type callable or null}}: settings only, no program text.
protopformer_amd.train.get_args_parser is held to this table by tests/test_train_driver_cpu.py.

Modules main.py imports that are absent here are replaced by stand-ins through sys.modules, for their NAMES only (nothing of them runs
while a parser is built): timm (models through _timm_standins.py; data / loss / utils / scheduler names), torch.utils.tensorboard,
torchvision, cv2."""
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)


def _install_standins():
    import _timm_standins as standins
    standins.install(REF)

    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class Name:                                # a class that can be imported, subclassed and never used
        def __init__(self, *a, **k):
            raise RuntimeError("stand-in: not available in the build container")

    mod("timm.data", Mixup=Name, create_transform=None)
    mod("timm.data.constants", IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225))
    mod("timm.loss", LabelSmoothingCrossEntropy=Name, SoftTargetCrossEntropy=Name)
    mod("timm.utils", NativeScaler=Name, get_state_dict=None, ModelEma=Name, accuracy=None)
    mod("timm.scheduler", CosineLRScheduler=Name, StepLRScheduler=Name)
    mod("torch.utils.tensorboard", SummaryWriter=Name)
    folder = mod("torchvision.datasets.folder", ImageFolder=Name, default_loader=None)
    utils = mod("torchvision.datasets.utils", download_url=None, extract_archive=None, list_dir=None, download_and_extract_archive=None,
                verify_str_arg=None)
    datasets = mod("torchvision.datasets", VisionDataset=Name, folder=folder, utils=utils, ImageFolder=Name)
    transforms = mod("torchvision.transforms")
    mod("torchvision", datasets=datasets, transforms=transforms)
    mod("cv2", transform=None)


def table():
    _install_standins()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import main as ref_main                    # the reference's main.py
    out = {}
    for act in ref_main.get_args_parser()._actions:
        entry = {"default": act.default, "type": getattr(act.type, "__name__", None) if act.type is not None else None}
        if act.dest in out:                    # --model_ema / --no-model-ema, --pin-mem / --no-pin-mem: one dest, the parser's final default
            assert out[act.dest]["type"] == entry["type"]
        out[act.dest] = entry
    defaults = vars(ref_main.get_args_parser().parse_args([]))
    for dest, entry in out.items():
        entry["default"] = defaults[dest]      # after set_defaults()
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "train_args.json")
    with open(path, "w") as f:
        json.dump(table(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(json.load(open(path)))} dests")


if __name__ == "__main__":
    main()
