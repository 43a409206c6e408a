"""protopformer_amd.tooling: what the command-line tools set up alike -- the "stop after N images" iteration, and the model built from
the training flags.  No GPU: list "loaders" and CPU construction only."""
import pytest
import torch

from protopformer_amd import tooling as T


def _loader(width):
    """Three batches of 4 images; `width` elements per batch tuple: (x,), or (x, y, ids) with ids a list as a collate may leave it."""
    x = torch.arange(12.0).reshape(12, 1)
    full = [(x[i:i + 4], x[i:i + 4, 0].long() * 10, list(range(100 + i, 104 + i))) for i in range(0, 12, 4)]
    return [b[:width] for b in full]


@pytest.mark.parametrize("width", [3, 1])
@pytest.mark.parametrize("max_images, sizes", [(0, [4, 4, 4]), (None, [4, 4, 4]), (3, [3]), (4, [4]), (6, [4, 2]), (100, [4, 4, 4])])
def test_take_images_counts_truncates_every_element_and_stops(width, max_images, sizes):
    loader = _loader(width)
    pulled = []

    def counting():
        for b in loader:
            pulled.append(1)
            yield b

    got = list(T.take_images(counting(), max_images))
    assert [len(b) for b in got] == [width] * len(sizes)
    assert [b[0].shape[0] for b in got] == sizes
    n = sum(sizes)
    assert torch.equal(torch.cat([b[0] for b in got]), torch.arange(float(n)).reshape(n, 1))
    for b in got:                                                   # every element of a batch is cut to the same images
        if width == 3:
            assert b[1].tolist() == [int(v) * 10 for v in b[0][:, 0]] and list(b[2]) == [100 + int(v) for v in b[0][:, 0]]
    assert len(pulled) == len(sizes)                                # nothing is pulled after the batch that reaches the count


def test_regroup_over_take_images():
    from protopformer_amd.interpret import _regroup
    x = torch.arange(14.0).reshape(14, 1)
    passes = list(_regroup([(x[i:i + 4], None) for i in range(0, 14, 4)], 3, 10))
    assert [p.shape[0] for p in passes] == [3, 3, 3, 1]
    assert torch.equal(torch.cat(passes), x[:10]) and all(p.dtype == torch.float32 and p.is_contiguous() for p in passes)


def _args(*argv):
    from protopformer_amd.train import get_args_parser
    return get_args_parser().parse_args(list(argv))


def test_model_from_args_is_the_call_the_tools_spelled_out():
    from protopformer_amd.protopformer import construct_PPNet
    # the parser's defaults, and the three flags without which no PPNet is built (use_global with one reserve layer)
    args = _args("--no-pretrained", "--base_architecture", "deit_tiny_patch16_224", "--use_global", "true", "--reserve_layers", "11",
                 "--reserve_token_nums", "81")
    ref = construct_PPNet(base_architecture=args.base_architecture, pretrained=not args.no_pretrained, img_size=args.img_size,
                          prototype_shape=args.prototype_shape, num_classes=200, reserve_layers=args.reserve_layers,
                          reserve_token_nums=args.reserve_token_nums, use_global=args.use_global, use_ppc_loss=args.use_ppc_loss,
                          ppc_cov_thresh=args.ppc_cov_thresh, ppc_mean_thresh=args.ppc_mean_thresh, global_coe=args.global_coe,
                          global_proto_per_class=args.global_proto_per_class,
                          prototype_activation_function=args.prototype_activation_function, add_on_layers_type=args.add_on_layers_type)
    got = T.model_from_args(args, 200)
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    assert shapes(got) == shapes(ref) and list(got.state_dict()) == list(ref.state_dict())
    assert got.img_size == ref.img_size == 224 and got.num_classes == 200


def test_model_from_args_overrides(monkeypatch):
    """interp_eval's case: its parser has --input_size and neither --img_size nor --no-pretrained."""
    import protopformer_amd.protopformer as PP
    seen = {}
    monkeypatch.setattr(PP, "construct_PPNet", lambda **kw: seen.update(kw) or "model")
    args = _args("--no-pretrained", "--use_global", "true", "--reserve_layers", "11", "--reserve_token_nums", "81")
    assert T.model_from_args(args, 7) == "model"
    assert seen["pretrained"] is False and seen["img_size"] == 224 and seen["num_classes"] == 7 and seen["use_global"] is True
    assert seen["reserve_layers"] == [11] and seen["reserve_token_nums"] == [81] and len(seen) == 15
    T.model_from_args(args, 7, img_size=96, pretrained=True)
    assert seen["pretrained"] is True and seen["img_size"] == 96
    del args.img_size, args.no_pretrained
    T.model_from_args(args, 7, img_size=64, pretrained=True)
    assert seen["img_size"] == 64
