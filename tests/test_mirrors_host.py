"""CPU-only checks that the two model mirrors (model.py: VGG16, new_model.py: ResNet-50-FPN) stay ONE implementation with two sets of
constants: the detector methods live in a shared base, and the four target makers hand ops.rpn_targets / ops.head_targets exactly the
arguments the two separate copies did.  Every expected value below is written down from those copies, not read from the package."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = ("predict", "detect", "_suppress", "count_parameters", "check_device_status")
# mirror -> (variant, label_offset, max_pos, total), the short-sample message, forward's argument names (head maker, RPN maker)
HEAD = {"vgg": ((0, 1, 32, 128), "FastRcnnTargetMaker: fewer than 128 samples (the reference fails here too, model_.py:340)",
                ["self", "bbox", "label", "rois", "n_rois", "n_gt", "empty"], ["self", "bbox", "anchor", "n_gt"]),
        "fpn": ((1, 0, 128, 512), "FRCNNTargetMaker: fewer than 512 samples (assert at new_model.py:183)",
                ["self", "boxes", "labels", "rois", "n_rois", "n_gt", "empty"], ["self", "boxes", "anchors", "n_gt"])}
N_ANCHORS, N_ROIS, G = 40, 30, 3


@pytest.fixture(scope="module")
def mirrors():
    if not os.path.exists(os.path.join(ROOT, "faster_rcnn_pytorch_amd", "lib", "libfrcnn_hip.so")):
        import __graft_entry__ as g
        g.build()
    from faster_rcnn_pytorch_amd import model, new_model
    vgg, fpn = model.FRCNN(num_classes=3), new_model.FRCNN(num_classes=3)
    return {"vgg": (model, vgg, vgg.rpn_target_maker, vgg.fast_rcnn_target_maker),
            "fpn": (new_model, fpn, fpn.rpn_target_maker, fpn.frcnn_target_maker)}


def test_the_detector_methods_are_written_once(mirrors):
    from faster_rcnn_pytorch_amd import model
    vgg, fpn = mirrors["vgg"][1], mirrors["fpn"][1]
    shared = [c for c in type(vgg).__mro__ if c in type(fpn).__mro__ and c.__module__ == model.__name__]
    assert shared and all(issubclass(c, torch.nn.Module) for c in shared)
    assert not list(shared[0]().parameters())                                   # the base has no parameters of its own
    for name in SHARED:
        assert name not in vars(type(vgg)) and name not in vars(type(fpn)), name
        assert any(name in vars(c) for c in shared), name
        assert getattr(type(vgg), name) is getattr(type(fpn), name)
    for m in (vgg, fpn):                                                        # what stays per mirror
        assert "forward" in vars(type(m)) and "graph_stages" in vars(type(m))
        assert m.rpn_target_maker.sampler is m.sampler and m.last_proposal_count is None
    assert vgg.fast_rcnn_target_maker.sampler is vgg.sampler and fpn.frcnn_target_maker.sampler is fpn.sampler
    assert vgg.count_parameters() == sum(p.numel() for p in vgg.parameters() if p.requires_grad)


def test_target_maker_signatures_keep_the_mirrors_names(mirrors):
    for key, (_, _, rpn_maker, head_maker) in mirrors.items():
        assert list(inspect.signature(type(head_maker).forward).parameters) == HEAD[key][2]
        assert list(inspect.signature(type(rpn_maker).forward).parameters) == HEAD[key][3]


class _Recorder(object):
    """Stands in for ops.rpn_targets / ops.head_targets: binds each call against the real signature (so a default counts as the value
    that arrives and an unknown keyword fails), records it, and returns correctly shaped CPU tensors with the counts it was told."""

    def __init__(self, real, counts):
        self.sig, self.counts, self.calls = inspect.signature(real), counts, []

    def __call__(self, *a, **kw):
        b = self.sig.bind(*a, **kw)
        passed = set(b.arguments)
        b.apply_defaults()
        self.calls.append((dict(b.arguments), passed))
        n = b.arguments.get("total", N_ANCHORS)
        out = (torch.zeros(n, dtype=torch.int64), torch.zeros(n, 4))
        counts = torch.tensor(self.counts, dtype=torch.int32)
        return out + ((torch.zeros(n, 4), None, counts) if "total" in b.arguments else (counts,))


def _inputs():
    g = torch.Generator().manual_seed(0)
    return {"anchor": torch.rand(N_ANCHORS, 4, generator=g), "rois": torch.rand(N_ROIS, 4, generator=g), "bbox": torch.rand(G, 4, generator=g),
            "label": torch.tensor([1, 2, 1], dtype=torch.int32), "n_rois": torch.tensor([N_ROIS], dtype=torch.int32),
            "n_gt": torch.tensor([G], dtype=torch.int32), "empty": torch.zeros(1, dtype=torch.int32)}


@pytest.mark.parametrize("key", ["vgg", "fpn"])
def test_head_target_maker_constants_and_sampling_branches(mirrors, monkeypatch, key):
    from faster_rcnn_pytorch_amd import ops
    _, m, _, maker = mirrors[key]
    (variant, label_offset, max_pos, total), message = HEAD[key][:2]
    t = _inputs()

    def run(sampling, counts):
        rec = _Recorder(ops.head_targets, counts)
        monkeypatch.setattr(ops, "head_targets", rec)
        monkeypatch.setattr(m.sampler, "sampling", sampling)
        try:
            return rec.calls, maker([t["bbox"]], [t["label"]], t["rois"], n_rois=t["n_rois"], n_gt=t["n_gt"], empty=t["empty"])
        finally:
            monkeypatch.undo()

    def common(a):
        assert a["rois"] is t["rois"] and a["gt"] is t["bbox"]                    # the one-element lists are unwrapped
        assert a["gt_label"].dtype == torch.int64 and a["gt_label"].tolist() == [1, 2, 1]
        assert (a["variant"], a["label_offset"], a["max_pos"], a["total"]) == (variant, label_offset, max_pos, total)
        assert a["n_rois"] is t["n_rois"] and a["n_gt"] is t["n_gt"] and not a["want_keep"]

    calls, out = run("device", [7, 11, total, 0])
    assert len(calls) == 1 and len(out) == 3 and out[0].shape == (total,) and out[2].shape == (total, 4)
    a, passed = calls[0]
    common(a)
    assert a["philox_state"] is m.sampler.state(t["rois"].device) and a["status"] is m.sampler.status.word(t["rois"].device)
    assert a["empty"] is t["empty"] and not passed & {"perm_pos", "perm_neg", "seed", "offset"}

    torch.manual_seed(3)
    calls, out = run("host", [7, 11, total, 0])
    torch.manual_seed(3)
    want_pos, want_neg = torch.randperm(7), torch.randperm(11)                   # positives first: the reference's RNG stream
    assert len(calls) == 2 and len(out) == 3
    for a, passed in calls:
        common(a)
        assert not passed & {"philox_state", "status", "seed", "offset"}
    assert not calls[0][1] & {"perm_pos", "perm_neg"} and calls[0][0]["empty"] is None      # the counting call writes nothing
    assert torch.equal(calls[1][0]["perm_pos"], want_pos) and torch.equal(calls[1][0]["perm_neg"], want_neg)
    assert calls[1][0]["empty"] is t["empty"]

    with pytest.raises(RuntimeError, match="^" + re.escape(message) + "$"):
        run("host", [7, 11, total - 1, 0])
    run("device", [7, 11, total - 1, 0])                                         # device mode reports through the status word, not here


@pytest.mark.parametrize("key", ["vgg", "fpn"])
def test_rpn_target_maker_variant_and_sampling_branches(mirrors, monkeypatch, key):
    from faster_rcnn_pytorch_amd import ops
    _, m, maker, _ = mirrors[key]
    variant = HEAD[key][0][0]
    t = _inputs()

    def run(sampling, counts):
        rec = _Recorder(ops.rpn_targets, counts)
        monkeypatch.setattr(ops, "rpn_targets", rec)
        monkeypatch.setattr(m.sampler, "sampling", sampling)
        try:
            return rec.calls, maker([t["bbox"]], t["anchor"], n_gt=t["n_gt"])
        finally:
            monkeypatch.undo()

    calls, out = run("device", [200, 5000, 0, 0])
    assert len(calls) == 1 and len(out) == 2 and out[0].shape == (N_ANCHORS,) and out[1].shape == (N_ANCHORS, 4)
    a, passed = calls[0]
    assert a["anchors"] is t["anchor"] and a["gt"] is t["bbox"] and a["variant"] == variant and a["n_gt"] is t["n_gt"]
    assert a["philox_state"] is m.sampler.state(t["anchor"].device) and not passed & {"perm_pos", "perm_neg", "seed", "offset"}

    # (n_pos, n_neg) -> which permutations are drawn: positives only above 128, negatives only above 256 - n_pos
    for (n_pos, n_neg), (draw_pos, draw_neg) in {(200, 5000): (True, True), (129, 128): (True, True), (128, 129): (False, True),
                                                 (100, 5000): (False, True), (128, 128): (False, False), (100, 156): (False, False),
                                                 (200, 56): (True, False), (10, 100): (False, False), (0, 0): (False, False)}.items():
        torch.manual_seed(5)
        calls, out = run("host", [n_pos, n_neg, 0, 0])
        torch.manual_seed(5)
        want_pos = torch.randperm(n_pos) if draw_pos else None
        want_neg = torch.randperm(n_neg) if draw_neg else None
        assert len(calls) == 2 and len(out) == 2
        for a, passed in calls:
            assert a["anchors"] is t["anchor"] and a["gt"] is t["bbox"] and a["variant"] == variant and a["n_gt"] is t["n_gt"]
            assert not passed & {"philox_state", "seed", "offset"}
        assert not calls[0][1] & {"perm_pos", "perm_neg"}
        for name, want in (("perm_pos", want_pos), ("perm_neg", want_neg)):
            got = calls[1][0][name]
            assert (got is None) if want is None else torch.equal(got, want), (n_pos, n_neg, name)

    with pytest.raises(RuntimeError, match="^RPNTargetMaker: permutation length mismatch$"):
        run("host", [10, 100, 1, 0])
    with pytest.raises(RuntimeError, match=r"^RPNTargetMaker: n_gt outside \[1, %d\]$" % G):
        run("host", [10, 100, 16, 0])                                            # RPN_ERR_GT_COUNT alone


def test_proposal_tables_and_rpn_head_reference_form(mirrors):
    model, new_model = mirrors["vgg"][0], mirrors["fpn"][0]
    assert (model.RegionProposal.top_k("test"), model.RegionProposal.top_k("train")) == ((6000, 300), (12000, 2000))
    assert (new_model.RegionProposalNetwork.top_k("test"), new_model.RegionProposalNetwork.top_k("train")) == ((2000, 1000), (4000, 1000))
    torch.manual_seed(1)
    for head, channels, anchors in ((mirrors["vgg"][1].rpn, 512, 9), (mirrors["fpn"][1].rpn.rpn_head, 256, 3)):
        assert [n for n, _ in head.named_parameters()] == ["inter_layer.weight", "inter_layer.bias", "cls_layer.weight", "cls_layer.bias",
                                                           "reg_layer.weight", "reg_layer.bias"]
        x = torch.randn(2, channels, 3, 5)
        with torch.no_grad():
            cls, reg = head(x)                                                   # on the CPU both heads take the reference form
            h = torch.relu(torch.nn.functional.conv2d(x, head.inter_layer.weight, head.inter_layer.bias, padding=1))
            want_cls = torch.nn.functional.conv2d(h, head.cls_layer.weight, head.cls_layer.bias).permute(0, 2, 3, 1).reshape(2, -1, 2)
            want_reg = torch.nn.functional.conv2d(h, head.reg_layer.weight, head.reg_layer.bias).permute(0, 2, 3, 1).reshape(2, -1, 4)
        assert cls.shape == (2, 15 * anchors, 2) and reg.shape == (2, 15 * anchors, 4)
        assert torch.equal(cls, want_cls) and torch.equal(reg, want_reg)
    assert type(mirrors["fpn"][1].rpn.rpn_head).forward is type(mirrors["vgg"][1].rpn).__mro__[1].forward      # one reference form
