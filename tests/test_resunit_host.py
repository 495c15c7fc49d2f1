"""Host side of the ResNet input heads: ``nn.ResidualUnit`` against the torch restatement of tests/resunit_ref.py (names, shapes,
initialisation), ``Generator(head=...)``, the arguments that are refused, the ``gen_head`` / ``gen_act`` hyper-parameters through a
checkpoint, the training states' parameter sets and the ``"head"`` / ``"act"`` keys of ``python -m unet_bssfp_amd.train``.  Modules
are built on the CPU and never called: the package has no CPU arithmetic."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resunit_ref as RR  # noqa: E402
from oracle import unet_ref as R  # noqa: E402

MODALITIES = ("dwi-tensor", "pc-bssfp", "bssfp", "t1w")
TINY = (4, 4, 8, 8, 16, 4)          # U-Net widths for the tests that only look at the heads


def _unit_keys(cin, cout, subunits=3, batch=True):
    keys = []
    for i in range(subunits):
        keys += [f"conv.unit{i}.conv.weight", f"conv.unit{i}.conv.bias", f"conv.unit{i}.adn.N.weight", f"conv.unit{i}.adn.N.bias"]
        if batch:
            keys += [f"conv.unit{i}.adn.N.{k}" for k in ("running_mean", "running_var", "num_batches_tracked")]
    return keys + (["residual.weight", "residual.bias"] if cin != cout else [])


@pytest.mark.parametrize("cin,cout", [(6, 24), (24, 24)])
@pytest.mark.parametrize("norm", ["BATCH", ("INSTANCE", {"affine": True})])
def test_state_dict_is_the_torch_restatements(cin, cout, norm):
    import unet_bssfp_amd as M
    batch = norm == "BATCH"
    torch.manual_seed(0)
    unit = M.ResidualUnit(3, cin, cout, subunits=3, act="RELU", norm=norm)
    after_unit = torch.rand(1)
    torch.manual_seed(0)
    ref = RR.RefResidualUnit(cin, cout, subunits=3, norm="batch" if batch else "instance")
    after_ref = torch.rand(1)
    sd, rsd = unit.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd) == _unit_keys(cin, cout, 3, batch)
    for k in sd:
        assert sd[k].shape == rsd[k].shape and sd[k].dtype == rsd[k].dtype, k
        assert torch.equal(sd[k], rsd[k]), k
    assert torch.equal(after_unit, after_ref)                      # the same random numbers were consumed
    assert sd["conv.unit0.conv.weight"].shape == (cout, cin, 3, 3, 3) and sd["conv.unit1.conv.weight"].shape == (cout, cout, 3, 3, 3)
    assert isinstance(unit.residual, torch.nn.Identity) == (cin == cout)
    if batch:
        assert sd["conv.unit2.adn.N.num_batches_tracked"].dtype == torch.long
    ref.load_state_dict(sd, strict=True), unit.load_state_dict(rsd, strict=True)


def test_default_is_two_subunits_and_the_fused_tail():
    import unet_bssfp_amd as M
    unit = M.ResidualUnit(3, 6, 24)
    assert list(unit.state_dict()) == _unit_keys(6, 24, 2) and M.ResidualUnit.fuse_tail is True


@pytest.mark.parametrize("kw", [dict(strides=2), dict(kernel_size=5), dict(dropout=0.1), dict(bias=False), dict(spatial_dims=2),
                                dict(act="PRELU"), dict(act=("prelu", {"init": 0.1})), dict(norm="INSTANCE"),
                                dict(norm=("INSTANCE", {"affine": False})), dict(norm="GROUP")])
def test_refused_arguments_raise(kw):
    import unet_bssfp_amd as M
    args = dict(spatial_dims=3, in_channels=6, out_channels=24)
    args.update(kw)
    with pytest.raises(NotImplementedError) as err:
        M.ResidualUnit(**args)
    assert "ResidualUnit" in str(err.value)


def test_generator_heads():
    import unet_bssfp_amd as M
    torch.manual_seed(0)
    gen = M.Generator("t1w", head="resnet", features=TINY)
    heads = [gen.blocks[m] for m in MODALITIES]
    assert all(isinstance(h, M.ResidualUnit) for h in heads) and len({id(h) for h in heads}) == 4
    assert [h.in_channels for h in heads] == [6, 24, 24, 6] and all(h.out_channels == 24 and h.subunits == 3 for h in heads)
    assert [isinstance(h.residual, M.Conv3d) for h in heads] == [True, False, False, True]
    torch.manual_seed(0)
    ref = RR.ref_generator("t1w", head="resnet", unet_cls=lambda **kw: R.RefBasicUNet(**dict(kw, features=TINY)))
    sd, rsd = gen.state_dict(), ref.state_dict()
    expected = [f"blocks.{m}.{k}" for m in MODALITIES for k in _unit_keys(RR.HEAD_CHANNELS[m], 24)]
    assert list(sd)[:len(expected)] == expected and list(sd) == list(rsd)
    assert all(torch.equal(sd[k], rsd[k]) for k in sd)             # same construction order, same initialisation
    with pytest.raises(ValueError):
        M.Generator("t1w", head="vit")


def test_conv_head_is_the_parents_network():
    import unet_bssfp_amd as M
    torch.manual_seed(3)
    gen, default = M.Generator("t1w", head="conv", features=TINY), None
    torch.manual_seed(3)
    default = M.Generator("t1w", features=TINY)
    torch.manual_seed(3)
    ref = R.RefGenerator("t1w", unet_cls=lambda **kw: R.RefBasicUNet(**dict(kw, features=TINY)))
    assert list(gen.state_dict()) == list(default.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in gen.state_dict().items())
    assert gen.blocks["bssfp"] is gen.blocks["pc-bssfp"] and gen.blocks["t1w"] is gen.blocks["dwi-tensor"]
    assert isinstance(gen.blocks["t1w"], M.DownSampleConv)


def test_fp8_is_refused_with_resnet_heads():
    import unet_bssfp_amd as M
    gen = M.Generator("bssfp", head="resnet", features=TINY)
    with pytest.raises(NotImplementedError):
        M.set_compute_dtype(gen, "fp8")
    M.set_compute_dtype(gen, "bf16")
    assert gen.blocks["bssfp"].compute_dtype == torch.bfloat16
    M.set_compute_dtype(M.Generator("bssfp", features=TINY), "fp8")     # (the reference's heads still take it)


def _model(**kw):
    from unet_bssfp_amd.gan import bSSFPToDWITensorModel
    return bSSFPToDWITensorModel("bssfp", optimizer_class=torch.optim.AdamW, **kw)


def test_hyper_parameters_and_checkpoint_round_trip(tmp_path):
    import unet_bssfp_amd as M
    from unet_bssfp_amd import checkpoint
    torch.manual_seed(1)
    plain = _model()
    hp = checkpoint.checkpoint_dict(plain)["hyper_parameters"]
    assert "gen_head" not in hp and "gen_act" not in hp and plain.gen.head == "conv"
    only_head = checkpoint.checkpoint_dict(_model(gen_head="resnet"))["hyper_parameters"]
    assert only_head["gen_head"] == "resnet" and "gen_act" not in only_head

    thesis = _model(gen_head="resnet", gen_act=("prelu", {"init": 0.2}))
    assert isinstance(thesis.gen.blocks["t1w"], M.ResidualUnit) and hasattr(thesis.gen.blocks["unet"].conv_0.conv_0.adn, "A")
    path = str(tmp_path / "thesis.ckpt")
    checkpoint.save_checkpoint(thesis, path)
    stored = torch.load(path, map_location="cpu", weights_only=True)["hyper_parameters"]       # plain containers only
    assert stored["gen_head"] == "resnet" and stored["gen_act"] == ["prelu", {"init": 0.2}]
    torch.manual_seed(2)                                            # (the rebuilt model's own initialisation must not matter)
    back, _info = checkpoint.load_from_checkpoint(path)             # strict: every key has to match
    assert back.gen_head == "resnet" and back.gen_act == ["prelu", {"init": 0.2}]
    sd, bsd = thesis.state_dict(), back.state_dict()
    assert list(sd) == list(bsd) and all(torch.equal(sd[k], bsd[k]) for k in sd)
    assert any(k.endswith("adn.A.weight") for k in bsd) and "gen.blocks.bssfp.conv.unit2.adn.N.running_var" in bsd
    handed = M.Generator("bssfp", head="resnet", act=("prelu", {"init": 0.2}))
    third, _info = checkpoint.load_from_checkpoint(path, gen=handed)            # a generator handed over replaces the stored description
    assert third.gen is handed and third.gen_head is None and torch.equal(handed.state_dict()["blocks.t1w.residual.weight"],
                                                                          sd["gen.blocks.t1w.residual.weight"])
    # an override rebuilds another architecture, which the stored weights then do not fit
    with pytest.raises(RuntimeError):
        checkpoint.load_from_checkpoint(path, gen_head="conv")

    # a file without the keys builds the parent's model
    old = str(tmp_path / "plain.ckpt")
    checkpoint.save_checkpoint(plain, old)
    again, _info = checkpoint.load_from_checkpoint(old)
    assert again.gen_head is None and again.gen_act is None and again.gen.head == "conv"
    assert list(again.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError):
        _model(gen=plain.gen, gen_head="resnet")


@pytest.mark.parametrize("modality", ["dwi-tensor", "bssfp"])
def test_transfer_trains_the_selected_head_only(modality):
    from unet_bssfp_amd import ddp, stages
    import unet_bssfp_amd as M
    model = _model(gen=M.Generator("bssfp", head="resnet", features=TINY), discr=torch.nn.Conv3d(30, 1, 1))
    gen = model.gen
    head = {id(p) for p in gen.blocks[modality].parameters()}
    unet = {id(p) for p in gen.blocks["unet"].parameters()}
    others = {id(p) for m in MODALITIES if m != modality for p in gen.blocks[m].parameters()}
    assert len(head) in (14, 12) and not (head & others) and not (head & unet)
    frozen = {id(p) for p in stages.frozen_parameters(stages.TrainingState.TRANSFER, gen)}
    assert frozen == unet
    assert {id(p) for p in ddp.used_parameters(gen, modality)} == head | unet
    assert {id(p) for p in ddp.used_parameters(gen, modality, frozen)} == head
    model.change_training_state("TRANSFER", modality)
    assert {id(p) for p in gen.parameters() if p.requires_grad} == head | others           # (the unused heads are not frozen, they are unused)
    late, early = M.nn.backward_stages(gen, modality, model._frozen)
    assert not late and {id(p) for p in early} == head
    gen_opt, _ = model.optimizers()
    assert {id(p) for grp in gen_opt.param_groups for p in grp["params"]} == head | others


def test_train_main_reads_head_and_act(tmp_path, monkeypatch):
    """the manifest's "head" / "act" reach the model that ``train_model`` builds (queues and the fit loop are stubs)"""
    from unet_bssfp_amd import data, train
    import unet_bssfp_amd as M
    seen = {}

    class StubTrainer:
        def __init__(self, **kw):
            pass

        def fit(self, model, train_queue, val_queue):
            seen["model"] = model

    monkeypatch.setattr(data, "subjects_from_nifti", lambda files, device: files)
    monkeypatch.setattr(data, "PatchQueue", lambda subjects, modality, seed=0: ("queue", modality))
    monkeypatch.setattr(train, "Trainer", StubTrainer)
    manifest = {"modality": "t1w", "dirpath": str(tmp_path), "train": [{}], "val": [], "device": "cpu", "head": "resnet", "act": "prelu"}
    path = tmp_path / "manifest.json"
    path.write_text(json.dumps(manifest))
    assert train.main([str(path)]) == 0
    model = seen["model"]
    assert model.gen_head == "resnet" and model.gen_act == "prelu" and model.input_modality == "t1w"
    assert isinstance(model.gen.blocks["t1w"], M.ResidualUnit) and hasattr(model.gen.blocks["unet"].conv_0.conv_0.adn, "A")
    del manifest["head"], manifest["act"]
    path.write_text(json.dumps(manifest))
    assert train.main([str(path)]) == 0
    assert seen["model"].gen_head is None and isinstance(seen["model"].gen.blocks["t1w"], M.DownSampleConv)
