"""GPU: the ModifiedResNet backbones end to end -- RN-tiny features in every PREC against the
plain-torch restatement (tests/resnet_util.py) in fp64, a batch permutation, one full-size RN50,
and the trainers that run on a ResNet (ZeroshotCLIP, CoOp, CoCoOp, LinearProbeCLIP) or refuse it
(IVLP, MaPLe, PromptSRC, LoRA).

fp32 / fp32s gate: max |d| <= 8 x the restatement's own fp32-vs-fp64 error + 1e-7 max |ref| (the
form and factor of tests/test_lora_kernels_gpu.py); 16-bit gate: 1 - cos <= 5e-3.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import resnet_util as R

pytestmark = pytest.mark.gpu


def _encoder(sd, arch_name, prec, dev):
    from fsp_amd.clip import synth
    from fsp_amd.clip.model import ResNetEncoder
    return ResNetEncoder(sd, synth.ARCHS[arch_name], prec, dev)


@pytest.mark.parametrize("prec", ["fp32", "fp32s", "fp16", "bf16", "amp"])
@pytest.mark.parametrize("arch", ["RN-tiny", "RN-tiny-96"])
def test_rn_tiny_features(dev, arch, prec):
    sd, img, f64, f32 = R.reference(arch, 2)
    enc = _encoder(sd, arch, prec, dev)
    assert enc.input_resolution == int(arch == "RN-tiny-96") * 32 + 64 and enc.output_dim == 128
    got = enc(torch.from_numpy(img).to(dev))
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == (2, 128) and bool(torch.isfinite(got).all())
    err = float((got.double() - f64).abs().max())
    own = float((f32.double() - f64).abs().max())
    cos = R.cos_err(got, f64)
    print(f"{arch} {prec}: max |d| {err:.3e}, restatement fp32 vs fp64 {own:.3e} (ratio {err / own:.2f}), "
          f"1 - cos {cos:.3e}, max |ref| {float(f64.abs().max()):.3e}")
    if prec in ("fp32", "fp32s"):
        assert err <= 8 * own + 1e-7 * float(f64.abs().max())
    else:
        assert cos <= 5e-3
    with pytest.raises(RuntimeError):
        enc(torch.zeros(1, 3, 32, 32, device=dev))
    with pytest.raises(RuntimeError):
        enc(torch.from_numpy(img).to(dev).requires_grad_(True))
    with pytest.raises(ValueError):
        enc.forward_prompted(torch.from_numpy(img).to(dev), None)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_batch_permutation_is_bitwise(dev, prec):
    from fsp_amd.clip import synth
    sd = R.reference("RN-tiny-96", 2)[0]
    enc = _encoder(sd, "RN-tiny-96", prec, dev)
    img = torch.from_numpy(synth.make_images(3, 96, seed=9)).to(dev)
    perm = [2, 0, 1]
    a = enc(img)
    b = enc(img[perm].contiguous())
    assert torch.equal(a[perm], b)
    assert torch.equal(enc(img), a)  # and a second call agrees bitwise
    assert not torch.equal(a[0], a[1])


def test_full_rn50_fp16(dev):
    """The real channel counts and the 56 / 28 / 14 / 7 maps: RN50, B = 1, fp16, fp16-valued
    synthetic weights, against the fp32 CPU restatement."""
    sd, img, _, f32 = R.reference("RN50", 1, fp16_values=True)
    enc = _encoder(sd, "RN50", "fp16", dev)
    got = enc(torch.from_numpy(img).to(dev)).cpu()
    assert got.shape == (1, 1024) and bool(torch.isfinite(got).all())
    cos = R.cos_err(got, f32)
    print(f"RN50 fp16 B=1: 1 - cos {cos:.3e}, max |feat| {float(f32.abs().max()):.3e}")
    assert cos <= 5e-3


# ---------------------------------------------------------------- trainers
N_CLS = 6


def _cfg(trainer, outdir, backbone="RN-tiny", prec="fp32"):
    from fsp_amd.clip import synth
    from fsp_amd.engine.config import get_cfg_default
    cfg = get_cfg_default()
    res = synth.ARCHS[backbone].image_resolution
    cfg.INPUT.SIZE = (res, res)
    cfg.MODEL.BACKBONE.NAME = backbone
    cfg.DATASET.NAME = "Caltech101"
    cfg.OUTPUT_DIR = str(outdir)
    cfg.OPTIM.MAX_EPOCH = 1
    cfg.OPTIM.WARMUP_EPOCH = 1
    cfg.OPTIM.WARMUP_TYPE = "constant"
    cfg.OPTIM.LR = 0.01
    cfg.DATALOADER.TRAIN_X.BATCH_SIZE = 4
    cfg.TEST.NO_TEST = True
    cfg.TRAIN.PRINT_FREQ = 1
    cfg.TRAINER.NAME = trainer
    c = cfg.TRAINER.COOP
    c.N_CTX, c.CTX_INIT, c.PREC = 4, "", prec
    c = cfg.TRAINER.COCOOP
    c.N_CTX, c.CTX_INIT, c.PREC = 4, "a photo of a", prec
    for sec in ("LINEAR_PROBE", "IVLP", "MAPLE", "PROMPTSRC", "LORA"):
        cfg.TRAINER[sec].PREC = prec
    return cfg


def _build(trainer, cfg, dev):
    import fsp_amd.trainers  # noqa: F401
    from fsp_amd.data.synthetic import SyntheticDataManager
    from fsp_amd.engine.registry import TRAINER_REGISTRY
    dm = SyntheticDataManager(N_CLS, cfg.INPUT.SIZE[0], 4, n_batches=2, n_test=4, test_batch=4, device=dev)
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        return TRAINER_REGISTRY.get(trainer)(cfg, dm=dm)


def _epochs(tr, seen=None):
    losses = []
    fb = tr.forward_backward

    def step(batch):
        if seen is not None:
            seen.append((tr.epoch, batch))
        out = fb(batch)
        losses.append(float(out["loss"]))
        return out

    tr.forward_backward = step
    with contextlib.redirect_stdout(io.StringIO()):
        for tr.epoch in range(tr.max_epoch):
            tr.run_epoch()
            tr.after_epoch()
    tr.forward_backward = fb
    return losses


def test_zeroshot_clip_logits(dev, tmp_path):
    """fp32 logits within 1e-3 (the project's logit bar) of the restatement's image features
    composed with the oracle's text path."""
    from oracle import clip_oracle as O
    from fsp_amd.clip import synth
    from fsp_amd.clip.tokenizer import tokenize
    tr = _build("ZeroshotCLIP", _cfg("ZeroshotCLIP", tmp_path), dev)
    img = tr.dm.test_loader[0]["img"]
    with torch.no_grad():
        got = tr.model_inference(img).cpu()
    sd = synth.make_state_dict("RN-tiny", seed=0)
    p = {k: v for k, v in O.as_torch_sd(sd).items()}
    names = tr.dm.dataset.classnames
    tok = torch.from_numpy(tokenize([f"a photo of a {c}." for c in names]).astype(np.int64))
    with torch.no_grad():
        txt = O.normalize(O.encode_text(p, O.token_embed(p, tok), tok))
        imf = O.normalize(R.encode_image(sd, img.cpu().numpy(), torch.float64).float())
        want = float(np.exp(sd["logit_scale"])) * imf @ txt.t()
    err = float((got - want).abs().max())
    print(f"ZeroshotCLIP RN-tiny fp32: max |d logit| {err:.3e} (logits up to {float(want.abs().max()):.2f})")
    assert got.shape == (4, N_CLS)
    assert err <= 1e-3


@pytest.mark.parametrize("trainer", ["CoOp", "CoCoOp"])
def test_prompt_trainers_train_on_a_resnet(dev, tmp_path, trainer):
    tr = _build(trainer, _cfg(trainer, tmp_path / "rn"), dev)
    from fsp_amd.clip.model import ResNetEncoder
    assert isinstance(tr.model.image_encoder, ResNetEncoder)
    start = {k: p.detach().clone() for k, p in tr.model.prompt_learner.named_parameters()}
    assert "ctx" in start and (trainer == "CoOp" or "meta_net.linear1.weight" in start)
    losses = _epochs(tr)
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    for k, p in tr.model.prompt_learner.named_parameters():
        assert not torch.equal(p.detach(), start[k]), k  # it moved
        assert bool(torch.isfinite(p).all()), k
    ck = os.path.join(str(tmp_path / "rn"), "prompt_learner", "model.pth.tar-1")
    assert os.path.exists(ck)
    vit = _build(trainer, _cfg(trainer, tmp_path / "vit", backbone="tiny"), dev)
    _epochs(vit)
    keys_rn = sorted(tr.load_checkpoint(ck)["state_dict"])
    keys_vit = sorted(vit.load_checkpoint(os.path.join(str(tmp_path / "vit"), "prompt_learner",
                                                       "model.pth.tar-1"))["state_dict"])
    assert keys_rn == keys_vit
    with torch.no_grad():
        logits = tr.model_inference(tr.dm.test_loader[0]["img"])
    assert logits.shape == (4, N_CLS) and bool(torch.isfinite(logits).all())


def test_linear_probe_feature_cache(dev, tmp_path):
    cfg = _cfg("LinearProbeCLIP", tmp_path)
    cfg.OPTIM.MAX_EPOCH = 2
    cfg.TRAINER.LINEAR_PROBE.CACHE_FEATURES = True
    cfg.TRAINER.LINEAR_PROBE.CACHE_SHUFFLE = False
    tr = _build("LinearProbeCLIP", cfg, dev)
    first = []
    real = tr.model.image_features

    def counted(image):
        out = real(image)
        first.append((tr.epoch, out.detach().clone()))
        return out

    tr.model.image_features = counted
    seen = []
    losses = _epochs(tr, seen)
    assert len(losses) == 4 and all(np.isfinite(losses))
    assert [e for e, _ in first] == [0, 0]  # the ResNet ran in epoch 0 only
    replay = [b["feat"] for e, b in seen if e == 1]
    assert len(replay) == 2
    for (_, f0), f1 in zip(first, replay):
        assert f0.shape == (4, 128) and torch.equal(f0, f1)
    # and the encoder itself repeats bitwise
    again = real(tr.dm.train_loader_x[0]["img"])
    assert torch.equal(again, first[0][1])


@pytest.mark.parametrize("trainer", ["IVLP", "MaPLe", "PromptSRC", "LoRA"])
def test_vit_only_trainers_refuse_a_resnet(dev, tmp_path, trainer):
    with pytest.raises(ValueError, match="RN50"):
        _build(trainer, _cfg(trainer, tmp_path, backbone="RN50"), dev)
