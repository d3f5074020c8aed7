"""A plain-torch restatement of OpenAI CLIP's ModifiedResNet (PromptSRC/clip/model.py:10-150),
built from a state dict and runnable in fp64 and fp32 on the CPU: the reference of the ResNet
backbone tests. It follows the definition, not the native code: NCHW, F.conv2d / F.avg_pool2d, the
BatchNorm formula, and an attention pool written out (checked against
F.multi_head_attention_forward in test_resnet_cpu.py)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def to_torch(sd, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def batch_norm(p, key, x):
    """Eval-mode BatchNorm2d: (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias."""
    v = lambda n: p[f"{key}.{n}"][None, :, None, None]
    return (x - v("running_mean")) / torch.sqrt(v("running_var") + 1e-5) * v("weight") + v("bias")


def bottleneck(p, pre, x, stride):
    out = F.relu(batch_norm(p, pre + "bn1", F.conv2d(x, p[pre + "conv1.weight"])))
    out = F.relu(batch_norm(p, pre + "bn2", F.conv2d(out, p[pre + "conv2.weight"], padding=1)))
    if stride > 1:
        out = F.avg_pool2d(out, stride)
    out = batch_norm(p, pre + "bn3", F.conv2d(out, p[pre + "conv3.weight"]))
    identity = x
    if pre + "downsample.0.weight" in p:
        identity = F.avg_pool2d(x, stride) if stride > 1 else x
        identity = batch_norm(p, pre + "downsample.1", F.conv2d(identity, p[pre + "downsample.0.weight"]))
    return F.relu(out + identity)


def attnpool(p, x, heads, pre="visual.attnpool."):
    """AttentionPool2d on tokens x [B, HW, C]: the mean token is prepended and is the only query."""
    B, HW, C = x.shape
    x = torch.cat([x.mean(1, keepdim=True), x], 1) + p[pre + "positional_embedding"]
    q = x[:, :1] @ p[pre + "q_proj.weight"].t() + p[pre + "q_proj.bias"]
    k = x @ p[pre + "k_proj.weight"].t() + p[pre + "k_proj.bias"]
    v = x @ p[pre + "v_proj.weight"].t() + p[pre + "v_proj.bias"]
    hd = C // heads
    q = q.reshape(B, 1, heads, hd).transpose(1, 2) * hd ** -0.5
    k = k.reshape(B, HW + 1, heads, hd).transpose(1, 2)
    v = v.reshape(B, HW + 1, heads, hd).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2), -1)
    o = (a @ v).transpose(1, 2).reshape(B, C)
    return o @ p[pre + "c_proj.weight"].t() + p[pre + "c_proj.bias"]


def stem(p, image):
    x = image
    for k, stride in ((1, 2), (2, 1), (3, 1)):
        x = F.relu(batch_norm(p, f"visual.bn{k}", F.conv2d(x, p[f"visual.conv{k}.weight"], stride=stride, padding=1)))
    return F.avg_pool2d(x, 2)


def block_counts(p):
    return tuple(len({k.split(".")[2] for k in p if k.startswith(f"visual.layer{b}.")}) for b in (1, 2, 3, 4))


def encode_image(sd, image, dtype=torch.float64):
    """ModifiedResNet.forward: image [B,3,R,R] -> [B, E] in ``dtype`` (weights and image cast to it)."""
    p = to_torch(sd, dtype)
    x = stem(p, torch.as_tensor(np.asarray(image)).to(dtype))
    for l, n in enumerate(block_counts(p), 1):
        for i in range(n):
            x = bottleneck(p, f"visual.layer{l}.{i}.", x, 2 if (l > 1 and i == 0) else 1)
    B, C = x.shape[:2]
    return attnpool(p, x.reshape(B, C, -1).permute(0, 2, 1), C // 64)


@functools.lru_cache(maxsize=None)
def reference(arch, n_images, fp16_values=False, seed=0):
    """(state dict, images, fp64 features, fp32 features) of a synthetic backbone, computed once
    and shared by the tests that need them; callers must not modify them."""
    from fsp_amd.clip import synth
    sd = synth.make_state_dict(arch, seed=seed, fp16_values=fp16_values)
    img = synth.make_images(n_images, synth.ARCHS[arch].image_resolution, seed=1)
    with torch.no_grad():
        f64 = encode_image(sd, img, torch.float64)
        f32 = encode_image(sd, img, torch.float32)
    return sd, img, f64, f32


def cos_err(a, b):
    a, b = a.double(), b.double()
    return float((1.0 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())
