"""Record the golden vectors of the variational-dropout U-Net from the REFERENCE modules (authoring machine only: needs the
reference checkout; never runs where the tests run).

    python tools/gen_bayes_golden.py /path/to/reference

The reference's two files (segmentation/models/3d_bayes_layers.py, 3d_bayes_unet.py) have names Python cannot import, and the
U-Net file does `from .layers import *`: both are loaded by path into a made-up package, the layers module registered as
`<pkg>.layers` before the U-Net file executes.  The reference draws its noise with `Tensor.normal_()` inside forward; that call is
wrapped to capture the noise of the train-mode run (and to replay the same tensors in the eval-mode run, so one set serves both).
tests/bayes_ref.py, fed the captured noise, must then equal the reference bit for bit: outputs, loss and every gradient.

Writes tests/golden/bayes_unet.npz (input seed, noise, sampled outputs, loss, per-parameter gradient norms; bayes=True train and
eval, bayes=False train) and tests/golden/bayes_state_keys.json (state_dict keys and shapes of the four variants).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bayes_ref  # noqa: E402
from util import grad_norms, param_checksum, sample, seeded_randn  # noqa: E402

CHANNELS = [1, 4, 8, 8, 16]
SHAPE = (1, 1, 16, 16, 32)
MODEL_SEED, INPUT_SEED = 0, 41


def load_reference(ref_root):
    models = os.path.join(ref_root, "segmentation", "models")
    pkg = types.ModuleType("ref_bayes")
    pkg.__path__ = [models]
    sys.modules["ref_bayes"] = pkg
    out = []
    for name, fname in (("layers", "3d_bayes_layers.py"), ("unet", "3d_bayes_unet.py")):
        spec = importlib.util.spec_from_file_location("ref_bayes." + name, os.path.join(models, fname))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_bayes." + name] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


class NormalTap:
    """Wraps torch.Tensor.normal_ while active: records what the reference draws, or replays a recorded list."""

    def __init__(self, replay=None):
        self.replay, self.seen = replay, []

    def __enter__(self):
        self.orig = orig = torch.Tensor.normal_
        tap = self

        def normal_(t, *a, **k):
            if tap.replay is not None:
                t.copy_(tap.replay[len(tap.seen)])
            else:
                orig(t, *a, **k)
            tap.seen.append(t.detach().clone())
            return t
        torch.Tensor.normal_ = normal_
        return self

    def __exit__(self, *exc):
        torch.Tensor.normal_ = self.orig
        return False


def step(model, x, train):
    model.train(train)
    model.zero_grad(set_to_none=True)
    out = model(x)
    loss = (out ** 2).mean()
    loss.backward()
    return out.detach(), loss.detach()


def record(ref_unet, bayes, train, noise):
    torch.manual_seed(MODEL_SEED)
    ref = ref_unet.UNet3D(2, CHANNELS, bayes=bayes, shorten=True)
    torch.manual_seed(MODEL_SEED)
    mine = bayes_ref.UNet3D(2, CHANNELS, bayes=bayes, shorten=True)
    assert list(ref.state_dict()) == list(mine.state_dict())
    for (k, a), b in zip(ref.state_dict().items(), mine.state_dict().values()):
        assert torch.equal(a, b), "same seed, different initial %s" % k
    x = seeded_randn(INPUT_SEED, SHAPE)
    with NormalTap(noise) as tap:
        out_r, loss_r = step(ref, x, train)
    tape = bayes_ref.NoiseTape(tap.seen).install(mine)
    out_m, loss_m = step(mine, x, train)
    assert tape.pos == len(tap.seen)
    assert torch.equal(out_r, out_m) and torch.equal(loss_r, loss_m), "restatement differs from the reference"
    for (k, a), b in zip(ref.named_parameters(), mine.parameters()):
        assert torch.equal(a.grad, b.grad), "gradient of %s differs from the reference" % k
    smp, stride = sample(out_r)
    rec = {"out_sample": smp, "out_stride": np.int64(stride), "out_shape": np.array(out_r.shape), "loss": np.float64(loss_r.item()),
           "grad_norms": grad_norms(ref), "param_checksum": param_checksum(ref)}
    return rec, tap.seen


def main(ref_root):
    _, ref_unet = load_reference(ref_root)
    data = {"input_seed": np.int64(INPUT_SEED), "model_seed": np.int64(MODEL_SEED), "shape": np.array(SHAPE), "channels": np.array(CHANNELS)}
    rec, noise = record(ref_unet, True, True, None)
    assert len(noise) == 19
    data.update({"bayes_train_" + k: v for k, v in rec.items()})
    data.update({"noise_%02d" % i: t.numpy() for i, t in enumerate(noise)})
    rec, seen = record(ref_unet, True, False, noise)
    assert all(torch.equal(a, b) for a, b in zip(seen, noise))
    data.update({"bayes_eval_" + k: v for k, v in rec.items()})
    rec, seen = record(ref_unet, False, True, None)
    assert not seen
    data.update({"plain_train_" + k: v for k, v in rec.items()})
    gold = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(gold, "bayes_unet.npz"), **data)
    keys = {}
    for shorten in (False, True):
        for bayes in (False, True):
            m = ref_unet.UNet3D(2, CHANNELS, bayes=bayes, shorten=shorten)
            keys["shorten=%s,bayes=%s" % (shorten, bayes)] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(gold, "bayes_state_keys.json"), "w") as f:
        json.dump({"n_classes": 2, "n_channels": CHANNELS, "variants": keys}, f, indent=0)
    print("wrote bayes_unet.npz (%d bytes), bayes_state_keys.json" % os.path.getsize(os.path.join(gold, "bayes_unet.npz")))


if __name__ == "__main__":
    main(sys.argv[1])
