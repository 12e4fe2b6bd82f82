"""Monte-Carlo predictive inference: sample a stochastic model's forward pass and read out a prediction with its uncertainty.

The stochastic models here are ``UNet3D(bayes=True)`` (``BayesConv3d`` draws its noise in train AND eval mode), ``Modified3DUNet``
(``Dropout3d(0.6)``) and ``unet.UNet(monte_carlo_dropout=p)``.  ``mc_predict`` runs the draws; ``MCAccumulator`` folds each
draw's logits into per-voxel sums on the device (``ops.mc_accumulate``) and turns them into

  mean         (N, C, D, H, W)  mean over draws of softmax(logits)
  variance     (N, C, D, H, W)  population variance of the class probabilities over draws
  entropy      (N, D, H, W)     predictive entropy  H[mean]                              (total uncertainty, nats)
  mutual_info  (N, D, H, W)     H[mean] - mean over draws of H[softmax(logits)]          (the model's share of it, BALD)
  mask         (N, D, H, W)     uint8 arg-max of the mean

in one pass (``ops.mc_finalize``).  No logits, probabilities or per-draw maps are kept: the state is 2C + 1 floats per voxel.
"""
import torch
import torch.nn as tnn

from .. import ops

OUTPUTS = ops.MC_OUTPUTS


class MCAccumulator:
    """Owner of the accumulation state for logits of logical shape `shape` = (N, C, D, H, W) on `device`."""

    def __init__(self, shape, device):
        self.shape = tuple(int(s) for s in shape)
        self.state = ops.mc_state(self.shape, device)
        self._samples = 0

    @property
    def samples(self):
        return self._samples

    def reset(self):
        """Forget every draw (the next `add` overwrites the state; nothing is cleared)."""
        self._samples = 0

    def add(self, logits, reps=1):
        """Fold in `reps` draws stacked along the batch: `logits` is (reps*N, C, D, H, W), draw r of volume n at r*N + n."""
        n, rest = self.shape[0], self.shape[1:]
        if tuple(logits.shape) != (reps * n,) + rest:
            raise RuntimeError("MCAccumulator.add: expected logits of shape %s for reps=%d, got %s"
                               % ((reps * n,) + rest, reps, tuple(logits.shape)))
        ops.mc_accumulate(self.state, logits, first=self._samples == 0, reps=reps)
        self._samples += reps

    def result(self, want=OUTPUTS):
        if self._samples == 0:
            raise RuntimeError("MCAccumulator.result: no draw has been added")
        out = ops.mc_finalize(self.state, self.shape, self._samples, want)
        out["samples"] = self._samples      # how many draws the maps are statistics of
        return out


class _sampling_mode:
    """model.eval() with (optionally) every Dropout3d back in train mode; every module's previous mode is restored on exit."""

    def __init__(self, model, dropout):
        self.model, self.dropout = model, dropout

    def __enter__(self):
        self.modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        if self.dropout:
            for m, _ in self.modes:
                if isinstance(m, tnn.Dropout3d):     # the package's Dropout3d derives from torch's
                    m.train()
        return self

    def __exit__(self, *exc):
        for m, was in self.modes:
            m.training = was
        return False


def mc_predict(model, inputs, n_samples, samples_per_pass=1, dropout=True, want=OUTPUTS):
    """`n_samples` stochastic forward passes of `model` on `inputs` (N, Cin, D, H, W) -> the dict of `MCAccumulator.result`
    (the entries of `want`, and "samples" = n_samples).

    The model runs under no_grad in eval mode: BatchNorm uses its running statistics, BayesConv3d applies its eval-mode mask and
    still samples.  dropout=True puts every Dropout3d back in train mode for the call.  Every module's mode is restored on exit.
    samples_per_pass=k runs the draws k at a time on inputs.repeat(k, 1, 1, 1, 1): the caller's statement that batch elements are
    independent in this mode (instance-normalised and eval-mode batch-normalised models).  The random stream is torch's device
    generator, so two calls after the same torch.manual_seed give the same bits."""
    ops._require_device(inputs)
    if n_samples < 1 or samples_per_pass < 1:
        raise RuntimeError("mc_predict: n_samples and samples_per_pass must be at least 1")
    acc = None
    with torch.no_grad(), _sampling_mode(model, dropout):
        done = 0
        while done < n_samples:
            k = min(samples_per_pass, n_samples - done)
            logits = model(inputs if k == 1 else inputs.repeat(k, 1, 1, 1, 1))
            if acc is None:
                acc = MCAccumulator((inputs.shape[0],) + tuple(logits.shape[1:]), logits.device)
            acc.add(logits, reps=k)
            done += k
    return acc.result(want)
