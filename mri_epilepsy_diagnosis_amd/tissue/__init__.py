"""Bias-field correction and tissue classes on the device: a Gaussian mixture on log-intensity with a smooth
polynomial field, the model behind the bias-corrected `_restore` image the reference takes from FSL FAST."""
from .segment import TissueSegmentation, bias_correct, segment  # noqa: F401
