"""Affine registration to a template on the device: host parametrisation and search in `affine`, the pyramid and
the device-driven coarse-to-fine loop in `register`."""
from .affine import compose, corner_displacement, invert, level_matrix, optimise, params_to_matrix, step_vector  # noqa: F401
from .register import Pyramid, Registration, apply, register  # noqa: F401
