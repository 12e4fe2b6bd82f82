"""float64 numpy restatement of the motion artefact and the intensity rescaling of segmentation/transforms.py (RandomMotion,
RescaleIntensity), written from their definitions (include/mri3d.h, "Augmentation"; TorchIO itself is absent, "parity unpinned").

`fft_composite` is the library formulation: Fourier-transform every volume, fill slabs of the shifted spectrum along the last
axis, transform back, keep the real part.  `mix` is the double sum the device kernel computes.  The two agree to float64
rounding when the filters come from `transforms.motion_coefficients` (tests/test_motion.py)."""
import numpy as np


def fft_composite(images, times):
    """images: (n, D, H, W), image 0 the unmoved volume, image k the volume moved by transform k; times: n - 1 ascending
    numbers.  Returns the (D, H, W) float64 composite."""
    images = np.asarray(images, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64).reshape(-1)
    n, w = images.shape[0], images.shape[-1]
    assert len(times) == n - 1
    spectra = [np.fft.fftshift(np.fft.fftn(im)) for im in images]
    above = np.nonzero(times > 0.5)[0]
    idx = int(above.min()) if len(above) else n - 1
    spectra[0], spectra[idx] = spectra[idx], spectra[0]
    result = np.empty_like(spectra[0])
    ini = 0
    for j, t in enumerate(list(times) + [1.0]):
        fin = w if j == n - 1 else int(np.floor(w * t))
        result[..., ini:fin] = spectra[j][..., ini:fin]
        ini = fin
    return np.fft.ifftn(np.fft.ifftshift(result)).real


def mix(images, coef):
    """out[d,h,z] = sum_m sum_z' coef[m, (z - z') mod W] images[m,d,h,z'] in float64.  images (n, D, H, W), coef (n, W)."""
    images, coef = np.asarray(images, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    n, w = coef.shape
    z = np.arange(w)
    out = np.zeros(images.shape[1:], dtype=np.float64)
    for m in range(n):
        circulant = coef[m][(z[:, None] - z[None, :]) % w]          # [z, z']
        out += images[m] @ circulant.T
    return out


def rescale(x, out_min_max, percentiles=(0, 100)):
    """Clip x to its two percentiles (np.percentile, linear) and map them linearly onto out_min_max; no range -> out_min."""
    x = np.asarray(x, dtype=np.float64)
    low, high = np.percentile(x, percentiles)
    out_min, out_max = (float(v) for v in out_min_max)
    if not high > low:
        return np.full_like(x, out_min)
    return (np.clip(x, low, high) - low) / (high - low) * (out_max - out_min) + out_min
