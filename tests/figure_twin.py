"""A NumPy restatement of the byte conversion of `FigureRenderer.render_rgba8` (csrc/figure.hip, image_rgba8): the same
IEEE operations in the same order, so the device's bytes are compared exactly."""
import numpy as np


def rgba8_twin(img, background=(1.0, 1.0, 1.0)) -> np.ndarray:
    """`(..., 4)` uint8 from `(..., 4)` float64 premultiplied colour and alpha over `background`: per colour channel
    `c = C + (1 - alpha) * b`, `q = floor(255 * min(1, max(0, c)) + 0.5)`, 0 for a `c` that is not finite; the fourth
    byte is the same rule applied to alpha."""
    img = np.asarray(img, dtype=np.float64)
    b = np.asarray(background, dtype=np.float64)
    a = img[..., 3]
    with np.errstate(invalid="ignore", over="ignore"):
        c = img[..., :3] + (1.0 - a)[..., None] * b
        full = np.concatenate([c, a[..., None]], axis=-1)
        fin = np.isfinite(full)
        s = np.minimum(1.0, np.maximum(0.0, np.where(fin, full, 0.0)))
        q = np.floor(255.0 * s + 0.5)
    return np.where(fin, q, 0.0).astype(np.uint8)
