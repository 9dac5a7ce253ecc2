"""NumPy restatement of the overview pyramid (csrc/pyramid.hip, codec.build_overviews): the two halvings and the chain.
No tests here; test_pyramid_cpu.py holds the restatement to float64, test_gpu_pyramid.py holds the kernels to it.

A level is ceil(H/2) x ceil(W/2).  Output pixel (y, x) is taken from source rows 2y and min(2y+1, H-1) and columns 2x
and min(2x+1, W-1); with a = top-left, b = top-right, c = bottom-left, d = bottom-right
  uint8  [H,W,C]:  (a + b + c + d + 2) >> 2 in integers, per channel
  float32 [C,H,W]: ((a + b) + (c + d)) * 0.25f, every step rounded to float32."""
import numpy as np


def halved(n):
    return (n + 1) // 2


def shapes(H, W, n):
    """[(H, W), ...]: the sizes of the image and of its n levels"""
    out = [(H, W)]
    for _ in range(n):
        out.append((halved(out[-1][0]), halved(out[-1][1])))
    return out


def _taps(L):
    """source indices (first, second) of every output position of an axis of L"""
    first = 2 * np.arange(halved(L))
    return first, np.minimum(first + 1, L - 1)


def halve_u8(img):
    """uint8 [H,W,C] -> uint8 [ceil(H/2), ceil(W/2), C]"""
    assert img.dtype == np.uint8 and img.ndim == 3
    y0, y1 = _taps(img.shape[0])
    x0, x1 = _taps(img.shape[1])
    v = img.astype(np.int32)
    s = v[y0][:, x0] + v[y0][:, x1] + v[y1][:, x0] + v[y1][:, x1] + 2
    return (s >> 2).astype(np.uint8)


def halve_f32(img):
    """float32 [C,H,W] -> float32 [C, ceil(H/2), ceil(W/2)]"""
    assert img.dtype == np.float32 and img.ndim == 3
    y0, y1 = _taps(img.shape[1])
    x0, x1 = _taps(img.shape[2])
    with np.errstate(invalid="ignore", over="ignore"):
        top = img[:, y0][:, :, x0] + img[:, y0][:, :, x1]
        bottom = img[:, y1][:, :, x0] + img[:, y1][:, :, x1]
        out = (top + bottom) * np.float32(0.25)
    assert out.dtype == np.float32
    return out


def halve(img):
    return halve_u8(img) if img.dtype == np.uint8 else halve_f32(img)


def chain(img, n):
    """[img, level 1, ..., level n], each level from the one before it"""
    out = [img]
    for _ in range(n):
        out.append(halve(out[-1]))
    return out
