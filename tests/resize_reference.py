"""What the resize tests share: the shapes and images of the acceptance list, Pillow's answer, and a numpy restatement of the
two integer passes of Pillow's 8-bit resample (the arithmetic itermvs_resize_rgb8 performs on the package's tables)."""
import numpy as np

# (Hs, Ws) -> (H, W): both axes shrinking, DTU's 1200 -> 1152 ratio, both growing (square result), one axis only (each
# skipped pass), both growing, an 11-tap footprint, vertical only
SHAPES = [((36, 40), (32, 32)), ((75, 100), (64, 96)), ((48, 64), (64, 64)), ((32, 50), (32, 32)), ((37, 32), (32, 32)),
          ((20, 24), (32, 64)), ((150, 200), (32, 64)), ((50, 64), (48, 64))]
IMAGES = ["random", "white", "black"]


def make_image(kind: str, hs: int, ws: int, seed: int = 0) -> np.ndarray:
    if kind == "white":
        return np.full((hs, ws, 3), 255, np.uint8)
    if kind == "black":
        return np.zeros((hs, ws, 3), np.uint8)
    return np.random.default_rng(1000 * hs + ws + seed).integers(0, 256, (hs, ws, 3), dtype=np.uint8)


def pillow_resize(raw: np.ndarray, h: int, w: int) -> np.ndarray:
    from PIL import Image
    return np.array(Image.fromarray(raw).resize((w, h), Image.BILINEAR))


def _pass(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray, axis: int) -> np.ndarray:
    """one integer pass along ``axis`` (0 = vertical, 1 = horizontal) of img [H,W,3] uint8"""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.uint8)
    for i, (first, count) in enumerate(bounds):
        acc = (1 << 21) + np.tensordot(kk[i, :count].astype(np.int64), src[first:first + count], axes=(0, 0))
        out[i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def integer_resize(raw: np.ndarray, h: int, w: int, tables) -> np.ndarray:
    """horizontal pass, uint8 intermediate, vertical pass; a pass is skipped when its axis keeps its size"""
    xb, xk, yb, yk = tables
    img = raw
    if raw.shape[1] != w:
        img = _pass(img, xb, xk, 1)
    if raw.shape[0] != h:
        img = _pass(img, yb, yk, 0)
    return np.ascontiguousarray(img)
