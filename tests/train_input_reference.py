"""Restatements of the reference's training input side (datasets/dtu_yao.py, datasets/blendedmvs.py) for the tests of
itermvs_amd/train_dataset.py (the small dataset trees they read come from itermvs_amd/dataset_trees.py).

cv2 is not installed: ``nn_resize`` restates cv2.resize(INTER_NEAREST) from OpenCV's published resizeNN
(x_ofs = min(cvFloor(x * (1.0 / inv_scale_x)), src_w - 1), inv_scale_x = dst_w / src_w), so the ground-truth maps it gives
are unpinned against the library itself, like oracle/image_oracle.py's bilinear resize.  The jitter reference is the
installed Pillow (PIL.ImageEnhance), which is what torchvision calls for PIL images."""
import numpy as np

from itermvs_amd.dataset_trees import write_blended_tree, write_dtu_tree  # noqa: F401  (the tests' trees)


def nn_resize(a: np.ndarray, dst_w: int, dst_h: int) -> np.ndarray:
    """cv2.resize(a, (dst_w, dst_h), interpolation=cv2.INTER_NEAREST) for a 2-D array"""
    src_h, src_w = a.shape[:2]
    xs = np.minimum(np.floor(np.arange(dst_w, dtype=np.float64) * (1.0 / (dst_w / src_w))).astype(np.int64), src_w - 1)
    ys = np.minimum(np.floor(np.arange(dst_h, dtype=np.float64) * (1.0 / (dst_h / src_h))).astype(np.int64), src_h - 1)
    return a[ys][:, xs]


def dtu_depth_mask(depth_file: np.ndarray, visual: np.ndarray, scale, img_wh=(640, 512)):
    """dtu_yao.py:80-119 on the flipped (top-down) depth [H,W] and the depth_visual bytes -> ({level: depth}, {level: mask})"""
    def prepare_img(hr_img):                                          # dtu_yao.py:80-91
        h, w = hr_img.shape
        hr_img = nn_resize(hr_img, w // 2, h // 2)
        h, w = hr_img.shape
        target_h, target_w = img_wh[1], img_wh[0]
        start_h, start_w = (h - target_h) // 2, (w - target_w) // 2
        return hr_img[start_h: start_h + target_h, start_w: start_w + target_w]
    depth_hr = np.array(depth_file, dtype=np.float32) * scale
    depth_lr = prepare_img(depth_hr)
    mask = (np.array(visual, dtype=np.float32) > 10).astype(np.float32)
    mask = prepare_img(mask).astype(np.bool_).astype(np.float32)
    h, w = depth_lr.shape
    d, m = {}, {}
    for i in range(4):
        d[f"level_{i}"] = nn_resize(depth_lr, w // (2 ** i), h // (2 ** i))
        m[f"level_{i}"] = nn_resize(mask, w // (2 ** i), h // (2 ** i))
    return d, m


def blended_depth_mask(depth_file: np.ndarray, sf: float, scale, depth_min: float, depth_max: float, img_wh=(768, 576)):
    """blendedmvs.py:62-83 on the flipped (top-down) depth [H,W] -> ({level: depth}, {level: mask})"""
    depth = np.array(depth_file, dtype=np.float32)
    depth = depth * sf * scale
    mask = (depth >= depth_min) & (depth <= depth_max)
    mask = mask.astype(np.float32)
    depth = nn_resize(depth, img_wh[0], img_wh[1])
    h, w = depth.shape
    d, m = {}, {}
    for i in range(4):
        d[f"level_{i}"] = nn_resize(depth, w // (2 ** i), h // (2 ** i))
        m[f"level_{i}"] = nn_resize(mask, w // (2 ** i), h // (2 ** i))
    return d, m


def read_cam(filename):
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.fromstring(' '.join(lines[1:5]), dtype=np.float32, sep=' ').reshape((4, 4))
    intrinsics = np.fromstring(' '.join(lines[7:10]), dtype=np.float32, sep=' ').reshape((3, 3))
    return intrinsics, extrinsics, float(lines[11].split()[0]), float(lines[11].split()[-1])


def dtu_proj(cam_file: str, scale):
    """dtu_yao.py:165-188 -> {level: [4,4]}"""
    intrinsics, extrinsics, _, _ = read_cam(cam_file)
    extrinsics[:3, 3] *= scale
    intrinsics[0] *= 4
    intrinsics[1] *= 4
    return _levels(intrinsics, extrinsics)


def blended_proj(cam_file: str, sf: float, scale):
    """blendedmvs.py:45-60 + 146-166 -> {level: [4,4]}"""
    intrinsics, extrinsics, _, _ = read_cam(cam_file)
    extrinsics[:3, 3] *= sf
    extrinsics[:3, 3] *= scale
    return _levels(intrinsics, extrinsics)


def _levels(intrinsics, extrinsics):
    out = {}
    proj_mat = extrinsics.copy()
    intrinsics[:2, :] *= 0.125
    proj_mat[:3, :4] = np.matmul(intrinsics, proj_mat[:3, :4])
    out["level_3"] = proj_mat
    for lvl in (2, 1, 0):
        proj_mat = extrinsics.copy()
        intrinsics[:2, :] *= 2
        proj_mat[:3, :4] = np.matmul(intrinsics, proj_mat[:3, :4])
        out[f"level_{lvl}"] = proj_mat
    return out


def pil_jitter(raw: np.ndarray, draw) -> np.ndarray:
    """torchvision ColorJitter.forward on a PIL image for one draw (brightness, contrast, contrast_first): the bytes
    PIL.ImageEnhance produces"""
    from PIL import Image, ImageEnhance
    if draw is None:
        return raw
    b, c, contrast_first = draw
    img = Image.fromarray(raw)
    for fn in ((1, 0) if contrast_first else (0, 1)):
        img = ImageEnhance.Brightness(img).enhance(b) if fn == 0 else ImageEnhance.Contrast(img).enhance(c)
    return np.asarray(img)
