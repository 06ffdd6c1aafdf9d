"""CPU restatement of the training transform list with RandomBackground's folder (utils/data_transforms.py:415-452): the list of
oracle.data.transform_views with one change - a view whose coin says so takes the sample's photograph, not the flat colour, wherever
its resized alpha is exactly zero.  TEST INFRASTRUCTURE ONLY.

The reference blends alpha * bg_color + (1 - alpha) * img with alpha = (resized alpha == 0) as 0.0 / 1.0, so the blend is a select;
bg_color is either the photograph as cv2.imread(...).astype(np.float32) / 255. or the colour as float64, and the image is float64 from
there on.  The photograph has the size of the resized rendering (anything else cannot broadcast) and is flipped with the finished
image.  PINNED: tests/golden/bg_photo_cases.npz holds outputs of the reference's own Compose (tests/golden/make_bg_photo_golden.py);
tests/test_cpu_bg_photo.py asserts that this function reproduces them element for element."""
import numpy as np

from oracle import data as OD


def oracle_prm(p):
    """the dict oracle.data.transform_views takes, from a swinvox_amd.data.AugParams"""
    return dict(bg=np.asarray(p.bg), jitter_value=list(p.jitter_value), jitter_order=list(p.jitter_order), noise_alpha=np.asarray(p.noise_alpha),
                flips=list(p.flips), perm=list(p.perm))


def transform_views_bg(images_u8, prm, photo=None, take=(), img_size=(224, 224), crop_size=(128, 128), mean=(0.5, 0.5, 0.5),
                       std=(0.5, 0.5, 0.5)):
    """images_u8 [V, Hs, Ws, C] -> float32 [V, 3, H, W].  prm: the dict of oracle.data.transform_views.  photo: uint8 [H, W, 3] or
    None; take: one flag per view (empty = no view takes the photograph)."""
    out = []
    names = ["brightness", "contrast", "saturation"]
    take = list(take) if len(take) else [False] * len(images_u8)
    if photo is not None:
        photo = np.asarray(photo)
        if photo.dtype != np.uint8 or photo.shape != (img_size[0], img_size[1], 3):
            raise ValueError("a photograph has the size of the resized rendering")          # the reference: operands could not be broadcast
        photo = photo.astype(np.float32) / np.float32(255.)
    for v, u8 in enumerate(images_u8):
        img = u8.astype(np.float32) / 255.0
        H, W, C = img.shape
        if H > crop_size[0] and W > crop_size[1]:
            x0, y0 = int(W - crop_size[1]) // 2, int(H - crop_size[0]) // 2
            img = img[y0:y0 + crop_size[0], x0:x0 + crop_size[1]]
        img = OD.resize_linear(img, img_size[0], img_size[1]).astype(np.float64)
        if C == 4:
            behind = photo.astype(np.float64) if (take[v] and photo is not None) else np.asarray(prm["bg"], np.float64).reshape(1, 1, 3)
            img = np.where(img[:, :, 3:4] == 0, behind, img[:, :, :3])                       # the select
        for idx in prm["jitter_order"]:
            a = prm["jitter_value"][idx]
            gs = OD._grey(img)
            if names[idx] == "contrast":
                img = a * img + (1 - a) * np.mean(gs[:, :, 0])
            elif names[idx] == "saturation":
                img = a * img + (1 - a) * gs
            else:
                img = a * img + (1 - a) * 0
        nz = OD.noise_rgb_of(np.asarray(prm["noise_alpha"], dtype=np.float64))
        img = img.copy()
        rev = img[:, :, ::-1]
        for i in range(3):
            rev[:, :, i] += nz[i]
        img = (img - np.asarray(mean)) / np.asarray(std)
        if prm["flips"][v]:
            img = np.fliplr(img)
        img = img[..., prm["perm"]]
        out.append(np.transpose(img, (2, 0, 1)))
    return np.stack(out).astype(np.float32)


def sample_reference(images_u8, p, bank=None, **kw):
    """transform_views_bg for one sample from its AugParams and the bank (uint8 [N, H, W, 3] or None)"""
    photo = None if (bank is None or p.bg_index is None) else np.asarray(bank)[int(p.bg_index)]
    return transform_views_bg(images_u8, oracle_prm(p), photo, list(p.bg_photo), **kw)
