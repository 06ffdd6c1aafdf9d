"""Device-side input preparation for one training batch (B x V renderings + B volumes) next to the CPU restatement of the
reference's per-sample numpy path.  python scripts/bench_data.py [--batch 32]"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swinvox_amd as S  # noqa: E402
from oracle import data as OD  # noqa: E402
from swinvox_amd import data as D  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--views", type=int, default=8)
a = ap.parse_args()
dev = torch.device("cuda:0")
cfg = S.default_cfg()
rng = np.random.default_rng(0)
imgs = rng.integers(0, 256, size=(a.batch, a.views, 137, 137, 4), dtype=np.uint8)
imgs[..., 3] = np.where(rng.random((a.batch, a.views, 137, 137)) < 0.5, 0, 255)
vols = [rng.random((32, 32, 32)) < 0.05 for _ in range(a.batch)]
files = [OD.write_binvox(v) for v in vols]
params = [D.draw_train_params(a.views, cfg) for _ in range(a.batch)]
x = torch.from_numpy(imgs).to(dev)


def timed(fn, n=20):
    fn(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


t_aug = timed(lambda: D.augment_views(x, params, cfg))
t_vox = timed(lambda: D.decode_binvox_batch(files, dev, check=False))
t0 = time.perf_counter()
for b in range(min(a.batch, 4)):
    p = params[b]
    OD.transform_views(imgs[b], dict(bg=np.asarray(p.bg), jitter_value=p.jitter_value, jitter_order=list(p.jitter_order),
                                     noise_alpha=np.asarray(p.noise_alpha), flips=list(p.flips), perm=list(p.perm)))
    OD.read_binvox(files[b])
t_cpu = (time.perf_counter() - t0) / min(a.batch, 4) * a.batch * 1e3
vol_dev = torch.from_numpy(np.stack(vols)).to(dev)
t_enc = timed(lambda: D.encode_binvox_batch(vol_dev))
t0 = time.perf_counter()
for b in range(a.batch):
    OD.write_binvox(vols[b])
t_wr = (time.perf_counter() - t0) * 1e3
# photographs with bounding boxes (the Pascal3D / Pix3D branch): 32 images of 640 x 480 x 3, each cropped to its jittered box
photos = [rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8) for _ in range(32)]
boxes = [(0.1 + 0.2 * rng.random(), 0.1 + 0.2 * rng.random(), 0.7 + 0.35 * rng.random(), 0.7 + 0.35 * rng.random()) for _ in photos]
pparams = [D.draw_train_params(1, cfg, n_channels=3, bounding_box=b) for b in boxes]
t_box = timed(lambda: D.augment_images(photos, boxes, pparams, cfg, device=dev))
t0 = time.perf_counter()
for im, box, p in list(zip(photos, boxes, pparams))[:4]:
    xl, xr, yt, yb, pl, pr, pt, pb = D.bbox_crop_rect(480, 640, box, p.crop_draws)
    crop = np.pad(im[yt:yb + 1, xl:xr + 1], ((pt, pb), (pl, pr), (0, 0)), mode="edge")
    OD.transform_views(crop[None], dict(bg=np.asarray(p.bg), jitter_value=p.jitter_value, jitter_order=list(p.jitter_order),
                                        noise_alpha=np.asarray(p.noise_alpha), flips=list(p.flips), perm=list(p.perm)),
                       crop_size=(max(crop.shape[0], 224) + 1, max(crop.shape[1], 224) + 1))
t_box_cpu = (time.perf_counter() - t0) / 4 * len(photos) * 1e3
n = a.batch * a.views
print(f"augment_images  {t_box:7.3f} ms / batch of {len(photos)} photographs 640x480x3 with boxes ({len(photos) / t_box * 1e3:9.0f} images/s, host packing and "
      f"the H2D copy of {sum(im.size for im in photos) / 1e6:.1f} MB included); numpy restatement of the same path, one core: {t_box_cpu:7.1f} ms")
print(f"augment_views   {t_aug:7.3f} ms / batch of {n} views ({n / t_aug * 1e3:9.0f} views/s, host parameter packing included)")
print(f"binvox decode   {t_vox:7.3f} ms / {a.batch} volumes (header parsing + H2D of the run-length bytes included)")
print(f"binvox encode   {t_enc:7.3f} ms / {a.batch} volumes (pair counts + trimmed payload D2H and header formatting included); "
      f"oracle.data.write_binvox on the host, one core: {t_wr:7.2f} ms")
print(f"numpy restatement of the reference path, one core: {t_cpu:8.1f} ms / batch ({n / t_cpu * 1e3:7.0f} views/s)")
