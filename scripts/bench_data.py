"""Device-side input preparation for one training batch (B x V renderings + B volumes) next to the CPU restatement of the
reference's per-sample numpy path.  python scripts/bench_data.py [--batch 32]"""
import argparse
import ctypes
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
from swinvox_amd.hip import call, ptr  # noqa: E402

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
# the same renderings over photographs (RandomBackground with a folder): a bank of 64, every second view takes its sample's photograph
bank = D.background_bank(np.random.default_rng(1).integers(0, 256, size=(64, 224, 224, 3), dtype=np.uint8), cfg, device=dev)
bparams = [D.AugParams(**{**vars(p), "bg_index": b % 64, "bg_photo": [v % 2 == 0 for v in range(a.views)]}) for b, p in enumerate(params)]
t_aug_bg = timed(lambda: D.augment_views(x, bparams, cfg, backgrounds=bank))
# ... and the launch pairs alone, by device events, on buffers prepared once
aug_arr, aug_flips = D._pack_aug_samples(params, a.views, cfg, "bench_data")
aug_prm = torch.frombuffer(bytearray(bytes(aug_arr)), dtype=torch.uint8).to(dev)
aug_fl = torch.from_numpy(aug_flips).to(dev)
aug_ws = torch.empty(a.batch * a.views, dtype=torch.float64, device=dev)
aug_out = torch.empty(a.batch, a.views, 3, 224, 224, dtype=torch.float32, device=dev)
aug_tab = D._bg_index_table(bparams, a.views, cfg, bank)
aug_tab_dev = torch.empty(a.batch * a.views, dtype=torch.int32, device=dev)
aug_head = (ptr(x), a.batch * a.views, a.views, 137, 137, 4, cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W, 224, 224, ptr(aug_prm), ptr(aug_fl))


def timed_events(fn, n=50):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


t_aug_kernel = timed_events(lambda: call("sv_augment_views", *aug_head, ptr(aug_ws), ptr(aug_out)))
t_aug_bg_kernel = timed_events(lambda: call("sv_augment_views_bg", *aug_head, ptr(bank), 64, aug_tab.ctypes.data, ptr(aug_tab_dev), ptr(aug_ws),
                                            ptr(aug_out)))
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
# exposed voxel faces of the same 32 volumes as PLY files next to a plain per-voxel face loop on the host (what a mesh cost before:
# a device-to-host copy of the volumes and this loop)
SURF_DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
SURF_CORNERS = (((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)), ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),
                ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)), ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)))


def host_face_loop(vol):
    pad = np.pad(vol, 1)
    quads = []
    for x, y, z in np.argwhere(vol):
        for (dx, dy, dz), corners in zip(SURF_DIRS, SURF_CORNERS):
            if not pad[x + 1 + dx, y + 1 + dy, z + 1 + dz]:
                quads.append([((x + a) * 33 + y + b) * 33 + z + c for a, b, c in corners])
    lat = np.asarray(quads, np.int64).reshape(-1, 4)
    used = np.unique(lat)
    verts = np.stack([used // 1089, used // 33 % 33, used % 33], axis=1)
    return D.mesh_file(verts, np.searchsorted(used, lat), "ply")


t_mesh = timed(lambda: D.encode_mesh_batch(vol_dev), n=50)
t_surf = timed(lambda: D.extract_surface_batch(vol_dev), n=50)
sv, sf, sc = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((a.batch, 33 ** 3), (a.batch, 3 * 32 ** 3 + 3 * 32 ** 2, 4), (a.batch, 2)))
vol_u8 = vol_dev.view(torch.uint8)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
surf_launch = lambda: call("sv_voxel_surface", ptr(vol_u8), 1, a.batch, 32, 32, 32, -1.0, ptr(sv), sv.shape[1], ptr(sf), sf.shape[1], ptr(sc))  # noqa: E731
surf_launch(); torch.cuda.synchronize()
ev0.record()
for _ in range(50):
    surf_launch()
ev1.record(); torch.cuda.synchronize()
t_surf_kernel = ev0.elapsed_time(ev1) / 50
t0 = time.perf_counter()
host_meshes = [host_face_loop(v) for v in vols]
t_mesh_cpu = (time.perf_counter() - t0) * 1e3
assert host_meshes == D.encode_mesh_batch(vol_dev)
# the picture of each of the same 32 volumes at the reference's 640 x 480 from its camera (sv_render_volumes) next to the numpy
# restatement of the same rule on the host (tests/volume_view_ref.py: ray-cast + shading); matplotlib, which the reference calls, takes
# seconds per volume
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import volume_view_ref as VR  # noqa: E402

t_view = timed(lambda: D.render_views_batch(vol_dev), n=50)
view_cam = D.view_camera((32, 32, 32))
cam_arr = (S.hip.ViewCamera * 1).from_buffer_copy(view_cam.astype(np.float32).tobytes())
colours = [(ctypes.c_ubyte * len(v))(*v) for v in ([c for rgb in D.VIEW_FACE_RGB for c in rgb], (0, 0, 0), (255, 255, 255))]
cam_ws = torch.empty(72, dtype=torch.uint8, device=dev)
mask_ws = torch.empty(a.batch * 1024, dtype=torch.int32, device=dev)
view_ids = torch.empty(a.batch, 1, 480, 640, dtype=torch.int32, device=dev)
view_rgb = torch.empty(a.batch, 1, 3, 480, 640, dtype=torch.uint8, device=dev)
view_launch = lambda: call("sv_render_volumes", ptr(vol_u8), 1, a.batch, 32, 32, 32, -1.0, ctypes.addressof(cam_arr), 1, ptr(cam_ws), 480, 640,  # noqa: E731
                           *(ctypes.addressof(c) for c in colours), None, ptr(mask_ws), ptr(view_ids), ptr(view_rgb))
view_launch(); torch.cuda.synchronize()
ev0.record()
for _ in range(50):
    view_launch()
ev1.record(); torch.cuda.synchronize()
t_view_kernel = ev0.elapsed_time(ev1) / 50
t0 = time.perf_counter()
host_views = np.stack([VR.shade(VR.render_ids(v, view_cam, (480, 640)), D.VIEW_FACE_RGB) for v in vols])
t_view_cpu = (time.perf_counter() - t0) * 1e3
view_diff = int((host_views != D.render_views_batch(vol_dev)[:, 0].cpu().numpy()).any(axis=1).sum())
# mesh voxelisation (sv_voxelise_meshes): the voxel surfaces of the same volumes as triangle meshes, the last one replaced by the surface of a
# half-filled volume (about 100 k triangles), back to 32^3 in mode "both"; next to the numpy restatement of the rule (tests/mesh_voxel_ref.py,
# clipped to bounding boxes) on the host, timed on the first VOX_SAMPLE triangles of a small and of the large mesh and scaled by the counts
import mesh_voxel_ref as MR  # noqa: E402

VOX_SAMPLE = 2000
vox_meshes = D.extract_surface_batch(vol_dev)
vox_meshes[-1] = D.extract_surface_batch(torch.from_numpy(np.random.default_rng(2).random((1, 32, 32, 32)) < 0.5).to(dev))[0]
t_voxelise = timed(lambda: D.voxelise_mesh_batch(vox_meshes, 32, fit=None, device=dev), n=10)
vox_packed, vox_table, vox_nv, vox_nt, _, _ = D.pack_meshes(vox_meshes, 32, fit=None)
vox_buf = torch.from_numpy(vox_packed).to(dev)
vox_out = torch.empty(a.batch, 32, 32, 32, dtype=torch.float32, device=dev)
vox_ws = torch.empty(S.hip.load().sv_voxelise_meshes_workspace_bytes(a.batch, 32, 32, 32), dtype=torch.uint8, device=dev)
vox_launch = lambda: call("sv_voxelise_meshes", ptr(vox_buf), vox_nv, ptr(vox_buf) + 12 * vox_nv, vox_nt, vox_table.ctypes.data, a.batch,  # noqa: E731
                          32, 32, 32, 2, 0, ptr(vox_out), ptr(vox_ws))
t_voxelise_kernel = [timed_events(vox_launch, n=20) for _ in range(2)]
t_voxelise_cpu, vox_diff = [], 0
for run in range(2):
    t_run = 0.0
    for b in (0, a.batch - 1):
        v, nv_b, t0_b, nt_b = (int(x) for x in vox_table[b])
        verts_b = vox_packed[3 * v:3 * (v + nv_b)].reshape(-1, 3)
        tris_b = vox_packed[3 * vox_nv + 3 * t0_b:3 * vox_nv + 3 * (t0_b + nt_b)].reshape(-1, 3)[:VOX_SAMPLE]
        t0 = time.perf_counter()
        want = MR.voxelise(verts_b, tris_b, (32, 32, 32), "both", clip=True)
        per_tri = (time.perf_counter() - t0) / len(tris_b)
        t_run += per_tri * (vox_nt - int(vox_table[-1, 3]) if b == 0 else int(vox_table[-1, 3])) * 1e3
        if run == 0:
            got = D.voxelise_mesh_batch([(verts_b / 1024.0, tris_b)], 32, fit=None, device=dev)[0][0].cpu().numpy() != 0
            vox_diff += int((got != want).sum())
    t_voxelise_cpu.append(t_run)
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
print(f"augment_views   {t_aug_bg:7.3f} ms / batch of {n} views over a bank of 64 photographs 224x224x3, every second view taking one "
      f"({n / t_aug_bg * 1e3:9.0f} views/s, host parameter and table packing included; {t_aug_bg / t_aug:.2f} x the line above); the launch pairs alone "
      f"by device events: {t_aug_bg_kernel:6.3f} ms with the bank, {t_aug_kernel:6.3f} ms without ({t_aug_bg_kernel / t_aug_kernel:.2f} x)")
print(f"binvox decode   {t_vox:7.3f} ms / {a.batch} volumes (header parsing + H2D of the run-length bytes included)")
print(f"binvox encode   {t_enc:7.3f} ms / {a.batch} volumes (pair counts + trimmed payload D2H and header formatting included); "
      f"oracle.data.write_binvox on the host, one core: {t_wr:7.2f} ms")
print(f"voxel surface   {t_mesh:7.3f} ms / {a.batch} volumes as PLY files (counts + trimmed payload D2H, lattice decode and PLY formatting included; "
      f"{t_surf:7.3f} ms without the formatting, {t_surf_kernel:6.3f} ms the kernel alone by device events; {sum(len(m) for m in host_meshes) / 1e6:.2f} MB of files); per-voxel numpy face loop + the same formatting on "
      f"the host, one core: {t_mesh_cpu:7.1f} ms")
print(f"volume views    {t_view:7.3f} ms / {a.batch} volumes as {a.batch} pictures of 640x480 on the device (allocation of the outputs and the camera copy "
      f"included; {t_view_kernel:6.3f} ms the three launches alone by device events); numpy restatement of the same ray-cast and shading on the host, "
      f"one core: {t_view_cpu:7.1f} ms; pixels that differ between the two: {view_diff}")
print(f"mesh voxelise    {t_voxelise:7.3f} ms / {a.batch} meshes of {vox_nt} triangles in all (the largest {int(vox_table[-1, 3])}) -> 32^3, mode both (fan "
      f"triangulation, snapping, packing, the H2D copy of {vox_packed.nbytes / 1e6:.1f} MB and the counter read-back included); the launches alone by "
      f"device events, two runs: {t_voxelise_kernel[0]:6.3f} / {t_voxelise_kernel[1]:6.3f} ms; numpy restatement of the same rule on the host, one core, "
      f"scaled from {VOX_SAMPLE} triangles of a small and of the large mesh, two runs: {t_voxelise_cpu[0]:8.0f} / {t_voxelise_cpu[1]:8.0f} ms; voxels that "
      f"differ between the two on those triangles: {vox_diff}")
print(f"numpy restatement of the reference path, one core: {t_cpu:8.1f} ms / batch ({n / t_cpu * 1e3:7.0f} views/s)")
