"""Measurement of the SURVEY 8f rows on one MI355X (HIP-event medians; inputs resident on the device), each next to a
bounded host-side restatement of what the reference does for the same call (numpy / torch CPU on this box's cores).

  python tools/bench_rows.py > profiles/<round>_rows.json      (one JSON object per line)
  python tools/bench_rows.py augment                            (the 3-D augmentation row alone)
  python tools/bench_rows.py augment2d                          (the 2-D training chain row alone)
  python tools/bench_rows.py transforms2d                       (the full 2-D transform list row alone)
  python tools/bench_rows.py resize3d                           (the CropResize row alone)
  python tools/bench_rows.py components                         (the connected-component rows alone)
  python tools/bench_rows.py morphology                         (the binary morphology rows alone)
  python tools/bench_rows.py lesions                            (the lesion-wise matching rows alone)
  python tools/bench_rows.py detect                             (the lesion-candidate rows alone)
  python tools/bench_rows.py slice2d                            (the slice-wise 2-D inference row alone)
"""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from hdf_rt import inference
from hdf_rt.loss_fn import RunningDice, compute_dice
from hdf_rt.optim import FlatAdam

DEV = torch.device("cuda", 0)


def gpu_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def cpu_s(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def augment_row(C=4, n_cls=4, S=128):
    """hdf_augment_3d on one 4x128^3 sample, all three outputs, next to two streaming yardsticks that move the same bytes
    in the same run: hdf_onehot_from_labels on the sample's voxels plus a device copy of the image"""
    from hdf_rt import augment_3d, trz_matrix
    gen = torch.Generator().manual_seed(11)
    V = S ** 3
    img = torch.randn(C, S, S, S, generator=gen).to(DEV)
    lab_h = torch.randint(0, n_cls, (S, S, S), generator=gen, dtype=torch.uint8)
    lab1 = lab_h.to(DEV)
    aff = trz_matrix("tr", np.random.RandomState(11))
    o_img, o_oh, o_lab = torch.empty_like(img), torch.empty((n_cls, S, S, S), device=DEV), torch.empty_like(lab1)
    us = 1e3 * gpu_ms(lambda: augment_3d(img, lab1, n_cls, aff, True, False, o_img, o_oh, o_lab), reps=30, warm=5)
    us_oh = 1e3 * gpu_ms(lambda: inference.onehot_from_labels(lab1[None], n_cls), reps=30, warm=5)
    us_cp = 1e3 * gpu_ms(lambda: o_img.copy_(img), reps=30, warm=5)
    by = (4 * C + 1 + 4 * C + 4 * n_cls + 1) * V
    try:
        from scipy.ndimage import map_coordinates
        p = np.mgrid[:S, :S, :S].astype(np.float64) - S / 2
        coords = np.einsum("ij,jdhw->idhw", aff[:, :3], p) + aff[:, 3, None, None, None] + S / 2
        img_np, lab_np = img.cpu().numpy(), lab_h.numpy()

        def ref_chain():   # transformer_3d.py:108-117: one warp per channel and one per foreground class
            for ch in img_np:
                map_coordinates(ch, coords, order=1, mode="grid-constant", cval=0, prefilter=False)
            for z in range(1, n_cls):
                map_coordinates((lab_np == z).astype(np.float32), coords, order=1, mode="grid-constant", cval=0, prefilter=False)

        cpu = {"kind": "port", "what": f"scipy.ndimage.map_coordinates order 1, {C + n_cls - 1} warps of {S}^3 (transformer_3d.py:108-117)",
               "s_per_sample": cpu_s(ref_chain, reps=1), "threads": 1}
    except ImportError as exc:
        cpu = {"kind": "not measured", "what": repr(exc)}
    emit(row="augment_3d", config=f"{C}x{S}^3 fp32 + uint8 labels, n_cls {n_cls}, mode 'tr' + H flip, image + labels + one-hot out",
         gpu_us=us, algorithmic_bytes=by, achieved_GBps=by / us / 1e3, hbm_peak_GBps=8000,
         yardstick_us={"onehot_from_labels": us_oh, "image_copy": us_cp}, ratio_to_yardsticks=us / (us_oh + us_cp),
         cpu_baseline=cpu)


def augment2d_row(B=24, C=2, n_cls=2, S=384):
    """one TrainTransform2D call (clone, per-plane MRNormalize, one hdf_augment_2d launch) on the reference's 2-D batch,
    24 x 2 x 384^2 (config.py:69-77), and its gather alone; next to the host chain it replaces, timed on this box:
    MRNormalize + three PIL rotations per sample + flip + To_Tensor (transformer_2d.py, data_loader.py), one thread"""
    from hdf_rt import TrainTransform2D, augment_2d, flip2d_code, rotate_degree, rotate_matrix
    import random
    gen = torch.Generator().manual_seed(12)
    img = (torch.rand(B, C, S, S, generator=gen) * 900).to(DEV)
    lab_h = torch.randint(0, n_cls, (B, S, S), generator=gen, dtype=torch.uint8)
    lab = lab_h.to(DEV)
    random.seed(12), np.random.seed(12)
    tf = TrainTransform2D(n_cls)
    us = 1e3 * gpu_ms(lambda: tf(img, lab), reps=30, warm=5)
    us_val = 1e3 * gpu_ms(lambda: TrainTransform2D(n_cls, degrees=(), flip="")(img, lab), reps=30, warm=5)
    mats = [rotate_matrix(rotate_degree(), S, S) for _ in range(B)]
    codes = [flip2d_code() for _ in range(B)]
    o_img, o_oh = torch.empty_like(img), torch.empty((B, n_cls, S, S), device=DEV)
    us_k = 1e3 * gpu_ms(lambda: augment_2d(img, lab, n_cls, mats, codes, o_img, o_oh), reps=30, warm=5)
    by = (4 * C + 1 + 4 * C + 4 * n_cls) * B * S * S
    try:
        from PIL import Image
        img_np, lab_np = img.cpu().numpy(), lab_h.numpy()

        def ref_chain():
            for b in range(B):
                x = img_np[b].copy()
                for c in range(C):                                   # MRNormalize
                    if x[c].max() != 0:
                        x[c] = x[c] / x[c].max()
                x[x < 0] = 0
                deg = random.choice([-15, -10, -5, 0, 5, 10, 15])    # RandomRotate2D
                x = np.asarray([np.array(Image.fromarray(ch).rotate(deg, Image.BILINEAR)).astype(np.float32) for ch in x])
                y = np.array(Image.fromarray(lab_np[b]).rotate(deg, Image.NEAREST)).astype(np.float32)
                u = np.random.uniform(0, 1)                          # RandomFlip2D
                if u < 0.3:
                    x, y = x[:, :, ::-1], y[:, ::-1]
                elif u < 0.6:
                    x, y = x[:, ::-1, :], y[::-1, :]
                x, y = x.copy(), y.copy()
                oh = np.empty((n_cls,) + y.shape, dtype=np.float32)  # To_Tensor
                for z in range(1, n_cls):
                    oh[z] = (y == z).astype(np.float32)
                oh[0] = np.amax(oh[1:], axis=0) == 0

        import PIL
        cpu = {"kind": "port", "what": f"MRNormalize + {C + 1} PIL {PIL.__version__} rotations per sample + flip + To_Tensor, {B} samples",
               "s_per_batch": cpu_s(ref_chain), "threads": 1}
    except ImportError as exc:
        cpu = {"kind": "not measured", "what": repr(exc)}
    emit(row="TrainTransform2D", config=f"{B}x{C}x{S}^2 fp32 + uint8 labels, n_cls {n_cls}, normalize 'mr', 7 degrees, flip 'hv'",
         gpu_us=us, validation_form_us=us_val, augment_2d_alone_us=us_k, algorithmic_bytes_gather=by,
         achieved_GBps_gather=by / us_k / 1e3, hbm_peak_GBps=8000, cpu_baseline=cpu)


def transforms2d_row(B=24, C=3, n_cls=2, S=384):
    """one TrainTransform2D.from_ids(n_cls, [1,3,4,6,7,8,9,10]) call -- clone, MRNormalize, the label bounding boxes and
    their copy to the host, hdf_zoom_2d, hdf_augment_2d, hdf_intensity_2d -- on 24 x 3 x 384^2, and its new parts alone:
    the bounding-box reduction, the erase + zoom gather with a zoom on every sample, gamma + noise with BOTH on every
    sample (the chain draws noise for one sample in ten).  Same protocol as augment2d_row."""
    from hdf_rt import (TrainTransform2D, erase2d_keep, gamma2d, intensity_2d_, label_bbox_2d, zoom2d_canvas, zoom_2d)
    import random
    gen = torch.Generator().manual_seed(13)
    img = (torch.rand(B, C, S, S, generator=gen) * 900).to(DEV)
    lab_h = torch.zeros((B, S, S), dtype=torch.uint8)
    for b in range(0, B, 2):                                         # every other sample carries a lesion-sized box
        r, c = 40 + 11 * b, 300 - 9 * b
        lab_h[b, r:r + 30, c:c + 24] = 1
    lab = lab_h.to(DEV)
    random.seed(13), np.random.seed(13)
    tf = TrainTransform2D.from_ids(n_cls, [1, 3, 4, 6, 7, 8, 9, 10])
    us = 1e3 * gpu_ms(lambda: tf(img, lab), reps=30, warm=5)
    us_default = 1e3 * gpu_ms(lambda: TrainTransform2D(n_cls)(img, lab), reps=30, warm=5)
    us_bbox = 1e3 * gpu_ms(lambda: label_bbox_2d(lab), reps=30, warm=5)
    bbox = label_bbox_2d(lab).cpu().numpy()
    keeps = [erase2d_keep(bbox[b], S, S) for b in range(B)]
    canvases = [zoom2d_canvas(bbox[b], S, S) for b in range(B)]
    norm = torch.rand(B, C, S, S, generator=gen).to(DEV)
    o_img, o_lab = torch.empty_like(norm), torch.empty_like(lab)
    us_zoom = 1e3 * gpu_ms(lambda: zoom_2d(norm, lab, keeps, canvases, o_img, o_lab), reps=30, warm=5)
    gammas = [gamma2d() for _ in range(B)]
    us_int = 1e3 * gpu_ms(lambda: intensity_2d_(o_img, gammas, [1] * B, 13, 0.0), reps=30, warm=5)
    us_gamma = 1e3 * gpu_ms(lambda: intensity_2d_(o_img, gammas, [0] * B, 13, 0.0), reps=30, warm=5)
    px = B * S * S
    emit(row="TrainTransform2D full list", config=f"{B}x{C}x{S}^2 fp32 + uint8 labels, n_cls {n_cls}, transform_2d [1,3,4,6,7,8,9,10]",
         gpu_us=us, default_chain_us=us_default, label_bbox_2d_us=us_bbox, zoom_2d_alone_us=us_zoom,
         intensity_2d_gamma_and_noise_on_every_sample_us=us_int, intensity_2d_gamma_alone_us=us_gamma,
         algorithmic_bytes_zoom=(8 * C + 2) * px, achieved_GBps_zoom=(8 * C + 2) * px / us_zoom / 1e3,
         algorithmic_bytes_intensity=8 * C * px, achieved_GBps_intensity=8 * C * px / us_int / 1e3, hbm_peak_GBps=8000)


def resize3d_row(C=2, n_cls=3, src=(173, 191, 205), S=144):
    """one crop_resize call (hdf_resize_3d: three gather passes per image channel and per foreground class) on a
    2 x 173x191x205 sample to 144^3, next to the host sequence it replaces, timed on this box on one thread: per plane
    scipy.ndimage.gaussian_filter + zoom(order=1, grid_mode=True) in fp32 arrays, the arithmetic of
    skimage.transform.resize (data_loader.py:103-119); plus the whole [2,3,4,5,6] chain on the same sample"""
    from hdf_rt import TrainTransform3D, crop_resize
    gen = torch.Generator().manual_seed(14)
    img = torch.randn((C,) + src, generator=gen).to(DEV)
    lab_h = torch.randint(0, n_cls, tuple(-(-s // 8) for s in src), generator=gen, dtype=torch.uint8)
    lab_h = lab_h.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:src[0], :src[1], :src[2]]
    lab = lab_h.contiguous().to(DEV)
    dim = (S, S, S)
    us = 1e3 * gpu_ms(lambda: crop_resize(img, lab, n_cls, dim), reps=30, warm=5)
    np.random.seed(14)
    tf = TrainTransform3D.from_ids(n_cls, [2, 3, 4, 5, 6], input_shape=dim)
    us_chain = 1e3 * gpu_ms(lambda: tf(img, lab), reps=30, warm=5)
    vi, vo = src[0] * src[1] * src[2], S ** 3
    by = (4 * C + (n_cls - 1)) * vi + (4 * C + (n_cls - 1)) * vo     # sources read once per plane, results written
    try:
        from scipy import ndimage as ndi
        img_np, lab_np = img.cpu().numpy(), lab_h.numpy()
        sigma = [max(0.0, (i / o - 1) / 2) for i, o in zip(src, dim)]
        zoom = [o / i for i, o in zip(src, dim)]

        def ref_chain():
            for ch in img_np:
                ndi.zoom(ndi.gaussian_filter(ch, sigma, mode="mirror", cval=0), zoom, order=1, mode="mirror", cval=0,
                         grid_mode=True)
            out = np.zeros(dim, dtype=np.float32)
            for z in range(1, n_cls):
                roi = ndi.zoom(ndi.gaussian_filter((lab_np == z).astype(np.float32), sigma, mode="grid-constant", cval=0),
                               zoom, order=1, mode="grid-constant", cval=0, grid_mode=True)
                out[roi >= 0.5] = z

        import scipy
        cpu = {"kind": "port", "what": f"scipy {scipy.__version__} gaussian_filter + zoom(order 1, grid_mode), {C + n_cls - 1} "
                                       f"planes of {src} -> {S}^3 (data_loader.py:103-119)",
               "s_per_sample": cpu_s(ref_chain, reps=3), "threads": 1}
    except ImportError as exc:
        cpu = {"kind": "not measured", "what": repr(exc)}
    emit(row="crop_resize", config=f"{C}x{src[0]}x{src[1]}x{src[2]} fp32 + uint8 labels -> {S}^3, n_cls {n_cls}",
         gpu_us=us, launches=3 * (C + n_cls - 1), chain_2_3_4_5_6_us=us_chain, algorithmic_bytes=by,
         achieved_GBps=by / us / 1e3, hbm_peak_GBps=8000, cpu_baseline=cpu)


def components_row(shapes=((144, 144, 144), (448, 512, 512)), connectivity=26):
    """hdf_cc_label, hdf_cc_filter (keep the largest component of each value) and hdf_cc_table (4096 rows, no score), each
    timed alone on a three-class blob map -- a smoothed 1/8-resolution noise field, thresholded and repeated 8x along each
    axis -- next to scipy.ndimage.label + find_objects per class on the same array, one host thread, copies not counted"""
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    for shape in shapes:
        rng = np.random.default_rng(15)
        try:
            from scipy import ndimage as ndi
            low = ndi.gaussian_filter(rng.random(tuple(s // 8 for s in shape)), 1.5, mode="nearest")
        except ImportError:
            ndi, low = None, rng.random(tuple(s // 8 for s in shape))
        cls = np.digitize(low, np.quantile(low, [0.6, 0.8, 0.93])).astype(np.uint8)
        vol_np = np.ascontiguousarray(cls.repeat(8, 0).repeat(8, 1).repeat(8, 2))
        vol = torch.from_numpy(vol_np).to(DEV)
        V = vol.numel()
        ws = torch.empty(lib().hdf_cc_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
        ids = torch.empty(shape, dtype=torch.int32, device=DEV)
        out = torch.empty_like(vol)
        res = torch.empty(2, dtype=torch.int64, device=DEV)
        table = torch.empty((4096, 9), dtype=torch.int64, device=DEV)
        st = stream_ptr()

        def label():
            check(lib().hdf_cc_label(ptr(vol), 0, connectivity, *shape, ptr(ids), ptr(res), ptr(ws), ws.numel(), st), "label")

        us_label = 1e3 * gpu_ms(label, reps=30, warm=5)
        n, fg = res.cpu().tolist()
        us_filter = 1e3 * gpu_ms(lambda: check(lib().hdf_cc_filter(ptr(vol), ptr(ids), *shape, 0, 1, ptr(out), ptr(res), ptr(ws),
                                                                    ws.numel(), st), "filter"), reps=30, warm=5)
        kept = res.cpu().tolist()
        us_table = 1e3 * gpu_ms(lambda: check(lib().hdf_cc_table(ptr(vol), ptr(ids), None, *shape, 4096, ptr(table), None, st),
                                              "table"), reps=30, warm=5)
        if ndi is not None:
            import scipy
            struct = ndi.generate_binary_structure(3, 3)

            def ref_chain():
                for k in (1, 2, 3):
                    lab, _ = ndi.label(vol_np == k, struct)
                    ndi.find_objects(lab)

            cpu = {"kind": "port", "what": f"scipy {scipy.__version__} ndimage.label + find_objects, three classes, structure 3x3x3",
                   "s_per_volume": cpu_s(ref_chain, reps=1), "threads": 1}
        else:
            cpu = {"kind": "not measured", "what": "scipy is not installed"}
        emit(row="connected components", config=f"{shape[0]}x{shape[1]}x{shape[2]} uint8, three classes, connectivity {connectivity}, label 0",
             components=n, foreground_voxels=fg, kept=kept, hdf_cc_label_us=us_label, hdf_cc_filter_us=us_filter,
             hdf_cc_table_us=us_table, voxels=V, label_ns_per_voxel=us_label * 1e3 / V, cpu_baseline=cpu)
        del vol, ws, ids, out
        torch.cuda.empty_cache()


def morphology_row(shapes=((144, 144, 144), (448, 512, 512))):
    """hdf_morph (dilate, 1 and 3 iterations, connectivity 6; close, 3 iterations, connectivity 18) and hdf_fill_holes
    (connectivity 6), each timed alone with label 0 in MASK mode on the three-class blob map of components_row, next to the
    scipy.ndimage calls on the same array, one host thread, copies not counted.  Bytes moved, hdf_morph with s steps in all:
    the byte map read by the pack and the unpack kernel and written once (3 V), a packed buffer of P bytes written by the
    pack kernel and read by the unpack kernel, read and written by every step (2 P + 2 s P).  hdf_fill_holes: only the
    passes of its own kernels over the maps are counted (the complement and the flags written, the map read twice, the ids
    read once, the output written: 9 V), not the labelling between them, whose traffic depends on the data."""
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    from scipy import ndimage as ndi
    import scipy
    for shape in shapes:
        rng = np.random.default_rng(15)
        low = ndi.gaussian_filter(rng.random(tuple(s // 8 for s in shape)), 1.5, mode="nearest")
        cls = np.digitize(low, np.quantile(low, [0.6, 0.8, 0.93])).astype(np.uint8)
        vol_np = np.ascontiguousarray(cls.repeat(8, 0).repeat(8, 1).repeat(8, 2))
        mask_np = vol_np != 0
        vol = torch.from_numpy(vol_np).to(DEV)
        V = vol.numel()
        P = shape[0] * shape[1] * ((shape[2] + 31) // 32) * 4
        ws = torch.empty(lib().hdf_morph_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
        out = torch.empty_like(vol)
        res = torch.empty(2, dtype=torch.int64, device=DEV)
        st = stream_ptr()
        rows = {}
        for name, op, conn, n, steps, ref in (
                ("dilate_1", 0, 6, 1, 1, lambda: ndi.binary_dilation(mask_np, ndi.generate_binary_structure(3, 1), 1)),
                ("dilate_3", 0, 6, 3, 3, lambda: ndi.binary_dilation(mask_np, ndi.generate_binary_structure(3, 1), 3)),
                ("close_3_c18", 3, 18, 3, 6, lambda: ndi.binary_closing(mask_np, ndi.generate_binary_structure(3, 2), 3))):
            us = 1e3 * gpu_ms(lambda: check(lib().hdf_morph(ptr(vol), 0, op, conn, n, 0, 0, *shape, ptr(out), ptr(res), ptr(ws),
                                                            ws.numel(), st), "hdf_morph"), reps=30, warm=5)
            moved = 3 * V + 2 * P + 2 * steps * P
            rows[name] = {"us": us, "bytes_moved": moved, "GBps": moved / us / 1e3, "result": res.cpu().tolist(),
                          "scipy_s": cpu_s(ref, reps=1)}
        del ws
        ws = torch.empty(lib().hdf_fill_holes_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
        us = 1e3 * gpu_ms(lambda: check(lib().hdf_fill_holes(ptr(vol), 0, 6, 0, *shape, ptr(out), ptr(res), ptr(ws), ws.numel(), st),
                                        "hdf_fill_holes"), reps=30, warm=5)
        rows["fill_holes_c6"] = {"us": us, "bytes_moved": 9 * V, "GBps": 9 * V / us / 1e3, "result": res.cpu().tolist(),
                                 "scipy_s": cpu_s(lambda: ndi.binary_fill_holes(mask_np), reps=1)}
        emit(row="morphology", config=f"{shape[0]}x{shape[1]}x{shape[2]} uint8, three classes, label 0, border_value 0, MASK mode",
             voxels=V, packed_bytes=P, cpu_baseline={"kind": "port", "what": f"scipy {scipy.__version__} ndimage.binary_*", "threads": 1},
             **rows)
        del vol, ws, out
        torch.cuda.empty_cache()


def lesions_row(shapes=((144, 144, 144), (448, 512, 512))):
    """hdf_cc_pairs (both zero flags, the truth map as the mask, 4096 rows) on the id maps hdf_cc_label gives a truth and
    a predicted blob map -- two smoothed 1/8-resolution noise fields that share most of their noise, thresholded to a few
    dozen lesions a map and repeated 8x along each axis -- and hdf_rt.match_components / lesion_wise_scores end to end on
    the two maps (wall time: labelling, dilation, the table, the one copy, the host part).  Two yardsticks of the same run:
    the host path (both id maps copied to the host, np.unique(..., return_counts=True) over the 64-bit keys, one thread),
    and hdf_cc_table on the predicted map, a pass of the same shape.  GBps: 9 bytes a voxel over the time of the whole
    entry (init, voxel pass, compaction, sort, rows)."""
    from hdf_rt import lesions
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    from hdf_rt.components import _label
    from scipy import ndimage as ndi
    for shape in shapes:
        rng = np.random.default_rng(17)
        low = tuple(s // 8 for s in shape)
        sigma, q = (1.5, 0.93) if low[0] * low[1] * low[2] < 50000 else (3.0, 0.97)
        f = ndi.gaussian_filter(rng.random(low), sigma, mode="nearest")
        g = f + 0.35 * ndi.gaussian_filter(rng.random(low) - 0.5, sigma, mode="nearest")
        up = lambda m: torch.from_numpy(np.ascontiguousarray(m.astype(np.uint8).repeat(8, 0).repeat(8, 1).repeat(8, 2))).to(DEV)
        truth, pred = up(f > np.quantile(f, q)), up(g > np.quantile(g, q))
        V = truth.numel()
        ids_p, res_p = _label(pred, 26, 0)
        ids_t, res_t = _label(truth, 26, 0)
        cap = 4096
        ws = torch.empty(lib().hdf_cc_pairs_workspace_bytes(cap), dtype=torch.uint8, device=DEV)
        pairs = torch.empty((cap, 4), dtype=torch.int64, device=DEV)
        res = torch.empty(4, dtype=torch.int64, device=DEV)
        table = torch.empty((cap, 9), dtype=torch.int64, device=DEV)
        st = stream_ptr()
        us_pairs = 1e3 * gpu_ms(lambda: check(lib().hdf_cc_pairs(ptr(ids_p), ptr(ids_t), ptr(truth), 3, *shape, cap, ptr(pairs),
                                                                 ptr(res), ptr(ws), ws.numel(), st), "hdf_cc_pairs"), reps=30, warm=5)
        us_nomask = 1e3 * gpu_ms(lambda: check(lib().hdf_cc_pairs(ptr(ids_p), ptr(ids_t), None, 0, *shape, cap, ptr(pairs),
                                                                  ptr(res), ptr(ws), ws.numel(), st), "hdf_cc_pairs"), reps=30, warm=5)
        us_table = 1e3 * gpu_ms(lambda: check(lib().hdf_cc_table(ptr(pred), ptr(ids_p), None, *shape, cap, ptr(table), None, st),
                                              "hdf_cc_table"), reps=30, warm=5)
        check(lib().hdf_cc_pairs(ptr(ids_p), ptr(ids_t), ptr(truth), 3, *shape, cap, ptr(pairs), ptr(res), ptr(ws), ws.numel(), st),
              "hdf_cc_pairs")
        result = res.cpu().tolist()

        def host_path():
            a, b = ids_p.cpu().numpy().ravel().astype(np.int64), ids_t.cpu().numpy().ravel().astype(np.int64)
            return np.unique((a << 32) | b, return_counts=True)

        def wall(fn, reps):
            fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
            return sorted(ts)[len(ts) // 2]

        t = time.perf_counter()
        keys, _ = host_path()
        host_s = time.perf_counter() - t
        ms_match = 1e3 * wall(lambda: lesions.match_components(pred, truth), 5)
        ms_lw = 1e3 * wall(lambda: lesions.lesion_wise_scores(pred, truth, 1), 5)
        lw = lesions.lesion_wise_scores(pred, truth, 1)
        emit(row="lesions", config=f"{shape[0]}x{shape[1]}x{shape[2]}, two uint8 blob maps, connectivity 26, capacity {cap}",
             voxels=V, pred_components=res_p.cpu().tolist()[0], truth_components=res_t.cpu().tolist()[0], pairs_result=result,
             host_pairs=int(len(keys) - 1), hdf_cc_pairs_us=us_pairs, hdf_cc_pairs_no_mask_no_flags_us=us_nomask,
             hdf_cc_table_us=us_table, pairs_GBps_at_9B_per_voxel=9 * V / us_pairs / 1e3,
             no_mask_GBps_at_8B_per_voxel=8 * V / us_nomask / 1e3, match_components_ms=ms_match, lesion_wise_scores_ms=ms_lw,
             lesion_dice=lw["lesion_dice"], lesion_false_positives=lw["fp"],
             cpu_baseline={"kind": "port", "what": "D2H copy of both int32 id maps + np.unique(a << 32 | b, return_counts=True)",
                           "s_per_volume": host_s, "threads": 1})
        del truth, pred, ids_p, ids_t, ws
        lesions.clear_workspaces()
        from hdf_rt import surface
        surface.clear_workspaces()
        torch.cuda.empty_cache()


def detect_row(shapes=((24, 384, 384), (160, 160, 160))):
    """hdf_rt.extract_lesion_candidates (defaults: five lesions, peak / 2.5, connectivity 6, remove_adjacent, chunks of
    eight rounds) on a blob-like fp32 probability map resident on the device -- a smoothed 1/8-resolution noise field cut at
    its 93rd percentile, interpolated up, with 0.5 % noise voxels -- as wall time around the call (median of 5; it ends in
    its own D2H copies), and one hdf_detect_candidates call of eight rounds by HIP events (median of 10 after 3): the first
    rounds extract, the rest run on an empty mask.  The yardstick of the same run: the map copied to the host and the loop
    with scipy.ndimage.label / binary_dilation a user writes today, one run, one host thread; its table must equal the
    device's in every word."""
    from hdf_rt import detection
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    from scipy import ndimage as ndi
    for shape in shapes:
        rng = np.random.default_rng(23)
        low = tuple(max(s // 8, 2) for s in shape)
        f = ndi.gaussian_filter(rng.random(low), 1.5, mode="nearest")
        f = np.clip((f - np.quantile(f, 0.93)) / (f.max() - np.quantile(f, 0.93)), 0.0, 1.0)
        p = (0.9 * ndi.zoom(f, [s / l for s, l in zip(shape, low)], order=1)).astype(np.float32)
        assert p.shape == shape
        noise = rng.random(shape) < 0.005
        p[noise] = rng.uniform(0.0, 0.3, int(noise.sum())).astype(np.float32)
        dp = torch.from_numpy(p).to(DEV)
        V = dp.numel()

        def host_path():
            w = dp.cpu().numpy().copy()
            idx, kept, rows = np.zeros(shape, np.int32), 0, []
            while kept < 5:
                a = int(np.argmax(w))
                m = w.reshape(-1)[a]
                if float(m) < 0.01:
                    break
                thr = float(m) / 2.5
                labels, _ = ndi.label(w.astype(np.float64) > thr)
                cur = labels == labels.reshape(-1)[a]
                status = 1 if (ndi.binary_dilation(idx > 0, np.ones((3, 3, 3), bool)) & cur).any() else 0
                if status == 0:
                    kept += 1
                    idx[cur] = kept
                w[cur] = 0
                rows.append([kept if status == 0 else 0, int(np.float32(m).view(np.uint32)), int(cur.sum()), a, status,
                             int(np.float64(thr).view(np.int64))])
            return rows

        def wall(fn, reps):
            fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
            return sorted(ts)[len(ts) // 2]

        t = time.perf_counter()
        rows = host_path()
        host_s = time.perf_counter() - t
        got = detection._extract(dp, 5, 2.5, 0.01, 6, True, 0, 256, 8)
        ms_call = 1e3 * wall(lambda: detection.extract_lesion_candidates(dp), 5)
        ws = torch.empty(lib().hdf_detect_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
        det, idx = torch.empty(shape, dtype=torch.float32, device=DEV), torch.empty(shape, dtype=torch.int32, device=DEV)
        table, res = torch.empty((256, 6), dtype=torch.int64, device=DEV), torch.empty(4, dtype=torch.int64, device=DEV)
        st = stream_ptr()
        ms_chunk = gpu_ms(lambda: check(lib().hdf_detect_candidates(ptr(dp), *shape, 5, 2.5, 0.01, 6, 1, 0, 0, 8, ptr(det), ptr(idx),
                                                                    ptr(table), 256, ptr(res), ptr(ws), ws.numel(), st),
                                        "hdf_detect_candidates"))
        emit(row="detect", config=f"{shape[0]}x{shape[1]}x{shape[2]} fp32 map, 5 lesions, factor 2.5, connectivity 6, sync_every 8",
             voxels=V, rounds=got[3][0], kept=got[3][1], finished=got[3][2], d2h_copies=got[4], tables_equal=got[2] == rows,
             extract_lesion_candidates_ms=ms_call, one_call_of_8_rounds_ms=ms_chunk, rounds_in_that_call=res.cpu().tolist()[0],
             cpu_baseline={"kind": "port", "what": "D2H copy of the fp32 map + the scipy.ndimage.label / binary_dilation loop",
                           "s_per_volume": host_s, "threads": 1})
        del dp, ws, det, idx
        detection.clear_workspaces()
        torch.cuda.empty_cache()


def slice2d_row(C=3, D=24, S=384, slice_batch=24):
    """slice_predict of HDenseFormer_2D_32(3, 2, (384, 384), 24) on a 3 x 24 x 384^2 volume (the reference's 2-D workload,
    config.py:69-77; bf16, one in-plane window, no mirroring: one hdf_plane_max, one hdf_slice_gather, one forward of 24
    slices, one hdf_slice_accumulate, one hdf_sw_finalize), next to two figures of the same run: the eval forward of the 24
    slices alone, and the same volume through the per-window entries driven with windows of depth 1 -- a copy (the
    normalisation is in place), MRNormalize per plane as chunked mr_normalize_ calls (64 planes a call), one hdf_sw_gather
    and one hdf_sw_accumulate_tta per slice, the same forward and vote.  Medians of 30 calls after 5, with the extremes."""
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    from models.HDenseFormer_2D import HDenseFormer_2D_32
    gen = torch.Generator().manual_seed(16)
    net = HDenseFormer_2D_32(C, 2, (S, S), 24).to(DEV).eval()
    net.compute_dtype = "bf16"
    vol = (torch.rand(C, D, S, S, generator=gen) * 900).to(DEV)
    x = torch.rand(slice_batch, C, S, S, generator=gen).to(DEV)
    pv, st = S * S, stream_ptr()

    def per_window():
        v = vol.clone()
        planes = v.view(C * D, S, S)
        for i in range(0, C * D, 64):
            inference.mr_normalize_(planes[i:i + 64])
        psum, wsum = torch.zeros((2, D, S, S), device=DEV), torch.zeros((D, S, S), device=DEV)
        for z0 in range(0, D, slice_batch):
            nz = min(slice_batch, D - z0)
            data = torch.empty((nz, C, S, S), device=DEV)
            for k in range(nz):
                check(lib().hdf_sw_gather(ptr(v), C, D, S, S, z0 + k, 0, 0, 1, S, S, 1, S, S, 0, ptr(data) + k * C * pv * 4, st),
                      "hdf_sw_gather")
            logits = net(data)[0].contiguous()
            per = 2 * pv * logits.element_size()
            for k in range(nz):
                check(lib().hdf_sw_accumulate_tta(inference._SW_DT[logits.dtype], ptr(logits) + k * per, 0, 2, 1, S, S, 1, S, S,
                                                  None, None, ptr(psum), ptr(wsum), D, S, S, z0 + k, 0, 0, st),
                      "hdf_sw_accumulate_tta")
        label = torch.empty((D, S, S), dtype=torch.uint8, device=DEV)
        check(lib().hdf_sw_finalize(ptr(psum), ptr(wsum), 2, D * pv, ptr(label), st), "hdf_sw_finalize")
        return label

    def timed(fn):
        for _ in range(5):
            fn()
        ts = sorted(gpu_ms(fn, reps=1, warm=0) for _ in range(30))
        return {"median_ms": ts[15], "min_ms": ts[0], "max_ms": ts[-1]}

    with torch.no_grad():
        same = bool(torch.equal(inference.slice_predict(net, vol, slice_batch), per_window()))
        a = timed(lambda: inference.slice_predict(net, vol, slice_batch))
        b = timed(lambda: net(x))
        c = timed(per_window)
    emit(row="slice2d", config=f"HDenseFormer_2D_32({C}, 2, ({S}, {S}), 24) bf16, {C}x{D}x{S}^2 fp32 volume, slice_batch {slice_batch}, "
         "normalize 'mr', no importance, no mirroring", slice_predict=a, forward_alone=b, per_window_entries=c,
         library_launches_beside_the_forward={"slice_predict": 4, "per_window_entries": 3 * (-(-C * D // 64)) + 2 * D + 1},
         labels_equal=same, tail_ms={"slice_predict": a["median_ms"] - b["median_ms"],
                                     "per_window_entries": c["median_ms"] - b["median_ms"]})


if sys.argv[1:] == ["slice2d"]:
    slice2d_row()
    sys.exit(0)
if sys.argv[1:] == ["components"]:
    components_row()
    sys.exit(0)
if sys.argv[1:] == ["morphology"]:
    morphology_row()
    sys.exit(0)
if sys.argv[1:] == ["lesions"]:
    lesions_row()
    sys.exit(0)
if sys.argv[1:] == ["detect"]:
    detect_row()
    sys.exit(0)
if sys.argv[1:] == ["resize3d"]:
    resize3d_row()
    sys.exit(0)
if sys.argv[1:] == ["augment"]:
    augment_row()
    sys.exit(0)
if sys.argv[1:] == ["augment2d"]:
    augment2d_row()
    sys.exit(0)
if sys.argv[1:] == ["transforms2d"]:
    transforms2d_row()
    sys.exit(0)

g = torch.Generator().manual_seed(7)
B, C, S = 2, 4, 128
vox = S ** 3
logits = torch.randn(B, C, S, S, S, generator=g).to(DEV).to(torch.bfloat16)
lab = torch.randint(0, C, (B, S, S, S), generator=g, dtype=torch.uint8)
onehot = torch.nn.functional.one_hot(lab.long(), C).permute(0, 4, 1, 2, 3).float().contiguous().to(DEV)
lab_d = lab.to(DEV)

# ---- 8f-1: step metrics
ms = gpu_ms(lambda: compute_dice(logits, onehot))
by = logits.numel() * 2 + onehot.numel() * 4
lg_c, oh_c = logits[:1].float().cpu(), onehot[:1].cpu()


def ref_dice():   # trainer.py:919-945 on the host, one sample: softmax, argmax, per-class overlap
    p = torch.softmax(lg_c, 1).argmax(1)
    t = oh_c.argmax(1)
    return [float(2 * ((p == c) & (t == c)).sum() / (((p == c).sum() + (t == c).sum()).clamp(min=1))) for c in range(1, C)]


emit(row="8f-1 compute_dice", config=f"{B}x{C}x{S}^3 bf16 logits + fp32 one-hot", gpu_ms=ms, algorithmic_bytes=by,
     achieved_GBps=by / ms / 1e6, hbm_peak_GBps=8000, cpu_baseline={"kind": "port", "what": "torch CPU softmax+argmax+overlap, one sample",
                                                                     "s_per_sample": cpu_s(ref_dice), "threads": torch.get_num_threads()})
rd = RunningDice(list(range(C)), ignore_label=-1)
ms = gpu_ms(lambda: rd.update_from_logits(onehot, logits))
gt_np, pr_np = lab[:1].numpy().ravel(), lg_c.argmax(1).numpy().ravel().astype(np.uint8)
emit(row="8f-1 RunningDice.update_matrix", config=f"{B}x{C}x{S}^3 (one-hot, logits) -> {C}x{C} counts", gpu_ms=ms,
     algorithmic_bytes=by, achieved_GBps=by / ms / 1e6, hbm_peak_GBps=8000,
     cpu_baseline={"kind": "port", "what": "numpy bincount confusion matrix of two label maps, one sample (metrics.py:104-133 without the D2H)",
                   "s_per_sample": cpu_s(lambda: np.bincount(gt_np.astype(np.int64) * C + pr_np, minlength=C * C)), "threads": 1})

# ---- 8f-3: staging
ms = gpu_ms(lambda: inference.onehot_from_labels(lab_d, C))
by = lab_d.numel() + lab_d.numel() * C * 4
emit(row="8f-3 onehot_from_labels", config=f"{B}x{S}^3 uint8 -> fp32 one-hot", gpu_ms=ms, algorithmic_bytes=by,
     achieved_GBps=by / ms / 1e6, hbm_peak_GBps=8000,
     cpu_baseline={"kind": "port", "what": "numpy one-hot of one sample (data_loader.py:146-151)", "threads": 1,
                   "s_per_sample": cpu_s(lambda: np.stack([(lab[0].numpy() == c) for c in range(C)]).astype(np.float32))})
vol = torch.rand(C, S, S, S, generator=g).to(DEV) * 900
ms = gpu_ms(lambda: inference.mr_normalize_(vol.clone()))
ms0 = gpu_ms(lambda: vol.clone())
by = vol.numel() * 4 * 3      # statistics pass + read + write
vol_np = vol.cpu().numpy()


def ref_mr():
    out = np.empty_like(vol_np)
    for c in range(C):
        v = vol_np[c]
        out[c] = (v - v.min()) / max(v.max() - v.min(), 1e-8)
    return out


emit(row="8f-3 mr_normalize_", config=f"{C}x{S}^3 fp32 in place (clone time {ms0:.3f} ms subtracted)", gpu_ms=ms - ms0,
     algorithmic_bytes=by, achieved_GBps=by / max(ms - ms0, 1e-6) / 1e6, hbm_peak_GBps=8000,
     cpu_baseline={"kind": "port", "what": "numpy per-channel min/max rescale of the same volume", "s_per_sample": cpu_s(ref_mr),
                   "threads": 1})

augment_row()
augment2d_row()
transforms2d_row()
slice2d_row()
torch.cuda.empty_cache()

# ---- 8f-2: sliding-window inference
from models.HDenseFormer import HDenseFormer
net = HDenseFormer(4, 4, 32, image_size=(128, 128, 128), transformer_depth=24).to(DEV)
net.compute_dtype = "bf16"
net.eval()
big = torch.rand(4, 192, 192, 160, generator=g).to(DEV)
steps = inference.cal_steps(tuple(big.shape[1:]), (128, 128, 128), (64, 64, 64))
nwin = len(steps[0]) * len(steps[1]) * len(steps[2])
for wb in (1, 4):
    ms = gpu_ms(lambda: inference.sliding_window_predict(net, big, (128, 128, 128), (64, 64, 64), window_batch=wb), reps=3, warm=1)
    emit(row="8f-2 sliding_window_predict", config=f"4x192x192x160 volume, 128^3 patch, step 64: {nwin} windows, window_batch={wb}, bf16",
         gpu_ms=ms, windows_per_s=nwin / ms * 1e3, ms_per_window=ms / nwin)
xb = torch.rand(4, 4, 128, 128, 128, generator=g).to(DEV)
with torch.no_grad():
    ms = gpu_ms(lambda: net(xb), reps=5, warm=2)
emit(row="8f-2 (forward alone)", config="4 windows of 4x128^3 in one eval forward, bf16", gpu_ms=ms, ms_per_window=ms / 4)
del net, xb, big
torch.cuda.empty_cache()

# ---- 8f-4: the 2-D model (BASELINE configs[0] geometry: 4 channels, 256^2)
from loss.combine_loss import CEPlusDice, DeepSuperloss
from models.HDenseFormer_2D import HDenseFormer_2D_32
net2 = HDenseFormer_2D_32(4, 2, (256, 256), 24).to(DEV)
net2.compute_dtype = "bf16"
x2 = torch.rand(2, 4, 256, 256, generator=g).to(DEV)
net2.eval()
with torch.no_grad():
    ms = gpu_ms(lambda: net2(x2), reps=5, warm=2)
emit(row="8f-4 HDenseFormer_2D_32 eval forward", config="batch 2 of 4x256^2, n_cls 2, td 24, bf16 (native depth-1 path, round 6)",
     gpu_ms=ms, samples_per_s=2 / ms * 1e3)
net2.train()
crit = DeepSuperloss(criterion=CEPlusDice(weight=None, ignore_index=0))
opt = FlatAdam(net2, lr=1e-3, weight_decay=1e-4)
t2 = torch.nn.functional.one_hot(torch.randint(0, 2, (2, 256, 256), generator=g), 2).permute(0, 3, 1, 2).float().contiguous().to(DEV)


def step2():
    opt.zero_grad()
    loss = crit(net2(x2), t2)
    loss.backward()
    opt.step()


ms = gpu_ms(step2, reps=5, warm=2)
emit(row="8f-4 HDenseFormer_2D_32 train step", config="batch 2 of 4x256^2, fwd + DeepSuper CE+Dice + bwd + Adam, bf16", gpu_ms=ms,
     samples_per_s=2 / ms * 1e3)

# ---- 8f-4 at the reference's own 2-D workload: PI-CAI 384^2, batch 24 (config.py:69-77), the model of test.py:4-13
del net2, opt
torch.cuda.empty_cache()
try:
    net3 = HDenseFormer_2D_32(2, 2, (384, 384), 16).to(DEV)
    net3.compute_dtype = "bf16"
    x3 = torch.rand(24, 2, 384, 384, generator=g).to(DEV)
    net3.eval()
    with torch.no_grad():
        ms = gpu_ms(lambda: net3(x3), reps=3, warm=1)
    emit(row="8f-4 HDenseFormer_2D_32 eval forward, PI-CAI shape", config="batch 24 of 2x384^2, n_cls 2, td 16, bf16 (native depth-1 path, round 6)",
         gpu_ms=ms, samples_per_s=24 / ms * 1e3)
    net3.train()
    opt3 = FlatAdam(net3, lr=1e-3, weight_decay=1e-4)
    t3 = torch.nn.functional.one_hot(torch.randint(0, 2, (24, 384, 384), generator=g), 2).permute(0, 3, 1, 2).float().contiguous().to(DEV)

    def step3():
        opt3.zero_grad()
        loss = crit(net3(x3), t3)
        loss.backward()
        opt3.step()

    ms = gpu_ms(step3, reps=3, warm=1)
    emit(row="8f-4 HDenseFormer_2D_32 train step, PI-CAI shape", config="batch 24 of 2x384^2, fwd + DeepSuper CE+Dice + bwd + Adam, bf16",
         gpu_ms=ms, samples_per_s=24 / ms * 1e3)
    # the loss the reference trainer builds for this two-class workload (config.py:127, trainer.py:755-757)
    from loss.cross_entropy import FocalLoss
    crit_fl = DeepSuperloss(criterion=FocalLoss(reduction="sum"))

    def step3_focal():
        opt3.zero_grad()
        loss = crit_fl(net3(x3), t3)
        loss.backward()
        opt3.step()

    ms = gpu_ms(step3_focal, reps=3, warm=1)
    emit(row="8f-4 HDenseFormer_2D_32 train step, PI-CAI shape, focal loss",
         config="batch 24 of 2x384^2, fwd + DeepSuper FocalLoss('sum') + bwd + Adam, bf16", gpu_ms=ms,
         samples_per_s=24 / ms * 1e3)
except Exception as exc:  # report, do not hide: the row then says why it is missing
    emit(row="8f-4 PI-CAI shape", error=repr(exc)[:300])
