"""Sliding-window inference on the device (reference: SemanticSeg.inference_slidingwindow / cal_steps,
trainer.py:488-618).  The reference runs every window through the net, takes the softmax on the GPU, then adds into two
full-size fp32 accumulators with indexed torch ops and finally argmaxes a softmax of their quotient on the GPU and
moves it to the host.  Here the per-window tail (softmax + accumulate + count) is ONE HIP kernel reading the logits
once, the vote is one kernel writing a uint8 map; the model is the MI355X-native HDenseFormer.  No CPU fallback.
Two options the reference only sketches stay on the device as well: its Gaussian importance map (get_gaussian,
trainer.py:620-638, bit for bit) and mirror test-time augmentation (csrc/sw_infer.hip).  slice_predict does the same for
the 2-D model, slice by slice (eval.py:125-230; csrc/slice_infer.hip), and returns the same uint8 map."""
import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

_SW_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def cal_steps(image_size, patch_size, step_size):
    """Window origins along every axis (reference: SemanticSeg.cal_steps, trainer.py:595-618): an axis no longer than
    the patch gets the single origin 0; otherwise the span `size - patch` is covered by the fewest windows whose
    spacing does not exceed `step`, spread evenly (rounded), so that the last window ends at the volume's end."""
    origins = []
    for size, patch, step in zip(image_size, patch_size, step_size):
        span = size - patch
        if span <= 0:
            origins.append([0])
            continue
        n = int(np.ceil(span / step)) + 1
        origins.append([int(np.round(span / (n - 1) * k)) for k in range(n)])
    return origins


def gaussian_tables(extent, sigma_scale=1. / 8):
    """Per-axis factors of the reference's importance map (SemanticSeg.get_gaussian, trainer.py:620-638): three fp64
    vectors tz, ty, tx such that scipy.ndimage.gaussian_filter of a unit impulse at the centre n // 2 of every axis,
    sigma = n * sigma_scale, mode='constant', equals (tz[z] * ty[y]) * tx[x] in every bit.  Per axis that filter is a
    correlation with the kernel exp(-0.5 / sigma^2 * j^2), |j| <= int(4 sigma + 0.5), normalised to sum 1: of the impulse
    it leaves the kernel itself, cut where it leaves the axis.  Host-side numpy; include/hdf.h (hdf_sw_accumulate_tta)
    states how the kernels turn the tables into weights."""
    tables = []
    for n in extent:
        n = int(n)
        sigma = n * float(sigma_scale)
        if n < 1 or not sigma > 0:
            raise ValueError(f"gaussian_tables: extent {tuple(extent)} and sigma_scale {sigma_scale} must be positive")
        r = int(4.0 * sigma + 0.5)
        k = np.exp(-0.5 / (sigma * sigma) * np.arange(-r, r + 1) ** 2)
        k = k / k.sum()
        off = np.arange(n) - n // 2
        inside = np.abs(off) <= r
        t = np.zeros(n, dtype=np.float64)
        t[inside] = k[off[inside] + r]
        tables.append(t)
    return tuple(tables)


def _mirror_mask(mirror_axes):
    """axes of [D, H, W] -> the C ABI's mask (bit 0 = z, 1 = y, 2 = x)"""
    mask = 0
    for a in tuple(mirror_axes):
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (0, 1, 2) or mask >> int(a) & 1:
            raise ValueError(f"mirror_axes must be a subset of (0, 1, 2) without repeats, got {mirror_axes!r}")
        mask |= 1 << int(a)
    return mask


def _accumulate_tta(net, image, origins, ext, patch, psum, wsum, window_batch, mask, tables):
    """The window loop with importance weights (tables: gaussian_tables of the extent, or None) and / or mirroring: per
    group of windows one hdf_sw_gather per window into the forward's batch [windows x K variants], one forward, one
    hdf_sw_accumulate_tta per window.  The tables and the map's floor go to the device once; nothing waits on the host."""
    dev = image.device
    n_cls, size, ch = psum.shape[0], tuple(psum.shape[1:]), image.shape[0]
    K = 1 << bin(mask).count("1")
    tab = floor = None
    if tables is not None:
        tab = torch.from_numpy(np.concatenate(tables)).to(dev)
        floor = torch.empty(1, device=dev)
        check(lib().hdf_sw_importance_floor(ptr(tab), *ext, ptr(floor), stream_ptr()), "hdf_sw_importance_floor")
    per_group = max(1, window_batch // K)
    pvox = patch[0] * patch[1] * patch[2]
    for i0 in range(0, len(origins), per_group):
        group = origins[i0:i0 + per_group]
        data = torch.empty((len(group) * K, ch) + patch, device=dev)
        for k, origin in enumerate(group):
            check(lib().hdf_sw_gather(ptr(image), ch, *size, *origin, *ext, *patch, mask,
                                      ptr(data) + k * K * ch * pvox * 4, stream_ptr()), "hdf_sw_gather")
        logits = net(data)[0]
        if logits.dtype not in _SW_DT:
            raise _lib.HdfError(f"unsupported logits dtype {logits.dtype}")
        logits = logits.contiguous()
        per = K * n_cls * pvox * logits.element_size()
        for k, origin in enumerate(group):
            check(lib().hdf_sw_accumulate_tta(_SW_DT[logits.dtype], ptr(logits) + k * per, mask, n_cls, *ext, *patch,
                                              ptr(tab), ptr(floor), ptr(psum), ptr(wsum), *size, *origin, stream_ptr()),
                  "hdf_sw_accumulate_tta")


@torch.no_grad()
def sliding_window_predict(net, image, patch_size, step_size, return_probabilities=False, window_batch=4, *,
                           importance=None, sigma_scale=1. / 8, mirror_axes=()):
    """image: [C, D, H, W] (numpy or tensor, any device).  Returns the uint8 label volume [D, H, W] on the model's
    device (and the mean class probabilities when asked).

    importance='gaussian' weights every window voxel by the reference's get_gaussian map (sigma = extent * sigma_scale
    per axis; gaussian_tables), so that a voxel at a window's border counts less than one at its centre; mirror_axes, a
    subset of the axes (0, 1, 2) of [D, H, W], also runs every window mirrored along each subset of those axes and averages
    the un-mirrored softmaxes.  With either, a window costs three launches beside its forward (hdf_sw_gather, the forward
    of its K = 2^len(mirror_axes) variants as one batch, hdf_sw_accumulate_tta), `window_batch // K` windows (at least
    one) share a forward, and the probabilities returned are prob_sum / weight_sum.  With neither (the defaults) the
    call is what it was before these options existed, launch for launch.

    Reference loop: trainer.py:527-584.  Windows are gathered `window_batch` at a time into ONE forward of the plan
    (the reference runs them one by one).  An axis shorter than the patch yields the reference's clipped window
    (trainer.py:529-541: `ub = x + patch if it fits else the volume's end`); the reference would hand that smaller
    tensor to the net, which HDenseFormer itself cannot take (its position embeddings fix the token grid), so the
    window is zero-padded up to the patch, run, and only the logits over the real voxels are accumulated."""
    psum, cnt = _sliding_window_sums(net, image, patch_size, step_size, window_batch, importance, sigma_scale, mirror_axes)
    label = torch.empty(psum.shape[1:], dtype=torch.uint8, device=psum.device)
    check(lib().hdf_sw_finalize(ptr(psum), ptr(cnt), psum.shape[0], psum[0].numel(), ptr(label), stream_ptr()),
          "hdf_sw_finalize")
    if return_probabilities:
        return label, psum / cnt
    return label


@torch.no_grad()
def _sliding_window_sums(net, image, patch_size, step_size, window_batch, importance, sigma_scale, mirror_axes):
    """the two accumulators of sliding_window_predict before the vote: prob_sum [n_cls, D, H, W] and the count (the sum
    of the weights under an importance map) [D, H, W], fp32 on the model's device"""
    if importance not in (None, "gaussian"):
        raise ValueError(f"importance must be None or 'gaussian', got {importance!r}")
    mask = _mirror_mask(mirror_axes)
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise _lib.HdfError("sliding_window_predict needs the model on a GPU (there is no CPU path)")
    image = torch.as_tensor(image).float().to(dev)
    if image.dim() != 4:
        raise ValueError(f"image must be [C, D, H, W], got {tuple(image.shape)}")
    size = tuple(int(s) for s in image.shape[1:])
    patch = tuple(int(p) for p in patch_size)
    if patch != tuple(net.image_size):
        raise ValueError(f"patch {patch} differs from the model's image_size {tuple(net.image_size)}")
    ext = tuple(min(s, p) for s, p in zip(size, patch))          # clipped window extent (trainer.py:529-541)
    was_training = net.training
    net.eval()
    n_cls = net.n_cls
    psum = torch.zeros((n_cls,) + size, device=dev)
    cnt = torch.zeros(size, device=dev)
    steps = cal_steps(size, patch, step_size)
    origins = [(x, y, z) for x in steps[0] for y in steps[1] for z in steps[2]]
    wb = max(1, int(window_batch))
    try:
        if importance is None and not mask:
            _accumulate_plain(net, image, origins, ext, patch, psum, cnt, wb)
        else:
            tables = gaussian_tables(ext, sigma_scale) if importance else None
            _accumulate_tta(net, image.contiguous(), origins, ext, patch, psum, cnt, wb, mask, tables)
    finally:
        net.train(was_training)
    return psum, cnt


def _accumulate_plain(net, image, origins, ext, patch, psum, cnt, wb):
    """the window loop without options: `wb` windows per forward, one hdf_sw_accumulate per window"""
    dev, n_cls, size = image.device, psum.shape[0], tuple(psum.shape[1:])
    for i0 in range(0, len(origins), wb):
        group = origins[i0:i0 + wb]
        if ext == patch:
            data = torch.stack([image[:, x:x + patch[0], y:y + patch[1], z:z + patch[2]] for x, y, z in group])
        else:
            data = torch.zeros((len(group), image.shape[0]) + patch, device=dev)
            for k, (x, y, z) in enumerate(group):
                data[k, :, :ext[0], :ext[1], :ext[2]] = image[:, x:x + ext[0], y:y + ext[1], z:z + ext[2]]
        logits = net(data.contiguous())[0]
        if logits.dtype not in _SW_DT:
            raise _lib.HdfError(f"unsupported logits dtype {logits.dtype}")
        if ext != patch:
            logits = logits[:, :, :ext[0], :ext[1], :ext[2]]
        logits = logits.contiguous()
        per = logits[0].numel() * logits.element_size()
        for k, (x, y, z) in enumerate(group):
            check(lib().hdf_sw_accumulate(_SW_DT[logits.dtype], ptr(logits) + k * per, n_cls, ext[0], ext[1],
                                          ext[2], ptr(psum), ptr(cnt), size[0], size[1], size[2], x, y, z,
                                          stream_ptr()), "hdf_sw_accumulate")


_NORM_MODE = {None: 0, "mr": 1, "max": 2}


def _plane_mirror_mask(mirror_axes):
    """axes of the plane [H, W] -> the C ABI's mask of the slice entries (bit 0 = y, 1 = x)"""
    mask = 0
    for a in tuple(mirror_axes):
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (0, 1) or mask >> int(a) & 1:
            raise ValueError(f"mirror_axes must be a subset of (0, 1) without repeats, got {mirror_axes!r}")
        mask |= 1 << int(a)
    return mask


def plane_floor(tables):
    """the smallest non-zero weight of the plane's importance map: float((ty[y] * tx[x]) / (ty[eh/2] * tx[ew/2])) over the
    window, from the two host tables of gaussian_tables((eh, ew)) -- what hdf_slice_accumulate takes as `floor`"""
    ty, tx = tables
    raw = ((ty[:, None] * tx[None, :]) / (ty[len(ty) // 2] * tx[len(tx) // 2])).astype(np.float32)
    return float(raw[raw != 0].min())


@torch.no_grad()
def slice_predict(net, volume, slice_batch=24, *, normalize="mr", step_size=None, importance=None, sigma_scale=1. / 8,
                  mirror_axes=(), return_probabilities=False):
    """Slice-wise inference of a volume with the 2-D model (reference: eval.py:125-230, which normalises every plane,
    pushes the slices through the net, takes the softmax, stacks to [n_cls, D, H, W] and argmaxes on the host).
    volume: [C, D, H, W] (numpy or tensor, any device).  Returns the uint8 label volume [D, H, W] on the model's device --
    what sliding_window_predict returns for the 3-D model -- and, when asked, prob_sum / weight_sum as [n_cls, D, H, W],
    the array predict_process returns after its transpose.

    normalize: "mr" is MRNormalize plane by plane (data_loader.py:39-50, the validation chain of trainer.py:173-176),
    "max" is eval.py's Normalize_2d (the same without the clamp of negatives), None takes the planes as they are; the
    maximum is that of the whole plane [H, W] of a channel.  In the plane the windows follow sliding_window_predict's
    rules: an axis no longer than the model's image_size gives the origin 0 and a zero-padded clipped window, a longer
    one is covered by cal_steps with step_size (default: half the patch, the ratio of config.py:118-119).
    importance='gaussian' weights a window's pixels by get_gaussian((eh, ew)) (trainer.py:620-638); mirror_axes, a subset
    of the axes (0, 1) of the plane, also runs every slice mirrored along each subset of them and averages the
    un-mirrored softmaxes.  In-plane origins outer, slices inner, in groups of max(1, slice_batch // K), K =
    2^len(mirror_axes): a group costs one hdf_slice_gather, one forward of [slices x K variants] and one
    hdf_slice_accumulate; a call adds one hdf_plane_max and one hdf_sw_finalize.  Nothing waits on the host.  The
    defaults with normalize="max" on planes of the model's size are eval.py:208-230."""
    psum, wsum = _slice_sums(net, volume, slice_batch, normalize, step_size, importance, sigma_scale, mirror_axes)
    label = torch.empty(psum.shape[1:], dtype=torch.uint8, device=psum.device)
    check(lib().hdf_sw_finalize(ptr(psum), ptr(wsum), psum.shape[0], psum[0].numel(), ptr(label), stream_ptr()),
          "hdf_sw_finalize")
    if return_probabilities:
        return label, psum / wsum
    return label


@torch.no_grad()
def _slice_sums(net, volume, slice_batch, normalize, step_size, importance, sigma_scale, mirror_axes):
    """the two accumulators of slice_predict before the vote: prob_sum [n_cls, D, H, W] and weight_sum [D, H, W], fp32 on
    the model's device"""
    if importance not in (None, "gaussian"):
        raise ValueError(f"importance must be None or 'gaussian', got {importance!r}")
    if normalize not in _NORM_MODE:
        raise ValueError(f"normalize must be 'mr', 'max' or None, got {normalize!r}")
    mask = _plane_mirror_mask(mirror_axes)
    from models.HDenseFormer_2D import HDenseFormer_2D
    if not isinstance(net, HDenseFormer_2D):
        raise ValueError(f"slice_predict takes a HDenseFormer_2D (sliding_window_predict runs the 3-D model), got "
                         f"{type(net).__name__}")
    dev = next(net.parameters()).device
    if dev.type != "cuda":
        raise _lib.HdfError("slice_predict needs the model on a GPU (there is no CPU path)")
    volume = torch.as_tensor(volume).float().to(dev).contiguous()
    if volume.dim() != 4 or volume.shape[0] != net.in_channels:
        raise ValueError(f"volume must be [{net.in_channels}, D, H, W], got {tuple(volume.shape)}")
    ch, depth = int(volume.shape[0]), int(volume.shape[1])
    plane = tuple(int(s) for s in volume.shape[2:])
    patch = tuple(int(p) for p in net.image_size)
    step = tuple(max(1, p // 2) for p in patch) if step_size is None else tuple(int(s) for s in step_size)
    if len(step) != 2 or min(step) < 1:
        raise ValueError(f"step_size must be two positive steps (y, x), got {step_size!r}")
    ext = tuple(min(s, p) for s, p in zip(plane, patch))          # clipped window extent, as in the 3-D loop
    K = 1 << bin(mask).count("1")
    per_group = max(1, int(slice_batch) // K)
    n_cls, mode = net.n_cls, _NORM_MODE[normalize]
    tab, floor = None, 0.0
    if importance:
        tables = gaussian_tables(ext, sigma_scale)
        tab, floor = torch.from_numpy(np.concatenate(tables)).to(dev), plane_floor(tables)
    pmax = None
    if mode:
        pmax = torch.empty(ch * depth, device=dev)
        check(lib().hdf_plane_max(ptr(volume), ch * depth, plane[0] * plane[1], ptr(pmax), stream_ptr()), "hdf_plane_max")
    psum = torch.zeros((n_cls, depth) + plane, device=dev)
    wsum = torch.zeros((depth,) + plane, device=dev)
    steps = cal_steps(plane, patch, step)
    was_training = net.training
    if was_training:          # (a walk over the model's modules, about a millisecond: not for a net already in eval mode)
        net.eval()
    try:
        for y0 in steps[0]:
            for x0 in steps[1]:
                for z0 in range(0, depth, per_group):
                    nz = min(per_group, depth - z0)
                    data = torch.empty((nz * K, ch) + patch, device=dev)
                    check(lib().hdf_slice_gather(ptr(volume), ch, depth, *plane, z0, nz, y0, x0, *ext, *patch, mask, mode,
                                                 ptr(pmax), ptr(data), stream_ptr()), "hdf_slice_gather")
                    logits = net(data)[0]
                    if logits.dtype not in _SW_DT:
                        raise _lib.HdfError(f"unsupported logits dtype {logits.dtype}")
                    logits = logits.contiguous()
                    check(lib().hdf_slice_accumulate(_SW_DT[logits.dtype], ptr(logits), mask, n_cls, nz, *ext, *patch,
                                                     ptr(tab), floor, ptr(psum), ptr(wsum), depth, *plane, z0, y0, x0,
                                                     stream_ptr()), "hdf_slice_accumulate")
    finally:
        if was_training:
            net.train()
    return psum, wsum


def _normalize(image, mode, mean=0.0, w=1024.0):
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError("device-side normalisation needs a GPU tensor (there is no CPU path)")
    if image.dtype != torch.float32 or image.dim() < 2:
        raise ValueError("image must be a float32 tensor [C, ...]")
    img = image.contiguous()
    c, vox = img.shape[0], img[0].numel()
    ws = torch.empty(lib().hdf_normalize_workspace_bytes(c), dtype=torch.uint8, device=img.device)
    if mode == 0:
        check(lib().hdf_normalize_mr(ptr(img), c, vox, ptr(ws), stream_ptr()), "hdf_normalize_mr")
    else:
        check(lib().hdf_normalize_petct(ptr(img), c, vox, float(mean), float(w), ptr(ws), stream_ptr()),
              "hdf_normalize_petct")
    if img.data_ptr() != image.data_ptr():
        image.copy_(img)
    return image


def mr_normalize_(image):
    """MRNormalize (data_utils/data_loader.py:39-50) in place on a device sample [C, D, H, W]: the raw volume crosses
    PCIe once and is scaled where the step consumes it."""
    return _normalize(image, 0)


def pet_ct_normalize_(image, mean=0, w=1024):
    """PETandCTNormalize (data_utils/data_loader.py:53-68) in place on a device sample [2+, D, H, W]."""
    return _normalize(image, 1, mean, w)


def onehot_from_labels(labels, n_cls):
    """uint8 class map [N, D, H, W] (device tensor) -> fp32 one-hot [N, n_cls, D, H, W], the To_Tensor layout of
    data_utils/data_loader.py:146-151 (values >= n_cls count as background)."""
    if labels.device.type != "cuda":
        raise _lib.HdfError("onehot_from_labels needs a device tensor (there is no CPU path)")
    labels = labels.to(torch.uint8).contiguous()
    n = labels.shape[0]
    vox = labels[0].numel()
    out = torch.empty((n, n_cls) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    check(lib().hdf_onehot_from_labels(ptr(labels), ptr(out), n, n_cls, vox, stream_ptr()), "hdf_onehot_from_labels")
    return out
