"""Binary morphology on the device (csrc/morphology.hip, hdf_rt/morphology.py) against the numpy restatement of the
definitions in include/hdf.h (tests/morph_ref.py, itself held to live scipy by tests/test_morph_ref_cpu.py).

Shapes (morph_ref.SHAPES): (1,1,1); (1,37,70), the 2-D case; (4,5,W) for W = 31, 32, 33, 63, 64, 65 around the word
boundaries and (3,5,48), a row that ends on half a word; (5,3,300), a row longer than a workgroup; (19,67,131), odd on
every axis; the cap of 1024 on each axis in turn; (40,48,56), whose random fills carry three values.  Masks per shape
(morph_ref.MASKS): random fills at 0.2 / 0.5 / 0.8 / 0.97, empty, full, the corners and the centre, the 3-D checkerboard,
the end of a row beside the start of the next, a hollow box, a hollow box whose wall has a gap that only an 18- or
26-connected background passes, a hole that touches a face, nested boxes, two classes in contact.

Every (shape, mask) pair runs 36 of the 288 combinations of connectivity 6 / 18 / 26, the four ops, border_value 0 / 1,
iterations 1 / 2 / 3 / 17 and (MASK, label 0) / (MASK, label 2) / (MAP, label 2) (morph_ref.morph_params: every shape runs
every combination), every op once more in place, and fill holes for the three connectivities in the three mode / label pairs.
Every comparison is exact (morph_ref.mismatches): each byte of `out` and both result words.  Outputs are pre-filled with a
marker and carry a guard tail; the workspace of a shape is filled with 0x5A once and then reused by every call on every
mask without clearing; every call runs twice and the two outputs must agree.  Nothing here measures time: the largest
volume has 166 763 voxels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import morph_ref as mr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
MARK = 0xEE
IDS = ["%s-%s" % ("x".join(map(str, s)), k) for s, k in mr.CASES]
_ws = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(shape, fill):
    key = (shape, fill)
    if key not in _ws:
        n = (lib().hdf_fill_holes_workspace_bytes if fill else lib().hdf_morph_workspace_bytes)(*shape)
        assert n > 0
        _ws[key] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    return _ws[key]


def _call(vol, shape, in_place, enqueue):
    """enqueue(src, out, res) on a marked output with a guard tail -> (out uint8 shaped, [two result words])"""
    v = int(np.prod(shape))
    out = torch.full((v + GUARD,), MARK, dtype=torch.uint8, device=DEV)
    if in_place:
        out[:v] = vol.reshape(-1)
    res = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    enqueue(out if in_place else vol, out, res)
    o, r = out.cpu().numpy(), res.cpu().tolist()
    assert (o[v:] == MARK).all() and r[2] == -7, "write past the end of an output"
    return o[:v].reshape(shape), r[:2]


def _morph(vol, shape, conn, op, bv, n, mode, label, in_place=False):
    ws = _workspace(shape, False)
    return _call(vol, shape, in_place, lambda src, out, res: check(
        lib().hdf_morph(ptr(src), label, op, conn, n, bv, mode, *shape, ptr(out), ptr(res), ptr(ws), ws.numel(), st()),
        "hdf_morph"))


def _fill(vol, shape, conn, mode, label, in_place=False):
    ws = _workspace(shape, True)
    return _call(vol, shape, in_place, lambda src, out, res: check(
        lib().hdf_fill_holes(ptr(src), label, conn, mode, *shape, ptr(out), ptr(res), ptr(ws), ws.numel(), st()),
        "hdf_fill_holes"))


def _where(got, want):
    w = np.argwhere(got[0] != want[0])
    return len(w), w[:4].tolist(), got[1], want[1]


@pytest.mark.parametrize("index", range(len(mr.CASES)), ids=IDS)
def test_dilate_erode_open_close_every_byte(index):
    shape, kind = mr.CASES[index]
    vol_h = mr.case(shape, kind)
    vol = _dev(vol_h)
    for conn, op, bv, n, mode, label in mr.morph_params(index):
        want = mr.morph(vol_h, label, op, conn, n, bv, mode)
        got = _morph(vol, shape, conn, op, bv, n, mode, label)
        assert mr.mismatches(got, want) == [], (conn, op, bv, n, mode, label, _where(got, want))
        again = _morph(vol, shape, conn, op, bv, n, mode, label)
        assert mr.mismatches(again, got) == [], (conn, op, bv, n, mode, label)
    # in place: out is volume
    for op in mr.OPS:
        conn, bv, n = mr.CONNECTIVITIES[(index + op) % 3], (index + op) % 2, 1 + (index + op) % 3
        mode, label = mr.MODE_LABEL[(index + op) % 3]
        want = mr.morph(vol_h, label, op, conn, n, bv, mode)
        got = _morph(vol, shape, conn, op, bv, n, mode, label, in_place=True)
        assert mr.mismatches(got, want) == [], ("in place", conn, op, bv, n, mode, label, _where(got, want))
    assert np.array_equal(vol.cpu().numpy(), vol_h), "the input was written to"


@pytest.mark.parametrize("index", range(len(mr.CASES)), ids=IDS)
def test_fill_holes_every_byte(index):
    shape, kind = mr.CASES[index]
    vol_h = mr.case(shape, kind)
    vol = _dev(vol_h)
    for k, (conn, mode, label) in enumerate(mr.FILL_PARAMS):
        want = mr.fill_holes(vol_h, label, conn, mode)
        got = _fill(vol, shape, conn, mode, label)
        assert mr.mismatches(got, want) == [], (conn, mode, label, _where(got, want))
        again = _fill(vol, shape, conn, mode, label, in_place=k % 3 == index % 3)
        assert mr.mismatches(again, got) == [], (conn, mode, label)
    assert np.array_equal(vol.cpu().numpy(), vol_h), "the input was written to"


def test_refused_arguments_launch_nothing_on_the_device():
    shape = (4, 5, 6)
    need, fill_need = lib().hdf_morph_workspace_bytes(*shape), lib().hdf_fill_holes_workspace_bytes(*shape)
    vol = torch.full((256,), 2, dtype=torch.uint8, device=DEV)
    out = torch.full((256,), MARK, dtype=torch.uint8, device=DEV)
    res = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.full((fill_need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    listed = mr.refusals(ptr(vol), ptr(out), ptr(res), ptr(ws), need, fill_need, shape)
    assert len(listed) >= 40
    for what, entry, args in listed:
        rc = getattr(lib(), entry)(*(args[:-1] + (st(),)))
        assert rc == 1 and lib().hdf_last_error().startswith(b"morphology:"), (what, entry, rc, lib().hdf_last_error())
    torch.cuda.synchronize()
    assert (vol.cpu() == 2).all() and (out.cpu() == MARK).all() and res.cpu().tolist() == [-7, -7]
    assert (ws.cpu() == 0x5A).all()
    from hdf_rt import HdfError, binary_dilation, fill_class_holes, morph_class
    with pytest.raises(HdfError):
        binary_dilation(torch.zeros((1, 4, 1025), dtype=torch.uint8, device=DEV))
    with pytest.raises(HdfError):
        binary_dilation(vol[:120].view(shape), iterations=0)
    with pytest.raises(HdfError):
        fill_class_holes(vol[:120].view(shape), 0)
    with pytest.raises(ValueError):
        morph_class(vol[:120].view(shape), 2, "dilation")


# ------------------------------------------------------------------------------------------------------ Python surface
SURFACE = (19, 67, 131)
FUNCTIONS = {"binary_dilation": mr.DILATE, "binary_erosion": mr.ERODE, "binary_opening": mr.OPEN, "binary_closing": mr.CLOSE}


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_binary_op_wrapper(name):
    import hdf_rt
    fn, op = getattr(hdf_rt, name), FUNCTIONS[name]
    vol_h = mr.case(SURFACE, "rand50")
    vol = _dev(vol_h)
    got = fn(vol)                                            # scipy's defaults: connectivity 6, one iteration, border 0
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == SURFACE
    assert np.array_equal(got.cpu().numpy(), mr.morph(vol_h, 0, op, 6, 1, 0, mr.MASK)[0])
    want = mr.morph(vol_h, 0, op, 18, 3, 1, mr.MASK)
    got, counts = fn(vol_h, connectivity=18, iterations=3, border_value=1, return_counts=True)      # a numpy input
    assert counts.is_cuda and counts.dtype == torch.int64 and mr.mismatches((got.cpu().numpy(), counts.cpu().tolist()), want) == []
    assert np.array_equal(fn(vol_h != 0, 18, 3, border_value=1).cpu().numpy(), want[0])              # bool
    assert np.array_equal(fn(vol == 2, 26, 2).cpu().numpy(), mr.morph((vol_h == 2).astype(np.uint8), 0, op, 26, 2, 0, mr.MASK)[0])
    assert np.array_equal(fn(vol, 26, 2, label=2).cpu().numpy(), mr.morph(vol_h, 2, op, 26, 2, 0, mr.MASK)[0])
    flat = mr.case((1, 37, 70), "rand50")                    # [H, W] is [1, H, W]
    g2 = fn(flat[0], 18, 2)
    assert tuple(g2.shape) == (37, 70) and np.array_equal(g2.cpu().numpy(), mr.morph(flat, 0, op, 18, 2, 0, mr.MASK)[0][0])
    buf = vol.clone()
    assert fn(buf, out=buf).data_ptr() == buf.data_ptr()
    assert np.array_equal(buf.cpu().numpy(), mr.morph(vol_h, 0, op, 6, 1, 0, mr.MASK)[0])


def test_binary_fill_holes_wrapper():
    from hdf_rt import binary_fill_holes
    for kind in ("nested", "rand80"):
        vol_h = mr.case(SURFACE, kind)
        vol = _dev(vol_h)
        got, counts = binary_fill_holes(vol, return_counts=True)
        want = mr.fill_holes(vol_h, 0, 6, mr.MASK)
        assert want[1][1] > 0 and mr.mismatches((got.cpu().numpy(), counts.cpu().tolist()), want) == []
        assert np.array_equal(binary_fill_holes(vol_h != 0, 26).cpu().numpy(), mr.fill_holes(vol_h, 0, 26, mr.MASK)[0])
        assert np.array_equal(binary_fill_holes(vol_h, 18, label=2).cpu().numpy(), mr.fill_holes(vol_h, 2, 18, mr.MASK)[0])
    flat = mr.case((1, 37, 70), "box")
    g2 = binary_fill_holes(flat[0])
    assert tuple(g2.shape) == (37, 70) and np.array_equal(g2.cpu().numpy(), mr.fill_holes(flat, 0, 6, mr.MASK)[0][0])
    buf = vol.clone()
    assert binary_fill_holes(buf, out=buf).data_ptr() == buf.data_ptr()
    assert np.array_equal(buf.cpu().numpy(), mr.fill_holes(vol_h, 0, 6, mr.MASK)[0])


def test_morph_class_wrapper():
    from hdf_rt import morph_class
    vol_h = mr.case((40, 48, 56), "rand50")                  # three classes
    vol = _dev(vol_h)
    for name, op in (("dilate", mr.DILATE), ("erode", mr.ERODE), ("open", mr.OPEN), ("close", mr.CLOSE)):
        want = mr.morph(vol_h, 2, op, 18, 2, 0, mr.MAP)
        got, counts = morph_class(vol, 2, name, 18, 2, return_counts=True)
        assert mr.mismatches((got.cpu().numpy(), counts.cpu().tolist()), want) == [], name
        other = (vol_h != 0) & (vol_h != 2)
        assert np.array_equal(got.cpu().numpy()[other], vol_h[other])
    s_h = mr.case(SURFACE, "contact")
    assert np.array_equal(morph_class(s_h, 2, "dilate", 26, 3, border_value=1).cpu().numpy(),
                          mr.morph(s_h, 2, mr.DILATE, 26, 3, 1, mr.MAP)[0])


def test_fill_class_holes_wrapper_and_the_chain_to_a_score():
    """fill_class_holes -> keep_largest_component -> multi_dice without a copy to the host, against the same chain with
    scipy and cc_ref"""
    import cc_ref as cr
    from scipy import ndimage as ndi
    from hdf_rt import fill_class_holes, keep_largest_component, morphology, multi_dice, surface
    s_h = mr.case(SURFACE, "nested")
    got, counts = fill_class_holes(s_h, 2, return_counts=True)
    assert mr.mismatches((got.cpu().numpy(), counts.cpu().tolist()), mr.fill_holes(s_h, 2, 6, mr.MAP)) == []
    shape = (40, 48, 56)
    pred_h, tgt_h = mr.case(shape, "rand80"), mr.case(shape, "rand50")
    pred = _dev(pred_h)
    filled = fill_class_holes(pred, 2)
    kept = keep_largest_component(filled)
    assert kept.is_cuda and kept.dtype == torch.uint8
    hole = ndi.binary_fill_holes(pred_h == 2, ndi.generate_binary_structure(3, 1)) & (pred_h == 0)
    assert hole.any()
    ref_filled = np.where(hole, 2, pred_h).astype(np.uint8)
    assert np.array_equal(filled.cpu().numpy(), ref_filled)
    ref_kept = cr.full(ref_filled, 26, 0)["filters"][(0, 1)][0]
    assert np.array_equal(kept.cpu().numpy(), ref_kept)
    a, b = multi_dice(tgt_h, kept, 3), multi_dice(tgt_h, ref_kept, 3)
    assert a == b and not np.isnan(a[1])
    assert sum(1 for key in morphology._workspaces if key[0].startswith("hdf_fill") and key[-3:] == shape) == 1
    surface.clear_workspaces()
    assert not morphology._workspaces
