"""Region measurements on the device (csrc/measure.hip, hdf_rt.regions) against the numpy / fsum restatement
tests/measure_ref.py, itself held to live scipy.ndimage, a plain loop and seven planted defects by
tests/test_measure_ref_cpu.py.

The comparison is measure_ref.mismatches: n, the coordinate sums, min, max (as bits), pos and result exactly, the fp64 sums
to bounds derived in measure_ref's docstring from u = 2^-53 and the component's size -- never from what the device gives.
Where the image holds small integers every sum is exact and must equal fsum in every bit.

Shapes (measure_ref.SHAPES): (1,1,1); (1,37,70), the 2-D case; (19,67,131), odd on every axis, whose full-volume component
gives each of the eight slabs 82 trips of a workgroup and a ragged last slab; (5,3,300), a row longer than 256 lanes; 1024 on
each axis in turn.  No grid of measure.hip is capped (the walk has one workgroup per 8192 voxels, the slab passes one per
(id, slab, channel), the finishing kernels one thread per row), so there is no case past a cap.
Id maps: cc_ref's random fills, empty, full, checkerboard and serpentine labelled on the host under 26 neighbours, the
checkerboard also under 6 (every voxel its own component: 83 382 of them on the large shape, more than the largest
capacity); a numbering with gaps and negative ids; a three-class map; components of 1 and 3 voxels, fewer than slabs, one
of them spread over a box far larger than itself.  capacity = the largest id + 3, and once below it.
Images: measure_ref.IMAGES with C = 3, and one of them per id map with C = 1.

Every call is made twice into the same workspace, which is filled with 0x5A once and never cleared; every output byte of
the two must agree.  Outputs are pre-filled with a marker and carry guard tails.  Nothing here measures time."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import measure_ref as mr  # noqa: E402
from hdf_rt._lib import lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
MAX_CAP = 65536
_ws = {}

IDS_KEYS = [("label", m, 26) for m in mr.MASKS] + [("label", "checker", 6), ("special", "gaps"), ("special", "classes"),
                                                     ("special", "tiny")]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the shared inputs are read-only)


def _workspace(C, cap):
    if (C, cap) not in _ws:
        n = lib().hdf_cc_measure_workspace_bytes(C, cap)
        assert n > 0
        _ws[C, cap] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    return _ws[C, cap]


class Buffers:
    """the outputs of a call, pre-filled with a marker, with a guard tail each"""

    def __init__(self, C, cap, marker):
        self.C, self.cap, self.marker = C, cap, marker
        self.geom = torch.full((cap * 4 + GUARD,), marker, dtype=torch.int64, device=DEV)
        self.stats = torch.full((C * cap * 8 + GUARD,), float(marker), dtype=torch.float64, device=DEV)
        self.pos = torch.full((C * cap * 2 + GUARD,), marker, dtype=torch.int64, device=DEV)
        self.res = torch.full((4 + GUARD,), marker, dtype=torch.int64, device=DEV)

    def tensors(self):
        return self.geom, self.stats, self.pos, self.res

    def call(self, ids, img, dims):
        ws = _workspace(self.C, self.cap)
        rc = lib().hdf_cc_measure(ptr(ids), ptr(img), self.C, *dims, self.cap, ptr(self.geom), ptr(self.stats), ptr(self.pos),
                                  ptr(self.res), ptr(ws), ws.numel(), st())
        assert rc == 0, lib().hdf_last_error()

    def outputs(self):
        geom, stats, pos, res = (t.cpu().numpy() for t in self.tensors())
        C, cap, m = self.C, self.cap, self.marker
        assert (geom[cap * 4:] == m).all() and (stats[C * cap * 8:] == m).all(), "write past the end of geom or stats"
        assert (pos[C * cap * 2:] == m).all() and (res[4:] == m).all(), "write past the end of pos or result"
        return dict(geom=geom[:cap * 4].reshape(cap, 4), stats=stats[:C * cap * 8].reshape(C, cap, 8),
                    pos=pos[:C * cap * 2].reshape(C, cap, 2), result=res[:4].tolist())


def _run(ids_dev, img_dev, dims, C, cap):
    """two calls with different markers into the same workspace: the first call's outputs, after both were compared byte
    for byte"""
    a, b = Buffers(C, cap, -5), Buffers(C, cap, -9)
    a.call(ids_dev, img_dev, dims)
    b.call(ids_dev, img_dev, dims)
    out, again = a.outputs(), b.outputs()
    for k in ("geom", "stats", "pos"):
        assert out[k].tobytes() == again[k].tobytes(), ("two calls differ", k)
    assert out["result"] == again["result"]
    return out


def _ids_of(shape, key):
    return mr.labelled(shape, key[1], key[2]) if key[0] == "label" else mr.special_ids(shape, key[1])


def _check(shape, key, kind, C, cap, ids_dev):
    want = mr.reference(shape, key, kind, C, cap)
    got = _run(ids_dev, _dev(mr.image(kind, shape, C)), shape, C, cap)
    print("%s %s %s C=%d capacity=%d: worst error / bound %.3g" % (shape, key, kind, C, cap, mr.worst(got, want)))
    assert mr.mismatches(got, want) == [], (shape, key, kind, C, cap)
    if kind == "ints":                                           # every term and every partial sum is an integer below 2^53
        for k in (0, 1, 5, 6, 7):
            assert got["stats"][..., k].tobytes() == want["stats"][..., k].tobytes(), (mr.STAT_COLS[k], "not exact")
    return got


@pytest.mark.parametrize("key", IDS_KEYS, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("shape", mr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_restatement(shape, key):
    ids, top = _ids_of(shape, key)
    cap = min(top + 3, MAX_CAP)
    ids_dev = _dev(ids)
    for kind in mr.IMAGES:
        _check(shape, key, kind, 3, cap, ids_dev)
    one = mr.IMAGES[IDS_KEYS.index(key) % len(mr.IMAGES)]
    _check(shape, key, one, 1, cap, ids_dev)
    if top >= 2:                                                 # a capacity below the largest id: the rest is left out
        low = max(top // 2, 1)
        got = _check(shape, key, "signed", 3, low, ids_dev)
        assert got["result"][0] == top and got["result"][2] <= got["result"][1]
    assert np.array_equal(ids_dev.cpu().numpy(), ids), "the ids changed"


def test_more_components_than_the_largest_capacity():
    ids, n = mr.labelled(mr.BIG, "checker", 6)
    assert n == 83382 > MAX_CAP
    got = _check(mr.BIG, ("label", "checker", 6), "signed", 2, MAX_CAP, _dev(ids))
    assert got["result"] == [n, n, MAX_CAP, 0] and (got["geom"][:, 0] == 1).all()


def test_a_row_does_not_depend_on_the_capacity_or_on_the_workspace():
    """the same rows, bit for bit, at three capacities (their partial sums lie at different places of differently sized
    workspaces), after another call has left its own sums in the workspace, and with the workspace filled with ones"""
    shape = mr.BIG
    ids, n = mr.labelled(shape, "rand20", 26)
    assert n >= 50
    ids_dev, img = _dev(ids), _dev(mr.image("signed", shape, 2))
    base = _run(ids_dev, img, shape, 2, n)
    for cap in (n + 3, 4096, n - 7):
        got = _run(ids_dev, img, shape, 2, cap)
        rows = min(n, cap)
        for k in ("geom", "stats", "pos"):
            assert got[k][..., :rows, :].tobytes() == base[k][..., :rows, :].tobytes(), (k, cap)
    _run(_dev(mr.labelled(shape, "full", 26)[0]), _dev(mr.image("uniform", shape, 2)), shape, 2, n)   # other sums, same places
    _workspace(2, n + 3).fill_(0xFF)
    for cap in (n, n + 3):
        got = _run(ids_dev, img, shape, 2, cap)
        for k in ("geom", "stats", "pos"):
            assert got[k][..., :n, :].tobytes() == base[k].tobytes(), (k, cap)


def test_nan_and_infinity_stay_in_their_component():
    """a NaN or an infinity is the caller's error: that component's fp64 outputs are unspecified, every other row is what
    it was, the integers are exact"""
    shape = (5, 17, 33)
    ids, top = mr.special_ids(shape, "classes")
    img = np.array(mr.image("signed", shape, 2))
    clean = _run(_dev(ids), _dev(img), shape, 2, top)
    where = np.flatnonzero(ids.ravel() == 2)
    img.reshape(2, -1)[0, where[3]] = np.nan
    img.reshape(2, -1)[1, where[5]] = np.inf
    img.reshape(2, -1)[1, where[9]] = -np.inf
    got = _run(_dev(ids), _dev(img), shape, 2, top)
    assert got["result"] == clean["result"] and got["geom"].tobytes() == clean["geom"].tobytes()
    for r in (0, 2):
        assert got["stats"][:, r].tobytes() == clean["stats"][:, r].tobytes() and np.array_equal(got["pos"][:, r], clean["pos"][:, r])
    assert got["stats"][1, 1, 3] == -np.inf and got["stats"][1, 1, 4] == np.inf      # (the extrema of the infinities are exact)
    assert got["pos"][1, 1].tolist() == [where[9], where[5]]


def _close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= tol


def test_region_stats_and_pet_measures(monkeypatch):
    import hdf_rt
    from hdf_rt import pet_lesion_measures, region_measure, region_stats
    shape, spacing = (19, 67, 131), (3.0, 0.9765625, 1.25)
    ids, n = mr.labelled(shape, "rand20", 26)
    img = mr.image("ints", shape, 2)
    want = mr.measure(ids, img, n + 3)
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (copies.append(t.numel()), real(t, *a, **k))[1])
    got = region_stats(_dev(ids), _dev(img), capacity=n + 3, spacing=spacing)
    monkeypatch.undo()
    assert copies == [4 + (n + 3) * (4 + 2 * 8 + 2 * 2)], copies                     # one copy to the host
    ref = mr.dicts(want, shape, spacing)
    assert [d["id"] for d in got] == list(range(1, n + 1)) and len(ref) == n
    b = mr.bounds(want)
    for d, w in zip(got, ref):
        assert {k: d[k] for k in d if k != "channels"} == {k: w[k] for k in w if k != "channels"}
        for c, (ch, wc) in enumerate(zip(d["channels"], w["channels"])):
            assert list(ch) == list(wc)
            for k in ch:                                         # integer-valued sums are exact; M2 is within its bound
                if k in ("variance", "std"):
                    tol = b[c, d["id"] - 1, 2] / d["size"]
                    assert _close(ch["variance"], wc["variance"], tol)
                    # |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= tol / std, and one rounding of the root
                    assert _close(ch["std"], wc["std"], tol / wc["std"] + 2 * mr.U * wc["std"] if wc["std"] > 0 else math.sqrt(tol))
                elif k == "center_of_mass" or k == "center_of_mass_mm":
                    assert all(_close(a, e, 0.0) for a, e in zip(ch[k], wc[k])), (d["id"], k, ch[k], wc[k])
                else:
                    assert ch[k] == wc[k], (d["id"], c, k, ch[k], wc[k])
    # the device tensors; a numpy input, one channel, [H, W]; the defaults
    geom, stats, pos, res = region_measure(_dev(ids), _dev(img), capacity=n + 3)
    assert geom.is_cuda and stats.dtype == torch.float64 and tuple(stats.shape) == (2, n + 3, 8) and tuple(pos.shape) == (2, n + 3, 2)
    raw = dict(geom=geom.cpu().numpy(), stats=stats.cpu().numpy(), pos=pos.cpu().numpy(), result=res.cpu().tolist())
    assert mr.mismatches(raw, want) == []
    ids2, top2 = mr.special_ids((1, 37, 70), "gaps")
    img2 = mr.image("uniform", (1, 37, 70), 1)
    got2 = hdf_rt.region_stats(ids2[0].astype(np.int64), img2[0, 0])
    raw2 = _run(_dev(ids2), _dev(img2), (1, 37, 70), 1, 4096)
    assert mr.mismatches(raw2, mr.measure(ids2, img2, 4096)) == []
    assert got2 == mr.dicts(raw2, (1, 37, 70)) and [d["id"] for d in got2] == [3, 4, 9, 40]
    assert all(d["centroid"][0] == 0.0 and d["channels"][0]["argmax"][0] == 0 and "volume_mm3" not in d for d in got2)
    # PET: MTV in ml, SUVmax, SUVmean, TLG
    suv = mr.image("uniform", shape, 1)
    pet = pet_lesion_measures(_dev(ids), _dev(suv[0]), spacing, capacity=n + 3)
    wp = mr.measure(ids, suv, n + 3)
    bp = mr.bounds(wp)
    ml = spacing[0] * spacing[1] * spacing[2] / 1000.0
    assert len(pet) == n
    for d, r in zip(pet, range(n)):
        size, mean = int(wp["geom"][r, 0]), wp["stats"][0, r, 1]
        assert d["id"] == r + 1 and d["size"] == size and d["SUVmax"] == wp["stats"][0, r, 4]
        assert d["SUVpeak_at"] == tuple(int(v) for v in np.unravel_index(wp["pos"][0, r, 1], shape))
        assert abs(d["MTV"] - size * ml) <= 4 * mr.U * size * ml
        assert abs(d["SUVmean"] - mean) <= bp[0, r, 1]
        assert abs(d["TLG"] - mean * size * ml) <= (bp[0, r, 1] + 6 * mr.U * abs(mean)) * size * ml
    # more ids than the capacity; refused arguments
    with pytest.raises(hdf_rt.HdfError, match="capacity"):
        region_stats(_dev(ids), _dev(img), capacity=n - 1)
    with pytest.raises(hdf_rt.HdfError, match="components: measure:"):
        region_measure(_dev(ids), _dev(img), capacity=0)
    with pytest.raises(ValueError):
        region_measure(_dev(ids), _dev(img[:, :5]))
    with pytest.raises(ValueError):
        region_measure(_dev(ids).float(), _dev(img))
    with pytest.raises(ValueError):
        pet_lesion_measures(_dev(ids), _dev(img), spacing)


def test_refusals():
    """every one returns HDF_ERR_ARG = 1 with a "components: measure:" message, before anything is launched: the outputs
    keep their marker"""
    shape, Cn, cap = (3, 5, 7), 2, 10
    V = 105
    ids = _dev(mr.special_ids(shape, "classes")[0])
    img = _dev(mr.image("uniform", shape, Cn))
    buf = Buffers(Cn, cap, -5)
    ws = _workspace(Cn, cap)
    need = lib().hdf_cc_measure_workspace_bytes(Cn, cap)
    assert need == ws.numel()
    good = dict(ids=ptr(ids), image=ptr(img), C=Cn, D=3, H=5, W=7, cap=cap, geom=ptr(buf.geom), stats=ptr(buf.stats),
                pos=ptr(buf.pos), res=ptr(buf.res), ws=ptr(ws), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib().hdf_cc_measure(a["ids"], a["image"], a["C"], a["D"], a["H"], a["W"], a["cap"], a["geom"], a["stats"], a["pos"],
                                  a["res"], a["ws"], a["ws_bytes"], st())
        return rc, lib().hdf_last_error().decode()

    bad = [dict(C=0), dict(C=9), dict(D=0), dict(H=1025), dict(W=-1), dict(cap=0), dict(cap=65537), dict(ids=None),
           dict(image=None), dict(geom=None), dict(stats=None), dict(pos=None), dict(res=None), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws=ptr(ws) + 4, ws_bytes=need + 8), dict(geom=ptr(buf.geom) + 4),
           dict(stats=ptr(buf.stats) + 4), dict(pos=ptr(buf.pos) + 4), dict(res=ptr(buf.res) + 4)]
    sizes = dict(geom=cap * 32, stats=Cn * cap * 64, pos=Cn * cap * 16, res=32, ws=need)
    for name, nbytes in sizes.items():
        bad += [{name: ptr(ids)}, {name: ptr(ids) + 4 * V - 8}, {name: ptr(img) + 4 * V}, {name: ptr(img) + 8 * V - 8}]
        for other, obytes in sizes.items():
            if other != name:
                bad += [{name: good[other] + obytes - 8}, {name: good[other] - nbytes + 8}]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("components: measure:"), (kw, rc, msg)
    assert lib().hdf_cc_measure_workspace_bytes(9, 10) == -1 and lib().hdf_cc_measure_workspace_bytes(1, 0) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -5).all()) for t in buf.tensors())
    rc, msg = call()
    assert rc == 0, msg
