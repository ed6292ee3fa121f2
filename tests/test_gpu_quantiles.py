"""Per-region order statistics on the device (csrc/quantiles.hip, hdf_rt.regions) against the numpy restatement
tests/quantile_ref.py, itself held to np.sort, live np.quantile, scipy.ndimage.median, a plain loop on ties and seven
planted defects by tests/test_quantile_ref_cpu.py.

The comparison is quantile_ref.mismatches: every output byte.  The device selects exact order statistics with integer
counts and forms the interpolant with the three fp64 roundings of the definition, so there is nothing to allow for.

Shapes, id maps and images are measure_ref's: (1,1,1); (1,37,70), the 2-D case; (19,67,131), odd on every axis, 166 763 voxels
-- as ONE component (`full`) a single workgroup walks it in 652 trips, the last one ragged, and a counter passes 65 535 (a
constant image puts all 166 763 voxels into one counter in each of the four rounds); (5,3,300), a box row longer than the
256 lanes of a workgroup; 1024 on the first and on the last axis.  Id maps: random fills, empty, full and serpentine
labelled under 26 neighbours, the checkerboard under 6 (every voxel its own component: n = 1, and on the large shape 83 382
of them, more than the largest capacity), a numbering with gaps and negative ids, a three-class map, components of 1 and 3
voxels of which one is spread over a box far larger than itself; by hand, components of 1 and of 2 voxels and a diagonal.
Levels: the median alone (Q = 1) and quantile_ref.LEVELS16 (Q = 16: 0, 1, duplicates, unsorted, 1/3, 0.95).

Every call is made twice, into outputs filled with 0x5A that carry guard tails and a workspace that was filled with 0x5A
once and is never cleared; every output byte of the two must agree.  Nothing here measures time."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import measure_ref as mr  # noqa: E402
import quantile_ref as qr  # noqa: E402
from hdf_rt._lib import lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 512                                                      # bytes behind every output
MAX_CAP = 65536
SHAPES = [(1, 1, 1), (1, 37, 70), (19, 67, 131), (5, 3, 300), (1024, 3, 5), (3, 5, 1024)]
IDS_KEYS = [("label", "rand20", 26), ("label", "rand80", 26), ("label", "empty", 26), ("label", "full", 26),
            ("label", "checker", 6), ("label", "serpentine", 26), ("special", "gaps"), ("special", "classes"), ("special", "tiny")]
MEDIAN = (0.5,)
_ws = {}


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the shared inputs are read-only)


def _workspace(C_, cap, Q):
    n = lib().hdf_cc_quantiles_workspace_bytes(C_, cap, Q)
    assert n > 0
    if cap not in _ws:                                           # (the size depends on the capacity alone)
        _ws[cap] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    assert _ws[cap].numel() == n
    return _ws[cap]


def _levels(q):
    return (C.c_double * len(q))(*q)


class Buffers:
    """the outputs of a call, every byte 0x5A, with a guard tail each"""

    def __init__(self, C_, cap, Q):
        self.C, self.cap, self.Q = C_, cap, Q
        self.sizes = dict(count=cap * 8, values=C_ * cap * Q * 24, res=32)
        self.buf = {k: torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device=DEV) for k, n in self.sizes.items()}

    def call(self, ids, img, dims, q):
        ws = _workspace(self.C, self.cap, self.Q)
        rc = lib().hdf_cc_quantiles(ptr(ids), ptr(img), self.C, *dims, self.cap, _levels(q), self.Q, ptr(self.buf["count"]),
                                    ptr(self.buf["values"]), ptr(self.buf["res"]), ptr(ws), ws.numel(), st())
        assert rc == 0, lib().hdf_last_error()

    def untouched(self):
        return all(bool((b == 0x5A).all()) for b in self.buf.values())

    def outputs(self):
        host = {k: b.cpu().numpy() for k, b in self.buf.items()}
        for k, n in self.sizes.items():
            assert (host[k][n:] == 0x5A).all(), "write past the end of " + k
        return dict(count=host["count"][:self.sizes["count"]].view(np.int64).copy(),
                    values=host["values"][:self.sizes["values"]].view(np.float64).reshape(self.C, self.cap, self.Q, 3).copy(),
                    result=host["res"][:32].view(np.int64).tolist())


def _run(ids_dev, img_dev, dims, C_, cap, q):
    """two calls into fresh 0x5A outputs and the same workspace: the first call's outputs, after both were compared byte for
    byte"""
    a, b = Buffers(C_, cap, len(q)), Buffers(C_, cap, len(q))
    a.call(ids_dev, img_dev, dims, q)
    b.call(ids_dev, img_dev, dims, q)
    out, again = a.outputs(), b.outputs()
    for k in ("count", "values"):
        assert out[k].tobytes() == again[k].tobytes(), ("two calls differ", k)
    assert out["result"] == again["result"]
    return out


def _ids_of(shape, key):
    return mr.labelled(shape, key[1], key[2]) if key[0] == "label" else mr.special_ids(shape, key[1])


def _check(shape, ids, kind, C_, cap, q, ids_dev):
    img = mr.image(kind, shape, C_)
    want = qr.quantiles(ids, img, q, cap)
    got = _run(ids_dev, _dev(img), shape, C_, cap, q)
    assert qr.mismatches(got, want) == [], (shape, kind, C_, cap, len(q))
    return got


@pytest.mark.parametrize("key", IDS_KEYS, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_restatement(shape, key):
    ids, top = _ids_of(shape, key)
    cap = min(top + 3, MAX_CAP)
    ids_dev = _dev(ids)
    at = IDS_KEYS.index(key)
    # every image on the large shape under four of the id maps; elsewhere the constant one (all four rounds put everything
    # into one counter) and two more
    every = shape == mr.BIG and key[1] in ("rand20", "full", "gaps", "tiny")
    kinds = mr.IMAGES if every else ["constant", mr.IMAGES[at % 6], mr.IMAGES[(at + 3) % 6]]
    for kind in kinds:
        _check(shape, ids, kind, 3, cap, qr.LEVELS16, ids_dev)
    _check(shape, ids, mr.IMAGES[(at + 1) % 6], 1, cap, MEDIAN, ids_dev)
    if top >= 2:                                                 # a capacity below the largest id: the rest is left out
        low = max(top // 2, 1)
        got = _check(shape, ids, "signed", 3, low, (0.1, 0.5, 0.9), ids_dev)
        assert got["result"][0] == top and got["result"][2] <= got["result"][1]
    assert np.array_equal(ids_dev.cpu().numpy(), ids), "the ids changed"


def test_a_counter_passes_65535():
    ids, n = mr.labelled(mr.BIG, "full", 26)
    assert n == 1 and int((ids == 1).sum()) == 166763 > 65535
    for kind in ("constant", "levels"):
        got = _check(mr.BIG, ids, kind, 2, 1, qr.LEVELS16, _dev(ids))
        assert got["count"].tolist() == [166763]


def test_components_of_one_and_two_voxels_and_a_thin_one_in_a_large_box():
    shape = (19, 67, 131)
    ids = np.zeros(shape, np.int32)
    ids[3, 4, 5] = 1                                             # one voxel
    ids[7, 8, 9] = ids[7, 8, 10] = 2                             # two, side by side
    ids[0, 0, 0] = ids[18, 66, 130] = 4                          # two, at opposite corners: the box is the volume
    for k in range(19):                                          # a diagonal: 19 voxels in a box of 19 x 55 x 109
        ids[k, 3 * k, 6 * k + 2] = 6
    ids_dev = _dev(ids)
    for kind in ("signed", "zeros_denormals", "constant"):
        got = _check(shape, ids, kind, 3, 8, qr.LEVELS16, ids_dev)
        assert got["count"].tolist() == [1, 2, 0, 2, 0, 19, 0, 0]
    got = _check(shape, ids, "signed", 1, 8, MEDIAN, ids_dev)
    a, b = sorted(float(x) for x in (mr.image("signed", shape, 1)[0, 7, 8, 9], mr.image("signed", shape, 1)[0, 7, 8, 10]))
    assert got["values"][0, 1, 0].tolist() == [a, b, a + 0.5 * (b - a)]   # the median of two: their mean, as the definition rounds it


def test_every_level_of_sixteen_is_the_row_of_a_call_with_that_level_alone():
    shape = mr.BIG
    ids, n = mr.labelled(shape, "rand20", 26)
    ids_dev, img = _dev(ids), _dev(mr.image("signed", shape, 2))
    all16 = _run(ids_dev, img, shape, 2, n, qr.LEVELS16)
    assert qr.mismatches(all16, qr.quantiles(ids, mr.image("signed", shape, 2), qr.LEVELS16, n)) == []
    for k, q in enumerate(qr.LEVELS16):
        one = _run(ids_dev, img, shape, 2, n, (q,))
        assert one["values"][:, :, 0].tobytes() == np.ascontiguousarray(all16["values"][:, :, k]).tobytes(), (k, q)
        assert one["count"].tobytes() == all16["count"].tobytes()


def test_more_components_than_the_largest_capacity():
    ids, n = mr.labelled(mr.BIG, "checker", 6)
    assert n == 83382 > MAX_CAP
    got = _check(mr.BIG, ids, "signed", 2, MAX_CAP, (0.25, 0.5, 1.0), _dev(ids))
    assert got["result"] == [n, n, MAX_CAP, 0] and (got["count"] == 1).all()


def test_a_row_does_not_depend_on_the_capacity_or_on_the_workspace():
    shape = mr.BIG
    ids, n = mr.labelled(shape, "rand20", 26)
    assert n >= 50
    ids_dev, img = _dev(ids), _dev(mr.image("signed", shape, 2))
    q = (0.1, 0.5, 0.9)
    base = _run(ids_dev, img, shape, 2, n, q)
    for cap in (n + 3, 4096, n - 7):
        got = _run(ids_dev, img, shape, 2, cap, q)
        rows = min(n, cap)
        assert got["count"][:rows].tobytes() == base["count"][:rows].tobytes(), cap
        assert np.ascontiguousarray(got["values"][:, :rows]).tobytes() == np.ascontiguousarray(base["values"][:, :rows]).tobytes(), cap
    _run(_dev(mr.labelled(shape, "full", 26)[0]), _dev(mr.image("uniform", shape, 2)), shape, 2, n, q)   # other boxes, same places
    _workspace(2, n + 3, 3).fill_(0xFF)
    for cap in (n, n + 3):
        got = _run(ids_dev, img, shape, 2, cap, q)
        assert np.ascontiguousarray(got["values"][:, :n]).tobytes() == base["values"].tobytes(), cap


def _measure(ids_dev, img_dev, dims, C_, cap):
    n = lib().hdf_cc_measure_workspace_bytes(C_, cap)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    geom = torch.empty((cap, 4), dtype=torch.int64, device=DEV)
    stats = torch.empty((C_, cap, 8), dtype=torch.float64, device=DEV)
    pos = torch.empty((C_, cap, 2), dtype=torch.int64, device=DEV)
    res = torch.empty(4, dtype=torch.int64, device=DEV)
    rc = lib().hdf_cc_measure(ptr(ids_dev), ptr(img_dev), C_, *dims, cap, ptr(geom), ptr(stats), ptr(pos), ptr(res), ptr(ws), n, st())
    assert rc == 0, lib().hdf_last_error()
    return geom.cpu().numpy(), stats.cpu().numpy(), res.cpu().tolist()


@pytest.mark.parametrize("kind", ["signed", "zeros_denormals", "levels"])
def test_the_ends_are_the_min_and_max_of_hdf_cc_measure(kind):
    shape = mr.BIG
    ids, n = mr.labelled(shape, "rand20", 26)
    ids_dev, img = _dev(ids), _dev(mr.image(kind, shape, 2))
    got = _run(ids_dev, img, shape, 2, n + 3, (0.0, 1.0))
    geom, stats, res = _measure(ids_dev, img, shape, 2, n + 3)
    assert got["result"] == res and got["count"].tobytes() == np.ascontiguousarray(geom[:, 0]).tobytes()
    for j in range(3):
        assert np.ascontiguousarray(got["values"][:, :, 0, j]).tobytes() == np.ascontiguousarray(stats[..., 3]).tobytes(), ("min", j)
        assert np.ascontiguousarray(got["values"][:, :, 1, j]).tobytes() == np.ascontiguousarray(stats[..., 4]).tobytes(), ("max", j)


def test_nan_and_infinity_stay_in_their_component():
    """a NaN or an infinity is the caller's error: that component's values are unspecified, every other row is what it was,
    the counts are exact"""
    shape = (5, 17, 33)
    ids, top = mr.special_ids(shape, "classes")
    img = np.array(mr.image("signed", shape, 2))
    clean = _run(_dev(ids), _dev(img), shape, 2, top, qr.LEVELS16)
    where = np.flatnonzero(ids.ravel() == 2)
    img.reshape(2, -1)[0, where[3]] = np.nan
    img.reshape(2, -1)[1, where[5]] = np.inf
    img.reshape(2, -1)[1, where[9]] = -np.inf
    got = _run(_dev(ids), _dev(img), shape, 2, top, qr.LEVELS16)
    assert got["result"] == clean["result"] and got["count"].tobytes() == clean["count"].tobytes()
    for r in (0, 2):
        assert np.ascontiguousarray(got["values"][:, r]).tobytes() == np.ascontiguousarray(clean["values"][:, r]).tobytes()
    k0, k1 = qr.LEVELS16.index(0.0), qr.LEVELS16.index(1.0)
    assert got["values"][1, 1, k0, 0] == -np.inf and got["values"][1, 1, k1, 1] == np.inf   # (keys like any other)


def test_the_python_surface():
    import hdf_rt
    from hdf_rt import region_median, region_order_stats, region_quantiles
    shape = (19, 67, 131)
    ids, n = mr.labelled(shape, "rand20", 26)
    img = mr.image("signed", shape, 2)
    q = (0.1, 0.5, 0.9)
    want = qr.quantiles(ids, img, q, n + 3)
    count, values, res = region_quantiles(_dev(ids), _dev(img), q, capacity=n + 3)
    assert count.is_cuda and values.dtype == torch.float64 and tuple(values.shape) == (2, n + 3, 3, 3) and tuple(count.shape) == (n + 3,)
    raw = dict(count=count.cpu().numpy(), values=values.cpu().numpy(), result=res.cpu().tolist())
    assert qr.mismatches(raw, want) == []
    got = region_order_stats(_dev(ids), _dev(img), q, capacity=n + 3)
    assert [d["id"] for d in got] == list(range(1, n + 1))
    for d in got:
        r = d["id"] - 1
        assert d["size"] == int(want["count"][r]) and len(d["channels"]) == 2
        for c, ch in enumerate(d["channels"]):
            assert list(ch) == ["quantiles", "lower", "upper"]
            assert ch["quantiles"] == want["values"][c, r, :, 2].tolist()
            assert ch["lower"] == want["values"][c, r, :, 0].tolist() and ch["upper"] == want["values"][c, r, :, 1].tolist()
    med = region_median(_dev(ids), _dev(img), capacity=n + 3)
    assert med.is_cuda and med.dtype == torch.float64 and tuple(med.shape) == (2, n + 3)
    assert med.cpu().numpy().tobytes() == np.ascontiguousarray(want["values"][:, :, 1, 2]).tobytes()
    # the defaults: the median; one channel; [H, W]; an integer map of another width
    ids2, _ = mr.special_ids((1, 37, 70), "gaps")
    img2 = mr.image("uniform", (1, 37, 70), 1)
    c2, v2, r2 = region_quantiles(_dev(ids2[0].astype(np.int64)), _dev(img2[0, 0]))
    want2 = qr.quantiles(ids2, img2, (0.5,), 4096)
    assert qr.mismatches(dict(count=c2.cpu().numpy(), values=v2.cpu().numpy(), result=r2.cpu().tolist()), want2) == []
    got2 = region_order_stats(_dev(ids2[0]), _dev(img2[0, 0]))
    assert [d["id"] for d in got2] == [3, 4, 9, 40] and len(got2[0]["channels"][0]["quantiles"]) == 3
    # what is refused
    with pytest.raises(hdf_rt.HdfError, match="capacity"):
        region_order_stats(_dev(ids), _dev(img), q, capacity=n - 1)
    with pytest.raises(hdf_rt.HdfError, match="components: quantiles:"):
        region_quantiles(_dev(ids), _dev(img), q, capacity=0)
    with pytest.raises(hdf_rt.HdfError, match="components: quantiles:"):
        region_quantiles(_dev(ids), _dev(img), (0.5, 1.5))
    with pytest.raises(hdf_rt.HdfError, match="components: quantiles:"):
        region_quantiles(_dev(ids), _dev(img), ())
    for fn in (region_quantiles, region_order_stats, region_median):
        with pytest.raises(ValueError):                          # tensors on the CPU
            fn(torch.from_numpy(np.array(ids)), _dev(img))
        with pytest.raises(ValueError):
            fn(_dev(ids), torch.from_numpy(np.array(img)))
        with pytest.raises(ValueError):                          # wrong dtypes
            fn(_dev(ids).float(), _dev(img))
        with pytest.raises(ValueError):
            fn(_dev(ids), _dev(img).to(torch.int32))
        with pytest.raises(ValueError):                          # wrong shapes
            fn(_dev(ids), _dev(img[:, :5]))
        with pytest.raises(ValueError):
            fn(_dev(ids).reshape(-1), _dev(img))


def test_refusals():
    """every one returns HDF_ERR_ARG = 1 with a "components: quantiles:" message, before anything is launched: the outputs
    keep their marker"""
    shape, Cn, cap, Q = (3, 5, 7), 2, 10, 3
    V = 105
    ids = _dev(mr.special_ids(shape, "classes")[0])
    img = _dev(mr.image("uniform", shape, Cn))
    buf = Buffers(Cn, cap, Q)
    ws = _workspace(Cn, cap, Q)
    need = lib().hdf_cc_quantiles_workspace_bytes(Cn, cap, Q)
    assert need == ws.numel()
    good = dict(ids=ptr(ids), image=ptr(img), C=Cn, D=3, H=5, W=7, cap=cap, q=_levels((0.1, 0.5, 0.9)), Q=Q,
                count=ptr(buf.buf["count"]), values=ptr(buf.buf["values"]), res=ptr(buf.buf["res"]), ws=ptr(ws), ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib().hdf_cc_quantiles(a["ids"], a["image"], a["C"], a["D"], a["H"], a["W"], a["cap"], a["q"], a["Q"], a["count"],
                                    a["values"], a["res"], a["ws"], a["ws_bytes"], st())
        return rc, lib().hdf_last_error().decode()

    bad = [dict(C=0), dict(C=9), dict(D=0), dict(H=1025), dict(W=-1), dict(cap=0), dict(cap=65537), dict(ids=None),
           dict(image=None), dict(count=None), dict(values=None), dict(res=None), dict(ws=None), dict(ws_bytes=need - 1),
           dict(ws=ptr(ws) + 4, ws_bytes=need + 8), dict(count=good["count"] + 4), dict(values=good["values"] + 4),
           dict(res=good["res"] + 4), dict(Q=0), dict(Q=17), dict(q=None), dict(q=_levels((0.1, float("nan"), 0.9))),
           dict(q=_levels((0.1, 0.5, 1.0000001))), dict(q=_levels((-0.25, 0.5, 0.9)))]
    sizes = dict(count=cap * 8, values=Cn * cap * Q * 24, res=32, ws=need)
    for name, nbytes in sizes.items():
        bad += [{name: ptr(ids)}, {name: ptr(ids) + 4 * V - 8}, {name: ptr(img) + 4 * V}, {name: ptr(img) + 8 * V - 8}]
        for other, obytes in sizes.items():
            if other != name:
                bad += [{name: good[other] + obytes - 8}, {name: good[other] - nbytes + 8}]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("components: quantiles:"), (kw, rc, msg)
    assert lib().hdf_cc_quantiles_workspace_bytes(9, 10, 1) == -1 and lib().hdf_cc_quantiles_workspace_bytes(1, 0, 1) == -1
    assert lib().hdf_cc_quantiles_workspace_bytes(1, 10, 17) == -1
    torch.cuda.synchronize()
    assert buf.untouched()
    rc, msg = call()
    assert rc == 0, msg
