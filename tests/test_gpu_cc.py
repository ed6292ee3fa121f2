"""Connected components on the device (csrc/components.hip, hdf_rt/components.py) against the scipy restatement of the
definitions in include/hdf.h (tests/cc_ref.py, itself held to a flood fill by tests/test_cc_ref_cpu.py).

Shapes (cc_ref.SHAPES): (1,1,1); (1,37,70), the 2-D case; (19,67,131), odd and across a wave and a block on every axis;
(5,3,300), a row longer than 256 lanes; the cap of 1024 on each axis in turn; (40,48,56), whose random fills carry three
values.  Masks per shape (cc_ref.MASKS): random fills at 0.2 / 0.5 / 0.8, empty, full, the 3-D checkerboard (V/2
components under 6-connectivity: the widest prefix sum), one serpentine path through the volume (the longest union chains,
every late merge against index order), a comb joined in its last row, pairs touching across an edge or a corner only, the
end of a row beside the start of the next (and of a plane), two values in alternate planes, components of equal size.

Every comparison is exact (cc_ref.mismatches): each int32 of ids, both result words, each int64 of the table, each fp32
of score_max bit for bit, each byte of the eight filtered maps and their result words, for connectivity 6 / 18 / 26 and
label 0 / 2.  Outputs are pre-filled with a marker and carry a guard tail; the workspace of a shape is filled with 0x5A
once and then reused by every call on every mask without clearing; hdf_cc_label runs twice on every input and the two
id maps must agree.  Nothing here measures time: the largest volume has 166 763 voxels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cc_ref as cr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
CASES = [(s, k) for s in cr.SHAPES for k in cr.MASKS]
_ws = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(shape):
    if shape not in _ws:
        n = lib().hdf_cc_workspace_bytes(*shape)
        assert n > 0
        _ws[shape] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    return _ws[shape]


def _label(vol, shape, conn, lab, ws):
    v = int(np.prod(shape))
    ids = torch.full((v + GUARD,), -77, dtype=torch.int32, device=DEV)
    res = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    check(lib().hdf_cc_label(ptr(vol), lab, conn, *shape, ptr(ids), ptr(res), ptr(ws), ws.numel(), st()), "hdf_cc_label")
    host, r = ids.cpu().numpy(), res.cpu().tolist()
    assert (host[v:] == -77).all() and r[2] == -7, "write past the end of an output"
    return ids, host[:v].reshape(shape), r[:2]


def _table(vol, ids, score, shape, cap):
    table = torch.full((cap * 9 + GUARD,), -5, dtype=torch.int64, device=DEV)
    smax = torch.full((cap + GUARD,), -3.0, dtype=torch.float32, device=DEV)
    check(lib().hdf_cc_table(ptr(vol), ptr(ids), ptr(score), *shape, cap, ptr(table), ptr(smax), st()), "hdf_cc_table")
    t, s = table.cpu().numpy(), smax.cpu().numpy()
    assert (t[cap * 9:] == -5).all() and (s[cap:] == -3.0).all(), "write past the end of the table"
    return t[:cap * 9].reshape(cap, 9), s[:cap]


def _filter(vol, ids, shape, ms, kl, ws, in_place=False):
    v = int(np.prod(shape))
    out = torch.full((v + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
    if in_place:
        out[:v] = vol.reshape(-1)
    src = out if in_place else vol
    res = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    check(lib().hdf_cc_filter(ptr(src), ptr(ids), *shape, ms, kl, ptr(out), ptr(res), ptr(ws), ws.numel(), st()),
          "hdf_cc_filter")
    o, r = out.cpu().numpy(), res.cpu().tolist()
    assert (o[v:] == 0xEE).all() and r[2] == -7, "write past the end of an output"
    return o[:v].reshape(shape), r[:2]


@pytest.mark.parametrize("shape,kind", CASES, ids=["%s-%s" % ("x".join(map(str, s)), k) for s, k in CASES])
def test_label_table_filter_every_element(shape, kind):
    vol_h = cr.case(shape, kind)
    vol, score_h = _dev(vol_h), cr.score_of(shape)
    score = _dev(score_h)
    ws = _workspace(shape)
    for conn in cr.CONNECTIVITIES:
        for lab in (0, 2):
            want = cr.case_ref(shape, kind, conn, lab)
            n = want["result"][0]
            ids, ids_h, res = _label(vol, shape, conn, lab, ws)
            got = dict(ids=ids_h, result=res, filters={})
            cap = n + 3
            t, s = _table(vol, ids, score, shape, cap)
            assert (t[n:] == 0).all() and (s[n:] == 0).all(), "rows past the last component are zeros"
            got["table"], got["score_max"] = t[:n], s[:n]
            for ms in want["min_sizes"]:
                for kl in (0, 1):
                    got["filters"][(ms, kl)] = _filter(vol, ids, shape, ms, kl, ws)
            bad = cr.mismatches(got, want)
            if bad and "ids" in bad:
                w = np.argwhere(ids_h != want["ids"])
                bad.append((len(w), w[:4].tolist()))
            assert bad == [], (conn, lab, bad, res, want["result"])
            # the same call again: the same ids in every element
            _, again, res2 = _label(vol, shape, conn, lab, ws)
            assert np.array_equal(again, ids_h) and res2 == res, (conn, lab)
            # without a score the table is the same and score_max is not touched
            table = torch.full((cap * 9,), -5, dtype=torch.int64, device=DEV)
            check(lib().hdf_cc_table(ptr(vol), ptr(ids), None, *shape, cap, ptr(table), None, st()), "hdf_cc_table")
            assert np.array_equal(table.cpu().numpy().reshape(cap, 9), t), (conn, lab)
            # in place: out is volume
            for ms, kl in ((want["min_sizes"][2], 1), (1, 0)):
                o, r = _filter(vol, ids, shape, ms, kl, ws, in_place=True)
                assert np.array_equal(o, want["filters"][(ms, kl)][0]) and r == want["filters"][(ms, kl)][1], (conn, lab, ms, kl)
            # more components than rows: the first seven, and nothing past them
            if n > 7:
                t7, s7 = _table(vol, ids, score, shape, 7)
                assert np.array_equal(t7, want["table"][:7]), (conn, lab)
                assert np.array_equal(s7.view(np.int32), want["score_max"][:7].view(np.int32)), (conn, lab)


def test_the_checkerboard_overflows_a_table_of_seven_rows():
    shape = (19, 67, 131)
    want = cr.case_ref(shape, "checker", 6, 0)
    assert want["result"][0] == (19 * 67 * 131 + 1) // 2 > 7
    vol = _dev(cr.case(shape, "checker"))
    ids, _, res = _label(vol, shape, 6, 0, _workspace(shape))
    assert res == want["result"]
    t7, s7 = _table(vol, ids, _dev(cr.score_of(shape)), shape, 7)
    assert np.array_equal(t7, want["table"][:7]) and np.array_equal(s7.view(np.int32), want["score_max"][:7].view(np.int32))


def test_wrappers_on_three_values():
    from hdf_rt import (component_stats, component_table, connected_components, keep_largest_component, multi_dice,
                        remove_small_components)
    shape = (40, 48, 56)
    pred_h, tgt_h = cr.case(shape, "rand80"), cr.case(shape, "rand50")
    want = cr.case_ref(shape, "rand80", 26, 0)
    pred = _dev(pred_h)
    ids, count = connected_components(pred)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == shape and count.dim() == 0 and count.is_cuda
    assert np.array_equal(ids.cpu().numpy(), want["ids"]) and int(count) == want["result"][0]
    # sliding_window_predict's map -> keep_largest_component -> multi_dice, all on the device
    kept = keep_largest_component(pred)
    assert kept.is_cuda and kept.dtype == torch.uint8
    ref_map = want["filters"][(0, 1)][0]
    assert np.array_equal(kept.cpu().numpy(), ref_map)
    a, b = multi_dice(tgt_h, kept, 3), multi_dice(tgt_h, ref_map, 3)
    assert a == b and not np.isnan(a[1])
    ms = want["min_sizes"][2]
    assert np.array_equal(remove_small_components(pred_h, ms).cpu().numpy(), want["filters"][(ms, 0)][0])
    assert np.array_equal(keep_largest_component(pred_h == 2, 6).cpu().numpy(),
                          cr.full((pred_h == 2).astype(np.uint8), 6, 0)["filters"][(0, 1)][0])
    buf = pred.clone()
    assert keep_largest_component(buf, out=buf).data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), ref_map)
    # the list of dicts against the restatement's table
    w20 = cr.case_ref(shape, "rand20", 18, 2)
    score = cr.score_of(shape)
    stats = component_stats(cr.case(shape, "rand20"), 18, 2, score=score, capacity=w20["result"][0] + 5)
    assert len(stats) == w20["result"][0]
    for row, sm, got in zip(w20["table"].tolist(), w20["score_max"].tolist(), stats):
        assert got == {"size": row[0], "value": row[1], "first": row[2], "bbox": tuple(row[3:]), "score_max": sm}
    assert component_stats(cr.case(shape, "empty")) == []
    table = component_table(pred, ids, capacity=16)
    n = want["result"][0]
    assert 0 < n < 16 and np.array_equal(table.cpu().numpy()[:n], want["table"]) and not table[n:].any()
    # [H, W] is [1, H, W]
    flat = cr.case((1, 37, 70), "rand50")
    i2, c2 = connected_components(flat[0], 6)
    i3, c3 = connected_components(flat, 6)
    assert tuple(i2.shape) == (37, 70) and torch.equal(i2, i3[0]) and int(c2) == int(c3)
    assert torch.equal(keep_largest_component(flat[0], 6), keep_largest_component(flat, 6)[0])
    from hdf_rt import components, surface
    assert sum(1 for key in components._workspaces if key[-3:] == shape) == 1
    surface.clear_workspaces()
    assert not components._workspaces


def test_refused_arguments_launch_nothing_on_the_device():
    from hdf_rt import HdfError, connected_components
    shape = (4, 5, 6)
    vol = torch.ones(shape, dtype=torch.uint8, device=DEV)
    ids = torch.full((120,), -77, dtype=torch.int32, device=DEV)
    res = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = _workspace(shape)
    assert lib().hdf_cc_label(ptr(vol), 0, 8, *shape, ptr(ids), ptr(res), ptr(ws), ws.numel(), st()) == 1
    assert lib().hdf_cc_label(ptr(vol), 0, 26, *shape, ptr(ids), ptr(res), ptr(ws), ws.numel() - 1, st()) == 1
    assert lib().hdf_last_error().startswith(b"components:")
    assert lib().hdf_cc_filter(ptr(vol), ptr(ids), *shape, -1, 0, ptr(vol), ptr(res), ptr(ws), ws.numel(), st()) == 1
    assert res.cpu().tolist() == [-7, -7] and (ids.cpu() == -77).all() and (vol.cpu() == 1).all()
    with pytest.raises(HdfError):
        connected_components(torch.zeros((1, 4, 1025), dtype=torch.uint8, device=DEV))
    with pytest.raises(HdfError):
        connected_components(vol, connectivity=8)
