"""The workspace sizes of the entries on a [D][H][W] volume, held to literals: the figures below were recorded from the
library as it stood BEFORE the carve structs were rebuilt on one Carver (csrc/volume_host.h), not from the code under
test.  A caller sizes its allocation by these calls and the launchers carve the same bytes: a part that moved, grew or
lost its 256-byte rounding shows here first.  No device is needed."""
import ctypes as C
import os

import pytest

from conftest import ROOT

FNS = ("hdf_surface_workspace_bytes", "hdf_surface_asd_workspace_bytes", "hdf_surface_mm_workspace_bytes",
       "hdf_cc_workspace_bytes", "hdf_morph_workspace_bytes", "hdf_fill_holes_workspace_bytes")
PREFIX = (b"surface:", b"surface:", b"surface:", b"components:", b"morphology:", b"morphology:")
# shape -> bytes, in the order of FNS
RECORDED = {
    (1, 1, 1):          (1280, 1792, 50688, 3072, 512, 4096),
    (1, 5, 7):          (1280, 1792, 51200, 3072, 512, 4096),
    (3, 17, 33):        (21248, 26880, 78848, 11264, 1024, 22016),
    (8, 9, 10):         (8192, 9472, 62464, 6400, 1024, 11264),
    (64, 64, 64):       (2407424, 2455552, 4507136, 1315072, 65536, 2888448),
    (448, 512, 512):    (1059853312, 1062744832, 1996603904, 588122368, 29360128, 1292765952),
    (1024, 1024, 1024): (9676235264, 9688806144, 18253726208, 5377100032, 268435456, 11819551488),
}
# capacity -> bytes of hdf_cc_pairs_workspace_bytes; 2^20 is past the cap of 65536
RECORDED_PAIRS = {1: 1792, 33: 3328, 4096: 196864, 2 ** 20: -1}
RECORDED_SELECT_U64_WS = 49408
# the bad dimensions the entries' own tests refuse (test_surface_ref_cpu, test_asd_ref_cpu, test_surface_mm_ref_cpu,
# test_cc_ref_cpu, test_morph_ref_cpu)
BAD_DIMS = [(0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (-3, 8, 8), (2048, 1024, 1024),
            (1024, 1024, 2048), (65536, 65536, 1), (1025, 1, 1), (0, 4, 4), (4, 1025, 4), (4, 4, -1)]


@pytest.fixture(scope="module")
def lib():
    from hdf_rt import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(ROOT, "h-denseformer_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("shape", sorted(RECORDED))
def test_volume_workspace_sizes_are_the_recorded_ones(lib, shape):
    got = tuple(getattr(lib, fn)(*shape) for fn in FNS)
    assert got == RECORDED[shape], dict(zip(FNS, zip(got, RECORDED[shape])))
    assert all(n % 256 == 0 for n in got)


def test_pair_table_workspace_sizes_are_the_recorded_ones(lib):
    for capacity, want in RECORDED_PAIRS.items():
        assert lib.hdf_cc_pairs_workspace_bytes(capacity) == want, capacity
        if want < 0:
            assert lib.hdf_last_error().startswith(b"components:")


def test_select_workspace_is_the_recorded_one(lib):
    with open(os.path.join(ROOT, "include", "hdf.h")) as fh:
        assert "#define HDF_SELECT_U64_WS %d " % RECORDED_SELECT_U64_WS in fh.read()
    # the entry asks for exactly that: one byte less is refused on the host (the addresses are never dereferenced)
    buf = (C.c_uint64 * 4)()
    a = C.addressof(buf)
    assert lib.hdf_op_select_u64(a, 8, 0, a, RECORDED_SELECT_U64_WS - 1, a, None) == 1
    assert lib.hdf_last_error() == b"surface: select_u64: workspace of %d bytes, %d needed" % (
        RECORDED_SELECT_U64_WS - 1, RECORDED_SELECT_U64_WS)
    # never above the workspace of the entries that carve it
    assert all(sizes[2] >= RECORDED_SELECT_U64_WS for sizes in RECORDED.values())


@pytest.mark.parametrize("fn,prefix", list(zip(FNS, PREFIX)))
def test_bad_dimensions_return_minus_one_with_the_family_prefix(lib, fn, prefix):
    for dims in BAD_DIMS:
        assert getattr(lib, fn)(*dims) == -1, (fn, dims)
        assert lib.hdf_last_error().startswith(prefix + b" "), (fn, dims, lib.hdf_last_error())
