"""build.py's unit list against csrc/: a unit left out of SOURCES compiles nowhere and shows up only as an undefined symbol
when the library is loaded; a stale entry or a stale per-file flag set fails the build or silently applies to nothing."""
import importlib.util
import os

from conftest import ROOT

PKG = os.path.join(ROOT, "h-denseformer_amd")


def _build_module():
    spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_unit_is_built_exactly_once():
    b = _build_module()
    on_disk = sorted(f for f in os.listdir(os.path.join(PKG, "csrc")) if f.endswith(".hip"))
    assert on_disk, "no units found"
    for f in on_disk:
        assert b.SOURCES.count(f) == 1, f"csrc/{f} appears {b.SOURCES.count(f)} times in build.SOURCES"


def test_every_source_entry_exists():
    b = _build_module()
    for f in b.SOURCES:
        assert os.path.isfile(os.path.join(PKG, "csrc", f)), f"build.SOURCES names csrc/{f}, which does not exist"


def test_every_extra_flag_set_belongs_to_a_source():
    b = _build_module()
    for f in b.EXTRA:
        assert f in b.SOURCES, f"build.EXTRA has flags for {f}, which is not in build.SOURCES"
