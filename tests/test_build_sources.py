"""The source list of the library build (tacex_amd/_build.py) against the tree: every listed translation unit exists, every csrc/*.hip is
listed, and a listed file that is missing stops the build instead of linking a library without it."""
import pytest
from conftest import REPO


def test_sources_match_the_tree():
    from tacex_amd import _build

    on_disk = sorted(p.name for p in (REPO / "tacex_amd" / "csrc").glob("*.hip"))
    assert sorted(_build.SOURCES) == on_disk
    assert len(set(_build.SOURCES)) == len(_build.SOURCES)
    assert set(_build.FILE_FLAGS) <= set(_build.SOURCES)


def test_missing_source_is_an_error(monkeypatch, tmp_path):
    from tacex_amd import _build

    monkeypatch.setattr(_build, "SOURCES", list(_build.SOURCES) + ["no_such_unit.hip"])
    monkeypatch.setattr(_build, "PKG", tmp_path)  # (the check comes before anything is compiled or written; were it not, not into the tree)
    with pytest.raises(RuntimeError, match="no_such_unit.hip"):
        _build._build_locked("digest", False)
