"""crt_renderer_last_launch_frozen, the export that says which twin of a plain variant-8 kernel ran (no GPU): the
header declares it within ABI 3, the bindings list it as optional, and a library from before it still loads, with
Renderer.last_launch_frozen() naming the missing entry."""
import re
from pathlib import Path

import pytest

import crt_amd
from crt_amd import _lib

REPO = Path(__file__).resolve().parents[1]
NAME = "crt_renderer_last_launch_frozen"


def test_header_declares_the_export_within_abi_3():
    text = (REPO / "include" / "crt_hip.h").read_text()
    assert re.search(r"^int crt_renderer_last_launch_frozen\(const crt_renderer\* r\);", text, re.M)
    assert re.search(r"^#define CRT_ABI_VERSION 3\b", text, re.M)
    assert _lib.ABI_VERSION == 3
    assert NAME in _lib.HIP_SYMBOLS and NAME in _lib.OPTIONAL_SYMBOLS
    assert NAME in (REPO / "INTEGRATION.md").read_text()


def test_the_built_library_exports_it_and_answers_a_null_handle():
    L = _lib.hip()
    assert L.crt_abi_version() == 3
    assert L.crt_renderer_last_launch_frozen(None) == 0


class _OlderLibrary:
    """A library of the same ABI version from before the export: everything but it."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name == NAME:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_an_older_library_loads_and_the_front_end_names_what_is_missing(monkeypatch):
    real = _lib.hip()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda *a, **k: _OlderLibrary(real))
    old = _lib.hip()                                   # the binding loop passes over the entry it does not find
    assert isinstance(old, _OlderLibrary) and old.crt_abi_version() == 3
    assert not hasattr(old, NAME) and hasattr(old, "crt_renderer_last_kernel_name")
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    assert renderer.last_kernel_name() == ""           # the older entries still answer
    with pytest.raises(crt_amd.CrtError, match=NAME):
        renderer.last_launch_frozen()
    monkeypatch.setattr(_lib, "_hip", real)
    assert renderer.last_launch_frozen() == 0
