"""Tail fill of a variant-8 launch, the parts that need no GPU: the source rule (no block ever waits for another: the
helpers of the kernel's prologue and epilogue hold no loop, and the body calls them outside its loops), the two exports
within ABI 3, and the list-schedule model that screens K and delta (tools/tail_fill_model.py)."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import crt_amd
from crt_amd import _lib

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tools"))
import tail_fill_model as model  # noqa: E402

CSRC = REPO / "raytracer-cuda_amd" / "csrc"
NAMES = ("crt_renderer_set_tail_fill", "crt_renderer_last_tail_fill")


def _code(text):
    """C++ source without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _helpers():
    text = (CSRC / "crt_hip.hip").read_text()
    a = text.index("// ---- tail fill: the prologue and epilogue of a variant-8 block")
    b = text.index("// ---- end of the tail-fill helpers ----")
    assert a < b
    return _code(text[a:b])


def test_the_helpers_hold_no_loop_and_no_wait():
    code = _helpers()
    assert "fill_prologue(" in code and "fill_epilogue(" in code
    for word in ("for", "while", "do", "goto", "s_sleep", "__builtin_amdgcn_s_sleep", "asm"):
        assert not re.search(rf"\b{word}\b", code), word
    # one acquire read of the flag and one release write, both at agent scope; nothing calls a helper again
    assert len(re.findall(r"__hip_atomic_load\(", code)) == 1 and len(re.findall(r"__hip_atomic_store\(", code)) == 1
    assert code.count("__HIP_MEMORY_SCOPE_AGENT") == 2 and "__ATOMIC_ACQUIRE" in code and "__ATOMIC_RELEASE" in code
    assert len(re.findall(r"\bfill_prologue\(", code)) == 1 and len(re.findall(r"\bfill_epilogue\(", code)) == 1


def test_the_body_calls_them_once_outside_its_loops():
    body = _code((CSRC / "crt_render_body.inc").read_text())
    pro = [m.start() for m in re.finditer(r"\bfill_prologue\(", body)]
    epi = [m.start() for m in re.finditer(r"\bfill_epilogue\(", body)]
    loops = [m.start() for m in re.finditer(r"\b(for|while)\s*\(", body)]
    assert len(pro) == 1 and len(epi) == 1 and loops
    assert pro[0] < min(loops)                      # before the first loop of any variant
    assert epi[0] > body.index("rng_store(r, S.s);", body.rindex("traverse_step4"))   # after the block's state store
    # between the epilogue call and the end of the body only the counters' loops of the profiling builds remain
    assert "traverse_step" not in body[epi[0]:] and "next_ray" not in body[epi[0]:]
    assert re.search(r"if constexpr \(VARIANT == 8\) \{\s*if \(!fill_prologue\(", body)
    assert re.search(r"if constexpr \(TILED\) fill_epilogue\(", body)


def test_header_declares_the_exports_within_abi_3():
    text = (REPO / "include" / "crt_hip.h").read_text()
    assert re.search(r"^int crt_renderer_set_tail_fill\(crt_renderer\* r, int tiles, int spp\);", text, re.M)
    assert re.search(r"^int crt_renderer_last_tail_fill\(crt_renderer\* r, int out\[4\]\);", text, re.M)
    assert re.search(r"^#define CRT_ABI_VERSION 3\b", text, re.M)
    for name in NAMES:
        doc = text[:text.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "Results never depend on it" in " ".join(doc.split()), name
        assert name in _lib.HIP_SYMBOLS and name in _lib.OPTIONAL_SYMBOLS
        assert name in (REPO / "INTEGRATION.md").read_text()


def test_the_built_library_exports_them_and_rejects_a_null_handle():
    L = _lib.hip()
    assert L.crt_abi_version() == 3
    assert L.crt_renderer_set_tail_fill(None, 1, 1) != 0
    assert L.crt_renderer_last_tail_fill(None, None) != 0


class _OlderLibrary:
    """A library of the same ABI version from before the exports: everything but them."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in NAMES:
            raise AttributeError(name)
        return getattr(self._real, name)


def test_an_older_library_still_loads_and_the_front_ends_name_the_missing_entry(monkeypatch):
    real = _lib.hip()
    monkeypatch.setattr(_lib, "_hip", None)
    monkeypatch.setattr(_lib.C, "CDLL", lambda *a, **k: _OlderLibrary(real))
    old = _lib.hip()
    assert isinstance(old, _OlderLibrary) and not hasattr(old, NAMES[0])
    renderer = crt_amd.Renderer._borrow(None, 8, 4, 0, None)
    with pytest.raises(crt_amd.CrtError, match=NAMES[0]):
        renderer.set_tail_fill(1, 1)
    with pytest.raises(crt_amd.CrtError, match=NAMES[1]):
        renderer.last_tail_fill()


# ---- the list-schedule model ----
def test_model_without_fill_is_the_plain_list_schedule():
    d = model.synthetic_durations(5760, seed=3)
    base, ends = model.list_schedule(d, 716)
    assert base == pytest.approx(float(ends.max()))
    assert base >= d.sum() / 716 and base >= d.max()
    for k, frac in ((0, 0.125), (2880, 0.0)):
        m = model.tail_fill_schedule(d, 716, k, frac)
        assert m["span"] == pytest.approx(base) and m["swept"] == 0


def test_model_part_with_an_unfinished_head_goes_to_the_sweep():
    # 4 tiles on 8 slots: every tail part is dispatched at t = 0, while its head runs: all four are swept, after the
    # main launch's 7.5: span 7.5 + 2.5
    m = model.tail_fill_schedule([10.0] * 4, 8, 4, 0.25)
    assert (m["swept"], m["in_launch"]) == (4, 0)
    assert m["main_span"] == pytest.approx(7.5, abs=0.01) and m["span"] == pytest.approx(10.0, abs=0.01)
    # 4 tiles on 2 slots, the first two split in halves: heads 0-2, 0-2, tiles 2-6, 2-6, parts 6-8, 6-8 in the launch
    m = model.tail_fill_schedule([4.0] * 4, 2, 2, 0.5)
    assert (m["swept"], m["in_launch"]) == (0, 2) and m["span"] == pytest.approx(8.0)
    # a surcharge lengthens only the parts
    m = model.tail_fill_schedule([4.0] * 4, 2, 2, 0.5, surcharge=0.5)
    assert m["span"] == pytest.approx(9.0)


def test_model_fill_shortens_the_drain_of_a_long_launch():
    """8 items per slot, shaped like config C's launch at a tenth of its size: the plain launch ends with a drain; with
    1/8 of the samples of the first half of the order held back no part finds its head unfinished, and the span lies
    between the work bound and the plain span."""
    d = model.synthetic_durations(5760, seed=1)
    slots = 716
    base = model.list_schedule(d, slots)[0]
    bound = d.sum() / slots
    assert base > 1.04 * bound                       # the drain the fill is for
    m = model.tail_fill_schedule(d, slots, len(d) // 2, 1 / 8)
    assert m["swept"] == 0 and m["in_launch"] == len(d) // 2
    assert bound <= m["span"] < base
    assert m["span"] < base - 0.25 * (base - bound)   # at least a quarter of the drain is recovered
    rows = model.screen(d, slots)
    assert len(rows) == 13 and rows[0]["change"] == 0.0
    assert all(np.isfinite(r["span"]) and r["span"] >= bound - 1e-6 for r in rows)
