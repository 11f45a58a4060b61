"""Video scope taps without a device: the numpy model of the record on pictures with closed-form answers, the header's text, and
mx_video_scope_record_bytes (host only) through ctypes."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import video_scope_model as vm

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mixlab_gpu.h").read_text()


@pytest.mark.parametrize("w,h", [(64, 36), (1000, 562), (1920, 1080)])
def test_blank_frame_lands_on_one_counter_per_scope(w, h):
    c = vm.counts(*vm.blank(w, h), 256, True)
    n_c = (w >> 1) * (h >> 1)
    assert c["hist"][0][0] == w * h and c["hist"][0].sum() == w * h
    assert c["hist"][1][128] == c["hist"][2][128] == c["vec"][64][64] == n_c
    assert c["hist"][1].sum() == c["hist"][2].sum() == c["vec"].sum() == n_c
    assert c["wave"][:, 1:].sum() == 0 and c["wave"].sum() == w * h


@pytest.mark.parametrize("w", [1000, 1918])
@pytest.mark.parametrize("cols", [64, 128, 256])
def test_ramp_bucket_populations_follow_the_floor_rule(w, cols):
    h = 6
    y, u, v = vm.ramp(w, h)
    c = vm.counts(y, u, v, cols, True)
    # bucket c holds the columns x with c * W <= x * C < (c + 1) * W: ceil((c + 1) W / C) - ceil(c W / C) of them, every row
    edges = [-(-(k * w) // cols) for k in range(cols + 1)]
    assert edges[0] == 0 and edges[-1] == w
    assert w % cols != 0 and len({b - a for a, b in zip(edges, edges[1:])}) > 1     # uneven buckets: the rule is exercised
    assert [int(r.sum()) for r in c["wave"]] == [h * (b - a) for a, b in zip(edges, edges[1:])]
    for k in (0, 1, cols // 2, cols - 1):                                           # and each bucket holds exactly its columns' values
        want = np.bincount(y[:, edges[k]:edges[k + 1]].ravel(), minlength=256)
        assert np.array_equal(c["wave"][k], want)
    assert c["hist"][0].sum() == c["wave"].sum() == w * h
    assert np.array_equal(c["wave"].sum(axis=0), c["hist"][0])
    assert c["vec"].sum() == c["hist"][1].sum() == (w >> 1) * (h >> 1)
    # V = 255 - U, so (V >> 1) + (U >> 1) = 127: the vectorscope is the anti-diagonal
    vv, uu = np.nonzero(c["vec"])
    assert len(vv) > 1 and np.all(vv + uu == 127)


def test_invariants_on_noise_and_record_shapes():
    rng = np.random.default_rng(5)
    w, h = 130, 70
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h >> 1, w >> 1), dtype=np.uint8)
    v = rng.integers(0, 256, (h >> 1, w >> 1), dtype=np.uint8)
    for cols in vm.WAVE_COLS:
        for vec in (False, True):
            c = vm.counts(y, u, v, cols, vec)
            assert c["hist"].dtype == np.uint32 and c["hist"][0].sum() == w * h
            assert (c["wave"] is None) == (cols == 0) and (c["vec"] is None) == (not vec)
            if cols:
                assert c["wave"].shape == (cols, 256) and c["wave"].sum() == w * h
            if vec:
                assert c["vec"].sum() == c["hist"][1].sum()
                assert c["vec"][int(v[3, 5]) >> 1][int(u[3, 5]) >> 1] >= 1
    r = vm.record(None, 7, 64, True)
    assert (r["present"], r["counted"], r["tick_in_run"]) == (0, 0, 7) and not r["hist"].any() and not r["wave"].any() and not r["vec"].any()
    r = vm.record((4, 16, 8, None), 0, 0, False)          # packed RGB: present, not counted
    assert (r["present"], r["counted"], r["pixfmt"], r["width"], r["height"]) == (1, 0, 4, 16, 8) and not r["hist"].any()
    # legal-range violations are sums over hist (no fields of their own)
    c = vm.counts(*vm.blank(16, 8), 0, False)
    assert c["hist"][0][:16].sum() == 16 * 8 and c["hist"][0][236:].sum() == 0


def test_header_declares_the_scope_calls_and_keeps_the_abi_constants():
    for decl in (r"int\s+mx_graph_set_video_scopes\s*\(\s*mx_graph\s*\*\s*g\s*,\s*const\s+mx_port_ref\s*\*\s*ports\s*,\s*size_t\s+n\s*,\s*const\s+mx_video_scope_params\s*\*",
                 r"int\s+mx_graph_read_video_scopes\s*\(\s*mx_graph\s*\*\s*g\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+cap_bytes\s*,\s*uint32_t\s*\*\s*n_records\s*\)",
                 r"int\s+mx_video_scope_record_bytes\s*\(\s*const\s+mx_video_scope_params\s*\*\s*\w+\s*,\s*size_t\s*\*\s*bytes\s*\)",
                 r"int\s+mx_video_scope\s*\(\s*const\s+mx_dframe\s*\*\s*in\s*,\s*const\s+mx_video_scope_params\s*\*\s*\w+\s*,\s*void\s*\*\s*device_record\s*,\s*void\s*\*\s*stream\s*\)"):
        assert re.search(decl, HEADER), decl
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+wave_cols[^}]*vectorscope[^}]*hop[^}]*\}\s*mx_video_scope_params\s*;", HEADER)
    assert re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER)
    assert re.search(r"#define\s+MX_ABI_VERSION\s+4u\b", HEADER)
    assert "no fields" in HEADER.lower() or "NO fields" in HEADER       # min / max / mean / legal range: sums over hist, said so


def test_record_bytes_through_the_library_for_every_parameter_combination():
    from mixlab_amd import abi
    assert abi.lib.mx_abi_version() == 4
    for cols in vm.WAVE_COLS:
        for vec in (0, 1):
            n = C.c_size_t()
            p = abi.VideoScopeParams(cols, vec, 1)
            assert abi.lib.mx_video_scope_record_bytes(C.byref(p), C.byref(n)) == abi.MX_OK
            assert n.value == 32 + 4 * (768 + 256 * cols + 16384 * vec) == vm.record_bytes(cols, bool(vec))
            assert abi.video_scope_record_bytes(cols, bool(vec)) == n.value
    assert vm.record_bytes(256, True) == 330784
    n = C.c_size_t()
    p = abi.VideoScopeParams(256, 7, 0)                      # any non-zero vectorscope is on; hop is not looked at
    assert abi.lib.mx_video_scope_record_bytes(C.byref(p), C.byref(n)) == abi.MX_OK and n.value == 330784
    for bad in (1, 32, 63, 65, 192, 512, 0xffffffff):
        p = abi.VideoScopeParams(bad, 0, 1)
        assert abi.lib.mx_video_scope_record_bytes(C.byref(p), C.byref(n)) == abi.MX_ERR_INVALID
        assert b"wave_cols" in abi.lib.mx_last_error()
    assert abi.lib.mx_video_scope_record_bytes(None, C.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope_record_bytes(C.byref(abi.VideoScopeParams(0, 0, 1)), None) == abi.MX_ERR_INVALID
