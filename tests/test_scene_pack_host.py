"""CPU tier of the scene pack (GS_FRAME_SCENE_PACK, include/gs_abi.h): the size query, the validation of a flagged frame, which
frame descriptions would read a pack, and the ctypes mirror of the descriptor's trailing fields.  No kernel is launched here:
every call below is refused or answered on the host before anything is enqueued."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from gs_testutil import FAKE, fake_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GS_E_INVALID = -1

_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "gs_abi.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(gs_frame), sizeof(gs_frame_scene), offsetof(gs_frame_scene, frame),
           offsetof(gs_frame_scene, scene_pack_a), offsetof(gs_frame_scene, scene_pack_b),
           offsetof(gs_frame_scene, scene_pack_a_bytes), offsetof(gs_frame_scene, scene_pack_b_bytes));
    return 0;
}
"""


def _packed_frame(**kw):
    from gaussian import _lib

    kw = dict(dict(training=0, N=140_000, W=320, H=240), **kw)
    base = fake_frame(**kw)
    f = _lib.GsFrameScene()  # a gs_frame followed by the four pack fields
    C.memmove(C.byref(f), C.byref(base), C.sizeof(_lib.GsFrame))
    a, b = C.c_size_t(), C.c_size_t()
    _lib.gs_scene_pack_bytes(f.N, C.byref(a), C.byref(b))
    f.flags |= _lib.GS_FRAME_SCENE_PACK
    f.scene_pack_a, f.scene_pack_b = FAKE + (10 << 30), FAKE + (11 << 30)
    f.scene_pack_a_bytes, f.scene_pack_b_bytes = a.value, b.value
    return f


def test_flag_value_and_descriptor_mirror():
    from gaussian import _lib

    assert _lib.GS_FRAME_SCENE_PACK == 8192
    assert _lib.GS_FRAME_SCENE_PACK & (_lib.GS_FRAME_POSE_GRAD | _lib.GS_FRAME_AUX | _lib.GS_FRAME_CULL_DILATE_NEAR) == 0
    assert _lib.gs_abi_version() == 8
    # the four fields follow an UNCHANGED gs_frame (gs_frame_scene): the earlier layout and its size are untouched
    S, G = _lib.GsFrameScene, _lib.GsFrame
    assert issubclass(S, G) and [n for n, _ in G._fields_][-1] == "pose_workspace_bytes"
    assert [n for n, _ in S._fields_] == ["scene_pack_a", "scene_pack_b", "scene_pack_a_bytes", "scene_pack_b_bytes"]
    assert S.scene_pack_a.offset == C.sizeof(G) == G.pose_workspace_bytes.offset + C.sizeof(C.c_size_t)
    assert C.sizeof(S) == C.sizeof(G) + 2 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_size_t)
    for name in ("gs_scene_pack_bytes", "gs_scene_pack_build", "gs_frame_reads_scene_pack"):
        assert name in _lib.EXPORTS


def test_ctypes_mirror_matches_the_header(tmp_path):
    from gaussian import _lib

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler on PATH")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(_LAYOUT_C)
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.GsFrameScene
    assert got == [C.sizeof(_lib.GsFrame), C.sizeof(S), 0, S.scene_pack_a.offset, S.scene_pack_b.offset,
                   S.scene_pack_a_bytes.offset, S.scene_pack_b_bytes.offset]


def test_scene_pack_size_query():
    from gaussian import _lib

    def q(n):
        a, b = C.c_size_t(123), C.c_size_t(456)
        total = _lib.gs_scene_pack_bytes(n, C.byref(a), C.byref(b))
        assert total == a.value + b.value
        return total, a.value, b.value

    ns = (0, 1, 3, 15, 16, 17, 255, 256, 257, 5000, 140_000, 376_467, 2_400_000, (1 << 31) - 1)
    sizes = [q(n) for n in ns]
    assert [s[0] for s in sizes] == sorted(s[0] for s in sizes)  # monotone in N
    for n, (_, a, b) in zip(ns, sizes):  # 16 N and 64 N, each rounded up to whole 256-byte units
        assert a == (16 * n + 255) // 256 * 256 and b == (64 * n + 255) // 256 * 256
    assert q(2_400_000)[0] == 80 * 2_400_000  # 192 MB at 2.4 M
    assert q(-1) == (0, 0, 0) and q(-(1 << 40)) == (0, 0, 0)
    assert _lib.gs_scene_pack_bytes(1000, None, None) == 16128 + 64000  # either out pointer may be NULL


def test_flagged_frame_validation_is_host_only():
    from gaussian import _lib

    fwd = _lib.gs_frame_forward
    assert _lib.gs_frame_binning_variant(C.byref(_packed_frame())) == 4  # a valid description, strip variant

    def refused(f, *needles):
        assert fwd(C.byref(f), None) == GS_E_INVALID
        err = _lib.gs_last_error()
        assert b"GS_FRAME_SCENE_PACK" in err and all(n in err for n in needles), err

    f = _packed_frame()
    f.scene_pack_a = None
    refused(f, b"scene_pack_a")
    f = _packed_frame()
    f.scene_pack_b = None
    refused(f, b"scene_pack_b")
    f = _packed_frame()
    f.scene_pack_a_bytes -= 256
    refused(f, b"scene_pack_a_bytes")
    f = _packed_frame()
    f.scene_pack_b_bytes -= 256
    refused(f, b"scene_pack_b_bytes")
    f = _packed_frame()
    f.scene_pack_a += 8  # not 16-byte aligned
    refused(f, b"scene_pack_a", b"16-byte")
    f = _packed_frame()
    f.scene_pack_b += 16  # 16-byte aligned, which plane A may be, but not a 64-byte line
    refused(f, b"scene_pack_b", b"64-byte")
    f = _packed_frame(training=1)
    refused(f, b"training")
    # the other entry points validate the same way
    f = _packed_frame()
    f.scene_pack_b = None
    assert _lib.gs_frame_binning_variant(C.byref(f)) == GS_E_INVALID
    # where the pack does not apply the flag is still validated, and a well-formed flagged frame is accepted (and ignored)
    assert _lib.gs_frame_binning_variant(C.byref(_packed_frame(N=10_000, W=256, H=256))) == 2
    # without the flag the four fields are not read at all: garbage behind the descriptor, or a plain gs_frame, validates
    f = _packed_frame()
    f.flags &= ~_lib.GS_FRAME_SCENE_PACK
    f.scene_pack_a, f.scene_pack_b, f.scene_pack_a_bytes, f.scene_pack_b_bytes = 8, 16, 0, 0
    assert _lib.gs_frame_binning_variant(C.byref(f)) == 4
    assert _lib.gs_frame_binning_variant(C.byref(fake_frame(training=0, N=140_000, W=320, H=240))) == 4


def test_which_frames_read_a_pack():
    from gaussian import _lib

    reads = _lib.gs_frame_reads_scene_pack
    assert reads(C.byref(fake_frame(training=0, N=140_000, W=320, H=240))) == 1  # (asked of the description, flagged or not)
    assert reads(C.byref(_packed_frame())) == 1
    assert reads(C.byref(fake_frame(training=0, N=10_000, W=256, H=256))) == 0  # table variant
    assert reads(C.byref(fake_frame(training=1, N=140_000, W=320, H=240))) == 0  # training frame
    assert reads(C.byref(fake_frame(training=0, N=0, W=320, H=240))) == 0
    f = fake_frame(training=0, N=140_000, W=320, H=240)
    f.flags |= _lib.GS_FRAME_TABLE_BIN
    assert reads(C.byref(f)) == 0
    f = fake_frame(training=0, N=10_000, W=256, H=256)
    f.flags |= _lib.GS_FRAME_STRIP_BIN  # the strip variant whatever the size
    assert reads(C.byref(f)) == 1
    for mode in (0, 1):
        f = fake_frame(training=0, N=140_000, W=320, H=240)
        f.sort_mode = mode
        assert reads(C.byref(f)) == 0
    assert reads(None) == 0
