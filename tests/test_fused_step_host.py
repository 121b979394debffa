"""CPU tier of the fused backward + Adam step (include/gs_abi.h: gs_frame_backward_adam, gs_frame_backward_adam_aux,
gs_frame_backward_adam_pose): what each of the three entry points answers, and with which sentence, for every combination of
the frame's flags, colour model and training state with a good, an all-zero and a missing optimizer descriptor and a missing
image.  A caller sees only the first refusal, so the table below pins the ORDER of the checks (gs_frame.hip:
frame_backward_adam_impl behind each entry point's own flag preconditions); its values are what the three separate
implementations this path replaced answered.  Everything happens on fake pointers: no kernel is launched."""
import ctypes as C

import pytest

from gs_testutil import FAKE, fake_adam, fake_frame

PLAIN, AUX, POSE = "gs_frame_backward_adam", "gs_frame_backward_adam_aux", "gs_frame_backward_adam_pose"
GS_E_INVALID, GS_E_UNSUPPORTED = -1, -2
GIMG = FAKE + (10 << 30)

# outcome -> (return code, how gs_last_error() begins; {0} = the entry point)
OUTCOMES = {
    "ok": (0, None),  # accepted; called with N = 0: returns before anything is enqueued
    "skip": None,  # accepted pose frame, not called: even N = 0 enqueues the twelve zeros of its pose gradient
    "no_aux": (GS_E_UNSUPPORTED, "{0}: GS_FRAME_AUX frames are not supported (use gs_frame_backward + an optimizer step)"),
    "no_pose": (GS_E_UNSUPPORTED, "{0}: GS_FRAME_POSE_GRAD frames are not supported (use gs_frame_backward + an optimizer step)"),
    "want_aux": (GS_E_INVALID, "{0}: invalid argument: the frame is not flagged GS_FRAME_AUX"),
    "want_pose": (GS_E_INVALID, "{0}: invalid argument: the frame is not flagged GS_FRAME_POSE_GRAD"),
    "sh_pose": (GS_E_UNSUPPORTED, "{0}: GS_FRAME_POSE_GRAD needs rgb colours (color_dim 3): with SH colours the image also "
                                  "depends on the pose through the pixels' ray directions"),
    "train": (GS_E_INVALID, "{0}: invalid argument: {0} needs a training forward (image_padded kept)"),
    "null": (GS_E_INVALID, "{0}: invalid argument: null pointer"),
    "step": (GS_E_INVALID, "gs_validate_adam_fused: invalid argument: step counts from 1"),
}
ARGS = ("good", "zero", "null_adam", "null_image")  # the columns: descriptor good / all-zero / NULL, and a NULL grad_image
# (entry point, GS_FRAME_AUX, GS_FRAME_POSE_GRAD, color_dim, training): the outcome per column
EXPECTED = {
    (PLAIN, 0, 0,  3, 1): ('ok', 'step', 'null', 'null'),
    (PLAIN, 0, 0,  3, 0): ('train', 'train', 'train', 'train'),
    (PLAIN, 0, 0, 27, 1): ('ok', 'step', 'null', 'null'),
    (PLAIN, 0, 0, 27, 0): ('train', 'train', 'train', 'train'),
    (PLAIN, 0, 1,  3, 1): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (PLAIN, 0, 1,  3, 0): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (PLAIN, 0, 1, 27, 1): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (PLAIN, 0, 1, 27, 0): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (PLAIN, 1, 0,  3, 1): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 0,  3, 0): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 0, 27, 1): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 0, 27, 0): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 1,  3, 1): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),  # both flags: GS_FRAME_AUX is named
    (PLAIN, 1, 1,  3, 0): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 1, 27, 1): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (PLAIN, 1, 1, 27, 0): ('no_aux', 'no_aux', 'no_aux', 'no_aux'),
    (AUX,   0, 0,  3, 1): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 0,  3, 0): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 0, 27, 1): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 0, 27, 0): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 1,  3, 1): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 1,  3, 0): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 1, 27, 1): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   0, 1, 27, 0): ('want_aux', 'want_aux', 'want_aux', 'want_aux'),
    (AUX,   1, 0,  3, 1): ('ok', 'step', 'null', 'ok'),  # a NULL image is the zero image
    (AUX,   1, 0,  3, 0): ('train', 'train', 'train', 'train'),
    (AUX,   1, 0, 27, 1): ('ok', 'step', 'null', 'ok'),
    (AUX,   1, 0, 27, 0): ('train', 'train', 'train', 'train'),
    (AUX,   1, 1,  3, 1): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (AUX,   1, 1,  3, 0): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),  # ... even for a frame that is not training
    (AUX,   1, 1, 27, 1): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),  # ... or has SH colours
    (AUX,   1, 1, 27, 0): ('no_pose', 'no_pose', 'no_pose', 'no_pose'),
    (POSE,  0, 0,  3, 1): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  0, 0,  3, 0): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  0, 0, 27, 1): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  0, 0, 27, 0): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  0, 1,  3, 1): ('skip', 'step', 'null', 'null'),
    (POSE,  0, 1,  3, 0): ('train', 'train', 'train', 'train'),
    (POSE,  0, 1, 27, 1): ('sh_pose', 'sh_pose', 'sh_pose', 'sh_pose'),
    (POSE,  0, 1, 27, 0): ('sh_pose', 'sh_pose', 'sh_pose', 'sh_pose'),  # the colour model comes before the training check
    (POSE,  1, 0,  3, 1): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  1, 0,  3, 0): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  1, 0, 27, 1): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  1, 0, 27, 0): ('want_pose', 'want_pose', 'want_pose', 'want_pose'),
    (POSE,  1, 1,  3, 1): ('skip', 'step', 'null', 'skip'),
    (POSE,  1, 1,  3, 0): ('train', 'train', 'train', 'train'),
    (POSE,  1, 1, 27, 1): ('sh_pose', 'sh_pose', 'sh_pose', 'sh_pose'),
    (POSE,  1, 1, 27, 0): ('sh_pose', 'sh_pose', 'sh_pose', 'sh_pose'),
}


def test_the_table_is_the_whole_matrix():
    assert set(EXPECTED) == {(s, a, p, cd, tr) for s in (PLAIN, AUX, POSE) for a in (0, 1) for p in (0, 1) for cd in (3, 27)
                             for tr in (1, 0)}
    assert all(len(row) == len(ARGS) and set(row) <= set(OUTCOMES) for row in EXPECTED.values())
    # only frames that would launch are answered with 0 or left out, and only pose frames are left out
    for (sym, aux, pose, cd, tr), row in EXPECTED.items():
        for outcome in row:
            if outcome in ("ok", "skip"):
                assert tr and (aux, pose) == {PLAIN: (0, 0), AUX: (1, 0), POSE: (aux, 1)}[sym]
                assert (outcome == "skip") == bool(pose)


@pytest.mark.parametrize("sym", [PLAIN, AUX, POSE])
def test_refusal_matrix(sym):
    from gaussian import _lib

    call = getattr(_lib, sym)
    for (s, aux, pose, cd, tr), row in EXPECTED.items():
        for arg, outcome in zip(ARGS, row):
            if s != sym or OUTCOMES[outcome] is None:
                continue
            want_rc, want_msg = OUTCOMES[outcome]
            f = fake_frame(pose=bool(pose), aux=bool(aux), color_dim=cd, training=tr, N=0 if outcome == "ok" else 1000)
            adam = {"good": fake_adam(), "zero": fake_adam(good=False), "null_adam": None, "null_image": fake_adam()}[arg]
            rc = call(C.byref(f), None if arg == "null_image" else GIMG, C.byref(adam) if adam is not None else None, None)
            cell = (sym, aux, pose, cd, tr, arg)
            assert rc == want_rc, (cell, rc, _lib.gs_last_error())
            if want_msg is not None:
                assert _lib.gs_last_error().decode().startswith(want_msg.format(sym)), (cell, _lib.gs_last_error())
